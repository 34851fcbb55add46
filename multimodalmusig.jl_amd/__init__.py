"""multimodalmusig.jl_amd -- MI355X (gfx950) backend for the variational-EM hot path of MultiModalMuSig.jl.

Exports mirror the reference module (src/MultiModalMuSig.jl:9): IMMCTM, MMCTM, LDA, fit (`fit!`),
format_counts_lda / _ctm / _mmctm.  ILDA rides on the LDA kernels with feature-folded topic tables.
"""
from . import _lib
from ._lib import Context, MmmError, build, comm_unique_id, default_context, lib
from .models import (ILDA, LDA, calculate_elbo, calculate_loglikelihood, fit, fit_bang, update_Elnβ, update_Elnθ, update_β, update_γ, update_θ,
                     update_λ, update_ϕ)
from .ctm import (calculate_docmodality_loglikelihood, calculate_modality_loglikelihood, calculate_Ndivζ, calculate_sumθ, α_objective, λ_objective, ν_objective,
                  IMMCTM, MMCTM, calculate_loglikelihoods, fit_restarts, fitdoc, pick_optimal_modality_models, update_Elnϕ, update_props, update_α, update_Σ, update_ζ, update_μ,
                  update_ν)
from .inference import fit_heldout, predict_modality_η, transform
from .restarts import fit_lda_restarts
from .bootstrap import BootstrapResult, bootstrap_exposures, replicate_summary, resample_counts
from .match import (ConsensusResult, SignatureMatch, cosine_similarity, match_restarts, match_signatures, restart_consensus,
                    signature_consensus)
from .select import (KPick, KSelection, MMSelection, ScoreResult, holdout, pick_k, score_exposures, score_restarts, select_num_signatures,
                     select_num_signatures_mmctm, split_counts)
from .refit import RefitIntervals, RefitResult, refit_exposures
from .simulate import FitCheck, goodness_of_fit, simulate_counts
from .presence import PresenceResult, signature_presence
from .power import PowerResult, presence_power
from .attribute import AttributionResult, attribute_mutations, mutation_table
from .compare import ComparisonResult, compare_exposures, deal_counts
from .trajectory import TrajectoryResult, bin_by_order, exposure_trajectory
from .decompose import Decomposition, SearchResult, decompose_search, decompose_signatures
from .extract import Extraction, extract_signatures
from .cluster import SampleClusters, cluster_samples
from .associate import ExposureAssociations, associate_exposures
from .regress import ExposureRegressions, regress_exposures
from .survival import GroupTest, KMCurve, SurvivalAssociations, kaplan_meier, survival_association, survival_scores
from .classify import ExposureClassifier, classify_exposures
from .cox import ExposureCoxModel, cox_exposures
from .io import read_signatures_tsv
from .utils import (PackedCorpus, format_counts_ctm, format_counts_lda, format_counts_mmctm, make_count_matrix, pack_lda,
                    pack_mm, read_counts_tsv, shard_documents)

__all__ = ["ILDA", "IMMCTM", "MMCTM", "LDA", "fit", "fit_bang", "format_counts_lda", "format_counts_ctm", "format_counts_mmctm", "Context",
           "MmmError", "build", "fit_restarts", "fit_lda_restarts", "transform", "fit_heldout", "predict_modality_η",
           "bootstrap_exposures", "resample_counts", "replicate_summary", "BootstrapResult", "PackedCorpus",
           "cosine_similarity", "match_signatures", "match_restarts", "restart_consensus", "signature_consensus", "SignatureMatch", "ConsensusResult",
           "split_counts", "holdout", "score_exposures", "score_restarts", "pick_k", "select_num_signatures", "select_num_signatures_mmctm",
           "ScoreResult", "KPick", "KSelection", "MMSelection", "read_signatures_tsv", "refit_exposures", "RefitResult", "RefitIntervals",
           "simulate_counts", "goodness_of_fit", "FitCheck", "signature_presence", "PresenceResult", "presence_power", "PowerResult",
           "attribute_mutations", "AttributionResult", "mutation_table",
           "compare_exposures", "deal_counts", "ComparisonResult", "exposure_trajectory", "bin_by_order", "TrajectoryResult",
           "decompose_signatures", "decompose_search", "Decomposition", "SearchResult", "extract_signatures", "Extraction",
           "cluster_samples", "SampleClusters", "associate_exposures", "ExposureAssociations", "regress_exposures", "ExposureRegressions",
           "survival_association", "survival_scores", "kaplan_meier", "SurvivalAssociations", "GroupTest", "KMCurve",
           "classify_exposures", "ExposureClassifier", "cox_exposures", "ExposureCoxModel"]
