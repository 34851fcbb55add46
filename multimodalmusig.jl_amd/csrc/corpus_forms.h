// corpus_forms.h -- what a model handle learns about a caller's corpus and the forms it keeps of it on the device, host only (plain
// C++17, no HIP): the creates of lda.hip and ctm.hip build every form here, and tests/corpus_forms_main.cpp compiles this file alone.
//
// A corpus arrives as CSR segments: doc_ptr[0 .. D] are absolute offsets into term / count (one segment for LDA, one per modality for
// CTM, whose offsets continue from one modality into the next).  Every function below takes checked arrays (mmm_check_csr, check_corpus).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// (term, count) and (document, count): the layout of HIP's int2, which the kernels read
struct alignas(8) CountPair { int32_t x, y; };      // (aligned like it: a pair is one 8-byte store)

// ---- rows of counts: a document's V counts as 16 lanes x `slots` term slots, LANE-major -- the slots of lane l (terms l, 16 + l, ...)
// are contiguous, so a lane requests its part of a row with one load (device side: row_slot, lda_rows.cuh) -----------------------------
// term slots per lane of the builds that cover V terms (0: none)
inline int count_row_slots(int V) { return V <= 32 ? 2 : (V <= 48 ? 3 : (V <= 96 ? 6 : (V <= 128 ? 8 : 0))); }
// position of term w in a row of 16 x slots
constexpr int count_row_slot(int w, int slots) { return (w & 15) * slots + (w >> 4); }
// 16-bit rows keep an even number of slots per lane (a lane's part starts on a 32-bit word) and kRows16Spare elements after the last
// row: the ll sweeps read 16 bytes from a lane's first slot
constexpr int count_row_slots16(int slots) { return (slots + 1) & ~1; }
constexpr size_t kRows16Spare = 8;

// ---- facts of one segment ---------------------------------------------------------------------------------------------------------
struct CorpusFacts {
    int max_count = 0;          // largest count
    int64_t longest_doc = 0;    // most entries of a document
    bool repeats = false;       // some document lists a term twice; only looked for on request (false otherwise)
};

// the repeated-term test of every sweep: seen[t] is the last document that listed term t (-1: none yet)
inline bool listed_twice(int* seen, int d, int term) { const bool twice = seen[term] == d; seen[term] = d; return twice; }

// [D][16 x slots] counts as T (+ spare zero elements).  A term a document lists twice keeps its last count: callers keep rows only of
// corpora without one (CorpusFacts::repeats).  facts (with V, the vocabulary): the sweep also gathers the segment's facts, in locals --
// beside its scattered stores that costs nothing, where a sweep of its own reads the corpus once more
template <class T>
std::vector<T> pack_count_rows(int D, int slots, size_t spare, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, int V = 0, CorpusFacts* facts = nullptr)
{
    const size_t Vp = (size_t)16 * slots;
    std::vector<T> rows((size_t)D * Vp + spare, 0);
    T* const r = rows.data();
    if (!facts) {
        for (int d = 0; d < D; ++d)
            for (int64_t e = doc_ptr[d]; e < doc_ptr[d + 1]; ++e) r[(size_t)d * Vp + count_row_slot(term[e], slots)] = (T)count[e];
        return rows;
    }
    std::vector<int> seen((size_t)V, -1);
    int* const sn = seen.data();
    int max_count = 0; int64_t longest = 0; bool repeats = false;
    for (int d = 0; d < D; ++d) {
        longest = std::max(longest, doc_ptr[d + 1] - doc_ptr[d]);
        for (int64_t e = doc_ptr[d]; e < doc_ptr[d + 1]; ++e) {
            max_count = std::max(max_count, count[e]);
            repeats |= listed_twice(sn, d, term[e]);
            r[(size_t)d * Vp + count_row_slot(term[e], slots)] = (T)count[e];
        }
    }
    facts->max_count = max_count; facts->longest_doc = longest; facts->repeats = repeats;
    return rows;
}

// the stand-alone sweep over a checked segment
inline CorpusFacts corpus_facts(int D, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count, bool scan_repeats)
{
    CorpusFacts f;
    for (int64_t e = doc_ptr[0]; e < doc_ptr[D]; ++e) f.max_count = std::max(f.max_count, count[e]);
    for (int d = 0; d < D; ++d) f.longest_doc = std::max<int64_t>(f.longest_doc, doc_ptr[d + 1] - doc_ptr[d]);
    if (scan_repeats) {
        std::vector<int> seen((size_t)V, -1);
        for (int d = 0; d < D && !f.repeats; ++d)
            for (int64_t e = doc_ptr[d]; e < doc_ptr[d + 1] && !f.repeats; ++e) f.repeats = listed_twice(seen.data(), d, term[e]);
    }
    return f;
}

// ---- (term, count) pairs -------------------------------------------------------------------------------------------------------------
inline std::vector<CountPair> term_count_pairs(int64_t nnz, const int32_t* term, const int32_t* count)
{
    std::vector<CountPair> tc((size_t)nnz);
    for (int64_t e = 0; e < nnz; ++e) tc[(size_t)e] = CountPair{term[e], count[e]};
    return tc;
}

// [D][V] rows of a document's (term, count) entries padded with (-1, 0): for a segment from offset 0 whose longest document has at
// most V entries
inline std::vector<CountPair> padded_term_rows(int D, int V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count)
{
    std::vector<CountPair> ell((size_t)D * V, CountPair{-1, 0});
    for (int d = 0; d < D; ++d)
        for (int64_t e = doc_ptr[d]; e < doc_ptr[d + 1]; ++e) ell[(size_t)d * V + (e - doc_ptr[d])] = CountPair{term[e], count[e]};
    return ell;
}

// ---- postings by term (the wide builds): the summation order of k_lda_stats_terms / k_ctm_stats_terms ----------------------------------
// waves per term block: segments of >= 128 postings on average, at most 8
inline int postings_stats_waves(int64_t nnz, int nterms)
{
    const int64_t avg = nnz / std::max(1, nterms);
    int w = 1;
    while (w < 8 && avg / (w * 2) >= 128) w *= 2;
    return w;
}

struct Postings {
    int nterms = 0;                     // sum of the vocabularies
    std::vector<int64_t> term_ptr;      // [nterms + 1], modality-major: the postings of term v of modality i are post[term_ptr[voff_i + v] .. )
    std::vector<CountPair> post;        // (document, count), documents ascending within a term
    int stats_waves = 1;
};

// counting sort over M segments of D + 1 offsets each (doc_ptr + i (D + 1)), which continue one another from 0
inline Postings postings_by_term(int D, int M, const int* V, const int64_t* doc_ptr, const int32_t* term, const int32_t* count)
{
    Postings p;
    std::vector<int> voff((size_t)M + 1, 0);
    for (int i = 0; i < M; ++i) voff[(size_t)i + 1] = voff[(size_t)i] + V[i];
    p.nterms = voff[(size_t)M];
    const int64_t nnz = doc_ptr[(size_t)(M - 1) * (D + 1) + D];
    p.term_ptr.assign((size_t)p.nterms + 1, 0);
    for (int i = 0; i < M; ++i) {
        const int64_t* dp = doc_ptr + (size_t)i * (D + 1);
        for (int64_t e = dp[0]; e < dp[D]; ++e) p.term_ptr[(size_t)voff[(size_t)i] + term[e] + 1]++;
    }
    for (int t = 0; t < p.nterms; ++t) p.term_ptr[(size_t)t + 1] += p.term_ptr[(size_t)t];
    p.post.resize((size_t)nnz);
    std::vector<int64_t> fill(p.term_ptr.begin(), p.term_ptr.end() - 1);
    for (int i = 0; i < M; ++i) {
        const int64_t* dp = doc_ptr + (size_t)i * (D + 1);
        for (int d = 0; d < D; ++d)
            for (int64_t e = dp[d]; e < dp[d + 1]; ++e) p.post[(size_t)fill[(size_t)voff[(size_t)i] + term[e]]++] = CountPair{d, count[e]};
    }
    p.stats_waves = postings_stats_waves(nnz, p.nterms);
    return p;
}
