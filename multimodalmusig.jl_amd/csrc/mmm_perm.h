// mmm_perm.h -- what the permutation tests share (assoc.hip, survival.hip, classify.hip, cox.hip): the doubled midranks the host forms, and the block-level sort
// that builds a within-stratum permutation from Philox keys (include/mmmusig.h, mmm_associate_exposures, has the definition)
#pragma once
#include "mmm_philox.h"

#include <algorithm>
#include <utility>
#include <vector>

// doubled midranks of v[0], v[stride], ..: 2 #{less} + #{equal} + 1 (IEEE comparisons: -0.0 equals 0.0).  idx returns the order: the indices
// in ascending (v, index).
inline void perm_ranks(const double* v, size_t stride, int n, std::vector<int>& idx, uint16_t* out, size_t ostride)
{
    std::vector<std::pair<double, int>> t((size_t)n);           // sorted as pairs: the values lie side by side
    for (int i = 0; i < n; ++i) t[i] = std::make_pair(v[(size_t)i * stride], i);
    std::sort(t.begin(), t.end());
    for (int lo = 0; lo < n;) {
        int hi = lo + 1;
        while (hi < n && t[hi].first == t[lo].first) ++hi;
        for (int j = lo; j < hi; ++j) { idx[j] = t[j].second; out[(size_t)t[j].second * ostride] = (uint16_t)(2 * lo + (hi - lo) + 1); }
        lo = hi;
    }
}

// Every thread of the block calls this.  keys [n2] in LDS (n2 = the power of two >= D) receives the composites
// (stratum << 44 | key << 12 | d) of the replicate with GLOBAL index bg in ascending order, padded with all-ones: keys[j] & 0xFFF is e_j.
// A thread computes the Philox words of four samples; the sort is bitonic.  Ends behind a barrier.
__device__ __forceinline__ void perm_sorted_keys(unsigned long long* keys, int tid, int nt, int D, int n2, const uint16_t* strat, uint32_t bits, uint32_t bg,
                                                 uint32_t stream, uint32_t k0, uint32_t k1)
{
    for (int i4 = tid; 4 * i4 < n2; i4 += nt) {
        uint32_t u[4];
        philox4x32_10((uint32_t)i4, bits, bg, stream, k0, k1, u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = 4 * i4 + j;
            if (d < n2) keys[d] = d < D ? ((unsigned long long)strat[d] << 44) | ((unsigned long long)u[j] << 12) | (unsigned long long)d : ~0ull;
        }
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += nt) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long ka = keys[i], kb = keys[l];
                if ((ka > kb) == ((i & k) == 0)) { keys[i] = kb; keys[l] = ka; }
            }
            __syncthreads();
        }
}
