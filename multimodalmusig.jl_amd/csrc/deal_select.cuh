// deal_select.cuh -- the fixed-size dealing of include/mmmusig.h (mmm_deal_counts, mmm_compare_exposures, mmm_exposure_trajectory) for one
// wave, the one copy that compare.hip and trajectory.hip run.  Mutation i carries the key k_i = u_i >> (32 - key_bits), u_i its own Philox
// word; the dealt set is the Na smallest (k_i, i).  A wave never materialises the keys: Philox is counter-based, so it regenerates them.  A
// radix select over 256 wave-private LDS bins finds the Na-th smallest key digit by digit (8 bits a pass); one more pass, chunks of 256
// mutations ascending, deals every key below that threshold and, by a ballot prefix in index order, the first r of the keys equal to it.
// Integer throughout: the same bits under every geometry.
#pragma once
#include <cstdint>
#include "mmm_philox.h"
#include "mixture_fit.cuh"

// Second Philox counter word of a dealing: 0xD0000000 | d.  High nibble 0xD is set by no other user of these words: extract.hip sets
// 0x80000000 | j, classify.hip 0x90000000, survival.hip 0xA0000000, cox.hip 0xB0000000, cluster.hip 0xC0000000 | k (k <= 32), assoc.hip
// 0xE0000000 (kExRowBit, kCfBits, kSvBits, kCxBits, kClBits and kAsBits of those files, checked against them: bits 31, 30 and 28 without
// bit 29 are set by none); the resampler, the split and the simulator put a document or item index below 2^31 there.  Hence D <= 2^28.
constexpr uint32_t kDealTag = 0xD0000000u;
constexpr int kDealMaxD = 1 << 28;
constexpr int kDealBins = 256;                  // one 8-bit digit of the key per pass

struct DealCut {
    uint32_t key, ties;              // set a = every key below `key` and the first `ties` (in index order) of the keys equal to it
};

// The Na-th smallest key (1 <= Na <= N) of the N mutations of (item, b) and how many of the keys equal to it belong to set a.  bins: the
// wave's 256 LDS words.  Lane l owns bins 4 l .. 4 l + 3 when the threshold bin is looked up.
__device__ __forceinline__ DealCut deal_select(int lane, uint32_t N, uint32_t Na, int key_bits, uint32_t* bins, uint32_t item, uint32_t b, uint32_t stream,
                                               uint32_t k0, uint32_t k1)
{
    const int shift = 32 - key_bits;
    const uint32_t nblk = (N + 3u) >> 2;
    uint32_t prefix = 0u, mask = 0u, need = Na;
    for (int s = ((key_bits + 7) >> 3) * 8 - 8; s >= 0; s -= 8) {
        for (int i = lane; i < kDealBins; i += 64) bins[i] = 0u;
        rf_wave_sync();
        for (uint32_t i4 = (uint32_t)lane; i4 < nblk; i4 += 64u) {
            uint32_t u[4];
            philox4x32_10(i4, item, b, stream, k0, k1, u);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t k = u[j] >> shift;
                if (4u * i4 + (uint32_t)j < N && (k & mask) == prefix) atomicAdd(&bins[(k >> s) & 255u], 1u);
            }
        }
        rf_wave_sync();
        uint32_t c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = bins[4 * lane + q];
        const uint32_t tot = (c[0] + c[1]) + (c[2] + c[3]);
        uint32_t inc = tot;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
        // the candidates of this pass number >= need >= 1: exactly one lane holds the bin of the need-th smallest
        uint32_t run = inc - tot, digit = 0u, below = 0u;
        const bool here = inc >= need && run < need;
        if (here) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (run < need && run + c[q] >= need) { digit = (uint32_t)(4 * lane + q); below = run; }
                run += c[q];
            }
        }
        const int src = __ffsll((long long)__ballot(here)) - 1;
        digit = __shfl(digit, src, 64); below = __shfl(below, src, 64);
        need -= below;
        prefix |= digit << s; mask |= 255u << s;
        rf_wave_sync();
    }
    DealCut r;
    r.key = prefix; r.ties = need;
    return r;
}

// The dealing pass: chunks of 256 mutations (64 Philox blocks) ascending; within a chunk the index order is (lane, word).  `slot(i)` is the
// place of mutation i in hist (the term or entry it lies in); integer atomics commute, so only the ranks of the ties depend on the order.
template <class Slot, class Hist>
__device__ __forceinline__ void deal_pass(int lane, uint32_t N, const DealCut cut, int key_bits, Slot slot, Hist* hist, uint32_t item, uint32_t b,
                                          uint32_t stream, uint32_t k0, uint32_t k1)
{
    const int shift = 32 - key_bits;
    const uint32_t nblk = (N + 3u) >> 2;
    const unsigned long long lower = (1ull << lane) - 1ull;
    uint32_t ties_seen = 0u;                                   // the same in every lane
    for (uint32_t base = 0u; base < nblk; base += 64u) {
        const uint32_t i4 = base + (uint32_t)lane;
        uint32_t u[4] = {0u, 0u, 0u, 0u};
        if (i4 < nblk) philox4x32_10(i4, item, b, stream, k0, k1, u);
        bool lt[4], eq[4];
        uint32_t rank = ties_seen, total = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = i4 < nblk && 4u * i4 + (uint32_t)j < N;
            const uint32_t k = u[j] >> shift;
            lt[j] = valid && k < cut.key;
            eq[j] = valid && k == cut.key;
            const unsigned long long m = __ballot(eq[j]);
            rank += (uint32_t)__popcll(m & lower);
            total += (uint32_t)__popcll(m);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool take = lt[j] || (eq[j] && rank < cut.ties);
            rank += eq[j] ? 1u : 0u;
            if (take) atomicAdd(&hist[slot(4u * i4 + (uint32_t)j)], (Hist)1);
        }
        ties_seen += total;
    }
}
