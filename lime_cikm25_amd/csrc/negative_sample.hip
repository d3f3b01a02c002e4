// The epoch's negative sampling on the device (Train_Dataset.negative_sampling, dataset.py:42-77): per train record the candidate
// tables [positive, K sampled non-clicked news] -- news index, the record's freshness repeated, lifetime -- written from the
// resident CSR of every record's non-clicked news.  The rule per record with n non-clicked news:
//     n <= K : slot j takes j % n                                                      (dataset.py:59-63)
//     n >  K : K distinct indices, uniform over [0, m), m = n - 1 (the reference's randint has an exclusive upper bound, so its
//              last non-clicked news is never drawn) or m = n (`inclusive`)            (dataset.py:64-74)
// The reference draws and rejects; here a partial Fisher-Yates over a "virtual swap" list does the same thing -- uniform without
// replacement -- in exactly K steps: slot j takes r = (u32 * (m - j)) >> 32 among the m - j values still free, reads the value at
// r, and moves the last free value into r; the moves (at most K) are remembered as (position, value) pairs, a position never moved
// still holds its own number.  The multiply-shift picks a value with probability within (m - j) / 2^32 (relative) of 1 / (m - j).
// The draws are counter-based: u32 of draw j of record i is the upper half of the splitmix64 finaliser of dropout.h at counter
// 16 i + j under the key of (seed, site = epoch), so a row is a function of (seed, epoch, i) alone: not of N, K's neighbours, the
// grid or the launch split.  Integer arithmetic only: device_data.counter_negative_sampling states it in NumPy, bit for bit.
//
// Launch form: a flat grid, one thread per record, no loop over memory, no LDS, no atomics.  The swap list lives in registers: every
// access is an unrolled compare-and-select over the compile-time bound LIME_NEG_MAX_K (a dynamically indexed per-thread array would
// go to scratch).  Bandwidth: 20 bytes read + 12 (1 + K) written + 8 K gathered per record; at K = 4 that is 112 bytes a record.
#include "common.h"
#include "dropout.h"

namespace {

constexpr int MAXK = LIME_NEG_MAX_K;

__global__ __launch_bounds__(256) void negative_sample_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ neg_index,
                                                              const float* __restrict__ neg_lifetime, const int32_t* __restrict__ pos_index,
                                                              const float* __restrict__ pos_lifetime, const float* __restrict__ freshness,
                                                              int32_t* __restrict__ cand_index, float* __restrict__ cand_freshness,
                                                              float* __restrict__ cand_lifetime, long i0, unsigned rows, long nnz, int K,
                                                              int inclusive, LimeDropout d) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;            // rows < 2^31 (the host splits longer calls)
    if (t >= rows) return;
    const long i = i0 + t;
    // every offset is clamped into [0, nnz]: a broken table reads inside the arrays whatever it says
    long lo = offsets[i], hi = offsets[i + 1];
    lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
    hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
    const unsigned n = (unsigned)(hi - lo);                        // nnz < 2^31
    const long o = i * (long)(K + 1);
    const float fr = freshness[i];
    const int p_idx = pos_index[i];
    const float p_lt = pos_lifetime[i];
    cand_index[o] = p_idx;
    cand_freshness[o] = fr;
    cand_lifetime[o] = p_lt;
    const unsigned m = inclusive ? n : n - 1u;
    const bool draw = n > (unsigned)K;
    unsigned pos[MAXK], val[MAXK];                                 // the virtual swaps: position pos[s] holds val[s] (the latest wins)
    unsigned cyc = 0;
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
        if (j >= K) continue;                                      // K is uniform: a scalar branch; the trip count stays a constant
        unsigned k;
        if (draw) {
            const unsigned c = m - (unsigned)j;                    // values still free: positions 0 .. c - 1
            const unsigned u = (unsigned)(lime_hash4(d, (uint64_t)i * (uint64_t)MAXK + (uint64_t)j) >> 32);
            const unsigned r = (unsigned)(((uint64_t)u * (uint64_t)c) >> 32);
            unsigned last = c - 1u;
            k = r;
#pragma unroll
            for (int s = 0; s < j; ++s) {
                k = pos[s] == r ? val[s] : k;
                last = pos[s] == c - 1u ? val[s] : last;
            }
            pos[j] = r;
            val[j] = last;
        } else {
            k = cyc;                                               // j % n without a division
            cyc = cyc + 1u == n ? 0u : cyc + 1u;
        }
        // a record without non-clicked news (refused by the host layers) repeats its positive: nothing is read out of range
        cand_index[o + 1 + j] = n ? neg_index[lo + k] : p_idx;
        cand_freshness[o + 1 + j] = fr;
        cand_lifetime[o + 1 + j] = n ? neg_lifetime[lo + k] : p_lt;
    }
}

}  // namespace

extern "C" int lime_negative_sample(const int64_t* offsets, const int32_t* neg_index, const float* neg_lifetime, int64_t nnz,
                                    const int32_t* pos_index, const float* pos_lifetime, const float* freshness, int32_t* cand_index,
                                    float* cand_freshness, float* cand_lifetime, int64_t N, int32_t K, uint64_t seed, uint32_t epoch,
                                    int32_t inclusive, void* stream) {
    LIME_REQUIRE(offsets && neg_index && neg_lifetime && pos_index && pos_lifetime && freshness && cand_index && cand_freshness &&
                 cand_lifetime, LIME_ERR_BAD_ARG, "lime_negative_sample: NULL pointer");
    LIME_REQUIRE(K >= 1 && K <= MAXK, LIME_ERR_BAD_ARG, "lime_negative_sample: K %d outside [1, %d]", K, MAXK);
    LIME_REQUIRE(N >= 0 && N < (1LL << 56), LIME_ERR_BAD_ARG, "lime_negative_sample: bad record count %lld", (long long)N);
    LIME_REQUIRE(nnz >= 0 && nnz < (1LL << 31), LIME_ERR_BAD_ARG, "lime_negative_sample: nnz %lld outside [0, 2^31)", (long long)nnz);
    const LimeDropout d = lime_make_dropout(0.f, seed, epoch);     // the key of (seed, epoch); the threshold and scale are unused
    const int64_t rows_per_launch = 0x7FFFFF00LL;                  // 32-bit thread index in the kernel
    for (int64_t i0 = 0; i0 < N; i0 += rows_per_launch) {
        const unsigned rows = (unsigned)(N - i0 < rows_per_launch ? N - i0 : rows_per_launch);
        hipLaunchKernelGGL(negative_sample_kernel, dim3((rows + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, offsets, neg_index,
                           neg_lifetime, pos_index, pos_lifetime, freshness, cand_index, cand_freshness, cand_lifetime, (long)i0, rows,
                           (long)nnz, (int)K, (int)(inclusive != 0), d);
        const int st = lime_check_launch("lime_negative_sample");
        if (st != LIME_OK) return st;
    }
    return LIME_OK;
}
