// The order of the device top-k (topk_rows_f32.hip, topk_segments_f32.hip) in one place: the 64-bit key of an entry, the sort of a
// workgroup's keys and the write of a sorted list's head.
//
// Each entry becomes ONE 64-bit key, all keys of a row (a segment) distinct, larger = better:
//     high word: the score's bits made monotone (sign flipped for positives, all bits for negatives; -0.0 first folded onto +0.0;
//                any NaN -> 0, below -inf's 0x007FFFFF)            low word: 0xFFFFFFFF - position
// so "descending score, equal scores lower position first, NaN behind every number" is the plain descending order of the keys, and
// key 0 (no position gives it) stands for "no entry".
#pragma once
#include "common.h"

constexpr int TOPK_MAX = 128;        // k and the length of a chunk's list
constexpr int TOPK_CHUNK = 4096;     // entries per pass-1 workgroup = keys one sort holds
typedef unsigned long long tkey;

__device__ __forceinline__ tkey score_key(float v, unsigned pos) {
    unsigned b = __float_as_uint(v);
    unsigned u;
    if (v != v) u = 0u;
    else {
        if (v == 0.f) b = 0u;
        u = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return ((tkey)u << 32) | (tkey)(0xFFFFFFFFu - pos);
}

// descending bitonic sort of s[0 .. n) (n a power of two, >= 2), all 256 threads; ends with a barrier
__device__ __forceinline__ void sort_desc(tkey* s, int n) {
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (n >> 1); i += 256) {
                const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo | stride;
                const bool desc = (lo & size) == 0;
                const tkey a = s[lo], b = s[hi];
                if ((a < b) == desc) {
                    s[lo] = b;
                    s[hi] = a;
                }
            }
            __syncthreads();
        }
}

// the first k keys of a sorted list -> one row of the outputs (key 0: position -1, score -inf).  `scores`: the row's (segment's)
// first entry, positions count from it; `positions` / `top`: the row's k output slots.
__device__ __forceinline__ void write_row(const tkey* s, const float* __restrict__ scores, int k, int* __restrict__ positions,
                                          float* __restrict__ top) {
    for (int j = threadIdx.x; j < k; j += 256) {
        const tkey key = s[j];
        const unsigned pos = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
        positions[j] = key ? (int)pos : -1;
        top[j] = key ? scores[pos] : -INFINITY;
    }
}

__device__ __forceinline__ int pow2_at_least(int n, int least) {
    int p = least;
    while (p < n) p <<= 1;
    return p;
}

// One merge of a row's chunk lists (n_chunk lists of TOPK_MAX keys at `mine`), 31 at a time beside the best TOPK_MAX so far, in
// s[0 .. TOPK_CHUNK): leaves the best TOPK_MAX keys sorted in s[0 .. TOPK_MAX).
__device__ __forceinline__ void merge_lists(tkey* s, const tkey* __restrict__ mine, int n_chunk) {
    constexpr int PER = TOPK_CHUNK / TOPK_MAX - 1;           // chunk lists per round, beside the best so far
    for (int j = threadIdx.x; j < TOPK_MAX; j += 256) s[j] = 0ull;
    for (int c = 0; c < n_chunk; c += PER) {
        const int n = (n_chunk - c < PER ? n_chunk - c : PER) * TOPK_MAX;
        const int n2 = pow2_at_least(TOPK_MAX + n, 2 * TOPK_MAX);
        for (int i = threadIdx.x; i < n2 - TOPK_MAX; i += 256) s[TOPK_MAX + i] = i < n ? mine[(long)c * TOPK_MAX + i] : 0ull;
        __syncthreads();
        sort_desc(s, n2);
    }
}
