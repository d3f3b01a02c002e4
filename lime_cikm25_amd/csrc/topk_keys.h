// The order of the device top-k (topk_rows_f32.hip, topk_segments_f32.hip, topk_quota_f32.hip) in one place: the 64-bit key of an
// entry, the sort of a workgroup's keys, the merge of a row's chunk lists, the write of a sorted list's head, and the split of a
// CSR's segments into chunks.
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

inline long chunks_of(long C) { return (C + TOPK_CHUNK - 1) / TOPK_CHUNK; }          // pass-1 workgroups of a row of C entries

__device__ __forceinline__ int pow2_at_least(int n, int least) {
    int p = least;
    while (p < n) p <<= 1;
    return p;
}

// One merge of a row's chunk lists (n_chunk lists of TOPK_MAX keys at `mine`), 31 at a time beside the best TOPK_MAX so far, in
// s[0 .. TOPK_CHUNK): leaves the best TOPK_MAX keys sorted in s[0 .. TOPK_MAX).  `keep(n2)` runs after every round's sort, by all 256
// threads, over the n2 sorted keys: what it leaves in s[0 .. TOPK_MAX) (sorted, behind a barrier of its own) is "the best so far" of
// the next round -- the plain top-k keeps the head as it is, the quota top-k (topk_quota_f32.hip) walks the round first.
template <class Keep>
__device__ __forceinline__ void merge_lists(tkey* s, const tkey* __restrict__ mine, int n_chunk, Keep keep) {
    constexpr int PER = TOPK_CHUNK / TOPK_MAX - 1;           // chunk lists per round, beside the best so far
    for (int j = threadIdx.x; j < TOPK_MAX; j += 256) s[j] = 0ull;
    for (int c = 0; c < n_chunk; c += PER) {
        const int n = (n_chunk - c < PER ? n_chunk - c : PER) * TOPK_MAX;
        const int n2 = pow2_at_least(TOPK_MAX + n, 2 * TOPK_MAX);
        for (int i = threadIdx.x; i < n2 - TOPK_MAX; i += 256) s[TOPK_MAX + i] = i < n ? mine[(long)c * TOPK_MAX + i] : 0ull;
        __syncthreads();
        sort_desc(s, n2);
        keep(n2);
    }
}

__device__ __forceinline__ void merge_lists(tkey* s, const tkey* __restrict__ mine, int n_chunk) {
    merge_lists(s, mine, n_chunk, [](int) {});
}

// ---- ragged segments (topk_segments_f32.hip, topk_quota_f32.hip): a CSR's segment, clamped, its chunk count and the pass-0 scan -------
constexpr int SCAN_THREADS = 256;

struct seg_range {
    long lo;
    int n;
};

// segment u of a CSR over P entries: every offset clamped into [0, P], the end to the start at the least, the length below 2^31
__device__ __forceinline__ seg_range segment_of(const long* __restrict__ offsets, long u, long P) {
    long lo = offsets[u], hi = offsets[u + 1];
    lo = lo < 0 ? 0 : (lo > P ? P : lo);
    hi = hi < lo ? lo : (hi > P ? P : hi);
    const long n = hi - lo;
    return seg_range{lo, (int)(n > 0x7FFFFFFFL ? 0x7FFFFFFFL : n)};
}

__device__ __forceinline__ int chunks_in(int n) { return n <= TOPK_CHUNK ? 1 : (int)(((long)n + TOPK_CHUNK - 1) / TOPK_CHUNK); }

// chunk_start[u], list_start[u] for u <= U: exclusive running sums of the segments' chunk counts and list counts (only a segment of
// more than one chunk has lists).  The body of a one-workgroup kernel of SCAN_THREADS threads.
__device__ __forceinline__ void seg_scan(const long* __restrict__ offsets, long U, long P, int* __restrict__ chunk_start,
                                         int* __restrict__ list_start) {
    __shared__ long part[2][SCAN_THREADS];                   // (chunks << 32 | lists) per thread: both sums stay below 2^31
    const long per = (U + SCAN_THREADS - 1) / SCAN_THREADS;
    const long u0 = per * threadIdx.x, u1 = u0 + per < U ? u0 + per : U;
    long mine = 0;
    for (long u = u0; u < u1; ++u) {
        const int c = chunks_in(segment_of(offsets, u, P).n);
        mine += ((long)c << 32) | (long)(c > 1 ? c : 0);
    }
    part[0][threadIdx.x] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {             // inclusive scan over the threads' sums
        const long v = part[cur][threadIdx.x] + (threadIdx.x >= d ? part[cur][threadIdx.x - d] : 0);
        part[cur ^ 1][threadIdx.x] = v;
        cur ^= 1;
        __syncthreads();
    }
    long run = part[cur][threadIdx.x] - mine;
    for (long u = u0; u < u1; ++u) {
        chunk_start[u] = (int)(run >> 32);
        list_start[u] = (int)(run & 0xFFFFFFFFL);
        const int c = chunks_in(segment_of(offsets, u, P).n);
        run += ((long)c << 32) | (long)(c > 1 ? c : 0);
    }
    if (threadIdx.x == SCAN_THREADS - 1) {
        const long all = part[cur][threadIdx.x];
        chunk_start[U] = (int)(all >> 32);
        list_start[U] = (int)(all & 0xFFFFFFFFL);
    }
}

// the segment u < U with chunk_start[u] <= b < chunk_start[u + 1], by bisection
__device__ __forceinline__ long segment_of_chunk(const int* __restrict__ chunk_start, long U, int b) {
    long lo = 0, hi = U;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (chunk_start[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the workspace of the segment forms: the two int32 [U + 1] sums (an even count of floats), then 2 (P / TOPK_CHUNK) list slots
inline int64_t seg_head_floats(int64_t U) { return ((2 * (U + 1) + 1) / 2) * 2; }
inline int64_t seg_list_slots(int64_t P) { return 2 * (P / TOPK_CHUNK); }
