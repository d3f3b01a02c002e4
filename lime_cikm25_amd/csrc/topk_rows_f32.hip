// The k best entries of every row of a score matrix, on the device (Model.recommend).  Order: descending score; equal scores -- +0.0
// and -0.0 are equal -- lower position first; a NaN ranks behind every number, NaNs among themselves in position order.
//
// Each entry becomes ONE 64-bit key, all keys of a row distinct, larger = better:
//     high word: the score's bits made monotone (sign flipped for positives, all bits for negatives; -0.0 first folded onto +0.0;
//                any NaN -> 0, below -inf's 0x007FFFFF)            low word: 0xFFFFFFFF - position
// so the order above is the plain descending order of the keys, and key 0 (no position gives it) stands for "no entry".
// Pass 1, a workgroup per (row, chunk of 4096 columns): keys into LDS, bitonic sort, the best 128 to the workspace (or, when the row is
// one chunk, straight to the outputs).  Pass 2, a workgroup per row: the chunks' lists, 31 at a time beside the best 128 so far, sorted
// again.  The result is the k largest of a set of distinct integers: it does not depend on the chunking, the merge order or the run.
// The returned score is read back from `scores` at the position, so its bits (the sign of a zero, a NaN's payload) are the input's.
#include "common.h"

namespace {

constexpr int TOPK_MAX = 128;        // k and the length of a chunk's list
constexpr int TOPK_CHUNK = 4096;     // columns per pass-1 workgroup = keys one sort holds
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

// the first k keys of a sorted list -> the outputs of row `row` (key 0: position -1, score -inf)
__device__ __forceinline__ void write_row(const tkey* s, const float* __restrict__ scores, long ld, long row, int k,
                                          int* __restrict__ positions, float* __restrict__ top) {
    for (int j = threadIdx.x; j < k; j += 256) {
        const tkey key = s[j];
        const unsigned pos = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
        positions[row * k + j] = key ? (int)pos : -1;
        top[row * k + j] = key ? scores[row * ld + pos] : -INFINITY;
    }
}

__device__ __forceinline__ int pow2_at_least(int n, int least) {
    int p = least;
    while (p < n) p <<= 1;
    return p;
}

__global__ __launch_bounds__(256) void topk_chunk_kernel(const float* __restrict__ scores, long ld, int C, int k, tkey* __restrict__ lists,
                                                          int* __restrict__ positions, float* __restrict__ top) {
    __shared__ tkey s[TOPK_CHUNK];
    const long row = blockIdx.y;
    const int c0 = blockIdx.x * TOPK_CHUNK;
    const int n = C - c0 < TOPK_CHUNK ? C - c0 : TOPK_CHUNK;
    const int n2 = pow2_at_least(n, TOPK_MAX);
    for (int i = threadIdx.x; i < n2; i += 256) s[i] = i < n ? score_key(scores[row * ld + c0 + i], (unsigned)(c0 + i)) : 0ull;
    __syncthreads();
    sort_desc(s, n2);
    if (gridDim.x == 1) {
        write_row(s, scores, ld, row, k, positions, top);
    } else {
        tkey* out = lists + (row * gridDim.x + blockIdx.x) * TOPK_MAX;
        for (int j = threadIdx.x; j < TOPK_MAX; j += 256) out[j] = s[j];
    }
}

__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ scores, long ld, int n_chunk, int k,
                                                          const tkey* __restrict__ lists, int* __restrict__ positions, float* __restrict__ top) {
    __shared__ tkey s[TOPK_CHUNK];
    constexpr int PER = TOPK_CHUNK / TOPK_MAX - 1;           // chunk lists per round, beside the best so far
    const long row = blockIdx.x;
    const tkey* mine = lists + row * n_chunk * TOPK_MAX;
    for (int j = threadIdx.x; j < TOPK_MAX; j += 256) s[j] = 0ull;
    for (int c = 0; c < n_chunk; c += PER) {
        const int n = (n_chunk - c < PER ? n_chunk - c : PER) * TOPK_MAX;
        const int n2 = pow2_at_least(TOPK_MAX + n, 2 * TOPK_MAX);
        for (int i = threadIdx.x; i < n2 - TOPK_MAX; i += 256) s[TOPK_MAX + i] = i < n ? mine[(long)c * TOPK_MAX + i] : 0ull;
        __syncthreads();
        sort_desc(s, n2);
    }
    write_row(s, scores, ld, row, k, positions, top);
}

inline long chunks_of(long C) { return (C + TOPK_CHUNK - 1) / TOPK_CHUNK; }

}  // namespace

extern "C" int64_t lime_topk_rows_workspace(int64_t U, int64_t C) {
    if (U <= 0 || C <= TOPK_CHUNK) return 0;
    return U * chunks_of(C) * TOPK_MAX * 2;                  // one 64-bit key = two floats
}

extern "C" int lime_topk_rows_f32(const float* scores, int64_t ld, int64_t U, int64_t C, int32_t k, int32_t* positions, float* top_scores,
                                  float* workspace, int64_t workspace_floats, void* stream) {
    LIME_REQUIRE(scores && positions && top_scores, LIME_ERR_BAD_ARG, "lime_topk_rows_f32: NULL pointer");
    LIME_REQUIRE(U >= 0 && C >= 1 && ld >= C, LIME_ERR_BAD_ARG, "lime_topk_rows_f32: bad dims (U %lld, C %lld, ld %lld)", (long long)U,
                 (long long)C, (long long)ld);
    LIME_REQUIRE(k >= 1 && k <= TOPK_MAX && C <= 0x7FFFFFFFL && U <= 65535, LIME_ERR_UNSUPPORTED,
                 "lime_topk_rows_f32: k %d, C %lld, U %lld outside 1 <= k <= %d, C < 2^31, U <= 65535", k, (long long)C, (long long)U, TOPK_MAX);
    const int64_t need = lime_topk_rows_workspace(U, C);
    LIME_REQUIRE(need == 0 || (workspace && workspace_floats >= need), LIME_ERR_BAD_ARG,
                 "lime_topk_rows_f32: workspace of %lld floats, lime_topk_rows_workspace() asks for %lld", (long long)workspace_floats, (long long)need);
    LIME_REQUIRE(need == 0 || ((uintptr_t)workspace & 7) == 0, LIME_ERR_BAD_ARG, "lime_topk_rows_f32: workspace must be 8-byte aligned");
    if (U == 0) return LIME_OK;
    const long n_chunk = chunks_of(C);
    tkey* lists = reinterpret_cast<tkey*>(workspace);
    hipLaunchKernelGGL(topk_chunk_kernel, dim3((unsigned)n_chunk, (unsigned)U), dim3(256), 0, (hipStream_t)stream, scores, (long)ld, (int)C, k,
                       lists, positions, top_scores);
    int st = lime_check_launch("lime_topk_rows_f32");
    if (st != LIME_OK || n_chunk == 1) return st;
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)U), dim3(256), 0, (hipStream_t)stream, scores, (long)ld, (int)n_chunk, k,
                       (const tkey*)lists, positions, top_scores);
    return lime_check_launch("lime_topk_rows_f32");
}
