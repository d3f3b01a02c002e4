// The k best entries of every row of a score matrix, on the device (Model.recommend).  Order: descending score; equal scores -- +0.0
// and -0.0 are equal -- lower position first; a NaN ranks behind every number, NaNs among themselves in position order.
//
// The key of an entry, the sort and the merge are topk_keys.h's (shared with topk_segments_f32.hip).
// Pass 1, a workgroup per (row, chunk of 4096 columns): keys into LDS, bitonic sort, the best 128 to the workspace (or, when the row is
// one chunk, straight to the outputs).  Pass 2, a workgroup per row: the chunks' lists, 31 at a time beside the best 128 so far, sorted
// again.  The result is the k largest of a set of distinct integers: it does not depend on the chunking, the merge order or the run.
// The returned score is read back from `scores` at the position, so its bits (the sign of a zero, a NaN's payload) are the input's.
#include "topk_keys.h"

namespace {

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
        write_row(s, scores + row * ld, k, positions + row * k, top + row * k);
    } else {
        tkey* out = lists + (row * gridDim.x + blockIdx.x) * TOPK_MAX;
        for (int j = threadIdx.x; j < TOPK_MAX; j += 256) out[j] = s[j];
    }
}

__global__ __launch_bounds__(256) void topk_merge_kernel(const float* __restrict__ scores, long ld, int n_chunk, int k,
                                                          const tkey* __restrict__ lists, int* __restrict__ positions, float* __restrict__ top) {
    __shared__ tkey s[TOPK_CHUNK];
    const long row = blockIdx.x;
    merge_lists(s, lists + row * n_chunk * TOPK_MAX, n_chunk);
    write_row(s, scores + row * ld, k, positions + row * k, top + row * k);
}

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
