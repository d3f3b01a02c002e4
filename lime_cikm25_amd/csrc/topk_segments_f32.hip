// The k best entries of every segment of a flat score vector, on the device (Model.recommend_lists): lime_topk_rows_f32's order
// (topk_keys.h) over ragged segments given as a CSR, positions counted within the segment.
//
// The grid is bounded without reading the device: a segment of n entries takes max(1, ceil(n / 4096)) chunks, at most 1 + n / 4096,
// so U + P / 4096 workgroups cover every split.  Pass 0, one workgroup: the running chunk count of the segments (which chunk workgroup
// b is) and the running count of chunk LISTS (only a segment of more than one chunk has any: at most 2 (P / 4096) in all) into the
// head of the workspace.  Pass 1, a workgroup per chunk: finds its segment by bisection, keys into LDS, bitonic sort, the best 128 to
// the outputs (a one-chunk segment, an empty one included) or to its list.  Pass 2, a workgroup per segment: a segment of several
// chunks merges its lists.  The result is the k largest of a set of distinct integers: independent of the split, the merge order and
// the run.  Every offset is clamped into [0, P] and a segment's end to its start at the least; a list slot beyond the workspace's
// (possible only with offsets that decrease) is neither written nor read.
#include "topk_keys.h"

namespace {

__global__ __launch_bounds__(SCAN_THREADS) void topk_seg_scan_kernel(const long* __restrict__ offsets, long U, long P,
                                                                       int* __restrict__ chunk_start, int* __restrict__ list_start) {
    seg_scan(offsets, U, P, chunk_start, list_start);
}

__global__ __launch_bounds__(256) void topk_seg_chunk_kernel(const float* __restrict__ scores, const long* __restrict__ offsets, long U,
                                                              long P, int k, const int* __restrict__ chunk_start,
                                                              const int* __restrict__ list_start, tkey* __restrict__ lists, long list_cap,
                                                              int* __restrict__ positions, float* __restrict__ top) {
    __shared__ tkey s[TOPK_CHUNK];
    const int b = blockIdx.x;
    if (b >= chunk_start[U]) return;                         // (workgroup-uniform)
    const long u = segment_of_chunk(chunk_start, U, b);
    const seg_range seg = segment_of(offsets, u, P);
    const int c = b - chunk_start[u], n_chunk = chunks_in(seg.n);
    if (c < 0 || c >= n_chunk) return;                       // (offsets that decrease can break the sums: stay inside the segment)
    const long c0 = (long)c * TOPK_CHUNK;
    const int n = seg.n - c0 < TOPK_CHUNK ? (int)(seg.n - c0) : TOPK_CHUNK;
    const int n2 = pow2_at_least(n, TOPK_MAX);
    for (int i = threadIdx.x; i < n2; i += 256) s[i] = i < n ? score_key(scores[seg.lo + c0 + i], (unsigned)(c0 + i)) : 0ull;
    __syncthreads();
    sort_desc(s, n2);
    if (n_chunk == 1) {
        write_row(s, scores + seg.lo, k, positions + u * k, top + u * k);
    } else {
        const long slot = (long)list_start[u] + c;
        if (slot >= 0 && slot < list_cap)
            for (int j = threadIdx.x; j < TOPK_MAX; j += 256) lists[slot * TOPK_MAX + j] = s[j];
    }
}

__global__ __launch_bounds__(256) void topk_seg_merge_kernel(const float* __restrict__ scores, const long* __restrict__ offsets, long P,
                                                              int k, const int* __restrict__ list_start, const tkey* __restrict__ lists,
                                                              long list_cap, int* __restrict__ positions, float* __restrict__ top) {
    __shared__ tkey s[TOPK_CHUNK];
    const long u = blockIdx.x;
    const long first = list_start[u];
    long n_list = list_start[u + 1] - first;
    if (n_list <= 0 || first < 0) return;                    // one chunk: pass 1 wrote the row (workgroup-uniform)
    if (first + n_list > list_cap) n_list = list_cap > first ? list_cap - first : 0;
    merge_lists(s, lists + first * TOPK_MAX, (int)n_list);
    __syncthreads();
    write_row(s, scores + segment_of(offsets, u, P).lo, k, positions + u * k, top + u * k);
}

}  // namespace

extern "C" int64_t lime_topk_segments_workspace(int64_t U, int64_t P) {
    if (U <= 0 || P < 0) return 0;
    return seg_head_floats(U) + seg_list_slots(P) * TOPK_MAX * 2;    // one 64-bit key = two floats
}

extern "C" int lime_topk_segments_f32(const float* scores, const int64_t* offsets, int64_t U, int64_t P, int32_t k, int32_t* positions,
                                      float* top_scores, float* workspace, int64_t workspace_floats, void* stream) {
    LIME_REQUIRE(offsets && positions && top_scores && (scores || P == 0), LIME_ERR_BAD_ARG, "lime_topk_segments_f32: NULL pointer");
    LIME_REQUIRE(U >= 0 && P >= 0, LIME_ERR_BAD_ARG, "lime_topk_segments_f32: bad dims (U %lld, P %lld)", (long long)U, (long long)P);
    LIME_REQUIRE(k >= 1 && k <= TOPK_MAX && U + P / TOPK_CHUNK < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED,
                 "lime_topk_segments_f32: k %d, U %lld, P %lld outside 1 <= k <= %d, U + P / %d < 2^31", k, (long long)U, (long long)P,
                 TOPK_MAX, TOPK_CHUNK);
    if (U == 0) return LIME_OK;
    const int64_t need = lime_topk_segments_workspace(U, P);
    LIME_REQUIRE(workspace && workspace_floats >= need, LIME_ERR_BAD_ARG,
                 "lime_topk_segments_f32: workspace of %lld floats, lime_topk_segments_workspace() asks for %lld", (long long)workspace_floats,
                 (long long)need);
    LIME_REQUIRE(((uintptr_t)workspace & 7) == 0, LIME_ERR_BAD_ARG, "lime_topk_segments_f32: workspace must be 8-byte aligned");
    int* chunk_start = reinterpret_cast<int*>(workspace);
    int* list_start = chunk_start + (U + 1);
    tkey* lists = reinterpret_cast<tkey*>(workspace + seg_head_floats(U));
    const long list_cap = seg_list_slots(P);
    hipLaunchKernelGGL(topk_seg_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, (const long*)offsets, (long)U, (long)P,
                       chunk_start, list_start);
    int st = lime_check_launch("lime_topk_segments_f32");
    if (st != LIME_OK) return st;
    hipLaunchKernelGGL(topk_seg_chunk_kernel, dim3((unsigned)(U + P / TOPK_CHUNK)), dim3(256), 0, (hipStream_t)stream, scores,
                       (const long*)offsets, (long)U, (long)P, k, (const int*)chunk_start, (const int*)list_start, lists, list_cap, positions,
                       top_scores);
    st = lime_check_launch("lime_topk_segments_f32");
    if (st != LIME_OK || list_cap == 0) return st;
    hipLaunchKernelGGL(topk_seg_merge_kernel, dim3((unsigned)U), dim3(256), 0, (hipStream_t)stream, scores, (const long*)offsets, (long)P, k,
                       (const int*)list_start, (const tkey*)lists, list_cap, positions, top_scores);
    return lime_check_launch("lime_topk_segments_f32");
}
