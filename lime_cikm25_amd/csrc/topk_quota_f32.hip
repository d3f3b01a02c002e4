// The k best entries of every row (segment) under a quota per group, on the device (Model.recommend / recommend_schedule /
// recommend_lists with max_per_topic).  Walk the entries in lime_topk_rows_f32's order (topk_keys.h: descending score, +0.0 == -0.0,
// equal scores lower position first, NaN behind every number in position order); take an entry unless `quota` entries of its group
// were taken before it; stop at k.  A dropped entry (its drop byte is set, or its key is outside [0, n_keys)) takes no part.
//
// Two facts make the walk parallel (both checked against a sequential walk on the host: tests/test_topk_quota_cpu.py):
//   1. The result is the k best of the union, over the groups, of each group's `quota` best.
//   2. A chunk of the row may be reduced to the first 128 (TOPK_MAX) entries of ITS OWN quota walk, and the merged set walked again,
//      in any number of rounds: the result equals the global walk for every k <= 128.  (Every survivor of a chunk that beats a
//      globally taken entry e was itself taken before e -- its group's quota was not full in the chunk, so it is not full among the
//      better entries of the whole row either -- hence fewer than k of them exist and the truncation to 128 >= k loses none.)  The
//      filter has to run BEFORE the truncation: the plain best 128 of a chunk, filtered afterwards, may all belong to one group.
//      The proof asks of the cut only that it keeps k entries, so every walk here stops at k taken: a chunk's list holds the first k
//      entries of its walk and "no entry" behind them, and a slate of ten under a quota of two is usually found in the first block.
//
// So the passes are lime_topk_rows_f32's / lime_topk_segments_f32's with one step added.  Pass 1, a workgroup per chunk of 4096
// entries: keys into LDS (a dropped entry: key 0, "no entry"), bitonic sort, QUOTA WALK, the survivors' list of 128 to the workspace
// or, for a one-chunk row, the first k to the outputs.  Pass 2, a workgroup per row: 31 chunk lists at a time beside the survivors so
// far, sorted, walked again.  The key, the sort, the merge staging, the segment scan and write_row are topk_keys.h's.
//
// The walk (of the two forms that were on the table: this one, or a second sort on a (group | score | slot) key that ranks every
// entry within its group): ONE wave goes down the sorted keys 64 at a time.  A lane fetches its entry's group (keys[position], a
// gather the next block's is issued ahead of), the block's equal groups are ranked by ballot -- one round per DISTINCT group of the
// block --, a byte per group in LDS holds how many were taken in earlier blocks (saturating at min(quota, 128), so a byte is
// enough), and the taken entries are compacted in place (the write index never passes the read index).  It stops at k taken or at
// the first block of empty keys.  Chosen over the second sort because it needs no second 32 KB key array (LDS: 32 KB keys + 8 KB
// counts = 40 KB, four workgroups in a CU's 160 KB where the plain kernel's 32 KB admit five; the second sort's 72 KB leave two),
// because it stops early -- where no quota binds it reads k entries -- and because the sort it would repeat is the expensive step
// of the plain kernel.  Its worst case is a row that cannot fill k (few groups, a small quota): every block down to the first empty
// one is walked, a ballot round per distinct group in each.
//
// No atomics on global memory; the result is a fixed function of the inputs: each walk is a function of a set of distinct keys, and
// fact 2 makes the outcome independent of the chunking and of the merge order.  Positions taken from a chunk list are checked against
// the row's length and the group against n_keys before either is used, so a workspace slot that nobody wrote (possible only with
// offsets that decrease) reads nothing outside the buffers.
#include "topk_keys.h"

namespace {

constexpr int QUOTA_KEYS = 8192;     // groups: lime_list_plan's table size; one count byte each

// the group of a key's entry, -1 for "no entry": keys[position] for a position inside the row and a group inside [0, n_keys)
__device__ __forceinline__ int group_of(tkey key, const int* __restrict__ keys, int n, int n_keys) {
    const unsigned pos = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    if (!key || pos >= (unsigned)n) return -1;
    const int g = keys[pos];
    return (unsigned)g < (unsigned)n_keys ? g : -1;
}

// The quota walk over the sorted keys s[0 .. n_sorted) (n_sorted a multiple of 64, >= TOPK_MAX), all 256 threads: leaves the first k
// taken keys, in order, at the head of s[0 .. TOPK_MAX) (key 0 behind the last) and ends with a barrier.  keys: the row's
// (segment's) groups, n its length; quota already clamped to TOPK_MAX; k <= TOPK_MAX; cnt: QUOTA_KEYS count bytes.
__device__ __forceinline__ void quota_walk(tkey* s, int n_sorted, const int* __restrict__ keys, int n, int n_keys, int quota, int k,
                                           unsigned char* cnt) {
    for (int i = threadIdx.x; i < (n_keys + 3) / 4; i += 256) reinterpret_cast<unsigned*>(cnt)[i] = 0u;
    __syncthreads();
    if (threadIdx.x < 64) {                                  // (one whole wave)
        const int lane = threadIdx.x;
        const unsigned long long below = (1ull << lane) - 1ull;
        int total = 0;
        tkey key = s[lane];
        int g = group_of(key, keys, n, n_keys);
        for (int b = 0; b < n_sorted; b += 64) {
            tkey key_next = 0ull;                            // the next block's keys and groups, ahead of this block's ranking
            int g_next = -1;
            if (b + 64 < n_sorted) {
                key_next = s[b + 64 + lane];
                g_next = group_of(key_next, keys, n, n_keys);
            }
            if (__ballot(key != 0ull) == 0ull) break;        // sorted: nothing but "no entry" from here on
            bool take = false;
            unsigned long long todo = __ballot(g >= 0);
            while (todo) {                                   // one round per distinct group of the block (wave-uniform)
                const int lead = __ffsll((long long)todo) - 1;
                const int gl = __builtin_amdgcn_readlane(g, lead);
                const unsigned long long same = __ballot(g == gl);
                if (g == gl) {
                    const int have = cnt[gl];
                    take = have + __popcll(same & below) < quota;
                    const int now = have + __popcll(same);
                    if (lane == lead) cnt[gl] = (unsigned char)(now < quota ? now : quota);
                }
                todo &= ~same;
            }
            const unsigned long long taken = __ballot(take);
            const int at = total + __popcll(taken & below);  // at <= b + lane: inside the blocks already read
            if (take && at < k) s[at] = key;
            total += __popcll(taken);
            if (total >= k) break;
            key = key_next;
            g = g_next;
        }
        for (int j = (total < k ? total : k) + lane; j < TOPK_MAX; j += 64) s[j] = 0ull;
    }
    __syncthreads();
}

// the key of entry `at` of a row (segment) at position pos: 0 for a dropped one
__device__ __forceinline__ tkey quota_key(const float* __restrict__ scores, const int* __restrict__ keys, const unsigned char* __restrict__ drop,
                                          long at, unsigned pos, int n_keys) {
    if ((unsigned)keys[at] >= (unsigned)n_keys || (drop && drop[at])) return 0ull;
    return score_key(scores[at], pos);
}

__global__ __launch_bounds__(256) void quota_chunk_kernel(const float* __restrict__ scores, long ld, int C, const int* __restrict__ keys,
                                                           int n_keys, int quota, const unsigned char* __restrict__ drop, long drop_rows,
                                                           int k, tkey* __restrict__ lists, int* __restrict__ positions,
                                                           float* __restrict__ top) {
    __shared__ tkey s[TOPK_CHUNK];
    __shared__ __attribute__((aligned(4))) unsigned char cnt[QUOTA_KEYS];
    const long row = blockIdx.y;
    const int c0 = blockIdx.x * TOPK_CHUNK;
    const int n = C - c0 < TOPK_CHUNK ? C - c0 : TOPK_CHUNK;
    const int n2 = pow2_at_least(n, TOPK_MAX);
    const float* mine = scores + row * ld;
    const unsigned char* gone = drop ? drop + (row % drop_rows) * (long)C : nullptr;     // row r is masked by drop[r % drop_rows]
    for (int i = threadIdx.x; i < n2; i += 256) s[i] = i < n ? quota_key(mine, keys, gone, c0 + i, (unsigned)(c0 + i), n_keys) : 0ull;
    __syncthreads();
    sort_desc(s, n2);
    quota_walk(s, n2, keys, C, n_keys, quota, k, cnt);
    if (gridDim.x == 1) {
        write_row(s, mine, k, positions + row * k, top + row * k);
    } else {
        tkey* out = lists + (row * gridDim.x + blockIdx.x) * TOPK_MAX;
        for (int j = threadIdx.x; j < TOPK_MAX; j += 256) out[j] = s[j];
    }
}

__global__ __launch_bounds__(256) void quota_merge_kernel(const float* __restrict__ scores, long ld, int C, const int* __restrict__ keys,
                                                           int n_keys, int quota, int n_chunk, int k, const tkey* __restrict__ lists,
                                                           int* __restrict__ positions, float* __restrict__ top) {
    __shared__ tkey s[TOPK_CHUNK];
    __shared__ __attribute__((aligned(4))) unsigned char cnt[QUOTA_KEYS];
    const long row = blockIdx.x;
    merge_lists(s, lists + row * n_chunk * TOPK_MAX, n_chunk, [&](int n2) { quota_walk(s, n2, keys, C, n_keys, quota, k, cnt); });
    write_row(s, scores + row * ld, k, positions + row * k, top + row * k);
}

__global__ __launch_bounds__(SCAN_THREADS) void quota_seg_scan_kernel(const long* __restrict__ offsets, long U, long P,
                                                                        int* __restrict__ chunk_start, int* __restrict__ list_start) {
    seg_scan(offsets, U, P, chunk_start, list_start);
}

__global__ __launch_bounds__(256) void quota_seg_chunk_kernel(const float* __restrict__ scores, const long* __restrict__ offsets, long U,
                                                               long P, const int* __restrict__ keys, int n_keys, int quota,
                                                               const unsigned char* __restrict__ drop, int k,
                                                               const int* __restrict__ chunk_start, const int* __restrict__ list_start,
                                                               tkey* __restrict__ lists, long list_cap, int* __restrict__ positions,
                                                               float* __restrict__ top) {
    __shared__ tkey s[TOPK_CHUNK];
    __shared__ __attribute__((aligned(4))) unsigned char cnt[QUOTA_KEYS];
    const int b = blockIdx.x;
    if (b >= chunk_start[U]) return;                         // (workgroup-uniform)
    const long u = segment_of_chunk(chunk_start, U, b);
    const seg_range seg = segment_of(offsets, u, P);
    const int c = b - chunk_start[u], n_chunk = chunks_in(seg.n);
    if (c < 0 || c >= n_chunk) return;                       // (offsets that decrease can break the sums: stay inside the segment)
    const long c0 = (long)c * TOPK_CHUNK;
    const int n = seg.n - c0 < TOPK_CHUNK ? (int)(seg.n - c0) : TOPK_CHUNK;
    const int n2 = pow2_at_least(n, TOPK_MAX);
    for (int i = threadIdx.x; i < n2; i += 256)
        s[i] = i < n ? quota_key(scores, keys, drop, seg.lo + c0 + i, (unsigned)(c0 + i), n_keys) : 0ull;
    __syncthreads();
    sort_desc(s, n2);
    quota_walk(s, n2, keys + seg.lo, seg.n, n_keys, quota, k, cnt);
    if (n_chunk == 1) {
        write_row(s, scores + seg.lo, k, positions + u * k, top + u * k);
    } else {
        const long slot = (long)list_start[u] + c;
        if (slot >= 0 && slot < list_cap)
            for (int j = threadIdx.x; j < TOPK_MAX; j += 256) lists[slot * TOPK_MAX + j] = s[j];
    }
}

__global__ __launch_bounds__(256) void quota_seg_merge_kernel(const float* __restrict__ scores, const long* __restrict__ offsets, long P,
                                                               const int* __restrict__ keys, int n_keys, int quota, int k,
                                                               const int* __restrict__ list_start, const tkey* __restrict__ lists,
                                                               long list_cap, int* __restrict__ positions, float* __restrict__ top) {
    __shared__ tkey s[TOPK_CHUNK];
    __shared__ __attribute__((aligned(4))) unsigned char cnt[QUOTA_KEYS];
    const long u = blockIdx.x;
    const long first = list_start[u];
    long n_list = list_start[u + 1] - first;
    if (n_list <= 0 || first < 0) return;                    // one chunk: pass 1 wrote the row (workgroup-uniform)
    if (first + n_list > list_cap) n_list = list_cap > first ? list_cap - first : 0;
    const seg_range seg = segment_of(offsets, u, P);
    merge_lists(s, lists + first * TOPK_MAX, (int)n_list, [&](int n2) { quota_walk(s, n2, keys + seg.lo, seg.n, n_keys, quota, k, cnt); });
    __syncthreads();
    write_row(s, scores + seg.lo, k, positions + u * k, top + u * k);
}

}  // namespace

extern "C" int64_t lime_topk_rows_quota_workspace(int64_t U, int64_t C) {
    if (U <= 0 || C <= TOPK_CHUNK) return 0;
    return U * chunks_of(C) * TOPK_MAX * 2;                  // one 64-bit key = two floats
}

extern "C" int lime_topk_rows_quota_f32(const float* scores, int64_t ld, int64_t U, int64_t C, const int32_t* keys, int32_t n_keys,
                                        int32_t quota, const uint8_t* drop, int64_t drop_rows, int32_t k, int32_t* positions,
                                        float* top_scores, float* workspace, int64_t workspace_floats, void* stream) {
    LIME_REQUIRE(scores && keys && positions && top_scores, LIME_ERR_BAD_ARG, "lime_topk_rows_quota_f32: NULL pointer");
    LIME_REQUIRE(U >= 0 && C >= 1 && ld >= C, LIME_ERR_BAD_ARG, "lime_topk_rows_quota_f32: bad dims (U %lld, C %lld, ld %lld)", (long long)U,
                 (long long)C, (long long)ld);
    LIME_REQUIRE(quota >= 1 && n_keys >= 1 && (!drop || drop_rows >= 1), LIME_ERR_BAD_ARG,
                 "lime_topk_rows_quota_f32: quota %d, n_keys %d, drop_rows %lld: quota >= 1, n_keys >= 1 and, with a drop mask, drop_rows >= 1", quota,
                 n_keys, (long long)drop_rows);
    LIME_REQUIRE(k >= 1 && k <= TOPK_MAX && C <= 0x7FFFFFFFL && U <= 65535 && n_keys <= QUOTA_KEYS, LIME_ERR_UNSUPPORTED,
                 "lime_topk_rows_quota_f32: k %d, C %lld, U %lld, n_keys %d outside 1 <= k <= %d, C < 2^31, U <= 65535, n_keys <= %d", k,
                 (long long)C, (long long)U, n_keys, TOPK_MAX, QUOTA_KEYS);
    const int64_t need = lime_topk_rows_quota_workspace(U, C);
    LIME_REQUIRE(need == 0 || (workspace && workspace_floats >= need), LIME_ERR_BAD_ARG,
                 "lime_topk_rows_quota_f32: workspace of %lld floats, lime_topk_rows_quota_workspace() asks for %lld", (long long)workspace_floats,
                 (long long)need);
    LIME_REQUIRE(need == 0 || ((uintptr_t)workspace & 7) == 0, LIME_ERR_BAD_ARG, "lime_topk_rows_quota_f32: workspace must be 8-byte aligned");
    if (U == 0) return LIME_OK;
    const long n_chunk = chunks_of(C);
    const int q = quota < TOPK_MAX ? quota : TOPK_MAX;       // no walk takes more than TOPK_MAX entries in all
    tkey* lists = reinterpret_cast<tkey*>(workspace);
    hipLaunchKernelGGL(quota_chunk_kernel, dim3((unsigned)n_chunk, (unsigned)U), dim3(256), 0, (hipStream_t)stream, scores, (long)ld, (int)C,
                       (const int*)keys, (int)n_keys, q, (const unsigned char*)drop, (long)drop_rows, k, lists, positions, top_scores);
    int st = lime_check_launch("lime_topk_rows_quota_f32");
    if (st != LIME_OK || n_chunk == 1) return st;
    hipLaunchKernelGGL(quota_merge_kernel, dim3((unsigned)U), dim3(256), 0, (hipStream_t)stream, scores, (long)ld, (int)C, (const int*)keys,
                       (int)n_keys, q, (int)n_chunk, k, (const tkey*)lists, positions, top_scores);
    return lime_check_launch("lime_topk_rows_quota_f32");
}

extern "C" int64_t lime_topk_segments_quota_workspace(int64_t U, int64_t P) {
    if (U <= 0 || P < 0) return 0;
    return seg_head_floats(U) + seg_list_slots(P) * TOPK_MAX * 2;    // one 64-bit key = two floats
}

extern "C" int lime_topk_segments_quota_f32(const float* scores, const int64_t* offsets, int64_t U, int64_t P, const int32_t* keys,
                                            int32_t n_keys, int32_t quota, const uint8_t* drop, int32_t k, int32_t* positions,
                                            float* top_scores, float* workspace, int64_t workspace_floats, void* stream) {
    LIME_REQUIRE(offsets && positions && top_scores && ((scores && keys) || P == 0), LIME_ERR_BAD_ARG,
                 "lime_topk_segments_quota_f32: NULL pointer");
    LIME_REQUIRE(U >= 0 && P >= 0, LIME_ERR_BAD_ARG, "lime_topk_segments_quota_f32: bad dims (U %lld, P %lld)", (long long)U, (long long)P);
    LIME_REQUIRE(quota >= 1 && n_keys >= 1, LIME_ERR_BAD_ARG, "lime_topk_segments_quota_f32: quota %d, n_keys %d: both must be >= 1", quota,
                 n_keys);
    LIME_REQUIRE(k >= 1 && k <= TOPK_MAX && U + P / TOPK_CHUNK < 0x7FFFFFFFL && n_keys <= QUOTA_KEYS, LIME_ERR_UNSUPPORTED,
                 "lime_topk_segments_quota_f32: k %d, U %lld, P %lld, n_keys %d outside 1 <= k <= %d, U + P / %d < 2^31, n_keys <= %d", k,
                 (long long)U, (long long)P, n_keys, TOPK_MAX, TOPK_CHUNK, QUOTA_KEYS);
    if (U == 0) return LIME_OK;
    const int64_t need = lime_topk_segments_quota_workspace(U, P);
    LIME_REQUIRE(workspace && workspace_floats >= need, LIME_ERR_BAD_ARG,
                 "lime_topk_segments_quota_f32: workspace of %lld floats, lime_topk_segments_quota_workspace() asks for %lld",
                 (long long)workspace_floats, (long long)need);
    LIME_REQUIRE(((uintptr_t)workspace & 7) == 0, LIME_ERR_BAD_ARG, "lime_topk_segments_quota_f32: workspace must be 8-byte aligned");
    int* chunk_start = reinterpret_cast<int*>(workspace);
    int* list_start = chunk_start + (U + 1);
    tkey* lists = reinterpret_cast<tkey*>(workspace + seg_head_floats(U));
    const long list_cap = seg_list_slots(P);
    const int q = quota < TOPK_MAX ? quota : TOPK_MAX;
    hipLaunchKernelGGL(quota_seg_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, (const long*)offsets, (long)U, (long)P,
                       chunk_start, list_start);
    int st = lime_check_launch("lime_topk_segments_quota_f32");
    if (st != LIME_OK) return st;
    hipLaunchKernelGGL(quota_seg_chunk_kernel, dim3((unsigned)(U + P / TOPK_CHUNK)), dim3(256), 0, (hipStream_t)stream, scores,
                       (const long*)offsets, (long)U, (long)P, (const int*)keys, (int)n_keys, q, (const unsigned char*)drop, k,
                       (const int*)chunk_start, (const int*)list_start, lists, list_cap, positions, top_scores);
    st = lime_check_launch("lime_topk_segments_quota_f32");
    if (st != LIME_OK || list_cap == 0) return st;
    hipLaunchKernelGGL(quota_seg_merge_kernel, dim3((unsigned)U), dim3(256), 0, (hipStream_t)stream, scores, (const long*)offsets, (long)P,
                       (const int*)keys, (int)n_keys, q, k, (const int*)list_start, (const tkey*)lists, list_cap, positions, top_scores);
    return lime_check_launch("lime_topk_segments_quota_f32");
}
