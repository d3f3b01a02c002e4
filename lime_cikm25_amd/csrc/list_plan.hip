// The grouping plan of per-user candidate lists, on the device (Model.score_lists): recommend.list_plan bit for bit.
//
// keys int32 [P] (the topic id of every pair, 0 <= key < T_all <= 8192), offsets int64 [U + 1] (user u owns pairs offsets[u] ..
// offsets[u + 1] - 1).  A user's distinct keys take slots 0 .. n_distinct[u] - 1 in ascending key order; group u S + s is (user u, its
// s-th key); order lists each user's pairs sorted by slot, stable in list order, inside the user's own range.
//
// One workgroup per user, one LDS table of T_all + 1 bins: (1) the list is counted into the bins (LDS atomics on integers: the counts
// do not depend on the order of the adds); (2) each thread owns a run of consecutive bins, a scan over the threads' (distinct, pairs)
// sums gives each present key its slot and its first row -- written as slot_key / group_offsets, and left in the bin as the key's
// cursor; (3) the list is walked in order, 256 pairs at a time: a pair goes to its key's cursor plus the number of equal keys before
// it in its chunk, and the last pair of a key in the chunk moves the cursor on.  No global atomics, nothing depends on the schedule:
// the result is a fixed function of the inputs.  A list of any length takes the same loops (L / 256 chunks of 256 compares a thread).
//
// A pair whose key is outside [0, T_all) is counted in the extra bin T_all, which takes no slot: such pairs go, in list order, behind
// the user's last group, so order stays a permutation of the user's range and every pair with a key in range is in its right group.
// Every offset is clamped into [0, P] and a user's end to its start at the least.
#include "common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_MAX_KEYS = 8192;

struct list_range {
    long lo, n;
};

__device__ __forceinline__ list_range list_of(const long* __restrict__ offsets, long u, long P) {
    long lo = offsets[u], hi = offsets[u + 1];
    lo = lo < 0 ? 0 : (lo > P ? P : lo);
    hi = hi < lo ? lo : (hi > P ? P : hi);
    return list_range{lo, hi - lo};
}

__device__ __forceinline__ int bin_of(int key, int T_all) { return (key >= 0 && key < T_all) ? key : T_all; }

// bins[0 .. T_all] <- how often each key stands in the list (bin T_all: keys out of range); ends with a barrier
__device__ __forceinline__ void count_list(int* bins, const int* __restrict__ keys, list_range r, int T_all) {
    for (int t = threadIdx.x; t <= T_all; t += LP_THREADS) bins[t] = 0;
    __syncthreads();
    for (long i = threadIdx.x; i < r.n; i += LP_THREADS) atomicAdd(&bins[bin_of(keys[r.lo + i], T_all)], 1);
    __syncthreads();
}

// inclusive scan of one value per thread over the workgroup, `total` its last entry; ends with a barrier.  The values are
// (distinct << 32 | pairs): both sums stay below 2^31
__device__ __forceinline__ long scan_threads(long (*part)[LP_THREADS], long mine, long& total) {
    part[0][threadIdx.x] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < LP_THREADS; d <<= 1) {
        const long v = part[cur][threadIdx.x] + (threadIdx.x >= d ? part[cur][threadIdx.x - d] : 0);
        part[cur ^ 1][threadIdx.x] = v;
        cur ^= 1;
        __syncthreads();
    }
    total = part[cur][LP_THREADS - 1];
    return part[cur][threadIdx.x];
}

__global__ __launch_bounds__(LP_THREADS) void list_count_kernel(const int* __restrict__ keys, const long* __restrict__ offsets, long P,
                                                                 int T_all, int* __restrict__ n_distinct) {
    __shared__ int bins[LP_MAX_KEYS + 1];
    __shared__ long part[2][LP_THREADS];
    const long u = blockIdx.x;
    count_list(bins, keys, list_of(offsets, u, P), T_all);
    long mine = 0;
    for (int t = threadIdx.x; t < T_all; t += LP_THREADS) mine += bins[t] > 0;
    long all;
    scan_threads(part, mine, all);
    if (threadIdx.x == 0) n_distinct[u] = (int)all;
}

__global__ __launch_bounds__(LP_THREADS) void list_plan_kernel(const int* __restrict__ keys, const long* __restrict__ offsets, long P,
                                                                int T_all, int S, long* __restrict__ order,
                                                                long* __restrict__ group_offsets, int* __restrict__ slot_key) {
    __shared__ int bins[LP_MAX_KEYS + 1];
    __shared__ long part[2][LP_THREADS];
    __shared__ int chunk_bin[LP_THREADS];
    __shared__ int first_key;
    const long u = blockIdx.x;
    const list_range r = list_of(offsets, u, P);
    if (threadIdx.x == 0) first_key = 0;                     // (a user with an empty list: key 0)
    count_list(bins, keys, r, T_all);

    // (2) slots and first rows: thread t owns bins t per .. t per + per - 1
    const int per = (T_all + LP_THREADS - 1) / LP_THREADS;
    const int t0 = per * (int)threadIdx.x, t1 = t0 + per < T_all ? t0 + per : T_all;
    long mine = 0;
    for (int t = t0; t < t1; ++t) {
        const int c = bins[t];
        mine += c > 0 ? (1L << 32) + c : 0L;
    }
    long total;
    const long incl = scan_threads(part, mine, total);
    const int n_slot = (int)(total >> 32);
    const long n_valid = total & 0xFFFFFFFFL;
    long run = incl - mine;
    for (int t = t0; t < t1; ++t) {
        const int c = bins[t];
        if (c > 0) {
            const int slot = (int)(run >> 32);
            const long start = run & 0xFFFFFFFFL;
            if (slot < S) {
                slot_key[u * S + slot] = t;
                group_offsets[u * S + slot] = r.lo + start;
            }
            if (slot == 0) first_key = t;
            bins[t] = (int)start;                            // the key's cursor, counted from the user's first row
            run += (1L << 32) + c;
        }
    }
    if (threadIdx.x == 0) bins[T_all] = (int)n_valid;        // pairs with a key out of range: behind every group
    __syncthreads();
    for (int s = n_slot + (int)threadIdx.x; s < S; s += LP_THREADS) {        // unused slots: empty, the user's first key
        slot_key[u * S + s] = first_key;
        group_offsets[u * S + s] = r.lo + n_valid;
    }
    if (u == (long)gridDim.x - 1 && threadIdx.x == 0) group_offsets[(u + 1) * S] = r.lo + n_valid;

    // (3) stable placement, a chunk of 256 pairs at a time
    for (long i0 = 0; i0 < r.n; i0 += LP_THREADS) {          // (workgroup-uniform)
        const long i = i0 + threadIdx.x;
        const int n_here = r.n - i0 < LP_THREADS ? (int)(r.n - i0) : LP_THREADS;
        const bool live = i < r.n;
        const int b = live ? bin_of(keys[r.lo + i], T_all) : -1;
        chunk_bin[threadIdx.x] = b;
        __syncthreads();
        int before = 0, after = 0;
        for (int j = 0; j < n_here; ++j) {
            const bool same = chunk_bin[j] == b;
            before += same && j < (int)threadIdx.x;
            after += same && j > (int)threadIdx.x;
        }
        const int cursor = live ? bins[b] : 0;
        __syncthreads();
        if (live) {
            order[r.lo + cursor + before] = r.lo + i;
            if (after == 0) bins[b] = cursor + before + 1;
        }
        __syncthreads();
    }
}

}  // namespace

static int list_plan_args(const char* who, const void* keys, const void* offsets, int64_t U, int64_t P, int32_t T_all) {
    LIME_REQUIRE(offsets && (keys || P == 0), LIME_ERR_BAD_ARG, "%s: NULL pointer", who);
    LIME_REQUIRE(U >= 0 && P >= 0 && T_all >= 1, LIME_ERR_BAD_ARG, "%s: bad dims (U %lld, P %lld, T_all %d)", who, (long long)U, (long long)P,
                 T_all);
    LIME_REQUIRE(T_all <= LP_MAX_KEYS && U < 0x7FFFFFFFL && P < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED,
                 "%s: T_all %d, U %lld, P %lld outside T_all <= %d (one LDS table of bins per workgroup), U and P < 2^31", who, T_all,
                 (long long)U, (long long)P, LP_MAX_KEYS);
    return LIME_OK;
}

extern "C" int lime_list_plan_count(const int32_t* keys, const int64_t* offsets, int64_t U, int64_t P, int32_t T_all, int32_t* n_distinct,
                                    void* stream) {
    const int st = list_plan_args("lime_list_plan_count", keys, offsets, U, P, T_all);
    if (st != LIME_OK) return st;
    LIME_REQUIRE(n_distinct || U == 0, LIME_ERR_BAD_ARG, "lime_list_plan_count: NULL pointer");
    if (U == 0) return LIME_OK;
    hipLaunchKernelGGL(list_count_kernel, dim3((unsigned)U), dim3(LP_THREADS), 0, (hipStream_t)stream, keys, (const long*)offsets, (long)P,
                       T_all, n_distinct);
    return lime_check_launch("lime_list_plan_count");
}

extern "C" int lime_list_plan(const int32_t* keys, const int64_t* offsets, int64_t U, int64_t P, int32_t T_all, int32_t S, int64_t* order,
                              int64_t* group_offsets, int32_t* slot_key, void* stream) {
    const int st = list_plan_args("lime_list_plan", keys, offsets, U, P, T_all);
    if (st != LIME_OK) return st;
    LIME_REQUIRE(group_offsets && (order || P == 0) && (slot_key || U == 0), LIME_ERR_BAD_ARG, "lime_list_plan: NULL pointer");
    LIME_REQUIRE(S >= 1, LIME_ERR_BAD_ARG, "lime_list_plan: S = %d slots, at least 1 is needed", S);
    if (U == 0) {                                            // no user: the CSR of no group
        const hipError_t e = hipMemsetAsync(group_offsets, 0, sizeof(int64_t), (hipStream_t)stream);
        LIME_REQUIRE(e == hipSuccess, LIME_ERR_LAUNCH, "lime_list_plan: hipMemsetAsync failed: %s", hipGetErrorString(e));
        return LIME_OK;
    }
    hipLaunchKernelGGL(list_plan_kernel, dim3((unsigned)U), dim3(LP_THREADS), 0, (hipStream_t)stream, keys, (const long*)offsets, (long)P,
                       T_all, S, (long*)order, (long*)group_offsets, slot_key);
    return lime_check_launch("lime_list_plan");
}
