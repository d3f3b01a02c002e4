// The dev / test pass behind the scores, on the device (util.py:113-123 + evaluate.py:32-89): per impression the 1-based rank of
// every candidate under a stable descending order, and AUC / MRR / nDCG@5 / nDCG@10 from those ranks; then the sums of the four
// metrics over the counted impressions.
//
// Rank by COUNTING, not sorting:
//     rank_i      = 1 + #{j in the impression : s_j > s_i or (s_j == s_i and j < i)}
//     ahead_pos_i =     #{j ... the same condition ... and label_j != 0}
// Stable by construction (ties keep the candidate order; +0.0 == -0.0 under the IEEE comparison), no data-dependent control flow.
// evaluate.scoring feeds 1 / rank into every metric, so the metrics are functions of the ranks of the positives alone
// (P positives, N = n - P negatives, q = the rank of a positive):
//     AUC    = (P N - sum_pos (q - 1 - ahead_pos)) / (P N)        an exact 64-bit integer numerator, one fp64 division
//     MRR    = (sum_pos 1 / q) / P
//     nDCG@k = (sum_pos, q <= k  disc[q - 1]) / (sum_{p < min(k, P)} disc[p])
//
// Work distribution (one launch, the form is chosen per impression from `offsets` inside it): a workgroup of four waves takes a
// group of four consecutive impressions.
//   * n <= 512 rows: ONE WAVE per impression.  Its (score, label) pairs sit in the wave's 4 KB slice of LDS; lanes own rows i, the j
//     loop reads one LDS address per step for all lanes (a broadcast: no bank conflict).
//   * n > 512: the WHOLE WORKGROUP, one such impression after the other, with j tiled through the 16 KB (2048 rows) the four slices
//     make together and four rows i per thread in registers: any length.
// No inter-workgroup communication.  Every fp64 sum inside an impression has a fixed operand order -- a lane's rows in row order,
// then the xor shuffle tree of the wave, then (workgroup form) the four waves in wave order -- and which form an impression takes
// depends on its length alone, so per_imp does not depend on the grid.  The sums over the impressions are a second, fixed-order tree
// over per_imp: chunks of 1024 impressions (reduce_chunks_kernel: any grid, a chunk's sum does not depend on which workgroup took
// it), then one workgroup over the chunk sums (reduce_final_kernel).  No floating-point atomics anywhere.
#include "common.h"

namespace {

constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
constexpr int WAVE_CAP = 512;                // rows of an impression one wave keeps in its LDS slice
constexpr int TILE = WAVES * WAVE_CAP;       // rows of a j tile of the workgroup form
constexpr int IB = 4;                        // rows i per thread of the workgroup form
constexpr int CHUNK = 1024;                  // impressions per leaf of the reduction tree

struct Acc {
    double mrr, d5, d10;
    long long neg_ahead;                     // sum over the positives of the negatives ranked ahead of them
    int pos, bad;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// rows [0, cnt) of an LDS tile (global row j0 + j) against NB rows i of this lane: one broadcast ds_read_b64 per step
template <int NB>
__device__ __forceinline__ void count_tile(const uint2* __restrict__ tile, int cnt, int j0, const float (&si)[NB], const int (&ii)[NB],
                                           int (&rk)[NB], int (&ap)[NB]) {
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
        const uint2 e = tile[j];
        const float sj = __uint_as_float(e.x);
        const int gj = j0 + j;
        const int pj = e.y != 0u;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int beats = (sj > si[b]) | ((sj == si[b]) & (gj < ii[b]));
            rk[b] += beats;
            ap[b] += beats & pj;
        }
    }
}

// what row i with 1-based rank q adds to its impression's sums
__device__ __forceinline__ void add_row(Acc& a, int q, int ahead_pos, unsigned lab, float s, const double* __restrict__ disc) {
    a.bad |= (lab > 1u) | (s != s);
    if (lab != 0u) {
        a.pos += 1;
        a.neg_ahead += q - 1 - ahead_pos;
        a.mrr += 1.0 / (double)q;
        if (q <= 10) {
            const double d = disc[q - 1];
            a.d10 += d;
            if (q <= 5) a.d5 += d;
        }
    }
}

// one thread: the impression's status and four metrics from its sums
__device__ __forceinline__ void finish(int imp, int n, int skipped, int pos, int bad, long long neg_ahead, double mrr, double d5, double d10,
                                       const double* __restrict__ disc, double* __restrict__ per_imp, int* __restrict__ status) {
    int st;
    if (skipped || n == 0) st = 1;
    else if (bad) st = 3;
    else if (pos == 0 || pos == n) st = 2;
    else st = 0;
    double auc = 0.0, m = 0.0, n5 = 0.0, n10 = 0.0;
    if (st == 0) {
        const long long pairs = (long long)pos * (long long)(n - pos);
        auc = (double)(pairs - neg_ahead) / (double)pairs;
        m = mrr / (double)pos;
        double ideal = 0.0, ideal5 = 0.0;
        for (int p = 0; p < 10 && p < pos; ++p) {
            ideal += disc[p];
            if (p == 4 || (p < 4 && p == pos - 1)) ideal5 = ideal;
        }
        n5 = d5 / ideal5;
        n10 = d10 / ideal;
    }
    double* o = per_imp + (long)imp * 4;
    o[0] = auc;
    o[1] = m;
    o[2] = n5;
    o[3] = n10;
    status[imp] = st;
}

__global__ __launch_bounds__(THREADS) void rank_metrics_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ labels,
                                                                const int* __restrict__ offsets, const unsigned char* __restrict__ skip,
                                                                const double* __restrict__ disc, int* __restrict__ ranks,
                                                                double* __restrict__ per_imp, int* __restrict__ status, int R, int n_imp,
                                                                int n_groups) {
    __shared__ uint2 sm[TILE];               // (score bits, label): four wave slices, or one tile of the workgroup form
    __shared__ double red_f[WAVES][3];
    __shared__ long long red_n[WAVES];
    __shared__ int red_i[WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
        // ---- a wave per impression -------------------------------------------------------------------------------------------
        const int imp = g * WAVES + wave;
        int beg = 0, n = 0;
        if (imp < n_imp) {                   // offsets are clamped into [0, R]: a malformed list cannot take a store out of bounds
            beg = min(max(offsets[imp], 0), R);
            n = min(max(offsets[imp + 1], beg), R) - beg;
        }
        const bool small = imp < n_imp && n <= WAVE_CAP;
        uint2* sl = sm + wave * WAVE_CAP;
        if (small)
            for (int r = lane; r < n; r += 64) sl[r] = make_uint2(__float_as_uint(scores[beg + r]), (unsigned)labels[beg + r]);
        __syncthreads();
        if (small) {
            Acc a = {0.0, 0.0, 0.0, 0ll, 0, 0};
            for (int c0 = 0; c0 < n; c0 += 64) {
                const int i = c0 + lane;
                const bool live = i < n;
                const uint2 e = sl[live ? i : 0];
                const float si[1] = {__uint_as_float(e.x)};
                const int ii[1] = {live ? i : -1};
                int rk[1] = {0}, ap[1] = {0};
                count_tile<1>(sl, n, 0, si, ii, rk, ap);
                if (live) {
                    ranks[beg + i] = rk[0] + 1;
                    add_row(a, rk[0] + 1, ap[0], e.y, si[0], disc);
                }
            }
            const int pos = wave_sum_i32(a.pos), bad = wave_sum_i32(a.bad);
            const long long na = wave_sum_i64(a.neg_ahead);
            const double mrr = wave_sum_f64(a.mrr), d5 = wave_sum_f64(a.d5), d10 = wave_sum_f64(a.d10);
            if (lane == 0) finish(imp, n, skip != nullptr && skip[imp] != 0, pos, bad, na, mrr, d5, d10, disc, per_imp, status);
        }
        // ---- the workgroup, for every longer impression of the group in turn (the conditions are workgroup-uniform) -------------
        for (int k = 0; k < WAVES; ++k) {
            const int impk = g * WAVES + k;
            if (impk >= n_imp) break;
            const int bk = min(max(offsets[impk], 0), R);
            const int nk = min(max(offsets[impk + 1], bk), R) - bk;
            if (nk <= WAVE_CAP) continue;
            Acc a = {0.0, 0.0, 0.0, 0ll, 0, 0};
            for (int i0 = 0; i0 < nk; i0 += THREADS * IB) {
                float si[IB];
                unsigned li[IB];
                int ii[IB], rk[IB], ap[IB];
#pragma unroll
                for (int b = 0; b < IB; ++b) {
                    const int i = i0 + b * THREADS + tid;
                    const bool live = i < nk;
                    si[b] = live ? scores[bk + i] : 0.f;
                    li[b] = live ? (unsigned)labels[bk + i] : 0u;
                    ii[b] = live ? i : -1;
                    rk[b] = 0;
                    ap[b] = 0;
                }
                for (int j0 = 0; j0 < nk; j0 += TILE) {
                    const int cnt = min(TILE, nk - j0);
                    __syncthreads();         // the previous tile (or the wave slices) has been read by everyone
                    for (int r = tid; r < cnt; r += THREADS)
                        sm[r] = make_uint2(__float_as_uint(scores[bk + j0 + r]), (unsigned)labels[bk + j0 + r]);
                    __syncthreads();
                    count_tile<IB>(sm, cnt, j0, si, ii, rk, ap);
                }
#pragma unroll
                for (int b = 0; b < IB; ++b)
                    if (ii[b] >= 0) {
                        ranks[bk + ii[b]] = rk[b] + 1;
                        add_row(a, rk[b] + 1, ap[b], li[b], si[b], disc);
                    }
            }
            const int pos = wave_sum_i32(a.pos), bad = wave_sum_i32(a.bad);
            const long long na = wave_sum_i64(a.neg_ahead);
            const double mrr = wave_sum_f64(a.mrr), d5 = wave_sum_f64(a.d5), d10 = wave_sum_f64(a.d10);
            if (lane == 0) {
                red_f[wave][0] = mrr;
                red_f[wave][1] = d5;
                red_f[wave][2] = d10;
                red_n[wave] = na;
                red_i[wave][0] = pos;
                red_i[wave][1] = bad;
            }
            __syncthreads();
            if (tid == 0) {
                double f0 = red_f[0][0], f1 = red_f[0][1], f2 = red_f[0][2];
                long long nn = red_n[0];
                int p = red_i[0][0], bd = red_i[0][1];
                for (int w = 1; w < WAVES; ++w) {
                    f0 += red_f[w][0];
                    f1 += red_f[w][1];
                    f2 += red_f[w][2];
                    nn += red_n[w];
                    p += red_i[w][0];
                    bd += red_i[w][1];
                }
                finish(impk, nk, skip != nullptr && skip[impk] != 0, p, bd, nn, f0, f1, f2, disc, per_imp, status);
            }
            __syncthreads();                 // red_* may be written again by the next long impression
        }
        __syncthreads();                     // the next group's wave slices overwrite sm
    }
}

// this thread's five partial sums -> the workgroup's, in thread 0: the wave shuffle tree, then the waves in wave order
__device__ __forceinline__ void block_sum5(double (&s)[4], long long& cnt, double (*red)[4], long long* redc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 0; m < 4; ++m) s[m] = wave_sum_f64(s[m]);
    cnt = wave_sum_i64(cnt);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < 4; ++m) red[wave][m] = s[m];
        redc[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WAVES; ++w) {
#pragma unroll
            for (int m = 0; m < 4; ++m) s[m] += red[w][m];
            cnt += redc[w];
        }
    }
}

// leaf c of the tree: the counted impressions [c CHUNK, (c + 1) CHUNK); thread t adds impressions t, t + 256, ... of it in order
__global__ __launch_bounds__(THREADS) void reduce_chunks_kernel(const double* __restrict__ per_imp, const int* __restrict__ status, int n_imp,
                                                                 int n_chunks, double* __restrict__ part, long long* __restrict__ part_cnt) {
    __shared__ double red[WAVES][4];
    __shared__ long long redc[WAVES];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        long long cnt = 0;
#pragma unroll
        for (int k = 0; k < CHUNK / THREADS; ++k) {
            const long i = (long)c * CHUNK + k * THREADS + threadIdx.x;
            if (i < n_imp && status[i] == 0) {
                const double2 lo = *reinterpret_cast<const double2*>(per_imp + i * 4);
                const double2 hi = *reinterpret_cast<const double2*>(per_imp + i * 4 + 2);
                s[0] += lo.x;
                s[1] += lo.y;
                s[2] += hi.x;
                s[3] += hi.y;
                cnt += 1;
            }
        }
        block_sum5(s, cnt, red, redc);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int m = 0; m < 4; ++m) part[(long)c * 4 + m] = s[m];
            part_cnt[c] = cnt;
        }
    }
}

// the root: one workgroup; thread t adds chunk sums t, t + 256, ... in order
__global__ __launch_bounds__(THREADS) void reduce_final_kernel(const double* __restrict__ part, const long long* __restrict__ part_cnt,
                                                                int n_chunks, double* __restrict__ sums, long long* __restrict__ count) {
    __shared__ double red[WAVES][4];
    __shared__ long long redc[WAVES];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    long long cnt = 0;
    for (int c = threadIdx.x; c < n_chunks; c += THREADS) {
#pragma unroll
        for (int m = 0; m < 4; ++m) s[m] += part[(long)c * 4 + m];
        cnt += part_cnt[c];
    }
    block_sum5(s, cnt, red, redc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int m = 0; m < 4; ++m) sums[m] = s[m];
        *count = cnt;
    }
}

inline int64_t chunk_count(int64_t n_imp) { return (n_imp + CHUNK - 1) / CHUNK; }
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int64_t lime_rank_metrics_workspace(int32_t n_imp) {
    return n_imp > 0 ? chunk_count(n_imp) * (int64_t)(4 * sizeof(double) + sizeof(long long)) : 0;
}

extern "C" int lime_rank_metrics(const lime_rank_metrics_args* args, void* stream) {
    LIME_REQUIRE(args, LIME_ERR_BAD_ARG, "lime_rank_metrics: NULL args");
    const lime_rank_metrics_args& a = *args;
    LIME_REQUIRE(a.n_imp >= 0 && a.R >= 0 && a.R <= INT32_MAX, LIME_ERR_BAD_ARG, "lime_rank_metrics: bad dims (R %lld, n_imp %d)",
                 (long long)a.R, a.n_imp);
    LIME_REQUIRE(a.reserved == 0 && a.rank_blocks >= 0 && a.reduce_blocks >= 0, LIME_ERR_BAD_ARG,
                 "lime_rank_metrics: reserved must be 0, the block counts >= 0");
    LIME_REQUIRE(a.offsets && a.disc && a.sums && a.count, LIME_ERR_BAD_ARG, "lime_rank_metrics: NULL pointer");
    LIME_REQUIRE(a.n_imp == 0 || (a.per_imp && a.status), LIME_ERR_BAD_ARG, "lime_rank_metrics: NULL per_imp / status");
    LIME_REQUIRE(a.R == 0 || (a.scores && a.labels && a.ranks), LIME_ERR_BAD_ARG, "lime_rank_metrics: NULL scores / labels / ranks");
    LIME_REQUIRE(aligned(a.per_imp, 16) && aligned(a.sums, 8) && aligned(a.count, 8) && aligned(a.disc, 8) && aligned(a.workspace, 8),
                 LIME_ERR_BAD_ARG, "lime_rank_metrics: per_imp must be 16-byte, sums / count / disc / workspace 8-byte aligned");
    const int64_t n_chunks = chunk_count(a.n_imp);
    LIME_REQUIRE(a.n_imp == 0 || (a.workspace && a.workspace_bytes >= lime_rank_metrics_workspace(a.n_imp)), LIME_ERR_BAD_ARG,
                 "lime_rank_metrics: workspace of %lld bytes needed", (long long)lime_rank_metrics_workspace(a.n_imp));
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(a.workspace);
    long long* part_cnt = reinterpret_cast<long long*>(part + n_chunks * 4);
    if (a.n_imp > 0) {
        const int n_groups = (int)(((int64_t)a.n_imp + WAVES - 1) / WAVES);
        const int grid = a.rank_blocks > 0 ? min(a.rank_blocks, n_groups) : min(n_groups, 8192);
        hipLaunchKernelGGL(rank_metrics_kernel, dim3(grid), dim3(THREADS), 0, st, a.scores, a.labels, a.offsets, a.skip, a.disc, a.ranks,
                           a.per_imp, a.status, (int)a.R, a.n_imp, n_groups);
        int rc = lime_check_launch("lime_rank_metrics");
        if (rc != LIME_OK) return rc;
        const int rgrid = a.reduce_blocks > 0 ? (int)min((int64_t)a.reduce_blocks, n_chunks) : (int)min(n_chunks, (int64_t)1024);
        hipLaunchKernelGGL(reduce_chunks_kernel, dim3(rgrid), dim3(THREADS), 0, st, a.per_imp, a.status, a.n_imp, (int)n_chunks, part,
                           part_cnt);
        rc = lime_check_launch("lime_rank_metrics (chunk sums)");
        if (rc != LIME_OK) return rc;
    }
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(THREADS), 0, st, part, part_cnt, (int)n_chunks, a.sums, (long long*)a.count);
    return lime_check_launch("lime_rank_metrics (sums)");
}
