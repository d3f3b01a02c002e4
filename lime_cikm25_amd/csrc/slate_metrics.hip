// What a recommended slate is worth, on the device (util.evaluate_slates_on_device; recommend.slate_metrics states it on the host):
// per slate of k slots -- positions into the slate's own list (offsets) or into one shared pool -- nDCG@k, RR@k, hit@k and recall@k
// against the impression's labels, the intra-list distance 1 - mean pairwise cosine of the slots' similarity rows, the number of
// distinct keys (topics), the number of filled slots and the mean of a caller's value; then their sums over the counted slates.
//
// A slot is FILLED when its position lies inside the list (the pool) and the news id behind it inside [0, n); every other slot is
// empty: it earns nothing, reads nothing and still occupies its slot.
//
// Two forms, chosen by k alone: a wave per slate up to 16 slots (slate_metrics_wave_kernel, below), and for wider slates
// one workgroup of 256 threads per slate (grid-stride: any R).  Threads 0 .. k - 1 resolve the slots into LDS; all threads count the
// impression's positives over its rows; thread 0 sums the gains and the values in slot order (fp64, k <= 128 steps).  The cosines: as
// mmr_rows_f32.hip does, the 16 groups of 16 lanes own the rows g, g + 16, .. and form the inverse norms from global memory (16-byte
// loads, explicit fmaf in element order, lime_dev::row16_sum); then the NORMALISED rows go through LDS 64 floats at a time
// (128 rows x 68 floats: the padding puts the 16 rows a wave reads side by side on 16 different quads of banks) and thread (g, t) keeps
// the dot products of rows g + 16 i with rows t + 16 j, j >= i, in registers -- 36 accumulators at k = 128, one at k <= 16; only the
// pairs a < b are summed, in fp64: the thread's pairs in (i, j) order, the wave's shuffle tree, the four waves in wave order.
//
// No atomics, no workspace: a slate's row of per_slate is a function of the slate's own operands.  The sums are a second launch over
// per_slate / status: ONE workgroup per output (8 sums, 3 counts) adds all R slates in a fixed order -- thread t the slates t, t + 256,
// .., then the tree above --, so the number of workgroups only decides which workgroup owns which output.  These sums carry their
// rounding errors along (pair_add): a sum comes out as its terms' exact sum rounded once.
#include "dev_helpers.h"

namespace {

constexpr int SM_MAX = 128;                  // slots of a slate: the top-k kernels' k limit
constexpr int SM_CH = 64;                    // floats of every row in LDS at a time
constexpr int SM_LD = SM_CH + 4;             // the LDS row stride (see above)
constexpr int SM_T = SM_MAX / 16;            // rows of a 16-lane group, and row tiles of a thread
constexpr int SM_OUT = 11;                   // outputs of the second launch: sums [8], counts [3]
constexpr int SM_W = 16;                     // slots of a slate that one wave takes

template <typename T>
__device__ __forceinline__ T wave_total(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// the sum over the workgroup in every thread: the wave tree, then the waves in wave order (red: 4 entries; safe back to back)
template <typename T>
__device__ __forceinline__ T block_total(T v, T* red) {
    v = wave_total(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- what both forms share: the slate's rows, a slot, the impression's labels, the status, the slate's row of per_slate ------------
struct slot_t {
    int id, key;                             // the news id of a filled slot (-1: empty) and its key (-1: none)
    unsigned lab;
    float val;
};

// the rows a position of slate r counts in: [beg, beg + len) of the [P] arrays (offsets clamped into [0, P]: a malformed list cannot
// take a load out of bounds)
__device__ __forceinline__ void slate_rows(const lime_slate_metrics_args& a, long r, long& beg, long& len) {
    beg = 0;
    len = a.P;
    if (a.offsets) {
        beg = min(max((long)a.offsets[r], 0l), (long)a.P);
        len = min(max((long)a.offsets[r + 1], beg), (long)a.P) - beg;
    }
}

__device__ __forceinline__ slot_t read_slot(const lime_slate_metrics_args& a, long r, int j, long beg, long len) {
    slot_t s = {-1, -1, 0u, 0.f};
    if (j >= a.k) return s;
    const int pos = a.positions[r * a.ldp + j];
    if (pos < 0 || (long)pos >= len) return s;
    const long row = beg + pos;
    const int nid = a.news[row];
    if (nid < 0 || (long)nid >= a.n) return s;
    s.id = nid;
    if (a.labels) s.lab = a.labels[row];
    if (a.value) s.val = a.value[row];
    if (a.keys) {
        const int key = a.keys[nid];
        s.key = key >= 0 && key < a.n_keys ? key : -1;
    }
    return s;
}

// this thread's part (rows first, first + step, ..) of the impression's positives and of "a label outside {0, 1}"
__device__ __forceinline__ void count_labels(const lime_slate_metrics_args& a, long beg, long len, int first, int step, int& n_pos, int& bad) {
    n_pos = 0;
    bad = 0;
    if (a.labels)
        for (long i = first; i < len; i += step) {
            const unsigned l = a.labels[beg + i];
            n_pos += l != 0u;
            bad |= l > 1u;
        }
}

// The slate's status and row of per_slate from its sums (one thread).  dcg, hits, first: over the filled slots that hold a positive, in
// slot order; vsum: the values of the filled slots; m, distinct: the filled slots and their distinct keys.
__device__ __forceinline__ void write_slate(const lime_slate_metrics_args& a, long r, long len, int n_pos, int bad, double dcg, int hits,
                                            int first, double vsum, int m, int distinct, double pair_sum) {
    int st;
    if ((a.skip != nullptr && a.skip[r] != 0) || a.labels == nullptr || len == 0) st = 1;
    else if (bad) st = 3;
    else if (n_pos == 0 || (long)n_pos == len) st = 2;
    else st = 0;
    double ideal = 0.0;
    for (int p = 0; p < a.k && p < n_pos; ++p) ideal += a.disc[p];
    double* o = a.per_slate + r * 8;
    o[0] = st == 0 ? dcg / ideal : 0.0;
    o[1] = st == 0 && first >= 0 ? 1.0 / (double)(1 + first) : 0.0;
    o[2] = st == 0 && hits > 0 ? 1.0 : 0.0;
    o[3] = st == 0 ? (double)hits / (double)n_pos : 0.0;
    o[4] = a.table && m >= 2 ? 1.0 - pair_sum / (double)(m * (m - 1) / 2) : 0.0;
    o[5] = a.keys ? (double)distinct : 0.0;
    o[6] = (double)m;
    o[7] = a.value && m >= 1 ? vsum / (double)m : 0.0;
    a.status[r] = st;
}

template <bool VEC>
__global__ __launch_bounds__(256) void slate_metrics_kernel(const lime_slate_metrics_args a) {
    __shared__ float x[SM_MAX * SM_LD];
    __shared__ int id_of[SM_MAX];            // the news id of a filled slot, -1 of an empty one
    __shared__ int key_of[SM_MAX];           // its key, -1: none
    __shared__ float val_of[SM_MAX];
    __shared__ unsigned char lab_of[SM_MAX];
    __shared__ float inv[SM_MAX];
    __shared__ double red_f[4];
    __shared__ int red_i[4];
    const int tid = threadIdx.x, g = tid >> 4, t = tid & 15;
    const int k = a.k, na = (k + 15) >> 4, nq = a.E >> 2;

    for (long r = blockIdx.x; r < a.R; r += gridDim.x) {
        long beg, len;
        slate_rows(a, r, beg, len);
        if (tid < SM_MAX) {
            const slot_t s = read_slot(a, r, tid, beg, len);
            id_of[tid] = s.id;
            key_of[tid] = s.key;
            val_of[tid] = s.val;
            lab_of[tid] = (unsigned char)s.lab;
            inv[tid] = 0.f;
        }
        int n_pos, bad;                      // over the impression's rows
        count_labels(a, beg, len, tid, 256, n_pos, bad);
        n_pos = block_total(n_pos, red_i);   // (its barriers publish the slots)
        bad = block_total(bad, red_i);
        int mine = 0, fresh = 0;             // this thread's slot: filled; the first of its key
        if (tid < k && id_of[tid] >= 0) {
            mine = 1;
            const int key = key_of[tid];
            fresh = key >= 0;
            for (int j = 0; j < tid; ++j) fresh &= key_of[j] != key;
        }
        const int m = block_total(mine, red_i), distinct = block_total(fresh, red_i);

        double pair_sum = 0.0;
        if (a.table && m >= 2) {             // (workgroup-uniform)
            const float* rows[SM_T];
#pragma unroll
            for (int i = 0; i < SM_T; ++i) {
                const int id = i < na ? id_of[g + 16 * i] : -1;
                rows[i] = id >= 0 ? a.table + (long)id * a.ld : nullptr;
            }
            float ss[SM_T] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int q = t; q < nq; q += 16) {
#pragma unroll
                for (int i = 0; i < SM_T; ++i)
                    if (rows[i]) {
                        const f32x4 v = row_quad<VEC, long>(rows[i], (long)q, a.E);
                        ss[i] = fma_dot4(v, v, ss[i]);
                    }
            }
#pragma unroll
            for (int i = 0; i < SM_T; ++i) {
                const float s = lime_dev::row16_sum(ss[i]);
                if (t == 0 && rows[i]) inv[g + 16 * i] = s > 0.f ? 1.0f / sqrtf(s) : 0.f;
            }
            __syncthreads();
            float scale[SM_T];
#pragma unroll
            for (int i = 0; i < SM_T; ++i) scale[i] = i < na ? inv[g + 16 * i] : 0.f;

            float d[SM_T][SM_T];
#pragma unroll
            for (int i = 0; i < SM_T; ++i)
#pragma unroll
                for (int j = 0; j < SM_T; ++j) d[i][j] = 0.f;
            for (int q0 = 0; q0 < nq; q0 += SM_CH / 4) {
                if (q0) __syncthreads();     // the readers of the chunk before
#pragma unroll
                for (int i = 0; i < SM_T; ++i)
                    if (i < na) {
                        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                        if (rows[i] && q0 + t < nq) v = row_quad<VEC, long>(rows[i], (long)(q0 + t), a.E) * scale[i];
                        *reinterpret_cast<f32x4*>(&x[(g + 16 * i) * SM_LD + 4 * t]) = v;
                    }
                __syncthreads();
                const int cq = nq - q0 < SM_CH / 4 ? nq - q0 : SM_CH / 4;
                for (int q = 0; q < cq; ++q) {
                    f32x4 av[SM_T], bv[SM_T];
#pragma unroll
                    for (int i = 0; i < SM_T; ++i)
                        if (i < na) {
                            av[i] = *reinterpret_cast<const f32x4*>(&x[(g + 16 * i) * SM_LD + 4 * q]);
                            bv[i] = *reinterpret_cast<const f32x4*>(&x[(t + 16 * i) * SM_LD + 4 * q]);
                        }
#pragma unroll
                    for (int i = 0; i < SM_T; ++i)
#pragma unroll
                        for (int j = i; j < SM_T; ++j)
                            if (j < na) d[i][j] = fma_dot4(av[i], bv[j], d[i][j]);
                }
            }
            double s = 0.0;                  // (an empty slot's row is zeros: its pairs add 0)
#pragma unroll
            for (int i = 0; i < SM_T; ++i)
#pragma unroll
                for (int j = i; j < SM_T; ++j)
                    if (j < na && g + 16 * i < t + 16 * j && t + 16 * j < k) s += (double)d[i][j];
            pair_sum = block_total(s, red_f);
        }

        if (tid == 0) {                      // the gains and the values in slot order
            double dcg = 0.0, vsum = 0.0;
            int hits = 0, first = -1;
            for (int j = 0; j < k; ++j)
                if (id_of[j] >= 0) {
                    vsum += (double)val_of[j];
                    if (lab_of[j] != 0) {
                        dcg += a.disc[j];
                        hits += 1;
                        if (first < 0) first = j;
                    }
                }
            write_slate(a, r, len, n_pos, bad, dcg, hits, first, vsum, m, distinct, pair_sum);
        }
        __syncthreads();                     // the next slate overwrites the slots
    }
}

// k <= 16 (the slates a user sees): a WAVE per slate, four slates a workgroup and no workgroup barrier.  Lanes 0 .. k - 1 keep
// the slots in registers (every lane reads them by shuffle); the four 16-lane groups own the rows g, g + 4, g + 8, g + 12, their
// inverse norms stay in the group's registers, the normalised rows go through the wave's own 16 x 68 floats of LDS with the next
// chunk's global loads in flight, and lane (g, t) keeps the four dot products of rows g + 4 i with row t.  The same arithmetic in
// the same order as the workgroup form for every column but the pair sum's tree.
template <bool VEC>
__global__ __launch_bounds__(256) void slate_metrics_wave_kernel(const lime_slate_metrics_args a) {
    __shared__ float xs[4][SM_W * SM_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, t = lane & 15;
    const int k = a.k, nq = a.E >> 2;
    float* x = xs[wave];

    for (long r = (long)blockIdx.x * 4 + wave; r < a.R; r += (long)gridDim.x * 4) {
        long beg, len;
        slate_rows(a, r, beg, len);
        const slot_t slot = read_slot(a, r, lane, beg, len);           // this lane's slot (lanes >= k: empty)
        const int id = slot.id, key = slot.key;
        int n_pos, bad;
        count_labels(a, beg, len, lane, 64, n_pos, bad);
        n_pos = wave_total(n_pos);
        bad = wave_total(bad);
        int fresh = id >= 0 && key >= 0;
#pragma unroll
        for (int j = 0; j < SM_W - 1; ++j) {
            const int kj = __shfl(key, j);
            if (j < lane) fresh &= kj != key;
        }
        const int m = __popcll(__ballot(id >= 0)), distinct = __popcll(__ballot(fresh));

        double pair_sum = 0.0;
        if (a.table && m >= 2) {             // (wave-uniform)
            const float* rows[4];
            float scale[4], ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idi = __shfl(id, g + 4 * i);
                rows[i] = idi >= 0 ? a.table + (long)idi * a.ld : nullptr;
            }
            for (int q = t; q < nq; q += 16) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (rows[i]) {
                        const f32x4 v = row_quad<VEC, long>(rows[i], (long)q, a.E);
                        ss[i] = fma_dot4(v, v, ss[i]);
                    }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float s = lime_dev::row16_sum(ss[i]);
                scale[i] = rows[i] && s > 0.f ? 1.0f / sqrtf(s) : 0.f;
            }
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            f32x4 buf[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                buf[i] = rows[i] && t < nq ? row_quad<VEC, long>(rows[i], (long)t, a.E) : f32x4{0.f, 0.f, 0.f, 0.f};
            for (int q0 = 0; q0 < nq; q0 += SM_CH / 4) {
                wave_lds_fence();            // the reads of the chunk before
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(&x[(g + 4 * i) * SM_LD + 4 * t]) = buf[i] * scale[i];
                const int qn = q0 + SM_CH / 4 + t;       // the next chunk's loads fly while this one is used
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    buf[i] = rows[i] && qn < nq ? row_quad<VEC, long>(rows[i], (long)qn, a.E) : f32x4{0.f, 0.f, 0.f, 0.f};
                wave_lds_fence();
                const int cq = nq - q0 < SM_CH / 4 ? nq - q0 : SM_CH / 4;
                for (int q = 0; q < cq; ++q) {
                    const f32x4 bv = *reinterpret_cast<const f32x4*>(&x[t * SM_LD + 4 * q]);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        d[i] = fma_dot4(*reinterpret_cast<const f32x4*>(&x[(g + 4 * i) * SM_LD + 4 * q]), bv, d[i]);
                }
            }
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (g + 4 * i < t && t < k) s += (double)d[i];
            pair_sum = wave_total(s);
        }

        // every lane walks the slots in slot order; lane 0 writes
        double dcg = 0.0, vsum = 0.0;
        int hits = 0, first = -1;
        for (int j = 0; j < k; ++j) {
            const int idj = __shfl(id, j);
            const unsigned lj = __shfl(slot.lab, j);
            const float vj = __shfl(slot.val, j);
            if (idj >= 0) {
                vsum += (double)vj;
                if (lj != 0u) {
                    dcg += a.disc[j];
                    hits += 1;
                    if (first < 0) first = j;
                }
            }
        }
        if (lane == 0) write_slate(a, r, len, n_pos, bad, dcg, hits, first, vsum, m, distinct, pair_sum);
    }
}

// A sum of many fp64 terms kept as an unevaluated pair hi + lo (lo: the rounding errors of the additions, by Knuth's two-sum): a plain
// fp64 sum of R terms near 1 is off by up to an ulp of R per addition, which is more than R 2^-53 once R is a few dozen; the pair's
// hi + lo is the sum of the terms rounded once, whatever R.
struct pair_t {
    double hi, lo;
};
__device__ __forceinline__ pair_t pair_add(pair_t a, pair_t b) {
    const double s = a.hi + b.hi, t = s - a.hi;
    const double e = ((a.hi - (s - t)) + (b.hi - t)) + (a.lo + b.lo);
    const double hi = s + e;
    return pair_t{hi, e - (hi - s)};
}

// output o of the sums: o < 8 column o of per_slate over its counted set, o >= 8 the size of counted set o - 8
__global__ __launch_bounds__(256) void slate_sums_kernel(const double* __restrict__ per_slate, const int* __restrict__ status,
                                                          const unsigned char* __restrict__ skip, long R, double* __restrict__ sums,
                                                          long long* __restrict__ counts) {
    __shared__ pair_t red_f[4];
    __shared__ long long red_n[4];
    for (int o = blockIdx.x; o < SM_OUT; o += gridDim.x) {
        const int set = o >= 8 ? o - 8 : (o < 4 ? 0 : (o == 4 ? 1 : 2));
        pair_t s = {0.0, 0.0};
        long long c = 0;
        for (long r = threadIdx.x; r < R; r += 256) {
            bool in;
            if (set == 0) in = status[r] == 0;
            else in = !(skip != nullptr && skip[r] != 0) && per_slate[r * 8 + 6] >= (set == 1 ? 2.0 : 1.0);
            if (in) {
                c += 1;
                if (o < 8) s = pair_add(s, pair_t{per_slate[r * 8 + o], 0.0});
            }
        }
        if (o < 8) {                             // the wave's shuffle tree, then the waves in wave order
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) s = pair_add(s, pair_t{__shfl_xor(s.hi, off), __shfl_xor(s.lo, off)});
            __syncthreads();
            if ((threadIdx.x & 63) == 0) red_f[threadIdx.x >> 6] = s;
            __syncthreads();
            if (threadIdx.x == 0) {
                s = pair_add(pair_add(pair_add(red_f[0], red_f[1]), red_f[2]), red_f[3]);
                sums[o] = s.hi + s.lo;
            }
        } else {
            c = block_total(c, red_n);
            if (threadIdx.x == 0) counts[o - 8] = c;
        }
    }
}

}  // namespace

extern "C" int lime_slate_metrics_f32(const lime_slate_metrics_args* args, void* stream) {
    LIME_REQUIRE(args, LIME_ERR_BAD_ARG, "lime_slate_metrics_f32: NULL args");
    const lime_slate_metrics_args& a = *args;
    LIME_REQUIRE(a.positions && a.news && a.disc && a.per_slate && a.status && a.sums && a.counts, LIME_ERR_BAD_ARG,
                 "lime_slate_metrics_f32: NULL pointer (positions, news, disc, per_slate, status, sums and counts are required)");
    LIME_REQUIRE(a.labels == nullptr || a.offsets != nullptr, LIME_ERR_BAD_ARG,
                 "lime_slate_metrics_f32: labels need offsets (a pool has no impression to count the positives of)");
    LIME_REQUIRE(a.R >= 0 && a.P >= 0 && a.k >= 1 && a.k <= a.ldp && a.E >= 0 && a.ld >= a.E && a.n >= 1, LIME_ERR_BAD_ARG,
                 "lime_slate_metrics_f32: bad dims (R %lld, P %lld, k %d, ldp %lld, E %d, ld %lld, n %lld): R, P >= 0, 1 <= k <= ldp, "
                 "0 <= E <= ld, n >= 1",
                 (long long)a.R, (long long)a.P, a.k, (long long)a.ldp, a.E, (long long)a.ld, (long long)a.n);
    LIME_REQUIRE((a.table == nullptr || a.E >= 1) && (a.keys == nullptr || a.n_keys >= 1), LIME_ERR_BAD_ARG,
                 "lime_slate_metrics_f32: a table needs E >= 1, keys need n_keys >= 1 (E %d, n_keys %d)", a.E, a.n_keys);
    LIME_REQUIRE(a.reserved == 0 && a.reduce_blocks >= 0, LIME_ERR_BAD_ARG, "lime_slate_metrics_f32: reserved must be 0, reduce_blocks >= 0");
    LIME_REQUIRE(a.k <= SM_MAX && a.E % 4 == 0, LIME_ERR_UNSUPPORTED, "lime_slate_metrics_f32: k %d, E %d outside k <= %d, E %% 4 == 0", a.k,
                 a.E, SM_MAX);
    hipStream_t st = (hipStream_t)stream;
    if (a.R == 0) {                          // nothing to launch: zero sums and counts
        const hipError_t e0 = hipMemsetAsync(a.sums, 0, 8 * sizeof(double), st), e1 = hipMemsetAsync(a.counts, 0, 3 * sizeof(int64_t), st);
        LIME_REQUIRE(e0 == hipSuccess && e1 == hipSuccess, LIME_ERR_LAUNCH, "lime_slate_metrics_f32: cannot clear sums / counts");
        return LIME_OK;
    }
    const bool vec = lime_al16(a.table, (long)a.ld);
    if (a.k <= SM_W) {                       // a wave per slate, four a workgroup
        const unsigned grid = lime_grid_cap((long)a.R, 4, 16384);
        if (vec) hipLaunchKernelGGL(slate_metrics_wave_kernel<true>, dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(slate_metrics_wave_kernel<false>, dim3(grid), dim3(256), 0, st, a);
    } else {
        const unsigned grid = lime_grid_cap((long)a.R, 1, 16384);
        if (vec) hipLaunchKernelGGL(slate_metrics_kernel<true>, dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(slate_metrics_kernel<false>, dim3(grid), dim3(256), 0, st, a);
    }
    const int rc = lime_check_launch("lime_slate_metrics_f32");
    if (rc != LIME_OK) return rc;
    const int rgrid = a.reduce_blocks > 0 ? min(a.reduce_blocks, SM_OUT) : SM_OUT;
    hipLaunchKernelGGL(slate_sums_kernel, dim3(rgrid), dim3(256), 0, st, (const double*)a.per_slate, (const int*)a.status, a.skip, (long)a.R,
                       a.sums, (long long*)a.counts);
    return lime_check_launch("lime_slate_metrics_f32 (sums)");
}
