// Calibrated slates (Steck, RecSys 2018): a slate whose topic mix follows the reader's own, on the device (Model.recommend* with
// calibrate_lambda; recommend.calibrated_select / recommend.slate_miscalibration state both entries on the host).
//
// The TARGET of a row is the topic distribution of its history: hist_keys[h] is the group of history slot h (a key outside
// [0, n_keys) is no click), hist_weight[h] its weight (NULL: 1 each; a weight that is not finite or not > 0 removes the slot).  W is
// the weight sum over the live slots, p[g] the weight sum of the live slots of group g divided by W -- both summed in slot order --,
// and a row whose W is 0 (or not finite) has no target.  The SUPPORT is the groups with a live slot, in the order of their first slot.
//
// lime_calibrate_rows_f32: the greedy selection over a shortlist of M <= 128 entries, best first (scores[j], ids[j] the news id).  Dead
// entries and rel[j] are lime_mmr_rows_f32's.  In round t (t entries taken, c[g] of them in group g, T = t + 1) entry j of group g has
//     gain[j] = p[g] (ln q(c[g] + 1) - ln q(c[g])) / ln(1 / alpha),   q(c) = (1 - alpha) c / T + alpha p[g]
// (0 without a target, without a group, or for a group outside the support), and the round takes the live, untaken j of the largest
// v[j] = lam rel[j] + (1 - lam) gain[j], the lower rank on equal v.  Adding j changes only its own group's term of
// KL(p || q) at slate size T, so the largest gain is the smallest KL: Steck's greedy in O(M) a round.
//
// lime_slate_miscalibration: sum over the support of p[g] ln(p[g] / ((1 - alpha) c[g] / F + alpha p[g])) of a finished slate, c
// counting its F filled slots (lime_slate_metrics_f32's rule), in fp64.
//
// The form: a WAVE per row (per slate), four to a 256-thread workgroup, no workgroup barrier, grid-stride over any R -- a row is M <= 128
// entries, at most H <= 128 groups and k rounds: a workgroup per row would leave three waves in four idle.  Lane l owns entries
// (slots) l and l + 64, history slots l and l + 64 and support groups l and l + 64.  build_support (shared by both entries, fp32 or
// fp64) leaves the support's keys and p in the wave's own LDS; per round the lanes form the gain ONCE PER SUPPORT GROUP (logf, not
// the fast intrinsic) into LDS, every entry reads its group's, a wave reduction on (v, rank) picks, and the owner of the winner's group
// bumps its count.  Two entries of one group with equal score bits therefore carry the same v bits, and rank decides between them.
// Fixed-order sums, no atomics, no workspace: a row's result is a function of its own operands alone.  lam == 1 (and a row without a
// target) reads neither keys nor history.  LDS: 2.5 KB a wave (fp32), 3 KB (fp64).
#include "dev_helpers.h"

namespace {

constexpr int CAL_MAX = 128;             // entries of a shortlist, slots of a slate, slots of a history
constexpr int CAL_MAX_KEYS = 8192;       // the groups of a corpus: the quota kernels' limit

// the wave's own LDS: the history while the support is built (afterwards hk / hw are free for the caller), then the support
template <typename T>
struct support_lds {
    int hk[CAL_MAX];                     // the key of a live history slot, -1 of every other
    T hw[CAL_MAX];                       // its weight, 0 of every other
    int skey[CAL_MAX];                   // the key of support group s
    T sp[CAL_MAX];                       // its p
};

// The support of one history row (hkeys / hweight: its H slots; hweight may be NULL) into `s`, by one wave -> the number of support groups, 0 when the
// row has no target.  Every lane walks the H slots in slot order, so a group's sum and W are fixed-order sums (a dead slot adds an
// exact 0).
template <typename T>
__device__ __forceinline__ int build_support(support_lds<T>& s, const int* __restrict__ hkeys, const float* __restrict__ hweight, int H,
                                             int n_keys, int lane) {
    int key[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int h = lane + 64 * i;
        int kk = -1;
        float w = 0.f;
        if (h < H) {
            kk = hkeys[h];
            w = hweight ? hweight[h] : 1.0f;
        }
        const bool live = kk >= 0 && kk < n_keys && __builtin_isfinite(w) && w > 0.f;
        key[i] = live ? kk : -1;
        s.hk[h] = key[i];
        s.hw[h] = live ? (T)w : (T)0;
    }
    wave_lds_fence();
    T sum[2] = {(T)0, (T)0}, W = (T)0;
    bool earlier[2] = {false, false};
    for (int h = 0; h < H; ++h) {
        const int kk = s.hk[h];
        const T w = s.hw[h];
        W += w;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool same = kk == key[i];
            sum[i] += same ? w : (T)0;
            earlier[i] = earlier[i] || (same && h < lane + 64 * i);
        }
    }
    const bool first0 = key[0] >= 0 && !earlier[0], first1 = key[1] >= 0 && !earlier[1];
    const unsigned long long b0 = __ballot(first0), b1 = __ballot(first1), below = (1ull << lane) - 1ull;
    const bool target = W > (T)0 && __builtin_isfinite(W);
    if (target) {
        if (first0) {
            const int at = __popcll(b0 & below);
            s.skey[at] = key[0];
            s.sp[at] = sum[0] / W;
        }
        if (first1) {
            const int at = __popcll(b0) + __popcll(b1 & below);
            s.skey[at] = key[1];
            s.sp[at] = sum[1] / W;
        }
    }
    wave_lds_fence();
    return target ? __popcll(b0) + __popcll(b1) : 0;
}

// the support group of `key` among the first S (-1: none; key < 0 is never in the support)
template <typename T>
__device__ __forceinline__ void find_groups(const support_lds<T>& s, int S, const int (&key)[2], int (&at)[2]) {
    at[0] = at[1] = -1;
    for (int g = 0; g < S; ++g) {
        const int kk = s.skey[g];
        if (kk == key[0]) at[0] = g;
        if (kk == key[1]) at[1] = g;
    }
}

__global__ __launch_bounds__(256) void calibrate_rows_kernel(const float* __restrict__ scores, const int* __restrict__ ids, long R, int M,
                                                              const int* __restrict__ keys, long n, int n_keys,
                                                              const int* __restrict__ hist_keys, const float* __restrict__ hist_weight,
                                                              long hist_rows, int H, float lam, float alpha, float inv_ln, int k,
                                                              int* __restrict__ picks) {
    __shared__ support_lds<float> lds[4];
    __shared__ float gains[4][CAL_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    support_lds<float>& s = lds[wave];
    float* gain = gains[wave];
    const float oml = 1.0f - lam, oma = 1.0f - alpha;
    const int j0 = lane, j1 = lane + 64;

    for (long row = (long)blockIdx.x * 4 + wave; row < R; row += (long)gridDim.x * 4) {
        const float* sr = scores + row * M;
        const int* idr = ids + row * M;
        int* out = picks + row * k;
        // the lane's two entries, the row's first / last live entry, lam rel (lime_mmr_rows_f32's, to the letter)
        const float s0 = j0 < M ? sr[j0] : 0.f, s1 = j1 < M ? sr[j1] : 0.f;
        const int i0 = j0 < M ? idr[j0] : -1, i1 = j1 < M ? idr[j1] : -1;
        const bool live0 = i0 >= 0 && (long)i0 < n && __builtin_isfinite(s0);
        const bool live1 = i1 >= 0 && (long)i1 < n && __builtin_isfinite(s1);
        const unsigned long long m0 = __ballot(live0), m1 = __ballot(live1);
        float a0 = 0.f, a1 = 0.f;
        if (m0 | m1) {                                            // (wave-uniform)
            const int first = m0 ? __ffsll((long long)m0) - 1 : 64 + __ffsll((long long)m1) - 1;
            const int last = m1 ? 127 - __clzll((long long)m1) : 63 - __clzll((long long)m0);
            const float lo0 = __shfl(s0, first & 63), lo1 = __shfl(s1, first & 63);
            const float hi0 = __shfl(s0, last & 63), hi1 = __shfl(s1, last & 63);
            const float s_first = first < 64 ? lo0 : lo1, s_last = last < 64 ? hi0 : hi1;
            const float span = s_first - s_last;
            if (span != 0.f) {
                a0 = live0 ? lam * ((s0 - s_last) / span) : 0.f;
                a1 = live1 ? lam * ((s1 - s_last) / span) : 0.f;
            }
        }
        a0 = a0 == a0 ? a0 : -3.402823466e38f;                    // (a span that overflowed: a NaN ranks as the lowest number)
        a1 = a1 == a1 ? a1 : -3.402823466e38f;
        bool open0 = live0, open1 = live1;                        // live and not taken

        // the target, and the support group of the lane's entries -- neither keys nor history are read when the gain has no weight
        int S = 0, at[2] = {-1, -1};
        if (oml != 0.f && H > 0 && (m0 | m1)) {
            S = build_support(s, hist_keys + (row % hist_rows) * H, hist_weight ? hist_weight + (row % hist_rows) * H : nullptr, H, n_keys,
                              lane);
            if (S > 0) {
                int e[2] = {live0 ? keys[i0] : -1, live1 ? keys[i1] : -1};
                e[0] = e[0] < n_keys ? e[0] : -1;
                e[1] = e[1] < n_keys ? e[1] : -1;
                find_groups(s, S, e, at);
            }
        }
        const float p0 = lane < S ? s.sp[lane] : 0.f, p1 = lane + 64 < S ? s.sp[lane + 64] : 0.f;     // the lane's two groups
        int c0 = 0, c1 = 0;

        int r = 0;
        for (; r < k; ++r) {
            float v0 = a0, v1 = a1;
            if (S > 0) {                                          // (wave-uniform) the gain, once per support group
                const float fT = (float)(r + 1);
                wave_lds_fence();                                 // the reads of the round before
                if (lane < S)
                    gain[lane] = p0 > 0.f ? p0 * (logf(oma * ((float)(c0 + 1) / fT) + alpha * p0) - logf(oma * ((float)c0 / fT) + alpha * p0)) * inv_ln
                                          : 0.f;
                if (lane + 64 < S)
                    gain[lane + 64] = p1 > 0.f ? p1 * (logf(oma * ((float)(c1 + 1) / fT) + alpha * p1) - logf(oma * ((float)c1 / fT) + alpha * p1)) * inv_ln
                                               : 0.f;
                wave_lds_fence();
                v0 = fmaf(oml, at[0] >= 0 ? gain[at[0]] : 0.f, a0);
                v1 = fmaf(oml, at[1] >= 0 ? gain[at[1]] : 0.f, a1);
            }
            const best_pick b0 = open0 ? best_pick{v0, j0} : best_pick{-INFINITY, 0x7FFFFFFF};
            const best_pick b1 = open1 ? best_pick{v1, j1} : best_pick{-INFINITY, 0x7FFFFFFF};
            const best_pick best = wave_best_pick(better_pick(b0, b1));
            if (best.j == 0x7FFFFFFF) break;                      // no live entry left
            if (lane == 0) out[r] = best.j;
            open0 = open0 && j0 != best.j;
            open1 = open1 && j1 != best.j;
            const int w0 = __shfl(at[0], best.j & 63), w1 = __shfl(at[1], best.j & 63);
            const int won = best.j < 64 ? w0 : w1;                // the winner's support group (-1: none)
            c0 += won == lane;
            c1 += won == lane + 64;
        }
        for (int j = r + lane; j < k; j += 64) out[j] = -1;
    }
}

struct miscal_args {
    const int* positions;
    const long long* offsets;
    const int* news;
    const int* keys;
    const int* hist_keys;
    const float* hist_weight;
    double* value;
    int* status;
    long R, P, ldp, n, hist_rows;
    int k, n_keys, H;
    double alpha;
};

__global__ __launch_bounds__(256) void slate_miscalibration_kernel(const miscal_args a) {
    __shared__ support_lds<double> lds[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    support_lds<double>& s = lds[wave];

    for (long r = (long)blockIdx.x * 4 + wave; r < a.R; r += (long)gridDim.x * 4) {
        // the slate's rows (offsets clamped into [0, P]) and the key of the lane's two slots (-1: empty, or no key)
        long beg = 0, len = a.P;
        if (a.offsets) {
            beg = min(max((long)a.offsets[r], 0l), a.P);
            len = min(max((long)a.offsets[r + 1], beg), a.P) - beg;
        }
        int key[2];
        bool filled[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int j = lane + 64 * i;
            key[i] = -1;
            filled[i] = false;
            if (j < a.k) {
                const int pos = a.positions[r * a.ldp + j];
                if (pos >= 0 && (long)pos < len) {
                    const int nid = a.news[beg + pos];
                    if (nid >= 0 && (long)nid < a.n) {
                        filled[i] = true;
                        const int kk = a.keys[nid];
                        key[i] = kk >= 0 && kk < a.n_keys ? kk : -1;
                    }
                }
            }
        }
        const int F = __popcll(__ballot(filled[0])) + __popcll(__ballot(filled[1]));
        const long hr = r % a.hist_rows;
        const int S = a.H > 0 ? build_support(s, a.hist_keys + hr * a.H, a.hist_weight ? a.hist_weight + hr * a.H : nullptr, a.H, a.n_keys, lane)
                              : 0;
        double total = 0.0;
        if (S > 0 && F > 0) {                                     // (wave-uniform)
            s.hk[lane] = key[0];                                  // the history is done with: the slots' keys take its place
            s.hk[lane + 64] = key[1];
            wave_lds_fence();
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int g = lane + 64 * i;
                if (g < S) {
                    const int kk = s.skey[g];
                    int c = 0;
                    for (int j = 0; j < a.k; ++j) c += s.hk[j] == kk;
                    const double p = s.sp[g];
                    s.hw[g] = p > 0.0 ? p * log(p / ((1.0 - a.alpha) * ((double)c / (double)F) + a.alpha * p)) : 0.0;
                }
            }
            wave_lds_fence();
            for (int g = 0; g < S; ++g) total += s.hw[g];         // support order, one addition after the other
        }
        if (lane == 0) {
            a.value[r] = total;
            a.status[r] = S == 0 ? 1 : (F == 0 ? 2 : 0);
        }
        wave_lds_fence();                                         // the next slate overwrites the LDS
    }
}

}  // namespace

extern "C" int lime_calibrate_rows_f32(const float* scores, const int32_t* ids, int64_t R, int32_t M, const int32_t* keys, int64_t n,
                                       int32_t n_keys, const int32_t* hist_keys, const float* hist_weight, int64_t hist_rows, int32_t H,
                                       float lam, float alpha, int32_t k, int32_t* picks, void* stream) {
    LIME_REQUIRE(scores && ids && keys && hist_keys && picks, LIME_ERR_BAD_ARG,
                 "lime_calibrate_rows_f32: NULL pointer (only hist_weight may be NULL)");
    LIME_REQUIRE(R >= 0 && M >= 1 && k >= 1 && k <= M && n >= 1 && n_keys >= 1 && H >= 0 && hist_rows >= 0 && (H == 0 || hist_rows >= 1),
                 LIME_ERR_BAD_ARG,
                 "lime_calibrate_rows_f32: bad dims (R %lld, M %d, k %d, n %lld, n_keys %d, hist_rows %lld, H %d): R >= 0, 1 <= k <= M, "
                 "n >= 1, n_keys >= 1, H >= 0, hist_rows >= 1 with H > 0",
                 (long long)R, M, k, (long long)n, n_keys, (long long)hist_rows, H);
    LIME_REQUIRE(lam >= 0.f && lam <= 1.f, LIME_ERR_BAD_ARG, "lime_calibrate_rows_f32: lam %g outside [0, 1]", (double)lam);
    LIME_REQUIRE(alpha > 0.f && alpha < 1.f, LIME_ERR_BAD_ARG, "lime_calibrate_rows_f32: alpha %g outside (0, 1)", (double)alpha);
    LIME_REQUIRE(M <= CAL_MAX && H <= CAL_MAX && n_keys <= CAL_MAX_KEYS, LIME_ERR_UNSUPPORTED,
                 "lime_calibrate_rows_f32: M %d, H %d, n_keys %d outside M <= %d, H <= %d, n_keys <= %d", M, H, n_keys, CAL_MAX, CAL_MAX,
                 CAL_MAX_KEYS);
    if (R == 0) return LIME_OK;
    const float inv_ln = (float)(1.0 / log(1.0 / (double)alpha));
    hipLaunchKernelGGL(calibrate_rows_kernel, dim3(lime_grid_cap((long)R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, scores,
                       (const int*)ids, (long)R, (int)M, (const int*)keys, (long)n, (int)n_keys, (const int*)hist_keys, hist_weight,
                       (long)(hist_rows > 0 ? hist_rows : 1), (int)H, lam, alpha, inv_ln, (int)k, (int*)picks);
    return lime_check_launch("lime_calibrate_rows_f32");
}

extern "C" int lime_slate_miscalibration(const int32_t* positions, int64_t R, int64_t ldp, int32_t k, const int64_t* offsets,
                                         const int32_t* news, int64_t P, const int32_t* keys, int64_t n, int32_t n_keys,
                                         const int32_t* hist_keys, const float* hist_weight, int64_t hist_rows, int32_t H, float alpha,
                                         double* value, int32_t* status, void* stream) {
    LIME_REQUIRE(positions && news && keys && hist_keys && value && status, LIME_ERR_BAD_ARG,
                 "lime_slate_miscalibration: NULL pointer (only offsets and hist_weight may be NULL)");
    LIME_REQUIRE(R >= 0 && P >= 0 && k >= 1 && k <= ldp && n >= 1 && n_keys >= 1 && H >= 0 && hist_rows >= 0 && (H == 0 || hist_rows >= 1),
                 LIME_ERR_BAD_ARG,
                 "lime_slate_miscalibration: bad dims (R %lld, P %lld, k %d, ldp %lld, n %lld, n_keys %d, hist_rows %lld, H %d): R, P >= 0, "
                 "1 <= k <= ldp, n >= 1, n_keys >= 1, H >= 0, hist_rows >= 1 with H > 0",
                 (long long)R, (long long)P, k, (long long)ldp, (long long)n, n_keys, (long long)hist_rows, H);
    LIME_REQUIRE(alpha > 0.f && alpha < 1.f, LIME_ERR_BAD_ARG, "lime_slate_miscalibration: alpha %g outside (0, 1)", (double)alpha);
    LIME_REQUIRE(k <= CAL_MAX && H <= CAL_MAX && n_keys <= CAL_MAX_KEYS, LIME_ERR_UNSUPPORTED,
                 "lime_slate_miscalibration: k %d, H %d, n_keys %d outside k <= %d, H <= %d, n_keys <= %d", k, H, n_keys, CAL_MAX, CAL_MAX,
                 CAL_MAX_KEYS);
    if (R == 0) return LIME_OK;
    miscal_args a;
    a.positions = (const int*)positions;
    a.offsets = (const long long*)offsets;
    a.news = (const int*)news;
    a.keys = (const int*)keys;
    a.hist_keys = (const int*)hist_keys;
    a.hist_weight = hist_weight;
    a.value = value;
    a.status = (int*)status;
    a.R = (long)R, a.P = (long)P, a.ldp = (long)ldp, a.n = (long)n, a.hist_rows = (long)(hist_rows > 0 ? hist_rows : 1);
    a.k = k, a.n_keys = n_keys, a.H = H;
    a.alpha = (double)alpha;                                      // the fp32 number the selection reads, widened
    hipLaunchKernelGGL(slate_miscalibration_kernel, dim3(lime_grid_cap((long)R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, a);
    return lime_check_launch("lime_slate_miscalibration");
}
