// History-vs-candidate attention + dot-product match + remaining-lifetime weight for GROUPS of pairs that share one refined history
// (Model.score_pool: a group is one (user, candidate topic), its pairs are the pool's news of that topic).  Per pair p of group i:
//     s[h]   = kp[i, h, :] . qp[p, :] * scale            alpha = softmax_h(s)
//     m[h]   = g[i, h, :] . cand[p, :]
//     logits[p] = (sum_h alpha[h] m[h]) * w(remaining[p])
// -- the function of lime_interest_match_f32 with (sum_h alpha[h] g[h]) . cand re-associated as sum_h alpha[h] (g[h] . cand), which
// turns a pair into two columns of the products  KP . QP_tile^T  and  G . CAND_tile^T  [16 T x 64] on the matrix cores.
//
// A workgroup (four waves) takes 64-pair tiles of one group, a wave 16 pairs of the tile.  The shared operand (kp, then g) goes
// through LDS in chunks of 16 columns, as the swizzled [row][64-byte] image of dev_helpers.h: H padded to 16 T rows with zeros in LDS
// only, chunk c + 1 on its way from global memory into registers while chunk c is multiplied, two buffers and one barrier per chunk.
// The pair's own operand (qp, then cand) is read by its wave straight from global memory, 16 bytes per lane.  Columns behind A / D
// are zeros in registers; no load goes past a row.
// Exact fp32: v_mfma_f32_16x16x4_f32 (mfma16).  A lane's four loaded columns go to four accumulators; every FLUSH chunks the four are
// added as (c0 + c1) + (c2 + c3) into a compensated running sum and start again from zero.  The softmax and the weighted sum over h
// run on the results (h over the lane's 4 T registers in order, then the two butterfly steps over the lanes 16 and 32 apart).  Every sum has
// a fixed order that depends on H, A and D alone: a pair's bits depend neither on P, G, the group's position, the pair's place in its
// tile nor the grid.  No atomics.
//
// The indexed form (lime_grouped_match_indexed_f32): the pair's own operands are rows of two TABLES, qp [n, A] and cand [n, D], and
// pair p reads row index[p] of both -- a candidate whose representation depends on the news alone is not copied once per (user,
// candidate) pair.  Nothing else changes: only the row that tile_product reads as Y differs, so a pair's bits are those of the plain
// form on the gathered rows.  An index outside [0, n) is clamped into it (as the offsets are clamped): a bad plan reads in range.
#include "dev_helpers.h"

namespace {

using namespace lime_dev;

constexpr int PAIRS = 64;            // pairs of a workgroup tile: 16 per wave
constexpr int CHUNK = 16;            // columns of an LDS chunk: one 64-byte row of the swizzled image
constexpr int FLUSH = 2;             // chunks between two flushes of the MFMA accumulators into the compensated sum

// One [16 T x 16] tile product per wave over K columns: out[t][r] = X[16 t + 4 (lane >> 4) + r, :K] . Y[pair of lane & 15, :K].
// X: the group's rows x0 .. x0 + H - 1 of a dense [*, K] matrix (shared by the workgroup, through `img`); Y: row `yrow` of a dense
// [*, K] matrix, or nothing (zeros) when `ylive` is false.  Ends with a barrier: `img` is free again when it returns.
template <int T>
__device__ __forceinline__ void tile_product(const float* __restrict__ X, long x0, int H, const float* __restrict__ Y, long yrow, bool ylive,
                                             int K, float* img, f32x4 (&out)[T]) {
    constexpr int NL = T < 4 ? 1 : T / 4;                    // 16-byte pieces of a chunk per thread: 16 T rows x 4 segments / 256
    const int lane = threadIdx.x & 63;
    const int ar = lane & 15, as = lane >> 4;                // this lane's row of a 16-row tile and its 16-byte segment
    const int n_chunk = (K + CHUNK - 1) / CHUNK;
    f32x4 xs[NL], ys;
    f32x4 acc[T][4];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto fetch = [&](int c) {
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int piece = (int)threadIdx.x + 256 * j;
            const int row = piece >> 2, col = c * CHUNK + 4 * (piece & 3);
            xs[j] = (row < H && col < K) ? *reinterpret_cast<const f32x4*>(X + (x0 + row) * K + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int col = c * CHUNK + 4 * as;
        ys = (ylive && col < K) ? *reinterpret_cast<const f32x4*>(Y + yrow * K + col) : f32x4{0.f, 0.f, 0.f, 0.f};
    };

    // The accumulators are emptied every FLUSH chunks into a compensated sum (tot + comp, Knuth's two-sum): one fmaf chain over all
    // K / 4 of a lane's column groups loses about three times what lime_interest_match_f32's shuffle trees lose at K = 400; chains
    // of 4 FLUSH products with an exactly corrected running sum behind them lose less than those trees.
    f32x4 tot[T], comp[T];
#pragma unroll
    for (int t = 0; t < T; ++t) tot[t] = comp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto flush = [&]() {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const f32x4 v = (acc[t][0] + acc[t][1]) + (acc[t][2] + acc[t][3]);
            const f32x4 s = tot[t] + v;
            const f32x4 b = s - tot[t];
            comp[t] += (tot[t] - (s - b)) + (v - b);
            tot[t] = s;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };

    fetch(0);
    for (int c = 0; c < n_chunk; ++c) {
        float* buf = img + (c & 1) * (16 * T * CHUNK);
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int piece = (int)threadIdx.x + 256 * j;
            const int row = piece >> 2, seg = piece & 3;
            if (row < 16 * T) *reinterpret_cast<f32x4*>(buf + row * CHUNK + 4 * (seg ^ swz4((row >> 2) & 3))) = xs[j];
        }
        const f32x4 b = ys;
        lds_barrier();                                       // (two buffers: the chunk written here was last read two barriers ago)
        if (c + 1 < n_chunk) fetch(c + 1);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int row = 16 * t + ar;
            const f32x4 a = *reinterpret_cast<const f32x4*>(buf + row * CHUNK + 4 * (as ^ swz4((row >> 2) & 3)));
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][i] = mfma16(a[i], b[i], acc[t][i]);
        }
        if ((c + 1) % FLUSH == 0 || c + 1 == n_chunk) flush();
    }
#pragma unroll
    for (int t = 0; t < T; ++t) out[t] = tot[t] + comp[t];
    lds_barrier();
}

// INDEXED: qp / cand are tables of n rows and pair p reads row index[p] (clamped into [0, n)) of both; else row p (index unread).
template <int T, bool INDEXED>
__global__ __launch_bounds__(256) void grouped_match_kernel(const float* __restrict__ kp, const float* __restrict__ g,
                                                             const float* __restrict__ qp, const float* __restrict__ cand,
                                                             const float* __restrict__ remaining, const long* __restrict__ offsets,
                                                             const int* __restrict__ index, int n, float* __restrict__ logits, long P, int H,
                                                             int A, int D, float scale, float alpha_s, float beta_s, int use_weight,
                                                             int use_penalty) {
    __shared__ __attribute__((aligned(16))) float img[2 * 16 * T * CHUNK];
    const long grp = blockIdx.x;
    long lo = offsets[grp], hi = offsets[grp + 1];
    lo = lo < 0 ? 0 : (lo > P ? P : lo);                     // every offset clamped into [0, P]: a bad plan reads and writes in range
    hi = hi < lo ? lo : (hi > P ? P : hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n_tile = (hi - lo + PAIRS - 1) / PAIRS;
    for (long tile = blockIdx.y; tile < n_tile; tile += gridDim.y) {         // (workgroup-uniform: the barriers inside stay whole)
        const long p = lo + tile * PAIRS + 16 * wave + (lane & 15);
        const bool live = p < hi;
        long y = p;                                          // the pair's row of qp and cand
        if constexpr (INDEXED) {
            const int i = live ? index[p] : 0;
            y = i < 0 ? 0 : (i >= n ? n - 1 : i);
        }
        f32x4 s[T], m[T];
        tile_product<T>(kp, grp * H, H, qp, y, live, A, img, s);
        tile_product<T>(g, grp * H, H, cand, y, live, D, img, m);
        // softmax over the history (unmasked, userEncoders.py:164) and the weighted sum, on this lane's 4 T values of its pair
        const int h0 = 4 * (lane_here() >> 4);               // (recomputed: hoisted out of the tile loop, the 4 T padding tests
                                                             // would sit in SGPR pairs through both products and spill)
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[t][r] = (16 * t + h0 + r < H) ? s[t][r] * scale : -INFINITY;
                mx = fmaxf(mx, s[t][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float den = 0.f, num = 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = expf(s[t][r] - mx);          // (a padded row holds -inf: exactly 0)
                den += e;
                num = fmaf(e, m[t][r], num);
            }
        den += __shfl_xor(den, 16);
        den += __shfl_xor(den, 32);
        num += __shfl_xor(num, 16);
        num += __shfl_xor(num, 32);
        if (live && lane < 16) {
            const float base = num / den;
            logits[p] = use_weight ? base * lifetime_weight(remaining[p], alpha_s, beta_s, use_penalty) : base;
        }
    }
}

}  // namespace

namespace {

// The checks and the launch both entries share.  index == nullptr: the plain form (qp / cand hold P rows).
int grouped_match_launch(const char* who, const float* kp, const float* g, const float* qp, const float* cand, const float* remaining,
                         const int64_t* offsets, const int32_t* index, int64_t n, bool indexed, float* logits, int64_t G, int64_t P,
                         int32_t H, int32_t A, int32_t D, float scale, float alpha_s, float beta_s, int32_t use_weight,
                         int32_t use_penalty, void* stream) {
    LIME_REQUIRE(kp && g && qp && cand && offsets && logits && (!indexed || index), LIME_ERR_BAD_ARG, "%s: NULL pointer", who);
    LIME_REQUIRE(!use_weight || remaining, LIME_ERR_BAD_ARG, "%s: remaining is NULL", who);
    LIME_REQUIRE(G >= 0 && P >= 0 && H > 0 && A > 0 && D > 0 && n >= 0, LIME_ERR_BAD_ARG, "%s: bad dims", who);
    LIME_REQUIRE(H <= 128 && A <= 2048 && D <= 2048 && A % 4 == 0 && D % 4 == 0 && G < 0x7FFFFFFFL && n <= 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED,
                 "%s: H %d, A %d, D %d outside 1 <= H <= 128, A and D multiples of 4 up to 2048 (or %lld groups / %lld table rows >= 2^31)",
                 who, H, A, D, (long long)G, (long long)n);
    LIME_REQUIRE(lime_al16(kp, A) && lime_al16(qp, A) && lime_al16(g, D) && lime_al16(cand, D), LIME_ERR_BAD_ARG,
                 "%s: kp, qp, g and cand must be 16-byte aligned", who);
    LIME_REQUIRE(!indexed || n > 0 || P == 0, LIME_ERR_BAD_ARG, "%s: %lld pairs index an empty table", who, (long long)P);
    if (G == 0 || P == 0) return LIME_OK;
    // tile slices per group: enough workgroups to fill the chip when the groups are few (one group per user with the candidate-aware
    // attention off), never more than the tiles the pairs can make.  The split changes which workgroup takes a tile, not its bits.
    const long all_tiles = (P + PAIRS - 1) / PAIRS;
    long slices = (8L * lime_num_cus() + G - 1) / G;
    slices = slices > all_tiles ? all_tiles : slices;
    slices = slices < 1 ? 1 : (slices > 65535 ? 65535 : slices);
    const dim3 grid((unsigned)G, (unsigned)slices);
#define LIME_GM_LAUNCH(T_, I_)                                                                                                          \
    hipLaunchKernelGGL((grouped_match_kernel<T_, I_>), grid, dim3(256), 0, (hipStream_t)stream, kp, g, qp, cand, remaining,             \
                       (const long*)offsets, (const int*)index, (int)n, logits, (long)P, H, A, D, scale, alpha_s, beta_s, use_weight,   \
                       use_penalty)
#define LIME_GM_PICK(I_)                                                                                                                \
    do {                                                                                                                                \
        if (H <= 16) LIME_GM_LAUNCH(1, I_);                                                                                             \
        else if (H <= 32) LIME_GM_LAUNCH(2, I_);                                                                                        \
        else if (H <= 64) LIME_GM_LAUNCH(4, I_);                                                                                        \
        else LIME_GM_LAUNCH(8, I_);                                                                                                     \
    } while (0)
    if (indexed) LIME_GM_PICK(true);
    else LIME_GM_PICK(false);
#undef LIME_GM_PICK
#undef LIME_GM_LAUNCH
    return lime_check_launch(who);
}

}  // namespace

extern "C" int lime_grouped_match_f32(const float* kp, const float* g, const float* qp, const float* cand, const float* remaining,
                                      const int64_t* offsets, float* logits, int64_t G, int64_t P, int32_t H, int32_t A, int32_t D,
                                      float scale, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty, void* stream) {
    return grouped_match_launch("lime_grouped_match_f32", kp, g, qp, cand, remaining, offsets, nullptr, 0, false, logits, G, P, H, A, D,
                                scale, alpha_s, beta_s, use_weight, use_penalty, stream);
}

extern "C" int lime_grouped_match_indexed_f32(const float* kp, const float* g, const float* qp, const float* cand, const float* remaining,
                                              const int64_t* offsets, const int32_t* index, int64_t n, float* logits, int64_t G, int64_t P,
                                              int32_t H, int32_t A, int32_t D, float scale, float alpha_s, float beta_s,
                                              int32_t use_weight, int32_t use_penalty, void* stream) {
    return grouped_match_launch("lime_grouped_match_indexed_f32", kp, g, qp, cand, remaining, offsets, index, n, true, logits, G, P, H, A,
                                D, scale, alpha_s, beta_s, use_weight, use_penalty, stream);
}
