// What the grouped matches share (grouped_match_f32.hip, grouped_mlp_match_f32.hip): the [16 T x 16] tile product of a group's shared
// rows with a wave's 16 pairs, and the softmax over the history on its result.  One copy: both kernels' first product and softmax are
// the same instructions, so a pair's attention weights are the same bits in both.  Below the device code, the host half: the H -> T
// choice, the tile-slice rule and the argument checks that the launchers of those two units and of grouped_match_schedule_f32.hip share.
#pragma once
#include "dev_helpers.h"

namespace lime_dev {

constexpr int GM_PAIRS = 64;            // pairs of a workgroup tile: 16 per wave
constexpr int GM_CHUNK = 16;            // columns of an LDS chunk: one 64-byte row of the swizzled image
constexpr int GM_FLUSH = 2;             // chunks between two flushes of the MFMA accumulators into the compensated sum

// Where a pair's own operands come from: its own row p (GM_PLAIN); row index[p] of a table (GM_INDEXED); or that row plus row occ[p]
// of an occurrence table, one fp32 add per element (GM_OCCURRENCE).
constexpr int GM_PLAIN = 0, GM_INDEXED = 1, GM_OCCURRENCE = 2;

// What the occurrence-composed form adds to the indexed form's arguments: qt [n_occ, A] beside the qp table, vt [n_occ, D or Dh]
// beside the table of the second operand (cand / nw), and the pairs' rows of both, occ int32 [P].
struct GmOccurrence {
    const float* qt;
    const float* vt;
    const int* occ;
    int n_occ;
};

// Pair p's row of the occurrence tables: occ[p] clamped into [0, n_occ), as an index is into [0, n) -- a bad plan reads in range.
__device__ __forceinline__ long gm_occurrence_row(const GmOccurrence& oc, long p, bool live) {
    const int o = live ? oc.occ[p] : 0;
    return o < 0 ? 0 : (o >= oc.n_occ ? oc.n_occ - 1 : o);
}

// One [16 T x 16] tile product per wave over K columns: out[t][r] = X[16 t + 4 (lane >> 4) + r, :K] . Y[pair of lane & 15, :K].
// X: the group's rows x0 .. x0 + H - 1 of a dense [*, K] matrix (shared by the workgroup, through `img`); Y: row `yrow` of a dense
// [*, K] matrix, or nothing (zeros) when `ylive` is false.  Ends with a barrier: `img` is free again when it returns.
// ADD (the occurrence-composed forms): the pair's operand is Y[yrow, :] + Y2[y2row, :], one fp32 add per element, a + t in that order,
// made when the chunk is fetched -- only the sum lives across the barrier, and the product is that of the plain form on the composed row.
template <int T, bool ADD = false>
__device__ __forceinline__ void gm_tile_product(const float* __restrict__ X, long x0, int H, const float* __restrict__ Y, long yrow, bool ylive,
                                             int K, float* img, f32x4 (&out)[T], const float* __restrict__ Y2 = nullptr, long y2row = 0) {
    constexpr int NL = T < 4 ? 1 : T / 4;                    // 16-byte pieces of a chunk per thread: 16 T rows x 4 segments / 256
    const int lane = threadIdx.x & 63;
    const int ar = lane & 15, as = lane >> 4;                // this lane's row of a 16-row tile and its 16-byte segment
    const int n_chunk = (K + GM_CHUNK - 1) / GM_CHUNK;
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
            const int row = piece >> 2, col = c * GM_CHUNK + 4 * (piece & 3);
            xs[j] = (row < H && col < K) ? *reinterpret_cast<const f32x4*>(X + (x0 + row) * K + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int col = c * GM_CHUNK + 4 * as;
        ys = (ylive && col < K) ? *reinterpret_cast<const f32x4*>(Y + yrow * K + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (ADD) ys += (ylive && col < K) ? *reinterpret_cast<const f32x4*>(Y2 + y2row * K + col) : f32x4{0.f, 0.f, 0.f, 0.f};
    };

    // The accumulators are emptied every GM_FLUSH chunks into a compensated sum (tot + comp, Knuth's two-sum): one fmaf chain over all
    // K / 4 of a lane's column groups loses about three times what lime_interest_match_f32's shuffle trees lose at K = 400; chains
    // of 4 GM_FLUSH products with an exactly corrected running sum behind them lose less than those trees.
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
        float* buf = img + (c & 1) * (16 * T * GM_CHUNK);
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int piece = (int)threadIdx.x + 256 * j;
            const int row = piece >> 2, seg = piece & 3;
            if (row < 16 * T) *reinterpret_cast<f32x4*>(buf + row * GM_CHUNK + 4 * (seg ^ swz4((row >> 2) & 3))) = xs[j];
        }
        const f32x4 b = ys;
        lds_barrier();                                       // (two buffers: the chunk written here was last read two barriers ago)
        if (c + 1 < n_chunk) fetch(c + 1);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int row = 16 * t + ar;
            const f32x4 a = *reinterpret_cast<const f32x4*>(buf + row * GM_CHUNK + 4 * (as ^ swz4((row >> 2) & 3)));
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][i] = mfma16(a[i], b[i], acc[t][i]);
        }
        if ((c + 1) % GM_FLUSH == 0 || c + 1 == n_chunk) flush();
    }
#pragma unroll
    for (int t = 0; t < T; ++t) out[t] = tot[t] + comp[t];
    lds_barrier();
}

// The softmax over the history (unmasked, userEncoders.py:164) on a tile product's scores, this lane's 4 T values of its pair (h =
// 16 t + 4 (lane >> 4) + r): s becomes e = exp(s * scale - max), exactly 0 for a padded row h >= H; returns the pair's sum of e over
// all h (h over the lane's registers in order, then the two butterfly steps over the lanes 16 and 32 apart), in every lane of the pair.
template <int T>
__device__ __forceinline__ float gm_tile_softmax(f32x4 (&s)[T], int H, float scale) {
    const int h0 = 4 * (lane_here() >> 4);                   // (recomputed: hoisted out of the tile loop, the 4 T padding tests
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
    float den = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[t][r] = expf(s[t][r] - mx);                    // (a padded row holds -inf: exactly 0)
            den += s[t][r];
        }
    den += __shfl_xor(den, 16);
    den += __shfl_xor(den, 32);
    return den;
}

}  // namespace lime_dev

// ---- host side: what the launchers of grouped_match_f32.hip, grouped_mlp_match_f32.hip and grouped_match_schedule_f32.hip share ----

// The kernels' T: the 16-row tiles that hold a history of H <= 128 rows.
static inline int gm_history_tiles(int H) { return H <= 16 ? 1 : H <= 32 ? 2 : H <= 64 ? 4 : 8; }

// L_(T, ...) with the T of a history of H_ rows as a literal, for a launch macro L_ that names a kernel instantiation.
#define LIME_GM_PICK(H_, L_, ...)                                                                                                       \
    do {                                                                                                                                \
        switch (gm_history_tiles(H_)) {                                                                                                 \
            case 1: L_(1, __VA_ARGS__); break;                                                                                          \
            case 2: L_(2, __VA_ARGS__); break;                                                                                          \
            case 4: L_(4, __VA_ARGS__); break;                                                                                          \
            default: L_(8, __VA_ARGS__);                                                                                                \
        }                                                                                                                               \
    } while (0)

// Tile slices per group (gridDim.y) for G >= 1 groups over P >= 1 pairs: enough workgroups to fill the chip when the groups are few
// (one group per user with the candidate-aware attention off), never more than the tiles the pairs can make.  The split changes which
// workgroup takes a tile, not its bits.
static inline long gm_tile_slices(int64_t G, int64_t P) {
    const long all_tiles = (P + lime_dev::GM_PAIRS - 1) / lime_dev::GM_PAIRS;
    long slices = (8L * lime_num_cus() + G - 1) / G;
    slices = slices > all_tiles ? all_tiles : slices;
    return slices < 1 ? 1 : (slices > 65535 ? 65535 : slices);
}

// The checks the three launchers share, in their order, behind the unit's own NULL checks: the dimensions, their bounds and the
// 2^31 bounds of G / n / n_occ, the unit's alignment rule (``aligned``: whether it holds, ``align_rule``: its words), the empty tables.
// The second operand is W columns wide, a multiple of ``w_mult``, and the unit calls it ``w_name``; ``widths``: its words for the
// two widths' rule.  indexed / composed: whether the pairs read a table of n rows / an occurrence table of n_occ rows.
static inline int gm_check_shared(const char* who, int64_t G, int64_t P, int32_t H, int32_t A, int32_t W, const char* w_name, int w_mult,
                                  const char* widths, bool aligned, const char* align_rule, bool indexed, int64_t n, bool composed,
                                  int64_t n_occ) {
    LIME_REQUIRE(G >= 0 && P >= 0 && H > 0 && A > 0 && W > 0 && n >= 0 && n_occ >= 0, LIME_ERR_BAD_ARG, "%s: bad dims", who);
    LIME_REQUIRE(H <= 128 && A <= 2048 && W <= 2048 && A % 4 == 0 && W % w_mult == 0 && G < 0x7FFFFFFFL && n <= 0x7FFFFFFFL &&
                     n_occ <= 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED,
                 "%s: H %d, A %d, %s %d outside 1 <= H <= 128, %s up to 2048 (or %lld groups / %lld, %lld table rows >= 2^31)", who, H, A,
                 w_name, W, widths, (long long)G, (long long)n, (long long)n_occ);
    LIME_REQUIRE(aligned, LIME_ERR_BAD_ARG, "%s: %s", who, align_rule);
    LIME_REQUIRE(!indexed || n > 0 || P == 0, LIME_ERR_BAD_ARG, "%s: %lld pairs index an empty table", who, (long long)P);
    LIME_REQUIRE(!composed || n_occ > 0 || P == 0, LIME_ERR_BAD_ARG, "%s: %lld pairs index an empty occurrence table", who, (long long)P);
    return LIME_OK;
}
