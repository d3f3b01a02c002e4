// The grouped match over a SCHEDULE of S time slots (Model.score_schedule): lime_grouped_match_occurrence_f32's function for every
// slot of a pair in one launch.  A LIME candidate under 'add' or 'concat' + project is A[news] + T[occurrence] with only linear maps
// behind it, and of the two only the occurrence row (and the remaining lifetime) moves with the slot, so per (slot s, pair p of group i)
//     s[h]        = (kp[i H + h] . qa[index[p]]  +  kp[i H + h] . qt[occ[s, p]]) * scale            a = softmax_h(s)
//     logits[s,p] = (sum_h a[h] (g[i H + h] . ca[index[p]]  +  g[i H + h] . ct[occ[s, p]])) * w(remaining[s, p])
// The first terms -- the H x A and H x D products per pair that are the whole cost of the twin kernels -- do not depend on the slot:
// they are made ONCE per pair by the pass body of grouped_match_f32.hip (gm_tile_product: exact fp32 on v_mfma_f32_16x16x4_f32, the
// compensated sum) and stay in the lane's registers, 2 T f32x4, across the slot loop.  The second terms take one of n_occ values per
// (group, history row): the workgroup forms its group's two tables  kt[z][h] = kp[i H + h] . qt[z]  and  gt[z][h] = g[i H + h] . ct[z]
// with the SAME tile product -- the occurrence rows standing where a tile's 64 pairs stand, ceil(n_occ / 64) times per table -- and keeps
// them in LDS for all its tiles.  A slot is then an epilogue: two f32x4 LDS reads and two adds per 4 history rows, the softmax of
// grouped_tile.h, the weighted sum, the weight.  No workspace, no launch and no buffer beyond occ / remaining / logits grows with S P.
//
// LDS (dynamic): the two chunk buffers of the tile product, 2 x 16 T x 16 floats, then kt and gt, n_occ x Hs floats each with Hs = H
// rounded up to 4 (a lane's four history rows h = 16 t + 4 (lane >> 4) .. + 3 are one aligned f32x4; rows behind Hs are never stored and
// never read: the softmax gives them weight exactly 0).  2048 T + 8 n_occ Hs bytes, at most 64 KiB: H = 50 with 100 occurrences takes
// 8 + 40.6 KiB.  Beyond it the entry returns LIME_ERR_UNSUPPORTED before any launch.
//
// Without occurrence tables (qt == ct == NULL, n_occ == 0: a baseline model, whose weight alone moves with the slot) the table terms are
// absent -- not added as zeros -- and the bits of (s, p) are those of lime_grouped_match_indexed_f32 for that pair with remaining[s, p].
// Fixed-order sums, no atomics, vector stores only: the bits of (s, p) depend on its own operands and on H, A and D alone -- not on S,
// the slot's position, the other slots, P, G, the group's position or the pair's place in its tile.
#include "grouped_tile.h"

namespace {

using namespace lime_dev;

constexpr long GMS_LDS_MAX = 65536;     // bytes of dynamic LDS a workgroup may ask for without an attribute on the function

inline long gms_lds_bytes(int T, int H, long n_occ) { return 4L * (2 * 16 * T * GM_CHUNK) + 8L * n_occ * ((H + 3) & ~3); }

// OCC: the occurrence tables are there (qt, ct, occ non-NULL, n_occ >= 1); else the baseline form.
template <int T, bool OCC>
__global__ __launch_bounds__(256) void grouped_match_schedule_kernel(const float* __restrict__ kp, const float* __restrict__ g,
                                                                      const float* __restrict__ qa, const float* __restrict__ ca,
                                                                      const float* __restrict__ qt, const float* __restrict__ ct,
                                                                      const float* __restrict__ remaining, const long* __restrict__ offsets,
                                                                      const int* __restrict__ index, int n, const int* __restrict__ occ,
                                                                      int n_occ, float* __restrict__ logits, long P, int S, int H, int A,
                                                                      int D, float scale, float alpha_s, float beta_s, int use_weight,
                                                                      int use_penalty) {
    extern __shared__ __attribute__((aligned(16))) float gms_lds[];
    float* img = gms_lds;                                    // the tile product's two chunk buffers
    const int Hs = (H + 3) & ~3;
    float* ktab = img + 2 * 16 * T * GM_CHUNK;               // kt [n_occ][Hs]
    float* gtab = ktab + (long)n_occ * Hs;                   // gt [n_occ][Hs]
    const long grp = blockIdx.x;
    long lo = offsets[grp], hi = offsets[grp + 1];
    lo = lo < 0 ? 0 : (lo > P ? P : lo);                     // every offset clamped into [0, P]: a bad plan reads and writes in range
    hi = hi < lo ? lo : (hi > P ? P : hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h0 = 4 * (lane >> 4);                          // this lane's first history row of a 16-row tile
    const long n_tile = (hi - lo + GM_PAIRS - 1) / GM_PAIRS;
    if ((long)blockIdx.y >= n_tile) return;                  // (workgroup-uniform) no tile here: no tables either
    if constexpr (OCC) {
        // the group's occurrence terms, once per workgroup: 64 occurrence rows at a time where a tile's pairs stand
        for (int z0 = 0; z0 < n_occ; z0 += GM_PAIRS) {
            const int z = z0 + 16 * wave + (lane & 15);
            const bool zlive = z < n_occ;
            f32x4 o[T];
            gm_tile_product<T>(kp, grp * H, H, qt, z, zlive, A, img, o);
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (zlive && 16 * t + h0 < Hs) *reinterpret_cast<f32x4*>(ktab + (long)z * Hs + 16 * t + h0) = o[t];
            gm_tile_product<T>(g, grp * H, H, ct, z, zlive, D, img, o);
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (zlive && 16 * t + h0 < Hs) *reinterpret_cast<f32x4*>(gtab + (long)z * Hs + 16 * t + h0) = o[t];
        }
        // (read behind the barriers of the tile products below: every tile runs two of them before its slot loop)
    }
    for (long tile = blockIdx.y; tile < n_tile; tile += gridDim.y) {         // (workgroup-uniform: the barriers inside stay whole)
        const long p = lo + tile * GM_PAIRS + 16 * wave + (lane & 15);
        const bool live = p < hi;
        const int i = live ? index[p] : 0;
        const long y = i < 0 ? 0 : (i >= n ? n - 1 : i);
        f32x4 sa[T], ma[T];                                  // the slot-independent products: in registers across the slot loop
        gm_tile_product<T>(kp, grp * H, H, qa, y, live, A, img, sa);
        gm_tile_product<T>(g, grp * H, H, ca, y, live, D, img, ma);
        for (int slot = 0; slot < S; ++slot) {
            const long sp = (long)slot * P + p;
            long zrow = 0;
            if constexpr (OCC) {
                const int o = live ? occ[sp] : 0;
                zrow = (long)(o < 0 ? 0 : (o >= n_occ ? n_occ - 1 : o)) * Hs;
            }
            f32x4 e[T];
#pragma unroll
            for (int t = 0; t < T; ++t) {
                e[t] = sa[t];
                if constexpr (OCC)
                    if (16 * t + h0 < Hs) e[t] += *reinterpret_cast<const f32x4*>(ktab + zrow + 16 * t + h0);
            }
            float den = gm_tile_softmax<T>(e, H, scale), num = 0.f;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                f32x4 m = ma[t];
                if constexpr (OCC)
                    if (16 * t + h0 < Hs) m += *reinterpret_cast<const f32x4*>(gtab + zrow + 16 * t + h0);
#pragma unroll
                for (int r = 0; r < 4; ++r) num = fmaf(e[t][r], m[r], num);
            }
            num += __shfl_xor(num, 16);
            num += __shfl_xor(num, 32);
            if (live && lane < 16) {
                const float base = num / den;
                logits[sp] = use_weight ? base * lifetime_weight(remaining[sp], alpha_s, beta_s, use_penalty) : base;
            }
        }
    }
}

}  // namespace

extern "C" int lime_grouped_match_schedule_f32(const float* kp, const float* g, const float* qa, const float* ca, const float* qt,
                                               const float* ct, const float* remaining, const int64_t* offsets, const int32_t* index,
                                               int64_t n, const int32_t* occ, int64_t n_occ, float* logits, int64_t G, int64_t P, int32_t S,
                                               int32_t H, int32_t A, int32_t D, float scale, float alpha_s, float beta_s,
                                               int32_t use_weight, int32_t use_penalty, void* stream) {
    const char* who = "lime_grouped_match_schedule_f32";
    const bool tables = qt || ct;
    // the checks of the occurrence form (lime_grouped_match_occurrence_f32; the occurrence tables are optional here) ...
    LIME_REQUIRE(kp && g && qa && ca && offsets && logits && index, LIME_ERR_BAD_ARG, "%s: NULL pointer", who);
    LIME_REQUIRE(!use_weight || remaining, LIME_ERR_BAD_ARG, "%s: remaining is NULL", who);
    const bool aligned = lime_al16(kp, A) && lime_al16(qa, A) && lime_al16(g, D) && lime_al16(ca, D) && lime_al16(qt, A) && lime_al16(ct, D);
    if (const int bad = gm_check_shared(who, G, P, H, A, D, "D", 4, "A and D multiples of 4", aligned,
                                        "kp, qa, g and ca (and the occurrence tables) must be 16-byte aligned", true, n, tables, n_occ))
        return bad;
    // ... then the schedule's own
    LIME_REQUIRE(S >= 1, LIME_ERR_BAD_ARG, "%s: S = %d slots, at least one is needed", who, S);
    LIME_REQUIRE(!tables || occ, LIME_ERR_BAD_ARG, "%s: occurrence tables without occ", who);
    LIME_REQUIRE((qt != nullptr) == (ct != nullptr) && (tables || n_occ == 0), LIME_ERR_BAD_ARG,
                 "%s: qt and ct come together, and n_occ = %lld rows need them", who, (long long)n_occ);
    const int T = gm_history_tiles(H);
    const long lds = gms_lds_bytes(T, H, tables ? n_occ : 0);
    LIME_REQUIRE(lds <= GMS_LDS_MAX, LIME_ERR_UNSUPPORTED,
                 "%s: %lld occurrences x H %d take %ld bytes of LDS (2048 T + 8 n_occ Hs, T = %d, Hs = H rounded up to 4), the limit is %ld",
                 who, (long long)n_occ, H, lds, T, GMS_LDS_MAX);
    if (G == 0 || P == 0) return LIME_OK;
    // tile slices per group as in lime_grouped_match_f32 -- enough workgroups to fill the chip when the groups are few --, but every
    // workgroup forms its group's tables first (2 ceil(n_occ / 64) tile products), so a slice keeps at least as many tiles of its own
    // where the groups have them.  The split changes which workgroup takes a tile, not its bits.
    long slices = gm_tile_slices(G, P);
    if (tables) {
        const long all_tiles = (P + GM_PAIRS - 1) / GM_PAIRS;
        const long per_group = (all_tiles + G - 1) / G, table_tiles = (n_occ + GM_PAIRS - 1) / GM_PAIRS;
        const long cap = per_group / table_tiles;
        if (slices > cap) slices = cap < 1 ? 1 : cap;
    }
    const dim3 grid((unsigned)G, (unsigned)slices);
#define LIME_GMS_LAUNCH(T_, O_)                                                                                                         \
    hipLaunchKernelGGL((grouped_match_schedule_kernel<T_, O_>), grid, dim3(256), (size_t)lds, (hipStream_t)stream, kp, g, qa, ca, qt,   \
                       ct, remaining, (const long*)offsets, (const int*)index, (int)n, (const int*)occ, (int)(tables ? n_occ : 0),      \
                       logits, (long)P, S, H, A, D, scale, alpha_s, beta_s, use_weight, use_penalty)
    if (tables) LIME_GM_PICK(H, LIME_GMS_LAUNCH, true);
    else LIME_GM_PICK(H, LIME_GMS_LAUNCH, false);
#undef LIME_GMS_LAUNCH
    return lime_check_launch(who);
}
