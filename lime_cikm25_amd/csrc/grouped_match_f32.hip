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
// Exact fp32: v_mfma_f32_16x16x4_f32 (mfma16).  A lane's four loaded columns go to four accumulators; every GM_FLUSH chunks the four are
// added as (c0 + c1) + (c2 + c3) into a compensated running sum and start again from zero.  The softmax and the weighted sum over h
// run on the results (h over the lane's 4 T registers in order, then the two butterfly steps over the lanes 16 and 32 apart).  Every sum has
// a fixed order that depends on H, A and D alone: a pair's bits depend neither on P, G, the group's position, the pair's place in its
// tile nor the grid.  No atomics.
//
// The indexed form (lime_grouped_match_indexed_f32): the pair's own operands are rows of two TABLES, qp [n, A] and cand [n, D], and
// pair p reads row index[p] of both -- a candidate whose representation depends on the news alone is not copied once per (user,
// candidate) pair.  Nothing else changes: only the row that gm_tile_product reads as Y differs, so a pair's bits are those of the plain
// form on the gathered rows.  An index outside [0, n) is clamped into it (as the offsets are clamped): a bad plan reads in range.
//
// The occurrence-composed form (lime_grouped_match_occurrence_f32): a LIME candidate under 'add' or 'concat' + project is
// A[news] + T[occurrence] with everything behind it linear, so the pair's operands are sums of a row of a news table and a row of an
// occurrence table: qp = qa[index[p]] + qt[occ[p]], cand = ca[index[p]] + ct[occ[p]], one fp32 add per element as the operand is
// fetched (gm_tile_product<T, true>).  A pair's bits are those of the plain form on rows composed with that add; occ is clamped into
// [0, n_occ) as index is into [0, n).  No LDS beyond the plain form's, no atomics.
#include "grouped_tile.h"        // the tile product and the softmax, shared with grouped_mlp_match_f32.hip

namespace {

using namespace lime_dev;

// INDEXED: qp / cand are tables of n rows and pair p reads row index[p] (clamped into [0, n)) of both; else row p (index unread).
// OCC: nothing, or one GmOccurrence behind the other arguments (the occurrence-composed form, INDEXED): the pair's operands are its
// table rows plus row occ[p] (clamped into [0, n_occ)) of the occurrence tables.  A trailing pack, so that the plain and the indexed
// instantiations keep their signatures and their code.
template <int T, bool INDEXED, class... OCC>
__global__ __launch_bounds__(256) void grouped_match_kernel(const float* __restrict__ kp, const float* __restrict__ g,
                                                             const float* __restrict__ qp, const float* __restrict__ cand,
                                                             const float* __restrict__ remaining, const long* __restrict__ offsets,
                                                             const int* __restrict__ index, int n, float* __restrict__ logits, long P, int H,
                                                             int A, int D, float scale, float alpha_s, float beta_s, int use_weight,
                                                             int use_penalty, OCC... occurrence) {
    __shared__ __attribute__((aligned(16))) float img[2 * 16 * T * GM_CHUNK];
    const long grp = blockIdx.x;
    long lo = offsets[grp], hi = offsets[grp + 1];
    lo = lo < 0 ? 0 : (lo > P ? P : lo);                     // every offset clamped into [0, P]: a bad plan reads and writes in range
    hi = hi < lo ? lo : (hi > P ? P : hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n_tile = (hi - lo + GM_PAIRS - 1) / GM_PAIRS;
    for (long tile = blockIdx.y; tile < n_tile; tile += gridDim.y) {         // (workgroup-uniform: the barriers inside stay whole)
        const long p = lo + tile * GM_PAIRS + 16 * wave + (lane & 15);
        const bool live = p < hi;
        long y = p;                                          // the pair's row of qp and cand
        if constexpr (INDEXED) {
            const int i = live ? index[p] : 0;
            y = i < 0 ? 0 : (i >= n ? n - 1 : i);
        }
        f32x4 s[T], m[T];
        if constexpr (sizeof...(OCC) != 0) {
            const GmOccurrence oc = (occurrence, ...);
            const long z = gm_occurrence_row(oc, p, live);   // the pair's row of the occurrence tables qt (oc.qt) and ct (oc.vt)
            gm_tile_product<T, true>(kp, grp * H, H, qp, y, live, A, img, s, oc.qt, z);
            gm_tile_product<T, true>(g, grp * H, H, cand, y, live, D, img, m, oc.vt, z);
        } else {
            gm_tile_product<T>(kp, grp * H, H, qp, y, live, A, img, s);
            gm_tile_product<T>(g, grp * H, H, cand, y, live, D, img, m);
        }
        // softmax over the history (grouped_tile.h: s becomes exp(s - max)) and the weighted sum, on this lane's 4 T values of its pair
        float den = gm_tile_softmax<T>(s, H, scale), num = 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) num = fmaf(s[t][r], m[t][r], num);
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

// The checks and the launch the three entries share.  form GM_PLAIN: qp / cand hold P rows (index unread); GM_INDEXED: tables of n rows;
// GM_OCCURRENCE: those tables plus qt / ct of n_occ rows, read through occ.
int grouped_match_launch(const char* who, int form, const float* kp, const float* g, const float* qp, const float* cand, const float* qt,
                         const float* ct, const float* remaining, const int64_t* offsets, const int32_t* index, int64_t n,
                         const int32_t* occ, int64_t n_occ, float* logits, int64_t G, int64_t P, int32_t H, int32_t A, int32_t D,
                         float scale, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty, void* stream) {
    const bool indexed = form != GM_PLAIN, composed = form == GM_OCCURRENCE;
    LIME_REQUIRE(kp && g && qp && cand && offsets && logits && (!indexed || index) && (!composed || (qt && ct && occ)), LIME_ERR_BAD_ARG,
                 "%s: NULL pointer", who);
    LIME_REQUIRE(!use_weight || remaining, LIME_ERR_BAD_ARG, "%s: remaining is NULL", who);
    const bool aligned = lime_al16(kp, A) && lime_al16(qp, A) && lime_al16(g, D) && lime_al16(cand, D) &&
                         (!composed || (lime_al16(qt, A) && lime_al16(ct, D)));
    if (const int bad = gm_check_shared(who, G, P, H, A, D, "D", 4, "A and D multiples of 4", aligned,
                                        "kp, qp, g and cand (and the occurrence tables) must be 16-byte aligned", indexed, n, composed, n_occ))
        return bad;
    if (G == 0 || P == 0) return LIME_OK;
    const dim3 grid((unsigned)G, (unsigned)gm_tile_slices(G, P));
#define LIME_GM_LAUNCH(T_, I_)                                                                                                          \
    hipLaunchKernelGGL((grouped_match_kernel<T_, I_>), grid, dim3(256), 0, (hipStream_t)stream, kp, g, qp, cand, remaining,             \
                       (const long*)offsets, (const int*)index, (int)n, logits, (long)P, H, A, D, scale, alpha_s, beta_s, use_weight,   \
                       use_penalty)
#define LIME_GM_LAUNCH_OCC(T_, I_)                                                                                                      \
    hipLaunchKernelGGL((grouped_match_kernel<T_, I_, GmOccurrence>), grid, dim3(256), 0, (hipStream_t)stream, kp, g, qp, cand,          \
                       remaining, (const long*)offsets, (const int*)index, (int)n, logits, (long)P, H, A, D, scale, alpha_s, beta_s,    \
                       use_weight, use_penalty, GmOccurrence{qt, ct, (const int*)occ, (int)n_occ})
    if (composed) LIME_GM_PICK(H, LIME_GM_LAUNCH_OCC, true);
    else if (indexed) LIME_GM_PICK(H, LIME_GM_LAUNCH, true);
    else LIME_GM_PICK(H, LIME_GM_LAUNCH, false);
#undef LIME_GM_LAUNCH_OCC
#undef LIME_GM_LAUNCH
    return lime_check_launch(who);
}

}  // namespace

extern "C" int lime_grouped_match_f32(const float* kp, const float* g, const float* qp, const float* cand, const float* remaining,
                                      const int64_t* offsets, float* logits, int64_t G, int64_t P, int32_t H, int32_t A, int32_t D,
                                      float scale, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty, void* stream) {
    return grouped_match_launch("lime_grouped_match_f32", GM_PLAIN, kp, g, qp, cand, nullptr, nullptr, remaining, offsets, nullptr, 0,
                                nullptr, 0, logits, G, P, H, A, D, scale, alpha_s, beta_s, use_weight, use_penalty, stream);
}

extern "C" int lime_grouped_match_indexed_f32(const float* kp, const float* g, const float* qp, const float* cand, const float* remaining,
                                              const int64_t* offsets, const int32_t* index, int64_t n, float* logits, int64_t G, int64_t P,
                                              int32_t H, int32_t A, int32_t D, float scale, float alpha_s, float beta_s,
                                              int32_t use_weight, int32_t use_penalty, void* stream) {
    return grouped_match_launch("lime_grouped_match_indexed_f32", GM_INDEXED, kp, g, qp, cand, nullptr, nullptr, remaining, offsets, index,
                                n, nullptr, 0, logits, G, P, H, A, D, scale, alpha_s, beta_s, use_weight, use_penalty, stream);
}

extern "C" int lime_grouped_match_occurrence_f32(const float* kp, const float* g, const float* qa, const float* ca, const float* qt,
                                                 const float* ct, const float* remaining, const int64_t* offsets, const int32_t* index,
                                                 int64_t n, const int32_t* occ, int64_t n_occ, float* logits, int64_t G, int64_t P,
                                                 int32_t H, int32_t A, int32_t D, float scale, float alpha_s, float beta_s,
                                                 int32_t use_weight, int32_t use_penalty, void* stream) {
    return grouped_match_launch("lime_grouped_match_occurrence_f32", GM_OCCURRENCE, kp, g, qa, ca, qt, ct, remaining, offsets, index, n,
                                occ, n_occ, logits, G, P, H, A, D, scale, alpha_s, beta_s, use_weight, use_penalty, stream);
}
