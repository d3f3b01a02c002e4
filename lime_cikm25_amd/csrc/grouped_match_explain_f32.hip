// The grouped match of grouped_match_f32.hip with its terms kept: why a pair scores what it scores.  Per pair p of group i
//     s[h] = kp[i, h, :] . qp[p, :] * scale      e[h] = exp(s[h] - max)      den = sum_h e[h]      m[h] = g[i, h, :] . cand[p, :]
//     base[p] = (sum_h e[h] m[h]) / den          weight[p] = w(remaining[p])  (1 with use_weight off)        logits[p] = base * weight
//     attn[p, h] = e[h] / den                    contrib[p, h] = (attn[p, h] * m[h]) * weight[p]
// -- the score IS a sum over the history slots (times the lifetime weight), so a slot's share of it needs no surrogate model: the twin
// holds every e[h] and m[h] of a pair in registers across four lanes and writes their sum alone; this kernel writes the terms too.
//
// The two products and the softmax are gm_tile_product / gm_tile_softmax of grouped_tile.h, called as the twin calls them, and num, den,
// base and the weight are formed by the twin's own expressions: logits[p] has the bits of lime_grouped_match_*_f32 on the same operands,
// in the plain, the indexed and the occurrence-composed form (one kernel template, the twin's three instantiations per T).
//
// On top, per pair: the m history slots of largest contrib (by = LIME_EXPLAIN_BY_CONTRIBUTION) or largest attn
// (LIME_EXPLAIN_BY_ATTENTION), among the slots whose byte of mask [G / hist_div, H] is set (row grp / hist_div, as the refinement reads a
// shared history; NULL: every slot).  The softmax stays unmasked, as in the reference (userEncoders.py:164): the mask gates which slots
// may be NAMED, not what they weigh.  Order: the keys of topk_keys.h -- larger value first, equal values (+0.0 and -0.0 are equal) lower
// slot first, a NaN behind every number --; slots behind the last eligible one hold -1 / 0.0.  The selection runs in the pair's four
// lanes on the registers the products left there: every value becomes its key once, then m rounds of a register argmax over the lane's
// 4 T keys and the two butterfly steps over the lanes 16 and 32 apart; the winner's key is cleared in the lane that owns it and its value
// bits travel the same two steps (an OR: three lanes hold 0).  No LDS beyond gm_tile_product's image, no workspace, no atomics; every
// sum has the twin's fixed order: a pair's bits depend neither on P, G, the group's position, the pair's place in its tile nor the grid.
#include "grouped_tile.h"
#include "topk_keys.h"           // score_key: the order of the device top-k

namespace {

using namespace lime_dev;

constexpr int GX_MAX_TOP = 16;   // slots named per pair

// What the explain form adds to the twin's arguments.  attn / contrib [P, H] may be NULL (both are optional, each on its own).
struct GmExplain {
    const unsigned char* mask;   // u8 [ceil(G / hist_div), H] or NULL
    int hist_div, m, by_attention;
    float* base;                 // [P]
    float* weight;               // [P]
    float* attn;                 // [P, H] or NULL
    float* contrib;              // [P, H] or NULL
    int* top_slot;               // [P, m]
    float* top_value;            // [P, m]
};

template <int T, bool INDEXED, class... OCC>
__global__ __launch_bounds__(256) void grouped_match_explain_kernel(const float* __restrict__ kp, const float* __restrict__ g,
                                                                     const float* __restrict__ qp, const float* __restrict__ cand,
                                                                     const float* __restrict__ remaining, const long* __restrict__ offsets,
                                                                     const int* __restrict__ index, int n, float* __restrict__ logits, long P,
                                                                     int H, int A, int D, float scale, float alpha_s, float beta_s,
                                                                     int use_weight, int use_penalty, GmExplain ex, OCC... occurrence) {
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
            const long z = gm_occurrence_row(oc, p, live);
            gm_tile_product<T, true>(kp, grp * H, H, qp, y, live, A, img, s, oc.qt, z);
            gm_tile_product<T, true>(g, grp * H, H, cand, y, live, D, img, m, oc.vt, z);
        } else {
            gm_tile_product<T>(kp, grp * H, H, qp, y, live, A, img, s);
            gm_tile_product<T>(g, grp * H, H, cand, y, live, D, img, m);
        }
        // the twin's epilogue, expression for expression: logits[p] carries its bits
        float den = gm_tile_softmax<T>(s, H, scale), num = 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) num = fmaf(s[t][r], m[t][r], num);
        num += __shfl_xor(num, 16);
        num += __shfl_xor(num, 32);
        const float base = num / den;                        // (num and den are the pair's in all four of its lanes)
        const float w = (use_weight && live) ? lifetime_weight(remaining[p], alpha_s, beta_s, use_penalty) : 1.f;
        if (live && lane < 16) {
            logits[p] = use_weight ? base * w : base;
            ex.base[p] = base;
            ex.weight[p] = w;
        }
        // the terms: this lane holds the slots h = 16 t + h0 + r of its pair.  s becomes attn, m becomes contrib; each value's key
        // (0: the slot takes no part -- padded, masked out or the pair dead) is formed once
        const int h0 = 4 * (lane_here() >> 4);
        const unsigned char* mrow = ex.mask ? ex.mask + (grp / ex.hist_div) * H : nullptr;
        tkey key[T][4];
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int h = 16 * t + h0 + r;
                const bool in = live && h < H;
                const float a = s[t][r] / den;
                const float c = (a * m[t][r]) * w;
                s[t][r] = a;
                m[t][r] = c;
                if (in && ex.attn) ex.attn[p * H + h] = a;
                if (in && ex.contrib) ex.contrib[p * H + h] = c;
                const bool open = in && (mrow == nullptr || mrow[h] != 0);
                key[t][r] = open ? score_key(ex.by_attention ? a : c, (unsigned)h) : 0ull;
            }
        for (int j = 0; j < ex.m; ++j) {
            tkey best = 0ull;
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) best = key[t][r] > best ? key[t][r] : best;
            tkey other = __shfl_xor(best, 16);
            best = other > best ? other : best;
            other = __shfl_xor(best, 32);
            best = other > best ? other : best;
            // the lane that owns the winner clears its key and gives the value's bits; keys of a pair are distinct, so one lane does
            unsigned bits = 0u;
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool won = best != 0ull && key[t][r] == best;
                    bits = won ? __float_as_uint(ex.by_attention ? s[t][r] : m[t][r]) : bits;
                    key[t][r] = won ? 0ull : key[t][r];
                }
            bits |= __shfl_xor(bits, 16);
            bits |= __shfl_xor(bits, 32);
            if (live && lane < 16) {
                ex.top_slot[p * ex.m + j] = best ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) : -1;
                ex.top_value[p * ex.m + j] = best ? __uint_as_float(bits) : 0.f;
            }
        }
    }
}

// The checks and the launch.  The form follows the pointers: index NULL: plain (qp / cand hold P rows); index alone: tables of n rows;
// index with occ, qt and ct: those tables plus the occurrence tables of n_occ rows.
int grouped_match_explain_launch(const char* who, const float* kp, const float* g, const float* qp, const float* cand, const float* qt,
                                 const float* ct, const float* remaining, const int64_t* offsets, const int32_t* index, int64_t n,
                                 const int32_t* occ, int64_t n_occ, float* logits, const GmExplain& ex, int64_t G, int64_t P, int32_t H,
                                 int32_t A, int32_t D, float scale, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty,
                                 void* stream) {
    const bool any_occ = occ || qt || ct, composed = occ && qt && ct, indexed = index != nullptr;
    LIME_REQUIRE(kp && g && qp && cand && offsets && logits && ex.base && ex.weight && ex.top_slot && ex.top_value, LIME_ERR_BAD_ARG,
                 "%s: NULL pointer", who);
    LIME_REQUIRE(any_occ == composed && (!composed || indexed), LIME_ERR_BAD_ARG,
                 "%s: the occurrence-composed form takes index, occ, qt and ct together", who);
    LIME_REQUIRE(!use_weight || remaining, LIME_ERR_BAD_ARG, "%s: remaining is NULL", who);
    const bool aligned = lime_al16(kp, A) && lime_al16(qp, A) && lime_al16(g, D) && lime_al16(cand, D) &&
                         (!composed || (lime_al16(qt, A) && lime_al16(ct, D)));
    if (const int bad = gm_check_shared(who, G, P, H, A, D, "D", 4, "A and D multiples of 4", aligned,
                                        "kp, qp, g and cand (and the occurrence tables) must be 16-byte aligned", indexed, indexed ? n : 0,
                                        composed, composed ? n_occ : 0))
        return bad;
    LIME_REQUIRE(ex.m >= 1 && ex.m <= H && ex.hist_div >= 1, LIME_ERR_BAD_ARG, "%s: m %d outside 1 <= m <= H = %d, or hist_div %d < 1", who,
                 ex.m, H, ex.hist_div);
    LIME_REQUIRE(ex.m <= GX_MAX_TOP, LIME_ERR_UNSUPPORTED, "%s: m %d > %d", who, ex.m, GX_MAX_TOP);
    if (G == 0 || P == 0) return LIME_OK;
    const dim3 grid((unsigned)G, (unsigned)gm_tile_slices(G, P));
#define LIME_GX_LAUNCH(T_, I_)                                                                                                          \
    hipLaunchKernelGGL((grouped_match_explain_kernel<T_, I_>), grid, dim3(256), 0, (hipStream_t)stream, kp, g, qp, cand, remaining,     \
                       (const long*)offsets, (const int*)index, (int)n, logits, (long)P, H, A, D, scale, alpha_s, beta_s, use_weight,   \
                       use_penalty, ex)
#define LIME_GX_LAUNCH_OCC(T_, I_)                                                                                                      \
    hipLaunchKernelGGL((grouped_match_explain_kernel<T_, I_, GmOccurrence>), grid, dim3(256), 0, (hipStream_t)stream, kp, g, qp, cand,  \
                       remaining, (const long*)offsets, (const int*)index, (int)n, logits, (long)P, H, A, D, scale, alpha_s, beta_s,    \
                       use_weight, use_penalty, ex, GmOccurrence{qt, ct, (const int*)occ, (int)n_occ})
    if (composed) LIME_GM_PICK(H, LIME_GX_LAUNCH_OCC, true);
    else if (indexed) LIME_GM_PICK(H, LIME_GX_LAUNCH, true);
    else LIME_GM_PICK(H, LIME_GX_LAUNCH, false);
#undef LIME_GX_LAUNCH_OCC
#undef LIME_GX_LAUNCH
    return lime_check_launch(who);
}

}  // namespace

extern "C" int lime_grouped_match_explain_f32(const float* kp, const float* g, const float* qp, const float* cand, const float* qt,
                                              const float* ct, const float* remaining, const int64_t* offsets, const int32_t* index,
                                              int64_t n, const int32_t* occ, int64_t n_occ, const uint8_t* mask, int32_t hist_div, int32_t m,
                                              int32_t by, float* logits, float* base, float* weight, float* attn, float* contrib,
                                              int32_t* top_slot, float* top_value, int64_t G, int64_t P, int32_t H, int32_t A, int32_t D,
                                              float scale, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty,
                                              void* stream) {
    const char* who = "lime_grouped_match_explain_f32";
    LIME_REQUIRE(by == LIME_EXPLAIN_BY_CONTRIBUTION || by == LIME_EXPLAIN_BY_ATTENTION, LIME_ERR_BAD_ARG, "%s: by %d is neither "
                 "LIME_EXPLAIN_BY_CONTRIBUTION nor LIME_EXPLAIN_BY_ATTENTION", who, by);
    const GmExplain ex{mask, hist_div, m, by == LIME_EXPLAIN_BY_ATTENTION, base, weight, attn, contrib, top_slot, top_value};
    return grouped_match_explain_launch(who, kp, g, qp, cand, qt, ct, remaining, offsets, index, n, occ, n_occ, logits, ex, G, P, H, A, D,
                                        scale, alpha_s, beta_s, use_weight, use_penalty, stream);
}
