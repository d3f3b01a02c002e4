// History-vs-candidate attention + the MLP click predictor (reference model.py:113-115, :182-184) for GROUPS of pairs that share one
// refined history, with mlp.weight [Dh, 2 D] split into its user half W_u and its news half W_n.  Per pair p of group i:
//     s[h]   = kp[i, h, :] . qp[p, :] * scale              a = softmax_h(s)
//     u[j]   = sum_h a[h] gu[i, h, j]                      gu = g W_u^T  [G H, Dh]: the user half of the hidden layer, per history row
//     logits[p] = sum_j relu(u[j] + nw[p, j]) w_out[j] + b_out          nw = cand W_n^T + mlp.bias  [P, Dh]
// The ReLU stands between the pooled user vector and the sum over j, so the weighted sum over h cannot move behind a dot product
// with the candidate as in grouped_match_f32.hip: the pooled hidden row u has to exist per pair.  It exists in registers alone, 16
// columns at a time -- no [P, D] user row and no [P, Dh] hidden row reach memory.
//
// A workgroup (four waves) takes 64-pair tiles of one group, a wave 16 pairs of the tile.  The first product and the softmax are
// grouped_tile.h's (the instructions of lime_grouped_match_f32).  The softmax weights leave them in the MFMA's C layout -- pair =
// lane & 15, h = 16 t + 4 (lane >> 4) + r -- which is the B operand B[k = lane >> 4][lane & 15] of v_mfma_f32_16x16x4_f32 when the
// four k slots of MFMA (t, r) stand for h = 16 t + 4 k + r: the weights go from the softmax into the second product without leaving
// their registers.  Its A operand is gu^T: lane l supplies gu[16 t + 4 (l >> 4) + r][j0 + (l & 15)] from a chunk of 16 columns of
// the group's gu rows in LDS ([16 T rows][GS floats], H padded with zero rows in LDS only; chunk c + 1 on its way from global memory
// into registers while chunk c is multiplied, two buffers and one barrier per chunk).  The result C[column j0 + 4 (l >> 4) + r'][pair
// l & 15] leaves a lane four columns of its pair's u: it adds its pair's nw (read straight from global memory, 8 bytes per load),
// applies the ReLU, multiplies by w_out and adds into the pair's scalar; the lanes 16 and 32 apart are added at the end.
// Exact fp32.  The sum over h of a column runs in four MFMA chains (one per r, t ascending), added as (c0 + c1) + (c2 + c3); the sum
// over j runs r' = 0 .. 3 per chunk, chunks ascending, then the two butterfly steps.  Every order depends on H, A and Dh alone: a
// pair's bits depend neither on P, G, the group's position, the pair's place in its tile nor the grid.  No atomics.
// Dh is any even number: rows of gu and nw are read 8 bytes at a time, columns behind Dh are zeros in registers (relu(0) * 0).
//
// The indexed form (lime_grouped_mlp_match_indexed_f32): qp [n, A] and nw [n, Dh] are tables and pair p reads row index[p] of both,
// clamped into [0, n) -- the rules of lime_grouped_match_indexed_f32.
// The occurrence-composed form (lime_grouped_mlp_match_occurrence_f32): qp = qa[index[p]] + qt[occ[p]] and nw = na[index[p]] +
// nt[occ[p]], one fp32 add per element as the operand is fetched -- the rules of lime_grouped_match_occurrence_f32.
#include "grouped_tile.h"

namespace {

using namespace lime_dev;

constexpr int GS = 20;               // floats of an LDS row of the gu chunk (16 used): the four k slots' rows, 4 apart, land 80 floats
                                     // = 16 banks apart, so a wave's ds_read_b32 of 4 rows x 16 columns touches every bank once

// INDEXED, OCC: as in grouped_match_f32.hip -- the pair's row p of qp / nw, row index[p] of two tables, or (one GmOccurrence behind the
// other arguments) that row plus row occ[p] of the occurrence tables qt (oc.qt) and nt (oc.vt).
template <int T, bool INDEXED, class... OCC>
__global__ __launch_bounds__(256) void grouped_mlp_match_kernel(const float* __restrict__ kp, const float* __restrict__ gu,
                                                                 const float* __restrict__ qp, const float* __restrict__ nw,
                                                                 const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                                 const long* __restrict__ offsets, const int* __restrict__ index, int n,
                                                                 float* __restrict__ logits, long P, int H, int A, int Dh, float scale,
                                                                 OCC... occurrence) {
    constexpr int ROWS = 16 * T;
    constexpr int NP = T < 2 ? 1 : T / 2;                    // 8-byte pieces of a gu chunk per thread: 16 T rows x 8 pieces / 256
    __shared__ __attribute__((aligned(16))) float img[2 * ROWS * GS];       // (the first product uses 2 * ROWS * GM_CHUNK of it)
    const long grp = blockIdx.x;
    long lo = offsets[grp], hi = offsets[grp + 1];
    lo = lo < 0 ? 0 : (lo > P ? P : lo);                     // every offset clamped into [0, P]: a bad plan reads and writes in range
    hi = hi < lo ? lo : (hi > P ? P : hi);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ar = lane & 15, as = lane >> 4;
    const float bias = b_out ? *b_out : 0.f;
    const long x0 = grp * H;
    const int n_chunk = (Dh + GM_CHUNK - 1) / GM_CHUNK;
    const long n_tile = (hi - lo + GM_PAIRS - 1) / GM_PAIRS;
    for (long tile = blockIdx.y; tile < n_tile; tile += gridDim.y) {         // (workgroup-uniform: the barriers inside stay whole)
        const long p = lo + tile * GM_PAIRS + 16 * wave + ar;
        const bool live = p < hi;
        long y = p;                                          // the pair's row of qp and nw
        if constexpr (INDEXED) {
            const int i = live ? index[p] : 0;
            y = i < 0 ? 0 : (i >= n ? n - 1 : i);
        }
        f32x4 a[T];
        const float* nt = nullptr;                           // the occurrence table beside nw and the pair's row of it (composed form)
        long z = 0;
        if constexpr (sizeof...(OCC) != 0) {
            const GmOccurrence oc = (occurrence, ...);
            nt = oc.vt;
            z = gm_occurrence_row(oc, p, live);
            gm_tile_product<T, true>(kp, x0, H, qp, y, live, A, img, a, oc.qt, z);
        } else {
            gm_tile_product<T>(kp, x0, H, qp, y, live, A, img, a);
        }
        const float den = gm_tile_softmax<T>(a, H, scale);
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) a[t][r] = a[t][r] / den;             // (a padded row h >= H: exactly 0)

        // the second product, a^T . gu over h, in chunks of 16 columns of gu, and each chunk's epilogue
        f32x2 xs[NP], n0, n1;
        f32x4 wo;
        auto fetch = [&](int c) {
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int piece = (int)threadIdx.x + 256 * j;
                const int row = piece >> 3, col = c * GM_CHUNK + 2 * (piece & 7);
                xs[j] = (row < H && col < Dh) ? *reinterpret_cast<const f32x2*>(gu + (x0 + row) * Dh + col) : f32x2{0.f, 0.f};
            }
            const int col = c * GM_CHUNK + 4 * as;           // this lane's four columns of the chunk's result (Dh is even: a pair of
                                                             // columns lies within the row or behind it)
            n0 = (live && col < Dh) ? *reinterpret_cast<const f32x2*>(nw + y * Dh + col) : f32x2{0.f, 0.f};
            n1 = (live && col + 2 < Dh) ? *reinterpret_cast<const f32x2*>(nw + y * Dh + col + 2) : f32x2{0.f, 0.f};
            if constexpr (sizeof...(OCC) != 0) {             // nw = na[index] + nt[occ], a + t, as the columns are fetched
                n0 += (live && col < Dh) ? *reinterpret_cast<const f32x2*>(nt + z * Dh + col) : f32x2{0.f, 0.f};
                n1 += (live && col + 2 < Dh) ? *reinterpret_cast<const f32x2*>(nt + z * Dh + col + 2) : f32x2{0.f, 0.f};
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) wo[r] = col + r < Dh ? w_out[col + r] : 0.f;
        };
        float part = 0.f;
        fetch(0);
        for (int c = 0; c < n_chunk; ++c) {
            float* buf = img + (c & 1) * (ROWS * GS);
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int piece = (int)threadIdx.x + 256 * j;
                const int row = piece >> 3, seg = piece & 7;
                if (row < ROWS) *reinterpret_cast<f32x2*>(buf + row * GS + 2 * seg) = xs[j];
            }
            const f32x4 nwc = f32x4{n0[0], n0[1], n1[0], n1[1]}, woc = wo;
            lds_barrier();                                   // (two buffers: the chunk written here was last read two barriers ago)
            if (c + 1 < n_chunk) fetch(c + 1);
            f32x4 acc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = mfma16(buf[(16 * t + 4 * as + r) * GS + ar], a[t][r], acc[r]);
            const f32x4 u = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
            for (int r = 0; r < 4; ++r) part = fmaf(fmaxf(u[r] + nwc[r], 0.f), woc[r], part);
        }
        lds_barrier();                                       // the last chunk is read: the next tile's first product may write img
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (live && lane < 16) logits[p] = part + bias;
    }
}

// The checks and the launch the three entries share.  form GM_PLAIN: qp / nw hold P rows (index unread); GM_INDEXED: tables of n rows;
// GM_OCCURRENCE: those tables plus qt / nt of n_occ rows, read through occ.
int grouped_mlp_match_launch(const char* who, int form, const float* kp, const float* gu, const float* qp, const float* nw, const float* qt,
                             const float* nt, const float* w_out, const float* b_out, const int64_t* offsets, const int32_t* index,
                             int64_t n, const int32_t* occ, int64_t n_occ, float* logits, int64_t G, int64_t P, int32_t H, int32_t A,
                             int32_t Dh, float scale, void* stream) {
    const bool indexed = form != GM_PLAIN, composed = form == GM_OCCURRENCE;
    LIME_REQUIRE(kp && gu && qp && nw && w_out && offsets && logits && (!indexed || index) && (!composed || (qt && nt && occ)),
                 LIME_ERR_BAD_ARG, "%s: NULL pointer", who);
    const bool aligned = lime_al16(kp, A) && lime_al16(qp, A) && (uintptr_t)gu % 8 == 0 && (uintptr_t)nw % 8 == 0 &&
                         (uintptr_t)w_out % 4 == 0 && (uintptr_t)b_out % 4 == 0 && (!composed || (lime_al16(qt, A) && (uintptr_t)nt % 8 == 0));
    if (const int bad = gm_check_shared(who, G, P, H, A, Dh, "Dh", 2, "A a multiple of 4 and Dh even, both", aligned,
                                        "kp and qp (and qt) must be 16-byte aligned, gu and nw (and nt) 8-byte aligned", indexed, n, composed,
                                        n_occ))
        return bad;
    if (G == 0 || P == 0) return LIME_OK;
    const dim3 grid((unsigned)G, (unsigned)gm_tile_slices(G, P));
#define LIME_GMM_LAUNCH(T_, I_)                                                                                                         \
    hipLaunchKernelGGL((grouped_mlp_match_kernel<T_, I_>), grid, dim3(256), 0, (hipStream_t)stream, kp, gu, qp, nw, w_out, b_out,       \
                       (const long*)offsets, (const int*)index, (int)n, logits, (long)P, H, A, Dh, scale)
#define LIME_GMM_LAUNCH_OCC(T_, I_)                                                                                                     \
    hipLaunchKernelGGL((grouped_mlp_match_kernel<T_, I_, GmOccurrence>), grid, dim3(256), 0, (hipStream_t)stream, kp, gu, qp, nw,       \
                       w_out, b_out, (const long*)offsets, (const int*)index, (int)n, logits, (long)P, H, A, Dh, scale,                 \
                       GmOccurrence{qt, nt, (const int*)occ, (int)n_occ})
    if (composed) LIME_GM_PICK(H, LIME_GMM_LAUNCH_OCC, true);
    else if (indexed) LIME_GM_PICK(H, LIME_GMM_LAUNCH, true);
    else LIME_GM_PICK(H, LIME_GMM_LAUNCH, false);
#undef LIME_GMM_LAUNCH_OCC
#undef LIME_GMM_LAUNCH
    return lime_check_launch(who);
}

}  // namespace

extern "C" int lime_grouped_mlp_match_f32(const float* kp, const float* gu, const float* qp, const float* nw, const float* w_out,
                                          const float* b_out, const int64_t* offsets, float* logits, int64_t G, int64_t P, int32_t H,
                                          int32_t A, int32_t Dh, float scale, void* stream) {
    return grouped_mlp_match_launch("lime_grouped_mlp_match_f32", GM_PLAIN, kp, gu, qp, nw, nullptr, nullptr, w_out, b_out, offsets, nullptr,
                                    0, nullptr, 0, logits, G, P, H, A, Dh, scale, stream);
}

extern "C" int lime_grouped_mlp_match_indexed_f32(const float* kp, const float* gu, const float* qp, const float* nw, const float* w_out,
                                                  const float* b_out, const int64_t* offsets, const int32_t* index, int64_t n,
                                                  float* logits, int64_t G, int64_t P, int32_t H, int32_t A, int32_t Dh, float scale,
                                                  void* stream) {
    return grouped_mlp_match_launch("lime_grouped_mlp_match_indexed_f32", GM_INDEXED, kp, gu, qp, nw, nullptr, nullptr, w_out, b_out,
                                    offsets, index, n, nullptr, 0, logits, G, P, H, A, Dh, scale, stream);
}

extern "C" int lime_grouped_mlp_match_occurrence_f32(const float* kp, const float* gu, const float* qa, const float* na, const float* qt,
                                                     const float* nt, const float* w_out, const float* b_out, const int64_t* offsets,
                                                     const int32_t* index, int64_t n, const int32_t* occ, int64_t n_occ, float* logits,
                                                     int64_t G, int64_t P, int32_t H, int32_t A, int32_t Dh, float scale, void* stream) {
    return grouped_mlp_match_launch("lime_grouped_mlp_match_occurrence_f32", GM_OCCURRENCE, kp, gu, qa, na, qt, nt, w_out, b_out, offsets,
                                    index, n, occ, n_occ, logits, G, P, H, A, Dh, scale, stream);
}
