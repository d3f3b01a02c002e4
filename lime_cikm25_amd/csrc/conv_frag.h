// What the windowed conv GEMMs share (conv_sp_f32.hip, conv_pool_sp_f32.hip), defined once: the 32-deep chunk and its LDS row pitch, the
// 16 x 16 accumulator tile's operand fragment in both arithmetics (split product / fp32 MFMA), the source row of a window tap, the
// two-stage chunk loop, and the 128 x 128 tile product over (tap, chunk) that conv_sp_kernel and conv_pool_sp_kernel put their
// epilogues behind.
#pragma once
#include "common.h"
#include "dev_helpers.h"
#include "split_mfma.h"

namespace lime_dev {

constexpr int CONV_KC = 32;             // chunk depth (one bf16 MFMA's k)
constexpr int CONV_PITCH = 36;          // floats per LDS row: 32 + 4 (conflict-free 16-byte reads of 16 rows)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// the 32-deep product of one chunk for one 16 x 16 accumulator tile: w = eight k values of output column fi, x = eight k values of
// row fi (lane group kg: k = 8 kg .. 8 kg + 7)
template <bool SPLIT>
struct Frag;
template <>
struct Frag<true> {
    SplitFrag f;
    __device__ __forceinline__ void load_frag(const float* p) { f = split_frag(ld4(p), ld4(p + 4)); }
};
template <>
struct Frag<false> {
    float x[8];
    __device__ __forceinline__ void load_frag(const float* p) {
        const f32x4 a = ld4(p), b = ld4(p + 4);
        x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3];
        x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
    }
};
__device__ __forceinline__ f32x4 frag_prod(const Frag<true>& w, const Frag<true>& x, f32x4 c) { return split_mfma16(w.f, x.f, c); }
// v_mfma_f32_16x16x4_f32: lane (fi, kg) supplies A[fi][kg] and B[kg][fi]; product q takes k = 8 kg + q in slot kg (the same label
// on both operands)
__device__ __forceinline__ f32x4 frag_prod(const Frag<false>& w, const Frag<false>& x, f32x4 c) {
#pragma unroll
    for (int q = 0; q < 8; ++q) c = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x[q], x.x[q], c, 0, 0, 0);
    return c;
}

// source row of output row r under tap j (window offset j - pad), as a float offset into a / the table, or -1: zeros
__device__ __forceinline__ long window_row(const int* ids, long lda, int r, int j, int pad, int T) {
    const int s = r / T, t = r - s * T, tt = t + j - pad;
    if (tt < 0 || tt >= T) return -1;
    const int q = r + j - pad;
    return (long)(ids ? ids[q] : q) * lda;
}

// The two-stage chunk loop: chunk k + 1's global loads are in flight under chunk k's products, one barrier per chunk.  nk >= 1.
template <class Load, class Store, class Compute>
__device__ __forceinline__ void two_stage_loop(int nk, Load&& gload, Store&& sstore, Compute&& compute) {
    gload(0);
    sstore(0);
    lds_barrier();
    for (int k = 0; k < nk; ++k) {
        const bool more = k + 1 < nk;
        if (more) gload(k + 1);                        // in flight under this chunk's products
        compute(k & 1);
        if (more) sstore((k + 1) & 1);                 // the other stage: its last reader finished before the previous barrier
        lds_barrier();
    }
}

// ---- the windowed tile product ------------------------------------------------------------------------------------------
// 256 threads (four waves), tile 128 rows x 128 columns, wave w owns rows 64 (w & 1) .. + 63 and columns 64 (w >> 1) .. + 63: 4 x 4
// accumulator tiles of 16 x 16, the transposed product D^T = W A^T so that a lane holds four consecutive output columns of one row.
// Chunks go global -> registers -> LDS (fp32, CONV_PITCH-float rows), two stages: 74 KB.
constexpr int CONV_BM = 128;
constexpr int CONV_BN = 128;
constexpr int CONV_A_FL = CONV_BM * CONV_PITCH;
constexpr int CONV_W_FL = CONV_BN * CONV_PITCH;
constexpr int CONV_STAGE = CONV_A_FL + CONV_W_FL;
static_assert(2 * CONV_STAGE * 4 <= 81920, "two workgroups per CU");

// what tap(sj) returns for the weight's tap block sj: the source the tap reads and its window offset j
struct ConvTap {
    const float* a;
    long lda;
    const int* ids;
    int j;
};

// acc = sum over the n_taps tap blocks sj and the 32-deep chunks of the C source columns of A(r, tap(sj))[c] W[n, sj C + c], for the
// rows row0 .. row0 + 127 that are < row_end (the others read zeros) and the columns col0 .. col0 + 127 that are < N.  lds: the
// kernel's 2 * CONV_STAGE floats; every reader is past the last barrier on return.  Lane (fi = lane & 15, kg = lane >> 4) of wave
// (wr = wave & 1, wc = wave >> 1) holds row 64 wr + 16 i + fi, columns 64 wc + 16 t + 4 kg + e in acc[i][t][e].
template <bool SPLIT, class Tap>
__device__ __forceinline__ void conv_tile_product(float* lds, f32x4 (&acc)[4][4], Tap&& tap, int n_taps, const float* w, long ldw, int C,
                                                  int N, int T, int pad, int row0, int row_end, int col0) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave & 1, wc = wave >> 1;
    const int fi = lane & 15, kg = lane >> 4;
    const int seg = tid & 7, lrow = tid >> 3;          // loader: rows lrow + 32 u of the tile, floats 4 seg .. + 3 of the chunk
    const int nq = (C + CONV_KC - 1) / CONV_KC, nk = n_taps * nq;

    long aoff[4];
    const float* asrc = nullptr;
    f32x4 ra[4], rw[4];
    auto gload = [&](int k) {
        const int sj = k / nq, q = k - sj * nq;
        if (q == 0) {                                  // a new tap: the four source rows of this thread
            const ConvTap s = tap(sj);
            asrc = s.a;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = row0 + lrow + 32 * u;
                aoff[u] = r < row_end ? window_row(s.ids, s.lda, r, s.j, pad, T) : -1;
            }
        }
        const int c = q * CONV_KC + 4 * seg;
        const bool cin = c < C;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) ra[u] = (cin && aoff[u] >= 0) ? ld4(asrc + aoff[u] + c) : z;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int n = col0 + lrow + 32 * u;
            rw[u] = (cin && n < N) ? ld4(w + (long)n * ldw + (long)sj * C + c) : z;
        }
    };
    auto sstore = [&](int st) {
        float* const s = lds + st * CONV_STAGE;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            *reinterpret_cast<f32x4*>(s + (lrow + 32 * u) * CONV_PITCH + 4 * seg) = ra[u];
            *reinterpret_cast<f32x4*>(s + CONV_A_FL + (lrow + 32 * u) * CONV_PITCH + 4 * seg) = rw[u];
        }
    };

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto compute = [&](int st) {
        const float* const sa = lds + st * CONV_STAGE + (64 * wr + fi) * CONV_PITCH + 8 * kg;
        const float* const sw = lds + st * CONV_STAGE + CONV_A_FL + (64 * wc + fi) * CONV_PITCH + 8 * kg;
        Frag<SPLIT> x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i].load_frag(sa + i * 16 * CONV_PITCH);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            Frag<SPLIT> wf;
            wf.load_frag(sw + t * 16 * CONV_PITCH);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][t] = frag_prod(wf, x[i], acc[i][t]);
        }
    };
    two_stage_loop(nk, gload, sstore, compute);
}

}  // namespace lime_dev
