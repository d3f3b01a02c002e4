// What the windowed conv GEMMs share (conv_sp_f32.hip, conv_pool_sp_f32.hip), defined once: the 32-deep chunk and its LDS row pitch, the
// 16 x 16 accumulator tile's operand fragment in both arithmetics (split product / fp32 MFMA), and the source row of a window tap.
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

}  // namespace lime_dev
