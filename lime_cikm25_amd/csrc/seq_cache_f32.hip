// lime_seq_pack_f32 / lime_cne_gate_cached_f32: the two row movers of CNE's per-news recurrence cache (newsEncoders.CNERecurrenceCache).
//
// The LSTM output of a text depends on the news alone, and so does its half of the gate pre-activation, H h_t (newsEncoders.py:517-518 of
// the reference).  The cache keeps both for the LIVE tokens only, packed: news i owns rows offsets[i] .. offsets[i] + lens[i] - 1.
//     pack : dst[offsets[i] + t, :] = src[i S + t, :]                                            t < lens[i]       (building the cache)
//     gate : out[r S + t, :] = h[offsets[j] + t, :] * sigmoid(hh[offsets[j] + t, :] + tm[r, :])  t < lens[j], else 0;  j = idx[r]
// The gate is the per-batch hot path: it stands for the H GEMM with the memory term as a residual, the dense copy of hout and
// lime_gate_mul_f32 -- one launch that reads every live token once and writes every slot once (rows behind a length as zeros: the
// attention GEMM behind it reads all of them).  Both are bandwidth bound: 16 bytes moved per lane and step, ~ 10 flops.
//
// Launch form: a wave owns one (slot, token) row at a time -- blockIdx.y strides over the slots, the four waves of the workgroups of a
// grid row over the tokens -- so idx / lens / offsets are wave-uniform scalar loads and the row's C / 4 column groups go to the lanes
// as 16-byte pieces, 64 at a step.  Row and element offsets are 64-bit (sum(lens) C passes 2^31 on a real corpus).  No LDS, no atomics;
// every output element is one fixed expression of its own operands: its bits depend neither on the slot, on n_rows_dev nor on the grid.
#include "common.h"
#include "dev_helpers.h"

namespace {

constexpr int WAVES = 4;                             // waves (= token rows in flight) of a workgroup
constexpr int MAX_TOKEN_GROUPS = 8;                  // workgroups along the tokens of a slot: a wave then takes S / 32 rows of its slot

__global__ __launch_bounds__(256) void seq_pack_kernel(const float* __restrict__ src, const int* __restrict__ lens,
                                                       const long* __restrict__ offsets, float* __restrict__ dst, int n, int S, int C4) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        const int len = lens[i] < S ? lens[i] : S;
        const long d0 = offsets[i];
        for (int t = blockIdx.x * WAVES + wave; t < len; t += gridDim.x * WAVES) {
            const f32x4* s = reinterpret_cast<const f32x4*>(src) + ((long)i * S + t) * C4;
            f32x4* d = reinterpret_cast<f32x4*>(dst) + (d0 + t) * C4;
            for (int c = lane; c < C4; c += 64) d[c] = s[c];
        }
    }
}

__global__ __launch_bounds__(256) void cne_gate_cached_kernel(const float* __restrict__ h, const float* __restrict__ hh,
                                                              const long* __restrict__ offsets, const int* __restrict__ lens,
                                                              const int* __restrict__ idx, const float* __restrict__ tm,
                                                              float* __restrict__ out, int cap, int S, int C4,
                                                              const int* __restrict__ n_rows_dev) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = lime_dev::live_count(n_rows_dev, cap);
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = blockIdx.y; r < n; r += gridDim.y) {
        const long j = idx[r];
        const int len = lens[j];
        const long s0 = offsets[j];
        const f32x4* m4 = reinterpret_cast<const f32x4*>(tm) + (long)r * C4;
        for (int t = blockIdx.x * WAVES + wave; t < S; t += gridDim.x * WAVES) {
            f32x4* o = reinterpret_cast<f32x4*>(out) + ((long)r * S + t) * C4;
            if (t >= len) {                          // behind the length: zeros, nothing is read
                for (int c = lane; c < C4; c += 64) o[c] = zero4;
                continue;
            }
            const f32x4* hv = reinterpret_cast<const f32x4*>(h) + (s0 + t) * C4;
            const f32x4* pv = reinterpret_cast<const f32x4*>(hh) + (s0 + t) * C4;
            for (int c = lane; c < C4; c += 64) {
                const f32x4 x = hv[c], p = pv[c], m = m4[c];
                f32x4 g;
#pragma unroll
                for (int k = 0; k < 4; ++k) g[k] = x[k] * lime_sigmoid(p[k] + m[k]);
                o[c] = g;
            }
        }
    }
}

// workgroups along the tokens (x) and the slots (y, the kernel strides over what the grid limit leaves out)
dim3 seq_grid(int rows, int S) {
    const int tg = (S + WAVES - 1) / WAVES;
    return dim3((unsigned)(tg < MAX_TOKEN_GROUPS ? tg : MAX_TOKEN_GROUPS), (unsigned)(rows < 65535 ? rows : 65535));
}

}  // namespace

extern "C" int lime_seq_pack_f32(const float* src, const int32_t* lens, const int64_t* offsets, float* dst, int32_t n, int32_t S, int32_t C,
                                 void* stream) {
    LIME_REQUIRE(src && lens && offsets && dst, LIME_ERR_BAD_ARG, "lime_seq_pack_f32: NULL pointer");
    LIME_REQUIRE(n >= 0 && S >= 1 && C > 0 && C % 4 == 0, LIME_ERR_BAD_ARG,
                 "lime_seq_pack_f32: bad dims n=%d S=%d C=%d (S >= 1, C a positive multiple of 4)", n, S, C);
    LIME_REQUIRE(lime_al16(src, C) && lime_al16(dst, C) && (uintptr_t)offsets % 8 == 0, LIME_ERR_BAD_ARG,
                 "lime_seq_pack_f32: src and dst must be 16-byte aligned, offsets 8-byte aligned");
    if (n == 0) return LIME_OK;
    hipLaunchKernelGGL(seq_pack_kernel, seq_grid(n, S), dim3(256), 0, (hipStream_t)stream, src, lens, (const long*)offsets, dst, n, S, C / 4);
    return lime_check_launch("lime_seq_pack_f32");
}

extern "C" int lime_cne_gate_cached_f32(const float* h, const float* hh, const int64_t* offsets, const int32_t* lens, const int32_t* idx,
                                        const float* tm, float* out, int32_t cap, int32_t S, int32_t C, const int32_t* n_rows_dev,
                                        void* stream) {
    LIME_REQUIRE(h && hh && offsets && lens && idx && tm && out, LIME_ERR_BAD_ARG, "lime_cne_gate_cached_f32: NULL pointer");
    LIME_REQUIRE(cap >= 0 && S >= 1 && C > 0 && C % 4 == 0, LIME_ERR_BAD_ARG,
                 "lime_cne_gate_cached_f32: bad dims cap=%d S=%d C=%d (cap >= 0, S >= 1, C a positive multiple of 4)", cap, S, C);
    LIME_REQUIRE(lime_al16(h, C) && lime_al16(hh, C) && lime_al16(tm, C) && lime_al16(out, C) && (uintptr_t)offsets % 8 == 0, LIME_ERR_BAD_ARG,
                 "lime_cne_gate_cached_f32: h, hh, tm and out must be 16-byte aligned, offsets 8-byte aligned");
    if (cap == 0) return LIME_OK;
    hipLaunchKernelGGL(cne_gate_cached_kernel, seq_grid(cap, S), dim3(256), 0, (hipStream_t)stream, h, hh, (const long*)offsets, lens, idx, tm,
                       out, cap, S, C / 4, n_rows_dev);
    return lime_check_launch("lime_cne_gate_cached_f32");
}
