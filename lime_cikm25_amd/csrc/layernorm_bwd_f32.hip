// lime_layernorm_bwd_f32 / lime_layernorm_bwd_dropout_f32 / lime_relu_bwd_f32: the backward of the encoder layers' LayerNorm and ReLU.
//
//   layernorm_bwd_kernel / _vec_kernel   dZ of y = LayerNorm(z) from (dY, y, rstd) + per-workgroup column sums for d gamma / d beta / bias
//   reduce_ln3_kernel                    those three column sums in one launch, in a fixed order
//   relu_bwd_kernel                      dH *= (h > 0)
#include "common.h"
#include "dropout.h"
#include "gemm_pp.h"

namespace {

// The three column sums of layernorm_bwd (dgamma, dbeta, dzsum) out of its per-workgroup partials ws[blk][3][E] in ONE launch:
// a workgroup owns 16 groups of four consecutive floats of the 3 E, its 16 split lanes take the blocks s, s + 16, ... (up to 768
// blocks: 48 independent 16-byte loads per thread instead of 192 dependent-issue ones in two workgroups, 18 us per vector) and their
// sums meet in LDS in a fixed order.  E % 4 == 0.
__global__ __launch_bounds__(256) void reduce_ln3_kernel(const float* __restrict__ ws, int nblk, int E, float* __restrict__ o0,
                                                          float* __restrict__ o1, float* __restrict__ o2, int accumulate) {
    __shared__ f32x4 red[16][16];
    const int cg = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const int g = blockIdx.x * 16 + cg, ng = 3 * E / 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (g < ng) {
        const float* p = ws + 4L * g;
        int i = sl;
        for (; i + 48 < nblk; i += 64) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(p + (long)(i + 16 * u) * 3 * E);
#pragma unroll
            for (int u = 0; u < 4; ++u) s += v[u];
        }
        for (; i < nblk; i += 16) s += *reinterpret_cast<const f32x4*>(p + (long)i * 3 * E);
    }
    red[sl][cg] = s;
    __syncthreads();
    if (sl == 0 && g < ng) {
        f32x4 t = red[0][cg];
#pragma unroll
        for (int u = 1; u < 16; ++u) t += red[u][cg];
        const int c = 4 * g, k = c / E, cc = c - k * E;          // E % 4 == 0: a group never leaves its vector
        float* const o = k == 0 ? o0 : (k == 1 ? o1 : o2);
        if (o) {
            f32x4* q = reinterpret_cast<f32x4*>(o + cc);
            *q = accumulate ? *q + t : t;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// LayerNorm backward.  y = gamma * xhat + beta with xhat = (z - mean) * rstd; given dY, y and rstd:
//   g = dY * gamma;  dZ = rstd * (g - mean(g) - xhat * mean(g * xhat)),   xhat = (y - beta) / gamma
// dY row of output row r is dy[(r / dy_div)] * dy_scale (the mean-pool backward of newsEncoders.py:317,321 broadcasts one
// pooled-gradient row over the S tokens with 1 / S).  One wave per row, CPL columns per lane; partial column sums
// (d gamma, d beta, sum dZ) per workgroup in ws[blk][3][E].
// ---------------------------------------------------------------------------------------------------
template <int CPL>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, long lddy, int dy_div, float dy_scale,
                                                             const float* __restrict__ y, long ldy, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ rstd,
                                                             float* __restrict__ dz, long lddz, int M, int E,
                                                             float* __restrict__ ws) {
    __shared__ float red[4][3][64 * CPL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ga[CPL], be[CPL], inv_ga[CPL], sg[CPL], sb[CPL], sz[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        const int c = lane + 64 * j;
        ga[j] = c < E ? gamma[c] : 0.f;
        be[j] = c < E ? beta[c] : 0.f;
        inv_ga[j] = c < E ? 1.0f / ga[j] : 0.f;
        sg[j] = sb[j] = sz[j] = 0.f;
    }
    const float inv_e = 1.0f / (float)E;
    for (long r = (long)blockIdx.x * 4 + wave; r < M; r += (long)gridDim.x * 4) {
        const float* pdy = dy + (r / dy_div) * lddy;
        const float* py = y + r * ldy;
        float d[CPL], xh[CPL];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + 64 * j;
            d[j] = c < E ? pdy[c] * dy_scale : 0.f;
            xh[j] = c < E ? (py[c] - be[j]) * inv_ga[j] : 0.f;
            const float g = d[j] * ga[j];
            s1 += g;
            s2 += g * xh[j];
        }
        s1 = wave_sum(s1) * inv_e;
        s2 = wave_sum(s2) * inv_e;
        const float rs = rstd[r];
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + 64 * j;
            const float v = rs * (d[j] * ga[j] - s1 - xh[j] * s2);
            if (c < E) dz[r * lddz + c] = v;
            sg[j] += d[j] * xh[j];
            sb[j] += d[j];
            sz[j] += c < E ? v : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
        red[wave][0][lane + 64 * j] = sg[j];
        red[wave][1][lane + 64 * j] = sb[j];
        red[wave][2][lane + 64 * j] = sz[j];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * E; e += 256) {
        const int k = e / E, c = e - k * E;
        ws[((long)blockIdx.x * 3 + k) * E + c] = red[0][k][c] + red[1][k][c] + red[2][k][c] + red[3][k][c];
    }
}

// The same with 16 lanes per row (four rows per wave at a time) and 16-byte accesses: E % 4 == 0, 16-byte aligned rows.
template <int V4>        // float4 per lane: ceil(E / 64)
__global__ __launch_bounds__(256) void layernorm_bwd_vec_kernel(const float* __restrict__ dy, long lddy, int dy_div, float dy_scale,
                                                                 const float* __restrict__ y, long ldy,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ rstd, float* __restrict__ dz, long lddz,
                                                                 int M, int E, float* __restrict__ ws,
                                                                 float* __restrict__ dz_drop, long lddd, LimeDropout drop) {
    __shared__ float red[4][3][64 * V4];
    __shared__ __attribute__((aligned(16))) float Gs[64 * V4], Bs[64 * V4], IGs[64 * V4];   // gamma, beta, 1 / gamma (registers are
                                                                                          // for the column sums: occupancy)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rg = lane >> 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int c = threadIdx.x; c < 64 * V4; c += 256) {
        const float g = c < E ? gamma[c] : 0.f;
        Gs[c] = g;
        Bs[c] = c < E ? beta[c] : 0.f;
        IGs[c] = c < E ? 1.0f / g : 0.f;
    }
    __syncthreads();
    f32x4 sg[V4], sb[V4], sz[V4];
#pragma unroll
    for (int j = 0; j < V4; ++j) sg[j] = sb[j] = sz[j] = zero;
    const float inv_e = 1.0f / (float)E;
    for (long r4 = ((long)blockIdx.x * 4 + wave) * 4; r4 < M; r4 += (long)gridDim.x * 16) {
        const long r = r4 + rg;
        const bool rin = r < M;
        const float* pdy = dy + ((rin ? r : 0) / dy_div) * lddy;
        const float* py = y + (rin ? r : 0) * ldy;
        f32x4 d[V4], xh[V4];
        float s1 = 0.f, s2 = 0.f;
        // the three vectors are re-read from LDS for every row: hidden from the optimiser, which would otherwise hoist the
        // loop-invariant loads back into 60 registers
        const float *gs = Gs, *bs = Bs, *igs = IGs;
        asm volatile("" : "+v"(gs), "+v"(bs), "+v"(igs));
#pragma unroll
        for (int j = 0; j < V4; ++j) {
            const int c = 4 * (sub + 16 * j);
            const bool ok = rin && c < E;
            const f32x4 ga = *reinterpret_cast<const f32x4*>(&gs[c]), be = *reinterpret_cast<const f32x4*>(&bs[c]);
            d[j] = ok ? *reinterpret_cast<const f32x4*>(pdy + c) * dy_scale : zero;
            const f32x4 yv = ok ? *reinterpret_cast<const f32x4*>(py + c) : be;
            xh[j] = (yv - be) * *reinterpret_cast<const f32x4*>(&igs[c]);
            const f32x4 g = d[j] * ga;
#pragma unroll
            for (int e = 0; e < 4; ++e) { s1 += g[e]; s2 += g[e] * xh[j][e]; }
        }
        s1 += __shfl_xor(s1, 1); s2 += __shfl_xor(s2, 1);
        s1 += __shfl_xor(s1, 2); s2 += __shfl_xor(s2, 2);
        s1 += __shfl_xor(s1, 4); s2 += __shfl_xor(s2, 4);
        s1 += __shfl_xor(s1, 8); s2 += __shfl_xor(s2, 8);
        s1 *= inv_e; s2 *= inv_e;
        const float rs = rin ? rstd[r] : 0.f;
#pragma unroll
        for (int j = 0; j < V4; ++j) {
            const int c = 4 * (sub + 16 * j);
            const bool ok = rin && c < E;
            f32x4 v = (d[j] * *reinterpret_cast<const f32x4*>(&gs[c]) - s1 - xh[j] * s2) * rs;
            if (!ok) v = zero;
            if (ok) *reinterpret_cast<f32x4*>(dz + r * lddz + c) = v;
            f32x4 t = v;
            if (dz_drop != nullptr && ok) {            // the gradient through the dropout in front of the residual add, written alongside
                const unsigned keep = lime_keep4(drop, ((uint64_t)r * (uint64_t)E + (uint64_t)c) >> 2);
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = (keep >> e) & 1u ? v[e] * drop.scale : 0.f;
                *reinterpret_cast<f32x4*>(dz_drop + r * lddd + c) = t;
            }
            sg[j] += d[j] * xh[j];
            sb[j] += d[j];
            sz[j] += t;                                // column sums of what goes on to the linear in front: its bias gradient
        }
    }
    // the four row groups of the wave, then the four waves
#pragma unroll
    for (int j = 0; j < V4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = sg[j][e], b = sb[j][e], c = sz[j][e];
            a += __shfl_xor(a, 16); b += __shfl_xor(b, 16); c += __shfl_xor(c, 16);
            a += __shfl_xor(a, 32); b += __shfl_xor(b, 32); c += __shfl_xor(c, 32);
            if (rg == 0) {
                const int col = 4 * (sub + 16 * j) + e;
                red[wave][0][col] = a; red[wave][1][col] = b; red[wave][2][col] = c;
            }
        }
    __syncthreads();
    for (int e = threadIdx.x; e < 3 * E; e += 256) {
        const int k = e / E, c = e - k * E;
        ws[((long)blockIdx.x * 3 + k) * E + c] = (red[0][k][c] + red[1][k][c]) + (red[2][k][c] + red[3][k][c]);
    }
}

__global__ __launch_bounds__(256) void relu_bwd_kernel(float* __restrict__ dh, long lddh, const float* __restrict__ h, long ldh,
                                                        long rows, int cols, float scale) {
    const long total = rows * cols;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / cols;
        const int c = (int)(e - r * cols);
        const float g = dh[r * lddh + c];
        dh[r * lddh + c] = h[r * ldh + c] > 0.f ? g * scale : 0.f;
    }
}

int ln_blocks(int M) { const int b = (M + 15) / 16; return b > 768 ? 768 : b; }   // persistent: 3 workgroups per CU

}  // namespace

extern "C" int64_t lime_layernorm_bwd_workspace(int32_t M, int32_t E) {
    if (M <= 0 || E <= 0) return 0;
    return (int64_t)ln_blocks(M) * 3 * E;
}

static int layernorm_bwd(const float* dy, int64_t lddy, int32_t dy_div, float dy_scale, const float* y, int64_t ldy,
                         const float* gamma, const float* beta, const float* rstd, float* dz, int64_t lddz,
                         int32_t M, int32_t E, float* dgamma, float* dbeta, float* dzsum, int32_t accumulate,
                         float* workspace, int64_t workspace_floats, float* dz_drop, int64_t lddd, const LimeDropout& drop, void* stream) {
    LIME_REQUIRE(dy && y && gamma && beta && rstd && dz && workspace, LIME_ERR_BAD_ARG, "lime_layernorm_bwd_f32: null pointer");
    LIME_REQUIRE(M > 0 && E > 0 && dy_div >= 1, LIME_ERR_BAD_ARG, "lime_layernorm_bwd_f32: bad dimensions");
    LIME_REQUIRE(E <= 512, LIME_ERR_UNSUPPORTED, "lime_layernorm_bwd_f32: E = %d > 512", E);
    LIME_REQUIRE(lddy >= E && ldy >= E && lddz >= E, LIME_ERR_BAD_ARG, "lime_layernorm_bwd_f32: leading dimension smaller than E");
    const int nblk = ln_blocks(M);
    LIME_REQUIRE(workspace_floats >= (int64_t)nblk * 3 * E, LIME_ERR_BAD_ARG, "lime_layernorm_bwd_f32: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = E % 4 == 0 && lddy % 4 == 0 && ldy % 4 == 0 && lddz % 4 == 0 &&
                     ((((uintptr_t)dy) | ((uintptr_t)y) | ((uintptr_t)dz) | ((uintptr_t)gamma) | ((uintptr_t)beta)) & 15) == 0;
    LIME_REQUIRE(dz_drop == nullptr || (vec && lime_al16(dz_drop, lddd) && lddd >= E), LIME_ERR_UNSUPPORTED,
                 "lime_layernorm_bwd_dropout_f32: the dropped copy needs 16-byte friendly operands (E, leading dimensions multiples of 4)");
    if (vec) {
        const int v4 = (E + 63) / 64;
#define LN_BWD_V(C) layernorm_bwd_vec_kernel<C><<<nblk, 256, 0, s>>>(dy, lddy, dy_div, dy_scale, y, ldy, gamma, beta, rstd, dz, lddz, M, E, workspace, dz_drop, lddd, drop)
        if (v4 <= 2) LN_BWD_V(2); else if (v4 <= 5) LN_BWD_V(5); else LN_BWD_V(8);
#undef LN_BWD_V
    } else {
        const int cpl = (E + 63) / 64;
#define LN_BWD(C) layernorm_bwd_kernel<C><<<nblk, 256, 0, s>>>(dy, lddy, dy_div, dy_scale, y, ldy, gamma, beta, rstd, dz, lddz, M, E, workspace)
        if (cpl <= 2) LN_BWD(2); else if (cpl <= 5) LN_BWD(5); else LN_BWD(8);
#undef LN_BWD
    }
    int st = lime_check_launch("layernorm_bwd_kernel");
    if (st != LIME_OK) return st;
    if (E % 4 == 0 && ((((uintptr_t)dgamma) | ((uintptr_t)dbeta) | ((uintptr_t)dzsum) | ((uintptr_t)workspace)) & 15) == 0) {
        reduce_ln3_kernel<<<(3 * E / 4 + 15) / 16, 256, 0, s>>>(workspace, nblk, E, dgamma, dbeta, dzsum, accumulate);
        return lime_check_launch("reduce_ln3_kernel");
    }
    float* outs[3] = {dgamma, dbeta, dzsum};
    for (int k = 0; k < 3; ++k) {
        if (!outs[k]) continue;
        st = lime_reduce_partials(workspace + (long)k * E, 3L * E, nblk, E, outs[k], E, 1, E, accumulate, s);
        if (st != LIME_OK) return st;
    }
    return LIME_OK;
}

extern "C" int lime_layernorm_bwd_f32(const float* dy, int64_t lddy, int32_t dy_div, float dy_scale, const float* y, int64_t ldy,
                                      const float* gamma, const float* beta, const float* rstd, float* dz, int64_t lddz,
                                      int32_t M, int32_t E, float* dgamma, float* dbeta, float* dzsum, int32_t accumulate,
                                      float* workspace, int64_t workspace_floats, void* stream) {
    return layernorm_bwd(dy, lddy, dy_div, dy_scale, y, ldy, gamma, beta, rstd, dz, lddz, M, E, dgamma, dbeta, dzsum, accumulate, workspace,
                         workspace_floats, nullptr, 0, lime_make_dropout(0.f, 0, 0), stream);
}

extern "C" int lime_layernorm_bwd_dropout_f32(const float* dy, int64_t lddy, int32_t dy_div, float dy_scale, const float* y, int64_t ldy,
                                              const float* gamma, const float* beta, const float* rstd, float* dz, int64_t lddz,
                                              int32_t M, int32_t E, float* dgamma, float* dbeta, float* dzsum, int32_t accumulate,
                                              float* workspace, int64_t workspace_floats, float* dz_drop, int64_t lddd, float dropout_p,
                                              uint64_t seed, uint32_t site, void* stream) {
    LIME_REQUIRE(dz_drop != nullptr, LIME_ERR_BAD_ARG, "lime_layernorm_bwd_dropout_f32: dz_drop is NULL");
    LIME_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, LIME_ERR_BAD_ARG, "lime_layernorm_bwd_dropout_f32: dropout_p outside [0, 1)");
    return layernorm_bwd(dy, lddy, dy_div, dy_scale, y, ldy, gamma, beta, rstd, dz, lddz, M, E, dgamma, dbeta, dzsum, accumulate, workspace,
                         workspace_floats, dz_drop, lddd, lime_make_dropout(dropout_p, seed, site), stream);
}

extern "C" int lime_relu_bwd_f32(float* dh, int64_t lddh, const float* h, int64_t ldh, int64_t rows, int32_t cols, float scale,
                                 void* stream) {
    LIME_REQUIRE(dh && h, LIME_ERR_BAD_ARG, "lime_relu_bwd_f32: null pointer");
    LIME_REQUIRE(rows >= 0 && cols > 0 && lddh >= cols && ldh >= cols, LIME_ERR_BAD_ARG, "lime_relu_bwd_f32: bad dimensions");
    if (rows == 0) return LIME_OK;
    relu_bwd_kernel<<<lime_grid_cap(rows * cols, 256, 8192), 256, 0, (hipStream_t)stream>>>(dh, lddh, h, ldh, rows, cols, scale);
    return lime_check_launch("relu_bwd_kernel");
}
