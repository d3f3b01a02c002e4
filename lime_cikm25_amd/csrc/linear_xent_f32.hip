// lime_linear_xent_f32: a linear classifier and its cross-entropy in one launch -- CROWN's category predictor on the title intent
// vector (reference newsEncoders.py:358-364, CategoryPredictor :375-393; F.cross_entropy on a one-hot probability target):
//     z[c]       = x[r, :] . w[c, :] + b[c]
//     row_loss   = scale (logsumexp(z) - z[target])               (max-subtracted)
//     dlogits[c] = scale (softmax(z)[c] - [c == target])
//     dx[r, :]   = sum_c dlogits[c] w[c, :]
// A target outside [0, C) is the all-zero one-hot row: the row's loss and both of its gradients are exact zeros.
//
// A wave owns a row, four rows per workgroup pass, the workgroups stride over the rows.  The row of x stays in the lanes' registers
// (lane l holds the float4 groups l, l + 64, ...) for the C dot products and is not read again; rows wider than 2048 columns are
// streamed a second time instead (NQ = 0).  w is staged once per workgroup in LDS, rows padded with zeros to whole float4 groups,
// while C * ceil(D / 4) * 16 bytes fit 64 KB (the model: 18 x 400 floats = 28.8 KB); a larger w is read through L2 in the same order.
// The logits live in registers as well: class c on lane c % 64 of register c / 64, handed to the softmax without LDS and to the
// dx sum by a lane broadcast.
// Every sum has fixed operands in a fixed order -- a logit is the lane's own float4 groups in rising order, then the wave shuffle tree;
// the softmax denominator the lane's registers in rising order, then the tree; a column of dx a serial sum over the classes -- and
// every multiply-add is an explicit fmaf, so a row's bits depend on neither M, the row's place, the route of w nor the run.  No atomics.
// 16-byte loads and stores when D % 4 == 0 and x, w, dx (with their leading dimensions) allow (VEC), the same lane-to-element assignment
// otherwise.
#include "common.h"

namespace {

// the store that goes with row_quad (common.h): elements behind the end of the row are dropped
template <bool VEC>
__device__ __forceinline__ void store_quad(float* __restrict__ p, int j, int n, f32x4 v) {
    if (VEC) {
        *reinterpret_cast<f32x4*>(p + 4 * (long)j) = v;
        return;
    }
    const long e = 4 * (long)j;
    if (e < n) p[e] = v.x;
    if (e + 1 < n) p[e + 1] = v.y;
    if (e + 2 < n) p[e + 2] = v.z;
    if (e + 3 < n) p[e + 3] = v.w;
}

// float4 group j of class c of w: from the LDS copy (rows of D4 whole groups) or from memory
template <bool VEC, bool WLDS>
__device__ __forceinline__ f32x4 w_quad(const float* __restrict__ w, const float* sm, int c, int j, int D, int D4) {
    if (WLDS) return *reinterpret_cast<const f32x4*>(sm + 4 * (c * D4 + j));
    return row_quad<VEC>(w + (long)c * D, (long)j, D);
}

// NQ: float4 groups of x a lane keeps (D <= 256 NQ), 0: the row is streamed.  CK: registers of logits a lane keeps (C <= 64 CK).
template <int NQ, int CK, bool VEC, bool WLDS>
__global__ __launch_bounds__(256) void linear_xent_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ w,
                                                           const float* __restrict__ b, const int* __restrict__ target, float scale,
                                                           float* __restrict__ row_loss, float* __restrict__ dlogits,
                                                           float* __restrict__ dx, long lddx, int M, int D, int C) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D4 = (D + 3) >> 2;
    constexpr int NX = NQ > 0 ? NQ : 1;
    if (WLDS) {
        for (int e = threadIdx.x; e < C * D4; e += 256) {
            const int c = e / D4;
            *reinterpret_cast<f32x4*>(sm + 4 * e) = row_quad<VEC>(w + (long)c * D, (long)(e - c * D4), D);
        }
        __syncthreads();
    }
    for (long row = (long)blockIdx.x * 4 + wave; row < M; row += (long)gridDim.x * 4) {
        const float* xr = x + row * ldx;
        const int t = target[row];
        const bool hit = t >= 0 && t < C;
        f32x4 xv[NX];
        if constexpr (NQ > 0) {
#pragma unroll
            for (int q = 0; q < NX; ++q) {
                const int j = lane + 64 * q;
                xv[q] = j < D4 ? row_quad<VEC>(xr, (long)j, D) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        // the logits, four classes in flight: class 64 k + cc lands on lane cc of zr[k]
        float zr[CK];
#pragma unroll
        for (int k = 0; k < CK; ++k) {
            zr[k] = -INFINITY;
            const int cend = C - 64 * k < 64 ? C - 64 * k : 64;
            for (int cc = 0; cc < cend; cc += 4) {
                const int c0 = 64 * k + cc;
                float part[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (NQ > 0) {
#pragma unroll
                    for (int q = 0; q < NX; ++q) {
                        const int j = lane + 64 * q;
                        if (j < D4) {
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (cc + u < cend) part[u] = fma_dot4(xv[q], w_quad<VEC, WLDS>(w, sm, c0 + u, j, D, D4), part[u]);
                        }
                    }
                } else {
                    for (int j = lane; j < D4; j += 64) {
                        const f32x4 xq = row_quad<VEC>(xr, (long)j, D);
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (cc + u < cend) part[u] = fma_dot4(xq, w_quad<VEC, WLDS>(w, sm, c0 + u, j, D, D4), part[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (cc + u < cend) {
                        float z = wave_sum(part[u]);
                        if (b != nullptr) z += b[c0 + u];
                        if (lane == cc + u) zr[k] = z;
                    }
                }
            }
        }
        // the max-subtracted log-sum-exp; lanes behind the last class hold -inf and add exp(-inf) = 0
        float mx = zr[0];
#pragma unroll
        for (int k = 1; k < CK; ++k) mx = fmaxf(mx, zr[k]);
        mx = wave_max(mx);
        float den = 0.f;
#pragma unroll
        for (int k = 0; k < CK; ++k) den += expf(zr[k] - mx);
        den = wave_sum(den);
        const float inv = 1.0f / den;
        float zt = 0.f;
#pragma unroll
        for (int k = 0; k < CK; ++k) {
            const float v = __shfl(zr[k], t & 63);
            if (hit && (t >> 6) == k) zt = v;
        }
        if (lane == 0) row_loss[row] = hit ? scale * (logf(den) - (zt - mx)) : 0.f;      // differences against the maximum only
        if (dlogits == nullptr && dx == nullptr) continue;
        // zr[k] becomes dlogits (zero behind the last class and on a row without a target)
#pragma unroll
        for (int k = 0; k < CK; ++k) {
            const int c = 64 * k + lane;
            const float p = expf(zr[k] - mx) * inv;
            zr[k] = (hit && c < C) ? scale * (p - (c == t ? 1.0f : 0.f)) : 0.f;
            if (dlogits != nullptr && c < C) dlogits[row * C + c] = zr[k];
        }
        if (dx == nullptr) continue;
        float* dxr = dx + row * lddx;
        const int nj = NQ > 0 ? NX : (D4 + 63) >> 6;
        if constexpr (NQ > 0) {
            f32x4 acc[NX];
#pragma unroll
            for (int q = 0; q < NX; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (hit) {
#pragma unroll
                for (int k = 0; k < CK; ++k) {
                    const int cend = C - 64 * k < 64 ? C - 64 * k : 64;
                    for (int cc = 0; cc < cend; ++cc) {
                        const float dl = __shfl(zr[k], cc);
#pragma unroll
                        for (int q = 0; q < NX; ++q) {
                            const int j = lane + 64 * q;
                            if (j < D4) acc[q] = fma_axpy4(dl, w_quad<VEC, WLDS>(w, sm, 64 * k + cc, j, D, D4), acc[q]);
                        }
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < NX; ++q) {
                const int j = lane + 64 * q;
                if (j < D4) store_quad<VEC>(dxr, j, D, acc[q]);
            }
        } else {
            for (int jq = 0; jq < nj; ++jq) {                 // every lane walks every step: the broadcasts need the whole wave
                const int j = lane + 64 * jq;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                if (hit) {
#pragma unroll
                    for (int k = 0; k < CK; ++k) {
                        const int cend = C - 64 * k < 64 ? C - 64 * k : 64;
                        for (int cc = 0; cc < cend; ++cc) {
                            const float dl = __shfl(zr[k], cc);
                            if (j < D4) acc = fma_axpy4(dl, w_quad<VEC, WLDS>(w, sm, 64 * k + cc, j, D, D4), acc);
                        }
                    }
                }
                if (j < D4) store_quad<VEC>(dxr, j, D, acc);
            }
        }
    }
}

constexpr int XENT_MAX_C = 1024;
constexpr size_t XENT_LDS_BYTES = 65536;       // what a workgroup may take without raising the kernel's dynamic-LDS limit

template <int NQ, int CK, bool VEC, bool WLDS>
void xent_launch(unsigned grid, size_t lds, hipStream_t s, const float* x, long ldx, const float* w, const float* b, const int* target,
                 float scale, float* row_loss, float* dlogits, float* dx, long lddx, int M, int D, int C) {
    hipLaunchKernelGGL((linear_xent_kernel<NQ, CK, VEC, WLDS>), dim3(grid), dim3(256), lds, s, x, ldx, w, b, target, scale, row_loss,
                       dlogits, dx, lddx, M, D, C);
}

template <int NQ, int CK>
void xent_route(bool vec, bool wlds, unsigned grid, size_t lds, hipStream_t s, const float* x, long ldx, const float* w, const float* b,
                const int* target, float scale, float* row_loss, float* dlogits, float* dx, long lddx, int M, int D, int C) {
    if (vec && wlds) xent_launch<NQ, CK, true, true>(grid, lds, s, x, ldx, w, b, target, scale, row_loss, dlogits, dx, lddx, M, D, C);
    else if (vec) xent_launch<NQ, CK, true, false>(grid, lds, s, x, ldx, w, b, target, scale, row_loss, dlogits, dx, lddx, M, D, C);
    else if (wlds) xent_launch<NQ, CK, false, true>(grid, lds, s, x, ldx, w, b, target, scale, row_loss, dlogits, dx, lddx, M, D, C);
    else xent_launch<NQ, CK, false, false>(grid, lds, s, x, ldx, w, b, target, scale, row_loss, dlogits, dx, lddx, M, D, C);
}

}  // namespace

extern "C" int lime_linear_xent_f32(const float* x, int64_t ldx, const float* w, const float* b, const int32_t* target, float scale,
                                    float* row_loss, float* dlogits, float* dx, int64_t lddx, int32_t M, int32_t D, int32_t C,
                                    void* stream) {
    LIME_REQUIRE(x && w && target && row_loss, LIME_ERR_BAD_ARG, "lime_linear_xent_f32: NULL pointer");
    LIME_REQUIRE(M >= 1 && D >= 1 && C >= 1, LIME_ERR_BAD_ARG, "lime_linear_xent_f32: M %d, D %d and C %d must be positive", M, D, C);
    LIME_REQUIRE(ldx >= D && (!dx || lddx >= D), LIME_ERR_BAD_ARG, "lime_linear_xent_f32: ldx %lld / lddx %lld below D %d",
                 (long long)ldx, (long long)lddx, D);
    LIME_REQUIRE(C <= XENT_MAX_C, LIME_ERR_UNSUPPORTED, "lime_linear_xent_f32: C %d > %d", C, XENT_MAX_C);
    const int D4 = (D + 3) / 4;
    const bool vec = D % 4 == 0 && lime_al16(x, ldx) && lime_al16(w, D) && lime_al16(dx, lddx);
    const size_t wbytes = (size_t)C * D4 * 16;
    const bool wlds = wbytes <= XENT_LDS_BYTES;
    const size_t lds = wlds ? wbytes : 0;
    const unsigned grid = lime_grid_cap(M, 4, 2 * lime_num_cus());
    hipStream_t s = (hipStream_t)stream;
#define LIME_XENT_ROUTE(NQ_, CK_) \
    xent_route<NQ_, CK_>(vec, wlds, grid, lds, s, x, (long)ldx, w, b, target, scale, row_loss, dlogits, dx, (long)lddx, M, D, C)
    if (C <= 64) {
        if (D4 <= 128) LIME_XENT_ROUTE(2, 1); else if (D4 <= 512) LIME_XENT_ROUTE(8, 1); else LIME_XENT_ROUTE(0, 1);
    } else {
        if (D4 <= 128) LIME_XENT_ROUTE(2, 16); else if (D4 <= 512) LIME_XENT_ROUTE(8, 16); else LIME_XENT_ROUTE(0, 16);
    }
#undef LIME_XENT_ROUTE
    return lime_check_launch("lime_linear_xent_f32");
}
