// The tail of the pooled user encoders (userEncoders ATT / MHSA) in one launch: additive attention pool over the history
// (layers.py:288-299 behind the affine1 + tanh GEMM), dot product with every candidate and the remaining-lifetime weight
// (util.py:23-49):
//     a[h]   = hidden[b, h, :] . w2              (-1e9 where mask[b, h] == 0)
//     alpha  = softmax_h(a)
//     u      = sum_h alpha[h] x[b, h, :]         -> user_rep[b, :]
//     logits[b, n] = (u . cand[b, n, :]) * w(remaining[b, n])
// The kernel is bandwidth bound: it reads hidden and x once, 4 H (A + D) bytes a row, against 2 H (A + D) + 2 N D flops.
//
// Two forms of ONE body (template parameter W = waves that share a row):
//   * W = 4, a workgroup per row: the four waves take the history rows of the score pass, the column groups of the weighted sum
//     and the candidates of the match in turn.  Chosen while the rows alone do not fill the chip (B < 2048: training batches).
//   * W = 1, a wave per row, four rows per workgroup: chosen from B = 2048 rows on (the eval layout: N = 1 and B in the
//     thousands), where a workgroup per row would spend its time on launch and barrier latency with most of its threads idle
//     behind the D / 4 = 100 column groups of the weighted sum.
// Every sum has the same operands in the same order in both forms -- a score is one wave's lanes over A then the wave shuffle
// tree, the softmax denominator is one wave's lanes over H, a column of u is a serial sum over h, a logit is one wave's lanes
// over D -- and every multiply-add is an explicit fmaf, so a row's bits depend neither on the form nor on B, N or the run.
// 16-byte loads on x, cand and the LDS copy of u always (D % 4 == 0, aligned rows are required); on hidden / w2 when their
// alignment allows (VEC), with the same lane-to-element assignment otherwise.
#include "common.h"

namespace {

template <int W, bool VEC>
__global__ __launch_bounds__(256) void pool_match_kernel(const float* __restrict__ hidden, long ldh, const float* __restrict__ w2,
                                                          const float* __restrict__ x, long ldx,
                                                          const unsigned char* __restrict__ mask, const float* __restrict__ cand,
                                                          const float* __restrict__ remaining, float alpha_s, float beta_s,
                                                          int use_weight, int use_penalty, float* __restrict__ user_rep,
                                                          float* __restrict__ logits, long B, int N, int H, int A, int D) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = (W == 4) ? wave : 0;                       // this wave's place among the W waves of its row
    const int Hp = (H + 3) & ~3;
    float* sc = sm + (long)((W == 4) ? 0 : wave) * (Hp + D);  // [Hp] scores, then weights
    float* us = sc + Hp;                                     // [D]  the pooled user vector
    long row = (W == 4) ? (long)blockIdx.x : (long)blockIdx.x * 4 + wave;
    const bool live = row < B;                               // a wave behind the last row redoes row B - 1 and stores nothing:
    if (!live) row = B - 1;                                  // the workgroup's barriers stay uniform
    const long r0 = row * H;

    // scores: a wave streams four history rows at a time, lanes over A
    const int A4 = (A + 3) >> 2;
    for (int h0 = w; h0 < H; h0 += 4 * W) {
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = lane; j < A4; j += 64) {
            const f32x4 wv = row_quad<VEC>(w2, j, A);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int h = h0 + u * W;
                if (h < H) part[u] = fma_dot4(row_quad<VEC>(hidden + (r0 + h) * ldh, j, A), wv, part[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int h = h0 + u * W;
            const float t = wave_sum(part[u]);
            if (lane == 0 && h < H) sc[h] = (mask != nullptr && mask[r0 + h] == 0) ? -1e9f : t;
        }
    }
    __syncthreads();
    // softmax over the history: every wave of the row computes the same maximum and denominator, wave 0 of it writes the weights
    float mx = -INFINITY;
    for (int h = lane; h < H; h += 64) mx = fmaxf(mx, sc[h]);
    mx = wave_max(mx);
    float den = 0.f;
    for (int h = lane; h < H; h += 64) den += expf(sc[h] - mx);
    const float inv = 1.0f / wave_sum(den);
    __syncthreads();
    if (w == 0)
        for (int h = lane; h < H; h += 64) sc[h] = expf(sc[h] - mx) * inv;
    __syncthreads();
    // u = sum_h alpha[h] x[b, h, :]: a thread owns four columns, eight rows in flight, added in history order
    const int D4 = D >> 2;
    const float* xr = x + r0 * ldx;
    for (int c = (W == 4) ? (int)threadIdx.x : lane; c < D4; c += W * 64) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        int h = 0;
        for (; h + 8 <= H; h += 8) {
            f32x4 xv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) xv[k] = *reinterpret_cast<const f32x4*>(xr + (long)(h + k) * ldx + 4 * c);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc = fma_axpy4(sc[h + k], xv[k], acc);
        }
        for (; h < H; ++h) acc = fma_axpy4(sc[h], *reinterpret_cast<const f32x4*>(xr + (long)h * ldx + 4 * c), acc);
        *reinterpret_cast<f32x4*>(us + 4 * c) = acc;
        if (user_rep != nullptr && live) *reinterpret_cast<f32x4*>(user_rep + row * D + 4 * c) = acc;
    }
    if (logits == nullptr) return;
    __syncthreads();
    // the match: a wave per candidate, lanes over D
    for (int n = w; n < N; n += W) {
        const float* cp = cand + (row * N + n) * D;
        float part = 0.f;
        for (int c = lane; c < D4; c += 64)
            part = fma_dot4(*reinterpret_cast<const f32x4*>(us + 4 * c), *reinterpret_cast<const f32x4*>(cp + 4 * c), part);
        const float base = wave_sum(part);
        if (lane == 0 && live)
            logits[row * N + n] = use_weight ? base * lifetime_weight(remaining[row * N + n], alpha_s, beta_s, use_penalty) : base;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int lime_pool_match_f32(const float* hidden, int64_t ldh, const float* w2, const float* x, int64_t ldx, const uint8_t* mask,
                                   const float* cand, const float* remaining, float alpha_s, float beta_s, int32_t use_weight,
                                   int32_t use_penalty, float* user_rep, float* logits, int32_t B, int32_t N, int32_t H, int32_t A,
                                   int32_t D, void* stream) {
    LIME_REQUIRE(hidden && w2 && x, LIME_ERR_BAD_ARG, "lime_pool_match_f32: NULL pointer");
    LIME_REQUIRE(user_rep || logits, LIME_ERR_BAD_ARG, "lime_pool_match_f32: both outputs are NULL");
    LIME_REQUIRE(!logits || cand, LIME_ERR_BAD_ARG, "lime_pool_match_f32: logits need cand");
    LIME_REQUIRE(!(use_weight && logits) || remaining, LIME_ERR_BAD_ARG, "lime_pool_match_f32: remaining is NULL");
    LIME_REQUIRE(B >= 0 && N > 0 && H > 0 && A > 0 && D > 0, LIME_ERR_BAD_ARG, "lime_pool_match_f32: bad dims");
    LIME_REQUIRE(D % 4 == 0 && ldx % 4 == 0 && ldx >= D && ldh >= A, LIME_ERR_BAD_ARG,
                 "lime_pool_match_f32: D %d and ldx %lld must be multiples of 4, ldx >= D, ldh >= A", D, (long long)ldx);
    LIME_REQUIRE(aligned16(x) && (!logits || aligned16(cand)) && aligned16(user_rep), LIME_ERR_BAD_ARG,
                 "lime_pool_match_f32: x, cand and user_rep must be 16-byte aligned");
    LIME_REQUIRE(H <= 512 && D <= 2048, LIME_ERR_UNSUPPORTED, "lime_pool_match_f32: H %d > 512 or D %d > 2048", H, D);
    if (B == 0) return LIME_OK;
    const bool vec = A % 4 == 0 && ldh % 4 == 0 && aligned16(hidden) && aligned16(w2);
    const size_t per_row = (size_t)(((H + 3) & ~3) + D) * sizeof(float);          // <= 10 KB
    const bool packed = B >= 2048;                                               // a wave per row, four rows per workgroup
    const dim3 grid((unsigned)(packed ? ((long)B + 3) / 4 : B));
    const size_t lds = packed ? 4 * per_row : per_row;
#define LIME_PM_LAUNCH(W_, V_)                                                                                                      \
    hipLaunchKernelGGL((pool_match_kernel<W_, V_>), grid, dim3(256), lds, (hipStream_t)stream, hidden, (long)ldh, w2, x, (long)ldx, \
                       mask, cand, remaining, alpha_s, beta_s, use_weight, use_penalty, user_rep, logits, (long)B, N, H, A, D)
    if (packed) {
        if (vec) LIME_PM_LAUNCH(1, true); else LIME_PM_LAUNCH(1, false);
    } else {
        if (vec) LIME_PM_LAUNCH(4, true); else LIME_PM_LAUNCH(4, false);
    }
#undef LIME_PM_LAUNCH
    return lime_check_launch("lime_pool_match_f32");
}
