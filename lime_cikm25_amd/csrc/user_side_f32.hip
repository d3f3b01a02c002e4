// The user side of the scoring path, one fused kernel per stage: the candidate-aware attention weights over the history (three
// forward forms of one row loop, layers.py:66-81), the GraphSAGE mean, the gated residual + LayerNorm (alone, and fused with that
// mean), the history-vs-candidate interest match with the remaining-lifetime weight, and the plain lifetime-weighted dot product.
// All reductions are fixed-order (wave64 shuffles, then LDS across the waves): results are bitwise reproducible run to run.
// Their backward, and the training-mode candidate attention: tail_backward_f32.hip.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// candidate-aware attention weights
// ---------------------------------------------------------------------------------------------------
// One query row of one head against the H <= 512 keys of that head, by one wave: `q` is the row and `Kh` the key tile in LDS (pitch
// hdp = hd + 1, odd: conflict-free column walks), `mrow` the history's mask row.  Key c * 64 + lane is the lane's term c; the row
// maximum and sum go by wave shuffles.  sc[c] comes back as exp(score - row maximum) of every term with a key and the function
// returns 1 / their sum: the softmaxed weight is sc[c] * that, a product the accumulating callers fuse into their add (fp
// contraction; scaled in here, it would round on its own and change their bits).  The terms behind (c + 1) * 64 >= H are not
// touched (a skipped term would add -inf to the maximum and 0 to the sum: the same bits either way).
__device__ __forceinline__ float cand_attn_row(const float* q, const float* Kh, const unsigned char* __restrict__ mrow, int H, int hd,
                                              int hdp, float inv_scale, int lane, float (&sc)[8]) {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int h = c * 64 + lane;
        float v = -INFINITY;
        if (h < H) {
            float dot = 0.f;
            for (int j = 0; j < hd; ++j) dot += q[j] * Kh[h * hdp + j];
            v = dot * inv_scale;
            if (mrow[h] == 0) v = -1e9f;                             // layers.py:72
        }
        sc[c] = v;
        mx = fmaxf(mx, v);
        if ((c + 1) * 64 >= H) break;
    }
    mx = wave_max(mx);
    float den = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        sc[c] = (c * 64 + lane < H) ? expf(sc[c] - mx) : 0.f;
        den += sc[c];
        if ((c + 1) * 64 >= H) break;
    }
    return 1.0f / wave_sum(den);
}

// The tail of the two one-launch forms, by the whole workgroup behind a barrier: asum [N][H] (the sum over the heads of the softmaxed
// weights) and qn2 [N] (the squared query norms) -> agg [H] of this row.  qw (N floats) and v (H floats) are LDS the caller no longer
// needs.
__device__ __forceinline__ void cand_attn_tail(const float* asum, const float* qn2, float* qw, float* v, float* red,
                                               float* __restrict__ agg, int N, int H) {
    // query weights: softmax over the candidates of ||Q_n||_2 (layers.py:79); N <= 128
    float mx = -INFINITY;
    for (int n = 0; n < N; ++n) mx = fmaxf(mx, sqrtf(qn2[n]));
    float den = 0.f;
    for (int n = 0; n < N; ++n) den += expf(sqrtf(qn2[n]) - mx);
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += 256) qw[n] = expf(sqrtf(qn2[n]) - mx) / den;
    __syncthreads();
    // agg = softmax_H(sum_n qw_n * asum[n][h])  (layers.py:80-81)
    for (int h = threadIdx.x; h < H; h += 256) {
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc += asum[n * H + h] * qw[n];
        v[h] = acc;
    }
    const float inv = block_softmax_terms(v, H, red);
    for (int h = threadIdx.x; h < H; h += 256) agg[h] = v[h] * inv;
}

// one workgroup per impression row, heads one after the other: the only form for large N * H
__global__ __launch_bounds__(256) void cand_attn_weights_serial_kernel(const float* __restrict__ qp, const float* __restrict__ kp,
                                                                 const unsigned char* __restrict__ mask, float* __restrict__ agg,
                                                                 int N, int H, int D, int n_head) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hd = D / n_head;
    const int hdp = hd + 1;                        // odd pitch: conflict-free column walks
    float* Qh = sm;                                // [N][hdp]   this head's query tile
    float* Kh = Qh + N * hdp;                      // [H][hdp]   this head's key tile
    float* asum = Kh + H * hdp;                    // [N][H]     sum over heads of the softmaxed weights
    float* qn2 = asum + N * H;                     // [N]        squared norm of the full query
    float* red = qn2 + N;                          // [4]
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_scale = 1.0f / sqrtf((float)D);
    for (int e = threadIdx.x; e < N * H; e += 256) asum[e] = 0.f;
    for (int e = threadIdx.x; e < N; e += 256) qn2[e] = 0.f;
    for (int head = 0; head < n_head; ++head) {
        __syncthreads();
        // per-head K / Q tiles, coalesced along the head dim
        for (int e = threadIdx.x; e < N * hd; e += 256) {
            const int n = e / hd, j = e - n * hd;
            Qh[n * hdp + j] = qp[((long)b * N + n) * D + head * hd + j];
        }
        for (int e = threadIdx.x; e < H * hd; e += 256) {
            const int h = e / hd, j = e - h * hd;
            Kh[h * hdp + j] = kp[((long)b * H + h) * D + head * hd + j];
        }
        __syncthreads();
        if (threadIdx.x < N) {
            float q2 = 0.f;
            for (int j = 0; j < hd; ++j) q2 += Qh[threadIdx.x * hdp + j] * Qh[threadIdx.x * hdp + j];
            qn2[threadIdx.x] += q2;
        }
        // one wave per query row; keys across the 64 lanes; row max / sum by wave shuffles
        for (int n = wave; n < N; n += 4) {
            float sc[8];                                            // H <= 512 -> at most 8 keys per lane
            const float inv = cand_attn_row(Qh + n * hdp, Kh, mask + (long)b * H, H, hd, hdp, inv_scale, lane, sc);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int h = c * 64 + lane;
                if (h < H) asum[n * H + h] += sc[c] * inv;               // this wave owns row n: no race
            }
        }
    }
    __syncthreads();
    cand_attn_tail(asum, qn2, Qh, Kh, red, agg + (long)b * H, N, H);     // the Q and K tiles are free: qw, v
}

// Same result, heads spread over the four waves: wave w owns heads w, w + 4, ... with its own K / Q tiles and its own
// partial sums, so the head loop needs no workgroup barrier (the serial kernel spends most of its 80 us in them).
// Per (head, candidate) the softmax terms are identical; the sum over heads is taken wave 0..3 in a fixed order.
__global__ __launch_bounds__(256) void cand_attn_weights_kernel(const float* __restrict__ qp, const float* __restrict__ kp,
                                                                 const unsigned char* __restrict__ mask, float* __restrict__ agg,
                                                                 int N, int H, int D, int n_head) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hd = D / n_head;
    const int hdp = hd + 1;                        // odd pitch: conflict-free column walks
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per_wave = (N + H) * hdp + N * H + N;
    float* Qh = sm + wave * per_wave;              // [N][hdp]   this wave's query tile
    float* Kh = Qh + N * hdp;                      // [H][hdp]   this wave's key tile
    float* asum = Kh + H * hdp;                    // [N][H]     this wave's sum over its heads of the softmaxed weights
    float* qn2 = asum + N * H;                     // [N]        this wave's share of the squared query norm
    float* red = sm + 4 * per_wave;                // [4]
    const int b = blockIdx.x;
    const float inv_scale = 1.0f / sqrtf((float)D);
    for (int e = lane; e < N * H; e += 64) asum[e] = 0.f;
    for (int e = lane; e < N; e += 64) qn2[e] = 0.f;
    for (int head = wave; head < n_head; head += 4) {
        wave_lds_fence();
        for (int e = lane; e < N * hd; e += 64) {
            const int n = e / hd, j = e - n * hd;
            Qh[n * hdp + j] = qp[((long)b * N + n) * D + head * hd + j];
        }
        for (int e = lane; e < H * hd; e += 64) {
            const int h = e / hd, j = e - h * hd;
            Kh[h * hdp + j] = kp[((long)b * H + h) * D + head * hd + j];
        }
        wave_lds_fence();
        for (int n = lane; n < N; n += 64) {
            float q2 = 0.f;
            for (int j = 0; j < hd; ++j) q2 += Qh[n * hdp + j] * Qh[n * hdp + j];
            qn2[n] += q2;
        }
        for (int n = 0; n < N; ++n) {              // keys across the 64 lanes; row max / sum by wave shuffles
            float sc[8];                           // H <= 512 -> at most 8 keys per lane
            const float inv = cand_attn_row(Qh + n * hdp, Kh, mask + (long)b * H, H, hd, hdp, inv_scale, lane, sc);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int h = c * 64 + lane;
                if (h < H) asum[n * H + h] += sc[c] * inv;
            }
        }
    }
    __syncthreads();
    // fold the four waves' partials into wave 0's arrays (fixed order)
    float* asum0 = sm + (N + H) * hdp;
    float* qn20 = asum0 + N * H;
    for (int e = threadIdx.x; e < N * H; e += 256) {
        float t = asum0[e];
        for (int w = 1; w < 4; ++w) t += sm[w * per_wave + (N + H) * hdp + e];
        asum0[e] = t;
    }
    for (int e = threadIdx.x; e < N; e += 256) {
        float t = qn20[e];
        for (int w = 1; w < 4; ++w) t += sm[w * per_wave + (N + H) * hdp + N * H + e];
        qn20[e] = t;
    }
    __syncthreads();
    cand_attn_tail(asum0, qn20, sm, sm + N * hdp, red, agg + (long)b * H, N, H);      // wave 0's Q and K tiles are free: qw, v
}

}  // namespace

extern "C" int lime_cand_attn_weights_f32(const float* qp, const float* kp, const uint8_t* mask, float* agg, int32_t B,
                                          int32_t N, int32_t H, int32_t D, int32_t n_head, void* stream) {
    LIME_REQUIRE(qp && kp && mask && agg, LIME_ERR_BAD_ARG, "lime_cand_attn_weights_f32: NULL pointer");
    LIME_REQUIRE(B >= 0 && N > 0 && H > 0 && D > 0 && n_head > 0 && D % n_head == 0, LIME_ERR_BAD_ARG,
                 "lime_cand_attn_weights_f32: bad dims B=%d N=%d H=%d D=%d heads=%d", B, N, H, D, n_head);
    LIME_REQUIRE(N <= 128 && H <= 512, LIME_ERR_UNSUPPORTED, "lime_cand_attn_weights_f32: N <= 128 and H <= 512 only");
    if (B == 0) return LIME_OK;
    const int hdp = D / n_head + 1;
    const size_t per_wave = (size_t)((N + H) * hdp + N * H + N);
    const size_t lds_par = (4 * per_wave + 4) * sizeof(float);
    if (lds_par <= 64 * 1024) {                 // heads spread over the waves
        hipLaunchKernelGGL(cand_attn_weights_kernel, dim3((unsigned)B), dim3(256), lds_par, (hipStream_t)stream, qp, kp, mask, agg, N,
                           H, D, n_head);
        return lime_check_launch("lime_cand_attn_weights_f32");
    }
    const size_t lds = (per_wave + 4) * sizeof(float);
    LIME_REQUIRE(lds <= 160 * 1024, LIME_ERR_UNSUPPORTED, "lime_cand_attn_weights_f32: %zu B of LDS needed", lds);
    static int reserved = 64 * 1024;              // what a kernel may use without asking
    if (const int st = lime_reserve_lds((const void*)cand_attn_weights_serial_kernel, (int)lds, reserved, "lime_cand_attn_weights_f32")) return st;
    hipLaunchKernelGGL(cand_attn_weights_serial_kernel, dim3((unsigned)B), dim3(256), lds, (hipStream_t)stream, qp, kp, mask, agg, N, H,
                       D, n_head);
    return lime_check_launch("lime_cand_attn_weights_f32");
}

namespace {

// ---- the same weights with (row, head) parallelism: B = 32 rows put 32 workgroups on 256 CUs and the launch took 64 us ------------
// pass 1: one wave per (row b, head): that head's softmaxed weights P[b][head][n][h] and its share of ||Q_n||^2 -> workspace
// hist_div > 1: kp / mask hold ONE history for hist_div consecutive rows b (Model.score_impressions: the K candidates of an impression)
__global__ __launch_bounds__(64) void cand_attn_head_kernel(const float* __restrict__ qp, const float* __restrict__ kp,
                                                            const unsigned char* __restrict__ mask, float* __restrict__ ws,
                                                            int N, int H, int D, int n_head, int hist_div) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int hd = D / n_head, hdp = hd + 1;       // odd pitch: conflict-free column walks
    const int lane = threadIdx.x;
    const int b = blockIdx.x / n_head, head = blockIdx.x - b * n_head;
    const long bh = b / hist_div;                  // the history (keys, mask) of this row
    float* Qh = sm;                                // [N][hdp]
    float* Kh = sm + N * hdp;                      // [H][hdp]
    float* P = ws + ((long)blockIdx.x * N) * (H + 1);             // [N][H] probabilities, then [N] squared-norm shares behind them
    float* q2out = P + (long)N * H;
    // a row's head slice is hd contiguous floats: one coalesced load per row, eight rows in flight (a load -> LDS store chain per
    // row made the 55 rows 55 L2 round trips)
    for (int j = lane; j < hd; j += 64) {
        for (int r0 = 0; r0 < N + H; r0 += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = r0 + u;
                const float* src = r < N ? qp + ((long)b * N + r) * D + head * hd : kp + (bh * H + (r - N)) * D + head * hd;
                t[u] = r < N + H ? src[j] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (r0 + u < N + H) sm[(r0 + u) * hdp + j] = t[u];
        }
    }
    wave_lds_fence();
    for (int n = lane; n < N; n += 64) {
        float q2 = 0.f;
        for (int j = 0; j < hd; ++j) q2 += Qh[n * hdp + j] * Qh[n * hdp + j];
        q2out[n] = q2;
    }
    const float inv_scale = 1.0f / sqrtf((float)D);
    for (int n = 0; n < N; ++n) {                  // keys across the 64 lanes; row max / sum by wave shuffles
        float sc[8];                               // H <= 512 -> at most 8 keys per lane
        const float inv = cand_attn_row(Qh + n * hdp, Kh, mask + bh * H, H, hd, hdp, inv_scale, lane, sc);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int h = c * 64 + lane;
            if (h < H) P[(long)n * H + h] = sc[c] * inv;
            if ((c + 1) * 64 >= H) break;
        }
    }
}

// pass 2: one workgroup per row: sums over the heads in head order, query weights softmax_N(||Q_n||) (layers.py:79), agg (:80-81)
__global__ __launch_bounds__(256) void cand_attn_finish_kernel(const float* __restrict__ ws, float* __restrict__ agg, int N, int H, int n_head) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* qn = sm;                                // [N]  ||Q_n||
    float* v = sm + N;                             // [H]
    float* red = v + H;                            // [4]
    const int b = blockIdx.x;
    const float* base = ws + ((long)b * n_head * N) * (H + 1);
    const long hstride = (long)N * (H + 1);
    for (int n = threadIdx.x; n < N; n += 256) {
        float t = 0.f;
        for (int h0 = 0; h0 < n_head; h0 += 16) {
            float u[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) u[k] = h0 + k < n_head ? base[(h0 + k) * hstride + (long)N * H + n] : 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) t += u[k];               // head order
        }
        qn[n] = sqrtf(t);
    }
    __syncthreads();
    float qmx = -INFINITY, qden = 0.f;
    for (int n = 0; n < N; ++n) qmx = fmaxf(qmx, qn[n]);
    for (int n = 0; n < N; ++n) qden += expf(qn[n] - qmx);
    for (int h = threadIdx.x; h < H; h += 256) {
        float acc = 0.f;
        for (int n = 0; n < N; ++n) {
            float a = 0.f;
            for (int h0 = 0; h0 < n_head; h0 += 16) {              // a batch of heads in flight, added in head order
                float u[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) u[k] = h0 + k < n_head ? base[(h0 + k) * hstride + (long)n * H + h] : 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k) a += u[k];
            }
            acc += a * (expf(qn[n] - qmx) / qden);
        }
        v[h] = acc;
    }
    const float inv = block_softmax_terms(v, H, red);
    for (int h = threadIdx.x; h < H; h += 256) agg[(long)b * H + h] = v[h] * inv;
}

}  // namespace

extern "C" int64_t lime_cand_attn_weights_workspace(int32_t B, int32_t N, int32_t H, int32_t n_head) {
    return (int64_t)B * n_head * N * (H + 1);
}

extern "C" int lime_cand_attn_weights_shared_f32(const float* qp, const float* kp, const uint8_t* mask, float* agg, int32_t B, int32_t N,
                                                 int32_t H, int32_t D, int32_t n_head, int32_t hist_div, float* workspace,
                                                 int64_t workspace_floats, void* stream) {
    LIME_REQUIRE(hist_div >= 1, LIME_ERR_BAD_ARG, "lime_cand_attn_weights_shared_f32: hist_div < 1");
    LIME_REQUIRE(qp && kp && mask && agg && workspace, LIME_ERR_BAD_ARG, "lime_cand_attn_weights_ws_f32: NULL pointer");
    LIME_REQUIRE(B >= 0 && N > 0 && H > 0 && D > 0 && n_head > 0 && D % n_head == 0, LIME_ERR_BAD_ARG, "lime_cand_attn_weights_ws_f32: bad dims");
    LIME_REQUIRE(N <= 128 && H <= 512, LIME_ERR_UNSUPPORTED, "lime_cand_attn_weights_ws_f32: N <= 128, H <= 512 (N=%d H=%d)", N, H);
    LIME_REQUIRE(workspace_floats >= lime_cand_attn_weights_workspace(B, N, H, n_head), LIME_ERR_BAD_ARG, "lime_cand_attn_weights_ws_f32: workspace too small");
    LIME_REQUIRE((long)B * n_head < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_cand_attn_weights_ws_f32: too many (row, head) pairs");
    if (B == 0) return LIME_OK;
    const size_t lds1 = (size_t)(N + H) * (D / n_head + 1) * sizeof(float);
    LIME_REQUIRE(lds1 <= 64 * 1024, LIME_ERR_UNSUPPORTED, "lime_cand_attn_weights_ws_f32: %zu B of LDS needed", lds1);
    hipLaunchKernelGGL(cand_attn_head_kernel, dim3((unsigned)(B * n_head)), dim3(64), lds1, (hipStream_t)stream, qp, kp, mask, workspace, N, H, D, n_head, hist_div);
    hipLaunchKernelGGL(cand_attn_finish_kernel, dim3((unsigned)B), dim3(256), (size_t)(N + H + 4) * sizeof(float), (hipStream_t)stream,
                       (const float*)workspace, agg, N, H, n_head);
    return lime_check_launch("lime_cand_attn_weights_ws_f32");
}

extern "C" int lime_cand_attn_weights_ws_f32(const float* qp, const float* kp, const uint8_t* mask, float* agg, int32_t B, int32_t N, int32_t H,
                                             int32_t D, int32_t n_head, float* workspace, int64_t workspace_floats, void* stream) {
    return lime_cand_attn_weights_shared_f32(qp, kp, mask, agg, B, N, H, D, n_head, 1, workspace, workspace_floats, stream);
}

namespace {

// ---------------------------------------------------------------------------------------------------
// GraphSAGE mean over the first n_src node slots of cat[hist[b], user_nodes]
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sage_mean_kernel(const float* __restrict__ hist, const float* __restrict__ user_nodes,
                                                         float* __restrict__ out, int H, int n_src, int D) {
    const long b = blockIdx.x;
    const float inv = 1.0f / (float)n_src;
    for (int d = threadIdx.x; d < D; d += 256) {
        float acc = 0.f;
        int u = 0;
        for (; u + 8 <= n_src; u += 8) {             // eight node rows in flight, added in slot order
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (u + k < H) ? hist[(b * H + u + k) * D + d] : user_nodes[(long)(u + k - H) * D + d];
#pragma unroll
            for (int k = 0; k < 8; ++k) acc += v[k];
        }
        for (; u < n_src; ++u) acc += (u < H) ? hist[(b * H + u) * D + d] : user_nodes[(long)(u - H) * D + d];
        out[b * D + d] = acc * inv;
    }
}

}  // namespace

extern "C" int lime_sage_mean_f32(const float* hist, const float* user_nodes, float* out, int32_t B, int32_t H, int32_t n_user,
                                  int32_t n_src, int32_t D, void* stream) {
    LIME_REQUIRE(hist && user_nodes && out, LIME_ERR_BAD_ARG, "lime_sage_mean_f32: NULL pointer");
    LIME_REQUIRE(B >= 0 && H > 0 && n_user >= 0 && D > 0 && n_src > 0, LIME_ERR_BAD_ARG, "lime_sage_mean_f32: bad dims");
    LIME_REQUIRE(n_src <= H + n_user, LIME_ERR_BAD_ARG,
                 "lime_sage_mean_f32: n_src %d exceeds the %d node slots (the reference raises an index error here)", n_src,
                 H + n_user);
    if (B == 0) return LIME_OK;
    hipLaunchKernelGGL(sage_mean_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, hist, user_nodes, out, H, n_src, D);
    return lime_check_launch("lime_sage_mean_f32");
}

namespace {

// ---------------------------------------------------------------------------------------------------
// history-vs-candidate attention + dot-product interest match + remaining-lifetime weight:
// one workgroup per (impression row, candidate)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void interest_match_kernel(const float* __restrict__ kp, const float* __restrict__ qp,
                                                              const float* __restrict__ g, const float* __restrict__ cand,
                                                              const float* __restrict__ remaining, float* __restrict__ user_rep,
                                                              float* __restrict__ logits, int N, int H, int A, int D, float scale,
                                                              float alpha_s, float beta_s, int use_weight, int use_penalty) {
    // one workgroup per (impression row, candidate): B * N workgroups instead of B keep the chip busy
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Qs = sm;                     // [A]  this candidate's query
    float* al = Qs + A;                 // [H]  attention logits, then weights
    float* red = al + H;                // [4]
    const long bn = blockIdx.x;
    const long b = bn / N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = threadIdx.x; e < A; e += 256) Qs[e] = qp[bn * A + e];
    __syncthreads();
    // a[h] = kp[b,h,:] . q * scale: a wave streams one key row (coalesced), lanes over A, shuffle reduction
    // (four rows of a wave in flight: the loop is a chain of L2 round trips otherwise; the order of the additions is unchanged)
    for (int h0 = wave; h0 < H; h0 += 16) {
        float part[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = lane; j < A; j += 64) {
            const float q = Qs[j];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int h = h0 + 4 * u;
                part[u] += (h < H ? kp[(b * H + h) * A + j] : 0.f) * q;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float t = wave_sum(part[u]);
            if (lane == 0 && h0 + 4 * u < H) al[h0 + 4 * u] = t * scale;
        }
    }
    __syncthreads();
    // softmax over the history (unmasked, userEncoders.py:164)
    const float inv = block_softmax_terms(al, H, red);
    // u = sum_h alpha[h] g[b,h,:];  base = u . cand[b,n,:]
    float part = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        float u = 0.f;
        int h = 0;
        for (; h + 8 <= H; h += 8) {                 // eight rows in flight, added in the same order
            float gv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) gv[k] = g[(b * H + h + k) * D + d];
#pragma unroll
            for (int k = 0; k < 8; ++k) u += (al[h + k] * inv) * gv[k];
        }
        for (; h < H; ++h) u += (al[h] * inv) * g[(b * H + h) * D + d];
        if (user_rep) user_rep[bn * D + d] = u;
        part += u * cand[bn * D + d];
    }
    const float base = block_sum(part, red);
    if (threadIdx.x == 0 && logits) logits[bn] = use_weight ? base * lifetime_weight(remaining[bn], alpha_s, beta_s, use_penalty) : base;
}

}  // namespace

extern "C" int lime_interest_match_f32(const float* kp, const float* qp, const float* g, const float* cand,
                                       const float* remaining, float* user_rep, float* logits, int32_t B, int32_t N, int32_t H,
                                       int32_t A, int32_t D, float scale, float alpha_s, float beta_s, int32_t use_weight,
                                       int32_t use_penalty, void* stream) {
    LIME_REQUIRE(kp && qp && g && cand && (logits || user_rep), LIME_ERR_BAD_ARG, "lime_interest_match_f32: NULL pointer");
    LIME_REQUIRE(!(use_weight && logits) || remaining, LIME_ERR_BAD_ARG, "lime_interest_match_f32: remaining is NULL");
    LIME_REQUIRE(B >= 0 && N > 0 && H > 0 && A > 0 && D > 0, LIME_ERR_BAD_ARG, "lime_interest_match_f32: bad dims");
    if (B == 0) return LIME_OK;
    const size_t lds = (size_t)(A + H + 4) * sizeof(float);
    LIME_REQUIRE(lds <= 64 * 1024, LIME_ERR_UNSUPPORTED, "lime_interest_match_f32: %zu B of LDS needed", lds);
    hipLaunchKernelGGL(interest_match_kernel, dim3((unsigned)(B * N)), dim3(256), lds, (hipStream_t)stream, kp, qp, g, cand, remaining,
                       user_rep, logits, N, H, A, D, scale, alpha_s, beta_s, use_weight, use_penalty);
    return lime_check_launch("lime_interest_match_f32");
}

namespace {

__global__ __launch_bounds__(256) void lifetime_score_kernel(const float* __restrict__ user, const float* __restrict__ news,
                                                             const float* __restrict__ remaining, float* __restrict__ logits,
                                                             long rows, int D, float alpha_s, float beta_s, int use_weight,
                                                             int use_penalty) {
    // one wave per (row, candidate): lanes over the embedding dim, fixed-order shuffle reduction
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float part = 0.f;
    for (int d = lane; d < D; d += 64) part += user[r * D + d] * news[r * D + d];
    const float base = wave_sum(part);
    if (lane == 0) logits[r] = use_weight ? base * lifetime_weight(remaining[r], alpha_s, beta_s, use_penalty) : base;
}

}  // namespace

extern "C" int lime_lifetime_score_f32(const float* user, const float* news, const float* remaining, float* logits, int64_t rows,
                                       int32_t D, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty,
                                       void* stream) {
    LIME_REQUIRE(user && news && logits, LIME_ERR_BAD_ARG, "lime_lifetime_score_f32: NULL pointer");
    LIME_REQUIRE(!use_weight || remaining, LIME_ERR_BAD_ARG, "lime_lifetime_score_f32: remaining is NULL");
    LIME_REQUIRE(rows >= 0 && D > 0, LIME_ERR_BAD_ARG, "lime_lifetime_score_f32: bad dims");
    if (rows == 0) return LIME_OK;
    hipLaunchKernelGGL(lifetime_score_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, user, news,
                       remaining, logits, (long)rows, D, alpha_s, beta_s, use_weight, use_penalty);
    return lime_check_launch("lime_lifetime_score_f32");
}

namespace {

__global__ __launch_bounds__(256) void gate_ln_kernel(const float* __restrict__ y, const float* __restrict__ x,
                                                       const float* __restrict__ scale, const float* __restrict__ bias,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                       float* __restrict__ out, int D) {
    extern __shared__ __attribute__((aligned(16))) float sm[];      // [D] blended row, then 4 floats of scratch
    float* v = sm;
    float* red = sm + D;
    const long r = blockIdx.x;
    const float s = scale[r];
    float part = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        const float xv = x[r * D + d];
        const float g = lime_sigmoid(s * y[r * D + d] + bias[d]);
        const float wc = s * xv;
        const float val = g * wc + (1.f - g) * xv;
        v[d] = val;
        part += val;
    }
    const float mean = block_sum(part, red) / (float)D;
    part = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        const float dv = v[d] - mean;
        part += dv * dv;
    }
    const float rstd = 1.0f / sqrtf(block_sum(part, red) / (float)D + eps);
    for (int d = threadIdx.x; d < D; d += 256) out[r * D + d] = (v[d] - mean) * rstd * gamma[d] + beta[d];
}

}  // namespace

extern "C" int lime_gate_ln_f32(const float* y, const float* x, const float* scale, const float* bias, const float* gamma,
                                const float* beta, float eps, float* out, int64_t rows, int32_t D, void* stream) {
    LIME_REQUIRE(y && x && scale && bias && gamma && beta && out, LIME_ERR_BAD_ARG, "lime_gate_ln_f32: NULL pointer");
    LIME_REQUIRE(rows >= 0 && D > 0, LIME_ERR_BAD_ARG, "lime_gate_ln_f32: bad dims");
    LIME_REQUIRE(D <= 8192, LIME_ERR_UNSUPPORTED, "lime_gate_ln_f32: D %d > 8192", D);
    if (rows == 0) return LIME_OK;
    hipLaunchKernelGGL(gate_ln_kernel, dim3((unsigned)rows), dim3(256), (size_t)(D + 4) * sizeof(float), (hipStream_t)stream, y, x,
                       scale, bias, gamma, beta, eps, out, D);
    return lime_check_launch("lime_gate_ln_f32");
}

namespace {

// gate_ln over the H history rows of one user row + the GraphSAGE mean of the result, in one pass (userEncoders.py:121,151-157 behind
// layers.py:83-91): workgroup g = one (impression, candidate) row; its history rows are read from impression g / row_div (the
// scoring layout keeps ONE copy of a history for its row_div candidates), blended with this row's attention weights, normalised
// and written to out[g * H + h]; the column sums over the first n_hist node slots + `node_const` (the sum of the user-node rows the
// mean also covers: the same vector for every row) times inv_n are the SAGEConv aggregate mean_out[g].  A wave owns a row at a time
// (row statistics by wave shuffles); the four waves' column sums are added in wave order.  D <= 512.
template <int NW>
__global__ __launch_bounds__(NW * 64) void gate_ln_sage_kernel(const float* __restrict__ y, const float* __restrict__ x,
                                                            const float* __restrict__ scale, const float* __restrict__ bias,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                            float* __restrict__ out, const float* __restrict__ node_const,
                                                            float* __restrict__ mean_out, int H, int D, int row_div, int n_hist, float inv_n) {
    __shared__ float part[NW][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long g = blockIdx.x;
    const long src = (g / row_div) * H;
    const int nj = (D + 63) >> 6;                  // <= 8
    float bi[8], ga[8], be[8], csum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int d = lane + 64 * j;
        const bool ok = j < nj && d < D;
        bi[j] = ok ? bias[d] : 0.f;
        ga[j] = ok ? gamma[d] : 0.f;
        be[j] = ok ? beta[d] : 0.f;
        csum[j] = 0.f;
    }
    const float inv_d = 1.0f / (float)D;
    for (int h = wave; h < H; h += NW) {
        const float s = scale[g * H + h];
        const float* xr = x + (src + h) * D;
        const float* yr = y + (src + h) * D;
        float v[8];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = lane + 64 * j;
            v[j] = 0.f;
            if (j < nj && d < D) {
                const float xv = xr[d];
                const float gt = lime_sigmoid(s * yr[d] + bi[j]);
                v[j] = gt * (s * xv) + (1.f - gt) * xv;
                sum += v[j];
            }
        }
        const float mean = wave_sum(sum) / (float)D;        // (a quotient, as in gate_ln_kernel: exact on a constant row)
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = lane + 64 * j;
            if (j < nj && d < D) { const float dv = v[j] - mean; sq += dv * dv; }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(sq) * inv_d + eps);
        float* orow = out + (g * H + h) * D;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int d = lane + 64 * j;
            if (j < nj && d < D) {
                const float o = (v[j] - mean) * rstd * ga[j] + be[j];
                orow[d] = o;
                if (h < n_hist) csum[j] += o;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) part[wave][lane + 64 * j] = csum[j];
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += NW * 64) {
        float t = part[0][d];
#pragma unroll
        for (int w = 1; w < NW; ++w) t += part[w][d];          // wave order: fixed
        if (node_const) t += node_const[d];
        mean_out[g * D + d] = t * inv_n;
    }
}

}  // namespace

extern "C" int lime_gate_ln_sage_f32(const float* y, const float* x, const float* scale, const float* bias, const float* gamma,
                                     const float* beta, float eps, float* out, const float* node_const, float* mean_out, int64_t groups,
                                     int32_t H, int32_t D, int32_t row_div, int32_t n_src, void* stream) {
    LIME_REQUIRE(y && x && scale && bias && gamma && beta && out && mean_out, LIME_ERR_BAD_ARG, "lime_gate_ln_sage_f32: NULL pointer");
    LIME_REQUIRE(groups >= 0 && H > 0 && D > 0 && row_div >= 1 && n_src > 0, LIME_ERR_BAD_ARG, "lime_gate_ln_sage_f32: bad dims");
    LIME_REQUIRE(D <= 512, LIME_ERR_UNSUPPORTED, "lime_gate_ln_sage_f32: D %d > 512 (use lime_gate_ln_f32 + lime_sage_mean_f32)", D);
    LIME_REQUIRE(n_src <= H || node_const, LIME_ERR_BAD_ARG, "lime_gate_ln_sage_f32: n_src %d > H %d needs node_const", n_src, H);
    LIME_REQUIRE(groups < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_gate_ln_sage_f32: too many rows");
    if (groups == 0) return LIME_OK;
    // few rows (a training-shape batch: 32 .. 256 user rows): sixteen waves share a row's H history rows, the launch is a latency chain
    // otherwise; many rows (the scoring layout): four waves per workgroup, more workgroups per CU.  (The wave count changes the order
    // in which a column's H values are added: the two forms differ by fp32 rounding, each is deterministic.)
    if (groups < 4096)
        hipLaunchKernelGGL(gate_ln_sage_kernel<16>, dim3((unsigned)groups), dim3(1024), 0, (hipStream_t)stream, y, x, scale, bias, gamma, beta, eps,
                           out, n_src > H ? node_const : nullptr, mean_out, H, D, row_div, n_src < H ? n_src : H, 1.0f / (float)n_src);
    else
        hipLaunchKernelGGL(gate_ln_sage_kernel<4>, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, y, x, scale, bias, gamma, beta, eps,
                           out, n_src > H ? node_const : nullptr, mean_out, H, D, row_div, n_src < H ? n_src : H, 1.0f / (float)n_src);
    return lime_check_launch("lime_gate_ln_sage_f32");
}
