// lime_grad_clip_coef_f32 / lime_adam_f32 / lime_nll_softmax_f32: clip_grad_norm_ + Adam over flat buffers (reference trainer.py:33,
// 146-148) and the loss of trainer.py:71-73.  All sums in a fixed order.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// optimizer: sum of squares -> clip coefficient -> Adam   (trainer.py:33, 146-148)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) s += g[e] * g[e];
    s = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[0] = total norm, out[1] = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_); max_norm <= 0: 1
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ partial, int n, float max_norm,
                                                         float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int e = threadIdx.x; e < n; e += 256) s += partial[e];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(s);
        out[0] = norm;
        out[1] = max_norm > 0.f ? fminf(1.0f, max_norm / (norm + 1e-6f)) : 1.0f;
    }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, long n, float lr, float beta1, float beta2, float eps,
                                                    float weight_decay, float bias1, float bias2_sqrt,
                                                    const float* __restrict__ grad_scale) {
    const float gs = grad_scale ? *grad_scale : 1.0f;
    const float step = lr / bias1;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
        float gr = g[e] * gs;
        const float pe = p[e];
        if (weight_decay != 0.f) gr += weight_decay * pe;
        const float me = beta1 * m[e] + (1.0f - beta1) * gr;
        const float ve = beta2 * v[e] + (1.0f - beta2) * gr * gr;
        m[e] = me;
        v[e] = ve;
        p[e] = pe - step * (me / (sqrtf(ve) / bias2_sqrt + eps));
    }
}

// loss = mean_b (-log_softmax(logits[b])[0]);  dlogits = (softmax - onehot_0) / B      (trainer.py:71-73)
__global__ __launch_bounds__(256) void nll_softmax_kernel(const float* __restrict__ logits, long ld, int B, int K,
                                                           float* __restrict__ loss, float* __restrict__ dlogits, long ldd) {
    __shared__ float red[4];
    float part = 0.f;
    const float inv_b = 1.0f / (float)B;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float* x = logits + (long)b * ld;
        float mx = x[0];
        for (int j = 1; j < K; ++j) mx = fmaxf(mx, x[j]);
        float s = 0.f;
        for (int j = 0; j < K; ++j) s += expf(x[j] - mx);
        // every difference is taken against the row's maximum: x[j] - (mx + logf(s)) rounds at the size of the logits (4e-6 at 100),
        // which 1 - softmax[0] of a confident row does not survive (logits of 100 occur: the dot product of unnormalised vectors)
        part += logf(s) - (x[0] - mx);
        const float inv_s = 1.0f / s;
        if (dlogits)
            for (int j = 0; j < K; ++j) dlogits[(long)b * ldd + j] = (expf(x[j] - mx) * inv_s - (j == 0 ? 1.0f : 0.f)) * inv_b;
    }
    const float tot = block_sum(part, red);
    if (threadIdx.x == 0) *loss = tot * inv_b;
}

}  // namespace

extern "C" int lime_grad_clip_coef_f32(const float* g, int64_t n, float max_norm, float* out2, float* workspace,
                                       int64_t workspace_floats, void* stream) {
    LIME_REQUIRE(g && out2 && workspace, LIME_ERR_BAD_ARG, "lime_grad_clip_coef_f32: null pointer");
    LIME_REQUIRE(n > 0 && workspace_floats >= 1024, LIME_ERR_BAD_ARG, "lime_grad_clip_coef_f32: n <= 0 or workspace < 1024 floats");
    hipStream_t s = (hipStream_t)stream;
    const int grid = (int)lime_grid_cap(n, 256, 1024);
    sumsq_kernel<<<grid, 256, 0, s>>>(g, n, workspace);
    int st = lime_check_launch("sumsq_kernel");
    if (st != LIME_OK) return st;
    clip_coef_kernel<<<1, 256, 0, s>>>(workspace, grid, max_norm, out2);
    return lime_check_launch("clip_coef_kernel");
}

extern "C" int lime_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int32_t step, const float* grad_scale, void* stream) {
    LIME_REQUIRE(p && g && m && v, LIME_ERR_BAD_ARG, "lime_adam_f32: null pointer");
    LIME_REQUIRE(n >= 0 && step >= 1, LIME_ERR_BAD_ARG, "lime_adam_f32: n < 0 or step < 1");
    if (n == 0) return LIME_OK;
    const double b1 = 1.0 - pow((double)beta1, (double)step), b2 = sqrt(1.0 - pow((double)beta2, (double)step));
    adam_kernel<<<lime_grid_cap(n, 256, 4096), 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, (float)b1, (float)b2, grad_scale);
    return lime_check_launch("adam_kernel");
}

extern "C" int lime_nll_softmax_f32(const float* logits, int64_t ld, int32_t B, int32_t K, float* loss, float* dlogits, int64_t ldd,
                                    void* stream) {
    LIME_REQUIRE(logits && loss, LIME_ERR_BAD_ARG, "lime_nll_softmax_f32: null pointer");
    LIME_REQUIRE(B > 0 && K > 0 && ld >= K && (!dlogits || ldd >= K), LIME_ERR_BAD_ARG, "lime_nll_softmax_f32: bad dimensions");
    nll_softmax_kernel<<<1, 256, 0, (hipStream_t)stream>>>(logits, ld, B, K, loss, dlogits, ldd);
    return lime_check_launch("nll_softmax_kernel");
}
