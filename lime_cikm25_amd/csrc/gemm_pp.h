// Internal interface between lime_linear_f32's dispatcher (gemm_f32.hip) and the big-M / mid-M kernels behind it (gemm_pp_f32.hip,
// gemm_sp_f32.hip, gemm_mid_f32.hip), their shared parameter block, and the split-product entry points other units dispatch to.
#pragma once
#include "common.h"
#include "dropout.h"

#define LIME_PP_NOT_APPLICABLE 1

struct PPParams {
    const float* a; long lda; const int* a_ids;
    const float* w; long ldw; const float* bias;
    const float* res; long ldr; int res_mod; const int* res_ids; const float* res_pe; long ldr_pe; int res_period;
    const float* ln_g; const float* ln_b; float ln_eps; float* ln_rstd;
    float* c; long ldc; int M, N, K;
    int ln_count;        // LayerNorm divides by this many columns (N unless the caller zero-padded N)
    int n_row_blocks, n_col_blocks;
    const int* m_dev;    // optional device-side row count: the kernel runs min(*m_dev, M) rows (M is the capacity)
    const int* c_ids;    // optional (CID instantiations): output row of A row r is c_ids[r]; a periodic residual is indexed by it
    int act = 0;         // gemm_sp_kernel only, instantiations without the ReLU template flag: LIME_ACT_TANH / LIME_ACT_SIGMOID at run time
    int res_div = 1;     // gemm_sp_kernel only (RES == 1 without res_mod): residual row = r / res_div (one row broadcast to res_div rows)
    float act_scale = 1.f;   // gemm_sp_kernel, RES == 3 (LIME_ACT_RELU_GRAD): v = res > 0 ? v * act_scale : 0
    LimeDropout drop = {0, 0, 1.f};   // gemm_sp_kernel, ReLU instantiations without residual: thresh != 0 -> the dropout mask behind the ReLU
#ifdef LIME_STAMPS
    unsigned long long* stamps;
#endif
};

// The fields of PPParams that every dispatcher takes from its argument block unchanged (lime_linear_args, or lime_linear_bf16_args with
// its bf16 operands behind float pointers).  Left to the caller: ln_rstd, ln_count where it is not N, act / res_div / act_scale / drop;
// to launch(): the block counts.
template <class Args>
static inline PPParams lime_pp_params(const Args* a) {
    PPParams p;
    p.a = (const float*)a->a; p.lda = a->lda; p.a_ids = a->a_ids;
    p.w = (const float*)a->w; p.ldw = a->ldw; p.bias = a->bias;
    p.res = (const float*)a->res; p.ldr = a->ldr; p.res_mod = a->res_mod; p.res_ids = a->res_ids;
    p.res_pe = a->res_pe; p.ldr_pe = a->ldr_pe; p.res_period = a->res_period > 0 ? a->res_period : 1;
    p.ln_g = a->ln_gamma; p.ln_b = a->ln_beta; p.ln_eps = a->ln_eps; p.ln_rstd = nullptr;
    p.c = (float*)a->c; p.ldc = a->ldc; p.M = a->M; p.N = a->N; p.K = a->K; p.ln_count = a->N;
    p.n_row_blocks = p.n_col_blocks = 0;
    p.m_dev = a->m_dev; p.c_ids = a->c_ids;
    return p;
}

// The tile width that pads N least: true = 320 columns, false = 256.  The dispatchers differ on a tie (N = 1280 k): the split-product
// kernel takes the wide tile (tie_wide), the fp32-MFMA kernels the narrow one.
static inline bool lime_pp_wide(int N, bool tie_wide) {
    const int pad5 = (N + 319) / 320 * 320 - N, pad4 = (N + 255) / 256 * 256 - N;
    return tie_wide ? pad5 <= pad4 : pad5 < pad4;
}

int lime_linear_pp(const lime_linear_args* a, hipStream_t stream);
int lime_linear_sp(const lime_linear_args* a, hipStream_t stream);       // gemm_sp_f32.hip (split product on the bf16 cores), same convention
int lime_linear_mid(const lime_linear_args* a, hipStream_t stream);      // gemm_mid_f32.hip, same return convention

// wgrad_sp_f32.hip: the weight gradient on the split product (lime_linear_wgrad_f32's big-M path, wgrad_f32.hip dispatches)
struct LimeWgradSpPlan { bool swap; int n_tiles, k_tiles, splits, rows_per_split; long np, kp; double fill; };
LimeWgradSpPlan lime_wgrad_sp_plan(int M, int N, int K);
int lime_wgrad_sp_launch(const LimeWgradSpPlan& w, const float* dy, long ldy, const float* x, long ldx, float* ws, int M, int N, int K,
                         int ones_col, hipStream_t s);
int lime_wgrad_sp_reduce_t(const LimeWgradSpPlan& w, const float* ws, float* dw, long lddw, int N, int K, int accumulate, hipStream_t s);
// wgrad_f32.hip: out[r, c] (+)= sum over the splits of ws[split * split_stride + r * ldw + c], in a fixed order; extra (optional):
// column `cols` of the partial grid into extra[r] in the same launch.  Hidden: between units of the library only, not in its dynamic
// symbol table.
__attribute__((visibility("hidden")))
int lime_reduce_partials(const float* ws, long split_stride, int splits, long ldw, float* out, long ldo, int rows, int cols,
                         int accumulate, hipStream_t s, float* extra = nullptr);
int lime_split_mode();                                                   // gemm_sp_f32.hip: the lime_set_split_gemm() setting
// token_attn_sp_f32.hip: unmasked S = 32 / 64 / 128 attention on the split product (LIME_PP_NOT_APPLICABLE: not taken)
int lime_token_attention_sp(const float* q, const float* k, const float* v, long ld, const int* row_map, const int* n_seq_dev,
                            float* out, long ldo, int n_seq, int S, int n_head, int hd, float scale, float* lse, hipStream_t s,
                            const LimeDropout* drop = nullptr);
// token_attn_bwd_sp_f32.hip: the one-pass attention backward (64 < S <= 128, no key mask) with all its products on the split product
int lime_token_attention_bwd_sp(const float* q, const float* k, const float* v, long ld, const float* dout, long ldo, float* dq, float* dk,
                                float* dv, long ldd, int n_seq, int S, int n_head, int head_dim, int head_stride, float scale,
                                const LimeDropout& drop, hipStream_t s);
