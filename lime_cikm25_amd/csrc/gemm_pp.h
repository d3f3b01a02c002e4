// Internal interface between lime_linear_f32's routing (gemm_f32.hip) and the big-M / mid-M kernels behind it (gemm_pp_f32.hip,
// gemm_sp_f32.hip, gemm_mid_f32.hip): each unit's pure chooser and the launch of what it chose, the predicates the choosers share,
// the kernels' parameter block, and the split-product entry points other units dispatch to.
#pragma once
#include "common.h"
#include "dropout.h"

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

// ---- lime_linear_f32's routing ------------------------------------------------------------------------------------------------
// A chooser is a pure function of the argument block (pointers are looked at for NULL-ness and alignment only), the split mode and
// the CU count: false = this family does not take the call, true = *c holds the template arguments of the instantiation that does.
// lime_*_name prints them as rocprofv3 prints the kernel (plan and launch<> both call it; the string lives until the thread's next
// call); lime_*_launch runs that instantiation, or returns LIME_ERR_UNSUPPORTED with a message when the unit does not build it.  The order of preference between the families:
// linear_route() in gemm_f32.hip.

// What the LDS-DMA kernels ask of their operands, written once.  All of them decline only, so their order does not matter.
// 16-byte loads / stores of every row (the mid-M kernel: of a, w, c and res; it takes no res_pe)
static inline bool lime_pp_al16(const lime_linear_args* a) {
    return a->K % 4 == 0 && a->N % 4 == 0 && lime_al16(a->a, a->lda) && lime_al16(a->w, a->ldw) && lime_al16(a->c, a->ldc) &&
           lime_al16(a->res, a->ldr) && lime_al16(a->res_pe, a->ldr_pe);
}
// residual class (the RES template argument): 0 none, 1 dense / periodic / broadcast fp32 rows, 2 rows gathered by res_ids,
// 3 no residual: res is the forward ReLU output that gates the result (LIME_ACT_RELU_GRAD)
static inline int lime_pp_res_class(const lime_linear_args* a) {
    return a->act == LIME_ACT_RELU_GRAD ? 3 : !a->res ? 0 : a->res_ids ? 2 : 1;
}
// 32-bit byte offsets: within one block of `bm` rows of a dense operand, within the whole of a gathered / periodic / scattered one
static inline bool lime_pp_offsets32(const lime_linear_args* a, long bm) {
    const long lim = 0x7FFFFFF0L;
    if (a->bias && (uintptr_t)a->bias % 4) return false;
    if (bm * a->lda * 4 >= lim || (long)a->N * a->ldw * 4 >= lim || bm * a->ldc * 4 >= lim || bm * a->ldr * 4 >= lim || (long)a->M * 4 >= lim) return false;
    if (a->c_ids && (long)a->M * a->ldc * 4 >= lim) return false;
    return !(lime_pp_res_class(a) == 1 && a->res_mod > 0 && (long)a->res_mod * a->ldr * 4 >= lim);
}
// c_ids: compacted in_proj only -- a periodic residual indexed by the scattered row, no LayerNorm, act none
static inline bool lime_pp_cids_form(const lime_linear_args* a) {
    return !a->c_ids || (a->res && !a->res_ids && a->res_mod > 0 && !a->ln_gamma && a->act == LIME_ACT_NONE);
}
// pool32: LayerNorm over a dense residual, whole 32-row blocks
static inline bool lime_pp_pool_form(const lime_linear_args* a) {
    return !a->pool32 || (a->ln_gamma && a->res && !a->res_ids && a->res_div <= 1 && a->M % 32 == 0);
}
// LayerNorm: one tile spans the row, and the ReLU instantiations carry no LayerNorm
static inline bool lime_pp_ln_form(const lime_linear_args* a) { return !a->ln_gamma || (a->N <= 320 && a->act != LIME_ACT_RELU); }

struct LimeSpChoice { int ct, res; bool ln, relu, pool, rstd, cid; };                 // gemm_sp_kernel<CT, LN, RELU, RES, POOL, RSTD, CID>
struct LimePpChoice { int ntl, res, trim; bool ln, relu, pool, rstd, cid; };          // gemm_pp_kernel<NTL, LN, RELU, RES, false, POOL, RSTD, CID, TRIM>
struct LimeMidChoice { int shape; long ntiles; };                                     // gemm_mid_kernel: tile shape 0 = 64 x 64, 1 = 32 x 64, 2 = 32 x 32
bool lime_sp_choose(const lime_linear_args* a, int mode, int n_cu, LimeSpChoice* c);  // gemm_sp_f32.hip (split product on the bf16 cores)
bool lime_pp_choose(const lime_linear_args* a, LimePpChoice* c);                      // gemm_pp_f32.hip (fp32 MFMA, LDS-DMA staging)
bool lime_mid_choose(const lime_linear_args* a, int n_cu, LimeMidChoice* c);          // gemm_mid_f32.hip (64-row tiles and smaller)
const char* lime_sp_name(const LimeSpChoice& c);
const char* lime_pp_name(const LimePpChoice& c, bool bf);
static inline const char* lime_mid_name() { return "gemm_mid_kernel"; }
static inline const char* lime_tf(bool v) { return v ? "true" : "false"; }
int lime_sp_launch(const LimeSpChoice& c, const lime_linear_args* a, hipStream_t stream);
int lime_pp_launch(const LimePpChoice& c, const lime_linear_args* a, hipStream_t stream);
int lime_mid_launch(const LimeMidChoice& c, const lime_linear_args* a, hipStream_t stream);

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
