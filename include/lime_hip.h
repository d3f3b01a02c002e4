/*
 * lime_hip.h -- C ABI of liblime_hip.so: hand-written gfx950 (MI355X) kernels for LIME's
 * candidate-scoring path.
 *
 * The reference (seongeunryu/lime-cikm25) has no FFI layer: its boundary is the Python nn.Module
 * surface.  Every entry point below replaces a PyTorch op sequence of the
 * reference and cites it (file:line into the reference repository).  The drop-in nn.Modules in
 * lime_cikm25_amd/ bind these through ctypes; INTEGRATION.md shows the stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (row-major, fp32 unless stated);
 *     the library never allocates, frees, copies to the host or synchronises;
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns at once;
 *   - return value: LIME_OK (0) or a negative lime_status; lime_last_error_string() describes the
 *     last failure of the calling thread;
 *   - calls are stateless and re-entrant; every entry point of the scoring path is bitwise reproducible run to run (no
 *     atomics in any reduction).  Two training-step kernels add with float atomics and are reproducible only up to the
 *     order of those fp32 additions: lime_embed_bwd_f32 (word rows repeat across tokens; lime_embed_bwd_sorted_f32 is the atomic-free
 *     replacement the training step uses) and the S > 128 path of
 *     lime_token_attention_bwd_f32 (dq from the key blocks).
 */
#ifndef LIME_HIP_H
#define LIME_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIME_ABI_VERSION 14

typedef enum {
    LIME_OK = 0,
    LIME_ERR_BAD_ARG = -1,      /* null pointer, non-positive dimension, misaligned leading dimension */
    LIME_ERR_UNSUPPORTED = -2,  /* shape outside what the kernels are built for */
    LIME_ERR_LAUNCH = -3,       /* hipGetLastError() after the launch was not hipSuccess */
    LIME_NOT_APPLICABLE = 1     /* nothing was launched and nothing is wrong: the entry does not cover this call (lime_token_attention_f32, vocab form) */
} lime_status;

int lime_abi_version(void);
const char* lime_last_error_string(void);
/* compute units of the current device as the library's launch geometry counts them (persistent grids: one workgroup per CU) */
int64_t lime_device_cus(void);

/* activation applied after bias (+ residual) */
enum { LIME_ACT_NONE = 0, LIME_ACT_RELU = 1, LIME_ACT_TANH = 2, LIME_ACT_SIGMOID = 3,
       LIME_ACT_RELU_GRAD = 4 /* backward of a ReLU: v = res(r, n) > 0 ? v * act_scale : 0, res = the forward activation (no residual add) */ };

/*
 * lime_linear_f32: C = epilogue(A . W^T + bias), exact-fp32 MFMA: v_mfma_f32_16x16x4_f32 in the LDS-DMA kernel that takes the
 * large 16-byte-aligned problems (gemm_pp_kernel: the four GEMMs of an encoder layer), v_mfma_f32_32x32x2_f32 in the general
 * kernel behind every other shape (gemm_f32_kernel).
 *
 * Replaces every nn.Linear on the path, with the surrounding element-wise work fused:
 *   in_proj / out_proj / linear1 / linear2 of the two TransformerEncoderLayers (newsEncoders.py:244-247,316,320),
 *   intent_layers (newsEncoders.py:284-295), Attention.affine1 (layers.py:288), FreshnessEncoder.dense
 *   (newsEncoders.py:82), LIME.project (newsEncoders.py:152-153), gate_proj (layers.py:87), SAGEConv lin_l / lin_r (userEncoders.py:153), K / Q (userEncoders.py:161-162),
 *   MultiHeadAttention W_Q/W_K/W_V (layers.py:224-226).
 *
 * A operand, row r (0 <= r < M), K columns:
 *   a_ids == NULL : a[r * lda + k]
 *   a_ids != NULL : a[a_ids[r] * lda + k] (+ a_pe[(r % a_period) * lda_pe + k] when a_pe != NULL)
 *                   -- the word-embedding gather and the positional table of newsEncoders.py:311-312,827
 *                      fused into the operand fetch; `a` is then the [V, K] table.
 * W is [N, K] row-major with leading dimension ldw (the nn.Linear weight as stored).
 * Epilogue, in this order, per output element (r, n):
 *   v  = acc + bias[n]                                   (bias may be NULL)
 *   v  = act(v)                                          (LIME_ACT_*)
 *   v += residual(r, n)                                  (res may be NULL)
 *        res_ids == NULL : res[(r / res_div) * ldr + n]   (res_div >= 1; > 1 broadcasts one row to res_div rows);
 *                          with res_mod > 0 the row is ((r / res_div) % res_mod): a [res_mod, N] table repeated down
 *                          the rows -- in_proj of the encoder layers uses it for the positional term, which is linear:
 *                          (E[ids] + PE) W^T + b = E[ids] W^T + (PE W^T + b)[r % S]
 *        res_ids != NULL : res[res_ids[r] * ldr + n] (+ res_pe[(r % res_period) * ldr_pe + n])
 *   ln_gamma != NULL : v = LayerNorm over the N columns of row r (eps = ln_eps); requires N <= 320 and either no
 *        activation (residual allowed) or ReLU without residual
 *   c[r * ldc + n] = v                                   (pool32 == 0)
 *   pool32 == 1: c[(r / 32) * ldc + n] = mean over the 32 rows of block r / 32 of v -- the token mean pooling of
 *        newsEncoders.py:317,321 taken in the epilogue (a 32-token title is finished; a longer sequence is the mean of its
 *        S / 32 block rows).  Needs M % 32 == 0, M >= 4096, the LayerNorm epilogue with a dense residual, 16-byte operands.
 * lda/ldw/ldr/ldc are in elements.
 */
typedef struct {
    const float* a;       int64_t lda;
    const int32_t* a_ids; const float* a_pe; int64_t lda_pe; int32_t a_period;
    const float* w;       int64_t ldw;
    const float* bias;
    const float* res;     int64_t ldr;   int32_t res_div;
    const int32_t* res_ids; const float* res_pe; int64_t ldr_pe; int32_t res_period;
    const float* ln_gamma; const float* ln_beta; float ln_eps;
    float* c;             int64_t ldc;
    int32_t M, N, K;
    int32_t act;
    int32_t res_mod;      /* > 0 (res_ids == NULL): residual row = (r / res_div) % res_mod -- a periodic table */
    int32_t pool32;       /* 1: (LayerNorm epilogue) c is [M / 32, N]: row r = mean of result rows 32 r .. 32 r + 31 */
    float* ln_rstd;       /* optional [M]: 1 / sqrt(var + eps) of every row's LayerNorm, kept for lime_layernorm_bwd_f32 */
    const int32_t* m_dev; /* optional DEVICE int: the launch computes min(*m_dev, M) rows -- M is then the capacity the buffers were
                             sized for.  Lets a launch captured in a HIP graph follow a per-batch row count (the live rows that
                             lime_compact_sequences counted) without a host round trip.  Needs 16-byte friendly operands (the LDS-DMA kernels). */
    const int32_t* c_ids; /* optional int32 [M]: the A rows are a compacted row list -- result row r is stored at c[c_ids[r] * ldc] and
                             the periodic residual is res[(c_ids[r] % res_mod) * ldr].  Needs res with res_mod > 0, no LayerNorm, act none
                             (the in_proj GEMM over the non-padding tokens of a batch). */
    float act_scale;      /* LIME_ACT_RELU_GRAD only: the factor on the passed gradient (1 / (1 - p) when the forward ReLU output went
                             through dropout in place: h > 0 <=> ReLU passed AND the mask kept); dH = dY W2 with the ReLU gradient of
                             linear1 applied in the epilogue (trainer.py:145 through newsEncoders.py:244-247).  res = h, dense rows. */
    float dropout_p;      /* > 0 (act none or ReLU, no residual / LayerNorm / pool32): v = keep(r * N + n) ? v / (1 - p) : 0 behind the activation,
                             the counter-based mask of (dropout_seed, dropout_site) as lime_dropout_f32 draws it over the [M, N] result --
                             nn.TransformerEncoderLayer's dropout behind linear1's ReLU in training mode (newsEncoders.py:244-247) */
    uint64_t dropout_seed;
    uint32_t dropout_site;
} lime_linear_args;

int lime_linear_f32(const lime_linear_args* args, void* stream);

/* n (1 .. 8) INDEPENDENT problems in one launch of the small / mid-M kernel (csrc/gemm_mid_f32.hip): the GEMMs around the token
 * encoders are latency bound -- a launch costs one tile's k loop, >= 10 us however small --, so two that do not depend on each other
 * (the two intent-attention affine1 layers, layers.py:288; gate_proj and Q, layers.py:87 / userEncoders.py:162; the positional tables
 * of the two encoders through in_proj) take one launch's time side by side.  Every problem must be one that kernel takes: 16-byte
 * friendly operands (K, N multiples of 4, aligned rows), K >= 16, no LayerNorm / pool32 / a_pe / c_ids / res_pe; m_dev is honoured.
 * Any M (it is meant for M < 4096); LIME_ERR_UNSUPPORTED names the first problem outside the kernel. */
int lime_linear_group_f32(const lime_linear_args* args, int32_t n, void* stream);

/* The kernel instantiation the calling thread's last lime_linear_f32 launched (e.g. "gemm_pp_kernel<10, true, false, 1>"),
 * as rocprofv3 names it: lets a profiler harness match its own event timings to the kernel trace. */
const char* lime_last_linear_kernel(void);

/* What lime_linear_f32 would run for an argument block, without running it: the routing decision (csrc/gemm_f32.hip, linear_route)
 * as data.  A pure function of the block, the lime_set_split_gemm() setting and the CU count: no launch, no pointer of the block is
 * read through (only NULL-ness and alignment count), and with n_cu > 0 no call into the HIP runtime; n_cu <= 0 asks the current device.
 * Returns what lime_linear_f32 would return for a block nothing takes (same status, same lime_last_error_string()), else LIME_OK and
 *   family       which unit's kernel: LIME_LINEAR_SP gemm_sp_kernel (split product), _PP gemm_pp_kernel (fp32 MFMA, LDS-DMA),
 *                _MID gemm_mid_kernel, _GENERAL gemm_f32_kernel; LIME_LINEAR_NONE for M == 0 (nothing is launched)
 *   second_pass  bits: passes over C behind the GEMM where the epilogue is not fused -- LIME_LINEAR_PASS_RELU_BWD lime_relu_bwd_f32
 *                (LIME_ACT_RELU_GRAD), LIME_LINEAR_PASS_DROPOUT lime_dropout_f32 (dropout_p); the GEMM then runs without them
 *   mid_shape    _MID: the tile shape 0 = 64 x 64, 1 = 32 x 64, 2 = 32 x 32, and `tiles` their number (= workgroups); else -1 / 0
 *   name         the instantiation as lime_last_linear_kernel() reports it after the launch (and as rocprofv3 prints it) */
enum { LIME_LINEAR_NONE = 0, LIME_LINEAR_SP = 1, LIME_LINEAR_PP = 2, LIME_LINEAR_MID = 3, LIME_LINEAR_GENERAL = 4 };
enum { LIME_LINEAR_PASS_RELU_BWD = 1, LIME_LINEAR_PASS_DROPOUT = 2 };
typedef struct {
    int32_t family;
    int32_t second_pass;
    int32_t mid_shape;
    int32_t reserved;
    int64_t tiles;
    char name[96];
} lime_linear_plan;

int lime_linear_plan_f32(const lime_linear_args* args, int32_t n_cu, lime_linear_plan* out);

/* Which kernels take the large 16-byte-aligned problems of lime_linear_f32 (M x N tiles >= 96 of 256 x 320) -- and, with the same bit 0, of
 * lime_linear_wgrad_f32 (M >= 4096), the unmasked padded-head lime_token_attention_f32 (S = 32 ... 512) and lime_token_attention_bwd_f32
 * (S > 64, no key mask):
 *   1 (default): csrc/gemm_sp_f32.hip -- fp32 operands split in registers into three bf16 terms each, six bf16 MFMAs per product
 *                block with fp32 accumulation: the error of one fp32 rounding per product (the same bound as the fp32 MFMA), fp32's
 *                exponent range, 2.7x the fp32 matrix rate;
 *   0          : csrc/gemm_pp_f32.hip -- v_mfma_f32_16x16x4_f32 (an fp32 fma chain).
 *   1 | 2      : as 1, and also the gathered-residual LayerNorm GEMM (out_proj), which is slower there and stays on the fp32 kernel by default;
 *   1 | 4      : as 1, without the rules that leave badly filling launches (few 256-row tiles) to the 128- / 64-row tile kernels (tests, A/B runs);
 *   4          : as 0, without the rule that hands big-M problems with few 128-row tiles to the 64-row-tile kernel (tests).
 * Process-wide; returns the previous setting; any other argument only queries.  LIME_SPLIT_GEMM=0 in the environment sets the start value. */
int lime_set_split_gemm(int on);

/*
 * lime_linear_bf16: the same operation on the bf16 matrix cores (BASELINE config 3: "bf16 MFMA with fp32
 * accumulate / softmax / LayerNorm").  A (or the gathered table), W and C are bf16 (uint16 storage, row-major);
 * accumulation, bias, activation, residual add and LayerNorm are fp32; the result is rounded to bf16 (nearest even).
 *   K % 8 == 0, K >= 64, lda % 8 == 0, ldw % 8 == 0 (16-byte rows); N % 4 == 0, ldc % 4 == 0.  K = 300 / N = 300 of the
 *   encoder layers are passed as 304 with zero columns / zero weight rows (lime_to_bf16 pads while converting).
 *   res_kind: 0 none; 1 fp32 rows res[(r or r % res_mod) * ldr + n]; 2 bf16 rows gathered by res_ids (+ fp32
 *   res_pe[(r % res_period)]); 3 bf16 rows res[r * ldr + n].  Kinds 2 and 3 are built with the LayerNorm epilogue only,
 *   kind 1 without it; act is none, or ReLU without residual.  ln_count: the number of real columns LayerNorm divides
 *   by (zero-padded columns must have zero weights, bias, residual, gamma and beta: they come out as zeros).
 *   Any M works; the kernel is built for M >= 4096 (two 128-row workgroups per CU).
 */
typedef struct {
    const uint16_t* a;    int64_t lda;
    const int32_t* a_ids;
    const uint16_t* w;    int64_t ldw;
    const float* bias;
    const void* res;      int64_t ldr;   int32_t res_kind; int32_t res_mod;
    const int32_t* res_ids; const float* res_pe; int64_t ldr_pe; int32_t res_period;
    const float* ln_gamma; const float* ln_beta; float ln_eps; int32_t ln_count;
    uint16_t* c;          int64_t ldc;      /* pool32: float* instead, [M / 32, N] (see lime_linear_args.pool32) */
    int32_t M, N, K;
    int32_t act;
    int32_t pool32;       /* 1: LayerNorm epilogue with a bf16 residual (res_kind 3) only; M % 32 == 0; fp32 block means */
    int32_t reserved;     /* must be 0 */
    const int32_t* m_dev; /* optional device int: min(*m_dev, M) rows are computed (see lime_linear_args.m_dev) */
    const int32_t* c_ids; /* optional int32 [M]: result row r goes to c[c_ids[r] * ldc], the fp32 periodic residual (res_kind 1 with
                             res_mod > 0) is indexed by c_ids[r] % res_mod; no LayerNorm, act none (see lime_linear_args.c_ids) */
} lime_linear_bf16_args;

int lime_linear_bf16(const lime_linear_bf16_args* args, void* stream);

/*
 * lime_encoder_ffn_bf16: the feed-forward half of an encoder layer in one launch on the bf16 matrix cores
 * (newsEncoders.py:244-247 as nn.TransformerEncoderLayer runs it, :316-321 with the token mean pooling):
 *     y = LayerNorm(x + W2 relu(W1 x + b1) + b2)          out = y (bf16 rows), or with pool32 the fp32 means of 32-row blocks
 * x: bf16 [M, ldx], the E real columns followed by zero columns up to lime_ffn_bf16_model_columns() (304; E = 300 is carried as
 * 304, as lime_linear_bf16 produces it).  w1p / w2p: the weights as lime_ffn_pack_bf16 lays them out.  The hidden state stays
 * in registers and the layer input is read once: against lime_linear_bf16 x 2 the launch moves 0.6 KB instead of 3.8 KB per token
 * through HBM.  Accumulation, residual and LayerNorm are fp32; b1 is applied in bf16 (it rides in the GEMM).
 * Built for 289 <= E < 304 and F % 128 == 0; anything else returns LIME_ERR_UNSUPPORTED (use lime_linear_bf16).
 * m_dev: optional device row count, as in lime_linear_args.
 */
typedef struct {
    const uint16_t* x;    int64_t ldx;
    const uint16_t* w1p;                    /* lime_ffn_pack_bf16's two outputs (opaque: the kernel's weight-ring slots, */
    const uint16_t* w2p;                    /* each one contiguous block in the order of its LDS image); 16-byte aligned   */
    const float* b2;                        /* fp32 [E] */
    const float* ln_gamma; const float* ln_beta; float ln_eps;     /* fp32 [E] */
    int32_t pool32;                         /* 1: out is float [M / 32, ldo] (M % 32 == 0); 0: out is bf16 [M, ldo] */
    void* out;            int64_t ldo;      /* >= 304 columns; the columns behind E come out as zeros */
    int32_t M, E, F;
    int32_t reserved;                       /* must be 0 */
    const int32_t* m_dev;
} lime_ffn_bf16_args;

int lime_encoder_ffn_bf16(const lime_ffn_bf16_args* args, void* stream);

/* w1 fp32 [F, E] (ld ldw1), b1 fp32 [F], w2 fp32 [E, F] (ld ldw2) -> w1p, w2p: bf16 buffers of lime_ffn_pack_bf16_size(F, 0) and
 * (F, 1) elements (F * 320 and F * 304). */
int64_t lime_ffn_pack_bf16_size(int32_t F, int32_t which);
int lime_ffn_pack_bf16(const float* w1, int64_t ldw1, const float* b1, const float* w2, int64_t ldw2, int32_t E, int32_t F,
                       uint16_t* w1p, uint16_t* w2p, void* stream);

/*
 * lime_encoder_ffn_sp: the fp32 feed-forward half of an encoder layer in one launch, split products on the bf16 matrix cores
 * (three bf16 terms per fp32 operand, six MFMAs per block: fp32-level products, as lime_linear_f32's split-product kernel):
 *     y = LayerNorm(x + W2 relu(W1 x + b1) + b2)          out = y (fp32 rows [M, ldo]), or with pool32 the means of 32-row blocks
 * x: fp32 [M, ldx], 16-byte aligned rows.  w1p / w2p: the weights as lime_ffn_pack_sp lays them out.  The hidden state stays in
 * registers.  Only the E real columns of out are written.  Built for E <= 304, E % 4 == 0 and F a multiple of 128 up to 4096;
 * anything else returns LIME_ERR_UNSUPPORTED (use lime_linear_f32 twice).  m_dev: optional device row count, as in lime_linear_args
 * (with pool32 a multiple of 32: a block is live or dead as a whole).  One 512-thread workgroup per CU (two waves per SIMD), 16 rows
 * per wave; a row's bits, and with pool32 a block's, do not depend on where in a launch it sits.
 */
typedef struct {
    const float* x;       int64_t ldx;
    const uint16_t* w1p;                    /* lime_ffn_pack_sp's two outputs (opaque: the kernel's weight-ring slots, three bf16 */
    const uint16_t* w2p;                    /* term images each, one contiguous block per slot); 16-byte aligned                  */
    const float* b1;                        /* fp32 [F] */
    const float* b2;                        /* fp32 [E] */
    const float* ln_gamma; const float* ln_beta; float ln_eps;     /* fp32 [E] */
    int32_t pool32;                         /* 1: out is [M / 32, ldo] (M % 32 == 0); 0: out is [M, ldo] */
    float* out;           int64_t ldo;
    int32_t M, E, F;
    int32_t reserved;                       /* must be 0 */
    const int32_t* m_dev;
} lime_ffn_sp_args;

int lime_encoder_ffn_sp(const lime_ffn_sp_args* args, void* stream);

/* w1 fp32 [F, E] (ld ldw1), w2 fp32 [E, F] (ld ldw2) -> w1p, w2p: bf16 buffers of lime_ffn_pack_sp_size(F, 0) and (F, 1) elements
 * (F * 960 and F * 912). */
int64_t lime_ffn_pack_sp_size(int32_t F, int32_t which);
int lime_ffn_pack_sp(const float* w1, int64_t ldw1, const float* w2, int64_t ldw2, int32_t E, int32_t F, uint16_t* w1p, uint16_t* w2p,
                     void* stream);

/*
 * lime_encoder_oproj_sp: out_proj + residual + norm1 of an fp32 encoder layer in one launch, split products on the bf16 matrix
 * cores (the arithmetic of lime_encoder_ffn_sp's linear2 half):
 *     x1 = LayerNorm(residual + attn Wo^T + bo)           out = x1 (fp32 rows [M, ldo]; only the E real columns are written)
 * attn: fp32 [M, lda], 16-byte aligned rows (the attention output).  wp: Wo as lime_oproj_pack_sp lays it out.  The residual of
 * row r is res[r] (res_ids NULL: res is [M, ldr]) or res[res_ids[r]] + res_pe[r % res_period] (res is the [V, ldr] word table,
 * ids unchecked in [0, V); res_pe NULL: no positional term).  Rows at or beyond the row count are neither read nor written.
 * Built for E <= 304 and E % 4 == 0; anything else returns LIME_ERR_UNSUPPORTED (use lime_linear_f32).  m_dev: optional device row
 * count, as in lime_linear_args.  One 512-thread workgroup per CU (two waves per SIMD), 16 rows per wave; a row's bits do not
 * depend on where in a launch it sits.
 */
typedef struct {
    const float* attn;    int64_t lda;
    const uint16_t* wp;                     /* lime_oproj_pack_sp's output (opaque: the kernel's weight-ring slots); 16-byte aligned */
    const float* bias;                      /* fp32 [E] */
    const float* res;     int64_t ldr;      /* 16-byte aligned rows */
    const int32_t* res_ids;                 /* int32 [M] or NULL */
    const float* res_pe;  int64_t ldr_pe;   /* [>= res_period, ldr_pe] or NULL (with res_ids only) */
    int32_t res_period;
    float ln_eps;
    const float* ln_gamma; const float* ln_beta;                   /* fp32 [E] */
    float* out;           int64_t ldo;
    int32_t M, E;
    const int32_t* m_dev;
} lime_oproj_sp_args;

int lime_encoder_oproj_sp(const lime_oproj_sp_args* args, void* stream);

/* w fp32 [E, E] (ld ldw) -> wp: a bf16 buffer of lime_oproj_pack_sp_size() elements (10 * 3 * 304 * 32). */
int64_t lime_oproj_pack_sp_size(void);
int lime_oproj_pack_sp(const float* w, int64_t ldw, int32_t E, uint16_t* wp, void* stream);

/*
 * lime_encoder_block_bf16: everything of an encoder layer behind the attention core in one launch
 * (nn.TransformerEncoderLayer as newsEncoders.py:244-247, 316-321 run it):
 *     x1 = LayerNorm1(res + add_rows + attn Wo^T)          y = LayerNorm2(x1 + W2 relu(W1 x1 + b1) + b2)
 * attn: bf16 [M, lda] (the E real columns + zero columns up to 304, as lime_token_attention_bf16 writes it with out_cols = 304).
 * res (bf16 rows of 304 columns): res_kind 2 = the word table [res_rows, ldr] gathered by res_ids[M] (layer 0), res_kind 3 = the layer
 * input [M, ldr].  add_rows: fp32 [add_period, ld_add], row r % add_period is added to token r -- out_proj's bias, with the positional
 * rows added to it where the residual is the bare word rows (add_period = S), or the bias alone (add_period = 1).
 * x1 is rounded to bf16 (it feeds the bf16 GEMM and is the second residual, exactly as when lime_linear_bf16 stores it) and never
 * leaves the CU: the attention tile, the residual rows and x1 share one stationary LDS image.  out / pool32 / m_dev as in
 * lime_encoder_ffn_bf16.  w0p: lime_oproj_pack_bf16's output; ln1_* fp32 [E], 16-byte aligned.
 */
typedef struct {
    const uint16_t* attn; int64_t lda;
    const uint16_t* w0p;
    const float* add_rows; int64_t ld_add; int32_t add_period;
    int32_t res_kind;
    const uint16_t* res;  int64_t ldr;  int64_t res_rows;
    const int32_t* res_ids;
    const float* ln1_gamma; const float* ln1_beta; float ln1_eps;
    int32_t pool32;
    const uint16_t* w1p;  const uint16_t* w2p;  const float* b2;
    const float* ln2_gamma; const float* ln2_beta; float ln2_eps;
    int32_t M, E, F;
    void* out;            int64_t ldo;
    const int32_t* m_dev;
} lime_encoder_block_bf16_args;

int lime_encoder_block_bf16(const lime_encoder_block_bf16_args* args, void* stream);

/* out_proj weight fp32 [E, E] (ld ldw) -> wp: bf16 buffer of lime_oproj_pack_bf16_size() elements (the kernel's ring slots) */
int64_t lime_oproj_pack_bf16_size(void);
int lime_oproj_pack_bf16(const float* w, int64_t ldw, int32_t E, uint16_t* wp, void* stream);

/*
 * lime_inproj_bf16: the q / k / v projection in front of lime_token_attention_bf16, activation-stationary (csrc/inproj_bf16.hip):
 *     out[c_ids[r] or r, n] = bf16( a[a_ids[r] or r, :] . w[n, :] + add_rows[(c_ids[r] or r) % add_period, n] ),   n < N
 * a: bf16 rows of K valid columns (the word table gathered by a_ids, or the layer input); wp: lime_inproj_pack_bf16's output for the
 * fp32 weight [N, K] with the heads already padded to 32 columns (lime_pad_heads_f32), N a multiple of 320, K <= 320, K % 8 == 0;
 * add_rows fp32 [add_period, >= N]: bias, or positional rows x weight + bias (the linear identity of SURVEY section 7).
 * The same operation as lime_linear_bf16 with c_ids (that kernel remains for other shapes); this one reads the tile once for all
 * N columns.  a_rows / out_rows: the row counts of a and out (32-bit offset checks).  m_dev: optional device row count.
 */
typedef struct {
    const uint16_t* a;   int64_t lda;  int64_t a_rows;  const int32_t* a_ids;
    const uint16_t* wp;
    const float* add_rows; int64_t ld_add; int32_t add_period;
    int32_t M, N, K;
    int32_t reserved;
    const int32_t* c_ids;
    uint16_t* out;       int64_t ldo;  int64_t out_rows;
    const int32_t* m_dev;
} lime_inproj_bf16_args;

int lime_inproj_bf16(const lime_inproj_bf16_args* args, void* stream);
int64_t lime_inproj_pack_bf16_size(int32_t N);
int lime_inproj_pack_bf16(const float* w, int64_t ldw, int32_t N, int32_t K, uint16_t* wp, void* stream);

/* the column count (304) the bf16 encoder-block kernels carry the model dimension in */
int32_t lime_ffn_bf16_model_columns(void);

/*
 * lime_to_bf16: dst[r, c] = bf16(src[r, c]) for r < rows, c < cols, zero for the padding up to [rows_out, cols_out]
 * (src fp32 [rows, cols] with leading dimension lds; dst bf16 [rows_out, ldd]).  Converts the word table, the weights
 * and pads K = 300 -> 304 / N = 300 -> 304 on the way.
 */
int lime_to_bf16(const float* src, int64_t lds, int64_t rows, int32_t cols, uint16_t* dst, int64_t ldd, int64_t rows_out,
                 int32_t cols_out, void* stream);

/* lime_mean_pool_bf16: out[s, 0:dim) = mean_t float(x[(s * S + t), 0:dim))  -- bf16 input, fp32 output */
int lime_mean_pool_bf16(const uint16_t* x, int64_t ldx, float* out, int64_t ldo, int32_t n_seq, int32_t S, int32_t dim,
                        void* stream);

/*
 * lime_embed_pe_f32: out[r, :] = table[ids[r], :] + pe[(r % period), :]   (pe may be NULL)
 * The stand-alone word-embedding gather (newsEncoders.py:311-312 + :827); the HBM-bound kernel of the
 * path.  ids int32 [rows]; table [V, dim]; out [rows, ldo].
 */
int lime_embed_pe_f32(const int32_t* ids, const float* table, int64_t ld_table, const float* pe, int64_t ld_pe,
                      int32_t period, float* out, int64_t ldo, int64_t rows, int32_t dim, void* stream);

/*
 * lime_compact_sequences: index lists for encoding only what differs in a batch of token sequences (ids int32 [n_seq, S], 0 = the
 * padding word).  The reference encodes every slot (newsEncoders.py:311-321), including history slots padded with the all-zero
 * <PAD> news (corpus.py:476-477) and the padding behind every text; those are exact repetitions:
 *   seq_inv  [n_seq]          compact index of every sequence; all-padding sequences share ONE representative (index n_live)
 *   ids_c    [(n_seq + 1) S]  ids in compact order (representative: zeros)
 *   row_map  [(n_seq + 1) S]  compact token row -> its q/k/v row: itself when live, pad_base + t for a padding token
 *   tok_ids / tok_rows [(n_seq + 1) S]  ids and compact rows of the live tokens, in (compact sequence, position) order; behind them S
 *                             more entries (id 0 -> row pad_base + t): the padding rows themselves, for callers that produce them
 *                             in the same in_proj launch (counts[4] rows)
 *   counts   [5]              n_live + 1, (n_live + 1) S, live tokens, n_live, live tokens + S   (device memory: the m_dev /
 *                             n_seq_dev arguments of the other entry points)
 * Ordered and deterministic (no atomics).  work: lime_compact_sequences_workspace(n_seq) int32 words.
 */
int lime_compact_sequences(const int32_t* ids, int32_t n_seq, int32_t S, int32_t pad_base, int32_t* seq_inv, int32_t* ids_c,
                           int32_t* row_map, int32_t* tok_ids, int32_t* tok_rows, int32_t* counts, int32_t* work, void* stream);

/* dst[r, 0 .. cols) = src[r % S, 0 .. cols) for every row r < rows with ids[r] == 0 (the padding word); other rows are left alone.  The q / k / v
 * rows of a padding token depend on its position only (table[0] W^T + (PE W^T + b)[t]): the training forward runs in_proj over the live
 * tokens (lime_linear_f32 with c_ids) and copies the S padding rows into the rest with this.  cols % 4 == 0, 16-byte aligned rows. */
int lime_fill_pad_rows_f32(const int32_t* ids, const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int32_t S, int32_t cols,
                           void* stream);
int64_t lime_compact_sequences_workspace(int32_t n_seq);

/*
 * lime_compact_batch: lime_compact_sequences for the titles (ids_t [n, T]) and the bodies (ids_b [n, L]) of n news, and the NEWS level,
 * in three launches (count, one-workgroup scan, emit).  The *_t / *_b outputs are lime_compact_sequences' for each text.  News level:
 * nothing behind the token encoders mixes news (intent layers, intent attention, LIME.project: row-wise in eval mode), so the
 * repetitions of the padding news need that arithmetic once.  News i repeats the padding news iff its title is all padding, its body
 * is all padding and its key (cat, sub, the BITS of fresh and life) equals the key of the FIRST news with an all-padding title and
 * body -- the representative.  A news that looks padded under another key stays live.
 *   news_src  [n + 1]   compact news -> original news: live news in order, then the representative (-1 when the batch has no
 *                       padding news; the count is then the number of live news); unused slots -1
 *   news_inv  [n]       original news -> compact news
 *   title_row / body_row [n + 1]   seq_inv_t[news_src[j]] / seq_inv_b[news_src[j]]; unused slots 0
 *   cat_c, sub_c, fresh_c, life_c [n + 1]   the keys in compact order; unused slots 0
 *   news_counts [4]     n_news, count_mult * n_news, live news, the representative's original index or -1  (device memory: m_dev arguments)
 * Ordered and deterministic (no atomics).  work: lime_compact_batch_workspace(n) int32 words; the two sides' seq_src lists
 * (compact -> original sequence) stay in it at work + n and work + 4 n + 2, n + 1 entries each.
 */
int lime_compact_batch(const int32_t* ids_t, int32_t T, int32_t pad_base_t, int32_t* seq_inv_t, int32_t* ids_c_t, int32_t* row_map_t,
                       int32_t* tok_ids_t, int32_t* tok_rows_t, int32_t* counts_t, const int32_t* ids_b, int32_t L, int32_t pad_base_b,
                       int32_t* seq_inv_b, int32_t* ids_c_b, int32_t* row_map_b, int32_t* tok_ids_b, int32_t* tok_rows_b, int32_t* counts_b,
                       int32_t n, const int32_t* cat, const int32_t* sub, const float* fresh, const float* life, int32_t count_mult,
                       int32_t* news_src, int32_t* news_inv, int32_t* title_row, int32_t* body_row, int32_t* cat_c, int32_t* sub_c,
                       float* fresh_c, float* life_c, int32_t* news_counts, int32_t* work, void* stream);
int64_t lime_compact_batch_workspace(int32_t n);

/*
 * lime_news_xin_f32: the pooled texts of the distinct news (lime_compact_batch) into the intent layers' input.  For j < min(cap, *n_news):
 *   xin[j, 0 .. dim)        = mean of the nblk_t rows  title_blocks[title_row[j] * nblk_t + 0 .. nblk_t)
 *   xin[cap + j, 0 .. dim)  = mean of the nblk_b rows  body_blocks[body_row[j] * nblk_b + 0 .. nblk_b)
 * rows added in order and scaled by 1 / nblk as lime_mean_pool_count_f32 does (nblk = 1: the row itself); the other rows and the columns
 * from dim on are left alone.  1 <= nblk <= 16, dim % 4 == 0, 16-byte aligned rows.
 */
int lime_news_xin_f32(const float* title_blocks, int64_t ld_t, int32_t nblk_t, const float* body_blocks, int64_t ld_b, int32_t nblk_b,
                      const int32_t* title_row, const int32_t* body_row, const int32_t* n_news, float* xin, int64_t ldx, int32_t cap,
                      int32_t dim, void* stream);

/*
 * lime_token_attention_f32: softmax(Q K^T * scale [+ key mask]) V per (sequence, head) in fp32, from one argument block.  Replaces the
 * attention core of nn.MultiheadAttention inside the TransformerEncoderLayers (newsEncoders.py:316,320; unmasked) and
 * layers.MultiHeadAttention.forward (layers.py:227-237; key mask filled with -1e9).  `form` says which call it is; fields a form does not
 * have are 0 / NULL.  Each form's refusals carry the name it had as an entry of its own (given with the form below).
 * Which kernels a call runs: DESIGN.md section 5.2 has the routing table, lime_token_attention_plan_f32 below returns a call's row.
 *
 * All forms: q / k / v row (seq * S + t), column (head * head_stride + d), d < head_dim, leading dimension ld_qkv (the three may alias
 * one packed buffer).  head_stride == head_dim is the packed layout of the reference; head_stride = 32 (heads padded with zero columns,
 * see lime_pad_heads_f32) lets the kernels use aligned 16-byte loads.  out[(seq * S + t) * ldo + head * head_dim + d] (always packed).
 * S <= 512, head_stride >= head_dim, and head_dim <= 32 -- or 32 < head_dim <= 128 under the wide-head limits stated at
 * lime_token_attention_bwd_workspace_wide (not the rows and vocab forms).
 *
 * PLAIN, COUNT (lime_token_attention_count_f32): key_mask uint8 [n_seq, S], 0 = masked, or NULL.  n_seq_dev, optional: a device int;
 * min(*n_seq_dev, n_seq) sequences are computed and n_seq is the capacity -- the masked attention of a compacted batch inside a HIP
 * graph, where the count changes per batch.  COUNT is PLAIN that hands a count over.
 *
 * LSE (lime_token_attention_lse_f32): no key mask, no device count; also writes lse [tokens, n_head] -- per (token, head) the
 * log2-domain log-sum-exp of the scaled scores, max + log2(sum 2^(s - max)) with s = scale * log2(e) * q . k -- for a training step
 * whose backward (LIME_BWD_ATTN_ENTRY_LSE) reads it: S > 128 pays a Q K^T pass of its own for the statistics otherwise.
 *
 * ROWS (lime_token_attention_rows_f32): unmasked, head_stride = 32, over COMPACTED sequences: the q / k / v row of token (seq * S + t)
 * is row_map[seq * S + t] -- a live token's own row, or one of the S rows that all padding tokens at position t share
 * (lime_compact_sequences); n_seq_dev as above.  out rows stay dense: (seq * S + t).  S in {32, 64, 96, 128, 256, 512}, head_dim <= 32;
 * q / k / v 16-byte aligned, ld_qkv % 4 == 0.
 *
 * VOCAB (lime_token_attention_vocab_f32): the attention of the FIRST encoder layer over a per-vocabulary in_proj product.  The q / k / v
 * row of token (seq * S + t) is qkv_vocab[ids[seq * S + t]] + pos_rows[t]: qkv_vocab is the [V, ld_qkv] table E W_in^T (q | k | v at
 * columns 0, W, 2W with W = n_head * 32), pos_rows the [S, ld_qkv] table PE W_in^T + b in the same layout, the sum one fp32 add per
 * element -- bit for bit PLAIN over the materialised rows.  The block holds q = qkv_vocab, k = q + W, v = q + 2 W, row_map = ids,
 * head_stride = 32.  A padding token is id 0 at its position; ids are not range-checked; n_seq_dev as above.  Split-product kernel
 * only: returns LIME_NOT_APPLICABLE, launching nothing, under lime_set_split_gemm(0) or outside S in {32, 64, 128}, head_dim <= 32,
 * ld_qkv % 4 == 0, 3 W <= ld_qkv <= 2^21, 16-byte aligned tables -- the caller then runs in_proj and the ROWS form.
 *
 * DROPOUT (lime_token_attention_dropout_f32): dropout on the probabilities (nn.MultiheadAttention(dropout=p) in training mode):
 * out = (keep * softmax(scale q k^T) / (1 - p)) v, no key mask, mask element ((seq * n_head + head) * S + i) * S + j drawn from
 * (dropout_p, dropout_seed, dropout_site) as stated at lime_dropout_f32.  head_dim <= 32 needs head_stride <= 32; there S > 128 runs
 * in 128 x 128 blocks and needs lime_token_attention_stats_workspace(n_seq, S, n_head) floats of workspace (the row statistics; the
 * larger lime_token_attention_bwd_workspace does as well), else workspace may be NULL.
 */
enum { LIME_ATTN_FORM_PLAIN = 0, LIME_ATTN_FORM_COUNT = 1, LIME_ATTN_FORM_LSE = 2, LIME_ATTN_FORM_ROWS = 3, LIME_ATTN_FORM_VOCAB = 4,
       LIME_ATTN_FORM_DROPOUT = 5 };
typedef struct {
    const float* q;
    const float* k;
    const float* v;
    int64_t ld_qkv;
    const float* pos_rows;
    const int32_t* row_map;
    const uint8_t* key_mask;
    const int32_t* n_seq_dev;
    float* lse;
    float* out;
    int64_t ldo;
    float* workspace;
    int64_t workspace_floats;
    uint64_t dropout_seed;
    float dropout_p;
    uint32_t dropout_site;
    int32_t n_seq, S, n_head, head_dim, head_stride;
    float scale;
    int32_t form;
    int32_t reserved;
} lime_token_attention_args;

int lime_token_attention_f32(const lime_token_attention_args* args, void* stream);

/* What the fp32 token-attention forward would run for an argument block, without running it: the routing decision
 * (csrc/token_attn_f32.hip, lime_attn_route) as data.  A pure function of the block and the
 * lime_set_split_gemm() setting: no launch, no call into the HIP runtime, no pointer of the block is read through (only NULL-ness
 * and alignment count); the CU count sizes the grids and chooses no kernel.  Returns what lime_token_attention_f32 would return
 * where it launches nothing -- the form's refusal (same status, same lime_last_error_string()) or LIME_NOT_APPLICABLE (vocab form) -- else
 * LIME_OK and
 *   family      LIME_ATTN_SP token_attn_sp_kernel (split product, S = 32 / 64 / 128 in one pass), _SP_LONG token_attn_sp_long_kernel
 *               (S = 256 / 512 in key blocks), _SP_VOCAB token_attn_sp_vocab_kernel, _MFMA token_attn_kernel (exact-fp32 MFMA),
 *               _WIDE wide_fwd_kernel (head_dim > 32), _DROPOUT token_attn_fwd_dropout_kernel (one pass, S <= 128), _DROPOUT_LONG
 *               attn_fwd_long_dropout_kernel (key blocks); LIME_ATTN_NONE for n_seq == 0 (nothing is launched)
 *   stats_pass  the row-statistics launch in front of it: LIME_ATTN_STATS_NONE, _FP32 (attn_stats_kernel<false>) or _SPLIT
 *               (attn_stats_kernel<true>: Q K^T as split products)
 *   n_launches  0, 1 or 2
 *   name        the n_launches instantiations in launch order, as rocprofv3 prints them */
enum { LIME_ATTN_NONE = 0, LIME_ATTN_SP = 1, LIME_ATTN_SP_LONG = 2, LIME_ATTN_SP_VOCAB = 3, LIME_ATTN_MFMA = 4, LIME_ATTN_WIDE = 5,
       LIME_ATTN_DROPOUT = 6, LIME_ATTN_DROPOUT_LONG = 7 };
enum { LIME_ATTN_STATS_NONE = 0, LIME_ATTN_STATS_FP32 = 1, LIME_ATTN_STATS_SPLIT = 2 };
typedef struct {
    int32_t family;
    int32_t stats_pass;
    int32_t n_launches;
    int32_t reserved;
    char name[2][64];
} lime_token_attention_plan;

int lime_token_attention_plan_f32(const lime_token_attention_args* args, lime_token_attention_plan* out);

/* lime_token_attention_rows_bf16: lime_token_attention_bf16 over compacted sequences (row_map / n_seq_dev as in
 * the ROWS form of lime_token_attention_f32); S in {32, 64, 128}, even head_dim. */
int lime_token_attention_rows_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld_qkv, const int32_t* row_map,
                                   const int32_t* n_seq_dev, uint16_t* out, int64_t ldo, int32_t n_seq, int32_t S, int32_t n_head,
                                   int32_t head_dim, float scale, int32_t out_cols, void* stream);

/*
 * lime_token_attention_bf16: the unmasked encoder-layer attention on bf16 storage (config 3): q / k / v bf16 with every
 * head at 32 columns (64-byte head rows), out bf16 packed [.., n_head * head_dim] plus zero columns up to out_cols (the
 * K padding the next GEMM reads).  S in {32, 64, 128}: Q.K^T and P.V on v_mfma_f32_32x32x16_bf16 (fp32 scores, softmax and
 * accumulation; P rounded to bf16); S in {256, 512}: operands widened to fp32, fp32 MFMA core.
 */
int lime_token_attention_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t ld_qkv, uint16_t* out,
                              int64_t ldo, int32_t n_seq, int32_t S, int32_t n_head, int32_t head_dim, float scale,
                              int32_t out_cols, void* stream);

/*
 * lime_pad_heads_f32: dst[(blk * head_stride + d), :] = d < head_dim ? src[(blk * head_dim + d), :] : 0 for blk < n_blk.
 * Pads the rows of in_proj_weight / in_proj_bias (n_blk = 3 * n_head blocks of head_dim rows, `cols` columns) so that the
 * in_proj GEMM writes every head at a 128-byte aligned column offset.  src [n_blk * head_dim, cols] (ld lds),
 * dst [n_blk * head_stride, cols] (ld ldd).
 */
int lime_pad_heads_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t n_blk, int32_t head_dim,
                       int32_t head_stride, int32_t cols, void* stream);

/* lime_mean_pool_f32: out[s, :] = mean_t x[(s * S + t), :]   (newsEncoders.py:317,321; padding included) */
int lime_mean_pool_f32(const float* x, int64_t ldx, float* out, int64_t ldo, int32_t n_seq, int32_t S, int32_t dim,
                       void* stream);
/* the same over the first min(n_seq, *n_seq_dev) sequences (a compacted batch: device-side count, the rows behind it are not
 * read and their outputs not written); S <= 16 rows per sequence (the block means `pool32` leaves), dim % 4 == 0 */
int lime_mean_pool_count_f32(const float* x, int64_t ldx, float* out, int64_t ldo, int32_t n_seq, int32_t S, int32_t dim,
                             const int32_t* n_seq_dev, void* stream);

/*
 * lime_bucketize_f32: b = min(trunc(log(max(x,1)) / log(86400) * (10/7)), 9)  (newsEncoders.py:53-58),
 * evaluated by comparison against the nine fp32 cut points of the reference's own fp32 evaluation, so the
 * indices are bit-exact without a device logf.  out int32 [n].  NaN -> 0, +inf -> 9 (the reference raises).
 */
int lime_bucketize_f32(const float* x, int32_t* out, int64_t n, void* stream);
/* The same rule for another num_buckets (config.py:59): out = #{k : x >= cuts[k]} against an ascending device table of the
 * num_buckets - 1 fp32 cut points of b = min(trunc(log(max(x,1)) / log(86400) * (num_buckets/7)), num_buckets - 1), which the
 * host derives from the reference formula's own fp32 evaluation (lime_cikm25_amd.newsEncoders.bucket_cut_points). */
int lime_bucketize_cuts_f32(const float* x, const float* cuts, int32_t n_cuts, int32_t* out, int64_t n, void* stream);

/*
 * lime_topic_rep_f32: out[r, :] = category_affine(cat[cat_table[cat[r]], sub_table[sub[r]]])
 * (newsEncoders.py:340-342 and userEncoders.py:103-105,115-117).  cat/sub int32 [rows]; tables [*, dc]/[*, ds];
 * w [dout, dc + ds]; also writes the two raw embedding rows to emb_out[r, 0:dc+ds] when emb_out != NULL
 * (feature_fusion, newsEncoders.py:221-225).
 */
int lime_topic_rep_f32(const int32_t* cat, const int32_t* sub, const float* cat_table, const float* sub_table,
                       int32_t dc, int32_t ds, const float* w, const float* bias, int32_t dout, float* out, int64_t ldo,
                       float* emb_out, int64_t ld_emb, int64_t rows, void* stream);

/*
 * lime_news_keys_f32: what the tail over the distinct news of a batch (lime_compact_batch) takes from the compact keys, in one launch
 * over `rows` = the capacity n + 1 (unused slots hold key 0: a valid id and bucket).  For compact news j:
 *   pair[j]                           = bucket(fresh[j]) * nb + bucket(life[j])   (the rule of lime_bucketize_f32 when cuts == NULL
 *                                       and nb == 10, else of lime_bucketize_cuts_f32 with n_cuts == nb - 1 ascending device cut points)
 *   xin[j, col0 .. col0 + dout)       = lime_topic_rep_f32's row (same lanes, same order of the sums: the same bits)
 *   xin[rows + j, col0 .. col0 + dout) = the same row again (the title half and the body half of the intent layers' input)
 *   xin[j | rows + j, col0 + dout .. ldx) = 0                                     (the pad columns that keep the rows 16-byte aligned)
 *   emb_out[j, 0 .. dc + ds)          = the two raw embedding rows
 * xin is [2 rows, ldx]; its columns [0, col0) are not touched (lime_news_xin_f32 writes them).  w [dout, dc + ds]; bias may be NULL.
 */
int lime_news_keys_f32(const int32_t* cat, const int32_t* sub, const float* fresh, const float* life, const float* cuts, int32_t n_cuts,
                       int32_t nb, const float* cat_table, const float* sub_table, int32_t dc, int32_t ds, const float* w,
                       const float* bias, int32_t dout, float* xin, int64_t ldx, int32_t col0, float* emb_out, int64_t ld_emb,
                       int32_t* pair, int64_t rows, void* stream);

/*
 * lime_intent_fuse_f32: the tail of newsEncoders.CROWN.forward (:355-371).
 *   intents   [2, M, k, D]  title rows then body rows (the relu'd intent embeddings, :288)
 *   att_hidden[2, M, k, A]  tanh(affine1(intents)) (layers.py:288)
 *   affine2_t / affine2_b [A]  (layers.py:290, no bias)
 *   per news: alpha = softmax_k(att_hidden . affine2); x = sum_k alpha_k intents_k (layers.py:296-299), for title
 *   and body; s = (cos(title, body) + 1) / 2 (:297-300); content[m] = [title(D), s * body(D)] written at
 *   content[m * ldc + 0 .. 2D).
 */
int lime_intent_fuse_f32(const float* intents, const float* att_hidden, const float* affine2_t, const float* affine2_b,
                         float* content, int64_t ldc, int64_t M, int32_t k, int32_t D, int32_t A, void* stream);
/* the same over the first min(M, *m_dev) news (device-side count; the rows behind it are neither read nor written); M stays the
 * capacity that places the body half of intents / att_hidden */
int lime_intent_fuse_count_f32(const float* intents, const float* att_hidden, const float* affine2_t, const float* affine2_b,
                               float* content, int64_t ldc, int64_t M, int32_t k, int32_t D, int32_t A, const int32_t* m_dev, void* stream);

/*
 * lime_additive_pool_f32: layers.Attention.forward (layers.py:285-300) after affine1:
 *   a[t] = hidden[s, t, :] . affine2;  masked_fill(mask == 0, -1e9);  alpha = softmax_t;  out[s] = sum_t alpha_t x[s, t, :]
 * hidden [n_seq * S, A] (ld ldh), x [n_seq * S, D] (ldx), mask uint8 [n_seq, S] or NULL, out [n_seq, ldo].
 */
int lime_additive_pool_f32(const float* hidden, int64_t ldh, const float* affine2, int32_t A, const float* x, int64_t ldx,
                           int32_t D, const uint8_t* mask, float* out, int64_t ldo, int32_t n_seq, int32_t S, void* stream);
/* the same with an optional device-side sequence count: sequences >= min(*n_seq_dev, n_seq) are skipped, their output rows untouched (the
 * compacted batch of newsEncoders.MHSA: the rows behind the live sequences hold stale data) */
int lime_additive_pool_count_f32(const float* hidden, int64_t ldh, const float* affine2, int32_t A, const float* x, int64_t ldx, int32_t D,
                                 const uint8_t* mask, const int32_t* n_seq_dev, float* out, int64_t ldo, int32_t n_seq, int32_t S, void* stream);

/*
 * lime_cand_attn_weights_f32: the attention-weight part of CandidateAware_ClickedNewsAttention.forward
 * (layers.py:70-81), one workgroup per row b.  qp = query_proj(cand_topic) [B, N, D] and kp = key_proj(hist_topic)
 * [B, H, D] come from lime_linear_f32 (layers.py:66-67).  Per head (D / n_head columns, staged in LDS):
 * scores = Q_h K_h^T / sqrt(D); masked_fill(mask == 0, -1e9); softmax over H (row max / sum by wave64 shuffles);
 * then query weights qw = softmax_N(||Q_n||_2) (:79) and agg = softmax_H(sum_n qw_n sum_heads A) (:80-81).
 * mask uint8 [B, H] (0 = padded history slot); agg out [B, H].  Requires N <= 128, H <= 512.
 */
int lime_cand_attn_weights_f32(const float* qp, const float* kp, const uint8_t* mask, float* agg, int32_t B, int32_t N,
                               int32_t H, int32_t D, int32_t n_head, void* stream);
/* The same result with (row, head) parallelism -- one wave per (b, head) writes that head's softmaxed weights and its share of
 * ||Q_n||^2 to `workspace` (lime_cand_attn_weights_workspace(B, N, H, n_head) floats), one workgroup per row sums the heads in head
 * order and finishes: two short launches that fill the chip at B = 32 (the one-workgroup-per-row kernel above: 32 workgroups, 64 us). */
int64_t lime_cand_attn_weights_workspace(int32_t B, int32_t N, int32_t H, int32_t n_head);
int lime_cand_attn_weights_ws_f32(const float* qp, const float* kp, const uint8_t* mask, float* agg, int32_t B, int32_t N, int32_t H,
                                  int32_t D, int32_t n_head, float* workspace, int64_t workspace_floats, void* stream);
/* the same with ONE history (kp [B / hist_div, H, D], mask [B / hist_div, H]) shared by hist_div consecutive rows: the K candidate rows of an
 * impression in Model.score_impressions -- their key projections and topic representations are computed once per impression, not per row */
int lime_cand_attn_weights_shared_f32(const float* qp, const float* kp, const uint8_t* mask, float* agg, int32_t B, int32_t N, int32_t H,
                                      int32_t D, int32_t n_head, int32_t hist_div, float* workspace, int64_t workspace_floats, void* stream);

/*
 * lime_gate_ln_f32: the gated residual + LayerNorm of CandidateAware_ClickedNewsAttention (layers.py:84-89), one
 * workgroup per history row.  y = gate_proj.weight . x (no bias, from lime_linear_f32), s = agg[row]:
 *   g = sigmoid(s * y + bias);  v = g * (s * x) + (1 - g) * x;  out = LayerNorm(v) * gamma + beta
 * (gate_proj(s * x) = s * (W x) + b: the row scale commutes with the projection).  x, y, out: [rows, D] contiguous.
 */
int lime_gate_ln_f32(const float* y, const float* x, const float* scale, const float* bias, const float* gamma,
                     const float* beta, float eps, float* out, int64_t rows, int32_t D, void* stream);

/* lime_gate_ln_f32 over the H history rows of each user row and the GraphSAGE aggregate of the result in one pass (layers.py:83-91 +
 * userEncoders.py:121,151-157).  Group g (one impression row of the user encoder; `groups` of them) reads its H history rows from
 * impression g / row_div -- x and y = gate_proj(x) are [groups / row_div, H, D]: Model.score_impressions keeps ONE copy of a history for
 * its row_div candidates -- and scale[g * H + h]; writes out[g, h, :] as lime_gate_ln_f32 does and
 *     mean_out[g, :] = (sum_{h < min(H, n_src)} out[g, h, :] + node_const) / n_src,
 * node_const [D] = the sum of the first n_src - H user-node rows (the part of the SAGEConv mean that is the same for every row; may be
 * NULL when n_src <= H).  D <= 512. */
int lime_gate_ln_sage_f32(const float* y, const float* x, const float* scale, const float* bias, const float* gamma, const float* beta,
                          float eps, float* out, const float* node_const, float* mean_out, int64_t groups, int32_t H, int32_t D,
                          int32_t row_div, int32_t n_src, void* stream);

/*
 * lime_sage_mean_f32: m[b, :] = mean over the first n_src node slots of row b of cat[hist[b] (H rows),
 * user_nodes (n_user rows)] -- the aggregation PyG's SAGEConv performs for the edge list of
 * create_bipartite_graph (userEncoders.py:91-98,121,153).  Requires n_src <= H + n_user.
 */
int lime_sage_mean_f32(const float* hist, const float* user_nodes, float* out, int32_t B, int32_t H, int32_t n_user,
                       int32_t n_src, int32_t D, void* stream);

/*
 * lime_interest_match_f32: userEncoders.py:163-169 + util.py:23-49 fused, one workgroup per (row b, candidate n):
 *   a[n, h] = kp[b, h, :] . qp[b, n, :] * scale;  alpha = softmax_h (unmasked);  u[b, n, :] = sum_h alpha g[b, h, :]
 *   base = u . cand[b, n, :];  w = sigmoid(alpha_s * r) (x beta_s where r < 0 when use_penalty; |r| when not)
 *   logits[b, n] = use_weight ? base * w : base;   user_rep receives u.  Either of user_rep / logits may be NULL.
 * kp [B, H, A], qp [B, N, A], g [B, H, D], cand [B, N, D], remaining [B, N].
 */
int lime_interest_match_f32(const float* kp, const float* qp, const float* g, const float* cand, const float* remaining,
                            float* user_rep, float* logits, int32_t B, int32_t N, int32_t H, int32_t A, int32_t D,
                            float scale, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty,
                            void* stream);

/*
 * lime_lifetime_score_f32: RemainingLifetimeWeighting.forward stand-alone (util.py:23-49):
 * logits[r] = (user[r, :] . news[r, :]) * w(remaining[r]); rows = B * N.  Same weight rule as above.
 */
int lime_lifetime_score_f32(const float* user, const float* news, const float* remaining, float* logits, int64_t rows,
                            int32_t D, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty, void* stream);

/* lime_row_scale_f32: out[r, :] = scale[r] * x[r, :]   (layers.py:84 when use_residual_connection is off) */
int lime_row_scale_f32(const float* x, const float* scale, float* out, int64_t rows, int32_t D, void* stream);

/*
 * The masked title encoder (newsEncoders.py:566-595, LIME-MHSA-CROWN) on a compacted batch.  lime_mhsa_live_ids: ids_eff = ids with
 * -1 in the first position of every all-zero sequence whose key mask is NOT the padding news' mask (first position set,
 * corpus.py:476-477): such a sequence must be encoded, and the sentinel makes lime_compact_sequences count it as live.
 * lime_mhsa_compact_mask: behind lime_compact_sequences -- ids_c[e] = max(ids_c[e], 0) (the sentinel back to the padding word) and
 * mask_c[cs, t] = mask[seq_src[cs], t] (a compact slot without a source sequence gets the padding news' mask); n_compact_slots =
 * n_seq + 1.  mask / mask_c: uint8, non-zero = attend.
 */
int lime_mhsa_live_ids(const int32_t* ids, const uint8_t* mask, int32_t n_seq, int32_t T, int32_t* ids_eff, void* stream);
int lime_mhsa_compact_mask(int32_t* ids_c, const int32_t* seq_src, const uint8_t* mask, int32_t n_compact_slots, int32_t T,
                           uint8_t* mask_c, void* stream);

/* lime_fuse_rows_f32: LIME's fusion_method 'add' (gate == NULL: out = a + b) and 'gated' (out = gate * a + (1 - gate) * b),
 * newsEncoders.py:154-159; [rows, cols] matrices with leading dimensions. */
int lime_fuse_rows_f32(const float* a, int64_t lda, const float* b, int64_t ldb, const float* gate, int64_t ldg, float* out, int64_t ldo,
                       int64_t rows, int32_t cols, void* stream);

/* lime_gather_rows_f32: out[r, 0:dim) = table[idx[r], 0:dim)   (nn.Embedding lookups of small tables) */
int lime_gather_rows_f32(const int32_t* idx, const float* table, int64_t ld_table, float* out, int64_t ldo, int64_t rows,
                         int32_t dim, void* stream);

/*
 * lime_multi_copy: dst_i[0:bytes_i) = src_i[0:bytes_i) for up to LIME_MAX_COPIES device buffers in ONE launch.
 * The drop-in Model replays a HIP graph captured on its own input buffers; the caller's 17 input tensors
 * (model.py:151-154) are moved there with this instead of 17 separate copies (5 us of launch floor each).
 * `descs` is a HOST array (the only host pointer of this ABI; it is copied into the kernel arguments before the call
 * returns).  Buffers must not overlap.
 */
#define LIME_MAX_COPIES 32
typedef struct {
    const void* src;
    void* dst;
    int64_t bytes;
} lime_copy_desc;
int lime_multi_copy(const lime_copy_desc* descs, int32_t n, void* stream);

/*
 * lime_gather_rows_multi: for up to LIME_MAX_GATHERS tables at once, out_f[r, 0:row_bytes_f) = table_f[idx[r], 0:row_bytes_f)
 * (byte rows; strides in bytes).  The device-side batch assembly of dataset.py:105-141 / :192-227: one launch gathers the
 * eight per-news arrays (category, subCategory, title / abstract text, mask, entity: corpus.py:360-367) of every history
 * slot and candidate of a batch by news index, another the per-behaviour rows by behaviour index.  idx int32 [n_rows];
 * `descs` is a HOST array (copied into the kernel arguments).  Indices are not range checked (as nn.Embedding's device path).
 */
#define LIME_MAX_GATHERS 16
typedef struct {
    const void* table;  int64_t table_stride;   /* bytes between table rows */
    void* out;          int64_t out_stride;     /* bytes between output rows */
    int32_t row_bytes;  int32_t reserved;
} lime_gather_desc;
int lime_gather_rows_multi(const int32_t* idx, int64_t n_rows, const lime_gather_desc* descs, int32_t n, void* stream);

/* =====================================================================================================
 * Training step: the backward of the token encoder layers and the optimizer of
 * trainer.py:33,71-73,131-148.  Gradients of matrix products reuse lime_linear_f32 (dX = dY . W with the transposed
 * weight as its W operand); the entry points below are the pieces lime_linear_f32 cannot express.  Dense reductions
 * over the rows go through caller-provided workspaces and are fixed-order; lime_embed_bwd_f32 alone uses float atomics
 * (a word row receives contributions from many tokens), so the word-table gradient is reproducible only up to the
 * order of its fp32 additions.
 * ===================================================================================================== */

/* dW[n, k] (+)= sum_m dy[m, n] * x[m, k]: the weight gradient of y = x W^T (nn.Linear backward; loss.backward() at
 * trainer.py:145).  dy [M, N], x [M, K], dw [N, K]; exact-fp32 MFMA, M split over workgroups, partial tiles in
 * `workspace` (lime_linear_wgrad_workspace(M, N, K) floats), summed in split order.  accumulate != 0: dw += ...
 * db (optional, [N]) (+)= sum_m dy[m, n], the bias gradient: taken in the same pass as an extra all-ones column of x when
 * the padded tile grid has room for one (K = 300 of the encoder layers does), else by a column-sum pass. */
int64_t lime_linear_wgrad_workspace(int32_t M, int32_t N, int32_t K);
int lime_linear_wgrad_f32(const float* dy, int64_t ldy, const float* x, int64_t ldx, float* dw, int64_t lddw, float* db,
                          int32_t M, int32_t N, int32_t K, int32_t accumulate, float* workspace, int64_t workspace_floats,
                          void* stream);

/* out[n] (+)= sum_m x[m, n]: the bias gradient.  workspace: lime_colsum_workspace(M, N) floats. */
int64_t lime_colsum_workspace(int32_t M, int32_t N);
int lime_colsum_f32(const float* x, int64_t ldx, int32_t M, int32_t N, float* out, int32_t accumulate, float* workspace,
                    int64_t workspace_floats, void* stream);

/* Backward of y = LayerNorm(z) (norm1 / norm2 of the encoder layers, newsEncoders.py:244-247) from what the forward keeps:
 * y itself and rstd (lime_linear_args.ln_rstd); xhat is recovered as (y - beta) / gamma (gamma must be non-zero).
 *   dY(r, :) = dy[(r / dy_div), :] * dy_scale      (dy_div = S, dy_scale = 1 / S: the mean pooling of :317,:321 folded in)
 *   dz[r, :] = rstd[r] * (g - mean(g) - xhat * mean(g * xhat)),  g = dY * gamma
 *   dgamma (+)= sum_r dY * xhat;  dbeta (+)= sum_r dY;  dzsum (+)= sum_r dz (the bias gradient of the linear layer whose
 *   output fed the residual sum); each of the three may be NULL.  E <= 512.
 * workspace: lime_layernorm_bwd_workspace(M, E) floats. */
int64_t lime_layernorm_bwd_workspace(int32_t M, int32_t E);
int lime_layernorm_bwd_f32(const float* dy, int64_t lddy, int32_t dy_div, float dy_scale, const float* y, int64_t ldy,
                           const float* gamma, const float* beta, const float* rstd, float* dz, int64_t lddz, int32_t M,
                           int32_t E, float* dgamma, float* dbeta, float* dzsum, int32_t accumulate, float* workspace,
                           int64_t workspace_floats, void* stream);
/* The same with a second result dz_drop[r, c] = keep(r * E + c) ? dz[r, c] / (1 - p) : 0 -- the gradient through the dropout that sits in
 * front of the residual add (dropout1 / dropout2 of the encoder layer, newsEncoders.py:244-247) with the forward's (p, seed, site) --
 * written in the same pass instead of a lime_dropout_f32 pass over dz; `dzsum` is then the column sums of dz_drop (the bias gradient of
 * the linear in front of that dropout), not of dz.  16-byte friendly operands only. */
int lime_layernorm_bwd_dropout_f32(const float* dy, int64_t lddy, int32_t dy_div, float dy_scale, const float* y, int64_t ldy,
                                   const float* gamma, const float* beta, const float* rstd, float* dz, int64_t lddz, int32_t M, int32_t E,
                                   float* dgamma, float* dbeta, float* dzsum, int32_t accumulate, float* workspace,
                                   int64_t workspace_floats, float* dz_drop, int64_t lddd, float dropout_p, uint64_t seed, uint32_t site,
                                   void* stream);

/* dh[r, c] = h[r, c] > 0 ? dh[r, c] * scale : 0, in place: ReLU backward on the saved activation of linear1 (scale = 1), or
 * ReLU + the dropout that follows it when h is the dropped-out activation (scale = 1 / (1 - p)) */
int lime_relu_bwd_f32(float* dh, int64_t lddh, const float* h, int64_t ldh, int64_t rows, int32_t cols, float scale, void* stream);

/* lime_token_attention_bwd_f32 (below, behind its argument block): backward of lime_token_attention_f32 (the encoder layers;
 * optionally the key mask of MHSA).  Given q / k / v as the forward read them and dout [tokens, n_head * head_dim] (packed), writes dq / dk / dv in the layout of q / k / v (row stride ld_dqkv, head
 * h at column h * head_stride; columns head_dim .. head_stride - 1 come out as zeros).  The probabilities are recomputed.
 * S <= 512, head_dim <= head_stride <= 32 (wider heads: see lime_token_attention_bwd_workspace_wide below).  S <= 128: one pass per (sequence, head); `out` and `workspace` may be NULL.
 * 128 < S <= 512 (the 512-token bodies of BASELINE config 4): 128 x 128 blocks; needs the forward output `out` (packed like
 * dout) and lime_token_attention_bwd_workspace(n_seq, S, n_head) floats: the row statistics and one dq slab per key block behind the
 * first -- the key blocks' shares of dq are stored (no atomics) and summed in block order, so the result is bitwise reproducible.  dropout_p > 0: the forward was the DROPOUT form with the same (dropout_p, seed, site).
 * key_mask (uint8 [n_seq, S], 0 = masked, or NULL; S <= 128): the masked attention of layers.MultiHeadAttention
 * (layers.py:227-232) -- masked scores are constants (-1e9) and receive no gradient.
 * Which kernels a call runs: DESIGN.md section 5.5 has the routing table, lime_token_attention_bwd_plan_f32 below returns a call's row. */
int64_t lime_token_attention_bwd_workspace(int32_t n_seq, int32_t S, int32_t n_head);
/* the row-statistics part of it (lse and delta per (token, head)): what the forward's DROPOUT form needs for S > 128 */
int64_t lime_token_attention_stats_workspace(int32_t n_seq, int32_t S, int32_t n_head);
/* Wide heads (32 < head_dim <= 128, head_dim % 4 == 0, head_stride % 4 == 0, S <= 512, 16-byte aligned operands, leading dimensions
 * multiples of 4; csrc/token_attn_wide_f32.hip): lime_token_attention_f32 (forms PLAIN, COUNT, LSE, DROPOUT) and
 * lime_token_attention_bwd_f32 send them to exact-fp32 MFMA kernels that stream the keys in blocks of 64 (key mask, device
 * count, lse output and dropout as for the narrow heads; lime_set_split_gemm has no effect on them).  Their backward recomputes the row
 * statistics at every S (`out` and `lse` are accepted and not read), sums in a fixed order (bitwise reproducible) and needs
 * lime_token_attention_bwd_workspace_wide(n_seq, S, n_head, head_dim) floats of workspace -- for head_dim <= 32 that is
 * lime_token_attention_bwd_workspace(n_seq, S, n_head).  The forward with dropout needs no workspace for wide heads. */
int64_t lime_token_attention_bwd_workspace_wide(int32_t n_seq, int32_t S, int32_t n_head, int32_t head_dim);
/* `entry` says which backward it is.  PLAIN does not look at lse.  LSE (its own two refusals speak as lime_token_attention_bwd_lse_f32,
 * all others as lime_token_attention_bwd_f32): behind a forward of the LSE form, reading the lse [tokens, n_head] it wrote instead of
 * recomputing the statistics (S > 128); dropout_p = 0, key_mask = NULL. */
enum { LIME_BWD_ATTN_ENTRY_PLAIN = 0, LIME_BWD_ATTN_ENTRY_LSE = 1 };
typedef struct {
    const float* q;
    const float* k;
    const float* v;
    int64_t ld_qkv;
    const float* out;
    int64_t ld_out;
    const float* lse;
    const float* dout;
    int64_t ldo;
    float* dq;
    float* dk;
    float* dv;
    int64_t ld_dqkv;
    float* workspace;
    int64_t workspace_floats;
    const uint8_t* key_mask;
    uint64_t dropout_seed;
    float dropout_p;
    uint32_t dropout_site;
    int32_t n_seq, S, n_head, head_dim, head_stride;
    float scale;
    int32_t entry;
    int32_t reserved;
} lime_token_attention_bwd_args;

int lime_token_attention_bwd_f32(const lime_token_attention_bwd_args* args, void* stream);

/* What lime_token_attention_bwd_f32 would run for an argument block, without running it: the backward's routing
 * decision (csrc/token_attn_f32.hip, lime_attn_bwd_route; DESIGN.md section 5.5 has the table) as data, under the contract of
 * lime_token_attention_plan_f32 -- a pure function of the block and the lime_set_split_gemm() setting, no launch, no pointer read
 * through.  Returns the entry's refusal (same status, same lime_last_error_string()) where it launches nothing, else LIME_OK and
 *   family      LIME_BWD_ATTN_ONE_PASS token_attn_bwd_kernel<32 | 64 | 128> (exact-fp32 MFMA, S <= 128), _SP attn_bwd_sp_kernel<FULL>
 *               (split product, 64 < S <= 128), _LONG attn_bwd_long_kernel / _LONG_SP attn_bwd_long_sp_kernel (key blocks, S > 128),
 *               _WIDE wide_bwd_q_kernel<NK> + wide_bwd_kv_kernel<NK> (head_dim > 32); LIME_BWD_ATTN_NONE for n_seq == 0
 *   stats_pass  the launch in front of a blocked kernel: LIME_BWD_ATTN_PASS_NONE, _STATS_FP32 (attn_stats_kernel<false>), _STATS_SPLIT
 *               (attn_stats_kernel<true>) or _DELTA (attn_delta_kernel: the lse entry)
 *   n_launches  0 to 3 (a blocked kernel is followed by attn_dq_reduce_kernel)
 *   name        the n_launches instantiations in launch order, as rocprofv3 prints them */
enum { LIME_BWD_ATTN_NONE = 0, LIME_BWD_ATTN_ONE_PASS = 1, LIME_BWD_ATTN_SP = 2, LIME_BWD_ATTN_LONG = 3, LIME_BWD_ATTN_LONG_SP = 4,
       LIME_BWD_ATTN_WIDE = 5 };
enum { LIME_BWD_ATTN_PASS_NONE = 0, LIME_BWD_ATTN_PASS_STATS_FP32 = 1, LIME_BWD_ATTN_PASS_STATS_SPLIT = 2, LIME_BWD_ATTN_PASS_DELTA = 3 };
typedef struct {
    int32_t family;
    int32_t stats_pass;
    int32_t n_launches;
    int32_t reserved;
    char name[3][64];
} lime_token_attention_bwd_plan;

int lime_token_attention_bwd_plan_f32(const lime_token_attention_bwd_args* args, lime_token_attention_bwd_plan* out);

/* Backward of lime_additive_pool_f32 (layers.Attention over a title's tokens, layers.py:285-300 / newsEncoders.py:591-592; the MHSA content
 * encoder in training): dhidden [n_seq * S, A], dx [n_seq * S, D] and da2_part [n_seq, A], the per-sequence partial rows of the
 * affine2 gradient (sum them with lime_colsum_f32).  Masked tokens receive no score gradient (their score is the constant -1e9). */
int lime_additive_pool_bwd_f32(const float* hidden, int64_t ldh, const float* affine2, int32_t A, const float* x, int64_t ldx, int32_t D,
                               const uint8_t* mask, const float* dout, int64_t ldo, float* dhidden, int64_t lddh, float* dx, int64_t lddx,
                               float* da2_part, int32_t n_seq, int32_t S, void* stream);

/* ---- dropout inside the token encoders in training mode --------------------------------------------------------------
 * Masks are a pure function of (seed, site, element index) (csrc/dropout.h); the backward regenerates the mask from the same
 * triple.  One splitmix64 value serves four consecutive elements, 16 bits each:
 *     key    = seed * 0x9E3779B97F4A7C15 + (uint64)(uint32)(site + 1) * 0xD1B54A32D192ED03          (wrapping uint64)
 *     z      = (e >> 2) + key;  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *     thresh = p <= 0 ? 0 : min(floor(p * 2^16 + 0.5), 0xFFFF)                                     (round(p * 2^16))
 *     element e is kept iff ((z >> 16 (e & 3)) & 0xFFFF) >= thresh
 * so p is realised in steps of 2^-16 (the keep probability is 1 - thresh / 2^16), while kept values are scaled by the exact fp32
 * 1 / (1 - p).  tests/dropout_cases.py states the same on the host.  torch's Philox stream is not reproduced (it differs between
 * torch's own CPU and GPU generators as well). */

/* dst[r, c] = keep(r * cols + c) ? src[r, c] / (1 - p) : 0   (src == dst allowed).  Forward of nn.Dropout, and -- applied to a
 * gradient with the forward's (seed, site) -- its backward. */
int lime_dropout_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int32_t cols, float p, uint64_t seed,
                     uint32_t site, void* stream);
/* dst = dropout_site2(dropout_site1(src)) in one pass (the same values as two lime_dropout_f32 calls): the backward through the two
 * input dropouts of an encoder layer (positional, then embedding: newsEncoders.py:311-312, :827). */
int lime_dropout2_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int32_t cols, float p, uint64_t seed,
                      uint32_t site1, uint32_t site2, void* stream);

/* out[r, :] = drop_pe(drop_emb(table[ids[r], :]) + pe[r % period, :]): the inplace dropout on the word embeddings
 * (newsEncoders.py:311-312) and PositionalEncoding's dropout (:827) in one pass; element index r * dim + c for both sites. */
int lime_embed_pe_dropout_f32(const int32_t* ids, const float* table, int64_t ld_table, const float* pe, int64_t ld_pe,
                              int32_t period, float* out, int64_t ldo, int64_t rows, int32_t dim, float p, uint64_t seed,
                              uint32_t site_emb, uint32_t site_pe, void* stream);

/* y = LayerNorm(res + drop(t)) per row (norm1(x + dropout1(sa(x))) / norm2(x + dropout2(ff(x))) of nn.TransformerEncoderLayer);
 * rstd (optional, [M]) as lime_linear_args.ln_rstd.  E <= 512. */
int lime_dropout_add_layernorm_f32(const float* t, int64_t ldt, const float* res, int64_t ldr, const float* gamma, const float* beta,
                                   float eps, float* y, int64_t ldy, float* rstd, int64_t M, int32_t E, float p, uint64_t seed,
                                   uint32_t site, void* stream);

/* dtable[ids[r], :] += dx[r, :] (nn.Embedding backward, newsEncoders.py:311-312).  dtable must be initialised by the
 * caller (zeros, or a gradient to add to).  Rows with ids[r] == hot_id (the padding word, pass -1 for none) are summed
 * per wave before they touch memory.  dim <= 512. */
int lime_embed_bwd_f32(const int32_t* ids, const float* dx, int64_t lddx, float* dtable, int64_t ld_table, int64_t rows,
                       int32_t dim, int32_t hot_id, void* stream);

/* The same for a table of at most 32 rows (FreshnessEncoder's two 10-row bucket tables, newsEncoders.py:75-76): per-column
 * LDS accumulation, no atomics, fixed summation order.  Rows whose id is outside [0, table_rows) are ignored. */
/* lime_embed_bwd_sorted_f32: the same sum WITHOUT atomics -- bitwise reproducible.  order: the token positions sorted by id with a
 * stable sort, sorted_ids = ids[order] (both int32 [rows]); every row of dtable that receives a contribution is written exactly
 * once, in a fixed association (runs of equal ids summed in sorted order, in chunks of 256 positions; partials of a run that
 * crosses chunks added in chunk order); rows without a contribution keep the caller's value -- zero dtable first.  dim <= 320.
 * workspace: lime_embed_bwd_sorted_workspace(rows, dim) floats. */
int lime_embed_bwd_sorted_f32(const int32_t* order, const int32_t* sorted_ids, const float* dx, int64_t lddx, float* dtable,
                              int64_t ld_table, int64_t rows, int32_t dim, float* workspace, int64_t workspace_floats, void* stream);
int64_t lime_embed_bwd_sorted_workspace(int64_t rows, int32_t dim);

int lime_embed_bwd_small_f32(const int32_t* ids, const float* dx, int64_t lddx, float* dtable, int64_t ld_table, int64_t rows,
                             int32_t dim, int32_t table_rows, void* stream);

/* out2[0] = ||g||_2 over the flat gradient buffer, out2[1] = min(1, max_norm / (out2[0] + 1e-6))  -- the coefficient of
 * torch.nn.utils.clip_grad_norm_ (trainer.py:146-147); max_norm <= 0: out2[1] = 1.  workspace >= 1024 floats. */
int lime_grad_clip_coef_f32(const float* g, int64_t n, float max_norm, float* out2, float* workspace, int64_t workspace_floats,
                            void* stream);

/* One torch.optim.Adam step (trainer.py:33,148; amsgrad off) over flat buffers, the gradient scaled by *grad_scale (device
 * scalar, e.g. out2 + 1 above; NULL = 1): step is the 1-based step count used for the bias corrections. */
int lime_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, const float* grad_scale, void* stream);

/* loss[0] = mean_b(-log_softmax(logits[b, :])[0]) (trainer.py:71-73); dlogits (optional) = its gradient [B, K] */
int lime_nll_softmax_f32(const float* logits, int64_t ld, int32_t B, int32_t K, float* loss, float* dlogits, int64_t ldd,
                         void* stream);

/* A linear classifier and its cross-entropy against an integer target in one launch (csrc/linear_xent_f32.hip): CROWN's category
 * predictor on the title intent vector (newsEncoders.py:358-364, :375-393; F.cross_entropy on a one-hot probability target).  Per row r
 * of x [M, D] (leading dimension ldx >= D: a column slice of a wider tensor), with w [C, D], b [C] (NULL: no bias), in fp32:
 *     z = x[r] w^T + b;   row_loss[r] = scale (logsumexp(z) - z[target[r]])   (max-subtracted);
 *     dlogits[r, :] = scale (softmax(z) - onehot(target[r]))   [M, C];   dx[r, :] = dlogits[r, :] w   [M, D], leading dimension lddx.
 * dlogits and dx are optional (NULL: not computed).  A target outside [0, C) is the all-zero one-hot row: its row_loss, dlogits and dx
 * are exact zeros and nothing is read at its index.  The scalar loss is the sum of row_loss (lime_colsum_f32 over [M, 1]: fixed order);
 * scale = weight / M gives the weighted mean.  M, D, C >= 1, ldx >= D, lddx >= D (LIME_ERR_BAD_ARG otherwise, as for a NULL x, w,
 * target or row_loss); C <= 1024 (LIME_ERR_UNSUPPORTED beyond), checked in that order before any launch.  A wave per row, w staged in LDS
 * while it fits 64 KB and read through L2 beyond; 16-byte accesses when D % 4 == 0 and x, w, dx and their leading dimensions are
 * 16-byte aligned.  Explicit fmaf, fixed-order sums, no atomics, no workspace: a row's bits depend on neither M, its place nor the run. */
int lime_linear_xent_f32(const float* x, int64_t ldx, const float* w, const float* b, const int32_t* target, float scale,
                         float* row_loss, float* dlogits, float* dx, int64_t lddx, int32_t M, int32_t D, int32_t C, void* stream);

/* ---- backward of the fused tail kernels (csrc/tail_backward_f32.hip) -------------------------------------------------- */

/* Backward of lime_intent_fuse_f32 (newsEncoders.py:355-371: intent attention over the k intents of title and body, cosine
 * similarity, concat): dcontent [M, ldc] holds the gradient of content[:, 0:2D]; writes d_intents [2 M k, D], d_hidden
 * [2 M k, A] and the two affine2 gradients [A] (summed over the news in a fixed order through `workspace`,
 * lime_intent_fuse_bwd_workspace(M, A) floats). */
int64_t lime_intent_fuse_bwd_workspace(int64_t M, int32_t A);
int lime_intent_fuse_bwd_f32(const float* intents, const float* hidden, const float* aff2_title, const float* aff2_body,
                             const float* dcontent, int64_t ldc, float* d_intents, float* d_hidden, float* d_aff2_title,
                             float* d_aff2_body, int64_t M, int32_t k, int32_t D, int32_t A, float* workspace,
                             int64_t workspace_floats, void* stream);

/* Backward of lime_gate_ln_f32 (layers.py:84-89): out = LayerNorm(g s x + (1 - g) x), g = sigmoid(s y + bias), s = scale[row].
 * Writes dy, dx [rows, D] (dx: the direct path only; y = W_g x is the caller's GEMM), dscale [rows], dbias / dgamma / dbeta
 * [D].  workspace: lime_gate_ln_bwd_workspace(rows, D) floats. */
int64_t lime_gate_ln_bwd_workspace(int64_t rows, int32_t D);
int lime_gate_ln_bwd_f32(const float* y, const float* x, const float* scale, const float* bias, const float* gamma, const float* beta,
                         float eps, const float* dout, float* dy, float* dx, float* dscale, float* dbias, float* dgamma,
                         float* dbeta, int64_t rows, int32_t D, float* workspace, int64_t workspace_floats, void* stream);

/* Backward of lime_interest_match_f32 (userEncoders.py:158-169 + util.py:23-49) from dlogits [B, N]: dkp [B, H, A], dqp
 * [B, N, A], dg [B, H, D], dcand [B, N, D] (the lifetime weight is a constant of the parameters).  workspace:
 * lime_interest_match_bwd_workspace(B, N, H, A, D) floats (per-candidate shares of dkp / dg, summed over n in order). */
int64_t lime_interest_match_bwd_workspace(int32_t B, int32_t N, int32_t H, int32_t A, int32_t D);
int lime_interest_match_bwd_f32(const float* kp, const float* qp, const float* g, const float* cand, const float* remaining,
                                const float* dlogits, float* dkp, float* dqp, float* dg, float* dcand, int32_t B, int32_t N,
                                int32_t H, int32_t A, int32_t D, float scale, float alpha, float beta, int32_t use_weight,
                                int32_t use_penalty, float* workspace, int64_t workspace_floats, void* stream);

/* Candidate-aware attention weights (layers.py:66-81) in training mode: as lime_cand_attn_weights_f32 with the dropout of
 * layers.py:74 on the per-head probabilities (mask element ((b * n_head + h) * N + n) * H + j; dropout_p = 0: none), and its
 * backward from dagg [B, H] to dqp [B, N, D] / dkp [B, H, D] (the same dropout_p / seed / site regenerate the mask).
 * N <= 16, H <= 256; Q, K and the probabilities of one impression row live in LDS. */
int lime_cand_attn_weights_train_f32(const float* qp, const float* kp, const uint8_t* mask, float* agg, int32_t B, int32_t N, int32_t H,
                                     int32_t D, int32_t n_head, float dropout_p, uint64_t seed, uint32_t site, void* stream);
int lime_cand_attn_weights_bwd_f32(const float* qp, const float* kp, const uint8_t* mask, const float* dagg, float* dqp, float* dkp,
                                   int32_t B, int32_t N, int32_t H, int32_t D, int32_t n_head, float dropout_p, uint64_t seed,
                                   uint32_t site, void* stream);

/* =====================================================================================================
 * 1-D convolution over the tokens of a sequence (layers.py:98-135 Conv1D, the CNN content encoder newsEncoders.py:535-563) as a
 * GEMM over a gathered window (csrc/conv_sp_f32.hip; split product, or exact-fp32 MFMA under lime_set_split_gemm(0)):
 *   out[r, o] = (accumulate ? out[r, o] : 0) + act(bias[o] + sum_{j < window} sum_{c < C} A(r, j)[c] * w[o * ldw + j * C + c])
 *   row r = token t = r % T of sequence r / T; A(r, j) = source row r + j - pad (pad = (window - 1) / 2), ZEROS when t + j - pad is
 *   outside [0, T); source row q = a[ids[q] * lda ...] (a gathered table row) or a[q * lda ...] (ids == NULL).
 * w is the nn.Conv1d weight permuted to [N, window, C].  window odd; C, lda, ldw multiples of 4, a and w 16-byte aligned; M % T == 0;
 * act NONE or RELU; bias optional; m_dev: optional device row count (rows >= min(*m_dev, M) are left untouched).  The data gradient
 * is this call with the dense dY as A and the taps reversed in w ([C, window, N], w[c, j, o] = W[o, c, window - 1 - j]). */
int lime_conv1d_window_f32(const float* a, int64_t lda, const int32_t* ids, const float* w, int64_t ldw, const float* bias,
                           float* out, int64_t ldc, int32_t M, int32_t N, int32_t C, int32_t T, int32_t window, int32_t act,
                           int32_t accumulate, const int32_t* m_dev, void* stream);

/* dw[o, j * C + c] (+)= sum_r dy[r, o] * A(r, j)[c] with the windowed operand of lime_conv1d_window_f32 (dw [N, window * C]).  Rows are
 * split over workgroups, partial tiles in `workspace` (lime_conv1d_wgrad_workspace floats) summed in split order: bitwise
 * reproducible.  N, C, ldy, lda multiples of 4; dy, a, workspace 16-byte aligned. */
int64_t lime_conv1d_wgrad_workspace(int32_t M, int32_t N, int32_t C, int32_t window);
int lime_conv1d_wgrad_f32(const float* dy, int64_t ldy, const float* a, int64_t lda, const int32_t* ids, float* dw, int64_t lddw,
                          int32_t M, int32_t N, int32_t C, int32_t T, int32_t window, int32_t accumulate, float* workspace,
                          int64_t workspace_floats, void* stream);

/* =====================================================================================================
 * Knowledge-aware convolution + ReLU + max pool in one launch (layers.py:138-190 Conv2D_Pool, the KCNN content encoder
 * newsEncoders.py:598-638; csrc/conv_pool_sp_f32.hip: split product, or exact-fp32 MFMA under lime_set_split_gemm(0)):
 *   pre[s, t, o] = bias[o] + sum_{src < n_src} sum_{j < window} sum_{c < C} X_src(s T + t + j - pad)[c] * w[o * ldw + (src * window + j) * C + c]
 *   pooled[s * ldp + o] = max(0, max_{t < P} pre[s, t, o]);  arg[s * ldarg + o] = the smallest t attaining it, -1 where pooled is 0
 *   X_src(q) = a[src][ids[src][q] * lda[src] ...] (a gathered table row) or a[src][q * lda[src] ...] (ids[src] == NULL); ZEROS where
 *   the position t + j - pad is outside [0, T).
 * w is the nn.Conv2d weight [N, C, window, n_src] permuted to [N, n_src, window, C].  1 <= n_src <= 3, 1 <= window <= T, 0 <= pad <
 * window, 1 <= P <= T <= 128 (a 128-row tile holds floor(128 / T) whole sequences).  C, N, lda[], ldw multiples of 4; a[], w, bias
 * 16-byte aligned; anything else is refused before any launch.  bias and arg are optional.  n_seq_dev: optional device-side sequence
 * count (sequences >= min(*n_seq_dev, n_seq) are neither computed nor written).  No atomics; the pre-activations stay in the
 * workgroup; the bits of a (sequence, column) do not depend on the batch around the sequence. */
typedef struct lime_conv_pool_args {
    const float* a[3];
    int64_t lda[3];
    const int32_t* ids[3];
    const float* w;
    int64_t ldw;
    const float* bias;
    float* pooled;
    int64_t ldp;
    int32_t* arg;
    int64_t ldarg;
    const int32_t* n_seq_dev;
    int32_t n_seq, T, N, C;
    int32_t n_src, window, pad, P;
} lime_conv_pool_args;
int lime_conv_pool_f32(const lime_conv_pool_args* args, void* stream);

/* The same pooled / arg from dense pre-activations pre[(s T + t) * ldpre + o] (+ bias): one thread per (sequence, four columns).
 * N, ldpre, ldp multiples of 4; pre, pooled, bias 16-byte aligned. */
int lime_relu_maxpool_f32(const float* pre, int64_t ldpre, const float* bias, float* pooled, int64_t ldp, int32_t* arg, int64_t ldarg,
                          int32_t n_seq, int32_t T, int32_t P, int32_t N, const int32_t* n_seq_dev, void* stream);

/* Backward of the pooling: dpre[(s T + t) * ldpre + o] = (arg[s, o] == t) ? dpooled[s, o] : 0 for every t < T -- all n_seq * T rows are
 * written, each by the one thread that owns its (sequence, four columns) strip: no atomics, no pre-zeroing. */
int lime_relu_maxpool_bwd_f32(const float* dpooled, int64_t lddp, const int32_t* arg, int64_t ldarg, float* dpre, int64_t ldpre,
                              int32_t n_seq, int32_t T, int32_t N, void* stream);

/* =====================================================================================================
 * Additive attention pool in one launch (layers.py:285-300 Attention, the NAML content encoder newsEncoders.py:686-694;
 * csrc/attn_pool_sp_f32.hip: split product, or exact-fp32 MFMA under lime_set_split_gemm(0)):
 *   out[s * ldo + :D] = sum_t alpha[s, t] x[(s T + t) * ldx + :D],  alpha[s] = softmax_t(w2 . tanh(W1 x[s T + t] + b1))
 *   score of a key with mask[s T + t] == 0: -1e9 (mask optional, u8 [n_seq * T]).
 * The [rows, A] hidden state never leaves registers.  A tile of 128 rows holds floor(128 / T) whole sequences: a sequence's output
 * has the same bits in any tile slot and for any n_seq.  w1p: W1 [A, D] as lime_attn_pool_pack_sp lays it out (opaque; repack after
 * every change of W1).  b1 [A] (may be NULL: zeros), w2 [A].  T <= 128, D % 4 == 0, D <= 16384, A <= 512; x, out 16-byte aligned,
 * ldx, ldo multiples of 4.  n_seq_dev: optional device sequence count (sequences >= min(*n_seq_dev, n_seq) are neither read nor
 * written). */
int64_t lime_attn_pool_pack_sp_size(int32_t D, int32_t A);
int lime_attn_pool_pack_sp(const float* w1, int64_t ldw1, int32_t D, int32_t A, uint16_t* w1p, void* stream);
int lime_attn_pool_sp_f32(const float* x, int64_t ldx, int32_t D, const uint16_t* w1p, const float* b1, const float* w2, int32_t A,
                          const uint8_t* mask, float* out, int64_t ldo, int32_t n_seq, int32_t T, const int32_t* n_seq_dev, void* stream);

/* =====================================================================================================
 * Tail of the pooled user encoders in one launch (userEncoders ATT / MHSA; csrc/user_pool_match_f32.hip): additive attention pool
 * over the history (layers.py:288-299, behind the affine1 + tanh GEMM), dot product with every candidate, remaining-lifetime weight
 * (util.py:23-49, the rule of lime_interest_match_f32 / lime_lifetime_score_f32):
 *   a[h] = hidden[(b H + h) * ldh + :A] . w2   (-1e9 where mask[b H + h] == 0);   alpha = softmax_h(a)
 *   u[b, :] = sum_h alpha[h] x[(b H + h) * ldx + :D]                               -> user_rep [B, D] (may be NULL)
 *   logits[b, n] = (u[b, :] . cand[b, n, :]) * w(remaining[b, n])                  -> logits [B, N]  (may be NULL; not both)
 * mask: optional u8 [B, H].  cand [B, N, D] and remaining [B, N] (use_weight) are read only when logits is given.
 * H <= 512, D <= 2048, D % 4 == 0, ldx % 4 == 0; x, cand, user_rep 16-byte aligned (LIME_ERR_BAD_ARG otherwise); hidden / w2 are read
 * 16 bytes at a time when A % 4 == 0, ldh % 4 == 0 and both are aligned, element by element otherwise.  A workgroup per row below
 * B = 2048, a wave per row (four rows a workgroup) from there on; a row's bits are the same in both forms, for any B and N. */
int lime_pool_match_f32(const float* hidden, int64_t ldh, const float* w2, const float* x, int64_t ldx, const uint8_t* mask,
                        const float* cand, const float* remaining, float alpha_s, float beta_s, int32_t use_weight,
                        int32_t use_penalty, float* user_rep, float* logits, int32_t B, int32_t N, int32_t H, int32_t A, int32_t D,
                        void* stream);

/* =====================================================================================================
 * The occurrence side of the per-news content cache in one launch (LIME.encode_cached; csrc/cached_occurrence_f32.hip).  A news
 * occurs in many impressions, each time with its own freshness and lifetime; FreshnessEncoder's output
 * tanh(dense(cat(E_f[b_f], E_l[b_l]))) (newsEncoders.py:60-83) takes only nb^2 values (nb = num_buckets), so the caller keeps
 * them -- and everything linear behind them -- as tables of nb^2 rows, row b_f * nb + b_l.  For every occurrence r < R:
 *     pair = bucket(freshness[r]) * nb + bucket(lifetime[r])               (the rule of lime_bucketize_f32 / _cuts_f32; NaN -> 0)
 *     LIME_OCC_CONCAT, LIME_OCC_ADD : out[r, :] = A[idx[r], :] + T[pair, :]
 *     LIME_OCC_GATED                : g = sigmoid(P[idx[r], :] + Q[pair, :]);  out[r, :] = fma(g, A[idx[r], :], (1 - g) * T[pair, :])
 * with, per fusion method of newsEncoders.py:111-126, :151-159 (c = content width, F = the nb^2 freshness representations):
 *     concat + project : A = content . W_p[:, :c]^T  [n, D],  T = F . W_p[:, c:]^T + b_p     (P, Q ignored; D = lime_output_dim)
 *     add              : A = content                 [n, D],  T = F                          (P, Q ignored; D = c)
 *     gated            : A = content, P = content . W_g[:, :c]^T,  T = F,  Q = F . W_g[:, c:]^T + b_g            (D = c)
 * A, P, T, Q and out are row-strided (lda .. ldo, in floats), so A and P may be column views of one cache tensor.
 * idx int32 [R]: every id must be in [0, n) -- unchecked, as in lime_gather_rows_f32.  cuts: NULL for num_buckets = 10 (the
 * built-in table of lime_bucketize_f32; n_cuts is ignored) or the n_cuts = nb - 1 ascending device cut points of
 * lime_bucketize_cuts_f32.  n_pairs: the row count of T (and Q), which must equal nb^2 (LIME_ERR_BAD_ARG otherwise: a bucket pair can
 * then never point behind the tables).  D % 4 == 0, every base pointer 16-byte aligned and every row stride a multiple of 4
 * (LIME_ERR_BAD_ARG otherwise); 16-byte loads and stores throughout, no LDS, no atomics.  Every output element is one fixed
 * expression of its own operands: a row's bits depend neither on R nor on its position. */
enum { LIME_OCC_CONCAT = 0, LIME_OCC_ADD = 1, LIME_OCC_GATED = 2 };
int lime_cached_occurrence_f32(int32_t mode, const int32_t* idx, const float* freshness, const float* lifetime, const float* cuts,
                               int32_t n_cuts, const float* A, int64_t lda, const float* P, int64_t ldp, const float* T, int64_t ldt,
                               const float* Q, int64_t ldq, int64_t n_pairs, float* out, int64_t ldo, int64_t R, int32_t D,
                               void* stream);

/* =====================================================================================================
 * The dev / test pass behind the scores in one call (util.py:113-123 rank rule + evaluate.py:32-89 metrics;
 * csrc/rank_metrics.hip): per impression the 1-based rank of every candidate row under a stable descending order
 *     rank_i = 1 + #{j in the impression : s_j > s_i or (s_j == s_i and j < i)}       (+0.0 ties with -0.0)
 * and, from the ranks q of its P positives among n rows (N = n - P; ahead_pos = positives ranked ahead of the row),
 *     AUC    = (P N - sum_pos (q - 1 - ahead_pos)) / (P N)
 *     MRR    = (sum_pos 1 / q) / P
 *     nDCG@k = (sum_pos, q <= k  disc[q - 1]) / (sum_{p < min(k, P)} disc[p])          k = 5, 10
 * -- what evaluate.scoring computes from the rank file, which feeds 1 / rank into every metric.
 *   scores fp32 [R], labels u8 [R] (0 / 1), offsets int32 [n_imp + 1] (rows offsets[i] .. offsets[i + 1] - 1 belong to impression i;
 *   non-decreasing, offsets[n_imp] == R: the caller checks that, the kernel clamps every offset into [0, R]), skip u8 [n_imp] or
 *   NULL (non-zero: the impression's truth line has no labels; it is ranked but not counted), disc fp64 [10] = 1 / log2(p + 2).
 *   ranks int32 [R]; per_imp fp64 [n_imp, 4] = AUC, MRR, nDCG@5, nDCG@10 (zeros unless status is 0);
 *   status int32 [n_imp]: 0 counted, 1 skipped or no rows, 2 one class only, 3 a label outside {0, 1} or a NaN score (checked in
 *   that order; the ranks of a status-3 impression follow the counting rule under IEEE comparisons);
 *   sums fp64 [4] and count int64 [1]: over the status == 0 impressions (their means are the split's metrics; a sharded pass
 *   all-reduces these five numbers).
 * A wave per impression up to 512 rows, a workgroup above (any length).  Bitwise reproducible and independent of the grids: fixed
 * summation orders, no atomics.  rank_blocks / reduce_blocks: workgroups of the rank launch and of the first reduction level, 0 = the
 * default (tests and A/B runs).  workspace: lime_rank_metrics_workspace(n_imp) bytes, 8-byte aligned; per_imp 16-byte aligned. */
typedef struct {
    const float* scores;
    const uint8_t* labels;
    const int32_t* offsets;
    const uint8_t* skip;
    const double* disc;
    int32_t* ranks;
    double* per_imp;
    int32_t* status;
    double* sums;
    int64_t* count;
    void* workspace;      int64_t workspace_bytes;
    int64_t R;
    int32_t n_imp;
    int32_t rank_blocks;
    int32_t reduce_blocks;
    int32_t reserved;     /* must be 0 */
} lime_rank_metrics_args;

int64_t lime_rank_metrics_workspace(int32_t n_imp);
int lime_rank_metrics(const lime_rank_metrics_args* args, void* stream);

/* =====================================================================================================
 * What recommended slates are worth (util.evaluate_slates_on_device; recommend.slate_metrics states the rule on the host;
 * csrc/slate_metrics.hip).  R slates of k slots: slot j < k of slate r is positions[r ldp + j] (int32 [R, ldp], k <= ldp: a prefix of
 * a wider slate is evaluated in place).  With offsets int64 [R + 1] a position counts inside the slate's OWN list -- rows offsets[r] ..
 * offsets[r + 1] - 1 of the [P] arrays, the impression's rows (every offset is clamped into [0, P]) --, without it inside ONE pool of P
 * rows that all slates share.  news int32 [P]: the news id of a row, the row of table fp32 [n, E] (leading dimension ld) and of keys
 * int32 [n] (0 <= key < n_keys; a key outside is no key).  labels u8 [P] (needs offsets), skip u8 [R], value fp32 [P], table and keys
 * may each be NULL.  disc fp64 [k] = 1 / log2(p + 2).
 *   A slot is FILLED when its position lies inside the list (the pool) and the news id behind it inside [0, n); every other slot
 *   (-1 is the usual one) is empty: it earns nothing, nothing is read for it, and it still occupies its slot.
 *   status int32 [R], lime_rank_metrics' rule in its order: 1 skipped, no labels or no rows; 3 a label outside {0, 1} among the
 *   impression's rows; 2 one class only among them; 0 counted.  Ppos: the positives among the impression's rows.
 *   per_slate fp64 [R, 8]:
 *     0  nDCG@k   = (sum over the filled slots j with label 1 of disc[j]) / (sum_{p < min(k, Ppos)} disc[p])     } zeros unless
 *     1  RR@k     = 1 / (1 + the first slot that holds a positive), 0 without one                                 } status is 0
 *     2  hit@k    = 1 with a positive in a filled slot, else 0                                                    }
 *     3  recall@k = the positives in filled slots / Ppos                                                          }
 *     4  ILD      = 1 - mean over the pairs a < b of filled slots of cos(table[news_a], table[news_b]); cos is 0 when either norm
 *                   is 0 (lime_mmr_rows_f32's rule); inverse norms and dot products fp32 in a fixed order, the pair sum fp64 in a
 *                   fixed order; 0 with fewer than two filled slots or without a table
 *     5  the distinct keys among the filled slots (0 without keys)
 *     6  the filled slots
 *     7  the mean of value over the filled slots, summed in fp64 in slot order (0 without value or without a filled slot)
 *   sums fp64 [8], counts int64 [3]: counts[0] the slates with status 0 -- columns 0-3 are summed over them --, counts[1] the slates
 *   with skip unset and >= 2 filled slots -- column 4 --, counts[2] those with skip unset and >= 1 filled slot -- columns 5-7.
 * A wave per slate up to k = 16, a workgroup above (any R); the sums are a second launch over per_slate / status, one workgroup per output adding all slates in
 * a fixed order and carrying the additions' rounding errors along (a sum is its terms' exact sum rounded once, whatever R): no
 * atomics, no workspace, and reduce_blocks (workgroups of that launch, 0 = one per output) never changes a bit.
 * Bitwise reproducible; a slate's row depends on its own operands alone, not on R, its place in the batch or the grid.
 * Statuses before any launch, in this order: LIME_ERR_BAD_ARG for a NULL args / positions / news / disc / per_slate / status / sums /
 * counts; for labels without offsets; for R < 0, P < 0, k < 1, k > ldp, E < 0, ld < E, n < 1; for a table with E < 1 or keys with
 * n_keys < 1; for reserved != 0 or reduce_blocks < 0; LIME_ERR_UNSUPPORTED for k > 128 or E % 4 != 0.  R == 0 is a success without a
 * launch that leaves zero sums and counts. */
typedef struct {
    const int32_t* positions;
    const int64_t* offsets;
    const int32_t* news;
    const uint8_t* labels;
    const uint8_t* skip;
    const float* value;
    const float* table;
    const int32_t* keys;
    const double* disc;
    double* per_slate;
    int32_t* status;
    double* sums;
    int64_t* counts;
    int64_t R;
    int64_t P;
    int64_t ldp;
    int64_t ld;
    int64_t n;
    int32_t k;
    int32_t E;
    int32_t n_keys;
    int32_t reduce_blocks;
    int32_t reserved;     /* must be 0 */
} lime_slate_metrics_args;

int lime_slate_metrics_f32(const lime_slate_metrics_args* args, void* stream);

/* =====================================================================================================
 * The epoch's negative sampling on the device (Train_Dataset.negative_sampling, dataset.py:42-77; csrc/negative_sample.hip).  The
 * non-clicked news of the N train records are resident as CSR: offsets int64 [N + 1] (record i owns entries offsets[i] ..
 * offsets[i + 1] - 1; every offset is clamped into [0, nnz] by the kernel), neg_index int32 [nnz], neg_lifetime fp32 [nnz]; per
 * record pos_index int32 [N], pos_lifetime fp32 [N], freshness fp32 [N].  Written in full, row i of [N, 1 + K] each:
 *     cand_index     = [pos_index[i],    neg_index[lo + k_0],    ..., neg_index[lo + k_{K-1}]]            lo = offsets[i]
 *     cand_freshness = [freshness[i], ... repeated]
 *     cand_lifetime  = [pos_lifetime[i], neg_lifetime[lo + k_0], ..., neg_lifetime[lo + k_{K-1}]]
 * with, for n = offsets[i + 1] - offsets[i] non-clicked news:
 *     n <= K : k_j = j % n
 *     n >  K : K distinct values, uniform over [0, m), m = n - 1 (inclusive == 0: the reference's randint excludes its upper bound, so
 *              the last non-clicked news is never drawn) or m = n (inclusive != 0), by a partial Fisher-Yates: with
 *              u = hi32(splitmix64(key(seed, epoch) + 16 i + j)) -- the generator and key mixing of csrc/dropout.h with site = epoch --
 *              slot j takes the value at position r = (u * (m - j)) >> 32 of the m - j still free, and the last free value moves to r.
 *              The multiply-shift is within (m - j) / 2^32 (relative) of uniform.
 *     n == 0 : the row repeats its positive (the reference divides by zero; the host layers refuse such a record before any launch).
 * Row i is a function of (seed, epoch, i) and the record alone.  1 <= K <= LIME_NEG_MAX_K, 0 <= nnz < 2^31 and non-NULL pointers, or
 * LIME_ERR_BAD_ARG before any launch.  One thread per record; no LDS, no atomics, no allocation, no synchronise. */
#define LIME_NEG_MAX_K 16
int lime_negative_sample(const int64_t* offsets, const int32_t* neg_index, const float* neg_lifetime, int64_t nnz,
                         const int32_t* pos_index, const float* pos_lifetime, const float* freshness, int32_t* cand_index,
                         float* cand_freshness, float* cand_lifetime, int64_t N, int32_t K, uint64_t seed, uint32_t epoch,
                         int32_t inclusive, void* stream);

/* =====================================================================================================
 * One time step of a bidirectional single-layer LSTM (csrc/lstm_f32.hip): the recurrence of the CNE content encoder
 * (newsEncoders.py:439-532: nn.LSTM(bidirectional=True) under pack_padded_sequence).  nn.LSTM's cell and parameter layout as stored:
 * gate order i, f, g, o; whh = [weight_hh_l0; weight_hh_l0_reverse], [2, 4h, h].  R sequences of T token slots, sequence r runs over
 * its FIRST len[r] slots (len is clamped into [0, T]).
 *   gi [R T, >= 2 . 4h] (leading dimension ldgi): x_t W_ih^T + b_ih + b_hh of every token, forward gates in columns [0, 4h), backward
 *   in [4h, 8h) -- one lime_linear_f32 launch over the two W_ih stacked row-wise, ahead of the time loop.
 * Step `step` (the caller launches step = 0 .. T - 1 in order on one stream), both directions in one launch: sequence r is active iff
 * step < len[r]; forward works on token t = step, backward on token t = len[r] - 1 - step:
 *     pre   = gi[r T + t, direction] + W_hh h_prev         h_prev = hout[r T + t - 1, :h] (forward) / hout[r T + t + 1, h:] (backward),
 *                                                            zero at step 0 (nothing is read then, neither hout nor c)
 *     i, f, o = sigmoid(pre_i, pre_f, pre_o), g = tanh(pre_g);   c' = f c + i g;   hout[r T + t, direction] = o tanh(c')
 *   c [2, R, h] is updated in place (after step T - 1 it is c_n of both directions; h_n is hout at token len - 1 / token 0).
 *   Inactive sequences are left untouched; the caller zeroes hout once, so the rows behind a length stay zero (pad_packed_sequence).
 *   n_rows_dev (optional DEVICE int): only the first min(*n_rows_dev, R) sequences are worked on (R stays the capacity: c's stride).
 *   gates [R T, 2 . 4h], c_seq [R T, 2h], h_prev [R T, 2h] (all three or none): what lime_lstm_step_bwd_f32 needs -- the four gate
 *   activations, c_t and the h_{t-1} the step read (zero for a direction's first token: NOT hout shifted by one row).
 * h must be a multiple of 16 (a workgroup owns 64 sequences x 16 units with all four gates; v_mfma_f32_16x16x4_f32), every pointer
 * 16-byte aligned.  A (sequence, unit) result is a fixed-order sum: its bits do not depend on R, the sequence's position, n_rows_dev.
 *
 * lime_lstm_step_bwd_f32: the gate gradients of step `step` (the caller runs step = T - 1 .. 0).  dh [2, R, h] is the gradient carried
 * through W_hh (zeros at the start), dc [2, R, h] the cell carry (d c_n at the start, updated in place); dhout [R T, lddh >= 2h] (or
 * NULL) is added at the step that produced the row.  Writes the pre-activation gradients to dgi [R T, 2 . 4h] (layout of gi, dense)
 * and to dgs [2, R, 4h] (this step's rows, zeros for inactive sequences); the next carry is dh[d] = dgs[d] . W_hh[d], one
 * lime_linear_group_f32 launch by the caller.  Inactive sequences keep their dc; their dh stays zero.
 *
 * lime_mask_lengths: len[r] = max(#non-zero bytes of mask[r, :T], min_len).
 *
 * lime_gate_mul_f32 (dense [rows, cols] fp32, cols a multiple of 4; min(*n_rows_dev, rows) rows when n_rows_dev is given):
 *   mode 0: out = x * sigmoid(g) (out == g allowed) -- CNE's cross-selective gate applied to the LSTM output (newsEncoders.py:517-521)
 *   mode 1: out[r] = x[r] * g[r / div] * scale -- the scaled-dot-product scores of :527-528 as the summands h_t (K^T q) / sqrt(A),
 *                                                 which lime_additive_pool_f32 sums (affine2 = ones), masks, soft-maxes and pools. */
int lime_lstm_step_f32(const float* gi, int64_t ldgi, const float* whh, const int32_t* len, float* hout, float* c, float* gates,
                       float* c_seq, float* h_prev, int32_t R, int32_t T, int32_t h, int32_t step, const int32_t* n_rows_dev,
                       void* stream);
int lime_lstm_step_bwd_f32(const float* dhout, int64_t lddh, const float* gates, const float* c_seq, const int32_t* len,
                           const float* dh, float* dc, float* dgi, float* dgs, int32_t R, int32_t T, int32_t h, int32_t step,
                           void* stream);
int lime_mask_lengths(const uint8_t* mask, int32_t R, int32_t T, int32_t min_len, int32_t* len, void* stream);
int lime_gate_mul_f32(const float* x, const float* g, float* out, int64_t rows, int32_t cols, int32_t div, int32_t mode, float scale,
                      const int32_t* n_rows_dev, void* stream);

/* =====================================================================================================
 * CNE's per-news recurrence cache (csrc/seq_cache_f32.hip; newsEncoders.CNERecurrenceCache).  The LSTM output h_t of a text and the
 * hidden-state half of its gate pre-activation, H h_t (newsEncoders.py:517-518), depend on the news alone: the cache keeps both for the
 * live tokens only, PACKED -- news i owns the rows offsets[i] .. offsets[i] + lens[i] - 1 of [sum(lens), C] tensors (C = 2 hidden_dim),
 * token slots 0 .. lens[i] - 1 in order; offsets int64 [n + 1] is the exclusive prefix sum of lens int32 [n].
 *
 * lime_seq_pack_f32: dst[offsets[i] + t, :] = src[i S + t, :] for t < min(lens[i], S), i < n -- a dense [n S, C] chunk into the packed
 * rows.  offsets holds DESTINATION rows (of dst as passed); no other row of dst is written.
 *
 * lime_cne_gate_cached_f32: the cross-selective gate of a batch from the cache, one launch.  For batch slot r < min(*n_rows_dev, cap)
 * (n_rows_dev NULL: cap) and token slot t < S, with j = idx[r] (int32 news index into the cache; every id must be in [0, n) --
 * unchecked, as in lime_gather_rows_f32):
 *     out[r S + t, :] = t < lens[j] ?  h[offsets[j] + t, :] * sigmoid(hh[offsets[j] + t, :] + tm[r, :])  :  0
 * tm [cap, C] is the partner's memory term M m_partner + b per slot.  Rows behind a length are written as zeros (the attention GEMM
 * behind the gate reads all cap S rows); rows of slots >= *n_rows_dev are not touched.
 *
 * Both: C % 4 == 0, S >= 1, n / cap >= 0 (0: LIME_OK without a launch), src / dst / h / hh / tm / out 16-byte aligned
 * (LIME_ERR_BAD_ARG otherwise); 16-byte loads and stores, 64-bit row offsets, no LDS, no atomics.  Every output element is one fixed
 * expression of its own operands: a row's bits depend neither on its slot nor on n_rows_dev. */
int lime_seq_pack_f32(const float* src, const int32_t* lens, const int64_t* offsets, float* dst, int32_t n, int32_t S, int32_t C,
                      void* stream);
int lime_cne_gate_cached_f32(const float* h, const float* hh, const int64_t* offsets, const int32_t* lens, const int32_t* idx,
                             const float* tm, float* out, int32_t cap, int32_t S, int32_t C, const int32_t* n_rows_dev, void* stream);

/* =====================================================================================================
 * Pool recommendation (Model.score_pool / Model.recommend).
 *
 * lime_grouped_match_f32 (csrc/grouped_match_f32.hip): the function of lime_interest_match_f32 for GROUPS of pairs that share one
 * refined history -- a group is one (user, candidate topic), its pairs are the pool's news of that topic.  kp [G H, A] and g [G H, D]
 * per group; qp [P, A], cand [P, D], remaining [P] (read when use_weight != 0) per pair; offsets int64 [G + 1] on the device: the pairs
 * of group i are rows offsets[i] .. offsets[i + 1] - 1 (every offset is clamped into [0, P] by the kernel; pairs outside every group
 * are not written).  For pair p of group i:
 *     s[h] = kp[i H + h, :] . qp[p, :] * scale,  alpha = softmax_h(s),  logits[p] = (sum_h alpha[h] (g[i H + h, :] . cand[p, :])) * w(remaining[p])
 * with w the weight of lime_interest_match_f32 (alpha_s, beta_s, use_weight, use_penalty).  Exact fp32 on v_mfma_f32_16x16x4_f32, a
 * workgroup per 64-pair tile of a group; fixed-order sums, no atomics: a pair's bits depend neither on P, G, the group's position nor
 * the pair's place in its tile.  1 <= H <= 128, A and D multiples of 4 up to 2048 (LIME_ERR_UNSUPPORTED otherwise); kp, g, qp, cand
 * 16-byte aligned (LIME_ERR_BAD_ARG otherwise).  H = 1 is the match of one pooled user vector g[i] per group (alpha = 1).
 *
 * lime_grouped_match_indexed_f32 (same file): the same function with the pairs' own operands read through an index -- qp [n, A] and
 * cand [n, D] are TABLES of n rows and pair p reads row index[p] of both (index int32 [P] on the device); remaining, offsets and
 * logits stay per pair.  For a model whose candidate representation depends on the news alone (no LIME: Model._match_pass) the tables
 * are the pool's rows or the news cache itself, and no [P, D] copy of them exists.  A pair's bits equal those of
 * lime_grouped_match_f32 on the gathered rows qp[index], cand[index].  An index outside [0, n) is CLAMPED into it by the kernel (as
 * the offsets are): a bad plan reads in range and gives the result of the row it was clamped to.  n = 0 with P > 0 is
 * LIME_ERR_BAD_ARG; n < 2^31 (LIME_ERR_UNSUPPORTED beyond); the other limits and statuses are those of lime_grouped_match_f32, checked
 * in the same order before any launch.
 *
 * lime_grouped_mlp_match_f32 (csrc/grouped_mlp_match_f32.hip): the grouped match under the MLP click predictor (config.click_predictor =
 * 'mlp', reference model.py:113-115, :182-184: logits = out(relu(mlp(cat[user, news])))), with mlp.weight [Dh, 2 D] split into its
 * user half W_u = mlp.weight[:, :D] and its news half W_n = mlp.weight[:, D:].  kp [G H, A] and gu = g W_u^T [G H, Dh] per group; qp
 * [P, A] and nw = cand W_n^T + mlp.bias [P, Dh] per pair; w_out [Dh] = out.weight, b_out = out.bias, ONE float on the device (NULL:
 * 0); offsets as in lime_grouped_match_f32.  For pair p of group i:
 *     s[h] = kp[i H + h, :] . qp[p, :] * scale,  a = softmax_h(s),  u[j] = sum_h a[h] gu[i H + h, j],
 *     logits[p] = sum_j relu(u[j] + nw[p, j]) w_out[j] + b_out
 * There is no remaining-lifetime weight under this predictor.  The pooled hidden row u exists in registers alone: no [P, D] user row
 * and no [P, Dh] hidden row is written.  Exact fp32 on v_mfma_f32_16x16x4_f32, a workgroup per 64-pair tile of a group; the first
 * product and the softmax are the instructions of lime_grouped_match_f32; fixed-order sums, no atomics: a pair's bits depend on H, A
 * and Dh alone -- not on P, G, the group's position or the pair's place in its tile.  1 <= H <= 128, A a multiple of 4 up to 2048, Dh
 * any EVEN number up to 2048 (LIME_ERR_UNSUPPORTED otherwise); kp, qp 16-byte aligned, gu, nw 8-byte aligned (LIME_ERR_BAD_ARG
 * otherwise).  H = 1 is the predictor on one pooled user vector per group (a = 1; kp and qp are not felt).
 *
 * lime_grouped_mlp_match_indexed_f32 (same file): qp [n, A] and nw [n, Dh] are TABLES of n rows and pair p reads row index[p] of both
 * (index int32 [P] on the device).  A pair's bits equal those of lime_grouped_mlp_match_f32 on the gathered rows.  The clamping of an
 * index outside [0, n), n = 0 with P > 0 (LIME_ERR_BAD_ARG) and n < 2^31 are the rules of lime_grouped_match_indexed_f32, checked in
 * the same order before any launch.
 *
 * lime_grouped_match_occurrence_f32 (csrc/grouped_match_f32.hip): the indexed form with each pair's own operands COMPOSED from a
 * news table and an occurrence table -- qa [n, A] and ca [n, D] read through index int32 [P], qt [n_occ, A] and ct [n_occ, D] read
 * through occ int32 [P] (both on the device):
 *     qp[p, :] = qa[index[p], :] + qt[occ[p], :],   cand[p, :] = ca[index[p], :] + ct[occ[p], :]
 * one fp32 add per element, a + t in that order, made while the operand is loaded.  A LIME candidate under 'add' or 'concat' +
 * project is A[news] + T[b_f nb + b_l] with everything behind it linear (Model._candidate_tables): no [P, D] row and no [P, A] Q row
 * exists.  A pair's bits equal those of lime_grouped_match_f32 on rows composed with that one fp32 add, and depend neither on P, G,
 * the group's position, the pair's place in its tile, n nor n_occ.  index is CLAMPED into [0, n) and occ into [0, n_occ) by the
 * kernel, as the offsets are.  LIME_ERR_BAD_ARG before any launch: a NULL index, occ or table, a table that is not 16-byte aligned,
 * n = 0 or n_occ = 0 with P > 0; n, n_occ < 2^31 and the dims of lime_grouped_match_f32 (LIME_ERR_UNSUPPORTED beyond), checked in the
 * order of lime_grouped_match_indexed_f32 with each occurrence check behind its indexed twin.  No LDS beyond the plain form's, no
 * atomics.
 *
 * lime_grouped_mlp_match_occurrence_f32 (csrc/grouped_mlp_match_f32.hip): the same composition under the MLP click predictor --
 *     qp[p, :] = qa[index[p], :] + qt[occ[p], :],   nw[p, :] = na[index[p], :] + nt[occ[p], :]
 * with na [n, Dh] = ca W_n^T + mlp.bias and nt [n_occ, Dh] = ct W_n^T (no bias: it is in na).  A pair's bits equal those of
 * lime_grouped_mlp_match_f32 on the composed rows; clamping, statuses and their order are those of
 * lime_grouped_match_occurrence_f32, with na / nt 8-byte aligned as nw is.
 *
 * lime_grouped_match_schedule_f32 (csrc/grouped_match_schedule_f32.hip): lime_grouped_match_occurrence_f32 for S time slots of every
 * pair in one launch (Model.score_schedule).  kp, g, qa, ca, qt, ct, offsets, index, n, n_occ and the weight parameters are the
 * twin's; occ int32 [S, P], remaining fp32 [S, P] (read when use_weight != 0) and logits fp32 [S, P] have leading dimension P.  Per
 * (slot s, pair p of group i), in the FACTORISED form
 *     s[h] = (kp[i H + h, :] . qa[index[p], :] + kp[i H + h, :] . qt[occ[s, p], :]) * scale,   a = softmax_h(s),
 *     logits[s, p] = (sum_h a[h] (g[i H + h, :] . ca[index[p], :] + g[i H + h, :] . ct[occ[s, p], :])) * w(remaining[s, p])
 * The news-table products run once per pair (the pass body of lime_grouped_match_f32: exact fp32 on v_mfma_f32_16x16x4_f32, the
 * compensated sum) and stay in registers across the slot loop.  The occurrence terms are FORMED IN THE KERNEL: every workgroup makes its
 * group's [n_occ, H] products with qt and with ct by the same tile product and keeps them in LDS for all its tiles -- there is no
 * workspace, and no launch and no buffer other than occ, remaining and logits grows with S P.  It rounds two partial sums where the
 * twin rounds one composed operand: the results agree to fp32 rounding, not bit for bit.
 * Without occurrence tables -- qt == ct == NULL and n_occ == 0 (occ is then not read and may be NULL), a baseline model -- the table
 * terms are absent and the bits of (s, p) are those of lime_grouped_match_indexed_f32 for pair p with remaining[s, p].
 * A workgroup per 64-pair tile of a group, fixed-order sums, no atomics: the bits of (s, p) depend on its own operands and on H, A and
 * D alone -- not on S, the slot's position, the other slots, P, G, the group's position or the pair's place in its tile.  index, occ
 * and offsets are clamped as in the twin.  Statuses before any launch: the twin's, in its order (the occurrence tables may be absent);
 * then LIME_ERR_BAD_ARG for S < 1, for occurrence tables with a NULL occ, for one table without the other or n_occ > 0 without tables;
 * then LIME_ERR_UNSUPPORTED where the tables do not fit the workgroup's LDS: 2048 T + 8 n_occ Hs bytes <= 65536, with T = 1, 2, 4, 8
 * for H <= 16, 32, 64, 128 and Hs = H rounded up to a multiple of 4 (H = 50 with 100 occurrences: 49,792 bytes; H = 128: n_occ <= 48).
 *
 * lime_grouped_match_explain_f32 (csrc/grouped_match_explain_f32.hip): the grouped match with its terms kept (Model.explain_lists /
 * Model.explain; recommend.explain_pairs states it on the host).  The score of a pair is a sum over the history slots,
 *     base[p] = sum_h attn[p, h] m[h],   attn[p, :] = softmax_h(s),   m[h] = g[i H + h, :] . cand[p, :],   logits[p] = base[p] weight[p]
 * with weight[p] = w(remaining[p]) (1 with use_weight == 0), and the entry writes, beside logits / base / weight fp32 [P]:
 *     attn fp32 [P, H] = e[h] / den   and   contrib fp32 [P, H] = (attn[p, h] m[h]) weight[p]          (each may be NULL: not written)
 *     top_slot int32 [P, m], top_value fp32 [P, m]: the m slots of largest contrib (by = LIME_EXPLAIN_BY_CONTRIBUTION) or largest attn
 *     (LIME_EXPLAIN_BY_ATTENTION) among the slots whose byte of mask is set, and the written value's bits at each.
 * mask uint8 [ceil(G / hist_div), H]: group i reads row i / hist_div -- hist_div consecutive groups share one history, as in the
 * refinement -- (NULL: every slot is eligible).  The softmax is NOT masked (reference userEncoders.py:164): the mask gates which slots
 * may be named, not what they weigh.  Order: lime_topk_rows_f32's -- larger value first, equal values (+0.0 and -0.0 are equal) lower
 * slot first, a NaN behind every number; with fewer than m eligible slots the tail holds slot -1 and value 0.0.
 * The operands take the three forms of the twins by their pointers: index == NULL: qp [P, A], cand [P, D] (lime_grouped_match_f32; occ,
 * qt, ct NULL, n and n_occ unread); index alone: tables of n rows (lime_grouped_match_indexed_f32); index, occ, qt and ct together: the
 * occurrence-composed form (lime_grouped_match_occurrence_f32).  The two products, the softmax and the expressions behind them are the
 * twins': logits[p] has the BITS of the twin on the same operands.  The selection runs in the pair's four lanes on the registers the
 * products left there (m rounds of a register argmax and two butterfly steps); no LDS beyond the twins', no workspace, no atomics,
 * fixed-order sums: a pair's bits depend neither on P, G, the group's position, the pair's place in its tile nor the grid.  index, occ
 * and offsets are clamped as in the twins; pairs outside every group are not written.  Statuses before any launch, in this order:
 * LIME_ERR_BAD_ARG for a `by` that is neither constant, a NULL kp / g / qp / cand / offsets / logits / base / weight / top_slot /
 * top_value, occ / qt / ct given in part or without index, use_weight without remaining; the twins' dimension, alignment and table
 * checks with their statuses; LIME_ERR_BAD_ARG for m < 1, m > H or hist_div < 1; LIME_ERR_UNSUPPORTED for m > 16.  G == 0 or P == 0 is
 * a success without a launch.
 *
 * lime_topk_rows_f32 (csrc/topk_rows_f32.hip): per row u < U of scores [U, C] (leading dimension ld >= C) the k best entries:
 * positions int32 [U, k] (column indices) and top_scores fp32 [U, k] (the input's bits at those positions), in descending order of
 * the score; equal scores -- +0.0 and -0.0 are equal -- lower position first; a NaN ranks behind every number, NaNs in position
 * order.  Slots behind the C-th hold position -1 and score -inf.  1 <= k <= 128, 1 <= C < 2^31, U <= 65535 (LIME_ERR_UNSUPPORTED
 * otherwise).  A row is split over workgroups of 4096 columns, their lists merged by one workgroup per row; the result is the k
 * largest of distinct integer keys and so independent of the split and the run.  workspace: lime_topk_rows_workspace(U, C) floats
 * (0 for C <= 4096: workspace may be NULL), 8-byte aligned.
 *
 * lime_topk_rows_quota_f32 (csrc/topk_quota_f32.hip): lime_topk_rows_f32 under a quota per group (Model.recommend(max_per_topic=)).
 * Column j belongs to group keys[j] (int32 [C], shared by all rows).  Walk a row's entries in lime_topk_rows_f32's order; take an
 * entry unless `quota` entries of its group were taken before it; stop at k.  positions / top_scores [U, k] hold the taken entries in
 * that order (the input's bits), the slots behind the last taken one position -1 and score -inf.  drop: NULL, or uint8 [drop_rows, C]
 * (contiguous): row r is masked by drop[r % drop_rows] -- the [S U, C] view of a schedule shares one [U, C] mask -- and an entry
 * whose byte is not 0 takes no part: it uses no quota and is never returned.  An entry whose key is outside [0, n_keys) is dropped
 * the same way; nothing outside the buffers is read.  Equivalently: the k best of the union, over the groups, of each group's `quota`
 * best -- and a chunk of the row may be cut to the first 128 entries of its OWN walk before the merged set is walked again, so the
 * passes are lime_topk_rows_f32's with a walk behind every sort, and the result does not depend on the split or the run.  Statuses
 * before any launch: LIME_ERR_BAD_ARG for a NULL scores / keys / output, bad dims, quota < 1, n_keys < 1, a drop mask with
 * drop_rows < 1, a short or misaligned workspace; LIME_ERR_UNSUPPORTED outside 1 <= k <= 128, C < 2^31, U <= 65535, n_keys <= 8192
 * (lime_list_plan's table size).  workspace: lime_topk_rows_quota_workspace(U, C) floats (0 for C <= 4096: workspace may be NULL),
 * 8-byte aligned; what it holds on entry does not matter.
 *
 * lime_mmr_rows_f32 (csrc/mmr_rows_f32.hip): maximal marginal relevance over a shortlist per row (Model.recommend(mmr_lambda=);
 * recommend.mmr_select states it on the host).  scores fp32 [R, M] and ids int32 [R, M] (both contiguous): a row's shortlist, best
 * first, as the top-k kernels return it, and the row of table fp32 [n, E] (leading dimension ld >= E) behind each entry.  An entry
 * is DEAD when its id is outside [0, n) or its score is not finite: it is never taken and its table row is never read.  With
 * first / last the first and last live entries of the row, rel[j] = (s[j] - s[last]) / (s[first] - s[last]) (0 for every j when
 * the two are equal) and cos(j, i) the cosine of table rows ids[j] and ids[i] (0 when either norm is 0), a round takes the live,
 * untaken j that maximises lam rel[j] - (1 - lam) max(0, max over the taken i of cos(j, i)), the lower j on equal values, until k
 * are taken or no live entry is left.  picks int32 [R, k]: the taken j in the order taken, -1 behind the last.  lam = 1 is the plain
 * order of the live entries (no table row is read), lam = 0 takes `first` first.  One workgroup per row: the inverse norms once,
 * then per round the picked row, normalised, staged in LDS and its M dot products with the shortlist rows; fp32 throughout,
 * fixed-order sums, no atomics, no workspace: a row's picks depend on its own operands alone, not on R, the row's position or the
 * run.  Statuses before any launch, in this order: LIME_ERR_BAD_ARG for a NULL pointer; LIME_ERR_BAD_ARG for R < 0, M < 1, k < 1,
 * k > M, n < 1, E < 1, ld < E, or lam outside [0, 1] or NaN; LIME_ERR_UNSUPPORTED for M > 128 (the top-k kernels' k limit),
 * E % 4 != 0, R > 65535.  R == 0 is a success without a launch.
 *
 * lime_calibrate_rows_f32 / lime_slate_miscalibration (csrc/calibrate_rows.hip): calibrated slates -- a slate whose topic mix follows
 * the reader's own (Steck, RecSys 2018; Model.recommend(calibrate_lambda=); recommend.calibrated_select and
 * recommend.slate_miscalibration state them on the host).
 *   The TARGET of a row: hist_keys int32 [hist_rows, H] holds the group of every history slot (a key outside [0, n_keys) is no click;
 *   -1 is the usual one), hist_weight fp32 [hist_rows, H] its weight (NULL: 1 each; a weight that is not finite or not > 0 removes
 *   the slot).  Row r reads history row r % hist_rows (the [S U] rows of a schedule share U histories).  W is the weight sum over the
 *   live slots and p[g] the weight sum of the live slots of group g divided by W, both summed in slot order; a row with W == 0 (or
 *   not finite) has NO TARGET.  The support is the groups with a live slot.  keys int32 [n]: the group of every news (a key outside
 *   [0, n_keys) is no group).
 *   lime_calibrate_rows_f32: scores fp32 [R, M] and ids int32 [R, M] (both contiguous) are a row's shortlist, best first, ids the
 *   news id.  DEAD entries and rel[j] are lime_mmr_rows_f32's: an id outside [0, n) or a non-finite score; rel[j] = (s[j] - s[last])
 *   / (s[first] - s[last]) over the live entries, 0 everywhere when the span is 0.  Round t has t entries taken, c[g] of them in
 *   group g; with T = t + 1 and q(c) = (1 - alpha) c / T + alpha p[g], entry j of group g has
 *       gain[j] = p[g] (ln q(c[g] + 1) - ln q(c[g])) / ln(1 / alpha)
 *   -- 0 when the row has no target, j has no group or p[g] is 0 --, and the round takes the live, untaken j of the largest
 *   v[j] = lam rel[j] + (1 - lam) gain[j], the lower j on equal v, until k are taken or none is left.  picks int32 [R, k]: the taken
 *   j in the order taken, -1 behind the last.  The largest gain is the smallest KL(p || q) of the slate with j added; gain lies in
 *   [0, 1] like rel; lam = 1 is the plain order of the live entries and reads neither keys nor the history.  The gain is formed once
 *   per support group and rel from the score alone: two entries of one group with equal score bits carry the same v bits, and the
 *   lower j wins.  A wave per row, four rows a workgroup, any R (the grid strides); fp32 throughout (logf, not the fast intrinsic),
 *   fixed-order sums, no atomics, no workspace: a row's picks depend on its own operands alone, not on R, its position or the run.
 *   Statuses before any launch, in this order: LIME_ERR_BAD_ARG for a NULL pointer (hist_weight may be NULL); for R < 0, M < 1,
 *   k < 1, k > M, n < 1, n_keys < 1, H < 0, hist_rows < 0 or hist_rows < 1 with H > 0; for lam outside [0, 1] or NaN; for alpha
 *   outside (0, 1) or NaN; LIME_ERR_UNSUPPORTED for M > 128, H > 128 or n_keys > 8192.  R == 0 is a success without a launch.
 *   lime_slate_miscalibration: positions int32 [R, ldp], k, offsets int64 [R + 1] or NULL and news int32 [P] with the meanings they
 *   have in lime_slate_metrics_f32 (a slot is FILLED when its position lies inside the list / the pool and the news id behind it
 *   inside [0, n)).  With c[g] the filled slots of group g and F their number,
 *       value[r] = sum over the support of p[g] ln(p[g] / ((1 - alpha) c[g] / F + alpha p[g]))      (fp64 [R])
 *   status int32 [R]: 1 no target; else 2 no filled slot; else 0 -- and value is 0 where status is not.  alpha is the fp32 number the
 *   selection reads, widened: the metric measures the objective that was optimised.  fp64 sums and fp64 log, p
 *   in slot order and the terms in the order of the groups' first slots; a wave per slate.  Statuses before any launch, in this
 *   order: LIME_ERR_BAD_ARG for a NULL pointer (offsets and hist_weight may be NULL); for R < 0, P < 0, k < 1, k > ldp, n < 1,
 *   n_keys < 1, H < 0, hist_rows < 0 or hist_rows < 1 with H > 0; for alpha outside (0, 1) or NaN; LIME_ERR_UNSUPPORTED for k > 128,
 *   H > 128 or n_keys > 8192.  R == 0 is a success without a launch. */
int lime_grouped_match_f32(const float* kp, const float* g, const float* qp, const float* cand, const float* remaining,
                           const int64_t* offsets, float* logits, int64_t G, int64_t P, int32_t H, int32_t A, int32_t D, float scale,
                           float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty, void* stream);
int lime_grouped_match_indexed_f32(const float* kp, const float* g, const float* qp, const float* cand, const float* remaining,
                                   const int64_t* offsets, const int32_t* index, int64_t n, float* logits, int64_t G, int64_t P,
                                   int32_t H, int32_t A, int32_t D, float scale, float alpha_s, float beta_s, int32_t use_weight,
                                   int32_t use_penalty, void* stream);
int lime_grouped_mlp_match_f32(const float* kp, const float* gu, const float* qp, const float* nw, const float* w_out, const float* b_out,
                               const int64_t* offsets, float* logits, int64_t G, int64_t P, int32_t H, int32_t A, int32_t Dh, float scale,
                               void* stream);
int lime_grouped_mlp_match_indexed_f32(const float* kp, const float* gu, const float* qp, const float* nw, const float* w_out,
                                       const float* b_out, const int64_t* offsets, const int32_t* index, int64_t n, float* logits,
                                       int64_t G, int64_t P, int32_t H, int32_t A, int32_t Dh, float scale, void* stream);
int lime_grouped_match_occurrence_f32(const float* kp, const float* g, const float* qa, const float* ca, const float* qt, const float* ct,
                                      const float* remaining, const int64_t* offsets, const int32_t* index, int64_t n,
                                      const int32_t* occ, int64_t n_occ, float* logits, int64_t G, int64_t P, int32_t H, int32_t A,
                                      int32_t D, float scale, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty,
                                      void* stream);
int lime_grouped_mlp_match_occurrence_f32(const float* kp, const float* gu, const float* qa, const float* na, const float* qt,
                                          const float* nt, const float* w_out, const float* b_out, const int64_t* offsets,
                                          const int32_t* index, int64_t n, const int32_t* occ, int64_t n_occ, float* logits, int64_t G,
                                          int64_t P, int32_t H, int32_t A, int32_t Dh, float scale, void* stream);
int lime_grouped_match_schedule_f32(const float* kp, const float* g, const float* qa, const float* ca, const float* qt, const float* ct,
                                    const float* remaining, const int64_t* offsets, const int32_t* index, int64_t n, const int32_t* occ,
                                    int64_t n_occ, float* logits, int64_t G, int64_t P, int32_t S, int32_t H, int32_t A, int32_t D,
                                    float scale, float alpha_s, float beta_s, int32_t use_weight, int32_t use_penalty, void* stream);
/* what lime_grouped_match_explain_f32 ranks the history slots of a pair by */
enum { LIME_EXPLAIN_BY_CONTRIBUTION = 0, LIME_EXPLAIN_BY_ATTENTION = 1 };
int lime_grouped_match_explain_f32(const float* kp, const float* g, const float* qp, const float* cand, const float* qt, const float* ct,
                                   const float* remaining, const int64_t* offsets, const int32_t* index, int64_t n, const int32_t* occ,
                                   int64_t n_occ, const uint8_t* mask, int32_t hist_div, int32_t m, int32_t by, float* logits, float* base,
                                   float* weight, float* attn, float* contrib, int32_t* top_slot, float* top_value, int64_t G, int64_t P,
                                   int32_t H, int32_t A, int32_t D, float scale, float alpha_s, float beta_s, int32_t use_weight,
                                   int32_t use_penalty, void* stream);
int64_t lime_topk_rows_workspace(int64_t U, int64_t C);
int lime_topk_rows_f32(const float* scores, int64_t ld, int64_t U, int64_t C, int32_t k, int32_t* positions, float* top_scores,
                       float* workspace, int64_t workspace_floats, void* stream);
int64_t lime_topk_rows_quota_workspace(int64_t U, int64_t C);
int lime_topk_rows_quota_f32(const float* scores, int64_t ld, int64_t U, int64_t C, const int32_t* keys, int32_t n_keys, int32_t quota,
                             const uint8_t* drop, int64_t drop_rows, int32_t k, int32_t* positions, float* top_scores, float* workspace,
                             int64_t workspace_floats, void* stream);
int lime_mmr_rows_f32(const float* scores, const int32_t* ids, int64_t R, int32_t M, const float* table, int64_t ld, int64_t n, int32_t E,
                      float lam, int32_t k, int32_t* picks, void* stream);
int lime_calibrate_rows_f32(const float* scores, const int32_t* ids, int64_t R, int32_t M, const int32_t* keys, int64_t n, int32_t n_keys,
                            const int32_t* hist_keys, const float* hist_weight, int64_t hist_rows, int32_t H, float lam, float alpha,
                            int32_t k, int32_t* picks, void* stream);
int lime_slate_miscalibration(const int32_t* positions, int64_t R, int64_t ldp, int32_t k, const int64_t* offsets, const int32_t* news,
                              int64_t P, const int32_t* keys, int64_t n, int32_t n_keys, const int32_t* hist_keys, const float* hist_weight,
                              int64_t hist_rows, int32_t H, float alpha, double* value, int32_t* status, void* stream);

/* =====================================================================================================
 * Candidate lists (Model.score_lists / Model.recommend_lists): U users, each with its OWN list of candidates, as a CSR over P
 * (user, candidate) pairs -- offsets int64 [U + 1] on the device, user u owns pairs offsets[u] .. offsets[u + 1] - 1.
 *
 * lime_list_plan_count / lime_list_plan (csrc/list_plan.hip): the device form of recommend.list_plan, bit for bit.  keys int32 [P] is
 * the topic id of every pair, 0 <= key < T_all <= 8192 (LIME_ERR_UNSUPPORTED beyond: one LDS table of bins per workgroup; U, P < 2^31).
 * The count writes n_distinct int32 [U], the number of distinct keys of each list.  The plan takes S >= max(1, max n_distinct) slots
 * per user and writes
 *     order int64 [P]: the pairs of user u stay in rows offsets[u] .. offsets[u + 1] - 1, sorted by key, stable in list order;
 *     group_offsets int64 [U S + 1]: group u S + s -- user u's s-th key in ascending order -- owns rows group_offsets[u S + s] ..
 *         group_offsets[u S + s + 1] - 1 of order; a slot behind the user's last key is an empty group;
 *     slot_key int32 [U S]: the key of each slot; an unused slot repeats the key of the user's slot 0 (key 0 for an empty list).
 * One workgroup per user, no global atomics: the result is a fixed function of the inputs.  Every offset is clamped into [0, P].  A
 * pair whose key is outside [0, T_all) takes no slot: such pairs go behind the user's last key in order, so order stays a permutation,
 * every pair with a key in range is in its right group and nothing outside the buffers is read or written; the last user's such pairs
 * lie behind group_offsets[U S] -- in no group --, another user's lie in the rows of that user's last slot.  With an S below a user's
 * n_distinct the keys beyond S get no slot entry (their rows run on into the next group).
 *
 * lime_topk_segments_f32 (csrc/topk_segments_f32.hip): lime_topk_rows_f32 over the segments of a flat scores fp32 [P]: positions
 * int32 [U, k] -- counted WITHIN the segment -- and top_scores fp32 [U, k] (the input's bits), the same order (descending; +0.0 ==
 * -0.0; equal scores lower position first; a NaN behind every number, NaNs in position order); slots behind the segment's length
 * -- all k of an empty segment -- hold -1 and -inf.  1 <= k <= 128, every segment shorter than 2^31, U + P / 4096 < 2^31
 * (LIME_ERR_UNSUPPORTED otherwise).  A segment longer than 4096 is split into chunks whose lists one workgroup merges; the grid is
 * U + P / 4096 chunks, which covers every split without reading the device, and the result -- the k largest of distinct integer
 * keys -- is independent of the split and the run.  Offsets are clamped into [0, P].  workspace: lime_topk_segments_workspace(U, P)
 * floats (never 0 for U >= 1), 8-byte aligned; what it holds on entry does not matter.
 *
 * lime_topk_segments_quota_f32 (csrc/topk_quota_f32.hip): lime_topk_rows_quota_f32's walk over the segments of a CSR
 * (Model.recommend_lists(max_per_topic=)): keys int32 [P] and drop uint8 [P] (or NULL) lie beside scores, entry by entry; positions
 * count WITHIN the segment.  Limits, grid rule and clamped offsets are lime_topk_segments_f32's, with quota >= 1 and 1 <= n_keys <=
 * 8192 added as in the row form.  workspace: lime_topk_segments_quota_workspace(U, P) floats, 8-byte aligned; what it holds on entry
 * does not matter. */
int lime_list_plan_count(const int32_t* keys, const int64_t* offsets, int64_t U, int64_t P, int32_t T_all, int32_t* n_distinct,
                         void* stream);
int lime_list_plan(const int32_t* keys, const int64_t* offsets, int64_t U, int64_t P, int32_t T_all, int32_t S, int64_t* order,
                   int64_t* group_offsets, int32_t* slot_key, void* stream);
int64_t lime_topk_segments_workspace(int64_t U, int64_t P);
int lime_topk_segments_f32(const float* scores, const int64_t* offsets, int64_t U, int64_t P, int32_t k, int32_t* positions,
                           float* top_scores, float* workspace, int64_t workspace_floats, void* stream);
int64_t lime_topk_segments_quota_workspace(int64_t U, int64_t P);
int lime_topk_segments_quota_f32(const float* scores, const int64_t* offsets, int64_t U, int64_t P, const int32_t* keys, int32_t n_keys,
                                 int32_t quota, const uint8_t* drop, int32_t k, int32_t* positions, float* top_scores, float* workspace,
                                 int64_t workspace_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIME_HIP_H */
