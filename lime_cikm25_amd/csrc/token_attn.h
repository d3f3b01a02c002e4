// Between the fp32 token-attention routing (token_attn_f32.hip: lime_token_attention_f32 and lime_token_attention_bwd_f32, each taking
// its argument block, one pure route per direction) and the units that own the kernels: one launcher per
// family, which runs the instantiation the route chose and decides nothing itself.  A choice outside the table of built
// instantiations is LIME_ERR_UNSUPPORTED with a message, as in gemm_pp.h.
#pragma once
#include "common.h"
#include "dropout.h"

// ---- forward
// n: the family's template argument -- NT of token_attn_sp_kernel / _sp_vocab_kernel / token_attn_kernel, NK of wide_fwd_kernel, the
// length bucket of token_attn_fwd_dropout_kernel; fast / map: token_attn_kernel<NT, FAST, false, MAP>, map: token_attn_sp_kernel<NT, MAP>
// and token_attn_sp_long_kernel<MAP>; stats: the LIME_ATTN_STATS_* pass in front of attn_fwd_long_dropout_kernel.
struct LimeAttnRoute { int family, n; bool fast, map; int stats; };

// Pure: a function of the block (pointers: NULL-ness and alignment only) and the split mode; no HIP call.  LIME_OK with r->family set
// (LIME_ATTN_NONE: nothing to launch), LIME_NOT_APPLICABLE (vocab form), or the form's refusal.
int lime_attn_route(const lime_token_attention_args& a, int split_mode, LimeAttnRoute* r);
const char* lime_attn_entry(int form);                // the historical name the form's messages carry
static inline LimeDropout lime_attn_dropout(const lime_token_attention_args& a) {
    return a.form == LIME_ATTN_FORM_DROPOUT ? lime_make_dropout(a.dropout_p, a.dropout_seed, a.dropout_site) : LimeDropout{0, 0, 1.f};
}
int lime_attn_sp_launch(const LimeAttnRoute& r, const lime_token_attention_args& a, hipStream_t s);        // token_attn_sp_f32.hip: _SP, _SP_LONG, _SP_VOCAB
int lime_attn_mfma_launch(const LimeAttnRoute& r, const lime_token_attention_args& a, hipStream_t s);      // token_attn_f32.hip: _MFMA
int lime_attn_wide_launch(const LimeAttnRoute& r, const lime_token_attention_args& a, hipStream_t s);      // token_attn_wide_f32.hip: _WIDE
int lime_attn_dropout_launch(const LimeAttnRoute& r, const lime_token_attention_args& a, hipStream_t s);   // token_attn_train_f32.hip: _DROPOUT, _DROPOUT_LONG
// token_attn_wide_f32.hip: what every wide call (forward and backward) checks first; names `entry` in its messages
int lime_attn_wide_limits(const char* entry, int S, int n_head, int hd, int hs, long n_seq);

// ---- backward
// n: the length bucket SP of token_attn_bwd_kernel, FULL (0 / 1) of attn_bwd_sp_kernel, NK of the wide pair; pass: the LIME_BWD_ATTN_PASS_*
// launch in front of a blocked kernel; reduce: attn_dq_reduce_kernel follows it.
struct LimeAttnBwdRoute { int family, n, pass; bool reduce; };

// Pure, as lime_attn_route: LIME_OK with r->family set (LIME_BWD_ATTN_NONE: nothing to launch), or the refusal of the form a.entry names.
int lime_attn_bwd_route(const lime_token_attention_bwd_args& a, int split_mode, LimeAttnBwdRoute* r);
static inline LimeDropout lime_attn_bwd_dropout(const lime_token_attention_bwd_args& a) {
    return lime_make_dropout(a.dropout_p, a.dropout_seed, a.dropout_site);       // the lse form's block holds p = 0
}
// token_attn_train_f32.hip: the blocked backward's workspace, stated once for the size query, the route's check and the launch -- the row
// statistics (lse and delta per (token, head)) in its first `stats` floats, behind them one [tokens][n_head * 32] dq slab per key block
// behind the first (n_blk - 1 of them), `total` floats in all
struct LimeAttnBwdCarve { int n_blk; int64_t stats, total; };
LimeAttnBwdCarve lime_attn_bwd_carve(int n_seq, int S, int n_head);
int lime_attn_bwd_launch(const LimeAttnBwdRoute& r, const lime_token_attention_bwd_args& a, hipStream_t s);        // token_attn_train_f32.hip: _ONE_PASS, _LONG, _LONG_SP
int lime_attn_bwd_sp_launch(const LimeAttnBwdRoute& r, const lime_token_attention_bwd_args& a, hipStream_t s);     // token_attn_bwd_sp_f32.hip: _SP
int lime_attn_bwd_wide_launch(const LimeAttnBwdRoute& r, const lime_token_attention_bwd_args& a, hipStream_t s);   // token_attn_wide_f32.hip: _WIDE
