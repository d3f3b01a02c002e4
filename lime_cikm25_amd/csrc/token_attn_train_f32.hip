// The token attention that only training runs: the fp32 kernels of lime_token_attention_bwd_f32 (dQ / dK / dV of
// softmax(scale Q K^T) V per (sequence, head), probabilities recomputed) and of lime_token_attention_f32's dropout form (the forward with
// probability dropout).  The two entries, the checks and the choice among these kernels: token_attn_f32.hip (one pure route per direction).
//
//   S <= 128   token_attn_bwd_kernel<SP>, token_attn_fwd_dropout_kernel<SP>: one pass, fp32 MFMA (64 < S <= 128 without a key mask: the
//              split-product backward of token_attn_bwd_sp_f32.hip, and the forward of token_attn_sp_f32.hip, come first)
//   S > 128    attn_stats_kernel<SPX> (row statistics: serves the forward with dropout AND the backward), or attn_delta_kernel behind a
//              forward that kept its log-sum-exp; then attn_fwd_long_dropout_kernel, or attn_bwd_long_kernel (fp32 MFMA) /
//              attn_bwd_long_sp_kernel (split product, lime_set_split_gemm) + attn_dq_reduce_kernel over the key blocks' dQ slabs
#include "dev_helpers.h"
#include "dropout.h"
#include "gemm_pp.h"
#include "token_attn.h"
#include "split_mfma.h"

using namespace lime_dev;

namespace {

// ---------------------------------------------------------------------------------------------------
// token attention backward (unmasked encoder-layer attention, newsEncoders.py:316,320).
// A problem = one (sequence, head); a wave owns 16 query rows (and, for dK / dV, the 16 key rows of the same numbers);
// a problem takes SP / 16 waves, an eight-wave workgroup 128 / SP problems.  Everything goes through
// v_mfma_f32_16x16x4_f32:
//   S = scale Q K^T -> P = softmax(S) (registers) -> LDS;   dP = dO V^T (registers);  delta = rowsum(P dP)
//   dV = P^T dO;   dS = scale P (dP - delta) -> LDS over P;   dQ = dS K;   dK = dS^T Q
// The grid is persistent (one workgroup per CU: the P / dS image leaves room for one): a workgroup walks its problems and
// holds the NEXT problem's Q / K / V / dO rows in registers while it computes the current one, so the global latency of
// the staging is off the critical path; two waves per SIMD cover each other's softmax and LDS phases.
// ---------------------------------------------------------------------------------------------------
// (scores are taken to the log2 domain, LOG2E of dev_helpers.h: p = exp2(s' - max') on v_exp_f32, as the forward kernel of
// token_attn_f32.hip computes them)
constexpr int AB_LD = 36;        // Q / K / V / dO rows: 32 columns + 4: 16-byte aligned rows for ds_read_b128 / ds_write_b128
#ifndef LIME_ATTN_BWD_ABLATE
#define LIME_ATTN_BWD_ABLATE 0   // tools/attn_bwd_ablate.py builds variants with phases removed (results garbage)
#endif

template <int SP>
__global__ __launch_bounds__(512) void token_attn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                              const float* __restrict__ v, long ld, const float* __restrict__ dout,
                                                              long ldo, float* __restrict__ dq, float* __restrict__ dk,
                                                              float* __restrict__ dv, long ldd, int n_seq, int S, int n_head,
                                                              int head_dim, int head_stride, float scale, int vec,
                                                              LimeDropout drop, const unsigned char* __restrict__ key_mask) {
    constexpr int NT = SP / 16;                 // 16-column score tiles per row
    constexpr int WPP = SP / 16;                // waves per problem
    constexpr int PPW = 8 / WPP;                // problems per workgroup
    constexpr int TPP = 64 * WPP;               // threads per problem
    constexpr int LDP = SP + 2;
    constexpr int PROB_FLOATS = 4 * SP * AB_LD + SP * LDP;
    constexpr int NV4 = SP * 8 / TPP;           // float4 per thread and operand (Q, K, V): 2
    constexpr int NV2 = SP * 16 / TPP;          // float2 per thread (dO): 4
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, kg = lane >> 4;
    const int pw = wave / WPP;                  // problem slot of this wave
    const int wr = wave % WPP;                  // which 16-row block of the problem
    const int lt = tid - pw * TPP;              // thread index inside the problem
    const long n_prob = (long)n_seq * n_head;
    float* Qs = smem + pw * PROB_FLOATS;
    float* Ks = Qs + SP * AB_LD;
    float* Vs = Ks + SP * AB_LD;
    float* Os = Vs + SP * AB_LD;                // dO
    float* Ps = Os + SP * AB_LD;                // P, then dS
    const int R0 = 16 * wr;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};

    f32x4 rq[NV4], rk[NV4], rv[NV4];
    f32x2 ro[NV2];
    auto fetch = [&](long prob) {               // rows of problem `prob` -> registers (vec layout only)
        const bool live = prob < n_prob;
        const int seq = live ? (int)(prob / n_head) : 0, head = live ? (int)(prob % n_head) : 0;
        const long row_base = (long)seq * S;
#pragma unroll
        for (int u = 0; u < NV4; ++u) {
            const int e = lt + TPP * u, r = e >> 3, c = (e & 7) * 4;
            const bool ok = live && r < S && !(LIME_ATTN_BWD_ABLATE & 1);
            const long g = (row_base + (ok ? r : 0)) * ld + (long)head * head_stride + c;
            rq[u] = ok ? *reinterpret_cast<const f32x4*>(q + g) : z4;
            rk[u] = ok ? *reinterpret_cast<const f32x4*>(k + g) : z4;
            rv[u] = ok ? *reinterpret_cast<const f32x4*>(v + g) : z4;
        }
#pragma unroll
        for (int u = 0; u < NV2; ++u) {
            const int e = lt + TPP * u, r = e >> 4, c = (e & 15) * 2;
            const bool ok = live && r < S && c < head_dim && !(LIME_ATTN_BWD_ABLATE & 1);
            f32x2 d = {0.f, 0.f};
            if (ok) d = *reinterpret_cast<const f32x2*>(dout + (row_base + r) * ldo + (long)head * head_dim + c);
            ro[u] = d;
        }
    };
    auto commit = [&]() {                       // registers -> this problem's LDS images
#pragma unroll
        for (int u = 0; u < NV4; ++u) {
            const int e = lt + TPP * u, r = e >> 3, c = (e & 7) * 4;
            *reinterpret_cast<f32x4*>(&Qs[r * AB_LD + c]) = rq[u];
            *reinterpret_cast<f32x4*>(&Ks[r * AB_LD + c]) = rk[u];
            *reinterpret_cast<f32x4*>(&Vs[r * AB_LD + c]) = rv[u];
        }
#pragma unroll
        for (int u = 0; u < NV2; ++u) {
            const int e = lt + TPP * u, r = e >> 4, c = (e & 15) * 2;
            *reinterpret_cast<f32x2*>(&Os[r * AB_LD + c]) = ro[u];
        }
    };
    auto stage_scalar = [&](long prob) {        // any layout: straight into LDS (zero beyond S rows / head_dim columns)
        const bool live = prob < n_prob;
        const int seq = live ? (int)(prob / n_head) : 0, head = live ? (int)(prob % n_head) : 0;
        const long row_base = (long)seq * S;
        for (int e = lt; e < SP * 32; e += TPP) {
            const int r = e >> 5, c = e & 31;
            const bool ok = live && r < S && c < head_dim;
            const long g = (row_base + r) * ld + (long)head * head_stride + c;
            Qs[r * AB_LD + c] = ok ? q[g] : 0.f;
            Ks[r * AB_LD + c] = ok ? k[g] : 0.f;
            Vs[r * AB_LD + c] = ok ? v[g] : 0.f;
            Os[r * AB_LD + c] = ok ? dout[(row_base + r) * ldo + (long)head * head_dim + c] : 0.f;
        }
    };

    const long n_group = (n_prob + PPW - 1) / PPW;
    if (vec && (long)blockIdx.x < n_group) fetch((long)blockIdx.x * PPW + pw);
    for (long grp = blockIdx.x; grp < n_group; grp += gridDim.x) {
        const long prob = grp * PPW + pw;
        const bool live = prob < n_prob;
        const int seq = live ? (int)(prob / n_head) : 0, head = live ? (int)(prob % n_head) : 0;
        if (vec) commit(); else stage_scalar(prob);
        __syncthreads();
        if (vec && grp + gridDim.x < n_group) fetch((grp + gridDim.x) * PPW + pw);       // in flight during the compute below

        // ---- S tiles and dP tiles of this wave's 16 query rows ------------------------------------------------------
        f32x4 p[NT], dp[NT], pd[NT];
        {
            // the summation index d is only a label: lane group kg takes d = 8 kg .. 8 kg + 7 over the eight MFMA steps, so a
            // lane's eight operands are 32 consecutive bytes of its row -- two ds_read_b128 instead of eight ds_read_b32
            f32x4 qa[2], oa[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                qa[h] = *reinterpret_cast<const f32x4*>(&Qs[(R0 + fi) * AB_LD + 8 * kg + 4 * h]);
                oa[h] = *reinterpret_cast<const f32x4*>(&Os[(R0 + fi) * AB_LD + 8 * kg + 4 * h]);
            }
            // two score tiles at a time (four independent accumulator chains), the next pair's K / V fragments are requested
            // before this pair's MFMAs are issued
            f32x4 kb[2][2][2], vb[2][2][2];               // [buffer][tile of the pair][half]
            auto load_pair = [&](int buf, int ct) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        if constexpr ((LIME_ATTN_BWD_ABLATE & 64) != 0) {      // no K / V fragment reads: MFMAs on register operands
                            kb[buf][t][h] = qa[h] + (float)ct;
                            vb[buf][t][h] = oa[h] + (float)ct;
                            continue;
                        }
                        kb[buf][t][h] = *reinterpret_cast<const f32x4*>(&Ks[(16 * (ct + t) + fi) * AB_LD + 8 * kg + 4 * h]);
                        vb[buf][t][h] = *reinterpret_cast<const f32x4*>(&Vs[(16 * (ct + t) + fi) * AB_LD + 8 * kg + 4 * h]);
                    }
            };
            load_pair(0, 0);
#pragma unroll
            for (int ct = 0; ct < NT; ct += 2) {
                const int buf = (ct >> 1) & 1;
                if (ct + 2 < NT) load_pair(buf ^ 1, ct + 2);
                f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, d0 = s0, s1 = s0, d1 = s0;
#pragma unroll
                for (int s = 0; s < ((LIME_ATTN_BWD_ABLATE & 2) ? 0 : 8); ++s) {
                    s0 = mfma16(qa[s >> 2][s & 3], kb[buf][0][s >> 2][s & 3], s0);
                    d0 = mfma16(oa[s >> 2][s & 3], vb[buf][0][s >> 2][s & 3], d0);
                    s1 = mfma16(qa[s >> 2][s & 3], kb[buf][1][s >> 2][s & 3], s1);
                    d1 = mfma16(oa[s >> 2][s & 3], vb[buf][1][s >> 2][s & 3], d1);
                }
                p[ct] = s0; dp[ct] = d0; p[ct + 1] = s1; dp[ct + 1] = d1;
            }
        }
        // key mask of layers.MultiHeadAttention (layers.py:227-232: masked_fill(mask == 0, -1e9) before the softmax): a masked
        // score is a constant, its dS is zero
        bool kmask[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
            kmask[ct] = key_mask != nullptr && live && 16 * ct + fi < S && key_mask[(long)seq * S + 16 * ct + fi] == 0;
        // softmax over the row (columns: tiles ct x the 16 lanes with the same kg), then delta and dS
#pragma unroll
        for (int r = 0; r < ((LIME_ATTN_BWD_ABLATE & 4) ? 0 : 4); ++r) {
            float mx = -INFINITY;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const bool col_ok = 16 * ct + fi < S;
                const float sv = col_ok ? (kmask[ct] ? -1e9f * LOG2E : p[ct][r] * (scale * LOG2E)) : -INFINITY;
                p[ct][r] = sv;
                mx = fmaxf(mx, sv);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2));
            mx = fmaxf(mx, __shfl_xor(mx, 4)); mx = fmaxf(mx, __shfl_xor(mx, 8));
            float sum = 0.f;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const float e = __builtin_amdgcn_exp2f(p[ct][r] - mx);
                p[ct][r] = e;
                sum += e;
            }
            sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4); sum += __shfl_xor(sum, 8);
            const float inv = 1.0f / sum;
            float dl = 0.f;
            // attention-probability dropout (nn.MultiheadAttention's dropout, newsEncoders.py:244-247): the forward used
            // keep * P / (1 - p); its mask is regenerated from the element's index.  kq[ct]: the factor on P for the dV product.
            const uint64_t mrow = ((uint64_t)prob * S + (uint64_t)(R0 + 4 * kg + r)) * (uint64_t)S;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                p[ct][r] *= inv;
                if (drop.thresh != 0) {
                    const float f = lime_keep(drop, mrow + (uint64_t)(16 * ct + fi)) ? drop.scale : 0.f;
                    dp[ct][r] *= f;
                    pd[ct][r] = p[ct][r] * f;
                }
                dl += p[ct][r] * dp[ct][r];
            }
            dl += __shfl_xor(dl, 1); dl += __shfl_xor(dl, 2); dl += __shfl_xor(dl, 4); dl += __shfl_xor(dl, 8);
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) dp[ct][r] = kmask[ct] ? 0.f : scale * p[ct][r] * (dp[ct][r] - dl);      // dS
        }
        // P (as the forward multiplied it into V) -> LDS
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Ps[(R0 + 4 * kg + r) * LDP + 16 * ct + fi] = drop.thresh != 0 ? pd[ct][r] : p[ct][r];
        __syncthreads();

        const long out_row0 = (long)seq * S + R0;
        auto store_tile = [&](float* dst, int dt, const f32x4& a) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * kg + r, col = 16 * dt + fi;
                if (live && R0 + row < S && col < head_stride && !((LIME_ATTN_BWD_ABLATE & 32) && a[r] != 12345.f))
                    dst[(out_row0 + row) * ldd + (long)head * head_stride + col] = a[r];
            }
        };
        // ---- dV[j, d] = sum_i P[i, j] dO[i, d] for the wave's key rows j ---------------------------------------------
        {
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll 8
            for (int s = 0; s < ((LIME_ATTN_BWD_ABLATE & 8) ? 0 : SP / 4); ++s) {
                const int i = 4 * s + kg;
                const float a = Ps[i * LDP + R0 + fi];
                a0 = mfma16(a, Os[i * AB_LD + fi], a0);
                a1 = mfma16(a, Os[i * AB_LD + 16 + fi], a1);
            }
            store_tile(dv, 0, a0);
            store_tile(dv, 1, a1);
        }
        __syncthreads();
        // dS over P
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ps[(R0 + 4 * kg + r) * LDP + 16 * ct + fi] = dp[ct][r];
        __syncthreads();
        // ---- dQ[i, d] = sum_j dS[i, j] K[j, d];  dK[j, d] = sum_i dS[i, j] Q[i, d] -----------------------------------
        {
            f32x4 aq0 = {0.f, 0.f, 0.f, 0.f}, aq1 = aq0, ak0 = aq0, ak1 = aq0;
#pragma unroll 8
            for (int s = 0; s < ((LIME_ATTN_BWD_ABLATE & 16) ? 0 : SP / 4); ++s) {
                const int j = 4 * s + kg;
                const float ds_row = Ps[(R0 + fi) * LDP + j];          // dS[i = this wave's query row, j]
                aq0 = mfma16(ds_row, Ks[j * AB_LD + fi], aq0);
                aq1 = mfma16(ds_row, Ks[j * AB_LD + 16 + fi], aq1);
                const float ds_col = Ps[j * LDP + R0 + fi];            // dS[i = j, this wave's key row]
                ak0 = mfma16(ds_col, Qs[j * AB_LD + fi], ak0);
                ak1 = mfma16(ds_col, Qs[j * AB_LD + 16 + fi], ak1);
            }
            store_tile(dq, 0, aq0); store_tile(dq, 1, aq1);
            store_tile(dk, 0, ak0); store_tile(dk, 1, ak1);
        }
        __syncthreads();                        // the images are free for the next problem
    }
}

// ---------------------------------------------------------------------------------------------------
// Training-mode forward of the encoder attention WITH probability dropout: out = (keep * softmax(scale Q K^T) / (1 - p)) V.
// Eight waves, 16 query rows each, S <= 128; the scoring kernel in token_attn_f32.hip stays free of the mask arithmetic.
// The scores are computed TRANSPOSED (S^T = K Q^T): the MFMA result layout then holds, per lane, P^T[j = 4 kg + r][i = lane's
// query] -- exactly the B operand of the second product O^T = V^T P^T -- so the probabilities never leave the registers (no
// P image in LDS; K and V images only, 37 KB per workgroup); the softmax of a query is a reduction over the lane's own
// registers and its three kg partners; and the four r of an accumulator are four consecutive keys: one mask hash each.
// ---------------------------------------------------------------------------------------------------
template <int SP>
__global__ __launch_bounds__(512, 2) void token_attn_fwd_dropout_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                         const float* __restrict__ v, long ld, float* __restrict__ out,
                                                                         long ldo, int n_seq, int S, int n_head, int head_dim,
                                                                         int head_stride, float scale, LimeDropout drop, int vec) {
    constexpr int NT = SP / 16, WPP = SP / 16, PPW = 8 / WPP, TPP = 64 * WPP;
    constexpr int PROB_FLOATS = 2 * SP * AB_LD;            // K and V images; a lane's Q operand comes straight from global
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, kg = lane >> 4;
    const int pw = wave / WPP, wr = wave % WPP, lt = tid - pw * TPP;
    const long n_prob = (long)n_seq * n_head;
    const long prob = (long)blockIdx.x * PPW + pw;
    const bool live = prob < n_prob;
    const int seq = live ? (int)(prob / n_head) : 0, head = live ? (int)(prob % n_head) : 0;
    float* Ks = smem + pw * PROB_FLOATS;
    float* Vs = Ks + SP * AB_LD;
    const int R0 = 16 * wr;
    const long row_base = (long)seq * S;
    // B operand of S^T = K Q^T: Q[i = R0 + fi][d = 8 kg .. 8 kg + 7] (k-permuted: 32 consecutive bytes of the lane's row)
    f32x4 qf[2];
    {
        const bool ok = live && R0 + fi < S;
        const float* qrow = q + (row_base + (ok ? R0 + fi : 0)) * ld + (long)head * head_stride + 8 * kg;
        if (vec) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            qf[0] = ok ? *reinterpret_cast<const f32x4*>(qrow) : z;
            qf[1] = ok ? *reinterpret_cast<const f32x4*>(qrow + 4) : z;
        } else {
#pragma unroll
            for (int t = 0; t < 8; ++t) qf[t >> 2][t & 3] = (ok && 8 * kg + t < head_dim) ? qrow[t] : 0.f;
        }
    }
    if (vec) {                  // 32-float head rows on 16-byte boundaries, zero padding columns
        for (int e = lt; e < SP * 8; e += TPP) {
            const int r = e >> 3, c = (e & 7) * 4;
            const bool ok = live && r < S;
            const long g = (row_base + (ok ? r : 0)) * ld + (long)head * head_stride + c;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(&Ks[r * AB_LD + c]) = ok ? *reinterpret_cast<const f32x4*>(k + g) : z;
            *reinterpret_cast<f32x4*>(&Vs[r * AB_LD + c]) = ok ? *reinterpret_cast<const f32x4*>(v + g) : z;
        }
    } else {
        for (int e = lt; e < SP * 32; e += TPP) {
            const int r = e >> 5, c = e & 31;
            const bool ok = live && r < S && c < head_dim;
            const long g = (row_base + r) * ld + (long)head * head_stride + c;
            Ks[r * AB_LD + c] = ok ? k[g] : 0.f;
            Vs[r * AB_LD + c] = ok ? v[g] : 0.f;
        }
    }
    __syncthreads();
    // S^T tiles: rows = keys 16 ct + 4 kg + r, column = this lane's query R0 + fi
    f32x4 p[NT];
    {
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            f32x4 kf[2];                       // A operand: K[j = 16 ct + fi][d = 8 kg ..]
#pragma unroll
            for (int h = 0; h < 2; ++h) kf[h] = *reinterpret_cast<const f32x4*>(&Ks[(16 * ct + fi) * AB_LD + 8 * kg + 4 * h]);
#pragma unroll
            for (int t = 0; t < 8; ++t) a = mfma16(kf[t >> 2][t & 3], qf[t >> 2][t & 3], a);
            p[ct] = a;
        }
    }
    // softmax over the keys of this lane's query: the lane's registers, then the kg partners (lanes +-16, +-32)
    float mx = -INFINITY;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sv = (16 * ct + 4 * kg + r < S) ? p[ct][r] * (scale * LOG2E) : -INFINITY;
            p[ct][r] = sv;
            mx = fmaxf(mx, sv);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __builtin_amdgcn_exp2f(p[ct][r] - mx);
            p[ct][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = drop.scale / sum;
    // mask element ((prob S + i) S + j): the four r of an accumulator are keys 16 ct + 4 kg .. + 3 -- one hash
    const uint64_t mrow = ((uint64_t)prob * S + (uint64_t)(R0 + fi)) * (uint64_t)S;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
        unsigned m = 0xFu;
        if (drop.thresh != 0) {
            const uint64_t idx = mrow + (uint64_t)(16 * ct + 4 * kg);
            if ((idx & 3) == 0) m = lime_keep4(drop, idx >> 2);
            else
#pragma unroll
                for (int r = 0; r < 4; ++r) m = (m & ~(1u << r)) | ((lime_keep(drop, idx + r) ? 1u : 0u) << r);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) p[ct][r] = (m >> r) & 1u ? p[ct][r] * inv : 0.f;
    }
    // O^T[d][i] = sum_j V^T[d][j] P^T[j][i]: A = V[j = 16 ct + 4 kg + t][d = 16 dt + fi] from LDS, B = p[ct][t] from registers
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = 16 * ct + 4 * kg + t;
            o0 = mfma16(Vs[j * AB_LD + fi], p[ct][t], o0);
            o1 = mfma16(Vs[j * AB_LD + 16 + fi], p[ct][t], o1);
        }
    // the lane holds O[i = R0 + fi][d = 4 kg + r] (o0) and [16 + 4 kg + r] (o1)
    if (live && R0 + fi < S) {
        float* o = out + (row_base + R0 + fi) * ldo + (long)head * head_dim;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (4 * kg + r < head_dim) o[4 * kg + r] = o0[r];
            if (16 + 4 * kg + r < head_dim) o[16 + 4 * kg + r] = o1[r];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Sequences longer than 128 tokens (BASELINE config 4: body length 512): the same mathematics in 128 x 128 blocks.
//   attn_stats_kernel      per query row: lse = log2 sum_j exp(scale q.k_j) over ALL keys, delta = dO . O (O: the forward output)
//   attn_bwd_long_kernel   one workgroup per (sequence, head, key block): P = exp(scale S - lse) needs no row reduction any
//                          more; dK / dV of the block accumulate in registers over the query blocks; key block 0 writes its dQ
//                          share to dq, every other block to a slab of its own
//   attn_dq_reduce_kernel  adds the slabs to dq in block order (no atomics: bitwise reproducible)
// Eight waves, 16 rows each, as in token_attn_bwd_kernel.
// ---------------------------------------------------------------------------------------------------
constexpr int LB = 128;          // block edge

__device__ __forceinline__ void stage_rows(float* dst, const float* src, long ld, long row0, int rows_valid, int col0, int cols_valid,
                                           int tid) {
    // dst[r][c] (pitch AB_LD), r < 128, c < 32  <-  src[(row0 + r) * ld + col0 + c], zero outside the valid rows / columns
    for (int e = tid; e < LB * 32; e += 512) {
        const int r = e >> 5, c = e & 31;
        dst[r * AB_LD + c] = (r < rows_valid && c < cols_valid) ? src[(row0 + r) * ld + col0 + c] : 0.f;
    }
}

// dst: three bf16 images [128][SPLIT_PITCH] (split_mfma.h) of src rows row0 .. row0 + 127, columns col0 .. col0 + 31 (zero outside the
// valid rows / columns): the operand of the split-product Q K^T / dO V^T of the blocked kernels
__device__ __forceinline__ void stage_rows_split(unsigned short* dst, const float* src, long ld, long row0, int rows_valid, int col0,
                                                 int cols_valid, int tid) {
    for (int e = tid; e < LB * 16; e += 512) {
        const int r = e >> 4, c = (e & 15) * 2;
        const float* const p = src + (row0 + r) * ld + col0 + c;
        const float a = (r < rows_valid && c < cols_valid) ? p[0] : 0.f, b = (r < rows_valid && c + 1 < cols_valid) ? p[1] : 0.f;
        lime_dev::split_store2(dst, LB * lime_dev::SPLIT_PITCH, r, c, a, b);
    }
}

// SPX: the scores on the bf16 matrix cores as split products (K staged as three bf16 images, the wave's Q rows split in registers:
// six 16x16x32 MFMAs per 16 x 16 tile instead of eight 16x16x4 fp32 ones -- 96 cycles against 256)
template <bool SPX>
__global__ __launch_bounds__(512) void attn_stats_kernel(const float* __restrict__ q, const float* __restrict__ k, long ld,
                                                          const float* __restrict__ out, long ldout, const float* __restrict__ dout,
                                                          long ldo, float* __restrict__ stats, int S, int n_head, int head_dim,
                                                          int head_stride, float scale, int n_blk) {
    __shared__ float Qs[LB * AB_LD];
    __shared__ __attribute__((aligned(16))) float Ks[SPX ? (3 * LB * lime_dev::SPLIT_PITCH) / 2 : LB * AB_LD];
    unsigned short* const Kt = reinterpret_cast<unsigned short*>(Ks);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, kg = lane >> 4;
    const int qb = blockIdx.x % n_blk;
    const long prob = blockIdx.x / n_blk;
    const int seq = (int)(prob / n_head), head = (int)(prob % n_head);
    const long row_base = (long)seq * S;
    const int q0 = qb * LB, q_valid = min(LB, S - q0);
    stage_rows(Qs, q, ld, row_base + q0, q_valid, head * head_stride, head_dim, tid);
    __syncthreads();
    const int R0 = 16 * wave;
    f32x4 qa[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) qa[h] = *reinterpret_cast<const f32x4*>(&Qs[(R0 + fi) * AB_LD + 8 * kg + 4 * h]);
    lime_dev::SplitFrag qs;
    if constexpr (SPX) {
        const float x[8] = {qa[0][0], qa[0][1], qa[0][2], qa[0][3], qa[1][0], qa[1][1], qa[1][2], qa[1][3]};
        qs = lime_dev::split_frag(x);
    }
    float m[4], l[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
    for (int kb = 0; kb < n_blk; ++kb) {
        const int k0 = kb * LB, k_valid = min(LB, S - k0);
        __syncthreads();
        if constexpr (SPX) stage_rows_split(Kt, k, ld, row_base + k0, k_valid, head * head_stride, head_dim, tid);
        else stage_rows(Ks, k, ld, row_base + k0, k_valid, head * head_stride, head_dim, tid);
        __syncthreads();
        f32x4 sc[LB / 16];
#pragma unroll
        for (int ct = 0; ct < LB / 16; ++ct) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if constexpr (SPX) {
                a = lime_dev::split_mfma16(qs, lime_dev::split_load(Kt, LB * lime_dev::SPLIT_PITCH, 16 * ct + fi, kg), a);
            } else {
                f32x4 kf[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) kf[h] = *reinterpret_cast<const f32x4*>(&Ks[(16 * ct + fi) * AB_LD + 8 * kg + 4 * h]);
#pragma unroll
                for (int t = 0; t < 8; ++t) a = mfma16(qa[t >> 2][t & 3], kf[t >> 2][t & 3], a);
            }
            sc[ct] = a;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = -INFINITY;
#pragma unroll
            for (int ct = 0; ct < LB / 16; ++ct) {
                const float sv = (16 * ct + fi < k_valid) ? sc[ct][r] * (scale * LOG2E) : -INFINITY;
                sc[ct][r] = sv;
                mx = fmaxf(mx, sv);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2));
            mx = fmaxf(mx, __shfl_xor(mx, 4)); mx = fmaxf(mx, __shfl_xor(mx, 8));
            const float mn = fmaxf(m[r], mx);
            float sum = 0.f;
#pragma unroll
            for (int ct = 0; ct < LB / 16; ++ct) sum += __builtin_amdgcn_exp2f(sc[ct][r] - mn);
            sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4); sum += __shfl_xor(sum, 8);
            l[r] = l[r] * __builtin_amdgcn_exp2f(m[r] - mn) + sum;
            m[r] = mn;
        }
    }
    // lse of this wave's rows 4 kg + r (the 16 lanes of a kg group hold the same value), delta by one thread per row
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = R0 + 4 * kg + r;
        if (fi == 0 && row < q_valid) stats[((row_base + q0 + row) * n_head + head) * 2] = m[r] + log2f(l[r]);   // log2 domain
    }
    if (tid < q_valid && out != nullptr) {
        const float* po = out + (row_base + q0 + tid) * ldout + (long)head * head_dim;
        const float* pd = dout + (row_base + q0 + tid) * ldo + (long)head * head_dim;
        float d = 0.f;
        for (int c = 0; c < head_dim; ++c) d += po[c] * pd[c];
        stats[((row_base + q0 + tid) * n_head + head) * 2 + 1] = d;
    }
}

// Training-mode forward for 128 < S <= 512 with probability dropout: row statistics first (attn_stats_kernel), then one
// workgroup per (sequence, head, query block) walks the key blocks: out = sum_blocks (keep * exp2(s' - lse) / (1 - p)) V.
__global__ __launch_bounds__(512) void attn_fwd_long_dropout_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                     const float* __restrict__ v, long ld, const float* __restrict__ stats,
                                                                     float* __restrict__ out, long ldo, int S, int n_head, int head_dim,
                                                                     int head_stride, float scale, int n_blk, LimeDropout drop) {
    constexpr int NT = LB / 16, LDP = LB + 2;
    extern __shared__ float smem[];
    float* Qs = smem;
    float* Ks = Qs + LB * AB_LD;
    float* Vs = Ks + LB * AB_LD;
    float* Ps = Vs + LB * AB_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, kg = lane >> 4;
    const int qb = blockIdx.x % n_blk;
    const long prob = blockIdx.x / n_blk;
    const int seq = (int)(prob / n_head), head = (int)(prob % n_head);
    const long row_base = (long)seq * S;
    const int q0 = qb * LB, q_valid = min(LB, S - q0);
    const int R0 = 16 * wave;
    stage_rows(Qs, q, ld, row_base + q0, q_valid, head * head_stride, head_dim, tid);
    __syncthreads();
    f32x4 qa[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) qa[h] = *reinterpret_cast<const f32x4*>(&Qs[(R0 + fi) * AB_LD + 8 * kg + 4 * h]);
    float lse[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = R0 + 4 * kg + r;
        lse[r] = row < q_valid ? stats[((row_base + q0 + row) * n_head + head) * 2] : INFINITY;
    }
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
    for (int kb = 0; kb < n_blk; ++kb) {
        const int k0 = kb * LB, k_valid = min(LB, S - k0);
        __syncthreads();
        stage_rows(Ks, k, ld, row_base + k0, k_valid, head * head_stride, head_dim, tid);
        stage_rows(Vs, v, ld, row_base + k0, k_valid, head * head_stride, head_dim, tid);
        __syncthreads();
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            f32x4 kf[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) kf[h] = *reinterpret_cast<const f32x4*>(&Ks[(16 * ct + fi) * AB_LD + 8 * kg + 4 * h]);
#pragma unroll
            for (int t = 0; t < 8; ++t) a = mfma16(qa[t >> 2][t & 3], kf[t >> 2][t & 3], a);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t idx = ((uint64_t)prob * S + (uint64_t)(q0 + R0 + 4 * kg + r)) * (uint64_t)S + (uint64_t)(k0 + 16 * ct + fi);
                const float pv = (16 * ct + fi < k_valid) ? __builtin_amdgcn_exp2f(a[r] * (scale * LOG2E) - lse[r]) : 0.f;
                const float f = (drop.thresh == 0 || lime_keep(drop, idx)) ? drop.scale : 0.f;
                Ps[(R0 + 4 * kg + r) * LDP + 16 * ct + fi] = pv * f;
            }
        }
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < LB / 4; ++t) {
            const int j = 4 * t + kg;
            const float a = Ps[(R0 + fi) * LDP + j];
            o0 = mfma16(a, Vs[j * AB_LD + fi], o0);
            o1 = mfma16(a, Vs[j * AB_LD + 16 + fi], o1);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = R0 + 4 * kg + r;
        if (row < q_valid) {
            float* o = out + (row_base + q0 + row) * ldo + (long)head * head_dim;
            if (fi < head_dim) o[fi] = o0[r];
            if (16 + fi < head_dim) o[16 + fi] = o1[r];
        }
    }
}

__global__ __launch_bounds__(512) void attn_bwd_long_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ v, long ld, const float* __restrict__ dout,
                                                             long ldo, const float* __restrict__ stats, float* __restrict__ dq,
                                                             float* __restrict__ dk, float* __restrict__ dv, long ldd, int S,
                                                             int n_head, int head_dim, int head_stride, float scale, int n_blk,
                                                             LimeDropout drop, float* __restrict__ dq_slabs, long n_tok) {
    constexpr int NT = LB / 16, LDP = LB + 2;
    extern __shared__ float smem[];
    float* Qs = smem;
    float* Ks = Qs + LB * AB_LD;
    float* Vs = Ks + LB * AB_LD;
    float* Os = Vs + LB * AB_LD;
    float* Ps = Os + LB * AB_LD;
    float* Ls = Ps + LB * LDP;                  // lse of the query block
    float* Ds = Ls + LB;                        // delta of the query block
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, kg = lane >> 4;
    const int kb = blockIdx.x % n_blk;
    const long prob = blockIdx.x / n_blk;
    const int seq = (int)(prob / n_head), head = (int)(prob % n_head);
    const long row_base = (long)seq * S;
    const int k0 = kb * LB, k_valid = min(LB, S - k0);
    const int R0 = 16 * wave;
    stage_rows(Ks, k, ld, row_base + k0, k_valid, head * head_stride, head_dim, tid);
    stage_rows(Vs, v, ld, row_base + k0, k_valid, head * head_stride, head_dim, tid);
    f32x4 av0 = {0.f, 0.f, 0.f, 0.f}, av1 = av0, ak0 = av0, ak1 = av0;
    for (int qb = 0; qb < n_blk; ++qb) {
        const int q0 = qb * LB, q_valid = min(LB, S - q0);
        __syncthreads();                        // the previous block's images are no longer read
        stage_rows(Qs, q, ld, row_base + q0, q_valid, head * head_stride, head_dim, tid);
        stage_rows(Os, dout, ldo, row_base + q0, q_valid, head * head_dim, head_dim, tid);
        if (tid < LB) {
            const bool ok = tid < q_valid;
            const float* st = stats + ((row_base + q0 + (ok ? tid : 0)) * n_head + head) * 2;
            Ls[tid] = ok ? st[0] : INFINITY;    // exp(x - inf) = 0: rows beyond S contribute nothing
            Ds[tid] = ok ? st[1] : 0.f;
        }
        __syncthreads();
        f32x4 p[NT], dp[NT];
        {
            f32x4 qa[2], oa[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                qa[h] = *reinterpret_cast<const f32x4*>(&Qs[(R0 + fi) * AB_LD + 8 * kg + 4 * h]);
                oa[h] = *reinterpret_cast<const f32x4*>(&Os[(R0 + fi) * AB_LD + 8 * kg + 4 * h]);
            }
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, d0 = s0;
                f32x4 kf[2], vf[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    kf[h] = *reinterpret_cast<const f32x4*>(&Ks[(16 * ct + fi) * AB_LD + 8 * kg + 4 * h]);
                    vf[h] = *reinterpret_cast<const f32x4*>(&Vs[(16 * ct + fi) * AB_LD + 8 * kg + 4 * h]);
                }
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    s0 = mfma16(qa[t >> 2][t & 3], kf[t >> 2][t & 3], s0);
                    d0 = mfma16(oa[t >> 2][t & 3], vf[t >> 2][t & 3], d0);
                }
                p[ct] = s0; dp[ct] = d0;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float lse = Ls[R0 + 4 * kg + r], dl = Ds[R0 + 4 * kg + r];
            const uint64_t mrow = ((uint64_t)prob * S + (uint64_t)(q0 + R0 + 4 * kg + r)) * (uint64_t)S + (uint64_t)k0;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const float pv = (16 * ct + fi < k_valid) ? __builtin_amdgcn_exp2f(p[ct][r] * (scale * LOG2E) - lse) : 0.f;
                // probability dropout: the forward multiplied keep / (1 - p) into P before the V product (delta = dO . O
                // already contains it)
                const float f = (drop.thresh == 0 || lime_keep(drop, mrow + (uint64_t)(16 * ct + fi))) ? drop.scale : 0.f;
                p[ct][r] = pv * f;                                   // what the dV product needs
                dp[ct][r] = scale * pv * (dp[ct][r] * f - dl);       // dS
            }
        }
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ps[(R0 + 4 * kg + r) * LDP + 16 * ct + fi] = p[ct][r];
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < LB / 4; ++t) {      // dV[j, d] += sum_i P[i, j] dO[i, d]
            const int i = 4 * t + kg;
            const float a = Ps[i * LDP + R0 + fi];
            av0 = mfma16(a, Os[i * AB_LD + fi], av0);
            av1 = mfma16(a, Os[i * AB_LD + 16 + fi], av1);
        }
        __syncthreads();
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) Ps[(R0 + 4 * kg + r) * LDP + 16 * ct + fi] = dp[ct][r];
        __syncthreads();
        f32x4 aq0 = {0.f, 0.f, 0.f, 0.f}, aq1 = aq0;
#pragma unroll 8
        for (int t = 0; t < LB / 4; ++t) {
            const int j = 4 * t + kg;
            const float ds_row = Ps[(R0 + fi) * LDP + j];
            aq0 = mfma16(ds_row, Ks[j * AB_LD + fi], aq0);
            aq1 = mfma16(ds_row, Ks[j * AB_LD + 16 + fi], aq1);
            const float ds_col = Ps[j * LDP + R0 + fi];
            ak0 = mfma16(ds_col, Qs[j * AB_LD + fi], ak0);
            ak1 = mfma16(ds_col, Qs[j * AB_LD + 16 + fi], ak1);
        }
        // this key block's share of dQ: key block 0 stores straight into dq, block kb > 0 into slab kb - 1 ([tokens][n_head * 32]);
        // attn_dq_reduce_kernel adds the slabs in block order -- no atomics, the result is bitwise reproducible
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = R0 + 4 * kg + r;
            if (row < q_valid) {
                float* d = kb == 0 ? dq + (row_base + q0 + row) * ldd + (long)head * head_stride
                                   : dq_slabs + ((long)(kb - 1) * n_tok + row_base + q0 + row) * ((long)n_head * 32) + (long)head * 32;
                if (fi < head_stride) d[fi] = aq0[r];
                if (16 + fi < head_stride) d[16 + fi] = aq1[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = R0 + 4 * kg + r;
        if (row < k_valid) {
            const long o = (row_base + k0 + row) * ldd + (long)head * head_stride;
            if (fi < head_stride) { dv[o + fi] = av0[r]; dk[o + fi] = ak0[r]; }
            if (16 + fi < head_stride) { dv[o + 16 + fi] = av1[r]; dk[o + 16 + fi] = ak1[r]; }
        }
    }
}

// The blocked backward with all five products as split products on the bf16 matrix cores (lime_set_split_gemm(1), the default;
// split_mfma.h: six 16x16x32 MFMAs per 16 x 16 x 32 block, 96 matrix cycles against the 256 of eight fp32 ones).  The key block's K and
// V are staged once, the query side goes in blocks of 64 rows; K, V, Q, dO are swizzled split images that serve row reads and transposed
// reads (split_mfma.h).  Wave w owns the keys 16 w .. 16 w + 15 of the block:
//   S = Q K^T and dP = dO V^T for its 16 keys x the 64 queries: result tiles with the KEY on the lane and the queries on the registers --
//   so P~ and dS are, as they stand (split in registers), the B operands of the two products that sum over the queries:
//   dV^T[d, j] += sum_i dO^T[d, i] P~[i, j],  dK^T[d, j] += sum_i Q^T[d, i] dS[i, j]   (dO^T / Q^T: ds_read_b64_tr_b16 block reads),
//   accumulated in registers over the query blocks, no P image, no barrier between the score products and these.
//   dQ sums over the keys -- the other orientation: dS goes through an fp32 image once ([query][key], 528-byte rows); wave w = query tile
//   w & 3 x head-dim half w >> 2 reads its queries' rows back as B operands (two ds_read_b128 per step, split in registers) against K^T
//   (transposed block reads of the K image): dQ^T[d, i] = sum_j K^T[d, j] dS^T[j, i].  Slabs per key block and the reduction order over
//   key blocks as before.
// FOUR-wave workgroups, TWO per CU (60 KB of LDS each): the phases of a query block are short and separated by barriers, so one lock-step
// workgroup per CU left the matrix pipe, the VALU and the LDS each 25-40 % busy one after the other (profiles/r03_attn_bwd_sp_counters.txt);
// two independent workgroups overlap them.  Wave w owns the keys 32 w .. 32 w + 31 (two 16-key tiles; their K and V fragments stay in
// registers for the whole key block, V never goes to LDS), the query side goes in blocks of 32 rows.  dS reaches the dQ product as a
// split image [key][query] (the producer writes the three terms it has split for dK anyway, four consecutive queries = 8 bytes per
// term), read back TRANSPOSED: no second split.  Three barriers per query block, 960 matrix cycles per wave and block (dV / dK / dQ on
// the fp32 MFMA: 3072).
constexpr int LQ = 32;
__global__ __launch_bounds__(256, 2) void attn_bwd_long_sp_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v, long ld, const float* __restrict__ dout,
                                                                   long ldo, const float* __restrict__ stats, float* __restrict__ dq,
                                                                   float* __restrict__ dk, float* __restrict__ dv, long ldd, int S,
                                                                   int n_head, int head_dim, int head_stride, float scale, int n_blk,
                                                                   LimeDropout drop, float* __restrict__ dq_slabs, long n_tok) {
    constexpr int KT = LB * SWZ_ROW, QT = LQ * SWZ_ROW;
    static_assert(LQ == SWZ_ROW, "the dS image has one row per key and LQ queries per row");
    extern __shared__ float smem[];
    unsigned short* const Kt = reinterpret_cast<unsigned short*>(smem);       // three swizzled bf16 images of the K block, [LB][32]
    unsigned short* const Di = Kt + 3 * KT;      // ... of dS^T: [LB keys][LQ queries]
    unsigned short* const Qi = Di + 3 * KT;      // ... of the query block's Q rows, [LQ][32]
    unsigned short* const Oi = Qi + 3 * QT;      // ... and of its dO rows
    float* const Ls = smem + 3 * KT + 3 * QT;    // (2 x 3 KT + 2 x 3 QT bf16)
    float* const Ds = Ls + LQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, kg = lane >> 4;
    const int kb = blockIdx.x % n_blk;
    const long prob = blockIdx.x / n_blk;
    const int seq = (int)(prob / n_head), head = (int)(prob % n_head);
    const long row_base = (long)seq * S;
    const int k0 = kb * LB, k_valid = min(LB, S - k0);
    const int R0 = 32 * wave, qi = wave & 1, hh = wave >> 1;
    for (int e = tid; e < LB * 16; e += 256) {      // K rows -> split images (zero outside the valid rows / columns)
        const int r = e >> 4, c = (e & 15) * 2;
        const bool ok0 = r < k_valid && c < head_dim, ok1 = r < k_valid && c + 1 < head_dim;
        const long g = (row_base + k0 + (r < k_valid ? r : 0)) * ld + head * head_stride + c;
        swz_store2(Kt, KT, r, c, ok0 ? k[g] : 0.f, ok1 ? k[g + 1] : 0.f);
    }
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 av[2][2] = {{z4, z4}, {z4, z4}}, ak[2][2] = {{z4, z4}, {z4, z4}};   // dV^T / dK^T of key tile u: [head dim 16 c + 4 kg + r][key R0 + 16 u + fi]
    const int n_qblk = (S + LQ - 1) / LQ;
    // the NEXT query block's Q / dO rows (two pairs each per thread) and statistics wait in registers while the current block is computed
    float pq[4], po[4], pl = INFINITY, pd = 0.f;
    auto fetch_q = [&](int qb) {
        const int q0 = qb * LQ, q_valid = min(LQ, S - q0);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + 256 * u, r = e >> 4, c = (e & 15) * 2;
            const bool ok0 = r < q_valid && c < head_dim, ok1 = r < q_valid && c + 1 < head_dim;
            const float* const qs = q + (row_base + q0 + (r < q_valid ? r : 0)) * ld + head * head_stride + c;
            const float* const os = dout + (row_base + q0 + (r < q_valid ? r : 0)) * ldo + head * head_dim + c;
            pq[2 * u] = ok0 ? qs[0] : 0.f; pq[2 * u + 1] = ok1 ? qs[1] : 0.f;
            po[2 * u] = ok0 ? os[0] : 0.f; po[2 * u + 1] = ok1 ? os[1] : 0.f;
        }
        if (tid < LQ) {
            const bool ok = tid < q_valid;
            const float* st = stats + ((row_base + q0 + (ok ? tid : 0)) * n_head + head) * 2;
            pl = ok ? st[0] : INFINITY;         // exp(x - inf) = 0: rows beyond S contribute nothing
            pd = ok ? st[1] : 0.f;
        }
    };
    fetch_q(0);
    // this wave's V rows straight from global memory into split fragments (lane: key R0 + 16 u + fi, head dims 8 kg .. 8 kg + 7)
    SplitFrag kB[2], vB[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int r = R0 + 16 * u + fi;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = 8 * kg + e;
            x[e] = (r < k_valid && c < head_dim) ? v[(row_base + k0 + r) * ld + head * head_stride + c] : 0.f;
        }
        vB[u] = split_frag(x);
    }
    __syncthreads();                            // the K image is complete
#pragma unroll
    for (int u = 0; u < 2; ++u) kB[u] = swz_row_load(Kt, KT, R0 + 16 * u + fi, kg);
    const float c2 = scale * LOG2E;
    for (int qb = 0; qb < n_qblk; ++qb) {
        const int q0 = qb * LQ, q_valid = min(LQ, S - q0);
        __syncthreads();                        // the previous block's images are no longer read
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int e = tid + 256 * u, r = e >> 4, c = (e & 15) * 2;
            swz_store2(Qi, QT, r, c, pq[2 * u], pq[2 * u + 1]);
            swz_store2(Oi, QT, r, c, po[2 * u], po[2 * u + 1]);
        }
        if (tid < LQ) { Ls[tid] = pl; Ds[tid] = pd; }
        __syncthreads();
        if (qb + 1 < n_qblk) fetch_q(qb + 1);
        // ---- S and dP of this wave's two key tiles x the two query tiles, then P~ and dS in place -----------------------------
        f32x4 p[2][2], dp[2][2];                // [key tile u][query tile t]: [query 16 t + 4 kg + r][key R0 + 16 u + fi]
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const SplitFrag qA = swz_row_load(Qi, QT, 16 * t + fi, kg), oA = swz_row_load(Oi, QT, 16 * t + fi, kg);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                p[u][t] = split_mfma16(qA, kB[u], z4);
                dp[u][t] = split_mfma16(oA, vB[u], z4);
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4 lse4 = *reinterpret_cast<const f32x4*>(Ls + 16 * t + 4 * kg);
            const f32x4 dl4 = *reinterpret_cast<const f32x4*>(Ds + 16 * t + 4 * kg);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int col = R0 + 16 * u + fi;
                const bool key_ok = col < k_valid;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * t + 4 * kg + r;
                    const float pv = key_ok ? __builtin_amdgcn_exp2f(__builtin_fmaf(p[u][t][r], c2, -lse4[r])) : 0.f;
                    float f = 1.f;
                    if (drop.thresh != 0)
                        f = lime_keep(drop, ((uint64_t)prob * S + (uint64_t)(q0 + row)) * (uint64_t)S + (uint64_t)(k0 + col)) ? drop.scale : 0.f;
                    p[u][t][r] = pv * f;                                    // what the dV product needs
                    dp[u][t][r] = scale * pv * (dp[u][t][r] * f - dl4[r]);  // dS
                }
            }
        }
        // ---- dV^T += dO^T P~: the result registers of the two query tiles are the eight k values of the B operand ---------------------
        {
            const SplitFrag o0 = swz_tr_load(Oi, QT, 0, 0, fi, kg), o1 = swz_tr_load(Oi, QT, 0, 1, fi, kg);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const SplitFrag bp = split_frag(p[u][0], p[u][1]);
                av[u][0] = split_mfma16(o0, bp, av[u][0]);
                av[u][1] = split_mfma16(o1, bp, av[u][1]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);      // (one pair of transposed fragments at a time: registers)
        // ---- dK^T += Q^T dS; the same three terms of dS go to the [key][query] image the dQ product reads (8 bytes per tile and term) ----
        {
            const SplitFrag q0f = swz_tr_load(Qi, QT, 0, 0, fi, kg), q1f = swz_tr_load(Qi, QT, 0, 1, fi, kg);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const SplitFrag bd = split_frag(dp[u][0], dp[u][1]);
                const u32x4 bh = __builtin_bit_cast(u32x4, bd.h), bm = __builtin_bit_cast(u32x4, bd.m), bl = __builtin_bit_cast(u32x4, bd.l);
#pragma unroll
                for (int t = 0; t < 2; ++t) {   // elements 4 t .. 4 t + 3 of the fragment: queries 16 t + 4 kg .. + 3 of key R0 + 16 u + fi
                    unsigned short* const d = Di + swz_off(R0 + 16 * u + fi, 16 * t + 4 * kg);
                    *reinterpret_cast<u32x2*>(d) = u32x2{bh[2 * t], bh[2 * t + 1]};
                    *reinterpret_cast<u32x2*>(d + KT) = u32x2{bm[2 * t], bm[2 * t + 1]};
                    *reinterpret_cast<u32x2*>(d + 2 * KT) = u32x2{bl[2 * t], bl[2 * t + 1]};
                }
                ak[u][0] = split_mfma16(q0f, bd, ak[u][0]);
                ak[u][1] = split_mfma16(q1f, bd, ak[u][1]);
            }
        }
        __syncthreads();                        // the dS image is complete
        // ---- this key block's share of dQ^T (head dims 16 hh .. 16 hh + 15 x query tile qi) = K^T dS^T: both operands by transposed
        // block reads, k values = keys 16 t0 + 4 kg + {0..3} and 16 (t0 + 1) + 4 kg + {0..3} ------------------------------------------
        f32x4 aq = z4;
#pragma unroll
        for (int s4 = 0; s4 < LB / 32; ++s4)
            aq = split_mfma16(swz_tr_load(Kt, KT, 2 * s4, hh, fi, kg), swz_tr_load(Di, KT, 2 * s4, qi, fi, kg), aq);
        {
            const int row = 16 * qi + fi;       // aq[r] = dQ[query row][head dim 16 hh + 4 kg + r]
            if (row < q_valid) {
                float* d = kb == 0 ? dq + (row_base + q0 + row) * ldd + (long)head * head_stride
                                   : dq_slabs + ((long)(kb - 1) * n_tok + row_base + q0 + row) * ((long)n_head * 32) + (long)head * 32;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (16 * hh + 4 * kg + r < head_stride) d[16 * hh + 4 * kg + r] = aq[r];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int col = R0 + 16 * u + fi;
        if (col < k_valid) {
            const long o = (row_base + k0 + col) * ldd + (long)head * head_stride;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d0 = 4 * kg + r;
                if (d0 < head_stride) { dv[o + d0] = av[u][0][r]; dk[o + d0] = ak[u][0][r]; }
                if (16 + d0 < head_stride) { dv[o + 16 + d0] = av[u][1][r]; dk[o + 16 + d0] = ak[u][1][r]; }
            }
        }
    }
}

// stats[(token, head)] = (lse from the forward, delta = dO . O): the statistics pass without its Q K^T products, for a forward that
// kept its log-sum-exp (the forward's lse form)
__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ out, long ldout, const float* __restrict__ dout, long ldo,
                                                          const float* __restrict__ lse, float* __restrict__ stats, long n_tok, int n_head,
                                                          int head_dim) {
    // one wave per token: coalesced row reads, the products parked in LDS, lane h sums head h's in column order (fixed order:
    // reproducible bits); n_head * head_dim <= 1024, n_head <= 64
    __shared__ float prod[4][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int width = n_head * head_dim;
    for (long row = (long)blockIdx.x * 4 + wave; row < n_tok; row += (long)gridDim.x * 4) {
        const float* po = out + row * ldout;
        const float* pd = dout + row * ldo;
        for (int c = lane; c < width; c += 64) prod[wave][c] = po[c] * pd[c];
        wave_lds_fence();
        if (lane < n_head) {
            float d = 0.f;
            for (int c = 0; c < head_dim; ++c) d += prod[wave][lane * head_dim + c];
            const long e = row * n_head + lane;
            stats[e * 2] = lse[e];
            stats[e * 2 + 1] = d;
        }
        wave_lds_fence();
    }
}

// dq[row, head * hs + j] += sum over slabs 0 .. n_slab - 1 (key blocks 1 ..) of slab[row][head * 32 + j], in slab order
__global__ __launch_bounds__(256) void attn_dq_reduce_kernel(float* __restrict__ dq, long ldd, const float* __restrict__ slabs, long n_tok,
                                                              int n_head, int hs, int n_slab) {
    const long total = n_tok * n_head * hs;
    const long wcols = (long)n_head * 32;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long row = e / (n_head * hs);
        const int c = (int)(e - row * (n_head * hs));
        const int head = c / hs, j = c - head * hs;
        float t = dq[row * ldd + c];
        for (int b = 0; b < n_slab; ++b) t += slabs[((long)b * n_tok + row) * wcols + head * 32 + j];
        dq[row * ldd + c] = t;
    }
}

template <int SP>
int launch_attn_bwd(const lime_token_attention_bwd_args& a, hipStream_t s) {
    constexpr int PPW = 8 / (SP / 16);
    constexpr int BYTES = PPW * (4 * SP * AB_LD + SP * (SP + 2)) * 4;
    static int reserved = 0;
    if (const int st = lime_reserve_lds((const void*)token_attn_bwd_kernel<SP>, BYTES, reserved, "lime_token_attention_bwd_f32")) return st;
    const long n_group = ((long)a.n_seq * a.n_head + PPW - 1) / PPW;
    const int grid = (int)lime_persistent_grid(n_group);                 // persistent: one workgroup per CU
    // vector staging: 32-float head rows on 16-byte boundaries with zero padding columns, dO pairs on 8-byte boundaries
    const bool vec = a.head_stride == 32 && lime_al16(a.q, a.ld_qkv) && lime_al16(a.k, a.ld_qkv) && lime_al16(a.v, a.ld_qkv) &&
                     a.head_dim % 2 == 0 && a.ldo % 2 == 0 && (((uintptr_t)a.dout) & 7) == 0;
    token_attn_bwd_kernel<SP><<<grid, 512, BYTES, s>>>(a.q, a.k, a.v, a.ld_qkv, a.dout, a.ldo, a.dq, a.dk, a.dv, a.ld_dqkv, a.n_seq, a.S,
                                                      a.n_head, a.head_dim, a.head_stride, a.scale, vec ? 1 : 0, lime_attn_bwd_dropout(a),
                                                      a.key_mask);
    return lime_check_launch("token_attn_bwd_kernel");
}

template <int SP>
int launch_attn_fwd_dropout(const float* q, const float* k, const float* v, long ld, float* out, long ldo, int n_seq, int S,
                            int n_head, int head_dim, int head_stride, float scale, const LimeDropout& drop, hipStream_t s) {
    constexpr int PPW = 8 / (SP / 16);
    constexpr int BYTES = PPW * (2 * SP * AB_LD) * 4;
    static int reserved = 0;
    if (const int st = lime_reserve_lds((const void*)token_attn_fwd_dropout_kernel<SP>, BYTES, reserved, "lime_token_attention_dropout_f32")) return st;
    const long n_group = ((long)n_seq * n_head + PPW - 1) / PPW;
    const bool vec = head_stride == 32 && lime_al16(q, ld) && lime_al16(k, ld) && lime_al16(v, ld);
    token_attn_fwd_dropout_kernel<SP><<<(unsigned)n_group, 512, BYTES, s>>>(q, k, v, ld, out, ldo, n_seq, S, n_head, head_dim, head_stride,
                                                                           scale, drop, vec ? 1 : 0);
    return lime_check_launch("token_attn_fwd_dropout_kernel");
}

// the row statistics of the blocked paths (out / dout NULL: the forward, lse only); spx: Q K^T as split products on the bf16 matrix cores
int launch_attn_stats(bool spx, const float* q, const float* k, long ld, const float* out, long ldout, const float* dout, long ldo,
                      float* stats, long n_prob, int S, int n_head, int head_dim, int head_stride, float scale, int n_blk, hipStream_t s) {
    const unsigned grid = (unsigned)(n_prob * n_blk);
    if (spx) attn_stats_kernel<true><<<grid, 512, 0, s>>>(q, k, ld, out, ldout, dout, ldo, stats, S, n_head, head_dim, head_stride, scale, n_blk);
    else attn_stats_kernel<false><<<grid, 512, 0, s>>>(q, k, ld, out, ldout, dout, ldo, stats, S, n_head, head_dim, head_stride, scale, n_blk);
    return lime_check_launch("attn_stats_kernel");
}

int launch_attn_dq_reduce(float* dq, long ldd, const float* slabs, long n_tok, int n_head, int hs, int n_slab, hipStream_t s) {
    attn_dq_reduce_kernel<<<lime_grid_cap(n_tok * n_head * hs, 256, 8192), 256, 0, s>>>(dq, ldd, slabs, n_tok, n_head, hs, n_slab);
    return lime_check_launch("attn_dq_reduce_kernel");
}
}  // namespace

extern "C" int64_t lime_token_attention_stats_workspace(int32_t n_seq, int32_t S, int32_t n_head) {
    return S > 128 ? (int64_t)n_seq * S * n_head * 2 : 0;            // lse and delta per (token, head) for the blocked paths
}

// the blocked backward (S > 128): the row statistics, then one [tokens][n_head * 32] slab per key block behind the first (their shares
// of dq, summed in block order)
LimeAttnBwdCarve lime_attn_bwd_carve(int n_seq, int S, int n_head) {
    const int n_blk = (S + LB - 1) / LB;
    const int64_t stats = lime_token_attention_stats_workspace(n_seq, S, n_head);
    return LimeAttnBwdCarve{n_blk, stats, stats + (n_blk - 1) * (int64_t)n_seq * S * n_head * 32};
}

extern "C" int64_t lime_token_attention_bwd_workspace(int32_t n_seq, int32_t S, int32_t n_head) {
    return S > 128 ? lime_attn_bwd_carve(n_seq, S, n_head).total : 0;
}

// The fp32 kernels of the backward at head_dim <= 32 (token_attn_f32.hip chose r and made the checks): the one-pass kernel's length
// bucket r.n, or the pass r.pass (row statistics, or delta alone) + the key-block kernel on the arithmetic of r.family + the sum of the
// key blocks' dq slabs.
int lime_attn_bwd_launch(const LimeAttnBwdRoute& r, const lime_token_attention_bwd_args& a, hipStream_t s) {
    if (r.family == LIME_BWD_ATTN_ONE_PASS) {
        switch (r.n) {
            case 32: return launch_attn_bwd<32>(a, s);
            case 64: return launch_attn_bwd<64>(a, s);
            case 128: return launch_attn_bwd<128>(a, s);
        }
        LIME_REQUIRE(false, LIME_ERR_UNSUPPORTED, "lime_token_attention_bwd_f32: token_attn_bwd_kernel<%d> is not built", r.n);
    }
    const LimeAttnBwdCarve w = lime_attn_bwd_carve(a.n_seq, a.S, a.n_head);
    float* const stats = a.workspace;
    float* const dq_slabs = a.workspace + w.stats;
    const long n_prob = (long)a.n_seq * a.n_head, n_tok = (long)a.n_seq * a.S;
    int st;
    if (r.pass == LIME_BWD_ATTN_PASS_DELTA) {                    // the forward kept its log-sum-exp: only delta = dO . O is left
        attn_delta_kernel<<<lime_grid_cap(n_tok, 4, 8192), 256, 0, s>>>(a.out, a.ld_out, a.dout, a.ldo, a.lse, stats, n_tok, a.n_head, a.head_dim);
        st = lime_check_launch("attn_delta_kernel");
    } else st = launch_attn_stats(r.pass == LIME_BWD_ATTN_PASS_STATS_SPLIT, a.q, a.k, a.ld_qkv, a.out, a.ld_out, a.dout, a.ldo, stats, n_prob,
                                  a.S, a.n_head, a.head_dim, a.head_stride, a.scale, w.n_blk, s);
    if (st != LIME_OK) return st;
    // the two blocked kernels take the same arguments; they differ in LDS bytes and workgroup size (two four-wave workgroups per CU
    // for the split product, one eight-wave workgroup for the fp32 MFMA)
    constexpr int BYTES = (4 * LB * AB_LD + LB * (LB + 2) + 2 * LB) * 4;
    constexpr int BYTES_SP = (3 * LB * lime_dev::SWZ_ROW + 3 * LQ * lime_dev::SWZ_ROW + 2 * LQ) * 4;
    static_assert(2 * BYTES_SP <= 163840, "LDS budget: two workgroups per CU");
    static int reserved[2] = {0, 0};
    const bool spx = r.family == LIME_BWD_ATTN_LONG_SP;          // Q K^T / dO V^T as split products on the bf16 matrix cores
    const auto kernel = spx ? attn_bwd_long_sp_kernel : attn_bwd_long_kernel;
    const int bytes = spx ? BYTES_SP : BYTES;
    st = lime_reserve_lds((const void*)kernel, bytes, reserved[spx], "lime_token_attention_bwd_f32");
    if (st != LIME_OK) return st;
    kernel<<<(unsigned)(n_prob * w.n_blk), spx ? 256 : 512, bytes, s>>>(a.q, a.k, a.v, a.ld_qkv, a.dout, a.ldo, stats, a.dq, a.dk, a.dv, a.ld_dqkv,
                                                                     a.S, a.n_head, a.head_dim, a.head_stride, a.scale, w.n_blk,
                                                                     lime_attn_bwd_dropout(a), dq_slabs, n_tok);
    st = lime_check_launch(spx ? "attn_bwd_long_sp_kernel" : "attn_bwd_long_kernel");
    if (st != LIME_OK || !r.reduce) return st;
    return launch_attn_dq_reduce(a.dq, a.ld_dqkv, dq_slabs, n_tok, a.n_head, a.head_stride, w.n_blk - 1, s);
}

// The fp32 kernels of the dropout forward (token_attn_f32.hip chose r and made the checks): the one-pass kernel's length bucket
// r.n, or the row statistics (r.stats: on which arithmetic) + the key-block kernel.
int lime_attn_dropout_launch(const LimeAttnRoute& r, const lime_token_attention_args& a, hipStream_t s) {
    const LimeDropout drop = lime_attn_dropout(a);
    if (r.family == LIME_ATTN_DROPOUT) {
        switch (r.n) {
            case 32: return launch_attn_fwd_dropout<32>(a.q, a.k, a.v, a.ld_qkv, a.out, a.ldo, a.n_seq, a.S, a.n_head, a.head_dim, a.head_stride, a.scale, drop, s);
            case 64: return launch_attn_fwd_dropout<64>(a.q, a.k, a.v, a.ld_qkv, a.out, a.ldo, a.n_seq, a.S, a.n_head, a.head_dim, a.head_stride, a.scale, drop, s);
            case 128: return launch_attn_fwd_dropout<128>(a.q, a.k, a.v, a.ld_qkv, a.out, a.ldo, a.n_seq, a.S, a.n_head, a.head_dim, a.head_stride, a.scale, drop, s);
        }
        LIME_REQUIRE(false, LIME_ERR_UNSUPPORTED, "lime_token_attention_dropout_f32: token_attn_fwd_dropout_kernel<%d> is not built", r.n);
    }
    const int n_blk = (a.S + LB - 1) / LB;
    const long n_prob = (long)a.n_seq * a.n_head;
    int st = launch_attn_stats(r.stats == LIME_ATTN_STATS_SPLIT, a.q, a.k, a.ld_qkv, nullptr, 0, nullptr, 0, a.workspace, n_prob, a.S, a.n_head,
                               a.head_dim, a.head_stride, a.scale, n_blk, s);
    if (st != LIME_OK) return st;
    constexpr int BYTES = (3 * LB * AB_LD + LB * (LB + 2)) * 4;
    static int reserved = 0;
    st = lime_reserve_lds((const void*)attn_fwd_long_dropout_kernel, BYTES, reserved, "lime_token_attention_dropout_f32");
    if (st != LIME_OK) return st;
    attn_fwd_long_dropout_kernel<<<(unsigned)(n_prob * n_blk), 512, BYTES, s>>>(a.q, a.k, a.v, a.ld_qkv, a.workspace, a.out, a.ldo, a.S, a.n_head,
                                                                               a.head_dim, a.head_stride, a.scale, n_blk, drop);
    return lime_check_launch("attn_fwd_long_dropout_kernel");
}
