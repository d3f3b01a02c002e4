// Token attention for heads wider than 32 columns (32 < head_dim <= 128, head_dim % 4 == 0, S <= 512): the reference's head_num 3 and 5
// (300 / 3 = 100, 300 / 5 = 60 columns per head, config.py:72) and layers.MultiHeadAttention with head_dim > 32.  Forward
// softmax(scale Q K^T [key mask]) V with optional log-sum-exp output, device-side sequence count and probability dropout, and the
// backward (dQ / dK / dV).  Every product is v_mfma_f32_16x16x4_f32 (exact fp32); lime_set_split_gemm has no effect here.
//
// One shape serves all three kernels.  A four-wave workgroup OWNS 64 rows of one (sequence, head) -- 16 per wave, one per lane & 15 --
// whose operand rows sit in registers as MFMA B fragments, and STREAMS the other side through LDS in blocks of 64 rows:
//   tile   = Y X^T    16 streamed rows x the wave's 16 own rows; lane (fi, kg) holds streamed rows 16 ct + 4 kg + 0..3 of own row fi,
//                     which is, as it stands, the B operand of
//   acc^T += Y^T tile the products that sum over the streamed rows (the own row stays on the lane: acc[dt][r] = column 16 dt + 4 kg + r).
//   wide_fwd_kernel     owns queries, streams K / V:  S^T = K Q^T, running-maximum softmax over the key blocks, O^T += V^T P^T
//   wide_bwd_q_kernel   owns queries, streams K / V twice: pass 1 S^T and dP^T = V dO^T -> max, 1 / sum and delta = sum_j P~ dP per query (written
//                       to the workspace); pass 2 the same tiles -> dS^T -> dQ^T += K^T dS^T
//   wide_bwd_kv_kernel  owns keys, streams Q / dO and the queries' statistics:  S = Q K^T, dP = dO V^T -> P~, dS -> dV^T += dO^T P~,
//                       dK^T += Q^T dS
// Every sum runs in a fixed order inside one workgroup -- no atomics, no slabs: two runs agree bitwise.  The price is that the score and
// dP tiles are computed three times in the backward (nine products instead of the seven of a slab design).
// The head dimension is padded to a multiple of 16 in LDS / registers only (zeros); columns from head_dim on are never read from memory.
// Every wait is a __syncthreads().
#include "dev_helpers.h"
#include "dropout.h"
#include "gemm_pp.h"
#include "token_attn.h"

using namespace lime_dev;

namespace {

constexpr int WB = 64;                             // rows per block: own rows of a workgroup, streamed rows of an LDS image

// NK: 16-column steps of the padded head dimension (3 .. 8).  Pitch of an LDS row: a multiple of 32 floats + 4, so the ds_read_b128 of
// 16 consecutive rows (tile product) and the ds_read_b32 of 16 consecutive columns (accumulating product) spread over the banks.
template <int NK>
struct WideGeom {
    static constexpr int HDP = 16 * NK;
    static constexpr int LD = ((HDP + 31) / 32) * 32 + 4;
    static constexpr int IMAGE = WB * LD;          // floats of one 64-row image
};

struct WideP {
    const float* q; const float* k; const float* v; long ld;
    const unsigned char* mask;                     // [n_seq, S], 0 = masked key, or NULL
    const int* n_seq_dev;                          // forward: optional device-side sequence count
    float* out; long ldo;                          // forward
    float* lse;                                    // forward, optional [tokens, n_head]
    const float* dout; long ldg;                   // backward: dO [tokens, n_head * head_dim]
    float* dq; float* dk; float* dv; long ldd;     // backward
    float* stats;                                  // backward workspace [tokens, n_head, 3]: row maximum (log2 domain), 1 / sum, delta
    int S, n_head, hd, hs, n_blk;
    float scale;
    LimeDropout drop;
};

// rows row0 .. row0 + 63 of one head (src points at its first column) -> dst[64][LD]; zeros beyond rows_valid and from column hd on
template <int NK>
__device__ __forceinline__ void stage_wide(float* dst, const float* src, long ld, long row0, int rows_valid, int hd, int tid) {
    constexpr int C4 = 4 * NK, LD = WideGeom<NK>::LD;
    for (int e = tid; e < WB * C4; e += 256) {
        const int r = e / C4, c = (e - r * C4) * 4;
        f32x4 val = {0.f, 0.f, 0.f, 0.f};
        if (r < rows_valid && c < hd) val = *reinterpret_cast<const f32x4*>(src + (row0 + r) * ld + c);
        *reinterpret_cast<f32x4*>(&dst[r * LD + c]) = val;
    }
}

// the lane's own row as B fragments: x[s4] = row[16 s4 + 4 kg .. + 3] times `mul` (row NULL: the row does not exist, zeros)
template <int NK>
__device__ __forceinline__ void own_row(f32x4 (&x)[NK], const float* row, int hd, int kg, float mul) {
#pragma unroll
    for (int s4 = 0; s4 < NK; ++s4) {
        const int c = 16 * s4 + 4 * kg;
        f32x4 val = {0.f, 0.f, 0.f, 0.f};
        if (row != nullptr && c < hd) val = *reinterpret_cast<const f32x4*>(row + c);
        x[s4] = val * mul;
    }
}

// tile[r] = sum_d Y[16 ct + 4 kg + r][d] x_own[d].  The summation index is only a label: lane group kg takes d = 16 s4 + 4 kg + u, so
// its operands of four MFMA steps are one ds_read_b128.
template <int NK>
__device__ __forceinline__ f32x4 tile_product(const float* Y, int ct, const f32x4 (&x)[NK], int fi, int kg) {
    constexpr int LD = WideGeom<NK>::LD;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s4 = 0; s4 < NK; ++s4) {
        const f32x4 yf = *reinterpret_cast<const f32x4*>(&Y[(16 * ct + fi) * LD + 16 * s4 + 4 * kg]);
#pragma unroll
        for (int u = 0; u < 4; ++u) a = mfma16(yf[u], x[s4][u], a);
    }
    return a;
}

// acc[dt][r] (column 16 dt + 4 kg + r of the lane's own row) += sum over the tile's streamed rows of Y[row][column] * tile[row]
template <int NK>
__device__ __forceinline__ void acc_product(f32x4 (&acc)[NK], const float* Y, int ct, const f32x4& t, int fi, int kg) {
    constexpr int LD = WideGeom<NK>::LD;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float* yrow = &Y[(16 * ct + 4 * kg + u) * LD + fi];
#pragma unroll
        for (int dt = 0; dt < NK; ++dt) acc[dt] = mfma16(yrow[16 * dt], t[u], acc[dt]);
    }
}

// the lane's own row of a result: columns < hd from acc (times mul), zeros from hd to hs
template <int NK>
__device__ __forceinline__ void store_own(float* row, const f32x4 (&acc)[NK], int hd, int hs, int kg, float mul) {
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) {
        const int c = 16 * dt + 4 * kg;
        if (c < hd) *reinterpret_cast<f32x4*>(row + c) = acc[dt] * mul;
    }
    for (int c = hd + 4 * kg; c < hs; c += 16) *reinterpret_cast<f32x4*>(row + c) = f32x4{0.f, 0.f, 0.f, 0.f};
}

// keep bits of the four consecutive mask elements idx .. idx + 3 (one hash when they share a group of four)
__device__ __forceinline__ unsigned keep_row4(const LimeDropout& d, uint64_t idx) {
    if ((idx & 3) == 0) return lime_keep4(d, idx >> 2);
    unsigned m = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) m |= (lime_keep(d, idx + r) ? 1u : 0u) << r;
    return m;
}

__device__ __forceinline__ float quad_max(float v) {         // over the four kg partners of a lane (lanes +-16, +-32)
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

// scores of one key block for the lane's query, in place: -inf beyond S, the -1e9 fill on masked keys (layers.py:233); returns their max
__device__ __forceinline__ float mask_scores(f32x4 (&sc)[4], const unsigned char* km, int k0, int S, int kg) {
    float mc = -INFINITY;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = k0 + 16 * ct + 4 * kg + r;
            float s = sc[ct][r];
            if (j >= S) s = -INFINITY;
            else if (km != nullptr && km[j] == 0) s = -1e9f * LOG2E;
            sc[ct][r] = s;
            mc = fmaxf(mc, s);
        }
    return mc;
}

template <int NK>
__global__ __launch_bounds__(256) void wide_fwd_kernel(const WideP p) {
    constexpr int IMAGE = WideGeom<NK>::IMAGE;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;
    float* Vs = smem + IMAGE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, kg = lane >> 4;
    const int qb = blockIdx.x % p.n_blk;
    const long prob = blockIdx.x / p.n_blk;
    const int seq = (int)(prob / p.n_head), head = (int)(prob % p.n_head);
    if (p.n_seq_dev != nullptr && seq >= __builtin_amdgcn_readfirstlane(*p.n_seq_dev)) return;     // uniform over the workgroup
    const int S = p.S, hd = p.hd;
    const long row_base = (long)seq * S, col0 = (long)head * p.hs;
    const int qi = qb * WB + 16 * wave + fi;                 // this lane's query
    const bool q_ok = qi < S;
    f32x4 qf[NK];
    own_row<NK>(qf, q_ok ? p.q + (row_base + qi) * p.ld + col0 : nullptr, hd, kg, p.scale * LOG2E);   // scores in the log2 domain
    const unsigned char* km = p.mask != nullptr ? p.mask + row_base : nullptr;
    const uint64_t mrow = ((uint64_t)prob * S + (uint64_t)qi) * (uint64_t)S;
    f32x4 o[NK];
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;                            // l: this lane's share of the sum (its kg partners hold the rest)
    for (int kb = 0; kb < p.n_blk; ++kb) {
        const int k0 = kb * WB, k_valid = min(WB, S - k0);
        __syncthreads();                                     // the previous block's images are no longer read
        stage_wide<NK>(Ks, p.k + col0, p.ld, row_base + k0, k_valid, hd, tid);
        stage_wide<NK>(Vs, p.v + col0, p.ld, row_base + k0, k_valid, hd, tid);
        __syncthreads();
        f32x4 sc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) sc[ct] = tile_product<NK>(Ks, ct, qf, fi, kg);
        const float m_new = fmaxf(m, quad_max(mask_scores(sc, km, k0, S, kg)));    // finite from the first block on: key 0 exists
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);                     // 0 on the first block, 1 while the maximum stands
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < NK; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            unsigned keep = 0xFu;
            if (p.drop.thresh != 0) keep = keep_row4(p.drop, mrow + (uint64_t)(k0 + 16 * ct + 4 * kg));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(sc[ct][r] - m_new);
                l += e;
                sc[ct][r] = (keep >> r) & 1u ? e : 0.f;
            }
            acc_product<NK>(o, Vs, ct, sc[ct], fi, kg);
        }
        m = m_new;
    }
    l = quad_sum(l);
    if (q_ok) {
        if (p.lse != nullptr && kg == 0) p.lse[(row_base + qi) * p.n_head + head] = m + log2f(l);
        store_own<NK>(p.out + (row_base + qi) * p.ldo + (long)head * hd, o, hd, hd, kg, p.drop.scale / l);
    }
}

// dropout factor on P for the four keys of a tile register group (consecutive mask elements)
__device__ __forceinline__ f32x4 keep_factor4(const LimeDropout& d, uint64_t idx) {
    f32x4 f = {1.f, 1.f, 1.f, 1.f};
    if (d.thresh != 0) {
        const unsigned keep = keep_row4(d, idx);
#pragma unroll
        for (int r = 0; r < 4; ++r) f[r] = (keep >> r) & 1u ? d.scale : 0.f;
    }
    return f;
}

template <int NK>
__global__ __launch_bounds__(256) void wide_bwd_q_kernel(const WideP p) {
    constexpr int IMAGE = WideGeom<NK>::IMAGE;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;
    float* Vs = smem + IMAGE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, kg = lane >> 4;
    const int qb = blockIdx.x % p.n_blk;
    const long prob = blockIdx.x / p.n_blk;
    const int seq = (int)(prob / p.n_head), head = (int)(prob % p.n_head);
    const int S = p.S, hd = p.hd;
    const long row_base = (long)seq * S, col0 = (long)head * p.hs;
    const int qi = qb * WB + 16 * wave + fi;
    const bool q_ok = qi < S;
    f32x4 qf[NK], gf[NK];                                    // the lane's Q row (log2-domain scale folded in) and dO row
    own_row<NK>(qf, q_ok ? p.q + (row_base + qi) * p.ld + col0 : nullptr, hd, kg, p.scale * LOG2E);
    own_row<NK>(gf, q_ok ? p.dout + (row_base + qi) * p.ldg + (long)head * hd : nullptr, hd, kg, 1.0f);
    const unsigned char* km = p.mask != nullptr ? p.mask + row_base : nullptr;
    const uint64_t mrow = ((uint64_t)prob * S + (uint64_t)qi) * (uint64_t)S;
    // ---- pass 1: m = max_j s_j, l = sum_j 2^(s_j - m) and delta = sum_j P~_j dP_j (P~ = keep P / (1 - p): what the forward multiplied into V) --------
    float m = -INFINITY, l = 0.f, dl = 0.f;
    for (int kb = 0; kb < p.n_blk; ++kb) {
        const int k0 = kb * WB, k_valid = min(WB, S - k0);
        __syncthreads();
        stage_wide<NK>(Ks, p.k + col0, p.ld, row_base + k0, k_valid, hd, tid);
        stage_wide<NK>(Vs, p.v + col0, p.ld, row_base + k0, k_valid, hd, tid);
        __syncthreads();
        f32x4 sc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) sc[ct] = tile_product<NK>(Ks, ct, qf, fi, kg);
        const float m_new = fmaxf(m, quad_max(mask_scores(sc, km, k0, S, kg)));
        const float alpha = __builtin_amdgcn_exp2f(m - m_new);
        l *= alpha;
        dl *= alpha;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const f32x4 dp = tile_product<NK>(Vs, ct, gf, fi, kg);
            const f32x4 f = keep_factor4(p.drop, mrow + (uint64_t)(k0 + 16 * ct + 4 * kg));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(sc[ct][r] - m_new);
                l += e;
                dl += e * f[r] * dp[r];
            }
        }
        m = m_new;
    }
    // the maximum and the sum stay apart: under a key mask that covers a whole sequence the maximum is the -1e9 fill, and
    // max + log2(sum) would round the sum away (P = exp2(s - max) / sum is exact there: uniform weights)
    const float inv_l = 1.0f / quad_sum(l);
    const float delta = quad_sum(dl) * inv_l;
    if (q_ok && kg == 0) {
        float* st = p.stats + ((row_base + qi) * p.n_head + head) * 3;
        st[0] = m;
        st[1] = inv_l;
        st[2] = delta;
    }
    // ---- pass 2: dS^T = scale P (keep dP / (1 - p) - delta), zero on masked keys (their scores are constants); dQ^T += K^T dS^T -------
    f32x4 dq[NK];
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < p.n_blk; ++kb) {
        const int k0 = kb * WB, k_valid = min(WB, S - k0);
        if (p.n_blk > 1) {                                   // a single block is still staged
            __syncthreads();
            stage_wide<NK>(Ks, p.k + col0, p.ld, row_base + k0, k_valid, hd, tid);
            stage_wide<NK>(Vs, p.v + col0, p.ld, row_base + k0, k_valid, hd, tid);
            __syncthreads();
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const f32x4 sc = tile_product<NK>(Ks, ct, qf, fi, kg);
            const f32x4 dp = tile_product<NK>(Vs, ct, gf, fi, kg);
            const f32x4 f = keep_factor4(p.drop, mrow + (uint64_t)(k0 + 16 * ct + 4 * kg));
            f32x4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = k0 + 16 * ct + 4 * kg + r;
                const bool live = j < S && !(km != nullptr && km[j < S ? j : 0] == 0);
                ds[r] = live ? p.scale * (__builtin_amdgcn_exp2f(sc[r] - m) * inv_l) * (f[r] * dp[r] - delta) : 0.f;
            }
            acc_product<NK>(dq, Ks, ct, ds, fi, kg);
        }
    }
    if (q_ok) store_own<NK>(p.dq + (row_base + qi) * p.ldd + col0, dq, hd, p.hs, kg, 1.0f);
}

template <int NK>
__global__ __launch_bounds__(256) void wide_bwd_kv_kernel(const WideP p) {
    constexpr int IMAGE = WideGeom<NK>::IMAGE;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;
    float* Gs = smem + IMAGE;                                // dO
    float* Ms = smem + 2 * IMAGE;                            // row maximum, 1 / sum and delta of the query block
    float* Ls = Ms + WB;
    float* Ds = Ls + WB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fi = lane & 15, kg = lane >> 4;
    const int kb = blockIdx.x % p.n_blk;
    const long prob = blockIdx.x / p.n_blk;
    const int seq = (int)(prob / p.n_head), head = (int)(prob % p.n_head);
    const int S = p.S, hd = p.hd;
    const long row_base = (long)seq * S, col0 = (long)head * p.hs;
    const int kj = kb * WB + 16 * wave + fi;                 // this lane's key
    const bool k_ok = kj < S;
    f32x4 kf[NK], vf[NK];
    own_row<NK>(kf, k_ok ? p.k + (row_base + kj) * p.ld + col0 : nullptr, hd, kg, p.scale * LOG2E);
    own_row<NK>(vf, k_ok ? p.v + (row_base + kj) * p.ld + col0 : nullptr, hd, kg, 1.0f);
    const bool kmasked = p.mask != nullptr && k_ok && p.mask[row_base + kj] == 0;
    f32x4 dk[NK], dv[NK];
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = dk[dt]; }
    for (int qb = 0; qb < p.n_blk; ++qb) {                   // query blocks in order: a fixed summation order
        const int q0 = qb * WB, q_valid = min(WB, S - q0);
        __syncthreads();
        stage_wide<NK>(Qs, p.q + col0, p.ld, row_base + q0, q_valid, hd, tid);
        stage_wide<NK>(Gs, p.dout + (long)head * hd, p.ldg, row_base + q0, q_valid, hd, tid);
        if (tid < WB) {
            const bool ok = tid < q_valid;
            const float* st = p.stats + ((row_base + q0 + (ok ? tid : 0)) * p.n_head + head) * 3;
            Ms[tid] = ok ? st[0] : 0.f;
            Ls[tid] = ok ? st[1] : 0.f;                      // rows beyond S contribute nothing
            Ds[tid] = ok ? st[2] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const f32x4 sc = tile_product<NK>(Qs, ct, kf, fi, kg);       // S[query 16 ct + 4 kg + r][this lane's key]
            const f32x4 dp = tile_product<NK>(Gs, ct, vf, fi, kg);
            f32x4 pd, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = 16 * ct + 4 * kg + r;
                const float s = kmasked ? -1e9f * LOG2E : sc[r];
                const float pv = k_ok ? __builtin_amdgcn_exp2f(s - Ms[il]) * Ls[il] : 0.f;
                float f = 1.f;
                if (p.drop.thresh != 0)
                    f = lime_keep(p.drop, ((uint64_t)prob * S + (uint64_t)(q0 + il)) * (uint64_t)S + (uint64_t)kj) ? p.drop.scale : 0.f;
                pd[r] = pv * f;
                ds[r] = kmasked ? 0.f : p.scale * pv * (f * dp[r] - Ds[il]);
            }
            acc_product<NK>(dv, Gs, ct, pd, fi, kg);         // dV^T += dO^T P~
            acc_product<NK>(dk, Qs, ct, ds, fi, kg);         // dK^T += Q^T dS
        }
    }
    if (k_ok) {
        store_own<NK>(p.dk + (row_base + kj) * p.ldd + col0, dk, hd, p.hs, kg, 1.0f);
        store_own<NK>(p.dv + (row_base + kj) * p.ldd + col0, dv, hd, p.hs, kg, 1.0f);
    }
}

template <int NK>
int launch_wide(int which, const WideP& p, unsigned grid, hipStream_t s, const char* entry) {
    constexpr int BYTES = (2 * WideGeom<NK>::IMAGE + 3 * WB) * 4;
    static_assert(BYTES <= 163840, "LDS budget");
    static int reserved[3] = {0, 0, 0};
    const auto kernel = which == 0 ? wide_fwd_kernel<NK> : (which == 1 ? wide_bwd_q_kernel<NK> : wide_bwd_kv_kernel<NK>);
    if (const int st = lime_reserve_lds((const void*)kernel, BYTES, reserved[which], entry)) return st;
    kernel<<<grid, 256, BYTES, s>>>(p);
    return lime_check_launch(entry);
}

// nk = ceil(head_dim / 16): the instantiation that holds the padded head
int launch_wide_nk(int which, int nk, const WideP& p, unsigned grid, hipStream_t s, const char* entry) {
    switch (nk) {
        case 3: return launch_wide<3>(which, p, grid, s, entry);
        case 4: return launch_wide<4>(which, p, grid, s, entry);
        case 5: return launch_wide<5>(which, p, grid, s, entry);
        case 6: return launch_wide<6>(which, p, grid, s, entry);
        case 7: return launch_wide<7>(which, p, grid, s, entry);
        case 8: return launch_wide<8>(which, p, grid, s, entry);
    }
    LIME_REQUIRE(false, LIME_ERR_UNSUPPORTED, "%s: the wide kernels are not built for %d 16-column steps", entry, nk);
}

}  // namespace

// what every wide call checks before a launch
int lime_attn_wide_limits(const char* entry, int S, int n_head, int hd, int hs, long n_seq) {
    LIME_REQUIRE(hd > 32 && hd <= 128 && hd % 4 == 0 && S <= 512 && hs >= hd && hs % 4 == 0, LIME_ERR_UNSUPPORTED,
                 "%s: head_dim > 32 needs head_dim <= 128, head_dim %% 4 == 0, head_stride %% 4 == 0, head_stride >= head_dim and S <= 512 "
                 "(got head_dim=%d head_stride=%d S=%d); head_dim <= 32 takes any head_dim", entry, hd, hs, S);
    LIME_REQUIRE(n_seq * n_head * ((S + WB - 1) / WB) < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "%s: too many blocks", entry);
    return LIME_OK;
}

// The forward of every fp32 form at head_dim > 32 (token_attn_f32.hip has made the checks): r.n is NK
int lime_attn_wide_launch(const LimeAttnRoute& r, const lime_token_attention_args& a, hipStream_t s) {
    WideP p{};
    p.q = a.q; p.k = a.k; p.v = a.v; p.ld = a.ld_qkv; p.mask = a.key_mask; p.n_seq_dev = a.n_seq_dev; p.out = a.out; p.ldo = a.ldo; p.lse = a.lse;
    p.S = a.S; p.n_head = a.n_head; p.hd = a.head_dim; p.hs = a.head_stride; p.n_blk = (a.S + WB - 1) / WB; p.scale = a.scale;
    p.drop = lime_attn_dropout(a);
    return launch_wide_nk(0, r.n, p, (unsigned)((long)a.n_seq * a.n_head * p.n_blk), s, lime_attn_entry(a.form));
}

extern "C" int64_t lime_token_attention_bwd_workspace_wide(int32_t n_seq, int32_t S, int32_t n_head, int32_t head_dim) {
    if (head_dim <= 32) return lime_token_attention_bwd_workspace(n_seq, S, n_head);
    return (int64_t)n_seq * S * n_head * 3;          // row maximum, 1 / sum and delta per (token, head), at every S
}

// The backward at head_dim > 32 (token_attn_f32.hip has made the checks): r.n is NK; the statistics + dQ, then dK and dV, which reads
// the statistics
int lime_attn_bwd_wide_launch(const LimeAttnBwdRoute& r, const lime_token_attention_bwd_args& a, hipStream_t s) {
    const char* const entry = "lime_token_attention_bwd_f32";
    WideP p{};
    p.q = a.q; p.k = a.k; p.v = a.v; p.ld = a.ld_qkv; p.mask = a.key_mask; p.dout = a.dout; p.ldg = a.ldo; p.dq = a.dq; p.dk = a.dk; p.dv = a.dv;
    p.ldd = a.ld_dqkv; p.stats = a.workspace; p.S = a.S; p.n_head = a.n_head; p.hd = a.head_dim; p.hs = a.head_stride;
    p.n_blk = (a.S + WB - 1) / WB; p.scale = a.scale; p.drop = lime_attn_bwd_dropout(a);
    const unsigned grid = (unsigned)((long)a.n_seq * a.n_head * p.n_blk);
    if (const int st = launch_wide_nk(1, r.n, p, grid, s, entry)) return st;
    return launch_wide_nk(2, r.n, p, grid, s, entry);
}
