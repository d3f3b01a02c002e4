// lime_attn_pool_sp_f32: layers.Attention (layers.py:285-300) in ONE launch -- the additive attention pool of the NAML content
// encoder (newsEncoders.py:686-694) over n_seq sequences of T rows of x [n_seq T, D]:
//
//   out[s] = sum_t alpha[s, t] x[s T + t],   alpha[s] = softmax_t(w2 . tanh(W1 x[s T + t] + b1))   (masked keys: score -1e9)
//
// Replaces ops.linear(act='tanh') + ops.additive_pool, whose [rows, A] fp32 hidden state went to HBM and back (360 MB each way for
// the config-2 bodies).  The linear1 pass mirrors csrc/ffn_sp_f32.hip:
//   * a workgroup (4 waves, one per SIMD, one per CU) owns a 128-row tile holding floor(128 / T) WHOLE sequences (no sequence
//     straddles two tiles: a sequence's output depends on its own rows only, whatever the tile slot it lands in); a wave owns 32 rows
//     (two 16-row halves).
//   * the hidden state runs in passes of 128 columns (A <= 512: at most four).  A step is two 32-deep k chunks: x's fragments are read
//     straight from global memory one step ahead and split into three bf16 terms in registers; W1 is pre-split by
//     lime_attn_pool_pack_sp (inside the forward: parameters may change between graph replays), each step's slot one contiguous block
//     copied by LDS-DMA into a two-slot ring (step s + 1 issued during step s, one vmcnt(0) wait + barrier per step).
//   * split products (split_mfma.h: six v_mfma_f32_16x16x32_bf16 per block), or under lime_set_split_gemm(0) eight
//     v_mfma_f32_16x16x4_f32 per block on the fp32 sums of the same three term images.
//   * the epilogue of a pass: tanhf(acc + b1) (the tanh of the split GEMM's act='tanh' epilogue) times w2, summed per lane in a fixed
//     order; after the last pass the four lanes that share a row meet through two shuffles: one fp32 score per row.
//   * then, in the same workgroup: the softmax per sequence (max-subtracted expf, as additive_pool_kernel) and the weighted sum over
//     t = 0 .. T - 1 in order, re-reading the tile's x rows (L2 hits).
// A device sequence count (n_seq_dev) bounds the work of a compacted batch: sequences beyond it are neither read nor written.
#include "common.h"
#include "dev_helpers.h"
#include "split_mfma.h"

using namespace lime_dev;

int lime_split_mode();

namespace {

constexpr int BM = 128;                    // rows per tile (4 waves x 32)
constexpr int PW = 128;                    // hidden columns per pass
constexpr int NT1 = PW / 16;               // output tiles per pass
constexpr int TERM = PW * 64;              // bytes of one term image of one 32-deep chunk: [128 rows][32 bf16]
constexpr int CHUNK = 3 * TERM;            // 24,576
constexpr int SLOT = 2 * CHUNK;            // 49,152: a step (two chunks)
constexpr int A_MAX = 512;
constexpr int T_MAX = BM;
constexpr int CONST_OFF = 2 * SLOT;        // b1 [A_MAX], w2 [A_MAX], scores / weights [BM] fp32
constexpr int LDS_BYTES = CONST_OFF + (2 * A_MAX + BM) * 4;      // 102,912 of the CU's 163,840
constexpr int NI = SLOT / 1024;            // DMA instructions per slot (1 KB each)
constexpr int DMA_PER_WAVE = NI / 4;       // 12

struct AttnPoolP {
    const float* x; long ldx;
    const uint16_t* w1p; const float* b1; const float* w2;
    const unsigned char* mask;
    float* out; long ldo;
    int D, A, n_seq, T, spt, steps, passes;
    const int* n_seq_dev;
};

// one 16 x 16 x 32 block: w = eight k values of hidden column fi (the three LDS term images), x = eight k values of row fi
template <bool SPLIT>
struct WFrag;
template <>
struct WFrag<true> {
    SplitFrag f;
    __device__ __forceinline__ void load(const unsigned char* b) {
        f.h = *reinterpret_cast<const bf16x8*>(b);
        f.m = *reinterpret_cast<const bf16x8*>(b + TERM);
        f.l = *reinterpret_cast<const bf16x8*>(b + 2 * TERM);
    }
};
template <>
struct WFrag<false> {
    float v[8];
    static __device__ __forceinline__ float lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
    static __device__ __forceinline__ float hi(unsigned u) { return __builtin_bit_cast(float, u & 0xFFFF0000u); }
    __device__ __forceinline__ void load(const unsigned char* b) {
        const u32x4 h = *reinterpret_cast<const u32x4*>(b);
        const u32x4 m = *reinterpret_cast<const u32x4*>(b + TERM);
        const u32x4 l = *reinterpret_cast<const u32x4*>(b + 2 * TERM);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[2 * q] = (lo(h[q]) + lo(m[q])) + lo(l[q]);
            v[2 * q + 1] = (hi(h[q]) + hi(m[q])) + hi(l[q]);
        }
    }
};
template <bool SPLIT>
struct XFrag;
template <>
struct XFrag<true> {
    SplitFrag f;
    __device__ __forceinline__ void set(const f32x4 a, const f32x4 b) { f = split_frag(a, b); }
};
template <>
struct XFrag<false> {
    f32x4 a, b;
    __device__ __forceinline__ void set(const f32x4 a_, const f32x4 b_) { a = a_; b = b_; }
};
__device__ __forceinline__ f32x4 prod(const WFrag<true>& w, const XFrag<true>& x, f32x4 c) { return split_mfma16(w.f, x.f, c); }
// v_mfma_f32_16x16x4_f32: lane (fi, kg) supplies A[fi][kg] and B[kg][fi]; product q takes k = 8 kg + q in slot kg (the same label on
// both operands), the result has the layout of the bf16 block
__device__ __forceinline__ f32x4 prod(const WFrag<false>& w, const XFrag<false>& x, f32x4 c) {
#pragma unroll
    for (int q = 0; q < 4; ++q) c = __builtin_amdgcn_mfma_f32_16x16x4f32(w.v[q], x.a[q], c, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; ++q) c = __builtin_amdgcn_mfma_f32_16x16x4f32(w.v[4 + q], x.b[q], c, 0, 0, 0);
    return c;
}

template <bool SPLIT>
__global__ __launch_bounds__(256, 1) void attn_pool_sp_kernel(const AttnPoolP p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_live = live_count(p.n_seq_dev, p.n_seq);
    const int T = p.T, spt = p.spt, D = p.D;
    const int ntiles = (n_live + spt - 1) / spt;
    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    const int S = p.steps, NP = p.passes;

    float* const cb1 = reinterpret_cast<float*>(lds + CONST_OFF);
    float* const cw2 = cb1 + A_MAX;
    float* const score = cw2 + A_MAX;
    for (int c = tid; c < NP * PW; c += 256) {
        cb1[c] = (c < p.A && p.b1) ? p.b1[c] : 0.f;
        cw2[c] = c < p.A ? p.w2[c] : 0.f;
    }
    __syncthreads();                                   // nothing in flight yet

    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(p.w1p);
    // step s of a tile (pass s / S, position s % S) is packed block s; instruction i of wave w copies its 1 KB piece
    // (4 i + w + rot) % NI -- the rotation by the CU's position in its XCD spreads the L2 requests (ffn_sp_f32.hip)
    const int rot = (int)((blockIdx.x >> 3) * 5u);
    auto issue_one = [&](int s, int slot, int i) {
        const int b = (4 * i + wave + rot) % NI;
        dma16(rs_w, lds + slot * SLOT + b * 1024, (unsigned)lane * 16u, s * SLOT + b * 1024);
    };
    auto issue_w = [&](int s, int slot) {
        for (int i = 0; i < DMA_PER_WAVE; ++i) issue_one(s, slot, i);
    };
    // x fragments of a step: chunks 2 pos, 2 pos + 1, row halves tt, k 8 kg .. 8 kg + 7 as two quads (D % 4 == 0: a quad is real or
    // beyond D as a whole; rows beyond the tile's sequences and quads beyond D read zeros)
    f32x4 xn[2][2][2];
    auto load_x = [&](int t, int pos) {
        const int n_here = n_live - t * spt;
        const int rows = (n_here < spt ? n_here : spt) * T;
        const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(p.x + (long)t * spt * T * p.ldx);
        const int ln = lane_here(), fi = ln & 15, kg = ln >> 4;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int rl = 32 * wave + 16 * tt + fi;
            const unsigned ro = (unsigned)rl * (unsigned)p.ldx * 4u;
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int col = 32 * (2 * pos + cc) + 8 * kg + 4 * q;
                    const unsigned vo = (rl < rows && col < D) ? ro + (unsigned)col * 4u : OOB;
                    xn[cc][tt][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, vo, 0, 0));
                }
        }
    };

    // MFMA lane layout (a = W1 rows = hidden columns, b = x rows): the result is D^T, lane (row fi, kg) holds hidden columns
    // 16 t + 4 kg + r, r = 0..3
    const int w_off = (lane & 15) * 64 + (((lane >> 4) ^ swz4(((lane & 15) >> 2) & 3)) * 16);
    f32x4 acc[2][NT1];
    float sc[2];

    issue_w(0, 0);
    load_x(tile, 0);
    wait_vm<0>();
    ring_barrier();
    int gs = 0;                                        // steps run by this workgroup (ring position)
    for (; tile < ntiles; tile += gridDim.x) {
        const bool last = tile + (int)gridDim.x >= ntiles;
        sc[0] = 0.f;
        sc[1] = 0.f;
        for (int pass = 0; pass < NP; ++pass) {
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int t = 0; t < NT1; ++t) acc[tt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int pos = 0; pos < S; ++pos) {
                const unsigned char* const sb = lds + (gs & 1) * SLOT + w_off;
                f32x4 xc[2][2][2];
#pragma unroll
                for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) { xc[cc][tt][0] = xn[cc][tt][0]; xc[cc][tt][1] = xn[cc][tt][1]; }
                // the next step: its x fragments now, its weight slot one DMA instruction per MFMA group below
                const bool wrap = pos == S - 1 && pass == NP - 1;
                const bool go = !(wrap && last);
                const int ns = wrap ? 0 : pass * S + pos + 1;
                const int nslot = (gs + 1) & 1;
                if (go) load_x(wrap ? tile + (int)gridDim.x : tile, pos + 1 == S ? 0 : pos + 1);
                WFrag<SPLIT> w[2];
                w[0].load(sb);
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) {
                    XFrag<SPLIT> x0, x1;
                    x0.set(xc[cc][0][0], xc[cc][0][1]);
                    x1.set(xc[cc][1][0], xc[cc][1][1]);
#pragma unroll
                    for (int t = 0; t < NT1; ++t) {
                        const int i = cc * NT1 + t;
                        if (i + 1 < 2 * NT1) w[(i + 1) & 1].load(sb + ((i + 1) / NT1) * CHUNK + ((i + 1) % NT1) * 1024);
                        acc[0][t] = prod(w[i & 1], x0, acc[0][t]);
                        acc[1][t] = prod(w[i & 1], x1, acc[1][t]);
                        __builtin_amdgcn_sched_barrier(0);
                        if (go && i < DMA_PER_WAVE) issue_one(ns, nslot, i);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                wait_vm<0>();                          // this wave's part of the next slot (and its x fragments)
                ring_barrier();                        // ... everyone's: the next slot is complete, this one is free
                ++gs;
            }
            // the pass's 128 hidden columns: tanh(acc + b1) . w2, summed per lane in column order
            const int kg = lane_here() >> 4;
            const float* const b1 = cb1 + PW * pass + 4 * kg;
            const float* const w2 = cw2 + PW * pass + 4 * kg;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                float s = sc[tt];
#pragma unroll
                for (int t = 0; t < NT1; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s += tanhf(acc[tt][t][r] + b1[16 * t + r]) * w2[16 * t + r];
                sc[tt] = s;
            }
        }

        // ---- scores -> LDS (the four lanes of a row: two shuffles, the same bits in each), softmax per sequence, weighted sum
        const int n_here = n_live - tile * spt;
        const int nseq = n_here < spt ? n_here : spt;
        const int rows = nseq * T;
        const long row0 = (long)tile * spt * T;
        {
            const int ln = lane_here(), fi = ln & 15, kg = ln >> 4;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                float v = sc[tt];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                const int rl = 32 * wave + 16 * tt + fi;
                if (kg == 0 && rl < rows) score[rl] = (p.mask && p.mask[row0 + rl] == 0) ? -1e9f : v;
            }
        }
        ring_barrier();
        if (T <= 32) {                                 // one thread per sequence, t in order
            if (tid < nseq) {
                float* const a = score + tid * T;
                float mx = -INFINITY;
                for (int t = 0; t < T; ++t) mx = fmaxf(mx, a[t]);
                float sum = 0.f;
                for (int t = 0; t < T; ++t) {
                    const float e = expf(a[t] - mx);
                    a[t] = e;
                    sum += e;
                }
                const float inv = 1.0f / sum;
                for (int t = 0; t < T; ++t) a[t] *= inv;
            }
        } else {                                       // one wave per sequence, t over the lanes (T <= 128: two per lane)
            for (int sq = wave; sq < nseq; sq += 4) {
                float* const a = score + sq * T;
                const bool in0 = lane < T, in1 = lane + 64 < T;
                const float v0 = in0 ? a[lane] : -INFINITY, v1 = in1 ? a[lane + 64] : -INFINITY;
                const float mx = wave_max(fmaxf(v0, v1));
                const float e0 = in0 ? expf(v0 - mx) : 0.f, e1 = in1 ? expf(v1 - mx) : 0.f;
                const float inv = 1.0f / wave_sum(e0 + e1);
                if (in0) a[lane] = e0 * inv;
                if (in1) a[lane + 64] = e1 * inv;
            }
        }
        ring_barrier();
        // out[s, 4 q .. 4 q + 3] = sum_t alpha[s, t] x[s T + t, 4 q ..], t in order (the next tile's scores are written after at least
        // one more ring barrier)
        const int nq = D >> 2;
        const float* const xt = p.x + row0 * p.ldx;
        for (int it = tid; it < nseq * nq; it += 256) {
            const int sl = it / nq, q = it - sl * nq;
            const float* xr = xt + (long)sl * T * p.ldx + 4 * q;
            const float* const al = score + sl * T;
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int t = 0; t < T; ++t) {
                o += al[t] * *reinterpret_cast<const f32x4*>(xr);
                xr += p.ldx;
            }
            *reinterpret_cast<f32x4*>(p.out + ((long)tile * spt + sl) * p.ldo + 4 * q) = o;
        }
    }
}

// W1 [A, D] (ld ldw1) as the kernel's ring slots, three bf16 term images each (x = hi + mid + lo, split_pair's rounding), every step's
// slot one contiguous block in the order of its LDS image: w1p [passes][steps][2 chunks][3 terms][128 rows][32] holds
// W1[128 pass + row, 32 (2 step + chunk) + k], zero beyond A and D; row r's 32 bf16 are four 16-byte segments, logical segment kg at
// physical kg ^ swz4((r >> 2) & 3).
__global__ void attn_pool_pack_kernel(const float* __restrict__ w1, long ldw1, int D, int A, int nch, long n, uint16_t* __restrict__ w1p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int pk = (int)(i & 31), row = (int)((i >> 5) % PW);
    const long chunk = i / (32 * PW);                  // pass * nch + chunk
    const int c = (int)(chunk % nch), pass = (int)(chunk / nch);
    const int kg = (pk >> 3) ^ swz4((row >> 2) & 3), e = pk & 7;
    const int hcol = PW * pass + row, k = 32 * c + 8 * kg + e;
    const SplitPair t = split_pair(hcol < A && k < D ? w1[(long)hcol * ldw1 + k] : 0.f, 0.f);
    uint16_t* const d = w1p + chunk * (3 * PW * 32) + row * 32 + pk;
    d[0] = (uint16_t)(t.h & 0xFFFFu);
    d[PW * 32] = (uint16_t)(t.m & 0xFFFFu);
    d[2 * PW * 32] = (uint16_t)(t.l & 0xFFFFu);
}

int steps_of(int D) { return (D + 63) / 64; }
int passes_of(int A) { return (A + PW - 1) / PW; }
bool dims_ok(int D, int A) { return D > 0 && D % 4 == 0 && D <= 0x4000 && A > 0 && A <= A_MAX; }

}  // namespace

extern "C" int64_t lime_attn_pool_pack_sp_size(int32_t D, int32_t A) {
    if (!dims_ok(D, A)) return 0;
    return (int64_t)passes_of(A) * steps_of(D) * (SLOT / 2);
}

extern "C" int lime_attn_pool_pack_sp(const float* w1, int64_t ldw1, int32_t D, int32_t A, uint16_t* w1p, void* stream) {
    LIME_REQUIRE(w1 && w1p, LIME_ERR_BAD_ARG, "lime_attn_pool_pack_sp: NULL pointer");
    LIME_REQUIRE(dims_ok(D, A), LIME_ERR_UNSUPPORTED, "lime_attn_pool_pack_sp: built for D %% 4 == 0, D <= 16384 (D = %d) and A <= %d (A = %d)",
                 D, A_MAX, A);
    LIME_REQUIRE(ldw1 >= D, LIME_ERR_BAD_ARG, "lime_attn_pool_pack_sp: leading dimension < row");
    const long n = (long)passes_of(A) * steps_of(D) * 2 * PW * 32;
    hipLaunchKernelGGL(attn_pool_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w1, (long)ldw1, D, A,
                       2 * steps_of(D), n, w1p);
    return lime_check_launch("lime_attn_pool_pack_sp");
}

extern "C" int lime_attn_pool_sp_f32(const float* x, int64_t ldx, int32_t D, const uint16_t* w1p, const float* b1, const float* w2,
                                     int32_t A, const uint8_t* mask, float* out, int64_t ldo, int32_t n_seq, int32_t T,
                                     const int32_t* n_seq_dev, void* stream) {
    LIME_REQUIRE(x && w1p && w2 && out, LIME_ERR_BAD_ARG, "lime_attn_pool_sp_f32: NULL pointer");
    LIME_REQUIRE(n_seq >= 0 && T > 0, LIME_ERR_BAD_ARG, "lime_attn_pool_sp_f32: bad n_seq %d / T %d", n_seq, T);
    LIME_REQUIRE(T <= T_MAX && dims_ok(D, A), LIME_ERR_UNSUPPORTED,
                 "lime_attn_pool_sp_f32: built for T <= %d (T = %d), D %% 4 == 0, D <= 16384 (D = %d) and A <= %d (A = %d)", T_MAX, T, D,
                 A_MAX, A);
    LIME_REQUIRE(ldx >= D && ldx % 4 == 0 && (uintptr_t)x % 16 == 0, LIME_ERR_BAD_ARG,
                 "lime_attn_pool_sp_f32: x rows must be 16-byte aligned (ldx %% 4 == 0)");
    LIME_REQUIRE(ldo >= D && ldo % 4 == 0 && (uintptr_t)out % 16 == 0, LIME_ERR_BAD_ARG,
                 "lime_attn_pool_sp_f32: out rows must be 16-byte aligned (ldo %% 4 == 0)");
    LIME_REQUIRE((uintptr_t)w1p % 16 == 0, LIME_ERR_BAD_ARG, "lime_attn_pool_sp_f32: packed W1 must be 16-byte aligned");
    LIME_REQUIRE(128L * ldx * 4 < 0x7FFFFFF0L, LIME_ERR_UNSUPPORTED, "lime_attn_pool_sp_f32: x rows too wide for 32-bit offsets");
    if (n_seq == 0) return LIME_OK;
    AttnPoolP p{};
    p.x = x; p.ldx = ldx; p.w1p = w1p; p.b1 = b1; p.w2 = w2; p.mask = mask; p.out = out; p.ldo = ldo;
    p.D = D; p.A = A; p.n_seq = n_seq; p.T = T; p.spt = BM / T; p.steps = steps_of(D); p.passes = passes_of(A);
    p.n_seq_dev = n_seq_dev;
    const long ntiles = ((long)n_seq + p.spt - 1) / p.spt;
    const long nwg = lime_persistent_grid(ntiles);
    hipStream_t s = (hipStream_t)stream;
    if (lime_split_mode() & 1) hipLaunchKernelGGL((attn_pool_sp_kernel<true>), dim3((unsigned)nwg), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((attn_pool_sp_kernel<false>), dim3((unsigned)nwg), dim3(256), 0, s, p);
    return lime_check_launch("lime_attn_pool_sp_f32");
}
