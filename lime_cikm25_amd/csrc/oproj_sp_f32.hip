// lime_encoder_oproj_sp: out_proj + residual + norm1 of an fp32 encoder layer, x1 = LayerNorm(res + attn Wo^T + bo), in one
// launch with split products on the bf16 matrix cores (split_mfma.h: three bf16 terms per fp32 operand, six MFMAs per 16 x 16 x 32
// block).  Token-stationary, the geometry and the weight ring of ffn_sp_f32.hip's linear2 half:
//
//   * a workgroup (8 waves, two per SIMD, one workgroup per CU) owns a 128-token tile; wave w owns tokens 16 w .. 16 w + 15 x all
//     304 model columns: 19 accumulator tiles, zero at the start of a tile.  Two waves share a SIMD so that one's waits leave the
//     matrix pipe to the other.
//   * ten steps per tile, one 32-deep k chunk each.  Wo is pre-split into three bf16 term images by lime_oproj_pack_sp (inside the
//     forward, or once per weight change: newsEncoders.WeightProducts), every chunk ONE contiguous block in the order of its LDS image
//     (swizzled [row][64-byte] rows: conflict-free ds_read_b128 fragments), copied by LDS-DMA into two ring slots: step s + 1 is
//     issued during step s (one instruction per MFMA group), then one vmcnt(0) wait + barrier per step.
//   * B operand: the attention output rows of the wave's own tokens, straight from global memory one step ahead (two 16-byte
//     loads per lane and step), split in registers.
//   * epilogue: + bo, + the residual row -- res[row], or the word row table[res_ids[row]] (an HBM gather, through a 64-bit row
//     address per lane) and then the positional row pe[row % period] (cache-hot) in a second sweep -- LayerNorm over the E real
//     columns (the four lanes that share a token meet through two shuffles), fp32 rows out.  The word rows are requested BEFORE the
//     tile's last step (their latency falls under its 114 MFMAs; the 76 landing registers are free), the positional rows behind it,
//     ahead of the first sweep.
//   * a row's arithmetic does not depend on the tile or the launch it sits in: one k order, one reduction order.
#include <type_traits>

#include "common.h"
#include "dev_helpers.h"
#include "split_mfma.h"

using namespace lime_dev;

namespace {

constexpr int NW = 8, NTHR = 64 * NW;        // waves per workgroup: two per SIMD
constexpr int BM = 16 * NW;                // tokens per tile: 128, one 16-token MFMA tile per wave
constexpr int ND = 19, DP = 16 * ND;       // model columns carried: 304
constexpr int NCH = 10;                    // 32-deep k chunks (320 >= E): the steps of a tile
constexpr int TERM = DP * 64;              // bytes of one term image of a chunk: [304 rows][32 bf16]
constexpr int SLOT = 3 * TERM;             // 58,368: a step
constexpr int NI = SLOT / 1024;            // 57 DMA instructions (1 KB each) per slot
constexpr int DMA_PER_WAVE = (NI + NW - 1) / NW;     // 8: at most this many per wave and slot
constexpr int CONST_OFF = 2 * SLOT;        // bo, gamma, beta [304] fp32
constexpr int LDS_BYTES = CONST_OFF + 3 * DP * 4;                // 120,384 of the CU's 163,840

struct OprojSpP {
    const float* a; long lda;
    const uint16_t* wp;
    const float* bias; const float* g; const float* beta; float eps;
    const float* res; long ldr; const int* ids; const float* pe; long ldpe; int period;
    float* out; long ldo;
    int M, E;
    const int* m_dev;
};

__global__ __launch_bounds__(NTHR, 1) void oproj_sp_kernel(const OprojSpP p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fi = lane & 15, kg = lane >> 4;
    const int M = live_count(p.m_dev, p.M);
    const int ntiles = (M + BM - 1) / BM;
    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    const int E = p.E;

    float* const cs = reinterpret_cast<float*>(lds + CONST_OFF);
    for (int c = tid; c < DP; c += NTHR) {
        cs[c] = c < E ? p.bias[c] : 0.f;
        cs[DP + c] = c < E ? p.g[c] : 0.f;
        cs[2 * DP + c] = c < E ? p.beta[c] : 0.f;
    }
    __syncthreads();                                   // nothing in flight yet

    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(p.wp), rs_pe = make_rsrc(p.pe);
    // step s of a tile is chunk s: one contiguous block of 57 KB = 57 DMA instructions (1 KB each, lane l lands at +16 l), instruction
    // i of wave w is block (8 i + w + rot) % 57.  The rotation by the CU's position in its XCD keeps the 32 CUs that share an L2 from
    // asking for the same lines at the same moment.
    const int rot = (int)((blockIdx.x >> 3) * 5u);
    auto issue_one = [&](int s, int slot, int i) {
        const int idx = NW * i + wave;
        if (idx < NI) {
            const int b = (idx + rot) % NI;
            dma16(rs_w, lds + slot * SLOT + b * 1024, (unsigned)lane * 16u, s * SLOT + b * 1024);
        }
    };
    // Every load below is branch-free (dead_bit, dev_helpers.h): a join of divergent control flow would wait vmcnt(0) in front of the
    // MFMAs -- with the residual gather in flight.
    // the attention rows of step s: k 32 s + 8 kg .. + 7 as two quads (E % 4 == 0: a quad is real or beyond E as a
    // whole; rows beyond M and quads beyond E read zeros)
    f32x4 xn[2];
    auto load_x = [&](int t, int s) {
        const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(p.a + (long)t * BM * p.lda);
        const int rows_left = M - t * BM;
        const int ln = lane_here(), fi = ln & 15, kg = ln >> 4;
        const int rl = 16 * wave + fi;
        const unsigned ro = (unsigned)rl * (unsigned)p.lda * 4u;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int col = 32 * s + 8 * kg + 4 * q;
            xn[q] = buf_load4(rs_x, (ro + (unsigned)col * 4u) | dead_bit(rows_left - 1 - rl, E - 1 - col), 0);
        }
    };
    // the word id of the lane's token (0 without ids and for rows beyond M), read at the top of the tile: a step of its own ahead of
    // the row it addresses
    int rid;
    auto load_ids = [&](int t) {
        const __amdgpu_buffer_rsrc_t rs_i = make_rsrc(p.ids + (long)t * BM);
        const int rows_left = p.ids ? M - t * BM : 0;
        const int rl = 16 * wave + (lane_here() & 15);
        rid = buf_load_i32(rs_i, (unsigned)rl * 4u | dead_bit(rows_left - 1 - rl, 0));
    };
    // the residual rows of tile t: the 19 quads of res[row] or table[rid], through a 64-bit row address.  A lane whose row is beyond
    // M asks for row 0, a quad beyond E for quad 0 of its row (both are there); neither value is used -- the statistics and the
    // stores skip them.
    f32x4 rr[ND], pq[ND];
    auto load_res = [&](int t) {
        const int ln = lane_here(), fi = ln & 15, kg = ln >> 4;
        const long row = (long)t * BM + 16 * wave + fi;
        int id = rid;
        asm volatile("" : "+v"(id));                   // the id is waited for HERE (its address arithmetic would be hoisted to the load)
        const float* const rp = p.res + (row < M ? (p.ids ? (long)id : row) : 0L) * p.ldr;
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int col = 16 * i + 4 * kg;
            rr[i] = *reinterpret_cast<const f32x4*>(rp + (col < E ? col : 0));
        }
    };
    // ... and their positional rows pe[row % period] (a few KB shared by every tile: cache hits); zeros without a positional table
    auto load_pe = [&](int t) {
        const int ln = lane_here(), fi = ln & 15, kg = ln >> 4;
        const int row = t * BM + 16 * wave + fi;
        const unsigned ro = ((unsigned)row % (unsigned)(p.pe ? p.period : 1)) * (unsigned)p.ldpe * 4u;
        const int live = p.pe ? M - 1 - row : -1;
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const int col = 16 * i + 4 * kg;
            pq[i] = buf_load4(rs_pe, (ro + (unsigned)col * 4u) | dead_bit(live, E - 1 - col), 0);
        }
    };

    // MFMA lane layout (v_mfma_f32_16x16x32_bf16, a = weight rows = output columns, b = tokens): lane (fi, kg) reads k 8 kg .. 8 kg + 7
    // of row fi; the result is D^T: lane (token fi, kg) holds columns 16 t + 4 kg + r, r = 0..3
    const int w_off = fi * 64 + ((kg ^ swz4((fi >> 2) & 3)) * 16);
    auto wfrag = [&](const unsigned char* b) {
        SplitFrag f;
        f.h = *reinterpret_cast<const bf16x8*>(b);
        f.m = *reinterpret_cast<const bf16x8*>(b + TERM);
        f.l = *reinterpret_cast<const bf16x8*>(b + 2 * TERM);
        return f;
    };
    f32x4 acc[ND];
    // vmcnt(0) with the attention fragments passed through it (wait_vm0_landed, dev_helpers.h): hipcc's own wait would sit in front of
    // the fragments' first use, at the top of the next step -- where the tile's word ids and the previous tile's stores are in flight
    auto wait_all = [&]() { wait_vm0_landed(xn[0], xn[1]); };

    // prologue: the first step of this workgroup's first tile
    for (int i = 0; i < DMA_PER_WAVE; ++i) issue_one(0, 0, i);
    load_x(tile, 0);
    wait_all();
    ring_barrier();
    int gs = 0;                                        // steps run by this workgroup (ring position)
    for (; tile < ntiles; tile += gridDim.x) {
        const bool last = tile + (int)gridDim.x >= ntiles;
#pragma unroll
        for (int t = 0; t < ND; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        load_ids(tile);                                // (lands behind step 0's wait)
        // step s: its attention fragments (loaded one step ahead) leave xn before the next step's loads reuse it; the next step's
        // weights go into the other slot (everyone has left it: the barrier behind the previous step), one DMA instruction per MFMA
        // group.  One weight fragment (three terms) is read ahead of the MFMAs that use the previous one; sched_barriers keep hipcc
        // from hoisting more.  The tile's last step also carries the residual (word) rows and the next tile's first step.
        auto step = [&](auto last_c, int s) {
            constexpr bool LAST = decltype(last_c)::value;
            const unsigned char* const sb = lds + (gs & 1) * SLOT + w_off;
            const SplitFrag x0 = split_frag(xn[0], xn[1]);
            __builtin_amdgcn_sched_barrier(0);
            const bool go = !(LAST && last);
            const int ns = LAST ? 0 : s + 1;
            const int nslot = (gs + 1) & 1;
            if constexpr (LAST) load_res(tile);
            // (unconditional: behind this workgroup's last tile every row is beyond M and nothing is read; under `if (go)` the
            // fragments become a phi whose copy waits for these loads -- and the gather in front of them -- ahead of the MFMAs)
            load_x(LAST ? tile + (int)gridDim.x : tile, ns);
            SplitFrag w[2];
            w[0] = wfrag(sb);
#pragma unroll
            for (int t = 0; t < ND; ++t) {
                if (t + 1 < ND) w[(t + 1) & 1] = wfrag(sb + (t + 1) * 1024);
                acc[t] = split_mfma16(w[t & 1], x0, acc[t]);
                __builtin_amdgcn_sched_barrier(0);
                if (go && t < DMA_PER_WAVE) issue_one(ns, nslot, t);
                __builtin_amdgcn_sched_barrier(0);
            }
            wait_all();                                // this wave's part of the next slot, its attention fragments (and residual rows)
            ring_barrier();                            // ... everyone's: the next slot is complete, this one is free
            ++gs;
        };
#pragma unroll 1
        for (int s = 0; s < NCH - 1; ++s) step(std::false_type{}, s);
        step(std::true_type{}, NCH - 1);

        // ---- epilogue: + bo + residual, LayerNorm over the E real columns (the statistics and the stores skip quads beyond E), fp32 rows
        const long row0 = (long)tile * BM;
        const int rows_left = M - (int)row0;
        const int le = lane_here(), fi = le & 15, kg = le >> 4;      // epilogue-only offsets are computed here, not carried through the tile
        const float* const cs_ = cs + 4 * kg;
        const float inv_n = 1.0f / (float)E;
        // the word rows are here (the wait behind the last step); the cache-hot positional rows are requested now and land under
        // the first sweep
        load_pe(tile);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(cs_ + 16 * t);
            acc[t] = acc[t] + b + rr[t];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < ND; ++t) acc[t] += pq[t];
        __builtin_amdgcn_sched_barrier(0);
        float s1 = 0.f;
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            if (16 * t + 4 * kg < E) {
                const f32x4 v = acc[t];
                s1 += (v[0] + v[1]) + (v[2] + v[3]);
            }
        }
        s1 += __shfl_xor(s1, 16);
        s1 += __shfl_xor(s1, 32);
        const float mean = s1 * inv_n;
        float s2 = 0.f;
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            if (16 * t + 4 * kg < E) {
                const f32x4 d = acc[t] - mean;
                s2 += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
            }
        }
        s2 += __shfl_xor(s2, 16);
        s2 += __shfl_xor(s2, 32);
        const float rstd = rsqrtf(s2 * inv_n + p.eps);
        __builtin_amdgcn_sched_barrier(0);
        const float* const gs_ = cs_ + DP;
        const float* const es_ = cs_ + 2 * DP;
        const __amdgpu_buffer_rsrc_t rs_c = make_rsrc(p.out + row0 * p.ldo);
        const int rl = 16 * wave + fi;
        const unsigned ro = (unsigned)rl * (unsigned)p.ldo * 4u;
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            const f32x4 ga = *reinterpret_cast<const f32x4*>(gs_ + 16 * t);
            const f32x4 be = *reinterpret_cast<const f32x4*>(es_ + 16 * t);
            const int col = 16 * t + 4 * kg;
            buf_store4((acc[t] - mean) * rstd * ga + be, rs_c, (rl < rows_left && col < E) ? ro + (unsigned)col * 4u : OOB, 0);
        }
    }
}

// Wo as the kernel's ring slots: [10 chunks][3 terms][304 rows][32] bf16 (x = hi + mid + lo, split_pair's rounding), every chunk one
// contiguous block in the order of its LDS image; row n's 32 bf16 are four 16-byte segments, logical segment kg at physical
// kg ^ swz4((n >> 2) & 3); logical position 8 kg + e of row n in chunk c holds Wo[n, 32 c + 8 kg + e], zero for n >= E or k >= E.
__global__ void oproj_sp_pack_kernel(const float* __restrict__ w, long ldw, int E, uint16_t* __restrict__ wp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NCH * DP * 32) return;
    const int pk = i & 31, n = (i >> 5) % DP, c = i / (32 * DP);
    const int kg = (pk >> 3) ^ swz4((n >> 2) & 3), e = pk & 7;
    const int k = 32 * c + 8 * kg + e;
    const SplitPair t = split_pair((n < E && k < E) ? w[(long)n * ldw + k] : 0.f, 0.f);
    uint16_t* const d = wp + (long)c * (3 * DP * 32) + n * 32 + pk;
    d[0] = (uint16_t)(t.h & 0xFFFFu);
    d[DP * 32] = (uint16_t)(t.m & 0xFFFFu);
    d[2 * DP * 32] = (uint16_t)(t.l & 0xFFFFu);
}

}  // namespace

extern "C" int64_t lime_oproj_pack_sp_size(void) { return (int64_t)NCH * 3 * DP * 32; }

extern "C" int lime_oproj_pack_sp(const float* w, int64_t ldw, int32_t E, uint16_t* wp, void* stream) {
    LIME_REQUIRE(w && wp, LIME_ERR_BAD_ARG, "lime_oproj_pack_sp: NULL pointer");
    LIME_REQUIRE(E > 0 && E <= DP && E % 4 == 0, LIME_ERR_UNSUPPORTED, "lime_oproj_pack_sp: built for E <= %d, E %% 4 == 0 (E = %d)", DP, E);
    LIME_REQUIRE(ldw >= E, LIME_ERR_BAD_ARG, "lime_oproj_pack_sp: leading dimension < row");
    hipLaunchKernelGGL(oproj_sp_pack_kernel, dim3((NCH * DP * 32 + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, (long)ldw, E, wp);
    return lime_check_launch("lime_oproj_pack_sp");
}

extern "C" int lime_encoder_oproj_sp(const lime_oproj_sp_args* a, void* stream) {
    LIME_REQUIRE(a != nullptr, LIME_ERR_BAD_ARG, "lime_encoder_oproj_sp: args is NULL");
    LIME_REQUIRE(a->attn && a->wp && a->bias && a->res && a->ln_gamma && a->ln_beta && a->out, LIME_ERR_BAD_ARG,
                 "lime_encoder_oproj_sp: NULL pointer");
    LIME_REQUIRE(a->M >= 0 && a->M < 0x7FF00000 && a->E > 0 && a->E <= DP && a->E % 4 == 0, LIME_ERR_UNSUPPORTED,
                 "lime_encoder_oproj_sp: built for E <= %d, E %% 4 == 0 (E = %d) and M < 2^31 - 2^20", DP, a->E);
    LIME_REQUIRE(a->lda >= a->E && lime_al16(a->attn, a->lda), LIME_ERR_BAD_ARG,
                 "lime_encoder_oproj_sp: attn rows must be 16-byte aligned (lda %% 4 == 0)");
    LIME_REQUIRE((uintptr_t)a->wp % 16 == 0, LIME_ERR_BAD_ARG,
                 "lime_encoder_oproj_sp: packed weights must be 16-byte aligned (see lime_oproj_pack_sp)");
    LIME_REQUIRE(a->ldr >= a->E && lime_al16(a->res, a->ldr), LIME_ERR_BAD_ARG,
                 "lime_encoder_oproj_sp: res rows must be 16-byte aligned (ldr %% 4 == 0)");
    LIME_REQUIRE(a->res_ids || !a->res_pe, LIME_ERR_BAD_ARG, "lime_encoder_oproj_sp: res_pe needs res_ids");
    if (a->res_pe)
        LIME_REQUIRE(a->res_period > 0 && a->ldr_pe >= a->E && lime_al16(a->res_pe, a->ldr_pe), LIME_ERR_BAD_ARG,
                     "lime_encoder_oproj_sp: res_pe needs res_period > 0 and 16-byte aligned rows (ldr_pe %% 4 == 0)");
    LIME_REQUIRE(a->ldo >= a->E && lime_al16(a->out, a->ldo), LIME_ERR_BAD_ARG,
                 "lime_encoder_oproj_sp: out rows must be 16-byte aligned (ldo %% 4 == 0)");
    const long lim = 0x7FFFFFF0L;
    LIME_REQUIRE(128L * a->lda * 4 < lim && 128L * a->ldo * 4 < lim && (!a->res_pe || (long)a->res_period * a->ldr_pe * 4 < lim), LIME_ERR_UNSUPPORTED,
                 "lime_encoder_oproj_sp: operand too large for 32-bit offsets");
    if (a->M == 0) return LIME_OK;
    OprojSpP p{};
    p.a = a->attn; p.lda = a->lda; p.wp = a->wp;
    p.bias = a->bias; p.g = a->ln_gamma; p.beta = a->ln_beta; p.eps = a->ln_eps;
    p.res = a->res; p.ldr = a->ldr; p.ids = a->res_ids; p.pe = a->res_pe; p.ldpe = a->ldr_pe; p.period = a->res_period;
    p.out = a->out; p.ldo = a->ldo; p.M = a->M; p.E = a->E; p.m_dev = a->m_dev;
    const long ntiles = ((long)a->M + BM - 1) / BM;
    hipLaunchKernelGGL(oproj_sp_kernel, dim3((unsigned)lime_persistent_grid(ntiles)), dim3(NTHR), 0, (hipStream_t)stream, p);
    return lime_check_launch("lime_encoder_oproj_sp");
}
