// lime_encoder_ffn_sp: the fp32 feed-forward half of an encoder layer (linear1, ReLU, linear2, residual, norm2, and the token mean
// pooling behind the last layer) in ONE launch with split products on the bf16 matrix cores (gemm_sp_f32.hip: three bf16 terms per
// fp32 operand, six MFMAs per 16 x 16 x 32 block).  Replaces two gemm_sp_kernel launches whose 512-wide hidden state made an HBM round
// trip (2 KB written and read back per token) and whose LayerNorm launch filled the chip badly at the title shape.
//
//   * a workgroup (8 waves, two per SIMD, one workgroup per CU) owns a 128-token tile; wave w owns tokens 16 w .. 16 w + 15 x all
//     304 model columns: 19 accumulator tiles for linear2 stay in registers through the whole tile.  Two waves share a SIMD so that
//     one's waits (LDS fragments, the step's vmcnt(0), the register splits, the epilogue's loads) leave the matrix pipe to the other.
//   * the hidden state runs in passes of 128 columns.  Linear1 (five steps, two 32-deep k chunks each): the layer input's fragments
//     are read straight from global memory (a wave's tokens are its own; the rows are L2 resident after the first pass) one step
//     ahead, split in registers; b1 is the accumulator init.  After ReLU the hidden tiles 2 kc, 2 kc + 1 are split in registers
//     and fed back as linear2's B operand IN REGISTER ORDER (four steps, one 32-wide hidden chunk each): the k index of an MFMA is
//     only a summation label, so linear2's weight columns are packed in the order the hidden registers come out (the trick of
//     ffn_bf16.hip).  No LDS round trip, no cross-lane movement for the hidden state.
//   * weights: pre-split into three bf16 term images by lime_ffn_pack_sp (inside the forward, or -- CROWN's scoring path -- once per weight
//     change, refilled in place before a graph replay: newsEncoders.WeightProducts), every step's slot ONE contiguous block in the order of its LDS image (swizzled [row][64-byte] rows: conflict-free
//     ds_read_b128 fragments), copied by LDS-DMA into two ring slots: step s + 1 is issued during step s (one instruction per
//     MFMA group), then one vmcnt(0) wait + barrier per step (the two-stage drain of gemm_sp_f32.hip).
//   * epilogue: + b2 + the residual rows (fp32, re-read: L2 hits, all 19 quads of a lane requested before the first is used),
//     LayerNorm (the four lanes that share a token meet through two shuffles), then fp32 rows or, with `pool32`, the 32-token
//     block means of the wave pair 2 b, 2 b + 1: the odd wave hands its normalised values to the even one through the ring slot the
//     tile's last step has just left.
//   * every load is branch-free and the next step's (behind a tile's last step: the next tile's) fragments are requested
//     unconditionally, so the only vmcnt waits of the tile loop are the one that ends each step and the epilogue's.
#include <type_traits>

#include "common.h"
#include "dev_helpers.h"
#include "split_mfma.h"

using namespace lime_dev;

namespace {

constexpr int NW = 8, NTHR = 64 * NW;        // waves per workgroup: two per SIMD
constexpr int BM = 16 * NW;                // tokens per tile: 128, one 16-token MFMA tile per wave
constexpr int ND = 19, DP = 16 * ND;       // model columns carried: 304
constexpr int NCH = 10;                    // 32-deep k chunks of the layer input (320 >= E)
constexpr int PW = 128;                    // hidden columns per pass
constexpr int NT1 = PW / 16;               // linear1 output tiles per pass
constexpr int L1_STEPS = NCH / 2;          // linear1 steps per pass (two chunks each)
constexpr int STEPS = L1_STEPS + PW / 32;  // per pass: five linear1 steps, four linear2 steps
constexpr int TERM1 = PW * 64;             // bytes of one term image of one linear1 chunk: [128 rows][32 bf16]
constexpr int CHUNK1 = 3 * TERM1;          // 24,576
constexpr int SLOT1 = 2 * CHUNK1;          // 49,152: a linear1 step
constexpr int TERM2 = DP * 64;             // [304 rows][32 bf16]
constexpr int SLOT2 = 3 * TERM2;           // 58,368: a linear2 step
constexpr int SLOT = SLOT2;
constexpr int CONST_OFF = 2 * SLOT;        // b2, gamma, beta [304] fp32, then b1 [F]
constexpr int F_MAX = 4096;
constexpr int LDS_BYTES = CONST_OFF + (3 * DP + F_MAX) * 4;      // 133,120 of the CU's 163,840

struct FfnSpP {
    const float* x; long ldx;
    const uint16_t* w1p; const uint16_t* w2p;
    const float* b1; const float* b2; const float* g; const float* beta; float eps;
    float* out; long ldo;
    int M, E, F;
    const int* m_dev;
};

template <bool POOL>
__global__ __launch_bounds__(NTHR, 1) void ffn_sp_kernel(const FfnSpP p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fi = lane & 15, kg = lane >> 4;
    const int M = live_count(p.m_dev, p.M);
    const int ntiles = (M + BM - 1) / BM;
    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    const int NP = p.F / PW;
    const int E = p.E;

    float* const cs = reinterpret_cast<float*>(lds + CONST_OFF);
    for (int c = tid; c < DP; c += NTHR) {
        cs[c] = c < E ? p.b2[c] : 0.f;
        cs[DP + c] = c < E ? p.g[c] : 0.f;
        cs[2 * DP + c] = c < E ? p.beta[c] : 0.f;
    }
    for (int c = tid; c < p.F; c += NTHR) cs[3 * DP + c] = p.b1[c];
    __syncthreads();                                   // nothing in flight yet

    const __amdgpu_buffer_rsrc_t rs_w1 = make_rsrc(p.w1p), rs_w2 = make_rsrc(p.w2p);
    // step s of a tile: pass s / 9, position s % 9 (0..4 linear1, 5..8 linear2).  The packed slot is one contiguous block: a slot of
    // n KB is n DMA instructions (1 KB each, lane l lands at +16 l), instruction i of wave w is block (8 i + w + rot) % n.  The
    // rotation by the CU's position in its XCD keeps the 32 CUs that share an L2 from asking for the same lines at the same moment.
    const int rot = (int)((blockIdx.x >> 3) * 5u);
    auto issue_one = [&](int s, int slot, int i) {
        const int pass = s / STEPS, pos = s - pass * STEPS;
        unsigned char* const dst = lds + slot * SLOT;
        if (pos < L1_STEPS) {
            constexpr int NI = SLOT1 / 1024;
            const int idx = NW * i + wave;
            if (idx < NI) {
                const int b = (idx + rot) % NI;
                dma16(rs_w1, dst + b * 1024, (unsigned)lane * 16u, (pass * L1_STEPS + pos) * SLOT1 + b * 1024);
            }
        } else {
            constexpr int NI = SLOT2 / 1024;
            const int idx = NW * i + wave;
            if (idx < NI) {
                const int b = (idx + rot) % NI;
                dma16(rs_w2, dst + b * 1024, (unsigned)lane * 16u, (pass * (PW / 32) + pos - L1_STEPS) * SLOT2 + b * 1024);
            }
        }
    };
    constexpr int DMA_PER_WAVE = (SLOT2 / 1024 + NW - 1) / NW;     // 8: at most this many instructions per wave and slot
    auto issue_w = [&](int s, int slot) {
        for (int i = 0; i < DMA_PER_WAVE; ++i) issue_one(s, slot, i);
    };
    // the layer input fragments of a linear1 step: chunks 2 pos, 2 pos + 1, k 8 kg .. 8 kg + 7 as two quads
    // (E % 4 == 0: a quad is real or beyond E as a whole; rows beyond M and quads beyond E read zeros).  Branch-free (dead_bit,
    // dev_helpers.h): as `cond ? offset : OOB` every load became two exec-masked loads with a vmcnt(0) between them.
    f32x4 xn[2][2];
    auto load_x = [&](int t, int pos) {
        const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(p.x + (long)t * BM * p.ldx);
        const int rows_left = M - t * BM;
        const int ln = lane_here(), fi = ln & 15, kg = ln >> 4;
        const int rl = 16 * wave + fi;
        const unsigned ro = (unsigned)rl * (unsigned)p.ldx * 4u;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int col = 32 * (2 * pos + cc) + 8 * kg + 4 * q;
                xn[cc][q] = buf_load4(rs_x, (ro + (unsigned)col * 4u) | dead_bit(rows_left - 1 - rl, E - 1 - col), 0);
            }
    };
    // vmcnt(0) with the fragments passed through it (wait_vm0_landed, dev_helpers.h): hipcc's own wait would sit in front of their
    // first use, at the top of the next step, behind that step's loads
    auto wait_x = [&]() {
        wait_vm0_landed(xn[0][0], xn[0][1], xn[1][0], xn[1][1]);
    };

    // MFMA lane layout (v_mfma_f32_16x16x32_bf16, a = weight rows = output columns, b = tokens): lane (fi, kg) reads k 8 kg .. 8 kg + 7
    // of row fi; the result is D^T: lane (token fi, kg) holds columns 16 t + 4 kg + r, r = 0..3
    const int w_off = fi * 64 + ((kg ^ swz4((fi >> 2) & 3)) * 16);
    auto wfrag = [&](const unsigned char* b, int term) {
        SplitFrag f;
        f.h = *reinterpret_cast<const bf16x8*>(b);
        f.m = *reinterpret_cast<const bf16x8*>(b + term);
        f.l = *reinterpret_cast<const bf16x8*>(b + 2 * term);
        return f;
    };
    f32x4 acc1[NT1], acc2[ND];

    // prologue: the first step of this workgroup's first tile
    issue_w(0, 0);
    load_x(tile, 0);
    wait_x();
    ring_barrier();
    int gs = 0;                                        // steps run by this workgroup (ring position)
    for (; tile < ntiles; tile += gridDim.x) {
        const bool last = tile + (int)gridDim.x >= ntiles;
#pragma unroll
        for (int t = 0; t < ND; ++t) acc2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        // step `pos` of pass `pass`: the fragments of its layer input (loaded one step ahead) leave xn before the next step's loads
        // reuse it; the next step goes into the other slot (everyone has left it: the barrier behind the previous step).  One weight
        // fragment (three terms) is read ahead of the MFMAs that use the previous one; sched_barriers keep hipcc from hoisting more.
        auto step = [&](auto pos_c, int pass) {
            constexpr int POS = decltype(pos_c)::value;
            const unsigned char* const sb = lds + (gs & 1) * SLOT + w_off;
            f32x4 xc[2][2];
            if constexpr (POS < L1_STEPS) {
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) { xc[cc][0] = xn[cc][0]; xc[cc][1] = xn[cc][1]; }
            }
            // the next step: its layer input fragments now, its weight slot one DMA instruction per MFMA group below (issued all at
            // once, a wave's 6-8 instructions queue in the CU's address path and the wave waits there before its first MFMA)
            const bool wrap = POS == STEPS - 1 && pass == NP - 1;
            const bool go = !(wrap && last);
            const int ns = wrap ? 0 : pass * STEPS + POS + 1;
            const int nslot = (gs + 1) & 1;
            // (unconditional: behind this workgroup's last tile every row is beyond M and nothing is read; under `if (go)` the
            // fragments become a phi whose copy waits for these loads ahead of the MFMAs)
            constexpr int NPOS = (POS + 1) % STEPS;
            if constexpr (NPOS < L1_STEPS) load_x(wrap ? tile + (int)gridDim.x : tile, NPOS);
            auto part = [&](int i) {
                if (go && i < DMA_PER_WAVE) issue_one(ns, nslot, i);
            };
            if constexpr (POS < L1_STEPS) {
                if constexpr (POS == 0) {              // b1 is the accumulator init of a pass
                    const float* const b1 = cs + 3 * DP + PW * pass + 4 * kg;
#pragma unroll
                    for (int t = 0; t < NT1; ++t) {
                        const f32x4 b = *reinterpret_cast<const f32x4*>(b1 + 16 * t);
                        acc1[t] = b;
                    }
                }
                SplitFrag w[2];
                w[0] = wfrag(sb, TERM1);
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) {
                    const SplitFrag x0 = split_frag(xc[cc][0], xc[cc][1]);
#pragma unroll
                    for (int t = 0; t < NT1; ++t) {
                        const int i = cc * NT1 + t;
                        if (i + 1 < 2 * NT1) w[(i + 1) & 1] = wfrag(sb + ((i + 1) / NT1) * CHUNK1 + ((i + 1) % NT1) * 1024, TERM1);
                        acc1[t] = split_mfma16(w[i & 1], x0, acc1[t]);
                        __builtin_amdgcn_sched_barrier(0);
                        part(i);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                if constexpr (POS == L1_STEPS - 1) {
#pragma unroll
                    for (int t = 0; t < NT1; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc1[t][r] = fmaxf(acc1[t][r], 0.f);
                }
            } else {
                // hidden chunk KC: tiles 2 KC and 2 KC + 1 side by side are the lane's 8 k slots (k = 32 KC + 16 a + 4 kg + r at slot
                // 4 a + r: the order lime_ffn_pack_sp gives linear2's weight columns)
                constexpr int KC = POS - L1_STEPS;
                const SplitFrag h0 = split_frag(acc1[2 * KC], acc1[2 * KC + 1]);
                SplitFrag w[2];
                w[0] = wfrag(sb, TERM2);
#pragma unroll
                for (int t = 0; t < ND; ++t) {
                    if (t + 1 < ND) w[(t + 1) & 1] = wfrag(sb + (t + 1) * 1024, TERM2);
                    acc2[t] = split_mfma16(w[t & 1], h0, acc2[t]);
                    __builtin_amdgcn_sched_barrier(0);
                    part(t);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (NPOS < L1_STEPS) wait_x();   // this wave's part of the next slot (and its layer input fragments)
            else wait_vm<0>();
            ring_barrier();                           // ... everyone's: the next slot is complete, this one is free
            ++gs;
        };
        for (int pass = 0; pass < NP; ++pass) {
            step(std::integral_constant<int, 0>{}, pass);
            step(std::integral_constant<int, 1>{}, pass);
            step(std::integral_constant<int, 2>{}, pass);
            step(std::integral_constant<int, 3>{}, pass);
            step(std::integral_constant<int, 4>{}, pass);
            step(std::integral_constant<int, 5>{}, pass);
            step(std::integral_constant<int, 6>{}, pass);
            step(std::integral_constant<int, 7>{}, pass);
            step(std::integral_constant<int, 8>{}, pass);
        }

        // ---- epilogue: + b2 + residual, LayerNorm over the E real columns (pad columns are exact zeros: zero weight rows, zero b2,
        // residual quads beyond E not read), then rows or 32-token block means
        const long row0 = (long)tile * BM;
        const __amdgpu_buffer_rsrc_t rs_r = make_rsrc(p.x + row0 * p.ldx);
        const int rows_left = M - (int)row0;
        const int le = lane_here(), fi = le & 15, kg = le >> 4;      // epilogue-only offsets are computed here, not carried through the tile
        const float* const cs_ = cs + 4 * kg;
        const float inv_n = 1.0f / (float)E;
        // the residual rows: all 19 quads of the lane's token are requested before the first is used (the fence: left alone, hipcc
        // sinks each load to its use and waits vmcnt(0) behind every one -- 19 round trips in a row per tile)
        const int rl = 16 * wave + fi;
        f32x4 rr[ND];
        {
            const unsigned ro = (unsigned)rl * (unsigned)p.ldx * 4u;
#pragma unroll
            for (int t = 0; t < ND; ++t) {
                const int col = 16 * t + 4 * kg;
                rr[t] = buf_load4(rs_r, (ro + (unsigned)col * 4u) | dead_bit(rows_left - 1 - rl, E - 1 - col), 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        float s1 = 0.f;
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            const f32x4 r = rr[t];
            const f32x4 b = *reinterpret_cast<const f32x4*>(cs_ + 16 * t);
            const f32x4 v = acc2[t] + b + r;
            acc2[t] = v;
            s1 += (v[0] + v[1]) + (v[2] + v[3]);
        }
        s1 += __shfl_xor(s1, 16);
        s1 += __shfl_xor(s1, 32);
        const float mean = s1 * inv_n;
        float s2 = 0.f;
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            if (16 * t + 4 * kg < E) {
                const f32x4 d = acc2[t] - mean;
                s2 += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
            }
        }
        s2 += __shfl_xor(s2, 16);
        s2 += __shfl_xor(s2, 32);
        const float rstd = rsqrtf(s2 * inv_n + p.eps);
        __builtin_amdgcn_sched_barrier(0);
        const float* const gs_ = cs_ + DP;
        const float* const es_ = cs_ + 2 * DP;
        auto norm = [&](int t) {
            const f32x4 ga = *reinterpret_cast<const f32x4*>(gs_ + 16 * t);
            const f32x4 be = *reinterpret_cast<const f32x4*>(es_ + 16 * t);
            return (acc2[t] - mean) * rstd * ga + be;
        };
        if constexpr (POOL) {
            // block row (row0 + 32 b) / 32: the column means over the 32 tokens of the wave pair 2 b, 2 b + 1 (all valid or all beyond
            // M).  The odd wave hands its normalised values to the even wave (same lane, same register: y = y_even + y_odd, then the
            // 16-lane sum, then 1/32) through the ring slot the tile's last step has just left -- the other one holds the next tile's
            // first step.  A slot takes 57 of the 76 KB the four pairs have: two rounds of ten and nine column tiles.  The barrier
            // behind the second round stands in front of the next tile's first step, whose DMA goes into this slot.
            constexpr int RT = (ND + 1) / 2;
            const int pair = wave >> 1;
            const bool odd = (wave & 1) != 0;
            f32x4* const stage = reinterpret_cast<f32x4*>(lds + ((gs + 1) & 1) * SLOT) + pair * RT * 64 + le;
            const int rl0 = 32 * pair;
            const __amdgpu_buffer_rsrc_t rs_p = make_rsrc(p.out + ((row0 + rl0) >> 5) * p.ldo);
            const bool rows_ok = rl0 < rows_left;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                constexpr int T1[2] = {RT, ND};
                if (odd) {
#pragma unroll
                    for (int t = RT * r; t < T1[r]; ++t) stage[(t - RT * r) * 64] = norm(t);
                }
                ring_barrier();
                if (!odd) {
#pragma unroll
                    for (int t = RT * r; t < T1[r]; ++t) {
                        f32x4 y = norm(t);
                        y += stage[(t - RT * r) * 64];
#pragma unroll
                        for (int j = 0; j < 4; ++j) y[j] = row16_sum(y[j]) * (1.0f / 32.0f);
                        const int col = 16 * t + 4 * kg;
                        buf_store4(y, rs_p, (rows_ok && fi == 0 && col < E) ? (unsigned)col * 4u : OOB, 0);
                    }
                }
                ring_barrier();
            }
        } else {
            const __amdgpu_buffer_rsrc_t rs_c = make_rsrc(p.out + row0 * p.ldo);
            const unsigned ro = (unsigned)rl * (unsigned)p.ldo * 4u;
#pragma unroll
            for (int t = 0; t < ND; ++t) {
                const int col = 16 * t + 4 * kg;
                buf_store4(norm(t), rs_c, (rl < rows_left && col < E) ? ro + (unsigned)col * 4u : OOB, 0);
            }
        }
    }
}

// The weights as the kernel's ring slots, three bf16 term images each (x = hi + mid + lo, split_pair's rounding), every slot one
// contiguous block in the order of its LDS image; row r's 32 bf16 are four 16-byte segments, logical segment kg at physical
// kg ^ swz4((r >> 2) & 3):
//   w1p [F / 128 passes][5 steps][2 chunks][3 terms][128 rows][32]: W1[128 pass + row, 32 (2 step + chunk) + k], zero for k >= E;
//   w2p [F / 32 chunks][3 terms][304 rows][32]: zero rows n >= E; logical position 8 kg + 4 a + r of a row holds
//   W2[n, 32 chunk + 16 a + 4 kg + r] -- the order in which the MFMA result registers of two neighbouring 16-column tiles (a = 0, 1)
//   of the hidden state sit in a lane.
__device__ __forceinline__ void split3(float v, uint16_t& h, uint16_t& m, uint16_t& l) {
    const SplitPair t = split_pair(v, 0.f);
    h = (uint16_t)(t.h & 0xFFFFu);
    m = (uint16_t)(t.m & 0xFFFFu);
    l = (uint16_t)(t.l & 0xFFFFu);
}
__global__ void ffn_sp_pack_kernel(const float* __restrict__ w1, long ldw1, const float* __restrict__ w2, long ldw2, int E, int F,
                                   uint16_t* __restrict__ w1p, uint16_t* __restrict__ w2p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n1 = (long)F * (NCH * 32), n2 = (long)F * DP;           // positions (three terms each)
    uint16_t h, m, l;
    if (i < n1) {
        const int pk = (int)(i & 31), row = (int)((i >> 5) % PW);
        const long chunk = i / (32 * PW);                              // pass * 10 + chunk
        const int c = (int)(chunk % NCH), pass = (int)(chunk / NCH);
        const int kg = (pk >> 3) ^ swz4((row >> 2) & 3), e = pk & 7;
        const int n = PW * pass + row, k = 32 * c + 8 * kg + e;
        split3(k < E ? w1[(long)n * ldw1 + k] : 0.f, h, m, l);
        uint16_t* const d = w1p + chunk * (3 * PW * 32) + row * 32 + pk;
        d[0] = h; d[PW * 32] = m; d[2 * PW * 32] = l;
    } else if (i < n1 + n2) {
        const long o = i - n1;
        const int pk = (int)(o & 31), n = (int)((o >> 5) % DP);
        const long blk = o / (32 * DP);
        const int kg = (pk >> 3) ^ swz4((n >> 2) & 3), a = (pk >> 2) & 1, r = pk & 3;
        split3(n < E ? w2[(long)n * ldw2 + 32 * blk + 16 * a + 4 * kg + r] : 0.f, h, m, l);
        uint16_t* const d = w2p + blk * (3 * DP * 32) + n * 32 + pk;
        d[0] = h; d[DP * 32] = m; d[2 * DP * 32] = l;
    }
}

}  // namespace

extern "C" int64_t lime_ffn_pack_sp_size(int32_t F, int32_t which) { return which == 0 ? (int64_t)F * (NCH * 32) * 3 : (int64_t)F * DP * 3; }

extern "C" int lime_ffn_pack_sp(const float* w1, int64_t ldw1, const float* w2, int64_t ldw2, int32_t E, int32_t F, uint16_t* w1p,
                                uint16_t* w2p, void* stream) {
    LIME_REQUIRE(w1 && w2 && w1p && w2p, LIME_ERR_BAD_ARG, "lime_ffn_pack_sp: NULL pointer");
    LIME_REQUIRE(E > 0 && E <= DP && E % 4 == 0 && F > 0 && F % PW == 0 && F <= F_MAX, LIME_ERR_UNSUPPORTED,
                 "lime_ffn_pack_sp: built for E <= %d, E %% 4 == 0 (E = %d) and F a multiple of %d up to %d (F = %d)", DP, E, PW, F_MAX, F);
    LIME_REQUIRE(ldw1 >= E && ldw2 >= F, LIME_ERR_BAD_ARG, "lime_ffn_pack_sp: leading dimension < row");
    const long n = (long)F * (NCH * 32) + (long)F * DP;
    hipLaunchKernelGGL(ffn_sp_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w1, (long)ldw1, w2,
                       (long)ldw2, E, F, w1p, w2p);
    return lime_check_launch("lime_ffn_pack_sp");
}

extern "C" int lime_encoder_ffn_sp(const lime_ffn_sp_args* a, void* stream) {
    LIME_REQUIRE(a != nullptr, LIME_ERR_BAD_ARG, "lime_encoder_ffn_sp: args is NULL");
    LIME_REQUIRE(a->x && a->w1p && a->w2p && a->b1 && a->b2 && a->ln_gamma && a->ln_beta && a->out, LIME_ERR_BAD_ARG,
                 "lime_encoder_ffn_sp: NULL pointer");
    LIME_REQUIRE(a->M >= 0 && a->E > 0 && a->E <= DP && a->E % 4 == 0 && a->F > 0 && a->F % PW == 0 && a->F <= F_MAX, LIME_ERR_UNSUPPORTED,
                 "lime_encoder_ffn_sp: built for E <= %d, E %% 4 == 0 (E = %d) and F a multiple of %d up to %d (F = %d)", DP, a->E, PW, F_MAX, a->F);
    LIME_REQUIRE(a->ldx >= a->E && a->ldx % 4 == 0 && (uintptr_t)a->x % 16 == 0, LIME_ERR_BAD_ARG,
                 "lime_encoder_ffn_sp: x rows must be 16-byte aligned (ldx %% 4 == 0)");
    LIME_REQUIRE((uintptr_t)a->w1p % 16 == 0 && (uintptr_t)a->w2p % 16 == 0, LIME_ERR_BAD_ARG,
                 "lime_encoder_ffn_sp: packed weights must be 16-byte aligned (see lime_ffn_pack_sp)");
    LIME_REQUIRE(a->pool32 == 0 || a->pool32 == 1, LIME_ERR_BAD_ARG, "lime_encoder_ffn_sp: pool32 must be 0 / 1");
    LIME_REQUIRE(a->ldo >= a->E && a->ldo % 4 == 0 && (uintptr_t)a->out % 16 == 0, LIME_ERR_BAD_ARG,
                 "lime_encoder_ffn_sp: out rows must be 16-byte aligned (ldo %% 4 == 0)");
    if (a->pool32) LIME_REQUIRE(a->M % 32 == 0, LIME_ERR_BAD_ARG, "lime_encoder_ffn_sp: pool32 needs M %% 32 == 0");
    const long lim = 0x7FFFFFF0L;
    LIME_REQUIRE(128L * a->ldx * 4 < lim && 128L * a->ldo * 4 < lim && (long)a->F * 320 * 6 < lim, LIME_ERR_UNSUPPORTED,
                 "lime_encoder_ffn_sp: operand too large for 32-bit offsets");
    if (a->M == 0) return LIME_OK;
    FfnSpP p{};
    p.x = a->x; p.ldx = a->ldx; p.w1p = a->w1p; p.w2p = a->w2p;
    p.b1 = a->b1; p.b2 = a->b2; p.g = a->ln_gamma; p.beta = a->ln_beta; p.eps = a->ln_eps;
    p.out = a->out; p.ldo = a->ldo; p.M = a->M; p.E = a->E; p.F = a->F; p.m_dev = a->m_dev;
    const long ntiles = ((long)a->M + BM - 1) / BM;
    const long nwg = lime_persistent_grid(ntiles);
    hipStream_t s = (hipStream_t)stream;
    if (a->pool32) hipLaunchKernelGGL((ffn_sp_kernel<true>), dim3((unsigned)nwg), dim3(NTHR), 0, s, p);
    else hipLaunchKernelGGL((ffn_sp_kernel<false>), dim3((unsigned)nwg), dim3(NTHR), 0, s, p);
    return lime_check_launch("lime_encoder_ffn_sp");
}
