// lime_lstm_step_f32 / lime_lstm_step_bwd_f32 / lime_mask_lengths: ONE time step of a bidirectional single-layer LSTM (nn.LSTM's
// cell and parameter layout: gate order i, f, g, o; weight_hh [4h, h]) over R sequences of T token slots with per-sequence lengths --
// the recurrence of the CNE content encoder (newsEncoders.py:439-532 of the reference).
//
// The input projection x_t W_ih^T + b_ih + b_hh of every token and both directions is ONE lime_linear_f32 launch ahead of the time
// loop (gi [R T, 2 . 4h]); a step is then h_{t-1} W_hh^T + gi_t followed by the gate arithmetic.  Work split of the forward step: a
// workgroup owns 64 sequences x 16 hidden units x ALL FOUR gates of those units of one direction, as four 16 x 16 accumulators per wave
// of the transposed product D^T = W_hh h^T on v_mfma_f32_16x16x4_f32 (dev_helpers.h mfma16): lane (fi, kg) ends up with sequence fi and
// units 4 kg .. 4 kg + 3 of every gate, so sigma / tanh, c' = f c + i g and h' = o tanh(c') are epilogue arithmetic on its own
// accumulators -- no LDS exchange, no [R, 4h] pre-activation round trip through memory.  Operands go global -> registers -> LDS
// (two 16-deep stages, one barrier per chunk, the next chunk's loads in flight under this chunk's MFMAs); every wait is vmcnt(0).
//
// The previous hidden state is read from the output buffer itself (hout [R T, 2h]: forward columns of token t - 1, backward columns of
// token t + 1), which the PREVIOUS launch wrote: the time loop is on the host, T launches, no cooperative launch, no grid barrier, no
// workgroup waits for another.  A workgroup whose 64 sequences are all past their length at this step returns at once.
//
// A (sequence, unit) result is one fixed-order fma chain over k (chunks in order, the MFMA's k slots in order): its bits do not depend on
// R, on the sequence's position, on n_rows_dev or on the run.  No atomics anywhere in this file.
#include "common.h"
#include "dev_helpers.h"

using namespace lime_dev;

namespace {

constexpr int RT = 64, UT = 16, KC = 16;             // sequences and hidden units of a workgroup; k depth of a chunk
constexpr int LSTM_STAGE = (RT + 4 * UT) * KC;       // floats of one LDS stage: the h_{t-1} rows, then the 4 x 16 W_hh rows

struct LstmP {
    const float* gi; long ldgi;
    const float* whh;            // [2, 4h, h]
    const int* len;              // [R]
    float* hout;                 // [R T, 2h]
    float* c;                    // [2, R, h]
    float* gates;                // [R T, 2 . 4h] activations i, f, g, o (training), or NULL
    float* c_seq;                // [R T, 2h] c_t (training)
    float* h_prev;               // [R T, 2h] h_{t-1} as the step read it (training)
    int R, T, h, step;
    const int* n_rows_dev;
};

__device__ __forceinline__ int clamp_len(int l, int T) { return l < 0 ? 0 : (l > T ? T : l); }

template <bool SAVE>
__global__ __launch_bounds__(256) void lstm_step_kernel(const LstmP p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * LSTM_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fi = lane & 15, kg = lane >> 4;
    const int dir = blockIdx.z, u0 = blockIdx.y * UT, row0 = blockIdx.x * RT;
    const int h = p.h, T = p.T, s = p.step;
    const int R = live_count(p.n_rows_dev, p.R);
    // every wave looks at the same 64 sequences (lane l: row0 + l), so the verdict is uniform over the workgroup
    {
        const int r = row0 + lane;
        const int l = r < R ? clamp_len(p.len[r], T) : 0;
        if (__builtin_amdgcn_ballot_w64(s < l) == 0ull) return;
    }

    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (s > 0) {                                     // at step 0 the previous state is zero: nothing is read
        // loader: thread -> one 16-byte piece of an h_{t-1} row and one of a W_hh row per chunk
        const int lrow = tid >> 2, lseg = tid & 3;
        const int lpos = lrow * KC + ((lseg ^ swz4((lrow >> 2) & 3)) * 4);
        const float* a_ptr = nullptr;
        {
            const int r = row0 + lrow;
            if (r < R) {
                const int l = clamp_len(p.len[r], T);
                if (s < l) {
                    const int tprev = dir == 0 ? s - 1 : l - s;
                    a_ptr = p.hout + ((long)r * T + tprev) * (2L * h) + (long)dir * h + lseg * 4;
                }
            }
        }
        const float* w_ptr = p.whh + ((long)dir * 4 * h + (long)(lrow >> 4) * h + u0 + (lrow & 15)) * h + lseg * 4;
        const int pseg = (kg ^ swz4((fi >> 2) & 3)) * 4;
        const int a_off = (16 * wave + fi) * KC + pseg, w_off = RT * KC + fi * KC + pseg;
        const int nchunk = h / KC;
        const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 ra = a_ptr ? *reinterpret_cast<const f32x4*>(a_ptr) : zero4;
        f32x4 rw = *reinterpret_cast<const f32x4*>(w_ptr);
        *reinterpret_cast<f32x4*>(lds + lpos) = ra;
        *reinterpret_cast<f32x4*>(lds + RT * KC + lpos) = rw;
        __syncthreads();
        for (int c = 0; c < nchunk; ++c) {
            const bool more = c + 1 < nchunk;
            if (more) {
                ra = a_ptr ? *reinterpret_cast<const f32x4*>(a_ptr + (c + 1) * KC) : zero4;
                rw = *reinterpret_cast<const f32x4*>(w_ptr + (c + 1) * KC);
            }
            const float* sb = lds + (c & 1) * LSTM_STAGE;
            const f32x4 af = *reinterpret_cast<const f32x4*>(sb + a_off);
            f32x4 wf[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) wf[g] = *reinterpret_cast<const f32x4*>(sb + w_off + g * UT * KC);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = mfma16(wf[g][q], af[q], acc[g]);
            if (more) {                              // the other stage: every wave read it an iteration (and a barrier) ago
                float* nb = lds + ((c + 1) & 1) * LSTM_STAGE;
                *reinterpret_cast<f32x4*>(nb + lpos) = ra;
                *reinterpret_cast<f32x4*>(nb + RT * KC + lpos) = rw;
            }
            __syncthreads();
        }
    }

    // ---- epilogue: lane (fi, kg) holds sequence row0 + 16 wave + fi, units u0 + 4 kg .. + 3, all four gates ----------------------
    const int r = row0 + 16 * wave + fi;
    if (r >= R) return;
    const int l = clamp_len(p.len[r], T);
    if (s >= l) return;                              // frozen: state and hout rows stay as they are
    const int t = dir == 0 ? s : l - 1 - s;
    const long tok = (long)r * T + t;
    const int u = u0 + 4 * kg;
    const float* gi = p.gi + tok * p.ldgi + (long)dir * 4 * h + u;
    const f32x4 pi = acc[0] + *reinterpret_cast<const f32x4*>(gi);
    const f32x4 pf = acc[1] + *reinterpret_cast<const f32x4*>(gi + h);
    const f32x4 pg = acc[2] + *reinterpret_cast<const f32x4*>(gi + 2 * h);
    const f32x4 po = acc[3] + *reinterpret_cast<const f32x4*>(gi + 3 * h);
    float* const cp = p.c + ((long)dir * p.R + r) * h + u;
    f32x4 cv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) cv = *reinterpret_cast<const f32x4*>(cp);
    f32x4 vi, vf, vg, vo, hv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        vi[j] = lime_sigmoid(pi[j]);
        vf[j] = lime_sigmoid(pf[j]);
        vg[j] = tanhf(pg[j]);
        vo[j] = lime_sigmoid(po[j]);
        cv[j] = vf[j] * cv[j] + vi[j] * vg[j];
        hv[j] = vo[j] * tanhf(cv[j]);
    }
    *reinterpret_cast<f32x4*>(cp) = cv;
    const long ho = tok * (2L * h) + (long)dir * h + u;
    *reinterpret_cast<f32x4*>(p.hout + ho) = hv;
    if (SAVE) {
        float* gs = p.gates + tok * (8L * h) + (long)dir * 4 * h + u;
        *reinterpret_cast<f32x4*>(gs) = vi;
        *reinterpret_cast<f32x4*>(gs + h) = vf;
        *reinterpret_cast<f32x4*>(gs + 2 * h) = vg;
        *reinterpret_cast<f32x4*>(gs + 3 * h) = vo;
        *reinterpret_cast<f32x4*>(p.c_seq + ho) = cv;
        f32x4 hp = f32x4{0.f, 0.f, 0.f, 0.f};        // NOT hout shifted by a row: the first token of a direction has a zero past
        if (s > 0) hp = *reinterpret_cast<const f32x4*>(p.hout + ((long)r * T + (dir == 0 ? t - 1 : t + 1)) * (2L * h) + (long)dir * h + u);
        *reinterpret_cast<f32x4*>(p.h_prev + ho) = hp;
    }
}

struct LstmBwdP {
    const float* dhout; long lddh;   // [R T, 2h] or NULL
    const float* gates; const float* c_seq; const int* len;
    const float* dh;                 // [2, R, h] carry through W_hh (read)
    float* dc;                       // [2, R, h] carry, in place
    float* dgi;                      // [R T, 2 . 4h]
    float* dgs;                      // [2, R, 4h]: this step's pre-activation gradients, zeros for frozen rows
    int R, T, h, step;
};

// One lane per (direction, sequence, four units): the gate gradients of step `step`.  The dh carry of the NEXT (earlier) step is
// dgs W_hh, which the caller takes with lime_linear_group_f32 (frozen rows: zeros in, zeros out -- their carry is zero until they wake).
__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(const LstmBwdP p) {
    const int h = p.h, h4 = h >> 2, T = p.T, s = p.step;
    const long total = 2L * p.R * h4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int u = (int)(idx % h4) * 4;
        const long dr = idx / h4;
        const int r = (int)(dr % p.R), dir = (int)(dr / p.R);
        const int l = clamp_len(p.len[r], T);
        float* const gs = p.dgs + dr * (4L * h) + u;
        const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if (s >= l) {
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(gs + (long)g * h) = zero4;
            continue;
        }
        const int t = dir == 0 ? s : l - 1 - s;
        const long tok = (long)r * T + t;
        const long ho = tok * (2L * h) + (long)dir * h + u;
        const float* ga = p.gates + tok * (8L * h) + (long)dir * 4 * h + u;
        const f32x4 vi = *reinterpret_cast<const f32x4*>(ga), vf = *reinterpret_cast<const f32x4*>(ga + h),
                    vg = *reinterpret_cast<const f32x4*>(ga + 2 * h), vo = *reinterpret_cast<const f32x4*>(ga + 3 * h);
        const f32x4 ct = *reinterpret_cast<const f32x4*>(p.c_seq + ho);
        f32x4 cprev = zero4;
        if (s > 0) cprev = *reinterpret_cast<const f32x4*>(p.c_seq + ((long)r * T + (dir == 0 ? t - 1 : t + 1)) * (2L * h) + (long)dir * h + u);
        f32x4 dh = *reinterpret_cast<const f32x4*>(p.dh + dr * h + u);
        if (p.dhout) dh += *reinterpret_cast<const f32x4*>(p.dhout + tok * p.lddh + (long)dir * h + u);
        float* const dcp = p.dc + dr * h + u;
        f32x4 dc = *reinterpret_cast<const f32x4*>(dcp);
        f32x4 di, df, dg, dou;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float tc = tanhf(ct[j]);
            dc[j] += dh[j] * vo[j] * (1.f - tc * tc);
            dou[j] = dh[j] * tc * vo[j] * (1.f - vo[j]);
            di[j] = dc[j] * vg[j] * vi[j] * (1.f - vi[j]);
            df[j] = dc[j] * cprev[j] * vf[j] * (1.f - vf[j]);
            dg[j] = dc[j] * vi[j] * (1.f - vg[j] * vg[j]);
            dc[j] *= vf[j];
        }
        *reinterpret_cast<f32x4*>(dcp) = dc;
        float* const go = p.dgi + tok * (8L * h) + (long)dir * 4 * h + u;
        *reinterpret_cast<f32x4*>(go) = di;
        *reinterpret_cast<f32x4*>(go + h) = df;
        *reinterpret_cast<f32x4*>(go + 2 * h) = dg;
        *reinterpret_cast<f32x4*>(go + 3 * h) = dou;
        *reinterpret_cast<f32x4*>(gs) = di;
        *reinterpret_cast<f32x4*>(gs + h) = df;
        *reinterpret_cast<f32x4*>(gs + 2L * h) = dg;
        *reinterpret_cast<f32x4*>(gs + 3L * h) = dou;
    }
}

// len[r] = max(number of non-zero mask bytes of row r, min_len)
__global__ __launch_bounds__(256) void mask_lengths_kernel(const unsigned char* __restrict__ mask, int R, int T, int min_len, int* __restrict__ len) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    int n = 0;
    for (int t = 0; t < T; ++t) n += mask[(long)r * T + t] ? 1 : 0;
    len[r] = n < min_len ? min_len : n;
}

// mode 0: out = x * sigmoid(g) (g dense, [rows, cols]); mode 1: out[r] = x[r] * g[r / div] * scale (one g row per div rows)
// (mode 0 may run in place, out == g: a lane reads its element before it writes it; hence no __restrict__ on the two)
__global__ __launch_bounds__(256) void gate_mul_kernel(const float* __restrict__ x, const float* g, float* out, long rows,
                                                       int cols4, int div, int mode, float scale, const int* __restrict__ n_rows_dev) {
    if (n_rows_dev) {
        const long m = *n_rows_dev;
        rows = m < rows ? (m < 0 ? 0 : m) : rows;
    }
    const long total = rows * cols4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long r = idx / cols4;
        const int c4 = (int)(idx - r * cols4);
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[idx];
        f32x4 o;
        if (mode == 0) {
            const f32x4 gv = reinterpret_cast<const f32x4*>(g)[idx];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = xv[j] * lime_sigmoid(gv[j]);
        } else {
            const f32x4 gv = reinterpret_cast<const f32x4*>(g)[(r / div) * cols4 + c4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = xv[j] * gv[j] * scale;
        }
        reinterpret_cast<f32x4*>(out)[idx] = o;
    }
}

}  // namespace

static bool lstm_dims_ok(int R, int T, int h) { return R >= 0 && T >= 1 && h >= 16 && h % 16 == 0 && (long)R * T < 0x7FFFFFFFL && R <= 65535 * RT; }

extern "C" int lime_lstm_step_f32(const float* gi, int64_t ldgi, const float* whh, const int32_t* len, float* hout, float* c, float* gates,
                                  float* c_seq, float* h_prev, int32_t R, int32_t T, int32_t h, int32_t step, const int32_t* n_rows_dev,
                                  void* stream) {
    LIME_REQUIRE(gi && whh && len && hout && c, LIME_ERR_BAD_ARG, "lime_lstm_step_f32: NULL pointer");
    LIME_REQUIRE((gates != nullptr) == (c_seq != nullptr) && (gates != nullptr) == (h_prev != nullptr), LIME_ERR_BAD_ARG,
                 "lime_lstm_step_f32: gates, c_seq and h_prev are given together or not at all");
    LIME_REQUIRE(lstm_dims_ok(R, T, h), LIME_ERR_UNSUPPORTED,
                 "lime_lstm_step_f32: R=%d T=%d h=%d: the hidden size must be a multiple of 16 (a workgroup owns 16 units with their four gates)", R, T, h);
    LIME_REQUIRE(step >= 0 && step < T && ldgi >= 8L * h, LIME_ERR_BAD_ARG, "lime_lstm_step_f32: step %d outside 0 .. T - 1 or ldgi < 8 h", step);
    LIME_REQUIRE(lime_al16(gi, ldgi) && lime_al16(whh, h) && lime_al16(hout, h) && lime_al16(c, h) && lime_al16(gates, h) && lime_al16(c_seq, h) &&
                 lime_al16(h_prev, h), LIME_ERR_BAD_ARG, "lime_lstm_step_f32: operands must be 16-byte aligned, ldgi a multiple of 4");
    if (R == 0) return LIME_OK;
    LstmP p{gi, (long)ldgi, whh, len, hout, c, gates, c_seq, h_prev, R, T, h, step, n_rows_dev};
    const dim3 grid((unsigned)((R + RT - 1) / RT), (unsigned)(h / UT), 2);
    if (gates) hipLaunchKernelGGL(lstm_step_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(lstm_step_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, p);
    return lime_check_launch("lime_lstm_step_f32");
}

extern "C" int lime_lstm_step_bwd_f32(const float* dhout, int64_t lddh, const float* gates, const float* c_seq, const int32_t* len,
                                      const float* dh, float* dc, float* dgi, float* dgs, int32_t R, int32_t T, int32_t h, int32_t step,
                                      void* stream) {
    LIME_REQUIRE(gates && c_seq && len && dh && dc && dgi && dgs, LIME_ERR_BAD_ARG, "lime_lstm_step_bwd_f32: NULL pointer");
    LIME_REQUIRE(lstm_dims_ok(R, T, h), LIME_ERR_UNSUPPORTED, "lime_lstm_step_bwd_f32: R=%d T=%d h=%d: the hidden size must be a multiple of 16", R, T, h);
    LIME_REQUIRE(step >= 0 && step < T && (!dhout || lddh >= 2L * h), LIME_ERR_BAD_ARG, "lime_lstm_step_bwd_f32: step %d outside 0 .. T - 1 or lddh < 2 h", step);
    LIME_REQUIRE(lime_al16(dhout, lddh) && lime_al16(gates, h) && lime_al16(c_seq, h) && lime_al16(dh, h) && lime_al16(dc, h) && lime_al16(dgi, h) &&
                 lime_al16(dgs, h), LIME_ERR_BAD_ARG, "lime_lstm_step_bwd_f32: operands must be 16-byte aligned, lddh a multiple of 4");
    if (R == 0) return LIME_OK;
    LstmBwdP p{dhout, (long)lddh, gates, c_seq, len, dh, dc, dgi, dgs, R, T, h, step};
    hipLaunchKernelGGL(lstm_step_bwd_kernel, dim3(lime_grid_cap(2L * R * (h / 4), 256, 8 * lime_num_cus())), dim3(256), 0, (hipStream_t)stream, p);
    return lime_check_launch("lime_lstm_step_bwd_f32");
}

extern "C" int lime_mask_lengths(const uint8_t* mask, int32_t R, int32_t T, int32_t min_len, int32_t* len, void* stream) {
    LIME_REQUIRE(mask && len, LIME_ERR_BAD_ARG, "lime_mask_lengths: NULL pointer");
    LIME_REQUIRE(R >= 0 && T >= 1 && min_len >= 0 && min_len <= T, LIME_ERR_BAD_ARG, "lime_mask_lengths: bad dims R=%d T=%d min_len=%d", R, T, min_len);
    if (R == 0) return LIME_OK;
    hipLaunchKernelGGL(mask_lengths_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask, R, T, min_len, len);
    return lime_check_launch("lime_mask_lengths");
}

extern "C" int lime_gate_mul_f32(const float* x, const float* g, float* out, int64_t rows, int32_t cols, int32_t div, int32_t mode, float scale,
                                 const int32_t* n_rows_dev, void* stream) {
    LIME_REQUIRE(x && g && out, LIME_ERR_BAD_ARG, "lime_gate_mul_f32: NULL pointer");
    LIME_REQUIRE(rows >= 0 && cols > 0 && cols % 4 == 0 && div >= 1 && (mode == 0 || mode == 1) && (mode == 1 || div == 1), LIME_ERR_BAD_ARG,
                 "lime_gate_mul_f32: bad dims rows=%ld cols=%d div=%d mode=%d (cols must be a multiple of 4)", (long)rows, cols, div, mode);
    LIME_REQUIRE(lime_al16(x, cols) && lime_al16(g, cols) && lime_al16(out, cols), LIME_ERR_BAD_ARG, "lime_gate_mul_f32: operands must be 16-byte aligned");
    if (rows == 0) return LIME_OK;
    hipLaunchKernelGGL(gate_mul_kernel, dim3(lime_grid_cap(rows * (cols / 4), 256, 16 * lime_num_cus())), dim3(256), 0, (hipStream_t)stream, x, g, out,
                       (long)rows, cols / 4, div, mode, scale, n_rows_dev);
    return lime_check_launch("lime_gate_mul_f32");
}
