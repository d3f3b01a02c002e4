// lime_conv1d_window_f32 / lime_conv1d_wgrad_f32: the 1-D convolution over the tokens of a sequence (layers.py:98-135, the CNN
// content encoder's Conv1D) as a GEMM whose A operand is a gathered window, with the split product of gemm_sp_f32.hip (each fp32
// operand = three bf16 terms, six v_mfma_f32_16x16x32_bf16 per block, fp32 accumulation: the error of one fp32 rounding per
// product).  lime_set_split_gemm(0) switches both kernels to v_mfma_f32_16x16x4_f32 on the same fp32 LDS images (exact-fp32 MFMA).
//
//   out[r, o] = (accumulate ? out[r, o] : 0) + act(bias[o] + sum_j sum_c A(r, j)[c] W[o, j C + c])
//   A(r, j) = source row s T + t + j - pad  (r = s T + t, pad = (window - 1) / 2), zeros where t + j - pad is outside [0, T)
//   source row q = table[ids[q]] (gathered word embedding) or a[q] (ids == NULL: a dense fp32 matrix)
//
// No im2col matrix exists: the K loop runs over (tap j, 32-deep chunk q of the C source columns) and every chunk's A rows are
// fetched straight from the table / dense rows of tap j.  K per tap is padded to whole 32-column chunks: the A and W loads of a
// 16-byte segment past column C are masked to zeros (W needs no repacking beyond [O, window, C]), so a chunk never straddles taps.
// C % 4 == 0 (a segment is valid or not as a whole).
//
// Structure: the tile product is conv_frag.h's conv_tile_product (shared with conv_pool_sp_f32.hip): 256-thread workgroups (four
// waves), tile 128 rows x 128 columns, wave w owns rows 64 (w & 1) .. + 63 and columns 64 (w >> 1) .. + 63 (4 x 4 accumulator tiles
// of 16 x 16, the transposed product D^T = W A^T so that a lane holds four consecutive output columns of one row).  Chunks go
// global -> registers -> LDS (fp32, 144-byte rows), two stages, one barrier per chunk (conv_frag.h's two_stage_loop): chunk k + 1's
// loads are in flight while chunk k is split and multiplied.  74 KB of LDS: two workgroups per CU.  This file passes its single
// source as the tap and M as the row end, and keeps the epilogue.
// The epilogue honours a device-side row count (m_dev: rows >= min(*m_dev, M) are neither computed nor stored) and an output
// leading dimension (the group3 convolutions write their column slices of one output).
//
// The data gradient is the same kernel: dX(r)[c] = sum_j' dY(r + j' - pad)[:] . Wd[c, j' O + :] with the dense dY as the source and
// Wd[c, j', o] = W[o, c, window - 1 - j'] (taps reversed; the caller repacks), accumulate = 1 for the second and third group3 conv.
//
// The weight gradient dW[o, j C + c] = sum_r dY[r, o] A(r, j)[c] (conv_wgrad_sp_kernel) reads the same windowed operand: tiles of
// 64 o x 128 c of one tap over one slice of the rows, both operands stored into LDS transposed ([column][row]) so that a fragment
// (eight consecutive rows of one column) is one 32-byte read, its own load / store / product bodies in the same two_stage_loop; the
// slices' partial tiles go to a workspace and are summed in slice order by conv_wgrad_reduce_kernel -- no atomics, the same bits on
// every run.
#include "conv_frag.h"

using namespace lime_dev;

int lime_split_mode();

namespace {

struct ConvParams {
    const float* a;
    long lda;
    const int* ids;
    const float* w;
    long ldw;
    const float* bias;
    float* c;
    long ldc;
    const int* m_dev;
    int M, N, C, T, win, pad, relu, accumulate, vec_out, n_col_blocks;
};

constexpr int BM = CONV_BM, BN = CONV_BN;

template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void conv_sp_kernel(const ConvParams p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * CONV_STAGE];
    const int M = live_count(p.m_dev, p.M);
    const int rb = blockIdx.x / p.n_col_blocks, cb = blockIdx.x - rb * p.n_col_blocks;
    const int row0 = rb * BM, col0 = cb * BN;
    if (row0 >= M) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave & 1, wc = wave >> 1;
    const int fi = lane & 15, kg = lane >> 4;

    f32x4 acc[4][4];
    conv_tile_product<SPLIT>(lds, acc, [&p](int j) { return ConvTap{p.a, p.lda, p.ids, j}; }, p.win, p.w, p.ldw, p.C, p.N, p.T, p.pad,
                             row0, M, col0);

    // epilogue: lane (fi, kg) holds row 64 wr + 16 i + fi, columns 64 wc + 16 t + 4 kg + e in acc[i][t][e]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = row0 + 64 * wr + 16 * i + fi;
        if (r >= M) continue;
        float* const crow = p.c + (long)r * p.ldc;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = col0 + 64 * wc + 16 * t + 4 * kg;
            if (n >= p.N) continue;
            f32x4 v = acc[i][t];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float y = v[e] + ((p.bias && n + e < p.N) ? p.bias[n + e] : 0.f);
                if (p.relu) y = fmaxf(y, 0.f);
                v[e] = y;
            }
            if (p.vec_out) {                           // N % 4 == 0, 16-byte rows: a segment is valid as a whole
                if (p.accumulate) v = ld4(crow + n) + v;
                *reinterpret_cast<f32x4*>(crow + n) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (n + e < p.N) crow[n + e] = p.accumulate ? crow[n + e] + v[e] : v[e];
                }
            }
        }
    }
}

// ---- weight gradient -------------------------------------------------------------------------------------------------
constexpr int BO = 64, BC = 128;
constexpr int WY_FL = BO * CONV_PITCH, WX_FL = BC * CONV_PITCH, WSTAGE = WY_FL + WX_FL;
static_assert(2 * WSTAGE * 4 <= 81920, "two workgroups per CU");

struct WgradParams {
    const float* dy;
    long ldy;
    const float* a;
    long lda;
    const int* ids;
    float* ws;                                         // [splits][N][win C]
    int M, N, C, T, win, pad, n_o_blocks, n_c_blocks, rows_per_split;
};

template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void conv_wgrad_sp_kernel(const WgradParams p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * WSTAGE];
    const int per_split = p.n_o_blocks * p.win * p.n_c_blocks;
    const int split = blockIdx.x / per_split;
    int rest = blockIdx.x - split * per_split;
    const int ob = rest / (p.win * p.n_c_blocks);
    rest -= ob * (p.win * p.n_c_blocks);
    const int j = rest / p.n_c_blocks, cblk = rest - j * p.n_c_blocks;
    const int o0 = ob * BO, c0 = cblk * BC;
    const int m_begin = split * p.rows_per_split;
    const int m_end = m_begin + p.rows_per_split < p.M ? m_begin + p.rows_per_split : p.M;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave & 1, wk = wave >> 1;
    const int fi = lane & 15, kg = lane >> 4;
    const int nk = (m_end - m_begin + CONV_KC - 1) / CONV_KC;

    // loader: dY chunk [32 rows][64 o] = 2 segments per thread (row (tid >> 4) + 16 u, o 4 (tid & 15)); X chunk [32 rows][128 c] =
    // 4 segments (row (tid >> 5) + 8 u, c 4 (tid & 31)); both stored transposed: image[column][row]
    f32x4 ry[2], rx[4];
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    auto gload = [&](int k) {
        const int m0 = m_begin + k * CONV_KC;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = m0 + (tid >> 4) + 16 * u, o = o0 + 4 * (tid & 15);
            ry[u] = (r < m_end && o < p.N) ? ld4(p.dy + (long)r * p.ldy + o) : z;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = m0 + (tid >> 5) + 8 * u, c = c0 + 4 * (tid & 31);
            const long off = (r < m_end && c < p.C) ? window_row(p.ids, p.lda, r, j, p.pad, p.T) : -1;
            rx[u] = off >= 0 ? ld4(p.a + off + c) : z;
        }
    };
    auto sstore = [&](int st) {
        float* const sy = lds + st * WSTAGE;
        float* const sx = sy + WY_FL;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = (tid >> 4) + 16 * u, o = 4 * (tid & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) sy[(o + e) * CONV_PITCH + r] = ry[u][e];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = (tid >> 5) + 8 * u, c = 4 * (tid & 31);
#pragma unroll
            for (int e = 0; e < 4; ++e) sx[(c + e) * CONV_PITCH + r] = rx[u][e];
        }
    };

    // wave (wo, wk): o rows 32 wo + 16 i (i < 2), c columns 64 wk + 16 t (t < 4); D^T = X^T dY: lane holds c = 4 kg + e, o = fi
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto compute = [&](int st) {
        const float* const sy = lds + st * WSTAGE + (32 * wo + fi) * CONV_PITCH + 8 * kg;
        const float* const sx = lds + st * WSTAGE + WY_FL + (64 * wk + fi) * CONV_PITCH + 8 * kg;
        Frag<SPLIT> y[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) y[i].load_frag(sy + i * 16 * CONV_PITCH);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            Frag<SPLIT> x;
            x.load_frag(sx + t * 16 * CONV_PITCH);
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[i][t] = frag_prod(x, y[i], acc[i][t]);
        }
    };

    if (nk > 0) two_stage_loop(nk, gload, sstore, compute);
    // partial tile -> workspace slice `split` (every element of the [N][win C] slice that this tile covers is written, zeros for an
    // empty row range, so the reduction never reads stale data)
    const long ldw = (long)p.win * p.C;
    float* const wsp = p.ws + (long)split * p.N * ldw;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int o = o0 + 32 * wo + 16 * i + fi;
        if (o >= p.N) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = c0 + 64 * wk + 16 * t + 4 * kg;
            if (c < p.C) *reinterpret_cast<f32x4*>(wsp + (long)o * ldw + (long)j * p.C + c) = acc[i][t];
        }
    }
}

// dw[o, k] (+)= sum over the splits in order of ws[s][o][k]
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ ws, int splits, long slice, float* dw, long lddw,
                                                                int N, long K, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * K) return;
    const int o = (int)(i / K);
    const long k = i - (long)o * K;
    float t = 0.f;
    for (int s = 0; s < splits; ++s) t += ws[(long)s * slice + i];
    float* const q = dw + (long)o * lddw + k;
    *q = accumulate ? *q + t : t;
}

struct WgradPlan {
    int n_o_blocks, n_c_blocks, splits, rows_per_split;
};
WgradPlan wgrad_plan(int M, int N, int C, int win) {
    WgradPlan w;
    w.n_o_blocks = (N + BO - 1) / BO;
    w.n_c_blocks = (C + BC - 1) / BC;
    const long ntile = (long)w.n_o_blocks * win * w.n_c_blocks;
    long splits = 512 / (ntile > 0 ? ntile : 1);           // about two workgroups per CU
    const long max_splits = ((long)M + 255) / 256;          // at least 8 chunks per workgroup
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    long rps = ((long)M + splits - 1) / splits;
    rps = (rps + CONV_KC - 1) / CONV_KC * CONV_KC;
    w.rows_per_split = (int)rps;
    w.splits = (int)(((long)M + rps - 1) / rps);
    if (w.splits < 1) w.splits = 1;
    return w;
}

}  // namespace

extern "C" int lime_conv1d_window_f32(const float* a, int64_t lda, const int32_t* ids, const float* w, int64_t ldw, const float* bias,
                                      float* out, int64_t ldc, int32_t M, int32_t N, int32_t C, int32_t T, int32_t window, int32_t act,
                                      int32_t accumulate, const int32_t* m_dev, void* stream) {
    LIME_REQUIRE(a && w && out, LIME_ERR_BAD_ARG, "lime_conv1d_window_f32: null pointer");
    LIME_REQUIRE(M > 0 && N > 0 && C > 0 && T > 0 && window > 0, LIME_ERR_BAD_ARG, "lime_conv1d_window_f32: non-positive dimension");
    LIME_REQUIRE(window % 2 == 1, LIME_ERR_UNSUPPORTED, "lime_conv1d_window_f32: window %d is even (the output would be T - 1 long)", window);
    LIME_REQUIRE(M % T == 0, LIME_ERR_BAD_ARG, "lime_conv1d_window_f32: M = %d is not a whole number of sequences of T = %d", M, T);
    LIME_REQUIRE(lda >= C && ldw >= (int64_t)window * C && ldc >= N, LIME_ERR_BAD_ARG,
                 "lime_conv1d_window_f32: leading dimension smaller than the row");
    LIME_REQUIRE(C % 4 == 0 && lda % 4 == 0 && ldw % 4 == 0 && lime_al16(a, 0) && lime_al16(w, 0), LIME_ERR_UNSUPPORTED,
                 "lime_conv1d_window_f32: C, lda, ldw must be multiples of 4 and a, w 16-byte aligned");
    LIME_REQUIRE(act == LIME_ACT_NONE || act == LIME_ACT_RELU, LIME_ERR_UNSUPPORTED, "lime_conv1d_window_f32: act %d (none / relu only)", act);
    LIME_REQUIRE((long)M * lda < 0x7FFFFFFFL * 4L, LIME_ERR_UNSUPPORTED, "lime_conv1d_window_f32: operand too large");
    ConvParams p;
    p.a = a; p.lda = lda; p.ids = ids; p.w = w; p.ldw = ldw; p.bias = bias; p.c = out; p.ldc = ldc; p.m_dev = m_dev;
    p.M = M; p.N = N; p.C = C; p.T = T; p.win = window; p.pad = (window - 1) / 2;
    p.relu = act == LIME_ACT_RELU; p.accumulate = accumulate != 0;
    p.vec_out = (N % 4 == 0 && ldc % 4 == 0 && lime_al16(out, 0)) ? 1 : 0;
    p.n_col_blocks = (N + BN - 1) / BN;
    const long grid = (long)((M + BM - 1) / BM) * p.n_col_blocks;
    LIME_REQUIRE(grid < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_conv1d_window_f32: grid too large");
    hipStream_t s = (hipStream_t)stream;
    if (lime_split_mode() & 1) conv_sp_kernel<true><<<(unsigned)grid, 256, 0, s>>>(p);
    else conv_sp_kernel<false><<<(unsigned)grid, 256, 0, s>>>(p);
    return lime_check_launch("lime_conv1d_window_f32");
}

extern "C" int64_t lime_conv1d_wgrad_workspace(int32_t M, int32_t N, int32_t C, int32_t window) {
    if (M <= 0 || N <= 0 || C <= 0 || window <= 0) return 0;
    const WgradPlan w = wgrad_plan(M, N, C, window);
    return (int64_t)w.splits * N * window * C;
}

extern "C" int lime_conv1d_wgrad_f32(const float* dy, int64_t ldy, const float* a, int64_t lda, const int32_t* ids, float* dw,
                                     int64_t lddw, int32_t M, int32_t N, int32_t C, int32_t T, int32_t window, int32_t accumulate,
                                     float* workspace, int64_t workspace_floats, void* stream) {
    LIME_REQUIRE(dy && a && dw && workspace, LIME_ERR_BAD_ARG, "lime_conv1d_wgrad_f32: null pointer");
    LIME_REQUIRE(M > 0 && N > 0 && C > 0 && T > 0 && window > 0, LIME_ERR_BAD_ARG, "lime_conv1d_wgrad_f32: non-positive dimension");
    LIME_REQUIRE(window % 2 == 1, LIME_ERR_UNSUPPORTED, "lime_conv1d_wgrad_f32: window %d is even", window);
    LIME_REQUIRE(M % T == 0, LIME_ERR_BAD_ARG, "lime_conv1d_wgrad_f32: M = %d is not a whole number of sequences of T = %d", M, T);
    LIME_REQUIRE(ldy >= N && lda >= C && lddw >= (int64_t)window * C, LIME_ERR_BAD_ARG,
                 "lime_conv1d_wgrad_f32: leading dimension smaller than the row");
    LIME_REQUIRE(N % 4 == 0 && C % 4 == 0 && ldy % 4 == 0 && lda % 4 == 0 && lime_al16(dy, 0) && lime_al16(a, 0) && lime_al16(workspace, 0), LIME_ERR_UNSUPPORTED,
                 "lime_conv1d_wgrad_f32: N, C, ldy, lda must be multiples of 4 and dy, a, workspace 16-byte aligned");
    const WgradPlan w = wgrad_plan(M, N, C, window);
    const long slice = (long)N * window * C;
    LIME_REQUIRE(workspace_floats >= (int64_t)w.splits * slice, LIME_ERR_BAD_ARG,
                 "lime_conv1d_wgrad_f32: workspace holds %lld floats, needs %lld", (long long)workspace_floats, (long long)(w.splits * slice));
    WgradParams p;
    p.dy = dy; p.ldy = ldy; p.a = a; p.lda = lda; p.ids = ids; p.ws = workspace;
    p.M = M; p.N = N; p.C = C; p.T = T; p.win = window; p.pad = (window - 1) / 2;
    p.n_o_blocks = w.n_o_blocks; p.n_c_blocks = w.n_c_blocks; p.rows_per_split = w.rows_per_split;
    const long grid = (long)w.splits * w.n_o_blocks * window * w.n_c_blocks;
    hipStream_t s = (hipStream_t)stream;
    if (lime_split_mode() & 1) conv_wgrad_sp_kernel<true><<<(unsigned)grid, 256, 0, s>>>(p);
    else conv_wgrad_sp_kernel<false><<<(unsigned)grid, 256, 0, s>>>(p);
    int rc = lime_check_launch("conv_wgrad_sp_kernel");
    if (rc != LIME_OK) return rc;
    const long K = (long)window * C;
    conv_wgrad_reduce_kernel<<<(unsigned)((N * K + 255) / 256), 256, 0, s>>>(workspace, w.splits, slice, dw, lddw, N, K, accumulate != 0);
    return lime_check_launch("conv_wgrad_reduce_kernel");
}
