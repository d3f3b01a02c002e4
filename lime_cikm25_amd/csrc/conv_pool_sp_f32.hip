// lime_conv_pool_f32 / lime_relu_maxpool_f32 / lime_relu_maxpool_bwd_f32: the knowledge-aware convolution of the KCNN content encoder
// (layers.py:138-190 Conv2D_Pool, newsEncoders.py:598-638) -- a 1-D convolution over the tokens of a sequence whose input is up to
// three [tokens, C] sources side by side (the word row and the two transformed entity rows), ReLU, and the maximum over the first P
// positions of the sequence -- as ONE windowed GEMM with the pooling in its epilogue:
//
//   pre[s, t, o] = bias[o] + sum_{src < n_src} sum_{j < win} sum_{c < C} X_src(s T + t + j - pad)[c] W[o, (src win + j) C + c]
//   pooled[s, o] = max(0, max_{t < P} pre[s, t, o]),   arg[s, o] = the smallest t that attains it, -1 where pooled is 0
//   X_src(q) = table_src[ids_src[q]] or a_src[q] (ids NULL), zeros where the position t + j - pad is outside [0, T)
//
// The GEMM is conv_sp_f32.hip's, the one conv_tile_product of conv_frag.h (32-deep chunks of one tap of one source, fp32 LDS images,
// split product or fp32 MFMA under lime_set_split_gemm(0); 256 threads, 128 x 128 tile, two stages, one barrier per chunk), given the
// three-way source select as its tap and the end of the tile's live rows.  A tile holds floor(128 / T) WHOLE
// sequences (T <= 128), so the maximum over a sequence never crosses workgroups: no atomics, and the pre-activations go from the
// accumulators to the LDS the operand stages have left (132-float rows) and from there to one thread per (sequence, column), which
// walks t = 0 .. P - 1 in order.  They never reach memory.  The chunk order of an output element is fixed, so its bits do not depend
// on the tile slot its sequence occupies or on the batch around it.
//
// The two row kernels are the unfused partner (dense pre-activations from lime_conv1d_window_f32 -> pooled / arg) and the backward of
// the pooling (dpre = dpooled at row s T + arg, zeros elsewhere, every element written once by the thread that owns its
// (sequence, four columns) strip).
#include "conv_frag.h"

using namespace lime_dev;

int lime_split_mode();

namespace {

constexpr int BM = CONV_BM, BN = CONV_BN;
constexpr int EP_PITCH = BN + 4;        // the epilogue's [BM][BN] pre-activation image
static_assert(BM * EP_PITCH <= 2 * CONV_STAGE, "the epilogue image fits the operand stages");

struct PoolParams {
    const float* a0; const float* a1; const float* a2;
    long lda0, lda1, lda2;
    const int* ids0; const int* ids1; const int* ids2;
    const float* w;
    long ldw;
    const float* bias;
    float* pooled;
    long ldp;
    int* arg;
    long ldarg;
    const int* n_seq_dev;
    int n_seq, T, N, C, n_src, win, pad, P, seq_per_tile, n_col_blocks;
};

template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void conv_pool_sp_kernel(const PoolParams p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * CONV_STAGE];
    const int n_seq = live_count(p.n_seq_dev, p.n_seq);
    const int rb = blockIdx.x / p.n_col_blocks, cb = blockIdx.x - rb * p.n_col_blocks;
    const int seq0 = rb * p.seq_per_tile, col0 = cb * BN;
    if (seq0 >= n_seq) return;
    const int n_here = n_seq - seq0 < p.seq_per_tile ? n_seq - seq0 : p.seq_per_tile;      // sequences of this tile
    const int rows = n_here * p.T, row0 = seq0 * p.T;                                      // its live rows: row0 .. row0 + rows - 1
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave & 1, wc = wave >> 1;
    const int fi = lane & 15, kg = lane >> 4;

    f32x4 acc[4][4];
    auto tap = [&p](int sj) {                          // sj = src win + j: the weight's tap block
        const int src = sj / p.win;
        return ConvTap{src == 0 ? p.a0 : src == 1 ? p.a1 : p.a2, src == 0 ? p.lda0 : src == 1 ? p.lda1 : p.lda2,
                       src == 0 ? p.ids0 : src == 1 ? p.ids1 : p.ids2, sj - src * p.win};
    };
    conv_tile_product<SPLIT>(lds, acc, tap, p.n_src * p.win, p.w, p.ldw, p.C, p.N, p.T, p.pad, row0, row0 + rows, col0);

    // epilogue 1: the pre-activations of the tile into LDS (every reader of the stages is past the loop's last barrier); lane (fi, kg)
    // holds row 64 wr + 16 i + fi, columns 64 wc + 16 t + 4 kg + e in acc[i][t][e]
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int nl = 64 * wc + 16 * t + 4 * kg, n = col0 + nl;
        f32x4 b = {0.f, 0.f, 0.f, 0.f};
        if (p.bias && n < p.N) b = ld4(p.bias + n);    // N % 4 == 0: a segment is valid as a whole
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(lds + (64 * wr + 16 * i + fi) * EP_PITCH + nl) = acc[i][t] + b;
    }
    lds_barrier();
    // epilogue 2: one thread per (sequence, column), positions in order: the first t that attains the maximum wins
    for (int it = tid; it < n_here * BN; it += 256) {
        const int s = it / BN, nl = it - s * BN, n = col0 + nl;
        if (n >= p.N) continue;
        const float* const col = lds + (s * p.T) * EP_PITCH + nl;
        float best = 0.f;
        int at = -1;
        for (int t = 0; t < p.P; ++t) {
            const float v = col[t * EP_PITCH];
            if (v > best) { best = v; at = t; }
        }
        p.pooled[(long)(seq0 + s) * p.ldp + n] = best;
        if (p.arg) p.arg[(long)(seq0 + s) * p.ldarg + n] = at;
    }
}

// pooled / arg from dense pre-activations: one thread per (sequence, four columns)
__global__ __launch_bounds__(256) void relu_maxpool_kernel(const float* __restrict__ pre, long ldpre, const float* __restrict__ bias,
                                                           float* __restrict__ pooled, long ldp, int* __restrict__ arg, long ldarg,
                                                           int n_seq, int T, int P, int N, const int* __restrict__ n_seq_dev) {
    n_seq = live_count(n_seq_dev, n_seq);
    const int n4 = N >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n_seq * n4) return;
    const int s = (int)(i / n4), n = 4 * (int)(i - (long)s * n4);
    const f32x4 b = bias ? ld4(bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 best = {0.f, 0.f, 0.f, 0.f};
    int at[4] = {-1, -1, -1, -1};
    const float* q = pre + (long)s * T * ldpre + n;
    for (int t = 0; t < P; ++t, q += ldpre) {
        const f32x4 v = ld4(q) + b;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v[e] > best[e]) { best[e] = v[e]; at[e] = t; }
    }
    *reinterpret_cast<f32x4*>(pooled + (long)s * ldp + n) = best;
    if (arg) {
        int* const d = arg + (long)s * ldarg + n;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = at[e];
    }
}

// dpre[s T + t, n] = arg[s, n] == t ? dpooled[s, n] : 0, every row of the strip written by its owner
__global__ __launch_bounds__(256) void relu_maxpool_bwd_kernel(const float* __restrict__ dpooled, long lddp, const int* __restrict__ arg,
                                                               long ldarg, float* __restrict__ dpre, long ldpre, int n_seq, int T, int N) {
    const int n4 = N >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n_seq * n4) return;
    const int s = (int)(i / n4), n = 4 * (int)(i - (long)s * n4);
    const f32x4 g = ld4(dpooled + (long)s * lddp + n);
    int at[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) at[e] = arg[(long)s * ldarg + n + e];
    float* q = dpre + (long)s * T * ldpre + n;
    for (int t = 0; t < T; ++t, q += ldpre) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = at[e] == t ? g[e] : 0.f;
        *reinterpret_cast<f32x4*>(q) = v;
    }
}

}  // namespace

extern "C" int lime_conv_pool_f32(const lime_conv_pool_args* args, void* stream) {
    LIME_REQUIRE(args, LIME_ERR_BAD_ARG, "lime_conv_pool_f32: NULL args");
    const lime_conv_pool_args& a = *args;
    LIME_REQUIRE(a.w && a.pooled, LIME_ERR_BAD_ARG, "lime_conv_pool_f32: null pointer");
    LIME_REQUIRE(a.n_src >= 1 && a.n_src <= 3, LIME_ERR_BAD_ARG, "lime_conv_pool_f32: n_src = %d (1 .. 3 sources)", a.n_src);
    LIME_REQUIRE(a.n_seq > 0 && a.T > 0 && a.N > 0 && a.C > 0, LIME_ERR_BAD_ARG, "lime_conv_pool_f32: non-positive dimension");
    LIME_REQUIRE(a.T <= BM, LIME_ERR_UNSUPPORTED, "lime_conv_pool_f32: T = %d: a tile holds whole sequences of at most %d tokens", a.T, BM);
    LIME_REQUIRE(a.window >= 1 && a.window <= a.T && a.P >= 1 && a.P <= a.T, LIME_ERR_BAD_ARG,
                 "lime_conv_pool_f32: window %d / pooled positions %d outside 1 .. T = %d", a.window, a.P, a.T);
    LIME_REQUIRE(a.pad >= 0 && a.pad < a.window, LIME_ERR_BAD_ARG, "lime_conv_pool_f32: pad %d outside 0 .. window - 1", a.pad);
    LIME_REQUIRE(a.C % 4 == 0 && a.N % 4 == 0, LIME_ERR_UNSUPPORTED, "lime_conv_pool_f32: C = %d and N = %d must be multiples of 4", a.C, a.N);
    LIME_REQUIRE(a.ldw >= (int64_t)a.n_src * a.window * a.C && a.ldp >= a.N && (!a.arg || a.ldarg >= a.N), LIME_ERR_BAD_ARG,
                 "lime_conv_pool_f32: leading dimension smaller than the row");
    LIME_REQUIRE(lime_al16(a.w, a.ldw) && lime_al16(a.bias, 0), LIME_ERR_UNSUPPORTED,
                 "lime_conv_pool_f32: w (ldw a multiple of 4) and bias must be 16-byte aligned");
    LIME_REQUIRE((long)a.n_seq * a.T < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_conv_pool_f32: too many tokens");
    for (int s = 0; s < a.n_src; ++s) {
        LIME_REQUIRE(a.a[s], LIME_ERR_BAD_ARG, "lime_conv_pool_f32: source %d is NULL", s);
        LIME_REQUIRE(a.lda[s] >= a.C, LIME_ERR_BAD_ARG, "lime_conv_pool_f32: source %d: leading dimension smaller than the row", s);
        LIME_REQUIRE(lime_al16(a.a[s], a.lda[s]), LIME_ERR_UNSUPPORTED,
                     "lime_conv_pool_f32: source %d must be 16-byte aligned with a leading dimension that is a multiple of 4", s);
    }
    PoolParams p;
    p.a0 = a.a[0]; p.a1 = a.n_src > 1 ? a.a[1] : nullptr; p.a2 = a.n_src > 2 ? a.a[2] : nullptr;
    p.lda0 = a.lda[0]; p.lda1 = a.n_src > 1 ? a.lda[1] : 0; p.lda2 = a.n_src > 2 ? a.lda[2] : 0;
    p.ids0 = a.ids[0]; p.ids1 = a.n_src > 1 ? a.ids[1] : nullptr; p.ids2 = a.n_src > 2 ? a.ids[2] : nullptr;
    p.w = a.w; p.ldw = a.ldw; p.bias = a.bias; p.pooled = a.pooled; p.ldp = a.ldp; p.arg = a.arg; p.ldarg = a.ldarg;
    p.n_seq_dev = a.n_seq_dev;
    p.n_seq = a.n_seq; p.T = a.T; p.N = a.N; p.C = a.C; p.n_src = a.n_src; p.win = a.window; p.pad = a.pad; p.P = a.P;
    p.seq_per_tile = BM / a.T;
    p.n_col_blocks = (a.N + BN - 1) / BN;
    const long grid = (long)((a.n_seq + p.seq_per_tile - 1) / p.seq_per_tile) * p.n_col_blocks;
    LIME_REQUIRE(grid < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_conv_pool_f32: grid too large");
    hipStream_t s = (hipStream_t)stream;
    if (lime_split_mode() & 1) conv_pool_sp_kernel<true><<<(unsigned)grid, 256, 0, s>>>(p);
    else conv_pool_sp_kernel<false><<<(unsigned)grid, 256, 0, s>>>(p);
    return lime_check_launch("lime_conv_pool_f32");
}

extern "C" int lime_relu_maxpool_f32(const float* pre, int64_t ldpre, const float* bias, float* pooled, int64_t ldp, int32_t* arg,
                                     int64_t ldarg, int32_t n_seq, int32_t T, int32_t P, int32_t N, const int32_t* n_seq_dev, void* stream) {
    LIME_REQUIRE(pre && pooled, LIME_ERR_BAD_ARG, "lime_relu_maxpool_f32: null pointer");
    LIME_REQUIRE(n_seq > 0 && T > 0 && N > 0, LIME_ERR_BAD_ARG, "lime_relu_maxpool_f32: non-positive dimension");
    LIME_REQUIRE(P >= 1 && P <= T, LIME_ERR_BAD_ARG, "lime_relu_maxpool_f32: pooled positions %d outside 1 .. T = %d", P, T);
    LIME_REQUIRE(ldpre >= N && ldp >= N && (!arg || ldarg >= N), LIME_ERR_BAD_ARG, "lime_relu_maxpool_f32: leading dimension smaller than the row");
    LIME_REQUIRE(N % 4 == 0 && lime_al16(pre, ldpre) && lime_al16(pooled, ldp) && lime_al16(bias, 0), LIME_ERR_UNSUPPORTED,
                 "lime_relu_maxpool_f32: N, ldpre, ldp must be multiples of 4 and pre, pooled, bias 16-byte aligned");
    const long total = (long)n_seq * (N / 4);
    LIME_REQUIRE((total + 255) / 256 < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_relu_maxpool_f32: grid too large");
    relu_maxpool_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(pre, ldpre, bias, pooled, ldp, arg, ldarg, n_seq, T,
                                                                                         P, N, n_seq_dev);
    return lime_check_launch("lime_relu_maxpool_f32");
}

extern "C" int lime_relu_maxpool_bwd_f32(const float* dpooled, int64_t lddp, const int32_t* arg, int64_t ldarg, float* dpre, int64_t ldpre,
                                         int32_t n_seq, int32_t T, int32_t N, void* stream) {
    LIME_REQUIRE(dpooled && arg && dpre, LIME_ERR_BAD_ARG, "lime_relu_maxpool_bwd_f32: null pointer");
    LIME_REQUIRE(n_seq > 0 && T > 0 && N > 0, LIME_ERR_BAD_ARG, "lime_relu_maxpool_bwd_f32: non-positive dimension");
    LIME_REQUIRE(lddp >= N && ldarg >= N && ldpre >= N, LIME_ERR_BAD_ARG, "lime_relu_maxpool_bwd_f32: leading dimension smaller than the row");
    LIME_REQUIRE(N % 4 == 0 && lime_al16(dpooled, lddp) && lime_al16(dpre, ldpre), LIME_ERR_UNSUPPORTED,
                 "lime_relu_maxpool_bwd_f32: N, lddp, ldpre must be multiples of 4 and dpooled, dpre 16-byte aligned");
    const long total = (long)n_seq * (N / 4);
    LIME_REQUIRE((total + 255) / 256 < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_relu_maxpool_bwd_f32: grid too large");
    relu_maxpool_bwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(dpooled, lddp, arg, ldarg, dpre, ldpre, n_seq, T, N);
    return lime_check_launch("lime_relu_maxpool_bwd_f32");
}
