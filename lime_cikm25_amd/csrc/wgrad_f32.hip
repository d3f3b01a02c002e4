// lime_linear_wgrad_f32 / lime_colsum_f32: the fp32 weight gradient of a linear layer (reference
// trainer.py:131-148 drives loss.backward() through the encoder layers of newsEncoders.py:244-247,311-321).
//
//   wgrad_kernel / wgrad_dma_kernel   dW[n, k] = sum_m dY[m, n] X[m, k]   split over M, exact-fp32 MFMA, partial tiles in the workspace
//   colsum_kernel                     db[n] = sum_m dY[m, n]              (when K fills its tiles: otherwise a ones column of X)
//   reduce_partials(_vec4)_kernel     the partials summed in a fixed order; lime_reduce_partials() serves the other units too
//
// Big problems go to the split-product kernel of wgrad_sp_f32.hip; the choice is made here.
#include "dev_helpers.h"
#include "gemm_pp.h"

using namespace lime_dev;

namespace {

// ---------------------------------------------------------------------------------------------------
// reduce_partials: out[r, c] (+)= sum_s ws[s * split_stride + r * ldw + c].  A workgroup owns 64 consecutive outputs; its
// four waves take the splits s = wave, wave + 4, ... and the four sums are added in a fixed order.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ ws, long split_stride, int splits,
                                                               long ldw, float* __restrict__ out, long ldo, int rows, int cols,
                                                               int accumulate) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long e = (long)blockIdx.x * 64 + lane;
    const bool ok = e < (long)rows * cols;
    const int r = ok ? (int)(e / cols) : 0, c = ok ? (int)(e - (long)r * cols) : 0;
    float s = 0.f;
    if (ok) {
        const float* p = ws + (long)r * ldw + c;
        for (int i = g; i < splits; i += 4) s += p[(long)i * split_stride];
    }
    red[g][lane] = s;
    __syncthreads();
    if (g == 0 && ok) {
        const float t = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        float* o = out + (long)r * ldo + c;
        *o = accumulate ? *o + t : t;
    }
}

// The same with four consecutive outputs per lane (16-byte accesses; cols % 4 == 0 so a group never leaves its row) and four
// splits of a wave in flight: the scalar version reads 256 B per wave and load, 0.7 TB/s on the 39 MB of in_proj's 32 partial
// tiles.  Same association as above (a wave sums its splits in order, the four waves' sums are added pairwise): same bits.
// `extra` (optional): column `cols` of the partial grid also holds a sum -- the ones column's bias gradient -- and goes to extra[r] in the
// same launch (a second launch per weight gradient for N floats was 19 launches of 6 us per training step).
__global__ __launch_bounds__(256) void reduce_partials_vec4_kernel(const float* __restrict__ ws, long split_stride, int splits,
                                                                    long ldw, float* __restrict__ out, long ldo, int rows, int cols,
                                                                    int accumulate, float* __restrict__ extra) {
    __shared__ f32x4 red4[4][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int c4 = (cols >> 2) + (extra != nullptr ? 1 : 0);
    const long e = (long)blockIdx.x * 64 + lane;                 // group of four columns
    const bool ok = e < (long)rows * c4;
    const int r = ok ? (int)(e / c4) : 0, c = ok ? (int)(e - (long)r * c4) * 4 : 0;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
        const float* p = ws + (long)r * ldw + c;
        int i = g;
        for (; i + 12 < splits; i += 16) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(p + (long)(i + 4 * u) * split_stride);
#pragma unroll
            for (int u = 0; u < 4; ++u) s += v[u];
        }
        for (; i < splits; i += 4) s += *reinterpret_cast<const f32x4*>(p + (long)i * split_stride);
    }
    red4[g][lane] = s;
    __syncthreads();
    if (g == 0 && ok) {
        const f32x4 t = (red4[0][lane] + red4[1][lane]) + (red4[2][lane] + red4[3][lane]);
        if (c == cols) {                                   // the extra column (only with `extra`)
            extra[r] = accumulate ? extra[r] + t[0] : t[0];
        } else {
            f32x4* o = reinterpret_cast<f32x4*>(out + (long)r * ldo + c);
            *o = accumulate ? *o + t : t;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// wgrad: workgroup = one 128 x TK tile of dW (TK = 64 NKT: the whole K of the encoder layers' 300-wide operands) over one
// slice of the M rows.  Eight waves in a 2 x 4 grid, each a 64 x 16 NKT patch (4 x NKT accumulator tiles of 16 x 16), two
// waves per SIMD so one wave's LDS waits sit under the other's MFMAs.  64-row chunks of dY and X go global -> registers
// -> LDS (one stage): the loads of chunk i + 1 are issued right after chunk i has been written to LDS and are in flight
// for the whole of its MFMA phase (56 KB per workgroup -- one 32-row chunk in flight left the kernel latency-bound).
// ---------------------------------------------------------------------------------------------------
constexpr int WG_TN = 128;
constexpr int WG_MC = 64;
constexpr int WG_THREADS = 512;

template <int NKT, bool VEC>       // NKT: 16-column accumulator tiles per wave along K (TK = 64 NKT); VEC: 16-byte loads
__global__ __launch_bounds__(WG_THREADS) void wgrad_kernel(const float* __restrict__ dy, long ldy, const float* __restrict__ x,
                                                            long ldx, float* __restrict__ ws, int M, int N, int K, int n_tiles,
                                                            int k_tiles, int rows_per_split, int ones_col) {
    constexpr int TK = 64 * NKT;
    constexpr int LDA = WG_TN + 16;          // pitch % 32 == 16: the two row groups of a half-wave hit disjoint banks
    constexpr int LDB = TK + 16;
    constexpr int A4 = WG_MC * WG_TN / 4 / WG_THREADS;                    // float4 per thread per chunk (dY tile): 2
    constexpr int B4 = (WG_MC * TK / 4 + WG_THREADS - 1) / WG_THREADS;    // (X tile): 3, 4 or 5
    extern __shared__ float wg_smem[];
    float* const As = wg_smem;                                            // [WG_MC * LDA]
    float* const Bs = wg_smem + WG_MC * LDA;                              // [WG_MC * LDB]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, kg = lane >> 4;
    const int ntile = n_tiles * k_tiles;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int split = logical / ntile, tile = logical - split * ntile;
    const int n0 = (tile / k_tiles) * WG_TN, k0 = (tile % k_tiles) * TK;
    const long m_begin = (long)split * rows_per_split;
    const long m_end = min((long)M, m_begin + rows_per_split);
    const int wn = (wave >> 2) * 64, wk = (wave & 3) * (16 * NKT);

    f32x4 acc[4][NKT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NKT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Loads are branch-free buffer loads: rows beyond the slice and columns beyond N / K carry the OOB offset and read zeros.
    // Offsets are relative to the first row of the slice (the host checks that a slice spans < 2 GB).
    f32x4 ra[A4], rb[B4];
    const __amdgpu_buffer_rsrc_t rs_a = make_rsrc(dy + m_begin * ldy + n0);
    const __amdgpu_buffer_rsrc_t rs_b = make_rsrc(x + m_begin * ldx + k0);
    const int rows_here = (int)(m_end - m_begin);
    unsigned a_off[A4], b_off[B4];
    int a_row[A4], b_row[B4];
    bool a_cin[A4][VEC ? 1 : 4], b_cin[B4][VEC ? 1 : 4];
    int b_one[B4];                                          // which element of this lane's X float4 is the ones column (-1: none)
#pragma unroll
    for (int j = 0; j < A4; ++j) {
        const int f = tid + WG_THREADS * j, r = f / (WG_TN / 4), c = (f % (WG_TN / 4)) * 4;
        a_row[j] = r;
        a_off[j] = (unsigned)r * (unsigned)(ldy * 4) + (unsigned)c * 4u;
        if constexpr (VEC) a_cin[j][0] = n0 + c < N;
        else
#pragma unroll
            for (int e = 0; e < 4; ++e) a_cin[j][e] = n0 + c + e < N;
    }
#pragma unroll
    for (int j = 0; j < B4; ++j) {
        const int f = tid + WG_THREADS * j, r = f / (TK / 4), c = (f % (TK / 4)) * 4;
        const bool in_tile = f < WG_MC * TK / 4;
        b_row[j] = in_tile ? r : (1 << 30);
        b_off[j] = (unsigned)r * (unsigned)(ldx * 4) + (unsigned)c * 4u;
        b_one[j] = (ones_col && K >= k0 + c && K < k0 + c + 4) ? K - (k0 + c) : -1;
        if constexpr (VEC) b_cin[j][0] = k0 + c < K;
        else
#pragma unroll
            for (int e = 0; e < 4; ++e) b_cin[j][e] = k0 + c + e < K;
    }
    auto load_chunk = [&](int mrel) {                       // mrel: first row of the chunk relative to the slice
        const int soff_a = mrel * (int)(ldy * 4), soff_b = mrel * (int)(ldx * 4);
#pragma unroll
        for (int j = 0; j < A4; ++j) {
            const bool rin = mrel + a_row[j] < rows_here;
            if constexpr (VEC) ra[j] = buf_load4(rs_a, rin && a_cin[j][0] ? a_off[j] : OOB, soff_a);
            else
#pragma unroll
                for (int e = 0; e < 4; ++e) ra[j][e] = buf_load1(rs_a, rin && a_cin[j][e] ? a_off[j] + 4u * e : OOB, soff_a);
        }
#pragma unroll
        for (int j = 0; j < B4; ++j) {
            const bool rin = mrel + b_row[j] < rows_here;
            if constexpr (VEC) rb[j] = buf_load4(rs_b, rin && b_cin[j][0] ? b_off[j] : OOB, soff_b);
            else
#pragma unroll
                for (int e = 0; e < 4; ++e) rb[j][e] = buf_load1(rs_b, rin && b_cin[j][e] ? b_off[j] + 4u * e : OOB, soff_b);
            // column K of X reads as 1 on the valid rows: column K of dW then holds sum_m dY[m, n], the bias gradient
            if (b_one[j] >= 0 && rin) rb[j][b_one[j]] = 1.0f;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int j = 0; j < A4; ++j) {
            const int f = tid + WG_THREADS * j, r = f / (WG_TN / 4), c = (f % (WG_TN / 4)) * 4;
            *reinterpret_cast<f32x4*>(&As[r * LDA + c]) = ra[j];
        }
#pragma unroll
        for (int j = 0; j < B4; ++j) {
            const int f = tid + WG_THREADS * j, r = f / (TK / 4), c = (f % (TK / 4)) * 4;
            if (f < WG_MC * TK / 4) *reinterpret_cast<f32x4*>(&Bs[r * LDB + c]) = rb[j];
        }
    };

    if (rows_here > 0) {
        load_chunk(0);
        const float* as = &As[kg * LDA + wn + fi];
        const float* bs = &Bs[kg * LDB + wk + fi];
        for (int m0 = 0; m0 < rows_here; m0 += WG_MC) {
            __syncthreads();                               // every wave is done reading the previous chunk
            store_chunk();
            __syncthreads();
            if (m0 + WG_MC < rows_here) load_chunk(m0 + WG_MC);
#pragma unroll
            for (int s = 0; s < WG_MC / 4; ++s) {
                float a[4], b[NKT];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = as[4 * s * LDA + 16 * i];
#pragma unroll
                for (int j = 0; j < NKT; ++j) b[j] = bs[4 * s * LDB + 16 * j];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NKT; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
            }
        }
    }
    // partial tile -> ws[split][n][k] over the padded [n_tiles * 128, k_tiles * TK] grid
    const long ldw = (long)k_tiles * TK;
    float* o = ws + (long)split * ((long)n_tiles * WG_TN) * ldw;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                o[(long)(n0 + wn + 16 * i + 4 * kg + r) * ldw + k0 + wk + 16 * j + fi] = acc[i][j][r];
}

// ---------------------------------------------------------------------------------------------------
// wgrad with LDS-DMA staging (16-byte aligned operands): the same tiling as wgrad_kernel, but 32-row chunks go global -> LDS
// directly (raw_ptr_buffer_load_lds, 1 KB per wave instruction, rows packed without padding), two stages, ONE barrier per
// chunk: chunk c + 1 is in flight while chunk c is multiplied; no staging registers, no LDS stores.
// ---------------------------------------------------------------------------------------------------
constexpr int WD_MC = 32;          // rows per chunk: two stages of 32 rows = 112 KB at TK = 320 (16-row chunks with two workgroups
                                   // per CU measured the same kernel time and double the partial tiles to sum)

template <int NKT>
__global__ __launch_bounds__(WG_THREADS) void wgrad_dma_kernel(const float* __restrict__ dy, long ldy, const float* __restrict__ x,
                                                                long ldx, float* __restrict__ ws, int M, int N, int K, int n_tiles,
                                                                int k_tiles, int rows_per_split, int ones_col) {
    constexpr int TK = 64 * NKT;
    constexpr int A_FLOATS = WD_MC * WG_TN, B_FLOATS = WD_MC * TK, STAGE = A_FLOATS + B_FLOATS;
    constexpr int A_P = A_FLOATS / 256, B_P = B_FLOATS / 256;     // 1 KB DMA pieces per chunk: 8 and 12 / 16 / 20
    constexpr int A_PW = (A_P + 7) / 8, B_PW = (B_P + 7) / 8;     // per wave (piece q = wave + 8 j, q < P)
    extern __shared__ float wg_smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, kg = lane >> 4;
    const int ntile = n_tiles * k_tiles;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int split = logical / ntile, tile = logical - split * ntile;
    const int n0 = (tile / k_tiles) * WG_TN, k0 = (tile % k_tiles) * TK;
    const long m_begin = (long)split * rows_per_split;
    const int rows_here = (int)(min((long)M, m_begin + rows_per_split) - m_begin);
    const int wn = (wave >> 2) * 64, wk = (wave & 3) * (16 * NKT);

    f32x4 acc[4][NKT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NKT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (rows_here > 0) {
        const __amdgpu_buffer_rsrc_t rs_a = make_rsrc(dy + m_begin * ldy + n0);
        const __amdgpu_buffer_rsrc_t rs_b = make_rsrc(x + m_begin * ldx + k0);
        // this lane's 16-byte pieces: piece q of the wave covers floats [256 q + 4 lane, + 4) of the packed [32][cols] image
        unsigned a_off[A_PW], b_off[B_PW];
        int a_row[A_PW], b_row[B_PW], b_one[B_PW], b_r[B_PW];
#pragma unroll
        for (int j = 0; j < A_PW; ++j) {
            const int q = wave + 8 * j, f = q * 256 + 4 * lane, r = f / WG_TN, c = f % WG_TN;
            a_row[j] = (q < A_P && n0 + c < N) ? r : (1 << 30);
            a_off[j] = (unsigned)r * (unsigned)(ldy * 4) + (unsigned)c * 4u;
        }
#pragma unroll
        for (int j = 0; j < B_PW; ++j) {
            const int q = wave + 8 * j, f = q * 256 + 4 * lane, r = f / TK, c = f % TK;
            b_row[j] = (q < B_P && k0 + c < K) ? r : (1 << 30);
            b_off[j] = (unsigned)r * (unsigned)(ldx * 4) + (unsigned)c * 4u;
            b_r[j] = r;
            // the all-ones column of X (bias gradient) falls into this lane's piece: the lane patches it after its DMA landed
            b_one[j] = (q < B_P && ones_col && K >= k0 + c && K < k0 + c + 4) ? K - k0 - c : -1;
        }
        auto issue = [&](int stage, int mrel) {
            float* const sb = wg_smem + stage * STAGE;
            const int soff_a = mrel * (int)(ldy * 4), soff_b = mrel * (int)(ldx * 4);
#pragma unroll
            for (int j = 0; j < A_PW; ++j)
                if (wave + 8 * j < A_P)
                    dma16(rs_a, sb + (wave + 8 * j) * 256, (mrel + a_row[j] < rows_here) ? a_off[j] : OOB, soff_a);
#pragma unroll
            for (int j = 0; j < B_PW; ++j)
                if (wave + 8 * j < B_P)
                    dma16(rs_b, sb + A_FLOATS + (wave + 8 * j) * 256, (mrel + b_row[j] < rows_here) ? b_off[j] : OOB, soff_b);
        };
        issue(0, 0);
        int stage = 0;
        for (int m0 = 0; m0 < rows_here; m0 += WD_MC) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of chunk m0 have landed
#pragma unroll
            for (int j = 0; j < B_PW; ++j)
                if (b_one[j] >= 0)
                    wg_smem[stage * STAGE + A_FLOATS + (wave + 8 * j) * 256 + 4 * lane + b_one[j]] = (m0 + b_r[j] < rows_here) ? 1.0f : 0.f;
            __syncthreads();                                           // everybody's have; the other stage is no longer read
            if (m0 + WD_MC < rows_here) issue(stage ^ 1, m0 + WD_MC);
            const float* as = wg_smem + stage * STAGE + kg * WG_TN + wn + fi;
            const float* bs = wg_smem + stage * STAGE + A_FLOATS + kg * TK + wk + fi;
#pragma unroll
            for (int s = 0; s < WD_MC / 4; ++s) {
                float a[4], b[NKT];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = as[4 * s * WG_TN + 16 * i];
#pragma unroll
                for (int j = 0; j < NKT; ++j) b[j] = bs[4 * s * TK + 16 * j];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NKT; ++j) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
            }
            stage ^= 1;
        }
    }
    const long ldw = (long)k_tiles * TK;
    float* o = ws + (long)split * ((long)n_tiles * WG_TN) * ldw;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NKT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                o[(long)(n0 + wn + 16 * i + 4 * kg + r) * ldw + k0 + wk + 16 * j + fi] = acc[i][j][r];
}

// ---------------------------------------------------------------------------------------------------
// colsum: partial[blk][c] = sum of x[r, c] over the block's rows
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, long ldx, int M, int N, int rows_per_block,
                                                      float* __restrict__ ws) {
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const long r0 = (long)blockIdx.y * rows_per_block;
    const long r1 = min((long)M, r0 + rows_per_block);
    float s = 0.f;
    if (c < N)
        for (long r = r0 + g; r < r1; r += 4) s += x[r * ldx + c];
    red[g][threadIdx.x & 63] = s;
    __syncthreads();
    if (g == 0 && c < N) ws[(long)blockIdx.y * N + c] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

struct WgradPlan { int nkt, tk, n_tiles, k_tiles, splits, rows_per_split; long np, kp; };

WgradPlan wgrad_plan(int M, int N, int K, int wg_per_cu = 1) {
    WgradPlan w;
    long best = -1;
    w.nkt = 4;
    for (int nkt = 3; nkt <= 5; ++nkt) {                          // the tile width 64 * nkt that pads K the least
        const long tk = 64L * nkt, kp = ((long)K + tk - 1) / tk * tk;
        if (best < 0 || kp < best || (kp == best && nkt == 4)) { best = kp; w.nkt = nkt; }
    }
    w.tk = 64 * w.nkt;
    w.n_tiles = (N + WG_TN - 1) / WG_TN;
    w.k_tiles = (K + w.tk - 1) / w.tk;
    w.np = (long)w.n_tiles * WG_TN;
    w.kp = (long)w.k_tiles * w.tk;
    const int ntile = w.n_tiles * w.k_tiles;
    int splits = 256 * wg_per_cu / ntile;                         // a single round of eight-wave workgroups, one per CU
    // at least 8 chunks of 64 rows per workgroup -- but the small-M problems of the layers around the encoders (B x 55 = 1760 rows: 36
    // workgroups of 9 serial chunks took 50 us) go down to 2 chunks so that a launch reaches ~150 workgroups
    const int max_splits = M >= 8192 ? (M + 511) / 512 : (M + 127) / 128;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
    int rps = (M + splits - 1) / splits;
    rps = (rps + WG_MC - 1) / WG_MC * WG_MC;
    w.rows_per_split = rps;
    w.splits = (M + rps - 1) / rps;
    if (w.splits < 1) w.splits = 1;
    return w;
}

template <int NKT>
int launch_wgrad_dma(const WgradPlan& w, const float* dy, long ldy, const float* x, long ldx, float* ws, int M, int N, int K,
                     int ones_col, hipStream_t s) {
    constexpr int BYTES = 2 * WD_MC * (WG_TN + 64 * NKT) * 4;
    static int reserved = 0;
    if (const int st = lime_reserve_lds((const void*)wgrad_dma_kernel<NKT>, BYTES, reserved, "lime_linear_wgrad_f32")) return st;
    const int grid = w.n_tiles * w.k_tiles * w.splits;
    wgrad_dma_kernel<NKT><<<grid, WG_THREADS, BYTES, s>>>(dy, ldy, x, ldx, ws, M, N, K, w.n_tiles, w.k_tiles, w.rows_per_split, ones_col);
    return lime_check_launch("wgrad_dma_kernel");
}

template <int NKT, bool VEC>
int launch_wgrad(const WgradPlan& w, const float* dy, long ldy, const float* x, long ldx, float* ws, int M, int N, int K,
                 int ones_col, hipStream_t s) {
    constexpr int BYTES = WG_MC * ((WG_TN + 16) + (64 * NKT + 16)) * 4;
    static int reserved = 0;
    if (const int st = lime_reserve_lds((const void*)wgrad_kernel<NKT, VEC>, BYTES, reserved, "lime_linear_wgrad_f32")) return st;
    const int grid = w.n_tiles * w.k_tiles * w.splits;
    wgrad_kernel<NKT, VEC><<<grid, WG_THREADS, BYTES, s>>>(dy, ldy, x, ldx, ws, M, N, K, w.n_tiles, w.k_tiles, w.rows_per_split, ones_col);
    return lime_check_launch("wgrad_kernel");
}

int colsum_blocks(int M) {
    int b = (M + 255) / 256;
    return b < 1 ? 1 : (b > 256 ? 256 : b);
}

}  // namespace

// out[r, c] (+)= the sum over the splits of a partial grid (gemm_pp.h: the layernorm backward and the split-product weight gradient
// sum theirs here too).  extra (optional): column `cols` of the partial grid summed into extra[rows] as well (the caller guarantees the
// grid has that column)
int lime_reduce_partials(const float* ws, long split_stride, int splits, long ldw, float* out, long ldo, int rows, int cols,
                         int accumulate, hipStream_t s, float* extra) {
    const long total = (long)rows * cols;
    if (cols % 4 == 0 && split_stride % 4 == 0 && lime_al16(ws, ldw) && lime_al16(out, ldo)) {
        const long groups = (long)rows * (cols / 4 + (extra ? 1 : 0));
        const int grid4 = (int)((groups + 63) / 64);
        reduce_partials_vec4_kernel<<<grid4, 256, 0, s>>>(ws, split_stride, splits, ldw, out, ldo, rows, cols, accumulate, extra);
        return lime_check_launch("reduce_partials");
    }
    if (extra) {                                            // scalar layout: the extra column as a launch of its own
        const int st = lime_reduce_partials(ws, split_stride, splits, ldw, out, ldo, rows, cols, accumulate, s);
        return st != LIME_OK ? st : lime_reduce_partials(ws + cols, split_stride, splits, ldw, extra, 1, rows, 1, accumulate, s);
    }
    const int grid = (int)((total + 63) / 64);
    reduce_partials_kernel<<<grid, 256, 0, s>>>(ws, split_stride, splits, ldw, out, ldo, rows, cols, accumulate);
    return lime_check_launch("reduce_partials");
}

extern "C" int64_t lime_colsum_workspace(int32_t M, int32_t N) {
    return M > 0 && N > 0 ? (int64_t)colsum_blocks(M) * N : 0;
}

extern "C" int lime_colsum_f32(const float* x, int64_t ldx, int32_t M, int32_t N, float* out, int32_t accumulate,
                               float* workspace, int64_t workspace_floats, void* stream) {
    LIME_REQUIRE(x && out && workspace, LIME_ERR_BAD_ARG, "lime_colsum_f32: null pointer");
    LIME_REQUIRE(M > 0 && N > 0 && ldx >= N, LIME_ERR_BAD_ARG, "lime_colsum_f32: bad dimensions");
    const int nblk = colsum_blocks(M);
    LIME_REQUIRE(workspace_floats >= (int64_t)nblk * N, LIME_ERR_BAD_ARG, "lime_colsum_f32: workspace too small (%ld < %ld)",
                 (long)workspace_floats, (long)nblk * N);
    hipStream_t s = (hipStream_t)stream;
    const int rpb = (M + nblk - 1) / nblk;
    colsum_kernel<<<dim3((N + 63) / 64, nblk), 256, 0, s>>>(x, ldx, M, N, rpb, workspace);
    const int st = lime_check_launch("colsum_kernel");
    if (st != LIME_OK) return st;
    return lime_reduce_partials(workspace, N, nblk, N, out, N, 1, N, accumulate, s);
}

// The split-product kernel (wgrad_sp_f32.hip) takes the problems that fill its 256 x 320 tiles: from 4096 rows on (below, the
// workgroups' slices are a handful of chunks), 16-byte friendly operands, at least half of the padded tile grid real.
static bool wgrad_sp_shape(int M, int N, int K) { return M >= 4096 && N % 4 == 0 && K % 4 == 0 && N >= 64 && K >= 64 && lime_wgrad_sp_plan(M, N, K).fill >= 0.5; }

extern "C" int64_t lime_linear_wgrad_workspace(int32_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const WgradPlan w = wgrad_plan(M, N, K);
    int64_t need = (int64_t)w.splits * w.np * w.kp;
    if (wgrad_sp_shape(M, N, K)) {                                               // whichever kernel the call ends up on
        const LimeWgradSpPlan sp = lime_wgrad_sp_plan(M, N, K);
        const int64_t need_sp = (int64_t)sp.splits * sp.np * sp.kp;
        if (need_sp > need) need = need_sp;
    }
    return need + (int64_t)colsum_blocks(M) * N;                                  // + the column-sum fallback of db
}

extern "C" int lime_linear_wgrad_f32(const float* dy, int64_t ldy, const float* x, int64_t ldx, float* dw, int64_t lddw,
                                     float* db, int32_t M, int32_t N, int32_t K, int32_t accumulate, float* workspace,
                                     int64_t workspace_floats, void* stream) {
    LIME_REQUIRE(dy && x && dw && workspace, LIME_ERR_BAD_ARG, "lime_linear_wgrad_f32: null pointer");
    LIME_REQUIRE(M > 0 && N > 0 && K > 0, LIME_ERR_BAD_ARG, "lime_linear_wgrad_f32: non-positive dimension");
    LIME_REQUIRE(ldy >= N && ldx >= K && lddw >= K, LIME_ERR_BAD_ARG, "lime_linear_wgrad_f32: leading dimension smaller than the row");
    const bool vec = N % 4 == 0 && K % 4 == 0 && lime_al16(dy, ldy) && lime_al16(x, ldx);
    static const bool no_dma = getenv("LIME_WGRAD_NO_DMA") != nullptr;        // A/B switch for tools/, not a product option
    const WgradPlan w = wgrad_plan(M, N, K, 1);
    LIME_REQUIRE(workspace_floats >= lime_linear_wgrad_workspace(M, N, K), LIME_ERR_BAD_ARG,
                 "lime_linear_wgrad_f32: workspace holds %ld floats, lime_linear_wgrad_workspace() asks for %ld",
                 (long)workspace_floats, (long)lime_linear_wgrad_workspace(M, N, K));
    hipStream_t s = (hipStream_t)stream;
    LIME_REQUIRE(((long)w.rows_per_split + WG_MC) * (ldy > ldx ? ldy : ldx) * 4 < 0x7FFFFFF0L, LIME_ERR_UNSUPPORTED,
                 "lime_linear_wgrad_f32: a row slice spans more than 2 GB (rows %d, ld %ld)", w.rows_per_split, (long)(ldy > ldx ? ldy : ldx));
    int st;
    static const bool no_sp = getenv("LIME_WGRAD_NO_SP") != nullptr;          // A/B switch for tools/
    if (vec && !no_sp && (lime_split_mode() & 1) && wgrad_sp_shape(M, N, K)) {
        const LimeWgradSpPlan sp = lime_wgrad_sp_plan(M, N, K);
        LIME_REQUIRE(((long)sp.rows_per_split + 32) * (ldy > ldx ? ldy : ldx) * 4 < 0x7FFFFFF0L, LIME_ERR_UNSUPPORTED,
                     "lime_linear_wgrad_f32: a row slice spans more than 2 GB (rows %d, ld %ld)", sp.rows_per_split, (long)(ldy > ldx ? ldy : ldx));
        const int ones = (!sp.swap && db != nullptr && K < sp.kp) ? 1 : 0;
        st = lime_wgrad_sp_launch(sp, dy, ldy, x, ldx, workspace, M, N, K, ones, s);
        if (st != LIME_OK) return st;
        const int64_t used = (int64_t)sp.splits * sp.np * sp.kp;
        if (sp.swap) st = lime_wgrad_sp_reduce_t(sp, workspace, dw, lddw, N, K, accumulate, s);
        else st = lime_reduce_partials(workspace, sp.np * sp.kp, sp.splits, sp.kp, dw, lddw, N, K, accumulate, s, ones ? db : nullptr);
        if (st != LIME_OK || db == nullptr || ones) return st;
        return lime_colsum_f32(dy, ldy, M, N, db, accumulate, workspace + used, workspace_floats - used, stream);
    }
    const int ones_col = (db != nullptr && K < w.kp) ? 1 : 0;          // room for a ones column in the padded tile grid
#define WGRAD(NKT) (vec ? (no_dma ? launch_wgrad<NKT, true>(w, dy, ldy, x, ldx, workspace, M, N, K, ones_col, s)              \
                                  : launch_wgrad_dma<NKT>(w, dy, ldy, x, ldx, workspace, M, N, K, ones_col, s))                \
                        : launch_wgrad<NKT, false>(w, dy, ldy, x, ldx, workspace, M, N, K, ones_col, s))
    if (w.nkt == 5) st = WGRAD(5); else if (w.nkt == 3) st = WGRAD(3); else st = WGRAD(4);
#undef WGRAD
    if (st != LIME_OK) return st;
    st = lime_reduce_partials(workspace, w.np * w.kp, w.splits, w.kp, dw, lddw, N, K, accumulate, s, ones_col ? db : nullptr);   // db: column K of the partial tiles
    if (st != LIME_OK || db == nullptr || ones_col) return st;
    float* cws = workspace + (int64_t)w.splits * w.np * w.kp;             // K fills its tiles: a separate column-sum pass
    return lime_colsum_f32(dy, ldy, M, N, db, accumulate, cws, workspace_floats - (int64_t)w.splits * w.np * w.kp, stream);
}
