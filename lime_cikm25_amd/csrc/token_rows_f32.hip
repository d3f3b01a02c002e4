// Rows of tokens in and out of the token encoders, all HBM-bound: the embedding gather (+ positional table), the mean over the
// tokens of a sequence (three kernels by shape, a counted form for compacted batches), the intent layers' input from the pooled
// block rows of the distinct news, head padding of a weight, the copy of the position-only rows into padding tokens, and the two
// bf16 helpers of the bf16 encoder path (fp32 -> bf16 with zero padding, mean pool of bf16 rows).  Sums run in row order.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// embedding gather (+ positional table)
// ---------------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void embed_pe_kernel(const int* __restrict__ ids, const float* __restrict__ table,
                                                        long ld_table, const float* __restrict__ pe, long ld_pe, int period,
                                                        float* __restrict__ out, long ldo, long rows, int dim) {
    typedef float vec_t __attribute__((ext_vector_type(VEC)));
    const int vpr = dim / VEC;                                  // vectors per row
    const long total = rows * vpr;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / vpr;
        const int c = (int)(e - r * vpr) * VEC;
        vec_t v = *reinterpret_cast<const vec_t*>(table + (long)ids[r] * ld_table + c);
        if (pe) v += *reinterpret_cast<const vec_t*>(pe + (r % period) * ld_pe + c);
        *reinterpret_cast<vec_t*>(out + r * ldo + c) = v;
    }
}

__global__ __launch_bounds__(256) void embed_pe_scalar_kernel(const int* __restrict__ ids, const float* __restrict__ table,
                                                               long ld_table, const float* __restrict__ pe, long ld_pe,
                                                               int period, float* __restrict__ out, long ldo, long rows,
                                                               int dim) {
    const long total = rows * dim;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / dim;
        const int c = (int)(e - r * dim);
        float v = table[(long)ids[r] * ld_table + c];
        if (pe) v += pe[(r % period) * ld_pe + c];
        out[r * ldo + c] = v;
    }
}

}  // namespace

extern "C" int lime_embed_pe_f32(const int32_t* ids, const float* table, int64_t ld_table, const float* pe, int64_t ld_pe,
                                 int32_t period, float* out, int64_t ldo, int64_t rows, int32_t dim, void* stream) {
    LIME_REQUIRE(ids && table && out, LIME_ERR_BAD_ARG, "lime_embed_pe_f32: NULL pointer");
    LIME_REQUIRE(rows >= 0 && dim > 0 && ld_table >= dim && ldo >= dim, LIME_ERR_BAD_ARG, "lime_embed_pe_f32: bad dims");
    LIME_REQUIRE(!pe || (period > 0 && ld_pe >= dim), LIME_ERR_BAD_ARG, "lime_embed_pe_f32: pe needs period > 0, ld_pe >= dim");
    if (rows == 0) return LIME_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = dim % 4 == 0 && ld_table % 4 == 0 && ldo % 4 == 0 && (!pe || ld_pe % 4 == 0) &&
                    ((uintptr_t)table % 16 == 0) && ((uintptr_t)out % 16 == 0) && (!pe || (uintptr_t)pe % 16 == 0);
    if (v4)
        hipLaunchKernelGGL((embed_pe_kernel<4>), dim3(lime_grid_cap(rows * (dim / 4), 256, 8192)), dim3(256), 0, s, ids, table,
                           (long)ld_table, pe, (long)ld_pe, period, out, (long)ldo, (long)rows, dim);
    else
        hipLaunchKernelGGL(embed_pe_scalar_kernel, dim3(lime_grid_cap(rows * dim, 256, 8192)), dim3(256), 0, s, ids, table,
                           (long)ld_table, pe, (long)ld_pe, period, out, (long)ldo, (long)rows, dim);
    return lime_check_launch("lime_embed_pe_f32");
}

namespace {

// ---------------------------------------------------------------------------------------------------
// mean over the tokens of a sequence: one workgroup per sequence
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mean_pool_kernel(const float* __restrict__ x, long ldx, float* __restrict__ out,
                                                         long ldo, int S, int dim) {
    const long s = blockIdx.x;
    const float inv = 1.0f / (float)S;
    for (int d = threadIdx.x; d < dim; d += 256) {
        const float* px = x + s * S * ldx + d;
        float acc = 0.f;
        for (int t = 0; t < S; ++t) acc += px[(long)t * ldx];
        out[s * ldo + d] = acc * inv;
    }
}

// 16-byte variant: dim / 4 column threads x RG row groups (each sums every RG-th token in order), then a fixed-order
// sum of the RG partials through LDS -- whole 1200-byte rows per wave instruction, ~2x the bytes in flight
__global__ __launch_bounds__(256) void mean_pool_vec4_kernel(const float* __restrict__ x, long ldx, float* __restrict__ out,
                                                              long ldo, int S, int dim) {
    __shared__ f32x4 part[256];
    const long s = blockIdx.x;
    const int nc = dim >> 2;                       // float4 columns (<= 256)
    const int rg_n = 256 / nc;                     // row groups
    const int c = threadIdx.x % nc, rg = threadIdx.x / nc;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (rg < rg_n) {
        const float* px = x + s * S * ldx + c * 4;
        for (int t = rg; t < S; t += rg_n) acc += *reinterpret_cast<const f32x4*>(px + (long)t * ldx);
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (rg == 0) {
        for (int g = 1; g < rg_n; ++g) acc += part[g * nc + c];
        const float inv = 1.0f / (float)S;
        float* po = out + s * ldo + c * 4;
        po[0] = acc[0] * inv; po[1] = acc[1] * inv; po[2] = acc[2] * inv; po[3] = acc[3] * inv;
    }
}

// short "sequences" (the S / 32 block rows the pooled GEMM epilogue leaves: 4 rows at S = 128, 16 at S = 512): one thread per
// (sequence, four columns), rows summed in order -- a workgroup per sequence would be 8,000+ workgroups of almost no work
__global__ __launch_bounds__(256) void mean_pool_flat_kernel(const float* __restrict__ x, long ldx, float* __restrict__ out,
                                                              long ldo, long n_seq, int S, int dim, const int* __restrict__ n_seq_dev) {
    const int nc = dim >> 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (n_seq_dev) n_seq = min(n_seq, (long)*n_seq_dev);               // compacted batch: the sequences behind the count hold nothing
    if (e >= n_seq * nc) return;
    const long s = e / nc;
    const int c = (int)(e - s * nc) * 4;
    const float* px = x + s * S * ldx + c;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int t = 0;
    for (; t + 4 <= S; t += 4) {                                        // four rows in flight, added in row order
        const f32x4 r0 = *reinterpret_cast<const f32x4*>(px + (long)t * ldx);
        const f32x4 r1 = *reinterpret_cast<const f32x4*>(px + (long)(t + 1) * ldx);
        const f32x4 r2 = *reinterpret_cast<const f32x4*>(px + (long)(t + 2) * ldx);
        const f32x4 r3 = *reinterpret_cast<const f32x4*>(px + (long)(t + 3) * ldx);
        acc += r0; acc += r1; acc += r2; acc += r3;
    }
    for (; t < S; ++t) acc += *reinterpret_cast<const f32x4*>(px + (long)t * ldx);
    const float inv = 1.0f / (float)S;
    float* po = out + s * ldo + c;
    po[0] = acc[0] * inv; po[1] = acc[1] * inv; po[2] = acc[2] * inv; po[3] = acc[3] * inv;
}

}  // namespace

static int mean_pool(const float* x, int64_t ldx, float* out, int64_t ldo, int32_t n_seq, int32_t S, int32_t dim, const int32_t* n_seq_dev,
                     void* stream, const char* who) {
    LIME_REQUIRE(x && out, LIME_ERR_BAD_ARG, "lime_mean_pool_f32: NULL pointer");
    LIME_REQUIRE(n_seq >= 0 && S > 0 && dim > 0 && ldx >= dim && ldo >= dim, LIME_ERR_BAD_ARG, "lime_mean_pool_f32: bad dims");
    if (n_seq == 0) return LIME_OK;
    const bool v4 = dim % 4 == 0 && dim <= 1024 && ldx % 4 == 0 && ((uintptr_t)x % 16 == 0);
    LIME_REQUIRE(!n_seq_dev || (v4 && S <= 16), LIME_ERR_BAD_ARG,
                 "lime_mean_pool_count_f32: the counted form covers S <= 16 rows per sequence, dim %% 4 == 0, 16-byte aligned rows");
    if (v4 && S <= 16 && (n_seq >= 512 || n_seq_dev))
        hipLaunchKernelGGL(mean_pool_flat_kernel, dim3((unsigned)(((long)n_seq * (dim >> 2) + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           x, (long)ldx, out, (long)ldo, (long)n_seq, S, dim, n_seq_dev);
    else if (v4)
        hipLaunchKernelGGL(mean_pool_vec4_kernel, dim3((unsigned)n_seq), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, out,
                           (long)ldo, S, dim);
    else
        hipLaunchKernelGGL(mean_pool_kernel, dim3((unsigned)n_seq), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, out, (long)ldo,
                           S, dim);
    return lime_check_launch(who);
}

extern "C" int lime_mean_pool_f32(const float* x, int64_t ldx, float* out, int64_t ldo, int32_t n_seq, int32_t S, int32_t dim,
                                  void* stream) {
    return mean_pool(x, ldx, out, ldo, n_seq, S, dim, nullptr, stream, "lime_mean_pool_f32");
}

extern "C" int lime_mean_pool_count_f32(const float* x, int64_t ldx, float* out, int64_t ldo, int32_t n_seq, int32_t S, int32_t dim,
                                        const int32_t* n_seq_dev, void* stream) {
    LIME_REQUIRE(n_seq_dev, LIME_ERR_BAD_ARG, "lime_mean_pool_count_f32: NULL count");
    return mean_pool(x, ldx, out, ldo, n_seq, S, dim, n_seq_dev, stream, "lime_mean_pool_count_f32");
}

namespace {

// The pooled title and body of the DISTINCT news of a batch (lime_compact_batch) into the intent layers' input: row j of the title
// half is the mean of the nblk_t block rows of pooled sequence title_row[j], row cap + j of the body half the same from body_row[j];
// one thread per (half, news, four columns), block rows added in row order and scaled as mean_pool_flat_kernel does (one block row:
// the row itself).  News at or beyond *n_news are left alone.
__global__ __launch_bounds__(256) void news_xin_kernel(const float* __restrict__ tb, long ld_t, int nblk_t, const float* __restrict__ bb,
                                                        long ld_b, int nblk_b, const int* __restrict__ title_row,
                                                        const int* __restrict__ body_row, const int* __restrict__ n_news,
                                                        float* __restrict__ xin, long ldx, long cap, int dim) {
    const int nc = dim >> 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = min(cap, (long)*n_news);
    if (e >= 2 * cap * nc) return;
    const int half = e >= cap * nc;
    const long q = e - half * cap * nc;
    const long j = q / nc;
    if (j >= n) return;
    const int c = (int)(q - j * nc) * 4;
    const int S = half ? nblk_b : nblk_t;
    const long ld = half ? ld_b : ld_t;
    const float* px = (half ? bb : tb) + (long)(half ? body_row[j] : title_row[j]) * S * ld + c;
    float* po = xin + (half * cap + j) * ldx + c;
    if (S == 1) {
        *reinterpret_cast<f32x4*>(po) = *reinterpret_cast<const f32x4*>(px);
        return;
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < S; ++t) acc += *reinterpret_cast<const f32x4*>(px + (long)t * ld);
    const float inv = 1.0f / (float)S;
    po[0] = acc[0] * inv; po[1] = acc[1] * inv; po[2] = acc[2] * inv; po[3] = acc[3] * inv;
}

}  // namespace

extern "C" int lime_news_xin_f32(const float* title_blocks, int64_t ld_t, int32_t nblk_t, const float* body_blocks, int64_t ld_b,
                                 int32_t nblk_b, const int32_t* title_row, const int32_t* body_row, const int32_t* n_news, float* xin,
                                 int64_t ldx, int32_t cap, int32_t dim, void* stream) {
    LIME_REQUIRE(title_blocks && body_blocks && title_row && body_row && n_news && xin, LIME_ERR_BAD_ARG, "lime_news_xin_f32: NULL pointer");
    LIME_REQUIRE(cap >= 0 && dim > 0 && ld_t >= dim && ld_b >= dim && ldx >= dim, LIME_ERR_BAD_ARG, "lime_news_xin_f32: bad dims");
    LIME_REQUIRE(nblk_t >= 1 && nblk_t <= 16 && nblk_b >= 1 && nblk_b <= 16 && dim % 4 == 0 && ld_t % 4 == 0 && ld_b % 4 == 0 && ldx % 4 == 0 &&
                     (uintptr_t)title_blocks % 16 == 0 && (uintptr_t)body_blocks % 16 == 0 && (uintptr_t)xin % 16 == 0,
                 LIME_ERR_UNSUPPORTED, "lime_news_xin_f32: 1 .. 16 block rows per sequence, dim %% 4 == 0, 16-byte aligned rows");
    if (cap == 0) return LIME_OK;
    const long total = 2L * cap * (dim >> 2);
    LIME_REQUIRE((total + 255) / 256 <= 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_news_xin_f32: too many rows");
    hipLaunchKernelGGL(news_xin_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, title_blocks, (long)ld_t,
                       nblk_t, body_blocks, (long)ld_b, nblk_b, title_row, body_row, n_news, xin, (long)ldx, (long)cap, dim);
    return lime_check_launch("lime_news_xin_f32");
}

namespace {

__global__ __launch_bounds__(256) void pad_heads_kernel(const float* __restrict__ src, long lds_, float* __restrict__ dst, long ldd,
                                                         int n_blk, int hd, int hs, int cols) {
    const long total = (long)n_blk * hs * cols;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long row = e / cols;
        const int c = (int)(e - row * cols);
        const int blk = (int)(row / hs), d = (int)(row - (long)blk * hs);
        dst[row * ldd + c] = d < hd ? src[((long)blk * hd + d) * lds_ + c] : 0.f;
    }
}

}  // namespace

extern "C" int lime_pad_heads_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t n_blk, int32_t head_dim,
                                  int32_t head_stride, int32_t cols, void* stream) {
    LIME_REQUIRE(src && dst, LIME_ERR_BAD_ARG, "lime_pad_heads_f32: NULL pointer");
    LIME_REQUIRE(n_blk > 0 && head_dim > 0 && head_stride >= head_dim && cols > 0 && lds >= cols && ldd >= cols, LIME_ERR_BAD_ARG,
                 "lime_pad_heads_f32: bad dims");
    hipLaunchKernelGGL(pad_heads_kernel, dim3(lime_grid_cap((long)n_blk * head_stride * cols, 256, 2048)), dim3(256), 0, (hipStream_t)stream, src,
                       (long)lds, dst, (long)ldd, n_blk, head_dim, head_stride, cols);
    return lime_check_launch("lime_pad_heads_f32");
}

namespace {

// ---------------------------------------------------------------------------------------------------
// dst[r, :] = src[r % S, :] for the rows whose id is the padding word (0): the q / k / v rows of padding tokens depend on the position
// only, so the training forward computes in_proj over the live tokens and copies these S rows into the rest (cols % 4 == 0, 16-byte rows)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fill_pad_rows_kernel(const int* __restrict__ ids, const float* __restrict__ src, long lds,
                                                             float* __restrict__ dst, long ldd, long rows, int S, int c4n) {
    const long total = rows * c4n;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
        const long r = q / c4n;
        const int c = (int)(q - r * c4n) * 4;
        if (ids[r] == 0) *reinterpret_cast<f32x4*>(dst + r * ldd + c) = *reinterpret_cast<const f32x4*>(src + (r % S) * lds + c);
    }
}

}  // namespace

extern "C" int lime_fill_pad_rows_f32(const int32_t* ids, const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int32_t S,
                                      int32_t cols, void* stream) {
    LIME_REQUIRE(ids && src && dst, LIME_ERR_BAD_ARG, "lime_fill_pad_rows_f32: NULL pointer");
    LIME_REQUIRE(rows >= 0 && S > 0 && cols > 0 && lds >= cols && ldd >= cols, LIME_ERR_BAD_ARG, "lime_fill_pad_rows_f32: bad dimensions");
    LIME_REQUIRE(cols % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0, LIME_ERR_UNSUPPORTED,
                 "lime_fill_pad_rows_f32: needs 16-byte aligned rows and cols % 4 == 0");
    if (rows == 0) return LIME_OK;
    const long total = rows * (cols / 4);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(fill_pad_rows_kernel, dim3((unsigned)(blocks > 16384 ? 16384 : blocks)), dim3(256), 0, (hipStream_t)stream, ids, src,
                       (long)lds, dst, (long)ldd, (long)rows, S, cols / 4);
    return lime_check_launch("lime_fill_pad_rows_f32");
}

// ---------------------------------------------------------------------------------------------------
// bf16 path helpers (BASELINE config 3)
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {          // round to nearest even (finite inputs)
    unsigned u = __builtin_bit_cast(unsigned, f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// four output columns per thread (cols_out % 4 == 0): 8-byte stores
__global__ __launch_bounds__(256) void to_bf16_kernel(const float* __restrict__ src, long lds, long rows, int cols,
                                                      unsigned short* __restrict__ dst, long ldd, long rows_out, int cols_out) {
    const int q = cols_out >> 2;
    const long total = rows_out * q;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / q;
        const int c = (int)(e - r * q) * 4;
        unsigned short v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (r < rows && c + j < cols) ? f32_to_bf16(src[r * lds + c + j]) : (unsigned short)0;
        unsigned lo = v[0] | ((unsigned)v[1] << 16), hi = v[2] | ((unsigned)v[3] << 16);
        *reinterpret_cast<uint2*>(dst + r * ldd + c) = make_uint2(lo, hi);
    }
}

extern "C" int lime_to_bf16(const float* src, int64_t lds, int64_t rows, int32_t cols, uint16_t* dst, int64_t ldd, int64_t rows_out,
                            int32_t cols_out, void* stream) {
    LIME_REQUIRE(src && dst, LIME_ERR_BAD_ARG, "lime_to_bf16: NULL pointer");
    LIME_REQUIRE(rows >= 0 && cols > 0 && rows_out >= rows && cols_out >= cols && lds >= cols && ldd >= cols_out, LIME_ERR_BAD_ARG,
                 "lime_to_bf16: bad dims");
    LIME_REQUIRE(cols_out % 4 == 0 && ldd % 4 == 0 && (uintptr_t)dst % 8 == 0, LIME_ERR_BAD_ARG,
                 "lime_to_bf16: cols_out and ldd must be multiples of 4, dst 8-byte aligned");
    if (rows_out == 0) return LIME_OK;
    hipLaunchKernelGGL(to_bf16_kernel, dim3(lime_grid_cap(rows_out * (cols_out / 4), 256, 2048)), dim3(256), 0, (hipStream_t)stream, src,
                       (long)lds, (long)rows, cols, dst, (long)ldd, (long)rows_out, cols_out);
    return lime_check_launch("lime_to_bf16");
}

// one workgroup per sequence; thread = 4 columns x row group, fixed-order combine through LDS (as mean_pool_vec4_kernel)
__global__ __launch_bounds__(256) void mean_pool_bf16_kernel(const unsigned short* __restrict__ x, long ldx, float* __restrict__ out,
                                                              long ldo, int S, int dim) {
    __shared__ f32x4 part[256];
    const long s = blockIdx.x;
    const int nc = (dim + 3) >> 2;                 // 4-column groups (<= 256)
    const int rg_n = 256 / nc;
    const int c = threadIdx.x % nc, rg = threadIdx.x / nc;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (rg < rg_n) {
        const unsigned short* px = x + s * S * ldx + c * 4;
        for (int t = rg; t < S; t += rg_n) {
            const uint2 v = *reinterpret_cast<const uint2*>(px + (long)t * ldx);
            acc[0] += __builtin_bit_cast(float, v.x << 16);
            acc[1] += __builtin_bit_cast(float, v.x & 0xFFFF0000u);
            acc[2] += __builtin_bit_cast(float, v.y << 16);
            acc[3] += __builtin_bit_cast(float, v.y & 0xFFFF0000u);
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (rg == 0) {
        for (int g = 1; g < rg_n; ++g) acc += part[g * nc + c];
        const float inv = 1.0f / (float)S;
        for (int j = 0; j < 4; ++j)
            if (c * 4 + j < dim) out[s * ldo + c * 4 + j] = acc[j] * inv;
    }
}

extern "C" int lime_mean_pool_bf16(const uint16_t* x, int64_t ldx, float* out, int64_t ldo, int32_t n_seq, int32_t S, int32_t dim,
                                   void* stream) {
    LIME_REQUIRE(x && out, LIME_ERR_BAD_ARG, "lime_mean_pool_bf16: NULL pointer");
    LIME_REQUIRE(n_seq >= 0 && S > 0 && dim > 0 && ldo >= dim, LIME_ERR_BAD_ARG, "lime_mean_pool_bf16: bad dims");
    LIME_REQUIRE(dim <= 1024 && ldx % 4 == 0 && ldx >= (dim + 3) / 4 * 4 && (uintptr_t)x % 8 == 0, LIME_ERR_UNSUPPORTED,
                 "lime_mean_pool_bf16: dim <= 1024, ldx a multiple of 4 and >= dim rounded up to 4, x 8-byte aligned");
    if (n_seq == 0) return LIME_OK;
    hipLaunchKernelGGL(mean_pool_bf16_kernel, dim3((unsigned)n_seq), dim3(256), 0, (hipStream_t)stream, x, (long)ldx, out, (long)ldo,
                       S, dim);
    return lime_check_launch("lime_mean_pool_bf16");
}
