// Id and batch staging: what puts a batch into the layout the encoders read, without arithmetic beyond a compare or a blend --
// lifetime / freshness buckets, the live-sequence ids and the compact-order key mask of the masked title encoder, LIME's add / gated
// row fusion, row gathers (one table, or several tables by one index list), a multi-buffer copy and a per-row scale.
#include "common.h"
#include "dev_helpers.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// lifetime / freshness buckets: comparison against the fp32 cut points (lime_dev::bucket_of, dev_helpers.h)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bucketize_kernel(const float* __restrict__ x, int* __restrict__ out, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) out[e] = lime_dev::bucket_of(x[e], nullptr, 0);
}

}  // namespace

extern "C" int lime_bucketize_f32(const float* x, int32_t* out, int64_t n, void* stream) {
    LIME_REQUIRE(x && out, LIME_ERR_BAD_ARG, "lime_bucketize_f32: NULL pointer");
    LIME_REQUIRE(n >= 0, LIME_ERR_BAD_ARG, "lime_bucketize_f32: negative count");
    if (n == 0) return LIME_OK;
    hipLaunchKernelGGL(bucketize_kernel, dim3(lime_grid_cap(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x, out, (long)n);
    return lime_check_launch("lime_bucketize_f32");
}

namespace {

// the same against a caller-supplied ascending cut-point table (num_buckets != 10)
__global__ __launch_bounds__(256) void bucketize_cuts_kernel(const float* __restrict__ x, const float* __restrict__ cuts, int n_cuts,
                                                              int* __restrict__ out, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) out[e] = lime_dev::bucket_of(x[e], cuts, n_cuts);
}

}  // namespace

extern "C" int lime_bucketize_cuts_f32(const float* x, const float* cuts, int32_t n_cuts, int32_t* out, int64_t n, void* stream) {
    LIME_REQUIRE(x && out && cuts, LIME_ERR_BAD_ARG, "lime_bucketize_cuts_f32: NULL pointer");
    LIME_REQUIRE(n >= 0 && n_cuts >= 0 && n_cuts <= 4096, LIME_ERR_BAD_ARG, "lime_bucketize_cuts_f32: bad counts");
    if (n == 0) return LIME_OK;
    hipLaunchKernelGGL(bucketize_cuts_kernel, dim3(lime_grid_cap(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x, cuts, n_cuts, out, (long)n);
    return lime_check_launch("lime_bucketize_cuts_f32");
}

namespace {

// The masked title encoder (newsEncoders.py:566-595) on a compacted batch: a sequence repeats the all-padding representative when its
// ids are all zero AND its mask is the padding news' mask (first position set, corpus.py:476-477); an all-zero sequence under any
// other mask must be encoded -- it gets a sentinel (-1) in its first id so that lime_compact_sequences counts it as live.
// One wave per sequence.
__global__ __launch_bounds__(256) void mhsa_live_ids_kernel(const int* __restrict__ ids, const unsigned char* __restrict__ mask, int n, int T,
                                                             int* __restrict__ ids_eff) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n) return;
    bool allz = true, padmask = true;
    for (int t = lane; t < T; t += 64) {
        allz = allz && ids[(long)s * T + t] == 0;
        padmask = padmask && ((mask[(long)s * T + t] != 0) == (t == 0));
    }
    const bool odd = (__ballot(!allz) == 0ull) && (__ballot(!padmask) != 0ull);
    for (int t = lane; t < T; t += 64) {
        const int id = ids[(long)s * T + t];
        ids_eff[(long)s * T + t] = (t == 0 && odd) ? -1 : id;
    }
}

}  // namespace

extern "C" int lime_mhsa_live_ids(const int32_t* ids, const uint8_t* mask, int32_t n_seq, int32_t T, int32_t* ids_eff, void* stream) {
    LIME_REQUIRE(ids && mask && ids_eff, LIME_ERR_BAD_ARG, "lime_mhsa_live_ids: NULL pointer");
    LIME_REQUIRE(n_seq >= 0 && T > 0, LIME_ERR_BAD_ARG, "lime_mhsa_live_ids: bad dims");
    if (n_seq == 0) return LIME_OK;
    hipLaunchKernelGGL(mhsa_live_ids_kernel, dim3((unsigned)((n_seq + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ids, mask, n_seq, T, ids_eff);
    return lime_check_launch("lime_mhsa_live_ids");
}

namespace {

// ... and behind the compaction: the sentinel back to the padding word, the key mask in compact order (a compact slot without a
// source sequence -- the representative, unused slots -- carries the padding news' mask)
__global__ __launch_bounds__(256) void mhsa_compact_mask_kernel(int* __restrict__ ids_c, const int* __restrict__ seq_src,
                                                                 const unsigned char* __restrict__ mask, long total, int T,
                                                                 unsigned char* __restrict__ mask_c) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long cs = e / T;
        const int t = (int)(e - cs * T);
        const int src = seq_src[cs];
        mask_c[e] = src < 0 ? (unsigned char)(t == 0) : (unsigned char)(mask[(long)src * T + t] != 0);
        const int id = ids_c[e];
        if (id < 0) ids_c[e] = 0;
    }
}

}  // namespace

extern "C" int lime_mhsa_compact_mask(int32_t* ids_c, const int32_t* seq_src, const uint8_t* mask, int32_t n_compact_slots, int32_t T,
                                      uint8_t* mask_c, void* stream) {
    LIME_REQUIRE(ids_c && seq_src && mask && mask_c, LIME_ERR_BAD_ARG, "lime_mhsa_compact_mask: NULL pointer");
    LIME_REQUIRE(n_compact_slots >= 0 && T > 0, LIME_ERR_BAD_ARG, "lime_mhsa_compact_mask: bad dims");
    const long total = (long)n_compact_slots * T;
    if (total == 0) return LIME_OK;
    hipLaunchKernelGGL(mhsa_compact_mask_kernel, dim3(lime_grid_cap(total, 256, 2048)), dim3(256), 0, (hipStream_t)stream, ids_c, seq_src, mask, total, T, mask_c);
    return lime_check_launch("lime_mhsa_compact_mask");
}

namespace {

// LIME's 'add' / 'gated' fusion (newsEncoders.py:154-159): out = a + b, or gate * a + (1 - gate) * b
__global__ __launch_bounds__(256) void fuse_rows_kernel(const float* __restrict__ a, long lda, const float* __restrict__ b, long ldb,
                                                         const float* __restrict__ gate, long ldg, float* __restrict__ out, long ldo,
                                                         long rows, int cols) {
    const long total = rows * cols;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / cols;
        const int c = (int)(e - r * cols);
        const float x = a[r * lda + c], y = b[r * ldb + c];
        float v;
        if (gate) {
            const float g = gate[r * ldg + c];
            v = g * x + (1.0f - g) * y;
        } else {
            v = x + y;
        }
        out[r * ldo + c] = v;
    }
}

}  // namespace

extern "C" int lime_fuse_rows_f32(const float* a, int64_t lda, const float* b, int64_t ldb, const float* gate, int64_t ldg, float* out,
                                  int64_t ldo, int64_t rows, int32_t cols, void* stream) {
    LIME_REQUIRE(a && b && out, LIME_ERR_BAD_ARG, "lime_fuse_rows_f32: NULL pointer");
    LIME_REQUIRE(rows >= 0 && cols > 0 && lda >= cols && ldb >= cols && ldo >= cols && (!gate || ldg >= cols), LIME_ERR_BAD_ARG,
                 "lime_fuse_rows_f32: bad dims");
    if (rows == 0) return LIME_OK;
    hipLaunchKernelGGL(fuse_rows_kernel, dim3(lime_grid_cap(rows * cols, 256, 2048)), dim3(256), 0, (hipStream_t)stream, a, (long)lda, b, (long)ldb, gate,
                       (long)ldg, out, (long)ldo, (long)rows, cols);
    return lime_check_launch("lime_fuse_rows_f32");
}

namespace {

__global__ __launch_bounds__(256) void gather_rows_kernel(const int* __restrict__ idx, const float* __restrict__ table,
                                                           long ld_table, float* __restrict__ out, long ldo, long rows,
                                                           int dim) {
    const long total = rows * dim;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / dim;
        const int c = (int)(e - r * dim);
        out[r * ldo + c] = table[(long)idx[r] * ld_table + c];
    }
}

}  // namespace

extern "C" int lime_gather_rows_f32(const int32_t* idx, const float* table, int64_t ld_table, float* out, int64_t ldo,
                                    int64_t rows, int32_t dim, void* stream) {
    LIME_REQUIRE(idx && table && out, LIME_ERR_BAD_ARG, "lime_gather_rows_f32: NULL pointer");
    LIME_REQUIRE(rows >= 0 && dim > 0 && ld_table >= dim && ldo >= dim, LIME_ERR_BAD_ARG, "lime_gather_rows_f32: bad dims");
    if (rows == 0) return LIME_OK;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(lime_grid_cap(rows * dim, 256, 2048)), dim3(256), 0, (hipStream_t)stream, idx, table,
                       (long)ld_table, out, (long)ldo, (long)rows, dim);
    return lime_check_launch("lime_gather_rows_f32");
}

// ---------------------------------------------------------------------------------------------------
// multi-table row gather (device-side batch assembly): blockIdx.y = table, blockIdx.x = output row
// ---------------------------------------------------------------------------------------------------
struct GatherTable {
    lime_gather_desc d[LIME_MAX_GATHERS];
};

__global__ __launch_bounds__(64) void gather_rows_multi_kernel(const int* __restrict__ idx, const GatherTable t) {
    const lime_gather_desc d = t.d[blockIdx.y];
    const long r = blockIdx.x;
    const char* src = (const char*)d.table + (long)idx[r] * d.table_stride;
    char* dst = (char*)d.out + r * d.out_stride;
    const int n = d.row_bytes;
    if ((((uintptr_t)src | (uintptr_t)dst) & 3) == 0) {
        const int nw = n >> 2;
        for (int i = threadIdx.x; i < nw; i += 64) reinterpret_cast<unsigned*>(dst)[i] = reinterpret_cast<const unsigned*>(src)[i];
        for (int i = (nw << 2) + threadIdx.x; i < n; i += 64) dst[i] = src[i];
    } else {
        for (int i = threadIdx.x; i < n; i += 64) dst[i] = src[i];
    }
}

extern "C" int lime_gather_rows_multi(const int32_t* idx, int64_t n_rows, const lime_gather_desc* descs, int32_t n, void* stream) {
    LIME_REQUIRE(n >= 0 && n <= LIME_MAX_GATHERS, LIME_ERR_BAD_ARG, "lime_gather_rows_multi: n = %d outside [0, %d]", n, LIME_MAX_GATHERS);
    LIME_REQUIRE(n_rows >= 0 && n_rows <= 0x7FFFFFFF, LIME_ERR_BAD_ARG, "lime_gather_rows_multi: bad row count");
    if (n == 0 || n_rows == 0) return LIME_OK;
    LIME_REQUIRE(idx && descs, LIME_ERR_BAD_ARG, "lime_gather_rows_multi: NULL pointer");
    GatherTable t;
    for (int i = 0; i < n; ++i) {
        LIME_REQUIRE(descs[i].table && descs[i].out && descs[i].row_bytes > 0 && descs[i].table_stride >= descs[i].row_bytes &&
                     descs[i].out_stride >= descs[i].row_bytes, LIME_ERR_BAD_ARG, "lime_gather_rows_multi: bad descriptor %d", i);
        t.d[i] = descs[i];
    }
    hipLaunchKernelGGL(gather_rows_multi_kernel, dim3((unsigned)n_rows, (unsigned)n), dim3(64), 0, (hipStream_t)stream, idx, t);
    return lime_check_launch("lime_gather_rows_multi");
}

// ---------------------------------------------------------------------------------------------------
// multi-copy: blockIdx.y = buffer, blockIdx.x = 16 KB piece of it
// ---------------------------------------------------------------------------------------------------
struct CopyTable {
    lime_copy_desc d[LIME_MAX_COPIES];
};
constexpr long COPY_PIECE = 16384;

__global__ __launch_bounds__(256) void multi_copy_kernel(const CopyTable t) {
    const lime_copy_desc d = t.d[blockIdx.y];
    const long b0 = (long)blockIdx.x * COPY_PIECE;
    if (b0 >= d.bytes) return;
    const long n = d.bytes - b0 < COPY_PIECE ? d.bytes - b0 : COPY_PIECE;
    const char* src = (const char*)d.src + b0;
    char* dst = (char*)d.dst + b0;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const long nv = n >> 4;
        for (long i = threadIdx.x; i < nv; i += 256) reinterpret_cast<f32x4*>(dst)[i] = reinterpret_cast<const f32x4*>(src)[i];
        for (long i = (nv << 4) + threadIdx.x; i < n; i += 256) dst[i] = src[i];
    } else {
        for (long i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
    }
}

extern "C" int lime_multi_copy(const lime_copy_desc* descs, int32_t n, void* stream) {
    LIME_REQUIRE(n >= 0 && n <= LIME_MAX_COPIES, LIME_ERR_BAD_ARG, "lime_multi_copy: n = %d outside [0, %d]", n, LIME_MAX_COPIES);
    LIME_REQUIRE(n == 0 || descs, LIME_ERR_BAD_ARG, "lime_multi_copy: NULL descriptor table");
    CopyTable t;
    long most = 0;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        LIME_REQUIRE(descs[i].bytes >= 0, LIME_ERR_BAD_ARG, "lime_multi_copy: negative size");
        if (descs[i].bytes == 0) continue;
        LIME_REQUIRE(descs[i].src && descs[i].dst, LIME_ERR_BAD_ARG, "lime_multi_copy: NULL buffer");
        t.d[m++] = descs[i];
        most = descs[i].bytes > most ? descs[i].bytes : most;
    }
    if (m == 0) return LIME_OK;
    const long pieces = (most + COPY_PIECE - 1) / COPY_PIECE;
    LIME_REQUIRE(pieces <= 0x7FFFFFFF, LIME_ERR_UNSUPPORTED, "lime_multi_copy: buffer too large");
    hipLaunchKernelGGL(multi_copy_kernel, dim3((unsigned)pieces, (unsigned)m), dim3(256), 0, (hipStream_t)stream, t);
    return lime_check_launch("lime_multi_copy");
}

namespace {

__global__ __launch_bounds__(256) void row_scale_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                         float* __restrict__ out, long rows, int D) {
    const long total = rows * D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) out[e] = x[e] * scale[e / D];
}

}  // namespace

extern "C" int lime_row_scale_f32(const float* x, const float* scale, float* out, int64_t rows, int32_t D, void* stream) {
    LIME_REQUIRE(x && scale && out, LIME_ERR_BAD_ARG, "lime_row_scale_f32: NULL pointer");
    LIME_REQUIRE(rows >= 0 && D > 0, LIME_ERR_BAD_ARG, "lime_row_scale_f32: bad dims");
    if (rows == 0) return LIME_OK;
    hipLaunchKernelGGL(row_scale_kernel, dim3(lime_grid_cap(rows * D, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x, scale, out, (long)rows,
                       D);
    return lime_check_launch("lime_row_scale_f32");
}
