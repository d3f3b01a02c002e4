// The occurrence side of the per-news content cache in one launch (LIME.encode_cached): a news occurs in many impressions, each
// time with its own freshness and lifetime, and the freshness representation tanh(dense(cat(E_f[b_f], E_l[b_l]))) takes only
// num_buckets^2 values (newsEncoders.py:60-83).  Per occurrence r: two threshold bucketings, two (four) row gathers, one combine:
//     pair = bucket(freshness[r]) * nb + bucket(lifetime[r])
//     CONCAT / ADD : out[r, :] = A[idx[r], :] + T[pair, :]
//     GATED        : g = sigmoid(P[idx[r], :] + Q[pair, :]);   out[r, :] = g * A[idx[r], :] + (1 - g) * T[pair, :]
// (what A / P / T / Q hold per fusion method: include/lime_hip.h).  The kernel is bandwidth bound: 12 + 4 D (rows read + 1) bytes
// an occurrence against D (CONCAT / ADD) or ~ 12 D (GATED) flops; the <= 100-row tables stay in L2.
//
// Launch form: a flat grid, one thread per 16 bytes of output, no loop, no LDS.  The compiler's report for the two instantiations is
// 16 / 29 VGPRs (add / gated), no scratch, 8 waves a SIMD (liblime_hip.resources.json), so latency is hidden by occupancy; a wave per row would
// idle 28 of 128 lane slots at D = 400 (100 column groups) and 31 of 256 at D = 900 for the sake of wave-uniform bucketing, which
// is ~ 40 VALU instructions a thread here, well under the memory time of its 48 - 80 bytes.  Each output element is a function of
// its own operands alone, written with explicit fmaf / single operations: a row's bits depend neither on R, on the row's position,
// nor on the grid.
#include "common.h"
#include "dev_helpers.h"

namespace {

template <bool GATED>
__global__ __launch_bounds__(256) void cached_occurrence_kernel(const int* __restrict__ idx, const float* __restrict__ freshness,
                                                                 const float* __restrict__ lifetime, const float* __restrict__ cuts,
                                                                 int n_cuts, const float* __restrict__ A, long lda,
                                                                 const float* __restrict__ P, long ldp, const float* __restrict__ T,
                                                                 long ldt, const float* __restrict__ Q, long ldq,
                                                                 float* __restrict__ out, long ldo, unsigned total, unsigned D4) {
    const unsigned e = blockIdx.x * 256u + threadIdx.x;            // total = rows * D4 < 2^31 (the host splits longer calls)
    if (e >= total) return;
    const unsigned r = e / D4;
    const int c = (int)(e - r * D4) * 4;
    const long n = idx[r];
    const int nb = (cuts != nullptr ? n_cuts : 9) + 1;
    const long pair = lime_dev::bucket_of(freshness[r], cuts, n_cuts) * nb + lime_dev::bucket_of(lifetime[r], cuts, n_cuts);
    const f32x4 a = *reinterpret_cast<const f32x4*>(A + n * lda + c);
    const f32x4 t = *reinterpret_cast<const f32x4*>(T + pair * ldt + c);
    f32x4 o;
    if (GATED) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(P + n * ldp + c);
        const f32x4 q = *reinterpret_cast<const f32x4*>(Q + pair * ldq + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float g = lime_sigmoid(p[k] + q[k]);
            o[k] = fmaf(g, a[k], (1.0f - g) * t[k]);               // one fixed order: the product of the freshness side, then the fma
        }
    } else {
        o = a + t;
    }
    *reinterpret_cast<f32x4*>(out + (long)r * ldo + c) = o;
}

}  // namespace

extern "C" int lime_cached_occurrence_f32(int32_t mode, const int32_t* idx, const float* freshness, const float* lifetime,
                                          const float* cuts, int32_t n_cuts, const float* A, int64_t lda, const float* P, int64_t ldp,
                                          const float* T, int64_t ldt, const float* Q, int64_t ldq, int64_t n_pairs, float* out,
                                          int64_t ldo, int64_t R, int32_t D, void* stream) {
    LIME_REQUIRE(mode == LIME_OCC_CONCAT || mode == LIME_OCC_ADD || mode == LIME_OCC_GATED, LIME_ERR_BAD_ARG,
                 "lime_cached_occurrence_f32: unknown mode %d", mode);
    const bool gated = mode == LIME_OCC_GATED;
    LIME_REQUIRE(idx && freshness && lifetime && A && T && out && (!gated || (P && Q)), LIME_ERR_BAD_ARG,
                 "lime_cached_occurrence_f32: NULL pointer");
    LIME_REQUIRE(R >= 0, LIME_ERR_BAD_ARG, "lime_cached_occurrence_f32: negative count");
    LIME_REQUIRE(D > 0 && D % 4 == 0, LIME_ERR_BAD_ARG, "lime_cached_occurrence_f32: D %d must be a positive multiple of 4", D);
    LIME_REQUIRE(cuts ? (n_cuts >= 0 && n_cuts <= 4096) : true, LIME_ERR_BAD_ARG, "lime_cached_occurrence_f32: bad cut count %d", n_cuts);
    const int64_t nb = (cuts ? n_cuts : 9) + 1;
    LIME_REQUIRE(n_pairs == nb * nb, LIME_ERR_BAD_ARG, "lime_cached_occurrence_f32: the tables must have %lld rows (num_buckets^2), got %lld",
                 (long long)(nb * nb), (long long)n_pairs);
    LIME_REQUIRE(lda >= D && ldt >= D && ldo >= D && (!gated || (ldp >= D && ldq >= D)), LIME_ERR_BAD_ARG,
                 "lime_cached_occurrence_f32: a row stride is smaller than D");
    LIME_REQUIRE(lime_al16(A, lda) && lime_al16(T, ldt) && lime_al16(out, ldo) && (!gated || (lime_al16(P, ldp) && lime_al16(Q, ldq))),
                 LIME_ERR_BAD_ARG, "lime_cached_occurrence_f32: rows must be 16-byte aligned (base pointers and row strides % 4)");
    const unsigned D4 = (unsigned)(D / 4);
    const int64_t rows_per_launch = 0x7FFFFF00LL / D4;             // rows * D4 stays below 2^31: 32-bit index arithmetic in the kernel
    for (int64_t r0 = 0; r0 < R; r0 += rows_per_launch) {
        const int64_t rows = R - r0 < rows_per_launch ? R - r0 : rows_per_launch;
        const unsigned total = (unsigned)(rows * D4);
        const dim3 grid((total + 255u) / 256u);
        float* o = out + r0 * ldo;
        if (gated)
            hipLaunchKernelGGL((cached_occurrence_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, idx + r0, freshness + r0,
                               lifetime + r0, cuts, n_cuts, A, (long)lda, P, (long)ldp, T, (long)ldt, Q, (long)ldq, o, (long)ldo, total, D4);
        else
            hipLaunchKernelGGL((cached_occurrence_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, idx + r0, freshness + r0,
                               lifetime + r0, cuts, n_cuts, A, (long)lda, P, (long)ldp, T, (long)ldt, Q, (long)ldq, o, (long)ldo, total, D4);
        const int st = lime_check_launch("lime_cached_occurrence_f32");
        if (st != LIME_OK) return st;
    }
    return LIME_OK;
}
