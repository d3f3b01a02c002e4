// The tail of the news encoders behind the token layers, one workgroup per news or sequence: the topic representation (category +
// subcategory embeddings through a small dense layer), CROWN's intent attention + cosine similarity + concat, and the additive
// attention pool of the MHSA encoder.  The `_count_` entries take the number of live rows from the device (a compacted batch).
// All reductions are fixed-order (wave64 shuffles, then LDS across the four waves): results are bitwise reproducible run to run.
// Their backward: tail_backward_f32.hip.
#include "common.h"
#include "dev_helpers.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// topic representation: one 64-thread workgroup per news
// ---------------------------------------------------------------------------------------------------
// Row r of the topic representation, by the 64 threads of a workgroup: the raw embedding pair into emb_out (when given), the dense
// layer over it into out and -- when given -- the same values into out2 (a second copy of the row: each lane stores what it summed).
// Stated once for topic_rep_kernel and news_keys_kernel: same lanes, same order of the sums.
__device__ __forceinline__ void topic_rep_row(long r, const int* __restrict__ cat, const int* __restrict__ sub,
                                              const float* __restrict__ cat_table, const float* __restrict__ sub_table, int dc, int ds,
                                              const float* __restrict__ w, const float* __restrict__ bias, int dout,
                                              float* __restrict__ out, float* __restrict__ out2, long ldo, float* __restrict__ emb_out,
                                              long ld_emb, float* e) {
    const int din = dc + ds;
    const float* crow = cat_table + (long)cat[r] * dc;
    const float* srow = sub_table + (long)sub[r] * ds;
    for (int i = threadIdx.x; i < din; i += 64) {
        const float v = (i < dc) ? crow[i] : srow[i - dc];
        e[i] = v;
        if (emb_out) emb_out[r * ld_emb + i] = v;
    }
    __syncthreads();
    if (out) {
        for (int o = threadIdx.x; o < dout; o += 64) {
            const float* wr = w + (long)o * din;
            float acc = 0.f;
            for (int i = 0; i < din; ++i) acc += wr[i] * e[i];
            const float y = acc + (bias ? bias[o] : 0.f);
            out[r * ldo + o] = y;
            if (out2) out2[r * ldo + o] = y;
        }
    }
}

__global__ __launch_bounds__(64) void topic_rep_kernel(const int* __restrict__ cat, const int* __restrict__ sub,
                                                        const float* __restrict__ cat_table, const float* __restrict__ sub_table,
                                                        int dc, int ds, const float* __restrict__ w, const float* __restrict__ bias,
                                                        int dout, float* __restrict__ out, long ldo, float* __restrict__ emb_out,
                                                        long ld_emb) {
    __shared__ float e[256];
    topic_rep_row(blockIdx.x, cat, sub, cat_table, sub_table, dc, ds, w, bias, dout, out, nullptr, ldo, emb_out, ld_emb, e);
}

// What the distinct news of a batch need from their keys, one 64-thread workgroup per compact news j of `rows` (the capacity: unused
// slots hold key 0, a valid id and bucket): the bucket pair, the topic row into BOTH halves of the intent layers' input xin
// [2 rows, ldx] (rows j and rows + j, columns [col0, col0 + dout)), zeros into the pad columns [col0 + dout, ldx) of both, and the raw
// embedding pair into emb_out.  Columns [0, col0) belong to lime_news_xin_f32.
__global__ __launch_bounds__(64) void news_keys_kernel(const int* __restrict__ cat, const int* __restrict__ sub,
                                                        const float* __restrict__ fresh, const float* __restrict__ life,
                                                        const float* __restrict__ cuts, int n_cuts, int nb,
                                                        const float* __restrict__ cat_table, const float* __restrict__ sub_table,
                                                        int dc, int ds, const float* __restrict__ w, const float* __restrict__ bias,
                                                        int dout, float* __restrict__ xin, long ldx, int col0, long rows,
                                                        float* __restrict__ emb_out, long ld_emb, int* __restrict__ pair) {
    __shared__ float e[256];
    const long j = blockIdx.x;
    if (threadIdx.x == 0) pair[j] = lime_dev::bucket_of(fresh[j], cuts, n_cuts) * nb + lime_dev::bucket_of(life[j], cuts, n_cuts);
    float* top = xin + col0;
    float* bot = xin + rows * ldx + col0;
    for (int c = dout + threadIdx.x; c < (int)ldx - col0; c += 64) {
        top[j * ldx + c] = 0.f;
        bot[j * ldx + c] = 0.f;
    }
    topic_rep_row(j, cat, sub, cat_table, sub_table, dc, ds, w, bias, dout, top, bot, ldx, emb_out, ld_emb, e);
}

}  // namespace

extern "C" int lime_topic_rep_f32(const int32_t* cat, const int32_t* sub, const float* cat_table, const float* sub_table,
                                  int32_t dc, int32_t ds, const float* w, const float* bias, int32_t dout, float* out,
                                  int64_t ldo, float* emb_out, int64_t ld_emb, int64_t rows, void* stream) {
    LIME_REQUIRE(cat && sub && cat_table && sub_table, LIME_ERR_BAD_ARG, "lime_topic_rep_f32: NULL pointer");
    LIME_REQUIRE(out || emb_out, LIME_ERR_BAD_ARG, "lime_topic_rep_f32: nothing to write");
    LIME_REQUIRE(!out || (w && dout > 0 && ldo >= dout), LIME_ERR_BAD_ARG, "lime_topic_rep_f32: out needs w, dout, ldo");
    LIME_REQUIRE(dc > 0 && ds > 0 && dc + ds <= 256, LIME_ERR_UNSUPPORTED, "lime_topic_rep_f32: dc + ds must be in (0, 256]");
    LIME_REQUIRE(!emb_out || ld_emb >= dc + ds, LIME_ERR_BAD_ARG, "lime_topic_rep_f32: ld_emb too small");
    if (rows <= 0) return rows == 0 ? LIME_OK : LIME_ERR_BAD_ARG;
    hipLaunchKernelGGL(topic_rep_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, cat, sub, cat_table, sub_table, dc,
                       ds, w, bias, dout, out, (long)ldo, emb_out, (long)ld_emb);
    return lime_check_launch("lime_topic_rep_f32");
}

extern "C" int lime_news_keys_f32(const int32_t* cat, const int32_t* sub, const float* fresh, const float* life, const float* cuts,
                                  int32_t n_cuts, int32_t nb, const float* cat_table, const float* sub_table, int32_t dc, int32_t ds,
                                  const float* w, const float* bias, int32_t dout, float* xin, int64_t ldx, int32_t col0, float* emb_out,
                                  int64_t ld_emb, int32_t* pair, int64_t rows, void* stream) {
    LIME_REQUIRE(cat && sub && fresh && life && cat_table && sub_table && w && xin && emb_out && pair, LIME_ERR_BAD_ARG,
                 "lime_news_keys_f32: NULL pointer");
    LIME_REQUIRE(cuts ? (n_cuts >= 0 && n_cuts <= 4096 && nb == n_cuts + 1) : nb == 10, LIME_ERR_BAD_ARG,
                 "lime_news_keys_f32: nb %d does not match the cut points (%d given; 10 buckets built in)", nb, cuts ? n_cuts : 9);
    LIME_REQUIRE(dc > 0 && ds > 0 && dc + ds <= 256, LIME_ERR_UNSUPPORTED, "lime_news_keys_f32: dc + ds must be in (0, 256]");
    LIME_REQUIRE(dout > 0 && col0 >= 0 && ldx >= (int64_t)col0 + dout && ldx < 0x7FFFFFFFL && ld_emb >= dc + ds, LIME_ERR_BAD_ARG,
                 "lime_news_keys_f32: bad dims dout=%d col0=%d ldx=%ld ld_emb=%ld", dout, col0, (long)ldx, (long)ld_emb);
    if (rows <= 0) return rows == 0 ? LIME_OK : LIME_ERR_BAD_ARG;
    LIME_REQUIRE(rows < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_news_keys_f32: too many rows");
    hipLaunchKernelGGL(news_keys_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, cat, sub, fresh, life, cuts, n_cuts, nb,
                       cat_table, sub_table, dc, ds, w, bias, dout, xin, (long)ldx, col0, (long)rows, emb_out, (long)ld_emb, pair);
    return lime_check_launch("lime_news_keys_f32");
}

namespace {

// ---------------------------------------------------------------------------------------------------
// intent attention + cosine similarity + concat: one workgroup per news
// ---------------------------------------------------------------------------------------------------
constexpr int MAX_INTENT = 8;

__global__ __launch_bounds__(256) void intent_fuse_kernel(const float* __restrict__ intents, const float* __restrict__ hidden,
                                                           const float* __restrict__ aff2_t, const float* __restrict__ aff2_b,
                                                           float* __restrict__ content, long ldc, long M, int k, int D, int A,
                                                           const int* __restrict__ m_dev) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // [2][D] pooled vectors, then 4 floats of scratch
    float* pooled = sm;
    float* red = sm + 2 * D;
    const long m = blockIdx.x;
    if (m_dev && m >= (long)*m_dev) return;                      // (uniform per workgroup) distinct news only: the rows behind the count hold nothing
    for (int tb = 0; tb < 2; ++tb) {
        const float* aff2 = tb == 0 ? aff2_t : aff2_b;
        const float* hid = hidden + ((long)tb * M + m) * k * A;
        const float* itn = intents + ((long)tb * M + m) * k * D;
        float a[MAX_INTENT];
        float mx = -INFINITY;
        for (int kk = 0; kk < k; ++kk) {
            float part = 0.f;
            for (int j = threadIdx.x; j < A; j += 256) part += hid[kk * A + j] * aff2[j];
            a[kk] = block_sum(part, red);
            mx = fmaxf(mx, a[kk]);
        }
        float den = 0.f;
        for (int kk = 0; kk < k; ++kk) {
            a[kk] = expf(a[kk] - mx);
            den += a[kk];
        }
        const float inv = 1.0f / den;
        for (int d = threadIdx.x; d < D; d += 256) {
            float x = 0.f;
            for (int kk = 0; kk < k; ++kk) x += (a[kk] * inv) * itn[kk * D + d];
            pooled[tb * D + d] = x;
        }
    }
    __syncthreads();
    float dot = 0.f, n1 = 0.f, n2 = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        const float t = pooled[d], b = pooled[D + d];
        dot += t * b;
        n1 += t * t;
        n2 += b * b;
    }
    dot = block_sum(dot, red);
    n1 = block_sum(n1, red);
    n2 = block_sum(n2, red);
    // F.cosine_similarity(eps = 1e-8): each norm is clamped from below
    const float cosv = dot / (fmaxf(sqrtf(n1), 1e-8f) * fmaxf(sqrtf(n2), 1e-8f));
    const float s = (cosv + 1.0f) * 0.5f;
    for (int d = threadIdx.x; d < D; d += 256) {
        content[m * ldc + d] = pooled[d];
        content[m * ldc + D + d] = s * pooled[D + d];
    }
}

}  // namespace

static int intent_fuse(const float* intents, const float* att_hidden, const float* affine2_t, const float* affine2_b, float* content,
                       int64_t ldc, int64_t M, int32_t k, int32_t D, int32_t A, const int32_t* m_dev, void* stream) {
    LIME_REQUIRE(intents && att_hidden && affine2_t && affine2_b && content, LIME_ERR_BAD_ARG, "lime_intent_fuse_f32: NULL pointer");
    LIME_REQUIRE(M >= 0 && k > 0 && D > 0 && A > 0 && ldc >= 2 * (int64_t)D, LIME_ERR_BAD_ARG, "lime_intent_fuse_f32: bad dims");
    LIME_REQUIRE(k <= MAX_INTENT && D <= 4096, LIME_ERR_UNSUPPORTED, "lime_intent_fuse_f32: k <= 8 and D <= 4096 only");
    if (M == 0) return LIME_OK;
    const size_t lds = (size_t)(2 * D + 4) * sizeof(float);
    hipLaunchKernelGGL(intent_fuse_kernel, dim3((unsigned)M), dim3(256), lds, (hipStream_t)stream, intents, att_hidden, affine2_t,
                       affine2_b, content, (long)ldc, (long)M, k, D, A, m_dev);
    return lime_check_launch("lime_intent_fuse_f32");
}

extern "C" int lime_intent_fuse_f32(const float* intents, const float* att_hidden, const float* affine2_t,
                                    const float* affine2_b, float* content, int64_t ldc, int64_t M, int32_t k, int32_t D,
                                    int32_t A, void* stream) {
    return intent_fuse(intents, att_hidden, affine2_t, affine2_b, content, ldc, M, k, D, A, nullptr, stream);
}

extern "C" int lime_intent_fuse_count_f32(const float* intents, const float* att_hidden, const float* affine2_t, const float* affine2_b,
                                          float* content, int64_t ldc, int64_t M, int32_t k, int32_t D, int32_t A, const int32_t* m_dev,
                                          void* stream) {
    LIME_REQUIRE(m_dev, LIME_ERR_BAD_ARG, "lime_intent_fuse_count_f32: NULL count");
    return intent_fuse(intents, att_hidden, affine2_t, affine2_b, content, ldc, M, k, D, A, m_dev, stream);
}

namespace {

// ---------------------------------------------------------------------------------------------------
// additive attention pooling over the tokens of a sequence (MHSA news encoder): one workgroup / sequence
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void additive_pool_kernel(const float* __restrict__ hidden, long ldh,
                                                             const float* __restrict__ aff2, int A, const float* __restrict__ x,
                                                             long ldx, int D, const unsigned char* __restrict__ mask,
                                                             float* __restrict__ out, long ldo, int S, const int* __restrict__ n_seq_dev) {
    __shared__ float alpha[512];
    __shared__ float red[4];
    const long s = blockIdx.x;
    // a compacted batch: only min(*n_seq_dev, grid) sequences are live (the rows behind them hold stale data: 100 MB of reads at config 2)
    if (n_seq_dev != nullptr && (int)blockIdx.x >= *n_seq_dev) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < S; t += 4) {
        const float* h = hidden + (s * S + t) * ldh;
        float part = 0.f;
        for (int j = lane; j < A; j += 64) part += h[j] * aff2[j];
        part = wave_sum(part);
        if (lane == 0) alpha[t] = (mask && mask[s * S + t] == 0) ? -1e9f : part;
    }
    __syncthreads();
    const float inv = block_softmax_terms(alpha, S, red);
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) {
        float acc = 0.f;
        for (int t = 0; t < S; ++t) acc += (alpha[t] * inv) * x[(s * S + t) * ldx + d];
        out[s * ldo + d] = acc;
    }
}

}  // namespace

extern "C" int lime_additive_pool_count_f32(const float* hidden, int64_t ldh, const float* affine2, int32_t A, const float* x,
                                            int64_t ldx, int32_t D, const uint8_t* mask, const int32_t* n_seq_dev, float* out, int64_t ldo,
                                            int32_t n_seq, int32_t S, void* stream) {
    LIME_REQUIRE(hidden && affine2 && x && out, LIME_ERR_BAD_ARG, "lime_additive_pool_f32: NULL pointer");
    LIME_REQUIRE(n_seq >= 0 && S > 0 && A > 0 && D > 0 && ldh >= A && ldx >= D && ldo >= D, LIME_ERR_BAD_ARG,
                 "lime_additive_pool_f32: bad dims");
    LIME_REQUIRE(S <= 512, LIME_ERR_UNSUPPORTED, "lime_additive_pool_f32: S %d > 512", S);
    if (n_seq == 0) return LIME_OK;
    hipLaunchKernelGGL(additive_pool_kernel, dim3((unsigned)n_seq), dim3(256), 0, (hipStream_t)stream, hidden, (long)ldh, affine2, A,
                       x, (long)ldx, D, mask, out, (long)ldo, S, n_seq_dev);
    return lime_check_launch("lime_additive_pool_f32");
}

extern "C" int lime_additive_pool_f32(const float* hidden, int64_t ldh, const float* affine2, int32_t A, const float* x,
                                      int64_t ldx, int32_t D, const uint8_t* mask, float* out, int64_t ldo, int32_t n_seq,
                                      int32_t S, void* stream) {
    return lime_additive_pool_count_f32(hidden, ldh, affine2, A, x, ldx, D, mask, nullptr, out, ldo, n_seq, S, stream);
}
