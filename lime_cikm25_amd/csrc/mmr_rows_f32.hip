// Maximal marginal relevance over a shortlist, a row per workgroup (Model.recommend / recommend_schedule / recommend_lists with
// mmr_lambda; recommend.mmr_select states it on the host).  A row is a shortlist of M <= 128 entries, best first: scores[j], and
// ids[j], the row of `table` [n, E] behind entry j.  An entry is DEAD when its id is outside [0, n) or its score is not finite: it is
// never taken and its table row is never read.  With first / last the first and last live entries,
//     rel[j] = (s[j] - s[last]) / (s[first] - s[last])      (0 for every j when the two are equal)
//     v[j]   = lam rel[j] - (1 - lam) pen[j],   pen[j] = max(0, max over the taken i of cos(j, i))
// and a round takes the live, untaken j of the largest v, the lower rank on equal v, until k are taken or none is left.
//
// The form (of the two that were on the table: a Gram matrix of the shortlist up front, or the picked row against the shortlist once
// per round): per round.  It is k M E multiply-adds against M^2 E / 2, k is far below M wherever this is called (10 of 64 or 128), and
// a [128, 128] fp32 Gram alone is the 64 KB of LDS a workgroup here may use.  So: the M inverse norms once; then per round the picked
// row, scaled by its inverse norm, goes to LDS in chunks of MMR_CHUNK floats, and its M dot products with the shortlist rows are
// formed from global memory (the rows sit in L2 after the norms) and fold into pen[] in LDS.  Every E is served: a lane keeps its
// partial sums across the chunks, so the sum's order is a function of E alone.
//
// Who does what, 256 threads: the 16 GROUPS of 16 lanes own the rows g, g + 16, .. (eight at the most); a group's lane t sums the
// quads t, t + 16, .. of a row with explicit fmaf in element order, the 16 partial sums meet in lime_dev::row16_sum and the group's
// lane 0 is the one that uses the total.  The selection state is kept by EVERY wave for itself, lane l owning the entries l and
// l + 64 (lam rel, live, taken): each wave reads pen[] and finds the round's pick by a wave reduction on (v, rank), the lower rank
// winning equal v -- the four waves compute the same pick from the same numbers, so nothing is broadcast and the loop's exit is
// uniform.  A NaN v (a table that holds non-finite values) ranks as the lowest number.
//
// All arithmetic fp32, fixed order, no atomics, no workspace: a row's picks are a function of its own operands (and of lam, k, M, E)
// alone -- not of R, the row's position or the run.  lam == 1 reads no table row at all.  LDS: 8 KB chunk + 1.5 KB.
#include "dev_helpers.h"

namespace {

constexpr int MMR_MAX = 128;         // entries of a shortlist: the top-k kernels' k limit
constexpr int MMR_CHUNK = 2048;      // floats of the picked row in LDS at a time (a multiple of 64: a lane's quads stay its own)
constexpr int MMR_ROWS = MMR_MAX / 16;

// The group's part of one chunk: acc[i] += sum over the chunk's quads q = t, t + 16, .. of row[i] . (SELF ? row[i] : x), rows with a
// null pointer skipped.  q0: the chunk's first quad, nq: its quads.
template <bool VEC, bool SELF>
__device__ __forceinline__ void group_dots(const float* const (&rows)[MMR_ROWS], const f32x4* x, int q0, int nq, int E, int t,
                                           float (&acc)[MMR_ROWS]) {
    for (int q = t; q < nq; q += 16) {
        f32x4 xq = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!SELF) xq = x[q];
#pragma unroll
        for (int i = 0; i < MMR_ROWS; ++i) {
            if (rows[i]) {
                const f32x4 a = row_quad<VEC, long>(rows[i], (long)(q0 + q), E);
                acc[i] = fma_dot4(a, SELF ? a : xq, acc[i]);
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void mmr_rows_kernel(const float* __restrict__ scores, const int* __restrict__ ids, int M,
                                                        const float* __restrict__ table, long ld, long n, int E, float lam, int k,
                                                        int* __restrict__ picks) {
    __shared__ f32x4 x[MMR_CHUNK / 4];
    __shared__ int id_of[MMR_MAX];
    __shared__ float inv[MMR_MAX];
    __shared__ float pen[MMR_MAX];
    const long row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, g = tid >> 4, t = tid & 15;
    const float* s = scores + row * M;
    const int* idr = ids + row * M;
    int* out = picks + row * k;
    const float oml = 1.0f - lam;

    // every wave: its lanes' two entries, the row's first / last live entry, lam rel
    const int j0 = lane, j1 = lane + 64;
    const float s0 = j0 < M ? s[j0] : 0.f, s1 = j1 < M ? s[j1] : 0.f;
    const int i0 = j0 < M ? idr[j0] : -1, i1 = j1 < M ? idr[j1] : -1;
    const bool live0 = i0 >= 0 && (long)i0 < n && __builtin_isfinite(s0);
    const bool live1 = i1 >= 0 && (long)i1 < n && __builtin_isfinite(s1);
    const unsigned long long m0 = __ballot(live0), m1 = __ballot(live1);
    if (tid < 64) {
        id_of[j0] = live0 ? i0 : -1;
        id_of[j1] = live1 ? i1 : -1;
        pen[j0] = 0.f;
        pen[j1] = 0.f;
        inv[j0] = 0.f;
        inv[j1] = 0.f;
    }
    float a0 = 0.f, a1 = 0.f;                                 // lam rel of the lane's entries
    if (m0 | m1) {                                            // (wave-uniform)
        const int first = m0 ? __ffsll((long long)m0) - 1 : 64 + __ffsll((long long)m1) - 1;
        const int last = m1 ? 127 - __clzll((long long)m1) : 63 - __clzll((long long)m0);
        const float lo0 = __shfl(s0, first & 63), lo1 = __shfl(s1, first & 63);
        const float hi0 = __shfl(s0, last & 63), hi1 = __shfl(s1, last & 63);
        const float s_first = first < 64 ? lo0 : lo1, s_last = last < 64 ? hi0 : hi1;
        const float span = s_first - s_last;
        if (span != 0.f) {
            a0 = live0 ? lam * ((s0 - s_last) / span) : 0.f;
            a1 = live1 ? lam * ((s1 - s_last) / span) : 0.f;
        }
    }
    bool open0 = live0, open1 = live1;                        // live and not taken
    __syncthreads();

    // the group's rows (null: dead, or behind M), and their inverse norms
    const bool cosines = oml != 0.f;                          // lam == 1: the penalty has no weight
    const float* rows[MMR_ROWS];
#pragma unroll
    for (int i = 0; i < MMR_ROWS; ++i) {
        const int id = id_of[g + 16 * i];                     // (-1 behind M: written above for all 128)
        rows[i] = cosines && id >= 0 ? table + (long)id * ld : nullptr;
    }
    const int nq_all = E / 4;
    if (cosines) {
        float acc[MMR_ROWS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        group_dots<VEC, true>(rows, nullptr, 0, nq_all, E, t, acc);
#pragma unroll
        for (int i = 0; i < MMR_ROWS; ++i) {
            const float ss = lime_dev::row16_sum(acc[i]);
            if (t == 0 && rows[i]) inv[g + 16 * i] = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
        }
        __syncthreads();
    }

    int r = 0;
    for (; r < k; ++r) {
        // every wave: the round's pick
        float v0 = a0 - oml * pen[j0], v1 = a1 - oml * pen[j1];
        v0 = v0 == v0 ? v0 : -3.402823466e38f;
        v1 = v1 == v1 ? v1 : -3.402823466e38f;
        const best_pick b0 = open0 ? best_pick{v0, j0} : best_pick{-INFINITY, 0x7FFFFFFF};
        const best_pick b1 = open1 ? best_pick{v1, j1} : best_pick{-INFINITY, 0x7FFFFFFF};
        const best_pick best = wave_best_pick(better_pick(b0, b1));
        if (best.j == 0x7FFFFFFF) break;                      // no live entry left (the same in every wave)
        if (tid == 0) out[r] = best.j;
        open0 = open0 && j0 != best.j;
        open1 = open1 && j1 != best.j;
        if (r + 1 == k || !cosines) continue;
        // the picked row against the shortlist, a chunk at a time
        const float* picked = table + (long)id_of[best.j] * ld;
        const float scale = inv[best.j];
        float acc[MMR_ROWS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int q0 = 0; q0 < nq_all; q0 += MMR_CHUNK / 4) {
            const int nq = nq_all - q0 < MMR_CHUNK / 4 ? nq_all - q0 : MMR_CHUNK / 4;
            if (q0) __syncthreads();                          // the readers of the chunk before
            for (int q = tid; q < nq; q += 256) x[q] = row_quad<VEC, long>(picked, (long)(q0 + q), E) * scale;
            __syncthreads();
            group_dots<VEC, false>(rows, x, q0, nq, E, t, acc);
        }
#pragma unroll
        for (int i = 0; i < MMR_ROWS; ++i) {
            const float dot = lime_dev::row16_sum(acc[i]);
            const int j = g + 16 * i;
            if (t == 0 && rows[i]) pen[j] = fmaxf(pen[j], dot * inv[j]);     // (a NaN cosine leaves pen as it is)
        }
        __syncthreads();                                      // pen[] for the next round; x[] is free again
    }
    for (int j = r + tid; j < k; j += 256) out[j] = -1;
}

}  // namespace

extern "C" int lime_mmr_rows_f32(const float* scores, const int32_t* ids, int64_t R, int32_t M, const float* table, int64_t ld, int64_t n,
                                 int32_t E, float lam, int32_t k, int32_t* picks, void* stream) {
    LIME_REQUIRE(scores && ids && table && picks, LIME_ERR_BAD_ARG, "lime_mmr_rows_f32: NULL pointer");
    LIME_REQUIRE(R >= 0 && M >= 1 && k >= 1 && k <= M && n >= 1 && E >= 1 && ld >= E, LIME_ERR_BAD_ARG,
                 "lime_mmr_rows_f32: bad dims (R %lld, M %d, k %d, n %lld, E %d, ld %lld): R >= 0, 1 <= k <= M, n >= 1, 1 <= E <= ld",
                 (long long)R, M, k, (long long)n, E, (long long)ld);
    LIME_REQUIRE(lam >= 0.f && lam <= 1.f, LIME_ERR_BAD_ARG, "lime_mmr_rows_f32: lam %g outside [0, 1]", (double)lam);
    LIME_REQUIRE(M <= MMR_MAX && E % 4 == 0 && R <= 65535, LIME_ERR_UNSUPPORTED,
                 "lime_mmr_rows_f32: M %d, E %d, R %lld outside M <= %d, E %% 4 == 0, R <= 65535", M, E, (long long)R, MMR_MAX);
    if (R == 0) return LIME_OK;
    if (lime_al16(table, (long)ld))
        hipLaunchKernelGGL(mmr_rows_kernel<true>, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, scores, (const int*)ids, (int)M, table,
                           (long)ld, (long)n, (int)E, lam, (int)k, (int*)picks);
    else
        hipLaunchKernelGGL(mmr_rows_kernel<false>, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, scores, (const int*)ids, (int)M, table,
                           (long)ld, (long)n, (int)E, lam, (int)k, (int*)picks);
    return lime_check_launch("lime_mmr_rows_f32");
}
