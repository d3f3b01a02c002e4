// lime_compact_sequences: which token sequences of a batch are worth encoding, and which of their rows.
//
// The reference pushes every slot of every impression through the token encoders (newsEncoders.py:311-321): H history slots
// that are padded with the all-zero <PAD> news (corpus.py:476-477, dataset.py:105-141) and, inside every real news, the
// padding tokens behind its text.  Both are exact repetitions:
//   * an all-padding sequence has the same pooled output wherever it occurs (the encoder layer has no mask and no
//     cross-sequence term), so ONE representative is encoded and every such slot reads its result;
//   * a padding token's in_proj row depends on its position only ((E[0] + PE[t]) W^T + b), so in_proj runs over the live
//     tokens and attention reads the S table rows for the rest (lime_token_attention_f32, rows form).
// Nothing is approximated and nothing is cached between forwards.  This file turns the [n_seq, S] id matrix into the index
// lists those kernels consume -- on the device, in fixed-size buffers, with the counts in device memory, so that the
// whole forward stays one HIP graph:
//   seq_inv  [n_seq]           original sequence -> compact sequence (all-padding sequences -> n_live, the representative)
//   ids_c    [(n_seq + 1) S]   token ids in compact order (representative: zeros)
//   row_map  [(n_seq + 1) S]   compact token row -> its q/k/v row: itself when live, pad_base + t when padding
//   tok_ids  [(n_seq + 1) S]   the live tokens' ids, compacted in (compact sequence, position) order
//   tok_rows [(n_seq + 1) S]   the compact token row of each of them
//   counts   [5]               n_c = n_live + 1, n_c * S, number of live tokens, n_live, live tokens + S
// Behind the live tokens tok_ids / tok_rows carry S more entries (id 0 -> row pad_base + t): the padding rows themselves, so that
// ONE in_proj launch over counts[4] rows produces the live rows and the table the row map points the padding tokens at.
// Everything is ordered and deterministic (no atomics): a single-workgroup scan over the per-sequence counts between two
// wide passes.
#include "common.h"

namespace {

// pass 1: one wave per sequence -> number of live (non-zero) tokens
__device__ __forceinline__ void count_seq(const int* __restrict__ ids, int s, int S, int* __restrict__ live_cnt) {
    const int lane = threadIdx.x & 63;
    int c = 0;
    for (int t = lane; t < S; t += 64) c += ids[(long)s * S + t] != 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) live_cnt[s] = c;
}

__global__ __launch_bounds__(256) void seq_count_kernel(const int* __restrict__ ids, int n_seq, int S, int* __restrict__ live_cnt) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_seq) return;
    count_seq(ids, s, S, live_cnt);
}

// pass 2: ONE workgroup: ordered exclusive scans over the sequences (live flag -> compact index, live tokens -> row offset)
__global__ __launch_bounds__(1024) void seq_scan_kernel(const int* __restrict__ live_cnt, int n_seq, int S, int* __restrict__ seq_src,
                                                        int* __restrict__ seq_inv, int* __restrict__ tok_off, int* __restrict__ counts) {
    __shared__ int part_seq[1024], part_tok[1024];
    const int tid = threadIdx.x;
    const int per = (n_seq + 1023) / 1024;
    const int lo = tid * per, hi = min(n_seq, lo + per);
    int ns = 0, nt = 0;
    for (int s = lo; s < hi; ++s) {
        const int c = live_cnt[s];
        ns += c > 0;
        nt += c;
    }
    part_seq[tid] = ns;
    part_tok[tid] = nt;
    __syncthreads();
    // Hillis-Steele inclusive scan over the 1024 partials (two arrays)
    for (int o = 1; o < 1024; o <<= 1) {
        int a = 0, b = 0;
        if (tid >= o) { a = part_seq[tid - o]; b = part_tok[tid - o]; }
        __syncthreads();
        part_seq[tid] += a;
        part_tok[tid] += b;
        __syncthreads();
    }
    const int n_live = part_seq[1023], n_tok = part_tok[1023];
    int ps = part_seq[tid] - ns, pt = part_tok[tid] - nt;        // exclusive prefixes of this thread's range
    for (int s = lo; s < hi; ++s) {
        const int c = live_cnt[s];
        if (c > 0) {
            seq_src[ps] = s;
            seq_inv[s] = ps;
            tok_off[ps] = pt;
            ++ps;
            pt += c;
        } else {
            seq_inv[s] = n_live;                                   // the all-padding representative
        }
    }
    for (int i = n_live + 1 + tid; i <= n_seq; i += 1024) seq_src[i] = -1;      // unused compact slots: no source sequence
    if (tid == 0) {
        seq_src[n_live] = -1;
        tok_off[n_live] = n_tok;
        counts[0] = n_live + 1;
        counts[1] = (n_live + 1) * S;
        counts[2] = n_tok;
        counts[3] = n_live;
        counts[4] = n_tok + S;
    }
}

// pass 3: one wave per compact sequence -> ids_c, row_map, and the live tokens' (id, row) appended at the sequence's offset
__device__ __forceinline__ void emit_seq(const int cs, const int* __restrict__ ids, int S, const int* __restrict__ seq_src,
                                         const int* __restrict__ tok_off, const int* __restrict__ counts, int pad_base,
                                         int* __restrict__ ids_c, int* __restrict__ row_map, int* __restrict__ tok_ids,
                                         int* __restrict__ tok_rows) {
    const int lane = threadIdx.x & 63;
    const int n_c = counts[0];
    if (cs >= n_c) return;
    const int src = seq_src[cs];
    int base = tok_off[cs];
    for (int t0 = 0; t0 < S; t0 += 64) {
        const int t = t0 + lane;
        int id = 0;
        if (t < S && src >= 0) id = ids[(long)src * S + t];
        const bool live = id != 0;
        const unsigned long long m = __ballot(live);
        if (t < S) {
            const int row = cs * S + t;
            ids_c[row] = id;
            row_map[row] = live ? row : pad_base + t;
            if (cs == n_c - 1) {                       // the representative: its offset is the end of the live list
                tok_ids[base + t] = 0;
                tok_rows[base + t] = pad_base + t;
            }
            if (live) {
                const int k = base + __popcll(m & ((1ull << lane) - 1ull));
                tok_ids[k] = id;
                tok_rows[k] = row;
            }
        }
        base += __popcll(m);
    }
}

__global__ __launch_bounds__(256) void seq_emit_kernel(const int* __restrict__ ids, int n_seq, int S, const int* __restrict__ seq_src,
                                                       const int* __restrict__ tok_off, const int* __restrict__ counts, int pad_base,
                                                       int* __restrict__ ids_c, int* __restrict__ row_map, int* __restrict__ tok_ids,
                                                       int* __restrict__ tok_rows) {
    emit_seq(blockIdx.x * 4 + (threadIdx.x >> 6), ids, S, seq_src, tok_off, counts, pad_base, ids_c, row_map, tok_ids, tok_rows);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// lime_compact_batch: the two texts of a batch of news (title [n, T], body [n, L]) and the NEWS level in the same three passes.
//
// Behind the token encoders nothing of a news' representation depends on another news (intent layers, intent attention, fuse,
// LIME.project: row-wise in eval mode), so the padding news -- all-zero title and body, category 0 / subCategory 0, freshness 0 /
// lifetime 0 (dataset.py:105-141, corpus.py:476-477) -- gets the same arithmetic in every history slot it fills.  News n REPEATS the
// padding news iff its title is all padding, its body is all padding and its key (category, subCategory, freshness bits, lifetime
// bits) equals the key of the FIRST news whose title and body are both all padding; that first one is the representative.  A news
// that looks padded but carries another key stays live.  The raw float bits are compared (equal bits give equal buckets), so the
// compaction does not wait for a bucketize launch.  Outputs, capacity n + 1, counts in device memory:
//   news_src  [n + 1]   compact news -> original news: the live news in order, then the representative (the first padding news, or -1
//                       when the batch has none; the count is then the number of live news); unused slots -1
//   news_inv  [n]       original news -> compact news
//   title_row / body_row [n + 1]   seq_inv_title[news_src[j]] / seq_inv_body[news_src[j]]: the pooled row of compact news j
//   cat_c, sub_c, fresh_c, life_c [n + 1]   the keys in compact order; unused slots hold 0 (valid ids for a consumer that runs over
//                       the capacity)
//   news_counts [4]     n_news, count_mult * n_news, live news, the representative's original index (-1: none)
// ---------------------------------------------------------------------------------------------------------------------------------
struct SeqSide {
    const int* ids; int S, pad_base;
    int *live_cnt, *seq_src, *tok_off;                           // work
    int *seq_inv, *ids_c, *row_map, *tok_ids, *tok_rows, *counts;
};
struct NewsSide {
    const int *cat, *sub, *fresh, *life;                         // fresh / life: the floats' bits
    int *news_src, *news_inv, *title_row, *body_row, *cat_c, *sub_c, *fresh_c, *life_c, *counts;
    int count_mult;
};

// pass 1: one wave per sequence, titles then bodies
__global__ __launch_bounds__(256) void batch_count_kernel(const SeqSide t, const SeqSide b, int n) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= 2 * n) return;
    if (w < n) count_seq(t.ids, w, t.S, t.live_cnt);
    else count_seq(b.ids, w - n, b.S, b.live_cnt);
}

// what seq_scan_kernel writes for one side, from the scanned partials of this thread's range [lo, hi)
__device__ __forceinline__ void scan_side_write(const SeqSide& d, int n, int lo, int hi, int ps, int pt, int n_live, int n_tok) {
    const int tid = threadIdx.x;
    for (int s = lo; s < hi; ++s) {
        const int c = d.live_cnt[s];
        if (c > 0) {
            d.seq_src[ps] = s;
            d.seq_inv[s] = ps;
            d.tok_off[ps] = pt;
            ++ps;
            pt += c;
        } else {
            d.seq_inv[s] = n_live;
        }
    }
    for (int i = n_live + 1 + tid; i <= n; i += 1024) d.seq_src[i] = -1;
    if (tid == 0) {
        d.seq_src[n_live] = -1;
        d.tok_off[n_live] = n_tok;
        d.counts[0] = n_live + 1;
        d.counts[1] = (n_live + 1) * d.S;
        d.counts[2] = n_tok;
        d.counts[3] = n_live;
        d.counts[4] = n_tok + d.S;
    }
}

// pass 2: ONE workgroup: the ordered scans of seq_scan_kernel for the titles and for the bodies, and the news level
__global__ __launch_bounds__(1024) void batch_scan_kernel(const SeqSide t, const SeqSide b, const NewsSide w, int n) {
    __shared__ int part[5][1024];                 // title sequences / tokens, body sequences / tokens, live news
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int lo = min(n, tid * per), hi = min(n, lo + per);
    // the representative: the first news whose title and body are both all padding (ordered minimum over the threads' ranges)
    int first = 0x7FFFFFFF;
    for (int s = hi - 1; s >= lo; --s)
        if (t.live_cnt[s] == 0 && b.live_cnt[s] == 0) first = s;
    part[0][tid] = first;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) part[0][tid] = min(part[0][tid], part[0][tid + o]);
        __syncthreads();
    }
    first = part[0][0];
    __syncthreads();
    const bool has_pad = first != 0x7FFFFFFF;
    int kc = 0, ks = 0, kf = 0, kl = 0;
    if (has_pad) { kc = w.cat[first]; ks = w.sub[first]; kf = w.fresh[first]; kl = w.life[first]; }
    auto repeats = [&](int s) {
        return has_pad && t.live_cnt[s] == 0 && b.live_cnt[s] == 0 && w.cat[s] == kc && w.sub[s] == ks && w.fresh[s] == kf && w.life[s] == kl;
    };
    int v[5] = {0, 0, 0, 0, 0};
    for (int s = lo; s < hi; ++s) {
        const int ct = t.live_cnt[s], cb = b.live_cnt[s];
        v[0] += ct > 0; v[1] += ct;
        v[2] += cb > 0; v[3] += cb;
        v[4] += !repeats(s);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) part[i][tid] = v[i];
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {          // Hillis-Steele inclusive scan over the 1024 partials (five arrays)
        int a[5] = {0, 0, 0, 0, 0};
        if (tid >= o) {
#pragma unroll
            for (int i = 0; i < 5; ++i) a[i] = part[i][tid - o];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 5; ++i) part[i][tid] += a[i];
        __syncthreads();
    }
    scan_side_write(t, n, lo, hi, part[0][tid] - v[0], part[1][tid] - v[1], part[0][1023], part[1][1023]);
    scan_side_write(b, n, lo, hi, part[2][tid] - v[2], part[3][tid] - v[3], part[2][1023], part[3][1023]);
    const int n_live = part[4][1023];
    int pn = part[4][tid] - v[4];
    for (int s = lo; s < hi; ++s) {
        if (repeats(s)) {
            w.news_inv[s] = n_live;
        } else {
            w.news_src[pn] = s;
            w.news_inv[s] = pn;
            ++pn;
        }
    }
    for (int i = n_live + 1 + tid; i <= n; i += 1024) w.news_src[i] = -1;
    if (tid == 0) {
        const int n_news = n_live + (has_pad ? 1 : 0);
        w.news_src[n_live] = has_pad ? first : -1;
        w.counts[0] = n_news;
        w.counts[1] = w.count_mult * n_news;
        w.counts[2] = n_live;
        w.counts[3] = has_pad ? first : -1;
    }
}

// pass 3: the title lists (one wave per compact sequence), the body lists, then the news lists (one thread per compact news)
__global__ __launch_bounds__(256) void batch_emit_kernel(const SeqSide t, const SeqSide b, const NewsSide w, int n, int seq_blocks) {
    const int blk = blockIdx.x;
    const int wave = threadIdx.x >> 6;
    if (blk < seq_blocks) {
        emit_seq(blk * 4 + wave, t.ids, t.S, t.seq_src, t.tok_off, t.counts, t.pad_base, t.ids_c, t.row_map, t.tok_ids, t.tok_rows);
        return;
    }
    if (blk < 2 * seq_blocks) {
        emit_seq((blk - seq_blocks) * 4 + wave, b.ids, b.S, b.seq_src, b.tok_off, b.counts, b.pad_base, b.ids_c, b.row_map, b.tok_ids, b.tok_rows);
        return;
    }
    const int j = (blk - 2 * seq_blocks) * 256 + threadIdx.x;
    if (j > n) return;
    const int src = j < w.counts[0] ? w.news_src[j] : -1;
    const bool on = src >= 0;
    w.title_row[j] = on ? t.seq_inv[src] : 0;
    w.body_row[j] = on ? b.seq_inv[src] : 0;
    w.cat_c[j] = on ? w.cat[src] : 0;
    w.sub_c[j] = on ? w.sub[src] : 0;
    w.fresh_c[j] = on ? w.fresh[src] : 0;
    w.life_c[j] = on ? w.life[src] : 0;
}

}  // namespace

extern "C" int lime_compact_sequences(const int32_t* ids, int32_t n_seq, int32_t S, int32_t pad_base, int32_t* seq_inv, int32_t* ids_c,
                                      int32_t* row_map, int32_t* tok_ids, int32_t* tok_rows, int32_t* counts, int32_t* work, void* stream) {
    LIME_REQUIRE(ids && seq_inv && ids_c && row_map && tok_ids && tok_rows && counts && work, LIME_ERR_BAD_ARG, "lime_compact_sequences: NULL pointer");
    LIME_REQUIRE(n_seq > 0 && S > 0 && pad_base >= 0, LIME_ERR_BAD_ARG, "lime_compact_sequences: bad dims n_seq=%d S=%d pad_base=%d", n_seq, S, pad_base);
    LIME_REQUIRE((long)(n_seq + 1) * S + S < 0x7FFFFFFFL && (long)pad_base + S < 0x7FFFFFFFL, LIME_ERR_UNSUPPORTED, "lime_compact_sequences: too many rows");
    hipStream_t s = (hipStream_t)stream;
    int* live_cnt = work;                        // [n_seq]
    int* seq_src = work + n_seq;                 // [n_seq + 1]
    int* tok_off = work + 2 * n_seq + 1;         // [n_seq + 1]
    hipLaunchKernelGGL(seq_count_kernel, dim3((n_seq + 3) / 4), dim3(256), 0, s, ids, n_seq, S, live_cnt);
    hipLaunchKernelGGL(seq_scan_kernel, dim3(1), dim3(1024), 0, s, live_cnt, n_seq, S, seq_src, seq_inv, tok_off, counts);
    hipLaunchKernelGGL(seq_emit_kernel, dim3((n_seq + 1 + 3) / 4), dim3(256), 0, s, ids, n_seq, S, seq_src, tok_off, counts, pad_base, ids_c,
                       row_map, tok_ids, tok_rows);
    return lime_check_launch("lime_compact_sequences");
}

// int32 words `work` must hold
extern "C" int64_t lime_compact_sequences_workspace(int32_t n_seq) { return 3L * n_seq + 2; }

extern "C" int lime_compact_batch(const int32_t* ids_t, int32_t T, int32_t pad_base_t, int32_t* seq_inv_t, int32_t* ids_c_t, int32_t* row_map_t,
                                  int32_t* tok_ids_t, int32_t* tok_rows_t, int32_t* counts_t, const int32_t* ids_b, int32_t L, int32_t pad_base_b,
                                  int32_t* seq_inv_b, int32_t* ids_c_b, int32_t* row_map_b, int32_t* tok_ids_b, int32_t* tok_rows_b,
                                  int32_t* counts_b, int32_t n, const int32_t* cat, const int32_t* sub, const float* fresh, const float* life,
                                  int32_t count_mult, int32_t* news_src, int32_t* news_inv, int32_t* title_row, int32_t* body_row,
                                  int32_t* cat_c, int32_t* sub_c, float* fresh_c, float* life_c, int32_t* news_counts, int32_t* work,
                                  void* stream) {
    LIME_REQUIRE(ids_t && seq_inv_t && ids_c_t && row_map_t && tok_ids_t && tok_rows_t && counts_t && ids_b && seq_inv_b && ids_c_b &&
                     row_map_b && tok_ids_b && tok_rows_b && counts_b && work,
                 LIME_ERR_BAD_ARG, "lime_compact_batch: NULL pointer (sequence level)");
    LIME_REQUIRE(cat && sub && fresh && life && news_src && news_inv && title_row && body_row && cat_c && sub_c && fresh_c && life_c && news_counts,
                 LIME_ERR_BAD_ARG, "lime_compact_batch: NULL pointer (news level)");
    LIME_REQUIRE(n > 0 && T > 0 && L > 0 && pad_base_t >= 0 && pad_base_b >= 0 && count_mult >= 1, LIME_ERR_BAD_ARG,
                 "lime_compact_batch: bad dims n=%d T=%d L=%d pad_base=%d/%d count_mult=%d", n, T, L, pad_base_t, pad_base_b, count_mult);
    LIME_REQUIRE((long)(n + 1) * T + T < 0x7FFFFFFFL && (long)pad_base_t + T < 0x7FFFFFFFL && (long)(n + 1) * L + L < 0x7FFFFFFFL &&
                     (long)pad_base_b + L < 0x7FFFFFFFL && (long)count_mult * (n + 1) < 0x7FFFFFFFL,
                 LIME_ERR_UNSUPPORTED, "lime_compact_batch: too many rows");
    hipStream_t s = (hipStream_t)stream;
    int* const work_b = work + 3L * n + 2;
    const SeqSide t = {ids_t, T, pad_base_t, work, work + n, work + 2 * n + 1, seq_inv_t, ids_c_t, row_map_t, tok_ids_t, tok_rows_t, counts_t};
    const SeqSide b = {ids_b, L, pad_base_b, work_b, work_b + n, work_b + 2 * n + 1, seq_inv_b, ids_c_b, row_map_b, tok_ids_b, tok_rows_b, counts_b};
    const NewsSide w = {cat, sub, (const int*)fresh, (const int*)life, news_src, news_inv, title_row, body_row, cat_c, sub_c,
                        (int*)fresh_c, (int*)life_c, news_counts, count_mult};
    const int seq_blocks = (n + 1 + 3) / 4;
    hipLaunchKernelGGL(batch_count_kernel, dim3((unsigned)((2L * n + 3) / 4)), dim3(256), 0, s, t, b, n);
    hipLaunchKernelGGL(batch_scan_kernel, dim3(1), dim3(1024), 0, s, t, b, w, n);
    hipLaunchKernelGGL(batch_emit_kernel, dim3((unsigned)(2 * seq_blocks + (n + 1 + 255) / 256)), dim3(256), 0, s, t, b, w, n, seq_blocks);
    return lime_check_launch("lime_compact_batch");
}

// int32 words `work` must hold: the two sides' lime_compact_sequences workspaces back to back
extern "C" int64_t lime_compact_batch_workspace(int32_t n) { return 2 * (3L * n + 2); }
