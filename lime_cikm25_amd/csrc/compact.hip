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

// what seq_scan_kernel writes for sequence s of one side (c live tokens) at this thread's running prefixes ps / pt ...
__device__ __forceinline__ void scan_side_put(const SeqSide& d, int s, int c, int& ps, int& pt, int n_live) {
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
// ... and behind the live sequences: the unused slots, the end of the token list, the counts
__device__ __forceinline__ void scan_side_tail(const SeqSide& d, int n, int n_live, int n_tok) {
    const int tid = threadIdx.x;
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

// everything the scan reads of one news: the live tokens of its title and body, and its key
struct NewsRow { int ct, cb, cat, sub, fresh, life; };
__device__ __forceinline__ NewsRow load_row(const SeqSide& t, const SeqSide& b, const NewsSide& w, int s) {
    return {t.live_cnt[s], b.live_cnt[s], w.cat[s], w.sub[s], w.fresh[s], w.life[s]};
}

// pass 2: ONE workgroup: the ordered scans of seq_scan_kernel for the titles and for the bodies, and the news level.  A thread owns
// per = ceil(n / 1024) consecutive news.  One workgroup hides no latency, so the kernel's time is its chain of dependent round trips
// to memory, and there are two: PER > 0 (per <= PER, picked by the host) loads the rows of the thread's range into registers at the
// start -- 6 PER independent loads, no branch between them -- and the key of the representative once it is known; every other step
// reads registers.  PER == 0 (any n) reads a row's six words afresh in each of its three passes, still without a branch between the
// loads.  The five scans (title sequences / tokens, body sequences / tokens, live news) go together through ONE wave-level scan
// (shuffles, no LDS) and one pass over the 16 wave totals, the representative through a wave-level minimum: two workgroup barriers.
template <int PER>
__global__ __launch_bounds__(1024) void batch_scan_kernel(const SeqSide t, const SeqSide b, const NewsSide w, int n) {
    __shared__ int wave_first[16];
    __shared__ int wave_tot[5][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (n + 1023) / 1024;
    const int lo = min(n, tid * per), hi = min(n, lo + per);
    NewsRow reg[PER > 0 ? PER : 1];
    if (PER > 0) {
#pragma unroll
        for (int i = 0; i < PER; ++i) reg[i] = load_row(t, b, w, min(lo + i, n - 1));       // (clamped: a valid address whatever the range)
    }
    // f(s, row of s) for the news of the thread's range, in order: PER > 0 unrolls over the registers, PER == 0 loops and loads
    auto each_own = [&](auto&& f) {
        if constexpr (PER > 0) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if (lo + i < hi) f(lo + i, reg[i]);
            }
        } else {
            for (int s = lo; s < hi; ++s) f(s, load_row(t, b, w, s));
        }
    };
    // the representative: the first news whose title and body are both all padding (ordered minimum over the threads' ranges);
    // the four scans that do not depend on it are summed on the way
    int first = 0x7FFFFFFF;
    int v[5] = {0, 0, 0, 0, 0};
    each_own([&](int s, const NewsRow& r) {
        v[0] += r.ct > 0; v[1] += r.ct;
        v[2] += r.cb > 0; v[3] += r.cb;
        if (r.ct == 0 && r.cb == 0) first = min(first, s);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
    if (lane == 0) wave_first[wave] = first;
    __syncthreads();
    first = wave_first[lane & 15];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o));
    const bool has_pad = first != 0x7FFFFFFF;
    NewsRow key = {0, 0, 0, 0, 0, 0};
    if (has_pad) key = load_row(t, b, w, first);
    auto repeats = [&](const NewsRow& r) {        // (bitwise: one test, no branch per member)
        return has_pad & (r.ct == 0) & (r.cb == 0) & (r.cat == key.cat) & (r.sub == key.sub) & (r.fresh == key.fresh) & (r.life == key.life);
    };
    each_own([&](int, const NewsRow& r) { v[4] += !repeats(r); });
    // inclusive scan of the five partials over the wave's lanes, ...
    int inc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) inc[i] = v[i];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int up = __shfl_up(inc[i], o);
            if (lane >= o) inc[i] += up;
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < 5; ++i) wave_tot[i][wave] = inc[i];
    }
    __syncthreads();
    // ... then every wave scans the 16 wave totals itself (lanes 0 .. 15) and takes its own offset and the grand total from them
    int ex[5], tot[5];                            // exclusive prefix of this thread's range, total over the workgroup
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        int x = lane < 16 ? wave_tot[i][lane] : 0;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const int up = __shfl_up(x, o);
            if (lane >= o) x += up;
        }
        const int before = __shfl(x, wave > 0 ? wave - 1 : 0);
        tot[i] = __shfl(x, 15);
        ex[i] = (wave > 0 ? before : 0) + inc[i] - v[i];
    }
    const int n_live = tot[4];
    each_own([&](int s, const NewsRow& r) {
        scan_side_put(t, s, r.ct, ex[0], ex[1], tot[0]);
        scan_side_put(b, s, r.cb, ex[2], ex[3], tot[2]);
        if (repeats(r)) {
            w.news_inv[s] = n_live;
        } else {
            w.news_src[ex[4]] = s;
            w.news_inv[s] = ex[4];
            ++ex[4];
        }
    });
    scan_side_tail(t, n, tot[0], tot[1]);
    scan_side_tail(b, n, tot[2], tot[3]);
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
    if ((n + 1023) / 1024 <= 2) hipLaunchKernelGGL(batch_scan_kernel<2>, dim3(1), dim3(1024), 0, s, t, b, w, n);     // (the thread's rows in registers)
    else hipLaunchKernelGGL(batch_scan_kernel<0>, dim3(1), dim3(1024), 0, s, t, b, w, n);
    hipLaunchKernelGGL(batch_emit_kernel, dim3((unsigned)(2 * seq_blocks + (n + 1 + 255) / 256)), dim3(256), 0, s, t, b, w, n, seq_blocks);
    return lime_check_launch("lime_compact_batch");
}

// int32 words `work` must hold: the two sides' lime_compact_sequences workspaces back to back
extern "C" int64_t lime_compact_batch_workspace(int32_t n) { return 2 * (3L * n + 2); }
