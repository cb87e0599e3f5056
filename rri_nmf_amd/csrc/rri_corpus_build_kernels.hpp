// rri_corpus_build_kernels.hpp -- a resident corpus from a list of pairs, and the split of one by entry (DESIGN "A corpus from
// pairs; a split by entry"; the semantics, the rules and the constants are rri_corpus_build.hpp's; the sorting networks, the key
// and the compaction are rri_corpus_kernels.hpp's, the generator and the pieces rri_derive.hpp's).
//
//   k_pairs_check      grid-stride over the pair positions 0 .. n_pairs - 1 and nothing else: the smallest offending position of
//                      each rule leaves by a 64-bit integer minimum.  Nothing else runs before the host has read the verdict.
//   k_pairs_count      a wave per 64 consecutive pairs: a lane whose row differs from the row in front of it heads a run, and the
//   k_pairs_claim      head alone adds the run's length to its row's counter -- one integer atomic per run, not per pair, so a
//                      list grouped by row does not serialise 64 lanes on one address.  The claim hands the run consecutive
//                      slots of its row and writes the pair positions into them; the order of the slots is whatever the
//                      scheduling made it and does not survive the sort.
//   k_pairs_sort_wave  rows of 1 .. CORPUS_WAVE_MAX pairs, a wave each: key (column << 32 | pair position) per lane, the bitonic
//                      network of rri_corpus_kernels.hpp, the run of a column summed by its first lane in the order given.
//   k_pairs_sort_block one workgroup per longer row, the keys in LDS (launched per padded length) or, beyond CORPUS_LDS_MAX, in a
//                      global buffer; every thread sums the runs that begin in its share of the sorted row, sequentially.
//                      Both write the merged row into a staging pair at the row's raw offset, its canonical length, and the
//                      counters (duplicates, zeros, negatives, rows that were not canonical as given, long ones among them) by
//                      integer atomics.  A row was canonical as given iff, sorted, its positions ascend, no column repeats and
//                      no value is 0.  k_corpus_compact writes the final arrays where a row became shorter.
//   k_entries_count    (split) a wave per piece: the held entries of the piece, by word 0 of block 0 of (row, column, seed)
//   k_entries_write    both outputs at the piece's two offsets, in source order, the values copied bit for bit; counts the
//                      negative values of either side
// No floating-point sum crosses a thread and no float atomic exists, so two ingests of one list give the same bytes.
#pragma once

#include "rri_corpus_build.hpp"
#include "rri_corpus_kernels.hpp"
#include "rri_derive_kernels.hpp"

namespace rri {

// words of the ingest's counters beside CORPUS_STAT_*: 0 .. 2 err
enum { PAIRS_STAT_REWRITTEN = 11, PAIRS_STAT_LONG = 12, PAIRS_STAT_SCRATCH = 13 };
enum { ENTRIES_STAT_NEG_OBS = 0, ENTRIES_STAT_NEG_HELD = 1 };

__global__ __launch_bounds__(256) void k_pairs_check(const void* __restrict__ rows, const void* __restrict__ cols, int idt, i64 stride,
                                                     const void* __restrict__ values, int vdt, i64 n_rows, i64 n_cols, i64 n_pairs,
                                                     u64* __restrict__ err) {
    const i64 step = (i64)gridDim.x * 256;
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += step) {
        const i64 r = pairs_index(rows, idt, stride, p), j = pairs_index(cols, idt, stride, p);
        if (r < 0 || r >= n_rows) atomicMin(&err[0], (u64)p);
        if (j < 0 || j >= n_cols) atomicMin(&err[1], (u64)p);
        if (values && !corpus_finite(corpus_val(values, vdt, p))) atomicMin(&err[2], (u64)p);
    }
}

// The run of equal rows that lane `lane` of a wave over the pairs base .. base + 63 stands in: its row (-1 beyond the list), the
// lane that heads it and, for the head, its length.  The list has passed the check; all 64 lanes call
struct PairsRun {
    i64 row;
    int head, len;
    bool is_head;
};
__device__ inline PairsRun pairs_run(const void* __restrict__ rows, int idt, i64 stride, i64 base, i64 n_pairs, int lane) {
    const i64 p = base + lane;
    const bool in = p < n_pairs;
    PairsRun q;
    q.row = in ? pairs_index(rows, idt, stride, p) : -1;
    const i64 before = in && lane > 0 ? pairs_index(rows, idt, stride, p - 1) : -2;
    q.is_head = in && q.row != before;
    const u64 hm = __ballot(q.is_head), im = __ballot(in);
    const u64 upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);             // lanes 0 .. lane
    const u64 mine = hm & upto, rest = hm & ~upto;
    q.head = mine ? 63 - __clzll((long long)mine) : 0;
    q.len = (rest ? __ffsll((long long)rest) - 1 : __popcll(im)) - lane;         // the lanes inside the list are 0 .. popc - 1
    return q;
}

__global__ __launch_bounds__(256) void k_pairs_count(const void* __restrict__ rows, int idt, i64 stride, i64 n_pairs,
                                                     unsigned* __restrict__ cnt) {
    const i64 gid = (i64)blockIdx.x * 256 + threadIdx.x, step = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 base = gid - lane; base < n_pairs; base += step) {        // uniform per wave
        const PairsRun q = pairs_run(rows, idt, stride, base, n_pairs, lane);
        if (q.is_head) atomicAdd(&cnt[q.row], (unsigned)q.len);
    }
}

// fill: zeroed counters, one per row; ptr: the exclusive scan of the counts; slots[ptr[r] .. ptr[r + 1]) gets the positions of row r
__global__ __launch_bounds__(256) void k_pairs_claim(const void* __restrict__ rows, int idt, i64 stride, i64 n_pairs,
                                                     const i64* __restrict__ ptr, unsigned* __restrict__ fill,
                                                     unsigned* __restrict__ slots) {
    const i64 gid = (i64)blockIdx.x * 256 + threadIdx.x, step = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 base = gid - lane; base < n_pairs; base += step) {
        const PairsRun q = pairs_run(rows, idt, stride, base, n_pairs, lane);
        unsigned first = 0;
        if (q.is_head) first = atomicAdd(&fill[q.row], (unsigned)q.len);
        first = (unsigned)__shfl((int)first, q.head);
        if (q.row >= 0) slots[ptr[q.row] + (i64)first + (lane - q.head)] = (unsigned)(base + lane);
    }
}

__global__ __launch_bounds__(256) void k_pairs_sort_wave(const i64* __restrict__ list, i64 n_list, const i64* __restrict__ ptr,
                                                         const unsigned* __restrict__ slots, const void* __restrict__ cols, int idt,
                                                         i64 stride, const void* __restrict__ values, int vdt,
                                                         int* __restrict__ out_idx, double* __restrict__ out_val,
                                                         i64* __restrict__ clen, u64* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const i64 item = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_list) return;                                      // a whole wave
    const i64 r = list[item], lo = ptr[r];
    const int len = (int)(ptr[r + 1] - lo);                          // 1 .. CORPUS_WAVE_MAX
    const bool valid = lane < len;                                   // the real keys stand below the pad
    const unsigned at = valid ? slots[lo + lane] : 0u;
    u64 key = valid ? corpus_key(pairs_index(cols, idt, stride, (i64)at), (i64)at) : CORPUS_KEY_PAD;
    key = corpus_sort_wave_key(key, lane);
    const int col = (int)corpus_key_col(key);
    const unsigned pos = corpus_key_pos(key);
    const double v = valid ? corpus_val(values, vdt, (i64)pos) : 0.0;
    const int before = __shfl(col, lane > 0 ? lane - 1 : 0);
    const unsigned pos_before = (unsigned)__shfl((int)pos, lane > 0 ? lane - 1 : 0);
    const bool head = valid && (lane == 0 || col != before);
    double sum = v;
    for (int s = 1; s < 64; ++s) {                                   // uniform: the entries s places behind, while any run goes on
        const int src = lane + s < 64 ? lane + s : 63;
        const int c2 = __shfl(col, src);
        const double v2 = corpus_shfl(v, src);
        const bool in_run = head && lane + s < len && c2 == col;
        if (!__ballot(in_run)) break;
        if (in_run) sum += v2;
    }
    const bool keep = head && sum != 0.0;
    const u64 hm = __ballot(head), km = __ballot(keep), nm = __ballot(keep && sum < 0.0);
    const u64 odd = __ballot(valid && (v == 0.0 || (lane > 0 && pos < pos_before)));       // a stored zero, or not in the order given
    if (keep) {
        const i64 o = lo + __popcll(km & ((1ull << lane) - 1ull));
        out_idx[o] = col;
        out_val[o] = sum;
    }
    if (lane == 0) {
        const int heads = __popcll(hm), kept = __popcll(km);
        clen[r] = kept;
        if (len > heads) atomicAdd(&stats[CORPUS_STAT_DUP], (u64)(len - heads));
        if (heads > kept) atomicAdd(&stats[CORPUS_STAT_ZERO], (u64)(heads - kept));
        if (nm) atomicAdd(&stats[CORPUS_STAT_NEG], (u64)__popcll(nm));
        if (odd || len > heads) atomicAdd(&stats[PAIRS_STAT_REWRITTEN], 1ull);
    }
}

// One workgroup per listed row.  IN_LDS: the P keys live in dynamic LDS (P is the launch's padded length); otherwise in
// keybuf + keyoff[item], corpus_pad(len) of them
template <bool IN_LDS>
__global__ __launch_bounds__(1024) void k_pairs_sort_block(const i64* __restrict__ list, const i64* __restrict__ keyoff,
                                                           u64* __restrict__ keybuf, i64 P_lds, const i64* __restrict__ ptr,
                                                           const unsigned* __restrict__ slots, const void* __restrict__ cols, int idt,
                                                           i64 stride, const void* __restrict__ values, int vdt,
                                                           int* __restrict__ out_idx, double* __restrict__ out_val,
                                                           i64* __restrict__ clen, u64* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int cnt[1024];
    __shared__ int tot[4];                                           // heads, kept, negatives, not canonical as given
    const int tid = threadIdx.x, nt = blockDim.x;
    const i64 item = blockIdx.x;
    const i64 r = list[item], lo = ptr[r], len = ptr[r + 1] - lo;
    const i64 P = IN_LDS ? P_lds : corpus_pad(len);
    u64* keys = IN_LDS ? reinterpret_cast<u64*>(smem) : keybuf + keyoff[item];
    if (tid < 4) tot[tid] = 0;
    for (i64 i = tid; i < P; i += nt) {
        const unsigned at = i < len ? slots[lo + i] : 0u;
        keys[i] = i < len ? corpus_key(pairs_index(cols, idt, stride, (i64)at), (i64)at) : CORPUS_KEY_PAD;
    }
    __syncthreads();
    corpus_sort_keys(keys, P, tid, nt);
    // every thread takes a contiguous share of the sorted row and the runs that begin in it
    const i64 share = (len + nt - 1) / nt;
    const i64 a0 = (i64)tid * share < len ? (i64)tid * share : len, a1 = a0 + share < len ? a0 + share : len;
    int heads = 0, kept = 0, neg = 0, odd = 0;
    for (int pass = 0; pass < 2; ++pass) {
        i64 o = 0;
        if (pass == 1) {
            cnt[tid] = kept;
            __syncthreads();
            for (int off = 1; off < nt; off <<= 1) {
                const int t = tid >= off ? cnt[tid - off] : 0;
                __syncthreads();
                cnt[tid] += t;
                __syncthreads();
            }
            o = lo + cnt[tid] - kept;
        }
        for (i64 i = a0; i < a1; ++i) {
            const unsigned col = corpus_key_col(keys[i]);
            if (i > 0 && corpus_key_col(keys[i - 1]) == col) continue;        // inside a run: a repeated column, counted by len > heads
            if (pass == 0 && i > 0 && corpus_key_pos(keys[i]) < corpus_key_pos(keys[i - 1])) odd = 1;
            double s = corpus_val(values, vdt, (i64)corpus_key_pos(keys[i]));
            if (pass == 0 && s == 0.0) odd = 1;
            for (i64 e = i + 1; e < len && corpus_key_col(keys[e]) == col; ++e) s += corpus_val(values, vdt, (i64)corpus_key_pos(keys[e]));
            if (pass == 0) {
                heads += 1;
                kept += s != 0.0;
                neg += s < 0.0;
            } else if (s != 0.0) {
                out_idx[o] = (int)col;
                out_val[o] = s;
                ++o;
            }
        }
    }
    if (heads) atomicAdd(&tot[0], heads);
    if (kept) atomicAdd(&tot[1], kept);
    if (neg) atomicAdd(&tot[2], neg);
    if (odd) atomicOr(&tot[3], 1);
    __syncthreads();
    if (tid == 0) {
        clen[r] = tot[1];
        if (len > tot[0]) atomicAdd(&stats[CORPUS_STAT_DUP], (u64)(len - tot[0]));
        if (tot[0] > tot[1]) atomicAdd(&stats[CORPUS_STAT_ZERO], (u64)(tot[0] - tot[1]));
        if (tot[2]) atomicAdd(&stats[CORPUS_STAT_NEG], (u64)tot[2]);
        if (tot[3] || len > tot[0]) {
            atomicAdd(&stats[PAIRS_STAT_REWRITTEN], 1ull);
            if (!IN_LDS) atomicAdd(&stats[PAIRS_STAT_LONG], 1ull);
        }
    }
}

// ---- the split by entry -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_entries_count(const i64* __restrict__ piece_row, const i64* __restrict__ piece_src,
                                                       const int* __restrict__ piece_len, i64 n_pieces, const int* __restrict__ src_idx,
                                                       unsigned thr, u64 seed, int* __restrict__ piece_nh) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 pc = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); pc < n_pieces; pc += nwaves) {
        const i64 r = piece_row[pc], src = piece_src[pc];
        const int len = piece_len[pc];
        int nh = 0;
        for (int s = 0; s < len; s += 64) {
            const int e = s + lane;
            const bool held = e < len && split_entry_held(r, src_idx[src + (e < len ? e : 0)], thr, seed);
            nh += __popcll(__ballot(held));
        }
        if (lane == 0) piece_nh[pc] = nh;
    }
}

__global__ __launch_bounds__(256) void k_entries_write(const i64* __restrict__ piece_row, const i64* __restrict__ piece_src,
                                                       const int* __restrict__ piece_len, const i64* __restrict__ piece_oh,
                                                       const i64* __restrict__ piece_oo, i64 n_pieces, const int* __restrict__ src_idx,
                                                       const double* __restrict__ src_val, unsigned thr, u64 seed,
                                                       int* __restrict__ h_idx, double* __restrict__ h_val, int* __restrict__ o_idx,
                                                       double* __restrict__ o_val, u64* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 pc = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); pc < n_pieces; pc += nwaves) {
        const i64 r = piece_row[pc], src = piece_src[pc];
        const int len = piece_len[pc];
        i64 oh = piece_oh[pc], oo = piece_oo[pc];
        for (int s = 0; s < len; s += 64) {
            const int e = s + lane;
            const bool in = e < len;
            const int col = in ? src_idx[src + e] : 0;
            const double v = in ? src_val[src + e] : 0.0;
            const bool held = in && split_entry_held(r, col, thr, seed), obs = in && !held;
            const u64 mh = __ballot(held), mo = __ballot(obs);
            if (held) {
                const i64 at = oh + __popcll(mh & derive_below(lane));
                h_idx[at] = col;
                h_val[at] = v;
            }
            if (obs) {
                const i64 at = oo + __popcll(mo & derive_below(lane));
                o_idx[at] = col;
                o_val[at] = v;
            }
            oh += __popcll(mh);
            oo += __popcll(mo);
            corpus_count(&stats[ENTRIES_STAT_NEG_HELD], held && v < 0.0);
            corpus_count(&stats[ENTRIES_STAT_NEG_OBS], obs && v < 0.0);
        }
    }
}

}  // namespace rri
