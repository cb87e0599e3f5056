// rri_derive_kernels.hpp -- corpora derived from a resident canonical corpus (DESIGN "Corpora derived on the device"; the
// semantics, the generator, the pieces and the limits are rri_derive.hpp's).
//
// Every kernel but the two grid-stride ones works by PIECES: up to DERIVE_PIECE consecutive source entries of one row, cut by the
// host from its copy of indptr, a wave per piece (four per workgroup, wave-stride over the list), so a row of a million entries is
// a thousand waves' work and no launch waits for one wave.  A wave walks its piece 64 entries at a time, in order; what a stride
// keeps is placed by a ballot, a popcount of the lanes below and the piece's running offset, so the output is in source order and
// the same on every run.  No floating-point sum is formed anywhere: values are copied, or are integers.
//   k_derive_count          (select with keep) the kept entries of every piece, through the column map (new column, or -1)
//   k_derive_write          (select) the piece's kept entries at the piece's output offset; counts the negative values kept
//   k_derive_column_counts  grid-stride over the entries: a 64-bit integer atomic per entry on df[column]
//   k_split_check           grid-stride over the values: the smallest offending position of each rule by an integer minimum
//   k_split_held            pass A: the held part of every entry into an int32 array, and per piece the entries whose held part
//                           and whose remainder are above 0.  A count up to SPLIT_LANE_MAX is thinned by its lane; a larger one by
//                           the whole wave, lane l taking the Philox blocks l, l + 64, ..., summed as integers over the lanes
//   k_split_write           pass B: both outputs at the piece's two offsets
// Loop bounds and the piece are uniform over a wave, so every ballot and shuffle runs with all 64 lanes.
#pragma once

#include "rri_corpus_kernels.hpp"
#include "rri_derive.hpp"

namespace rri {

enum { DERIVE_STAT_NEG = 4, DERIVE_STAT_WORDS = 8 };    // words of a derivation's counters; 0 .. 2: the split's err

__device__ inline u64 derive_below(int lane) { return (1ull << lane) - 1ull; }

__global__ __launch_bounds__(256) void k_derive_count(const i64* __restrict__ piece_src, const int* __restrict__ piece_len, i64 n_pieces,
                                                      const int* __restrict__ src_idx, const int* __restrict__ colmap,
                                                      int* __restrict__ piece_cnt) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 pc = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); pc < n_pieces; pc += nwaves) {
        const i64 src = piece_src[pc];
        const int len = piece_len[pc];
        int cnt = 0;
        for (int s = 0; s < len; s += 64) {
            const int e = s + lane;
            const bool kept = e < len && colmap[src_idx[src + e]] >= 0;
            cnt += __popcll(__ballot(kept));
        }
        if (lane == 0) piece_cnt[pc] = cnt;
    }
}

// colmap NULL: every column is kept under its own number
__global__ __launch_bounds__(256) void k_derive_write(const i64* __restrict__ piece_src, const int* __restrict__ piece_len,
                                                      const i64* __restrict__ piece_out, i64 n_pieces, const int* __restrict__ src_idx,
                                                      const double* __restrict__ src_val, const int* __restrict__ colmap,
                                                      int* __restrict__ out_idx, double* __restrict__ out_val, u64* __restrict__ negatives) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 pc = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); pc < n_pieces; pc += nwaves) {
        const i64 src = piece_src[pc];
        const int len = piece_len[pc];
        i64 o = piece_out[pc];
        for (int s = 0; s < len; s += 64) {
            const int e = s + lane;
            const bool in = e < len;
            const int col = in ? src_idx[src + e] : 0;
            const double v = in ? src_val[src + e] : 0.0;
            const int ncol = !in ? -1 : colmap ? colmap[col] : col;
            const bool kept = ncol >= 0;
            const u64 m = __ballot(kept);
            if (kept) {
                const i64 at = o + __popcll(m & derive_below(lane));
                out_idx[at] = ncol;
                out_val[at] = v;
            }
            o += __popcll(m);
            corpus_count(negatives, kept && v < 0.0);
        }
    }
}

__global__ __launch_bounds__(256) void k_derive_column_counts(const int* __restrict__ idx, i64 nnz, u64* __restrict__ df) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < nnz; p += stride) atomicAdd(&df[idx[p]], 1ull);
}

__global__ __launch_bounds__(256) void k_split_check(const double* __restrict__ val, i64 nnz, u64* __restrict__ err) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < nnz; p += stride) {
        const double v = val[p];
        if (v < 0.0) atomicMin(&err[0], (u64)p);
        if (v != floor(v)) atomicMin(&err[1], (u64)p);
        if (v > (double)SPLIT_COUNT_MAX) atomicMin(&err[2], (u64)p);
    }
}

__device__ inline int derive_wave_sum(int v) {
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// the values have passed k_split_check: whole numbers in [1, SPLIT_COUNT_MAX]
__global__ __launch_bounds__(256) void k_split_held(const i64* __restrict__ piece_row, const i64* __restrict__ piece_src,
                                                    const int* __restrict__ piece_len, i64 n_pieces, const int* __restrict__ src_idx,
                                                    const double* __restrict__ src_val, unsigned thr, u64 seed, int* __restrict__ held,
                                                    int* __restrict__ piece_nh, int* __restrict__ piece_no) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 pc = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); pc < n_pieces; pc += nwaves) {
        const i64 r = piece_row[pc], src = piece_src[pc];
        const int len = piece_len[pc];
        int nh = 0, no = 0;
        for (int s = 0; s < len; s += 64) {
            const int e = s + lane;
            const bool in = e < len;
            const int col = in ? src_idx[src + e] : 0;
            const int count = in ? (int)src_val[src + e] : 0;
            const bool big = count > SPLIT_LANE_MAX;
            int h = big ? 0 : (int)split_held(r, col, count, thr, seed);
            for (u64 bm = __ballot(big); bm; bm &= bm - 1) {          // uniform: one large entry at a time, its blocks over the lanes
                const int owner = __ffsll((long long)bm) - 1;
                const int col2 = __shfl(col, owner), count2 = __shfl(count, owner);
                const int total = derive_wave_sum((int)split_held_blocks(r, col2, count2, thr, seed, lane, 64));
                if (lane == owner) h = total;
            }
            if (in) held[src + e] = h;
            nh += __popcll(__ballot(h > 0));
            no += __popcll(__ballot(count - h > 0));
        }
        if (lane == 0) {
            piece_nh[pc] = nh;
            piece_no[pc] = no;
        }
    }
}

__global__ __launch_bounds__(256) void k_split_write(const i64* __restrict__ piece_src, const int* __restrict__ piece_len,
                                                     const i64* __restrict__ piece_oh, const i64* __restrict__ piece_oo, i64 n_pieces,
                                                     const int* __restrict__ src_idx, const double* __restrict__ src_val,
                                                     const int* __restrict__ held, int* __restrict__ h_idx, double* __restrict__ h_val,
                                                     int* __restrict__ o_idx, double* __restrict__ o_val) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 pc = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); pc < n_pieces; pc += nwaves) {
        const i64 src = piece_src[pc];
        const int len = piece_len[pc];
        i64 oh = piece_oh[pc], oo = piece_oo[pc];
        for (int s = 0; s < len; s += 64) {
            const int e = s + lane;
            const bool in = e < len;
            const int col = in ? src_idx[src + e] : 0;
            const int count = in ? (int)src_val[src + e] : 0;
            const int h = in ? held[src + e] : 0;
            const u64 mh = __ballot(h > 0), mo = __ballot(count - h > 0);
            if (h > 0) {
                const i64 at = oh + __popcll(mh & derive_below(lane));
                h_idx[at] = col;
                h_val[at] = (double)h;
            }
            if (count - h > 0) {
                const i64 at = oo + __popcll(mo & derive_below(lane));
                o_idx[at] = col;
                o_val[at] = (double)(count - h);
            }
            oh += __popcll(mh);
            oo += __popcll(mo);
        }
    }
}

}  // namespace rri
