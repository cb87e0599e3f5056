// rri_rowsplit_kernels.hpp -- the split of a resident corpus by row (DESIGN "A split by row"; the key, the quota, the bound and the
// constants are rri_rowsplit.hpp's; the pieces and the ballot-ranked writes are rri_derive_kernels.hpp's).
//
// The host knows every row's quota h from its copy of indptr.  A row with h = 0 or h = L has its bound (0, all ones) written by the
// host; the rows with 0 < h < L are listed by class and their bound K* + 1, K* the h-th smallest key of the row, is found here:
//   k_rowsplit_select_wave   rows of up to ROWSPLIT_WAVE_MAX entries, a wave each: a key per lane (a lane beyond the row holds all
//                            ones, above every key), the rank of a key is the number of smaller keys among the 64 lanes -- the keys
//                            of a row are distinct, so the ranks are a permutation -- and the lane of rank h - 1 writes the bound.
//   k_rowsplit_select_block  any longer row, a workgroup each: a radix select from the most significant digit, ROWSPLIT_PASSES passes
//                            of ROWSPLIT_DIGIT_BITS bits.  In a pass the threads stride over the row, recompute the key, and count
//                            the keys that carry the prefix found so far into a histogram of ROWSPLIT_BINS bins in LDS; one wave
//                            scans the bins, picks the bin that holds the wanted rank, and narrows the prefix and the rank.  The LDS
//                            atomics are integer adds, so the histogram and the bound are the same on every run.  Keys are not
//                            cached: one class serves every length, at eight reads of the row's columns and eight Philox blocks per
//                            entry.  A workgroup waits for nothing outside itself: a very long row is slow, never stuck.
//   k_rowsplit_count         a wave per piece: the entries of the piece with K < bound[row]
//   k_rowsplit_write         both outputs at the piece's two offsets, in source order, the values copied bit for bit; counts the
//                            negative values of either side.  A piece of a row whose bound is 0 or all ones computes no key.
// Loop bounds, the piece, the row and its bound are uniform over a wave, so every ballot and shuffle runs with all 64 lanes.
#pragma once

#include "rri_corpus_build_kernels.hpp"
#include "rri_rowsplit.hpp"

namespace rri {

__device__ inline u64 rowsplit_shfl(u64 v, int src) {
    const int lo = __shfl((int)(unsigned)(v & 0xffffffffull), src), hi = __shfl((int)(unsigned)(v >> 32), src);
    return ((u64)(unsigned)hi << 32) | (u64)(unsigned)lo;
}
// whether entry (r, col) lies under the bound of its row; the two known bounds need no key (uniform over the wave)
__device__ inline bool rowsplit_held(i64 r, int col, u64 bound, u64 seed) {
    if (bound == ROWSPLIT_BOUND_ALL) return true;
    if (bound == ROWSPLIT_BOUND_NONE) return false;
    return rowsplit_key(r, col, seed) < bound;
}

// list[0 .. n_list): rows of 2 .. ROWSPLIT_WAVE_MAX entries; quota[item] in [1, length)
__global__ __launch_bounds__(256) void k_rowsplit_select_wave(const i64* __restrict__ list, const i64* __restrict__ quota, i64 n_list,
                                                              const i64* __restrict__ ptr, const int* __restrict__ src_idx, u64 seed,
                                                              u64* __restrict__ bound) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 item = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); item < n_list; item += nwaves) {          // uniform per wave
        const i64 r = list[item], lo = ptr[r];
        const int len = (int)(ptr[r + 1] - lo), h = (int)quota[item];
        const bool valid = lane < len;
        const u64 key = valid ? rowsplit_key(r, src_idx[lo + lane], seed) : ROWSPLIT_BOUND_ALL;
        int rank = 0;
        for (int s = 0; s < len; ++s) rank += (int)(rowsplit_shfl(key, s) < key);
        if (valid && rank == h - 1) bound[r] = key + 1;
    }
}

// list[0 .. n_list): rows of more than ROWSPLIT_WAVE_MAX entries; quota[item] in [1, length)
__global__ __launch_bounds__(ROWSPLIT_BLOCK_THREADS) void k_rowsplit_select_block(const i64* __restrict__ list, const i64* __restrict__ quota,
                                                                                  i64 n_list, const i64* __restrict__ ptr,
                                                                                  const int* __restrict__ src_idx, u64 seed,
                                                                                  u64* __restrict__ bound) {
    __shared__ unsigned hist[ROWSPLIT_BINS];
    __shared__ u64 s_prefix;
    __shared__ i64 s_want;
    const int tid = threadIdx.x, lane = tid & 63;
    for (i64 item = blockIdx.x; item < n_list; item += gridDim.x) {          // uniform per workgroup
        const i64 r = list[item], lo = ptr[r], len = ptr[r + 1] - lo;
        u64 prefix = 0;                     // the digits found so far, in place; the digits below are 0
        i64 want = quota[item];             // the rank looked for among the keys that carry the prefix, 1-based
        for (int pass = 0; pass < ROWSPLIT_PASSES; ++pass) {
            const int shift = 64 - ROWSPLIT_DIGIT_BITS * (pass + 1);
            const u64 above = pass ? ~0ull << (shift + ROWSPLIT_DIGIT_BITS) : 0ull;          // the bits of the digits found so far
            hist[tid] = 0u;
            __syncthreads();
            for (i64 e = tid; e < len; e += ROWSPLIT_BLOCK_THREADS) {
                const u64 key = rowsplit_key(r, src_idx[lo + e], seed);
                if ((key & above) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & (ROWSPLIT_BINS - 1)], 1u);
            }
            __syncthreads();
            if (tid < 64) {                 // one wave: lane l has the bins 4 l .. 4 l + 3 and the keys in the bins below them
                i64 c[4], mine = 0;
                for (int b = 0; b < 4; ++b) {
                    c[b] = (i64)hist[4 * lane + b];
                    mine += c[b];
                }
                i64 upto = mine;            // inclusive scan over the lanes
                for (int off = 1; off < 64; off <<= 1) {
                    const i64 t = (i64)rowsplit_shfl((u64)upto, lane >= off ? lane - off : lane);
                    if (lane >= off) upto += t;
                }
                i64 below = upto - mine;
                for (int b = 0; b < 4; ++b) {          // at least `want` keys carry the prefix: exactly one bin holds that rank
                    if (below < want && want <= below + c[b]) {
                        s_prefix = prefix | ((u64)(4 * lane + b) << shift);
                        s_want = want - below;
                    }
                    below += c[b];
                }
            }
            __syncthreads();
            prefix = s_prefix;
            want = s_want;
        }
        if (tid == 0) bound[r] = prefix + 1;          // all 64 bits are found: the key itself
        __syncthreads();                              // (s_prefix is read before the next row's first pass can write it)
    }
}

__global__ __launch_bounds__(256) void k_rowsplit_count(const i64* __restrict__ piece_row, const i64* __restrict__ piece_src,
                                                        const int* __restrict__ piece_len, i64 n_pieces, const int* __restrict__ src_idx,
                                                        const u64* __restrict__ bound, u64 seed, int* __restrict__ piece_nh) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 pc = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); pc < n_pieces; pc += nwaves) {
        const i64 r = piece_row[pc], src = piece_src[pc];
        const int len = piece_len[pc];
        const u64 bnd = bound[r];
        int nh = 0;
        for (int s = 0; s < len; s += 64) {
            const int e = s + lane;
            const bool held = e < len && rowsplit_held(r, src_idx[src + (e < len ? e : 0)], bnd, seed);
            nh += __popcll(__ballot(held));
        }
        if (lane == 0) piece_nh[pc] = nh;
    }
}

__global__ __launch_bounds__(256) void k_rowsplit_write(const i64* __restrict__ piece_row, const i64* __restrict__ piece_src,
                                                        const int* __restrict__ piece_len, const i64* __restrict__ piece_oh,
                                                        const i64* __restrict__ piece_oo, i64 n_pieces, const int* __restrict__ src_idx,
                                                        const double* __restrict__ src_val, const u64* __restrict__ bound, u64 seed,
                                                        int* __restrict__ h_idx, double* __restrict__ h_val, int* __restrict__ o_idx,
                                                        double* __restrict__ o_val, u64* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 pc = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); pc < n_pieces; pc += nwaves) {
        const i64 r = piece_row[pc], src = piece_src[pc];
        const int len = piece_len[pc];
        const u64 bnd = bound[r];
        i64 oh = piece_oh[pc], oo = piece_oo[pc];
        for (int s = 0; s < len; s += 64) {
            const int e = s + lane;
            const bool in = e < len;
            const int col = in ? src_idx[src + e] : 0;
            const double v = in ? src_val[src + e] : 0.0;
            const bool held = in && rowsplit_held(r, col, bnd, seed), obs = in && !held;
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
