// rri_corpus_rank_kernels.hpp -- the device work that ranking against resident corpora adds to k_topn_rows and k_rank_entries
// (DESIGN "Rank and recommend against resident corpora"; the classification, the row terms, the lane rule and the trees are
// rri_corpus_rank.hpp's).
//
// The two scoring kernels read an exclusion corpus where it lies through their `erow` argument; nothing of it is copied.  Here:
//   k_crank_count           pieces per row of the targets corpus, one lane per row; slot n_rows takes 0
//   k_crank_scan_part/top/apply   the exclusive scan of those n_rows + 1 counts in place, tiles of CRANK_SCAN_TILE: the sums of the
//                           tiles, their exclusive scan by one workgroup, the scan inside each tile.  Slot n_rows ends up holding
//                           the number of pieces, the one int64 the host reads back to size the scoring launch
//   k_crank_cut             one lane per row writes the row's pieces (crank_piece) at its offset
//   k_crank_rows            one wave per row of the targets corpus, lanes striding the row's entries in corpus order.  Counts, the
//                           smallest rank and the sum of ranks are integers, added by the xor butterfly; the lane's hits add
//                           table[rank] in ascending order and the butterfly at 32 .. 1 is crank_tree64 in lane 0, which forms the
//                           row's terms (crank_row_terms) and stores them with plain stores.  No LDS, no barrier
//   k_crank_sum             one level of the totals (crank_sum_level): workgroup b adds the items b R .. (b + 1) R - 1 (R =
//                           CRANK_SUM_ROWS; `stride` 256) -- or, as the single workgroup of the second level, all block sums
//                           (`stride` 256, `per` = the number of items) -- slot t taking t, t + 256, ... in ascending order; the
//                           waves by the butterfly, the four wave sums through LDS as (w0 + w1) + (w2 + w3).  Plain stores, no atomics
#pragma once

#include "rri_corpus_rank.hpp"
#include "rri_rank_kernels.hpp"

namespace rri {

constexpr int CRANK_SCAN_PER = 4;                            // counts per thread of a scan tile
constexpr int CRANK_SCAN_TILE = 256 * CRANK_SCAN_PER;

__global__ __launch_bounds__(256) void k_crank_count(const i64* __restrict__ indptr, i64 n_rows, i64* __restrict__ cnt) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r > n_rows) return;
    cnt[r] = r < n_rows ? crank_row_pieces(indptr[r + 1] - indptr[r]) : 0;
}

// the inclusive scan of one value per thread of a 256-thread workgroup, through buf[256]
__device__ inline i64 crank_scan256(i64 v, i64* buf) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const i64 t = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += t;
        __syncthreads();
    }
    return buf[tid];
}

__global__ __launch_bounds__(256) void k_crank_scan_part(const i64* __restrict__ cnt, i64 len, i64* __restrict__ part) {
    __shared__ i64 buf[256];
    const i64 base = (i64)blockIdx.x * CRANK_SCAN_TILE + (i64)threadIdx.x * CRANK_SCAN_PER;
    i64 s = 0;
    for (int e = 0; e < CRANK_SCAN_PER; ++e)
        if (base + e < len) s += cnt[base + e];
    const i64 incl = crank_scan256(s, buf);
    if (threadIdx.x == 255) part[blockIdx.x] = incl;
}
// one workgroup: part <- its exclusive scan, 256 tiles at a time with the carry of those before
__global__ __launch_bounds__(256) void k_crank_scan_top(i64* __restrict__ part, i64 tiles) {
    __shared__ i64 buf[256];
    __shared__ i64 carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (i64 base = 0; base < tiles; base += 256) {
        const i64 mine = base + tid < tiles ? part[base + tid] : 0;
        const i64 incl = crank_scan256(mine, buf);
        if (base + tid < tiles) part[base + tid] = carry + incl - mine;
        __syncthreads();
        if (tid == 255) carry += incl;
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_crank_scan_apply(i64* __restrict__ cnt, i64 len, const i64* __restrict__ part) {
    __shared__ i64 buf[256];
    const i64 base = (i64)blockIdx.x * CRANK_SCAN_TILE + (i64)threadIdx.x * CRANK_SCAN_PER;
    i64 v[CRANK_SCAN_PER];
    i64 s = 0;
    for (int e = 0; e < CRANK_SCAN_PER; ++e) {
        v[e] = base + e < len ? cnt[base + e] : 0;
        s += v[e];
    }
    i64 before = part[blockIdx.x] + crank_scan256(s, buf) - s;
    for (int e = 0; e < CRANK_SCAN_PER; ++e) {
        if (base + e < len) cnt[base + e] = before;
        before += v[e];
    }
}

// first: the exclusive scan of the counts (n_rows + 1 entries); pieces: first[n_rows] of them
__global__ __launch_bounds__(256) void k_crank_cut(const i64* __restrict__ indptr, i64 n_rows, const i64* __restrict__ first,
                                                   RankPiece* __restrict__ pieces) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rows) return;
    const i64 at = first[r], c = first[r + 1] - at;
    for (i64 p = 0; p < c; ++p) pieces[at + p] = crank_piece(reinterpret_cast<const int64_t*>(indptr), r, p);
}

__device__ inline i64 crank_butterfly_add(i64 v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_crank_rows(const i64* __restrict__ indptr, const double* __restrict__ values, i64 n_rows,
                                                    const int* __restrict__ rank, const int* __restrict__ eligible, i64 n_items,
                                                    double relevant_from, const double* __restrict__ table,
                                                    const double* __restrict__ ideal, double* __restrict__ terms) {
    const int lane = threadIdx.x & 63;
    const i64 nwaves = (i64)gridDim.x * 4;
    for (i64 r = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); r < n_rows; r += nwaves) {      // uniform per wave
        const i64 e0 = indptr[r], e1 = indptr[r + 1];
        i64 T = 0, P = 0, hits = 0, S = 0, rmin = INT64_MAX;
        double dcg = 0.0;
        for (i64 e = e0 + lane; e < e1; e += 64) {
            if (!crank_relevant(values[e], relevant_from)) continue;
            ++T;
            const int rk = rank[e];
            if (!crank_eligible(rk)) continue;
            ++P;
            S += rk;
            rmin = rk < rmin ? rk : rmin;
            if (crank_hit(rk, n_items)) {
                ++hits;
                dcg = dcg + table[rk];
            }
        }
        T = crank_butterfly_add(T);
        P = crank_butterfly_add(P);
        hits = crank_butterfly_add(hits);
        S = crank_butterfly_add(S);
        for (int off = 32; off >= 1; off >>= 1) {
            const i64 o = __shfl_xor(rmin, off, 64);
            rmin = o < rmin ? o : rmin;
            dcg = dcg + __shfl_xor(dcg, off, 64);
        }
        if (lane == 0) {
            const CrankRow w{T, P, hits, P < 1 ? 0 : rmin, S, (i64)eligible[r]};
            double t[CRANK_TERMS];
            crank_row_terms(w, dcg, n_items, ideal, t);
            for (int i = 0; i < CRANK_TERMS; ++i) terms[r * CRANK_TERMS + i] = t[i];
        }
    }
}

// out[b * CRANK_TERMS + i] = the sum of term i over the items [b per, min((b + 1) per, items)), slot t taking t, t + 256, ...
__global__ __launch_bounds__(256) void k_crank_sum(const double* __restrict__ in, i64 items, i64 per, double* __restrict__ out) {
    __shared__ double ws[4][CRANK_TERMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 lo = (i64)blockIdx.x * per, hi = lo + per < items ? lo + per : items;
    double s[CRANK_TERMS];
#pragma unroll
    for (int i = 0; i < CRANK_TERMS; ++i) s[i] = 0.0;
    for (i64 r = lo + tid; r < hi; r += 256) {
#pragma unroll
        for (int i = 0; i < CRANK_TERMS; ++i) s[i] = s[i] + in[r * CRANK_TERMS + i];
    }
#pragma unroll
    for (int i = 0; i < CRANK_TERMS; ++i) {
        for (int off = 32; off >= 1; off >>= 1) s[i] = s[i] + __shfl_xor(s[i], off, 64);
        if (lane == 0) ws[wave][i] = s[i];
    }
    __syncthreads();
    if (tid < CRANK_TERMS) out[(i64)blockIdx.x * CRANK_TERMS + tid] = (ws[0][tid] + ws[1][tid]) + (ws[2][tid] + ws[3][tid]);
}

}  // namespace rri
