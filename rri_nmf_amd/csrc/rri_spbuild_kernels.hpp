// rri_spbuild_kernels.hpp -- the blocked store of a CSR handle, built on the device from canonical arrays that are there already
// (rri_upload_X_corpus; the steps, the key and the host restatement are rri_spbuild.hpp's, the layout is build_sp_copy's).
//
//   k_spb_count_rows   copy 0: a thread per (row, column block): two bisections of the row, no atomic; the longest row by an
//                      integer maximum
//   k_spb_count_cols   copy 1: a thread per stored entry, its row by bisection of indptr: an integer histogram
//   k_spb_scan_part / k_spb_scan_top / k_spb_scan_apply
//                      the inclusive prefix sum of the counts rounded up to quads, in place, over the flat [nblk][nseg + 1]
//                      array: tile sums, their exclusive scan by one workgroup, the tiles once more
//   k_spb_fill         idx = bw, perm = -1 everywhere: the pads
//   k_spb_claim_rows   copy 0: slot = segptr[b][r] + (p - first entry of the row in block b): the stable order, no atomic
//   k_spb_claim_cols   copy 1: a slot of the segment from an integer counter, the key (p << 32 | offset) into it
//   k_spb_sort_wave    copy 1: segments of up to 64 padded entries, a wave each: the corpus ingest's register network
//   k_spb_sort_block   copy 1: a workgroup per longer segment, its keys in LDS: the corpus ingest's LDS network
// Integer atomics only; the two places whose outcome depends on arrival (the counter of k_spb_claim_cols) are followed by the sort
// by the unique key, so two builds of one matrix leave the same bytes.  Every index is derived from the canonical arrays of a
// corpus, which rri_corpus_create has checked: indptr monotone from 0 to nnz, every column inside [0, d).
#pragma once

#include "rri_corpus_kernels.hpp"
#include "rri_spbuild.hpp"

namespace rri {

constexpr int SPB_SCAN_PER_THREAD = 8, SPB_SCAN_TILE = 256 * SPB_SCAN_PER_THREAD;

// the row of stored position p: the last r with indptr[r] <= p (0 <= p < indptr[n])
__device__ inline i64 spb_row_of(const i64* __restrict__ indptr, i64 n, i64 p) {
    i64 a = 0, b = n;                   // indptr[a] <= p < indptr[b]
    while (b - a > 1) {
        const i64 m = a + ((b - a) >> 1);
        if (indptr[m] <= p) a = m;
        else b = m;
    }
    return a;
}
// the first position of [lo, hi) whose column is not below `bound` (columns ascend)
__device__ inline i64 spb_lower_bound(const int* __restrict__ col, i64 lo, i64 hi, i64 bound) {
    while (lo < hi) {
        const i64 m = lo + ((hi - lo) >> 1);
        if ((i64)col[m] < bound) lo = m + 1;
        else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_spb_count_rows(const i64* __restrict__ indptr, const int* __restrict__ col, i64 n, int nblk,
                                                        int bw, i64 stride, i64* __restrict__ cnt, int* __restrict__ longest) {
    const i64 step = (i64)gridDim.x * 256, items = n * nblk;
    int mine = 0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < items; i += step) {
        const i64 r = i / nblk;
        const int b = (int)(i - r * nblk);
        const i64 lo = indptr[r], hi = indptr[r + 1];
        i64 c = hi - lo;
        if (nblk > 1) {
            const i64 f0 = spb_lower_bound(col, lo, hi, (i64)b * bw);
            c = spb_lower_bound(col, f0, hi, (i64)(b + 1) * bw) - f0;
        }
        cnt[(i64)b * stride + r + 1] = c;
        if (b == 0 && (int)(hi - lo) > mine) mine = (int)(hi - lo);
    }
    if (mine > 0) atomicMax(longest, mine);
}

__global__ __launch_bounds__(256) void k_spb_count_cols(const i64* __restrict__ indptr, const int* __restrict__ col, i64 n, i64 nnz,
                                                        int bw, i64 stride, u64* __restrict__ cnt) {
    const i64 step = (i64)gridDim.x * 256;
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < nnz; p += step) {
        const i64 b = spb_row_of(indptr, n, p) / bw;
        atomicAdd(&cnt[b * stride + col[p] + 1], (u64)1);
    }
}

__device__ inline i64 spb_quads(i64 c) { return (c + 3) / 4 * 4; }

// the sum of the padded counts of tile blockIdx.x
__global__ __launch_bounds__(256) void k_spb_scan_part(const i64* __restrict__ cnt, i64 len, i64* __restrict__ part) {
    __shared__ i64 red[256];
    const i64 base = (i64)blockIdx.x * SPB_SCAN_TILE + (i64)threadIdx.x * SPB_SCAN_PER_THREAD;
    i64 s = 0;
    for (int e = 0; e < SPB_SCAN_PER_THREAD; ++e)
        if (base + e < len) s += spb_quads(cnt[base + e]);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
// one workgroup: part <- its exclusive prefix sum, 1024 tiles at a time with the carry of those before
__global__ __launch_bounds__(1024) void k_spb_scan_top(i64* __restrict__ part, i64 tiles) {
    __shared__ i64 buf[1024];
    __shared__ i64 carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (i64 base = 0; base < tiles; base += 1024) {
        const i64 mine = base + tid < tiles ? part[base + tid] : 0;
        buf[tid] = mine;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const i64 t = tid >= off ? buf[tid - off] : 0;
            __syncthreads();
            buf[tid] += t;
            __syncthreads();
        }
        if (base + tid < tiles) part[base + tid] = carry + buf[tid] - mine;
        __syncthreads();
        if (tid == 1023) carry += buf[1023];
        __syncthreads();
    }
}
// cnt <- the inclusive prefix sum of its padded counts; part: the tiles' exclusive offsets
__global__ __launch_bounds__(256) void k_spb_scan_apply(i64* __restrict__ cnt, i64 len, const i64* __restrict__ part) {
    __shared__ i64 buf[256];
    const int tid = threadIdx.x;
    const i64 base = (i64)blockIdx.x * SPB_SCAN_TILE + (i64)tid * SPB_SCAN_PER_THREAD;
    i64 v[SPB_SCAN_PER_THREAD];
    i64 s = 0;
    for (int e = 0; e < SPB_SCAN_PER_THREAD; ++e) {
        s += base + e < len ? spb_quads(cnt[base + e]) : 0;
        v[e] = s;
    }
    buf[tid] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const i64 t = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += t;
        __syncthreads();
    }
    const i64 before = part[blockIdx.x] + buf[tid] - s;
    for (int e = 0; e < SPB_SCAN_PER_THREAD; ++e)
        if (base + e < len) cnt[base + e] = before + v[e];
}

__global__ __launch_bounds__(256) void k_spb_fill(unsigned short* __restrict__ idx, int* __restrict__ perm, i64 cntp, int bw) {
    const i64 step = (i64)gridDim.x * 256;
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < cntp; q += step) {
        idx[q] = (unsigned short)bw;
        perm[q] = -1;
    }
}

__global__ __launch_bounds__(256) void k_spb_claim_rows(const i64* __restrict__ indptr, const int* __restrict__ col, i64 n, i64 nnz,
                                                        int nblk, int bw, i64 stride, const i64* __restrict__ segptr,
                                                        unsigned short* __restrict__ idx, int* __restrict__ perm) {
    const i64 step = (i64)gridDim.x * 256;
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < nnz; p += step) {
        const i64 r = spb_row_of(indptr, n, p);
        const i64 j = col[p], b = j / bw;
        const i64 first = nblk > 1 ? spb_lower_bound(col, indptr[r], p, b * bw) : indptr[r];
        const i64 q = segptr[b * stride + r] + (p - first);
        idx[q] = (unsigned short)(j - b * bw);
        perm[q] = (int)p;
    }
}

__global__ __launch_bounds__(256) void k_spb_claim_cols(const i64* __restrict__ indptr, const int* __restrict__ col, i64 n, i64 nnz,
                                                        int bw, i64 stride, i64 nseg, const i64* __restrict__ segptr,
                                                        int* __restrict__ fill, u64* __restrict__ keys) {
    const i64 step = (i64)gridDim.x * 256;
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < nnz; p += step) {
        const i64 r = spb_row_of(indptr, n, p);
        const i64 j = col[p], b = r / bw;
        const int slot = atomicAdd(&fill[b * nseg + j], 1);
        keys[segptr[b * stride + j] + slot] = spbuild_key(p, r - b * bw);
    }
}

__device__ inline void spb_write(u64 key, i64 q, unsigned short* __restrict__ idx, int* __restrict__ perm, int bw) {
    const bool pad = key == CORPUS_KEY_PAD;
    idx[q] = pad ? (unsigned short)bw : spbuild_key_off(key);
    perm[q] = pad ? -1 : spbuild_key_pos(key);
}

// a wave per (block, segment) of up to CORPUS_WAVE_MAX padded entries; the longer ones are k_spb_sort_block's
__global__ __launch_bounds__(256) void k_spb_sort_wave(const i64* __restrict__ segptr, i64 nflat, i64 nseg, const u64* __restrict__ keys,
                                                       unsigned short* __restrict__ idx, int* __restrict__ perm, int bw) {
    const int lane = threadIdx.x & 63;
    const i64 step = (i64)gridDim.x * 4;
    for (i64 f = (i64)blockIdx.x * 4 + (threadIdx.x >> 6); f < nflat; f += step) {       // uniform per wave
        const i64 at = f / nseg * (nseg + 1) + f % nseg;
        const i64 lo = segptr[at], len = segptr[at + 1] - lo;
        if (len == 0 || !spbuild_wave_sorted(len)) continue;
        u64 key = lane < len ? keys[lo + lane] : CORPUS_KEY_PAD;
        key = corpus_sort_wave_key(key, lane);
        if (lane < len) spb_write(key, lo + lane, idx, perm, bw);
    }
}

// a workgroup per listed segment (list: its place in the flat segptr), P keys in dynamic LDS, P the launch's padded length
__global__ __launch_bounds__(1024) void k_spb_sort_block(const i64* __restrict__ list, const i64* __restrict__ segptr, i64 P,
                                                         const u64* __restrict__ keys, unsigned short* __restrict__ idx,
                                                         int* __restrict__ perm, int bw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* k = reinterpret_cast<u64*>(smem);
    const int tid = threadIdx.x, nt = blockDim.x;
    const i64 at = list[blockIdx.x];
    const i64 lo = segptr[at], len = segptr[at + 1] - lo;        // len <= P: the host took P from this very segptr
    for (i64 i = tid; i < P; i += nt) k[i] = i < len ? keys[lo + i] : CORPUS_KEY_PAD;
    __syncthreads();
    corpus_sort_keys(k, P, tid, nt);
    for (i64 i = tid; i < len; i += nt) spb_write(k[i], lo + i, idx, perm, bw);
}

}  // namespace rri
