// rri_fiterr_kernels.hpp -- k_fiterr_entries, k_fiterr_sum and k_value_range: the clipped prediction error of W T at the stored
// entries of a resident corpus, and the range of its values (DESIGN "Fit from a resident corpus"; the term and the request check
// are rri_fiterr.hpp's, the pieces, the chunks, the lane rule and the butterfly rri_loglik's).
//
// What the kernels read.  W as the handle keeps it, transposed: Wt (k x n, stride ldw).  T through the transposed copy made once
// per call, Tt (d x kp, kp = loglik_kp(k), the pad zero).  The corpus's indices and values where they lie: a chunk is a pair of
// offsets into them, nothing of the corpus's size is copied.
//
// k_fiterr_entries<LANES> follows k_loglik_entries.  A 256-thread workgroup takes four pieces, one per wave; the wave stages its
// request's row of W in LDS (kp doubles; the four rows of a workgroup take at most 32 KB at RRI_MAX_K).  LANES = loglik_lanes(k)
// lanes share an entry: lane l of the group takes the pairs of topics l, l + LANES, ... with one 16-byte load from the entry's row
// of Tt and one from the staged row each, and the group's lanes are added by the xor butterfly, in which every lane forms the same
// sums in the same order.  Group g of the G = 64 / LANES groups takes the entries g, g + G, ... of the piece in ascending order,
// adds their r^2 and |r|, and its lane 0 stores the clipped prediction when the call asks for it (a plain store to a slot no other
// lane writes).  The groups are added by the same butterfly at the distances LANES .. 32 and lane 0 stores the piece's two
// partials with plain stores.  Every order depends on LANES (that is, on k) and on the piece alone.
//
// k_fiterr_sum.  One lane per request of the chunk adds the request's pieces in ascending order; a request without a piece gets
// zeros.  k_value_range.  One stage of a min / max: every workgroup leaves one pair; run over the values into <= 1024 pairs, then
// once more, as a single workgroup, over those.  No atomics anywhere.
#pragma once

#include "rri_fiterr.hpp"
#include "rri_loglik_kernels.hpp"

namespace rri {

template <int LANES>
__global__ __launch_bounds__(256) void k_fiterr_entries(const double* __restrict__ Wt, i64 ldw, const double* __restrict__ Tt, int k,
                                                        const i64* __restrict__ rows, i64 q0, const LoglikPiece* __restrict__ pieces,
                                                        i64 npieces, const int* __restrict__ indices, const double* __restrict__ values,
                                                        double lo, double hi, double* __restrict__ pred, double* __restrict__ psq,
                                                        double* __restrict__ pabs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int kp = loglik_kp(k), kp2 = kp >> 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* wrow = reinterpret_cast<double*>(smem) + (size_t)wave * kp;        // [4][kp]
    const i64 piece = (i64)blockIdx.x * 4 + wave;
    const bool live = piece < npieces;
    LoglikPiece pc{0, 0, 0};
    if (live) {
        pc = pieces[piece];
        const i64 row = rows ? rows[pc.req] : q0 + pc.req;
        for (int t = lane; t < kp; t += 64) wrow[t] = t < k ? Wt[(i64)t * ldw + row] : 0.0;
    }
    __syncthreads();
    if (!live) return;
    constexpr int G = 64 / LANES;
    const int grp = lane / LANES, gl = lane % LANES;
    const double2* w2 = reinterpret_cast<const double2*>(wrow);
    double sq = 0.0, ab = 0.0;
    for (int e = grp; e < pc.cnt; e += G) {
        const int j = indices[pc.e0 + e];
        const double v = values[pc.e0 + e];
        const double2* t2 = reinterpret_cast<const double2*>(Tt) + (i64)j * kp2;
        double p = 0.0;
        for (int c = gl; c < kp2; c += LANES) {
            const double2 t = t2[c], w = w2[c];
            p = fma(w.x, t.x, p);
            p = fma(w.y, t.y, p);
        }
        p = loglik_butterfly(p, LANES / 2, 1);
        const double cl = fiterr_clip(p, lo, hi), r = cl - v;
        sq += r * r;
        ab += fabs(r);
        if (pred && gl == 0) pred[pc.e0 + e] = cl;
    }
    if (G > 1) {
        sq = loglik_butterfly(sq, 32, LANES);
        ab = loglik_butterfly(ab, 32, LANES);
    }
    if (lane == 0) {
        psq[piece] = sq;
        pabs[piece] = ab;
    }
}

__global__ __launch_bounds__(256) void k_fiterr_sum(const i64* __restrict__ first, i64 nreq, const double* __restrict__ psq,
                                                    const double* __restrict__ pabs, double* __restrict__ sq_out,
                                                    double* __restrict__ abs_out) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= nreq) return;
    double sq = 0.0, ab = 0.0;
    for (i64 p = first[r]; p < first[r + 1]; ++p) {
        sq += psq[p];
        ab += pabs[p];
    }
    sq_out[r] = sq;
    abs_out[r] = ab;
}

// one stage of the range: workgroup b leaves (min of in_min, max of in_max) over the items it strides across in out[2 b],
// out[2 b + 1].  First stage: in_min = in_max = the values, a grid of at most 1024; second: the pairs of the first (strided by 2),
// one workgroup.  Every workgroup of a grid no larger than ceil(items / 256) has an item.
__global__ __launch_bounds__(256) void k_value_range(const double* in_min, const double* in_max, i64 step, i64 items, double* out) {
    __shared__ double smin[4], smax[4];
    double lo = INFINITY, hi = -INFINITY;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < items; i += (i64)gridDim.x * 256) {
        lo = fmin(lo, in_min[i * step]);
        hi = fmax(hi, in_max[i * step]);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, off, 64));
        hi = fmax(hi, __shfl_xor(hi, off, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        smin[wave] = lo;
        smax[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[2 * (i64)blockIdx.x] = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
        out[2 * (i64)blockIdx.x + 1] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    }
}

}  // namespace rri
