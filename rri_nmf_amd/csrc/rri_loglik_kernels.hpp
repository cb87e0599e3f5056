// rri_loglik_kernels.hpp -- k_loglik_entries and k_loglik_sum: the log-likelihood of stored counts under the rows of W T, two
// launches per chunk of requests (DESIGN "Log-likelihood of entries"; the term, the pieces, the chunks and the lane rule are
// rri_loglik.hpp's).
//
// What the kernels read.  W as the handle keeps it, transposed: Wt (k x n, stride ldw), so W[i,:] is strided.  T through a
// transposed copy made once per call, Tt (d x kp, kp = loglik_kp(k), the pad zero): an entry's k factors are then contiguous and
// 16-byte aligned (400 B at k = 50), and at 10000 x 50 the copy is 4 MB, which stays in L2 and the Infinity Cache.
//
// k_loglik_entries<LANES>.  A 256-thread workgroup takes four pieces, one per wave.  The wave stages its request's row of W in
// LDS once (kp doubles, at most 8 KB at RRI_MAX_K; the four rows of a workgroup take at most 32 KB).  LANES = loglik_lanes(k)
// lanes share an entry (4 up to k = 128, 16 above; 64 only in a measurement build that asks for it):
// lane l of the group takes the pairs of topics l, l + LANES, ... with one 16-byte load from the entry's row of Tt and one from
// the staged row each, and adds the two products in topic order; the group's lanes are then added by a butterfly of cross-lane
// moves (distances LANES / 2 .. 1), in which every lane forms the same sums in the same order, so each lane of the group holds the
// entry's p and forms the same term.  Group g of the G = 64 / LANES groups takes the entries g, g + G, g + 2 G, ... of the piece
// in ascending order and adds their terms, values and floored flags; the groups are added by the same butterfly at the distances
// LANES .. 32, and lane 0 stores the piece's three partials with plain stores.  Every order here depends on LANES (that is, on k)
// and on the piece alone.
//
// k_loglik_sum.  One lane per request of the chunk adds the request's pieces in ascending order and writes the three outputs; a
// request without a piece gets zeros.  No atomics anywhere.
#pragma once

#include "rri_loglik.hpp"
#include "rri_device.hpp"

namespace rri {

// the sum over the lanes at the xor distances from .. to (both powers of two, from >= to), the same bits in every lane
template <typename V>
__device__ inline V loglik_butterfly(V v, int from, int to) {
    for (int off = from; off >= to; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int LANES>
__global__ __launch_bounds__(256) void k_loglik_entries(const double* __restrict__ Wt, i64 ldw, const double* __restrict__ Tt, int k,
                                                        const i64* __restrict__ rows, i64 q0, const LoglikPiece* __restrict__ pieces,
                                                        i64 npieces, const int* __restrict__ indices, const double* __restrict__ values,
                                                        double floor, double* __restrict__ pll, double* __restrict__ pmass,
                                                        i64* __restrict__ pfloored) {
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
    double ll = 0.0, mass = 0.0;
    int fl = 0;
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
        ll += loglik_term(v, p, floor);
        mass += v;
        fl += loglik_floored(v, p, floor);
    }
    if (G > 1) {
        ll = loglik_butterfly(ll, 32, LANES);
        mass = loglik_butterfly(mass, 32, LANES);
        fl = loglik_butterfly(fl, 32, LANES);
    }
    if (lane == 0) {
        pll[piece] = ll;
        pmass[piece] = mass;
        pfloored[piece] = (i64)fl;
    }
}

__global__ __launch_bounds__(256) void k_loglik_sum(const i64* __restrict__ first, i64 nreq, const double* __restrict__ pll,
                                                    const double* __restrict__ pmass, const i64* __restrict__ pfloored,
                                                    double* __restrict__ ll_out, double* __restrict__ mass_out,
                                                    i64* __restrict__ floored_out) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= nreq) return;
    double ll = 0.0, mass = 0.0;
    i64 fl = 0;
    for (i64 p = first[r]; p < first[r + 1]; ++p) {
        ll += pll[p];
        mass += pmass[p];
        fl += pfloored[p];
    }
    ll_out[r] = ll;
    mass_out[r] = mass;
    floored_out[r] = fl;
}

}  // namespace rri
