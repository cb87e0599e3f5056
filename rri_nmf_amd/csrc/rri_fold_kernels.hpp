// rri_fold_kernels.hpp -- k_wfold_rows and k_wfold_verdict: the W half of every topic of a sweep in one launch, for a pattern-only
// handle with T fixed (the update of an entry, the eligibility rule and the LDS formula are rri_fold.hpp's).
//
// k_wfold_rows<SX, KT>.  A 256-thread workgroup takes FOLD_ROWS = 16 rows.  It stages their entries of the k-major W in LDS (16
// contiguous doubles of every column) and writes what it read to Wprev, the copy k_wsweep_repair restores from.  Then wave w
// takes the rows w, w + 4, w + 8, w + 12 of the group, one at a time:
//   * the row's stored entries in steps of four.  In a step quarter h of the wave holds entry e + h: lane l loads
//     Tt[col][16 a + (l & 15)] for the KT = ceil(k / 16) topic tiles a -- 128 contiguous bytes per quarter and tile -- and that one
//     double is both the A operand (A[l & 15][l >> 4]) and the B operand (B[l >> 4][l & 15]) of v_mfma_f64_16x16x4_f64, so the tile
//     (a, b) of G = sum_e t_e t_e^T takes one instruction per step from registers alone; only the tiles a <= b are formed and the
//     others are their mirror images.  q = sum_e x_e t_e is one multiply-add per tile beside it, the four quarters added at the end
//     by the xor butterfly at distances 16 and 32.  Four steps are loaded before the first is used.  Zeros stand in for the
//     entries past the row's end and the topics past k, so every sum depends on the row's own entries and on k alone;
//   * G goes to the wave's LDS (result register r of lane l: row (l >> 4) + 4 r, column l & 15 of the tile), mirrored;
//   * lane t holds topic t: s_t = q_t - sum_{l != t} G[t][l] w_l with l ascending, then the topics t0 .. k - 1 in order, each
//     fold_entry on lane t and the rank-one correction of every other lane's s.
// At the end the group writes the columns t0 .. k - 1 back and leaves, per topic, the sum of its 16 new entries and the count of
// its negative denominators, rows ascending.  No atomics; which workgroup or wave holds a row changes nothing.
//
// k_wfold_verdict.  One workgroup: a wave per topic adds the groups' partials in a fixed order, then thread 0 applies wwcol_code
// in topic order and halts at the first topic that fails, with the position next_step gives -- what k_wcheck_wcol reports on the
// launch-per-topic schedule.  A reset event leaves pad0 = t* + 1 for k_wsweep_repair.
#pragma once

#include "rri_fold.hpp"
#include "rri_kernels.hpp"

namespace rri {

template <typename SX, int KT>
__global__ __launch_bounds__(256) void k_wfold_rows(double* __restrict__ Wt, double* __restrict__ Wprev, i64 ldw, int n, int k, int t0,
                                                    const i64* __restrict__ rowptr, const int* __restrict__ col,
                                                    const SX* __restrict__ xv, const double* __restrict__ Tt, int kp,
                                                    double* __restrict__ colsum, double* __restrict__ negsum, int nwg, KParams p,
                                                    const DevState* __restrict__ st) {
    if (st->halt) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int KPAD = 16 * KT, GLD = KPAD + 1, WLD = FOLD_ROWS + 1, NTILE = KT * (KT + 1) / 2, U = 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lq = lane >> 4, lr = lane & 15;
    double* gsh = reinterpret_cast<double*>(smem) + (size_t)wave * KPAD * GLD;          // [FOLD_WAVES][KPAD][GLD]
    double* wsh = reinterpret_cast<double*>(smem) + (size_t)FOLD_WAVES * KPAD * GLD;    // [KPAD][WLD]
    unsigned char* nsh = reinterpret_cast<unsigned char*>(wsh + (size_t)KPAD * WLD);    // [KPAD][FOLD_ROWS]
    const i64 i0 = (i64)blockIdx.x * FOLD_ROWS;
    for (int q = tid; q < k * FOLD_ROWS; q += 256) {
        const int t = q / FOLD_ROWS, r = q - t * FOLD_ROWS;
        const i64 i = i0 + r;
        double v = 0.0;
        if (i < n) {
            v = Wt[(i64)t * ldw + i];
            Wprev[(i64)t * ldw + i] = v;
        }
        wsh[t * WLD + r] = v;
        nsh[t * FOLD_ROWS + r] = 0;
    }
    __syncthreads();
    const int grow = lane < KPAD ? lane : KPAD - 1;       // (lanes past the pad read a row that exists and use nothing of it)
    for (int r = wave; r < FOLD_ROWS; r += FOLD_WAVES) {  // the same four rounds for every wave: the barriers below are uniform
        const i64 i = i0 + r;
        const bool live = i < n;
        f64x4 acc[NTILE];
        double qa[KT];
#pragma unroll
        for (int m = 0; m < NTILE; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < KT; ++a) qa[a] = 0.0;
        const i64 e0 = live ? rowptr[i] : 0, e1 = live ? rowptr[i + 1] : 0;
        for (i64 e = e0; e < e1; e += 4 * U) {
            double v[U][KT], x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const i64 ee = e + 4 * u + lq;
                const bool ok = ee < e1;
                const i64 j = ok ? (i64)col[ee] : 0;
                x[u] = ok ? (double)xv[ee] : 0.0;
#pragma unroll
                for (int a = 0; a < KT; ++a) v[u][a] = (ok && 16 * a + lr < k) ? Tt[j * kp + 16 * a + lr] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int m = 0;
#pragma unroll
                for (int a = 0; a < KT; ++a) {
                    qa[a] = fma(x[u], v[u][a], qa[a]);
#pragma unroll
                    for (int b = a; b < KT; ++b, ++m) acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u][a], v[u][b], acc[m], 0, 0, 0);
                }
            }
        }
        double qt = 0.0;
#pragma unroll
        for (int a = 0; a < KT; ++a) {
            qa[a] += __shfl_xor(qa[a], 16);
            qa[a] += __shfl_xor(qa[a], 32);
            if (lq == a) qt = qa[a];          // lane l holds topic l = 16 (l >> 4) + (l & 15)
        }
        {
            int m = 0;
#pragma unroll
            for (int a = 0; a < KT; ++a)
#pragma unroll
                for (int b = a; b < KT; ++b, ++m)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int row = 16 * a + lq + 4 * rr, cg = 16 * b + lr;
                        gsh[row * GLD + cg] = acc[m][rr];
                        if (a != b) gsh[cg * GLD + row] = acc[m][rr];
                    }
        }
        __syncthreads();
        double w = lane < k ? wsh[lane * WLD + r] : 0.0;
        double s = qt;
        for (int l = 0; l < k; ++l) {
            const double wl = __shfl(w, l);
            const double g = gsh[grow * GLD + l];
            if (l != lane) s = fma(-g, wl, s);
        }
        const double gtt = gsh[grow * GLD + grow];
        int negf = 0;
        for (int t = t0; t < k; ++t) {
            int neg = 0;
            const double wn = fold_entry(s, gtt, p, &neg);
            const double dw = __shfl(wn - w, t);
            const double g = gsh[grow * GLD + t];
            if (lane == t) { w = wn; negf = neg; }
            else s = fma(-g, dw, s);
        }
        if (live && lane >= t0 && lane < k) {
            wsh[lane * WLD + r] = w;
            nsh[lane * FOLD_ROWS + r] = (unsigned char)negf;
        }
        __syncthreads();          // the wave's G is free for its next row; after the last round: the tile is complete
    }
    for (int q = tid; q < k * FOLD_ROWS; q += 256) {
        const int t = q / FOLD_ROWS, r = q - t * FOLD_ROWS;
        const i64 i = i0 + r;
        if (t >= t0 && i < n) Wt[(i64)t * ldw + i] = wsh[t * WLD + r];
    }
    if (tid >= t0 && tid < k) {
        double a = 0.0, f = 0.0;
        for (int r = 0; r < FOLD_ROWS; ++r) {       // (rows past n were staged as zeros and never written)
            a += wsh[tid * WLD + r];
            f += (double)nsh[tid * FOLD_ROWS + r];
        }
        colsum[(i64)tid * nwg + blockIdx.x] = a;
        negsum[(i64)tid * nwg + blockIdx.x] = f;
    }
}

__global__ __launch_bounds__(1024) void k_wfold_verdict(const double* __restrict__ colsum, const double* __restrict__ negsum, int nwg,
                                                        int k, int t0, int sweep, KParams p, DevState* st) {
    if (st->halt) return;
    __shared__ double ssum[FOLD_MAX_K], sneg[FOLD_MAX_K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = t0 + wave; t < k; t += 16) {
        double a = ordered_sum<8>(colsum + (i64)t * nwg, 1, lane, nwg, 64);
        double f = ordered_sum<8>(negsum + (i64)t * nwg, 1, lane, nwg, 64);
        a = wave_sum<double>(a);
        f = wave_sum<double>(f);
        if (lane == 0) { ssum[t] = a; sneg[t] = f; }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int t = t0; t < k; ++t) {
        const int code = wwcol_code(ssum[t], sneg[t], p);
        if (code != 0) {
            const StepPos next = next_step(sweep, t, k);         // where a resumed run continues
            halt_set(st, code, t, next.sweep, next.pos);
            st->pad1 = 1;
            if (code == HALT_EVENT_RESET_W) st->pad0 = t + 1;
            return;
        }
    }
}

}  // namespace rri
