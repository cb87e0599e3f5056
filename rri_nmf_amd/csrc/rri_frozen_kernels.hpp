// rri_frozen_kernels.hpp -- the device side of the frozen statistics (rri_frozen.hpp; DESIGN 4.11 "Frozen rows").
//
//   k_frozen_add      the frozen rows' share of a T-row step, added into red right after k_reduce -- the place where a row-sharded
//                     run all-reduces it -- and, for a column check without a T-row step, into the two doubles of ctail
//   k_wtx_panel       the whole panel W^T X of a dense handle in ONE pass over X, on the float64 matrix cores
//   k_panel_sum       the row blocks' partial panels added in a fixed order: F <- decay F + sum_b part[b]
//   k_frozen_gram     A <- decay A + W^T W and s <- decay s + 1^T W, every entry one workgroup's ordered sum
//   k_frozen_axpy_t   F <- decay F + R^T for the d x m result of the CSR product (X^T Q of the blocked store)
//   k_frozen_clear    a reset of topic t: row t of B, row and column t of A, s[t]
//   k_frozen_dot      <B, T> as 256 block partials (the objective's share)
// No atomics anywhere: a rerun leaves the same bits.
//
// k_wtx_panel.  P = Wt X contracts over the rows of X.  A workgroup of four waves takes a block of rows and 64 CT columns, all
// 16 NT topics of a chunk: v_mfma_f64_16x16x4_f64 with A = a 16-topic x 4-row tile of Wt and B = a 4-row x 16-column tile of X
// widened exactly to float64 (operand and result layouts as in k_topn_rows).  Wt is k-major, so the 32 rows of a step are 32
// contiguous doubles per topic: the four waves stage them in LDS once and every wave reads its A fragments from there; X goes
// from global memory straight into the B operand, 16 consecutive columns per quarter wave and 64 per row over the four waves.
// (NT, CT) = (4, 4) up to 64 topics in the chunk and (8, 2) up to 128: 64 accumulator registers per lane either way, and the
// wider column block of the small chunk halves what is re-read of Wt per byte of X.  Each row block stores its partial panel;
// k_panel_sum adds them.  k <= 128 reads X once; a larger k re-reads it per chunk of 128 topics.
#pragma once

#include "rri_frozen.hpp"

namespace rri {

constexpr int FZ_CHUNK = 128;         // topics per launch of k_wtx_panel
constexpr int FZ_RCH = 32;            // rows staged per step
constexpr int FZ_WLD = FZ_RCH + 1;    // LDS stride of a topic's staged values

// red[j] += B[t,j]; slice 0 of the Gram part += [A[t,:] | A[t,t] | s[tprev] or nothing]   (frozen_red_gram)
__global__ __launch_bounds__(256) void k_frozen_add(double* __restrict__ red, i64 ldz, int k, int t, int tprev,
                                                    const double* __restrict__ B, const double* __restrict__ A,
                                                    const double* __restrict__ s) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j < ldz) red[frozen_red_col(j)] += B[(i64)t * ldz + j];
    if (blockIdx.x == 0)
        for (int l = threadIdx.x; l < k + 2; l += 256) {
            if (l < k) red[frozen_red_gram(ldz, l)] += A[(i64)t * k + l];
            else if (l == k) red[frozen_red_gram(ldz, l)] += A[(i64)t * k + t];
            else if (tprev >= 0) red[frozen_red_gram(ldz, l)] += s[tprev];
        }
}
// the column check that no T-row step carries: tail[0] (this handle's sum W[:,tprev], k_colsum_tail) += s[tprev]
__global__ void k_frozen_add_tail(double* __restrict__ tail, int tprev, const double* __restrict__ s) {
    if (threadIdx.x == 0 && blockIdx.x == 0) tail[0] += s[tprev];
}

template <typename SX, int NT, int CT>
__global__ __launch_bounds__(256) void k_wtx_panel(const SX* __restrict__ X, i64 ldx, int n, int d,
                                                   const double* __restrict__ Wt, i64 ldw, int t0, int kc, int rows_per_block,
                                                   double* __restrict__ part, i64 ldp) {
    __shared__ double wsh[16 * NT * FZ_WLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int ntile = (kc + 15) >> 4;                                  // <= NT (the host picks NT from kc)
    const i64 r0 = (i64)blockIdx.y * rows_per_block;
    const i64 r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    i64 jcol[CT];
    bool jok[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        jcol[c] = ((i64)blockIdx.x * CT + c) * 64 + wave * 16 + lr;
        jok[c] = jcol[c] < d;
    }
    f64x4 acc[NT][CT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[tt][c] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int sr = tid & 31, st0 = tid >> 5;                           // staging: row of the step, first topic
    // The loads of step i + 1 are in flight while the matrix cores work on step i: every thread keeps its share of the next W
    // tile (wr) and its B operands of the next step (xr) in registers.  A slot of xr is refilled as soon as its MFMAs have been
    // issued, so each load has the rest of the step to arrive.
    double wr[2 * NT];
    SX xr[FZ_RCH / 4][CT];
    auto load_w = [&](i64 i0) {
#pragma unroll
        for (int q = 0; q < 2 * NT; ++q) {
            const int tt = st0 + 8 * q;
            wr[q] = (tt < kc && i0 + sr < r1) ? Wt[(i64)(t0 + tt) * ldw + i0 + sr] : 0.0;
        }
    };
    auto load_x = [&](i64 i0, int s) {
        const i64 i = i0 + 4 * s + lk;
#pragma unroll
        for (int c = 0; c < CT; ++c) xr[s][c] = (jok[c] && i < r1) ? X[i * ldx + jcol[c]] : (SX)0;
    };
    load_w(r0);
#pragma unroll
    for (int s = 0; s < FZ_RCH / 4; ++s) load_x(r0, s);
    for (i64 i0 = r0; i0 < r1; i0 += FZ_RCH) {
        __syncthreads();                                               // the tile of the step before has been read
#pragma unroll
        for (int q = 0; q < 2 * NT; ++q) {
            const int tt = st0 + 8 * q;
            if (tt < 16 * ntile) wsh[tt * FZ_WLD + sr] = wr[q];
        }
        __syncthreads();
        load_w(i0 + FZ_RCH);                                           // (past r1: zeros, nothing is read)
#pragma unroll
        for (int s = 0; s < FZ_RCH / 4; ++s) {
            double b[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) b[c] = (double)xr[s][c];         // widened exactly
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) {
                if (tt < ntile) {
                    const double a = wsh[(16 * tt + lr) * FZ_WLD + 4 * s + lk];
#pragma unroll
                    for (int c = 0; c < CT; ++c) acc[tt][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[c], acc[tt][c], 0, 0, 0);
                }
            }
            load_x(i0 + FZ_RCH, s);
        }
    }
    // result register r of tile (tt, c): topic 16 tt + lk + 4 r of the chunk, column jcol[c]
#pragma unroll
    for (int tt = 0; tt < NT; ++tt)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tp = 16 * tt + lk + 4 * r;
                if (tp < kc && jok[c]) part[((i64)blockIdx.y * kc + tp) * ldp + jcol[c]] = acc[tt][c][r];
            }
}

// F[t0 + tp, j] <- decay F[t0 + tp, j] + sum_b part[b][tp][j], b ascending; one thread per entry, j < d (the pad columns stay 0)
__global__ __launch_bounds__(256) void k_panel_sum(const double* __restrict__ part, int nblocks, int kc, i64 ldp, int d, int t0,
                                                   double decay, double* F) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    const int tp = blockIdx.y;
    if (j >= d || tp >= kc) return;
    double a = 0.0;
    for (int b = 0; b < nblocks; ++b) a += part[((i64)b * kc + tp) * ldp + j];
    double* f = F + (i64)(t0 + tp) * ldp + j;
    *f = decay * *f + a;
}

// block (a, b): b < k and b >= a: A[a,b] = A[b,a] <- decay A[a,b] + <Wt[a,:], Wt[b,:]>; b == k: s[a] <- decay s[a] + sum Wt[a,:]
__global__ __launch_bounds__(256) void k_frozen_gram(const double* __restrict__ Wt, i64 ldw, i64 n, int k, double decay,
                                                     double* A, double* s) {
    __shared__ double scratch[40];
    const int a = blockIdx.x, b = blockIdx.y;
    if (b < a) return;
    double v = 0.0;
    if (b < k) for (i64 i = threadIdx.x; i < n; i += 256) v = fma(Wt[(i64)a * ldw + i], Wt[(i64)b * ldw + i], v);
    else for (i64 i = threadIdx.x; i < n; i += 256) v += Wt[(i64)a * ldw + i];
    v = block_sum(v, scratch);
    if (threadIdx.x != 0) return;
    if (b < k) {
        const double f = decay * A[(i64)a * k + b] + v;
        A[(i64)a * k + b] = f;
        A[(i64)b * k + a] = f;
    } else {
        s[a] = decay * s[a] + v;
    }
}

// F[t0 + l, j] <- decay F[t0 + l, j] + R[j, l] for the d x m result R of the CSR product
__global__ __launch_bounds__(256) void k_frozen_axpy_t(const double* __restrict__ R, int m, int d, int t0, double decay, double* F,
                                                       i64 ldf) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    const int l = blockIdx.y;
    if (j >= d || l >= m) return;
    double* f = F + (i64)(t0 + l) * ldf + j;
    *f = decay * *f + R[j * m + l];
}

__global__ __launch_bounds__(256) void k_frozen_clear(double* __restrict__ B, i64 ldb, double* __restrict__ A, int k,
                                                      double* __restrict__ s, int t) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j < ldb) B[(i64)t * ldb + j] = 0.0;
    if (j < k) { A[(i64)t * k + j] = 0.0; A[j * k + t] = 0.0; }
    if (j == 0) s[t] = 0.0;
}

// out[b] = block b's share of <B, T> over k x ld entries (pad columns are zero in both), 256 blocks
__global__ __launch_bounds__(256) void k_frozen_dot(const double* __restrict__ B, const double* __restrict__ T, i64 total,
                                                    double* __restrict__ out) {
    __shared__ double scratch[40];
    double v = 0.0;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < total; i += (i64)gridDim.x * 256) v = fma(B[i], T[i], v);
    v = block_sum(v, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = v;
}

}  // namespace rri
