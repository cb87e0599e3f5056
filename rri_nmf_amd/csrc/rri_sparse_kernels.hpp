// rri_sparse_kernels.hpp -- the weighted flavour (WRRI, nmf.py:687-701, :735-746) when W_mat is a 0/1
// observation pattern given as CSR: the recommender case (sklearn_interface.py:78-102), where only the
// observed entries of X - W T ever enter a sum.  Same algebra and the same schedule as rri_wrri_kernels.hpp
// (maintained masked residual E, pass B / pass C per topic step), but E lives on the pattern only:
//
//   CSR copy  (rowptr, col, e )   row products      b_i = sum_j e'_ij t_j ,  nt_i = sum_j t_j^2     (j in row i)
//   CSC copy  (colptr, row, ec)   column sums       a_j = sum_i w_i e'_ij ,  nw_j = sum_i w_i^2     (i in column j)
//
// Both copies take every rank-one correction e' = e - (a1_i b1_j + a2_i b2_j) with the same operations in
// the same order, so they stay bit-identical and every sum has a fixed order (no atomics).  One kernel serves
// both orientations: a "segment" is a row of the CSR copy or a column of the CSC copy, the per-segment factors
// come from one vector pair, the per-entry factors from LDS tables (k_sp_blk below; gathering them from L2
// instead ran at 1.3-1.7 TB/s of index / value traffic, bound by L2 sector bandwidth).
//
// Bytes per observed entry and topic step (fp32 values, uint16 block offsets): pass B 6 (CSR read), pass C
// 10 + 10 (read + write of both copies) = 26 B, against 12.25 B per DENSE entry of the bit-packed dense
// schedule: the sparse formulation moves fewer bytes below ~47 % density (at the 5 % of BASELINE config 5: 9x).
#pragma once
#include "rri_kernels.hpp"
#include "rri_layout.hpp"

namespace rri {

// Blocked segment store.  A copy of the pattern is cut into blocks along its GATHER dimension (column blocks
// of the CSR copy, row blocks of the CSC copy), at most SP_BLOCK_BYTES / (3 * sizeof(TF)) wide, so that the three
// factor vectors an entry needs {b1, b2, v}[gather index] sit in LDS for the whole block (10240 entries of fp32
// factors for an fp32 handle, 5120 of fp64 for an fp64 handle) and the per-entry index is a uint16 offset into
// the block.  Entries are ordered (block, segment, offset); segptr[block][segment] delimits them.  The sums of a
// segment come out per block -- S[block][segment] -- and the consumers that already add row-dot panels
// (k_wwcol) or row-block partials (k_reduce) add the blocks in a fixed order.
//
// Factors are rounded to the table type TF on BOTH sides (the per-segment scalars too), so the CSR and the CSC
// copy apply bit-identical corrections; for an fp32 handle that is the rounding the stored residual has anyway.
// (SP_BLOCK_BYTES = 120 KiB, spx_block_cap and the work item SpWork are in rri_layout.hpp, with the host code that cuts the blocks)
template <typename SX> struct SpTab { typedef float type; };
template <> struct SpTab<double> { typedef double type; };

template <int LPS>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int off = LPS >> 1; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

//   e' = e - (A1[s] * B1[g] + [UPD2] A2[s] * B2[g])            g = block offset + idx[p]
//   WRITE: val[p] = e' (rounded to the storage type; the sums then use the stored value, as the dense pass does)
//   DO_S : S1[blk][s] = sum e' * V[g] ,  S2[blk][s] = sum V[g]^2
// Every segment is padded to a multiple of 4 entries, so a lane moves 4 consecutive entries per load: 8 bytes of offsets +
// 16 (fp32) / 32 (fp64) bytes of values, up to 8 such quads in flight per lane; with one entry per load the passes ran at
// a third of the bandwidth.  One segment per group of LPS lanes; 1024 threads share the tables.
//
// Round 3 (tools/sp_blk_probe.hip: this kernel, round 2's and the candidates that lost, outside the library on BASELINE
// config 5's pattern; profiles/r03_sp_blk_probe*.log): 141 -> 100 us per pass at 5e7 entries, 0.44 -> 0.63 of 8 TB/s.
//   * ONE ROUND OF WORKGROUPS.  The work list had ~3 x 256 items "of equal entry count" -- 774 to 780 in fact: three full
//     rounds of the 256 CUs (one 1024-thread workgroup each, the LDS tables) and a fourth for the last 6 to 12 items, a
//     quarter of the launch with 250 CUs idle.  The host now cuts at most n_cu items (rri_upload_observed_csr): 138 -> 115 us.
//   * PLAIN loads and stores instead of non-temporal ones: 115 -> 100 us (both copies; the read-modify-write of a line it
//     has just loaded is what the L2 is for).
//   * pads point at a ZERO SLOT of the tables (offset bw, written by the host when it builds the copies) instead of being
//     branched around: `if (gi == SP_PAD) continue` had become control flow per ENTRY, each entry's gathers issued, waited
//     for and consumed before the next entry's were issued (the ISA: lgkmcnt 2, 1, 0 per entry).  -8 % at 774 items.
//   * {b1, b2} of an offset side by side in one table: one 8-byte gather (ds_read_b64, the bank behaviour of a 4-byte one)
//     instead of two; SQ_LDS_BANK_CONFLICT 11.9e6 -> 8.0e6, SQ_LDS_IDX_ACTIVE 22.1e6 -> 16.8e6 cycles per launch, time
//     unchanged within the noise -- the LDS was not what the pass waited for.
// What did NOT help, measured on the same copies: a software pipeline across segments (the next segment's quads requested
// before this one is worked on, bounds and factors staged in LDS, dump quads for the idle lanes so that no memory
// instruction sits under divergent control flow: waves parked on s_waitcnt 67 % -> 20 %, but stalled at ISSUE 66 %, 150-175
// us); fp32 fused multiply-adds for the two corrections (-25 % vector-ALU instructions, 129.7 against 130.8 us, and a
// quarter of the stored values an ulp away); requesting the next segment's bounds ahead; starting half of the waves late.
template <typename SX> struct SpPair;
template <> struct SpPair<float> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct SpPair<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <typename SX> struct SpQuad;
template <> struct SpQuad<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct SpQuad<double> { typedef double type __attribute__((ext_vector_type(4))); };
typedef unsigned short sp_us4 __attribute__((ext_vector_type(4)));
// dynamic LDS of k_sp_blk: {b1, b2} pairs and v for bw + 1 offsets (the last one: the zero slot of the pads)
template <typename SX>
__host__ __device__ constexpr size_t sp_lds_bytes(int bw) { return (size_t)3 * (bw + 1) * sizeof(typename SpTab<SX>::type); }

template <typename SX, bool DO_S, bool UPD2, bool WRITE, int LPS>
__global__ __launch_bounds__(1024) void k_sp_blk(const SpWork* __restrict__ work, const i64* __restrict__ segptr,
                                                 i64 nseg, const unsigned short* __restrict__ idx,
                                                 SX* __restrict__ val, int bw, i64 gdim,
                                                 const double* __restrict__ B1, const double* __restrict__ B2,
                                                 const double* __restrict__ V, const double* __restrict__ A1,
                                                 const double* __restrict__ A2, double* __restrict__ S1,
                                                 double* __restrict__ S2, i64 lds, const DevState* __restrict__ st) {
    typedef typename SpTab<SX>::type TF;
    typedef typename SpPair<TF>::type TF2;
    typedef typename SpQuad<SX>::type V4;
    if (st->halt) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int bw1 = bw + 1;                        // slot bw: the zero entry the pads point at
    TF2* tb12 = reinterpret_cast<TF2*>(smem);      // [bw1] {b1, b2}
    TF* tv = reinterpret_cast<TF*>(tb12 + bw1);    // [bw1]
    const SpWork w = work[blockIdx.x];
    const i64 g0 = (i64)w.blk * bw;
    for (int g = threadIdx.x; g < bw1; g += 1024) {
        const bool in = g < bw && g0 + g < gdim;
        TF2 p;
        p[0] = in ? (TF)B1[g0 + g] : TF(0);
        p[1] = (UPD2 && in) ? (TF)B2[g0 + g] : TF(0);
        tb12[g] = p;
        if (DO_S) tv[g] = in ? (TF)V[g0 + g] : TF(0);
    }
    __syncthreads();
    constexpr int UNR = 8;
    constexpr int GROUPS = 1024 / LPS;
    const int sub = threadIdx.x % LPS, grp = threadIdx.x / LPS;
    const i64* sp = segptr + (i64)w.blk * (nseg + 1);
    const sp_us4* idx4 = reinterpret_cast<const sp_us4*>(idx);
    V4* val4 = reinterpret_cast<V4*>(val);
    for (int s = w.s0 + grp; s < w.s1; s += GROUPS) {
        const i64 q0 = sp[s] >> 2, q1 = sp[s + 1] >> 2;     // in quads: segment bounds are multiples of 4
        const double c1 = (double)(TF)A1[s];
        const double c2 = UPD2 ? (double)(TF)A2[s] : 0.0;
        double s1 = 0.0, s2 = 0.0;
        for (i64 q = q0 + sub; q < q1; q += (i64)LPS * UNR) {
            sp_us4 g[UNR];
            V4 e[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const i64 qq = q + (i64)u * LPS;
                if (qq < q1) {
                    g[u] = idx4[qq];
                    e[u] = val4[qq];
                } else {
                    const unsigned short z = (unsigned short)bw;
                    g[u] = sp_us4{z, z, z, z};
                    e[u] = V4{SX(0), SX(0), SX(0), SX(0)};
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const i64 qq = q + (i64)u * LPS;
                if (qq >= q1) break;
                V4 out = e[u];
                TF2 f12[4];
                TF fv[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {                // the gathers of a quad first, then its arithmetic
                    const int gi = g[u][m];
                    f12[m] = tb12[gi];
                    fv[m] = DO_S ? tv[gi] : TF(0);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    double corr = c1 * (double)f12[m][0];
                    if (UPD2) corr = fma(c2, (double)f12[m][1], corr);
                    double x = (double)e[u][m] - corr;
                    if (WRITE) {
                        const SX r = (SX)x;
                        out[m] = r;
                        x = (double)r;
                    }
                    if (DO_S) {
                        const double v = (double)fv[m];
                        s1 = fma(x, v, s1);
                        s2 = fma(v, v, s2);
                    }
                }
                if (WRITE) val4[qq] = out;
            }
        }
        if (DO_S) {
            s1 = group_sum<LPS>(s1);
            s2 = group_sum<LPS>(s2);
            if (sub == 0) { S1[(i64)w.blk * lds + s] = s1; S2[(i64)w.blk * lds + s] = s2; }
        }
    }
}

// ---- the unweighted flavour with X kept as CSR (RRI_UNWEIGHTED_SPARSE) ------------------------------------------------
// A Gram-form topic step needs two products of X: the row dots X t_t (for the W column of topic t) and the column sums
// w_{t+1}^T X (for the next T row).  Both inputs are ready at the same moment, so ONE read-only launch serves both: its work
// list holds the items of the row copy (segments = rows, gathered from a table of t_t over the item's column block) followed
// by those of the column copy (segments = columns, gathered from a table of w_{t+1} over the item's row block); item i takes
// the copy work[i].pad.  S[copy][blk * lds + seg] are the per-block partial sums in the layout k_wcol (Ypart: column blocks x
// n) and k_reduce / k_trow_small (Zpart: row blocks x LD) already add in a fixed order.  No corrections, no write-back: 6 B
// per stored entry and copy for fp32 X (2 of offset, 4 of value), 12 B per entry and topic step for both.
//
// The tables hold the factors as DOUBLES (the dense pass multiplies by the float64 factors; rounding them to the storage type
// would move the sums by 1e-7 of their size against the dense handle): one vector per block instead of k_sp_blk's three, so a
// block is SP_BLOCK_BYTES / 8 ~ 15296 wide -- 1.5x k_sp_blk's fp32 width, 3x its fp64 width -- and the uint16 offsets still fit.
// What k_sp_blk learnt is kept: quads of entries per load, 8 in flight per lane, plain loads, pads into the zero slot of the
// table (offset bw) rather than a branch per entry, and at most n_cu items in all, cut by entry count (the host's work lists).
constexpr int SPX_UNR = 8;
__host__ __device__ constexpr size_t spx_lds_bytes(int bw) { return (size_t)(bw + 1) * sizeof(double); }

template <typename SX>
struct SpxArgs {
    const SpWork* work;                 // items of copy 0, then of copy 1
    int first;                          // first item of this launch (a launch may run one copy's items only)
    const i64* segptr[2];
    const unsigned short* idx[2];
    const SX* val[2];
    const double* F[2];                 // per-entry factor: T[t, :] (copy 0, d entries) / W[:, tz] (copy 1, n entries)
    double* S[2];                       // S[blk * lds + seg]
    i64 nseg[2], gdim[2], lds[2];
    int bw[2], lps[2];
};

template <typename SX, int LPS>
__device__ __forceinline__ void spx_segments(const SpWork& w, const i64* __restrict__ segptr, i64 nseg,
                                             const unsigned short* __restrict__ idx, const SX* __restrict__ val, int bw,
                                             const double* __restrict__ tab, double* __restrict__ S, i64 lds) {
    typedef typename SpQuad<SX>::type V4;
    constexpr int GROUPS = 1024 / LPS;
    const int sub = threadIdx.x % LPS, grp = threadIdx.x / LPS;
    const i64* sp = segptr + (i64)w.blk * (nseg + 1);
    const sp_us4* idx4 = reinterpret_cast<const sp_us4*>(idx);
    const V4* val4 = reinterpret_cast<const V4*>(val);
    for (int s = w.s0 + grp; s < w.s1; s += GROUPS) {
        const i64 q0 = sp[s] >> 2, q1 = sp[s + 1] >> 2;     // segment bounds are multiples of 4 entries
        double acc = 0.0;
        for (i64 q = q0 + sub; q < q1; q += (i64)LPS * SPX_UNR) {
            sp_us4 g[SPX_UNR];
            V4 e[SPX_UNR];
#pragma unroll
            for (int u = 0; u < SPX_UNR; ++u) {
                const i64 qq = q + (i64)u * LPS;
                if (qq < q1) {
                    g[u] = idx4[qq];
                    e[u] = val4[qq];
                } else {                                     // the zero slot: no branch per entry below
                    const unsigned short z = (unsigned short)bw;
                    g[u] = sp_us4{z, z, z, z};
                    e[u] = V4{SX(0), SX(0), SX(0), SX(0)};
                }
            }
#pragma unroll
            for (int u = 0; u < SPX_UNR; ++u) {
                double f[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) f[m] = tab[g[u][m]];     // the gathers of a quad first, then its arithmetic
#pragma unroll
                for (int m = 0; m < 4; ++m) acc = fma((double)e[u][m], f[m], acc);
            }
        }
        acc = group_sum<LPS>(acc);
        if (sub == 0) S[(i64)w.blk * lds + s] = acc;
    }
}

template <typename SX>
__global__ __launch_bounds__(1024) void k_spx_pass(SpxArgs<SX> a, const DevState* __restrict__ st) {
    if (st->halt) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* tab = reinterpret_cast<double*>(smem);   // [bw + 1]; slot bw: the zero entry the pads point at
    const SpWork w = a.work[a.first + blockIdx.x];
    const int cp = w.pad;
    const int bw = a.bw[cp];
    const i64 g0 = (i64)w.blk * bw, gdim = a.gdim[cp];
    const double* F = a.F[cp];
    for (int g = threadIdx.x; g <= bw; g += 1024) tab[g] = (g < bw && g0 + g < gdim) ? F[g0 + g] : 0.0;
    __syncthreads();
    switch (a.lps[cp]) {
        case 8: spx_segments<SX, 8>(w, a.segptr[cp], a.nseg[cp], a.idx[cp], a.val[cp], bw, tab, a.S[cp], a.lds[cp]); break;
        case 16: spx_segments<SX, 16>(w, a.segptr[cp], a.nseg[cp], a.idx[cp], a.val[cp], bw, tab, a.S[cp], a.lds[cp]); break;
        case 32: spx_segments<SX, 32>(w, a.segptr[cp], a.nseg[cp], a.idx[cp], a.val[cp], bw, tab, a.S[cp], a.lds[cp]); break;
        default: spx_segments<SX, 64>(w, a.segptr[cp], a.nseg[cp], a.idx[cp], a.val[cp], bw, tab, a.S[cp], a.lds[cp]); break;
    }
}

// X T^T on the canonical CSR for the W half with T fixed (k_wsweep_rows, the fold-in): Qt[l][i] = sum_p x_p Tt[col_p][l],
// one wave per row, lane = topic (64 topics per round), entries of the row in order.  Tt: d x kp (T transposed, pad 0).
template <typename SX>
__global__ __launch_bounds__(256) void k_spx_xtt(const i64* __restrict__ rowptr, const int* __restrict__ col,
                                                 const SX* __restrict__ xval, i64 n, const double* __restrict__ Tt, int k,
                                                 int kp, double* __restrict__ Qt, i64 ldq) {
    const int lane = threadIdx.x & 63;
    const i64 i = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const i64 p0 = rowptr[i], p1 = rowptr[i + 1];
    for (int l0 = 0; l0 < k; l0 += 64) {
        const int l = l0 + lane;
        double acc = 0.0;
        for (i64 p = p0; p < p1; ++p) {
            const double x = (double)xval[p];
            if (l < k) acc = fma(x, Tt[(i64)col[p] * kp + l], acc);
        }
        if (l < k) Qt[(i64)l * ldq + i] = acc;
    }
}

// Residual on the pattern (the sparse counterpart of k_resid): r_ij = x_ij - W[i,:] . T[:,j] for the entries of
// row i.  One wave per row, 8 lanes per entry (lane q of a group takes the topics q, q+8, ...: one 64-byte
// read of the TRANSPOSED T per step), 8 entries per wave in flight.  Tt: d x kp (kp = k rounded up to 8, pad 0).
//   E      != NULL: E[p] = r                                   (refresh of the maintained residual)
//   rowobj != NULL: rowobj[i] = sum_j r^2                      (true_objective, nmf.py:71-94, on the mask)
//   rowpos != NULL: rowpos[i] = sum_j max(r, 0)^2              (reset search, nmf.py:770-773: outside the
//                                                               pattern x = 0 and max(0 - WT, 0) = 0)
//   rowhat != NULL: rowhat[i] = sum_j (W T)_ij^2               (unweighted X on CSR: ||X - W T||^2 = sum r^2 +
//                                                               <W^T W, T T^T> - sum of these over the pattern)
template <typename SX>
__global__ __launch_bounds__(256) void k_sp_resid(const i64* __restrict__ rowptr, const int* __restrict__ col,
                                                  const SX* __restrict__ xval, i64 n, const double* __restrict__ Wt,
                                                  i64 ldw, const double* __restrict__ Tt, int k, int kp,
                                                  SX* __restrict__ E, double* __restrict__ rowobj,
                                                  double* __restrict__ rowpos, double* __restrict__ rowhat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* wsh = reinterpret_cast<double*>(smem);   // [4][kp]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 i = (i64)blockIdx.x * 4 + wave;
    const bool live = i < n;
    for (int l = lane; l < kp; l += 64) wsh[wave * kp + l] = (live && l < k) ? Wt[(i64)l * ldw + i] : 0.0;
    __syncthreads();
    const int q = lane & 7, slot = lane >> 3;
    const double* wrow = wsh + wave * kp;
    double obj = 0.0, pos = 0.0, hat = 0.0;
    const i64 p0 = live ? rowptr[i] : 0, p1 = live ? rowptr[i + 1] : 0;
    for (i64 pb = p0; pb < p1; pb += 8) {
        const i64 p = pb + slot;
        const bool ok = p < p1;
        const int j = ok ? col[p] : 0;
        const double* trow = Tt + (i64)j * kp;
        double a0 = 0.0, a1 = 0.0;
        int l = q;
        for (; l + 8 < kp; l += 16) {
            a0 = fma(wrow[l], trow[l], a0);
            a1 = fma(wrow[l + 8], trow[l + 8], a1);
        }
        if (l < kp) a0 = fma(wrow[l], trow[l], a0);
        double acc = a0 + a1;
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 4, 64);
        if (ok && q == 0) {
            const double r = (double)xval[p] - acc;
            if (E) E[p] = (SX)r;
            obj = fma(r, r, obj);
            const double rp = fmax(r, 0.0);
            pos = fma(rp, rp, pos);
            hat = fma(acc, acc, hat);
        }
    }
    if (rowobj || rowpos || rowhat) {
        obj = wave_sum<double>(obj);
        pos = wave_sum<double>(pos);
        hat = wave_sum<double>(hat);
        if (lane == 0 && live) {
            if (rowobj) rowobj[i] = obj;
            if (rowpos) rowpos[i] = pos;
            if (rowhat) rowhat[i] = hat;
        }
    }
}

// a blocked copy of the residual after a refresh: out[q] = e[perm[q]] (perm < 0: padding of a segment, kept 0)
template <typename SX>
__global__ __launch_bounds__(256) void k_sp_permute(const SX* __restrict__ e, const int* __restrict__ perm, i64 count,
                                                    SX* __restrict__ out) {
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < count; q += (i64)gridDim.x * 256) {
        const int p = perm[q];
        out[q] = p >= 0 ? e[p] : SX(0);
    }
}

// ---- tf-idf and row normalisation of an X kept as CSR (matrixops.py:124-179; rri_csr_column_positive_counts, rri_csr_scale_X) ----
// Preprocessing rewrites the canonical values sp_x; the two blocked copies are then gathered from them again by k_sp_permute.
//   k_spx_poscount  df_j = number of stored x_ij > 0 (explicit zeros and the pads of a segment do not count): a wave walks the
//                   segments of column j in the column copy, row block after row block, and adds integers -- exact, no atomics
//                   (atomic increments of a d-long counter from the canonical CSR took 2.0 ms at 6.3 M Zipf entries, nearly all
//                   of it the 10^5 increments of the one counter of the most frequent term; this walk takes 0.23 ms there, the
//                   time of the one wave that walks that term's 10^5 entries)
//   k_spx_rowtot    tot_i = sum_j (double(x_ij) * s_j) + spacing(1), one group of LPS lanes per row, lane-strided, the products
//                   rounded before they are added (the host adds the stored products of X.multiply(idf)); *nzero counts the rows
//                   with tot_i < 1e-10 -- normalize's zero_sum_fix makes those DENSE rows 1/d, which a CSR pattern cannot take, so
//                   the host launches nothing further when there is one and X stays as it was
//   k_spx_scale     x_ij <- (1 / tot_i) * (double(x_ij) * s_j), or double(x_ij) * s_j without tot; rounded once, when stored
//                   (UNI: 0 in the rows with tot_i < 1e-10, which the handle then keeps as uniform rows, below)
template <typename SX>
__global__ __launch_bounds__(256) void k_spx_poscount(const i64* __restrict__ segptr, i64 nseg, int nblk,
                                                      const SX* __restrict__ val, double* __restrict__ df) {
    const int lane = threadIdx.x & 63;
    const i64 j = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);      // one wave per column: it leaves or stays as a whole
    if (j >= nseg) return;
    unsigned cnt = 0;
    for (int b = 0; b < nblk; ++b) {
        const i64 p0 = segptr[(i64)b * (nseg + 1) + j], p1 = segptr[(i64)b * (nseg + 1) + j + 1];
        for (i64 p = p0 + lane; p < p1; p += 64) cnt += val[p] > SX(0) ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) df[j] = (double)cnt;
}

template <typename SX, int LPS>
__global__ __launch_bounds__(256) void k_spx_rowtot(const i64* __restrict__ rowptr, const int* __restrict__ col,
                                                    const SX* __restrict__ xval, i64 n, const double* __restrict__ s,
                                                    double* __restrict__ tot, unsigned long long* __restrict__ nzero) {
    const int sub = threadIdx.x % LPS;
    const i64 i = (i64)blockIdx.x * (256 / LPS) + threadIdx.x / LPS;
    const bool live = i < n;                                 // the lanes of a dead group still take part in the shuffles
    const i64 p0 = live ? rowptr[i] : 0, p1 = live ? rowptr[i + 1] : 0;
    double acc = 0.0;
    for (i64 p = p0 + sub; p < p1; p += LPS) {
        const double x = (double)xval[p];
        acc += s ? __dmul_rn(x, s[col[p]]) : x;
    }
    acc = group_sum<LPS>(acc);
    if (live && sub == 0) {
        const double t = acc + 2.220446049250313e-16;        // np.spacing(1), matrixops.py:140
        tot[i] = t;
        if (t < 1e-10) atomicAdd(nzero, 1ull);
    }
}

template <typename SX, int LPS, bool UNI = false>
__global__ __launch_bounds__(256) void k_spx_scale(const i64* __restrict__ rowptr, const int* __restrict__ col,
                                                   SX* __restrict__ xval, i64 n, const double* __restrict__ s,
                                                   const double* __restrict__ tot) {
    const int sub = threadIdx.x % LPS;
    const i64 i = (i64)blockIdx.x * (256 / LPS) + threadIdx.x / LPS;
    if (i >= n) return;
    const i64 p0 = rowptr[i], p1 = rowptr[i + 1];
    const double r = tot ? 1.0 / tot[i] : 1.0;
    if (UNI && tot && tot[i] < 1e-10) {                      // a uniform row (rri_csr_scale_X_uniform): stored zeros
        for (i64 p = p0 + sub; p < p1; p += LPS) xval[p] = SX(0);
        return;
    }
    for (i64 p = p0 + sub; p < p1; p += LPS) {
        const double x = (double)xval[p];
        const double t = s ? x * s[col[p]] : x;              // X * idf               (matrixops.py:172)
        xval[p] = (SX)(tot ? r * t : t);                     // diag(1 / tot) X       (:141-142)
    }
}

// Sparse-times-dense products with the X on the pattern, for the randomized SVD behind the NNDSVD start of the
// recommender flavour (initialization.py:104-105 on W_mat .* X; 16 such products, 0.5 s each in scipy at 5e7 entries):
//   out[blk][seg][v] = sum over the entries p of segment (blk, seg) of x_p * B[blk * bw + idx[p]][v]      v < m <= 64
// on a blocked copy of the pattern (rows as segments: X B; columns as segments: X^T Q).  One wave per segment, lane =
// column v of B: every entry costs one coalesced row of B (L2-resident); x_p comes through the copy's permutation
// from the canonical CSR values.  The blocks of a segment are added by k_sp_sum_blocks.
template <typename SX>
__global__ __launch_bounds__(256) void k_sp_spmm(const i64* __restrict__ segptr, i64 nseg, int nblk,
                                                 const unsigned short* __restrict__ idx, const int* __restrict__ perm,
                                                 const SX* __restrict__ xcanon, int bw, const double* __restrict__ B,
                                                 int m, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const i64 wid = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (i64)nblk * nseg) return;
    const int blk = (int)(wid / nseg);
    const i64 seg = wid - (i64)blk * nseg;
    const i64 p0 = segptr[(i64)blk * (nseg + 1) + seg], p1 = segptr[(i64)blk * (nseg + 1) + seg + 1];
    const double* Bb = B + (i64)blk * bw * m;
    double acc = 0.0;
    for (i64 p = p0; p < p1; p += 4) {                 // segments are padded to multiples of 4 (SP_PAD, perm < 0)
        int off[4], pp[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { off[u] = idx[p + u]; pp[u] = perm[p + u]; }
        double xv[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = pp[u] >= 0;
            xv[u] = ok ? (double)xcanon[pp[u]] : 0.0;
            bv[u] = (ok && lane < m) ? Bb[(i64)off[u] * m + lane] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fma(xv[u], bv[u], acc);
    }
    if (lane < m) out[wid * m + lane] = acc;
}

// res[seg][v] = sum_blk part[blk][seg][v], blocks in order
__global__ __launch_bounds__(256) void k_sp_sum_blocks(const double* __restrict__ part, i64 count, int nblk,
                                                       double* __restrict__ res) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    res[e] = ordered_sum<8>(part + e, count, 0, nblk, 1);
}

// the reset row max(X[mi,:] - W[mi,:] T, 0) (nmf.py:770-775) from the pattern of row mi = *row_idx; out has d
// entries and was zeroed by the caller
template <typename SX>
__global__ __launch_bounds__(256) void k_sp_reset_row(const i64* __restrict__ rowptr, const int* __restrict__ col,
                                                      const SX* __restrict__ xval, const double* __restrict__ Wt,
                                                      i64 ldw, const double* __restrict__ T, i64 ldt, int k,
                                                      const i64* __restrict__ row_idx, double* __restrict__ out) {
    const i64 mi = *row_idx;
    const i64 p = rowptr[mi] + (i64)blockIdx.x * 256 + threadIdx.x;
    if (p >= rowptr[mi + 1]) return;
    const int j = col[p];
    double acc = 0.0;
    for (int l = 0; l < k; ++l) acc = fma(Wt[(i64)l * ldw + mi], T[(i64)l * ldt + j], acc);
    out[j] = fmax((double)xval[p] - acc, 0.0);
}


// ---- uniform rows of an X kept as CSR (rri_set_uniform_rows, rri_csr_scale_X_uniform) -----------------------------------------
// normalize's zero_sum_fix (matrixops.py:143-147) turns a row whose total is below 1e-10 into the DENSE row 1/d.  The pattern
// cannot hold it, but such rows are few and all alike: with U their sorted list and c their value, X = S + c e_U 1^T, where S is
// the stored CSR with zeros in the rows of U.  Every product with X is the product with S (the kernels above, unchanged) plus a
// term of O(|U| + n + d) work, added by one small launch AFTER the product into what the product left.  Every sum below has a
// fixed order (thread-strided partial sums, then block_sum or a loop over the partials), float64, no atomics; all sums over
// columns run over j < d, never over the pad columns.  With U empty none of these kernels is launched.

// the topic step: Ypart[0][i] += c sum_j trow[j] for i in U (the last workgroup), Zpart[0][j] += c sum_{i in U} wc[i] for j < d
// (workgroups 0 .. nzb-1, each taking the |U| terms itself): block 0 of the partials that k_wcol / k_reduce / k_trow_* add in order
template <bool DO_Y, bool DO_Z>
__global__ __launch_bounds__(1024) void k_spu_pass(const int* __restrict__ U, int nu, double cval,
                                                   const double* __restrict__ trow, i64 d, const double* __restrict__ wc,
                                                   double* __restrict__ Ypart0, double* __restrict__ Zpart0, int nzb,
                                                   const DevState* __restrict__ st) {
    if (st->halt) return;
    __shared__ double scratch[16];
    if (DO_Z && (int)blockIdx.x < nzb) {
        double a = 0.0;
        for (int u = threadIdx.x; u < nu; u += 1024) a += wc[U[u]];
        a = block_sum(a, scratch);
        const i64 j = (i64)blockIdx.x * 1024 + threadIdx.x;
        if (j < d) Zpart0[j] += cval * a;
    } else if (DO_Y) {
        double a = 0.0;
        for (i64 j = threadIdx.x; j < d; j += 1024) a += trow[j];
        a = block_sum(a, scratch);
        for (int u = threadIdx.x; u < nu; u += 1024) Ypart0[U[u]] += cval * a;
    }
}

// T fixed: Qt[l][i] += c sum_j Tm[l][j] for i in U; one workgroup per row l of Tm
__global__ __launch_bounds__(256) void k_spu_xtt(const int* __restrict__ U, int nu, double cval, const double* __restrict__ Tm,
                                                 i64 ldt, i64 d, double* __restrict__ Qt, i64 ldq) {
    __shared__ double scratch[4];
    const int l = blockIdx.x;
    double a = 0.0;
    for (i64 j = threadIdx.x; j < d; j += 256) a += Tm[(i64)l * ldt + j];
    a = block_sum(a, scratch);
    for (int u = threadIdx.x; u < nu; u += 256) Qt[(i64)l * ldq + U[u]] += cval * a;
}

// sh[v] = sum over r in [r0, r1) of B[row(r)][v], v < m <= 64, row(r) = idx ? idx[r] : r; B row-major with m columns.  1024 threads:
// 16 groups of 64 lanes take every 16th row, the groups are added in order.  sh: 17 x 64 doubles; the result is in sh[16 * 64 + v]
__device__ __forceinline__ void spu_panel_sum(const double* __restrict__ B, const int* __restrict__ idx, i64 r0, i64 r1, int m,
                                              double* sh) {
    const int v = threadIdx.x & 63, g = threadIdx.x >> 6;
    double a = 0.0;
    if (v < m)
        for (i64 r = r0 + g; r < r1; r += 16) a += B[(idx ? (i64)idx[r] : r) * m + v];
    sh[g * 64 + v] = a;
    __syncthreads();
    if (g == 0) {
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += sh[q * 64 + v];
        sh[16 * 64 + v] = t;
    }
    __syncthreads();
}
// X B: part[b][v] = sum of B's rows of chunk b (rows < d), then out[i][v] += c sum_b part[b][v] for i in U
__global__ __launch_bounds__(1024) void k_spu_panel_part(const double* __restrict__ B, i64 d, int m, i64 chunk,
                                                         double* __restrict__ part) {
    __shared__ double sh[17 * 64];
    const i64 r0 = (i64)blockIdx.x * chunk;
    spu_panel_sum(B, nullptr, r0, r0 + chunk < d ? r0 + chunk : d, m, sh);
    if (threadIdx.x < 64) part[(i64)blockIdx.x * 64 + threadIdx.x] = sh[16 * 64 + threadIdx.x];
}
__global__ __launch_bounds__(256) void k_spu_panel_rows(const int* __restrict__ U, int nu, double cval,
                                                        const double* __restrict__ part, int nb, int m, double* __restrict__ out) {
    const int v = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= nu || v >= m) return;
    double t = 0.0;
    for (int b = 0; b < nb; ++b) t += part[(i64)b * 64 + v];
    out[(i64)U[u] * m + v] += cval * t;
}
// X^T Q: out[j][v] += c sum_{i in U} Q[i][v] for every j < d; a workgroup takes the |U| rows itself, then 256 rows of out
__global__ __launch_bounds__(1024) void k_spu_panel_all(const int* __restrict__ U, int nu, double cval, const double* __restrict__ Q,
                                                        int m, i64 d, double* __restrict__ out) {
    __shared__ double sh[17 * 64];
    spu_panel_sum(Q, U, 0, nu, m, sh);
    const int v = threadIdx.x & 63, g = threadIdx.x >> 6;
    if (v >= m) return;
    const double add = cval * sh[16 * 64 + v];
    const i64 j0 = (i64)blockIdx.x * 256;
    for (i64 j = j0 + g; j < j0 + 256 && j < d; j += 16) out[j * m + v] += add;
}

// the residual of a uniform row is dense: r_ij = c - (W T)_ij for all j < d.  One workgroup per row of U, T read coalesced along
// j (k d work per row); it REPLACES what k_sp_resid left for that row (there: the row's stored zeros)
//   rowobj[i] = sum_j r^2,  rowpos[i] = sum_j max(r, 0)^2,  rowhat[i] = sum_j (W T)_ij^2     (all j < d: the objective's
//   pattern form subtracts rowhat from <W^T W, T T^T>, which for this row leaves exactly sum_j r^2)
__global__ __launch_bounds__(256) void k_spu_resid(const int* __restrict__ U, double cval, const double* __restrict__ Wt, i64 ldw,
                                                   const double* __restrict__ T, i64 ldt, i64 d, int k,
                                                   double* __restrict__ rowobj, double* __restrict__ rowpos,
                                                   double* __restrict__ rowhat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* wsh = reinterpret_cast<double*>(smem);   // [k]
    __shared__ double scratch[4];
    const i64 i = U[blockIdx.x];
    for (int l = threadIdx.x; l < k; l += 256) wsh[l] = Wt[(i64)l * ldw + i];
    __syncthreads();
    double obj = 0.0, pos = 0.0, hat = 0.0;
    for (i64 j = threadIdx.x; j < d; j += 256) {
        double acc = 0.0;
        for (int l = 0; l < k; ++l) acc = fma(wsh[l], T[(i64)l * ldt + j], acc);
        const double r = cval - acc;
        obj = fma(r, r, obj);
        const double rp = fmax(r, 0.0);
        pos = fma(rp, rp, pos);
        hat = fma(acc, acc, hat);
    }
    obj = block_sum(obj, scratch);
    pos = block_sum(pos, scratch);
    hat = block_sum(hat, scratch);
    if (threadIdx.x == 0) {
        if (rowobj) rowobj[i] = obj;
        if (rowpos) rowpos[i] = pos;
        if (rowhat) rowhat[i] = hat;
    }
}

// the reset row when row mi = *row_idx is uniform: out[j] = max(c - W[mi,:] T[:,j], 0) for all j < d (after k_sp_reset_row,
// whose entries for that row it overwrites); any other row: nothing
__global__ __launch_bounds__(256) void k_spu_reset_row(const int* __restrict__ U, int nu, double cval, const double* __restrict__ Wt,
                                                       i64 ldw, const double* __restrict__ T, i64 ldt, i64 d, int k,
                                                       const i64* __restrict__ row_idx, double* __restrict__ out) {
    const i64 mi = *row_idx;
    int lo = 0, hi = nu;                 // U is sorted: first entry >= mi
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((i64)U[mid] < mi) lo = mid + 1; else hi = mid;
    }
    if (lo >= nu || (i64)U[lo] != mi) return;
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    double acc = 0.0;
    for (int l = 0; l < k; ++l) acc = fma(Wt[(i64)l * ldw + mi], T[(i64)l * ldt + j], acc);
    out[j] = fmax(cval - acc, 0.0);
}

// the stored values of the rows of U become 0 (the pattern stays); one wave per row
template <typename SX>
__global__ __launch_bounds__(256) void k_spu_zero_rows(const int* __restrict__ U, int nu, const i64* __restrict__ rowptr,
                                                       SX* __restrict__ xval) {
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= nu) return;
    const i64 i = U[u];
    for (i64 p = rowptr[i] + (threadIdx.x & 63); p < rowptr[i + 1]; p += 64) xval[p] = SX(0);
}

// rows with tot_i < 1e-10 in row order (rri_csr_scale_X_uniform): one workgroup, a contiguous range of rows per thread, counted,
// scanned and then written -- no atomics, so the list comes out sorted.  rows: room for n entries
__global__ __launch_bounds__(1024) void k_spu_collect(const double* __restrict__ tot, i64 n, int* __restrict__ rows,
                                                      i64* __restrict__ count) {
    __shared__ int cnt[1024];
    const i64 per = (n + 1023) / 1024;
    const i64 i0 = (i64)threadIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
    int c = 0;
    for (i64 i = i0; i < i1; ++i) c += tot[i] < 1e-10 ? 1 : 0;
    cnt[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0;
        for (int t = 0; t < 1024; ++t) { const int v = cnt[t]; cnt[t] = a; a += v; }
        *count = a;
    }
    __syncthreads();
    int o = cnt[threadIdx.x];
    for (i64 i = i0; i < i1; ++i)
        if (tot[i] < 1e-10) rows[o++] = (int)i;
}

}  // namespace rri
