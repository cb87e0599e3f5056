// rri_kernels.hpp -- hand-written gfx950 kernels of the RRI topic step (Gram form).
//
// One topic step t of nmf.py:415-476 is, in the reference, two BLAS2 products over X:
//     w_t^T X  (nmf.py:672)   and   X t_t  (nmf.py:729)
// Here ONE streaming pass over X (k_pass) computes  X t_t  (row dots, for the W-column
// update of topic t) AND  w_{t+1}^T X  (column sums, for the T-row update of topic t+1):
// column t+1 of W is not touched between the two (only column t changes in step t), so
// the fused pass is exact and X is read k (+1) times per sweep instead of 2k.
//
// Chain per topic (all on one stream, no host sync):
//   k_reduce      partial column sums / Gram row  -> reduce buffer (the multi-GPU all-reduce point)
//   k_trow_numer  numer_T = w^T X - (w^T W)_{-t} T - reg ; closed-form qf_min       (nmf.py:437-447)
//   k_trow_final  simplex projection / one-hot / reset check; writes T[t,:]          (nmf.py:447,751-761)
//   k_tgram       T T[t,:]^T (k-vector, entry t zeroed) and ||T[t,:]||^2               (nmf.py:730-734)
//   k_pass        the X pass (HBM-bound, the roofline kernel)
//   k_wcol        numer_W = X t - W (T t)_{-t} - reg ; qf_min ; writes W[:,t];
//                 Gram row / norm partials of the NEXT topic                             (nmf.py:464-469,673-676)
// Precision: X (and the mask / masked residual) live in HBM in the handle's storage type SX
// (fp32 or fp64; a dense X that is only read -- the Gram form without weights -- also as float16, see
// XVec<_Float16>).  EVERYTHING else -- W, T, partial sums, the closed-form updates -- is float64:
// the streaming pass converts each loaded X element and accumulates with v_fma_f64.  The pass is
// HBM-bound with the vector ALU ~85 % idle, so float64 arithmetic costs no time, X traffic is
// unchanged, and the result follows the reference's float64 numpy to summation-order rounding
// instead of the ~1e-4 an fp32 accumulation gives on these iterations.
// Rare branches (reset conditions, unbounded problems, dead columns) set DevState::halt;
// every later kernel of the queue then returns at once and the host resolves the event.
// The rules that decide them, and DevState and KParams, are in rri_halt.hpp.
#pragma once
#include <type_traits>

#include "rri_device.hpp"
#include "rri_early_deal.hpp"
#include "rri_halt.hpp"
#include "rri_hip.h"
#include "rri_layout.hpp"
#include "rri_xnarrow.hpp"
#include "rri_xpack.hpp"

namespace rri {

// =========================================================================================
// k_pass: the fused streaming pass over X.
//   grid = npg * nrb workgroups of 256 threads (4 waves); geometry in the comment at the kernel.
//   Per row a wave issues one 16-byte load per lane (1 KiB coalesced; non-temporal: X is never
//   reused inside a pass), keeps U rows in flight, holds its slice of the active T row (DO_Y)
//   and its column-sum accumulators (DO_Z) in registers (float64), and reads the active W-column
//   entries from LDS.  Narrow per-wave panels keep the register count low (more waves resident,
//   more bytes in flight): measured 6.0 TB/s against 4.8 TB/s for 4 KiB-wide panels.
//   UPD: the explicit-residual form north_star names: X is the residual R and the pass first
//   applies the rank-one update R <- R - a b^T (a from LDS, b slice in registers), writes R back
//   and takes the row dots / column sums of the UPDATED residual in the same sweep over memory.
// =========================================================================================
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned __attribute__((may_alias)) u32_any;      // a dword of LDS that other code holds as doubles

template <typename SX> struct XVec;
template <> struct XVec<float> {
    typedef f32x4 type;
    static constexpr int N = 4;
    static __device__ __forceinline__ void unpack(const f32x4& v, double (&o)[4]) {
        o[0] = (double)v[0]; o[1] = (double)v[1]; o[2] = (double)v[2]; o[3] = (double)v[3];
    }
    static __device__ __forceinline__ f32x4 pack(const double (&o)[4]) {
        return f32x4{(float)o[0], (float)o[1], (float)o[2], (float)o[3]};
    }
    static __device__ __forceinline__ f32x4 zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
};
template <> struct XVec<double> {
    typedef f64x2 type;
    static constexpr int N = 2;
    static __device__ __forceinline__ void unpack(const f64x2& v, double (&o)[2]) { o[0] = v[0]; o[1] = v[1]; }
    static __device__ __forceinline__ f64x2 pack(const double (&o)[2]) { return f64x2{o[0], o[1]}; }
    static __device__ __forceinline__ f64x2 zero() { return f64x2{0.0, 0.0}; }
};
// float16 storage (RRI_F16): read-only handles of the Gram form.  8 elements per 16-byte load; half -> float -> double is
// exact for every finite half, subnormals included, so the arithmetic sees the stored values.  pack() only ever re-packs
// values that were read as halves (the ragged edge of k_xtt_mfma): no kernel rounds anything to float16 but k_store_half.
// With 8 elements per lane a workgroup of k_pass / k_colsums covers 2048 columns; k_pass<_Float16, true, true, ...> holds tv[8],
// zacc[8] and 8 rows of 4 VGPRs per lane: 202 VGPRs, 2 waves per SIMD -- and 0.337 ms per pass at 100000 x 10000 against 0.397 for
// the same halves read 8 bytes per lane in the fp32 geometry (122 VGPRs, 4 waves), which was measured and removed.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
template <> struct XVec<_Float16> {
    typedef f16x8 type;
    static constexpr int N = 8;
    static __device__ __forceinline__ void unpack(const f16x8& v, double (&o)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (double)(float)v[e];
    }
    static __device__ __forceinline__ f16x8 pack(const double (&o)[8]) {
        f16x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (_Float16)(float)o[e];
        return r;
    }
    static __device__ __forceinline__ f16x8 zero() {
        return f16x8{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
};

// uint8 storage (RRI_U8): counts 0..255 of a read-only handle of the Gram form.  byte -> float (the per-byte convert instruction)
// -> double is exact.  The X the kernels see is (C[i][j] * cscale[j]) * rscale[i] (XScale below): the two vectors never enter a row
// loop -- X^T w = cscale .* (C^T (rscale .* w)) and X t = rscale .* (C (cscale .* t)), so they are applied where an operand vector
// is loaded and where a partial sum is stored.  pack() only re-packs values read as bytes (the ragged edge of k_xtt_mfma).
// 8 elements per 8-byte load: the register layout of the float16 pass (tv[8], zacc[8], 8 rows in flight; 202 VGPRs, 2 waves per
// SIMD) and its geometry -- a workgroup of k_pass / k_colsums covers 2048 columns -- at half the bytes per row: 0.260 ms per pass
// at 100000 x 10000.  16 elements per 16-byte load (4096 columns per workgroup) takes tv[16] and zacc[16]: 256 VGPRs and 100 AGPRs,
// one wave per SIMD, 0.418 ms; it was measured beside this one in one process and removed.
typedef unsigned char u8x8 __attribute__((ext_vector_type(8)));
template <> struct XVec<unsigned char> {
    typedef u8x8 type;
    static constexpr int N = 8;
    static __device__ __forceinline__ void unpack(const u8x8& v, double (&o)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (double)(float)v[e];
    }
    static __device__ __forceinline__ u8x8 pack(const double (&o)[8]) {
        u8x8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (unsigned char)o[e];
        return r;
    }
    static __device__ __forceinline__ u8x8 zero() { return u8x8{0, 0, 0, 0, 0, 0, 0, 0}; }
};
// The two float64 scale vectors of an RRI_U8 handle: row[n], col[LD] (pad columns hold 1).  Both NULL for every other storage type,
// whose kernels never look at them (`if constexpr` on XSCALED).
struct XScale {
    const double* row;
    const double* col;
};
template <typename SX> constexpr bool XSCALED = std::is_same<SX, unsigned char>::value;
// element (i, j) as the handle's X: (c * s_j) * r_i, in this order everywhere an element is formed on its own
template <typename SX>
__device__ __forceinline__ double x_elem(const SX* __restrict__ X, i64 ldx, i64 i, i64 j, const XScale& xs) {
    if constexpr (XSCALED<SX>) return ((double)(float)X[i * ldx + j] * xs.col[j]) * xs.row[i];
    else return (double)X[i * ldx + j];
}

// streaming load of one vector (16 bytes; 8 for uint8 counts); NT = non-temporal (X is read once per pass, never reused)
template <bool NT, typename V>
__device__ __forceinline__ V stream_load(const V* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

template <bool NT, typename V>
__device__ __forceinline__ void stream_store(V* p, const V& v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// A small job that rides in the grid of a streaming pass instead of costing a launch of its own: the Gram row
// T T[t,:]^T of the topic whose row dots the pass takes (k_tgram below describes it).  T[t,:] is final when the
// pass starts and the result is first read by the k_wcol after the pass, so the two have no order to keep.
// The first `nblocks` workgroups of the grid do the job, the others the pass.
struct TgramJob {
    const double* T; i64 ldt; int d, k, t;
    double* Ttpart; const double* tpart; int ntb, nsplit, finish, sweep;
    KParams p; DevState* st;
    int nblocks;          // k * nsplit, or 0: no job
};
__device__ __forceinline__ void tgram_block(const double* __restrict__ T, i64 ldt, int d, int k, int t, int l, int split,
                                            int ns, double* __restrict__ Ttpart, const double* __restrict__ tpart,
                                            int nblk, int finish, int sweep, const KParams& p, DevState* st,
                                            double* scratch) {
    const int chunk = (d + ns - 1) / ns;
    const int j0 = split * chunk, j1 = min(d, j0 + chunk);
    double acc = 0.0;
    for (int j = j0 + threadIdx.x; j < j1; j += 256) acc = fma(T[(i64)l * ldt + j], T[(i64)t * ldt + j], acc);
    acc = block_sum(acc, scratch);
    if (threadIdx.x == 0) Ttpart[split * k + l] = acc;
    if (finish && l == 0 && split == 0) {
        double ps = 0.0;
        ps = ordered_sum<4>(tpart, 1, threadIdx.x, nblk, 256);
        ps = block_sum(ps, scratch);
        if (threadIdx.x == 0) {
            const int mode = st->tmode;
            st->nt1 = (mode == 0) ? ps : 1.0;
            st->sumT = ps;
            if (trow_resets(ps, p)) halt_set(st, HALT_EVENT_RESET_T, t, sweep, t);
        }
    }
}

// The early-sums schedule (RRI_EARLY_SUMS): a second job in the grid of the fused pass of topic step t.  Of what
// k_wcol<true, true> computes after the pass, everything but the row dots y = X t_t comes from W and T T[t,:]^T alone, which are
// final before the pass is launched (k_trow_early leaves the partials of T T[t,:]^T): per row the dot sum_{l != t} W[i,l] (T T[t,:]^T)[l],
// and for the next topic tn the Gram entries w_tn^T w_l (l != t) and ||w_tn||^2.  `nblocks` workgroups, placed from `first` on among
// the pass's own (after its first round: early_job_first in rri_layout.hpp), `stride` of the pass's own behind each of them
// (early_slot in rri_early_deal.hpp; 0: one contiguous run), walk `tpb` 64-row tiles each with k_wcol's loop --
// the same tiles, the same four-wave split of the columns, the same order of every sum -- and write dot[n], Gpart[b][0..k+2)
// (entries t and k + 1 zero: k_wfin leaves those two per tile) and nt[0] = ||T[t,:]||^2.  No block of the grid reads them.
struct EarlyJob {
    const double* Wt; i64 ldw; int n, k, t, tn;
    const double* Tearly; int nte;             // nte partial vectors T T[t,:]^T (entry t: the share of ||T[t,:]||^2)
    double *dot, *Gpart, *nt;
    int first, nblocks, tpb;                   // nblocks == 0: no job
    int stride;
};
// CH: columns per batch of loads per wave (k_wcol: 16).  The job must fit the registers of the pass it rides in, whatever they
// are (the float64 pass: 74): the batch is as small as that takes; the order of every sum is the same for every CH.
template <int CH>
__device__ __forceinline__ void early_block(const EarlyJob& e, int b, double* sm) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = e.k, t = e.t;
    double* tts = sm;                // [k]
    double* gsh = tts + k;           // [k+2]
    double* dsh = gsh + k + 2;       // [4][64]
    for (int l = tid; l < k + 2; l += 256) gsh[l] = 0.0;
    for (int l = tid; l < k; l += 256) tts[l] = ordered_sum<8>(e.Tearly + l, k, 0, e.nte, 1);
    __syncthreads();
    if (b == 0 && tid == 0) e.nt[0] = tts[t];
    __syncthreads();
    if (tid == 0) tts[t] = 0.0;      // Tt[t] = 0 (nmf.py:732)
    __syncthreads();
    const int ntiles = (e.n + 63) / 64;
    const int tile1 = min(ntiles, (b + 1) * e.tpb);
    for (int tile = b * e.tpb; tile < tile1; ++tile) {
        const i64 i = (i64)tile * 64 + lane;
        const bool valid = i < e.n;
        const double wn = valid ? e.Wt[(i64)e.tn * e.ldw + i] : 0.0;
        double dotv = 0.0;
        for (int l0 = wave; l0 < k; l0 += 4 * CH) {
            double wl[CH];
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int l = l0 + 4 * q;
                wl[q] = (l < k && valid && l != t) ? e.Wt[(i64)l * e.ldw + i] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int l = l0 + 4 * q;
                if (l < k) {   // wave-uniform
                    dotv = fma(wl[q], tts[l], dotv);
                    if (l != t) {
                        const double g = wave_sum<double>(wn * wl[q]);
                        if (lane == 0) gsh[l] += g;   // column l belongs to this wave alone
                    }
                }
            }
        }
        dsh[wave * 64 + lane] = dotv;
        __syncthreads();
        if (wave == 0) {
            if (valid) e.dot[i] = (dsh[lane] + dsh[64 + lane]) + (dsh[128 + lane] + dsh[192 + lane]);
            const double nwp = wave_sum<double>(wn * wn);
            if (lane == 0) gsh[k] += nwp;
        }
        __syncthreads();   // dsh is reused by the next tile
    }
    double* gp = e.Gpart + (i64)b * (k + 2);
    for (int l = tid; l < k + 2; l += 256) gp[l] = gsh[l];
}

// What a row does with its unpacked elements xe[] (the row dots against tv, the column sums against wv), and what ends a chunk
// of U rows: shared by the fp32 / float64 / float16 row loop and the packed one, which differ in how xe[] is filled.
#define RRI_PASS_ROW_SUMS \
            double yp = 0.0;                                                                                      \
        _Pragma("unroll")                                                                                         \
            for (int e = 0; e < VN; ++e) {                                                                        \
                if (DO_Y) yp = fma(xe[e], tv[e], yp);                                                             \
                if (DO_Z) zacc[e] = fma(wv, xe[e], zacc[e]);                                                      \
            }                                                                                                     \
            if constexpr (DO_Y && RS) wave_rowsum8_park(tile, u, lane, yp);                                       \
            else if (DO_Y) {                                                                                      \
                /* the same six DPP steps as wave_sum: the total where they leave it (lane 63), stored from there */ \
                const double tot = wave_sum_lane63<double>(yp);                                                   \
                if (lane == 63) ysh[wave * rpb + l0 + u] = tot;                                                   \
            }
#define RRI_PASS_CHUNK_SUMS \
        if constexpr (DO_Y && RS) {                                                                               \
            const double tot = wave_rowsum8_finish(tile, lane);                                                   \
            if ((lane & 7) == 0) ysh[wave * rpb + l0 + (lane >> 3)] = tot;                                        \
        }

// The row loop of k_pass with the load policy LNT.  A macro, because the kernel needs the loop twice (a workgroup of a
// non-temporal read-only pass takes default-policy loads in its kept row blocks) and every function form costs registers: as
// a lambda -- even one called once -- the float64 read-only pass takes 82 VGPRs instead of 74, 5 waves per SIMD instead of 6.
// One policy per WORKGROUP: a uniform branch around the 8 loads of a chunk is merged by the compiler into one plain load
// (no nt left in the kernel), and two row loops one after the other cost the fp32 pass a wave per SIMD.
#define RRI_PASS_ROWS(LNT) \
    for (int l0 = 0; l0 < rpb; l0 += U) {                                                                         \
        const int r = grow(l0);  /* the U rows of a chunk are consecutive */                                      \
        if (r >= n) break;  /* later chunks lie further down still */                                             \
        V x[U];                                                                                                   \
        _Pragma("unroll")                                                                                         \
        for (int u = 0; u < U; ++u) {                                                                             \
            const int rr = r + u;                                                                                 \
            x[u] = XV::zero();                                                                                    \
            if (rr < n && ok) x[u] = stream_load<LNT>(reinterpret_cast<const V*>(X + (i64)rr * ldx + col));       \
        }                                                                                                         \
        _Pragma("unroll")                                                                                         \
        for (int u = 0; u < U; ++u) {                                                                             \
            const int rr = r + u;                                                                                 \
            double wv = 0.0, na = 0.0, na2 = 0.0;                                                                 \
            if (DO_Z && rr < n) wv = wsh[l0 + u];                                                                 \
            if (UPD > 0 && rr < n) na = -ash[l0 + u];                                                             \
            if (UPD > 1 && rr < n) na2 = -ash2[l0 + u];                                                           \
            double xe[VN];                                                                                        \
            XV::unpack(x[u], xe);                                                                                 \
            if constexpr (UPD > 0) {                                                                              \
        _Pragma("unroll")                                                                                         \
                for (int e = 0; e < VN; ++e) {                                                                    \
                    xe[e] = fma(na, bv[e], xe[e]);                                                                \
                    if (UPD > 1) xe[e] = fma(na2, bv2[e], xe[e]);                                                 \
                }                                                                                                 \
                const V rounded = XV::pack(xe);                                                                   \
                if (rr < n && ok) stream_store<NT>(reinterpret_cast<V*>(X + (i64)rr * ldx + col), rounded);       \
                /* the stored residual is what later passes read: continue with the ROUNDED values */             \
                if constexpr (sizeof(SX) == 4) XV::unpack(rounded, xe);                                           \
            }                                                                                                     \
            RRI_PASS_ROW_SUMS                                                                                     \
        }                                                                                                         \
        RRI_PASS_CHUNK_SUMS                                                                                       \
    }

// The row loop over the packed copy of an fp32 X (rri_xpack.hpp; PK): the chunk of 8 rows is one 7 KiB record per wave, seven
// 16-byte loads per lane instead of eight, unpacked into the same xe[] in the same order, so every sum keeps its bits.  Rows
// past n and columns past ncols were encoded as +0; a lane with col >= ncols skips its loads as in the fp32 loop (codes of
// all ones: zeros).
#define RRI_PASS_ROWS_PK(LNT) \
    for (int l0 = 0; l0 < rpb; l0 += U) {                                                                         \
        const int r = grow(l0);                                                                                   \
        if (r >= n) break;                                                                                        \
        const u32x4* rec = reinterpret_cast<const u32x4*>(XP + xpack::record_offset((unsigned)r >> 3,             \
                                                          (unsigned)(pg * 4 + wave), (unsigned)npg * 4u)) + lane; \
        unsigned xw[4 * xpack::SLOTS];                                                                            \
        _Pragma("unroll")                                                                                         \
        for (int i = 0; i < (int)xpack::SLOTS; ++i) {                                                             \
            const unsigned fill = i == (int)xpack::CODE_SLOT ? ~0u : 0u;                                          \
            u32x4 v = u32x4{fill, fill, fill, fill};                                                              \
            if (ok) v = stream_load<LNT>(rec + i * (int)xpack::LANES);                                            \
            xw[4 * i] = v[0]; xw[4 * i + 1] = v[1]; xw[4 * i + 2] = v[2]; xw[4 * i + 3] = v[3];                   \
        }                                                                                                         \
        _Pragma("unroll")                                                                                         \
        for (int u = 0; u < U; ++u) {                                                                             \
            const int rr = r + u;                                                                                 \
            double wv = 0.0;                                                                                      \
            if (DO_Z && rr < n) wv = wsh[l0 + u];                                                                 \
            unsigned xb[4];                                                                                       \
            xpack::decode_row(xw, u, base4, xb);                                                                  \
            double xe[VN];                                                                                        \
        _Pragma("unroll")                                                                                         \
            for (int e = 0; e < VN; ++e) xe[e] = (double)__uint_as_float(xb[e]);                                  \
            RRI_PASS_ROW_SUMS                                                                                     \
        }                                                                                                         \
        RRI_PASS_CHUNK_SUMS                                                                                       \
    }

// The row loop over the 26-bit copy of an fp32 X (rri_xnarrow.hpp; PK == 2): the chunk of 8 rows is one 6.5 KiB record per wave,
// six 16-byte loads and one 8-byte load per lane, and the record's exception entries -- 16 bits each, lanes take entries lane,
// lane + 64, ... of the list the directory names.  An entry's exponent byte goes to a byte map in LDS, row u of it 64 dwords at
// the start of row u of the wave's row-sum tile; every lane reads back the dword of its row before it decodes the row, which puts
// the exponent in place before xe[] feeds the sums: the same xe[] in the same order as the fp32 loop.
// The overlay is safe because all of it is the wave's own LDS traffic, which the LDS serves in program order, and the compiler
// keeps that order (the map is written as bytes and read as u32_any, which alias the tile's doubles): the map rows are cleared
// after the previous chunk's wave_rowsum8_finish has read the tile, the entries are scattered after the clear, the s_waitcnt and
// wave barrier stand between the scatter and the first read, and wave_rowsum8_park of row u writes only row u of the tile, after
// the map dword of row u was read and before that of row u + 1 is.  The directory words of the next chunk are loaded a chunk
// ahead, and the first 64 entries before the record, so that no load of a chunk waits for another.
// Padding (rows past n, lanes past ncols) decodes to a finite positive number: it meets wv = 0, tv = 0 or a row nobody stores.
#define RRI_PASS_ROWS_PN(LNT) \
    {                                                                                                             \
        unsigned char* const mapb = reinterpret_cast<unsigned char*>(tile);                                       \
        u32_any* const mapw = reinterpret_cast<u32_any*>(tile);                                                   \
        constexpr unsigned MAP_ROW = 72 * sizeof(double);                                                         \
        const unsigned wpanel = (unsigned)(pg * 4 + wave), wpanels = (unsigned)npg * 4u;                          \
        unsigned e0 = 0u, e1 = 0u;                                                                                \
        if (grow(0) < n) {                                                                                        \
            const unsigned long long ri0 = xnarrow::record_index((unsigned)grow(0) >> 3, wpanel, wpanels);        \
            e0 = xdir[ri0]; e1 = xdir[ri0 + 1];                                                                   \
        }                                                                                                         \
        for (int l0 = 0; l0 < rpb; l0 += U) {                                                                     \
            const int r = grow(l0);                                                                               \
            if (r >= n) break;                                                                                    \
            const unsigned long long ri = xnarrow::record_index((unsigned)r >> 3, wpanel, wpanels);               \
            const unsigned char* recb = XP + ri * xnarrow::RECORD_BYTES;                                          \
            unsigned en = 0u;                                                                                     \
            if (e0 + (unsigned)lane < e1) en = xexc[e0 + (unsigned)lane];                                         \
            unsigned n0 = 0u, n1 = 0u;                                                                            \
            if (l0 + U < rpb && grow(l0 + U) < n) {                                                               \
                const unsigned long long rin = xnarrow::record_index((unsigned)grow(l0 + U) >> 3, wpanel, wpanels); \
                n0 = xdir[rin]; n1 = xdir[rin + 1];                                                               \
            }                                                                                                     \
            unsigned xw[xnarrow::LANE_DWORDS];                                                                    \
        _Pragma("unroll")                                                                                         \
            for (int i = 0; i < (int)xnarrow::WIDE_SLOTS; ++i) {                                                  \
                u32x4 v = u32x4{0u, 0u, 0u, 0u};                                                                  \
                if (ok) v = stream_load<LNT>(reinterpret_cast<const u32x4*>(recb) + i * (int)xnarrow::LANES + lane); \
                xw[4 * i] = v[0]; xw[4 * i + 1] = v[1]; xw[4 * i + 2] = v[2]; xw[4 * i + 3] = v[3];               \
            }                                                                                                     \
            {                                                                                                     \
                u32x2 v = u32x2{0u, 0u};                                                                          \
                if (ok) v = stream_load<LNT>(reinterpret_cast<const u32x2*>(recb + xnarrow::dword_offset(24u, 0u)) + lane); \
                xw[24] = v[0]; xw[25] = v[1];                                                                     \
            }                                                                                                     \
        _Pragma("unroll")                                                                                         \
            for (int u = 0; u < U; ++u) mapw[u * (int)(MAP_ROW / 4u) + lane] = 0u;                                \
            if (e0 + (unsigned)lane < e1)                                                                         \
                mapb[xnarrow::map_offset(en & 2047u, MAP_ROW)] = (unsigned char)xnarrow::rare_entry(xbooks, en >> xnarrow::POS_BITS); \
            for (unsigned b = e0 + 64u; b < e1; b += 64u) {      /* wave-uniform: a record with more than 64 entries */ \
                const unsigned j = b + (unsigned)lane;                                                            \
                if (j < e1) {                                                                                     \
                    const unsigned en2 = xexc[j];                                                                 \
                    mapb[xnarrow::map_offset(en2 & 2047u, MAP_ROW)] = (unsigned char)xnarrow::rare_entry(xbooks, en2 >> xnarrow::POS_BITS); \
                }                                                                                                 \
            }                                                                                                     \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                    \
            __builtin_amdgcn_wave_barrier();                                                                      \
        _Pragma("unroll")                                                                                         \
            for (int u = 0; u < U; ++u) {                                                                         \
                const int rr = r + u;                                                                             \
                double wv = 0.0;                                                                                  \
                if (DO_Z && rr < n) wv = wsh[l0 + u];                                                             \
                const unsigned mapped = mapw[u * (int)(MAP_ROW / 4u) + lane];                                     \
                unsigned xb[4];                                                                                   \
                xnarrow::decode_row(xw, u, mapped, xbooks.lo, xbooks.hi, xb);                                     \
                double xe[VN];                                                                                    \
        _Pragma("unroll")                                                                                         \
                for (int e = 0; e < VN; ++e) xe[e] = (double)__uint_as_float(xb[e]);                              \
                RRI_PASS_ROW_SUMS                                                                                 \
            }                                                                                                     \
            RRI_PASS_CHUNK_SUMS                                                                                   \
            if constexpr (!(DO_Y && RS)) __builtin_amdgcn_wave_barrier();                                         \
            e0 = n0; e1 = n1;                                                                                     \
        }                                                                                                         \
    }

// Block = 4 waves = 4 ADJACENT column panels (one per wave, 64 lanes * 16 B each) x one row block.
// Every wave walks all rows of the block, U rows in flight; the 4 row-dot partials of a row meet in
// LDS slots [wave][row] and are added in a fixed order at the end (Ypart has one slice per 4 panels);
// column sums belong to one wave each and go straight to Zpart.
// UPD = 0: X is read only.  UPD = 1: R <- R - a b^T.  UPD = 2: R <- R - a b^T - a2 (b2 - b2sub)^T, the two pending
// rank-one terms of one topic step of the explicit-residual schedule (dw_{t-1} t_{t-1}^T and w_t dt_t^T; b2sub = the
// T row before its update, so dt is formed in registers).  a, a2 come through LDS, b, b2 live in registers.
// PK: the workgroup reads its rows from the packed copy XP (fp32, UPD = 0) unless one of its tiles is flagged (xflags: one byte
// per 8-row chunk and column group, set where an element is outside the window of xbase .. xbase + 14): then it runs today's
// loop on X.  ONE policy per workgroup for the whole row loop, taken in the prologue.
// EJ: the build of the fused read-only pass that carries the early-sums job (EarlyJob); every other launch runs the build without
// it, whose workgroups read no field of `ejob` and start as they always did.
template <typename SX, bool DO_Y, bool DO_Z, int UPD, int U, bool NT, bool RS, int PK = 0, bool EJ = false>
__global__ __launch_bounds__(256) void k_pass(typename std::conditional<(UPD > 0), SX, const SX>::type* __restrict__ X,
                                              i64 ldx, int n, int ncols,
                                              const double* __restrict__ trow, const double* __restrict__ wcol,
                                              double* __restrict__ Ypart, double* __restrict__ Zpart, i64 ldz,
                                              int rpb, int npg, const double* __restrict__ avec,
                                              const double* __restrict__ bvec, const double* __restrict__ avec2,
                                              const double* __restrict__ bvec2, const double* __restrict__ bsub2,
                                              const DevState* __restrict__ st, const TgramJob job, int nrb_il_rot,
                                              int keep_q, const unsigned char* __restrict__ XP = nullptr,
                                              const unsigned char* __restrict__ xflags = nullptr, int xbase = 0,
                                              const double* __restrict__ rscale = nullptr,
                                              const double* __restrict__ cscale = nullptr,
                                              const unsigned* __restrict__ xdir = nullptr,
                                              const unsigned short* __restrict__ xexc = nullptr,
                                              const xnarrow::Books xbooks = xnarrow::Books{},
                                              const EarlyJob ejob = EarlyJob{}) {
    static_assert(!XSCALED<SX> || UPD == 0, "counts with scales are only read");
    static_assert(!PK || (std::is_same<SX, float>::value && UPD == 0 && U == 8), "the packed copy is of a read-only fp32 X");
    static_assert(!EJ || (DO_Y && DO_Z && UPD == 0), "the early-sums job rides in the fused read-only pass");
    typedef XVec<SX> XV;
    typedef typename XV::type V;
    constexpr int VN = XV::N;
    constexpr int PW = 64 * VN;          // columns per wave
    if (st->halt) return;
    if ((int)blockIdx.x < job.nblocks) {
        __shared__ double jscratch[40];
        tgram_block(job.T, job.ldt, job.d, job.k, job.t, (int)blockIdx.x % job.k, (int)blockIdx.x / job.k, job.nsplit,
                    job.Ttpart, job.tpart, job.ntb, job.finish, job.sweep, job.p, job.st, jscratch);
        return;
    }
    // Workgroups are dealt to the 8 XCDs round-robin by blockIdx.x (which XCD block 0 gets is not fixed).  `rot` (top bits of
    // the argument; RRI_PASS_ROT, diagnostics) rotates the tile a workgroup takes inside its group of 8: another XCD for
    // every tile, nothing else changed.
    const int nrb_il = nrb_il_rot & 0x07ffffff;
    const int rot = (int)((unsigned)nrb_il_rot >> 27);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int bid = (int)blockIdx.x - job.nblocks;
    int njobs = job.nblocks;       // workgroups of the grid that are not the pass's own
    if constexpr (EJ) {
        // the early-sums job of the fused pass: ejob.nblocks workgroups from position ejob.first on, the pass's own around them
        const EarlySlot slot = early_slot(bid, ejob.first, ejob.nblocks, ejob.stride);
        if (slot.job) {
            early_block<(sizeof(SX) == 8 ? 4 : 8)>(ejob, slot.index, reinterpret_cast<double*>(smem));
            return;
        }
        bid = slot.index;
        njobs += ejob.nblocks;
    }
    if (rot != 0 && (bid | 7) < (int)gridDim.x - njobs) bid = (bid & ~7) | ((bid + rot) & 7);
    double* ysh = reinterpret_cast<double*>(smem);            // [4 waves][rpb]
    double* wsh = ysh + 4 * rpb;                              // [rpb]
    double* ash = wsh + rpb;                                  // [rpb], only with UPD
    double* ash2 = ash + rpb;                                 // [rpb], only with UPD == 2
    static_assert(!RS || U == 8, "the LDS row-sum path reduces 8 rows at a time");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* tile = wsh + (1 + UPD) * rpb + wave * (8 * 72);   // [4][8*72] private row-sum tiles (RS)
    const int pg = bid % npg;
    const int rb = bid / npg;
    // Rows of this block, local index li = q U + u  ->  global row.  Interleaved (nrb_il > 0): chunk q of U rows is
    // chunk number q nrb + rb of the matrix, so the blocks that run at one time walk ONE contiguous window of X, as a
    // linear stream does (worth 2 % at 20000 x 5000, nothing at C3: the host picks).  Contiguous (nrb_il == 0): rows
    // rb rpb .. rb rpb + rpb - 1.
    auto grow = [&](int li) -> int {
        return nrb_il > 0 ? ((li / U) * nrb_il + rb) * U + (li % U) : rb * rpb + li;
    };
    const int col = (pg * 4 + wave) * PW + lane * VN;
    int xflag = 0;
    if constexpr (PK) {
        for (int l0 = (int)threadIdx.x * U; l0 < rpb; l0 += 256 * U) {
            const int g = grow(l0);
            if (g < n) xflag |= xflags[(i64)(g >> 3) * npg + pg];
        }
    }
    if (DO_Z || UPD > 0) {
        for (int i = threadIdx.x; i < rpb; i += 256) {
            const int g = grow(i);
            if constexpr (XSCALED<SX>) { if (DO_Z) wsh[i] = g < n ? wcol[g] * rscale[g] : 0.0; }
            else if (DO_Z) wsh[i] = g < n ? wcol[g] : 0.0;
            if (UPD > 0) ash[i] = g < n ? avec[g] : 0.0;
            if (UPD > 1) ash2[i] = g < n ? avec2[g] : 0.0;
        }
        if constexpr (PK) xflag = __syncthreads_or(xflag);
        else __syncthreads();
    } else if constexpr (PK) xflag = __syncthreads_or(xflag);
    const unsigned base4 = (unsigned)xbase * 0x01010101u;
    const bool ok = col < ncols;
    const bool wave_has_cols = (pg * 4 + wave) * PW < ncols;   // wave-uniform
    double tv[VN], zacc[VN], bv[VN], bv2[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) {
        zacc[e] = 0.0;
        if constexpr (XSCALED<SX>) tv[e] = (DO_Y && ok) ? trow[col + e] * cscale[col + e] : 0.0;
        else tv[e] = (DO_Y && ok) ? trow[col + e] : 0.0;
        bv[e] = (UPD > 0 && ok) ? bvec[col + e] : 0.0;
        bv2[e] = (UPD > 1 && ok) ? bvec2[col + e] - bsub2[col + e] : 0.0;
    }
    if (wave_has_cols) {
        // keep_q of the nrb row blocks, spread evenly over the launch order, are read with default-policy loads and stay in
        // the Infinity Cache from pass to pass; the others stream past it (host: pass_keep in rri_hip.hip)
        if constexpr (PK && NT) {
            // three expansions, not four: a flagged workgroup streams its fp32 rows whether its row block is a kept one or not
            const unsigned nrb = ((unsigned)gridDim.x - (unsigned)njobs) / (unsigned)npg;
            const bool kept = ((unsigned)(rb + 1) * (unsigned)keep_q) / nrb != ((unsigned)rb * (unsigned)keep_q) / nrb;
            if constexpr (PK == 2) {
                if (xflag) { RRI_PASS_ROWS(true) }
                else if (kept) { RRI_PASS_ROWS_PN(false) }
                else { RRI_PASS_ROWS_PN(true) }
            } else {
                if (xflag) { RRI_PASS_ROWS(true) }
                else if (kept) { RRI_PASS_ROWS_PK(false) }
                else { RRI_PASS_ROWS_PK(true) }
            }
        } else if constexpr (PK == 2) {
            if (xflag) { RRI_PASS_ROWS(false) }
            else { RRI_PASS_ROWS_PN(false) }
        } else if constexpr (PK) {
            if (xflag) { RRI_PASS_ROWS(false) }
            else { RRI_PASS_ROWS_PK(false) }
        } else if constexpr (NT && UPD == 0) {
            const unsigned nrb = ((unsigned)gridDim.x - (unsigned)njobs) / (unsigned)npg;
            const bool kept = ((unsigned)(rb + 1) * (unsigned)keep_q) / nrb != ((unsigned)rb * (unsigned)keep_q) / nrb;
            if (kept) { RRI_PASS_ROWS(false) }
            else { RRI_PASS_ROWS(true) }
        } else {
            RRI_PASS_ROWS(NT)
        }
        if (DO_Z && ok) {
#pragma unroll
            for (int e = 0; e < VN; ++e) {
                if constexpr (XSCALED<SX>) Zpart[(i64)rb * ldz + col + e] = zacc[e] * cscale[col + e];
                else Zpart[(i64)rb * ldz + col + e] = zacc[e];
            }
        }
    } else if (DO_Y) {
        for (int i = lane; i < rpb; i += 64) ysh[wave * rpb + i] = 0.0;
    }
    if (DO_Y) {
        __syncthreads();
        for (int i = threadIdx.x; i < rpb; i += 256) {
            const int g = grow(i);
            if constexpr (XSCALED<SX>) {
                if (g < n) Ypart[(i64)pg * n + g] = ((ysh[i] + ysh[rpb + i]) + (ysh[2 * rpb + i] + ysh[3 * rpb + i])) * rscale[g];
            } else {
                if (g < n) Ypart[(i64)pg * n + g] = (ysh[i] + ysh[rpb + i]) + (ysh[2 * rpb + i] + ysh[3 * rpb + i]);
            }
        }
    }
}

#undef RRI_PASS_ROWS
#undef RRI_PASS_ROWS_PK
#undef RRI_PASS_ROWS_PN
#undef RRI_PASS_ROW_SUMS
#undef RRI_PASS_CHUNK_SUMS

// =========================================================================================
// The two one-time kernels behind the packed copy (rri_xpack.hpp), in the geometry of the pass: a work item is one 8-row chunk
// of one column group, a wave takes one of its four 256-column panels, a lane 8 rows x 4 columns, read exactly where the fp32
// row loop reads them (rows < n, columns < ncols; everything else counts as +0).
// k_xpack_max: the largest top byte in [1, 0x7e] present in X (one integer max: *hmax, zeroed before the launch).
// k_xpack_encode: reads X once more and writes the copy; a tile with an element outside the window of *hmax gets its flag byte
// set by a plain vector store of the constant 1 (the flags were zeroed before the launch).
// =========================================================================================
__device__ __forceinline__ void xpack_load_lane(const float* __restrict__ X, i64 ldx, int n, int ncols, int q, int col,
                                                unsigned (&bits)[xpack::ROWS][xpack::COLS]) {
#pragma unroll
    for (int u = 0; u < (int)xpack::ROWS; ++u) {
        const int rr = q * (int)xpack::ROWS + u;
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (rr < n && col < ncols) v = *reinterpret_cast<const u32x4*>(X + (i64)rr * ldx + col);
        bits[u][0] = v[0]; bits[u][1] = v[1]; bits[u][2] = v[2]; bits[u][3] = v[3];
    }
}
__global__ __launch_bounds__(256) void k_xpack_max(const float* __restrict__ X, i64 ldx, int n, int ncols, int npg, i64 nitems,
                                                   unsigned* __restrict__ hmax) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned m = 0u;
    for (i64 it = blockIdx.x; it < nitems; it += gridDim.x) {
        const int q = (int)(it / npg), pg = (int)(it % npg);
        unsigned bits[xpack::ROWS][xpack::COLS];
        xpack_load_lane(X, ldx, n, ncols, q, (pg * 4 + wave) * 256 + lane * 4, bits);
#pragma unroll
        for (int u = 0; u < (int)xpack::ROWS; ++u)
#pragma unroll
            for (int e = 0; e < (int)xpack::COLS; ++e) m = max(m, xpack::window_candidate(bits[u][e]));
    }
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if (lane == 0 && m != 0u) atomicMax(hmax, m);
}
__global__ __launch_bounds__(256) void k_xpack_encode(const float* __restrict__ X, i64 ldx, int n, int ncols, int npg, i64 nitems,
                                                      const unsigned* __restrict__ hmax, unsigned char* __restrict__ XP,
                                                      unsigned char* __restrict__ xflags) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned base = xpack::base_of(*hmax);
    for (i64 it = blockIdx.x; it < nitems; it += gridDim.x) {
        const int q = (int)(it / npg), pg = (int)(it % npg);
        unsigned bits[xpack::ROWS][xpack::COLS], out[4 * xpack::SLOTS];
        xpack_load_lane(X, ldx, n, ncols, q, (pg * 4 + wave) * 256 + lane * 4, bits);
        bool bad;
        xpack::encode_lane(bits, base, out, bad);
        u32x4* rec = reinterpret_cast<u32x4*>(XP + xpack::record_offset((unsigned)q, (unsigned)(pg * 4 + wave), (unsigned)npg * 4u)) + lane;
#pragma unroll
        for (int i = 0; i < (int)xpack::SLOTS; ++i)
            rec[i * (int)xpack::LANES] = u32x4{out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]};
        if (bad) xflags[it] = 1;
    }
}

// The one-time kernels behind the 26-bit copy (rri_xnarrow.hpp), in the same geometry, three reads of X in all.
// k_xnarrow_hist: k_xpack_max's pass, which also counts the exponent byte of every element of X of sign 0 (hist[256], zeroed
// before the launch; padding is not counted): the host picks the books from it.
// k_xnarrow_encode<false>: the tile flags of the 28-bit format, computed as k_xpack_encode computes them (an element in neither
// book flags its tile too; the books hold the whole window, so there is none), and the number of exception entries of every record.
// k_xnarrow_encode<true>: writes the fixed parts, and every record's entries where the directory (the host's prefix sum of the
// counts) puts them, lane after lane.
__global__ __launch_bounds__(256) void k_xnarrow_hist(const float* __restrict__ X, i64 ldx, int n, int ncols, int npg, i64 nitems,
                                                      unsigned* __restrict__ hmax, unsigned long long* __restrict__ hist) {
    __shared__ unsigned long long h[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    h[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned m = 0u;
    for (i64 it = blockIdx.x; it < nitems; it += gridDim.x) {
        const int q = (int)(it / npg), pg = (int)(it % npg);
        const int col = (pg * 4 + wave) * 256 + lane * 4;
        unsigned bits[xpack::ROWS][xpack::COLS];
        xpack_load_lane(X, ldx, n, ncols, q, col, bits);
#pragma unroll
        for (int u = 0; u < (int)xpack::ROWS; ++u)
#pragma unroll
            for (int e = 0; e < (int)xpack::COLS; ++e) {
                m = max(m, xpack::window_candidate(bits[u][e]));
                if (q * (int)xpack::ROWS + u < n && col < ncols && !(bits[u][e] >> 31)) atomicAdd(&h[bits[u][e] >> 23], 1ull);
            }
    }
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    if (lane == 0 && m != 0u) atomicMax(hmax, m);
    __syncthreads();
    if (h[threadIdx.x] != 0ull) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
template <bool WRITE>
__global__ __launch_bounds__(256) void k_xnarrow_encode(const float* __restrict__ X, i64 ldx, int n, int ncols, int npg, i64 nitems,
                                                        unsigned base, const unsigned char* __restrict__ cls,
                                                        unsigned char* __restrict__ XN, unsigned char* __restrict__ xflags,
                                                        unsigned* __restrict__ counts, const unsigned* __restrict__ dir,
                                                        unsigned short* __restrict__ exc) {
    __shared__ unsigned char scls[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    scls[threadIdx.x] = cls[threadIdx.x];
    __syncthreads();
    for (i64 it = blockIdx.x; it < nitems; it += gridDim.x) {
        const int q = (int)(it / npg), pg = (int)(it % npg);
        const int col = (pg * 4 + wave) * 256 + lane * 4;
        unsigned bits[xpack::ROWS][xpack::COLS], out[xnarrow::LANE_DWORDS];
        xpack_load_lane(X, ldx, n, ncols, q, col, bits);
        const unsigned rows_valid = col < ncols ? (unsigned)min(n - q * (int)xpack::ROWS, (int)xpack::ROWS) : 0u;
        const unsigned long long ri = xnarrow::record_index((unsigned)q, (unsigned)(pg * 4 + wave), (unsigned)npg * 4u);
        unsigned nexc;
        bool neither;
        xnarrow::encode_lane(bits, rows_valid, scls, (unsigned)lane, out, nullptr, nexc, neither);
        unsigned upto = nexc;           // the entries of lanes 0 .. lane
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = (unsigned)__shfl_up((int)upto, off);
            if (lane >= off) upto += o;
        }
        if constexpr (!WRITE) {
            bool bad = neither;
#pragma unroll
            for (int u = 0; u < (int)xpack::ROWS; ++u)
#pragma unroll
                for (int e = 0; e < (int)xpack::COLS; ++e) bad = bad || !xpack::in_window(bits[u][e], base);
            if (bad) xflags[it] = 1;
            if (lane == 63) counts[ri] = upto;
        } else {
            xnarrow::encode_lane(bits, rows_valid, scls, (unsigned)lane, out, exc + ((size_t)dir[ri] + (upto - nexc)), nexc, neither);
            unsigned char* rec = XN + ri * xnarrow::RECORD_BYTES;
#pragma unroll
            for (int i = 0; i < (int)xnarrow::WIDE_SLOTS; ++i)
                reinterpret_cast<u32x4*>(rec)[i * (int)xnarrow::LANES + lane] = u32x4{out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]};
            reinterpret_cast<u32x2*>(rec + xnarrow::dword_offset(24u, 0u))[lane] = u32x2{out[24], out[25]};
        }
    }
}

// =========================================================================================
// k_colsums: column sums of X against NV row-vectors at once (X^T Q for the randomized SVD behind NNDSVD,
// initialization.py:105): the geometry of k_pass -- 4 waves = 4 adjacent 1 KiB panels x a row block, 4 rows in
// flight -- with NV accumulator sets per lane, so X is read once per NV vectors instead of once per vector.
// Qt: the vectors as rows (NV x n, stride ldq).  Zmulti[v][row block][column], stride ldz.
// =========================================================================================
template <typename SX, int NV>
__global__ __launch_bounds__(256) void k_colsums(const SX* __restrict__ X, i64 ldx, int n, int ncols,
                                                 const double* __restrict__ Qt, i64 ldq, int nv,
                                                 double* __restrict__ Zmulti, i64 ldz, int rpb, int npg, int nrb,
                                                 const XScale xs) {
    typedef XVec<SX> XV;
    typedef typename XV::type V;
    constexpr int VN = XV::N;
    constexpr int PW = 64 * VN;
    constexpr int U = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* wsh = reinterpret_cast<double*>(smem);   // [NV][rpb]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pg = blockIdx.x % npg, rb = blockIdx.x / npg;
    const int row0 = rb * rpb, row1 = min(n, row0 + rpb);
    const int col = (pg * 4 + wave) * PW + lane * VN;
    for (int i = threadIdx.x; i < (row1 - row0) * NV; i += 256) {
        const int v = i / (row1 - row0), r = i - v * (row1 - row0);
        if constexpr (XSCALED<SX>) wsh[v * rpb + r] = v < nv ? Qt[(i64)v * ldq + row0 + r] * xs.row[row0 + r] : 0.0;
        else wsh[v * rpb + r] = v < nv ? Qt[(i64)v * ldq + row0 + r] : 0.0;
    }
    __syncthreads();
    if ((pg * 4 + wave) * PW >= ncols) return;       // wave-uniform
    const bool ok = col < ncols;
    double acc[NV][VN];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int e = 0; e < VN; ++e) acc[v][e] = 0.0;
    for (int r = row0; r < row1; r += U) {
        V x[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            x[u] = (r + u < row1 && ok) ? stream_load<true>(reinterpret_cast<const V*>(X + (i64)(r + u) * ldx + col)) : XV::zero();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (r + u >= row1) break;
            double xe[VN];
            XV::unpack(x[u], xe);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const double wv = wsh[v * rpb + r + u - row0];
#pragma unroll
                for (int e = 0; e < VN; ++e) acc[v][e] = fma(wv, xe[e], acc[v][e]);
            }
        }
    }
    if (ok) {
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int e = 0; e < VN; ++e) {
                if constexpr (XSCALED<SX>) Zmulti[((i64)v * nrb + rb) * ldz + col + e] = acc[v][e] * xs.col[col + e];
                else Zmulti[((i64)v * nrb + rb) * ldz + col + e] = acc[v][e];
            }
    }
}

// =========================================================================================
// Preprocessing of the resident X (matrixops.py:124-179: tf-idf and row normalisation), SURVEY 8f rank 3.
//   k_col_count  df_j = #{i : X_ij > 0}, geometry of k_colsums (partials per row block, k_reduce adds them)
//   k_row_inverse  xs_i = sum of the row-dot panels + spacing(1); inv_i = 1 / xs_i; rows with xs_i < 1e-10 are flagged
//                  (inv_i = -1): they become uniform 1/d (normalize's zero_sum_fix)
//   k_scale2d    X_ij <- (X_ij * s_j) * inv_i in place, one linear stream (the fastest read-modify-write pattern)
// =========================================================================================
template <typename SX>
__global__ __launch_bounds__(256) void k_col_count(const SX* __restrict__ X, i64 ldx, int n, int ncols,
                                                   double* __restrict__ Zpart, i64 ldz, int rpb, int npg) {
    typedef XVec<SX> XV;
    typedef typename XV::type V;
    constexpr int VN = XV::N;
    constexpr int PW = 64 * VN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pg = blockIdx.x % npg, rb = blockIdx.x / npg;
    const int row0 = rb * rpb, row1 = min(n, row0 + rpb);
    const int col = (pg * 4 + wave) * PW + lane * VN;
    if (col >= ncols) return;
    double acc[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[e] = 0.0;
    for (int r = row0; r < row1; r += 4) {
        V x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            x[u] = (r + u < row1) ? stream_load<true>(reinterpret_cast<const V*>(X + (i64)(r + u) * ldx + col)) : XV::zero();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            double xe[VN];
            XV::unpack(x[u], xe);
#pragma unroll
            for (int e = 0; e < VN; ++e) acc[e] += xe[e] > 0.0 ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int e = 0; e < VN; ++e) Zpart[(i64)rb * ldz + col + e] = acc[e];
}

__global__ __launch_bounds__(256) void k_row_inverse(const double* __restrict__ Ypart, int npanels, int n,
                                                     double* __restrict__ inv) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double xs = 0.0;
    xs = ordered_sum<8>(Ypart + i, n, 0, npanels, 1);
    xs += 2.220446049250313e-16;                      // np.spacing(1), matrixops.py:140
    inv[i] = xs < 1e-10 ? -1.0 : 1.0 / xs;
}

template <typename SX>
__global__ __launch_bounds__(256) void k_scale2d(SX* __restrict__ X, i64 ldx, i64 n, int d, const double* __restrict__ s,
                                                 const double* __restrict__ inv) {
    typedef XVec<SX> XV;
    typedef typename XV::type V;
    constexpr int VN = XV::N;
    const i64 vpr = ldx / VN, total = n * vpr;         // ldx is a multiple of the vector width
    const double uniform = 1.0 / (double)d;
    for (i64 v = (i64)blockIdx.x * 256 + threadIdx.x; v < total; v += (i64)gridDim.x * 256) {
        const i64 i = v / vpr;
        const int j = (int)(v - i * vpr) * VN;
        V* p = reinterpret_cast<V*>(X + i * ldx + j);
        double xe[VN];
        XV::unpack(__builtin_nontemporal_load(p), xe);
        const double r = inv ? inv[i] : 1.0;
#pragma unroll
        for (int e = 0; e < VN; ++e) {
            if (j + e >= d) { xe[e] = 0.0; continue; }                       // pad columns stay zero
            const double t = s ? xe[e] * s[j + e] : xe[e];                    // X * idf               (:172)
            xe[e] = r < 0.0 ? uniform : r * t;                                // d * X, or the zero-sum fix (:143-147)
        }
        __builtin_nontemporal_store(XV::pack(xe), p);
    }
}

// =========================================================================================
// W is stored k-major on the device (Wt: k x ldw, ldw >= n): column t of W is the contiguous
// row Wt[t,:], so the pass reads the active column coalesced and k_wcol needs no LDS staging.
//
// k_wcol: W-column update of topic t (UPDATE) and the Gram row w_tn^T W / ||w_tn||^2 of the NEXT
// topic tn (CARRY), one thread per row of W.  Gpart[b][0..k) = sum_i wn_i W[i,:], [k] = sum wn_i^2,
// [k+1] = sum_i W[i,t] (new).  T T[t]^T arrives as nsplit partial vectors from k_tgram.
// =========================================================================================
// (WCOL_TILES, the 64-row tiles per k_wcol block, and GRAM_SLICES, the slices k_reduce sums the Gpart rows in: rri_layout.hpp)

template <bool UPDATE, bool CARRY>
__global__ __launch_bounds__(256) void k_wcol(double* __restrict__ Wt, i64 ldw, int n, int k, int t, int tn,
                                              const double* __restrict__ Ypart, int npanels,
                                              const double* __restrict__ Ttpart, int nsplit,
                                              double* __restrict__ Gpart, double* __restrict__ xyp, int sweep,
                                              KParams p, DevState* st) {
    // Block = TILES tiles of 64 rows of W (lane = row); its 4 waves split the k columns (wave w takes
    // l = w, w+4, ...): four times the waves of a row-per-thread layout, dependent chains a quarter as
    // long.  Gram partials of the tiles add up in LDS (one owner wave per column: fixed order).
    if (st->halt) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* tts = reinterpret_cast<double*>(smem);   // [k]
    double* gsh = tts + k;                           // [k+2] Gram partial of the block
    double* dsh = gsh + k + 2;                       // [4][64] partial W.Tt per wave
    double* wsh = dsh + 256;                         // [64] new column entries
    double cden = 0.0;
    int mode = 0;
    // (requesting the first tile's operands before the reduction of T T[t]^T below, so that the two round trips to L2
    // overlap, was tried: +48 VGPRs, 3 instead of 4 waves per SIMD, 18.5 -> 24.8 us at C3 and no gain at 10000 x 1000)
    for (int l = tid; l < k + 2; l += 256) gsh[l] = 0.0;
    if (UPDATE) {
        for (int l = tid; l < k; l += 256) {
            tts[l] = ordered_sum<8>(Ttpart + l, k, 0, nsplit, 1);                               // entry t holds ||T[t,:]||^2 until zeroed below
        }
        __syncthreads();
        cden = tts[t] + p.reg_w_l2;                   // denom = nt + reg_w_l2 (nmf.py:465)
        __syncthreads();
        if (tid == 0) tts[t] = 0.0;                   // Tt[t] = 0 (nmf.py:732)
        mode = wcol_denominator_mode(cden, p);        // scalar c<=0 with s=None (optimization.py:60-67): entries at ub, or unbounded
        if (mode < 0) {
            if (blockIdx.x == 0 && tid == 0) halt_set(st, mode, t, sweep, t);
            return;
        }
    }
    __syncthreads();
    constexpr int CH = 16;   // columns per batch of loads per wave (all of a wave's columns when k <= 64)
    constexpr int TILES = WCOL_TILES;
    for (int tile = 0; tile < TILES; ++tile) {
        const i64 i = ((i64)blockIdx.x * TILES + tile) * 64 + lane;
        if (((i64)blockIdx.x * TILES + tile) * 64 >= n) break;   // block-uniform
        const bool valid = i < n;
        const double wn = (CARRY && valid) ? Wt[(i64)tn * ldw + i] : 0.0;
        double y = 0.0;
        if (UPDATE && wave == 0 && valid) y = ordered_sum<8>(Ypart + i, n, 0, npanels, 1);
        double dotv = 0.0;
        for (int l0 = wave; l0 < k; l0 += 4 * CH) {
            double wl[CH];
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int l = l0 + 4 * q;
                wl[q] = (l < k && valid && !(UPDATE && l == t)) ? Wt[(i64)l * ldw + i] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < CH; ++q) {
                const int l = l0 + 4 * q;
                if (l < k) {   // wave-uniform
                    if (UPDATE) dotv = fma(wl[q], tts[l], dotv);
                    if (CARRY && !(UPDATE && l == t)) {
                        const double g = wave_sum<double>(wn * wl[q]);
                        if (lane == 0) gsh[l] += g;   // column l belongs to this wave alone
                    }
                }
            }
        }
        double wnew = 0.0;
        if (UPDATE) {
            dsh[wave * 64 + lane] = dotv;
            __syncthreads();
            if (wave == 0) {
                const double dot = (dsh[lane] + dsh[64 + lane]) + (dsh[128 + lane] + dsh[192 + lane]);
                if (valid) {
                    const double numer = (y - dot) - p.reg_w_l1;
                    if (mode == 0) wnew = fmax(numer, 0.0) / (cden + p.eps);
                    else wnew = (-numer + cden < 0.0) ? p.w_row_sum : 0.0;
                    Wt[(i64)t * ldw + i] = wnew;
                }
                wsh[lane] = wnew;
            }
            __syncthreads();
            wnew = wsh[lane];
        }
        if (wave == 0) {
            const double nwp = wave_sum<double>(wn * wn);
            const double swp = wave_sum<double>(wnew);
            if (lane == 0) { gsh[k] += nwp; gsh[k + 1] += swp; }
            if (UPDATE) {   // <w_t, X t_t> of this block's rows: the cross term of the objective, for free
                const double xy = wave_sum<double>(wnew * y);
                if (lane == 0) xyp[(i64)blockIdx.x * TILES + tile] = xy;
            }
        } else if (wave == 1 && UPDATE && CARRY) {
            const double gt = wave_sum<double>(wn * wnew);   // Gram entry against the NEW column t
            if (lane == 0) gsh[t] += gt;
        }
        if (UPDATE) __syncthreads();   // dsh / wsh are reused by the next tile
    }
    __syncthreads();
    double* gp = Gpart + (i64)blockIdx.x * (k + 2);
    for (int l = tid; l < k + 2; l += 256) gp[l] = gsh[l];
}

// =========================================================================================
// k_wsweep_rows: the W half of EVERY topic of a sweep in one launch, for runs with T fixed (the fold-in of new rows,
// sklearn_interface.py:327-333; the w_row refit, nmf.py:531-539).  With T fixed the update of W[i, t] (nmf.py:464-469, 728-734)
//     numer = (X T^T)[i, t] - sum_{l != t} W[i, l] (T T^T)[l, t] - reg_w_l1 ,   denom = ||T[t,:]||^2 + reg_w_l2
// involves row i of W alone: Q = X T^T (k_xtt_mfma) and G = T T^T (k_gram) are constants of the run, taken once per T, and a lane
// walks the k topics of its row with the row and G in LDS -- k^2 fused multiply-adds per row, no pass over X, one launch where
// the launch-per-topic schedule takes three per topic (k_tgram, k_wcol, k_check_wcol).  Same branches of qf_min as k_wcol.
// What couples the rows is the column check after every update (nmf.py:471-476, 793-816): the kernel leaves the column sums as
// one partial per workgroup and topic, k_wsweep_verdict takes the verdicts in topic order after the launch, and when a
// column asks for a reset at topic t* (rare), k_wsweep_repair puts the columns after t* back to what they were before the
// sweep (Wprev, written here on the way in): the state in which the launch-per-topic schedule halts.  The cross terms
// <w_t, X t_t> of the objective go to xyp as k_wcol leaves them (one partial per 64 rows).
// =========================================================================================
// Four topics at a time: the terms of the four dots that come from columns OUTSIDE the block share one read of W[i, l] and two
// 16-byte reads of G[l, t .. t+3] (three LDS reads for four multiply-adds where a topic on its own takes eight); the six terms
// inside the block follow in registers, topic by topic.  (X T^T)[i, t .. t+3] of the NEXT block is requested before this one is
// worked on.  A dot is therefore summed as (columns before the block, ascending) + (columns after it) + (the block's others).
__host__ __device__ constexpr int wsweep_kp(int k) { return (k + 3) & ~3; }
__host__ __device__ constexpr size_t wsweep_lds_bytes(int k) { return ((size_t)k * wsweep_kp(k) + 64 * (size_t)k) * sizeof(double); }

__global__ __launch_bounds__(64) void k_wsweep_rows(double* __restrict__ Wt, double* __restrict__ Wprev, i64 ldw, int n, int k,
                                                    int t0, const double* __restrict__ Qt, const double* __restrict__ G,
                                                    double* __restrict__ colsum, int nwb, double* __restrict__ xyp,
                                                    i64 xy_stride, KParams p, const DevState* __restrict__ st) {
    if (st->halt) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int kp = wsweep_kp(k);
    double* gsh = reinterpret_cast<double*>(smem);   // [k][kp]  (symmetric to the bit: k_gram writes both halves from one sum)
    double* wsh = gsh + (size_t)k * kp;              // [k][64] the rows' entries of W, current
    const int lane = threadIdx.x;
    const i64 i = (i64)blockIdx.x * 64 + lane;
    const bool valid = i < n;
    for (int q = lane; q < k * kp; q += 64) {
        const int l = q / kp, c = q - l * kp;
        gsh[q] = c < k ? G[(i64)l * k + c] : 0.0;
    }
    constexpr int CH = 8;
    for (int l0 = 0; l0 < k; l0 += CH) {
        double wv[CH];
#pragma unroll
        for (int q = 0; q < CH; ++q) wv[q] = (l0 + q < k && valid) ? Wt[(i64)(l0 + q) * ldw + i] : 0.0;
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            const int l = l0 + q;
            if (l < k) {
                wsh[l * 64 + lane] = wv[q];
                if (valid) Wprev[(i64)l * ldw + i] = wv[q];
            }
        }
    }
    const int tb0 = t0 & ~3;
    double yv[4], yn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) yv[j] = (tb0 + j < k && valid) ? Qt[(i64)(tb0 + j) * ldw + i] : 0.0;
    __syncthreads();
    for (int tb = tb0; tb < k; tb += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) yn[j] = (tb + 4 + j < k && valid) ? Qt[(i64)(tb + 4 + j) * ldw + i] : 0.0;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        auto outside = [&](int la, int lb) {
#pragma unroll 4
            for (int l = la; l < lb; ++l) {
                const double wl = wsh[l * 64 + lane];
                const f64x2 g01 = *reinterpret_cast<const f64x2*>(gsh + (size_t)l * kp + tb);
                const f64x2 g23 = *reinterpret_cast<const f64x2*>(gsh + (size_t)l * kp + tb + 2);
                acc[0] = fma(wl, g01[0], acc[0]);
                acc[1] = fma(wl, g01[1], acc[1]);
                acc[2] = fma(wl, g23[0], acc[2]);
                acc[3] = fma(wl, g23[1], acc[3]);
            }
        };
        outside(0, tb);
        outside(min(tb + 4, k), k);
        double wb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wb[j] = tb + j < k ? wsh[(tb + j) * 64 + lane] : 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = tb + j;
            if (t >= k || t < t0) continue;           // (wave-uniform)
            const double* gr = gsh + (size_t)t * kp;
            const double cden = gr[t] + p.reg_w_l2;   // denom = nt + reg_w_l2 (nmf.py:465)
            const int mode = wcol_denominator_mode(cden, p);   // scalar c <= 0 with s = None (optimization.py:60-67): entries at ub, or
            if (mode < 0) continue;                   // unbounded -- k_wsweep_verdict reports it at this topic; the column stays
            double dot = acc[j];
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2)
                if (j2 != j && tb + j2 < k) dot = fma(wb[j2], gr[tb + j2], dot);     // Tt[t] = 0 (nmf.py:732): j2 == j left out
            const double y = yv[j];
            const double numer = (y - dot) - p.reg_w_l1;
            double wnew = 0.0;
            if (valid) {
                if (mode == 0) wnew = fmax(numer, 0.0) / (cden + p.eps);
                else wnew = (-numer + cden < 0.0) ? p.w_row_sum : 0.0;
                Wt[(i64)t * ldw + i] = wnew;
            }
            wb[j] = wnew;
            wsh[t * 64 + lane] = wnew;
            const double sw = wave_sum<double>(wnew);
            const double xy = wave_sum<double>(wnew * y);
            if (lane == 0) {
                colsum[(i64)t * nwb + blockIdx.x] = sw;
                xyp[(i64)t * xy_stride + blockIdx.x] = xy;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) yv[j] = yn[j];
    }
}

// the column checks of a k_wsweep_rows launch, in topic order: stage bit 0 -- sums[t] = sum over the workgroups' partials (a
// wave per topic, fixed order); bit 1 -- the verdicts on sums (row-sharded runs all-reduce sums in between), those of k_wcol
// (unbounded: a non-positive denominator with no bound to jump to) and k_check_wcol, halting at the FIRST topic that fails
// with the position the launch-per-topic schedule reports.  A reset event also leaves pad0 = t* + 1 for k_wsweep_repair.
__global__ __launch_bounds__(1024) void k_wsweep_verdict(const double* __restrict__ colsum, int nwb, double* __restrict__ sums,
                                                         const double* __restrict__ G, int k, int t0, int sweep, int stage,
                                                         KParams p, DevState* st) {
    if (st->halt) return;
    __shared__ double ssum[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (stage & 1) {
        for (int t = t0 + wave; t < k; t += 16) {
            double a = ordered_sum<8>(colsum + (i64)t * nwb, 1, lane, nwb, 64);
            a = wave_sum<double>(a);
            if (lane == 0) { sums[t] = a; ssum[t] = a; }
        }
    }
    if (!(stage & 2)) return;
    if (!(stage & 1))
        for (int t = t0 + (int)threadIdx.x; t < k; t += 1024) ssum[t] = sums[t];
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int t = t0; t < k; ++t) {
        const double cden = G[(i64)t * k + t] + p.reg_w_l2;
        const int mode = wcol_denominator_mode(cden, p);
        if (mode < 0) {
            halt_set(st, mode, t, sweep, t);
            return;
        }
        const int code = wcol_code(ssum[t], p);
        if (code != 0) {
            const StepPos next = next_step(sweep, t, k);         // where a resumed run continues
            halt_set(st, code, t, next.sweep, next.pos);
            if (code == HALT_EVENT_RESET_W) st->pad0 = t + 1;
            return;
        }
    }
}

// after a reset event of k_wsweep_verdict at topic t*: columns t* + 1 .. k - 1 of W as they were before the sweep
__global__ __launch_bounds__(256) void k_wsweep_repair(double* __restrict__ Wt, const double* __restrict__ Wprev, i64 ldw, int n,
                                                       int k, const DevState* __restrict__ st) {
    const int from = st->pad0;
    if (from <= 0 || st->halt != HALT_EVENT_RESET_W) return;
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    for (int l = from; l < k; ++l) Wt[(i64)l * ldw + i] = Wprev[(i64)l * ldw + i];
}

// =========================================================================================
// k_wcol_resid: W-column update of topic t in the explicit-residual schedule ("explicit-residual variant"):
//     numer_W = R t' + w_t ||t'||^2 - reg_w_l1      (R: the stored residual, which already contains w_t t'^T)
// y = R t' arrives as the row-dot panels of the pass; the new column goes to Wt[t,:], dw = new - old stays in `dw`
// as the row factor of the rank-one term  - dw t'^T  that the NEXT pass folds into R.  One thread per row.
// Gpart[b] (k+2 entries per block of 256 rows): [t] = <dw, w_tn> -- the coefficient with which that pending term enters
// the column sums of the next topic tn --, [k] = ||w_tn||^2, [k+1] = sum of the new column, every other entry 0.
// UPDATE = false (prologue): only [k] = ||w_tn||^2.
// =========================================================================================
template <bool UPDATE>
__global__ __launch_bounds__(256) void k_wcol_resid(double* __restrict__ Wt, i64 ldw, int n, int k, int t, int tn,
                                                    const double* __restrict__ Ypart, int npanels,
                                                    const double* __restrict__ Ttpart, int nsplit,
                                                    double* __restrict__ dw, double* __restrict__ Gpart, int sweep,
                                                    KParams p, DevState* st) {
    if (st->halt) return;
    __shared__ double scratch[40];
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    double cden = 1.0, nt = 0.0;
    int mode = 0;
    if (UPDATE) {
        nt = ordered_sum<8>(Ttpart + t, k, 0, nsplit, 1);      // ||T[t,:]||^2 from the slices of k_tgram
        cden = nt + p.reg_w_l2;                                // denom = nt + reg_w_l2 (nmf.py:465)
        mode = wcol_denominator_mode(cden, p);                 // optimization.py:60-67
        if (mode < 0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) halt_set(st, mode, t, sweep, t);
            return;
        }
    }
    double wnew = 0.0, dwi = 0.0, wn = 0.0;
    if (i < n) {
        if (UPDATE) {
            const double y = ordered_sum<8>(Ypart + i, n, 0, npanels, 1);
            const double w0 = Wt[(i64)t * ldw + i];
            const double numer = fma(w0, nt, y) - p.reg_w_l1;
            if (mode == 0) wnew = fmax(numer, 0.0) / (cden + p.eps);
            else wnew = (-numer + cden < 0.0) ? p.w_row_sum : 0.0;
            Wt[(i64)t * ldw + i] = wnew;
            dwi = wnew - w0;
            dw[i] = dwi;
        }
        wn = (UPDATE && tn == t) ? wnew : Wt[(i64)tn * ldw + i];
    }
    const double g = block_sum(wn * dwi, scratch);
    const double nwp = block_sum(wn * wn, scratch);
    const double sw = block_sum(wnew, scratch);
    double* gp = Gpart + (i64)blockIdx.x * (k + 2);
    for (int l = threadIdx.x; l < k + 2; l += 256) gp[l] = (l == t && UPDATE) ? g : (l == k ? nwp : (l == k + 1 ? sw : 0.0));
}

// =========================================================================================
// k_reduce: fixed-order reduction of the row-block partials into the reduce buffer
//   red[0..ldz) = w^T X ; red[ldz + g*(k+2) + ...), g < GRAM_SLICES: slice sums of [w^T W | ||w||^2 | sum W[:,tprev]]
// (in the row-sharded multi-GPU run this buffer is what the ranks all-reduce).
// 1024 threads: column blocks take 32 columns x 32 row-block groups, the last block the Gram row.
// =========================================================================================
// one workgroup (1024 threads) of the reduction: block bx of nb; the last GRAM_SLICES take the Gram row (none when Gpart == NULL)
__device__ __forceinline__ void reduce_block(int bx, int nb, const double* __restrict__ Zpart, i64 ldz, int nrb,
                                             const double* __restrict__ Gpart, int nwb, int k, double* __restrict__ red,
                                             double* sh) {
    const int tid = threadIdx.x;
    // Gpart == NULL: column blocks only (the grid then has no Gram blocks)
    const int ngram = Gpart ? GRAM_SLICES : 0;
    const int nzb = nb - ngram;
    if (bx < nzb) {
        const int c = tid & 31, g = tid >> 5;
        const i64 j = (i64)bx * 32 + c;
        double a = 0.0;
        if (j < ldz) a = ordered_sum<8>(Zpart + j, ldz, g, nrb, 32);
        sh[g * 33 + c] = a;
        __syncthreads();
        if (tid < 32 && j < ldz) {   // here c == tid
            double s = 0.0;
            for (int q = 0; q < 32; ++q) s += sh[q * 33 + tid];
            red[j] = s;
        }
    } else {
        // Gram slice gs: rows [b0, b1) of Gpart, 16 waves striding over them, lanes over the k+2 entries
        const int gs = bx - nzb;
        const int per = (nwb + GRAM_SLICES - 1) / GRAM_SLICES;
        const int b0 = gs * per, b1 = min(nwb, b0 + per);
        const int lane = tid & 63, wave = tid >> 6;  // 16 waves
        for (int l0 = 0; l0 < k + 2; l0 += 64) {
            const int l = l0 + lane;
            double a = 0.0;
            if (l < k + 2) a = ordered_sum<8>(Gpart + l, k + 2, b0 + wave, b1, 16);
            __syncthreads();
            sh[wave * 64 + lane] = a;
            __syncthreads();
            if (wave == 0 && l < k + 2) {
                double s = 0.0;
                for (int q = 0; q < 16; ++q) s += sh[q * 64 + lane];
                red[ldz + (i64)gs * (k + 2) + l] = s;
            }
        }
    }
}
__global__ __launch_bounds__(1024) void k_reduce(const double* __restrict__ Zpart, i64 ldz, int nrb,
                                                 const double* __restrict__ Gpart, int nwb, int k,
                                                 double* __restrict__ red, const DevState* __restrict__ st) {
    if (st->halt) return;
    __shared__ double sh[32 * 33];
    reduce_block((int)blockIdx.x, (int)gridDim.x, Zpart, ldz, nrb, Gpart, nwb, k, red, sh);
}

// =========================================================================================
// k_wfin: the one launch between the fused pass of step t and the T-row update of topic tn on the early-sums schedule.
// Everything it reads the pass's grid left behind.  1024 threads; the first `nredb` workgroups are k_reduce's (the column sums
// of Zpart in its order; the Gram slices over the early job's Gpart rows), the others take 16 tiles of 64 rows each, one per
// wave: y from Ypart in k_wcol's order, numer = (y - dot) - reg with k_wcol's branches of qf_min and its halt, W[:,t], and per
// tile <w_tn, w_t'> and sum w_t' (wfp[0][tile], wfp[1][tile]: two dense vectors, which k_trow_early reads coalesced; the column
// sum also as entry k + 1 of row `tile` of Gtile, where k_check_wcol looks for it) and <w_t', y> (xyp, one per 64 rows as k_wcol
// leaves them).
// =========================================================================================
__global__ __launch_bounds__(1024) void k_wfin(double* __restrict__ Wt, i64 ldw, int n, int k, int t, int tn,
                                               const double* __restrict__ Ypart, int npanels,
                                               const double* __restrict__ dot, const double* __restrict__ nt,
                                               double* __restrict__ Gtile, double* __restrict__ wfp, int ntiles,
                                               double* __restrict__ xyp, const double* __restrict__ Zpart, i64 ldz, int nrb,
                                               const double* __restrict__ Gearly, int ne, double* __restrict__ red,
                                               int nredb, int sweep, KParams p, DevState* st) {
    static_assert(WFIN_TILES == 16 && WCOL_TILES == 1, "a wave per tile, a row of Gtile and an entry of xyp per tile");
    __shared__ double sh[32 * 33];
    if ((int)blockIdx.x < nredb) {
        if (st->halt) return;
        reduce_block((int)blockIdx.x, nredb, Zpart, ldz, nrb, Gearly, ne, k, red, sh);
        return;
    }
    const int b = (int)blockIdx.x - nredb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 tile = (i64)b * 16 + wave;
    const i64 i = tile * 64 + lane;
    const bool valid = i < n;
    // Every load of a tile wave in ONE round trip: none of the addresses depends on a loaded value, so the halt word, nt[0], the
    // row's wn and dot and its first WFIN_YB partials of y are issued before the first wait and the branches come behind them (a
    // wave that returns has asked for values it never uses; load_here, because the compiler sinks plain loads under the branches,
    // four round trips in a row).  Rows past n read row n - 1, partials past npanels the last one, and neither enters a sum:
    // the terms of y are added in ordered_sum<8>'s order, zeros where it adds zeros.
    constexpr int WFIN_YB = 16;
    const i64 ic = valid ? i : (i64)n - 1;
    const int halted = load_here(&st->halt);
    const double nt0 = load_here(nt);
    const double wnl = load_here(Wt + (i64)tn * ldw + ic);
    const double dtl = load_here(dot + ic);
    double yv[WFIN_YB];
#pragma unroll
    for (int q = 0; q < WFIN_YB; ++q) yv[q] = load_here(Ypart + (i64)min(q, npanels - 1) * n + ic);
    __builtin_amdgcn_sched_barrier(0);                  // the first use (and its wait) behind the last load, not among them
    if (__builtin_amdgcn_readfirstlane(halted)) return;
    const double cden = nt0 + p.reg_w_l2;               // denom = nt + reg_w_l2 (nmf.py:465)
    const int mode = wcol_denominator_mode(cden, p);
    if (mode < 0) {
        if (b == 0 && threadIdx.x == 0) halt_set(st, mode, t, sweep, t);
        return;
    }
    if (tile * 64 >= n) return;                         // wave-uniform; no barrier follows
    double wn = 0.0, y = 0.0, wnew = 0.0;
    if (valid) {
        wn = wnl;
        const double dt = dtl;
#pragma unroll
        for (int q = 0; q < WFIN_YB; ++q) y += q < npanels ? yv[q] : 0.0;
        if (npanels > WFIN_YB) y = ordered_sum_acc<8>(y, Ypart + i, n, WFIN_YB, npanels, 1);
        const double numer = (y - dt) - p.reg_w_l1;
        if (mode == 0) wnew = fmax(numer, 0.0) / (cden + p.eps);
        else wnew = (-numer + cden < 0.0) ? p.w_row_sum : 0.0;
        Wt[(i64)t * ldw + i] = wnew;
    }
    const double swp = wave_sum<double>(wnew);
    const double xy = wave_sum<double>(wnew * y);
    const double gt = wave_sum<double>(wn * wnew);      // Gram entry against the NEW column t
    if (lane == 0) {
        wfp[tile] = gt;
        wfp[ntiles + tile] = swp;
        Gtile[tile * (k + 2) + k + 1] = swp;
        xyp[tile] = xy;
    }
}

// red[ldz + g*(k+2) + l], g < GRAM_SLICES -> entry l of [w^T W | ||w||^2 | sum W[:,tprev]]
__device__ __forceinline__ double red_gram(const double* __restrict__ red, i64 ldz, int k, int l) {
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < GRAM_SLICES; ++g) s += red[ldz + (i64)g * (k + 2) + l];
    return s;
}

// =========================================================================================
// k_trow_numer: numerator of the T-row update and the closed-form minimiser (before any
// simplex projection).  Also evaluates the pending W-column check of the previous topic
// (_check_reset_W + assert, nmf.py:471-476) from the reduced column sum.  When no projection
// follows, the new row is written straight into T.  blockDim = 128.
// =========================================================================================
__global__ __launch_bounds__(128) void k_trow_numer(double* __restrict__ T, i64 ldt, int d, int k, int t,
                                                    const double* __restrict__ red, i64 ldz,
                                                    double* __restrict__ xraw, double* __restrict__ tpart,
                                                    i64* __restrict__ tpart_idx, int check_prev, int tprev,
                                                    int sweep, KParams p, DevState* st, int resid_form,
                                                    double* __restrict__ told) {
    // resid_form (explicit-residual schedule): red[0..d) = R^T w_t over the stored residual, the Gram part holds the
    // coefficient of the one pending rank-one term (slot tprev: <dw_tprev, w_t>) and zeros; the topic's own term
    // comes back as + ||w_t||^2 T[t,:]  (numer_T = R^T w + t ||w||^2).  told: the row before its update.
    if (st->halt) return;
    const int tid = threadIdx.x;
    __shared__ double scratch[40];
    __shared__ double gsh[RRI_MAX_K];
    const double nw = red_gram(red, ldz, k, k);
    if (check_prev) {
        const int code = wcol_code(red_gram(red, ldz, k, k + 1), p);
        if (code != 0) {
            if (blockIdx.x == 0 && tid == 0) halt_set(st, code, tprev, sweep, t);
            return;
        }
    }
    const double c = nw + p.reg_t_l2;  // denom = nw + reg_t_l2 (nmf.py:438)
    const bool project = p.project_T && p.has_trs;
    const int mode = trow_denominator_mode(c, p);   // optimization.py:60-73
    if (mode < 0) {
        if (blockIdx.x == 0 && tid == 0) halt_set(st, mode, t, sweep, t);
        return;
    }
    for (int l = tid; l < k; l += 128) gsh[l] = (l == t) ? (resid_form ? -nw : 0.0) : red_gram(red, ldz, k, l);
    __syncthreads();
    const i64 j = (i64)blockIdx.x * 128 + tid;
    double x = 0.0, mx = -1.0e300;
    if (j < d) {
        if (told) told[j] = T[(i64)t * ldt + j];
        // gsh[t] == 0, so row t may be read like the others; 16 loads are issued before the first use
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        for (int l0 = 0; l0 < k; l0 += 16) {
            double tv[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) tv[q] = (l0 + q < k) ? T[(i64)(l0 + q) * ldt + j] : 0.0;
#pragma unroll
            for (int q = 0; q < 16; q += 4) {
                if (l0 + q < k) a0 = fma(gsh[l0 + q], tv[q], a0);
                if (l0 + q + 1 < k) a1 = fma(gsh[l0 + q + 1], tv[q + 1], a1);
                if (l0 + q + 2 < k) a2 = fma(gsh[l0 + q + 2], tv[q + 2], a2);
                if (l0 + q + 3 < k) a3 = fma(gsh[l0 + q + 3], tv[q + 3], a3);
            }
        }
        const double acc = (a0 + a1) + (a2 + a3);
        const double numer = (red[j] - acc) - p.reg_t_l1;
        if (mode == 0) x = fmax(numer, 0.0) / (c + p.eps);
        else if (mode == 1) x = (-numer + c < 0.0) ? p.t_row_sum : 0.0;
        else { x = numer; mx = numer; }
        xraw[j] = x;
        if (mode == 1 || (mode == 0 && !project)) T[(i64)t * ldt + j] = x;
    }
    if (mode != 2) {
        const double s = block_sum(x, scratch);
        if (tid == 0) tpart[blockIdx.x] = s;
    } else {
        i64 idx = (j < d) ? j : (i64)0x7fffffffffffffffLL;
        wave_argmax(mx, idx);
        __shared__ double wm[2];
        __shared__ i64 wi[2];
        if ((tid & 63) == 0) { wm[tid >> 6] = mx; wi[tid >> 6] = idx; }
        __syncthreads();
        if (tid == 0) {
            if (wm[1] > wm[0] || (wm[1] == wm[0] && wi[1] < wi[0])) { wm[0] = wm[1]; wi[0] = wi[1]; }
            tpart[blockIdx.x] = wm[0];
            tpart_idx[blockIdx.x] = wi[0];
        }
    }
    if (blockIdx.x == 0 && tid == 0) st->tmode = mode;
}

// =========================================================================================
// k_trow_early: k_trow_numer for the early-sums schedule -- no projection configured, the Gram form: the row is stored here
// and T T[t,:]^T, which the next pass's early job needs before that pass is launched, is left as one partial vector per
// workgroup.  1024 threads = 256 columns: wave w takes the topics l = q, q + 4, ... (q = w & 3) of the 64 columns cw = w >> 2,
// so the four accumulators a0..a3 of k_trow_numer belong to four waves, each with its terms in ascending l, and
// numer = (a0 + a1) + (a2 + a3) keeps its bits; a wave's first 16 T values come in one batch of loads and are still in
// registers when x_j is known: times x_j and wave-summed they are the wave's share of (T T[t,:]^T)[l] (l == t: sum x_j^2).
// tpart keeps its grouping of 128 columns (two column waves, added as block_sum adds them).
// wfp != NULL: the W half before this step was k_wfin's (of topic twfin), and the two sums that need the new column -- <w_t, w_twfin>
// and sum W[:,twfin] -- are its two vectors of `ntiles` tile partials; every workgroup adds them in one fixed order.
// =========================================================================================
__global__ __launch_bounds__(1024) void k_trow_early(double* __restrict__ T, i64 ldt, int d, int k, int t,
                                                     const double* __restrict__ red, i64 ldz,
                                                     const double* __restrict__ wfp, int ntiles, int twfin,
                                                     double* __restrict__ xraw, double* __restrict__ tpart,
                                                     double* __restrict__ Tearly, int check_prev, int tprev,
                                                     int sweep, KParams p, DevState* st) {
    static_assert(TROW_EARLY_COLS == 256, "16 waves: 4 topic residues x 4 column waves");
    if (st->halt) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = wave & 3, cw = wave >> 2;
    __shared__ double scratch[40];
    __shared__ double gsh[RRI_MAX_K];
    __shared__ double ash[4][256];
    __shared__ double xsh[256];
    __shared__ double wsum[4];
    __shared__ double psh[4][RRI_MAX_K];
    static_assert(RRI_MAX_K <= 1024, "a thread per topic");
    const int cl = cw * 64 + lane;
    const i64 j = (i64)blockIdx.x * 256 + cl;
    const bool in = j < d;
    constexpr int CH = 16;
    // every load that waits for nothing first, so that they share one round trip: the wave's first batch of T (row t among them:
    // gsh[t] == 0, so it may be read like the others), the reduced column sum, the Gram row, the per-tile partials
    double tv0[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) tv0[i] = (q + 4 * i < k && in) ? T[(i64)(q + 4 * i) * ldt + j] : 0.0;
    const double zj = (q == 0 && in) ? red[j] : 0.0;
    const double gl = tid < k ? red_gram(red, ldz, k, tid) : 0.0;
    const double nw = red_gram(red, ldz, k, k);
    double gprev = 0.0, colsum = 0.0;
    if (wfp) {
        const double ga = ordered_sum<2>(wfp, 1, tid, ntiles, 1024);
        const double gb = ordered_sum<2>(wfp + ntiles, 1, tid, ntiles, 1024);
        // the two workgroup sums side by side: wave sums, then the 16 wave totals in wave order (block_sum's order)
        const double wa = wave_sum<double>(ga), wb = wave_sum<double>(gb);
        if (lane == 0) { scratch[wave] = wa; scratch[16 + wave] = wb; }
        __syncthreads();
        for (int i = 0; i < 16; ++i) { gprev += scratch[i]; colsum += scratch[16 + i]; }
        // what k_wfin's Gram slices hold in these two places is zero; frozen rows have added their share there (k_frozen_add)
        colsum += red_gram(red, ldz, k, k + 1);
    } else if (check_prev) colsum = red_gram(red, ldz, k, k + 1);
    if (check_prev) {
        const int code = wcol_code(colsum, p);
        if (code != 0) {
            if (blockIdx.x == 0 && tid == 0) halt_set(st, code, tprev, sweep, t);
            return;
        }
    }
    const double c = nw + p.reg_t_l2;  // denom = nw + reg_t_l2 (nmf.py:438)
    const int mode = trow_denominator_mode(c, p);   // optimization.py:60-73; no projection here: 0, 1 or an error
    if (mode < 0) {
        if (blockIdx.x == 0 && tid == 0) halt_set(st, mode, t, sweep, t);
        return;
    }
    if (tid < k) gsh[tid] = (tid == t) ? 0.0 : ((wfp && tid == twfin) ? gprev + gl : gl);
    __syncthreads();
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < CH; ++i)
        if (q + 4 * i < k) a = fma(gsh[q + 4 * i], tv0[i], a);
    for (int l0 = q + 4 * CH; l0 < k; l0 += 4 * CH) {
        double tv[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) tv[i] = (l0 + 4 * i < k && in) ? T[(i64)(l0 + 4 * i) * ldt + j] : 0.0;
#pragma unroll
        for (int i = 0; i < CH; ++i)
            if (l0 + 4 * i < k) a = fma(gsh[l0 + 4 * i], tv[i], a);
    }
    ash[q][cl] = a;
    __syncthreads();
    if (q == 0) {
        double x = 0.0;
        if (in) {
            const double acc = (ash[0][cl] + ash[1][cl]) + (ash[2][cl] + ash[3][cl]);
            const double numer = (zj - acc) - p.reg_t_l1;
            if (mode == 0) x = fmax(numer, 0.0) / (c + p.eps);
            else x = (-numer + c < 0.0) ? p.t_row_sum : 0.0;
            xraw[j] = x;
            T[(i64)t * ldt + j] = x;
        }
        xsh[cl] = x;
        const double ws = wave_sum<double>(x);
        if (lane == 0) wsum[cw] = ws;
    }
    __syncthreads();
    const double x = xsh[cl];
    if (tid < 2 && ((i64)blockIdx.x * 2 + tid) * 128 < d) tpart[blockIdx.x * 2 + tid] = (0.0 + wsum[2 * tid]) + wsum[2 * tid + 1];
    // T T[t,:]^T of the row as stored: this workgroup's 256 columns (rows l != t are final; row t is x)
#pragma unroll
    for (int i = 0; i < CH; ++i) {
        const int l = q + 4 * i;
        if (l < k) {   // wave-uniform
            const double s = wave_sum<double>((l == t ? x : tv0[i]) * x);
            if (lane == 0) psh[cw][l] = s;
        }
    }
    for (int l0 = q + 4 * CH; l0 < k; l0 += 4 * CH) {
        double tv[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int l = l0 + 4 * i;
            tv[i] = (l < k && in && l != t) ? T[(i64)l * ldt + j] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int l = l0 + 4 * i;
            if (l < k) {
                const double s = wave_sum<double>((l == t ? x : tv[i]) * x);
                if (lane == 0) psh[cw][l] = s;
            }
        }
    }
    __syncthreads();
    for (int l = tid; l < k; l += 1024) Tearly[(i64)blockIdx.x * k + l] = (psh[0][l] + psh[1][l]) + (psh[2][l] + psh[3][l]);
    if (blockIdx.x == 0 && tid == 0) st->tmode = mode;
}

// =========================================================================================
// k_trow_small: k_reduce and k_trow_numer in ONE launch, for problems small enough that every workgroup can afford
// to reduce the Gram partials itself (nwb (k+2) doubles, L2-resident): launch-bound sizes lose a dependent launch per
// topic step.  Block = 32 columns x 32 groups (1024 threads): the groups share the row blocks of Zpart for the column
// sums, the Gpart rows for the Gram entries and the topics for (w^T W)_{-t} T; partials meet in LDS and are added in a
// fixed order.  Also writes red (columns and slice 0 of the Gram part, the other slices zero), so whoever reads the
// reduce buffer afterwards sees what k_reduce would have left up to the order of the sums.
// tpart / tpart_idx then hold one entry per 32 columns.
// =========================================================================================
__global__ __launch_bounds__(1024) void k_trow_small(double* __restrict__ T, i64 ldt, int d, int k, int t,
                                                     const double* __restrict__ Zpart, int nrb,
                                                     const double* __restrict__ Gpart, int nwb, double* __restrict__ red,
                                                     i64 ldz, double* __restrict__ xraw, double* __restrict__ tpart,
                                                     i64* __restrict__ tpart_idx, int check_prev, int tprev, int sweep,
                                                     KParams p, DevState* st, int resid_form, double* __restrict__ told) {
    if (st->halt) return;
    const int tid = threadIdx.x;
    __shared__ double sh[32 * 33];
    __shared__ double gsh[RRI_MAX_K + 2];
    __shared__ double zs[32];
    const int cc = tid & 31, g = tid >> 5;
    const i64 j = (i64)blockIdx.x * 32 + cc;
    // The three sets of operands of this kernel -- Gram partials, column-sum partials, rows of T -- do not depend on
    // each other: the column-sum partials (the first 16 per thread) and the rows of T (the first 4 per thread) are
    // requested here, before the Gram stage and its barriers, so the three round trips to L2 overlap instead of
    // following one another (launch-bound sizes: this kernel is a chain of dependent latencies, nothing else).
    constexpr int ZB = 16;
    double zpre[ZB];
#pragma unroll
    for (int q = 0; q < ZB; ++q) {
        const int r = g + 32 * q;
        zpre[q] = (j < ldz && r < nrb) ? Zpart[(i64)r * ldz + j] : 0.0;
    }
    double tkeep[4];     // T[g + 32 q][j]: the first round of the (w^T W) T sum (all there is when k <= 128)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int l = g + 32 * q;
        tkeep[q] = (j < d && l < k && (l != t || resid_form)) ? T[(i64)l * ldt + j] : 0.0;
    }
    // Gram entries [w^T W (k) | ||w||^2 | sum W[:,tprev]]: 32 groups over the Gpart rows, 32 entries per round
    for (int l0 = 0; l0 < k + 2; l0 += 32) {
        const int l = l0 + cc;
        double a = 0.0;
        if (l < k + 2) a = ordered_sum<8>(Gpart + l, k + 2, g, nwb, 32);
        __syncthreads();
        sh[g * 33 + cc] = a;
        __syncthreads();
        if (tid < 32 && l < k + 2) {
            double s = 0.0;
            for (int q = 0; q < 32; ++q) s += sh[q * 33 + tid];
            gsh[l] = s;
        }
    }
    __syncthreads();
    const double nw = gsh[k];
    if (check_prev) {
        const int code = wcol_code(gsh[k + 1], p);
        if (code != 0) {
            if (blockIdx.x == 0 && tid == 0) halt_set(st, code, tprev, sweep, t);
            return;
        }
    }
    const double c = nw + p.reg_t_l2;  // denom = nw + reg_t_l2 (nmf.py:438)
    const bool project = p.project_T && p.has_trs;
    const int mode = trow_denominator_mode(c, p);   // optimization.py:60-73
    if (mode < 0) {
        if (blockIdx.x == 0 && tid == 0) halt_set(st, mode, t, sweep, t);
        return;
    }
    if (blockIdx.x == 0)   // the reduce buffer as k_reduce leaves it: slice 0 carries the sums, the rest zeros
        for (int i = tid; i < GRAM_SLICES * (k + 2); i += 1024) red[ldz + i] = i < k + 2 ? gsh[i] : 0.0;
    {
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < ZB; ++q) a += zpre[q];                          // rows g, g + 32, ...: the same order as before
        if (j < ldz) a = ordered_sum_acc<8>(a, Zpart + j, ldz, g + 32 * ZB, nrb, 32);
        sh[g * 33 + cc] = a;
    }
    __syncthreads();
    if (tid < 32) {   // here cc == tid
        double s = 0.0;
        for (int q = 0; q < 32; ++q) s += sh[q * 33 + tid];
        zs[tid] = s;
        if (j < ldz) red[j] = s;
    }
    __syncthreads();
    {
        double a = 0.0;
        if (j < d)
            for (int l0 = g; l0 < k; l0 += 32 * 4) {   // 4 rows of T in flight, added in topic order
                double tv[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int l = l0 + 32 * q;
                    if (l0 == g) tv[q] = tkeep[q];
                    else tv[q] = (l < k && (l != t || resid_form)) ? T[(i64)l * ldt + j] : 0.0;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int l = l0 + 32 * q;
                    if (l < k && l != t) a = fma(gsh[l], tv[q], a);
                    else if (l == t && resid_form) a = fma(-nw, tv[q], a);   // + ||w_t||^2 T[t,:] (explicit-residual form)
                }
            }
        sh[g * 33 + cc] = a;
    }
    __syncthreads();
    if (tid < 64) {   // wave 0; lanes 0..31 own a column each
        double x = 0.0, mx = -1.0e300;
        i64 idx = (i64)0x7fffffffffffffffLL;
        if (tid < 32 && j < d) {
            double acc = 0.0;
            for (int q = 0; q < 32; ++q) acc += sh[q * 33 + tid];
            if (told) told[j] = T[(i64)t * ldt + j];
            const double numer = (zs[tid] - acc) - p.reg_t_l1;
            if (mode == 0) x = fmax(numer, 0.0) / (c + p.eps);
            else if (mode == 1) x = (-numer + c < 0.0) ? p.t_row_sum : 0.0;
            else { x = numer; mx = numer; idx = j; }
            xraw[j] = x;
            if (mode == 1 || (mode == 0 && !project)) T[(i64)t * ldt + j] = x;
        }
        if (mode != 2) {
            const double s = wave_sum<double>(x);
            if (tid == 0) tpart[blockIdx.x] = s;
        } else {
            wave_argmax(mx, idx);
            if (tid == 0) { tpart[blockIdx.x] = mx; tpart_idx[blockIdx.x] = idx; }
        }
    }
    if (blockIdx.x == 0 && tid == 0) st->tmode = mode;
}

// Michelot's fixed point for the Euclidean simplex projection (same active set, hence the same
// theta = (sum_active - s)/|active|, as the sort of matrixops.py:58-63).  Single workgroup.
__device__ inline double simplex_theta(const double* v, int d, double s, double* scratch, int* iters) {
    double theta = -1.0e300;
    i64 cnt_prev = -1;
    int it = 0;
    for (; it < d + 2; ++it) {
        double sum = 0.0, cnt = 0.0;
        for (int j = threadIdx.x; j < d; j += blockDim.x) {
            const double x = v[j];
            if (x > theta) { sum += x; cnt += 1.0; }
        }
        sum = block_sum(sum, scratch);
        cnt = block_sum(cnt, scratch);
        const i64 ci = (i64)cnt;
        if (ci == cnt_prev || ci == 0) break;
        theta = (sum - s) / cnt;
        cnt_prev = ci;
    }
    *iters = it;
    return theta;
}

// =========================================================================================
// k_trow_final: finishes qf_min (simplex projection or one-hot), the row checks of
// _project_and_check_reset_t (nmf.py:751-769) and writes T[t,:].  One workgroup of 1024.
// `light` = no projection configured: the row is already in T and only the sums are needed.
// =========================================================================================
__global__ __launch_bounds__(1024) void k_trow_final(double* __restrict__ T, i64 ldt, int d, int t,
                                                     double* __restrict__ xraw, const double* __restrict__ tpart,
                                                     const i64* __restrict__ tpart_idx, int nblk, int sweep,
                                                     KParams p, DevState* st) {
    if (st->halt) return;
    __shared__ double scratch[40];
    const int tid = threadIdx.x;
    const int mode = st->tmode;
    const bool project = p.project_T && p.has_trs;
    double nx = 1.0, sumT = 0.0;
    int iters = 0;
    bool row_dirty = false;  // xraw differs from what k_trow_numer stored in T
    if (mode == 2) {
        double bm = tpart[0];
        i64 bi = tpart_idx[0];
        for (int b = 1; b < nblk; ++b)
            if (tpart[b] > bm) { bm = tpart[b]; bi = tpart_idx[b]; }
        for (int j = tid; j < d; j += blockDim.x) xraw[j] = (j == bi) ? 1.0 : 0.0;
        row_dirty = true;
    } else {
        double ps = 0.0;
        ps = ordered_sum<4>(tpart, 1, tid, nblk, (int)blockDim.x);
        ps = block_sum(ps, scratch);
        if (mode == 0) nx = ps;
        sumT = ps;
        if (mode == 0 && project) {
            const double th = simplex_theta(xraw, d, p.t_row_sum, scratch, &iters);
            for (int j = tid; j < d; j += blockDim.x) xraw[j] = fmax(xraw[j] - th, 0.0);
            if (tid == 0) st->theta = th;
            row_dirty = true;
        }
    }
    if (row_dirty) {
        __syncthreads();
        sumT = 0.0;
        for (int j = tid; j < d; j += blockDim.x) sumT += xraw[j];
        sumT = block_sum(sumT, scratch);
    }
    if (trow_kept(sumT, p)) {
        // nmf.py:759-761: project again when the row is not on the simplex to 1e-15
        if (p.has_trs && p.t_row_sum != 0.0 && p.project_T && fabs(sumT - p.t_row_sum) > 1e-15) {
            int it2 = 0;
            const double th = simplex_theta(xraw, d, p.t_row_sum, scratch, &it2);
            for (int j = tid; j < d; j += blockDim.x) xraw[j] = fmax(xraw[j] - th, 0.0);
            iters += it2;
            row_dirty = true;
        }
    }
    if (row_dirty) {
        __syncthreads();
        for (int j = tid; j < d; j += blockDim.x) T[(i64)t * ldt + j] = xraw[j];
    }
    if (tid == 0) {
        st->nt1 = nx;
        st->sumT = sumT;
        st->proj_iters = iters;
        if (trow_resets(sumT, p)) halt_set(st, HALT_EVENT_RESET_T, t, sweep, t);
    }
}

// k_tgram: partial T T[t,:]^T over column slice blockIdx.y: Ttpart[y][l] = <T[l,slice], T[t,slice]>
// (entry l == t is the slice's share of ||T[t,:]||^2; k_wcol sums the slices, nmf.py:730-734).
// finish != 0 (no projection configured, so k_trow_numer already stored the row): block (0,0) also does
// what is left of _project_and_check_reset_t: nt1, sum(T[t,:]) and the reset decision (nmf.py:757-769).
__global__ __launch_bounds__(256) void k_tgram(const double* __restrict__ T, i64 ldt, int d, int k, int t,
                                               double* __restrict__ Ttpart, const double* __restrict__ tpart,
                                               int nblk, int finish, int sweep, KParams p, DevState* st) {
    if (st->halt) return;
    __shared__ double scratch[40];
    tgram_block(T, ldt, d, k, t, blockIdx.x, blockIdx.y, gridDim.y, Ttpart, tpart, nblk, finish, sweep, p, st, scratch);
}

// W[:,t] *= nt1 (nmf.py:450-452); only observable when fix_W keeps the column.
__global__ __launch_bounds__(256) void k_scale_wcol(double* Wt, i64 ldw, int n, int t, const DevState* st) {
    if (st->halt) return;
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) Wt[(i64)t * ldw + i] *= st->nt1;
}

// the W-column check alone, against the reduced buffer (row-sharded runs, after the last sweep)
__global__ __launch_bounds__(64) void k_check_red(const double* __restrict__ red, i64 ldz, int k, int tprev,
                                                  int sweep, int pos, KParams p, DevState* st) {
    if (st->halt) return;
    if (threadIdx.x == 0) {
        const int code = wcol_code(red_gram(red, ldz, k, k + 1), p);
        if (code != 0) halt_set(st, code, tprev, sweep, pos);
    }
}

// stand-alone W-column check for the paths without a following T-row step
__global__ __launch_bounds__(256) void k_check_wcol(const double* __restrict__ Gpart, int nwb, int k, int tprev,
                                                    int sweep, int pos, KParams p, DevState* st) {
    if (st->halt) return;
    __shared__ double scratch[40];
    double a = 0.0;
    a = ordered_sum<8>(Gpart + k + 1, k + 2, threadIdx.x, nwb, (int)blockDim.x);
    a = block_sum(a, scratch);
    if (threadIdx.x == 0) {
        const int code = wcol_code(a, p);
        if (code != 0) halt_set(st, code, tprev, sweep, pos);
    }
}

// row-sharded runs: this rank's share of sum W[:,tprev] (and no negative-denominator flag) into tail[0..1]; the
// verdict is taken on the all-reduced pair (k_wcheck_tail)
__global__ __launch_bounds__(256) void k_colsum_tail(const double* __restrict__ Gpart, int nwb, int k,
                                                     double* __restrict__ tail, const DevState* __restrict__ st) {
    if (st->halt) return;
    __shared__ double scratch[40];
    double a = ordered_sum<8>(Gpart + k + 1, k + 2, threadIdx.x, nwb, (int)blockDim.x);
    a = block_sum(a, scratch);
    if (threadIdx.x == 0) { tail[0] = a; tail[1] = 0.0; }
}

// max-residual reset of a row-sharded run: this rank's candidate (largest row-residual norm, its GLOBAL row index)
__global__ void k_pack_candidate(const double* __restrict__ rowpos, const i64* __restrict__ idx, i64 row_offset,
                                 double* __restrict__ out) {
    const i64 i = idx[0];
    out[0] = rowpos[i];
    out[1] = (double)(row_offset + i);
}

// =========================================================================================
// k_proj_rows: Euclidean projection of every row of W on the simplex of radius s (scalar) or
// s_vec[i] (matrixops.py:72-100; nmf.py:481-484, 519-529).  One thread per row; the k entries
// of a row are k coalesced loads from the k-major Wt (re-read per Michelot iteration from L2).
// =========================================================================================
__global__ __launch_bounds__(256) void k_proj_rows(double* __restrict__ Wt, i64 ldw, int n, int k, double s_scalar,
                                                   const double* __restrict__ s_vec) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double s = s_vec ? s_vec[i] : s_scalar;
    double theta = -1.0e300;
    int cnt_prev = -1;
    for (int it = 0; it < k + 2; ++it) {
        double sum = 0.0;
        int cnt = 0;
        for (int l = 0; l < k; ++l) {
            const double x = Wt[(i64)l * ldw + i];
            if (x > theta) { sum += x; ++cnt; }
        }
        if (cnt == cnt_prev || cnt == 0) break;
        theta = (sum - s) / (double)cnt;
        cnt_prev = cnt;
    }
    for (int l = 0; l < k; ++l) Wt[(i64)l * ldw + i] = fmax(Wt[(i64)l * ldw + i] - theta, 0.0);
}

// =========================================================================================
// k_resid: E = X - W T on 64x64 tiles with a 4x4 register tile per thread (a dense k-panel
// GEMM on the vector ALU; not on the per-sweep hot path).  Used for
//   - true_objective (nmf.py:77-83): rowobj[i] = sum_j (Wm_ij) E_ij^2
//   - 'max_resid_document' (nmf.py:771-773): rowpos[i] = sum_j max(E_ij,0)^2
//   - WRITE_E: the masked residual M .* E of the weighted flavour.
// grid = ceil(n/64) workgroups of 256; each walks all column tiles (deterministic sums).
// =========================================================================================
template <typename SX, bool MASKED, bool WRITE_E>
__global__ __launch_bounds__(256) void k_resid(const SX* __restrict__ X, i64 ldx, const SX* __restrict__ M, i64 ldm,
                                               const unsigned* __restrict__ Mb, i64 ldb,
                                               const double* __restrict__ Wt, i64 ldw, const double* __restrict__ T,
                                               i64 ldt, int n, int d, int k, double* __restrict__ rowobj,
                                               double* __restrict__ rowpos, SX* __restrict__ E, i64 lde,
                                               int w_resident, const XScale xs) {
    typedef double S;
    constexpr int KC = 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // w_resident: the whole 64-row tile of W (k x 64) stays in LDS for all column tiles (k <= 256); otherwise only a
    // KC-topic slice at a time, reloaded per column tile (large k: correctness path, L2 traffic n k 8 per column tile)
    S* Wsh = reinterpret_cast<S*>(smem);          // [k or KC][64]  (transposed tile of W)
    S* Tsh = Wsh + (size_t)(w_resident ? k : KC) * 64;   // [KC][64]
    double* red = reinterpret_cast<double*>(Tsh + KC * 64);  // [64][17]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const i64 row0 = (i64)blockIdx.x * 64;
    if (w_resident)
        for (int idx = tid; idx < 64 * k; idx += 256) {
            const int l = idx >> 6, r = idx & 63;
            Wsh[l * 64 + r] = (row0 + r < n) ? Wt[(i64)l * ldw + row0 + r] : S(0);
        }
    double so[4] = {0, 0, 0, 0}, sp[4] = {0, 0, 0, 0};
    for (i64 c0 = 0; c0 < d; c0 += 64) {
        S acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = S(0);
        for (int l0 = 0; l0 < k; l0 += KC) {
            const int kc = min(KC, k - l0);
            __syncthreads();
            for (int idx = tid; idx < kc * 64; idx += 256) {
                const int l = idx >> 6, c = idx & 63;
                Tsh[l * 64 + c] = (c0 + c < d) ? T[(i64)(l0 + l) * ldt + c0 + c] : S(0);
                if (!w_resident) Wsh[l * 64 + c] = (row0 + c < n) ? Wt[(i64)(l0 + l) * ldw + row0 + c] : S(0);
            }
            __syncthreads();
            const int wbase = w_resident ? l0 : 0;
            for (int l = 0; l < kc; ++l) {
                S wv[4], tv[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) wv[a] = Wsh[(wbase + l) * 64 + ty * 4 + a];
#pragma unroll
                for (int b = 0; b < 4; ++b) tv[b] = Tsh[l * 64 + tx * 4 + b];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = fma(wv[a], tv[b], acc[a][b]);
            }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const i64 i = row0 + ty * 4 + a;
            if (i >= n) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const i64 j = c0 + tx * 4 + b;
                if (j >= d) continue;
                S e = x_elem(X, ldx, i, j, xs) - acc[a][b];
                const S m = !MASKED ? S(1)
                                    : (Mb ? (S)((Mb[(i >> 3) * ldb + (j >> 2)] >> ((int)((i & 7) << 2) + (int)(j & 3))) & 1u)
                                          : (S)M[i * ldm + j]);
                if (WRITE_E) E[i * lde + j] = (SX)(m * e);
                so[a] += (double)m * (double)e * (double)e;
                const double ep = e > S(0) ? (double)e : 0.0;
                sp[a] += ep * ep;
            }
        }
    }
    __syncthreads();
    // reduce the 16 column-group partials of every row in a fixed order
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int a = 0; a < 4; ++a) red[(ty * 4 + a) * 17 + tx] = pass == 0 ? so[a] : sp[a];
        __syncthreads();
        if (tid < 64 && row0 + tid < n) {
            double s = 0.0;
            for (int q = 0; q < 16; ++q) s += red[tid * 17 + q];
            if (pass == 0) { if (rowobj) rowobj[row0 + tid] = s; }
            else { if (rowpos) rowpos[row0 + tid] = s; }
        }
        __syncthreads();
    }
}

// =========================================================================================
// k_resid_mfma: the same residual on the matrix cores, for k <= 64: E tile (64 rows x 64 columns per step) =
// X - W T with v_mfma_f64_16x16x4_f64.  Wave w of the block owns rows 16w .. 16w+15: its A fragments (W rows,
// one double per lane and k-step: lane l holds W[row l&15][4s + (l>>4)]) stay in registers for the whole row
// block; the T tile of a step (4 KS x 64 doubles) is shared by the 4 waves through LDS, double-buffered: the loads
// of step j+1 (T tile and X) are in flight while the 4 KS MFMAs of step j run.
// The 4 MFMA tiles of a step take INTERLEAVED columns -- tile c owns columns c0 + 4m + c, m < 16 -- so the 4 results
// a lane holds for one row (f64 MFMA result layout: lane l, register r = row (l>>4) + 4r, tile column l&15) are 4
// CONSECUTIVE columns of X: one 16-byte load (and store) per lane and row, 256 contiguous bytes per 16 lanes, and
// one mask nibble.  The T tile is parked in LDS permuted to match (column 4m + c at slot 16c + m), so a B fragment
// read is 16 consecutive doubles: no bank conflicts.
// =========================================================================================
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int RESID_TS = 64;   // row stride of k_resid_mfma's T tile in LDS, in doubles (80 -- the two k-rows a half-wave reads then lie
                               // 32 banks apart instead of on the same banks -- measured the same: 2.81 ms at BASELINE config 5)

// SUMS = false (a rebuild of the stored residual that wants neither row sums): the epilogue is convert, subtract, store.
template <typename SX, bool MASKED, bool WRITE_E, int KS, int WAVES, bool SUMS = true>   // KS = k-steps of 4 (4, 8, 12, 13 or 16): k <= 4 KS
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(2))) void k_resid_mfma(const SX* __restrict__ X, i64 ldx, const SX* __restrict__ M,
                                                    i64 ldm, const unsigned* __restrict__ Mb, i64 ldb,
                                                    const double* __restrict__ Wt, i64 ldw,
                                                    const double* __restrict__ T, i64 ldt, int n, int d, int k,
                                                    double* __restrict__ rowobj, double* __restrict__ rowpos,
                                                    SX* __restrict__ E, i64 lde, int dchunk, const XScale xs) {
    // blockIdx.y: the column range [y dchunk, (y+1) dchunk) of the row block (dchunk a multiple of 64; the builds that take row
    // sums run with one range).  A row block over ALL columns is a long workgroup, and 1563 of them on 256 CUs x 2 are 3.05
    // rounds: the last 26 ran a fourth round on an empty chip.
    constexpr int kp = 4 * KS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* tsh = reinterpret_cast<double*>(smem);   // [2][kp][RESID_TS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 row0 = (i64)blockIdx.x * (16 * WAVES) + wave * 16;
    const int lr = lane & 15, lk = lane >> 4;
    double afrag[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int l = 4 * s + lk;
        afrag[s] = (l < k && row0 + lr < n) ? Wt[(i64)l * ldw + row0 + lr] : 0.0;
    }
    // cooperative load of a T tile: thread -> column tid & 63 (parked at its permuted slot), rows (tid >> 6) + WAVES i
    const int tc = tid & 63, tr = tid >> 6;
    const int slot = 16 * (tc & 3) + (tc >> 2);
    constexpr int NST = (kp + WAVES - 1) / WAVES;
    double stage[NST];
    // (a float16 X is staged as float: exact; counts are staged as float64, with both scales already applied: (c s_j) r_i)
    typedef typename std::conditional<sizeof(SX) <= 4 && !XSCALED<SX>, float, double>::type XR;
    XR xq[4][4];                                     // the lane's 4 rows x 4 consecutive columns of X, as stored
    XR xn[4][4];                                     // ... of the NEXT step: requested at the start of a step, so that
                                                     // nothing issued late in a step is waited for before its barrier
    auto fetch = [&](i64 c0) {
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int l = tr + WAVES * i;
            stage[i] = (l < k && c0 + tc < d) ? T[(i64)l * ldt + c0 + tc] : 0.0;
        }
    };
    auto park = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NST; ++i)
            if (tr + WAVES * i < kp) tsh[((size_t)buf * kp + tr + WAVES * i) * RESID_TS + slot] = stage[i];
    };
    // X: rows row0 + lk + 4r, columns c0 + 4 lr .. + 3 (a 16-byte vector when the storage type is fp32 and the
    // columns are all there; elementwise at the ragged edge and for fp64 storage)
    auto fetch_x = [&](i64 c0, XR (&dst)[4][4]) {
        const i64 j = c0 + 4 * lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const i64 i = row0 + lk + 4 * r;
            bool done = false;
            if constexpr (sizeof(SX) == 4) {
                if (i < n && j + 3 < d) {
                    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(X + i * ldx + j));
                    dst[r][0] = v[0]; dst[r][1] = v[1]; dst[r][2] = v[2]; dst[r][3] = v[3];
                    done = true;
                }
            }
            if constexpr (sizeof(SX) == 2) {         // float16: the 4 columns are one 8-byte vector (row stride a multiple of 8)
                if (i < n && j + 3 < d) {
                    const f16x4 v = __builtin_nontemporal_load(reinterpret_cast<const f16x4*>(X + i * ldx + j));
                    dst[r][0] = (float)v[0]; dst[r][1] = (float)v[1]; dst[r][2] = (float)v[2]; dst[r][3] = (float)v[3];
                    done = true;
                }
            }
            if constexpr (XSCALED<SX>) {                // the 4 counts of a row are one 4-byte word (row stride a multiple of 8)
                if (i < n && j + 3 < d) {
                    const unsigned w = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(X + i * ldx + j));
                    const double ri = xs.row[i];
#pragma unroll
                    for (int c = 0; c < 4; ++c) dst[r][c] = ((double)(float)((w >> (8 * c)) & 0xffu) * xs.col[j + c]) * ri;
                    done = true;
                }
            }
            if (!done) {
#pragma unroll
                for (int c = 0; c < 4; ++c) dst[r][c] = (i < n && j + c < d) ? (XR)x_elem(X, ldx, i, j + c, xs) : XR(0);
            }
        }
    };
    // the lane's nibble rows of the bit-packed mask, requested with the X tile of the same step (round 4: loaded where they
    // were used, each of the four words was waited for on its own -- s_waitcnt vmcnt(0) four times per step and wave, with the
    // next step's T and X tiles in the same queue: the matrix cores were busy 38 % of the rebuild, SQ_VALU_MFMA_BUSY_CYCLES)
    unsigned mq[4] = {0xFu, 0xFu, 0xFu, 0xFu}, mn[4] = {0xFu, 0xFu, 0xFu, 0xFu};
    auto fetch_m = [&](i64 c0, unsigned (&dst)[4]) {
        if (!(MASKED && Mb)) return;
        const i64 j = c0 + 4 * lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const i64 i = row0 + lk + 4 * r;
            dst[r] = (i < n && j < d) ? Mb[(i >> 3) * ldb + (j >> 2)] : 0u;      // the raw word: shifted where it is used (a
                                                                                   // shift here is a wait for the load here)
        }
    };
    double so[4] = {0, 0, 0, 0}, sp[4] = {0, 0, 0, 0};
    const i64 cb = (i64)blockIdx.y * dchunk;
    const i64 ce = cb + dchunk < (i64)d ? cb + dchunk : (i64)d;
    fetch(cb);
    fetch_x(cb, xq);
    fetch_m(cb, mq);
    park(0);
    __syncthreads();
    int buf = 0;
    for (i64 c0 = cb; c0 < ce; c0 += 64, buf ^= 1) {
        const bool more = c0 + 64 < ce;
        if (more) {                                  // the next T tile AND the next X tile: in flight during the MFMAs
            fetch(c0 + 64);                          // and the epilogue below (round 1 asked for X after the epilogue and
            fetch_x(c0 + 64, xn);                    // then waited for it -- vmcnt(0) before the park -- once per step)
            fetch_m(c0 + 64, mn);
        }
        f64x4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
        const double* tb = tsh + (size_t)buf * kp * RESID_TS;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const double b = tb[(4 * s + lk) * RESID_TS + 16 * c + lr];
                acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(afrag[s], b, acc[c], 0, 0, 0);
            }
        }
        // the next T tile goes to LDS BEFORE the epilogue's stores are issued: the wait for its loads is a wait for everything this
        // wave has in the vector-memory queue, and after the epilogue that includes the four 16-byte stores of E -- their
        // acknowledgement was waited for in every step (round 4, from the ISA: s_waitcnt vmcnt(0) between the last store and the
        // first ds_write).  Here the stores of a step have the matrix-core phase of the next one to land.
        if (more) park(buf ^ 1);
        // epilogue: e = x - (W T), masked; sums per row; tile c, register r -> row lk + 4r, column 4 lr + c
        const i64 j0 = c0 + 4 * lr;
        // a tile with all its rows and columns there, fp32 storage, no array mask (wave-uniform): the same arithmetic without the
        // per-element edge tests -- those were a branch per element and row in the ISA, hundreds per step
        // (the builds without row sums only: with them the second epilogue takes the k = 52 masked build past 256 registers)
        const bool interior = !SUMS && sizeof(SX) == 4 && row0 + 15 < n && c0 + 64 <= (i64)d && (!MASKED || Mb);
        if (interior) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const i64 i = row0 + lk + 4 * r;
                const unsigned bits = MASKED ? mq[r] >> ((int)(i & 7) << 2) : 0xFu;
                double ev[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double e = (double)xq[r][c] - acc[c][r];
                    const double m = MASKED ? (double)((bits >> c) & 1u) : 1.0;
                    if constexpr (SUMS) {
                        so[r] += m * e * e;
                        const double ep = e > 0.0 ? e : 0.0;
                        sp[r] += ep * ep;
                    }
                    ev[c] = MASKED ? m * e : e;
                }
                if constexpr (WRITE_E && sizeof(SX) == 4) {
                    const f32x4 o = f32x4{(float)ev[0], (float)ev[1], (float)ev[2], (float)ev[3]};
                    __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(E + i * lde + j0));
                }
            }
        } else
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const i64 i = row0 + lk + 4 * r;
            if (i >= n) continue;
            unsigned bits = 0xFu;
            if (MASKED && Mb) bits = mq[r] >> ((int)(i & 7) << 2);
            double ev[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const i64 j = j0 + c;
                double e = 0.0, m = 0.0;
                if (j < d) {
                    e = (double)xq[r][c] - acc[c][r];
                    m = !MASKED ? 1.0 : (Mb ? (double)((bits >> c) & 1u) : (double)M[i * ldm + j]);
                    if constexpr (SUMS) {
                        so[r] += m * e * e;
                        const double ep = e > 0.0 ? e : 0.0;
                        sp[r] += ep * ep;
                    }
                }
                ev[c] = MASKED ? m * e : e;
            }
            if (WRITE_E) {
                bool stored = false;
                if constexpr (sizeof(SX) == 4) {
                    if (j0 + 3 < d) {
                        const f32x4 o = f32x4{(float)ev[0], (float)ev[1], (float)ev[2], (float)ev[3]};
                        __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(E + i * lde + j0));
                        stored = true;
                    }
                }
                if (!stored) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (j0 + c < d) E[i * lde + j0 + c] = (SX)ev[c];
                }
            }
        }
        if (more) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) xq[r][c] = xn[r][c];
#pragma unroll
            for (int r = 0; r < 4; ++r) mq[r] = mn[r];
        }
        __syncthreads();
    }
    if constexpr (!SUMS) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            so[r] += __shfl_xor(so[r], off, 64);
            sp[r] += __shfl_xor(sp[r], off, 64);
        }
        const i64 i = row0 + lk + 4 * r;
        if (lr == 0 && i < n) {
            if (rowobj) rowobj[i] = so[r];
            if (rowpos) rowpos[i] = sp[r];
        }
    }
}

// =========================================================================================
// k_xtt_mfma: Qt = (X Tm^T)^T for up to 64 rows of Tm (topics, or the columns of a dense operand) on the matrix
// cores: D(16 rows of X x 16 topics) += A(16 rows x 4 columns of X) * B(4 columns x 16 topics), f64 MFMA 16x16x4.
// Wave w of the block owns rows 16w .. 16w+15.  Per step of 64 columns:
//   * the wave's X tile (16 x 64, storage type) is read coalesced -- 4 rows x 256 bytes per load -- and parked in a
//     wave-private LDS tile; a lane (row i = l&15, group g = l>>4) then picks its A values as 4 vectors
//     xs[i][16m + 4g .. +3]: MFMA number (m, e) contracts the four columns {16m + 4g + e}, g = 0..3 -- any order
//     of the columns is as good as another for a sum, and this one costs no lane movement;
//   * the T tile (64 columns x 16 NT topics) is shared by the 4 waves through LDS, stored [column][topic] (stride
//     16 NT + 1: the transposing stores hit different banks), so the B fragment of (m, e), topic tile c is 16
//     consecutive doubles; double-buffered: the next tile's loads are in flight during the MFMAs.
// Result layout (f64 MFMA): lane l, register r = X row (l>>4) + 4r, topic 16c + (l&15).
// =========================================================================================
template <typename SX, int NT>
__global__ __launch_bounds__(256) void k_xtt_mfma(const SX* __restrict__ X, i64 ldx, const double* __restrict__ T,
                                                  i64 ldt, int n, int d, int m, double* __restrict__ Qt, i64 ldq,
                                                  const XScale sc) {
    typedef XVec<SX> XV;
    typedef typename XV::type V;
    constexpr int VN = XV::N;                 // elements per vector: 4 (fp32), 2 (fp64), 8 (float16, uint8)
    constexpr int TS = 16 * NT + 1;           // row stride of the T tile [column][topic]
    constexpr int XS = 64 + VN;               // row stride of the X tile (elements)
    constexpr int NI = (16 * NT) / 4;         // T rows per thread and tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* tsh = reinterpret_cast<double*>(smem);                         // [2][64][TS]
    SX* xsh = reinterpret_cast<SX*>(tsh + 2 * 64 * TS);                    // [4 waves][16][XS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const i64 row0 = (i64)blockIdx.x * 64 + wave * 16;
    const int li = lane & 15, lg = lane >> 4;
    SX* xs = xsh + (size_t)wave * 16 * XS;
    const int tc = tid & 63, tr = tid >> 6;
    double stage[NI];
    auto fetch = [&](i64 c0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int l = tr + 4 * i;
            if constexpr (XSCALED<SX>) stage[i] = (l < m && c0 + tc < d) ? T[(i64)l * ldt + c0 + tc] * sc.col[c0 + tc] : 0.0;
            else stage[i] = (l < m && c0 + tc < d) ? T[(i64)l * ldt + c0 + tc] : 0.0;
        }
    };
    auto park = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NI; ++i) tsh[((size_t)buf * 64 + tc) * TS + tr + 4 * i] = stage[i];
    };
    // X tile: VN-element vectors, 64 / VN per row, 64 lanes cover (64 * VN / 64) = VN rows per load
    constexpr int VPR = 64 / VN, RPL = 64 / VPR, NL = 16 / RPL;
    V xv[NL];
    auto fetch_x = [&](i64 c0) {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int r = q * RPL + lane / VPR, cv = lane % VPR;
            const i64 i = row0 + r, j = c0 + (i64)cv * VN;
            if (i < n && j + VN - 1 < d) {
                xv[q] = __builtin_nontemporal_load(reinterpret_cast<const V*>(X + i * ldx + j));
            } else {
                double e[VN];
#pragma unroll
                for (int c = 0; c < VN; ++c) e[c] = (i < n && j + c < d) ? (double)X[i * ldx + j + c] : 0.0;
                xv[q] = XV::pack(e);
            }
        }
    };
    auto park_x = [&]() {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int r = q * RPL + lane / VPR, cv = lane % VPR;
            *reinterpret_cast<V*>(xs + r * XS + cv * VN) = xv[q];
        }
    };
    f64x4 acc[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    fetch_x(0);
    park(0);
    park_x();
    __syncthreads();
    int buf = 0;
    for (i64 c0 = 0; c0 < d; c0 += 64, buf ^= 1) {
        const bool more = c0 + 64 < d;
        if (more) { fetch(c0 + 64); fetch_x(c0 + 64); }
        const double* tb = tsh + (size_t)buf * 64 * TS;
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) {
            double a4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) a4[e] = (double)xs[li * XS + 16 * mm + 4 * lg + e];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double* brow = tb + (size_t)(16 * mm + 4 * lg + e) * TS + li;
#pragma unroll
                for (int c = 0; c < NT; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a4[e], brow[16 * c], acc[c], 0, 0, 0);
            }
        }
        __syncthreads();              // every wave is done with this step's tiles (its own X tile included)
        if (more) { park(buf ^ 1); park_x(); }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < NT; ++c) {
        const int l = 16 * c + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const i64 i = row0 + lg + 4 * r;
            if constexpr (XSCALED<SX>) { if (l < m && i < n) Qt[(i64)l * ldq + i] = acc[c][r] * sc.row[i]; }
            else if (l < m && i < n) Qt[(i64)l * ldq + i] = acc[c][r];
        }
    }
}

// partial sums of v, v^2 and |v| over a strided matrix: out[b] = {sum, sumsq, sumabs}
__global__ __launch_bounds__(256) void k_norms(const double* __restrict__ A, i64 rows, i64 cols, i64 ld,
                                               double* __restrict__ out) {
    __shared__ double scratch[40];
    double s1 = 0, s2 = 0, s3 = 0;
    const i64 total = rows * cols;
    for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
        const i64 r = idx / cols, c = idx - r * cols;
        const double v = A[r * ld + c];
        s1 += v; s2 += v * v; s3 += fabs(v);
    }
    s1 = block_sum(s1, scratch);
    s2 = block_sum(s2, scratch);
    s3 = block_sum(s3, scratch);
    if (threadIdx.x == 0) { out[blockIdx.x * 3 + 0] = s1; out[blockIdx.x * 3 + 1] = s2; out[blockIdx.x * 3 + 2] = s3; }
}

// sum of squares of the stored X (float64 accumulation): out[b] partial of block b
template <typename SX>
__global__ __launch_bounds__(256) void k_sqsum(const SX* __restrict__ X, i64 ldx, i64 n, i64 d, double* __restrict__ out,
                                               const XScale xs) {
    __shared__ double scratch[40];
    double s = 0.0;
    const i64 total = n * d;
    for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
        const i64 r = idx / d, c = idx - r * d;
        const double v = x_elem(X, ldx, r, c, xs);
        s = fma(v, v, s);
    }
    s = block_sum(s, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// Gram matrix of the rows of a k x len matrix: G[a*k + b] = <A[a,:], A[b,:]>, one workgroup per (a, b >= a)
__global__ __launch_bounds__(256) void k_gram(const double* __restrict__ A, i64 ld, i64 len, int k, double* __restrict__ G) {
    __shared__ double scratch[40];
    const int a = blockIdx.x, b = blockIdx.y;
    if (b < a) return;
    double s = 0.0;
    for (i64 i = threadIdx.x; i < len; i += 256) s = fma(A[(i64)a * ld + i], A[(i64)b * ld + i], s);
    s = block_sum(s, scratch);
    if (threadIdx.x == 0) { G[a * k + b] = s; G[b * k + a] = s; }
}

// A (m x len, row stride ld) <- L^-1 A for a lower-triangular L (m x m, row-major, m <= 64): forward substitution down every
// column, one thread per column, the column in registers.  With L = chol(A A^T) the rows of the result are orthonormal:
// the Cholesky-QR step of the range finder behind the NNDSVD start (rri_range_finder; initialization.py:105).
__global__ __launch_bounds__(256) void k_lsolve_rows(double* __restrict__ A, i64 ld, i64 len, int m, const double* __restrict__ L) {
    __shared__ double Lsh[64 * 64];
    for (int e = threadIdx.x; e < m * m; e += 256) Lsh[e] = L[e];
    __syncthreads();
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= len) return;
    double v[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) v[i] = i < m ? A[(i64)i * ld + r] : 0.0;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i < m) {
            double acc = v[i];
#pragma unroll
            for (int j = 0; j < i; ++j) acc = fma(-Lsh[i * m + j], v[j], acc);
            v[i] = acc / Lsh[i * m + i];
        }
    }
#pragma unroll
    for (int i = 0; i < 64; ++i)
        if (i < m) A[(i64)i * ld + r] = v[i];
}

// ---- the same two steps of Cholesky-QR on a TALL panel: Y is rows x m, row-major with no padding (m <= 64), the layout in which
// k_sp_spmm reads its operand and writes its result (rri_sparse_range_finder) ----
//
// Partial Gram matrices of Y: the panel is read ONCE (k_gram reads an m x len panel once per entry of G).  A workgroup stages
// TG_ROWS rows at a time in LDS (rows padded to 64 doubles, columns m..63 zero) and keeps a 64 x 64 accumulator in registers,
// thread (ta, tb) the entries (tb + 16 i, ta + 16 j): in a step all lanes read one row -- 16 consecutive doubles per j across ta
// (one 128-byte run per half wave, no bank shared) and 4 broadcast addresses per i.  Workgroup w takes the tiles w, w + grid, ...
// in that order and leaves its sum at part[w][64][64] (entries a <= b < m only; the lower half is never read): no atomics,
// the same bits on every run for a given grid.  (TG_ROWS = 32: rri_layout.hpp)
__global__ __launch_bounds__(256) void k_tall_gram_part(const double* __restrict__ Y, i64 rows, int m, double* __restrict__ part) {
    __shared__ double tile[TG_ROWS * 64];
    const int ta = threadIdx.x & 15, tb = threadIdx.x >> 4;
    for (int e = threadIdx.x; e < TG_ROWS * 64; e += 256) tile[e] = 0.0;
    double s[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[i][j] = 0.0;
    const i64 ntile = (rows + TG_ROWS - 1) / TG_ROWS;
    for (i64 t = blockIdx.x; t < ntile; t += gridDim.x) {
        const i64 r0 = t * TG_ROWS;
        const int nr = (int)((rows - r0) < (i64)TG_ROWS ? (rows - r0) : (i64)TG_ROWS);
        const double* src = Y + r0 * m;               // nr * m consecutive doubles
        __syncthreads();                              // the previous tile has been read (first round: the zero fill is done)
        for (int e = threadIdx.x; e < TG_ROWS * m; e += 256) {
            const int r = e / m, cc = e - r * m;
            tile[r * 64 + cc] = r < nr ? src[e] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < TG_ROWS; ++r) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = tile[r * 64 + tb + 16 * i]; b[i] = tile[r * 64 + ta + 16 * i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) s[i][j] = fma(a[i], b[j], s[i][j]);
        }
    }
    double* P = part + (i64)blockIdx.x * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = tb + 16 * i, b = ta + 16 * j;
            if (a <= b && b < m) P[a * 64 + b] = s[i][j];
        }
}

// G (m x m, row-major) = the partial Gram matrices added in workgroup order; both halves written from the one sum (as k_gram does)
__global__ __launch_bounds__(256) void k_tall_gram_sum(const double* __restrict__ part, int npart, int m, double* __restrict__ G) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m * m) return;
    const int a = e / m, b = e - a * m;
    if (a > b) return;
    const double s = ordered_sum<8>(part + a * 64 + b, 4096, 0, npart, 1);
    G[a * m + b] = s;
    G[b * m + a] = s;
}

// Y (rows x m, row-major) <- Y L^-T for a lower-triangular L, row by row: z L^T = y by forward substitution.  A wave holds
// TS_ROWS rows, lane = column: a row is m consecutive doubles, so its load and its store are one contiguous run per wave
// instruction, and TS_ROWS consecutive rows one run of TS_ROWS * m doubles.  Step j broadcasts z_j = v_j / L_jj from lane j
// (readlane) and every lane i > j subtracts L_ij z_j.  Lp is L as the host packed it for this access: Lp[j * 64 + i] = L_ij for
// j < i < m and 0 elsewhere (column j of the strictly lower part is one contiguous LDS read, and the lanes i <= j, whose entry is
// final or not begun, need no predicate), then Lp[4096 + i] = 1 / L_ii (0 for i >= m).  The quotient is a product with that
// reciprocal: an f64 division per step and row would be most of the kernel, and the Cholesky-QR passes that follow repair more
// than the one rounding it adds.
constexpr int TS_ROWS = 4;
__global__ __launch_bounds__(256) void k_tall_lsolve(double* __restrict__ Y, i64 rows, int m, const double* __restrict__ Lp) {
    __shared__ double Lsh[64 * 64 + 64];
    for (int e = threadIdx.x; e < 64 * 64 + 64; e += 256) Lsh[e] = Lp[e];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* invd = Lsh + 4096;
    const double inv_i = invd[lane];
    const i64 ngroup = (rows + TS_ROWS - 1) / TS_ROWS;
    for (i64 g = (i64)blockIdx.x * 4 + wave; g < ngroup; g += (i64)gridDim.x * 4) {
        const i64 r0 = g * TS_ROWS;
        double v[TS_ROWS];
#pragma unroll
        for (int u = 0; u < TS_ROWS; ++u) v[u] = (lane < m && r0 + u < rows) ? Y[(r0 + u) * m + lane] : 0.0;
        for (int j = 0; j < m; ++j) {
            const double l = Lsh[j * 64 + lane], dj = invd[j];
#pragma unroll
            for (int u = 0; u < TS_ROWS; ++u) v[u] = fma(-l, lane_get(v[u], j) * dj, v[u]);
        }
#pragma unroll
        for (int u = 0; u < TS_ROWS; ++u)
            if (lane < m && r0 + u < rows) Y[(r0 + u) * m + lane] = v[u] * inv_i;
    }
}

// out[t] = sum_{b < nb} part[t * stride + b], fixed order, one workgroup per t
__global__ __launch_bounds__(256) void k_rows_sum(const double* __restrict__ part, int nb, int stride, double* __restrict__ out) {
    __shared__ double scratch[40];
    double s = 0.0;
    s = ordered_sum<8>(part + (i64)blockIdx.x * stride, 1, threadIdx.x, nb, 256);
    s = block_sum(s, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// sum of a double vector -> out[0]; argmax (first index) -> out_idx[0].  One workgroup.
__global__ __launch_bounds__(1024) void k_vec_sum_argmax(const double* __restrict__ v, i64 n, double* out_sum,
                                                         i64* out_idx) {
    __shared__ double scratch[40];
    __shared__ double wm[16];
    __shared__ i64 wi[16];
    double s = 0.0, mx = -1.0e300;
    i64 mi = (i64)0x7fffffffffffffffLL;
    for (i64 i = threadIdx.x; i < n; i += blockDim.x) {
        const double x = v[i];
        s += x;
        if (x > mx) { mx = x; mi = i; }   // ascending i per thread: keeps the first index
    }
    s = block_sum(s, scratch);
    wave_argmax(mx, mi);
    if ((threadIdx.x & 63) == 0) { wm[threadIdx.x >> 6] = mx; wi[threadIdx.x >> 6] = mi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
            if (wm[w] > wm[0] || (wm[w] == wm[0] && wi[w] < wi[0])) { wm[0] = wm[w]; wi[0] = wi[w]; }
        if (out_sum) out_sum[0] = s;
        if (out_idx) out_idx[0] = wi[0];
    }
}

// 'max_resid_document' reset, step 1: row = max(X[mi,:] - W[mi,:] T, 0) (nmf.py:771,774)
template <typename SX>
__global__ __launch_bounds__(256) void k_reset_row(const SX* __restrict__ X, i64 ldx, const double* __restrict__ Wt,
                                                   i64 ldw, const double* __restrict__ T, i64 ldt, int d, int k,
                                                   const i64* __restrict__ mi_ptr, double* __restrict__ rowout,
                                                   const XScale xs) {
    const i64 mi = *mi_ptr;
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    double acc = 0.0;
    for (int l = 0; l < k; ++l) acc = fma(Wt[(i64)l * ldw + mi], T[(i64)l * ldt + j], acc);
    rowout[j] = fmax(x_elem(X, ldx, mi, j, xs) - acc, 0.0);
}
// step 2: T[t,:] = row ; W[:,t] = e_mi (nmf.py:774-776)
__global__ __launch_bounds__(256) void k_reset_commit(double* __restrict__ Wt, i64 ldw, double* __restrict__ T,
                                                      i64 ldt, int n, int d, int t, const i64* __restrict__ mi_ptr,
                                                      const double* __restrict__ rowin) {
    const i64 mi = *mi_ptr;
    const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
    if (idx < d) T[(i64)t * ldt + idx] = rowin[idx];
    if (idx < n) Wt[(i64)t * ldw + idx] = (idx == mi) ? 1.0 : 0.0;
}
// explicit reset vectors ('random', nmf.py:778-783): T[t,:] and W[:,t] from double buffers
__global__ __launch_bounds__(256) void k_set_row_col(double* __restrict__ Wt, i64 ldw, double* __restrict__ T,
                                                     i64 ldt, int n, int d, int t, const double* __restrict__ trow,
                                                     const double* __restrict__ wcolv) {
    const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
    if (trow && idx < d) T[(i64)t * ldt + idx] = trow[idx];
    if (wcolv && idx < n) Wt[(i64)t * ldw + idx] = wcolv[idx];
}

__global__ __launch_bounds__(256) void k_argmax_rows(const double* __restrict__ Wt, i64 ldw, int n, int k,
                                                     int* __restrict__ out) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double best = Wt[i];
    int bi = 0;
    for (int l = 1; l < k; ++l) {
        const double v = Wt[(i64)l * ldw + i];
        if (v > best) { best = v; bi = l; }
    }
    out[i] = bi;
}

// sum over listed entries of (clip((W T)_ij) - val)^2  (sklearn_interface.py:85-91,172-182)
__global__ __launch_bounds__(256) void k_masked_sqerr(const double* __restrict__ Wt, i64 ldw,
                                                      const double* __restrict__ T, i64 ldt, int k,
                                                      const i64* __restrict__ ij, const double* __restrict__ vals,
                                                      i64 count, double lo, double hi, double* __restrict__ out) {
    __shared__ double scratch[40];
    double s = 0.0;
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < count; e += (i64)gridDim.x * 256) {
        const i64 i = ij[2 * e], j = ij[2 * e + 1];
        double acc = 0.0;
        for (int l = 0; l < k; ++l) acc = fma(Wt[(i64)l * ldw + i], T[(i64)l * ldt + j], acc);
        double pr = acc < lo ? lo : (acc > hi ? hi : acc);
        const double df = pr - vals[e];
        s += df * df;
    }
    s = block_sum(s, scratch);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// 2-D copy with type conversion (host staging -> padded device layout); TRANSPOSE: dst[c][r] = src[r][c]
template <typename Src, typename Dst, bool TRANSPOSE>
__global__ __launch_bounds__(256) void k_convert2d(const Src* __restrict__ src, i64 lds_, Dst* __restrict__ dst,
                                                   i64 ldd, i64 rows, i64 cols) {
    const i64 total = rows * cols;
    for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
        if (TRANSPOSE) {   // idx runs along the DESTINATION rows (coalesced writes)
            const i64 c = idx / rows, r = idx - c * rows;
            dst[c * ldd + r] = (Dst)src[r * lds_ + c];
        } else {
            const i64 r = idx / cols, c = idx - r * cols;
            dst[r * ldd + c] = (Dst)src[r * lds_ + c];
        }
    }
}

// Upload of a float16 X: dst = half(src), rounded to nearest even in ONE step from the host type (the double -> _Float16 cast is
// a single rounding: double -> float -> half would double-round, 1 + 2^-11 + 2^-30 -> 1.0 where numpy's astype gives 1 + 2^-10),
// and what the rounding cost: part[3 b ..] = {sum (x - half(x))^2, sum x^2, values not finite once rounded (|x| >= 65520, inf,
// NaN)} of block b, float64, every thread's terms in index order and the block's sum in a fixed order.
template <typename Src>
__global__ __launch_bounds__(256) void k_store_half(const Src* __restrict__ src, i64 lds_, _Float16* __restrict__ dst, i64 ldd,
                                                    i64 rows, i64 cols, double* __restrict__ part) {
    __shared__ double scratch[40];
    const i64 total = rows * cols;
    double se = 0.0, sx = 0.0, bad = 0.0;
    for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
        const i64 r = idx / cols, c = idx - r * cols;
        const Src x = src[r * lds_ + c];
        const _Float16 h = (_Float16)x;
        dst[r * ldd + c] = h;
        const double xd = (double)x, hd = (double)(float)h;
        if (fabs(hd) <= 65504.0) {            // finite (false for inf and NaN)
            const double e = xd - hd;
            se = fma(e, e, se);
            sx = fma(xd, xd, sx);
        } else bad += 1.0;
    }
    se = block_sum(se, scratch);
    sx = block_sum(sx, scratch);
    bad = block_sum(bad, scratch);
    if (threadIdx.x == 0) { part[3 * blockIdx.x] = se; part[3 * blockIdx.x + 1] = sx; part[3 * blockIdx.x + 2] = bad; }
}

// Upload of a uint8 X from a floating host type: dst = the value as a byte, and part[b] = how many values of block b are not
// integers in 0..255 (fractions, negatives, inf, NaN: the comparison is false for NaN).  Nothing is rounded: one such value fails
// the upload.
template <typename Src>
__global__ __launch_bounds__(256) void k_store_u8(const Src* __restrict__ src, i64 lds_, unsigned char* __restrict__ dst, i64 ldd,
                                                  i64 rows, i64 cols, double* __restrict__ part) {
    __shared__ double scratch[40];
    const i64 total = rows * cols;
    double bad = 0.0;
    for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
        const i64 r = idx / cols, c = idx - r * cols;
        const double x = (double)src[r * lds_ + c];
        const bool good = x >= 0.0 && x <= 255.0 && x == floor(x);
        dst[r * ldd + c] = good ? (unsigned char)(int)x : (unsigned char)0;
        if (!good) bad += 1.0;
    }
    bad = block_sum(bad, scratch);
    if (threadIdx.x == 0) part[blockIdx.x] = bad;
}

// vec[0 .. total) = value (the scale vectors of an RRI_U8 handle start as ones, pad columns included)
__global__ __launch_bounds__(256) void k_fill(double* __restrict__ vec, i64 total, double value) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < total) vec[i] = value;
}
// Row normalisation of an RRI_U8 handle: Ypart holds the row totals sum_j c_ij cscale_j rscale_i as panels (the pass against a row
// of ones).  inv_i = 1 / (tot_i + spacing(1)); rows with a total below 1e-10 are counted (nzero) and nothing is written for
// them.  APPLY: rscale_i *= inv_i -- launched only once the count came back zero.
template <bool APPLY>
__global__ __launch_bounds__(256) void k_row_scale_update(const double* __restrict__ Ypart, int npanels, int n,
                                                          double* __restrict__ rscale, unsigned long long* __restrict__ nzero) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double xs = 0.0;
    xs = ordered_sum<8>(Ypart + i, n, 0, npanels, 1);
    xs += 2.220446049250313e-16;                      // np.spacing(1), matrixops.py:140
    if constexpr (APPLY) rscale[i] *= 1.0 / xs;
    else if (xs < 1e-10) atomicAdd(nzero, 1ull);
}
// cscale[j] *= s[j], j < d
__global__ __launch_bounds__(256) void k_vec_mul(double* __restrict__ v, const double* __restrict__ s, i64 len) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < len) v[i] *= s[i];
}

// plain 16-byte streaming copy: the achievable-HBM yardstick measured beside the pass kernel
// diagnostics: which XCD (accelerator complex die) each workgroup of a launch on this stream lands on -- out[blockIdx] = XCC_ID
__global__ __launch_bounds__(64) void k_xcc_probe(int* __restrict__ out) {
    unsigned v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    if (threadIdx.x == 0) out[blockIdx.x] = (int)(v & 0xfu);
}

__global__ __launch_bounds__(256) void k_stream_copy(const float4* __restrict__ src, float4* __restrict__ dst, i64 nvec) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (i64)gridDim.x * 256) dst[i] = src[i];
}

}  // namespace rri
