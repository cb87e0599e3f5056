// rri_topn_kernels.hpp -- k_topn_rows: the N best columns of W T for a list of rows, scores and selection in one launch
// (DESIGN "Top-N rows"; the order, the exclusion search and the clip are rri_topn.hpp's).
//
// One 256-thread workgroup takes 64 requested rows, wave w the rows 16 w .. 16 w + 15 of them.  It walks d in chunks of 64
// columns; a chunk's scores are four 16 x 16 tiles per wave, v_mfma_f64_16x16x4_f64 over k in steps of 4 (operand and result
// layouts as in k_resid_mfma).  k is taken in panels of TOPN_KP = 32: the A fragments of a panel (W is stored transposed, a
// gathered row reads W[t ldw + rows[r]]) are 8 doubles per lane -- with k <= 32 they are loaded once and stay for the whole
// walk, with more they are reloaded per chunk and panel from L2 --, and the panel's T tile (32 x 64 doubles, contiguous rows of
// T) is shared by the four waves through LDS.  Zeros stand in for k .. 4 ceil(k / 4) and for the rows and columns that are
// not there.
//
// Selection.  Every row keeps its N best (score, column) in LDS, sorted, empty slots (-1, NaN) behind the filled ones.  A list
// belongs to ONE wave, and lane p of that wave is the only thread that ever reads or writes slot p of it (N <= 64 = the lanes
// of a wave), so no list needs a barrier or an atomic.  The last slot of each of a lane's four rows is mirrored in registers:
// a score that does not enter (topn_enters) costs one compare.  The lanes whose score would enter are found with a ballot and
// taken one after the other by the whole wave: the candidate's score comes by a lane read, its row's current last slot is
// asked again (an earlier candidate of the same ballot may have moved it), the row's exclusion segment is searched -- halved
// until at most 64 entries are left, which the lanes compare at once --, and the insertion is one step: every lane asks
// whether its slot stays ahead of the candidate, the count of those that do is the candidate's place, the slots behind take
// their left neighbour's content by a lane shift.  About N ln(d / N) insertions per row, so serial per wave is cheap.
// The exclusion is a CSR pattern with one row per request, or -- erow given -- any CSR pattern of which request q reads row
// erow[q]: a resident corpus of the handle's shape, read where it lies through the row list (rri_corpus_rank.hpp).
#pragma once

#include "rri_topn.hpp"

namespace rri {

constexpr int TOPN_ROWS = 64;    // requested rows per workgroup
constexpr int TOPN_COLS = 64;    // columns per chunk
constexpr int TOPN_KP = 32;      // k-panel depth

// dynamic LDS: the T tile, then the lists' values, then their columns
inline size_t topn_lds_bytes(int N) { return (size_t)TOPN_KP * TOPN_COLS * 8 + (size_t)TOPN_ROWS * N * (8 + 4); }

__global__ __launch_bounds__(256) void k_topn_rows(const double* __restrict__ Wt, i64 ldw, const double* __restrict__ T, i64 ldt,
                                                   int d, int k, const i64* __restrict__ rows, i64 count, int N,
                                                   const i64* __restrict__ eptr, const int* __restrict__ eidx,
                                                   const i64* __restrict__ erow, double lo, double hi, int* __restrict__ idx_out,
                                                   double* __restrict__ val_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* tsh = reinterpret_cast<double*>(smem);                         // [TOPN_KP][TOPN_COLS]
    double* lv = tsh + TOPN_KP * TOPN_COLS;                                // [TOPN_ROWS][N]
    int* lj = reinterpret_cast<int*>(lv + (size_t)TOPN_ROWS * N);          // [TOPN_ROWS][N]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const i64 q0 = (i64)blockIdx.x * TOPN_ROWS + wave * 16;                // the wave's first request
    const double nan = __builtin_nan("");

    // the wave's 16 lists start empty (lane p: slot p of each)
    if (lane < N)
        for (int r = 0; r < 16; ++r) { lv[(wave * 16 + r) * N + lane] = nan; lj[(wave * 16 + r) * N + lane] = -1; }
    // the last slot of the lane's rows lk + 4 r, mirrored
    double thv[4] = {nan, nan, nan, nan};
    int thj[4] = {-1, -1, -1, -1};

    // A operand: lane holds W[row lr][4 s + lk] of the panel; the row it gathers
    const bool arow_ok = q0 + lr < count;
    const i64 arow = arow_ok ? (rows ? rows[q0 + lr] : q0 + lr) : 0;
    constexpr int KS = TOPN_KP / 4;
    const int npan = (k + TOPN_KP - 1) / TOPN_KP;
    double afrag[KS];
    auto load_a = [&](int k0) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int l = k0 + 4 * s + lk;
            afrag[s] = (arow_ok && l < k) ? Wt[(i64)l * ldw + arow] : 0.0;
        }
    };
    if (npan == 1) load_a(0);
    // cooperative load of a T tile: thread -> column tid & 63, rows (tid >> 6) + 4 i
    const int tc = tid & 63, tr = tid >> 6;

    for (i64 c0 = 0; c0 < d; c0 += TOPN_COLS) {
        f64x4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int pan = 0; pan < npan; ++pan) {
            const int k0 = pan * TOPN_KP;
            const int kn = k - k0 < TOPN_KP ? k - k0 : TOPN_KP;           // rows of T in this panel
            const int ks = (kn + 3) >> 2;                                 // its k-steps
            __syncthreads();                                              // the tile of the step before has been read
#pragma unroll
            for (int i = 0; i < TOPN_KP / 4; ++i) {
                const int l = tr + 4 * i;
                if (l < 4 * ks) tsh[l * TOPN_COLS + tc] = (l < kn && c0 + tc < d) ? T[(i64)(k0 + l) * ldt + c0 + tc] : 0.0;
            }
            if (npan > 1) load_a(k0);
            __syncthreads();
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (s < ks) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const double b = tsh[(4 * s + lk) * TOPN_COLS + 16 * c + lr];
                        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(afrag[s], b, acc[c], 0, 0, 0);
                    }
                }
            }
        }
        // selection: result register r of tile c is row lk + 4 r, column c0 + 16 c + lr
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = acc[c][r];
                const int j = (int)c0 + 16 * c + lr;
                const bool cand = j < d && q0 + lk + 4 * r < count && topn_enters(v, j, thv[r], thj[r]);
                unsigned long long todo = __ballot(cand);
                while (todo) {
                    const int b = __ffsll((long long)todo) - 1;           // uniform: the candidate's lane
                    todo &= todo - 1;
                    const double cv = __shfl(v, b);
                    const int cj = (int)c0 + 16 * c + (b & 15);
                    const int row = (b >> 4) + 4 * r;                     // of the wave's 16
                    if (!topn_enters(cv, cj, __shfl(thv[r], b), __shfl(thj[r], b))) continue;
                    if (eptr) {
                        const i64 er = erow ? erow[q0 + row] : q0 + row;   // the exclusion's row that serves the request
                        i64 e0 = eptr[er], e1 = eptr[er + 1];
                        while (e1 - e0 > 64) {                            // halve; the half kept can still hold cj
                            const i64 mid = e0 + (e1 - e0) / 2;
                            if (eidx[mid] < cj) e0 = mid + 1;
                            else e1 = mid + 1;
                        }
                        if (__ballot(e0 + lane < e1 && eidx[e0 + lane] == cj)) continue;
                    }
                    // one step: the candidate's place is the number of slots that stay ahead of it
                    double* rv = lv + (wave * 16 + row) * N;
                    int* rj = lj + (wave * 16 + row) * N;
                    const double ov = lane < N ? rv[lane] : nan;
                    const int oj = lane < N ? rj[lane] : -1;
                    const int pos = __popcll(__ballot(lane < N && topn_stays_ahead(ov, oj, cv, cj)));
                    const double uv = __shfl_up(ov, 1);
                    const int uj = __shfl_up(oj, 1);
                    const double nv = lane == pos ? cv : (lane > pos ? uv : ov);
                    const int nj = lane == pos ? cj : (lane > pos ? uj : oj);
                    if (lane < N && lane >= pos) { rv[lane] = nv; rj[lane] = nj; }
                    const double lastv = __shfl(nv, N - 1);
                    const int lastj = __shfl(nj, N - 1);
                    if (lk == (b >> 4)) { thv[r] = lastv; thj[r] = lastj; }
                }
            }
        }
    }
    // what leaves: lane p writes slot p of each of the wave's lists, the values clipped
    if (lane < N)
        for (int r = 0; r < 16; ++r) {
            if (q0 + r >= count) break;
            const double v = lv[(wave * 16 + r) * N + lane];
            const int j = lj[(wave * 16 + r) * N + lane];
            idx_out[(q0 + r) * N + lane] = j;
            val_out[(q0 + r) * N + lane] = j >= 0 ? topn_clip(v, lo, hi) : nan;
        }
}

}  // namespace rri
