// rri_rank_kernels.hpp -- k_rank_entries: the rank of listed columns in the total order of W T's rows, scores and counting in one
// launch (DESIGN "Ranks of entries"; the order, the predicates and the pieces are rri_rank.hpp's).
//
// The scoring walk is k_topn_rows': a 256-thread workgroup takes 64 PIECES (a request's row and at most RANK_SEG = 64 of its
// targets), wave w the pieces 16 w .. 16 w + 15 of them; d in chunks of 64 columns, four 16 x 16 tiles per wave and chunk,
// v_mfma_f64_16x16x4_f64 over k in panels of TOPN_KP, the panel's T tile shared through LDS, W gathered through the row list,
// zeros beyond k, d and the piece count.  The walk is done TWICE by the same code (score_chunk), so that a target's own score is
// produced by the instruction sequence and panel order that produce the scores it is compared with:
//   walk 1  visits only the chunks that hold a target of the workgroup and keeps the targets' scores in LDS.  Per visited chunk
//           lane p marks, for each of its wave's pieces, target p in a 64-byte slot row (the target's index at its column) when
//           the column is inside the chunk; a lane whose score sits on a marked column stores it.  The next chunk to visit is the
//           smallest chunk behind this one that holds a target: a minimum over the same 16 reads, across the waves through LDS.
//   walk 2  visits every chunk and counts.  Lane p owns target p of each of the wave's 16 pieces: 16 counters in registers.  For
//           result register r and target index e every lane reads target e of ITS row (an LDS broadcast among the 16 lanes that
//           share the row) and asks rank_counts for each of its four tiles; one ballot per tile, and lane e adds the popcount of
//           each 16-bit quarter of it to its counter of row quarter + 4 r.  Integers and no atomics: the counts do not depend on
//           any order of arrival.  e runs to the longest target list among the wave's pieces; the slots behind a piece's targets
//           hold (NaN, -1), against which nothing counts.
// Exclusion (walk 2).  The segment ascends and so does the walk: every piece keeps a cursor into its segment.  Per chunk the
// wave's lanes read the next up to 64 entries, mark those inside the chunk in the piece's 64-byte flag row (the slot rows of
// walk 1, reused) and move the cursor on by their number: work per piece is its segment's length plus the number of chunks, and
// a score's eligibility is one LDS read and v == v.  NaN scores outside the exclusion are counted per piece:
// eligible = d - |segment| - that count, reported by a request's first piece.  Whether a TARGET is excluded is asked once per
// target at the end (topn_excluded).  The segment of a request is row req of the exclusion CSR, or -- erow given -- row erow[req] of
// any CSR pattern: a resident corpus of the handle's shape, read where it lies (rri_corpus_rank.hpp).
//
// Who may touch what in LDS: the rows of a piece (scores, columns, slots / flags, cursor) belong to the piece's wave alone.  A
// row is cleared at the top of a chunk's step, marked between the two barriers of the chunk's first panel and read after the
// last panel, so the barriers the T tile needs anyway separate clear, mark and read.
//
// 69 KiB of LDS let two workgroups share a CU; the second launch bound keeps the registers inside that (246 VGPRs, no scratch).
#pragma once

#include "rri_rank.hpp"
#include "rri_topn_kernels.hpp"

namespace rri {

constexpr int RANK_PIECES = TOPN_ROWS;     // pieces per workgroup

// dynamic LDS: the T tile (16 KiB), the targets' scores (32 KiB) and columns (16 KiB), the slot / flag rows (4 KiB), the
// exclusion cursors and segment ends (1 KiB), the waves' next chunks
inline size_t rank_lds_bytes() {
    return (size_t)TOPN_KP * TOPN_COLS * 8 + (size_t)RANK_PIECES * RANK_SEG * (8 + 4) + (size_t)RANK_PIECES * TOPN_COLS +
           (size_t)RANK_PIECES * 16 + 16;
}

__global__ __launch_bounds__(256, 2) void k_rank_entries(const double* __restrict__ Wt, i64 ldw, const double* __restrict__ T, i64 ldt,
                                                      int d, int k, const i64* __restrict__ rows, const RankPiece* __restrict__ pieces,
                                                      i64 npieces, const int* __restrict__ tidx, const i64* __restrict__ eptr,
                                                      const int* __restrict__ eidx, const i64* __restrict__ erow, double lo, double hi,
                                                      int* __restrict__ rank_out, double* __restrict__ val_out,
                                                      int* __restrict__ elig_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* tsh = reinterpret_cast<double*>(smem);                             // [TOPN_KP][TOPN_COLS]
    double* tsc = tsh + TOPN_KP * TOPN_COLS;                                   // [RANK_PIECES][RANK_SEG] scores of the targets
    int* tcol = reinterpret_cast<int*>(tsc + RANK_PIECES * RANK_SEG);          // [RANK_PIECES][RANK_SEG] their columns
    unsigned char* flag = reinterpret_cast<unsigned char*>(tcol + RANK_PIECES * RANK_SEG);   // [RANK_PIECES][TOPN_COLS]
    i64* ecur = reinterpret_cast<i64*>(flag + RANK_PIECES * TOPN_COLS);        // [RANK_PIECES] cursor into the exclusion segment
    i64* eend = ecur + RANK_PIECES;                                            // [RANK_PIECES] its end
    int* wnext = reinterpret_cast<int*>(eend + RANK_PIECES);                   // [4] walk 1: a wave's next chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const i64 p0 = (i64)blockIdx.x * RANK_PIECES + wave * 16;                  // the wave's first piece
    const double nan = __builtin_nan("");
    constexpr int NOCHUNK = 0x7fffffff;

    // the wave's 16 pieces: lane p takes target p of each; the cursors of their exclusion segments
    int emax = 0;
    for (int r = 0; r < 16; ++r) {
        const int pl = wave * 16 + r;
        int cnt = 0;
        i64 t0 = 0, req = 0;
        if (p0 + r < npieces) { cnt = pieces[p0 + r].cnt; t0 = pieces[p0 + r].t0; req = pieces[p0 + r].req; }
        emax = cnt > emax ? cnt : emax;
        tcol[pl * RANK_SEG + lane] = lane < cnt ? tidx[t0 + lane] : -1;
        tsc[pl * RANK_SEG + lane] = nan;
        if (lane == 0) {
            const bool seg = eptr && p0 + r < npieces;
            const i64 er = (seg && erow) ? erow[req] : req;                  // the exclusion's row that serves the request
            ecur[pl] = seg ? eptr[er] : 0;
            eend[pl] = seg ? eptr[er + 1] : 0;
        }
    }
    // a cleared slot row holds 0xff (no target at the column), a cleared flag row 0 (not excluded); thread -> its own 16 bytes,
    // which lie in a row of its own wave
    auto clear_rows = [&](unsigned v) {
        uint4* p = reinterpret_cast<uint4*>(flag) + tid;
        *p = make_uint4(v, v, v, v);
    };

    // A operand: lane holds W[row lr][4 s + lk] of the panel; the row it gathers
    const bool arow_ok = p0 + lr < npieces;
    i64 arow = 0;
    if (arow_ok) { const i64 req = pieces[p0 + lr].req; arow = rows ? rows[req] : req; }
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
    const int tc = tid & 63, tr = tid >> 6;
    // the scores of the chunk at c0: k_topn_rows' walk.  `between` runs between the two barriers of the first panel.
    auto score_chunk = [&](i64 c0, f64x4* acc, auto&& between) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int pan = 0; pan < npan; ++pan) {
            const int k0 = pan * TOPN_KP;
            const int kn = k - k0 < TOPN_KP ? k - k0 : TOPN_KP;               // rows of T in this panel
            const int ks = (kn + 3) >> 2;                                     // its k-steps
            __syncthreads();                                                  // the tile of the step before has been read
#pragma unroll
            for (int i = 0; i < TOPN_KP / 4; ++i) {
                const int l = tr + 4 * i;
                if (l < 4 * ks) tsh[l * TOPN_COLS + tc] = (l < kn && c0 + tc < d) ? T[(i64)(k0 + l) * ldt + c0 + tc] : 0.0;
            }
            if (npan > 1) load_a(k0);
            if (pan == 0) between();
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
    };

    // ---- walk 1: the targets' scores ---------------------------------------------------------------------------------------
    // marks the wave's targets inside [c0, c0 + 64) (c0 < 0: none) and posts the wave's first chunk at or behind `from`
    auto mark_targets = [&](i64 c0, i64 from) {
        int nxt = NOCHUNK;
        for (int r = 0; r < 16; ++r) {
            const int pl = wave * 16 + r;
            const int tj = tcol[pl * RANK_SEG + lane];
            if (c0 >= 0 && tj >= c0 && tj < c0 + TOPN_COLS) flag[pl * TOPN_COLS + (tj - (int)c0)] = (unsigned char)lane;
            if (tj >= from && (tj >> 6) < nxt) nxt = tj >> 6;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(nxt, o);
            nxt = other < nxt ? other : nxt;
        }
        if (lane == 0) wnext[wave] = nxt;
    };
    auto next_chunk = [&]() {
        int c = wnext[0];
        for (int w = 1; w < 4; ++w) c = wnext[w] < c ? wnext[w] : c;
        return c;
    };
    mark_targets(-1, 0);
    __syncthreads();
    int chunk = next_chunk();
    while (chunk != NOCHUNK) {
        const i64 c0 = (i64)chunk * TOPN_COLS;
        f64x4 acc[4];
        clear_rows(0xffffffffu);
        score_chunk(c0, acc, [&]() { mark_targets(c0, c0 + TOPN_COLS); });
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pl = wave * 16 + lk + 4 * r;
                const unsigned sl = flag[pl * TOPN_COLS + 16 * c + lr];
                if (sl < (unsigned)RANK_SEG) tsc[pl * RANK_SEG + sl] = acc[c][r];
            }
        }
        chunk = next_chunk();          // posted before the chunk's second barrier; rewritten behind the next chunk's first
    }

    // ---- walk 2: count ------------------------------------------------------------------------------------------------------
    int cnt[16];          // lane p: what stands before target p of the wave's piece r
    int nanl[4];          // the lane's own NaN scores outside the exclusion, by result register
#pragma unroll
    for (int r = 0; r < 16; ++r) cnt[r] = 0;
    bool pvalid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { nanl[r] = 0; pvalid[r] = p0 + lk + 4 * r < npieces; }
    clear_rows(0u);
    for (i64 c0 = 0; c0 < d; c0 += TOPN_COLS) {
        f64x4 acc[4];
        if (eptr) clear_rows(0u);
        score_chunk(c0, acc, [&]() {
            if (!eptr) return;
            for (int r = 0; r < 16; ++r) {
                const int pl = wave * 16 + r;
                const i64 cur = ecur[pl], e1 = eend[pl];
                if (cur >= e1) continue;                                      // uniform: the segment is used up (or there is none)
                const int ej = cur + lane < e1 ? eidx[cur + lane] : -1;
                const bool in = ej >= c0 && ej < c0 + TOPN_COLS;
                if (in) flag[pl * TOPN_COLS + (ej - (int)c0)] = 1;
                const int took = __popcll(__ballot(in));
                if (lane == 0) ecur[pl] = cur + took;
            }
        });
        // the competitors: a score that is not open (beyond d or the pieces, or excluded) is NaN here and competes with nothing
        double sc[4][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double v = acc[c][r];
                const int j = (int)c0 + 16 * c + lr;
                const bool open = j < d && pvalid[r] && flag[(wave * 16 + lk + 4 * r) * TOPN_COLS + 16 * c + lr] == 0;
                nanl[r] += (open && v != v) ? 1 : 0;
                sc[c][r] = open ? v : nan;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pl = wave * 16 + lk + 4 * r;
#pragma unroll 2
            for (int e = 0; e < emax; ++e) {
                const double ts = tsc[pl * RANK_SEG + e];
                const int tj = tcol[pl * RANK_SEG + e];
                int pc[4] = {0, 0, 0, 0};                                     // uniform: the four tiles' counts by quarter
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int j = (int)c0 + 16 * c + lr;
                    const unsigned long long b = __ballot(rank_counts(sc[c][r], j, ts, tj));
#pragma unroll
                    for (int q = 0; q < 4; ++q) pc[q] += __popc((unsigned)(b >> (16 * q)) & 0xffffu);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) cnt[q + 4 * r] += lane == e ? pc[q] : 0;
            }
        }
    }
    // the NaN count of a piece: over the 16 lanes that share its row
#pragma unroll
    for (int r = 0; r < 4; ++r)
        for (int o = 8; o > 0; o >>= 1) nanl[r] += __shfl_xor(nanl[r], o);

    // what leaves: lane p writes target p of each of the wave's pieces; a request's first piece its eligible count
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (p0 + r < npieces) {                                              // uniform: every lane of the wave is here
            const RankPiece pc = pieces[p0 + r];
            const int pl = wave * 16 + r;
            const i64 er = (eptr && erow) ? erow[pc.req] : pc.req;
            const i64 e0 = eptr ? eptr[er] : 0, e1 = eptr ? eptr[er + 1] : 0;
            const int nanr = __shfl(nanl[r >> 2], (r & 3) * 16);
            if (lane < pc.cnt) {
                const double ts = tsc[pl * RANK_SEG + lane];
                const int tj = tcol[pl * RANK_SEG + lane];
                const bool excluded = eptr && topn_excluded(eidx, e0, e1, tj);
                rank_out[pc.t0 + lane] = rank_result(cnt[r], ts, excluded);
                val_out[pc.t0 + lane] = rank_value(ts, excluded, lo, hi);
            }
            if (lane == 0 && pc.first && elig_out) elig_out[pc.req] = d - (int)(e1 - e0) - nanr;
        }
    }
}

}  // namespace rri
