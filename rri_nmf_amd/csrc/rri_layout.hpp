// rri_layout.hpp -- everything a handle decides about its shape: plain integer arithmetic on n, d, k, the storage type, the
// flavour, the CU count and the environment switches.  Host-only: no HIP header, no rri_ctx, no getenv, so a plain host compiler
// builds it (tests/c/layout_main.cpp, tests/test_layout_cpu.py) and the rules run on a machine without a device.  rri_hip.hip
// copies the results into the handle, allocates and launches; the kernel headers take from here the constants they share with
// the host (row and column tile sizes, the work item of the blocked store).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "rri_early_deal.hpp"
#include "rri_hip.h"

namespace rri {

typedef long long i64;
inline i64 round_up(i64 a, i64 b) { return (a + b - 1) / b * b; }

// ---- storage widths ----------------------------------------------------------------------------------------------------
constexpr size_t dtype_size(int dt) { return dt == RRI_F32 ? 4 : dt == RRI_F64 ? 8 : dt == RRI_F16 ? 2 : dt == RRI_U8 ? 1 : 0; }
// elements per load: 4, 2, 8 (float16) of a 16-byte load; uint8: 8 of an 8-byte load (rri_hip.hip asserts XVec<SX>::N per type)
constexpr int load_elems(int dt) { return dt == RRI_U8 ? 8 : dtype_size(dt) ? (int)(16 / dtype_size(dt)) : 0; }
constexpr int load_bytes(int dt) { return load_elems(dt) * (int)dtype_size(dt); }

// ---- constants the kernels share with the host -------------------------------------------------------------------------
constexpr int WCOL_TILES = 1;   // 64-row tiles per k_wcol block (1 = most blocks in flight)
constexpr int GRAM_SLICES = RRI_GRAM_SLICES;  // k_reduce sums the Gpart rows in this many slices; consumers add the slices
constexpr int TG_ROWS = 32;     // rows of a tall matrix k_tall_gram_part stages in LDS at a time
constexpr int SP_BLOCK_BYTES = 120 * 1024;   // LDS of the factor tables of one block of the blocked segment store (rri_sparse_kernels.hpp)
constexpr i64 spx_block_cap() { return (i64)(SP_BLOCK_BYTES / 8 - 64) / 64 * 64; }   // X on CSR: ONE table of float64 factors per block
struct SpWork { int blk, s0, s1, pad; };   // one workgroup: segments [s0, s1) of block blk
constexpr int ONCHIP_THREADS = 512, ONCHIP_WAVES = ONCHIP_THREADS / 64;
constexpr int ONCHIP_SMALL_K = 22;    // k + 2 Gram entries = 8 waves x 3 in flight: one round of loads in phase A (KT = 3)
constexpr int ONCHIP_MAX_K = 64;      // KT = 8: two rounds beyond k = 46
constexpr int ONCHIP_CWA = 32;          // columns of T per worker
constexpr int ONCHIP_PG = ONCHIP_THREADS / ONCHIP_CWA;   // groups of workgroup partials in the column-sum reduction

// What of the 256 MiB Infinity Cache the default-policy traffic of one topic step may fill, in MB (1e6 bytes): the chain's own
// working set and, in what is left, a fixed part of X (pass_keep).  Chosen on sweeps/s by tools/pass_keep_probe.py.
constexpr double PASS_CACHE_MB = 256.0;
// the most rows a workgroup of the read-only pass walks on a dense fp32 handle of the Gram form: the size that streams the packed copy of X (dense_plan)
constexpr int PK_ROWS_MAX = 512;

// The environment switches a handle keeps: read once, by rri_create (read_switches in rri_hip.hip), so that a handle created
// later under another environment cannot change the schedule of one that is already running (INTEGRATION.md lists them)
struct rri_switches {
    bool onchip = true;        // RRI_ONCHIP=0: never the register-resident persistent sweep (rri_onchip_kernels.hpp)
    bool onchip_obj = true;    // RRI_ONCHIP_OBJ=0: the persistent sweep does not leave the objective of its last sweep (rri_objective takes the Gram kernels)
    bool wsweep = true;        // RRI_WSWEEP=0: runs with T fixed take the launch-per-topic W half (k_tgram, k_wcol, k_check_wcol per topic)
    bool trow_fused = true;    // RRI_TROW_SMALL=0: launch-bound sizes keep k_reduce and k_trow_numer apart (never k_trow_small): the route of a
                               // row-sharded handle and of one with frozen statistics
    bool obj_direct = false;   // RRI_OBJ_DIRECT=1: the objective always through the residual (k_resid)
    bool wmcorr_cols = true;   // RRI_WMCORR_COLS=0: the mask-only correction always walks every bit (k_wmcorr), also on a sparse mask
    bool wnw_mask = true;      // RRI_WNW_MASK=0: the one-pass step keeps taking nw = (w^2)^T M in the read-modify-write pass on a sparse 0/1 mask too
    int pass_rot = -1;         // RRI_PASS_ROT=0..7: rotate the tiles of the passes inside every group of 8 workgroups (another XCD per tile) by this
                               // much; unset: the handle's own calibrated 0 or 1 (calibrate_rot)
    int rot_cal = 1;           // RRI_ROT_CAL=0: no calibration, rotation 0; 1: rotations {0, 1}; n > 1: rotations 0 .. n-1
    bool rot_debug = false;    // RRI_ROT_DEBUG (set): calibrate_rot prints its timings
    bool mask_bits = true;     // RRI_MASK_BITS=0: a 0/1 mask stays an fp array (no bit-packed copy)
    double pass_cache_mb = PASS_CACHE_MB;   // RRI_PASS_CACHE_MB: what of the Infinity Cache a topic step may fill (pass_keep); 0: all of X streams
    int pk_rows = 0;           // RRI_PASS_PK_GEOM=<rows>[i|c] (diagnostics): rows per workgroup of the read-only pass (rounded up to 16, at most the
    int pk_il = -1;            // LDS cap) and interleaved (i) or contiguous (c) chunks, for dense fp32 handles of the Gram form (dense_plan)
    int x_pack = -1;           // RRI_X_PACK: the packed copy of an fp32 X for the read-only pass (xpack_ensure): 0 never, 1 the 28-bit copy
                               // wherever the pass can read it, 2 the 26-bit copy there (rri_xnarrow.hpp), unset: where X does not fit
                               // the budget of pass_keep, the 26-bit copy if few elements are exceptions (xnarrow_build), else the 28-bit
    bool early_sums = true;    // RRI_EARLY_SUMS=0: the W-sized sums of a topic step stay in k_wcol after the pass (never the early job
                               // in the pass's grid, k_wfin and k_trow_early)
    bool early_deal = false;   // RRI_EARLY_DEAL=1: the early job's workgroups are dealt through the pass's grid behind its first round
                               // (rri_early_deal.hpp), not placed there in one contiguous run; no sum depends on it, and at the
                               // flagship shape the pass takes the same time either way
};

// ---- the blocked store of a CSR pattern: dimensions ----------------------------------------------------------------------
// The two blocked copies (rri_sparse_kernels.hpp): which = 0 rows as segments, cut into column blocks (= Ypart panels); 1 columns
// as segments, cut into row blocks (= Zpart rows).  Block widths so that three factor tables of a block fit SP_BLOCK_BYTES of
// LDS (X on CSR: ONE table of float64 factors per block, spx_block_cap -- k_spx_pass).
struct SpDims { int nblk = 1, bw = 1; i64 nseg = 0, gdim = 0; };
inline SpDims sp_dims(i64 n, i64 d, int which, bool sparse_x, size_t es) {
    const i64 block_bytes = SP_BLOCK_BYTES;
    const i64 cap = sparse_x ? std::min<i64>(spx_block_cap(), std::max<i64>(64, (block_bytes / 8 - 64) / 64 * 64))
                             : block_bytes / (3 * (i64)es);
    SpDims s;
    s.gdim = which == 0 ? d : n;
    s.nseg = which == 0 ? n : d;
    s.nblk = (int)((s.gdim + cap - 1) / cap);
    s.bw = (int)round_up((s.gdim + s.nblk - 1) / s.nblk, 64);
    return s;
}
// work items per copy: the pattern-only handle runs a copy per launch, one item per CU; with X on CSR one launch runs the items
// of both copies, half of the chip's CUs each, so that all of them are ONE round of workgroups
inline int sp_target_items(int n_cu, bool sparse_x) { return std::max(1, sparse_x ? n_cu / 2 : n_cu); }

// ---- the dense plan ------------------------------------------------------------------------------------------------------
// read-only passes deal their row blocks as interleaved chunks only while the launch has few workgroups (the passes that write
// the matrix back always do): ONE predicate for the launch sites and for rri_layout_info
inline bool ro_pass_interleaved(int ro_il, int npanels, int nrb) { return ro_il >= 0 ? ro_il != 0 : npanels * nrb <= 1024; }
// the dense weighted T-row step whose partial sums fit ONE launch (k_wtrow_small): one device, few row blocks
inline bool wtrow_small(bool has_comm, int nrb) { return !has_comm && nrb <= 64; }

struct DensePlan {
    i64 n = 0, d = 0, LD = 0;
    int k = 0, dtype = RRI_F32, weighted = 0;     // weighted: the flavour of the algorithm (the two storage flavours are RRI_UNWEIGHTED)
    bool explicit_resid = false, sparse_x = false, sparse = false;
    int VN = 4, PW = 1024, kp = 8;
    int npanels = 1, rpb = 1, nrb = 1, nwb = 1, nwb256 = 1, ntb = 1, ntb32 = 1, nsplit = 4;
    i64 red_elems = 0;
    int ro_il = -1;        // interleaved (1) or contiguous (0) row chunks forced by RRI_PASS_PK_GEOM; -1: by the workgroup count
    int cpart_rows = 0;    // rows of Cpart / N2part (dense weighted)
    i64 gpart_rows = 1, ttpart_rows = 1, tpart_rows = 1;      // rows allocated in Gpart, Ttpart, tpart
    int xy_stride = 1;
    SpDims sp[2];          // the blocked copies (sparse flavours)
    // the early-sums schedule (early_* below): workgroups of k_trow_early (= partial vectors T T[t,:]^T), workgroups of the early
    // job in the pass's grid (= rows of its Gpart) and the 64-row tiles each walks, tile workgroups of k_wfin
    int nte = 1, e_blocks = 1, e_tpb = 1, nwfin = 1;
    int e_stride = 0;      // own workgroups of the pass between two of the job (early_deal_stride; 0: the job's are contiguous)
};

// ---- the early-sums schedule (k_trow_early, the early job of k_pass, k_wfin) ------------------------------------------------
constexpr int TROW_EARLY_COLS = 256;   // columns per workgroup of k_trow_early: 16 waves = 4 topic residues x 4 column waves
constexpr int WFIN_TILES = 16;         // 64-row tiles per workgroup of k_wfin (one per wave)
// workgroups of the early job: a quarter of a CU count's worth, so that they fit the slots the last round of the pass leaves
// empty at the flagship shape (88 of 1024) and each walks its tiles in a fraction of a pass; never more than there are tiles
inline int early_job_blocks(i64 n, int n_cu) { return (int)std::max<i64>(1, std::min<i64>((n + 63) / 64, std::max(n_cu, 4) / 4)); }
// where they sit among the pass's own workgroups: after the first round (4 workgroups of the pass per CU), so that they neither
// delay the start of the stream nor, where the pass fills whole rounds, wait for its tail; a pass of one round has them last,
// beside it.  This is where the FIRST of them sits: the others follow it in a contiguous run or dealt through what is left of
// the pass's grid (DensePlan::e_stride; the map is early_slot in rri_early_deal.hpp)
inline int early_job_first(int pass_blocks, int n_cu) { return std::min(pass_blocks, 4 * std::max(n_cu, 1)); }
// LDS of the early job (doubles): T T[t,:]^T, the block's Gram partial, the four partial dots of a tile
inline size_t early_job_lds_doubles(int k) { return (size_t)(2 * k + 2 + 256); }

// flavour: as passed to rri_create (RRI_UNWEIGHTED .. RRI_UNWEIGHTED_SPARSE)
inline DensePlan dense_plan(i64 n, i64 d, int k, int dtype, int flavour, const rri_switches& sw, int n_cu) {
    DensePlan p;
    p.explicit_resid = flavour == RRI_UNWEIGHTED_RESIDUAL;
    p.sparse_x = flavour == RRI_UNWEIGHTED_SPARSE;
    const int weighted = (p.explicit_resid || p.sparse_x) ? (int)RRI_UNWEIGHTED : flavour;   // the same flavour of the algorithm: another schedule / storage
    const bool explicit_resid = p.explicit_resid;
    p.n = n; p.d = d; p.k = k; p.dtype = dtype; p.weighted = weighted;
    p.sparse = weighted == RRI_WEIGHTED_SPARSE || p.sparse_x;
    p.kp = (int)round_up(k, 8);
    p.VN = load_elems(dtype);
    p.PW = 64 * p.VN * 4;   // columns per workgroup: 4 waves x (64 lanes x one load)
    p.LD = round_up(d, p.VN);

    // geometry of the streaming pass
    p.npanels = (int)((p.LD + p.PW - 1) / p.PW);
    // Workgroups: a multiple of 512 (2 per CU: with 525 on 256 CUs some CUs get three and the pass waits for them),
    // as many as possible up to 2048 while each still walks ~192 rows or more -- with 49 rows each (20000 x 5000 at
    // 2048 workgroups) ramp-up and tail cost 13 % of the pass (profiles/r01_pass_workgroups_mid_size.log).
    // LDS per workgroup = (5 rows-doubles plain | 11 weighted) * rpb + 4 row-sum tiles (18 KiB): kept under 40 KiB so
    // that 4 workgroups (16 waves) fit a CU's 160 KiB -- with 62 KiB the weighted passes ran at 2 workgroups per CU
    // and 20 % slower.  (The explicit update kernel takes a sixth array and may run at 3 per CU.)
    const i64 rpb_cap = ((40 * 1024 - 4 * 8 * 72 * 8) / ((weighted ? 11 : explicit_resid ? 7 : 5) * 8)) / 16 * 16;
    i64 rpb = 0;
    {
        // handles whose passes write a residual back (explicit-residual, dense weighted): the read-modify-write pass
        // likes ~8192 workgroups of >= 96 rows (+3 % at C3 for the residual schedule, +6 % for the weighted one)
        // (round 4) the one-pass weighted step: ~16384 workgroups of >= 48 rows -- 1.40 against 1.50 - 1.55 ms per pass at BASELINE
        // config 5, engines made alternately in one process; 24576: the same, 32768: 1.44; the partial column sums grow with the
        // row blocks, +17 us per launch of the T-row chain (profiles/r04_wpass_one_variants.log)
        const bool rmw = explicit_resid || weighted == RRI_WEIGHTED_DENSE;
        // (round 4, late) the read-only pass: at most 1024 -- which at BASELINE config 3 means the LDS cap below decides, 560 rows per
        // workgroup and 1790 workgroups instead of 496 rows and 2020: 0.647-0.653 against 0.662-0.664 ms in four processes of five,
        // equal in the fifth (N-way in one process, tools/env_ab.py; the row count is a stride between concurrent streams and
        // the pass is sensitive to it: 544 rows, between the two, 0.695 ms -- profiles/r04_pass_rows_per_workgroup.log)
        const int total_max = weighted == RRI_WEIGHTED_DENSE ? 16384 : rmw ? 8192 : 1024;
        const i64 rows_min = weighted == RRI_WEIGHTED_DENSE ? 48 : rmw ? 96 : 192;
        for (int total = total_max; total >= 512 && rpb == 0; total -= 512) {
            const int nrb_t = std::max(1, total / p.npanels);
            const i64 r = (n + nrb_t - 1) / nrb_t;
            if (r >= rows_min || total == 512) rpb = r;
        }
    }
    rpb = std::max<i64>(rpb, 32);
    rpb = std::min<i64>(round_up(rpb, 16), rpb_cap);
    // A dense fp32 handle of the Gram form walks at most PK_ROWS_MAX rows per workgroup: more than that it only ever got from the
    // LDS cap (560), which takes 1024 workgroups of 1024 columns -- an X of 2 GB and more, which streams the packed copy
    // (xpack_ensure).  The 560 were tuned on the fp32 stream (above), and in the copy that stride is 7/8 of it.  Known at ONE
    // shape only, BASELINE config 3, and jagged there -- engines made alternately in one process, three visits each: 560 rows
    // 0.5758 ms per pass (0.5684 .. 0.5760), 528 0.5640, 512 0.5516 (0.5491 .. 0.5520), 496 0.5541, 480 0.5637, 448 0.5648, 400
    // 0.5500; 560 interleaved 0.5790 (profiles/r13_xpack_refill_steps.log, tools/pk_geom_probe.py; DESIGN 4.5 has the second
    // process, the fp32 stream at 512 rows and another shape).  The rule looks at n, d, storage and flavour only, not at
    // RRI_X_PACK or RRI_PASS_CACHE_MB: tests/test_xpack_gpu.py and tests/test_pass_keep_gpu.py compare W, T and the objective bit
    // for bit across those switches at 60007 x 10004, where the cap decides, so a handle must have the same geometry -- the same
    // order of its partial sums -- with the copy and without it; it keeps it when the copy is released.  RRI_PASS_PK_GEOM
    // (diagnostics) sets other rows and the chunk order for such handles.
    if (dtype == RRI_F32 && !weighted && !explicit_resid && !p.sparse) {
        rpb = sw.pk_rows > 0 ? std::min<i64>(round_up(std::max(sw.pk_rows, 16), 16), rpb_cap) : std::min<i64>(rpb, PK_ROWS_MAX);
        if (sw.pk_rows > 0) p.ro_il = sw.pk_il;
    }
    p.rpb = (int)rpb;
    p.nrb = (int)((n + rpb - 1) / rpb);
    if (p.sparse) {
        // no dense pass: the row copy is cut into column blocks (= Ypart panels), the column copy into row blocks (= Zpart rows)
        for (int w = 0; w < 2; ++w) p.sp[w] = sp_dims(n, d, w, p.sparse_x, dtype_size(dtype));
        p.npanels = p.sp[0].nblk;
        p.nrb = p.sp[1].nblk;
    }
    p.nwb = (int)((n + 64 * WCOL_TILES - 1) / (64 * WCOL_TILES));   // k_wcol blocks = rows of Gpart
    p.nwb256 = (int)((n + 255) / 256);
    p.ntb = (int)((d + 127) / 128);
    p.ntb32 = (int)((p.LD + 31) / 32);      // 32-column blocks of k_trow_small
    p.nsplit = (int)std::max<i64>(1, std::min<i64>(8, d / 2048));   // column slices of k_tgram
    p.red_elems = round_up(std::max<i64>(p.LD + (i64)GRAM_SLICES * (k + 2), weighted ? 2 * p.LD + 2 : 0), 4);
    p.gpart_rows = std::max(p.nwb, p.nrb);      // k_wcol leaves a row per 64-row tile, the fused pass one per row block
    p.xy_stride = (int)std::max<i64>(std::max<i64>(p.gpart_rows, (i64)p.nwb * WCOL_TILES), (i64)std::max(n_cu, 1));   // the on-chip sweep leaves one per CU
    p.ttpart_rows = std::max(p.nsplit, p.ntb32);   // k_tgram: nsplit column slices; k_trow_small: one per 32 columns
    p.tpart_rows = std::max(p.ntb, p.ntb32);
    if (weighted && !p.sparse) p.cpart_rows = (int)std::max<i64>(256, (n + 2047) / 2048);
    p.nte = (int)((d + TROW_EARLY_COLS - 1) / TROW_EARLY_COLS);
    p.e_blocks = early_job_blocks(n, n_cu);
    p.e_tpb = (int)(((n + 63) / 64 + p.e_blocks - 1) / p.e_blocks);
    p.nwfin = (int)((n + 64 * WFIN_TILES - 1) / (64 * WFIN_TILES));
    if (sw.early_deal && !p.sparse) p.e_stride = early_deal_stride(p.npanels * p.nrb, early_job_first(p.npanels * p.nrb, n_cu), p.e_blocks);
    return p;
}

// How the read-only pass over a dense X loads it (rri_ctx::keep_q).  Between two passes the other kernels of a topic step load
// and store, with default policy, W (read by k_wcol), the column-sum and row-dot partials (written by the pass, read by
// k_reduce / k_wcol), T (read and written) and the Gram partials: a line of X survives in the Infinity Cache from one pass to
// the next only while it and all of that fit (MI355X: about 256 MiB).  What the chain leaves of the capacity C is the budget of
// X: an X inside it is read with default-policy loads throughout (-1); of a larger one, as many whole row blocks as fit, the
// same ones in every pass, and the rest non-temporally, which neither allocates there nor evicts (k_pass).  C = 0 streams all.
struct PassKeepTerms { double chain, budget, block, x_bytes; };
inline PassKeepTerms pass_keep_terms(const DensePlan& p, int k, i64 ldw, size_t es, bool xp_valid, double pass_cache_mb) {
    PassKeepTerms t;
    t.chain = 8.0 * ((double)k * (double)ldw + 2.0 * (double)p.nrb * (double)p.LD + 2.0 * (double)p.npanels * (double)p.n +
                     2.0 * (double)k * (double)p.LD + 2.0 * (double)p.nwb * (double)(k + 2));
    t.budget = pass_cache_mb * 1.0e6 - t.chain;
    // bytes per element and columns of what the pass reads: X, or its packed copy (whole 1024-column groups of 3.5 bytes)
    const double eb = xp_valid ? 3.5 : (double)es, cols = xp_valid ? (double)p.npanels * 1024.0 : (double)p.LD;
    t.block = (double)p.rpb * cols * eb;
    t.x_bytes = (double)p.n * cols * eb;
    return t;
}
inline int pass_keep(const DensePlan& p, int k, i64 ldw, size_t es, bool xp_valid, double pass_cache_mb) {
    const PassKeepTerms t = pass_keep_terms(p, k, ldw, es, xp_valid, pass_cache_mb);
    if (t.x_bytes <= t.budget) return -1;
    if (!(t.budget > 0.0)) return 0;
    const double blocks = t.budget / t.block;      // whole row blocks that fit: the floor, at most all of them
    return blocks >= (double)p.nrb ? p.nrb : (int)blocks;
}

// ---- the blocked store of a CSR pattern: work items -------------------------------------------------------------------------
// Work items: runs of segments of one block, at most `target_items` in all and of equal entry count -- ONE round of
// workgroups (a 1024-thread workgroup with the block's tables per CU).  Round 2 cut "about 3 x 256" items and got
// 774-780: three rounds of the 256 CUs and a fourth for the last few, a quarter of every launch with the chip idle
// (profiles/r03_sp_blk_probe.log: 138 -> 115 us per pass).  Every (block, segment) belongs to exactly one item --
// also the empty ones, whose sums the consumers still read.  `segptr`: [nblk][nseg + 1], the padded prefix of the copy --
// the host builder's (build_sp_copy) or the one the device builder left and the host read back (rri_spbuild.hpp): the one
// cutter of both routes.
inline void sp_cut_work(const i64* segptr, const SpDims& cp, int which, int target_items, std::vector<SpWork>& work) {
    const i64 nseg = cp.nseg, stride = nseg + 1;
    std::vector<i64> eb((size_t)cp.nblk);
    i64 total = 0;
    for (int b = 0; b < cp.nblk; ++b) {
        const i64* row = segptr + (size_t)b * stride;
        eb[(size_t)b] = row[nseg] - row[0];
        total += eb[(size_t)b];
    }
    const i64 spare = std::max<i64>(0, (i64)target_items - cp.nblk);      // every block needs one item; the rest by share
    for (int b = 0; b < cp.nblk; ++b) {
        const i64* row = segptr + (size_t)b * stride;
        i64 items_b = 1 + (total > 0 ? spare * eb[(size_t)b] / total : 0);
        items_b = std::max<i64>(1, std::min<i64>(items_b, eb[(size_t)b] / 4096));      // no items of a few entries
        i64 s0 = 0;
        for (i64 j = 1; j <= items_b && s0 < nseg; ++j) {
            i64 s1 = nseg;
            if (j < items_b) {
                const i64 want = row[0] + eb[(size_t)b] * j / items_b;     // first segment boundary at or past the j-th share
                s1 = std::lower_bound(row + s0 + 1, row + nseg, want) - row;
                s1 = std::min<i64>(std::max<i64>(s1, s0 + 1), nseg);
            }
            work.push_back(SpWork{b, (int)s0, (int)s1, which});
            s0 = s1;
        }
        if (s0 < nseg) work.push_back(SpWork{b, (int)s0, (int)nseg, which});
    }
}
// lanes per segment: 4 quads of 4 entries per lane and iteration
inline int sp_lanes_per_segment(i64 nnz, const SpDims& cp) {
    const i64 avg = nnz / std::max<i64>(1, (i64)cp.nblk * cp.nseg);
    return avg >= 768 ? 64 : avg >= 384 ? 32 : avg >= 192 ? 16 : 8;
}

// ---- the blocked store of a CSR pattern: contents ------------------------------------------------------------------------
// One blocked copy of a validated pattern (column indices strictly increasing in every row), on the host: counting sort, stable,
// so offsets ascend inside a segment.  `target_items`: work items of the copy (SpWork.pad = the copy).
struct SpCopyHost {
    std::vector<i64> segptr;            // [nblk][nseg + 1]
    std::vector<unsigned short> idx;    // offset inside the block; pads: bw, the zero slot of the factor tables
    std::vector<int> perm;              // position in the canonical CSR; pads: -1
    std::vector<SpWork> work;
    i64 count = 0;                      // entries incl. the padding of every segment to a multiple of 4
    int lps = 8;                        // lanes per segment
    i64 longest_row = 0;
};
inline SpCopyHost build_sp_copy(const int64_t* indptr, const int32_t* indices, i64 n, i64 nnz, int which, const SpDims& cp,
                                int target_items) {
    SpCopyHost out;
    const int w = which;
    for (i64 r = 0; r < n; ++r) out.longest_row = std::max<i64>(out.longest_row, (i64)(indptr[r + 1] - indptr[r]));
    const i64 nseg = cp.nseg, stride = nseg + 1;
    std::vector<i64>& sp = out.segptr;
    sp.assign((size_t)cp.nblk * stride, 0);
    // count: entry (r, j) lives in block (gather index / bw), segment (the other index)
    for (i64 r = 0; r < n; ++r)
        for (i64 p = indptr[r]; p < indptr[r + 1]; ++p) {
            const i64 j = indices[p];
            const i64 g = w == 0 ? j : r, sgm = w == 0 ? r : j;
            sp[(size_t)((g / cp.bw) * stride + sgm + 1)] += 1;
        }
    i64 run = 0;   // exclusive prefix over (block, segment); every block row keeps nseg + 1 pointers.
    // Segments are padded to multiples of 4 entries (k_sp_blk moves quads).
    for (int b = 0; b < cp.nblk; ++b) {
        i64* row = sp.data() + (size_t)b * stride;
        row[0] = run;
        for (i64 q = 1; q <= nseg; ++q) {
            run += (row[q] + 3) / 4 * 4;
            row[q] = run;
        }
    }
    out.count = run;
    const size_t cntp = (size_t)std::max<i64>(run, 4);
    out.idx.assign(cntp, (unsigned short)cp.bw);      // pads: the zero slot of the factor tables
    out.perm.assign(cntp, -1);
    {
        std::vector<i64> fill((size_t)cp.nblk * nseg);
        for (int b = 0; b < cp.nblk; ++b)
            for (i64 q = 0; q < nseg; ++q) fill[(size_t)b * nseg + q] = sp[(size_t)b * stride + q];
        for (i64 r = 0; r < n; ++r)
            for (i64 p = indptr[r]; p < indptr[r + 1]; ++p) {
                const i64 j = indices[p];
                const i64 g = w == 0 ? j : r, sgm = w == 0 ? r : j;
                const i64 b = g / cp.bw;
                const i64 q = fill[(size_t)(b * nseg + sgm)]++;
                out.idx[(size_t)q] = (unsigned short)(g - b * cp.bw);
                out.perm[(size_t)q] = (int)p;
            }
    }
    sp_cut_work(sp.data(), cp, w, target_items, out.work);
    out.lps = sp_lanes_per_segment(nnz, cp);
    return out;
}

// ---- CSR argument checks -------------------------------------------------------------------------------------------------
// The error text of the first rule the host arrays of a call break; empty: fine.  CSR_ROWS: the arrays and the row pointers;
// CSR_COLUMNS: and every column index inside [0, d); CSR_INCREASING: and strictly increasing inside every row.
enum CsrRules { CSR_ROWS = 0, CSR_COLUMNS = 1, CSR_INCREASING = 2 };
inline std::string csr_check(const int64_t* indptr, const int32_t* indices, const void* data, i64 nnz, int data_dtype, i64 n, i64 d,
                             CsrRules rules) {
    if (!indptr || (nnz > 0 && (!indices || !data)) || nnz < 0) return "bad CSR arrays";
    if (data_dtype != RRI_F32 && data_dtype != RRI_F64) return "bad CSR data dtype";
    if (indptr[0] != 0 || indptr[n] != nnz) return "indptr does not span nnz";
    for (i64 r = 0; r < n; ++r)
        if (indptr[r + 1] < indptr[r]) return "indptr not monotone at row " + std::to_string(r);
    if (rules >= CSR_COLUMNS)
        for (i64 p = 0; p < nnz; ++p)
            if (indices[p] < 0 || indices[p] >= d) return "column index out of range at " + std::to_string(p);
    if (rules >= CSR_INCREASING)
        for (i64 r = 0; r < n; ++r)
            for (i64 p = indptr[r] + 1; p < indptr[r + 1]; ++p)
                if (indices[p] <= indices[p - 1]) return "column indices of row " + std::to_string(r) + " are not strictly increasing";
    return std::string();
}
// on arrays whose rows are sorted (csr_sort_rows): a column stored twice is refused
inline std::string csr_duplicates(const int64_t* indptr, const int32_t* indices, i64 n) {
    for (i64 r = 0; r < n; ++r)
        for (i64 p = indptr[r] + 1; p < indptr[r + 1]; ++p)
            if (indices[p] == indices[p - 1])
                return "row " + std::to_string(r) + " stores column " + std::to_string(indices[p]) + " twice (sum the duplicates first)";
    return std::string();
}
// Column indices sorted inside every row, stable; `ds` bytes per value.  Copies are made only when a row is unsorted: true means
// sidx / sval hold the sorted arrays, false that the caller's are sorted already and the vectors stay empty.
inline bool csr_sort_rows(const int64_t* indptr, const int32_t* indices, const void* data, i64 n, i64 nnz, size_t ds,
                          std::vector<int32_t>& sidx, std::vector<unsigned char>& sval) {
    const unsigned char* bytes = (const unsigned char*)data;
    for (i64 r = 0; r < n; ++r) {
        bool sorted = true;
        for (i64 p = indptr[r] + 1; p < indptr[r + 1] && sorted; ++p) sorted = indices[p] > indices[p - 1];
        if (sorted) continue;
        if (sidx.empty()) {
            sidx.assign(indices, indices + nnz);
            sval.assign(bytes, bytes + (size_t)nnz * ds);
        }
        std::vector<i64> ord((size_t)(indptr[r + 1] - indptr[r]));
        for (size_t q = 0; q < ord.size(); ++q) ord[q] = indptr[r] + (i64)q;
        std::stable_sort(ord.begin(), ord.end(), [&](i64 a, i64 b) { return indices[a] < indices[b]; });
        for (size_t q = 0; q < ord.size(); ++q) {
            sidx[(size_t)indptr[r] + q] = indices[ord[q]];
            std::copy(bytes + (size_t)ord[q] * ds, bytes + (size_t)ord[q] * ds + ds, sval.begin() + (std::ptrdiff_t)(((size_t)indptr[r] + q) * ds));
        }
    }
    return !sidx.empty();
}

// ---- register-resident persistent sweeps (rri_onchip_kernels.hpp) --------------------------------------------------------
struct OnchipGeom { int CG, RG, rows_wg, rpw, NA, kS, G; size_t shmem; };
constexpr int ONCHIP_UNTIL_CAP = 512;   // sweeps per launch of rri_sweep_until (a slot row of 256 shares each)
constexpr int ONCHIP_MAX_RPW = 20;    // rows per wave held in registers (float4 each): 32 spills at 256 VGPRs
// beyond ONCHIP_SMALL_K topics the k-term dots keep 8 terms per lane and the registers take fewer resident rows WITHOUT a spill
// (round 4, compiler's resource report: plain 18 rows / 253 VGPRs, with the projection 14 rows / 249; 20 rows spilled 10 / 16 -- and
// 68 in round 3's build: the allocation moves with every edit, the report of `python -m rri_nmf_amd.build --report` is the record)
constexpr int ONCHIP_MAX_RPW_K64 = 18, ONCHIP_MAX_RPW_K64_PROJ = 14;
// The rows per wave an instantiation of k_onchip_sweeps holds (its RPW): every (storage type, PROJ, KT) is built twice, for
// `few` rows (8) and for the most the registers take, so that a small problem does not carry the large build's registers
constexpr int onchip_rpw(bool f32, bool proj, int kt, bool few) {
    const int rows = few ? 8 : kt == 8 ? (proj ? ONCHIP_MAX_RPW_K64_PROJ : ONCHIP_MAX_RPW_K64) : ONCHIP_MAX_RPW;
    return f32 ? rows : rows / 2;       // float64 X: 8 registers per row and lane
}
constexpr int onchip_kt(int k) { return k > ONCHIP_SMALL_K ? 8 : 3; }
// proj: the simplex projection of T is configured (the projection stage stages the whole T row per worker: d <= 1024)
inline bool onchip_geometry(i64 n, i64 LD, int k, bool is_f32, bool proj, int n_cu, OnchipGeom* g) {
    if (LD > (proj ? 1024 : 2048) || n_cu < 1) return false;
    g->G = std::min(n_cu, 256);                     // the workers take 16 partials per lane group: G <= 16 ONCHIP_PG
    g->CG = LD <= 256 ? 1 : LD <= 512 ? 2 : LD <= 1024 ? 4 : 8;
    g->RG = ONCHIP_WAVES / g->CG;
    g->rows_wg = (int)((n + g->G - 1) / g->G);
    g->rpw = (g->rows_wg + g->RG - 1) / g->RG;
    g->NA = (int)((LD + ONCHIP_CWA - 1) / ONCHIP_CWA);      // workgroups that also own a column slice of T
    g->kS = k | 1;                                  // odd row stride of the LDS copy of W: no bank conflicts down a column
    if (g->rpw > onchip_rpw(is_f32, proj, onchip_kt(k), false) || g->NA > 64 || g->NA > g->G || (i64)g->rows_wg * g->kS > 6144) return false;
    const size_t doubles = (size_t)g->rows_wg * g->kS + (size_t)k * ONCHIP_CWA + (k + 2) + (k + 1) +
                           (size_t)ONCHIP_PG * ONCHIP_CWA + (size_t)g->CG * g->rows_wg + 2 * (size_t)g->rows_wg +
                           (size_t)ONCHIP_WAVES * 256 + (size_t)ONCHIP_WAVES * 8 * 72 + 1024 + 40;
    g->shmem = doubles * sizeof(double);
    return g->shmem <= 150 * 1024;
}
// the shapes the persistent kernel covers: 2 <= k <= ONCHIP_MAX_K and a geometry inside its registers and LDS
inline bool onchip_shape_ok(i64 n, i64 LD, int k, bool is_f32, bool proj, int n_cu, OnchipGeom* g) {
    return k >= 2 && k <= ONCHIP_MAX_K && onchip_geometry(n, LD, k, is_f32, proj, n_cu, g);
}

// ---- small grids -----------------------------------------------------------------------------------------------------------
// c = M^T (wn .* dw) as row-block partials in Cpart (k_wmcorr, k_wmcorr_cols): npg column groups x nrb row blocks of rpb rows;
// wcorr_nrb: the partial rows the T-row step then adds
struct WmcorrGrid { int npg; i64 nrb, rpb; int wcorr_nrb; };
// a sparse 0/1 mask, the set bits only (k_wmcorr_cols): 16 workgroups per CU (4: 60 us, 8: 48, 16: 46, 32: 44 at BASELINE config
// 5), row blocks of a multiple of 32 rows, at most 2048
inline WmcorrGrid wmcorr_cols_grid(i64 n, i64 LD, int n_cu) {
    WmcorrGrid g;
    g.npg = (int)((LD + 255) / 256);
    g.nrb = std::min<i64>(256, std::max<i64>(1, (16 * (i64)std::max(n_cu, 1) + g.npg - 1) / g.npg));
    g.rpb = std::min<i64>(2048, round_up((n + g.nrb - 1) / g.nrb, 32));
    g.nrb = (n + g.rpb - 1) / g.rpb;            // <= cpart_rows (256, or n / 2048 where that is more: dense_plan)
    g.wcorr_nrb = (int)g.nrb;
    return g;
}
// every bit or every stored weight (k_wmcorr): ~4 workgroups per CU, row blocks of a multiple of 64 rows, at most 4096 (32 KiB of
// LDS); a packed mask has a column group per 256 words of a row, a stored one per panel of the pass
inline WmcorrGrid wmcorr_grid(i64 n, bool bits, i64 ldb, int npanels, int n_cu, int cpart_rows) {
    WmcorrGrid g;
    g.npg = bits ? (int)((ldb + 255) / 256) : npanels;
    g.nrb = std::min<i64>(256, std::max<i64>(1, (4 * (i64)std::max(n_cu, 1) + g.npg - 1) / g.npg));
    g.rpb = std::min<i64>(4096, round_up((n + g.nrb - 1) / g.nrb, 64));
    g.nrb = (n + g.rpb - 1) / g.rpb;
    g.wcorr_nrb = (int)std::min<i64>(g.nrb, cpart_rows);     // (cpart_rows covers every n: see dense_plan)
    return g;
}
// k_resid_mfma (k <= 64): the k-panel depth of its instantiation
constexpr int resid_ks(int k) { return k <= 16 ? 4 : k <= 32 ? 8 : k <= 48 ? 12 : k <= 52 ? 13 : 16; }
// ... and the grid of 64-row blocks x column ranges.  With the row sums every block walks all columns; a residual written without
// them is cut into column ranges per row block: ~12 rounds of the chip's 2 workgroups per CU or more, so that the last, partly
// filled round costs a twelfth and not a quarter
struct ResidGrid { unsigned nb, ny; int nsplit, dchunk; };
inline ResidGrid resid_grid(i64 n, i64 d, int n_cu, bool sums) {
    ResidGrid g;
    g.nb = (unsigned)((n + 63) / 64);
    g.ny = 1u;
    g.nsplit = 1;
    g.dchunk = (int)round_up(d, 64);
    if (!sums) {
        const i64 per_round = 2 * (i64)std::max(n_cu, 1);
        g.nsplit = (int)std::min<i64>((d + 63) / 64, std::max<i64>(1, (12 * per_round + g.nb - 1) / g.nb));
        g.dchunk = (int)round_up((d + g.nsplit - 1) / g.nsplit, 64);
        g.ny = (unsigned)((d + g.dchunk - 1) / g.dchunk);
    }
    return g;
}
// launch-bound sizes: k_reduce and k_trow_numer as one launch (every workgroup reduces the Gram partials itself)
inline bool trow_small(int gpart_rows, int k, int ntb32) { return (double)gpart_rows * (k + 2) * ntb32 <= 4.0e6; }
// partial Gram matrices of a tall matrix (k_tall_gram_part)
inline int tall_gram_parts(i64 rows) { return (int)std::max<i64>(1, std::min<i64>(512, (rows + TG_ROWS - 1) / TG_ROWS)); }
// k_spx_rowtot / k_spx_scale on the canonical CSR: one group of 8 lanes per row, a whole wave from 64 entries per row on -- the
// summation order of a row is fixed by the shape
inline int spx_scale_lps(i64 nnz, i64 n) { return nnz / std::max<i64>(n, 1) >= 64 ? 64 : 8; }
// the packed copy of an fp32 X: one tile per `tile_rows`-row chunk and column panel; with more than an eighth of the tiles flagged
// (an element outside the window) the copy is not worth keeping
inline i64 xpack_tiles(i64 n, int npanels, int tile_rows) { return (n + tile_rows - 1) / tile_rows * npanels; }
inline bool xpack_too_many_flagged(i64 flagged, i64 tiles) { return flagged * 8 > tiles; }

}  // namespace rri
