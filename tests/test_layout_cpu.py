"""The geometry of a handle (rri_nmf_amd/csrc/rri_layout.hpp), on the CPU.

tests/c/layout_main.cpp is a stand-alone program with its own main that includes only that header and include/rri_hip.h.  It is
built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once, over every request of this
module (tests/layout_cases.py).  Checked:

  1. agreement with the Python restatements the suites keep, over their own case lists, equality throughout: both blocked copies
     of every run of wsb_cases.blocked_runs() at 256 and 304 CUs against sp_copy_layout; the dense weighted plan of every
     wsb_cases.dense_cases() and BIG shape against dense_layout; the persistent geometry of every onchip_cases.edge_cases(n_cu)
     against onchip_cases.geometry; VN, LD and the load width of every ld_cases.CASES entry; the terms of pass_keep against
     test_pass_keep_gpu.geometry at that file's shapes; the tile count of the packed copy against test_xpack_gpu.tiles_of;
  2. every blocked copy is a permutation of the stored entries with pads of (-1, bw), quad-aligned ascending segment pointers and
     work items that cover every (block, segment) exactly once;
  3. the rules no suite restates, at values worked out by hand from rri_create as it stood before the header existed (the
     arithmetic is in the comments of each case); 3b: the early-sums schedule at the shapes of tests/test_early_sums_routes_gpu.py
     and 256 CUs -- the pass's own workgroups against early_job_first, tiles per job workgroup, the grids behind the pass;
  4. every refusal text of the CSR checks for the input that triggers it, and the row sort."""
import numpy as np
import pytest
import scipy.sparse as sp

import layout_cases as lc
import ld_cases
import onchip_cases as oc
import test_early_sums_routes_gpu as er
import test_onchip_cases_cpu
import test_pass_keep_gpu as pk
import test_xpack_gpu as xg
import wsb_cases as wc
from layout_cases import RRI_F32, RRI_F64, RRI_F16, RRI_U8

ES = {'fp32': 4, 'fp64': 8}
N_CUS = (256, 304)
ALL_TYPES = (RRI_F32, RRI_F64, RRI_F16, RRI_U8)
VN = {RRI_F32: 4, RRI_F64: 2, RRI_F16: 8, RRI_U8: 8}      # elements of a 16-byte load; uint8: of an 8-byte one


class Asked(object):
    """the requests of every section, made before the one run of the program"""

    def __init__(self):
        s = self.s = lc.Session()
        # 1a. the blocked copies: one request per (pattern, copy, block cap, work-item target)
        self.patterns, self.copies, self.copy_runs = {}, {}, []
        for name, make, k, flavour, store in wc.blocked_runs():
            A = self.patterns.get(name)
            if A is None:
                A = self.patterns[name] = make()
            csrx = flavour == 'csrx'
            for n_cu in N_CUS:
                for w in (0, 1):
                    key = (name, w, wc.sp_block_cap(store, csrx), max(1, n_cu // 2 if csrx else n_cu))
                    if key not in self.copies:
                        self.copies[key] = s.ask(lc.copy_line(A, w, csrx, ES[store], n_cu))
                    self.copy_runs.append((name, store, csrx, n_cu, w, key))
        # 1b. the dense weighted plan
        self.dense = []
        shapes = sorted(set((c[1], c[2]) for c in wc.dense_cases()))
        for store in ('fp32', 'fp64'):
            for n, d in shapes + [wc.BIG[store]]:
                self.dense.append((n, d, store, s.ask(lc.plan_line(n, d, 5, lc.DTYPE_CODE[store], lc.WEIGHTED_DENSE))))
        # 1c. the persistent sweep
        self.onchip = []
        for n_cu in test_onchip_cases_cpu.N_CUS:
            for case in oc.edge_cases(n_cu):
                proj = oc.projected(case.flags)
                g = oc.geometry(case.n, case.d, case.k, case.store, proj, n_cu)
                self.onchip.append((case, n_cu, g, s.ask(lc.plan_line(case.n, case.d, case.k, lc.DTYPE_CODE[case.store], n_cu=n_cu)),
                                    s.ask('onchip %d %d %d %d %d %d' % (case.n, g['LD'], case.k, case.store == 'fp32', proj, n_cu))))
        # 1d. storage widths
        self.ld = [(c, s.ask(lc.plan_line(c.n, c.d, 2, lc.code_of(c.dtype)))) for c in ld_cases.CASES.values()]
        # 1e. pass_keep
        self.keep = []
        for n, d, k, dtype in [(v[0], v[1], 4, v[2]) for v in pk.LARGE.values()] + [(60007, 10004, 3, np.float32), (3001, 1203, 5, np.float32),
                                                                                  (286721, 2056, 3, np.uint8)]:
            self.keep.append((n, d, k, dtype, s.ask(lc.plan_line(n, d, k, lc.code_of(dtype))), s.ask(lc.keep_line(n, d, k, lc.code_of(dtype)))))
        self.xpack = [(n, d, s.ask(lc.plan_line(n, d, k, RRI_F32)), None) for n, d, k, _, _, _ in xg.SMALL.values()]
        self.misc = {}

    def ask(self, name, line):
        self.misc[name] = self.s.ask(line)

    def __getitem__(self, name):
        return self.s[self.misc[name]]


# ---- 3. values worked out by hand ----------------------------------------------------------------------------------------
# rows per workgroup are capped by the LDS of a pass: (40 KiB - 4 tiles of 8 x 72 doubles) / (arrays of a row, 8 bytes each), rounded
# down to 16: plain 5 arrays -> 22528 / 40 = 563 -> 560; explicit residual 7 -> 402 -> 400; weighted 11 -> 256
HAND_PLANS = {
    # fp32 Gram 100000 x 10000: 10 panels of 1024; 1024 workgroups -> 102 row blocks -> 981 rows -> 992 -> LDS cap 560 -> 512 (the cap of the
    # packed-copy handles); ceil(100000 / 512) = 196
    'fp32-100000x10000': ((100000, 10000, 4, RRI_F32), dict(npanels=10, rpb=512, nrb=196, interleaved=0, ro_il=-1)),
    # RRI_PASS_PK_GEOM=560i: 560 rows as asked (the LDS cap admits them), ceil(100000 / 560) = 179, interleaved although 1790 > 1024
    'fp32-100000x10000-560i': ((100000, 10000, 4, RRI_F32, dict(pk_rows=560, pk_il=1)), dict(npanels=10, rpb=560, nrb=179, interleaved=1, ro_il=1)),
    # float64: 20 panels of 512; 51 row blocks -> 1961 rows -> the LDS cap
    'fp64-100000x10000': ((100000, 10000, 4, RRI_F64), dict(npanels=20, rpb=560, nrb=179, interleaved=0)),
    # and the switch leaves a float64 handle alone
    'fp64-100000x10000-448c': ((100000, 10000, 4, RRI_F64, dict(pk_rows=448, pk_il=0)), dict(npanels=20, rpb=560, nrb=179, ro_il=-1)),
    # uint8: panels of 2048; 512 row blocks -> 561 rows -> 576 -> 560; ceil(286721 / 560) = 513, the last of one row; 1026 workgroups
    'u8-286721x2056': ((286721, 2056, 3, RRI_U8), dict(npanels=2, rpb=560, nrb=513, interleaved=0, LD=2056)),
    # LD 4104 = 3 panels; 341 row blocks of 18 rows are too short down to 512 workgroups: 170 blocks -> 36 rows -> 48; 126 blocks
    'u8-6011x4099': ((6011, 4099, 4, RRI_U8), dict(npanels=3, rpb=48, nrb=126, interleaved=1, LD=4104)),
    # 10 panels; 102 row blocks -> 589 rows -> 592 -> 560 -> 512, whatever RRI_X_PACK and RRI_PASS_CACHE_MB say
    'fp32-60007x10004': ((60007, 10004, 3, RRI_F32), dict(npanels=10, rpb=512, nrb=118, interleaved=0)),
    'fp32-60007x10004-nocopy': ((60007, 10004, 3, RRI_F32, dict(x_pack=0)), dict(npanels=10, rpb=512, nrb=118)),
    'fp32-60007x10004-copy': ((60007, 10004, 3, RRI_F32, dict(x_pack=1, cache_mb=0.0)), dict(npanels=10, rpb=512, nrb=118)),
    # test_xpack_refill_gpu.py: 600000 x 1024 is one panel; 1024 blocks -> 586 rows -> 592 -> 560 -> 512; 448 rows where asked for
    'fp32-600000x1024': ((600000, 1024, 2, RRI_F32), dict(npanels=1, rpb=512, nrb=1172)),
    'fp32-600000x1024-448c': ((600000, 1024, 2, RRI_F32, dict(pk_rows=448, pk_il=0)), dict(rpb=448, nrb=1340, interleaved=0, ro_il=0)),
    # 200 x 1030 (two panels): 512 workgroups -> 256 blocks -> 1 row -> the floor of 32 rows; the switch: rows rounded up to 16, at
    # least 16, at most the LDS cap
    'fp32-200x1030': ((200, 1030, 2, RRI_F32), dict(npanels=2, rpb=32, nrb=7, interleaved=1)),
    'fp32-200x1030-40i': ((200, 1030, 2, RRI_F32, dict(pk_rows=40, pk_il=1)), dict(rpb=48, nrb=5, interleaved=1)),
    'fp32-200x1030-16': ((200, 1030, 2, RRI_F32, dict(pk_rows=16)), dict(rpb=16, nrb=13, interleaved=1, ro_il=-1)),
    'fp32-200x1030-100000c': ((200, 1030, 2, RRI_F32, dict(pk_rows=100000, pk_il=0)), dict(rpb=560, nrb=1, interleaved=0)),
    # explicit residual: up to 8192 workgroups of 96 rows or more; one panel, 3400000 rows: 8192 blocks -> 416 rows -> LDS cap 400
    'resid-3400000x4': ((3400000, 4, 1, RRI_F32, dict(flavour=lc.UNWEIGHTED_RESIDUAL)), dict(npanels=1, rpb=400, nrb=8500, cpart_rows=0)),
    # ... and where the cap does not decide: 500000 rows: 5120 blocks are the most with 96 rows or more (98) -> 112
    'resid-500000x64': ((500000, 64, 2, RRI_F32, dict(flavour=lc.UNWEIGHTED_RESIDUAL)), dict(npanels=1, rpb=112, nrb=4465)),
    # dense weighted: up to 16384 workgroups of 48 rows or more; 4300000 rows: 263 rows -> 272 -> LDS cap 256; Cpart rows: n / 2048
    'weighted-4300000x4': ((4300000, 4, 1, RRI_F32, dict(flavour=lc.WEIGHTED_DENSE)), dict(npanels=1, rpb=256, nrb=16797, cpart_rows=2100)),
    'weighted-3400000x4': ((3400000, 4, 1, RRI_F32, dict(flavour=lc.WEIGHTED_DENSE)), dict(npanels=1, rpb=208, nrb=16347, cpart_rows=1661)),
    # the other sums of a handle, at the smoke shape 1500 x 700, k = 8, fp32: 47 row blocks of 32 rows (Gpart has a row for each), 24
    # blocks of 64 rows, 6 of 256; 6 blocks of 128 columns, 22 of 32; one column slice of k_tgram; red: 700 + 8 slices (RRI_GRAM_SLICES) x 10 = 780; one XYpart entry per CU
    'fp32-1500x700': ((1500, 700, 8, RRI_F32), dict(LD=700, VN=4, PW=1024, kp=8, nwb=24, nwb256=6, ntb=6, ntb32=22, nsplit=1, red_elems=780,
                                                   gpart_rows=47, ttpart_rows=22, tpart_rows=22, xy_stride=256, rpb=32, nrb=47)),
    # weighted: red holds two rows of LD and two scalars; d / 2048 column slices, at most 8
    'weighted-300x20000': ((300, 20000, 3, RRI_F64, dict(flavour=lc.WEIGHTED_DENSE, n_cu=304)),
                           dict(LD=20000, nsplit=8, red_elems=40004, cpart_rows=256, xy_stride=304, kp=8, wtrow_small=1)),
}
for _code in ALL_TYPES:
    _pw = 64 * VN[_code] * 4
    # tiny shapes: one row block at the floor of 32 rows; d one past a panel width: LD is the next multiple of a load, two panels
    HAND_PLANS['tiny-1x1-%d' % _code] = ((1, 1, 1, _code), dict(LD=VN[_code], VN=VN[_code], PW=_pw, npanels=1, rpb=32, nrb=1, nwb=1, ntb=1, ntb32=1,
                                                               interleaved=1, load_bytes=8 if _code == RRI_U8 else 16))
    HAND_PLANS['tiny-17x5-%d' % _code] = ((17, 5, 2, _code), dict(LD=-(-5 // VN[_code]) * VN[_code], npanels=1, rpb=32, nrb=1))
    HAND_PLANS['tiny-panel+1-%d' % _code] = ((33, _pw + 1, 2, _code), dict(LD=_pw + VN[_code], npanels=2, rpb=32, nrb=2))


# ---- 3b. the early-sums schedule at the shapes of tests/test_early_sums_routes_gpu.py, 256 CUs: F = early_job_first's 4 n_cu = 1024 -------
# fields: npanels, rpb, nrb, P = npanels nrb, first = min(P, F), e_blocks = min(tiles, 64), e_tpb = ceil(tiles / e_blocks), idle =
# e_blocks - ceil(tiles / e_tpb) job workgroups without a tile, nte = ceil(d / 256), nwfin = ceil(n / 1024), nsplit = min(8, d / 2048)
EARLY_A1 = {
    # RRI_PASS_PK_GEOM=16c / 16i, fp32, d = 130 (one panel): P = ceil(n / 16)
    'F-1': dict(npanels=1, rpb=16, nrb=1023, P=1023, first=1023, e_blocks=64, tiles=256, e_tpb=4, idle=0, nte=1, nwfin=16, nsplit=1),
    'F': dict(npanels=1, rpb=16, nrb=1024, P=1024, first=1024, e_blocks=64, tiles=256, e_tpb=4, idle=0, nte=1, nwfin=16, nsplit=1),
    # 16385 rows: 257 tiles -> 5 per job workgroup, 52 of the 64 walk tiles
    'F+1': dict(npanels=1, rpb=16, nrb=1025, P=1025, first=1024, e_blocks=64, tiles=257, e_tpb=5, idle=12, nte=1, nwfin=17, nsplit=1),
    'F+11': dict(npanels=1, rpb=16, nrb=1035, P=1035, first=1024, e_blocks=64, tiles=259, e_tpb=5, idle=12, nte=1, nwfin=17, nsplit=1),
    '2F': dict(npanels=1, rpb=16, nrb=2048, P=2048, first=1024, e_blocks=64, tiles=512, e_tpb=8, idle=0, nte=1, nwfin=32, nsplit=1),
    # 5473 x 2503: LD 2504, 3 panels x 343 row blocks; 86 tiles -> 2 per job workgroup, 43 walk tiles; 10 workgroups of k_trow_early
    'three-panels': dict(npanels=3, rpb=16, nrb=343, P=1029, first=1024, e_blocks=64, tiles=86, e_tpb=2, idle=21, nte=10, nwfin=6, nsplit=1),
    # 3300 x 4100: 5 panels x 207 row blocks; 52 tiles, a job workgroup each; the Gram-row job in two column slices
    'five-panels-nsplit2': dict(npanels=5, rpb=16, nrb=207, P=1035, first=1024, e_blocks=52, tiles=52, e_tpb=1, idle=0, nte=17, nwfin=4, nsplit=2),
}
EARLY_ROWS = {      # d = 130, k = 5, no switch: a pass of one round, the job last
    1024: dict(tiles=16, e_blocks=16, e_tpb=1, idle=0, nwfin=1), 1025: dict(tiles=17, e_blocks=17, e_tpb=1, idle=0, nwfin=2),
    4096: dict(tiles=64, e_blocks=64, e_tpb=1, idle=0, nwfin=4),
    # 65 tiles on 64 job workgroups: two each, 33 walk tiles, 31 store a row of zeros
    4097: dict(tiles=65, e_blocks=64, e_tpb=2, idle=31, nwfin=5), 4160: dict(tiles=65, e_blocks=64, e_tpb=2, idle=31, nwfin=5),
}
EARLY_COLS = {128: (1, 1), 129: (1, 2), 255: (1, 2), 256: (1, 2), 257: (2, 3), 384: (2, 3), 385: (2, 4)}      # n = 200: d -> (nte, ntb = ceil(d / 128))


@pytest.fixture(scope='module')
def asked(tmp_path_factory):
    a = Asked()
    for name in er.A1_SHAPES:
        n, d, k, _, _ = er.a1_shape(name, 256)
        for il in (0, 1):
            a.ask('early-%s-%d' % (name, il), lc.early_line(n, d, k, RRI_F32, pk_rows=16, pk_il=il))
    for code in (RRI_F32, RRI_F64):
        for n in EARLY_ROWS:
            a.ask('early-n%d-%d' % (n, code), lc.early_line(n, 130, 5, code))
        for d in EARLY_COLS:
            a.ask('early-d%d-%d' % (d, code), lc.early_line(200, d, 5, code))
    a.ask('early-lds-16rows', lc.early_line(16368, 130, 1024, RRI_F32, pk_rows=16, pk_il=0))
    a.ask('early-lds-32rows', lc.early_line(1000, 300, 1024, RRI_F64))
    for name, (args, _) in HAND_PLANS.items():
        a.ask(name, lc.plan_line(*args[:4], **(args[4] if len(args) > 4 else {})))
    # pass_keep at 30011 x 2503, k = 4 (fp32: LD 2504, 3 panels; 170 blocks -> 177 rows -> 192 rows, 157 blocks; 469 blocks of 64 rows)
    for name, kw in (('default', {}), ('default-copy', dict(xp_valid=True)), ('zero', dict(cache_mb=0.0)), ('zero-copy', dict(cache_mb=0.0, xp_valid=True)),
                     ('chain', dict(cache_mb=8.0)), ('fits', dict(cache_mb=1000.0)), ('fits-just', dict(cache_mb=309.4864)),
                     ('just-short', dict(cache_mb=309.4863)), ('all-blocks-but-x', dict(cache_mb=310.0, xp_valid=True))):
        a.ask('keep-' + name, lc.keep_line(30011, 2503, 4, RRI_F32, **kw))
    a.ask('keep-small', lc.keep_line(1500, 700, 8, RRI_F32))
    a.ask('keep-ldw', lc.keep_line(30011, 2503, 4, RRI_F32, ldw=40000))
    for name, line in CSR_REQUESTS.items():
        a.ask(name, line)
    for name, line in SMALL_GRIDS.items():
        a.ask(name, line)
    a.s.run(lc.build_program(tmp_path_factory.mktemp('layout'), sanitize=True))
    return a


# ---- 1. the restatements ----------------------------------------------------------------------------------------------------
def test_blocked_copies_equal_the_restatement_and_are_permutations(asked):
    checked = set()
    for name, store, csrx, n_cu, w, key in asked.copy_runs:
        A, got = asked.patterns[name], asked.s[asked.copies[key]]
        want = wc.sp_copy_layout(A, w, store, csrx, n_cu)
        tag = (name, store, csrx, n_cu, w)
        for f in ('nblk', 'bw', 'lps', 'nwork'):
            assert got[f] == want[f], (tag, f, got[f], want[f])
        assert [tuple(r) for r in got['work'][:, :3].tolist()] == want['work'], tag
        assert (got['work'][:, 3] == w).all(), tag
        nblk, nseg = want['nblk'], got['nseg']
        assert (got['nseg'], got['gdim']) == ((A.shape[0], A.shape[1]) if w == 0 else (A.shape[1], A.shape[0])), tag
        ptr = got['segptr'].reshape(nblk, nseg + 1)
        assert np.array_equal(np.diff(ptr, axis=1), (want['seg_len'] + 3) // 4 * 4), tag      # per-segment lengths, padded to quads
        assert got['longest_row'] == (np.diff(A.indptr).max() if A.shape[0] else 0), tag
        if key in checked:
            continue
        checked.add(key)
        # 2. the copy is a permutation
        assert ptr[0, 0] == 0 and ptr[-1, -1] == got['count'] and (ptr % 4 == 0).all(), tag
        assert (ptr[1:, 0] == ptr[:-1, -1]).all() and (np.diff(ptr, axis=1) >= 0).all(), tag
        idx, perm = got['idx'], got['perm']
        assert len(idx) == len(perm) == max(got['count'], 4), tag
        stored = perm >= 0
        assert np.array_equal(np.sort(perm[stored]), np.arange(A.nnz)), (tag, 'every stored entry exactly once')
        assert (perm[~stored] == -1).all() and np.array_equal(idx == got['bw'], ~stored), (tag, 'pads are (-1, bw), and nothing else is')
        lens = np.diff(ptr, axis=1).ravel()
        blk_of = np.repeat(np.repeat(np.arange(nblk), nseg), lens)
        seg_of = np.repeat(np.tile(np.arange(nseg), nblk), lens)
        rows, cols = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), A.indices
        q = np.flatnonzero(stored[:got['count']])
        g, sgm = (cols, rows) if w == 0 else (rows, cols)
        p = perm[q]
        assert np.array_equal(blk_of[q], g[p] // got['bw']) and np.array_equal(seg_of[q], sgm[p]), (tag, 'an entry in the wrong block or segment')
        assert np.array_equal(idx[q], g[p] - blk_of[q] * got['bw']), (tag, 'offset inside the block')
        same = (blk_of[q][1:] == blk_of[q][:-1]) & (seg_of[q][1:] == seg_of[q][:-1])
        assert (np.diff(idx[q])[same] > 0).all(), (tag, 'offsets ascend inside a segment')
        cnt = np.zeros((nblk, nseg), dtype=np.int64)
        np.add.at(cnt, (blk_of[q], seg_of[q]), 1)
        assert np.array_equal(cnt, want['seg_len']), tag
        cover = np.zeros((nblk, nseg), dtype=np.int64)
        for b, s0, s1, _ in got['work'].tolist():
            assert 0 <= s0 < s1 <= nseg, tag
            cover[b, s0:s1] += 1
        assert (cover == 1).all(), (tag, 'every (block, segment) in exactly one work item')
    assert len(checked) == len(asked.copies)


def test_dense_weighted_plan_equals_the_restatement(asked):
    for n, d, store, i in asked.dense:
        got, want = asked.s[i], wc.dense_layout(n, d, store)
        for f in ('rpb', 'nrb', 'npanels', 'LD'):
            assert got[f] == want[f], (n, d, store, f, got[f], want[f])
        assert bool(got['wtrow_small']) == want['wtrow_small'] and bool(got['interleaved']) == want['interleaved'], (n, d, store)


def test_persistent_geometry_equals_the_restatement(asked):
    assert asked.onchip
    for case, n_cu, g, ip, io in asked.onchip:
        plan, got = asked.s[ip], asked.s[io]
        assert plan['LD'] == g['LD'], (case.name, n_cu)
        assert bool(got['ok']) == g['eligible'] == case.expect_eligible, (case.name, n_cu, got, g)
        assert got['KT'] == g['KT'], (case.name, n_cu)
        if 'CG' not in g:                               # refused for k or LD: nothing else is defined
            continue
        for f in ('CG', 'RG', 'rows_wg', 'rpw', 'NA', 'kS', 'G', 'RPW'):
            assert got[f] == g[f], (case.name, n_cu, f, got[f], g[f])
        assert bool(got['few']) == g['few'] and got['cap'] == oc.rpw_of(case.store, oc.projected(case.flags), g['KT'], False), (case.name, n_cu)
        if not set(g['refusals']) & {'rpw', 'NA', 'w_lds'}:       # (the code sizes the LDS block only for a shape the other limits admit)
            assert got['shmem'] == g['shmem'], (case.name, n_cu, got['shmem'], g['shmem'])
        assert bool(got['geom']) == (not g['refusals']), (case.name, n_cu)


def test_storage_widths_equal_the_restatement(asked):
    for c, i in asked.ld:
        got, vn = asked.s[i], ld_cases.vn_of(c.dtype)
        assert ld_cases.strides_of(c.d, c.dtype) == ((c.d + got['VN'], 0), (c.d + 65 * got['VN'], got['VN'])), c.name
        assert got['VN'] == vn and got['LD'] == -(-c.d // vn) * vn == c.d, c.name
        assert got['load_bytes'] == vn * np.dtype(c.dtype).itemsize and got['dtype_size'] == np.dtype(c.dtype).itemsize, c.name
        assert got['PW'] == 256 * vn, c.name


def test_pass_keep_terms_equal_the_restatement(asked):
    for n, d, k, dtype, ip, ik in asked.keep:
        plan, got = asked.s[ip], asked.s[ik]
        xb, block, chain = pk.geometry(n, d, k, dtype, plan)
        assert (got['x_bytes'], got['block'], got['chain']) == (xb, block, chain), (n, d, got, (xb, block, chain))
        assert got['budget'] == 256.0e6 - chain


def test_packed_copy_tiles_equal_the_restatement(asked):
    for n, d, ip, _ in asked.xpack:
        plan = asked.s[ip]
        for flagged in (0, 1):
            assert asked['xpack-%dx%d-%d' % (n, d, flagged)]['tiles'] == xg.tiles_of(n, plan), (n, d)


# ---- 3. by hand ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(HAND_PLANS))
def test_plan_values_worked_out_by_hand(asked, name):
    got = asked[name]
    for f, v in HAND_PLANS[name][1].items():
        assert got[f] == v, (name, f, got[f], v)


@pytest.mark.parametrize('name', er.A1_SHAPES)
def test_early_job_sits_where_the_gpu_cases_say(asked, name):
    """the shapes of test_early_sums_routes_gpu.test_job_inside_the_grid at 256 CUs: the job's first workgroup against the pass's own
    count P on the side of F = 1024 that the case names, in both chunk orders"""
    n, d, k, P, side = er.a1_shape(name, 256)
    for il in (0, 1):
        got = asked['early-%s-%d' % (name, il)]
        for f, v in EARLY_A1[name].items():
            assert got[f] == v, (name, il, f, got[f], v)
        assert got['P'] == P and got['interleaved'] == il
        assert {'below': P < 1024 and got['first'] == P, 'at': P == 1024 and got['first'] == P,
                'above': P > 1024 and got['first'] == 1024}[side], (name, got)
        assert got['job_lds'] <= got['pass_lds']
    assert [nm for nm in er.A1_SHAPES if er.a1_shape(nm, 256)[4] == 'above'] == list(er.A1_INSIDE)
    assert er.a1_shape('F+11', 256)[3] % 8 == 3 and er.a1_shape('five-panels-nsplit2', 256)[1] >= 4096


def test_early_job_tiles_and_the_grids_behind_it(asked):
    """the row and column edges of test_early_sums_routes_gpu.py: tiles per job workgroup and job workgroups without a tile, the tile
    workgroups of k_wfin, the workgroups of k_trow_early and the entries of tpart; the job's LDS inside the pass's at k = 1024"""
    for code in (RRI_F32, RRI_F64):
        for n, want in EARLY_ROWS.items():
            got = asked['early-n%d-%d' % (n, code)]
            for f, v in dict(want, nte=1, npanels=1, first=got['P']).items():
                assert got[f] == v, (n, code, f, got[f], v)
            assert got['P'] <= 1024
        for d, (nte, ntb) in EARLY_COLS.items():
            got = asked['early-d%d-%d' % (d, code)]
            assert (got['nte'], got['ntb'], got['tiles'], got['e_blocks'], got['e_tpb'], got['idle'], got['nwfin']) == (nte, ntb, 4, 4, 1, 0, 1), (d, code, got)
            # k_trow_early's guard `(blockIdx.x * 2 + tid) * 128 < d` writes exactly the ntb entries of tpart that k_tgram adds
            assert sum((2 * b + tid) * 128 < d for b in range(nte) for tid in (0, 1)) == ntb, d
    # early_job_lds_doubles(1024) = 2 * 1024 + 2 + 256 = 2306 doubles against the pass's 5 rpb + 4 * 8 * 72: 2384 at 16 rows, 2464 at 32
    small, floor = asked['early-lds-16rows'], asked['early-lds-32rows']
    assert (small['rpb'], small['job_lds'], small['pass_lds']) == (16, 2306, 2384) and (floor['rpb'], floor['job_lds'], floor['pass_lds']) == (32, 2306, 2464)


def test_pass_keep_by_hand(asked):
    """fp32 30011 x 2503, k = 4: chain = 8 (k ldw + 2 nrb LD + 2 npanels n + 2 k LD + 2 nwb (k + 2)) = 8 (120044 + 786256 + 180066 + 20032
    + 5628) = 8896208 bytes; X 30011 x 2504 x 4 = 300590176 bytes, a row block 192 x 2504 x 4 = 1923072; the packed copy has
    3 x 1024 columns of 3.5 bytes: 322678272 and 2064384"""
    chain = 8896208
    d = asked['keep-default']
    assert (d['chain'], d['x_bytes'], d['block'], d['nrb']) == (chain, 300590176, 1923072, 157)
    assert d['budget'] == 256e6 - chain and d['q'] == 128                  # 247103792 / 1923072 = 128.49
    c = asked['keep-default-copy']
    assert (c['x_bytes'], c['block'], c['q']) == (322678272, 2064384, 119)   # 247103792 / 2064384 = 119.69
    assert asked['keep-zero']['q'] == 0 and asked['keep-zero-copy']['q'] == 0      # RRI_PASS_CACHE_MB=0: all of X streams
    assert asked['keep-chain']['q'] == 0 and asked['keep-chain']['budget'] < 0      # 8 MB: the chain alone takes more
    assert asked['keep-fits']['q'] == -1
    # X and the chain take 300590176 + 8896208 = 309486384 bytes: 16 bytes more hold all of X, 84 bytes less hold 156 of the 157 row
    # blocks (300590092 / 1923072 = 156.3), the last of which has 59 rows
    assert asked['keep-fits-just']['q'] == -1 and asked['keep-just-short']['q'] == 156
    # 310 MB: the copy's 322678272 bytes do not fit 310e6 - chain = 301103792, 145 of its blocks do (145.9)
    assert asked['keep-all-blocks-but-x']['q'] == 145
    assert asked['keep-small']['q'] == -1
    assert asked['keep-ldw']['chain'] == chain + 8 * 4 * (40000 - 30011)


SMALL_GRIDS = {
    # k_wmcorr_cols: 16 workgroups per CU over npg = ceil(LD / 256) column groups, at most 256 row blocks, of a multiple of 32 rows
    'cols-203x144': 'wmcorr_cols 203 144 256',            # 1 group; 256 blocks -> 1 row -> 32 rows; 7 blocks
    'cols-100000x5000': 'wmcorr_cols 100000 5000 256',    # 20 groups; ceil(4096 / 20) = 205 blocks -> 488 rows -> 512; 196 blocks
    'cols-3000000x8': 'wmcorr_cols 3000000 8 256',        # 256 blocks -> 11719 rows -> 2048 at most; 1465 blocks
    # k_wmcorr: 4 per CU; a packed mask has ceil(ldb / 256) groups (ldb = LD / 4 words), a stored one a group per panel
    'bits-203x144': 'wmcorr 203 1 36 1 256 256',          # 256 blocks -> 1 row -> 64 rows; 4 blocks
    'stored-100000x5000': 'wmcorr 100000 0 0 5 256 256',  # ceil(1024 / 5) = 205 blocks -> 488 rows -> 512; 196 blocks
    'bits-3000000x8': 'wmcorr 3000000 1 2 1 304 1465',    # 256 blocks -> 11719 rows -> 4096 at most; 733 blocks
    'bits-short-cpart': 'wmcorr 3000000 1 2 1 304 700',   # (never more partial rows than Cpart has)
    # k_resid_mfma without the row sums: 24 blocks of 64 rows; 12 rounds of 512 workgroups over 24 = 256 ranges, at most the 11 tiles of
    # 64 columns: 11 ranges of 64 columns; with the sums one range of 704
    'resid-split': 'resid 1500 700 8 256 0', 'resid-sums': 'resid 1500 700 8 256 1',
    # 100000 rows = 1563 blocks; ceil(6144 / 1563) = 4 ranges of ceil(10000 / 4) = 2500 -> 2560 columns
    'resid-wide': 'resid 100000 10000 16 256 0',
    'tall-1': 'tall 1', 'tall-32': 'tall 32', 'tall-33': 'tall 33', 'tall-16384': 'tall 16384', 'tall-16385': 'tall 16385',
    'spx-63': 'spxlps 6399 100', 'spx-64': 'spxlps 6400 100', 'spx-empty': 'spxlps 0 0',
    # Gram partial rows x (k + 2) x blocks of 32 columns, up to 4e6: 1000 x 5 x 800 is the last; no all-reduce and up to 64 row blocks
    'small-at': 'small 1000 3 800 0 64', 'small-past': 'small 1000 3 801 0 65', 'small-comm': 'small 1 1 1 1 64',
}
SMALL_GRIDS.update(('ks-%d' % k, 'resid 64 64 %d 256 1' % k) for k in (1, 16, 17, 32, 33, 48, 49, 52, 53, 64))
for _n, _d, _, _, _, _ in xg.SMALL.values():          # chunks of 8 rows (rri_xpack.hpp) x panels of 1024 columns
    for _f in (0, 1):
        SMALL_GRIDS['xpack-%dx%d-%d' % (_n, _d, _f)] = 'xpack %d %d 8 %d' % (_n, -(-_d // 1024), _f)
SMALL_GRIDS.update({'xpack-eighth': 'xpack 64 1 8 1', 'xpack-past-eighth': 'xpack 64 2 8 3'})      # 8 tiles, 1 flagged; 16 tiles, 3 flagged


def test_small_grids_by_hand(asked):
    assert asked['cols-203x144'] == dict(npg=1, nrb=7, rpb=32, wcorr_nrb=7)
    assert asked['cols-100000x5000'] == dict(npg=20, nrb=196, rpb=512, wcorr_nrb=196)
    assert asked['cols-3000000x8'] == dict(npg=1, nrb=1465, rpb=2048, wcorr_nrb=1465)
    assert asked['bits-203x144'] == dict(npg=1, nrb=4, rpb=64, wcorr_nrb=4)
    assert asked['stored-100000x5000'] == dict(npg=5, nrb=196, rpb=512, wcorr_nrb=196)
    assert asked['bits-3000000x8'] == dict(npg=1, nrb=733, rpb=4096, wcorr_nrb=733)
    assert asked['bits-short-cpart'] == dict(npg=1, nrb=733, rpb=4096, wcorr_nrb=700)
    assert asked['resid-split'] == dict(ks=4, nb=24, ny=11, nsplit=11, dchunk=64)
    assert asked['resid-sums'] == dict(ks=4, nb=24, ny=1, nsplit=1, dchunk=704)
    assert asked['resid-wide'] == dict(ks=4, nb=1563, ny=4, nsplit=4, dchunk=2560)
    for k, ks in ((1, 4), (16, 4), (17, 8), (32, 8), (33, 12), (48, 12), (49, 13), (52, 13), (53, 16), (64, 16)):
        assert asked['ks-%d' % k]['ks'] == ks, k
    assert [asked['tall-%d' % r]['parts'] for r in (1, 32, 33, 16384, 16385)] == [1, 1, 2, 512, 512]      # blocks of 32 rows, at most 512
    assert [asked[nm]['lps'] for nm in ('spx-63', 'spx-64', 'spx-empty')] == [8, 64, 8]
    assert asked['small-at'] == dict(trow_small=1, wtrow_small=1) and asked['small-past'] == dict(trow_small=0, wtrow_small=0)
    assert asked['small-comm'] == dict(trow_small=1, wtrow_small=0)
    for n, d, _, _, _, _ in xg.SMALL.values():
        assert asked['xpack-%dx%d-0' % (n, d)]['too_many'] == 0
    assert asked['xpack-eighth'] == dict(tiles=8, too_many=0) and asked['xpack-past-eighth'] == dict(tiles=16, too_many=1)


# ---- 4. CSR checks --------------------------------------------------------------------------------------------------------------
_IP, _IX = [0, 2, 2, 4], [0, 3, 1, 2]          # 3 x 4, rows of 2, 0 and 2 entries
CSR_REQUESTS = {
    'csr-fine': lc.csr_line(lc.CSR_INCREASING, 3, 4, 4, RRI_F64, _IP, _IX),
    'csr-no-indptr': lc.csr_line(lc.CSR_ROWS, 3, 4, 4, RRI_F64, None, _IX),
    'csr-no-indices': lc.csr_line(lc.CSR_ROWS, 3, 4, 4, RRI_F64, _IP, None),
    'csr-no-data': lc.csr_line(lc.CSR_ROWS, 3, 4, 4, RRI_F64, _IP, _IX, has_data=False),
    'csr-negative-nnz': lc.csr_line(lc.CSR_ROWS, 3, 4, -1, RRI_F64, [0, 0, 0, -1], []),
    'csr-half-data': lc.csr_line(lc.CSR_ROWS, 3, 4, 4, RRI_F16, _IP, _IX),
    'csr-count-data': lc.csr_line(lc.CSR_ROWS, 3, 4, 4, RRI_U8, _IP, _IX),
    'csr-first-pointer': lc.csr_line(lc.CSR_ROWS, 3, 4, 4, RRI_F32, [1, 2, 2, 4], _IX),
    'csr-last-pointer': lc.csr_line(lc.CSR_ROWS, 3, 4, 4, RRI_F32, [0, 2, 2, 3], _IX),
    'csr-not-monotone': lc.csr_line(lc.CSR_ROWS, 3, 4, 4, RRI_F32, [0, 2, 1, 4], _IX),
    'csr-column-low': lc.csr_line(lc.CSR_COLUMNS, 3, 4, 4, RRI_F32, _IP, [0, 3, -1, 2]),
    'csr-column-high': lc.csr_line(lc.CSR_COLUMNS, 3, 4, 4, RRI_F32, _IP, [0, 4, 1, 2]),
    'csr-column-unchecked': lc.csr_line(lc.CSR_ROWS, 3, 4, 4, RRI_F32, _IP, [0, 4, 1, 2]),
    'csr-equal-columns': lc.csr_line(lc.CSR_INCREASING, 3, 4, 4, RRI_F32, _IP, [0, 3, 2, 2]),
    'csr-descending': lc.csr_line(lc.CSR_INCREASING, 3, 4, 4, RRI_F32, _IP, [3, 0, 1, 2]),
    'csr-descending-unchecked': lc.csr_line(lc.CSR_COLUMNS, 3, 4, 4, RRI_F32, _IP, [3, 0, 1, 2]),
    # nothing stored: the index and value arrays may be null
    'csr-nnz0': lc.csr_line(lc.CSR_INCREASING, 3, 4, 0, RRI_F64, [0, 0, 0, 0], None, has_data=False),
    'csr-nnz0-arrays': lc.csr_line(lc.CSR_INCREASING, 3, 4, 0, RRI_F64, [0, 0, 0, 0], []),
    'csr-nnz0-pointer': lc.csr_line(lc.CSR_INCREASING, 3, 4, 0, RRI_F64, [0, 0, 0, 1], None, has_data=False),
    'csr-scipy-empty': lc.csr_line(lc.CSR_INCREASING, 3, 4, 0, RRI_F64, sp.csr_matrix((3, 4)).indptr.tolist(), sp.csr_matrix((3, 4)).indices.tolist()),
    # the row sort: 8-byte and 4-byte values travel with their columns
    'sort-sorted': lc.sort_line(8, _IP, _IX, [10, 11, 12, 13]),
    'sort-one-row': lc.sort_line(8, [0, 3, 3, 5], [2, 0, 1, 1, 3], [10, 11, 12, 13, 14]),
    'sort-one-row-f32': lc.sort_line(4, [0, 3, 3, 5], [2, 0, 1, 3, 1], [10, 11, 12, 13, 14]),
    'sort-duplicates': lc.sort_line(8, [0, 3, 3, 5], [2, 0, 2, 1, 3], [10, 11, 12, 13, 14]),
    'sort-sorted-duplicates': lc.sort_line(8, [0, 2, 4], [1, 1, 0, 3], [10, 11, 12, 13]),
    'sort-empty': lc.sort_line(8, [0, 0, 0], [], []),
}


def test_csr_refusals_and_the_row_sort(asked):
    assert asked['csr-fine'] == 'ok'
    for nm in ('csr-no-indptr', 'csr-no-indices', 'csr-no-data', 'csr-negative-nnz'):
        assert asked[nm] == 'bad CSR arrays', nm
    assert asked['csr-half-data'] == asked['csr-count-data'] == 'bad CSR data dtype'
    assert asked['csr-first-pointer'] == asked['csr-last-pointer'] == asked['csr-nnz0-pointer'] == 'indptr does not span nnz'
    assert asked['csr-not-monotone'] == 'indptr not monotone at row 1'
    assert asked['csr-column-low'] == 'column index out of range at 2' and asked['csr-column-high'] == 'column index out of range at 1'
    assert asked['csr-column-unchecked'] == 'ok' and asked['csr-descending-unchecked'] == 'ok'
    assert asked['csr-equal-columns'] == 'column indices of row 2 are not strictly increasing'
    assert asked['csr-descending'] == 'column indices of row 0 are not strictly increasing'
    assert asked['csr-nnz0'] == 'ok' and asked['csr-nnz0-arrays'] == 'ok'
    s = asked['sort-sorted']
    assert (s['copied'], s['copies'], s['dup']) == (0, '0/0', 'ok') and s['indices'].tolist() == _IX and s['values'].tolist() == [10, 11, 12, 13]
    s = asked['sort-one-row']
    assert (s['copied'], s['copies'], s['dup']) == (1, '5/40', 'ok')
    assert s['indices'].tolist() == [0, 1, 2, 1, 3] and s['values'].tolist() == [11, 12, 10, 13, 14]
    s = asked['sort-one-row-f32']
    assert (s['copied'], s['copies'], s['dup']) == (1, '5/20', 'ok')
    assert s['indices'].tolist() == [0, 1, 2, 1, 3] and s['values'].tolist() == [11, 12, 10, 14, 13]
    s = asked['sort-duplicates']           # stable: the two entries of column 2 keep their order
    assert s['copied'] == 1 and s['dup'] == 'row 0 stores column 2 twice (sum the duplicates first)'
    assert s['indices'].tolist() == [0, 2, 2, 1, 3] and s['values'].tolist() == [11, 10, 12, 13, 14]
    s = asked['sort-sorted-duplicates']    # equal neighbours are not "sorted": the row is copied, and refused afterwards
    assert s['copied'] == 1 and s['dup'] == 'row 0 stores column 1 twice (sum the duplicates first)'
    s = asked['sort-empty']
    assert (s['copied'], s['dup']) == (0, 'ok') and len(s['indices']) == 0
    assert asked['csr-scipy-empty'] == 'ok'       # an empty matrix as scipy hands it over
