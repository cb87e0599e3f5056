"""The early-sums schedule (tests/test_early_sums_gpu.py has its first tests) through the geometry, storage and
parameter cases that file does not reach.  Helpers, tolerances and the environment (RRI_ONCHIP=0, RRI_TROW_SMALL=0) are that
file's, by import; every case asserts layout_info()['early_steps'], so none can pass on another route.

What each test is there to break (rri_kernels.hpp unless said otherwise):

  test_job_inside_the_grid           k_pass: `if (bid >= ejob.first) bid -= ejob.nblocks;` and `njobs += ejob.nblocks` -- the pass
                                     has more than early_job_first = 4 n_cu own workgroups, so its workgroups behind the job must be
                                     renumbered (a missing or shifted remap leaves 64 row blocks unread or read twice: an error of
                                     order one); with RRI_PASS_ROT=3 the bound `(bid | 7) < gridDim.x - njobs` of the rotation, which
                                     must count the pass's own workgroups only (P = F + 11: the last group of 8 is partial); with d =
                                     4100 the Gram-row job of nsplit = 2, 2k workgroups in front of both (`bid = blockIdx.x - job.nblocks`).
                                     P = F - 1 and P = F: `early_job_first` = min(P, F), the job last, the remap the identity.
  test_every_build_of_the_pass       rri_hip.hip pass_cfg / pass_k: the twelve k_pass<.., NT, RS, PK, EJ = true> (table below);
                                     early_block<CH>'s batch by sizeof(SX) (4 for float64, 8 otherwise); with NT the kept-block test
                                     `nrb = (gridDim.x - njobs) / npg`, which must not count the job's workgroups.
  test_packed_copies_same_bits       the PK = 1 / 2 builds with the job: the copies decode to X's bits and the job reads no X, so W, T
                                     and the objective equal the fp32 pass's bit for bit.
  test_exception_heavy_records       PK = 2: the byte map of a record's exceptions overlays the row-sum tiles in the dynamic LDS that
                                     the job's workgroups of the same launch use as scratch (tts / gsh / dsh of early_block).
  test_bound_X_inside_nan_bands      the EJ builds read X with the bound stride ldx, the job reads W with ldw: a NaN from the bands
                                     is a read at the wrong stride or past row n.
  test_rank_edges                    early_block: `for (l0 = wave; l0 < k; l0 += 4 * CH)` and `l < k` inside a round of 4 CH columns
                                     (k = 15/16/17 float64, 31/32/33 otherwise); k_trow_early: the first batch `q + 4 i < k` of 64
                                     topics and the loop `l0 = q + 4 * CH` behind it (k = 63/65, 127/128/129), in both halves of it.
  test_row_edges                     early_block: `tile1 = min(ntiles, (b + 1) * e.tpb)` -- at n = 4097 and 4160 about half of the 64
                                     job workgroups walk no tile and store a zero Gpart row that k_wfin's reduce_block sums; k_wfin:
                                     `tile * 64 >= n` at 16 tiles per workgroup (n = 1024 / 1025).
  test_column_edges                  k_trow_early: `((i64)blockIdx.x * 2 + tid) * 128 < d` for tpart (d = 128/129, 384/385) and the
                                     ragged last workgroup of 256 columns (d = 255/256/257).
  test_parameters                    k_wfin: `numer = (y - dt) - p.reg_w_l1`, `cden = nt[0] + p.reg_w_l2` and the `mode == 1`
                                     branch; k_trow_early: `numer = (zj - acc) - p.reg_t_l1`, `c = nw + p.reg_t_l2` and its bounded
                                     branch.
  test_parameters_without_the_schedule   LK::early_ok (rri_hip.hip): fix_T, fix_W and a projected T keep k_wcol.

The twelve builds of the pass that carry the job, and the test that launches each with early_steps asserted (NT: a handle whose X
does not fit RRI_PASS_CACHE_MB, keep_q >= 0 -- here 30011 x 2503 with one row block kept and with none; plain: 200 x 1030):

    storage            plain loads                                   NT (kept row blocks)
    fp32, PK = 0       test_packed_copies_same_bits[200x1030]        test_packed_copies_same_bits[30011x2503-*]
    fp32, PK = 1       test_packed_copies_same_bits[200x1030]        test_packed_copies_same_bits[30011x2503-*]
    fp32, PK = 2       test_packed_copies_same_bits[200x1030]        test_packed_copies_same_bits[30011x2503-*]
    float64            test_every_build_of_the_pass[fp64-200x1030]   test_every_build_of_the_pass[fp64-30011x2503-*]
    float16            test_every_build_of_the_pass[fp16-200x1030]   test_every_build_of_the_pass[fp16-30011x2503-*]
    uint8 and scales   test_every_build_of_the_pass[u8-200x1030]     test_every_build_of_the_pass[u8-30011x2503-*]

Which parameter sets reach the bounded branches (qf_min's scalar c <= 0 with an upper bound, optimization.py:60-65):
  * k_trow_early, mode == 1: c = ||w_t||^2 + reg_t_l2 <= 0 with t_row_sum set -- a dead column of W.  'T-bounded' (t_row_sum = 1,
    reg_t_l1 = -0.01): the numerator is +0.01 everywhere and the row comes out t_row_sum; 'W-bounded': the numerator is 0, the row 0.
  * k_wfin, mode == 1: cden = ||T[t,:]||^2 + reg_w_l2 <= 0 with w_row_sum set.  It needs the T half of the same topic to have left a
    row of zeros WITHOUT ending the run: resets off (the row is kept), a dead column and no negative reg_t_l1 -- 'W-bounded'
    (t_row_sum = w_row_sum = 1, reg_w_l1 = -0.01, reset_topic_method=None): the numerator is +0.01 and the column comes out
    w_row_sum.  With resets on the zero row halts the run first, and the reset that follows drops early_valid: the W half is k_wcol's.
Every other set takes mode 0 in both kernels; the test asserts the branch from the sign of the oracle's own denominator.

Tolerances: single steps against the closed form in float64 numpy on the stored values at 1e-12 in norm and 1e-11 of the largest
entry element-wise (the step tolerance of tests/test_kernel_buckets_gpu.check_steps, which the float16 and uint8 suites use); two
sweeps against the float64 oracle at 2e-9 (their sweep tolerance and tests/test_hip_parity.py's)."""
import numpy as np
import pytest

import cs_cases as cs
import ld_cases as lc
import test_pass_keep_gpu as pk
import test_xnarrow_gpu as xn
import test_xpack_gpu as xg
from conftest import relfro
from test_early_sums_gpu import PARITY_TOL, STEP_TOL, drive, engine, launch_per_phase, oracle, problem, stored  # noqa: F401 (launch_per_phase: autouse)

pytestmark = pytest.mark.gpu

REGS = ('reg_t_l1', 'reg_t_l2', 'reg_w_l1', 'reg_w_l2')


def close(what, got, want):
    """the check of test_single_steps_against_float64; a reference of zeros (a bounded branch) is met exactly"""
    nrm = np.linalg.norm(want)
    if nrm == 0.0:
        print('%s: the reference is 0' % what)
        assert np.array_equal(got, want), (what, float(np.abs(got).max()))
        return
    err = np.linalg.norm(got - want) / nrm
    print('%s: relative error %.3g' % (what, err))
    assert err <= STEP_TOL, (what, err)
    assert np.abs(got - want).max() <= 10 * STEP_TOL * np.abs(want).max(), (what, 'element-wise', float(np.abs(got - want).max() / np.abs(want).max()))


def check_steps(e, Xs, k, ts, params=None, tag=''):
    """update_T_row(t), update_W_col(t) for t in ts on the early-sums schedule, each against the closed form of the step from the
    factors on the device before it (as test_early_sums_gpu.test_single_steps_against_float64, with the penalties and bounds of
    `params` handed to qf_min); everything outside row t / column t bit-equal; early_steps grows by one per topic.  Returns the
    branch of qf_min each step took by the oracle's denominator, as (t, T mode, W mode)."""
    orc, p = oracle(), dict(params or {})
    l1t, l2t, l1w, l2w = (p.get(r, 0.0) for r in REGS)
    steps, modes = e.layout_info()['early_steps'], []
    for t in ts:
        others = np.arange(k) != t
        Wa, Ta = e.get_W(), e.get_T()
        e.update_T_row(t)
        Wb, Tb = e.get_W(), e.get_T()
        wR, nw = orc.residual_products_T(Xs, Wa, Ta, t)
        want = orc.qf_min(-(wR - l1t), nw + l2t, s=None, ub=p.get('t_row_sum'))[0]
        close('%sT row %d' % (tag, t), Tb[t], want)
        assert np.array_equal(Tb[others], Ta[others]) and np.array_equal(Wb, Wa), ('T step', t, 'wrote outside row t')
        e.update_W_col(t)
        Wc, Tc = e.get_W(), e.get_T()
        Rt, nt = orc.residual_products_W(Xs, Wb, Tb, t)
        want = orc.qf_min(-(Rt - l1w), nt + l2w, s=None, ub=p.get('w_row_sum'))[0]
        close('%sW column %d' % (tag, t), Wc[:, t], want)
        assert np.array_equal(Wc[:, others], Wb[:, others]) and np.array_equal(Tc, Tb), ('W step', t, 'wrote outside column t')
        steps += 1
        assert e.layout_info()['early_steps'] == steps, ('the W half of topic %d did not take k_wfin' % t, e.layout_info()['early_steps'], steps)
        modes.append((t, int(not nw + l2t > 0.0), int(not nt + l2w > 0.0)))
    return modes


def two_sweeps_on_the_schedule(e, k, ref, tag=''):
    """two sweeps (no event), every W half through k_wfin, W and T against the oracle's at 2e-9; returns (W, T, objective)"""
    before = e.layout_info()['early_steps']
    assert drive(e, 2) == []
    took = e.layout_info()['early_steps'] - before
    assert took == 2 * k, ('%sW halves that took k_wfin' % tag, took, 2 * k)
    W, T = e.get_W(), e.get_T()
    ew, et = relfro(W, ref['W']), relfro(T, ref['T'])
    print('%stwo sweeps against the oracle: W %.3g T %.3g' % (tag, ew, et))
    assert ew < PARITY_TOL and et < PARITY_TOL, (tag, ew, et)
    return W, T, e.objective()


def reference(Xs, k, W0, T0):
    return oracle().nmf(Xs, k, W_in=W0.copy(), T_in=T0.copy(), max_iter=2, eps_stop=-1)


# ---- A1. the job inside the grid ---------------------------------------------------------------------------------------------
# RRI_PASS_PK_GEOM=16c / 16i: 16 rows per workgroup of an fp32 handle, so that P = npanels * ceil(n / 16) passes F = 4 n_cu at sizes
# of a few MB.  d = 130 is one panel; 2503 three; 4100 five, with nsplit = 2 column slices of the Gram-row job (d >= 4096).  Where
# P is not to be a multiple of the panel count's row blocks the last row block holds ONE row (n = 16 (nrb - 1) + 1), at d = 4100 four.
A1_SHAPES = ('F-1', 'F', 'F+1', 'F+11', '2F', 'three-panels', 'five-panels-nsplit2')
A1_INSIDE = A1_SHAPES[2:]


def a1_shape(name, n_cu):
    """(n, d, k, P, the side of F = 4 n_cu that P lies on); at n_cu = 256: n = 16368, 16384, 16385, 16545, 32768, 5473 (P = 1029), 3300 (P = 1035)"""
    F = 4 * n_cu
    if name in ('F-1', 'F', '2F'):
        P = {'F-1': F - 1, 'F': F, '2F': 2 * F}[name]
        return 16 * P, 130, 5, P, 'below' if P < F else 'at' if P == F else 'above'
    if name in ('F+1', 'F+11'):             # F + 8 + 3: the last group of 8 workgroups is partial
        P = F + int(name[2:])
        return 16 * (P - 1) + 1, 130, 5, P, 'above'
    if name == 'three-panels':
        nrb = F // 3 + 2
        return 16 * (nrb - 1) + 1, 2503, 4, 3 * nrb, 'above'
    nrb = F // 5 + 3
    return 16 * (nrb - 1) + 4, 4100, 4, 5 * nrb, 'above'


_N_CU = []


def device_n_cu(monkeypatch):
    if not _N_CU:
        with engine(monkeypatch, None, 64, 8, 2, dtype=np.float64) as e:
            _N_CU.append(e.layout_info()['n_cu'])
    return _N_CU[0]


A1_CASES = [(name, geom, rot) for name in A1_SHAPES for geom in ('16c', '16i') for rot in ((None, '3') if name in A1_INSIDE else (None,))]


@pytest.mark.parametrize('name,geom,rot', A1_CASES, ids=['%s-%s%s' % (nm, g, '-rot3' if r else '') for nm, g, r in A1_CASES])
def test_job_inside_the_grid(monkeypatch, name, geom, rot):
    n_cu = device_n_cu(monkeypatch)
    F = 4 * n_cu
    n, d, k, P, side = a1_shape(name, n_cu)
    X, W0, T0 = problem(n, d, k, seed=23)
    Xs = stored(X, np.float32)
    monkeypatch.setenv('RRI_PASS_PK_GEOM', geom)
    if rot is not None:
        monkeypatch.setenv('RRI_PASS_ROT', rot)
    with engine(monkeypatch, None, n, d, k, dtype=np.float32) as e:
        monkeypatch.delenv('RRI_PASS_PK_GEOM'), monkeypatch.delenv('RRI_PASS_ROT', raising=False)
        e.upload_X(X.astype(np.float32)); e.set_W(W0); e.set_T(T0); e.set_params()
        info = e.layout_info()
        assert info['early_sums'] and info['rpb'] == 16 and info['interleaved'] == (geom == '16i'), info
        got_P = info['npanels'] * info['nrb']
        assert got_P == P and info['npanels'] == {130: 1, 2503: 3, 4100: 5}[d], (info, P)
        assert {'below': got_P < F, 'at': got_P == F, 'above': got_P > F}[side], \
            'the pass has %d own workgroups, 4 n_cu = %d: the case is not on the side of it that it names (%s)' % (got_P, F, side)
        check_steps(e, Xs, k, sorted({0, 1, k - 1}))
        e.set_W(W0); e.set_T(T0)
        two_sweeps_on_the_schedule(e, k, reference(Xs, k, W0, T0))
        assert e.n_resets_used == 0


# ---- A2. every build of the pass that carries the job -----------------------------------------------------------------------------
SMALL, LARGE = (200, 1030, 5), (30011, 2503, 4)
CAPS = ('one row block kept', 'nothing kept')
_PROBLEMS = {}


def store_problem(store, shape):
    """(dtype, load(e), X as stored in float64, W0, T0, the oracle's two sweeps); the one large problem of a store is kept until
    another is asked for (600 MB of float64 each)"""
    key = (store, shape)
    if key not in _PROBLEMS:
        _PROBLEMS.clear()
        n, d, k = shape
        if store == 'u8':                   # counts times scales, as tests/test_count_storage_gpu.py and test_pass_keep_gpu.py form them
            C, r, s, Xs, W0, T0 = pk.count_problem(n, d, k, seed=5)
            dtype, load = np.uint8, pk.load_counts(C, r, s)
        else:
            X, W0, T0 = pk.host_problem(n, d, k, seed=5)
            dtype = {'fp16': np.float16, 'fp32': np.float32, 'fp64': np.float64}[store]
            Xd = X.astype(dtype)
            Xs = np.ascontiguousarray(Xd.astype(np.float64))       # float16: the stored values cast back
            load = lambda e: e.upload_X(Xd)
        _PROBLEMS[key] = (dtype, load, Xs, W0, T0, reference(Xs, k, W0, T0))
    return _PROBLEMS[key]


def streams(n, d, k, dtype, info, cap):
    """pass_keep restated: does an X of this geometry stream (non-temporal loads, keep_q >= 0) under the capacity `cap` (MB; None:
    the default 256)?"""
    xb, block, chain = pk.geometry(n, d, k, dtype, info)
    return xb > (256.0 if cap is None else float(cap)) * 1e6 - chain


def run_build(monkeypatch, tag, shape, dtype, load, Xs, W0, T0, ref, cap=None, pack=None):
    """one handle on the schedule: two sweeps against the oracle, then single steps from where they ended (the packed copies are
    built by the first sweep); returns (W, T, objective) after the sweeps and layout_info at the end"""
    n, d, k = shape
    for name, val in ((pk.ENV, cap), (xg.ENV, pack)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    with engine(monkeypatch, None, n, d, k, dtype=dtype) as e:
        monkeypatch.delenv(pk.ENV, raising=False), monkeypatch.delenv(xg.ENV, raising=False)
        load(e); e.set_W(W0); e.set_T(T0); e.set_params()
        assert e.layout_info()['early_sums']
        out = two_sweeps_on_the_schedule(e, k, ref, tag)
        check_steps(e, Xs, k, sorted({0, 1, k - 1}), tag=tag)
        info = e.layout_info()
        assert streams(n, d, k, dtype, info, cap) == (shape == LARGE), (tag, 'non-temporal loads', info)
        assert e.n_resets_used == 0
    return out, info


BUILDS = [(store, SMALL, None) for store in ('fp16', 'u8', 'fp64')] + [(store, LARGE, cap) for store in ('fp16', 'u8', 'fp64') for cap in CAPS]


def build_id(store, shape, cap):
    return '%s%dx%d%s' % (store + '-' if store else '', shape[0], shape[1], '-' + cap.replace(' ', '_') if cap else '')


@pytest.mark.parametrize('store,shape,cap', BUILDS, ids=[build_id(*b) for b in BUILDS])
def test_every_build_of_the_pass(monkeypatch, store, shape, cap):
    dtype, load, Xs, W0, T0, ref = store_problem(store, shape)
    caps = pk.settings(shape[0], shape[1], shape[2], dtype)[1] if cap else {None: None}
    run_build(monkeypatch, '%s, %s: ' % (store, cap or 'plain loads'), shape, dtype, load, Xs, W0, T0, ref, cap=caps[cap])


PACKED = [(None, SMALL, None)] + [(None, LARGE, cap) for cap in CAPS]


@pytest.mark.parametrize('store,shape,cap', PACKED, ids=[build_id(*b) for b in PACKED])
def test_packed_copies_same_bits(monkeypatch, store, shape, cap):
    """fp32 under RRI_X_PACK=0, 1 and 2, the schedule on: each against float64, and the three equal bit for bit"""
    dtype, load, Xs, W0, T0, ref = store_problem('fp32', shape)
    caps = pk.settings(shape[0], shape[1], shape[2], dtype)[1] if cap else {None: None}
    res = {}
    for pack, bits in (('0', 0), ('1', 28), ('2', 26)):
        res['RRI_X_PACK=' + pack], info = run_build(monkeypatch, 'RRI_X_PACK=%s, %s: ' % (pack, cap or 'plain loads'), shape, dtype, load, Xs, W0, T0,
                                                    ref, cap=caps[cap], pack=pack)
        assert info['x_pack_bits'] == bits and info['x_pack'] == (bits > 0), info
    pk.assert_same_bits(res)


def exception_heavy():
    """test_xnarrow_gpu.hand_built with one record in which every element is an exception (chunk 5, panel 1: sixteen exponent bytes
    of the window, none frequent enough for the book) and one with 65 of them (the last chunk, panel 0: a second round of the
    entry loop), positions 0 and 2047 among them"""
    n, d, k, X, W0, T0, base, rs = xn.hand_built(47)
    q = 5
    for j in range(16):
        X[8 * q:8 * q + 8, 256 + 16 * j:272 + 16 * j] = xn.with_exponent(rs, (8, 16), 2 * base + 1 + j)
    q2, rare = 24, 2 * base + 18
    blk = xn.with_exponent(rs, (8, 256), 127)
    where = {(0, 0), (7, 255)}
    while len(where) < 65:
        where.add((int(rs.randint(8)), int(rs.randint(256))))
    for r, c in where:
        blk[r, c] = xn.with_exponent(rs, (), rare)
    X[8 * q2:8 * q2 + 8, 0:256] = blk
    assert xg.window_base(X) == base
    book, _ = xn.books_of(X, base, n * 2)
    assert [xn.exceptions_of_record(X, book, q, 1), xn.exceptions_of_record(X, book, q2, 0)] == [2048, 65], book
    return n, d, k, X, W0, T0, base


def test_exception_heavy_records(monkeypatch):
    """the byte map of the exceptions and the job's scratch in the LDS of ONE launch: three ways, equal bits, early_steps == 2k (asserted
    by two_sweeps_on_the_schedule) and each against float64"""
    n, d, k, X, W0, T0, base = exception_heavy()
    Xs = np.ascontiguousarray(X.astype(np.float64))
    ref = reference(Xs, k, W0, T0)
    res, infos = {}, {}
    for pack in ('0', '1', '2'):
        res['RRI_X_PACK=' + pack], infos[pack] = run_build(monkeypatch, 'RRI_X_PACK=%s: ' % pack, (n, d, k), np.float32, lambda e: e.upload_X(X), Xs,
                                                           W0, T0, ref, pack=pack)
    xn.check_infos(infos, n, base, infos['1']['x_pack_flagged'], X, pad_zeros=n * 2)
    assert infos['2']['x_pack_exceptions'] >= 2048 + 65
    pk.assert_same_bits(res)


@pytest.mark.parametrize('store', ['fp32', 'fp64'])
def test_bound_X_inside_nan_bands(monkeypatch, store):
    """a bound X of two column panels with a row stride 65 vectors above d and a column offset, NaN all around it"""
    import torch
    c = lc.CASES[lc.cases(store=store, widths=(2,), pads=(1,))[0]]
    k = 3
    X = lc.case_matrix(c)
    g = lc.guarded(torch, X, c.ld, c.c0, device='cuda:0')
    torch.cuda.synchronize()
    rs = np.random.RandomState(1)
    a = float(np.sqrt(X.mean() / k))
    W0, T0 = a * rs.rand(c.n, k), a * rs.rand(k, c.d)
    Xs = np.ascontiguousarray(X.astype(np.float64))
    with engine(monkeypatch, None, c.n, c.d, k, dtype=c.dtype) as e:
        e.bind_X_device(g.ptr, g.ld); e.set_W(W0); e.set_T(T0); e.set_params()
        info = e.layout_info()
        assert info['early_sums'] and info['npanels'] == 2 and info['rpb'] <= lc.G, info
        W, T, obj = two_sweeps_on_the_schedule(e, k, reference(Xs, k, W0, T0))
        assert np.isfinite(W).all() and np.isfinite(T).all() and np.isfinite(obj)
        check_steps(e, Xs, k, [0, 1, 2])
    g.check('the bound X')


# ---- A3. edges of k, n and d ---------------------------------------------------------------------------------------------------------
RANKS = [15, 16, 17, 31, 32, 33, 63, 65, 127, 128, 129]


def edge_topics(k):
    """0, k - 1, and around every batch edge below k: the last topic of a full batch and the first of the next -- rounds of 16
    (float64) and 32 columns of early_block, batches of 64 topics of k_trow_early"""
    ts = {0, k - 1}
    for b in (16, 32, 64, 128):
        if b < k:
            ts |= {b - 1, b}
    return sorted(ts)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('k', RANKS)
def test_rank_edges(monkeypatch, k, dtype):
    n, d = 200, 300
    X, W0, T0 = problem(n, d, k, seed=29)
    with engine(monkeypatch, None, n, d, k, dtype=dtype) as e:
        e.upload_X(X.astype(dtype)); e.set_W(W0); e.set_T(T0); e.set_params()
        assert e.layout_info()['early_sums']
        check_steps(e, stored(X, dtype), k, edge_topics(k))
        assert e.n_resets_used == 0


def steps_at(monkeypatch, n, d, k, dtype, seed):
    X, W0, T0 = problem(n, d, k, seed=seed)
    with engine(monkeypatch, None, n, d, k, dtype=dtype) as e:
        e.upload_X(X.astype(dtype)); e.set_W(W0); e.set_T(T0); e.set_params()
        assert e.layout_info()['early_sums']
        check_steps(e, stored(X, dtype), k, sorted({0, 1, k - 1}))
        assert e.n_resets_used == 0


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('n', [1024, 1025, 4096, 4097, 4160])
def test_row_edges(monkeypatch, n, dtype):
    """d = 130, k = 5.  1024 / 1025: 16 tiles, one tile workgroup of k_wfin, and a 17th tile in a second; 4096: 64 tiles, one for each
    of the 64 job workgroups; 4097 (a tile of one row) and 4160 (a full one): 65 tiles, two per job workgroup, so that 33 walk tiles
    and 31 store a row of zeros (tests/test_layout_cpu.py pins these counts at 256 CUs)"""
    steps_at(monkeypatch, n, 130, 5, dtype, seed=31)


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['fp64', 'fp32'])
@pytest.mark.parametrize('d', [128, 129, 255, 256, 257, 384, 385])
def test_column_edges(monkeypatch, d, dtype):
    """n = 200, k = 5: workgroups of 256 columns in k_trow_early, each leaving two entries of tpart of 128 columns"""
    steps_at(monkeypatch, 200, d, 5, dtype, seed=37)


# ---- A4. parameters ------------------------------------------------------------------------------------------------------------------
ON = {name: dict(p) for name, p in cs.PARAMS.items() if cs.early_schedule(name)}      # free, clip (t_row_sum), pen_a (all four penalties), pen_b (l2)
ON.update({'w_row_sum': dict(w_row_sum=1.0), 'both_row_sums': dict(t_row_sum=1.0, w_row_sum=1.0),
           'both_row_sums_pen_a': dict(cs.PARAMS['pen_a'], t_row_sum=1.0, w_row_sum=1.0)})
OFF = {name: dict(p) for name, p in cs.PARAMS.items() if not cs.early_schedule(name)}
DEAD = 2
# a dead column of W and resets off: the parameter sets that reach qf_min's bounded branch, and in which kernel (module docstring)
BOUNDED = {'T-bounded': (dict(t_row_sum=1.0, reg_t_l1=-0.01, reset_topic_method=None), (1, 0)),
           'W-bounded': (dict(t_row_sum=1.0, w_row_sum=1.0, reg_w_l1=-0.01, reset_topic_method=None), (1, 1))}


@pytest.mark.parametrize('name', list(ON) + list(BOUNDED))
def test_parameters(monkeypatch, name):
    n, d, k = 200, 1030, 6
    X, W0, T0 = problem(n, d, k, seed=41)
    params, dead_modes = BOUNDED[name] if name in BOUNDED else (ON[name], None)
    if dead_modes:
        W0 = W0.copy(); W0[:, DEAD] = 0.0
    with engine(monkeypatch, None, n, d, k, dtype=np.float64) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(**params)
        assert e.layout_info()['early_sums']
        modes = check_steps(e, X, k, [0, 1, DEAD, k - 1], params={key: val for key, val in params.items() if key != 'reset_topic_method'})
        for t, mt, mw in modes:         # the branch, from the oracle's own denominators
            assert (mt, mw) == (dead_modes if dead_modes and t == DEAD else (0, 0)), (name, t, mt, mw)
        if dead_modes:
            want = params['t_row_sum'] if name == 'T-bounded' else 0.0
            assert (e.get_T()[DEAD] == want).all(), 'k_trow_early, mode == 1: the bound or nothing'
            if name == 'W-bounded':
                assert (e.get_W()[:, DEAD] == params['w_row_sum']).all(), 'k_wfin, mode == 1: every entry at w_row_sum'
        assert e.n_resets_used == 0


def test_the_parameter_sets_are_those_of_the_state_suite():
    assert sorted(ON) == ['both_row_sums', 'both_row_sums_pen_a', 'clip', 'free', 'pen_a', 'pen_b', 'w_row_sum'] and sorted(OFF) == ['fix_T', 'fix_W', 'simplex']


@pytest.mark.parametrize('name', sorted(cs.PARAMS))
def test_parameters_without_the_schedule(monkeypatch, name):
    """projection, fix_W, fix_T: early_sums is false and a sweep takes no k_wfin; every other set of cs_cases.PARAMS: true, and it does"""
    n, d, k = 200, 1030, 6
    X, W0, T0 = problem(n, d, k, seed=41)
    params = cs.PARAMS[name]
    with engine(monkeypatch, None, n, d, k, dtype=np.float64) as e:
        if name == 'simplex':
            T0 = oracle().proj_rows_simplex(T0.copy(), 1.0)
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(**params)
        assert e.layout_info()['early_sums'] == (name in ON), (name, e.layout_info())
        e.sweep(1)
        assert e.layout_info()['early_steps'] == (k if name in ON else 0), (name, e.layout_info())
