"""rri_bind_X_device / rri_bind_mask_device on a column-and-row slice of a wider device array: row stride ld > d, the slice inside
bands of NaN (tests/ld_cases.py).

Every test makes twin handles of one shape and storage type.  Handle A gets upload_X (and upload_mask) of the host matrix,
handle B is bound to the guarded slice on the device; both get the same W0, T0 and parameters.  Then, operation by operation:
  (a) B's outputs are finite -- a kernel that read the band, by a wrong stride or past column d / row n, returns NaN;
  (b) B's outputs equal A's bit for bit: kernels, grids and summation orders take n, d and the handle's geometry, never ldx
      (a bound X has no pad columns, so d % VN == 0 and A's stride is d: the two differ in the stride alone).  The one place
      where this is not asserted is a persistent launch that gave up on one twin only (a shared device): the launch-per-phase
      schedule sums in another order, which rri_sweep documents;
  (c) B's outputs meet the float64 numpy / oracle reference at the bound the suite holds that operation to elsewhere
      (test_kernel_buckets_gpu.py for single operations, 2e-9 of test_hip_parity.py for sweeps, the fp32 stored-residual bound
      of test_fuzz_gpu.py, one storage ulp of test_residual_gpu.py for a stored residual);
  (d) after both handles are closed and the device synchronised, the whole guarded allocation -- matrix included -- has the bits
      it had before the bind: bound memory is never written.

The weighted cases bind X and the mask from two allocations with DIFFERENT strides, so a swapped ldx / ldm shows.

uint8 counts (RRI_U8) join every test the float16 cases join.  Their band is the byte 0xFF (tests/ld_cases.py says what that sees
and what it cannot), so for them (a) says nothing and (c) carries the check: a 255 in a sum is far outside every bound.  Both twins
get log-uniform row and column scales AFTER the upload / the bind, which puts both vectors back to ones, and the reference is the
oracle on (C * s) * r[:, None].  One test is theirs alone: rri_scale_X on bound memory, which writes the scale vectors only.
"""
import contextlib
import threading

import numpy as np
import pytest

import ld_cases as lc
import test_kernel_buckets_gpu as kb
from conftest import relfro
from rri_nmf_amd.synthetic import scaled_init

pytestmark = pytest.mark.gpu

K = 5
TOPIC = dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
FLAGS = {'plain': dict(), 'topic': TOPIC}
SWEEP_TOL = 2e-9                    # test_hip_parity.py: same algorithm, another summation order
STORED_FP32_TOL = 5e-3              # test_fuzz_gpu.py: a maintained fp32 residual is rounded at every update
DENSE = ('fp32', 'fp64')            # the storage types of everything that is not the read-only Gram form
READ_ONLY = ('fp16', 'u8')          # the stores that never take the persistent launch


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def oracle():
    from oracle import rri_oracle
    return rri_oracle


def other_stride(c):
    """the (ld, c0) of the case's width that the case itself does not use: the mask's, so that ldm != ldx"""
    (a, b) = lc.strides_of(c.d, c.dtype)
    return b if (c.ld, c.c0) == a else a


class Twins(object):
    pass


@contextlib.contextmanager
def twins(case, k=K, kind='plain', X=None, M=None, bind_only=False, scales=None):
    """A: uploaded, B: bound to the guarded slice(s).  X / M: host matrices (default: the case's own X, no mask).  uint8: both
    get scales (default: the case's own) once X is there, and X64 is the scaled matrix.  On exit both handles are closed, the
    device is synchronised and every guarded allocation is compared with what it was (d)."""
    import torch
    c = lc.CASES[case]
    X = lc.case_matrix(c) if X is None else np.ascontiguousarray(np.asarray(X).astype(c.dtype))
    kw = dict(dtype=c.dtype)
    if kind == 'residual':
        kw['schedule'] = 'residual'
    elif kind == 'weighted':
        kw['weighted'] = True
    t = Twins()
    t.case, t.X, t.X64 = c, X, np.ascontiguousarray(X.astype(np.float64))
    t.scales = None
    if c.store == 'u8':
        t.scales = lc.case_scales(c) if scales is None else scales
        t.X64 = lc.scaled(X, *t.scales)
    t.gx = lc.guarded(torch, X, c.ld, c.c0, device='cuda:0')
    t.gm = None
    if M is not None:
        M = np.ascontiguousarray(np.asarray(M).astype(c.dtype))
        ldm, c0m = other_stride(c)
        assert ldm != c.ld
        t.gm = lc.guarded(torch, M, ldm, c0m, device='cuda:0')
    torch.cuda.synchronize()
    t.A = None if bind_only else engine(c.n, c.d, k, **kw)
    t.B = engine(c.n, c.d, k, **kw)
    try:
        if t.A is not None:
            t.A.upload_X(X)
            if M is not None:
                t.A.upload_mask(M)
        t.B.bind_X_device(t.gx.ptr, t.gx.ld)
        if M is not None:
            t.B.bind_mask_device(t.gm.ptr, t.gm.ld)
        if t.scales is not None:
            for e in (t.A, t.B):
                if e is not None:
                    e.set_X_scales(*t.scales)
        assert lc.G >= t.B.layout_info()['rpb'], 'the guard rows must cover a row block of the pass: %r' % (t.B.layout_info(),)
        yield t
    finally:
        for e in (t.A, t.B):
            if e is not None:
                e.close()
        torch.cuda.synchronize()
    t.gx.check('the allocation X was bound in')
    if t.gm is not None:
        t.gm.check('the allocation the mask was bound in')


def both(t, fn):
    """fn on the uploaded twin, then on the bound one"""
    return fn(t.A), fn(t.B)


def flat(out):
    if isinstance(out, (tuple, list)):
        return [v for o in out for v in flat(o)]
    return [np.asarray(out)]


def assert_finite(out, what):
    for i, v in enumerate(flat(out)):
        if v.dtype.kind == 'f':
            assert np.isfinite(v).all(), '%s: output %d of the bound handle has %d non-finite value(s)' % (what, i, int((~np.isfinite(v)).sum()))


def assert_same_bits(a, b, what):
    fa, fb = flat(a), flat(b)
    assert len(fa) == len(fb)
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i, x.shape, y.shape, x.dtype, y.dtype)
        if x.tobytes() != y.tobytes():
            diff = np.atleast_2d(x != y) | np.atleast_2d(np.isnan(x) != np.isnan(y))
            raise AssertionError('%s: output %d of the bound handle differs from the uploaded twin in %d of %d elements: %s' % (
                what, i, int(diff.sum()), diff.size, '; '.join(kb.blocks(diff)[:6])))


def start(c, X64, k, flags=None, seed=1):
    W0, T0 = scaled_init(X64, k, seed=seed)
    if flags and flags.get('project_T_each_iter'):
        T0 = oracle().proj_rows_simplex(T0, flags['t_row_sum'])       # what the driver hands over; the oracle's own projection is then the identity
    return np.ascontiguousarray(W0), np.ascontiguousarray(T0)


def run_sweeps(e, W0, T0, sweeps, flags):
    e.set_W(W0); e.set_T(T0); e.set_params(**flags)
    e.sweep(sweeps)
    return e.get_W(), e.get_T(), e.objective(), e.n_resets_used


def check_sweeps(t, W0, T0, sweeps, flags, tol, what, same_bits=True, M=None):
    a, b = both(t, lambda e: run_sweeps(e, W0, T0, sweeps, flags))
    assert_finite(b, what)
    if same_bits:
        assert_same_bits(a, b, what)
    ref = oracle().nmf(t.X64, W0.shape[1], W_mat=M, W_in=W0.copy(), T_in=T0.copy(), max_iter=sweeps, eps_stop=-1,
                       do_final_project_W=False, **flags)        # (the projection after the last sweep is the driver's, not rri_sweep's)
    ew, et = relfro(b[0], ref['W']), relfro(b[1], ref['T'])
    print('%s: relfro W %.3e T %.3e (bound %.1e)' % (what, ew, et, tol))
    assert ew < tol and et < tol and b[3] == ref['n_resets_used'], (what, ew, et, tol, b[3], ref['n_resets_used'])
    return a, b


# ---- RRI_UNWEIGHTED: sweeps -------------------------------------------------------------------------------------------------
SWEEP_PARAMS = [(name, flags, route) for name in lc.CASES for flags in FLAGS
                for route in (('phases',) if lc.CASES[name].store in READ_ONLY else ('phases', 'default'))]


@pytest.mark.parametrize('case,flags,route', SWEEP_PARAMS, ids=['%s-%s-%s' % p for p in SWEEP_PARAMS])
def test_two_sweeps(monkeypatch, case, flags, route):
    """route 'phases': RRI_ONCHIP=0, the launch-per-phase schedule (k_pass with ldx, non-temporal or plain); 'default': the
    persistent launch wherever the shape is eligible (its loader takes a.ldx).  A float16 or uint8 handle never takes that
    launch, so it has the one route."""
    c = lc.CASES[case]
    if route == 'phases':
        monkeypatch.setenv('RRI_ONCHIP', '0')
    else:
        monkeypatch.delenv('RRI_ONCHIP', raising=False)
    with twins(case) as t:
        W0, T0 = start(c, t.X64, K, FLAGS[flags])
        for e in (t.A, t.B):
            e.set_W(W0); e.set_T(T0); e.set_params(**FLAGS[flags])
        # rri_onchip_info: plain with d <= 2048, the topic-model flags with d <= 1024 -- and no back-off pending: a persistent launch
        # that gave up on a shared device (this test's or an earlier one's in the process) keeps every handle off the path for a
        # while, so eligibility depends on the clock.  The uploaded twin, read FIRST, is the control: time can only end a back-off
        # between the two reads, so "uploaded eligible, bound not" is never the clock
        want = route == 'default' and (flags == 'plain' or c.d <= 1024)
        eligible = t.A.onchip_info()[0], t.B.onchip_info()[0]
        assert not (eligible[0] and not eligible[1]), 'a bound X with a 16-byte stride is as eligible as an uploaded one'
        if not want:
            assert eligible == (False, False), (eligible, flags, route)
        check_sweeps(t, W0, T0, 2, FLAGS[flags], SWEEP_TOL, 'two sweeps, %s, %s' % (flags, route),
                     same_bits=False)
        fell_back = t.A.onchip_fallbacks(), t.B.onchip_fallbacks()
        if not want:
            assert t.A.onchip_info()[1] == 0 and t.B.onchip_info()[1] == 0
        elif eligible == (True, True) and fell_back == (0, 0):
            # (no back-off before the sweeps and none started by them: both ran as persistent launches)
            assert t.A.onchip_info()[1] >= 1 and t.B.onchip_info()[1] >= 1, ('a persistent launch was expected', t.A.onchip_info(), t.B.onchip_info())
        a = t.A.get_W(), t.A.get_T(), t.A.objective()
        b = t.B.get_W(), t.B.get_T(), t.B.objective()
        if fell_back == (0, 0):         # (a launch that gave up on one twin reran on the other schedule: another summation order)
            assert_same_bits(a, b, 'two sweeps, %s, %s' % (flags, route))


# every width and both strides of every storage type, at the larger row count of the width
STEP_CASES = [n for n in lc.CASES if lc.CASES[n].n != 130]
# (W fixed at a random start empties rows of T: with the default reset method the run goes through rri_apply_reset_max_resid --
# the arg-max search and the reset row, both over X with ldx -- where the reference, without one, raises "unbounded")
HALVES = {'fix_T-one-launch': ('1', dict(fix_T=True, reset_topic_method=None)),
          'fix_T-per-topic': ('0', dict(fix_T=True, reset_topic_method=None)), 'fix_W': ('1', dict(fix_W=True))}


@pytest.mark.parametrize('half', list(HALVES))
@pytest.mark.parametrize('case', STEP_CASES)
def test_two_sweeps_with_a_fixed_half(monkeypatch, case, half):
    """fix_T: X T^T by k_xtt_mfma (ldx) once per T, then the W half as one launch per sweep or, RRI_WSWEEP=0, topic by topic;
    fix_W: the T rows alone"""
    c = lc.CASES[case]
    wsweep, flags = HALVES[half]
    monkeypatch.setenv('RRI_WSWEEP', wsweep)
    with twins(case) as t:
        W0, T0 = start(c, t.X64, K)
        for e in (t.A, t.B):
            e.timing_enable(True)
        check_sweeps(t, W0, T0, 2, flags, SWEEP_TOL, half)
        if 'fix_T' in half:
            launches = t.B.timing_read(1)[0]
            assert launches == 2 if wsweep == '1' else launches >= 2 * K, (half, launches)


@pytest.mark.parametrize('flags', list(FLAGS))
@pytest.mark.parametrize('case', STEP_CASES)
def test_single_half_steps(case, flags):
    """update_T_row(t) and update_W_col(t) alone, against the closed form of the step (test_kernel_buckets_gpu.check_steps)"""
    c = lc.CASES[case]
    with twins(case) as t:
        W0, T0 = start(c, t.X64, K, FLAGS[flags])
        for e in (t.A, t.B):
            e.set_W(W0); e.set_T(T0); e.set_params(**FLAGS[flags])
        kb.check_steps(t.B, t.X64, K, FLAGS[flags])                # t = 0 and k - 1
        for tt in (0, K - 1):
            t.A.update_T_row(tt)
            t.A.update_W_col(tt)
        b = t.B.get_W(), t.B.get_T()
        assert_finite(b, 'half steps')
        assert_same_bits((t.A.get_W(), t.A.get_T()), b, 'half steps')


# ---- RRI_UNWEIGHTED: the residual kernel family -------------------------------------------------------------------------------
RESID_K = [5, 70, 300]           # k_resid_mfma | k_resid with the W tile in LDS | k_resid with a W slice per column tile


@pytest.mark.parametrize('k', RESID_K, ids=[kb.resid_bucket(k) for k in RESID_K])
@pytest.mark.parametrize('case', STEP_CASES)
def test_objective_right_after_set_factors(case, k):
    c = lc.CASES[case]
    with twins(case, k=k) as t:
        W0, T0 = start(c, t.X64, k)
        regs = dict(reg_w_l1=0.03, reg_w_l2=0.2, reg_t_l1=0.01, reg_t_l2=0.5)

        def run(e):
            e.set_W(W0); e.set_T(T0); e.set_params()
            out = [e.objective(), e.objective_parts()]
            e.set_params(**regs)
            return out + [e.objective()]
        a, b = both(t, run)
        assert_finite(b, 'objective')
        assert_same_bits(a, b, 'objective')
        want = oracle().true_objective(t.X64, W0, T0)
        kb.assert_rel(b[0], want, 1e-12, 'objective')
        kb.assert_rel(b[1][0], want, 1e-12, 'objective_parts[0]')
        kb.assert_rel(b[1][1], float((W0 ** 2).sum()), 1e-12, 'objective_parts[1]')
        kb.assert_rel(b[1][2], float(np.abs(W0).sum()), 1e-12, 'objective_parts[2]')
        kb.assert_rel(b[2], oracle().true_objective(t.X64, W0, T0, **regs), 1e-12, 'objective with penalties')


@pytest.mark.parametrize('k', RESID_K, ids=[kb.resid_bucket(k) for k in RESID_K])
@pytest.mark.parametrize('case', STEP_CASES)
def test_max_resid_row_and_reset_row(case, k):
    """the arg-max row is the LAST row of the matrix: the row whose lower neighbour is the band"""
    c = lc.CASES[case]
    X = lc.case_matrix(c).astype(np.float64)
    star = c.n - 1
    scales = None
    if c.store == 'u8':         # counts end at 255: the other rows a quarter of theirs, and the largest row scale twice over
        X = np.floor(X / 4.0)
        X[star] = 255.0
        r, s = lc.case_scales(c)
        r[star] = 2.0 * r.max()
        scales = (r, s)
    else:
        X[star] += 2.0 * X.max()
    with twins(case, k=k, X=X, scales=scales) as t:
        W0, T0 = start(c, t.X64, k)
        R = t.X64 - W0 @ T0
        pos = (np.maximum(R, 0.0) ** 2).sum(axis=1)
        assert np.argmax(pos) == star and np.sort(pos)[-2] < 0.5 * pos[star]
        rows = sorted({star, 0, 64, c.n - 2})

        def run(e):
            e.set_W(W0); e.set_T(T0); e.set_params()
            val, row = e.resid_row_argmax()
            return [val, np.int64(row)] + [e.reset_row(i) for i in rows]
        a, b = both(t, run)
        assert_finite(b, 'resid_row_argmax / reset_row')
        assert_same_bits(a, b, 'resid_row_argmax / reset_row')
        assert int(b[1]) == star, 'arg-max row %d, want %d' % (b[1], star)
        kb.assert_rel(b[0], pos[star], 1e-12, 'sum_j max(X - W T, 0)^2 of row %d' % star)
        bound = kb.resid_bound(t.X64, W0, T0)
        for i, got in zip(rows, b[2:]):
            kb.assert_elementwise(got[None, :], np.maximum(R[i], 0.0)[None, :], bound[i][None, :], 'reset row %d' % i)


# ---- RRI_UNWEIGHTED: products with the resident X -----------------------------------------------------------------------------
@pytest.mark.parametrize('m', [3, 17, 64])
@pytest.mark.parametrize('case', STEP_CASES)
def test_X_times_and_Xt_times(case, m):
    c = lc.CASES[case]
    rs = np.random.RandomState(m)
    B, Q = rs.randn(c.d, m), rs.randn(c.n, m)
    with twins(case) as t:
        a, b = both(t, lambda e: (e.X_times(B), e.Xt_times(Q)))
        assert_finite(b, 'X B, X^T Q')
        assert_same_bits(a, b, 'X B, X^T Q')
        Xs = t.X64
        kb.assert_elementwise(b[0], Xs @ B, 4.0 * (c.d + 2) * kb.U * (np.abs(Xs) @ np.abs(B)), 'X B', cols_are='column group of 64')
        kb.assert_elementwise(b[1], Xs.T @ Q, 4.0 * (c.n + 2) * kb.U * (np.abs(Xs).T @ np.abs(Q)), 'X^T Q',
                              rows_are='column tile of X', cols_are='column group of 64')
        for name, got, want in (('X B', b[0], Xs @ B), ('X^T Q', b[1], Xs.T @ Q)):
            for j in range(m):
                err = np.linalg.norm(got[:, j] - want[:, j]) / np.linalg.norm(want[:, j])
                assert err <= 1e-13, '%s: column %d relative error %.3g' % (name, j, err)


RF_CASES = [n for n in STEP_CASES if lc.CASES[n].c0]


@pytest.mark.parametrize('transpose', [False, True], ids=['A=X', 'A=Xt'])
@pytest.mark.parametrize('case', RF_CASES)
def test_range_finder(case, transpose):
    """rri_range_finder: Q orthonormal, B = Q^T A, the range of A (A^T A)^q Q0 -- the checks of test_nmf_gpu.py"""
    c = lc.CASES[case]
    m, n_iter = 8, 2
    with twins(case) as t:
        A = t.X64.T if transpose else t.X64
        Q0 = np.random.RandomState(5).randn(A.shape[1], m)
        a, b = both(t, lambda e: e.range_finder(Q0, n_iter, transpose=transpose))
        assert_finite(b, 'range finder')
        assert_same_bits(a, b, 'range finder')
        Qr, Br = b
        assert np.abs(Qr.T @ Qr - np.eye(m)).max() < 1e-12
        assert relfro(Br, Qr.T @ A) < 1e-12
        Y = A @ Q0
        for _ in range(n_iter):
            Y = A @ np.linalg.qr(A.T @ np.linalg.qr(Y)[0])[0]
        assert relfro(Qr @ (Qr.T @ Y), Y) < 1e-10


@pytest.mark.parametrize('case', [n for n in STEP_CASES if lc.CASES[n].store in DENSE])
def test_column_positive_counts_and_scale_X_refused(case):
    """df[j] = #{i: X[i, j] > 0}: exact integers.  The band holds NaN, and NaN > 0 is false: what shows a wrong stride here is
    the count of the zeros, so a third of the matrix is zero and the last row is not.  rri_scale_X rewrites X in place: on bound
    memory it is refused and nothing is written (the exit of twins() compares the allocation)."""
    c = lc.CASES[case]
    X = lc.case_matrix(c).astype(np.float64)
    X[np.random.RandomState(3).rand(c.n, c.d) < 0.33] = 0.0
    X[c.n - 1] = 1.0
    with twins(case, X=X) as t:
        a, b = both(t, lambda e: e.column_positive_counts())
        assert_same_bits(a, b, 'column_positive_counts')
        assert np.array_equal(b, (t.X64 > 0).sum(axis=0).astype(np.float64))
        with pytest.raises(ValueError, match='bound caller memory'):
            t.B.scale_X(np.full(c.d, 2.0), normalize_rows=True)
        with pytest.raises(ValueError, match='bound caller memory'):
            t.B.scale_X(None, normalize_rows=False)
        assert np.array_equal(t.B.column_positive_counts(), b)


@pytest.mark.parametrize('case', [n for n in STEP_CASES if lc.CASES[n].store == 'u8'])
def test_counts_are_rescaled_on_bound_memory(case):
    """What only a uint8 handle allows on bound memory: rri_scale_X and the preprocessing on top of it write the two scale
    vectors, no matrix.  column_positive_counts(), scale_X(col, False), scale_X(None, True) and preprocess(tfidf, normalize)
    succeed on the bound slice, each leaves every byte of the allocation as it was and the stored matrix equal to the uploaded
    twin's bit for bit, and the end is matrixops.normalize(matrixops.tfidf(C)) to 1e-14 (tests/test_count_storage_gpu.py)."""
    import torch
    from rri_nmf_amd.matrixops import tfidf, normalize
    c = lc.CASES[case]
    C = lc.case_matrix(c)
    C[np.random.RandomState(3).rand(c.n, c.d) < 0.33] = 0
    C[c.n - 1] = 1                                  # the last row, whose lower neighbour is the band, is in every count
    C[:, 5] = 0
    ones = (np.ones(c.n), np.ones(c.d))
    with twins(case, X=C, scales=ones) as t:
        stored = lambda e: e.X_times(np.eye(c.d))

        def settled(what):
            torch.cuda.synchronize()
            t.gx.check('the allocation X was bound in, after ' + what)
            a, b = both(t, stored)
            assert_same_bits(a, b, 'the stored matrix after ' + what)
            assert_same_bits(t.A.X_scales(), t.B.X_scales(), 'the scale vectors after ' + what)
            return b
        a, b = both(t, lambda e: e.column_positive_counts())
        assert_same_bits(a, b, 'column_positive_counts')
        assert np.array_equal(b, (C > 0).sum(axis=0).astype(np.float64))
        assert np.array_equal(settled('column_positive_counts'), C)
        col = 0.5 + np.random.RandomState(4).rand(c.d)
        both(t, lambda e: e.scale_X(col, False))
        assert np.array_equal(settled('scale_X(col, False)'), C * col)
        both(t, lambda e: e.scale_X(None, True))
        got = settled('scale_X(None, True)')
        assert relfro(got, normalize(C * col)) < 1e-14, relfro(got, normalize(C * col))
        for e in (t.A, t.B):
            e.set_X_scales(*ones)
        ia, ib = both(t, lambda e: e.preprocess(tfidf=True, normalize=True))
        Xt, idf = tfidf(C.astype(np.float64), return_idf=True)
        assert np.array_equal(ia, ib) and np.array_equal(ib, np.asarray(idf, dtype=np.float64).ravel())
        got = settled('preprocess(tfidf=True, normalize=True)')
        err = relfro(got, normalize(Xt))
        print('%s: preprocess on the bound slice against matrixops: relfro %.3e' % (case, err))
        assert err < 1e-14, err


@pytest.mark.parametrize('case', [n for n in STEP_CASES if lc.CASES[n].store in DENSE and lc.CASES[n].c0])
def test_bench_kernels_stay_inside_the_slice(case):
    """rri_bench_stream_copy and rri_bench_rank1_update copy X into a scratch buffer: from the first element of the slice to the
    end of its last row, ((n - 1) ld + d) elements, not n ld -- the ld - d elements behind the last row are not the handle's.
    Here they are band, so the check is status and band; the byte count is in rri_hip.hip (x_span_bytes)."""
    c = lc.CASES[case]
    with twins(case, bind_only=True) as t:
        W0, T0 = start(c, t.X64, K)
        t.B.set_W(W0); t.B.set_T(T0); t.B.set_params()
        assert t.B.bench_stream_copy(reps=2) >= 0.0
        assert t.B.bench_rank1_update(reps=2) >= 0.0
        # the handle goes on as before: the scratch copy was the only thing written
        t.B.sweep(1)
        assert_finite((t.B.get_W(), t.B.get_T()), 'a sweep after the bench calls')


STREAM_CASES = ['fp32-n203xd140-ld400-c4', 'fp64-n203xd142-ld272-c2', 'fp16-n203xd136-ld656-c8', 'fp32-n70xd1028-ld1032-c0',
                'u8-n203xd136-ld656-c8']


@pytest.mark.parametrize('case', STREAM_CASES)
def test_streaming_regime_by_a_fractional_capacity(monkeypatch, case):
    """RRI_PASS_CACHE_MB a fraction of one MB, the way tests/test_pass_keep_gpu.py sets it: room for one row block beside the
    chain, the others stream with non-temporal loads -- on a strided X.  A load policy changes no value: the same bits as the
    default capacity, and the oracle's factors."""
    import test_pass_keep_gpu as pk
    c = lc.CASES[case]
    monkeypatch.setenv('RRI_ONCHIP', '0')
    monkeypatch.delenv(pk.ENV, raising=False)
    with engine(c.n, c.d, K, dtype=c.dtype) as e:
        info = e.layout_info()
    xb, block, chain = pk.geometry(c.n, c.d, K, c.dtype, info)
    assert info['nrb'] >= 3, info
    cap = (chain + 1.5 * block) / 1e6
    assert cap < 1.0 and cap % 1.0 != 0.0 and cap * 1e6 < xb + chain
    res = {}
    for name, value in (('default', None), ('one row block kept', repr(cap)), ('nothing kept', '0')):
        if value is None:
            monkeypatch.delenv(pk.ENV, raising=False)
        else:
            monkeypatch.setenv(pk.ENV, value)
        with twins(case) as t:
            W0, T0 = start(c, t.X64, K)
            a, b = check_sweeps(t, W0, T0, 2, dict(), SWEEP_TOL, 'streaming: ' + name)
            res[name] = b
    monkeypatch.delenv(pk.ENV, raising=False)
    assert_same_bits(res['default'], res['one row block kept'], 'one row block kept against the default capacity')
    assert_same_bits(res['default'], res['nothing kept'], 'nothing kept against the default capacity')


# ---- RRI_UNWEIGHTED_RESIDUAL: X bound, the residual the handle's own ------------------------------------------------------------
RESIDUAL_CASES = [n for n in STEP_CASES if lc.CASES[n].store in DENSE]


def storage_ulp(dtype):
    return {np.float64: 2.0 ** -52, np.float32: 2.0 ** -23}[dtype]


@pytest.mark.parametrize('case', RESIDUAL_CASES)
def test_explicit_residual_rebuild_and_update(case):
    c = lc.CASES[case]
    rs = np.random.RandomState(c.n + c.d)
    with twins(case, kind='residual') as t:
        W0, T0 = start(c, t.X64, K)
        vec = [(rs.rand(c.n) - 0.3, rs.rand(c.d) - 0.3, rs.rand(c.d), rs.rand(c.n), a2, b2)
               for a2, b2 in ((None, None), (rs.rand(c.n) - 0.5, rs.rand(c.d) - 0.5))]

        def run(e):
            e.set_W(W0); e.set_T(T0); e.set_params()
            e.residual_rebuild()
            out = [e.get_residual()]
            for a_, b_, trow, wcol, a2, b2 in vec:
                out += list(e.residual_update(a_, b_, trow, wcol, a2=a2, b2=b2)) + [e.get_residual()]
            return out
        a, b = both(t, run)
        assert_finite(b, 'residual rebuild / update')
        assert_same_bits(a, b, 'residual rebuild / update')
        want = t.X64 - W0 @ T0
        bound = kb.resid_bound(t.X64, W0, T0)
        if c.dtype == np.float32:
            bound = bound + np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
        kb.assert_elementwise(b[0].astype(np.float64), want, bound, 'R = X - W T after rri_residual_rebuild')
        ulp = storage_ulp(c.dtype)
        Rb = b[0].astype(np.float64)
        for i, (a_, b_, trow, wcol, a2, b2) in enumerate(vec):
            y, z, R1 = b[1 + 3 * i], b[2 + 3 * i], b[3 + 3 * i].astype(np.float64)
            want = Rb - np.outer(a_, b_) - (np.outer(a2, b2) if a2 is not None else 0.0)
            assert np.abs(R1 - want).max() <= ulp * max(np.abs(want).max(), 1.0) * 1.01, (i, np.abs(R1 - want).max())
            assert relfro(R1, want) < 2 * ulp, (i, relfro(R1, want))
            assert relfro(y, R1 @ trow) < 1e-13 and relfro(z, R1.T @ wcol) < 1e-13, (relfro(y, R1 @ trow), relfro(z, R1.T @ wcol))
            Rb = R1


@pytest.mark.parametrize('flags', list(FLAGS))
@pytest.mark.parametrize('case', RESIDUAL_CASES)
def test_two_sweeps_on_the_explicit_residual(case, flags):
    c = lc.CASES[case]
    tol = SWEEP_TOL if c.dtype == np.float64 else STORED_FP32_TOL
    with twins(case, kind='residual') as t:
        W0, T0 = start(c, t.X64, K, FLAGS[flags])
        check_sweeps(t, W0, T0, 2, FLAGS[flags], tol, 'explicit residual, two sweeps, ' + flags)
        a, b = both(t, lambda e: e.get_residual())
        assert_finite(b, 'the stored residual')
        assert_same_bits(a, b, 'the stored residual')


# ---- RRI_WEIGHTED_DENSE: X and the mask bound, each in its own allocation, different strides ------------------------------------
def mask_of(kind, c):
    rs = np.random.RandomState(c.n + c.d)
    if kind == 'fractional':
        return 0.25 + rs.rand(c.n, c.d)
    M = (rs.rand(c.n, c.d) < (0.06 if kind == 'sparse01' else 0.5)).astype(np.float64)
    M[0, :] = 1.0            # no column without an observation
    M[:, 0] = 1.0
    return M


MASKS = ['sparse01', 'half01', 'fractional']
WEIGHTED_CASES = [n for n in STEP_CASES if lc.CASES[n].store in DENSE]
WFLAGS = dict(t_row_sum=1.0, reset_topic_method=None)


def weighted_problem(case, mask):
    c = lc.CASES[case]
    M = mask_of(mask, c).astype(c.dtype).astype(np.float64)
    X = lc.case_matrix(c).astype(np.float64) * (M > 0)
    return c, X, M


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('case', WEIGHTED_CASES)
def test_weighted_two_sweeps(case, mask):
    """0/1 masks are bit-packed at the bind (k_mask_nonbinary and k_mask_pack read the mask with ldm: a packer that scanned the
    band would call the mask non-binary); below 12 % set the first topic step makes the column-major bit copy and takes
    k_wmcorr_cols, at 50 % the dense-bit kernels.  A fractional mask stays bound and every pass reads it with ldm."""
    c, X, M = weighted_problem(case, mask)
    tol = SWEEP_TOL if c.dtype == np.float64 else STORED_FP32_TOL
    with twins(case, kind='weighted', X=X, M=M) as t:
        W0, T0 = start(c, t.X64, K)
        for e in (t.A, t.B):
            assert e.layout_info()['mask_bits'] is (mask != 'fractional'), (mask, e.layout_info())
        check_sweeps(t, W0, T0, 2, WFLAGS, tol, 'weighted, two sweeps, ' + mask, M=M)
        for e in (t.A, t.B):
            info = e.layout_info()
            assert info['mask_cols'] is (mask == 'sparse01'), (mask, info)
            if mask != 'fractional':
                assert abs(info['mask_density'] - M.mean()) < 1e-8, (info, M.mean())


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('case', WEIGHTED_CASES)
def test_weighted_single_operations(case, mask):
    """objective, resid_row_argmax / reset_row, X_times / Xt_times on a weighted handle.  The reset search of the reference takes
    max(X - W T, 0) without the mask (nmf.py:770-773)."""
    c, X, M = weighted_problem(case, mask)
    star = c.n - 1
    X[star] += 2.0 * X.max()
    rs = np.random.RandomState(9)
    B, Q = rs.randn(c.d, 17), rs.randn(c.n, 3)
    with twins(case, kind='weighted', X=X, M=M) as t:
        W0, T0 = start(c, t.X64, K)
        rows = sorted({star, 0, 64})

        def run(e):
            e.set_W(W0); e.set_T(T0); e.set_params(**WFLAGS)
            val, row = e.resid_row_argmax()
            return [e.objective(), e.objective_parts(), val, np.int64(row), e.X_times(B), e.Xt_times(Q)] + [e.reset_row(i) for i in rows]
        a, b = both(t, run)
        assert_finite(b, 'weighted single operations')
        assert_same_bits(a, b, 'weighted single operations')
        Xs = t.X64
        want = oracle().true_objective(Xs, W0, T0, Wm=M)
        kb.assert_rel(b[0], want, 1e-12, 'weighted objective, ' + mask)
        kb.assert_rel(b[1][0], want, 1e-12, 'weighted objective_parts[0], ' + mask)
        kb.assert_rel(b[1][1], float((W0 ** 2).sum()), 1e-12, 'weighted objective_parts[1]')
        R = Xs - W0 @ T0
        pos = (np.maximum(R, 0.0) ** 2).sum(axis=1)
        assert np.argmax(pos) == star and np.sort(pos)[-2] < 0.5 * pos[star]
        assert int(b[3]) == star
        kb.assert_rel(b[2], pos[star], 1e-12, 'sum_j max(X - W T, 0)^2 of row %d' % star)
        kb.assert_elementwise(b[4], Xs @ B, 4.0 * (c.d + 2) * kb.U * (np.abs(Xs) @ np.abs(B)), 'X B', cols_are='column group of 64')
        kb.assert_elementwise(b[5], Xs.T @ Q, 4.0 * (c.n + 2) * kb.U * (np.abs(Xs).T @ np.abs(Q)), 'X^T Q',
                              rows_are='column tile of X', cols_are='column group of 64')
        bound = kb.resid_bound(Xs, W0, T0)
        for i, got in zip(rows, b[6:]):
            kb.assert_elementwise(got[None, :], np.maximum(R[i], 0.0)[None, :], bound[i][None, :], 'reset row %d' % i)


# ---- two ranks, each bound to its row block of ONE guarded allocation -----------------------------------------------------------
class ThreadTransport(object):
    """the three collectives of rri_comm_create_host between the threads of one process (one thread per rank): every call
    deposits, waits at a barrier, reads.  A rank that fails breaks the barrier, so its peer returns an error instead of waiting."""

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world, timeout=60)
        self.slots = [None] * world

    def _exchange(self, rank, value):
        self.slots[rank] = value
        self.barrier.wait()
        out = list(self.slots)
        self.barrier.wait()
        return out

    def group(self, rank, sizes):
        import ctypes as C
        from rri_nmf_amd import _capi
        from rri_nmf_amd.distributed import RowGroup
        arr = lambda ptr, count: np.ctypeslib.as_array(ptr, shape=(int(count),))

        def guard(fn):
            def call(*args):
                try:
                    fn(*args)
                    return 0
                except Exception:  # noqa: BLE001  (a non-zero return becomes RRI_ERR_COMM)
                    self.barrier.abort()
                    return 1
            return call

        def allreduce(user, buf, count):
            parts = self._exchange(rank, arr(buf, count).copy())
            arr(buf, count)[:] = np.sum(parts, axis=0)      # rank order on every rank: the same bits everywhere

        def allgather(user, send, count, recv):
            arr(recv, count * self.world)[:] = np.concatenate(self._exchange(rank, arr(send, count).copy()))

        def broadcast(user, buf, count, root):
            arr(buf, count)[:] = self._exchange(rank, arr(buf, count).copy())[root]

        cbs = (_capi.ALLREDUCE_FN(guard(allreduce)), _capi.ALLGATHER_FN(guard(allgather)), _capi.BROADCAST_FN(guard(broadcast)))
        comm = C.c_void_p()
        st = _capi.load_library().rri_comm_create_host(C.byref(comm), rank, self.world, cbs[0], cbs[1], cbs[2], None)
        assert st == _capi.RRI_OK, st
        return RowGroup(comm, rank, self.world, sizes, keep=cbs)


SHARD_CASES = {'plain-fp32': ('fp32-n203xd140-ld400-c4', 'plain', dict()),
               'topic-fp64': ('fp64-n203xd142-ld144-c0', 'plain', TOPIC),
               'weighted-fp64': ('fp64-n203xd142-ld272-c2', 'weighted', WFLAGS)}


@pytest.mark.parametrize('name', list(SHARD_CASES))
def test_two_ranks_bound_to_row_blocks_of_one_allocation(name):
    """Host transport, both ranks on the one GPU, one thread per rank.  Rank 0 holds rows 0 .. 99, rank 1 rows 100 .. 202 of the
    SAME guarded slice: what lies below rank 0's last row is rank 1's data, finite and wrong, not NaN -- a rank that read past
    its rows would not show as NaN but against the unsharded handle (tolerance of tests/test_sharded_gpu.py)."""
    import torch
    case, kind, flags = SHARD_CASES[name]
    c = lc.CASES[case]
    M = None
    X = lc.case_matrix(c).astype(np.float64)
    if kind == 'weighted':
        _, X, M = weighted_problem(case, 'half01')
    X = np.ascontiguousarray(X.astype(c.dtype))
    X64 = X.astype(np.float64)
    W0, T0 = start(c, X64, K, flags)
    sizes = [100, c.n - 100]
    gx = lc.guarded(torch, X, c.ld, c.c0, device='cuda:0')
    gm = None
    if M is not None:
        gm = lc.guarded(torch, M.astype(c.dtype), *other_stride(c), device='cuda:0')
    torch.cuda.synchronize()
    transport = ThreadTransport(2)
    out, errors = [None, None], []

    def rank_main(rank):
        grp = e = None
        try:
            grp = transport.group(rank, sizes)
            lo, hi = grp.row_lo, grp.row_lo + grp.n_local
            e = engine(hi - lo, c.d, K, dtype=c.dtype, weighted=kind == 'weighted')
            e.bind_X_device(*gx.rows(lo, hi))
            if gm is not None:
                e.bind_mask_device(*gm.rows(lo, hi))
            assert lc.G >= e.layout_info()['rpb'], 'the guard rows must cover a row block of this rank: %r' % (e.layout_info(),)
            e.set_W(W0[lo:hi]); e.set_T(T0); e.set_params(**flags)
            e.attach_group(grp)
            e.sweep(2)
            out[rank] = e.get_W(), e.get_T(), e.objective(), e.n_resets_used
        except BaseException as err:  # noqa: BLE001  (reported by the test; the peer must not wait)
            transport.barrier.abort()
            errors.append((rank, repr(err)))
        finally:
            if e is not None:
                e.close()
            if grp is not None:
                grp.close()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    with engine(c.n, c.d, K, dtype=c.dtype, weighted=kind == 'weighted') as e:
        e.upload_X(X)
        if M is not None:
            e.upload_mask(M.astype(c.dtype))
        want = run_sweeps(e, W0, T0, 2, flags)
    torch.cuda.synchronize()
    gx.check('the allocation both ranks bound their rows of X in')
    if gm is not None:
        gm.check('the allocation both ranks bound their rows of the mask in')
    W = np.vstack([out[0][0], out[1][0]])
    assert_finite((W, out[0][1], out[1][1], out[0][2]), 'two ranks')
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]            # replicated, bit for bit
    tol = 1e-10                          # tests/test_sharded_gpu.py: float64 storage, or no stored fp32 residual
    ew, et = relfro(W, want[0]), relfro(out[0][1], want[1])
    print('%s: two ranks against one handle: W %.3e T %.3e' % (name, ew, et))
    assert ew < tol and et < tol, (ew, et)
    assert abs(out[0][2] - want[2]) <= tol * abs(want[2]) and out[0][3] == out[1][3] == want[3]


# ---- rebinding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,pair', [('plain', ('fp32-n203xd140-ld144-c0', 'fp32-n203xd140-ld400-c4')),
                                      ('plain', ('fp64-n203xd142-ld272-c2', 'fp64-n203xd142-ld144-c0')),
                                      ('plain', ('fp16-n203xd136-ld144-c0', 'fp16-n203xd136-ld656-c8')),
                                      ('residual', ('fp32-n203xd140-ld400-c4', 'fp32-n203xd140-ld144-c0')),
                                      ('plain', ('u8-n203xd136-ld144-c0', 'u8-n203xd136-ld656-c8'))],
                         ids=['fp32', 'fp64', 'fp16', 'residual-fp32', 'u8'])
def test_rebinding_leaves_no_stale_stride(monkeypatch, kind, pair):
    """bind slice 1, sweep, bind slice 2 -- another matrix in another allocation with another ld --, sweep: the same bits as a
    fresh handle bound to slice 2 that took the same steps on the launch-per-phase schedule (changed(c, CH_X) drops whatever
    was derived from the first X or its stride).  uint8: each bind is followed by its own scales; the second bind must have put
    the first ones back to ones before.
    """
    import torch
    monkeypatch.setenv('RRI_ONCHIP', '0')
    c1, c2 = lc.CASES[pair[0]], lc.CASES[pair[1]]
    assert (c1.n, c1.d) == (c2.n, c2.d) and c1.ld != c2.ld
    X1, X2 = lc.case_matrix(c1, seed=1), lc.case_matrix(c2, seed=2)
    g1 = lc.guarded(torch, X1, c1.ld, c1.c0, device='cuda:0')
    g2 = lc.guarded(torch, X2, c2.ld, c2.c0, device='cuda:0')
    torch.cuda.synchronize()
    X64 = X2.astype(np.float64)
    u8 = c2.store == 'u8'
    if u8:
        sc1, sc2 = lc.case_scales(c1, seed=1), lc.case_scales(c2, seed=2)
        X64 = lc.scaled(X2, *sc2)
    W0, T0 = start(c2, X64, K)
    kw = dict(dtype=c2.dtype, **(dict(schedule='residual') if kind == 'residual' else {}))

    def steps(e):
        """what both handles do once slice 2 is bound"""
        e.bind_X_device(g2.ptr, g2.ld)
        assert lc.G >= e.layout_info()['rpb'], 'the guard rows must cover a row block of the pass: %r' % (e.layout_info(),)
        if u8:
            assert np.array_equal(e.X_scales()[0], np.ones(c2.n)) and np.array_equal(e.X_scales()[1], np.ones(c2.d))
            e.set_X_scales(*sc2)
        e.set_W(W0); e.set_T(T0)
        e.sweep(1)
        out = [e.get_W(), e.get_T(), e.objective()]
        e.update_T_row(1)
        return out + [e.get_T(), e.X_times(np.ones((c2.d, 2)))]

    with engine(c1.n, c1.d, K, **kw) as e:
        e.bind_X_device(g1.ptr, g1.ld)
        assert lc.G >= e.layout_info()['rpb']
        if u8:
            e.set_X_scales(*sc1)
        e.set_W(W0); e.set_T(T0); e.set_params(reset_topic_method=None)
        e.sweep(1)
        e.objective()
        got = steps(e)
    with engine(c2.n, c2.d, K, **kw) as e:
        e.set_params(reset_topic_method=None)
        want = steps(e)
    torch.cuda.synchronize()
    g1.check('the first allocation')
    g2.check('the second allocation')
    assert_finite(got, 'after the rebind')
    assert_same_bits(want, got, 'a rebound handle against a fresh one')
    ref = oracle().nmf(X64, K, W_in=W0.copy(), T_in=T0.copy(), max_iter=1, eps_stop=-1, reset_topic_method=None, do_final_project_W=False)
    tol = STORED_FP32_TOL if kind == 'residual' else SWEEP_TOL
    assert relfro(got[0], ref['W']) < tol and relfro(got[1], ref['T']) < tol, (relfro(got[0], ref['W']), relfro(got[1], ref['T']))
    if kind == 'plain':
        # the objective of the factors the sweep left, assembled from its cross terms: the bound of test_hip_parity.py
        want_obj = oracle().true_objective(X64, got[0], got[1])
        assert abs(got[2] - want_obj) <= 1e-11 * max(want_obj, 1e-3 * float((X64 ** 2).sum())), (got[2], want_obj)
