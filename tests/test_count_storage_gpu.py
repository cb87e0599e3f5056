"""uint8 count storage of a read-only dense X (RRI_U8, nmf(..., dtype=np.uint8)) on the GPU.

A uint8 handle stores counts C (0..255, one byte each) and two float64 vectors, and every kernel sees
X[i, j] = (C[i, j] * cscale[j]) * rscale[i] in float64.  Nothing is rounded at upload, so the handle must compute what the
float64 reference computes on that matrix.  Bounds:

    TOL = 2e-9    "same algorithm, other summation order" (tests/test_hip_parity.py): whole runs against the oracle on the X64
                  built from the handle's own scale vectors
    1e-8          the project's bound for a device-preprocessed X against host preprocessing (tests/test_preprocess_gpu.py):
                  whole runs against the oracle on matrixops.normalize(matrixops.tfidf(C))

(the oracle alone moves by at most 2e-11 on such inputs when X is formed in the factored order with the row totals summed in
another order).  Single steps are checked with the bounds and helpers of tests/test_kernel_buckets_gpu.py.

Geometry that was kept: 8-byte loads, 8 counts per lane, so a workgroup of the pass spans SPAN = 2048 columns, rows are padded to
VN = 8 bytes, and a bound array needs a row stride that is a multiple of 8."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, load_golden, relfro
from rri_nmf_amd.synthetic import planted_X, scaled_init
from test_hip_parity import run_oracle
from test_kernel_buckets_gpu import (U, FLAGS, assert_elementwise, assert_rel, check_steps, resid_bound, resid_bucket, xtt_bucket)

pytestmark = pytest.mark.gpu

U8 = np.uint8
TOL = 2e-9
TM = dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
VN = 8
SPAN = 4 * 64 * VN


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def oracle():
    from oracle import rri_oracle
    return rri_oracle


def stored_matrix(e):
    """the X the handle factorises, element by element: a product with the identity adds only zeros"""
    return e.X_times(np.eye(e.d))


def some_counts(n, d, seed):
    rs = np.random.RandomState(seed)
    C = rs.randint(0, 256, size=(n, d))
    C.flat[::5] = 0
    C.flat[::7] = 255
    C[-1, -1] = 201                                   # the last element of the last panel
    return C


def scales(n, d, seed):
    """log-uniform over 1e-3 .. 1e3; one column scale exactly 0, one negative and tiny (the idf of a term in every document)"""
    rs = np.random.RandomState(seed)
    r, s = 10.0 ** rs.uniform(-3, 3, n), 10.0 ** rs.uniform(-3, 3, d)
    s[d // 2] = 0.0
    s[d // 3] = -2.220446049250313e-16
    return r, s


def x64(C, r, s):
    return np.ascontiguousarray((np.asarray(C, dtype=np.float64) * s) * r[:, None])


# ---- 1. what is stored ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [7, 16, 17, 300, SPAN - 1, SPAN, SPAN + 1])
@pytest.mark.parametrize('n', [1, 63, 65, 1000])
def test_stored_matrix_equals_the_counts(n, d):
    C = some_counts(n, d, n + d)
    with engine(n, d, 2, dtype=U8) as e:
        assert e.layout_info()['npanels'] == -(-(-(-d // VN) * VN) // SPAN)
        for src in (np.float64, np.float32, U8):
            e.upload_X(np.ascontiguousarray(C.astype(src)))
            got = stored_matrix(e)
            bad = got != C
            assert not bad.any(), ('host %s: %d elements differ, first at %s: stored %r, given %r' % (
                np.dtype(src).name, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], C[bad][0]))
            assert e.storage_relerr == 0.0
            r, s = e.X_scales()
            assert np.array_equal(r, np.ones(n)) and np.array_equal(s, np.ones(d))


# ---- 2. refused at upload ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [256.0, -1.0, 0.5, np.nan, np.inf])
@pytest.mark.parametrize('src', [np.float64, np.float32])
def test_values_that_are_no_counts_are_refused_at_upload(bad, src):
    C = some_counts(70, 24, 0)
    W0, T0 = scaled_init(C.astype(np.float64), 3, seed=1)
    with engine(70, 24, 3, dtype=U8) as e:
        e.upload_X(C); e.set_W(W0); e.set_T(T0); e.set_params()
        e.sweep(1)                                          # a good X first: the refusal must take it away
        Xb = C.astype(src)
        Xb[69, 23] = bad
        with pytest.raises(ValueError, match='integer in 0..255'):
            e.upload_X(Xb)
        with pytest.raises(ValueError, match='X, W, T and params must be set'):
            e.sweep(1)
        e.upload_X(C)                                       # ... and the handle takes a good one again
        e.sweep(1)


# ---- 3. scales -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, d', [(65, 17), (203, 300), (33, SPAN + 1)])
def test_scales_enter_every_element_in_float64(n, d):
    C = some_counts(n, d, 3)
    C[:, 5] = 0                                          # one column of zeros
    r, s = scales(n, d, 4)
    want = x64(C, r, s)
    with engine(n, d, 2, dtype=U8) as e:
        e.upload_X(C.astype(U8))
        e.set_X_scales(r, s)
        got = stored_matrix(e)
        assert_elementwise(got, want, 1e-15 * np.abs(want), 'stored (C * s) * r')
        gr, gs = e.X_scales()
        assert np.array_equal(gr, r) and np.array_equal(gs, s)
        e.set_X_scales(None, 2.0 * s)                       # one vector at a time
        gr, gs = e.X_scales()
        assert np.array_equal(gr, r) and np.array_equal(gs, 2.0 * s)
        e.set_X_scales(r / 2.0, None)
        assert np.array_equal(stored_matrix(e), x64(C, r / 2.0, 2.0 * s))
        df = e.column_positive_counts()                     # the counts, whatever the scales are
        assert np.array_equal(df, (C > 0).sum(0))
        e.upload_X(C.astype(U8))                            # a new X: both vectors are ones again
        gr, gs = e.X_scales()
        assert np.array_equal(gr, np.ones(n)) and np.array_equal(gs, np.ones(d))
        assert np.array_equal(stored_matrix(e), C)
    with engine(n, d, 2, dtype=np.float32) as e:            # no other store has scale vectors
        e.upload_X(C.astype(np.float64))
        with pytest.raises(ValueError, match='RRI_U8'):
            e.set_X_scales(r, s)
        with pytest.raises(ValueError, match='RRI_U8'):
            e.X_scales()


# ---- 4. single steps against the oracle on X64 ------------------------------------------------------------------------------
def count_problem(n, d, k, seed):
    """planted counts 0..255 with a zero column, wild scales, and a random start scaled to X64"""
    P = planted_X(n, d, min(k, 8) + 1, seed=seed + k, dtype=np.float64)
    C = np.minimum(np.round(40.0 * P / P.mean()), 255.0).astype(U8)
    C[:, d // 4] = 0
    r, s = scales(n, d, seed + 1)
    X = x64(C, r, s)
    W0, T0 = scaled_init(np.abs(X), k, seed=seed + k + 1)
    return C, r, s, X, W0, T0


def near_count_solution(n, d, k, seed):
    """counts close to a rank-k product, mild scales, and a start within 0.1 % of the factors: whole sweeps from here keep every
    row of T and column of W alive at any k (tests/test_kernel_buckets_gpu.py near_solution)"""
    rs = np.random.RandomState(seed)
    Ws, Ts = rs.rand(n, k), rs.rand(k, d)
    P = Ws @ Ts
    a = 200.0 / P.max()
    C = np.round(a * P).astype(U8)
    r, s = 10.0 ** rs.uniform(-1, 1, n), 10.0 ** rs.uniform(-1, 1, d)
    X = x64(C, r, s)
    return C, r, s, X, (a * r[:, None]) * Ws * (1 + 1e-3 * rs.rand(n, k)), (Ts * s) * (1 + 1e-3 * rs.rand(k, d))


def loaded(e, C, r, s, W0, T0, **params):
    e.upload_X(C); e.set_X_scales(r, s); e.set_W(W0); e.set_T(T0); e.set_params(**params)


STEP_RANKS = [1, 2, 16, 17, 33, 49, 53, 64, 65, 257]


@pytest.mark.parametrize('flags', list(FLAGS))
@pytest.mark.parametrize('k', STEP_RANKS, ids=[resid_bucket(k) for k in STEP_RANKS])
def test_objective_and_topic_steps_in_every_rank_bucket(k, flags):
    """k_resid_mfma with KS = 4 / 8 / 12 / 13 / 16 and k_resid with the W tile and the W slice (the objective right after
    set_W / set_T, the max-residual row, the reset row), then single T-row and W-column steps through the pass"""
    orc = oracle()
    n, d = 203, 141
    C, r, s, X, W0, T0 = count_problem(n, d, k, seed=7)
    with engine(n, d, k, dtype=U8) as e:
        loaded(e, C, r, s, W0, T0, **FLAGS[flags])
        assert not e.onchip_info()[0]
        assert_rel(e.objective(), orc.true_objective(X, W0, T0), 1e-12, 'objective right after set_W / set_T')
        R = X - W0 @ T0
        pos = (np.maximum(R, 0.0) ** 2).sum(axis=1)
        val, row = e.resid_row_argmax()
        assert row == int(np.argmax(pos))
        assert_rel(val, pos.max(), 1e-12, 'sum_j max(X - W T, 0)^2 of the max-residual row')
        bound = resid_bound(X, W0, T0)
        for i in sorted({row, 0, n - 1, 70}):
            assert_elementwise(e.reset_row(i)[None, :], np.maximum(R[i], 0.0)[None, :], bound[i][None, :], 'reset row %d' % i)
        for t in sorted({0, k - 1}):
            wR, nw = e.topic_sums(t)
            want_wR, want_nw = orc.residual_products_T(X, W0.copy(), T0, t)
            assert_elementwise(wR[None, :], want_wR[None, :], 1e-12 * np.abs(want_wR).max(), 'wR of topic %d' % t)
            assert_rel(nw, float(want_nw), 1e-13, '||w_t||^2 of topic %d' % t)
        check_steps(e, X, k, FLAGS[flags])
        W, T = e.get_W(), e.get_T()
        assert_rel(e.objective(), orc.true_objective(X, W, T), 1e-12, 'objective after the steps')


# Rows: small n get row blocks of 32 (rri_create: at least 32 rows per block), so n = 31, 32, 33 are one ragged block, one full
# block, and two blocks with one row in the second.  Columns: one load below, at and above the span of one workgroup.
@pytest.mark.parametrize('d', [SPAN - VN, SPAN - 1, SPAN, SPAN + 1])
@pytest.mark.parametrize('n', [31, 32, 33, 65])
def test_single_steps_at_the_geometry_edges(n, d):
    orc = oracle()
    for k, flags in ((2, 'topic'), (50, 'plain')):
        C, r, s, X, W0, T0 = count_problem(n, d, k, seed=n + d)
        with engine(n, d, k, dtype=U8) as e:
            info = e.layout_info()
            assert info['npanels'] == -(-(-(-d // VN) * VN) // SPAN), info
            assert info['rpb'] == 32 and info['nrb'] == -(-n // 32), info
            loaded(e, C, r, s, W0, T0, **FLAGS[flags])
            assert_rel(e.objective(), orc.true_objective(X, W0, T0), 1e-12, 'objective right after set_W / set_T')
            check_steps(e, X, k, FLAGS[flags])
            W, T = e.get_W(), e.get_T()
            assert_rel(e.objective(), orc.true_objective(X, W, T), 1e-12, 'objective after the steps')


# Row blocks that are not the 32-row minimum.  rri_create takes ceil(n / (total / npanels)) rows with total = 1024 if that gives
# 192 rows or more and with total = 512 otherwise, then max(., 32), rounded up to 16:
#   6011 x 4099: LD 4104, 3 panels, 512 / 3 = 170 blocks, ceil(6011 / 170) = 36 -> 48 rows, 126 blocks, the last of 11 rows
#   8209 x 6150: LD 6152, 4 panels, 512 / 4 = 128 blocks, ceil(8209 / 128) = 65 -> 80 rows, 103 blocks, the last of 49 rows
#                (six interleaved chunks of 8 rows and one row)
# 378 and 412 workgroups: interleaved chunks.
BLOCK_SHAPES = {'6011x4099-48rows': (6011, 4099, 3, 48, 126, 11), '8209x6150-80rows': (8209, 6150, 4, 80, 103, 49)}


@pytest.mark.parametrize('shape', list(BLOCK_SHAPES))
def test_single_steps_with_row_blocks_above_the_minimum(shape):
    """several panels times a hundred row blocks of 48 and 80 rows with a ragged last block: the objective right after
    set_W / set_T, the max-residual row and the reset row of the last row, and single topic steps, against the oracle on X64"""
    orc = oracle()
    n, d, npanels, rpb, nrb, last = BLOCK_SHAPES[shape]
    for k, flags in ((2, 'topic'), (50, 'plain')):
        C, r, s, X, W0, T0 = count_problem(n, d, k, seed=n + d)
        with engine(n, d, k, dtype=U8) as e:
            info = e.layout_info()
            assert (info['npanels'], info['rpb'], info['nrb']) == (npanels, rpb, nrb) and n - (nrb - 1) * rpb == last, info
            assert info['interleaved'] and npanels * nrb <= 1024, info
            loaded(e, C, r, s, W0, T0, **FLAGS[flags])
            got, want = e.objective(), orc.true_objective(X, W0, T0)
            print('%s k=%d %s: objective after set factors, relative error %.3e' % (shape, k, flags, abs(got - want) / abs(want)))
            assert_rel(got, want, 1e-12, 'objective right after set_W / set_T')
            R = X - W0 @ T0
            pos = (np.maximum(R, 0.0) ** 2).sum(axis=1)
            val, row = e.resid_row_argmax()
            assert row == int(np.argmax(pos)), (row, int(np.argmax(pos)))
            print('%s k=%d %s: max-residual row %d (row block %d), relative error %.3e' % (
                shape, k, flags, row, row // rpb, abs(val - pos.max()) / pos.max()))
            assert_rel(val, pos.max(), 1e-12, 'sum_j max(X - W T, 0)^2 of the max-residual row')
            i = n - 1
            assert_elementwise(e.reset_row(i)[None, :], np.maximum(R[i], 0.0)[None, :], resid_bound(X[i:], W0[i:], T0),
                               'reset row %d (the last row of the ragged block)' % i)
            del R
            check_steps(e, X, k, FLAGS[flags])
            W, T = e.get_W(), e.get_T()
            got, want = e.objective(), orc.true_objective(X, W, T)
            print('%s k=%d %s: objective after the steps, relative error %.3e' % (shape, k, flags, abs(got - want) / abs(want)))
            assert_rel(got, want, 1e-12, 'objective after the steps')


XT_M = [1, 16, 17, 33, 49, 64, 65, 129]
XTQ_M = [1, 8, 9, 17]


@pytest.mark.parametrize('n, d', [(203, 141), (33, SPAN + 1)])
def test_products_with_the_resident_X(n, d):
    """rri_X_times: k_xtt_mfma<NT> for every NT and the chunk loop; rri_Xt_times: colsums8 in groups of 8 vectors, also with more
    than 8; the range finder on top of both"""
    C, r, s, X, _, _ = count_problem(n, d, 3, seed=11)
    rs = np.random.RandomState(n)
    with engine(n, d, 3, dtype=U8) as e:
        e.upload_X(C); e.set_X_scales(r, s)
        for m in XT_M:
            B = rs.randn(d, m)
            got, want = e.X_times(B), X @ B
            for j in range(m):
                err = np.linalg.norm(got[:, j] - want[:, j]) / np.linalg.norm(want[:, j])
                assert err <= 1e-13, ('X B', xtt_bucket(m), j, err)
            assert_elementwise(got, want, 4.0 * (d + 2) * U * (np.abs(X) @ np.abs(B)), 'X B, ' + xtt_bucket(m))
        for m in XTQ_M:
            Q = rs.randn(n, m)
            got, want = e.Xt_times(Q), X.T @ Q
            for j in range(m):
                err = np.linalg.norm(got[:, j] - want[:, j]) / np.linalg.norm(want[:, j])
                assert err <= 1e-13, ('X^T Q', m, j, err)
            assert_elementwise(got, want, 4.0 * (n + 2) * U * (np.abs(X).T @ np.abs(Q)), 'X^T Q, m = %d' % m,
                               rows_are='column tile of X')
        Q0 = rs.randn(d, 5)
        Q, B = e.range_finder(Q0, 2)
        assert np.allclose(Q.T @ Q, np.eye(5), atol=1e-10)
        assert relfro(Q @ (Q.T @ X), X) < 1.0 and relfro(B, Q.T @ X) < 1e-9


FIXED_K = [2, 17, 33, 64, 65, 109, 110]


@pytest.mark.parametrize('k', FIXED_K)
def test_sweeps_with_one_factor_fixed(k):
    """T fixed: the whole-sweep W half on Qt = X T^T (k_xtt_mfma in every NT bucket, the chunk loop above 64, one launch per
    sweep up to k = 109 and a launch per topic above); W fixed: the T half through the column sums of the pass.  The objective
    after a sweep is assembled from ||X||^2 (k_sqsum) and the cross terms the pass left."""
    n, d, sweeps = 203, 141, 3
    C, r, s, X, W0, T0 = near_count_solution(n, d, k, seed=k)
    with engine(n, d, k, dtype=U8) as e:
        loaded(e, C, r, s, W0, T0, fix_T=True, reset_topic_method=None)
        e.timing_enable(True)
        e.sweep(sweeps)
        launches = e.timing_read(1)[0]
        W, T = e.get_W(), e.get_T()
        obj = e.objective()
    assert launches == sweeps if k <= 109 else launches >= sweeps * k, launches
    ref = oracle().nmf(X, k, W_in=W0.copy(), T_in=T0.copy(), max_iter=sweeps, eps_stop=-1, fix_T=True, reset_topic_method=None)
    assert relfro(W, ref['W']) < TOL and np.array_equal(T, T0), relfro(W, ref['W'])
    want = oracle().true_objective(X, W, T)
    assert abs(obj - want) <= 1e-12 * 0.5 * float((X ** 2).sum()) * k, ('objective with T fixed', obj, want)
    # W fixed, topic-model flags (in the plain flavour the kept column takes the 1-norm of its new T row, nmf.py:450-452, and from
    # this start the reference itself ends in "unbounded" at k >= 17): the start is prepared as the oracle prepares it
    T0p = oracle().proj_rows_simplex(np.maximum(T0, 0).copy(), 1.0)
    with engine(n, d, k, dtype=U8) as e:
        loaded(e, C, r, s, W0, T0p, fix_W=True, reset_topic_method=None, **TM)
        e.sweep(sweeps)
        W, T = e.get_W(), e.get_T()
    ref = oracle().nmf(X, k, W_in=W0.copy(), T_in=T0.copy(), max_iter=sweeps, eps_stop=-1, fix_W=True, reset_topic_method=None, **TM)
    assert relfro(T, ref['T']) < TOL and relfro(W, ref['W']) < TOL, (relfro(T, ref['T']), relfro(W, ref['W']))
    with engine(n, d, k, dtype=U8) as e:                    # both halves free: ||X||^2 and the cross terms of a whole sweep
        loaded(e, C, r, s, W0, T0, reset_topic_method=None)
        e.sweep(1)
        W, T = e.get_W(), e.get_T()
        obj = e.objective()
    want = oracle().true_objective(X, W, T)
    assert abs(obj - want) <= 1e-12 * 0.5 * float((X ** 2).sum()) * k, ('assembled objective after a sweep', obj, want)


def test_changing_a_scale_drops_what_the_handle_computed_from_X():
    """a scale is a part of X: ||X||^2 and the cross terms of a sweep (the assembled objective) and Qt = X T^T of a run with T
    fixed must not outlive rri_set_X_scales or rri_scale_X"""
    orc = oracle()
    n, d, k = 203, 141, 5
    C, r, s, X, W0, T0 = near_count_solution(n, d, k, seed=21)
    with engine(n, d, k, dtype=U8) as e:
        loaded(e, C, r, s, W0, T0, reset_topic_method=None)
        e.sweep(1)
        W, T = e.get_W(), e.get_T()
        assert abs(e.objective() - orc.true_objective(X, W, T)) <= 1e-12 * 0.5 * float((X ** 2).sum()) * k
        r2, s2 = 1.5 * r, s * np.linspace(0.5, 2.0, d)
        e.set_X_scales(r2, s2)
        assert_rel(e.objective(), orc.true_objective(x64(C, r2, s2), W, T), 1e-12, 'objective after set_X_scales')
        e.set_params(fix_T=True, reset_topic_method=None)
        e.sweep(1)                                          # Qt of (C, r2, s2) is on the handle now
        for change, Xnew in ((lambda: e.set_X_scales(r, None), x64(C, r, s2)),
                             (lambda: e.scale_X(np.full(d, 2.0), False), x64(C, r, 2.0 * s2))):
            change()
            e.set_W(W0)
            e.sweep(1)
            ref = orc.nmf(Xnew, k, W_in=W0.copy(), T_in=T.copy(), max_iter=1, eps_stop=-1, fix_T=True, reset_topic_method=None)
            assert relfro(e.get_W(), ref['W']) < TOL, relfro(e.get_W(), ref['W'])
            assert np.array_equal(stored_matrix(e), Xnew)


# ---- 5. whole runs through nmf() ------------------------------------------------------------------------------------------
_cache = {}


def poisson_counts(n, d, k):
    """Poisson counts with k planted topics, 3 per entry on average: every row non-empty, two columns empty.  The yardstick of
    the two bounds is the reference's own sensitivity on these very matrices (CPU, oracle against oracle over 30 sweeps, X formed
    as matrixops does against X formed in the factored order with the row totals summed backwards, 1.1e-16 apart): 2000 x 300
    plain W 1.2e-13 T 6.6e-14, topic model W 2.4e-11 T 5.0e-11; 500 x 100 below 5e-14 -- the two orders of magnitude under
    2e-9 that the bound presumes.  (Sharper planted topics, factors drawn as rand^4 at 1.5 per entry, are another matter: there
    the reference alone moves by 4e-10 in the topic-model flavour, and no summation order stays inside 2e-9 of another.)"""
    key = ('C', n, d, k)
    if key not in _cache:
        rs = np.random.RandomState(n + d)
        lam = rs.rand(n, k) @ rs.rand(k, d)
        C = np.minimum(rs.poisson(lam * (3.0 / lam.mean())), 255)
        C[:, [3, d - 1]] = 0
        C[C.sum(1) == 0, 0] = 1
        assert (C.sum(1) > 0).all() and ((C.sum(0) == 0).sum() >= 2)
        from rri_nmf_amd.matrixops import tfidf, normalize
        Xt, idf = tfidf(C.astype(np.float64), return_idf=True)
        Xh = np.ascontiguousarray(normalize(Xt))
        W0, T0 = scaled_init(Xh, k, seed=1)
        _cache[key] = C.astype(U8), Xh, np.asarray(idf, dtype=np.float64).ravel(), W0, T0
    return _cache[key]


def oracle_run(tag, X, W0, T0, S, kw):
    key = (tag, X.shape, S, tuple(sorted(kw)))
    if key not in _cache:
        _cache[key] = run_oracle(X, W0, T0, S, **kw)
    return _cache[key]


@pytest.mark.parametrize('S', [1, 5, 30])
@pytest.mark.parametrize('flavour', ['plain', 'topic'])
@pytest.mark.parametrize('n, d, k', [(2000, 300, 20), (500, 100, 5)])
def test_nmf_on_counts_with_device_tfidf_and_normalisation(n, d, k, flavour, S):
    from rri_nmf_amd.nmf import nmf, ResidentProblem
    C, Xh, idf, W0, T0 = poisson_counts(n, d, k)
    kw = TM if flavour == 'topic' else {}
    holder = ResidentProblem()
    try:
        got = nmf(C, k, dtype=U8, preprocess=('tfidf', 'normalize'), W_in=W0, T_in=T0, eps_stop=-1, max_iter=S,
                  resident=holder, **kw)
        r, s = holder.engine.X_scales()
    finally:
        holder.close()
    assert np.array_equal(got['idf'], idf)                      # bit for bit the host's idf
    assert got['x_storage_relerr'] == 0.0
    # (a) against host preprocessing
    ref = oracle_run('host', Xh, W0, T0, S, kw)
    ew, et = relfro(got['W'], ref['W']), relfro(got['T'], ref['T'])
    print('%dx%d k=%d %s, %d sweeps, against matrixops: W %.3e  T %.3e' % (n, d, k, flavour, S, ew, et))
    assert ew < 1e-8 and et < 1e-8, (ew, et)
    # (b) against the matrix the handle factorises
    X64 = x64(C, r, s)
    assert np.array_equal(s, idf) and relfro(X64, Xh) < 1e-14
    ref = oracle_run('x64', X64, W0, T0, S, kw)
    ew, et = relfro(got['W'], ref['W']), relfro(got['T'], ref['T'])
    print('%dx%d k=%d %s, %d sweeps, against X64 of the scales: W %.3e  T %.3e' % (n, d, k, flavour, S, ew, et))
    assert ew < TOL and et < TOL, (ew, et)


def test_nmf_options_that_see_X_on_the_host():
    """host callbacks, store_gradients with listed rows, the Gaussian mechanism, a kept handle, obj_calculator and an NNDSVD start:
    all on the device route, against the same call on a float64 store of the host-preprocessed matrix"""
    from rri_nmf_amd.nmf import nmf, ResidentProblem
    n, d, k = 500, 100, 5
    C, Xh, idf, W0, T0 = poisson_counts(n, d, k)
    seen = []

    def spy(X, W, T):
        seen.append(np.array(X, copy=True))
        return float(np.linalg.norm(X - W @ T))
    rows = [0, 7, 499]
    common = dict(W_in=W0, T_in=T0, eps_stop=-1, max_iter=3, compute_obj_each_iter=True)
    a = nmf(C, k, dtype=U8, preprocess=('tfidf', 'normalize'), diagnostics=[spy], store_gradients=True, ind_rows_to_store=rows,
            **common)
    assert len(seen) == 4 and all(relfro(x, Xh) < 1e-14 for x in seen)          # the callbacks see the scaled matrix
    b = nmf(Xh, k, dtype=np.float64, diagnostics=[spy], store_gradients=True, ind_rows_to_store=rows, **common)
    assert relfro(a['W'], b['W']) < 1e-8 and relfro(a['T'], b['T']) < 1e-8
    for it in range(3):
        assert relfro(a['numer_W'][it], b['numer_W'][it]) < 1e-8 and relfro(a['denom_W'][it], b['denom_W'][it]) < 1e-8
    assert np.allclose(a['diagnostics']['spy'], b['diagnostics']['spy'], rtol=1e-8)
    assert np.allclose(a['obj_history'], b['obj_history'], rtol=1e-9)
    # obj_calculator makes a handle of the same store and re-applies the idf
    assert_rel(a['obj_calculator'].true_objective(), oracle().true_objective(Xh, a['W'], a['T']), 1e-10, 'obj_calculator')
    # the Gaussian mechanism: the same draws from numpy's global RNG on either store
    gm = dict(eps_gauss_t=1e7, delta_gauss_t=0.5, W_in=W0, T_in=T0, eps_stop=-1, max_iter=2)
    np.random.seed(3)
    a = nmf(C, k, dtype=U8, preprocess=('tfidf', 'normalize'), **gm)
    np.random.seed(3)
    b = nmf(Xh, k, dtype=np.float64, **gm)
    assert relfro(a['W'], b['W']) < 1e-8 and relfro(a['T'], b['T']) < 1e-8
    # a kept handle is reused, with its scales
    holder = ResidentProblem()
    try:
        a = nmf(C, k, dtype=U8, preprocess=('tfidf', 'normalize'), resident=holder, W_in=W0, T_in=T0, eps_stop=-1, max_iter=2)
        a2 = nmf(C, k, dtype=U8, preprocess=('tfidf', 'normalize'), resident=holder, W_in=W0, T_in=T0, eps_stop=-1, max_iter=2)
        assert holder.reuses == 1
    finally:
        holder.close()
    assert np.array_equal(a['W'], a2['W']) and np.array_equal(a['T'], a2['T']) and np.array_equal(a['idf'], a2['idf'])
    # the NNDSVD start runs its range finder on the uint8 handle
    kw = dict(init='nndsvd', device_init=True, random_state=0, max_iter=3, eps_stop=-1, **TM)
    a = nmf(C, k, dtype=U8, preprocess=('tfidf', 'normalize'), **kw)
    b = nmf(Xh, k, dtype=np.float64, **kw)
    assert relfro(a['W'], b['W']) < 1e-8 and relfro(a['T'], b['T']) < 1e-8, (relfro(a['W'], b['W']), relfro(a['T'], b['T']))
    # uint8 is never chosen for the caller, and what is no count is refused
    assert 'x_storage_relerr' not in nmf(C, k, W_in=W0, T_in=T0, eps_stop=-1, max_iter=1)
    with pytest.raises(ValueError, match='integer in 0..255'):
        nmf(C + 0.5, k, dtype=U8, W_in=W0, T_in=T0, max_iter=1)


# ---- 6. the reference's text fixture through the estimator ----------------------------------------------------------------
def test_topic_model_estimator_on_the_text_fixture(monkeypatch):
    from rri_nmf_amd.engine import RRIEngine
    from rri_nmf_amd.sklearn_interface import NMF_TM_Estimator
    counts = sp.load_npz(os.path.join(GOLDEN, 'ref_data', 'text_data_train.npz')).toarray()
    new = sp.load_npz(os.path.join(GOLDEN, 'ref_data', 'text_data_test.npz')).toarray()
    assert counts.shape == (100, 200) and counts.max() == 111 and np.array_equal(counts, np.round(counts))
    assert (counts.sum(1) > 0).all() and (counts.sum(0) == 0).sum() == 58 and (new.sum(1) > 0).all()
    n, d = counts.shape
    made = []
    real_init = RRIEngine.__init__

    def spy(self, *a, **kw):
        made.append(np.dtype(kw.get('dtype', np.float32)))
        return real_init(self, *a, **kw)
    monkeypatch.setattr(RRIEngine, '__init__', spy)
    out = {}
    for dt in (np.float64, U8):
        est = NMF_TM_Estimator(n, d, 5, max_iter=8, random_state=0, handle_tfidf=True, handle_normalization=True,
                               nmf_kwargs={'dtype': dt})
        made[:] = []
        est.fit(counts)
        assert made and all(m == dt for m in made), made
        fitted = est.W.copy(), est.T.copy()
        hist = list(est.nmf_outputs['obj_history'])
        est.one_iter(counts)
        made[:] = []
        Wnew = est.transform(new)
        assert made == [np.dtype(dt)], made                 # the handle made inside transform follows the store of the fit
        out[dt] = fitted + (est.W.copy(), est.T.copy(), Wnew, est.idf.copy())
        assert all(b <= a + 1e-12 * abs(hist[0]) for a, b in zip(hist, hist[1:])), hist          # monotone
        for M in (fitted[0], fitted[1], est.W, est.T, Wnew):
            assert np.abs(M.sum(1) - 1).max() < 1e-13 and M.min() >= 0
    names = ('W of fit', 'T of fit', 'W after one_iter', 'T after one_iter', 'transform(test)')
    for a, b, what in zip(out[U8], out[np.float64], names):
        assert relfro(a, b) < 1e-8, (what, relfro(a, b))
    assert np.array_equal(out[U8][5], out[np.float64][5])       # the idf


# ---- 7. normalising an empty row ---------------------------------------------------------------------------------------------
def test_normalising_an_empty_row_changes_nothing():
    from rri_nmf_amd.engine import ZeroTotalRows
    n, d = 70, 24
    C = some_counts(n, d, 5).astype(U8)
    C[[3, 69]] = 0
    r, s = scales(n, d, 6)
    r, s = np.abs(r), np.abs(s) + 1e-3
    with engine(n, d, 2, dtype=U8) as e:
        e.upload_X(C); e.set_X_scales(r, s)
        before = stored_matrix(e)
        for call in (lambda: e.scale_X(None, True), lambda: e.scale_X(np.full(d, 3.0), True),
                     lambda: e.preprocess(tfidf=True, normalize=True)):
            with pytest.raises(ValueError) as ei:
                call()
            assert isinstance(ei.value, ZeroTotalRows) and ei.value.count == 2
            gr, gs = e.X_scales()
            assert np.array_equal(gr, r) and np.array_equal(gs, s)
            assert np.array_equal(stored_matrix(e), before)
        e.scale_X(np.full(d, 3.0), False)                   # without normalisation the same column scale is taken
        assert np.array_equal(e.X_scales()[1], 3.0 * s)
    from rri_nmf_amd.nmf import nmf
    with pytest.raises(ValueError, match=r'\b2 row'):
        nmf(C, 2, dtype=U8, preprocess=('normalize',), max_iter=1)


def test_normalisation_matches_matrixops_and_composes():
    from rri_nmf_amd.matrixops import tfidf, normalize
    n, d = 203, 300
    C = np.random.RandomState(2).poisson(0.8, size=(n, d))
    C[C.sum(1) == 0, 1] = 2
    C[:, 7] = 0
    C[:, 9] = np.maximum(C[:, 9], 1)                         # a term in every document: its idf is zero (or negative and tiny)
    Xt, idf = tfidf(C.astype(np.float64), return_idf=True)
    idf = np.asarray(idf, dtype=np.float64).ravel()
    assert idf[9] <= 0 and idf[7] > 30
    want = normalize(Xt)
    with engine(n, d, 2, dtype=U8) as e:
        e.upload_X(C)
        got_idf = e.preprocess(tfidf=True, normalize=True)
        assert np.array_equal(got_idf, idf)
        got = stored_matrix(e)
        assert relfro(got, want) < 1e-14
        assert_elementwise(got, want, 8 * (d + 2) * U * np.abs(want), 'tf-idf and normalisation through the scales')
        e.preprocess(normalize=True)                        # once more: rows that sum to 1 stay, to rounding
        assert relfro(stored_matrix(e), want) < 1e-14


# ---- 8. the reset path ---------------------------------------------------------------------------------------------------------
def test_a_dead_column_is_reset_to_the_max_residual_document():
    g = load_golden('g6_rare_branches')
    n, d, k = [int(v) for v in g['shape']]
    P = planted_X(n, d, k, seed=3, dtype=np.float64)
    C = np.minimum(np.round(40.0 * P / P.mean()), 255.0).astype(U8)
    rs = np.random.RandomState(8)
    r, s = 10.0 ** rs.uniform(-1, 1, n), 10.0 ** rs.uniform(-1, 1, d)
    X = x64(C, r, s)
    _, T0 = scaled_init(X, k, seed=4)
    Wd = g['dead_W0'] * np.sqrt(X.mean() / P.mean())
    assert (Wd.sum(0) == 0).any()
    with engine(n, d, k, dtype=U8) as e:
        loaded(e, C, r, s, np.maximum(Wd, 0), np.maximum(T0, 0), t_row_sum=1.0)
        e.sweep(2)
        W, T, nres = e.get_W(), e.get_T(), e.n_resets_used
    ref = run_oracle(X, Wd, T0, 2, t_row_sum=1.0)
    assert nres >= 1 and nres == ref['n_resets_used']
    assert relfro(W, ref['W']) < TOL and relfro(T, ref['T']) < TOL, (relfro(W, ref['W']), relfro(T, ref['T']))


# ---- 9. binding a torch.uint8 tensor -------------------------------------------------------------------------------------------
def test_bind_X_device_with_a_padded_torch_uint8_tensor():
    import torch
    n, d, k, ld = 300, SPAN + VN, 5, SPAN + 4 * VN
    C = some_counts(n, d, 9).astype(U8)
    r, s = scales(n, d, 10)
    W0, T0 = scaled_init(np.abs(x64(C, r, s)), k, seed=3)
    buf = torch.full((n, ld), 0xFF, dtype=torch.uint8, device='cuda')       # pad bytes that must never reach a sum
    buf[:, :d] = torch.as_tensor(C, device='cuda')
    torch.cuda.synchronize()
    with engine(n, d, k, dtype=U8) as a, engine(n, d, k, dtype=U8) as b:
        a.upload_X(C)
        a.set_X_scales(r, s)
        b.set_X_scales(r, s)                                # binding is a new X: the scales are ones again
        b.bind_X_device(buf.data_ptr(), ld)
        assert np.array_equal(b.X_scales()[0], np.ones(n)) and np.array_equal(b.X_scales()[1], np.ones(d))
        assert np.array_equal(stored_matrix(b), C) and b.storage_relerr == 0.0
        b.set_X_scales(r, s)
        assert np.array_equal(stored_matrix(a), stored_matrix(b))
        assert np.array_equal(a.column_positive_counts(), b.column_positive_counts())
        for e in (a, b):
            e.set_W(W0); e.set_T(T0); e.set_params(reset_topic_method=None)
            e.sweep(2)
        assert np.array_equal(a.get_W(), b.get_W()) and np.array_equal(a.get_T(), b.get_T())
        assert a.objective() == b.objective()
        with pytest.raises(ValueError):
            b.bind_X_device(buf.data_ptr(), ld + VN // 2)       # no multiple of the load width
        with pytest.raises(ValueError):
            b.bind_X_device(buf.data_ptr() + VN // 2, ld)       # not aligned to the load width
    with engine(n, d - 3, k, dtype=U8) as e:
        with pytest.raises(ValueError):                         # d must be a multiple of the load width: no pad columns in bound memory
            e.bind_X_device(buf.data_ptr(), ld)


# ---- 10. refusals at the ABI -----------------------------------------------------------------------------------------------------
def test_rri_create_takes_uint8_for_the_unweighted_flavour_only():
    from rri_nmf_amd import _capi
    lib = _capi.load_library()
    names = {_capi.RRI_WEIGHTED_DENSE: 'RRI_WEIGHTED_DENSE', _capi.RRI_WEIGHTED_SPARSE: 'RRI_WEIGHTED_SPARSE',
             _capi.RRI_UNWEIGHTED_RESIDUAL: 'RRI_UNWEIGHTED_RESIDUAL', _capi.RRI_UNWEIGHTED_SPARSE: 'RRI_UNWEIGHTED_SPARSE'}
    for flavour, name in names.items():
        h = ctypes.c_void_p()
        st = lib.rri_create(ctypes.byref(h), 64, 32, 2, _capi.RRI_U8, flavour, 0, None)
        assert st == _capi.RRI_ERR_UNSUPPORTED and not h.value, (name, st)
        assert name.encode() in lib.rri_last_error(None) and b'RRI_U8' in lib.rri_last_error(None), lib.rri_last_error(None)
    h = ctypes.c_void_p()
    assert lib.rri_create(ctypes.byref(h), 64, 32, 2, _capi.RRI_U8, _capi.RRI_UNWEIGHTED, 0, None) == _capi.RRI_OK
    assert lib.rri_destroy(h) == _capi.RRI_OK
    for code in (3, 5):                                   # 3 was never a storage type and stays none; RRI_U8 is 4
        assert lib.rri_create(ctypes.byref(h), 64, 32, 2, code, _capi.RRI_UNWEIGHTED, 0, None) == _capi.RRI_ERR_INVALID


def test_a_uint8_handle_refuses_what_float16_refuses_and_never_runs_on_chip():
    from rri_nmf_amd import _capi
    C = some_counts(64, 32, 0).astype(U8)
    W0, T0 = scaled_init(C.astype(np.float64), 2, seed=1)
    with engine(64, 32, 2, dtype=U8) as e:
        e.upload_X(C); e.set_W(W0); e.set_T(T0); e.set_params()
        before = stored_matrix(e)
        Cs = sp.csr_matrix(C.astype(np.float64))
        for call in (lambda: e.upload_mask(np.ones((64, 32))), lambda: e.upload_mask_csr_pattern(Cs),
                     lambda: e.bind_mask_device(1 << 20, 32),
                     lambda: e.upload_X_csr(Cs), lambda: e.upload_observed_csr(Cs),
                     lambda: e.residual_update(np.ones(64), np.ones(32), np.ones(32), np.ones(64)),
                     lambda: e.residual_rebuild(), lambda: e.get_residual(np.float32),
                     lambda: e.bench_rank1_update(1), lambda: e.bench_stream_copy(1)):
            with pytest.raises(NotImplementedError, match='RRI_U8'):
                call()
        assert np.array_equal(stored_matrix(e), before)            # nothing touched X
        e.sweep(1)                                                 # ... or the handle's state
        lib = _capi.load_library()
        keep = (_capi.ALLREDUCE_FN(lambda u, b, c: 0), _capi.ALLGATHER_FN(lambda u, s, c, r: 0),
                _capi.BROADCAST_FN(lambda u, b, c, r: 0))
        comm = ctypes.c_void_p()
        assert lib.rri_comm_create_host(ctypes.byref(comm), 0, 1, keep[0], keep[1], keep[2], None) == _capi.RRI_OK
        try:
            assert lib.rri_attach_comm(e._h, comm, 0, 64) == _capi.RRI_ERR_UNSUPPORTED
            assert b'RRI_U8' in lib.rri_last_error(e._h)
        finally:
            lib.rri_comm_destroy(comm)
    from rri_nmf_amd.engine import RRIEngine
    for kw in (dict(weighted=True), dict(weighted='sparse'), dict(schedule='residual'), dict(sparse_x=True)):
        with pytest.raises(ValueError, match='uint8'):
            RRIEngine(64, 32, 2, dtype=U8, **kw)
    # never the persistent on-chip kernel: at 1000 x 128 a float32 handle takes it, a uint8 handle runs launch by launch
    rs = np.random.RandomState(1)
    C = rs.poisson(2.0, size=(1000, 128)).astype(U8)
    W0, T0 = scaled_init(C.astype(np.float64), 20, seed=1)
    took = {}
    for dt in (np.float32, U8):
        with engine(1000, 128, 20, dtype=dt) as e:
            e.upload_X(C.astype(np.float64)); e.set_W(W0); e.set_T(T0); e.set_params()
            took[dt] = e.onchip_info()[0]
            e.sweep(2)
            took[dt, 'launches'] = e.onchip_info()[1]
            if dt is U8:
                info = e.layout_info()
                assert info['npanels'] == 1 and not info['x_pack'], info
    assert took[np.float32] and not took[U8] and took[U8, 'launches'] == 0, took
