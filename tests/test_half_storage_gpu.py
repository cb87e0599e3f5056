"""Float16 storage of a read-only dense X (RRI_F16, nmf(..., dtype=np.float16)) on the GPU.

A float16 handle rounds X ONCE, at upload, to nearest even from the host type; every float16 value is exact in float64 and the
arithmetic is float64, so the handle must compute what the float64 reference computes on X.astype(np.float16).  Hence the
bound of tests/test_hip_parity.py for "same algorithm, different summation order" applies unchanged:

    TOL = 2e-9   relative Frobenius distance to the oracle run on X.astype(np.float16).astype(np.float64)

(the oracle's own sensitivity on these inputs -- a start perturbed by 8e-16 -- is at most 3.9e-11 over 1 / 5 / 30 sweeps at
2000 x 300 k = 20: the same figures as on the float32-rounded X).  A miss means a kernel bug or a rounding that is not single.
Single steps are checked element by element with the bounds of tests/test_kernel_buckets_gpu.py, whose helpers are imported.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, load_golden, relfro
from rri_nmf_amd.synthetic import planted_X, scaled_init
from test_hip_parity import run_engine, run_oracle
from test_kernel_buckets_gpu import (U, FLAGS, assert_elementwise, assert_rel, check_steps, near_solution, problem)

pytestmark = pytest.mark.gpu

H = np.float16
TOL = 2e-9


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def oracle():
    from oracle import rri_oracle
    return rri_oracle


def rounded(X):
    """X as a float16 handle holds it, in float64"""
    return np.ascontiguousarray(np.asarray(X).astype(H).astype(np.float64))


def stored_matrix(e):
    """the stored X, exactly: sums with zeros are exact"""
    return e.X_times(np.eye(e.d))


# the values at which a rounding that is not single, not to even, or not exact for subnormals shows
SPECIALS = [1 + 2.0 ** -11 + 2.0 ** -30, -(1 + 2.0 ** -11 + 2.0 ** -30),      # double -> float -> half would give 1.0
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11,                               # exact ties: to even
            2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15, 2.0 ** -26,               # subnormals; one that rounds to zero
            65504.0, 65519.9, 0.0, 2048.0, 2049.0]


# ---- 1. what is stored ------------------------------------------------------------------------------------------------
def test_the_special_values_are_rounded_once_to_even():
    X = np.zeros((4, 8))
    X.flat[:len(SPECIALS)] = SPECIALS
    want = np.array([1 + 2.0 ** -10, -(1 + 2.0 ** -10), 1.0, 1 + 2.0 ** -9, 2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -15, 0.0,
                     65504.0, 65504.0, 0.0, 2048.0, 2048.0])
    assert np.array_equal(X.astype(H).astype(np.float64).flat[:len(SPECIALS)], want)       # numpy's answer, spelled out
    with engine(4, 8, 2, dtype=H) as e:
        e.upload_X(X)
        got = stored_matrix(e)
    assert np.array_equal(got.flat[:len(SPECIALS)], want), (got.flat[:len(SPECIALS)], want)


@pytest.mark.parametrize('d', [7, 8, 9, 300, 2047, 2048, 2049])
@pytest.mark.parametrize('n', [1, 63, 65, 1000])
def test_stored_matrix_equals_numpys_astype_bit_for_bit(n, d):
    rs = np.random.RandomState(n + d)
    X = rs.rand(n, d) * np.where(rs.rand(n, d) < 0.3, 1e-4, 50.0)          # many float16 subnormals among them
    idx = np.arange(0, n * d, 3)
    X.flat[idx] = np.resize(np.roll(SPECIALS, n + d), idx.size)
    X[-1, -1] = SPECIALS[0]                                                   # the last element of the last panel
    with engine(n, d, 2, dtype=H) as e:
        npan = e.layout_info()['npanels']
        assert npan == -(-(-(-d // 8) * 8) // 2048), npan
        for src in (np.float64, np.float32, H):
            Xh = np.ascontiguousarray(X.astype(src))
            e.upload_X(Xh)
            got = stored_matrix(e)
            want = Xh.astype(H).astype(np.float64)
            bad = got != want
            assert not bad.any(), ('host %s: %d elements differ, first at %s: stored %r, numpy %r' % (
                np.dtype(src).name, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], want[bad][0]))
            num = float(((Xh.astype(np.float64) - want) ** 2).sum())
            den = float((Xh.astype(np.float64) ** 2).sum())
            assert abs(e.storage_relerr - np.sqrt(num / den)) <= 1e-12 * np.sqrt(num / den), (e.storage_relerr, np.sqrt(num / den))
            assert (e.storage_relerr == 0.0) == (src is H)


def test_storage_relerr_is_zero_for_integer_counts():
    X = np.random.RandomState(0).randint(0, 2049, size=(130, 77)).astype(np.float64)
    with engine(130, 77, 3, dtype=H) as e:
        e.upload_X(X)
        assert e.storage_relerr == 0.0
        assert np.array_equal(stored_matrix(e), X)
    with engine(130, 77, 3, dtype=np.float32) as e:        # nothing is reported on the other stores
        e.upload_X(X + 0.1)
        assert e.storage_relerr == 0.0


@pytest.mark.parametrize('bad', [65520.0, -65520.0, np.inf, np.nan])
@pytest.mark.parametrize('src', [np.float64, np.float32])
def test_values_outside_the_float16_range_are_refused_at_upload(bad, src):
    X = planted_X(70, 24, 3, seed=0, dtype=np.float64)
    W0, T0 = scaled_init(X, 3, seed=1)
    with engine(70, 24, 3, dtype=H) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
        e.sweep(1)                                          # a good X first: the refusal must take it away
        Xb = X.astype(src)
        Xb[69, 23] = bad
        with pytest.raises(ValueError, match='float16 range'):
            e.upload_X(Xb)
        with pytest.raises(ValueError, match='X, W, T and params must be set'):
            e.sweep(1)
        e.upload_X(X)                                       # ... and the handle takes a good one again
        e.sweep(1)
    if np.isfinite(bad):
        Xb = X.astype(H)
        Xb[0, 0] = H(np.inf)
        with engine(70, 24, 3, dtype=H) as e:
            with pytest.raises(ValueError, match='float16 range'):
                e.upload_X(Xb)


# ---- 2. parity with the oracle on the rounded X -------------------------------------------------------------------------
def g5_problem(tag):
    g = load_golden('g5_plain_' + tag)
    n, d, k = [int(v) for v in g['shape']]
    X = planted_X(n, d, k, seed=0, dtype=np.float64)
    W0, T0 = scaled_init(X, k, seed=1)
    return X, W0, T0


def assert_close(W, T, ref, what):
    ew, et = relfro(W, ref['W']), relfro(T, ref['T'])
    print('%s: W %.3e  T %.3e' % (what, ew, et))
    assert ew < TOL and et < TOL, (what, ew, et)


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_plain_flavour_matches_the_oracle_on_the_rounded_X(tag):
    X, W0, T0 = g5_problem(tag)
    Xs = rounded(X)
    assert relfro(Xs, X) > 1e-5            # the rounding is there: the float64 X is NOT what the handle factorises
    for S in (1, 5, 30):
        W, T, _ = run_engine(X, W0, T0, S, H)
        assert_close(W, T, run_oracle(Xs, W0, T0, S), 'plain %s, %d sweeps' % (tag, S))


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_topic_model_flavour_on_the_row_normalised_X(tag):
    """rows of X sum to 1: 4-10 % of the positive entries are float16 subnormals"""
    X, W0, T0 = g5_problem(tag)
    orc = oracle()
    Xn = orc.normalize(X.copy())
    Xs = rounded(Xn)
    pos = Xs[Xs > 0]
    assert 0.02 < (pos < 2.0 ** -14).mean() < 0.2, (pos < 2.0 ** -14).mean()
    T0p = orc.proj_rows_simplex(np.maximum(T0, 0).copy(), 1.0)
    tm = dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
    for S in (1, 5):
        W, T, _ = run_engine(Xn, W0, T0p, S, H, final_proj=1.0, **tm)
        assert_close(W, T, run_oracle(Xs, W0, T0, S, **tm), 'topic model %s, %d sweeps' % (tag, S))
        assert np.abs(T.sum(1) - 1).max() < 1e-12 and np.abs(W.sum(1) - 1).max() < 1e-12
        assert W.min() >= 0 and T.min() >= 0


def test_regularisers_and_fixed_halves():
    X, W0, T0 = g5_problem('a')
    Xs = rounded(X)
    regs = dict(reg_w_l1=0.01, reg_t_l1=0.02, reg_w_l2=0.05, reg_t_l2=0.03)
    W, T, _ = run_engine(X, W0, T0, 5, H, **regs)
    assert_close(W, T, run_oracle(Xs, W0, T0, 5, **regs), 'all four regularisers')
    W, T, _ = run_engine(X, W0, T0, 3, H, fix_T=True)
    ref = run_oracle(Xs, W0, T0, 3, fix_T=True)
    assert relfro(W, ref['W']) < TOL and np.array_equal(T, np.maximum(T0, 0))
    W, T, _ = run_engine(X, W0, T0, 3, H, fix_W=True)
    assert_close(W, T, run_oracle(Xs, W0, T0, 3, fix_W=True), 'fix_W')


def test_rare_branches_against_the_oracle_on_the_rounded_X():
    """the cases of tests/test_hip_parity.py::test_rare_branches, compared with the oracle on the rounded X (not with the stored
    vectors, which were made from the float64 X): k_resid and k_reset_row are reached in float16"""
    g = load_golden('g6_rare_branches')
    n, d, k = [int(v) for v in g['shape']]
    X = planted_X(n, d, k, seed=3, dtype=np.float64)
    W0, T0 = scaled_init(X, k, seed=4)
    orc = oracle()
    Xs = rounded(X)
    Xn = orc.normalize(X.copy())
    Xns = rounded(Xn)
    T0p = orc.proj_rows_simplex(np.maximum(T0, 0).copy(), 1.0)
    tm = dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
    # T side c <= 0 -> one-hot rows; W side c <= 0 -> entries at ub
    W, T, _ = run_engine(Xn, W0, T0p, 3, H, final_proj=1.0, reg_t_l2=-50.0, **tm)
    assert_close(W, T, run_oracle(Xns, W0, T0, 3, reg_t_l2=-50.0, **tm), 'negative reg_t_l2')
    W, T, _ = run_engine(Xn, W0, T0p, 2, H, reg_w_l2=-5.0, **tm)
    assert_close(W, T, run_oracle(Xns, W0, T0, 2, reg_w_l2=-5.0, do_final_project_W=False, **tm), 'negative reg_w_l2')
    Wd = g['dead_W0']
    with pytest.raises(ValueError, match='unbounded'):
        run_engine(X, Wd, T0, 2, H)
    with pytest.raises(ValueError, match='unbounded'):
        run_oracle(Xs, Wd, T0, 2)
    # a dead column, reset to the max-residual document on the device (k_resid, k_reset_row on the float16 X)
    W, T, nres = run_engine(X, Wd, T0, 2, H, t_row_sum=1.0)
    ref = run_oracle(Xs, Wd, T0, 2, t_row_sum=1.0)
    assert nres >= 1 and nres == ref['n_resets_used']
    assert_close(W, T, ref, 'dead column, max_resid_document')
    # resets off / exhausted: the reference's assert, from the handle and from the oracle
    for kw in (dict(reset_topic_method=None), dict(n_resets=0)):
        with pytest.raises(AssertionError, match='sums to 0'):
            run_engine(X, Wd, T0, 2, H, t_row_sum=1.0, w_row_sum=1.0, **kw)
        with pytest.raises(AssertionError, match='sums to 0'):
            run_oracle(Xs, Wd, T0, 2, t_row_sum=1.0, w_row_sum=1.0, do_final_project_W=False, **kw)
    with pytest.raises(ValueError, match='unbounded'):
        run_engine(X, Wd, T0, 2, H, t_row_sum=1.0, reset_topic_method=None)
    # every T row killed by a huge l1 penalty: k resets in one sweep; the same from the W side, both reset methods
    W, T, nres = run_engine(X, W0, T0, 1, H, t_row_sum=1.0, reg_t_l1=1e6)
    assert nres == k
    assert_close(W, T, run_oracle(Xs, W0, T0, 1, t_row_sum=1.0, reg_t_l1=1e6), 'six T-row resets in one sweep')
    W, T, nres = run_engine(X, W0, T0, 1, H, t_row_sum=1.0, reg_w_l1=1e6)
    assert nres == k
    assert_close(W, T, run_oracle(Xs, W0, T0, 1, t_row_sum=1.0, reg_w_l1=1e6), 'six W-column resets in one sweep')
    W, T, nres = run_engine(X, W0, T0, 1, H, t_row_sum=1.0, reg_w_l1=1e6, reset_topic_method='random', fix_reset_seed=True)
    assert nres == k
    assert_close(W, T, run_oracle(Xs, W0, T0, 1, t_row_sum=1.0, reg_w_l1=1e6, reset_topic_method='random', fix_reset_seed=True),
                 "six W-column resets, 'random'")


# ---- 3. single steps at the geometry edges --------------------------------------------------------------------------------
# A workgroup of the float16 pass covers 2048 columns (4 waves x 64 lanes x 8 halves): d = 2040 / 2048 / 2056 lie one vector
# below, at and above one panel group, 4104 = 2 x 2048 + 8 has a third group of one vector, d = 8 is one vector in all.
# Rows: the host gives small n row blocks of 32 (rri_create: at least 32 rows per block), so n = 31, 32, 33 are rpb - 1, rpb,
# rpb + 1 -- one ragged block, one full block, two blocks with one row in the second -- and 64 / 65 two full blocks and a third.
EDGE_D = [8, 2040, 2048, 2056, 4104]
EDGE_N = [31, 32, 33, 64, 65]
EDGE_K = [1, 2, 50, 65, 110]              # crosses ONCHIP_MAX_K = 64 and the one-launch fixed-T bound at 109 / 110


@pytest.mark.parametrize('d', EDGE_D)
@pytest.mark.parametrize('n', EDGE_N)
@pytest.mark.parametrize('k', EDGE_K)
def test_single_steps_at_the_geometry_edges(k, n, d):
    orc = oracle()
    # (a random start at k >= 65 on 8 columns leaves some T rows with nothing to explain: the closed form is the zero row and the
    # step ends in a reset; from a start near a solution every row and column stays alive, as in tests/test_kernel_buckets_gpu.py)
    X, W0, T0 = near_solution(n, d, k, seed=n + d) if k >= 65 else problem(n, d, k, seed=n + d)
    Xs = rounded(X)
    for flags in (['plain', 'topic'] if k in (2, 50) else ['plain']):
        with engine(n, d, k, dtype=H) as e:
            info = e.layout_info()
            ld = -(-d // 8) * 8
            assert info['npanels'] == -(-ld // 2048), info                  # a silent fallback to another vector width shows here
            assert info['rpb'] == 32 and info['nrb'] == -(-n // 32), info   # ... and the row blocks are the ones described above
            e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(**FLAGS[flags])
            assert not e.onchip_info()[0]
            assert_rel(e.objective(), orc.true_objective(Xs, W0, T0), 1e-12, 'objective right after set_W / set_T')
            for t in sorted({0, k - 1}):
                wR, nw = e.topic_sums(t)
                want_wR, want_nw = orc.residual_products_T(Xs, W0.copy(), T0, t)
                assert_elementwise(wR[None, :], want_wR[None, :], 1e-12 * np.abs(want_wR).max(), 'wR of topic %d' % t)
                assert_rel(nw, float(want_nw), 1e-13, '||w_t||^2 of topic %d' % t)
            check_steps(e, Xs, k, FLAGS[flags])
            W, T = e.get_W(), e.get_T()
            assert_rel(e.objective(), orc.true_objective(Xs, W, T), 1e-12, 'objective after the steps')
    rs = np.random.RandomState(k + n + d)
    B, Q = rs.randn(d, 3), rs.randn(n, 9)
    with engine(n, d, k, dtype=H) as e:
        e.upload_X(X)
        got, want = e.X_times(B), Xs @ B
        for j in range(B.shape[1]):
            err = np.linalg.norm(got[:, j] - want[:, j]) / np.linalg.norm(want[:, j])
            assert err <= 1e-13, ('X B column', j, err)
        assert_elementwise(got, want, 4.0 * (d + 2) * U * (np.abs(Xs) @ np.abs(B)), 'X B')
        got, want = e.Xt_times(Q), Xs.T @ Q
        for j in range(Q.shape[1]):
            err = np.linalg.norm(got[:, j] - want[:, j]) / np.linalg.norm(want[:, j])
            assert err <= 1e-13, ('X^T Q column', j, err)
        assert_elementwise(got, want, 4.0 * (n + 2) * U * (np.abs(Xs).T @ np.abs(Q)), 'X^T Q', rows_are='column tile of X')


@pytest.mark.parametrize('k', [109, 110], ids=['k=109-one-launch', 'k=110-launch-per-topic'])
def test_fixed_T_sweeps_on_both_sides_of_the_one_launch_bound(k):
    n, d = 203, 2056
    X, W0, T0 = near_solution(n, d, k, seed=k)
    Xs = rounded(X)
    with engine(n, d, k, dtype=H) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(fix_T=True, reset_topic_method=None)
        e.timing_enable(True)
        e.sweep(3)
        launches = e.timing_read(1)[0]
        W, T = e.get_W(), e.get_T()
    assert launches == 3 if k <= 109 else launches >= 3 * k, launches
    ref = oracle().nmf(Xs, k, W_in=W0.copy(), T_in=T0.copy(), max_iter=3, eps_stop=-1, fix_T=True, reset_topic_method=None)
    assert relfro(W, ref['W']) < TOL and np.array_equal(T, T0)


# ---- 4. same values, other store ----------------------------------------------------------------------------------------
def integer_problem(n=2000, d=300, k=20):
    P = planted_X(n, d, k, seed=0, dtype=np.float64)
    X = np.minimum(np.round(4.0 * P / P.mean()), 15.0)
    W0, T0 = scaled_init(X, k, seed=1)
    return X, W0, T0


def test_integer_X_gives_the_same_result_in_either_store_and_the_same_bits_twice():
    X, W0, T0 = integer_problem()
    assert X.max() <= 15 and X.min() >= 0 and np.array_equal(X, np.round(X)) and len(np.unique(X)) > 8
    W16, T16, _ = run_engine(X, W0, T0, 5, H)
    W32, T32, _ = run_engine(X, W0, T0, 5, np.float32)
    assert relfro(W16, W32) < TOL and relfro(T16, T32) < TOL, (relfro(W16, W32), relfro(T16, T32))
    Wb, Tb, _ = run_engine(X, W0, T0, 5, H)
    assert np.array_equal(W16, Wb) and np.array_equal(T16, Tb)


# ---- 5. never the persistent on-chip kernel -----------------------------------------------------------------------------------
def test_a_float16_handle_runs_launch_by_launch():
    X, W0, T0 = integer_problem()
    n, d = X.shape
    took = {}
    for dt in (np.float32, H):
        with engine(n, d, 20, dtype=dt) as e:
            e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
            took[dt] = e.onchip_info()[0]
            e.sweep(2)
            took[dt, 'launches'] = e.onchip_info()[1]
    assert took[np.float32] and not took[H], took
    assert took[H, 'launches'] == 0


# ---- 6. refusals at the ABI -------------------------------------------------------------------------------------------------
def test_rri_create_refuses_float16_for_the_other_flavours():
    from rri_nmf_amd import _capi
    lib = _capi.load_library()
    names = {_capi.RRI_WEIGHTED_DENSE: 'RRI_WEIGHTED_DENSE', _capi.RRI_WEIGHTED_SPARSE: 'RRI_WEIGHTED_SPARSE',
             _capi.RRI_UNWEIGHTED_RESIDUAL: 'RRI_UNWEIGHTED_RESIDUAL', _capi.RRI_UNWEIGHTED_SPARSE: 'RRI_UNWEIGHTED_SPARSE'}
    for flavour, name in names.items():
        h = ctypes.c_void_p()
        st = lib.rri_create(ctypes.byref(h), 64, 32, 2, _capi.RRI_F16, flavour, 0, None)
        assert st == _capi.RRI_ERR_UNSUPPORTED and not h.value, (name, st)
        assert name.encode() in lib.rri_last_error(None), lib.rri_last_error(None)
    h = ctypes.c_void_p()
    assert lib.rri_create(ctypes.byref(h), 64, 32, 2, _capi.RRI_F16, _capi.RRI_UNWEIGHTED, 0, None) == _capi.RRI_OK
    assert lib.rri_destroy(h) == _capi.RRI_OK
    assert lib.rri_create(ctypes.byref(h), 64, 32, 2, 3, _capi.RRI_UNWEIGHTED, 0, None) == _capi.RRI_ERR_INVALID


def test_a_float16_handle_refuses_what_rewrites_X_or_needs_another_store():
    from rri_nmf_amd import _capi
    X = planted_X(64, 32, 3, seed=0, dtype=np.float64)
    W0, T0 = scaled_init(X, 2, seed=1)
    with engine(64, 32, 2, dtype=H) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
        before = stored_matrix(e)
        for call in (lambda: e.preprocess(tfidf=True), lambda: e.preprocess(normalize=True),
                     lambda: e.scale_X(np.ones(32)), lambda: e.column_positive_counts(),
                     lambda: e.upload_mask(np.ones((64, 32))), lambda: e.upload_mask_csr_pattern(sp.csr_matrix(X)),
                     lambda: e.upload_X_csr(sp.csr_matrix(X)), lambda: e.upload_observed_csr(sp.csr_matrix(X)),
                     lambda: e.residual_update(np.ones(64), np.ones(32), np.ones(32), np.ones(64)),
                     lambda: e.residual_rebuild(), lambda: e.get_residual(np.float32),
                     lambda: e.bench_rank1_update(1), lambda: e.bench_stream_copy(1)):
            with pytest.raises(NotImplementedError, match='RRI_F16'):
                call()
        assert np.array_equal(stored_matrix(e), before)            # nothing touched X
        e.sweep(1)                                                 # ... or the handle's state
        # row-sharding: refused at attach (one rank, host transport)
        lib = _capi.load_library()
        keep = (_capi.ALLREDUCE_FN(lambda u, b, c: 0), _capi.ALLGATHER_FN(lambda u, s, c, r: 0),
                _capi.BROADCAST_FN(lambda u, b, c, r: 0))
        comm = ctypes.c_void_p()
        assert lib.rri_comm_create_host(ctypes.byref(comm), 0, 1, keep[0], keep[1], keep[2], None) == _capi.RRI_OK
        try:
            assert lib.rri_attach_comm(e._h, comm, 0, 64) == _capi.RRI_ERR_UNSUPPORTED
            assert b'RRI_F16' in lib.rri_last_error(e._h)
        finally:
            lib.rri_comm_destroy(comm)
    from rri_nmf_amd.engine import RRIEngine
    for kw in (dict(weighted=True), dict(weighted='sparse'), dict(schedule='residual'), dict(sparse_x=True)):
        with pytest.raises(ValueError, match='float16'):
            RRIEngine(64, 32, 2, dtype=H, **kw)


# ---- 7. binding a torch.float16 tensor --------------------------------------------------------------------------------------
def test_bind_X_device_with_a_torch_float16_tensor():
    import torch
    n, d, k = 300, 2056, 5
    X = planted_X(n, d, k, seed=2, dtype=np.float64)
    W0, T0 = scaled_init(X, k, seed=3)
    xt = torch.as_tensor(X.astype(H), device='cuda')
    assert xt.dtype == torch.float16
    torch.cuda.synchronize()
    with engine(n, d, k, dtype=H) as a, engine(n, d, k, dtype=H) as b:
        a.upload_X(X)
        b.bind_X_device(xt.data_ptr(), xt.stride(0))
        assert b.storage_relerr == 0.0 and a.storage_relerr > 0.0
        assert np.array_equal(stored_matrix(a), stored_matrix(b))
        for e in (a, b):
            e.set_W(W0); e.set_T(T0); e.set_params()
            e.sweep(3)
        assert np.array_equal(a.get_W(), b.get_W()) and np.array_equal(a.get_T(), b.get_T())
        with pytest.raises(ValueError):
            b.bind_X_device(xt.data_ptr() + 2, xt.stride(0))        # not 16-byte aligned
    with engine(n, 2052, k, dtype=H) as e:
        with pytest.raises(ValueError):                             # d must be a multiple of 8: no pad columns in bound memory
            e.bind_X_device(xt.data_ptr(), xt.stride(0))


# ---- 8. through the public surface ---------------------------------------------------------------------------------------------
def test_nmf_with_float16_storage_matches_the_oracle_on_the_rounded_X():
    from rri_nmf_amd.nmf import nmf
    X, W0, T0 = g5_problem('a')
    k = W0.shape[1]
    Xs = rounded(X)
    got = nmf(X, k, dtype=H, W_in=W0, T_in=T0, eps_stop=-1, max_iter=5)
    ref = run_oracle(Xs, W0, T0, 5)
    assert_close(got['W'], got['T'], ref, 'nmf(dtype=float16), 5 sweeps')
    assert abs(got['x_storage_relerr'] - relfro(Xs, X)) <= 1e-12 * relfro(Xs, X)
    assert 'x_storage_relerr' not in nmf(X, k, dtype=np.float32, W_in=W0, T_in=T0, eps_stop=-1, max_iter=1)
    # per-row weights: sqrt(w_row) * X in float64 on the host, rounded once; the refit with T fixed on its own float16 handle
    w_row = np.random.RandomState(5).rand(X.shape[0], 1) + 0.5
    got = nmf(X, k, dtype=H, w_row=w_row, W_in=W0, T_in=T0, eps_stop=-1, max_iter=3)
    ref = nmf(rounded(np.sqrt(w_row) * X), k, dtype=np.float64, W_in=W0, T_in=T0, eps_stop=-1, max_iter=3)
    assert relfro(got['T'], ref['T']) < TOL, relfro(got['T'], ref['T'])
    assert got['W'].shape == W0.shape and got['W'].min() >= 0 and np.isfinite(got['W']).all()
    with pytest.raises(ValueError, match='float16 range'):
        nmf(X * 1e5, k, dtype=H, W_in=W0, T_in=T0, max_iter=1)


def test_nndsvd_start_runs_its_range_finder_on_the_float16_handle():
    from rri_nmf_amd.nmf import nmf
    X, _, _ = g5_problem('a')
    k = 6
    Xs = rounded(X)
    kw = dict(init='nndsvd', device_init=True, random_state=0, max_iter=3, eps_stop=-1)
    a = nmf(X, k, dtype=H, **kw)
    b = nmf(Xs, k, dtype=np.float64, **kw)
    # the bound tests/test_preprocess_gpu.py uses for two routes to the same NNDSVD start
    assert relfro(a['W'], b['W']) < 1e-8 and relfro(a['T'], b['T']) < 1e-8, (relfro(a['W'], b['W']), relfro(a['T'], b['T']))
    # tf-idf and normalisation: in float64 on the host, rounded once
    from rri_nmf_amd.matrixops import tfidf, normalize
    C = np.random.RandomState(1).poisson(0.7, size=(240, 152)).astype(np.float64)
    kw = dict(init='nndsvd', device_init=True, random_state=0, max_iter=3, eps_stop=-1, project_T_each_iter=True, t_row_sum=1.0,
              w_row_sum=1.0)
    a = nmf(C, 4, dtype=H, preprocess=('tfidf', 'normalize'), **kw)
    b = nmf(rounded(normalize(tfidf(C))), 4, dtype=np.float64, **kw)
    assert relfro(a['W'], b['W']) < 1e-8 and relfro(a['T'], b['T']) < 1e-8, (relfro(a['W'], b['W']), relfro(a['T'], b['T']))
    assert a['x_storage_relerr'] > 0


def test_topic_model_estimator_with_a_float16_store(monkeypatch):
    import os
    from rri_nmf_amd.engine import RRIEngine
    from rri_nmf_amd.sklearn_interface import NMF_TM_Estimator
    counts = sp.load_npz(os.path.join(GOLDEN, 'ref_data', 'text_data_train.npz')).toarray()
    assert np.array_equal(counts.astype(H).astype(np.float64), counts) and counts.max() == 111
    n, d = counts.shape
    made = []
    real_init = RRIEngine.__init__

    def spy(self, *a, **kw):
        made.append(np.dtype(kw.get('dtype', np.float32)))
        return real_init(self, *a, **kw)
    monkeypatch.setattr(RRIEngine, '__init__', spy)
    out = {}
    for dt in (np.float64, H):
        est = NMF_TM_Estimator(n, d, 5, max_iter=8, nmf_kwargs={'dtype': dt})
        made[:] = []
        est.fit(counts)
        assert made and all(m == dt for m in made), made
        made[:] = []
        Wnew = est.transform(counts)
        assert made == [np.dtype(dt)], made             # the handle made inside transform follows the store of the fit
        out[dt] = est.W.copy(), est.T.copy(), Wnew
    for a, b, what in zip(out[H], out[np.float64], ('W', 'T', 'transform(X)')):
        assert relfro(a, b) < TOL, (what, relfro(a, b))
    assert np.array_equal(np.argmax(out[H][0], 1), np.argmax(out[np.float64][0], 1))
    assert np.array_equal(np.argmax(out[H][2], 1), np.argmax(out[np.float64][2], 1))


# ---- 9. full size ------------------------------------------------------------------------------------------------------------------
N, D, K = 100000, 10000, 50
EPS = float(np.spacing(10))


@pytest.fixture(scope='module')
def full_size():
    """the problem of tests/test_full_size_gpu.py, made on the device and kept as halves (2 GB)"""
    import torch
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    Ts = torch.rand(K, D, device=dev, generator=g) * (torch.rand(K, D, device=dev, generator=g) < 0.3)
    X = torch.empty(N, D, device=dev, dtype=torch.float16)
    for lo in range(0, N, 25000):
        Ws = torch.rand(25000, K, device=dev, generator=g) * (torch.rand(25000, K, device=dev, generator=g) < 0.3)
        blk = torch.matmul(Ws, Ts)
        blk.add_(torch.rand(25000, D, device=dev, generator=g), alpha=0.01)
        X[lo:lo + 25000] = blk.to(torch.float16)
        del blk
    a = float(torch.sqrt(X.mean(dtype=torch.float64) / K))
    W0 = a * torch.rand(N, K, device=dev, generator=g, dtype=torch.float64)
    T0 = a * torch.rand(K, D, device=dev, generator=g, dtype=torch.float64)
    torch.cuda.synchronize()
    yield X, W0, T0
    del X
    torch.cuda.empty_cache()


def test_full_size_one_topic_step_equals_the_closed_form(full_size):
    import torch
    from test_full_size_gpu import f64_matvec
    X, W0, T0 = full_size
    t = 3
    with engine(N, D, K, dtype=H) as e:
        e.bind_X_device(X.data_ptr(), X.stride(0))
        info = e.layout_info()
        assert info['npanels'] == 5, info                  # 10000 columns in workgroups of 2048
        e.set_W(W0.cpu().numpy()); e.set_T(T0.cpu().numpy()); e.set_params()
        e.update_T_row(t)
        T1 = torch.from_numpy(e.get_T()).to(X.device)
        e.update_W_col(t)
        W1 = torch.from_numpy(e.get_W()).to(X.device)
    w = W0[:, t]
    g = w @ W0
    g[t] = 0
    wR = f64_matvec(X, w, True) - g @ T0
    want_T = torch.clamp(wR, min=0) / (w @ w + EPS)
    err_T = float(torch.linalg.norm(T1[t] - want_T) / torch.linalg.norm(want_T))
    assert err_T < 1e-12, err_T
    assert torch.equal(T1[torch.arange(K) != t], T0[torch.arange(K) != t].to(T1.dtype))
    tt = T1[t]
    h = T1 @ tt
    nt = float(h[t])
    h[t] = 0
    Rt = f64_matvec(X, tt, False) - W0 @ h
    want_W = torch.clamp(Rt, min=0) / (nt + EPS)
    err_W = float(torch.linalg.norm(W1[:, t] - want_W) / torch.linalg.norm(want_W))
    assert err_W < 1e-12, err_W


def test_full_size_sweeps_decrease_the_objective_and_resume_exactly(full_size):
    X, W0, T0 = full_size
    W0h, T0h = W0.cpu().numpy(), T0.cpu().numpy()
    objs = []
    with engine(N, D, K, dtype=H) as e:
        e.bind_X_device(X.data_ptr(), X.stride(0)); e.set_W(W0h); e.set_T(T0h); e.set_params()
        objs.append(e.objective())
        for _ in range(3):
            e.sweep(1)
            objs.append(e.objective())
        Wa, Ta = e.get_W(), e.get_T()
        assert e.n_resets_used == 0
    assert all(b <= a for a, b in zip(objs, objs[1:])), objs
    assert Wa.min() >= 0 and Ta.min() >= 0 and np.isfinite(Wa).all() and np.isfinite(Ta).all()
    with engine(N, D, K, dtype=H) as e:
        e.bind_X_device(X.data_ptr(), X.stride(0)); e.set_W(W0h); e.set_T(T0h); e.set_params()
        e.sweep(3)
        Wb, Tb = e.get_W(), e.get_T()
    assert np.array_equal(Wa, Wb) and np.array_equal(Ta, Tb)      # three calls of one sweep == one call of three
