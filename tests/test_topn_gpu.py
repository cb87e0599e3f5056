"""Top-N rows on the device (rri_topn_rows, RRIEngine.topn_rows, NMF_RS_Estimator.recommend) against the numpy restatement of
tests/topn_cases.py.

Exact cases: W, T integers in 0..7 -- every product and every sum is exact in any order, ties are everywhere -- so indices and
values must EQUAL the restatement.  Real-valued cases: uniform random factors at k = 5, 20, 200, 1024 (d = 257, 65 rows, N = 10)
under the rules of topn_cases.check_real, whose tolerance 2 k 2^-52 max_j (|W[i]| |T|)_j follows from the rounding of two
differently ordered length-k sums; no row is left out.  The same real-valued cases once more on a dense weighted, a
pattern-only, a CSR-X, a float16 and a uint8 handle: the call reads W and T alone and must not care.  Then clip, repeatability,
permuted requests, that no state a sweep reads is disturbed (bit for bit, on a handle that takes the register-resident sweep and
on an explicit-residual one), refusals, and the estimator end to end on the recommender fixture."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import topn_cases as tc
from conftest import load_golden
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def factors_only(W, T):
    """a float64 unweighted handle with factors and no X"""
    e = engine(W.shape[0], T.shape[1], W.shape[1], dtype=np.float64)
    e.set_W(W), e.set_T(T)
    return e


def test_the_case_list_covers_what_it_promises():
    cs = tc.EXACT_CASES
    assert {c.k for c in cs} == tc.K_VALUES and {c.d for c in cs} == tc.D_VALUES
    assert {c.count for c in cs} == tc.COUNT_VALUES and tc.N_VALUES <= {c.n_top for c in cs}
    assert any(c.n_top > c.d for c in cs)
    assert {c.excl for c in cs} == {None, 'empty', 'all', 'short'} and {c.rows for c in cs} == {None, 'perm'}
    for tail in (lambda c: c.d % 16, lambda c: c.count % 64, lambda c: c.k % 4):
        assert any(tail(c) and c.excl in ('all', 'short') for c in cs) and any(tail(c) and c.excl is None for c in cs)


@pytest.mark.parametrize('case', tc.EXACT_CASES, ids=[tc.case_id(c) for c in tc.EXACT_CASES])
def test_exact_cases_equal_the_restatement(case):
    W, T, rows, excl = tc.make_exact(case)
    want_j, want_v = tc.topn_reference(W, T, rows, case.n_top, excl)
    if case.excl in ('all', 'short'):
        assert (want_j == -1).any()                     # the case does leave a row short
    before = None if excl is None else (excl.indptr.copy(), excl.indices.copy())
    e = factors_only(W, T)
    try:
        got_j, got_v = e.topn_rows(rows, case.n_top, exclude=excl)
    finally:
        e.close()
    assert got_j.dtype == np.int32 and got_v.dtype == np.float64
    assert np.array_equal(got_j, want_j), np.argwhere(got_j != want_j)[:5]
    assert np.array_equal(got_v, want_v, equal_nan=True)
    if before is not None:                              # sorted on a copy: the caller's arrays are as they were
        assert np.array_equal(excl.indptr, before[0]) and np.array_equal(excl.indices, before[1])


REAL_K = (5, 20, 200, 1024)


def real_problem(k):
    W, T = tc.make_real(k)
    excl = tc.make_exclusion('short', W.shape[0], T.shape[1], 10, seed=k)
    return W, T, excl


@pytest.mark.parametrize('k', REAL_K)
def test_real_valued_cases_within_the_rounding_of_two_sums(k):
    W, T, excl = real_problem(k)
    e = factors_only(W, T)
    try:
        for ex in (None, excl):
            j, v = e.topn_rows(None, 10, exclude=ex)
            worst = tc.check_real(W, T, None, 10, ex, (None, None), j, v)
            print('k = %d, %s: largest difference / tolerance %.3f' % (k, 'exclusion' if ex is not None else 'no exclusion', worst))
    finally:
        e.close()


def _weighted(n, d, k):
    X = planted_X(n, d, k, seed=3, dtype=np.float64)
    e = engine(n, d, k, dtype=np.float64, weighted=True)
    e.upload_X(X), e.upload_mask((np.random.RandomState(4).rand(n, d) < 0.3).astype(np.float64))
    return e


def _sparse(kind):
    def make(n, d, k):
        X = planted_X(n, d, k, seed=3, dtype=np.float64) * (np.random.RandomState(4).rand(n, d) < 0.2)
        X[:, 0] = 1.0                                   # no empty row
        e = engine(n, d, k, dtype=np.float64, **({'weighted': 'sparse'} if kind == 'pattern' else {'sparse_x': True}))
        (e.upload_observed_csr if kind == 'pattern' else e.upload_X_csr)(sp.csr_matrix(X))
        return e
    return make


def _read_only(dtype):
    def make(n, d, k):
        X = np.random.RandomState(3).randint(0, 9, size=(n, d))
        e = engine(n, d, k, dtype=dtype)
        e.upload_X(X.astype(dtype))
        return e
    return make


FLAVOURS = {'weighted-dense': _weighted, 'pattern-only': _sparse('pattern'), 'csr-x': _sparse('csr'),
            'float16': _read_only(np.float16), 'uint8': _read_only(np.uint8)}


@pytest.mark.parametrize('k', REAL_K)
@pytest.mark.parametrize('flavour', sorted(FLAVOURS))
def test_the_call_does_not_care_about_the_flavour(flavour, k):
    W, T, excl = real_problem(k)
    e = FLAVOURS[flavour](W.shape[0], T.shape[1], k)
    try:
        e.set_W(W), e.set_T(T)
        j, v = e.topn_rows(None, 10, exclude=excl, clip=(None, 0.25 * k))
        tc.check_real(W, T, None, 10, excl, (None, 0.25 * k), j, v)
    finally:
        e.close()


def test_clip_repeatability_and_permuted_requests():
    W, T, excl = real_problem(20)
    e = factors_only(W, T)
    try:
        j0, v0 = e.topn_rows(None, 10, exclude=excl)
        lo, hi = float(np.nanpercentile(v0, 30)), float(np.nanpercentile(v0, 70))
        for clip in ((lo, hi), (None, hi), (lo, None), (float('nan'), hi)):
            j, v = e.topn_rows(None, 10, exclude=excl, clip=clip)
            assert np.array_equal(j, j0)                                    # ranked by the unclipped score
            assert np.array_equal(v, tc.clip_values(v0, clip), equal_nan=True)
        assert (tc.clip_values(v0, (lo, hi)) != v0).sum() > 100
        # twice the same call: the same bits
        j1, v1 = e.topn_rows(None, 10, exclude=excl)
        assert np.array_equal(j1, j0) and np.array_equal(v1.view(np.uint64), v0.view(np.uint64))
        # a permuted list with duplicates gives the permuted result, bit for bit
        rows = np.random.RandomState(0).randint(0, W.shape[0], size=150)
        jp, vp = e.topn_rows(rows, 10, exclude=excl[rows])
        assert np.array_equal(jp, j0[rows]) and np.array_equal(vp.view(np.uint64), v0[rows].view(np.uint64))
    finally:
        e.close()


@pytest.mark.parametrize('schedule', ['gram', 'residual'])
def test_no_state_of_a_run_is_disturbed(schedule):
    from rri_nmf_amd.engine import device_memory
    n, d, k = 50, 30, 3
    X = planted_X(n, d, k, seed=0, dtype=np.float32)
    W0, T0 = scaled_init(X.astype(np.float64), k, seed=1)
    rows = np.array([7, 3, 3, 49, 0], dtype=np.int64)
    excl = sp.csr_matrix(np.random.RandomState(1).rand(rows.size, d) < 0.3)

    def run(with_call):
        e = engine(n, d, k, dtype=np.float32, schedule=schedule)
        try:
            e.upload_X(X), e.set_W(W0), e.set_T(T0)
            e.set_params(reset_topic_method=None)
            if schedule == 'gram':
                assert e.onchip_info()[0], 'this shape takes the register-resident sweep'
            e.sweep(1)
            got = None
            if with_call:
                W1, T1 = e.get_W(), e.get_T()
                before = device_memory()
                got = e.topn_rows(rows, 4, exclude=excl, clip=(0.0, None))
                assert device_memory() == before
                tc.check_real(W1, T1, rows, 4, excl, (0.0, None), *got)
            e.sweep(1)
            obj = e.objective()
            if schedule == 'gram':
                assert e.onchip_info()[1] >= 2
            return e.get_W(), e.get_T(), obj
        finally:
            e.close()
    Wa, Ta, oa = run(False)
    Wb, Tb, ob = run(True)
    assert np.array_equal(Wa.view(np.uint64), Wb.view(np.uint64)) and np.array_equal(Ta.view(np.uint64), Tb.view(np.uint64))
    assert np.float64(oa).view(np.uint64) == np.float64(ob).view(np.uint64)


def test_refusals():
    from rri_nmf_amd import _capi
    W, T = tc.make_real(5, d=33, n=9)
    e = engine(9, 33, 5, dtype=np.float64)
    try:
        with pytest.raises(ValueError, match='W and T'):        # factors not set
            e.topn_rows(None, 3)
        e.set_W(W)
        with pytest.raises(ValueError, match='W and T'):
            e.topn_rows(None, 3)
        e.set_T(T)
        for n_top in (0, 65):
            with pytest.raises(NotImplementedError):
                e.topn_rows(None, n_top)
        for rows in ([0, 9], [-1]):
            with pytest.raises(ValueError, match='out of range'):
                e.topn_rows(rows, 3)
        with pytest.raises(ValueError):
            e.topn_rows([0, 1], 3, exclude=sp.csr_matrix((3, 33)))        # one row per requested row
        # raw exclusion arrays through the ABI: unsorted, repeated, out of range
        rows = np.array([2, 5], dtype=np.int64)
        idx, val = np.empty((2, 3), dtype=np.int32), np.empty((2, 3))

        def raw(indptr, indices):
            ip, ii = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32)
            return e._lib.rri_topn_rows(e._h, rows.ctypes.data_as(C.POINTER(C.c_int64)), 2, 3, ip.ctypes.data_as(C.POINTER(C.c_int64)),
                                        ii.ctypes.data_as(C.POINTER(C.c_int32)), float('nan'), float('nan'),
                                        idx.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_double)))
        assert raw([0, 2, 3], [1, 4, 0]) == _capi.RRI_OK
        tc.check_real(W, T, rows, 3, sp.csr_matrix((np.ones(3), [1, 4, 0], [0, 2, 3]), shape=(2, 33)), (None, None), idx, val)
        for indptr, indices in (([0, 2, 3], [4, 1, 0]), ([0, 2, 3], [1, 1, 0]), ([0, 2, 3], [1, 33, 0]), ([0, 2, 3], [-1, 4, 0]),
                                ([1, 2, 3], [1, 4, 0]), ([0, 3, 2], [1, 4, 0])):
            assert raw(indptr, indices) == _capi.RRI_ERR_INVALID, (indptr, indices)
        # no request: nothing to do, nothing touched
        assert e._lib.rri_topn_rows(e._h, None, 0, 3, None, None, 0.0, 1.0, None, None) == _capi.RRI_OK
        j, v = e.topn_rows([], 3)
        assert j.shape == (0, 3) and v.shape == (0, 3)
    finally:
        e.close()


def test_recommend_on_the_recommender_fixture():
    from rri_nmf_amd import sklearn_interface as si
    R = load_golden('g4_wrri')['X']
    n, d = R.shape
    E = si.NMF_RS_Estimator(n, d, 5, random_state=0, max_iter=5).fit_from_Xtr(R)
    assert np.array_equal(E.seen_.toarray() != 0, R != 0)
    clip = (E.min_rating, E.max_rating)
    items, scores = E.recommend()
    assert items.shape == (n, 10) and scores.shape == (n, 10)
    tc.check_real(E.W, E.T, None, 10, E.seen_, clip, items, scores)
    seen = E.seen_.toarray() != 0
    for i in range(n):
        assert not seen[i, items[i][items[i] >= 0]].any()
    ii, jj = np.nonzero(items >= 0)
    pred = E.predict(np.column_stack((ii, items[ii, jj])).astype(float))
    assert np.abs(pred - scores[ii, jj]).max() <= 2 * 5 * 2.0 ** -52 * (np.abs(E.W) @ np.abs(E.T)).max()
    users = np.array([3, 0, 3, n - 1])
    it_u, sc_u = E.recommend(users, n_items=3, exclude_seen=False)
    tc.check_real(E.W, E.T, users, 3, None, clip, it_u, sc_u)
