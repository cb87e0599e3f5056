"""Ranks of entries on the device (rri_rank_entries, RRIEngine.rank_entries, NMF_RS_Estimator.rank / ranking_score) against the
numpy restatement of tests/rank_cases.py.

Exact cases: W, T integers in 0..7 -- every sum is exact in any order and ties are everywhere -- so rank, val and eligible must
EQUAL the restatement: every geometry of topn_cases.EXACT_CASES with every kind of target list (none, one, 64 | 65 targets, every
column, targets inside the exclusion).  A case with NaN scores.  Real-valued cases at k = 5, 20, 200, 1024 with every open column
of every row a target: the rank must lie in the band that topn_cases.check_real's tolerance leaves, and the test first shows on
the restatement alone that the band is a single integer for every target, so the ranks must equal the restatement's.  Then the
property that ties the call to top-N (bit for bit), repeatability and permuted requests, handle flavours, that no state a sweep
reads is disturbed, refusals, and the estimator end to end on the recommender fixture."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import rank_cases as rc
import topn_cases as tc
from conftest import GOLDEN
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


def same(got, want):
    assert got.rank.dtype == np.int32 and got.val.dtype == np.float64 and got.eligible.dtype == np.int32
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.rank, want.rank), np.flatnonzero(got.rank != want.rank)[:5]
    assert np.array_equal(got.val, want.val, equal_nan=True)
    assert np.array_equal(got.eligible, want.eligible), np.flatnonzero(got.eligible != want.eligible)[:5]


def same_bits(a, b):
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    assert np.array_equal(a.rank, b.rank) and np.array_equal(a.eligible, b.eligible)
    assert np.array_equal(a.val.view(np.uint64), b.val.view(np.uint64))


@pytest.mark.parametrize('case', tc.EXACT_CASES, ids=[tc.case_id(c) for c in tc.EXACT_CASES])
def test_exact_cases_equal_the_restatement(case):
    W, T, rows, excl = tc.make_exact(case)
    e = factors_only(W, T)
    try:
        for n, kind in enumerate(rc.KINDS):
            targets = rc.make_targets(kind, case, excl, seed=n)
            before = (targets.indptr.copy(), targets.indices.copy())
            want = rc.rank_reference(W, T, rows, targets, excl)
            got = e.rank_entries(rows, targets, exclude=excl)
            if targets.nnz == 0:                        # nothing to rank: nothing is launched, nothing is counted
                assert got.rank.size == 0 and got.val.size == 0 and np.all(got.eligible == -1), kind
                continue
            same(got, want)
            sizes = np.diff(want.indptr)
            if kind == 'none':
                assert sizes[0] == 0
            if kind == 'edge' and case.d == 257:
                assert sizes[0] == 64 and (case.count == 1 or sizes[1] == 65)
            if kind == 'all':
                assert np.all(sizes == case.d)
            if kind == 'excluded' and case.excl in ('all', 'short'):
                assert (want.rank == -1).any() and np.isnan(want.val[want.rank == -1]).all()
            assert np.array_equal(targets.indptr, before[0]) and np.array_equal(targets.indices, before[1])     # sorted on a copy
    finally:
        e.close()


def test_nan_scores_are_not_eligible_not_counted_and_rank_minus_one():
    rng = np.random.RandomState(11)
    n, k, d = 37, 6, 131
    W = rng.randint(0, 4, size=(n, k)).astype(np.float64)
    T = rng.randint(0, 4, size=(k, d)).astype(np.float64)
    W[5, 2] = np.nan                                    # a whole row of NaN scores
    T[3, 70] = np.inf                                   # a column of +inf ... and NaN where W holds a 0 at that topic
    W[:, 3] = rng.randint(0, 2, size=n)
    W[5, 3] = 1.0
    S = W @ T
    assert np.isnan(S[5]).all() and np.isnan(S[:, 70]).sum() > 5 and np.isinf(S[:, 70]).sum() > 5
    excl = sp.csr_matrix(rng.rand(n, d) < 0.2)
    targets = sp.csr_matrix(rng.rand(n, d) < 0.3)
    targets = (targets + sp.csr_matrix((np.ones(n), (np.arange(n), np.full(n, 70))), shape=(n, d))).tocsr()
    e = factors_only(W, T)
    try:
        for ex in (None, excl):
            want = rc.rank_reference(W, T, None, targets, ex)
            assert want.eligible[5] == 0 and (want.rank == -1).sum() > 10 and (want.rank == 0).sum() > 5
            same(e.rank_entries(None, targets, exclude=ex), want)
    finally:
        e.close()


REAL_K = (5, 20, 200, 1024)
_real = {}


def real_problem(k):
    """W, T, the `short` exclusion, and per exclusion (None | short) the targets -- every open column of every row -- with the
    restatement's ranks and bands; computed once per k"""
    if k not in _real:
        W, T = tc.make_real(k)
        excl = tc.make_exclusion('short', W.shape[0], T.shape[1], 10, seed=k)
        per = []
        for ex in (None, excl):
            targets = sp.csr_matrix(~tc.exclusion_mask(ex, W.shape[0], T.shape[1]))
            per.append((ex, targets) + rc.rank_bands(W, T, None, targets, ex))
        _real[k] = (W, T, excl, per)
    return _real[k]


def check_real(got, ref, lo, hi, tol, clip=(None, None)):
    assert np.array_equal(lo, hi), 'the band of %d targets is wider than one integer' % np.count_nonzero(lo != hi)
    assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
    assert np.all(got.rank >= lo) and np.all(got.rank <= hi), np.flatnonzero((got.rank < lo) | (got.rank > hi))[:5]
    assert np.array_equal(got.rank, ref.rank)           # what a single-integer band comes to
    err = np.abs(got.val - tc.clip_values(ref.val, clip))
    assert np.all(err <= tol), (err.max(), tol.min())
    assert np.array_equal(got.eligible, ref.eligible)
    return float((err / tol).max())


@pytest.mark.parametrize('k', REAL_K)
def test_real_valued_cases_within_the_rounding_of_two_sums(k):
    W, T, _, per = real_problem(k)
    e = factors_only(W, T)
    try:
        for ex, targets, ref, lo, hi, tol in per:
            assert ref.indices.size > 11000 and np.all(ref.rank >= 0)
            worst = check_real(e.rank_entries(None, targets, exclude=ex), ref, lo, hi, tol)
            print('k = %d, %s: %d targets, largest value difference / tolerance %.3f'
                  % (k, 'exclusion' if ex is not None else 'no exclusion', ref.indices.size, worst))
    finally:
        e.close()


def slots_as_targets(idx, d):
    q, p = np.nonzero(idx >= 0)
    return sp.csr_matrix((np.ones(q.size), (q, idx[q, p])), shape=(idx.shape[0], d)), q, p


@pytest.mark.parametrize('k', [20, 200])
def test_the_column_in_slot_p_of_a_top_n_list_has_rank_p_and_the_same_bits(k):
    W, T, excl, _ = real_problem(k)
    rows = np.random.RandomState(k).randint(0, W.shape[0], size=70)
    e = factors_only(W, T)
    try:
        for n_top in (1, 10, 64):
            for r, ex in ((None, excl), (rows, excl[rows]), (None, None)):
                idx, val = e.topn_rows(r, n_top, exclude=ex, clip=(None, 0.26 * k))
                targets, q, p = slots_as_targets(idx, T.shape[1])
                got = e.rank_entries(r, targets, exclude=ex, clip=(None, 0.26 * k))
                pos = np.array([got.indptr[a] + np.searchsorted(got.indices[got.indptr[a]:got.indptr[a + 1]], idx[a, b])
                                for a, b in zip(q, p)], dtype=np.int64)
                assert np.array_equal(got.indices[pos], idx[q, p])
                assert np.array_equal(got.rank[pos], p), (n_top, np.flatnonzero(got.rank[pos] != p)[:5])
                assert np.array_equal(got.val[pos].view(np.uint64), val[q, p].view(np.uint64))
                short = (idx < 0).any(axis=1)           # a list that is not full holds every eligible column
                assert np.array_equal(got.eligible[short], (idx[short] >= 0).sum(axis=1)) and np.all(got.eligible[~short] >= n_top)
    finally:
        e.close()


def test_the_top_n_property_on_exact_factors_with_ties():
    case = tc.Case(5, 257, 130, 64, 'short', None)
    W, T, rows, excl = tc.make_exact(case)
    e = factors_only(W, T)
    try:
        idx, val = e.topn_rows(rows, 64, exclude=excl)
        targets, q, p = slots_as_targets(idx, case.d)
        got = e.rank_entries(rows, targets, exclude=excl)
        dense = np.full((case.count, case.d), -9, dtype=np.int64)
        dense[np.repeat(np.arange(case.count), np.diff(got.indptr)), got.indices] = got.rank
        assert np.array_equal(dense[q, idx[q, p]], p)
    finally:
        e.close()


def test_repeatability_permuted_requests_and_clip():
    W, T, excl, per = real_problem(20)
    _, targets, ref, lo, hi, tol = per[1]
    e = factors_only(W, T)
    try:
        a = e.rank_entries(None, targets, exclude=excl)
        same_bits(e.rank_entries(None, targets, exclude=excl), a)               # twice the same call: the same bits
        rows = np.random.RandomState(0).randint(0, W.shape[0], size=150)        # a permuted list with duplicates
        b = e.rank_entries(rows, targets[rows], exclude=excl[rows])
        assert np.array_equal(np.diff(b.indptr), np.diff(a.indptr)[rows]) and np.array_equal(b.eligible, a.eligible[rows])
        for n, r in enumerate(rows):
            sa, sb = slice(a.indptr[r], a.indptr[r + 1]), slice(b.indptr[n], b.indptr[n + 1])
            assert np.array_equal(b.indices[sb], a.indices[sa]) and np.array_equal(b.rank[sb], a.rank[sa])
            assert np.array_equal(b.val[sb].view(np.uint64), a.val[sa].view(np.uint64))
        lo_c, hi_c = float(np.percentile(a.val, 30)), float(np.percentile(a.val, 70))
        for clip in ((lo_c, hi_c), (None, hi_c), (lo_c, None), (float('nan'), hi_c)):
            c = e.rank_entries(None, targets, exclude=excl, clip=clip)
            assert np.array_equal(c.rank, a.rank) and np.array_equal(c.eligible, a.eligible)       # ranked by the unclipped score
            assert np.array_equal(c.val, tc.clip_values(a.val, clip))
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
_plain = {}


@pytest.mark.parametrize('k', [20, 200])
@pytest.mark.parametrize('flavour', sorted(FLAVOURS))
def test_the_call_does_not_care_about_the_flavour(flavour, k):
    W, T, excl, per = real_problem(k)
    _, targets, ref, lo, hi, tol = per[1]
    clip = (None, 0.25 * k)
    if k not in _plain:                                 # the answer of a factors-only handle, once
        p = factors_only(W, T)
        try:
            _plain[k] = p.rank_entries(None, targets, exclude=excl, clip=clip)
        finally:
            p.close()
    e = FLAVOURS[flavour](W.shape[0], T.shape[1], k)
    try:
        e.set_W(W), e.set_T(T)
        got = e.rank_entries(None, targets, exclude=excl, clip=clip)
    finally:
        e.close()
    check_real(got, ref, lo, hi, tol, clip)
    same_bits(got, _plain[k])


@pytest.mark.parametrize('schedule', ['gram', 'residual'])
def test_no_state_of_a_run_is_disturbed(schedule):
    from rri_nmf_amd.engine import device_memory
    n, d, k = 50, 30, 3
    X = planted_X(n, d, k, seed=0, dtype=np.float32)
    W0, T0 = scaled_init(X.astype(np.float64), k, seed=1)
    rows = np.array([7, 3, 3, 49, 0], dtype=np.int64)
    excl = sp.csr_matrix(np.random.RandomState(1).rand(rows.size, d) < 0.3)
    targets = sp.csr_matrix(np.random.RandomState(2).rand(rows.size, d) < 0.4)

    def run(with_call):
        e = engine(n, d, k, dtype=np.float32, schedule=schedule)
        try:
            e.upload_X(X), e.set_W(W0), e.set_T(T0)
            e.set_params(reset_topic_method=None)
            if schedule == 'gram':
                assert e.onchip_info()[0], 'this shape takes the register-resident sweep'
            e.sweep(1)
            if with_call:
                W1, T1 = e.get_W(), e.get_T()
                before = device_memory()
                got = e.rank_entries(rows, targets, exclude=excl, clip=(0.0, None))
                assert device_memory() == before
                ref, lo, hi, tol = rc.rank_bands(W1, T1, rows, targets, excl)
                assert np.all(got.rank >= lo) and np.all(got.rank <= hi) and np.array_equal(got.eligible, ref.eligible)
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
    one = sp.csr_matrix(([1.0], ([0], [4])), shape=(9, 33))
    e = engine(9, 33, 5, dtype=np.float64)
    try:
        with pytest.raises(ValueError, match='W and T'):        # factors not set
            e.rank_entries(None, one)
        e.set_W(W)
        with pytest.raises(ValueError, match='W and T'):
            e.rank_entries(None, one)
        e.set_T(T)
        for rows in ([0, 9], [-1, 0]):
            with pytest.raises(ValueError, match='out of range'):
                e.rank_entries(rows, one[:2])
        with pytest.raises(ValueError, match='targets'):
            e.rank_entries([0, 1], sp.csr_matrix((3, 33)))                    # one row per requested row
        with pytest.raises(ValueError, match='targets'):
            e.rank_entries([0, 1], sp.csr_matrix((2, 34)))
        with pytest.raises(ValueError, match='exclude'):
            e.rank_entries([0, 1], one[:2], exclude=sp.csr_matrix((3, 33)))
        # raw target arrays through the ABI: unsorted, repeated, out of range, no indptr
        rows = np.array([2, 5], dtype=np.int64)
        rank, val, elig = np.empty(3, dtype=np.int32), np.empty(3), np.empty(2, dtype=np.int32)
        I64P, I32P, DP = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)

        def raw(indptr, indices, elig_out=elig):
            ip = None if indptr is None else np.asarray(indptr, dtype=np.int64)
            ii = np.asarray(indices, dtype=np.int32)
            return e._lib.rri_rank_entries(e._h, rows.ctypes.data_as(I64P), 2, None if ip is None else ip.ctypes.data_as(I64P),
                                           ii.ctypes.data_as(I32P), None, None, float('nan'), float('nan'), rank.ctypes.data_as(I32P),
                                           val.ctypes.data_as(DP), None if elig_out is None else elig_out.ctypes.data_as(I32P))
        want = rc.rank_reference(W, T, rows, sp.csr_matrix((np.ones(3), [1, 4, 0], [0, 2, 3]), shape=(2, 33)), None)
        assert raw([0, 2, 3], [1, 4, 0]) == _capi.RRI_OK
        assert np.array_equal(rank, want.rank) and np.array_equal(elig, want.eligible) and np.all(elig == 33)
        rank[:] = -5
        assert raw([0, 2, 3], [1, 4, 0], elig_out=None) == _capi.RRI_OK and np.array_equal(rank, want.rank)     # eligible_out may be NULL
        for indptr, indices in (([0, 2, 3], [4, 1, 0]), ([0, 2, 3], [1, 1, 0]), ([0, 2, 3], [1, 33, 0]), ([0, 2, 3], [-1, 4, 0]),
                                ([1, 2, 3], [1, 4, 0]), ([0, 3, 2], [1, 4, 0]), (None, [1, 4, 0])):
            assert raw(indptr, indices) == _capi.RRI_ERR_INVALID, (indptr, indices)
        # no request, or no target: nothing to do, nothing touched
        zero = np.zeros(3, dtype=np.int64)
        assert e._lib.rri_rank_entries(e._h, None, 0, zero.ctypes.data_as(I64P), None, None, None, 0.0, 1.0, None, None, None) == _capi.RRI_OK
        assert e._lib.rri_rank_entries(e._h, None, 2, zero.ctypes.data_as(I64P), None, None, None, 0.0, 1.0, None, None, None) == _capi.RRI_OK
        got = e.rank_entries([], sp.csr_matrix((0, 33)))
        assert got.rank.shape == (0,) and got.val.shape == (0,) and got.eligible.shape == (0,) and got.indptr.tolist() == [0]
    finally:
        e.close()


def test_ranking_score_on_the_recommender_fixture():
    from rri_nmf_amd import sklearn_interface as si
    train = sp.load_npz(os.path.join(GOLDEN, 'ref_data', 'recsys_data_train.npz')).tocsr()
    test = sp.load_npz(os.path.join(GOLDEN, 'ref_data', 'recsys_data_test.npz')).tocsr()
    n, d = train.shape
    E = si.NMF_RS_Estimator(n, d, 5, random_state=0, max_iter=5).fit_from_Xtr(train)
    ti, tj = test.nonzero()
    A = sp.csr_matrix((np.ones(ti.size), (ti, tj)), shape=(n, d))
    ref, lo, hi, _ = rc.rank_bands(E.W, E.T, None, A, E.seen_)
    print('%d held-out pairs, %d with a band wider than one integer' % (ti.size, np.count_nonzero(lo != hi)))
    rank, elig = E.rank(test)
    dense = np.full((n, d), -7, dtype=np.int64)
    dense[np.repeat(np.arange(n), np.diff(ref.indptr)), ref.indices] = np.arange(ref.indices.size)
    pos = dense[ti, tj]
    assert rank.shape == (ti.size,) and np.all(rank >= lo[pos]) and np.all(rank <= hi[pos])
    assert np.array_equal(elig, ref.eligible[ti]) and np.array_equal(elig, d - np.diff(E.seen_.indptr)[ti])
    for n_items, rel in ((10, None), (100, None), (10, 4.0)):
        got = E.ranking_score(test, n_items=n_items, relevant_from=rel)
        keep = np.ones(ti.size, dtype=bool) if rel is None else np.asarray(test[ti, tj]).ravel() >= rel
        # the restatement's metrics from the device's ranks (equal to the restatement's wherever the band is one integer)
        want = rc.metrics_reference(ti[keep], rank[keep], elig[keep], n_items)
        assert set(got) == set(want)
        for name in want:
            assert got[name] == pytest.approx(want[name], rel=1e-13, abs=0), (name, n_items, rel)
        if np.array_equal(lo, hi):
            full = rc.metrics_reference(ti[keep], ref.rank[pos][keep], ref.eligible[ti][keep], n_items)
            assert all(got[name] == pytest.approx(full[name], rel=1e-13, abs=0) for name in full)
        assert got['targets'] == keep.sum() and got['targets_not_eligible'] == 0 and 0.0 <= got['auc'] <= 1.0
    # a pair of the training set is in seen_: not eligible
    both = sp.vstack([test[:1], train[1:2], sp.csr_matrix((n - 2, d))]).tocsr()
    more = E.ranking_score(both, n_items=10)
    assert more['targets_not_eligible'] == train[1:2].nnz and more['targets'] == test[:1].nnz + train[1:2].nnz
