"""The log-likelihood of stored counts on the device (rri_entries_loglik, RRIEngine.entries_loglik, NMF_TM_Estimator.log_likelihood
and perplexity) against the numpy restatement (tests/loglik_cases.py).

The bound, derived and not measured, with u = 2^-52 and L_q the length of a request's segment:
    |ll_q - want_q| <= u [2 (k + 2) mass_q + (L_q + 4) sum_e v_e |log p~_e|]
(lc.reference returns it per request); mass is equal for integer values and within L_q u mass_q for real ones; the floored count
is compared where no reference p lies within 1e-9 relative of the floor, which the test asserts of its inputs first.

Shapes are the smallest at which the kernels can go wrong: k on both sides of the border 128 | 129 of loglik_lanes (and of 16 | 17,
where a border was first proposed), k = 1, 2, 3 (the zero pad of the transposed T), 50 and RRI_MAX_K; segments of 0, 1, G - 1, G,
G + 1 entries for each instantiation's G = 64 / lanes groups (16 and 4) and around LL_SEG; 1, 63, 64, 65 and 257 requests; d = 1
and a full row of d = 300; and the one size at which a second chunk appears: 1366 full requests of 4096 columns."""
import numpy as np
import pytest
import scipy.sparse as sp

import loglik_cases as lc
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu

S = lc.LL_SEG


@pytest.fixture(scope='module')
def handles():
    """factors-only handles by (n, d, k, seed, kind), made on first use and closed with the module"""
    from rri_nmf_amd.engine import RRIEngine
    made = {}

    def get(n, d, k, seed=0, kind='uniform'):
        key = (n, d, k, seed, kind)
        if key not in made:
            W, T = lc.disjoint_factors(n, d, k, seed) if kind == 'disjoint' else lc.factors(n, d, k, seed, simplex=kind == 'simplex')
            e = RRIEngine(n, d, k, dtype=np.float64)
            e.set_W(W), e.set_T(T)
            made[key] = (e, W, T)
        return made[key]
    yield get
    for e, _, _ in made.values():
        e.close()


def check(h, rows, A, floor=1e-12):
    e, W, T = h
    got = e.entries_loglik(rows, A, floor)
    ll, mass, floored, p, bound = lc.reference(W, T, rows, A, floor)
    m = sp.csr_matrix(A).shape[0]
    assert [x.dtype for x in got] == [np.float64, np.float64, np.int64] and all(x.shape == (m,) for x in got)
    assert lc.floor_is_comparable(p, floor)
    assert np.array_equal(got[2], floored), np.flatnonzero(got[2] != floored)[:5]
    fin = np.isfinite(ll)
    assert np.array_equal(np.isnan(got[0]), np.isnan(ll)) and np.array_equal(got[0][~fin & ~np.isnan(ll)], ll[~fin & ~np.isnan(ll)])
    err = np.abs(got[0][fin] - ll[fin])
    assert np.all(err <= bound[fin]), (np.flatnonzero(err > bound[fin])[:5], err.max(), bound[fin].max())
    data = sp.csr_matrix(A).data
    if np.all(data == np.floor(data)):
        assert np.array_equal(got[1], mass)
    else:
        assert np.all(np.abs(got[1] - mass) <= np.diff(sp.csr_matrix(A).indptr) * lc.U * mass)
    return got


def around(G, d):
    """segment lengths around a lane-group count: none, one, G - 1, G, G + 1, and the full row"""
    return sorted({L for L in (0, 1, G - 1, G, G + 1, d) if 0 <= L <= d})


@pytest.mark.parametrize('k', [1, 2, 3, 16, 17, 50, 128, 129, 1024])
def test_topic_counts_on_both_sides_of_every_border_of_the_lane_rule(handles, k):
    from rri_nmf_amd import _capi
    assert _capi.RRI_MAX_K == 1024 and [lc.lanes(x) for x in (16, 17, 128, 129, 1024)] == [4, 4, 4, 16, 16]
    n, d = 12, 33
    h = handles(n, d, k)
    lengths = (around(64 // lc.lanes(k), d) * 3)[:n]
    for integer in (True, False):
        ll, mass, _ = check(h, None, lc.segments(lengths, d, seed=k, integer=integer, zeros=0.1))
        assert np.all(mass[np.array(lengths) == d] > 0) and np.all(np.isfinite(ll))


@pytest.mark.parametrize('k', [128, 129], ids=['16-groups', '4-groups'])
def test_segment_lengths_around_the_group_count_and_the_piece(handles, k):
    G = 64 // lc.lanes(k)
    n, d = 10, 600
    h = handles(n, d, k)
    lengths = [0, 1, G - 1, G, G + 1, S - 1, S, S + 1, 2 * S + 3, 0]
    check(h, None, lc.segments(lengths, d, seed=1))
    check(h, None, lc.segments(lengths[::-1], d, seed=2, integer=False, zeros=0.05))
    # one column, and a full row of 300
    h1 = handles(5, 1, k)
    check(h1, None, lc.segments([1, 0, 1, 1, 0], 1, seed=3))
    h300 = handles(3, 300, k)
    ll, mass, _ = check(h300, None, lc.segments([300, 0, 300], 300, seed=4))
    assert mass[1] == 0 and ll[1] == 0


@pytest.mark.parametrize('count', [1, 63, 64, 65, 257])
def test_request_counts_around_the_workgroup_and_the_sum_kernel(handles, count):
    n, d, k = 257, 40, 5
    h = handles(n, d, k)
    lengths = list(np.random.RandomState(count).randint(0, 41, size=count))
    lengths[-1] = 40                                      # the last request counts
    A = lc.segments(lengths, d, seed=count)
    got = check(h, None if count == n else np.arange(count), A)
    assert got[1][-1] > 0


def test_rows_permuted_and_a_row_listed_three_times_with_different_segments(handles):
    n, d, k = 20, 50, 50
    h = handles(n, d, k)
    rows = np.random.RandomState(0).permutation(n)
    A = lc.segments(list(np.random.RandomState(1).randint(0, 51, size=n)), d, seed=5)
    by_row = check(h, rows, A)
    plain = check(h, None, A[np.argsort(rows)])           # the same pairs of row and segment, in row order
    assert all(np.array_equal(a, b[rows]) for a, b in zip(by_row, plain))
    three = check(h, [7, 3, 7, 7], lc.segments([10, 50, 0, 37], d, seed=6))
    assert three[1][2] == 0 and len({three[0][0], three[0][2], three[0][3]}) == 3


def test_exact_zeros_are_floored_or_minus_infinity_and_an_explicit_zero_adds_nothing(handles):
    n, d, k = 8, 40, 6
    h = handles(n, d, k, kind='disjoint')
    A = lc.segments([40, 40, 7, 0, 40, 13, 40, 40], d, seed=7)
    p, req = lc.entry_p(h[1], h[2], None, A)
    same_parity = (req % 2) == (A.indices % 2)
    assert np.all(p[same_parity] == 0) and np.all(p[~same_parity] > 1e-6) and same_parity.sum() > 50
    ll, mass, floored = check(h, None, A, floor=1e-12)
    assert np.array_equal(floored, np.bincount(req[same_parity], minlength=n)) and np.all(np.isfinite(ll))
    ll0, mass0, floored0 = check(h, None, A, floor=0.0)
    assert not floored0.any() and np.array_equal(np.isneginf(ll0), floored > 0) and floored[0] > 0 and np.array_equal(mass0, mass)
    # explicit zeros at every entry whose p is 0: the terms are 0, not NaN, and the rest is finite
    Z = A.copy()
    Z.data[same_parity] = 0.0
    llz, _, flz = check(h, None, Z, floor=0.0)
    assert np.all(np.isfinite(llz)) and not flz.any() and Z.nnz == A.nnz
    assert not check(h, None, Z, floor=1e-12)[2].any()          # a zero count is never floored


def test_a_nan_in_one_row_of_w_stays_in_that_request_alone():
    from rri_nmf_amd.engine import RRIEngine
    n, d, k = 9, 33, 17
    W, T = lc.factors(n, d, k, seed=8)
    A = lc.segments([33, 5, 0, 20, 33, 1, 4, 17, 9], d, seed=8)
    Wn = W.copy()
    Wn[4, 11] = np.nan
    with RRIEngine(n, d, k, dtype=np.float64) as e:
        e.set_W(W), e.set_T(T)
        clean = check((e, W, T), None, A)
        e.set_W(Wn)
        dirty = check((e, Wn, T), None, A)
    assert np.isnan(dirty[0][4]) and dirty[1][4] == clean[1][4] and dirty[2][4] == 0
    others = np.arange(n) != 4
    assert np.array_equal(dirty[0][others].view(np.uint64), clean[0][others].view(np.uint64))


def test_a_request_alone_among_others_and_twice_gives_the_same_bits(handles):
    n, d, k = 65, 600, 50
    h = handles(n, d, k)
    lengths = list(np.random.RandomState(3).randint(0, 120, size=n))
    lengths[17] = 2 * S + 3                              # three pieces
    lengths[1] = 5
    A = lc.segments(lengths, d, seed=9, integer=False, zeros=0.05)
    A.indices[A.indptr[1]:A.indptr[2]] = A.indices[A.indptr[1]:A.indptr[2]][::-1].copy()          # an unsorted row
    A.data[A.indptr[1]:A.indptr[2]] = A.data[A.indptr[1]:A.indptr[2]][::-1].copy()
    A.has_sorted_indices = False
    A.has_canonical_format = False
    keep = (A.indptr.copy(), A.indices.copy(), A.data.copy())
    C = A.copy()
    C.sort_indices()
    among = check(h, None, C)
    again = h[0].entries_loglik(None, A, 1e-12)                # the caller's unsorted matrix
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(among, again))
    assert all(np.array_equal(x, y) for x, y in zip(keep, (A.indptr, A.indices, A.data)))
    for q in (0, 17, 64):
        alone = h[0].entries_loglik([q], C[q], 1e-12)
        assert all(a.view(np.uint64)[0] == b.view(np.uint64)[q] for a, b in zip(alone, among)), q
    # other dtypes and formats of the same matrix: converted on copies
    other = h[0].entries_loglik(None, sp.coo_matrix(C.astype(np.float32).astype(np.float64)), 1e-12)
    f32 = h[0].entries_loglik(None, C.astype(np.float32), 1e-12)
    assert all(np.array_equal(a, b) for a, b in zip(other, f32))


def test_the_smallest_call_with_a_second_chunk_and_a_call_without_entries(handles):
    """64 MiB at 12 bytes per entry are 5592405 entries: 1365 full requests of 4096 columns, so request 1365 is the second chunk"""
    n, d, k = 1366, 4096, 2
    assert (64 << 20) // 12 // d == n - 1
    h = handles(n, d, k, kind='simplex')
    e = h[0]
    counts = np.random.RandomState(10).randint(1, 4, size=(n, d)).astype(np.float64)
    A = sp.csr_matrix(counts)
    assert A.nnz == n * d
    e.timing_enable(True)
    e.timing_read(7)
    ll, mass, floored = check(h, None, A)
    assert e.timing_read(7)[0] == 5                          # the transposed copy of T, then two launches per chunk, two chunks
    assert np.array_equal(mass, counts.sum(axis=1)) and not floored.any() and np.all(ll < 0)
    one = e.entries_loglik(None, sp.vstack([A[:n - 1], sp.csr_matrix((1, d))]).tocsr(), 1e-12)       # one chunk: the last request is empty
    assert e.timing_read(7)[0] == 3 and one[1][-1] == 0 and one[0][-1] == 0
    assert np.array_equal(one[0][:-1].view(np.uint64), ll[:-1].view(np.uint64))     # the cut into chunks changes no bits
    for empty in (sp.csr_matrix((n, d)), sp.csr_matrix((0, d))):
        got = e.entries_loglik(None if empty.shape[0] else [], empty, 1e-12)
        assert all(not x.any() and x.shape == (empty.shape[0],) for x in got)
    assert e.timing_read(7)[0] == 0
    e.timing_enable(False)


def test_refusals_through_the_engine():
    from rri_nmf_amd.engine import RRIEngine
    n, d, k = 4, 6, 3
    W, T = lc.factors(n, d, k, seed=11)
    A = lc.segments([2, 0, 6, 1], d, seed=11)
    with RRIEngine(n, d, k, dtype=np.float64) as e:
        with pytest.raises(ValueError, match='W and T must be set first'):
            e.entries_loglik(None, A, 1e-12)
        e.set_W(W)
        with pytest.raises(ValueError, match='W and T must be set first'):
            e.entries_loglik(None, A, 1e-12)
        e.set_T(T)
        check((e, W, T), None, A)
        neg = A.copy()
        neg.data[1] = -1.0
        with pytest.raises(ValueError, match='value -1 at entry 1 of request 0'):
            e.entries_loglik(None, neg, 1e-12)
        for bad in (float('nan'), float('inf'), -1.0):
            with pytest.raises(ValueError, match='floor'):
                e.entries_loglik(None, A, bad)
        with pytest.raises(ValueError, match='one row per requested row'):
            e.entries_loglik([0, 1], A, 1e-12)
        with pytest.raises(ValueError, match=r'rows\[1\] = 4 is out of range'):
            e.entries_loglik([0, 4, 1, 2], A, 1e-12)
        # a column twice: the engine sums duplicates of a matrix that says it is not canonical; the library refuses the raw arrays
        twice = sp.csr_matrix((np.array([1.0, 2.0]), np.array([3, 3], dtype=np.int32), np.array([0, 2, 2, 2, 2])), shape=(n, d))
        summed = e.entries_loglik(None, twice, 1e-12)
        assert summed[1].tolist() == [3.0, 0.0, 0.0, 0.0]
        import ctypes as C
        I64P, I32P, DP = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
        ptr, ind, val = np.array([0, 2], dtype=np.int64), np.array([3, 3], dtype=np.int32), np.array([1.0, 2.0])
        out, fl = np.zeros(1), np.zeros(1, dtype=np.int64)
        st = e._lib.rri_entries_loglik(e._h, None, 1, ptr.ctypes.data_as(I64P), ind.ctypes.data_as(I32P), val.ctypes.data_as(DP), 1e-12,
                                       out.ctypes.data_as(DP), out.ctypes.data_as(DP), fl.ctypes.data_as(I64P))
        from rri_nmf_amd import _capi
        assert st == _capi.RRI_ERR_INVALID and 'do not ascend strictly' in e._err()


@pytest.mark.parametrize('flavour', ['float32-dense', 'csr-x', 'weighted'])
def test_every_flavour_answers_and_no_state_of_a_run_is_disturbed(flavour):
    from rri_nmf_amd.engine import RRIEngine, device_memory
    n, d, k = 50, 30, 3
    X = planted_X(n, d, k, seed=0, dtype=np.float64)
    X = X * (np.random.RandomState(4).rand(n, d) < 0.5)
    X[:, 0] = X.max()                                # no empty row
    W0, T0 = scaled_init(X, k, seed=1)
    A = lc.segments(list(np.random.RandomState(2).randint(0, 31, size=n)), d, seed=12)

    def run(with_call):
        if flavour == 'float32-dense':
            e = RRIEngine(n, d, k, dtype=np.float32)
            e.upload_X(X.astype(np.float32))
        elif flavour == 'csr-x':
            e = RRIEngine(n, d, k, dtype=np.float64, sparse_x=True)
            e.upload_X_csr(sp.csr_matrix(X))
        else:
            e = RRIEngine(n, d, k, dtype=np.float64, weighted=True)
            e.upload_X(X), e.upload_mask((np.random.RandomState(5).rand(n, d) < 0.6).astype(np.float64))
        try:
            e.set_W(W0), e.set_T(T0)
            e.set_params(reset_topic_method=None)
            e.sweep(1)
            if with_call:
                before = device_memory()
                e.timing_enable(True)
                got = check((e, e.get_W(), e.get_T()), None, A)
                assert e.timing_read(7)[0] == 3 and e.timing_read(7)[0] == 0
                e.timing_enable(False)
                assert device_memory() == before
                assert got[1].sum() > 0
            e.sweep(1)
            return e.get_W(), e.get_T(), e.objective()
        finally:
            e.close()
    Wa, Ta, oa = run(False)
    Wb, Tb, ob = run(True)
    assert np.array_equal(Wa.view(np.uint64), Wb.view(np.uint64)) and np.array_equal(Ta.view(np.uint64), Tb.view(np.uint64))
    assert np.float64(oa).view(np.uint64) == np.float64(ob).view(np.uint64)


def test_log_likelihood_and_perplexity_of_the_fixture_end_to_end():
    import os
    from rri_nmf_amd import sklearn_interface as si
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g1_tm_estimator.npz'))
    X, Xte, W, T, Wte = z['X'], z['Xte'], z['W_s10'], z['T_s10'], z['Wte']
    n, d, k = X.shape[0], X.shape[1], T.shape[0]
    E = si.NMF_TM_Estimator(n, d, k, W=W, T=T)
    for data, Wd in ((X, W), (Xte, Wte)):
        A = sp.csr_matrix(data)
        Z = Wd.dot(T.sum(axis=1))
        assert np.all(np.abs(Z - 1) < 1e-12)                     # the model is proper: every row of W T is a distribution
        ll, mass, floored, p, bound = lc.reference(Wd / Z[:, None], T, None, A, 1e-12)
        assert lc.floor_is_comparable(p, 1e-12) and p[p > 0].min() > 1e-5
        for corpus in (A, data):
            got = E.log_likelihood(corpus, W=Wd)
            assert got['documents'] == data.shape[0] and got['floor'] == 1e-12
            assert np.all(np.abs(got['per_document'] - ll) <= bound)
            assert np.all(np.abs(got['tokens'] - mass) <= np.diff(A.indptr) * lc.U * mass)
            assert np.array_equal(got['floored'], floored) and got['floored'].sum() == 1      # one entry whose p is exactly 0
            assert abs(got['log_likelihood'] - ll.sum()) <= bound.sum() + lc.U * data.shape[0] * np.abs(ll).sum()
            assert got['per_token'] == got['log_likelihood'] / got['tokens'].sum()
            assert got['perplexity'] == np.exp(-got['per_token']) and got['perplexity'] < d   # d: the uniform model
    # W=None runs the fold-in; document completion folds in on one part and scores the other
    ppl = E.perplexity(Xte)
    assert isinstance(ppl, float) and np.isfinite(ppl) and ppl < d
    counts = sp.csr_matrix(np.round(40 * Xte))
    observed, held = si.split_counts(counts, held_out=0.5, random_state=0)
    done = E.perplexity(held, observed=observed)
    assert np.isfinite(done) and 1 < done
