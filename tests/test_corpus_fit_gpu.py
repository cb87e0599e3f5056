"""The recommender fit from a resident corpus on the GPU (include/rri_corpus_fit.h): the store of a pattern-only handle built on the
device from a corpus (rri_upload_observed_corpus) against the one the host builds (rri_upload_observed_csr); the clipped
prediction error at the entries of a corpus (rri_corpus_entries_error) against the numpy restatement of tests/fiterr_cases.py
within its bounds, and its bit-equality rules; the value range; nmf(corpus, observed_only=True) against nmf(A, W_mat=pattern,
sparse_pattern=True); NMF_RS_Estimator.fit_corpus / score_corpus against fit_from_Xtr / score.

Store equality is equality of every field and every array, values compared as bits.  Fit equality is equality of bits of W and T
wherever both routes start from the same factors and take the same stop decisions: the sweeps read the same bytes.  The default
start is compared with device_init=True on the host route: nmf() takes scikit-learn's SVD on the host below 2e7 entries unless
told otherwise, while a corpus is always started through the handle's products -- the same algorithm, other roundings."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

import fiterr_cases as fc
import spbuild_cases as sc
import wsb_cases as wc
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
K = 5
INF = float('inf')
FIELDS = ('nblk', 'bw', 'nseg', 'gdim', 'count', 'nwork', 'lps', 'nnz', 'longest_row')       # info fields 0 .. 8
ARRAYS = ('segptr', 'idx', 'perm', 'work')


def lib():
    from rri_nmf_amd import engine
    return engine


def cf():
    from rri_nmf_amd import corpus_fit
    return corpus_fit


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_store(a, b):
    for f in FIELDS:
        assert a[f] == b[f], f
    for f in ARRAYS:
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), f
    assert a['val'].dtype == b['val'].dtype and np.array_equal(bits(a['val']), bits(b['val'])), 'val'


def factors(n, d, k=K, seed=0):
    rng = np.random.RandomState(seed)
    return 0.1 + rng.rand(n, k), 0.1 + rng.rand(k, d)


# ---- the store -----------------------------------------------------------------------------------------------------------------------
# every case of the CSR-X builder, and two patterns that a pattern-only handle cuts into more than one block per copy (its blocks
# hold three factor tables: 5120 float64 or 10240 float32 rows or columns)
STORE_CASES = sc.cases() + [('12000x150', lambda: wc.pat_density(12000, 150, 0.02, seed=31)),
                            ('300x11000', lambda: wc.pat_density(300, 11000, 0.02, seed=32))]


def routes(A, dtype, sweeps=0):
    """per route (host arrays, corpus): the two blocked copies, and W, T and the objective after `sweeps` sweeps from given factors,
    the corpus closed before the first one"""
    E = lib()
    n, d = A.shape
    out = []
    for route in ('csr', 'corpus'):
        with E.RRIEngine(n, d, K, dtype=dtype, weighted='sparse') as eng:
            corpus = E.DeviceCorpus(A)
            try:
                assert corpus.nnz == A.nnz and corpus.rows_rewritten == 0
                if route == 'csr':
                    eng.upload_observed_csr(corpus.to_scipy())
                else:
                    cf().upload_observed_corpus(eng, corpus)
            finally:
                corpus.close()
            stores = [eng.sparse_store(w) for w in (0, 1)]
            fit = None
            if sweeps:
                # factors whose product is about the mean stored value: from a start far above the data the first sweeps clamp
                # whole columns of W to zero on these sparse patterns (healthy on the CPU oracle for every case that sweeps)
                s = np.sqrt(A.data.mean() / (K * 0.36))
                W0, T0 = (s * f for f in factors(n, d))
                eng.set_W(W0)
                eng.set_T(T0)
                eng.set_params(reset_topic_method=None)
                eng.sweep(sweeps)
                fit = (eng.get_W(), eng.get_T(), eng.objective())
            out.append((stores, fit))
    return out


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('name,make', STORE_CASES, ids=[c[0] for c in STORE_CASES])
def test_the_device_builds_the_observed_store_the_host_builds(name, make, dtype):
    A = make()
    # sweeps need entries and a rank below both sides: the other cases (an empty pattern, three columns) compare the stores alone
    sweeps = 4 if A.nnz > 0 and min(A.shape) > K else 0
    (host, fit_h), (dev, fit_d) = routes(A, dtype, sweeps)
    for w in (0, 1):
        same_store(host[w], dev[w])
        assert host[w]['build_us'] == 0 and (dev[w]['build_us'] > 0 or A.nnz == 0)
        got = dev[w]
        perm = got['perm']
        real = perm >= 0
        assert got['nnz'] == A.nnz and real.sum() == A.nnz and np.array_equal(np.sort(perm[real]), np.arange(A.nnz))
        assert not got['val'].any()                      # the copies of a pattern-only handle hold the residual: zero until a sweep
    if name in ('12000x150', '300x11000'):
        assert max(dev[0]['nblk'], dev[1]['nblk']) > 1
    if sweeps:
        assert np.array_equal(bits(fit_h[0]), bits(fit_d[0])) and np.array_equal(bits(fit_h[1]), bits(fit_d[1])) and fit_h[2] == fit_d[2]
        assert np.isfinite(fit_d[2])


def test_two_builds_of_one_corpus_give_the_same_bytes():
    A = wc.pat_density(12000, 150, 0.02, seed=31)
    first, second = routes(A, np.float32)[1][0], routes(A, np.float32)[1][0]
    for w in (0, 1):
        same_store(first[w], second[w])


def test_upload_refusals_leave_the_handle_and_the_counters_as_they_were():
    E = lib()
    from rri_nmf_amd import _capi
    A = wc.pat_density(60, 90, 0.3, seed=1)
    with E.DeviceCorpus(A) as fits, E.DeviceCorpus(A[:50]) as short, E.RRIEngine(60, 90, K, dtype=np.float64, weighted='sparse') as eng:
        cf().upload_observed_corpus(eng, fits)
        kept = [eng.sparse_store(w) for w in (0, 1)]
        mem, cor = E.device_memory(), E.corpus_memory()

        def refused(handle, pointer, status, text):
            assert handle._lib.rri_upload_observed_corpus(handle._h, pointer) == status
            assert text in handle._err(), handle._err()
            assert E.device_memory() == mem and E.corpus_memory() == cor

        with pytest.raises(ValueError, match='the corpus is 50 x 90, the handle 60 x 90'):
            cf().upload_observed_corpus(eng, short)
        refused(eng, short._ptr(), _capi.RRI_ERR_INVALID, 'the corpus is 50 x 90, the handle 60 x 90')
        refused(eng, None, _capi.RRI_ERR_INVALID, 'the corpus is NULL or has been destroyed')
        gone = E.DeviceCorpus(A)
        where = ctypes.c_void_p(gone._ptr().value)
        gone.close()
        with pytest.raises(ValueError, match='the corpus is closed'):
            cf().upload_observed_corpus(eng, gone)
        refused(eng, where, _capi.RRI_ERR_INVALID, 'the corpus is NULL or has been destroyed')       # held against the live corpora: never read
        for w in (0, 1):
            same_store(kept[w], eng.sparse_store(w))
        # the host route still works on the same handle afterwards, and leaves the same store
        eng.upload_observed_csr(A)
        for w in (0, 1):
            same_store(kept[w], eng.sparse_store(w))
        # handles of another kind
        for kw, status, text in ((dict(), _capi.RRI_ERR_INVALID, 'not created with weighted=RRI_WEIGHTED_SPARSE'),
                                 (dict(weighted=True), _capi.RRI_ERR_INVALID, 'not created with weighted=RRI_WEIGHTED_SPARSE'),
                                 (dict(sparse_x=True), _capi.RRI_ERR_INVALID, 'not created with weighted=RRI_WEIGHTED_SPARSE'),
                                 (dict(dtype=np.float16), _capi.RRI_ERR_UNSUPPORTED, 'is not available on an RRI_F16 handle')):
            with E.RRIEngine(60, 90, K, **dict(dict(dtype=np.float64), **kw)) as other:
                mem = E.device_memory()
                refused(other, fits._ptr(), status, text)
                with pytest.raises(ValueError if status == _capi.RRI_ERR_INVALID else NotImplementedError):
                    cf().upload_observed_corpus(other, fits)
                with pytest.raises(ValueError, match='no blocked store'):
                    other.sparse_store(0)


# ---- the error at the entries ----------------------------------------------------------------------------------------------------------
D_EDGE, N_W = 800, 12
KS = [1, 2, 5, 50, 128, 129, 1024]          # the pad of an odd k, the lane switch at 128 / 129, RRI_MAX_K
CLIPS = [(-INF, INF), (1.0, 5.0), (3.0, 3.0), (100.0, 200.0)]        # open, the stars, lo = hi, a range that clips every entry


def rows_for(m):
    """row of W per request: reversed, with repeats (12 rows of W for up to 9 requests)"""
    return np.array([(N_W - 1 - q) % 7 for q in range(m)], dtype=np.int64)


@pytest.fixture(scope='module')
def edge_corpora():
    """(scipy matrix, corpus) of the four edge corpora: stars, reals of either sign, and the two short variants with stars"""
    E = lib()
    variants = fc.edge_variants()
    kinds = ['stars', 'real', 'stars', 'negative']
    made = []
    for i, (lengths, kind) in enumerate(zip(variants, kinds)):
        A = fc.ratings(lengths, D_EDGE, seed=40 + i, kind=kind)
        made.append((A, E.DeviceCorpus(A)))
    assert sorted(fc.pieces_of(v) % 4 for v in variants) == [0, 1, 2, 3]
    yield made
    for _, corpus in made:
        corpus.close()


def factors_only(W, T):
    eng = lib().RRIEngine(W.shape[0], T.shape[1], W.shape[1], dtype=np.float64, weighted=False)
    eng.set_W(W)
    eng.set_T(T)
    return eng


@pytest.mark.parametrize('k', KS)
def test_entries_error_against_the_restatement_within_its_bounds(edge_corpora, k):
    W, T = factors(N_W, D_EDGE, k, seed=k)
    W *= 3.0 / np.sqrt(k)          # predictions around the ratings: some below 1, some above 5
    T *= 3.0 / np.sqrt(k)
    with factors_only(W, T) as eng:
        for v, (A, corpus) in enumerate(edge_corpora):
            assert corpus.nnz == A.nnz and (corpus.negatives > 0) == (v in (1, 3))
            for rows in (None, rows_for(A.shape[0])):
                for lo, hi in (CLIPS if v < 2 else CLIPS[1:2]):
                    want = fc.reference(W, T, rows, A, lo, hi)
                    got = cf().entries_error(eng, corpus, rows=rows, clip=(lo, hi), predictions=True)
                    fc.check(got, want, (k, v, lo, hi))
                    assert got['entries'] == A.nnz and got['pred'].min() >= lo and got['pred'].max() <= hi
                    tot_sq = tot_ab = 0.0
                    for q in range(A.shape[0]):
                        tot_sq += got['sq'][q]
                        tot_ab += got['abs'][q]
                    assert got['totals'] == (tot_sq, tot_ab)
                    assert got['rmse'] == np.sqrt(tot_sq / A.nnz) and got['mae'] == tot_ab / A.nnz and got['kernel_ms'] > 0
                    if (lo, hi) == (100.0, 200.0):
                        assert np.all(got['pred'] == 100.0)                  # every entry clipped: the predictions are the bound
                    if (lo, hi) == (3.0, 3.0):
                        assert np.all(got['pred'] == 3.0)
                    empty = np.diff(A.indptr) == 0
                    assert not got['sq'][empty].any() and not got['abs'][empty].any()
                    # None on a side is the open side
                    if (lo, hi) == (-INF, INF):
                        none = cf().entries_error(eng, corpus, rows=rows)
                        assert none['pred'] is None and np.array_equal(bits(none['sq']), bits(got['sq']))


@pytest.mark.parametrize('k', [5, 129])
def test_a_request_has_the_same_bits_alone_twice_and_on_another_handle(edge_corpora, k):
    E = lib()
    W, T = factors(N_W, D_EDGE, k, seed=100 + k)
    A, corpus = edge_corpora[1]
    rows = rows_for(A.shape[0])
    P = wc.pat_density(N_W, D_EDGE, 0.05, seed=5)
    with factors_only(W, T) as eng, E.RRIEngine(N_W, D_EDGE, k, dtype=np.float32, weighted='sparse') as pat:
        pat.upload_observed_csr(P)
        pat.set_W(W)
        pat.set_T(T)
        a = cf().entries_error(eng, corpus, rows=rows, clip=(1.0, 5.0), predictions=True)
        b = cf().entries_error(eng, corpus, rows=rows, clip=(1.0, 5.0), predictions=True)
        c = cf().entries_error(pat, corpus, rows=rows, clip=(1.0, 5.0), predictions=True)
        for other in (b, c):
            for key in ('sq', 'abs', 'pred'):
                assert np.array_equal(bits(a[key]), bits(other[key])), key
            assert a['totals'] == other['totals']
        for q in range(A.shape[0]):                  # a row alone: a one-row corpus, derived on the device
            with corpus[q:q + 1] as one:
                alone = cf().entries_error(eng, one, rows=rows[q:q + 1], clip=(1.0, 5.0), predictions=True)
            assert bits(alone['sq'])[0] == bits(a['sq'])[q] and bits(alone['abs'])[0] == bits(a['abs'])[q]
            assert np.array_equal(bits(alone['pred']), bits(a['pred'][A.indptr[q]:A.indptr[q + 1]]))


def test_scoring_between_two_sweeps_changes_nothing():
    E = lib()
    A = wc.pat_density(60, 90, 0.3, seed=1)
    held = fc.ratings([5, 0, 12] * 20, 90, seed=7)
    s = np.sqrt(A.data.mean() / (K * 0.36))          # a start about as large as the data (see routes())
    W0, T0 = (s * f for f in factors(60, 90))
    out = []
    with E.DeviceCorpus(held) as corpus:
        for score in (False, True):
            with E.RRIEngine(60, 90, K, dtype=np.float64, weighted='sparse') as eng:
                eng.upload_observed_csr(A)
                eng.set_W(W0)
                eng.set_T(T0)
                eng.set_params(reset_topic_method=None)
                eng.sweep(1)
                if score:
                    mem = E.device_memory()
                    W1, T1 = eng.get_W(), eng.get_T()
                    got = cf().entries_error(eng, corpus, clip=(1.0, 5.0))
                    fc.check(got, fc.reference(W1, T1, None, held, 1.0, 5.0))             # the current factors, not the start's
                    assert E.device_memory() == mem
                eng.sweep(1)
                out.append((eng.get_W(), eng.get_T(), eng.objective()))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1])) and out[0][2] == out[1][2]


def test_entries_error_refusals_and_the_empty_corpus():
    E = lib()
    W, T = factors(N_W, 90)
    A = fc.ratings([3, 0, 4], 90, seed=2)
    with E.DeviceCorpus(A) as corpus, E.DeviceCorpus(sp.csr_matrix((4, 90))) as empty, E.DeviceCorpus(sp.csr_matrix(np.ones((3, 80)))) as narrow, \
            E.DeviceCorpus(fc.ratings([1] * (N_W + 1), 90, seed=3)) as tall:
        with E.RRIEngine(N_W, 90, K, dtype=np.float64) as bare:
            got = cf().entries_error(bare, empty, predictions=True)          # nothing to score: W and T are not even needed
            assert got['entries'] == 0 and not got['sq'].any() and not got['abs'].any() and got['pred'].size == 0 and got['kernel_ms'] == 0
            assert np.isnan(got['rmse']) and np.isnan(got['mae']) and got['totals'] == (0.0, 0.0)
            with pytest.raises(ValueError, match='W and T must be set first'):
                cf().entries_error(bare, corpus)
        with factors_only(W, T) as eng:
            mem, cor = E.device_memory(), E.corpus_memory()
            with pytest.raises(ValueError, match='the corpus has 80 columns, W T has 90'):
                cf().entries_error(eng, narrow)
            with pytest.raises(ValueError, match='clip_lo 5 is above clip_hi 1'):
                cf().entries_error(eng, corpus, clip=(5.0, 1.0))
            with pytest.raises(ValueError, match='a clip bound is NaN'):
                cf().entries_error(eng, corpus, clip=(float('nan'), 1.0))
            with pytest.raises(ValueError, match=r'rows\[1\] = 12 is out of range'):
                cf().entries_error(eng, corpus, rows=[0, N_W, 1])
            with pytest.raises(ValueError, match=r'rows\[2\] = -1 is out of range'):
                cf().entries_error(eng, corpus, rows=[0, 1, -1])
            with pytest.raises(ValueError, match='rows is NULL and the corpus has 13 rows, W has 12'):
                cf().entries_error(eng, tall)
            with pytest.raises(ValueError, match='one row of W per row of the corpus'):
                cf().entries_error(eng, corpus, rows=[0, 1])
            assert cf().entries_error(eng, tall, rows=np.zeros(N_W + 1, dtype=np.int64))['entries'] == N_W + 1       # with rows: any count
            assert E.device_memory() == mem and E.corpus_memory() == cor


# ---- the value range -----------------------------------------------------------------------------------------------------------------
def test_value_range():
    E = lib()
    one = sp.csr_matrix((np.array([-2.5]), (np.array([3]), np.array([7]))), shape=(5, 9))
    with E.DeviceCorpus(one) as c:
        assert c.value_range() == (-2.5, -2.5)
    neg = fc.ratings([4, 0, 300, 1], 400, seed=8, kind='negative')
    with E.DeviceCorpus(neg) as c:
        assert c.value_range() == (neg.data.min(), neg.data.max()) and neg.data.max() < 0
    # more entries than one round of the first stage's grid (1024 workgroups of 256): every workgroup strides
    big = wc.pat_density(12000, 150, 0.2, seed=9)
    big.data[:] = np.random.RandomState(9).randn(big.nnz)
    assert big.nnz > 1024 * 256
    mem, cor = E.device_memory(), None
    with E.DeviceCorpus(big) as c:
        cor = E.corpus_memory()
        assert c.value_range() == (big.data.min(), big.data.max())
        assert E.corpus_memory() == cor and E.device_memory() == mem
    with E.DeviceCorpus(sp.csr_matrix((5, 9))) as c:
        with pytest.raises(ValueError, match='the corpus is empty'):
            c.value_range()


# ---- nmf(corpus, observed_only=True) ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def recsys():
    """the reference's recommender fixture, 100 x 200 with 617 ratings: the scipy matrix, its pattern and a corpus"""
    A = sp.load_npz(os.path.join(GOLDEN, 'ref_data', 'recsys_data_train.npz')).tocsr().astype(np.float64)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    assert A.shape == (100, 200) and A.nnz == 617
    corpus = lib().DeviceCorpus(A)
    yield A, corpus
    corpus.close()


def pattern(A):
    M = A.copy()
    M.data = np.ones(M.nnz)
    return M


RS = dict(max_iter=30, max_time=7200, compute_obj_each_iter=True, reset_topic_method=None, t_row_sum=1.0, random_state=0)


def nmf(X, **kw):
    from rri_nmf_amd.nmf import nmf as f
    return f(X, K, **dict(RS, **kw))


def same_fit(a, b):
    assert np.array_equal(bits(a['W']), bits(b['W'])) and np.array_equal(bits(a['T']), bits(b['T']))
    assert len(a['obj_history']) == len(b['obj_history']) > 0
    assert np.array_equal(bits(np.array(a['obj_history'])), bits(np.array(b['obj_history'])))


def test_observed_only_is_the_weighted_fit_on_the_pattern(recsys):
    A, corpus = recsys
    E = lib()
    mem, cor = E.device_memory(), E.corpus_memory()
    W0, T0 = factors(*A.shape, seed=4)
    T0 /= T0.sum(axis=1, keepdims=True)
    a = nmf(corpus, observed_only=True, W_in=W0, T_in=T0, max_iter=6)
    b = nmf(A, W_mat=pattern(A), sparse_pattern=True, W_in=W0, T_in=T0, max_iter=6)
    same_fit(a, b)
    # the objective is re-evaluated on the corpus: the same handle, the same bytes, the same number as the host route's
    again = a['obj_calculator'].true_objective()
    assert again == b['obj_calculator'].true_objective() and abs(again - a['obj_history'][-1]) <= 1e-6 * abs(a['obj_history'][-1])
    # the default start: through the handle's products on both routes (device_init=True on the host route, see the module docstring)
    a = nmf(corpus, observed_only=True, max_iter=6)
    b = nmf(A, W_mat=pattern(A), sparse_pattern=True, device_init=True, max_iter=6)
    same_fit(a, b)
    # float32 storage of the ratings: stars are exact in it, so the same bits again
    same_fit(nmf(corpus, observed_only=True, W_in=W0, T_in=T0, max_iter=3, dtype=np.float32),
             nmf(A, W_mat=pattern(A), sparse_pattern=True, W_in=W0, T_in=T0, max_iter=3, dtype=np.float32))
    assert E.device_memory() == mem and E.corpus_memory() == cor


def split_of(corpus):
    """corpus.split_entries(0.2, random_state=3) as (train corpus, held corpus, the host's device_entries for the same split)"""
    train, held = corpus.split_entries(0.2, random_state=3)
    H = held.to_scipy().tocoo()
    lo, hi = corpus.value_range()
    return train, held, (H.row, H.col, H.data, lo, hi)


def stop_with(**attrs):
    def stop(X, W, T):
        raise AssertionError('scored on the device')
    for key, val in attrs.items():
        setattr(stop, key, val)
    return stop


def recorded_host_scores(monkeypatch):
    E = lib()
    scores = []
    plain = E.RRIEngine.masked_rmse

    def recording(self, *a):
        scores.append(plain(self, *a))
        return scores[-1]
    monkeypatch.setattr(E.RRIEngine, 'masked_rmse', recording)
    return scores


def comparable(scores):
    """the stop decision is comparable only when successive held-out scores are not near-ties: a condition on the inputs"""
    s = np.array(scores)
    assert s.size >= 2
    gaps = np.abs(np.diff(s)) / np.abs(s[:-1])
    print('held-out scores of the host route:', scores, 'smallest relative gap %.3e' % gaps.min())
    assert gaps.min() > 1e-6
    return True


def test_the_early_stop_on_a_held_out_corpus_takes_the_host_routes_decisions(recsys, monkeypatch):
    A, corpus = recsys
    train, held, entries = split_of(corpus)
    try:
        assert train.nnz + held.nnz == A.nnz and held.nnz > 50
        Atr = train.to_scipy()
        scores = recorded_host_scores(monkeypatch)
        b = nmf(Atr, W_mat=pattern(Atr), sparse_pattern=True, device_init=True, early_stop=stop_with(device_entries=entries))
        assert comparable(scores)
        assert len(b['obj_history']) < RS['max_iter'] and scores[-1] > scores[-2]         # the score rose: the rollback path ran
        n_host = len(scores)
        a = nmf(train, observed_only=True, early_stop=stop_with(device_corpus=(held,) + entries[3:]))
        assert len(scores) == n_host                                                        # (the corpus route scored elsewhere)
        assert len(a['obj_history']) == len(b['obj_history']) and len(a['iter_cputime']) == len(b['iter_cputime'])
        for key in ('W', 'T'):
            assert np.linalg.norm(a[key] - b[key]) <= 1e-10 * np.linalg.norm(b[key]), key
    finally:
        train.close()
        held.close()


# ---- the estimator -------------------------------------------------------------------------------------------------------------------
def test_fit_corpus_without_early_stopping_is_fit_from_Xtr_in_bits(recsys):
    from rri_nmf_amd import sklearn_interface as si
    A, corpus = recsys
    kw = dict(random_state=0, max_iter=8, use_validation_early_stopping=False, nmf_kwargs={'device_init': True})
    Ea = si.NMF_RS_Estimator(100, 200, K, **kw).fit_corpus(corpus, keep_seen=True)
    Eb = si.NMF_RS_Estimator(100, 200, K, **kw).fit_from_Xtr(corpus.to_scipy())
    assert np.array_equal(bits(Ea.W), bits(Eb.W)) and np.array_equal(bits(Ea.T), bits(Eb.T))
    assert (Ea.min_rating, Ea.max_rating) == (Eb.min_rating, Eb.max_rating) == (A.data.min(), A.data.max())
    for S in (Ea.seen_, Eb.seen_):
        assert S.has_canonical_format and np.all(S.data == 1)
    assert np.array_equal(Ea.seen_.indptr, Eb.seen_.indptr) and np.array_equal(Ea.seen_.indices, Eb.seen_.indices)
    assert np.array_equal(Ea.recommend([0, 5, 99], 4)[0], Eb.recommend([0, 5, 99], 4)[0])
    # keep_seen=False: nothing is downloaded, and recommend(exclude_seen=True) raises as it does without the pairs
    Ec = si.NMF_RS_Estimator(100, 200, K, **kw).fit_corpus(corpus, keep_seen=False)
    assert Ec.seen_ is None and np.array_equal(bits(Ec.W), bits(Ea.W))
    with pytest.raises(ValueError, match='exclude_seen=True needs the pairs given to fit'):
        Ec.recommend([0], 4)


def test_fit_corpus_with_a_held_out_corpus_is_the_host_route_fed_the_same_split(recsys, monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    A, corpus = recsys
    train, held, entries = split_of(corpus)
    try:
        Atr = train.to_scipy()
        scores = recorded_host_scores(monkeypatch)
        b = nmf(Atr, W_mat=pattern(Atr), sparse_pattern=True, device_init=True, early_stop=stop_with(device_entries=entries),
                project_T_each_iter=False, project_W_each_iter=False, w_row_sum=None, reg_w_l1=0, reg_t_l1=0)
        assert comparable(scores)
        E = si.NMF_RS_Estimator(100, 200, K, random_state=0, max_iter=RS['max_iter']).fit_corpus(train, held)
        assert (E.min_rating, E.max_rating) == entries[3:]
        assert len(E.nmf_outputs['obj_history']) == len(b['obj_history'])
        assert np.linalg.norm(E.W - b['W']) <= 1e-10 * np.linalg.norm(b['W']) and np.linalg.norm(E.T - b['T']) <= 1e-10 * np.linalg.norm(b['T'])
        # seen_ is the pattern of train and held together: the whole fixture's
        assert np.array_equal(E.seen_.indptr, A.indptr) and np.array_equal(E.seen_.indices, A.indices)
        # without a held-out corpus the split is made and closed inside: the caller's corpora are neither closed nor counted twice
        cor = lib().corpus_memory()
        E2 = si.NMF_RS_Estimator(100, 200, K, random_state=0, max_iter=5).fit_corpus(corpus)
        assert lib().corpus_memory() == cor and E2.W.shape == (100, K) and np.array_equal(E2.seen_.indices, A.indices)
    finally:
        train.close()
        held.close()


def test_score_corpus_is_score_within_the_bound(recsys):
    from rri_nmf_amd import sklearn_interface as si
    A, corpus = recsys
    test = sp.load_npz(os.path.join(GOLDEN, 'ref_data', 'recsys_data_test.npz')).tocsr().astype(np.float64)
    test.sum_duplicates()
    test.eliminate_zeros()
    E = si.NMF_RS_Estimator(100, 200, K, random_state=0, max_iter=5, use_validation_early_stopping=False).fit_corpus(corpus, keep_seen=False)
    with lib().DeviceCorpus(test) as held:
        got, want = E.score_corpus(held), E.score(held.to_scipy())
    # sum r^2 within the restatement's bound per request, and (requests + entries + 4) roundings of whatever order adds them up;
    # the square root halves the relative error and adds a rounding a side
    ref = fc.reference(E.W, E.T, None, test, E.min_rating, E.max_rating)
    N, tot = test.nnz, ref['totals'][0]
    bound_tot = ref['sq_bound'].sum() + (test.shape[0] + N + 4) * fc.U * tot
    bound = bound_tot / (2.0 * N * want) + 4 * fc.U * want
    print('score_corpus %.17g score %.17g bound %.3e' % (got, want, bound))
    assert abs(got - want) <= bound and abs(want - np.sqrt(tot / N)) <= bound


def test_fit_corpus_reaches_the_references_score_on_its_fixture():
    """the reference's number for NMF_RS_Estimator without early stopping (g4_wrri: rs_noes_score), at the tolerance
    tests/test_nmf_gpu.py holds fit_from_Xtr to"""
    from rri_nmf_amd import sklearn_interface as si
    g4 = load_golden('g4_wrri')
    X = g4['X']
    n, d = X.shape
    with lib().DeviceCorpus(X) as corpus:
        E = si.NMF_RS_Estimator(n, d, 5, random_state=0, max_iter=20, use_validation_early_stopping=False).fit_corpus(corpus)
    print('score %.9f, the reference %.9f' % (E.score(X), float(g4['rs_noes_score'])))
    assert abs(E.score(X) - float(g4['rs_noes_score'])) < 1e-4
