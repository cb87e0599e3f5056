"""The fit from a DeviceCorpus on the GPU: the blocked store of a CSR-X handle built on the device (rri_upload_X_corpus) against
the one the host builds (rri_upload_X_csr) and against the numpy restatement of tests/wsb_cases.py; fits from a corpus against
fits from its scipy matrix; ownership and refusals.

Store equality is equality of every field and every array, values compared as bits: the device builder must leave what the
host's stable counting sort leaves, whatever order its claims arrived in.  Fit equality is equality of bits of W, T and the
objective history wherever both routes start from the same factors: the sweeps read the same bytes.  The shapes are the smallest
at which the layout changes (tests/spbuild_cases.py)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import corpus_cases as cc
import spbuild_cases as sc
import wsb_cases as wc

pytestmark = pytest.mark.gpu
K = 5
FIELDS = ('nblk', 'bw', 'nseg', 'gdim', 'count', 'nwork', 'lps', 'nnz', 'longest_row')
ARRAYS = ('segptr', 'idx', 'perm', 'work')


def lib():
    from rri_nmf_amd import engine
    return engine


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_store(a, b):
    for f in FIELDS:
        assert a[f] == b[f], f
    for f in ARRAYS:
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), f
    assert a['val'].dtype == b['val'].dtype and np.array_equal(bits(a['val']), bits(b['val'])), 'val'


def stores_of(A, dtype):
    """(stores by the host route, stores by the device route, n_cu) of the canonical scipy matrix A"""
    E = lib()
    n, d = A.shape
    with E.DeviceCorpus(A) as corpus:
        assert corpus.nnz == A.nnz and corpus.rows_rewritten == 0
        with E.RRIEngine(n, d, K, dtype=dtype, sparse_x=True) as ea, E.RRIEngine(n, d, K, dtype=dtype, sparse_x=True) as eb:
            ea.upload_X_csr(corpus.to_scipy())
            eb.upload_X_corpus(corpus)
            n_cu = eb.layout_info()['n_cu']
            return [ea.sparse_store(w) for w in (0, 1)], [eb.sparse_store(w) for w in (0, 1)], n_cu


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('name,make', sc.cases(), ids=[c[0] for c in sc.cases()])
def test_the_device_builds_the_store_the_host_builds(name, make, dtype):
    A = make()
    host, dev, n_cu = stores_of(A, dtype)
    for w in (0, 1):
        same_store(host[w], dev[w])
        assert host[w]['build_us'] == 0 and (dev[w]['build_us'] > 0 or A.nnz == 0)
        # ... and both are what the restatement says, so the two routes are not wrong together
        L = wc.sp_copy_layout(A, w, 'fp64', True, n_cu)
        got = dev[w]
        assert {f: got[f] for f in ('nblk', 'bw', 'lps', 'nwork', 'gdim')} == {f: L[f] for f in ('nblk', 'bw', 'lps', 'nwork', 'gdim')}
        assert np.array_equal(np.diff(got['segptr'], axis=1), (L['seg_len'] + 3) // 4 * 4)
        assert np.array_equal(got['work'], np.array([item + (w,) for item in L['work']], dtype=np.int32).reshape(-1, 4))
        assert got['nnz'] == A.nnz and got['longest_row'] == np.diff(A.indptr).max() and got['count'] == got['segptr'][-1, -1]
        # the entries of every segment in canonical order, its pads behind them; the values are X's
        perm, idx = got['perm'], got['idx']
        real = perm >= 0
        assert real.sum() == A.nnz and np.all(idx[~real] == got['bw']) and np.array_equal(np.sort(perm[real]), np.arange(A.nnz))
        assert np.array_equal(bits(got['val'][real]), bits(A.data[perm[real]].astype(dtype))) and not got['val'][~real].any()
        for b in range(got['nblk']):
            for s in np.flatnonzero(L['seg_len'][b])[:50]:
                lo, m = got['segptr'][b, s], L['seg_len'][b, s]
                assert np.all(np.diff(perm[lo:lo + m]) > 0) and np.all(perm[lo + m:got['segptr'][b, s + 1]] == -1), (b, s)


def test_two_builds_of_one_corpus_give_the_same_bytes():
    A = wc.pat_density(15400, 40, 0.1, seed=13)
    _, first, _ = stores_of(A, np.float64)
    _, second, _ = stores_of(A, np.float64)
    for w in (0, 1):
        same_store(first[w], second[w])


# ---- fits ------------------------------------------------------------------------------------------------------------------------
def nmf(X, **kw):
    from rri_nmf_amd.nmf import nmf as f
    return f(X, K, **dict(dict(max_iter=3, compute_obj_each_iter=True, random_state=0), **kw))


def same_fit(a, b):
    assert np.array_equal(bits(a['W']), bits(b['W'])) and np.array_equal(bits(a['T']), bits(b['T']))
    assert len(a['obj_history']) == len(b['obj_history']) > 0
    assert np.array_equal(bits(np.array(a['obj_history'])), bits(np.array(b['obj_history'])))


def factors(n, d, seed=0):
    rng = np.random.RandomState(seed)
    return 0.1 + rng.rand(n, K), 0.1 + rng.rand(K, d)


@pytest.fixture(scope='module')
def counts():
    """300 x 120 term counts without an empty row, as a scipy matrix and as a corpus"""
    rng = np.random.RandomState(3)
    X = rng.poisson(0.3, size=(300, 120)).astype(np.float64)
    X[:, 0] += 1.0
    A = sp.csr_matrix(X)
    corpus = lib().DeviceCorpus(A)
    yield A, corpus
    corpus.close()


@pytest.mark.parametrize('name', ['57x33', '200x15297', '15400x40'])
def test_a_fit_from_given_factors_is_the_fit_from_the_scipy_matrix(name):
    A = dict(sc.cases())[name]()
    W0, T0 = factors(*A.shape)
    with lib().DeviceCorpus(A) as corpus:
        same_fit(nmf(corpus, W_in=W0, T_in=T0), nmf(corpus.to_scipy(), sparse_X=True, W_in=W0, T_in=T0))
        assert nmf(corpus, W_in=W0, T_in=T0, dtype=np.float32)['W'].dtype == np.float64


def test_preprocessing_and_the_default_start_on_the_device(counts):
    A, corpus = counts
    a = nmf(corpus, preprocess=('tfidf', 'normalize'))
    b = nmf(A, sparse_X=True, preprocess=('tfidf', 'normalize'))
    same_fit(a, b)
    assert np.array_equal(a['idf'], b['idf'])


def test_uniform_rows_fold_in_and_frozen_batches(counts):
    A, corpus = counts
    E = lib()
    # empty documents: kept as uniform rows on both routes
    H = A.tolil()
    H[5:8, :] = 0
    H = sp.csr_matrix(H.tocsr())
    H.eliminate_zeros()
    with E.DeviceCorpus(H) as holes:
        kw = dict(preprocess=('tfidf', 'normalize'), uniform_rows=True)
        same_fit(nmf(holes, **kw), nmf(H, sparse_X=True, **kw))
        # without uniform_rows there is no host to fall back to, and no handle is left behind
        before = E.device_memory()
        with pytest.raises(ValueError, match='uniform_rows=True'):
            nmf(holes, preprocess=('normalize',))
        assert E.device_memory() == before
    # the fold-in: T fixed
    W0, T0 = factors(*A.shape, seed=1)
    same_fit(nmf(corpus, W_in=W0, T_in=T0, fix_T=True), nmf(A, sparse_X=True, W_in=W0, T_in=T0, fix_T=True))
    # two batches, the first frozen into the second
    A1, A2 = A[:180], A[180:]
    with E.DeviceCorpus(A1) as c1, E.DeviceCorpus(A2) as c2:
        outs = []
        for X1, X2, extra in ((c1, c2, {}), (A1, A2, dict(sparse_X=True))):
            r1 = nmf(X1, W_in=W0[:180], T_in=T0, frozen=True, **extra)
            r2 = nmf(X2, W_in=W0[180:], T_in=r1['T'], frozen=r1['frozen'], **extra)
            outs.append((r1, r2))
        same_fit(outs[0][0], outs[1][0])
        same_fit(outs[0][1], outs[1][1])
        assert np.array_equal(bits(outs[0][1]['frozen'].B), bits(outs[1][1]['frozen'].B))


def test_the_estimator_takes_the_corpus(counts):
    from rri_nmf_amd.sklearn_interface import NMF_TM_Estimator
    A, corpus = counts
    n, d = A.shape
    made = []
    for X in (corpus, A):
        E = NMF_TM_Estimator(n, d, K, handle_tfidf=True, handle_normalization=True, max_iter=3, nmf_kwargs={'sparse_X': True},
                             keep_resident=X is corpus)
        E.fit(X)
        fitted = (E.W.copy(), E.T.copy())
        if X is corpus:
            E.one_iter(X)
            assert E._resident.reuses == 1              # the handle of fit() served one_iter() on the same corpus object
            E.release()
            E.W, E.T = fitted
        folded = E.transform(X)
        P = NMF_TM_Estimator(n, d, K, handle_tfidf=True, handle_normalization=True, nmf_kwargs={'sparse_X': True})
        first, second = (corpus, corpus) if X is corpus else (A, A)
        P.partial_fit(first, sweeps=2)
        P.partial_fit(second, sweeps=2)
        made.append(fitted + (folded, P.W, P.T))
    for a, b in zip(*made):
        assert np.array_equal(bits(a), bits(b))
    with pytest.raises(TypeError, match='DeviceCorpus'):
        E.score(corpus)


def test_a_raw_corpus_and_device_tensors_fit_to_the_same_bits():
    import torch
    E = lib()
    raw = cc.raw_rows([0, 1, 2, 40, 63, 64, 65, 200, 7, 90] * 6, 150, seed=9, zeros=0.1)
    A = cc.scipy_canonical(*raw)
    W0, T0 = factors(*A.shape, seed=2)
    want = nmf(A, sparse_X=True, W_in=W0, T_in=T0)
    with E.DeviceCorpus.from_arrays(*raw) as corpus:
        assert corpus.rows_rewritten > 0 and corpus.duplicates_merged > 0 and corpus.zeros_dropped > 0
        same_fit(nmf(corpus, W_in=W0, T_in=T0), want)
    t = [torch.as_tensor(a).cuda() for a in raw[:3]]
    with E.DeviceCorpus.from_device(t[0], t[1], t[2], raw[3]) as corpus:
        same_fit(nmf(corpus, W_in=W0, T_in=T0), want)


# ---- ownership and refusals ------------------------------------------------------------------------------------------------------
def test_the_handle_owns_its_store_and_the_corpus_may_go():
    E = lib()
    A = wc.pat_density(200, 300, 0.05, seed=4)
    W0, T0 = factors(*A.shape, seed=3)
    mem0, cor0 = E.device_memory(), E.corpus_memory()
    out = []
    for route in ('corpus', 'csr'):
        eng = E.RRIEngine(200, 300, K, dtype=np.float64, sparse_x=True)
        if route == 'corpus':
            corpus = E.DeviceCorpus(A)
            cor1 = E.corpus_memory()
            eng.upload_X_corpus(corpus)
            assert E.corpus_memory() == cor1 and same_arrays(corpus.to_scipy(), A)         # not modified, not counted twice
            corpus.close()
            assert E.corpus_memory() == cor0
        else:
            eng.upload_X_csr(A)
        eng.set_W(W0)
        eng.set_T(T0)
        eng.set_params()
        eng.sweep(2)
        out.append((eng.get_W(), eng.get_T(), eng.objective()))
        eng.close()
        assert E.device_memory() == mem0
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1])) and out[0][2] == out[1][2]


def same_arrays(A, B):
    return A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)


def test_refusals_leave_the_handle_and_the_counters_as_they_were():
    E = lib()
    from rri_nmf_amd import _capi
    A = wc.pat_density(60, 90, 0.3, seed=1)
    with E.DeviceCorpus(A) as fits, E.DeviceCorpus(A[:50]) as short, E.RRIEngine(60, 90, K, dtype=np.float64, sparse_x=True) as eng:
        eng.upload_X_corpus(fits)
        kept = [eng.sparse_store(w) for w in (0, 1)]
        mem, cor = E.device_memory(), E.corpus_memory()

        def refused(handle, pointer, status, text):
            assert handle._lib.rri_upload_X_corpus(handle._h, pointer) == status
            assert text in handle._err(), handle._err()
            assert E.device_memory() == mem and E.corpus_memory() == cor

        with pytest.raises(ValueError, match='the corpus is 50 x 90, the handle 60 x 90'):
            eng.upload_X_corpus(short)
        refused(eng, short._ptr(), _capi.RRI_ERR_INVALID, 'the corpus is 50 x 90, the handle 60 x 90')
        refused(eng, None, _capi.RRI_ERR_INVALID, 'the corpus is NULL or has been destroyed')
        gone = E.DeviceCorpus(A)
        where = ctypes.c_void_p(gone._ptr().value)
        gone.close()
        with pytest.raises(ValueError, match='the corpus is closed'):
            eng.upload_X_corpus(gone)
        refused(eng, where, _capi.RRI_ERR_INVALID, 'the corpus is NULL or has been destroyed')       # held against the live corpora: never read
        for w in (0, 1):
            same_store(kept[w], eng.sparse_store(w))
        # handles of another kind
        for kw, status, text in ((dict(), _capi.RRI_ERR_INVALID, 'this handle keeps a dense X'),
                                 (dict(weighted=True), _capi.RRI_ERR_INVALID, 'this handle keeps a dense X'),
                                 (dict(weighted='sparse'), _capi.RRI_ERR_INVALID, 'takes its data through rri_upload_observed_csr'),
                                 (dict(dtype=np.float16), _capi.RRI_ERR_UNSUPPORTED, 'X from a corpus is not available on an RRI_F16 handle')):
            with E.RRIEngine(60, 90, K, **dict(dict(dtype=np.float64), **kw)) as other:
                mem = E.device_memory()
                refused(other, fits._ptr(), status, text)
                with pytest.raises(ValueError if status == _capi.RRI_ERR_INVALID else NotImplementedError):
                    other.upload_X_corpus(fits)
                with pytest.raises(ValueError, match='no blocked store'):
                    other.sparse_store(0)
    with E.RRIEngine(60, 90, K, dtype=np.float64, sparse_x=True) as eng:
        with pytest.raises(ValueError, match='no blocked store'):
            eng.sparse_store(1)
        eng.upload_X_csr(A)
        with pytest.raises(ValueError, match='which = 2'):
            eng.sparse_store(2)
