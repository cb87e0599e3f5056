"""Host side of tf-idf / row normalisation for a scipy sparse X (nmf(..., preprocess=), NMF_TM_Estimator's handle_* flags): which
route the option takes (nmf.preprocess_route), what the engine is handed on each of them, the way back to the host when a CSR
handle meets a row that normalisation would make dense, and the agreement of header and binding on the two exports behind it.
No GPU: a recording engine stands in for RRIEngine where nmf() would make one."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT


def counts_csr(n=12, d=9, seed=0, empty_row=None):
    """term counts without an empty or zero-total row (every row has a term that not every document has)"""
    rs = np.random.RandomState(seed)
    X = rs.randint(0, 4, size=(n, d)).astype(np.float64)
    X[:, 0] = 0
    X[np.arange(n), 1 + np.arange(n) % (d - 1)] += 1      # no empty row ...
    X[0, 0] = 2                                           # ... and column 0 occurs in one document only
    if empty_row is not None:
        X[empty_row, :] = 0
    return sp.csr_matrix(X)


def recording_engine(log, zero_total_on=()):
    """an RRIEngine that computes nothing: it records what it is given and runs a whole (one-sweep) nmf() call.  The engines whose
    index (in order of creation) is in `zero_total_on` raise ZeroTotalRows from preprocess()."""
    made = []

    class Recording(object):
        def __init__(self, n, d, k, dtype=np.float32, weighted=False, device=0, stream=None, schedule='gram', sparse_x=False):
            self.index = len(made)
            made.append(self)
            log.append(('init', self.index, np.dtype(dtype), bool(sparse_x)))
            self.n, self.d, self.k, self.dtype = n, d, k, np.dtype(dtype)
            self.sparse_x, self.n_resets_used, self.closed = bool(sparse_x), 0, False

        def upload_X(self, X):
            log.append(('upload_X', self.index, np.array(X, copy=True)))

        def upload_X_csr(self, A):
            log.append(('upload_X_csr', self.index, sp.csr_matrix(A).toarray()))

        def preprocess(self, **kw):
            log.append(('preprocess', self.index, kw))
            if self.index in zero_total_on:
                from rri_nmf_amd.engine import ZeroTotalRows
                raise ZeroTotalRows(1)
            return np.full(self.d, 0.5) if kw.get('tfidf') is True else None

        def begin_run(self):
            self.n_resets_used = 0

        def set_W(self, W):
            self.W = np.array(W, dtype=np.float64)

        def set_T(self, T):
            self.T = np.array(T, dtype=np.float64)

        def set_params(self, **kw):
            pass

        def sweep(self, m=1):
            return m

        def objective(self):
            return 1.0

        def get_W(self):
            return self.W

        def get_T(self):
            return self.T

        def close(self):
            if not self.closed:
                log.append(('close', self.index))
            self.closed = True

    return Recording


def run(nmf_mod, X, **kw):
    n, d = X.shape
    return nmf_mod.nmf(X, 2, W_in=np.ones((n, 2)), T_in=np.ones((2, d)), max_iter=1, **kw)


def names(log):
    return [e[0] for e in log]


# ---- the route function, case by case -----------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(W_mat=True), dict(w_row=True), dict(host_callbacks=True), dict(half=True)])
@pytest.mark.parametrize('csr, sparse', [(False, False), (False, True), (True, True)])
def test_route_host_conditions_stay(kw, csr, sparse):
    from rri_nmf_amd.nmf import preprocess_route
    assert preprocess_route(csr, sparse, normalize=True, **kw) == 'host'
    assert preprocess_route(csr, sparse, normalize=False, **kw) == 'host'


def test_route_of_a_csr_handle():
    from rri_nmf_amd.nmf import preprocess_route
    assert preprocess_route(True, True) == 'device'
    assert preprocess_route(True, True, normalize=True) == 'device'
    assert preprocess_route(True, False, normalize=True) == 'device'                 # a dense X converted for sparse_X=True
    # an empty row: only row normalisation makes it dense
    assert preprocess_route(True, True, normalize=True, has_empty_row=True) == 'host'
    assert preprocess_route(True, True, normalize=False, has_empty_row=True) == 'device'


def test_route_of_dense_handles():
    from rri_nmf_amd.nmf import preprocess_route
    assert preprocess_route(False, False, normalize=True) == 'device'
    # a scipy sparse X densified on the device: the dense kernel writes the uniform rows itself
    assert preprocess_route(False, True, normalize=True) == 'device'
    assert preprocess_route(False, True, normalize=True, has_empty_row=True) == 'device'


def test_route_under_a_group():
    from rri_nmf_amd.nmf import preprocess_route
    assert preprocess_route(False, False, normalize=True, group=True) == 'device'
    for kw in (dict(x_is_sparse=True), dict(x_is_sparse=False, W_mat=True), dict(x_is_sparse=False, w_row=True),
               dict(x_is_sparse=False, host_callbacks=True)):
        with pytest.raises(NotImplementedError):
            preprocess_route(False, group=True, **kw)
    with pytest.raises(NotImplementedError):
        preprocess_route(True, True, group=True)


def test_route_of_a_call_takes_the_answer_of_sparse_x_route(monkeypatch):
    """the automatic rule: a sparse X whose dense copy does not fit goes onto the CSR handle, and only there does an empty row
    matter"""
    from rri_nmf_amd import nmf as nmf_mod
    X = counts_csr(empty_row=3)
    for free, want in ((1 << 40, ('device', False)), (16, ('host', True))):
        monkeypatch.setattr(nmf_mod, '_device_free_bytes', lambda device, free=free: free)
        assert nmf_mod._route_of_call(X, (True, True)) == want
    assert nmf_mod._route_of_call(X, (True, False), sparse_X=True) == ('device', True)
    assert nmf_mod._route_of_call(X.toarray(), (True, True), sparse_X=True) == ('host', True)
    assert nmf_mod._route_of_call(counts_csr().toarray(), (True, True), sparse_X=True) == ('device', True)
    assert nmf_mod._route_of_call(X, (True, True), sparse_X=True, W_mat=X) == ('host', None)


# ---- what the engine is handed --------------------------------------------------------------------------------------------
def test_csr_handle_gets_the_raw_values_and_preprocesses_them(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    X = counts_csr()
    assert np.all(np.diff(X.indptr) > 0)
    out = run(nmf_mod, X, sparse_X=True, preprocess=('tfidf', 'normalize'))
    assert names(log) == ['init', 'upload_X_csr', 'preprocess', 'close']
    assert log[0][2:] == (np.float64, True)                       # raw values in `dtype or float64`, as on the dense route
    assert np.array_equal(log[1][2], X.toarray())                 # the RAW counts
    assert log[2][2] == {'tfidf': True, 'normalize': True}
    assert np.array_equal(out['idf'], np.full(X.shape[1], 0.5))   # the idf the engine used
    log[:] = []
    run(nmf_mod, X.astype(np.float32), sparse_X=True, preprocess='normalize', dtype=np.float32)
    assert log[0][2:] == (np.float32, True) and log[2][2] == {'tfidf': False, 'normalize': True}


def test_csr_handle_with_an_empty_row_takes_the_host_route(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    X = counts_csr(empty_row=4)
    want, idf = nmf_mod._preprocess_on_host(X, True, True)
    out = run(nmf_mod, X, sparse_X=True, preprocess=('tfidf', 'normalize'))
    assert names(log) == ['init', 'upload_X_csr', 'close']        # preprocess() is never called
    assert np.array_equal(log[1][2], want.toarray()) and np.array_equal(out['idf'], idf)
    assert np.allclose(log[1][2][4], 1.0 / X.shape[1])            # the uniform row travels as stored values
    # tf-idf alone leaves the row empty: the device route again
    log[:] = []
    run(nmf_mod, X, sparse_X=True, preprocess='tfidf')
    assert names(log) == ['init', 'upload_X_csr', 'preprocess', 'close'] and np.array_equal(log[1][2], X.toarray())
    # ... and resident= keeps its refusal where the route is the host's
    with pytest.raises(ValueError, match='resident'):
        run(nmf_mod, X, sparse_X=True, preprocess=('tfidf', 'normalize'), resident=nmf_mod.ResidentProblem())


def test_densified_sparse_X_goes_up_raw(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    monkeypatch.setattr(nmf_mod, '_device_free_bytes', lambda device: 1 << 40)
    X = counts_csr(empty_row=2)
    run(nmf_mod, X, preprocess=('tfidf', 'normalize'))
    assert names(log) == ['init', 'upload_X_csr', 'preprocess', 'close']
    assert log[0][2:] == (np.float64, False) and np.array_equal(log[1][2], X.toarray())
    log[:] = []
    run(nmf_mod, X, sparse_X=False, preprocess=('tfidf', 'normalize'))
    assert names(log) == ['init', 'upload_X_csr', 'preprocess', 'close'] and log[0][3] is False


@pytest.mark.parametrize('with_holder', [False, True])
def test_zero_total_rows_lead_back_to_the_host(monkeypatch, with_holder):
    """the engine reports a row whose tf-idf total is 0: that handle is closed, a second engine gets host-preprocessed values,
    the call returns, and a holder given with resident= ends empty"""
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log, zero_total_on=(0,)))
    X = counts_csr()
    want, idf = nmf_mod._preprocess_on_host(X, True, True)
    holder = nmf_mod.ResidentProblem() if with_holder else None
    out = run(nmf_mod, X, sparse_X=True, preprocess=('tfidf', 'normalize'), resident=holder)
    assert names(log) == ['init', 'upload_X_csr', 'preprocess', 'close', 'init', 'upload_X_csr', 'close']
    assert [e[1] for e in log] == [0, 0, 0, 0, 1, 1, 1]
    assert np.array_equal(log[1][2], X.toarray()) and np.array_equal(log[5][2], want.toarray())
    assert log[4][2:] == (np.float64, True)
    assert np.array_equal(out['idf'], idf) and out['W'].shape == (X.shape[0], 2)
    if with_holder:
        assert holder.engine is None and holder.key is None and holder.given == (None, None)


def test_resident_holder_keeps_the_csr_handle(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    X = counts_csr()
    holder = nmf_mod.ResidentProblem()
    for _ in range(3):
        out = run(nmf_mod, X, sparse_X=True, preprocess=('tfidf', 'normalize'), resident=holder)
        assert np.array_equal(out['idf'], np.full(X.shape[1], 0.5))
    assert names(log) == ['init', 'upload_X_csr', 'preprocess'] and holder.reuses == 2
    X2 = counts_csr(seed=5)
    run(nmf_mod, X2, sparse_X=True, preprocess=('tfidf', 'normalize'), resident=holder)
    assert names(log)[3:] == ['close', 'init', 'upload_X_csr', 'preprocess'] and holder.reuses == 2
    holder.close()
    assert names(log)[-1] == 'close'


def test_estimator_asks_the_route_for_a_sparse_X(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    calls = []

    def fake_nmf(X, k, **kw):
        calls.append(kw)
        return {'W': np.zeros((X.shape[0], k)), 'T': np.zeros((k, X.shape[1])), 'idf': None}
    monkeypatch.setattr(si, '_nmf', fake_nmf)
    X = counts_csr()
    make = lambda **kw: si.NMF_TM_Estimator(X.shape[0], X.shape[1], 2, handle_tfidf=True, handle_normalization=True,
                                            keep_resident=True, **kw)
    est = make(nmf_kwargs={'sparse_X': True})
    est.fit(X)
    est.one_iter(X)
    assert calls[0]['resident'] is calls[1]['resident'] is est._resident and est._resident is not None
    est = make(nmf_kwargs={'sparse_X': True})
    est.fit(counts_csr(empty_row=1))                 # the host route: no holder, no error -- as before
    assert 'resident' not in calls[-1]
    est = make(nmf_kwargs={'sparse_X': False})       # densified on the device
    est.fit(counts_csr(empty_row=1))
    assert calls[-1]['resident'] is est._resident
    est = si.NMF_TM_Estimator(X.shape[0], X.shape[1], 2, keep_resident=True, nmf_kwargs={'sparse_X': True})
    est.fit(X)                                       # nothing to preprocess: a sparse X gets no holder, as before
    assert 'resident' not in calls[-1]
    est.fit(X.toarray())
    assert calls[-1]['resident'] is est._resident


# ---- header and binding ---------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_csr_exports():
    import ctypes as C
    from rri_nmf_amd import _capi
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    assert 'matrixops.py:124-179' in text
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'rri_status\s+rri_csr_column_positive_counts\s*\(\s*rri_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*df_out\s*\)\s*;', code)
    assert re.search(r'rri_status\s+rri_csr_scale_X\s*\(\s*rri_ctx\s*\*\s*ctx\s*,\s*const\s+double\s*\*\s*col_scale\s*,\s*int32_t\s+'
                     r'normalize_rows\s*,\s*int64_t\s*\*\s*zero_rows_out\s*\)\s*;', code)
    res, args = _capi.PROTOTYPES['rri_csr_column_positive_counts']
    assert res is C.c_int32 and args == [C.c_void_p, C.POINTER(C.c_double)]
    res, args = _capi.PROTOTYPES['rri_csr_scale_X']
    assert res is C.c_int32 and args == [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int64)]
    assert re.search(r'#define\s+RRI_ABI_VERSION\s+1\b', code) and _capi.ABI_VERSION == 1      # additive
    # the dense pair keeps its signatures
    assert _capi.PROTOTYPES['rri_scale_X'][1] == [C.c_void_p, C.POINTER(C.c_double), C.c_int32]


def test_zero_total_rows_is_a_value_error_with_the_count():
    from rri_nmf_amd.engine import ZeroTotalRows
    e = ZeroTotalRows(3)
    assert isinstance(e, ValueError) and e.count == 3 and '3 row' in str(e)


def test_a_document_of_universal_terms_has_a_zero_tfidf_total():
    """why an empty-row check on the host is not enough: log(n / (n + spacing(1))) is exactly 0.0"""
    from rri_nmf_amd import nmf as nmf_mod
    X = counts_csr().tolil()
    X[:, 3] = 1
    X[5, :] = 0
    X[5, 3] = 7                                      # document 5 holds the one term that every document holds
    X = X.tocsr()
    assert np.all(np.diff(X.indptr) > 0)
    Xt, idf = nmf_mod._preprocess_on_host(X, True, False)
    assert idf[3] == 0.0 and Xt[5].sum() == 0.0
