"""Host side of the uniform rows of a CSR-resident X (nmf(..., uniform_rows=True); rri_set_uniform_rows, rri_get_uniform_rows,
rri_csr_scale_X_uniform): header and binding, the answers of nmf.preprocess_route, what nmf() asks of the engine when a matrix
has an empty document, and what the option refuses.  No GPU: the recording engine of test_sparse_preprocess_cpu.py stands in for
RRIEngine where nmf() would make one."""
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_sparse_preprocess_cpu import counts_csr, names, recording_engine, run


def test_header_and_binding_agree_on_the_uniform_row_exports():
    import ctypes as C
    from rri_nmf_amd import _capi
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    ws = lambda s: re.sub(r'\s+', r'\\s*', s)
    assert re.search(ws(r'rri_status rri_set_uniform_rows \( rri_ctx \* ctx , const\s+int32_t \* rows , int64_t\s+count , '
                        r'double\s+value \) ;'), code)
    assert re.search(ws(r'rri_status rri_get_uniform_rows \( rri_ctx \* ctx , int32_t \* rows_out , int64_t\s+capacity , '
                        r'int64_t \* count_out , double \* value_out \) ;'), code)
    assert re.search(ws(r'rri_status rri_csr_scale_X_uniform \( rri_ctx \* ctx , const\s+double \* col_scale , int32_t\s+'
                        r'normalize_rows , int64_t \* uniform_rows_out \) ;'), code)
    P = _capi.PROTOTYPES
    assert P['rri_set_uniform_rows'] == (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.c_int64, C.c_double])
    assert P['rri_get_uniform_rows'] == (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64),
                                                     C.POINTER(C.c_double)])
    assert P['rri_csr_scale_X_uniform'] == (C.c_int32, [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int64)])
    assert P['rri_csr_scale_X_uniform'][1] == P['rri_csr_scale_X'][1]
    assert re.search(r'#define\s+RRI_ABI_VERSION\s+1\b', code) and _capi.ABI_VERSION == 1      # additive


def test_route_with_uniform_rows():
    from rri_nmf_amd.nmf import preprocess_route
    assert preprocess_route(True, True, normalize=True, has_empty_row=True, uniform_rows=True) == 'device'
    assert preprocess_route(True, False, normalize=True, has_empty_row=True, uniform_rows=True) == 'device'
    assert preprocess_route(True, True, normalize=True, has_empty_row=True) == 'host'
    # what needs the preprocessed X on the host keeps the host route
    assert preprocess_route(True, True, normalize=True, has_empty_row=True, uniform_rows=True, host_callbacks=True) == 'host'
    # every answer with uniform_rows=False is the answer without the argument
    flags = ('normalize', 'has_empty_row', 'W_mat', 'w_row', 'host_callbacks', 'half', 'counts')
    for csr, sparse in ((False, False), (False, True), (True, False), (True, True)):
        for bits in itertools.product((False, True), repeat=len(flags)):
            kw = dict(zip(flags, bits))
            assert preprocess_route(csr, sparse, uniform_rows=False, **kw) == preprocess_route(csr, sparse, **kw), (csr, sparse, kw)
    assert preprocess_route(False, False, normalize=True, group=True, uniform_rows=False) == 'device'
    for kw in (dict(x_is_sparse=True), dict(x_is_sparse=False, W_mat=True)):
        with pytest.raises(NotImplementedError):
            preprocess_route(False, group=True, uniform_rows=False, **kw)


def test_route_of_a_call_with_uniform_rows():
    from rri_nmf_amd import nmf as nmf_mod
    X = counts_csr(empty_row=3)
    assert nmf_mod._route_of_call(X, (True, True), sparse_X=True) == ('host', True)
    assert nmf_mod._route_of_call(X, (True, True), sparse_X=True, uniform_rows=True) == ('device', True)
    assert nmf_mod._route_of_call(X, (True, True), sparse_X=True, uniform_rows=False) == ('host', True)


def test_an_empty_row_stays_on_the_device_with_uniform_rows(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    host = []
    real = nmf_mod._preprocess_on_host
    monkeypatch.setattr(nmf_mod, '_preprocess_on_host', lambda *a, **kw: (host.append(1), real(*a, **kw))[1])
    X = counts_csr(empty_row=4)
    assert np.diff(X.indptr)[4] == 0
    holder = nmf_mod.ResidentProblem()
    out = run(nmf_mod, X, sparse_X=True, preprocess=('tfidf', 'normalize'), uniform_rows=True, resident=holder)
    assert names(log) == ['init', 'upload_X_csr', 'preprocess']           # one engine, not closed: the holder keeps it
    assert log[0][2:] == (np.float64, True)
    assert np.array_equal(log[1][2], X.toarray())                        # the RAW counts
    assert log[2][2] == {'tfidf': True, 'normalize': True, 'uniform_rows': True}
    assert host == []                                                     # never preprocessed on the host
    assert holder.engine is not None and holder.reuses == 0
    assert np.array_equal(out['idf'], np.full(X.shape[1], 0.5))
    run(nmf_mod, X, sparse_X=True, preprocess=('tfidf', 'normalize'), uniform_rows=True, resident=holder)
    assert names(log) == ['init', 'upload_X_csr', 'preprocess'] and holder.reuses == 1
    # the option is part of the resident key: without it the same holder starts again (and here takes the host route's refusal)
    with pytest.raises(ValueError, match='resident'):
        run(nmf_mod, X, sparse_X=True, preprocess=('tfidf', 'normalize'), resident=holder)
    holder.close()
    # a matrix without such a row: the same handle, the same key rule
    log[:] = []
    holder = nmf_mod.ResidentProblem()
    Y = counts_csr()
    run(nmf_mod, Y, sparse_X=True, preprocess=('tfidf', 'normalize'), uniform_rows=True, resident=holder)
    run(nmf_mod, Y, sparse_X=True, preprocess=('tfidf', 'normalize'), resident=holder)
    assert names(log) == ['init', 'upload_X_csr', 'preprocess', 'close', 'init', 'upload_X_csr', 'preprocess']
    assert 'uniform_rows' not in log[6][2] and holder.reuses == 0
    holder.close()


def test_default_calls_do_not_mention_the_option(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    for flag in (None, False):
        log[:] = []
        run(nmf_mod, counts_csr(), sparse_X=True, preprocess=('tfidf', 'normalize'), uniform_rows=flag)
        assert log[2][2] == {'tfidf': True, 'normalize': True}
        log[:] = []
        run(nmf_mod, counts_csr(empty_row=4), sparse_X=True, preprocess=('tfidf', 'normalize'), uniform_rows=flag)
        assert names(log) == ['init', 'upload_X_csr', 'close']             # the host route, as before


@pytest.mark.parametrize('kw, word', [
    (dict(W_mat=np.ones((12, 9))), 'W_mat'),
    (dict(w_row=np.ones((12, 1))), 'w_row'),
    (dict(group=object()), 'group='),
    (dict(schedule='residual'), "schedule='residual'"),
    (dict(dtype=np.float16), 'float16'),
    (dict(dtype=np.uint8), 'uint8'),
    (dict(diagnostics=[lambda *a, **k: 0]), 'host callbacks'),
    (dict(store_gradients=True), 'host callbacks'),
    (dict(early_stop=lambda *a, **k: False), 'host callbacks'),
    (dict(sparse_X=False), 'sparse_X=False'),
])
def test_refusals_of_uniform_rows(monkeypatch, kw, word):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    X = counts_csr(empty_row=4)
    args = dict(sparse_X=True, preprocess=('tfidf', 'normalize'), uniform_rows=True)
    args.update(kw)
    with pytest.raises(ValueError, match='uniform_rows=True.*' + re.escape(word)):
        run(nmf_mod, X.toarray() if 'dtype' in kw else X, **args)
    assert log == []


def test_uniform_rows_needs_the_csr_handle(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    monkeypatch.setattr(nmf_mod, '_device_free_bytes', lambda device: 1 << 40)      # the automatic route densifies
    X = counts_csr(empty_row=4)
    for extra in (dict(preprocess=('tfidf', 'normalize')), dict()):
        with pytest.raises(ValueError, match='uniform_rows=True needs an X kept as CSR'):
            run(nmf_mod, X, uniform_rows=True, **extra)
        with pytest.raises(ValueError, match='uniform_rows=True needs an X kept as CSR'):
            run(nmf_mod, X.toarray(), uniform_rows=True, **extra)
    assert log == []
    monkeypatch.setattr(nmf_mod, '_device_free_bytes', lambda device: 16)           # ... or keeps a sparse X as CSR
    run(nmf_mod, X, uniform_rows=True, preprocess=('tfidf', 'normalize'))
    assert names(log) == ['init', 'upload_X_csr', 'preprocess', 'close'] and log[0][3] is True and log[2][2]['uniform_rows'] is True
    with pytest.raises(ValueError, match='must be True, False or None'):
        run(nmf_mod, X, sparse_X=True, uniform_rows=1)


def test_estimator_passes_the_option_on(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    calls = []

    def fake_nmf(X, k, **kw):
        calls.append(kw)
        return {'W': np.zeros((X.shape[0], k)), 'T': np.zeros((k, X.shape[1])), 'idf': np.ones(X.shape[1])}
    monkeypatch.setattr(si, '_nmf', fake_nmf)
    X = counts_csr(empty_row=1)
    est = si.NMF_TM_Estimator(X.shape[0], X.shape[1], 2, handle_tfidf=True, handle_normalization=True, keep_resident=True,
                              nmf_kwargs={'sparse_X': True, 'uniform_rows': True})
    est.fit(X)
    est.one_iter(X)
    assert calls[0]['uniform_rows'] is True and calls[1]['uniform_rows'] is True
    assert calls[0]['resident'] is calls[1]['resident'] is est._resident and est._resident is not None      # the holder is kept
    est.transform(X)
    assert calls[2]['uniform_rows'] is True and calls[2]['sparse_X'] is True and calls[2]['fix_T'] is True
    est = si.NMF_TM_Estimator(X.shape[0], X.shape[1], 2, handle_tfidf=True, handle_normalization=True, nmf_kwargs={'sparse_X': True})
    est.fit(X)
    est.transform(X)
    assert 'uniform_rows' not in calls[-1] and 'uniform_rows' not in calls[-2]


def test_row_indices_are_not_wrapped_into_int32():
    """RRIEngine.set_uniform_rows hands int32 to the library: an index beyond int32 (2^32 + 1 would wrap to row 1) or one that is
    no integer is refused on the way, and what fits arrives unchanged"""
    from rri_nmf_amd.engine import RRIEngine
    got = []

    class Lib:
        @staticmethod
        def rri_set_uniform_rows(h, ptr, count, value):
            got.append(([ptr[q] for q in range(count)], value))
            return 0

    e = object.__new__(RRIEngine)
    e._lib, e._h, e.n, e._check = Lib, None, 100, lambda status: None
    for rows in ([2 ** 32 + 1], [3, -2 ** 31 - 1], np.array([2 ** 32 + 1], dtype=np.uint64), np.array([2 ** 31], dtype=np.int64)):
        with pytest.raises(ValueError, match='out of range'):
            e.set_uniform_rows(rows, 0.5)
    for rows in ([1.0], [1.5], ['3']):
        with pytest.raises(ValueError, match='integers'):
            e.set_uniform_rows(rows, 0.5)
    assert got == []
    e.set_uniform_rows(np.array([7, 2], dtype=np.int64), 0.25)
    e.set_uniform_rows([], 0.5)
    e.set_uniform_rows(np.array([5], dtype=np.uint8), 1)
    assert got == [([7, 2], 0.25), ([], 0.5), ([5], 1.0)]
