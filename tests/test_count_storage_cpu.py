"""Host side of uint8 count storage (nmf(..., dtype=np.uint8), RRI_U8): what is refused before any engine is made, that the
preprocessing takes the device route on the raw counts, that an empty row is an error and never a change of store, that uint8 is
never chosen by itself, and the agreement of header and binding.  No GPU: a recording engine stands in for RRIEngine where
nmf() would make one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT


class EngineMade(Exception):
    """raised by the stand-in once nmf() has handed it everything this file looks at"""


def recording_engine(log, stop_at='preprocess'):
    class Recording(object):
        def __init__(self, n, d, k, dtype=np.float32, weighted=False, device=0, stream=None, schedule='gram', sparse_x=False):
            log.append(('init', np.dtype(dtype), bool(weighted), schedule, bool(sparse_x)))
            self.n, self.d, self.k, self.dtype = n, d, k, np.dtype(dtype)

        def upload_X(self, X):
            log.append(('upload_X', np.array(X, copy=True)))
            if stop_at == 'upload_X':
                raise EngineMade()

        def upload_X_csr(self, A):
            log.append(('upload_X_csr', A))
            raise EngineMade()

        def attach_group(self, group):
            log.append(('attach_group',))

        def preprocess(self, **kw):
            log.append(('preprocess', kw))
            raise EngineMade()

        def close(self):
            log.append(('close',))
    return Recording


def counts(n=12, d=8, seed=0):
    X = np.random.RandomState(seed).randint(0, 6, size=(n, d))
    X[:, 0] += 1                                     # no empty row
    return X


@pytest.mark.parametrize('kw, word', [
    (dict(W_mat=np.ones((12, 8))), 'W_mat'),
    (dict(schedule='residual'), "schedule='residual'"),
    (dict(sparse_X=True), 'sparse_X=True'),
    (dict(group=object()), 'group='),
    (dict(w_row=np.ones((12, 1))), 'w_row'),
    (dict(W_mat=np.ones((12, 8)), schedule='residual', w_row=np.ones((12, 1))), "W_mat, schedule='residual', w_row"),
])
def test_uint8_refuses_what_rewrites_masks_or_reweights_X_before_any_engine(monkeypatch, kw, word):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    with pytest.raises(ValueError, match=re.escape(word)) as ei:
        nmf_mod.nmf(counts(), 2, dtype=np.uint8, max_iter=1, **kw)
    assert 'uint8' in str(ei.value)
    assert log == []


def test_uint8_refuses_a_scipy_sparse_X_and_points_to_sparse_X(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    X = sp.csr_matrix(counts().astype(np.float64))
    with pytest.raises(ValueError, match='sparse_X=True'):
        nmf_mod.nmf(X, 2, dtype=np.uint8, max_iter=1)
    assert log == []


@pytest.mark.parametrize('in_dtype', [np.float64, np.float32, np.uint8, np.int64])
@pytest.mark.parametrize('callbacks', [False, True])
def test_uint8_preprocesses_on_the_device_from_the_raw_counts(monkeypatch, in_dtype, callbacks):
    """the engine receives the counts as they are and its own preprocess() is called with what was asked for -- also with host
    callbacks, which send every other store through the host route"""
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    X = counts().astype(in_dtype)
    extra = dict(diagnostics=[lambda X, W, T: 0.0], store_gradients=True) if callbacks else {}
    with pytest.raises(EngineMade):
        nmf_mod.nmf(X, 2, dtype=np.uint8, preprocess=('tfidf', 'normalize'), max_iter=1, **extra)
    assert [e[0] for e in log] == ['init', 'upload_X', 'preprocess', 'close']
    assert log[0][1] == np.uint8 and log[0][2:] == (False, 'gram', False)
    assert np.array_equal(log[1][1], X) and log[1][1].dtype == X.dtype
    assert log[2][1] == {'tfidf': True, 'normalize': True}
    # the same call on a float32 store with callbacks keeps today's route: matrixops on the host, no preprocess() on the engine
    if callbacks:
        log[:] = []
        monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log, stop_at='upload_X'))
        with pytest.raises(EngineMade):
            nmf_mod.nmf(X.astype(np.float32), 2, dtype=np.float32, preprocess=('tfidf', 'normalize'), max_iter=1, **extra)
        assert [e[0] for e in log] == ['init', 'upload_X', 'close']
        assert not np.array_equal(log[1][1], X)


def test_preprocess_route_keeps_every_existing_answer():
    from rri_nmf_amd.nmf import preprocess_route
    import itertools
    names = ('normalize', 'has_empty_row', 'W_mat', 'w_row', 'host_callbacks', 'half')
    for csr, xs in itertools.product((False, True), repeat=2):
        for flags in itertools.product((False, True), repeat=len(names)):
            kw = dict(zip(names, flags))
            assert preprocess_route(csr, xs, counts=False, **kw) == preprocess_route(csr, xs, **kw)
    assert preprocess_route(False, False, normalize=True, host_callbacks=True) == 'host'
    assert preprocess_route(False, False, normalize=True, host_callbacks=True, counts=True) == 'device'
    assert preprocess_route(False, False, normalize=True, counts=True) == 'device'


@pytest.mark.parametrize('in_dtype', [np.float64, np.uint8])
def test_an_empty_row_with_normalisation_is_an_error_and_no_other_store_is_tried(monkeypatch, in_dtype):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    X = counts().astype(in_dtype)
    X[3] = 0
    X[7] = 0
    with pytest.raises(ValueError, match=r'\b2 row') as ei:
        nmf_mod.nmf(X, 2, dtype=np.uint8, preprocess=('tfidf', 'normalize'), max_iter=1)
    assert 'uint8' in str(ei.value)
    assert log == []
    # without normalisation an empty row is a row of zeros like any other
    with pytest.raises(EngineMade):
        nmf_mod.nmf(X, 2, dtype=np.uint8, preprocess=('tfidf',), max_iter=1)
    assert log[0][1] == np.uint8 and log[2][1] == {'tfidf': True, 'normalize': False}


def test_rows_whose_tfidf_total_is_zero_raise_with_their_number(monkeypatch):
    """what the device reports (ZeroTotalRows from preprocess()) becomes a ValueError that names the rows: no host fallback"""
    from rri_nmf_amd import nmf as nmf_mod
    from rri_nmf_amd.engine import ZeroTotalRows
    log = []
    Rec = recording_engine(log)

    def refuse(self, **kw):
        log.append(('preprocess', kw))
        raise ZeroTotalRows(3)
    Rec.preprocess = refuse
    monkeypatch.setattr(nmf_mod, 'RRIEngine', Rec)
    with pytest.raises(ValueError, match=r'\b3 row') as ei:
        nmf_mod.nmf(counts(), 2, dtype=np.uint8, preprocess=('tfidf', 'normalize'), max_iter=1)
    assert 'uint8' in str(ei.value)
    assert [e[0] for e in log] == ['init', 'upload_X', 'preprocess', 'close']        # one engine, closed; none after it


def test_uint8_is_never_chosen_for_the_caller(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    assert nmf_mod._storage_dtype(np.ones((2, 2), dtype=np.uint8), None) == np.float64
    assert nmf_mod._storage_dtype(np.ones((2, 2), dtype=np.float64), np.uint8) == np.uint8
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log, stop_at='upload_X'))
    with pytest.raises(EngineMade):
        nmf_mod.nmf(np.ones((6, 8), dtype=np.uint8), 2, max_iter=1)
    assert log[0][1] == np.float64
    log[:] = []
    with pytest.raises(EngineMade):          # ... and device preprocessing of a uint8 input stores float64, as for every other input
        nmf_mod.nmf(np.ones((6, 8), dtype=np.uint8), 2, max_iter=1, preprocess=('normalize',))
    assert log[0][1] == np.float64


def test_header_and_binding_agree_on_RRI_U8_and_the_scale_calls():
    """RRI_U8 is 4, not the 3 first planned for it: tests/test_half_storage_gpu.py holds rri_create to refusing code 3 as no
    storage type, so that code stays unassigned"""
    from rri_nmf_amd import _capi
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'enum\s*\{\s*(RRI_F32\s*=.*?)\};', text, re.S)
    assert m, 'storage-type enum not found in the header'
    values = dict((k, int(v)) for k, v in re.findall(r'(RRI_[FU]\d+)\s*=\s*(\d+)', m.group(1)))
    assert values == {'RRI_F32': 0, 'RRI_F64': 1, 'RRI_F16': 2, 'RRI_U8': 4}
    assert _capi.RRI_U8 == 4
    D = C.POINTER(C.c_double)
    for name in ('rri_set_X_scales', 'rri_get_X_scales'):
        res, args = _capi.PROTOTYPES[name]
        assert res is C.c_int32 and args == [C.c_void_p, D, D]
    assert re.search(r'rri_status\s+rri_set_X_scales\s*\(\s*rri_ctx\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*\)\s*;', text)
    assert re.search(r'rri_status\s+rri_get_X_scales\s*\(\s*rri_ctx\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*\)\s*;', text)


def test_engine_argument_checks_for_uint8():
    """the part of RRIEngine.__init__ that runs before the library is opened"""
    from rri_nmf_amd.engine import RRIEngine, check_storage_options, _NP2RRI
    from rri_nmf_amd import _capi
    assert _NP2RRI[np.dtype(np.uint8)] == _capi.RRI_U8
    assert check_storage_options(np.uint8) == np.uint8
    assert check_storage_options('uint8', weighted=False, schedule='gram', sparse_x=False) == np.uint8
    for kw, word in ((dict(weighted=True), 'weighted=True'), (dict(weighted='sparse'), "weighted='sparse'"),
                     (dict(schedule='residual'), "schedule='residual'"), (dict(sparse_x=True), 'sparse_x=True')):
        with pytest.raises(ValueError, match=re.escape(word)):
            check_storage_options(np.uint8, **kw)
        with pytest.raises(ValueError, match='uint8'):         # ... and the constructor says so before rri_create is reached
            RRIEngine(10, 16, 2, dtype=np.uint8, **kw)
    for bad in (np.int8, np.uint16, np.int32, np.bool_):
        with pytest.raises(ValueError, match='float32, float64 or float16'):
            check_storage_options(bad)


def test_estimator_transform_follows_the_uint8_store(monkeypatch):
    """the fold-in uploads the new rows in the store the fit used (as it follows float16 and sparse_X), and in no other case"""
    from rri_nmf_amd import sklearn_interface as si
    calls = []

    def fake_nmf(X, k, **kw):
        calls.append(kw)
        return {'W': np.zeros((X.shape[0], k)), 'T': np.ones((k, X.shape[1])) / X.shape[1], 'idf': np.ones(X.shape[1]),
                'iter_cputime': [0.0], 'random_state': 0, 'n_resets_used': 0}
    monkeypatch.setattr(si, '_nmf', fake_nmf)
    X = np.ones((5, 8))
    est = si.NMF_TM_Estimator(5, 8, 2, nmf_kwargs={'dtype': np.uint8}, T=np.ones((2, 8)) / 8)
    est.transform(X)
    assert calls[-1]['dtype'] == np.uint8 and calls[-1]['fix_T'] is True
    est = si.NMF_TM_Estimator(5, 8, 2, nmf_kwargs={'dtype': 'uint8'}, T=np.ones((2, 8)) / 8)
    est.transform(X)
    assert calls[-1]['dtype'] == np.uint8
    for kwargs in ({}, {'dtype': np.float32}, {'dtype': np.float64}):
        est = si.NMF_TM_Estimator(5, 8, 2, nmf_kwargs=kwargs, T=np.ones((2, 8)) / 8)
        est.transform(X)
        assert 'dtype' not in calls[-1]
