"""Host side of float16 storage (nmf(..., dtype=np.float16), RRI_F16): what is refused before any engine is made, the route
the preprocessing takes, that float16 is never chosen by itself, and the agreement of header and binding.  No GPU: a recording
engine stands in for RRIEngine where nmf() would make one."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT


class EngineMade(Exception):
    """raised by the stand-in once nmf() has handed it everything this file looks at"""


def recording_engine(log):
    class Recording(object):
        def __init__(self, n, d, k, dtype=np.float32, weighted=False, device=0, stream=None, schedule='gram', sparse_x=False):
            log.append(('init', np.dtype(dtype), bool(weighted), schedule, bool(sparse_x)))
            self.n, self.d, self.k, self.dtype = n, d, k, np.dtype(dtype)

        def upload_X(self, X):
            log.append(('upload_X', np.array(X, copy=True)))
            raise EngineMade()

        def upload_X_csr(self, A):
            log.append(('upload_X_csr', A))
            raise EngineMade()

        def preprocess(self, **kw):
            log.append(('preprocess', kw))

        def close(self):
            log.append(('close',))
    return Recording


@pytest.mark.parametrize('kw, word', [
    (dict(W_mat=np.ones((6, 8))), 'W_mat'),
    (dict(schedule='residual'), "schedule='residual'"),
    (dict(sparse_X=True), 'sparse_X=True'),
    (dict(group=object()), 'group='),
    (dict(W_mat=np.ones((6, 8)), schedule='residual'), "W_mat, schedule='residual'"),
])
def test_float16_refuses_what_rewrites_or_masks_X_before_any_engine(monkeypatch, kw, word):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    X = np.arange(48, dtype=np.float64).reshape(6, 8)
    with pytest.raises(ValueError, match=re.escape(word)) as ei:
        nmf_mod.nmf(X, 2, dtype=np.float16, max_iter=1, **kw)
    assert 'float16' in str(ei.value)
    assert log == []


def test_float16_refuses_a_scipy_sparse_X_and_points_to_sparse_X(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    X = sp.random(6, 8, density=0.5, random_state=0, format='csr')
    with pytest.raises(ValueError, match='sparse_X=True'):
        nmf_mod.nmf(X, 2, dtype=np.float16, max_iter=1)
    assert log == []


@pytest.mark.parametrize('in_dtype', [np.float64, np.float32, np.float16])
def test_float16_preprocesses_on_the_host_in_float64(monkeypatch, in_dtype):
    """tf-idf and normalisation happen in float64 on the host, whatever X is, so that X is rounded once (at upload): the engine
    receives the preprocessed float64 matrix and its own preprocess() is never called"""
    from rri_nmf_amd import nmf as nmf_mod
    from rri_nmf_amd import matrixops
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    rs = np.random.RandomState(0)
    X = rs.randint(0, 6, size=(12, 8)).astype(in_dtype)
    with pytest.raises(EngineMade):
        nmf_mod.nmf(X, 2, dtype=np.float16, preprocess=('tfidf', 'normalize'), max_iter=1)
    assert [e[0] for e in log] == ['init', 'upload_X', 'close']
    assert log[0][1] == np.float16 and log[0][2:] == (False, 'gram', False)
    want = matrixops.normalize(matrixops.tfidf(X))
    got = log[1][1]
    assert got.dtype == np.float64
    assert np.array_equal(got, np.asarray(want, dtype=np.float64))
    # the float32 handle of the same call keeps today's route: raw upload, preprocessing on the device
    log[:] = []
    with pytest.raises(EngineMade):
        nmf_mod.nmf(X.astype(np.float32), 2, dtype=np.float32, preprocess=('tfidf', 'normalize'), max_iter=1)
    assert np.array_equal(log[1][1], X.astype(np.float32))


def test_w_row_is_folded_in_float64_before_the_one_rounding(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    rs = np.random.RandomState(1)
    X = rs.randint(0, 6, size=(12, 8)).astype(np.float64)
    w_row = rs.rand(12, 1) + 0.5
    with pytest.raises(EngineMade):
        nmf_mod.nmf(X, 2, dtype=np.float16, w_row=w_row, max_iter=1)
    assert log[0][1] == np.float16
    assert log[1][1].dtype == np.float64 and np.array_equal(log[1][1], np.sqrt(w_row) * X)


def test_float16_is_never_chosen_for_the_caller(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    assert nmf_mod._storage_dtype(np.ones((2, 2), dtype=np.float16), None) == np.float64
    assert nmf_mod._storage_dtype(np.ones((2, 2), dtype=np.float32), None) == np.float32
    assert nmf_mod._storage_dtype(np.ones((2, 2), dtype=np.float64), np.float16) == np.float16
    log = []
    monkeypatch.setattr(nmf_mod, 'RRIEngine', recording_engine(log))
    with pytest.raises(EngineMade):
        nmf_mod.nmf(np.ones((6, 8), dtype=np.float16), 2, max_iter=1)
    assert log[0][1] == np.float64


def test_header_and_binding_agree_on_the_storage_types():
    from rri_nmf_amd import _capi
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'enum\s*\{\s*(RRI_F32\s*=.*?)\};', text, re.S)
    assert m, 'storage-type enum not found in the header'
    values = dict((k, int(v)) for k, v in re.findall(r'(RRI_F\d+)\s*=\s*(\d+)', m.group(1)))
    assert values == {'RRI_F32': 0, 'RRI_F64': 1, 'RRI_F16': 2}
    assert _capi.RRI_F16 == 2 == values['RRI_F16']
    assert (_capi.RRI_F32, _capi.RRI_F64) == (values['RRI_F32'], values['RRI_F64'])
    assert 'rri_storage_error' in _capi.PROTOTYPES and re.search(r'\brri_storage_error\s*\(', text)


def test_engine_argument_checks_for_float16():
    """the part of RRIEngine.__init__ that runs before the library is opened"""
    from rri_nmf_amd.engine import RRIEngine, check_storage_options, _NP2RRI
    from rri_nmf_amd import _capi
    assert _NP2RRI[np.dtype(np.float16)] == _capi.RRI_F16
    assert check_storage_options(np.float16) == np.float16
    assert check_storage_options('float16', weighted=False, schedule='gram', sparse_x=False) == np.float16
    for kw, word in ((dict(weighted=True), 'weighted=True'), (dict(weighted='sparse'), "weighted='sparse'"),
                     (dict(schedule='residual'), "schedule='residual'"), (dict(sparse_x=True), 'sparse_x=True')):
        with pytest.raises(ValueError, match=re.escape(word)):
            check_storage_options(np.float16, **kw)
        with pytest.raises(ValueError, match='float16'):       # ... and the constructor says so before rri_create is reached
            RRIEngine(10, 16, 2, dtype=np.float16, **kw)
        assert check_storage_options(np.float32, **kw) == np.float32     # no business of this check
    for bad in (np.int32, np.complex64, 'float128' if hasattr(np, 'float128') else np.int8):
        with pytest.raises(ValueError, match='float32, float64 or float16'):
            check_storage_options(bad)


def test_estimator_transform_follows_the_float16_store(monkeypatch):
    """the fold-in uploads the new rows in the store the fit used (as it follows sparse_X), and in no other case"""
    from rri_nmf_amd import sklearn_interface as si
    calls = []

    def fake_nmf(X, k, **kw):
        calls.append(kw)
        return {'W': np.zeros((X.shape[0], k))}
    monkeypatch.setattr(si, '_nmf', fake_nmf)
    X = np.ones((5, 8))
    est = si.NMF_TM_Estimator(5, 8, 2, nmf_kwargs={'dtype': np.float16}, T=np.ones((2, 8)) / 8)
    est.transform(X)
    assert calls[-1]['dtype'] == np.float16 and calls[-1]['fix_T'] is True
    for kwargs in ({}, {'dtype': np.float32}, {'dtype': np.float64}):
        est = si.NMF_TM_Estimator(5, 8, 2, nmf_kwargs=kwargs, T=np.ones((2, 8)) / 8)
        est.transform(X)
        assert 'dtype' not in calls[-1]
