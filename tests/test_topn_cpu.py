"""Top-N rows without a GPU: the order and the request validation of rri_nmf_amd/csrc/rri_topn.hpp under sanitizers, the ABI
surface, and the plumbing of NMF_RS_Estimator.recommend with stand-ins for the solver and the device handle.

tests/c/topn_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once: 60 seeded streams (three values only; mostly
distinct; NaN, both infinities and ties), each offered pair by pair in a permuted order to topn_insert at N = 1, 2, 10, 64 and
lengths 0, 1, 5, 64, 300.  The lists it prints are compared with the restatement of tests/topn_cases.py (np.lexsort((j, -s)))."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import topn_cases as tc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUESTS = {'all_rows': 0, 'listed_rows_with_duplicates': 0, 'longest_list': 0, 'no_rows': 0, 'exclusion': 0,
            'exclusion_all_rows': 0, 'empty_exclusion': 0,
            'negative_count': _capi.RRI_ERR_INVALID, 'topn_zero': _capi.RRI_ERR_UNSUPPORTED,
            'topn_too_long': _capi.RRI_ERR_UNSUPPORTED, 'more_rows_than_W_has': _capi.RRI_ERR_INVALID,
            'row_n': _capi.RRI_ERR_INVALID, 'row_negative': _capi.RRI_ERR_INVALID, 'indptr_not_from_zero': _capi.RRI_ERR_INVALID,
            'indptr_decreases': _capi.RRI_ERR_INVALID, 'indices_null': _capi.RRI_ERR_INVALID, 'column_d': _capi.RRI_ERR_INVALID,
            'column_negative': _capi.RRI_ERR_INVALID, 'column_twice': _capi.RRI_ERR_INVALID,
            'columns_descend': _capi.RRI_ERR_INVALID}


def as_double(bits):
    return struct.unpack('<d', struct.pack('<Q', int(bits, 16)))[0]


def pairs(text):
    out = [p.split(':') for p in text.split()]
    return np.array([int(j) for j, _ in out], dtype=np.int64), np.array([as_double(b) for _, b in out], dtype=np.float64)


def test_insertion_order_and_request_validation_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'topn')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'topn_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok 60 streams', lines[-1]

    streams = {}
    for ln in lines:
        if ln.startswith('stream '):
            head, body = ln[7:].split(' :')
            sid, N, length = (int(x) for x in head.split())
            j, v = pairs(body)
            assert j.size == length and sorted(j) == list(range(length))      # every column once, in some order
            streams[sid] = (N, j, v)
    assert len(streams) == 60 and {s[0] for s in streams.values()} == {1, 2, 10, 64}
    assert any(np.isnan(v).any() and np.isinf(v).any() for _, _, v in streams.values())
    assert any(v.size == 300 and np.unique(v).size <= 3 for _, _, v in streams.values())          # heavy ties
    checked = 0
    for ln in lines:
        if not ln.startswith('list '):
            continue
        head, body = ln[5:].split(' :')
        N, j, v = streams[int(head)]
        got_j, got_v = pairs(body)
        s = np.empty(j.size)
        s[j] = v                                                            # the scores by column
        want_j, want_v = tc.topn_from_scores(s[None, :], N, np.zeros((1, s.size), dtype=bool))
        assert np.array_equal(got_j, want_j[0]), ln
        assert np.array_equal(got_v, want_v[0], equal_nan=True), ln
        checked += 1
    assert checked == 60

    clips = [ln for ln in lines if ln.startswith('clip ')]
    assert len(clips) == 20
    for ln in clips:
        v, lo, hi, got = (as_double(b) for b in ln[5:].replace(':', ' ').split())
        assert got == tc.clip_values([v], (lo, hi))[0] == tc.clip_values([v], (None if np.isnan(lo) else lo, None if np.isnan(hi) else hi))[0], ln

    got = dict(re.match(r'req (\w+) : (-?\d+)$', ln).groups() for ln in lines if ln.startswith('req '))
    assert {name: int(code) for name, code in got.items()} == REQUESTS


def gpu_present():
    lib = _capi.load_library()
    h = ctypes.c_void_p()
    st = lib.rri_create(ctypes.byref(h), 4, 4, 2, 0, 0, 0, None)
    if st == 0:
        lib.rri_destroy(h)
    return st == 0


def test_the_entry_point_is_declared_bound_and_refuses_a_null_handle():
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    assert re.search(r'^#define RRI_MAX_TOPN 64$', text, flags=re.M) and _capi.RRI_MAX_TOPN == 64
    assert re.search(r'#define RRI_ABI_VERSION 1\b', text) and _capi.ABI_VERSION == 1          # an addition, not a new ABI
    res, args = _capi.PROTOTYPES['rri_topn_rows']
    I64P, I32P, DP = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    assert res is ctypes.c_int32
    assert args == [ctypes.c_void_p, I64P, ctypes.c_int64, ctypes.c_int32, I64P, I32P, ctypes.c_double, ctypes.c_double, I32P, DP]
    lib = _capi.load_library()
    idx, val = (ctypes.c_int32 * 4)(), (ctypes.c_double * 4)()
    assert lib.rri_topn_rows(None, None, 2, 2, None, None, float('nan'), float('nan'), idx, val) == _capi.RRI_ERR_INVALID
    for doc in ('INTEGRATION.md', 'README.md', 'DESIGN.md'):
        assert 'rri_topn_rows' in open(os.path.join(ROOT, doc)).read(), doc
    if not gpu_present():       # no host route: the estimator's call needs the device like everything else
        from rri_nmf_amd import sklearn_interface as si
        E = si.NMF_RS_Estimator(4, 3, 2, W=np.ones((4, 2)), T=np.ones((2, 3)))
        with pytest.raises(_capi.RRIHipUnavailable):
            E.recommend(exclude_seen=False)


class FakeEngine(object):
    """stands in for RRIEngine behind NMF_RS_Estimator.recommend: answers from the restatement and keeps a log"""
    log = []

    def __init__(self, n, d, k, **kw):
        self.shape, self.kw, self.closed, self.calls = (n, d, k), kw, False, []
        FakeEngine.log.append(self)

    def set_W(self, W):
        assert isinstance(W, np.ndarray) and W.shape == (self.shape[0], self.shape[2])
        self.W = W

    def set_T(self, T):
        assert isinstance(T, np.ndarray) and T.shape == (self.shape[2], self.shape[1])
        self.T = T

    def topn_rows(self, rows=None, n_top=10, exclude=None, clip=(None, None)):
        assert not self.closed
        self.calls.append((np.array(rows), n_top, exclude, clip))
        return tc.topn_reference(self.W, self.T, rows, n_top, exclude, clip)

    def close(self):
        self.closed = True


def test_recommend_plumbing_with_stand_ins(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    n, d, k = 23, 11, 3
    rng = np.random.RandomState(5)

    def fake_nmf(X, kk, **kw):
        assert sp.issparse(X) and X.shape == (n, d)
        r = np.random.RandomState(kw.get('random_state', 0))
        return {'W': r.rand(n, kk), 'T': r.rand(kk, d), 'obj_history': []}
    monkeypatch.setattr(si._nmf_module, 'nmf', fake_nmf)
    monkeypatch.setattr(si, 'RRIEngine', FakeEngine)
    FakeEngine.log = []

    mask = rng.rand(n, d) < 0.4
    ij = np.column_stack(np.nonzero(mask))
    ij = np.vstack([ij[rng.permutation(len(ij))], ij[:3]])       # any order, three pairs twice
    y = rng.randint(1, 6, size=len(ij)).astype(np.float64)
    y[0] = 0.0                                                    # a rating of zero is still a pair that was given
    for hold_out in (True, False):
        E = si.NMF_RS_Estimator(n, d, k, use_validation_early_stopping=hold_out, nmf_kwargs={'device': 3}).fit(ij, y)
        assert sp.issparse(E.seen_) and E.seen_.shape == (n, d) and E.seen_.has_sorted_indices
        assert np.array_equal(E.seen_.toarray() != 0, mask) and E.seen_.nnz == mask.sum()     # the hold-out included

        items, sc = E.recommend(n_items=4)
        eng = FakeEngine.log[-1]
        assert eng.shape == (n, d, k) and eng.kw == dict(dtype=np.float64, weighted=False, device=3) and eng.closed
        assert len(eng.calls) == 1 and eng.calls[0][3] == (E.min_rating, E.max_rating) == (0.0, 5.0)
        want = tc.topn_reference(E.W, E.T, None, 4, E.seen_, (0.0, 5.0))
        assert np.array_equal(items, want[0]) and np.array_equal(sc, want[1], equal_nan=True)
        assert items.dtype == np.int32 and sc.dtype == np.float64
        for i in range(n):
            assert not mask[i, items[i][items[i] >= 0]].any()
        # the scores are what predict gives for those pairs
        ii, jj = np.nonzero(items >= 0)
        assert np.allclose(E.predict(np.column_stack((ii, items[ii, jj])).astype(float)), sc[ii, jj], rtol=0, atol=1e-12)

        # chunks of at most _RECOMMEND_CHUNK users, one handle for all of them
        monkeypatch.setattr(si, '_RECOMMEND_CHUNK', 7)
        items7, sc7 = E.recommend(n_items=4)
        eng = FakeEngine.log[-1]
        assert [c[0].size for c in eng.calls] == [7, 7, 7, 2] and eng.closed
        assert np.array_equal(np.concatenate([c[0] for c in eng.calls]), np.arange(n))
        assert all(c[2].shape == (c[0].size, d) for c in eng.calls)
        assert np.array_equal(items7, items) and np.array_equal(sc7, sc, equal_nan=True)
        # a subset in any order, with duplicates, across a chunk border
        users = np.array([5, 0, 22, 5, 5, 9, 1, 1, 17])
        it_u, sc_u = E.recommend(users, n_items=4)
        assert np.array_equal(it_u, items[users]) and np.array_equal(sc_u, sc[users], equal_nan=True)
        assert [c[0].size for c in FakeEngine.log[-1].calls] == [7, 2]
        monkeypatch.setattr(si, '_RECOMMEND_CHUNK', 1 << 20)
        assert si._RECOMMEND_CHUNK == 2 ** 20

        # nothing excluded
        it_all, sc_all = E.recommend(users, n_items=d + 2, exclude_seen=False)
        assert FakeEngine.log[-1].calls[0][2] is None
        want = tc.topn_reference(E.W, E.T, users, d + 2, None, (0.0, 5.0))
        assert np.array_equal(it_all, want[0]) and np.all(it_all[:, d:] == -1) and np.all(np.isnan(sc_all[:, d:]))
        # no users: two empty arrays
        it0, sc0 = E.recommend([], n_items=4)
        assert it0.shape == (0, 4) and sc0.shape == (0, 4)

        # sparsified factors are densified on copies: the estimator keeps its sparse ones
        E.sparsify()
        it_s, sc_s = E.recommend(n_items=4)
        assert sp.issparse(E.W) and sp.issparse(E.T)
        assert np.array_equal(it_s, items) and np.array_equal(sc_s, sc, equal_nan=True)
        E.densify()

        with pytest.raises(ValueError, match='row indices'):
            E.recommend([0, n])
        with pytest.raises(ValueError, match='row indices'):
            E.recommend([-1])
        del E.seen_
        with pytest.raises(ValueError, match='seen_'):
            E.recommend()
        assert E.recommend(exclude_seen=False)[0].shape == (n, 10)
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_RS_Estimator(n, d, k).recommend()
