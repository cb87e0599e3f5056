"""The recommender fit from a resident corpus without a GPU: the term, the clip, the request check and the plain loop of
rri_nmf_amd/csrc/rri_fiterr.hpp under sanitizers, the ABI surface of include/rri_corpus_fit.h and the refusals of the real library
without a handle, the plumbing of nmf(corpus, observed_only=True) and of an early stop on a resident held-out corpus behind
stand-ins for the device, and NMF_RS_Estimator.fit_corpus / score_corpus behind a stand-in solver.

tests/c/fiterr_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once; what it prints is compared with what is written
here by hand and with the numpy restatement (tests/fiterr_cases.py).  No sanitizer is loaded into Python."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import fiterr_cases as fc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD, UNSUPPORTED = 0, _capi.RRI_ERR_INVALID, _capi.RRI_ERR_UNSUPPORTED
INF = float('inf')

REQUESTS = {'fine': OK, 'rows_null': OK, 'duplicate_rows': OK, 'open': OK, 'lo_is_hi': OK, 'no_requests': OK, 'widest_d': OK,
            'd_too_wide': UNSUPPORTED, 'lo_nan': BAD, 'hi_nan': BAD, 'lo_above_hi': BAD, 'other_columns': BAD,
            'rows_null_corpus_above_n': BAD, 'row_n': BAD, 'row_negative': BAD}
TEXT = {'d_too_wide': 'a full row of d = 5592406 entries does not fit the budget of 67108864 bytes',
        'lo_nan': 'a clip bound is NaN (an open side is -inf or +inf)', 'hi_nan': 'a clip bound is NaN (an open side is -inf or +inf)',
        'lo_above_hi': 'clip_lo 5.5 is above clip_hi 5', 'other_columns': 'the corpus has 7 columns, W T has 6',
        'rows_null_corpus_above_n': 'rows is NULL and the corpus has 3 rows, W has 2', 'row_n': 'rows[1] = 4 is out of range',
        'row_negative': 'rows[2] = -1 is out of range'}
RULES = 6       # d, NaN bound, lo above hi, columns, rows NULL, row range
# (clipped prediction, term) of fiterr_main.cpp's cases, by hand
TERMS = {'inside': (2.5, -0.5), 'below': (1.0, -2.0), 'above': (5.0, 2.0), 'at_lo': (1.0, 0.0), 'at_hi': (5.0, 1.0),
         'open': (-7.5, -5.5), 'open_below': (-7.5, -9.5), 'open_above': (1e300, 1e300), 'lo_is_hi': (3.0, 1.0),
         'negative_value': (0.5, 2.0), 'nan_p': (np.nan, np.nan), 'nan_p_open': (np.nan, np.nan)}
# the 3 x 4 case: W T = [[2, 2, 2, 8.5], [0.5, 0, 1, 0.25], [3.5, 1, 6, 5.5]]; the corpus's rows hold the columns (0, 2, 3), (), (1, 3)
# with the values (3, -1, 4.5), (), (2, 0.25)
W34 = np.array([[1.0, 2.0], [0.5, 0.0], [3.0, 1.0]])
T34 = np.array([[1.0, 0.0, 2.0, 0.5], [0.5, 1.0, 0.0, 4.0]])
A34 = sp.csr_matrix((np.array([3.0, -1.0, 4.5, 2.0, 0.25]), np.array([0, 2, 3, 1, 3], dtype=np.int32), np.array([0, 3, 3, 5], dtype=np.int64)),
                    shape=(3, 4))
PLAIN = {0: dict(rows=[2, 0, 1], clip=(-INF, INF), sq=[50.25, 0.0, 4.0], abs=[8.5, 0.0, 2.0], pred=[3.5, 6.0, 5.5, 0.0, 0.25]),
         1: dict(rows=[2, 0, 1], clip=(1.0, 5.0), sq=[36.5, 0.0, 1.5625], abs=[7.0, 0.0, 1.75], pred=[3.5, 5.0, 5.0, 1.0, 1.0]),
         2: dict(rows=None, clip=(2.0, 2.0), sq=[16.25, 0.0, 3.0625], abs=[6.5, 0.0, 1.75], pred=[2.0, 2.0, 2.0, 2.0, 2.0])}


def test_term_clip_request_check_and_plain_loop_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'fiterr')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'fiterr_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok', lines[-1]

    # the clip and the term: inside, at and beyond each bound, open sides, lo = hi, a negative value, a NaN prediction
    terms = {ln.split()[1]: tuple(float(x) for x in ln.split(' : ')[1].split()) for ln in lines if ln.startswith('term ')}
    assert set(terms) == set(TERMS)
    for name, want in TERMS.items():
        assert np.array_equal(terms[name], want, equal_nan=True), (name, terms[name])

    # the request check, rule by rule: the verdict, and a text for every broken rule
    got = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'req (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    assert {name: code for name, (code, _) in got.items()} == REQUESTS
    for name, (code, text) in got.items():
        assert (text == '') == (code == OK), name
        if code != OK:
            assert text == TEXT[name], (name, text)
    assert len({re.sub(r'-?\d[\w.+-]*', '#', t) for t in TEXT.values()}) == RULES

    # the plain loop: the three passes over the 3 x 4 case, against the values worked out by hand (all exact in binary)
    at = {int(ln.split()[1]): i for i, ln in enumerate(lines) if ln.startswith('plain ')}
    assert set(at) == set(PLAIN)
    for p, want in PLAIN.items():
        vals = {ln.split(' :')[0]: [float(x) for x in ln.split(' :')[1].split()] for ln in lines[at[p] + 1:at[p] + 4]}
        assert vals == {'sq': want['sq'], 'abs': want['abs'], 'pred': want['pred']}, (p, vals)


def test_the_numpy_restatement_on_the_hand_computed_case():
    assert np.array_equal(W34 @ T34, [[2, 2, 2, 8.5], [0.5, 0, 1, 0.25], [3.5, 1, 6, 5.5]])
    for p, want in PLAIN.items():
        ref = fc.reference(W34, T34, want['rows'], A34, *want['clip'])
        assert np.array_equal(ref['sq'], want['sq']) and np.array_equal(ref['abs'], want['abs']) and np.array_equal(ref['pred'], want['pred'])
        assert ref['totals'] == (sum(want['sq']), sum(want['abs']), 5.0)
        # the bounds are what the docstring says, and small: a few hundred ulps of the sums
        assert np.all(ref['sq_bound'] <= 1e-12) and np.all(ref['abs_bound'] <= 1e-12) and np.all(ref['pred_bound'] <= 1e-13)
        assert ref['sq_bound'][1] == 0 and ref['abs_bound'][1] == 0          # a request without entries: exactly 0
        fc.check({'sq': np.array(want['sq']), 'abs': np.array(want['abs']), 'pred': np.array(want['pred'])}, ref)
        with pytest.raises(AssertionError):
            fc.check({'sq': np.array(want['sq']) + [1e-9, 0, 0], 'abs': np.array(want['abs']), 'pred': None}, ref)
    # the piece counts of the edge corpora take every value mod 4
    assert [fc.pieces_of(v) for v in fc.edge_variants()] == [11, 10, 9, 8]


PROTOS = {
    'rri_upload_observed_corpus': 'rri_ctx* ctx, const rri_corpus* corpus',
    'rri_corpus_entries_error': 'rri_ctx* ctx, const rri_corpus* corpus, const int64_t* rows, double clip_lo, double clip_hi, '
                                'double* sq_out, double* abs_out, double* pred_out, double totals[3], double* kernel_ms',
    'rri_corpus_value_range': 'rri_ctx* ctx, const rri_corpus* corpus, double out[2]',
}
CTYPES = {'rri_ctx*': ctypes.c_void_p, 'const rri_corpus*': ctypes.c_void_p, 'const int64_t*': ctypes.POINTER(ctypes.c_int64),
          'double': ctypes.c_double, 'double*': ctypes.POINTER(ctypes.c_double)}


def test_the_new_header_is_plain_c_bound_exported_documented_and_refuses_without_a_handle():
    text = open(os.path.join(ROOT, 'include', 'rri_corpus_fit.h')).read()
    assert '#include "rri_hip.h"' in text and _capi.ABI_VERSION == 1
    assert re.search(r'#define RRI_ABI_VERSION 1\b', open(os.path.join(ROOT, 'include', 'rri_hip.h')).read())      # additions, not a new ABI
    declared = re.findall(r'^rri_status (rri_\w+)\(', text, flags=re.M)
    assert sorted(declared) == sorted(PROTOS) == sorted(_capi.CORPUS_FIT_PROTOTYPES)
    assert not set(_capi.CORPUS_FIT_PROTOTYPES) & (set(_capi.PROTOTYPES) | set(_capi.CORPUS_OPS_PROTOTYPES) | set(_capi.CORPUS_BUILD_PROTOTYPES))
    for name, want in PROTOS.items():
        proto = re.search(r'^rri_status %s\(([^;]*)\);' % name, text, flags=re.M)
        assert proto and re.sub(r'\s+', ' ', proto.group(1)) == want, name
        res, args = _capi.CORPUS_FIT_PROTOTYPES[name]
        kinds = [re.sub(r' ?\w+\[\d+\]$', '*', a) if '[' in a else a.rsplit(' ', 1)[0] for a in want.split(', ')]
        assert res is ctypes.c_int32 and args == [CTYPES[kd] for kd in kinds], name
    # the header compiles as C99, alone
    cc_ = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    assert cc_, 'no host C compiler'
    subprocess.run([cc_, '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c', '-I' + os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'include', 'rri_corpus_fit.h')], check=True)
    # every declared symbol is exported and typed by load_library
    lib = _capi.load_library()
    for name, (res, args) in _capi.CORPUS_FIT_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args, name
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        body = open(os.path.join(ROOT, doc)).read()
        assert all(name in body for name in PROTOS) and 'rri_corpus_fit.h' in body, doc
    assert 'corpus_rs_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()
    build = open(os.path.join(ROOT, 'rri_nmf_amd', 'build.py')).read()
    assert 'rri_corpus_fit.h' in build
    hip = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_hip.hip')).read()
    assert '#include "rri_corpus_fit.h"' in hip and '#include "rri_fiterr_kernels.hpp"' in hip
    # NULL arguments: RRI_ERR_INVALID without a device, and nothing is written or counted
    out = (ctypes.c_double * 3)(7.0, 8.0, 9.0)
    ms = ctypes.c_double(5.0)
    assert lib.rri_upload_observed_corpus(None, None) == BAD
    assert lib.rri_corpus_entries_error(None, None, None, 1.0, 5.0, None, None, None, out, ctypes.byref(ms)) == BAD
    assert lib.rri_corpus_value_range(None, None, out) == BAD
    assert list(out) == [7.0, 8.0, 9.0] and ms.value == 5.0
    for counter in (lib.rri_corpus_memory, lib.rri_device_memory):
        a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert counter(ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (0, 0)


# ---- routing, with stand-ins ---------------------------------------------------------------------------------------------------
class FakeCorpus(object):
    """stands in for DeviceCorpus: a shape, a device, a count, and a to_scipy that must never be called"""
    made = []

    def __init__(self, A, device=0):
        self.A, self.shape, self.device, self.closed = sp.csr_matrix(A), A.shape, device, False
        self.nnz, self.negatives = self.A.nnz, 0
        FakeCorpus.made.append(self)

    def to_scipy(self):
        raise AssertionError('a fit from a corpus downloads nothing')

    def _ptr(self):
        if self.closed:
            raise ValueError('the corpus is closed')
        return self

    def value_range(self):
        return float(self.A.data.min()), float(self.A.data.max())

    def split_entries(self, held_out=0.05, random_state=0):
        self.split_args = (held_out, random_state)
        held = sp.csr_matrix(self.A.shape)
        held = held.tolil()
        i, j = self.A.nonzero()
        held[i[0], j[0]] = self.A[i[0], j[0]]
        held = held.tocsr()
        return FakeCorpus(self.A - held), FakeCorpus(held)

    def close(self):
        self.closed = True


class FakeEngine(object):
    """stands in for RRIEngine behind nmf(): keeps what it was made with and what it was given"""
    log = []

    def __init__(self, n, d, k, **kw):
        self.n, self.d, self.k, self.kw, self.closed, self.calls = n, d, k, kw, False, []
        self.n_resets_used, self.sparse, self.group, self.dtype, self.device = 0, True, None, kw.get('dtype'), kw.get('device', 0)
        self.obj = 100.0
        FakeEngine.log.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def upload_X_corpus(self, corpus):
        self.calls.append(('corpus', corpus))

    def upload_X_csr(self, A):
        self.calls.append(('csr', A))

    def upload_observed_csr(self, A):
        self.calls.append(('observed_csr', A))

    def upload_X(self, X):
        self.calls.append(('dense', X))

    def upload_mask(self, M):
        self.calls.append(('mask', M))

    def X_times(self, B):
        self.calls.append(('X_times',))
        return np.ones((self.n, np.shape(B)[1]))

    def set_W(self, W):
        self.W = np.array(W, dtype=np.float64)

    def set_T(self, T):
        self.T = np.array(T, dtype=np.float64)

    def set_params(self, **kw):
        self.params = kw

    def snapshot(self):
        self.calls.append(('snapshot',))

    def rollback(self):
        self.calls.append(('rollback',))

    def masked_rmse(self, *entries):
        self.calls.append(('masked_rmse',))
        return 1.0

    def sweep(self, n=1):
        self.calls.append(('sweep', n))
        return n

    def sweep_until(self, *a):
        return None

    def objective(self):
        self.obj *= 0.5
        return self.obj

    def project_W_rows(self, s):
        pass

    def get_W(self):
        return self.W

    def get_T(self):
        return self.T

    def close(self):
        self.closed = True


@pytest.fixture
def fakes(monkeypatch):
    from rri_nmf_amd import nmf as nm, sklearn_interface as si
    monkeypatch.setattr(nm, 'RRIEngine', FakeEngine)
    monkeypatch.setattr(nm, 'DeviceCorpus', FakeCorpus)
    monkeypatch.setattr(si, 'DeviceCorpus', FakeCorpus)
    FakeEngine.log, FakeCorpus.made = [], []
    scores = []

    def upload(engine, corpus):
        engine.calls.append(('observed_corpus', corpus))

    def error(engine, corpus, rows=None, clip=(None, None), predictions=False):
        engine.calls.append(('entries_error', corpus, tuple(clip)))
        return {'rmse': scores.pop(0)}
    monkeypatch.setattr(nm, 'upload_observed_corpus', upload)
    monkeypatch.setattr(nm, 'entries_error', error)

    def initialize(X, k, init, engine=None, **kw):
        # whatever start is asked for sees the X that exists only on the device, never a host matrix
        assert isinstance(X, nm._ResidentX) and X._engine is FakeEngine.log[-1] and init in nm._KNOWN_INITS
        FakeEngine.log[-1].calls.append(('init', init, engine is not None))
        return np.ones((X.shape[0], k)), np.ones((k, X.shape[1]))
    monkeypatch.setattr(nm, 'initialize_nmf', initialize)
    return nm, si, scores


X0 = np.array([[2.0, 0.0, 1.0, 1.0], [0.0, 4.0, 0.0, 0.0], [0.0, 0.0, 3.0, 0.0]])
W0 = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]])
T0 = np.array([[0.5, 0.25, 0.25, 0.0], [0.0, 0.25, 0.25, 0.5]])


def stop_on(held, lo=1.0, hi=5.0):
    def stop(X, W, T):
        raise AssertionError('scored on the device')
    stop.device_corpus = (held, lo, hi)
    return stop


def test_every_refusal_of_observed_only_comes_before_any_device_call(fakes):
    nm, _, _ = fakes
    corpus = FakeCorpus(X0)
    go = dict(W_in=W0, T_in=T0, max_iter=2, observed_only=True)
    stop = lambda X, W, T: 0.0
    for X in (X0, sp.csr_matrix(X0)):
        with pytest.raises(ValueError, match='observed_only=True takes a DeviceCorpus X'):
            nm.nmf(X, 2, **go)
    refused = [(dict(W_mat=np.ones((3, 4))), 'W_mat'), (dict(preprocess=('normalize',)), 'preprocess'), (dict(uniform_rows=True), 'uniform_rows=True'),
               (dict(frozen=True), 'frozen='), (dict(resident=nm.ResidentProblem()), 'resident='), (dict(w_row=np.ones((3, 1))), 'w_row'),
               (dict(group=object()), 'group='), (dict(schedule='residual'), "schedule='residual'"), (dict(dtype=np.float16), 'dtype=float16'),
               (dict(dtype=np.uint8), 'dtype=uint8'), (dict(diagnostics=[stop]), 'diagnostics'),
               (dict(store_gradients=True), 'store_gradients'), (dict(early_stop=stop), 'an early_stop function without device_entries'),
               (dict(eps_gauss_t=1.0, delta_gauss_t=0.1), 'the Gaussian mechanism')]
    for kw, text in refused:
        with pytest.raises(ValueError, match='observed_only=True keeps .* does not combine with ' + re.escape(text)):
            nm.nmf(corpus, 2, **dict(go, **kw))
    with pytest.raises(NotImplementedError, match="init='coherence_beam_search'"):
        nm.nmf(corpus, 2, init='coherence_beam_search', max_iter=2, observed_only=True)
    with pytest.raises(ValueError, match='lives on device 0, the call asks for device 1'):
        nm.nmf(corpus, 2, device=1, **go)
    shut = FakeCorpus(X0)
    shut.closed = True
    with pytest.raises(ValueError, match='the corpus is closed'):
        nm.nmf(shut, 2, **go)
    # the refusals of a corpus call without the option keep their texts: W_mat still does not combine with a DeviceCorpus X
    with pytest.raises(ValueError, match='a DeviceCorpus X is kept as CSR on one device .* does not combine with W_mat'):
        nm.nmf(corpus, 2, W_mat=np.ones((3, 4)), W_in=W0, T_in=T0)
    with pytest.raises(ValueError, match='does not combine with an early_stop function without device_entries'):
        nm.nmf(corpus, 2, early_stop=stop, W_in=W0, T_in=T0)
    assert FakeEngine.log == []


def test_every_refusal_of_a_held_out_corpus_comes_before_any_device_call(fakes):
    nm, _, _ = fakes
    corpus, held = FakeCorpus(X0), FakeCorpus(X0)
    go = dict(W_in=W0, T_in=T0, max_iter=2, compute_obj_each_iter=True)
    wide, far, shut, empty = FakeCorpus(np.ones((3, 5))), FakeCorpus(X0, device=1), FakeCorpus(X0), FakeCorpus(np.zeros((3, 4)))
    shut.closed = True
    for X, more in ((corpus, dict(observed_only=True)), (corpus, {}), (X0, {}), (sp.csr_matrix(X0), dict(sparse_X=True))):
        kw = dict(go, **more)
        with pytest.raises(ValueError, match='the held-out corpus is 3 x 5, the problem 3 x 4'):
            nm.nmf(X, 2, early_stop=stop_on(wide), **kw)
        with pytest.raises(ValueError, match='the held-out corpus lives on device 1, the call asks for device 0'):
            nm.nmf(X, 2, early_stop=stop_on(far), **kw)
        with pytest.raises(ValueError, match='the corpus is closed'):
            nm.nmf(X, 2, early_stop=stop_on(shut), **kw)
        with pytest.raises(ValueError, match='the held-out corpus is empty'):
            nm.nmf(X, 2, early_stop=stop_on(empty), **kw)
        with pytest.raises(ValueError, match='must be \\(held_corpus, lo, hi\\)'):
            nm.nmf(X, 2, early_stop=stop_on(X0), **kw)
    with pytest.raises(NotImplementedError, match='not collective'):
        nm.nmf(X0, 2, early_stop=stop_on(held), group=object(), **go)
    assert FakeEngine.log == []


def test_observed_only_reaches_upload_observed_corpus_on_a_pattern_only_engine_and_nothing_else(fakes):
    nm, _, _ = fakes
    corpus = FakeCorpus(X0)
    out = nm.nmf(corpus, 2, W_in=W0, T_in=T0, max_iter=2, device=0, observed_only=True, compute_obj_each_iter=True)
    (eng,) = FakeEngine.log
    assert eng.kw['weighted'] == 'sparse' and 'sparse_x' not in eng.kw and eng.kw['dtype'] == np.float64 and eng.closed
    uploads = ('observed_corpus', 'corpus', 'csr', 'observed_csr', 'dense', 'mask')
    assert [c for c in eng.calls if c[0] in uploads] == [('observed_corpus', corpus)]
    assert np.array_equal(out['W'], W0) and np.array_equal(out['T'], T0)
    # the objective is re-evaluated on the corpus, on a handle of the same kind
    FakeEngine.log = []
    out['obj_calculator'].true_objective()
    (eng,) = FakeEngine.log
    assert eng.kw['weighted'] == 'sparse' and [c for c in eng.calls if c[0] in uploads] == [('observed_corpus', corpus)] and eng.closed
    # the default start goes through the handle's products; float32 storage is passed on
    FakeEngine.log = []
    nm.nmf(corpus, 2, max_iter=1, observed_only=True, dtype=np.float32)
    (eng,) = FakeEngine.log
    assert ('init', 'nndsvd', True) in eng.calls and eng.kw['dtype'] == np.float32
    assert [c for c in eng.calls if c[0] in uploads] == [('observed_corpus', corpus)]
    # without the option the corpus goes where it went: the unweighted CSR handle
    FakeEngine.log = []
    nm.nmf(corpus, 2, W_in=W0, T_in=T0, max_iter=1)
    assert FakeEngine.log[0].kw.get('sparse_x') is True and ('corpus', corpus) in FakeEngine.log[0].calls


def test_an_early_stop_on_a_held_out_corpus_is_scored_between_sweeps(fakes):
    nm, _, scores = fakes
    corpus, held = FakeCorpus(X0), FakeCorpus(X0)
    scores[:] = [3.0, 2.0, 1.5, 1.75, 9.0]
    out = nm.nmf(corpus, 2, W_in=W0, T_in=T0, max_iter=10, observed_only=True, compute_obj_each_iter=True, eps_stop=0.0,
                 early_stop=stop_on(held, 1.0, 5.0))
    (eng,) = FakeEngine.log
    names = [c[0] for c in eng.calls if c[0] in ('snapshot', 'rollback', 'entries_error', 'sweep', 'masked_rmse')]
    # a snapshot first; then score, snapshot, sweep while the score falls; the fourth score rises: rollback, and the sweep is dropped
    assert names == ['snapshot'] + ['entries_error', 'snapshot', 'sweep'] * 3 + ['entries_error', 'rollback']
    assert all(c[1] is held and c[2] == (1.0, 5.0) for c in eng.calls if c[0] == 'entries_error')
    assert len(out['obj_history']) == 2 and scores == [9.0]
    # the same callable on a host matrix: allowed wherever device_entries is
    FakeEngine.log, scores[:] = [], [1.0, 2.0]
    nm.nmf(sp.csr_matrix(X0), 2, W_in=W0, T_in=T0, max_iter=5, sparse_X=True, early_stop=stop_on(held), compute_obj_each_iter=True)
    assert [c[0] for c in FakeEngine.log[0].calls if c[0] in ('entries_error', 'masked_rmse', 'rollback')] == ['entries_error', 'entries_error', 'rollback']


# ---- the estimator, behind a stand-in solver -----------------------------------------------------------------------------------
@pytest.fixture
def solver(fakes, monkeypatch):
    nm, si, _ = fakes
    calls = []

    def nmf(X, k, **kw):
        calls.append((X, k, kw))
        return {'W': W0.copy(), 'T': T0.copy(), 'obj_history': [1.0]}
    monkeypatch.setattr(nm, 'nmf', nmf)
    from rri_nmf_amd import corpus_fit
    downloads = []

    def pattern_of(corpus):
        downloads.append(corpus)
        P = corpus.A.copy()
        P.data[:] = 1.0
        return P
    monkeypatch.setattr(corpus_fit, 'pattern_of', pattern_of)
    return si, calls, downloads


def test_fit_corpus_behind_a_stand_in_solver(solver):
    si, calls, downloads = solver
    train = FakeCorpus(X0)
    # early stopping on, no held-out corpus: the split is made, used and closed here; the range is the whole corpus's
    E = si.NMF_RS_Estimator(3, 4, 2, max_iter=7, wr1=0.25, nmf_kwargs={'device': 0})
    assert E.fit_corpus(train) is E
    (X, k, kw), = calls
    sub, own = FakeCorpus.made[-2:]
    assert train.split_args == (0.05, 0) and X is sub and k == 2 and sub.closed and own.closed and not train.closed
    assert kw['observed_only'] is True and 'W_mat' not in kw and kw['max_iter'] == 7 and kw['reg_w_l1'] == 0.25 and kw['device'] == 0
    assert kw['t_row_sum'] == 1.0 and kw['reset_topic_method'] is None and kw['compute_obj_each_iter'] is True
    assert kw['early_stop'].device_corpus == (own, 1.0, 4.0) and (E.min_rating, E.max_rating) == (1.0, 4.0)
    assert downloads == [train] and np.array_equal(E.seen_.toarray(), (X0 != 0).astype(float))
    assert np.array_equal(E.W, W0) and np.array_equal(E.T, T0)
    # a held-out corpus of the caller's: no split, nothing closed, the range and seen_ are the union's
    del calls[:], downloads[:]
    H = np.zeros((3, 4))
    H[1, 0], H[2, 3] = 5.0, 0.5
    held = FakeCorpus(H)
    E = si.NMF_RS_Estimator(3, 4, 2)
    E.fit_corpus(train, held)
    (X, k, kw), = calls
    assert X is train and kw['early_stop'].device_corpus == (held, 0.5, 5.0) and not train.closed and not held.closed
    assert downloads == [train, held] and np.array_equal(E.seen_.toarray(), ((X0 != 0) | (H != 0)).astype(float))
    assert E.seen_.has_canonical_format
    # early stopping off: no split, no callable; keep_seen=False leaves seen_ None and recommend(exclude_seen=True) raises
    del calls[:], downloads[:]
    E = si.NMF_RS_Estimator(3, 4, 2, use_validation_early_stopping=False)
    E.fit_corpus(train, keep_seen=False)
    (X, k, kw), = calls
    assert X is train and kw['early_stop'] is False and E.seen_ is None and downloads == []
    with pytest.raises(ValueError, match='exclude_seen=True needs the pairs given to fit'):
        E.recommend([0], 2)
    # what is not a corpus, or not the estimator's shape, is refused
    with pytest.raises(TypeError, match='fit_corpus takes DeviceCorpus objects'):
        E.fit_corpus(sp.csr_matrix(X0))
    with pytest.raises(ValueError, match='the corpora must be 3 x 4'):
        E.fit_corpus(FakeCorpus(np.ones((3, 5))))
    with pytest.raises(ValueError, match='there are no ratings to fit'):
        E.fit_corpus(FakeCorpus(np.zeros((3, 4))))
    # the two pinned routes stay downloads
    for name in ('fit_from_Xtr', 'score'):
        assert 'the weighted fit from a resident corpus is not built' in getattr(si.NMF_RS_Estimator, name).__doc__


def test_score_corpus_behind_a_stand_in_engine(solver, monkeypatch):
    si, _, _ = solver
    from rri_nmf_amd import corpus_fit
    seen = []

    def error(engine, corpus, rows=None, clip=(None, None), predictions=False):
        seen.append((engine, corpus, clip))
        return {'rmse': 0.625}
    monkeypatch.setattr(corpus_fit, 'entries_error', error)
    monkeypatch.setattr(si, 'RRIEngine', FakeEngine)
    E = si.NMF_RS_Estimator(3, 4, 2, W=W0, T=T0)
    E.min_rating, E.max_rating = 1.0, 4.0
    test = FakeCorpus(X0)
    FakeEngine.log = []
    assert E.score_corpus(test) == 0.625
    (eng,) = FakeEngine.log
    assert (eng.n, eng.d, eng.k) == (3, 4, 2) and eng.kw['weighted'] is False and eng.kw['dtype'] == np.float64 and eng.closed
    assert np.array_equal(eng.W, W0) and np.array_equal(eng.T, T0) and eng.calls == []       # factors only: nothing uploaded
    assert seen == [(eng, test, (1.0, 4.0))]
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_RS_Estimator(3, 4, 2).score_corpus(test)
