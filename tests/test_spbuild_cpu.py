"""The fit from a DeviceCorpus, without a GPU: the device builder's algorithm as the plain loop of
rri_nmf_amd/csrc/rri_spbuild.hpp under sanitizers, the work-item cutter both routes share, the ABI surface, the texts of the
argument check, and the routing of nmf() and NMF_TM_Estimator with stand-ins for the engine and the corpus.

tests/c/spbuild_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built once with the
host compiler under AddressSanitizer and UndefinedBehaviorSanitizer.  For every matrix it is fed it builds the blocked copy by
build_sp_copy (the specification) and by count / padded scan / claim / sort with the claims arriving in two shuffled orders and in
ascending order, and says whether all arrays are equal element for element; what it prints of the layout is held against the
numpy restatement of tests/wsb_cases.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import spbuild_cases as sc
import wsb_cases as wc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('spbuild') / 'spbuild')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'spbuild_main.cpp'), '-o', exe], check=True)
    return exe


def run(exe, requests):
    """requests: (A, which, csrx, store); returns the check lines and one record per request"""
    text = []
    for i, (A, which, csrx, store) in enumerate(requests):
        n, d = A.shape
        text.append('copy %d %d %d %d %d %d %d %d %d' % (which, int(csrx), np.dtype(wc.STORES[store]).itemsize, wc.N_CU, n, d, A.nnz,
                                                        1000 + i, 5000 + i))
        text.append(' '.join(str(int(v)) for v in A.indptr))
        text.append(' '.join(str(int(v)) for v in A.indices))
    res = subprocess.run([exe], input='\n'.join(text) + '\n', stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok %d cases' % len(requests), lines[-1]
    recs = [dict() for _ in requests]
    for ln in lines:
        kind, _, rest = ln.partition(' ')
        if kind == 'copy':
            idx, _, fields = rest.partition(' ')
            recs[int(idx)].update((k, v) for k, v in (f.split('=') for f in fields.split()))
        elif kind in ('work', 'seglen'):
            idx, _, body = rest.partition(' :')
            recs[int(idx)][kind] = np.array(body.split(), dtype=np.int64)
    return lines, recs


def hold_against_restatement(rec, A, which, csrx, store, name):
    L = wc.sp_copy_layout(A, which, store, csrx)
    assert rec['equal'] == '1' and rec['differs'] == '-', (name, which, rec['differs'])       # claim-then-sort = the stable counting sort
    assert rec['shuffled'] == '1', name
    for key in ('nblk', 'bw', 'lps', 'nwork', 'gdim'):
        assert int(rec[key]) == L[key], (name, which, key)
    assert np.array_equal(rec['seglen'], L['seg_len'].ravel()), (name, which)
    assert np.array_equal(rec['work'].reshape(-1, 4), np.array([w + (which,) for w in L['work']], dtype=np.int64).reshape(-1, 4)), (name, which)
    padded = (L['seg_len'] + 3) // 4 * 4
    assert int(rec['count']) == padded.sum() and int(rec['slots']) == max(int(padded.sum()), 4), (name, which)
    assert int(rec['pads']) == int(rec['slots']) - A.nnz and int(rec['longest_row']) == (np.diff(A.indptr).max() if A.shape[0] else 0)
    return L


def test_claim_then_sort_reproduces_the_stable_order(program):
    mats = [(name, make()) for name, make in sc.cases()]
    requests = [(A, which, True, 'fp64') for _, A in mats for which in (0, 1)]
    _, recs = run(program, requests)
    lay = {}
    for i, (A, which, csrx, store) in enumerate(requests):
        name = mats[i // 2][0]
        lay[name, which] = hold_against_restatement(recs[i], A, which, csrx, store, name)
    # the cases still make their point
    assert lay['57x33', 0]['nblk'] == 1 and lay['57x33', 1]['nblk'] == 1
    assert lay['200x15297', 0]['nblk'] == 2 and lay['200x15297', 1]['nblk'] == 1
    L = lay['15400x40', 1]
    assert L['nblk'] == 2 and ((L['seg_len'] + 3) // 4 * 4).sum(axis=1).min() > 8192
    assert max(sum(1 for w in L['work'] if w[0] == b) for b in range(2)) > 1              # a block cut into several work items
    assert lay['15296x3-full-column', 1]['nblk'] == 1 and lay['15296x3-full-column', 1]['seg_len'].max() == sc.CAP == lay['15296x3-full-column', 1]['bw']
    L = lay['15297x3-full-column', 1]
    assert L['nblk'] == 2 and L['seg_len'][:, 1].tolist() == [L['bw'], sc.CAP + 1 - L['bw']]
    assert [lay[name, 0]['lps'] for name, _ in mats if name.startswith('lps-')] == [8, 16, 16, 32, 32, 64]
    L = lay['holes', 0]
    assert L['nblk'] == 2 and L['seg_len'][1].sum() == 0 and (L['seg_len'][0] == 0).sum() >= 3 and (lay['holes', 1]['seg_len'] == 0).any()
    assert lay['nnz=0', 0]['seg_len'].sum() == 0 and lay['nnz=0', 0]['nwork'] == 1


def test_the_cutter_both_routes_call_cuts_what_it_cut_before(program):
    """the work items of every blocked case of tests/wsb_cases.py, through build_sp_copy and through the plain loop, which both
    call sp_cut_work: the items of the restatement, which has not changed"""
    requests, names = [], []
    for name, make, _, flavour, store in wc.blocked_runs():
        A = make()
        for which in (0, 1):
            requests.append((A, which, flavour == 'csrx', store))
            names.append(wc.run_id((name, make, _, flavour, store)))
    _, recs = run(program, requests)
    several = 0
    for rec, (A, which, csrx, store), name in zip(recs, requests, names):
        L = hold_against_restatement(rec, A, which, csrx, store, name)
        several += L['nwork'] > L['nblk']
    assert several >= 2          # ... and some of them are cut into more items than blocks


def test_the_argument_check_says_what_is_wrong(program):
    lines, _ = run(program, [])
    got = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'check (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    OK, INVALID, UNSUPPORTED = 0, _capi.RRI_ERR_INVALID, _capi.RRI_ERR_UNSUPPORTED           # = TOPN_REQ_* of rri_topn.hpp
    assert (INVALID, UNSUPPORTED) == (-1, -3)
    assert got == {'fine': (OK, ''), 'most_entries': (OK, ''),
                   'dead': (INVALID, 'the corpus is NULL or has been destroyed'),
                   'dead_wins': (INVALID, 'the corpus is NULL or has been destroyed'),
                   'device': (INVALID, 'the corpus lives on device 2, the handle on device 1'),
                   'rows': (INVALID, 'the corpus is 4 x 7, the handle 5 x 7'),
                   'cols': (INVALID, 'the corpus is 5 x 8, the handle 5 x 7'),
                   'too_many_entries': (UNSUPPORTED, 'more than 2^31-1 stored entries')}
    # the key: the canonical position above the offset inside the block, both recovered; up to 64 entries a wave sorts
    assert 'key : %d 2147483646 15295' % ((2147483646 << 32) | 15295) in lines
    assert 'wave : 1 1 0' in lines


PROTOS = {
    'rri_upload_X_corpus': 'rri_ctx* ctx, const rri_corpus* corpus',
    'rri_sparse_store_get': 'rri_ctx* ctx, int32_t which, int64_t* info, int32_t n_info, int64_t* segptr, uint16_t* idx, int32_t* perm, '
                            'void* val, int32_t* work',
}
CTYPES = {'rri_ctx*': ctypes.c_void_p, 'const rri_corpus*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int32_t': ctypes.c_int32,
          'int64_t*': ctypes.POINTER(ctypes.c_int64), 'int32_t*': ctypes.POINTER(ctypes.c_int32), 'uint16_t*': ctypes.POINTER(ctypes.c_uint16)}


def test_the_entry_points_are_declared_bound_and_documented():
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    assert re.search(r'#define RRI_ABI_VERSION 1\b', text) and _capi.ABI_VERSION == 1          # additions, not a new ABI
    assert re.search(r'#define RRI_SPARSE_STORE_INFO_FIELDS 10\b', text) and _capi.RRI_SPARSE_STORE_INFO_FIELDS == 10
    for name, want in PROTOS.items():
        proto = re.search(r'^rri_status %s\(([^;]*)\);' % name, text, flags=re.M)
        assert proto and re.sub(r'\s+', ' ', proto.group(1)) == want, name
        res, args = _capi.PROTOTYPES[name]
        assert res is ctypes.c_int32 and args == [CTYPES[a.rsplit(' ', 1)[0]] for a in want.split(', ')], name
    lib = _capi.load_library()
    assert lib.rri_abi_version() == 1
    # without a handle nothing is read
    assert lib.rri_upload_X_corpus(None, None) == _capi.RRI_ERR_INVALID
    assert lib.rri_sparse_store_get(None, 0, None, 0, None, None, None, None, None) == _capi.RRI_ERR_INVALID
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        body = open(os.path.join(ROOT, doc)).read()
        assert 'rri_upload_X_corpus' in body, doc
    assert 'rri_sparse_store_get' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'corpus_fit_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()


# ---- routing, with stand-ins ---------------------------------------------------------------------------------------------------
class FakeCorpus(object):
    """stands in for DeviceCorpus: a shape, a device, the count of negatives, and a to_scipy that must never be called"""

    def __init__(self, A, device=0, negatives=0):
        self.A, self.shape, self.device, self.negatives, self.closed = sp.csr_matrix(A), A.shape, device, negatives, False

    def to_scipy(self):
        raise AssertionError('a fit from a corpus downloads nothing')

    def _ptr(self):
        if self.closed:
            raise ValueError('the corpus is closed')
        return self


class FakeEngine(object):
    """stands in for RRIEngine behind nmf(): keeps what it was made with and what it was given"""
    log = []
    zero_rows = 0

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

    def upload_X(self, X):
        self.calls.append(('dense', X))

    def preprocess(self, tfidf=False, normalize=False, uniform_rows=False):
        from rri_nmf_amd.engine import ZeroTotalRows
        self.calls.append(('preprocess', tfidf is not False, normalize, uniform_rows))
        if FakeEngine.zero_rows and not uniform_rows:
            raise ZeroTotalRows(FakeEngine.zero_rows)
        return np.ones(self.d) if tfidf is True else None

    def X_times(self, B):
        self.calls.append(('X_times',))
        return np.ones((self.n, np.shape(B)[1]))

    def begin_run(self):
        self.calls.append(('begin_run',))

    def set_W(self, W):
        self.W = np.array(W, dtype=np.float64)

    def set_T(self, T):
        self.T = np.array(T, dtype=np.float64)

    def set_params(self, **kw):
        self.params = kw

    def set_frozen(self, f):
        self.calls.append(('frozen', f))

    def absorb(self, decay=1.0):
        self.calls.append(('absorb', decay))

    def get_frozen(self):
        return None

    def clear_frozen(self):
        pass

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
    FakeEngine.log, FakeEngine.zero_rows = [], 0

    def initialize(X, k, init, engine=None, **kw):
        # whatever start is asked for sees the X that exists only on the device, never a host matrix
        assert isinstance(X, nm._ResidentX) and X._engine is FakeEngine.log[-1] and init in nm._KNOWN_INITS
        FakeEngine.log[-1].calls.append(('init', init, engine is not None))
        return np.ones((X.shape[0], k)), np.ones((k, X.shape[1]))
    monkeypatch.setattr(nm, 'initialize_nmf', initialize)
    return nm, si


X0 = np.array([[2.0, 0.0, 1.0, 1.0], [0.0, 4.0, 0.0, 0.0], [0.0, 0.0, 3.0, 0.0]])
W0 = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]])
T0 = np.array([[0.5, 0.25, 0.25, 0.0], [0.0, 0.25, 0.25, 0.5]])


def test_every_refusal_comes_before_any_device_call(fakes):
    nm, _ = fakes
    corpus = FakeCorpus(X0)
    go = dict(W_in=W0, T_in=T0, max_iter=2)
    stop = lambda X, W, T: 0.0
    refused = [(dict(W_mat=np.ones((3, 4))), 'W_mat'), (dict(w_row=np.ones((3, 1))), 'w_row'), (dict(group=object()), 'group='),
               (dict(schedule='residual'), "schedule='residual'"), (dict(dtype=np.float16), 'dtype=float16'),
               (dict(dtype=np.uint8), 'dtype=uint8'), (dict(diagnostics=[stop]), 'diagnostics'),
               (dict(store_gradients=True), 'store_gradients'), (dict(early_stop=stop), 'an early_stop function without device_entries'),
               (dict(eps_gauss_t=1.0, delta_gauss_t=0.1), 'the Gaussian mechanism')]
    for kw, text in refused:
        with pytest.raises(ValueError, match='does not combine with ' + re.escape(text)):
            nm.nmf(corpus, 2, **dict(go, **kw))
    with pytest.raises(ValueError, match='sparse_X=False would densify it'):
        nm.nmf(corpus, 2, sparse_X=False, **go)
    with pytest.raises(NotImplementedError, match="init='coherence_beam_search'"):
        nm.nmf(corpus, 2, init='coherence_beam_search', max_iter=2)
    with pytest.raises(ValueError, match='lives on device 0, the call asks for device 1'):
        nm.nmf(corpus, 2, device=1, **go)
    with pytest.raises(ValueError, match='frozen statistics are for k = 2, d = 5'):
        nm.nmf(corpus, 2, frozen=nm.FrozenRows.zeros(2, 5), **go)
    shut = FakeCorpus(X0)
    shut.closed = True
    with pytest.raises(ValueError, match='the corpus is closed'):
        nm.nmf(shut, 2, **go)
    assert FakeEngine.log == []


def test_a_corpus_reaches_upload_X_corpus_and_nothing_else(fakes):
    nm, _ = fakes
    corpus = FakeCorpus(X0)
    out = nm.nmf(corpus, 2, W_in=W0, T_in=T0, max_iter=2, device=0)
    (eng,) = FakeEngine.log
    assert eng.kw['sparse_x'] is True and eng.kw['dtype'] == np.float64 and eng.closed
    assert [c for c in eng.calls if c[0] in ('corpus', 'csr', 'dense')] == [('corpus', corpus)]
    assert np.array_equal(out['W'], W0) and np.array_equal(out['T'], T0)
    # preprocess= runs on the device, with uniform_rows where asked; the default init goes through the device products
    FakeEngine.log = []
    nm.nmf(corpus, 2, max_iter=1, preprocess=('tfidf', 'normalize'), uniform_rows=True, init='smart_random', random_state=1)
    (eng,) = FakeEngine.log
    assert ('preprocess', True, True, True) in eng.calls and ('init', 'smart_random', False) in eng.calls and ('corpus', corpus) in eng.calls
    FakeEngine.log = []
    nm.nmf(corpus, 2, max_iter=1)                       # no preprocessing: the default start still runs on the device products
    assert ('init', 'nndsvd', True) in FakeEngine.log[0].calls
    assert not any(c[0] in ('csr', 'dense') for c in eng.calls)
    # a row that normalisation would make dense: no host fallback, the handle is closed
    FakeEngine.log, FakeEngine.zero_rows = [], 2
    with pytest.raises(ValueError, match='uniform_rows=True'):
        nm.nmf(corpus, 2, W_in=W0, T_in=T0, max_iter=1, preprocess=('normalize',))
    assert len(FakeEngine.log) == 1 and FakeEngine.log[0].closed
    FakeEngine.zero_rows = 0
    # frozen= and fix_T pass through
    FakeEngine.log = []
    nm.nmf(corpus, 2, W_in=W0, T_in=T0, max_iter=1, frozen=nm.FrozenRows.zeros(2, 4))
    assert [c[0] for c in FakeEngine.log[0].calls if c[0] in ('corpus', 'frozen', 'absorb')] == ['corpus', 'frozen', 'absorb']
    FakeEngine.log = []
    nm.nmf(corpus, 2, T_in=T0, fix_T=True, max_iter=1, init='random', random_state=0)
    assert FakeEngine.log[0].params['fix_T'] is True and ('corpus', corpus) in FakeEngine.log[0].calls


def test_the_estimator_takes_a_corpus_and_keeps_its_handle_by_identity(fakes):
    nm, si = fakes
    c1, c2 = FakeCorpus(X0), FakeCorpus(X0)
    E = si.NMF_TM_Estimator(3, 4, 2, W=W0, T=T0, max_iter=2, keep_resident=True)
    E.fit(c1)
    E.one_iter(c1)
    assert len(FakeEngine.log) == 1 and not FakeEngine.log[0].closed and E._resident.reuses == 1
    assert [c for c in FakeEngine.log[0].calls if c[0] == 'corpus'] == [('corpus', c1)]        # uploaded once
    E.one_iter(c2)                                      # another object, equal or not: a new handle, the old one closed
    assert len(FakeEngine.log) == 2 and FakeEngine.log[0].closed and not FakeEngine.log[1].closed
    assert [c for c in FakeEngine.log[1].calls if c[0] == 'corpus'] == [('corpus', c2)]
    E.release()
    assert FakeEngine.log[1].closed
    # transform: a fold-in on a fresh handle, T fixed
    E.transform(c1)
    assert FakeEngine.log[-1].params['fix_T'] is True and ('corpus', c1) in FakeEngine.log[-1].calls and FakeEngine.log[-1].closed
    # the non-negativity assertion reads the corpus's own count; score() stays on the host
    with pytest.raises(AssertionError, match='non-negative'):
        E.fit(FakeCorpus(X0, negatives=1))
    with pytest.raises(AssertionError, match='non-negative'):
        E.partial_fit(FakeCorpus(X0, negatives=3))
    with pytest.raises(TypeError, match='DeviceCorpus'):
        E.score(c1)
