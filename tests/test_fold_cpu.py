"""The fold-in of rows against a fixed T, without a GPU: rri_fold.hpp under the host compiler and the sanitizers (the plain loop
against the numpy restatement of tests/fold_cases.py, every branch of the update, the eligibility rule over the cross product of
its inputs, the LDS formula against its bound), the header include/rri_fold.h (plain C, bound, exported, documented, refusing a
NULL handle without a device), the refusals of nmf(fold_in=True), and NMF_RS_Estimator.transform_corpus and the W= arguments
behind stand-ins for the solver and the handle."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import fold_cases as fo
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _capi.RRI_ERR_INVALID
EPS = 2.0 ** -49
# (shape, flag set, t0): the row constructions of the GPU tests, t0 > 0, every flag set
FILE_CASES = [((70, 40, 1, 0.3), 'plain', 0), ((130, 90, 16, 0.4), 'regs', 0), ((131, 90, 17, 0.4), 'wrs', 5), ((64, 300, 4, 0.08), 'plain', 3),
              ((40, 70, 64, 0.5), 'regs', 63), ((30, 20, 3, 0.5), 'neg', 1)]
FLAGSETS = dict(fo.FLAGSETS, neg=dict(w_row_sum=0.7, reg_w_l2=-1e9))


def _write_cases(path):
    made = []
    with open(path, 'w') as f:
        for shape, name, t0 in FILE_CASES:
            A, X, M, W0, T0 = fo.problem(*shape)
            fl = FLAGSETS[name]
            wrs = fl.get('w_row_sum')
            f.write('%d %d %d %d %s %s %d %s %s\n' % (shape[0], shape[1], shape[2], t0, float(fl.get('reg_w_l1', 0.0)).hex(),
                                                      float(fl.get('reg_w_l2', 0.0)).hex(), wrs is not None, float(wrs or 0.0).hex(),
                                                      float(fo.EPS_DIV).hex()))
            for arr in (A.indptr, A.indices):
                f.write(' '.join('%d' % x for x in arr) + '\n')
            for arr in (A.data, T0.ravel(), W0.ravel()):
                f.write(' '.join(float(x).hex() for x in arr) + '\n')
            made.append((A, T0, W0, t0, fl))
    return made


def test_the_plain_loop_the_update_the_rule_and_the_lds_formula_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe, cases = str(tmp_path / 'fold'), str(tmp_path / 'cases.txt')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'fold_main.cpp'), '-o', exe], check=True)
    made = _write_cases(cases)
    res = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok', lines[-1]

    # the LDS formula: what the kernel lays out, inside the bound for every rank the walk covers
    limit = int(next(ln for ln in lines if ln.startswith('limit ')).split()[1])
    assert limit == 150 * 1024
    lds = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith('lds ')]
    assert [r[0] for r in lds] == list(range(1, 65))
    for k, nbytes, kt, kpad, gld in lds:
        assert kt == (k + 15) // 16 and kpad == 16 * kt and gld == kpad + 1
        assert nbytes == (4 * kpad * gld + kpad * 17) * 8 + kpad * 16 and 0 < nbytes <= limit, k
    assert lds[-1][1] == 142848

    # the eligibility rule over the cross product of its inputs
    rules = [ln for ln in lines if ln.startswith('rule ')]
    assert len(rules) == 128 * 6
    for ln in rules:
        a, w, s, x, fT, fW, c, k, _, got = (int(v) if v != ':' else v for v in ln.split()[1:])
        assert got == int(bool(a and w and s and not x and fT and not fW and not c and 1 <= k <= 64)), ln

    # every branch of the update
    entry = {m.group(1): (float.fromhex(m.group(2)) if 'nan' not in m.group(2) else float('nan'), int(m.group(3)))
             for m in (re.match(r'entry (\w+) : (\S+) (-?\d+)$', ln) for ln in lines) if m}
    assert entry == {'closed_form': (2.5 / (2.5 + EPS), 0), 'numerator_below_zero': (0.0, 0), 'denominator_zero': (0.0, 0),
                     'denominator_negative': (0.0, 1), 'bounded_above': (0.7, 0), 'bound_not_reached': (1.0 / (2.0 + EPS), 0),
                     'negative_with_bound': (0.0, 1), 'nan_numerator': (0.0, 0)}

    # the argument check: the verdict, and a text of its own for every broken rule
    args = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'args (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    assert {name: code for name, (code, _) in args.items()} == {'fine': 0, 'null_handle': -1, 'other_flavour': -1, 'null_out': -1}
    assert args['fine'][1] == '' and args['null_handle'][1] == 'the handle is NULL' and args['null_out'][1] == 'out is NULL'
    assert 'pattern-only handle (RRI_WEIGHTED_SPARSE)' in args['other_flavour'][1]

    # the plain loop against the numpy restatement: the same formulas, sums in another order
    for c, (A, T0, W0, t0, fl) in enumerate(made):
        at = lines.index('case %d' % c)
        W, colsum, negs = (np.array([float.fromhex(x) for x in lines[at + j].split(' :')[1].split()]) for j in (1, 2, 3))
        want_W, want_sum, want_neg = fo.fold_sweep(A, T0, W0, t0=t0, **fl)
        W = W.reshape(W0.shape)
        assert np.array_equal(W[:, :t0], W0[:, :t0])                                    # topics below t0 are not touched
        assert fo.relfro(W, want_W) < 1e-12, (c, fo.relfro(W, want_W))
        assert np.allclose(colsum[t0:], want_sum[t0:], rtol=1e-12, atol=1e-300) and np.array_equal(negs[t0:], want_neg[t0:]), c
        assert np.all(colsum[:t0] == -1.0) and np.all(negs[:t0] == -1.0)
        assert np.allclose(colsum[t0:], W[:, t0:].sum(axis=0), rtol=1e-12)
        if 'reg_w_l2' in fl and fl['reg_w_l2'] < -1:       # every denominator negative: the column empties, every row counted
            assert np.all(W[:, t0:] == 0) and np.all(negs[t0:] == W0.shape[0])
        # and the restatement against the reference's own arithmetic where no column halts: one sweep of the oracle
        if t0 == 0:
            from oracle import rri_oracle as orc
            X = A.toarray()
            M = np.zeros(A.shape)
            M[np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), A.indices] = 1.0          # (explicit zeros are observed)
            ref = orc.nmf(X, W0.shape[1], W_in=W0.copy(), T_in=T0.copy(), W_mat=M, fix_T=True, max_iter=1, eps_stop=-1,
                          do_final_project_W=False, reset_topic_method=None, **fl)
            assert fo.relfro(W, ref['W']) < 1e-12, (c, fo.relfro(W, ref['W']))


PROTOS = {'rri_set_fold_schedule': 'rri_ctx* ctx, int on', 'rri_fold_info': 'const rri_ctx* ctx, int64_t out[6]'}


def test_the_new_header_is_plain_c_bound_exported_documented_and_refuses_without_a_handle():
    text = open(os.path.join(ROOT, 'include', 'rri_fold.h')).read()
    assert '#include "rri_hip.h"' in text and _capi.ABI_VERSION == 1
    assert re.search(r'#define RRI_ABI_VERSION 1\b', open(os.path.join(ROOT, 'include', 'rri_hip.h')).read())      # additions, not a new ABI
    declared = re.findall(r'^rri_status (rri_\w+)\(', text, flags=re.M)
    assert sorted(declared) == sorted(PROTOS) == sorted(_capi.FOLD_PROTOTYPES)
    others = (_capi.PROTOTYPES, _capi.CORPUS_OPS_PROTOTYPES, _capi.CORPUS_BUILD_PROTOTYPES, _capi.CORPUS_FIT_PROTOTYPES, _capi.CORPUS_RANK_PROTOTYPES)
    assert not any(set(_capi.FOLD_PROTOTYPES) & set(t) for t in others)
    assert not set(declared) & set(re.findall(r'(rri_\w+)\(', open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()))
    for name, want in PROTOS.items():
        proto = re.search(r'^rri_status %s\(([^;]*)\);' % name, text, flags=re.M)
        assert proto and re.sub(r'\s+', ' ', proto.group(1)) == want, name
    assert _capi.FOLD_PROTOTYPES['rri_set_fold_schedule'] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int])
    assert _capi.FOLD_PROTOTYPES['rri_fold_info'] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)])
    # the header states the limits and what a halt leaves
    for phrase in ('1 <= k <= 64', 'RRI_WEIGHTED_SPARSE', 'as they were before the sweep', 'touches no cached state', 'rows per workgroup'):
        assert phrase in text, phrase
    cc_ = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    assert cc_, 'no host C compiler'
    subprocess.run([cc_, '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c', '-I' + os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'include', 'rri_fold.h')], check=True)
    lib = _capi.load_library()
    for name, (res, args) in _capi.FOLD_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args, name
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        body = open(os.path.join(ROOT, doc)).read()
        assert all(name in body for name in PROTOS) and 'rri_fold.h' in body, doc
    assert '4.18' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'transform_corpus' in open(os.path.join(ROOT, 'README.md')).read()
    assert 'fold_corpus_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()
    assert 'r31_fold_corpus_probe.jsonl' in open(os.path.join(ROOT, 'profiles', 'README.md')).read()
    assert 'rri_fold.h' in open(os.path.join(ROOT, 'rri_nmf_amd', 'build.py')).read()
    hip = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_hip.hip')).read()
    assert '#include "rri_fold.h"' in hip and '#include "rri_fold_kernels.hpp"' in hip
    # opt-in, per handle: no environment switch, and rri_params is what it was
    assert 'getenv("RRI_FOLD' not in hip and 'fold_schedule' not in open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    # NULL handles: RRI_ERR_INVALID without a device, and nothing is written or counted
    out = (ctypes.c_int64 * 6)(*range(1, 7))
    assert lib.rri_set_fold_schedule(None, 1) == BAD and lib.rri_fold_info(None, out) == BAD and list(out) == list(range(1, 7))
    assert b'NULL' in lib.rri_last_error(None)
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.rri_device_memory(ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    # module functions, not engine methods
    from rri_nmf_amd import engine, fold
    assert callable(fold.set_fold_schedule) and callable(fold.fold_info) and fold.FOLD_MAX_K == 64
    assert not hasattr(engine.RRIEngine, 'set_fold_schedule') and not hasattr(engine.RRIEngine, 'fold_info')


# ---- nmf(fold_in=True) ---------------------------------------------------------------------------------------------------------------
class FakeCorpus(object):
    """stands in for DeviceCorpus: a shape, a device, and a to_scipy that must never be called"""

    def __init__(self, shape, device=0, nnz=5):
        self.shape, self.device, self.nnz = shape, device, nnz

    def to_scipy(self):
        raise AssertionError('folding in from a corpus downloads nothing')

    def _ptr(self):
        return self


def test_fold_in_is_refused_before_any_device_call(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod

    def no_device(*a, **kw):
        raise AssertionError('a handle was asked for')
    monkeypatch.setattr(nmf_mod, '_engine_with_problem', no_device)
    monkeypatch.setattr(nmf_mod, 'RRIEngine', no_device)
    sig = inspect.signature(nmf_mod.nmf)
    names = list(sig.parameters)
    assert names[-2:] == ['observed_only', 'fold_in'] and sig.parameters['fold_in'].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters['fold_in'].default is False
    A = sp.random(30, 20, 0.2, format='csr', random_state=0)
    Mp = A.copy()
    Mp.data[:] = 1.0
    T = np.random.RandomState(0).rand(3, 20)
    with pytest.raises(ValueError, match='fold_in=True folds rows in against a fixed T'):
        nmf_mod.nmf(A, 3, W_mat=Mp, sparse_pattern=True, fold_in=True, T_in=T)
    with pytest.raises(ValueError, match='fold_in=True runs on a pattern-only handle'):
        nmf_mod.nmf(A, 3, W_mat=Mp, fix_T=True, fold_in=True, T_in=T)                       # sparse_pattern left to the density rule
    with pytest.raises(ValueError, match='fold_in=True runs on a pattern-only handle'):
        nmf_mod.nmf(A, 3, W_mat=Mp, sparse_pattern=False, fix_T=True, fold_in=True, T_in=T)
    with pytest.raises(ValueError, match='fold_in=True runs on a pattern-only handle'):
        nmf_mod.nmf(A.toarray(), 3, fix_T=True, fold_in=True, T_in=T)                        # no weights at all
    with pytest.raises(ValueError, match='does not combine with group='):
        nmf_mod.nmf(A, 3, W_mat=Mp, sparse_pattern=True, fix_T=True, fold_in=True, T_in=T, group=object())
    with pytest.raises(ValueError, match='does not combine with resident='):
        nmf_mod.nmf(A, 3, W_mat=Mp, sparse_pattern=True, fix_T=True, fold_in=True, T_in=T, resident=object())
    with pytest.raises(ValueError, match='observed_only=True takes a DeviceCorpus'):
        nmf_mod.nmf(A, 3, observed_only=True, fix_T=True, fold_in=True, T_in=T)
    # the accepted forms reach the handle: a rank above 64 is not refused
    for k in (3, 65):
        with pytest.raises(AssertionError, match='a handle was asked for'):
            nmf_mod.nmf(A, k, W_mat=Mp, sparse_pattern=True, fix_T=True, fold_in=True, T_in=np.ones((k, 20)), W_in=np.ones((30, k)))


# ---- the estimator, behind stand-ins -------------------------------------------------------------------------------------------------
class FakeEngine(object):
    log = []

    def __init__(self, n, d, k, **kw):
        self.n, self.d, self.k, self.kw, self.closed, self.device = n, d, k, kw, False, kw.get('device', 0)
        FakeEngine.log.append(self)

    def set_W(self, W):
        self.W = np.array(W)

    def set_T(self, T):
        self.T = np.array(T)

    def close(self):
        self.closed = True


W0 = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]])
T0 = np.array([[0.5, 0.25, 0.25, 0.0], [0.0, 0.25, 0.25, 0.5]])
WN = np.array([[0.25, 0.75], [1.0, 1.0], [0.5, 0.0], [0.0, 0.0], [2.0, 1.0]])       # five folded users


@pytest.fixture
def device(monkeypatch):
    from rri_nmf_amd import corpus_fit, corpus_rank, sklearn_interface as si
    monkeypatch.setattr(si, 'RRIEngine', FakeEngine)
    monkeypatch.setattr(si, 'DeviceCorpus', FakeCorpus)
    FakeEngine.log = []
    calls = []

    def solver(*a, **kw):
        calls.append(('nmf', a, kw))
        return {'W': np.full((a[0].shape[0], a[1]), 0.5), 'T': kw['T_in']}

    def topn_rows(engine, rows=None, n_top=10, exclude=None, clip=(None, None)):
        calls.append(('topn', engine, np.array(rows), n_top, exclude, clip))
        return np.repeat(np.asarray(rows, dtype=np.int32)[:, None], n_top, axis=1), np.full((len(rows), n_top), 2.5), 0.25

    def rank_entries(engine, targets, rows=None, exclude=None, clip=(None, None), values=True):
        calls.append(('rank', engine, targets, exclude))
        return {'rank': np.arange(targets.nnz, dtype=np.int32), 'val': None, 'eligible': np.full(targets.shape[0], 4, dtype=np.int32), 'kernel_ms': 0.5}

    def ranking_metrics(engine, targets, n_items=10, rows=None, exclude=None, relevant_from=None):
        calls.append(('metrics', engine, targets, n_items, exclude, relevant_from))
        return {'users': 1}

    def entries_error(engine, corpus, rows=None, clip=(None, None), predictions=False):
        calls.append(('error', engine, corpus, clip))
        return {'rmse': 0.75}
    monkeypatch.setattr(si, '_nmf', solver)
    monkeypatch.setattr(corpus_rank, 'topn_rows', topn_rows)
    monkeypatch.setattr(corpus_rank, 'rank_entries', rank_entries)
    monkeypatch.setattr(corpus_rank, 'ranking_metrics', ranking_metrics)
    monkeypatch.setattr(corpus_fit, 'entries_error', entries_error)
    E = si.NMF_RS_Estimator(3, 4, 2, wr1=0.125, tr1=0.25, random_state=7, W=W0, T=T0, nmf_kwargs={'device': 0, 'dtype': np.float32})
    E.min_rating, E.max_rating = 1.0, 5.0
    return si, E, calls


def test_transform_corpus_hands_the_options_of_transform_to_the_solver(device):
    si, E, calls = device
    new = FakeCorpus((5, 4))
    W = E.transform_corpus(new)
    assert W.shape == (5, 2) and FakeEngine.log == []
    (call,) = calls
    assert call[1][0] is new and call[1][1] == 2
    assert call[2].pop('T_in') is T0
    assert call[2] == dict(max_iter=4, max_time=7200, project_W_each_iter=False, project_T_each_iter=False, observed_only=True,
                           fold_in=True, fix_T=True, reg_w_l1=0.125, reg_t_l1=0.25, t_row_sum=1.0, w_row_sum=None,
                           reset_topic_method='random', random_state=7, device=0, dtype=np.float32)
    # transform itself is what it was: a host mask, no fold_in
    del calls[:]
    E.transform(sp.csr_matrix(np.array([[0.0, 3.0, 0.0, 1.0]])))
    kw = calls[0][2]
    assert 'fold_in' not in kw and 'observed_only' not in kw and kw['max_iter'] == 4 and kw['fix_T'] and kw['reset_topic_method'] == 'random'
    # any number of rows; the refusals come before the solver
    del calls[:]
    assert E.transform_corpus(FakeCorpus((1, 4))).shape == (1, 2) and E.transform_corpus(FakeCorpus((70000, 4))).shape == (70000, 2)
    del calls[:]
    with pytest.raises(TypeError, match='transform_corpus takes a DeviceCorpus, not csr_matrix'):
        E.transform_corpus(sp.csr_matrix((5, 4)))
    with pytest.raises(ValueError, match='the corpus has 3 columns, the estimator 4'):
        E.transform_corpus(FakeCorpus((5, 3)))
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_RS_Estimator(3, 4, 2).transform_corpus(new)
    assert calls == []


def test_the_resident_calls_take_the_folded_rows(device):
    si, E, calls = device
    new, other = FakeCorpus((5, 4), nnz=6), FakeCorpus((3, 4))
    items, scores = E.recommend_corpus([4, 0], n_items=2, exclude=new, W=WN)
    eng = FakeEngine.log[-1]
    assert (eng.n, eng.d, eng.k) == (5, 4, 2) and eng.kw['weighted'] is False and eng.closed
    assert np.array_equal(eng.W, WN) and np.array_equal(eng.T, T0)
    assert calls[-1][0] == 'topn' and calls[-1][2].tolist() == [4, 0] and calls[-1][4] is new and items.tolist() == [[4, 4], [0, 0]]
    rank, eligible = E.rank_corpus(new, exclude=new, W=WN)
    assert FakeEngine.log[-1].n == 5 and rank.size == 6 and eligible.size == 5
    assert E.ranking_score_corpus(new, n_items=3, exclude=None, relevant_from=4.0, W=WN) == {'users': 1}
    assert FakeEngine.log[-1].n == 5 and calls[-1][3] == 3 and calls[-1][5] == 4.0
    assert E.score_corpus(new, W=WN) == 0.75
    eng = FakeEngine.log[-1]
    assert (eng.n, eng.d, eng.k) == (5, 4, 2) and np.array_equal(eng.W, WN) and calls[-1][2] is new and calls[-1][3] == (1.0, 5.0) and eng.closed
    # None keeps the fitted W
    E.recommend_corpus([2], n_items=1, exclude=other)
    assert FakeEngine.log[-1].n == 3 and np.array_equal(FakeEngine.log[-1].W, W0)
    assert E.score_corpus(other) == 0.75 and FakeEngine.log[-1].n == 3
    # the shapes are checked before a handle is opened
    opened = len(FakeEngine.log)
    with pytest.raises(ValueError, match='with W of 5 rows, exclude must be a DeviceCorpus of shape 5 x 4'):
        E.recommend_corpus([0], exclude=other, W=WN)
    with pytest.raises(ValueError, match='with W of 5 rows, targets must be a DeviceCorpus of shape 5 x 4'):
        E.rank_corpus(other, W=WN)
    with pytest.raises(ValueError, match='with W of 5 rows, corpus must be a DeviceCorpus of shape 5 x 4'):
        E.score_corpus(other, W=WN)
    with pytest.raises(ValueError, match=r'W must be an \(m, 2\) array of folded rows'):
        E.ranking_score_corpus(new, W=WN[:, :1])
    with pytest.raises(ValueError, match=r'users must be row indices in \[0, 5\)'):
        E.recommend_corpus([5], W=WN)
    assert len(FakeEngine.log) == opened + 1 and all(e.closed for e in FakeEngine.log)
    # an estimator that holds only T serves folded rows
    only_T = si.NMF_RS_Estimator(3, 4, 2, T=T0, nmf_kwargs={})
    only_T.min_rating, only_T.max_rating = 1.0, 5.0
    assert only_T.score_corpus(new, W=WN) == 0.75
