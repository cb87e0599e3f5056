"""A CSR corpus on the device, without a GPU: the check and its texts, the row classes and the plain loop of
rri_nmf_amd/csrc/rri_corpus.hpp under sanitizers, the ABI surface and the refusals of the real library that need no device, and
NMF_TM_Estimator.coherence / log_likelihood / perplexity with stand-ins for the device handle and the corpus.

tests/c/corpus_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once; what it prints -- the verdict and text of 34 raw
matrices, the class and pad of 13 row lengths, the key, and six seeded matrices with their canonical form -- is compared with
what is written here and with the numpy restatement (tests/corpus_cases.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import corpus_cases as cc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINE = ['fine', 'unsorted_duplicates_zeros_negatives', 'pattern', 'narrow_dtypes', 'no_rows', 'no_entries', 'widest_n_cols',
        'pattern_ignores_values']
ARGS = {'negative_n_rows': 'n_rows -1 is negative', 'negative_n_cols': 'n_cols -1 is negative',
        'negative_nnz': 'nnz_stored -1 is negative', 'indptr_dtype': 'indptr dtype code 0 is neither RRI_I32 nor RRI_I64',
        'indices_dtype': 'indices dtype code 7 is neither RRI_I32 nor RRI_I64',
        'values_dtype': 'values dtype code 8 is neither RRI_F32 nor RRI_F64', 'indptr_null': 'indptr is NULL',
        'indices_null': 'indices is NULL with 5 entries'}
NARROW = {'narrow_column_6_at_entry_3': 'column 6 at entry 3 is out of range', 'narrow_value_inf_at_entry_1': 'value inf at entry 1 is not finite'}


def test_check_classes_and_plain_loop_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'corpus')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'corpus_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok 6 cases', lines[-1]

    # the check: the verdict and the text of every refusal, each rule at two places, the first broken rule wins
    got = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'req (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    assert set(got) == set(FINE) | set(ARGS) | set(NARROW) | set(cc.MALFORMED)
    for name in FINE:
        assert got[name] == (cc.OK, ''), name
    for name, text in list(ARGS.items()) + list(NARROW.items()):
        assert got[name] == (cc.INVALID, text), name
    for name, (indptr, indices, values, shape) in cc.MALFORMED.items():
        want = cc.check(indptr, indices, values, shape)
        assert want[1] == cc.TEXT[name] and want[0] == (cc.UNSUPPORTED if name.startswith('n_cols') else cc.INVALID), name
        assert got[name] == want, name
    assert len({re.sub(r'-?\d[\w.+-]*|-?nan|-?inf', '#', t.replace('2^31', 'two_31')) for t in cc.TEXT.values()}) == cc.RULES

    # the classes on both sides of every border, and the pad
    assert 'borders : %d %d %d' % (cc.WAVE_MAX, cc.LDS_MAX, cc.PAD_MIN) in lines
    classes = {int(ln.split()[1]): [int(x) for x in ln.split(' :')[1].split()] for ln in lines if ln.startswith('class ')}
    assert set(classes) == {0, 1, 2, 63, 64, 65, 127, 128, 129, 16383, 16384, 16385, 1 << 20}
    for length, (plain, flagged, padded) in classes.items():
        assert plain == cc.ROW_CANONICAL == cc.row_class(False, length) and flagged == cc.row_class(True, length), length
        assert padded == cc.pad(length) and padded >= length and padded & (padded - 1) == 0, length
    assert [classes[n][1] for n in (64, 65, 16384, 16385)] == [cc.ROW_SHORT, cc.ROW_MEDIUM, cc.ROW_MEDIUM, cc.ROW_LONG]
    assert cc.WAVE_MAX < cc.LDS_MAX and cc.LDS_MAX * 8 + 8192 <= 160 * 1024           # the keys of the longest LDS row fit a CU's LDS
    assert 'key : 2147483647 4294967294 1 1' in lines

    # the plain loop against the restatement: the same float64 additions in the same order, so equality is exact
    rec = {}
    for ln in lines:
        kind, _, rest = ln.partition(' ')
        if kind in ('case', 'rawptr', 'rawidx', 'rawval', 'indptr', 'indices', 'values', 'stats'):
            head, _, body = rest.partition(' :')
            rec.setdefault(int(head), {})[kind] = np.array(body.split(), dtype=np.float64)
    assert len(rec) == 6
    seen = dict(duplicates=0, zeros=0, negatives=0, pattern=0, float32=0, int32=0, empty_row=0, no_rows=0, order_of_the_sum=0)
    for cid, r in sorted(rec.items()):
        n_rows, n_cols, pdt, idt, vdt, pattern = (int(x) for x in r['case'])
        values = None if pattern else r['rawval'].astype(np.float32) if vdt == _capi.RRI_F32 else r['rawval']
        if values is not None:
            assert np.array_equal(values.astype(np.float64), r['rawval']), cid              # float32 cases print float32 numbers
        indptr, indices, vals, st = cc.canonical(r['rawptr'], r['rawidx'], values, (n_rows, n_cols))
        assert np.array_equal(r['indptr'], indptr) and np.array_equal(r['indices'], indices), cid
        assert np.array_equal(r['values'], vals), cid
        assert [int(x) for x in r['stats']] == [st[key] for key in ('rows_rewritten', 'duplicates_merged', 'zeros_dropped', 'negatives', 'long_rows')], cid
        assert r['rawidx'].size == indices.size + st['duplicates_merged'] + st['zeros_dropped'], cid
        assert all(np.all(np.diff(indices[indptr[q]:indptr[q + 1]]) > 0) for q in range(n_rows)) and not np.any(vals == 0), cid
        seen['duplicates'] += st['duplicates_merged'] > 0
        seen['zeros'] += st['zeros_dropped'] > 0
        seen['negatives'] += st['negatives'] > 0
        seen['pattern'] += pattern
        seen['float32'] += vdt == _capi.RRI_F32 and not pattern
        seen['int32'] += pdt == _capi.RRI_I32 or idt == _capi.RRI_I32
        seen['empty_row'] += bool(n_rows and (np.diff(indptr) == 0).any())
        seen['no_rows'] += n_rows == 0
        if cid == 3:        # the two planted rows: (1e16 + 1) - 1e16 = 0 is dropped, (1e16 - 1e16) + 1 = 1 stays
            a, b = n_rows - 2, n_rows - 1
            assert indices[indptr[a]:indptr[a + 1]].tolist() == [2] and vals[indptr[a]:indptr[a + 1]].tolist() == [5.0]
            assert indices[indptr[b]:indptr[b + 1]].tolist() == [1, 2] and vals[indptr[b]:indptr[b + 1]].tolist() == [1.0, 5.0]
            seen['order_of_the_sum'] += 1
    assert all(seen.values()), seen


def test_the_restatement_agrees_with_scipy_on_integers():
    lengths = [0, 1, 2, 63, 64, 65, 200]
    raw = cc.raw_rows(lengths, 150, seed=5, zeros=0.1)
    indptr, indices, vals, st = cc.canonical(*raw)
    A = cc.scipy_canonical(*raw)
    assert np.array_equal(A.indptr, indptr) and np.array_equal(A.indices, indices) and np.array_equal(A.data, vals)
    assert st['duplicates_merged'] > 0 and st['zeros_dropped'] > 0 and st['negatives'] > 0 and st['rows_rewritten'] >= 5
    assert np.diff(raw[0]).tolist() == lengths and raw[1].size == indices.size + st['duplicates_merged'] + st['zeros_dropped']
    assert cc.canonical(A.indptr, A.indices, A.data, A.shape)[3]['rows_rewritten'] == 0       # canonical stays as it is


def gpu_present():
    lib = _capi.load_library()
    h = ctypes.c_void_p()
    st = lib.rri_create(ctypes.byref(h), 4, 4, 2, 0, 0, 0, None)
    if st == 0:
        lib.rri_destroy(h)
    return st == 0


PROTOS = {
    'rri_corpus_create': 'rri_ctx* ctx, rri_corpus** out, int64_t n_rows, int64_t n_cols, int64_t nnz_stored, const void* indptr, '
                         'int32_t indptr_dtype, const void* indices, int32_t indices_dtype, const void* values, int32_t values_dtype, '
                         'int32_t on_device',
    'rri_corpus_destroy': 'rri_corpus* corpus',
    'rri_corpus_info': 'const rri_corpus* corpus, int64_t* out, int32_t n, double* ingest_ms',
    'rri_corpus_get': 'rri_ctx* ctx, const rri_corpus* corpus, int64_t* indptr_out, int32_t* indices_out, double* values_out',
    'rri_corpus_memory': 'int64_t* corpora, int64_t* bytes',
    'rri_corpus_cooccurrence_counts': 'rri_ctx* ctx, const rri_corpus* corpus, const int32_t* words, int32_t n_groups, '
                                      'int32_t group_size, int64_t* df_out, int64_t* codf_out',
    'rri_corpus_entries_loglik': 'rri_ctx* ctx, const rri_corpus* corpus, const int64_t* rows, double floor, double* ll_out, '
                                 'double* mass_out, int64_t* floored_out',
}
CTYPES = {'rri_ctx*': ctypes.c_void_p, 'rri_corpus*': ctypes.c_void_p, 'const rri_corpus*': ctypes.c_void_p, 'const void*': ctypes.c_void_p,
          'rri_corpus**': ctypes.POINTER(ctypes.c_void_p), 'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'double': ctypes.c_double,
          'int64_t*': ctypes.POINTER(ctypes.c_int64), 'const int64_t*': ctypes.POINTER(ctypes.c_int64),
          'int32_t*': ctypes.POINTER(ctypes.c_int32), 'const int32_t*': ctypes.POINTER(ctypes.c_int32), 'double*': ctypes.POINTER(ctypes.c_double)}


def test_the_entry_points_are_declared_bound_documented_and_refuse_without_a_device():
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    assert re.search(r'#define RRI_ABI_VERSION 1\b', text) and _capi.ABI_VERSION == 1          # additions, not a new ABI
    assert re.search(r'typedef struct rri_corpus rri_corpus;', text)
    assert re.search(r'RRI_I32 = 8, RRI_I64 = 9', text) and (_capi.RRI_I32, _capi.RRI_I64) == (8, 9)
    assert re.search(r'#define RRI_CORPUS_INFO_FIELDS 10\b', text) and _capi.RRI_CORPUS_INFO_FIELDS == 10
    for name, want in PROTOS.items():
        proto = re.search(r'^rri_status %s\(([^;]*)\);' % name, text, flags=re.M)
        assert proto and re.sub(r'\s+', ' ', proto.group(1)) == want, name
        res, args = _capi.PROTOTYPES[name]
        assert res is ctypes.c_int32 and args == [CTYPES[a.rsplit(' ', 1)[0]] for a in want.split(', ')], name
    # the header still compiles as C99
    cc_ = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    assert cc_, 'no host C compiler'
    subprocess.run([cc_, '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'rri_hip.h')], check=True)
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        body = open(os.path.join(ROOT, doc)).read()
        assert 'DeviceCorpus' in body and 'rri_corpus_create' in body, doc
    assert 'corpus_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()

    # without a handle nothing is made, read or counted; the counter needs none
    lib = _capi.load_library()
    ptr, ind, val = (ctypes.c_int64 * 3)(0, 1, 2), (ctypes.c_int32 * 2)(0, 1), (ctypes.c_double * 2)(1.0, 2.0)
    out = ctypes.c_void_p(7)
    BAD = _capi.RRI_ERR_INVALID
    assert lib.rri_corpus_create(None, ctypes.byref(out), 2, 2, 2, ptr, 9, ind, 8, val, 1, 0) == BAD and out.value == 7
    assert lib.rri_corpus_destroy(None) == BAD and lib.rri_corpus_info(None, None, 0, None) == BAD
    assert lib.rri_corpus_get(None, None, None, None, None) == BAD
    assert lib.rri_corpus_cooccurrence_counts(None, None, None, 1, 1, None, None) == BAD
    assert lib.rri_corpus_entries_loglik(None, None, None, 0.0, None, None, None) == BAD
    corpora, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.rri_corpus_memory(ctypes.byref(corpora), ctypes.byref(nbytes)) == 0 and (corpora.value, nbytes.value) == (0, 0)
    assert lib.rri_corpus_memory(None, None) == 0
    from rri_nmf_amd import engine
    assert engine.corpus_memory() == (0, 0)
    if gpu_present():       # with a handle: the arguments are refused before any device call, and a NULL corpus by every consumer
        h = ctypes.c_void_p()
        assert lib.rri_create(ctypes.byref(h), 4, 4, 2, 0, 0, 0, None) == 0
        try:
            assert lib.rri_corpus_create(h, None, 2, 2, 2, ptr, 9, ind, 8, val, 1, 0) == BAD and b'output pointer is NULL' in lib.rri_last_error(h)
            assert lib.rri_corpus_create(h, ctypes.byref(out), -1, 2, 2, ptr, 9, ind, 8, val, 1, 0) == BAD and not out.value
            assert b'n_rows -1 is negative' in lib.rri_last_error(h)
            assert lib.rri_corpus_create(h, ctypes.byref(out), 2, 2, 2, ptr, 1, ind, 8, val, 1, 0) == BAD and b'indptr dtype code 1' in lib.rri_last_error(h)
            assert lib.rri_corpus_create(h, ctypes.byref(out), 2, 2, 2, None, 9, ind, 8, val, 1, 0) == BAD
            assert lib.rri_corpus_create(h, ctypes.byref(out), 2, 2, 2, ptr, 9, None, 8, val, 1, 0) == BAD
            assert lib.rri_corpus_get(h, None, None, None, None) == BAD and b'the corpus is NULL' in lib.rri_last_error(h)
            assert lib.rri_corpus_memory(ctypes.byref(corpora), None) == 0 and corpora.value == 0
        finally:
            lib.rri_destroy(h)
    else:                   # no host route: a corpus needs the device like everything else
        with pytest.raises(_capi.RRIHipUnavailable):
            engine.DeviceCorpus(sp.csr_matrix(np.ones((2, 2))))


class FakeCorpus(object):
    """stands in for DeviceCorpus: a shape, a device, and a to_scipy that counts its downloads"""

    def __init__(self, A, device=5):
        self.A, self.shape, self.device, self.downloads = sp.csr_matrix(A), A.shape, device, 0

    def to_scipy(self):
        self.downloads += 1
        return self.A


class FakeEngine(object):
    """stands in for RRIEngine behind the estimator: keeps what it was made with and what it was given"""
    log = []

    def __init__(self, n, d, k, **kw):
        self.shape, self.kw, self.closed, self.calls = (n, d, k), kw, False, []
        FakeEngine.log.append(self)

    def set_W(self, W):
        self.W = np.array(W)

    def set_T(self, T):
        self.T = np.array(T)

    def cooccurrence_counts(self, A, words):
        self.calls.append(('cooc', A))
        g, M = words.shape
        return np.ones((g, M), dtype=np.int64), np.ones((g, M, M), dtype=np.int64)

    def entries_loglik(self, rows, A, floor=0.0):
        self.calls.append(('loglik', A))
        m = A.shape[0]
        return -np.ones(m), np.ones(m), np.zeros(m, dtype=np.int64)

    def close(self):
        self.closed = True


def test_the_estimator_hands_a_corpus_to_the_corpus_route_and_a_matrix_to_the_old_one(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    monkeypatch.setattr(si, 'RRIEngine', FakeEngine)
    monkeypatch.setattr(si, 'DeviceCorpus', FakeCorpus)
    FakeEngine.log = []
    T = np.array([[0.5, 0.25, 0.25, 0.0], [0.0, 0.25, 0.25, 0.5]])
    W = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]])
    X = np.array([[2.0, 0.0, 1.0, 1.0], [0.0, 4.0, 0.0, 0.0], [0.0, 0.0, 3.0, 0.0]])
    E = si.NMF_TM_Estimator(3, 4, 2, W=W, T=T, nmf_kwargs={'device': 3})
    corpus = FakeCorpus(X)
    # coherence: the corpus goes through as it is, on the corpus's device; a matrix still arrives as a CSR matrix on the estimator's
    E.coherence(corpus, n_words=2)
    eng = FakeEngine.log[-1]
    assert eng.closed and eng.calls[0][1] is corpus and eng.kw['device'] == 5 and corpus.downloads == 0
    out = E.coherence(sp.coo_matrix(X), n_words=2)
    eng = FakeEngine.log[-1]
    assert sp.isspmatrix_csr(eng.calls[0][1]) and eng.kw['device'] == 3 and out['documents'] == 3
    with pytest.raises(ValueError, match='columns'):
        E.coherence(FakeCorpus(X[:, :3]))
    # log_likelihood with W: no download, the corpus reaches entries_loglik; a matrix reaches it as a CSR matrix
    got = E.log_likelihood(corpus, W=W)
    eng = FakeEngine.log[-1]
    assert eng.calls == [('loglik', corpus)] and eng.shape == (3, 4, 2) and eng.kw['device'] == 5 and corpus.downloads == 0
    assert got['documents'] == 3 and got['log_likelihood'] == -3.0
    E.log_likelihood(X, W=W)
    assert sp.isspmatrix_csr(FakeEngine.log[-1].calls[0][1]) and FakeEngine.log[-1].kw['device'] == 3
    # without W the fold-in runs on the downloaded matrix; perplexity(held, observed=matrix) downloads nothing
    folded = []

    def transform(Xnew):
        folded.append(Xnew)
        return W
    monkeypatch.setattr(E, 'transform', transform)
    E.log_likelihood(corpus)
    assert corpus.downloads == 1 and folded[-1] is corpus.A and FakeEngine.log[-1].calls == [('loglik', corpus)]
    E.perplexity(corpus)
    assert corpus.downloads == 2 and folded[-1] is corpus.A
    observed = sp.csr_matrix(2.0 * X)
    ppl = E.perplexity(corpus, observed=observed)
    assert corpus.downloads == 2 and folded[-1] is observed and FakeEngine.log[-1].calls == [('loglik', corpus)] and isinstance(ppl, float)
    with pytest.raises(ValueError, match='one row per document'):
        E.log_likelihood(corpus, W=W[:2])
