"""Ranking against resident corpora without a GPU: the request check, the pieces, the row terms and the totals of
rri_nmf_amd/csrc/rri_corpus_rank.hpp under sanitizers, the ABI surface of include/rri_corpus_rank.h and the refusals of the real
library without a handle, and NMF_RS_Estimator.recommend_corpus / rank_corpus / ranking_score_corpus behind stand-ins for the
device.

tests/c/corpus_rank_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once; what it prints is compared with what is written here
by hand, with the numpy restatement (tests/corpus_rank_cases.py) bit for bit, and through it with ranking_score's own host
arithmetic fed the same ranks.  No sanitizer is loaded into Python."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import corpus_rank_cases as cc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD, UNSUPPORTED = 0, _capi.RRI_ERR_INVALID, _capi.RRI_ERR_UNSUPPORTED
NAN = float('nan')

REQUESTS = {'fine': OK, 'rows_null': OK, 'duplicate_rows': OK, 'no_exclusion': OK, 'open': OK, 'lo_is_hi': OK, 'metrics_fine': OK,
            'metrics_many_items': OK, 'topn_fine': OK, 'topn_no_requests': OK,
            'targets_null': BAD, 'targets_destroyed': BAD, 'targets_other_device': BAD, 'exclusion_destroyed': BAD,
            'exclusion_other_device': BAD, 'exclusion_other_rows': BAD, 'exclusion_other_columns': BAD, 'other_columns': BAD,
            'rows_null_corpus_above_n': BAD, 'row_n': BAD, 'row_negative': BAD, 'lo_nan': BAD, 'hi_nan': BAD, 'lo_above_hi': BAD,
            'no_items': BAD, 'topn_negative_count': BAD, 'topn_zero': UNSUPPORTED, 'topn_65': UNSUPPORTED,
            'topn_rows_null_count_above_n': BAD, 'topn_row_n': BAD}
TEXT = {'targets_null': 'the targets corpus is NULL or has been destroyed', 'targets_destroyed': 'the targets corpus is NULL or has been destroyed',
        'targets_other_device': 'the targets corpus lives on device 1, the handle on device 0',
        'exclusion_destroyed': 'the exclusion corpus has been destroyed',
        'exclusion_other_device': 'the exclusion corpus lives on device 2, the handle on device 0',
        'exclusion_other_rows': 'the exclusion corpus is 3 x 6, the handle 4 x 6',
        'exclusion_other_columns': 'the exclusion corpus is 4 x 7, the handle 4 x 6',
        'other_columns': 'the corpus has 7 columns, W T has 6',
        'rows_null_corpus_above_n': 'rows is NULL and the corpus has 3 rows, W has 2', 'row_n': 'rows[1] = 4 is out of range',
        'row_negative': 'rows[2] = -1 is out of range', 'lo_nan': 'a clip bound is NaN (an open side is -inf or +inf)',
        'hi_nan': 'a clip bound is NaN (an open side is -inf or +inf)', 'lo_above_hi': 'clip_lo 5.5 is above clip_hi 5',
        'no_items': 'n_items 0 is not a positive integer', 'topn_negative_count': 'count -1 is negative',
        'topn_zero': 'topn 0 outside 1 .. 64', 'topn_65': 'topn 65 outside 1 .. 64',
        'topn_rows_null_count_above_n': 'rows is NULL and count 5 exceeds the 4 rows of W', 'topn_row_n': 'rows[0] = 4 is out of range'}
RULES = 14      # targets gone, their device, exclusion gone, its device, its shape, count, topn, rows NULL (two calls), columns,
#                 n_items, NaN bound, lo above hi, row range

# the case worked out by hand (corpus_rank_main.cpp): five rows of (value, rank) and an eligible count L
#   row 0  (5, 0) (3, 9) (1, -1)   L = 10        row 1  no entry   L = -1        row 2  (2, 1) (3, 2)   L = 3
#   row 3  (5, 0)   L = 1                        row 4  (5, -1)    L = 0
# pass 0: N = 1, every entry.  Row 0: P = 2, one hit, S = 9: recall 1/2, dcg / ideal = 1 / 1, auc 1 - (9 - 1) / (2 * 8) = 1/2,
#   S / (L - 1) = 9 / 9.  Row 2: P = 2, no hit, r0 = 1, S = 3: auc 1 - (3 - 1) / (2 * 1) = 0, S / (L - 1) = 3/2.  Row 3: L = P = 1:
#   neither an auc term nor a percentile.  Row 4: one target, not eligible: no user.
# pass 1: N = 2, values >= 4.  Row 0: only (5, 0): P = 1, precision 1/2, auc 1 - 0 / 9, S = 0.  Row 2: nothing relevant.
HAND_INDPTR = np.array([0, 3, 3, 5, 6, 7], dtype=np.int64)
HAND_VALUES = np.array([5.0, 3.0, 1.0, 2.0, 3.0, 5.0, 5.0])
HAND_RANK = np.array([0, 9, -1, 1, 2, 0, -1], dtype=np.int32)
HAND_ELIG = np.array([10, -1, 3, 1, 0], dtype=np.int32)
#          user targets not_el hit  prec  recall ndcg mrr  auc  room  mpr  wide
HAND = {0: dict(n_items=1, relevant_from=NAN,
                terms=[[1, 3, 1, 1, 1.0, 0.5, 1, 1.0, 0.5, 1, 1.0, 2],
                       [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                       [1, 2, 0, 0, 0, 0, 0, 0.5, 0.0, 1, 1.5, 2],
                       [1, 1, 0, 1, 1.0, 1.0, 1, 1.0, 0, 0, 0, 0],
                       [0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]],
                totals=[3, 7, 2, 2, 2.0, 1.5, 2, 2.5, 0.5, 2, 2.5, 4, 0, 0, 0, 0]),
        1: dict(n_items=2, relevant_from=4.0,
                terms=[[1, 1, 0, 1, 0.5, 1.0, 1, 1.0, 1.0, 1, 0.0, 1],
                       [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                       [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                       [1, 1, 0, 1, 0.5, 1.0, 1, 1.0, 0, 0, 0, 0],
                       [0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]],
                totals=[2, 3, 1, 2, 1.0, 2.0, 2, 2.0, 1.0, 1, 0.0, 1, 0, 0, 0, 0])}

# the cases of the file: (rows, d, seed, n_items, relevant_from); 2500 rows take three blocks of the totals' first level
FILE_CASES = [(40, 130, 1, 10, None), (40, 130, 1, 1, 4.0), (40, 130, 1, 200, 3.0), (2500, 50, 2, 5, None), (1, 30, 3, 3, None),
              (1025, 20, 4, 64, 2.0)]


def _write_cases(path):
    made = []
    with open(path, 'w') as f:
        for m, d, seed, n_items, rf in FILE_CASES:
            A, rank, elig = cc.random_case(m, d, seed)
            made.append((A, rank, elig, n_items, rf))
            f.write('%d %d %d %s\n' % (m, d, n_items, 'nan' if rf is None else repr(rf)))
            for arr, fmt in ((A.indptr, '%d'), (A.data, '%.17g'), (rank, '%d'), (elig, '%d')):
                f.write(' '.join(fmt % x for x in arr) + '\n')
    return made


def test_request_check_pieces_row_terms_and_totals_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe, cases = str(tmp_path / 'corpus_rank'), str(tmp_path / 'cases.txt')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'corpus_rank_main.cpp'), '-o', exe], check=True)
    made = _write_cases(cases)
    res = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok', lines[-1]

    # the request check, rule by rule: the verdict, and a text of its own for every broken rule
    got = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'req (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    assert {name: code for name, (code, _) in got.items()} == REQUESTS
    for name, (code, text) in got.items():
        assert (text == '') == (code == OK), name
        if code != OK:
            assert text == TEXT[name], (name, text)
    assert len({re.sub(r'-?\d[\w.+-]*', '#', t) for t in TEXT.values()}) == RULES

    # the pieces cut per corpus row: rank_cut_pieces without the rows that have no entry, and the restatement
    named = {ln.split(' :')[0]: ln.split(' :')[1].split() for ln in lines if ln.startswith(('pieces :', 'rank_cut_pieces :', 'first :'))}
    indptr = np.concatenate(([0], np.cumsum([0, 1, 63, 64, 65, 129])))
    want = cc.pieces(indptr)
    assert want == [(1, 0, 1, 1), (2, 1, 63, 1), (3, 64, 64, 1), (4, 128, 64, 1), (4, 192, 1, 0), (5, 193, 64, 1), (5, 257, 64, 0), (5, 321, 1, 0)]
    assert named['pieces'] == named['rank_cut_pieces'] == ['%d,%d,%d,%d' % p for p in want]
    assert [int(x) for x in named['first']] == [0, 0, 1, 2, 3, 5, 8]
    assert [ln for ln in lines if ln.startswith('entry :')] == ['entry : 1 1 0 1 0 1 0 0']

    # the plain loops on the hand-computed case: every term and total exact in binary
    for p, want in HAND.items():
        at = lines.index('hand %d' % p)
        terms = np.array([float(x) for x in lines[at + 1].split(' :')[1].split()]).reshape(5, cc.TERMS)
        tot = np.array([float(x) for x in lines[at + 2].split(' :')[1].split()])
        assert np.array_equal(terms, np.array(want['terms'], dtype=np.float64)), (p, terms)
        assert np.array_equal(tot, np.array(want['totals'], dtype=np.float64)), (p, tot)

    # the plain loops on the file's cases against the numpy restatement, bit for bit, and -- after the division -- against
    # ranking_score's own host arithmetic fed the same ranks, within the bound
    for c, (A, rank, elig, n_items, rf) in enumerate(made):
        at = lines.index('file %d' % c)
        terms = np.array([float.fromhex(x) for x in lines[at + 1].split(' :')[1].split()]).reshape(A.shape[0], cc.TERMS)
        tot = np.array([float.fromhex(x) for x in lines[at + 2].split(' :')[1].split()])
        ref = cc.row_terms(A.indptr, A.data, rank, elig, n_items, rf, A.shape[1])
        assert np.array_equal(cc.bits(terms), cc.bits(ref)), c
        assert np.array_equal(cc.bits(tot), cc.bits(cc.totals(ref))), c
        cc.check_metrics(cc.metrics(tot, n_items), cc.host_ranking_score(A, rank, elig, n_items, rf))


def test_the_numpy_restatement_on_the_hand_computed_case():
    for p, want in HAND.items():
        rf = None if want['relevant_from'] != want['relevant_from'] else want['relevant_from']
        terms = cc.row_terms(HAND_INDPTR, HAND_VALUES, HAND_RANK, HAND_ELIG, want['n_items'], rf, 20)
        assert np.array_equal(terms, np.array(want['terms'], dtype=np.float64)), p
        assert np.array_equal(cc.totals(terms), np.array(want['totals'], dtype=np.float64)), p
    # the division: the keys of ranking_score, NaN metrics and telling counts without a user
    got = cc.metrics(HAND[0]['totals'], 1)
    assert got == {'n_items': 1, 'users': 3, 'targets': 7, 'targets_not_eligible': 2, 'hit_rate': 2 / 3, 'precision': 2 / 3, 'recall': 0.5,
                   'ndcg': 2 / 3, 'mrr': 2.5 / 3, 'auc': 0.25, 'mean_percentile_rank': 0.625}
    A = sp.csr_matrix((HAND_VALUES, np.array([0, 1, 2, 4, 5, 7, 3], dtype=np.int32), HAND_INDPTR), shape=(5, 20))
    host = cc.host_ranking_score(A, HAND_RANK, HAND_ELIG, 1, None)
    assert set(host) == set(got)
    cc.check_metrics(got, host)
    none = cc.metrics([0, 4, 4] + [0] * 13, 10)
    assert none['users'] == 0 and none['targets'] == 4 and none['targets_not_eligible'] == 4 and all(np.isnan(none[m]) for m in cc.METRICS)
    # the trees: the order is fixed, and it is not the ascending one
    big = np.zeros(64)
    big[0], big[32], big[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert cc.tree64(big) == 1.0 and (big[0] + (big[32] + big[1])) > 1.0


PROTOS = {
    'rri_corpus_topn_rows': 'rri_ctx* ctx, const int64_t* rows, int64_t count, int32_t topn, const rri_corpus* exclude, double clip_lo, '
                            'double clip_hi, int32_t* idx_out, double* val_out, double* kernel_ms',
    'rri_corpus_rank_entries': 'rri_ctx* ctx, const rri_corpus* targets, const int64_t* rows, const rri_corpus* exclude, double clip_lo, '
                               'double clip_hi, int32_t* rank_out, double* val_out, int32_t* eligible_out, double* kernel_ms',
    'rri_corpus_ranking_metrics': 'rri_ctx* ctx, const rri_corpus* targets, const int64_t* rows, const rri_corpus* exclude, '
                                  'int64_t n_items, double relevant_from, double out[16], double* kernel_ms',
}
CTYPES = {'rri_ctx*': ctypes.c_void_p, 'const rri_corpus*': ctypes.c_void_p, 'const int64_t*': ctypes.POINTER(ctypes.c_int64),
          'double': ctypes.c_double, 'double*': ctypes.POINTER(ctypes.c_double), 'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32,
          'int32_t*': ctypes.POINTER(ctypes.c_int32)}


def test_the_new_header_is_plain_c_bound_exported_documented_and_refuses_without_a_handle():
    text = open(os.path.join(ROOT, 'include', 'rri_corpus_rank.h')).read()
    assert '#include "rri_hip.h"' in text and _capi.ABI_VERSION == 1
    assert re.search(r'#define RRI_ABI_VERSION 1\b', open(os.path.join(ROOT, 'include', 'rri_hip.h')).read())      # additions, not a new ABI
    declared = re.findall(r'^rri_status (rri_\w+)\(', text, flags=re.M)
    assert sorted(declared) == sorted(PROTOS) == sorted(_capi.CORPUS_RANK_PROTOTYPES)
    assert not set(_capi.CORPUS_RANK_PROTOTYPES) & (set(_capi.PROTOTYPES) | set(_capi.CORPUS_OPS_PROTOTYPES) | set(_capi.CORPUS_BUILD_PROTOTYPES) |
                                                    set(_capi.CORPUS_FIT_PROTOTYPES))
    for name, want in PROTOS.items():
        proto = re.search(r'^rri_status %s\(([^;]*)\);' % name, text, flags=re.M)
        assert proto and re.sub(r'\s+', ' ', proto.group(1)) == want, name
        res, args = _capi.CORPUS_RANK_PROTOTYPES[name]
        kinds = [re.sub(r' ?\w+\[\d+\]$', '*', a) if '[' in a else a.rsplit(' ', 1)[0] for a in want.split(', ')]
        assert res is ctypes.c_int32 and args == [CTYPES[kd] for kd in kinds], name
    # the header compiles as C99, alone
    cc_ = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    assert cc_, 'no host C compiler'
    subprocess.run([cc_, '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c', '-I' + os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'include', 'rri_corpus_rank.h')], check=True)
    # every declared symbol is exported and typed by load_library
    lib = _capi.load_library()
    for name, (res, args) in _capi.CORPUS_RANK_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args, name
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        body = open(os.path.join(ROOT, doc)).read()
        assert all(name in body for name in PROTOS) and 'rri_corpus_rank.h' in body, doc
    assert 'corpus_rank_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()
    assert 'rri_corpus_rank.h' in open(os.path.join(ROOT, 'rri_nmf_amd', 'build.py')).read()
    hip = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_hip.hip')).read()
    assert '#include "rri_corpus_rank.h"' in hip and '#include "rri_corpus_rank_kernels.hpp"' in hip
    # the two scoring kernels take the row of the exclusion that serves a request; the entry points of host lists pass none
    for kernel in ('rri_topn_kernels.hpp', 'rri_rank_kernels.hpp'):
        assert 'const i64* __restrict__ erow' in open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', kernel)).read(), kernel
    # NULL arguments: RRI_ERR_INVALID without a device, and nothing is written or counted
    out = (ctypes.c_double * 16)(*range(1, 17))
    ms = ctypes.c_double(5.0)
    idx, val = (ctypes.c_int32 * 2)(7, 8), (ctypes.c_double * 2)(7.0, 8.0)
    assert lib.rri_corpus_topn_rows(None, None, 2, 1, None, 1.0, 5.0, idx, val, ctypes.byref(ms)) == BAD
    assert lib.rri_corpus_rank_entries(None, None, None, None, 1.0, 5.0, idx, val, idx, ctypes.byref(ms)) == BAD
    assert lib.rri_corpus_ranking_metrics(None, None, None, None, 10, NAN, out, ctypes.byref(ms)) == BAD
    assert list(out) == list(range(1, 17)) and ms.value == 5.0 and list(idx) == [7, 8] and list(val) == [7.0, 8.0]
    for counter in (lib.rri_corpus_memory, lib.rri_device_memory):
        a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert counter(ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (0, 0)


# ---- the estimator, behind stand-ins for the device ------------------------------------------------------------------------------
class FakeCorpus(object):
    """stands in for DeviceCorpus: a shape, a device, and a to_scipy that must never be called"""

    def __init__(self, shape, device=0, nnz=5):
        self.shape, self.device, self.nnz = shape, device, nnz

    def to_scipy(self):
        raise AssertionError('ranking against a corpus downloads nothing')

    def _ptr(self):
        return self


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


@pytest.fixture
def device(monkeypatch):
    from rri_nmf_amd import corpus_rank, sklearn_interface as si
    monkeypatch.setattr(si, 'RRIEngine', FakeEngine)
    monkeypatch.setattr(si, 'DeviceCorpus', FakeCorpus)
    FakeEngine.log = []
    calls = []

    def topn_rows(engine, rows=None, n_top=10, exclude=None, clip=(None, None)):
        calls.append(('topn', engine, np.array(rows), n_top, exclude, clip))
        m = len(rows)
        return np.repeat(np.asarray(rows, dtype=np.int32)[:, None], n_top, axis=1), np.full((m, n_top), 2.5), 0.25

    def rank_entries(engine, targets, rows=None, exclude=None, clip=(None, None), values=True):
        calls.append(('rank', engine, targets, rows, exclude, clip, values))
        return {'rank': np.arange(targets.nnz, dtype=np.int32), 'val': None, 'eligible': np.full(targets.shape[0], 4, dtype=np.int32), 'kernel_ms': 0.5}

    sums = [[2, 5, 1, 1, 0.5, 1.5, 1.25, 1.5, 0.5, 1, 0.75, 3, 0, 0, 0, 0]]

    def ranking_sums(engine, targets, n_items=10, rows=None, exclude=None, relevant_from=None):
        calls.append(('metrics', engine, targets, n_items, rows, exclude, relevant_from))
        return np.array(sums[0], dtype=np.float64), 0.125
    monkeypatch.setattr(corpus_rank, 'topn_rows', topn_rows)
    monkeypatch.setattr(corpus_rank, 'rank_entries', rank_entries)
    monkeypatch.setattr(corpus_rank, 'ranking_sums', ranking_sums)
    E = si.NMF_RS_Estimator(3, 4, 2, W=W0, T=T0, nmf_kwargs={'device': 0})
    E.min_rating, E.max_rating = 1.0, 5.0
    return si, E, calls, sums


def test_recommend_corpus_behind_a_stand_in_device(device, monkeypatch):
    si, E, calls, _ = device
    full = FakeCorpus((3, 4))
    items, scores = E.recommend_corpus([2, 0, 2], n_items=2, exclude=full)
    (eng,) = FakeEngine.log
    assert (eng.n, eng.d, eng.k) == (3, 4, 2) and eng.kw['weighted'] is False and eng.kw['dtype'] == np.float64 and eng.closed
    assert np.array_equal(eng.W, W0) and np.array_equal(eng.T, T0)          # factors only: nothing else reaches the handle
    (call,) = calls
    assert call[1] is eng and call[2].tolist() == [2, 0, 2] and call[3] == 2 and call[4] is full and call[5] == (1.0, 5.0)
    assert items.dtype == np.int32 and items.tolist() == [[2, 2], [0, 0], [2, 2]] and scores.shape == (3, 2) and np.all(scores == 2.5)
    # every user; chunks of _RECOMMEND_CHUNK users, the exclusion passed whole to each
    del calls[:]
    monkeypatch.setattr(si, '_RECOMMEND_CHUNK', 2)
    items, _ = E.recommend_corpus(n_items=1)
    assert [c[2].tolist() for c in calls] == [[0, 1], [2]] and all(c[4] is None for c in calls) and items[:, 0].tolist() == [0, 1, 2]
    del calls[:]
    E.recommend_corpus([1, 1, 0], n_items=1, exclude=full)
    assert [c[2].tolist() for c in calls] == [[1, 1], [0]] and all(c[4] is full for c in calls)
    # refusals, each before any device call; every handle that was opened is closed
    del calls[:]
    with pytest.raises(ValueError, match=r'users must be row indices in \[0, 3\)'):
        E.recommend_corpus([0, 3])
    with pytest.raises(TypeError, match='exclude must be a DeviceCorpus, not csr_matrix'):
        E.recommend_corpus([0], exclude=sp.csr_matrix((3, 4)))
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_RS_Estimator(3, 4, 2).recommend_corpus([0])
    assert calls == [] and all(e.closed for e in FakeEngine.log)
    # the host routes keep their downloads and say where the resident ones are
    assert 'recommend_corpus' in si.NMF_RS_Estimator.recommend.__doc__ and 'rank_corpus' in si.NMF_RS_Estimator.rank.__doc__
    assert 'ranking_score_corpus' in si.NMF_RS_Estimator.ranking_score.__doc__
    for name in ('rank', 'ranking_score'):
        assert 'through one\n        to_scipy() download' in getattr(si.NMF_RS_Estimator, name).__doc__ or \
            'through one to_scipy() download' in getattr(si.NMF_RS_Estimator, name).__doc__


def test_rank_corpus_and_ranking_score_corpus_behind_a_stand_in_device(device):
    si, E, calls, sums = device
    test, full = FakeCorpus((3, 4), nnz=5), FakeCorpus((3, 4), nnz=9)
    rank, eligible = E.rank_corpus(test, exclude=full)
    (call,) = calls
    assert call[2] is test and call[3] is None and call[4] is full and call[5] == (1.0, 5.0) and call[6] is False
    assert rank.tolist() == [0, 1, 2, 3, 4] and eligible.tolist() == [4, 4, 4] and FakeEngine.log[-1].closed
    del calls[:]
    got = E.ranking_score_corpus(test, n_items=7, exclude=full, relevant_from=4.0)
    (call,) = calls
    assert call[2] is test and call[3] == 7 and call[4] is None and call[5] is full and call[6] == 4.0 and FakeEngine.log[-1].closed
    assert got == {'n_items': 7, 'users': 2, 'targets': 5, 'targets_not_eligible': 1, 'hit_rate': 0.5, 'precision': 0.25, 'recall': 0.75,
                   'ndcg': 0.625, 'mrr': 0.75, 'auc': 0.5, 'mean_percentile_rank': 0.25}
    # the keys are ranking_score's; without a user the metrics are NaN and the counts tell why
    A = sp.csr_matrix((HAND_VALUES, np.array([0, 1, 2, 4, 5, 7, 3], dtype=np.int32), HAND_INDPTR), shape=(5, 20))
    assert set(got) == set(cc.host_ranking_score(A, HAND_RANK, HAND_ELIG, 1, None))
    sums[0] = [0, 5, 5] + [0] * 13
    got = E.ranking_score_corpus(test)
    assert got['users'] == 0 and got['targets'] == 5 and got['targets_not_eligible'] == 5 and got['n_items'] == 10
    assert all(np.isnan(got[m]) for m in cc.METRICS)
    # refusals, each before any device call
    del calls[:]
    with pytest.raises(ValueError, match='n_items must be a positive integer, not 0'):
        E.ranking_score_corpus(test, n_items=0)
    for method in (E.rank_corpus, E.ranking_score_corpus):
        with pytest.raises(TypeError, match='targets must be a DeviceCorpus, not csr_matrix'):
            method(sp.csr_matrix((3, 4)))
        with pytest.raises(TypeError, match='exclude must be a DeviceCorpus, not ndarray'):
            method(test, exclude=np.zeros((3, 4)))
        with pytest.raises(ValueError, match='targets must be a DeviceCorpus of shape 3 x 4'):
            method(FakeCorpus((3, 5)))
        with pytest.raises(ValueError, match='targets must be a DeviceCorpus of shape 3 x 4'):
            method(None)
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_RS_Estimator(3, 4, 2).rank_corpus(test)
    assert calls == [] and all(e.closed for e in FakeEngine.log)


def test_the_python_functions_check_their_arguments_before_the_library():
    from rri_nmf_amd import corpus_rank as cr

    class Eng(object):
        n, d, device = 3, 4, 0
    with pytest.raises(TypeError, match='corpus must be a DeviceCorpus'):
        cr.rank_entries(Eng(), sp.csr_matrix((3, 4)))
    one = cr.metrics_from_sums([1, 1, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0], 3)
    assert np.isnan(one['auc']) and np.isnan(one['mean_percentile_rank']) and one['mrr'] == 1.0      # a user, but no room and no width
    assert cr._clip((None, 5.0)) == (float('-inf'), 5.0) and cr._clip((1, None)) == (1.0, float('inf'))
