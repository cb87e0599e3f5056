"""Log-likelihood of stored counts and held-out perplexity without a GPU: the request check, the pieces, the chunks, the lane rule
and the plain loop of rri_nmf_amd/csrc/rri_loglik.hpp under sanitizers, the ABI surface and the refusals of the real library, and
NMF_TM_Estimator.log_likelihood / perplexity and split_counts with a stand-in for the device handle.

tests/c/loglik_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once; what it prints -- the verdict and text of 31
requests, the pieces of six segments, six cuts into chunks, the lanes for k = 1 .. 1024 and the results of eight seeded cases --
is compared with what is written here and with the numpy restatement (tests/loglik_cases.py)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import loglik_cases as lc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD, UNSUPPORTED = 0, _capi.RRI_ERR_INVALID, _capi.RRI_ERR_UNSUPPORTED

REQUESTS = {'fine': OK, 'no_requests': OK, 'no_entries': OK, 'rows_null': OK, 'duplicate_rows': OK, 'explicit_zero_value': OK,
            'floor_zero': OK, 'widest_d': OK, 'd_too_wide': UNSUPPORTED, 'negative_count': BAD, 'floor_negative': BAD,
            'floor_nan': BAD, 'floor_infinite': BAD, 'indptr_null': BAD, 'rows_null_count_above_n': BAD, 'row_n': BAD,
            'row_negative': BAD, 'indptr_not_from_zero': BAD, 'indptr_decreases': BAD, 'indices_null': BAD, 'values_null': BAD,
            'column_d': BAD, 'column_negative': BAD, 'column_twice': BAD, 'columns_descend': BAD, 'value_negative': BAD,
            'value_nan': BAD, 'value_infinite': BAD, 'll_null': BAD, 'mass_null': BAD, 'floored_null': BAD}
# requests that break the same rule at another place, or with another number, share the rule's text but for that
TEXT = {'d_too_wide': 'a full row of d = 5592406 entries does not fit the upload budget of 67108864 bytes',
        'negative_count': 'count -1 is negative', 'floor_negative': 'floor -1e-300 is not a finite number >= 0',
        'floor_nan': 'floor nan is not a finite number >= 0', 'floor_infinite': 'floor inf is not a finite number >= 0',
        'indptr_null': 'indptr is NULL', 'rows_null_count_above_n': 'rows is NULL and count 3 exceeds the 2 rows of W',
        'row_n': 'rows[1] = 4 is out of range', 'row_negative': 'rows[2] = -1 is out of range',
        'indptr_not_from_zero': 'indptr[0] = 1, not 0', 'indptr_decreases': 'indptr decreases at 2',
        'indices_null': 'indices is NULL with entries in request 0', 'values_null': 'values is NULL with entries in request 0',
        'column_d': 'column 6 of request 0 is out of range', 'column_negative': 'column -1 of request 0 is out of range',
        'column_twice': 'columns of request 2 do not ascend strictly at entry 3',
        'columns_descend': 'columns of request 0 do not ascend strictly at entry 1',
        'value_negative': 'value -0.5 at entry 2 of request 2 is not a finite number >= 0',
        'value_nan': 'value nan at entry 3 of request 2 is not a finite number >= 0',
        'value_infinite': 'value inf at entry 4 of request 2 is not a finite number >= 0',
        'll_null': 'an output array is NULL with 3 requests', 'mass_null': 'an output array is NULL with 3 requests',
        'floored_null': 'an output array is NULL with 3 requests'}
RULES = 14        # texts that differ by more than a place or a number: d, count, floor, indptr NULL, rows NULL, row range, indptr[0],
#                   indptr decreasing, indices NULL, values NULL, column range, column order, value, output NULL
S = lc.LL_SEG
# a request without entries in front, the segment, a request of one entry behind: (request:first entry:count), then first piece per request
PIECES = {0: (['2:0:1'], [0, 0, 0, 1]), 1: (['1:0:1', '2:1:1'], [0, 0, 1, 2]),
          S - 1: (['1:0:%d' % (S - 1), '2:%d:1' % (S - 1)], [0, 0, 1, 2]), S: (['1:0:%d' % S, '2:%d:1' % S], [0, 0, 1, 2]),
          S + 1: (['1:0:%d' % S, '1:%d:1' % S, '2:%d:1' % (S + 1)], [0, 0, 2, 3]),
          2 * S + 3: (['1:0:%d' % S, '1:%d:%d' % (S, S), '1:%d:3' % (2 * S), '2:%d:1' % (2 * S + 3)], [0, 0, 3, 4])}
CHUNKS = {'none': ([], 1200), 'budget_below_one_request': ([5, 0, 7, 3], 24), 'exactly_one_chunk': ([40, 0, 50, 10, 0], 1200),
          'one_entry_more': ([40, 0, 50, 11, 0], 1200), 'budget_not_a_multiple': ([40, 0, 50, 10, 1], 1211),
          'empty_requests_in_front': ([0, 0, 100, 1], 1200)}


def expected_chunks(lengths, budget):
    """whole requests while their entries fit budget // 12, at least one request per chunk"""
    cap, out, q0 = budget // 12, [], 0
    while q0 < len(lengths):
        q1 = q0 + 1
        while q1 < len(lengths) and sum(lengths[q0:q1 + 1]) <= cap:
            q1 += 1
        out.append((q0, q1))
        q0 = q1
    return out


def test_request_check_pieces_chunks_lanes_and_plain_loop_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'loglik')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'loglik_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok 8 cases', lines[-1]

    # the request check, rule by rule: the verdict, and a text for every broken rule
    got = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'req (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    assert {name: code for name, (code, _) in got.items()} == REQUESTS
    for name, (code, text) in got.items():
        assert (text == '') == (code == OK), name
        if code != OK:
            assert text == TEXT[name], (name, text)
    assert len({re.sub(r'-?\d[\w.+-]*|nan|inf', '#', t) for t in TEXT.values()}) == RULES

    # the pieces: at most LL_SEG entries each, in order, relative to the chunk; no entry, no piece
    assert 'seg : %d' % S in lines
    pieces = {int(ln.split()[1]): ln.split(' :')[1] for ln in lines if ln.startswith('pieces ')}
    assert set(pieces) == set(PIECES)
    for length, (want, first) in PIECES.items():
        pc, fi = pieces[length].split('|')
        assert pc.split() == want and [int(x) for x in fi.split()] == first, length

    # the chunks
    assert 'budget : %d 12' % (64 << 20) in lines
    chunks = {ln.split()[1]: [tuple(int(x) for x in c.split(':')) for c in ln.split(' :')[1].split()] for ln in lines if ln.startswith('chunks ')}
    assert set(chunks) == set(CHUNKS)
    for name, args in CHUNKS.items():
        assert chunks[name] == expected_chunks(*args), name
    assert chunks['none'] == [] and len(chunks['budget_below_one_request']) == 4 and chunks['exactly_one_chunk'] == [(0, 5)]
    assert chunks['one_entry_more'] == [(0, 3), (3, 5)] and chunks['budget_not_a_multiple'] == [(0, 4), (4, 5)]

    # the lanes that share an entry: 4 up to k = 128, 16 above (the measured border); the padded width of a row
    lanes = [int(x) for x in next(ln for ln in lines if ln.startswith('lanes :')).split(' :')[1].split()]
    assert len(lanes) == 1024 and lanes == [lc.lanes(k) for k in range(1, 1025)]
    assert lanes[127:129] == [4, 16] and set(lanes[:128]) == {4} and set(lanes[128:]) == {16}
    assert next(ln for ln in lines if ln.startswith('kp :')).split(' :')[1].split() == ['2', '2', '4', '4', '6', '6', '8', '8', '10']

    # the plain loop against the numpy restatement
    rec = {}
    for ln in lines:
        kind, _, rest = ln.partition(' ')
        if kind in ('case', 'W', 'T', 'rows', 'indptr', 'indices', 'values', 'll', 'mass', 'floored'):
            head, _, body = rest.partition(' :')
            rec.setdefault(int(head), {})[kind] = np.array(body.split(), dtype=np.float64)
    assert len(rec) == 8
    seen = {'empty_request': 0, 'explicit_zero': 0, 'floored': 0, 'minus_inf': 0, 'nan': 0, 'duplicate_rows': 0, 'real_values': 0}
    for cid, r in sorted(rec.items()):
        n, d, k, count = (int(x) for x in r['case'][:4])
        floor = r['case'][4]
        W, T = r['W'].reshape(n, k), r['T'].reshape(k, d)
        rows = r['rows'].astype(np.int64)
        A = sp.csr_matrix((r['values'], r['indices'].astype(np.int32), r['indptr'].astype(np.int64)), shape=(count, d))
        ll, mass, floored, p, bound = lc.reference(W, T, rows, A, floor)
        assert lc.floor_is_comparable(p, floor), cid
        assert np.array_equal(r['floored'], floored), cid
        finite = np.isfinite(ll)
        assert np.array_equal(np.isnan(r['ll']), np.isnan(ll)) and np.array_equal(r['ll'][~finite & ~np.isnan(ll)], ll[~finite & ~np.isnan(ll)])
        assert np.all(np.abs(r['ll'][finite] - ll[finite]) <= bound[finite]), cid
        assert np.all(np.abs(r['mass'] - mass) <= np.diff(A.indptr) * lc.U * mass), cid
        if np.all(A.data == np.floor(A.data)):
            assert np.array_equal(r['mass'], mass), cid
        seen['empty_request'] += bool((np.diff(A.indptr) == 0).any())
        seen['explicit_zero'] += bool((A.data == 0).any())
        seen['floored'] += bool(floored.any())
        seen['minus_inf'] += bool(np.isneginf(ll).any())
        seen['nan'] += bool(np.isnan(ll).any()) and not np.isnan(ll).all()
        seen['duplicate_rows'] += np.unique(rows).size < rows.size
        seen['real_values'] += bool((A.data != np.floor(A.data)).any())
    assert all(seen.values()), seen


def gpu_present():
    lib = _capi.load_library()
    h = ctypes.c_void_p()
    st = lib.rri_create(ctypes.byref(h), 4, 4, 2, 0, 0, 0, None)
    if st == 0:
        lib.rri_destroy(h)
    return st == 0


def test_the_entry_point_is_declared_bound_documented_and_refuses_before_any_device_call():
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    assert re.search(r'#define RRI_ABI_VERSION 1\b', text) and _capi.ABI_VERSION == 1          # an addition, not a new ABI
    proto = re.search(r'^rri_status rri_entries_loglik\(([^;]*)\);', text, flags=re.M)
    assert proto and re.sub(r'\s+', ' ', proto.group(1)) == (
        'rri_ctx* ctx, const int64_t* rows, int64_t count, const int64_t* indptr, const int32_t* indices, const double* values, '
        'double floor, double* ll_out, double* mass_out, int64_t* floored_out')
    assert re.search(r'7 = the launches of rri_entries_loglik', text)
    res, args = _capi.PROTOTYPES['rri_entries_loglik']
    I64P, I32P, DP = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    assert res is ctypes.c_int32
    assert args == [ctypes.c_void_p, I64P, ctypes.c_int64, I64P, I32P, DP, ctypes.c_double, DP, DP, I64P]
    for doc in ('INTEGRATION.md', 'README.md', 'DESIGN.md'):
        body = open(os.path.join(ROOT, doc)).read()
        assert 'rri_entries_loglik' in body and 'log_likelihood' in body and 'perplexity' in body, doc
    assert 'split_counts' in open(os.path.join(ROOT, 'README.md')).read()
    assert 'loglik_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()

    # without a handle there is nothing to score: the call is refused before any device call, whatever the request looks like
    lib = _capi.load_library()
    ptr, ind, val = (ctypes.c_int64 * 3)(0, 1, 2), (ctypes.c_int32 * 2)(0, 1), (ctypes.c_double * 2)(1.0, 2.0)
    ll, mass, fl = (ctypes.c_double * 2)(7.0, 7.0), (ctypes.c_double * 2)(7.0, 7.0), (ctypes.c_int64 * 2)(7, 7)

    def call(h=None, rows=None, count=2, ptr=ptr, ind=ind, val=val, floor=1e-12, ll=ll, mass=mass, fl=fl):
        return lib.rri_entries_loglik(h, rows, count, ptr, ind, val, floor, ll, mass, fl)
    assert call() == BAD and call(count=0) == BAD and call(count=-1) == BAD and call(ptr=None) == BAD and call(ll=None) == BAD
    assert call(floor=float('nan')) == BAD and call(val=(ctypes.c_double * 2)(-1.0, 2.0)) == BAD
    assert list(ll) == [7.0, 7.0] and list(mass) == [7.0, 7.0] and list(fl) == [7, 7]         # a refused call writes nothing
    if gpu_present():       # with a handle the request is checked before the factors are asked for and before any HIP call
        h = ctypes.c_void_p()
        assert lib.rri_create(ctypes.byref(h), 4, 4, 2, 0, 0, 0, None) == OK
        try:
            assert call(h, count=-1) == BAD and b'count -1 is negative' in lib.rri_last_error(h)
            assert call(h, floor=float('inf')) == BAD and call(h, ind=(ctypes.c_int32 * 2)(0, 4)) == BAD
            assert call(h, count=0) == OK and call(h, ptr=(ctypes.c_int64 * 3)(0, 0, 0)) == OK and list(ll) == [0.0, 0.0]
            assert call(h) == BAD and b'W and T must be set first' in lib.rri_last_error(h)
        finally:
            lib.rri_destroy(h)
    else:                   # no host route: the estimator's call needs the device like everything else
        from rri_nmf_amd import sklearn_interface as si
        E = si.NMF_TM_Estimator(4, 3, 2, W=np.ones((4, 2)), T=np.ones((2, 3)))
        with pytest.raises(_capi.RRIHipUnavailable):
            E.log_likelihood(sp.csr_matrix(np.ones((4, 3))), W=np.ones((4, 2)))


class FakeEngine(object):
    """stands in for RRIEngine behind NMF_TM_Estimator.log_likelihood: answers from the numpy restatement and keeps a log"""
    log = []

    def __init__(self, n, d, k, **kw):
        self.shape, self.kw, self.closed, self.calls, self.W, self.T = (n, d, k), kw, False, [], None, None
        FakeEngine.log.append(self)

    def set_W(self, W):
        assert W.shape == self.shape[::2]
        self.W = np.array(W)

    def set_T(self, T):
        assert T.shape == self.shape[:0:-1]
        self.T = np.array(T)

    def entries_loglik(self, rows, A, floor=0.0):
        assert not self.closed and sp.issparse(A) and self.W is not None and self.T is not None
        self.calls.append((rows, A, floor))
        return lc.reference(self.W, self.T, rows, A, floor)[:3]

    def close(self):
        self.closed = True


# Three documents over four words, two topics.  T's rows sum to 1; W's rows to 1, 2 (rescaled by Z = 2) and 0 (left as it is).
#   doc 0: W = (1, 0):          p = T[0] = (.5, .25, .25, 0);  counts (2, 0, 1, 1): 2 log .5 + log .25 + log floor, one floored
#   doc 1: W = (1, 1) / Z = 2:  p = (.25, .25, .25, .25);      counts (0, 4, 0, 0): 4 log .25
#   doc 2: W = (0, 0), Z = 0:   p = 0;                         counts (0, 0, 3, 0): 3 log floor, one floored
T_HAND = np.array([[0.5, 0.25, 0.25, 0.0], [0.0, 0.25, 0.25, 0.5]])
W_HAND = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 0.0]])
X_HAND = np.array([[2.0, 0.0, 1.0, 1.0], [0.0, 4.0, 0.0, 0.0], [0.0, 0.0, 3.0, 0.0]])
KEYS = {'per_document', 'tokens', 'floored', 'log_likelihood', 'per_token', 'perplexity', 'floor', 'documents'}


def test_log_likelihood_and_perplexity_of_a_hand_computed_corpus(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    monkeypatch.setattr(si, 'RRIEngine', FakeEngine)
    FakeEngine.log = []
    E = si.NMF_TM_Estimator(3, 4, 2, W=W_HAND, T=T_HAND, nmf_kwargs={'device': 3})
    lf = math.log(1e-12)
    per = [2 * math.log(0.5) + math.log(0.25) + lf, 4 * math.log(0.25), 3 * lf]
    for X in (sp.csr_matrix(X_HAND), X_HAND, sp.coo_matrix(X_HAND)):
        got = E.log_likelihood(X, W=W_HAND)
        eng = FakeEngine.log[-1]
        assert eng.closed and len(eng.calls) == 1 and eng.kw == {'dtype': np.float64, 'device': 3} and eng.shape == (3, 4, 2)
        assert eng.calls[0][0] is None and eng.calls[0][1].shape == (3, 4) and eng.calls[0][2] == 1e-12
        assert np.array_equal(eng.W, [[1.0, 0.0], [0.5, 0.5], [0.0, 0.0]]) and np.array_equal(eng.T, T_HAND)       # the Z_i scaling
        assert set(got) == KEYS and got['documents'] == 3 and got['floor'] == 1e-12
        assert got['per_document'] == pytest.approx(per, rel=1e-14) and got['tokens'].tolist() == [4.0, 4.0, 3.0]
        assert got['floored'].tolist() == [1, 0, 1] and got['floored'].dtype == np.int64
        assert got['log_likelihood'] == pytest.approx(sum(per), rel=1e-14)
        assert got['per_token'] == pytest.approx(sum(per) / 11, rel=1e-14)
        assert got['perplexity'] == pytest.approx(math.exp(-sum(per) / 11), rel=1e-13)
    assert np.array_equal(W_HAND[1], [1.0, 1.0])                                     # the caller's W stays as it is
    # another floor; floor = 0 leaves -inf and counts nothing as floored
    assert E.log_likelihood(X_HAND, W=W_HAND, floor=1e-3)['per_document'][2] == pytest.approx(3 * math.log(1e-3), rel=1e-14)
    zero = E.log_likelihood(X_HAND, W=W_HAND, floor=0.0)
    assert zero['per_document'][0] == -np.inf and zero['floored'].tolist() == [0, 0, 0] and zero['perplexity'] == np.inf
    # no token at all: per_token and perplexity are NaN
    none = E.log_likelihood(sp.csr_matrix((3, 4)), W=W_HAND)
    assert none['log_likelihood'] == 0.0 and np.isnan(none['per_token']) and np.isnan(none['perplexity']) and none['tokens'].tolist() == [0, 0, 0]
    # a sparsified T answers the same; a corpus of another number of documents
    E.sparsify()
    assert E.log_likelihood(X_HAND, W=W_HAND)['per_document'] == pytest.approx(per, rel=1e-14)
    E.densify()
    assert E.log_likelihood(np.vstack([X_HAND, X_HAND]), W=np.vstack([W_HAND, W_HAND]))['documents'] == 6

    # W=None folds in on X; W given runs no fold-in; perplexity(X, observed) folds in on observed and scores X
    folded = []

    def transform(Xnew):
        folded.append(Xnew)
        return W_HAND
    monkeypatch.setattr(E, 'transform', transform)
    a = E.log_likelihood(X_HAND)
    assert len(folded) == 1 and folded[0] is X_HAND
    b = E.log_likelihood(X_HAND, W=W_HAND)
    assert len(folded) == 1 and np.array_equal(a['per_document'], b['per_document'])
    observed = sp.csr_matrix(2.0 * X_HAND)
    ppl = E.perplexity(X_HAND, observed=observed, floor=1e-3)
    assert len(folded) == 2 and folded[1] is observed and isinstance(ppl, float)
    assert ppl == E.log_likelihood(X_HAND, W=W_HAND, floor=1e-3)['perplexity'] and FakeEngine.log[-2].calls[0][2] == 1e-3
    assert np.array_equal(FakeEngine.log[-2].calls[0][1].toarray(), X_HAND)          # scored: X, not observed
    assert E.perplexity(X_HAND) == a['perplexity'] and folded[2] is X_HAND
    # the refusals
    with pytest.raises(ValueError, match='columns'):
        E.log_likelihood(X_HAND[:, :3], W=W_HAND)
    with pytest.raises(ValueError, match='one row per document'):
        E.log_likelihood(X_HAND, W=W_HAND[:2])
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_TM_Estimator(3, 4, 2).log_likelihood(X_HAND, W=W_HAND)


def test_split_counts_thins_every_count_binomially():
    from rri_nmf_amd import sklearn_interface as si
    rng = np.random.RandomState(0)
    X = sp.csr_matrix(rng.poisson(0.7, size=(60, 40)).astype(np.float64))
    X.data[::9] = 0.0                                           # explicit zeros
    keep = (X.indptr.copy(), X.indices.copy(), X.data.copy())
    obs, held = si.split_counts(X, held_out=0.5, random_state=0)
    assert sp.isspmatrix_csr(obs) and sp.isspmatrix_csr(held) and obs.shape == held.shape == X.shape
    assert np.array_equal((obs + held).toarray(), X.toarray())
    assert obs.data.min() > 0 and held.data.min() > 0            # explicit zeros are dropped from both parts
    assert np.all(obs.data == np.floor(obs.data)) and np.all(held.data == np.floor(held.data))
    assert all(np.array_equal(x, y) for x, y in zip(keep, (X.indptr, X.indices, X.data)))
    # the seeds: the same split again, another one for another seed, a RandomState taken as it is
    obs2, held2 = si.split_counts(X, 0.5, 0)
    assert np.array_equal(held.toarray(), held2.toarray()) and np.array_equal(obs.toarray(), obs2.toarray())
    assert not np.array_equal(si.split_counts(X, 0.5, 1)[1].toarray(), held.toarray())
    assert np.array_equal(si.split_counts(X, 0.5, np.random.RandomState(0))[1].toarray(), held.toarray())
    # held = binomial(x, held_out) over the stored values, in storage order
    Xc = sp.csr_matrix(X)
    want = np.random.RandomState(0).binomial(Xc.data.astype(np.int64), 0.5)
    assert np.array_equal(sp.csr_matrix((want.astype(np.float64), Xc.indices, Xc.indptr), shape=X.shape).toarray(), held.toarray())
    # the share that is held out: 3 sigma of a binomial over all tokens
    N = X.sum()
    for share in (0.2, 0.5, 0.9):
        h = si.split_counts(X, share, 3)[1].sum()
        assert abs(h - share * N) <= 3 * math.sqrt(N * share * (1 - share)), share
    # dense and integer input
    D = X.toarray().astype(np.int64)
    od, hd = si.split_counts(D, 0.5, 0)
    assert sp.isspmatrix_csr(od) and sp.isspmatrix_csr(hd) and np.array_equal((od + hd).toarray(), D)
    assert 0 < hd.sum() < D.sum() and hd.dtype == od.dtype == np.int64
    # the refusals
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='held_out'):
            si.split_counts(X, bad)
    for bad in (np.array([[1.5, 0.0]]), np.array([[-1.0, 2.0]]), np.array([[np.nan, 1.0]]), np.array([[np.inf, 1.0]])):
        with pytest.raises(ValueError, match='counts'):
            si.split_counts(bad)
