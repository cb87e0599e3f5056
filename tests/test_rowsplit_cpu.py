"""The split of a corpus by row, without a GPU: the quota, the refusals and the plain loop of rri_nmf_amd/csrc/rri_rowsplit.hpp under
sanitizers, the ABI surface of include/rri_corpus_rowsplit.h and the refusal of the real library that needs no device, the argument
checks of DeviceCorpus.split_rows, sklearn_interface.split_rows and NMF_RS_Estimator.ranking_score_new_users with stand-ins for the
device, and the host route of sklearn_interface.split_rows.

tests/c/rowsplit_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built once with the
host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once: it holds the plain loop against a full sort of
every row, a degenerate key, the nesting of the held sets and the agreement with split_entries_plain itself; what it prints is
compared with what is written here and with the numpy restatement (tests/rowsplit_cases.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import corpus_build_cases as cb
import derive_cases as dc
import rowsplit_cases as rc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('rowsplit') / 'rowsplit')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'rowsplit_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    out = res.stdout.strip().splitlines()
    assert out[-1] == 'ok 13 cases', out[-1]
    return out


def records(lines, kinds):
    rec = {}
    for ln in lines:
        kind, _, rest = ln.partition(' ')
        if kind in kinds:
            head, _, body = rest.partition(' :')
            rec.setdefault(int(head), {})[kind] = np.array(body.split(), dtype=np.float64)
    return rec


def matrix(r, name):
    n_rows, n_cols = (int(x) for x in r[name + 'shape'])
    return sp.csr_matrix((r[name + 'val'], r[name + 'idx'].astype(np.int32), r[name + 'ptr'].astype(np.int64)), shape=(n_rows, n_cols))


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same(A, B):
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(bits(A.data), bits(B.data)))


def test_the_constants_the_quota_at_its_edges_and_every_refusal_by_name(lines):
    assert 'consts : %d %d %d %d %d %d %d' % (rc.WAVE_MAX, rc.BLOCK_THREADS, rc.DIGIT_BITS, rc.BINS, rc.PASSES, rc.BOUND_NONE, rc.BOUND_ALL) in lines
    assert rc.BINS == 1 << rc.DIGIT_BITS == rc.BLOCK_THREADS and rc.PASSES * rc.DIGIT_BITS == 64
    assert 'classes : %d %d %d %d %d %d %d' % tuple(rc.row_class(L, h) for L, h in ((0, 0), (5, 0), (5, 5), (2, 1), (64, 63), (65, 1), (65, 65))) in lines
    assert [rc.row_class(L, h) for L, h in ((2, 1), (64, 63), (65, 1), (65, 65))] == [rc.CLASS_WAVE, rc.CLASS_WAVE, rc.CLASS_BLOCK, rc.CLASS_NONE]
    # the key of one entry: word 0 of block 0 of the counter (column, row low, row high, 0) under (seed low, seed high), above the column
    A = sp.csr_matrix(([1.0], ([0], [9])), shape=(1, 10))
    w0 = int(dc.philox(9, 7, 5, 0, 2, 3)[0])
    assert 'key : %d' % ((w0 << 32) | 9) in lines
    assert int(rc.keys(A, 0)[0]) == (int(dc.philox(9, 0, 0, 0, 0, 0)[0]) << 32) | 9
    # the quota against the restatement, line by line, and the values that matter written out
    got = {}
    for ln in lines:
        m = re.match(r'quota (\d+) (-?\d+) (\S+) (\d+) : (\d+)$', ln)
        if m:
            got[(int(m.group(1)), int(m.group(2)), float(m.group(3)), int(m.group(4)))] = int(m.group(5))
    assert len(got) == 3 * 3 * 2 + 12 * 5 * 3
    for (L, k, f, mo), h in got.items():
        want = rc.quota([L], n_held=k if k >= 1 else None, held_out=None if k >= 1 else f, min_observed=mo)[0]
        assert h == want and 0 <= h <= max(L - mo, 0), (L, k, f, mo, h)
    assert [got[(L, 1, 0.0, mo)] for L in (0, 1, 2) for mo in (0, 1, 5)] == [0, 0, 0, 1, 0, 0, 1, 1, 0]
    assert [got[(L, 3, 0.0, mo)] for L in (0, 1, 2) for mo in (0, 1, 5)] == [0, 0, 0, 1, 0, 0, 2, 1, 0]             # a count above the length
    assert [got[(L, -1, 1.0, 0)] for L in (0, 1, 2, 7, 1001)] == [0, 1, 2, 7, 1001]                                 # the whole row
    assert [got[(L, -1, 1.0, 1)] for L in (0, 1, 2, 7, 1001)] == [0, 0, 1, 6, 1000]
    assert [got[(L, -1, 0.5, 0)] for L in (1, 2, 3, 5, 7, 11)] == [1, 1, 2, 3, 4, 6]                                # half-way rounds up
    assert [got[(L, -1, 0.25, 0)] for L in (1, 2, 6, 10)] == [0, 1, 2, 3]
    assert [got[(L, -1, 0.1, 0)] for L in (4, 5, 10, 1000)] == [0, 1, 1, 100] and got[(10, -1, 0.2, 5)] == 2 and got[(6, -1, 1.0, 5)] == 1
    # every refusal, by the name of its case
    req = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'req (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    assert set(req) == set(rc.REQUEST_FINE) | set(rc.REQUEST_TEXT)
    for name in rc.REQUEST_FINE:
        assert req[name] == (rc.OK, ''), name
    for name, text in rc.REQUEST_TEXT.items():
        assert req[name] == (rc.INVALID, text), name
    kinds = {}
    for name, text in rc.REQUEST_TEXT.items():
        kinds.setdefault(re.sub(r'-?\d[\w.]*|-?nan', '#', text), []).append(name)
    assert all(len(v) >= 2 for v in kinds.values()) and len(kinds) == 6, kinds
    # what the program checked itself
    assert 'degenerate : 1' in lines
    nested = next(ln for ln in lines if ln.startswith('nested : '))
    assert int(nested.split()[2]) > 500                                         # pairs of quotas at which a row's held set grew
    agree = [int(x) for x in next(ln for ln in lines if ln.startswith('agree : ')).split()[2:]]
    assert agree[0] == sum(agree[1:]) and min(agree) >= 15, agree               # rows compared with split_entries_plain: m = 1, 2, more


def test_the_plain_loop_against_the_restatement(lines):
    rec = records(lines, ('rsplit',) + tuple(n + k for n in ('from', 'obs', 'held') for k in ('shape', 'ptr', 'idx', 'val')))
    assert len(rec) == 13
    seen = dict(count=0, fraction=0, min_observed_0=0, min_observed_5=0, whole_row=0, high_seed=0, no_rows=0, empty_rows=0, wave=0, block=0, negatives=0)
    for cid, r in sorted(rec.items()):
        n_held, fraction, min_observed, seed = int(r['rsplit'][0]), float(r['rsplit'][1]), int(r['rsplit'][2]), int(r['rsplit'][3])
        A, obs, held = matrix(r, 'from'), matrix(r, 'obs'), matrix(r, 'held')
        mode = dict(n_held=n_held) if n_held >= 1 else dict(held_out=fraction)
        want = rc.split_rows(A, min_observed=min_observed, seed=seed, **mode)
        assert same(obs, want[0]) and same(held, want[1]), cid
        total = sp.csr_matrix(obs + held)
        total.sort_indices()
        assert same(total, A) and obs.nnz + held.nnz == A.nnz and obs.multiply(held).nnz == 0, cid
        lengths = np.diff(A.indptr)
        h = rc.quota(lengths, min_observed=min_observed, **mode)
        assert np.array_equal(np.diff(held.indptr), h), cid
        classes = [rc.row_class(L, q) for L, q in zip(lengths, h)]
        seen['count'] += n_held >= 1
        seen['fraction'] += n_held == -1
        seen['min_observed_0'] += min_observed == 0
        seen['min_observed_5'] += min_observed == 5
        seen['whole_row'] += A.nnz > 0 and held.nnz == A.nnz
        seen['high_seed'] += seed >> 32 != 0
        seen['no_rows'] += A.shape[0] == 0
        seen['empty_rows'] += A.shape[0] > 0 and A.nnz == 0
        seen['wave'] += rc.CLASS_WAVE in classes
        seen['block'] += rc.CLASS_BLOCK in classes
        seen['negatives'] += bool((A.data < 0).any())
    assert all(seen.values()), seen
    # the two properties, from the restatement as well: nested in the quota, and the held set of split_entries where the counts agree
    A = matrix(rec[9], 'from')
    for seed in (3, (7 << 32) | 1):
        h1, h2 = rc.split_rows(A, n_held=1, min_observed=0, seed=seed)[1], rc.split_rows(A, n_held=2, min_observed=0, seed=seed)[1]
        assert h1.multiply(h2).nnz == h1.nnz and h2.nnz > h1.nnz
        by_entry = cb.split_entries(A, dc.threshold(0.01), seed)[1]
        m = np.diff(by_entry.indptr)
        for k in np.unique(m[m > 0]):
            by_row = rc.split_rows(A, n_held=int(k), min_observed=0, seed=seed)[1]
            for r in np.flatnonzero(m == k):
                assert np.array_equal(by_row[r].indices, by_entry[r].indices), (seed, k, r)
    # a degenerate key: the lowest columns
    held = rc.split_rows(A, n_held=3, min_observed=1, key=(np.uint64(5) << np.uint64(32)) | A.indices.astype(np.uint64))[1]
    for r in range(A.shape[0]):
        assert np.array_equal(held[r].indices, A[r].indices[:min(3, max(A[r].nnz - 1, 0))])


def test_the_corpora_of_the_gpu_tests_and_the_share_of_rows_that_agree_with_split_entries():
    A = rc.edge_corpus()
    lengths = np.diff(A.indptr)
    assert A.shape == (39, rc.EDGE_D) and sorted(set(lengths.tolist())) == rc.EDGE_LENGTHS and all((lengths == L).sum() == 3 for L in rc.EDGE_LENGTHS)
    assert len(dc.pieces([0, 2500])) == 3 and len(dc.pieces([0, dc.PIECE])) == 1 and len(dc.pieces([0, dc.PIECE + 1])) == 2
    B = rc.random_corpus()
    assert (np.diff(B.indptr) == 0).sum() >= 2 and (B.data < 0).any()
    # what tests/test_rowsplit_gpu.py asserts on the device: with held_out 0.1 and seed 12345 at least a tenth of the rows hold 1, 2 or
    # 3 entries out under split_entries and have that number as their quota (min_observed = 1)
    share = agreeing_rows(B, 0.1, 12345)[1]
    print('rows of the random corpus that qualify for some m in 1..3: %.3f' % share)
    assert share >= 0.1


def agreeing_rows(B, held_out, seed):
    """(m per row from split_entries where the row qualifies for the comparison with n_held = m in 1..3, else 0; their share)"""
    by_entry = cb.split_entries(B, dc.threshold(held_out), seed)[1]
    m = np.diff(by_entry.indptr)
    ok = np.zeros(B.shape[0], dtype=np.int64)
    for k in (1, 2, 3):
        q = rc.quota(np.diff(B.indptr), n_held=k, min_observed=1)
        ok[(m == k) & (q == k)] = k
    return ok, float((ok > 0).mean())


PROTOS = {
    'rri_corpus_split_rows': 'rri_ctx* ctx, const rri_corpus* src, int64_t n_held, double fraction, int64_t min_observed, uint64_t seed, '
                             'rri_corpus** observed, rri_corpus** held',
}
CTYPES = {'rri_ctx*': ctypes.c_void_p, 'const rri_corpus*': ctypes.c_void_p, 'rri_corpus**': ctypes.POINTER(ctypes.c_void_p),
          'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'double': ctypes.c_double}


def test_the_new_header_is_plain_c_bound_exported_documented_and_refuses_without_a_handle():
    text = open(os.path.join(ROOT, 'include', 'rri_corpus_rowsplit.h')).read()
    assert '#include "rri_hip.h"' in text and _capi.ABI_VERSION == 1
    assert re.search(r'#define RRI_ABI_VERSION 1\b', open(os.path.join(ROOT, 'include', 'rri_hip.h')).read())      # an addition, not a new ABI
    declared = re.findall(r'^rri_status (rri_\w+)\(', text, flags=re.M)
    assert sorted(declared) == sorted(PROTOS) == sorted(_capi.CORPUS_ROWSPLIT_PROTOTYPES)
    others = (_capi.PROTOTYPES, _capi.CORPUS_OPS_PROTOTYPES, _capi.CORPUS_BUILD_PROTOTYPES, _capi.CORPUS_FIT_PROTOTYPES, _capi.CORPUS_RANK_PROTOTYPES,
              _capi.FOLD_PROTOTYPES)
    assert not any(set(_capi.CORPUS_ROWSPLIT_PROTOTYPES) & set(t) for t in others)
    for name, want in PROTOS.items():
        proto = re.search(r'^rri_status %s\(([^;]*)\);' % name, text, flags=re.M)
        assert proto and re.sub(r'\s+', ' ', proto.group(1)) == want, name
        res, args = _capi.CORPUS_ROWSPLIT_PROTOTYPES[name]
        assert res is ctypes.c_int32 and args == [CTYPES[a.rsplit(' ', 1)[0]] for a in want.split(', ')], name
    # the header states the contract
    for phrase in ('(word0 << 32)', 'floor(fraction * L + 0.5)', 'min(want, max(L - min_observed, 0))', 'n_held == -1', 'outputs are NULL',
                   'exactly h', 'inside its held set for h + 1', 'ingest_ms'):
        assert phrase in text, phrase
    cc_ = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    assert cc_, 'no host C compiler'
    subprocess.run([cc_, '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c', '-I' + os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'include', 'rri_corpus_rowsplit.h')], check=True)
    lib = _capi.load_library()
    for name, (res, args) in _capi.CORPUS_ROWSPLIT_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args, name
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        body = open(os.path.join(ROOT, doc)).read()
        assert all(name in body for name in PROTOS) and 'rri_corpus_rowsplit.h' in body, doc
    readme, design = open(os.path.join(ROOT, 'README.md')).read(), open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert '4.19' in design and 'k_rowsplit_select_block' in design and 'split_rows(n_held=1)' in readme and 'ranking_score_new_users' in readme
    assert 'rowsplit_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()
    assert 'r32_rowsplit_probe.jsonl' in open(os.path.join(ROOT, 'profiles', 'README.md')).read()
    assert 'rri_corpus_rowsplit.h' in open(os.path.join(ROOT, 'rri_nmf_amd', 'build.py')).read()
    hip = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_hip.hip')).read()
    assert '#include "rri_corpus_rowsplit.h"' in hip and '#include "rri_rowsplit_kernels.hpp"' in hip
    # the kernels of the split by entry are not edited: the new pair stands beside them
    kernels = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_rowsplit_kernels.hpp')).read()
    assert all('void %s(' % k in kernels for k in ('k_rowsplit_select_wave', 'k_rowsplit_select_block', 'k_rowsplit_count', 'k_rowsplit_write'))
    assert 'asm' not in kernels
    # a NULL handle: RRI_ERR_INVALID without a device, and nothing is written or counted
    out, out2 = ctypes.c_void_p(7), ctypes.c_void_p(9)
    assert lib.rri_corpus_split_rows(None, None, 1, 0.0, 1, 0, ctypes.byref(out), ctypes.byref(out2)) == _capi.RRI_ERR_INVALID
    assert (out.value, out2.value) == (7, 9)
    corpora, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.rri_corpus_memory(ctypes.byref(corpora), ctypes.byref(nbytes)) == 0 and (corpora.value, nbytes.value) == (0, 0)


# ---- the Python layers, with stand-ins for the device ------------------------------------------------------------------------------------
class FakeLib(object):
    def __init__(self):
        self.calls = []

    def rri_corpus_split_rows(self, h, src, n_held, fraction, min_observed, seed, observed, held):
        self.calls.append(dict(n_held=n_held, fraction=fraction, min_observed=min_observed, seed=seed))
        return 0


class FakeEngine(object):
    _h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def _check(self, st):
        assert st == 0


def patched(monkeypatch):
    from rri_nmf_amd.engine import DeviceCorpus
    lib = FakeLib()
    monkeypatch.setattr(_capi, 'load_library', lambda path=None: lib)
    monkeypatch.setattr(DeviceCorpus, '_handle', lambda self: FakeEngine())
    monkeypatch.setattr(DeviceCorpus, '_read_info', lambda self: None)
    monkeypatch.setattr(DeviceCorpus, 'close', lambda self: None)
    monkeypatch.setattr(DeviceCorpus, '_adopt', classmethod(lambda cls, c, device, lib_: ('corpus', device)))
    c = DeviceCorpus.__new__(DeviceCorpus)
    c._c, c._lib, c.device, c.shape = ctypes.c_void_p(1), lib, 3, (6, 4)
    return DeviceCorpus, lib, c


BAD_REQUESTS = (dict(), dict(n_held=1, held_out=0.5), dict(n_held=0), dict(n_held=-1), dict(held_out=0.0), dict(held_out=-0.5), dict(held_out=1.5),
                dict(held_out=float('nan')), dict(n_held=1, min_observed=-1), dict(held_out=0.5, min_observed=-2))
BAD_TYPES = (dict(n_held=1.5), dict(n_held=True), dict(held_out='half'), dict(n_held=1, min_observed=0.5))


def test_split_rows_checks_its_arguments_before_any_device_call_and_hands_the_request_over(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    D, lib, c = patched(monkeypatch)
    assert c.split_rows(n_held=1) == (('corpus', 3), ('corpus', 3)) and lib.calls[-1] == dict(n_held=1, fraction=0.0, min_observed=1, seed=0)
    c.split_rows(held_out=0.2, min_observed=0, random_state=(5 << 32) | 7)
    assert lib.calls[-1] == dict(n_held=-1, fraction=0.2, min_observed=0, seed=(5 << 32) | 7)
    c.split_rows(n_held=np.int64(3), min_observed=np.int32(5))
    assert lib.calls[-1] == dict(n_held=3, fraction=0.0, min_observed=5, seed=0)
    c.split_rows(held_out=1, random_state=np.random.RandomState(3))
    lo, hi = (int(v) for v in np.random.RandomState(3).randint(0, 1 << 32, size=2, dtype=np.uint64))
    assert lib.calls[-1] == dict(n_held=-1, fraction=1.0, min_observed=1, seed=lo | (hi << 32))
    made = len(lib.calls)
    for bad in BAD_REQUESTS:
        with pytest.raises(ValueError, match='n_held|held_out|min_observed'):
            c.split_rows(**bad)
    for bad in BAD_TYPES:
        with pytest.raises(TypeError):
            c.split_rows(**bad)
    with pytest.raises(TypeError):
        c.split_rows(n_held=1, random_state=1.5)
    assert len(lib.calls) == made
    c._c = ctypes.c_void_p()
    with pytest.raises(ValueError, match='closed'):
        c.split_rows(n_held=1)
    # the quota of the Python side is the restatement's
    L = np.array([0, 1, 2, 3, 5, 7, 10, 11, 64, 1001])
    for kw in (dict(n_held=1), dict(n_held=3, min_observed=0), dict(held_out=0.5, min_observed=0), dict(held_out=0.2, min_observed=5), dict(held_out=1.0)):
        assert np.array_equal(D._split_rows_quota(L, *D._split_rows_request(kw.get('n_held'), kw.get('held_out'), kw.get('min_observed', 1))), rc.quota(L, **kw))

    # the public function dispatches a corpus and refuses the same requests on the host route
    class Corpus(D):
        def __init__(self):
            self.calls = []

        def split_rows(self, n_held=None, held_out=None, min_observed=1, random_state=0):
            self.calls.append((n_held, held_out, min_observed, random_state))
            return 'observed', 'held'
    k = Corpus()
    assert si.split_rows(k, n_held=2) == ('observed', 'held') and k.calls == [(2, None, 1, 0)]
    assert si.split_rows(k, held_out=0.25, min_observed=3, random_state=9) == ('observed', 'held') and k.calls[-1] == (None, 0.25, 3, 9)
    X = sp.random(20, 15, density=0.3, format='csr', random_state=1)
    for bad in BAD_REQUESTS:
        with pytest.raises(ValueError, match='n_held|held_out|min_observed'):
            si.split_rows(X, **bad)
    for bad in BAD_TYPES:
        with pytest.raises(TypeError):
            si.split_rows(X, **bad)
    doc = si.split_rows.__doc__
    assert 'DeviceCorpus' in doc and 'different split' in doc and 'equally valid' in doc and 'different generators' in doc


def test_the_host_route_gives_every_row_its_quota(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    rng = np.random.RandomState(5)
    X = sp.random(80, 60, density=0.25, format='csr', random_state=rng, data_rvs=lambda m: rng.randn(m))
    X.data[:7] = 0.0
    X = sp.vstack([X, sp.csr_matrix((2, 60)), sp.csr_matrix(np.ones((1, 60)))]).tocsr()
    A = sp.csr_matrix(X, copy=True)
    A.eliminate_zeros()
    A.sort_indices()
    lengths = np.diff(A.indptr)
    assert (lengths == 0).any() and (lengths == 60).any()
    for kw in (dict(n_held=1), dict(n_held=2, min_observed=0), dict(n_held=100, min_observed=5), dict(held_out=0.2), dict(held_out=0.5, min_observed=0),
               dict(held_out=1.0), dict(held_out=1.0, min_observed=0)):
        for seed in (0, 11):
            observed, held = si.split_rows(X, random_state=seed, **kw)
            assert np.array_equal(np.diff(held.indptr), rc.quota(lengths, **kw)), kw                   # exact counts per row
            total = sp.csr_matrix(observed + held)
            total.sort_indices()
            assert same(total, A) and observed.multiply(held).nnz == 0 and observed.nnz + held.nnz == A.nnz        # disjoint; their union is A
            assert (observed.has_canonical_format or observed.nnz == 0) and (held.has_canonical_format or held.nnz == 0)
            for part in (observed, held):                                                               # values preserved, bit for bit
                i, j = part.nonzero()
                assert part.nnz == 0 or np.array_equal(bits(part.data), bits(np.asarray(A[i, j]).ravel()))
            again = si.split_rows(X, random_state=seed, **kw)
            assert same(again[0], observed) and same(again[1], held)
        other = si.split_rows(X, random_state=12, **kw)[1]
        if 0 < held.nnz < A.nnz:
            assert not same(other, held)
    assert si.split_rows(X, held_out=1.0, min_observed=0)[0].nnz == 0
    # leave-one-out is uniform over a row's entries: 6000 rows of 4, each position held about a quarter of the time
    Y = sp.csr_matrix(np.ones((6000, 4)))
    held = si.split_rows(Y, n_held=1, random_state=3)[1]
    counts = np.bincount(held.indices, minlength=4)
    assert counts.sum() == 6000 and np.all(np.abs(counts - 1500) <= 5 * np.sqrt(6000 * 0.25 * 0.75)), counts


def test_ranking_score_new_users_is_the_composition_and_refuses_before_any_device_call(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    from rri_nmf_amd.engine import DeviceCorpus as Real
    log = []

    class Corpus(object):
        _split_rows_request = staticmethod(Real._split_rows_request)

        def __init__(self, shape, nnz, name):
            self.shape, self.nnz, self.name, self.closed = shape, nnz, name, False

        def split_rows(self, **kw):
            log.append(('split', self.name, kw))
            self.parts = Corpus(self.shape, 14, 'observed'), Corpus(self.shape, 6, 'held')
            return self.parts

        def close(self):
            self.closed = True
    monkeypatch.setattr(si, 'DeviceCorpus', Corpus)
    E = si.NMF_RS_Estimator(3, 4, 2, random_state=7, W=np.ones((3, 2)), T=np.ones((2, 4)))
    W_new = np.full((5, 2), 0.5)
    monkeypatch.setattr(si.NMF_RS_Estimator, 'transform_corpus', lambda self, c: log.append(('fold', c.name)) or W_new)
    monkeypatch.setattr(si.NMF_RS_Estimator, 'ranking_score_corpus',
                        lambda self, targets, n_items=10, exclude=None, relevant_from=None, W=None:
                        log.append(('rank', targets.name, n_items, exclude.name, relevant_from, W)) or {'users': 5, 'hit_rate': 0.5})
    new = si.DeviceCorpus((5, 4), 20, 'new')
    got = E.ranking_score_new_users(new)
    assert got == {'users': 5, 'hit_rate': 0.5, 'observed_entries': 14, 'held_entries': 6}
    assert log[0] == ('split', 'new', dict(n_held=None, held_out=0.2, min_observed=1, random_state=7))           # the defaults: a fifth, the estimator's seed
    assert log[1] == ('fold', 'observed') and log[2][:5] == ('rank', 'held', 10, 'observed', None) and log[2][5] is W_new and len(log) == 3
    assert all(p.closed for p in new.parts) and not new.closed
    del log[:]
    E.ranking_score_new_users(new, n_items=3, n_held=1, min_observed=2, relevant_from=4.0, random_state=11)
    assert log[0] == ('split', 'new', dict(n_held=1, held_out=None, min_observed=2, random_state=11)) and log[2][:5] == ('rank', 'held', 3, 'observed', 4.0)
    del log[:]
    with pytest.raises(TypeError, match='takes a DeviceCorpus, not csr_matrix'):
        E.ranking_score_new_users(sp.csr_matrix((5, 4)))
    for bad in (dict(n_held=1, held_out=0.5), dict(n_held=0), dict(held_out=1.5), dict(held_out=float('nan')), dict(min_observed=-1), dict(n_items=0)):
        with pytest.raises(ValueError, match='n_held|held_out|min_observed|n_items'):
            E.ranking_score_new_users(new, **bad)
    with pytest.raises(TypeError):
        E.ranking_score_new_users(new, n_held=2.5)
    with pytest.raises(ValueError, match='the corpus has 3 columns, the estimator 4'):
        E.ranking_score_new_users(si.DeviceCorpus((5, 3), 20, 'narrow'))
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_RS_Estimator(3, 4, 2).ranking_score_new_users(new)
    assert log == []
