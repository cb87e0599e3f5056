"""Co-document counts and topic coherence without a GPU: the request check, the membership table, the row chunks and the plain
counter of rri_nmf_amd/csrc/rri_cooc.hpp under sanitizers, the ABI surface and the refusals of the real library, and
NMF_TM_Estimator.top_words / coherence with a stand-in for the device handle.

tests/c/cooc_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once; what it prints -- the verdict and text of 28
requests, four membership tables, nine cuts and the counts of eight seeded corpora -- is compared with what is written here and
with numpy on the dense 0/1 form (tests/cooc_cases.py)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import cooc_cases as cc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD, UNSUPPORTED = 0, _capi.RRI_ERR_INVALID, _capi.RRI_ERR_UNSUPPORTED

REQUESTS = {'fine': OK, 'no_rows': OK, 'no_entries': OK, 'only_empty_slots': OK, 'same_words_in_two_groups': OK,
            'negative_rows': BAD, 'negative_cols': BAD, 'negative_groups': BAD, 'negative_group_size': BAD,
            'group_size_0': UNSUPPORTED, 'no_groups': UNSUPPORTED, 'group_size_32': OK, 'group_size_33': UNSUPPORTED,
            'groups_max_k': OK, 'groups_max_k_plus_1': UNSUPPORTED, 'indptr_null': BAD, 'words_null': BAD, 'indices_null': BAD,
            'indptr_not_from_zero': BAD, 'indptr_decreases': BAD, 'negative_nnz': BAD, 'column_n_cols': BAD, 'column_negative': BAD,
            'column_twice': BAD, 'columns_descend': BAD, 'word_n_cols': BAD, 'word_below_minus_one': BAD,
            'word_twice_in_a_group': BAD}
# requests that break the same rule at another place share the rule's text but for the place
TEXT = {'negative_rows': 'n_rows -1 is negative', 'negative_cols': 'n_cols -1 outside', 'negative_groups': 'n_groups -1 is negative',
        'negative_group_size': 'group_size -1 is negative', 'group_size_0': 'group_size 0 outside 1 .. 32',
        'no_groups': 'n_groups 0 outside 1 .. 1024', 'group_size_33': 'group_size 33 outside 1 .. 32',
        'groups_max_k_plus_1': 'n_groups 1025 outside 1 .. 1024', 'indptr_null': 'indptr is NULL', 'words_null': 'words is NULL',
        'indices_null': 'indices is NULL with 5 entries', 'indptr_not_from_zero': 'indptr does not span nnz',
        'indptr_decreases': 'indptr not monotone at row 1', 'negative_nnz': 'bad CSR arrays',
        'column_n_cols': 'column index out of range at 1', 'column_negative': 'column index out of range at 0',
        'column_twice': 'column indices of row 2 are not strictly increasing',
        'columns_descend': 'column indices of row 0 are not strictly increasing', 'word_n_cols': 'word 5 of group 0 is out of range',
        'word_below_minus_one': 'word -2 of group 0 is out of range', 'word_twice_in_a_group': 'word 0 stands twice in group 0'}
MEMB = {'mixed': ([0, 0, 1, 4, 5, 6, 6], ['0.1', '0.0', '1.1', '2.2', '2.0', '1.2']),
        'only_empty_slots': ([0, 0, 0, 0], []), 'one_column': ([0, 3], ['0.0', '1.0', '2.0']), 'slot_31': ([0, 0, 1], ['0.31'])}
BUDGET = 64 << 20
CUTS = {'none': (0, 50, 1 << 20), 'one_row': (1, 50, 1 << 20), 'budget_below_a_tile': (70, 1024, 1000),
        'exactly_one_chunk': (64, 2, 512), 'one_row_more': (65, 2, 512), 'not_whole_tiles': (100, 2, 600),
        'max_k': (16385, 1024, BUDGET), 'max_k_one_chunk': (16384, 1024, BUDGET), 'fifty_topics': (100000, 50, BUDGET)}


def expected_cut(n_rows, n_groups, budget):
    per = max(32, budget // (4 * n_groups) // 32 * 32)
    return per, [(r0, min(n_rows, r0 + per), -(-(min(n_rows, r0 + per) - r0) // 32) * 32) for r0 in range(0, n_rows, per)]


def test_request_check_membership_table_row_chunks_and_plain_counter_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'cooc')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'cooc_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok 8 corpora', lines[-1]

    # the request check, rule by rule: the verdict, and a text of its own for every broken rule
    got = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'req (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    assert {name: code for name, (code, _) in got.items()} == REQUESTS
    for name, (code, text) in got.items():
        assert (text == '') == (code == OK), name
        if code != OK:
            assert text.startswith(TEXT[name]), (name, text)
    assert len(set(TEXT.values())) == len(TEXT)

    # the membership table: ptr per column, then (group.slot) of every slot that names the column, groups ascending
    tables = {ln.split()[1]: ln.split(' :')[1] for ln in lines if ln.startswith('memb ')}
    assert set(tables) == set(MEMB)
    for name, (ptr, ent) in MEMB.items():
        p, e = tables[name].split('|')
        assert [int(x) for x in p.split()] == ptr and e.split() == ent, name

    # the row chunks: budget // (4 n_groups) rows in whole tiles of 32, at least one tile; the mask rows padded to whole tiles
    cuts = {ln.split()[1]: (int(ln.split()[2]), ln.split(' :')[1].split()) for ln in lines if ln.startswith('cut ')}
    assert set(cuts) == set(CUTS)
    for name, args in CUTS.items():
        per, chunks = expected_cut(*args)
        assert cuts[name][0] == per and [tuple(int(x) for x in c.split(':')) for c in cuts[name][1]] == chunks, name
    assert len(cuts['none'][1]) == 0 and len(cuts['budget_below_a_tile'][1]) == 3 and len(cuts['exactly_one_chunk'][1]) == 1
    assert len(cuts['one_row_more'][1]) == 2 and len(cuts['max_k'][1]) == 2 and len(cuts['max_k_one_chunk'][1]) == 1
    assert len(cuts['fifty_topics'][1]) == 1

    # the instantiation of the counting kernel: the smallest of 1, 2, 4, 9 pairs per lane that holds M (M + 1) / 2 pairs on 64 lanes
    ppt = [int(x) for x in next(ln for ln in lines if ln.startswith('ppt :')).split(' :')[1].split()]
    assert ppt == [min(c for c in (1, 2, 4, 9) if 64 * c >= M * (M + 1) // 2) for M in range(1, 33)]
    assert ppt[9:11] == [1, 2] and ppt[14:16] == [2, 4] and ppt[21:23] == [4, 9] and ppt[31] == 9       # borders at 10 | 11, 15 | 16, 22 | 23

    # the plain counter against numpy on the dense 0/1 form
    rec = {}
    for ln in lines:
        kind, _, rest = ln.partition(' ')
        if kind in ('corpus', 'indptr', 'indices', 'words', 'df', 'codf'):
            head, _, body = rest.partition(' :')
            rec.setdefault(int(head), {})[kind] = np.array(body.split(), dtype=np.int64)
    assert len(rec) == 8
    seen = {'empty_slot': 0, 'empty_group': 0, 'word_in_every_row': 0, 'word_in_no_row': 0, 'shared_word': 0, 'group_size_32': 0}
    for cid, r in sorted(rec.items()):
        n_rows, n_cols, g, M = r['corpus']
        A = sp.csr_matrix((np.ones(r['indices'].size), r['indices'], r['indptr']), shape=(n_rows, n_cols))
        words = r['words'].reshape(g, M)
        df, codf = cc.dense_counts(A.toarray(), words)
        assert np.array_equal(r['df'].reshape(g, M), df), cid
        assert np.array_equal(r['codf'].reshape(g, M, M), codf), cid
        assert np.array_equal(codf, codf.transpose(0, 2, 1))
        seen['empty_slot'] += bool((words < 0).any())
        seen['empty_group'] += bool((words < 0).all(axis=1).any())
        seen['word_in_every_row'] += bool((df[words >= 0] == n_rows).any())
        seen['word_in_no_row'] += bool((df[words >= 0] == 0).any())
        seen['shared_word'] += bool(np.unique(words[words >= 0]).size < (words >= 0).sum())
        seen['group_size_32'] += M == 32
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
    assert re.search(r'^#define RRI_MAX_COOC_WORDS 32$', text, flags=re.M) and _capi.RRI_MAX_COOC_WORDS == 32
    assert re.search(r'#define RRI_ABI_VERSION 1\b', text) and _capi.ABI_VERSION == 1          # an addition, not a new ABI
    assert re.search(r'^rri_status rri_cooccurrence_counts\(', text, flags=re.M)
    assert re.search(r'6 = the launches of rri_cooccurrence_counts', text)
    res, args = _capi.PROTOTYPES['rri_cooccurrence_counts']
    I64P, I32P = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    assert res is ctypes.c_int32
    assert args == [ctypes.c_void_p, I64P, I32P, ctypes.c_int64, ctypes.c_int64, I32P, ctypes.c_int32, ctypes.c_int32, I64P, I64P]
    for doc in ('INTEGRATION.md', 'README.md', 'DESIGN.md'):
        assert 'rri_cooccurrence_counts' in open(os.path.join(ROOT, doc)).read(), doc
    assert 'cooc_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()

    # the request is checked before the handle is looked at and before any HIP call: the verdicts need no device
    lib = _capi.load_library()
    ptr, ind = (ctypes.c_int64 * 3)(0, 1, 2), (ctypes.c_int32 * 2)(0, 1)
    words = (ctypes.c_int32 * 2050)(*([0, 1] * 1025))
    df, codf = (ctypes.c_int64 * 2050)(), (ctypes.c_int64 * 4100)()

    def call(h=None, ptr=ptr, ind=ind, n_rows=2, n_cols=2, words=words, g=1, M=2, df=df, codf=codf):
        return lib.rri_cooccurrence_counts(h, ptr, ind, n_rows, n_cols, words, g, M, df, codf)
    assert call() == BAD                                                    # a fine request and a NULL handle
    assert call(M=33) == UNSUPPORTED and call(M=0) == UNSUPPORTED
    assert call(g=_capi.RRI_MAX_K + 1, M=1) == UNSUPPORTED and call(g=0) == UNSUPPORTED
    assert call(g=_capi.RRI_MAX_K, M=2) == BAD and call(n_cols=40, M=32, words=(ctypes.c_int32 * 32)(*range(32))) == BAD    # inside the limits: the handle
    assert call(ptr=None) == BAD and call(ind=None) == BAD and call(words=None) == BAD
    assert call(n_rows=-1) == BAD and call(n_cols=-1) == BAD and call(g=-1) == BAD and call(M=-1) == BAD
    assert call(n_cols=1) == BAD                                            # column 1 and word 1 out of range
    assert call(words=(ctypes.c_int32 * 2)(1, 1)) == BAD                    # a word twice in one group
    assert call(ptr=(ctypes.c_int64 * 3)(0, 2, 2), ind=(ctypes.c_int32 * 2)(1, 0)) == BAD       # a row that descends
    if not gpu_present():       # no host route: the estimator's call needs the device like everything else
        from rri_nmf_amd import sklearn_interface as si
        E = si.NMF_TM_Estimator(4, 3, 2, W=np.ones((4, 2)), T=np.ones((2, 3)))
        with pytest.raises(_capi.RRIHipUnavailable):
            E.coherence(sp.csr_matrix(np.ones((4, 3))), n_words=2)


def test_top_words_orders_by_value_then_by_column_and_keeps_positive_entries_only():
    from rri_nmf_amd import sklearn_interface as si
    T = np.array([[0.1, 0.4, 0.0, 0.4, 0.1, 0.0],          # ties at 0.4 and at 0.1: the smaller column first
                  [0.0, 0.0, 1.0, 0.0, 0.0, 0.0],          # one positive entry
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],          # none
                  [0.2, -0.5, np.nan, 0.2, 0.2, 0.3]])     # a negative entry and a NaN do not qualify
    E = si.NMF_TM_Estimator(5, 6, 4, W=np.ones((5, 4)), T=T)
    want = np.array([[1, 3, 0, 4, -1, -1, -1], [2, -1, -1, -1, -1, -1, -1], [-1] * 7, [5, 0, 3, 4, -1, -1, -1]], dtype=np.int32)
    for n_words in (1, 2, 3, 4, 7):
        got = E.top_words(n_words)
        assert got.dtype == np.int32 and got.shape == (4, n_words) and np.array_equal(got, want[:, :n_words]), n_words
    assert E.top_words().shape == (4, 10) and np.array_equal(E.top_words()[:, :7], want) and np.all(E.top_words()[:, 6:] == -1)
    # a sparsified T answers the same, and stays sparse
    E.T = np.where(np.isnan(T), 0.0, T)
    dense = E.top_words(4)
    E.sparsify()
    assert sp.issparse(E.T) and np.array_equal(E.top_words(4), dense) and sp.issparse(E.T)
    with pytest.raises(ValueError, match='n_words'):
        E.top_words(0)
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_TM_Estimator(5, 6, 4).top_words()


class FakeEngine(object):
    """stands in for RRIEngine behind NMF_TM_Estimator.coherence: counts in numpy on the dense form and keeps a log"""
    log = []

    def __init__(self, n, d, k, **kw):
        self.shape, self.kw, self.closed, self.calls = (n, d, k), kw, False, []
        FakeEngine.log.append(self)

    def cooccurrence_counts(self, A, words):
        assert not self.closed and sp.issparse(A)
        self.calls.append((A, np.array(words)))
        return cc.dense_counts(A.toarray(), words)

    def close(self):
        self.closed = True


# Four documents over six words:  doc 0 = {0, 1, 3, 5}, doc 1 = {0, 1, 5}, doc 2 = {0, 2, 5}, doc 3 = {0, 5}.  N = 4.
#   D_0 = D_5 = 4, D_1 = 2, D_2 = D_3 = 1, D_4 = 0;  D_05 = 4 (= N), D_13 = 1, D_12 = D_32 = 0, D_04 = D_54 = 0.
# topic 0, words 1 3 2:   pairs (1,3): D_ab 1, D_a 2, D_b 1;  (1,2): 0, 2, 1;  (3,2): 0, 1, 1
#   npmi   (1,3): log(.25 / (.5 * .25)) / -log(.25) = log 2 / (2 log 2) = 1/2;  the other two -1:  (1/2 - 2) / 3 = -1/2
#   umass  log(2/2), log(1/2), log(1/1):  -log 2 / 3            pmi  log(2*4/2), log(1*4/2), log(1*4/1):  5 log 2 / 3
# topic 1, words 0 5 4 (T ties 0 | 5 by the smaller column):   (0,5): D_ab = N;  (0,4) and (5,4): D_b = 0
#   npmi   1, two pairs undefined        pmi  log(5*4/16) = log 1.25, two undefined
#   umass  (log(5/4) + 2 log(1/4)) / 3, none undefined (D_a = 4)
# topic 2, words 4 0 -1:  the one pair (4,0) has D_a = 0: undefined for every measure, the topic's figure NaN
# diversity: 8 non-empty slots, 6 distinct words.
DOCS = np.array([[1, 1, 0, 1, 0, 1], [1, 1, 0, 0, 0, 1], [1, 0, 1, 0, 0, 1], [1, 0, 0, 0, 0, 1]], dtype=np.float64)
TOPICS = np.array([[0.0, 0.5, 0.1, 0.4, 0.0, 0.0], [0.4, 0.0, 0.0, 0.0, 0.2, 0.4], [0.3, 0.0, 0.0, 0.0, 0.7, 0.0]])
L2 = math.log(2.0)
HAND = {'npmi': ([-0.5, 1.0, np.nan], [0, 2, 1]),
        'umass': ([-L2 / 3, (math.log(1.25) - 4 * L2) / 3, np.nan], [0, 0, 1]),
        'pmi': ([5 * L2 / 3, math.log(1.25), np.nan], [0, 2, 1])}


def test_coherence_of_a_hand_computed_corpus_for_every_measure(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    monkeypatch.setattr(si, 'RRIEngine', FakeEngine)
    FakeEngine.log = []
    E = si.NMF_TM_Estimator(4, 6, 3, W=np.ones((4, 3)), T=TOPICS, nmf_kwargs={'device': 3})
    assert E.top_words(3).tolist() == [[1, 3, 2], [0, 5, 4], [4, 0, -1]]
    for measure, (per, undefined) in HAND.items():
        for X in (sp.csr_matrix(DOCS), DOCS, sp.coo_matrix(DOCS)):
            got = E.coherence(X, n_words=3, measure=measure)
            eng = FakeEngine.log[-1]
            assert eng.closed and len(eng.calls) == 1 and eng.kw['device'] == 3 and eng.calls[0][0].shape == (4, 6)
            assert set(got) == {'measure', 'per_topic', 'mean', 'words', 'df', 'codf', 'documents', 'pairs_undefined', 'diversity'}
            assert got['measure'] == measure and got['documents'] == 4 and got['diversity'] == 0.75
            assert got['words'].tolist() == [[1, 3, 2], [0, 5, 4], [4, 0, -1]]
            assert got['df'].tolist() == [[2, 1, 1], [4, 4, 0], [0, 4, 0]]
            assert got['codf'][0].tolist() == [[2, 1, 0], [1, 1, 0], [0, 0, 1]] and got['codf'][1, 0, 1] == 4
            assert np.isnan(got['per_topic'][2]) and got['per_topic'][:2] == pytest.approx(per[:2], rel=1e-14, abs=1e-15)
            assert got['pairs_undefined'].tolist() == undefined
            assert got['mean'] == pytest.approx(np.mean(per[:2]), rel=1e-14)
            ref, undef = cc.measure_reference(measure, got['words'], got['df'], got['codf'], 4, 1.0)
            assert np.array_equal(undef, undefined) and got['per_topic'] == pytest.approx(ref, rel=1e-14, abs=1e-15, nan_ok=True)
    # eps: not used by npmi; umass and pmi take it as given, also 0 (a pair that never co-occurs is then -inf)
    assert E.coherence(DOCS, 3, 'npmi', eps=7.0)['per_topic'][0] == -0.5
    assert E.coherence(DOCS, 3, 'umass', eps=0.5)['per_topic'][0] == pytest.approx((math.log(1.5 / 2) + math.log(0.5 / 2) + math.log(0.5)) / 3, rel=1e-14)
    assert E.coherence(DOCS, 3, 'pmi', eps=0.0)['per_topic'][0] == -np.inf

    # words= overrides the top words: an empty slot in the middle leaves one pair, (1, 3); any number of groups
    got = E.coherence(DOCS, measure='npmi', words=[[1, -1, 3], [-1, -1, -1]])
    assert FakeEngine.log[-1].calls[0][1].tolist() == [[1, -1, 3], [-1, -1, -1]]
    assert got['per_topic'][0] == 0.5 and np.isnan(got['per_topic'][1]) and got['mean'] == 0.5
    assert got['pairs_undefined'].tolist() == [0, 0] and got['diversity'] == 1.0 and got['words'].dtype == np.int32
    assert got['df'].tolist() == [[2, 0, 1], [0, 0, 0]]
    none = E.coherence(DOCS, words=[[-1, -1]])
    assert np.isnan(none['mean']) and np.isnan(none['diversity']) and np.isnan(none['per_topic'][0])
    assert E.coherence(DOCS, words=[[0, 5], [5, 0]])['diversity'] == 0.5
    # a sparsified T, and a corpus that is not the training matrix (another number of documents)
    E.sparsify()
    assert E.coherence(np.vstack([DOCS, DOCS, DOCS[:1]]), 3)['documents'] == 9
    assert E.coherence(np.vstack([DOCS, DOCS]), 3)['per_topic'][:2] == pytest.approx([-0.5, 1.0], rel=1e-14)
    E.densify()
    # the refusals
    with pytest.raises(ValueError, match='measure'):
        E.coherence(DOCS, measure='c_v')
    with pytest.raises(ValueError, match='columns'):
        E.coherence(DOCS[:, :5])
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_TM_Estimator(4, 6, 3).coherence(DOCS)
