"""Ranks of entries without a GPU: the predicates, the piece cutter and the request validation of rri_nmf_amd/csrc/rri_rank.hpp
under sanitizers, the ABI surface, and NMF_RS_Estimator.rank / ranking_score with stand-ins for the solver and the device handle.

tests/c/rank_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once: 45 seeded rows of scores (three values only; mostly
distinct; NaN, both infinities and ties) of lengths 1, 5, 64, 65, 300 with an exclusion segment and random targets, targets among
the excluded columns, or every column as a target.  What it prints is compared with the restatement of tests/rank_cases.py."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import rank_cases as rc
import topn_cases as tc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = _capi.RRI_ERR_INVALID

REQUESTS = {'all_rows': 0, 'listed_rows_with_duplicates': 0, 'no_rows': 0, 'no_targets': 0, 'targets_and_exclusion': 0,
            'empty_exclusion': 0, 'negative_count': BAD, 'more_rows_than_W_has': BAD, 'row_n': BAD, 'row_negative': BAD,
            'tgt_indptr_null': BAD, 'tgt_indptr_not_from_zero': BAD, 'tgt_indptr_decreases': BAD, 'tgt_indices_null': BAD,
            'target_d': BAD, 'target_negative': BAD, 'target_twice': BAD, 'targets_descend': BAD, 'excl_indptr_decreases': BAD,
            'excl_indices_null': BAD, 'excluded_column_d': BAD, 'excluded_columns_descend': BAD}


def as_double(bits):
    return struct.unpack('<d', struct.pack('<Q', int(bits, 16)))[0]


def expected_pieces(counts):
    out = []
    t = 0
    for q, c in enumerate(counts):
        sizes = [64] * (c // 64) + ([c % 64] if c % 64 or c == 0 else [])
        for n, s in enumerate(sizes):
            out.append((q, t, s, int(n == 0)))
            t += s
    return out


def test_rank_count_pieces_and_request_validation_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'rank')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'rank_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok 45 streams', lines[-1]

    rec = {}
    for ln in lines:
        kind, _, rest = ln.partition(' ')
        if kind in ('stream', 'excl', 'tgt', 'rank', 'elig'):
            head, body = rest.split(' :')
            rec.setdefault(int(head.split()[0]), {})[kind] = (head.split()[1:], body.split())
    assert len(rec) == 45
    seen = {'ties': 0, 'nan_inf': 0, 'excluded_target': 0, 'not_eligible': 0, 'clipped': 0}
    for sid, r in sorted(rec.items()):
        (length, lo, hi), sbits = r['stream']
        s = np.array([as_double(b) for b in sbits])
        lo, hi = as_double(lo), as_double(hi)
        d = int(length)
        assert s.size == d
        excl = np.array(r['excl'][1], dtype=np.int64)
        tgt = np.array(r['tgt'][1], dtype=np.int64)
        mask = np.zeros((1, d), dtype=bool)
        mask[0, excl] = True
        targets = sp.csr_matrix((np.ones(tgt.size), tgt, [0, tgt.size]), shape=(1, d))
        want = rc.ranks_from_scores(s[None, :], targets, mask, (lo, hi))
        got_rank = np.array([int(p.split(':')[0]) for p in r['rank'][1]], dtype=np.int64)
        got_val = np.array([as_double(p.split(':')[1]) for p in r['rank'][1]])
        assert np.array_equal(want.indices, tgt)
        assert np.array_equal(got_rank, want.rank), (sid, got_rank, want.rank)
        assert np.array_equal(got_val, want.val, equal_nan=True), sid
        assert int(r['elig'][1][0]) == want.eligible[0], sid
        seen['ties'] += d == 300 and np.unique(s).size <= 3
        seen['nan_inf'] += bool(np.isnan(s).any() and np.isinf(s).any())
        seen['excluded_target'] += bool(mask[0, tgt].any())
        seen['not_eligible'] += bool((got_rank < 0).any())
        seen['clipped'] += bool(np.any(got_val[got_rank >= 0] != s[tgt][got_rank >= 0]))
    assert all(seen.values()), seen

    cuts = {ln.split(' :')[0][4:]: ln.split(' :')[1].split() for ln in lines if ln.startswith('cut ')}
    for name, counts in (('none', []), ('empty_requests', [0, 0, 3, 0]), ('borders', [1, 63, 64, 65, 128, 129, 0, 257])):
        assert [tuple(int(x) for x in p.split(':')) for p in cuts[name]] == expected_pieces(counts), name
    assert len(cuts['borders']) == 1 + 1 + 1 + 2 + 2 + 3 + 1 + 5

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
    assert re.search(r'#define RRI_ABI_VERSION 1\b', text) and _capi.ABI_VERSION == 1          # an addition, not a new ABI
    assert re.search(r'^rri_status rri_rank_entries\(', text, flags=re.M)
    res, args = _capi.PROTOTYPES['rri_rank_entries']
    I64P, I32P, DP = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    assert res is ctypes.c_int32
    assert args == [ctypes.c_void_p, I64P, ctypes.c_int64, I64P, I32P, I64P, I32P, ctypes.c_double, ctypes.c_double, I32P, DP, I32P]
    lib = _capi.load_library()
    ptr, ind = (ctypes.c_int64 * 3)(0, 1, 2), (ctypes.c_int32 * 2)(0, 1)
    rank, val, elig = (ctypes.c_int32 * 2)(), (ctypes.c_double * 2)(), (ctypes.c_int32 * 2)()
    assert lib.rri_rank_entries(None, None, 2, ptr, ind, None, None, float('nan'), float('nan'), rank, val, elig) == _capi.RRI_ERR_INVALID
    for doc in ('INTEGRATION.md', 'README.md', 'DESIGN.md'):
        assert 'rri_rank_entries' in open(os.path.join(ROOT, doc)).read(), doc
    if not gpu_present():       # no host route: the estimator's calls need the device like everything else
        from rri_nmf_amd import sklearn_interface as si
        E = si.NMF_RS_Estimator(4, 3, 2, W=np.ones((4, 2)), T=np.ones((2, 3)))
        with pytest.raises(_capi.RRIHipUnavailable):
            E.rank(np.array([[0, 1]]), exclude_seen=False)
        with pytest.raises(_capi.RRIHipUnavailable):
            E.ranking_score(np.array([[0, 1]]), exclude_seen=False)


class FakeEngine(object):
    """stands in for RRIEngine behind NMF_RS_Estimator.rank: answers from the restatement and keeps a log"""
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

    def rank_entries(self, rows, targets, exclude=None, clip=(None, None)):
        assert not self.closed
        self.calls.append((np.array(rows), targets, exclude, clip))
        return rc.rank_reference(self.W, self.T, rows, targets, exclude, clip)

    def close(self):
        self.closed = True


def reference_answers(E, ij, exclude_seen):
    """(rank, eligible) per given pair from the restatement on the estimator's factors, all users at once"""
    n, d = E.W.shape[0], E.T.shape[1]
    A = sp.csr_matrix((np.ones(len(ij)), (ij[:, 0], ij[:, 1])), shape=(n, d))
    ref = rc.rank_reference(E.W, E.T, None, A, E.seen_ if exclude_seen else None)
    dense = np.full((n, d), -7, dtype=np.int64)
    dense[np.repeat(np.arange(n), np.diff(ref.indptr)), ref.indices] = ref.rank
    return dense[ij[:, 0], ij[:, 1]].astype(np.int32), ref.eligible[ij[:, 0]]


def test_rank_and_ranking_score_plumbing_with_stand_ins(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    n, d, k = 23, 11, 3
    rng = np.random.RandomState(5)

    def fake_nmf(X, kk, **kw):
        r = np.random.RandomState(kw.get('random_state', 0))
        return {'W': r.rand(n, kk), 'T': r.rand(kk, d), 'obj_history': []}
    monkeypatch.setattr(si._nmf_module, 'nmf', fake_nmf)
    monkeypatch.setattr(si, 'RRIEngine', FakeEngine)
    FakeEngine.log = []

    seen = rng.rand(n, d) < 0.3
    seen[4] = False
    ij = np.column_stack(np.nonzero(seen))
    y = rng.randint(1, 6, size=len(ij)).astype(np.float64)
    E = si.NMF_RS_Estimator(n, d, k, nmf_kwargs={'device': 3}).fit(ij, y)
    held = (rng.rand(n, d) < 0.25) & ~seen
    held[7] = False                                               # a user without a held-out pair
    test = np.column_stack(np.nonzero(held))
    in_seen = ij[[0, 5]]                                          # two pairs that were given to fit
    pairs = np.vstack([test[rng.permutation(len(test))], test[:4], in_seen])      # any order, four pairs twice
    vals = rng.randint(1, 6, size=len(pairs)).astype(np.float64)

    for exclude_seen in (True, False):
        rank, elig = E.rank(pairs, exclude_seen=exclude_seen)
        eng = FakeEngine.log[-1]
        assert eng.shape == (n, d, k) and eng.kw == dict(dtype=np.float64, weighted=False, device=3) and eng.closed
        assert len(eng.calls) == 1 and eng.calls[0][3] == (E.min_rating, E.max_rating)
        assert (eng.calls[0][2] is None) == (not exclude_seen)
        want_rank, want_elig = reference_answers(E, pairs, exclude_seen)
        assert rank.dtype == np.int32 and elig.dtype == np.int32 and rank.shape == elig.shape == (len(pairs),)
        assert np.array_equal(rank, want_rank) and np.array_equal(elig, want_elig)
        # a pair of seen_ is not taken out of the exclusion silently
        assert np.all(rank[-2:] == -1) == exclude_seen and np.all(rank[:-2] >= 0)
        assert np.array_equal(rank[-6:-2], rank[[np.flatnonzero((pairs[:-6] == p).all(1))[0] for p in test[:4]]])

        # chunks of at most _RECOMMEND_CHUNK users, one handle for all of them, only users that have a pair
        monkeypatch.setattr(si, '_RECOMMEND_CHUNK', 7)
        rank7, elig7 = E.rank(pairs, exclude_seen=exclude_seen)
        eng = FakeEngine.log[-1]
        users = np.unique(pairs[:, 0])
        assert 7 not in users and [c[0].size for c in eng.calls] == [7] * (users.size // 7) + [users.size % 7] and eng.closed
        assert np.array_equal(np.concatenate([c[0] for c in eng.calls]), users)
        assert all(c[1].shape == (c[0].size, d) and (c[2] is None or c[2].shape == (c[0].size, d)) for c in eng.calls)
        assert np.array_equal(rank7, rank) and np.array_equal(elig7, elig)
        monkeypatch.setattr(si, '_RECOMMEND_CHUNK', 1 << 20)

        # matrix input, sparse and dense: the order of X.nonzero(); a stored zero is no pair
        M = sp.csr_matrix((vals[:len(test)], (pairs[:len(test), 0], pairs[:len(test), 1])), shape=(n, d))
        M.data[3] = 0.0
        mi, mj = M.nonzero()
        for X in (M, M.toarray()):
            rank_m, elig_m = E.rank(X, exclude_seen=exclude_seen)
            want = reference_answers(E, np.column_stack((mi, mj)), exclude_seen)
            assert rank_m.shape == (M.nnz - 1,) and np.array_equal(rank_m, want[0]) and np.array_equal(elig_m, want[1])

        # every metric against the plain loops, at several N (no cap at 64) and with relevant_from
        for n_items in (1, 3, 10, 200):
            for y_, rel in ((None, None), (vals, 3.0), (vals, None)):
                got = E.ranking_score(pairs, y_, n_items=n_items, exclude_seen=exclude_seen, relevant_from=rel)
                keep = np.ones(len(pairs), dtype=bool) if rel is None else vals >= rel
                uniq = np.unique(pairs[keep], axis=0)
                r, L = reference_answers(E, uniq, exclude_seen)
                want = rc.metrics_reference(uniq[:, 0], r, L, n_items)
                assert set(got) == set(want) == set(rc.METRICS) | {'n_items', 'users', 'targets', 'targets_not_eligible'}
                for name in want:
                    assert got[name] == pytest.approx(want[name], rel=1e-13, abs=0), (name, n_items, rel)
                assert got['targets'] == len(uniq) and got['targets_not_eligible'] == (2 * exclude_seen if rel is None else got['targets_not_eligible'])
        # a matrix's stored values stand in for y
        got = E.ranking_score(M, n_items=3, exclude_seen=exclude_seen, relevant_from=3.0)
        want = E.ranking_score(np.column_stack((mi, mj)), M.data[M.data != 0], n_items=3, exclude_seen=exclude_seen, relevant_from=3.0)
        assert got == want and 0 < got['targets'] < M.nnz - 1

    # sparsified factors are densified on copies: the estimator keeps its sparse ones
    rank, elig = E.rank(pairs)
    E.sparsify()
    rank_s, elig_s = E.rank(pairs)
    assert sp.issparse(E.W) and sp.issparse(E.T) and np.array_equal(rank_s, rank) and np.array_equal(elig_s, elig)
    E.densify()
    # no pairs: two empty arrays, and metrics that say why they are NaN
    r0, e0 = E.rank(np.zeros((0, 2)))
    assert r0.shape == (0,) and e0.shape == (0,) and r0.dtype == np.int32
    none = E.ranking_score(in_seen)
    assert none['targets'] == 2 and none['targets_not_eligible'] == 2 and none['users'] == 0
    assert all(np.isnan(none[name]) for name in rc.METRICS)

    # the refusals
    for bad in ([[0, d]], [[n, 0]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(ValueError, match='inside'):
            E.rank(np.array(bad))
    with pytest.raises(ValueError, match='n_items'):
        E.ranking_score(pairs, n_items=0)
    with pytest.raises(ValueError, match='relevant_from'):
        E.ranking_score(pairs, relevant_from=3.0)
    with pytest.raises(ValueError, match='one value per pair'):
        E.ranking_score(pairs, vals[:-1], relevant_from=3.0)
    with pytest.raises(ValueError, match='must be'):
        E.rank(sp.csr_matrix((n, d + 1)))
    del E.seen_
    with pytest.raises(ValueError, match='seen_'):
        E.rank(pairs)
    with pytest.raises(ValueError, match='seen_'):
        E.ranking_score(pairs)
    assert E.rank(pairs, exclude_seen=False)[0].shape == (len(pairs),)
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_RS_Estimator(n, d, k).rank(pairs)
    with pytest.raises(ValueError, match='not fitted'):
        si.NMF_RS_Estimator(n, d, k).ranking_score(pairs)


def test_the_metrics_of_a_hand_computed_example_of_five_items(monkeypatch):
    """Two users, five items, T the identity: a user's scores are their row of W.
    user 0: scores 5 1 4 2 3, item 1 seen.  Eligible 0 2 3 4 (L = 4), order 0 2 4 3.  Held out: items 2 and 3, ranks 1 and 3.
    user 1: scores 1 2 2 0 9, nothing seen.  L = 5, order 4 1 2 0 3 (the tie 1 | 2 by the smaller item).  Held out: item 2, rank 2,
            and item 4, rank 0.
    At N = 2:  hit_rate (1 + 1) / 2 = 1;  precision (1/2 + 1/2) / 2 = 1/2;  recall (1/2 + 1/2) / 2 = 1/2;
      ndcg: ideal 1 + 1/log2(3) for both (P = 2);  user 0 has 1/log2(3), user 1 has 1;
      mrr (1/2 + 1) / 2 = 3/4;
      auc: user 0: 1 - ((1 - 0) + (3 - 1)) / (2 * 2) = 1/4;  user 1: 1 - ((0 - 0) + (2 - 1)) / (2 * 3) = 5/6;  mean 13/24;
      mean percentile rank: (1/3 + 3/3 + 2/4 + 0/4) / 4 = 11/24."""
    from rri_nmf_amd import sklearn_interface as si
    monkeypatch.setattr(si, 'RRIEngine', FakeEngine)
    W = np.array([[5.0, 1.0, 4.0, 2.0, 3.0], [1.0, 2.0, 2.0, 0.0, 9.0]])
    E = si.NMF_RS_Estimator(2, 5, 5, W=W, T=np.eye(5))
    E.min_rating, E.max_rating = 0.0, 10.0
    E.seen_ = sp.csr_matrix(([1.0], ([0], [1])), shape=(2, 5))
    pairs = np.array([[1, 2], [0, 3], [0, 2], [1, 4]])
    rank, elig = E.rank(pairs)
    assert rank.tolist() == [2, 3, 1, 0] and elig.tolist() == [5, 4, 4, 5]
    got = E.ranking_score(pairs, n_items=2)
    ideal = 1.0 + 1.0 / np.log2(3.0)
    want = {'n_items': 2, 'users': 2, 'targets': 4, 'targets_not_eligible': 0, 'hit_rate': 1.0, 'precision': 0.5, 'recall': 0.5,
            'ndcg': ((1.0 / np.log2(3.0)) / ideal + 1.0 / ideal) / 2, 'mrr': 0.75, 'auc': 13.0 / 24.0, 'mean_percentile_rank': 11.0 / 24.0}
    assert set(got) == set(want)
    for name in want:
        assert got[name] == pytest.approx(want[name], rel=1e-14), name
    assert rc.metrics_reference(pairs[:, 0], rank, elig, 2) == pytest.approx(want, rel=1e-14)
    # the seen pair as a target: not eligible, counted, and out of every mean
    more = E.ranking_score(np.vstack([pairs, [[0, 1]]]), n_items=2)
    assert more['targets'] == 5 and more['targets_not_eligible'] == 1
    assert all(more[name] == got[name] for name in rc.METRICS)
