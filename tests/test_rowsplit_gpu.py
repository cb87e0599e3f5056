"""The split of a resident corpus by row on the GPU: DeviceCorpus.split_rows (include/rri_corpus_rowsplit.h) and what is composed of
it, NMF_RS_Estimator.ranking_score_new_users and leave-one-out for known users.

The oracle is the numpy restatement of rri_rowsplit.hpp (tests/rowsplit_cases.py: the Philox of tests/derive_cases.py, a full sort of
every row's keys), held against the plain loop on the CPU; both outputs are compared array for array -- indptr, indices, the values'
bits.  The edge corpus has rows of 0, 1, 2, 63, 64, 65 (the wave class ends at 64 entries), 255, 256, 257 (a workgroup's stride),
1023, 1024, 1025 (a piece) and 2500 entries (three pieces); no shape is larger.  Every refusal exercised here is an argument check
that returns a status."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

import corpus_build_cases as cb
import corpus_rank_cases as cc
import derive_cases as dc
import fold_cases as fo
import rowsplit_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MODES = [dict(n_held=1), dict(n_held=2), dict(n_held=64), dict(n_held=3000), dict(held_out=0.2), dict(held_out=0.5), dict(held_out=1.0)]
SEEDS = (12345, (5 << 32) | 12345)          # the second has a non-zero high word


def D():
    from rri_nmf_amd.engine import DeviceCorpus
    return DeviceCorpus


def si():
    from rri_nmf_amd import sklearn_interface
    return sklearn_interface


def memory():
    from rri_nmf_amd.engine import corpus_memory, device_memory
    return corpus_memory(), device_memory()


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same(A, B):
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(bits(A.data), bits(B.data)))


def load(name):
    A = sp.load_npz(os.path.join(GOLDEN, 'ref_data', name)).tocsr().astype(np.float64)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A


@pytest.fixture(scope='module')
def corpora():
    return {'edge': rc.edge_corpus(), 'random': rc.random_corpus()}


def check_split(corpus, A, seed, min_observed, **mode):
    """split_rows against the restatement, byte for byte, with the counts, the info fields and the memory counters; returns held"""
    want_o, want_h = rc.split_rows(A, min_observed=min_observed, seed=seed, **mode)
    before = memory()
    observed, held = corpus.split_rows(min_observed=min_observed, random_state=seed, **mode)
    with observed, held:
        O, H = observed.to_scipy(), held.to_scipy()
        assert same(O, want_o) and same(H, want_h), (mode, min_observed, seed)
        assert np.array_equal(np.diff(H.indptr), rc.quota(np.diff(A.indptr), min_observed=min_observed, **mode))        # exactly the quota
        total = sp.csr_matrix(O + H)
        total.sort_indices()
        assert same(total, A) and O.multiply(H).nnz == 0 and O.nnz + H.nnz == A.nnz                    # disjoint, and their union is A
        assert (O.has_canonical_format or O.nnz == 0) and (H.has_canonical_format or H.nnz == 0)
        for part, M in ((observed, O), (held, H)):
            assert part.shape == A.shape and part.nnz == part.stored == M.nnz and part.negatives == (M.data < 0).sum()
            assert part.rows_rewritten == part.duplicates_merged == part.zeros_dropped == part.long_rows == 0 and part.ingest_ms >= 0
        assert memory()[0] == (before[0][0] + 2, before[0][1] + observed.device_bytes + held.device_bytes) and memory()[1] == before[1]
    assert memory() == before
    return H


@pytest.mark.parametrize('name', ['edge', 'random'])
def test_both_outputs_equal_the_restatement_byte_for_byte(corpora, name):
    A = corpora[name]
    with D()(A) as corpus:
        held = {}
        for mode in MODES:
            for min_observed in (0, 1, 5):
                for seed in SEEDS:
                    held[(tuple(mode.items()), min_observed, seed)] = check_split(corpus, A, seed, min_observed, **mode)
        assert same(corpus.to_scipy(), A)                                                 # the source is what it was
    one, other = held[((('n_held', 1),), 1, SEEDS[0])], held[((('n_held', 1),), 1, SEEDS[1])]
    assert not same(one, other) and one.nnz == (np.diff(A.indptr) >= 2).sum()           # a second seed gives another split
    assert held[((('held_out', 1.0),), 0, SEEDS[0])].nnz == A.nnz                       # everything, with nothing kept back
    # nested in the quota: what one entry per row gives up is among what two give up, row by row
    for seed in SEEDS:
        h1, h2 = held[((('n_held', 1),), 0, seed)], held[((('n_held', 2),), 0, seed)]
        assert h2.nnz > h1.nnz > 0
        for r in range(A.shape[0]):
            assert set(h1.indices[h1.indptr[r]:h1.indptr[r + 1]].tolist()) <= set(h2.indices[h2.indptr[r]:h2.indptr[r + 1]].tolist()), r


def test_where_split_entries_holds_m_entries_of_a_row_a_quota_of_m_holds_the_same(corpora):
    """device against device: with held_out 0.1 and seed 12345, 71 % of the rows of the random corpus hold 1, 2 or 3 entries out under
    split_entries and have that number as their quota (computed on the CPU first, tests/test_rowsplit_cpu.py); at least a tenth must"""
    A = corpora['random']
    held_out, seed = 0.1, 12345
    with D()(A) as corpus:
        o, by_entry = corpus.split_entries(held_out=held_out, random_state=seed)
        with o, by_entry:
            E = by_entry.to_scipy()
        assert same(E, cb.split_entries(A, dc.threshold(held_out), seed)[1])
        m = np.diff(E.indptr)
        compared = 0
        for k in (1, 2, 3):
            o, by_row = corpus.split_rows(n_held=k, min_observed=1, random_state=seed)
            with o, by_row:
                R = by_row.to_scipy()
            rows = np.flatnonzero((m == k) & (np.diff(R.indptr) == k) & (rc.quota(np.diff(A.indptr), n_held=k, min_observed=1) == k))
            for r in rows:
                assert np.array_equal(R.indices[R.indptr[r]:R.indptr[r + 1]], E.indices[E.indptr[r]:E.indptr[r + 1]]), (k, r)
            compared += rows.size
    print('rows compared with split_entries: %d of %d' % (compared, A.shape[0]))
    assert compared >= 0.1 * A.shape[0]


def test_two_calls_give_the_same_bytes_and_empty_corpora_work(corpora):
    A = corpora['edge']
    with D()(A) as corpus:
        for kw in (dict(n_held=1), dict(held_out=0.2, min_observed=0)):
            a = corpus.split_rows(random_state=9, **kw)
            b = corpus.split_rows(random_state=9, **kw)
            with a[0], a[1], b[0], b[1]:
                assert same(a[0].to_scipy(), b[0].to_scipy()) and same(a[1].to_scipy(), b[1].to_scipy()) and a[1].nnz > 0
        observed, held = si().split_rows(corpus, n_held=2, random_state=7)               # the public dispatch
        with observed, held:
            assert same(held.to_scipy(), rc.split_rows(A, n_held=2, seed=7)[1])
    for empty in (sp.csr_matrix((0, 5)), sp.csr_matrix((4, 5))):
        with D()(empty) as corpus:
            for kw in (dict(n_held=1), dict(held_out=1.0, min_observed=0)):
                assert check_split(corpus, empty, 1, kw.pop('min_observed', 1), **kw).nnz == 0


def test_every_refusal_leaves_the_outputs_null_and_the_counters_as_they_were():
    from rri_nmf_amd.engine import RRIEngine
    A = dc.count_corpus([3, 0, 70, 300], 400, seed=3)
    start = memory()
    with D()(A) as c:
        gone = D()(A)               # made while c lives, so its address is not c's
        stale = gone._ptr().value
        gone.close()
        before = memory()
        requests = {'count_zero': (0, 0.0, 1), 'count_minus_two': (-2, 0.0, 1), 'both_modes': (3, 0.5, 1), 'count_with_nan': (1, float('nan'), 1),
                    'fraction_zero': (-1, 0.0, 1), 'fraction_above_one': (-1, 1.5, -1), 'fraction_negative': (-1, -0.25, 1),
                    'fraction_nan': (-1, float('nan'), 1), 'min_observed_negative': (1, 0.0, -1), 'min_observed_negative_last': (-1, 0.5, -4)}
        with RRIEngine(1, 1, 1, dtype=np.float64) as eng:
            split = eng._lib.rri_corpus_split_rows
            inside = memory()             # with the handle's own buffers
            for name, (n_held, fraction, min_observed) in requests.items():
                observed, held = C.c_void_p(5), C.c_void_p(6)
                st = split(eng._h, c._ptr(), n_held, fraction, min_observed, 3, C.byref(observed), C.byref(held))
                assert st == -1 and eng._err() == rc.REQUEST_TEXT[name] and not observed.value and not held.value, name
                assert memory() == inside, name
            observed, held = C.c_void_p(5), C.c_void_p(6)
            assert split(eng._h, c._ptr(), 1, 0.0, 1, 3, None, C.byref(held)) == -1 and eng._err() == rc.REQUEST_TEXT['observed_null'] and not held.value
            assert split(eng._h, c._ptr(), 0, 2.0, -1, 3, C.byref(observed), None) == -1 and eng._err() == rc.REQUEST_TEXT['held_null_first'] and not observed.value
            for dead in (None, C.c_void_p(stale)):
                observed, held = C.c_void_p(5), C.c_void_p(6)
                assert split(eng._h, dead, 1, 0.0, 1, 3, C.byref(observed), C.byref(held)) == -1 and 'NULL or has been destroyed' in eng._err()
                assert not observed.value and not held.value
            assert memory() == inside
        assert memory() == before
        # a good call after the refusals, and its outputs destroyed: the counters return to their start
        observed, held = c.split_rows(n_held=1)
        assert memory()[0][0] == before[0][0] + 2 and held.nnz == 3
        observed.close()
        held.close()
        assert memory() == before
        for bad in (dict(), dict(n_held=1, held_out=0.5), dict(n_held=0), dict(held_out=1.5), dict(n_held=1, min_observed=-1)):
            with pytest.raises(ValueError):
                c.split_rows(**bad)
        assert memory() == before
    assert memory() == start


# ---- the two protocols on the reference's recommender fixture ---------------------------------------------------------------------------
KW = dict(random_state=0, max_iter=8, use_validation_early_stopping=False, nmf_kwargs={'device_init': True})


def host_protocol(E, observed, held, n_items):
    """the protocol through the host: the two parts downloaded, transform, ranking_score with the held pairs against an estimator
    that holds the folded rows and has seen the observed pairs"""
    O, H = observed.to_scipy(), held.to_scipy()
    W_host = E.transform(O)
    host = si().NMF_RS_Estimator(O.shape[0], O.shape[1], E.k, W=W_host, T=E.T)
    host.min_rating, host.max_rating = E.min_rating, E.max_rating
    host.seen_ = sp.csr_matrix((np.ones(O.nnz), O.indices, O.indptr), shape=O.shape)
    return W_host, host.ranking_score(H, n_items=n_items), O


def test_ranking_score_new_users_is_the_three_calls_written_out_and_agrees_with_the_host_route():
    A, B = load('recsys_data_train.npz'), load('recsys_data_test.npz')
    assert A.shape == (100, 200) and A.nnz == 617 and B.shape == (100, 200)
    with D()(A) as ratings:
        with ratings.take_rows(np.arange(60)) as known:
            E = si().NMF_RS_Estimator(60, 200, 5, **KW).fit_corpus(known, keep_seen=False)
        # users the fit never saw, with at least 3 ratings: the other rows of the 617-rating fixture, and the rows of its held-out twin
        for source, M, first in ((ratings, A, 60), (None, B, 0)):
            users = np.flatnonzero(np.diff(M.indptr) >= 3)
            users = users[users >= first]
            assert users.size >= 15
            src = source if source is not None else D()(M)
            try:
                with src.take_rows(users) as new:
                    before = memory()
                    got = E.ranking_score_new_users(new, n_items=10, n_held=1)
                    assert memory() == before
                    # the composition by hand
                    observed, held = new.split_rows(n_held=1, min_observed=1, random_state=E.random_state)
                    with observed, held:
                        W_new = E.transform_corpus(observed)
                        want = E.ranking_score_corpus(held, 10, exclude=observed, W=W_new)
                        assert set(got) == set(want) | {'observed_entries', 'held_entries'}
                        for key in want:
                            assert np.array_equal(bits(got[key]), bits(want[key])), (key, got[key], want[key])
                        assert got['held_entries'] == users.size == held.nnz and got['observed_entries'] == new.nnz - users.size == observed.nnz
                        assert got['users'] == users.size and got['targets'] == users.size and got['targets_not_eligible'] == 0
                        # through the host: the fold within test_fold_gpu.py's bound on this fixture, the metrics within
                        # test_corpus_rank_gpu.py's
                        W_host, host, O = host_protocol(E, observed, held, 10)
                        mask = (O != 0).toarray()
                        err = fo.relfro(mask * (W_new @ E.T), mask * (W_host @ E.T))
                        print('transform_corpus vs transform on the observed part: M.(W T) %.3e' % err)
                        assert err < 1e-6
                        cc.check_metrics(got, host)
                    # the default: a fifth of every user's ratings, the estimator's own seed
                    fifth = E.ranking_score_new_users(new)
                    lengths = np.diff(M.indptr)[users]
                    assert fifth['held_entries'] == rc.quota(lengths, held_out=0.2).sum() and fifth['observed_entries'] == new.nnz - fifth['held_entries']
                    assert memory() == before
            finally:
                if source is None:
                    src.close()


def test_leave_one_out_for_known_users():
    A = load('recsys_data_train.npz')
    lengths = np.diff(A.indptr)
    with D()(A) as ratings:
        train, test = ratings.split_rows(n_held=1)
        with train, test:
            assert test.nnz == (lengths >= 2).sum() == 74 and train.nnz == 617 - 74
            E = si().NMF_RS_Estimator(100, 200, 5, **KW).fit_corpus(train, keep_seen=False)
            got = E.ranking_score_corpus(test, exclude=train)
            assert got['users'] == got['targets'] == 74 and got['targets_not_eligible'] == 0
            rank, eligible = E.rank_corpus(test, exclude=train)
            assert rank.size == 74 and np.all(rank >= 0)                       # one ranked entry for every user with two ratings or more
            T_ = test.to_scipy()
            assert np.array_equal(np.diff(T_.indptr), (lengths >= 2).astype(np.int64))
            assert np.all(eligible[lengths >= 2] == 200 - (lengths[lengths >= 2] - 1)) and np.all(eligible[lengths < 2] == -1)
            assert 0.0 <= got['hit_rate'] <= 1.0 and 0.0 < got['mrr'] <= 1.0
