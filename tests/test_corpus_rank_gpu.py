"""Ranking against resident corpora on the GPU (include/rri_corpus_rank.h): rri_corpus_rank_entries and rri_corpus_topn_rows against
rri_rank_entries and rri_topn_rows given the same lists as host arrays, bit for bit; rri_corpus_ranking_metrics against
NMF_RS_Estimator.ranking_score on the downloaded corpus (the parent's route) within the bound of tests/corpus_rank_cases.py, and
against the numpy restatement of the plain loop bit for bit; the bit-equality rules, the memory counters and the refusals; and the
three estimator methods on the reference's recommender fixture.

The shapes are the smallest that reach every edge: 150 rows of W (200 pieces: four workgroups of k_rank_entries), d = 130 (two full
64-column chunks and a tail of 2), k = 5, 33 and 129 (one panel, TOPN_KP + 1, five panels), targets rows of 0, 1, 63, 64, 65 and 129
entries, a row whose exclusion holds every column, a target inside its row's exclusion, a row of W with a NaN, two equal columns
of T, and the row list absent, permuted and with repeats."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

import corpus_rank_cases as cc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
KS = [5, 33, 129]
N, D = cc.N_EDGE, cc.D_EDGE
bits = cc.bits


def lib():
    from rri_nmf_amd import engine
    return engine


def cr():
    from rri_nmf_amd import corpus_rank
    return corpus_rank


def factors_only(W, T):
    eng = lib().RRIEngine(W.shape[0], T.shape[1], W.shape[1], dtype=np.float64, weighted=False)
    eng.set_W(W)
    eng.set_T(T)
    return eng


@pytest.fixture(scope='module')
def edge():
    """the targets and the exclusion of the edge case: scipy matrices and corpora"""
    E = lib()
    tgt = cc.edge_targets()
    exc = cc.edge_exclusion(tgt)
    lens = np.diff(tgt.indptr)
    assert set(cc.LENS) <= set(lens.tolist()) and lens.max() == 129 <= D - 1 and len(cc.pieces(tgt.indptr)) > 64
    assert exc[cc.ROW_FULL].nnz == D and exc[cc.ROW_INSIDE, tgt.indices[tgt.indptr[cc.ROW_INSIDE]]] == 1 and exc[5].nnz == 0
    tc, ec = E.DeviceCorpus(tgt), E.DeviceCorpus(exc)
    assert tc.nnz == tgt.nnz and ec.nnz == exc.nnz
    yield tgt, exc, tc, ec
    tc.close()
    ec.close()


def rows_of(kind):
    rows = cc.edge_rows(kind)
    return rows, (np.arange(N) if rows is None else rows)


# ---- 1. the corpus entry points are the host-list entry points, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_ranks_values_eligible_counts_and_top_n_lists_equal_the_host_list_entry_points(edge, k):
    tgt, exc, tc, ec = edge
    W, T = cc.edge_factors(k)
    has = np.diff(tgt.indptr) > 0
    with factors_only(W, T) as eng:
        for kind in ('null', 'permuted', 'repeat'):
            rows, i = rows_of(kind)
            for excl, clip in ((True, (1.0, 5.0)), (False, (None, None))):
                want = eng.rank_entries(rows, tgt, exclude=exc[i] if excl else None, clip=clip)
                got = cr().rank_entries(eng, tc, rows=rows, exclude=ec if excl else None, clip=clip)
                assert np.array_equal(want.indices, tgt.indices)
                assert np.array_equal(got['rank'], want.rank), (kind, excl)
                assert np.array_equal(bits(got['val']), bits(want.val)), (kind, excl)
                assert np.array_equal(got['eligible'][has], want.eligible[has]) and np.all(got['eligible'][~has] == -1), (kind, excl)
                assert got['kernel_ms'] > 0
                if kind == 'null' and excl:          # the edges are what they were made to be
                    seg = lambda r: slice(tgt.indptr[r], tgt.indptr[r + 1])
                    assert np.all(got['rank'][seg(cc.ROW_FULL)] == -1) and got['eligible'][cc.ROW_FULL] == 0
                    assert got['rank'][tgt.indptr[cc.ROW_INSIDE]] == -1 and np.isnan(got['val'][tgt.indptr[cc.ROW_INSIDE]])
                    assert np.all(got['rank'][seg(cc.ROW_NAN)] == -1) and got['eligible'][cc.ROW_NAN] == 0
                    assert got['eligible'][5] == D
                    r = cc.ROW_INSIDE + 6                 # both tied columns are targets there, and neither is excluded here
                    cols = tgt.indices[seg(r)].tolist()
                    if not exc[r, cc.TIE[0]] and not exc[r, cc.TIE[1]]:
                        a, b = (got['rank'][seg(r)][cols.index(c)] for c in cc.TIE)
                        assert b == a + 1                  # equal scores: the smaller column stands right before the larger
                # outputs that are not asked for
                only = cr().rank_entries(eng, tc, rows=rows, exclude=ec if excl else None, clip=clip, values=False)
                assert only['val'] is None and np.array_equal(only['rank'], want.rank)
            for topn in (1, 10, 64):
                for excl, clip in ((True, (1.0, 5.0)), (False, (None, None))):
                    wj, wv = eng.topn_rows(rows, topn, exclude=exc[i] if excl else None, clip=clip)
                    gj, gv, ms = cr().topn_rows(eng, rows, topn, exclude=ec if excl else None, clip=clip)
                    assert np.array_equal(gj, wj) and np.array_equal(bits(gv), bits(wv)) and ms > 0, (kind, topn, excl)
            # any list of rows, shorter or longer than n, against the whole exclusion
            some = np.array([cc.ROW_FULL, 3, 3, 149, cc.ROW_NAN, 0] * 30, dtype=np.int64)
            wj, wv = eng.topn_rows(some, 10, exclude=exc[some], clip=(1.0, 5.0))
            gj, gv, _ = cr().topn_rows(eng, some, 10, exclude=ec, clip=(1.0, 5.0))
            assert np.array_equal(gj, wj) and np.array_equal(bits(gv), bits(wv)) and np.all(gj[0] == -1)


# ---- 2. the metrics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', KS)
def test_metrics_against_ranking_score_on_the_download_and_the_restatement_in_bits(edge, k):
    """Counts equal.  Each metric within (m + 16) 2^-52 relative, m the number of users averaged: every term is a non-negative
    float64 of a few correctly rounded operations, and the two routes differ only in the order of at most m additions (and at most
    64 in a row's dcg).  The totals equal the plain loop's restatement bit for bit."""
    from rri_nmf_amd import sklearn_interface as si
    tgt, exc, tc, ec = edge
    W, T = cc.edge_factors(k)
    est = si.NMF_RS_Estimator(N, D, k, W=W, T=T)
    est.min_rating, est.max_rating = 1.0, 5.0
    est.seen_ = exc
    with factors_only(W, T) as eng:
        for n_items in (1, 10, 200):
            for rf in (None, 4.0):
                for excl in (True, False):
                    want = est.ranking_score(tc.to_scipy(), n_items=n_items, exclude_seen=excl, relevant_from=rf)        # the parent's route
                    got = est.ranking_score_corpus(tc, n_items=n_items, exclude=ec if excl else None, relevant_from=rf)
                    assert set(got) == set(want)
                    assert want['users'] > 90 and want['targets_not_eligible'] > 0
                    cc.check_metrics(got, want)
                for kind in ('null', 'permuted', 'repeat'):
                    rows, _ = rows_of(kind)
                    ranks = cr().rank_entries(eng, tc, rows=rows, exclude=ec)
                    sums, ms = cr().ranking_sums(eng, tc, n_items, rows=rows, exclude=ec, relevant_from=rf)
                    ref = cc.totals(cc.row_terms(tgt.indptr, tgt.data, ranks['rank'], ranks['eligible'], n_items, rf, D))
                    assert np.array_equal(bits(sums), bits(ref)), (n_items, rf, kind, sums, ref)
                    assert ms > 0 and not sums[12:].any()


def test_metrics_of_more_rows_than_one_block_of_the_totals():
    """2500 corpus rows against 40 rows of W: three blocks of the first level of the totals, rows repeated"""
    E = lib()
    A, _, _ = cc.random_case(2500, 70, seed=11, lens=np.random.RandomState(11).randint(0, 6, size=2500))
    rng = np.random.RandomState(12)
    W, T = 0.1 + rng.rand(40, 7), 0.1 + rng.rand(7, 70)
    rows = rng.randint(0, 40, size=2500).astype(np.int64)
    with E.DeviceCorpus(A) as tc, factors_only(W, T) as eng:
        ranks = cr().rank_entries(eng, tc, rows=rows)
        want = eng.rank_entries(rows, A)
        assert np.array_equal(ranks['rank'], want.rank)
        sums, _ = cr().ranking_sums(eng, tc, 10, rows=rows, relevant_from=3.0)
        ref = cc.totals(cc.row_terms(A.indptr, A.data, ranks['rank'], ranks['eligible'], 10, 3.0, 70))
        assert np.array_equal(bits(sums), bits(ref)) and sums[0] > 1024


# ---- 3. the same bits alone, among others, twice and on handles of another flavour; nothing is kept --------------------------------------
@pytest.mark.parametrize('k', [5, 129])
def test_a_request_has_the_same_bits_alone_twice_and_on_another_handle(edge, k):
    E = lib()
    tgt, exc, tc, ec = edge
    W, T = cc.edge_factors(k)
    rows, _ = rows_of('repeat')
    rng = np.random.RandomState(5)
    P = sp.csr_matrix((rng.rand(N, D) < 0.05).astype(np.float64))
    with factors_only(W, T) as eng, E.RRIEngine(N, D, k, dtype=np.float64) as dense, E.RRIEngine(N, D, k, dtype=np.float32, weighted='sparse') as pat:
        dense.upload_X(rng.rand(N, D))
        pat.upload_observed_csr(P)
        for h in (dense, pat):
            h.set_W(W)
            h.set_T(T)
        mem, cor = E.device_memory(), E.corpus_memory()
        a = cr().rank_entries(eng, tc, rows=rows, exclude=ec, clip=(1.0, 5.0))
        sa, _ = cr().ranking_sums(eng, tc, 10, rows=rows, exclude=ec, relevant_from=4.0)
        ja, va, _ = cr().topn_rows(eng, rows, 10, exclude=ec, clip=(1.0, 5.0))
        assert E.device_memory() == mem and E.corpus_memory() == cor
        for h in (eng, dense, pat):                       # a second call; two other flavours
            b = cr().rank_entries(h, tc, rows=rows, exclude=ec, clip=(1.0, 5.0))
            assert np.array_equal(a['rank'], b['rank']) and np.array_equal(bits(a['val']), bits(b['val'])) and np.array_equal(a['eligible'], b['eligible'])
            sb, _ = cr().ranking_sums(h, tc, 10, rows=rows, exclude=ec, relevant_from=4.0)
            assert np.array_equal(bits(sa), bits(sb))
            jb, vb, _ = cr().topn_rows(h, rows, 10, exclude=ec, clip=(1.0, 5.0))
            assert np.array_equal(ja, jb) and np.array_equal(bits(va), bits(vb))
            assert E.device_memory() == mem and E.corpus_memory() == cor
        terms = cc.row_terms(tgt.indptr, tgt.data, a['rank'], a['eligible'], 10, 4.0, D)
        for q in list(range(12)) + [19, 20, 149]:        # a row alone: a one-row corpus, derived on the device
            with tc[q:q + 1] as one:
                alone = cr().rank_entries(eng, one, rows=rows[q:q + 1], exclude=ec, clip=(1.0, 5.0))
                s1, _ = cr().ranking_sums(eng, one, 10, rows=rows[q:q + 1], exclude=ec, relevant_from=4.0)
            seg = slice(tgt.indptr[q], tgt.indptr[q + 1])
            assert np.array_equal(alone['rank'], a['rank'][seg]) and np.array_equal(bits(alone['val']), bits(a['val'][seg]))
            assert alone['eligible'][0] == a['eligible'][q]
            assert np.array_equal(bits(s1[:cc.TERMS]), bits(terms[q])), q        # the totals of one row are the row's terms
        assert E.device_memory() == mem and E.corpus_memory() == cor


def test_ranking_between_two_sweeps_changes_nothing():
    E = lib()
    rng = np.random.RandomState(1)
    obs = sp.csr_matrix((rng.rand(60, 90) < 0.3) * rng.randint(1, 6, size=(60, 90)).astype(np.float64))
    s = np.sqrt(obs.data.mean() / (5 * 0.36))            # a start about as large as the data
    W0, T0 = s * (0.1 + rng.rand(60, 5)), s * (0.1 + rng.rand(5, 90))
    A, _, _ = cc.random_case(60, 90, seed=7, lens=rng.randint(0, 20, size=60))
    out = []
    with E.DeviceCorpus(A) as tc, E.DeviceCorpus(obs) as ec:
        for score in (False, True):
            with E.RRIEngine(60, 90, 5, dtype=np.float64, weighted='sparse') as eng:
                eng.upload_observed_csr(obs)
                eng.set_W(W0)
                eng.set_T(T0)
                eng.set_params(reset_topic_method=None)
                eng.sweep(1)
                if score:
                    mem = E.device_memory()
                    W1, T1 = eng.get_W(), eng.get_T()
                    got = cr().ranking_sums(eng, tc, 10, exclude=ec)[0]
                    lists = cr().topn_rows(eng, None, 5, exclude=ec)
                    with factors_only(W1, T1) as ref:          # the current factors, not the start's
                        assert np.array_equal(bits(got), bits(cr().ranking_sums(ref, tc, 10, exclude=ec)[0])) and got[0] > 0
                        assert np.array_equal(lists[0], ref.topn_rows(None, 5, exclude=obs)[0])
                    assert E.device_memory() == mem
                eng.sweep(1)
                out.append((eng.get_W(), eng.get_T(), eng.objective()))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1])) and out[0][2] == out[1][2]


# ---- 4. refusals and the empty corpus ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was_and_an_empty_corpus_returns_zeros(edge):
    E = lib()
    from rri_nmf_amd import _capi
    tgt, exc, tc, ec = edge
    W, T = cc.edge_factors(5)
    I32P, DP = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    with E.DeviceCorpus(sp.csr_matrix((4, D))) as empty, E.DeviceCorpus(sp.csr_matrix(np.ones((3, D - 1)))) as narrow, \
            E.DeviceCorpus(sp.csr_matrix(np.ones((N + 1, D)))) as tall, E.DeviceCorpus(sp.csr_matrix(np.ones((N - 1, D)))) as short:
        with E.RRIEngine(N, D, 5, dtype=np.float64) as bare:
            got = cr().rank_entries(bare, empty)          # nothing to score: W and T are not even needed
            assert got['rank'].size == 0 and got['val'].size == 0 and np.all(got['eligible'] == -1) and got['kernel_ms'] == 0
            sums, ms = cr().ranking_sums(bare, empty, 10)
            assert not sums.any() and ms == 0
            none = cr().ranking_metrics(bare, empty, 10)
            assert none['users'] == 0 and none['targets'] == 0 and all(np.isnan(none[m]) for m in cc.METRICS)
            j, v, ms = cr().topn_rows(bare, np.zeros(0, dtype=np.int64), 10, exclude=ec)
            assert j.shape == (0, 10) and ms == 0
            for call in (lambda: cr().rank_entries(bare, tc), lambda: cr().ranking_sums(bare, tc, 10), lambda: cr().topn_rows(bare, [0], 1)):
                with pytest.raises(ValueError, match='W and T must be set first'):
                    call()
        with factors_only(W, T) as eng:
            before = cr().rank_entries(eng, tc, exclude=ec)
            mem, cor = E.device_memory(), E.corpus_memory()
            rank3 = (lambda **kw: cr().rank_entries(eng, **kw), lambda **kw: cr().ranking_sums(eng, n_items=10, **kw))
            for call in rank3:
                with pytest.raises(ValueError, match='the corpus has %d columns, W T has %d' % (D - 1, D)):
                    call(targets=narrow)
                with pytest.raises(ValueError, match='rows is NULL and the corpus has %d rows, W has %d' % (N + 1, N)):
                    call(targets=tall)
                with pytest.raises(ValueError, match=r'rows\[1\] = %d is out of range' % N):
                    call(targets=tc, rows=np.r_[0, N, np.zeros(N - 2, dtype=np.int64)])
                with pytest.raises(ValueError, match=r'rows\[2\] = -1 is out of range'):
                    call(targets=tc, rows=np.r_[0, 1, -1, np.zeros(N - 3, dtype=np.int64)])
                with pytest.raises(ValueError, match='one row of W per row of the corpus'):
                    call(targets=tc, rows=[0, 1])
                with pytest.raises(ValueError, match='the exclusion corpus is %d x %d, the handle %d x %d' % (N - 1, D, N, D)):
                    call(targets=tc, exclude=short)
            with pytest.raises(ValueError, match='clip_lo 5 is above clip_hi 1'):
                cr().rank_entries(eng, tc, clip=(5.0, 1.0))
            with pytest.raises(ValueError, match='a clip bound is NaN'):
                cr().rank_entries(eng, tc, clip=(float('nan'), 1.0))
            with pytest.raises(ValueError, match='a clip bound is NaN'):
                cr().topn_rows(eng, [0], 3, clip=(1.0, float('nan')))
            with pytest.raises(ValueError, match='n_items 0 is not a positive integer'):
                cr().ranking_sums(eng, tc, 0)
            for topn in (0, _capi.RRI_MAX_TOPN + 1):
                with pytest.raises(NotImplementedError, match='topn %d outside 1 .. 64' % topn):
                    cr().topn_rows(eng, [0], topn, exclude=ec)
            with pytest.raises(ValueError, match=r'rows\[1\] = %d is out of range' % N):
                cr().topn_rows(eng, [0, N], 3)
            # the library's own checks of what the Python functions check first: a destroyed corpus, an exclusion of another shape
            gone = E.DeviceCorpus(tgt)
            where = ctypes.c_void_p(gone._ptr().value)
            gone.close()
            with pytest.raises(ValueError, match='the corpus is closed'):
                cr().rank_entries(eng, gone)
            out, ms = (ctypes.c_double * 16)(*[7.0] * 16), ctypes.c_double(5.0)
            L = eng._lib
            assert L.rri_corpus_ranking_metrics(eng._h, where, None, None, 10, float('nan'), out, ctypes.byref(ms)) == _capi.RRI_ERR_INVALID
            assert 'the targets corpus is NULL or has been destroyed' in eng._err()
            assert L.rri_corpus_ranking_metrics(eng._h, None, None, None, 10, float('nan'), out, ctypes.byref(ms)) == _capi.RRI_ERR_INVALID
            assert 'the targets corpus is NULL or has been destroyed' in eng._err()
            assert L.rri_corpus_ranking_metrics(eng._h, tc._ptr(), None, where, 10, float('nan'), out, ctypes.byref(ms)) == _capi.RRI_ERR_INVALID
            assert 'the exclusion corpus has been destroyed' in eng._err()
            assert L.rri_corpus_ranking_metrics(eng._h, tc._ptr(), None, short._ptr(), 10, float('nan'), out, ctypes.byref(ms)) == _capi.RRI_ERR_INVALID
            assert 'the exclusion corpus is %d x %d, the handle %d x %d' % (N - 1, D, N, D) in eng._err()
            idx, val = (ctypes.c_int32 * 4)(), (ctypes.c_double * 4)()
            assert L.rri_corpus_topn_rows(eng._h, None, 1, 4, where, 1.0, 5.0, idx, val, ctypes.byref(ms)) == _capi.RRI_ERR_INVALID
            assert 'the exclusion corpus has been destroyed' in eng._err()
            assert L.rri_corpus_topn_rows(eng._h, None, 1, 4, None, 1.0, 5.0, None, val, ctypes.byref(ms)) == _capi.RRI_ERR_INVALID
            assert 'an output array is NULL' in eng._err()
            assert L.rri_corpus_ranking_metrics(eng._h, tc._ptr(), None, None, 10, float('nan'), None, ctypes.byref(ms)) == _capi.RRI_ERR_INVALID
            assert list(out) == [7.0] * 16 and ms.value == 5.0
            assert E.device_memory() == mem and E.corpus_memory() == cor
            # with rows, a corpus of any number of rows; and the handle answers as before
            assert cr().ranking_metrics(eng, tall, 10, rows=np.zeros(N + 1, dtype=np.int64))['targets'] == (N + 1) * D
            after = cr().rank_entries(eng, tc, exclude=ec)
            assert np.array_equal(before['rank'], after['rank']) and np.array_equal(bits(before['val']), bits(after['val']))
            assert E.device_memory() == mem and E.corpus_memory() == cor


# ---- 5. the estimator on the reference's recommender fixture -------------------------------------------------------------------------------
def test_the_estimator_methods_on_the_recsys_fixture():
    from rri_nmf_amd import sklearn_interface as si
    from rri_nmf_amd.corpus_fit import pattern_of
    E = lib()
    A = sp.load_npz(os.path.join(GOLDEN, 'ref_data', 'recsys_data_train.npz')).tocsr().astype(np.float64)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    assert A.shape == (100, 200) and A.nnz == 617
    with E.DeviceCorpus(A) as full:
        train, test = full.split_entries(0.2, random_state=3)
        try:
            assert train.nnz + test.nnz == 617 and test.nnz > 50
            est = si.NMF_RS_Estimator(100, 200, 5, random_state=0, max_iter=8, use_validation_early_stopping=False).fit_corpus(train, keep_seen=False)
            mem, cor = E.device_memory(), E.corpus_memory()
            got_lists = est.recommend_corpus(n_items=10, exclude=full)
            got_some = est.recommend_corpus([99, 0, 0, 57], n_items=64, exclude=full)
            got_rank = est.rank_corpus(test, exclude=full)
            got = {(n, rf): est.ranking_score_corpus(test, n_items=n, exclude=full, relevant_from=rf) for n in (1, 10) for rf in (None, 4.0)}
            assert E.device_memory() == mem and E.corpus_memory() == cor
            # the parent's route: seen_ from the full corpus, the held-out pairs through a download
            est.seen_ = pattern_of(full)
            T_ = test.to_scipy()
            for key, g in got.items():
                cc.check_metrics(g, est.ranking_score(T_, n_items=key[0], relevant_from=key[1]))
            # every held-out pair is in the full corpus: with it as the exclusion nothing is eligible, and the counts say so
            assert got[(10, None)]['users'] == 0 and got[(10, None)]['targets'] == test.nnz == got[(10, None)]['targets_not_eligible']
            assert np.all(got_rank[0] == -1)
            # against the training corpus the held-out pairs are ranked: the usual evaluation
            est.seen_ = pattern_of(train)
            for n, rf in ((10, None), (5, 4.0)):
                g = est.ranking_score_corpus(test, n_items=n, exclude=train, relevant_from=rf)
                assert g['users'] > 20 and g['targets_not_eligible'] == 0
                cc.check_metrics(g, est.ranking_score(T_, n_items=n, relevant_from=rf))
            rank, eligible = est.rank_corpus(test, exclude=train)
            i, j = T_.nonzero()
            want_rank, want_elig = est.rank(np.column_stack((i, j)))
            assert np.array_equal(rank, want_rank) and np.array_equal(eligible[i], want_elig) and np.all(eligible[np.diff(T_.indptr) == 0] == -1)
            est.seen_ = pattern_of(full)
            for (gj, gv), users, n in ((got_lists, None, 10), (got_some, [99, 0, 0, 57], 64)):
                wj, wv = est.recommend(users, n_items=n)
                assert np.array_equal(gj, wj) and np.array_equal(bits(gv), bits(wv))
        finally:
            train.close()
            test.close()
