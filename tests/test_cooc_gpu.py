"""Co-document counts on the device (rri_cooccurrence_counts, RRIEngine.cooccurrence_counts, NMF_TM_Estimator.coherence) against
numpy on the dense 0/1 form of the corpus (tests/cooc_cases.py).  The counts are integers: every comparison is equality.

Shapes are the smallest at which the two kernels can go wrong: rows around the 32-row tile and the 64-word step of a counting
wave, 4200 rows (past a wave's 1024 words and a workgroup's 4096), rows shorter and longer than the 8 and 64 lanes that share
one (both instantiations of k_cooc_masks: mean row length below and above 64), groups of 1, 2, 31 and 32 words and the borders
10 | 11, 15 | 16, 22 | 23 between the instantiations of k_cooc_count, 1, 2, 64 and 65 groups, one column, a word shared by every
group, empty slots, and the one size at which a second row chunk appears: 16385 rows at RRI_MAX_K groups."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import cooc_cases as cc
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


@pytest.fixture(scope='module')
def eng():
    e = engine(4, 4, 2, dtype=np.float64)         # no X, W or T: the handle gives the device and the stream
    yield e
    e.close()


def check(e, A, words):
    A = sp.csr_matrix(A)
    df, codf = e.cooccurrence_counts(A, words)
    want_df, want_codf = cc.dense_counts(A.toarray(), words)
    assert df.dtype == np.int64 and codf.dtype == np.int64
    assert df.shape == want_df.shape and codf.shape == want_codf.shape
    assert np.array_equal(codf, want_codf), np.argwhere(codf != want_codf)[:5]
    assert np.array_equal(df, want_df)
    return df, codf


def random_corpus(n_rows, n_cols, density, seed):
    B = np.random.RandomState(seed).rand(n_rows, n_cols) < density
    B[::5] = False                                 # empty rows
    return sp.csr_matrix(B.astype(np.float64))


@pytest.mark.parametrize('n_rows', [1, 63, 64, 65, 257])
def test_row_counts_around_the_tile_and_the_counting_step(eng, n_rows):
    for n_cols, M in ((33, 5), (1, 1), (1, 2)):
        A = random_corpus(n_rows, n_cols, 0.4, n_rows)
        if n_rows > 1:
            A = sp.vstack([A[:-1], sp.csr_matrix(np.ones((1, n_cols)))]).tocsr()      # the last row counts
        check(eng, A, cc.random_words(3, M, n_cols, seed=1))


@pytest.mark.parametrize('lengths', [[0, 1, 8, 9, 64, 65, 300, 0, 2, 17] * 4 + [1], [300, 64, 65, 300, 1, 0, 8, 9, 300, 300] * 4],
                         ids=['8-lanes-per-row', 'a-wave-per-row'])
def test_row_lengths_on_both_sides_of_the_lane_groups(eng, lengths):
    from rri_nmf_amd import _capi
    A = cc.corpus_with_row_lengths(lengths, 400, seed=3)
    assert (A.nnz // A.shape[0] >= 64) == (lengths[0] == 300)           # which instantiation of k_cooc_masks this takes
    for M in (1, 2, 31, 32):
        df, _ = check(eng, A, cc.random_words(7, M, 400, seed=M, empty=0.1))
        assert df.max() > 0
    assert _capi.RRI_MAX_COOC_WORDS == 32


def test_group_sizes_and_group_counts(eng):
    A = random_corpus(130, 33, 0.3, 7)
    for M in (1, 2, 31, 32):
        for g in (1, 2, 64, 65):
            check(eng, A, cc.random_words(g, M, 33, seed=100 * M + g))
    # the borders between the instantiations of k_cooc_count (1, 2, 4, 9 pairs per lane), at more rows than a wave's 1024 words
    # and a workgroup's 4096
    B = random_corpus(4200, 33, 0.5, 8)
    for M in (10, 11, 15, 16, 22, 23, 32):
        df, codf = check(eng, B, cc.random_words(3, M, 33, seed=M))
        assert codf.min() > 0


def test_shared_words_empty_slots_and_words_in_no_and_in_every_document(eng):
    B = (np.random.RandomState(11).rand(97, 20) < 0.35).astype(np.float64)
    B[:, 0] = 1.0                                   # in every document
    B[:, 1] = 0.0                                   # in none
    words = cc.random_words(65, 6, 18, seed=5) + 2
    words[:, 0] = 0                                 # a word shared by all groups ...
    words[:, 3] = 1                                 # ... and one that never occurs
    words[3, 0] = words[3, 1] = -1                  # empty slots at the front
    words[4, 2] = words[4, 4] = -1                  # and in the middle
    words[5] = -1                                   # a group made only of empty slots
    df, codf = check(eng, B, words)
    assert np.all(df[[0, 1, 2], 0] == 97) and np.all(df[[0, 1, 2], 3] == 0) and np.all(df[5] == 0) and np.all(codf[5] == 0)
    assert np.all(codf[3, :2] == 0) and np.all(codf[3, :, :2] == 0) and np.all(codf[4, 2] == 0) and np.all(codf[4, :, 4] == 0)
    assert np.array_equal(codf, codf.transpose(0, 2, 1))
    assert np.array_equal(codf[np.arange(65)[:, None], np.arange(6), np.arange(6)], df)
    # every slot empty: nothing is launched and everything is 0
    df0, codf0 = check(eng, B, np.full((2, 3), -1))
    assert not df0.any() and not codf0.any()


def test_an_empty_corpus_launches_nothing(eng):
    eng.timing_enable(True)
    eng.timing_read(6)
    words = np.array([[0, 2, 1]])
    for A in (sp.csr_matrix((5, 7)), sp.csr_matrix((0, 7)), sp.csr_matrix(([0.0, 0.0], ([1, 3], [2, 2])), shape=(5, 7))):
        df, codf = check(eng, A, words)
        assert not df.any() and not codf.any()
    assert eng.timing_read(6)[0] == 0
    eng.timing_enable(False)


def test_the_smallest_corpus_with_a_second_row_chunk(eng):
    """64 MiB of masks at 4 bytes per row and group: 16384 rows at RRI_MAX_K = 1024 groups, so row 16384 is alone in the second chunk"""
    from rri_nmf_amd import _capi
    n_rows, n_cols, g = 16385, 64, _capi.RRI_MAX_K
    A = cc.corpus_with_row_lengths([3] * (n_rows - 1) + [n_cols], n_cols, seed=9)
    words = cc.random_words(g, 2, n_cols, seed=2)
    eng.timing_enable(True)
    eng.timing_read(6)
    df, codf = check(eng, A, words)
    assert eng.timing_read(6)[0] == 4                # two launches per chunk, two chunks
    eng.timing_enable(False)
    without_last = cc.dense_counts(A[:-1].toarray(), words)[1]
    assert np.array_equal(codf - without_last, (words[:, :, None] >= 0) & (words[:, None, :] >= 0))     # the second chunk's one row


def test_two_calls_give_the_same_bits_and_the_callers_matrix_stays_as_it_is(eng):
    A = random_corpus(300, 50, 0.2, 21)
    A.data[::7] = 0.0                                # explicit zeros are no occurrences
    assert A.indptr[2] - A.indptr[1] > 1
    A.indices[A.indptr[1]:A.indptr[2]] = A.indices[A.indptr[1]:A.indptr[2]][::-1].copy()         # an unsorted row
    A.has_sorted_indices = False
    keep = (A.indptr.copy(), A.indices.copy(), A.data.copy())
    words = cc.random_words(9, 10, 50, seed=3)
    a = check(eng, A, words)
    b = eng.cooccurrence_counts(A, words.tolist())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(x, y) for x, y in zip(keep, (A.indptr, A.indices, A.data)))
    with pytest.raises(ValueError, match='twice'):
        eng.cooccurrence_counts(A, [[1, 2, 1]])
    with pytest.raises(ValueError, match='out of range'):
        eng.cooccurrence_counts(A, [[1, 50]])
    with pytest.raises(NotImplementedError, match='group_size'):
        eng.cooccurrence_counts(A, np.arange(33)[None, :])
    with pytest.raises(NotImplementedError, match='n_groups'):
        eng.cooccurrence_counts(A, np.zeros((1025, 1)))
    I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    ptr, ind, w = np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([0], dtype=np.int32)
    out = np.zeros(1, dtype=np.int64)
    from rri_nmf_amd import _capi
    args = (eng._h, ptr.ctypes.data_as(I64P), ind.ctypes.data_as(I32P), 1, 1, w.ctypes.data_as(I32P), 1, 1)
    assert eng._lib.rri_cooccurrence_counts(*args, None, out.ctypes.data_as(I64P)) == _capi.RRI_ERR_INVALID
    assert eng._lib.rri_cooccurrence_counts(*args, out.ctypes.data_as(I64P), None) == _capi.RRI_ERR_INVALID
    assert eng._lib.rri_cooccurrence_counts(*args, out.ctypes.data_as(I64P), out.ctypes.data_as(I64P)) == _capi.RRI_OK and out[0] == 1


_answers = {}


@pytest.mark.parametrize('flavour', ['float32-dense', 'csr-x', 'weighted'])
def test_every_flavour_answers_the_same_and_no_state_of_a_run_is_disturbed(flavour):
    from rri_nmf_amd.engine import device_memory
    n, d, k = 50, 30, 3
    X = planted_X(n, d, k, seed=0, dtype=np.float64)
    X = X * (np.random.RandomState(4).rand(n, d) < 0.5)
    X[:, 0] = X.max()                                # no empty row
    W0, T0 = scaled_init(X, k, seed=1)
    A = random_corpus(200, 45, 0.3, 31)              # not the handle's shape
    words = cc.random_words(6, 10, 45, seed=8, empty=0.1)

    def run(with_call):
        if flavour == 'float32-dense':
            e = engine(n, d, k, dtype=np.float32)
            e.upload_X(X.astype(np.float32))
        elif flavour == 'csr-x':
            e = engine(n, d, k, dtype=np.float64, sparse_x=True)
            e.upload_X_csr(sp.csr_matrix(X))
        else:
            e = engine(n, d, k, dtype=np.float64, weighted=True)
            e.upload_X(X), e.upload_mask((np.random.RandomState(5).rand(n, d) < 0.6).astype(np.float64))
        try:
            e.set_W(W0), e.set_T(T0)
            e.set_params(reset_topic_method=None)
            e.sweep(1)
            if with_call:
                before = device_memory()
                e.timing_enable(True)
                got = check(e, A, words)
                assert e.timing_read(6)[0] == 2 and e.timing_read(6)[0] == 0
                e.timing_enable(False)
                assert device_memory() == before
                first = _answers.setdefault('counts', got)
                assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
            e.sweep(1)
            return e.get_W(), e.get_T(), e.objective()
        finally:
            e.close()
    Wa, Ta, oa = run(False)
    Wb, Tb, ob = run(True)
    assert np.array_equal(Wa.view(np.uint64), Wb.view(np.uint64)) and np.array_equal(Ta.view(np.uint64), Tb.view(np.uint64))
    assert np.float64(oa).view(np.uint64) == np.float64(ob).view(np.uint64)


def test_coherence_of_a_fitted_topic_model_end_to_end():
    from rri_nmf_amd import sklearn_interface as si
    n, d, k = 150, 40, 4
    X = planted_X(n, d, k, seed=2, dtype=np.float64)
    X = X * (X > np.percentile(X, 60))               # a document holds the words its planted topics weigh most
    E = si.NMF_TM_Estimator(n, d, k, random_state=0, max_iter=5).fit(X)
    held = X[::2][:61]                               # a reference corpus of another size
    for n_words in (5, 10):
        words = E.top_words(n_words)
        df, codf = cc.dense_counts(held, words)
        for measure in ('umass', 'pmi', 'npmi'):
            for corpus in (sp.csr_matrix(held), held):
                got = E.coherence(corpus, n_words=n_words, measure=measure, eps=1.0)
                per, undefined = cc.measure_reference(measure, words, df, codf, 61, 1.0)
                assert np.array_equal(got['words'], words) and np.array_equal(got['df'], df) and np.array_equal(got['codf'], codf)
                assert got['documents'] == 61 and np.array_equal(got['pairs_undefined'], undefined)
                assert np.allclose(got['per_topic'], per, rtol=1e-12, atol=1e-12, equal_nan=True)
                assert np.isfinite(got['mean']) and abs(got['mean'] - np.nanmean(per)) <= 1e-12
                used = words[words >= 0]
                assert got['diversity'] == np.unique(used).size / used.size
    # words= overrides the top words
    mine = np.array([[0, 1, -1, 2], [3, 0, 4, -1]])
    got = E.coherence(sp.csr_matrix(held), measure='umass', words=mine)
    df, codf = cc.dense_counts(held, mine)
    assert np.array_equal(got['codf'], codf)
    assert np.allclose(got['per_topic'], cc.measure_reference('umass', mine, df, codf, 61, 1.0)[0], rtol=1e-12, atol=1e-12, equal_nan=True)
