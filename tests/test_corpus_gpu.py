"""DeviceCorpus on the GPU: a raw CSR matrix is checked and made canonical on the device, and the evaluation calls take it.

The canonical arrays are held against scipy's (sum_duplicates, eliminate_zeros, sort_indices) on integers, where every sum is
exact, and against the numpy restatement (tests/corpus_cases.py) where the order of a float64 sum shows; the counters against
the restatement.  The row lengths stand on both sides of every border at which the ingest takes another path -- B_wave = 64 (one
wave), every power of two up to B_lds = 16384 (the padded length of a workgroup's row in LDS) and B_lds + 1 (global memory).
Every malformed matrix of the CPU list is refused with the same text, from host arrays and from device tensors, and leaves the
counters where they were.  The two consumers are held bit for bit against the same call on the canonical scipy matrix, at the
sizes at which test_cooc_gpu.py and test_loglik_gpu.py reach their second chunk."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import cooc_cases as co
import corpus_cases as cc
import loglik_cases as lc

pytestmark = pytest.mark.gpu


def DeviceCorpus(*a, **kw):
    from rri_nmf_amd.engine import DeviceCorpus as D
    return D(*a, **kw)


def from_arrays(raw, **kw):
    from rri_nmf_amd.engine import DeviceCorpus as D
    return D.from_arrays(*raw, **kw)


def memory():
    from rri_nmf_amd.engine import corpus_memory, device_memory
    return corpus_memory(), device_memory()


STATS = ('rows_rewritten', 'duplicates_merged', 'zeros_dropped', 'negatives', 'long_rows')


def same_arrays(A, B):
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(np.asarray(A.data, dtype=np.float64).view(np.uint64), np.asarray(B.data, dtype=np.float64).view(np.uint64)))


def check_against_scipy(raw, stats=True):
    before = memory()
    with from_arrays(raw) as c:
        got = c.to_scipy()
        want = cc.scipy_canonical(*raw)
        assert same_arrays(got, want)
        assert got.data.dtype == np.float64 and sp.isspmatrix_csr(got) and got.has_sorted_indices      # (scipy picks the index dtype)
        assert c.shape == raw[3] and c.stored == len(raw[1]) and c.nnz == want.nnz
        assert c.stored == c.nnz + c.duplicates_merged + c.zeros_dropped
        assert c.device_bytes == 8 * max(c.shape[0] + 1, 1) + 12 * c.nnz or c.nnz == 0
        assert c.ingest_ms > 0
        if stats:
            st = cc.canonical(*raw)[3]
            assert {key: getattr(c, key) for key in STATS} == st
        assert memory()[0] == (before[0][0] + 1, before[0][1] + c.device_bytes) and memory()[1] == before[1]
        info = c
    assert memory() == before
    return info


BORDERS = [0, 1, 2, cc.WAVE_MAX - 1, cc.WAVE_MAX, cc.WAVE_MAX + 1]
POWERS = [p for p in (128, 256, 512, 1024, 2048, 4096, 8192) if cc.WAVE_MAX < p < cc.LDS_MAX]


@pytest.mark.parametrize('lengths', [BORDERS, [n for p in POWERS[:4] for n in (p - 1, p, p + 1)], [n for p in POWERS[4:] for n in (p - 1, p, p + 1)],
                                     [cc.LDS_MAX - 1, cc.LDS_MAX, 5]], ids=['wave', 'lds_small', 'lds_large', 'lds_full'])
def test_rows_on_both_sides_of_every_border_against_scipy(lengths):
    raw = cc.raw_rows(lengths, 12000, seed=len(lengths), zeros=0.05)
    c = check_against_scipy(raw)
    assert c.rows_rewritten >= len([n for n in lengths if n > 2]) and c.duplicates_merged > 0 and c.long_rows == 0
    assert c.zeros_dropped > 0 and c.negatives > 0


def test_one_row_beyond_lds_beside_a_few_short_ones():
    raw = cc.raw_rows([3, cc.LDS_MAX + 1, 0, 70], 12000, seed=3)
    c = check_against_scipy(raw)
    assert c.long_rows == 1 and c.rows_rewritten >= 3


def test_sorted_rows_with_duplicates_and_rows_of_one_column():
    """sorted input whose only fault are repeats, a row that is one column 300 times (one run for one thread), a row of zeros"""
    indptr, indices, values, shape = cc.raw_rows([40, 90, 300, 7], 500, seed=4, shuffle=False)
    indices[indptr[2]:indptr[3]] = 17
    values[indptr[3]:] = 0.0
    c = check_against_scipy((indptr, indices, values, shape))
    assert c.rows_rewritten == 4 and c.duplicates_merged >= 299 and c.zeros_dropped >= 1


def test_the_order_of_a_sum_is_the_stored_order():
    """(1e16 + 1) - 1e16 is 0 in float64 and the entry is dropped; (1e16 - 1e16) + 1 is 1: both sides add in the same order, so
    equality with the restatement is exact.  Once in a wave's row, once in a row of the LDS class, once beyond it."""
    for filler in (0, 100, cc.LDS_MAX):
        fill = np.arange(10, 10 + filler)
        rows = [np.concatenate([[7, 5], fill[::-1], [5, 5]]), np.concatenate([[5, 7, 5], fill[::-1], [5]])]
        vals = [np.concatenate([[2.0, 1e16], np.ones(filler), [1.0, -1e16]]), np.concatenate([[1e16, 2.0, -1e16], np.ones(filler), [1.0]])]
        raw = (np.array([0, rows[0].size, rows[0].size + rows[1].size]), np.concatenate(rows), np.concatenate(vals), (2, 20000))
        indptr, indices, values, st = cc.canonical(*raw)
        with from_arrays(raw) as c:
            got = c.to_scipy()
            assert np.array_equal(got.indptr, indptr) and np.array_equal(got.indices, indices)
            assert np.array_equal(got.data.view(np.uint64), values.view(np.uint64))
            assert got[0, 5] == 0.0 and got[1, 5] == 1.0 and got[0, 7] == got[1, 7] == 2.0
            assert c.zeros_dropped == st['zeros_dropped'] == 1 and c.duplicates_merged == 4 and c.long_rows == 2 * (filler == cc.LDS_MAX)


def test_input_types_give_one_corpus_and_two_ingests_the_same_bytes():
    rng = np.random.RandomState(6)
    A = sp.random(300, 200, density=0.1, format='csr', random_state=rng, data_rvs=lambda m: rng.randint(1, 9, size=m).astype(np.float64))
    assert A.has_canonical_format
    with DeviceCorpus(A) as c:                                 # canonical already: copied as it is
        assert c.rows_rewritten == c.duplicates_merged == c.zeros_dropped == c.negatives == 0 and c.nnz == c.stored == A.nnz
        assert same_arrays(c.to_scipy(), A)
    with from_arrays((A.indptr, A.indices, None, A.shape)) as c:          # a pattern: every stored entry is 1
        got = c.to_scipy()
        assert np.array_equal(got.indices, A.indices) and np.all(got.data == 1.0) and got.nnz == A.nnz
    raw = cc.raw_rows([0, 5, 64, 65, 700, 3], 900, seed=7, zeros=0.1)
    base = from_arrays(raw).to_scipy()
    for pdt, idt, vdt in ((np.int32, np.int32, np.float32), (np.int32, np.int64, np.float64), (np.int64, np.int32, np.float32),
                          (np.int16, np.uint16, np.int64)):
        with from_arrays((raw[0].astype(pdt), raw[1].astype(idt), raw[2].astype(vdt), raw[3])) as c:
            assert same_arrays(c.to_scipy(), base), (pdt, idt, vdt)
    again = from_arrays(raw).to_scipy()
    assert same_arrays(again, base)
    # a scipy matrix that is not canonical, a COO matrix and a dense array
    M = sp.csr_matrix((raw[2], raw[1], raw[0]), shape=raw[3])
    dense = M.toarray()
    for X in (M, M.tocoo(), dense):
        with DeviceCorpus(X) as c:
            assert np.array_equal(c.to_scipy().toarray(), dense)
    for empty in (sp.csr_matrix((0, 5)), sp.csr_matrix((4, 5)), sp.csr_matrix((3, 0))):
        with DeviceCorpus(empty) as c:
            assert c.nnz == 0 and c.to_scipy().shape == empty.shape and c.to_scipy().nnz == 0


def test_from_device_memory_gives_the_corpus_of_the_host_route():
    import torch
    raw = cc.raw_rows([0, 5, 64, 65, 700, 3, cc.LDS_MAX + 1], 12000, seed=8, zeros=0.1)
    base = from_arrays(raw).to_scipy()
    from rri_nmf_amd.engine import DeviceCorpus as D
    before = memory()
    for pdt, idt, vdt in ((torch.int64, torch.int64, torch.float64), (torch.int32, torch.int32, torch.float32)):
        t = [torch.as_tensor(a).to('cuda', dtype=dt) for a, dt in zip(raw[:3], (pdt, idt, vdt))]
        with D.from_device(t[0], t[1], t[2], raw[3]) as c:
            assert same_arrays(c.to_scipy(), base) and c.long_rows == 1
        with D.from_device(t[0], t[1], None, raw[3]) as c:
            assert np.array_equal(c.to_scipy().toarray(), cc.scipy_canonical(raw[0], raw[1], None, raw[3]).toarray())
        assert np.array_equal(t[1].cpu().numpy(), raw[1]) and np.array_equal(t[0].cpu().numpy(), raw[0])       # read, not written
    A = cc.scipy_canonical(*raw)
    X = torch.sparse_csr_tensor(torch.as_tensor(A.indptr), torch.as_tensor(A.indices.astype(np.int64)), torch.as_tensor(A.data),
                                size=A.shape).to('cuda')
    with DeviceCorpus(X) as c:
        assert same_arrays(c.to_scipy(), base) and c.rows_rewritten == 0 and c.device == 0
    with pytest.raises(ValueError, match='GPU tensors'):
        D.from_device(torch.as_tensor(raw[0]), torch.as_tensor(raw[1]), None, raw[3])
    with pytest.raises(TypeError, match='values'):
        D.from_device(torch.as_tensor(raw[0]).cuda(), torch.as_tensor(raw[1]).cuda(), torch.as_tensor(raw[2]).cuda().half(), raw[3])
    assert memory() == before


@pytest.mark.parametrize('name', sorted(cc.MALFORMED))
def test_a_malformed_matrix_is_refused_with_its_text_and_nothing_is_kept(name):
    import torch
    from rri_nmf_amd.engine import DeviceCorpus as D
    indptr, indices, values, shape = cc.MALFORMED[name]
    kind = NotImplementedError if name.startswith('n_cols') else ValueError
    before = memory()
    with pytest.raises(kind) as e:
        from_arrays((np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int64), np.array(values), shape))
    assert str(e.value) == cc.TEXT[name]
    with pytest.raises(kind) as e:
        from_arrays((np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int32), np.array(values, dtype=np.float32), shape))
    assert str(e.value) == cc.TEXT[name]
    with pytest.raises(kind) as e:
        D.from_device(torch.tensor(indptr, dtype=torch.int64, device='cuda'), torch.tensor(indices, dtype=torch.int32, device='cuda'),
                      torch.tensor(values, dtype=torch.float64, device='cuda'), shape)
    assert str(e.value) == cc.TEXT[name]
    assert memory() == before


def test_a_large_malformed_matrix_names_the_smallest_position_whatever_workgroup_finds_it():
    raw = list(cc.raw_rows([50] * 4000, 3000, seed=9))
    raw[1] = raw[1].copy()
    raw[1][[150001, 77777, 199999]] = [3000, -4, 3001]
    before = memory()
    for _ in range(2):
        with pytest.raises(ValueError) as e:
            from_arrays(raw)
        assert str(e.value) == 'column -4 at entry 77777 is out of range' == cc.check(*raw)[1]
    assert memory() == before


def test_a_corpus_serves_a_second_handle_and_outlives_the_one_that_made_it():
    from rri_nmf_amd.engine import RRIEngine
    A = co.corpus_with_row_lengths([3, 0, 9, 20, 1], 30, seed=1)
    words = co.random_words(3, 4, 30, seed=2)
    before = memory()
    c = DeviceCorpus(A)                  # the handle that made it is closed by now
    with RRIEngine(4, 4, 2) as a, RRIEngine(7, 5, 3, dtype=np.float64, weighted=True) as b:
        mem = memory()[1]
        want = a.cooccurrence_counts(A, words)
        for eng in (a, b):
            got = eng.cooccurrence_counts(c, words)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert memory()[1] == mem
        c.device = 1                    # what a corpus on another device looks like to the engine
        with pytest.raises(ValueError, match='device 1'):
            a.cooccurrence_counts(c, words)
        c.device = 0
    c.close()
    c.close()
    with pytest.raises(ValueError, match='closed'):
        c.to_scipy()
    assert memory() == before


def test_cooccurrence_counts_of_a_corpus_at_the_second_row_chunk():
    from rri_nmf_amd import _capi
    from rri_nmf_amd.engine import RRIEngine
    n_rows, n_cols, g = 16385, 64, _capi.RRI_MAX_K
    A = co.corpus_with_row_lengths([3] * (n_rows - 1) + [n_cols], n_cols, seed=9)
    words = co.random_words(g, 2, n_cols, seed=2)
    raw = cc.raw_rows([40, 0, 64, 65, 3], n_cols, seed=10, duplicated=0.5, zeros=0.2)        # and a small one that is rewritten
    with RRIEngine(1, 1, 1, dtype=np.float64) as eng, DeviceCorpus(A) as c, from_arrays(raw) as small:
        mem = memory()
        eng.timing_enable(True)
        eng.timing_read(6)
        df, codf = eng.cooccurrence_counts(c, words)
        assert eng.timing_read(6)[0] == 4                # two launches per chunk, two chunks
        eng.timing_enable(False)
        want = eng.cooccurrence_counts(A, words)
        assert df.dtype == codf.dtype == np.int64 and np.array_equal(df, want[0]) and np.array_equal(codf, want[1])
        w2 = co.random_words(5, 6, n_cols, seed=3, empty=0.2)
        got, want = eng.cooccurrence_counts(small, w2), eng.cooccurrence_counts(sp.csr_matrix((raw[2], raw[1], raw[0]), shape=raw[3]), w2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[1], co.dense_counts(small.to_scipy().toarray(), w2)[1])
        with pytest.raises(ValueError, match='out of range'):
            eng.cooccurrence_counts(small, [[0, n_cols]])
        with pytest.raises(NotImplementedError, match='group_size'):
            eng.cooccurrence_counts(small, np.zeros((1, 33), dtype=np.int32) - 1)
        assert memory() == mem


def bits(x):
    return np.asarray(x).view(np.uint64) if np.asarray(x).dtype == np.float64 else np.asarray(x)


def test_entries_loglik_of_a_corpus_at_the_second_chunk_of_requests():
    from rri_nmf_amd.engine import RRIEngine
    n, d, k = 1366, 4096, 2
    assert (64 << 20) // 12 // d == n - 1
    W, T = lc.factors(n, d, k, seed=1, simplex=True)
    counts = np.random.RandomState(10).randint(1, 4, size=(n, d)).astype(np.float32)
    A = sp.csr_matrix(counts)
    with RRIEngine(n, d, k, dtype=np.float64) as eng, DeviceCorpus(A) as c:
        eng.set_W(W)
        eng.set_T(T)
        assert c.nnz == n * d and c.rows_rewritten == 0
        mem = memory()
        eng.timing_enable(True)
        eng.timing_read(7)
        got = eng.entries_loglik(None, c, 1e-12)
        assert eng.timing_read(7)[0] == 5                # the transposed copy of T, then two launches per chunk, two chunks
        eng.timing_enable(False)
        want = eng.entries_loglik(None, c.to_scipy(), 1e-12)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))
        assert np.array_equal(got[1], counts.sum(axis=1)) and np.all(got[0] < 0)
        assert memory() == mem


def test_entries_loglik_of_a_rewritten_corpus_rows_permuted_and_its_refusals():
    from rri_nmf_amd.engine import RRIEngine
    n, d, k = 9, 300, 5
    W, T = lc.disjoint_factors(n, d, k, seed=2)
    raw = list(cc.raw_rows([0, 5, 64, 65, 300, 257, 1, 90, 30], d, seed=11, duplicated=0.0, zeros=0.1))
    raw[2] = np.abs(raw[2])
    neg = list(raw)
    neg[2] = raw[2].copy()
    neg[2][np.flatnonzero(neg[2])[3]] *= -1.0
    with RRIEngine(n, d, k, dtype=np.float64) as eng, from_arrays(raw) as c, from_arrays(neg) as cneg:
        eng.set_W(W)
        eng.set_T(T)
        mem = memory()
        A = c.to_scipy()
        assert c.zeros_dropped > 0 and c.rows_rewritten >= 6 and c.negatives == 0 and cneg.negatives == 1
        for rows in (None, np.random.RandomState(3).permutation(n), np.array([4] * n)):
            for floor in (1e-12, 0.0):
                got, want = eng.entries_loglik(rows, c, floor), eng.entries_loglik(rows, A, floor)
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))
                ref = lc.reference(W, T, rows, A, floor)
                assert np.array_equal(got[2], ref[2]) and np.array_equal(got[1], ref[1])
        assert got[0].shape == (n,) and np.isneginf(got[0]).any()
        # negatives are refused by the log-likelihood alone; the counts take the same corpus
        with pytest.raises(ValueError, match='negative'):
            eng.entries_loglik(None, cneg, 1e-12)
        assert eng.cooccurrence_counts(cneg, [[0, 1, 2]])[0].shape == (1, 3)
        with pytest.raises(ValueError, match='floor'):
            eng.entries_loglik(None, c, -1.0)
        with pytest.raises(ValueError, match='out of range'):
            eng.entries_loglik(np.arange(n) + 1, c, 1e-12)
        with pytest.raises(ValueError, match='one row per requested row'):
            eng.entries_loglik(np.arange(3), c, 1e-12)
        with RRIEngine(n, d + 1, k, dtype=np.float64) as other:
            with pytest.raises(ValueError, match='d columns'):
                other.entries_loglik(None, c, 1e-12)
            out = (np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64))
            import ctypes as C
            st = other._lib.rri_corpus_entries_loglik(other._h, c._ptr(), None, 1e-12, out[0].ctypes.data_as(C.POINTER(C.c_double)),
                                                      out[1].ctypes.data_as(C.POINTER(C.c_double)), out[2].ctypes.data_as(C.POINTER(C.c_int64)))
            assert st == -1 and 'the corpus has 300 columns, W T has 301' in other._err()
        assert memory() == mem


def test_coherence_and_held_out_perplexity_of_the_text_fixture_with_a_corpus():
    from rri_nmf_amd import sklearn_interface as si
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g1_tm_estimator.npz'))
    X, Xte, W, T = z['X'], z['Xte'], z['W_s10'], z['T_s10']
    n, d, k = X.shape[0], X.shape[1], T.shape[0]
    E = si.NMF_TM_Estimator(n, d, k, W=W, T=T)
    before = memory()
    with DeviceCorpus(sp.csr_matrix(X)) as cx:
        for measure in ('umass', 'npmi'):
            got, want = E.coherence(cx, n_words=8, measure=measure), E.coherence(sp.csr_matrix(X), n_words=8, measure=measure)
            assert np.array_equal(got['df'], want['df']) and np.array_equal(got['codf'], want['codf'])
            assert np.array_equal(bits(got['per_topic']), bits(want['per_topic'])) and got['documents'] == want['documents'] == n
        a, b = E.log_likelihood(cx, W=W), E.log_likelihood(sp.csr_matrix(X), W=W)
        assert all(np.array_equal(bits(a[key]), bits(b[key])) for key in ('per_document', 'tokens', 'floored'))
        assert a['perplexity'] == b['perplexity'] and a['floored'].sum() == 1
    counts = sp.csr_matrix(np.round(40 * Xte))
    observed, held = si.split_counts(counts, held_out=0.5, random_state=0)
    with DeviceCorpus(held) as ch:
        done = E.perplexity(ch, observed=observed)
        assert done == E.perplexity(held, observed=observed) and np.isfinite(done) and 1 < done
        assert E.perplexity(ch) == E.perplexity(held)           # without observed: the fold-in runs on the downloaded corpus
    assert memory() == before
