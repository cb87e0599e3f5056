"""Corpora derived from a resident corpus on the GPU: DeviceCorpus.take_rows / select_words / document_frequency / prune_words /
split_counts (include/rri_corpus_ops.h).

A selection is held against the DeviceCorpus of scipy's A[rows][:, keep], array for array and info field for info field; the
column counts against scipy; a split against the numpy restatement of the generator (tests/derive_cases.py), exactly.  The source
has rows of 0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257 entries (a wave's stride and its multiples), 1023, 1024, 1025, 2047,
2048, 2049 (both sides of the piece length, the one border at which the kernels take another path: a row's second and third
piece) and d = 3000 (a full row).  Every refusal exercised here is an argument or value check that returns a status."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import derive_cases as dc

pytestmark = pytest.mark.gpu

INFO = ('shape', 'nnz', 'stored', 'rows_rewritten', 'duplicates_merged', 'zeros_dropped', 'negatives', 'device_bytes', 'long_rows')


def DeviceCorpus(*a, **kw):
    from rri_nmf_amd.engine import DeviceCorpus as D
    return D(*a, **kw)


def memory():
    from rri_nmf_amd.engine import corpus_memory, device_memory
    return corpus_memory(), device_memory()


def bits(x):
    return np.asarray(x).view(np.uint64) if np.asarray(x).dtype == np.float64 else np.asarray(x)


def same(A, B):
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(bits(np.asarray(A.data, dtype=np.float64)), bits(np.asarray(B.data, dtype=np.float64))))


def canonical(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


@pytest.fixture(scope='module')
def counts():
    """the source of most tests: whole counts 1 .. 9, column 7 in every row that has an entry"""
    A = dc.count_corpus(dc.GPU_LENGTHS, dc.GPU_D, seed=1, always=7)
    assert A.shape == (40, 3000) and {0, 1, 63, 64, 65, dc.PIECE - 1, dc.PIECE, dc.PIECE + 1, 2 * dc.PIECE + 1, dc.GPU_D} <= set(dc.GPU_LENGTHS)
    corpus = DeviceCorpus(A)
    yield A, corpus
    corpus.close()


def check_select(corpus, A, rows, keep):
    """corpus._select(rows, keep) against the DeviceCorpus of scipy's selection: arrays and info"""
    want = A if rows is None else A[rows]
    want = canonical(want if keep is None else want[:, keep])
    before = memory()
    got = corpus._select(None if rows is None else np.asarray(rows, dtype=np.int64), None if keep is None else np.asarray(keep, dtype=np.int32))
    try:
        with DeviceCorpus(want) as ref:
            assert same(got.to_scipy(), want) and same(ref.to_scipy(), want)
            assert {key: getattr(got, key) for key in INFO} == {key: getattr(ref, key) for key in INFO}
        assert got.stored == got.nnz == want.nnz and got.ingest_ms >= 0 and got.device == corpus.device
        assert memory()[0] == (before[0][0] + 1, before[0][1] + got.device_bytes) and memory()[1] == before[1]
    finally:
        got.close()
    assert memory() == before
    return want


ROWS = {'all': None, 'none': [], 'reversed': list(range(39, -1, -1)), 'repeats': [14, 3, 14, 0, 12, 13, 13, 39, 16, 17, 18, 2, 14],
        'one_row_100_times': [12] * 100}


@pytest.mark.parametrize('which', sorted(ROWS))
def test_select_against_the_corpus_of_scipys_selection(counts, which):
    A, corpus = counts
    d = A.shape[1]
    first_only = np.setdiff1d(np.arange(d), A[dc.GPU_LENGTHS.index(63)].indices)        # empties some rows, not all
    keeps = {'all': None, 'none': [], 'every': np.arange(d), 'first': [0], 'last': [d - 1], 'every_other': np.arange(0, d, 2),
             'empties_some_rows': first_only, 'the_shared_column': [7]}
    for name, keep in keeps.items():
        want = check_select(corpus, A, ROWS[which], keep)
        if name == 'empties_some_rows' and which == 'all':
            empty = np.diff(want.indptr) == 0
            assert empty[dc.GPU_LENGTHS.index(63)] and not empty.all() and empty.sum() > dc.GPU_LENGTHS.count(0)
    # a keep that empties all rows: the columns nobody uses, of the source without its full row
    B = A[np.array(dc.GPU_LENGTHS) != d]
    unused = np.flatnonzero(np.asarray((B != 0).sum(0)).ravel() == 0)
    assert unused.size > 1 and B.shape[0] == 39
    with DeviceCorpus(B) as without:
        want = check_select(without, B, None if ROWS[which] is None else [min(r, 38) for r in ROWS[which]], unused)
        assert want.nnz == 0 and want.shape[1] == unused.size
        df = without.document_frequency()
        assert np.array_equal(df, np.asarray((B != 0).sum(0)).ravel()) and (df[unused] == 0).all()       # columns nobody uses
    assert same(corpus.to_scipy(), A)                           # the source is what it was


def test_select_of_sources_without_rows_without_entries_and_with_negative_values():
    for empty in (sp.csr_matrix((0, 5)), sp.csr_matrix((4, 5))):
        with DeviceCorpus(empty) as c:
            check_select(c, empty, None, None)
            check_select(c, empty, None, [1, 3])
            check_select(c, empty, [] if empty.shape[0] == 0 else [3, 3, 0], [0, 4])
            assert c.document_frequency().tolist() == [0] * 5
    A = dc.count_corpus([0, 5, 64, 65, dc.PIECE + 1, 300, 1], 1500, seed=2, negatives=True)
    assert (A.data < 0).any() and (A.data != np.floor(A.data)).all()
    with DeviceCorpus(A) as c:
        assert c.negatives == (A.data < 0).sum() > 0
        for rows, keep in ((None, None), ([4, 4, 1], None), (None, np.arange(0, 1500, 3)), ([6, 5, 4, 3, 2, 1, 0], np.arange(700, 1500))):
            want = check_select(c, A, rows, keep)
            with c._select(None if rows is None else np.array(rows), None if keep is None else np.asarray(keep, dtype=np.int32)) as got:
                assert got.negatives == (want.data < 0).sum()
        # a second run gives the same bytes
        runs = []
        for _ in range(2):
            with c._select(np.array([4, 2, 4, 5]), np.arange(1, 1500, 2, dtype=np.int32)) as got:
                runs.append(got.to_scipy())
        assert same(runs[0], runs[1])
        assert same(c.to_scipy(), A)


def test_the_public_calls_and_the_refusals_of_a_selection(counts):
    A, corpus = counts
    before = memory()
    with corpus.take_rows([5, 5, 0]) as t, corpus[3:30:4] as s, corpus[np.arange(40) % 7 == 0] as m, corpus[-1] as last:
        assert same(t.to_scipy(), A[[5, 5, 0]]) and same(s.to_scipy(), A[3:30:4]) and same(m.to_scipy(), A[np.arange(40) % 7 == 0])
        assert same(last.to_scipy(), A[39])
    mask = np.zeros(3000, dtype=bool)
    mask[[0, 7, 2999]] = True
    with corpus.select_words(mask) as w, corpus.select_words([7, 8, 9]) as w2:
        assert same(w.to_scipy(), canonical(A[:, [0, 7, 2999]])) and same(w2.to_scipy(), canonical(A[:, [7, 8, 9]]))
    for bad, text in (([0, 40], r'rows\[1\] = 40 is out of range'), ([-1], r'rows\[0\] = -1 is out of range')):
        with pytest.raises(ValueError, match=text):
            corpus.take_rows(bad)
    for bad, text in (([3, 3], r'keep\[1\] = 3 does not ascend strictly'), ([5, 2], r'keep\[1\] = 2 does not ascend strictly')):
        with pytest.raises(ValueError, match=text):
            corpus.select_words(bad)
    # the library's own refusals, through the entry point
    from rri_nmf_amd.engine import RRIEngine
    with RRIEngine(1, 1, 1, dtype=np.float64) as eng:
        lib, out = eng._lib, C.c_void_p(5)
        rows, keep = (C.c_int64 * 2)(0, 1), (C.c_int32 * 2)(0, 1)
        for args, text in (((corpus._ptr(), rows, -1, keep, 2), 'n_rows_out -1 is negative'), ((corpus._ptr(), rows, 2, keep, -3), 'n_cols_out -3 is negative'),
                           ((corpus._ptr(), None, 2, keep, 2), 'rows is NULL with a count of 2'), ((corpus._ptr(), rows, 2, None, 1), 'keep is NULL with a count of 1'),
                           ((None, rows, 2, keep, 2), 'the corpus is NULL or has been destroyed')):
            out.value = 5
            assert lib.rri_corpus_select(eng._h, *args, C.byref(out)) == -1 and not out.value and text in eng._err(), text
        assert lib.rri_corpus_select(eng._h, corpus._ptr(), rows, 2, keep, 2, None) == -1 and 'output pointer is NULL' in eng._err()
        assert lib.rri_corpus_column_counts(eng._h, None, None) == -1 and 'NULL or has been destroyed' in eng._err()
        assert lib.rri_corpus_column_counts(eng._h, corpus._ptr(), None) == -1 and 'output pointer is NULL' in eng._err()
        gone = DeviceCorpus(A[:3])
        ptr = C.c_void_p(gone._ptr().value)
        gone.close()
        assert lib.rri_corpus_select(eng._h, ptr, None, 0, None, 0, C.byref(out)) == -1 and 'destroyed' in eng._err() and not out.value
    corpus.device = 1                                   # what a corpus on another device looks like: refused before the library sees it
    try:
        with pytest.raises(Exception):
            corpus.take_rows([0])
    finally:
        corpus.device = 0
    assert memory() == before and same(corpus.to_scipy(), A)


def test_column_counts_against_scipy_and_prune_words(counts):
    A, corpus = counts
    before = memory()
    df = corpus.document_frequency()
    want = np.asarray((A != 0).sum(0)).ravel()
    assert df.dtype == np.int64 and np.array_equal(df, want)
    assert df.min() == 1 and df[7] == (np.diff(A.indptr) > 0).sum() == df.max()          # a column only the full row uses, one every row uses
    assert np.array_equal(corpus.document_frequency(), df)
    pruned, kept = corpus.prune_words(min_df=2, max_df=0.5, max_words=500)
    with pruned:
        from rri_nmf_amd.engine import DeviceCorpus as D
        assert np.array_equal(kept, D._prune_selection(want, 40, 2, 0.5, 500)) and kept.size == 500 and np.all(np.diff(kept) > 0)
        assert 7 not in kept and same(pruned.to_scipy(), canonical(A[:, kept])) and pruned.shape == (40, 500)
    nothing, kept = corpus.prune_words(min_df=41)
    with nothing:
        assert kept.size == 0 and nothing.shape == (40, 0) and nothing.nnz == 0
    assert memory() == before and same(corpus.to_scipy(), A)


@pytest.fixture(scope='module')
def wide_counts():
    """counts 1 .. 9, both sides of SPLIT_LANE_MAX, a multiple of 256 and 2^20, planted in rows of every length"""
    A = dc.count_corpus(dc.GPU_LENGTHS, dc.GPU_D, seed=3)
    planted = [dc.LANE_MAX - 1, dc.LANE_MAX, dc.LANE_MAX + 1, 512, 1000, dc.COUNT_MAX, 4 * dc.LANE_MAX, 257]
    at = np.linspace(0, A.nnz - 1, 5 * len(planted)).astype(np.int64)
    A.data[at] = np.tile(planted, 5)
    A.data[A.indptr[dc.GPU_LENGTHS.index(65)]:A.indptr[dc.GPU_LENGTHS.index(65)] + 3] = [dc.LANE_MAX + 1, 300, 2]    # two large ones in one stride
    assert set(range(1, 10)) <= set(A.data.astype(np.int64).tolist())
    return A


def test_split_against_the_restatement_exactly(wide_counts):
    A = wide_counts
    before = memory()
    with DeviceCorpus(A) as corpus:
        made = {}
        for held_out, seed in ((0.5, 12345), (0.5, 12346), (0.3, (9 << 32) | 5)):
            thr = dc.threshold(held_out)
            want_o, want_h = dc.split(A, thr, seed)
            mid = memory()
            observed, held = corpus.split_counts(held_out=held_out, random_state=seed)
            with observed, held:
                got_o, got_h = observed.to_scipy(), held.to_scipy()
                assert same(got_o, want_o) and same(got_h, want_h), (held_out, seed)
                assert same(canonical(got_o + got_h), A) and (got_o.data > 0).all() and (got_h.data > 0).all()
                for part, want in ((observed, want_o), (held, want_h)):
                    with DeviceCorpus(want) as ref:
                        assert {key: getattr(part, key) for key in INFO} == {key: getattr(ref, key) for key in INFO}
                    assert part.shape == A.shape and part.ingest_ms > 0
                assert memory()[0] == (mid[0][0] + 2, mid[0][1] + observed.device_bytes + held.device_bytes) and memory()[1] == mid[1]
            assert memory() == mid
            made[(held_out, seed)] = got_h
        assert not same(made[(0.5, 12345)], made[(0.5, 12346)])                 # two seeds differ
        # the same split from a shuffled raw matrix with duplicates as from the canonical one: it depends on (row, column, count, seed)
        rng = np.random.RandomState(4)
        first = np.where(A.data > 1, np.floor(A.data / 2), A.data)
        rest = A.data - first
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        r2, c2, v2 = (np.concatenate([a, a[rest > 0]]) for a in (rows, A.indices, first))
        v2[A.nnz:] = rest[rest > 0]
        order = np.lexsort((rng.rand(r2.size), r2))                            # shuffled inside every row
        raw_ptr = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=A.shape[0]))])
        from rri_nmf_amd.engine import DeviceCorpus as D
        from rri_nmf_amd import sklearn_interface as si
        with D.from_arrays(raw_ptr, c2[order], v2[order], A.shape) as shuffled:
            assert shuffled.duplicates_merged == (rest > 0).sum() > 0 and shuffled.rows_rewritten > 0 and same(shuffled.to_scipy(), A)
            observed, held = si.split_counts(shuffled, held_out=0.5, random_state=12345)            # the public dispatch
            with observed, held:
                assert same(held.to_scipy(), made[(0.5, 12345)])
        # a RandomState supplies two 32-bit words
        lo, hi = (int(v) for v in np.random.RandomState(8).randint(0, 1 << 32, size=2, dtype=np.uint64))
        observed, held = corpus.split_counts(held_out=0.5, random_state=np.random.RandomState(8))
        with observed, held:
            assert same(held.to_scipy(), dc.split(A, 1 << 31, lo | (hi << 32))[1])
        assert same(corpus.to_scipy(), A)
    assert memory() == before


def test_split_of_corpora_without_rows_and_without_entries():
    for empty in (sp.csr_matrix((0, 5)), sp.csr_matrix((4, 5))):
        with DeviceCorpus(empty) as c:
            observed, held = c.split_counts(0.5, 1)
            with observed, held:
                assert observed.shape == held.shape == empty.shape and observed.nnz == held.nnz == 0
                assert same(observed.to_scipy(), empty) and same(held.to_scipy(), empty)


@pytest.mark.parametrize('name,values,kind,text', [
    ('too_large', {5000: dc.COUNT_MAX + 1.0, 9000: 2.0 ** 21}, NotImplementedError, 'value 1048577 at entry 5000 is above 1048576, the largest count that is split'),
    ('half', {9000: 0.5, 70: 2.5}, ValueError, 'value 2.5 at entry 70 is not a whole number: a split takes counts'),
    ('negative', {8191: -1.0, 8192: -1.0}, ValueError, 'value -1 at entry 8191 is negative: a split takes counts'),
    ('two_rules', {100: dc.COUNT_MAX + 1.0, 9500: 0.25, 9600: -3.0, 9700: -4.0}, ValueError, 'value -3 at entry 9600 is negative: a split takes counts'),
    ('two_rules_the_second', {100: dc.COUNT_MAX + 1.0, 9500: 0.25}, ValueError, 'value 0.25 at entry 9500 is not a whole number: a split takes counts'),
])
def test_a_split_of_values_that_are_no_counts_is_refused_and_nothing_is_kept(counts, name, values, kind, text):
    A = counts[0].copy()
    for at, v in values.items():
        A.data[at] = v
    assert dc.check_values(A.data)[1] == text and A.nnz > 9700
    with DeviceCorpus(A) as c:
        before = memory()
        for _ in range(2):
            with pytest.raises(kind) as e:
                c.split_counts(0.5, 3)
            assert str(e.value) == text
        # through the entry point: the outputs are NULL
        from rri_nmf_amd.engine import RRIEngine
        with RRIEngine(1, 1, 1, dtype=np.float64) as eng:
            observed, held = C.c_void_p(5), C.c_void_p(6)
            st = eng._lib.rri_corpus_split(eng._h, c._ptr(), 1 << 31, 3, C.byref(observed), C.byref(held))
            assert st == (-3 if kind is NotImplementedError else -1) and not observed.value and not held.value and eng._err() == text
            st = eng._lib.rri_corpus_split(eng._h, c._ptr(), 0, 3, C.byref(observed), C.byref(held))
            assert st == -1 and 'threshold 0' in eng._err()
            assert eng._lib.rri_corpus_split(eng._h, c._ptr(), 5, 3, None, C.byref(held)) == -1 and 'output pointer is NULL' in eng._err()
        assert memory() == before and same(c.to_scipy(), A)
        for bad in (0.0, 1.0, 2.0 ** -33):
            with pytest.raises(ValueError, match='held_out'):
                c.split_counts(bad)


def test_a_handle_that_lends_itself_to_the_three_calls_sweeps_as_its_twin(counts):
    """two equal engines sweep side by side; between two sweeps one lends its handle to all three calls: W, T and the objective
    stay bit-equal -- the calls keep and touch nothing of a handle's state"""
    from rri_nmf_amd.engine import RRIEngine
    A, corpus = counts
    import frozen_cases as fc
    n, d, k = 96, 80, 5
    _, _, X, W0, T0, flags = fc.make_case(1, n, d, k, seed=6, flavour='tm')       # planted factors: every topic stays alive
    engines = []
    for _ in range(2):
        eng = RRIEngine(n, d, k, dtype=np.float64)
        eng.upload_X(X)
        eng.set_W(W0)
        eng.set_T(T0)
        eng.set_params(reset_topic_method='max_resid_document', n_resets=23, **flags)
        engines.append(eng)
    a, b = engines
    try:
        for step in range(3):
            a.sweep(1)
            b.sweep(1)
            mem = memory()
            out, obs, held = C.c_void_p(), C.c_void_p(), C.c_void_p()
            rows, keep, df = (C.c_int64 * 3)(39, 14, 14), (C.c_int32 * 3)(0, 7, 2999), np.zeros(A.shape[1], dtype=np.int64)
            assert a._lib.rri_corpus_select(a._h, corpus._ptr(), rows, 3, keep, 3, C.byref(out)) == 0
            assert a._lib.rri_corpus_column_counts(a._h, corpus._ptr(), df.ctypes.data_as(C.POINTER(C.c_int64))) == 0
            assert a._lib.rri_corpus_split(a._h, corpus._ptr(), 1 << 31, step, C.byref(obs), C.byref(held)) == 0
            assert a._lib.rri_corpus_select(a._h, corpus._ptr(), rows, 3, keep, -1, C.byref(C.c_void_p())) == -1          # and a refusal
            assert memory()[1] == mem[1] and memory()[0][0] == mem[0][0] + 3
            info = (C.c_int64 * 10)()
            a._lib.rri_corpus_info(out, info, 10, None)
            assert list(info)[:2] == [3, 3] and df[7] == (np.diff(A.indptr) > 0).sum()
            for ptr in (out, obs, held):
                assert a._lib.rri_corpus_destroy(ptr) == 0
            assert memory() == mem
            assert np.array_equal(bits(a.get_W()), bits(b.get_W())) and np.array_equal(bits(a.get_T()), bits(b.get_T()))
            assert a.objective() == b.objective()
    finally:
        a.close()
        b.close()


@pytest.fixture(scope='module')
def chain():
    """ingest -> prune words -> split rows into train and test -> split the test counts: all on the device"""
    A = dc.count_corpus([25 + (q * 7) % 40 for q in range(60)], 400, seed=7, top=6)
    corpus = DeviceCorpus(A)
    pruned, kept = corpus.prune_words(min_df=2, max_df=0.9, max_words=300)
    train, test = pruned[:40], pruned[40:]
    observed, held = test.split_counts(held_out=0.5, random_state=12345)
    yield A, kept, pruned, train, test, observed, held
    for c in (corpus, pruned, train, test, observed, held):
        c.close()


def test_the_chain_fits_and_scores_without_a_download(chain, monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    from rri_nmf_amd.engine import DeviceCorpus as D
    A, kept, pruned, train, test, observed, held = chain
    host = {name: c.to_scipy() for name, c in (('train', train), ('observed', observed), ('held', held))}
    Ap = canonical(A[:, kept])
    assert same(host['train'], Ap[:40]) and same(canonical(host['observed'] + host['held']), Ap[40:]) and 250 <= kept.size <= 300
    assert (np.diff(host['observed'].indptr) > 0).all() and (np.diff(host['held'].indptr) > 0).all()

    def no_download(self):
        raise AssertionError('the corpus was downloaded')
    n, d, k = train.shape[0], train.shape[1], 4
    with monkeypatch.context() as m:
        m.setattr(D, 'to_scipy', no_download)
        E = si.NMF_TM_Estimator(n, d, k, max_iter=4, nmf_kwargs={'sparse_X': True})
        E.fit(train)
        Wo = E.transform(observed)
        got = E.log_likelihood(held, W=Wo)
    with DeviceCorpus(host['train']) as rt, DeviceCorpus(host['observed']) as ro, DeviceCorpus(host['held']) as rh:
        R = si.NMF_TM_Estimator(n, d, k, max_iter=4, nmf_kwargs={'sparse_X': True})
        R.fit(rt)
        assert np.array_equal(bits(E.W), bits(R.W)) and np.array_equal(bits(E.T), bits(R.T))
        Wr = R.transform(ro)
        assert np.array_equal(bits(Wo), bits(Wr))
        want = R.log_likelihood(rh, W=Wr)
    assert all(np.array_equal(bits(got[key]), bits(want[key])) for key in ('per_document', 'tokens', 'floored'))
    assert got['perplexity'] == want['perplexity'] and np.isfinite(got['perplexity']) and got['documents'] == 20
    assert np.array_equal(got['tokens'], np.asarray(host['held'].sum(1)).ravel())


def test_partial_fit_over_slices_of_a_corpus_is_partial_fit_over_corpora_of_the_slices(chain):
    from rri_nmf_amd import sklearn_interface as si
    A, kept, pruned, train, test, observed, held = chain
    Ap = pruned.to_scipy()
    n, d, k = 20, pruned.shape[1], 3
    made = []
    for batches in ([pruned[a:a + 20] for a in (0, 20, 40)], [DeviceCorpus(Ap[a:a + 20]) for a in (0, 20, 40)]):
        E = si.NMF_TM_Estimator(n, d, k, nmf_kwargs={'sparse_X': True})
        for batch in batches:
            E.partial_fit(batch, sweeps=2)
            batch.close()
        F = E.frozen_
        made.append((E.W, E.T, F.B, F.A, F.s, np.array([F.c, F.rows])))
    for a, b in zip(*made):
        assert np.array_equal(bits(a), bits(b))
    assert made[0][5][1] == 60
