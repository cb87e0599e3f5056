"""A corpus from (row, column, value) pairs and the split of a corpus by entry on the GPU: DeviceCorpus.from_pairs / split_entries
(include/rri_corpus_build.h).

The oracle of from_pairs is the merged code path: DeviceCorpus.from_arrays on the raw CSR matrix whose row i holds the pairs of
row i in the order given (a stable sort by row, made in numpy), compared array for array -- indptr, indices, the values' bits --
and info field for info field but for the device bytes and ingest_ms; the numpy restatement (tests/corpus_build_cases.py) is a
second oracle on the small lists.  The split is held against the restatement of the generator, exactly.  The lists have rows of
0, 1, 2, 63, 64, 65 (a wave), 127, 128, 129 (the shortest pad), 16384 and 16385 pairs (the LDS and the global class) and 0, 1,
63, 64, 65, 255, 256, 257, 262143, 262144, 262145 pairs in all (a wave, a workgroup and the full grid of a pass over the pairs).
Every refusal exercised here is an argument or value check that returns a status."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import corpus_build_cases as cb
import derive_cases as dc

pytestmark = pytest.mark.gpu

INFO = ('shape', 'nnz', 'stored', 'rows_rewritten', 'duplicates_merged', 'zeros_dropped', 'negatives', 'long_rows')


def D():
    from rri_nmf_amd.engine import DeviceCorpus
    return DeviceCorpus


def memory():
    from rri_nmf_amd.engine import corpus_memory, device_memory
    return corpus_memory(), device_memory()


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same(A, B):
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(bits(A.data), bits(B.data)))


def arrays(c):
    A = c.to_scipy()
    return A.indptr.astype(np.int64).tobytes(), A.indices.astype(np.int32).tobytes(), bits(A.data).tobytes()


def oracle(rows, cols, values, shape):
    """the merged path: from_arrays on the stable-by-row raw CSR; (arrays, info)"""
    indptr, indices, vals = cb.raw_csr(rows, cols, values, shape)
    with D().from_arrays(indptr, indices, vals, shape) as ref:
        return arrays(ref), {key: getattr(ref, key) for key in INFO}


def check_list(rows, cols, values, shape, restate=False, **kw):
    """from_pairs(rows, cols=cols) against the oracle (and the restatement); returns the arrays"""
    before = memory()
    want, info = oracle(rows, cols, values, shape)
    got = D().from_pairs(rows, values, shape=shape, cols=cols, **kw)
    try:
        mine = arrays(got)
        assert mine == want
        assert {key: getattr(got, key) for key in INFO} == info
        assert got.stored == len(rows) and got.ingest_ms >= 0 and got.device_bytes > 0
        assert memory()[0] == (before[0][0] + 1, before[0][1] + got.device_bytes) and memory()[1] == before[1]
        if restate:
            ptr, idx, val, st = cb.from_pairs(rows, cols, values, shape)
            assert mine == (ptr.tobytes(), idx.tobytes(), bits(val).tobytes())
            assert {key: getattr(got, key) for key in cb.INFO} == st
    finally:
        got.close()
    assert memory() == before
    return mine, info


@pytest.fixture(scope='module')
def edges():
    return cb.edge_list()


@pytest.mark.parametrize('order', ['as_sorted', 'reversed', 'shuffled'])
def test_rows_on_both_sides_of_every_class_border(edges, order):
    rows, cols, values, shape = edges
    lengths = set(np.bincount(rows, minlength=shape[0]).tolist())
    assert set(cb.EDGE_LENGTHS) <= lengths and rows.size < 100000 and rows.min() > 0 and rows.max() == shape[0] - 1 and cols.max() == shape[1] - 1
    perm = {'as_sorted': np.arange(rows.size), 'reversed': np.arange(rows.size)[::-1], 'shuffled': np.random.RandomState(3).permutation(rows.size)}[order]
    r, c, v = rows[perm].copy(), cols[perm].copy(), values[perm].copy()
    mine, info = check_list(r, c, v, shape)
    if order == 'as_sorted':
        assert info['rows_rewritten'] == 0 and info['long_rows'] == 0 and info['duplicates_merged'] == 0 and info['nnz'] == rows.size
    else:
        assert info['long_rows'] == 1 and info['duplicates_merged'] == 0 and info['nnz'] == rows.size
        if order == 'reversed':         # every row of two pairs or more descends
            assert info['rows_rewritten'] == (np.bincount(rows) >= 2).sum()
    # one row more in the shape: an empty last row
    wider, _ = check_list(r, c, v, (shape[0] + 1, shape[1]))
    assert wider[1:] == mine[1:]
    if order == 'shuffled':         # a second ingest gives the same bytes
        with D().from_pairs(r, v, shape=shape, cols=c) as again:
            assert arrays(again) == mine


def test_lists_on_both_sides_of_every_cut_of_the_passes_over_the_pairs():
    assert cb.grid_edges() == [0, 1, 63, 64, 65, 255, 256, 257, cb.SWEEP_PAIRS - 1, cb.SWEEP_PAIRS, cb.SWEEP_PAIRS + 1]
    shape = (3000, 500)
    for m in cb.grid_edges():
        for grouped in (False, True):
            rows, cols, values = cb.random_list(m, shape, seed=m % 1000 + grouped, grouped=grouped)
            check_list(rows, cols, values, shape, restate=m <= 257)
    # no rows and no pairs; rows and no pairs; all pairs in one row, between the LDS and the global class
    none = np.zeros(0, dtype=np.int64)
    check_list(none, none, np.zeros(0), (0, 0), restate=True)
    check_list(none, none, np.zeros(0), (0, 7), restate=True)
    check_list(none, none, None, (5, 7), restate=True)
    for m in (300, cb.SWEEP_PAIRS + 1):
        rows, cols, values = cb.random_list(m, (1, 70000), seed=9)
        mine, info = check_list(rows + 2, cols, values, (4, 70000))
        assert info['rows_rewritten'] == 1 and info['long_rows'] == (m > 16384) and info['duplicates_merged'] > 0


def test_the_values_of_one_entry_are_added_in_the_order_given():
    seq = np.array([1e16, 1.0, -1e16, 1.0] * 8)
    results = []
    for perm in (np.arange(32), np.random.RandomState(1).permutation(32), np.arange(32)[::-1]):
        rows, cols, vals = [], [], []
        for p, v in enumerate(seq[perm]):
            rows += [5, p % 4]; cols += [9, p % 7]; vals += [float(v), 0.5 * (p + 1)]           # other rows' pairs in between
        rows += [6, 6, 2, 3, 3]; cols += [10, 10, 11, 11, 11]; vals += [3.0, -3.0, 0.0, -1.0, -1.5]   # a group summing to 0, a zero, negatives
        rows, cols, vals = np.array(rows), np.array(cols), np.array(vals)
        mine, info = check_list(rows, cols, vals, (8, 12), restate=True)
        want = 0.0
        for v in seq[perm]:
            want += float(v)                    # its own stable-order sum
        with D().from_pairs(rows, vals, shape=(8, 12), cols=cols) as c:
            A = c.to_scipy()
            assert bits(A[5, 9]) == bits(want) and A[6, 10] == 0 and A[2, 11] == 0 and A[3, 11] == -2.5
            assert (A[5].nnz == 1) == (want != 0)                 # a sum that is exactly 0 is dropped, not stored
            assert c.zeros_dropped == 2 + (want == 0) and c.duplicates_merged == 31 + 2 + 4 and c.negatives == 1 + (want < 0)
        results.append(want)
    assert results == [1.0, 2.0, 0.0]           # the order matters for these values, and one order sums to exactly 0


def test_every_representation_of_one_list_gives_the_same_bytes():
    import torch
    shape = (700, 900)
    rows, cols, values = cb.random_list(5000, shape, seed=4)
    f32 = values.astype(np.float32)
    want, info = check_list(rows, cols, values, shape)
    pairs = np.column_stack((rows, cols))
    assert pairs.flags.c_contiguous
    seen = []
    for idt in (np.int32, np.int64):
        for vals in (values, f32, None):
            ref = want if vals is not None else None
            both = []
            for stride in (1, 2):
                p = pairs.astype(idt)
                host = D().from_pairs(p, vals, shape=shape) if stride == 2 else D().from_pairs(p[:, 0].copy(), vals, shape=shape, cols=p[:, 1].copy())
                tp = torch.as_tensor(p, device='cuda')
                tv = None if vals is None else torch.as_tensor(vals, device='cuda')
                dev = D().from_pairs(tp, tv, shape=shape) if stride == 2 else D().from_pairs(tp[:, 0].contiguous(), tv, shape=shape, cols=tp[:, 1].contiguous())
                with host, dev:
                    both += [arrays(host), arrays(dev)]
                    assert host.stored == dev.stored == 5000 and {key: getattr(host, key) for key in INFO} == {key: getattr(dev, key) for key in INFO}
            assert all(b == both[0] for b in both) and (ref is None or both[0] == ref)
            seen.append(both[0])
    # values=None counts occurrences: np.add.at on the host
    counts = np.zeros(shape)
    np.add.at(counts, (rows, cols), 1.0)
    with D().from_pairs(pairs) as c:             # the shape from the largest indices
        assert c.shape == (rows.max() + 1, cols.max() + 1) and same(c.to_scipy(), sp.csr_matrix(counts[:rows.max() + 1, :cols.max() + 1]))
    with pytest.raises(ValueError, match='shape'):
        D().from_pairs(torch.as_tensor(pairs, device='cuda'))
    with D().from_pairs(np.zeros((0, 2), dtype=np.int64)) as c:
        assert c.shape == (0, 0) and c.nnz == 0


REFUSALS = [
    ('row', dict(rows={40: 700}), ValueError, 'row 700 at pair 40 is out of range'),
    ('row_two_offenders', dict(rows={4000: -1, 300: 701}), ValueError, 'row 701 at pair 300 is out of range'),
    ('column', dict(cols={4999: 900}), ValueError, 'column 900 at pair 4999 is out of range'),
    ('column_two_offenders', dict(cols={70: -5, 69: 2 ** 31}), ValueError, 'column 2147483648 at pair 69 is out of range'),
    ('value', dict(values={0: np.nan}), ValueError, 'value nan at pair 0 is not finite'),
    ('value_two_offenders', dict(values={2500: np.inf, 2499: -np.inf}), ValueError, 'value -inf at pair 2499 is not finite'),
    ('row_before_column', dict(rows={4500: 700}, cols={3: -1}), ValueError, 'row 700 at pair 4500 is out of range'),
    ('column_before_value', dict(cols={4500: 900}, values={3: np.nan}), ValueError, 'column 900 at pair 4500 is out of range'),
]


@pytest.mark.parametrize('name,planted,kind,text', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_malformed_list_is_refused_by_its_first_broken_rule_and_nothing_is_kept(name, planted, kind, text):
    shape = (700, 900)
    rows, cols, values = cb.random_list(5000, shape, seed=4)
    given = dict(rows=rows, cols=cols, values=values)
    for key, at in planted.items():
        for p, v in at.items():
            given[key][p] = v
    assert cb.check(rows, cols, values, shape)[1] == text
    before = memory()
    for stride in (1, 2):
        with pytest.raises(kind) as e:
            if stride == 1:
                D().from_pairs(rows, values, shape=shape, cols=cols)
            else:
                D().from_pairs(np.column_stack((rows, cols)), values, shape=shape)
        assert str(e.value) == text
    from rri_nmf_amd.engine import RRIEngine
    with RRIEngine(1, 1, 1, dtype=np.float64) as eng:
        out = C.c_void_p(5)
        st = eng._lib.rri_corpus_from_pairs(eng._h, C.byref(out), shape[0], shape[1], rows.size, C.c_void_p(rows.ctypes.data),
                                            C.c_void_p(cols.ctypes.data), 9, 1, C.c_void_p(values.ctypes.data), 1, 0)
        assert st == -1 and not out.value and eng._err() == text
    assert memory() == before


def test_the_arguments_are_refused_before_any_array_is_read():
    from rri_nmf_amd.engine import RRIEngine
    rows, cols, values = cb.random_list(100, (20, 30), seed=1)
    before = memory()
    with pytest.raises(NotImplementedError, match='n_cols 2147483648 is 2\\^31 or more'):
        D().from_pairs(rows, values, shape=(20, 2 ** 31), cols=cols)
    with RRIEngine(1, 1, 1, dtype=np.float64) as eng:
        def call(n_rows=20, n_cols=30, m=100, r=rows.ctypes.data, c=cols.ctypes.data, idt=9, stride=1, v=values.ctypes.data, vdt=1, out=True):
            o = C.c_void_p(5)
            st = eng._lib.rri_corpus_from_pairs(eng._h, C.byref(o) if out else None, n_rows, n_cols, m, C.c_void_p(r), C.c_void_p(c), idt, stride,
                                                C.c_void_p(v), vdt, 0)
            assert not out or not o.value
            return st, eng._err()
        assert call(stride=0) == (-1, 'index_stride 0 is below 1')
        assert call(n_cols=2 ** 31) == (-3, 'n_cols 2147483648 is 2^31 or more')
        assert call(m=2 ** 31) == (-3, 'n_pairs 2147483648 is above 2^31 - 1: the pair position is half of a sort key')
        assert call(m=-1) == (-1, 'n_pairs -1 is negative') and call(n_rows=-2)[0] == -1
        assert call(idt=1)[0] == -1 and call(vdt=9)[0] == -1 and call(r=None)[0] == -1 and call(c=None) == (-1, 'cols is NULL with 100 pairs')
        assert call(out=False) == (-1, 'the output pointer is NULL')
    assert memory() == before


# ---- the split by entry -------------------------------------------------------------------------------------------------------------
def check_split(corpus, A, held_out, seed):
    thr = dc.threshold(held_out)
    want_o, want_h = cb.split_entries(A, thr, seed)
    before = memory()
    observed, held = corpus.split_entries(held_out=held_out, random_state=seed)
    with observed, held:
        O, H = observed.to_scipy(), held.to_scipy()
        assert same(O, want_o) and same(H, want_h)
        total = sp.csr_matrix(O + H)
        total.sort_indices()
        assert same(total, A) and O.multiply(H).nnz == 0 and O.nnz + H.nnz == A.nnz                    # disjoint, and their union is A
        assert (O.has_canonical_format or O.nnz == 0) and (H.has_canonical_format or H.nnz == 0)
        for part, M in ((observed, O), (held, H)):
            assert part.shape == A.shape and part.nnz == part.stored == M.nnz and part.negatives == (M.data < 0).sum()
            assert part.rows_rewritten == part.duplicates_merged == part.zeros_dropped == part.long_rows == 0 and part.ingest_ms >= 0
        assert memory()[0] == (before[0][0] + 2, before[0][1] + observed.device_bytes + held.device_bytes) and memory()[1] == before[1]
    assert memory() == before
    return want_h


def test_split_entries_against_the_restatement(edges):
    rows, cols, values, shape = edges
    with D().from_pairs(rows, values, shape=shape, cols=cols) as corpus:
        A = corpus.to_scipy()
        h1 = check_split(corpus, A, 0.05, 12345)
        h2 = check_split(corpus, A, 0.05, 12346)
        check_split(corpus, A, 0.5, (5 << 32) | 12345)                  # a seed with a non-zero high word
        assert not same(h1, h2) and 0 < h1.nnz < A.nnz
        lo = check_split(corpus, A, 2.0 ** -32, 3)                       # threshold 1
        hi = check_split(corpus, A, float(np.nextafter(1.0, 0.0)), 3)    # threshold 2^32 - 1
        assert lo.nnz <= 1 and hi.nnz >= A.nnz - 1
        assert same(corpus.to_scipy(), A)
    # negative and fractional values: copied bit for bit, no value check
    B = dc.count_corpus([0, 5, 64, 65, dc.PIECE + 1, 300, 1, 2 * dc.PIECE + 1], 3000, seed=2, negatives=True)
    assert (B.data < 0).any() and (B.data != np.floor(B.data)).all()
    with D()(B) as corpus:
        check_split(corpus, B, 0.3, 7)
        observed, held = si().split_entries(corpus, held_out=0.3, random_state=7)           # the public dispatch
        with observed, held:
            assert same(held.to_scipy(), cb.split_entries(B, dc.threshold(0.3), 7)[1])
    for empty in (sp.csr_matrix((0, 5)), sp.csr_matrix((4, 5))):
        with D()(empty) as corpus:
            check_split(corpus, empty, 0.5, 1)


def si():
    from rri_nmf_amd import sklearn_interface
    return sklearn_interface


def test_a_pattern_of_ones_splits_as_split_counts_does():
    A = dc.count_corpus(dc.GPU_LENGTHS, dc.GPU_D, seed=1, top=1)
    assert (A.data == 1).all()
    with D()(A) as corpus:
        for held_out, seed in ((0.5, 0), (0.05, 12345), (0.3, (9 << 32) | 4)):
            a = corpus.split_entries(held_out=held_out, random_state=seed)
            b = corpus.split_counts(held_out=held_out, random_state=seed)
            with a[0], a[1], b[0], b[1]:
                assert same(a[0].to_scipy(), b[0].to_scipy()) and same(a[1].to_scipy(), b[1].to_scipy()) and a[1].nnz > 0


def test_the_held_share_of_a_split_by_entry_is_sane():
    """12060 entries, held_out 0.2, seed 7: the restatement holds 2439 out, +0.61 standard deviations from q N = 2412 (computed
    on the CPU first); the bound is five"""
    A = dc.count_corpus([200 + (q * 7) % 3 for q in range(60)], 3000, seed=11, negatives=True)
    q, N = 0.2, A.nnz
    assert N == 12060
    with D()(A) as corpus:
        held = check_split(corpus, A, q, 7)
    H = held.nnz
    print('split_entries sanity: q %.2f  N %d  H %d  %+.2f standard deviations' % (q, N, H, (H - q * N) / np.sqrt(q * (1 - q) * N)))
    assert abs(H - q * N) <= 5 * np.sqrt(q * (1 - q) * N)


def test_a_split_with_a_threshold_of_zero_or_without_an_output_is_refused():
    from rri_nmf_amd.engine import RRIEngine
    A = dc.count_corpus([3, 0, 70], 100, seed=3)
    with D()(A) as c:
        before = memory()
        with RRIEngine(1, 1, 1, dtype=np.float64) as eng:
            observed, held = C.c_void_p(5), C.c_void_p(6)
            st = eng._lib.rri_corpus_split_entries(eng._h, c._ptr(), 0, 3, C.byref(observed), C.byref(held))
            assert st == -1 and 'threshold 0' in eng._err() and not observed.value and not held.value
            held = C.c_void_p(6)
            assert eng._lib.rri_corpus_split_entries(eng._h, c._ptr(), 5, 3, None, C.byref(held)) == -1 and 'output pointer is NULL' in eng._err()
            assert not held.value
            assert eng._lib.rri_corpus_split_entries(eng._h, None, 5, 3, C.byref(observed), C.byref(held)) == -1 and 'NULL or has been destroyed' in eng._err()
        assert memory() == before
        for bad in (0.0, 1.0, 2.0 ** -33):
            with pytest.raises(ValueError, match='held_out'):
                c.split_entries(bad)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_tokens_become_a_corpus_that_is_pruned_fitted_and_scored_like_its_scipy_twin():
    rng = np.random.RandomState(6)
    n, d, k = 30, 60, 3
    doc_ids = rng.randint(0, n, size=900)
    word_ids = np.minimum(rng.geometric(0.08, size=900) - 1 + (doc_ids % 3) * 9, d - 1)
    counts = np.zeros((n, d))
    np.add.at(counts, (doc_ids, word_ids), 1.0)
    fits = []
    for corpus in (D().from_pairs(doc_ids, cols=word_ids, shape=(n, d)), D()(sp.csr_matrix(counts))):
        with corpus:
            pruned, kept = corpus.prune_words(min_df=2)
            observed, held = pruned.split_counts(held_out=0.5, random_state=5)
            with pruned, observed, held:
                E = si().NMF_TM_Estimator(n, kept.size, k, max_iter=5, nmf_kwargs={'sparse_X': True})
                E.fit(observed)
                fits.append((kept, np.asarray(E.W), np.asarray(E.T), E.log_likelihood(held, W=E.W)))
                E.release()
    (ka, Wa, Ta, la), (kb, Wb, Tb, lb) = fits
    assert np.array_equal(ka, kb) and np.array_equal(bits(Wa), bits(Wb)) and np.array_equal(bits(Ta), bits(Tb))
    assert set(la) == set(lb) and all(np.array_equal(bits(la[key]), bits(lb[key])) for key in la)


def test_ratings_are_split_fitted_and_ranked_like_their_scipy_twins():
    rng = np.random.RandomState(8)
    n, d, k = 40, 50, 3
    index_pairs = np.unique(np.column_stack((rng.randint(0, n, size=700), rng.randint(0, d, size=700))), axis=0)
    index_pairs = index_pairs[rng.permutation(len(index_pairs))]
    ratings = rng.randint(1, 6, size=len(index_pairs)).astype(np.float64) - 0.5
    with D().from_pairs(index_pairs, ratings, shape=(n, d)) as corpus:
        train, test = corpus.split_entries(held_out=0.2, random_state=3)
        with train, test:
            assert train.nnz + test.nnz == len(index_pairs) and test.nnz > 50
            out = []
            for tr, te in ((train, test), (train.to_scipy(), test.to_scipy())):
                E = si().NMF_RS_Estimator(n, d, k, max_iter=4, use_validation_early_stopping=False)
                E.fit_from_Xtr(tr)
                out.append((np.asarray(E.W), np.asarray(E.T), E.ranking_score(te, n_items=5), E.score(te), E.rank(te)))
    (Wa, Ta, ra, sa, ka), (Wb, Tb, rb, sb, kb) = out
    assert np.array_equal(bits(Wa), bits(Wb)) and np.array_equal(bits(Ta), bits(Tb)) and sa == sb
    assert ra.keys() == rb.keys() and all(ra[key] == rb[key] or (np.isnan(ra[key]) and np.isnan(rb[key])) for key in ra)
    assert np.array_equal(ka[0], kb[0]) and np.array_equal(ka[1], kb[1])
