"""tf-idf / row normalisation of an X kept as CSR on the device (rri_csr_column_positive_counts, rri_csr_scale_X) against the
CSR branch of nmf._preprocess_on_host (matrixops.py:124-179), the zero-total rule, and the routes of nmf() and of the topic-model
estimator that now end there."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import relfro

pytestmark = pytest.mark.gpu

# the bounds tests/test_preprocess_gpu.py uses for the dense route: times max(1, max |reference|)
TOL = {np.float64: 1e-15, np.float32: 2e-7}
COL_BLOCK = 15296          # width of a column block of the row copy / height of a row block of the column copy


def csr_counts(n, d, row_lens, seed, first_rows=(), stored_zeros=6):
    """term counts as canonical CSR: row i stores row_lens[i] distinct columns (the rows of `first_rows` exactly those columns),
    values 1..5, and `stored_zeros` of the values -- in rows of three or more entries, one per row -- are explicit zeros"""
    rs = np.random.RandomState(seed)
    cols = []
    for i in range(n):
        if i < len(first_rows):
            cols.append(np.unique(np.asarray(first_rows[i], dtype=np.int64)))
        else:
            cols.append(np.sort(rs.choice(d, size=int(row_lens[i]), replace=False)))
    indptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    indices = np.concatenate(cols).astype(np.int32)
    data = rs.randint(1, 6, size=indices.size).astype(np.float64)
    roomy = np.nonzero(np.diff(indptr) >= 3)[0]
    for i in rs.choice(roomy, size=min(stored_zeros, roomy.size), replace=False):
        data[indptr[i] + 1] = 0.0
    X = sp.csr_matrix((data, indices, indptr), shape=(n, d))
    assert X.has_canonical_format and X.nnz == indices.size
    return X


def shape_small():
    return csr_counts(57, 33, np.random.RandomState(1).randint(1, 12, size=57), seed=2)


def shape_one_past_a_column_block():
    """d = 15297, about 150 entries per row (a whole wave per row), a row of one entry in the last column, a row of 700"""
    d = COL_BLOCK + 1
    rs = np.random.RandomState(3)
    lens = rs.randint(100, 200, size=200)
    long_row = np.concatenate([rs.choice(d - 2, size=698, replace=False), [COL_BLOCK - 1, COL_BLOCK]])
    return csr_counts(200, d, lens, seed=4, first_rows=([d - 1], long_row))


def shape_one_past_two_column_blocks():
    """d = 30593, a few entries per row (eight lanes per row), a row of one entry in the last column, a row of 700"""
    d = 2 * COL_BLOCK + 1
    rs = np.random.RandomState(5)
    lens = rs.randint(1, 9, size=300)
    long_row = np.concatenate([rs.choice(d - 4, size=696, replace=False), [COL_BLOCK - 1, COL_BLOCK, 2 * COL_BLOCK - 1, 2 * COL_BLOCK]])
    return csr_counts(300, d, lens, seed=6, first_rows=([d - 1], long_row))


def shape_past_a_row_block():
    n = COL_BLOCK + 104
    return csr_counts(n, 40, np.random.RandomState(7).randint(1, 7, size=n), seed=8)


SHAPES = {'57x33': shape_small, 'd15297': shape_one_past_a_column_block, 'd30593': shape_one_past_two_column_blocks,
          'n15400': shape_past_a_row_block}
VARIANTS = {'tfidf': (True, False), 'normalize': (False, True), 'both': (True, True), 'given_idf': ('given', True)}


def host_reference(X, tf, norm):
    from rri_nmf_amd.nmf import _preprocess_on_host
    ref, idf = _preprocess_on_host(X, tf, norm)
    return (ref.toarray() if sp.issparse(ref) else np.asarray(ref)), idf


def assert_no_zero_total_row(X, tf, norm=False):
    """the comparisons below are of matrices that stay on the device route: no empty row, no row whose (tf-idf) total is 0"""
    assert np.all(np.diff(X.indptr) > 0)
    scaled, _ = host_reference(X, tf, False)
    assert np.all(scaled.sum(1) + np.spacing(1) >= 1e-10)


def upload_raw(eng, A):
    """the CSR arrays as they are (no canonicalisation on the way): explicit zeros and unsorted indices reach the library"""
    from rri_nmf_amd.engine import RRIEngine
    keep, args = RRIEngine._csr_args_raw(A)
    eng._check(eng._lib.rri_upload_X_csr(eng._h, *args))


def via_row_copy(eng):
    """the resident X as X @ eye, 64 identity columns at a time"""
    out = np.empty((eng.n, eng.d))
    B = np.zeros((eng.d, 64))
    for lo in range(0, eng.d, 64):
        m = min(64, eng.d - lo)
        B[lo + np.arange(m), np.arange(m)] = 1.0
        out[:, lo:lo + m] = eng.X_times(B[:, :m])
        B[lo + np.arange(m), np.arange(m)] = 0.0
    return out


def via_column_copy(eng):
    """the resident X as (X.T @ eye).T, 64 identity rows at a time"""
    out = np.empty((eng.n, eng.d))
    Q = np.zeros((eng.n, 64))
    for lo in range(0, eng.n, 64):
        m = min(64, eng.n - lo)
        Q[lo + np.arange(m), np.arange(m)] = 1.0
        out[lo:lo + m, :] = eng.Xt_times(Q[:, :m]).T
        Q[lo + np.arange(m), np.arange(m)] = 0.0
    return out


def csr_df(eng):
    df = np.empty(eng.d)
    eng._check(eng._lib.rri_csr_column_positive_counts(eng._h, df.ctypes.data_as(C.POINTER(C.c_double))))
    return df


@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_device_preprocessing_of_csr_matches_the_host(shape, store):
    from rri_nmf_amd.engine import RRIEngine
    from rri_nmf_amd.matrixops import tfidf
    X = SHAPES[shape]()
    n, d = X.shape
    assert np.count_nonzero(X.data == 0) > 0                      # explicit stored zeros
    lens = np.diff(X.indptr)
    if shape.startswith('d'):
        assert lens.min() == 1 and lens.max() >= 600 and X.indices.max() == d - 1
    _, idf_host = tfidf(X, return_idf=True)
    idf_host = np.asarray(idf_host.todense()).ravel()
    given = np.linspace(0.1, 3.0, d)
    for which, (tf, norm) in sorted(VARIANTS.items()):
        tf = given if tf == 'given' else tf
        assert_no_zero_total_row(X, tf)
        ref, _ = host_reference(X, tf, norm)
        with RRIEngine(n, d, 3, dtype=store, sparse_x=True) as eng:
            upload_raw(eng, X.astype(store))
            df = csr_df(eng)
            assert np.array_equal(df, np.asarray((X > 0).sum(0)).ravel()), which
            idf = eng.preprocess(tfidf=tf, normalize=norm)
            got_rows, got_cols = via_row_copy(eng), via_column_copy(eng)
        if tf is True:
            assert np.array_equal(idf, idf_host), which
        elif tf is not False:
            assert np.array_equal(idf, given)
        else:
            assert idf is None
        bound = TOL[store] * max(1.0, np.max(np.abs(ref)))
        err_rows, err_cols = np.max(np.abs(got_rows - ref)), np.max(np.abs(got_cols - ref))
        print('%s %s %s: max |device - host| %.3g (row copy) %.3g (column copy), bound %.3g'
              % (shape, np.dtype(store).name, which, err_rows, err_cols, bound))
        assert err_rows <= bound and err_cols <= bound, (which, err_rows, err_cols, bound)
        assert np.array_equal(got_rows, got_cols), which


@pytest.mark.parametrize('store', [np.float64, np.float32])
def test_unsorted_column_indices_at_upload(store):
    from rri_nmf_amd.engine import RRIEngine
    X = csr_counts(200, 150, np.random.RandomState(11).randint(1, 20, size=200), seed=12)
    A = X.copy()
    for i in range(A.shape[0]):
        a, b = A.indptr[i], A.indptr[i + 1]
        A.indices[a:b] = A.indices[a:b][::-1].copy()
        A.data[a:b] = A.data[a:b][::-1].copy()
    A.has_sorted_indices = False
    assert_no_zero_total_row(X, True)
    ref, idf_host = host_reference(X, True, True)
    with RRIEngine(200, 150, 3, dtype=store, sparse_x=True) as eng:
        upload_raw(eng, A.astype(store))
        idf = eng.preprocess(tfidf=True, normalize=True)
        got_rows, got_cols = via_row_copy(eng), via_column_copy(eng)
    bound = TOL[store] * max(1.0, np.max(np.abs(ref)))
    assert np.array_equal(idf, idf_host)
    assert np.max(np.abs(got_rows - ref)) <= bound and np.max(np.abs(got_cols - ref)) <= bound


def sweep_from(eng, W0, T0, sweeps=2):
    eng.set_W(W0)
    eng.set_T(T0)
    eng.set_params(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
    eng.sweep(sweeps)
    return eng.get_W(), eng.get_T()


@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape', ['57x33', 'd15297', 'n15400'])
def test_blocked_copies_follow_the_rewrite(shape, store):
    """The products above read the canonical values through the copies' positions; the sweeps read the values the two blocked
    copies hold themselves.  A handle that uploads exactly the preprocessed values (same pattern) gathers its copies at upload:
    sweeps on the preprocessed handle must give the same bits, which they only do when its copies were gathered again."""
    from rri_nmf_amd.engine import RRIEngine
    X = SHAPES[shape]()
    n, d = X.shape
    assert_no_zero_total_row(X, True)
    rs = np.random.RandomState(13)
    W0, T0 = rs.rand(n, 3), rs.rand(3, d)
    T0 /= T0.sum(1, keepdims=True)
    with RRIEngine(n, d, 3, dtype=store, sparse_x=True) as eng:
        upload_raw(eng, X.astype(store))
        eng.preprocess(tfidf=True, normalize=True)
        dense = via_row_copy(eng)
        a = sweep_from(eng, W0, T0)
    rows = np.repeat(np.arange(n), np.diff(X.indptr))
    same_pattern = sp.csr_matrix((dense[rows, X.indices].astype(store), X.indices, X.indptr), shape=X.shape)
    with RRIEngine(n, d, 3, dtype=store, sparse_x=True) as eng:
        upload_raw(eng, same_pattern)
        assert np.array_equal(via_row_copy(eng), dense)
        b = sweep_from(eng, W0, T0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with RRIEngine(n, d, 3, dtype=store, sparse_x=True) as eng:      # ... and the raw counts give something else
        upload_raw(eng, X.astype(store))
        c = sweep_from(eng, W0, T0)
    assert relfro(c[1], a[1]) > 1e-3


def universal_terms_document():
    """no empty row, but document 5 holds only the term that every document holds: idf 0, tf-idf total 0"""
    X = shape_small().tolil()
    X[:, 3] = 1
    X[5, :] = 0
    X[5, 3] = 7
    X = X.tocsr()
    assert np.all(np.diff(X.indptr) > 0)
    return X


def with_an_empty_row():
    X = shape_small().tolil()
    X[9, :] = 0
    X = X.tocsr()
    assert np.diff(X.indptr)[9] == 0
    return X


@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('case', ['empty_row', 'universal_terms'])
def test_zero_total_rows_leave_X_untouched(case, store):
    from rri_nmf_amd.engine import RRIEngine, ZeroTotalRows
    X = with_an_empty_row() if case == 'empty_row' else universal_terms_document()
    n, d = X.shape
    with RRIEngine(n, d, 3, dtype=store, sparse_x=True) as eng:
        eng.upload_X_csr(X.astype(store))
        before = via_row_copy(eng)
        assert np.array_equal(before, X.toarray())
        with pytest.raises(ZeroTotalRows) as ei:
            eng.preprocess(tfidf=True, normalize=True)
        assert ei.value.count == 1 and isinstance(ei.value, ValueError)
        assert np.array_equal(via_row_copy(eng), before) and np.array_equal(via_column_copy(eng), before)
        if case == 'empty_row':
            with pytest.raises(ZeroTotalRows):
                eng.preprocess(normalize=True)
            assert np.array_equal(via_row_copy(eng), before)
        # tf-idf alone has no dense row to write: it runs, and the handle is usable afterwards
        idf = eng.preprocess(tfidf=True)
        ref, idf_host = host_reference(X, True, False)
        assert np.array_equal(idf, idf_host)
        assert np.max(np.abs(via_row_copy(eng) - ref)) <= TOL[store] * max(1.0, np.max(np.abs(ref)))


TM_KW = dict(max_iter=6, random_state=0, project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0, compute_obj_each_iter=True)


@pytest.mark.parametrize('case', ['empty_row', 'universal_terms'])
def test_nmf_on_a_matrix_with_a_zero_total_row(case, caplog, monkeypatch):
    import logging
    from rri_nmf_amd import nmf as nmf_mod
    X = with_an_empty_row() if case == 'empty_row' else universal_terms_document()
    Xh, idf = nmf_mod._preprocess_on_host(X, True, True)
    a = nmf_mod.nmf(Xh, 4, sparse_X=True, **TM_KW)
    made = []
    real = nmf_mod.RRIEngine

    class Recording(real):
        def __init__(self, *args, **kw):
            made.append(bool(kw.get('sparse_x', False)))
            super().__init__(*args, **kw)

    monkeypatch.setattr(nmf_mod, 'RRIEngine', Recording)
    holder = nmf_mod.ResidentProblem() if case == 'universal_terms' else None
    with caplog.at_level(logging.INFO, logger=nmf_mod.logger.name):
        b = nmf_mod.nmf(X, 4, sparse_X=True, preprocess=('tfidf', 'normalize'), resident=holder, **TM_KW)
    # the empty row is seen on the host (one handle); the universal-terms document only by the device (a second handle)
    assert made == ([True] if case == 'empty_row' else [True, True])
    if case == 'universal_terms':
        assert holder.engine is None
        assert any('preprocessing on the host' in r.getMessage() for r in caplog.records)
    assert np.array_equal(b['idf'], idf)
    assert relfro(b['W'], a['W']) < 1e-8 and relfro(b['T'], a['T']) < 1e-8


def corpus(n=240, d=150, seed=21, empty_row=None):
    rs = np.random.RandomState(seed)
    X = rs.poisson(0.7, size=(n, d)).astype(np.float64)
    X[np.arange(n), rs.randint(0, d, size=n)] += 1
    if empty_row is not None:
        X[empty_row, :] = 0
    return sp.csr_matrix(X)


@pytest.mark.parametrize('init', ['nndsvd', 'random', 'smart_random'])
@pytest.mark.parametrize('route', ['csr_handle', 'densified'])
def test_nmf_preprocess_option_on_sparse_X_matches_host_preprocessing(route, init, monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    X = corpus(empty_row=7 if route == 'densified' else None)
    if route == 'csr_handle':
        assert_no_zero_total_row(X, True)
    Xh, idf = nmf_mod._preprocess_on_host(X, True, True)
    kw = dict(TM_KW, init=init, **({'sparse_X': True} if route == 'csr_handle' else {}))
    made = []
    real = nmf_mod.RRIEngine

    class Recording(real):
        def __init__(self, *args, **kws):
            made.append((bool(kws.get('sparse_x', False)), []))
            super().__init__(*args, **kws)

        def preprocess(self, **kws):
            made[-1][1].append(dict(kws))
            return super().preprocess(**kws)

    a = nmf_mod.nmf(Xh, 4, **kw)
    with monkeypatch.context() as mp:
        mp.setattr(nmf_mod, 'RRIEngine', Recording)
        b = nmf_mod.nmf(X, 4, preprocess={'tfidf': True, 'normalize': True}, **kw)
    assert len(made) == 1 and made[0][0] is (route == 'csr_handle') and len(made[0][1]) == 1      # one handle, preprocessed there
    assert np.array_equal(b['idf'], idf)
    print('%s %s: relfro W %.3g T %.3g' % (route, init, relfro(b['W'], a['W']), relfro(b['T'], a['T'])))
    assert relfro(b['W'], a['W']) < 1e-8 and relfro(b['T'], a['T']) < 1e-8
    assert np.allclose(b['obj_history'], a['obj_history'], rtol=1e-10)
    want = a['obj_calculator'].true_objective()
    assert abs(b['obj_calculator'].true_objective() - want) <= 1e-9 * abs(want)


@pytest.mark.parametrize('store', [np.float64, np.float32])
def test_preprocessing_twice_gives_the_same_bits(store):
    from rri_nmf_amd.engine import RRIEngine
    X = shape_one_past_a_column_block()
    n, d = X.shape
    outs = []
    for _ in range(2):
        with RRIEngine(n, d, 3, dtype=store, sparse_x=True) as eng:
            upload_raw(eng, X.astype(store))
            df = csr_df(eng)
            idf = eng.preprocess(tfidf=True, normalize=True)
            outs.append((df, idf, via_row_copy(eng), via_column_copy(eng)))
    for u, v in zip(*outs):
        assert np.array_equal(u, v)


def test_estimator_keeps_the_csr_handle():
    from rri_nmf_amd.sklearn_interface import NMF_TM_Estimator
    X, X2, Xte = corpus(seed=31), corpus(seed=32), corpus(n=60, seed=33)
    for A in (X, X2, Xte):
        assert_no_zero_total_row(A, True)
    n, d = X.shape
    runs = []
    for keep in (True, False):
        est = NMF_TM_Estimator(n, d, 4, handle_tfidf=True, handle_normalization=True, max_iter=5, random_state=3,
                               keep_resident=keep, nmf_kwargs={'sparse_X': True})
        steps = []
        A = X
        est.fit(A)
        steps.append((np.array(est.W), np.array(est.T), np.array(est.idf)))
        for _ in range(3):
            est.one_iter(A)
            steps.append((np.array(est.W), np.array(est.T), np.array(est.idf)))
        steps.append((est.transform(Xte),))
        if keep:
            assert est._resident.reuses == 3 and est._resident.engine is not None and est._resident.engine.sparse_x
            first = est._resident.engine
        else:
            assert est._resident is None
        del A
        A2 = X2
        est.one_iter(A2)                       # other counts of the same shape: a fresh handle, X2's factors
        steps.append((np.array(est.W), np.array(est.T), np.array(est.idf)))
        if keep:
            assert est._resident.reuses == 3 and est._resident.engine is not first and est._resident.given[0] is A2
            est.release()
            assert est._resident.engine is None
        runs.append(steps)
    for kept, fresh in zip(*runs):
        for u, v in zip(kept, fresh):
            assert np.array_equal(u, v)
    assert not np.array_equal(runs[0][3][2], runs[0][5][2])      # X2 has its own idf


def test_refusals():
    from rri_nmf_amd.engine import RRIEngine
    X = shape_small()
    n, d = X.shape
    dense = X.toarray()
    df = np.empty(d)
    ones = np.ones(d)
    zero_rows = C.c_int64(0)
    ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))

    def both_refused(eng):
        with pytest.raises(ValueError, match='RRI_UNWEIGHTED_SPARSE'):
            eng._check(eng._lib.rri_csr_column_positive_counts(eng._h, ptr(df)))
        with pytest.raises(ValueError, match='RRI_UNWEIGHTED_SPARSE'):
            eng._check(eng._lib.rri_csr_scale_X(eng._h, ptr(ones), 1, C.byref(zero_rows)))

    with RRIEngine(n, d, 3, dtype=np.float64) as eng:                          # dense
        eng.upload_X(dense)
        both_refused(eng)
        assert np.array_equal(eng.X_times(np.eye(d)), dense)
    with RRIEngine(n, d, 3, dtype=np.float64, weighted=True) as eng:           # weighted, dense
        eng.upload_X(dense)
        eng.upload_mask((dense > 0).astype(np.float64))
        both_refused(eng)
    with RRIEngine(n, d, 3, dtype=np.float64, weighted='sparse') as eng:       # weighted, pattern only
        eng.upload_observed_csr(X)
        both_refused(eng)
    with RRIEngine(n, d, 3, dtype=np.float64, sparse_x=True) as eng:
        both_refused(eng)                                                      # no X yet
        eng.upload_X_csr(X)
        before = via_row_copy(eng)
        with pytest.raises(ValueError, match='d entries'):
            eng.preprocess(tfidf=np.ones(d - 1))
        with pytest.raises(ValueError, match='d entries'):
            eng.preprocess(tfidf=np.ones(d + 1), normalize=True)
        with pytest.raises(ValueError):
            eng._check(eng._lib.rri_csr_column_positive_counts(eng._h, None))
        # the dense pair keeps refusing this handle
        with pytest.raises(ValueError):
            eng.column_positive_counts()
        with pytest.raises(ValueError):
            eng.scale_X(ones)
        assert np.array_equal(via_row_copy(eng), before)
