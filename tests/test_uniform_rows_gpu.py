"""Uniform rows of an X kept as CSR on the device (rri_set_uniform_rows, rri_get_uniform_rows, rri_csr_scale_X_uniform;
RRIEngine.set_uniform_rows / uniform_rows / preprocess(uniform_rows=True); nmf(..., uniform_rows=True)).  Row normalisation makes a
document whose total is below 1e-10 the DENSE row 1/d (matrixops.py:143-147); the handle keeps such rows as a sorted list U and a
value c beside the pattern, X = S + c e_U 1^T, and adds their share wherever it multiplies by X.  Checked here against the host's
preprocessing, the float64 oracle on the dense S + c e_U 1^T and a dense handle on the same matrix.

Shapes: the smallest at which the blocked copies change shape (COL_BLOCK = 15296 of test_sparse_preprocess_gpu.py): 57 x 33,
200 x 15297 (the last column alone in the second column block), 15400 x 40 (a second row block).  Tolerances are those of the
files named at each test."""
import ctypes as C
import logging

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import relfro
from rri_nmf_amd.synthetic import scaled_init
from test_sparse_preprocess_gpu import (COL_BLOCK, SHAPES as PRE_SHAPES, TOL as PRE_TOL, corpus, host_reference, upload_raw,
                                        via_column_copy, via_row_copy)

pytestmark = pytest.mark.gpu

TOL = 2e-9                      # test_sparse_x_gpu.py's TOL, both storage types
TM = dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
SHAPES = {'57x33': '57x33', '200x15297': 'd15297', '15400x40': 'n15400'}
UNIVERSAL = 3                   # the column every document holds (universal_terms_document of test_sparse_preprocess_gpu.py)


def oracle():
    from oracle import rri_oracle
    return rri_oracle


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


_cache = {}


def cached(key, make):
    """a reference, computed once and never written to"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def emptied_rows(n):
    """row 0 and row n - 1, two adjacent rows and, where there is one, a row past the first row block"""
    return [0, n - 1, 20, 21] + ([COL_BLOCK + 4] if n > COL_BLOCK else [])


STORED = 5                      # the zero-total row that stores something


def counts_with_zero_total_rows(shape, kind='empty'):
    """(term counts as CSR, sorted U); U: the rows whose tf-idf total is below 1e-10, from the host.
    kind 'empty':     the rows of emptied_rows store nothing, and document STORED stores one explicit zero -- a total of 0 with a
                      stored entry, whatever the idf (a term every document holds has idf 0 only while no document is empty)
    kind 'universal': no empty row; every document holds term UNIVERSAL, whose idf is therefore exactly 0, and document STORED --
                      like every document the base shape gave a single entry in that column -- holds nothing else
                      (universal_terms_document of test_sparse_preprocess_gpu.py)"""
    def make():
        X = PRE_SHAPES[SHAPES[shape]]().tolil()
        n = X.shape[0]
        if kind == 'universal':
            X[:, UNIVERSAL] = 1
            X[STORED, :] = 0
            X[STORED, UNIVERSAL] = 7
            X = X.tocsr()
            want = [STORED]
        else:
            empty = emptied_rows(n)
            for i in empty + [STORED]:
                X[i, :] = 0
            A = X.tocoo()
            rows, cols, vals = np.append(A.row, STORED), np.append(A.col, UNIVERSAL), np.append(A.data, 0.0)
            order = np.lexsort((cols, rows))
            X = sp.csr_matrix((vals[order], cols[order].astype(np.int32),
                               np.searchsorted(rows[order], np.arange(n + 1)).astype(np.int64)), shape=X.shape)
            want = empty + [STORED]
            assert np.array_equal(np.nonzero(np.diff(X.indptr) == 0)[0], sorted(empty))
        assert X.has_canonical_format and np.diff(X.indptr)[STORED] == 1
        scaled, _ = host_reference(X, True, False)
        U = np.nonzero(scaled.sum(1) + np.spacing(1) < 1e-10)[0].astype(np.int32)
        assert set(want) <= set(U.tolist()) and U.size < 0.01 * n + 8
        return X, U
    return cached(('counts', shape, kind), make)


def stored_S(shape):
    """(S as CSR with values exact in float32, sorted U): the counts of the base shape over 4 with the rows of emptied_rows
    emptied; U holds those and the adjacent rows STORED, STORED + 1, which keep the entries they store"""
    def make():
        X = PRE_SHAPES[SHAPES[shape]]().tolil()
        empty = emptied_rows(X.shape[0])
        for i in empty:
            X[i, :] = 0
        S = X.tocsr()
        S.sort_indices()
        S.data = S.data / 4.0
        assert np.all(np.diff(S.indptr)[[STORED, STORED + 1]] > 0) and np.any(S[STORED].data != 0)
        return S, np.array(sorted(empty + [STORED, STORED + 1]), dtype=np.int32)
    return cached(('S', shape), make)


def dense_of(S, U, c):
    D = S.toarray()
    D[U, :] = c
    return D


def start(D, k, tm, seed=1):
    W0, T0 = scaled_init(D + 1e-3, k, seed=seed)
    if tm:
        T0 = oracle().proj_rows_simplex(np.maximum(T0, 0).copy(), 1.0)
    return W0, T0


def run_oracle(D, W0, T0, sweeps, **kw):
    return oracle().nmf(D, W0.shape[1], W_in=W0.copy(), T_in=T0.copy(), max_iter=sweeps, eps_stop=-1, **kw)


def run(S, U, c, W0, T0, sweeps, store, final_proj=None, **params):
    n, d = S.shape
    with engine(n, d, W0.shape[1], dtype=store, sparse_x=True) as e:
        e.upload_X_csr(S.astype(store))
        if U is not None:
            e.set_uniform_rows(U, c)
        e.set_W(np.maximum(W0, 0))
        e.set_T(np.maximum(T0, 0))
        e.set_params(**params)
        e.sweep(sweeps)
        if final_proj is not None:
            e.project_W_rows(final_proj)
        return e.get_W(), e.get_T(), e.n_resets_used


# ---- 1. preprocessing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape, kind', [(sh, kd) for sh in sorted(SHAPES) for kd in ('empty', 'universal')] + [('57x33-none', 'none')])
def test_preprocessing_keeps_zero_total_rows_as_uniform_rows(shape, kind, store):
    """tests/test_sparse_preprocess_gpu.py's comparison and bound (TOL times max(1, max |reference|)), on matrices that file has to
    leave to the host"""
    if shape.endswith('-none'):                   # U empty: the entry point on a matrix without such a row
        X, U = PRE_SHAPES['57x33'](), np.zeros(0, dtype=np.int32)
    else:
        X, U = counts_with_zero_total_rows(shape, kind)
    n, d = X.shape
    ref, idf_host = cached(('host', shape, kind), lambda: host_reference(X, True, True))
    # the reference makes exactly the rows of U uniform
    assert np.array_equal(np.nonzero(np.all(ref == 1.0 / d, axis=1))[0], U)
    scaled, _ = host_reference(X, True, False)
    assert np.array_equal(np.nonzero(scaled.sum(1) + np.spacing(1) < 1e-10)[0], U)
    with engine(n, d, 3, dtype=store, sparse_x=True) as eng:
        upload_raw(eng, X.astype(store))
        assert eng.uniform_rows()[0].size == 0 and eng.uniform_rows()[1] == 0.0
        idf = eng.preprocess(tfidf=True, normalize=True, uniform_rows=True)
        rows, value = eng.uniform_rows()
        got_rows, got_cols = via_row_copy(eng), via_column_copy(eng)
    assert np.array_equal(idf, idf_host)
    assert rows.dtype == np.int32 and np.array_equal(rows, U)
    assert value == (1.0 / d if U.size else 0.0)
    bound = PRE_TOL[store] * max(1.0, np.max(np.abs(ref)))
    err_rows, err_cols = np.max(np.abs(got_rows - ref)), np.max(np.abs(got_cols - ref))
    print('%s %s %s: max |device - host| %.3g (row copy) %.3g (column copy), bound %.3g; |U| = %d'
          % (shape, kind, np.dtype(store).name, err_rows, err_cols, bound, U.size))
    assert err_rows <= bound and err_cols <= bound
    assert np.all(got_rows[U] == 1.0 / d) and np.all(got_cols[U] == 1.0 / d)


@pytest.mark.parametrize('store', [np.float64, np.float32])
def test_normalisation_alone_collects_the_empty_rows(store):
    X, U = counts_with_zero_total_rows('57x33')
    n, d = X.shape
    empty = np.nonzero(np.diff(X.indptr) == 0)[0]
    ref, _ = host_reference(X, False, True)
    with engine(n, d, 3, dtype=store, sparse_x=True) as eng:
        eng.upload_X_csr(X.astype(store))
        assert eng.preprocess(normalize=True, uniform_rows=True) is None
        rows, value = eng.uniform_rows()
        got = via_row_copy(eng)
    assert np.array_equal(rows, U) and value == 1.0 / d and 0 < empty.size < U.size      # (the stored zero sums to 0 too)
    assert np.max(np.abs(got - ref)) <= PRE_TOL[store] * max(1.0, np.max(np.abs(ref)))


# ---- 2. sweeps -------------------------------------------------------------------------------------------------------------
def sweep_reference(shape, c, tm, k, sweeps):
    def make():
        S, U = stored_S(shape)
        D = dense_of(S, U, c)
        W0, T0 = start(D, k, tm)
        ref = run_oracle(D, W0, T0, sweeps, **(TM if tm else {}))
        return ref['W'], ref['T'], ref['n_resets_used']
    return cached(('sweeps', shape, c, tm, k, sweeps), make)


@pytest.mark.parametrize('k', [4, 7])
@pytest.mark.parametrize('flags', ['plain', 'tm'])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_sweeps_against_the_oracle(shape, flags, k):
    """1, 2 and 5 sweeps on S + c e_U 1^T with c = 1/d and c = 0.37, both stores: test_sparse_x_gpu.py's TOL against the oracle"""
    S, U = stored_S(shape)
    tm = flags == 'tm'
    for c in (1.0 / S.shape[1], 0.37):
        D = dense_of(S, U, c)
        W0, T0 = start(D, k, tm)
        for sweeps in (1, 2, 5):
            Wr, Tr, nr = sweep_reference(shape, c, tm, k, sweeps)
            for store in (np.float64, np.float32):
                W, T, nres = run(S, U, c, W0, T0, sweeps, store, final_proj=1.0 if tm else None, **(TM if tm else {}))
                ew, et = relfro(W, Wr), relfro(T, Tr)
                print('%s %s k=%d c=%.4g sweeps=%d %s: W %.3g T %.3g' % (shape, flags, k, c, sweeps, np.dtype(store).name, ew, et))
                assert nres == nr and ew < TOL and et < TOL, (c, sweeps, store, ew, et)


@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_against_a_dense_handle_on_the_same_matrix(shape, store):
    """test_sparse_x_gpu.py::test_against_dense_handle's bound, 1e-10, factors and objective histories"""
    S, U = stored_S(shape)
    n, d = S.shape
    for c, params in ((1.0 / d, dict(TM)), (0.37, {})):
        D = dense_of(S, U, c)
        W0, T0 = start(D, 4, bool(params))
        outs = []
        for uniform in (True, False):
            # the dense handle stores float32 values: c itself only where float32 holds it, so it gets float64 there
            dt = store if uniform else np.float64
            with engine(n, d, 4, dtype=dt, sparse_x=uniform) as e:
                if uniform:
                    e.upload_X_csr(S.astype(store))
                    e.set_uniform_rows(U, c)
                else:
                    e.upload_X_csr(sp.csr_matrix(D))
                e.set_W(W0); e.set_T(T0); e.set_params(**params)
                obj = []
                for _ in range(4):
                    e.sweep(1)
                    obj.append(e.objective())
                outs.append((e.get_W(), e.get_T(), e.n_resets_used, obj))
        a, b = outs
        assert a[2] == b[2]
        assert relfro(a[0], b[0]) < 1e-10 and relfro(a[1], b[1]) < 1e-10, (relfro(a[0], b[0]), relfro(a[1], b[1]))
        assert np.allclose(a[3], b[3], rtol=1e-10, atol=0), (a[3], b[3])


@pytest.mark.parametrize('store', [np.float64, np.float32])
def test_every_row_uniform_and_none(store):
    S, _ = stored_S('57x33')
    n, d = S.shape
    for U, c in ((np.arange(n, dtype=np.int32), 0.37), (np.zeros(0, dtype=np.int32), 0.37)):
        D = dense_of(S, U, c)
        W0, T0 = start(D, 4, False)
        ref = run_oracle(D, W0, T0, 2, t_row_sum=1.0)
        W, T, nres = run(S, U, c, W0, T0, 2, store, t_row_sum=1.0)
        assert nres == ref['n_resets_used'] and relfro(W, ref['W']) < TOL and relfro(T, ref['T']) < TOL


# ---- 3. objective ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_objective_in_both_forms(shape, store):
    """1/2 ||X - W T||^2 on the full X after a complete sweep (cross terms) and off the sweep (pattern form):
    test_sparse_x_gpu.py::test_objective_off_the_sweep's bound, 1e-11 relative"""
    S, U = stored_S(shape)
    n, d = S.shape
    # test_objective_off_the_sweep's penalties (at these values of X they kill topics: the sweep resets some) and small ones
    for regs in (dict(reg_w_l1=0.3, reg_w_l2=0.1, reg_t_l1=0.4, reg_t_l2=0.2), dict(reg_w_l1=0.003, reg_w_l2=0.1, reg_t_l1=0.004, reg_t_l2=0.2)):
        order = (regs['reg_w_l2'], regs['reg_t_l2'], regs['reg_w_l1'], regs['reg_t_l1'])
        for c in (1.0 / d, 0.37):
            D = dense_of(S, U, c)
            W0, T0 = start(D, 5, False, seed=4)
            with engine(n, d, 5, dtype=store, sparse_x=True) as e:
                e.upload_X_csr(S.astype(store))
                e.set_uniform_rows(U, c)
                e.set_W(W0); e.set_T(T0)
                e.set_params(**regs)
                off = e.objective()
                e.sweep(1)
                after = e.objective()
                W1, T1 = e.get_W(), e.get_T()
                e.set_W(W1)                                   # from outside: the cross terms are gone, the pattern form again
                again = e.objective()
            want_off = oracle().true_objective(D, W0, T0, *order)
            want_after = oracle().true_objective(D, W1, T1, *order)
            print('%s %s c=%.4g l1=%.3g: off %.3g after %.3g again %.3g (relative)' % (shape, np.dtype(store).name, c, regs['reg_w_l1'],
                  abs(off - want_off) / abs(want_off), abs(after - want_after) / abs(want_after), abs(again - want_after) / abs(want_after)))
            assert np.count_nonzero(W1) > 0.2 * W1.size
            assert abs(off - want_off) <= 1e-11 * abs(want_off)
            assert abs(after - want_after) <= 1e-11 * abs(want_after)
            assert abs(again - want_after) <= 1e-11 * abs(want_after)


# ---- 4. T fixed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_fold_in_with_T_fixed(shape, store):
    S, U = stored_S(shape)
    for c in (1.0 / S.shape[1], 0.37):
        D = dense_of(S, U, c)
        for k in (4, 7):
            W0, T0 = start(D, k, True, seed=6)
            kw = dict(fix_T=True, t_row_sum=1.0, w_row_sum=1.0)
            Wr, Tr = cached(('fold', shape, c, k), lambda: (lambda r: (r['W'], r['T']))(run_oracle(D, W0, T0, 4, **kw)))
            W, T, nres = run(S, U, c, W0, T0, 4, store, final_proj=1.0, **kw)
            assert nres == 0 and np.array_equal(T, Tr)
            assert relfro(W, Wr) < TOL, (c, k, relfro(W, Wr))


# ---- 5. products -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_products_for_the_start(shape, store):
    """test_sparse_x_gpu.py::test_products_for_the_start's bound, 1e-13, more than 64 columns in chunks"""
    S, U = stored_S(shape)
    n, d = S.shape
    B = np.random.RandomState(72).rand(d, 70)
    Q = np.random.RandomState(73).rand(n, 70)
    with engine(n, d, 4, dtype=store, sparse_x=True) as e:
        e.upload_X_csr(S.astype(store))
        for c in (1.0 / d, 0.37):
            e.set_uniform_rows(U, c)
            D = dense_of(S, U, c)
            assert relfro(e.X_times(B), D @ B) < 1e-13
            assert relfro(e.Xt_times(Q), D.T @ Q) < 1e-13


def _power_panel(A, Q0, n_iter):
    Y = A @ Q0
    for _ in range(n_iter):
        Y = A @ np.linalg.qr(A.T @ np.linalg.qr(Y)[0])[0]
    return Y


@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_range_finder_in_both_orientations(shape, store):
    """against the same call on a handle that stores the uniform rows as ordinary dense CSR rows, and against numpy, with the
    bounds of test_sparse_range_finder_gpu.py::test_the_call.  (The other handle stores float64 with either store: float32 does
    not hold c = 0.37, which the handle under test keeps as a double beside its store.)"""
    S, U = stored_S(shape)
    n, d = S.shape
    c, m = 0.37, 16
    D = dense_of(S, U, c)
    with engine(n, d, 4, dtype=store, sparse_x=True) as e, engine(n, d, 4, dtype=np.float64, sparse_x=True) as f:
        e.upload_X_csr(S.astype(store))
        e.set_uniform_rows(U, c)
        f.upload_X_csr(sp.csr_matrix(D))
        for transpose in (False, True):
            A = D.T if transpose else D
            Q0 = np.random.RandomState(5).randn(A.shape[1], m)
            for n_iter in (0, 3):
                Q, B = e.sparse_range_finder(Q0, n_iter, transpose=transpose)
                Q2, B2 = f.sparse_range_finder(Q0, n_iter, transpose=transpose)
                Y = _power_panel(A, Q0, n_iter)
                Qh = np.linalg.qr(Y)[0]
                QB, QB2 = Q @ B, Q2 @ B2
                figs = (np.abs(Q.T @ Q - np.eye(m)).max(), relfro(B, (A.T @ Q).T), relfro(Q @ (Q.T @ Y), Y),
                        relfro(Qh @ (Qh.T @ QB), QB), relfro(Q2 @ (Q2.T @ QB), QB), relfro(QB, QB2))
                print('%s %s transpose=%d n_iter=%d: orth %.2e  B %.2e  range %.2e / %.2e  other handle %.2e / %.2e'
                      % ((shape, np.dtype(store).name, transpose, n_iter) + figs))
                assert figs[0] < 1e-12 and figs[1] < 1e-12
                assert figs[2] < 1e-10 and figs[3] < 1e-6
                assert figs[4] < 1e-6 and figs[5] < 1e-6


# ---- 6. resets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_resets_against_the_oracle(shape, store):
    """a dead topic under max_resid_document: with c = 3 a uniform row has the largest positive residual and T[t,:] becomes that
    dense row; with c = 1/d an ordinary row wins while U is not empty.  The bound of the oracle comparison of
    test_sparse_x_gpu.py::test_resets_against_oracle.  At 200 x 15297 the dense reset row takes more than one workgroup of
    k_spu_reset_row and crosses the column-block boundary that the next pass reads it over"""
    S, U = stored_S(shape)
    n, d = S.shape
    for c, uniform_wins in ((3.0, True), (1.0 / d, False)):
        D = dense_of(S, U, c)
        W0, T0 = start(D, 4, False, seed=10)
        W0[:, 2] = 0.0
        ref = cached(('reset', shape, c), lambda: run_oracle(D, W0, T0, 2, t_row_sum=1.0))
        W, T, nres = run(S, U, c, W0, T0, 2, store, t_row_sum=1.0)
        assert nres >= 1 and nres == ref['n_resets_used']
        ew, et = relfro(W, ref['W']), relfro(T, ref['T'])
        print('%s %s c=%.4g: resets %d, W %.3g T %.3g' % (shape, np.dtype(store).name, c, nres, ew, et))
        assert ew < TOL and et < TOL
        # the row that wins the search on the handle, and the row it would hand to the reset
        with engine(n, d, 4, dtype=store, sparse_x=True) as e:
            e.upload_X_csr(S.astype(store))
            e.set_uniform_rows(U, c)
            e.set_W(W0); e.set_T(T0); e.set_params(t_row_sum=1.0)
            val, mi = e.resid_row_argmax()
            row = e.reset_row(mi)
        R = np.maximum(D - W0 @ T0, 0.0)
        pos = (R ** 2).sum(1)
        assert mi == int(np.argmax(pos)) and (mi in set(U.tolist())) == uniform_wins
        assert abs(val - pos[mi]) <= 1e-12 * pos[mi]
        assert np.max(np.abs(row - R[mi])) <= 1e-13 * max(1.0, R[mi].max())
        if uniform_wins:
            assert np.count_nonzero(row) > S[mi].nnz          # dense: more than the pattern of that row could hold


# ---- 7. determinism and state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_twenty_sweeps_are_bit_identical(shape, store):
    S, U = stored_S(shape)
    D = dense_of(S, U, 0.37)
    W0, T0 = start(D, 5, True, seed=62)
    a = run(S, U, 0.37, W0, T0, 20, store, **TM)
    b = run(S, U, 0.37, W0, T0, 20, store, **TM)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize('store', [np.float64, np.float32])
def test_an_empty_list_changes_no_bit(store):
    """a handle on which the calls of this feature found nothing to do gives the bits of one on which none was made"""
    X = PRE_SHAPES['d15297']()
    n, d = X.shape
    rs = np.random.RandomState(13)
    W0, T0 = rs.rand(n, 3), rs.rand(3, d)
    T0 /= T0.sum(1, keepdims=True)
    outs = []
    for touched in (False, True):
        with engine(n, d, 3, dtype=store, sparse_x=True) as e:
            upload_raw(e, X.astype(store))
            if touched:
                e.set_uniform_rows([], 0.5)
                idf = e.preprocess(tfidf=True, normalize=True, uniform_rows=True)
                e.set_uniform_rows(np.zeros(0, dtype=np.int32), 0.25)
                assert e.uniform_rows()[0].size == 0 and e.uniform_rows()[1] == 0.0
            else:
                idf = e.preprocess(tfidf=True, normalize=True)
            e.set_W(W0); e.set_T(T0); e.set_params(**TM)
            e.sweep(3)
            obj = e.objective()
            e.set_T(T0)
            off = e.objective()
            outs.append((idf, e.get_W(), e.get_T(), np.array([obj, off]), e.X_times(np.ones((d, 2)))))
    for u, v in zip(*outs):
        assert np.array_equal(u, v)


def test_upload_clears_and_a_second_preprocessing_is_refused():
    X, U = counts_with_zero_total_rows('57x33')
    n, d = X.shape
    df = np.empty(d)
    ones = np.ones(d)
    count = C.c_int64(0)
    ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    with engine(n, d, 3, dtype=np.float64, sparse_x=True) as e:
        e.upload_X_csr(X)
        e.preprocess(tfidf=True, normalize=True, uniform_rows=True)
        assert np.array_equal(e.uniform_rows()[0], U)
        before = via_row_copy(e)
        for call in (lambda: e.preprocess(tfidf=True, normalize=True, uniform_rows=True), lambda: e.preprocess(normalize=True),
                     lambda: e.preprocess(tfidf=ones),
                     lambda: e._check(e._lib.rri_csr_column_positive_counts(e._h, ptr(df))),
                     lambda: e._check(e._lib.rri_csr_scale_X(e._h, ptr(ones), 1, C.byref(count))),
                     lambda: e._check(e._lib.rri_csr_scale_X_uniform(e._h, ptr(ones), 0, C.byref(count)))):
            with pytest.raises(ValueError, match='uniform rows'):
                call()
        assert np.array_equal(via_row_copy(e), before) and np.array_equal(via_column_copy(e), before)
        assert np.array_equal(e.uniform_rows()[0], U) and e.uniform_rows()[1] == 1.0 / d
        # a new X has no uniform rows, and is preprocessed like any other
        e.upload_X_csr(X)
        assert e.uniform_rows()[0].size == 0 and e.uniform_rows()[1] == 0.0
        assert np.array_equal(via_row_copy(e), X.toarray())
        e.preprocess(tfidf=True, normalize=True, uniform_rows=True)
        assert np.array_equal(via_row_copy(e), before)


def test_a_changed_list_drops_what_the_handle_cached():
    """||X||^2, the carried sums, the cross terms and X T^T all belong to the X with the old list"""
    S, U = stored_S('57x33')
    n, d = S.shape
    U2 = np.array([3, 30, 31], dtype=np.int32)
    D1, D2 = dense_of(S, U, 0.37), dense_of(S, U, 0.37)
    D2[U2, :] = 1.5
    D2[np.setdiff1d(U, U2), :] = 0.0                 # rows of the replaced list stay rows of zeros
    W0, T0 = start(D1, 4, False)
    with engine(n, d, 4, dtype=np.float64, sparse_x=True) as e:
        e.upload_X_csr(S)
        e.set_uniform_rows(U, 0.37)
        e.set_W(W0); e.set_T(T0); e.set_params()
        e.sweep(1)
        assert abs(e.objective() - oracle().true_objective(D1, e.get_W(), e.get_T())) <= 1e-11 * e.objective()
        W1, T1 = e.get_W(), e.get_T()
        e.set_uniform_rows(U2[::-1], 1.5)            # unsorted: kept sorted
        assert np.array_equal(e.uniform_rows()[0], U2) and e.uniform_rows()[1] == 1.5
        want = oracle().true_objective(D2, W1, T1)
        assert abs(e.objective() - want) <= 1e-11 * want
        e.sweep(2)
        ref = run_oracle(D2, W1, T1, 2)
        assert relfro(e.get_W(), ref['W']) < TOL and relfro(e.get_T(), ref['T']) < TOL
        # ... and with T fixed: X T^T of the old list must not be reused
        e.set_params(fix_T=True)
        e.sweep(1)
        Wf, Tf = e.get_W(), e.get_T()
        e.set_uniform_rows(U, 0.37)
        e.sweep(1)
        ref = run_oracle(D1 * (1.0 - np.isin(np.arange(n), np.setdiff1d(U2, U))[:, None]), Wf, Tf, 1, fix_T=True)
        assert relfro(e.get_W(), ref['W']) < TOL


def test_bad_arguments_change_nothing():
    S, U = stored_S('57x33')
    n, d = S.shape
    B = np.random.RandomState(1).rand(d, 3)
    with engine(n, d, 3, dtype=np.float64, sparse_x=True) as e:
        with pytest.raises(ValueError, match='rri_upload_X_csr'):
            e.set_uniform_rows([1], 0.5)                             # before an upload
        e.upload_X_csr(S)
        e.set_uniform_rows(U, 0.37)
        before = e.X_times(B)
        for rows, value, word in (([1, 2, 1], 0.5, 'twice'), ([-1], 0.5, 'out of range'), ([n], 0.5, 'out of range'),
                                  ([1], np.nan, 'finite'), ([1], np.inf, 'finite'), ([], -np.inf, 'finite'),
                                  ([2 ** 32 + 1], 0.5, 'out of range'),      # (row 1, were it wrapped into int32)
                                  (np.array([2 ** 32 + 1], dtype=np.uint64), 0.5, 'out of range'), ([1.0], 0.5, 'integers')):
            with pytest.raises(ValueError, match=word):
                e.set_uniform_rows(rows, value)
            got, c = e.uniform_rows()
            assert np.array_equal(got, U) and c == 0.37
        assert np.array_equal(e.X_times(B), before)
        with pytest.raises(ValueError):                              # a list too long for the caller's buffer
            small = np.empty(2, dtype=np.int32)
            e._check(e._lib.rri_get_uniform_rows(e._h, small.ctypes.data_as(C.POINTER(C.c_int32)), 2, None, None))
    dense = S.toarray()
    for kw, load in ((dict(), lambda g: g.upload_X(dense)), (dict(dtype=np.uint8), lambda g: g.upload_X(np.round(dense * 4))),
                     (dict(weighted='sparse'), lambda g: g.upload_observed_csr(S))):
        with engine(n, d, 3, **dict(dict(dtype=np.float64), **kw)) as g:
            load(g)
            with pytest.raises(ValueError, match='RRI_UNWEIGHTED_SPARSE'):
                g.set_uniform_rows([1], 0.5)
            with pytest.raises(ValueError, match='RRI_UNWEIGHTED_SPARSE'):
                g.uniform_rows()
            with pytest.raises(ValueError):
                g.preprocess(normalize=True, uniform_rows=True)


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------
TM_KW = dict(max_iter=6, random_state=0, project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0, compute_obj_each_iter=True)


def corpus_with_zero_total_rows(kind='empty', n=240, seed=21):
    """(counts, the rows normalisation makes uniform).  'empty': an empty document (row 7) and one that stores a single explicit
    zero (row 11); 'universal': no empty document, and row 11 holds only the term every document holds, whose idf is 0"""
    X = corpus(n=n, seed=seed).tolil()
    if kind == 'universal':
        X[:, UNIVERSAL] = 1
        X[11, :] = 0
        X[11, UNIVERSAL] = 4
        return X.tocsr(), [11]
    X[7, :] = 0
    X[11, :] = 0
    A = X.tocoo()
    rows, cols, vals = np.append(A.row, 11), np.append(A.col, UNIVERSAL), np.append(A.data, 0.0)
    order = np.lexsort((cols, rows))
    X = sp.csr_matrix((vals[order], cols[order].astype(np.int32), np.searchsorted(rows[order], np.arange(n + 1)).astype(np.int64)),
                      shape=X.shape)
    assert np.diff(X.indptr)[7] == 0 and np.diff(X.indptr)[11] == 1
    return X, [7, 11]


@pytest.mark.parametrize('kind', ['empty', 'universal'])
def test_nmf_keeps_the_device_route_and_the_resident_handle(kind, caplog, monkeypatch):
    """the factorisation on the device route against the host route: the 1e-8 tests/test_preprocess_gpu.py allows"""
    from rri_nmf_amd import nmf as nmf_mod
    X, uniform = corpus_with_zero_total_rows(kind)
    n, d = X.shape
    ref, _ = host_reference(X, True, True)
    assert np.array_equal(np.nonzero(np.all(ref == 1.0 / d, axis=1))[0], uniform)
    rs = np.random.RandomState(5)
    W0, T0 = rs.rand(n, 4), rs.rand(4, d)
    T0 /= T0.sum(1, keepdims=True)
    kw = dict(TM_KW, W_in=W0, T_in=T0, sparse_X=True, preprocess=('tfidf', 'normalize'))
    a = nmf_mod.nmf(X, 4, **kw)                                  # the host route
    made = []
    real = nmf_mod.RRIEngine

    class Recording(real):
        def __init__(self, *args, **kws):
            made.append(bool(kws.get('sparse_x', False)))
            super().__init__(*args, **kws)

    monkeypatch.setattr(nmf_mod, 'RRIEngine', Recording)
    holder = nmf_mod.ResidentProblem()
    with caplog.at_level(logging.INFO, logger=nmf_mod.logger.name):
        b = nmf_mod.nmf(X, 4, uniform_rows=True, resident=holder, **kw)
    assert made == [True]
    assert not any('preprocessing on the host instead' in r.getMessage() for r in caplog.records)
    assert np.array_equal(b['idf'], a['idf'])
    print('relfro W %.3g T %.3g' % (relfro(b['W'], a['W']), relfro(b['T'], a['T'])))
    assert relfro(b['W'], a['W']) < 1e-8 and relfro(b['T'], a['T']) < 1e-8
    assert np.allclose(b['obj_history'], a['obj_history'], rtol=1e-10)
    assert holder.engine is not None and holder.reuses == 0
    assert np.array_equal(holder.engine.uniform_rows()[0], uniform) and holder.engine.uniform_rows()[1] == 1.0 / d
    b2 = nmf_mod.nmf(X, 4, uniform_rows=True, resident=holder, **kw)
    assert made == [True] and holder.reuses == 1
    assert np.array_equal(b2['W'], b['W']) and np.array_equal(b2['T'], b['T'])
    holder.close()


def test_estimator_end_to_end():
    """fit, one_iter and transform with the option against the same steps without it (the host route):
    test_sparse_x_gpu.py::test_estimator_end_to_end's bound, 1e-9"""
    from rri_nmf_amd.sklearn_interface import NMF_TM_Estimator
    X, uniform = corpus_with_zero_total_rows()
    Xte, _ = corpus_with_zero_total_rows(n=60, seed=33)
    n, d = X.shape
    res = []
    for extra in ({'uniform_rows': True}, {}):
        est = NMF_TM_Estimator(n, d, 4, handle_tfidf=True, handle_normalization=True, max_iter=8, random_state=3,
                               keep_resident=True, nmf_kwargs=dict({'sparse_X': True, 'device_init': True}, **extra))
        est.fit(X)
        W1, T1 = np.asarray(est.W).copy(), np.asarray(est.T).copy()
        est.one_iter(X)
        W2, T2 = np.asarray(est.W).copy(), np.asarray(est.T).copy()
        if extra:
            assert est._resident is not None and est._resident.reuses == 1 and est._resident.engine.sparse_x
            assert np.array_equal(est._resident.engine.uniform_rows()[0], uniform)
        else:
            assert est._resident is None
        Wte = est.transform(Xte)
        assert Wte.shape == (60, 4) and np.all(np.isfinite(Wte))
        res.append((W1, T1, W2, T2, Wte))
        est.release()
    for a, b in zip(res[0], res[1]):
        assert relfro(a, b) < 1e-9, relfro(a, b)
