"""The unweighted flavour with X kept as CSR on the device (RRI_UNWEIGHTED_SPARSE, nmf(..., sparse_X=True)): the reference's
vectors, the dense handle on the same X and start, the CPU oracle on X.toarray(), resets, shapes that stress the blocked
layout, determinism, the topic-model estimator, and a matrix whose dense form does not fit the device at all."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import load_golden, relfro
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu

TOL = {np.float64: 2e-9, np.float32: 2e-9}
TM = dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def oracle():
    from oracle import rri_oracle
    return rri_oracle


def stored(X, dtype):
    X = X.toarray() if sp.issparse(X) else np.asarray(X)
    return np.ascontiguousarray(X.astype(dtype).astype(np.float64))


def run_oracle(X, W0, T0, sweeps, **kw):
    return oracle().nmf(X, W0.shape[1], W_in=W0.copy(), T_in=T0.copy(), max_iter=sweeps, eps_stop=-1, **kw)


def run(X, W0, T0, sweeps, dtype, sparse_x=True, final_proj=None, objectives=False, **params):
    """sweeps on a handle that keeps X as CSR (sparse_x) or densifies it; W, T, resets used, objective after every sweep"""
    n, d = X.shape
    with engine(n, d, W0.shape[1], dtype=dtype, sparse_x=sparse_x) as e:
        e.upload_X_csr(sp.csr_matrix(X))
        e.set_W(np.maximum(W0, 0))
        e.set_T(np.maximum(T0, 0))
        e.set_params(**params)
        obj = []
        for _ in range(sweeps if objectives else 1):
            e.sweep(1 if objectives else sweeps)
            if objectives:
                obj.append(e.objective())
        if final_proj is not None:
            e.project_W_rows(final_proj)
        return e.get_W(), e.get_T(), e.n_resets_used, obj


def sparsified(n, d, k, density, seed):
    """planted_X with all but `density` of its entries zeroed: a CSR matrix of nonnegative counts-like values"""
    X = planted_X(n, d, k, seed=seed, dtype=np.float64)
    keep = np.random.RandomState(seed + 1).rand(n, d) < density
    return sp.csr_matrix(X * keep)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_text_fixture_on_sparse_handle(dtype):
    """the reference's text fixture as CSR: vectors after 1, 2, 10 sweeps, exact topic assignments, the fold-in"""
    g = load_golden('g1_tm_estimator')
    X = sp.csr_matrix(g['X'])
    W0, T0 = g['W0'], g['T0']
    for S in (1, 2, 10):
        W, T, _, _ = run(X, W0, T0, S, dtype, final_proj=1.0, **TM)
        ref = run_oracle(stored(X, dtype), W0, T0, S, **TM)
        assert relfro(W, ref['W']) < TOL[dtype] and relfro(T, ref['T']) < TOL[dtype]
        if dtype == np.float64:
            assert relfro(W, g['W_s%d' % S]) < TOL[dtype] and relfro(T, g['T_s%d' % S]) < TOL[dtype]
    assert np.array_equal(np.argmax(W, 1), g['argmax_s10'])
    Wte, Tte, nres, _ = run(sp.csr_matrix(g['Xte']), g['Wte0'], g['T_s10'], 4, dtype, final_proj=1.0, fix_T=True,
                            t_row_sum=1.0, w_row_sum=1.0)
    assert nres == 0 and np.array_equal(Tte, g['T_s10'])
    assert relfro(Wte, g['Wte']) < (TOL[dtype] if dtype == np.float64 else 1e-6)
    assert np.array_equal(np.argmax(Wte, 1), g['argmax_te'])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('setting', ['plain', 'topic_model', 'regularised', 'fix_W', 'fix_T'])
def test_against_dense_handle(setting, dtype):
    """the same X and start on the densifying handle: factors and objective histories within 1e-10"""
    g = load_golden('g5_plain_a')
    n, d, k = [int(v) for v in g['shape']]
    X = sparsified(n, d, k, 0.08, seed=0)
    W0, T0 = scaled_init(X.toarray(), k, seed=1)
    params = {'plain': {}, 'topic_model': dict(TM), 'regularised': dict(reg_w_l1=0.01, reg_w_l2=0.02, reg_t_l1=0.01, reg_t_l2=0.03),
              'fix_W': dict(fix_W=True), 'fix_T': dict(fix_T=True)}[setting]
    if setting == 'topic_model':
        T0 = oracle().proj_rows_simplex(np.maximum(T0, 0).copy(), 1.0)
    Ws, Ts, ns, os_ = run(X, W0, T0, 6, dtype, sparse_x=True, objectives=True, **params)
    Wd, Td, nd, od = run(X, W0, T0, 6, dtype, sparse_x=False, objectives=True, **params)
    assert ns == nd
    assert relfro(Ws, Wd) < 1e-10 and relfro(Ts, Td) < 1e-10, (relfro(Ws, Wd), relfro(Ts, Td))
    assert np.allclose(os_, od, rtol=1e-10, atol=0), (os_, od)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_objective_off_the_sweep(dtype):
    """the objective where no complete sweep left its cross terms: the pattern's residual plus the Gram term"""
    X = sparsified(500, 300, 5, 0.05, seed=3)
    W0, T0 = scaled_init(X.toarray(), 5, seed=4)
    with engine(500, 300, 5, dtype=dtype, sparse_x=True) as e:
        e.upload_X_csr(X)
        e.set_W(W0); e.set_T(T0)
        e.set_params(reg_w_l1=0.3, reg_w_l2=0.1, reg_t_l1=0.4, reg_t_l2=0.2)
        got = e.objective()
    want = oracle().true_objective(stored(X, dtype), W0, T0, 0.1, 0.2, 0.3, 0.4)
    assert abs(got - want) <= 1e-11 * abs(want)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_resets_against_oracle(dtype):
    """g6's 'max_resid_document' and 'random' resets on the CSR handle: the same topics reset, the same factors"""
    g = load_golden('g6_rare_branches')
    n, d, k = [int(v) for v in g['shape']]
    X = sp.csr_matrix(planted_X(n, d, k, seed=3, dtype=np.float64))
    W0, T0 = scaled_init(X.toarray(), k, seed=4)
    tol = TOL[dtype] if dtype == np.float64 else 2e-5
    Wd = g['dead_W0']
    W, T, nres, _ = run(X, Wd, T0, 2, dtype, t_row_sum=1.0)
    assert nres >= 1 and relfro(T, g['dead_mrd_T']) < tol and relfro(W, g['dead_mrd_W']) < tol
    W, T, nres, _ = run(X, W0, T0, 1, dtype, t_row_sum=1.0, reg_w_l1=1e6)
    assert nres == k and relfro(T, g['l1killW_mrd_T']) < tol and relfro(W, g['l1killW_mrd_W']) < tol
    W, T, nres, _ = run(X, W0, T0, 1, dtype, t_row_sum=1.0, reg_w_l1=1e6, reset_topic_method='random', fix_reset_seed=True)
    assert nres == k and relfro(T, g['l1killW_rnd_T']) < max(tol, 1e-7) and relfro(W, g['l1killW_rnd_W']) < max(tol, 1e-7)
    # and against the oracle on a truly sparse X: the reset row is max(X - W T, 0), zero off the pattern
    Xs = sparsified(400, 250, 4, 0.1, seed=9)
    W0s, T0s = scaled_init(Xs.toarray(), 4, seed=10)
    W0s[:, 2] = 0.0
    W, T, nres, _ = run(Xs, W0s, T0s, 2, dtype, t_row_sum=1.0)
    ref = run_oracle(stored(Xs, dtype), W0s, T0s, 2, t_row_sum=1.0)
    assert nres >= 1 and relfro(W, ref['W']) < TOL[dtype] and relfro(T, ref['T']) < TOL[dtype]


def _zipf_csr(n, d, per_row, heavy_share, seed):
    """term counts: one column holds `heavy_share` of all entries, the rest Zipf over the columns"""
    rs = np.random.RandomState(seed)
    rows, cols = [], []
    p = 1.0 / np.arange(1, d + 1) ** 1.1
    p /= p.sum()
    for i in range(n):
        c = np.unique(rs.choice(d, size=per_row, p=p))
        if rs.rand() < heavy_share:
            c = np.union1d(c, [d // 3])
        rows.append(np.full(c.size, i)); cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rs.randint(1, 6, size=rows.size).astype(np.float64)
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, d))


SHAPES = {
    # empty rows and columns, explicit stored zeros
    'empty_and_zeros': lambda: _with_zeros(sparsified(300, 200, 4, 0.03, seed=21)),
    # d wider than one column block (15296 columns of float64 factors)
    'wide': lambda: sparsified(120, 40000, 4, 0.004, seed=22),
    # n taller than one row block
    'tall': lambda: sparsified(40000, 80, 4, 0.05, seed=23),
    # one column holds ~30 % of all entries
    'zipf': lambda: _zipf_csr(3000, 2000, 2, 0.9, seed=24),
}


def _with_zeros(X):
    X = X.tolil()
    X[5, :] = 0                        # an empty row
    X[:, 7] = 0                        # an empty column
    X = X.tocsr()
    X.eliminate_zeros()
    A = X.tocoo()
    rows = np.concatenate([A.row, [10, 11, 12]])
    cols = np.concatenate([A.col, [3, 4, 199]])
    vals = np.concatenate([A.data, [0.0, 0.0, 0.0]])   # explicit zeros stay stored
    order = np.lexsort((cols, rows))
    return sp.csr_matrix((vals[order], cols[order], np.searchsorted(rows[order], np.arange(X.shape[0] + 1))), shape=X.shape)


@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('k', [1, 5, 64])
def test_layout_shapes_against_oracle(shape, k):
    X = SHAPES[shape]()
    if shape == 'zipf':
        share = np.bincount(X.indices, minlength=X.shape[1]).max() / X.nnz
        assert share > 0.25
    n, d = X.shape
    W0, T0 = scaled_init(X.toarray() + 1e-3, k, seed=31)
    for dtype in (np.float64, np.float32):
        ref = run_oracle(stored(X, dtype), W0, T0, 3, t_row_sum=1.0)
        W, T, _, _ = run(X, W0, T0, 3, dtype, t_row_sum=1.0)
        assert relfro(W, ref['W']) < TOL[dtype] and relfro(T, ref['T']) < TOL[dtype], (shape, k, dtype)


def test_unsorted_indices_are_sorted_by_the_library():
    """CSR arrays with unsorted column indices in a row go in as they are (rri_upload_X_csr sorts them); duplicates are refused"""
    from rri_nmf_amd.engine import RRIEngine
    X = sparsified(200, 150, 3, 0.1, seed=41)
    perm_rows = X.copy()
    for i in range(perm_rows.shape[0]):
        a, b = perm_rows.indptr[i], perm_rows.indptr[i + 1]
        perm_rows.indices[a:b] = perm_rows.indices[a:b][::-1].copy()
        perm_rows.data[a:b] = perm_rows.data[a:b][::-1].copy()
    perm_rows.has_sorted_indices = False
    W0, T0 = scaled_init(X.toarray(), 3, seed=42)
    outs = []
    for A in (X, perm_rows):
        with engine(200, 150, 3, dtype=np.float64, sparse_x=True) as e:
            keep, args = RRIEngine._csr_args_raw(A)
            e._check(e._lib.rri_upload_X_csr(e._h, *args))
            e.set_W(W0); e.set_T(T0); e.set_params()
            e.sweep(3)
            outs.append((e.get_W(), e.get_T()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    dup = sp.csr_matrix((np.array([1.0, 2.0]), np.array([3, 3]), np.array([0, 2] + [2] * 199)), shape=(200, 150))
    with engine(200, 150, 3, dtype=np.float64, sparse_x=True) as e:
        keep, args = RRIEngine._csr_args_raw(dup)
        with pytest.raises(ValueError, match='twice'):
            e._check(e._lib.rri_upload_X_csr(e._h, *args))


def test_refusals_of_the_handle():
    X = sparsified(100, 80, 3, 0.1, seed=51)
    with engine(100, 80, 3, dtype=np.float32, sparse_x=True) as e:
        e.upload_X_csr(X)
        with pytest.raises(NotImplementedError, match='CSR'):
            e.upload_X(X.toarray())
        with pytest.raises(NotImplementedError, match='CSR'):
            e.upload_mask(np.ones((100, 80)))
        with pytest.raises(NotImplementedError):
            e.range_finder(np.ones((80, 4)), 1)
        with pytest.raises(ValueError):
            e.column_positive_counts()
        assert e.onchip_info()[0] is False          # never the persistent on-chip launch


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_twenty_sweeps_are_bit_identical(dtype):
    X = _zipf_csr(4000, 3000, 12, 0.3, seed=61)
    W0, T0 = scaled_init(X.toarray() + 1e-3, 10, seed=62)
    a = run(X, W0, T0, 20, dtype, objectives=True, **TM)
    b = run(X, W0, T0, 20, dtype, objectives=True, **TM)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]


def test_products_for_the_start():
    """rri_X_times / rri_Xt_times on the CSR (the randomized SVD behind NNDSVD), more than 64 columns in chunks"""
    X = sparsified(700, 500, 4, 0.05, seed=71)
    B = np.random.RandomState(72).rand(500, 70)
    Q = np.random.RandomState(73).rand(700, 70)
    with engine(700, 500, 4, dtype=np.float64, sparse_x=True) as e:
        e.upload_X_csr(X)
        assert relfro(e.X_times(B), X @ B) < 1e-13
        assert relfro(e.Xt_times(Q), X.T @ Q) < 1e-13


def test_estimator_end_to_end():
    """NMF_TM_Estimator with tf-idf and normalisation: fit, one_iter and transform on CSR agree with the dense route; the
    NNDSVD start runs on the device"""
    from rri_nmf_amd.sklearn_interface import NMF_TM_Estimator
    g = load_golden('g1_tm_estimator')
    X = sp.csr_matrix(g['X'])
    Xte = sp.csr_matrix(g['Xte'])
    n, d = X.shape
    res = []
    for kw in ({'sparse_X': True, 'device_init': True}, {'device_init': True}):
        est = NMF_TM_Estimator(n, d, 5, handle_tfidf=True, handle_normalization=True, max_iter=15, random_state=3,
                               nmf_kwargs=dict(kw))
        est.fit(X)
        W1, T1 = np.asarray(est.W).copy(), np.asarray(est.T).copy()
        est.one_iter(X)
        W2, T2 = np.asarray(est.W).copy(), np.asarray(est.T).copy()
        res.append((W1, T1, W2, T2, est.transform(Xte)))
    for a, b in zip(res[0], res[1]):
        assert relfro(a, b) < 1e-9, relfro(a, b)


def test_nmf_routes_sparse_X_to_the_csr_handle(monkeypatch):
    """nmf(X_csr, k, sparse_X=True) takes the CSR handle and agrees with the default (densifying) route"""
    from rri_nmf_amd import nmf as nmf_mod
    made = []
    real = nmf_mod.RRIEngine

    class Recording(real):
        def __init__(self, *a, **kw):
            made.append(bool(kw.get('sparse_x', False)))
            super().__init__(*a, **kw)

    monkeypatch.setattr(nmf_mod, 'RRIEngine', Recording)
    X = sparsified(600, 400, 5, 0.05, seed=81)
    W0, T0 = scaled_init(X.toarray(), 5, seed=82)
    kw = dict(W_in=W0, T_in=T0, max_iter=5, eps_stop=-1, compute_obj_each_iter=True, **TM)
    a = nmf_mod.nmf(X, 5, sparse_X=True, **kw)
    assert made == [True]
    b = nmf_mod.nmf(X, 5, **kw)
    assert made[-1] is False
    assert relfro(a['W'], b['W']) < 1e-10 and relfro(a['T'], b['T']) < 1e-10
    assert np.allclose(a['obj_history'], b['obj_history'], rtol=1e-10, atol=0)
    assert abs(a['obj_calculator'].true_objective() - b['obj_calculator'].true_objective()) <= 1e-10 * abs(b['obj_history'][-1])
    # a dense X with sparse_X=True is converted
    c = nmf_mod.nmf(X.toarray(), 5, sparse_X=True, **kw)
    assert made[-1] is True and relfro(c['W'], a['W']) < 1e-12


def test_matrix_larger_than_the_device(monkeypatch):
    """a CSR X whose dense form exceeds the device's total memory: the default route keeps it sparse, and it runs"""
    import torch
    from rri_nmf_amd import nmf as nmf_mod
    total = torch.cuda.mem_get_info(0)[1]
    d, per_row, k = 100000, 20, 8
    n = max(3000000, int(1.2 * total / (4 * d)) + 1)
    assert float(n) * d * 4 > total
    rs = np.random.RandomState(91)
    base = rs.randint(0, d, size=n).astype(np.int64)
    cols = np.sort((base[:, None] + np.arange(per_row, dtype=np.int64)[None, :] * 4999) % d, axis=1).astype(np.int32)
    vals = rs.randint(1, 8, size=n * per_row).astype(np.float32)
    X = sp.csr_matrix((vals, cols.ravel(), np.arange(0, n * per_row + 1, per_row, dtype=np.int64)), shape=(n, d))
    made = []
    real = nmf_mod.RRIEngine

    class Recording(real):
        def __init__(self, *a, **kw):
            made.append(bool(kw.get('sparse_x', False)))
            super().__init__(*a, **kw)

    monkeypatch.setattr(nmf_mod, 'RRIEngine', Recording)
    W0 = rs.rand(n, k) / k
    T0 = rs.rand(k, d)
    T0 /= T0.sum(1, keepdims=True)
    out = nmf_mod.nmf(X, k, W_in=W0, T_in=T0, max_iter=3, eps_stop=-1, compute_obj_each_iter=True, **TM)
    assert made == [True]          # never the densifying handle
    assert np.all(np.isfinite(out['W'])) and np.all(np.isfinite(out['T']))
    o = out['obj_history']
    assert len(o) == 3 and all(np.isfinite(o))
    if out['n_resets_used'] == 0:  # (a reset may raise the objective, nmf.py:762-816)
        assert all(o[i + 1] <= o[i] * (1 + 1e-12) for i in range(len(o) - 1)), o
