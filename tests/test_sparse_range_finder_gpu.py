"""The range finder of the randomized SVD resident on the device for the handles that keep X sparse (rri_sparse_range_finder,
RRIEngine.sparse_range_finder): the CSR X of sparse_x=True and the observed values of a pattern-only handle.  The call against
numpy, the SVD built on it against scikit-learn's, reruns to the bit, a factorisation in progress, a rank-one matrix, what it
refuses, and the route nmf() takes to it.

Thresholds: a numpy Cholesky-QR range finder (initialization._cholesky_floor, three passes) on these matrices stays below
1.1e-15 on orthonormality, 2.2e-15 on both subspace checks and 5e-14 on U, S, V against scikit-learn; the tolerances are those
of the dense call (test_nmf_gpu.py::test_device_products_and_device_init)."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import relfro
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu

TM = dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
FLAVOURS = ('csr', 'pattern')


def sparsified(n, d, k, density, seed):
    """planted_X with all but `density` of its entries zeroed: a CSR matrix of nonnegative counts-like values
    (as in test_sparse_x_gpu.py)"""
    X = planted_X(n, d, k, seed=seed, dtype=np.float64)
    keep = np.random.RandomState(seed + 1).rand(n, d) < density
    return sp.csr_matrix(X * keep)


def _holes(X):
    """column 7 and row 11 emptied: an empty segment in each blocked copy"""
    X = X.tolil()
    X[:, 7] = 0
    X[11, :] = 0
    X = X.tocsr()
    X.eliminate_zeros()
    X.sort_indices()
    return X


def _zipf_csr(n, d, per_row, heavy_share, seed):
    """term counts: one column holds `heavy_share` of all entries, the rest Zipf over the columns (as in test_sparse_x_gpu.py)"""
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


_CASES = {
    'S1': lambda: _holes(sparsified(700, 500, 4, 0.05, seed=71)),       # one block per copy
    'S2': lambda: _holes(sparsified(15400, 300, 5, 0.02, seed=91)),     # the column copy in several row blocks
    'S3': lambda: _holes(sparsified(300, 15400, 5, 0.02, seed=93)),     # the row copy in several column blocks
    'wide': lambda: _holes(sparsified(400, 900, 6, 0.10, seed=81)),
    'zipf': lambda: _holes(_zipf_csr(4000, 3000, 12, 0.3, seed=61)),
}
_K = {'S1': 4, 'S2': 5, 'S3': 5, 'wide': 6, 'zipf': 10}
_cache = {}


def case(name):
    """the CSR matrix of a case, built once and never written to"""
    if name not in _cache:
        _cache[name] = _CASES[name]()
    return _cache[name]


def stored(X, store):
    """the matrix the handle holds, in float64"""
    return X.astype(store).astype(np.float64)


def open_engine(X, k, store, flavour):
    from rri_nmf_amd.engine import RRIEngine
    n, d = X.shape
    if flavour == 'csr':
        e = RRIEngine(n, d, k, dtype=store, sparse_x=True)
        e.upload_X_csr(X)
    else:
        e = RRIEngine(n, d, k, dtype=store, weighted='sparse')
        A = X.copy()
        A.data = A.data.astype(store)
        e.upload_observed_csr(A)
    return e


def _power_panel(A, Q0, n_iter):
    Y = A @ Q0
    for _ in range(n_iter):
        Y = A @ np.linalg.qr(A.T @ np.linalg.qr(Y)[0])[0]
    return Y


@pytest.mark.parametrize('store', [np.float64, np.float32])
@pytest.mark.parametrize('flavour', FLAVOURS)
@pytest.mark.parametrize('name', ['S1', 'S2', 'S3'])
def test_the_call(name, flavour, store):
    """Q orthonormal, B = Q^T A, and the subspace of numpy's power iteration, for A = X and A = X^T"""
    X = case(name)
    Xs = stored(X, store)
    with open_engine(X, _K[name], store, flavour) as e:
        for transpose in (False, True):
            A = (Xs.T if transpose else Xs).tocsr()
            for m in (1, 16, 64):
                Q0 = np.random.RandomState(5).randn(A.shape[1], m)
                for n_iter in (0, 3):
                    Q, B = e.sparse_range_finder(Q0, n_iter, transpose=transpose)
                    assert Q.shape == (A.shape[0], m) and B.shape == (m, A.shape[1])
                    QtA = (A.T @ Q).T
                    Y = _power_panel(A, Q0, n_iter)
                    Qh = np.linalg.qr(Y)[0]
                    QB = Q @ B
                    figs = (np.abs(Q.T @ Q - np.eye(m)).max(), relfro(B, QtA), relfro(Q @ (Q.T @ Y), Y),
                            relfro(Qh @ (Qh.T @ QB), QB))
                    print('%s %s %s transpose=%d m=%d n_iter=%d: orth %.2e  B %.2e  range %.2e / %.2e'
                          % ((name, flavour, np.dtype(store).name, transpose, m, n_iter) + figs))
                    assert figs[0] < 1e-12
                    assert figs[1] < 1e-12
                    # the same subspace: the projectors agree (on what the panel resolves: its smallest directions are noise at
                    # n_iter = 3)
                    assert figs[2] < 1e-10 and figs[3] < 1e-6


@pytest.mark.parametrize('name,flavour', [('S1', 'csr'), ('S1', 'pattern'), ('S2', 'csr'), ('S3', 'csr'), ('wide', 'csr'),
                                          ('zipf', 'csr')])
def test_the_svd(name, flavour):
    """randomized_svd_device on the sparse handle = scikit-learn's randomized_svd of the same CSR matrix, to rounding"""
    from rri_nmf_amd.initialization import randomized_svd_device
    from sklearn.utils.extmath import randomized_svd
    X, k = case(name), _K[name]
    U0, S0, V0 = randomized_svd(X, k, random_state=3)
    with open_engine(X, k, np.float64, flavour) as e:
        U, S, V = randomized_svd_device(e, k, random_state=3)
    print('%s %s: S %.2e  U %.2e  V %.2e' % (name, flavour, np.abs(S / S0 - 1).max(), np.abs(U - U0).max(), np.abs(V - V0).max()))
    assert np.allclose(S, S0, rtol=1e-10, atol=0)
    assert np.abs(U - U0).max() < 1e-8 and np.abs(V - V0).max() < 1e-8


@pytest.mark.parametrize('flavour', FLAVOURS)
def test_a_rerun_gives_the_same_bits(flavour):
    X = case('S2')
    Q0 = np.random.RandomState(5).randn(X.shape[1], 16)
    with open_engine(X, 5, np.float32, flavour) as e:
        Qa, Ba = e.sparse_range_finder(Q0, 3)
        Qb, Bb = e.sparse_range_finder(Q0, 3)
    assert np.array_equal(Qa, Qb) and np.array_equal(Ba, Bb)


@pytest.mark.parametrize('flavour', FLAVOURS)
def test_a_factorisation_in_progress_is_undisturbed(flavour):
    X = case('S1')
    k = 4
    W0, T0 = scaled_init(X.toarray() + 1e-3, k, seed=2)
    params = dict(TM) if flavour == 'csr' else dict(t_row_sum=1.0, reset_topic_method=None)
    Q0 = np.random.RandomState(5).randn(X.shape[1], 16)
    with open_engine(X, k, np.float64, flavour) as e:
        e.set_W(W0), e.set_T(T0)
        e.set_params(**params)
        e.sweep(1)
        e.sparse_range_finder(Q0, 1)
        e.sweep(1)
        Wa, Ta = e.get_W(), e.get_T()
        e.set_W(W0), e.set_T(T0)
        e.sweep(2)
        assert relfro(Wa, e.get_W()) < 1e-13 and relfro(Ta, e.get_T()) < 1e-13


@pytest.mark.parametrize('flavour', FLAVOURS)
def test_rank_deficient_panel(flavour):
    """a rank-one matrix under a 16-column panel: the pivot floor keeps the factor finite, and Q B is still A"""
    u = np.random.RandomState(1).rand(600) * (np.random.RandomState(2).rand(600) < 0.1)
    v = np.random.RandomState(3).rand(400) * (np.random.RandomState(4).rand(400) < 0.1)
    X = sp.csr_matrix(np.outer(u, v))
    assert X.nnz == 2220
    Q0 = np.random.RandomState(5).randn(400, 16)
    with open_engine(X, 3, np.float64, flavour) as e:
        Q, B = e.sparse_range_finder(Q0, 3)
    assert np.all(np.isfinite(Q)) and np.all(np.isfinite(B))
    figs = (relfro(Q @ B, X.toarray()), relfro(B, (X.T @ Q).T))
    print('rank one, %s: Q B %.2e  B %.2e' % ((flavour,) + figs))
    assert figs[0] < 1e-10
    assert figs[1] < 1e-12


def test_refusals():
    from rri_nmf_amd.engine import RRIEngine
    X = case('S1')
    n, d = X.shape
    with RRIEngine(n, d, 4, dtype=np.float64) as e:         # a dense handle
        e.upload_X(X.toarray())
        with pytest.raises(ValueError):
            e.sparse_range_finder(np.ones((d, 4)), 1)
    with RRIEngine(n, d, 4, dtype=np.float64, sparse_x=True) as e:       # before the upload
        with pytest.raises(ValueError):
            e.sparse_range_finder(np.ones((d, 4)), 1)
    for flavour in FLAVOURS:
        with open_engine(X, 4, np.float64, flavour) as e:
            with pytest.raises(ValueError):
                e.sparse_range_finder(np.ones((d, 65)), 1)
            with pytest.raises(ValueError):
                e.sparse_range_finder(np.ones((d + 1, 4)), 1)
            with pytest.raises(ValueError):
                e.sparse_range_finder(np.ones((d, 4)), -1)
            with pytest.raises(NotImplementedError):
                e.range_finder(np.ones((d, 4)), 1)


def _recording(nmf_mod, monkeypatch):
    calls = {'sparse_range_finder': 0, 'range_finder': 0, 'wide_products': 0}
    real = nmf_mod.RRIEngine

    class Recording(real):
        def sparse_range_finder(self, *a, **kw):
            calls['sparse_range_finder'] += 1
            return super().sparse_range_finder(*a, **kw)

        def range_finder(self, *a, **kw):
            calls['range_finder'] += 1
            return super().range_finder(*a, **kw)

        def X_times(self, B):
            calls['wide_products'] += int(np.asarray(B).shape[1] > 1)
            return super().X_times(B)

        def Xt_times(self, Q):
            calls['wide_products'] += int(np.asarray(Q).shape[1] > 1)
            return super().Xt_times(Q)

    monkeypatch.setattr(nmf_mod, 'RRIEngine', Recording)
    return calls


def test_nmf_starts_a_csr_handle_this_way(monkeypatch):
    from rri_nmf_amd import nmf as nmf_mod
    calls = _recording(nmf_mod, monkeypatch)
    X = case('S1')
    kw = dict(sparse_X=True, max_iter=3, random_state=0, eps_stop=-1, **TM)
    a = nmf_mod.nmf(X, 4, device_init=True, **kw)
    assert calls == {'sparse_range_finder': 1, 'range_finder': 0, 'wide_products': 0}
    b = nmf_mod.nmf(X, 4, device_init=False, **kw)
    assert calls['sparse_range_finder'] == 1
    assert relfro(a['W'], b['W']) < 1e-6 and relfro(a['T'], b['T']) < 1e-6, (relfro(a['W'], b['W']), relfro(a['T'], b['T']))
    # k + 10 = 65 columns are more than the call takes: the products one by one, panels normalised on the host
    c = nmf_mod.nmf(X, 55, device_init=True, **kw)
    assert calls['sparse_range_finder'] == 1 and calls['wide_products'] > 0
    assert c['W'].shape == (700, 55) and np.all(np.isfinite(c['W'])) and np.all(np.isfinite(c['T']))


def test_nmf_starts_a_pattern_only_handle_this_way(monkeypatch):
    """the weighted call of test_sparse_wrri_gpu.py::test_products_and_device_init_on_a_pattern_only_handle"""
    from rri_nmf_amd import nmf as nmf_mod
    calls = _recording(nmf_mod, monkeypatch)
    n, d, k = 12500, 310, 5
    M = (np.random.RandomState(12).rand(n, d) < 0.1).astype(np.float64)
    X = planted_X(n, d, k, seed=2, dtype=np.float64) * M
    X[M > 0] += 0.05
    A = sp.csr_matrix(M)
    A.data = X[M > 0]
    kw = dict(max_iter=4, eps_stop=-1, t_row_sum=1.0, reset_topic_method=None, random_state=0)
    a = nmf_mod.nmf(A, k, W_mat=sp.csr_matrix(M), device_init=True, **kw)
    assert calls == {'sparse_range_finder': 1, 'range_finder': 0, 'wide_products': 0}
    b = nmf_mod.nmf(A, k, W_mat=sp.csr_matrix(M), device_init=False, **kw)
    assert calls['sparse_range_finder'] == 1
    assert relfro(a['W'], b['W']) < 1e-6 and relfro(a['T'], b['T']) < 1e-6, (relfro(a['W'], b['W']), relfro(a['T'], b['T']))
