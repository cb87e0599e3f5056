"""Host side of the sparse range finder (rri_sparse_range_finder): which engines randomized_svd_device sends to it, and the
declaration, the binding and the method that carry it.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import scipy.sparse as sp
from scipy import linalg

from rri_nmf_amd import _capi
from rri_nmf_amd.synthetic import planted_X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sparsified(n, d, k, density, seed):
    """planted_X with all but `density` of its entries zeroed (as in test_sparse_x_gpu.py)"""
    X = planted_X(n, d, k, seed=seed, dtype=np.float64)
    keep = np.random.RandomState(seed + 1).rand(n, d) < density
    return sp.csr_matrix(X * keep)


def _s1():
    X = sparsified(700, 500, 4, 0.05, seed=71).tolil()
    X[:, 7] = 0
    X[11, :] = 0
    X = X.tocsr()
    X.eliminate_zeros()
    return X


class _Products(object):
    """an engine that keeps X sparse and offers the two products only (an older library, a stand-in)"""
    sparse = True

    def __init__(self, X):
        self.X, (self.n, self.d) = X, X.shape
        self.products = 0

    def X_times(self, B):
        self.products += 1
        return self.X @ B

    def Xt_times(self, Q):
        self.products += 1
        return self.X.T @ Q


class _WithRangeFinder(_Products):
    """... and the range finder, as the device runs it: shifted Cholesky-QR in three passes around every product"""
    def __init__(self, X):
        _Products.__init__(self, X)
        self.range_finders = []

    @staticmethod
    def _orth(Y):
        from rri_nmf_amd.initialization import _cholesky_floor
        for rnd in range(3):
            G = Y.T @ Y
            L = _cholesky_floor(0.5 * (G + G.T), 1e-9 if rnd == 0 else 0.0)
            Y = linalg.solve_triangular(L, Y.T, lower=True, check_finite=False).T
        return Y

    def sparse_range_finder(self, Q0, n_iter, transpose=False):
        self.range_finders.append((Q0.shape, int(n_iter), bool(transpose)))
        A = self.X.T.tocsr() if transpose else self.X
        Q = Q0
        for _ in range(n_iter):
            Q = self._orth(A @ Q)
            Q = self._orth(A.T @ Q)
        Q = self._orth(A @ Q)
        return Q, (A.T @ Q).T


def test_an_engine_that_keeps_X_sparse_is_sent_to_its_range_finder():
    from sklearn.utils.extmath import randomized_svd
    from rri_nmf_amd.initialization import randomized_svd_device
    X, k = _s1(), 4
    U0, S0, V0 = randomized_svd(X, k, random_state=3)
    fake = _WithRangeFinder(X)
    U, S, V = randomized_svd_device(fake, k, random_state=3)
    assert fake.range_finders == [((500, 14), 7, False)] and fake.products == 0
    assert np.allclose(S, S0, rtol=1e-10, atol=0)
    assert np.abs(U - U0).max() < 1e-8 and np.abs(V - V0).max() < 1e-8
    # the transposed problem: scikit-learn works on X^T when n < d
    fake = _WithRangeFinder(X.T.tocsr())
    U, S, V = randomized_svd_device(fake, k, random_state=3)
    U0, S0, V0 = randomized_svd(X.T.tocsr(), k, random_state=3)
    assert fake.range_finders == [((500, 14), 7, True)] and fake.products == 0
    assert np.allclose(S, S0, rtol=1e-10, atol=0)
    assert np.abs(U - U0).max() < 1e-8 and np.abs(V - V0).max() < 1e-8
    # more than 64 columns, or resident=False: the products one by one
    fake = _WithRangeFinder(X)
    randomized_svd_device(fake, 55, random_state=3)
    assert fake.range_finders == [] and fake.products == 2 * 4 + 2
    fake = _WithRangeFinder(X)
    U, S, V = randomized_svd_device(fake, k, random_state=3, resident=False)
    assert fake.range_finders == [] and fake.products == 2 * 7 + 2


def test_an_engine_without_the_method_keeps_the_product_route():
    from sklearn.utils.extmath import randomized_svd
    from rri_nmf_amd.initialization import randomized_svd_device
    X, k = _s1(), 4
    fake = _Products(X)
    U, S, V = randomized_svd_device(fake, k, random_state=3)
    assert fake.products == 2 * 7 + 2
    U0, S0, V0 = randomized_svd(X, k, random_state=3)
    assert np.allclose(S, S0, rtol=1e-10, atol=0)
    assert np.abs(U - U0).max() < 1e-8 and np.abs(V - V0).max() < 1e-8


def test_declaration_binding_and_method():
    code = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rri_hip.h')).read(), flags=re.S)
    assert re.search(r'rri_status\s+rri_sparse_range_finder\s*\(\s*rri_ctx\s*\*\s*ctx\s*,\s*const\s+double\s*\*\s*Q0\s*,\s*int32_t\s+m\s*,'
                     r'\s*int32_t\s+n_iter\s*,\s*int32_t\s+transpose\s*,\s*double\s*\*\s*Q_out\s*,\s*double\s*\*\s*B_out\s*\)\s*;', code)
    res, args = _capi.PROTOTYPES['rri_sparse_range_finder']
    PD = C.POINTER(C.c_double)
    assert res is C.c_int32 and len(args) == 7
    assert args == [C.c_void_p, PD, C.c_int32, C.c_int32, C.c_int32, PD, PD]
    assert args == _capi.PROTOTYPES['rri_range_finder'][1]
    from rri_nmf_amd.engine import RRIEngine
    assert callable(RRIEngine.sparse_range_finder)
