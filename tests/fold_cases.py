"""What tests/test_fold_cpu.py and tests/test_fold_gpu.py share: the construction of the fold-in problems, and a numpy restatement
of one sweep of the W half with T fixed (rri_nmf_amd/csrc/rri_fold.hpp)."""
import numpy as np
import scipy.sparse as sp

from rri_nmf_amd.synthetic import planted_X, scaled_init

# (n, d, k, frac): k = 1, the 16 / 17 tile edge, the limit 64, row counts off every multiple, a row longer than any chunk
SHAPES = [(413, 187, 5, 0.2), (70, 40, 1, 0.3), (130, 90, 16, 0.4), (131, 90, 17, 0.4), (200, 150, 64, 0.5), (64, 2100, 4, 0.08)]
FLAGSETS = {'plain': {}, 'regs': dict(reg_w_l1=0.02, reg_w_l2=0.05), 'wrs': dict(w_row_sum=0.7)}
SEED = 3        # with it no column halts on these shapes and flag sets, except (200, 150, 64) without flags: the oracle resets once
EPS_DIV = float(np.spacing(10))     # nmf.py:52, what the engine passes as eps_div


def problem(n, d, k, frac, seed=SEED):
    """(A, X, M, W0, T0): rows 3-6 without entries, row 8 with one, rows 9, 10 and 11 with 63, 64 and 65 (or d, where d is smaller),
    row 12 full; X = planted_X .* M, +0.05 on the observed entries, every 11th observed entry an explicit zero; A is the CSR matrix
    of the observed entries with the zeros kept; T0 inside [0, 1]"""
    rs = np.random.RandomState(seed + 10)
    M = rs.rand(n, d) < frac
    M[3:7, :] = False
    M[8, :] = False
    M[8, 8 % d] = True
    for r, cnt in ((9, 63), (10, 64), (11, 65)):
        M[r, :] = False
        M[r, :min(cnt, d)] = True
    M[12, :] = True
    X = planted_X(n, d, k, seed=seed, dtype=np.float64) * M
    X[M] += 0.05
    obs = np.argwhere(M)
    zero = obs[::11]
    X[zero[:, 0], zero[:, 1]] = 0.0
    W0, T0 = scaled_init(X, k, seed=seed + 1)
    T0 = np.clip(T0, 0.0, 1.0)
    A = sp.csr_matrix((X[M], (obs[:, 0], obs[:, 1])), shape=(n, d))
    assert A.nnz == int(M.sum())
    return A, X, M.astype(np.float64), np.ascontiguousarray(W0), np.ascontiguousarray(T0)


def stored(A, X, store):
    """the CSR matrix and the dense X as a handle of storage type `store` holds them, in float64"""
    As = A.copy()
    As.data = A.data.astype(store).astype(np.float64)
    return As, X.astype(store).astype(np.float64)


def fold_sweep(A, T, W, t0=0, reg_w_l1=0.0, reg_w_l2=0.0, w_row_sum=None, eps=EPS_DIV):
    """One sweep of the W half for topics [t0, k) with T fixed, row by row, through q and G: (W_new, column sums, counts of negative
    denominators).  The formulas of rri_fold.hpp in float64; sums by numpy, so equal to the C loop within rounding only."""
    A = sp.csr_matrix(A)
    n, k = W.shape
    W = np.array(W, dtype=np.float64)
    colsum, negs = np.zeros(k), np.zeros(k)
    for i in range(n):
        lo, hi = A.indptr[i], A.indptr[i + 1]
        Tj = T[:, A.indices[lo:hi]]
        q = Tj @ A.data[lo:hi]
        G = Tj @ Tj.T
        w = W[i]
        s = q - G @ w + np.diag(G) * w
        for t in range(t0, k):
            c = G[t, t] + reg_w_l2
            wn = max(s[t] - reg_w_l1, 0.0) / (c + eps) if c > 0 else 0.0
            if w_row_sum is not None:
                wn = min(wn, w_row_sum)
            dw = wn - w[t]
            w[t] = wn
            s -= G[:, t] * dw
            s[t] += G[t, t] * dw
            colsum[t] += wn
            negs[t] += c < 0
    return W, colsum, negs


def relfro(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))
