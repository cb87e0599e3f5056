"""Top-N rows: a float64 numpy restatement of the semantics (rri_nmf_amd/csrc/rri_topn.hpp, DESIGN "Top-N rows") and the cases
tests/test_topn_cpu.py and tests/test_topn_gpu.py share.

For a requested row i: the score of column j is s_ij = sum_t W[i, t] T[t, j]; eligible are the columns that the row does not
exclude and whose score is not NaN; the order is larger score first, equal scores by the smaller column; the answer is the first
min(N, eligible) columns of that order and their values, clipped to [lo, hi] (None: open), then index -1 and value NaN."""
import collections

import numpy as np
import scipy.sparse as sp


def ordered(s, eligible):
    """the eligible columns of one row of scores in the order of the semantics: np.lexsort((j, -s))"""
    j = np.flatnonzero(eligible & ~np.isnan(s))
    return j[np.lexsort((j, -s[j]))]


def clip_values(v, clip):
    lo, hi = clip
    v = np.array(v, dtype=np.float64)
    if lo is not None and not np.isnan(lo):
        v = np.maximum(v, lo)
    if hi is not None and not np.isnan(hi):
        v = np.minimum(v, hi)
    return v


def exclusion_mask(exclude, m, d):
    if exclude is None:
        return np.zeros((m, d), dtype=bool)
    E = sp.csr_matrix(exclude)
    out = np.zeros((m, d), dtype=bool)
    rows = np.repeat(np.arange(m), np.diff(E.indptr))
    out[rows, E.indices] = True          # the pattern counts, stored zeros included
    return out


def topn_from_scores(S, n_top, excluded, clip=(None, None)):
    """(idx int32 (m, n_top), val float64 (m, n_top)) of a score matrix S (m, d) and a boolean exclusion mask"""
    m = S.shape[0]
    idx = np.full((m, n_top), -1, dtype=np.int32)
    val = np.full((m, n_top), np.nan)
    for i in range(m):
        J = ordered(S[i], ~excluded[i])[:n_top]
        idx[i, :J.size] = J
        val[i, :J.size] = clip_values(S[i, J], clip)
    return idx, val


def scores(W, T, rows=None):
    W = np.asarray(W, dtype=np.float64)
    return (W if rows is None else W[np.asarray(rows)]) @ np.asarray(T, dtype=np.float64)


def topn_reference(W, T, rows=None, n_top=10, exclude=None, clip=(None, None)):
    S = scores(W, T, rows)
    return topn_from_scores(S, n_top, exclusion_mask(exclude, S.shape[0], S.shape[1]), clip)


def check_real(W, T, rows, n_top, exclude, clip, idx, val):
    """The rules for real-valued factors, every row: with r the restatement's scores and
    tol_i = 2 k 2^-52 max_j (|W[i]| |T|)_j  (two length-k FMA sums taken in different orders each lie within k 2^-53 (|W||T|)_ij
    of the exact sum, to first order; 2 k 2^-52 is four times that)
      - the indices are distinct, eligible, min(N, eligible) of them, padded on the right with -1 / NaN
      - |clip(r[J]) - v| <= tol_i
      - r[J[a]] >= r[J[a+1]] - 2 tol_i
      - min r[J] >= max r[eligible, not returned] - 2 tol_i
    Returns the largest of the three differences over its tolerance, for printing."""
    W = np.asarray(W, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    Wr = W if rows is None else W[np.asarray(rows)]
    R = Wr @ T
    m, d = R.shape
    k = W.shape[1]
    tol = 2.0 * k * 2.0 ** -52 * (np.abs(Wr) @ np.abs(T)).max(axis=1)
    excluded = exclusion_mask(exclude, m, d)
    assert idx.shape == (m, n_top) and val.shape == (m, n_top) and idx.dtype == np.int32 and val.dtype == np.float64
    worst = 0.0
    for i in range(m):
        eligible = ~excluded[i] & ~np.isnan(R[i])
        cnt = min(n_top, int(eligible.sum()))
        J = idx[i, :cnt].astype(np.int64)
        assert np.all(idx[i, cnt:] == -1) and np.all(np.isnan(val[i, cnt:])), (i, idx[i], val[i])
        assert np.all(J >= 0) and np.all(J < d) and np.unique(J).size == cnt and np.all(eligible[J]), (i, J)
        if cnt == 0:
            continue
        t = tol[i]
        e_val = np.abs(clip_values(R[i, J], clip) - val[i, :cnt]).max()
        assert e_val <= t, (i, e_val, t)
        e_ord = float(np.max(R[i, J[1:]] - R[i, J[:-1]], initial=-np.inf))
        assert e_ord <= 2 * t, (i, e_ord, t)
        rest = eligible.copy()
        rest[J] = False
        e_out = float(R[i, rest].max() - R[i, J].min()) if rest.any() else -np.inf
        assert e_out <= 2 * t, (i, e_out, t)
        if t > 0:
            worst = max(worst, e_val / t, e_ord / (2 * t), e_out / (2 * t))
    return worst


# ---- exact cases: W, T integers in 0..7, so every product and every sum is exact in any order, and ties are everywhere -----------
Case = collections.namedtuple('Case', 'k d count n_top excl rows')
# excl: None | 'empty' (a pattern without entries) | 'all' (rows with every column excluded among random ones) |
#       'short' (rows left with fewer than n_top columns among random ones);  rows: None (all rows of W) | 'perm' (a permuted
#       list with duplicates, drawn from a W of 40 rows)
# every k, d, count and n_top of the list below at least once; every tail (d % 16, count % 64, k % 4) with and without exclusion
EXACT_CASES = [
    Case(1, 1, 1, 1, None, None),
    Case(3, 15, 15, 2, None, None),
    Case(4, 16, 16, 10, None, 'perm'),
    Case(5, 17, 17, 64, None, None),           # n_top > d
    Case(64, 257, 64, 64, None, None),
    Case(65, 257, 65, 10, None, 'perm'),
    Case(5, 257, 130, 10, None, None),
    Case(3, 15, 15, 2, 'empty', None),
    Case(5, 17, 17, 10, 'all', 'perm'),
    Case(65, 257, 65, 64, 'short', None),
    Case(4, 16, 64, 2, 'short', None),
    Case(1, 257, 130, 10, 'all', 'perm'),
    Case(64, 17, 1, 20, 'short', None),        # n_top > d
    Case(5, 1, 16, 1, 'all', None),
    Case(3, 257, 65, 64, 'empty', 'perm'),
    Case(4, 15, 17, 10, 'short', 'perm'),
]
K_VALUES, D_VALUES = {1, 3, 4, 5, 64, 65}, {1, 15, 16, 17, 257}
COUNT_VALUES, N_VALUES = {1, 15, 16, 17, 64, 65, 130}, {1, 2, 10, 64}


def case_id(c):
    return 'k%d-d%d-m%d-N%d-%s-%s' % (c.k, c.d, c.count, c.n_top, c.excl or 'noexcl', c.rows or 'allrows')


def make_exclusion(kind, m, d, n_top, seed):
    """a scipy CSR pattern (m, d) of the kind, its column indices DESCENDING inside every row (the caller's arrays need not be
    sorted), or None"""
    if kind is None:
        return None
    rng = np.random.RandomState(seed)
    mask = np.zeros((m, d), dtype=bool) if kind == 'empty' else rng.rand(m, d) < 0.3
    if kind == 'all':
        mask[0] = True
        mask[m // 2] = True
    if kind == 'short':
        left = max(0, min(n_top, d) - 1)                  # columns the last row keeps: fewer than it is asked for
        mask[m - 1] = True
        mask[m - 1, rng.permutation(d)[:left]] = False
        mask[0] = True
        mask[0, rng.permutation(d)[:left // 2]] = False
    A = sp.csr_matrix(mask.astype(np.float64))
    A.sort_indices()
    for i in range(m):
        A.indices[A.indptr[i]:A.indptr[i + 1]] = A.indices[A.indptr[i]:A.indptr[i + 1]][::-1].copy()
    A.has_sorted_indices = False
    return A


def make_exact(c, seed=0):
    """W (n, k), T (k, d) integers in 0..7 as float64, the row list (or None) and the exclusion of a case"""
    rng = np.random.RandomState(1000 + seed)
    n = c.count if c.rows is None else 40
    W = rng.randint(0, 8, size=(n, c.k)).astype(np.float64)
    T = rng.randint(0, 8, size=(c.k, c.d)).astype(np.float64)
    rows = None
    if c.rows is not None:
        rows = rng.permutation(np.arange(c.count) % n).astype(np.int64)
        rows[-1] = rows[0]                                   # a duplicate at every count
    return W, T, rows, make_exclusion(c.excl, c.count, c.d, c.n_top, seed + 7)


def make_real(k, d=257, n=65, seed=0):
    rng = np.random.RandomState(2000 + seed + k)
    return rng.rand(n, k), rng.rand(k, d)
