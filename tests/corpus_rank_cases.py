"""What the corpus-ranking tests share (no GPU needed to import): a numpy restatement of rri_nmf_amd/csrc/rri_corpus_rank.hpp -- the
pieces per corpus row, the row terms with the lane rule, the totals with their fixed tree --, NMF_RS_Estimator.ranking_score's own
host arithmetic fed given ranks, the bound that holds the two routes together, and the edge case of the GPU tests.

The restatement is bit for bit the header's plain loop: the same table (1 / log2(p + 2) through the C library's log2, a running
sum), the same order of every floating addition, IEEE divisions of exactly converted integers.
"""
import math

import numpy as np
import scipy.sparse as sp

TERMS, OUT, SUM_ROWS, SEG = 12, 16, 1024, 64
METRICS = ('hit_rate', 'precision', 'recall', 'ndcg', 'mrr', 'auc', 'mean_percentile_rank')
COUNTS = ('n_items', 'users', 'targets', 'targets_not_eligible')


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


# ---- the pieces ------------------------------------------------------------------------------------------------------------------
def pieces(indptr):
    """(req, t0, cnt, first) per piece: at most 64 entries of one row, in order; a row without entries has none"""
    out = []
    for r in range(len(indptr) - 1):
        for t0 in range(int(indptr[r]), int(indptr[r + 1]), SEG):
            out.append((r, t0, min(SEG, int(indptr[r + 1]) - t0), int(t0 == indptr[r])))
    return out


# ---- the table and the trees -------------------------------------------------------------------------------------------------------
def table(n_items, d):
    m = min(int(n_items), int(d))
    tab = np.array([1.0 / math.log2(p + 2.0) for p in range(m)], dtype=np.float64)
    ideal = np.zeros(m + 1)
    for p in range(m):
        ideal[p + 1] = ideal[p] + tab[p]
    return tab, ideal


def tree64(s):
    """s: (..., 64) -> (...): s[l] += s[l + off] for off = 32 .. 1"""
    s = np.array(s, dtype=np.float64)
    off = 32
    while off >= 1:
        s = s[..., :off] + s[..., off:2 * off]
        off //= 2
    return s[..., 0]


def tree256(s):
    """s: (..., 256) -> (...): the four waves' trees, then (w0 + w1) + (w2 + w3)"""
    w = tree64(np.reshape(s, np.shape(s)[:-1] + (4, 64)))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


# ---- the row terms -----------------------------------------------------------------------------------------------------------------
def row_terms(indptr, values, rank, eligible, n_items, relevant_from, d):
    """(rows, 12) float64: what crank_rows_plain leaves"""
    tab, ideal = table(n_items, d)
    m = len(indptr) - 1
    out = np.zeros((m, TERMS))
    N = int(n_items)
    for r in range(m):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        v, rk = np.asarray(values[lo:hi], dtype=np.float64), np.asarray(rank[lo:hi], dtype=np.int64)
        rel = np.ones(hi - lo, dtype=bool) if relevant_from is None or relevant_from != relevant_from else v >= relevant_from
        ok = rel & (rk >= 0)
        T, P = int(rel.sum()), int(ok.sum())
        out[r, 1], out[r, 2] = float(T), float(T - P)
        if P < 1:
            continue
        hit = ok & (rk < N)
        lanes = np.zeros(64)
        for e in np.flatnonzero(hit):                     # ascending: lane e % 64 adds its entries in order
            lanes[e % 64] = lanes[e % 64] + tab[rk[e]]
        dcg = float(tree64(lanes))
        hits, S, L = int(hit.sum()), int(rk[ok].sum()), int(eligible[r])
        out[r, 0] = 1.0
        out[r, 3] = 1.0 if hits > 0 else 0.0
        out[r, 4] = np.float64(hits) / np.float64(N)
        out[r, 5] = np.float64(hits) / np.float64(P)
        out[r, 6] = np.float64(dcg) / ideal[min(N, P)]
        out[r, 7] = np.float64(1.0) / np.float64(1 + int(rk[ok].min()))
        if L > P:
            out[r, 8] = np.float64(1.0) - np.float64(S - P * (P - 1) // 2) / np.float64(P * (L - P))
            out[r, 9] = 1.0
        if L > 1:
            out[r, 10] = np.float64(S) / np.float64(L - 1)
            out[r, 11] = float(P)
    return out


# ---- the totals --------------------------------------------------------------------------------------------------------------------
def _slots(x):
    """x: (items, 12) -> (256, 12): slot t adds the items t, t + 256, ... in ascending order from 0.0"""
    items = x.shape[0]
    rounds = max(1, -(-items // 256))
    pad = np.zeros((rounds * 256, TERMS))
    pad[:items] = x
    s = np.zeros((256, TERMS))
    for k in range(rounds):
        s = s + pad[k * 256:(k + 1) * 256]
    return s


def totals(terms):
    """(16,) float64: what crank_sum_plain leaves"""
    out = np.zeros(OUT)
    m = terms.shape[0]
    if m < 1:
        return out
    nb = -(-m // SUM_ROWS)
    part = np.zeros((nb, TERMS))
    for b in range(nb):
        part[b] = tree256(_slots(terms[b * SUM_ROWS:(b + 1) * SUM_ROWS]).T)
    out[:TERMS] = tree256(_slots(part).T)
    return out


def metrics(sums, n_items):
    """the division: the dict of ranking_score from the 16 sums"""
    from rri_nmf_amd.corpus_rank import metrics_from_sums
    return metrics_from_sums(sums, n_items)


# ---- the parent's host arithmetic, fed given ranks -----------------------------------------------------------------------------------
def host_ranking_score(A, rank, eligible, n_items, relevant_from):
    """NMF_RS_Estimator.ranking_score on the matrix A (canonical CSR, one user per row) with `rank` (per entry, corpus order) and
    `eligible` (per row) standing in for the device: the parent's code path, unchanged"""
    from rri_nmf_amd.sklearn_interface import NMF_RS_Estimator
    n, d = A.shape
    est = NMF_RS_Estimator(n, d, 1, W=np.zeros((n, 1)), T=np.zeros((1, d)))
    key = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr)) * d + A.indices
    rank, eligible = np.asarray(rank, dtype=np.int32), np.asarray(eligible, dtype=np.int32)

    def fed(pairs, exclude_seen=True):
        pairs = np.asarray(pairs, dtype=np.int64)
        at = np.searchsorted(key, pairs[:, 0] * d + pairs[:, 1])
        return rank[at], eligible[pairs[:, 0]]
    est.rank = fed
    return est.ranking_score(A, n_items=n_items, exclude_seen=False, relevant_from=relevant_from)


def bound(users):
    """relative: every term is a non-negative float64 of a few correctly rounded operations -- at most two divisions and a
    subtraction after exact integers, and a dcg of at most 64 additions per lane tree and row, together within 16 ulps --, and the
    two routes differ beyond that only in the order of at most `users` additions of non-negative numbers and one division"""
    return (users + 16) * 2.0 ** -52


def check_metrics(got, want):
    """counts equal; each metric within bound(users) relative; NaN where the other is NaN"""
    for name in COUNTS:
        assert got[name] == want[name], (name, got[name], want[name])
    for name in METRICS:
        g, w = got[name], want[name]
        if w != w or g != g:
            assert w != w and g != g, (name, g, w)
            continue
        err = abs(g - w)
        print('%-22s device %.17g  host %.17g  |diff| %.3e  bound %.3e' % (name, g, w, err, bound(want['users']) * abs(w)))
        assert err <= bound(want['users']) * abs(w), (name, g, w)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def random_case(m, d, seed, lens=None):
    """a targets matrix with star values, ranks and eligible counts that a device could have returned: per row distinct ranks in
    [0, L), some entries not eligible, some rows with L = 0, 1 or P"""
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, min(d - 1, 140), size=m) if lens is None else np.asarray(lens)
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(d, size=l, replace=False)) for l in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    values = rng.randint(1, 6, size=indptr[-1]).astype(np.float64)
    rank = np.full(indptr[-1], -1, dtype=np.int32)
    eligible = np.full(m, -1, dtype=np.int32)
    for r in range(m):
        l = int(lens[r])
        if l == 0:
            continue
        kind = rng.randint(0, 6)
        ok = rng.rand(l) < (0.0 if kind == 0 else 0.8)
        P = int(ok.sum())
        L = P if kind == 1 else (max(P, 1) if kind == 2 else int(rng.randint(P, d + 1)))
        eligible[r] = L if P else int(rng.randint(0, d - l + 1))
        rank[indptr[r]:indptr[r + 1]][ok] = rng.choice(L, size=P, replace=False) if P else []
    A = sp.csr_matrix((values, indices, indptr), shape=(m, d))
    return A, rank, eligible


# the edge case of the GPU tests: n = 150 rows of W, d = 130 columns (two full 64-column chunks and a tail of 2)
N_EDGE, D_EDGE = 150, 130
LENS = (0, 1, 63, 64, 65, 129)
ROW_FULL, ROW_INSIDE, ROW_NAN, TIE = 8, 9, 10, (10, 11)      # rows of W: wholly excluded, a target excluded, a NaN; equal columns of T


def edge_factors(k, seed=0):
    rng = np.random.RandomState(1000 * k + seed)
    W, T = 0.1 + rng.rand(N_EDGE, k), 0.1 + rng.rand(k, D_EDGE)
    T[:, TIE[1]] = T[:, TIE[0]]
    W[ROW_NAN, 0] = np.nan
    return W, T


def edge_targets(seed=1):
    """150 x 130, star values: the rows cycle through 0, 1, 63, 64, 65 and 129 entries -- 200 pieces, four workgroups"""
    rng = np.random.RandomState(seed)
    lens = [LENS[r % 6] for r in range(N_EDGE)]
    rows = [np.sort(rng.choice(D_EDGE, size=l, replace=False)) for l in lens]
    for r in (ROW_INSIDE, ROW_INSIDE + 6):
        if TIE[0] not in rows[r]:                     # the tied columns are targets somewhere
            rows[r][0:2] = TIE
            rows[r] = np.unique(rows[r])
    lens = [len(r) for r in rows]
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    values = rng.randint(1, 6, size=indices.size).astype(np.float64)
    return sp.csr_matrix((values, indices, indptr), shape=(N_EDGE, D_EDGE))


def edge_exclusion(targets, seed=2):
    """150 x 130: a fifth of the columns at random; row ROW_FULL holds every column; row ROW_INSIDE holds its first target"""
    rng = np.random.RandomState(seed)
    M = (rng.rand(N_EDGE, D_EDGE) < 0.2)
    M[ROW_FULL] = True
    M[ROW_INSIDE, targets.indices[targets.indptr[ROW_INSIDE]]] = True
    M[5] = False                                      # and a row that excludes nothing
    E = sp.csr_matrix(M.astype(np.float64))
    E.sort_indices()
    return E


def edge_rows(kind):
    if kind == 'null':
        return None
    rows = np.random.RandomState(3).permutation(N_EDGE).astype(np.int64)
    if kind == 'repeat':
        rows[20] = rows[19]
        rows[2] = ROW_FULL
    return rows
