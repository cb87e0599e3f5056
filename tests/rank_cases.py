"""Ranks of entries: a float64 numpy restatement of the semantics (rri_nmf_amd/csrc/rri_rank.hpp, DESIGN "Ranks of entries"),
the ranking metrics as plain loops, and the cases tests/test_rank_cpu.py and tests/test_rank_gpu.py share.

For request q (a row of W, an exclusion, ascending target columns) and its target column j: rank = the number of eligible columns
j' != j that stand before j in the order of tests/topn_cases.py -- j's 0-based place in an unbounded top-N list --, or -1 when j is
itself not eligible; val = the clipped score of an eligible target, else NaN; eligible = the number of eligible columns."""
import collections
import math

import numpy as np
import scipy.sparse as sp

import topn_cases as tc

Ranks = collections.namedtuple('Ranks', 'indptr indices rank val eligible')


def canonical(A, m, d):
    """sorted, deduplicated CSR pattern (indptr int64, indices int32) of a target or exclusion matrix"""
    A = sp.csr_matrix(A, copy=True)
    assert A.shape == (m, d), (A.shape, m, d)
    A.sum_duplicates()
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int32)


def ranks_from_scores(S, targets, excluded, clip=(None, None)):
    """Ranks of a score matrix S (m, d), a target pattern (m, d) and a boolean exclusion mask"""
    m, d = S.shape
    indptr, indices = canonical(targets, m, d)
    rank = np.empty(indices.size, dtype=np.int32)
    val = np.empty(indices.size, dtype=np.float64)
    eligible = np.empty(m, dtype=np.int32)
    for q in range(m):
        order = tc.ordered(S[q], ~excluded[q])                      # the unbounded list
        place = np.full(d, -1, dtype=np.int64)
        place[order] = np.arange(order.size)
        eligible[q] = order.size
        J = indices[indptr[q]:indptr[q + 1]]
        rank[indptr[q]:indptr[q + 1]] = place[J]
        val[indptr[q]:indptr[q + 1]] = np.where(place[J] >= 0, tc.clip_values(S[q, J], clip), np.nan)
    return Ranks(indptr, indices, rank, val, eligible)


def rank_reference(W, T, rows, targets, exclude, clip=(None, None)):
    S = tc.scores(W, T, rows)
    return ranks_from_scores(S, targets, tc.exclusion_mask(exclude, S.shape[0], S.shape[1]), clip)


METRICS = ('hit_rate', 'precision', 'recall', 'ndcg', 'mrr', 'auc', 'mean_percentile_rank')


def metrics_reference(users, rank, eligible, n_items):
    """the metrics of NMF_RS_Estimator.ranking_score from one (user, rank, eligible count of the user) triple per DISTINCT
    target pair: plain loops over users, nothing vectorised"""
    per_user = {}
    not_eligible = 0
    for u, r, L in zip(users, rank, eligible):
        if r < 0:
            not_eligible += 1
        else:
            per_user.setdefault(int(u), (int(L), []))[1].append(int(r))
    sums = dict.fromkeys(METRICS, 0.0)
    n_auc = n_mpr = 0
    for u, (L, rs) in per_user.items():
        rs.sort()
        P = len(rs)
        top = [r for r in rs if r < n_items]
        sums['hit_rate'] += 1.0 if top else 0.0
        sums['precision'] += len(top) / float(n_items)
        sums['recall'] += len(top) / float(P)
        sums['ndcg'] += sum(1.0 / math.log2(r + 2) for r in top) / sum(1.0 / math.log2(p + 2) for p in range(min(n_items, P)))
        sums['mrr'] += 1.0 / (1 + rs[0])
        if L > P:
            sums['auc'] += 1.0 - sum(r - a for a, r in enumerate(rs)) / float(P * (L - P))
            n_auc += 1
        if L > 1:
            for r in rs:
                sums['mean_percentile_rank'] += r / float(L - 1)
                n_mpr += 1
    nu = len(per_user)
    out = {'n_items': n_items, 'users': nu, 'targets': len(rank), 'targets_not_eligible': not_eligible}
    for name in METRICS:
        cnt = n_auc if name == 'auc' else n_mpr if name == 'mean_percentile_rank' else nu
        out[name] = sums[name] / cnt if cnt else float('nan')
    return out


# ---- exact cases: every geometry of topn_cases.EXACT_CASES with every kind of target list (one handle per geometry) ---------------
KINDS = ('none', 'one', 'edge', 'all', 'excluded')


def make_targets(kind, case, excl, seed=0):
    """a scipy CSR pattern (count, d) of the kind, column indices DESCENDING inside every row (the caller's arrays need not be
    sorted).  none: random lists, some requests without a target (request 0 always); one: one target per request; edge: 64 and 65
    targets in the first two requests where d allows, else every column, random lists elsewhere; all: every column of every
    request; excluded: the request's excluded columns (and one more where there is room), random ones without an exclusion."""
    rng = np.random.RandomState(3000 + seed)
    m, d = case.count, case.d
    mask = np.zeros((m, d), dtype=bool)
    if kind == 'none':
        mask = rng.rand(m, d) < 0.2
        mask[rng.rand(m) < 0.4] = False
        mask[0] = False
    elif kind == 'one':
        mask[np.arange(m), rng.randint(0, d, size=m)] = True
    elif kind == 'edge':
        mask = rng.rand(m, d) < 0.1
        for q, cnt in ((0, 64), (1 % m, 65)):
            mask[q] = False
            mask[q, rng.permutation(d)[:min(cnt, d)]] = True
    elif kind == 'all':
        mask[:] = True
    elif kind == 'excluded':
        mask = tc.exclusion_mask(excl, m, d) if excl is not None else rng.rand(m, d) < 0.3
        mask = mask.copy()
        mask[np.arange(m), rng.randint(0, d, size=m)] = True
    A = sp.csr_matrix(mask.astype(np.float64))
    A.sort_indices()
    for i in range(m):
        A.indices[A.indptr[i]:A.indptr[i + 1]] = A.indices[A.indptr[i]:A.indptr[i + 1]][::-1].copy()
    A.has_sorted_indices = False
    return A


# ---- real-valued factors --------------------------------------------------------------------------------------------------------
def rank_bands(W, T, rows, targets, exclude):
    """For real-valued factors: (Ranks of the restatement, lo, hi, tol per target) with R the restatement's scores and
    tol_i = 2 k 2^-52 max_j (|W[i]| |T|)_j, topn_cases.check_real's tolerance:
      lo = #{eligible j' != j : R_j' > R_j + 2 tol},  hi = #{eligible j' != j : R_j' >= R_j - 2 tol}
    A rank counted from scores that lie within tol of R lies in [lo, hi].  Targets that are not eligible get lo = hi = -1."""
    W = np.asarray(W, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    Wr = W if rows is None else W[np.asarray(rows)]
    R = Wr @ T
    m, d = R.shape
    tol_row = 2.0 * W.shape[1] * 2.0 ** -52 * (np.abs(Wr) @ np.abs(T)).max(axis=1)
    excluded = tc.exclusion_mask(exclude, m, d)
    ref = ranks_from_scores(R, targets, excluded)
    lo = np.full(ref.indices.size, -1, dtype=np.int64)
    hi = np.full(ref.indices.size, -1, dtype=np.int64)
    tol = np.repeat(tol_row, np.diff(ref.indptr))
    for q in range(m):
        el = ~excluded[q] & ~np.isnan(R[q])
        for p in range(ref.indptr[q], ref.indptr[q + 1]):
            j = ref.indices[p]
            if not el[j]:
                continue
            others = el.copy()
            others[j] = False
            lo[p] = np.count_nonzero(R[q, others] > R[q, j] + 2 * tol_row[q])
            hi[p] = np.count_nonzero(R[q, others] >= R[q, j] - 2 * tol_row[q])
    return ref, lo, hi, tol
