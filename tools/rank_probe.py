"""Ranks of held-out pairs at the recommender shape: the device route (rri_rank_entries behind NMF_RS_Estimator.rank and
ranking_score) against k_topn_rows, which walks the same tiles, and against a host route, in one process on one box.

    python tools/rank_probe.py [--n 100000 --d 10000 --k 20 --seen 500 --held 25 --out FILE]

Uniform random factors; per user `seen` excluded items and `held` held-out targets outside them; all users.  JSON lines:
  kernel      k_rank_entries by HIP events (rri_timing_read id 5): the mean of three calls after a warm-up, without and with the
              exclusion, the MFMA-only lower bound of its TWO walks (2 * 2 n d k flops at 78.6 TFLOP/s) beside it
  yardstick   k_topn_rows (N = 10, id 4) on the same handle, the same way
  call        wall time of RRIEngine.rank_entries for all users on a handle that already holds the factors
  score       wall time of NMF_RS_Estimator.ranking_score(): pairs to patterns, handle, factors up, the call, metrics
  host        chunked np.dot, mask and one compare-count per target -- chunks of 1000 users dealt to 16 threads
  small       ranking_score() of 64 users' pairs, device and host
  agreement   the two routes on every target: the same rank, or scores within the rounding of two differently ordered sums
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F64_MATRIX_FLOPS = 78.6e12


def random_patterns(n, d, seen, held, seed):
    """two disjoint CSR patterns with `seen` and `held` distinct columns per row"""
    rng = np.random.RandomState(seed)
    per_row = seen + held
    a = np.empty((n, seen), dtype=np.int32)
    b = np.empty((n, held), dtype=np.int32)
    for lo in range(0, n, 4096):            # per_row distinct columns per row: the smallest keys of a random matrix
        hi = min(n, lo + 4096)
        pick = np.argpartition(rng.rand(hi - lo, d), per_row, axis=1)[:, :per_row]
        a[lo:hi] = np.sort(pick[:, :seen], axis=1)
        b[lo:hi] = np.sort(pick[:, seen:], axis=1)

    def csr(ind):
        return sp.csr_matrix((np.ones(ind.size, dtype=np.int8), ind.reshape(-1), np.arange(n + 1, dtype=np.int64) * ind.shape[1]),
                             shape=(n, d))
    return csr(a), csr(b)


def host_route(W, T, seen, targets, users, threads=16, chunk=1000):
    """(rank, score) per target of `users`, in the order of targets[users]"""
    ptr = np.concatenate(([0], np.cumsum(np.diff(targets.indptr)[users])))
    rank = np.empty(ptr[-1], dtype=np.int32)
    score = np.empty(ptr[-1])

    def work(c0):
        u = users[c0:c0 + chunk]
        S = W[u] @ T
        if seen is not None:
            E = seen[u]
            S[np.repeat(np.arange(len(u)), np.diff(E.indptr)), E.indices] = -np.inf
        G = targets[u]
        cols_all = np.arange(S.shape[1])
        for r in range(len(u)):                          # one compare-count per target; ties by the smaller column
            cols = G.indices[G.indptr[r]:G.indptr[r + 1]]
            s = S[r, cols]
            before = (S[r][None, :] > s[:, None]) | ((S[r][None, :] == s[:, None]) & (cols_all[None, :] < cols[:, None]))
            out = slice(ptr[c0] + G.indptr[r], ptr[c0] + G.indptr[r + 1])
            rank[out] = before.sum(axis=1)
            score[out] = s
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(work, range(0, len(users), chunk)))
    return rank, score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--seen', type=int, default=500)
    ap.add_argument('--held', type=int, default=25)
    ap.add_argument('--host-users', type=int, default=None, help='users the host route ranks (default: all)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from rri_nmf_amd.engine import RRIEngine
    from rri_nmf_amd import sklearn_interface as si
    n, d, k = a.n, a.d, a.k
    rng = np.random.RandomState(0)
    W, T = rng.rand(n, k), rng.rand(k, d)
    lo, hi = 1.0, 0.3 * k
    t0 = time.perf_counter()
    seen, held = random_patterns(n, d, a.seen, a.held, 1)
    lines = [dict(what='problem', n=n, d=d, k=k, seen_per_user=a.seen, held_per_user=a.held, targets=int(held.nnz),
                  pattern_seconds=round(time.perf_counter() - t0, 3))]
    bound_ms = 2.0 * n * d * k / F64_MATRIX_FLOPS * 1e3

    e = RRIEngine(n, d, k, dtype=np.float64)
    e.set_W(W), e.set_T(T)
    e.rank_entries(np.arange(64), held[:64])                            # warm-up: the code objects, the first launches
    e.topn_rows(np.arange(64), 10)
    for label, ex in (('no exclusion', None), ('exclusion', seen)):
        e.timing_enable(True)
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = e.rank_entries(None, held, exclude=ex, clip=(lo, hi))
            walls.append(time.perf_counter() - t0)
        launches, ms = e.timing_read(5)
        for _ in range(3):
            e.topn_rows(None, 10, exclude=ex, clip=(lo, hi))
        tl, tms = e.timing_read(4)
        e.timing_enable(False)
        lines.append(dict(what='kernel', exclusion=label, launches=launches, kernel_ms=round(ms / launches, 3),
                          mfma_only_bound_ms_two_walks=round(2 * bound_ms, 3)))
        lines.append(dict(what='yardstick', kernel='k_topn_rows N=10', exclusion=label, launches=tl, kernel_ms=round(tms / tl, 3),
                          mfma_only_bound_ms=round(bound_ms, 3)))
        lines.append(dict(what='call', exclusion=label, wall_ms=[round(1e3 * w, 1) for w in walls]))
    e.close()

    E = si.NMF_RS_Estimator(n, d, k, W=W, T=T)
    E.min_rating, E.max_rating, E.seen_ = lo, hi, seen
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        score = E.ranking_score(held, n_items=10)
        walls.append(time.perf_counter() - t0)
    lines.append(dict(what='score', users=n, wall_ms=[round(1e3 * w, 1) for w in walls], metrics={m: round(v, 6) for m, v in score.items()}))

    users = np.arange(n if a.host_users is None else min(n, a.host_users))
    t0 = time.perf_counter()
    h_rank, h_score = host_route(W, T, seen, held, users)
    lines.append(dict(what='host', users=int(users.size), threads=16, wall_ms=[round(1e3 * (time.perf_counter() - t0), 1)]))

    few = np.arange(0, n, max(1, n // 64))[:64]
    few_pairs = held[few].tocoo()
    few_pairs = np.column_stack((few[few_pairs.row], few_pairs.col))
    wd, wh = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        E.ranking_score(few_pairs, n_items=10)
        wd.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        host_route(W, T, seen, held, few)
        wh.append(time.perf_counter() - t0)
    lines.append(dict(what='small', users=64, device_wall_ms=[round(1e3 * w, 2) for w in wd], host_wall_ms=[round(1e3 * w, 2) for w in wh]))

    m = int(held.indptr[users.size])
    same = h_rank == res.rank[:m]
    tol = np.repeat(2.0 * k * 2.0 ** -52 * (np.abs(W[users]) @ np.abs(T).max(axis=1)), np.diff(held.indptr)[users])
    close = np.abs(np.clip(h_score, lo, hi) - res.val[:m]) <= tol
    lines.append(dict(what='agreement', targets=m, same_rank=int(same.sum()), scores_within_rounding=int(close.sum()),
                      eligible_all=bool(np.all(res.eligible == d - a.seen))))
    assert close.all()
    text = '\n'.join(json.dumps(ln) for ln in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
