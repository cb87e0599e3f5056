"""Top-N recommendations at the recommender shape: the device route (rri_topn_rows behind NMF_RS_Estimator.recommend) against
the host route it replaces, in one process on one box.

    python tools/topn_probe.py [--n 100000 --d 10000 --k 20 --top 10 --seen 0.05 --out FILE]

Uniform random factors, a random `seen` pattern of the given density, all users.  JSON lines:
  kernel      k_topn_rows by HIP events (rri_timing_read id 4), three calls after a warm-up, with the MFMA-only lower bound
              2 n d k flops at 78.6 TFLOP/s (float64 matrix rate) beside it; once without and once with the exclusion
  call        wall time of RRIEngine.topn_rows for all users on a handle that already holds the factors (sort check of the
              pattern, the copies in and out, the kernel)
  recommend   wall time of NMF_RS_Estimator.recommend(): handle, factors up, the rows of seen_, the call(s), handle closed
  host        chunked np.dot, mask, argpartition, sort -- chunks of 1000 users dealt to 16 threads
  small       recommend() for 64 users, device and host
  agreement   the two routes on a sample of users: the same items, or scores within the rounding of two differently ordered sums
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


def random_pattern(n, d, density, seed):
    rng = np.random.RandomState(seed)
    per_row = max(1, int(round(density * d)))
    indices = np.empty((n, per_row), dtype=np.int32)
    for lo in range(0, n, 4096):            # per_row distinct columns per row: the smallest keys of a random matrix
        hi = min(n, lo + 4096)
        indices[lo:hi] = np.sort(np.argpartition(rng.rand(hi - lo, d), per_row, axis=1)[:, :per_row], axis=1)
    indptr = np.arange(n + 1, dtype=np.int64) * per_row
    return sp.csr_matrix((np.ones(n * per_row, dtype=np.int8), indices.reshape(-1), indptr), shape=(n, d))


def host_route(W, T, seen, users, top, lo, hi, threads=16, chunk=1000):
    items = np.empty((len(users), top), dtype=np.int32)
    scores = np.empty((len(users), top))

    def work(c0):
        u = users[c0:c0 + chunk]
        S = W[u] @ T
        if seen is not None:
            E = seen[u]
            S[np.repeat(np.arange(len(u)), np.diff(E.indptr)), E.indices] = -np.inf
        part = np.argpartition(-S, top - 1, axis=1)[:, :top]
        pv = np.take_along_axis(S, part, axis=1)
        order = np.lexsort((part, -pv), axis=1)
        items[c0:c0 + len(u)] = np.take_along_axis(part, order, axis=1)
        scores[c0:c0 + len(u)] = np.clip(np.take_along_axis(pv, order, axis=1), lo, hi)
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(work, range(0, len(users), chunk)))
    return items, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--top', type=int, default=10)
    ap.add_argument('--seen', type=float, default=0.05)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from rri_nmf_amd.engine import RRIEngine
    from rri_nmf_amd import sklearn_interface as si
    n, d, k, top = a.n, a.d, a.k, a.top
    rng = np.random.RandomState(0)
    W, T = rng.rand(n, k), rng.rand(k, d)
    lo, hi = 1.0, 0.3 * k
    t0 = time.perf_counter()
    seen = random_pattern(n, d, a.seen, 1)
    lines = [dict(what='problem', n=n, d=d, k=k, top=top, seen_density=a.seen, seen_entries=int(seen.nnz),
                  pattern_seconds=round(time.perf_counter() - t0, 3))]
    bound_ms = 2.0 * n * d * k / F64_MATRIX_FLOPS * 1e3

    e = RRIEngine(n, d, k, dtype=np.float64)
    e.set_W(W), e.set_T(T)
    e.topn_rows(np.arange(64), top)                                     # warm-up: the code object, the first launch
    for label, ex in (('no exclusion', None), ('exclusion', seen)):
        e.timing_enable(True)
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            res = e.topn_rows(None, top, exclude=ex, clip=(lo, hi))
            walls.append(time.perf_counter() - t0)
        launches, ms = e.timing_read(4)
        e.timing_enable(False)
        lines.append(dict(what='kernel', exclusion=label, launches=launches, kernel_ms=round(ms / launches, 3),
                          mfma_only_bound_ms=round(bound_ms, 3), tflops=round(2.0 * n * d * k / (ms / launches * 1e-3) / 1e12, 2)))
        lines.append(dict(what='call', exclusion=label, wall_ms=[round(1e3 * w, 1) for w in walls]))
    dev_items, dev_scores = res
    e.close()

    E = si.NMF_RS_Estimator(n, d, k, W=W, T=T)
    E.min_rating, E.max_rating, E.seen_ = lo, hi, seen
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        items, scores = E.recommend(n_items=top)
        walls.append(time.perf_counter() - t0)
    lines.append(dict(what='recommend', users=n, wall_ms=[round(1e3 * w, 1) for w in walls]))
    assert np.array_equal(items, dev_items)

    users = np.arange(n)
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        h_items, h_scores = host_route(W, T, seen, users, top, lo, hi)
        walls.append(time.perf_counter() - t0)
    lines.append(dict(what='host', users=n, threads=16, wall_ms=[round(1e3 * w, 1) for w in walls]))

    few = np.arange(0, n, max(1, n // 64))[:64]
    wd, wh = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        E.recommend(few, n_items=top)
        wd.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        host_route(W, T, seen, few, top, lo, hi)
        wh.append(time.perf_counter() - t0)
    lines.append(dict(what='small', users=64, device_wall_ms=[round(1e3 * w, 2) for w in wd], host_wall_ms=[round(1e3 * w, 2) for w in wh]))

    same = (h_items == items).all(axis=1)
    tol = 2.0 * k * 2.0 ** -52 * (np.abs(W) @ np.abs(T).max(axis=1))
    close = np.abs(h_scores - scores).max(axis=1) <= tol
    lines.append(dict(what='agreement', rows=n, same_items=int(same.sum()), scores_within_rounding=int(close.sum())))
    assert close.all()
    text = '\n'.join(json.dumps(ln) for ln in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
