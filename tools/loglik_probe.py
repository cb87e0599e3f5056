"""The log-likelihood of a corpus's stored counts under W T at the topic-model shape: the device route (rri_entries_loglik behind
RRIEngine.entries_loglik) against the chunked einsum restatement on the host, in one process on one box.

    python tools/loglik_probe.py [--n 100000 --d 10000 --k 50 --out FILE] [--borders-only --forced-lanes N]

Zipf term counts (tools/sparse_x_probe.zipf_counts) at the two densities the README quotes for a CSR X (asked 0.2 % and 5 %: about
1.6 M and 23.5 M stored entries); factors on the simplex, so every row of W T is a distribution.  JSON lines.

what = 'loglik', one per density:
  kernel_ms   the launches of one call by HIP events (rri_timing_read id 7): the transposed copy of T and, per chunk of requests,
              k_loglik_entries and k_loglik_sum; the mean of three calls after a warm-up, and launches_per_call
  wall_ms     RRIEngine.entries_loglik, three calls: the request check, the upload in chunks, the launches, the outputs back
  host_ms     the restatement: per chunk of 2^20 entries gather W[i, :] and T[:, j], einsum, log, and a bincount per request; the
              chunks dealt to 16 threads
  within_bound  whether every request's ll lies within tests/loglik_cases.py's bound of the host's, mass is equal and no entry is
              floored on either side; max_err_over_bound is the largest ratio
what = 'lanes', the border of loglik_lanes: the 1.6 M-entry corpus at the topic counts of --ks with the lane count the library
takes, kernel_ms of two runs of three calls.  The other lane counts come from measurement builds of the library, which take one
lane count for every k (forced: true in their lines):
    hipcc ... -DRRI_LOGLIK_LANES=4 (or 16, 64) ... -o librri_hip_l4.so
    RRI_HIP_LIB=librri_hip_l4.so python tools/loglik_probe.py --borders-only --forced-lanes 4 --out FILE
(--forced-lanes only labels the lines; a process loads one library).
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_x_probe import zipf_counts  # noqa: E402

U = 2.0 ** -52


def lanes(k):
    return 4 if k <= 128 else 16


def simplex_factors(n, d, k, seed):
    rng = np.random.RandomState(seed)
    W, T = rng.rand(n, k), rng.rand(k, d)
    return W / W.sum(axis=1, keepdims=True), T / T.sum(axis=1, keepdims=True)


def host_route(W, T, A, floor, threads=16, chunk=1 << 20):
    """(ll, mass, floored, sum of |term| per request) by the chunked einsum"""
    n = A.shape[0]
    req = np.repeat(np.arange(n), np.diff(A.indptr))
    Tt = np.ascontiguousarray(T.T)
    v = A.data.astype(np.float64)
    term, low = np.empty(A.nnz), np.empty(A.nnz, dtype=bool)

    def work(lo):
        s = slice(lo, min(lo + chunk, A.nnz))
        p = np.einsum('et,et->e', W[req[s]], Tt[A.indices[s]])
        low[s] = (v[s] > 0) & (p < floor)
        term[s] = np.where(v[s] == 0, 0.0, v[s] * np.log(np.where(p < floor, floor, p)))
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(work, range(0, A.nnz, chunk)))
    return (np.bincount(req, weights=term, minlength=n), np.bincount(req, weights=v, minlength=n),
            np.bincount(req, weights=low, minlength=n).astype(np.int64), np.bincount(req, weights=np.abs(term), minlength=n))


def device_times(e, A, floor, calls=3):
    e.timing_enable(True)
    e.timing_read(7)
    walls, got = [], None
    for _ in range(calls):
        t0 = time.perf_counter()
        got = e.entries_loglik(None, A, floor)
        walls.append(time.perf_counter() - t0)
    launches, ms = e.timing_read(7)
    e.timing_enable(False)
    return got, walls, launches // calls, ms / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--out', default=None)
    ap.add_argument('--borders-only', action='store_true')
    ap.add_argument('--forced-lanes', type=int, default=0)
    ap.add_argument('--ks', default='16,17,50,128,129,256,512,1024', help='topic counts of the lanes lines')
    a = ap.parse_args()
    from rri_nmf_amd.engine import RRIEngine
    n, d, k, floor = a.n, a.d, a.k, 1e-12
    lines = []
    corpora = {}
    for density in (0.002,) if a.borders_only else (0.002, 0.05):
        A = zipf_counts(n, d, density)
        A.sort_indices()
        A = A.astype(np.float64)                                   # the dtypes the library reads: no copy inside the call
        A.indptr = A.indptr.astype(np.int64)
        corpora[density] = A
    W, T = simplex_factors(n, d, k, seed=0)
    with RRIEngine(n, d, k, dtype=np.float64) as e:
        e.set_W(W), e.set_T(T)
        e.entries_loglik(None, corpora[0.002], floor)              # warm-up: the code objects, the first launches
        for density, A in ({} if a.borders_only else corpora).items():
            got, walls, launches, kernel_ms = device_times(e, A, floor)
            hosts = []
            for _ in range(2 if A.nnz < 5e6 else 1):
                t0 = time.perf_counter()
                ll, mass, floored, absl = host_route(W, T, A, floor)
                hosts.append(time.perf_counter() - t0)
            bound = U * (2 * (k + 2) * mass + (np.diff(A.indptr) + 4) * absl)
            ratio = float(np.max(np.abs(got[0] - ll) / np.maximum(bound, 1e-300)))
            ok = bool(ratio <= 1.0 and np.array_equal(got[1], mass) and not got[2].any() and not floored.any())
            lines.append(dict(what='loglik', n=n, d=d, k=k, lanes=lanes(k), nnz=int(A.nnz), launches_per_call=launches,
                              kernel_ms=round(kernel_ms, 3), wall_ms=[round(1e3 * w, 1) for w in walls],
                              host_ms=[round(1e3 * w, 1) for w in hosts], host_threads=16, within_bound=ok,
                              max_err_over_bound=round(ratio, 4), perplexity=round(float(np.exp(-got[0].sum() / got[1].sum())), 3)))
            print(json.dumps(lines[-1]), flush=True)
            assert ok
    # the borders of loglik_lanes
    A = corpora[0.002]
    for kk in (int(x) for x in a.ks.split(',')):
        Wk, Tk = simplex_factors(n, d, kk, seed=kk)
        with RRIEngine(n, d, kk, dtype=np.float64) as e:
            e.set_W(Wk), e.set_T(Tk)
            e.entries_loglik(None, A, floor)
            runs = [device_times(e, A, floor) for _ in range(2)]
            lines.append(dict(what='lanes', n=n, d=d, k=kk, lanes=a.forced_lanes or lanes(kk), forced=bool(a.forced_lanes),
                              nnz=int(A.nnz), kernel_ms=[round(r[3], 3) for r in runs],
                              wall_ms=[round(1e3 * w, 1) for r in runs for w in r[1]], ll_sum=float(runs[0][0][0].sum())))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(json.dumps(ln) for ln in lines) + '\n')


if __name__ == '__main__':
    main()
