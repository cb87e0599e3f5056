"""The fit from a DeviceCorpus at the topic-model shape: what a ready CSR handle costs by each route, and what a whole fit costs
from a corpus, from the scipy matrix and from GPU tensors, in one process on one box.

    python tools/corpus_fit_probe.py --step handle|fit --density 0.002|0.05 [--routes csr,corpus] [--tree DIR]
                                     [--n 100000 --d 10000 --k 50 --runs 5 --sweeps 30 --out FILE --tag TEXT]

Zipf term counts (tools/sparse_x_probe.zipf_counts) at the two densities of profiles/r23_corpus_probe.jsonl (asked 0.2 % and 5 %:
about 1.6 M and 23.5 M stored entries).  One step per process.  After a warm-up of every route the routes alternate, --runs
times; every figure is the median with the smallest and the largest beside it.  JSON lines.

--tree DIR imports rri_nmf_amd from another checkout (its library built): `--routes csr --tree <parent commit>` is the host route
of the parent commit, to be alternated with this commit's by the job that calls the probe.

--step handle -- the time from nothing to a handle that can sweep: RRIEngine(sparse_x=True) and
  csr_ms         upload_X_csr(A) of the canonical scipy matrix: the host's checks, three uploads, build_sp_copy twice on the host
  corpus_ms      upload_X_corpus(corpus) of a corpus made before: copies on the device, the store built there
  build_kernel_ms  the HIP-event time of the device build's kernels (rri_sparse_store_get, field 9)
  equal          whether both stores hold the same perm and idx arrays in both copies
--step fit -- NMF_TM_Estimator(handle_tfidf, handle_normalization, keep_resident, nmf_kwargs sparse_X, uniform_rows).fit, --sweeps
sweeps from one given start, the estimator released after every run:
  corpus_ms      fit(corpus), the corpus made before
  scipy_ms       fit(A)
  tensors_ms     DeviceCorpus.from_device(three torch GPU tensors) and fit(corpus): counts that are on the card already
  tensors_via_host_ms   the same tensors by the route this commit replaces: from_device, to_scipy(), fit(scipy matrix)
  equal          whether all four leave the same W and T
"""
import argparse
import ctypes
import json
import logging
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))


def stats(ms):
    return dict(median=round(float(np.median(ms)), 2), min=round(min(ms), 2), max=round(max(ms), 2), runs=[round(x, 2) for x in ms])


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return out, 1e3 * (time.perf_counter() - t0)


def counts(a):
    sys.path.insert(0, HERE)
    from sparse_x_probe import zipf_counts
    A = zipf_counts(a.n, a.d, a.density)
    A.sort_indices()
    return sp.csr_matrix((A.data.astype(np.float64), A.indices, A.indptr), shape=A.shape)


def step_handle(a, emit):
    from rri_nmf_amd import engine as E
    A = counts(a)
    routes = a.routes.split(',')
    corpus = E.DeviceCorpus(A) if 'corpus' in routes else None

    def ready(route, keep=False):
        def make():
            eng = E.RRIEngine(a.n, a.d, a.k, dtype=np.float64, sparse_x=True)
            if route == 'csr':
                eng.upload_X_csr(A)
            else:
                eng.upload_X_corpus(corpus)
            eng.synchronize()
            return eng
        eng, ms = clock(make)
        us = 0
        if route == 'corpus':
            info = (ctypes.c_int64 * 10)()
            eng._check(eng._lib.rri_sparse_store_get(eng._h, 0, info, 10, None, None, None, None, None))
            us = int(info[9])
        if keep:
            return eng, ms, us
        eng.close()
        return None, ms, us
    for r in routes:                    # warm-up: code objects, first launches, the allocator
        ready(r)
    ms = {r: [] for r in routes}
    kernel = []
    for _ in range(a.runs):
        for r in routes:
            _, t, us = ready(r)
            ms[r].append(t)
            if r == 'corpus':
                kernel.append(us / 1e3)
    line = dict(what='handle', tag=a.tag, n=a.n, d=a.d, k=a.k, stored=int(A.nnz))
    for r in routes:
        line[r + '_ms'] = stats(ms[r])
    if kernel:
        line['build_kernel_ms'] = stats(kernel)
    if len(routes) == 2:
        ea, eb = ready('csr', True)[0], ready('corpus', True)[0]
        line['equal'] = bool(all(np.array_equal(ea.sparse_store(w)[f], eb.sparse_store(w)[f]) for w in (0, 1) for f in ('segptr', 'perm', 'idx', 'work')))
        ea.close()
        eb.close()
    emit(line)
    if corpus is not None:
        corpus.close()


def step_fit(a, emit):
    import torch
    from rri_nmf_amd import nmf as nm, sklearn_interface as si
    from rri_nmf_amd.engine import DeviceCorpus
    nm.logger.setLevel(logging.WARNING)             # no objective between the sweeps: exactly --sweeps sweeps
    A = counts(a)
    rng = np.random.RandomState(2)
    W0, T0 = rng.rand(a.n, a.k), rng.rand(a.k, a.d)
    corpus = DeviceCorpus(A)
    tensors = [torch.as_tensor(x).cuda() for x in (A.indptr, A.indices, A.data)]
    torch.cuda.synchronize()

    def fit(X):
        est = si.NMF_TM_Estimator(a.n, a.d, a.k, handle_tfidf=True, handle_normalization=True, keep_resident=True, max_iter=a.sweeps,
                                  W=W0, T=T0, nmf_kwargs=dict(sparse_X=True, uniform_rows=True))
        est.fit(X)
        est.release()
        return est.W, est.T

    def from_tensors(via_host):
        with DeviceCorpus.from_device(tensors[0], tensors[1], tensors[2], A.shape) as c:
            return fit(c.to_scipy() if via_host else c)
    routes = dict(corpus=lambda: fit(corpus), scipy=lambda: fit(A), tensors=lambda: from_tensors(False),
                  tensors_via_host=lambda: from_tensors(True))
    out = {r: f() for r, f in routes.items()}           # warm-up, and the results to compare
    ms = {r: [] for r in routes}
    for _ in range(a.runs):
        for r, f in routes.items():
            ms[r].append(clock(f)[1])
    line = dict(what='fit', tag=a.tag, n=a.n, d=a.d, k=a.k, sweeps=a.sweeps, stored=int(A.nnz))
    for r in routes:
        line[r + '_ms'] = stats(ms[r])
    line['equal'] = bool(all(np.array_equal(out[r][0], out['scipy'][0]) and np.array_equal(out[r][1], out['scipy'][1]) for r in routes))
    emit(line)
    corpus.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', required=True, choices=['handle', 'fit'])
    ap.add_argument('--density', type=float, default=0.002)
    ap.add_argument('--routes', default='csr,corpus')
    ap.add_argument('--tree', default=os.path.dirname(HERE))
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--sweeps', type=int, default=30)
    ap.add_argument('--tag', default='')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(line) + '\n')
    (step_handle if a.step == 'handle' else step_fit)(a, emit)


if __name__ == '__main__':
    main()
