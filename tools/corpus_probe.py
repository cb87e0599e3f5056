"""A CSR corpus on the device at the topic-model shape: what the ingest costs, and what a repeated evaluation call saves, in one
process on one box.

    python tools/corpus_probe.py --step ingest|calls --density 0.002|0.05 [--n 100000 --d 10000 --k 50 --out FILE]

Zipf term counts (tools/sparse_x_probe.zipf_counts) at the two densities the README quotes for a CSR X (asked 0.2 % and 5 %: about
1.6 M and 23.5 M stored entries).  One step per process, so that a job runs each under a time limit of its own.  JSON lines.

--step ingest, one line per kind of matrix -- `canonical` (as scipy made it), `shuffled` (every row in random order) and
`duplicates` (shuffled, and a tenth of the entries stored twice, half the count each time):
  scipy_ms       the host's canonical copy that every call on a scipy matrix makes (copy, sum_duplicates, eliminate_zeros,
                 sort_indices), three times
  cooc_call_ms   one RRIEngine.cooccurrence_counts(A, words) on the scipy matrix, 50 groups of 10 words: canonical copy, upload,
                 kernels -- the host route of the parent commit, three times
  host_ms        DeviceCorpus(A): upload of the raw arrays, check, canonical form, three times; host_kernel_ms its kernels
  device_ms      DeviceCorpus.from_device on the same arrays as torch GPU tensors, three times; device_kernel_ms its kernels
  rows_rewritten, duplicates_merged, zeros_dropped, long_rows, device_bytes, and whether both corpora equal scipy's canonical copy
--step calls, one line per call -- `coherence` (n_words = 10, npmi) and `log_likelihood` (W given, on the simplex):
  scipy_ms       NMF_TM_Estimator.<call>(A, ...) on the scipy matrix, five times
  corpus_ms      the same call on a DeviceCorpus made once (ingest_ms: what making it cost), five times
  equal          whether the two give the same numbers
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cooc_probe import zipf_words  # noqa: E402
from sparse_x_probe import zipf_counts  # noqa: E402


def timed(f, reps):
    out, ms = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ms.append(round(1e3 * (time.perf_counter() - t0), 2))
    return out, ms


def shuffled(A, rng, duplicates=0.0):
    """the rows of the canonical A in random order; duplicates: that share of the entries is stored twice, half the count each"""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    cols, vals = A.indices.astype(np.int64), A.data.astype(np.float64)
    if duplicates:
        twice = np.flatnonzero(rng.rand(A.nnz) < duplicates)
        vals = vals.copy()
        vals[twice] *= 0.5
        rows, cols, vals = np.concatenate([rows, rows[twice]]), np.concatenate([cols, cols[twice]]), np.concatenate([vals, vals[twice]])
    order = np.lexsort((rng.rand(rows.size), rows))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.shape[0]))]).astype(np.int64)
    return sp.csr_matrix((vals[order], cols[order].astype(np.int32), indptr), shape=A.shape)


def same(A, B):
    return bool(np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data))


def step_ingest(a, emit):
    import torch
    from rri_nmf_amd.engine import DeviceCorpus, RRIEngine, corpus_memory
    rng = np.random.RandomState(0)
    base = zipf_counts(a.n, a.d, a.density)
    base.sort_indices()
    base = sp.csr_matrix((base.data.astype(np.float64), base.indices, base.indptr), shape=base.shape)
    words = zipf_words(a.k, 10, a.d, seed=10)
    eng = RRIEngine(4, 4, 2, dtype=np.float64)
    eng.cooccurrence_counts(base[:64], words)                      # warm-up: the code objects, the first launches
    DeviceCorpus(shuffled(base[:2000], rng, 0.1)).close()
    torch.zeros(1, device='cuda')
    for kind in ('canonical', 'shuffled', 'duplicates'):
        A = base if kind == 'canonical' else shuffled(base, rng, 0.1 if kind == 'duplicates' else 0.0)

        def canonical_copy():
            B = sp.csr_matrix(A, copy=True)
            B.sum_duplicates()
            B.eliminate_zeros()
            B.sort_indices()
            return B
        want, scipy_ms = timed(canonical_copy, 3)
        _, call_ms = timed(lambda: eng.cooccurrence_counts(A, words), 3)
        made, host_ms = [], []
        for _ in range(3):
            c, ms = timed(lambda: DeviceCorpus(A), 1)
            made.append(c)
            host_ms += ms
        t = [torch.as_tensor(x).cuda() for x in (A.indptr, A.indices, A.data)]
        torch.cuda.synchronize()
        dev, device_ms = [], []
        for _ in range(3):
            c, ms = timed(lambda: DeviceCorpus.from_device(t[0], t[1], t[2], A.shape), 1)
            dev.append(c)
            device_ms += ms
        c = made[-1]
        emit(dict(what='ingest', kind=kind, n=a.n, d=a.d, stored=int(A.nnz), canonical=c.nnz, scipy_ms=scipy_ms, cooc_call_ms=call_ms,
                  host_ms=host_ms, host_kernel_ms=[round(x.ingest_ms, 3) for x in made], device_ms=device_ms,
                  device_kernel_ms=[round(x.ingest_ms, 3) for x in dev], rows_rewritten=c.rows_rewritten,
                  duplicates_merged=c.duplicates_merged, zeros_dropped=c.zeros_dropped, long_rows=c.long_rows, device_bytes=c.device_bytes,
                  index_dtype=str(A.indices.dtype), equal=same(c.to_scipy(), want) and same(dev[-1].to_scipy(), want)))
        for x in made + dev:
            x.close()
        del t
    eng.close()
    assert corpus_memory() == (0, 0)


def step_calls(a, emit):
    from rri_nmf_amd import sklearn_interface as si
    from rri_nmf_amd.engine import DeviceCorpus
    rng = np.random.RandomState(1)
    A = zipf_counts(a.n, a.d, a.density)
    A.sort_indices()
    A = sp.csr_matrix((A.data.astype(np.float64), A.indices, A.indptr), shape=A.shape)
    W, T = rng.rand(a.n, a.k), rng.rand(a.k, a.d) ** 8          # a few heavy words per topic
    W, T = W / W.sum(axis=1, keepdims=True), T / T.sum(axis=1, keepdims=True)
    E = si.NMF_TM_Estimator(a.n, a.d, a.k, W=W, T=T)
    E.coherence(A[:64])                                            # warm-up
    corpus, made_ms = timed(lambda: DeviceCorpus(A), 1)
    calls = (('coherence', lambda X: E.coherence(X, n_words=10, measure='npmi'), ('df', 'codf', 'per_topic')),
             ('log_likelihood', lambda X: E.log_likelihood(X, W=W), ('per_document', 'tokens', 'floored')))
    for name, call, keys in calls:
        want, scipy_ms = timed(lambda: call(A), 5)
        got, corpus_ms = timed(lambda: call(corpus), 5)
        emit(dict(what='calls', call=name, n=a.n, d=a.d, k=a.k, stored=int(A.nnz), scipy_ms=scipy_ms, corpus_ms=corpus_ms,
                  corpus_made_ms=made_ms, ingest_ms=round(corpus.ingest_ms, 3),
                  equal=bool(all(np.array_equal(got[key], want[key], equal_nan=True) for key in keys))))
    corpus.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--step', required=True, choices=['ingest', 'calls'])
    ap.add_argument('--density', type=float, default=0.002)
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(line) + '\n')
    (step_ingest if a.step == 'ingest' else step_calls)(a, emit)


if __name__ == '__main__':
    main()
