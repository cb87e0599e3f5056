"""Corpora derived on the device at the topic-model shape: what a row subset, a pruned vocabulary, the document frequencies and a
split of the counts cost from a resident corpus, against the host route for the same result, in one process on one box.

    python tools/derive_probe.py --density 0.002|0.05 [--n 100000 --d 10000 --reps 5 --out FILE]

Zipf term counts (tools/sparse_x_probe.zipf_counts) at the two densities the README quotes for a CSR X (asked 0.2 % and 5 %: about
1.6 M and 23.5 M stored entries).  One density per process, so that a job runs each under a time limit of its own.  The routes
alternate inside the process (device, host, device, host ...), `reps` times each; every list holds all the times and `*_median`
their median.  JSON lines, one per operation:
  take_rows         a random half of the rows, in random order
  select_words      the words prune_words(min_df=5, max_df=0.5) keeps (the decision itself is timed under prune_words)
  prune_words       document_frequency, the host's decision over df, select_words
  document_frequency
  split_counts      held_out = 0.5
with
  device_ms         the DeviceCorpus call, from a resident corpus to a resident result
  kernel_ms         the HIP-event time of its kernels (ingest_ms of the result; for a split of either result; none for
                    document_frequency, whose call is the kernel, the d-sized download and a handle)
  host_ms           the host route on the scipy matrix: A[rows], A[:, keep], (A != 0).sum(0), sklearn_interface.split_counts
  host_reingest_ms  the host route and DeviceCorpus(result), which is what it takes to have the result resident again
  equal             whether the device's result equals the host's (for a split: observed + held == A on both routes, and the
                    held shares; the two generators differ, so the parts do not)
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
from sparse_x_probe import zipf_counts  # noqa: E402


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return out, round(1e3 * (time.perf_counter() - t0), 3)


def same(A, B):
    return bool(A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data))


def close(out):
    for c in out if isinstance(out, tuple) else (out,):
        if hasattr(c, 'close'):
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--density', type=float, default=0.002)
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from rri_nmf_amd import sklearn_interface as si
    from rri_nmf_amd.engine import DeviceCorpus, corpus_memory

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(line) + '\n')

    A = zipf_counts(a.n, a.d, a.density)
    A.sort_indices()
    A = sp.csr_matrix((A.data.astype(np.float64), A.indices, A.indptr), shape=A.shape)
    rng = np.random.RandomState(0)
    rows = rng.permutation(a.n)[:a.n // 2].astype(np.int64)
    small = DeviceCorpus(A[:2000])                                  # warm-up: the code objects, the first launches
    close(small.take_rows([1, 0]))
    close(small.select_words([0, 1]))
    close(small.split_counts(0.5, 0))
    small.document_frequency()
    small.close()
    corpus = DeviceCorpus(A)
    df = corpus.document_frequency()
    kept = DeviceCorpus._prune_selection(df, a.n, 5, 0.5)

    def canonical(M):
        M = sp.csr_matrix(M)
        M.sort_indices()
        return M

    def host_prune():
        host_df = np.asarray((A != 0).sum(0)).ravel()
        return canonical(A[:, DeviceCorpus._prune_selection(host_df, a.n, 5, 0.5)])
    ops = (('take_rows', lambda: corpus.take_rows(rows), lambda: canonical(A[rows])),
           ('select_words', lambda: corpus.select_words(kept), lambda: canonical(A[:, kept])),
           ('prune_words', lambda: corpus.prune_words(5, 0.5)[0], host_prune),
           ('document_frequency', corpus.document_frequency, lambda: np.asarray((A != 0).sum(0)).ravel()),
           ('split_counts', lambda: corpus.split_counts(0.5, 12345), lambda: si.split_counts(A, 0.5, 12345)))
    for name, device, host in ops:
        line = dict(what=name, n=a.n, d=a.d, stored=int(A.nnz), device_ms=[], kernel_ms=[], host_ms=[], host_reingest_ms=[])
        equal = True
        for _ in range(a.reps):
            got, ms = clock(device)
            line['device_ms'].append(ms)
            want, ms = clock(host)
            line['host_ms'].append(ms)
            if name != 'document_frequency':
                line['kernel_ms'].append(round((got[0] if isinstance(got, tuple) else got).ingest_ms, 3))

                def again():
                    out = host()
                    return tuple(DeviceCorpus(m) for m in out) if isinstance(out, tuple) else DeviceCorpus(out)
                made, ms = clock(again)
                line['host_reingest_ms'].append(ms)
                close(made)
            if name == 'document_frequency':
                equal = equal and bool(np.array_equal(got, want))
            elif name == 'split_counts':
                o, h = (c.to_scipy() for c in got)
                total = canonical(o + h)
                line['held_share'] = [round(float(h.data.sum() / A.data.sum()), 5), round(float(want[1].data.sum() / A.data.sum()), 5)]
                equal = equal and same(total, A) and same(canonical(want[0] + want[1]), A)
            else:
                equal = equal and same(got.to_scipy(), want)
                line['result'] = [int(got.shape[0]), int(got.shape[1]), int(got.nnz)]
            close(got)
        for key in ('device_ms', 'kernel_ms', 'host_ms', 'host_reingest_ms'):
            if line[key]:
                line[key + '_median'] = float(np.median(line[key]))
        line['equal'] = equal
        emit(line)
    corpus.close()
    assert corpus_memory() == (0, 0)


if __name__ == '__main__':
    main()
