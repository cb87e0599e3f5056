"""A corpus from (row, column, value) pairs and its split by entry at the topic-model shape: what the device routes cost against
the host's coo_matrix(...).tocsr(), in one process on one box.

    python tools/corpus_build_probe.py --density 0.002|0.05 [--n 100000 --d 10000 --reps 5 --out FILE]

Zipf term counts (tools/sparse_x_probe.zipf_counts) at the two densities the README quotes for a CSR X (asked 0.2 % and 5 %: about
1.6 M and 23.5 M stored entries), taken apart into (row, column, value) triples, one per stored entry.  One density per process,
so that a job runs each under a time limit of its own.  The routes alternate inside the process, `reps` times each; every list
holds all the times and `*_median` their median.  JSON lines:
  from_pairs, order = by_row | shuffled     the triples sorted by row (columns ascending), and in random order
    host_pairs_ms     DeviceCorpus.from_pairs(rows, values, cols=cols) from host arrays: upload, check, count, claim, sorts
    device_pairs_ms   the same from torch GPU tensors (absent without torch)
    kernel_ms         the HIP-event time of the kernels of either (ingest_ms)
    scipy_ms          coo_matrix((values, (rows, cols))).tocsr() with sum_duplicates() on the host, alone
    scipy_ingest_ms   that followed by DeviceCorpus(csr): what it takes today to have the corpus resident
    equal             whether all routes hold the same matrix
  split_entries       held_out = 0.05
    device_ms         corpus.split_entries(0.05, seed), from a resident corpus to two resident corpora
    kernel_ms         the HIP-event time of its kernels
    host_ms           sklearn_interface.split_entries on the scipy matrix (a mask of uniform draws)
    host_reingest_ms  that and DeviceCorpus of both parts
    equal             observed + held == A on both routes; held_share of either (the generators differ, so the parts do)
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
    try:
        import torch
        torch.cuda.init()
    except Exception:  # noqa: BLE001  (the torch routes are left out)
        torch = None

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(line) + '\n')

    A = zipf_counts(a.n, a.d, a.density)
    A.sort_indices()
    A = sp.csr_matrix((A.data.astype(np.float64), A.indices, A.indptr), shape=A.shape)
    shape = A.shape
    rows0 = np.repeat(np.arange(a.n, dtype=np.int32), np.diff(A.indptr))
    cols0, vals0 = A.indices.astype(np.int32), A.data.copy()
    small = DeviceCorpus.from_pairs(rows0[:5000], vals0[:5000], shape=shape, cols=cols0[:5000])        # warm-up: the code objects, the first launches
    close(small.split_entries(0.05, 0))
    small.close()
    close(DeviceCorpus(A[:2000]))
    perm = np.random.RandomState(0).permutation(rows0.size)
    for order, (rows, cols, vals) in (('by_row', (rows0, cols0, vals0)), ('shuffled', (rows0[perm], cols0[perm], vals0[perm]))):
        line = dict(what='from_pairs', order=order, n=a.n, d=a.d, pairs=int(rows.size), host_pairs_ms=[], host_pairs_kernel_ms=[], device_pairs_ms=[],
                    device_pairs_kernel_ms=[], scipy_ms=[], scipy_ingest_ms=[])
        if torch is not None:
            tr, tc, tv = (torch.as_tensor(x, device='cuda') for x in (rows, cols, vals))
            torch.cuda.synchronize()
        equal = True

        def by_scipy():
            M = sp.coo_matrix((vals, (rows, cols)), shape=shape).tocsr()
            M.sum_duplicates()
            return M
        for _ in range(a.reps):
            got, ms = clock(lambda: DeviceCorpus.from_pairs(rows, vals, shape=shape, cols=cols))
            line['host_pairs_ms'].append(ms)
            line['host_pairs_kernel_ms'].append(round(got.ingest_ms, 3))
            if torch is not None:
                dev, ms = clock(lambda: DeviceCorpus.from_pairs(tr, tv, shape=shape, cols=tc))
                line['device_pairs_ms'].append(ms)
                line['device_pairs_kernel_ms'].append(round(dev.ingest_ms, 3))
            want, ms = clock(by_scipy)
            line['scipy_ms'].append(ms)
            made, ms = clock(lambda: DeviceCorpus(by_scipy()))
            line['scipy_ingest_ms'].append(ms)
            want.sort_indices()
            equal = equal and same(got.to_scipy(), want) and same(made.to_scipy(), want) and (torch is None or same(dev.to_scipy(), want))
            line['rows_rewritten'] = int(got.rows_rewritten)
            close((got, made) + ((dev,) if torch is not None else ()))
        for key in [k for k in line if k.endswith('_ms')]:
            if line[key]:
                line[key + '_median'] = float(np.median(line[key]))
        line['equal'] = equal
        emit(line)

    corpus = DeviceCorpus(A)
    line = dict(what='split_entries', n=a.n, d=a.d, stored=int(A.nnz), held_out=0.05, device_ms=[], kernel_ms=[], host_ms=[], host_reingest_ms=[])
    equal = True
    for _ in range(a.reps):
        got, ms = clock(lambda: corpus.split_entries(0.05, 12345))
        line['device_ms'].append(ms)
        line['kernel_ms'].append(round(got[0].ingest_ms, 3))
        want, ms = clock(lambda: si.split_entries(A, 0.05, 12345))
        line['host_ms'].append(ms)
        made, ms = clock(lambda: tuple(DeviceCorpus(m) for m in si.split_entries(A, 0.05, 12345)))
        line['host_reingest_ms'].append(ms)
        o, h = (c.to_scipy() for c in got)
        total = sp.csr_matrix(o + h)
        total.sort_indices()
        back = sp.csr_matrix(want[0] + want[1])
        back.sort_indices()
        equal = equal and same(total, A) and same(back, A) and o.nnz + h.nnz == A.nnz
        line['held_share'] = [round(h.nnz / float(A.nnz), 5), round(want[1].nnz / float(A.nnz), 5)]
        close(got)
        close(made)
    for key in ('device_ms', 'kernel_ms', 'host_ms', 'host_reingest_ms'):
        line[key + '_median'] = float(np.median(line[key]))
    line['equal'] = equal
    emit(line)
    corpus.close()
    assert corpus_memory() == (0, 0)


if __name__ == '__main__':
    main()
