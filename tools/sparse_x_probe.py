"""Sparse-X topic models: sweeps/s of the handle that keeps a CSR X on the device (RRI_UNWEIGHTED_SPARSE) against the handle
that densifies it, on Zipf term counts, and the one read-only pass per topic step (k_spx_pass) timed by HIP events.

    python tools/sparse_x_probe.py [--large] [--sweeps S]

One JSON line per case.  Cases: 100000 x 10000 fp32, k = 50, at 0.2 %, 1 % and 5 % density (both handles), and with --large
the shape of tests/test_sparse_x_gpu.py::test_matrix_larger_than_the_device (sparse handle only: its dense form does not fit).
Bytes per pass = 12 B per stored entry (6 B per entry and copy: 2 of offset, 4 of value); per topic step add the 8 k n bytes
k_wcol reads for the Gram row."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rri_nmf_amd.engine import RRIEngine  # noqa: E402

HBM = 8.0e12


def zipf_counts(n, d, density, seed=0, a=1.1):
    """term counts: nnz draws of (row uniform, column Zipf(a)), duplicates summed"""
    rs = np.random.RandomState(seed)
    m = int(n * d * density)
    p = 1.0 / np.arange(1, d + 1) ** a
    cdf = np.cumsum(p / p.sum())
    cols = np.minimum(np.searchsorted(cdf, rs.rand(m)), d - 1).astype(np.int32)
    rows = rs.randint(0, n, size=m).astype(np.int32)
    X = sp.csr_matrix((np.ones(m, dtype=np.float32), (rows, cols)), shape=(n, d))
    X.sum_duplicates()
    return X


def fixed_rows(n, d, per_row, seed=0):
    rs = np.random.RandomState(seed)
    base = rs.randint(0, d, size=n).astype(np.int64)
    cols = np.sort((base[:, None] + np.arange(per_row, dtype=np.int64)[None, :] * 4999) % d, axis=1).astype(np.int32)
    vals = rs.randint(1, 8, size=n * per_row).astype(np.float32)
    return sp.csr_matrix((vals, cols.ravel(), np.arange(0, n * per_row + 1, per_row, dtype=np.int64)), shape=(n, d))


def measure(X, k, sparse_x, sweeps, warm=1):
    n, d = X.shape
    rs = np.random.RandomState(1)
    with RRIEngine(n, d, k, dtype=np.float32, sparse_x=sparse_x) as e:
        t0 = time.perf_counter()
        e.upload_X_csr(X)
        e.synchronize()
        upload_s = time.perf_counter() - t0
        T0 = rs.rand(k, d)
        e.set_W(rs.rand(n, k) / k)
        e.set_T(T0 / T0.sum(1, keepdims=True))
        e.set_params(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
        e.sweep(warm)
        e.synchronize()
        t0 = time.perf_counter()
        e.sweep(sweeps)
        e.synchronize()
        dt = time.perf_counter() - t0
        e.timing_enable(True)
        e.sweep(1)
        e.synchronize()
        launches, ms = e.timing_read(0)
        e.timing_enable(False)
    out = {'handle': 'csr' if sparse_x else 'dense', 'resets': e.n_resets_used, 'sweeps_per_s': sweeps / dt, 'ms_per_sweep': 1e3 * dt / sweeps,
           'upload_s': upload_s}
    if launches:
        out['pass_launches'] = int(launches)
        out['pass_us'] = 1e3 * ms / launches
        if sparse_x:
            out['pass_bytes'] = 12 * X.nnz
            out['pass_frac_8TBs'] = 12 * X.nnz / (ms / launches * 1e-3) / HBM
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--large', action='store_true')
    ap.add_argument('--sweeps', type=int, default=5)
    args = ap.parse_args()
    n, d, k = 100000, 10000, 50
    for dens in (0.002, 0.01, 0.05):
        X = zipf_counts(n, d, dens, seed=int(dens * 1e4))
        share = float(np.bincount(X.indices, minlength=d).max()) / X.nnz
        for sparse_x in (True, False):
            r = measure(X, k, sparse_x, args.sweeps)
            r.update({'case': '%dx%d fp32 k=%d Zipf %.1f%%' % (n, d, k, 100 * dens), 'nnz': int(X.nnz),
                      'density': X.nnz / float(n * d), 'top_column_share': share,
                      'step_bytes_csr': 12 * X.nnz + 8 * k * n})
            print(json.dumps(r), flush=True)
    if args.large:
        import torch
        total = torch.cuda.mem_get_info(0)[1]
        d, per_row, k = 100000, 20, 8
        n = max(3000000, int(1.2 * total / (4 * d)) + 1)
        X = fixed_rows(n, d, per_row)
        r = measure(X, k, True, 3)
        r.update({'case': '%dx%d fp32 k=%d, %d per row (dense form %.0f GB > device %.0f GB)' %
                  (n, d, k, per_row, 4.0 * n * d / 1e9, total / 1e9), 'nnz': int(X.nnz),
                  'step_bytes_csr': 12 * X.nnz + 8 * k * n})
        print(json.dumps(r), flush=True)


if __name__ == '__main__':
    main()
