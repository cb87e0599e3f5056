"""The recommender fit from a resident corpus against the host routes it replaces, in one process on one box.

    python tools/corpus_rs_probe.py --ratings 5000000|50000000 [--n 100000 --d 10000 --reps 5 --out FILE]
    python tools/corpus_rs_probe.py --fixture [--out FILE]        the 617-rating fixture of tests/golden, 100 x 200

Uniform random (user, item) pairs with stars 1 .. 5, as tools/e2e_rs_probe.py draws them (a pair drawn twice has its stars added,
on every route).  One size per process, so that a job runs each under a time limit of its own.  The routes alternate inside the
process, `reps` times each after one warm-up; every list holds all the times and `*_median` their median.  Host-clock times are
taken around blocking calls; kernel times are the library's HIP-event times.  JSON lines:
  store            a ready pattern-only handle (weighted='sparse') from data that is already where the route starts
    csr_ms           RRIEngine.upload_observed_csr(A) from the scipy matrix: checks, uploads, the host's counting sorts
    corpus_ms        corpus_fit.upload_observed_corpus(engine, corpus) from the resident corpus
    build_kernel_ms  the HIP-event time of the device build's kernels (sparse_store()['build_us'])
    equal            whether both leave the same two blocked copies
  score, k         one early-stop score on 5 % held-out entries with random factors of rank k
    host_ms          RRIEngine.masked_rmse on host (i, j, value) lists: the host's check, 24 bytes per entry up, one thread per entry
    corpus_ms        corpus_fit.entries_error on the resident held-out corpus
    kernel_ms        the HIP-event time of its kernels (transpose of T, the entries kernel, the sums)
    stream_bytes_per_entry, gather_bytes_per_entry   from the shapes: what the entries kernel streams from HBM per entry (4-byte
                     column, 8-byte value, a piece's 16-byte descriptor and 16 bytes of partials over its entries) and what it
                     gathers through the caches (the entry's row of the transposed T, kp doubles)
    rel_diff         |rmse_host - rmse_corpus| / rmse
  fit, k           end to end, max_iter sweeps at most, early stopping on 5 %
    pairs_ms         NMF_RS_Estimator.fit(index_pairs, ratings)
    corpus_ms        DeviceCorpus.from_pairs(index_pairs, ratings) and NMF_RS_Estimator.fit_corpus(corpus), the corpus closed after
    from_pairs_ms    the share of from_pairs in corpus_ms
    sweeps_*         sweeps kept; test_rmse_*: the clipped RMSE of either fit on 2 % fresh pairs (the two routes hold out
                     different 5 %, so their fits differ: only the times are compared)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock(f):
    t0 = time.perf_counter()
    out = f()
    return out, round(1e3 * (time.perf_counter() - t0), 3)


def medians(line):
    for key in [k for k in line if k.endswith('_ms')]:
        if line[key]:
            line[key + '_median'] = float(np.median(line[key]))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ratings', type=int, default=5000000)
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--max-iter', type=int, default=30)
    ap.add_argument('--fit-k', type=int, default=20)
    ap.add_argument('--fixture', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from rri_nmf_amd import sklearn_interface as si
    from rri_nmf_amd.corpus_fit import entries_error, upload_observed_corpus
    from rri_nmf_amd.engine import DeviceCorpus, RRIEngine, corpus_memory, device_memory

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(line) + '\n')

    rs = np.random.RandomState(0)
    if a.fixture:
        A = sp.load_npz(os.path.join(ROOT, 'tests', 'golden', 'ref_data', 'recsys_data_train.npz')).tocsr().astype(np.float64)
        A.eliminate_zeros()
        n, d = A.shape
        i, j = A.nonzero()
        ij, y = np.column_stack((i, j)).astype(np.int64), np.asarray(A[i, j]).ravel()
        T = sp.load_npz(os.path.join(ROOT, 'tests', 'golden', 'ref_data', 'recsys_data_test.npz')).tocsr().astype(np.float64)
        ti, tj = T.nonzero()
        tij, ty = np.column_stack((ti, tj)).astype(np.int64), np.asarray(T[ti, tj]).ravel()
        fit_k = 5
    else:
        n, d, m = a.n, a.d, a.ratings
        ij = np.column_stack((rs.randint(0, n, m), rs.randint(0, d, m))).astype(np.int64)
        y = rs.randint(1, 6, m).astype(np.float64)
        mt = max(m // 50, 1)
        tij = np.column_stack((rs.randint(0, n, mt), rs.randint(0, d, mt))).astype(np.int64)
        ty = rs.randint(1, 6, mt).astype(np.float64)
        fit_k = a.fit_k
    base = dict(n=n, d=d, ratings=int(y.size))

    # ---- (a) a ready pattern-only handle
    corpus = DeviceCorpus.from_pairs(ij, y, shape=(n, d))
    A = corpus.to_scipy()
    lo, hi = corpus.value_range()
    line = dict(base, what='store', stored=int(A.nnz), csr_ms=[], corpus_ms=[], build_kernel_ms=[])
    equal = True
    for rep in range(a.reps + 1):
        with RRIEngine(n, d, 5, dtype=np.float32, weighted='sparse') as ea, RRIEngine(n, d, 5, dtype=np.float32, weighted='sparse') as eb:
            _, t_csr = clock(lambda: ea.upload_observed_csr(A))
            _, t_cor = clock(lambda: upload_observed_corpus(eb, corpus))
            sa, sb = ea.sparse_store(1), eb.sparse_store(1)
            equal = equal and all(np.array_equal(sa[f], sb[f]) for f in ('segptr', 'idx', 'perm', 'work'))
            if rep:
                line['csr_ms'].append(t_csr)
                line['corpus_ms'].append(t_cor)
                line['build_kernel_ms'].append(sb['build_us'] / 1e3)
    line['equal'] = bool(equal)
    emit(medians(line))

    # ---- (b) one early-stop score on 5 % held out
    train, held = corpus.split_entries(0.05, 0)
    H = held.to_scipy().tocoo()
    hi_, hj_, hv_ = H.row.astype(np.int64), H.col.astype(np.int64), H.data.copy()
    pieces = int(np.sum(-(-np.diff(held.to_scipy().indptr) // 256)))
    for k in ((5,) if a.fixture else (20, 50)):
        W, T = rs.rand(n, k) * 3.0 / np.sqrt(k), rs.rand(k, d) * 3.0 / np.sqrt(k)
        line = dict(base, what='score', k=k, held=int(held.nnz), host_ms=[], corpus_ms=[], kernel_ms=[])
        with RRIEngine(n, d, k, dtype=np.float64, weighted=False) as eng:
            eng.set_W(W)
            eng.set_T(T)
            mem = device_memory()
            for rep in range(a.reps + 1):
                s_host, t_host = clock(lambda: eng.masked_rmse(hi_, hj_, hv_, lo, hi))
                res, t_cor = clock(lambda: entries_error(eng, held, clip=(lo, hi)))
                if rep:
                    line['host_ms'].append(t_host)
                    line['corpus_ms'].append(t_cor)
                    line['kernel_ms'].append(round(res['kernel_ms'], 4))
            assert device_memory() == mem
        kp = (k + 1) & ~1
        line.update(rmse=res['rmse'], rel_diff=abs(s_host - res['rmse']) / res['rmse'],
                    stream_bytes_per_entry=round(12.0 + 32.0 * pieces / max(held.nnz, 1), 3), gather_bytes_per_entry=8 * kp)
        emit(medians(line))
    train.close()
    held.close()
    corpus.close()

    # ---- (c) end to end
    test = DeviceCorpus.from_pairs(tij, ty, shape=(n, d))
    line = dict(base, what='fit', k=fit_k, max_iter=a.max_iter, pairs_ms=[], corpus_ms=[], from_pairs_ms=[])
    for rep in range(a.reps + 1):
        Ea = si.NMF_RS_Estimator(n, d, fit_k, random_state=0, max_iter=a.max_iter)
        _, t_pairs = clock(lambda: Ea.fit(ij, y))
        Eb = si.NMF_RS_Estimator(n, d, fit_k, random_state=0, max_iter=a.max_iter)
        t0 = time.perf_counter()
        c, t_from = clock(lambda: DeviceCorpus.from_pairs(ij, y, shape=(n, d)))
        Eb.fit_corpus(c)
        c.close()
        t_cor = round(1e3 * (time.perf_counter() - t0), 3)
        if rep:
            line['pairs_ms'].append(t_pairs)
            line['corpus_ms'].append(t_cor)
            line['from_pairs_ms'].append(t_from)
    line.update(sweeps_pairs=len(Ea.nmf_outputs['iter_cputime']), sweeps_corpus=len(Eb.nmf_outputs['iter_cputime']),
                test_rmse_pairs=Ea.score_corpus(test), test_rmse_corpus=Eb.score_corpus(test))
    emit(medians(line))
    test.close()
    assert corpus_memory() == (0, 0)


if __name__ == '__main__':
    main()
