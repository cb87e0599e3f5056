"""Co-document counts of topics' top words at the topic-model shape: the device route (rri_cooccurrence_counts behind
RRIEngine.cooccurrence_counts) against a scipy route, in one process on one box.

    python tools/cooc_probe.py [--n 100000 --d 10000 --k 50 --out FILE]

Zipf term counts (tools/sparse_x_probe.zipf_counts) at the two densities the README quotes for a CSR X (asked 0.2 % and 5 %: about
1.6 M and 23.5 M stored entries); k groups of n_words = 10 and 20 distinct words each, drawn from the same Zipf law, so a group
mixes frequent and rare words as a topic's top words do.  JSON lines, one per (density, n_words):
  kernel_ms   k_cooc_masks + k_cooc_count by HIP events (rri_timing_read id 6): the sum over the launches of one call, the mean of
              three calls after a warm-up
  masks_ms    k_cooc_masks alone, the same way in three further calls (timing every second launch of id 6)
  wall_ms     RRIEngine.cooccurrence_counts, three calls: canonical copy of the matrix, upload, the launches, the counts back
  abi_ms      the same without the canonical copy: rri_cooccurrence_counts on arrays that are canonical already
  host_ms     A.tocsc() once, then per group B = A[:, words] and B.T @ B, the groups dealt to 16 threads
  equal       whether the two routes give the same counts
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparse_x_probe import zipf_counts  # noqa: E402


def zipf_words(k, n_words, d, seed, a=1.1):
    rng = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, d + 1) ** a
    p /= p.sum()
    return np.stack([rng.choice(d, size=n_words, replace=False, p=p) for _ in range(k)]).astype(np.int32)


def host_route(A, words, threads=16):
    Ac = A.tocsc()
    codf = np.zeros((words.shape[0], words.shape[1], words.shape[1]), dtype=np.int64)

    def work(g):
        B = Ac[:, words[g]]
        codf[g] = (B.T @ B).toarray()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(work, range(words.shape[0])))
    return codf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from rri_nmf_amd.engine import RRIEngine
    n, d, k = a.n, a.d, a.k
    e = RRIEngine(4, 4, 2, dtype=np.float64)
    lines = []
    for density in (0.002, 0.05):
        A = zipf_counts(n, d, density)
        A.data = np.ones(A.nnz, dtype=np.int64)                  # presence: the host route's products are then the counts
        A.sort_indices()
        e.cooccurrence_counts(A[:64], zipf_words(2, 4, d, 0))      # warm-up: the code objects, the first launches
        for n_words in (10, 20):
            words = zipf_words(k, n_words, d, seed=n_words)
            e.timing_enable(True)
            e.timing_read(6)
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                df, codf = e.cooccurrence_counts(A, words)
                walls.append(time.perf_counter() - t0)
            launches, ms = e.timing_read(6)
            e.timing_enable(True, every=2)                            # every second launch of id 6, from the first: k_cooc_masks alone
            for _ in range(3):
                e.cooccurrence_counts(A, words)
            mask_launches, mask_ms = e.timing_read(6)
            e.timing_enable(False)
            assert launches == 6 and mask_launches == 3, (launches, mask_launches)      # one row chunk at these sizes
            indptr, indices = A.indptr.astype(np.int64), A.indices.astype(np.int32)
            df2, codf2 = np.zeros_like(df), np.zeros_like(codf)
            I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
            abi = []
            for _ in range(3):
                t0 = time.perf_counter()
                st = e._lib.rri_cooccurrence_counts(e._h, indptr.ctypes.data_as(I64P), indices.ctypes.data_as(I32P), n, d,
                                                    words.ctypes.data_as(I32P), k, n_words, df2.ctypes.data_as(I64P),
                                                    codf2.ctypes.data_as(I64P))
                abi.append(time.perf_counter() - t0)
                assert st == 0
            hosts = []
            for _ in range(2):
                t0 = time.perf_counter()
                want = host_route(A, words)
                hosts.append(time.perf_counter() - t0)
            equal = bool(np.array_equal(codf, want) and np.array_equal(codf2, want) and
                         np.array_equal(df, np.diagonal(want, axis1=1, axis2=2)))
            lines.append(dict(what='cooc', n=n, d=d, k=k, n_words=n_words, nnz=int(A.nnz), launches_per_call=launches // 3,
                              kernel_ms=round(ms / 3, 3), masks_ms=round(mask_ms / 3, 3), wall_ms=[round(1e3 * w, 1) for w in walls],
                              abi_ms=[round(1e3 * w, 1) for w in abi], host_ms=[round(1e3 * w, 1) for w in hosts], host_threads=16,
                              rows_with_a_word=int(np.count_nonzero(np.diff(A[:, np.unique(words)].tocsr().indptr))), equal=equal))
            print(json.dumps(lines[-1]), flush=True)
            assert equal
    e.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(json.dumps(ln) for ln in lines) + '\n')


if __name__ == '__main__':
    main()
