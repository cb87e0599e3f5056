"""The split of a resident corpus by row at the recommender shape: what DeviceCorpus.split_rows costs against the split by entry on
the same corpus and against the host route on the downloaded matrix, and ranking_score_new_users against the same protocol run by
hand through the host, in one process on one box.

    python tools/rowsplit_probe.py --drawn 5000000|50000000 [--n 100000 --d 10000 --reps 5 --k 8 --out FILE]

`drawn` uniform random (row, column) pairs with ratings 1 .. 5 become a corpus through DeviceCorpus.from_pairs (a pair drawn twice
is one entry).  At 5e6 drawn a row has about 50 entries -- mostly the wave class of the selection --, at 5e7 about 500: the block
class throughout.  One size per process, so that a job runs each under a time limit of its own.  The routes alternate inside the
process, `reps` times each; every list holds all the times and `*_median` their median.  JSON lines:
  split_rows, mode = n_held_1 | held_out_0.2
    device_ms            corpus.split_rows(...), from a resident corpus to two resident corpora
    kernel_ms            the HIP-event time of its kernels (ingest_ms): selection, count, write
    no_select_kernel_ms  ... of split_rows(held_out=1.0, min_observed=0) on the same corpus: no row needs a selection, so count and
                         write alone; select_ms_median = kernel - no_select, select_share = that over device_ms: the share of a call
                         that the selection (at 5e7: the block class) costs
    entries_device_ms    corpus.split_entries(0.05) on the same corpus, entries_kernel_ms its kernels
    host_ms              sklearn_interface.split_rows on the scipy matrix
    host_reingest_ms     that and DeviceCorpus of both parts: what it takes without the device route to have the parts resident
    rows_wave, rows_block, rows_known   the rows by selection class under this mode
    equal                observed + held == A and the per-row counts == the quota, on both routes (the generators differ, so the
                         parts do)
  new_users              the second half of the rows as users a fit on the first half (k topics, two sweeps) never saw, n_held = 1
    device_ms            NMF_RS_Estimator.ranking_score_new_users(new, n_items=10, n_held=1)
    host_ms              new.to_scipy(), sklearn_interface.split_rows, transform, ranking_score with the held pairs
    users, targets       of either route (equal; the metrics differ with the split)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def whole(parts, A, quota):
    """observed + held == A, and held has the quota of every row"""
    o, h = parts
    total = sp.csr_matrix(o + h)
    total.sort_indices()
    return same(total, A) and o.nnz + h.nnz == A.nnz and np.array_equal(np.diff(h.indptr), quota)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--drawn', type=int, default=5000000)
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--k', type=int, default=8)
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

    rng = np.random.RandomState(0)
    rows = rng.randint(0, a.n, size=a.drawn).astype(np.int32)
    cols = rng.randint(0, a.d, size=a.drawn).astype(np.int32)
    vals = rng.randint(1, 6, size=a.drawn).astype(np.float64)
    corpus = DeviceCorpus.from_pairs(rows, vals, shape=(a.n, a.d), cols=cols)
    del rows, cols, vals
    A = corpus.to_scipy()
    A.sort_indices()
    lengths = np.diff(A.indptr).astype(np.int64)
    small = corpus.take_rows(np.arange(min(a.n, 500)))          # warm-up: the code objects, the first launches
    for kw in (dict(n_held=1), dict(held_out=0.2), dict(held_out=1.0, min_observed=0)):
        close(small.split_rows(**kw))
    close(small.split_entries(0.05, 0))
    small.close()

    for mode, kw in (('n_held_1', dict(n_held=1)), ('held_out_0.2', dict(held_out=0.2))):
        quota = DeviceCorpus._split_rows_quota(lengths, *DeviceCorpus._split_rows_request(kw.get('n_held'), kw.get('held_out'), 1))
        select = (quota > 0) & (quota < lengths)
        line = dict(what='split_rows', mode=mode, n=a.n, d=a.d, drawn=a.drawn, stored=int(A.nnz), held=int(quota.sum()),
                    rows_wave=int((select & (lengths <= 64)).sum()), rows_block=int((select & (lengths > 64)).sum()), rows_known=int((~select).sum()),
                    device_ms=[], kernel_ms=[], no_select_kernel_ms=[], entries_device_ms=[], entries_kernel_ms=[], host_ms=[], host_reingest_ms=[])
        equal = True
        for rep in range(a.reps):
            got, ms = clock(lambda: corpus.split_rows(random_state=12345, **kw))
            line['device_ms'].append(ms)
            line['kernel_ms'].append(round(got[0].ingest_ms, 3))
            plain = corpus.split_rows(held_out=1.0, min_observed=0, random_state=12345)
            line['no_select_kernel_ms'].append(round(plain[0].ingest_ms, 3))
            close(plain)
            by_entry, ms = clock(lambda: corpus.split_entries(0.05, 12345))
            line['entries_device_ms'].append(ms)
            line['entries_kernel_ms'].append(round(by_entry[0].ingest_ms, 3))
            close(by_entry)
            want, ms = clock(lambda: si.split_rows(A, random_state=12345, **kw))
            line['host_ms'].append(ms)
            made, ms = clock(lambda: tuple(DeviceCorpus(m) for m in si.split_rows(A, random_state=12345, **kw)))
            line['host_reingest_ms'].append(ms)
            if rep == 0:            # once: the check itself is host work of the corpus's size
                equal = whole(tuple(c.to_scipy() for c in got), A, quota) and whole(want, A, quota)
            close(got)
            close(made)
            del want
        for key in [k for k in line if k.endswith('_ms')]:
            line[key + '_median'] = float(np.median(line[key]))
        line['select_ms_median'] = round(line['kernel_ms_median'] - line['no_select_kernel_ms_median'], 3)
        line['select_share'] = round(line['select_ms_median'] / line['device_ms_median'], 4)
        line['equal'] = bool(equal)
        emit(line)

    # users a fit never saw: the second half of the rows against a fit on the first
    half = a.n // 2
    with corpus.take_rows(np.arange(half)) as known:
        E = si.NMF_RS_Estimator(half, a.d, a.k, random_state=0, max_iter=2, use_validation_early_stopping=False,
                                nmf_kwargs={'device_init': True}).fit_corpus(known, keep_seen=False)
    new = corpus.take_rows(np.arange(half, a.n))

    def by_hand():
        N = new.to_scipy()
        O, H = si.split_rows(N, n_held=1, random_state=E.random_state)
        W = E.transform(O)
        est = si.NMF_RS_Estimator(O.shape[0], a.d, a.k, W=W, T=E.T)
        est.min_rating, est.max_rating = E.min_rating, E.max_rating
        est.seen_ = sp.csr_matrix((np.ones(O.nnz), O.indices, O.indptr), shape=O.shape)
        return est.ranking_score(H, n_items=10)
    line = dict(what='new_users', n=a.n - half, d=a.d, k=a.k, stored=int(new.nnz), n_held=1, device_ms=[], host_ms=[])
    for _ in range(a.reps):
        got, ms = clock(lambda: E.ranking_score_new_users(new, n_items=10, n_held=1))
        line['device_ms'].append(ms)
        want, ms = clock(by_hand)
        line['host_ms'].append(ms)
        line['users'], line['targets'] = [int(got['users']), int(want['users'])], [int(got['targets']), int(want['targets'])]
        line['hit_rate'] = [round(float(got['hit_rate']), 5), round(float(want['hit_rate']), 5)]
    for key in ('device_ms', 'host_ms'):
        line[key + '_median'] = float(np.median(line[key]))
    line['equal'] = bool(line['users'][0] == line['users'][1] and line['targets'][0] == line['targets'][1] == got['held_entries'])
    emit(line)
    new.close()
    corpus.close()
    assert corpus_memory() == (0, 0)


if __name__ == '__main__':
    main()
