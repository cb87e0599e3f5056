"""Ranking and recommending against resident corpora against the host routes they replace, in one process on one box.

    python tools/corpus_rank_probe.py --ratings 5000000|50000000 [--n 100000 --d 10000 --k 20 --reps 5 --out FILE]
    python tools/corpus_rank_probe.py --fixture [--out FILE]        the 617-rating fixture of tests/golden, 100 x 200

Uniform random (user, item) pairs with stars 1 .. 5, as tools/corpus_rs_probe.py draws them; 5 % of the entries are held out by
DeviceCorpus.split_entries.  One size per process, so that a job runs each under a time limit of its own.  The routes alternate
inside the process, `reps` times each after one warm-up; every list holds all the times and `*_median` their median.  Host-clock
times are taken around blocking calls; kernel times are the library's HIP-event times (kernel_ms of the new entry points).  The
factors are those of NMF_RS_Estimator.fit_corpus(train, max_iter=--max-iter).  JSON lines:
  ranking_score, exclusion    the ranking metrics of the held-out entries at n_items = 10; exclusion 'full' (train and held-out
                              together: what seen_ holds after a fit that was given both) or 'train'
    host_ms          NMF_RS_Estimator.ranking_score(test matrix) with seen_ set: the parent's route from host data
    download_ms      test.to_scipy(), which that route needs first when the held-out entries are resident
    seen_ms          corpus_fit.pattern_of(exclusion corpus), the download behind seen_
    parent_ms        host_ms + download_ms + seen_ms, rep by rep: the parent's route from resident data
    corpus_ms        NMF_RS_Estimator.ranking_score_corpus(test, exclude=corpus)
    kernel_ms        the HIP-event time of its kernels (pieces, ranks, row terms, totals), from a direct call
    equal_counts, max_rel_diff    the two dicts: counts equal, the largest relative difference of a metric
  recommend, users   the 10 best items per user, the full corpus excluded; users 'all' or 64
    host_ms          NMF_RS_Estimator.recommend(users) with seen_ set (the seen_ download is not counted again)
    corpus_ms        NMF_RS_Estimator.recommend_corpus(users, exclude=full)
    kernel_ms        the HIP-event time of k_topn_rows in the corpus route, from a direct call
    equal            items and scores equal
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
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--max-iter', type=int, default=3)
    ap.add_argument('--fixture', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from rri_nmf_amd import corpus_rank, sklearn_interface as si
    from rri_nmf_amd.corpus_fit import pattern_of
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
        full = DeviceCorpus(A)
        k, held_out = 5, 0.2
    else:
        n, d, m = a.n, a.d, a.ratings
        ij = np.column_stack((rs.randint(0, n, m), rs.randint(0, d, m))).astype(np.int64)
        y = rs.randint(1, 6, m).astype(np.float64)
        full = DeviceCorpus.from_pairs(ij, y, shape=(n, d))
        del ij, y
        k, held_out = a.k, 0.05
    train, test = full.split_entries(held_out, 0)
    base = dict(n=n, d=d, k=k, stored=int(full.nnz), held=int(test.nnz))
    est = si.NMF_RS_Estimator(n, d, k, random_state=0, max_iter=a.max_iter, use_validation_early_stopping=False).fit_corpus(train, keep_seen=False)
    eng = RRIEngine(n, d, k, dtype=np.float64, weighted=False)
    eng.set_W(est.W)
    eng.set_T(est.T)
    mem = device_memory()

    # ---- the ranking metrics of the held-out entries
    for name, excl in (('full', full), ('train', train)):
        line = dict(base, what='ranking_score', exclusion=name, n_items=10, host_ms=[], download_ms=[], seen_ms=[], parent_ms=[], corpus_ms=[],
                    kernel_ms=[])
        for rep in range(a.reps + 1):
            seen, t_seen = clock(lambda: pattern_of(excl))
            T, t_down = clock(test.to_scipy)
            est.seen_ = seen
            want, t_host = clock(lambda: est.ranking_score(T, n_items=10))
            got, t_cor = clock(lambda: est.ranking_score_corpus(test, n_items=10, exclude=excl))
            _, ms = corpus_rank.ranking_sums(eng, test, 10, exclude=excl)
            if rep:
                for key, val in (('host_ms', t_host), ('download_ms', t_down), ('seen_ms', t_seen), ('parent_ms', round(t_host + t_down + t_seen, 3)),
                                 ('corpus_ms', t_cor), ('kernel_ms', round(ms, 4))):
                    line[key].append(val)
        metrics = [m_ for m_ in corpus_rank.METRIC_NAMES if want[m_] == want[m_]]
        line.update(users=got['users'], targets_not_eligible=got['targets_not_eligible'],
                    equal_counts=all(got[c] == want[c] for c in ('users', 'targets', 'targets_not_eligible')),
                    max_rel_diff=max([abs(got[m_] - want[m_]) / abs(want[m_]) for m_ in metrics if want[m_] != 0] or [0.0]),
                    ndcg=got['ndcg'], hit_rate=got['hit_rate'])
        emit(medians(line))
        del T, seen

    # ---- the 10 best items per user, the full corpus excluded
    est.seen_ = pattern_of(full)
    for name, users in (('all', None), (64, rs.randint(0, n, 64).astype(np.int64))):
        line = dict(base, what='recommend', users=name, n_items=10, host_ms=[], corpus_ms=[], kernel_ms=[])
        for rep in range(a.reps + 1):
            want, t_host = clock(lambda: est.recommend(users, n_items=10))
            got, t_cor = clock(lambda: est.recommend_corpus(users, n_items=10, exclude=full))
            ms = corpus_rank.topn_rows(eng, users, 10, exclude=full, clip=(est.min_rating, est.max_rating))[2]
            if rep:
                line['host_ms'].append(t_host)
                line['corpus_ms'].append(t_cor)
                line['kernel_ms'].append(round(ms, 4))
        line['equal'] = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True))
        emit(medians(line))
    assert device_memory() == mem
    eng.close()
    for c in (train, test, full):
        c.close()
    assert corpus_memory() == (0, 0)


if __name__ == '__main__':
    main()
