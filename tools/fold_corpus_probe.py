"""The one-launch fold sweep of a pattern-only handle (include/rri_fold.h) against the launch-per-topic schedule, in one process on
one box; and NMF_RS_Estimator.transform_corpus against transform.

    python tools/fold_corpus_probe.py --ratings 5000000|50000000 --k 20|50 [--n 100000 --d 10000 --reps 5 --out FILE]
    python tools/fold_corpus_probe.py --new-users 64 [--per-user 50 --k 20 --out FILE]     64 new users on d = 10000 items
    python tools/fold_corpus_probe.py --fixture [--out FILE]                               the 617-rating fixture of tests/golden

Uniform random (user, item) pairs with stars 1 .. 5, as tools/corpus_rank_probe.py draws them.  One size per process, so that a job
runs each under a time limit of its own.  T is a random matrix with rows on the simplex (no fit is timed here); W starts from the
same random matrix on both sides.  JSON lines:
  schedules        twin handles built from the one corpus; in rep r handle r % 2 is asked for the schedule and the other one is
                   not (set_fold_schedule 1 / 0), so that neither schedule owns a buffer placement.  --sweeps sweeps (4: what
                   transform runs) with fix_T, the factors set again before each rep; one warm-up rep for each pairing.
    fold_ms, stepped_ms          wall time of the blocking sweep(--sweeps) call, per rep, and their medians
    fold_kernel_ms, stepped_kernel_ms     HIP-event time of the timed kernel ids of the handle (rri_timing_read) in one more rep
                                 each, timing enabled: {id: [scopes, ms]}; the fold launch is id 1 (k_wfold_rows, its verdict
                                 and repair), the launch-per-topic schedule's blocked passes are id 3 and its k_wwcol id 1; the
                                 column checks of that schedule are not timed by the library
    info             fold_info of handle 0 at the end;  rel_diff  ||W_fold - W_stepped|| / ||W_stepped|| after the last rep
  end_to_end       NMF_RS_Estimator.transform_corpus(new) against transform(matrix): corpus_ms, host_ms (the matrix already on
                   the host), download_ms (new.to_scipy(), which the host route needs first when the ratings are resident),
                   rel_diff of M .* (W T) between the two
What is NOT measured: a fit; the default start of W through the device products is inside both end-to-end routes; k > 64; more
than one device.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ratings', type=int, default=5000000)
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--sweeps', type=int, default=4)
    ap.add_argument('--new-users', type=int, default=0)
    ap.add_argument('--per-user', type=int, default=50)
    ap.add_argument('--fixture', action='store_true')
    ap.add_argument('--no-end-to-end', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from rri_nmf_amd import sklearn_interface as si
    from rri_nmf_amd.corpus_fit import upload_observed_corpus
    from rri_nmf_amd.engine import DeviceCorpus, RRIEngine
    from rri_nmf_amd.fold import fold_info, set_fold_schedule

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
        n, d, k = A.shape[0], A.shape[1], 5
        new = DeviceCorpus(A)
    else:
        n, d, k = (a.new_users, a.d, a.k) if a.new_users else (a.n, a.d, a.k)
        m = a.new_users * a.per_user if a.new_users else a.ratings
        ij = np.column_stack((rs.randint(0, n, m), rs.randint(0, d, m))).astype(np.int64)
        y = rs.randint(1, 6, m).astype(np.float64)
        new = DeviceCorpus.from_pairs(ij, y, shape=(n, d))
        del ij, y
    T = rs.rand(k, d)
    T /= T.sum(axis=1, keepdims=True)
    W0 = rs.rand(n, k)
    base = dict(n=n, d=d, k=k, stored=int(new.nnz), sweeps=a.sweeps)
    params = dict(fix_T=True, t_row_sum=1.0, reset_topic_method='random', fix_reset_seed=True)

    # ---- the two schedules on twin handles
    twins = []
    for _ in range(2):
        e = RRIEngine(n, d, k, dtype=np.float64, weighted='sparse')
        upload_observed_corpus(e, new)
        e.set_T(T)
        e.set_params(**params)
        twins.append(e)

    def rep(asked):
        """handle `asked` takes the fold schedule, the other one the launch-per-topic schedule: (fold ms, stepped ms)"""
        out = {}
        for h, e in enumerate(twins):
            set_fold_schedule(e, h == asked)
            e.set_W(W0)
            _, out[h == asked] = clock(lambda: e.sweep(a.sweeps))
        return out[True], out[False]

    line = dict(base, what='schedules', fold_ms=[], stepped_ms=[])
    for asked in (0, 1):
        rep(asked)                                   # warm-up of each pairing
    for r in range(a.reps):
        f_ms, s_ms = rep(r % 2)
        line['fold_ms'].append(f_ms)
        line['stepped_ms'].append(s_ms)
    line['rel_diff'] = float(np.linalg.norm(twins[0].get_W() - twins[1].get_W()) / np.linalg.norm(twins[1].get_W()))
    for key in ('fold_ms', 'stepped_ms'):
        line[key + '_median'] = float(np.median(line[key]))
        line[key[:-3] + '_per_sweep_ms'] = round(line[key + '_median'] / a.sweeps, 4)
    for e in twins:
        e.timing_enable()
    rep(0)
    for name, e in (('fold_kernel_ms', twins[0]), ('stepped_kernel_ms', twins[1])):
        line[name] = {i: [cnt, round(ms, 4)] for i in range(9) for cnt, ms in (e.timing_read(i),) if cnt}
    line['info'] = fold_info(twins[0])
    line['resets'] = [e.n_resets_used for e in twins]
    emit(line)
    for e in twins:
        e.close()

    # ---- end to end: the estimator's two fold-in routes
    if not a.no_end_to_end:
        est = si.NMF_RS_Estimator(n, d, k, random_state=0, T=T, nmf_kwargs={'device_init': True})
        est.min_rating, est.max_rating = 1.0, 5.0
        line = dict(base, what='end_to_end', corpus_ms=[], host_ms=[], download_ms=[])
        reps = a.reps if new.nnz <= 10000000 else 2
        for r in range(reps + 1):
            Wc, t_cor = clock(lambda: est.transform_corpus(new))
            A, t_down = clock(new.to_scipy)
            Wh, t_host = clock(lambda: est.transform(A))
            if r:
                line['corpus_ms'].append(t_cor)
                line['host_ms'].append(t_host)
                line['download_ms'].append(t_down)
        rows = np.repeat(np.arange(n), np.diff(A.indptr))
        pick = np.arange(0, A.nnz, max(1, A.nnz // 2000000))          # (at most ~2e6 of the entries: the products are nnz x k)
        pc = np.einsum('ij,ji->i', Wc[rows[pick]], T[:, A.indices[pick]])
        ph = np.einsum('ij,ji->i', Wh[rows[pick]], T[:, A.indices[pick]])
        line['rel_diff'] = float(np.linalg.norm(pc - ph) / np.linalg.norm(ph))
        for key in ('corpus_ms', 'host_ms', 'download_ms'):
            line[key + '_median'] = float(np.median(line[key]))
        emit(line)
    new.close()


if __name__ == '__main__':
    main()
