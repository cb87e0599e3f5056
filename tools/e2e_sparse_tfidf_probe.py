"""End-to-end wall time of the topic-model estimator on raw CSR term counts kept sparse on the device: where the time of
NMF_TM_Estimator(handle_tfidf=True, handle_normalization=True, nmf_kwargs={'sparse_X': True}).fit(X_csr) goes, and what
keep_resident=True saves per one_iter(X_csr) call.

    python tools/e2e_sparse_tfidf_probe.py [--density 0.002 0.01 0.05] [--reps 5] [--calls 20] [--label NAME] [--out FILE.jsonl]
                                           [--tree DIR] [--routes default products] [--empty-rows 0.001] [--uniform-rows both]

100000 x 10000 Zipf counts (tools/sparse_x_probe.zipf_counts), k = 50, fp32 storage, 30 sweeps per fit.  One JSON line per
density: medians over --reps fits of the wall time and of its parts --
    host_prep   matrixops on the host (nmf._preprocess_on_host)          upload    rri_upload_X_csr incl. the store build
    device_prep RRIEngine.preprocess                                     start     the starting W, T (NNDSVD)
    sweeps      rri_sweep / rri_sweep_until / rri_objective              other     the rest of the call
-- and the median of --calls one_iter calls with and without keep_resident, in the same process (--calls 0: fits only).
The start is also given alone (`start_s`: every fit's value, median, min, max) with the range finder of its randomized SVD as a
line of its own (`range_finder_s`: RRIEngine.sparse_range_finder, or the 16 products X_times / Xt_times where the start takes
them one by one; host LU / QR between them is not in it).  --routes default products fits each density under both starts in
turn, rep by rep (one line per route): `products` hides sparse_range_finder from the engine, which is the start as it was before
that call existed -- the two sides of the comparison on one device in one process.
--tree DIR imports rri_nmf_amd from another checkout (built there), to put two commits side by side on one device; --label
names the line.
--empty-rows F empties that share of the documents (seeded), as vocabulary pruning does: normalisation makes each the dense row
1/d, which sends the call to the host route -- unless nmf_kwargs carries uniform_rows=True (--uniform-rows on).  --uniform-rows
both fits and calls one_iter without and with the option in turn, rep by rep (one line per setting, `uniform_rows` says which;
without the option the calls are those of the commits before it), and the line with the option also carries the handle's own
timing of one sampled sweep: the X pass (`pass_us`, which brackets both launches) and the launch that adds the uniform rows'
share after it (`uniform_us`), per topic-step launch."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from sparse_x_probe import zipf_counts  # noqa: E402  (imports the package of THIS checkout for its own measurements only)

PARTS = ('host_prep', 'upload', 'device_prep', 'start', 'sweeps')


def load_package(tree):
    for name in [m for m in sys.modules if m == 'rri_nmf_amd' or m.startswith('rri_nmf_amd.')]:
        del sys.modules[name]
    sys.path.insert(0, os.path.abspath(tree))
    from rri_nmf_amd import engine, nmf, sklearn_interface
    assert os.path.abspath(os.path.dirname(os.path.dirname(nmf.__file__))) == os.path.abspath(tree)
    return engine, nmf, sklearn_interface


class Clock(object):
    """sums the wall time spent inside the wrapped functions, per part; nested parts count for the outer one only"""

    def __init__(self):
        self.t = dict.fromkeys(PARTS, 0.0)
        self.depth = 0

    def reset(self):
        self.t = dict.fromkeys(PARTS, 0.0)

    def wrap(self, fn, part):
        def timed(*a, **kw):
            if self.depth:
                return fn(*a, **kw)
            self.depth += 1
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                self.t[part] += time.perf_counter() - t0
                self.depth -= 1
        return timed


def instrument(engine, nmf, clock):
    E = engine.RRIEngine
    nmf._preprocess_on_host = clock.wrap(nmf._preprocess_on_host, 'host_prep')
    nmf._initialize_and_validate = clock.wrap(nmf._initialize_and_validate, 'start')
    E.upload_X_csr = clock.wrap(E.upload_X_csr, 'upload')
    E.preprocess = clock.wrap(E.preprocess, 'device_prep')
    for name in ('sweep', 'sweep_until', 'objective'):
        setattr(E, name, clock.wrap(getattr(E, name), 'sweeps'))


class Inner(object):
    """wall time inside the range finder of the start (counted within 'start', not beside it)"""

    def __init__(self, E):
        self.t, self.depth = 0.0, 0
        for name in ('sparse_range_finder', 'X_times', 'Xt_times'):
            if hasattr(E, name):
                setattr(E, name, self.wrap(getattr(E, name)))
        self.E, self.method = E, getattr(E, 'sparse_range_finder', None)

    def wrap(self, fn):
        def timed(*a, **kw):
            if self.depth:                      # X_times calls itself chunk by chunk beyond 64 columns
                return fn(*a, **kw)
            self.depth += 1
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                self.t += time.perf_counter() - t0
                self.depth -= 1
        return timed

    def route(self, name):
        if self.method is None:
            return
        if name == 'products' and hasattr(self.E, 'sparse_range_finder'):
            del self.E.sparse_range_finder
        elif name == 'default':
            self.E.sparse_range_finder = self.method


def spread(v):
    return {'median': median(v), 'min': float(min(v)), 'max': float(max(v)), 'all': [float(x) for x in v]}


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def fit_record(r):
    walls, parts = r['walls'], r['parts']
    split = {p: median([q[p] for q in parts]) for p in PARTS}
    split['other'] = median([w - sum(q.values()) for w, q in zip(walls, parts)])
    return {'wall_s_median': median(walls), 'wall_s': walls, 'split_s_median': split, 'sweeps': r['sweeps'],
            'start_s': spread([q['start'] for q in parts]), 'range_finder_s': spread(r['rf']),
            'route': 'host' if split['host_prep'] > 0 else 'device'}


def emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--density', type=float, nargs='+', default=[0.002, 0.01, 0.05])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--label', default='this checkout')
    ap.add_argument('--out', default=None)
    ap.add_argument('--tree', default=os.path.dirname(HERE))
    ap.add_argument('--routes', nargs='+', default=['default'], choices=['default', 'products'])
    ap.add_argument('--empty-rows', type=float, default=0.0)
    ap.add_argument('--uniform-rows', default='off', choices=['off', 'on', 'both'])
    args = ap.parse_args()
    if args.uniform_rows != 'off':
        return main_uniform(args)
    engine, nmf, si = load_package(args.tree)
    clock = Clock()
    instrument(engine, nmf, clock)
    inner = Inner(engine.RRIEngine)
    n, d, k = 100000, 10000, 50
    kw = dict(handle_tfidf=True, handle_normalization=True, random_state=0,
              nmf_kwargs={'sparse_X': True, 'dtype': np.float32, 'eps_stop': -1})
    for dens in args.density:
        X = zipf_counts(n, d, dens, seed=int(dens * 1e4))
        rec = {'tool': 'e2e_sparse_tfidf_probe', 'label': args.label, 'shape': [n, d], 'k': k, 'density_asked': dens,
               'nnz': int(X.nnz), 'density': X.nnz / float(n * d), 'empty_rows': int(np.sum(np.diff(X.indptr) == 0))}
        for route in args.routes:                                                    # warm-up: library, allocator, sklearn
            inner.route(route)
            si.NMF_TM_Estimator(n, d, k, max_iter=2, **kw).fit(X)
        runs = {route: {'walls': [], 'parts': [], 'sweeps': [], 'rf': []} for route in args.routes}
        for _ in range(args.reps):
            for route in args.routes:                                                # the routes in turn, rep by rep
                inner.route(route)
                est = si.NMF_TM_Estimator(n, d, k, max_iter=30, **kw)
                clock.reset()
                inner.t = 0.0
                t0 = time.perf_counter()
                est.fit(X)
                r = runs[route]
                r['walls'].append(time.perf_counter() - t0)
                r['parts'].append(dict(clock.t))
                r['rf'].append(inner.t)
                r['sweeps'].append(len(est.nmf_outputs['iter_cputime']))
        base = dict(rec)
        for route in args.routes[1:]:
            emit(args, dict(base, route_of_start=route, fit=fit_record(runs[route])))
        inner.route(args.routes[0])
        rec['route_of_start'] = args.routes[0]
        rec['fit'] = fit_record(runs[args.routes[0]])
        for keep in ((True, False) if args.calls > 0 else ()):
            est = si.NMF_TM_Estimator(n, d, k, max_iter=2, keep_resident=keep, **kw).fit(X)
            calls = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                est.one_iter(X)
                calls.append(time.perf_counter() - t0)
            holder = getattr(est, '_resident', None)
            rec['one_iter_keep_resident' if keep else 'one_iter'] = {
                'ms_median': 1e3 * median(calls), 'ms_min': 1e3 * min(calls), 'ms_max': 1e3 * max(calls),
                'handle_reuses': int(holder.reuses) if holder is not None else 0}
            if keep:
                est.release()
        emit(args, rec)


def with_empty_rows(X, share, seed=7):
    """X with that share of its rows emptied (the pattern loses them: no stored zeros)"""
    if share <= 0:
        return X
    import scipy.sparse as sp
    n = X.shape[0]
    rows = np.random.RandomState(seed).choice(n, size=max(1, int(round(share * n))), replace=False)
    keep = np.ones(n)
    keep[rows] = 0.0
    Y = (sp.diags(keep) @ X).tocsr()
    Y.eliminate_zeros()
    Y.sort_indices()
    return Y


def pass_timing(engine, X, W, T):
    """one sampled sweep from the fitted W, T on a handle with the uniform rows of X: microseconds per launch of the X pass's
    bracket (timing id 0: k_spx_pass and, inside it, the uniform rows' launch) and of that launch alone (id 3)"""
    n, d = X.shape
    k = T.shape[0]
    with engine.RRIEngine(n, d, k, dtype=np.float32, sparse_x=True) as e:
        e.upload_X_csr(X.astype(np.float32))
        e.preprocess(tfidf=True, normalize=True, uniform_rows=True)
        e.set_W(W); e.set_T(T)
        e.set_params(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
        e.sweep(2)
        e.timing_enable(True)
        e.sweep(1)
        e.timing_enable(False)
        (n0, ms0), (n3, ms3) = e.timing_read(0), e.timing_read(3)
        return {'uniform_rows': int(e.uniform_rows()[0].size), 'pass_launches': n0, 'pass_us': 1e3 * ms0 / max(n0, 1),
                'uniform_launches': n3, 'uniform_us': 1e3 * ms3 / max(n3, 1)}


def main_uniform(args):
    """--uniform-rows on / both: the fits and the one_iter calls of main(), per setting of nmf_kwargs' uniform_rows"""
    engine, nmf, si = load_package(args.tree)
    clock = Clock()
    instrument(engine, nmf, clock)
    n, d, k = 100000, 10000, 50
    modes = {'on': [True], 'both': [False, True]}[args.uniform_rows]

    def kwargs(mode):
        extra = {'uniform_rows': True} if mode else {}
        return dict(handle_tfidf=True, handle_normalization=True, random_state=0,
                    nmf_kwargs=dict({'sparse_X': True, 'dtype': np.float32, 'eps_stop': -1}, **extra))
    for dens in args.density:
        X = with_empty_rows(zipf_counts(n, d, dens, seed=int(dens * 1e4)), args.empty_rows)
        base = {'tool': 'e2e_sparse_tfidf_probe', 'label': args.label, 'shape': [n, d], 'k': k, 'density_asked': dens,
                'nnz': int(X.nnz), 'density': X.nnz / float(n * d), 'empty_rows': int(np.sum(np.diff(X.indptr) == 0))}
        for mode in modes:
            si.NMF_TM_Estimator(n, d, k, max_iter=2, **kwargs(mode)).fit(X)          # warm-up
        runs = {mode: {'walls': [], 'parts': [], 'sweeps': [], 'rf': []} for mode in modes}
        for _ in range(args.reps):
            for mode in modes:                                                       # the settings in turn, rep by rep
                est = si.NMF_TM_Estimator(n, d, k, max_iter=30, **kwargs(mode))
                clock.reset()
                t0 = time.perf_counter()
                est.fit(X)
                r = runs[mode]
                r['walls'].append(time.perf_counter() - t0)
                r['parts'].append(dict(clock.t))
                r['rf'].append(0.0)
                r['sweeps'].append(len(est.nmf_outputs['iter_cputime']))
        ests = {mode: si.NMF_TM_Estimator(n, d, k, max_iter=2, keep_resident=True, **kwargs(mode)).fit(X) for mode in modes}
        calls = {mode: [] for mode in modes}
        for _ in range(args.calls):
            for mode in modes:
                t0 = time.perf_counter()
                ests[mode].one_iter(X)
                calls[mode].append(time.perf_counter() - t0)
        for mode in modes:
            rec = dict(base, uniform_rows=bool(mode), fit=fit_record(runs[mode]))
            holder = getattr(ests[mode], '_resident', None)
            if args.calls > 0:
                rec['one_iter_keep_resident'] = {'ms_median': 1e3 * median(calls[mode]), 'ms_min': 1e3 * min(calls[mode]),
                                                 'ms_max': 1e3 * max(calls[mode]),
                                                 'handle_reuses': int(holder.reuses) if holder is not None else 0}
            ests[mode].release()
            if mode:
                rec['timing'] = pass_timing(engine, X, np.asarray(ests[mode].W), np.asarray(ests[mode].T))
            emit(args, rec)


if __name__ == '__main__':
    main()
