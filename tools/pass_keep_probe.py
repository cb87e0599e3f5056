#!/usr/bin/env python3
"""How much of the Infinity Cache may a topic step fill?  RRI_PASS_CACHE_MB = C gives the read-only pass a budget for X of
C minus the chain's own default-policy traffic (pass_keep, rri_hip.hip): an X inside it is read with plain loads, of a larger one
that many bytes (whole row blocks, the same in every pass) are, the rest streams non-temporally.  C = 0 streams all of X.

    python tools/pass_keep_probe.py [--shapes c3,c3h,mid,b180] [--caps 0,128,160,192,224,256] [--rounds 3] [--sweeps 5] [--out FILE]

The switch is read by rri_create, so engines are made alternately, one per capacity, in ONE process on the same resident X; every
capacity is visited --rounds times, so the spread of equal settings is in the log.  Per engine, after one warm sweep: ms per pass
(timer 0), per W column (1), per T-row chain (2), all by HIP events on every 4th launch, and sweeps/s by the wall clock over
--sweeps sweeps without event timing.  Then per shape and capacity the median and the range, and the capacity-0 spread against
which a difference counts (three times it).  The default is chosen on sweeps/s: a capacity that speeds the pass up by pushing W
out of the cache slows k_wcol down.
Shapes: c3 = 100000 x 10000 fp32 k = 50 (bench.py's default), c3h = the same in float16, mid = 20000 x 5000 fp32 k = 20
(bench.py --config mid), b180 = 18000 x 2500 fp32 k = 50 (180 MB: plain loads throughout before this switch existed)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import device_planted_shard          # noqa: E402
from rri_nmf_amd.engine import RRIEngine        # noqa: E402

SHAPES = {'c3': (100000, 10000, 50, np.float32), 'c3h': (100000, 10000, 50, np.float16),
          'mid': (20000, 5000, 20, np.float32), 'b180': (18000, 2500, 50, np.float32)}


def chain_bytes(n, k, info, ld):
    """the default-policy traffic of a topic step beside X, as pass_keep counts it"""
    nwb = (n + 63) // 64
    return 8 * (k * n + 2 * info['nrb'] * ld + 2 * info['npanels'] * n + 2 * k * ld + 2 * nwb * (k + 2))


def one_engine(X, n, d, k, dtype, cap, W0, T0, sweeps):
    os.environ['RRI_PASS_CACHE_MB'] = repr(float(cap))
    try:
        eng = RRIEngine(n, d, k, dtype=dtype, device=0)
    finally:
        os.environ.pop('RRI_PASS_CACHE_MB', None)
    eng.bind_X_device(X.data_ptr(), X.stride(0))
    eng.set_W(W0), eng.set_T(T0)
    eng.set_params()
    info = eng.layout_info()
    eng.sweep(1)
    eng.synchronize()
    t0 = time.perf_counter()
    eng.sweep(sweeps)
    eng.synchronize()
    dt = time.perf_counter() - t0
    eng.timing_enable(True, every=4)
    eng.sweep(2)
    eng.synchronize()
    ms = []
    for timer in (0, 1, 2):
        cnt, tot = eng.timing_read(timer)
        ms.append(tot / max(cnt, 1))
    eng.timing_enable(False)
    eng.close()
    es = np.dtype(dtype).itemsize
    ld = -(-d // (16 // es)) * (16 // es)
    block = info['rpb'] * ld * es
    budget = cap * 1e6 - chain_bytes(n, k, info, ld)
    xbytes = n * ld * es
    keep = -1 if xbytes <= budget else max(0, min(info['nrb'], int(budget // block)))
    return dict(pass_ms=ms[0], wcol_ms=ms[1], trow_ms=ms[2], sweeps_per_s=sweeps / dt, keep_q=keep, nrb=info['nrb'],
                kept_mb=(xbytes if keep < 0 else keep * block) / 1e6, x_mb=xbytes / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c3,c3h,mid,b180')
    ap.add_argument('--caps', default='0,128,160,192,224,256')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--sweeps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    caps = [float(c) for c in args.caps.split(',')]
    sink = open(args.out, 'a') if args.out else None

    def emit(line):
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()

    dev = torch.device('cuda', 0)
    for shape in args.shapes.split(','):
        n, d, k, dtype = SHAPES[shape]
        X = device_planted_shard(n, d, k, 0, dev)
        a = (float(X[:20000].mean()) / k) ** 0.5
        if dtype == np.float16:
            X = X.half()
        rng = np.random.RandomState(0)
        W0, T0 = a * rng.rand(n, k), a * rng.rand(k, d)
        torch.cuda.synchronize()
        rows = {c: [] for c in caps}
        for rnd in range(args.rounds):
            for c in caps:
                r = one_engine(X, n, d, k, dtype, c, W0, T0, args.sweeps)
                rows[c].append(r)
                emit(json.dumps(dict(shape=shape, round=rnd, cache_mb=c, **{kk: (round(v, 5) if isinstance(v, float) else v) for kk, v in r.items()})))
        emit('%s: %d x %d %s k = %d, X %.0f MB; median [min .. max] over %d visits' % (shape, n, d, np.dtype(dtype).name, k, rows[caps[0]][0]['x_mb'], args.rounds))
        emit('  %8s %14s %-26s %-26s %-26s %-26s' % ('cache MB', 'kept MB (q)', 'pass ms', 'W column ms', 'T-row chain ms', 'sweeps/s'))
        for c in caps:
            cells = []
            for key in ('pass_ms', 'wcol_ms', 'trow_ms', 'sweeps_per_s'):
                v = [r[key] for r in rows[c]]
                cells.append('%.4f [%.4f .. %.4f]' % (float(np.median(v)), min(v), max(v)))
            r0 = rows[c][0]
            emit('  %8g %14s %-26s %-26s %-26s %-26s' % (c, '%.0f (%s)' % (r0['kept_mb'], 'all' if r0['keep_q'] < 0 else '%d/%d' % (r0['keep_q'], r0['nrb'])), *cells))
        spread = {key: max(max(r[key] for r in rows[c]) - min(r[key] for r in rows[c]) for c in caps) for key in ('pass_ms', 'sweeps_per_s')}
        emit('  largest spread of one setting: pass %.4f ms, %.4f sweeps/s (a difference counts from three times that)' % (spread['pass_ms'], spread['sweeps_per_s']))
        del X
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
