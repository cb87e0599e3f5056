#!/usr/bin/env python3
"""The read-only pass over the packed copy of X: builds of librri_hip.so and geometries of the pass against each other
INSIDE one process.  An entry is a library and a value of RRI_PASS_PK_GEOM (rows per workgroup, i = interleaved / c = contiguous
chunks; empty = the handle's default); engines are made alternately, one per entry, on the same resident X, and every entry is
visited --rounds times, so the spread of equal settings is in the log.

    python tools/pk_geom_probe.py [--entries NAME=LIB[@GEOM],...] [--shapes c3,mid] [--rounds 3] [--sweeps 5] [--out FILE]

LIB: a path, or `.` for the library of this tree.  GEOM may end in `:nocopy`: the handle is made under RRI_X_PACK=0 and streams
the fp32 X (what a handle does whose copy was released or could not be allocated).  Examples:
    --entries parent=/tmp/parent.so,new=.                      two builds, the default geometry
    --entries d=.,r448c=.@448c,r448i=.@448i,r512c=.@512c       one build, four geometries
    --entries f560=.@560c:nocopy,f512=.@512c:nocopy            the fp32 stream at two geometries
Per engine, after one warm sweep (which builds the copy): sweeps/s by the wall clock over --sweeps sweeps without event timing, then
ms per pass (timer 0), per W column (1) and per T-row chain (2) by HIP events on every 4th launch, and a checksum of W's bits
(equal for equal geometries: the copy and its decode keep every bit).  Then per shape and entry the median and the range, and the
largest spread of one entry, against which a difference counts.
Shapes: c3 = 100000 x 10000 fp32 k = 50 (bench.py's default), mid = 20000 x 5000 fp32 k = 20 (bench.py --config mid), tall =
600000 x 1024 fp32 k = 20 (2.4 GB in one column group: the LDS cap decides its rows per workgroup as it does at c3)."""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import device_planted_shard          # noqa: E402
from rri_nmf_amd import _capi                   # noqa: E402
from rri_nmf_amd.engine import RRIEngine        # noqa: E402

SHAPES = {'c3': (100000, 10000, 50), 'mid': (20000, 5000, 20), 'tall': (600000, 1024, 20)}
ENV = 'RRI_PASS_PK_GEOM'


def one_engine(lib, geom, X, n, d, k, W0, T0, sweeps):
    _capi._lib = lib
    geom, _, nocopy = geom.partition(':')
    if geom:
        os.environ[ENV] = geom
    if nocopy:
        os.environ['RRI_X_PACK'] = '0'
    try:
        eng = RRIEngine(n, d, k, dtype=np.float32, device=0)
    finally:
        os.environ.pop(ENV, None)
        os.environ.pop('RRI_X_PACK', None)
    eng.bind_X_device(X.data_ptr(), X.stride(0))
    eng.set_W(W0), eng.set_T(T0)
    eng.set_params()
    eng.sweep(1)
    eng.synchronize()
    info = eng.layout_info()
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
    crc = zlib.crc32(np.ascontiguousarray(eng.get_W()).tobytes())
    eng.close()
    return dict(pass_ms=ms[0], wcol_ms=ms[1], trow_ms=ms[2], sweeps_per_s=sweeps / dt, rpb=info['rpb'], nrb=info['nrb'],
                interleaved=int(info['interleaved']), x_pack=int(info['x_pack']), keep_q=info.get('keep_q', None), w_crc=crc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--entries', default='default=.')
    ap.add_argument('--shapes', default='c3,mid')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--sweeps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    entries, libs = [], {}
    for item in args.entries.split(','):
        name, spec = item.split('=', 1)
        path, _, geom = spec.partition('@')
        path = None if path == '.' else os.path.abspath(path)
        if path not in libs:
            libs[path] = _capi.load_library(path)
        entries.append((name, libs[path], geom))
    sink = open(args.out, 'a') if args.out else None

    def emit(line):
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()

    dev = torch.device('cuda', 0)
    for shape in args.shapes.split(','):
        n, d, k = SHAPES[shape]
        X = device_planted_shard(n, d, k, 0, dev)
        a = (float(X[:20000].mean()) / k) ** 0.5
        rng = np.random.RandomState(0)
        W0, T0 = a * rng.rand(n, k), a * rng.rand(k, d)
        torch.cuda.synchronize()
        rows = {name: [] for name, _, _ in entries}
        for rnd in range(args.rounds):
            for name, lib, geom in entries:
                r = one_engine(lib, geom, X, n, d, k, W0, T0, args.sweeps)
                rows[name].append(r)
                emit(json.dumps(dict(shape=shape, round=rnd, entry=name, geom=geom,
                                     **{kk: (round(v, 5) if isinstance(v, float) else v) for kk, v in r.items()})))
        emit('%s: %d x %d fp32 k = %d; median [min .. max] over %d visits' % (shape, n, d, k, args.rounds))
        emit('  %-10s %-14s %-26s %-26s %-26s %-26s %s' % ('entry', 'rows (blocks)', 'pass ms', 'W column ms', 'T-row chain ms', 'sweeps/s', 'W crc'))
        for name, _, _ in entries:
            cells = []
            for key in ('pass_ms', 'wcol_ms', 'trow_ms', 'sweeps_per_s'):
                v = [r[key] for r in rows[name]]
                cells.append('%.4f [%.4f .. %.4f]' % (float(np.median(v)), min(v), max(v)))
            r0 = rows[name][0]
            crcs = sorted({'%08x' % r['w_crc'] for r in rows[name]})
            emit('  %-10s %-14s %-26s %-26s %-26s %-26s %s%s' % (name, '%d%s (%d)' % (r0['rpb'], 'i' if r0['interleaved'] else 'c', r0['nrb']), *cells,
                                                               ','.join(crcs), '' if r0['x_pack'] else '  fp32 stream'))
        spread = {key: max(max(r[key] for r in rows[nm]) - min(r[key] for r in rows[nm]) for nm in rows) for key in ('pass_ms', 'sweeps_per_s')}
        emit('  largest spread of one entry: pass %.4f ms, %.4f sweeps/s' % (spread['pass_ms'], spread['sweeps_per_s']))
        del X
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
