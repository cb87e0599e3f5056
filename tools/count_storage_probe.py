"""uint8 count storage of a read-only dense X (RRI_U8): the fused pass (k_pass) and the sweep of a uint8 handle against the
float16 and the fp32 handle of the same build, in ONE process, on the SAME values.

    python tools/count_storage_probe.py [--out FILE] [--one f32|f16|u8] [--reps R] [--sweeps S] [--lib NAME=PATH ...]

X is made on the device (seeded): small integers, a planted rank-4 pattern of counts plus 0/1 noise, at most 15 -- every value is
exact in float16 and in a byte, so all three stores hold the same matrix (the uint8 handle with both scale vectors at one).  At
100000 x 10000 and at 20000 x 5000 (k = 50, plain flavour) an fp32, a float16 and a uint8 handle are made alternately, three
times each; after 2 warm-up sweeps 20 sweeps are timed with the handle's HIP-event timing.  One JSON line per handle:
ms_per_pass (kernel id 0), sweeps_per_s, bytes per pass = n * LD * element size, TB/s and its fraction of 8 TB/s; then one summary
line per shape with the medians, ms_per_pass(u8) / ms_per_pass(f16) (the yardstick: byte ratio 0.5) and u8 / f32 (0.25).
--one: a single handle of that store at the large shape (for `rocprofv3 --kernel-trace --stats -- python ... --one u8`).
--lib NAME=PATH (repeatable): the uint8 handle once more on another build of librri_hip.so, as store `u8:NAME`, alternated with
the others in the same process -- how two builds of the pass are compared."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rri_nmf_amd import _capi  # noqa: E402
from rri_nmf_amd.engine import RRIEngine  # noqa: E402

HBM = 8.0e12
STORES = {'f32': np.float32, 'f16': np.float16, 'u8': np.uint8}


def planted_counts(n, d, seed=0):
    """integer counts 0..15 on the device, as float32 (exact in float16 and as bytes)"""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    A = torch.randint(0, 4, (n, 4), generator=g, device='cuda').float()
    B = torch.randint(0, 2, (4, d), generator=g, device='cuda').float()
    X = A @ B                                                  # 0 .. 12
    X += torch.randint(0, 2, (n, d), generator=g, device='cuda').float()
    return X.clamp_(0, 15).contiguous()


def measure(X, store, k, sweeps, warm=2, lib=None):
    import torch
    n, d = X.shape
    rs = np.random.RandomState(1)
    W0, T0 = rs.rand(n, k) / k, rs.rand(k, d)
    default = _capi.load_library()
    if lib is not None:
        _capi._lib = lib                # the engine made below binds to this build
    try:
        e = RRIEngine(n, d, k, dtype=STORES[store.split(':')[0]])
    finally:
        _capi._lib = default
    with e:
        try:
            e.bind_X_device(X.data_ptr(), X.stride(0))
            ld = X.stride(0)
        except ValueError:                  # d is no multiple of this build's load width: the handle's own padded copy
            e.upload_X(X.cpu().numpy())
            ld = -(-d // 8) * 8
        e.set_W(W0)
        e.set_T(T0)
        e.set_params(reset_topic_method=None)
        info = e.layout_info()
        e.sweep(warm)
        e.synchronize()
        e.timing_enable(True)
        t0 = time.perf_counter()
        e.sweep(sweeps)
        e.synchronize()
        dt = time.perf_counter() - t0
        launches, ms = e.timing_read(0)
        e.timing_enable(False)
        obj = e.objective()
    torch.cuda.synchronize()
    es = X.element_size()
    per_pass = ms / max(launches, 1)
    nbytes = n * ld * es
    return {'store': store, 'n': n, 'd': d, 'k': k, 'rpb': info['rpb'], 'nrb': info['nrb'], 'npanels': info['npanels'],
            'pass_launches': int(launches), 'ms_per_pass': per_pass, 'sweeps_per_s': sweeps / dt, 'bytes_per_pass': nbytes,
            'TB_per_s': nbytes / (per_pass * 1e-3) / 1e12, 'frac_8TBs': nbytes / (per_pass * 1e-3) / HBM, 'objective': obj}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', choices=sorted(STORES), default=None)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sweeps', type=int, default=20)
    ap.add_argument('--lib', action='append', default=[], metavar='NAME=PATH')
    ap.add_argument('--shapes', default=None, help='n,d[;n,d...] instead of the two standard shapes')
    args = ap.parse_args()
    sink = open(args.out, 'a') if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()

    libs = {}
    for spec in args.lib:
        name, path = spec.split('=', 1)
        libs['u8:' + name] = _capi.load_library(os.path.abspath(path))
    k = 50
    shapes = [(100000, 10000)] if args.one else [(100000, 10000), (20000, 5000)]
    if args.shapes:
        shapes = [tuple(int(v) for v in s.split(',')) for s in args.shapes.split(';')]
    for n, d in shapes:
        X32 = planted_counts(n, d)
        X = {'f32': X32, 'f16': X32.half(), 'u8': X32.to(torch.uint8)}
        assert bool((X['f16'].float() == X32).all()) and bool((X['u8'].float() == X32).all()), \
            'the probe matrix must be exact in float16 and as bytes'
        order = [args.one] if args.one else ['f32', 'f16', 'u8'] + sorted(libs)
        rows = []
        for rep in range(1 if args.one else args.reps):
            for store in order:
                r = measure(X[store.split(':')[0]], store, k, args.sweeps, lib=libs.get(store))
                r['rep'] = rep
                rows.append(r)
                emit(r)
        if not args.one:
            med = {s: float(np.median([r['ms_per_pass'] for r in rows if r['store'] == s])) for s in order}
            sps = {s: float(np.median([r['sweeps_per_s'] for r in rows if r['store'] == s])) for s in order}
            objs = {s: [r['objective'] for r in rows if r['store'] == s][0] for s in order}
            rec = {'summary': '%dx%d k=%d' % (n, d, k), 'median_ms_per_pass': med, 'median_sweeps_per_s': sps, 'objective': objs,
                   'byte_ratio_u8_over_f16': 0.5, 'byte_ratio_u8_over_f32': 0.25}
            for s in order:
                if s.startswith('u8'):
                    rec['pass_time_ratio_%s_over_f16' % s] = med[s] / med['f16']
                    rec['pass_time_ratio_%s_over_f32' % s] = med[s] / med['f32']
            emit(rec)
        del X, X32


if __name__ == '__main__':
    main()
