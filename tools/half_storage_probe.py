"""Float16 storage of a read-only dense X: the fused pass (k_pass) and the sweep of an RRI_F16 handle against the fp32 handle of
the same build, in ONE process, on the SAME values.

    python tools/half_storage_probe.py [--out FILE] [--one f16|f32] [--reps R] [--sweeps S]

X is made on the device (seeded): small integers, a planted rank-4 pattern of counts plus 0/1 noise, at most 15 -- every value is
exact in float16, so both stores hold the same matrix.  At 100000 x 10000 and at 20000 x 5000 (k = 50, plain flavour) an fp32 and
a float16 handle are made alternately, three times each; after 2 warm-up sweeps 20 sweeps are timed with the handle's HIP-event
timing.  One JSON line per handle: ms_per_pass (kernel id 0), sweeps_per_s, bytes per pass = n * LD * element size, TB/s and its
fraction of 8 TB/s; then one summary line per shape with the medians and ms_per_pass(f16) / ms_per_pass(f32).  The byte ratio is
0.5.  --one: a single handle of that store at the large shape (for `rocprofv3 --kernel-trace --stats -- python ... --one f16`)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rri_nmf_amd.engine import RRIEngine  # noqa: E402

HBM = 8.0e12
STORES = {'f32': np.float32, 'f16': np.float16}


def planted_counts(n, d, seed=0):
    """integer counts 0..15 on the device, as float32 (exact in float16 too)"""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    A = torch.randint(0, 4, (n, 4), generator=g, device='cuda').float()
    B = torch.randint(0, 2, (4, d), generator=g, device='cuda').float()
    X = A @ B                                                  # 0 .. 12
    X += torch.randint(0, 2, (n, d), generator=g, device='cuda').float()
    return X.clamp_(0, 15).contiguous()


def measure(X, store, k, sweeps, warm=2):
    import torch
    n, d = X.shape
    rs = np.random.RandomState(1)
    W0, T0 = rs.rand(n, k) / k, rs.rand(k, d)
    with RRIEngine(n, d, k, dtype=STORES[store]) as e:
        e.bind_X_device(X.data_ptr(), X.stride(0))
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
    es = np.dtype(STORES[store]).itemsize
    ld = X.stride(0)
    per_pass = ms / max(launches, 1)
    nbytes = n * ld * es
    return {'store': store, 'n': n, 'd': d, 'k': k, 'rpb': info['rpb'], 'nrb': info['nrb'], 'npanels': info['npanels'],
            'pass_launches': int(launches), 'ms_per_pass': per_pass, 'sweeps_per_s': sweeps / dt, 'bytes_per_pass': nbytes,
            'TB_per_s': nbytes / (per_pass * 1e-3) / 1e12, 'frac_8TBs': nbytes / (per_pass * 1e-3) / HBM, 'objective': obj}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', choices=sorted(STORES), default=None)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--sweeps', type=int, default=20)
    args = ap.parse_args()
    sink = open(args.out, 'a') if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()

    k = 50
    shapes = [(100000, 10000)] if args.one else [(100000, 10000), (20000, 5000)]
    for n, d in shapes:
        X32 = planted_counts(n, d)
        X = {'f32': X32, 'f16': X32.half()}
        assert bool((X['f16'].float() == X32).all()), 'the probe matrix must be exact in float16'
        rows = []
        for rep in range(1 if args.one else args.reps):
            for store in ([args.one] if args.one else ['f32', 'f16']):
                r = measure(X[store], store, k, args.sweeps)
                r['rep'] = rep
                rows.append(r)
                emit(r)
        if not args.one:
            med = {s: float(np.median([r['ms_per_pass'] for r in rows if r['store'] == s])) for s in STORES}
            sps = {s: float(np.median([r['sweeps_per_s'] for r in rows if r['store'] == s])) for s in STORES}
            emit({'summary': '%dx%d k=%d' % (n, d, k), 'median_ms_per_pass': med, 'median_sweeps_per_s': sps,
                  'pass_time_ratio_f16_over_f32': med['f16'] / med['f32'], 'byte_ratio': 0.5})
        del X, X32


if __name__ == '__main__':
    main()
