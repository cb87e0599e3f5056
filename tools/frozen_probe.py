"""Frozen rows at the flagship shape: what rri_frozen_absorb costs, what the statistics add to a T-row step, and an epoch of
batches against full-batch sweeps, in one process on one box.

    python tools/frozen_probe.py [--n 100000 --d 10000 --k 50 --batches 4 --sweeps 3 --out FILE]

A planted fp32 X (rri_nmf_amd.synthetic.planted_X, the benchmark's), plain flavour.  JSON lines.

what = 'absorb':
  absorb_ms     the launches of one rri_frozen_absorb by HIP events (rri_timing_read id 8): the panel W^T X in one pass over X on the
                float64 matrix cores with the sum of its row-block partials, then W^T W with 1^T W; three calls after a warm-up
  pass_ms       the read-only X pass of a sweep in the same process (id 0, the mean of its launches in two sweeps)
  k_passes_ms   k * pass_ms: what the panel costs through the existing pass, one topic at a time
  floor_ms      one read of X at the pass's measured rate = pass_ms (the pass reads X once); mfma_ms the float64 MFMA arithmetic
                of the panel, 2 n d (16 ceil(k / 16)) flop at 78.6 Tflop/s
what = 'trow': the T-row chain (id 2) per topic step in two sweeps without and with statistics (k_frozen_add sits inside it)
what = 'epoch': `batches` handles of n / batches rows, each swept `sweeps` times with the rows before it frozen and then absorbed
  (device_ms: sweeps and absorb; wall_ms: with the handle, the upload and the read-back of T), against `sweeps` sweeps of the
  handle that holds all rows; the objective on all rows of both T after a fold-in of 2 sweeps with T fixed
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_F64_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--batches', type=int, default=4)
    ap.add_argument('--sweeps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from rri_nmf_amd.engine import RRIEngine
    from rri_nmf_amd.synthetic import planted_X, scaled_init
    n, d, k = a.n, a.d, a.k
    X = planted_X(n, d, k, seed=0, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=1)
    W0, T0 = W0.astype(np.float64), T0.astype(np.float64)
    lines = []

    def say(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def fold_in_objective(eng, T):
        eng.clear_frozen()
        eng.set_W(W0)
        eng.set_T(T)
        eng.set_params(fix_T=True, reset_topic_method=None)
        eng.sweep(2)
        obj = eng.objective()
        eng.set_params()
        return obj

    with RRIEngine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X)
        e.set_W(W0), e.set_T(T0)
        e.set_params()
        e.sweep(1)                                   # warm-up: code objects, the packed copy of X, the rotation
        e.timing_enable(True)
        for kid in (0, 2, 8):
            e.timing_read(kid)
        e.sweep(2)
        p_launches, p_ms = e.timing_read(0)
        t_launches, t_ms = e.timing_read(2)
        pass_ms = p_ms / max(p_launches, 1)
        e.absorb(1.0)                                # warm-up
        e.timing_read(8)
        walls = []
        for _ in range(3):
            e.clear_frozen()
            t0 = time.perf_counter()
            e.absorb(1.0)
            walls.append(time.perf_counter() - t0)
        a_launches, a_ms = e.timing_read(8)
        say(what='absorb', n=n, d=d, k=k, absorb_ms=round(a_ms / 3, 3), brackets_per_call=a_launches // 3,
            wall_ms=[round(1e3 * w, 2) for w in walls], pass_ms=round(pass_ms, 4), pass_launches=p_launches,
            k_passes_ms=round(k * pass_ms, 2), ratio_k_passes_over_absorb=round(k * pass_ms / (a_ms / 3), 2), floor_ms=round(pass_ms, 4),
            mfma_ms=round(2.0 * n * d * 16 * -(-k // 16) / (MFMA_F64_TFLOPS * 1e9), 3), x_gb=round(X.nbytes / 1e9, 2))
        # the T-row chain with the statistics set (those just absorbed)
        e.timing_read(2)
        e.sweep(2)
        f_launches, f_ms = e.timing_read(2)
        say(what='trow', n=n, d=d, k=k, chain_us_plain=round(1e3 * t_ms / max(t_launches, 1), 2), launches_plain=t_launches,
            chain_us_frozen=round(1e3 * f_ms / max(f_launches, 1), 2), launches_frozen=f_launches)
        e.timing_enable(False)
        # full batch: `sweeps` sweeps from the start
        e.clear_frozen()
        e.set_W(W0), e.set_T(T0)
        e.synchronize()
        t0 = time.perf_counter()
        e.sweep(a.sweeps)
        e.synchronize()
        full_ms = 1e3 * (time.perf_counter() - t0)
        T_full = e.get_T()
        obj_start = fold_in_objective(e, T0)
        obj_full = fold_in_objective(e, T_full)
        # an epoch of batches
        nb = n // a.batches
        T, F = T0, None
        device_ms, wall_ms = 0.0, 0.0
        for b in range(a.batches):
            lo = b * nb
            t0 = time.perf_counter()
            with RRIEngine(nb, d, k, dtype=np.float32) as eb:
                eb.upload_X(X[lo:lo + nb])
                eb.set_W(W0[lo:lo + nb]), eb.set_T(T)
                eb.set_params()
                if F is not None:
                    eb.set_frozen(F)
                eb.synchronize()
                t1 = time.perf_counter()
                eb.sweep(a.sweeps)
                eb.absorb(1.0)
                eb.synchronize()
                device_ms += 1e3 * (time.perf_counter() - t1)
                T = eb.get_T()
                F = eb.get_frozen()                  # its row count: the rows set plus the rows absorbed
            wall_ms += 1e3 * (time.perf_counter() - t0)
        obj_epoch = fold_in_objective(e, T)
        say(what='epoch', n=n, d=d, k=k, batches=a.batches, sweeps=a.sweeps, epoch_device_ms=round(device_ms, 1),
            epoch_wall_ms=round(wall_ms, 1), full_ms=round(full_ms, 1), objective_start=obj_start, objective_full=obj_full,
            objective_epoch=obj_epoch, frozen_rows=F.rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(json.dumps(ln) for ln in lines) + '\n')


if __name__ == '__main__':
    main()
