"""End-to-end wall time of NMF_TM_Estimator(handle_tfidf, handle_normalization).fit on raw term counts at 100000 x 10000, k = 50,
30 sweeps, in the manner of tools/e2e_tfidf_probe.py: uint8 count storage (tf-idf and normalisation are the handle's two scale
vectors) against float32 storage (preprocessing on the device, X rewritten in place) and float16 storage (preprocessing in
float64 on the host, X rounded once at upload), in one job on the same counts.

    python tools/e2e_count_tfidf_probe.py [--out FILE] [--n N --d D --k K --sweeps S]

The counts are drawn on the device (Poisson, about 3 per entry on average, capped at 255) and handed to the estimator as a host
array, float32 for the floating stores and uint8 for the count store.  One JSON line per store."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rri_nmf_amd import sklearn_interface as si  # noqa: E402


def make_counts(n, d, k, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    out = np.empty((n, d), dtype=np.uint8)
    B = torch.rand(k, d, generator=g, device='cuda') ** 4
    step = 10000
    for lo in range(0, n, step):
        A = torch.rand(min(step, n - lo), k, generator=g, device='cuda') ** 4
        lam = A @ B
        lam *= 3.0 / lam.mean()
        blk = torch.poisson(lam, generator=g).clamp_(0, 255)
        blk[:, 0] += (blk.sum(1) == 0).float()            # no empty document
        out[lo:lo + blk.shape[0]] = blk.to(torch.uint8).cpu().numpy()
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--d', type=int, default=10000)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--sweeps', type=int, default=30)
    args = ap.parse_args()
    n, d, k = args.n, args.d, args.k
    C8 = make_counts(n, d, k)
    print('counts: %.1f %% non-zero, max %d' % (100.0 * np.count_nonzero(C8) / C8.size, C8.max()), flush=True)
    sink = open(args.out, 'a') if args.out else None
    for name, dt in (('uint8', np.uint8), ('float32', np.float32), ('float16', np.float16)):
        X = C8 if dt == np.uint8 else C8.astype(np.float32)
        est = si.NMF_TM_Estimator(n, d, k, random_state=0, max_iter=args.sweeps, handle_tfidf=True, handle_normalization=True,
                                  nmf_kwargs={'dtype': dt})
        t0 = time.perf_counter()
        est.fit(X)
        t1 = time.perf_counter()
        W = est.transform(X[:5000])
        t2 = time.perf_counter()
        oh = est.nmf_outputs['obj_history']
        rec = {'storage': name, 'n': n, 'd': d, 'k': k, 'fit_s': t1 - t0, 'sweeps': len(oh), 'objective_first': oh[0],
               'objective_last': oh[-1], 'transform_5000_s': t2 - t1, 'idf_min': float(est.idf.min()), 'idf_max': float(est.idf.max()),
               'x_storage_relerr': est.nmf_outputs.get('x_storage_relerr')}
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + '\n')
            sink.flush()
        assert np.all(np.diff(oh) <= 1e-12 * abs(oh[0])) and abs(W.sum(1) - 1).max() < 1e-9
        del est, X


if __name__ == '__main__':
    main()
