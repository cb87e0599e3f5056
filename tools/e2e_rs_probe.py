"""End-to-end wall time of NMF_RS_Estimator.fit at C5 scale (index pairs + ratings in, factors out), by phase.

    python tools/e2e_rs_probe.py [max_iter] [products]

`products` hides RRIEngine.sparse_range_finder: the NNDSVD start then takes its 16 products one by one, every panel through the
host, as it did before that call existed (the other side of the comparison, same process set-up)."""
import cProfile, pstats, sys, time
import numpy as np
sys.path.insert(0, '.')
from rri_nmf_amd import sklearn_interface as si
if 'products' in sys.argv[2:]:
    from rri_nmf_amd.engine import RRIEngine
    del RRIEngine.sparse_range_finder
n, d, k = 100000, 10000, 50
rs = np.random.RandomState(0)
m = 50000000
ij = np.column_stack((rs.randint(0, n, m), rs.randint(0, d, m)))
y = rs.randint(1, 6, m).astype(np.float64)
est = si.NMF_RS_Estimator(n, d, k, random_state=0, max_iter=int(sys.argv[1]) if len(sys.argv) > 1 else 10)
pr = cProfile.Profile()
t0 = time.perf_counter()
pr.enable()
est.fit(ij, y)
pr.disable()
print('fit wall %.2f s, sweeps run %d' % (time.perf_counter() - t0, len(est.nmf_outputs['iter_cputime'])))
pstats.Stats(pr).sort_stats('cumtime').print_stats(26)
