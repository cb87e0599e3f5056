"""What a handle keeps between calls must not outlive the T it was computed from: Qt = X T^T and Gfull = T T^T, which a sweep
with T fixed computes once and reuses (k_xtt / k_gram, k_wsweep_rows or k_wcol per topic).

Two sequences on ONE handle in which T changes between two fixed-T sweeps by a route that once kept both:
  * a handle of the explicit-residual schedule whose free sweep steps T (enqueue_rT_half);
  * a reset applied with no run paused (rri_apply_reset_vectors).
rri_apply_reset_max_resid has no engine wrapper outside a paused run (RRIEngine reaches it only through a pending event), so it
has no case here.

Reference: the CPU oracle, chained call by call with W_in / T_in, eps_stop=-1, in float64.  Tolerance: relfro < 1e-9 on W and
on T of a float64 handle (summation order only, as tests/test_residual_gpu.py between two float64 runs).  A stale Qt cannot
hide under it: given the T of the first fixed call in place of the current one, the oracle's last call ends with a W that is
off by relfro 1.2e-1 in the first sequence and by 8.2e-1 in the second.
"""
import numpy as np
import pytest

from conftest import relfro
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu

N, D, K = 700, 333, 6
TOL = 1e-9


def problem():
    X = planted_X(N, D, K, seed=5, dtype=np.float64)      # as test_residual_gpu.py's resumability case
    W0, T0 = scaled_init(X, K, seed=6)
    return X, W0, T0


def oracle_chain(X, W, T, calls):
    """calls: (sweeps, flags) one after the other, each starting from the factors the one before left"""
    from oracle import rri_oracle
    for sweeps, flags in calls:
        out = rri_oracle.nmf(X, K, W_in=W.copy(), T_in=T.copy(), max_iter=sweeps, eps_stop=-1, **flags)
        W, T = out['W'], out['T']
    return W, T


def engine_chain(X, W0, T0, calls, schedule):
    from rri_nmf_amd.engine import RRIEngine
    with RRIEngine(N, D, K, dtype=np.float64, schedule=schedule) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0)
        for sweeps, flags in calls:
            e.set_params(**flags)
            e.sweep(sweeps)
        return e.get_W(), e.get_T()


@pytest.mark.parametrize('wsweep', [None, '0'])
def test_residual_handle_free_sweep_between_two_fixed_T_sweeps(monkeypatch, wsweep):
    """sweep(2) free, T fixed sweep(1), free sweep(1), T fixed sweep(1): the last call must use the T of the third"""
    if wsweep is None:
        monkeypatch.delenv('RRI_WSWEEP', raising=False)
    else:
        monkeypatch.setenv('RRI_WSWEEP', wsweep)           # read at rri_create
    X, W0, T0 = problem()
    calls = [(2, {}), (1, dict(fix_T=True)), (1, {}), (1, dict(fix_T=True))]
    Wr, Tr = oracle_chain(X, W0, T0, calls)
    W, T = engine_chain(X, W0, T0, calls, 'residual')
    ew, et = relfro(W, Wr), relfro(T, Tr)
    print('residual handle vs oracle: W %.3e  T %.3e' % (ew, et))
    assert ew < TOL and et < TOL, (ew, et)
    Wg, Tg = engine_chain(X, W0, T0, calls, 'gram')        # and the default schedule
    ew, et = relfro(W, Wg), relfro(T, Tg)
    print('residual handle vs Gram-form handle: W %.3e  T %.3e' % (ew, et))
    assert ew < TOL and et < TOL, (ew, et)


def test_reset_outside_a_paused_run_between_two_fixed_T_sweeps(monkeypatch):
    """T fixed sweep(1), row 3 of T replaced by rri_apply_reset_vectors with no run paused, T fixed sweep(1)"""
    from rri_nmf_amd.engine import RRIEngine
    monkeypatch.setenv('RRI_ONCHIP', '0')
    X, W0, T0 = problem()
    new_row = np.random.RandomState(7).rand(D)
    new_row /= new_row.sum()
    W1, T1 = oracle_chain(X, W0, T0, [(1, dict(fix_T=True))])
    T1 = T1.copy()
    T1[3, :] = new_row
    Wr, Tr = oracle_chain(X, W1, T1, [(1, dict(fix_T=True))])
    with RRIEngine(N, D, K, dtype=np.float64) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0)
        e.set_params(fix_T=True)
        e.sweep(1)
        e.apply_reset_vectors(3, new_row, e.get_W()[:, 3])
        e.sweep(1)
        W, T = e.get_W(), e.get_T()
    ew, et = relfro(W, Wr), relfro(T, Tr)
    print('reset between fixed-T sweeps vs oracle: W %.3e  T %.3e' % (ew, et))
    assert ew < TOL and et < TOL, (ew, et)
