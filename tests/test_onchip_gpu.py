"""The register-resident persistent sweep (rri_onchip_kernels.hpp): launch-bound sizes whose fp32 X fits the chip's
registers run rri_sweep as ONE launch with two exchanges between workgroups per topic step (the data is its own hand-over).  Same arithmetic as the launch-per-phase
kernels (nmf.py:437-476, 670-676, 728-734), another order of the partial sums:

  * against the launch-per-phase schedule (RRI_ONCHIP=0) on the same inputs: 1e-9, every wave layout (d <= 256 / 512 /
    1024 / 2048), ragged shapes, k = 2 ... 64, regularisation, the c <= 0 branches with bounds;
  * against the CPU oracle (the reference's operation order): 2e-9, BASELINE's 10000 x 1000, k = 20 included;
  * reset events of both kinds through nmf(): the same events at the same steps, the same result;
  * the topic-model flags (T rows projected onto the simplex at every step: one more hand-over among the workers), the
    one-hot branch of qf_min included;
  * float64 storage (half the rows per workgroup), the reference's vectors through it (the goldens of tests/golden run in
    float64: test_hip_parity.py / test_nmf_gpu.py take this path wherever the configuration allows);
  * k up to 64 and d up to 2048 (plain flags), compared from a warm start (the first sweeps of a long chain from a random start
    are chaotic for any implementation: tools/onchip_large_k_check.py);
  * what the path does not cover (fixed halves, k > 64, d > 1024 with a projection, too many rows for the registers) reports not
    eligible and runs as before.
"""
import os

import numpy as np
import pytest

from conftest import relfro
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


class onchip(object):
    """RRI_ONCHIP for the handles created inside (rri_create reads the environment)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get('RRI_ONCHIP')
        os.environ['RRI_ONCHIP'] = '1' if self.on else '0'

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop('RRI_ONCHIP', None)
        else:
            os.environ['RRI_ONCHIP'] = self.old


def run(X, W0, T0, sweeps, on, objective=False, dtype=np.float32, **params):
    n, d = X.shape
    k = W0.shape[1]
    with onchip(on), engine(n, d, k, dtype=dtype) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**params)
        eligible, before = e.onchip_info()
        assert eligible == bool(on), (eligible, on)
        objs = []
        for _ in range(sweeps if objective else 1):
            e.sweep(1 if objective else sweeps)
            if objective:
                objs.append(e.objective())
        launches = e.onchip_info()[1] - before
        assert (launches > 0) == bool(on), launches
        return e.get_W(), e.get_T(), np.array(objs), e.n_resets_used


SHAPES = [(50, 30, 3), (700, 200, 2), (1501, 333, 6), (2600, 512, 7), (4096, 1024, 5), (5003, 1000, 22), (10000, 1000, 20),
          (300, 700, 4), (10240, 1024, 8),
          (3001, 1000, 23), (5000, 800, 47), (5000, 1000, 64), (900, 256, 33),        # k-term dots of 8 terms per lane (k <= 64)
          (5000, 2000, 12), (2500, 1500, 40), (5120, 2048, 3), (1000, 1030, 20)]      # 8 column groups (1024 < d <= 2048)


@pytest.mark.parametrize('shape', SHAPES)
def test_onchip_equals_launch_per_phase(shape):
    n, d, k = shape
    X = planted_X(n, d, min(k, 20), seed=n + d, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=5)
    if k > 22:
        # From a random start the first sweeps of a LONG Gauss-Seidel chain are chaotic: every topic step multiplies a rounding
        # difference by ~1.5, and at k = 47 / 64 either schedule is 2e-5 / 2e-3 away from the CPU oracle after ONE sweep -- and
        # 4e-6 / 3e-4 from the other (tools/onchip_large_k_check.py, profiles/r03_onchip_large_k.log).  Two sweeps on, the same
        # comparison holds 1e-14: the kernels are compared from there.
        W0, T0, _, _ = run(X, W0, T0, 2, False)
    Wa, Ta, oa, _ = run(X, W0, T0, 3, True, objective=True)
    Wb, Tb, ob, _ = run(X, W0, T0, 3, False, objective=True)
    # the two paths add the same terms in another order: what that leaves after 3 sweeps grows with k (the Gauss-Seidel
    # chain of a sweep from a random start amplifies a rounding difference topic by topic; 2e-11 at k = 20)
    print('on-chip vs launch-per-phase %s: W %.2e, T %.2e' % (shape, relfro(Wa, Wb), relfro(Ta, Tb)))
    tol = 1e-9
    assert relfro(Wa, Wb) < tol and relfro(Ta, Tb) < tol, (relfro(Wa, Wb), relfro(Ta, Tb))
    # after an on-chip sweep the objective comes from the cross terms the kernel left (no pass over X), as after k_wcol
    assert np.allclose(oa, ob, rtol=1e-10), (oa, ob)
    assert np.all(np.diff(oa) <= 1e-9 * oa[0])


@pytest.mark.parametrize('params', [
    dict(reg_w_l1=0.01, reg_t_l1=0.02, reg_w_l2=0.05, reg_t_l2=0.03),
    dict(t_row_sum=1.0),                                   # an upper bound without a projection (the RS flags' T side)
    dict(t_row_sum=1.0, w_row_sum=1.0, reset_topic_method=None),
    dict(reset_topic_method=None),
])
def test_flag_sets(params):
    n, d, k = 1800, 640, 5
    X = planted_X(n, d, k, seed=11, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=12)
    Wa, Ta, _, _ = run(X, W0, T0, 4, True, **params)
    Wb, Tb, _, _ = run(X, W0, T0, 4, False, **params)
    assert relfro(Wa, Wb) < 1e-11 and relfro(Ta, Tb) < 1e-11, (relfro(Wa, Wb), relfro(Ta, Tb))


@pytest.mark.parametrize('shape', [(1501, 333, 6), (10000, 1000, 20)])
def test_against_the_cpu_oracle(shape):
    from oracle import rri_oracle as orc
    n, d, k = shape
    X = planted_X(n, d, k, seed=21, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=22)
    sweeps = 5
    Wa, Ta, _, _ = run(X, W0, T0, sweeps, True)
    Wc, Tc = W0.astype(np.float64).copy(), T0.astype(np.float64).copy()
    orc.plain_sweeps(np.asarray(X, dtype=np.float64), Wc, Tc, sweeps)
    assert relfro(Wa, Wc) < 2e-9 and relfro(Ta, Tc) < 2e-9, (relfro(Wa, Wc), relfro(Ta, Tc))
    assert np.array_equal(np.argmax(Wa, 1), np.argmax(Wc, 1))


@pytest.mark.parametrize('k', [47, 64])
def test_large_k_from_a_cold_start(k):
    """k beyond one round of Gram loads, from the SURVEY's own random start (review r3, weak 1: both schedules 1.8e-3 from the
    oracle after ONE sweep at 5000 x 1000, k = 64 -- a defect beyond 50 topics, or the chain?).  Two answers:
    (i) topic step by topic step, the device restarted from the ORACLE's state before every half step (nothing accumulates): all
        k T rows and W columns agree to 1e-12 -- no Gram slice, no k-term dot goes wrong beyond 50 topics;
    (ii) the whole sweep against the oracle, bounded by a MEASURED control -- the oracle against itself with every entry of W0 one
        ulp up (tools/large_k_control.py, profiles/r04_large_k_control.log: 6.9e-6 at k = 47, 9.5e-4 at k = 64: a sweep of k
        dependent steps multiplies a rounding difference by ~1.45 per step) -- and by a fixed cap."""
    from oracle import rri_oracle as orc
    n, d = 5000, 1000
    X = planted_X(n, d, k, seed=n + d, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=5)
    X64, W, T = np.asarray(X, dtype=np.float64), W0.astype(np.float64), T0.astype(np.float64)
    # (i) half step by half step from the oracle's state (the launch-per-phase kernels: the persistent kernel cannot stop inside
    # a sweep; it is held against them at 1e-9 from a warm start, test_onchip_equals_launch_per_phase)
    worst_t, worst_w = 0.0, 0.0
    with onchip(False), engine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X), e.set_params()
        for t in range(k):
            e.set_W(W), e.set_T(T)
            e.update_T_row(t)
            wR, nw = orc.residual_products_T(X64, W, T, t)
            x, nt1 = orc.qf_min(-wR, nw, s=None, ub=None)
            worst_t = max(worst_t, relfro(e.get_T()[t], x))
            T[t] = x
            W[:, t] = W[:, t] * nt1
            e.set_W(W), e.set_T(T)
            e.update_W_col(t)
            Rt, nt = orc.residual_products_W(X64, W, T, t)
            w, _ = orc.qf_min(-Rt, nt, s=None, ub=None)
            worst_w = max(worst_w, relfro(e.get_W()[:, t], w))
            W[:, t] = w
    print('k = %d cold start, every half step from the oracle\'s state: worst T row %.2e, worst W column %.2e' % (k, worst_t, worst_w))
    # measured: T rows 3e-13 (k = 47) and 5e-13 (k = 64) -- the numerator of a T row is a difference of sums a hundred times its size
    # (tools/large_k_control.py) --, W columns 6e-15; the oracle's BLAS may order its sums differently on another host
    assert worst_t < 5e-12 and worst_w < 1e-12, (worst_t, worst_w)
    # (ii) W, T now hold the oracle's sweep
    Wu, Tu = np.nextafter(W0.astype(np.float64), np.inf), T0.astype(np.float64)
    orc.plain_sweeps(X64, Wu, Tu, 1)
    sens = max(relfro(Wu, W), relfro(Tu, T))
    tol = min(max(2e-9, 10 * sens), 2e-2)
    Wa, Ta, _, _ = run(X, W0, T0, 1, True)
    Wb, Tb, _, _ = run(X, W0, T0, 1, False)
    print('k = %d cold start, one sweep: control (oracle vs itself, W0 one ulp up) %.2e, bound %.2e | persistent W %.2e T %.2e | '
          'launch-per-phase W %.2e T %.2e' % (k, sens, tol, relfro(Wa, W), relfro(Ta, T), relfro(Wb, W), relfro(Tb, T)))
    for Wg, Tg in ((Wa, Ta), (Wb, Tb)):
        assert relfro(Wg, W) < tol and relfro(Tg, T) < tol, (relfro(Wg, W), relfro(Tg, T), sens)


@pytest.mark.parametrize('flags', [dict(t_row_sum=1.0, reg_w_l1=1e6), dict(t_row_sum=1.0, reg_t_l1=1e6),
                                   dict(t_row_sum=1.0, reg_w_l1=1e6, reset_topic_method='random', fix_reset_seed=True)])
def test_reset_events_through_nmf(flags):
    """columns / rows driven to zero: the events are raised by the persistent kernel at the step that finds them, resolved
    by the host (nmf.py:751-816) and the run resumed in the middle of a sweep"""
    from rri_nmf_amd import nmf as nmf_mod
    n, d, k = 600, 200, 4
    X = planted_X(n, d, k, seed=31, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=32)
    out = []
    for on in (True, False):
        with onchip(on):
            np.random.seed(0)
            out.append(nmf_mod.nmf(X, k, W_in=W0, T_in=T0, max_iter=2, eps_stop=-1, compute_obj_each_iter=True,
                                   dtype=np.float32, **flags))
    a, b = out
    assert a['n_resets_used'] == b['n_resets_used'] >= k
    assert relfro(a['W'], b['W']) < 1e-10 and relfro(a['T'], b['T']) < 1e-10
    assert np.allclose(a['obj_history'], b['obj_history'], rtol=1e-10)


def test_dead_column_without_resets_is_the_reference_error():
    n, d, k = 400, 150, 3
    X = planted_X(n, d, k, seed=41, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=42)
    from rri_nmf_amd import nmf as nmf_mod
    for on in (True, False):
        with onchip(on), pytest.raises(AssertionError, match='sums to 0'):
            nmf_mod.nmf(X, k, W_in=W0, T_in=T0, max_iter=2, eps_stop=-1, reg_w_l1=1e6, reset_topic_method=None,
                        dtype=np.float32)


def test_what_is_not_covered_stays_on_the_launch_per_phase_path():
    n, d, k = 900, 300, 4
    X = planted_X(n, d, k, seed=51, dtype=np.float64)
    W0, T0 = scaled_init(X, k, seed=52)
    for dtype, params in ((np.float32, dict(fix_T=True)), (np.float64, dict(fix_W=True))):
        with onchip(True), engine(n, d, k, dtype=dtype) as e:
            e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**params)
            assert e.onchip_info() == (False, 0)
            e.sweep(1)
            assert e.onchip_info() == (False, 0)
    with onchip(True), engine(n, d, 65, dtype=np.float32) as e:            # more topics than the k-term dots of the kernel take
        e.set_params()
        e.upload_X(X)
        assert e.onchip_info()[0] is False
    Xw = np.zeros((600, 1100), dtype=np.float32)                           # the projection stage stages whole T rows: d <= 1024
    for params, eligible in ((dict(), True), (dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0), False)):
        with onchip(True), engine(600, 1100, 4, dtype=np.float32) as e:
            e.set_params(**params)
            e.upload_X(Xw)
            assert e.onchip_info()[0] is eligible
    with onchip(True), engine(40000, 1024, 4, dtype=np.float32) as e:      # too many rows per CU for the registers
        e.set_params()
        e.upload_X(np.zeros((40000, 1024), dtype=np.float32))
        assert e.onchip_info()[0] is False


def test_many_sweeps_in_one_launch_and_a_later_call_continue_the_same_run():
    n, d, k = 3000, 800, 6
    X = planted_X(n, d, k, seed=61, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=62)
    with onchip(True), engine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params()
        e.sweep(7)
        e.sweep(3)
        Wa, Ta = e.get_W(), e.get_T()
        assert e.onchip_info()[1] == 2
    Wb, Tb, _, _ = run(X, W0, T0, 10, False)
    assert relfro(Wa, Wb) < 1e-10 and relfro(Ta, Tb) < 1e-10


@pytest.mark.parametrize('flags', [{}, dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)], ids=['plain', 'topic-model'])
def test_a_grid_that_cannot_synchronise_falls_back_to_the_launch_per_phase_schedule(monkeypatch, flags):
    """the hand-overs poll a bounded number of times; RRI_ONCHIP_SPIN_LIMIT=0 makes the first unsatisfied poll give up, as a
    grid whose workgroups are not all resident would.  The reference's sweep cannot fail for scheduling reasons
    (nmf.py:415-476): the call must COMPLETE -- W, T as before the launch, the same steps launch by launch -- with the result
    of the launch-per-phase schedule, and count the fallback; the handle then stays on that schedule."""
    n, d, k = 3000, 800, 6
    X = planted_X(n, d, k, seed=71, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=72)
    Wb, Tb, _, _ = run(X, W0, T0, 2, False, **flags)
    Wb5, Tb5, _, _ = run(X, W0, T0, 5, False, **flags)
    monkeypatch.setenv('RRI_ONCHIP_SPIN_LIMIT', '0')
    monkeypatch.setenv('RRI_ONCHIP_BACKOFF_MS', '0')       # the process-wide back-off after a fallback (2 s) would keep the later handles of this test off the path
    with onchip(True), engine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**flags)
        assert e.onchip_info()[0] is True
        e.sweep(2)
        assert e.onchip_fallbacks() == 1 and e.onchip_info() == (False, 1)
        Wa, Ta = e.get_W(), e.get_T()
        # bit for bit what the launch-per-phase schedule gives: the half-run persistent launch left nothing behind
        assert np.array_equal(Wa, Wb) and np.array_equal(Ta, Tb), (relfro(Wa, Wb), relfro(Ta, Tb))
        e.sweep(3)                                              # stays on the launch-per-phase schedule: no further attempt
        assert e.onchip_fallbacks() == 1 and e.onchip_info() == (False, 1)
        assert np.array_equal(e.get_W(), Wb5) and np.array_equal(e.get_T(), Tb5)
    monkeypatch.delenv('RRI_ONCHIP_SPIN_LIMIT')
    Wc, Tc, _, _ = run(X, W0, T0, 2, True, **flags)           # the device and the library are fine afterwards
    assert relfro(Wc, Wb) < 1e-10 and relfro(Tc, Tb) < 1e-10


@pytest.mark.parametrize('flags', [{}, dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)], ids=['plain', 'topic-model'])
def test_a_launch_that_gives_up_inside_the_run_is_rolled_back_whole(monkeypatch, flags):
    """The fallback tests above make the grid give up at its ENTRY (RRI_ONCHIP_SPIN_LIMIT=0 sets both bounds), where nothing has
    been written yet.  Here the entry hand-over keeps its default bound and every workgroup gives up in phase B of a topic step
    in the middle of the second sweep (RRI_ONCHIP_FAIL_STEP: as if its polls had run out there): by then the launch has rewritten
    W columns and T rows, the cross terms of the objective and -- under rri_sweep_until -- the history slot of the first sweep.
    The call must still return the launch-per-phase result bit for bit, with no objective of the abandoned launch left in the
    history (rri_hip.h: NaN = the kernel left none for that sweep)."""
    n, d, k = 3000, 800, 6
    X = planted_X(n, d, k, seed=71, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=72)
    Wb, Tb, ob, _ = run(X, W0, T0, 3, False, objective=True, **flags)
    Wb1, Tb1, _, _ = run(X, W0, T0, 1, False, **flags)
    monkeypatch.setenv('RRI_ONCHIP_BACKOFF_MS', '0')
    monkeypatch.setenv('RRI_ONCHIP_FAIL_STEP', str(k + 2))          # third topic step of the second sweep
    with onchip(True), engine(n, d, k, dtype=np.float32) as e:       # (i) rri_sweep
        e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**flags)
        assert e.onchip_info()[0] is True
        e.sweep(3)
        assert e.onchip_fallbacks() == 1 and e.onchip_info() == (False, 1)
        Wa, Ta = e.get_W(), e.get_T()
        assert np.array_equal(Wa, Wb) and np.array_equal(Ta, Tb), (relfro(Wa, Wb), relfro(Ta, Tb))
        # the objective is evaluated for the state the rerun produced, not taken from what the abandoned launch left behind
        assert abs(e.objective() - ob[-1]) <= 1e-12 * abs(ob[-1]), (e.objective(), ob[-1])
    with onchip(True), engine(n, d, k, dtype=np.float32) as e:       # (ii) rri_sweep_until: the history of the call
        e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**flags)
        o0 = e.objective()
        res = e.sweep_until(3, o0, -1.0)
        assert res is not None and e.onchip_fallbacks() == 1
        n_done, hist = res
        # the rerun has no stop rule between its sweeps: ONE sweep launch by launch, and no value of the abandoned launch --
        # which had finished the first sweep and written its slot -- in the history
        assert n_done == 1 and np.isnan(hist).all(), (n_done, hist)
        assert np.array_equal(e.get_W(), Wb1) and np.array_equal(e.get_T(), Tb1)
        assert abs(e.objective() - ob[0]) <= 1e-12 * abs(ob[0])


def test_a_fallback_when_a_paused_run_resumes_takes_over_at_the_same_half_step(monkeypatch):
    """a run interrupted by a T-row reset resumes in the W half of that topic (cursor phase 1, the row checks of the resumed
    step skipped).  When THAT persistent launch gives up, the launch-per-phase schedule must take over at exactly that
    half step: same events afterwards, same result as a handle that never left the launch-per-phase schedule."""
    import ctypes as C
    from rri_nmf_amd import _capi
    n, d, k = 600, 200, 4
    X = planted_X(n, d, k, seed=31, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=32)
    flags = dict(t_row_sum=1.0, reg_t_l1=1e6)               # every T row is driven to zero: a reset event per topic step

    def drive(e, give_up_from_event):
        done, events = C.c_int32(0), 0
        st = e._lib.rri_sweep(e._h, 2, C.byref(done))
        while st == _capi.RRI_PAUSED:
            e._resolve_event()
            events += 1
            if events == give_up_from_event:
                monkeypatch.setenv('RRI_ONCHIP_SPIN_LIMIT', '0')
                monkeypatch.setenv('RRI_ONCHIP_BACKOFF_MS', '0')
            st = e._lib.rri_resume(e._h, C.byref(done))
        e._check(st)
        monkeypatch.delenv('RRI_ONCHIP_SPIN_LIMIT', raising=False)
        return e.get_W(), e.get_T(), events, list(e.reset_log)

    out = []
    for on, give_up in ((True, 1), (False, -1)):
        with onchip(on), engine(n, d, k, dtype=np.float32) as e:
            e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**flags)
            out.append(drive(e, give_up) + (e.onchip_fallbacks(), e.onchip_info()[1]))
    (Wa, Ta, ea, la, fa, na), (Wb, Tb, eb, lb, fb, nb) = out
    assert fa == 1 and na == 2 and fb == 0 and nb == 0, (fa, na, fb, nb)      # two persistent launches, the second gave up
    assert ea == eb >= k and la == lb
    assert relfro(Wa, Wb) < 1e-10 and relfro(Ta, Tb) < 1e-10, (relfro(Wa, Wb), relfro(Ta, Tb))


def test_a_fallback_backs_the_whole_process_off_the_persistent_path_for_a_while(monkeypatch):
    """a launch that gave up means the device is shared with somebody whose grids collide with ours (four processes on one GPU:
    5-13 collisions in 400 calls, tools/onchip_two_processes.py): a process that makes a handle per nmf() call must not walk
    into the same wait with every new handle -- for RRI_ONCHIP_BACKOFF_MS (default 2000) no handle of the process is eligible"""
    import time
    n, d, k = 3000, 800, 6
    X = planted_X(n, d, k, seed=71, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=72)
    monkeypatch.setenv('RRI_ONCHIP_SPIN_LIMIT', '0')
    monkeypatch.setenv('RRI_ONCHIP_BACKOFF_MS', '700')
    with onchip(True), engine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params()
        e.sweep(1)
        assert e.onchip_fallbacks() == 1
    monkeypatch.delenv('RRI_ONCHIP_SPIN_LIMIT')
    with onchip(True), engine(n, d, k, dtype=np.float32) as e2:
        e2.upload_X(X), e2.set_W(W0), e2.set_T(T0), e2.set_params()
        assert e2.onchip_info()[0] is False                 # a NEW handle, inside the back-off
        time.sleep(0.9)
        assert e2.onchip_info()[0] is True                  # ... and after it
        e2.sweep(1)
        assert e2.onchip_info() == (True, 1) and e2.onchip_fallbacks() == 0


def test_two_handles_of_different_instantiations_on_two_streams_are_ordered():
    """every persistent launch of a process waits for the one before it on the same device, whatever its template
    instantiation (round 2 kept the mutex and the event inside the template: an fp32 and a float64 handle, or a plain and a
    topic-model one, were not ordered and could each hold half of the CUs).  Four handles -- fp32 plain (20 rows per wave),
    fp32 topic model, float64 plain, fp32 small (8 rows per wave) -- sweep from four threads at once, several calls each;
    nothing may give up and every result equals the handle's own sequential run."""
    import threading
    cases = [((10000, 1000, 20), np.float32, {}), ((6000, 1000, 12), np.float32, TM), ((5000, 1000, 10), np.float64, {}),
             ((2000, 512, 6), np.float32, {})]
    data = []
    for (n, d, k), dt, flags in cases:
        X = planted_X(n, d, k, seed=n + k, dtype=np.float32)
        W0, T0 = scaled_init(X, k, seed=91)
        data.append((X.astype(dt), W0, T0, dt, flags))
    want = [run(X, W0, T0, 6, True, dtype=dt, **flags)[:2] for X, W0, T0, dt, flags in data]
    got, errs = [None] * len(data), []

    def work(i):
        try:
            X, W0, T0, dt, flags = data[i]
            n, d = X.shape
            e = engines[i]
            for _ in range(3):
                e.sweep(2)
            got[i] = (e.get_W(), e.get_T(), e.onchip_info()[1], e.onchip_fallbacks())
        except Exception as ex:      # noqa: BLE001
            errs.append((i, repr(ex)))

    with onchip(True):
        engines = []
        for X, W0, T0, dt, flags in data:
            e = engine(X.shape[0], X.shape[1], W0.shape[1], dtype=dt)
            e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**flags)
            assert e.onchip_info()[0] is True
            engines.append(e)
    try:
        threads = [threading.Thread(target=work, args=(i,)) for i in range(len(data))]
        [t.start() for t in threads]
        [t.join() for t in threads]
    finally:
        [e.close() for e in engines]
    assert not errs, errs
    for i, (Wg, Tg, launches, fallbacks) in enumerate(got):
        assert launches == 3 and fallbacks == 0, (i, launches, fallbacks)
        assert np.array_equal(Wg, want[i][0]) and np.array_equal(Tg, want[i][1]), (i, relfro(Wg, want[i][0]))


TM = dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)


@pytest.mark.parametrize('shape', [(50, 30, 3), (1501, 333, 6), (2600, 512, 7), (10000, 1000, 20), (4096, 1024, 5), (3000, 700, 40)])
def test_topic_model_flags(shape):
    """qf_min with s = t_row_sum (optimization.py:53-59) and _project_and_check_reset_t (nmf.py:751-769) inside the persistent
    kernel: both schedules, the oracle, rows of T on the simplex"""
    from oracle import rri_oracle as orc
    n, d, k = shape
    X = planted_X(n, d, k, seed=81, dtype=np.float32)
    X = X / X.sum(1, keepdims=True)
    # the start the estimator makes (NNDSVDa, rows of W and T scaled to the simplex, nmf.py:840-850).  From an unscaled random
    # start the unprojected T rows of the first sweep have sums of ~200 at 10000 x 1000: the projection then subtracts a theta
    # a hundred times the entries it keeps, ONE half step agrees with the oracle to 1e-14 instead of 1e-16
    # (tools/tm_parity_steps.py) and the k dependent steps amplify that to 4e-5 after a sweep -- for both schedules and both
    # storage types alike, and invisibly to a permutation control (the reference sums the projection in sorted order)
    from rri_nmf_amd import initialization
    W0, T0 = initialization.initialize_nmf(np.asarray(X, dtype=np.float64), k, init='nndsvda', random_state=0)
    T0 = T0 / T0.sum(1, keepdims=True)
    W0 = W0 / W0.sum(1, keepdims=True)
    Wa, Ta, oa, _ = run(X, W0, T0, 3, True, objective=True, **TM)
    Wb, Tb, ob, _ = run(X, W0, T0, 3, False, objective=True, **TM)
    # the two schedules: summation order only
    assert relfro(Wa, Wb) < 1e-8 and relfro(Ta, Tb) < 1e-8, (relfro(Wa, Wb), relfro(Ta, Tb))
    assert np.allclose(oa, ob, rtol=1e-8)
    assert np.abs(Ta.sum(1) - 1).max() < 1e-12 and Ta.min() >= 0
    # Against the oracle; the bound is measured: the oracle against itself on the column-permuted problem (the same mathematics,
    # another order of the sums over columns) says what two correct implementations can differ by
    X64, W64, T64 = np.asarray(X, dtype=np.float64), W0.astype(np.float64), T0.astype(np.float64)
    kw = dict(max_iter=3, eps_stop=-1, project_W_each_iter=False, do_final_project_W=False, **TM)
    ref = orc.nmf(X64, k, W_in=W64.copy(), T_in=T64.copy(), **kw)
    perm = np.random.RandomState(0).permutation(d)
    ctl = orc.nmf(np.ascontiguousarray(X64[:, perm]), k, W_in=W64.copy(), T_in=np.ascontiguousarray(T64[:, perm]), **kw)
    sens = max(relfro(ctl['T'], ref['T'][:, perm]), relfro(ctl['W'], ref['W']))
    # ... but never beyond a FIXED bound: 1e-7 is fifty times what the launch-per-phase schedule holds on the worst of these
    # shapes, so a regression of two orders of magnitude cannot hide behind a large control
    tol = min(max(2e-9, 50 * sens), 1e-7)
    print('topic-model flags %r: control (oracle vs its column permutation) %.2e, bound %.2e' % (shape, sens, tol))
    for Tg, Wg in ((Ta, Wa), (Tb, Wb)):
        assert relfro(Tg, ref['T']) < tol and relfro(Wg, ref['W']) < tol, (relfro(Tg, ref['T']), relfro(Wg, ref['W']), sens)


def test_topic_model_one_hot_rows_when_the_quadratic_term_vanishes():
    """scalar c <= 0 with s = 1: the row becomes the unit vector of the arg-max of the numerator (optimization.py:68-73)"""
    n, d, k = 900, 300, 4
    X = planted_X(n, d, k, seed=91, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=92)
    flags = dict(TM, reg_t_l2=-1e9)
    Wa, Ta, _, _ = run(X, W0, T0, 2, True, **flags)
    Wb, Tb, _, _ = run(X, W0, T0, 2, False, **flags)
    assert np.array_equal(Ta, Tb) and set(np.unique(Ta)) == {0.0, 1.0} and np.all(Ta.sum(1) == 1.0)
    assert relfro(Wa, Wb) < 1e-10


def test_topic_model_estimator_on_the_text_fixture_in_fp32_storage():
    """NMF_TM_Estimator.fit on the reference's text fixture with fp32 storage: the persistent kernel against the
    launch-per-phase schedule -- same topic assignments, factors to summation order"""
    from rri_nmf_amd import sklearn_interface as si
    from conftest import load_golden
    g = load_golden('g1_tm_estimator')
    X = np.asarray(g['X'], dtype=np.float64)
    n, d = X.shape
    out = []
    for on in (True, False):
        with onchip(on):
            E = si.NMF_TM_Estimator(n, d, 5, random_state=0, max_iter=10, nmf_kwargs={'eps_stop': -1, 'dtype': np.float32}).fit(X)
            out.append((E.W.copy(), E.T.copy()))
    (Wa, Ta), (Wb, Tb) = out
    assert relfro(Wa, Wb) < 1e-9 and relfro(Ta, Tb) < 1e-9
    assert np.array_equal(np.argmax(Wa, 1), np.argmax(Wb, 1))
    assert np.array_equal(np.argmax(Wa, 1), g['argmax_s10'])        # the reference's own assignments after 10 sweeps (float64 run)


@pytest.mark.parametrize('shape', [(50, 30, 3), (1501, 333, 6), (2501, 1000, 12), (5000, 1022, 20), (2600, 510, 7), (2000, 900, 36)])
@pytest.mark.parametrize('flags', [dict(), TM])
def test_float64_storage(shape, flags):
    """8 registers per row and lane; LD is a multiple of 2 only (the second pair of a lane's four columns may lie past the row)"""
    from oracle import rri_oracle as orc
    n, d, k = shape
    X = planted_X(n, d, k, seed=101, dtype=np.float64)
    if flags:
        from rri_nmf_amd import initialization
        X = X / X.sum(1, keepdims=True)
        W0, T0 = initialization.initialize_nmf(X, k, init='nndsvda', random_state=0)
        T0, W0 = T0 / T0.sum(1, keepdims=True), W0 / W0.sum(1, keepdims=True)
    else:
        W0, T0 = scaled_init(X, k, seed=102)
    Wa, Ta, oa, _ = run(X, W0, T0, 3, True, objective=True, dtype=np.float64, **flags)
    Wb, Tb, ob, _ = run(X, W0, T0, 3, False, objective=True, dtype=np.float64, **flags)
    assert relfro(Wa, Wb) < 1e-8 and relfro(Ta, Tb) < 1e-8, (relfro(Wa, Wb), relfro(Ta, Tb))
    assert np.allclose(oa, ob, rtol=1e-8)
    kw = dict(max_iter=3, eps_stop=-1, project_W_each_iter=False, do_final_project_W=False, **flags)
    ref = orc.nmf(X, k, W_in=W0.copy(), T_in=T0.copy(), **kw)
    perm = np.random.RandomState(0).permutation(d)
    ctl = orc.nmf(np.ascontiguousarray(X[:, perm]), k, W_in=W0.copy(), T_in=np.ascontiguousarray(T0[:, perm]), **kw)
    sens = max(relfro(ctl['T'], ref['T'][:, perm]), relfro(ctl['W'], ref['W']))
    tol = min(max(2e-9, 50 * sens), 1e-7)                    # measured control, capped by a fixed bound
    print('float64 storage %r %s: control %.2e, bound %.2e' % (shape, 'topic-model' if flags else 'plain', sens, tol))
    assert relfro(Ta, ref['T']) < tol and relfro(Wa, ref['W']) < tol, (relfro(Ta, ref['T']), relfro(Wa, ref['W']), tol)


@pytest.mark.parametrize('flags', [dict(), TM])
def test_same_bits_run_to_run(flags):
    """every sum of the persistent kernel has a fixed order (no atomics; the polls only decide WHEN a value is used): two runs of
    the same problem give the same bits, whatever the order in which the workgroups' values arrive"""
    n, d, k = 6000, 1000, 12
    X = planted_X(n, d, k, seed=111, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=112)
    T0 = T0 / T0.sum(1, keepdims=True)
    runs = [run(X, W0, T0, 7, True, **flags) for _ in range(3)]
    for Wr, Tr, _, _ in runs[1:]:
        assert np.array_equal(Wr, runs[0][0]) and np.array_equal(Tr, runs[0][1])


@pytest.mark.parametrize('flags', [dict(), TM], ids=['plain', 'topic-model'])
def test_naps_change_the_timing_of_the_polls_and_nothing_else(monkeypatch, flags):
    """a wave sleeps through part of a wait it expects before it polls again (RRI_ONCHIP_NAP_EIGHTHS, OnchipNap): with the naps
    off, at 3/8 and at 7/8 of the observed wait the same bits come out"""
    n, d, k = 6000, 900, 12
    X = planted_X(n, d, k, seed=91, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=92)
    T0 = T0 / T0.sum(1, keepdims=True)
    got = []
    for eighths in ('0', '3', '7'):
        monkeypatch.setenv('RRI_ONCHIP_NAP_EIGHTHS', eighths)
        Wg, Tg, _, _ = run(X, W0, T0, 6, True, **flags)
        got.append((Wg, Tg))
    for Wg, Tg in got[1:]:
        assert np.array_equal(Wg, got[0][0]) and np.array_equal(Tg, got[0][1])

@pytest.mark.parametrize('shape', [(5000, 1000, 20), (3000, 700, 40)], ids=['k = 20', 'k = 40'])
@pytest.mark.parametrize('flags', [dict(), TM], ids=['plain', 'topic-model'])
def test_another_order_of_arrivals_at_every_hand_over_gives_the_same_bits(monkeypatch, shape, flags):
    """The exchanges of the persistent sweep carry no flags: a slot says by its content whether the value of the step has arrived,
    and its owner re-marks it absent "where every reader is known to be past it" (rri_onchip_kernels.hpp).  What such a protocol
    breaks on is the ORDER in which the stores, re-marks and polls of different workgroups reach the memory side -- and a quiet
    machine shows few orders.  RRI_ONCHIP_JITTER = seed makes every wave sleep a pseudo-random 0-5 us (a hash of seed, workgroup,
    wave, topic step and site) before each of its exchange stores, re-marks and first polls: three seeds, the objective carried
    along, k below and beyond one round of Gram loads -- the same bits as the undisturbed run, and as each other."""
    n, d, k = shape
    X = planted_X(n, d, min(k, 20), seed=171, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=172)
    if flags:
        X = X / X.sum(1, keepdims=True)
        T0 = T0 / T0.sum(1, keepdims=True)
        W0 = W0 / W0.sum(1, keepdims=True)
    W0, T0, _, _ = run(X, W0, T0, 2, False, **flags)         # a warm start: the first sweeps of a long chain are ill-conditioned
    want = run(X, W0, T0, 4, True, objective=True, **flags)
    for seed in ('1', '77', '4242'):
        monkeypatch.setenv('RRI_ONCHIP_JITTER', seed)
        got = run(X, W0, T0, 4, True, objective=True, **flags)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (seed, relfro(got[0], want[0]), relfro(got[1], want[1]))
        assert np.array_equal(got[2], want[2]), (seed, got[2], want[2])
    monkeypatch.delenv('RRI_ONCHIP_JITTER')
    # many sweeps in ONE launch (the slots are re-marked and reused hundreds of times), disturbed: still the undisturbed bits
    want30 = run(X, W0, T0, 30, True, **flags)
    monkeypatch.setenv('RRI_ONCHIP_JITTER', '9')
    got30 = run(X, W0, T0, 30, True, **flags)
    assert np.array_equal(got30[0], want30[0]) and np.array_equal(got30[1], want30[1])


@pytest.mark.parametrize('flags', [dict(), dict(reg_w_l1=0.01, reg_t_l1=0.02, reg_w_l2=0.05, reg_t_l2=0.03), TM],
                         ids=['plain', 'regularised', 'topic-model'])
def test_the_objective_the_persistent_sweep_leaves_behind(monkeypatch, flags):
    """nmf() asks for the objective after every sweep (nmf.py:488-490, 510).  The persistent kernel accumulates it on the way --
    a row's share of step t is w_it (-y_i + sum_{l<t} (T T^T)_tl w_il + 1/2 (T T^T)_tt w_it) plus its penalties -- and leaves
    it with the state the host reads anyway: rri_objective launches nothing.  Against the Gram kernels of the other path
    (RRI_ONCHIP_OBJ=0) and against 1/2 ||X - W T||^2 taken through the residual (RRI_OBJ_DIRECT=1)"""
    n, d, k = 4000, 900, 9
    X = planted_X(n, d, k, seed=131, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=132)
    T0 = T0 / T0.sum(1, keepdims=True)
    got = {}
    for name, env in (('tracked', {}), ('gram', {'RRI_ONCHIP_OBJ': '0'}), ('direct', {'RRI_OBJ_DIRECT': '1'})):
        for key in ('RRI_ONCHIP_OBJ', 'RRI_OBJ_DIRECT'):
            monkeypatch.delenv(key, raising=False)
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        Wg, Tg, objs, _ = run(X, W0, T0, 5, True, objective=True, **flags)
        with onchip(True), engine(n, d, k, dtype=np.float32) as e:          # and after a launch of several sweeps
            e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**flags)
            e.sweep(5)
            got[name] = (Wg, Tg, objs, e.objective())
    for name in ('gram', 'direct'):
        assert np.array_equal(got[name][0], got['tracked'][0]) and np.array_equal(got[name][1], got['tracked'][1])
        rel = np.abs(got['tracked'][2] - got[name][2]) / np.abs(got[name][2])
        print('objective left by the kernel vs %s: %s' % (name, ' '.join('%.1e' % r for r in rel)))
        assert rel.max() < 1e-9, (name, rel)
        assert abs(got['tracked'][3] - got[name][3]) < 1e-9 * abs(got[name][3])
        assert abs(got['tracked'][3] - got['tracked'][2][-1]) < 1e-12 * abs(got['tracked'][3])      # 5 sweeps in one launch or in five

@pytest.mark.parametrize('case', ['plain, the rule ends the run', 'plain, never stops', 'topic-model flags', 'regularised',
                                  'reset events inside a chunk', 'max_iter = 3'])
def test_nmf_runs_the_sweep_objective_stop_loop_on_the_device_in_chunks(monkeypatch, tmp_path, case):
    """nmf()'s loop -- sweep, objective, stop rule (nmf.py:377-516) -- as rri_sweep_until: the persistent kernel keeps every
    sweep's objective and ends the launch after the first sweep that satisfies optimization.py:284-291.  Against the same call
    sweep by sweep (RRI_NMF_CHUNK=0): the same number of sweeps, the same objectives, the same bits in W and T."""
    from rri_nmf_amd import nmf as nmf_mod
    n, d, k = 3000, 700, 8
    X = planted_X(n, d, k, seed=141, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=142)
    kw = dict(max_iter=60, eps_stop=1e-3, compute_obj_each_iter=True, dtype=np.float32)
    if case == 'plain, never stops':
        kw.update(eps_stop=-1, max_iter=25)
    elif case == 'topic-model flags':
        X = X / X.sum(1, keepdims=True)
        T0 = T0 / T0.sum(1, keepdims=True)
        W0 = W0 / W0.sum(1, keepdims=True)
        kw.update(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0, eps_stop=1e-2)
    elif case == 'regularised':
        kw.update(reg_w_l1=0.01, reg_t_l1=0.02, reg_w_l2=0.05, reg_t_l2=0.03)
    elif case == 'reset events inside a chunk':
        n, d, k = 600, 200, 4
        X = planted_X(n, d, k, seed=31, dtype=np.float32)
        W0, T0 = scaled_init(X, k, seed=32)
        kw.update(t_row_sum=1.0, reg_w_l1=1e6, max_iter=5, eps_stop=-1)       # every W column is driven to zero: an event per topic (23 resets allowed)
    elif case == 'max_iter = 3':
        kw.update(max_iter=3, eps_stop=-1)
    out = {}
    for chunk in ('1', '0'):
        monkeypatch.setenv('RRI_NMF_CHUNK', chunk)
        log = str(tmp_path / ('onchip_chunk_%s.log' % chunk))
        if os.path.exists(log):
            os.remove(log)
        monkeypatch.setenv('RRI_ONCHIP_LOG', log)
        np.random.seed(0)
        with onchip(True):
            out[chunk] = nmf_mod.nmf(X, k, W_in=W0, T_in=T0, **kw)
        out[chunk]['launches'] = sum(1 for _ in open(log)) if os.path.exists(log) else 0
    a, b = out['1'], out['0']
    print('%s: %d sweeps, %d persistent launches in chunks against %d sweep by sweep, %d resets'
          % (case, len(a['obj_history']), a['launches'], b['launches'], a['n_resets_used']))
    assert len(a['obj_history']) == len(b['obj_history']) == len(a['iter_cputime']) == len(b['iter_cputime'])
    assert a['n_resets_used'] == b['n_resets_used']
    if case == 'plain, the rule ends the run':
        assert 4 < len(a['obj_history']) < kw['max_iter']          # the rule, not max_iter, ended it -- on the device
    if 'reset' not in case:
        assert a['launches'] < b['launches'] or len(a['obj_history']) <= 3
        assert np.array_equal(a['W'], b['W']) and np.array_equal(a['T'], b['T'])
    else:
        assert a['n_resets_used'] >= k
        assert relfro(a['W'], b['W']) < 1e-10 and relfro(a['T'], b['T']) < 1e-10
    assert np.allclose(a['obj_history'], b['obj_history'], rtol=1e-11, atol=0)
    assert np.all(np.diff(a['iter_cputime']) >= 0)

def test_a_chunk_whose_launch_gives_up_costs_one_sweep_launch_by_launch(monkeypatch):
    """rri_sweep_until on a grid that cannot synchronise: the fallback has no stop rule between its sweeps, so the call ends after
    ONE sweep run launch by launch, its objective taken the ordinary way, and nmf() goes on sweep by sweep -- same sweeps, same
    objectives as the call that never used the device loop"""
    from rri_nmf_amd import nmf as nmf_mod
    from rri_nmf_amd.engine import RRIEngine
    n, d, k = 2000, 600, 6
    X = planted_X(n, d, k, seed=151, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=152)
    kw = dict(max_iter=12, eps_stop=-1, compute_obj_each_iter=True, dtype=np.float32)
    monkeypatch.setenv('RRI_ONCHIP_BACKOFF_MS', '0')
    monkeypatch.setenv('RRI_NMF_CHUNK', '0')
    with onchip(True):
        want = nmf_mod.nmf(X, k, W_in=W0, T_in=T0, **kw)
    monkeypatch.setenv('RRI_NMF_CHUNK', '1')
    real, seen = RRIEngine.sweep_until, []

    def giving_up(self, *a):
        os.environ['RRI_ONCHIP_SPIN_LIMIT'] = '0'              # read at every launch: this chunk's grid gives up at its entry
        try:
            res = real(self, *a)
        finally:
            del os.environ['RRI_ONCHIP_SPIN_LIMIT']
        seen.append((res if res is None else (res[0], [bool(np.isnan(v)) for v in res[1]]), self.onchip_fallbacks()))
        return res
    monkeypatch.setattr(RRIEngine, 'sweep_until', giving_up)
    with onchip(True):
        got = nmf_mod.nmf(X, k, W_in=W0, T_in=T0, **kw)
    assert seen[0] == ((1, [True]), 1) and seen[1][0] is None, seen      # one sweep, no objective from the kernel; then not eligible
    assert len(got['obj_history']) == len(want['obj_history']) == 12
    assert np.allclose(got['obj_history'], want['obj_history'], rtol=1e-11, atol=0)
    assert relfro(got['W'], want['W']) < 1e-10 and relfro(got['T'], want['T']) < 1e-10

@pytest.mark.parametrize('case', ['persistent path', 'launch per phase (k = 70)', 'weighted'])
def test_without_an_objective_to_watch_nmf_hands_over_whole_runs(monkeypatch, case):
    """the caller raised the logger's level (the documented way to switch the per-sweep objective off, nmf.py:366): nothing
    happens between the sweeps, and they go to the device in chunks -- same bits as sweep by sweep, iter_cputime of full length"""
    import logging
    from rri_nmf_amd import nmf as nmf_mod
    n, d, k = (2500, 600, 7) if case != 'launch per phase (k = 70)' else (1500, 500, 70)
    X = planted_X(n, d, min(k, 20), seed=161, dtype=np.float32)
    W0, T0 = scaled_init(X, k, seed=162)
    kw = dict(max_iter=14, dtype=np.float32)
    if case == 'weighted':
        kw['W_mat'] = (np.random.RandomState(3).rand(n, d) < 0.3).astype(np.float32)
    old = nmf_mod.logger.level
    nmf_mod.logger.setLevel(logging.WARNING)
    try:
        out = {}
        for chunk in ('1', '0'):
            monkeypatch.setenv('RRI_NMF_CHUNK', chunk)
            with onchip(True):
                out[chunk] = nmf_mod.nmf(X, k, W_in=W0, T_in=T0, **kw)
    finally:
        nmf_mod.logger.setLevel(old)
    a, b = out['1'], out['0']
    assert 'obj_history' not in a and 'obj_history' not in b
    assert len(a['iter_cputime']) == len(b['iter_cputime']) == 14 and np.all(np.diff(a['iter_cputime']) >= 0)
    assert np.array_equal(a['W'], b['W']) and np.array_equal(a['T'], b['T'])
