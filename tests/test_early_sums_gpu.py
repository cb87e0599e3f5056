"""The early-sums schedule (RRI_EARLY_SUMS): the W-sized sums of a topic step -- W (T t^T), the Gram row of the next
topic, its norm -- ride in the grid of the step's pass over X (the early job of k_pass), k_wfin finishes the column after the
pass and reduces the carry in the same launch, and k_trow_early leaves T T[t,:]^T for the next pass.  Unset means on for dense
unweighted handles of the Gram form; RRI_EARLY_SUMS=0 is the chain k_wcol / k_reduce / k_trow_numer.

Every test runs with RRI_ONCHIP=0 and RRI_TROW_SMALL=0 so that small shapes reach this path; layout_info()['early_steps'] counts
the W-column steps that took k_wfin, so a test that means to exercise the schedule asserts that it did.

Tolerances: single steps against the closed form in float64 numpy at 1e-12 in norm and 1e-11 of the largest entry element-wise,
as tests/test_kernel_buckets_gpu.py and tests/test_pass_keep_gpu.py check them; whole sweeps against the float64 oracle at the
2e-9 of tests/test_hip_parity.py (the iteration's own sensitivity), and the two settings of the switch no further apart."""
import ctypes as C
import gc

import numpy as np
import pytest

from conftest import relfro
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu

ENV = 'RRI_EARLY_SUMS'
PARITY_TOL = 2e-9          # tests/test_hip_parity.py: TOL
STEP_TOL = 1e-12


@pytest.fixture(autouse=True)
def launch_per_phase(monkeypatch):
    monkeypatch.setenv('RRI_ONCHIP', '0')
    monkeypatch.setenv('RRI_TROW_SMALL', '0')
    monkeypatch.delenv(ENV, raising=False)


def engine(monkeypatch, setting, *a, **kw):
    """a handle created under RRI_EARLY_SUMS=setting (None: unset); the switch is read by rri_create"""
    from rri_nmf_amd.engine import RRIEngine
    if setting is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, setting)
    e = RRIEngine(*a, **kw)
    monkeypatch.delenv(ENV, raising=False)
    return e


def oracle():
    from oracle import rri_oracle
    return rri_oracle


def stored(X, dtype):
    return np.ascontiguousarray(np.asarray(X).astype(dtype).astype(np.float64))


def problem(n, d, k, seed=0):
    X = planted_X(n, d, min(k, 8) + 1, seed=seed + k, dtype=np.float64)
    W0, T0 = scaled_init(X, k, seed=seed + k + 1)
    return X, W0, T0


# ---- 1. single steps -------------------------------------------------------------------------------------------------------
# 13 x 5: one tile, one column group, two topics; 64 x 256: an exact tile and an exact column group of k_trow_early; 65 x 1025 and
# 71 x 257: one row and one column past them; 200 x 1030, k = 50: the flagship's rank (a wave of the early job holds 12 or 13
# columns: two batches of loads); 1000 x 300: 16 tiles = exactly one tile workgroup of k_wfin, k = 64 one batch of k_trow_early per
# wave and k = 1024 (RRI_MAX_K) sixteen.
STEP_CASES = [(13, 5, 2, np.float32), (64, 256, 4, np.float32), (65, 1025, 5, np.float32), (71, 257, 3, np.float32),
              (200, 1030, 50, np.float32), (200, 1030, 50, np.float64), (1000, 300, 64, np.float32), (1000, 300, 1024, np.float32)]


@pytest.mark.parametrize('n,d,k,dtype', STEP_CASES, ids=['%dx%d-k%d-%s' % (n, d, k, np.dtype(dt).name) for n, d, k, dt in STEP_CASES])
def test_single_steps_against_float64(monkeypatch, n, d, k, dtype):
    """update_T_row(t), update_W_col(t) for t = 0, 1 (the T half of topic 1 takes up what k_wfin left) and k - 1 (the prologue's
    carry), each against the closed form of the step from the factors on the device before it; everything else bit-equal"""
    orc = oracle()
    X, W0, T0 = problem(n, d, k, seed=17)
    Xs = stored(X, dtype)
    with engine(monkeypatch, None, n, d, k, dtype=dtype) as e:
        e.upload_X(X.astype(dtype)); e.set_W(W0); e.set_T(T0); e.set_params()
        assert e.layout_info()['early_sums']
        steps = 0
        for t in sorted({0, 1, k - 1}):
            Wa, Ta = e.get_W(), e.get_T()
            e.update_T_row(t)
            Wb, Tb = e.get_W(), e.get_T()
            wR, nw = orc.residual_products_T(Xs, Wa, Ta, t)
            want = orc.qf_min(-wR, nw, s=None, ub=None)[0]
            err = np.linalg.norm(Tb[t] - want) / np.linalg.norm(want)
            print('T row %d: relative error %.3g' % (t, err))
            assert err <= STEP_TOL, ('T row', t, err)
            assert np.abs(Tb[t] - want).max() <= 10 * STEP_TOL * np.abs(want).max(), ('T row', t, 'element-wise')
            others = np.arange(k) != t
            assert np.array_equal(Tb[others], Ta[others]) and np.array_equal(Wb, Wa)
            e.update_W_col(t)
            Wc, Tc = e.get_W(), e.get_T()
            Rt, nt = orc.residual_products_W(Xs, Wb, Tb, t)
            want = orc.qf_min(-Rt, nt, s=None, ub=None)[0]
            err = np.linalg.norm(Wc[:, t] - want) / np.linalg.norm(want)
            print('W column %d: relative error %.3g' % (t, err))
            assert err <= STEP_TOL, ('W column', t, err)
            assert np.abs(Wc[:, t] - want).max() <= 10 * STEP_TOL * np.abs(want).max(), ('W column', t, 'element-wise')
            assert np.array_equal(Wc[:, others], Wb[:, others]) and np.array_equal(Tc, Tb)
            steps += 1
            assert e.layout_info()['early_steps'] == steps, 'the W half after a T half of the same topic takes k_wfin'
        assert e.n_resets_used == 0


def test_one_topic_takes_the_old_chain(monkeypatch):
    """k = 1: no next topic to carry sums for, nothing to move"""
    n, d, k = 65, 130, 1
    X, W0, T0 = problem(n, d, k, seed=3)
    with engine(monkeypatch, None, n, d, k, dtype=np.float64) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
        assert not e.layout_info()['early_sums']
        e.sweep(2)
        assert e.layout_info()['early_steps'] == 0
        W, T = e.get_W(), e.get_T()
    ref = oracle().nmf(X, k, W_in=W0.copy(), T_in=T0.copy(), max_iter=2, eps_stop=-1)
    assert relfro(W, ref['W']) < PARITY_TOL and relfro(T, ref['T']) < PARITY_TOL


# ---- 2. two sweeps, both settings ----------------------------------------------------------------------------------------------
def two_sweeps(monkeypatch, setting, X, W0, T0, dtype):
    n, d = X.shape
    k = W0.shape[1]
    with engine(monkeypatch, setting, n, d, k, dtype=dtype) as e:
        e.upload_X(X.astype(dtype)); e.set_W(W0); e.set_T(T0); e.set_params()
        e.sweep(2)
        return e.get_W(), e.get_T(), e.objective(), e.layout_info()['early_steps']


@pytest.mark.parametrize('n,d,k', [(200, 1030, 50), (30011, 2503, 4)], ids=['200x1030-k50', '30011x2503-k4'])
def test_two_sweeps_under_both_settings(monkeypatch, n, d, k):
    """30011 x 2503: 157 row blocks of 192 rows in 3 panels (one round of the pass: the early job sits last, beside it), 469 tiles
    on 64 job workgroups of 8 tiles (the last of 5) and 30 tile workgroups of k_wfin"""
    X, W0, T0 = problem(n, d, k, seed=5)
    Xs = stored(X, np.float32)
    on = two_sweeps(monkeypatch, None, X, W0, T0, np.float32)
    off = two_sweeps(monkeypatch, '0', X, W0, T0, np.float32)
    assert on[3] == 2 * k and off[3] == 0, (on[3], off[3])
    ref = oracle().nmf(Xs, k, W_in=W0.copy(), T_in=T0.copy(), max_iter=2, eps_stop=-1)
    for name, got in (('on', on), ('off', off)):
        ew, et = relfro(got[0], ref['W']), relfro(got[1], ref['T'])
        print('%s against the oracle: W %.3g T %.3g' % (name, ew, et))
        assert ew < PARITY_TOL and et < PARITY_TOL, (name, ew, et)
    ew, et = relfro(on[0], off[0]), relfro(on[1], off[1])
    print('on against off: W %.3g T %.3g objective %.3g' % (ew, et, abs(on[2] - off[2]) / abs(off[2])))
    assert ew < PARITY_TOL and et < PARITY_TOL and abs(on[2] - off[2]) <= PARITY_TOL * abs(off[2]), (ew, et)


# ---- 3. halts ------------------------------------------------------------------------------------------------------------------
def drive(e, sweeps):
    """rri_sweep with every event recorded as (kind, topic, sweep, resume_topic) before the engine resolves it; an error status
    raises what the engine raises"""
    from rri_nmf_amd import _capi
    from rri_nmf_amd.engine import Event
    events = []
    done = C.c_int32(0)
    st = e._lib.rri_sweep(e._h, int(sweeps), C.byref(done))
    while st == _capi.RRI_PAUSED:
        ev = Event()
        e._check(e._lib.rri_pending_event(e._h, C.byref(ev)))
        events.append((int(ev.kind), int(ev.topic), int(ev.sweep), int(ev.resume_topic)))
        e._resolve_event()
        st = e._lib.rri_resume(e._h, C.byref(done))
    e._check(st)
    return events


HALTS = {
    # every T row killed by a huge l1 penalty: a reset event per topic, taken by the row checks that ride in the pass
    'T-rows-reset': (dict(t_row_sum=1.0, reg_t_l1=1e6), None, 1),
    # every W column killed: the column verdict of step t is taken by the T-row step of topic t + 1 (from k_wfin's tile sums)
    'W-columns-reset': (dict(t_row_sum=1.0, reg_w_l1=1e6), None, 1),
    # one dead column and an upper bound: the T row of that topic comes out zero (qf_min's c <= 0 branch) and is reset; two sweeps
    'dead-column-reset': (dict(t_row_sum=1.0), 2, 2),
}


@pytest.mark.parametrize('case', list(HALTS))
def test_events_are_the_same_under_both_settings(monkeypatch, case):
    params, dead, sweeps = HALTS[case]
    n, d, k = 200, 1030, 6
    X, W0, T0 = problem(n, d, k, seed=9)
    if dead is not None:
        W0 = W0.copy(); W0[:, dead] = 0.0
    out = {}
    for setting in (None, '0'):
        with engine(monkeypatch, setting, n, d, k, dtype=np.float64) as e:
            e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(**params)
            ev = drive(e, sweeps)
            out[setting] = (ev, e.get_W(), e.get_T(), e.layout_info()['early_steps'])
    on, off = out[None], out['0']
    assert len(off[0]) >= 1 and on[0] == off[0], (on[0], off[0])
    assert off[3] == 0 and on[3] >= 1, (on[3], off[3])
    assert relfro(on[1], off[1]) < STEP_TOL and relfro(on[2], off[2]) < STEP_TOL, (relfro(on[1], off[1]), relfro(on[2], off[2]))


ERRORS = {
    'unbounded': (dict(), ValueError, 'unbounded'),
    'column-sums-to-0': (dict(t_row_sum=1.0, w_row_sum=1.0, reset_topic_method=None), AssertionError, 'sums to 0'),
}


@pytest.mark.parametrize('case', list(ERRORS))
def test_errors_are_the_same_under_both_settings(monkeypatch, case):
    """a dead column without a bound is qf_min's "unbounded"; with bounds and no resets the column assertion fails"""
    params, exc, text = ERRORS[case]
    n, d, k = 200, 1030, 6
    X, W0, T0 = problem(n, d, k, seed=9)
    W0 = W0.copy(); W0[:, 3] = 0.0
    msgs = []
    for setting in (None, '0'):
        with engine(monkeypatch, setting, n, d, k, dtype=np.float64) as e:
            e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(**params)
            with pytest.raises(exc, match=text) as info:
                e.sweep(2)
            msgs.append(str(info.value))
    assert msgs[0] == msgs[1], msgs


# ---- 4. stale early sums -------------------------------------------------------------------------------------------------------
def _set_W(e, rs, state):
    W = e.get_W() * (0.5 + rs.rand(e.n, e.k)); e.set_W(W)


def _set_T(e, rs, state):
    T = e.get_T() * (0.5 + rs.rand(e.k, e.d)); e.set_T(T)


def _set_params(e, rs, state):
    state['params'] = dict(t_row_sum=1.0, reg_w_l2=0.25, reg_t_l1=1e-3)
    e.set_params(**state['params'])


def _lone_T(e, rs, state):
    e.update_T_row(2)


def _lone_W(e, rs, state):
    e.update_W_col(3)


def _dead_column(e, rs, state):
    """the next sweep halts in the middle of topic 2's step (its T row comes out zero), resets it and resumes with the W half"""
    W = e.get_W(); W[:, 2] = 0.0; e.set_W(W)


STALE = {'set_W': _set_W, 'set_T': _set_T, 'set_params': _set_params, 'lone-T-half': _lone_T, 'lone-W-half': _lone_W,
         'resume-in-mid-step': _dead_column}


@pytest.mark.parametrize('op', list(STALE))
def test_next_sweep_after_a_change_equals_a_fresh_handle(monkeypatch, op):
    """a sweep on the early-sums schedule, the change, another sweep: equal at 1e-12 to one sweep of a fresh handle with the switch
    off that starts from the factors the first handle held after the change"""
    n, d, k = 200, 1030, 6
    X, W0, T0 = problem(n, d, k, seed=13)
    state = {'params': dict(t_row_sum=1.0)}
    with engine(monkeypatch, None, n, d, k, dtype=np.float64) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(**state['params'])
        e.sweep(1)
        assert e.layout_info()['early_steps'] == k
        STALE[op](e, np.random.RandomState(1), state)
        W1, T1 = e.get_W(), e.get_T()
        ev = drive(e, 1)
        got = (e.get_W(), e.get_T())
    with engine(monkeypatch, '0', n, d, k, dtype=np.float64) as f:
        f.upload_X(X); f.set_W(W1); f.set_T(T1); f.set_params(**state['params'])
        evf = drive(f, 1)
        want = (f.get_W(), f.get_T())
    assert ev == evf, (ev, evf)
    if op == 'resume-in-mid-step':
        assert len(ev) >= 1 and ev[0][:2] == (1, 2), ev      # RRI_EVENT_RESET_T of topic 2
    ew, et = relfro(got[0], want[0]), relfro(got[1], want[1])
    print('%s: W %.3g T %.3g' % (op, ew, et))
    assert ew < STEP_TOL and et < STEP_TOL, (op, ew, et)


# ---- 5. other paths and memory ---------------------------------------------------------------------------------------------------
OTHER = {
    'topic-model': (dict(), dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0), {}),
    'fix_W': (dict(), dict(fix_W=True), {}),
    'fix_T': (dict(), dict(fix_T=True), {}),
    'residual-schedule': (dict(schedule='residual'), dict(), {}),
    'k_trow_small': (dict(), dict(), {'RRI_TROW_SMALL': '1'}),
}


@pytest.mark.parametrize('case', list(OTHER))
def test_other_paths_keep_their_bits(monkeypatch, case):
    kw, params, env = OTHER[case]
    n, d, k = 203, 141, 5
    X, W0, T0 = problem(n, d, k, seed=21)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    res = []
    for setting in (None, '0'):
        with engine(monkeypatch, setting, n, d, k, dtype=np.float32, **kw) as e:
            e.upload_X(X.astype(np.float32)); e.set_W(W0); e.set_T(T0); e.set_params(**params)
            e.sweep(2)
            res.append((e.get_W(), e.get_T(), e.objective()))
            assert e.layout_info()['early_steps'] == 0
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


def test_device_memory_comes_back(monkeypatch):
    """the five arrays of the schedule are the handle's (dev_alloc): there while it lives, gone with it; none with the switch off"""
    from rri_nmf_amd.engine import device_memory
    n, d, k = 300, 130, 5
    X, W0, T0 = problem(n, d, k, seed=2)
    gc.collect()
    base = device_memory()
    alive = {}
    for setting in (None, '0'):
        e = engine(monkeypatch, setting, n, d, k, dtype=np.float32)
        try:
            e.upload_X(X.astype(np.float32)); e.set_W(W0); e.set_T(T0); e.set_params()
            ready = device_memory()
            e.sweep(2)
            assert device_memory() == ready, 'a sweep allocates nothing'
            alive[setting] = (ready[0] - base[0], ready[1] - base[1])
        finally:
            e.close()
        assert device_memory() == base
    assert alive[None][0] == alive['0'][0] + 5 and alive[None][1] > alive['0'][1], alive
