"""The register-resident persistent sweep (k_onchip_sweeps) against the float64 oracle on both sides of every limit of its host
geometry, and at every verdict of the halting rules -- the in-loop copies of rri_onchip_kernels.hpp that
tests/test_halt_rules_cpu.py cannot see included.  The cases, the second wording of the geometry and the yardstick are
tests/onchip_cases.py (checked without a GPU by tests/test_onchip_cases_cpu.py).

Every edge case: the library's eligibility equals the restated one; sweep(1), then sweep(2) on the same handle (the second call
crosses a sweep boundary and continues a run); after each call W, T and the resets against the oracle on X as stored, and the
objective the kernel left behind against 1/2 ||Xs - W T||^2 recomputed on the host from the device's own factors.  An eligible
case must have RUN as persistent launches with no fallback -- a launch that gave up and was rerun launch by launch fails the test
instead of passing as a persistent run -- and a case past a limit must have launched none: the same comparison then covers the
hand-over to the launch-per-phase schedule right at the limit.

Bounds (relative Frobenius, conftest.relfro): 2e-9 for k <= 22, what test_against_the_cpu_oracle holds this kernel to after five
sweeps.  Beyond k = 22 the start is the oracle's own state two sweeps on and the bound is max(2e-9, 20 x control), control = the
oracle against itself with every entry of that start one ulp up over the same sweeps (onchip_cases.control / bound).  The measured
error and the control of every case are printed; profiles/r12_onchip_edges.log is one full run."""
import numpy as np
import pytest

import onchip_cases as oc
from conftest import relfro

pytestmark = pytest.mark.gpu

EDGES = oc.edge_cases(256)          # ids from the 256-CU table: stable whatever the device reports
VERDICTS = oc.verdict_cases()


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


@pytest.fixture(scope='module')
def n_cu():
    with engine(64, 8, 2) as e:
        return int(e.layout_info()['n_cu'])


def locate(name, got, want, g, rows):
    """the workgroup (W) or the column group and worker slice (T) of the largest element-wise error"""
    i, j = np.unravel_index(np.argmax(np.abs(got - want)), want.shape)
    rows_wg = g.get('rows_wg', 0)
    if rows:        # W: row i belongs to a workgroup
        return '%s[%d, %d]: device %.17g, oracle %.17g -- workgroup %s (rows_wg %s)' % (
            name, i, j, got[i, j], want[i, j], i // rows_wg if rows_wg else '-', rows_wg or '-')
    return '%s[%d, %d]: device %.17g, oracle %.17g -- column group %d, worker slice %d' % (
        name, i, j, got[i, j], want[i, j], j // 256, j // 32)


def compare(tag, e, Xs, flags, k, ref_state, ctl, g, objective=True):
    W, T = e.get_W(), e.get_T()
    Wr, Tr, resets = ref_state
    ew, et = relfro(W, Wr), relfro(T, Tr)
    tol = oc.bound(k, ctl)
    half_xsq = 0.5 * float(np.sum(Xs * Xs))
    obj, host = (e.objective(), oc.objective_of(Xs, W, T, flags)) if objective else (0.0, 0.0)
    print('%s: W %.2e T %.2e | control %s bound %.1e | resets %d (oracle %d)%s'
          % (tag, ew, et, 'none (k <= 22)' if k <= oc.SMALL_K else '%.2e' % ctl if ctl is not None else 'n/a', tol,
             e.n_resets_used, resets,
             ' | objective off by %.1e of 1/2 ||X||^2' % (abs(obj - host) / half_xsq if half_xsq > 0 else 0.0) if objective else ''))
    assert e.n_resets_used == resets, (tag, e.n_resets_used, resets, e.reset_log)
    assert ew < tol and et < tol, '%s: W %.3e, T %.3e, bound %.1e\n  %s\n  %s' % (
        tag, ew, et, tol, locate('W', W, Wr, g, True), locate('T', T, Tr, g, False))
    # both sides from the same factors: what is left is the cross terms the kernel kept on the way
    assert abs(obj - host) <= 1e-10 * half_xsq, (tag, obj, host, half_xsq)


@pytest.mark.parametrize('name', [c.name for c in EDGES])
def test_edge(monkeypatch, n_cu, name):
    here = {c.name: c for c in oc.edge_cases(n_cu)}
    if name not in here:
        assert name in oc.edge_dropped(n_cu)
        pytest.skip('%d CUs: the case has no shape (more column slices than workgroups)' % n_cu)
    c = here[name]
    g = oc.geometry(c.n, c.d, c.k, c.store, oc.projected(c.flags), n_cu)
    assert g['eligible'] == c.expect_eligible
    monkeypatch.setenv('RRI_ONCHIP', '1')
    X, Xs, W0, T0 = oc.edge_problem(c)
    marks = (1, 3)
    ref = oc.oracle_run(Xs, W0, T0, marks, c.flags)
    assert ref.error is None, ref.error
    ctl = oc.control(Xs, W0, T0, marks, c.flags, ref) if c.k > oc.SMALL_K else {1: None, 3: None}
    with engine(c.n, c.d, c.k, dtype=oc.STORES[c.store]) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**c.flags)
        eligible, before = e.onchip_info()
        assert eligible == c.expect_eligible, 'the library says %s, the restated geometry %s: %r' % (eligible, c.expect_eligible, g)
        done = 0
        for call, sweeps in enumerate((1, 2)):
            e.sweep(sweeps)
            done += sweeps
            launches, fallbacks = e.onchip_info()[1] - before, e.onchip_fallbacks()
            if c.expect_eligible:
                assert fallbacks == 0, ('%s: %d persistent launch(es) gave up and were rerun launch by launch -- the device was shared '
                                        'with another process\'s grids; this is no persistent run' % (name, fallbacks))
                assert launches >= call + 1, (name, launches)
            else:
                assert launches == 0 and fallbacks == 0, (name, launches, fallbacks)
            compare('%s after %d sweep(s)' % (name, done), e, Xs, c.flags, c.k, ref.states[done], ctl[done], g)


@pytest.mark.parametrize('v', VERDICTS, ids=[v.name for v in VERDICTS])
def test_verdict(monkeypatch, v):
    monkeypatch.setenv('RRI_ONCHIP', '1')
    X, Xs, W0, T0 = oc.verdict_problem(v)
    marks = (v.sweeps,)
    np.random.seed(0)
    ref = oc.oracle_run(Xs, W0, T0, marks, v.flags)
    assert (ref.error is not None) == ('error' in v.expect)
    with engine(oc.VN, oc.VD, v.k, dtype=oc.STORES[v.store]) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0), e.set_params(**v.flags)
        eligible, before = e.onchip_info()
        assert eligible
        np.random.seed(0)
        if ref.error is not None:
            kind, word = ref.error
            with pytest.raises(kind, match=word):
                e.sweep(v.sweeps)
        else:
            e.sweep(v.sweeps)
        launches, fallbacks = e.onchip_info()[1] - before, e.onchip_fallbacks()
        assert fallbacks == 0, '%s: a persistent launch gave up -- the device was shared; this is no persistent run' % v.name
        assert launches >= 1, launches
        # the same topics reset, in the same order, by the same rule
        assert [(kind, t) for kind, t, _ in e.reset_log] == [(kind, t) for kind, t, _ in ref.log], (e.reset_log, ref.log)
        if ref.error is not None:
            print('%s: %s(%s) after %d reset(s), %d persistent launch(es)' % (v.name, ref.error[0].__name__, ref.error[1], len(ref.log), launches))
            assert e.n_resets_used == len(ref.log), (e.n_resets_used, ref.log)
            return
        ctl = None
        if v.k > oc.SMALL_K:
            np.random.seed(0)
            ctl = oc.control(Xs, W0, T0, marks, v.flags, ref)[v.sweeps]
        g = oc.geometry(oc.VN, oc.VD, v.k, v.store, oc.projected(v.flags), 256)
        compare(v.name, e, Xs, v.flags, v.k, ref.states[v.sweeps], ctl, g, objective=False)
