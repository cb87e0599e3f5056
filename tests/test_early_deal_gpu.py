"""Where the early-sums job sits in the grid of the fused pass (RRI_EARLY_DEAL, rri_early_deal.hpp), and k_wfin's one
batch of loads.  Helpers, tolerances and the environment (RRI_ONCHIP=0, RRI_TROW_SMALL=0) are tests/test_early_sums_gpu.py's and
tests/test_early_sums_routes_gpu.py's, by import; every case asserts layout_info()['early_steps'].

RRI_EARLY_DEAL moves workgroups and changes no sum: the same workgroup computes the same tiles in the same order.  So W, T and the
objective after two sweeps from a fixed start are compared BIT FOR BIT between RRI_EARLY_DEAL=0 (the job's workgroups in one run
behind the first round of the pass) and 1 (dealt through the rest of the grid), for fp32 under both packed copies and for
float64, and each against the float64 oracle at the 2e-9 of the early-sums suites.  A map that loses or doubles a row block is an
error of order one; one that hands a job workgroup another index leaves rows of the dot unwritten.

  test_dealt_equals_contiguous     the `above` shapes of test_early_sums_routes_gpu (the pass has more than 4 n_cu own workgroups,
                                   RRI_PASS_PK_GEOM=16c / 16i) and three more of the same kind, chosen by what lies behind `first`:
                                   fewer own workgroups than the job has (stride 0: dealing is the contiguous run), as many (stride
                                   1, nothing left over), and 3 nblocks + 1 (stride 3, ONE own workgroup behind the last of the
                                   job).  d = 130, k = 5: P = ceil(n / 16), and the last row block holds one row.
                                   (float64 takes no RRI_PASS_PK_GEOM: its pass has one round at these sizes, the job sits last and
                                   the map is the identity -- the float64 build of the pass with the map in it, nothing more.)
  test_dealt_under_rotation_behind_a_gram_job
                                   d = 4100: five panels and a Gram-row job of two column slices (2 k workgroups) in front of the
                                   grid, RRI_PASS_ROT=3 with a partial last group of 8 own workgroups, the job dealt with stride 2:
                                   `bid = blockIdx.x - job.nblocks` before the map, the rotation and the kept blocks on own indices.
  test_wfin_batch                  k_wfin: the halt word, nt, wn, dot and up to 16 partials of y in one batch of loads, the rest by
                                   ordered_sum_acc.  npanels = 1, 8, 9, 16 and 17 (d = 130, 8 * 1024 - 3, 8 * 1024 + 5, 16 * 1024 -
                                   7, 16 * 1024 + 5) at n = 200: a last tile of 8 rows (rows past n read row n - 1) and twelve waves
                                   without a tile.  The new column is compared bit for bit with RRI_EARLY_SUMS=0's, at a state where
                                   the two schedules are defined to agree: what differs between them is the ORDER of the sums T
                                   T[t,:]^T and ||T[t,:]||^2, so the state makes every such sum exact -- W0 and T0 are small dyadic
                                   numbers, column t of W0 is dead and reg_t_l1 < 0 with t_row_sum = 1, so that the T half leaves
                                   T[t,:] = 1 (qf_min's bounded branch) -- and y, the only inexact term, is ordered_sum<8>'s in both.
                                   Then against the closed form in float64 at the step tolerance of the early-sums suites."""
import numpy as np
import pytest

import test_early_sums_routes_gpu as er
import test_pass_keep_gpu as pk
import test_xpack_gpu as xg
from test_early_sums_gpu import ENV as EARLY_ENV, STEP_TOL, engine, launch_per_phase, oracle, stored  # noqa: F401 (launch_per_phase: autouse)

pytestmark = pytest.mark.gpu

ENV = 'RRI_EARLY_DEAL'

DEAL_SHAPES = ('less', 'equal', 'three-and-one')


def deal_shape(name, n_cu):
    """(n, d, k, P, stride): d = 130 is one panel, P = ceil(n / 16) own workgroups of the pass, F = 4 n_cu of them in front of the
    job's n_cu / 4 workgroups; at 256 CUs n = 17377, 17393, 19457"""
    F, e = 4 * n_cu, max(n_cu, 4) // 4
    behind, s = {'less': (e - 1, 0), 'equal': (e, 1), 'three-and-one': (3 * e + 1, 3)}[name]
    P = F + behind
    return 16 * (P - 1) + 1, 130, 5, P, s


def nsplit2_shape(n_cu):
    """(n, d, k, P, e_blocks, stride): five panels of 1024 columns, nsplit = 2; a tile workgroup of the job per tile"""
    F = 4 * n_cu
    nrb = (F + 2 * (max(n_cu, 4) // 4)) // 5 + 3
    n = 16 * (nrb - 1) + 4
    P, e = 5 * nrb, min((n + 63) // 64, max(n_cu, 4) // 4)
    return n, 4100, 4, P, e, (P - F) // e


def stride_of(info, n):
    """early_deal_stride restated on what the handle reports"""
    P, F = info['npanels'] * info['nrb'], 4 * info['n_cu']
    e = max(1, min((n + 63) // 64, max(info['n_cu'], 4) // 4))
    return (P - F) // e if P > F else 0


def two_sweeps(monkeypatch, deal, X, W0, T0, ref, dtype, geom=None, rot=None, pack=None, tag=''):
    """a handle created under RRI_EARLY_DEAL=deal: two sweeps on the schedule against the oracle; ((W, T, objective), layout_info)"""
    n, d = X.shape
    k = W0.shape[1]
    for name, val in ((ENV, deal), ('RRI_PASS_PK_GEOM', geom), ('RRI_PASS_ROT', rot), (xg.ENV, pack)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    with engine(monkeypatch, None, n, d, k, dtype=dtype) as e:
        for name in (ENV, 'RRI_PASS_PK_GEOM', 'RRI_PASS_ROT', xg.ENV):
            monkeypatch.delenv(name, raising=False)
        e.upload_X(X.astype(dtype)); e.set_W(W0); e.set_T(T0); e.set_params()
        assert e.layout_info()['early_sums']
        out = er.two_sweeps_on_the_schedule(e, k, ref, tag)
        info = e.layout_info()
        assert info['early_steps'] == 2 * k and info['early_steps'] > 0
        assert info['early_deal'] == (deal != '0') and info['early_stride'] == (stride_of(info, n) if deal != '0' else 0), (tag, info)
        assert e.n_resets_used == 0
    return out, info


def same_bits(res):
    names = list(res)
    for name in names[1:]:
        for what, a, b in zip(('W', 'T', 'objective'), res[names[0]], res[name]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), '%s differs between %s and %s' % (what, names[0], name)


def dealt_and_contiguous(monkeypatch, n, d, k, geom, want_P, want_stride, rot=None, seed=23):
    """the X of tests/test_pass_keep_gpu.host_problem, which both packed copies take (no element far below the others); fp32 values,
    so the float64 handle stores the same matrix and one run of the oracle serves the three stores"""
    X, W0, T0 = pk.host_problem(n, d, k, seed=seed)
    Xs = stored(X, np.float32)
    ref = er.reference(Xs, k, W0, T0)
    for store, dtype, pack in (('fp32, 28-bit copy', np.float32, '1'), ('fp32, 26-bit copy', np.float32, '2'), ('float64', np.float64, None)):
        f32 = dtype == np.float32
        res = {}
        for deal in ('0', '1'):
            tag = '%s, %s=%s: ' % (store, ENV, deal)
            res[deal], info = two_sweeps(monkeypatch, deal, X, W0, T0, ref, dtype, geom=geom, rot=rot, pack=pack, tag=tag)
            if f32:
                assert info['rpb'] == 16 and info['npanels'] * info['nrb'] == want_P and info['interleaved'] == (geom == '16i'), (tag, info)
                assert info['x_pack_bits'] == {'1': 28, '2': 26}[pack], (tag, info)
                assert info['early_stride'] == (want_stride if deal == '1' else 0), (tag, info, want_stride)
            else:
                assert info['npanels'] * info['nrb'] <= 4 * info['n_cu'] and info['early_stride'] == 0, (tag, info)
        same_bits(res)


A1 = [(name, geom) for name in er.A1_INSIDE for geom in ('16c', '16i')]
CASES = [('A1', name, geom) for name, geom in A1] + [('deal', name, geom) for name in DEAL_SHAPES for geom in ('16c', '16i')]


@pytest.mark.parametrize('kind,name,geom', CASES, ids=['%s-%s' % (nm, g) for _, nm, g in CASES])
def test_dealt_equals_contiguous(monkeypatch, kind, name, geom):
    n_cu = er.device_n_cu(monkeypatch)
    if kind == 'A1':
        n, d, k, P, side = er.a1_shape(name, n_cu)
        assert side == 'above'
        e = max(1, min((n + 63) // 64, max(n_cu, 4) // 4))
        s = (P - 4 * n_cu) // e
    else:
        n, d, k, P, s = deal_shape(name, n_cu)
    dealt_and_contiguous(monkeypatch, n, d, k, geom, P, s)


def test_dealt_under_rotation_behind_a_gram_job(monkeypatch):
    n_cu = er.device_n_cu(monkeypatch)
    n, d, k, P, e, s = nsplit2_shape(n_cu)
    assert s >= 1 and P % 8 != 0, 'the job is dealt and the last group of 8 own workgroups is partial'
    dealt_and_contiguous(monkeypatch, n, d, k, '16c', P, s, rot='3', seed=29)


# ---- k_wfin: one batch of loads ---------------------------------------------------------------------------------------------------
WFIN_D = {1: 130, 8: 8 * 1024 - 3, 9: 8 * 1024 + 5, 16: 16 * 1024 - 7, 17: 16 * 1024 + 5}
BOUNDED = dict(t_row_sum=1.0, reg_t_l1=-0.01, reset_topic_method=None)


def exact_state(n, d, k, t, seed):
    """X: fp32 values in [0, 1); W0, T0: multiples of 2^-10 and 2^-4 below 4, column t of W0 dead.  Every sum over them, and over
    the row of ones the T half of topic t leaves, is exact in float64 in any order."""
    rs = np.random.RandomState(seed)
    X = rs.rand(n, d).astype(np.float32)
    W0 = rs.randint(0, 4, size=(n, k)).astype(np.float64) * 2.0 ** -10
    T0 = rs.randint(0, 4, size=(k, d)).astype(np.float64) * 2.0 ** -4
    W0[:, t] = 0.0
    return X, W0, T0


@pytest.mark.parametrize('npanels', sorted(WFIN_D))
def test_wfin_batch(monkeypatch, npanels):
    n, d, k, t = 200, WFIN_D[npanels], 3, 1
    X, W0, T0 = exact_state(n, d, k, t, seed=43 + npanels)
    Xs = np.ascontiguousarray(X.astype(np.float64))
    orc = oracle()
    cols = {}
    for setting in (None, '0'):
        with engine(monkeypatch, setting, n, d, k, dtype=np.float32) as e:
            e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(**BOUNDED)
            info = e.layout_info()
            assert info['npanels'] == npanels and info['early_sums'] == (setting is None), info
            e.update_T_row(t)
            Wb, Tb = e.get_W(), e.get_T()
            assert (Tb[t] == 1.0).all() and np.array_equal(Wb, W0), 'the T half leaves a row of ones (the bounded branch)'
            e.update_W_col(t)
            Wc, Tc = e.get_W(), e.get_T()
            assert e.layout_info()['early_steps'] == (1 if setting is None else 0), (setting, e.layout_info())
            assert np.array_equal(Tc, Tb) and np.array_equal(np.delete(Wc, t, axis=1), np.delete(Wb, t, axis=1))
            assert e.n_resets_used == 0
        Rt, nt = orc.residual_products_W(Xs, Wb, Tb, t)
        assert nt == float(d)
        want = orc.qf_min(-Rt, nt, s=None, ub=None)[0]
        assert (want > 0.0).all(), 'every row takes the closed form, none is clipped'
        er.close('%s=%s, %d panels: W column %d' % (EARLY_ENV, setting, npanels, t), Wc[:, t], want)
        cols[setting] = Wc[:, t]
    assert STEP_TOL == 1e-12
    assert np.array_equal(cols[None], cols['0']), ('k_wfin against k_wcol', float(np.abs(cols[None] - cols['0']).max()))
