"""The packed row loop of the read-only pass (RRI_PASS_ROWS_PK, rri_kernels.hpp) at the edges of its chunk loop, and the geometry
rri_create gives a dense fp32 handle of the Gram form (at most 512 rows per workgroup; RRI_PASS_PK_GEOM, diagnostics).

The shape, flagged-tile, kept / streamed, bound-X and float64 tests below were designed around a row-by-row refill of the record's
registers inside that loop, which was measured and NOT built: they pin the loop as it is, at the edges any rewrite of
it has -- trip counts, lanes and waves without columns, a workgroup that falls back to the fp32 loop beside ones that do not.
Only the last two tests cover code of their own commit: the switch and the default rows per workgroup.

The yardstick is, as in test_xpack_gpu.py, the same handle under RRI_X_PACK=0: W, T and the objective after two sweeps are EQUAL
BIT FOR BIT -- the geometry does not depend on RRI_X_PACK, so the partial sums keep their order.

A workgroup has 32 rows at the small sizes, up to four chunks of 8 rows:
n = 8 exactly one chunk, 9 a second chunk of one row, 16 / 17 the same one chunk further, 32 a full workgroup, 33 and 40 a last
row block of one chunk, 71 three blocks; d = 4 one lane with columns, 257 a second wave with one lane, 1030 a second column group
and waves without columns.  Values as in test_xpack_gpu.py: 30 % zeros, denormals, both ends of the window.
Then: a flagged tile in the first and in the last chunk of a workgroup (the whole workgroup takes the fp32 loop, its neighbours
the packed one), kept and streamed row blocks mixed, a bound X with row stride > d inside NaN bands, single topic steps over
the copy against float64 numpy at 1e-12, and the switch: rows per workgroup and chunk order as asked for, rounded and capped, the
same bits as the fp32 pass of the same geometry, and no effect on a float64 handle.  RRI_ONCHIP=0 throughout."""
import numpy as np
import pytest

import ld_cases as lc
import test_pass_keep_gpu as pk
import test_xpack_gpu as xg

pytestmark = pytest.mark.gpu

NS = (8, 9, 16, 17, 32, 33, 40, 71)
DS = (4, 257, 1030)
K = 2


def chunks_of_block(info, n, rb):
    """the 8-row chunks of X that row block rb walks, in its order, as the kernel's grow() has them"""
    cpb, nq = info['rpb'] // 8, -(-n // 8)
    qs = [q * info['nrb'] + rb if info['interleaved'] else rb * cpb + q for q in range(cpb)]
    return [q for q in qs if q < nq]


@pytest.mark.parametrize('d', DS)
@pytest.mark.parametrize('n', NS)
def test_edge_shapes_same_bits_as_the_fp32_pass(monkeypatch, n, d):
    X, W0, T0 = xg.problem(n, d, K, seed=100 + 7 * n + d)
    X, base = xg.plant(X, seed=n + d)
    res = {}
    res['fp32'], info0 = xg.two_sweeps(monkeypatch, '0', n, d, K, lambda e: e.upload_X(X), W0, T0)
    res['packed'], info1 = xg.two_sweeps(monkeypatch, '1', n, d, K, lambda e: e.upload_X(X), W0, T0)
    assert info1['rpb'] == 32, info1
    assert not info0['x_pack'] and info1['x_pack'] and info1['x_pack_base'] == base, (info0, info1, base)
    assert info1['x_pack_tiles'] == xg.tiles_of(n, info1) and info1['x_pack_flagged'] == 0, info1
    pk.assert_same_bits(res)


@pytest.mark.parametrize('where', ['first chunk of a workgroup', 'last chunk of a workgroup'])
def test_a_flagged_tile_sends_its_workgroup_alone_to_the_fp32_loop(monkeypatch, where):
    """71 x 1030: three row blocks x two column groups.  One element below the window in the first / the last chunk the middle row
    block walks, in the second / the first column group: that workgroup runs the fp32 loop, the other five the packed one"""
    n, d = 71, 1030
    monkeypatch.setenv('RRI_ONCHIP', '0')
    with xg.engine(n, d, K, dtype=np.float32) as e:
        info = e.layout_info()
    assert info['rpb'] == 32 and info['nrb'] == 3 and info['npanels'] == 2, info
    mine = chunks_of_block(info, n, 1)
    assert len(mine) >= 2, (info, mine)
    first = where.startswith('first')
    q, col = (mine[0], 1027) if first else (mine[-1], 5)
    X, W0, T0 = xg.problem(n, d, K, seed=41)
    X, base = xg.plant(X, seed=9, below=(8 * q + (3 if first else 0), col))
    res = {}
    res['fp32'], _ = xg.two_sweeps(monkeypatch, '0', n, d, K, lambda e: e.upload_X(X), W0, T0)
    res['packed'], info1 = xg.two_sweeps(monkeypatch, '1', n, d, K, lambda e: e.upload_X(X), W0, T0)
    assert info1['x_pack'] and info1['x_pack_base'] == base and info1['x_pack_flagged'] == 1, info1
    pk.assert_same_bits(res)


def test_kept_and_streamed_row_blocks_mixed(monkeypatch):
    """135 x 1030, five row blocks of 32 rows (the last of one chunk): a fractional RRI_PASS_CACHE_MB keeps one of them (default-policy
    loads in the packed loop) and streams the others (non-temporal ones); and with nothing kept"""
    n, d = 135, 1030
    monkeypatch.setenv('RRI_ONCHIP', '0')
    info, caps = pk.settings(n, d, K, np.float32)
    assert info['rpb'] == 32 and info['nrb'] == 5, info
    X, W0, T0 = xg.problem(n, d, K, seed=43)
    X, base = xg.plant(X, seed=10)
    for nm in ('one row block kept', 'nothing kept'):
        res = {}
        res['fp32'], _ = xg.two_sweeps(monkeypatch, '0', n, d, K, lambda e: e.upload_X(X), W0, T0, cap=caps[nm])
        res['packed'], info1 = xg.two_sweeps(monkeypatch, '1', n, d, K, lambda e: e.upload_X(X), W0, T0, cap=caps[nm])
        assert info1['x_pack'] and info1['x_pack_base'] == base and info1['x_pack_flagged'] == 0, info1
        pk.assert_same_bits(res)


def test_bound_X_with_a_row_stride_above_d_inside_nan_bands(monkeypatch):
    import torch
    name = lc.cases(store='fp32', widths=(2,), pads=(1,))[0]
    c = lc.CASES[name]
    X, base = xg.plant(lc.case_matrix(c), seed=12)
    g = lc.guarded(torch, X, c.ld, c.c0, device='cuda:0')
    torch.cuda.synchronize()
    rs = np.random.RandomState(2)
    a = float(np.sqrt(X.mean() / K))
    W0, T0 = a * rs.rand(c.n, K), a * rs.rand(K, c.d)
    load = lambda e: e.bind_X_device(g.ptr, g.ld)
    res = {}
    res['fp32'], _ = xg.two_sweeps(monkeypatch, '0', c.n, c.d, K, load, W0, T0)
    res['packed'], info = xg.two_sweeps(monkeypatch, '1', c.n, c.d, K, load, W0, T0)
    assert info['x_pack'] and info['x_pack_base'] == base and info['x_pack_flagged'] == 0, info
    pk.assert_same_bits(res)
    g.check('the bound X')


@pytest.mark.parametrize('shape', [(17, 257), (71, 1030)])
def test_topic_steps_over_the_copy_against_float64(monkeypatch, shape):
    """update_T_row(t) and update_W_col(t) over the copy against the closed form of the step in float64 numpy, at the tolerance of
    test_xpack_gpu.py (1e-12 in norm, ten times that element-wise)"""
    from oracle import rri_oracle as orc
    n, d = shape
    k, tol = 3, 1e-12
    X, W0, T0 = xg.problem(n, d, k, seed=51 + n)
    X, _ = xg.plant(X, seed=13)
    Xs = np.ascontiguousarray(X.astype(np.float64))
    monkeypatch.setenv('RRI_ONCHIP', '0')
    monkeypatch.setenv(xg.ENV, '1')
    with xg.engine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
        e.sweep(1)                      # the first sweep builds the copy
        assert e.layout_info()['x_pack'] and e.layout_info()['x_pack_flagged'] == 0
        for t in (0, k - 1):
            Wa, Ta = e.get_W(), e.get_T()
            e.update_T_row(t)
            Wb, Tb = e.get_W(), e.get_T()
            wR, nw = orc.residual_products_T(Xs, Wa, Ta, t)
            want = orc.qf_min(-wR, nw, s=None, ub=None)[0]
            err = np.linalg.norm(Tb[t] - want) / np.linalg.norm(want)
            print('T row %d relative error %.3g' % (t, err))
            assert err <= tol, ('T row', t, err)
            assert np.abs(Tb[t] - want).max() <= 10 * tol * np.abs(want).max(), ('T row', t, 'element-wise')
            e.update_W_col(t)
            Wc = e.get_W()
            Rt, nt = orc.residual_products_W(Xs, Wb, Tb, t)
            want = orc.qf_min(-Rt, nt, s=None, ub=None)[0]
            err = np.linalg.norm(Wc[:, t] - want) / np.linalg.norm(want)
            print('W column %d relative error %.3g' % (t, err))
            assert err <= tol, ('W column', t, err)
            assert np.abs(Wc[:, t] - want).max() <= 10 * tol * np.abs(want).max(), ('W column', t, 'element-wise')
    monkeypatch.delenv(xg.ENV, raising=False)


GEOM = 'RRI_PASS_PK_GEOM'


@pytest.mark.parametrize('geom, rpb, il', [('48c', 48, False), ('48i', 48, True), ('40i', 48, True), ('16', 16, True), ('100000c', 560, False)])
def test_the_geometry_switch_is_honoured_and_changes_no_bit_against_the_fp32_pass(monkeypatch, geom, rpb, il):
    """200 x 1030 (default: 32 rows, interleaved): rows rounded up to 16 and capped by the LDS limit, the chunk order as asked for
    (no letter: by the workgroup count), and W, T, objective of the packed pass equal to those of the fp32 pass made under the
    same switch"""
    n, d = 200, 1030
    X, W0, T0 = xg.problem(n, d, K, seed=61)
    X, base = xg.plant(X, seed=14, below=(199, 1029))
    monkeypatch.setenv(GEOM, geom)
    res = {}
    res['fp32'], info0 = xg.two_sweeps(monkeypatch, '0', n, d, K, lambda e: e.upload_X(X), W0, T0)
    res['packed'], info1 = xg.two_sweeps(monkeypatch, '1', n, d, K, lambda e: e.upload_X(X), W0, T0)
    monkeypatch.delenv(GEOM, raising=False)
    for info in (info0, info1):
        assert info['rpb'] == rpb and info['nrb'] == -(-n // rpb) and info['interleaved'] == il, (geom, info)
    assert info1['x_pack'] and info1['x_pack_base'] == base and info1['x_pack_flagged'] == 1, info1
    pk.assert_same_bits(res)


def test_default_rows_per_workgroup_and_handles_the_switch_leaves_alone(monkeypatch):
    """the geometry is decided by rri_create from the shape alone (no X needed): a dense fp32 Gram-form handle large enough for the
    LDS cap to decide walks 512 rows per workgroup, with RRI_X_PACK=0 as well; a float64 handle of that shape keeps its own rows,
    and the switch does not touch it"""
    n, d = 600000, 1024
    monkeypatch.setenv('RRI_ONCHIP', '0')
    infos = {}
    for name, dtype, pack, geom in (('fp32', np.float32, None, None), ('fp32, no copy', np.float32, '0', None),
                                    ('fp32, 448 rows', np.float32, None, '448c'), ('fp64', np.float64, None, None),
                                    ('fp64, switch set', np.float64, None, '448c')):
        for env, val in ((xg.ENV, pack), (GEOM, geom)):
            if val is None:
                monkeypatch.delenv(env, raising=False)
            else:
                monkeypatch.setenv(env, val)
        with xg.engine(n, d, K, dtype=dtype) as e:
            infos[name] = e.layout_info()
    monkeypatch.delenv(xg.ENV, raising=False)
    monkeypatch.delenv(GEOM, raising=False)
    assert infos['fp32']['rpb'] == 512 and infos['fp32, no copy']['rpb'] == 512, infos
    assert infos['fp32, 448 rows']['rpb'] == 448 and not infos['fp32, 448 rows']['interleaved'], infos
    assert infos['fp64']['rpb'] > 512 and infos['fp64, switch set']['rpb'] == infos['fp64']['rpb'], infos
