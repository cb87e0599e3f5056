"""The read-only pass of a dense fp32 handle streams a lossless 28-bit copy of X (RRI_X_PACK; rri_xpack.hpp, xpack_ensure in
rri_hip.hip): three low bytes and a 4-bit code of the top byte per element, tiles with an element outside the window of fifteen
top bytes flagged and read as fp32.  The copy decodes to the bits of X and the row loop does the same arithmetic in the same
order, so the yardstick is the same handle with RRI_X_PACK=0 and W, T and the objective after two sweeps are EQUAL BIT FOR BIT; a
difference is a wrong record, a wrong byte of one, a stale copy, or a tile that should have been flagged.

RRI_ONCHIP=0 throughout: the launch-per-phase schedule, whatever the register-resident sweep would take.

Shapes, the smallest that reach every edge: 13 x 5 (one partial chunk, a partial lane), 71 x 257 (a one-column second panel, a ragged
last chunk), 200 x 1030 (a second column group), the two shapes of test_pass_keep_gpu.py on either side of 1024 workgroups with
its fractional RRI_PASS_CACHE_MB (interleaved and contiguous row blocks; kept and streamed blocks mixed), and one bound X with a
row stride > d inside NaN guard bands (ld_cases.py).
Values: 30 % exact zeros, denormals, a normal number with top byte 0, elements at the first and the last top byte of the window
with both values of exponent bit 0, one element just below the window (exactly one flagged tile), one negative element (one
more), and an X whose every tile is flagged (no copy at all)."""
import numpy as np
import pytest

import ld_cases as lc
import test_pass_keep_gpu as pk

pytestmark = pytest.mark.gpu

ENV = 'RRI_X_PACK'


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def window_base(X):
    """the first top byte of the window of X, as the format defines it"""
    hi = np.ascontiguousarray(X, dtype=np.float32).view(np.uint32) >> 24
    hi = hi[(hi >= 1) & (hi <= 0x7e)]
    return max(1, int(hi.max()) - 14) if hi.size else 1


def plant(X, seed, below=None, negative=None, zeros=True):
    """X with 30 % exact zeros and the special values of the format at seeded places; below / negative: (row, column) of one
    element just below the window / of one negative element.  Returns (X, base)."""
    rs = np.random.RandomState(seed)
    X = np.array(X, dtype=np.float32)
    if zeros:
        X[rs.rand(*X.shape) < 0.3] = 0.0
    base = window_base(X)
    assert base > 1
    top = base + 14
    specials = [0x00000001, 0x007fffff, 0x00812345,                       # denormals; a normal number whose top byte is 0
                base << 24 | 0x00000001, base << 24 | 0x00800000 | 0x2a5a5a,        # the first top byte, exponent bit 0 clear / set
                top << 24 | 0x00000000, top << 24 | 0x00800000 | 0x000001]          # the last one (no larger than 2^(2 top - 126))
    bits = X.view(np.uint32).reshape(-1)
    keep = [i for i in (below, negative) if i is not None]
    taken = {r * X.shape[1] + c for r, c in keep}
    places = [int(p) for p in rs.choice(bits.size, size=min(bits.size, 3 * len(specials)), replace=False) if int(p) not in taken]
    for p, s in zip(places, specials * 2):
        bits[p] = s
    if below is not None:
        X[below] = np.array([(base - 1) << 24 | 0x00923456], dtype=np.uint32).view(np.float32)[0]
    if negative is not None:
        X[negative] = -0.375
    assert window_base(X) == base, 'the planted values must not move the window'
    return X, base


def problem(n, d, k, seed):
    rs = np.random.RandomState(seed)
    X = (rs.rand(n, 3).astype(np.float32) @ rs.rand(3, d).astype(np.float32)) + 0.01 * rs.rand(n, d).astype(np.float32)
    a = float(np.sqrt(X.mean() / k))
    return X, a * rs.rand(n, k), a * rs.rand(k, d)


def two_sweeps(monkeypatch, pack, n, d, k, load, W0, T0, cap=None, sweeps=2):
    """(W, T, objective), layout_info of a handle created under RRI_X_PACK=pack (None: unset)"""
    monkeypatch.setenv('RRI_ONCHIP', '0')
    for name, val in ((ENV, pack), (pk.ENV, cap)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    with engine(n, d, k, dtype=np.float32) as e:
        load(e)
        e.set_W(W0); e.set_T(T0); e.set_params()
        assert not e.onchip_info()[0]
        e.sweep(sweeps)
        out = e.get_W(), e.get_T(), e.objective()
        info = e.layout_info()
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.delenv(pk.ENV, raising=False)
    return out, info


def tiles_of(n, info):
    return -(-n // 8) * info['npanels']


SMALL = {
    # name: (n, d, k, below, negative, flagged tiles)
    '13x5 one partial chunk, a partial lane': (13, 5, 2, None, None, 0),
    '71x257 one-column second panel, ragged last chunk': (71, 257, 3, (70, 256), None, 1),
    '200x1030 second column group': (200, 1030, 4, (199, 1029), (3, 500), 2),
}


@pytest.mark.parametrize('case', list(SMALL))
def test_small_shapes_same_bits_as_the_fp32_pass(monkeypatch, case):
    n, d, k, below, negative, flagged = SMALL[case]
    X, W0, T0 = problem(n, d, k, seed=11 + n)
    X, base = plant(X, seed=n, below=below, negative=negative)
    res = {}
    res['fp32'], info0 = two_sweeps(monkeypatch, '0', n, d, k, lambda e: e.upload_X(X), W0, T0)
    res['packed'], info1 = two_sweeps(monkeypatch, '1', n, d, k, lambda e: e.upload_X(X), W0, T0)
    assert not info0['x_pack'] and info0['x_pack_tiles'] == 0, info0
    assert info1['x_pack'] and info1['x_pack_base'] == base, (info1, base)
    assert info1['x_pack_tiles'] == tiles_of(n, info1) and info1['x_pack_flagged'] == flagged, info1
    pk.assert_same_bits(res)


def test_every_tile_flagged_means_no_copy(monkeypatch):
    n, d, k = 200, 1030, 4
    X, W0, T0 = problem(n, d, k, seed=3)
    X, _ = plant(X, seed=1)
    X[::8, 0] = 1e-30            # far below the window, in every 8-row chunk of both column groups
    X[::8, 1024] = 1e-30
    res = {}
    res['fp32'], _ = two_sweeps(monkeypatch, '0', n, d, k, lambda e: e.upload_X(X), W0, T0)
    res['packed'], info = two_sweeps(monkeypatch, '1', n, d, k, lambda e: e.upload_X(X), W0, T0)
    assert not info['x_pack'] and info['x_pack_flagged'] == info['x_pack_tiles'] == tiles_of(n, info), info
    pk.assert_same_bits(res)


def test_interleaved_row_blocks_kept_and_streamed_mixed(monkeypatch):
    """fp32 30011 x 2503 (fewer than 1024 workgroups: interleaved chunks) with test_pass_keep_gpu's fractional capacity: one row
    block kept, the others streamed -- and with nothing kept"""
    n, d, k = 30011, 2503, 4
    info, caps = pk.settings(n, d, k, np.float32)
    assert info['interleaved']
    X, W0, T0 = pk.host_problem(n, d, k, seed=5)
    X, base = plant(X, seed=2, below=(30010, 2502))
    for nm in ('one row block kept', 'nothing kept'):
        res = {}
        res['fp32'], _ = two_sweeps(monkeypatch, '0', n, d, k, lambda e: e.upload_X(X), W0, T0, cap=caps[nm])
        res['packed'], info1 = two_sweeps(monkeypatch, '1', n, d, k, lambda e: e.upload_X(X), W0, T0, cap=caps[nm])
        assert info1['x_pack'] and info1['x_pack_base'] == base and info1['x_pack_flagged'] == 1, info1
        pk.assert_same_bits(res)


def test_contiguous_row_blocks_auto_builds_the_copy(monkeypatch):
    """fp32 60007 x 10004 made on the device and bound (more than 1024 workgroups: contiguous row blocks; 2.4 GB, so the switch
    left unset builds the copy), one row block kept"""
    import torch
    n, d, k = 60007, 10004, 3
    info, caps = pk.settings(n, d, k, np.float32)
    assert not info['interleaved']
    g = torch.Generator(device='cuda:0').manual_seed(3)
    X = torch.rand(n, 3, device='cuda:0', generator=g) @ torch.rand(3, d, device='cuda:0', generator=g)
    X += 0.01 * torch.rand(n, d, device='cuda:0', generator=g)
    X *= (torch.rand(n, d, device='cuda:0', generator=g) >= 0.3)         # 30 % exact zeros
    X[17, 9] = 1e-40; X[60006, 10003] = 2e-39; X[4001, 5000] = 1.1754944e-38      # denormals, the smallest normal number
    X[n // 2, d // 2] = 1e-12                                                        # below the window of values around 1
    torch.cuda.synchronize()
    rs = np.random.RandomState(7)
    a = float(np.sqrt(float(X[:2000].mean()) / k))
    W0, T0 = a * rs.rand(n, k), a * rs.rand(k, d)
    load = lambda e: e.bind_X_device(X.data_ptr(), X.stride(0))
    res = {}
    res['fp32'], info0 = two_sweeps(monkeypatch, '0', n, d, k, load, W0, T0, cap=caps['one row block kept'])
    res['packed'], info1 = two_sweeps(monkeypatch, None, n, d, k, load, W0, T0, cap=caps['one row block kept'])
    assert not info0['x_pack'] and info1['x_pack'] and info1['x_pack_flagged'] == 1, (info0, info1)
    pk.assert_same_bits(res)


def test_bound_X_with_a_row_stride_above_d_inside_nan_bands(monkeypatch):
    import torch
    name = lc.cases(store='fp32', widths=(2,), pads=(1,))[0]
    c = lc.CASES[name]
    k = 3
    X, base = plant(lc.case_matrix(c), seed=4, below=(c.n - 1, c.d - 1))
    g = lc.guarded(torch, X, c.ld, c.c0, device='cuda:0')
    torch.cuda.synchronize()
    rs = np.random.RandomState(1)
    a = float(np.sqrt(X.mean() / k))
    W0, T0 = a * rs.rand(c.n, k), a * rs.rand(k, c.d)
    load = lambda e: e.bind_X_device(g.ptr, g.ld)
    res = {}
    res['fp32'], _ = two_sweeps(monkeypatch, '0', c.n, c.d, k, load, W0, T0)
    res['packed'], info = two_sweeps(monkeypatch, '1', c.n, c.d, k, load, W0, T0)
    assert info['x_pack'] and info['x_pack_base'] == base and info['x_pack_flagged'] == 1, info
    pk.assert_same_bits(res)
    g.check('the bound X')


@pytest.mark.parametrize('how', ['upload_X of another matrix', 'tf-idf scaling in place'])
def test_a_changed_X_gets_a_new_copy(monkeypatch, how):
    """sweep, change X, sweep again: the same bits as a fresh handle on the new X started from the same factors, and as the same
    sequence of calls under RRI_X_PACK=0"""
    n, d, k = 200, 1030, 4
    X1, W0, T0 = problem(n, d, k, seed=21)
    X1, base1 = plant(X1, seed=5)
    X2 = plant(problem(n, d, k, seed=22)[0] * np.float32(2.0 ** -31), seed=6)[0]        # another window altogether
    monkeypatch.setenv('RRI_ONCHIP', '0')

    def change(e):
        if how.startswith('upload'):
            e.upload_X(X2)
        else:
            e.preprocess(tfidf=True)

    def sequence(pack):
        monkeypatch.setenv(ENV, pack)
        with engine(n, d, k, dtype=np.float32) as e:
            e.upload_X(X1); e.set_W(W0); e.set_T(T0); e.set_params()
            e.sweep(1)
            mid = e.get_W(), e.get_T()
            infos = [e.layout_info()]
            change(e)
            e.sweep(1)
            infos.append(e.layout_info())
            return mid, (e.get_W(), e.get_T(), e.objective()), infos

    mid, packed, infos = sequence('1')
    _, plain, _ = sequence('0')
    assert infos[0]['x_pack'] and infos[0]['x_pack_base'] == base1 and infos[1]['x_pack'], infos
    if how.startswith('upload'):
        assert infos[1]['x_pack_base'] != base1, 'the new X has another window: %r' % (infos,)
    monkeypatch.setenv(ENV, '1')
    with engine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X1)
        change(e)
        e.set_W(mid[0]); e.set_T(mid[1]); e.set_params()
        e.sweep(1)
        fresh = e.get_W(), e.get_T(), e.objective()
        assert e.layout_info()['x_pack_base'] == infos[1]['x_pack_base']
    monkeypatch.delenv(ENV, raising=False)
    pk.assert_same_bits({'fresh handle': fresh, 'handle whose X changed': packed, 'the same calls, fp32 pass': plain})


def test_the_copy_is_released_with_the_handle_and_a_small_handle_makes_none(monkeypatch):
    from rri_nmf_amd.engine import device_memory
    n, d, k = 200, 1030, 4
    X, W0, T0 = problem(n, d, k, seed=8)
    monkeypatch.setenv('RRI_ONCHIP', '0')
    start = device_memory()
    used = {}
    for pack in ('0', '1', None):
        if pack is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, pack)
        with engine(n, d, k, dtype=np.float32) as e:
            e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
            e.sweep(1)
            used[pack] = device_memory(), e.layout_info()['x_pack']
        assert device_memory() == start, (pack, start, device_memory())
    assert used['1'][1] and not used['0'][1] and not used[None][1], used
    tiles = -(-n // 8) * 2
    assert used['1'][0][0] == used['0'][0][0] + 3 and used['1'][0][1] == used['0'][0][1] + tiles * (4 * 7168 + 1) + 4, used
    assert used[None][0] == used['0'][0], 'with the switch unset a small handle allocates no copy: %r' % (used,)


def test_topic_steps_over_the_copy_against_float64(monkeypatch):
    """fp32 30011 x 2503, one row block kept, the passes over the copy: update_T_row(t) and update_W_col(t) against the closed
    form of the step in float64 numpy, at the tolerance of test_pass_keep_gpu.py (1e-12 in norm, ten times that element-wise)"""
    from oracle import rri_oracle as orc
    n, d, k = 30011, 2503, 4
    tol = 1e-12
    _, caps = pk.settings(n, d, k, np.float32)
    X, W0, T0 = pk.host_problem(n, d, k, seed=5)
    X, _ = plant(X, seed=2, below=(30010, 2502))
    Xs = np.ascontiguousarray(X.astype(np.float64))
    monkeypatch.setenv('RRI_ONCHIP', '0')
    monkeypatch.setenv(ENV, '1')
    monkeypatch.setenv(pk.ENV, caps['one row block kept'])
    with engine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
        e.sweep(1)                      # the first sweep builds the copy
        assert e.layout_info()['x_pack'] and e.layout_info()['x_pack_flagged'] == 1
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
    monkeypatch.delenv(ENV, raising=False)
    monkeypatch.delenv(pk.ENV, raising=False)


def test_a_first_sweep_with_T_fixed_does_not_settle_the_question(monkeypatch):
    """sweeps with T fixed run the whole-sweep W half and read no pass: they build no copy, and the first ordinary sweep after the
    parameters change builds it -- the same bits as the same calls under RRI_X_PACK=0"""
    n, d, k = 200, 1030, 4
    X, W0, T0 = problem(n, d, k, seed=31)
    X, base = plant(X, seed=7)
    monkeypatch.setenv('RRI_ONCHIP', '0')

    def sequence(pack):
        monkeypatch.setenv(ENV, pack)
        with engine(n, d, k, dtype=np.float32) as e:
            e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(fix_T=True)
            e.sweep(1)
            first = e.layout_info()
            e.set_params()
            e.sweep(2)
            return (e.get_W(), e.get_T(), e.objective()), first, e.layout_info()

    packed, first, later = sequence('1')
    plain, _, _ = sequence('0')
    monkeypatch.delenv(ENV, raising=False)
    assert not first['x_pack'] and first['x_pack_tiles'] == 0, first
    assert later['x_pack'] and later['x_pack_base'] == base and later['x_pack_flagged'] == 0, later
    pk.assert_same_bits({'fp32': plain, 'packed': packed})
