"""The read-only pass keeps a fixed part of a large X in the Infinity Cache (RRI_PASS_CACHE_MB, pass_keep in rri_hip.hip): kept
row blocks take default-policy loads, the others non-temporal ones.  A load policy cannot change a value, so whatever the
capacity says -- nothing kept, the default, ONE row block kept, all of X kept -- W, T and the objective after two sweeps are the
same bits; a difference is a row block walked twice, not at all, or by the wrong rows.

Shapes: ragged (n odd, d not a multiple of the 16-byte vector nor of a workgroup's columns) in every storage type, on both sides
of 1024 workgroups (up to there a row block is interleaved chunks of 8 rows, above it a contiguous range), and a small X that a
fractional capacity below its size puts into the streaming regime.  One case goes against float64 numpy: the closed form of single
topic steps at the tolerance test_kernel_buckets_gpu.py holds the launch-per-phase steps to (1e-12, element-wise ten times that).

uint8 counts (8-byte loads, 2048 columns per workgroup, one byte per element in the budget of pass_keep) take part with row and
column scales set: 6011 x 4099 on the interleaved side, in row blocks of 48 rows, and 286721 x 2056 on the contiguous side, the
smallest X that the LDS cap of 560 rows puts above 1024 workgroups.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = 'RRI_PASS_CACHE_MB'


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def geometry(n, d, k, dtype, info):
    """(bytes of X as the pass counts them, bytes of one row block, default-policy bytes of the chain of a topic step): the
    terms of pass_keep, from the geometry the handle reports"""
    es = np.dtype(dtype).itemsize
    vn = 8 if np.dtype(dtype) == np.uint8 else 16 // es     # uint8 counts take 8-byte loads, every other store 16-byte ones
    ld = -(-d // vn) * vn
    nwb = -(-n // 64)
    chain = 8 * (k * n + 2 * info['nrb'] * ld + 2 * info['npanels'] * n + 2 * k * ld + 2 * nwb * (k + 2))
    return n * ld * es, info['rpb'] * ld * es, chain


def settings(n, d, k, dtype):
    """the four capacities of the bit-identity check, in MB: 0 (all of X streams), None (the default), one that leaves room for a
    single row block beside the chain, one that holds all of X"""
    with engine(n, d, k, dtype=dtype) as e:
        info = e.layout_info()
    xb, block, chain = geometry(n, d, k, dtype, info)
    assert info['nrb'] >= 3 and xb > chain + 2 * block, 'the shape must leave blocks unkept: %r' % (info,)
    one = (chain + 1.5 * block) / 1e6
    return info, {'nothing kept': '0', 'default': None, 'one row block kept': repr(one), 'all of X kept': repr(4.0 * (xb + chain) / 1e6)}


def two_sweeps(monkeypatch, n, d, k, dtype, load, cap, W0, T0, onchip=None):
    if cap is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, cap)                    # read when the handle is created
    if onchip is not None:
        monkeypatch.setenv('RRI_ONCHIP', onchip)
    with engine(n, d, k, dtype=dtype) as e:
        load(e)
        e.set_W(W0); e.set_T(T0); e.set_params()
        assert not e.onchip_info()[0], 'this test is about the launch-per-phase pass'
        e.sweep(2)
        out = e.get_W(), e.get_T(), e.objective()
    monkeypatch.delenv(ENV, raising=False)
    return out


def assert_same_bits(res):
    names = list(res)
    W0, T0, o0 = res[names[0]]
    assert np.isfinite(W0).all() and np.isfinite(T0).all() and W0.max() > 0 and T0.max() > 0
    for nm in names[1:]:
        W, T, o = res[nm]
        assert np.array_equal(T, T0), '%s against %s: T differs in rows %s' % (nm, names[0], np.flatnonzero(np.any(T != T0, axis=1)))
        assert np.array_equal(W, W0), '%s against %s: W differs in %d rows, first %s' % (
            nm, names[0], int(np.any(W != W0, axis=1).sum()), np.flatnonzero(np.any(W != W0, axis=1))[:8])
        assert o == o0, '%s against %s: objective %r / %r' % (nm, names[0], o, o0)


def host_problem(n, d, k, seed):
    rs = np.random.RandomState(seed)
    X = (rs.rand(n, 3).astype(np.float32) @ rs.rand(3, d).astype(np.float32)) + 0.01 * rs.rand(n, d).astype(np.float32)
    a = float(np.sqrt(X[:2000].mean() / k))
    return X, a * rs.rand(n, k), a * rs.rand(k, d)


def scales_of(n, d, seed):
    """row and column scales of a uint8 X, log-uniform over 0.1 .. 10"""
    rs = np.random.RandomState(seed)
    return 10.0 ** rs.uniform(-1, 1, n), 10.0 ** rs.uniform(-1, 1, d)


def count_problem(n, d, k, seed):
    """the X of host_problem as counts 0..255 (40 on average) under non-trivial scales, the float64 matrix a uint8 handle
    factorises, (C * s) * r, and a start scaled to it"""
    X, _, _ = host_problem(n, d, k, seed)
    C = np.minimum(np.round(40.0 * X / X.mean()), 255.0).astype(np.uint8)
    r, s = scales_of(n, d, seed + 1)
    X64 = np.ascontiguousarray((C.astype(np.float64) * s) * r[:, None])
    rs = np.random.RandomState(seed + 2)
    a = float(np.sqrt(X64[:2000].mean() / k))
    return C, r, s, X64, a * rs.rand(n, k), a * rs.rand(k, d)


def load_counts(C, r, s):
    def load(e):
        e.upload_X(C)
        e.set_X_scales(r, s)
    return load


LARGE = {'fp32-30011x2503': (30011, 2503, np.float32), 'fp64-20011x2503': (20011, 2503, np.float64),
         'fp16-60013x2503': (60013, 2503, np.float16),
         # 25 MB of counts, but 3 panels x 126 row blocks of 48 rows, the last of 11: no uint8 handle of a few MB leaves the 32-row
         # minimum of rri_create; the chain of a topic step takes 9 MB, a row block 197 KB
         'u8-6011x4099': (6011, 4099, np.uint8)}


@pytest.mark.parametrize('case', list(LARGE))
def test_large_ragged_X_same_bits_at_every_capacity(monkeypatch, case):
    """300-400 MB of X (uint8: 25 MB of counts with row and column scales), fewer than 1024 workgroups: interleaved row chunks"""
    n, d, dtype = LARGE[case]
    k = 4
    info, caps = settings(n, d, k, dtype)
    assert info['interleaved'] and info['npanels'] * info['nrb'] <= 1024, info
    if dtype == np.uint8:
        assert (info['npanels'], info['rpb'], info['nrb']) == (3, 48, 126), info
        C, r, s, _, W0, T0 = count_problem(n, d, k, seed=5)
        load = load_counts(C, r, s)
    else:
        X, W0, T0 = host_problem(n, d, k, seed=5)
        Xs = X.astype(dtype)
        load = lambda e: e.upload_X(Xs)
    res = {nm: two_sweeps(monkeypatch, n, d, k, dtype, load, cap, W0, T0) for nm, cap in caps.items()}
    assert_same_bits(res)


def test_contiguous_row_blocks_same_bits_at_every_capacity(monkeypatch):
    """more than 1024 workgroups (the LDS cap on the rows of a workgroup decides: 560 rows x 10 column panels): a row block is a
    contiguous range of rows.  2.4 GB of fp32 made on the device and bound."""
    import torch
    n, d, k, dtype = 60007, 10004, 3, np.float32          # (a bound X has no pad columns: d is a multiple of 4, not of a panel)
    info, caps = settings(n, d, k, dtype)
    assert not info['interleaved'] and info['npanels'] * info['nrb'] > 1024, info
    g = torch.Generator(device='cuda:0').manual_seed(3)
    X = torch.rand(n, 3, device='cuda:0', generator=g) @ torch.rand(3, d, device='cuda:0', generator=g)
    X += 0.01 * torch.rand(n, d, device='cuda:0', generator=g)
    torch.cuda.synchronize()                 # the handle's stream does not wait for torch's
    rs = np.random.RandomState(7)
    a = float(np.sqrt(float(X[:2000].mean()) / k))
    W0, T0 = a * rs.rand(n, k), a * rs.rand(k, d)
    res = {nm: two_sweeps(monkeypatch, n, d, k, dtype, lambda e: e.bind_X_device(X.data_ptr(), X.stride(0)), cap, W0, T0)
           for nm, cap in caps.items()}
    assert_same_bits(res)


def test_small_X_streamed_by_a_fractional_capacity_same_bits(monkeypatch):
    """14 MB of X: plain loads throughout by default; a capacity of a few MB, a fraction of one, streams it but for one row
    block.  RRI_ONCHIP=0: the launch-per-phase schedule, whatever the register-resident sweep would take."""
    n, d, k, dtype = 3001, 1203, 5, np.float32
    monkeypatch.setenv('RRI_ONCHIP', '0')
    info, caps = settings(n, d, k, dtype)
    xb, block, chain = geometry(n, d, k, dtype, info)
    assert float(caps['one row block kept']) * 1e6 < xb and float(caps['one row block kept']) % 1.0 != 0.0
    X, W0, T0 = host_problem(n, d, k, seed=9)
    res = {nm: two_sweeps(monkeypatch, n, d, k, dtype, lambda e: e.upload_X(X), cap, W0, T0, onchip='0') for nm, cap in caps.items()}
    assert_same_bits(res)


def steps_against_float64(monkeypatch, tag, n, d, k, dtype, caps, load, Xs, W0, T0, tol=1e-12):
    from oracle import rri_oracle as orc
    for nm in ('one row block kept', 'default'):
        if caps[nm] is None:
            monkeypatch.delenv(ENV, raising=False)
        else:
            monkeypatch.setenv(ENV, caps[nm])
        with engine(n, d, k, dtype=dtype) as e:
            load(e); e.set_W(W0); e.set_T(T0); e.set_params()
            for t in (0, k - 1):
                Wa, Ta = e.get_W(), e.get_T()
                e.update_T_row(t)
                Wb, Tb = e.get_W(), e.get_T()
                wR, nw = orc.residual_products_T(Xs, Wa, Ta, t)
                want = orc.qf_min(-wR, nw, s=None, ub=None)[0]
                err = np.linalg.norm(Tb[t] - want) / np.linalg.norm(want)
                print('%s%s: T row %d relative error %.3g' % (tag, nm, t, err))
                assert err <= tol, (tag, nm, 'T row', t, err)
                assert np.abs(Tb[t] - want).max() <= 10 * tol * np.abs(want).max(), (tag, nm, 'T row', t, 'element-wise')
                e.update_W_col(t)
                Wc = e.get_W()
                Rt, nt = orc.residual_products_W(Xs, Wb, Tb, t)
                want = orc.qf_min(-Rt, nt, s=None, ub=None)[0]
                err = np.linalg.norm(Wc[:, t] - want) / np.linalg.norm(want)
                print('%s%s: W column %d relative error %.3g' % (tag, nm, t, err))
                assert err <= tol, (tag, nm, 'W column', t, err)
                assert np.abs(Wc[:, t] - want).max() <= 10 * tol * np.abs(want).max(), (tag, nm, 'W column', t, 'element-wise')
                others = np.arange(k) != t
                assert np.array_equal(Wc[:, others], Wb[:, others]) and np.array_equal(Tb[others], Ta[others])
    monkeypatch.delenv(ENV, raising=False)


def test_topic_steps_of_a_partly_kept_X_against_float64(monkeypatch):
    """fp32 30011 x 2503, and uint8 counts with scales at 6011 x 4099 (row blocks of 48 rows in 3 panels), with one row block kept
    and with the default capacity: update_T_row(t) and update_W_col(t) against the closed form of the step in float64 numpy, from
    the factors on the device before it -- the check and the tolerance (1e-12 in norm, 1e-11 of the largest entry element-wise)
    of test_kernel_buckets_gpu.check_steps for the launch-per-phase steps"""
    n, d, dtype, k = 30011, 2503, np.float32, 4
    _, caps = settings(n, d, k, dtype)
    X, W0, T0 = host_problem(n, d, k, seed=5)
    Xs = np.ascontiguousarray(X.astype(dtype).astype(np.float64))
    steps_against_float64(monkeypatch, '', n, d, k, dtype, caps, lambda e: e.upload_X(X), Xs, W0, T0)
    n, d, dtype = LARGE['u8-6011x4099']
    _, caps = settings(n, d, k, dtype)
    C, r, s, X64, W0, T0 = count_problem(n, d, k, seed=5)
    steps_against_float64(monkeypatch, 'uint8 6011 x 4099, ', n, d, k, dtype, caps, load_counts(C, r, s), X64, W0, T0)


def test_contiguous_row_blocks_of_counts_same_bits_and_single_steps(monkeypatch):
    """uint8 above 1024 workgroups: 286721 x 2056 is 2 panels, and 1024 / 2 = 512 blocks give ceil(286721 / 512) = 561 rows, which
    the LDS cap cuts to 560: 513 row blocks, the last of ONE row, 1026 workgroups, each walking a contiguous range of rows.  It
    is the smallest X that reaches the cap (560 * 512 * 2056 bytes; every other panel count needs more): 589 MB of counts made on
    the device and bound.  Same bits of W, T and the objective at the four capacities; then, as float64 on the host cannot hold
    this X, update_T_row(0) and update_W_col(0) against the closed form with the two products of X formed in torch.float64 on
    the device in chunks of 8192 rows, X^T w = s * sum_chunks C^T (r * w) and X t = r * (C (s * t)), and qf_min on the host:
    1e-12 in norm, ten times that of the largest entry element-wise."""
    import torch
    from oracle import rri_oracle as orc
    n, d, k, dtype = 286721, 2056, 3, np.uint8
    info, caps = settings(n, d, k, dtype)
    assert (info['npanels'], info['rpb'], info['nrb']) == (2, 560, 513) and n - 512 * 560 == 1, info
    assert not info['interleaved'] and info['npanels'] * info['nrb'] > 1024, info
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(11)
    C = torch.empty(n, d, dtype=torch.uint8, device=dev)
    CH = 8192
    for a in range(0, n, CH):                   # Poisson-like small counts with three planted topics, 2.5 per entry on average
        rows = min(CH, n - a)
        lam = torch.rand(rows, 3, device=dev, generator=g) @ torch.rand(3, d, device=dev, generator=g) * (2.5 / 0.75)
        C[a:a + rows] = torch.poisson(lam, generator=g).clamp_(max=255).to(torch.uint8)
    del lam
    torch.cuda.synchronize()                    # the handle's stream does not wait for torch's
    r, s = scales_of(n, d, 13)
    rs = np.random.RandomState(7)
    mean = float(C[:2000].double().mean()) * float(r[:2000].mean()) * float(s.mean())
    a = float(np.sqrt(mean / k))
    W0, T0 = a * rs.rand(n, k), a * rs.rand(k, d)

    def load(e):
        e.bind_X_device(C.data_ptr(), d)
        e.set_X_scales(r, s)
    res = {nm: two_sweeps(monkeypatch, n, d, k, dtype, load, cap, W0, T0) for nm, cap in caps.items()}
    assert_same_bits(res)

    rt, st = torch.as_tensor(r, device=dev), torch.as_tensor(s, device=dev)

    def Xt_times(w):                            # s * sum_chunks C^T (r * w)
        w = torch.as_tensor(w, device=dev) * rt
        acc = torch.zeros(d, dtype=torch.float64, device=dev)
        for a in range(0, n, CH):
            acc += C[a:a + CH].double().T @ w[a:a + CH]
        return (st * acc).cpu().numpy()

    def X_times(t):                             # r * (C (s * t))
        t = torch.as_tensor(t, device=dev) * st
        out = torch.empty(n, dtype=torch.float64, device=dev)
        for a in range(0, n, CH):
            out[a:a + CH] = C[a:a + CH].double() @ t
        return (rt * out).cpu().numpy()
    tol, t = 1e-12, 0
    with engine(n, d, k, dtype=dtype) as e:
        load(e); e.set_W(W0); e.set_T(T0); e.set_params()
        e.update_T_row(t)
        Wb, Tb = e.get_W(), e.get_T()
        # w^T (X - sum_{j != t} w_j t_j) and ||w||^2: oracle.residual_products_T with the product of X taken on the device
        others = np.arange(k) != t
        w = W0[:, t]
        wR = Xt_times(w) - (w @ W0[:, others]) @ T0[others]
        want = orc.qf_min(-wR, float(w @ w), s=None, ub=None)[0]
        err = np.linalg.norm(Tb[t] - want) / np.linalg.norm(want)
        print('uint8 286721 x 2056, contiguous row blocks: T row %d relative error %.3g' % (t, err))
        assert err <= tol, ('T row', t, err)
        assert np.abs(Tb[t] - want).max() <= 10 * tol * np.abs(want).max(), ('T row', t, 'element-wise')
        assert np.array_equal(Wb, W0) and np.array_equal(Tb[others], T0[others])
        e.update_W_col(t)
        Wc = e.get_W()
        tt = Tb[t]
        Rt = X_times(tt) - Wb[:, others] @ (Tb[others] @ tt)
        want = orc.qf_min(-Rt, float(tt @ tt), s=None, ub=None)[0]
        err = np.linalg.norm(Wc[:, t] - want) / np.linalg.norm(want)
        print('uint8 286721 x 2056, contiguous row blocks: W column %d relative error %.3g' % (t, err))
        assert err <= tol, ('W column', t, err)
        assert np.abs(Wc[:, t] - want).max() <= 10 * tol * np.abs(want).max(), ('W column', t, 'element-wise')
        assert np.array_equal(Wc[:, others], Wb[:, others]) and np.array_equal(e.get_T(), Tb)
    monkeypatch.delenv(ENV, raising=False)
