"""The read-only pass of a dense fp32 handle streams a lossless 26-bit copy of X (RRI_X_PACK=2, or unset where the 28-bit copy
would be built and few elements are exceptions; rri_xnarrow.hpp, xnarrow_build in rri_hip.hip): 23 mantissa bits and a 3-bit code
into a book of the seven most frequent exponent bytes per element, code 7 an entry of the record's exception list.  Window, base
and tile flags are those of the 28-bit copy.  The copy decodes to the bits of X and the row loop does the same arithmetic in the
same order, so the yardstick is the same handle under RRI_X_PACK=0 and under =1: W, T and the objective after two sweeps are EQUAL
BIT FOR BIT; a difference is a wrong mantissa or code bit, a wrong or missing exception, a stale copy or book, or a stale byte of
the exception map.

Helpers, shapes and planted values are those of test_xpack_gpu.py (by import).  On top of them: records built by hand -- one with
no exception beside one where every element is one; one with exactly 64 and one with 65 (a second round of the entry loop), with
positions 0 and 2047 (the last lane's last element) and the last element of the ragged last panel among them."""
import numpy as np
import pytest

import ld_cases as lc
import test_pass_keep_gpu as pk
import test_xpack_gpu as xg

pytestmark = pytest.mark.gpu

ENV = xg.ENV


def books_of(X, base, pad_zeros=0):
    """(book, exceptions) as the format defines them: the exponent bytes of the window ordered by count (ties to the smaller
    value), the first seven; the elements of the window outside them.  pad_zeros: zeros of the padding columns the handle counts"""
    bits = np.ascontiguousarray(X, dtype=np.float32).view(np.uint32).reshape(-1)
    hist = np.bincount((bits[bits >> 31 == 0] >> 23).astype(np.int64), minlength=256)
    hist[0] += pad_zeros
    cand = [e for e in range(256) if (e >> 1) == 0 or base <= (e >> 1) <= base + 14]
    cand.sort(key=lambda e: (-int(hist[e]), e))
    return cand[:7], int(sum(hist[e] for e in cand[7:]))


def exceptions_of_record(X, book, q, p):
    """elements of record (8-row chunk q, 256-column panel p) whose exponent byte is outside the book"""
    blk = np.ascontiguousarray(X[8 * q:8 * q + 8, 256 * p:256 * p + 256]).view(np.uint32)
    return int((~np.isin(blk >> 23, book)).sum())


def with_exponent(rs, shape, eb):
    """seeded fp32 values of exponent byte eb, every mantissa bit in play"""
    return (np.uint32(eb << 23) | rs.randint(0, 1 << 23, size=shape).astype(np.uint32)).view(np.float32)


def three_ways(monkeypatch, n, d, k, load, W0, T0, cap=None, packs=('0', '1', '2')):
    res, infos = {}, {}
    for pack in packs:
        res['RRI_X_PACK=%s' % pack], infos[pack] = xg.two_sweeps(monkeypatch, pack, n, d, k, load, W0, T0, cap=cap)
    return res, infos


def check_infos(infos, n, base, flagged, X=None, pad_zeros=0):
    i0, i1, i2 = infos['0'], infos['1'], infos['2']
    assert not i0['x_pack'] and i0['x_pack_bits'] == 0 and i0['x_pack_book'] == [], i0
    assert i1['x_pack'] and i1['x_pack_bits'] == 28 and i1['x_pack_book'] == [], i1
    assert i2['x_pack'] and i2['x_pack_bits'] == 26, i2
    for name in ('x_pack_base', 'x_pack_flagged', 'x_pack_tiles', 'rpb', 'nrb', 'npanels', 'interleaved'):
        assert i2[name] == i1[name], (name, i1, i2)            # one geometry, one window, the same flagged tiles
    assert i2['x_pack_base'] == base and i2['x_pack_flagged'] == flagged and i2['x_pack_tiles'] == xg.tiles_of(n, i2), i2
    if X is not None:
        book, exceptions = books_of(X, base, pad_zeros)
        assert i2['x_pack_book'] == book and i2['x_pack_exceptions'] == exceptions, (i2, book, exceptions)


@pytest.mark.parametrize('case', list(xg.SMALL))
def test_small_shapes_same_bits_as_the_fp32_pass_and_the_28_bit_copy(monkeypatch, case):
    n, d, k, below, negative, flagged = xg.SMALL[case]
    X, W0, T0 = xg.problem(n, d, k, seed=11 + n)
    X, base = xg.plant(X, seed=n, below=below, negative=negative)
    res, infos = three_ways(monkeypatch, n, d, k, lambda e: e.upload_X(X), W0, T0)
    check_infos(infos, n, base, flagged, X, pad_zeros=n * (-d % 4))
    assert infos['2']['x_pack_exceptions'] > 0 or n * d < 100          # (65 elements may all be in the book)
    pk.assert_same_bits(res)


def hand_built(seed):
    """200 x 1030 of planted values; returns X, base, book and a seeded generator.  The records the tests shape afterwards are
    first filled with exponent byte 127, which is in the book"""
    n, d, k = 200, 1030, 4
    X, W0, T0 = xg.problem(n, d, k, seed=seed)
    X, base = xg.plant(X, seed=seed + 1, below=(100, 700), negative=(3, 500))
    return n, d, k, X, W0, T0, base, np.random.RandomState(seed + 2)


def test_a_record_without_exceptions_beside_one_of_nothing_else(monkeypatch):
    n, d, k, X, W0, T0, base, rs = hand_built(41)
    q = 5
    X[8 * q:8 * q + 8, 0:256] = with_exponent(rs, (8, 256), 127)
    for j in range(16):     # inside the window, far below the values around 1; sixteen exponent bytes, so that none gets into the book
        X[8 * q:8 * q + 8, 256 + 16 * j:272 + 16 * j] = with_exponent(rs, (8, 16), 2 * base + 1 + j)
    assert xg.window_base(X) == base
    book, _ = books_of(X, base, n * 2)
    assert exceptions_of_record(X, book, q, 0) == 0 and exceptions_of_record(X, book, q, 1) == 2048, book
    res, infos = three_ways(monkeypatch, n, d, k, lambda e: e.upload_X(X), W0, T0)
    check_infos(infos, n, base, 2, X, pad_zeros=n * 2)
    pk.assert_same_bits(res)


def test_records_of_64_and_65_exceptions_first_and_last_positions(monkeypatch):
    n, d, k, X, W0, T0, base, rs = hand_built(43)
    q, rare = 24, 2 * base + 5                      # the last chunk
    for p, count in ((0, 64), (1, 65)):
        blk = with_exponent(rs, (8, 256), 127)
        where = {(0, 0), (7, 255)}                  # position 0; position 2047: lane 63, row 7, its fourth column
        while len(where) < count:
            where.add((int(rs.randint(8)), int(rs.randint(256))))
        for r, c in where:
            blk[r, c] = with_exponent(rs, (), rare)
        X[8 * q:8 * q + 8, 256 * p:256 * p + 256] = blk
    X[8 * q:8 * q + 8, 1024:1030] = with_exponent(rs, (8, 6), 127)
    X[199, 1029] = with_exponent(rs, (), rare)                         # the last element of X, in the ragged last panel
    assert xg.window_base(X) == base
    book, _ = books_of(X, base, n * 2)
    assert [exceptions_of_record(X, book, q, p) for p in (0, 1)] == [64, 65], book
    res, infos = three_ways(monkeypatch, n, d, k, lambda e: e.upload_X(X), W0, T0)
    check_infos(infos, n, base, 2, X, pad_zeros=n * 2)
    pk.assert_same_bits(res)


def test_interleaved_row_blocks_one_kept_and_none_kept(monkeypatch):
    n, d, k = 30011, 2503, 4
    info, caps = pk.settings(n, d, k, np.float32)
    assert info['interleaved']
    X, W0, T0 = pk.host_problem(n, d, k, seed=5)
    X, base = xg.plant(X, seed=2, below=(30010, 2502))
    for nm in ('one row block kept', 'nothing kept'):
        res, infos = three_ways(monkeypatch, n, d, k, lambda e: e.upload_X(X), W0, T0, cap=caps[nm])
        check_infos(infos, n, base, 1, X, pad_zeros=n * (-d % 4))
        pk.assert_same_bits(res)


def test_bound_X_with_a_row_stride_above_d_inside_nan_bands(monkeypatch):
    import torch
    name = lc.cases(store='fp32', widths=(2,), pads=(1,))[0]
    c = lc.CASES[name]
    k = 3
    X, base = xg.plant(lc.case_matrix(c), seed=4, below=(c.n - 1, c.d - 1))
    g = lc.guarded(torch, X, c.ld, c.c0, device='cuda:0')
    torch.cuda.synchronize()
    rs = np.random.RandomState(1)
    a = float(np.sqrt(X.mean() / k))
    W0, T0 = a * rs.rand(c.n, k), a * rs.rand(k, c.d)
    res, infos = three_ways(monkeypatch, c.n, c.d, k, lambda e: e.bind_X_device(g.ptr, g.ld), W0, T0)
    check_infos(infos, c.n, base, 1)
    pk.assert_same_bits(res)
    g.check('the bound X')


def test_auto_takes_the_narrow_copy_only_with_few_exceptions(monkeypatch):
    """switch unset, RRI_PASS_CACHE_MB=0 (all of X streams, so a copy is built at any size): planted values around 1 get the 26-bit
    copy; an X with 20 % of its elements outside the best 7-entry book gets the 28-bit one, and layout_info() says so"""
    n, d, k = 200, 1030, 4
    X, W0, T0 = xg.problem(n, d, k, seed=51)
    X, base = xg.plant(X, seed=52)
    res, infos = three_ways(monkeypatch, n, d, k, lambda e: e.upload_X(X), W0, T0, cap='0', packs=('0', None))
    book, exceptions = books_of(X, base, n * 2)
    assert exceptions * 16 <= n * 1032
    assert infos[None]['x_pack'] and infos[None]['x_pack_bits'] == 26 and infos[None]['x_pack_book'] == book, infos[None]
    pk.assert_same_bits(res)

    rs = np.random.RandomState(53)
    ebs = np.array([127, 126, 125, 124, 123, 122, 121, 118, 117, 116])          # 80 % in seven exponent bytes, 20 % in three more
    pick = rs.choice(10, size=(n, d), p=[0.8 / 7] * 7 + [0.2 / 3] * 3)
    Y = (ebs[pick].astype(np.uint32) << 23 | rs.randint(0, 1 << 23, size=(n, d)).astype(np.uint32)).view(np.float32)
    ybase = xg.window_base(Y)
    _, yexc = books_of(Y, ybase, n * 2)
    assert abs(yexc / (n * d) - 0.2) < 0.01
    a = float(np.sqrt(Y.mean() / k))
    W1, T1 = a * rs.rand(n, k), a * rs.rand(k, d)
    res, infos = three_ways(monkeypatch, n, d, k, lambda e: e.upload_X(Y), W1, T1, cap='0', packs=('0', None, '2'))
    auto, forced = infos[None], infos['2']
    assert auto['x_pack'] and auto['x_pack_bits'] == 28 and auto['x_pack_book'] == [] and auto['x_pack_exceptions'] == yexc, auto
    assert forced['x_pack'] and forced['x_pack_bits'] == 26 and forced['x_pack_exceptions'] == yexc, forced
    assert auto['x_pack_base'] == forced['x_pack_base'] == ybase and auto['x_pack_flagged'] == forced['x_pack_flagged'] == 0
    pk.assert_same_bits(res)


@pytest.mark.parametrize('how', ['upload_X of another matrix', 'tf-idf scaling in place'])
def test_a_changed_X_gets_a_new_book_and_a_new_copy(monkeypatch, how):
    """sweep, change X, sweep again: the same bits as a fresh handle on the new X started from the same factors, and as the same
    sequence of calls under RRI_X_PACK=0"""
    n, d, k = 200, 1030, 4
    X1, W0, T0 = xg.problem(n, d, k, seed=21)
    X1, base1 = xg.plant(X1, seed=5)
    X2 = xg.plant(xg.problem(n, d, k, seed=22)[0] * np.float32(2.0 ** -31), seed=6)[0]        # another window, other exponents
    monkeypatch.setenv('RRI_ONCHIP', '0')

    def change(e):
        if how.startswith('upload'):
            e.upload_X(X2)
        else:
            e.preprocess(tfidf=True)

    def sequence(pack):
        monkeypatch.setenv(ENV, pack)
        with xg.engine(n, d, k, dtype=np.float32) as e:
            e.upload_X(X1); e.set_W(W0); e.set_T(T0); e.set_params()
            e.sweep(1)
            mid = e.get_W(), e.get_T()
            infos = [e.layout_info()]
            change(e)
            e.sweep(1)
            infos.append(e.layout_info())
            return mid, (e.get_W(), e.get_T(), e.objective()), infos

    mid, packed, infos = sequence('2')
    _, plain, _ = sequence('0')
    assert infos[0]['x_pack_bits'] == 26 and infos[0]['x_pack_base'] == base1 and infos[1]['x_pack_bits'] == 26, infos
    assert infos[0]['x_pack_book'] == books_of(X1, base1, n * 2)[0], infos[0]
    if how.startswith('upload'):
        base2 = xg.window_base(X2)
        assert infos[1]['x_pack_base'] == base2 != base1 and infos[1]['x_pack_book'] == books_of(X2, base2, n * 2)[0], infos
    monkeypatch.setenv(ENV, '2')
    with xg.engine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X1)
        change(e)
        e.set_W(mid[0]); e.set_T(mid[1]); e.set_params()
        e.sweep(1)
        fresh = e.get_W(), e.get_T(), e.objective()
        assert e.layout_info()['x_pack_book'] == infos[1]['x_pack_book'] and e.layout_info()['x_pack_base'] == infos[1]['x_pack_base']
        assert e.layout_info()['x_pack_exceptions'] == infos[1]['x_pack_exceptions']
    monkeypatch.delenv(ENV, raising=False)
    pk.assert_same_bits({'fresh handle': fresh, 'handle whose X changed': packed, 'the same calls, fp32 pass': plain})


def test_the_copy_is_released_with_the_handle(monkeypatch):
    """five buffers: the fixed parts (6.5 KiB per record), the directory (a dword per record and one), the entries (16 bits each),
    the flag bytes and the window's top byte"""
    from rri_nmf_amd.engine import device_memory
    n, d, k = 200, 1030, 4
    X, W0, T0 = xg.problem(n, d, k, seed=8)
    monkeypatch.setenv('RRI_ONCHIP', '0')
    start = device_memory()
    used = {}
    for pack in ('0', '2'):
        monkeypatch.setenv(ENV, pack)
        with xg.engine(n, d, k, dtype=np.float32) as e:
            e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
            e.sweep(1)
            used[pack] = device_memory(), e.layout_info()
        assert device_memory() == start, (pack, start, device_memory())
    monkeypatch.delenv(ENV, raising=False)
    info = used['2'][1]
    assert info['x_pack_bits'] == 26 and info['x_pack_exceptions'] > 0, info
    tiles = -(-n // 8) * 2
    records = 4 * tiles
    want = records * 6656 + (records + 1) * 4 + 2 * info['x_pack_exceptions'] + tiles + 4
    assert used['2'][0][0] == used['0'][0][0] + 5 and used['2'][0][1] == used['0'][0][1] + want, (used, want)


def test_topic_steps_over_the_narrow_copy_against_float64(monkeypatch):
    """fp32 30011 x 2503, one row block kept, the passes over the 26-bit copy: update_T_row(t) and update_W_col(t) against the
    closed form of the step in float64 numpy, at the tolerance of test_xpack_gpu.py (1e-12 in norm, ten times that element-wise)"""
    from oracle import rri_oracle as orc
    n, d, k = 30011, 2503, 4
    tol = 1e-12
    _, caps = pk.settings(n, d, k, np.float32)
    X, W0, T0 = pk.host_problem(n, d, k, seed=5)
    X, _ = xg.plant(X, seed=2, below=(30010, 2502))
    Xs = np.ascontiguousarray(X.astype(np.float64))
    monkeypatch.setenv('RRI_ONCHIP', '0')
    monkeypatch.setenv(ENV, '2')
    monkeypatch.setenv(pk.ENV, caps['one row block kept'])
    with xg.engine(n, d, k, dtype=np.float32) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
        e.sweep(1)                      # the first sweep builds the copy
        assert e.layout_info()['x_pack_bits'] == 26 and e.layout_info()['x_pack_flagged'] == 1
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
