"""The cases of tests/ld_cases.py and its guard-band builder, checked without a GPU: every case meets the conditions
rri_bind_X_device states, the slice is the matrix and everything else NaN (uint8 counts: the byte 0xFF), and the band checker
sees one changed element, in the band and in the matrix."""
import numpy as np
import pytest

import ld_cases as lc

ALL = list(lc.CASES)
# the thirty cases of the three stores that came first: names, order and (below) values are what they were
EARLIER = ['%s-n%dxd%d-ld%d-c%d' % (s, n, d, d + p * v, v if p > 1 else 0)
           for s, v, ws in (('fp32', 4, (36, 140, 1028)), ('fp64', 2, (38, 142, 516)), ('fp16', 8, (40, 136, 2056)))
           for i, d in enumerate(ws) for n in ((70,) if i == 2 else (130, 203)) for p in (1, 65)]


def test_the_matrices_of_the_earlier_stores_are_what_they_were():
    from rri_nmf_amd.synthetic import planted_X
    for name in EARLIER:
        c = lc.CASES[name]
        for seed in (0, 2):
            want = np.ascontiguousarray(planted_X(c.n, c.d, 6, seed=seed + c.n + c.d, dtype=np.float64).astype(c.dtype))
            assert lc.case_matrix(c, seed=seed).tobytes() == want.tobytes() and lc.vn_of(c.dtype) == 16 // want.itemsize
        assert np.isnan(lc.guard_of(c.dtype))


def test_the_uint8_matrices_are_counts_with_zeros_and_their_scales_are_positive():
    for name in lc.cases('u8'):
        c = lc.CASES[name]
        C = lc.case_matrix(c)
        assert C.dtype == np.uint8 and (C == 0).any() and C.max() == 255 and 20 < C.mean() < 60
        assert lc.guard_of(c.dtype) == 0xFF
        r, s = lc.case_scales(c)
        assert r.shape == (c.n,) and s.shape == (c.d,) and 0.1 <= min(r.min(), s.min()) and max(r.max(), s.max()) <= 10.0
        X = lc.scaled(C, r, s)
        assert X.dtype == np.float64 and X[3, 5] == (float(C[3, 5]) * s[5]) * r[3]


def test_the_case_table_is_the_written_one():
    assert lc.G >= 256
    assert len(ALL) == 4 * (2 * 2 + 1) * 2
    assert list(lc.STORES) == ['fp32', 'fp64', 'fp16', 'u8'] and ALL[:30] == EARLIER
    for store, dtype in lc.STORES.items():
        vn = lc.vn_of(dtype)
        assert vn == {'fp32': 4, 'fp64': 2, 'fp16': 8, 'u8': 8}[store]
        small, mid, wide = lc.WIDTHS[store]
        itemsize = np.dtype(dtype).itemsize
        assert small < 64 < mid and -(-mid // 64) == 3 and mid % 64 != 0
        panel = 4 * 64 * vn * itemsize                  # a workgroup of the pass: 4 waves x 64 lanes x one load
        assert panel == (2048 if store == 'u8' else 4096)
        assert panel < wide * itemsize <= 2 * panel                     # two column panels of the streaming pass
        seen = {(c.n, c.d, c.ld, c.c0) for c in lc.CASES.values() if c.store == store}
        want = set()
        for d in (small, mid, wide):
            for n in ((70,) if d == wide else (130, 203)):
                want |= {(n, d, d + vn, 0), (n, d, d + 65 * vn, vn)}
        assert seen == want
    assert set(lc.cases('fp32')) | set(lc.cases('fp64')) | set(lc.cases('fp16')) | set(lc.cases('u8')) == set(ALL)
    assert lc.cases('u8') == ['u8-n130xd40-ld48-c0', 'u8-n130xd40-ld560-c8', 'u8-n203xd40-ld48-c0', 'u8-n203xd40-ld560-c8',
                              'u8-n130xd136-ld144-c0', 'u8-n130xd136-ld656-c8', 'u8-n203xd136-ld144-c0', 'u8-n203xd136-ld656-c8',
                              'u8-n70xd2056-ld2064-c0', 'u8-n70xd2056-ld2576-c8']
    assert lc.cases('fp64', widths=(1,), rows=(1,), pads=(1,)) == ['fp64-n203xd142-ld272-c2']


@pytest.mark.parametrize('case', ALL)
def test_a_case_meets_the_conditions_of_the_bind(case):
    c = lc.CASES[case]
    vn, itemsize = lc.vn_of(c.dtype), np.dtype(c.dtype).itemsize
    X = lc.case_matrix(c)
    assert X.dtype == c.dtype and X.shape == (c.n, c.d) and np.isfinite(X).all() and (X > 0).any()
    g = lc.guarded(np, X, c.ld, c.c0)
    assert c.d % vn == 0, 'binding needs d % VN == 0'
    assert c.ld >= c.c0 + c.d and c.ld > c.d, 'the stride must exceed the width: that is the case'
    load = vn * itemsize                            # bytes of one load: 16, for uint8 counts 8
    assert load == (8 if c.store == 'u8' else 16)
    assert (c.ld * itemsize) % load == 0
    assert g.base % 16 == 0, 'the builder aligns its numpy allocation'
    assert (g.offset * itemsize) % load == 0 and g.ptr % load == 0, 'an aligned allocation gives a slice aligned to the load'
    assert g.ptr == g.view.ctypes.data and g.ld * itemsize == g.view.strides[0] and g.ld == c.ld
    assert g.buf.shape == (lc.G + c.n + lc.G, c.ld)
    assert g.rows(64, c.n) == (g.view[64:].ctypes.data, c.ld)


@pytest.mark.parametrize('case', ALL)
def test_the_slice_is_the_matrix_and_the_rest_is_nan(case):
    c = lc.CASES[case]
    X = lc.case_matrix(c)
    g = lc.guarded(np, X, c.ld, c.c0)
    assert g.view.shape == X.shape and g.view.tobytes() == X.tobytes()
    inside = np.zeros(g.buf.shape, dtype=bool)
    inside[lc.G:lc.G + c.n, c.c0:c.c0 + c.d] = True
    assert lc.is_guard(g.buf[~inside]).all() and int((~inside).sum()) == g.buf.size - X.size
    assert np.isfinite(g.buf[inside]).all() and np.array_equal(g.buf[inside].reshape(X.shape), X)
    if c.store == 'u8':
        assert g.buf.dtype == np.uint8 and (g.buf[~inside] == 0xFF).all() and not lc.is_guard(g.buf[inside]).all()
    else:
        assert np.isnan(g.buf[~inside]).all()
    # what lies right behind the last row of the matrix and right of its last column is band, inside the allocation
    assert lc.is_guard(g.buf[lc.G + c.n:, :]).all() and g.buf[lc.G + c.n:, :].shape[0] == lc.G
    assert lc.is_guard(g.buf[:, c.c0 + c.d:]).all() and g.buf[:, c.c0 + c.d:].shape[1] >= lc.vn_of(c.dtype)
    g.check()
    assert g.changed() == []


@pytest.mark.parametrize('case', ALL)
def test_the_checker_reports_one_changed_element(case):
    c = lc.CASES[case]
    X = lc.case_matrix(c)
    ints = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[np.dtype(c.dtype).itemsize]
    # one bit of a guard element flipped: still a NaN, another one (a byte: 0xFE)
    g = lc.guarded(np, X, c.ld, c.c0)
    i, j = lc.G + c.n, c.c0 + c.d - 1                 # first guard row below the matrix, under its last column
    g.buf.view(ints)[i, j] ^= 1
    assert (g.buf[i, j] == 0xFE if c.store == 'u8' else np.isnan(g.buf[i, j])) and g.changed() == [(i, j)]
    with pytest.raises(AssertionError, match=r'1 element\(s\) changed, first guard band \(row %d, column %d' % (i, j)):
        g.check()
    # the pad right of the last row: the element a flat copy of n * ld elements reads last
    g = lc.guarded(np, X, c.ld, c.c0)
    g.buf[lc.G + c.n - 1, c.ld - 1] = 0.0
    assert g.changed() == [(lc.G + c.n - 1, c.ld - 1)]
    # one element of the matrix changed by one unit in the last place
    g = lc.guarded(np, X, c.ld, c.c0)
    g.view[c.n - 1, 0] = g.view[c.n - 1, 0] ^ 1 if c.store == 'u8' else np.nextafter(g.view[c.n - 1, 0], c.dtype(np.inf))
    assert g.changed() == [(lc.G + c.n - 1, c.c0)]
    with pytest.raises(AssertionError, match=r'first matrix\[%d, 0\]' % (c.n - 1)):
        g.check()
    # +0.0 -> -0.0 compares equal as a number and is a change of bits (a byte has one zero: a count of 0 become the guard byte)
    g = lc.guarded(np, np.zeros_like(X), c.ld, c.c0)
    g.view[0, c.d - 1] = 0xFF if c.store == 'u8' else -0.0
    assert g.changed() == [(lc.G, c.c0 + c.d - 1)]
