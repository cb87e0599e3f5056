"""The cases of tests/ld_cases.py and its guard-band builder, checked without a GPU: every case meets the conditions
rri_bind_X_device states, the slice is the matrix and everything else NaN, and the band checker sees one changed element,
in the band and in the matrix."""
import numpy as np
import pytest

import ld_cases as lc

ALL = list(lc.CASES)


def test_the_case_table_is_the_written_one():
    assert lc.G >= 256
    assert len(ALL) == 3 * (2 * 2 + 1) * 2
    for store, dtype in lc.STORES.items():
        vn = lc.vn_of(dtype)
        assert vn == {'fp32': 4, 'fp64': 2, 'fp16': 8}[store]
        small, mid, wide = lc.WIDTHS[store]
        itemsize = np.dtype(dtype).itemsize
        assert small < 64 < mid and -(-mid // 64) == 3 and mid % 64 != 0
        assert 4096 < wide * itemsize <= 2 * 4096                       # two 4 KiB column panels of the streaming pass
        seen = {(c.n, c.d, c.ld, c.c0) for c in lc.CASES.values() if c.store == store}
        want = set()
        for d in (small, mid, wide):
            for n in ((70,) if d == wide else (130, 203)):
                want |= {(n, d, d + vn, 0), (n, d, d + 65 * vn, vn)}
        assert seen == want
    assert set(lc.cases('fp32')) | set(lc.cases('fp64')) | set(lc.cases('fp16')) == set(ALL)
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
    assert (c.ld * itemsize) % 16 == 0
    assert g.base % 16 == 0, 'the builder aligns its numpy allocation'
    assert (g.offset * itemsize) % 16 == 0 and g.ptr % 16 == 0, 'a 16-byte aligned allocation gives a 16-byte aligned slice'
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
    assert np.isnan(g.buf[~inside]).all() and int((~inside).sum()) == g.buf.size - X.size
    assert np.isfinite(g.buf[inside]).all()
    # what lies right behind the last row of the matrix and right of its last column is band, inside the allocation
    assert np.isnan(g.buf[lc.G + c.n:, :]).all() and g.buf[lc.G + c.n:, :].shape[0] == lc.G
    assert np.isnan(g.buf[:, c.c0 + c.d:]).all() and g.buf[:, c.c0 + c.d:].shape[1] >= lc.vn_of(c.dtype)
    g.check()
    assert g.changed() == []


@pytest.mark.parametrize('case', ALL)
def test_the_checker_reports_one_changed_element(case):
    c = lc.CASES[case]
    X = lc.case_matrix(c)
    ints = {2: np.int16, 4: np.int32, 8: np.int64}[np.dtype(c.dtype).itemsize]
    # one bit of a guard element flipped: still a NaN, another one
    g = lc.guarded(np, X, c.ld, c.c0)
    i, j = lc.G + c.n, c.c0 + c.d - 1                 # first guard row below the matrix, under its last column
    g.buf.view(ints)[i, j] ^= 1
    assert np.isnan(g.buf[i, j]) and g.changed() == [(i, j)]
    with pytest.raises(AssertionError, match=r'1 element\(s\) changed, first guard band \(row %d, column %d' % (i, j)):
        g.check()
    # the pad right of the last row: the element a flat copy of n * ld elements reads last
    g = lc.guarded(np, X, c.ld, c.c0)
    g.buf[lc.G + c.n - 1, c.ld - 1] = 0.0
    assert g.changed() == [(lc.G + c.n - 1, c.ld - 1)]
    # one element of the matrix changed by one unit in the last place
    g = lc.guarded(np, X, c.ld, c.c0)
    g.view[c.n - 1, 0] = np.nextafter(g.view[c.n - 1, 0], c.dtype(np.inf))
    assert g.changed() == [(lc.G + c.n - 1, c.c0)]
    with pytest.raises(AssertionError, match=r'first matrix\[%d, 0\]' % (c.n - 1)):
        g.check()
    # +0.0 -> -0.0 compares equal as a number and is a change of bits
    g = lc.guarded(np, np.zeros_like(X), c.ld, c.c0)
    g.view[0, c.d - 1] = -0.0
    assert g.changed() == [(lc.G, c.c0 + c.d - 1)]
