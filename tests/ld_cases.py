"""Matrices with a row stride larger than their width, inside bands of NaN (uint8: of 0xFF): the cases of tests/test_strided_bind_gpu.py
(tests/test_ld_cases_cpu.py checks the cases and the builder themselves, without a GPU).

rri_bind_X_device and rri_bind_mask_device take a row stride ld >= d, so that a slice Xwide[r0:r0 + n, c0:c0 + d] of a wider
device array can be handed over as it is.  A guarded matrix is that situation with everything around the slice made visible:
ONE allocation of (G + n + G) x ld elements of the storage type, every element NaN, the matrix at rows G .. G + n - 1 and columns
c0 .. c0 + d - 1.

    * a kernel that takes the handle's own stride (LD = d for a bound array) where ldx / ldm is meant reads other elements: NaN;
    * a kernel that reads past column d or past row n and multiplies what it read by 0 gets NaN, not 0;
    * a kernel that writes to bound memory changes the allocation, which is compared bit for bit (integer views) with what it was.

The guard rows BELOW the matrix are part of the construction, not an option: no test binds a slice whose last row ends its
allocation, so a read past the last row lands in the band, never outside the allocation.  G is at least the rows of a row block
of the streaming pass (rri_layout_info field 8, asserted by the GPU test), so a row block that starts inside the matrix ends
inside the allocation.

uint8 counts (RRI_U8) have no NaN.  Their guard byte is 0xFF, the largest count: a read at the wrong stride or past row n pulls
255s into a sum, far outside every bound that the sums are held to against the float64 reference (the band is then seen through
the reference, not through a non-finite output).  What is lost against NaN: a read past column d whose value is multiplied by an
operand of 0 adds 255 * 0 = 0 and stays invisible, where NaN * 0 is NaN.  Such a read is also harmless.  A write is seen as
before, bit for bit.  Their vectors are 8 bytes (VN = 8, a workgroup of the pass spans 2048 columns), their matrices counts
0 .. 255 with zeros.

The builder works on numpy arrays (the CPU test) and on torch tensors (the GPU test): guarded(np, ...) / guarded(torch, ...).

Case table, VN = 16 / itemsize (the elements of a 16-byte vector; uint8: the 8 of an 8-byte one; binding needs d % VN == 0 -- load_elems
and load_bytes of rri_nmf_amd/csrc/rri_layout.hpp, which tests/test_layout_cpu.py holds to vn_of and strides_of below):
    d       one column tile (d < 64) | three column tiles, the last ragged | two column panels of the streaming pass (256 vectors each)
    n       130 and 203 (3 and 4 row blocks of 64, both ragged) for the two small d; 70 for the two-panel d
    ld, c0  (d + VN, 0): the smallest legal pad;  (d + 65 VN, VN): a pad wider than the 64 vectors one wave covers, and a column
            offset -- a lane whose column test took ld for d still reads inside the allocation, and reads NaN
"""
import collections

import numpy as np

G = 256
STORES = {'fp32': np.float32, 'fp64': np.float64, 'fp16': np.float16, 'u8': np.uint8}
WIDTHS = {'fp32': (36, 140, 1028), 'fp64': (38, 142, 516), 'fp16': (40, 136, 2056), 'u8': (40, 136, 2056)}
GUARD_BYTE = 0xFF
ROWS_SMALL, ROWS_TWO_PANELS = (130, 203), (70,)

Case = collections.namedtuple('Case', 'name store dtype n d ld c0')


def vn_of(dtype):
    """elements of one load of the handle: a 16-byte vector; uint8 counts take 8-byte loads"""
    return 8 if np.dtype(dtype) == np.uint8 else 16 // np.dtype(dtype).itemsize


def guard_of(dtype):
    """what every element outside the matrix holds"""
    return GUARD_BYTE if np.dtype(dtype) == np.uint8 else float('nan')


def is_guard(a):
    """element-wise: does a (a numpy array of a storage type) hold the guard value?"""
    return a == GUARD_BYTE if a.dtype == np.uint8 else np.isnan(a)


def strides_of(d, dtype):
    """the two (ld, c0) of every width"""
    vn = vn_of(dtype)
    return ((d + vn, 0), (d + 65 * vn, vn))


def _cases():
    out = []
    for store, dtype in STORES.items():
        for i, d in enumerate(WIDTHS[store]):
            for n in (ROWS_TWO_PANELS if i == 2 else ROWS_SMALL):
                for ld, c0 in strides_of(d, dtype):
                    out.append(Case('%s-n%dxd%d-ld%d-c%d' % (store, n, d, ld, c0), store, dtype, n, d, ld, c0))
    return out


CASES = collections.OrderedDict((c.name, c) for c in _cases())


def cases(store=None, widths=None, rows=None, pads=None):
    """names of the cases of one storage type; widths / rows / pads: indices into WIDTHS[store], the row counts of a width and
    the two strides (None: all)"""
    out = []
    for c in CASES.values():
        if store is not None and c.store != store:
            continue
        wi = WIDTHS[c.store].index(c.d)
        ri = (ROWS_TWO_PANELS if wi == 2 else ROWS_SMALL).index(c.n)
        pi = 0 if c.c0 == 0 else 1
        if (widths is None or wi in widths) and (rows is None or ri in rows) and (pads is None or pi in pads):
            out.append(c.name)
    return out


_INT_NAME = {1: 'int8', 2: 'int16', 4: 'int32', 8: 'int64'}


def _is_numpy(xp):
    return xp is np


def _int_view(xp, a):
    """the same memory as integers of the element's size: comparisons are then of bits (NaN != NaN, +0.0 == -0.0 otherwise)"""
    if _is_numpy(xp):
        return a.view(getattr(np, _INT_NAME[a.itemsize]))
    return a.view(getattr(xp, _INT_NAME[a.element_size()]))


class Guarded(object):
    """buf: the whole (G + n + G) x ld allocation;  view: the n x d matrix inside it (a strided view, no copy);  ld: its row
    stride in elements;  offset: elements from the start of the allocation to view[0, 0];  ptr: the address of view[0, 0]"""

    def __init__(self, xp, values, ld, c0, g=G, device=None):
        values = np.ascontiguousarray(values)
        n, d = values.shape
        if ld < c0 + d:
            raise ValueError('the slice does not fit the row: ld=%d < c0 + d = %d' % (ld, c0 + d))
        self.xp, self.n, self.d, self.ld, self.c0, self.g = xp, n, d, int(ld), int(c0), int(g)
        rows = g + n + g
        if _is_numpy(xp):
            self.buf = _aligned_full(rows, ld, values.dtype)
            self.buf[g:g + n, c0:c0 + d] = values
            base = self.buf.ctypes.data
        else:
            self.buf = xp.full((rows, ld), guard_of(values.dtype), dtype=getattr(xp, np.dtype(values.dtype).name), device=device)
            self.buf[g:g + n, c0:c0 + d] = xp.from_numpy(values).to(device)
            base = self.buf.data_ptr()
        self.view = self.buf[g:g + n, c0:c0 + d]
        self.offset = g * self.ld + c0
        self.itemsize = np.dtype(values.dtype).itemsize
        self.base = base
        self.ptr = base + self.offset * self.itemsize
        ints = _int_view(xp, self.buf)
        self._before = ints.copy() if _is_numpy(xp) else ints.clone()

    def rows(self, lo, hi):
        """(address, ld) of rows lo .. hi - 1 of the matrix: a row block of it, as one rank of a row-sharded run binds"""
        if not 0 <= lo < hi <= self.n:
            raise ValueError('rows %d .. %d are not rows of the %d-row matrix' % (lo, hi, self.n))
        return self.ptr + lo * self.ld * self.itemsize, self.ld

    def changed(self):
        """(row, column) in the allocation of every element whose bits are not what they were when it was built"""
        now = _int_view(self.xp, self.buf)
        diff = now != self._before
        if _is_numpy(self.xp):
            return [tuple(int(v) for v in ij) for ij in np.argwhere(diff)]
        return [tuple(int(v) for v in ij) for ij in diff.nonzero().cpu().numpy()]

    def where(self, i, j):
        inside = self.g <= i < self.g + self.n and self.c0 <= j < self.c0 + self.d
        return 'matrix[%d, %d]' % (i - self.g, j - self.c0) if inside else 'guard band (row %d, column %d of the allocation)' % (i, j)

    def check(self, what='the guarded allocation'):
        """raises AssertionError naming the changed elements; the matrix itself counts: bound memory is never written"""
        bad = self.changed()
        if bad:
            raise AssertionError('%s was written: %d element(s) changed, first %s' % (
                what, len(bad), ', '.join(self.where(i, j) for i, j in bad[:6])))


def _aligned_full(rows, ld, dtype, align=64):
    """a rows x ld numpy array of guard values whose first element sits at a multiple of `align` bytes"""
    dtype = np.dtype(dtype)
    raw = np.empty(rows * ld * dtype.itemsize + align, dtype=np.uint8)
    skip = (-raw.ctypes.data) % align
    buf = raw[skip:skip + rows * ld * dtype.itemsize].view(dtype).reshape(rows, ld)
    buf[...] = guard_of(dtype)
    return buf


def guarded(xp, values, ld, c0, g=G, device=None):
    return Guarded(xp, values, ld, c0, g=g, device=device)


def case_matrix(case, seed=0):
    """the matrix of a case in its storage type: positive, low rank plus noise, rounded once (planted_X's recipe at any size);
    uint8: counts 0 .. 255 with zeros, round(40 P / mean(P)) clipped (count_problem of tests/test_count_storage_gpu.py)"""
    from rri_nmf_amd.synthetic import planted_X
    c = CASES[case] if isinstance(case, str) else case
    P = planted_X(c.n, c.d, 6, seed=seed + c.n + c.d, dtype=np.float64)
    if np.dtype(c.dtype) == np.uint8:
        P = np.minimum(np.round(40.0 * P / P.mean()), 255.0)
    return np.ascontiguousarray(P.astype(c.dtype))


def case_scales(case, seed=0):
    """(row_scale, col_scale) of a uint8 case, log-uniform over 0.1 .. 10: set after the bind, which puts both back to ones"""
    c = CASES[case] if isinstance(case, str) else case
    rs = np.random.RandomState(seed + 7 * c.n + c.d)
    return 10.0 ** rs.uniform(-1, 1, c.n), 10.0 ** rs.uniform(-1, 1, c.d)


def scaled(C, r, s):
    """the float64 matrix a uint8 handle factorises: (C * s) * r[:, None]"""
    return np.ascontiguousarray((np.asarray(C, dtype=np.float64) * s) * r[:, None])
