"""The canonical form of a raw CSR matrix and the check in front of it, restated in numpy for the CPU and GPU tests of DeviceCorpus
(rri_nmf_amd/csrc/rri_corpus.hpp has the definition), the constants it mirrors, the malformed matrices both suites refuse, and
generators for rows of given stored lengths."""
import numpy as np
import scipy.sparse as sp

WAVE_MAX = 64                # rri_corpus.hpp: CORPUS_WAVE_MAX, the longest row one wave sorts (B_wave)
LDS_MAX = 16384              # CORPUS_LDS_MAX, the longest row a workgroup sorts in LDS (B_lds)
PAD_MIN = 128                # CORPUS_PAD_MIN
ROW_CANONICAL, ROW_SHORT, ROW_MEDIUM, ROW_LONG = 0, 1, 2, 3
OK, INVALID, UNSUPPORTED = 0, -1, -3


def row_class(flagged, length):
    """corpus_row_class: flagged = not strictly ascending, or a stored zero"""
    return ROW_CANONICAL if not flagged else ROW_SHORT if length <= WAVE_MAX else ROW_MEDIUM if length <= LDS_MAX else ROW_LONG


def pad(length):
    """corpus_pad: the power of two at or above length, at least PAD_MIN"""
    p = PAD_MIN
    while p < length:
        p *= 2
    return p


def check(indptr, indices, values, shape):
    """corpus_check on arrays that are there: (code, text), the six rules in order, the smallest position of the first broken one"""
    n_rows, n_cols = shape
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    nnz = indices.size
    if indptr[0] != 0:
        return INVALID, 'indptr[0] = %d, not 0' % indptr[0]
    down = np.flatnonzero(np.diff(indptr) < 0)
    if down.size:
        return INVALID, 'indptr decreases at %d' % (down[0] + 1)
    if indptr[n_rows] != nnz:
        return INVALID, 'indptr ends at %d, not at the %d stored entries' % (indptr[n_rows], nnz)
    out = np.flatnonzero((indices < 0) | (indices >= n_cols))
    if out.size:
        return INVALID, 'column %d at entry %d is out of range' % (indices[out[0]], out[0])
    if values is not None:
        bad = np.flatnonzero(~np.isfinite(np.asarray(values, dtype=np.float64)))
        if bad.size:
            return INVALID, 'value %g at entry %d is not finite' % (values[bad[0]], bad[0])
    if n_cols >= 2 ** 31:
        return UNSUPPORTED, 'n_cols %d is 2^31 or more' % n_cols
    return OK, ''


def canonical(indptr, indices, values, shape):
    """the canonical form of a checked matrix as a Python loop: a stable argsort on the column, then a sequential float64 sum in
    stored order; sums that are exactly 0 are dropped.  Returns (indptr int64, indices int32, values float64, stats)."""
    n_rows = shape[0]
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    values = np.ones(indices.size) if values is None else np.asarray(values).astype(np.float64)      # float32 widens exactly
    optr, oidx, oval = [0], [], []
    st = dict(rows_rewritten=0, duplicates_merged=0, zeros_dropped=0, negatives=0, long_rows=0)
    for r in range(n_rows):
        cols, vals = indices[indptr[r]:indptr[r + 1]], values[indptr[r]:indptr[r + 1]]
        flagged = bool(np.any(vals == 0) or np.any(np.diff(cols) <= 0))
        st['rows_rewritten'] += flagged
        st['long_rows'] += row_class(flagged, cols.size) == ROW_LONG
        order = np.argsort(cols, kind='stable')
        i = 0
        while i < order.size:
            col, s, e = cols[order[i]], float(vals[order[i]]), i + 1
            while e < order.size and cols[order[e]] == col:
                s += float(vals[order[e]])
                e += 1
            st['duplicates_merged'] += e - i - 1
            if s == 0.0:
                st['zeros_dropped'] += 1
            else:
                oidx.append(col)
                oval.append(s)
                st['negatives'] += s < 0
            i = e
        optr.append(len(oidx))
    return np.array(optr, dtype=np.int64), np.array(oidx, dtype=np.int32), np.array(oval, dtype=np.float64), st


# ---- malformed matrices: name -> (indptr, indices, values, shape); three rows over six columns, five stored entries -------------
_PTR, _IDX, _VAL, _SHAPE = [0, 2, 2, 5], [0, 3, 1, 2, 5], [1.0, 2.0, 3.0, 1.0, 4.0], (3, 6)
NAN, INF = float('nan'), float('inf')
MALFORMED = {
    'indptr_from_one': ([1, 2, 2, 5], _IDX, _VAL, _SHAPE),
    'indptr_from_minus_two': ([-2, 2, 2, 5], _IDX, _VAL, _SHAPE),
    'indptr_decreases_at_2': ([0, 2, 1, 5], _IDX, _VAL, _SHAPE),
    'indptr_decreases_at_3': ([0, 2, 6, 5], _IDX, _VAL, _SHAPE),
    'indptr_ends_short': ([0, 2, 2, 4], _IDX, _VAL, _SHAPE),
    'indptr_ends_long': ([0, 2, 2, 7], _IDX, _VAL, _SHAPE),
    'column_6_at_entry_1': (_PTR, [0, 6, 1, 2, 5], _VAL, _SHAPE),
    'column_negative_at_entry_4': (_PTR, [0, 3, 1, 2, -1], _VAL, _SHAPE),
    'two_columns_the_first_is_named': (_PTR, [0, 3, 7, 2, -1], _VAL, _SHAPE),
    'value_nan_at_entry_3': (_PTR, _IDX, [1.0, 2.0, 3.0, NAN, 4.0], _SHAPE),
    'value_inf_at_entry_0': (_PTR, _IDX, [INF, 2.0, 3.0, 1.0, NAN], _SHAPE),
    'value_minus_inf_at_entry_4': (_PTR, _IDX, [1.0, 2.0, 3.0, 1.0, -INF], _SHAPE),
    'indptr_before_columns': ([0, 2, 1, 5], [0, 9, 1, 2, 5], _VAL, _SHAPE),
    'columns_before_values': (_PTR, [0, 3, 1, 2, 6], [NAN, 2.0, 3.0, 1.0, 4.0], _SHAPE),
    'n_cols_2_31': (_PTR, _IDX, _VAL, (3, 2 ** 31)),
    'n_cols_above_2_31': (_PTR, _IDX, _VAL, (3, 2 ** 31 + 5)),
}
TEXT = {
    'indptr_from_one': 'indptr[0] = 1, not 0', 'indptr_from_minus_two': 'indptr[0] = -2, not 0',
    'indptr_decreases_at_2': 'indptr decreases at 2', 'indptr_decreases_at_3': 'indptr decreases at 3',
    'indptr_ends_short': 'indptr ends at 4, not at the 5 stored entries', 'indptr_ends_long': 'indptr ends at 7, not at the 5 stored entries',
    'column_6_at_entry_1': 'column 6 at entry 1 is out of range', 'column_negative_at_entry_4': 'column -1 at entry 4 is out of range',
    'two_columns_the_first_is_named': 'column 7 at entry 2 is out of range',
    'value_nan_at_entry_3': 'value nan at entry 3 is not finite', 'value_inf_at_entry_0': 'value inf at entry 0 is not finite',
    'value_minus_inf_at_entry_4': 'value -inf at entry 4 is not finite',
    'indptr_before_columns': 'indptr decreases at 2', 'columns_before_values': 'column 6 at entry 4 is out of range',
    'n_cols_2_31': 'n_cols 2147483648 is 2^31 or more', 'n_cols_above_2_31': 'n_cols 2147483653 is 2^31 or more',
}
RULES = 6       # texts that differ by more than a place or a number


def raw_rows(lengths, n_cols, seed, duplicated=1.0 / 3, zeros=0.0, shuffle=True):
    """Raw CSR arrays (indptr int64, indices int64, values float64, shape) whose row q has lengths[q] stored entries: a share
    `duplicated` of them repeat a column the row already holds (so duplicates are certain from two entries on), a share `zeros`
    of the values is an explicit 0, the others are integers in -3 .. 9 without 0, and the entries stand in random order (shuffle)
    or sorted by column.  n_cols must hold the distinct columns of the longest row."""
    rng = np.random.RandomState(seed)
    cols = []
    for L in lengths:
        m = L - int(L * duplicated) if L else 0
        base = rng.choice(n_cols, size=m, replace=False)
        row = np.concatenate([base, rng.choice(base, size=L - m)]) if L else np.zeros(0, dtype=np.int64)
        cols.append(rng.permutation(row) if shuffle else np.sort(row, kind='stable'))
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate(cols + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    values = rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]), size=indices.size)
    if zeros:
        values[rng.rand(indices.size) < zeros] = 0.0
    return indptr, indices, values, (len(lengths), n_cols)


def scipy_canonical(indptr, indices, values, shape):
    """what scipy makes of the raw arrays: duplicates summed, zeros eliminated, indices sorted"""
    data = np.ones(len(indices)) if values is None else np.asarray(values, dtype=np.float64)
    A = sp.csr_matrix((data.copy(), np.asarray(indices).copy(), np.asarray(indptr).copy()), shape=shape)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A
