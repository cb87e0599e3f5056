"""A corpus from (row, column, value) pairs and the split of a corpus by entry, restated in numpy for the CPU and GPU tests
(rri_nmf_amd/csrc/rri_corpus_build.hpp has the definitions): the constants it mirrors, the check of a list with its texts, the
corpus of a list -- a stable argsort by row feeding the restatement of the canonical form in tests/corpus_cases.py --, the split
with the Philox of tests/derive_cases.py, the texts of the refusals by the names tests/c/corpus_build_main.cpp gives them, and the
lists the GPU tests are built from."""
import numpy as np
import scipy.sparse as sp

import corpus_cases as cc
import derive_cases as dc

WAVE_PAIRS = 64              # rri_corpus_build.hpp: CB_WAVE_PAIRS, the consecutive pairs of one wave
BLOCK_PAIRS = 256            # CB_BLOCK_PAIRS, ... of one workgroup
GRID_MAX = 1024              # CB_GRID_MAX, the most workgroups of a pass over the pairs
SWEEP_PAIRS = BLOCK_PAIRS * GRID_MAX     # CB_SWEEP_PAIRS: grid-stride beyond
PAIRS_MAX = 2 ** 31 - 1      # CB_PAIRS_MAX
RULES = 3
OK, INVALID, UNSUPPORTED = 0, -1, -3
INFO = ('rows_rewritten', 'duplicates_merged', 'zeros_dropped', 'negatives', 'long_rows')


def grid(n_pairs):
    """pairs_grid"""
    return max(1, min(GRID_MAX, -(-n_pairs // BLOCK_PAIRS)))


def check(rows, cols, values, shape):
    """pairs_check on arrays that are there: (code, text), the three rules in order, the smallest position of the first broken one
    (after the two limits that are refused before any array is read)"""
    n_rows, n_cols = shape
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if n_cols >= 2 ** 31:
        return UNSUPPORTED, 'n_cols %d is 2^31 or more' % n_cols
    for what, a, bound in (('row', rows, n_rows), ('column', cols, n_cols)):
        out = np.flatnonzero((a < 0) | (a >= bound))
        if out.size:
            return INVALID, '%s %d at pair %d is out of range' % (what, a[out[0]], out[0])
    if values is not None:
        bad = np.flatnonzero(~np.isfinite(np.asarray(values, dtype=np.float64)))
        if bad.size:
            return INVALID, 'value %g at pair %d is not finite' % (values[bad[0]], bad[0])
    return OK, ''


def raw_csr(rows, cols, values, shape):
    """the raw CSR matrix a list of pairs stands for: row i holds the pairs of row i in the order given (a stable sort by row).
    (indptr int64, indices int64, values or None)"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind='stable')
    indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=shape[0])))).astype(np.int64) if shape[0] else np.zeros(1, dtype=np.int64)
    return indptr, cols[order], None if values is None else np.asarray(values)[order]


def from_pairs(rows, cols, values, shape):
    """corpus_from_pairs_plain: (indptr int64, indices int32, values float64, stats) -- the canonical form of raw_csr"""
    indptr, indices, vals = raw_csr(rows, cols, values, shape)
    return cc.canonical(indptr, indices, vals, shape)


def split_entries(A, thr, seed):
    """split_entries_plain on a canonical scipy matrix: (observed, held); an entry is held when word 0 of block 0 of its
    (row, column) is below thr"""
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))
    r = rows.astype(np.uint64)
    w0 = dc.philox(A.indices, r & np.uint64(0xffffffff), r >> np.uint64(32), np.zeros(A.nnz, dtype=np.uint64), int(seed) & 0xffffffff, int(seed) >> 32)[0]
    held = w0 < np.uint64(thr)
    out = []
    for take in (~held, held):
        indptr = np.concatenate(([0], np.cumsum(np.bincount(rows[take], minlength=A.shape[0])))).astype(np.int64)
        out.append(sp.csr_matrix((A.data[take].copy(), A.indices[take].copy(), indptr), shape=A.shape))
    return out[0], out[1]


# the texts of the refusals (rri_corpus_build.hpp), by the name tests/c/corpus_build_main.cpp gives the case
REQUEST_FINE = ('fine', 'fine_without_values', 'empty', 'empty_null_arrays', 'values_dtype_unread_without_values')
REQUEST_TEXT = {
    'negative_rows': (INVALID, 'n_rows -1 is negative'), 'negative_rows_first': (INVALID, 'n_rows -4 is negative'),
    'negative_cols': (INVALID, 'n_cols -2 is negative'), 'negative_cols_first': (INVALID, 'n_cols -9 is negative'),
    'negative_pairs': (INVALID, 'n_pairs -1 is negative'), 'negative_pairs_first': (INVALID, 'n_pairs -3 is negative'),
    'index_dtype_unknown': (INVALID, 'index dtype code 1 is neither RRI_I32 nor RRI_I64'),
    'index_dtype_unknown_first': (INVALID, 'index dtype code 77 is neither RRI_I32 nor RRI_I64'),
    'values_dtype_unknown': (INVALID, 'values dtype code 8 is neither RRI_F32 nor RRI_F64'),
    'values_dtype_unknown_first': (INVALID, 'values dtype code 55 is neither RRI_F32 nor RRI_F64'),
    'stride_zero': (INVALID, 'index_stride 0 is below 1'), 'stride_negative_first': (INVALID, 'index_stride -2 is below 1'),
    'rows_null': (INVALID, 'rows is NULL with 4 pairs'), 'rows_null_first': (INVALID, 'rows is NULL with 2 pairs'),
    'cols_null': (INVALID, 'cols is NULL with 4 pairs'), 'cols_null_first': (INVALID, 'cols is NULL with 9 pairs'),
    'n_cols_2_31': (UNSUPPORTED, 'n_cols 2147483648 is 2^31 or more'),
    'n_cols_above_2_31_first': (UNSUPPORTED, 'n_cols 2147483653 is 2^31 or more'),
    'n_pairs_2_31': (UNSUPPORTED, 'n_pairs 2147483648 is above 2^31 - 1: the pair position is half of a sort key'),
    'n_pairs_above_2_31': (UNSUPPORTED, 'n_pairs 2147483655 is above 2^31 - 1: the pair position is half of a sort key'),
    'row_3_at_1': (INVALID, 'row 3 at pair 1 is out of range'), 'row_negative_at_2': (INVALID, 'row -1 at pair 2 is out of range'),
    'column_6_at_0': (INVALID, 'column 6 at pair 0 is out of range'), 'column_negative_at_3': (INVALID, 'column -1 at pair 3 is out of range'),
    'rows_before_columns': (INVALID, 'row 7 at pair 3 is out of range'),
    'value_nan_at_2': (INVALID, 'value nan at pair 2 is not finite'), 'value_minus_inf_at_3': (INVALID, 'value -inf at pair 3 is not finite'),
    'columns_before_values': (INVALID, 'column 8 at pair 3 is out of range'), 'rows_before_values': (INVALID, 'row 3 at pair 3 is out of range'),
    'no_rows_at_all': (INVALID, 'row 0 at pair 0 is out of range'),
    'interleaved_column_9_at_2': (INVALID, 'column 9 at pair 2 is out of range'),
}
KINDS = 13      # texts that differ by more than a place or a number

# ---- the lists of the GPU tests ---------------------------------------------------------------------------------------------------
# Row lengths on both sides of every class border of rri_corpus.hpp: nothing, one pair, a wave (64), the shortest pad of the LDS
# class (128), the longest row of the LDS class and the first of the global one
EDGE_ROWS, EDGE_COLS = 18000, 40000
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, cc.LDS_MAX, cc.LDS_MAX + 1]


def edge_list(seed=5):
    """(rows, cols, values, shape): under 100000 pairs sorted by row with ascending columns -- no row is rewritten as given --,
    whose rows hold EDGE_LENGTHS pairs (each length twice, and short rows scattered between), the first row empty, the last row and
    the last column used; with one row more in the shape the last row is empty too"""
    rng = np.random.RandomState(seed)
    place = {0: 0, EDGE_ROWS - 1: 3}
    free = [r for r in rng.permutation(np.arange(1, EDGE_ROWS - 1)).tolist()]
    for L in EDGE_LENGTHS + EDGE_LENGTHS[:-2]:
        place[free.pop()] = L
    for _ in range(400):
        place[free.pop()] = int(rng.randint(1, 40))
    rows, cols = [], []
    for r in sorted(place):
        L = place[r]
        c = np.sort(rng.choice(EDGE_COLS, size=L, replace=False))
        if r == EDGE_ROWS - 1:
            c[-1] = EDGE_COLS - 1
        rows.append(np.full(L, r, dtype=np.int64))
        cols.append(c.astype(np.int64))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    values = rng.choice(np.array([-2.5, -1.0, 0.25, 1.0, 2.0, 3.0, 7.5]), size=rows.size)
    assert rows.size < 100000 and rows[-1] == EDGE_ROWS - 1 and rows[0] > 0 and cols.max() == EDGE_COLS - 1
    return rows, cols, values, (EDGE_ROWS, EDGE_COLS)


def grid_edges():
    """the numbers of pairs at which the passes over the list cut their work: nothing, one, a wave, a workgroup and the full grid,
    one below, at and one above each"""
    out = [0, 1]
    for c in (WAVE_PAIRS, BLOCK_PAIRS, SWEEP_PAIRS):
        out += [c - 1, c, c + 1]
    return out


def random_list(n_pairs, shape, seed, zeros=0.05, grouped=False):
    """(rows, cols, values): n_pairs random pairs, duplicates as they fall, a share of explicit zeros; grouped: sorted by row (the
    columns in random order)"""
    rng = np.random.RandomState(seed)
    rows = rng.randint(0, shape[0], size=n_pairs).astype(np.int64)
    cols = rng.randint(0, shape[1], size=n_pairs).astype(np.int64)
    values = rng.choice(np.array([-3.0, -1.5, 0.5, 1.0, 2.0, 4.0]), size=n_pairs)
    values[rng.rand(n_pairs) < zeros] = 0.0
    if grouped:
        rows = np.sort(rows)
    return rows, cols, values
