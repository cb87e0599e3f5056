"""The split of a corpus by row, restated in numpy for the CPU and GPU tests (rri_nmf_amd/csrc/rri_rowsplit.hpp has the definitions):
the constants it mirrors, the 64-bit key of an entry with the Philox of tests/derive_cases.py, the quota of a row, the split of a
canonical scipy matrix -- a full sort of every row's keys --, the texts of the refusals by the names tests/c/rowsplit_main.cpp gives
them, and the two corpora the GPU tests are built from."""
import numpy as np
import scipy.sparse as sp

import derive_cases as dc

WAVE_MAX = 64                # rri_rowsplit.hpp: ROWSPLIT_WAVE_MAX, the longest row a wave ranks
BLOCK_THREADS = 256          # ROWSPLIT_BLOCK_THREADS
DIGIT_BITS, BINS, PASSES = 8, 256, 8
BOUND_NONE, BOUND_ALL = 0, 2 ** 64 - 1
CLASS_NONE, CLASS_WAVE, CLASS_BLOCK = 0, 1, 2
OK, INVALID = 0, -1


def keys(A, seed):
    """rowsplit_key of every stored entry of a canonical scipy matrix, in storage order (uint64): word 0 of block 0 of its (row,
    column) under the seed, shifted up 32 bits, with the column below"""
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr)).astype(np.uint64)
    w0 = dc.philox(A.indices, rows & np.uint64(0xffffffff), rows >> np.uint64(32), np.zeros(A.nnz, dtype=np.uint64), int(seed) & 0xffffffff,
                   int(seed) >> 32)[0]
    return (w0.astype(np.uint64) << np.uint64(32)) | A.indices.astype(np.uint64)


def quota(lengths, n_held=None, held_out=None, min_observed=1):
    """rowsplit_quota over an array of row lengths: min(want, max(L - min_observed, 0)), want = n_held or floor(held_out L + 0.5) in
    float64"""
    L = np.asarray(lengths, dtype=np.int64)
    assert (n_held is None) != (held_out is None)
    want = np.full(L.shape, n_held, dtype=np.int64) if n_held is not None else np.floor(np.float64(held_out) * L.astype(np.float64) + 0.5).astype(np.int64)
    return np.minimum(want, np.maximum(L - min_observed, 0))


def row_class(L, h):
    """rowsplit_class"""
    return CLASS_NONE if h <= 0 or h >= L else CLASS_WAVE if L <= WAVE_MAX else CLASS_BLOCK


def split_rows(A, n_held=None, held_out=None, min_observed=1, seed=0, key=None):
    """split_rows_plain on a canonical scipy matrix: (observed, held); the quota of every row, its entries sorted by the whole key,
    the first h held.  key: the keys to use instead of the generator's (one per stored entry)"""
    A = sp.csr_matrix(A)
    lengths = np.diff(A.indptr).astype(np.int64)
    h = quota(lengths, n_held, held_out, min_observed)
    K = keys(A, seed) if key is None else np.asarray(key, dtype=np.uint64)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), lengths)
    held = np.zeros(A.nnz, dtype=bool)
    for r in np.flatnonzero(h > 0):
        lo, hi = int(A.indptr[r]), int(A.indptr[r + 1])
        held[lo + np.argsort(K[lo:hi], kind='stable')[:int(h[r])]] = True
    out = []
    for take in (~held, held):
        indptr = np.concatenate(([0], np.cumsum(np.bincount(rows[take], minlength=A.shape[0])))).astype(np.int64)
        out.append(sp.csr_matrix((A.data[take].copy(), A.indices[take].copy(), indptr), shape=A.shape))
    return out[0], out[1]


# the texts of the refusals (rri_rowsplit.hpp), by the name tests/c/rowsplit_main.cpp gives the case
REQUEST_FINE = ('count_one', 'count_large', 'fraction_small', 'fraction_one', 'min_observed_zero')
REQUEST_TEXT = {
    'observed_null': 'the output pointer is NULL', 'held_null_first': 'the output pointer is NULL',
    'count_zero': 'n_held 0 holds nothing out: a count is at least 1', 'count_zero_first': 'n_held 0 holds nothing out: a count is at least 1',
    'count_minus_two': 'n_held -2 is neither a count nor -1, which asks for a fraction',
    'count_minus_nine_first': 'n_held -9 is neither a count nor -1, which asks for a fraction',
    'both_modes': 'n_held 3 and fraction 0.5 are both given: a split of rows takes one of them',
    'count_with_nan': 'n_held 1 and fraction nan are both given: a split of rows takes one of them',
    'fraction_zero': 'fraction 0 is outside (0, 1]', 'fraction_above_one': 'fraction 1.5 is outside (0, 1]',
    'fraction_negative': 'fraction -0.25 is outside (0, 1]', 'fraction_nan': 'fraction nan is outside (0, 1]',
    'min_observed_negative': 'min_observed -1 is negative', 'min_observed_negative_last': 'min_observed -4 is negative',
}

# ---- the corpora of the GPU tests ---------------------------------------------------------------------------------------------------
# Row lengths on both sides of the two borders at which the kernels take another path -- the wave class ends at 64 entries, a piece at
# 1024 --, the shortest rows, both sides of a workgroup's stride, and a row of three pieces
EDGE_D = 3000
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, dc.PIECE - 1, dc.PIECE, dc.PIECE + 1, 2500]


def edge_corpus(seed=11):
    """one canonical corpus with three rows of every length of EDGE_LENGTHS, shuffled, reals of either sign"""
    rng = np.random.RandomState(seed)
    lengths = rng.permutation(np.repeat(EDGE_LENGTHS, 3)).tolist()
    A = dc.count_corpus(lengths, EDGE_D, seed, negatives=True)
    assert (A.data < 0).any() and A.nnz == 3 * sum(EDGE_LENGTHS)
    return A


def random_corpus(seed=12, shape=(300, 200), density=0.08):
    """a few thousand entries, rows of about sixteen, reals of either sign, some rows empty"""
    rng = np.random.RandomState(seed)
    A = sp.random(shape[0], shape[1], density=density, format='csr', random_state=rng, data_rvs=lambda m: rng.choice([-2.5, -1.0, 0.5, 1.0, 2.0, 3.0, 4.5], size=m))
    A = sp.csr_matrix(A)
    for r in (5, 77):
        A.data[A.indptr[r]:A.indptr[r + 1]] = 0.0
    A.eliminate_zeros()
    A.sort_indices()
    A.indptr, A.indices = A.indptr.astype(np.int64), A.indices.astype(np.int32)
    assert A.has_canonical_format and 3000 < A.nnz < 6000
    return A
