"""Corpora derived from a resident corpus, restated in numpy for the CPU and GPU tests (rri_nmf_amd/csrc/rri_derive.hpp has the
definitions): the constants it mirrors, Philox4x32-10 and the held part of an entry vectorised over entries and blocks, the split
of a canonical scipy matrix, the value check with its texts, the pieces, the texts of the request refusals, and generators of
count matrices with rows of given lengths."""
import numpy as np
import scipy.sparse as sp

PIECE = 1024                 # rri_derive.hpp: DERIVE_PIECE, the most source entries of one piece (a wave's work)
LANE_MAX = 256               # SPLIT_LANE_MAX, the largest count one lane thins alone
COUNT_MAX = 1 << 20          # SPLIT_COUNT_MAX, the largest count that is split
RULES = 3
OK, INVALID, UNSUPPORTED = 0, -1, -3
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xffffffff)
_S32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays (or scalars) of 32-bit words held in uint64: the four output words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2              # 32 x 32 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c0, c1, c2, c3


def threshold(held_out):
    """split_threshold: floor(held_out 2^32), or None where the share is refused"""
    if not 0.0 < held_out < 1.0:
        return None
    thr = int(np.floor(held_out * 4294967296.0))
    return thr if thr >= 1 else None


def held_part(rows, cols, counts, thr, seed):
    """split_held for every entry (row, column, count): token t uses word t % 4 of block t / 4 with the counter (column, row low,
    row high, block) and the key (seed low, seed high), and is held when the word is below thr"""
    rows, cols, counts = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (rows, cols, counts))
    nb = (counts + 3) // 4
    ent = np.repeat(np.arange(counts.size), nb)
    b = np.arange(int(nb.sum()), dtype=np.int64) - np.repeat(np.cumsum(nb) - nb, nb)
    r = rows[ent].astype(np.uint64)
    words = philox(cols[ent], r & _M32, r >> _S32, b, int(seed) & 0xffffffff, int(seed) >> 32)
    left = counts[ent] - 4 * b
    hits = sum(((w < np.uint64(thr)) & (left > e)).astype(np.int64) for e, w in enumerate(words))
    out = np.zeros(counts.size, dtype=np.int64)
    np.add.at(out, ent, hits)
    return out


def split(A, thr, seed):
    """derive_split_plain on a canonical scipy matrix of counts: (observed, held)"""
    A = sp.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))
    counts = A.data.astype(np.int64)
    h = held_part(rows, A.indices, counts, thr, seed)
    out = []
    for part in (counts - h, h):
        M = sp.csr_matrix((part.astype(np.float64), A.indices.copy(), A.indptr.copy()), shape=A.shape)
        M.eliminate_zeros()
        out.append(M)
    return out[0], out[1]


def check_values(values):
    """split_check_values: (code, text), each rule over all positions before the next"""
    v = np.asarray(values, dtype=np.float64)
    for rule, (broken, code, text) in enumerate(((v < 0, INVALID, 'value %.17g at entry %d is negative: a split takes counts'),
                                                 (v != np.floor(v), INVALID, 'value %.17g at entry %d is not a whole number: a split takes counts'),
                                                 (v > COUNT_MAX, UNSUPPORTED, 'value %.17g at entry %d is above 1048576, the largest count that is split'))):
        at = np.flatnonzero(broken)
        if at.size:
            return code, text % (v[at[0]], at[0])
    return OK, ''


def pieces(indptr, rows=None):
    """derive_cut_pieces: (output row, source start, length) of every piece, in output order"""
    indptr = np.asarray(indptr, dtype=np.int64)
    out = []
    for q, r in enumerate(range(indptr.size - 1) if rows is None else rows):
        for lo in range(int(indptr[r]), int(indptr[r + 1]), PIECE):
            out.append((q, lo, min(PIECE, int(indptr[r + 1]) - lo)))
    return out


# the texts of the refusals of a request (rri_derive.hpp), by the name tests/c/derive_main.cpp gives the case
REQUEST_TEXT = {
    'negative_rows_out': 'n_rows_out -1 is negative', 'negative_rows_out_first': 'n_rows_out -7 is negative',
    'negative_cols_out': 'n_cols_out -2 is negative', 'negative_cols_out_first': 'n_cols_out -5 is negative',
    'rows_null_with_count': 'rows is NULL with a count of 3 (NULL takes all rows: the count is 0)',
    'rows_null_with_count_first': 'rows is NULL with a count of 2 (NULL takes all rows: the count is 0)',
    'keep_null_with_count': 'keep is NULL with a count of 3 (NULL keeps all columns: the count is 0)',
    'keep_null_with_count_first': 'keep is NULL with a count of 1 (NULL keeps all columns: the count is 0)',
    'row_negative_at_1': 'rows[1] = -1 is out of range', 'row_5_at_2': 'rows[2] = 5 is out of range',
    'rows_before_keep': 'rows[2] = 5 is out of range',
    'keep_negative_at_0': 'keep[0] = -2 is out of range', 'keep_6_at_2': 'keep[2] = 6 is out of range',
    'range_before_order': 'keep[0] = 3 is out of range',
    'keep_repeats_at_2': 'keep[2] = 2 does not ascend strictly', 'keep_descends_at_1': 'keep[1] = 1 does not ascend strictly',
    'corpus_dead': 'the corpus is NULL or has been destroyed',
    'corpus_elsewhere': 'the corpus lives on device 2, the handle on device 1',
    'corpus_elsewhere_too': 'the corpus lives on device 0, the handle on device 3',
    'threshold_zero': 'threshold 0 holds nothing out: held_out is at least 2^-32',
    'observed_null': 'the output pointer is NULL', 'held_null_first': 'the output pointer is NULL',
}
REQUEST_FINE = ('fine', 'all_rows_all_columns', 'empty_lists', 'corpus_fine', 'split_fine', 'counts_fine', 'no_values')
# the value refusals: name -> the values derive_main.cpp checks
VALUES = {
    'negative_at_2': [1.0, 2.0, -1.0, 3.0], 'negative_at_0': [-3.0, 2.0, -1.0, 3.0], 'half_at_1': [1.0, 0.5, 2.0, 2.25],
    'fraction_at_3': [1.0, 5.0, 2.0, 1048576.5], 'too_large_at_0': [1048577.0, 5.0, 2.0, 3.0], 'too_large_at_3': [1.0, 5.0, 2.0, 2097152.0],
    'negative_before_fraction': [0.5, 5.0, -2.0, 3.0], 'fraction_before_too_large': [4194304.0, 5.0, 2.5, 3.0],
    'negative_fraction_is_negative': [1.0, -0.5, 0.25, 3.0],
}

# row lengths at which a derivation can go wrong: nothing, one entry, both sides of a wave's stride and of its multiples, both
# sides of the piece length (the one border at which the kernels take another path: a second piece), and a full row
GPU_D = 3000
GPU_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, PIECE - 1, PIECE, PIECE + 1, GPU_D, 0, 2 * PIECE - 1, 2 * PIECE, 2 * PIECE + 1, 7,
               3, 12, 40, 5, 1, 0, 9, 30, 2, 64, 200, 17, 1, 4, 6, 8, 10, 11, 13, 90]


def count_corpus(lengths, d, seed, top=9, negatives=False, always=None):
    """A canonical scipy CSR matrix whose row q has lengths[q] entries in random ascending columns: whole counts 1 .. top, or
    (negatives) reals of either sign; `always`: a column every non-empty row holds"""
    rng = np.random.RandomState(seed)
    indptr, indices = [0], []
    for L in lengths:
        if always is not None and L:
            others = np.delete(np.arange(d), always)
            cols = np.sort(np.append(rng.choice(others, size=L - 1, replace=False), always))
        else:
            cols = np.sort(rng.choice(d, size=L, replace=False))
        indices.append(cols)
        indptr.append(indptr[-1] + L)
    indices = np.concatenate(indices + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    data = rng.randint(1, top + 1, size=indices.size).astype(np.float64)
    if negatives:
        data = np.where(rng.rand(indices.size) < 0.3, -1.0, 1.0) * (data + rng.rand(indices.size))
    A = sp.csr_matrix((data, indices, np.array(indptr, dtype=np.int64)), shape=(len(lengths), d))
    assert A.has_canonical_format and np.diff(A.indptr).tolist() == list(lengths)
    return A
