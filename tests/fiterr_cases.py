"""The clipped prediction error of W T at the stored entries of a corpus, restated in numpy for the CPU and GPU tests of
rri_corpus_entries_error (rri_nmf_amd/csrc/rri_fiterr.hpp has the definition), the error bounds the tests hold the device to, and
small generators."""
import numpy as np
import scipy.sparse as sp

import loglik_cases as lc

LL_SEG = lc.LL_SEG           # rri_loglik.hpp: entries per piece
U = 2.0 ** -52               # twice the unit roundoff of float64: covers the device's and the restatement's side
INF = float('inf')


def clip(p, lo, hi):
    """rri_fiterr.hpp's fiterr_clip: comparisons, so a NaN passes through and an open side never binds"""
    p = np.asarray(p, dtype=np.float64)
    a = np.where(p < lo, lo, p)
    return np.where(a > hi, hi, a)


def reference(W, T, rows, A, lo=-INF, hi=INF):
    """A dict of the requests' outputs and their bounds: sq, abs (per request), pred (per stored entry), totals (sum sq, sum abs,
    entries, the sums in ascending q) and the bounds sq_bound, abs_bound (per request), pred_bound (per entry).

    With U = 2^-52, a_e = sum_t |W_it| |T_tj| and L entries in the request:
      |pred_e - want| <= (k + 2) U a_e
      |abs - want|    <= U [(k + 2) sum_e a_e + (L + 2) sum_e |r_e|]
      |sq - want|     <= U [2 (k + 2) sum_e |r_e| a_e + (L + 4) sum_e r_e^2] + sum_e ((k + 2) U a_e)^2
    The reasoning: the sum of k products costs at most k + 1 roundings a side in p, whatever its order, so device and
    restatement differ by at most (k + 2) U a_e there (U is twice the unit roundoff; the 2 covers the second-order terms);
    the clip is exact and 1-Lipschitz, so the clipped predictions differ by no more; the subtraction, the square (or the
    absolute value, which is exact) and every addition of the sum cost one rounding each: (L + 2) roundings on sum |r|, (L + 4)
    on sum r^2; and (r + e)^2 - r^2 = 2 r e + e^2 carries the prediction's error e into the square, the last term being
    the e^2 of every entry."""
    A = sp.csr_matrix(A)
    W, T = np.asarray(W, dtype=np.float64), np.asarray(T, dtype=np.float64)
    m, k = A.shape[0], W.shape[1]
    p, req = lc.entry_p(W, T, rows, A)
    rws = np.arange(m) if rows is None else np.asarray(rows)
    a = np.einsum('et,te->e', np.abs(W)[rws[req]], np.abs(T)[:, A.indices])
    v = np.asarray(A.data, dtype=np.float64)
    pred = clip(p, lo, hi)
    r = pred - v
    L = np.diff(A.indptr)
    sq, ab, sra, sa, se2 = (np.zeros(m) for _ in range(5))
    for q in range(m):                         # in entry order, as the definition has it
        s = slice(A.indptr[q], A.indptr[q + 1])
        if L[q]:
            sq[q], ab[q] = np.sum(r[s] ** 2), np.sum(np.abs(r[s]))
            sra[q], sa[q] = np.sum(np.abs(r[s]) * a[s]), np.sum(a[s])
            se2[q] = np.sum(((k + 2) * U * a[s]) ** 2)
    tot_sq = tot_ab = 0.0
    for q in range(m):
        tot_sq += sq[q]
        tot_ab += ab[q]
    return {'sq': sq, 'abs': ab, 'pred': pred, 'totals': (tot_sq, tot_ab, float(A.nnz)),
            'sq_bound': U * (2 * (k + 2) * sra + (L + 4) * sq) + se2, 'abs_bound': U * ((k + 2) * sa + (L + 2) * ab),
            'pred_bound': (k + 2) * U * a}


def check(got, want, what=''):
    """a result of corpus_fit.entries_error (or a dict with sq, abs, pred) against reference() within the bounds"""
    assert np.all(np.abs(got['sq'] - want['sq']) <= want['sq_bound']), (what, 'sq', np.max(np.abs(got['sq'] - want['sq']) - want['sq_bound']))
    assert np.all(np.abs(got['abs'] - want['abs']) <= want['abs_bound']), (what, 'abs', np.max(np.abs(got['abs'] - want['abs']) - want['abs_bound']))
    if got.get('pred') is not None:
        assert np.all(np.abs(got['pred'] - want['pred']) <= want['pred_bound']), (what, 'pred')


def ratings(lengths, d, seed, kind='stars'):
    """a canonical CSR matrix whose row q has lengths[q] stored entries at random ascending columns: 'stars' 1 .. 5, 'real'
    reals of either sign (never 0), 'negative' all below 0"""
    A = lc.segments(lengths, d, seed, integer=True)
    rng = np.random.RandomState(seed + 1000)
    if kind == 'stars':
        A.data[:] = rng.randint(1, 6, size=A.nnz)
    elif kind == 'real':
        A.data[:] = (rng.rand(A.nnz) * 6.0 + 0.25) * np.where(rng.rand(A.nnz) < 0.4, -1.0, 1.0)
    elif kind == 'negative':
        A.data[:] = -(rng.rand(A.nnz) * 4.0 + 0.5)
    else:
        raise ValueError(kind)
    return A


# rows of 0, 1, 3, 255, 256, 257, 771, 0, 64 entries: the piece edges of LL_SEG = 256 (1 + 1 + 1 + 1 + 2 + 4 + 1 = 11 pieces), rows
# without a piece in front and inside, and a last workgroup with dead waves
EDGE_LENGTHS = [0, 1, 3, 255, 256, 257, 771, 0, 64]


def edge_variants():
    """EDGE_LENGTHS and the variants with 1, 2 and 3 one-piece rows dropped: 11, 10, 9 and 8 pieces, every value of the piece
    count mod 4"""
    out = [list(EDGE_LENGTHS)]
    for drop in ([1], [1, 2], [1, 2, 8]):
        out.append([L for i, L in enumerate(EDGE_LENGTHS) if i not in drop])
    return out


def pieces_of(lengths):
    return int(sum(-(-L // LL_SEG) for L in lengths))
