"""The log-likelihood of stored counts under the rows of W T, restated in numpy for the CPU and GPU tests of rri_entries_loglik
(rri_nmf_amd/csrc/rri_loglik.hpp has the definition), the error bound the tests hold the device to, and small generators."""
import numpy as np
import scipy.sparse as sp

LL_SEG = 256                 # rri_loglik.hpp: entries per piece
U = 2.0 ** -52               # twice the unit roundoff of float64: covers the device's and the restatement's side


def lanes(k):
    """rri_loglik.hpp's loglik_lanes: the lanes of a wave that share an entry"""
    return 4 if k <= 128 else 16


def entry_p(W, T, rows, A):
    """p of every stored entry of the canonical CSR A, request by request: einsum over the gathered factors"""
    A = sp.csr_matrix(A)
    rows = np.arange(A.shape[0]) if rows is None else np.asarray(rows)
    req = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return np.einsum('et,te->e', np.asarray(W, dtype=np.float64)[rows[req]], np.asarray(T, dtype=np.float64)[:, A.indices]), req


def reference(W, T, rows, A, floor):
    """(ll, mass, floored, p, bound) of the requests: the three outputs, p per stored entry and the bound on |ll - want| per
    request,  u [2 (k + 2) mass_q + (L_q + 4) sum_e v_e |log p~_e|]  (products of non-negative factors cost at most k + 1
    roundings a side in p, which log turns into an absolute error of that many u; log is good to an ulp; the sum costs at most a
    rounding per term)."""
    A = sp.csr_matrix(A)
    m = A.shape[0]
    p, req = entry_p(W, T, rows, A)
    v = np.asarray(A.data, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        logp = np.log(np.where(p < floor, floor, p))
        term = np.where(v == 0, 0.0, v * logp)
    ll, mass, absl = np.zeros(m), np.zeros(m), np.zeros(m)
    floored = np.zeros(m, dtype=np.int64)
    L = np.diff(A.indptr)
    for q in range(m):                         # in entry order, as the definition has it
        s = slice(A.indptr[q], A.indptr[q + 1])
        ll[q] = np.sum(term[s]) if L[q] else 0.0
        mass[q] = np.sum(v[s]) if L[q] else 0.0
        absl[q] = np.sum(np.abs(term[s])) if L[q] else 0.0
        floored[q] = np.count_nonzero((v[s] > 0) & (p[s] < floor))
    k = np.shape(W)[1]
    bound = U * (2 * (k + 2) * mass + (L + 4) * absl)
    return ll, mass, floored, p, bound


def floor_is_comparable(p, floor):
    """the floored count is only comparable where no p lies within 1e-9 relative of the floor: a condition on the inputs"""
    p = p[np.isfinite(p)]
    return floor == 0 or not np.any(np.abs(p - floor) <= 1e-9 * floor)


def segments(lengths, d, seed, integer=True, zeros=0.0):
    """a CSR matrix whose row q has lengths[q] stored entries at random ascending columns of [0, d): integer counts 1 .. 9 or
    reals in (0, 3), a fraction `zeros` of them explicit zeros"""
    rng = np.random.RandomState(seed)
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(d, size=L, replace=False)) for L in lengths] + [np.zeros(0, dtype=np.int64)])
    nnz = int(indptr[-1])
    data = rng.randint(1, 10, size=nnz).astype(np.float64) if integer else 3.0 * rng.rand(nnz) + 1e-3
    if zeros:
        data[rng.rand(nnz) < zeros] = 0.0
    A = sp.csr_matrix((data, indices.astype(np.int32), indptr), shape=(len(lengths), d))
    assert A.has_canonical_format
    return A


def factors(n, d, k, seed, simplex=False):
    """W (n, k) and T (k, d) of U(0, 1) entries; simplex: rows of T and of W sum to one, so every row of W T does"""
    rng = np.random.RandomState(seed)
    W, T = rng.rand(n, k), rng.rand(k, d)
    if simplex:
        W, T = W / W.sum(axis=1, keepdims=True), T / T.sum(axis=1, keepdims=True)
    return W, T


def disjoint_factors(n, d, k, seed):
    """factors with exact zeros: the rows of W with an even index live on the topics of the lower half and the even columns of T
    on those of the upper half (and the other way round), so p is exactly 0 where row and column have the same parity -- on the
    device and in numpy alike, since every product of the sum is 0 -- and positive elsewhere.  k >= 2."""
    W, T = factors(n, d, k, seed)
    low = np.arange(k) < k // 2
    W[0::2][:, ~low] = 0.0
    W[1::2][:, low] = 0.0
    T[:, 0::2][low] = 0.0
    T[:, 1::2][~low] = 0.0
    return W, T
