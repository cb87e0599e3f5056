"""The matrices of tests/test_spbuild_cpu.py and tests/test_spbuild_gpu.py: the smallest shapes at which the blocked store of a
CSR-X handle changes its layout (rri_nmf_amd/csrc/rri_layout.hpp: sp_dims, build_sp_copy; restated in tests/wsb_cases.py).
A block of a CSR-X handle is at most wsb_cases.SPX_BLOCK_CAP = 15296 wide."""
import numpy as np
import scipy.sparse as sp

import wsb_cases as wc

CAP = wc.SPX_BLOCK_CAP


def one_column_in_every_row(n):
    """n x 3 with column 1 stored in every row: copy 1 has one segment per row block, as long as the block is wide"""
    vals = 0.5 + np.arange(n, dtype=np.float64) % 7
    return sp.csr_matrix((vals, np.ones(n, dtype=np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, 3))


def holes():
    """empty rows, an empty column and a whole empty block: 100 x 15400 is cut into two column blocks of 7744, and nothing is
    stored from column 7744 on"""
    A = wc.pat_density(100, 7000, 0.01, seed=21).tolil()
    A[3:6, :] = 0
    A[:, 11] = 0
    A = sp.csr_matrix(A.tocsr())
    A.eliminate_zeros()
    A = sp.csr_matrix((A.data, A.indices, A.indptr), shape=(100, 15400))
    A.sort_indices()
    return A


def cases():
    """(id, factory of a canonical scipy CSR matrix with float64 values)"""
    out = [('57x33', lambda: wc.pat_density(57, 33, 0.3, seed=11)),
           ('200x15297', lambda: wc.pat_density(200, CAP + 1, 0.01, seed=12)),
           ('15400x40', lambda: wc.pat_density(15400, 40, 0.1, seed=13)),
           ('15296x3-full-column', lambda: one_column_in_every_row(CAP)),
           ('15297x3-full-column', lambda: one_column_in_every_row(CAP + 1))]
    out += [('lps-' + name, make) for name, make, _ in wc._lps_edges()]
    out += [('holes', holes), ('nnz=0', lambda: sp.csr_matrix((20, 30), dtype=np.float64))]
    return out


def expect(A):
    """what the layout must show for the cases above: used by both test files so that a case that lost its point is noticed"""
    return [wc.sp_copy_layout(A, w, 'fp64', True) for w in (0, 1)]
