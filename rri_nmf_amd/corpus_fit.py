"""The recommender side of the resident-corpus chain (include/rri_corpus_fit.h): functions that take an RRIEngine and a
DeviceCorpus.

    upload_observed_corpus(engine, corpus)   the observation pattern and ratings of a weighted='sparse' handle from a corpus
    entries_error(engine, corpus, ...)       the clipped prediction error of the handle's W T at the corpus's stored entries
    pattern_of(corpus)                       the corpus's pattern as a scipy CSR matrix of ones (indptr and indices only)

They are functions, not methods: the entry points are declared in a header of their own and typed from a table of their own
(_capi.CORPUS_FIT_PROTOTYPES).  The range of a corpus's values is DeviceCorpus.value_range().
"""
import ctypes as C

import numpy as np

from .engine import DeviceCorpus


def _same_device(engine, corpus):
    if not isinstance(corpus, DeviceCorpus):
        raise TypeError('corpus must be a DeviceCorpus, not %s' % type(corpus).__name__)
    if corpus.device != engine.device:
        raise ValueError('the corpus lives on device %d, the handle on device %d' % (corpus.device, engine.device))


def upload_observed_corpus(engine, corpus):
    """The stored entries of `corpus` (the handle's shape and device) become the observed ones of a weighted='sparse' handle, its
    values X on them (rri_upload_observed_corpus): the canonical arrays are copied device to device and the blocked store is built
    there -- the same bytes as engine.upload_observed_csr(corpus.to_scipy()) leaves, without the download, the host's sorts and the
    uploads.  The corpus is not kept: it may be closed right after the call."""
    _same_device(engine, corpus)
    if tuple(corpus.shape) != (engine.n, engine.d):
        raise ValueError('the corpus is %d x %d, the handle %d x %d' % (corpus.shape[0], corpus.shape[1], engine.n, engine.d))
    engine._check(engine._lib.rri_upload_observed_corpus(engine._h, corpus._ptr()))


def entries_error(engine, corpus, rows=None, clip=(None, None), predictions=False):
    """The clipped prediction error of the handle's current W T at every stored entry of `corpus`, summed per request on the device
    (rri_corpus_entries_error).  Request q is row q of the corpus scored against row rows[q] of W (rows None: row q; duplicates
    and any order are allowed); the corpus has d columns.  clip = (lo, hi), None leaving a side open.  Returns a dict:
    sq, abs (float64 per request: the sums of r^2 and |r| with r = clip(p) - v), pred (the clipped predictions per canonical entry
    when predictions=True, else None), entries, totals = (sum sq, sum abs), added in ascending request order, rmse =
    sqrt(sum sq / entries) and mae = sum abs / entries (NaN without entries), kernel_ms.  Reads the factors and changes nothing; a request returns the same bits alone and among others; row-sharded: local
    rows, no collective."""
    _same_device(engine, corpus)
    m = corpus.shape[0]
    rows_p = None
    if rows is not None:
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        if rows.size != m:
            raise ValueError('rows must name one row of W per row of the corpus: %d, not %d' % (m, rows.size))
        rows_p = rows.ctypes.data_as(C.POINTER(C.c_int64))
    lo, hi = (float(side) if b is None else float(b) for b, side in zip(clip, ('-inf', 'inf')))
    DP = C.POINTER(C.c_double)
    sq, ab = np.zeros(m, dtype=np.float64), np.zeros(m, dtype=np.float64)
    pred = np.zeros(corpus.nnz, dtype=np.float64) if predictions else None
    totals, ms = (C.c_double * 3)(), C.c_double(0.0)
    engine._check(engine._lib.rri_corpus_entries_error(engine._h, corpus._ptr(), rows_p, lo, hi, sq.ctypes.data_as(DP), ab.ctypes.data_as(DP),
                                                       pred.ctypes.data_as(DP) if predictions else None, totals, C.byref(ms)))
    entries = int(totals[2])
    nan = float('nan')
    return {'sq': sq, 'abs': ab, 'pred': pred, 'entries': entries, 'totals': (float(totals[0]), float(totals[1])),
            'rmse': float(np.sqrt(totals[0] / totals[2])) if entries else nan, 'mae': float(totals[1] / totals[2]) if entries else nan,
            'kernel_ms': float(ms.value)}


def pattern_of(corpus):
    """the pattern of a corpus as a scipy CSR matrix of ones: a download of indptr and indices (rri_corpus_get with values NULL)"""
    import scipy.sparse as sp
    indptr = np.zeros(corpus.shape[0] + 1, dtype=np.int64)
    indices = np.zeros(corpus.nnz, dtype=np.int32)
    with corpus._handle() as eng:
        eng._check(corpus._lib.rri_corpus_get(eng._h, corpus._ptr(), indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                              indices.ctypes.data_as(C.POINTER(C.c_int32)), None))
    return sp.csr_matrix((np.ones(indices.size), indices, indptr), shape=corpus.shape)


__all__ = ['upload_observed_corpus', 'entries_error', 'pattern_of']
