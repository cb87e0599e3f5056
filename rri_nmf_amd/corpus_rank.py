"""Top-N lists, ranks and ranking metrics against resident corpora (include/rri_corpus_rank.h): functions that take an RRIEngine
and DeviceCorpus objects.

    topn_rows(engine, rows, n_top, exclude=None, clip=...)             the n_top best columns of W T per listed row
    rank_entries(engine, targets, rows=None, exclude=None, clip=...)   the rank of every stored entry of `targets` in its row's order
    ranking_metrics(engine, targets, n_items, rows=None, exclude=None, relevant_from=None)
                                                                       the ranking metrics of those ranks, summed on the device
    ranking_sums(...)                                                  the sums themselves, with the kernels' time

`exclude` is a DeviceCorpus of the handle's shape: request q, scoring row rows[q] of W, leaves out the stored columns of row
rows[q] of it -- the whole training corpus is passed as it is for any list of rows.  Nothing of a corpus's size visits the host.
They are functions, not methods: the entry points are declared in a header of their own and typed from a table of their own
(_capi.CORPUS_RANK_PROTOTYPES).
"""
import ctypes as C

import numpy as np

from .corpus_fit import _same_device

METRIC_NAMES = ('hit_rate', 'precision', 'recall', 'ndcg', 'mrr', 'auc', 'mean_percentile_rank')
_I64P, _I32P, _DP = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)


def _exclusion(engine, exclude):
    if exclude is None:
        return None
    _same_device(engine, exclude)
    if tuple(exclude.shape) != (engine.n, engine.d):
        raise ValueError('the exclusion corpus is %d x %d, the handle %d x %d' % (exclude.shape[0], exclude.shape[1], engine.n, engine.d))
    return exclude._ptr()


def _rows(rows, m, what):
    """(array kept alive, pointer) of a row list with one row of W per request"""
    if rows is None:
        return None, None
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
    if m is not None and rows.size != m:
        raise ValueError('rows must name one row of W per %s: %d, not %d' % (what, m, rows.size))
    return rows, rows.ctypes.data_as(_I64P)


def _clip(clip):
    return tuple(float(side) if b is None else float(b) for b, side in zip(clip, ('-inf', 'inf')))


def topn_rows(engine, rows=None, n_top=10, exclude=None, clip=(None, None)):
    """RRIEngine.topn_rows with a resident exclusion (rri_corpus_topn_rows): (idx int32 (m, n_top), val float64 (m, n_top),
    kernel_ms).  rows None: all n rows.  clip = (lo, hi), None leaving a side open."""
    ex = _exclusion(engine, exclude)
    rows, rows_p = _rows(rows, None, 'request')
    m = engine.n if rows is None else rows.size
    n_top = int(n_top)
    lo, hi = _clip(clip)
    idx = np.empty((m, max(n_top, 0)), dtype=np.int32)
    val = np.empty((m, max(n_top, 0)), dtype=np.float64)
    ms = C.c_double(0.0)
    engine._check(engine._lib.rri_corpus_topn_rows(engine._h, rows_p, m, n_top, ex, lo, hi, idx.ctypes.data_as(_I32P), val.ctypes.data_as(_DP),
                                                   C.byref(ms)))
    return idx, val, float(ms.value)


def rank_entries(engine, targets, rows=None, exclude=None, clip=(None, None), values=True):
    """The rank of every stored entry of `targets` (d columns) in the order of topn_rows (rri_corpus_rank_entries).  Request q is
    row q of the corpus scored against row rows[q] of W (rows None: row q).  Returns a dict: rank int32 per canonical entry in
    corpus order (-1: excluded, or a NaN score), val float64 (the clipped score, NaN for such an entry; None with values=False),
    eligible int32 per corpus row (-1 for a row without entries: it is not scored), kernel_ms."""
    _same_device(engine, targets)
    ex = _exclusion(engine, exclude)
    m = targets.shape[0]
    rows, rows_p = _rows(rows, m, 'row of the corpus')
    lo, hi = _clip(clip)
    rank = np.zeros(targets.nnz, dtype=np.int32)
    val = np.zeros(targets.nnz, dtype=np.float64) if values else None
    eligible = np.full(m, -1, dtype=np.int32)
    ms = C.c_double(0.0)
    engine._check(engine._lib.rri_corpus_rank_entries(engine._h, targets._ptr(), rows_p, ex, lo, hi, rank.ctypes.data_as(_I32P),
                                                      val.ctypes.data_as(_DP) if values else None, eligible.ctypes.data_as(_I32P),
                                                      C.byref(ms)))
    return {'rank': rank, 'val': val, 'eligible': eligible, 'kernel_ms': float(ms.value)}


def metrics_from_sums(sums, n_items):
    """the dict NMF_RS_Estimator.ranking_score returns, from the 16 doubles of rri_corpus_ranking_metrics: the division"""
    s = [float(x) for x in sums]
    users, nan = s[0], float('nan')
    out = {'n_items': int(n_items), 'targets': int(s[1]), 'targets_not_eligible': int(s[2]), 'users': int(users)}
    if users == 0:
        out.update((name, nan) for name in METRIC_NAMES)
        return out
    for name, at in zip(METRIC_NAMES[:5], (3, 4, 5, 6, 7)):
        out[name] = s[at] / users
    out['auc'] = s[8] / s[9] if s[9] > 0 else nan
    out['mean_percentile_rank'] = s[10] / s[11] if s[11] > 0 else nan
    return out


def ranking_sums(engine, targets, n_items=10, rows=None, exclude=None, relevant_from=None):
    """(the 16 doubles of rri_corpus_ranking_metrics as a float64 array, kernel_ms): the sums ranking_metrics divides"""
    _same_device(engine, targets)
    ex = _exclusion(engine, exclude)
    rows, rows_p = _rows(rows, targets.shape[0], 'row of the corpus')
    sums, ms = (C.c_double * 16)(), C.c_double(0.0)
    engine._check(engine._lib.rri_corpus_ranking_metrics(engine._h, targets._ptr(), rows_p, ex, int(n_items),
                                                         float('nan') if relevant_from is None else float(relevant_from), sums, C.byref(ms)))
    return np.array(list(sums), dtype=np.float64), float(ms.value)


def ranking_metrics(engine, targets, n_items=10, rows=None, exclude=None, relevant_from=None):
    """The ranking metrics of NMF_RS_Estimator.ranking_score over the stored entries of `targets` whose value is >= relevant_from
    (None: all), ranked and summed on the device (rri_corpus_ranking_metrics): the same dict -- n_items, users, targets,
    targets_not_eligible, hit_rate, precision, recall, ndcg, mrr, auc, mean_percentile_rank; NaN metrics and telling counts when
    nothing is eligible.  A user is a row of the corpus."""
    return metrics_from_sums(ranking_sums(engine, targets, n_items, rows, exclude, relevant_from)[0], n_items)


__all__ = ['topn_rows', 'rank_entries', 'ranking_sums', 'ranking_metrics', 'metrics_from_sums', 'METRIC_NAMES']
