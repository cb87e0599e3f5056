"""RRIEngine: one device handle (= one nmf() call, or one row shard of it) behind a
small Python object.  All arithmetic happens in librri_hip.so; this class only moves
arguments, resolves the rare reset events and maps status codes to the exceptions
the reference raises (error conventions).

Storage types of X in HBM: float32, float64, and -- for the unweighted flavour in the Gram form on a dense X, where the stored
matrix is only ever read -- float16 (half the bytes of float32 per pass, twice the matrix per card).  The arithmetic is float64
whatever the store, and a float16 value converts to float64 exactly, so a float16 handle solves the float64 problem on
X.astype(float16): one rounding, at upload, none afterwards.  float16 suits magnitudes below 65520 (upload_X raises ValueError
beyond) and data of 11 significant bits: integers up to 2048 are exact; otherwise the relative rounding is 2^-11 above 6.1e-5
and the absolute one 3e-8 below it.  `storage_relerr` says what it came to.
The same handle also stores term counts: uint8, one byte per element, with a float64 scale per row and per column kept beside it.
The X it factorises is (C[i, j] * cscale[j]) * rscale[i], formed in float64 wherever it is read, so tf-idf and row normalisation
are two vector updates (no pass rewrites the matrix) and cost no rounding of the store at all.  upload_X refuses anything but the
integers 0..255; `set_X_scales` / `X_scales` write and read the two vectors.
"""
import collections
import ctypes as C
import re

import numpy as np

from . import _capi
from ._capi import Params, Event

EPS_DIV = float(np.spacing(10))  # nmf.py:52

_NP2RRI = {np.dtype(np.float32): _capi.RRI_F32, np.dtype(np.float64): _capi.RRI_F64, np.dtype(np.float16): _capi.RRI_F16,
           np.dtype(np.uint8): _capi.RRI_U8}
_READ_ONLY = (np.dtype(np.float16), np.dtype(np.uint8))        # stores of a dense X that is only ever read
_HOST_TYPES = (np.dtype(np.float32), np.dtype(np.float64))     # what W, T, masks and CSR values travel as
_RESET_CODES = {None: _capi.RESET_NONE, 'max_resid_document': _capi.RESET_MAX_RESID_DOCUMENT,
                'random': _capi.RESET_RANDOM}


# what RRIEngine.rank_entries returns: the canonical CSR of the targets, rank and val aligned with indices, eligible per request
RankResult = collections.namedtuple('RankResult', 'indptr indices rank val eligible')


class ZeroTotalRows(ValueError):
    """Row normalisation of an X kept as CSR (or as uint8 counts) met `count` rows whose total is below 1e-10 -- empty documents,
    or documents made only of terms that occur in every document (idf 0).  matrixops.normalize makes such a row the dense row
    1/d, which a CSR pattern (or a matrix of counts) cannot take: nothing was rewritten, the handle's X is unchanged."""

    def __init__(self, count):
        ValueError.__init__(self, '%d row(s) of X sum to less than 1e-10: normalisation would make them dense (1/d), which an X '
                                  'kept as CSR or as counts cannot hold; X was left unchanged' % count)
        self.count = int(count)


def _as_host(a, what, half=False, keep=None):
    """C-contiguous float32/float64 view or copy of a matrix (never mutates the caller's); half: a float16 array stays one
    (the X of a float16 handle); keep: another dtype that stays as it is (uint8 for the X of a uint8 handle)"""
    a = np.asarray(a)
    if a.dtype not in _HOST_TYPES and not (half and a.dtype == np.float16) and not (keep is not None and a.dtype == keep):
        a = a.astype(np.float64)
    if a.ndim != 2:
        raise ValueError('%s must be a 2-d array' % what)
    return np.ascontiguousarray(a)


def check_storage_options(dtype, weighted=False, schedule='gram', sparse_x=False):
    """The storage type of a handle against its flavour, before anything touches the library: float32 / float64 for all,
    float16 and uint8 (counts with row and column scales) for the unweighted flavour in the Gram form on a dense X only (the one
    handle whose stored matrix is never rewritten).  Returns the numpy dtype; ValueError names what does not combine."""
    dt = np.dtype(dtype)
    if dt not in _NP2RRI:
        raise ValueError('dtype must be float32, float64 or float16 (or uint8 for counts 0..255)')
    if dt in _READ_ONLY:
        refused = [name for name, on in (('weighted=%r' % (weighted,), bool(weighted)),
                                         ("schedule='residual'", schedule == 'residual'),
                                         ('sparse_x=True', bool(sparse_x))) if on]
        if refused:
            raise ValueError('dtype=%s stores a dense X that is only read (unweighted, schedule=\'gram\'); it does not '
                             'combine with %s' % (dt.name, ', '.join(refused)))
    return dt


class FrozenRows(object):
    """Rows that left the device, as the sums a T-row step sees of them: B = W_O^T X_O (k, d), A = W_O^T W_O (k, k),
    s = 1^T W_O (k,), c = ||X_O||^2, and how many rows went in.  Float64 copies; a value, never changed in place:
    `decay(rho)` scales the four sums (the count stays), `+` adds two sets of rows of the same model."""

    def __init__(self, B, A, s, c, rows=0):
        self.B = np.array(B, dtype=np.float64, ndmin=2)
        self.A = np.array(A, dtype=np.float64, ndmin=2)
        self.s = np.array(s, dtype=np.float64).reshape(-1)
        self.c = float(c)
        self.rows = int(rows)
        k = self.s.size
        if self.A.shape != (k, k) or self.B.shape[0] != k:
            raise ValueError('B must be (k, d), A (k, k) and s (k,): got %r, %r, %r' % (self.B.shape, self.A.shape, self.s.shape))

    k = property(lambda self: self.s.size)
    d = property(lambda self: self.B.shape[1])

    @classmethod
    def zeros(cls, k, d):
        return cls(np.zeros((k, d)), np.zeros((k, k)), np.zeros(k), 0.0, 0)

    @classmethod
    def of(cls, X, W):
        """the statistics of the rows X (dense or scipy sparse) with the factors W, on the host"""
        X = X.toarray() if hasattr(X, 'toarray') else np.asarray(X, dtype=np.float64)
        W = np.asarray(W, dtype=np.float64)
        return cls(W.T.dot(X), W.T.dot(W), W.sum(0), float((X ** 2).sum()), X.shape[0])

    def decay(self, rho):
        if not 0.0 < rho <= 1.0:
            raise ValueError('decay %r is outside (0, 1]' % (rho,))
        return FrozenRows(rho * self.B, rho * self.A, rho * self.s, rho * self.c, self.rows)

    def __add__(self, other):
        if not isinstance(other, FrozenRows):
            return NotImplemented
        if (self.k, self.d) != (other.k, other.d):
            raise ValueError('frozen statistics of different shapes: k, d = %r and %r' % ((self.k, self.d), (other.k, other.d)))
        return FrozenRows(self.B + other.B, self.A + other.A, self.s + other.s, self.c + other.c, self.rows + other.rows)

    def objective_share(self, T):
        """the frozen rows' share of the stacked objective 1/2 ||X - W T||^2: 1/2 (c - 2 <B, T> + <A, T T^T>)"""
        T = np.asarray(T, dtype=np.float64)
        return 0.5 * ((self.c - 2.0 * (self.B * T).sum()) + (self.A * T.dot(T.T)).sum())


def device_memory():
    """(buffers, bytes) of the device allocations that the handles of this process own right now (rri_device_memory): bound
    tensors and the temporaries of a call are not counted, and after every close() both are back where they were."""
    buffers, nbytes = C.c_int64(0), C.c_int64(0)
    _capi.load_library().rri_device_memory(C.byref(buffers), C.byref(nbytes))
    return int(buffers.value), int(nbytes.value)


def corpus_memory():
    """(corpora, bytes) of the DeviceCorpus objects alive in this process and their device bytes (rri_corpus_memory): they belong
    to no handle, so device_memory() does not count them, and after every close() both are back where they were."""
    corpora, nbytes = C.c_int64(0), C.c_int64(0)
    _capi.load_library().rri_corpus_memory(C.byref(corpora), C.byref(nbytes))
    return int(corpora.value), int(nbytes.value)


_INDEX_CODES = {'int32': _capi.RRI_I32, 'int64': _capi.RRI_I64}
_VALUE_CODES = {'float32': _capi.RRI_F32, 'float64': _capi.RRI_F64}


class DeviceCorpus(object):
    """A sparse corpus that lives on the device: checked and made canonical there, once (rri_corpus_create), and then taken by
    RRIEngine.cooccurrence_counts / entries_loglik and NMF_TM_Estimator.coherence / log_likelihood / perplexity in place of the
    scipy matrix, without the host's canonical copy and the upload of every call.

    X is a scipy sparse matrix (its arrays travel as they are: unsorted rows, duplicates and explicit zeros are dealt with on the
    device), a dense array (converted to CSR on the host first, the slow way in) or a torch sparse-CSR tensor on the GPU, whose
    arrays are read where they are (the corpus then lives on the tensor's device, whatever `device` says).  `from_device` takes the
    three arrays as GPU tensors, `from_arrays` raw host arrays.  The canonical form: per row strictly
    ascending columns, the stored entries of one column added in float64 in stored order, sums that are exactly 0 dropped; int32
    indices, float64 values.  ValueError names the first broken rule of a malformed matrix (a column out of range, a NaN, an
    indptr that decreases ...), NotImplementedError 2^31 columns or more.

    shape; nnz (canonical entries); stored (entries as given); rows_rewritten, duplicates_merged, zeros_dropped (stored = nnz +
    duplicates_merged + zeros_dropped); negatives (canonical values below 0: entries_loglik refuses such a corpus); device_bytes;
    long_rows; ingest_ms (the HIP-event time of the ingest's kernels); device.  The corpus belongs to no handle: it serves every
    RRIEngine on its device until close() (also: a context manager), and corpus_memory() counts it, device_memory() does not.

    New corpora are derived from it on the device, the source staying as it is: take_rows(rows) and corpus[a:b] / corpus[mask] /
    corpus[index_array] (row subsets, any order, repeats), select_words(keep), document_frequency(), prune_words(min_df, max_df,
    max_words) and split_counts(held_out, random_state) (include/rri_corpus_ops.h).  The two ends of that chain are on the device as
    well (include/rri_corpus_build.h): from_pairs(pairs, values) makes a corpus of (row, column, value) triples -- tokens, or a
    ratings log -- without a CSR matrix on the host, and split_entries(held_out, random_state) sends every entry, whole, to a
    training or a held-out corpus; split_rows(n_held | held_out, min_observed, random_state) holds out an exact number of entries
    of every row instead (include/rri_corpus_rowsplit.h).  value_range() is the (min, max) of the values, and the recommender fit takes a corpus where
    it lies (include/rri_corpus_fit.h; corpus_fit.upload_observed_corpus, corpus_fit.entries_error, nmf(corpus, k,
    observed_only=True), NMF_RS_Estimator.fit_corpus)."""

    def __init__(self, X, device=0):
        import scipy.sparse as sp
        self._c = C.c_void_p()
        if hasattr(X, 'crow_indices') and hasattr(X, 'col_indices'):          # a torch sparse-CSR tensor
            self._ingest_device(X.crow_indices(), X.col_indices(), X.values(), tuple(X.shape), None)      # where the tensor lives
            return
        A = X.tocsr() if sp.issparse(X) else sp.csr_matrix(np.asarray(X))
        if not sp.isspmatrix_csr(A):
            A = sp.csr_matrix(A)
        self._ingest_host(A.indptr, A.indices, A.data, A.shape, device)

    @classmethod
    def from_arrays(cls, indptr, indices, values, shape, device=0):
        """The corpus of three host arrays as they are -- what a scipy matrix holds, without scipy's own look at them: indptr and
        indices int32 or int64 (other integers are widened), values float32 or float64 (others become float64) or None for a
        pattern.  They are uploaded raw and checked on the device."""
        self = cls.__new__(cls)
        self._c = C.c_void_p()
        self._ingest_host(indptr, indices, values, shape, device)
        return self

    def _ingest_host(self, indptr, indices, values, shape, device):
        indptr, indices = (np.ascontiguousarray(a if a.dtype.name in _INDEX_CODES else a.astype(np.int64))
                           for a in (np.asarray(indptr).reshape(-1), np.asarray(indices).reshape(-1)))
        if values is not None:
            values = np.asarray(values).reshape(-1)
            values = np.ascontiguousarray(values if values.dtype.name in _VALUE_CODES else values.astype(np.float64))
            if values.size != indices.size:
                raise ValueError('values must have as many entries as indices (%d)' % indices.size)
        if len(shape) != 2 or indptr.size != int(shape[0]) + 1:
            raise ValueError('indptr must have shape[0] + 1 = %d entries' % (int(shape[0]) + 1))
        self._ingest(shape, int(indices.size), indptr.ctypes.data, _INDEX_CODES[indptr.dtype.name], indices.ctypes.data,
                     _INDEX_CODES[indices.dtype.name], values.ctypes.data if values is not None else None,
                     _VALUE_CODES[values.dtype.name] if values is not None else _capi.RRI_F64, 0, device, (indptr, indices, values))

    @classmethod
    def from_device(cls, indptr, indices, values, shape, device=None):
        """The corpus of three one-dimensional GPU tensors (anything with data_ptr(), dtype, device and numel(): torch tensors):
        indptr int32 / int64 with shape[0] + 1 entries, indices int32 / int64, values float32 / float64 or None for a pattern
        (every stored entry counts 1).  They are read during the call and not kept.  torch tensors' device is synchronised first;
        whoever hands over other objects has synchronised what produced them."""
        self = cls.__new__(cls)
        self._c = C.c_void_p()
        self._ingest_device(indptr, indices, values, tuple(shape), device)
        return self

    def _ingest_device(self, indptr, indices, values, shape, device):
        def code(t, table, what):
            name = str(t.dtype).split('.')[-1]
            if name not in table:
                raise TypeError('%s must be %s, not %s' % (what, ' or '.join(sorted(table)), t.dtype))
            return table[name]
        tensors = [t for t in (indptr, indices, values) if t is not None]
        tensors = [t.contiguous() if hasattr(t, 'contiguous') else t for t in tensors]
        index = {getattr(t.device, 'index', None) for t in tensors}
        if any(getattr(t.device, 'type', 'cuda') != 'cuda' for t in tensors) or len(index) != 1:
            raise ValueError('indptr, indices and values must be GPU tensors on one device')
        dev = index.pop()
        dev = 0 if dev is None else int(dev)
        if device is not None and int(device) != dev:
            raise ValueError('the tensors live on device %d, not on device %d' % (dev, int(device)))
        if len(shape) != 2 or int(tensors[0].numel()) != int(shape[0]) + 1:
            raise ValueError('indptr must have shape[0] + 1 = %d entries' % (int(shape[0]) + 1))
        nnz = int(tensors[1].numel())
        if values is not None and int(tensors[2].numel()) != nnz:
            raise ValueError('values must have as many entries as indices (%d)' % nnz)
        if type(tensors[0]).__module__.split('.')[0] == 'torch':
            import torch
            torch.cuda.synchronize(dev)
        self._ingest(shape, nnz, tensors[0].data_ptr(), code(tensors[0], _INDEX_CODES, 'indptr'), tensors[1].data_ptr(),
                     code(tensors[1], _INDEX_CODES, 'indices'), tensors[2].data_ptr() if values is not None else None,
                     code(tensors[2], _VALUE_CODES, 'values') if values is not None else _capi.RRI_F64, 1, dev, tensors)

    def _ingest(self, shape, stored, indptr, pdt, indices, idt, values, vdt, on_device, device, keep_alive):
        self._lib = _capi.load_library()
        self.device = int(device)
        self.shape = (int(shape[0]), int(shape[1]))
        with self._handle() as eng:
            eng._check(self._lib.rri_corpus_create(eng._h, C.byref(self._c), self.shape[0], self.shape[1], stored,
                                                   C.c_void_p(indptr), pdt, C.c_void_p(indices or None), idt,
                                                   C.c_void_p(values or None), vdt, on_device))
        del keep_alive
        self._read_info()

    @classmethod
    def from_pairs(cls, pairs, values=None, shape=None, cols=None, device=0):
        """The corpus of a list of (row, column, value) pairs, built on the device (rri_corpus_from_pairs, include/
        rri_corpus_build.h): `pairs` is an (m, 2) integer array -- an estimator's index_pairs, read where it lies when it is
        C-contiguous int32 or int64 -- or a one-dimensional array of rows with `cols=` for the columns; `values` one number per
        pair (float32 / float64; others become float64) or None: every pair counts 1, so (document, word) tokens become term
        counts.  The inputs are numpy arrays, or GPU tensors in the sense of from_device (data_ptr(), dtype, device, numel();
        torch's device is synchronised first), which are read where they are: the corpus then lives on the tensors' device.  It is
        the corpus DeviceCorpus makes of the CSR matrix whose row i holds the pairs of row i in the order given: the values of
        one (i, j) are added in float64 in that order, a sum that is exactly 0 is dropped.  shape=None is allowed for host arrays
        only: (max row + 1, max column + 1), and (0, 0) for an empty list.  ValueError names the first pair that is out of range or
        not finite; NotImplementedError 2^31 columns or more."""
        self = cls.__new__(cls)
        self._c = C.c_void_p()
        idt, n_pairs, rp, cp, vp, vdt, stride, on_device, dev, keep_alive = cls._pairs_arguments(pairs, values, cols, device)
        if shape is None:
            if on_device:
                raise ValueError('device tensors need shape=(n_rows, n_cols): the largest index is not looked for on the device')
            r, c_ = keep_alive[0], keep_alive[1]
            shape = (int(r.max()) + 1, int(c_.max()) + 1) if r.size else (0, 0)
        if len(shape) != 2:
            raise ValueError('shape must be (n_rows, n_cols)')
        self._lib = _capi.load_library()
        self.device = int(dev)
        self.shape = (int(shape[0]), int(shape[1]))
        with self._handle() as eng:
            eng._check(self._lib.rri_corpus_from_pairs(eng._h, C.byref(self._c), self.shape[0], self.shape[1], n_pairs, C.c_void_p(rp or None),
                                                       C.c_void_p(cp or None), idt, stride, C.c_void_p(vp or None), vdt, on_device))
        del keep_alive
        self._read_info()
        return self

    @staticmethod
    def _pairs_arguments(pairs, values, cols, device):
        """what rri_corpus_from_pairs is handed: (index dtype code, n_pairs, rows pointer, cols pointer, values pointer, values dtype
        code, index stride, on_device, device, what must stay alive during the call -- the row and column views first)"""
        def code(t, table, what):
            name = str(t.dtype).split('.')[-1]
            if name not in table:
                raise TypeError('%s must be %s, not %s' % (what, ' or '.join(sorted(table)), t.dtype))
            return table[name]
        on_device = hasattr(pairs, 'data_ptr')
        if on_device:
            tensors = [t for t in (pairs, cols, values) if t is not None]
            if not all(hasattr(t, 'data_ptr') for t in tensors):
                raise ValueError('pairs, cols and values must all be GPU tensors, or all host arrays')
            tensors = [t.contiguous() if hasattr(t, 'contiguous') else t for t in tensors]
            index = {getattr(t.device, 'index', None) for t in tensors}
            if any(getattr(t.device, 'type', 'cuda') != 'cuda' for t in tensors) or len(index) != 1:
                raise ValueError('pairs, cols and values must be GPU tensors on one device')
            dev = index.pop()
            dev = 0 if dev is None else int(dev)
            p = tensors[0]
            idt, isz = code(p, _INDEX_CODES, 'pairs'), 4 if str(p.dtype).split('.')[-1] == 'int32' else 8
            dims = tuple(getattr(p, 'shape', (int(p.numel()),)))
            if cols is None:
                if len(dims) != 2 or int(dims[1]) != 2:
                    raise ValueError('pairs must be an (m, 2) array of (row, column) indices, or rows with cols=')
                n_pairs, stride, rp, cp = int(dims[0]), 2, p.data_ptr(), p.data_ptr() + isz
            else:
                q = tensors[1]
                if len(dims) != 1 or code(q, _INDEX_CODES, 'cols') != idt or int(q.numel()) != int(p.numel()):
                    raise ValueError('rows and cols must be one-dimensional, of one dtype and one length')
                n_pairs, stride, rp, cp = int(p.numel()), 1, p.data_ptr(), q.data_ptr()
            v = tensors[-1] if values is not None else None
            if v is not None and int(v.numel()) != n_pairs:
                raise ValueError('values must have one entry per pair (%d)' % n_pairs)
            if type(p).__module__.split('.')[0] == 'torch':
                import torch
                torch.cuda.synchronize(dev)
            return (idt, n_pairs, rp if n_pairs else None, cp if n_pairs else None, v.data_ptr() if v is not None and n_pairs else None,
                    code(v, _VALUE_CODES, 'values') if v is not None else _capi.RRI_F64, stride, 1, dev, tensors)
        p = np.asarray(pairs)
        if p.size and p.dtype.kind not in 'iu':
            raise ValueError('pairs must be integers, not %s' % p.dtype)
        if p.dtype.name not in _INDEX_CODES:
            p = p.astype(np.int64)
        if cols is None:
            if p.ndim != 2 or p.shape[1] != 2:
                raise ValueError('pairs must be an (m, 2) array of (row, column) indices, or rows with cols=')
            p = np.ascontiguousarray(p)                 # no copy of a C-contiguous int32 / int64 array: read with a stride of 2
            r, q, stride = p[:, 0], p[:, 1], 2
        else:
            q = np.asarray(cols)
            if q.size and q.dtype.kind not in 'iu':
                raise ValueError('cols must be integers, not %s' % q.dtype)
            if p.ndim != 1 or q.ndim != 1 or p.size != q.size:
                raise ValueError('rows and cols must be one-dimensional and of one length')
            if q.dtype != p.dtype:                      # one dtype for both: the wider
                p, q = p.astype(np.int64), q.astype(np.int64)
            r, q, stride = np.ascontiguousarray(p), np.ascontiguousarray(q), 1
        n_pairs = int(r.shape[0])
        v = None
        if values is not None:
            v = np.asarray(values).reshape(-1)
            v = np.ascontiguousarray(v if v.dtype.name in _VALUE_CODES else v.astype(np.float64))
            if v.size != n_pairs:
                raise ValueError('values must have one entry per pair (%d)' % n_pairs)
        return (_INDEX_CODES[r.dtype.name], n_pairs, r.ctypes.data if n_pairs else None, q.ctypes.data if n_pairs else None,
                v.ctypes.data if v is not None and n_pairs else None, _VALUE_CODES[v.dtype.name] if v is not None else _capi.RRI_F64,
                stride, 0, int(device), (r, q, v, p))

    def split_entries(self, held_out=0.05, random_state=0):
        """(observed, held), two corpora on the same device: every entry goes, whole and bit for bit, to `held` with probability
        floor(held_out 2^32) / 2^32 and to `observed` otherwise (rri_corpus_split_entries) -- the split of observed ratings into a
        training and a held-out part.  The values may be negative or fractional; the two patterns are disjoint and their union is
        this corpus's.  The generator is split_counts's (Philox4x32-10 keyed by random_state, counted by (column, row)), so the
        split depends on (row, column, seed) alone and an entry whose count is 1 goes the same way in both."""
        thr, seed = self._split_threshold(held_out), self._split_seed(random_state)
        observed, held = C.c_void_p(), C.c_void_p()
        with self._handle() as eng:
            eng._check(self._lib.rri_corpus_split_entries(eng._h, self._ptr(), thr, seed, C.byref(observed), C.byref(held)))
        return DeviceCorpus._adopt(observed, self.device, self._lib), DeviceCorpus._adopt(held, self.device, self._lib)

    @staticmethod
    def _split_rows_request(n_held, held_out, min_observed):
        """what rri_corpus_split_rows is handed for the two modes of split_rows: (n_held or -1, fraction or 0.0, min_observed);
        ValueError / TypeError before any device call"""
        def whole(v, what):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError('%s must be an int, not %r' % (what, v))
            return int(v)
        if (n_held is None) == (held_out is None):
            raise ValueError('split_rows takes exactly one of n_held (a count per row) and held_out (a share of every row), not %s'
                             % ('both' if n_held is not None else 'neither'))
        min_observed = whole(min_observed, 'min_observed')
        if not 0 <= min_observed < (1 << 63):
            raise ValueError('min_observed must be at least 0, not %r' % (min_observed,))
        if n_held is not None:
            n_held = whole(n_held, 'n_held')
            if not 1 <= n_held < (1 << 63):
                raise ValueError('n_held must be at least 1, not %r' % (n_held,))
            return n_held, 0.0, min_observed
        if isinstance(held_out, (bool, np.bool_)) or not isinstance(held_out, (int, float, np.integer, np.floating)):
            raise TypeError('held_out must be a number in (0, 1], not %r' % (held_out,))
        if not 0.0 < float(held_out) <= 1.0:
            raise ValueError('held_out must lie inside (0, 1], not %r' % (held_out,))
        return -1, float(held_out), min_observed

    @staticmethod
    def _split_rows_quota(lengths, n_held, fraction, min_observed):
        """rowsplit_quota for an array of row lengths and a checked request (n_held or -1, fraction): what every row gives up"""
        L = np.asarray(lengths, dtype=np.int64)
        want = np.full(L.shape, n_held, dtype=np.int64) if n_held >= 1 else np.floor(fraction * L.astype(np.float64) + 0.5).astype(np.int64)
        return np.minimum(want, np.maximum(L - min_observed, 0))

    def split_rows(self, n_held=None, held_out=None, min_observed=1, random_state=0):
        """(observed, held), two corpora on the same device: every row gives up an exact number of its entries, whole and bit for bit
        (rri_corpus_split_rows, include/rri_corpus_rowsplit.h).  Exactly one of n_held (every row gives up n_held entries: leave-k-out)
        and held_out (a row of L entries gives up floor(held_out L + 0.5)) is given; either way a row keeps at least min_observed
        entries, giving up fewer -- or none -- where it is short: h = min(want, max(L - min_observed, 0)).  The entries given up are
        those with the smallest keys (Philox word << 32 | column), the Philox word being split_entries's for (row, column,
        random_state): for one seed the held set for h is inside that for h + 1, and where split_entries holds m entries of a row,
        a quota of m holds the same ones.  The two patterns are disjoint and their union is this corpus's."""
        n_held, fraction, min_observed = self._split_rows_request(n_held, held_out, min_observed)
        seed = self._split_seed(random_state)
        observed, held = C.c_void_p(), C.c_void_p()
        with self._handle() as eng:
            eng._check(self._lib.rri_corpus_split_rows(eng._h, self._ptr(), n_held, fraction, min_observed, seed, C.byref(observed),
                                                       C.byref(held)))
        return DeviceCorpus._adopt(observed, self.device, self._lib), DeviceCorpus._adopt(held, self.device, self._lib)

    def _read_info(self):
        info, ms = (C.c_int64 * _capi.RRI_CORPUS_INFO_FIELDS)(), C.c_double(0.0)
        self._lib.rri_corpus_info(self._c, info, _capi.RRI_CORPUS_INFO_FIELDS, C.byref(ms))
        (n_rows, n_cols, self.stored, self.nnz, self.rows_rewritten, self.duplicates_merged, self.zeros_dropped, self.negatives,
         self.device_bytes, self.long_rows) = (int(v) for v in info)
        self.shape = (n_rows, n_cols)
        self.ingest_ms = float(ms.value)

    @classmethod
    def _adopt(cls, c, device, lib):
        """the DeviceCorpus of a corpus the library has just made (rri_corpus_select, rri_corpus_split)"""
        self = cls.__new__(cls)
        self._c, self._lib, self.device = c, lib, int(device)
        self._read_info()
        return self

    # ---- corpora derived on the device (include/rri_corpus_ops.h): the source is never modified, nothing of its size visits the host
    @staticmethod
    def _rows_of_index(index, n):
        """what corpus[index] asks of take_rows: a slice (a step too), an int, a boolean mask of length n or an array of ints,
        negative ones counting from the end as in numpy: the int64 row numbers"""
        if isinstance(index, slice):
            return np.arange(*index.indices(n), dtype=np.int64)
        idx = np.asarray(index)
        if idx.ndim > 1:
            raise IndexError('a corpus is indexed by rows: a slice, an int, a mask or a one-dimensional array of ints')
        if idx.dtype == np.bool_:
            if idx.shape != (n,):
                raise IndexError('a boolean mask of rows must have length %d, not %r' % (n, idx.shape))
            return np.flatnonzero(idx).astype(np.int64)
        if idx.size and idx.dtype.kind not in 'iu':
            raise IndexError('row numbers must be integers, not %s' % idx.dtype)
        idx = idx.reshape(-1).astype(np.int64)
        if idx.size and (idx.min() < -n or idx.max() >= n):
            raise IndexError('row %d is out of range for %d rows' % (idx[(idx < -n) | (idx >= n)][0], n))
        return np.where(idx < 0, idx + n, idx)

    @staticmethod
    def _keep_of(keep, d):
        """what select_words takes: ascending columns, or a boolean mask of length d: the int32 columns"""
        keep = np.asarray(keep)
        if keep.dtype == np.bool_:
            if keep.shape != (d,):
                raise ValueError('a boolean mask of words must have length %d, not %r' % (d, keep.shape))
            return np.flatnonzero(keep).astype(np.int32)
        if keep.size and keep.dtype.kind not in 'iu':
            raise ValueError('columns must be integers, not %s' % keep.dtype)
        keep = keep.reshape(-1).astype(np.int64)
        if keep.size and (keep.min() < 0 or keep.max() >= d):
            raise ValueError('column %d is out of range for %d columns' % (keep[(keep < 0) | (keep >= d)][0], d))
        return keep.astype(np.int32)

    @staticmethod
    def _prune_selection(df, n_rows, min_df=1, max_df=1.0, max_words=None):
        """the columns prune_words keeps, ascending (int32), from the document frequencies: lo <= df <= hi, an int bound being a
        number of documents and a float in [0, 1] a share of the rows; where more than max_words remain, those of the largest df,
        a tie going to the lower column"""
        def bound(b, what):
            if isinstance(b, (float, np.floating)):
                if not 0.0 <= b <= 1.0:
                    raise ValueError('%s = %r: a float bound is a share of the rows in [0, 1]' % (what, b))
                return b * n_rows
            if int(b) < 0:
                raise ValueError('%s = %r is negative' % (what, b))
            return int(b)
        df = np.asarray(df, dtype=np.int64)
        lo, hi = bound(min_df, 'min_df'), bound(max_df, 'max_df')
        kept = np.flatnonzero((df >= lo) & (df <= hi))
        if max_words is not None:
            if int(max_words) < 0:
                raise ValueError('max_words = %r is negative' % (max_words,))
            if kept.size > int(max_words):        # stable on ascending columns: equal df keeps the lower column first
                kept = np.sort(kept[np.argsort(-df[kept], kind='stable')[:int(max_words)]])
        return kept.astype(np.int32)

    @staticmethod
    def _split_threshold(held_out):
        """floor(held_out 2^32): the share of the tokens that is held out is this over 2^32"""
        if not 0.0 < held_out < 1.0:
            raise ValueError('held_out must lie inside (0, 1), not %r' % (held_out,))
        thr = int(np.floor(float(held_out) * 4294967296.0))
        if thr < 1:
            raise ValueError('held_out = %r is below 2^-32: nothing would be held out' % (held_out,))
        return thr

    @staticmethod
    def _split_seed(random_state):
        """the 64-bit seed: an int in [0, 2^64), or two 32-bit words of a RandomState (low word first)"""
        if isinstance(random_state, np.random.RandomState):
            lo, hi = (int(v) for v in random_state.randint(0, 1 << 32, size=2, dtype=np.uint64))
            return lo | (hi << 32)
        if isinstance(random_state, (bool, np.bool_)) or not isinstance(random_state, (int, np.integer)):
            raise TypeError('random_state must be an int in [0, 2^64) or a numpy RandomState, not %r' % (random_state,))
        if not 0 <= int(random_state) < (1 << 64):
            raise ValueError('random_state %r is outside [0, 2^64)' % (random_state,))
        return int(random_state)

    def _select(self, rows, keep):
        """rri_corpus_select: rows None (all) or int64 row numbers, keep None (all) or ascending int32 columns"""
        def arg(a, dtype, ctype):
            if a is None:
                return None, None, 0
            a = np.ascontiguousarray(a, dtype=dtype)
            hold = a if a.size else np.zeros(1, dtype=dtype)        # an empty list is a list: not NULL
            return hold, hold.ctypes.data_as(C.POINTER(ctype)), int(a.size)
        hold_r, rp, m = arg(rows, np.int64, C.c_int64)
        hold_k, kp, dk = arg(keep, np.int32, C.c_int32)
        out = C.c_void_p()
        with self._handle() as eng:
            eng._check(self._lib.rri_corpus_select(eng._h, self._ptr(), rp, m, kp, dk, C.byref(out)))
        del hold_r, hold_k
        return DeviceCorpus._adopt(out, self.device, self._lib)

    def take_rows(self, rows):
        """A new corpus of the rows `rows` (row numbers in [0, n), any order, repeats allowed) in that order, on the same device
        (rri_corpus_select): the canonical form of A[rows], without a download or an upload of the entries."""
        rows = np.asarray(rows)
        if rows.size and rows.dtype.kind not in 'iu':
            raise ValueError('row numbers must be integers, not %s' % rows.dtype)
        return self._select(rows.reshape(-1).astype(np.int64), None)

    def __getitem__(self, index):
        """corpus[a:b], corpus[a:b:s], corpus[i], corpus[mask], corpus[index_array]: take_rows of those rows"""
        return self._select(self._rows_of_index(index, self.shape[0]), None)

    def select_words(self, keep):
        """A new corpus of the columns `keep` -- ascending columns, or a boolean mask of length d --, renumbered to their places
        in keep, on the same device: the canonical form of A[:, keep]."""
        return self._select(None, self._keep_of(keep, self.shape[1]))

    def document_frequency(self):
        """(d,) int64: the rows with an entry in each column, counted on the device (rri_corpus_column_counts)"""
        df = np.zeros(self.shape[1], dtype=np.int64)
        with self._handle() as eng:
            eng._check(self._lib.rri_corpus_column_counts(eng._h, self._ptr(), df.ctypes.data_as(C.POINTER(C.c_int64))))
        return df

    def prune_words(self, min_df=1, max_df=1.0, max_words=None):
        """(corpus, kept): the corpus of the words whose document frequency lies in [min_df, max_df] -- an int is a number of
        documents, a float in [0, 1] a share of the rows -- and, where more than max_words remain, of those with the largest
        document frequency (a tie goes to the lower column); kept: their source columns, ascending.  The decision over the
        d-sized frequency vector is made on the host; the entries stay on the device."""
        kept = self._prune_selection(self.document_frequency(), self.shape[0], min_df, max_df, max_words)
        return self.select_words(kept), kept

    def split_counts(self, held_out=0.5, random_state=0):
        """(observed, held), two corpora on the same device with observed + held == this corpus of counts: every token goes to
        `held` with probability floor(held_out 2^32) / 2^32, independently, by a counter-based generator (Philox4x32-10) keyed
        by random_state -- an int in [0, 2^64), or a RandomState that supplies two 32-bit words -- and counted by (column, row),
        so the split depends on (row, column, count, seed) alone (rri_corpus_split).  ValueError for a held_out outside (0, 1)
        or below 2^-32 and for values that are negative or not whole; NotImplementedError for a count above 2^20."""
        thr, seed = self._split_threshold(held_out), self._split_seed(random_state)
        observed, held = C.c_void_p(), C.c_void_p()
        with self._handle() as eng:
            eng._check(self._lib.rri_corpus_split(eng._h, self._ptr(), thr, seed, C.byref(observed), C.byref(held)))
        return DeviceCorpus._adopt(observed, self.device, self._lib), DeviceCorpus._adopt(held, self.device, self._lib)

    def _handle(self):
        """a handle for the device, the stream and the error text: it holds nothing of the corpus's size"""
        return RRIEngine(1, 1, 1, dtype=np.float64, weighted=False, device=self.device)

    def _ptr(self):
        if not self._c:
            raise ValueError('the corpus is closed')
        return self._c

    def to_scipy(self):
        """the canonical matrix as a scipy CSR matrix with float64 data (scipy picks the index dtype): a download"""
        import scipy.sparse as sp
        indptr = np.zeros(self.shape[0] + 1, dtype=np.int64)
        indices = np.zeros(self.nnz, dtype=np.int32)
        values = np.zeros(self.nnz, dtype=np.float64)
        with self._handle() as eng:
            eng._check(self._lib.rri_corpus_get(eng._h, self._ptr(), indptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                indices.ctypes.data_as(C.POINTER(C.c_int32)), values.ctypes.data_as(C.POINTER(C.c_double))))
        return sp.csr_matrix((values, indices, indptr), shape=self.shape)

    def value_range(self):
        """(min, max) of the canonical values, reduced on the device (rri_corpus_value_range, include/rri_corpus_fit.h): the rating
        range of a ratings corpus, without a download.  ValueError for an empty corpus."""
        out = (C.c_double * 2)()
        with self._handle() as eng:
            eng._check(self._lib.rri_corpus_value_range(eng._h, self._ptr(), out))
        return float(out[0]), float(out[1])

    def close(self):
        if getattr(self, '_c', None) is not None and self._c:
            self._lib.rri_corpus_destroy(self._c)
            self._c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RRIEngine(object):
    def __init__(self, n, d, k, dtype=np.float32, weighted=False, device=0, stream=None, schedule='gram', sparse_x=False):
        """schedule (unweighted handles): 'gram' -- the residual is never formed, one read of X per topic step
        (the reference's form, nmf.py:670-676, 728-734) -- or 'residual' -- R = X - W T is kept in HBM and every topic
        step is one rank-one residual update pass fused with the residual products (RRI_UNWEIGHTED_RESIDUAL).
        sparse_x (unweighted, 'gram'): X stays CSR on the device (RRI_UNWEIGHTED_SPARSE) -- upload_X_csr keeps it so, and
        there is no dense n x d array at all"""
        self.dtype = check_storage_options(dtype, weighted, schedule, sparse_x)
        self._lib = _capi.load_library()
        self.n, self.d, self.k = int(n), int(d), int(k)
        self.device = int(device)
        # weighted: False | True (dense W_mat) | 'sparse' (0/1 W_mat given as a CSR pattern, upload_observed_csr)
        self.sparse_x = bool(sparse_x)
        if self.sparse_x and (weighted or schedule != 'gram'):
            raise ValueError("sparse_x=True is the unweighted flavour in the Gram form: no weights, schedule='gram'")
        # pattern-only handles (weighted 'sparse') and X kept as CSR both take their products with X 64 columns at a time
        self.sparse = weighted == 'sparse' or self.sparse_x
        self.weighted = bool(weighted)
        if schedule not in ('gram', 'residual'):
            raise ValueError("schedule must be 'gram' or 'residual'")
        if schedule == 'residual' and self.weighted:
            raise ValueError('the weighted flavour always keeps its (masked) residual; schedule applies to unweighted handles')
        self.schedule = schedule
        self._h = C.c_void_p()
        self.n_resets_used = 0
        self.reset_log = []
        self.fix_reset_seed = False
        self._reset_method = None
        self.group = None
        st = self._lib.rri_create(C.byref(self._h), self.n, self.d, self.k, _NP2RRI[self.dtype],
                                  _capi.RRI_UNWEIGHTED_SPARSE if self.sparse_x else 3 if schedule == 'residual'
                                  else 2 if self.sparse else int(self.weighted), int(device),
                                  C.c_void_p(stream or 0))
        if st != _capi.RRI_OK:
            msg = self._lib.rri_last_error(None)
            self._h = C.c_void_p()
            text = 'rri_create failed (%d): %s' % (st, msg.decode() if msg else '?')
            # a refused option or argument is the caller's to fix (the statuses _check maps); anything else is the HIP
            # runtime or the device
            if st == _capi.RRI_ERR_UNSUPPORTED:
                raise NotImplementedError(text)
            if st == _capi.RRI_ERR_INVALID:
                raise ValueError(text)
            raise _capi.RRIHipUnavailable(text)

    def begin_run(self):
        """a handle kept from an earlier nmf() call starts another one: the per-run counters of the host side"""
        self.n_resets_used = 0
        self.reset_log = []

    # ---- plumbing -----------------------------------------------------------------------
    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._lib.rri_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _err(self):
        m = self._lib.rri_last_error(self._h)
        return m.decode() if m else ''

    def _check(self, st):
        if st >= 0:
            return st
        msg = self._err()
        if st == _capi.RRI_ERR_UNBOUNDED:
            raise ValueError('Minimum objective is unbounded. ' + msg)  # optimization.py:105-107
        if st == _capi.RRI_ERR_W_COL_ZERO:
            raise AssertionError('W[:, t] sums to 0')                    # nmf.py:476
        if st == _capi.RRI_ERR_NOT_IMPLEMENTED:
            raise NotImplementedError(msg)                               # optimization.py:72-73
        if st == _capi.RRI_ERR_INVALID:
            raise ValueError(msg)
        if st == _capi.RRI_ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        if st == _capi.RRI_ERR_COMM:
            raise RuntimeError('collective failed: ' + msg)
        raise RuntimeError('librri_hip: status %d: %s' % (st, msg))

    # ---- row-sharded runs -----------------------------------------------------------------
    def attach_group(self, group):
        """this handle holds rows [group.row_lo, group.row_lo + n) of the group's n_global-row problem: from here on
        sweep(), update_*(), objective() and the reset events are collective calls (distributed.RowGroup)"""
        if group is None:
            self._check(self._lib.rri_attach_comm(self._h, None, 0, 0))
            self.group = None
            return
        if group.closed:
            # NULL would DETACH (rri_attach_comm): a later objective() would silently be this rank's share only
            raise ValueError('the RowGroup has been closed: a group must outlive every handle and obj_calculator that uses it')
        if group.n_local != self.n:
            raise ValueError('the group registered %d rows for this rank, the handle has %d' % (group.n_local, self.n))
        self._check(self._lib.rri_attach_comm(self._h, group._comm, group.row_lo, group.n_global))
        self.group = group

    def comm_broadcast(self, values, root=0):
        """`values` (float64 array) of rank `root` on every rank; identity without a group"""
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._check(self._lib.rri_comm_broadcast(self._h, v.ctypes.data_as(C.POINTER(C.c_double)), v.size, int(root)))
        return v

    def comm_sum(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._check(self._lib.rri_comm_allreduce_sum(self._h, v.ctypes.data_as(C.POINTER(C.c_double)), v.size))
        return v

    def comm_stats(self):
        r, w, n = C.c_int32(0), C.c_int32(1), C.c_int64(0)
        self._check(self._lib.rri_comm_stats(self._h, C.byref(r), C.byref(w), C.byref(n)))
        return int(r.value), int(w.value), int(n.value)

    # ---- data ---------------------------------------------------------------------------
    def upload_X(self, X):
        """a float16 handle takes float16 / float32 / float64 arrays as they are and rounds once, from that type; a value
        outside the float16 range raises ValueError and leaves the handle without an X.  A uint8 handle takes uint8 / float32 /
        float64 arrays; a value that is not an integer in 0..255 raises ValueError and leaves the handle without an X, and both
        scale vectors are ones again afterwards"""
        X = _as_host(X, 'X', half=self.dtype == np.float16, keep=np.uint8 if self.dtype == np.uint8 else None)
        if X.shape != (self.n, self.d):
            raise ValueError('X has wrong dimensions')
        self._check(self._lib.rri_upload_X(self._h, X.ctypes.data, X.strides[0] // X.itemsize, _NP2RRI[X.dtype]))

    @property
    def storage_relerr(self):
        """||X - stored(X)||_F / ||X||_F of the last upload_X on a float16 handle (rri_storage_error); 0.0 on float32 / float64
        and uint8 handles (what a uint8 handle accepts it stores exactly), for bound arrays and for an all-zero X"""
        out = (C.c_double * 2)()
        self._check(self._lib.rri_storage_error(self._h, out))
        return float(np.sqrt(out[0] / out[1])) if out[1] > 0.0 else 0.0

    def upload_mask(self, M):
        M = _as_host(M, 'W_mat')
        if M.shape != (self.n, self.d):
            raise ValueError('W_mat has wrong dimensions')
        self._check(self._lib.rri_upload_mask(self._h, M.ctypes.data, M.strides[0] // M.itemsize, _NP2RRI[M.dtype]))

    def _csr_args(self, A):
        import scipy.sparse as sp
        A = sp.csr_matrix(A)
        if A.shape != (self.n, self.d):
            raise ValueError('sparse matrix has wrong dimensions')
        if not A.has_canonical_format:      # never reorder the caller's arrays in place
            A = A.copy()
            A.sum_duplicates()
        return self._csr_args_raw(A)

    @staticmethod
    def _csr_args_raw(A):
        data = A.data if A.data.dtype in _HOST_TYPES else A.data.astype(np.float64)
        indptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(A.indices, dtype=np.int32)
        data = np.ascontiguousarray(data)
        keep = (indptr, indices, data)   # alive for the duration of the call
        return keep, (indptr.ctypes.data_as(C.POINTER(C.c_int64)), indices.ctypes.data_as(C.POINTER(C.c_int32)),
                      data.ctypes.data, int(A.nnz), _NP2RRI[data.dtype])

    def upload_X_csr(self, A):
        """X from a scipy sparse matrix, densified on the device (no host .toarray()); kept as CSR on a sparse_x handle"""
        keep, args = self._csr_args(A)
        self._check(self._lib.rri_upload_X_csr(self._h, *args))

    def upload_X_corpus(self, corpus):
        """X of a sparse_x handle from a DeviceCorpus of the handle's shape and device (rri_upload_X_corpus): the canonical
        arrays are copied device to device and the blocked store is built there -- the same bytes as upload_X_csr(
        corpus.to_scipy()) leaves, without the download, the host's sorts and the uploads.  The corpus is not kept: it may be
        closed right after the call."""
        if tuple(corpus.shape) != (self.n, self.d):
            raise ValueError('the corpus is %d x %d, the handle %d x %d' % (corpus.shape[0], corpus.shape[1], self.n, self.d))
        self._check(self._lib.rri_upload_X_corpus(self._h, corpus._ptr()))

    def sparse_store(self, which):
        """Blocked copy `which` (0: rows as segments cut into column blocks, 1: columns as segments cut into row blocks) of a
        handle that keeps X or its observation pattern as CSR (rri_sparse_store_get), for tests and probes: a dict with nblk, bw,
        nseg, gdim, count, nwork, lps, nnz, longest_row, build_us (HIP-event time of a device build's kernels, 0 after a host
        build) and the arrays segptr [nblk, nseg + 1], idx (uint16), perm (int32), val (the storage type) of max(count, 4)
        entries each, work [nwork, 4]."""
        info = (C.c_int64 * _capi.RRI_SPARSE_STORE_INFO_FIELDS)()
        none = C.POINTER(C.c_int64)()
        self._check(self._lib.rri_sparse_store_get(self._h, int(which), info, _capi.RRI_SPARSE_STORE_INFO_FIELDS, none, None, None, None, None))
        names = ('nblk', 'bw', 'nseg', 'gdim', 'count', 'nwork', 'lps', 'nnz', 'longest_row', 'build_us')
        out = dict(zip(names, (int(v) for v in info)))
        cntp = max(out['count'], 4)
        out['segptr'] = np.zeros((out['nblk'], out['nseg'] + 1), dtype=np.int64)
        out['idx'] = np.zeros(cntp, dtype=np.uint16)
        out['perm'] = np.zeros(cntp, dtype=np.int32)
        out['val'] = np.zeros(cntp, dtype=self.dtype)
        out['work'] = np.zeros((max(out['nwork'], 1), 4), dtype=np.int32)
        self._check(self._lib.rri_sparse_store_get(
            self._h, int(which), info, 0, out['segptr'].ctypes.data_as(C.POINTER(C.c_int64)),
            out['idx'].ctypes.data_as(C.POINTER(C.c_uint16)), out['perm'].ctypes.data_as(C.POINTER(C.c_int32)),
            out['val'].ctypes.data, out['work'].ctypes.data_as(C.POINTER(C.c_int32))))
        out['work'] = out['work'][:out['nwork']]
        return out

    def upload_mask_csr_pattern(self, A):
        """W_mat = [A != 0] of a scipy sparse matrix, bit-packed on the device"""
        keep, args = self._csr_args(A)
        self._check(self._lib.rri_upload_mask_csr_pattern(self._h, *args))

    def upload_observed_csr(self, A):
        """sparse-pattern handles: the stored entries of the scipy sparse matrix A are the observed ones
        (W_mat = 1 there, explicit zeros included), A's values are X on them"""
        import scipy.sparse as sp
        A = sp.csr_matrix(A)
        if A.shape != (self.n, self.d):
            raise ValueError('sparse matrix has wrong dimensions')
        if not A.has_canonical_format:      # never reorder the caller's arrays in place
            A = A.copy()
            A.sum_duplicates()
        keep, args = self._csr_args_raw(A)
        self._check(self._lib.rri_upload_observed_csr(self._h, *args))

    def bind_X_device(self, ptr, ld):
        """X already on the device (row stride ld elements); the call synchronises the device once, later writes
        to that memory are the caller's to order against the handle's stream"""
        self._check(self._lib.rri_bind_X_device(self._h, C.c_void_p(ptr), int(ld)))

    def bind_mask_device(self, ptr, ld):
        self._check(self._lib.rri_bind_mask_device(self._h, C.c_void_p(ptr), int(ld)))

    def set_W(self, W):
        W = _as_host(W, 'W')
        if W.shape != (self.n, self.k):
            raise ValueError('W_in has wrong dimensions, must be n*k')   # nmf.py:853-854
        self._check(self._lib.rri_set_W(self._h, W.ctypes.data, W.strides[0] // W.itemsize, _NP2RRI[W.dtype]))

    def set_T(self, T):
        T = _as_host(T, 'T')
        if T.shape != (self.k, self.d):
            raise ValueError('T_in has wrong dimensions, must be k*d')   # nmf.py:858-859
        self._check(self._lib.rri_set_T(self._h, T.ctypes.data, T.strides[0] // T.itemsize, _NP2RRI[T.dtype]))

    def get_W(self, dtype=np.float64):
        out = np.empty((self.n, self.k), dtype=dtype)
        self._check(self._lib.rri_get_W(self._h, out.ctypes.data, self.k, _NP2RRI[out.dtype]))
        return out

    def get_T(self, dtype=np.float64):
        out = np.empty((self.k, self.d), dtype=dtype)
        self._check(self._lib.rri_get_T(self._h, out.ctypes.data, self.d, _NP2RRI[out.dtype]))
        return out

    def set_params(self, fix_W=False, fix_T=False, project_T_each_iter=False, t_row_sum=None,
                   w_row_sum=None, reset_topic_method='max_resid_document', n_resets=23,
                   reg_w_l1=0.0, reg_w_l2=0.0, reg_t_l1=0.0, reg_t_l2=0.0, fix_reset_seed=False):
        if reset_topic_method not in _RESET_CODES:
            raise ValueError('unknown reset_topic_method %r' % (reset_topic_method,))
        p = Params()
        p.fix_W, p.fix_T = int(bool(fix_W)), int(bool(fix_T))
        p.project_T_each_iter = int(bool(project_T_each_iter))
        p.has_t_row_sum = int(t_row_sum is not None)
        p.t_row_sum = float(t_row_sum) if t_row_sum is not None else 0.0
        scalar_w = w_row_sum is not None and np.isscalar(w_row_sum)
        p.has_w_row_sum = int(scalar_w)
        p.w_row_sum = float(w_row_sum) if scalar_w else 0.0
        p.reset_method = _RESET_CODES[reset_topic_method]
        p.resets_left = int(n_resets)
        p.reg_w_l1, p.reg_w_l2 = float(reg_w_l1), float(reg_w_l2)
        p.reg_t_l1, p.reg_t_l2 = float(reg_t_l1), float(reg_t_l2)
        p.eps_div = EPS_DIV
        self._params = p
        self._reset_method = reset_topic_method
        self.fix_reset_seed = bool(fix_reset_seed)
        self._check(self._lib.rri_set_params(self._h, C.byref(p)))

    # ---- the hot path -------------------------------------------------------------------
    def _resolve_event(self):
        ev = Event()
        self._check(self._lib.rri_pending_event(self._h, C.byref(ev)))
        t = ev.topic
        if self._reset_method == 'max_resid_document':       # nmf.py:770-776 / :804-810
            row = C.c_int64(-1)
            self._check(self._lib.rri_apply_reset_max_resid(self._h, t, C.byref(row)))
            self.reset_log.append((ev.kind, t, int(row.value)))
        elif self._reset_method == 'random' and self.group is not None:
            # row-sharded: rank 0 draws T[t,:] and the WHOLE column W[:,t] with numpy's global RNG, as the reference
            # does for the whole matrix, and broadcasts; every rank keeps its rows
            g = self.group
            buf = np.zeros(self.d + g.n_global)
            if g.rank == 0:
                if self.fix_reset_seed:
                    np.random.seed(t + int(np.argmax(self.get_T()[t, :])))
                trow = np.random.rand(1, self.d)
                buf[:self.d] = (trow / trow.sum()).ravel()
                buf[self.d:] = np.random.rand(g.n_global)
            buf = self.comm_broadcast(buf, 0)
            Trow = np.ascontiguousarray(buf[:self.d])
            Wcol = np.ascontiguousarray(buf[self.d + g.row_lo:self.d + g.row_lo + self.n])
            self._check(self._lib.rri_apply_reset_vectors(
                self._h, t, Trow.ctypes.data_as(C.POINTER(C.c_double)),
                Wcol.ctypes.data_as(C.POINTER(C.c_double))))
            self.reset_log.append((ev.kind, t, -1))
        elif self._reset_method == 'random':                 # nmf.py:778-783 / :811-816
            if self.fix_reset_seed:
                Trow_now = self.get_T()[t, :]
                np.random.seed(t + int(np.argmax(Trow_now)))
            Trow = np.random.rand(1, self.d)
            Trow = np.ascontiguousarray((Trow / Trow.sum()).ravel())
            Wcol = np.ascontiguousarray(np.random.rand(self.n))
            self._check(self._lib.rri_apply_reset_vectors(
                self._h, t, Trow.ctypes.data_as(C.POINTER(C.c_double)),
                Wcol.ctypes.data_as(C.POINTER(C.c_double))))
            self.reset_log.append((ev.kind, t, -1))
        else:
            self._check(self._lib.rri_skip_reset(self._h))
        self.n_resets_used += 1

    def _drive(self, st, done):
        while st == _capi.RRI_PAUSED:
            self._resolve_event()
            st = self._lib.rri_resume(self._h, C.byref(done))
        self._check(st)
        return int(done.value)

    def sweep(self, n_sweeps=1):
        """n_sweeps Gauss-Seidel sweeps (nmf.py:415-476) on the device."""
        done = C.c_int32(0)
        return self._drive(self._lib.rri_sweep(self._h, int(n_sweeps), C.byref(done)), done)

    def update_T_row(self, t):
        st = self._lib.rri_update_T_row(self._h, int(t))
        if st == _capi.RRI_PAUSED:
            self._resolve_event()
            st = self._lib.rri_resume(self._h, None)
        self._check(st)

    def update_W_col(self, t):
        st = self._lib.rri_update_W_col(self._h, int(t))
        if st == _capi.RRI_PAUSED:
            self._resolve_event()
            st = self._lib.rri_resume(self._h, None)
        self._check(st)

    # ---- the explicit residual (schedule='residual') ------------------------------------------
    def residual_rebuild(self):
        """R = X - W T for the factors now on the device"""
        self._check(self._lib.rri_residual_rebuild(self._h))

    def get_residual(self, dtype=None):
        out = np.empty((self.n, self.d), dtype=dtype or self.dtype)
        self._check(self._lib.rri_get_residual(self._h, out.ctypes.data, self.d, _NP2RRI[out.dtype]))
        return out

    def residual_update(self, a, b, trow, wcol, a2=None, b2=None):
        """R <- R - a b^T [- a2 b2^T]; returns (R_new @ trow, R_new.T @ wcol) of the updated stored residual"""
        vec = lambda v, m: None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(m))
        a, a2, wcol = vec(a, self.n), vec(a2, self.n), vec(wcol, self.n)
        b, b2, trow = vec(b, self.d), vec(b2, self.d), vec(trow, self.d)
        ptr = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_double))
        y, z = np.empty(self.n), np.empty(self.d)
        self._check(self._lib.rri_residual_update(self._h, ptr(a), ptr(b), ptr(a2), ptr(b2), ptr(trow), ptr(wcol),
                                                  ptr(y), ptr(z)))
        return y, z

    # ---- around the loop ----------------------------------------------------------------
    def project_W_rows(self, s):
        if np.isscalar(s):
            self._check(self._lib.rri_project_W_rows(self._h, float(s), None))
        else:
            v = np.ascontiguousarray(np.asarray(s, dtype=np.float64).ravel())
            if v.size != self.n:
                raise AssertionError('proj_mat_to_simplex: expected s to have size %d but s has size %d'
                                     % (self.n, v.size))
            self._check(self._lib.rri_project_W_rows(self._h, 0.0, v.ctypes.data_as(C.POINTER(C.c_double))))

    def objective(self):
        out = C.c_double(0.0)
        self._check(self._lib.rri_objective(self._h, C.byref(out)))
        return float(out.value)

    def objective_parts(self):
        out = (C.c_double * 3)()
        self._check(self._lib.rri_objective_parts(self._h, out))
        return [float(v) for v in out]

    def t_norms(self):
        """(sum T^2, sum |T|) of the replicated T, for the sharded objective"""
        T = self.get_T()
        return float((T ** 2).sum()), float(np.abs(T).sum())

    def argmax_rows(self):
        out = np.empty(self.n, dtype=np.int32)
        self._check(self._lib.rri_argmax_rows(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def masked_rmse(self, I, J, vals, lo, hi):
        """clipped RMSE of W T on the listed entries; row-sharded: local rows, collective, the global score on every rank"""
        ij = np.ascontiguousarray(np.stack([np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)], 1).reshape(-1, 2))
        v = np.ascontiguousarray(np.asarray(vals, dtype=np.float64))
        out = C.c_double(0.0)
        self._check(self._lib.rri_masked_rmse(self._h, ij.ctypes.data_as(C.POINTER(C.c_int64)),
                                              v.ctypes.data_as(C.POINTER(C.c_double)), v.size,
                                              float(lo), float(hi), C.byref(out)))
        return float(out.value)

    def topn_rows(self, rows=None, n_top=10, exclude=None, clip=(None, None)):
        """The n_top best columns of W T for the listed rows (None: all n), scored and selected on the device: (idx int32
        (m, n_top), val float64 (m, n_top)).  Ranked by the unclipped score, larger first, equal scores by the smaller column;
        columns of `exclude` -- a scipy sparse matrix with one row per REQUESTED row, of which only the pattern counts -- and
        columns whose score is NaN are left out; a row with fewer than n_top columns left is padded with index -1 and value NaN.
        The returned values are clipped to clip = (lo, hi), None leaving a side open.  Reads the handle's current factors and
        changes nothing; row-sharded: local rows, no collective."""
        if rows is None:
            m, rows_p = self.n, None
        else:
            rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
            m, rows_p = rows.size, rows.ctypes.data_as(C.POINTER(C.c_int64))
        n_top = int(n_top)
        ptr_p = ind_p = None
        if exclude is not None:
            import scipy.sparse as sp
            E = sp.csr_matrix(exclude, copy=True)       # sorted and deduplicated on a copy: the caller's arrays stay as they are
            if E.shape != (m, self.d):
                raise ValueError('exclude must have one row per requested row and d columns: %r, not %r' % ((m, self.d), E.shape))
            E.sum_duplicates()
            E.sort_indices()
            indptr = np.ascontiguousarray(E.indptr, dtype=np.int64)
            indices = np.ascontiguousarray(E.indices, dtype=np.int32)
            ptr_p, ind_p = indptr.ctypes.data_as(C.POINTER(C.c_int64)), indices.ctypes.data_as(C.POINTER(C.c_int32))
        lo, hi = (float('nan') if b is None else float(b) for b in clip)
        idx = np.empty((m, max(n_top, 0)), dtype=np.int32)
        val = np.empty((m, max(n_top, 0)), dtype=np.float64)
        self._check(self._lib.rri_topn_rows(self._h, rows_p, m, n_top, ptr_p, ind_p, lo, hi,
                                            idx.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_double))))
        return idx, val

    def rank_entries(self, rows, targets, exclude=None, clip=(None, None)):
        """The rank of listed columns in the order of topn_rows, counted on the device (rri_rank_entries).  `targets` and
        `exclude` are scipy sparse matrices with one row per REQUESTED row (rows None: all n), of which only the pattern counts;
        both are sorted and deduplicated on copies.  Returns a RankResult: indptr, indices (the canonical CSR of the targets),
        rank int32 aligned with indices -- the number of eligible columns that stand before the target, its 0-based place in an
        unbounded top-N list, or -1 when the target is excluded or its score is NaN --, val float64 (the clipped score, NaN for
        such a target) and eligible int32, one per request.  Without any target nothing is launched and eligible holds -1.
        Reads the handle's current factors and changes nothing; row-sharded: local rows, no collective."""
        import scipy.sparse as sp
        if rows is None:
            m, rows_p = self.n, None
        else:
            rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
            m, rows_p = rows.size, rows.ctypes.data_as(C.POINTER(C.c_int64))

        def pattern(A, what):
            A = sp.csr_matrix(A, copy=True)             # sorted and deduplicated on a copy: the caller's arrays stay as they are
            if A.shape != (m, self.d):
                raise ValueError('%s must have one row per requested row and d columns: %r, not %r' % (what, (m, self.d), A.shape))
            A.sum_duplicates()
            A.sort_indices()
            return np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32)
        I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        tptr, tind = pattern(targets, 'targets')
        eptr_p = eind_p = None
        if exclude is not None:
            eptr, eind = pattern(exclude, 'exclude')
            eptr_p, eind_p = eptr.ctypes.data_as(I64P), eind.ctypes.data_as(I32P)
        lo, hi = (float('nan') if b is None else float(b) for b in clip)
        rank = np.empty(tind.size, dtype=np.int32)
        val = np.empty(tind.size, dtype=np.float64)
        eligible = np.full(m, -1, dtype=np.int32)
        self._check(self._lib.rri_rank_entries(self._h, rows_p, m, tptr.ctypes.data_as(I64P), tind.ctypes.data_as(I32P), eptr_p, eind_p,
                                               lo, hi, rank.ctypes.data_as(I32P), val.ctypes.data_as(C.POINTER(C.c_double)),
                                               eligible.ctypes.data_as(I32P)))
        return RankResult(tptr, tind, rank, val, eligible)

    def _same_device(self, corpus):
        if corpus.device != self.device:
            raise ValueError('the corpus lives on device %d, the handle on device %d' % (corpus.device, self.device))

    def cooccurrence_counts(self, A, words):
        """Document and co-document frequencies of groups of words, counted on the device (rri_cooccurrence_counts).  A is a scipy
        sparse matrix, documents x dictionary, of which only the pattern counts: a stored non-zero means that the word occurs in
        the document (explicit zeros are dropped, duplicates summed and the rows sorted on a copy; the caller's matrix stays as it
        is).  `words` is array-like (g, M) of columns of A, -1 for an empty slot, a column at most once per group, M <= 32.
        Returns (df int64 (g, M), codf int64 (g, M, M)): the number of documents that contain words[g, a], and the number that
        contain both words[g, a] and words[g, b].  A need not have the handle's shape; the handle's factors and X are neither read
        nor changed, and on a row-sharded handle the call is not collective (counts of row blocks add).  A may also be a DeviceCorpus
        on the handle's device (ValueError on another): the same counts from the resident arrays (rri_corpus_cooccurrence_counts)."""
        import scipy.sparse as sp
        words = np.ascontiguousarray(np.asarray(words, dtype=np.int32))
        if words.ndim != 2:
            raise ValueError('words must be a (groups, words per group) array, not %r' % (words.shape,))
        g, M = words.shape
        I64P, I32P = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        if isinstance(A, DeviceCorpus):             # resident and canonical already: nothing of the corpus's size is copied
            self._same_device(A)
            df = np.zeros((g, M), dtype=np.int64)
            codf = np.zeros((g, M, M), dtype=np.int64)
            self._check(self._lib.rri_corpus_cooccurrence_counts(self._h, A._ptr(), words.ctypes.data_as(I32P), g, M,
                                                                 df.ctypes.data_as(I64P), codf.ctypes.data_as(I64P)))
            return df, codf
        A = sp.csr_matrix(A, copy=True)
        A.sum_duplicates()
        A.eliminate_zeros()
        A.sort_indices()
        indptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(A.indices, dtype=np.int32)
        df = np.zeros((g, M), dtype=np.int64)
        codf = np.zeros((g, M, M), dtype=np.int64)
        self._check(self._lib.rri_cooccurrence_counts(self._h, indptr.ctypes.data_as(I64P), indices.ctypes.data_as(I32P), A.shape[0],
                                                      A.shape[1], words.ctypes.data_as(I32P), g, M, df.ctypes.data_as(I64P),
                                                      codf.ctypes.data_as(I64P)))
        return df, codf

    def entries_loglik(self, rows, A, floor=0.0):
        """The log-likelihood of stored counts under the rows of W T, summed per request on the device (rri_entries_loglik).  A is
        a scipy sparse matrix with one row per REQUESTED row of W (rows None: all n) and d columns; its stored values are the
        counts, finite and >= 0.  Returns (ll float64 (m,), mass float64 (m,), floored int64 (m,)): for request q with row i and
        the stored entries (j, v) of row q of A, ll = sum v log(max(p, floor)) with p = (W T)[i, j], an entry with v == 0 adding
        exactly 0; mass = sum v; floored the number of entries with v > 0 and p < floor.  Explicit zeros are kept.  A is sorted and
        its duplicates summed on a copy when it is not canonical, and copied only where its arrays do not have the dtypes the
        library reads; the caller's matrix stays as it is.  Reads the handle's current factors and changes nothing; a request
        returns the same bits alone and among others; row-sharded: local rows, no collective.  A may also be a DeviceCorpus on the
        handle's device (ValueError on another) with one row per request: the same bits as for A.to_scipy(), from the resident
        arrays (rri_corpus_entries_loglik); its explicit zeros are gone, and one with negative values is refused."""
        import scipy.sparse as sp
        if rows is None:
            m, rows_p = self.n, None
        else:
            rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
            m, rows_p = rows.size, rows.ctypes.data_as(C.POINTER(C.c_int64))
        I64P, I32P, DP = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
        if isinstance(A, DeviceCorpus):             # the whole corpus, request q its row q; the kernels read the resident arrays
            self._same_device(A)
            if A.shape != (m, self.d):
                raise ValueError('A must have one row per requested row and d columns: %r, not %r' % ((m, self.d), A.shape))
            ll, mass, floored = np.zeros(m, dtype=np.float64), np.zeros(m, dtype=np.float64), np.zeros(m, dtype=np.int64)
            self._check(self._lib.rri_corpus_entries_loglik(self._h, A._ptr(), rows_p, float(floor), ll.ctypes.data_as(DP),
                                                            mass.ctypes.data_as(DP), floored.ctypes.data_as(I64P)))
            return ll, mass, floored
        if not sp.isspmatrix_csr(A):
            A = sp.csr_matrix(A)
        if A.shape != (m, self.d):
            raise ValueError('A must have one row per requested row and d columns: %r, not %r' % ((m, self.d), A.shape))
        if not A.has_canonical_format:
            A = A.copy()
            A.sum_duplicates()                          # sorts the rows as well; explicit zeros stay
        indptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(A.indices, dtype=np.int32)
        values = np.ascontiguousarray(A.data, dtype=np.float64)
        ll = np.zeros(m, dtype=np.float64)
        mass = np.zeros(m, dtype=np.float64)
        floored = np.zeros(m, dtype=np.int64)
        self._check(self._lib.rri_entries_loglik(self._h, rows_p, m, indptr.ctypes.data_as(I64P), indices.ctypes.data_as(I32P),
                                                 values.ctypes.data_as(DP), float(floor), ll.ctypes.data_as(DP),
                                                 mass.ctypes.data_as(DP), floored.ctypes.data_as(I64P)))
        return ll, mass, floored

    # ---- rows that left the device: frozen statistics (online fits) ---------------------------------
    def set_frozen(self, frozen):
        """From here on every T-row step and column check of this handle is that of the stacked problem [X_O; X] whose rows O
        are kept as `frozen` (a FrozenRows: B = W_O^T X_O, A = W_O^T W_O, s = 1^T W_O, c = ||X_O||^2) and never updated
        (rri_frozen_set).  None clears them.  NotImplementedError on the handles that do not take them (weighted, residual
        schedule, float16 / uint8, uniform rows, a group attached); ValueError for values that are negative, not finite or, for
        A, not symmetric."""
        if frozen is None:
            return self.clear_frozen()
        if frozen.k != self.k or frozen.d != self.d:
            raise ValueError('frozen statistics are for k = %d, d = %d; the handle has k = %d, d = %d' % (frozen.k, frozen.d, self.k, self.d))
        DP = C.POINTER(C.c_double)
        B, A, s = (np.ascontiguousarray(a, dtype=np.float64) for a in (frozen.B, frozen.A, frozen.s))
        self._check(self._lib.rri_frozen_set(self._h, B.ctypes.data_as(DP), A.ctypes.data_as(DP), s.ctypes.data_as(DP), float(frozen.c)))
        self._frozen_rows0 = int(frozen.rows)

    def clear_frozen(self):
        """drops the statistics and frees their device memory (rri_frozen_set with B = NULL); harmless when none are set"""
        self._check(self._lib.rri_frozen_set(self._h, None, None, None, 0.0))
        self._frozen_rows0 = 0

    def get_frozen(self):
        """the statistics as the handle holds them (rri_frozen_get): a FrozenRows whose `rows` is the count of the FrozenRows
        last set plus the rows absorbed since"""
        B, A, s = np.empty((self.k, self.d)), np.empty((self.k, self.k)), np.empty(self.k)
        c, rows = C.c_double(0.0), C.c_int64(0)
        DP = C.POINTER(C.c_double)
        self._check(self._lib.rri_frozen_get(self._h, B.ctypes.data_as(DP), A.ctypes.data_as(DP), s.ctypes.data_as(DP), C.byref(c), C.byref(rows)))
        return FrozenRows(B, A, s, float(c.value), getattr(self, '_frozen_rows0', 0) + int(rows.value))

    def absorb(self, decay=1.0):
        """F <- decay F + (W^T X, W^T W, 1^T W, ||X||^2) of the handle's own rows and current W (rri_frozen_absorb): the rows
        this handle holds join the frozen ones, from zeros when nothing is set; decay in (0, 1].  W, T and a sweep that follows
        are unchanged by it, and the same call on the same state leaves the same bits."""
        self._check(self._lib.rri_frozen_absorb(self._h, float(decay)))

    def snapshot(self):
        self._check(self._lib.rri_snapshot(self._h))

    def rollback(self):
        self._check(self._lib.rri_rollback(self._h))

    # ---- products with the resident X (initialisation) ----------------------------------------
    def X_times(self, B):
        """X @ B for a host (d, m) matrix, float64"""
        B = np.ascontiguousarray(B, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != self.d:
            raise ValueError('operand must be (d, m)')
        if self.sparse and B.shape[1] > 64:     # pattern-only handles take up to 64 columns per call
            return np.hstack([self.X_times(B[:, lo:lo + 64]) for lo in range(0, B.shape[1], 64)])
        out = np.empty((self.n, B.shape[1]))
        self._check(self._lib.rri_X_times(self._h, B.ctypes.data_as(C.POINTER(C.c_double)), B.shape[1],
                                          out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def Xt_times(self, Q):
        """X.T @ Q for a host (n, m) matrix, float64"""
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        if Q.ndim != 2 or Q.shape[0] != self.n:
            raise ValueError('operand must be (n, m)')
        if self.sparse and Q.shape[1] > 64:
            return np.hstack([self.Xt_times(Q[:, lo:lo + 64]) for lo in range(0, Q.shape[1], 64)])
        out = np.empty((self.d, Q.shape[1]))
        self._check(self._lib.rri_Xt_times(self._h, Q.ctypes.data_as(C.POINTER(C.c_double)), Q.shape[1],
                                           out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def range_finder(self, Q0, n_iter, transpose=False):
        """(Q, B) of the randomized range finder on the resident X, panels on the device (rri_range_finder): A = X, or X.T when
        `transpose`; Q0 is the (columns of A, m) test matrix, Q the orthonormal (rows of A, m) basis of range(A (A^T A)^n_iter Q0),
        B = Q^T A.  m <= 64, dense handles."""
        Q0 = np.ascontiguousarray(Q0, dtype=np.float64)
        rows, cols = (self.d, self.n) if transpose else (self.n, self.d)
        if Q0.ndim != 2 or Q0.shape[0] != cols:
            raise ValueError('test matrix must be (%d, m)' % cols)
        m = Q0.shape[1]
        Q, B = np.empty((rows, m)), np.empty((m, cols))
        self._check(self._lib.rri_range_finder(self._h, Q0.ctypes.data_as(C.POINTER(C.c_double)), m, int(n_iter), int(bool(transpose)),
                                               Q.ctypes.data_as(C.POINTER(C.c_double)), B.ctypes.data_as(C.POINTER(C.c_double))))
        return Q, B

    def sparse_range_finder(self, Q0, n_iter, transpose=False):
        """range_finder on a handle that keeps X sparse (rri_sparse_range_finder): the CSR X of sparse_x=True, the observed values
        of weighted='sparse'.  Same arguments, same shapes, same Cholesky-QR; the panels stay on the device as tall row-major
        matrices, the layout of the sparse products.  m <= 64; ValueError on a dense handle and before an upload."""
        Q0 = np.ascontiguousarray(Q0, dtype=np.float64)
        rows, cols = (self.d, self.n) if transpose else (self.n, self.d)
        if Q0.ndim != 2 or Q0.shape[0] != cols:
            raise ValueError('test matrix must be (%d, m)' % cols)
        m = Q0.shape[1]
        Q, B = np.empty((rows, m)), np.empty((m, cols))
        self._check(self._lib.rri_sparse_range_finder(self._h, Q0.ctypes.data_as(C.POINTER(C.c_double)), m, int(n_iter),
                                                      int(bool(transpose)), Q.ctypes.data_as(C.POINTER(C.c_double)),
                                                      B.ctypes.data_as(C.POINTER(C.c_double))))
        return Q, B

    # ---- preprocessing of the resident X (matrixops.py:124-179) ---------------------------
    def column_positive_counts(self):
        """df[j] = #{i: X[i, j] > 0}"""
        out = np.empty(self.d, dtype=np.float64)
        self._check(self._lib.rri_column_positive_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def scale_X(self, col_scale=None, normalize_rows=False):
        """X <- X * col_scale (per column), then rows divided by their sums when normalize_rows (in place)"""
        ptr = None
        if col_scale is not None:
            col_scale = np.ascontiguousarray(col_scale, dtype=np.float64).ravel()
            if col_scale.size != self.d:
                raise ValueError('col_scale must have d entries')
            ptr = col_scale.ctypes.data_as(C.POINTER(C.c_double))
        st = self._lib.rri_scale_X(self._h, ptr, int(bool(normalize_rows)))
        if st == _capi.RRI_ERR_INVALID and self.dtype == np.uint8:
            # counts cannot hold the dense row 1/d that normalize makes of an empty row: nothing was changed, the message starts
            # with how many there are (include/rri_hip.h)
            m = re.match(r'(\d+) row', self._err())
            if m:
                raise ZeroTotalRows(int(m.group(1)))
        self._check(st)

    def set_X_scales(self, row_scale=None, col_scale=None):
        """uint8 handles: the X that is factorised is (C * col_scale) * row_scale[:, None]; None leaves a vector as it is"""
        ptrs = []
        keep = []
        for v, size, what in ((row_scale, self.n, 'row_scale must have n entries'), (col_scale, self.d, 'col_scale must have d entries')):
            if v is None:
                ptrs.append(None)
                continue
            v = np.ascontiguousarray(v, dtype=np.float64).ravel()
            if v.size != size:
                raise ValueError(what)
            keep.append(v)
            ptrs.append(v.ctypes.data_as(C.POINTER(C.c_double)))
        self._check(self._lib.rri_set_X_scales(self._h, ptrs[0], ptrs[1]))

    def X_scales(self):
        """(row_scale, col_scale) of a uint8 handle, float64"""
        r, s = np.empty(self.n, dtype=np.float64), np.empty(self.d, dtype=np.float64)
        self._check(self._lib.rri_get_X_scales(self._h, r.ctypes.data_as(C.POINTER(C.c_double)),
                                               s.ctypes.data_as(C.POINTER(C.c_double))))
        return r, s

    def preprocess(self, tfidf=False, normalize=False, uniform_rows=False):
        """tf-idf and/or row normalisation of the resident X, as matrixops.tfidf / normalize produce them.
        tfidf: True (idf from this X), an idf vector (transform of new documents), or False.  Returns the idf used.
        uniform_rows=True (a handle that keeps X as CSR only): rows whose total is below 1e-10 become the handle's uniform rows,
        the dense row 1/d kept beside the pattern (uniform_rows()), and ZeroTotalRows is never raised."""
        if self.sparse_x:
            return self._preprocess_csr(tfidf, normalize, uniform_rows)
        if uniform_rows:
            raise ValueError('uniform_rows=True needs a handle that keeps X as CSR (sparse_x=True)')
        idf = None
        if tfidf is True:
            df = self.column_positive_counts()
            n_docs = self.n
            grp = getattr(self, 'group', None)
            if grp is not None:        # row-sharded: document frequencies are sums over the ranks, the corpus is all rows
                df = self.comm_sum(df)
                n_docs = grp.n_global
            idf = np.log(n_docs / (df + np.spacing(1)))       # matrixops.py:169-170
        elif tfidf is not False and tfidf is not None:
            idf = np.asarray(tfidf, dtype=np.float64).ravel()
        if idf is not None or normalize:
            self.scale_X(idf, normalize)
        return idf

    def _preprocess_csr(self, tfidf, normalize, uniform_rows=False):
        """preprocess() on a handle that keeps X as CSR (rri_csr_column_positive_counts, rri_csr_scale_X): the stored values are
        rewritten.  Row normalisation turns a row whose total is below 1e-10 into the dense row 1/d (matrixops.py:143-147),
        which the pattern cannot hold: ZeroTotalRows is raised then and X is what it was before the call -- or, with
        uniform_rows, those rows take zeros and the handle keeps them as uniform rows (rri_csr_scale_X_uniform)."""
        as_ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
        idf = None
        if tfidf is True:
            df = np.empty(self.d, dtype=np.float64)
            self._check(self._lib.rri_csr_column_positive_counts(self._h, as_ptr(df)))
            idf = np.log(self.n / (df + np.spacing(1)))       # matrixops.py:169-170
        elif tfidf is not False and tfidf is not None:
            idf = np.ascontiguousarray(tfidf, dtype=np.float64).ravel()
            if idf.size != self.d:
                raise ValueError('col_scale must have d entries')
        if idf is not None or normalize:
            zero_rows = C.c_int64(0)
            scale = self._lib.rri_csr_scale_X_uniform if uniform_rows else self._lib.rri_csr_scale_X
            self._check(scale(self._h, None if idf is None else as_ptr(idf), int(bool(normalize)), C.byref(zero_rows)))
            if zero_rows.value and not uniform_rows:
                raise ZeroTotalRows(int(zero_rows.value))
        return idf

    def set_uniform_rows(self, rows, value):
        """Declares rows of the resident CSR X as the dense row `value` (every column j < d): X = S + value * e_U 1^T, where S is
        the stored CSR with zeros in those rows.  An empty list clears them; a second call replaces the list."""
        rows = np.asarray(rows).ravel()
        if rows.size and rows.dtype.kind not in 'iu':
            raise ValueError('uniform rows are row indices: integers, not %s' % rows.dtype)
        # what int32 cannot hold is refused here, not wrapped into a row the handle would accept
        beyond = rows[(rows < np.iinfo(np.int32).min) | (rows > np.iinfo(np.int32).max)] if rows.size else rows
        if beyond.size:
            raise ValueError('uniform row %d is out of range (n = %d)' % (int(beyond[0]), self.n))
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        ptr =rows.ctypes.data_as(C.POINTER(C.c_int32)) if rows.size else None
        self._check(self._lib.rri_set_uniform_rows(self._h, ptr, int(rows.size), float(value)))

    def uniform_rows(self):
        """(rows, value): the sorted int32 list of the handle's uniform rows and their value (empty, 0.0 by default)"""
        count, value = C.c_int64(0), C.c_double(0.0)
        self._check(self._lib.rri_get_uniform_rows(self._h, None, 0, C.byref(count), C.byref(value)))
        rows = np.empty(int(count.value), dtype=np.int32)
        if rows.size:
            self._check(self._lib.rri_get_uniform_rows(self._h, rows.ctypes.data_as(C.POINTER(C.c_int32)), int(rows.size),
                                                       C.byref(count), C.byref(value)))
        return rows, float(value.value)

    # ---- row-sharded stepping -----------------------------------------------------------
    def reduce_buffer(self):
        ptr, cnt = C.c_void_p(), C.c_int64()
        self._check(self._lib.rri_reduce_buffer(self._h, C.byref(ptr), C.byref(cnt)))
        return ptr.value, int(cnt.value)

    def bind_reduce_buffer(self, ptr, n_elems):
        self._check(self._lib.rri_bind_reduce_buffer(self._h, C.c_void_p(ptr), int(n_elems)))

    def topic_reduce_local(self, t):
        self._check(self._lib.rri_topic_reduce_local(self._h, int(t)))

    def topic_finish(self, t):
        self._check(self._lib.rri_topic_finish(self._h, int(t)))

    def reduce_read(self, count):
        out = np.empty(int(count), dtype=np.float64)
        self._check(self._lib.rri_reduce_read(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), int(count)))
        return out

    def reduce_write(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self._check(self._lib.rri_reduce_write(self._h, v.ctypes.data_as(C.POINTER(C.c_double)), int(v.size)))

    def _stepping_event(self):
        """polls; a reset event is resolved as rri_sweep's are.  Returns its (kind, topic) or None."""
        if self.poll() != _capi.RRI_PAUSED:
            return None
        kind, topic, _ = self.pending_event()
        self._resolve_event()
        return kind, topic

    def sweep_with_T_noise(self, draw):
        """One sweep in which every T-row step sees wR + noise and max(nw + noise, 0): the Gaussian mechanism of
        nmf.py:422-435.  `draw(m)` returns m samples; it is called in the reference's order (wR first, then nw,
        after any reset of the previous column has drawn its own numbers)."""
        self.sweep_stepwise(draw=draw)

    def sweep_stepwise(self, draw=None, observe=None):
        """One sweep with the host between the two device stages of every T-row step: the sums of a topic step are
        taken on the device (rri_topic_reduce_local), read -- and, with `draw`, perturbed -- in the reduce buffer on the
        host, and the step finishes on the device (rri_topic_finish): the split stepping of the row-sharded path with
        the host in the place of the all-reduce.
          observe(t, wR, nw)  sees the sums of _compute_update_T (nmf.py:670-676, 687-701) before any noise:
                              store_gradients (nmf.py:454-456)
          draw(m)             the Gaussian mechanism (see sweep_with_T_noise)"""
        d, k = self.d, self.k
        ld = self._row_stride()
        for t in range(k):
            self.topic_reduce_local(t)
            self.topic_finish(-1)                       # the column check of topic t-1 (nmf.py:471-476)
            if self._stepping_event() is not None:      # dead column: reset, then the sums again
                self.topic_reduce_local(t)
            r, wR, nw, trow = self._topic_sums(t, ld, with_wR=observe is not None or self.weighted)
            if observe is not None:
                observe(t, np.array(wR), np.array(nw) if self.weighted else nw)
            if draw is not None and self.weighted:
                wR = wR + draw(d)
                nw2 = np.maximum(nw + draw(d), 0)
                r[:d] = wR - trow * nw2
                r[ld:ld + d] = nw2
            elif draw is not None:
                at = [ld + g * (k + 2) + k for g in range(_capi.RRI_GRAM_SLICES)]
                r[:d] += draw(d)                        # wR = w^T X - (w^T W) T: the noise passes through
                nw = nw + float(np.asarray(draw(1)).ravel()[0])
                for i in at:
                    r[i] = 0.0
                r[at[0]] = max(nw, 0.0)
            if draw is not None:
                self.reduce_write(r)
            self.topic_finish(t)
            if self._stepping_event() is not None:      # the new T row was (numerically) zero: reset, then its W half
                self.topic_finish_w(t)
        self.topic_reduce_local(0)                      # the last column's check rides on topic 0's sums
        self.topic_finish(-1)
        self._stepping_event()

    def _row_stride(self):
        """LD of the handle (rri_create): d rounded up to the elements of one load -- 16 bytes, but 8 for uint8 counts"""
        vn = 8 if self.dtype == np.uint8 else 16 // self.dtype.itemsize
        return -(-self.d // vn) * vn

    def _topic_sums(self, t, ld, with_wR=True):
        """(reduce buffer, wR, nw, T[t,:] or None) after rri_topic_reduce_local(t): the sums _compute_update_T returns
        (nmf.py:670-676 plain, :687-701 weighted)"""
        d, k = self.d, self.k
        if self.weighted:                               # red = [a | nw]; wR = a + t .* nw (rri_wrri_kernels.hpp)
            r = self.reduce_read(2 * ld)
            trow = self.get_T()[t, :]
            nw = r[ld:ld + d]
            return r, r[:d] + trow * nw, nw, trow
        r = self.reduce_read(ld + _capi.RRI_GRAM_SLICES * (k + 2))   # red = [w^T X | slices of (w^T W, ||w||^2, .)]
        nw = float(sum(r[ld + g * (k + 2) + k] for g in range(_capi.RRI_GRAM_SLICES)))
        wR = None
        if with_wR:
            wW = sum(r[ld + g * (k + 2):ld + g * (k + 2) + k] for g in range(_capi.RRI_GRAM_SLICES))
            wW[t] = 0.0                                 # nmf.py:672
            wR = r[:d] - wW.dot(self.get_T())
        return r, wR, nw, None

    def topic_sums(self, t):
        """(wR, nw) of topic t for the factors now on the device: w_t^T (X - sum_{j != t} w_j t_j) and ||w_t||^2, or
        their weighted counterparts (d-vectors)"""
        ld = self._row_stride()
        self.topic_reduce_local(t)
        _, wR, nw, _ = self._topic_sums(t, ld)
        return np.array(wR), (np.array(nw) if self.weighted else nw)

    def topic_finish_w(self, t):
        self._check(self._lib.rri_topic_finish_w(self._h, int(t)))

    def poll(self):
        """synchronises and returns RRI_OK or RRI_PAUSED (errors raise)"""
        return self._check(self._lib.rri_poll(self._h))

    def pending_event(self):
        ev = Event()
        self._check(self._lib.rri_pending_event(self._h, C.byref(ev)))
        return ev.kind, ev.topic, ev.resume_topic

    def resid_row_argmax(self):
        val, row = C.c_double(0.0), C.c_int64(-1)
        self._check(self._lib.rri_resid_row_argmax(self._h, C.byref(val), C.byref(row)))
        return float(val.value), int(row.value)

    def reset_row(self, local_row):
        out = np.empty(self.d, dtype=np.float64)
        self._check(self._lib.rri_reset_row(self._h, int(local_row), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def apply_reset_vectors(self, t, T_row, W_col):
        T_row = np.ascontiguousarray(T_row, dtype=np.float64)
        W_col = np.ascontiguousarray(W_col, dtype=np.float64)
        self._check(self._lib.rri_apply_reset_vectors(
            self._h, int(t), T_row.ctypes.data_as(C.POINTER(C.c_double)),
            W_col.ctypes.data_as(C.POINTER(C.c_double))))
        self.n_resets_used += 1

    # ---- measurement --------------------------------------------------------------------
    def timing_enable(self, on=True, every=1):
        """HIP-event timing of the streaming kernels; every=N samples each N-th launch"""
        self._check(self._lib.rri_timing_enable(self._h, int(every) if on else 0))

    def timing_read(self, kernel_id):
        cnt, ms = C.c_int64(0), C.c_double(0.0)
        self._check(self._lib.rri_timing_read(self._h, int(kernel_id), C.byref(cnt), C.byref(ms)))
        return int(cnt.value), float(ms.value)

    def onchip_info(self):
        """(would the next sweep() run as the register-resident persistent launch, how many such launches so far)"""
        el, n = C.c_int32(0), C.c_int64(0)
        self._check(self._lib.rri_onchip_info(self._h, C.byref(el), C.byref(n)))
        return bool(el.value), int(n.value)

    # rri_layout_info: four values per copy of a blocked store (row copy, then column copy), then one value per name
    LAYOUT_COPY_FIELDS = ('nblk', 'bw', 'lps', 'nwork')
    LAYOUT_FIELDS = ('rpb', 'nrb', 'npanels', 'mask_bits', 'mask_cols', 'mask_density', 'wtrow_small', 'nw_from_mask',
                     'interleaved', 'wcorr_nrb', 'n_cu', 'x_pack', 'x_pack_base', 'x_pack_flagged', 'x_pack_tiles', 'x_pack_bits',
                     'x_pack_book', 'x_pack_exceptions', 'early_sums', 'early_steps', 'early_deal', 'early_stride')
    assert 2 * len(LAYOUT_COPY_FIELDS) + len(LAYOUT_FIELDS) == _capi.RRI_LAYOUT_FIELDS

    def layout_info(self):
        """what the handle decided (rri_layout_info): per-copy values of a blocked CSR store as (row copy, column copy) pairs --
        nblk, bw, lps, nwork -- the pass geometry rpb / nrb / npanels, and which routes of the dense weighted step are taken
        (mask_density is None until the first topic step has measured it; nw_from_mask is what the last T-row step did), and the
        packed copy of an fp32 X: x_pack (the read-only pass streams it), x_pack_base, x_pack_flagged of x_pack_tiles tiles, x_pack_bits
        per element (28, 26 or 0), x_pack_book (the seven exponent bytes of a 26-bit copy) and x_pack_exceptions (elements outside it);
        early_sums (the handle takes the early-sums schedule with its current parameters) and early_steps (W-column steps that did);
        early_deal (RRI_EARLY_DEAL: the job's workgroups are dealt through the pass's grid) and early_stride (the pass's own workgroups
        between two of the job; 0: one contiguous run)"""
        nc = len(self.LAYOUT_COPY_FIELDS)
        out = (C.c_int64 * _capi.RRI_LAYOUT_FIELDS)()
        self._check(self._lib.rri_layout_info(self._h, out, _capi.RRI_LAYOUT_FIELDS))
        v = [int(x) for x in out]
        info = {name: (v[i], v[nc + i]) for i, name in enumerate(self.LAYOUT_COPY_FIELDS)}
        info.update(zip(self.LAYOUT_FIELDS, v[2 * nc:]))
        for name in ('mask_bits', 'mask_cols', 'wtrow_small', 'nw_from_mask', 'interleaved', 'x_pack', 'early_sums', 'early_deal'):
            info[name] = bool(info[name])
        info['mask_density'] = None if info['mask_density'] < 0 else info['mask_density'] * 1e-9
        info['x_pack_book'] = [info['x_pack_book'] >> (8 * i) & 0xff for i in range(7)] if info['x_pack_bits'] == 26 else []
        return info

    def debug_xcc(self, count=32):
        """diagnostics: the XCD each of `count` workgroups of a launch on this handle's stream lands on"""
        out = (C.c_int32 * count)()
        self._check(self._lib.rri_debug_xcc(self._h, out, count))
        return list(out)

    def onchip_fallbacks(self):
        """how many persistent launches of this handle gave up (workgroups not co-resident) and were rerun launch by launch"""
        n = C.c_int64(0)
        self._check(self._lib.rri_onchip_fallbacks(self._h, C.byref(n)))
        return int(n.value)

    def sweep_until(self, n_sweeps, obj_prev, stop_scale):
        """Up to n_sweeps sweeps of the register-resident kernel with every sweep's objective kept and the stop rule of
        nmf.py:510 applied on the device (rri_sweep_until): the run ends after the first sweep whose objective moved by no more
        than stop_scale (= eps_stop |o_0 - o_1|; negative: never).  Returns (sweeps run, their objectives -- NaN where the
        kernel left none: take objective() there), or None when the handle does not take the persistent path."""
        n_sweeps = int(n_sweeps)
        if not self.onchip_info()[0]:
            return None
        hist = np.full(n_sweeps, np.nan, dtype=np.float64)
        done = C.c_int32(0)
        st = self._lib.rri_sweep_until(self._h, n_sweeps, float(obj_prev), float(stop_scale),
                                       hist.ctypes.data_as(C.POINTER(C.c_double)), C.byref(done))
        if st == _capi.RRI_ERR_UNSUPPORTED:
            return None
        n_done = self._drive(st, done)
        return n_done, hist[:n_done]

    def synchronize(self):
        self._check(self._lib.rri_synchronize(self._h))

    def bench_rank1_update(self, reps=5):
        ms = C.c_double(0.0)
        self._check(self._lib.rri_bench_rank1_update(self._h, int(reps), C.byref(ms)))
        return float(ms.value)

    def bench_stream_copy(self, reps=5):
        ms = C.c_double(0.0)
        self._check(self._lib.rri_bench_stream_copy(self._h, int(reps), C.byref(ms)))
        return float(ms.value)
