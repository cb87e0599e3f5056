"""A corpus from (row, column, value) pairs and the split of a corpus by entry, without a GPU: the constants, the refusals and the
two plain loops of rri_nmf_amd/csrc/rri_corpus_build.hpp under sanitizers, the ABI surface of include/rri_corpus_build.h and the
refusals of the real library that need no device, and the host logic of DeviceCorpus.from_pairs / split_entries and of the
estimator's DeviceCorpus branches with stand-ins for the device.

tests/c/corpus_build_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built once with
the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once; what it prints is compared with what is
written here and with the numpy restatement (tests/corpus_build_cases.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import corpus_build_cases as cb
import derive_cases as dc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('corpus_build') / 'corpus_build')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'corpus_build_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    out = res.stdout.strip().splitlines()
    assert out[-1] == 'ok 16 9 cases', out[-1]
    return out


def records(lines, kinds):
    """{case id: {kind: float64 array}} of the lines `kind id : numbers`"""
    rec = {}
    for ln in lines:
        kind, _, rest = ln.partition(' ')
        if kind in kinds:
            head, _, body = rest.partition(' :')
            rec.setdefault(int(head), {})[kind] = np.array(body.split(), dtype=np.float64)
    return rec


def matrix(r, name):
    n_rows, n_cols = (int(x) for x in r[name + 'shape'])
    return sp.csr_matrix((r[name + 'val'], r[name + 'idx'].astype(np.int32), r[name + 'ptr'].astype(np.int64)), shape=(n_rows, n_cols))


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same(A, B):
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(bits(A.data), bits(B.data)))


def test_the_constants_and_every_refusal_with_its_verdict_and_text(lines):
    assert 'consts : %d %d %d %d %d %d' % (cb.WAVE_PAIRS, cb.BLOCK_PAIRS, cb.GRID_MAX, cb.SWEEP_PAIRS, cb.PAIRS_MAX, cb.RULES) in lines
    assert cb.BLOCK_PAIRS % cb.WAVE_PAIRS == 0 and cb.SWEEP_PAIRS == cb.BLOCK_PAIRS * cb.GRID_MAX and cb.PAIRS_MAX == 2 ** 31 - 1
    assert 'grid : %d %d %d %d %d' % tuple(cb.grid(m) for m in (0, 1, cb.BLOCK_PAIRS + 1, cb.SWEEP_PAIRS, cb.SWEEP_PAIRS + 1)) in lines
    assert cb.grid(cb.SWEEP_PAIRS + 1) == cb.GRID_MAX and cb.grid(cb.BLOCK_PAIRS) == 1
    got = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'req (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    assert set(got) == set(cb.REQUEST_FINE) | set(cb.REQUEST_TEXT)
    for name in cb.REQUEST_FINE:
        assert got[name] == (cb.OK, ''), name
    for name, want in cb.REQUEST_TEXT.items():
        assert got[name] == want, name
    # the three rules of a list that is there, from the restatement too
    R, Cc, V, nan, inf = [0, 2, 1, 2], [5, 0, 3, 0], [1.0, 2.0, -1.5, 0.0], float('nan'), float('inf')
    for name, args in (('row_3_at_1', ([0, 3, 1, 2], Cc, V)), ('row_negative_at_2', ([0, 2, -1, 5], Cc, V)), ('column_6_at_0', (R, [6, 0, 3, -1], V)),
                       ('column_negative_at_3', (R, [5, 0, 3, -1], V)), ('rows_before_columns', ([0, 2, 1, 7], [9, 0, 3, 0], V)),
                       ('value_nan_at_2', (R, Cc, [1.0, 2.0, nan, inf])), ('value_minus_inf_at_3', (R, Cc, [1.0, 2.0, 3.0, -inf])),
                       ('columns_before_values', (R, [5, 0, 3, 8], [nan, 2.0, 3.0, 1.0])), ('rows_before_values', ([0, 2, 1, 3], Cc, [inf, 2.0, 3.0, 1.0]))):
        assert cb.check(*args, shape=(3, 6)) == got[name], name
    assert cb.check(R, Cc, V, (3, 6)) == cb.check(R, Cc, None, (3, 6)) == (cb.OK, '')
    assert cb.check(R, Cc, V, (3, 2 ** 31)) == got['n_cols_2_31']
    # every kind of refusal stands at two places
    kinds = {}
    for name in cb.REQUEST_TEXT:
        kinds.setdefault(re.sub(r'-?\d[\w.]*|-?nan|-?inf', '#', got[name][1]), []).append(name)
    assert all(len(v) >= 2 for v in kinds.values()), kinds
    assert len(kinds) == cb.KINDS


def test_a_corpus_from_pairs_of_the_plain_loop_against_the_restatement(lines):
    rec = records(lines, ('pairs', 'prow', 'pcol', 'pval', 'cptr', 'cidx', 'cval', 'cstat'))
    assert len(rec) == 16
    seen = dict(int32=0, int64=0, stride_2=0, float32=0, pattern=0, no_pairs=0, no_rows=0, untouched=0, zero_stored=0, sum_zero=0, negatives=0,
                one_row=0, empty_row=0)
    for cid, r in sorted(rec.items()):
        n_rows, n_cols, m, stride, idt, vdt = (int(x) for x in r['pairs'])
        rows, cols = r['prow'].astype(np.int64), r['pcol'].astype(np.int64)
        values = None if vdt == -1 else r['pval']
        assert rows.size == cols.size == m and (values is None or values.size == m), cid
        assert cb.check(rows, cols, values, (n_rows, n_cols)) == (cb.OK, ''), cid
        ptr, idx, val, st = cb.from_pairs(rows, cols, values, (n_rows, n_cols))
        assert np.array_equal(r['cptr'].astype(np.int64), ptr) and np.array_equal(r['cidx'].astype(np.int32), idx), cid
        assert np.array_equal(bits(r['cval']), bits(val)), cid
        assert dict(zip(cb.INFO, (int(x) for x in r['cstat']))) == st, cid
        assert m == val.size + st['duplicates_merged'] + st['zeros_dropped'], cid
        # scipy's own reading of the triples agrees wherever the order of the additions cannot matter
        if values is None or np.all(np.abs(values) < 1e6):
            want = sp.coo_matrix((np.ones(m) if values is None else values, (rows, cols)), shape=(n_rows, n_cols)).tocsr()
            want.sum_duplicates()
            want.eliminate_zeros()
            want.sort_indices()
            assert same(sp.csr_matrix((val, idx, ptr), shape=(n_rows, n_cols)), want), cid
        seen['int32'] += idt == _capi.RRI_I32
        seen['int64'] += idt == _capi.RRI_I64
        seen['stride_2'] += stride == 2
        seen['float32'] += vdt == _capi.RRI_F32
        seen['pattern'] += vdt == -1
        seen['no_pairs'] += m == 0 and n_rows > 0
        seen['no_rows'] += n_rows == 0
        seen['untouched'] += m > 0 and st['rows_rewritten'] == 0
        seen['zero_stored'] += values is not None and bool((values == 0).any())
        seen['sum_zero'] += st['zeros_dropped'] > (0 if values is None else int((values == 0).sum()))
        seen['negatives'] += st['negatives'] > 0
        seen['one_row'] += m > 0 and np.unique(rows).size == 1
        seen['empty_row'] += n_rows > 0 and np.unique(rows).size < n_rows
    assert all(seen.values()), seen
    # the representations of one list: the same arrays (cases 0 .. 5; float32 rounds the eighths of these values exactly)
    for cid in range(1, 6):
        assert all(np.array_equal(bits(rec[cid][key]), bits(rec[0][key])) for key in ('cptr', 'cidx', 'cval', 'cstat')), cid
    # rows as given canonical: none rewritten, whether the rows are grouped or interleaved; one stored zero rewrites its row
    assert [int(rec[cid]['cstat'][0]) for cid in (8, 9, 10)] == [0, 0, 1]
    assert np.array_equal(rec[8]['cval'], rec[9]['cval']) and int(rec[10]['cstat'][2]) == 1
    # the order of summation: 1e16, 1, -1e16, 1, ... in the order given is 1; permuted, what its own order gives
    for cid in (11, 12):
        vals = rec[cid]['pval'][(rec[cid]['prow'] == 1) & (rec[cid]['pcol'] == 2)]
        want = 0.0
        for v in vals:
            want += float(v)
        A = sp.csr_matrix((rec[cid]['cval'], rec[cid]['cidx'].astype(np.int32), rec[cid]['cptr'].astype(np.int64)), shape=(3, 5))
        assert vals.size == 8 and bits(A[1, 2]) == bits(want) and A[0, 4] == 0 and int(rec[cid]['cstat'][2]) >= 1, cid
    assert sorted(rec[11]['pval'].tolist()) == sorted(rec[12]['pval'].tolist())


def test_the_split_by_entry_of_the_plain_loop_against_the_restatement_and_its_sanity_bound(lines):
    rec = records(lines, ('split', 'asone') + tuple(n + k for n in ('from', 'obs', 'held') for k in ('shape', 'ptr', 'idx', 'val')))
    assert len(rec) == 9
    helds = {}
    for cid, r in sorted(rec.items()):
        thr, seed = (int(x) for x in r['split'])
        A, obs, held = matrix(r, 'from'), matrix(r, 'obs'), matrix(r, 'held')
        want = cb.split_entries(A, thr, seed)
        assert same(obs, want[0]) and same(held, want[1]), cid
        total = sp.csr_matrix(obs + held)
        total.sort_indices()
        assert same(total, A) and obs.nnz + held.nnz == A.nnz and obs.multiply(held).nnz == 0, cid          # disjoint; their union is A
        assert (obs.has_canonical_format or obs.nnz == 0) and (held.has_canonical_format or held.nnz == 0), cid
        assert int(r['asone'][0]) == 1, cid
        # an entry whose count is 1 goes where the binomial split of the restated generator sends it
        ones = sp.csr_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
        assert np.array_equal(dc.split(ones, thr, seed)[1].indices, held.indices) and np.array_equal(dc.split(ones, thr, seed)[1].indptr, held.indptr), cid
        helds[cid] = (thr, seed, held, A)
    assert [helds[c][:2] for c in (0, 1, 2, 3, 4)] == [(1 << 31, 12345), (1 << 31, 12346), (1288490188, (5 << 32) | 12345), (1, 3), ((1 << 32) - 1, 3)]
    assert not same(helds[0][2], helds[1][2])                           # a second seed gives another split
    assert helds[3][2].nnz == 0 and helds[4][2].nnz == helds[4][3].nnz  # the extreme thresholds (these few entries: none and all)
    assert (helds[0][3].data < 0).any() and (helds[0][3].data != np.floor(helds[0][3].data)).any() and (np.diff(helds[0][3].indptr) == 0).any()
    assert (helds[5][3].data == 1).all() and helds[8][3].shape == (0, 5)
    # the sanity bound: about 12000 entries, the held share within five standard deviations of q N (seed 12345: -0.07 and -0.44)
    for cid, q_named in ((6, 0.05), (7, 0.3)):
        thr, seed, held, A = helds[cid]
        N, H, q = A.nnz, held.nnz, thr / 2.0 ** 32
        assert seed == 12345 and abs(q - q_named) < 2.0 ** -32 and 11000 <= N <= 13000, (cid, N)
        print('split_entries sanity: q %.2f  N %d  H %d  %+.2f standard deviations' % (q_named, N, H, (H - q * N) / np.sqrt(q * (1 - q) * N)))
        assert abs(H - q * N) <= 5 * np.sqrt(q * (1 - q) * N), (cid, N, H)


PROTOS = {
    'rri_corpus_from_pairs': 'rri_ctx* ctx, rri_corpus** out, int64_t n_rows, int64_t n_cols, int64_t n_pairs, const void* rows, '
                             'const void* cols, int32_t index_dtype, int64_t index_stride, const void* values, int32_t values_dtype, '
                             'int32_t on_device',
    'rri_corpus_split_entries': 'rri_ctx* ctx, const rri_corpus* src, uint32_t threshold, uint64_t seed, rri_corpus** observed, rri_corpus** held',
}
CTYPES = {'rri_ctx*': ctypes.c_void_p, 'const rri_corpus*': ctypes.c_void_p, 'rri_corpus**': ctypes.POINTER(ctypes.c_void_p),
          'int64_t': ctypes.c_int64, 'int32_t': ctypes.c_int32, 'uint32_t': ctypes.c_uint32, 'uint64_t': ctypes.c_uint64,
          'const void*': ctypes.c_void_p}


def test_the_new_header_is_plain_c_bound_exported_documented_and_refuses_without_a_handle():
    text = open(os.path.join(ROOT, 'include', 'rri_corpus_build.h')).read()
    assert '#include "rri_hip.h"' in text and _capi.ABI_VERSION == 1
    assert re.search(r'#define RRI_ABI_VERSION 1\b', open(os.path.join(ROOT, 'include', 'rri_hip.h')).read())      # additions, not a new ABI
    declared = re.findall(r'^rri_status (rri_\w+)\(', text, flags=re.M)
    assert sorted(declared) == sorted(PROTOS) == sorted(_capi.CORPUS_BUILD_PROTOTYPES)
    assert not set(_capi.CORPUS_BUILD_PROTOTYPES) & (set(_capi.PROTOTYPES) | set(_capi.CORPUS_OPS_PROTOTYPES))
    for name, want in PROTOS.items():
        proto = re.search(r'^rri_status %s\(([^;]*)\);' % name, text, flags=re.M)
        assert proto and re.sub(r'\s+', ' ', proto.group(1)) == want, name
        res, args = _capi.CORPUS_BUILD_PROTOTYPES[name]
        assert res is ctypes.c_int32 and args == [CTYPES[a.rsplit(' ', 1)[0]] for a in want.split(', ')], name
    # the header compiles as C99, alone
    cc_ = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    assert cc_, 'no host C compiler'
    subprocess.run([cc_, '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c', '-I' + os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'include', 'rri_corpus_build.h')], check=True)
    # every declared symbol is exported and typed by load_library
    lib = _capi.load_library()
    for name, (res, args) in _capi.CORPUS_BUILD_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args, name
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        body = open(os.path.join(ROOT, doc)).read()
        assert all(name in body for name in PROTOS) and 'rri_corpus_build.h' in body, doc
    assert 'corpus_build_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()
    assert 'rri_corpus_build.h' in open(os.path.join(ROOT, 'rri_nmf_amd', 'build.py')).read()
    # a NULL handle: RRI_ERR_INVALID without a device, and nothing is written or counted
    BAD = _capi.RRI_ERR_INVALID
    out, out2 = ctypes.c_void_p(7), ctypes.c_void_p(9)
    rows = (ctypes.c_int64 * 2)(0, 1)
    assert lib.rri_corpus_from_pairs(None, ctypes.byref(out), 2, 2, 2, rows, rows, _capi.RRI_I64, 1, None, _capi.RRI_F64, 0) == BAD and out.value == 7
    assert lib.rri_corpus_split_entries(None, None, 1 << 31, 0, ctypes.byref(out), ctypes.byref(out2)) == BAD and (out.value, out2.value) == (7, 9)
    corpora, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.rri_corpus_memory(ctypes.byref(corpora), ctypes.byref(nbytes)) == 0 and (corpora.value, nbytes.value) == (0, 0)


# ---- the host logic of DeviceCorpus.from_pairs and split_entries, with stand-ins for the device ------------------------------------
class FakeLib(object):
    """records what rri_corpus_from_pairs / rri_corpus_split_entries are handed, reading the arrays through the pointers"""

    def __init__(self, status=0):
        self.calls, self.status = [], status

    def rri_corpus_from_pairs(self, h, out, n_rows, n_cols, n_pairs, rows, cols, idt, stride, values, vdt, on_device):
        isz = 4 if idt == _capi.RRI_I32 else 8
        it = ctypes.c_int32 if isz == 4 else ctypes.c_int64

        def read(ptr):
            if not ptr.value or on_device:
                return ptr.value
            return [ctypes.cast(ptr.value + p * stride * isz, ctypes.POINTER(it))[0] for p in range(n_pairs)]
        vals = None
        if values.value and not on_device:
            vt = ctypes.c_float if vdt == _capi.RRI_F32 else ctypes.c_double
            vals = [ctypes.cast(values.value, ctypes.POINTER(vt))[p] for p in range(n_pairs)]
        self.calls.append(dict(shape=(n_rows, n_cols), n_pairs=n_pairs, rows=read(rows), cols=read(cols), idt=idt, stride=stride, values=vals,
                               has_values=bool(values.value), vdt=vdt, on_device=on_device, gap=(cols.value or 0) - (rows.value or 0)))
        return self.status

    def rri_corpus_split_entries(self, h, src, thr, seed, observed, held):
        self.calls.append(dict(thr=thr, seed=seed))
        return self.status


class FakeEngine(object):
    _h = None

    def __init__(self, status):
        self.status = status

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def _check(self, st):
        if st == _capi.RRI_ERR_INVALID:
            raise ValueError('refused')
        if st == _capi.RRI_ERR_UNSUPPORTED:
            raise NotImplementedError('too large')


def patched(monkeypatch, status=0):
    from rri_nmf_amd.engine import DeviceCorpus
    lib = FakeLib(status)
    monkeypatch.setattr(_capi, 'load_library', lambda path=None: lib)
    monkeypatch.setattr(DeviceCorpus, '_handle', lambda self: FakeEngine(status))
    monkeypatch.setattr(DeviceCorpus, '_read_info', lambda self: None)
    monkeypatch.setattr(DeviceCorpus, 'close', lambda self: None)
    return DeviceCorpus, lib


def test_from_pairs_picks_the_stride_widens_the_dtypes_and_infers_the_shape(monkeypatch):
    D, lib = patched(monkeypatch)
    R, Cc, V = [3, 0, 3, 1], [5, 2, 5, 0], [1.0, 2.5, -1.0, 4.0]
    # an (m, 2) int64 or int32 array: read where it lies, with a stride of 2, the columns one element behind the rows
    for dt, code, isz in ((np.int64, _capi.RRI_I64, 8), (np.int32, _capi.RRI_I32, 4)):
        pairs = np.column_stack((R, Cc)).astype(dt)
        c = D.from_pairs(pairs, V, shape=(4, 6))
        call = lib.calls[-1]
        assert (call['stride'], call['idt'], call['gap'], call['on_device']) == (2, code, isz, 0) and call['rows'] == R and call['cols'] == Cc
        assert call['values'] == V and call['vdt'] == _capi.RRI_F64 and call['shape'] == (4, 6) == c.shape and call['n_pairs'] == 4
    # other integers widen to int64; a Fortran-ordered or sliced array is copied to C order first
    for pairs in (np.column_stack((R, Cc)).astype(np.int16), np.asfortranarray(np.column_stack((R, Cc))), np.column_stack((R, Cc, R))[:, :2],
                  np.column_stack((R, Cc)).astype(np.uint32), [[3, 5], [0, 2], [3, 5], [1, 0]]):
        D.from_pairs(pairs, shape=(4, 6))
        call = lib.calls[-1]
        assert (call['stride'], call['idt'], call['gap']) == (2, _capi.RRI_I64, 8) and call['rows'] == R and call['cols'] == Cc
        assert not call['has_values'] and call['values'] is None                # values=None: NULL, every pair counts 1
    # rows with cols=: two arrays, a stride of 1; one dtype for both, the wider
    D.from_pairs(np.array(R, dtype=np.int32), V, shape=(4, 6), cols=np.array(Cc, dtype=np.int32))
    assert (lib.calls[-1]['stride'], lib.calls[-1]['idt'], lib.calls[-1]['rows'], lib.calls[-1]['cols']) == (1, _capi.RRI_I32, R, Cc)
    D.from_pairs(np.array(R, dtype=np.int32), V, shape=(4, 6), cols=np.array(Cc, dtype=np.int64))
    assert (lib.calls[-1]['stride'], lib.calls[-1]['idt'], lib.calls[-1]['rows'], lib.calls[-1]['cols']) == (1, _capi.RRI_I64, R, Cc)
    D.from_pairs(np.array(R)[::-1], V, shape=(4, 6), cols=np.array(Cc)[::-1])                        # views that are not contiguous
    assert lib.calls[-1]['rows'] == R[::-1] and lib.calls[-1]['cols'] == Cc[::-1]
    # values: float32 stays, anything else becomes float64
    D.from_pairs(np.column_stack((R, Cc)), np.array(V, dtype=np.float32), shape=(4, 6))
    assert lib.calls[-1]['vdt'] == _capi.RRI_F32 and lib.calls[-1]['values'] == V
    D.from_pairs(np.column_stack((R, Cc)), np.array([1, 2, 3, 4], dtype=np.int8), shape=(4, 6))
    assert lib.calls[-1]['vdt'] == _capi.RRI_F64 and lib.calls[-1]['values'] == [1.0, 2.0, 3.0, 4.0]
    # the shape of host arrays: the largest indices plus one; an empty list gives (0, 0) and NULL arrays
    assert D.from_pairs(np.column_stack((R, Cc))).shape == (4, 6) and lib.calls[-1]['shape'] == (4, 6)
    assert D.from_pairs(np.array(R), cols=np.array(Cc)).shape == (4, 6)
    assert D.from_pairs(np.zeros((0, 2), dtype=np.int64)).shape == (0, 0)
    assert lib.calls[-1]['n_pairs'] == 0 and lib.calls[-1]['rows'] is None and lib.calls[-1]['cols'] is None
    assert D.from_pairs(np.zeros((0, 2), dtype=np.int32), shape=(5, 3)).shape == (5, 3)
    for bad in (dict(pairs=np.array(R)), dict(pairs=np.column_stack((R, Cc, R))), dict(pairs=np.array([[0.5, 1.0]])),
                dict(pairs=np.array(R), cols=np.array(Cc[:3])), dict(pairs=np.array(R), cols=np.array([0.5] * 4)),
                dict(pairs=np.column_stack((R, Cc)), values=V[:3]), dict(pairs=np.column_stack((R, Cc)), shape=(4, 6, 1))):
        with pytest.raises(ValueError):
            D.from_pairs(**bad)


class FakeTensor(object):
    """a GPU tensor in the duck-typed sense of from_device"""

    class Dev(object):
        type, index = 'cuda', 2

    def __init__(self, ptr, dtype, shape):
        self.ptr, self.dtype, self.shape, self.device = ptr, dtype, shape, self.Dev()

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return int(np.prod(self.shape))


def test_from_pairs_reads_gpu_tensors_where_they_are_and_needs_their_shape(monkeypatch):
    D, lib = patched(monkeypatch)
    pairs, vals = FakeTensor(4096, 'torch.int32', (10, 2)), FakeTensor(8192, 'torch.float32', (10,))
    c = D.from_pairs(pairs, vals, shape=(7, 9), device=0)
    call = lib.calls[-1]
    assert (call['on_device'], call['stride'], call['idt'], call['rows'], call['cols'], call['vdt']) == (1, 2, _capi.RRI_I32, 4096, 4100, _capi.RRI_F32)
    assert c.device == 2 and call['n_pairs'] == 10 and call['has_values']                      # where the tensors live
    rows, cols = FakeTensor(4096, 'torch.int64', (10,)), FakeTensor(16384, 'torch.int64', (10,))
    D.from_pairs(rows, None, shape=(7, 9), cols=cols)
    call = lib.calls[-1]
    assert (call['on_device'], call['stride'], call['idt'], call['rows'], call['cols'], call['has_values']) == (1, 1, _capi.RRI_I64, 4096, 16384, False)
    with pytest.raises(ValueError, match='shape'):
        D.from_pairs(pairs, vals)
    with pytest.raises(ValueError):
        D.from_pairs(rows, None, shape=(7, 9), cols=FakeTensor(16384, 'torch.int32', (10,)))      # two dtypes
    with pytest.raises(ValueError):
        D.from_pairs(rows, None, shape=(7, 9))                                                     # rows without cols
    with pytest.raises(ValueError):
        D.from_pairs(pairs, FakeTensor(8192, 'torch.float32', (9,)), shape=(7, 9))
    with pytest.raises(ValueError):
        D.from_pairs(pairs, np.zeros(10), shape=(7, 9))                                            # a host array beside a tensor
    with pytest.raises(TypeError):
        D.from_pairs(FakeTensor(4096, 'torch.float32', (10, 2)), None, shape=(7, 9))


def test_refusals_of_the_library_become_the_exceptions_of_device_corpus(monkeypatch):
    D, lib = patched(monkeypatch, _capi.RRI_ERR_INVALID)
    with pytest.raises(ValueError, match='refused'):
        D.from_pairs(np.array([[0, 9]]), shape=(1, 5))
    D, lib = patched(monkeypatch, _capi.RRI_ERR_UNSUPPORTED)
    with pytest.raises(NotImplementedError):
        D.from_pairs(np.array([[0, 9]]), shape=(1, 2 ** 31))
    assert lib.calls[-1]['shape'] == (1, 2 ** 31)
    # the real mapping of RRIEngine._check, which DeviceCorpus goes through
    from rri_nmf_amd.engine import RRIEngine
    eng = RRIEngine.__new__(RRIEngine)
    eng._err = lambda: 'row 7 at pair 3 is out of range'
    with pytest.raises(ValueError, match='row 7 at pair 3'):
        eng._check(_capi.RRI_ERR_INVALID)
    with pytest.raises(NotImplementedError):
        eng._check(_capi.RRI_ERR_UNSUPPORTED)


def test_split_entries_takes_its_threshold_and_seed_from_split_counts_and_the_public_function_dispatches(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    D, lib = patched(monkeypatch)
    monkeypatch.setattr(D, '_adopt', classmethod(lambda cls, c, device, lib_: ('corpus', device)))
    c = D.__new__(D)
    c._c, c._lib, c.device = ctypes.c_void_p(1), lib, 3
    assert c.split_entries() == (('corpus', 3), ('corpus', 3)) and lib.calls[-1] == dict(thr=D._split_threshold(0.05), seed=0)
    assert lib.calls[-1]['thr'] == int(0.05 * 2 ** 32) == dc.threshold(0.05)
    c.split_entries(held_out=0.3, random_state=(5 << 32) | 7)
    assert lib.calls[-1] == dict(thr=1288490188, seed=(5 << 32) | 7)
    rs = np.random.RandomState(3)
    lo, hi = (int(v) for v in np.random.RandomState(3).randint(0, 1 << 32, size=2, dtype=np.uint64))
    c.split_entries(0.5, rs)
    assert lib.calls[-1] == dict(thr=1 << 31, seed=lo | (hi << 32))
    for bad in (0.0, 1.0, 2.0 ** -33):
        with pytest.raises(ValueError, match='held_out'):
            c.split_entries(bad)
    with pytest.raises(TypeError):
        c.split_entries(0.5, 1.5)
    c._c = ctypes.c_void_p()
    with pytest.raises(ValueError, match='closed'):
        c.split_entries()

    class Corpus(D):
        def __init__(self):
            self.calls = []

        def split_entries(self, held_out=0.05, random_state=0):
            self.calls.append((held_out, random_state))
            return 'observed', 'held'
    k = Corpus()
    assert si.split_entries(k) == ('observed', 'held') and k.calls == [(0.05, 0)]
    assert si.split_entries(k, held_out=0.25, random_state=rs) == ('observed', 'held') and k.calls[-1] == (0.25, rs)
    doc = si.split_entries.__doc__
    assert 'DeviceCorpus' in doc and 'different split' in doc and 'equally valid' in doc
    # the host route: whole entries with their values, disjoint, their union the canonical matrix; reproducible from its seed
    rng = np.random.RandomState(5)
    X = sp.random(60, 50, density=0.3, format='csr', random_state=rng, data_rvs=lambda m: rng.randn(m))
    X.data[:5] = 0.0
    A = sp.csr_matrix(X, copy=True)
    A.eliminate_zeros()
    for held_out, seed in ((0.05, 0), (0.3, 11)):
        observed, held = si.split_entries(X, held_out=held_out, random_state=seed)
        total = sp.csr_matrix(observed + held)
        total.sort_indices()
        assert same(total, A) and observed.multiply(held).nnz == 0 and observed.nnz + held.nnz == A.nnz
        assert observed.has_canonical_format and held.has_canonical_format
        mask = np.random.RandomState(seed).random_sample(A.nnz) < held_out
        assert np.array_equal(bits(held.data), bits(A.data[mask])) and np.array_equal(held.indices, A.indices[mask])
        again = si.split_entries(X, held_out=held_out, random_state=seed)
        assert same(again[0], observed) and same(again[1], held)
        assert abs(held.nnz - held_out * A.nnz) <= 5 * np.sqrt(held_out * (1 - held_out) * A.nnz)
    with pytest.raises(ValueError, match='held_out'):
        si.split_entries(X, held_out=1.0)


def test_the_recommender_takes_a_device_corpus_through_one_download(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    from rri_nmf_amd.engine import DeviceCorpus
    rng = np.random.RandomState(2)
    A = sp.random(12, 9, density=0.4, format='csr', random_state=rng, data_rvs=lambda m: rng.randint(1, 6, size=m).astype(np.float64))

    class Corpus(DeviceCorpus):
        def __init__(self):
            self.downloads, self.shape = 0, A.shape

        def to_scipy(self):
            self.downloads += 1
            return A.copy()

        def close(self):
            pass
    E = si.NMF_RS_Estimator(12, 9, 3)
    # fit_from_Xtr: the pairs and values of the downloaded matrix reach fit
    seen = []
    monkeypatch.setattr(si.NMF_RS_Estimator, 'fit', lambda self, X, y=None: seen.append((np.asarray(X), np.asarray(y))) or self)
    c = Corpus()
    assert E.fit_from_Xtr(c) is E and c.downloads == 1
    rows, cols = A.nonzero()
    assert np.array_equal(seen[-1][0], np.column_stack((rows, cols))) and np.array_equal(seen[-1][1], A.data)
    E.fit_from_Xtr(A)
    assert np.array_equal(seen[-1][0], seen[-2][0]) and np.array_equal(seen[-1][1], seen[-2][1])
    # score: the same number as for the matrix
    E.W, E.T = rng.rand(12, 3), rng.rand(3, 9)
    E.min_rating, E.max_rating = 1.0, 5.0
    c = Corpus()
    assert E.score(c) == E.score(A) and c.downloads == 1
    # rank and ranking_score: the matrix reaches the code below once, as pairs
    asked = []

    def fake_rank(self, X, exclude_seen=True):
        asked.append(X)
        m = len(X)
        return np.zeros(m, dtype=np.int32), np.full(m, 9, dtype=np.int32)
    c = Corpus()
    inner = si.NMF_RS_Estimator.rank
    monkeypatch.setattr(si.NMF_RS_Estimator, 'rank', fake_rank)
    got = E.ranking_score(c, n_items=3, exclude_seen=False)
    assert c.downloads == 1 and isinstance(asked[-1], np.ndarray) and asked[-1].shape == (A.nnz, 2) and got == E.ranking_score(A, n_items=3, exclude_seen=False)
    monkeypatch.setattr(si.NMF_RS_Estimator, 'rank', inner)
    pairs = []
    monkeypatch.setattr(si.NMF_RS_Estimator, '_pairs_of', lambda self, X, y=None: pairs.append(X) or (_ for _ in ()).throw(KeyError('stop')))
    c = Corpus()
    with pytest.raises(KeyError):
        E.rank(c, exclude_seen=False)
    assert c.downloads == 1 and sp.issparse(pairs[-1]) and same(pairs[-1], A)
    for fn in (si.NMF_RS_Estimator.fit_from_Xtr, si.NMF_RS_Estimator.score, inner, si.NMF_RS_Estimator.ranking_score):
        assert 'DeviceCorpus' in fn.__doc__ and 'to_scipy()' in fn.__doc__ and 'not built' in fn.__doc__
