"""Corpora derived from a resident corpus, without a GPU: the generator, the threshold, the held part, the pieces, the refusals and
the three plain loops of rri_nmf_amd/csrc/rri_derive.hpp under sanitizers, the ABI surface of include/rri_corpus_ops.h and the
refusals of the real library that need no device, and the host logic of DeviceCorpus with stand-ins for the device.

tests/c/derive_main.cpp is a stand-alone program with its own main that includes the header alone.  It is built once with the
host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once; what it prints is compared with what is written
here, with scipy and with the vectorised numpy restatement (tests/derive_cases.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import derive_cases as dc
from rri_nmf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('derive') / 'derive')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'derive_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    out = res.stdout.strip().splitlines()
    assert out[-1] == 'ok 6 6 cases', out[-1]
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


def same(A, B):
    return (A.shape == B.shape and np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)
            and np.array_equal(np.asarray(A.data, dtype=np.float64).view(np.uint64), np.asarray(B.data, dtype=np.float64).view(np.uint64)))


def test_the_generator_the_threshold_and_the_held_part(lines):
    assert 'consts : %d %d %d %d' % (dc.PIECE, dc.LANE_MAX, dc.COUNT_MAX, dc.RULES) in lines
    assert dc.PIECE % 64 == 0 and dc.LANE_MAX % 4 == 0 and dc.COUNT_MAX // 4 // 64 == 4096        # a lane walks 64, a wave's lane 4096 blocks
    # Philox4x32-10: the known answers, from the program and from the restatement
    kat = {0: ((0, 0, 0, 0, 0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           1: ((0xffffffff,) * 6, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           2: ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1')}
    for i, (args, want) in kat.items():
        assert 'philox %d : %s' % (i, want) in lines
        assert ' '.join('%08x' % int(w) for w in dc.philox(*args)) == want
    assert 'block : 1' in lines                    # counter (column, row low, row high, block), key (seed low, seed high)
    # the threshold: floor(held_out 2^32)
    thr = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in (re.match(r'thr (\w+) : (\d) (\d+)$', ln) for ln in lines) if m}
    assert thr == {'half': (1, 1 << 31), 'three_tenths': (1, 1288490188), 'smallest': (1, 1), 'below_smallest': (0, 0),
                   'below_one': (1, (1 << 32) - 1), 'one': (0, 0), 'zero': (0, 0), 'negative': (0, 0), 'nan': (0, 0)}
    assert 1288490188 == int(0.3 * 2 ** 32) and dc.threshold(0.3) == 1288490188 and dc.threshold(0.5) == 1 << 31
    assert dc.threshold(2.0 ** -32) == 1 and dc.threshold(np.nextafter(1.0, 0.0)) == (1 << 32) - 1 and dc.threshold(1.0) is None
    # the held part: token by token, as 64 lanes share the blocks, and the restatement
    held = [[int(x) for x in re.split(r'[ :]+', ln)[1:]] for ln in lines if ln.startswith('held ')]
    counts = [0, 1, 3, 4, 5, 8, 9, dc.LANE_MAX - 1, dc.LANE_MAX, dc.LANE_MAX + 1, dc.COUNT_MAX]
    assert [h[4] for h in held] == counts * 2 and len({(h[0], h[1], h[2]) for h in held}) == 2 and max(h[0] for h in held) > 2 ** 32
    for row, col, seed, t, count, plain, lanes in held:
        assert plain == lanes == dc.held_part([row], [col], [count], t, seed)[0], (row, col, count)
        assert 0 <= plain <= count
    big = [h for h in held if h[4] == dc.COUNT_MAX]
    for row, col, seed, t, count, plain, _ in big:          # a million tokens: within five standard deviations of the share
        q = t / 2.0 ** 32
        assert abs(plain - q * count) <= 5 * np.sqrt(q * (1 - q) * count)
    # the pieces of rows on both sides of the piece length
    pr = records(lines, ('piecerow', 'piecesrc', 'piecelen'))
    lengths = [0, 1, dc.PIECE - 1, dc.PIECE, dc.PIECE + 1, 2 * dc.PIECE + 1]
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    for cid, rows in ((0, None), (1, [5, 0, 4, 4, 1])):
        got = list(zip(*(pr[cid][key].astype(np.int64).tolist() for key in ('piecerow', 'piecesrc', 'piecelen'))))
        assert got == dc.pieces(indptr, rows), cid
        assert sum(g[2] for g in got) == sum(lengths[r] for r in (range(6) if rows is None else rows)) and max(g[2] for g in got) == dc.PIECE


def test_every_refusal_has_its_verdict_and_text_and_the_first_broken_rule_wins(lines):
    got = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'req (\w+) : (-?\d+) : (.*)$', ln) for ln in lines) if m}
    assert set(got) == set(dc.REQUEST_FINE) | set(dc.REQUEST_TEXT) | set(dc.VALUES)
    for name in dc.REQUEST_FINE:
        assert got[name] == (dc.OK, ''), name
    for name, text in dc.REQUEST_TEXT.items():
        assert got[name] == (dc.INVALID, text), name
    for name, values in dc.VALUES.items():
        want = dc.check_values(values)
        assert got[name] == want and want[0] == (dc.UNSUPPORTED if name.startswith('too_large') else dc.INVALID), name
    assert got['negative_at_2'][1] == 'value -1 at entry 2 is negative: a split takes counts'
    assert got['half_at_1'][1] == 'value 0.5 at entry 1 is not a whole number: a split takes counts'
    assert got['too_large_at_0'][1] == 'value 1048577 at entry 0 is above 1048576, the largest count that is split'
    assert dc.check_values([1.0, float(dc.COUNT_MAX)]) == (dc.OK, '')
    # every kind of refusal stands at two places
    kinds = {}
    for name in list(dc.REQUEST_TEXT) + list(dc.VALUES):
        kinds.setdefault(re.sub(r'-?\d[\w.]*', '#', got[name][1]), []).append(name)
    once = {('corpus_dead',), ('threshold_zero',)}              # a dead corpus and a threshold of 0 have no second place to stand
    assert all(len(v) >= 2 or tuple(v) in once for v in kinds.values()), kinds
    assert len(kinds) == 14


def test_select_and_column_counts_of_the_plain_loops_against_scipy(lines):
    rec = records(lines, ('select', 'srcshape', 'srcptr', 'srcidx', 'srcval', 'rows', 'keep', 'outshape', 'outptr', 'outidx', 'outval', 'df'))
    assert len(rec) == 6
    seen = dict(empty_row=0, negatives=0, reals=0, repeats=0, all_rows=0, all_cols=0, no_rows_taken=0, no_cols_kept=0, no_source_rows=0,
                emptied_rows=0)
    for cid, r in sorted(rec.items()):
        all_rows, all_cols = (bool(x) for x in r['select'])
        A, out = matrix(r, 'src'), matrix(r, 'out')
        assert A.has_canonical_format or A.nnz == 0, cid
        rows, keep = r['rows'].astype(np.int64), r['keep'].astype(np.int64)
        want = A if all_rows else A[rows]
        want = want if all_cols else want[:, keep]
        want = sp.csr_matrix(want)
        want.sort_indices()
        assert same(out, want), cid
        assert np.array_equal(r['df'].astype(np.int64), np.asarray((A != 0).sum(0)).ravel()), cid
        seen['empty_row'] += bool(A.shape[0] and (np.diff(A.indptr) == 0).any())
        seen['negatives'] += bool((A.data < 0).any())
        seen['reals'] += bool((A.data != np.floor(A.data)).any())
        seen['repeats'] += not all_rows and np.unique(rows).size < rows.size
        seen['all_rows'] += all_rows
        seen['all_cols'] += all_cols
        seen['no_rows_taken'] += not all_rows and rows.size == 0
        seen['no_cols_kept'] += not all_cols and keep.size == 0
        seen['no_source_rows'] += A.shape[0] == 0
        taken = np.diff(A.indptr)[slice(None) if all_rows else rows]
        seen['emptied_rows'] += bool(((taken > 0) & (np.diff(out.indptr) == 0)).any())
    assert all(seen.values()), seen


def test_split_of_the_plain_loop_against_the_restatement_and_its_sanity_bound(lines):
    rec = records(lines, ('split',) + tuple(n + k for n in ('from', 'obs', 'held') for k in ('shape', 'ptr', 'idx', 'val')))
    assert len(rec) == 6
    by_source = {}
    for cid, r in sorted(rec.items()):
        thr, seed = (int(x) for x in r['split'])
        A, obs, held = matrix(r, 'from'), matrix(r, 'obs'), matrix(r, 'held')
        want = dc.split(A, thr, seed)
        assert same(obs, want[0]) and same(held, want[1]), cid
        total = obs + held
        total.sort_indices()
        assert same(total, A), cid                                  # observed + held == A, exactly
        assert not (obs.data == 0).any() and not (held.data == 0).any() and (obs.data > 0).all() and (held.data > 0).all(), cid
        assert obs.has_canonical_format and held.has_canonical_format, cid
        by_source.setdefault((A.shape, A.nnz), []).append((thr, seed, held))
    small = by_source[((6, 20), rec[0]['fromidx'].size)]
    assert [s[:2] for s in small] == [(1 << 31, 12345), (1 << 31, 12346), (1288490188, (5 << 32) | 12345)]
    assert not same(small[0][2], small[1][2])                       # a second seed gives another split
    limits = matrix(rec[3], 'from')
    assert {dc.LANE_MAX - 1, dc.LANE_MAX, dc.LANE_MAX + 1, 1024, dc.COUNT_MAX} <= set(limits.data.astype(np.int64).tolist())
    # the sanity bound: about 12000 tokens, the held share within five standard deviations of q N (seed 12345: 0.57 and -1.3)
    for cid, q_named in ((4, 0.5), (5, 0.3)):
        thr, seed = (int(x) for x in rec[cid]['split'])
        A, held = matrix(rec[cid], 'from'), matrix(rec[cid], 'held')
        N, H, q = A.data.sum(), held.data.sum(), thr / 2.0 ** 32
        assert seed == 12345 and abs(q - q_named) < 2.0 ** -32 and 11000 <= N <= 13000, (cid, N)
        print('split sanity: q %.1f  N %d  H %d  %+.2f standard deviations' % (q_named, N, H, (H - q * N) / np.sqrt(q * (1 - q) * N)))
        assert abs(H - q * N) <= 5 * np.sqrt(q * (1 - q) * N), (cid, N, H)


PROTOS = {
    'rri_corpus_select': 'rri_ctx* ctx, const rri_corpus* src, const int64_t* rows, int64_t n_rows_out, const int32_t* keep, '
                         'int64_t n_cols_out, rri_corpus** out',
    'rri_corpus_column_counts': 'rri_ctx* ctx, const rri_corpus* src, int64_t* df_out',
    'rri_corpus_split': 'rri_ctx* ctx, const rri_corpus* src, uint32_t threshold, uint64_t seed, rri_corpus** observed, rri_corpus** held',
}
CTYPES = {'rri_ctx*': ctypes.c_void_p, 'const rri_corpus*': ctypes.c_void_p, 'rri_corpus**': ctypes.POINTER(ctypes.c_void_p),
          'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32, 'uint64_t': ctypes.c_uint64,
          'int64_t*': ctypes.POINTER(ctypes.c_int64), 'const int64_t*': ctypes.POINTER(ctypes.c_int64),
          'const int32_t*': ctypes.POINTER(ctypes.c_int32)}


def test_the_new_header_is_plain_c_bound_exported_documented_and_refuses_without_a_handle(tmp_path):
    text = open(os.path.join(ROOT, 'include', 'rri_corpus_ops.h')).read()
    assert '#include "rri_hip.h"' in text and _capi.ABI_VERSION == 1
    assert re.search(r'#define RRI_ABI_VERSION 1\b', open(os.path.join(ROOT, 'include', 'rri_hip.h')).read())      # additions, not a new ABI
    declared = re.findall(r'^rri_status (rri_\w+)\(', text, flags=re.M)
    assert sorted(declared) == sorted(PROTOS) == sorted(_capi.CORPUS_OPS_PROTOTYPES)
    assert not set(_capi.CORPUS_OPS_PROTOTYPES) & set(_capi.PROTOTYPES)
    for name, want in PROTOS.items():
        proto = re.search(r'^rri_status %s\(([^;]*)\);' % name, text, flags=re.M)
        assert proto and re.sub(r'\s+', ' ', proto.group(1)) == want, name
        res, args = _capi.CORPUS_OPS_PROTOTYPES[name]
        assert res is ctypes.c_int32 and args == [CTYPES[a.rsplit(' ', 1)[0]] for a in want.split(', ')], name
    # the header compiles as C99, alone
    cc_ = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    assert cc_, 'no host C compiler'
    subprocess.run([cc_, '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-x', 'c', '-I' + os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'include', 'rri_corpus_ops.h')], check=True)
    # every declared symbol is exported and typed by load_library
    lib = _capi.load_library()
    for name, (res, args) in _capi.CORPUS_OPS_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args, name
    for doc in ('README.md', 'DESIGN.md', 'INTEGRATION.md'):
        body = open(os.path.join(ROOT, doc)).read()
        assert all(name in body for name in PROTOS) and 'rri_corpus_ops.h' in body, doc
    assert 'derive_probe.py' in open(os.path.join(ROOT, 'tools', 'README.md')).read()
    assert 'rri_corpus_ops.h' in open(os.path.join(ROOT, 'rri_nmf_amd', 'build.py')).read()
    # a NULL handle: RRI_ERR_INVALID without a device, and nothing is written or counted
    BAD = _capi.RRI_ERR_INVALID
    out, out2, df = ctypes.c_void_p(7), ctypes.c_void_p(9), (ctypes.c_int64 * 2)(5, 5)
    assert lib.rri_corpus_select(None, None, None, 0, None, 0, ctypes.byref(out)) == BAD and out.value == 7
    assert lib.rri_corpus_column_counts(None, None, df) == BAD and list(df) == [5, 5]
    assert lib.rri_corpus_split(None, None, 1 << 31, 0, ctypes.byref(out), ctypes.byref(out2)) == BAD and (out.value, out2.value) == (7, 9)
    corpora, nbytes = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.rri_corpus_memory(ctypes.byref(corpora), ctypes.byref(nbytes)) == 0 and (corpora.value, nbytes.value) == (0, 0)


# ---- the host logic of DeviceCorpus, with stand-ins for the device ---------------------------------------------------------------
def stand_in(shape, df=None):
    """a DeviceCorpus that never saw the library: _select records what it is asked for, document_frequency returns df"""
    from rri_nmf_amd.engine import DeviceCorpus

    class StandIn(DeviceCorpus):
        def __init__(self):
            self.shape, self.device, self.asked = shape, 0, []

        def _select(self, rows, keep):
            self.asked.append((rows, keep))
            return 'derived'

        def document_frequency(self):
            return np.asarray(df, dtype=np.int64)

        def close(self):
            pass
    return StandIn()


def test_prune_words_selects_by_document_frequency_on_the_host():
    from rri_nmf_amd.engine import DeviceCorpus
    pick = DeviceCorpus._prune_selection
    df = np.array([0, 5, 10, 3, 10, 7, 1, 10, 2, 7])
    assert pick(df, 10).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9] and pick(df, 10).dtype == np.int32        # min_df = 1 drops the unused word
    assert pick(df, 10, min_df=0).tolist() == list(range(10))
    assert pick(df, 10, min_df=3).tolist() == [1, 2, 3, 4, 5, 7, 9]                       # an int: a number of documents
    assert pick(df, 10, min_df=3, max_df=7).tolist() == [1, 3, 5, 9]
    assert pick(df, 10, min_df=0.3, max_df=0.7).tolist() == [1, 3, 5, 9]                  # a float: a share of the rows
    assert pick(df, 20, min_df=0.3, max_df=0.7).tolist() == [2, 4, 5, 7, 9]               # ... of THESE rows: 6 <= df <= 14
    assert pick(df, 10, max_df=1.0).tolist() == pick(df, 10).tolist() and pick(df, 10, max_df=1).tolist() == [6]
    # max_words: the largest df, a tie goes to the lower column, and kept ascends
    assert pick(df, 10, max_words=3).tolist() == [2, 4, 7]
    assert pick(df, 10, max_words=2).tolist() == [2, 4]                                  # three words tie at the cut
    assert pick(df, 10, max_words=4).tolist() == [2, 4, 5, 7]                            # 5 and 9 tie: the lower column
    assert pick(df, 10, max_words=5).tolist() == [2, 4, 5, 7, 9]
    assert pick(df, 10, max_words=9).tolist() == pick(df, 10, max_words=50).tolist() == pick(df, 10).tolist()
    assert pick(df, 10, max_df=7, max_words=2).tolist() == [5, 9]                        # the cut applies to what the bounds left
    # every word dropped
    assert pick(df, 10, min_df=11).size == 0 and pick(df, 10, max_words=0).size == 0 and pick(df, 10, min_df=8, max_df=9).size == 0
    assert pick(np.zeros(0, dtype=np.int64), 10).size == 0
    for bad in (dict(min_df=1.5), dict(max_df=-0.1), dict(min_df=-1), dict(max_words=-1)):
        with pytest.raises(ValueError):
            pick(df, 10, **bad)
    # prune_words hands the selection to select_words and returns it
    c = stand_in((10, 10), df)
    out, kept = c.prune_words(min_df=3, max_df=0.7, max_words=3)
    assert out == 'derived' and kept.tolist() == [1, 5, 9] and len(c.asked) == 1
    assert c.asked[0][0] is None and c.asked[0][1].tolist() == [1, 5, 9] and c.asked[0][1].dtype == np.int32
    out, kept = c.prune_words(min_df=11)
    assert kept.size == 0 and c.asked[-1][1].size == 0 and c.asked[-1][1] is not None       # an empty list, not "all columns"


def test_slices_masks_and_index_arrays_become_row_and_column_lists():
    c = stand_in((10, 6))
    for index, want in ((slice(2, 5), [2, 3, 4]), (slice(None), list(range(10))), (slice(None, None, 3), [0, 3, 6, 9]),
                        (slice(8, 2, -2), [8, 6, 4]), (slice(7, 100), [7, 8, 9]), (slice(5, 5), []), (slice(-3, None), [7, 8, 9]),
                        (3, [3]), (-1, [9]), ([4, 4, 0, -2], [4, 4, 0, 8]), (np.array([], dtype=np.int64), []),
                        (np.arange(10) % 3 == 0, [0, 3, 6, 9]), (np.zeros(10, dtype=bool), [])):
        assert c[index] == 'derived'
        rows, keep = c.asked[-1]
        assert keep is None and rows.dtype == np.int64 and rows.tolist() == want, index
    for bad in ([10], [-11], np.ones(9, dtype=bool), [1.5], np.zeros((2, 2), dtype=np.int64)):
        with pytest.raises(IndexError):
            c[bad]
    assert c.take_rows([5, 0, 5]) == 'derived' and c.asked[-1][0].tolist() == [5, 0, 5] and c.asked[-1][1] is None
    assert c.take_rows(np.array([], dtype=np.int64)) == 'derived' and c.asked[-1][0].size == 0 and c.asked[-1][0] is not None
    with pytest.raises(ValueError):
        c.take_rows([0.5])
    # columns: an ascending list or a mask of length d; the order of a list is the library's to refuse
    for keep, want in (([0, 2, 5], [0, 2, 5]), (np.array([True, False, False, True, False, True]), [0, 3, 5]), ([], []),
                       (np.zeros(6, dtype=bool), []), (np.ones(6, dtype=bool), [0, 1, 2, 3, 4, 5])):
        assert c.select_words(keep) == 'derived'
        rows, got = c.asked[-1]
        assert rows is None and got.dtype == np.int32 and got.tolist() == want
    for bad in ([6], [-1], np.ones(5, dtype=bool), [0.5]):
        with pytest.raises(ValueError):
            c.select_words(bad)


def test_the_threshold_and_the_seed_of_split_counts():
    from rri_nmf_amd.engine import DeviceCorpus as D
    assert D._split_threshold(0.5) == 1 << 31 and D._split_threshold(0.3) == 1288490188 == dc.threshold(0.3)
    assert D._split_threshold(2.0 ** -32) == 1 and D._split_threshold(np.nextafter(1.0, 0.0)) == (1 << 32) - 1
    for bad in (0.0, 1.0, -0.5, 1.5, float('nan'), 2.0 ** -33, np.nextafter(2.0 ** -32, 0.0)):
        with pytest.raises(ValueError):
            D._split_threshold(bad)
    assert D._split_seed(0) == 0 and D._split_seed(12345) == 12345 and D._split_seed((1 << 64) - 1) == (1 << 64) - 1
    assert D._split_seed(np.int64(7)) == 7
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            D._split_seed(bad)
    for bad in (None, 1.5, 'seed', True):
        with pytest.raises(TypeError):
            D._split_seed(bad)
    lo, hi = (int(v) for v in np.random.RandomState(3).randint(0, 1 << 32, size=2, dtype=np.uint64))
    assert D._split_seed(np.random.RandomState(3)) == lo | (hi << 32) and hi > 0
    rs = np.random.RandomState(3)
    assert D._split_seed(rs) != D._split_seed(rs)              # a RandomState moves on: two calls, two splits


def test_split_counts_hands_a_corpus_to_the_device_and_leaves_the_host_route_as_it_was():
    from rri_nmf_amd import sklearn_interface as si
    from rri_nmf_amd.engine import DeviceCorpus

    class Corpus(DeviceCorpus):
        def __init__(self):
            self.calls = []

        def split_counts(self, held_out=0.5, random_state=0):
            self.calls.append((held_out, random_state))
            return 'observed', 'held'

        def close(self):
            pass
    c = Corpus()
    assert si.split_counts(c) == ('observed', 'held') and c.calls == [(0.5, 0)]
    rs = np.random.RandomState(4)
    assert si.split_counts(c, held_out=0.25, random_state=rs) == ('observed', 'held') and c.calls[-1] == (0.25, rs)
    doc = si.split_counts.__doc__
    assert 'DeviceCorpus' in doc and 'different split' in doc and 'equally valid' in doc
    # the host route: the same bits as the lines it has always run
    rng = np.random.RandomState(5)
    X = sp.random(40, 30, density=0.3, format='csr', random_state=rng, data_rvs=lambda m: rng.randint(1, 9, size=m).astype(np.float64))
    for held_out, seed in ((0.5, 0), (0.3, 11)):
        observed, held = si.split_counts(X, held_out=held_out, random_state=seed)
        A = sp.csr_matrix(X, copy=True)
        A.sum_duplicates()
        h = np.random.RandomState(seed).binomial(A.data.astype(np.int64), held_out).astype(A.dtype)
        want_h = sp.csr_matrix((h, A.indices.copy(), A.indptr.copy()), shape=A.shape)
        want_o = sp.csr_matrix((A.data - h, A.indices.copy(), A.indptr.copy()), shape=A.shape)
        want_h.eliminate_zeros()
        want_o.eliminate_zeros()
        assert same(held, want_h) and same(observed, want_o) and same((observed + held).tocsr(), A)
    with pytest.raises(ValueError, match='held_out'):
        si.split_counts(X, held_out=1.0)
    with pytest.raises(ValueError, match='counts'):
        si.split_counts(sp.csr_matrix(np.array([[0.5, 1.0]])))
