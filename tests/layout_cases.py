"""Talking to tests/c/layout_main.cpp, the stand-alone program over rri_nmf_amd/csrc/rri_layout.hpp: shared by
tests/test_layout_cpu.py (built under the sanitizers, compared with the Python restatements of the suites) and
tests/test_layout_plan_gpu.py (built plain, compared with what a handle reports).

A Session collects requests, runs the program ONCE over all of them and hands every request its answer: one dict of integers per
request, plus the arrays of a blocked copy or of a row sort.  Request lines (all fields integers but the capacity):

    plan  n d k dtype flavour n_cu pk_rows pk_il x_pack cache_mb        the dense plan of rri_create (dense_plan)
    keep  <the fields of plan> ldw xp_valid                             pass_keep and its terms
    early <the fields of plan> n_cu                                     the early-sums schedule of that plan (RRI_PASS_PK_GEOM: pk_rows, pk_il)
    onchip n LD k is_f32 proj n_cu                                      the persistent sweep's geometry
    copy  which sparse_x es n_cu n d nnz indptr... indices...           one blocked copy of a CSR pattern (build_sp_copy)
    csr   rules n d nnz dtype has_data len indptr... len indices...     csr_check (len -1: a null pointer)
    sort  ds n nnz indptr... indices... values...                       csr_sort_rows, then csr_duplicates
    wmcorr_cols | wmcorr | resid | small | tall | spxlps | xpack        the small grids
"""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RRI_F32, RRI_F64, RRI_F16, RRI_U8 = 0, 1, 2, 4        # include/rri_hip.h
DTYPE_CODE = {'fp32': RRI_F32, 'fp64': RRI_F64, 'fp16': RRI_F16, 'u8': RRI_U8}
UNWEIGHTED, WEIGHTED_DENSE, WEIGHTED_SPARSE, UNWEIGHTED_RESIDUAL, UNWEIGHTED_SPARSE = range(5)
CSR_ROWS, CSR_COLUMNS, CSR_INCREASING = 0, 1, 2
_LINES = {'copy': 5, 'sort': 3}


def code_of(dtype):
    return {np.dtype(np.float32): RRI_F32, np.dtype(np.float64): RRI_F64, np.dtype(np.float16): RRI_F16,
            np.dtype(np.uint8): RRI_U8}[np.dtype(dtype)]


def build_program(tmp_path, sanitize):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'layout')
    flags = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] if sanitize else ['-O1']
    subprocess.run([cxx, '-std=c++17'] + flags + ['-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'layout_main.cpp'), '-o', exe], check=True)
    return exe


def plan_line(n, d, k, dtype, flavour=UNWEIGHTED, n_cu=256, pk_rows=0, pk_il=-1, x_pack=-1, cache_mb=256.0):
    return 'plan %d %d %d %d %d %d %d %d %d %r' % (n, d, k, dtype, flavour, n_cu, pk_rows, pk_il, x_pack, float(cache_mb))


def keep_line(n, d, k, dtype, ldw=None, xp_valid=False, **kw):
    return 'keep' + plan_line(n, d, k, dtype, **kw)[4:] + ' %d %d' % (n if ldw is None else ldw, int(xp_valid))


def early_line(n, d, k, dtype, n_cu=256, **kw):
    return 'early' + plan_line(n, d, k, dtype, n_cu=n_cu, **kw)[4:] + ' %d' % n_cu


def copy_line(A, which, csrx, es, n_cu):
    """A: scipy CSR with sorted indices"""
    return 'copy %d %d %d %d %d %d %d %s %s' % (which, int(csrx), es, n_cu, A.shape[0], A.shape[1], A.nnz,
                                               ' '.join(map(str, A.indptr.tolist())), ' '.join(map(str, A.indices.tolist())))


def csr_line(rules, n, d, nnz, dtype, indptr, indices, has_data=True):
    arr = lambda a: '-1' if a is None else ' '.join(map(str, [len(a)] + list(a)))
    return 'csr %d %d %d %d %d %d %s %s' % (rules, n, d, nnz, dtype, int(has_data), arr(indptr), arr(indices))


def sort_line(ds, indptr, indices, values):
    return 'sort %d %d %d %s %s %s' % (ds, len(indptr) - 1, len(indices), ' '.join(map(str, indptr)), ' '.join(map(str, indices)),
                                      ' '.join(map(str, values)))


def _fields(line):
    out = {}
    for tok in line.split()[1:]:
        kk, vv = tok.split('=', 1)
        try:
            out[kk] = int(vv)
        except ValueError:
            out[kk] = float(vv)
    return out


def _array(line, name):
    toks = line.split()
    assert toks[0] == name, (name, line[:80])
    return np.array(toks[1:], dtype=np.int64)


class Session(object):
    def __init__(self):
        self.requests, self.answers = [], None

    def ask(self, line):
        self.requests.append(line)
        return len(self.requests) - 1

    def run(self, exe):
        res = subprocess.run([exe], input='\n'.join(self.requests) + '\n', stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert res.returncode == 0, res.stdout[-4000:]
        lines = res.stdout.splitlines()
        assert lines[-1] == 'ok', lines[-1]
        self.answers, at = [], 0
        for req in self.requests:
            kind = req.split(None, 1)[0]
            take = _LINES.get(kind, 1)
            chunk = lines[at:at + take]
            at += take
            assert chunk[0].split(None, 1)[0] == kind, (req[:80], chunk[0][:80])
            if kind == 'csr':
                self.answers.append(chunk[0][4:])
            elif kind == 'sort':
                head, dup = chunk[0].split(' dup=', 1)
                ans = dict(copied=int(head.split()[1].split('=')[1]), copies=head.split()[2].split('=')[1], dup=dup)
                ans.update(indices=_array(chunk[1], 'sorted_indices'), values=_array(chunk[2], 'sorted_values'))
                self.answers.append(ans)
            else:
                ans = _fields(chunk[0])
                if kind == 'copy':
                    ans.update(work=_array(chunk[1], 'work').reshape(-1, 4), segptr=_array(chunk[2], 'segptr'),
                               idx=_array(chunk[3], 'idx'), perm=_array(chunk[4], 'perm'))
                self.answers.append(ans)
        assert at == len(lines) - 1, 'the program printed %d lines, the requests account for %d' % (len(lines) - 1, at)
        return self

    def __getitem__(self, i):
        return self.answers[i]
