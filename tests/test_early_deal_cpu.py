"""Where the workgroups of the early-sums job sit in the grid of the fused pass (rri_nmf_amd/csrc/rri_early_deal.hpp),
on the CPU.

tests/c/early_deal_main.cpp is a stand-alone program with its own main over that header -- the text k_pass maps its block index
with -- and over the stride dense_plan hands to it.  It is built with the host compiler twice, plain and under AddressSanitizer
and UndefinedBehaviorSanitizer, and each binary is run once, directly.  For every grid (P own workgroups of the pass, the job's
first position, nblocks job workgroups) it walks every position 0 .. P + nblocks - 1 and checks, as this file does again on the
lines it prints against a restatement:
  * every job index 0 .. nblocks - 1 occurs exactly once, job workgroup i at first + i (s + 1), s = (P - first) // nblocks;
  * every own index 0 .. P - 1 occurs exactly once and in ascending order of position: a plain renumbering, which the rotation
    inside groups of 8 workgroups and the kept row blocks of k_pass rely on;
  * nothing is out of range;
  * s = 0 is the contiguous layout [first, first + nblocks) of RRI_EARLY_DEAL=0, position for position.

The grids: the flagship's plan (1960, 1024, 64: s = 14, 40 own workgroups behind the last of the job) and
    (1029, 1024, 43)            fewer workgroups behind `first` than the job has: s = 0
    (1024 + 43, 1024, 43)       as many: s = 1 and nothing left over
    (1024 + 3 * 43 + 1, ..)     s = 3 and ONE left over behind the last job workgroup
    (1100, 1024, 1)             one job workgroup: all 76 own workgroups follow it
    (2048, 1024, 64)            s = 16, nothing left over
    (700, 700, 10)              a pass of one round: first == P, the job last
each dealt and with s = 0.  The plan: the stride of the flagship shape and of the shapes of tests/test_early_deal_gpu.py at 256
compute units, with the switch on and off."""
import os
import shutil
import subprocess

import pytest

import test_early_deal_gpu as dg
from layout_cases import RRI_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRIDS = [(1960, 1024, 64), (1029, 1024, 43), (1024 + 43, 1024, 43), (1024 + 3 * 43 + 1, 1024, 43), (1100, 1024, 1), (2048, 1024, 64),
         (700, 700, 10)]
STRIDES = {(1960, 1024, 64): 14, (1029, 1024, 43): 0, (1067, 1024, 43): 1, (1154, 1024, 43): 3, (1100, 1024, 1): 76, (2048, 1024, 64): 16,
           (700, 700, 10): 0}


def stride(P, first, nblocks):
    return (P - first) // nblocks if nblocks > 0 and P > first else 0


def dealt(P, first, nblocks, s):
    """the layout, written the other way round from early_slot: position by position, (kind, index)"""
    out, own, job = [], 0, 0
    while own < first:
        out.append((0, own)); own += 1
    while job < nblocks:
        out.append((1, job)); job += 1
        for _ in range(s):
            out.append((0, own)); own += 1
    while own < P:
        out.append((0, own)); own += 1
    return out


def contiguous(P, first, nblocks):
    """today's placement: the job at [first, first + nblocks), the pass's own workgroups closed up around it"""
    return [(1, pos - first) if first <= pos < first + nblocks else (0, pos if pos < first else pos - nblocks) for pos in range(P + nblocks)]


def plan_line(n, d, k, deal, pk_rows=0, pk_il=-1, n_cu=256):
    return 'plan %d %d %d %d 0 %d %d %d %d' % (n, d, k, RRI_F32, n_cu, pk_rows, pk_il, deal)


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    tmp = tmp_path_factory.mktemp('early_deal')
    exes = {}
    for name, flags in (('plain', ['-O2']), ('sanitized', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exes[name] = str(tmp / ('early_deal_' + name))
        subprocess.run([cxx, '-std=c++17'] + flags + ['-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                        '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'early_deal_main.cpp'), '-o', exes[name]], check=True)
    return exes


def run(exe, requests):
    res = subprocess.run([exe], input='\n'.join(requests) + '\n', stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok', lines[-1]
    return lines[:-1]


@pytest.mark.parametrize('build', ['plain', 'sanitized'])
def test_every_position_of_every_grid(programs, build):
    requests, want = [], []
    for P, first, nblocks in GRIDS:
        s = stride(P, first, nblocks)
        assert s == STRIDES[(P, first, nblocks)], (P, first, nblocks, s)
        requests.append('stride %d %d %d' % (P, first, nblocks))
        for ss in (s, 0):
            requests.append('grid %d %d %d %d' % (P, first, nblocks, ss))
            want.append((P, first, nblocks, ss))
    lines = run(programs[build], requests)
    assert len(lines) == len(GRIDS) + 3 * len(want)
    at = 0
    for P, first, nblocks in GRIDS:
        assert lines[at] == 'stride %d' % stride(P, first, nblocks), lines[at]
        at += 1
        for ss in (stride(P, first, nblocks), 0):
            total = P + nblocks
            assert lines[at] == 'grid P=%d first=%d nblocks=%d s=%d positions=%d' % (P, first, nblocks, ss, total), lines[at]
            kind, index = lines[at + 1].split(), lines[at + 2].split()
            assert kind[0] == 'kind' and index[0] == 'index' and len(kind) == len(index) == total + 1
            got = [(int(a), int(b)) for a, b in zip(kind[1:], index[1:])]
            at += 3
            # the properties, on the program's own lines
            jobs = [(pos, i) for pos, (is_job, i) in enumerate(got) if is_job]
            owns = [i for is_job, i in got if not is_job]
            assert [i for _, i in jobs] == list(range(nblocks)), 'every job index once'
            assert [pos for pos, _ in jobs] == [first + i * (ss + 1) for i in range(nblocks)], 'job workgroup i at first + i (s + 1)'
            assert owns == list(range(P)), 'every own index once, ascending with the position'
            assert got == dealt(P, first, nblocks, ss), (P, first, nblocks, ss)
            if ss == 0:
                assert got == contiguous(P, first, nblocks), ('s = 0 is the contiguous layout', P, first, nblocks)
    assert at == len(lines)


def test_a_broken_request_is_refused(programs):
    res = subprocess.run([programs['plain']], input='grids 1 1 1 0\n', stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 2 and 'unknown request' in res.stdout


def test_stride_of_the_plan(programs):
    """dense_plan: the flagship (100000 x 10000: 10 panels x 196 row blocks of 512 rows, 1563 tiles on 64 job workgroups) deals with
    14 own workgroups between two of the job; RRI_EARLY_DEAL=0 leaves 0 and every other value of the plan as it was; a pass of one
    round (30011 x 2503: 471 workgroups) has the job last, stride 0; and the shapes of tests/test_early_deal_gpu.py at 256 CUs"""
    requests = [plan_line(100000, 10000, 50, 1), plan_line(100000, 10000, 50, 0), plan_line(30011, 2503, 4, 1)]
    want = ['plan P=1960 first=1024 e_blocks=64 e_tpb=25 e_stride=14', 'plan P=1960 first=1024 e_blocks=64 e_tpb=25 e_stride=0',
            'plan P=471 first=471 e_blocks=64 e_tpb=8 e_stride=0']
    for name in dg.DEAL_SHAPES:
        n, d, k, P, s = dg.deal_shape(name, 256)
        for deal in (1, 0):
            requests.append(plan_line(n, d, k, deal, pk_rows=16, pk_il=0))
            tiles = (n + 63) // 64
            e_blocks = min(tiles, 64)
            want.append('plan P=%d first=1024 e_blocks=%d e_tpb=%d e_stride=%d' % (P, e_blocks, -(-tiles // e_blocks), s if deal else 0))
    # the strides those shapes are there for, at 256 CUs: behind `first` fewer workgroups than the job's 64, as many, and 3 * 64 + 1
    assert [dg.deal_shape(name, 256)[3:] for name in ('less', 'equal', 'three-and-one')] == [(1024 + 63, 0), (1024 + 64, 1), (1024 + 193, 3)]
    for build in ('plain', 'sanitized'):
        assert run(programs[build], requests) == want
