"""The codec of the packed 28-bit copy of an fp32 X (rri_nmf_amd/csrc/rri_xpack.hpp), on the CPU.

tests/c/xpack_codec_main.cpp is a stand-alone program with its own main that includes the header the kernels include.  It is built
with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once.  It checks, for every top byte 0..255
and every base in {1, 50, 113, 240}, with the low parts {0, 1, 0x7fffff, 0x800000, 0xffffff} plus a seeded sample, that
decode(encode(b)) == b exactly when b is in the window and that b is flagged otherwise -- element by element and through the
whole-lane encoder and the row decoder the kernels use -- and that the record offsets of (q, p, lane, u, e) are a bijection onto
the 7 KiB of a record."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_codec_round_trip_and_record_bijection_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'xpack_codec')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'xpack_codec_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().splitlines()[-1].startswith('ok '), res.stdout
