"""The codec of the 26-bit copy of an fp32 X (rri_nmf_amd/csrc/rri_xnarrow.hpp), on the CPU.

tests/c/xnarrow_codec_main.cpp is a stand-alone program with its own main that includes the header the kernels include.  It is
built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once.  Through the lane encoder, the
exception map and the row decoder the kernels call, it checks: for every exponent byte and books that hold it in the 7-entry book,
only in the rare book, or nowhere, with the mantissas {0, 1, 0x3fffff, 0x400000, 0x7fffff} and a seeded sample, that a record
decodes to its bits exactly and that an element in neither book is reported for flagging; records with 0, 1, 63, 64, 65 and 2048
exceptions, at positions 0 and 2047; padding rows; the books chosen from a histogram with ties; directory offsets up to and past
2^32 entries; and that the lane offsets and bit places of the fixed part are a bijection onto the 6.5 KiB of a record."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_codec_round_trip_exceptions_books_and_directory_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'xnarrow_codec')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'xnarrow_codec_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().splitlines()[-1].startswith('ok '), res.stdout
