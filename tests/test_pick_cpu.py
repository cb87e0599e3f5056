"""The helper that turns run-time values into template arguments (rri_nmf_amd/csrc/rri_pick.hpp), on the CPU.

tests/c/pick_main.cpp is a stand-alone program with its own main that includes only that header and include/rri_hip.h (the
dtype codes).  It is built with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once.  Checked:
  * pick_int reaches the listed constant equal to the value, and the LAST listed one for any other value (the `default:` of the
    switches it replaces: 16 for the residual's rank buckets, 64 for the lanes per segment of k_sp_blk);
  * pick_bool and pick_type do the same over their domains; pick_type over a list without the half type never reaches it (a
    static_assert in the program), whatever the code;
  * the callable runs exactly once per pick, and what it returns comes back (a value, a reference, nothing);
  * a nest of three picks driven over all inputs visits each point of the cross product exactly once;
  * a nest shaped like the residual's (masked x write_e x rank bucket x row sums) with its `if constexpr` prune reaches exactly the
    30 instantiations that exist, out of the 40 of the cross product: the stand-in kernel template refuses to compile for the rest."""
import itertools
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RRI_F32, RRI_F64, RRI_F16 = 0, 1, 2        # include/rri_hip.h


def pick_int(listed, v):
    return v if v in listed else listed[-1]


def test_every_pick_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'pick')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'pick_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok', lines[-1]
    by_kind = {}
    for ln in lines[:-1]:
        by_kind.setdefault(ln.split()[0], []).append(ln)

    want = ['int5 %d -> %d calls 1' % (v, 3 * pick_int((4, 8, 12, 13, 16), v))
            for v in (-2 ** 31, -1, 0, 4, 5, 8, 12, 13, 14, 16, 17, 2 ** 31 - 1)]
    assert by_kind.pop('int5') == want
    assert by_kind.pop('int4') == ['int4 %d -> %d calls 1' % (v, pick_int((8, 16, 32, 64), v)) for v in (8, 16, 32, 64, 7, 0, 128)]
    assert by_kind.pop('int1') == ['int1 3 -> 7 calls 1']
    assert by_kind.pop('bool') == ['bool 0 -> 0 calls 1', 'bool 1 -> 1 calls 1']

    names = {RRI_F32: 'float', RRI_F64: 'double', RRI_F16: 'half'}
    want = []
    for code in (RRI_F32, RRI_F64, RRI_F16, -1, 3):
        want.append('type %d -> %s %s %s calls 3' % (code, names.get(code, 'half'), names[code] if code in (RRI_F32, RRI_F64) else 'double',
                                                     names[code] if code in (RRI_F32, RRI_F64) else 'float'))
    assert by_kind.pop('type') == want

    assert by_kind.pop('ref') == ['ref 2 7 1']
    assert by_kind.pop('nest') == ['nest %d %d -> 1 1' % (b, v) for b in (0, 1) for v in (0, 1, 2)]

    reached = set()
    site = by_kind.pop('site')
    assert len(site) == 40
    for ln, (masked, write_e, ks, sums) in zip(site, itertools.product((0, 1), (0, 1), (4, 8, 12, 13, 16), (0, 1))):
        sm = 1 if (sums or not write_e) else 0
        assert ln == 'site %d %d %d %d -> %d calls 1' % (masked, write_e, ks, sums, 1000 * masked + 100 * write_e + 10 * sm + ks), ln
        reached.add((masked, write_e, ks, sm))
    assert reached == {p for p in itertools.product((0, 1), (0, 1), (4, 8, 12, 13, 16), (0, 1)) if p[3] or p[1]}
    assert len(reached) == 30
    assert not by_kind, sorted(by_kind)
