"""The halting rules every kernel calls (rri_nmf_amd/csrc/rri_halt.hpp), on the CPU.

tests/c/halt_rules_main.cpp is a stand-alone program with its own main that includes only that header.  It is built with the
host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and run once.  It prints one line per case of the full cross
product of
    sum / denominator   NaN, -1, -0.0, 0.0, 5e-324, 1e-10, nextafter(1e-10, 1), 1.0, inf
    reset_method {0, 1, 2}   resets_left {0, 1, 3}   negflag {0, 1}   has_wrs {0, 1}   w_row_sum {0, 1}
    project_T {0, 1}   has_trs {0, 1}   t_row_sum {0, 1, 2}
with the verdict of every rule, then next_step at t = 0, k - 2, k - 1 and k = 1, and checks halt_set on a DevState on its stack
(four fields written, every other byte untouched).  Every line is compared here with a restatement of the reference's rules,
written beside the lines of the reference (nmf.py, optimization.py) and of oracle/rri_oracle.py they restate.

Two inputs on which the device has always parted from the reference are asserted as they behave:
  * a NaN column sum with a reset method and resets left: the reference resets (`nw1 > 1e-10` is false, nmf.py:794), the device
    reports HALT_ERR_W_COL_ZERO (its test is `sum <= 1e-10`, false for NaN, and the assertion of nmf.py:476 then fails);
  * a NaN scalar denominator: the reference takes neither `c > 0` nor `c <= 0` (optimization.py:53, 60) and fails on an unbound
    name; the device takes the `c <= 0` side (its test is `!(c > 0)`)."""
import itertools
import math
import os
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESET_T, RESET_W = 1, 2
UNBOUNDED, W_COL_ZERO, NOT_IMPLEMENTED = -4, -5, -6

VALUES = [float('nan'), -1.0, -0.0, 0.0, 5e-324, 1e-10, math.nextafter(1e-10, 1.0), 1.0, float('inf')]


def wcol_code(v, method, left):
    if v > 1e-10 or method == 0:            # nmf.py:794-795; oracle/rri_oracle.py:322-323
        pass
    elif left == 0:                         # nmf.py:797-800; oracle/rri_oracle.py:324-325
        pass
    elif not math.isnan(v):                 # nmf.py:801-816; oracle/rri_oracle.py:326-328  (NaN: see the docstring)
        return RESET_W
    return 0 if v > 0 else W_COL_ZERO       # nmf.py:476  assert np.sum(W[:, t]) > 0


def wwcol_code(v, negflag, has_wrs, method, left):
    if negflag > 0 and not has_wrs:         # optimization.py:76-77 with s = None, ub = w_row_sum (nmf.py:469)
        return UNBOUNDED
    return wcol_code(v, method, left)


def trow_kept(v, method):
    return v > 1e-10 or method == 0         # nmf.py:758; oracle/rri_oracle.py:311


def trow_resets(v, method, left):
    if trow_kept(v, method):
        return False
    return left != 0                        # nmf.py:765-769; oracle/rri_oracle.py:315-319


def scalar_qf_min_mode(c, s, ub):
    """optimization.py:53-73: which branch a scalar c takes."""
    if c > 0:                               # :53
        return 0
    if s is None:                           # :60-62  (NaN: see the docstring)
        return 1 if ub else UNBOUNDED       # :64-67
    if s == 1.0:                            # :68-70
        return 2
    return NOT_IMPLEMENTED                  # :71-73


def trow_denominator_mode(c, project_T, has_trs, t_row_sum):
    trs = float(t_row_sum) if has_trs else None
    s = trs if project_T else None          # nmf.py:447: s = t_row_sum where the row is projected in every iteration
    return scalar_qf_min_mode(c, s, trs)


def wcol_denominator_mode(c, has_wrs, w_row_sum):
    return scalar_qf_min_mode(c, None, float(w_row_sum) if has_wrs else None)      # nmf.py:469: s = None, ub = w_row_sum


def next_step(sweep, t, k):
    return (sweep + 1, 0) if t + 1 == k else (sweep, t + 1)     # the loop of nmf.py:415: topic t + 1, or topic 0 of the next sweep


def test_every_rule_over_the_cross_product_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'halt_rules')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'halt_rules_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok 7776 cases', lines[-1]

    # the program's inputs are the ones named above, bit for bit
    got_values = [ln.split() for ln in lines if ln.startswith('value ')]
    assert len(got_values) == len(VALUES)
    for (_, i, bits), v in zip(got_values, VALUES):
        dev = struct.unpack('<d', struct.pack('<Q', int(bits, 16)))[0]
        assert (math.isnan(dev) and math.isnan(v)) or struct.pack('<d', dev) == struct.pack('<d', v), (i, bits, v)

    seen = set()
    for ln in lines:
        if not ln.startswith('case '):
            continue
        key_s, got_s = ln[5:].split(' : ')
        key = tuple(int(x) for x in key_s.split())
        vi, method, left, negflag, has_wrs, wrs, project_T, has_trs, trs = key
        v = VALUES[vi]
        want = (wcol_code(v, method, left), wwcol_code(v, negflag, has_wrs, method, left), int(trow_kept(v, method)),
                int(trow_resets(v, method, left)), trow_denominator_mode(v, project_T, has_trs, trs),
                wcol_denominator_mode(v, has_wrs, wrs))
        assert tuple(int(x) for x in got_s.split()) == want, ln
        seen.add(key)
    assert seen == set(itertools.product(range(9), (0, 1, 2), (0, 1, 3), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2)))

    # the NaN column with resets left, as it behaves today
    assert wcol_code(float('nan'), 1, 3) == W_COL_ZERO and wcol_code(0.0, 1, 3) == RESET_W and wcol_code(0.0, 1, 0) == W_COL_ZERO

    steps = [ln for ln in lines if ln.startswith('next ')]
    want_steps = [(4, 0, 5), (4, 3, 5), (4, 4, 5), (0, 0, 2), (0, 1, 2), (4, 0, 1), (0, 0, 1)]    # t = 0, k - 2, k - 1; k = 1
    assert len(steps) == len(want_steps)
    for ln, (sweep, t, k) in zip(steps, want_steps):
        assert ln == 'next %d %d %d : %d %d' % ((sweep, t, k) + next_step(sweep, t, k)), ln
