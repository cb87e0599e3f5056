"""Frozen rows without a GPU: rri_frozen.hpp under the host compiler and sanitizers (the argument check, the addend's place, the
plain sweep against the numpy restatement of the stacked problem), the ABI surface and its documents, the refusals that need no
device, FrozenRows arithmetic, nmf(frozen=)'s refusals and partial_fit's plumbing behind a stand-in solver."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import frozen_cases as fc
from conftest import ROOT
from rri_nmf_amd import _capi
from rri_nmf_amd.engine import FrozenRows, RRIEngine


@pytest.fixture(scope='module')
def plain_output(tmp_path_factory):
    cxx = next((c for c in (os.environ.get('CXX'), 'c++', 'g++', 'clang++') if c and shutil.which(c)), None)
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('frozen') / 'frozen')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'rri_nmf_amd', 'csrc'),
                    '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'c', 'frozen_main.cpp'), '-o', exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-4000:]
    lines = res.stdout.strip().splitlines()
    assert lines[-1] == 'ok 6 cases', lines[-1]
    return lines


def test_the_argument_check_rule_by_rule(plain_output):
    got = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'chk (\w+) : (-?\d+) : (.*)$', ln) for ln in plain_output) if m}
    assert len(got) == 15
    for name in ('ok', 'A_symmetric_to_rounding', 'all_zero'):
        assert got[name] == (0, ''), (name, got[name])
    said = {'null_A': 'must all be given', 'null_s': 'must all be given', 'null_B': 'must all be given', 'k_zero': 'must be >= 1',
            'B_negative': r'B\[1, 1\] is negative', 'B_nan': r'B\[1, 2\] is negative or not finite', 'A_inf': r'A\[1, 1\]',
            'A_negative': r'A\[0, 0\] is negative', 'A_asymmetric': r'not symmetric at \[0, 1\]', 's_negative': r's\[1\]',
            'c_negative': 'c = ', 'c_nan': 'c = '}
    for name, text in said.items():
        assert got[name][0] == -1 and re.search(text, got[name][1]), (name, got[name])
    dec = {m.group(1): (int(m.group(2)), m.group(3)) for m in (re.match(r'decay (\w+) : (-?\d+) : (.*)$', ln) for ln in plain_output) if m}
    assert dec['one'] == (0, '') and dec['half'] == (0, '')
    for name in ('zero', 'negative', 'above', 'nan'):
        assert dec[name][0] == -1 and 'outside (0, 1]' in dec[name][1], (name, dec[name])


def test_the_addend_goes_to_the_columns_and_slice_zero_and_a_reset_clears_one_topic(plain_output):
    lay = next(ln for ln in plain_output if ln.startswith('layout ')).split()[1:]
    # red = [304 columns | slices of k + 2 = 19]: column 5; entries 0, k (||w||^2) and k + 1 (the column sum) of slice 0; the count
    assert [int(v) for v in lay] == [5, 304, 321, 322, 323]
    vec = lambda name: np.array(next(ln for ln in plain_output if ln.startswith(name + ' ')).split()[1:], dtype=np.float64)
    B, A, s = vec('clearB').reshape(3, 4), vec('clearA').reshape(3, 3), vec('clears')
    assert np.array_equal(B, [[1] * 4, [0] * 4, [1] * 4])
    assert np.array_equal(A, [[2, 0, 2], [0, 0, 0], [2, 0, 2]]) and np.array_equal(s, [3, 0, 3])


def _cases(lines):
    out, i = [], 0
    while i < len(lines):
        if not lines[i].startswith('case '):
            i += 1
            continue
        head = lines[i].split()
        c = dict(name=head[1], no=int(head[2]), nh=int(head[3]), d=int(head[4]), k=int(head[5]), sweeps=int(head[6]),
                 cleared=int(head[7]), project=int(head[8]), has_trs=int(head[9]), trs=float(head[10]),
                 regs=[float(v) for v in head[11:15]])
        for j in range(1, 13):
            parts = lines[i + j].split()
            c[parts[0]] = np.array(parts[1:], dtype=np.float64)
        out.append(c)
        i += 13
    return out


def test_the_plain_sweep_is_the_stacked_problem_with_the_frozen_rows_left_alone(plain_output):
    """frozen_sweep_plain, printed to 17 digits, against the numpy restatement of the STACKED problem after two sweeps.  The two
    differ in the order of sums of at most 20 non-negative terms (relative error 20 u = 4e-15 each) and in where the frozen rows
    enter; the numerators cancel by a factor of order 10 and 2 k <= 8 steps build on one another: 1e-12 leaves two decades."""
    cases = _cases(plain_output)
    assert [c['name'] for c in cases] == ['plain', 'plain_k1', 'simplex', 'penalties', 'cleared_topic', 'no_frozen_rows']
    for c in cases:
        no, nh, d, k = c['no'], c['nh'], c['d'], c['k']
        assert c['code'].tolist() == [0.0, -1.0], c['name']
        flags = dict(reg_w_l1=c['regs'][0], reg_w_l2=c['regs'][1], reg_t_l1=c['regs'][2], reg_t_l2=c['regs'][3])
        if c['project']:
            flags.update(project_T_each_iter=True, t_row_sum=c['trs'], w_row_sum=1.0)
        Wo = c['Wo'].reshape(no, k).copy()
        if c['cleared'] >= 0:
            Wo[:, c['cleared']] = 0.0
        st = fc.Stacked(c['Xo'].reshape(no, d), Wo, c['Xh'].reshape(nh, d), c['Wh0'].reshape(nh, k), c['T0'].reshape(k, d), **flags)
        # the sums the program took by plain loops are those of the (cleared) frozen rows
        B, A, s, cc = st.stats()
        assert np.allclose(c['B'].reshape(k, d), B, rtol=1e-14, atol=0) and np.allclose(c['A'].reshape(k, k), A, rtol=1e-14, atol=0)
        assert np.allclose(c['s'], s, rtol=1e-14, atol=0)
        W, T = st.sweep(c['sweeps'])
        assert st.resets == 0
        ew, et = fc.relfro(c['Wh'].reshape(nh, k), W), fc.relfro(c['T'].reshape(k, d), T)
        print('%s: W %.2e T %.2e' % (c['name'], ew, et))
        assert ew <= 1e-12 and et <= 1e-12, (c['name'], ew, et)
        # ... and the form from the statistics alone says the same
        W2, T2 = fc.frozen_sweep(B, A, s, c['Xh'].reshape(nh, d), c['Wh0'].reshape(nh, k), c['T0'].reshape(k, d), c['sweeps'], **flags)
        assert fc.relfro(W2, W) <= 1e-12 and fc.relfro(T2, T) <= 1e-12
        if c['project']:
            assert np.allclose(c['T'].reshape(k, d).sum(1), c['trs'], rtol=0, atol=1e-14)
        # the objective's share: the formula against 1/2 ||Xo - Wo T||^2, within a few ulp of the c it cancels against
        share, direct, csq = c['share']
        assert abs(share - direct) <= 1e-13 * max(0.5 * csq, 1.0), (c['name'], share, direct)
        assert abs(direct - 0.5 * float(((st.Xo - Wo.dot(c['T'].reshape(k, d))) ** 2).sum())) <= 1e-13 * max(0.5 * csq, 1.0)


# ---- the ABI surface ------------------------------------------------------------------------------------------------------
PROTOS = {
    'rri_frozen_set': 'rri_ctx* ctx, const double* B, const double* A, const double* s, double c',
    'rri_frozen_get': 'rri_ctx* ctx, double* B_out, double* A_out, double* s_out, double* c_out, int64_t* rows_out',
    'rri_frozen_absorb': 'rri_ctx* ctx, double decay',
}


def test_the_entry_points_are_declared_bound_and_documented():
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    assert re.search(r'#define RRI_ABI_VERSION 1\b', text) and _capi.ABI_VERSION == 1          # additions, not a new ABI
    for name, args in PROTOS.items():
        proto = re.search(r'^rri_status %s\(([^;]*)\);' % name, text, flags=re.M)
        assert proto and re.sub(r'\s+', ' ', proto.group(1)) == args, name
    D, P, I64 = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int64)
    assert _capi.PROTOTYPES['rri_frozen_set'] == (C.c_int32, [P, D, D, D, C.c_double])
    assert _capi.PROTOTYPES['rri_frozen_get'] == (C.c_int32, [P, D, D, D, D, I64])
    assert _capi.PROTOTYPES['rri_frozen_absorb'] == (C.c_int32, [P, C.c_double])
    assert re.search(r'\* 8 = the launches of rri_frozen_absorb', text)
    integ = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    readme = open(os.path.join(ROOT, 'README.md')).read()
    for name in PROTOS:
        assert name in integ, name
    assert 'RRI_TROW_SMALL' in integ
    assert re.search(r'^### 4\.11 ', design, flags=re.M) and 'k_wtx_panel' in design and 'frozen_sweep_plain' in design
    assert 'partial_fit' in readme and 'frozen' in readme
    # the semantics are written once, in a header the host compiler takes alone, and the kernels include it
    hpp = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_frozen.hpp')).read()
    assert 'hip_runtime' not in hpp and '__global__' not in hpp
    kern = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_frozen_kernels.hpp')).read()
    assert '#include "rri_frozen.hpp"' in kern and 'atomic' not in kern.replace('No atomics', '')
    for k in ('k_frozen_add', 'k_wtx_panel', 'k_panel_sum'):
        assert re.search(r'__global__[^;{]*\b%s\(' % k, kern), k
    assert '__builtin_amdgcn_mfma_f64_16x16x4f64' in kern


def test_a_null_handle_and_bad_arguments_answer_invalid_without_a_gpu():
    lib = _capi.load_library()
    D = C.POINTER(C.c_double)
    one = (C.c_double * 4)(1.0, 1.0, 1.0, 1.0)
    rows = C.c_int64(0)
    assert lib.rri_frozen_set(None, one, one, one, 1.0) == _capi.RRI_ERR_INVALID
    assert lib.rri_frozen_set(None, None, None, None, 0.0) == _capi.RRI_ERR_INVALID
    assert lib.rri_frozen_get(None, one, one, one, C.cast(one, D), C.byref(rows)) == _capi.RRI_ERR_INVALID
    assert lib.rri_frozen_absorb(None, 1.0) == _capi.RRI_ERR_INVALID
    assert lib.rri_frozen_absorb(None, float('nan')) == _capi.RRI_ERR_INVALID


def test_the_new_engine_methods_call_the_new_entry_points_only():
    src = open(os.path.join(ROOT, 'rri_nmf_amd', 'engine.py')).read()
    for meth in ('set_frozen', 'get_frozen', 'clear_frozen', 'absorb'):
        body = re.search(r'\n    def %s\(self.*?(?=\n    def |\Z)' % meth, src, flags=re.S).group(0)
        called = set(re.findall(r'_lib\.(rri_\w+)', body))
        assert called <= set(PROTOS), (meth, called)
        assert callable(getattr(RRIEngine, meth))
    # ... and none of the three needs an invalidation: their bodies in the library never call changed(
    hip = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_hip.hip')).read()
    for name in list(PROTOS) + ['frozen_absorb_panel', 'frozen_objective_add', 'frozen_alloc', 'frozen_release', 'frozen_clear_topic_dev']:
        m = re.search(r'^(?:static )?[\w:\*]+[\s\*]+%s\(.*?^}' % name, hip, flags=re.S | re.M)
        assert m and not re.search(r'\bchanged\(', m.group(0)), name


# ---- FrozenRows -----------------------------------------------------------------------------------------------------------
def test_frozen_rows_is_a_value_with_decay_and_sum():
    rs = np.random.RandomState(0)
    X1, W1, X2, W2 = rs.rand(7, 5), rs.rand(7, 3), rs.rand(4, 5), rs.rand(4, 3)
    f1, f2 = FrozenRows.of(X1, W1), FrozenRows.of(sp.csr_matrix(X2), W2)
    assert (f1.k, f1.d, f1.rows, f2.rows) == (3, 5, 7, 4)
    both = FrozenRows.of(np.vstack([X1, X2]), np.vstack([W1, W2]))
    tot = f1 + f2
    for a, b in ((tot.B, both.B), (tot.A, both.A), (tot.s, both.s), (tot.c, both.c)):
        assert np.allclose(a, b, rtol=1e-14, atol=0)
    assert tot.rows == 11 and np.array_equal(tot.A, tot.A.T)
    keep = f1.B.copy()
    h = f1.decay(0.5)
    assert np.array_equal(h.B, 0.5 * f1.B) and np.array_equal(h.A, 0.5 * f1.A) and np.array_equal(h.s, 0.5 * f1.s)
    assert h.c == 0.5 * f1.c and h.rows == 7 and np.array_equal(f1.B, keep)       # a value: the original is untouched
    assert np.array_equal(f1.decay(1.0).B, f1.B)
    z = FrozenRows.zeros(3, 5)
    assert np.array_equal((f1 + z).B, f1.B) and (f1 + z).rows == 7 and z.c == 0.0
    T = rs.rand(3, 5)
    assert f1.objective_share(T) == pytest.approx(0.5 * ((X1 - W1.dot(T)) ** 2).sum(), rel=1e-12)
    for bad in (0.0, -1.0, 1.5):
        with pytest.raises(ValueError, match='outside'):
            f1.decay(bad)
    with pytest.raises(ValueError, match='different shapes'):
        f1 + FrozenRows.zeros(2, 5)
    with pytest.raises(ValueError, match='must be'):
        FrozenRows(np.zeros((3, 5)), np.zeros((2, 2)), np.zeros(3), 0.0)
    with pytest.raises(TypeError):
        f1 + 1


# ---- nmf(frozen=) refuses before any device work ------------------------------------------------------------------------------
def test_nmf_refuses_the_combinations_that_frozen_rows_do_not_cover():
    from rri_nmf_amd.nmf import nmf
    rs = np.random.RandomState(0)
    X, W0, T0 = rs.rand(12, 8), rs.rand(12, 3), rs.rand(3, 8)
    F = FrozenRows.zeros(3, 8)
    base = dict(W_in=W0, T_in=T0, max_iter=1, frozen=F)
    for kw, said in ((dict(W_mat=np.ones((12, 8))), 'W_mat'), (dict(schedule='residual'), "schedule='residual'"),
                     (dict(dtype=np.float16), 'float16'), (dict(dtype=np.uint8), 'uint8'), (dict(fix_W=True), 'fix_W'),
                     (dict(w_row=np.ones((12, 1))), 'w_row'), (dict(early_stop=lambda *a: 0.0), 'early_stop'),
                     (dict(store_gradients=True), 'store_gradients'), (dict(eps_gauss_t=1.0, delta_gauss_t=0.1), 'Gaussian'),
                     (dict(group=object()), 'group='), (dict(uniform_rows=True, sparse_X=True), 'uniform_rows')):
        with pytest.raises(NotImplementedError, match=re.escape(said)):
            nmf(X, 3, **dict(base, **kw))
    with pytest.raises(ValueError, match='k = 2, d = 8'):
        nmf(X, 3, **dict(base, frozen=FrozenRows.zeros(2, 8)))
    with pytest.raises(ValueError, match='k = 3, d = 9'):
        nmf(X, 3, **dict(base, frozen=FrozenRows.zeros(3, 9)))
    with pytest.raises(ValueError, match='FrozenRows, True'):
        nmf(X, 3, **dict(base, frozen=(1, 2)))
    import inspect
    sig = inspect.signature(nmf)
    assert sig.parameters['frozen'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['frozen'].default is None
    names = list(sig.parameters)
    assert names.index('frozen') == names.index('resident') + 1


# ---- partial_fit behind a stand-in solver ---------------------------------------------------------------------------------------
def test_partial_fit_initialises_folds_in_sweeps_with_the_frozen_rows_and_keeps_the_last_W(monkeypatch):
    from rri_nmf_amd import sklearn_interface as si
    calls = []

    def fake_nmf(X, k, **kw):
        calls.append(dict(kw, X=X, k=k))
        n, d = X.shape
        W = np.full((n, k), float(len(calls)))
        T = np.full((k, d), 1.0 / d) if kw.get('fix_T') is None else kw['T_in']
        out = {'W': W, 'T': T, 'iter_cputime': [0.0], 'idf': np.arange(1, d + 1, dtype=np.float64)}
        if kw.get('frozen') is not None:
            prev = FrozenRows.zeros(k, d) if kw['frozen'] is True else kw['frozen']
            out['frozen'] = prev + FrozenRows(np.ones((k, d)), np.eye(k), np.ones(k), 1.0, n)
        return out

    monkeypatch.setattr(si, '_nmf', fake_nmf)
    E = si.NMF_TM_Estimator(10, 6, 2, wr1=0.1, tr2=0.2, handle_tfidf=True, nmf_kwargs={'dtype': np.float64})
    X1, X2 = np.ones((10, 6)), 2 * np.ones((4, 6))
    assert E.partial_fit(X1, sweeps=5) is E
    first = calls[0]
    # the first call is fit's call with max_iter = sweeps, plus "absorb this batch, nothing frozen yet"
    assert first['frozen'] is True and first['max_iter'] == 5 and first['X'] is X1 and first['dtype'] == np.float64
    assert first['project_T_each_iter'] is True and first['t_row_sum'] == 1.0 and first['w_row_sum'] == 1.0
    assert first['reg_w_l1'] == 0.1 and first['reg_t_l2'] == 0.2 and first['preprocess'] == {'tfidf': True, 'normalize': False}
    assert first['W_in'] == [] and first['T_in'] == []
    assert E.frozen_.rows == 10 and np.array_equal(E.idf, np.arange(1, 7))
    E.partial_fit(X2, sweeps=3, decay=0.5)
    fold, step = calls[1], calls[2]
    assert len(calls) == 3
    assert fold['fix_T'] is True and fold['max_iter'] == 4 and fold['X'] is X2 and fold.get('frozen') is None        # transform's flags
    assert np.array_equal(fold['preprocess']['tfidf'], np.arange(1, 7))                    # the idf of the first batch
    assert step['max_iter'] == 3 and step['X'] is X2 and np.array_equal(step['W_in'], np.full((4, 2), 2.0))
    assert np.array_equal(step['preprocess']['tfidf'], np.arange(1, 7))
    assert isinstance(step['frozen'], FrozenRows) and np.array_equal(step['frozen'].B, 0.5 * np.ones((2, 6))) and step['frozen'].rows == 10
    assert E.frozen_.rows == 14 and np.array_equal(E.frozen_.B, 1.5 * np.ones((2, 6))) and E.frozen_.c == 1.5
    assert E.W.shape == (4, 2) and np.array_equal(E.W, np.full((4, 2), 3.0))                # W of the last batch
    assert 'frozen' not in E.nmf_outputs
    for bad in (dict(sweeps=0), dict(decay=0.0), dict(decay=1.5)):
        with pytest.raises(ValueError):
            E.partial_fit(X2, **bad)
    assert len(calls) == 3
