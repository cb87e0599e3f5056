"""The blocked CSR store (pattern-only weighted handles, X kept as CSR) and the dense weighted one-pass step, topic step by
topic step against float64 numpy, at the sizes where the host code picks another layout or route.

The split step.  Before every topic step of two sweeps the factors are downloaded and the device's sums of the T-row step
(rri_topic_reduce_local: wR = a + t .* nw and nw) are compared element by element with the float64 sums of those factors;
after the step the new W column is compared with the closed form on the float64 sums, and every other row and column must be
bit-equal.  The new T row is compared here with the closed form on the sums the device itself took, to 1e-12 of the row's
norm and 1e-11 of its largest entry: that checks the solve on its own, and with wR and nw bounded just before it bounds the
row -- but an entry whose nw_j is tiny is then held only relative to the row's maximum.  The rebuild of the stored residual
before topic 0 of every sweep and the carry across it are inside the checked range.

sweep().  What only rri_sweep reaches (the fused T-row launch k_wtrow_small, taken while the handle has at most 64 row blocks)
is checked step by step too: a sweep rewrites row t of T and column t of W in step t alone, so every intermediate state
follows from the factors before and after the sweep, and replay_weighted_sweep holds every T row (float64 sums, their bounds
carried through the division: an entry with a tiny nw_j gets the large bound it deserves) and every W column of two sweeps
inside the same derived bounds, element by element.  Where the handle reports that sweep() and the split step take the same
route (nrb = 65, the 36100-row shapes) their results must be the same bits.  The whole-matrix yardstick of test_fuzz_gpu.py
is used for the comparison with the oracle's sweep and for nothing else.  X kept as CSR (unweighted, no stored state) goes
through update_T_row / update_W_col and check_steps of test_kernel_buckets_gpu, and through the same replay of sweep() with
check_steps' tolerances.

Bounds are derived in tests/wsb_cases.py (StepBound): a matrix B >= |E_device - E_true| carried alongside the reference, one
unit roundoff of the storage type per stored correction (and two per product of table-rounded factors on fp32 pattern-only
handles), plus the float64 forward bound C64 (terms + k + 2) 2^-53 of the sums, C64 = 2, times one safety factor 2.  Nothing
in a bound comes from a device result.  tests/test_weighted_sparse_layout_cpu.py checks on the CPU that an emulation of
the stored residual stays inside these bounds on the cases of this module and that single dropped entries, pads read as data,
skipped corrections and dropped blocks fall outside them, and says what the bounds cannot see.

Which bucket ran.  Every case asserts that the layout and routes the handle reports (rri_layout_info) are the restated ones
and the ones its id names; the restated work-item count uses the number of compute units the handle reports.
RRI_TEST_RATIOS=1 prints the worst error / bound per case (not asserted).

Measured on an MI355X (358 cases, 24 s).  Worst error / bound, fp32 / float64 storage -- split step: 0.48 / 0.18 pattern-only,
0.31 / 0.11 dense weighted; sweep() replayed: 0.27 / 0.10 pattern-only, 0.31 / 0.03 dense weighted.  The CPU emulation of the
same cases gives 0.48 / 0.12 pattern-only and 0.34 / 0.04 dense, case by case the device's figure where the two were compared
(bw=cap-csr, fp32: 0.462 both): the cases near 0.5 have columns of one or two entries, where the table rounding of w in
nw = w^2 attains its worst case 2 u against the bound 2 * 2 u; long columns sit at 0.01 - 0.1.
"""
import os

import numpy as np
import pytest

import wsb_cases as wc
from rri_nmf_amd.synthetic import scaled_init
from test_kernel_buckets_gpu import FLAGS, U, assert_elementwise, assert_rel, check_steps, engine, oracle, stored

pytestmark = pytest.mark.gpu

EPS = float(np.spacing(10))
STEP_FLAGS = wc.STEP_FLAGS
assert STEP_FLAGS['topic'] == FLAGS['topic'] and STEP_FLAGS['plain'] == FLAGS['plain']


def report(what, ratio):
    if os.environ.get('RRI_TEST_RATIOS', '0') == '1':
        print('\nRATIO %-60s %.3g' % (what, ratio))


def ratio_of(got, want, bound):
    err = np.abs(np.asarray(got) - np.asarray(want))
    ok = np.asarray(bound) > 0
    return float((err[ok] / np.asarray(bound)[ok]).max()) if ok.any() else 0.0


def assert_layout_reported(e, name, A, store, csrx):
    """the handle reports the restated layout (with the device's own number of compute units), and that layout is the bucket
    the case is named for"""
    info = e.layout_info()
    L = wc.sp_layout(A, store, csrx, info['n_cu'])
    wc.bucket_claims(name, L, store, csrx)
    for w, copy in enumerate(('row copy', 'column copy')):
        got = {f: info[f][w] for f in ('nblk', 'bw', 'lps', 'nwork')}
        want = {f: L[w][f] for f in ('nblk', 'bw', 'lps', 'nwork')}
        assert got == want, 'the %s reports %r, the restated build_sp_store gives %r' % (copy, got, want)
    return info


def drive_weighted_steps(e, sb, k, flags, sweeps, what):
    """`sweeps` sweeps through the split step with the checks of the module docstring; returns the worst error / bound"""
    orc = oracle()
    n, d = sb.X.shape
    ld = -(-d // (16 // e.dtype.itemsize)) * (16 // e.dtype.itemsize)
    regs = [flags.get(r, 0.0) for r in ('reg_w_l1', 'reg_w_l2', 'reg_t_l1', 'reg_t_l2')]
    no_regs = sum(abs(r) for r in regs) == 0
    fix_W = bool(flags.get('fix_W'))
    s = flags.get('t_row_sum') if flags.get('project_T_each_iter') else None
    worst = 0.0
    for sweep in range(sweeps):
        for t in range(k):
            where = '%s, sweep %d topic %d' % (what, sweep, t)
            e.topic_reduce_local(t)
            e.topic_finish(-1)
            assert e._stepping_event() is None, where
            W0, T0 = e.get_W(), e.get_T()
            if t == 0:
                sb.rebuild(W0, T0)              # the device rebuilds E before topic 0 of every sweep
            _, wR, nw, _ = e._topic_sums(t, ld)
            wR, nw = np.array(wR), np.array(nw)
            want_wR, want_nw, b_wR, b_nw = sb.T_sums(W0, T0, t)
            worst = max(worst, ratio_of(wR, want_wR, b_wR), ratio_of(nw, want_nw, b_nw))
            assert_elementwise(nw[None, :], want_nw[None, :], b_nw[None, :], 'nw = (w^2)^T M, ' + where, cols_are='columns')
            assert_elementwise(wR[None, :], want_wR[None, :], b_wR[None, :], 'wR = w^T (M .* R_t), ' + where, cols_are='columns')
            e.topic_finish(t)
            assert e._stepping_event() is None, where
            W1, T1 = e.get_W(), e.get_T()
            others = np.arange(k) != t
            # the T row: the closed form on the sums the device took
            want, nt1 = orc.qf_min(-(wR - regs[2]), nw + regs[3], s=s, ub=flags.get('t_row_sum'))
            assert np.linalg.norm(T1[t] - want) <= 1e-12 * np.linalg.norm(want), ('T row', where, np.linalg.norm(T1[t] - want))
            assert_elementwise(T1[t][None, :], want[None, :], 1e-11 * np.abs(want).max(), 'T row, ' + where, cols_are='columns')
            assert np.array_equal(T1[others], T0[others]), 'other rows of T changed, ' + where
            assert np.array_equal(W1[:, others], W0[:, others]), 'other columns of W changed, ' + where
            scale = nt1 if (fix_W and no_regs) else 1.0          # nmf.py:450-452; with a W half behind it the scale cancels
            Wm = W0.copy()
            Wm[:, t] *= scale
            sb.correct(W0[:, t], scale * T1[t] - T0[t], Wm, T1)
            if fix_W:
                # w * sum(T row): two sums of d non-negative terms in different orders, one product each
                assert_elementwise(W1[:, t][:, None], Wm[:, t][:, None], 2 * (d + 2) * U * np.abs(Wm[:, t][:, None]),
                                   'kept W column rescaled, ' + where)
                continue
            x, bx = sb.W_column(Wm, T1, t, regs[0], regs[1], flags.get('w_row_sum'), EPS)
            worst = max(worst, ratio_of(W1[:, t], x, bx))
            assert_elementwise(W1[:, t][:, None], x[:, None], bx[:, None], 'W column, ' + where, cols_are='column')
            sb.correct(W1[:, t] - Wm[:, t], T1[t], W1, T1)
    return worst


def yardstick(Xs, M, k, W0, T0, kw, store):
    """tests/test_fuzz_gpu.py: the oracle's sweep, and how far it moves when its start is perturbed by one ulp"""
    from conftest import relfro
    orc = oracle()
    kw = dict(kw, do_final_project_W=False)
    ref = orc.nmf(Xs, k, W_mat=M, W_in=W0.copy(), T_in=T0.copy(), max_iter=1, eps_stop=-1, **kw)
    Wp = W0 * (1.0 + 2.0 ** -52 * np.sign(np.random.RandomState(7).randn(*W0.shape)))
    per = orc.nmf(Xs, k, W_mat=M, W_in=Wp, T_in=T0.copy(), max_iter=1, eps_stop=-1, **kw)
    base = 1e-7 if (store == 'fp64' or M is None) else 5e-3
    return ref, max(base, 30.0 * max(relfro(per['W'], ref['W']), relfro(per['T'], ref['T'])))


def replay_weighted_sweep(sb, W0, T0, W1, T1, flags, what):
    """One whole sweep taken by rri_sweep, checked step by step although only its start (W0, T0) and its end (W1, T1) are
    known: a sweep rewrites row t of T and column t of W in step t and nowhere else, so the factors before step t are
    [W1[:, :t] | W0[:, t:]] and [T1[:t] ; T0[t:]].  For every step the new T row against the closed form on the float64 sums
    of that state (StepBound.T_row: the bounds of wR and nw carried through the division), then the new W column
    (StepBound.W_column), element by element, with the bound matrix carried along as in the split step.  Returns the worst
    error / bound."""
    k = W0.shape[1]
    d = T0.shape[1]
    regs = [flags.get(r, 0.0) for r in ('reg_w_l1', 'reg_w_l2', 'reg_t_l1', 'reg_t_l2')]
    no_regs = sum(abs(r) for r in regs) == 0
    fix_W = bool(flags.get('fix_W'))
    s = flags.get('t_row_sum') if flags.get('project_T_each_iter') else None
    sb.rebuild(W0, T0)
    worst = 0.0
    for t in range(k):
        where = '%s, sweep() topic %d' % (what, t)
        Wb, Tb = np.hstack([W1[:, :t], W0[:, t:]]), np.vstack([T1[:t], T0[t:]])
        wR, nw, b_wR, b_nw = sb.T_sums(Wb, Tb, t)
        want, bT, nx = sb.T_row(wR, nw, b_wR, b_nw, regs[2], regs[3], s, flags.get('t_row_sum'), EPS)
        worst = max(worst, ratio_of(T1[t], want, bT))
        assert_elementwise(T1[t][None, :], want[None, :], bT[None, :], 'T row, ' + where, cols_are='columns')
        Ta = Tb.copy()
        Ta[t] = T1[t]
        scale = nx if (fix_W and no_regs) else 1.0
        Wm = Wb.copy()
        Wm[:, t] *= scale
        sb.correct(Wb[:, t], scale * T1[t] - Tb[t], Wm, Ta)
        if fix_W:       # w * sum(x): the sum carries the bounds of the row before any scaling, and two roundings of d terms
            dsum = float(sb.T_row(wR, nw, b_wR, b_nw, regs[2], regs[3], None, flags.get('t_row_sum'), EPS)[1].sum())
            assert_elementwise(W1[:, t][:, None], Wm[:, t][:, None], (dsum + 2 * (d + 2) * U * nx) * np.abs(Wb[:, t][:, None]),
                               'kept W column rescaled, ' + where)
            continue
        x, bx = sb.W_column(Wm, Ta, t, regs[0], regs[1], flags.get('w_row_sum'), EPS)
        worst = max(worst, ratio_of(W1[:, t], x, bx))
        assert_elementwise(W1[:, t][:, None], x[:, None], bx[:, None], 'W column, ' + where, cols_are='column')
        Wa = Wm.copy()
        Wa[:, t] = W1[:, t]
        sb.correct(W1[:, t] - Wm[:, t], T1[t], Wa, Ta)
    return worst


def assert_whole_sweeps(make_engine, make_bound, stepwise, Xs, M, k, W0, T0, kw, store, what):
    """rri_sweep -- the fused T-row launch where the handle takes it -- twice, one sweep per call.  Each sweep is replayed step
    by step inside the derived bounds (replay_weighted_sweep); where the handle says that sweep() and the split step take the
    same route (no fused T-row launch) the first sweep must equal the stepwise run bit for bit; the oracle's sweep is compared
    under the yardstick of test_fuzz_gpu.py, which is kept for the oracle alone.  Returns the worst error / bound."""
    from conftest import relfro
    worst = 0.0
    with make_engine() as e:
        e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        Wa, Ta = W0, T0
        for sweep in range(2):
            e.sweep(1)
            Wb, Tb = e.get_W(), e.get_T()
            worst = max(worst, replay_weighted_sweep(make_bound(), Wa, Ta, Wb, Tb, kw, '%s, sweep %d' % (what, sweep)))
            if sweep == 0:
                W, T = Wb, Tb
            Wa, Ta = Wb, Tb
        same_route = not e.layout_info()['wtrow_small']
    if same_route:
        assert np.array_equal(T, stepwise[1]), '%s: sweep(1) and the split step take the same kernels, T differs in rows %s' % (
            what, np.flatnonzero(np.any(T != stepwise[1], axis=1)))
        assert np.array_equal(W, stepwise[0]), '%s: sweep(1) and the split step take the same kernels, W differs in columns %s' % (
            what, np.flatnonzero(np.any(W != stepwise[0], axis=0)))
    ref, tol = yardstick(Xs, M, k, W0, T0, kw, store)
    ew, et = relfro(W, ref['W']), relfro(T, ref['T'])
    assert ew < tol and et < tol, '%s: sweep(1) against the oracle: W %.3g T %.3g, yardstick %.3g' % (what, ew, et, tol)
    return worst


def replay_plain_sweep(Xs, W0, T0, W1, T1, what, tol=1e-12):
    """the same reconstruction for an unweighted handle (no stored state): every step of the sweep against the closed form,
    with the tolerances of check_steps"""
    from test_kernel_buckets_gpu import step_T_want, step_W_want
    k = W0.shape[1]
    for t in range(k):
        Wb, Tb = np.hstack([W1[:, :t], W0[:, t:]]), np.vstack([T1[:t], T0[t:]])
        want = step_T_want(Xs, Wb, Tb, t, {})
        assert np.linalg.norm(T1[t] - want) <= tol * np.linalg.norm(want), ('T row', what, t, np.linalg.norm(T1[t] - want) / np.linalg.norm(want))
        assert_elementwise(T1[t][None, :], want[None, :], 10 * tol * np.abs(want).max(), '%s, sweep() T row %d' % (what, t), cols_are='columns')
        Ta = Tb.copy()
        Ta[t] = T1[t]
        want = step_W_want(Xs, Wb, Ta, t, {})
        assert np.linalg.norm(W1[:, t] - want) <= tol * np.linalg.norm(want), ('W column', what, t, np.linalg.norm(W1[:, t] - want) / np.linalg.norm(want))
        assert_elementwise(W1[:, t][:, None], want[:, None], 10 * tol * np.abs(want).max(), '%s, sweep() W column %d' % (what, t), cols_are='column')


# ---- 1. the blocked store ---------------------------------------------------------------------------------------------
RUNS = wc.blocked_runs()
PAT_RUNS = [r for r in RUNS if r[3] == 'pat']
CSRX_RUNS = [r for r in RUNS if r[3] == 'csrx']


def pattern_engine(A, k, store):
    e = engine(A.shape[0], A.shape[1], k, dtype=wc.STORES[store], weighted='sparse')
    e.upload_observed_csr(A)
    return e


def csrx_engine(A, k, store):
    e = engine(A.shape[0], A.shape[1], k, dtype=wc.STORES[store], sparse_x=True)
    e.upload_X_csr(A)
    return e


@pytest.mark.parametrize('run', PAT_RUNS, ids=[wc.run_id(r) for r in PAT_RUNS])
def test_pattern_only_topic_steps(run):
    """weighted='sparse': k_sp_blk in every lane count, block width and segment length of the list, k_sp_resid at the rebuilds,
    k_wreduce / k_wtrow / k_wwcol on the per-block partial sums"""
    name, make, k, _, store = run
    A = make()
    n, d = A.shape
    A, W0, T0 = wc.planted(A, k)
    Xs, M = wc.pattern_problem(A, store)
    kw = dict(reset_topic_method=None)
    with pattern_engine(A, k, store) as e:
        assert_layout_reported(e, name, A, store, False)
        e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        sb = wc.StepBound(Xs, M, store, tables=True)
        worst = drive_weighted_steps(e, sb, k, kw, 2, wc.run_id(run))
    report('pattern-only steps ' + wc.run_id(run), worst)
    with pattern_engine(A, k, store) as e:
        e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        e.sweep_stepwise()
        stepwise = e.get_W(), e.get_T()
    worst = assert_whole_sweeps(lambda: pattern_engine(A, k, store), lambda: wc.StepBound(Xs, M, store, tables=True), stepwise,
                                Xs, M, k, W0, T0, kw, store, wc.run_id(run))
    report('pattern-only sweep() ' + wc.run_id(run), worst)


@pytest.mark.parametrize('run', CSRX_RUNS, ids=[wc.run_id(r) for r in CSRX_RUNS])
def test_csr_x_topic_steps(run):
    """sparse_x=True (k_spx_pass over both copies): half steps against the closed form, check_steps as it stands, twice"""
    name, make, k, _, store = run
    A = make()
    n, d = A.shape
    A, W0, T0 = wc.planted(A, k)
    Xs, _ = wc.pattern_problem(A, store)
    if k <= 8:                                     # unweighted: the zeros outside the pattern are data, W* T* is no solution
        W0, T0 = scaled_init(Xs, k, seed=k + 1)
    kw = dict(reset_topic_method=None)
    with csrx_engine(A, k, store) as e:
        assert_layout_reported(e, name, A, store, True)
        e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        for _ in range(2):
            check_steps(e, Xs, k, {})
    # rri_sweep: every step of two sweeps against the closed form (replay_plain_sweep), the first against the oracle
    with csrx_engine(A, k, store) as e:
        e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        e.sweep(1)
        W1, T1 = e.get_W(), e.get_T()
        e.sweep(1)
        W2, T2 = e.get_W(), e.get_T()
    replay_plain_sweep(Xs, W0, T0, W1, T1, wc.run_id(run) + ', sweep 0')
    replay_plain_sweep(Xs, W1, T1, W2, T2, wc.run_id(run) + ', sweep 1')
    from conftest import relfro
    ref, tol = yardstick(Xs, None, k, W0, T0, kw, store)
    ew, et = relfro(W1, ref['W']), relfro(T1, ref['T'])
    assert ew < tol and et < tol, '%s: sweep(1) against the oracle: W %.3g T %.3g, yardstick %.3g' % (wc.run_id(run), ew, et, tol)


@pytest.mark.parametrize('run', RUNS, ids=[wc.run_id(r) for r in RUNS])
def test_blocked_store_objective_rows_and_products(run):
    """rri_objective / rri_objective_parts, rri_resid_row_argmax / rri_reset_row (k_sp_resid) and rri_X_times / rri_Xt_times
    (k_sp_spmm over the blocks of both copies) on the same patterns, element by element against float64"""
    name, make, k, flavour, store = run
    A = make()
    n, d = A.shape
    csrx = flavour == 'csrx'
    A, W0, T0 = wc.planted(A, k)
    W0 = 0.96 * W0                                 # residuals of either sign
    Xs, M = wc.pattern_problem(A, store)
    absR = np.abs(Xs) + W0 @ T0
    R = Xs - W0 @ T0
    if csrx:
        want_obj = 0.5 * float((R ** 2).sum())
        obj_bound = wc.C64 * (n * d + k + 2) * U * 0.5 * float((absR ** 2).sum())
    else:
        want_obj = 0.5 * float((M * R ** 2).sum())
        obj_bound = wc.C64 * (A.nnz + k + 2) * U * 0.5 * float((M * absR ** 2).sum())
    pos = (np.maximum(R, 0.0) ** 2 * (1.0 if csrx else M)).sum(axis=1)
    rs = np.random.RandomState(A.nnz)
    with (csrx_engine if csrx else pattern_engine)(A, k, store) as e:
        e.set_W(W0); e.set_T(T0); e.set_params(reset_topic_method=None)
        got = e.objective()
        assert abs(got - want_obj) <= obj_bound, ('objective', got, want_obj, obj_bound)
        parts = e.objective_parts()
        assert abs(parts[0] - want_obj) <= obj_bound, ('objective_parts[0]', parts[0], want_obj, obj_bound)
        assert_rel(parts[1], float((W0 ** 2).sum()), 1e-12, 'objective_parts[1] = sum W^2')
        val, row = e.resid_row_argmax()
        assert pos[row] >= pos.max() * (1 - 1e-12), 'arg-max row %d holds %r, row %d holds %r' % (row, pos[row], np.argmax(pos), pos.max())
        assert pos[row] > 0, 'the case has no positive residual'
        assert_rel(val, pos[row], 1e-11, 'sum_j max(X - W T, 0)^2 of row %d' % row)
        bound = 4.0 * (k + 2) * U * absR
        for i in sorted({row, 0, n - 1, n // 2}):
            want = np.maximum(R[i], 0.0) * (1.0 if csrx else M[i])
            assert_elementwise(e.reset_row(i)[None, :], want[None, :], bound[i][None, :], 'reset row %d' % i, cols_are='columns')
        for m in (1, 9, 64):
            B, Q = rs.randn(d, m), rs.randn(n, m)
            assert_elementwise(e.X_times(B), Xs @ B, 4.0 * (d + 2) * U * (np.abs(Xs) @ np.abs(B)), 'X B, m = %d' % m,
                               rows_are='segments (rows)', cols_are='column group of 64')
            assert_elementwise(e.Xt_times(Q), Xs.T @ Q, 4.0 * (n + 2) * U * (np.abs(Xs).T @ np.abs(Q)), 'X^T Q, m = %d' % m,
                               rows_are='segments (columns)', cols_are='column group of 64')


# ---- 2. the dense weighted one-pass step ----------------------------------------------------------------------------------
DENSE = wc.dense_cases()


def dense_problem(n, d, k, M, store, seed=0):
    X, W0, T0 = wc.planted_dense(n, d, k, M, seed)
    return stored(X, wc.STORES[store]), W0, T0


def dense_engine(Xs, M, k, store):
    e = engine(Xs.shape[0], Xs.shape[1], k, dtype=wc.STORES[store], weighted=True)
    e.upload_X(Xs); e.upload_mask(M)
    return e


def assert_dense_routes(e, n, d, store, M, routes, what):
    info = e.layout_info()
    want = wc.dense_layout(n, d, store)
    for f in ('rpb', 'nrb', 'npanels', 'wtrow_small', 'interleaved'):
        assert info[f] == want[f], '%s: the handle reports %s = %r, rri_create restated gives %r' % (what, f, info[f], want[f])
    for f, v in routes.items():
        assert info[f] == v, '%s: the handle reports %s = %r, the case is named for %r (%r)' % (what, f, info[f], v, info)
    if info['mask_density'] is not None:
        assert abs(info['mask_density'] - float((M != 0).mean())) < 1e-8, (what, info['mask_density'], float((M != 0).mean()))
        assert info['mask_cols'] == (info['mask_density'] <= 0.12 and os.environ.get('RRI_WMCORR_COLS', '1') != '0'), (what, info)
    return info


@pytest.mark.parametrize('store', list(wc.STORES))
@pytest.mark.parametrize('case', DENSE, ids=[c[0] for c in DENSE])
def test_dense_weighted_topic_steps(monkeypatch, case, store):
    """k_wpass / k_wpass_occ4 with k_wmcorr / k_wmcorr_cols supplying the pending dw t^T term, k_wreduce + k_wtrow in the split
    step and k_wtrow_small inside sweep(), on either side of the mask-density switch and with the switches forced"""
    name, n, d, k, make_mask, env, routes, flags_name = case
    for key, val in env.items():
        monkeypatch.setenv(key, val)          # read when a handle is created
    M = make_mask()
    Xs, W0, T0 = dense_problem(n, d, k, M, store)
    kw = dict(STEP_FLAGS[flags_name], reset_topic_method=None)
    if kw.get('project_T_each_iter'):        # the start the oracle's own preparation leaves alone
        T0 = oracle().proj_rows_simplex(T0, kw['t_row_sum'])
    what = '%s-%s' % (name, store)
    with dense_engine(Xs, M, k, store) as e:
        e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        sb = wc.StepBound(Xs, M, store, tables=False)
        worst = drive_weighted_steps(e, sb, k, kw, 2, what)
        assert_dense_routes(e, n, d, store, M, routes, what)
    report('dense weighted steps ' + what, worst)
    with dense_engine(Xs, M, k, store) as e:
        e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        e.sweep_stepwise()
        step_WT = e.get_W(), e.get_T()
    worst = assert_whole_sweeps(lambda: dense_engine(Xs, M, k, store), lambda: wc.StepBound(Xs, M, store, tables=False), step_WT,
                                Xs, M, k, W0, T0, kw, store, what)
    report('dense weighted sweep() ' + what, worst)


@pytest.mark.parametrize('store', list(wc.BIG))
def test_dense_weighted_steps_without_interleaved_row_chunks(store):
    """npanels >= 2 and npanels * nrb > 1024: the read-only pass after a rebuild deals whole row-block ranges (the smallest
    shape that gets there in each storage type); nrb > 64, so sweep() takes k_wreduce + k_wtrow as the split step does and must
    give the same bits"""
    n, d = wc.BIG[store]
    k = 2
    M = wc.mask01(n, d, 0.3, 1)
    Xs, W0, T0 = dense_problem(n, d, k, M, store)
    kw = dict(reset_topic_method=None)
    what = 'npanels*nrb>1024-%s' % store
    with dense_engine(Xs, M, k, store) as e:
        e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        info = assert_dense_routes(e, n, d, store, M, dict(interleaved=False, wtrow_small=False, mask_bits=True), what)
        assert info['npanels'] >= 2 and info['npanels'] * info['nrb'] > 1024, info
        sb = wc.StepBound(Xs, M, store, tables=False)
        worst = drive_weighted_steps(e, sb, k, kw, 2, what)
    report('dense weighted steps ' + what, worst)
    with dense_engine(Xs, M, k, store) as e:
        e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        e.sweep_stepwise()
        step_WT = e.get_W(), e.get_T()
    worst = assert_whole_sweeps(lambda: dense_engine(Xs, M, k, store), lambda: wc.StepBound(Xs, M, store, tables=False), step_WT,
                                Xs, M, k, W0, T0, kw, store, what)
    report('dense weighted sweep() ' + what, worst)
