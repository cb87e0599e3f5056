"""What a handle keeps between calls must not outlive the T it was computed from: Qt = X T^T and Gfull = T T^T, which a sweep
with T fixed computes once and reuses (k_xtt / k_gram, k_wsweep_rows or k_wcol per topic).

Two sequences on ONE handle in which T changes between two fixed-T sweeps by a route that once kept both:
  * a handle of the explicit-residual schedule whose free sweep steps T (enqueue_rT_half);
  * a reset applied with no run paused (rri_apply_reset_vectors).
rri_apply_reset_max_resid has no engine wrapper outside a paused run (RRIEngine reaches it only through a pending event), so it
has no case here.

Those two came first and stay as they were.  Everything below them runs sequences of calls on ONE handle against the float64
model of tests/cs_cases.py, which caches nothing, operation by operation (cs_cases.run_sequence: the model restarts from the
handle's own W and T before every operation, so a failure names the operation and no rounding accumulates):
  * directed sequences, one test per row of the table above changed() in rri_hip.hip and per route that makes the row stale;
  * test_random_sequence: 12 operations drawn from the flavour's alphabet, 24 seeds per flavour (RRI_CACHED_STATE_CASES raises it).
Tolerances and what the operations are: the docstring of tests/cs_cases.py.  That a stale value cannot hide under them is
tests/test_cached_state_cases_cpu.py's to show.

Frozen statistics, uniform rows and an X built from a DeviceCorpus came after that table; rri_frozen_set / _absorb call no
changed() on purpose, rri_set_uniform_rows and rri_csr_scale_X_uniform reach one through rri_csr_scale_X, rri_upload_X_corpus
through upload_X_csr_kept.  The model holds all three, four flavours draw them into sequences ('gram-frozen' under RRI_ONCHIP=1,
'gram-frozen-fp32', 'csr-frozen', 'csr-uniform'), and the directed cases below put each between the operations that fill and use
the carry, the pending column verdict, the cross terms, the tracked objective, Qt and ||X||^2.  That these cases can fail was
checked with four mutations of rri_hip.hip, one at a time, the whole file run against each (every failure a wrong number or a
wrong verdict, none a fault):
  1. `!c->fzB` dropped from the tracked-objective condition of rri_objective: both cases of
     test_tracked_objective_and_persistent_launches_follow_the_statistics fail (objective() right behind set_frozen answers
     without the frozen rows' share, off by 18 % and more), and test_random_sequence[gram-frozen-4] and [gram-frozen-fp32-17];
  2. `!c->fzB` dropped from the k_trow_small condition of enqueue_T_half: 16 of the 20 cases of
     test_statistics_change_between_producer_and_consumer (all but xy-set and fixed_T, which run no free T-row step under
     statistics), test_column_verdict_with_and_without_statistics, test_carry_after_a_borrower[absorb-sweep] and its CSR twin,
     test_uniform_rows_behind_statistics_are_refused (the sweep behind the refusal), the [clear] case of the tracked-objective
     test (its sweep under statistics) and 52 random sequences of the three flavours with statistics (W off by 4e-3 .. 3e-2);
  3. changed(c, CH_X) taken out of the end of rri_csr_scale_X: all 15 set_uniform_rows cases of
     test_a_change_of_X_beside_the_pattern_drops_what_came_from_X (value, list and clear, each for x_sq, xy, q and both carries),
     its preprocess_csr_uniform-x_sq and -q cases, 9 random sequences of 'csr-uniform' and 2 of 'csr-frozen' (preprocess_csr);
  4. wcheck_now without the addend s[t] (k_frozen_add_tail not launched): both cases of
     test_column_verdict_with_and_without_statistics end the sweep under statistics in the error the oracle has only after
     clear_frozen.
No case failed on the unmodified library.

The early-sums schedule keeps four more fields -- early_valid / early_topic (the partials of T T[t,:]^T in Tearly) and
carry_wfin / wfin_topic (the carry is k_wfin's) -- and at 700 x 333 only RRI_TROW_SMALL=0 reaches it: the flavours 'gram-early',
'gram-early-fp32' and 'gram-early-u8' draw the alphabets of their twins and the evaluation calls into sequences on it (a sequence
with a sweep that admits the schedule must end with early_steps > 0: run_case), and the directed cases 'early-*' are "sweep, change,
sweep or half step" for every row of the table a plain handle has, for a change between the T half and the W half of one topic, for
every evaluation call between k_wfin and the T half that takes up its carry, for parameters that switch the schedule off and back
without a changed(), and for a call that ends in an error.  That they can fail: three more mutations, host-side flags only (every
index stays in bounds, the numbers go stale), one line at a time, the whole file against each:
  5. `if (what) c->early_valid = false;` taken out of changed(): the four cases of test_a_change_between_the_two_halves_of_a_topic
     (update_W_col(2) behind reset-own-topic off by 1.1e+0 in W, reset-other-topic 2.2e-2, rollback 9.5e-1, set_T 7.6e-1) and
     test_a_lone_W_half_of_the_last_topic_after_set_T (7.5e+0); no random sequence of the 24 default seeds puts a write from outside
     between the two halves of one topic, which is why the directed cases are there;
  6. `&& c->early_topic == t` taken out of enqueue_W_half: test_a_W_half_of_another_topic_than_the_T_half_before_it (W off by 5.4e-1),
     test_random_sequence[gram-early-20] (update_T_row(2), update_W_col(1): 9.4e-1) and [gram-frozen-21] (update_T_row(2),
     update_W_col(3) under statistics: 3.0e+0);
  7. `if (c->carry_wfin && !early) c->carry_valid = false;` taken out of enqueue_T_half: both cases of
     test_parameters_without_the_schedule_and_back (the sweep under fix_W off by 1.6e+0 in T and 1.8e+0 in W, update_T_row(0) by
     1.6e+0) and test_statistics_change_between_producer_and_consumer[plain-carry-clear-sweep] (the sweep behind clear_frozen, where
     a handle of this size goes back to k_trow_small: T off by 1.7e+0).
Again no case failed on the unmodified library.

Reference of the two earlier sequences: the CPU oracle, chained call by call with W_in / T_in, eps_stop=-1, in float64.  Tolerance: relfro < 1e-9 on W and
on T of a float64 handle (summation order only, as tests/test_residual_gpu.py between two float64 runs).  A stale Qt cannot
hide under it: given the T of the first fixed call in place of the current one, the oracle's last call ends with a W that is
off by relfro 1.2e-1 in the first sequence and by 8.2e-1 in the second.
"""
import numpy as np
import pytest

import cs_cases as cs
from conftest import relfro
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu

N, D, K = 700, 333, 6
TOL = 1e-9


def problem():
    X = planted_X(N, D, K, seed=5, dtype=np.float64)      # as test_residual_gpu.py's resumability case
    W0, T0 = scaled_init(X, K, seed=6)
    return X, W0, T0


def oracle_chain(X, W, T, calls):
    """calls: (sweeps, flags) one after the other, each starting from the factors the one before left"""
    from oracle import rri_oracle
    for sweeps, flags in calls:
        out = rri_oracle.nmf(X, K, W_in=W.copy(), T_in=T.copy(), max_iter=sweeps, eps_stop=-1, **flags)
        W, T = out['W'], out['T']
    return W, T


def engine_chain(X, W0, T0, calls, schedule):
    from rri_nmf_amd.engine import RRIEngine
    with RRIEngine(N, D, K, dtype=np.float64, schedule=schedule) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0)
        for sweeps, flags in calls:
            e.set_params(**flags)
            e.sweep(sweeps)
        return e.get_W(), e.get_T()


@pytest.mark.parametrize('wsweep', [None, '0'])
def test_residual_handle_free_sweep_between_two_fixed_T_sweeps(monkeypatch, wsweep):
    """sweep(2) free, T fixed sweep(1), free sweep(1), T fixed sweep(1): the last call must use the T of the third"""
    if wsweep is None:
        monkeypatch.delenv('RRI_WSWEEP', raising=False)
    else:
        monkeypatch.setenv('RRI_WSWEEP', wsweep)           # read at rri_create
    X, W0, T0 = problem()
    calls = [(2, {}), (1, dict(fix_T=True)), (1, {}), (1, dict(fix_T=True))]
    Wr, Tr = oracle_chain(X, W0, T0, calls)
    W, T = engine_chain(X, W0, T0, calls, 'residual')
    ew, et = relfro(W, Wr), relfro(T, Tr)
    print('residual handle vs oracle: W %.3e  T %.3e' % (ew, et))
    assert ew < TOL and et < TOL, (ew, et)
    Wg, Tg = engine_chain(X, W0, T0, calls, 'gram')        # and the default schedule
    ew, et = relfro(W, Wg), relfro(T, Tg)
    print('residual handle vs Gram-form handle: W %.3e  T %.3e' % (ew, et))
    assert ew < TOL and et < TOL, (ew, et)


def test_reset_outside_a_paused_run_between_two_fixed_T_sweeps(monkeypatch):
    """T fixed sweep(1), row 3 of T replaced by rri_apply_reset_vectors with no run paused, T fixed sweep(1)"""
    from rri_nmf_amd.engine import RRIEngine
    monkeypatch.setenv('RRI_ONCHIP', '0')
    X, W0, T0 = problem()
    new_row = np.random.RandomState(7).rand(D)
    new_row /= new_row.sum()
    W1, T1 = oracle_chain(X, W0, T0, [(1, dict(fix_T=True))])
    T1 = T1.copy()
    T1[3, :] = new_row
    Wr, Tr = oracle_chain(X, W1, T1, [(1, dict(fix_T=True))])
    with RRIEngine(N, D, K, dtype=np.float64) as e:
        e.upload_X(X), e.set_W(W0), e.set_T(T0)
        e.set_params(fix_T=True)
        e.sweep(1)
        e.apply_reset_vectors(3, new_row, e.get_W()[:, 3])
        e.sweep(1)
        W, T = e.get_W(), e.get_T()
    ew, et = relfro(W, Wr), relfro(T, Tr)
    print('reset between fixed-T sweeps vs oracle: W %.3e  T %.3e' % (ew, et))
    assert ew < TOL and et < TOL, (ew, et)


# ---- sequences against the model of cs_cases.py --------------------------------------------------------------------------
def run_case(monkeypatch, flavour, ops, raises=None):
    """the handle of the flavour through ops, every operation checked; on the RRI_ONCHIP=1 flavour every sweep with both factors
    free must have been a persistent launch (a launch that gave up for want of co-resident workgroups, onchip_fallbacks, keeps
    the handle off that path for seconds: then one launch is all that is asked)"""
    for key, val in cs.FLAVOURS[flavour]['env'].items():
        monkeypatch.setenv(key, val)                       # read at rri_create
    lines = []
    onchip = cs.FLAVOURS[flavour]['env'].get('RRI_ONCHIP') == '1'      # 'gram-onchip' and 'gram-frozen'
    e = cs.make_engine(flavour)
    try:
        if onchip:
            assert e.onchip_info()[0], '700 x 333 float64 is not eligible for the register-resident sweep'
        try:
            answers = cs.run_sequence(e, flavour, ops, log=lines.append, raises=raises)
        finally:
            print('\n'.join(lines))
        if onchip:
            launches, want = e.onchip_info()[1], cs.persistent_sweeps(ops)
            print('persistent launches: %d of %d free sweeps' % (launches, want))
            assert launches >= (want if e.onchip_fallbacks() == 0 else min(want, 1)), (launches, want, e.onchip_fallbacks())
        if flavour in cs.EARLY_FLAVOURS:
            # the flavour is there for the early-sums schedule: a sequence with a sweep under parameters that admit it has taken k_wfin
            info, want = e.layout_info(), cs.early_sweeps(ops, raises)
            print('early-sums schedule: %d W halves through k_wfin, %d sweeps that must have taken it' % (info['early_steps'], want))
            assert want == 0 or info['early_steps'] > 0, (info, want)
            assert info['early_sums'] == cs.early_schedule(final_pname(ops)), info
        return answers
    finally:
        e.close()


def final_pname(ops):
    """the parameter set (cs.PARAMS) a handle holds after ops"""
    ls = cs.LegalState('plain')
    for op in ops:
        ls.follow(op)
    return ls.pname


def directed(monkeypatch, name):
    case = cs.CASES[name]
    return run_case(monkeypatch, case.flavour, case.ops, raises=case.raises)


@pytest.mark.parametrize('route', ['upload_X', 'scale_X', 'bind_X_device'])
def test_x_sq_after_another_X(monkeypatch, route):
    """x_sq_valid: sweep(1), objective() takes ||X||^2, X changes, sweep(1), objective().  bind_X_device binds a torch tensor, at
    d = 334 (cs_cases); where this is the first use of torch.cuda in the process, the seconds it takes are torch's start"""
    directed(monkeypatch, 'x_sq-' + route)


@pytest.mark.parametrize('route', ['project_W_rows', 'rollback', 'apply_reset_vectors', 'set_T'])
def test_cross_terms_after_an_outside_write(monkeypatch, route):
    """xy_run / xy_valid: sweep(1), objective() from the cross terms, W or T written from outside, objective()"""
    directed(monkeypatch, 'xy-' + route)


def test_tracked_objective_after_other_penalties(monkeypatch):
    """obj_track_valid (RRI_ONCHIP=1): sweep(2), objective(), set_params with other penalties, objective() carries the new ones"""
    directed(monkeypatch, 'obj_track-set_params')


def test_tracked_objective_after_a_W_half(monkeypatch):
    """obj_track_valid (RRI_ONCHIP=1): sweep(2), update_W_col(1), objective()"""
    directed(monkeypatch, 'obj_track-update_W_col')


@pytest.mark.parametrize('route', ['set_T', 'rollback', 'scale_X', 'upload_X'])
def test_fixed_T_products_after_a_change(monkeypatch, route):
    """q_valid / gfull_valid: a fixed-T sweep(1), T or X changed, a fixed-T sweep(1)"""
    directed(monkeypatch, 'q-' + route)


@pytest.mark.parametrize('stored_by', ['sweep', 'objective'])
@pytest.mark.parametrize('route', ['set_W', 'set_T', 'rollback', 'project_W_rows', 'new_mask'])
@pytest.mark.parametrize('layout', ['weights', 'bits', 'pattern'])
def test_maintained_residual_after_an_outside_change(monkeypatch, layout, route, stored_by):
    """resid_valid: sweep(1), an outside change, sweep(1) on the three weighted layouts (dense weights, a dense 0/1 mask packed
    to bits, the observed pattern only).  A sweep rebuilds E at its start unless the objective has just stored it, so each route
    runs a second time with objective() before the change: with CH_M taken out of changed() only those cases fail"""
    directed(monkeypatch, 'resid-%s-%s%s' % (layout, route, '-after_objective' if stored_by == 'objective' else ''))


@pytest.mark.parametrize('layout', ['weights', 'bits', 'pattern'])
def test_maintained_residual_stored_by_the_objective(monkeypatch, layout):
    """resid_valid, the legitimate path: sweep(1), objective() stores E, and the sweep(1) that follows skips its rebuild"""
    directed(monkeypatch, 'resid-%s-objective_between_sweeps' % layout)


@pytest.mark.parametrize('stored_by', ['sweep', 'objective'])
def test_maintained_residual_after_a_bound_mask(monkeypatch, stored_by):
    """resid_valid, rri_bind_mask_device: sweep(1) [, objective()], a mask in caller-owned device memory (a torch tensor; a weighted
    float64 handle at d = 334, which the call accepts), sweep(1)"""
    directed(monkeypatch, 'resid-bound_mask' + ('-after_objective' if stored_by == 'objective' else ''))


def test_explicit_residual_after_a_foreign_rank_one_update(monkeypatch):
    """resid_valid, explicit-residual handle: sweep(1), residual_update(a, b, trow, wcol), sweep(1)"""
    directed(monkeypatch, 'resid-residual_update')


def test_explicit_residual_across_the_form_switch(monkeypatch):
    """resid_valid, explicit-residual handle: free sweep(1), fixed-T sweep(1) (stepped in the Gram form), free sweep(1): the form
    switch of rri_set_params"""
    directed(monkeypatch, 'resid-form_switch')


@pytest.mark.parametrize('then', ['sweep', 'update_T_row'])
@pytest.mark.parametrize('borrower', ['Xt_times', 'column_positive_counts', 'range_finder', 'X_times'] + cs.BORROWERS + ['absorb'])
def test_carry_after_a_borrower(monkeypatch, borrower, then):
    """carry_valid / carry_topic: after a free sweep Zpart / Gpart hold topic 0's partial sums; a borrower runs, then sweep(1) or
    update_T_row(0).  Only column_positive_counts tells: it sums into Zpart and reduces into red, and with CH_SCRATCH taken out
    of changed() its two cases fail (T off by 4e+1).  rri_Xt_times and rri_range_finder say CH_SCRATCH but keep their partial
    sums in a buffer of their own (DevTmp zm), and rri_X_times on a dense handle calls no changed() at all: their cases show
    that the carry survives them, which is all they can show.  The evaluation calls (topn_rows, rank_entries, entries_loglik,
    cooccurrence_counts, masked_rmse, argmax_rows) and absorb promise to write nothing a later sweep reads: their answers are
    checked against the handle's current W and T with each feature's own reference and bound (cs_cases.check_borrowed), W and T
    must be bit for bit what they were, and the step that follows must be the model's"""
    directed(monkeypatch, 'carry-%s-%s' % (borrower, then))


@pytest.mark.parametrize('then', ['sweep', 'update_T_row'])
@pytest.mark.parametrize('borrower', cs.CORPUS_BORROWERS + ['absorb'])
def test_carry_after_a_borrower_on_csr(monkeypatch, borrower, then):
    """the same on a CSR handle, for the two calls that score a live DeviceCorpus (rri_corpus_entries_loglik,
    rri_corpus_cooccurrence_counts; the corpus is closed after the call) and for absorb, which takes W^T X through the blocked
    product behind rri_Xt_times"""
    directed(monkeypatch, 'carry-%s-csr-%s' % (borrower, then))


@pytest.mark.parametrize('stored_by', ['sweep', 'objective'])
@pytest.mark.parametrize('flavour', ['weighted', 'pattern', 'residual'])
@pytest.mark.parametrize('borrower', cs.BORROWERS)
def test_maintained_residual_after_an_evaluation_call(monkeypatch, borrower, flavour, stored_by):
    """resid_valid: sweep(1) [, objective()], an evaluation call, sweep(1) on the handles that keep a residual between calls: the
    calls work on every flavour and must leave it alone"""
    directed(monkeypatch, 'resid-%s-%s%s' % (borrower, flavour, '-after_objective' if stored_by == 'objective' else ''))


def test_sweep_after_a_call_that_ended_in_an_error(monkeypatch):
    """CH_ENDED and the pending column verdict: W with a zero column and no resets, sweep(1) raises as the oracle does, then
    set_W(good), sweep(1)"""
    case = cs.CASES['ended-zero_column']
    run_case(monkeypatch, case.flavour, case.ops, raises=case.raises)


# ---- the uint8 store: the scale vectors are a part of X ----------------------------------------------------------------------
@pytest.mark.parametrize('row', ['x_sq', 'xy', 'q'])
def test_a_changed_scale_drops_what_came_from_X(monkeypatch, row):
    """rri_set_X_scales on a uint8 handle between the operations that fill and use ||X||^2 (x_sq_valid), the cross terms of a
    sweep (xy_valid) and Qt = X T^T of a fixed-T sweep (q_valid): it calls no changed() itself but goes through rri_scale_X"""
    directed(monkeypatch, row + '-set_X_scales')


@pytest.mark.parametrize('then', ['sweep', 'update_T_row'])
def test_carry_after_a_changed_scale(monkeypatch, then):
    """carry_valid: a free sweep leaves the partial sums of topic 0 taken from X; both scale vectors change; sweep(1) or
    update_T_row(0) must take them from the new X"""
    directed(monkeypatch, 'carry-set_X_scales-' + then)


@pytest.mark.parametrize('route', ['upload_X', 'bind_X'])
def test_a_new_X_puts_the_scales_back_to_ones(monkeypatch, route):
    """set_X_scales, sweep(1), other counts uploaded or bound, sweep(1), objective(): the new counts are factorised as they are"""
    directed(monkeypatch, 'scales-reset-by-' + route)


def test_fixed_T_products_after_scaling_a_bound_X(monkeypatch):
    """q_valid on bound memory: only a uint8 handle rescales a bound X (it writes the column scales, no matrix)"""
    directed(monkeypatch, 'q-scale_X-bound')


# ---- frozen statistics, uniform rows, an X built from a DeviceCorpus -----------------------------------------------------------------
@pytest.mark.parametrize('case', ['carry-set-sweep', 'carry-set-update_T_row', 'carry-clear-sweep', 'carry-other-sweep', 'xy-set', 'xy-clear',
                                  'reset', 'rollback', 'online', 'fixed_T'])
@pytest.mark.parametrize('store', ['plain', 'csr'])
def test_statistics_change_between_producer_and_consumer(monkeypatch, store, case):
    """rri_frozen_set / rri_frozen_absorb call no changed(): the statistics are read where a step uses them.  What one set of
    statistics produced -- the carried sums of topic 0 and the pending column verdict of a free sweep, the cross terms of the
    objective -- is consumed after they were set, cleared or replaced; a reset with no run paused zeroes topic t; a rollback
    restores W and T only; a new X behind an absorb (the online loop) brings its own ||X||^2 and leaves c; sweeps with T fixed
    ignore them.  The statistics are read back after every operation: bit for bit, after an absorb within the bound of
    test_absorb_takes_the_sums_of_the_handles_rows"""
    directed(monkeypatch, 'frozen-%s-%s' % (store, case))


@pytest.mark.parametrize('store', ['plain', 'csr'])
def test_column_verdict_with_and_without_statistics(monkeypatch, store):
    """wcheck_now: under 'pen_a' column K - 1 of W, zero on the handle's rows, stays zero through its W half; with statistics whose
    s[K - 1] > 0 the sweep ends without an error, after clear_frozen the next one ends in the oracle's"""
    case = cs.CASES['frozen-%s-verdict' % store]
    run_case(monkeypatch, case.flavour, case.ops, raises=case.raises)


@pytest.mark.parametrize('case', ['set', 'clear'])
def test_tracked_objective_and_persistent_launches_follow_the_statistics(monkeypatch, case):
    """RRI_ONCHIP=1: sweep(2) persistent, objective(), set_frozen, objective() must carry the frozen rows' share; then sweep(1), no
    persistent launch and onchip_info()[0] False, clear_frozen, sweep(1) persistent again, objective() (cs_cases.run_sequence
    counts the launches of every sweep)"""
    directed(monkeypatch, 'frozen-obj_track-' + case)


@pytest.mark.parametrize('use', ['x_sq', 'xy', 'q', 'carry-sweep', 'carry-update_T_row'])
@pytest.mark.parametrize('change', ['set_uniform_rows-value', 'set_uniform_rows-list', 'set_uniform_rows-clear', 'preprocess_csr_uniform',
                                    'upload_X_corpus'])
def test_a_change_of_X_beside_the_pattern_drops_what_came_from_X(monkeypatch, change, use):
    """rri_set_uniform_rows (another value only, another list, a clear) and rri_csr_scale_X_uniform reach changed(c, CH_X) through
    rri_csr_scale_X and write the list and the value after it; rri_upload_X_corpus goes through upload_X_csr_kept, and the
    corpus is closed before the next operation.  Each between the operations that fill and use ||X||^2, the cross terms, Qt of a
    fixed-T sweep and the carried sums of topic 0"""
    name = '%s-%s' % (use, change) if not use.startswith('carry-') else 'carry-%s-%s' % (change, use[len('carry-'):])
    directed(monkeypatch, name)


def test_a_corpus_empties_the_list(monkeypatch):
    directed(monkeypatch, 'uniform-emptied-by-upload_X_corpus')


def test_the_store_built_from_a_corpus_is_that_of_upload_X_csr(monkeypatch):
    """after rri_upload_X_corpus both blocked stores equal, byte for byte, those of a second handle given the canonical matrix
    through rri_upload_X_csr"""
    import scipy.sparse as sp
    a = cs.make_engine('csr-frozen')
    b = cs.make_engine('csr-frozen')
    try:
        m = cs.Model('csr-frozen')
        op = cs.Op('upload_X_corpus', 3)
        m.apply(op)
        cs.apply_engine(a, m, op)
        b.upload_X_csr(sp.csr_matrix(cs.corpus_raw(m.d, 3)[1]))
        for which in (0, 1):
            sa, sb = a.sparse_store(which), b.sparse_store(which)
            for key in sa:
                if key != 'build_us':
                    assert np.array_equal(sa[key], sb[key]) and np.asarray(sa[key]).tobytes() == np.asarray(sb[key]).tobytes(), (which, key)
    finally:
        a.close(), b.close()


@pytest.mark.parametrize('second', ['set_uniform_rows', 'preprocess_csr_uniform'])
def test_uniform_rows_behind_statistics_are_refused(monkeypatch, second):
    """statistics first, uniform rows second: RRI_ERR_UNSUPPORTED (NotImplementedError) as frozen_refusal() answers the other
    order, and X (both blocked stores), the list, the statistics, W and T are bit for bit what they were (cs_cases.fingerprint);
    the sweep(1) that follows is the model's"""
    case = cs.CASES['mixed-' + second]
    run_case(monkeypatch, case.flavour, case.ops, raises=case.raises)


# ---- the early-sums schedule: early_valid / early_topic, carry_wfin / wfin_topic ('gram-early': RRI_TROW_SMALL=0) -----------------------
EARLY_TABLE = ['x_sq-upload_X', 'x_sq-scale_X', 'xy-project_W_rows', 'xy-rollback', 'xy-apply_reset_vectors', 'xy-set_T', 'q-set_T', 'q-upload_X',
               'carry-upload_X-sweep', 'carry-upload_X-update_T_row', 'carry-scale_X-sweep', 'carry-scale_X-update_T_row']


@pytest.mark.parametrize('case', EARLY_TABLE)
def test_rows_of_the_table_on_the_early_sums_schedule(monkeypatch, case):
    """every row of the table above changed() that a plain Gram-form handle has (resid_valid belongs to the weighted and explicit-
    residual handles, obj_track_valid to the persistent sweep), as "sweep, change, sweep or half step" with the first sweep on the
    schedule: the carry that the change finds is k_wfin's"""
    directed(monkeypatch, 'early-' + case)


@pytest.mark.parametrize('change', ['reset-own-topic', 'reset-other-topic', 'rollback', 'set_T'])
def test_a_change_between_the_two_halves_of_a_topic(monkeypatch, change):
    """early_valid: sweep(1), update_T_row(2) leaves T T[2,:]^T in Tearly, T is written from outside, update_W_col(2) must take
    k_wcol and the current T"""
    directed(monkeypatch, 'early-halves-' + change)


def test_a_lone_W_half_of_the_last_topic_after_set_T(monkeypatch):
    """early_valid: a sweep ends with early_topic = K - 1; set_T; update_W_col(K - 1)"""
    directed(monkeypatch, 'early-lone_W_half-after-set_T')


def test_a_W_half_of_another_topic_than_the_T_half_before_it(monkeypatch):
    """early_topic: sweep(1), update_T_row(2), update_W_col(3): the partials in Tearly are topic 2's"""
    directed(monkeypatch, 'early-topic-other_W_half')


@pytest.mark.parametrize('then', ['sweep', 'update_T_row'])
@pytest.mark.parametrize('borrower', cs.BORROWERS)
def test_k_wfin_carry_after_a_borrower(monkeypatch, borrower, then):
    """carry_wfin / wfin_topic: after a sweep on the schedule the carry of topic 0 is k_wfin's -- red reduced, two Gram entries as
    tile sums in wfp; an evaluation call runs between it and the T half that takes it up (test_carry_after_a_borrower has the rules)"""
    directed(monkeypatch, 'early-carry-%s-%s' % (borrower, then))


@pytest.mark.parametrize('then', ['sweep', 'update_T_row'])
def test_parameters_without_the_schedule_and_back(monkeypatch, then):
    """carry_wfin under early_ok false: sweep(1), set_params(fix_W) (no penalty changes: no changed()), a T half that finds k_wfin's
    carry and must start from the prologue, set_params(free), sweep(1)"""
    directed(monkeypatch, 'early-off_and_on-' + then)


def test_sweep_on_the_schedule_after_a_call_that_ended_in_an_error(monkeypatch):
    """CH_ENDED: sweep(1), W with a zero column, sweep(1) raises as the oracle does in the middle of the schedule, set_W(good), sweep(1)"""
    case = cs.CASES['early-ended-zero_column']
    run_case(monkeypatch, case.flavour, case.ops, raises=case.raises)


@pytest.mark.parametrize('seed', range(cs.n_seeds()))
@pytest.mark.parametrize('flavour', cs.RANDOM_FLAVOURS)
def test_random_sequence(monkeypatch, flavour, seed):
    ops = cs.random_sequence(flavour, seed)
    print(ops)
    run_case(monkeypatch, flavour, ops)
