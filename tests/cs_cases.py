"""A float64 model of what one RRIEngine handle holds between calls, and the sequences of calls that tests/test_cached_state_gpu.py
runs against it (tests/test_cached_state_cases_cpu.py checks the cases themselves, without a GPU).

The handle caches (the table above changed() in rri_hip.hip): carry_valid / carry_topic, resid_valid, xy_run / xy_valid,
obj_track_valid, q_valid, gfull_valid, x_sq_valid.  The model caches nothing: it holds X, M (or None), W, T, the current
parameters and a snapshot, and every operation recomputes what it needs from those with numpy and the CPU oracle.  A sequence is
checked PER OPERATION (run_sequence): W and T are read from the handle before the operation (rri_get_W / rri_get_T touch no
flag), the model computes the state the operation must leave from those, the operation runs on the handle, and the handle's new
state is compared.  Rounding cannot accumulate over a sequence, and a failure names the operation.  The handle carries its
caches through the sequence and the model has none: that difference is the test.

Shape: n, d, k = 700, 333, 6, planted_X(seed=5) and scaled_init(seed=6) as the two sequences that test_cached_state_gpu.py had
before.  Two exceptions, both forced by rri_bind_X_device, which refuses a d that is no multiple of 16 bytes / itemsize:
the float32 flavour runs at d = 336 and the directed bind_X_device and bind_mask_device cases (float64) at d = 334.

The uint8 flavour ('gram-u8', d = 336, a multiple of its 8-byte loads) stores counts C with zeros and two float64 vectors; its X is
(C * s) * r[:, None].  The model holds C, r and s next to X: upload_X and bind_X (a torch.uint8 tensor) put both vectors back to
ones, set_X_scales(salt) replaces the row vector, the column vector or both, scale_X multiplies s, and preprocess leaves the
oracle's normalize(tfidf(X)) of the scaled matrix, with s * idf and r / row total in the vectors.  Nothing is rounded twice, so
scale_X and preprocess are in its alphabet at the float64 tolerance, and -- as they write no matrix -- also on a bound X.

What the operations deviate from a plain nmf() call in, and why:
  * 'simplex' (t_row_sum=1 with project_T_each_iter): rri_oracle.nmf projects the T it is given before its first sweep, as the
    reference does, and rri_sweep does not (the driver nmf.py projects and sets T).  So set_params('simplex') is the driver's
    pair -- set_params, then set_T of the projected T -- every T written from outside while they hold has rows that sum to 1, and rollback is
    drawn only onto a T that is feasible: the oracle's projection is then the identity (Model.sweep_from asserts 1e-12).
  * update_T_row leaves the rescaling of W[:, t] (nmf.py:474) to the W half that follows it (enqueue_T_half), so after it
    column t of W is not compared, as check_steps of test_kernel_buckets_gpu.py does not.
  * residual_update's return values depend on the stored residual, which is no part of the model (it is rebuilt from W and T
    before it is next used): they are not compared here; test_residual_gpu.py owns them.
  * preprocess(tfidf=True, normalize=True) is drawn only while the handle's X has zeros: planted_X is positive everywhere, its
    idf is log(1) = 0 and the X it would leave is the constant 1 / d.  It leaves an X some fifty times smaller, and factors of
    the old size overshoot it so far that the next sweep kills topics; so the operation is preprocess followed by set_W of
    W * mean(X after) / mean(X before), as a driver that preprocesses starts its factors at the new scale.  That set_W drops
    the first four rows of the table; ||X||^2, Qt and Gfull are left to preprocess's own CH_X, and scale_X is the pure case.

Tolerances (all the project's own): W and T after one operation relfro < 1e-9 on a float64 handle (the two earlier sequences
of test_cached_state_gpu.py, test_residual_gpu.py), 1e-7 on the float32 one (test_fuzz_gpu.py); the objective of a weighted
handle, which always takes the residual path, 1e-12 relative (test_kernel_buckets_gpu.py), and so the objective of an unweighted
handle wherever the cross terms of a whole sweep cannot be valid -- after any write from outside, lone half step or new X
(LegalState.xy_possible); right after a whole sweep with W free, where the handle answers from the cross terms or from the
residual as its flags allow, 1e-11 * max(want, 1e-3 ||X||^2) (test_hip_parity.py).

State that came after the table above changed(), none of it cached and all of it carried by a handle from call to call; the four
flavours 'gram-frozen', 'gram-frozen-fp32', 'csr-frozen' and 'csr-uniform' draw it into their sequences, and directed cases put
it between the operations that fill and use every row of the table:
  * frozen statistics F = (B, A, s, c) or None (rri_frozen_set / _get / _absorb; frozen_cases.stats_of of N_O = 41 planted rows
    per salt).  With F set a sweep with T free is frozen_cases.frozen_sweep under the current parameters, a sweep with T fixed
    ignores F, update_T_row adds B[t] - A[t, others] T[others] to the numerator and A[t, t] to the denominator, the objective
    and objective_parts[0] add 1/2 (c - 2 <B, T> + <A, T T^T>), a reset zeroes topic t of F, rollback restores W and T only, a
    new X leaves F alone (the online loop), absorb(decay) is F <- decay F + stats_of(X, W) and leaves W and T bit for bit.  fix_W
    is illegal while F is set, set_frozen and absorb under fix_W and while uniform rows exist.  Like W and T, F is read from the
    handle before every operation and compared after it: bit for bit, after an absorb within the elementwise bound of
    test_absorb_takes_the_sums_of_the_handles_rows (u (n + 2) |W|^T |X| and the like) plus two roundings for decay F + sums.
    The objective with F set: 1e-12 * 1/2 (||X||^2 + c) (test_the_objective_is_that_of_the_stacked_problem).  On the
    RRI_ONCHIP=1 flavour every sweep's persistent launches are counted: none, and onchip_info()[0] False, while F is set.
  * uniform rows of a CSR handle: the model's X is dense, S + v e_U 1^T with S zeroed in U; the rows of a replaced list stay
    zero.  set_uniform_rows(salt) replaces the list (salt % 3 == 0), only the value (1) or clears it (2) and passes the list
    unsorted; preprocess_csr_uniform is preprocess(tfidf=True, normalize=True, uniform_rows=True) with the set_W rescale of
    preprocess_csr, legal only without a list and with zero-total rows (other_X with a salt from ZERO_ROWS, or the rows a
    cleared list leaves); a new X empties the list; preprocess_csr is illegal while there is one.  The list and the value are
    read back after every operation.
  * upload_X_corpus(salt): corpus_cases.raw_rows (shuffled, every third row with duplicates, explicit zeros) through
    DeviceCorpus.from_arrays; the corpus is closed before the next operation; the model's X is corpus_cases.canonical of it.
  * statistics first and uniform rows second is refused (NotImplementedError), with the handle bit for bit as it was (fingerprint).
  * the evaluation calls (topn_rows, rank_entries, entries_loglik, cooccurrence_counts, masked_rmse, argmax_rows, and on CSR the
    two that score a live DeviceCorpus) are LOOKs of the new flavours and borrowers of the directed carry and residual cases;
    check_borrowed holds each answer to the handle's current W and T with the feature's own reference and bound.
No case on the MI355X needed a looser bound than these.

The early-sums schedule keeps four more fields on the handle -- early_valid / early_topic, carry_wfin / wfin_topic --
and at this shape only RRI_TROW_SMALL=0 reaches it: the flavours 'gram-early', 'gram-early-fp32' and 'gram-early-u8' are 'gram-phases',
'gram-fp32' and 'gram-u8' under that switch, with the evaluation calls among their LOOKs, and the directed cases 'early-*' put every
change between the steps that fill and use those fields.  The model is the same: it has no schedule.
"""
import os

import numpy as np
import scipy.sparse as sp

from rri_nmf_amd.synthetic import planted_X, scaled_init

N, D, K = 700, 333, 6
D_F32, D_BIND = 336, 334

# ---- parameters ------------------------------------------------------------------------------------------------------------
PARAMS = {
    'free': dict(),
    'fix_T': dict(fix_T=True),
    'fix_W': dict(fix_W=True),
    'clip': dict(t_row_sum=1.0),
    'simplex': dict(t_row_sum=1.0, project_T_each_iter=True),
    'pen_a': dict(reg_w_l2=0.3, reg_t_l2=0.2, reg_w_l1=0.05, reg_t_l1=0.02),
    'pen_b': dict(reg_w_l2=0.7, reg_t_l2=0.1),
}
REGS = ('reg_w_l2', 'reg_t_l2', 'reg_w_l1', 'reg_t_l1')


def oracle():
    from oracle import rri_oracle
    return rri_oracle


# ---- flavours --------------------------------------------------------------------------------------------------------------
# kind: plain | residual | weighted | pattern | csr;  env: read at rri_create
FLAVOURS = {
    'gram-onchip': dict(kind='plain', dtype=np.float64, d=D, env={'RRI_ONCHIP': '1'}),
    'gram-phases': dict(kind='plain', dtype=np.float64, d=D, env={'RRI_ONCHIP': '0'}),
    'residual': dict(kind='residual', dtype=np.float64, d=D, env={}),
    'weighted': dict(kind='weighted', dtype=np.float64, d=D, env={}),
    'pattern': dict(kind='pattern', dtype=np.float64, d=D, env={}),
    'csr': dict(kind='csr', dtype=np.float64, d=D, env={}),
    'gram-fp32': dict(kind='plain', dtype=np.float32, d=D_F32, env={}),
    # the directed bind_X_device / bind_mask_device cases only (no random sequences): float64 at an even d
    'gram-bind': dict(kind='plain', dtype=np.float64, d=D_BIND, env={'RRI_ONCHIP': '0'}),
    'weighted-bind': dict(kind='weighted', dtype=np.float64, d=D_BIND, env={}),
    # uint8 counts C with float64 row and column scales r, s (RRI_U8): X = (C * s) * r[:, None], nothing rounded.  Appended last:
    # draw_sequence seeds by the position in RANDOM_FLAVOURS, and the sequences of the flavours above stay what they were
    'gram-u8': dict(kind='plain', dtype=np.uint8, d=D_F32, env={}),
    # the state that came after the table above changed(): frozen statistics, uniform rows, an X built from a DeviceCorpus.  Appended
    # after 'gram-u8' in this order, for the same reason
    'gram-frozen': dict(kind='plain', dtype=np.float64, d=D, env={'RRI_ONCHIP': '1'}, frozen=True),
    'gram-frozen-fp32': dict(kind='plain', dtype=np.float32, d=D_F32, env={}, frozen=True),
    'csr-frozen': dict(kind='csr', dtype=np.float64, d=D, env={}, frozen=True, corpus=True),
    'csr-uniform': dict(kind='csr', dtype=np.float64, d=D, env={}, uniform=True, corpus=True),
    # the early-sums schedule (RRI_EARLY_SUMS, on by default): at this shape every flavour above takes k_trow_small or runs on chip
    # and never reaches it, but for those with statistics.  RRI_TROW_SMALL=0 puts the three plain stores on it -- the early job in
    # the pass's grid, k_wfin, k_trow_early -- with early_valid / early_topic / carry_wfin / wfin_topic to keep right between
    # calls.  Appended last, for the same reason as the four above them
    'gram-early': dict(kind='plain', dtype=np.float64, d=D, env={'RRI_ONCHIP': '0', 'RRI_TROW_SMALL': '0'}),
    'gram-early-fp32': dict(kind='plain', dtype=np.float32, d=D_F32, env={'RRI_ONCHIP': '0', 'RRI_TROW_SMALL': '0'}),
    'gram-early-u8': dict(kind='plain', dtype=np.uint8, d=D_F32, env={'RRI_ONCHIP': '0', 'RRI_TROW_SMALL': '0'}),
}
NEW_FLAVOURS = ['gram-frozen', 'gram-frozen-fp32', 'csr-frozen', 'csr-uniform']
EARLY_FLAVOURS = ['gram-early', 'gram-early-fp32', 'gram-early-u8']
RANDOM_FLAVOURS = [f for f in FLAVOURS if not f.endswith('-bind')]
DIRECTED_ONLY = ['bind_mask']        # operations that no random alphabet has: bind_mask_device refuses the odd d of the weighted flavours
WEIGHTED_KINDS = ('weighted', 'pattern')

STATE, LOOK = 'state', 'look'       # an operation changes the handle's state, or borrows / observes
_COMMON = ['sweep', 'set_params', 'set_W', 'set_T', 'reset', 'project_W', 'snapshot', 'rollback']
_HALVES = ['update_T_row', 'update_W_col']
ALPHABET = {
    'plain': _COMMON + _HALVES + ['upload_X', 'scale_X', 'preprocess',
                                  'X_times', 'Xt_times', 'range_finder', 'colcounts', 'bench_rank1', 'bench_copy',
                                  'objective', 'objective_parts'],
    'residual': _COMMON + _HALVES + ['upload_X', 'scale_X', 'preprocess', 'residual_update',
                                     'X_times', 'Xt_times', 'range_finder', 'colcounts', 'bench_rank1', 'bench_copy',
                                     'objective', 'objective_parts', 'residual_check'],
    'weighted': _COMMON + ['upload_X', 'upload_mask', 'upload_mask_pattern',
                           'X_times', 'Xt_times', 'range_finder', 'bench_copy', 'objective', 'objective_parts'],
    'pattern': _COMMON + ['upload_observed', 'X_times', 'Xt_times', 'sparse_range_finder', 'objective', 'objective_parts'],
    'csr': _COMMON + _HALVES + ['upload_X_csr', 'preprocess_csr',
                                'X_times', 'Xt_times', 'sparse_range_finder', 'objective', 'objective_parts'],
}
FROZEN_OPS = ['set_frozen', 'clear_frozen', 'absorb', 'get_frozen']
UNIFORM_OPS = ['set_uniform_rows', 'preprocess_csr_uniform']
# the evaluation calls, which promise to write nothing a later sweep reads (rri_hip.h), and the two that score a live DeviceCorpus
BORROWERS = ['topn_rows', 'rank_entries', 'entries_loglik', 'cooccurrence_counts', 'masked_rmse', 'argmax_rows']
CORPUS_BORROWERS = ['corpus_loglik', 'corpus_cooc']
# absorb is a LOOK for W and T and a state change for the statistics; get_frozen observes
LOOKS = {'X_times', 'Xt_times', 'range_finder', 'sparse_range_finder', 'colcounts', 'bench_rank1', 'bench_copy',
         'residual_update', 'objective', 'objective_parts', 'residual_check', 'absorb', 'get_frozen'} | set(BORROWERS) | set(CORPUS_BORROWERS)


def alphabet(flavour):
    f = FLAVOURS[flavour]
    ops = list(ALPHABET[f['kind']])
    if f['dtype'] == np.float32:
        # scale_X rewrites a float32 X in place: a second rounding whose order the model would have to mirror; the float64
        # flavours own it.  In exchange this flavour's d lets it bind
        ops = [o for o in ops if o not in ('scale_X', 'preprocess')] + ['bind_X']
    if f['dtype'] == np.uint8:
        # the two bandwidth probes are refused on this store (they write an X-sized buffer of the storage type); scale_X and
        # preprocess write the scale vectors only, so nothing is rounded twice and they stay, also on a bound X
        ops = [o for o in ops if o not in ('bench_rank1', 'bench_copy')] + ['bind_X', 'set_X_scales']
    return ops + new_ops(flavour) + (BORROWERS + (CORPUS_BORROWERS if f['kind'] == 'csr' else []) if flavour in NEW_FLAVOURS + EARLY_FLAVOURS else [])


def early_schedule(pname):
    """does a handle of an EARLY_FLAVOURS flavour take the early-sums schedule under these parameters (LK::early_ok: both factors
    free, no projection of T)?"""
    p = PARAMS[pname]
    return not (p.get('fix_T') or p.get('fix_W') or p.get('project_T_each_iter'))


def early_sweeps(ops, raises=None):
    """how many sweep() calls of ops run on the early-sums schedule: each takes k_wfin at least once (every W half whose T half ran
    in the same call), so layout_info()['early_steps'] must be positive after a sequence that holds one"""
    ls, count = LegalState('plain'), 0
    for i, op in enumerate(ops):
        if op.name == 'sweep' and early_schedule(ls.pname) and i != raises:
            count += 1
        ls.follow(op)
    return count


def new_ops(flavour):
    """the operations on the state that only the new flavours hold: draw_sequence takes one of them every other time it could
    right behind a sweep or an objective, and a sweep or an objective right behind one of them"""
    f = FLAVOURS[flavour]
    return (FROZEN_OPS if f.get('frozen') else []) + (UNIFORM_OPS if f.get('uniform') else []) + (['upload_X_corpus'] if f.get('corpus') else [])


def is_counts(flavour):
    return FLAVOURS[flavour]['dtype'] == np.uint8


def category(name):
    return LOOK if name in LOOKS else STATE


# ---- coverage: every function of rri_hip.hip that calls changed(), and who reaches it here ---------------------------------
# value: the operations of ALPHABET (or 'bind_X') that reach it, or ('excluded', reason)
COVERAGE = {
    # the steps of the schedule and the end of a run: every sweep and half step
    'enqueue_T_half': ['sweep', 'update_T_row'],
    'enqueue_W_half': ['sweep', 'update_W_col'],
    'enqueue_rT_half': ['sweep', 'update_T_row'],
    'enqueue_rW_half': ['sweep', 'update_W_col'],
    'enqueue_wT_solve': ['sweep'],
    'enqueue_wW_half': ['sweep'],
    'enqueue_wsweep': ['sweep'],
    'enqueue_onchip': ['sweep'],
    'read_state': ['sweep'],
    'status_from_halt': ['sweep'],
    'run_and_collect': ['sweep'],
    'reset_applied': ['reset'],
    # entry points
    'rri_upload_X': ['upload_X'],
    'rri_upload_mask': ['upload_mask'],
    'rri_upload_X_csr': ['upload_X_csr'],
    'upload_X_csr_kept': ['upload_X_csr'],
    'rri_upload_mask_csr_pattern': ['upload_mask_pattern'],
    'rri_upload_observed_csr': ['upload_observed'],
    'rri_bind_X_device': ['bind_X'],
    'rri_set_W': ['set_W'],
    'rri_set_T': ['set_T'],
    'rri_set_params': ['set_params'],
    'rri_project_W_rows': ['project_W'],
    'rri_rollback': ['rollback'],
    'rri_residual_update': ['residual_update'],
    'rri_Xt_times': ['Xt_times'],
    'rri_range_finder': ['range_finder'],
    'rri_column_positive_counts': ['colcounts'],
    'rri_scale_X': ['scale_X', 'preprocess'],
    'rri_csr_scale_X': ['preprocess_csr'],
    'rri_bench_rank1_update': ['bench_rank1'],
    'rri_bind_mask_device': ['bind_mask'],
    'rri_bind_reduce_buffer': ('excluded', 'the sharded and group tests own it'),
    'rri_topic_finish': ('excluded', 'topic_* and reduce_*: the sharded and group tests own them'),
    'rri_attach_comm': ('excluded', 'attach_group: the sharded and group tests own it'),
}
# entry points that call no changed() themselves and are in the alphabet all the same (they borrow, observe or copy)
NO_CHANGED = {'rri_X_times': 'X_times', 'rri_sparse_range_finder': 'sparse_range_finder', 'rri_bench_stream_copy': 'bench_copy',
              'rri_snapshot': 'snapshot', 'rri_objective': 'objective', 'rri_objective_parts': 'objective_parts',
              'rri_residual_rebuild': 'residual_check', 'rri_update_T_row': 'update_T_row', 'rri_update_W_col': 'update_W_col',
              'rri_apply_reset_vectors': 'reset', 'rri_sweep': 'sweep', 'rri_csr_column_positive_counts': 'preprocess_csr',
              # drops what the handle computed from X through rri_scale_X(c, nullptr, 0), not by a changed() of its own
              'rri_set_X_scales': 'set_X_scales',
              # reach changed(c, CH_X) through rri_csr_scale_X, where they leave a request (uni_req); the list and the value are
              # written after that changed() has run
              'rri_set_uniform_rows': 'set_uniform_rows', 'rri_csr_scale_X_uniform': 'preprocess_csr_uniform',
              'rri_upload_X_corpus': 'upload_X_corpus',         # through upload_X_csr_kept
              # call none on purpose: the statistics are read where a step uses them
              'rri_frozen_set': 'set_frozen', 'rri_frozen_get': 'get_frozen', 'rri_frozen_absorb': 'absorb',
              # the evaluation calls: "write nothing a later sweep reads"
              'rri_topn_rows': 'topn_rows', 'rri_rank_entries': 'rank_entries', 'rri_cooccurrence_counts': 'cooccurrence_counts',
              'rri_entries_loglik': 'entries_loglik', 'rri_masked_rmse': 'masked_rmse', 'rri_argmax_rows': 'argmax_rows',
              'rri_corpus_entries_loglik': 'corpus_loglik', 'rri_corpus_cooccurrence_counts': 'corpus_cooc',
              'rri_get_residual': 'residual_check'}
# every other `rri_status rri_*(` of include/rri_hip.h, and why no sequence calls it (test_cached_state_cases_cpu.py parses the
# header: a new entry point fails there until it stands in COVERAGE, NO_CHANGED or here)
EXCLUDED_ENTRY_POINTS = {
    'rri_create': 'lifetime: every sequence starts from one', 'rri_destroy': 'lifetime: every sequence ends in one',
    'rri_get_W': 'pure getter: run_sequence reads W before and after every operation',
    'rri_get_T': 'pure getter: run_sequence reads T before and after every operation',
    'rri_get_X_scales': 'pure getter of the uint8 scale vectors', 'rri_get_uniform_rows': 'pure getter: copies the list out',
    'rri_storage_error': 'pure getter of what the float16 / uint8 upload measured',
    'rri_sparse_store_get': 'diagnostics: copies a blocked store out (the corpus test of test_cached_state_gpu.py reads it)',
    'rri_resume': 'a paused run: resets are off in every sequence (test_fuzz_gpu.py, test_edge_cases_gpu.py own them)',
    'rri_pending_event': 'a paused run: resets are off in every sequence',
    'rri_apply_reset_max_resid': 'a paused run: no engine wrapper outside one',
    'rri_skip_reset': 'a paused run: resets are off in every sequence',
    'rri_corpus_create': 'lifetime of a DeviceCorpus, which belongs to no handle',
    'rri_corpus_destroy': 'lifetime of a DeviceCorpus, which belongs to no handle',
    'rri_corpus_info': 'pure getter of a DeviceCorpus', 'rri_corpus_get': 'pure getter of a DeviceCorpus (to_scipy)',
    'rri_corpus_memory': 'pure getter: counts the corpora of the process',
    'rri_comm_unique_id': 'communicator: the sharded and group tests own it', 'rri_comm_create': 'communicator: the sharded and group tests own it',
    'rri_comm_create_host': 'communicator: the sharded and group tests own it', 'rri_comm_destroy': 'communicator: the sharded and group tests own it',
    'rri_comm_broadcast': 'communicator: a no-op without one', 'rri_comm_allreduce_sum': 'communicator: a no-op without one',
    'rri_comm_stats': 'communicator: pure getter',
    'rri_reduce_buffer': 'sharded stepping: the sharded and group tests own it', 'rri_topic_reduce_local': 'sharded stepping: the sharded and group tests own it',
    'rri_reduce_read': 'sharded stepping: the sharded and group tests own it', 'rri_reduce_write': 'sharded stepping: the sharded and group tests own it',
    'rri_topic_finish_w': 'sharded stepping: the sharded and group tests own it', 'rri_resid_row_argmax': 'sharded reset: the sharded tests own it',
    'rri_reset_row': 'sharded reset: the sharded tests own it', 'rri_poll': 'sharded stepping: status word of an interrupted step',
    'rri_timing_enable': 'timing: changes no result', 'rri_timing_read': 'timing: pure getter', 'rri_synchronize': 'timing: drains the stream',
    'rri_onchip_info': 'diagnostics: run_sequence reads it on the RRI_ONCHIP=1 flavours', 'rri_onchip_fallbacks': 'diagnostics: pure getter',
    'rri_layout_info': 'diagnostics: pure getter', 'rri_device_memory': 'diagnostics: pure getter', 'rri_debug_xcc': 'diagnostics: a probe kernel of its own',
    'rri_sweep_until': 'out of scope here: test_onchip_gpu.py owns it, and it is refused while statistics are set',
}
EXCLUDED_METHODS = {'attach_group': 'the sharded and group tests own it', 'bind_reduce_buffer': 'the sharded and group tests own it',
                    'topic_reduce_local': 'sharded', 'topic_finish': 'sharded', 'topic_finish_w': 'sharded',
                    'reduce_read': 'sharded', 'reduce_write': 'sharded', 'reduce_buffer': 'sharded',
                    'apply_reset_max_resid': 'no wrapper outside a paused run (rri_apply_reset_max_resid)',
                    # every other public method that calls the library on the handle (the header-driven check)
                    'close': 'lifetime', 'get_W': 'pure getter', 'get_T': 'pure getter', 'X_scales': 'pure getter', 'uniform_rows': 'pure getter',
                    'storage_relerr': 'pure getter', 'sparse_store': 'diagnostics', 'comm_broadcast': 'communicator', 'comm_sum': 'communicator',
                    'comm_stats': 'communicator', 'poll': 'sharded', 'pending_event': 'a paused run', 'resid_row_argmax': 'sharded',
                    'reset_row': 'sharded', 'topic_sums': 'sharded', 'sweep_with_T_noise': 'sharded stepping', 'sweep_stepwise': 'sharded stepping',
                    'timing_enable': 'timing', 'timing_read': 'timing', 'synchronize': 'timing', 'onchip_info': 'diagnostics',
                    'onchip_fallbacks': 'diagnostics', 'layout_info': 'diagnostics', 'debug_xcc': 'diagnostics',
                    'sweep_until': 'out of scope: test_onchip_gpu.py owns it', 'begin_run': 'a paused run', 't_norms': 'pure getter'}
# operation -> the RRIEngine methods it calls (checked against engine.py)
OP_METHODS = {
    'sweep': ['sweep'], 'set_params': ['set_params', 'set_T'], 'set_W': ['set_W'], 'set_T': ['set_T'], 'reset': ['apply_reset_vectors'],
    'project_W': ['project_W_rows'], 'snapshot': ['snapshot'], 'rollback': ['rollback'], 'update_T_row': ['update_T_row'],
    'update_W_col': ['update_W_col'], 'upload_X': ['upload_X'], 'scale_X': ['scale_X'], 'preprocess': ['preprocess', 'set_W'],
    'bind_X': ['bind_X_device'], 'bind_mask': ['bind_mask_device'], 'upload_X_csr': ['upload_X_csr'], 'preprocess_csr': ['_preprocess_csr', 'set_W'],
    'upload_mask': ['upload_mask'], 'upload_mask_pattern': ['upload_mask_csr_pattern'], 'upload_observed': ['upload_observed_csr'],
    'X_times': ['X_times'], 'Xt_times': ['Xt_times'], 'range_finder': ['range_finder'], 'sparse_range_finder': ['sparse_range_finder'],
    'colcounts': ['column_positive_counts'], 'bench_rank1': ['bench_rank1_update'], 'bench_copy': ['bench_stream_copy'],
    'residual_update': ['residual_update'], 'objective': ['objective'], 'objective_parts': ['objective_parts'],
    'residual_check': ['residual_rebuild', 'get_residual'], 'set_X_scales': ['set_X_scales'],
    'set_frozen': ['set_frozen'], 'clear_frozen': ['clear_frozen'], 'absorb': ['absorb', 'get_frozen'], 'get_frozen': ['get_frozen'],
    'set_uniform_rows': ['set_uniform_rows'], 'preprocess_csr_uniform': ['preprocess', 'set_W'], 'upload_X_corpus': ['upload_X_corpus'],
    'topn_rows': ['topn_rows'], 'rank_entries': ['rank_entries'], 'entries_loglik': ['entries_loglik'],
    'cooccurrence_counts': ['cooccurrence_counts'], 'masked_rmse': ['masked_rmse'], 'argmax_rows': ['argmax_rows'],
    'corpus_loglik': ['entries_loglik'], 'corpus_cooc': ['cooccurrence_counts'],
}


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def stored(X, dtype):
    return np.ascontiguousarray(np.asarray(X, dtype=dtype).astype(np.float64))


def _sparse_ish(X, salt):
    """an X with zeros (a document-term matrix has them): 35 % of the entries kept"""
    return X * (np.random.RandomState(1000 + salt).rand(*X.shape) < 0.35)


def counts_of(X):
    """term counts 0..255 of a non-negative X with zeros, in float64: the positive entries 40 on average, clipped at 255"""
    return np.minimum(np.round(40.0 * X / X[X > 0].mean()), 255.0)


def x_scales(d, salt):
    """(row_scale or None, col_scale or None) of set_X_scales(salt): the row vector only, the column vector only, or both, drawn
    from 10^U(-1, 1)"""
    rs = np.random.RandomState(10000 + salt)
    r, s = 10.0 ** rs.uniform(-1, 1, N), 10.0 ** rs.uniform(-1, 1, d)
    return (r, None, r)[salt % 3], (None, s, s)[salt % 3]


def other_X(d, salt, dtype, sparse):
    """another X of the same family; three salts in four give one with zeros, as do the kinds whose X is sparse; for the uint8
    store counts, always with zeros"""
    X = planted_X(N, d, K, seed=15 + salt % ZERO_ROWS, dtype=np.float64)
    if dtype == np.uint8:
        return counts_of(_sparse_ish(X, salt))
    if sparse or salt % 4:
        X = _sparse_ish(X, salt % ZERO_ROWS)
    if salt >= ZERO_ROWS:
        X[zero_rows_of(salt), :] = 0.0
        X[LONE_TERM_ROW, :] = 0.0
        X[LONE_TERM_ROW, 0] = 1.0
        X[:, 0] = np.where(X.sum(1) > 0, np.maximum(X[:, 0], 0.5), 0.0)
    return stored(X, dtype)


# a salt of ZERO_ROWS or more (sparse kinds, the flavours with uniform rows): the X of salt - ZERO_ROWS with three empty rows, and
# one row made only of term 0, which every document that is not empty holds.  (With empty rows no term is in EVERY document: the
# idf of term 0 is log(n / (n - 3)), small and not 0, and that row stays an ordinary row of one entry.)
ZERO_ROWS = 100
LONE_TERM_ROW = 11


def zero_rows_of(salt):
    return np.sort(np.random.RandomState(13000 + salt).choice(np.arange(20, N), size=3, replace=False))


N_O = 41        # the planted rows behind a set of frozen statistics: N_O of test_frozen_gpu.py


def frozen_stats(flavour, salt):
    """(B, A, s, c) = frozen_cases.stats_of(Xo, Wo) of N_O planted rows drawn per salt, at the scale of the flavour's X (for a
    CSR flavour with its zeros) and as the flavour stores them.  salt 'dead': column K - 1 of Wo scaled by 1e-9, so that under
    the penalties 'pen_a' the T row of a topic whose own column of W is zero comes out 0 and the column stays 0 -- alive only by
    s[K - 1] > 0.  frozen_cases.frozen_sweep asserts on a T row that sums to 0 (it is for inputs that meet no reset); for these
    statistics alone the model sweeps with frozen_cases.Stacked on the rows themselves, which has the reference's rule"""
    import frozen_cases as fc
    return fc.stats_of(*frozen_rows(flavour, salt))


def frozen_rows(flavour, salt):
    """(Xo, Wo) behind frozen_stats"""
    f = FLAVOURS[flavour]
    dead, salt = salt == 'dead', 7 if salt == 'dead' else salt
    Xo = planted_X(N_O, f['d'], K, seed=400 + salt, dtype=np.float64)
    Wo = scaled_init(Xo, K, seed=500 + salt)[0] * (0.5 + np.random.RandomState(600 + salt).rand(N_O, K))
    if f['kind'] == 'csr':
        Xo = Xo * (np.random.RandomState(700 + salt).rand(*Xo.shape) < 0.35)
    if dead:
        Wo[:, K - 1] *= 1e-9
    return stored(Xo, f['dtype']), Wo


def uniform_list(salt):
    """(rows, unsorted; factor of the value) of set_uniform_rows(salt): 4 .. 11 distinct rows, the value factor * mean(X)"""
    rs = np.random.RandomState(11000 + salt)
    return rs.permutation(N)[:int(rs.randint(4, 12))].astype(np.int64), 0.5 + 2.0 * rs.rand()


_CORPUS = {}


def corpus_raw(d, salt):
    """(indptr, indices, values, shape), (X dense, canonical) of upload_X_corpus(salt): corpus_cases.raw_rows -- shuffled rows,
    every third row with duplicated columns, one entry in twenty an explicit zero -- with the values made positive (an NMF's X) and
    scaled by a power of two to the size of planted_X, so that the sums of duplicates stay exact"""
    if (d, salt) not in _CORPUS:
        import corpus_cases as cc
        rs = np.random.RandomState(12000 + salt)
        lengths = rs.randint(40, 160, size=N)
        dup = np.arange(N) % 3 == 0
        parts = {True: cc.raw_rows(lengths[dup], d, 12100 + salt, duplicated=1.0 / 3, zeros=0.05),
                 False: cc.raw_rows(lengths[~dup], d, 12200 + salt, duplicated=0.0, zeros=0.05)}
        at = {True: 0, False: 0}
        cols, vals = [], []
        for r in range(N):
            ptr, idx, val, _ = parts[bool(dup[r])]
            q = at[bool(dup[r])]
            cols.append(idx[ptr[q]:ptr[q + 1]]), vals.append(np.abs(val[ptr[q]:ptr[q + 1]]) / 64.0)
            at[bool(dup[r])] += 1
        indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        raw = (indptr, np.concatenate(cols).astype(np.int64), np.concatenate(vals), (N, d))
        cptr, cidx, cval, st = cc.canonical(*raw)
        assert st['duplicates_merged'] > 0 and st['zeros_dropped'] > 0 and st['rows_rewritten'] > N // 2 and st['negatives'] == 0
        _CORPUS[(d, salt)] = raw, sp.csr_matrix((cval, cidx, cptr), shape=(N, d))
    raw, A = _CORPUS[(d, salt)]
    return raw, A


def weights(d, salt):
    """a dense mask: half the entries observed, with weights in [0.5, 1.5)"""
    rs = np.random.RandomState(2000 + salt)
    return (rs.rand(N, d) < 0.5) * (0.5 + rs.rand(N, d))


def pattern(d, salt):
    return (np.random.RandomState(3000 + salt).rand(N, d) < 0.4).astype(np.float64)


def observed_csr(X, Mp):
    """the CSR matrix whose stored entries are the pattern Mp (explicit zeros kept) with X's values"""
    I, J = np.nonzero(Mp)
    return sp.csr_matrix((X[I, J], (I, J)), shape=X.shape)


def start(flavour):
    """(X as the handle stores it, M or None, W0, T0) of a flavour"""
    f = FLAVOURS[flavour]
    d, kind = f['d'], f['kind']
    X = planted_X(N, d, K, seed=5, dtype=np.float64)
    if f['dtype'] == np.uint8:
        X = counts_of(_sparse_ish(X, 0))
    W0, T0 = scaled_init(X, K, seed=6)
    M = None
    if kind == 'csr':
        X = _sparse_ish(X, 0)
    elif kind == 'weighted':
        M = weights(d, 0)
    elif kind == 'pattern':
        M = pattern(d, 0)
        X = X * M
    return stored(X, f['dtype']), M, W0, T0


def new_W(W0, salt):
    return W0 * (0.5 + np.random.RandomState(4000 + salt).rand(*W0.shape))


def t_row_total(T0, pname):
    """what the rows of a T written from outside sum to: 1 under 'simplex' (see the docstring), else what T0's rows do"""
    return 1.0 if pname == 'simplex' else float(T0.sum(1).mean())


def new_T(T0, salt, pname):
    T = T0 * (0.5 + np.random.RandomState(5000 + salt).rand(*T0.shape))
    return T / T.sum(1, keepdims=True) * t_row_total(T0, pname)


def reset_vectors(W0, T0, salt, pname):
    rs = np.random.RandomState(6000 + salt)
    row = rs.rand(T0.shape[1])
    return int(rs.randint(K)), row / row.sum() * t_row_total(T0, pname), 2.0 * W0.mean() * rs.rand(N)


# ---- the model -------------------------------------------------------------------------------------------------------------
class Op(object):
    def __init__(self, name, arg=None):
        self.name, self.arg = name, arg

    def __repr__(self):
        return self.name if self.arg is None else '%s(%s)' % (self.name, self.arg)


class LegalState(object):
    """What the next draw and the bounds may depend on, cheap to follow without running the oracle: the generator follows it
    alone, the model follows it next to its arrays (Model.apply), so there is one copy of these rules."""

    def __init__(self, kind, counts=False, flavour=None):
        self.pname = 'free'
        self.has_F = False                  # frozen statistics are set
        # uniform rows (CSR): the list, and the rows of the stored part whose total is zero -- emptied by a list that has been
        # replaced or cleared, or uploaded so (other_X, salts from ZERO_ROWS)
        self.U = frozenset(int(r) for r in uniform_list(0)[0]) if flavour and FLAVOURS[flavour].get('uniform') else frozenset()
        self.Z = frozenset()
        self.has_snap = False
        self.counts = counts                # a uint8 store: X always has zeros, and a bound X is rescaled like any other
        self.x_bound = False                # X is bound caller memory: rri_scale_X refuses it, unless it writes scale vectors only
        self.x_has_zeros = kind == 'csr' or counts    # preprocess needs an X with zeros (see the module docstring)
        self.t_feasible = False             # the rows of T sum to 1
        self.snap_feasible = False
        # could the cross terms of a whole sweep be valid (xy_valid)?  Only if the last operation that changed the state was a
        # sweep with W free: note_xy wants the W halves of topics 0 .. k-1 in order, and every write from outside, every lone
        # half step and every new X drops them.  Where this is False the objective comes from the residual
        self.xy_possible = False

    def legal(self, op):
        n, p = op.name, PARAMS[self.pname]
        if n == 'rollback':
            return self.has_snap and (self.pname != 'simplex' or self.snap_feasible)
        if n == 'update_T_row':
            return not p.get('fix_T')
        if n == 'update_W_col':
            return not p.get('fix_W')
        if n in ('scale_X', 'preprocess') and self.x_bound and not self.counts:
            return False
        if n == 'preprocess':
            return self.x_has_zeros
        if n == 'set_params':
            return op.arg != self.pname and not (self.has_F and PARAMS[op.arg].get('fix_W'))
        if n in ('set_frozen', 'absorb'):
            return not p.get('fix_W') and not self.U
        if n in ('get_frozen', 'clear_frozen'):
            return self.has_F
        if n == 'preprocess_csr':
            return not self.U and not self.Z        # ZeroTotalRows, or a second preprocessing of an X with uniform rows
        if n == 'preprocess_csr_uniform':
            return not self.U and bool(self.Z) and not self.has_F
        if n == 'set_uniform_rows':                 # salt % 3: another list, another value only, a clear
            return (bool(self.U) or op.arg % 3 == 0) and not self.has_F
        return True

    def follow(self, op):
        n, a, p = op.name, op.arg, PARAMS[self.pname]
        if category(n) == STATE and n not in ('snapshot', 'set_params', 'set_frozen', 'clear_frozen'):
            self.xy_possible = n == 'sweep' and not p.get('fix_W')
        if n == 'sweep' and not p.get('fix_T'):
            self.t_feasible = self.pname == 'simplex'
        elif n == 'set_params':
            self.pname = a
            if a == 'simplex':
                self.t_feasible = True
        elif n == 'set_T':
            self.t_feasible = self.pname == 'simplex'
        elif n == 'snapshot':
            self.has_snap, self.snap_feasible = True, self.t_feasible
        elif n == 'rollback':
            self.t_feasible = self.snap_feasible
        elif n == 'update_T_row' and self.pname != 'simplex':
            self.t_feasible = False
        elif n in ('upload_X', 'bind_X'):
            self.x_bound = n == 'bind_X'
            self.x_has_zeros = bool(a % 4) or self.counts          # other_X
        elif n in ('set_frozen', 'absorb'):
            self.has_F = True
        elif n == 'clear_frozen':
            self.has_F = False
        elif n in ('upload_X_csr', 'upload_X_corpus'):
            self.U = frozenset()
            self.Z = frozenset(int(r) for r in zero_rows_of(a)) if n == 'upload_X_csr' and a >= ZERO_ROWS else frozenset()
        elif n in UNIFORM_OPS and self.has_F:
            pass                            # refused, nothing changes
        elif n == 'preprocess_csr_uniform':
            self.U, self.Z = self.Z, frozenset()
        elif n == 'set_uniform_rows':
            new = self.U if a % 3 == 1 else frozenset() if a % 3 == 2 else frozenset(int(r) for r in uniform_list(a)[0])
            self.U, self.Z = new, (self.Z | self.U) - new


class Model(object):
    """X, M, W, T, params, snapshot: nothing cached.  apply(op) returns what the handle must answer (or None) and moves the
    model's W and T to what the handle must hold afterwards."""

    def __init__(self, flavour):
        self.flavour = flavour
        self.f = FLAVOURS[flavour]
        self.kind, self.d, self.dtype = self.f['kind'], self.f['d'], self.f['dtype']
        self.X, self.M, self.W0, self.T0 = start(flavour)
        self.W, self.T = self.W0.copy(), self.T0.copy()
        self.counts = is_counts(flavour)
        if self.counts:         # X = (C * s) * r[:, None]; upload_X and bind_X put both vectors back to ones
            self.C, self.r, self.s = self.X, np.ones(N), np.ones(self.d)
        self.ls = LegalState(self.kind, self.counts, flavour)
        self.snap = None
        self.F = None               # frozen statistics (B, A, s, c)
        self.U, self.v = np.zeros(0, dtype=np.int64), 0.0       # uniform rows (sorted) and their value: X = S + v e_U 1^T, dense
        self.uni_arg = None         # what the last set_uniform_rows passed: (rows as given, unsorted; value)
        if self.f.get('uniform'):   # this flavour starts with a list
            self._set_uniform(0)
        self.skip_col = None        # column of W the last operation leaves to the next W half (update_T_row)

    @property
    def pname(self):
        return self.ls.pname

    @property
    def params(self):
        return PARAMS[self.pname]

    @property
    def regs(self):
        return {r: self.params.get(r, 0.0) for r in REGS}

    def weighted(self):
        return self.kind in WEIGHTED_KINDS

    def legal(self, op):
        return self.ls.legal(op)

    # -- the operations --
    def _set_uniform(self, salt):
        """set_uniform_rows(salt): salt % 3 == 0 another list (and value), 1 another value for the list as it is, 2 a clear.  The
        rows of the list that is replaced stay rows of zeros"""
        rows, factor = uniform_list(salt)
        rows = self.U[np.random.RandomState(salt).permutation(self.U.size)] if salt % 3 == 1 else rows[:0] if salt % 3 == 2 else rows
        X = self.X.copy()
        X[self.U, :] = 0.0
        S_mean = float(X.mean())
        self.v = factor * S_mean if rows.size else 0.0
        X[rows, :] = self.v
        self.X, self.U, self.uni_arg = X, np.sort(rows), (rows, self.v)

    def sweep_from(self, X, M, W, T, sweeps, pname=None, F='own'):
        p = dict(PARAMS[self.pname if pname is None else pname])
        F = self.F if isinstance(F, str) else F
        if p.get('project_T_each_iter'):
            P = oracle().proj_rows_simplex(T.copy(), p['t_row_sum'])
            assert np.abs(P - T).max() <= 1e-12, 'the model was given a T off the simplex under project_T_each_iter'
        if F is not None and not p.get('fix_T'):    # the stacked problem, from the statistics (a sweep with T fixed ignores them)
            import frozen_cases as fc
            assert not p.get('fix_W')
            if np.array_equal(F[2], frozen_stats(self.flavour, 'dead')[2]):
                Xo, Wo = frozen_rows(self.flavour, 'dead')
                return fc.Stacked(Xo, Wo, X, W, T, **{key: val for key, val in p.items() if not key.startswith('fix_')}).sweep(sweeps)
            return fc.frozen_sweep(F[0], F[1], F[2], X, W, T, n_sweeps=sweeps, **p)
        out = oracle().nmf(X, K, W_mat=M, W_in=W.copy(), T_in=T.copy(), max_iter=sweeps, eps_stop=-1, do_final_project_W=False,
                           reset_topic_method=None, **p)
        assert out['n_resets_used'] == 0
        return out['W'], out['T']

    def objective_at(self, X, M, W, T, regs=None, F='own'):
        F = self.F if isinstance(F, str) else F
        share = 0.0 if F is None else 0.5 * ((F[3] - 2.0 * float((F[0] * T).sum())) + float((F[1] * T.dot(T.T)).sum()))
        return float(oracle().true_objective(X, W, T, Wm=M, **(self.regs if regs is None else regs))) + share

    def half_T(self, t):
        o, p = oracle(), self.params
        wR, nw = o.residual_products_T(self.X, self.W, self.T, t)
        if self.F is not None:
            others = np.arange(K) != t
            wR, nw = wR + self.F[0][t] - self.F[1][t, others].dot(self.T[others]), nw + self.F[1][t, t]
        s = p.get('t_row_sum') if p.get('project_T_each_iter') else None
        row = o.qf_min(-(wR - self.regs['reg_t_l1']), nw + self.regs['reg_t_l2'], s=s, ub=p.get('t_row_sum'))[0]
        if s and abs(row.sum() - s) > 1e-15:
            row = o.proj_simplex(row, s=s)                 # nmf.py:757-761
        return row

    def half_W(self, t):
        o = oracle()
        Rt, nt = o.residual_products_W(self.X, self.W, self.T, t)
        return o.qf_min(-(Rt - self.regs['reg_w_l1']), nt + self.regs['reg_w_l2'], s=None, ub=None)[0]

    def apply(self, op):
        want = self._apply(op)
        self.ls.follow(op)
        if op.name in ('upload_X', 'bind_X'):
            assert self.ls.x_has_zeros == bool((self.X == 0).any())
        if self.kind == 'csr':      # the generator's copy of the list and of the zero-total rows is the model's
            assert self.ls.U == frozenset(self.U.tolist()) and self.ls.has_F == (self.F is not None), op
            assert self.ls.Z == frozenset(np.flatnonzero(self.X.sum(1) == 0).tolist()), (op, self.ls.Z)
            assert self.U.size == 0 or (self.X[self.U] == self.v).all()
        return want

    def _apply(self, op):
        n, a = op.name, op.arg
        self.skip_col = None
        self.X_before = self.X
        if n == 'sweep':
            self.W, self.T = self.sweep_from(self.X, self.M, self.W, self.T, a)
        elif n == 'set_params':
            if a == 'simplex':
                self.T = oracle().proj_rows_simplex(self.T.copy(), 1.0)
        elif n == 'set_W':
            self.W = new_W(self.W0, a)
        elif n == 'zero_W_column':
            self.W = zero_column_W(self.W0, a)
        elif n == 'set_T':
            self.T = new_T(self.T0, a, self.pname)
        elif n == 'reset':
            t, row, col = reset_vectors(self.W0, self.T0, a, self.pname)
            self.T = self.T.copy()
            self.W = self.W.copy()
            self.T[t, :] = row
            self.W[:, t] = col
            if self.F is not None:      # W[:, t] = 0 on the rows that are not there
                B, A, s = self.F[0].copy(), self.F[1].copy(), self.F[2].copy()
                B[t, :], A[t, :], A[:, t], s[t] = 0.0, 0.0, 0.0, 0.0
                self.F = (B, A, s, self.F[3])
        elif n == 'project_W':
            self.W = oracle().proj_rows_simplex(self.W.copy(), float(a))
        elif n == 'snapshot':
            self.snap = (self.W.copy(), self.T.copy())
        elif n == 'rollback':
            self.W, self.T = self.snap[0].copy(), self.snap[1].copy()
        elif n == 'update_T_row':
            row = self.half_T(a)
            self.T = self.T.copy()
            self.T[a, :] = row
            self.skip_col = a
        elif n == 'update_W_col':
            col = self.half_W(a)
            self.W = self.W.copy()
            self.W[:, a] = col
        elif n == 'set_frozen':
            self.F = frozen_stats(self.flavour, a)
        elif n == 'clear_frozen':
            self.F = None
        elif n == 'absorb':
            import frozen_cases as fc
            old = self.F if self.F is not None else (0.0, 0.0, 0.0, 0.0)
            self.F = tuple(a * o + g for o, g in zip(old, fc.stats_of(self.X, self.W)))
            return self.F
        elif n == 'get_frozen':
            return self.F
        elif n == 'set_uniform_rows':
            if self.F is not None:
                raise NotImplementedError('frozen statistics are set')
            self._set_uniform(a)
        elif n == 'upload_X_corpus':
            self.X = np.ascontiguousarray(corpus_raw(self.d, a)[1].toarray())
            self.U, self.v = self.U[:0], 0.0
        elif n in BORROWERS or n in CORPUS_BORROWERS:
            return None                 # check_value takes the reference from the model's W and T
        elif n in ('upload_X', 'bind_X', 'upload_X_csr'):
            self.X = other_X(self.d, a, self.dtype, sparse=self.kind == 'csr')
            self.U, self.v = self.U[:0], 0.0
            if self.counts:
                self.C, self.r, self.s = self.X, np.ones(N), np.ones(self.d)
        elif n == 'set_X_scales':
            r, s = x_scales(self.d, a)
            self.r, self.s = self.r if r is None else r, self.s if s is None else s
            self.X = scaled_counts(self.C, self.r, self.s)
        elif n == 'scale_X':
            if self.counts:
                self.s = self.s * col_scale(self.d, a)
                self.X = scaled_counts(self.C, self.r, self.s)
            else:
                self.X = self.X * col_scale(self.d, a)
        elif n in ('preprocess', 'preprocess_csr', 'preprocess_csr_uniform'):
            if n == 'preprocess_csr_uniform':       # the oracle's normalize writes the dense row 1 / d itself (matrixops.py:143-147)
                assert self.U.size == 0
                if self.F is not None:
                    raise NotImplementedError('frozen statistics are set')
                self.U, self.v = np.array(sorted(self.ls.Z), dtype=np.int64), 1.0 / self.d
            before = float(self.X.mean())
            Xt = oracle().tfidf(self.X)
            if self.counts:     # what the two vectors hold afterwards; X itself is the oracle's, as for every other store
                idf = np.asarray(oracle().tfidf(self.X, return_idf=True)[1], dtype=np.float64).ravel()
                self.s, self.r = self.s * idf, self.r / (np.asarray(Xt.sum(1)).ravel() + np.spacing(1))
            self.X = oracle().normalize(Xt)
            self.W = self.W * (float(self.X.mean()) / before)
        elif n in ('upload_mask', 'bind_mask'):
            self.M = weights(self.d, a)
        elif n == 'upload_mask_pattern':
            self.M = pattern(self.d, a)
        elif n == 'upload_observed':
            self.M = pattern(self.d, a)
            self.X = planted_X(N, self.d, K, seed=15 + a, dtype=np.float64) * self.M
        elif n == 'X_times':
            return self.X.dot(operand(self.d, a))
        elif n == 'Xt_times':
            return self.X.T.dot(operand(N, a))
        elif n in ('range_finder', 'sparse_range_finder', 'bench_rank1', 'bench_copy', 'residual_update'):
            return None
        elif n == 'colcounts':
            return (self.X > 0).sum(0).astype(np.float64)
        elif n == 'objective':
            return self.objective_at(self.X, self.M, self.W, self.T)
        elif n == 'objective_parts':
            return [self.objective_at(self.X, self.M, self.W, self.T, regs={}), float((self.W ** 2).sum()), float(np.abs(self.W).sum())]
        elif n == 'residual_check':
            return self.X - self.W.dot(self.T)
        else:
            raise KeyError(n)
        return None

    def state(self):
        st = dict(X=self.X, M=self.M, W=self.W.copy(), T=self.T.copy(), pname=self.pname, F=self.F, U=self.U, v=self.v)
        if self.counts:
            st.update(C=self.C, r=self.r, s=self.s)
        return st


def scaled_counts(C, r, s):
    """the X of a uint8 handle, in the order its kernels multiply: (C * s) * r[:, None]"""
    return np.ascontiguousarray((C * s) * r[:, None])


def rescale_after_preprocess(X):
    """mean(preprocessed X) / mean(X): rows that sum to 1 are some fifty times smaller than planted_X's"""
    return float(oracle().normalize(oracle().tfidf(X)).mean()) / float(X.mean())


def col_scale(d, salt):
    return 0.5 + np.random.RandomState(7000 + salt).rand(d)


def operand(rows, salt, m=3):
    return np.random.RandomState(8000 + salt).randn(rows, m)


def update_vectors(d, salt):
    rs = np.random.RandomState(9000 + salt)
    return rs.rand(N), rs.rand(d), rs.rand(d), rs.rand(N)


# ---- the handle ------------------------------------------------------------------------------------------------------------
def make_engine(flavour):
    """a handle of the flavour with its X (and mask), W0, T0 and the free parameters; the caller has set FLAVOURS[..]['env']"""
    from rri_nmf_amd.engine import RRIEngine
    f = FLAVOURS[flavour]
    for key, val in f['env'].items():
        assert os.environ.get(key) == val, 'set %s=%s before the handle is created (rri_create reads it)' % (key, val)
    X, M, W0, T0 = start(flavour)
    kind = f['kind']
    kw = dict(dtype=f['dtype'])
    if kind == 'residual':
        kw['schedule'] = 'residual'
    elif kind == 'weighted':
        kw['weighted'] = True
    elif kind == 'pattern':
        kw['weighted'] = 'sparse'
    elif kind == 'csr':
        kw['sparse_x'] = True
    e = RRIEngine(N, f['d'], K, **kw)
    try:
        if kind == 'pattern':
            e.upload_observed_csr(observed_csr(X, M))
        elif kind == 'csr':
            e.upload_X_csr(sp.csr_matrix(X))
        else:
            e.upload_X(X.astype(f['dtype']))
            if kind == 'weighted':
                e.upload_mask(M)
        e.set_W(W0), e.set_T(T0)
        e.set_params(reset_topic_method=None)
        if f.get('uniform'):        # as Model.__init__
            e.set_uniform_rows(*Model(flavour).uni_arg)
    except Exception:
        e.close()
        raise
    e._cs_keep = []         # device memory bound to the handle stays alive with it
    return e


def apply_engine(e, m, op):
    """the operation on the handle; m is the model, which has the operation behind it (m.X_before: the X it had before)"""
    n, a = op.name, op.arg
    d, dt = m.d, m.dtype
    if n == 'sweep':
        return e.sweep(a)
    if n == 'set_params':
        e.set_params(reset_topic_method=None, **PARAMS[a])
        if a == 'simplex':      # as the driver enters a run (nmf.py:414-417)
            e.set_T(oracle().proj_rows_simplex(e.get_T(), 1.0))
        return None
    if n == 'set_W':
        return e.set_W(new_W(m.W0, a))
    if n == 'zero_W_column':
        return e.set_W(zero_column_W(m.W0, a))
    if n == 'set_T':
        return e.set_T(new_T(m.T0, a, m.pname))
    if n == 'reset':
        return e.apply_reset_vectors(*reset_vectors(m.W0, m.T0, a, m.pname))
    if n == 'project_W':
        return e.project_W_rows(float(a))
    if n in ('snapshot', 'rollback', 'update_T_row', 'update_W_col'):
        return getattr(e, n)(*(() if a is None else (a,)))
    if n == 'upload_X':
        return e.upload_X(other_X(d, a, dt, False).astype(dt))
    if n == 'bind_X':
        import torch
        t = torch.from_numpy(other_X(d, a, dt, False).astype(dt)).to('cuda:%d' % e.device).contiguous()
        torch.cuda.synchronize()
        e._cs_keep.append(t)
        return e.bind_X_device(t.data_ptr(), d)
    if n == 'upload_X_csr':
        return e.upload_X_csr(sp.csr_matrix(other_X(d, a, dt, True)))
    if n == 'upload_X_corpus':      # the corpus is closed at once: the handle keeps nothing of it (rri_hip.h)
        from rri_nmf_amd.engine import DeviceCorpus
        corpus = DeviceCorpus.from_arrays(*corpus_raw(d, a)[0], device=e.device)
        try:
            return e.upload_X_corpus(corpus)
        finally:
            corpus.close()
    if n == 'set_frozen':
        from rri_nmf_amd.engine import FrozenRows
        return e.set_frozen(FrozenRows(*frozen_stats(m.flavour, a), rows=N_O))
    if n == 'clear_frozen':
        return e.clear_frozen()
    if n == 'absorb':
        e.absorb(a)
        return e.get_frozen()
    if n == 'get_frozen':
        return e.get_frozen()
    if n == 'set_uniform_rows':
        rows, value = m.uni_arg if m.F is None else uniform_list(a)     # (refused while statistics are set: any list)
        return e.set_uniform_rows(rows, value)
    if n == 'preprocess_csr_uniform':
        W = e.get_W()
        idf = e.preprocess(tfidf=True, normalize=True, uniform_rows=True)
        e.set_W(W * rescale_after_preprocess(m.X_before))
        return idf
    if n in BORROWERS or n in CORPUS_BORROWERS:
        return borrow(e, m, n, a)
    if n == 'scale_X':
        return e.scale_X(col_scale(d, a))
    if n == 'set_X_scales':
        return e.set_X_scales(*x_scales(d, a))
    if n in ('preprocess', 'preprocess_csr'):
        W = e.get_W()
        idf = e.preprocess(tfidf=True, normalize=True) if n == 'preprocess' else e._preprocess_csr(True, True)
        e.set_W(W * rescale_after_preprocess(m.X_before))
        return idf
    if n == 'upload_mask':
        return e.upload_mask(weights(d, a))
    if n == 'bind_mask':
        import torch
        t = torch.from_numpy(np.ascontiguousarray(weights(d, a).astype(dt))).to('cuda:%d' % e.device).contiguous()
        torch.cuda.synchronize()
        e._cs_keep.append(t)
        return e.bind_mask_device(t.data_ptr(), d)
    if n == 'upload_mask_pattern':
        return e.upload_mask_csr_pattern(sp.csr_matrix(pattern(d, a)))
    if n == 'upload_observed':
        Mp = pattern(d, a)
        return e.upload_observed_csr(observed_csr(planted_X(N, d, K, seed=15 + a, dtype=np.float64) * Mp, Mp))
    if n == 'X_times':
        return e.X_times(operand(d, a))
    if n == 'Xt_times':
        return e.Xt_times(operand(N, a))
    if n == 'range_finder':
        Q, B = e.range_finder(operand(d, a, 4), 1)
        return Q, B
    if n == 'sparse_range_finder':
        Q, B = e.sparse_range_finder(operand(d, a, 4), 1)
        return Q, B
    if n == 'colcounts':
        return e.column_positive_counts()
    if n == 'bench_rank1':
        return e.bench_rank1_update(1)
    if n == 'bench_copy':
        return e.bench_stream_copy(1)
    if n == 'residual_update':
        return e.residual_update(*update_vectors(d, a))
    if n == 'objective':
        return e.objective()
    if n == 'objective_parts':
        return e.objective_parts()
    if n == 'residual_check':
        e.residual_rebuild()
        return e.get_residual(np.float64)
    raise KeyError(n)


# ---- the evaluation calls as borrowers: inputs per salt, the call, and the check of its answer against the CURRENT W and T ------
def borrow_inputs(name, d, salt, X=None):
    import cooc_cases as cc
    import loglik_cases as lc
    rs = np.random.RandomState(14000 + (salt or 0))
    rows = rs.randint(0, N, size=40).astype(np.int64)
    rows[-1] = rows[0]
    if name == 'topn_rows':
        return dict(rows=rows, n_top=10, exclude=sp.csr_matrix((rs.rand(40, d) < 0.2).astype(np.float64)))
    if name == 'rank_entries':
        return dict(rows=rows, targets=sp.csr_matrix((rs.rand(40, d) < 0.05).astype(np.float64)),
                    exclude=sp.csr_matrix((rs.rand(40, d) < 0.2).astype(np.float64)))
    if name in ('entries_loglik', 'corpus_loglik'):
        return dict(rows=rows, A=lc.segments(rs.randint(0, 60, size=40), d, 14100 + salt), floor=1e-12)
    if name in ('cooccurrence_counts', 'corpus_cooc'):
        return dict(A=cc.corpus_with_row_lengths(rs.randint(0, 40, size=90), d, 14200 + salt), words=cc.random_words(4, 8, d, 14300 + salt, empty=0.1))
    if name == 'masked_rmse':
        I, J = rs.randint(0, N, size=200), rs.randint(0, d, size=200)
        return dict(I=I, J=J, vals=X[I, J], lo=0.0, hi=float(X.max()))
    if name == 'argmax_rows':
        return dict()
    raise KeyError(name)


def borrow(e, m, name, salt):
    from rri_nmf_amd.engine import DeviceCorpus
    kw = borrow_inputs(name, m.d, salt, m.X)
    if name in CORPUS_BORROWERS:        # on a live corpus, closed after the call
        with DeviceCorpus(kw['A'], device=e.device) as corpus:
            if name == 'corpus_loglik':
                return e.entries_loglik(kw['rows'], corpus, kw['floor'])
            return e.cooccurrence_counts(corpus, kw['words'])
    return getattr(e, name)(**kw)


def reference_answer(name, W, T, kw):
    """what a handle that holds W and T answers, by the feature's own restatement (what the checks of check_borrowed accept)"""
    import cooc_cases as cc
    import loglik_cases as lc
    import rank_cases as rc
    import topn_cases as tc
    if name == 'topn_rows':
        return tc.topn_reference(W, T, kw['rows'], kw['n_top'], kw['exclude'])
    if name == 'rank_entries':
        return rc.rank_reference(W, T, kw['rows'], kw['targets'], kw['exclude'])
    if name in ('entries_loglik', 'corpus_loglik'):
        return lc.reference(W, T, kw['rows'], kw['A'], kw['floor'])[:3]
    if name in ('cooccurrence_counts', 'corpus_cooc'):
        return cc.dense_counts(kw['A'].toarray(), kw['words'])
    if name == 'masked_rmse':
        return float(np.sqrt(np.mean((np.clip(W.dot(T)[kw['I'], kw['J']], kw['lo'], kw['hi']) - kw['vals']) ** 2)))
    if name == 'argmax_rows':
        return np.argmax(W, 1).astype(np.int32)
    raise KeyError(name)


def check_borrowed(name, W, T, kw, got):
    """the answer `got` against the factors W and T, with the reference and the bound of the feature's own tests: topn_cases.check_real,
    rank_cases.rank_bands (test_rank_gpu.py), loglik_cases.reference with the checks of test_loglik_gpu.py, cooc_cases.dense_counts
    exactly, numpy for masked_rmse at 1e-12 relative (test_group_gpu.py) and for argmax_rows exactly (test_configs_gpu.py)"""
    import loglik_cases as lc
    import rank_cases as rc
    import topn_cases as tc
    if name == 'topn_rows':
        tc.check_real(W, T, kw['rows'], kw['n_top'], kw['exclude'], (None, None), got[0], got[1])
    elif name == 'rank_entries':
        ref, lo, hi, tol = rc.rank_bands(W, T, kw['rows'], kw['targets'], kw['exclude'])
        assert np.array_equal(got.indptr, ref.indptr) and np.array_equal(got.indices, ref.indices)
        assert np.all(got.rank >= lo) and np.all(got.rank <= hi) and np.array_equal(got.eligible, ref.eligible), name
        ok = ref.rank >= 0
        assert np.all(np.abs(got.val[ok] - ref.val[ok]) <= tol[ok]) and np.all(np.isnan(got.val[~ok])), name
    elif name in ('entries_loglik', 'corpus_loglik'):
        ll, mass, floored, p, bound = lc.reference(W, T, kw['rows'], kw['A'], kw['floor'])
        assert lc.floor_is_comparable(p, kw['floor'])
        assert np.array_equal(got[2], floored), name
        fin = np.isfinite(ll)
        assert np.array_equal(got[0][~fin], ll[~fin]) and np.all(np.abs(got[0][fin] - ll[fin]) <= bound[fin]), name
        assert np.array_equal(got[1], mass), name           # integer counts
    elif name in ('cooccurrence_counts', 'corpus_cooc'):
        want = reference_answer(name, W, T, kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
    elif name == 'masked_rmse':
        want = reference_answer(name, W, T, kw)
        assert abs(got - want) < 1e-12 * want, (name, got, want)
    elif name == 'argmax_rows':
        assert np.array_equal(got, np.argmax(W, 1)), name
    else:
        raise KeyError(name)


U53 = 2.0 ** -53


def check_frozen(got, want, absorbed=None):
    """the statistics of the handle (a FrozenRows, or None) against the model's (B, A, s, c): bit for bit, except after an absorb
    (absorbed = (X, W, decay, F before or None)), where the bound is that of test_absorb_takes_the_sums_of_the_handles_rows -- u (n + 2)
    |W|^T |X| and the like for the new sums -- plus one rounding each for the product with decay and the sum on top of what was there"""
    assert (got is None) == (want is None), 'the handle %s statistics, the model %s' % ('has' if got is not None else 'has no', 'has' if want is not None else 'none')
    if want is None:
        return
    B, A, s, c = want
    if absorbed is None:
        assert np.array_equal(got.B, B) and np.array_equal(got.A, A) and np.array_equal(got.s, s) and got.c == c, 'statistics changed'
        return
    X, W, decay, old = absorbed
    n = X.shape[0]
    bB = U53 * (n + 2) * np.abs(W).T.dot(np.abs(X)) + 2 * U53 * np.abs(B)
    bA = U53 * (n + 2) * np.abs(W).T.dot(np.abs(W)) + 2 * U53 * np.abs(A)
    bs = U53 * (n + 2) * np.abs(W).sum(0) + 2 * U53 * np.abs(s)
    bc = U53 * (X.size + 2) * float((X ** 2).sum()) + 2 * U53 * abs(c)
    assert (np.abs(got.B - B) <= bB).all() and (np.abs(got.A - A) <= bA).all() and (np.abs(got.s - s) <= bs).all() and abs(got.c - c) <= bc, \
        ('absorb', float((np.abs(got.B - B) / np.maximum(bB, 1e-300)).max()), float((np.abs(got.A - A) / np.maximum(bA, 1e-300)).max()))
    assert np.array_equal(got.A, got.A.T)


def handle_frozen(e):
    try:
        return e.get_frozen()
    except ValueError:          # RRI_ERR_INVALID: none are set
        return None


def fingerprint(e, m):
    """everything a refused call must leave bit for bit: W, T, the statistics, and on a CSR handle both blocked stores of X and
    the list and value of the uniform rows"""
    fz = handle_frozen(e)
    out = [e.get_W(), e.get_T()] + ([] if fz is None else [fz.B, fz.A, fz.s, np.float64(fz.c)])
    if m.kind == 'csr':
        for which in (0, 1):
            st = e.sparse_store(which)
            out += [st[key] for key in ('segptr', 'idx', 'perm', 'val')]
        rows, value = e.uniform_rows()
        out += [rows, np.float64(value)]
    return [np.array(a).tobytes() for a in out]


def relfro(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / (den if den > 0 else 1.0))


def factor_tol(flavour):
    return 1e-7 if FLAVOURS[flavour]['dtype'] == np.float32 else 1e-9       # uint8 counts with float64 scales: nothing is rounded


def objective_tol(m, want):
    """1e-12 relative where the objective comes from a residual (weighted handles always; unweighted ones whenever the cross
    terms cannot be valid: LegalState.xy_possible); the bound of the cross-term path only right after a whole sweep, where the
    handle may answer either way"""
    if m.F is not None:         # test_the_objective_is_that_of_the_stacked_problem: the formula cancels against c
        return 1e-12 * 0.5 * (float((m.X ** 2).sum()) + m.F[3])
    if m.weighted() or not m.ls.xy_possible:
        return 1e-12 * abs(want)
    return 1e-11 * max(abs(want), 1e-3 * float((m.X ** 2).sum()))


def check_value(m, op, got, want, log=None):
    """the answer of a borrower or an observer against numpy, at the bound its own tests use; m is the model (unchanged)"""
    n = op.name
    where = '%r' % (op,)
    if n in ('X_times', 'Xt_times'):
        err = relfro(got, want)                                  # test_nmf_gpu.py: 1e-13
        assert err < 1e-13, (where, err)
    elif n in ('range_finder', 'sparse_range_finder'):           # test_nmf_gpu.py / test_sparse_range_finder_gpu.py: 1e-12
        Q, B = got
        orth = float(np.abs(Q.T.dot(Q) - np.eye(Q.shape[1])).max())
        eb = relfro(B, Q.T.dot(m.X))
        assert orth < 1e-12 and eb < 1e-12, (where, orth, eb)
    elif n == 'colcounts':
        assert np.array_equal(got, want), where                  # test_preprocess_gpu.py
    elif n in ('bench_rank1', 'bench_copy'):
        assert got >= 0.0, where
    elif n == 'objective':
        if log:
            log('      objective: off by %.2e relative, bound %.0e (%s)' % (abs(got - want) / abs(want), objective_tol(m, want) / abs(want),
                                                                          'either path' if m.ls.xy_possible else 'residual path'))
        assert abs(got - want) <= objective_tol(m, want), (where, got, want, abs(got - want) / abs(want))
    elif n == 'objective_parts':
        assert abs(got[0] - want[0]) <= objective_tol(m, want[0]), (where, got[0], want[0])
        assert abs(got[1] - want[1]) <= 1e-12 * want[1] and abs(got[2] - want[2]) <= 1e-12 * want[2], (where, got, want)
    elif n in BORROWERS or n in CORPUS_BORROWERS:
        check_borrowed(n, m.W, m.T, borrow_inputs(n, m.d, op.arg, m.X), got)
    elif n == 'get_frozen':
        check_frozen(got, want)
    elif n == 'residual_check':
        # every entry is x - sum of k products, in float64: (k + 2) roundings of at most |x| + |w|^T |t| each, four times over
        bound = 4.0 * (K + 2) * 2.0 ** -53 * (np.abs(m.X) + np.abs(m.W).dot(np.abs(m.T)))
        assert np.all(np.abs(got - want) <= bound), (where, float(np.abs(got - want).max()))


def run_sequence(e, flavour, ops, log=None, raises=None):
    """ops on the handle e, each checked against a model that restarts from the handle's own W and T; returns the answers.
    raises: the index of the one operation that the oracle refuses, and the handle must refuse with the same exception type
    (as test_fuzz_gpu.py compares outcomes); an exception anywhere else is a failure of the test"""
    m = Model(flavour)
    tol = factor_tol(flavour)
    answers = []
    onchip = FLAVOURS[flavour]['env'].get('RRI_ONCHIP') == '1'
    for i, op in enumerate(ops):
        m.W, m.T = e.get_W(), e.get_T()
        fz = handle_frozen(e)
        assert (fz is None) == (m.F is None), 'before op %d %r of %r: the handle %s statistics' % (i, op, ops, 'has' if fz is not None else 'has no')
        if fz is not None:          # as W and T: the model restarts from what the handle holds
            m.F = (fz.B, fz.A, fz.s, fz.c)
        F_before, W_before, T_before = m.F, m.W, m.T
        launches = e.onchip_info()[1] if onchip else 0
        if i == raises:
            try:
                m.apply(op)
                refused = None
            except (ValueError, NotImplementedError) as exc:
                refused = type(exc)
            except AssertionError as exc:
                assert 'sums to 0' in str(exc) or 'negative entries' in str(exc), exc     # the oracle's own, not the model's
                refused = AssertionError
            assert refused is not None, 'the oracle accepts op %d %r of %r' % (i, op, ops)
            before = fingerprint(e, m) if refused is NotImplementedError else None
            try:
                apply_engine(e, m, op)
                raised = None
            except (ValueError, AssertionError, NotImplementedError) as exc:
                raised = type(exc)
            assert raised is refused, 'op %d %r of %r: the handle raised %r, the oracle %r' % (i, op, ops, raised, refused)
            if before is not None:      # RRI_ERR_UNSUPPORTED: "with nothing changed"
                assert fingerprint(e, m) == before, 'op %d %r of %r was refused and changed the handle' % (i, op, ops)
            m.ls.follow(op)
            answers.append(None)
            if log:
                log('op %2d %-24r both raise %s' % (i, op, refused.__name__))
            continue        # what a failed call leaves in W and T is read before the next operation, like any other state
        want = m.apply(op)
        got = apply_engine(e, m, op)
        answers.append(got)
        W, T = e.get_W(), e.get_T()
        cols = [c for c in range(K) if c != m.skip_col]
        ew, et = relfro(W[:, cols], m.W[:, cols]), relfro(T, m.T)
        if log:
            log('op %2d %-24r W %.2e  T %.2e' % (i, op, ew, et))
        assert ew < tol and et < tol, 'after op %d %r of %r: W %.3e T %.3e (tolerance %.0e)' % (i, op, ops, ew, et, tol)
        if category(op.name) == LOOK:
            check_value(m, op, got, want, log)
        if op.name in BORROWERS or op.name in CORPUS_BORROWERS or op.name in ('absorb', 'get_frozen', 'set_frozen', 'clear_frozen'):
            assert np.array_equal(W, W_before) and np.array_equal(T, T_before), 'op %d %r of %r changed W or T' % (i, op, ops)
        check_frozen(handle_frozen(e), m.F, absorbed=(m.X, m.W, op.arg, F_before) if op.name == 'absorb' else None)
        if m.kind == 'csr':
            rows, value = e.uniform_rows()
            assert np.array_equal(rows, m.U) and value == m.v, 'after op %d %r of %r: uniform rows %r, value %r' % (i, op, ops, rows, value)
        if onchip:      # persistent launches follow the statistics: none while they are set, and eligible again after a clear
            free = not PARAMS[m.pname].get('fix_W') and not PARAMS[m.pname].get('fix_T')      # (onchip_ok refuses a fixed factor as well)
            assert bool(e.onchip_info()[0]) == (m.F is None and free), 'after op %d %r of %r: onchip eligible %r' % (i, op, ops, e.onchip_info()[0])
            if op.name == 'sweep':
                took = e.onchip_info()[1] - launches
                p = PARAMS[m.pname]
                want_launch = F_before is None and not p.get('fix_W') and not p.get('fix_T')
                assert took == 0 if not want_launch else (took >= 1 or e.onchip_fallbacks() > 0), 'op %d %r of %r: %d persistent launches' % (i, op, ops, took)
        assert e.n_resets_used == (sum(1 for o in ops[:i + 1] if o.name == 'reset'))
    return answers


def run_model(flavour, ops):
    """the sequence on the model alone, chained: (model after the last operation, the answers, the state before each operation)"""
    m = Model(flavour)
    answers, states = [], []
    for op in ops:
        assert m.legal(op), (op, ops)
        states.append(m.state())
        answers.append(m.apply(op))
    return m, answers, states


# ---- seeded random sequences -----------------------------------------------------------------------------------------------
SEQ_LEN = 12
# legal least often first: get_frozen and clear_frozen want statistics, preprocess_csr_uniform zero-total rows and no list
OWN_HARD = ['preprocess_csr_uniform', 'get_frozen', 'clear_frozen']
OWN_FIRST = ['preprocess_csr_uniform', 'get_frozen', 'clear_frozen', 'upload_X_corpus', 'absorb', 'set_frozen', 'set_uniform_rows']
# how often a sweep or an objective is taken where neither rule about the flavour's own operations applies (the third rule of
# draw_sequence): chosen on the model, with the two rules above it, so that every own operation stands directly between two of
# those in at least 6 of the 24 default sequences and every operation of the alphabet is seen (test_cached_state_cases_cpu.py)
P3 = {'plain': 0.15, 'csr': 0.3}
_PARAM_NAMES = sorted(PARAMS)


def draw_op(rs, name):
    salt = int(rs.randint(1, 50))
    if name == 'sweep':
        return Op(name, int(rs.randint(1, 3)))
    if name == 'set_params':
        return Op(name, _PARAM_NAMES[int(rs.randint(len(_PARAM_NAMES)))])
    if name in ('update_T_row', 'update_W_col'):
        return Op(name, int(rs.randint(K)))
    if name == 'project_W':
        return Op(name, 1.0)
    if name in ('snapshot', 'rollback', 'preprocess', 'preprocess_csr', 'colcounts', 'bench_rank1', 'bench_copy', 'objective',
                'objective_parts', 'residual_check', 'clear_frozen', 'get_frozen', 'preprocess_csr_uniform', 'argmax_rows'):
        return Op(name)
    if name == 'absorb':
        return Op(name, (1.0, 0.9, 0.5)[salt % 3])
    return Op(name, salt)


def healthy(flavour, ops):
    """on the model alone: no exception, no reset, and no column of W or row of T anywhere near dead after any operation"""
    m = Model(flavour)
    try:
        for op in ops:
            if not m.legal(op):
                return False
            m.apply(op)
            if not (np.isfinite(m.W).all() and np.isfinite(m.T).all() and (m.W.sum(0) > 1e-6).all() and (m.T.sum(1) > 1e-6).all()):
                return False
    except (ValueError, AssertionError, NotImplementedError):
        return False
    return True


# A drawn sequence in which a topic dies on the model (a sweep right after X shrank fifty-fold under preprocess, say) is no case
# for this test: resets are off, and a column that is dead or alive by rounding compares nothing.  It is drawn again.  For the
# default seeds the redraws that this took are written down (test_cached_state_cases_cpu.py checks all of them on the model);
# above them random_sequence looks for the first healthy draw itself.
DEFAULT_SEEDS = 24
REDRAWS = {('gram-onchip', 2): 1, ('gram-onchip', 3): 1, ('gram-onchip', 7): 1, ('gram-onchip', 9): 1, ('gram-onchip', 13): 1,
           ('gram-onchip', 19): 1, ('gram-phases', 14): 1, ('residual', 10): 1, ('residual', 13): 1, ('csr', 3): 1, ('csr', 6): 1,
           ('csr', 10): 1, ('csr', 12): 1, ('csr', 22): 1, ('gram-fp32', 9): 1,
           ('gram-u8', 21): 1,
           ('gram-frozen', 6): 1, ('csr-uniform', 12): 1, ('csr-uniform', 17): 1,
           ('gram-early', 1): 1, ('gram-early', 10): 1, ('gram-early', 18): 1, ('gram-early', 20): 1, ('gram-early-u8', 2): 1}


def random_sequence(flavour, seed):
    """SEQ_LEN operations of the flavour's alphabet: at least half change the state, at least three borrow or observe, and the
    last two are sweep(1) and objective()"""
    if seed < DEFAULT_SEEDS:
        return draw_sequence(flavour, seed, REDRAWS.get((flavour, seed), 0))
    for attempt in range(64):
        ops = draw_sequence(flavour, seed, attempt)
        if healthy(flavour, ops):
            return ops
    raise AssertionError('no healthy sequence for %s, seed %d' % (flavour, seed))


def stand_in(m, op):
    n = op.name
    if n == 'rollback' and not m.has_snap:
        return Op('snapshot')
    if n == 'clear_frozen':
        return Op('set_frozen', 1 + op_salt(op))
    if n == 'get_frozen':
        return Op('absorb', 0.9)
    if n == 'preprocess_csr_uniform':
        return Op('set_uniform_rows', 2) if m.U else Op('upload_X_csr', ZERO_ROWS + 1)
    return op


def op_salt(op):
    return 0 if op.arg is None else int(op.arg) % 7 if not isinstance(op.arg, str) else 0


def draw_sequence(flavour, seed, attempt):
    rs = np.random.RandomState((97 * RANDOM_FLAVOURS.index(flavour) + attempt) * 100003 + seed)
    names = alphabet(flavour)
    by = {STATE: [x for x in names if category(x) == STATE], LOOK: [x for x in names if category(x) == LOOK]}
    slots = [STATE] * 6 + [LOOK] * 3 + ['any']
    rs.shuffle(slots)
    m = LegalState(FLAVOURS[flavour]['kind'], is_counts(flavour), flavour)
    own = new_ops(flavour)          # (empty for the flavours that came before them: nothing more is drawn from rs there)
    behind = ('sweep', 'objective', 'objective_parts')
    ops = []
    for pos, slot in enumerate(slots):
        pool = names if slot == 'any' else by[slot]
        for tries in range(100):
            op = draw_op(rs, pool[int(rs.randint(len(pool)))])
            # the alphabets of the new flavours are twice as long: where no rule below decides, their operations are taken in turn
            # over seeds and places, not by chance (the arguments stay drawn), so that 24 seeds see every one of them
            if own:
                turn = slots.count(slot) * seed + slots[:pos].count(slot)       # the how-manieth slot of its kind over the seeds
                op = draw_op(rs, pool[(turn + tries) % len(pool)])
                if not m.legal(op) and not tries:       # what it waits for, in its place: the next time it is its turn it is legal
                    op = stand_in(m, op)
                elif op.name == 'snapshot' and m.has_snap and m.legal(Op('rollback')):
                    op = Op('rollback')
            # the new state matters to what a sweep or an objective has just left on the handle and to the next one: right behind
            # one of those an operation of the flavour's own is taken every other time it could be (the rule of set_X_scales
            # below), right behind such an operation always a sweep or an objective, and elsewhere one of those with the chance P3
            if own and ops and ops[-1].name in behind:
                cand = [x for x in own if x in pool and m.legal(draw_op(np.random.RandomState(0), x))]
                fresh = [x for x in OWN_FIRST if x in cand and not any(o.name == x for o in ops)]
                if cand and rs.rand() < 0.5:        # one the sequence does not have yet -- the hardest to place first --, else any
                    hard = [x for x in fresh if x in OWN_HARD]
                    op = draw_op(rs, hard[0] if hard else fresh[seed % len(fresh)] if fresh else cand[int(rs.randint(len(cand)))])
                    if op.name == 'set_uniform_rows' and m.U and op.arg % 2 and not any(o.name == 'preprocess_csr_uniform' for o in ops):
                        op = Op(op.name, 3 * op.arg + 2)        # a clear: the rows it leaves empty are what preprocess_csr_uniform waits for
            elif own and ops and ops[-1].name in own:
                cand = [x for x in behind if x in pool]
                op = draw_op(rs, cand[int(rs.randint(len(cand)))])
            elif own and rs.rand() < P3[FLAVOURS[flavour]['kind']]:
                cand = [x for x in behind if x in pool]
                op = draw_op(rs, cand[int(rs.randint(len(cand)))])
            if FLAVOURS[flavour].get('uniform') and op.name == 'upload_X_csr' and op.arg % 2:
                op = Op(op.name, op.arg + ZERO_ROWS)       # every other one with zero-total rows, for preprocess_csr_uniform
            # preprocess is legal only after an X with zeros went up: taken every other time it could be, or it is hardly seen
            # (counts always have zeros: there it is drawn like any other operation)
            if 'preprocess' in pool and not m.counts and m.legal(Op('preprocess')) and not any(o.name == 'preprocess' for o in ops) and rs.rand() < 0.5:
                op = Op('preprocess')
            # counts: a changed scale matters to what a sweep or an objective has just left on the handle, and right behind one of
            # those it is one of the 15 state-changing operations of a pool of 21: taken every other time it could be
            if m.counts and 'set_X_scales' in pool and ops and ops[-1].name in ('sweep', 'objective', 'objective_parts') and rs.rand() < 0.5:
                op = draw_op(rs, 'set_X_scales')
            if m.legal(op):
                break
        else:
            raise AssertionError('no legal operation found')
        m.follow(op)
        ops.append(op)
    return ops + [Op('sweep', 1), Op('objective')]


def persistent_sweeps(ops):
    """how many sweep() calls of ops an RRI_ONCHIP=1 handle must run as persistent launches: those with both factors free
    (onchip_ok refuses fix_W and fix_T; penalties, the clip and the projection of T ride in the kernel)"""
    ls, count = LegalState('plain'), 0
    for op in ops:
        p = PARAMS[ls.pname]
        if op.name == 'sweep' and not p.get('fix_W') and not p.get('fix_T') and not ls.has_F:     # (and none while statistics are set)
            count += 1
        ls.follow(op)
    return count


def n_seeds():
    return int(os.environ.get('RRI_CACHED_STATE_CASES', '24'))


# ---- directed sequences ----------------------------------------------------------------------------------------------------
class Case(object):
    """row: the row of the table above changed() the case aims at.  stale: how a handle that kept the named value would answer
    the LAST operation, in oracle terms (stale_reference), or None with `waived` saying why that cannot be written.
      ('x_sq', j)        the objective with ||X||^2 of the X before operation j
      ('xy', j)          the objective with the cross terms <w_t, X t_t> of the W, T (and X) before operation j
      ('penalty', j)     the objective with the penalties before operation j
      ('objective', j)   the objective of the W and T before operation j (what the persistent launch left)
      ('factors', j, fields)  the last operation (a sweep) run from the current state with `fields` as they were before operation j
      ('T_row', j)       the last operation (update_T_row) with the row computed from the X before operation j
      ('scales', j)      the last two operations (sweep(1), objective) on the current counts under the scales before operation j
      ('frozen', j)      the last operation under the frozen statistics as they were before operation j
      ('uniform', j)     the last operation on the current stored part of X under the list and value of before operation j
      ('W_col', j, tt)   the last operation (update_W_col) with the early-sums partials T T[tt,:]^T of the T before operation j
    """

    def __init__(self, name, row, flavour, ops, stale=None, waived=None, raises=None):
        self.name, self.row, self.flavour, self.ops, self.stale, self.waived, self.raises = name, row, flavour, ops, stale, waived, raises
        assert (stale is None) != (waived is None)


S1, S2, OBJ = ('sweep', 1), ('sweep', 2), ('objective',)


def _case(name, row, flavour, steps, **kw):
    return Case(name, row, flavour, [Op(*s) for s in steps], **kw)


CASES = []
# x_sq_valid: sweep, objective (takes ||X||^2), another X, sweep, objective
for _name, _fl, _chg in (('upload_X', 'gram-phases', ('upload_X', 2)), ('scale_X', 'gram-phases', ('scale_X', 3)),
                         ('bind_X_device', 'gram-bind', ('bind_X', 2))):
    CASES.append(_case('x_sq-%s' % _name, 'x_sq_valid', _fl, [S1, OBJ, _chg, S1, OBJ], stale=('x_sq', 2)))
# xy_run / xy_valid: sweep, objective, W or T written from outside, objective
for _name, _chg in (('project_W_rows', ('project_W', 1.0)), ('rollback', ('rollback',)), ('apply_reset_vectors', ('reset', 4)),
                    ('set_T', ('set_T', 5))):
    _steps = [('snapshot',)] if _name == 'rollback' else []
    _steps += [S1, OBJ, _chg, OBJ]
    CASES.append(_case('xy-%s' % _name, 'xy_run / xy_valid', 'gram-phases', _steps, stale=('xy', len(_steps) - 2)))
# obj_track_valid: the objective a persistent launch left
CASES.append(_case('obj_track-set_params', 'obj_track_valid', 'gram-onchip', [S2, OBJ, ('set_params', 'pen_a'), OBJ], stale=('penalty', 2)))
CASES.append(_case('obj_track-update_W_col', 'obj_track_valid', 'gram-onchip', [S2, ('update_W_col', 1), OBJ], stale=('objective', 1)))
# q_valid / gfull_valid: two sweeps with T fixed, T or X changed between them
for _name, _chg, _fields in (('set_T', ('set_T', 6), ('T',)), ('rollback', ('rollback',), ('T',)), ('scale_X', ('scale_X', 7), ('X',)),
                             ('upload_X', ('upload_X', 4), ('X',))):
    _steps = [('snapshot',), S1] if _name == 'rollback' else []
    _steps += [('set_params', 'fix_T'), S1, _chg, S1]
    CASES.append(_case('q-%s' % _name, 'q_valid / gfull_valid', 'gram-phases', _steps, stale=('factors', len(_steps) - 2, _fields)))
# resid_valid: the maintained residual E of the three weighted layouts (dense weights, dense 0/1 bit-packed, pattern only)
_LAYOUTS = (('weights', 'weighted', []), ('bits', 'weighted', [('upload_mask_pattern', 1)]), ('pattern', 'pattern', []))
for _lname, _fl, _pre in _LAYOUTS:
    _newmask = ('upload_observed', 8) if _fl == 'pattern' else ('upload_mask_pattern', 9) if _lname == 'bits' else ('upload_mask', 9)
    for _name, _chg, _fields in (('set_W', ('set_W', 8), ('W',)), ('set_T', ('set_T', 9), ('T',)), ('rollback', ('rollback',), ('W', 'T')),
                                 ('project_W_rows', ('project_W', 1.0), ('W',)), ('new_mask', _newmask, ('M', 'X'))):
        # a sweep rebuilds E once, at its start, unless the objective has just stored it: only after objective() does the
        # second sweep depend on resid_valid having been dropped
        for _suffix, _between in (('', []), ('-after_objective', [OBJ])):
            _steps = list(_pre) + ([('snapshot',)] if _name == 'rollback' else []) + [S1] + _between + [_chg, S1]
            CASES.append(_case('resid-%s-%s%s' % (_lname, _name, _suffix), 'resid_valid', _fl, _steps,
                               stale=('factors', len(_steps) - 2, _fields)))
    if _lname == 'weights':     # the caller-owned counterpart of upload_mask, at the even d that rri_bind_mask_device accepts
        for _suffix, _between in (('', []), ('-after_objective', [OBJ])):
            _steps = [S1] + _between + [('bind_mask', 9), S1]
            CASES.append(_case('resid-bound_mask%s' % _suffix, 'resid_valid', 'weighted-bind', _steps,
                               stale=('factors', len(_steps) - 2, ('M',))))
    CASES.append(_case('resid-%s-objective_between_sweeps' % _lname, 'resid_valid', _fl, list(_pre) + [S1, OBJ, S1],
                       waived='the legitimate path: the objective stored E and the sweep skips its rebuild; nothing is stale'))
CASES.append(_case('resid-residual_update', 'resid_valid', 'residual', [S1, ('residual_update', 3), S1],
                   waived='the stored R after a foreign rank-one update is no function of W, T and X that the oracle has'))
CASES.append(_case('resid-form_switch', 'resid_valid', 'residual', [S1, ('set_params', 'fix_T'), S1, ('set_params', 'free'), S1],
                   stale=('factors', 2, ('W',))))
# carry_valid: after a free sweep Zpart / Gpart hold topic 0's partial sums; a borrower overwrites them
for _name, _b in (('Xt_times', ('Xt_times', 1)), ('column_positive_counts', ('colcounts',)), ('range_finder', ('range_finder', 2)),
                  ('X_times', ('X_times', 3))):
    for _nname, _next in (('sweep', S1), ('update_T_row', ('update_T_row', 0))):
        CASES.append(_case('carry-%s-%s' % (_name, _nname), 'carry_valid / carry_topic', 'gram-phases', [S1, _b, _next],
                           waived='an overwritten scratch buffer is no value the oracle can state'))
# after a call that ended in an error: CH_ENDED and the column verdict that was pending
CASES.append(_case('ended-zero_column', 'carry_valid / pending_wcheck (CH_ENDED)', 'gram-phases',
                   [('zero_W_column', 2), S1, ('set_W', 3), S1], raises=1,
                   waived='an error is a verdict, not a value'))
# ---- the uint8 store: the two scale vectors are per-handle state and a part of X -------------------------------------------------
_SC = ('set_X_scales', 5)       # 5 % 3 == 2: both vectors
CASES.append(_case('x_sq-set_X_scales', 'x_sq_valid', 'gram-u8', [S1, OBJ, _SC, S1, OBJ], stale=('x_sq', 2)))
CASES.append(_case('xy-set_X_scales', 'xy_run / xy_valid', 'gram-u8', [S1, OBJ, _SC, OBJ], stale=('xy', 2)))
CASES.append(_case('q-set_X_scales', 'q_valid / gfull_valid', 'gram-u8', [('set_params', 'fix_T'), S1, _SC, S1],
                   stale=('factors', 2, ('X',))))
# carry_valid: the partial sums of topic 0 that a free sweep leaves were taken from the old X; unlike an overwritten scratch
# buffer, that is a value the oracle has
CASES.append(_case('carry-set_X_scales-sweep', 'carry_valid / carry_topic', 'gram-u8', [S1, _SC, S1], stale=('factors', 1, ('X',))))
CASES.append(_case('carry-set_X_scales-update_T_row', 'carry_valid / carry_topic', 'gram-u8', [S1, _SC, ('update_T_row', 0)],
                   stale=('T_row', 1)))
# a new X puts both vectors back to ones: the stale handle factorises the new counts under the old scales
for _name, _chg in (('upload_X', ('upload_X', 2)), ('bind_X', ('bind_X', 2))):
    CASES.append(_case('scales-reset-by-%s' % _name, 'rscale / cscale', 'gram-u8', [_SC, S1, _chg, S1, OBJ], stale=('scales', 2)))
# rri_scale_X on a bound X, which only this store allows
CASES.append(_case('q-scale_X-bound', 'q_valid / gfull_valid', 'gram-u8',
                   [('bind_X', 3), ('set_params', 'fix_T'), S1, ('scale_X', 7), S1], stale=('factors', 3, ('X',))))
# ---- frozen statistics: read where a step uses them, and no row of the table is dropped for them (rri_frozen_set calls no changed()).
#      So what was produced under one set of statistics -- the carry, a pending column verdict, the cross terms, the tracked
#      objective -- is consumed under another ---------------------------------------------------------------------------------------
F1, F2, CLR = ('set_frozen', 1), ('set_frozen', 2), ('clear_frozen',)
for _tag, _fl in (('plain', 'gram-phases'), ('csr', 'csr')):
    _up = ('upload_X_csr', 2) if _tag == 'csr' else ('upload_X', 2)
    for _name, _steps, _kw in (
            # carry and pending verdict
            ('carry-set-sweep', [S1, F1, S1], dict(stale=('frozen', 1))),
            ('carry-set-update_T_row', [S1, F1, ('update_T_row', 0)], dict(stale=('frozen', 1))),
            ('carry-clear-sweep', [F1, S1, CLR, S1], dict(stale=('frozen', 2))),
            ('carry-other-sweep', [F1, S1, F2, S1], dict(stale=('frozen', 2))),
            # the column verdict: under 'pen_a' column K - 1 of W is 0 after its W half and lives by s[K - 1] alone
            ('verdict', [('set_params', 'pen_a'), ('zero_W_column', K - 1), ('set_frozen', 'dead'), S1, CLR, S1],
             dict(raises=5, waived='an error is a verdict, not a value')),
            # cross terms
            ('xy-set', [S1, OBJ, F1, OBJ], dict(stale=('frozen', 2))),
            ('xy-clear', [F1, S1, OBJ, CLR, OBJ], dict(stale=('frozen', 3))),
            # reset with no run paused: topic t of the statistics is zeroed
            ('reset', [F1, S1, ('reset', 4), ('get_frozen',), OBJ, S1], dict(stale=('frozen', 2))),
            # rollback restores W and T only: the rows absorbed since the snapshot stay absorbed
            ('rollback', [F1, ('snapshot',), S1, ('absorb', 1.0), ('rollback',), S1], dict(stale=('frozen', 3))),
            # the online loop: ||X||^2 is that of the new X, c that of the old
            ('online', [S1, ('absorb', 0.9), _up, ('set_W', 3), S1, OBJ], dict(stale=('x_sq', 2))),
            ('fixed_T', [F1, ('set_params', 'fix_T'), S1, CLR, S1],
             dict(waived='the legitimate path: a sweep with T fixed ignores the statistics, Qt and Gfull are reused; nothing is stale'))):
        CASES.append(_case('frozen-%s-%s' % (_tag, _name), 'carry_valid / pending_wcheck / xy_valid / obj_track_valid under frozen statistics',
                           _fl, _steps, **_kw))
# the tracked objective of a persistent launch (RRI_ONCHIP=1), and the launches themselves: none while statistics are set
CASES.append(_case('frozen-obj_track-set', 'obj_track_valid', 'gram-frozen', [S2, OBJ, F1, OBJ], stale=('frozen', 2)))
CASES.append(_case('frozen-obj_track-clear', 'obj_track_valid', 'gram-frozen', [S2, OBJ, F1, OBJ, S1, CLR, S1, OBJ], stale=('frozen', 5)))
# ---- uniform rows: the list and the value are a part of X ----------------------------------------------------------------------------
_UNI = (('value', ('set_uniform_rows', 4)), ('list', ('set_uniform_rows', 3)), ('clear', ('set_uniform_rows', 5)), )
_ZUP, _PPU, _UPC = ('upload_X_csr', ZERO_ROWS + 1), ('preprocess_csr_uniform',), ('upload_X_corpus', 3)


def _cache_cases(prefix, flavour, pre, chg):
    """fill one of the caches taken from X, change X by `chg`, use the cache"""
    n = len(pre)
    CASES.append(_case('x_sq-' + prefix, 'x_sq_valid', flavour, pre + [S1, OBJ, chg, S1, OBJ], stale=('x_sq', n + 2)))
    CASES.append(_case('xy-' + prefix, 'xy_run / xy_valid', flavour, pre + [S1, OBJ, chg, OBJ], stale=('xy', n + 2)))
    CASES.append(_case('q-' + prefix, 'q_valid / gfull_valid', flavour, pre + [('set_params', 'fix_T'), S1, chg, S1], stale=('factors', n + 2, ('X',))))
    CASES.append(_case('carry-%s-sweep' % prefix, 'carry_valid / carry_topic', flavour, pre + [S1, chg, S1], stale=('factors', n + 1, ('X',))))
    CASES.append(_case('carry-%s-update_T_row' % prefix, 'carry_valid / carry_topic', flavour, pre + [S1, chg, ('update_T_row', 0)], stale=('T_row', n + 1)))


for _vname, _chg in _UNI:
    _cache_cases('set_uniform_rows-' + _vname, 'csr-uniform', [], _chg)
_cache_cases('preprocess_csr_uniform', 'csr-uniform', [_ZUP], _PPU)
_cache_cases('upload_X_corpus', 'csr-frozen', [], _UPC)
# a corpus behind a handle that had a list: the list is emptied
CASES.append(_case('uniform-emptied-by-upload_X_corpus', 'uni_n / uni_value', 'csr-uniform', [S1, _UPC, S1, OBJ], stale=('uniform', 1)))
# ---- the state the header rules out: statistics first, uniform rows second.  Refused, with nothing changed ---------------------------
CASES.append(_case('mixed-set_uniform_rows', 'fzB / uni_n', 'csr-frozen', [F1, ('set_uniform_rows', 3), S1], raises=1,
                   waived='a refusal is a verdict, not a value'))
CASES.append(_case('mixed-preprocess_csr_uniform', 'fzB / uni_n', 'csr-frozen', [_ZUP, F1, _PPU, S1], raises=2,
                   waived='a refusal is a verdict, not a value'))
# ---- the evaluation calls as borrowers: they promise to write nothing a later sweep reads ---------------------------------------------
_BSALT = 7
for _b in BORROWERS + ['absorb']:
    _op = (_b,) if _b == 'argmax_rows' else ('absorb', 1.0) if _b == 'absorb' else (_b, _BSALT)
    for _nname, _next in (('sweep', S1), ('update_T_row', ('update_T_row', 0))):
        CASES.append(_case('carry-%s-%s' % (_b, _nname), 'carry_valid / carry_topic', 'gram-phases', [S1, _op, _next],
                           waived='an overwritten scratch buffer is no value the oracle can state'))
    if _b != 'absorb':      # (refused on weighted handles and on the explicit-residual schedule)
        for _fl in ('weighted', 'pattern', 'residual'):
            for _suffix, _between in (('', []), ('-after_objective', [OBJ])):
                CASES.append(_case('resid-%s-%s%s' % (_b, _fl, _suffix), 'resid_valid', _fl, [S1] + _between + [_op, S1],
                                   waived='the stored residual after a call that must not touch it: nothing is stale'))
for _b in CORPUS_BORROWERS + ['absorb']:
    _op = ('absorb', 1.0) if _b == 'absorb' else (_b, _BSALT)
    for _nname, _next in (('sweep', S1), ('update_T_row', ('update_T_row', 0))):
        CASES.append(_case('carry-%s-csr-%s' % (_b, _nname), 'carry_valid / carry_topic', 'csr', [S1, _op, _next],
                           waived='an overwritten scratch buffer is no value the oracle can state'))
# ---- the early-sums schedule ('gram-early': RRI_TROW_SMALL=0).  What it keeps between steps and calls: early_valid / early_topic, the
#      partials of T T[t,:]^T that k_trow_early leaves for the early job of topic t's pass, and carry_wfin / wfin_topic, which say
#      that the carry is k_wfin's (red reduced already, two Gram entries as tile sums in wfp).  Every case is "sweep, change,
#      sweep or half step"; after the first sweep the carry of topic 0 is k_wfin's and wfp is live -----------------------------------
_E = 'gram-early'
_EROW = 'early_valid / early_topic'
_CROW = 'carry_valid / carry_wfin / wfin_topic'
# the rows of the table above changed() that a plain Gram-form handle has (resid_valid belongs to the weighted and the explicit-
# residual handles, obj_track_valid to the persistent sweep: neither exists under this flavour's environment)
for _name, _chg in (('upload_X', ('upload_X', 2)), ('scale_X', ('scale_X', 3))):
    CASES.append(_case('early-x_sq-%s' % _name, 'x_sq_valid', _E, [S1, OBJ, _chg, S1, OBJ], stale=('x_sq', 2)))
for _name, _chg in (('project_W_rows', ('project_W', 1.0)), ('rollback', ('rollback',)), ('apply_reset_vectors', ('reset', 4)), ('set_T', ('set_T', 5))):
    _steps = ([('snapshot',)] if _name == 'rollback' else []) + [S1, OBJ, _chg, OBJ]
    CASES.append(_case('early-xy-%s' % _name, 'xy_run / xy_valid', _E, _steps, stale=('xy', len(_steps) - 2)))
for _name, _chg, _fields in (('set_T', ('set_T', 6), ('T',)), ('upload_X', ('upload_X', 4), ('X',))):
    # a free sweep first: the fixed-T sweeps run behind the schedule, whose last T half left early_valid and whose last W half the carry
    CASES.append(_case('early-q-%s' % _name, 'q_valid / gfull_valid', _E, [S1, ('set_params', 'fix_T'), S1, _chg, S1], stale=('factors', 3, _fields)))
# the carry of topic 0 as k_wfin leaves it, taken from the old X
for _name, _chg in (('upload_X', ('upload_X', 2)), ('scale_X', ('scale_X', 3))):
    CASES.append(_case('early-carry-%s-sweep' % _name, _CROW, _E, [S1, _chg, S1], stale=('factors', 1, ('X',))))
    CASES.append(_case('early-carry-%s-update_T_row' % _name, _CROW, _E, [S1, _chg, ('update_T_row', 0)], stale=('T_row', 1)))
# early_valid: a change between the T half and the W half of ONE topic -- the W half must not take T T[t,:]^T from Tearly.  reset(7)
# rewrites topic 2 itself, reset(13) topic 3 (entry 3 of T T[2,:]^T); the rollback takes T back to the snapshot
for _name, _chg in (('reset-own-topic', ('reset', 7)), ('reset-other-topic', ('reset', 13)), ('rollback', ('rollback',)), ('set_T', ('set_T', 5))):
    _steps = ([('snapshot',)] if _name == 'rollback' else []) + [S1, ('update_T_row', 2), _chg, ('update_W_col', 2)]
    CASES.append(_case('early-halves-%s' % _name, _EROW, _E, _steps, stale=('W_col', len(_steps) - 2, 2)))
# ... and a sweep ends with early_topic = K - 1: a lone W half of that topic after T was written from outside
CASES.append(_case('early-lone_W_half-after-set_T', _EROW, _E, [S1, ('set_T', 5), ('update_W_col', K - 1)], stale=('W_col', 1, K - 1)))
# early_topic: the partials are those of topic 2, the W half is topic 3's
CASES.append(_case('early-topic-other_W_half', _EROW, _E, [S1, ('update_T_row', 2), ('update_W_col', 3)], stale=('W_col', 2, 2)))
# the borrowers between k_wfin and the T half that takes up its carry
for _b in BORROWERS:
    _op = (_b,) if _b == 'argmax_rows' else (_b, _BSALT)
    for _nname, _next in (('sweep', S1), ('update_T_row', ('update_T_row', 0))):
        CASES.append(_case('early-carry-%s-%s' % (_b, _nname), _CROW, _E, [S1, _op, _next],
                           waived='an overwritten scratch buffer is no value the oracle can state'))
# set_params to a set without the schedule and back (no penalty changes: rri_set_params calls no changed()): the T half under fix_W
# finds k_wfin's carry, which only k_trow_early can take up (the `carry_wfin && !early` line of enqueue_T_half)
for _nname, _next in (('sweep', S1), ('update_T_row', ('update_T_row', 0))):
    CASES.append(_case('early-off_and_on-%s' % _nname, _CROW, _E, [S1, ('set_params', 'fix_W'), _next, ('set_params', 'free'), S1],
                       waived='k_wfin leaves the Gram row of its carry in another buffer than k_reduce reads: no value the oracle can state'))
# a call that ends in an error in the middle of the schedule, then a sweep
CASES.append(_case('early-ended-zero_column', 'carry_valid / pending_wcheck (CH_ENDED)', _E, [S1, ('zero_W_column', 2), S1, ('set_W', 3), S1], raises=2,
                   waived='an error is a verdict, not a value'))
CASES = {c.name: c for c in CASES}


def zero_column_W(W0, t):
    W = W0.copy()
    W[:, t] = 0.0
    return W


def stale_reference(case):
    """(what the last operation answers by the model, what a handle that kept the case's value would answer)"""
    m, answers, states = run_model(case.flavour, case.ops)
    kind, j = case.stale[0], case.stale[1]
    old, cur = states[j], states[-1]
    o = oracle()
    if kind == 'x_sq':
        return answers[-1], answers[-1] + 0.5 * (float((old['X'] ** 2).sum()) - float((m.X ** 2).sum()))
    if kind == 'xy':
        cross = sum(float(old['W'][:, t].dot(old['X'].dot(old['T'][t, :]))) for t in range(K))
        quad = float((m.W.T.dot(m.W) * m.T.dot(m.T.T)).sum())
        return answers[-1], 0.5 * float((m.X ** 2).sum()) - cross + 0.5 * quad
    if kind == 'penalty':
        return answers[-1], m.objective_at(m.X, m.M, m.W, m.T, regs={r: PARAMS[old['pname']].get(r, 0.0) for r in REGS})
    if kind == 'objective':
        return answers[-1], m.objective_at(m.X, m.M, old['W'], old['T'])
    if kind == 'factors':
        src = dict(cur)
        for f in case.stale[2]:
            src[f] = old[f]
        W, T = m.sweep_from(src['X'], src['M'], src['W'], src['T'], case.ops[-1].arg, pname=cur['pname'])
        return (m.W, m.T), (W, T)
    if kind == 'T_row':
        t = case.ops[-1].arg
        ms = Model(case.flavour)
        ms.ls.pname, ms.X, ms.W, ms.T = cur['pname'], old['X'], cur['W'], cur['T']
        T = m.T.copy()
        T[t, :] = ms.half_T(t)
        return (m.W, m.T), (m.W, T)
    if kind == 'W_col':
        # the early job's sums from stale partials: T T[tt,:]^T of the T before operation j in place of T T[t,:]^T of the current
        # one, its entry t for ||T[t,:]||^2; the row dots X T[t,:]^T are the pass's, from the current T
        t, tt = case.ops[-1].arg, case.stale[2]
        tts = old['T'].dot(old['T'][tt])
        nt, tts[t] = float(tts[t]), 0.0
        regs = {r: PARAMS[cur['pname']].get(r, 0.0) for r in REGS}
        numer = cur['X'].dot(cur['T'][t]) - cur['W'].dot(tts)
        W = cur['W'].copy()
        W[:, t] = o.qf_min(-(numer - regs['reg_w_l1']), nt + regs['reg_w_l2'], s=None, ub=None)[0]
        return (m.W, m.T), (W, m.T)
    if kind in ('frozen', 'uniform'):
        ms = Model(case.flavour)
        ms.ls.pname, ms.X, ms.M, ms.W, ms.T, ms.F, ms.U, ms.v = (cur[key] for key in ('pname', 'X', 'M', 'W', 'T', 'F', 'U', 'v'))
        if kind == 'frozen':
            ms.F = old['F']
        else:       # the rows of the old list hold the old value again
            ms.X = cur['X'].copy()
            ms.X[cur['U'], :] = 0.0
            ms.X[old['U'], :] = old['v']
        want = ms._apply(case.ops[-1])
        return (answers[-1], want) if category(case.ops[-1].name) == LOOK else ((m.W, m.T), (ms.W, ms.T))
    if kind == 'scales':
        assert [o.name for o in case.ops[-2:]] == ['sweep', 'objective']
        before = states[-2]
        Xs = scaled_counts(before['C'], old['r'], old['s'])
        W, T = m.sweep_from(Xs, None, before['W'], before['T'], case.ops[-2].arg, pname=before['pname'])
        return answers[-1], m.objective_at(Xs, None, W, T)
    raise KeyError(kind)
