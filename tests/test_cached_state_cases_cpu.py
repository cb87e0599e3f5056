"""The cases of tests/cs_cases.py, checked without a GPU: that their inputs can see the fault each aims at, that the written
coverage list is the code's, and that the seeded sequences are what they promise.

Every directed case whose staleness can be written in oracle terms carries a stale reference: what a handle that kept the named
value would answer (old T and X for Qt / Gfull, old X for ||X||^2, old W / T / X for the cross terms, old penalties or old
factors for the tracked objective, old mask / W / T for E; for the uint8 store the old scale vectors, also under new counts,
and the old X for the carried partial sums of topic 0).  It must lie at least 1e3 times the case's tolerance away from the true
answer.  Waived, with the reason in the case: the carry cases after a borrower and the foreign residual update (an overwritten
buffer is no value the oracle has), the legitimate stored-E path (nothing is stale) and the error case (a verdict, not a value).

The state that came after the table -- frozen statistics, uniform rows, an X built from a DeviceCorpus -- has stale references of
its own (the last operation under the statistics, or under the list and value, of before), and the entry points are no longer
found by a literal `changed(` alone: every `rri_status rri_*(` of include/rri_hip.h and every public RRIEngine method that
calls the library on its handle must be classified in cs_cases, so a new one fails here until someone does."""
import os
import re

import numpy as np
import pytest

import cs_cases as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STALE = [c for c in cs.CASES.values() if c.stale is not None]
WAIVED = [c for c in cs.CASES.values() if c.stale is None]


@pytest.mark.parametrize('case', STALE, ids=[c.name for c in STALE])
def test_a_stale_value_lies_far_outside_the_tolerance(case):
    true, stale = cs.stale_reference(case)
    if isinstance(true, tuple):
        dist = max(cs.relfro(stale[0], true[0]), cs.relfro(stale[1], true[1]))
        tol = cs.factor_tol(case.flavour)
    else:
        m, _, _ = cs.run_model(case.flavour, case.ops)
        dist, tol = abs(stale - true), cs.objective_tol(m, true)
    print('%s: stale reference at %.3e, tolerance %.1e' % (case.name, dist, tol))
    assert dist >= 1e3 * tol, (case.name, dist, tol)


@pytest.mark.parametrize('case', WAIVED, ids=[c.name for c in WAIVED])
def test_a_waived_case_says_why_and_runs_on_the_model(case):
    assert len(case.waived) > 20
    if case.raises is None:
        cs.run_model(case.flavour, case.ops)
    else:       # the oracle refuses the operation the case says, and nothing else
        m = cs.Model(case.flavour)
        for i, op in enumerate(case.ops):
            if i == case.raises:
                with pytest.raises((ValueError, AssertionError, NotImplementedError)):
                    m.apply(op)
                m.ls.follow(op)
            else:
                m.apply(op)


def test_the_seven_rows_of_the_table_have_cases():
    src = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_hip.hip')).read()
    table = src[src.index('// ---- what a handle keeps between steps and calls'):src.index('enum : unsigned {')]
    rows = re.findall(r'^//   (\w+(?: / \w+)?)\s+x', table, flags=re.M)
    assert len(rows) == 7, rows
    aimed = ' '.join(c.row for c in cs.CASES.values())
    for row in rows:
        for flag in row.split(' / '):
            assert flag in aimed, 'no directed case aims at %s' % flag


def functions_that_call_changed():
    src = open(os.path.join(ROOT, 'rri_nmf_amd', 'csrc', 'rri_hip.hip')).read().splitlines()
    head = re.compile(r'^(?:static |inline )*[\w:\*]+[\s\*]+(\w+)\s*\(')
    cur, found = None, set()
    for line in src:
        m = head.match(line)
        if m and not line.rstrip().endswith(';'):
            cur = m.group(1)
        if re.search(r'\bchanged\(', line) and cur != 'changed':
            found.add(cur)
    return found


def test_the_coverage_list_is_the_code():
    found = functions_that_call_changed()
    assert found == set(cs.COVERAGE), (sorted(found - set(cs.COVERAGE)), sorted(set(cs.COVERAGE) - found))
    everything = set()
    for flavour in cs.RANDOM_FLAVOURS:
        everything |= set(cs.alphabet(flavour))
    assert not everything & set(cs.DIRECTED_ONLY)
    for op in cs.DIRECTED_ONLY:
        assert any(o.name == op for c in cs.CASES.values() for o in c.ops), op
    everything |= set(cs.DIRECTED_ONLY)
    for fn, ops in cs.COVERAGE.items():
        if isinstance(ops, tuple):
            assert ops[0] == 'excluded' and len(ops[1]) > 10, fn
            continue
        for op in ops:
            assert op in everything, (fn, op)
    for op in cs.NO_CHANGED.values():
        assert op in everything, op
    # every operation is RRIEngine's own, and every RRIEngine method that reaches such a function is an operation or excluded
    from rri_nmf_amd.engine import RRIEngine
    esrc = open(os.path.join(ROOT, 'rri_nmf_amd', 'engine.py')).read()
    assert everything == set(cs.OP_METHODS), sorted(everything ^ set(cs.OP_METHODS))
    used = set()
    for op, methods in cs.OP_METHODS.items():
        for meth in methods:
            assert callable(getattr(RRIEngine, meth)), (op, meth)
            used.add(meth)
    entry_points = {fn for fn in cs.COVERAGE if fn.startswith('rri_')} | {'rri_apply_reset_vectors', 'rri_sweep', 'rri_update_T_row',
                                                                           'rri_update_W_col', 'rri_apply_reset_max_resid'}
    for mm in re.finditer(r'\n    def (\w+)\(self.*?(?=\n    def |\Z)', esrc, flags=re.S):
        meth, body = mm.group(1), mm.group(0)
        called = set(re.findall(r'_lib\.(rri_\w+)', body))
        if called & entry_points and not meth.startswith('_resolve') and meth not in ('sweep_until', 'attach_group'):
            assert meth in used or meth in cs.EXCLUDED_METHODS, meth
    for meth in cs.EXCLUDED_METHODS:
        assert meth == 'apply_reset_max_resid' or hasattr(RRIEngine, meth), meth
    assert not hasattr(RRIEngine, 'apply_reset_max_resid')


def test_every_entry_point_of_the_header_is_classified():
    """every `rri_status rri_*(` declared in include/rri_hip.h stands in exactly one of cs.COVERAGE (it calls changed()), cs.NO_CHANGED
    (it calls none and is in an alphabet all the same) and cs.EXCLUDED_ENTRY_POINTS (with a reason)"""
    header = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    declared = re.findall(r'^rri_status\s+(rri_\w+)\s*\(', header, flags=re.M)
    assert len(declared) >= 91 and len(set(declared)) == len(declared), len(declared)
    everything = set(cs.DIRECTED_ONLY)
    for flavour in cs.RANDOM_FLAVOURS:
        everything |= set(cs.alphabet(flavour))
    for fn in declared:
        where = [name for name, table in (('COVERAGE', cs.COVERAGE), ('NO_CHANGED', cs.NO_CHANGED), ('EXCLUDED_ENTRY_POINTS', cs.EXCLUDED_ENTRY_POINTS))
                 if fn in table]
        assert len(where) == 1, '%s is in %s: classify it in tests/cs_cases.py' % (fn, where or 'none of COVERAGE, NO_CHANGED, EXCLUDED_ENTRY_POINTS')
    for table in (cs.NO_CHANGED, cs.EXCLUDED_ENTRY_POINTS):
        assert set(table) <= set(declared), sorted(set(table) - set(declared))
    assert {fn for fn in cs.COVERAGE if fn.startswith('rri_')} <= set(declared)
    for fn, reason in cs.EXCLUDED_ENTRY_POINTS.items():
        assert isinstance(reason, str) and len(reason) > 10, fn
    for fn, op in cs.NO_CHANGED.items():
        assert op in everything, (fn, op)


def test_every_public_engine_method_that_calls_the_library_is_classified():
    """every public method of RRIEngine whose body calls _lib.rri_* is the method of an operation (cs.OP_METHODS) or stands in
    cs.EXCLUDED_METHODS"""
    from rri_nmf_amd.engine import RRIEngine
    esrc = open(os.path.join(ROOT, 'rri_nmf_amd', 'engine.py')).read()
    esrc = esrc[esrc.index('\nclass RRIEngine('):]
    used = {meth for methods in cs.OP_METHODS.values() for meth in methods}
    found = 0
    for mm in re.finditer(r'\n    def (\w+)\(self.*?(?=\n    def |\n\S|\Z)', esrc, flags=re.S):
        meth, body = mm.group(1), mm.group(0)
        if meth.startswith('_') or not re.search(r'_lib\.rri_\w+', body):
            continue
        found += 1
        assert hasattr(RRIEngine, meth)              # (a method or a property)
        assert (meth in used) != (meth in cs.EXCLUDED_METHODS), '%s: an operation of cs.OP_METHODS or a line of cs.EXCLUDED_METHODS, one of the two' % meth
    assert found > 60, found


@pytest.mark.parametrize('flavour', cs.NEW_FLAVOURS)
def test_every_new_operation_stands_between_two_sweeps_or_objectives(flavour):
    """over the 24 default seeds every operation on the flavour's own state stands directly between a sweep or an objective before
    it and one after it in at least 6 sequences"""
    behind = ('sweep', 'objective', 'objective_parts')
    own = cs.new_ops(flavour)
    assert own == {'gram-frozen': cs.FROZEN_OPS, 'gram-frozen-fp32': cs.FROZEN_OPS, 'csr-frozen': cs.FROZEN_OPS + ['upload_X_corpus'],
                   'csr-uniform': cs.UNIFORM_OPS + ['upload_X_corpus']}[flavour]
    count = dict.fromkeys(own, 0)
    for seed in range(cs.DEFAULT_SEEDS):
        names = [o.name for o in cs.random_sequence(flavour, seed)]
        for name in own:
            count[name] += any(names[i] == name and names[i - 1] in behind and names[i + 1] in behind for i in range(1, len(names) - 1))
    print(flavour, count)
    assert min(count.values()) >= 6, count


def test_the_alphabets_of_the_new_flavours():
    plain, csr = cs.ALPHABET['plain'], cs.ALPHABET['csr']
    borrowers = cs.BORROWERS
    assert cs.alphabet('gram-frozen') == plain + cs.FROZEN_OPS + borrowers
    assert cs.alphabet('gram-frozen-fp32') == [o for o in plain if o not in ('scale_X', 'preprocess')] + ['bind_X'] + cs.FROZEN_OPS + borrowers
    assert cs.alphabet('csr-frozen') == csr + cs.FROZEN_OPS + ['upload_X_corpus'] + borrowers + cs.CORPUS_BORROWERS
    assert cs.alphabet('csr-uniform') == csr + cs.UNIFORM_OPS + ['upload_X_corpus'] + borrowers + cs.CORPUS_BORROWERS
    for flavour in cs.RANDOM_FLAVOURS:
        if flavour not in cs.NEW_FLAVOURS + cs.EARLY_FLAVOURS:      # the borrowers went into the LOOK alphabets of the flavours that came after 'gram-u8' only
            assert not set(cs.alphabet(flavour)) & set(borrowers + cs.CORPUS_BORROWERS + cs.FROZEN_OPS + cs.UNIFORM_OPS + ['upload_X_corpus'])
    # the three flavours on the early-sums schedule: the alphabets of their twins and the borrowers, no state of their own
    for flavour, twin in zip(cs.EARLY_FLAVOURS, ('gram-phases', 'gram-fp32', 'gram-u8')):
        assert cs.alphabet(flavour) == cs.alphabet(twin) + borrowers and cs.new_ops(flavour) == [], flavour
        assert {key: cs.FLAVOURS[flavour][key] for key in ('kind', 'dtype', 'd')} == {key: cs.FLAVOURS[twin][key] for key in ('kind', 'dtype', 'd')}
        assert cs.FLAVOURS[flavour]['env'] == {'RRI_ONCHIP': '0', 'RRI_TROW_SMALL': '0'}, flavour
    assert cs.FLAVOURS['gram-frozen']['env'] == {'RRI_ONCHIP': '1'} and cs.FLAVOURS['gram-frozen-fp32']['d'] == cs.D_F32
    assert cs.factor_tol('gram-frozen-fp32') == 1e-7 and cs.Model('csr-uniform').U.size > 0


def test_persistent_sweeps_follow_the_statistics():
    ops = [cs.Op(*x) for x in (('sweep', 2), ('set_frozen', 1), ('sweep', 1), ('absorb', 0.9), ('sweep', 1), ('clear_frozen',), ('sweep', 1),
                               ('absorb', 1.0), ('sweep', 1), ('set_params', 'fix_T'), ('sweep', 1))]
    assert cs.persistent_sweeps(ops) == 2
    assert cs.persistent_sweeps(cs.CASES['frozen-obj_track-clear'].ops) == 2


@pytest.mark.parametrize('borrower', cs.BORROWERS + cs.CORPUS_BORROWERS + ['absorb'])
def test_a_borrower_that_scored_the_factors_of_before_fails_its_check(borrower):
    """sweep(1), the borrower: the answer taken from the W and T of BEFORE the sweep (by the feature's own restatement) fails
    cs.check_borrowed, the one taken from the current ones passes.  The two co-occurrence calls read neither W nor T -- their
    counts are those of the corpus they are given and cannot be stale in that sense -- so for them only the second half holds,
    and an answer for other words fails"""
    flavour = 'csr-frozen' if borrower in cs.CORPUS_BORROWERS else 'gram-frozen'
    m = cs.Model(flavour)
    W0, T0 = m.W.copy(), m.T.copy()
    m.apply(cs.Op('sweep', 1))
    if borrower == 'absorb':
        import frozen_cases as fc
        from rri_nmf_amd.engine import FrozenRows
        want = fc.stats_of(m.X, m.W)
        cs.check_frozen(FrozenRows(*want), want, absorbed=(m.X, m.W, 1.0, None))
        with pytest.raises(AssertionError):
            cs.check_frozen(FrozenRows(*fc.stats_of(m.X, W0)), want, absorbed=(m.X, m.W, 1.0, None))
        return
    kw = cs.borrow_inputs(borrower, m.d, 7, m.X)
    answer = cs.reference_answer(borrower, m.W, m.T, kw)
    if borrower == 'rank_entries':
        from rri_nmf_amd.engine import RankResult
        as_result = lambda r: RankResult(*r)
    else:
        as_result = lambda r: r
    cs.check_borrowed(borrower, m.W, m.T, kw, as_result(answer))
    if borrower in ('cooccurrence_counts', 'corpus_cooc'):
        stale = cs.reference_answer(borrower, m.W, m.T, dict(kw, words=cs.borrow_inputs(borrower, m.d, 8, m.X)['words']))
    else:
        stale = cs.reference_answer(borrower, W0, T0, kw)
    with pytest.raises(AssertionError):
        cs.check_borrowed(borrower, m.W, m.T, kw, as_result(stale))


@pytest.mark.parametrize('flavour', cs.RANDOM_FLAVOURS)
def test_the_random_sequences_meet_their_quotas(flavour):
    seen = set()
    for seed in range(cs.DEFAULT_SEEDS):
        ops = cs.random_sequence(flavour, seed)
        assert len(ops) == cs.SEQ_LEN
        assert [repr(o) for o in ops] == [repr(o) for o in cs.random_sequence(flavour, seed)]       # seeded
        names = [o.name for o in ops]
        assert set(names) <= set(cs.alphabet(flavour))
        assert sum(cs.category(x) == cs.STATE for x in names) >= cs.SEQ_LEN // 2, names
        assert sum(cs.category(x) == cs.LOOK for x in names) >= 3, names
        assert repr(ops[-2]) == 'sweep(1)' and repr(ops[-1]) == 'objective'
        seen |= set(names)
    assert seen == set(cs.alphabet(flavour)), 'never drawn in the default seeds: %s' % sorted(set(cs.alphabet(flavour)) - seen)


def test_the_sequences_of_the_earlier_flavours_are_what_they_were():
    """draw_sequence seeds by the position of a flavour in RANDOM_FLAVOURS and draws nothing more from its generator for a flavour
    without operations of its own (cs.new_ops): the four new flavours are appended after 'gram-u8', so the 24 default sequences of
    the eight flavours before them, and their redraws, are those that ran before they existed (the digests -- the first 16 hex
    digits of a sha256 per flavour -- were taken from the module as it was then)"""
    import hashlib
    earlier = {'gram-onchip': '45bbf291725351b2', 'gram-phases': '19883f57ff211b84', 'residual': 'c7214b4a5f8f5a9b', 'weighted': 'b33bae3231fea92d',
               'pattern': 'd61e7ca1a6c2ccf5', 'csr': '7d5639a21a7150a8', 'gram-fp32': 'ac38742c61bd4f9f', 'gram-u8': 'd9b8aea59e7e0128'}
    # the earlier lists as they were, as a prefix; the three flavours of the early-sums schedule behind them, in this order
    assert cs.RANDOM_FLAVOURS[:12] == list(earlier) + cs.NEW_FLAVOURS and list(cs.FLAVOURS)[-7:-3] == cs.NEW_FLAVOURS
    assert cs.NEW_FLAVOURS == ['gram-frozen', 'gram-frozen-fp32', 'csr-frozen', 'csr-uniform']
    assert cs.RANDOM_FLAVOURS[12:] == cs.EARLY_FLAVOURS == list(cs.FLAVOURS)[-3:] == ['gram-early', 'gram-early-fp32', 'gram-early-u8']
    for flavour, digest in earlier.items():
        h = hashlib.sha256()
        for seed in range(24):
            h.update(repr((flavour, seed, cs.random_sequence(flavour, seed))).encode())
        assert h.hexdigest()[:16] == digest, flavour
    h = hashlib.sha256()        # and the digest over the first seven together that this test held before
    for flavour in list(earlier)[:7]:
        for seed in range(24):
            h.update(repr((flavour, seed, cs.random_sequence(flavour, seed))).encode())
    assert h.hexdigest() == '9e0401d0fbd8dd1ea8897eb0db008bf5d8f96a8aaf8410c89329acce878e7085'
    before = {('gram-onchip', 2): 1, ('gram-onchip', 3): 1, ('gram-onchip', 7): 1, ('gram-onchip', 9): 1, ('gram-onchip', 13): 1,
              ('gram-onchip', 19): 1, ('gram-phases', 14): 1, ('residual', 10): 1, ('residual', 13): 1, ('csr', 3): 1, ('csr', 6): 1,
              ('csr', 10): 1, ('csr', 12): 1, ('csr', 22): 1, ('gram-fp32', 9): 1, ('gram-u8', 21): 1}
    assert {key: val for key, val in cs.REDRAWS.items() if key[0] not in cs.NEW_FLAVOURS + cs.EARLY_FLAVOURS} == before
    assert {key: val for key, val in cs.REDRAWS.items() if key[0] in cs.NEW_FLAVOURS} == {('gram-frozen', 6): 1, ('csr-uniform', 12): 1, ('csr-uniform', 17): 1}


def test_early_sweeps_counts_the_sweeps_on_the_schedule():
    """cs.early_sweeps: free, clipped and penalised sweeps run on the early-sums schedule, sweeps with a factor fixed or T projected
    do not, and the sweep that a case expects to raise is not counted; every default sequence of the three flavours ends in one"""
    ops = [cs.Op(*x) for x in (('sweep', 2), ('set_params', 'fix_T'), ('sweep', 1), ('set_params', 'pen_a'), ('sweep', 1), ('set_params', 'simplex'),
                               ('sweep', 1), ('set_params', 'clip'), ('update_T_row', 1), ('sweep', 1), ('set_params', 'fix_W'), ('sweep', 1))]
    assert cs.early_sweeps(ops) == 3 and cs.early_sweeps(ops, raises=0) == 2
    assert [cs.early_schedule(p) for p in sorted(cs.PARAMS)] == [True, False, False, True, True, True, False], sorted(cs.PARAMS)
    for flavour in cs.EARLY_FLAVOURS:
        for seed in range(cs.DEFAULT_SEEDS):
            ops = cs.random_sequence(flavour, seed)
            ls = cs.LegalState('plain')
            for op in ops[:-2]:
                ls.follow(op)
            assert cs.early_sweeps(ops) >= 1 or not cs.early_schedule(ls.pname), (flavour, seed)     # (the last two: sweep(1), objective)
    case = cs.CASES['early-ended-zero_column']
    assert cs.early_sweeps(case.ops, raises=case.raises) == 2


def test_the_uint8_model_keeps_counts_and_scales_consistent_with_its_X():
    """after every operation of every default sequence the model's X is (C * s) * r[:, None] of the C, r, s it holds (to the
    rounding of preprocess, which takes X from the oracle), and a new X has both vectors at one"""
    for seed in range(cs.DEFAULT_SEEDS):
        m = cs.Model('gram-u8')
        for op in cs.random_sequence('gram-u8', seed):
            m.apply(op)
            assert cs.relfro(cs.scaled_counts(m.C, m.r, m.s), m.X) < 1e-14, (seed, op)
            assert np.array_equal(m.C, np.round(m.C)) and m.C.min() == 0 and m.C.max() <= 255
            if op.name in ('upload_X', 'bind_X'):
                assert np.array_equal(m.r, np.ones(cs.N)) and np.array_equal(m.s, np.ones(m.d)) and np.array_equal(m.X, m.C)


@pytest.mark.parametrize('flavour', cs.RANDOM_FLAVOURS)
def test_no_default_sequence_meets_a_reset_a_dead_column_or_an_exception(flavour):
    """on the model alone, chained (cs_cases.healthy): Model.sweep_from asserts that no reset was used, the oracle asserts on a
    column that sums to 0 and raises on an unbounded step, and every operation is legal where it stands; and the redraws written
    down in cs_cases.REDRAWS are the first healthy draws, no more"""
    for seed in range(cs.DEFAULT_SEEDS):
        assert cs.healthy(flavour, cs.random_sequence(flavour, seed)), (flavour, seed)
        for attempt in range(cs.REDRAWS.get((flavour, seed), 0)):
            assert not cs.healthy(flavour, cs.draw_sequence(flavour, seed, attempt)), (flavour, seed, attempt)
