"""The cases of tests/cs_cases.py, checked without a GPU: that their inputs can see the fault each aims at, that the written
coverage list is the code's, and that the seeded sequences are what they promise.

Every directed case whose staleness can be written in oracle terms carries a stale reference: what a handle that kept the named
value would answer (old T and X for Qt / Gfull, old X for ||X||^2, old W / T / X for the cross terms, old penalties or old
factors for the tracked objective, old mask / W / T for E; for the uint8 store the old scale vectors, also under new counts,
and the old X for the carried partial sums of topic 0).  It must lie at least 1e3 times the case's tolerance away from the true
answer.  Waived, with the reason in the case: the carry cases after a borrower and the foreign residual update (an overwritten
buffer is no value the oracle has), the legitimate stored-E path (nothing is stale) and the error case (a verdict, not a value)."""
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
                with pytest.raises((ValueError, AssertionError)):
                    m.apply(op)
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
    """draw_sequence seeds by the position of a flavour in RANDOM_FLAVOURS: the uint8 flavour is appended after all others, so the
    24 default sequences of the seven flavours before it, and their redraws, are those that ran before it existed (the digest
    was taken from the module as it was then)"""
    import hashlib
    earlier = ['gram-onchip', 'gram-phases', 'residual', 'weighted', 'pattern', 'csr', 'gram-fp32']
    assert cs.RANDOM_FLAVOURS == earlier + ['gram-u8'] and list(cs.FLAVOURS)[-1] == 'gram-u8'
    h = hashlib.sha256()
    for flavour in earlier:
        for seed in range(24):
            h.update(repr((flavour, seed, cs.random_sequence(flavour, seed))).encode())
    assert h.hexdigest() == '9e0401d0fbd8dd1ea8897eb0db008bf5d8f96a8aaf8410c89329acce878e7085'
    before = {('gram-onchip', 2): 1, ('gram-onchip', 3): 1, ('gram-onchip', 7): 1, ('gram-onchip', 9): 1, ('gram-onchip', 13): 1,
              ('gram-onchip', 19): 1, ('gram-phases', 14): 1, ('residual', 10): 1, ('residual', 13): 1, ('csr', 3): 1, ('csr', 6): 1,
              ('csr', 10): 1, ('csr', 12): 1, ('csr', 22): 1, ('gram-fp32', 9): 1}
    assert {key: val for key, val in cs.REDRAWS.items() if key[0] != 'gram-u8'} == before


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
