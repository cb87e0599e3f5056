"""tests/onchip_cases.py itself, without a GPU: every named edge is what its name says under geometry(), at 256, 128, 64 and 32
CUs; no two cases of one CU count meet the same instantiation and geometry; the eligible ones stay small; and every verdict
case gives, on the float64 oracle alone, the outcome it claims."""
import numpy as np
import pytest

import onchip_cases as oc

N_CUS = (256, 128, 64, 32)


def _empty_and_last(case, g):
    used = -(-case.n // g['rows_wg'])
    return g['G'] - used, case.n - (used - 1) * g['rows_wg']


@pytest.mark.parametrize('n_cu', N_CUS)
def test_every_edge_is_what_its_name_says(n_cu):
    cases, claims = oc.edge_cases(n_cu), oc.edge_claims(n_cu)
    assert len(cases) == len(claims) == len(set(c.name for c in cases))
    for c in cases:
        g = oc.geometry(c.n, c.d, c.k, c.store, oc.projected(c.flags), n_cu)
        assert g['eligible'] == c.expect_eligible, (c.name, g)
        assert g['G'] == min(n_cu, 256)
        claim = dict(claims[c.name])
        if 'refused' in claim:
            # refused by the limit the name moves past, and by nothing else
            assert g['refusals'] == [claim.pop('refused')], (c.name, g['refusals'])
        else:
            assert g['refusals'] == [], (c.name, g['refusals'])
        if 'empty' in claim:
            assert _empty_and_last(c, g) == (claim.pop('empty'), claim.pop('last')), (c.name, _empty_and_last(c, g))
        for key, want in claim.items():
            assert g[key] == want, (c.name, key, g[key], want)


@pytest.mark.parametrize('n_cu', N_CUS)
def test_both_sides_of_every_limit(n_cu):
    """the pairs: one step in n, d or k, and exactly the named value of the geometry moves"""
    by = {c.name: c for c in oc.edge_cases(n_cu)}
    geo = lambda c: oc.geometry(c.n, c.d, c.k, c.store, oc.projected(c.flags), n_cu)
    pairs = 0
    for name, c in by.items():
        for a, b, key in (('rpw-few-', 'rpw-few+1-', 'few'), ('rpw-cap-', 'rpw-cap+1-', 'eligible'), ('wlds-94rows', 'wlds-95rows', 'eligible')):
            if name.startswith(a):
                other = by[name.replace(a, b, 1)]
                ga, gb = geo(c), geo(other)
                assert other.n == c.n + 1 and (other.d, other.k, other.store, other.flags) == (c.d, c.k, c.store, c.flags)
                assert ga[key] is True and gb[key] is False, (name, key)
                assert ga['rows_wg'] + 1 == gb['rows_wg'] and ga['CG'] == gb['CG'] and ga['KT'] == gb['KT']
                pairs += 1
    # few -> most and the cap of each of 2 storage types x plain / projected (x KT 3 / 8 for the caps), and the LDS copy of W
    assert pairs == 4 + 8 + 1, pairs
    steps = {('cols-d32', 'cols-d33'): ('NA', 1, 2), ('cols-d256', 'cols-d257'): ('CG', 1, 2), ('cols-d512', 'cols-d513'): ('CG', 2, 4),
             ('rank-k22', 'rank-k23'): ('KT', 3, 8)}
    if n_cu > 32:
        steps[('cols-d1024', 'cols-d1025')] = ('CG', 4, 8)
    for (a, b), (key, va, vb) in steps.items():
        for tail in ('-fp32-plain', '-fp64-plain'):
            assert geo(by[a + tail])[key] == va and geo(by[b + tail])[key] == vb, (a, b, tail)
    for store in ('fp32', 'fp64'):         # the projection loses eligibility at LD = 1025, and only it
        ga, gb = geo(by['cols-d1024-%s-tm' % store]), geo(by['cols-d1025-%s-tm' % store])
        assert ga['eligible'] and ga['CG'] == 4 and gb['refusals'] == ['LD']
    for store, d in (('fp32', 253), ('fp64', 255)):           # LD = 256 from a padded and from an unpadded d
        ga, gb = geo(by['cols-d%d-%s-plain' % (d, store)]), geo(by['cols-d256-%s-plain' % store])
        assert ga['LD'] == gb['LD'] == 256 and ga['CG'] == gb['CG'] == 1
    for k, ks in ((2, 3), (3, 3), (46, 47), (47, 47), (63, 63), (64, 65)):
        assert geo(by['rank-k%d-fp32-plain' % k])['kS'] == ks
    assert geo(by['rank-k65-fp32-plain'])['refusals'] == ['k'] and geo(by['cols-d2049-fp32-plain'])['refusals'] == ['LD']


@pytest.mark.parametrize('n_cu', N_CUS)
def test_no_two_cases_share_a_signature_and_the_eligible_ones_are_small(n_cu):
    seen = {}
    for c in oc.edge_cases(n_cu):
        sig = oc.signature(c, n_cu)
        assert sig not in seen, (c.name, seen[sig], sig)
        seen[sig] = c.name
        if c.expect_eligible:
            assert c.n * c.d * np.dtype(oc.STORES[c.store]).itemsize < 64e6, c.name
    # both storage types, both flag sets, both KT, few and most all occur among the eligible cases
    inst = set(s[:4] for s in seen if len(s) > 6)
    assert len(inst) == 16, sorted(inst)


def test_what_is_dropped_is_counted_and_nothing_is_dropped_at_256_cus(capsys):
    names = [c.name for c in oc.edge_cases(256)]
    assert oc.edge_dropped(256) == []
    for n_cu in N_CUS:
        kept, dropped = [c.name for c in oc.edge_cases(n_cu)], oc.edge_dropped(n_cu)
        assert sorted(kept + dropped) == sorted(names)            # the same names at every CU count: test ids are stable
        with capsys.disabled():
            print('\nn_cu = %3d: %d edge cases, %d dropped (NA > G)' % (n_cu, len(kept), len(dropped)), end='')
        if n_cu >= 64:
            assert dropped == []
        else:
            # 32 workgroups hold 32 slices of 32 columns: nothing wider than 1024 columns has a shape
            by = {c.name: c for c in oc.edge_cases(256)}
            assert dropped and all(by[name].d > 1024 for name in dropped)
    assert len(names) >= 80


def test_the_lds_block_never_refuses_what_the_other_limits_admit():
    worst = 0
    for k in range(2, oc.MAX_K + 1):
        for CG in (1, 2, 4, 8):
            RG = oc.WAVES // CG
            rows = min(oc.W_LDS_DOUBLES // (k | 1), 20 * RG)
            worst = max(worst, oc.lds_bytes(rows, k, k | 1, CG))
    assert worst <= 136280 < oc.LDS_BYTES, worst


VERDICTS = oc.verdict_cases()


def test_the_verdict_table_covers_every_outcome():
    names = [v.name for v in VERDICTS]
    assert len(names) == len(set(names))
    for k, store in ((5, 'fp32'), (30, 'fp64')):
        for stem in ('wcol-no-method', 'wcol-two-die-one-reset', 'trow-budget-2', 'trow-no-method', 'tden-bounds', 'tden-one-hot',
                     'tden-not-implemented', 'tden-unbounded-dead0', 'tden-unbounded-dead%d' % (k - 1), 'wden-bounds', 'wden-unbounded'):
            assert any(n.startswith('%s-k%d-%s-' % (stem, k, store)) for n in names), (stem, k, store)
    for store in ('fp32', 'fp64'):
        for stem in ('wcol-resets-maxresid', 'wcol-budget-ends-at-last-topic', 'trow-resets', 'tiny-sums', 'tiny-sums-no-method', 'sums-just-above'):
            assert '%s-k5-%s-plain' % (stem, store) in names
        assert 'wcol-budget-runs-out-k30-%s-plain' % store in names
    assert 'wcol-resets-random-k5-fp32-plain' in names
    for v in VERDICTS:          # eligible at every CU count the tables are built for
        for n_cu in N_CUS:
            g = oc.geometry(oc.VN, oc.VD, v.k, v.store, oc.projected(v.flags), n_cu)
            assert g['eligible'] and g['KT'] == (3 if v.k == 5 else 8), (v.name, n_cu, g)


@pytest.mark.parametrize('v', VERDICTS, ids=[v.name for v in VERDICTS])
def test_every_verdict_case_is_its_outcome_on_the_oracle(v):
    X, Xs, W0, T0 = oc.verdict_problem(v)
    assert X.dtype == oc.STORES[v.store] and np.array_equal(Xs, X.astype(np.float64))
    np.random.seed(0)
    r = oc.oracle_run(Xs, W0, T0, (v.sweeps,), v.flags)
    e = v.expect
    if 'error' in e:
        assert r.error == e['error'], (r.error, e['error'])
        assert v.sweeps not in r.states
    else:
        assert r.error is None, r.error
        if e.get('resets') is not None:
            assert r.states[v.sweeps][2] == e['resets'] == len(r.log)
    if 'topics' in e:
        assert [t for _, t, _ in r.log] == e['topics'], r.log
    budget = v.flags.get('n_resets', 23)
    assert len(r.log) <= budget
    if 'budget' in v.name:                                  # the budget is spent, and the run met a dead topic after that
        assert len(r.log) == budget
        last = r.log[-1][2]
        assert any(val <= 1e-10 for _, _, step, val in r.sums if step > last)
    k = v.k
    if v.name.startswith('wcol'):
        kinds = set(kind for kind, _, _ in r.log)
        assert kinds <= {oc.EVENT_W}
    if v.name.startswith('trow'):
        assert set(kind for kind, _, _ in r.log) <= {oc.EVENT_T}
    if e.get('tiny'):
        # every sum the reset rules judged is positive and at most 1e-10
        assert len(r.sums) == 2 * k * v.sweeps and all(0.0 < val <= 1e-10 for _, _, _, val in r.sums), r.sums
    if e.get('above'):
        # every column sum of W lies just above the threshold, the last topic's (judged after the step loop) included, and no
        # row sum of T is near it: nothing resets, and a threshold of 1e-9 would reset every column
        wsums = [val for kind, _, _, val in r.sums if kind == oc.EVENT_W]
        tsums = [val for kind, _, _, val in r.sums if kind == oc.EVENT_T]
        assert len(wsums) == k and all(1e-10 < val <= 1e-9 for val in wsums), wsums
        assert all(val > 1e-9 for val in tsums), tsums
    if v.name.startswith('tden-unbounded'):
        assert v.dead is not None and not W0[:, v.dead].any()
    if v.name.startswith(('tden-bounds', 'tden-one-hot', 'wden-bounds')):
        # the branch is taken at every step: the denominator is the negative regulariser plus a squared norm far below it
        W, T, _ = r.states[v.sweeps]
        if v.name.startswith('tden-bounds'):
            assert set(np.unique(T)) <= {0.0, 2.0}
        if v.name.startswith('tden-one-hot'):
            assert set(np.unique(T)) == {0.0, 1.0} and np.all(T.sum(1) == 1.0)
        if v.name.startswith('wden-bounds'):
            assert set(np.unique(W)) <= {0.0, 0.7}
