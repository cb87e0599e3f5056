"""No device: (1) the case lists of tests/wsb_cases.py reach every bucket of the blocked CSR store and of the dense weighted step
in each storage type, by the layout formulas restated there (the GPU module checks those against what a handle reports);
(2) the rounding bounds of StepBound hold for a numpy emulation of the stored residual, and are sharp enough to see the faults
these kernels can have: (a) one entry of a segment dropped from a sum, (b) one pad counted as a copy of its neighbour,
(c) one entry's correction skipped for one topic step, (d) one block's partial sums left out, and, for float64 storage,
(e) one stored entry off by 2^-24 relative.  Faults (a) and (b) are placed twice: where they are largest, and at the entry of
median size (a typical place: of the longest column, or among the padded columns), where they are looked for in wR and nw,
both of which they move; at its largest place (a) must show in wR alone and in nw alone.  (c) is injected in the first topic
step only and looked for in that step's W column; (d) and (e) sit where they are largest.  What the bounds do NOT see: an fp32
bound grows with the segment, a single entry does not -- at the 908-entry segment of the list the smallest relative error of
the largest term that still shows is 4.5e-3 (fp32) and 6.8e-8 (float64), so fault (e), 6.0e-8, is seen at the largest term of
a matrix but not inside its longest segment.  The dense weighted cases (no factor tables, non-binary weights, the topic flags,
W fixed) go through the same emulation.  RRI_TEST_RATIOS=1 prints the worst error / bound and the smallest fault / bound."""
import os

import numpy as np
import pytest

import wsb_cases as wc

RUNS = wc.blocked_runs()
PAT = [r for r in RUNS if r[3] == 'pat']


def test_case_list_reaches_every_bucket_of_the_blocked_store():
    seen = {}
    for run in RUNS:
        name, make, k, flavour, store = run
        L = wc.sp_layout(make(), store, flavour == 'csrx')
        wc.bucket_claims(name, L, store, flavour == 'csrx')
        s = seen.setdefault((flavour, store), set())
        for w, copy in enumerate(('csr', 'csc')):
            c = L[w]
            s.add('lps=%d-%s' % (c['lps'], copy))
            if c['avg'] in (191, 192, 383, 384, 767, 768):
                s.add('avg=%d-%s' % (c['avg'], copy))
            cap = wc.sp_block_cap(store, flavour == 'csrx')
            if c['gdim'] in (cap, cap + 1, 2 * cap + 1):
                s.add('gdim=%s-%s' % ({cap: 'cap', cap + 1: 'cap+1'}.get(c['gdim'], '2cap+1'), copy))
            lens = set(c['seg_len'].ravel().tolist())
            full = 4 * c['lps'] * 8
            if {0, 1, 3, 4, 5, full - 1, full, full + 1} <= lens:
                s.add('seglen-%s' % copy)
            per_block = np.bincount([x[0] for x in c['work']], minlength=c['nblk'])
            if per_block.max() >= 2 and per_block.min() == 1:
                s.add('items-many-and-one')
        s.add('k=1' if k == 1 else 'k>64' if k > 64 else 'k=5')
        if name.startswith('empty-zeros-heavy'):
            s.add('empty-zeros-heavy')
    need = {'items-many-and-one', 'k=1', 'k=5', 'k>64', 'empty-zeros-heavy'}
    for copy in ('csr', 'csc'):
        need |= {'lps=%d-%s' % (v, copy) for v in (8, 16, 32, 64)}
        need |= {'avg=%d-%s' % (v, copy) for v in (191, 192, 383, 384, 767, 768)}
        need |= {'gdim=%s-%s' % (v, copy) for v in ('cap', 'cap+1', '2cap+1')}
        need.add('seglen-%s' % copy)
    for key, s in seen.items():
        assert need <= s, '%s: no case for %s' % (key, sorted(need - s))
    assert len(seen) == 4


def test_case_list_reaches_every_route_of_the_dense_weighted_step():
    cases = wc.dense_cases()
    for store in wc.STORES:
        seen = set()
        for name, n, d, k, make_mask, env, routes, flags in cases:
            lay = wc.dense_layout(n, d, store)
            M = make_mask()
            assert lay['LD'] > d, 'd is ragged: the row stride exceeds it'
            if 'nrb' in routes:
                assert lay['nrb'] == routes['nrb'] and lay['wtrow_small'] == routes['wtrow_small'], (name, lay)
                seen.add('nrb=%d' % lay['nrb'])
            binary = bool(np.isin(M, (0.0, 1.0)).all())
            dens = float((M != 0).mean())
            bits = binary and env.get('RRI_MASK_BITS') != '0'
            assert routes.get('mask_bits', bits) == bits, name
            cols = bits and dens <= 0.12 and env.get('RRI_WMCORR_COLS') != '0'
            assert routes.get('mask_cols', cols) == cols, (name, dens)
            if 'nw_from_mask' in routes:
                assert routes['nw_from_mask'] == (cols and env.get('RRI_WNW_MASK') != '0'), name
            seen.add(('bits' if bits else 'stored-weights' if not binary else 'stored-01') + ('-cols' if cols else ''))
            if bits and not env and flags == 'plain' and n == 203:
                seen.add('density %s 0.12' % ('<=' if dens <= 0.12 else '>'))
            for key in env:
                seen.add('%s=0 at density %s 0.12' % (key, '<=' if dens <= 0.12 else '>'))
            seen.add(flags)
            if not M[17].any() and not M[:, 64].any():
                seen.add('zero row and column')
            if M.all():
                seen.add('ones')
        n, d = wc.BIG[store]
        lay = wc.dense_layout(n, d, store)
        assert lay['npanels'] >= 2 and not lay['interleaved'] and not lay['wtrow_small'], lay
        # ... and it is the smallest n (in steps of 100 rows) that gets there at this d
        assert wc.dense_layout(n - 100, d, store)['interleaved']
        need = {'nrb=64', 'nrb=65', 'bits', 'bits-cols', 'stored-weights', 'stored-01', 'density <= 0.12', 'density > 0.12',
                'plain', 'topic', 'fix_W', 'zero row and column', 'ones'}
        need |= {'%s=0 at density %s 0.12' % (key, side) for key in ('RRI_WMCORR_COLS', 'RRI_WNW_MASK') for side in ('<=', '>')}
        need.add('RRI_MASK_BITS=0 at density > 0.12')
        assert need <= seen, (store, sorted(need - seen))


def _faults(step, L1):
    """(name, ((|change of wR_j|, its bound), (|change of nw_j|, its bound))) for the single-step faults at this step: each of
    them moves both sums of its column, and a test that checks both sees it in either"""
    E, w, M = step['E'], step['w'], step['M']
    contrib = np.abs(w[:, None] * E) * M
    both = lambda i, j: ((contrib[i, j], step['b_wR'][j]), (w[i] ** 2 * M[i, j], step['b_nw'][j]))
    out = []
    i, j = np.unravel_index(np.argmax(contrib), contrib.shape)
    out.append(('a', both(i, j)[:1]))                                         # one entry dropped: the largest of the matrix, in wR
    out.append(('a-nw', both(i, j)[1:]))                                      # ... and in nw alone
    jl = int(np.argmax((M != 0).sum(axis=0)))                                 # ... and one of median size in the longest column
    rows = np.flatnonzero(M[:, jl])
    im = rows[np.argsort(contrib[rows, jl])[rows.size // 2]]
    if w[im] != 0:
        out.append(('a-median', both(im, jl)))
    lens = (M != 0).sum(axis=0).astype(int)
    padded = np.flatnonzero(lens % 4)
    if padded.size:                                                           # a pad read as a copy of the segment's last entry
        last = np.array([np.flatnonzero(M[:, c])[-1] for c in padded])
        v = contrib[last, padded]
        out.append(('b', both(last[np.argmax(v)], padded[np.argmax(v)])[:1]))
        live = np.flatnonzero(w[last] != 0)                                   # (a last entry whose w is zero adds nothing, rightly)
        if live.size:
            c = live[np.argsort(v[live])[live.size // 2]]
            out.append(('b-median', both(last[c], padded[c])))
    bw = L1['bw']                                                             # the row blocks of the column copy
    part = np.abs((w[:bw, None] * E[:bw]).sum(axis=0))
    j = int(np.argmax(part))
    out.append(('d', ((part[j], step['b_wR'][j]),)))
    return out


def _walk(name, Xs, M, W0, T0, store, tables, flags, L1=None):
    """the emulation stays inside every bound; with L1 (the column copy's layout) the faults fall outside.  Returns
    (worst error / bound, smallest fault / bound per fault, the first step)"""
    worst, seen, first = 0.0, {}, None
    steps = []
    for step in wc.emulate(Xs, M, W0, T0, store, tables, flags):
        steps.append(step)
        a = step['w'] @ step['E']
        nw = (step['w'] ** 2) @ step['M']
        for got, want, bound in ((a + step['trow'] * nw, step['wR'], step['b_wR']), (nw, step['nw'], step['b_nw'])):
            ok = bound > 0
            assert (np.abs(got - want) <= bound).all(), (name, step['sweep'], step['t'])
            worst = max(worst, float((np.abs(got - want)[ok] / bound[ok]).max()) if ok.any() else 0.0)
        if L1 is not None:
            for f, sums in _faults(step, L1):
                ratio = max(change / bound if bound > 0 else np.inf for change, bound in sums if change > 0 or bound > 0)
                assert ratio > 1, 'fault (%s) hides inside the bounds (change, bound: %r) at sweep %d topic %d' % (
                    f, sums, step['sweep'], step['t'])
                seen[f] = min(seen.get(f, np.inf), ratio)
            if store == 'fp64':                     # (e) one stored entry off by 2^-24 relative
                contrib = np.abs(step['w'][:, None] * step['E']) * step['M']
                i, j = np.unravel_index(np.argmax(contrib), contrib.shape)
                assert contrib[i, j] * 2.0 ** -24 > step['b_wR'][j], (name, contrib[i, j] * 2.0 ** -24, step['b_wR'][j])
            jl = int(np.argmax(step['M'].sum(axis=0)))      # the longest column: the relative fault of its largest term still seen
            top = float((np.abs(step['w'][:, None] * step['E']) * step['M'])[:, jl].max())
            seen['rel'] = max(seen.get('rel', 0.0), step['b_wR'][jl] / top if top > 0 else 0.0)
    for step in steps:       # the T row and the W column, which the emulation fills in once the step has run
        pairs = [(step['trow_emu'], step['trow_new'], step['b_trow'])]
        if 'x' in step:
            pairs.append((step['x_emu'], step['x'], step['bx']))
        for got, want, bound in pairs:
            ok = bound > 0
            assert (np.abs(got - want) <= bound).all(), (name, step['sweep'], step['t'])
            worst = max(worst, float((np.abs(got - want)[ok] / bound[ok]).max()) if ok.any() else 0.0)
    return worst, seen, steps[0]


@pytest.mark.parametrize('run', PAT, ids=[wc.run_id(r) for r in PAT])
def test_bounds_hold_for_an_emulated_residual_and_see_single_faults(run):
    name, make, k, _, store = run
    A, W0, T0 = wc.planted(make(), k)
    Xs, M = wc.pattern_problem(A, store)
    L1 = wc.sp_copy_layout(A, 1, store, False)
    worst, seen, first = _walk(name, Xs, M, W0, T0, store, True, {}, L1)
    # (c) one entry misses the T-row correction of the first step: the W column of that step shows it
    amp = np.abs(first['w'][:, None] * first['dt'][None, :] * (first['trow'] + first['dt'])[None, :]) * first['M']
    i, j = np.unravel_index(np.argmax(amp), amp.shape)
    gen = wc.emulate(Xs, M, W0, T0, store, True, sweeps=1, skip=(0, 0, int(i), int(j)))
    faulty = next(gen)
    try:
        next(gen)
    except StopIteration:
        pass
    assert abs(faulty['x_emu'][i] - faulty['x'][i]) > faulty['bx'][i], (
        'fault (c) hides inside the bound', name, abs(faulty['x_emu'][i] - faulty['x'][i]), faulty['bx'][i])
    if os.environ.get('RRI_TEST_RATIOS', '0') == '1':
        seg = int(max(wc.sp_copy_layout(A, w, store, False)['seg_len'].max() for w in (0, 1)))
        print('\nEMU %-50s worst error/bound %.3g; smallest fault/bound %s; longest segment %d' % (
            wc.run_id(run), worst, ' '.join('%s %.3g' % kv for kv in sorted(seen.items())), seg))


DENSE = wc.dense_cases()


@pytest.mark.parametrize('store', list(wc.STORES))
@pytest.mark.parametrize('case', DENSE, ids=[c[0] for c in DENSE])
def test_bounds_hold_for_the_emulated_dense_weighted_cases(case, store):
    """the dense cases of the GPU module (no factor tables; non-binary weights, the topic flags, W fixed): the same emulation
    inside the same bounds.  The two 36100-row shapes are left to the device: they add rows, no other arithmetic."""
    name, n, d, k, make_mask, env, routes, flags_name = case
    M = make_mask()
    X, W0, T0 = wc.planted_dense(n, d, k, M)
    Xs = np.asarray(X.astype(wc.STORES[store]), dtype=np.float64)
    flags = dict(wc.STEP_FLAGS[flags_name])
    if flags.get('project_T_each_iter'):
        T0 = T0 / T0.sum(axis=1, keepdims=True) * flags['t_row_sum']
    worst, _, _ = _walk(name, Xs, M, W0, T0, store, False, flags)
    if os.environ.get('RRI_TEST_RATIOS', '0') == '1':
        print('\nEMU-DENSE %-40s %s worst error/bound %.3g' % (name, store, worst))
