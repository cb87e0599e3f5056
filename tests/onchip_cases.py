"""The register-resident persistent sweep (k_onchip_sweeps) at every edge of its host geometry, and every halting verdict it can
reach: the cases of tests/test_onchip_edges_gpu.py (tests/test_onchip_cases_cpu.py checks the tables themselves, without a GPU).

Three things, none of which needs a device:

    geometry(n, d, k, store, proj, n_cu)    a SECOND WORDING of onchip_geometry / onchip_shape_ok / onchip_rpw (rri_layout.hpp) and
                                            the few-most choice of enqueue_onchip (rri_hip.hip), written from DESIGN 4.2 and the
                                            comments there -- not generated from the C++: the library's eligibility (on a device)
                                            and the header itself (tests/test_layout_cpu.py, no device) are checked against it on
                                            both sides of every limit, so when a limit moves, this file moves with it by hand
    edge_cases(n_cu)                        (name, n, d, k, store, flags, expect_eligible): one limit moves per case, everything
                                            else stays small; computed from G = min(n_cu, 256), so that on a device that reports
                                            fewer CUs the shapes still sit on the edges
    verdict_cases()                         300 x 70 at k = 5 (KT = 3) and k = 30 (KT = 8): one case per outcome of the halting
                                            rules -- resets of either kind, a budget that runs out, the reference's assertion, the
                                            branches of qf_min with a scalar denominator <= 0, sums in (0, 1e-10]

and the yardstick: oracle_run(), the float64 oracle's topic loop (oracle/rri_oracle.py:448-483 -- its own qf_min, residual
products and reset handlers) on X AS STORED, X.astype(store).astype(float64), with the resets it made and every sum it judged.

The rules restated (rri_layout.hpp "register-resident persistent sweeps" and its ONCHIP_* constants):

    LD        d rounded up to a 16-byte multiple of the storage type (4 columns of fp32, 2 of float64)
    G         min(n_cu, 256) workgroups of 8 waves
    CG        column groups of 256 columns: 1 (LD <= 256), 2 (<= 512), 4 (<= 1024), 8 (<= 2048);  RG = 8 / CG row groups
    rows_wg   ceil(n / G): the row block of a workgroup (trailing workgroups may own fewer rows, or none)
    rpw       ceil(rows_wg / RG): rows a wave holds in registers
    NA        ceil(LD / 32): workgroups that also own a 32-column slice of T
    kS        k | 1: the odd row stride of the LDS copy of W
    KT        3 (k <= 22: k + 2 Gram entries = 8 waves x 3) or 8 (k <= 64)
    RPW       every (storage, PROJ, KT) is built twice: `few` = 8 rows per wave, and the most the registers take --
              20 (KT 3), 18 (KT 8), 14 (KT 8 with the projection); float64 X takes twice the registers: 4 and 10 / 9 / 7
    refused   LD > 2048 (1024 with the projection: it stages whole T rows); k < 2 or k > 64; rpw above the cap; NA > 64 or NA > G;
              rows_wg * kS > 6144 doubles of LDS for W; the whole LDS block above 150 KiB
"""
import collections

import numpy as np

TM = dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)
STORES = {'fp32': np.float32, 'fp64': np.float64}

WAVES, CWA, PG = 8, 32, 16          # waves of a workgroup; columns of T per worker; groups of partials in the column-sum reduction
SMALL_K, MAX_K = 22, 64
RPW_FEW, RPW_MOST = 8, {(3, False): 20, (3, True): 20, (8, False): 18, (8, True): 14}     # fp32; float64 holds half of each
W_LDS_DOUBLES, LDS_BYTES = 6144, 150 * 1024


def projected(flags):
    """the topic-model instantiation: project_T_each_iter with a t_row_sum"""
    return bool(flags.get('project_T_each_iter')) and flags.get('t_row_sum') is not None


def round_up(a, m):
    return -(-a // m) * m


def rpw_of(store, proj, kt, few):
    rows = RPW_FEW if few else RPW_MOST[(kt, bool(proj))]
    return rows if store == 'fp32' else rows // 2


def lds_bytes(rows_wg, k, kS, CG):
    """the kernel's LDS block in bytes (all of it doubles): W rows, the worker's T slice, the Gram row and T T[t]^T, the
    column-sum partials, row-dot partials per column group, two row vectors, a 256-double tile per wave, the waves' 8 x 72 tiles
    of the row dots, 1024 + 40 of reduction scratch.

    The 150 KiB limit never refuses a shape that the other limits admit: rows_wg * kS <= 6144, k <= 64 (32 k <= 2048,
    2 k + 3 <= 131), rows_wg <= 20 RG so (CG + 2) rows_wg <= 20 * 8 + 2 * 160 = 480, and the fixed terms are 512 + 2048 + 4608 +
    1064: at most 17035 doubles = 136280 bytes.  No case sits on it; test_onchip_cases_cpu.py asserts this arithmetic."""
    doubles = (rows_wg * kS + k * CWA + (k + 2) + (k + 1) + PG * CWA + CG * rows_wg + 2 * rows_wg + WAVES * 256 + WAVES * 8 * 72
               + 1024 + 40)
    return 8 * doubles


def geometry(n, d, k, store, proj, n_cu):
    """dict of G, LD, CG, RG, rows_wg, rpw, NA, kS, KT, few, RPW, shmem, eligible -- and, where eligible is False, `refused`: the
    name of the first limit that refuses the shape ('k', 'LD', 'rpw', 'NA', 'w_lds', 'lds'), and `refusals`: every limit of the
    geometry that does (k and LD end the evaluation: nothing else is defined past them)"""
    vn = 4 if store == 'fp32' else 2
    g = dict(eligible=False, refused=None, refusals=[], LD=round_up(d, vn), G=min(n_cu, 256), kS=k | 1, KT=3 if k <= SMALL_K else 8)
    if k < 2 or k > MAX_K:
        g['refused'], g['refusals'] = 'k', ['k']
        return g
    if g['LD'] > (1024 if proj else 2048):
        g['refused'], g['refusals'] = 'LD', ['LD']
        return g
    LD, G = g['LD'], g['G']
    g['CG'] = 1 if LD <= 256 else 2 if LD <= 512 else 4 if LD <= 1024 else 8
    g['RG'] = WAVES // g['CG']
    g['rows_wg'] = -(-n // G)
    g['rpw'] = -(-g['rows_wg'] // g['RG'])
    g['NA'] = -(-LD // CWA)
    g['few'] = g['rpw'] <= rpw_of(store, proj, g['KT'], True)
    g['RPW'] = rpw_of(store, proj, g['KT'], g['few'])
    g['shmem'] = lds_bytes(g['rows_wg'], k, g['kS'], g['CG'])
    g['refusals'] = [name for name, hit in (('rpw', g['rpw'] > rpw_of(store, proj, g['KT'], False)),
                                            ('NA', g['NA'] > 64 or g['NA'] > G),
                                            ('w_lds', g['rows_wg'] * g['kS'] > W_LDS_DOUBLES),
                                            ('lds', g['shmem'] > LDS_BYTES)) if hit]
    g['refused'] = g['refusals'][0] if g['refusals'] else None
    g['eligible'] = g['refused'] is None
    return g


def signature(case, n_cu):
    """what two cases must not share by accident: the instantiation (storage, PROJ, KT, few) and the geometry the kernel sees,
    the pad columns, the workgroups without rows and the rows of the last non-empty one included"""
    g = geometry(case.n, case.d, case.k, case.store, projected(case.flags), n_cu)
    if not g['eligible']:
        return (case.store, projected(case.flags), g['refused'], case.n, case.d, case.k)
    r = g['rows_wg']
    used = -(-case.n // r)
    return (case.store, projected(case.flags), g['KT'], g['few'], g['CG'], r, g['NA'], case.k, g['LD'], g['LD'] - case.d,
            g['G'] - used, case.n - (used - 1) * r)


Case = collections.namedtuple('Case', 'name n d k store flags expect_eligible')


def _edge_table(n_cu):
    """(cases, claims, dropped): claims[name] is what the name says, as values of geometry() the CPU test holds it to;
    dropped names the cases that cannot be built at this n_cu (NA > G)"""
    G = min(n_cu, 256)
    cases, claims, dropped = [], {}, []

    def add(name, n, d, k, store, flags, eligible, **claim):
        proj = projected(flags)
        name = '%s-%s-%s' % (name, store, 'tm' if proj else 'plain')
        vn = 4 if store == 'fp32' else 2
        # the column slices of T need a workgroup each: at few CUs a wide case has no shape, on either side of its own limit
        if -(-round_up(d, vn) // CWA) > G and claim.get('refused') not in ('LD', 'k'):
            dropped.append(name)
            return
        cases.append(Case(name, int(n), int(d), int(k), store, dict(flags), bool(eligible)))
        claims[name] = claim

    # ---- columns: n = 2 G (every workgroup owns two rows), k = 4 -------------------------------------------------
    cg = lambda LD: 1 if LD <= 256 else 2 if LD <= 512 else 4 if LD <= 1024 else 8
    for store, flags, widths in (
            ('fp32', {}, (3, 32, 33, 253, 256, 257, 512, 513, 1024, 1025, 2046, 2048, 2049)),
            ('fp64', {}, (3, 32, 33, 255, 256, 257, 512, 513, 1024, 1025, 2046, 2048, 2049)),
            ('fp32', TM, (3, 33, 256, 257, 513, 1024, 1025)),
            ('fp64', TM, (33, 255, 257, 1024, 1025))):
        vn = 4 if store == 'fp32' else 2
        for d in widths:
            LD = round_up(d, vn)
            ok = LD <= (1024 if flags else 2048)
            claim = dict(LD=LD, CG=cg(LD), NA=-(-LD // CWA)) if ok else dict(LD=LD, refused='LD')
            add('cols-d%d' % d, 2 * G, d, 2 if d == 3 else 4, store, flags, ok, **claim)

    # ---- rows: d = 40 (one column group, eight row groups), k = 4 -------------------------------------------------
    for store, flags, ns in (('fp32', {}, ('G-1', 'G', 'G+1', '3G')), ('fp64', {}, ('G+1',)), ('fp32', TM, ('G+1',))):
        for tag in ns:
            n = {'G-1': G - 1, 'G': G, 'G+1': G + 1, '3G': 3 * G}[tag]
            add('rows-n%s' % tag, n, 40, 4, store, flags, True, rows_wg=-(-n // G), few=True, **(
                {'empty': G - (G + 2) // 2, 'last': 1 if G % 2 == 0 else 2} if tag == 'G+1' else
                {'empty': 1, 'last': 1} if tag == 'G-1' else {'empty': 0, 'last': -(-n // G)}))

    # ---- few -> most, the cap of every (storage, PROJ, KT) and one row past it -------------------------------------
    # plain flags: the CG = 8 layouts (RG = 1: rows_wg = rpw) keep n small; with the projection LD <= 1024, so CG = 4, RG = 2
    for store in ('fp32', 'fp64'):
        half = 1 if store == 'fp32' else 2
        wide, mid = (1028, 516) if store == 'fp32' else (1026, 514)
        # (at fewer than 33 CUs the 33 column slices of the wide layout have no workgroups: the plain cases take RG = 2 as well)
        for flags, d, RG in (({}, wide, 1) if G >= 64 else ({}, mid, 2), (TM, mid, 2)):
            few = RPW_FEW // half
            add('rpw-few', G * few * RG, d, 4, store, flags, True, RG=RG, rpw=few, few=True, RPW=few)
            add('rpw-few+1', G * few * RG + 1, d, 4, store, flags, True, RG=RG, rpw=few + 1, few=False,
                RPW=RPW_MOST[(3, bool(flags))] // half)
            for kt, k in ((3, 4), (8, 23)):
                cap = RPW_MOST[(kt, bool(flags))] // half
                add('rpw-cap-kt%d' % kt, G * cap * RG, d, k, store, flags, True, RG=RG, KT=kt, rpw=cap, few=False, RPW=cap)
                add('rpw-cap+1-kt%d' % kt, G * cap * RG + 1, d, k, store, flags, False, RG=RG, KT=kt, rpw=cap + 1, refused='rpw')

    # ---- the LDS copy of W: rows_wg * kS <= 6144 doubles (fp32 only: float64 holds at most 9 * 8 = 72 rows at k = 64) ------
    add('wlds-94rows', G * 94, 100, 64, 'fp32', {}, True, rows_wg=94, kS=65, KT=8)
    add('wlds-95rows', G * 94 + 1, 100, 64, 'fp32', {}, False, rows_wg=95, kS=65, refused='w_lds')

    # ---- rank: n = 2 G, d = 100 --------------------------------------------------------------------------------------
    for store, flags, ks in (('fp32', {}, (2, 3, 22, 23, 46, 47, 63, 64, 65)), ('fp64', {}, (22, 23)), ('fp32', TM, (22, 23, 64)),
                             ('fp64', TM, (23,))):
        for k in ks:
            claim = dict(refused='k') if k > MAX_K else dict(kS=k | 1, KT=3 if k <= 22 else 8)
            add('rank-k%d' % k, 2 * G, 100, k, store, flags, k <= MAX_K, **claim)
    return cases, claims, dropped


def edge_cases(n_cu):
    return _edge_table(n_cu)[0]


def edge_claims(n_cu):
    return _edge_table(n_cu)[1]


def edge_dropped(n_cu):
    return _edge_table(n_cu)[2]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
EVENT_T, EVENT_W = 1, 2         # the kinds of the engine's reset_log (RRI_EVENT_RESET_T / RRI_EVENT_RESET_W)
_WORDS = ('unbounded', 'not yet implemented', 'sums to 0', 'negative entries')

Oracle = collections.namedtuple('Oracle', 'states log sums error')


def as_stored(X, store):
    return np.ascontiguousarray(np.asarray(X).astype(STORES[store]))


def oracle_run(Xs, W0, T0, marks, flags):
    """The reference's topic loop (oracle/rri_oracle.py:448-483, its own functions) for max(marks) sweeps on the float64 Xs.
    states[m] = (W, T, resets used) after m sweeps for every m of marks; log = [(kind, topic, step)] of the resets, step =
    sweep * k + topic; sums = [(kind, topic, step, the sum the reset rule judged)]; error = (exception type, the distinguishing
    word of its message) of a run that raised -- states then holds the marks reached before.

    orc.nmf itself is not called: it returns the reference's sentinel for a negative regulariser without a bound before the loop
    runs (nmf.py:292-315), and RRIEngine.set_params has no such gate -- the verdicts behind it are exactly what is wanted."""
    from oracle import rri_oracle as orc
    f = dict(project_T_each_iter=False, t_row_sum=None, w_row_sum=None, reset_topic_method='max_resid_document', n_resets=23,
             fix_reset_seed=False, reg_w_l1=0.0, reg_w_l2=0.0, reg_t_l1=0.0, reg_t_l2=0.0)
    f.update(flags)
    X = np.asarray(Xs, dtype=np.float64)
    W, T = np.array(W0, dtype=np.float64), np.array(T0, dtype=np.float64)
    k = W.shape[1]
    log, sums, states = [], [], {}

    class Recording(orc._Resets):
        kind, step = 0, 0

        def _reseed(self, X_, W_, T_, t):
            log.append((self.kind, t, self.step))
            orc._Resets._reseed(self, X_, W_, T_, t)

    resets = Recording(f['n_resets'], f['reset_topic_method'], f['fix_reset_seed'])
    no_regs = abs(f['reg_w_l1']) + abs(f['reg_w_l2']) + abs(f['reg_t_l1']) + abs(f['reg_t_l2']) == 0
    error = None
    if 0 in marks:
        states[0] = (W.copy(), T.copy(), 0)
    try:
        for s in range(max(marks)):
            for t in range(k):
                resets.step = s * k + t
                wR, nw = orc.residual_products_T(X, W, T, t)
                T[t, :], nt1 = orc.qf_min(-(wR - f['reg_t_l1']), nw + f['reg_t_l2'],
                                          s=f['t_row_sum'] if f['project_T_each_iter'] else None, ub=f['t_row_sum'])
                if no_regs:
                    W[:, t] = W[:, t] * nt1
                resets.kind = EVENT_T
                sums.append((EVENT_T, t, resets.step, float(np.sum(T[t, :]))))
                resets.after_T(X, W, T, t, f['project_T_each_iter'], f['t_row_sum'])
                Rt, nt = orc.residual_products_W(X, W, T, t)
                W[:, t], _ = orc.qf_min(-(Rt - f['reg_w_l1']), nt + f['reg_w_l2'], s=None, ub=f['w_row_sum'])
                resets.kind = EVENT_W
                sums.append((EVENT_W, t, resets.step, float(np.sum(W[:, t]))))
                resets.after_W(X, W, T, t)
                assert np.all(W[:, t] >= 0), 'W contains negative entries'
                assert np.sum(W[:, t]) > 0, 'W[:, t] sums to 0'
            if s + 1 in marks:
                states[s + 1] = (W.copy(), T.copy(), resets.count)
    except (ValueError, NotImplementedError, AssertionError) as ex:
        word = [w for w in _WORDS if w in str(ex)]
        error = (type(ex), word[0] if word else str(ex))
    return Oracle(states, log, sums, error)


def one_ulp_up(a):
    return np.nextafter(np.asarray(a, dtype=np.float64), np.inf)


def relfro(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / (den if den > 0 else 1.0))


def control(Xs, W0, T0, marks, flags, ref):
    """{m: the oracle against itself with every entry of the start moved up one ulp, after m sweeps}: what two correct
    implementations of a chain of k dependent steps can differ by (None where that run took another turn: raised, or reset
    another number of topics)"""
    ctl = oracle_run(Xs, one_ulp_up(W0), one_ulp_up(T0), marks, flags)
    out = {}
    for m in marks:
        if m in ctl.states and m in ref.states and ctl.states[m][2] == ref.states[m][2]:
            out[m] = max(relfro(ctl.states[m][0], ref.states[m][0]), relfro(ctl.states[m][1], ref.states[m][1]))
        else:
            out[m] = None
    return out


def bound(k, ctl):
    """k <= 22: the 2e-9 test_against_the_cpu_oracle holds this kernel to after five sweeps.  Beyond: the longer chain of a sweep
    amplifies a rounding difference topic by topic, so the bound is measured on the oracle alone -- 20 x the one-ulp control, the
    factor tests/test_group_gpu.py uses for the same construction -- and never below 2e-9"""
    if k <= SMALL_K or ctl is None:
        return 2e-9
    return max(2e-9, 20.0 * ctl)


def objective_of(Xs, W, T, flags):
    """1/2 ||Xs - W T||^2 plus the penalties (nmf.py:71-94), float64 on the host"""
    R = Xs - W.dot(T)
    return (0.5 * float(np.sum(R * R)) + 0.5 * flags.get('reg_w_l2', 0.0) * float(np.sum(W * W))
            + 0.5 * flags.get('reg_t_l2', 0.0) * float(np.sum(T * T)) + flags.get('reg_t_l1', 0.0) * float(np.sum(np.abs(T)))
            + flags.get('reg_w_l1', 0.0) * float(np.sum(np.abs(W))))


def problem(n, d, k, store, flags, seed):
    """(X in its storage type, Xs = the same values in float64, W0, T0): planted_X's recipe, rounded once to the storage type.
    With the projection the rows of X, W0 and T0 lie on the simplex, the scale the estimator starts from (from an unscaled start
    the unprojected rows of the first sweep sum to hundreds and the projection subtracts a hundred times what it keeps:
    tests/test_onchip_gpu.py::test_topic_model_flags).  Beyond k = 22 the start is the ORACLE's state two sweeps on: the first
    sweeps of a long Gauss-Seidel chain from a random start amplify every rounding (test_onchip_equals_launch_per_phase takes
    the same two sweeps, but on the device)."""
    from rri_nmf_amd.synthetic import planted_X, scaled_init
    X = planted_X(n, d, max(2, min(k, d)), seed=seed, dtype=np.float64)
    if projected(flags):
        X = X / X.sum(1, keepdims=True)
    X = as_stored(X, store)
    Xs = X.astype(np.float64)
    W0, T0 = scaled_init(Xs, k, seed=seed + 1)
    if projected(flags):
        W0, T0 = W0 / W0.sum(1, keepdims=True), T0 / T0.sum(1, keepdims=True)
    if k > SMALL_K:
        warm = oracle_run(Xs, W0, T0, (2,), flags)
        assert warm.error is None, warm.error
        W0, T0 = warm.states[2][0], warm.states[2][1]
    return X, Xs, W0, T0


def edge_problem(case):
    return problem(case.n, case.d, case.k, case.store, case.flags, seed=1000 + case.n % 977 + case.d + 7 * case.k)


# ---- verdicts ----------------------------------------------------------------------------------------------------------------
# name, k, store, flags, sweeps, what: 'scaled' = the problem scaled by s (X by s^2, the starts by s), 'dead' = a planted dead
# column of W0, expect: dict of error=(type, word) | resets=<count> | spent=<True: the budget ran out before the end>
Verdict = collections.namedtuple('Verdict', 'name k store flags sweeps scale dead expect')
VN, VD = 300, 70


def verdict_cases():
    out = []

    def add(name, k, store, flags, sweeps=2, scale=None, dead=None, **expect):
        out.append(Verdict('%s-k%d-%s-%s' % (name, k, store, 'tm' if projected(flags) else 'plain'), k, store, dict(flags), sweeps,
                           scale, dead, expect))

    A, V, N = AssertionError, ValueError, NotImplementedError
    for k, store in ((5, 'fp32'), (30, 'fp64'), (5, 'fp64'), (30, 'fp32')):
        main = (k, store) in ((5, 'fp32'), (30, 'fp64'))       # every outcome on these two; the other pairing takes a subset
        budget = 23
        # -- W columns emptied (reg_w_l1 = 1e6 empties every column in turn: the first, the middle ones inside the step loop,
        #    the last after it).  t_row_sum bounds the T side as in test_reset_events_through_nmf.
        wl1 = dict(t_row_sum=1.0, reg_w_l1=1e6)
        if k == 5:
            add('wcol-resets-maxresid', k, store, wl1, sweeps=2, resets=2 * k, topics=list(range(k)) * 2)
            if main:
                add('wcol-resets-random', k, store, dict(wl1, reset_topic_method='random', fix_reset_seed=True), sweeps=2,
                    resets=2 * k, topics=list(range(k)) * 2)
            add('wcol-budget-ends-at-last-topic', k, store, dict(wl1, n_resets=k - 1), sweeps=1, error=(A, 'sums to 0'),
                topics=list(range(k - 1)))
        else:
            # 30 columns die per sweep: the budget of 23 runs out inside the first launch, and topic 23 raises the assertion
            add('wcol-budget-runs-out', k, store, wl1, sweeps=1, error=(A, 'sums to 0'), topics=list(range(budget)))
        add('wcol-no-method', k, store, dict(wl1, reset_topic_method=None), sweeps=1, error=(A, 'sums to 0'), topics=[])
        if main:
            add('wcol-two-die-one-reset', k, store, dict(wl1, n_resets=1), sweeps=1, error=(A, 'sums to 0'), topics=[0])
        # -- T rows driven to zero
        tl1 = dict(t_row_sum=1.0, reg_t_l1=1e6)
        if k == 5:
            add('trow-resets', k, store, tl1, sweeps=2, resets=2 * k, topics=list(range(k)) * 2)
        if main:
            # once the budget is spent the row stays zero; its W column then has a zero denominator and no bound: "unbounded"
            add('trow-budget-2', k, store, dict(tl1, n_resets=2), sweeps=1, error=(V, 'unbounded'), topics=[0, 1])
            add('trow-no-method', k, store, dict(tl1, reset_topic_method=None), sweeps=1, error=(V, 'unbounded'), topics=[])
            # ... and with a bound on W the zero row gives a zero column: the assertion
            add('trow-budget-2-wbound', k, store, dict(tl1, n_resets=2, w_row_sum=1.0), sweeps=1, error=(A, 'sums to 0'),
                topics=[0, 1])
        # -- sums in (0, 1e-10]: X scaled by s^2, the starts by s
        if k == 5:
            add('tiny-sums', k, store, {}, sweeps=2, scale=1e-10, resets=4 * k, tiny=True)
            add('tiny-sums-no-method', k, store, dict(reset_topic_method=None), sweeps=2, scale=1e-10, resets=0, tiny=True)
            # the neighbour on the other side of the threshold: every W column sums to a value in (1e-10, 1e-9], nothing resets
            add('sums-just-above', k, store, {}, sweeps=1, scale=SCALE_ABOVE, resets=0, above=True)
        # -- scalar denominator <= 0 (optimization.py:60-73)
        add('tden-bounds', k, store, dict(t_row_sum=2.0, reg_t_l2=-1e9), sweeps=2, resets=None)
        add('tden-one-hot', k, store, dict(TM, reg_t_l2=-1e9), sweeps=2, resets=None)
        add('tden-not-implemented', k, store, dict(project_T_each_iter=True, t_row_sum=2.0, w_row_sum=1.0, reg_t_l2=-1e9), sweeps=1,
            error=(N, 'not yet implemented'))
        for dead in ((0, k // 2, k - 1) if main else (k // 2,)):
            add('tden-unbounded-dead%d' % dead, k, store, {}, sweeps=1, dead=dead, error=(V, 'unbounded'))
        add('wden-bounds', k, store, dict(w_row_sum=0.7, reg_w_l2=-1e9), sweeps=2, resets=None)
        add('wden-unbounded', k, store, dict(reg_w_l2=-1e9), sweeps=1, error=(V, 'unbounded'))
    return out


SCALE_ABOVE = 2.8e-9


def verdict_problem(v):
    from rri_nmf_amd.synthetic import planted_X, scaled_init
    X = planted_X(VN, VD, 5, seed=77, dtype=np.float64)
    if projected(v.flags):
        X = X / X.sum(1, keepdims=True)
    W0, T0 = scaled_init(X, v.k, seed=78)
    if projected(v.flags):
        W0, T0 = W0 / W0.sum(1, keepdims=True), T0 / T0.sum(1, keepdims=True)
    if v.scale is not None:
        X, W0, T0 = X * v.scale ** 2, W0 * v.scale, T0 * v.scale
    if v.dead is not None:
        W0 = W0.copy()
        W0[:, v.dead] = 0.0
    X = as_stored(X, v.store)
    return X, X.astype(np.float64), W0, T0
