"""Frozen rows on the device: a handle on X_H with the statistics of (X_O, W_O) against the float64 restatement of the stacked
problem (frozen_cases.Stacked), empty and cleared statistics bit for bit, rri_frozen_absorb against W^T X etc. elementwise, the
objective's share, one forced reset, and partial_fit end to end."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import frozen_cases as fc
import onchip_cases as oc
from conftest import GOLDEN
from rri_nmf_amd.engine import FrozenRows, RRIEngine, device_memory

pytestmark = pytest.mark.gpu

U = 2.0 ** -53      # unit roundoff of float64
STORES = {'f32': np.float32, 'f64': np.float64, 'csr': np.float64}


def make_engine(Xh, k, storage, flags, W=None, T=None, n_resets=23):
    n, d = Xh.shape
    if storage == 'csr':
        eng = RRIEngine(n, d, k, dtype=np.float64, sparse_x=True)
        eng.upload_X_csr(sp.csr_matrix(Xh))
    else:
        eng = RRIEngine(n, d, k, dtype=STORES[storage])
        eng.upload_X(Xh.astype(STORES[storage]))
    if W is not None:
        eng.set_W(W)
    if T is not None:
        eng.set_T(T)
    eng.set_params(reset_topic_method='max_resid_document', n_resets=n_resets, **flags)
    return eng


def stored(X, storage):
    """X as the handle holds it, in float64 (a float32 store rounds once, at upload)"""
    return X.astype(STORES[storage]).astype(np.float64)


def takes_fused_trow(n, d, k):
    """rri_layout.hpp, trow_small: (Gram partial rows) (k + 2) (32-column blocks) <= 4e6; a column update leaves one partial row
    per 64 rows"""
    return -(-n // 64) * (k + 2) * -(-d // 32) <= 4.0e6


# ---- stacked equivalence --------------------------------------------------------------------------------------------------
# (flavour, storage, k, d, n_h): every k of {1, 2, 5, 17, 64, 65}, d of {1, 37, 300}, n_h of {1, 63, 257}, storage and flavour
EQUIV = [('plain', 'f32', 5, 300, 257), ('tm', 'f64', 17, 37, 63), ('pen', 'f32', 2, 37, 257), ('plain', 'f64', 1, 37, 63),
         ('plain', 'f32', 64, 300, 257), ('tm', 'f32', 65, 300, 63), ('plain', 'csr', 5, 37, 63), ('tm', 'csr', 17, 300, 257),
         ('pen', 'csr', 2, 37, 1), ('plain', 'f64', 5, 1, 63), ('tm', 'f32', 5, 37, 1), ('pen', 'f64', 65, 300, 257),
         ('tm', 'f64', 64, 300, 257)]
N_O = 41


@pytest.mark.parametrize('flavour,storage,k,d,n_h', EQUIV, ids=['-'.join(map(str, c)) for c in EQUIV])
def test_a_handle_with_statistics_runs_the_stacked_problem(flavour, storage, k, d, n_h):
    """W and T after 1 and after 3 sweeps against the restatement of the stacked problem, relative Frobenius error <= 1e-10 (the
    bound tests/test_sharded_gpu.py holds the same kind of reordering to on unweighted handles); the restatement meets no reset"""
    Xo, Wo, Xh, Wh, T, flags = fc.make_case(N_O, n_h, d, k, seed=k + d + n_h, flavour=flavour, integer=storage != 'f64')
    Xo, Xh = stored(Xo, storage), stored(Xh, storage)
    assert takes_fused_trow(n_h, d, k)        # without statistics this shape is on the k_trow_small route (or on chip)
    eng = make_engine(Xh, k, storage, flags, Wh, T)
    try:
        if (flavour, storage, k, d, n_h) == EQUIV[0]:
            # on-chip eligible without statistics, not with them, and again after a clear
            assert oc.geometry(n_h, d, k, 'fp32', False, eng.layout_info()['n_cu'])['eligible']
            assert eng.onchip_info()[0] == 1
            eng.set_frozen(FrozenRows(*fc.stats_of(Xo, Wo), rows=N_O))
            assert eng.onchip_info()[0] == 0
            eng.clear_frozen()
            assert eng.onchip_info()[0] == 1
        launches0 = eng.onchip_info()[1]
        eng.set_frozen(FrozenRows(*fc.stats_of(Xo, Wo), rows=N_O))
        st = fc.Stacked(Xo, Wo, Xh, Wh, T, reset_topic_method='max_resid_document', n_resets=23, **flags)
        done = 0
        for upto in (1, 3):
            eng.sweep(upto - done)
            Wr, Tr = st.sweep(upto - done)
            done = upto
            assert st.resets == 0 and eng.n_resets_used == 0
            ew, et = fc.relfro(eng.get_W(), Wr), fc.relfro(eng.get_T(), Tr)
            print('%d sweep(s): W %.2e T %.2e' % (upto, ew, et))
            assert ew <= 1e-10 and et <= 1e-10, (upto, ew, et)
        assert eng.onchip_info()[1] == launches0            # no persistent launch while statistics are set
        got = eng.get_frozen()                              # the statistics are inputs: a sweep leaves them as they were
        B, A, s, c = fc.stats_of(Xo, Wo)
        assert np.array_equal(got.B, B) and np.array_equal(got.A, A) and np.array_equal(got.s, s) and got.c == c and got.rows == N_O
    finally:
        eng.close()


# ---- empty and cleared statistics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flavour,storage', [('plain', 'f32'), ('tm', 'f64'), ('pen', 'csr')])
def test_empty_statistics_change_no_bit_and_a_cleared_handle_is_one_that_never_had_any(flavour, storage, monkeypatch):
    k, d, n = 6, 45, 130
    _, _, Xh, Wh, T, flags = fc.make_case(0, n, d, k, seed=3, flavour=flavour, integer=storage != 'f64')
    Xh = stored(Xh, storage)

    def run(prepare, env):
        for key in ('RRI_TROW_SMALL', 'RRI_ONCHIP'):
            monkeypatch.delenv(key, raising=False)
        for key, val in env.items():
            monkeypatch.setenv(key, val)                   # read when the handle is created
        eng = make_engine(Xh, k, storage, flags, Wh, T)
        try:
            prepare(eng)
            eng.sweep(2)
            return eng.get_W(), eng.get_T(), eng.objective()
        finally:
            eng.close()

    # all zeros: the sweep of a handle that is forced onto the same route (k_reduce and k_trow_numer apart, no persistent launch)
    zeros = run(lambda e: e.set_frozen(FrozenRows.zeros(k, d)), {})
    routed = run(lambda e: None, {'RRI_TROW_SMALL': '0', 'RRI_ONCHIP': '0'})
    assert np.array_equal(zeros[0], routed[0]) and np.array_equal(zeros[1], routed[1])
    assert abs(zeros[2] - routed[2]) <= 1e-12 * abs(routed[2])

    def set_and_clear(e):
        e.set_frozen(FrozenRows(np.ones((k, d)), np.eye(k), np.ones(k), 5.0))
        e.clear_frozen()
    cleared = run(set_and_clear, {})
    never = run(lambda e: None, {})
    assert np.array_equal(cleared[0], never[0]) and np.array_equal(cleared[1], never[1]) and cleared[2] == never[2]


# ---- absorb -----------------------------------------------------------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


@pytest.mark.parametrize('storage', ['f32', 'f64', 'csr'])
@pytest.mark.parametrize('k', [1, 16, 17, 50, 128, 129])
def test_absorb_takes_the_sums_of_the_handles_rows(k, storage):
    """B, A, s, c against W^T X, W^T W, 1^T W, ||X||^2 (taken in extended precision) elementwise, within u (n + 2) |W|^T |X| (and
    the like): n and d are no multiple of any tile (32-row steps, 16-column tiles, 64 / 128 / 256-column blocks)"""
    n, d = 333, 203
    rs = np.random.RandomState(k)
    X = fc.planted(n, d, 6, seed=k)
    if storage != 'f64':
        X = np.floor(5.0 * X / X.max() + 0.7 * rs.rand(n, d))
    X = stored(X, storage)
    W = rs.rand(n, k) * (rs.rand(n, k) < 0.8)
    T = rs.rand(k, d)
    before = device_memory()
    eng = make_engine(X, k, storage, {}, W, T)
    try:
        with_handle = device_memory()
        eng.absorb(1.0)
        assert device_memory()[0] == with_handle[0] + 4 and device_memory()[1] > with_handle[1]
        f1 = eng.get_frozen()
        Xl, Wl = _ld(X), _ld(W)
        refB, refA, refs, refc = Wl.T.dot(Xl), Wl.T.dot(Wl), Wl.sum(0), (Xl ** 2).sum()
        bB, bA, bs, bc = U * (n + 2) * np.abs(W).T.dot(np.abs(X)), U * (n + 2) * W.T.dot(W), U * (n + 2) * W.sum(0), U * (n * d + 2) * float(refc)
        print('k=%d %s: B %.2e of the bound, A %.2e, s %.2e, c %.2e' % (
            k, storage, float((np.abs(f1.B - refB) / np.maximum(bB, 1e-300)).max()), float((np.abs(f1.A - refA) / np.maximum(bA, 1e-300)).max()),
            float((np.abs(f1.s - refs) / np.maximum(bs, 1e-300)).max()), abs(f1.c - float(refc)) / bc))
        assert (np.abs(f1.B - refB) <= bB).all() and (np.abs(f1.A - refA) <= bA).all() and (np.abs(f1.s - refs) <= bs).all()
        assert abs(f1.c - float(refc)) <= bc and f1.rows == n
        assert np.array_equal(f1.A, f1.A.T)
        # absorb-then-get round trip through set, and twice the same bits
        eng.set_frozen(f1)
        back = eng.get_frozen()
        assert np.array_equal(back.B, f1.B) and np.array_equal(back.A, f1.A) and np.array_equal(back.s, f1.s) and back.c == f1.c
        assert back.rows == n
        eng.clear_frozen()
        assert device_memory() == with_handle
        eng.absorb(1.0)
        f2 = eng.get_frozen()
        assert np.array_equal(f2.B, f1.B) and np.array_equal(f2.A, f1.A) and np.array_equal(f2.s, f1.s) and f2.c == f1.c
        # decay 0.5 on top: F <- 0.5 F + the same sums = 1.5 of them, one more rounding per entry
        eng.absorb(0.5)
        f3 = eng.get_frozen()
        assert f3.rows == 2 * n
        g = 1.5 * (n + 2) + 1
        assert (np.abs(f3.B - 1.5 * refB) <= g * U * np.abs(W).T.dot(np.abs(X))).all()
        assert (np.abs(f3.A - 1.5 * refA) <= g * U * W.T.dot(W)).all() and (np.abs(f3.s - 1.5 * refs) <= g * U * W.sum(0)).all()
        assert abs(f3.c - 1.5 * float(refc)) <= 1.5 * bc + U * 1.5 * float(refc)
        with pytest.raises(ValueError, match='outside'):
            eng.absorb(0.0)
        with pytest.raises(ValueError, match='outside'):
            eng.absorb(1.5)
        eng.clear_frozen()
        assert device_memory() == with_handle
    finally:
        eng.close()
    assert device_memory() == before


@pytest.mark.parametrize('storage', ['f32', 'csr'])
def test_an_absorb_leaves_the_factors_and_the_sweep_that_follows_as_they_were(storage):
    k, d, n = 7, 77, 150
    _, _, Xh, Wh, T, flags = fc.make_case(0, n, d, k, seed=11, flavour='tm', integer=True)
    Xh = stored(Xh, storage)
    outs = []
    for absorb in (True, False):
        eng = make_engine(Xh, k, storage, flags, Wh, T)
        try:
            eng.sweep(1)
            W1, T1 = eng.get_W(), eng.get_T()
            if absorb:
                eng.absorb(1.0)
                assert np.array_equal(eng.get_W(), W1) and np.array_equal(eng.get_T(), T1)
                eng.clear_frozen()
            eng.sweep(1)
            outs.append((W1, T1, eng.get_W(), eng.get_T(), eng.objective()))
        finally:
            eng.close()
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert np.array_equal(a, b)
    assert outs[0][4] == outs[1][4]


def test_the_handles_that_do_not_take_statistics_say_so_and_change_nothing():
    k, d, n = 3, 20, 30
    rs = np.random.RandomState(0)
    X, W, T = np.floor(3 * rs.rand(n, d)), rs.rand(n, k), rs.rand(k, d)
    F = FrozenRows.of(X, W)
    made = [RRIEngine(n, d, k, dtype=np.float64, weighted=True), RRIEngine(n, d, k, dtype=np.float64, schedule='residual'),
            RRIEngine(n, d, k, dtype=np.float16), RRIEngine(n, d, k, dtype=np.uint8)]
    try:
        for eng in made:
            with pytest.raises(NotImplementedError):
                eng.set_frozen(F)
            with pytest.raises(NotImplementedError):
                eng.absorb(1.0)
            with pytest.raises(ValueError, match='no frozen statistics'):
                eng.get_frozen()
            eng.clear_frozen()         # harmless on any handle
    finally:
        for eng in made:
            eng.close()
    eng = make_engine(X, k, 'f64', {}, W, T)
    try:
        for bad in (FrozenRows(-F.B, F.A, F.s, F.c), FrozenRows(F.B, F.A + np.triu(np.ones((k, k)), 1), F.s, F.c),
                    FrozenRows(F.B, F.A, F.s * np.nan, F.c), FrozenRows(F.B, F.A, F.s, -1.0), FrozenRows.zeros(k + 1, d)):
            with pytest.raises(ValueError):
                eng.set_frozen(bad)
            with pytest.raises(ValueError, match='no frozen statistics'):
                eng.get_frozen()
        # W fixed while statistics are set: refused by the stepping calls, and taken again after a clear
        eng.set_frozen(F)
        eng.set_params(fix_W=True, reset_topic_method=None)
        W0, T0 = eng.get_W(), eng.get_T()
        with pytest.raises(NotImplementedError, match='fix_W'):
            eng.sweep(1)
        with pytest.raises(NotImplementedError, match='fix_W'):
            eng.update_T_row(0)
        with pytest.raises(NotImplementedError, match='fix_W'):
            eng.topic_reduce_local(0)
        assert np.array_equal(eng.get_W(), W0) and np.array_equal(eng.get_T(), T0)
        # T fixed: the sweeps ignore the statistics
        eng.set_params(fix_T=True, reset_topic_method=None)
        eng.sweep(2)
        Wf = eng.get_W()
        eng.clear_frozen()
        eng.set_W(W0)
        eng.sweep(2)
        assert np.array_equal(eng.get_W(), Wf)
    finally:
        eng.close()


# ---- the objective ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('storage', ['f32', 'f64', 'csr'])
def test_the_objective_is_that_of_the_stacked_problem(storage):
    """before a sweep (through the residual) and after one (from the sweep's cross terms), against 1/2 ||X - W T||^2 of the
    stacked restatement, within 1e-12 (1/2 ||X_stacked||^2): the formula cancels against c"""
    k, d, n_h = 5, 61, 120
    Xo, Wo, Xh, Wh, T, flags = fc.make_case(N_O, n_h, d, k, seed=5, flavour='pen', integer=storage != 'f64')
    Xo, Xh = stored(Xo, storage), stored(Xh, storage)
    scale = 0.5 * float((Xo ** 2).sum() + (Xh ** 2).sum())
    eng = make_engine(Xh, k, storage, flags, Wh, T)
    try:
        eng.set_frozen(FrozenRows(*fc.stats_of(Xo, Wo)))
        st = fc.Stacked(Xo, Wo, Xh, Wh, T, reset_topic_method='max_resid_document', n_resets=23, **flags)
        for step in range(2):
            Wd, Td = eng.get_W(), eng.get_T()
            X, W = np.vstack([Xo, Xh]), np.vstack([Wo, Wd])
            data = 0.5 * float(((X - W.dot(Td)) ** 2).sum())      # the device's own factors: only the objective is under test
            want = data + 0.5 * flags['reg_w_l2'] * (Wd ** 2).sum() + 0.5 * flags['reg_t_l2'] * (Td ** 2).sum() + \
                flags['reg_t_l1'] * np.abs(Td).sum() + flags['reg_w_l1'] * np.abs(Wd).sum()
            got, parts = eng.objective(), eng.objective_parts()
            print('%s step %d: objective off by %.2e of the scale, data term by %.2e' % (storage, step, abs(got - want) / scale, abs(parts[0] - data) / scale))
            assert abs(got - want) <= 1e-12 * scale and abs(parts[0] - data) <= 1e-12 * scale
            eng.sweep(1)
            st.sweep(1)
        assert st.resets == 0 and abs(eng.objective_parts()[0] - st.objective()) <= 1e-9 * scale
    finally:
        eng.close()


# ---- one forced reset ---------------------------------------------------------------------------------------------------------
def test_a_reset_clears_the_topics_statistics_and_the_run_matches_the_restatement():
    """Plain flavour.  Column t of W_in at 1e-30 (an exact zero makes the denominator of the T-row step zero, which is the
    reference's "unbounded" error, not a reset) and topic t's statistics zero: the T row of topic t comes out below 1e-10 in
    sum, the topic is reset among the handle's rows, its statistics stay cleared, and W, T match the restatement"""
    k, d, n_h, t = 4, 37, 63, 2
    Xo, Wo, Xh, Wh, T, flags = fc.make_case(N_O, n_h, d, k, seed=9, flavour='plain')
    Wo[:, t] = 0.0
    Wh[:, t] = 1e-30
    B, A, s, c = fc.stats_of(Xo, Wo)
    assert not B[t].any() and not A[t].any() and not A[:, t].any() and s[t] == 0.0
    eng = make_engine(Xh, k, 'f64', flags, Wh, T)
    try:
        eng.set_frozen(FrozenRows(B, A, s, c))
        st = fc.Stacked(Xo, Wo, Xh, Wh, T, reset_topic_method='max_resid_document', n_resets=23, **flags)
        eng.sweep(2)
        Wr, Tr = st.sweep(2)
        assert st.resets == 1 and eng.n_resets_used == 1 and eng.reset_log[0][1] == t
        ew, et = fc.relfro(eng.get_W(), Wr), fc.relfro(eng.get_T(), Tr)
        print('after the reset: W %.2e T %.2e' % (ew, et))
        assert ew <= 1e-10 and et <= 1e-10
        got = eng.get_frozen()
        assert not got.B[t].any() and not got.A[t].any() and not got.A[:, t].any() and got.s[t] == 0.0
        keep = [l for l in range(k) if l != t]
        assert np.array_equal(got.B[keep], B[keep]) and np.array_equal(got.A[np.ix_(keep, keep)], A[np.ix_(keep, keep)])
    finally:
        eng.close()


def test_a_reset_zeroes_statistics_that_were_not_zero():
    """the same through rri_apply_reset_vectors: row t of B, row and column t of A and s[t] go, the rest stays"""
    k, d, n = 4, 21, 30
    rs = np.random.RandomState(1)
    X, W, T = rs.rand(n, d), rs.rand(n, k), rs.rand(k, d)
    F = FrozenRows.of(rs.rand(9, d), rs.rand(9, k))
    eng = make_engine(X, k, 'f64', {}, W, T)
    try:
        eng.set_frozen(F)
        eng.apply_reset_vectors(1, rs.rand(d), rs.rand(n))
        got = eng.get_frozen()
        want = fc.stats_of(np.zeros((1, d)), np.zeros((1, k)))
        assert want[3] == 0.0
        B, A, s = F.B.copy(), F.A.copy(), F.s.copy()
        B[1] = 0; A[1] = 0; A[:, 1] = 0; s[1] = 0
        assert np.array_equal(got.B, B) and np.array_equal(got.A, A) and np.array_equal(got.s, s) and got.c == F.c
    finally:
        eng.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def text_counts():
    X = sp.load_npz(os.path.join(GOLDEN, 'ref_data', 'text_data_train.npz')).toarray().astype(np.float64)
    assert X.shape == (100, 200)
    rs = np.random.RandomState(4)
    W0 = rs.rand(100, 5)
    T0 = rs.rand(5, 200)
    return X, W0 / W0.sum(1, keepdims=True), T0 / T0.sum(1, keepdims=True)


def test_one_partial_fit_on_all_rows_is_fit_with_as_many_sweeps(text_counts):
    from rri_nmf_amd import sklearn_interface as si
    X, W0, T0 = text_counts
    a = si.NMF_TM_Estimator(100, 200, 5, max_iter=3, W=W0.copy(), T=T0.copy()).fit(X)
    b = si.NMF_TM_Estimator(100, 200, 5, W=W0.copy(), T=T0.copy()).partial_fit(X, sweeps=3)
    assert np.array_equal(a.W, b.W) and np.array_equal(a.T, b.T)
    assert b.frozen_.rows == 100 and b.frozen_.c == float((X ** 2).sum())


def test_two_batches_are_the_restatement_driven_the_same_way(text_counts):
    from oracle import rri_oracle as orc
    from rri_nmf_amd import sklearn_interface as si
    X, W0, T0 = text_counts
    X1, X2 = X[:50], X[50:]
    E = si.NMF_TM_Estimator(50, 200, 5, W=W0[:50].copy(), T=T0.copy())
    E.partial_fit(X1, sweeps=3)
    tm = fc.FLAVOURS['tm']
    none = np.zeros((0, 200)), np.zeros((0, 5))
    s1 = fc.Stacked(none[0], none[1], X1, W0[:50], T0, reset_topic_method='max_resid_document', n_resets=23, **tm)
    W1, T1 = s1.sweep(3)                                       # the W that is absorbed: before the final projection
    assert s1.resets == 0
    assert fc.relfro(E.T, T1) <= 1e-10 and fc.relfro(E.W, orc.proj_rows_simplex(W1.copy(), 1.0)) <= 1e-10
    E.partial_fit(X2, sweeps=3)
    fold = orc.nmf(X2, 5, T_in=T1.copy(), fix_T=True, max_iter=4, max_time=7200, project_W_each_iter=False, w_row_sum=1.0,
                   t_row_sum=1.0, do_final_project_W=True, random_state=0)['W']
    s2 = fc.Stacked(X1, W1, X2, fold, T1, reset_topic_method='max_resid_document', n_resets=23, **tm)
    W2, T2 = s2.sweep(3)
    assert s2.resets == 0
    ew, et = fc.relfro(E.W, orc.proj_rows_simplex(W2.copy(), 1.0)), fc.relfro(E.T, T2)
    print('two batches: W %.2e T %.2e' % (ew, et))
    assert ew <= 1e-10 and et <= 1e-10
    want = FrozenRows.of(X1, W1) + FrozenRows.of(X2, W2)
    assert E.frozen_.rows == 100
    assert fc.relfro(E.frozen_.B, want.B) <= 1e-10 and fc.relfro(E.frozen_.A, want.A) <= 1e-10 and fc.relfro(E.frozen_.s, want.s) <= 1e-10
    assert abs(E.frozen_.c - want.c) <= 1e-12 * want.c
