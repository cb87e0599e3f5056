"""Single device operations against float64 numpy at the sizes where the host code picks another kernel.

The buckets come from the dispatch in rri_hip.hip:
  * LK::resid -- k <= 64: k_resid_mfma with KS = 4 / 8 / 12 / 13 / 16 k-steps (k <= 16 / 32 / 48 / 52 / 64), and the column
    ranges of a rebuild without row sums; 64 < k <= 256: k_resid with the whole 64-row W tile in LDS ('Wtile');
    k > 256: k_resid with a 32-topic W slice reloaded per column tile ('Wslice').  Reached through rri_objective and
    rri_objective_parts right after set_W / set_T, rri_resid_row_argmax, and rri_residual_rebuild.
  * xtt_any -- k_xtt_mfma<NT> with NT = 1..4 for m <= 16 / 32 / 48 / 64 rows of the operand, larger m in chunks of 64
    (rri_X_times);  colsums8 -- groups of 8 vectors with a partial last group (rri_Xt_times).
  * topic steps at k > 64 (always the launch-per-phase schedule) against the closed form of one step;
  * wsweep_ok -- the whole-sweep W half with T fixed is taken while wsweep_lds_bytes(k) <= 150 KiB.

Every shape has a ragged last row block (n not a multiple of 64) and a ragged last column tile (d odd); one has d < 64.
Element-wise checks name the 64-row block / 64-column tile that failed; a wrong ragged edge of a few hundred rows would
move a whole-matrix relative norm by only a few per cent.
"""
import numpy as np
import pytest

from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
STORES = {'fp32': np.float32, 'fp64': np.float64}
SHAPES = {'n203xd141': (203, 141), 'n130xd37': (130, 37)}    # 4 and 3 row blocks; 3 column tiles and one (d < 64)
RANKS = [1, 2, 4, 15, 16, 17, 32, 33, 48, 49, 52, 53, 64, 65, 79, 80, 128, 256, 257, 1024]


def resid_bucket(k):
    if k <= 64:
        return 'k=%d-KS%d' % (k, 4 if k <= 16 else 8 if k <= 32 else 12 if k <= 48 else 13 if k <= 52 else 16)
    return 'k=%d-%s' % (k, 'Wtile' if k <= 256 else 'Wslice')


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def oracle():
    from oracle import rri_oracle
    return rri_oracle


def stored(X, dtype):
    """X as the device holds it (rounded to the storage type), in float64"""
    return np.ascontiguousarray(np.asarray(X).astype(dtype).astype(np.float64))


def problem(n, d, k, seed=0):
    X = planted_X(n, d, min(k, 8) + 1, seed=seed + k, dtype=np.float64)
    W0, T0 = scaled_init(X, k, seed=seed + k + 1)
    return X, W0, T0


def near_solution(n, d, k, seed):
    """X = W* T* (dense, rank k) + noise and a start within 0.1 % of (W*, T*): whole sweeps from here keep every row of T and
    column of W alive at any k -- from a random start, Gauss-Seidel sweeps at k in the hundreds empty columns faster than the
    reset budget refills them"""
    rs = np.random.RandomState(seed)
    Ws, Ts = rs.rand(n, k), rs.rand(k, d)
    X = Ws @ Ts + 0.01 * rs.rand(n, d)
    return X, Ws * (1 + 1e-3 * rs.rand(n, k)), Ts * (1 + 1e-3 * rs.rand(k, d))


def blocks(mask, rows_are='row block', cols_are='column tile'):
    """'row block 3 (rows 192..202) / column tile 2 (columns 128..140)' for every 64 x 64 block holding a True of mask"""
    m = np.atleast_2d(mask)
    out = []
    for rb in range(-(-m.shape[0] // 64)):
        for ct in range(-(-m.shape[1] // 64)):
            if m[64 * rb:64 * rb + 64, 64 * ct:64 * ct + 64].any():
                r1, c1 = min(64 * rb + 63, m.shape[0] - 1), min(64 * ct + 63, m.shape[1] - 1)
                out.append('%s %d (%d..%d) / %s %d (%d..%d)' % (rows_are, rb, 64 * rb, r1, cols_are, ct, 64 * ct, c1))
    return out


def assert_elementwise(got, want, bound, what, rows_are='row block', cols_are='column tile'):
    """|got - want| <= bound element by element; the message lists the 64 x 64 blocks that failed and the worst element"""
    got, want = np.atleast_2d(np.asarray(got, np.float64)), np.atleast_2d(np.asarray(want, np.float64))
    bound = np.broadcast_to(bound, want.shape)
    err = np.abs(got - want)
    bad = ~(err <= bound)
    if bad.any():
        ratio = np.where(bad, err / np.maximum(bound, np.finfo(float).tiny), 0.0)
        i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError('%s: %d of %d elements off in %s; worst [%d, %d]: got %r want %r bound %.3g'
                             % (what, int(bad.sum()), bad.size, '; '.join(blocks(bad, rows_are, cols_are)), i, j,
                                got[i, j], want[i, j], bound[i, j]))


def assert_rel(got, want, tol, what):
    err = abs(got - want) / abs(want)
    assert err <= tol, '%s: relative error %.3g > %.1g (got %r, want %r)' % (what, err, tol, got, want)


def resid_bound(X, W, T):
    """rounding bound of X - W T evaluated in float64 twice (device and numpy), k terms each"""
    k = W.shape[1]
    return 4.0 * (k + 2) * U * (np.abs(W) @ np.abs(T) + np.abs(X))


# ---- 1. the residual kernel family ------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(SHAPES), ids=list(SHAPES))
@pytest.mark.parametrize('store', list(STORES))
@pytest.mark.parametrize('k', RANKS, ids=[resid_bucket(k) for k in RANKS])
def test_objective_right_after_set_factors(k, store, shape):
    """rri_objective / rri_objective_parts with no sweep behind them (the residual route): plain without and with
    penalties, and dense weighted handles with a 0/1 mask (bit-packed Mbits) and with non-binary weights (M itself)"""
    orc = oracle()
    n, d = SHAPES[shape]
    dt = STORES[store]
    X, W0, T0 = problem(n, d, k)
    Xs = stored(X, dt)
    regs = dict(reg_w_l1=0.03, reg_w_l2=0.2, reg_t_l1=0.01, reg_t_l2=0.5)
    with engine(n, d, k, dtype=dt) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
        want = orc.true_objective(Xs, W0, T0)
        assert_rel(e.objective(), want, 1e-12, 'plain objective')
        parts = e.objective_parts()
        assert_rel(parts[0], want, 1e-12, 'objective_parts[0] = 1/2 ||X - W T||^2')
        assert_rel(parts[1], float((W0 ** 2).sum()), 1e-12, 'objective_parts[1] = sum W^2')
        assert_rel(parts[2], float(np.abs(W0).sum()), 1e-12, 'objective_parts[2] = sum |W|')
        e.set_params(**regs)
        assert_rel(e.objective(), orc.true_objective(Xs, W0, T0, **regs), 1e-12, 'objective with penalties')
    rs = np.random.RandomState(k + n)
    masks = {'0/1 mask (Mbits)': (rs.rand(n, d) < 0.4).astype(np.float64),
             # multiples of 1/8: the same weights in either storage type
             'non-binary weights (M)': rs.randint(0, 17, size=(n, d)) / 8.0}
    for name, M in masks.items():
        with engine(n, d, k, dtype=dt, weighted=True) as e:
            e.upload_X(X); e.upload_mask(M); e.set_W(W0); e.set_T(T0); e.set_params()
            want = orc.true_objective(Xs, W0, T0, Wm=M)
            assert_rel(e.objective(), want, 1e-12, 'weighted objective, ' + name)
            parts = e.objective_parts()
            assert_rel(parts[0], want, 1e-12, 'weighted objective_parts[0], ' + name)
            assert_rel(parts[1], float((W0 ** 2).sum()), 1e-12, 'weighted objective_parts[1], ' + name)


@pytest.mark.parametrize('shape', list(SHAPES), ids=list(SHAPES))
@pytest.mark.parametrize('store', list(STORES))
@pytest.mark.parametrize('k', RANKS, ids=[resid_bucket(k) for k in RANKS])
def test_max_resid_row_and_reset_row(k, store, shape):
    """rri_resid_row_argmax: argmax_i sum_j max(X - W T, 0)_ij^2 and its value; rri_reset_row: max(X[i] - W[i] T, 0).
    One row carries a clearly larger residual -- in the last, ragged row block for two ranks in three."""
    n, d = SHAPES[shape]
    dt = STORES[store]
    X, W0, T0 = problem(n, d, k, seed=7)
    star = n - 1 - k % 2 if k % 3 else 64 + k % 60
    X[star] += 2.0 * X.max()
    Xs = stored(X, dt)
    R = Xs - W0 @ T0
    pos = (np.maximum(R, 0.0) ** 2).sum(axis=1)
    assert np.argmax(pos) == star and np.sort(pos)[-2] < 0.5 * pos[star]
    bound = resid_bound(Xs, W0, T0)
    with engine(n, d, k, dtype=dt) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
        val, row = e.resid_row_argmax()
        assert row == star, 'arg-max row %d, want %d (row block %d)' % (row, star, star // 64)
        assert_rel(val, pos[star], 1e-12, 'sum_j max(X - W T, 0)^2 of row %d' % star)
        for i in sorted({star, 0, n - 1, 70}):
            assert_elementwise(e.reset_row(i)[None, :], np.maximum(R[i], 0.0)[None, :], bound[i][None, :],
                               'reset row %d (row block %d)' % (i, i // 64))


@pytest.mark.parametrize('shape', list(SHAPES), ids=list(SHAPES))
@pytest.mark.parametrize('store', list(STORES))
@pytest.mark.parametrize('k', RANKS[1:], ids=[resid_bucket(k) for k in RANKS[1:]])
def test_explicit_residual_rebuild(k, store, shape):
    """rri_residual_rebuild + rri_get_residual against X - W T element by element: k_resid_mfma with WRITE_E and no row sums
    (the column-range grid) for k <= 64, k_resid with WRITE_E above.  fp32: within one fp32 ulp of the float64 value rounded
    to fp32 (plus the float64 bound, which matters only where X - W T cancels); fp64: the float64 bound."""
    n, d = SHAPES[shape]
    dt = STORES[store]
    X, W0, T0 = problem(n, d, k, seed=11)
    Xs = stored(X, dt)
    want = Xs - W0 @ T0
    bound = resid_bound(Xs, W0, T0)
    if dt == np.float32:
        bound = bound + np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)
    with engine(n, d, k, dtype=dt, schedule='residual') as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params()
        e.residual_rebuild()
        got = e.get_residual().astype(np.float64)
        # the objective of this schedule is 1/2 ||R||^2 of the residual it stores while computing it
        obj = e.objective()
        got2 = e.get_residual().astype(np.float64)
    assert_elementwise(got, want, bound, 'R = X - W T after rri_residual_rebuild')
    assert_elementwise(got2, want, bound, 'R = X - W T stored by rri_objective')
    assert_rel(obj, 0.5 * float((want ** 2).sum()), 1e-12, 'objective of the residual schedule (summed before the rounding to the storage type)')


OBJ_DIRECT_RANKS = [2, 16, 17, 49, 53, 64, 65, 256, 257]


@pytest.mark.parametrize('k', OBJ_DIRECT_RANKS, ids=[resid_bucket(k) for k in OBJ_DIRECT_RANKS])
def test_objective_after_a_sweep_with_obj_direct(monkeypatch, k):
    """After a sweep the objective is assembled from the sweep's cross terms; RRI_OBJ_DIRECT=1 takes the residual kernel
    there instead.  Both against 1/2 ||X - W T||^2 of the factors the sweep left, in float64."""
    n, d = SHAPES['n203xd141']
    X, W0, T0 = near_solution(n, d, k, seed=13 + k)
    Xs = stored(X, np.float32)
    vals = {}
    for direct in ('0', '1'):
        monkeypatch.setenv('RRI_OBJ_DIRECT', direct)          # read when a handle is created
        with engine(n, d, k, dtype=np.float32) as e:
            e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(reset_topic_method=None)
            e.sweep(1)
            W, T = e.get_W(), e.get_T()
            vals[direct] = (e.objective(), oracle().true_objective(Xs, W, T))
    obj, want = vals['1']
    assert_rel(obj, want, 1e-12, 'RRI_OBJ_DIRECT=1 objective after a sweep')
    # the assembled value: 1/2 ||X||^2 - sum <w_t, X t_t> + 1/2 <W^T W, T T^T>, terms of the size of ||X||^2
    obj, want = vals['0']
    assert abs(obj - want) <= 1e-12 * 0.5 * float((Xs ** 2).sum()) * k, ('assembled objective after a sweep', obj, want)


# ---- 2. products with the resident X ----------------------------------------------------------------------------------
def xtt_bucket(m):
    return 'm=%d-NT%d' % (m, -(-m // 16)) if m <= 64 else 'm=%d-chunks%d-last%d' % (m, -(-m // 64), m - 64 * (m // 64) or 64)


XT_M = [1, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64, 65, 129]
XTQ_M = [1, 7, 8, 9, 16, 17]


@pytest.mark.parametrize('shape', list(SHAPES), ids=list(SHAPES))
@pytest.mark.parametrize('store', list(STORES))
@pytest.mark.parametrize('m', XT_M, ids=[xtt_bucket(m) for m in XT_M])
def test_X_times(m, store, shape):
    """rri_X_times(B) = X B column by column: k_xtt_mfma<NT> for every NT and the chunk loop (a last chunk of 1 at m = 129)"""
    n, d = SHAPES[shape]
    dt = STORES[store]
    X = planted_X(n, d, 5, seed=m, dtype=np.float64)
    Xs = stored(X, dt)
    B = np.random.RandomState(m).randn(d, m)
    with engine(n, d, 4, dtype=dt) as e:
        e.upload_X(X)
        got = e.X_times(B)
    want = Xs @ B
    for j in range(m):
        err = np.linalg.norm(got[:, j] - want[:, j]) / np.linalg.norm(want[:, j])
        assert err <= 1e-13, 'X B: column %d (chunk %d, row %d of Tm in it) relative error %.3g' % (j, j // 64, j % 64, err)
    assert_elementwise(got, want, 4.0 * (d + 2) * U * (np.abs(Xs) @ np.abs(B)), 'X B', cols_are='column group of 64')


@pytest.mark.parametrize('shape', list(SHAPES), ids=list(SHAPES))
@pytest.mark.parametrize('store', list(STORES))
@pytest.mark.parametrize('m', XTQ_M, ids=['m=%d-groups%d-last%d' % (m, -(-m // 8), m - 8 * (m // 8) or 8) for m in XTQ_M])
def test_Xt_times(m, store, shape):
    """rri_Xt_times(Q) = X^T Q column by column: colsums8 in groups of 8 vectors, the last one partial"""
    n, d = SHAPES[shape]
    dt = STORES[store]
    X = planted_X(n, d, 5, seed=m + 100, dtype=np.float64)
    Xs = stored(X, dt)
    Q = np.random.RandomState(m + 100).randn(n, m)
    with engine(n, d, 4, dtype=dt) as e:
        e.upload_X(X)
        got = e.Xt_times(Q)
    want = Xs.T @ Q
    for j in range(m):
        err = np.linalg.norm(got[:, j] - want[:, j]) / np.linalg.norm(want[:, j])
        assert err <= 1e-13, 'X^T Q: column %d (group %d, vector %d of it) relative error %.3g' % (j, j // 8, j % 8, err)
    assert_elementwise(got, want, 4.0 * (n + 2) * U * (np.abs(Xs).T @ np.abs(Q)), 'X^T Q',
                       rows_are='column tile of X', cols_are='column group of 64')


# ---- 3. topic steps at large rank -------------------------------------------------------------------------------------
FLAGS = {'plain': dict(),
         'topic': dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0)}


def step_T_want(Xs, W, T, t, flags):
    orc = oracle()
    wR, nw = orc.residual_products_T(Xs, W, T, t)
    s = flags.get('t_row_sum') if flags.get('project_T_each_iter') else None
    return orc.qf_min(-wR, nw, s=s, ub=flags.get('t_row_sum'))[0]


def step_W_want(Xs, W, T, t, flags):
    orc = oracle()
    Rt, nt = orc.residual_products_W(Xs, W, T, t)
    return orc.qf_min(-Rt, nt, s=None, ub=flags.get('w_row_sum'))[0]


def check_steps(e, Xs, k, flags, tol=1e-12):
    """update_T_row(t), then update_W_col(t), for t in {0, 63, 64, 255, 256, k - 1}: each against the closed form of the step
    taken from the factors on the device before it (nmf.py:670-676 / 728-734 through qf_min), and everything else bit-equal"""
    n, d = Xs.shape
    for t in sorted({0, 63, 64, 255, 256, k - 1} & set(range(k))):
        W0, T0 = e.get_W(), e.get_T()
        e.update_T_row(t)
        W1, T1 = e.get_W(), e.get_T()
        want = step_T_want(Xs, W0, T0, t, flags)
        assert np.linalg.norm(T1[t] - want) <= tol * np.linalg.norm(want), ('T row', t, np.linalg.norm(T1[t] - want) / np.linalg.norm(want))
        assert_elementwise(T1[t][None, :], want[None, :], 10 * tol * np.abs(want).max(), 'T row %d' % t)
        others = np.arange(k) != t
        assert np.array_equal(T1[others], T0[others]), 'T step %d changed other rows of T: %s' % (t, np.flatnonzero(np.any(T1 != T0, axis=1)))
        assert np.array_equal(W1[:, others], W0[:, others]), 'T step %d changed other columns of W' % t
        e.update_W_col(t)
        W2, T2 = e.get_W(), e.get_T()
        want = step_W_want(Xs, W1, T1, t, flags)
        assert np.linalg.norm(W2[:, t] - want) <= tol * np.linalg.norm(want), ('W column', t, np.linalg.norm(W2[:, t] - want) / np.linalg.norm(want))
        assert_elementwise(W2[:, t][:, None], want[:, None], 10 * tol * np.abs(want).max(), 'W column %d' % t)
        assert np.array_equal(T2, T1), 'W step %d changed T' % t
        assert np.array_equal(W2[:, others], W1[:, others]), 'W step %d changed other columns of W: %s' % (
            t, np.flatnonzero(np.any(W2[:, others] != W1[:, others], axis=0)))
        assert e.n_resets_used == 0


LARGE_K = [65, 128, 256, 257, 1024]


@pytest.mark.parametrize('flags', list(FLAGS))
@pytest.mark.parametrize('store', list(STORES))
@pytest.mark.parametrize('k', LARGE_K, ids=['k=%d%s' % (k, '-above-min-n-d' if k > 141 else '') for k in LARGE_K])
def test_topic_steps_at_large_rank(k, store, flags):
    n, d = SHAPES['n203xd141']
    dt = STORES[store]
    X, W0, T0 = problem(n, d, k, seed=17)
    with engine(n, d, k, dtype=dt) as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(**FLAGS[flags])
        check_steps(e, stored(X, dt), k, FLAGS[flags])


@pytest.mark.parametrize('flags', list(FLAGS))
def test_topic_steps_at_k128_explicit_residual(flags):
    """the explicit-residual handle (R = X - W T kept in HBM, rank-one updates), float64, one topic step at a time"""
    n, d, k = 203, 141, 128
    X, W0, T0 = problem(n, d, k, seed=19)
    with engine(n, d, k, dtype=np.float64, schedule='residual') as e:
        e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(**FLAGS[flags])
        check_steps(e, X, k, FLAGS[flags], tol=1e-11)


@pytest.mark.parametrize('flags', list(FLAGS))
def test_weighted_dense_at_k128(flags):
    """The weighted handle exposes no half steps: the sums of its T-row step (rri_topic_reduce_local: w^T (M .* R_t) and
    (w.^2)^T M) for single topics against the closed form, then one sweep of nmf() against the oracle with the yardstick of
    tests/test_fuzz_gpu.py (the oracle against itself from a start perturbed by one ulp), float64"""
    n, d, k = 203, 141, 128
    X, W0, T0 = near_solution(n, d, k, seed=29)
    M = (np.random.RandomState(5).rand(n, d) < 0.5).astype(np.float64)
    orc = oracle()
    kw = dict(FLAGS[flags], reset_topic_method=None)
    with engine(n, d, k, dtype=np.float64, weighted=True) as e:
        e.upload_X(X); e.upload_mask(M); e.set_W(W0); e.set_T(T0); e.set_params(**kw)
        for t in (0, 63, 64, k - 1):
            wR, nw = e.topic_sums(t)
            want_wR, want_nw = orc.residual_products_T(X, W0.copy(), T0, t, M)
            assert_elementwise(wR[None, :], want_wR[None, :], 1e-12 * np.abs(want_wR).max(), 'weighted wR of topic %d' % t)
            assert_elementwise(nw[None, :], want_nw[None, :], 1e-13 * np.abs(want_nw).max(), 'weighted nw of topic %d' % t)
    # the sweep through nmf(): the start is prepared (rows of T_in onto the simplex, ...) as the oracle prepares it
    from rri_nmf_amd.nmf import nmf
    got = nmf(X, k, W_mat=M, W_in=W0.copy(), T_in=T0.copy(), max_iter=1, eps_stop=-1, dtype=np.float64, **kw)
    W, T = got['W'], got['T']
    ref = orc.nmf(X, k, W_mat=M, W_in=W0.copy(), T_in=T0.copy(), max_iter=1, eps_stop=-1, **kw)
    Wp = W0 * (1.0 + 2.0 ** -52 * np.sign(np.random.RandomState(7).randn(*W0.shape)))
    per = orc.nmf(X, k, W_mat=M, W_in=Wp, T_in=T0.copy(), max_iter=1, eps_stop=-1, **kw)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    tol = max(1e-9, 30.0 * max(rel(per['W'], ref['W']), rel(per['T'], ref['T'])))
    assert rel(W, ref['W']) < tol and rel(T, ref['T']) < tol, (rel(W, ref['W']), rel(T, ref['T']), tol)


def wsweep_lds_bytes(k):
    """rri_kernels.hpp wsweep_lds_bytes: the k x kp Gram matrix and a 64 x k row tile in float64"""
    return (k * ((k + 3) & ~3) + 64 * k) * 8


@pytest.mark.parametrize('k', [109, 110], ids=['k=109-one-launch', 'k=110-launch-per-topic'])
def test_fixed_T_boundary_of_the_whole_sweep_launch(monkeypatch, k):
    """wsweep_ok takes the one-launch W half while wsweep_lds_bytes(k) <= 150 KiB: k = 109 is the last such rank.  Both sides
    against the launch-per-topic schedule (RRI_WSWEEP=0) and the oracle; the timing counter of kernel id 1 (the W half)
    says which route ran: one launch per sweep, or k."""
    boundary = max(kk for kk in range(1, 300) if wsweep_lds_bytes(kk) <= 150 * 1024)
    assert boundary == 109
    n, d = SHAPES['n203xd141']
    X, W0, T0 = near_solution(n, d, k, seed=k)
    monkeypatch.setenv('RRI_ONCHIP', '0')
    sweeps = 3
    out = {}
    for store in STORES.values():
        for sw in ('1', '0'):
            monkeypatch.setenv('RRI_WSWEEP', sw)
            with engine(n, d, k, dtype=store) as e:
                e.upload_X(X); e.set_W(W0); e.set_T(T0); e.set_params(fix_T=True, reset_topic_method=None)
                e.timing_enable(True)
                e.sweep(sweeps)
                launches = e.timing_read(1)[0]
                out[sw] = e.get_W(), e.get_T(), e.n_resets_used
            if sw == '1' and k <= boundary:
                assert launches == sweeps, ('one launch per sweep expected', store, launches)
            else:
                assert launches >= sweeps * k, ('a launch per topic expected', store, sw, launches)
        (Wa, Ta, ra), (Wb, Tb, rb) = out['1'], out['0']
        assert ra == rb and np.array_equal(Ta, Tb)
        err = np.linalg.norm(Wa - Wb) / np.linalg.norm(Wb)
        assert err < 1e-12, (store, err)
        ref = oracle().nmf(stored(X, store), k, W_in=W0.copy(), T_in=T0.copy(), max_iter=sweeps, eps_stop=-1, fix_T=True,
                           reset_topic_method=None)
        err = np.linalg.norm(Wa - ref['W']) / np.linalg.norm(ref['W'])
        assert err < 2e-9 and ref['n_resets_used'] == ra, (store, err, ra, ref['n_resets_used'])
