"""The one-launch fold sweep of a pattern-only handle on the GPU (include/rri_fold.h; k_wfold_rows): against the oracle on the stored
values, against the launch-per-topic schedule on a twin handle, its halts, its bit-equality rules, the cached state around it,
the opt-in, and the public route (nmf(fold_in=True), NMF_RS_Estimator.transform_corpus and the W= arguments).

Bounds.  2e-9 against the oracle is the bound tests/test_sparse_wrri_gpu.py and tests/test_hip_parity.py hold the weighted
flavour to; 1e-10 (float64) and 2e-5 (float32) between the two schedules are those of
test_sparse_pattern_matches_dense_weighted_engine, whose float32 side rounds its stored residual (the fold sweep does not: it
computes in float64 on the stored values, so against the oracle it meets 2e-9 for both storage types)."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import fiterr_cases as fc
import fold_cases as fo
from conftest import GOLDEN
from fold_cases import relfro

pytestmark = pytest.mark.gpu
SWEEPS = 4
RESET = dict(reset_topic_method='random', fix_reset_seed=True)
STORES = [np.float64, np.float32]


def lib():
    from rri_nmf_amd import engine
    return engine


def fold():
    from rri_nmf_amd import fold as f
    return f


def oracle():
    from oracle import rri_oracle
    return rri_oracle


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def case(shape, store_name):
    """the problem of a shape as a handle of that storage type holds it"""
    A, X, M, W0, T0 = fo.problem(*shape)
    As, Xs = fo.stored(A, X, np.dtype(store_name))
    return As, Xs, M, W0, T0


@functools.lru_cache(maxsize=None)
def oracle_run(shape, store_name, flag_items, sweeps=SWEEPS):
    As, Xs, M, W0, T0 = case(shape, store_name)
    return oracle().nmf(Xs, shape[2], W_in=W0.copy(), T_in=T0.copy(), W_mat=M, fix_T=True, max_iter=sweeps, eps_stop=-1,
                        do_final_project_W=False, **dict(flag_items))


def handle(A, k, store, W0, T0, asked, **flags):
    """a pattern-only handle with the factors and parameters set; asked: True, False (never asked) or 'off' (asked, taken back)"""
    n, d = A.shape
    e = lib().RRIEngine(n, d, k, dtype=store, weighted='sparse')
    try:
        B = A.copy()
        B.data = A.data.astype(store)
        e.upload_observed_csr(B)
        e.set_W(W0), e.set_T(T0)
        e.set_params(**flags)
        if asked:
            fold().set_fold_schedule(e)
        if asked == 'off':
            fold().set_fold_schedule(e, False)
    except Exception:
        e.close()
        raise
    return e


def run(shape, store, asked, flags, sweeps=SWEEPS, timing=False):
    As, _, _, W0, T0 = case(shape, np.dtype(store).name)
    with handle(As, shape[2], store, W0, T0, asked, fix_T=True, **flags) as e:
        if timing:
            e.timing_enable()
        e.sweep(sweeps)
        out = dict(W=e.get_W(), T=e.get_T(), resets=e.n_resets_used, log=list(e.reset_log), info=fold().fold_info(e))
        if timing:
            out['timed'] = (e.timing_read(1)[0], e.timing_read(3)[0])
    return out


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(fo.FLAGSETS))
@pytest.mark.parametrize('store', STORES)
@pytest.mark.parametrize('shape', fo.SHAPES)
def test_the_one_launch_sweep_is_the_oracle_and_the_launch_per_topic_schedule(shape, store, name):
    """Four sweeps.  No column halts on these inputs except (200, 150, 64) with no flags, where the oracle takes one reset: the
    reset is drawn with a fixed seed on all three sides, and the resumed sweep is one more launch."""
    flags = dict(fo.FLAGSETS[name], **RESET)
    got = run(shape, store, True, flags, timing=True)
    twin = run(shape, store, False, flags, timing=True)
    ref = oracle_run(shape, np.dtype(store).name, tuple(sorted(flags.items())))
    ew, tol = relfro(got['W'], ref['W']), (1e-10 if store == np.float64 else 2e-5)
    es = relfro(got['W'], twin['W'])
    print('fold %s %s %s: W vs oracle %.3e, vs launch per topic %.3e, resets %d' % (shape, np.dtype(store).name, name, ew, es, got['resets']))
    assert got['resets'] == twin['resets'] == ref['n_resets_used'] == (1 if shape[:3] == (200, 150, 64) and name == 'plain' else 0)
    assert ew < 2e-9 and relfro(got['T'], ref['T']) < 2e-9, ew
    assert es < tol and relfro(got['T'], twin['T']) < tol, es
    info = got['info']
    assert info['asked'] and info['eligible'] and info['stepped'] == 0 and info['rows_per_group'] == 16
    assert info['launches'] == SWEEPS + sum(1 for _, t, _ in got['log'] if t != shape[2] - 1) and info['halts'] == got['resets']
    # one timed scope per launch enqueued (those behind a halt return at once and are timed all the same), and no blocked pass ran
    assert got['timed'][1] == 0 and (got['timed'][0] == info['launches'] if got['resets'] == 0 else got['timed'][0] >= info['launches'])
    assert twin['timed'][1] > 0 and twin['info'] == dict(info, asked=False, eligible=False, launches=0, halts=0)


# ---- 2. halts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,flags,resets', [((200, 150, 64, 0.5), {}, 1), ((413, 187, 5, 0.2), dict(w_row_sum=0.7, reg_w_l2=-1e9), 20)])
def test_a_halt_inside_the_launch_leaves_what_the_launch_per_topic_schedule_leaves(shape, flags, resets):
    flags = dict(flags, **RESET)
    got, twin = run(shape, np.float64, True, flags), run(shape, np.float64, False, flags)
    ref = oracle_run(shape, 'float64', tuple(sorted(flags.items())))
    assert got['resets'] == twin['resets'] == ref['n_resets_used'] == resets and got['log'] == twin['log']
    assert relfro(got['W'], twin['W']) < 1e-10 and relfro(got['T'], twin['T']) < 1e-10
    assert relfro(got['W'], ref['W']) < 2e-9 and relfro(got['T'], ref['T']) < 2e-9
    # a launch per sweep, and one more per sweep resumed in its middle (after a reset at the last topic the next sweep simply begins)
    resumed = sum(1 for _, t, _ in got['log'] if t != shape[2] - 1)
    assert got['info']['halts'] == resets and got['info']['launches'] == SWEEPS + resumed and got['info']['stepped'] == 0
    if resets == 20:      # every step of four sweeps of five topics: the launch was entered at every t0
        assert sorted({t for _, t, _ in got['log']}) == list(range(5))


@pytest.mark.parametrize('asked', [True, False])
def test_the_references_errors_on_both_schedules(asked):
    with pytest.raises(AssertionError, match='sums to 0'):          # the 23 resets run out
        run((130, 90, 16, 0.4), np.float64, asked, dict(w_row_sum=0.7, reg_w_l2=-1e9, **RESET))
    with pytest.raises(ValueError, match='unbounded'):
        run((413, 187, 5, 0.2), np.float64, asked, dict(reg_w_l2=-1e9, reset_topic_method=None))


# ---- 3. row independence and repeatability -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', STORES)
@pytest.mark.parametrize('shape,name', [((413, 187, 5, 0.2), 'regs'), ((131, 90, 17, 0.4), 'plain'), ((64, 2100, 4, 0.08), 'wrs')])
def test_rows_are_folded_alone(shape, name, store):
    As, _, _, W0, T0 = case(shape, np.dtype(store).name)
    k, flags = shape[2], dict(fo.FLAGSETS[name], fix_T=True, reset_topic_method=None)

    def folded(A, W, sweeps=SWEEPS):
        with handle(A, k, store, W, T0, True, **flags) as e:
            e.sweep(sweeps)
            assert fold().fold_info(e)['launches'] == sweeps
            return e.get_W()
    a, b = folded(As, W0), folded(As, W0)
    assert np.array_equal(bits(a), bits(b))
    perm = np.random.RandomState(5).permutation(shape[0])
    assert np.array_equal(bits(folded(As[perm].tocsr(), np.ascontiguousarray(W0[perm]))), bits(a[perm]))
    # one row alone: a row whose entries of W all stay positive (alone, an emptied column would be the whole column and halt)
    one = folded(As, W0, 1)
    alone = [i for i in range(shape[0]) if np.all(one[i] > 1e-6)][:3]
    assert alone, 'no row keeps every topic'
    for i in alone:
        assert np.array_equal(bits(folded(As[i:i + 1].tocsr(), np.ascontiguousarray(W0[i:i + 1]), 1)), bits(one[i:i + 1])), i


# ---- 4. state ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('store', STORES)
def test_the_cached_state_around_a_one_launch_sweep(store):
    """free sweep -> fix_T -> one-launch sweep -> objective -> fix_T off -> free sweep: the stored residual is stale after the launch
    and whoever reads it next rebuilds it"""
    shape = (413, 187, 5, 0.2)
    As, Xs, M, W0, T0 = case(shape, np.dtype(store).name)
    k, free = shape[2], dict(t_row_sum=1.0, reset_topic_method=None)
    out = {}
    for asked in (True, False):
        with handle(As, k, store, W0, T0, asked, **free) as e:
            e.sweep(1)
            e.set_params(fix_T=True, **free)
            e.sweep(1)
            obj = e.objective()
            Wm, Tm = e.get_W(), e.get_T()
            e.set_params(**free)
            e.sweep(1)
            out[asked] = (e.get_W(), e.get_T(), obj, Wm, Tm, e.objective())
            assert fold().fold_info(e)['launches'] == (1 if asked else 0)
    got, twin = out[True], out[False]
    tol = 1e-10 if store == np.float64 else 2e-5
    for a, b in zip(got[:2] + got[3:5], twin[:2] + twin[3:5]):
        assert relfro(a, b) < tol, relfro(a, b)
    assert abs(got[2] - twin[2]) <= tol * abs(twin[2]) and abs(got[5] - twin[5]) <= tol * abs(twin[5])
    host = 0.5 * float(np.sum((M * (Xs - got[3] @ got[4])) ** 2))
    assert abs(got[2] - host) <= 1e-9 * host, (got[2], host)
    orc = oracle()
    kw = dict(W_mat=M, max_iter=1, eps_stop=-1, **free)
    r1 = orc.nmf(Xs, k, W_in=W0.copy(), T_in=T0.copy(), **kw)
    r2 = orc.nmf(Xs, k, W_in=r1['W'].copy(), T_in=r1['T'].copy(), fix_T=True, **kw)
    r3 = orc.nmf(Xs, k, W_in=r2['W'].copy(), T_in=r2['T'].copy(), **kw)
    if store == np.float64:      # (the free sweeps of a float32 handle round their stored residual: the twin above is their measure)
        assert relfro(got[3], r2['W']) < 2e-9 and relfro(got[0], r3['W']) < 2e-9 and relfro(got[1], r3['T']) < 2e-9
    # sweeps call by call are one call of three
    fixed = dict(fix_T=True, **free)
    with handle(As, k, store, W0, T0, True, **fixed) as e:
        for _ in range(3):
            e.sweep(1)
        step = e.get_W()
    with handle(As, k, store, W0, T0, True, **fixed) as e:
        e.sweep(3)
        assert np.array_equal(bits(e.get_W()), bits(step))


# ---- 5. opt-in and limits ------------------------------------------------------------------------------------------------------------
def test_a_handle_that_never_asks_sweeps_as_before_and_the_limits():
    shape = (413, 187, 5, 0.2)
    flags = dict(fo.FLAGSETS['regs'], **RESET)
    never, off = run(shape, np.float32, False, flags), run(shape, np.float32, 'off', flags)
    assert np.array_equal(bits(never['W']), bits(off['W'])) and never['info'] == off['info']
    assert off['info'] == dict(asked=False, eligible=False, launches=0, stepped=0, halts=0, rows_per_group=16)
    # k = 65: asked, not eligible, launch by launch, the same bits
    A, X, M, W0, T0 = fo.problem(90, 70, 65, 0.5)
    res = {}
    for asked in (True, False):
        with handle(A, 65, np.float64, W0, T0, asked, fix_T=True, **RESET) as e:
            e.sweep(2)
            res[asked] = (e.get_W(), fold().fold_info(e), e.n_resets_used)
    assert np.array_equal(bits(res[True][0]), bits(res[False][0])) and res[True][2] == res[False][2]
    assert res[True][1]['asked'] and not res[True][1]['eligible'] and res[True][1]['launches'] == 0
    assert res[True][1]['stepped'] >= 2 and res[False][1]['stepped'] == 0
    # memory: the documented buffers, at the first one-launch sweep only
    As, _, _, W0, T0 = case(shape, 'float64')
    n, k = shape[0], shape[2]
    with handle(As, k, np.float64, W0, T0, True, fix_T=True, reset_topic_method=None) as e:
        before = lib().device_memory()
        e.sweep(1)
        first = lib().device_memory()
        e.sweep(1)
        assert lib().device_memory() == first
    nwg = (n + 15) // 16
    extra = first[1] - before[1] - 8 * 2 * k * nwg
    assert first[0] - before[0] == 2 and extra % (8 * k) == 0 and n <= extra // (8 * k) < n + 512, (before, first)
    # the refusals
    with lib().RRIEngine(20, 10, 3, dtype=np.float64) as e:
        with pytest.raises(ValueError, match='pattern-only handle'):
            fold().set_fold_schedule(e)
        with pytest.raises(ValueError, match='pattern-only handle'):
            fold().fold_info(e)


# ---- 6. the public route -------------------------------------------------------------------------------------------------------------
def load(name):
    A = sp.load_npz(os.path.join(GOLDEN, 'ref_data', name)).tocsr().astype(np.float64)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def check_served(E, new, A, W_new):
    """recommend_corpus and score_corpus with the folded rows against the host's arithmetic"""
    m = A.shape[0]
    users = np.array([m - 1, 0, 0, m // 2])
    items, scores = E.recommend_corpus(users, 10, exclude=new, W=W_new)
    P = W_new @ E.T
    for u, it, sc in zip(users, items, scores):
        p = P[u].copy()
        p[A.indices[A.indptr[u]:A.indptr[u + 1]]] = -np.inf
        want = np.sort(p)[::-1][:10]
        assert len(set(it.tolist())) == 10 and not set(it.tolist()) & set(A.indices[A.indptr[u]:A.indptr[u + 1]].tolist())
        assert np.allclose(p[it], want, rtol=1e-12, atol=0) and np.allclose(sc, np.clip(want, E.min_rating, E.max_rating), rtol=1e-12, atol=0)
    got = E.score_corpus(new, W=W_new)
    ref = fc.reference(W_new, E.T, None, A, E.min_rating, E.max_rating)
    N, tot = A.nnz, ref['totals'][0]
    want = float(np.sqrt(tot / N))
    bound = (ref['sq_bound'].sum() + (m + N + 4) * fc.U * tot) / (2.0 * N * want) + 4 * fc.U * want
    assert abs(got - want) <= bound, (got, want, bound)
    with pytest.raises(ValueError, match='must be a DeviceCorpus of shape'):
        E.recommend_corpus([0], 10, exclude=new, W=W_new[:-1])


def test_transform_corpus_on_the_recommender_fixture():
    from rri_nmf_amd import sklearn_interface as si
    A, new_A = load('recsys_data_train.npz'), load('recsys_data_test.npz')
    assert A.shape == (100, 200) and A.nnz == 617 and new_A.shape[1] == 200
    kw = dict(random_state=0, max_iter=8, use_validation_early_stopping=False, nmf_kwargs={'device_init': True})
    with lib().DeviceCorpus(A) as corpus:
        E = si.NMF_RS_Estimator(100, 200, 5, **kw).fit_corpus(corpus, keep_seen=False)
    with lib().DeviceCorpus(new_A) as new:
        mem = lib().device_memory()
        W_new = E.transform_corpus(new)
        assert lib().device_memory() == mem and W_new.shape == (new_A.shape[0], 5)
        assert E.nmf_kwargs == {'device_init': True}
        W_host = E.transform(new_A)
        M = (new_A != 0).toarray()
        # denominators near 1e-27 make W itself incomparable on this fixture (test_weighted_recsys_fixture): the masked reconstruction
        err = relfro(M * (W_new @ E.T), M * (W_host @ E.T))
        print('transform_corpus vs transform on the fixture: M.(W T) %.3e' % err)
        assert err < 1e-6
        check_served(E, new, new_A, W_new)


def test_transform_corpus_on_a_synthetic_corpus():
    from rri_nmf_amd import nmf as nmf_mod, sklearn_interface as si
    n, d, k = 300, 120, 4
    A, X, M, W0, T0 = fo.problem(n, d, k, 0.15, seed=7)
    A.data = np.round(1.0 + 4.0 * A.data / A.data.max(), 3)
    new_A = fo.problem(n, d, k, 0.2, seed=9)[0]
    new_A.data = np.round(1.0 + 4.0 * new_A.data / new_A.data.max(), 3)
    kw = dict(random_state=0, max_iter=6, use_validation_early_stopping=False, nmf_kwargs={'device_init': True})
    with lib().DeviceCorpus(A) as corpus:
        E = si.NMF_RS_Estimator(n, d, k, **kw).fit_corpus(corpus, keep_seen=False)
    with lib().DeviceCorpus(new_A) as new:
        W_new, W_host = E.transform_corpus(new), E.transform(new_A)
        err = relfro(W_new, W_host)
        print('transform_corpus vs transform, 300 x 120: W %.3e' % err)
        assert err < 1e-10
        check_served(E, new, new_A, W_new)
        # the solver's own report: every sweep of the call one launch; a rank above 64 runs launch by launch and says so
        soln = nmf_mod.nmf(new, k, observed_only=True, fold_in=True, fix_T=True, T_in=E.T, max_iter=4, eps_stop=-1, random_state=0,
                           reset_topic_method='random', device_init=True)
        assert soln['fold_info']['launches'] >= 4 and soln['fold_info']['stepped'] == 0
