"""Who owns device memory: every device buffer of a handle is allocated by dev_alloc (or handed over by dev_adopt),
listed in the handle and freed by dev_release or rri_destroy; X, the mask and the reduce buffer may be bound caller memory
instead, which is neither listed nor freed.

Everything here is an exact integer equality on rri_device_memory (engine.device_memory): the buffers and bytes that the handles
of this process own.  No numerics, no tolerance.  torch.cuda.mem_get_info is device-wide and moves with other processes on a
shared device, so it is not used.  Every case collects garbage and reads its own baseline first: fixtures of other modules may
hold handles.  Nothing is tested by making an allocation fail.

Shapes: n, d, k = 300, 130, 5 -- pad columns in every storage type (LD = 132 in float32, 136 in float64, float16 and uint8); d = 128 for
the bind cases (rri_bind_X_device refuses pad columns); the persistent sweep at (50, 30, 3), the smallest shape of
tests/test_onchip_gpu.py.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import scipy.sparse as sp

from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu

N, D, K = 300, 130, 5
D_BIND = 128


def memory():
    from rri_nmf_amd.engine import device_memory
    return device_memory()


def baseline():
    gc.collect()
    return memory()


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def ld_of(d, dtype):
    vn = 8 if np.dtype(dtype) == np.uint8 else 16 // np.dtype(dtype).itemsize       # uint8 counts: 8-byte loads
    return -(-d // vn) * vn


def problem(d=D, seed=0, n=N, k=K):
    X = planted_X(n, d, k, seed=seed, dtype=np.float64)
    W0, T0 = scaled_init(X, k, seed=seed + 1)
    return X, W0, T0


def mask01(d=D, density=0.05, seed=2):
    return (np.random.RandomState(seed).rand(N, d) < density).astype(np.float64)


def reset_max_resid(e, t):
    row = C.c_int64(-1)
    e._check(e._lib.rri_apply_reset_max_resid(e._h, int(t), C.byref(row)))
    return int(row.value)


# flavour -> (RRIEngine keywords, upload(e, X)).  The sparse flavours see X on a 20 % pattern (no empty row).
def _dense(e, X):
    e.upload_X(X.astype(e.dtype))


def counts_of(X):
    """counts 0 .. 255 with the values of X at 40 on average"""
    return np.minimum(np.round(40.0 * X / X.mean()), 255.0).astype(np.uint8)


def scales_of(X, seed=6):
    """row and column scales that take counts_of(X) back to the size of X (the factors of problem() start there)"""
    rs = np.random.RandomState(seed)
    return (X.mean() / 40.0) * (0.5 + rs.rand(X.shape[0])), 0.5 + rs.rand(X.shape[1])


def _counts(e, X):
    """uint8 counts: X is the handle's, and so are the two scale vectors (n and LD float64, there from rri_create on)"""
    created = memory()
    e.upload_X(counts_of(X))
    own = memory()
    assert own == (created[0] + 1, created[1] + X.shape[0] * ld_of(X.shape[1], np.uint8)), (own, created)
    e.set_X_scales(*scales_of(X))
    assert memory() == own, 'rri_set_X_scales writes the vectors the handle has'


def _weighted_fp(e, X):
    e.upload_X(X)
    e.upload_mask(0.25 + np.random.RandomState(3).rand(N, D))


def _weighted_01(e, X):
    e.upload_X(X)
    e.upload_mask(mask01())


def _pattern(e, X):
    e.upload_observed_csr(sp.csr_matrix(X * mask01(density=0.2)))


def _csr(e, X):
    e.upload_X_csr(sp.csr_matrix(X * mask01(density=0.2)))


FLAVOURS = {
    'unweighted-f32': (dict(dtype=np.float32), _dense),
    'unweighted-f64': (dict(dtype=np.float64), _dense),
    'unweighted-f16': (dict(dtype=np.float16), _dense),
    'unweighted-residual': (dict(dtype=np.float32, schedule='residual'), _dense),
    'weighted-dense-fp-mask': (dict(dtype=np.float64, weighted=True), _weighted_fp),
    'weighted-dense-01-mask': (dict(dtype=np.float64, weighted=True), _weighted_01),
    'weighted-sparse': (dict(dtype=np.float64, weighted='sparse'), _pattern),
    'unweighted-sparse': (dict(dtype=np.float64, sparse_x=True), _csr),
    'unweighted-u8': (dict(dtype=np.uint8), _counts),
}


@pytest.mark.parametrize('flavour', sorted(FLAVOURS))
def test_close_returns_everything(flavour):
    """create, upload, factors, parameters, two sweeps, objective, snapshot and rollback, both kinds of reset: buffers and bytes
    are above the baseline while the handle lives and back at it after close()"""
    kw, upload = FLAVOURS[flavour]
    base = baseline()
    X, W0, T0 = problem()
    e = engine(N, D, K, **kw)
    try:
        upload(e, X)
        e.set_W(W0), e.set_T(T0)
        e.set_params(reset_topic_method=None)
        e.sweep(2)
        e.objective()
        e.snapshot()
        e.rollback()
        row = np.random.RandomState(4).rand(D)
        e.apply_reset_vectors(1, row / row.sum(), e.get_W()[:, 1])          # resetT, resetW
        before_rowpos = memory()
        reset_max_resid(e, 2)                                               # rowpos
        assert memory()[0] > before_rowpos[0] and memory()[1] >= before_rowpos[1] + N * 8, (memory(), before_rowpos)
        e.sweep(1)
        if flavour == 'weighted-dense-01-mask':       # the packed mask at the upload, its column-major copy at the first step
            info = e.layout_info()
            assert info['mask_bits'] and info['mask_cols'], info
        alive = memory()
        print('%s: %d buffers, %d bytes' % (flavour, alive[0] - base[0], alive[1] - base[1]))
        assert alive[0] > base[0] and alive[1] > base[1], (alive, base)
    finally:
        e.close()
    assert memory() == base


def host_group(n_local):
    """a host-callback communicator of one rank (rri_comm_create_host, as RowGroup.over_torch makes one per rank): the sums, the
    gathered rows and the broadcast of a world of one are the buffers as they are"""
    from rri_nmf_amd import _capi
    from rri_nmf_amd.distributed import RowGroup

    def allgather(user, send, count, recv):
        C.memmove(recv, send, int(count) * 8)
        return 0

    cbs = (_capi.ALLREDUCE_FN(lambda user, buf, count: 0), _capi.ALLGATHER_FN(allgather),
           _capi.BROADCAST_FN(lambda user, buf, count, root: 0))
    comm = C.c_void_p()
    assert _capi.load_library().rri_comm_create_host(C.byref(comm), 0, 1, cbs[0], cbs[1], cbs[2], None) == _capi.RRI_OK
    return RowGroup(comm, 0, 1, [n_local], keep=cbs)


def test_lazy_buffers_of_the_persistent_sweep(monkeypatch):
    """the nine arrays of the register-resident sweep and the two rollback copies appear with its first launch"""
    monkeypatch.setenv('RRI_ONCHIP', '1')           # read at rri_create
    n, d, k = 50, 30, 3
    base = baseline()
    X, W0, T0 = problem(d=d, seed=5, n=n, k=k)
    e = engine(n, d, k, dtype=np.float32)
    try:
        e.upload_X(X.astype(np.float32)), e.set_W(W0), e.set_T(T0)
        e.set_params(reset_topic_method=None)
        ready = memory()
        assert e.onchip_info() == (True, 0)
        e.sweep(1)
        assert e.onchip_info()[1] >= 1
        assert memory()[0] > ready[0] and memory()[1] > ready[1], (memory(), ready)
        swept = memory()
        e.sweep(1)
        assert memory() == swept
    finally:
        e.close()
    assert memory() == base


def test_lazy_buffers_of_the_whole_sweep_w_half(monkeypatch):
    """T fixed: Gfull, Wsweep0, wsum_part and wsums appear with the first sweep (enqueue_wsweep)"""
    monkeypatch.delenv('RRI_WSWEEP', raising=False)
    base = baseline()
    X, W0, T0 = problem()
    e = engine(N, D, K, dtype=np.float32)
    try:
        e.upload_X(X.astype(np.float32)), e.set_W(W0), e.set_T(T0)
        e.set_params(fix_T=True, reset_topic_method=None)
        ready = memory()
        e.sweep(1)
        assert memory()[0] >= ready[0] + 4 and memory()[1] >= ready[1] + 8 * (K * K + K * N + K), (memory(), ready)
        swept = memory()
        e.sweep(1)
        assert memory() == swept
    finally:
        e.close()
    assert memory() == base


def test_lazy_buffers_of_a_group_and_attaching_twice():
    """ctail and cand appear when a group is attached; attaching again replaces cand and adds nothing"""
    base = baseline()
    X, W0, T0 = problem()
    grp = host_group(N)
    e = engine(N, D, K, dtype=np.float64)
    try:
        e.upload_X(X), e.set_W(W0), e.set_T(T0)
        e.set_params(reset_topic_method=None)
        ready = memory()
        e.attach_group(grp)
        attached = memory()
        assert attached[0] >= ready[0] + 2 and attached[1] >= ready[1] + 8 * 8 + 2 * 1 * 8, (attached, ready)
        e.attach_group(grp)
        assert memory() == attached
        e.sweep(1)
        reset_max_resid(e, 0)           # the candidates of every rank travel through cand
        used = memory()
        e.attach_group(grp)
        assert memory() == used
    finally:
        e.close()
        grp.close()
    assert memory() == base


def csr_like(A, seed):
    """another matrix of the same pattern (the same shape and nnz)"""
    B = sp.csr_matrix(A, copy=True)
    B.data = 0.5 + np.random.RandomState(seed).rand(B.nnz)
    return B


def _replace_X(e):
    for seed in (0, 7):
        e.upload_X(problem(seed=seed)[0].astype(e.dtype))
        yield None


def _replace_mask(e):
    e.upload_X(problem()[0])
    fp = lambda seed: 0.25 + np.random.RandomState(seed).rand(N, D)
    # the packed copy replaces the fp array and the other way round: the same counters whenever the same kind is back
    for kind, M in (('01', mask01(seed=2)), ('01', mask01(seed=2)[::-1].copy()), ('fp', fp(3)), ('fp', fp(4)), ('01', mask01(seed=2))):
        e.upload_mask(M)
        yield kind


def _replace_csr(method):
    def steps(e):
        A = sp.csr_matrix(problem()[0] * mask01())
        if method == 'upload_mask_csr_pattern':
            e.upload_X(problem()[0])
        for seed in (0, 8):
            getattr(e, method)(csr_like(A, seed))
            yield None
    return steps


def _replace_counts(e):
    """a second X from each of the three host types a uint8 handle takes"""
    C = counts_of(problem()[0])
    e.upload_X(C)
    yield None
    for host in (np.float32, np.float64, np.uint8):
        e.upload_X(np.ascontiguousarray(C[::-1].astype(host)))
        yield None


def _rescale_counts(e):
    """the scale vectors are written where they are; the temporaries of a normalisation are given back"""
    X = problem()[0]
    e.upload_X(counts_of(X) * (np.random.RandomState(5).rand(N, D) < 0.5))        # with zeros: a term in every document has idf 0
    yield None
    for seed in (1, 2):
        e.set_X_scales(*scales_of(X, seed))
        yield None
        e.set_X_scales(None, scales_of(X, seed + 2)[1])
        yield None
        e.scale_X(None, True)
        yield None
        e.scale_X(0.5 + np.random.RandomState(seed).rand(D), True)
        yield None
        e.preprocess(tfidf=True, normalize=True)
        yield None


REPLACEMENTS = {
    'upload_X': (dict(dtype=np.float32), _replace_X),
    'upload_mask': (dict(dtype=np.float64, weighted=True), _replace_mask),
    'upload_X_csr-dense': (dict(dtype=np.float32), _replace_csr('upload_X_csr')),
    'upload_X_csr-kept': (dict(dtype=np.float64, sparse_x=True), _replace_csr('upload_X_csr')),
    'upload_observed_csr': (dict(dtype=np.float64, weighted='sparse'), _replace_csr('upload_observed_csr')),
    'upload_mask_csr_pattern': (dict(dtype=np.float64, weighted=True), _replace_csr('upload_mask_csr_pattern')),
    'upload_X-u8': (dict(dtype=np.uint8), _replace_counts),
    'set_X_scales-u8': (dict(dtype=np.uint8), _rescale_counts),
}


@pytest.mark.parametrize('name', sorted(REPLACEMENTS))
def test_replacement_does_not_grow(name):
    """data of the same shape and nnz uploaded again leaves buffers and bytes exactly where they were"""
    kw, steps = REPLACEMENTS[name]
    base = baseline()
    e = engine(N, D, K, **kw)
    try:
        created = memory()
        seen = {}
        for kind in steps(e):
            now = memory()
            assert now[0] > created[0] and now[1] > created[1], (now, created)
            assert seen.setdefault(kind, now) == now, (name, kind, seen, now)
        assert len(seen) == (2 if name == 'upload_mask' else 1)
    finally:
        e.close()
    assert memory() == base


def test_borrowed_memory_is_not_counted_and_not_freed():
    """bound X, mask and reduce buffer: the handle's own ones are given back at the bind, the bound ones are never counted, and
    close() leaves them as they were"""
    import torch
    base = baseline()
    X, W0, T0 = problem(d=D_BIND)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0').contiguous()
    # ---- X and the reduce buffer of a plain float32 handle
    x_bytes = N * ld_of(D_BIND, np.float32) * 4
    tX = dev(X.astype(np.float32))
    e = engine(N, D_BIND, K, dtype=np.float32)
    try:
        e.upload_X(X.astype(np.float32)), e.set_W(W0), e.set_T(T0)
        e.set_params(reset_topic_method=None)
        own = memory()
        red_elems = e.reduce_buffer()[1]
        tred = torch.zeros(red_elems, dtype=torch.float64, device='cuda:0')
        torch.cuda.synchronize()
        x_sum = float(tX.sum())
        e.bind_X_device(tX.data_ptr(), D_BIND)
        assert memory() == (own[0] - 1, own[1] - x_bytes)
        e.bind_reduce_buffer(tred.data_ptr(), red_elems)
        assert memory() == (own[0] - 2, own[1] - x_bytes - red_elems * 8)
        e.sweep(1)
        swept = memory()                              # (with what the sweep allocated on first use)
        e.upload_X(X.astype(np.float32))              # the handle's own X again
        assert memory() == (swept[0] + 1, swept[1] + x_bytes)
        e.bind_X_device(tX.data_ptr(), D_BIND)
        assert memory() == swept
        e.sweep(1)
        e.synchronize()
        red_sum = float(tred.sum())
    finally:
        e.close()
    assert memory() == base
    torch.cuda.synchronize()
    assert float(tX.sum()) == x_sum and float(tred.sum()) == red_sum
    # ---- X and the mask of a weighted float64 handle (an fp mask: nothing is packed from it)
    M = 0.25 + np.random.RandomState(3).rand(N, D_BIND)
    tX, tM = dev(X), dev(M)
    e = engine(N, D_BIND, K, dtype=np.float64, weighted=True)
    try:
        created = memory()
        xm_bytes = N * ld_of(D_BIND, np.float64) * 8
        e.upload_X(X), e.upload_mask(M)               # the handle's own X and mask: one buffer each
        assert memory() == (created[0] + 2, created[1] + 2 * xm_bytes)
        torch.cuda.synchronize()
        x_sum, m_sum = float(tX.sum()), float(tM.sum())
        e.bind_X_device(tX.data_ptr(), D_BIND)
        assert memory() == (created[0] + 1, created[1] + xm_bytes)
        e.bind_mask_device(tM.data_ptr(), D_BIND)
        assert memory() == created
        e.set_W(W0), e.set_T(T0)
        e.set_params(reset_topic_method=None)
        e.sweep(1)
        swept = memory()
        e.upload_mask(M)                              # the handle's own mask in place of the bound one
        assert memory() == (swept[0] + 1, swept[1] + N * ld_of(D_BIND, np.float64) * 8)
        e.bind_mask_device(tM.data_ptr(), D_BIND)
        assert memory() == swept
        e.sweep(1)
    finally:
        e.close()
    assert memory() == base
    torch.cuda.synchronize()
    assert float(tX.sum()) == x_sum and float(tM.sum()) == m_sum


def test_counts_bound_after_an_upload_and_uploaded_after_a_bind():
    """a uint8 handle: binding gives the handle's own X back (one buffer, n x LD bytes), an upload after a bind allocates it
    again, and neither touches the two scale vectors, which stay the handle's; the bound tensor is never counted, and close()
    leaves it as it was.  (Not an entry of REPLACEMENTS: a handle with a bound X owns less than one with its own.)"""
    import torch
    base = baseline()
    X, W0, T0 = problem(d=D_BIND)
    Cn = counts_of(X)
    r, s = scales_of(X)
    x_bytes = N * ld_of(D_BIND, np.uint8)
    tC = torch.from_numpy(Cn).to('cuda:0').contiguous()
    e = engine(N, D_BIND, K, dtype=np.uint8)
    try:
        created = memory()
        e.upload_X(Cn)
        assert memory() == (created[0] + 1, created[1] + x_bytes)
        e.set_X_scales(r, s), e.set_W(W0), e.set_T(T0)
        e.set_params(reset_topic_method=None)
        own = memory()
        assert own == (created[0] + 1, created[1] + x_bytes)
        torch.cuda.synchronize()
        c_sum = int(tC.sum())
        e.bind_X_device(tC.data_ptr(), D_BIND)
        assert memory() == created
        e.set_X_scales(r, s)
        e.scale_X(None, True)                         # legal on a bound X of this store: no matrix is written
        assert memory() == created
        e.sweep(1)
        swept = memory()                              # (with what the sweep allocated on first use)
        e.upload_X(Cn)
        assert memory() == (swept[0] + 1, swept[1] + x_bytes)
        e.bind_X_device(tC.data_ptr(), D_BIND)
        assert memory() == swept
        e.upload_X(Cn.astype(np.float64))
        assert memory() == (swept[0] + 1, swept[1] + x_bytes)
        e.set_X_scales(r, s)
        e.sweep(1)
        e.synchronize()
    finally:
        e.close()
    assert memory() == base
    torch.cuda.synchronize()
    assert int(tC.sum()) == c_sum
