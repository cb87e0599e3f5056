"""Host matrices with a row stride larger than their width (include/rri_hip.h: "`ld` arguments are row strides in ELEMENTS").

RRIEngine makes every host array C-contiguous and reads W, T and the residual into contiguous arrays, so through it the host
ld always equals the column count.  Here the library is called directly (e._lib / e._h, as tests/test_handle_memory_gpu.py
does) with ld = cols + 3:

  * inputs (rri_upload_X, rri_upload_mask, rri_set_W -- the transposing route --, rri_set_T): the pad holds NaN, and the handle
    must end in the state the contiguous call leaves: the same bits of get_W / get_T / objective, and of W and T after a sweep;
  * outputs (rri_get_W, rri_get_T, rri_get_residual): the buffer is prefilled with a sentinel bit pattern; the columns below
    `cols` equal the contiguous call bit for bit and the pad keeps the sentinel;
  * ld < cols, or a host type the call does not take: RRI_ERR_INVALID, nothing changed.

Shapes: (n, d, k) = (203, 141, 5) -- ragged in every tile, pad columns in the handle's own stride -- and (1, 37, 1).

A uint8 handle (RRI_U8) takes its counts from float32, float64 and uint8 host buffers.  The pad of a float buffer holds NaN, which
is no count and would be refused if it were read; the pad of a byte buffer holds 0xFF, which no element of the matrix does.  What
is compared is the stored matrix, both scale vectors, and the state as for every other store.
"""
import numpy as np
import pytest

from rri_nmf_amd import _capi
from rri_nmf_amd.engine import _NP2RRI
from rri_nmf_amd.synthetic import planted_X, scaled_init

pytestmark = pytest.mark.gpu

SHAPES = {'n203xd141xk5': (203, 141, 5), 'n1xd37xk1': (1, 37, 1)}
PAD = 3
F = {'fp32': np.float32, 'fp64': np.float64, 'fp16': np.float16, 'u8': np.uint8}
SENTINEL = {2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def engine(*a, **kw):
    from rri_nmf_amd.engine import RRIEngine
    return RRIEngine(*a, **kw)


def problem(n, d, k):
    X = planted_X(n, d, max(k, 2), seed=n + d, dtype=np.float64) + 0.05
    W0, T0 = scaled_init(X, k, seed=n + d + 1)
    return X, W0, T0


def count_problem(n, d, k):
    """counts 0 .. 254 with zeros, row and column scales over 0.1 .. 10, and a start scaled to (C * s) * r[:, None]"""
    X, _, _ = problem(n, d, k)
    C = np.minimum(np.round(40.0 * (X - 0.05) / X.mean()), 254.0)
    C[:, d // 4] = 0.0
    rs = np.random.RandomState(n + d + 2)
    r, s = 10.0 ** rs.uniform(-1, 1, n), 10.0 ** rs.uniform(-1, 1, d)
    W0, T0 = scaled_init((C * s) * r[:, None], k, seed=n + d + 1)
    return C, r, s, W0, T0


def stored_matrix(e):
    return e.X_times(np.eye(e.d))


def padded(a, fill=np.nan):
    """a copy of `a` inside rows of cols + PAD elements, the pad filled; returns (buffer, ld)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        fill = 0xFF
    buf = np.full((a.shape[0], a.shape[1] + PAD), fill, dtype=a.dtype)
    buf[:, :a.shape[1]] = a
    return buf, buf.shape[1]


def call(e, name, arr, ld):
    return getattr(e._lib, name)(e._h, arr.ctypes.data, int(ld), _NP2RRI[arr.dtype])


def state(e):
    """what the handle holds, and what one sweep makes of it"""
    out = [e.get_W(), e.get_T(), e.objective()]
    e.sweep(1)
    return out + [e.get_W(), e.get_T()]


def assert_same_state(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        assert np.isfinite(y).all(), '%s: value %d is not finite' % (what, i)
        assert x.tobytes() == y.tobytes(), '%s: value %d differs from the contiguous call in %d element(s)' % (what, i, int((x != y).sum()))


def flavour_kw(flavour):
    return {'plain': {}, 'weighted': dict(weighted=True), 'residual': dict(schedule='residual')}[flavour]


def load(e, X, M, W0, T0, strided, host):
    """every input through the library: contiguous (ld = cols) or with ld = cols + PAD and NaN in the pad"""
    for name, a in (('rri_upload_X', X.astype(host['X'])), ('rri_upload_mask', None if M is None else M.astype(host['M'])),
                    ('rri_set_W', W0.astype(host['W'])), ('rri_set_T', T0.astype(host['T']))):
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        buf, ld = padded(a) if name in strided else (a, a.shape[1])
        assert call(e, name, buf, ld) == _capi.RRI_OK, (name, e._err())
    e.set_params(reset_topic_method=None, **({'t_row_sum': 1.0} if M is not None else {}))


INPUTS = [('plain', store, hx, which) for store in ('fp32', 'fp64') for hx in ('fp32', 'fp64')
          for which in ('rri_upload_X', 'rri_set_W', 'rri_set_T')]
INPUTS += [('plain', 'fp16', hx, 'rri_upload_X') for hx in ('fp16', 'fp32', 'fp64')]
INPUTS += [('weighted', store, hx, 'rri_upload_mask') for store in ('fp32', 'fp64') for hx in ('fp32', 'fp64')]


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('flavour,store,host,which', INPUTS, ids=['%s-%s-handle-%s-host-%s' % p for p in INPUTS])
def test_a_strided_input_leaves_the_state_of_the_contiguous_call(flavour, store, host, which, shape):
    """`which` is the one call made with ld = cols + 3; `host` is the type of that call's host buffer (the others: float64,
    and X in the handle's type)"""
    n, d, k = SHAPES[shape]
    X, W0, T0 = problem(n, d, k)
    M = None
    if flavour == 'weighted':
        M = (np.random.RandomState(n).rand(n, d) < 0.5).astype(np.float64)
        M[0, :] = 1.0
        M[:, 0] = 1.0
    types = dict(X=F[store], M=np.float64, W=np.float64, T=np.float64)
    types[{'rri_upload_X': 'X', 'rri_upload_mask': 'M', 'rri_set_W': 'W', 'rri_set_T': 'T'}[which]] = F[host]
    out, err = [], []
    for strided in ((), (which,)):
        with engine(n, d, k, dtype=F[store], **flavour_kw(flavour)) as e:
            load(e, X, M, W0, T0, strided, types)
            err.append(e.storage_relerr)
            out.append(state(e))
    assert_same_state(out[0], out[1], '%s with ld = cols + %d' % (which, PAD))
    assert err[0] == err[1] and np.isfinite(err[1]), ('rri_storage_error', err)
    if store == 'fp16' and host != 'fp16':
        assert err[1] > 0.0, 'the upload rounded: rri_storage_error must say so'


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('host', ['fp32', 'fp64', 'u8'])
def test_strided_counts_leave_the_state_of_the_contiguous_call(host, shape):
    """rri_upload_X of a uint8 handle with ld = d + 3 from each host type it takes: the stored matrix, both scale vectors (ones
    after an upload, whatever they were), the storage error and the state after set factors and one sweep"""
    n, d, k = SHAPES[shape]
    C, r, s, W0, T0 = count_problem(n, d, k)
    a = np.ascontiguousarray(C.astype(F[host]))
    out = []
    for strided in (False, True):
        with engine(n, d, k, dtype=np.uint8) as e:
            e.upload_X(np.zeros((n, d), dtype=np.uint8))
            e.set_X_scales(r, s)                      # the upload below must put them back
            buf, ld = padded(a) if strided else (a, d)
            if strided:
                assert not (buf[:, d:] <= 255).any() if host != 'u8' else ((buf[:, d:] == 0xFF).all() and (a != 0xFF).all())
            assert call(e, 'rri_upload_X', buf, ld) == _capi.RRI_OK, e._err()
            got = [stored_matrix(e)] + list(e.X_scales()) + [e.storage_relerr]
            assert np.array_equal(got[0], C) and np.array_equal(got[1], np.ones(n)) and np.array_equal(got[2], np.ones(d)) and got[3] == 0.0
            e.set_X_scales(r, s)
            e.set_W(W0); e.set_T(T0); e.set_params(reset_topic_method=None)
            out.append(got + [stored_matrix(e)] + state(e))
    assert_same_state(out[0], out[1], 'rri_upload_X of counts with ld = cols + %d from %s' % (PAD, host))


OUTPUTS = [('plain', store, hx, which) for store in ('fp32', 'fp64') for hx in ('fp32', 'fp64') for which in ('rri_get_W', 'rri_get_T')]
OUTPUTS += [('residual', store, hx, 'rri_get_residual') for store in ('fp32', 'fp64') for hx in ('fp32', 'fp64')]


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('flavour,store,host,which', OUTPUTS, ids=['%s-%s-handle-%s-host-%s' % p for p in OUTPUTS])
def test_a_strided_output_fills_its_columns_and_keeps_the_pad(flavour, store, host, which, shape):
    n, d, k = SHAPES[shape]
    X, W0, T0 = problem(n, d, k)
    rows, cols = {'rri_get_W': (n, k), 'rri_get_T': (k, d), 'rri_get_residual': (n, d)}[which]
    dt = np.dtype(F[host])
    with engine(n, d, k, dtype=F[store], **flavour_kw(flavour)) as e:
        e.upload_X(X.astype(F[store])); e.set_W(W0); e.set_T(T0); e.set_params(reset_topic_method=None)
        if flavour == 'residual':
            e.residual_rebuild()
        else:
            e.sweep(1)
        want = np.empty((rows, cols), dtype=dt)
        assert call(e, which, want, cols) == _capi.RRI_OK, e._err()
        got = np.empty((rows, cols + PAD), dtype=dt)
        bits = got.view(UINT[dt.itemsize])
        bits[...] = SENTINEL[dt.itemsize]
        assert call(e, which, got, cols + PAD) == _capi.RRI_OK, e._err()
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        assert got[:, :cols].tobytes() == want.tobytes(), '%s: the columns differ from the contiguous call' % which
        assert (bits[:, cols:] == SENTINEL[dt.itemsize]).all(), '%s wrote %d element(s) of the pad' % (
            which, int((bits[:, cols:] != SENTINEL[dt.itemsize]).sum()))
        # ld < cols: refused, the buffer and the handle untouched
        if cols > 1:
            small = np.empty((rows, cols), dtype=dt)
            sb = small.view(UINT[dt.itemsize])
            sb[...] = SENTINEL[dt.itemsize]
            assert call(e, which, small, cols - 1) == _capi.RRI_ERR_INVALID
            assert (sb == SENTINEL[dt.itemsize]).all()
            again = np.empty((rows, cols), dtype=dt)
            assert call(e, which, again, cols) == _capi.RRI_OK and again.tobytes() == want.tobytes()


@pytest.mark.parametrize('flavour,store', [('plain', 'fp32'), ('plain', 'fp64'), ('plain', 'fp16'), ('weighted', 'fp64'), ('plain', 'u8')])
def test_a_refused_input_changes_nothing(flavour, store):
    """ld < cols, a NULL host pointer and a host type the call does not take: RRI_ERR_INVALID, and W, T, the objective and rri_storage_error are what
    they were (a float16 handle used to lose its X, and every handle its storage error, before the arguments were looked at).
    A uint8 handle with scales: its stored matrix and both scale vectors too; float16 halves are no host type of its X."""
    n, d, k = SHAPES['n203xd141xk5']
    X, W0, T0 = problem(n, d, k)
    M = (np.random.RandomState(1).rand(n, d) < 0.5).astype(np.float64) if flavour == 'weighted' else None
    Xin = X if store == 'fp16' else X.astype(F[store])          # (float16: rounded at upload, so rri_storage_error is not zero)
    scales = None
    if store == 'u8':
        X, r, s, W0, T0 = count_problem(n, d, k)
        Xin, scales = X.astype(np.uint8), (r, s)

    def seen(e):
        out = (e.get_W(), e.get_T(), e.objective(), e.storage_relerr)
        return out + ((stored_matrix(e),) + e.X_scales() if scales else ())
    with engine(n, d, k, dtype=F[store], **flavour_kw(flavour)) as e:
        e.upload_X(Xin)
        if scales:
            e.set_X_scales(*scales)
        if M is not None:
            e.upload_mask(M)
        e.set_W(W0); e.set_T(T0); e.set_params(reset_topic_method=None, **({'t_row_sum': 1.0} if M is not None else {}))
        before = seen(e)
        assert (before[3] > 0.0) is (store == 'fp16')
        if scales:
            assert np.array_equal(before[4], (X * s) * r[:, None]) and np.array_equal(before[5], r) and np.array_equal(before[6], s)
        other = (X + 1.0 if scales else 2.0 * X + 1.0), 3.0 * W0 + 1.0, 3.0 * T0 + 1.0         # (counts: still counts)
        calls = [('rri_upload_X', other[0].astype(F[store]), d), ('rri_upload_X', other[0], d),
                 ('rri_set_W', other[1], k), ('rri_set_T', other[2], d)]
        if M is not None:
            calls.append(('rri_upload_mask', 1.0 - M, d))
        for name, a, cols in calls:
            a = np.ascontiguousarray(a)
            assert call(e, name, a, cols - 1) == _capi.RRI_ERR_INVALID, name
            assert 'ld=' in e._err()
            after = seen(e)
            assert_same_state(before, after, name + ' with ld = cols - 1')
        # no host matrix at all: a NULL pointer with a good ld and a type the call takes (the refusal that shares its branch with ld)
        nulls = [('rri_upload_X', d, _NP2RRI[np.dtype(F[store])]), ('rri_upload_X', d, _capi.RRI_F64), ('rri_set_W', k, _capi.RRI_F64),
                 ('rri_set_T', d, _capi.RRI_F64)]
        if M is not None:
            nulls.append(('rri_upload_mask', d, _capi.RRI_F64))
        for name, cols, code in nulls:
            assert getattr(e._lib, name)(e._h, None, cols, code) == _capi.RRI_ERR_INVALID, (name, code)
            assert 'bad host matrix' in e._err(), (name, code, e._err())
            after = seen(e)
            assert_same_state(before, after, '%s with a NULL host pointer' % name)
        # a host type the call does not take: no such code at all, and halves for anything but the X of a float16 handle
        bad_types = [('rri_upload_X', 99), ('rri_set_W', 99), ('rri_set_T', 99), ('rri_set_W', _capi.RRI_F16)]
        if store != 'fp16':
            bad_types.append(('rri_upload_X', _capi.RRI_F16))
        if store == 'u8':
            bad_types += [('rri_set_W', _capi.RRI_U8), ('rri_set_T', _capi.RRI_U8)]     # bytes are a host type of its X alone
        if M is not None:
            bad_types += [('rri_upload_mask', 99), ('rri_upload_mask', _capi.RRI_F16)]
        room = np.ones((max(n, k), max(d, k)))                  # large enough for any of them, whatever the type is read as
        for name, code in bad_types:
            assert getattr(e._lib, name)(e._h, room.ctypes.data, room.shape[1], code) == _capi.RRI_ERR_INVALID, (name, code)
            assert 'host dtype' in e._err(), (name, code, e._err())
            after = seen(e)
            assert_same_state(before, after, '%s with host type %d' % (name, code))
        e.sweep(1)
        swept = e.get_W(), e.get_T()
    with engine(n, d, k, dtype=F[store], **flavour_kw(flavour)) as e:
        e.upload_X(Xin)
        if scales:
            e.set_X_scales(*scales)
        if M is not None:
            e.upload_mask(M)
        e.set_W(W0); e.set_T(T0); e.set_params(reset_topic_method=None, **({'t_row_sum': 1.0} if M is not None else {}))
        e.sweep(1)
        assert_same_state((e.get_W(), e.get_T()), swept, 'a sweep after the refused calls')


@pytest.mark.parametrize('store', ['fp32', 'fp64', 'fp16', 'u8'])
def test_a_column_slice_given_to_the_engine_equals_its_copy(store):
    """through RRIEngine: a column-sliced numpy view (Xw[:, 3:3 + d], strides (ld, 1)) given to upload_X / set_T / set_W
    (uint8 counts: the columns beside the slice hold 0xFF; scales are set on both handles after the upload)"""
    n, d, k = SHAPES['n203xd141xk5']
    X, W0, T0 = problem(n, d, k)
    wide = lambda a: np.pad(a, ((0, 0), (3, 4)), constant_values=0xFF if a.dtype == np.uint8 else np.nan)[:, 3:3 + a.shape[1]]
    scales = None
    if store == 'u8':
        X, r, s, W0, T0 = count_problem(n, d, k)
        scales = (r, s)
    Xs = X.astype(F[store])
    out = []
    for view in (False, True):
        with engine(n, d, k, dtype=F[store]) as e:
            args = [wide(a) if view else np.ascontiguousarray(a) for a in (Xs, W0, T0)]
            assert args[0].flags['C_CONTIGUOUS'] is not view
            e.upload_X(args[0]); e.set_W(args[1]); e.set_T(args[2]); e.set_params(reset_topic_method=None)
            if scales:
                e.set_X_scales(*scales)
            out.append([stored_matrix(e)] + state(e))
    assert_same_state(out[0], out[1], 'a column-sliced view')
