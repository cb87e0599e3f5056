"""Host side of the unweighted handle that keeps X as CSR (RRI_UNWEIGHTED_SPARSE, nmf(..., sparse_X=...)): the routing rule,
argument validation before any device work, and the agreement of header and ctypes binding on the new flavour.  No GPU."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT


def route(*a):
    from rri_nmf_amd.nmf import sparse_x_route
    return sparse_x_route(*a)


def test_route_explicit_choices():
    for x_sparse in (True, False):
        assert route(True, x_sparse, 10, 10, 4, 1e12) is True
        assert route(False, x_sparse, 10, 10, 4, 0) is False


def test_route_default_keeps_todays_route_until_the_dense_copy_does_not_fit():
    n, d = 1000, 1001                         # fp32 rows padded to 1004 entries (16 bytes)
    dense = n * 1004 * 4
    assert route(None, True, n, d, 4, dense) is False           # just fits: densified, as before
    assert route(None, True, n, d, 4, dense - 1) is True        # one byte short: kept as CSR
    assert route(None, True, n, d, 8, n * 1002 * 8) is False    # fp64: 1002 entries per row
    assert route(None, True, n, d, 8, n * 1002 * 8 - 1) is True
    assert route(None, False, n, d, 4, 0) is False              # a dense X never goes sparse by default


def test_route_rejects_other_values():
    with pytest.raises(ValueError):
        route('yes', True, 1, 1, 4, 0)


@pytest.mark.parametrize('kw, word', [
    (dict(W_mat=np.ones((6, 5))), 'W_mat'),
    (dict(schedule='residual'), 'residual'),
    (dict(group=object()), 'group'),
    (dict(w_row=np.ones(6)), 'w_row'),
    (dict(store_gradients=True), 'store_gradients'),
    (dict(eps_gauss_t=1.0, delta_gauss_t=0.1), 'Gaussian'),
])
def test_sparse_X_true_refuses_what_the_handle_cannot_do(kw, word):
    from rri_nmf_amd.nmf import nmf
    X = sp.random(6, 5, density=0.5, random_state=0, format='csr')
    with pytest.raises(ValueError, match=word):
        nmf(X, 2, sparse_X=True, max_iter=1, **kw)


def test_sparse_X_must_be_a_flag():
    from rri_nmf_amd.nmf import nmf
    with pytest.raises(ValueError, match='sparse_X'):
        nmf(np.ones((6, 5)), 2, sparse_X='auto', max_iter=1)


def test_engine_refuses_sparse_x_with_weights_or_the_residual_schedule():
    from rri_nmf_amd.engine import RRIEngine
    from rri_nmf_amd import _capi
    try:
        _capi.load_library()
    except Exception:               # noqa: BLE001 -- the checks come before the library is asked anything
        pass
    with pytest.raises(ValueError, match='sparse_x'):
        RRIEngine(10, 10, 2, weighted=True, sparse_x=True)
    with pytest.raises(ValueError, match='sparse_x'):
        RRIEngine(10, 10, 2, schedule='residual', sparse_x=True)


def test_header_and_binding_agree_on_the_flavours():
    from rri_nmf_amd import _capi
    text = open(os.path.join(ROOT, 'include', 'rri_hip.h')).read()
    m = re.search(r'enum\s*\{\s*(RRI_UNWEIGHTED\s*=.*?)\};', text, re.S)
    assert m, 'flavour enum not found in the header'
    values = dict((k, int(v)) for k, v in re.findall(r'(RRI_\w+)\s*=\s*(\d+)', m.group(1)))
    assert values['RRI_UNWEIGHTED_SPARSE'] == 4
    for name, v in values.items():
        assert getattr(_capi, name) == v, name
