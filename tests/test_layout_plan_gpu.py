"""The plan of rri_layout.hpp reaches the right members of a handle: what rri_layout_info and rri_onchip_info report equals what
the stand-alone program tests/c/layout_main.cpp prints for the same arguments and the CU count the handle reports.  The rules
themselves are checked on the CPU (tests/test_layout_cpu.py); this is the wiring.

  * a table of handles created WITHOUT an X (a large n costs the partial-sum buffers only, every handle stays under 256 MB): each
    of the five flavours in every storage type it admits, at 1 x 1, 17 x 5, one column past a panel, and at the shapes where a cap
    on the rows of a workgroup decides; the RRI_PASS_PK_GEOM cases of tests/test_xpack_refill_gpu.py.  Fields 8, 9, 10, 16, 18
    (rows per workgroup, row blocks, panels, interleaved chunks, CUs), the block counts and widths of the sparse flavours and the
    one-launch T-row route of the dense weighted one.  (The dense weighted handle whose LDS cap of 256 rows decides needs 4.2
    million rows, 72 bytes each: 300 MB.  The table has 3400000 x 4 instead, 248 MB and 208 rows per workgroup; the cap itself
    is in the CPU test.)
  * eligibility for the persistent sweep at the smallest shapes of tests/onchip_cases.py on both sides of its limits, with X, W,
    T and the parameters set;
  * a pattern-only handle and a CSR-X handle with the smallest pattern of tests/wsb_cases.py that gives a block two work items:
    fields 0 .. 7."""
import numpy as np
import pytest

import layout_cases as lc
import onchip_cases as oc
import wsb_cases as wc

pytestmark = pytest.mark.gpu

F32, F64, F16, U8 = np.float32, np.float64, np.float16, np.uint8
PW = {F32: 1024, F64: 512, F16: 2048, U8: 2048}          # columns of a panel
FLAVOURS = {lc.UNWEIGHTED: {}, lc.WEIGHTED_DENSE: dict(weighted=True), lc.WEIGHTED_SPARSE: dict(weighted='sparse'),
            lc.UNWEIGHTED_RESIDUAL: dict(schedule='residual'), lc.UNWEIGHTED_SPARSE: dict(sparse_x=True)}
GEOM = 'RRI_PASS_PK_GEOM'


def table():
    """(n, d, k, dtype, flavour, RRI_PASS_PK_GEOM or None)"""
    out = []
    for fl, dtypes in ((lc.UNWEIGHTED, (F32, F64, F16, U8)), (lc.WEIGHTED_DENSE, (F32, F64)), (lc.WEIGHTED_SPARSE, (F32, F64)),
                       (lc.UNWEIGHTED_RESIDUAL, (F32, F64)), (lc.UNWEIGHTED_SPARSE, (F32, F64))):
        for dt in dtypes:
            out += [(1, 1, 1, dt, fl, None), (17, 5, 2, dt, fl, None), (33, PW[dt] + 1, 2, dt, fl, None)]
    out += [(100000, 10000, 2, F32, lc.UNWEIGHTED, None), (100000, 10000, 2, F32, lc.UNWEIGHTED, '560i'), (100000, 10000, 2, F64, lc.UNWEIGHTED, None),
            (286721, 2056, 2, U8, lc.UNWEIGHTED, None), (286721, 2056, 2, F16, lc.UNWEIGHTED, None), (6011, 4099, 2, U8, lc.UNWEIGHTED, None),
            (60007, 10004, 2, F32, lc.UNWEIGHTED, None),
            (3400000, 4, 1, F32, lc.UNWEIGHTED_RESIDUAL, None), (500000, 64, 2, F32, lc.UNWEIGHTED_RESIDUAL, None),
            (3400000, 4, 1, F32, lc.WEIGHTED_DENSE, None), (2048, 37, 3, F32, lc.WEIGHTED_DENSE, None), (2049, 37, 3, F64, lc.WEIGHTED_DENSE, None),
            # block widths at the cap of the blocked store and one past it (wsb_cases.sp_block_cap)
            (40, wc.sp_block_cap('fp32', False) + 1, 2, F32, lc.WEIGHTED_SPARSE, None), (40, wc.sp_block_cap('fp64', False), 2, F64, lc.WEIGHTED_SPARSE, None),
            (wc.SPX_BLOCK_CAP + 1, 40, 2, F32, lc.UNWEIGHTED_SPARSE, None)]
    out += [(200, 1030, 2, F32, lc.UNWEIGHTED, g) for g in ('48c', '48i', '40i', '16', '100000c')]
    out += [(600000, 1024, 2, F32, lc.UNWEIGHTED, None), (600000, 1024, 2, F32, lc.UNWEIGHTED, '448c'), (600000, 1024, 2, F64, lc.UNWEIGHTED, '448c')]
    return out


def geom_switch(text):
    if text is None:
        return dict()
    rows = int(text.rstrip('ic'))
    return dict(pk_rows=rows, pk_il=1 if text.endswith('i') else 0 if text.endswith('c') else -1)


def onchip_subset(n_cu):
    keys = ('cols-d3-', 'cols-d2049-', 'cols-d1025-', 'rows-nG+1-', 'rank-k2-', 'rank-k65-', 'rpw-cap-kt3-', 'rpw-cap+1-kt3-', 'wlds-9')
    return [c for c in oc.edge_cases(n_cu) if c.name.startswith(keys)]


def test_handles_report_what_the_plan_says(monkeypatch, tmp_path):
    from rri_nmf_amd.engine import RRIEngine, device_memory
    monkeypatch.delenv(GEOM, raising=False)
    base = device_memory()
    # 1. the handles, and what each reports
    reports = []
    for n, d, k, dt, fl, geom in table():
        if geom is not None:
            monkeypatch.setenv(GEOM, geom)
        with RRIEngine(n, d, k, dtype=dt, **FLAVOURS[fl]) as e:
            info = e.layout_info()
            nbytes = device_memory()[1] - base[1]
        monkeypatch.delenv(GEOM, raising=False)
        assert nbytes < 256e6, (n, d, k, dt, fl, nbytes)
        reports.append(info)
    n_cu = reports[0]['n_cu']
    assert n_cu >= 1 and all(r['n_cu'] == n_cu for r in reports)

    eligible = []
    cases = onchip_subset(n_cu)
    assert any(c.expect_eligible for c in cases) and not all(c.expect_eligible for c in cases)
    for c in cases:
        rs = np.random.RandomState(3)
        X = oc.as_stored(0.1 + rs.rand(c.n, c.d), c.store)
        with RRIEngine(c.n, c.d, c.k, dtype=oc.STORES[c.store]) as e:
            e.upload_X(X)
            e.set_W(0.1 + rs.rand(c.n, c.k)); e.set_T(0.1 + rs.rand(c.k, c.d)); e.set_params(**c.flags)
            eligible.append((e.onchip_info()[0], e.layout_info()))

    name = 'k=70-csr'
    make = dict((c[0], c[1]) for c in wc.blocked_cases())[name]
    A = make()
    stored = []
    for fl in (lc.WEIGHTED_SPARSE, lc.UNWEIGHTED_SPARSE):
        with RRIEngine(A.shape[0], A.shape[1], 3, dtype=F32, **FLAVOURS[fl]) as e:
            (e.upload_X_csr if fl == lc.UNWEIGHTED_SPARSE else e.upload_observed_csr)(A)
            stored.append(e.layout_info())
    assert device_memory() == base

    # 2. the program, once, for the same arguments
    s = lc.Session()
    plans = [s.ask(lc.plan_line(n, d, k, lc.code_of(dt), fl, n_cu, **geom_switch(geom))) for n, d, k, dt, fl, geom in table()]
    shapes = [(s.ask(lc.plan_line(c.n, c.d, c.k, lc.DTYPE_CODE[c.store], n_cu=n_cu)),
               s.ask('onchip %d %d %d %d %d %d' % (c.n, -(-c.d // (4 if c.store == 'fp32' else 2)) * (4 if c.store == 'fp32' else 2), c.k,
                                                   c.store == 'fp32', oc.projected(c.flags), n_cu))) for c in cases]
    copies = [[s.ask(lc.copy_line(A, w, fl == lc.UNWEIGHTED_SPARSE, 4, n_cu)) for w in (0, 1)] for fl in (lc.WEIGHTED_SPARSE, lc.UNWEIGHTED_SPARSE)]
    copy_plans = [s.ask(lc.plan_line(A.shape[0], A.shape[1], 3, lc.RRI_F32, fl, n_cu)) for fl in (lc.WEIGHTED_SPARSE, lc.UNWEIGHTED_SPARSE)]
    s.run(lc.build_program(tmp_path, sanitize=False))

    def same_pass_geometry(info, plan, tag):
        want = (plan['rpb'], plan['nrb'], plan['npanels'], bool(plan['interleaved']) and not plan['sparse'])
        assert (info['rpb'], info['nrb'], info['npanels'], info['interleaved']) == want, (tag, info, plan)

    # 3. equality
    for row, info, i in zip(table(), reports, plans):
        plan = s[i]
        same_pass_geometry(info, plan, row)
        if plan['sparse']:
            assert info['nblk'] == (plan['sp0_nblk'], plan['sp1_nblk']) and info['bw'] == (plan['sp0_bw'], plan['sp1_bw']), (row, info, plan)
            assert (plan['npanels'], plan['nrb']) == info['nblk'], row
        else:
            assert info['nblk'] == info['bw'] == info['lps'] == info['nwork'] == (0, 0), (row, info)
        assert info['wtrow_small'] == (row[4] == lc.WEIGHTED_DENSE and bool(plan['wtrow_small'])), (row, info, plan)
    for c, (el, info), (ip, io) in zip(cases, eligible, shapes):
        same_pass_geometry(info, s[ip], c.name)
        assert el == bool(s[io]['ok']) == c.expect_eligible, (c.name, el, s[io])
    for info, (i0, i1), ip in zip(stored, copies, copy_plans):
        for f in ('nblk', 'bw', 'lps', 'nwork'):
            assert info[f] == (s[i0][f], s[i1][f]), (f, info, s[i0][f], s[i1][f])
        assert max(np.bincount(s[i0]['work'][:, 0]).max(), np.bincount(s[i1]['work'][:, 0]).max()) >= 2, 'no block with two work items'
        same_pass_geometry(info, s[ip], 'stored pattern')
