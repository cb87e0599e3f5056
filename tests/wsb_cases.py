"""Cases, layout formulas and rounding bounds shared by tests/test_weighted_sparse_buckets_gpu.py (device) and
tests/test_weighted_sparse_layout_cpu.py (no device).

Layout.  sp_layout / dense_layout restate what dense_plan, sp_dims and build_sp_copy (rri_nmf_amd/csrc/rri_layout.hpp) decide for a
handle; the GPU tests compare them with what the handle reports (rri_layout_info), the CPU test runs them over the case lists
below and asserts that every bucket has a case, and tests/test_layout_cpu.py holds the C++ to them over the same lists.

Bounds.  The weighted flavour keeps E = M .* (X - W T) in the storage type and rewrites it by rank-one corrections.  StepBound
carries, next to the float64 reference, a matrix B >= |E_device - E_true| entry by entry:
  * a rebuild rounds every entry once:                                   B = u |e|
  * a correction e' = e - a_i b_j stores one rounded value:              B += u (|e'| + B)
    and, where the factors pass through tables of the storage type (pattern-only handles, SpTab), multiplies two rounded
    factors, fl(a) fl(b) = a b (1 + d1)(1 + d2):                         B += (2 u + u^2) |a_i b_j|
    (tab_u = 0 on dense handles, whose passes read the float64 factors, and for float64 tables, which hold W and T exactly);
  * a topic step applies two corrections (the T-row change w dt^T, the W-column change dw t^T), so B grows twice per step
    and starts again at every rebuild (once per sweep, before topic 0).
u = 2^-24 or 2^-53 is the unit roundoff of the storage type.  A sum over a column, a_j = sum_i w_i e_ij, then carries
    |w|^T B  +  tab_u |w|^T (|E| + B)   [the summand w_i read from a table]   +  the float64 term
and nw_j = sum_i w_i^2 m_ij carries (2 tab_u + float64 term) nw_j.  The float64 term is C64 (terms + 2) 2^-53 times the same
sum over absolute values, |w|^T (M .* (|X| + |W||T|)), `terms` being the entries of the column inside the mask (the others are
exact zeros in either sum): the device adds `terms` products in some order (terms 2^-53 by the
standard forward bound of a recursive sum, any order), the reference forms every entry of the residual from k + 1 terms and
adds n of them (n + k + 2), together 2 n + k + 2 <= C64 (n + k + 2) with C64 = 2.  One safety factor SAFETY = 2 on the total,
for the second-order terms dropped above.  Nothing in a bound comes from a device result.
"""
import numpy as np
import scipy.sparse as sp

U32, U64 = 2.0 ** -24, 2.0 ** -53
C64 = 2.0
SAFETY = 2.0
STORES = {'fp32': np.float32, 'fp64': np.float64}
N_CU = 256                       # MI355X; the GPU tests pass the count the handle reports (it caps a copy's work items)
SP_BLOCK_BYTES = 120 * 1024
SPX_BLOCK_CAP = (SP_BLOCK_BYTES // 8 - 64) // 64 * 64      # 15296


def round_up(a, b):
    return -(-a // b) * b


# ---- layout restated --------------------------------------------------------------------------------------------------
def sp_block_cap(store, csrx):
    return SPX_BLOCK_CAP if csrx else SP_BLOCK_BYTES // (3 * np.dtype(STORES[store]).itemsize)


def sp_copy_layout(A, which, store, csrx, n_cu=None):
    """one blocked copy of the pattern of the scipy CSR matrix A (explicit zeros are entries): which = 0 rows as segments cut
    into column blocks, 1 columns as segments cut into row blocks.  build_sp_store, restated."""
    n, d = A.shape
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    cols = A.indices
    gdim, nseg = (d, n) if which == 0 else (n, d)
    g, s = (cols, rows) if which == 0 else (rows, cols)
    cap = sp_block_cap(store, csrx)
    nblk = -(-gdim // cap)
    bw = round_up(-(-gdim // nblk), 64)
    cnt = np.zeros((nblk, nseg), dtype=np.int64)
    np.add.at(cnt, (g // bw, s), 1)
    padded = (cnt + 3) // 4 * 4
    ptr = np.concatenate([[0], np.cumsum(padded.ravel())]).astype(np.int64)      # (block, segment) order, padded to quads
    eb = padded.sum(axis=1)
    total = int(eb.sum())
    n_cu = n_cu or N_CU
    target = max(1, n_cu // 2 if csrx else n_cu)
    spare = max(0, target - nblk)
    work = []
    for b in range(nblk):
        row = ptr[b * nseg:(b + 1) * nseg + 1]
        items = 1 + (spare * int(eb[b]) // total if total > 0 else 0)
        items = max(1, min(items, int(eb[b]) // 4096))
        s0 = 0
        for j in range(1, items + 1):
            if s0 >= nseg:
                break
            s1 = nseg
            if j < items:
                want = row[0] + int(eb[b]) * j // items
                s1 = s0 + 1 + int(np.searchsorted(row[s0 + 1:nseg], want, side='left'))
                s1 = min(max(s1, s0 + 1), nseg)
            work.append((b, s0, s1))
            s0 = s1
        if s0 < nseg:
            work.append((b, s0, nseg))
    avg = A.nnz // max(1, nblk * nseg)
    lps = 64 if avg >= 768 else 32 if avg >= 384 else 16 if avg >= 192 else 8
    return dict(nblk=nblk, bw=bw, lps=lps, nwork=len(work), work=work, seg_len=cnt, avg=avg, gdim=gdim)


def sp_layout(A, store, csrx, n_cu=None):
    return [sp_copy_layout(A, w, store, csrx, n_cu) for w in (0, 1)]


def dense_layout(n, d, store):
    """pass geometry of a dense weighted handle (rri_create) and the routes that follow from it"""
    es = np.dtype(STORES[store]).itemsize
    vn = 16 // es
    LD = round_up(d, vn)
    npanels = -(-LD // (64 * vn * 4))
    rpb_cap = ((40 * 1024 - 4 * 8 * 72 * 8) // (11 * 8)) // 16 * 16
    rpb = 0
    for total in range(16384, 511, -512):
        nrb_t = max(1, total // npanels)
        r = -(-n // nrb_t)
        if r >= 48 or total == 512:
            rpb = r
            break
    rpb = min(round_up(max(rpb, 32), 16), rpb_cap)
    nrb = -(-n // rpb)
    return dict(rpb=rpb, nrb=nrb, npanels=npanels, LD=LD, wtrow_small=nrb <= 64, interleaved=npanels * nrb <= 1024)


# ---- patterns -----------------------------------------------------------------------------------------------------------
def _csr(n, d, rows, cols, vals):
    A = sp.csr_matrix((np.asarray(vals, dtype=np.float64), (rows, cols)), shape=(n, d))      # keeps explicit zeros
    A.sort_indices()
    return A


def pat_exact(n, d, nnz, seed=0):
    """exactly nnz entries, uniformly placed"""
    rs = np.random.RandomState(seed)
    flat = np.sort(rs.choice(n * d, size=nnz, replace=False))
    return _csr(n, d, flat // d, flat % d, 0.05 + rs.rand(nnz))


def pat_density(n, d, frac, seed=0):
    return pat_exact(n, d, int(round(frac * n * d)), seed)


def pat_row_lengths(n, d, lengths, seed=0):
    """row i holds lengths[i % len(lengths)] entries at random columns"""
    rs = np.random.RandomState(seed)
    rows, cols = [], []
    for i in range(n):
        m = lengths[i % len(lengths)]
        rows += [i] * m
        cols += list(np.sort(rs.choice(d, size=m, replace=False)))
    return _csr(n, d, rows, cols, 0.05 + rs.rand(len(rows)))


def pat_dense_block_next_to_empty(n, d, width, empty_rows, seed=0):
    """columns [0, width) full except the rows `empty_rows`; one entry per row in the last column: the first column block
    takes several work items, the last a single one, and an item boundary of the first falls on the empty rows"""
    rs = np.random.RandomState(seed)
    full = np.array([i for i in range(n) if i not in set(empty_rows)])
    rows = np.concatenate([np.repeat(full, width), np.arange(n)])
    cols = np.concatenate([np.tile(np.arange(width), full.size), np.full(n, d - 1)])
    return _csr(n, d, rows, cols, 0.05 + rs.rand(rows.size))


def pat_zeros_zipf(n, d, seed=0):
    """rows and columns without entries, explicit stored zeros, and one column holding about a third of all entries"""
    rs = np.random.RandomState(seed)
    M = rs.rand(n, d) < 0.015
    M[:, 7] = True                      # the heavy column: n entries of ~ 3 n in all
    M[3:6, :] = False
    M[:, 11:14] = False
    rows, cols = np.nonzero(M)
    vals = 0.05 + rs.rand(rows.size)
    vals[::9] = 0.0
    return _csr(n, d, rows, cols, vals)


def transposed(A):
    T = sp.csr_matrix(A.T)
    T.sort_indices()
    return T


def _lps_edges():
    out = []
    for lo, n, d in ((192, 40, 400), (384, 40, 800), (768, 40, 1000)):
        for avg in (lo - 1, lo):
            # nnz // (nblk nseg) = avg: one entry short of the next quotient on the low side, exactly avg * n on the high side
            nnz = (lo * n - 1) if avg == lo - 1 else lo * n
            out.append(('avg=%d' % avg, lambda n=n, d=d, nnz=nnz: pat_exact(n, d, nnz, seed=nnz), 5))
    return out


def blocked_cases():
    """(id, pattern factory, k, flavours) -- flavours: 'pat' pattern-only weighted handle, 'csrx' X kept as CSR, or one
    (flavour, store) pair; the CSC copy sees the transposed pattern as the CSR copy sees the pattern"""
    base = [('lps=8', lambda: pat_density(60, 90, 0.3, 1), 5),
            ('lps=16', lambda: pat_density(90, 600, 0.5, 2), 5),
            ('lps=32', lambda: pat_density(70, 1100, 0.5, 3), 5),
            ('lps=64', lambda: pat_density(70, 1100, 0.8, 4), 5)] + _lps_edges() + [
            ('seglen-0-1-3-4-5-255-256-257', lambda: pat_row_lengths(40, 300, [0, 1, 3, 4, 5, 255, 256, 257], 5), 5),
            ('seglen-0-1-3-4-5-511-512-513', lambda: pat_row_lengths(40, 600, [0, 1, 3, 4, 5, 511, 512, 513], 6), 5),
            ('seglen-0-1-3-4-5-1023-1024-1025-1100', lambda: pat_row_lengths(45, 2100, [0, 1, 3, 4, 5, 1023, 1024, 1025, 1100], 10), 5),
            ('empty-zeros-heavy-column', lambda: pat_zeros_zipf(150, 130, 7), 5),
            ('k=1', lambda: pat_density(60, 90, 0.3, 8), 1),
            ('k=70', lambda: pat_density(90, 130, 0.97, 9), 70)]      # nearly every entry stored: X = W* T* + noise is close to
            # a rank-70 problem for the unweighted flavour too
    cases = []
    for name, make, k in base:
        cases.append((name + '-csr', make, k, ('pat', 'csrx')))
        cases.append((name + '-csc', lambda make=make: transposed(make()), k, ('pat', 'csrx')))
    # widths at the block cap: the cap depends on the flavour and, pattern-only, on the storage type
    for fl, st in (('pat', 'fp32'), ('pat', 'fp64'), ('csrx', 'fp32'), ('csrx', 'fp64')):
        cap = sp_block_cap(st, fl == 'csrx')
        for label, width in (('bw=cap', cap), ('bw=cap+1', cap + 1), ('bw=2cap+1', 2 * cap + 1)):
            make = lambda width=width: pat_density(40, width, 0.02, width)
            cases.append((label + '-csr', make, 5, ((fl, st),)))
            cases.append((label + '-csc', lambda make=make: transposed(make()), 5, ((fl, st),)))
    cases.append(('items-3+1-boundary-on-empty-csr', lambda: pat_dense_block_next_to_empty(40, 30593, 400, (13, 14)), 5,
                  ('pat', 'csrx')))
    return cases


def blocked_runs():
    """(case id, factory, k, flavour, store) for every run of the blocked store"""
    out = []
    for name, make, k, flavours in blocked_cases():
        for fl in flavours:
            for flavour, store in ([fl] if isinstance(fl, tuple) else [(fl, 'fp32'), (fl, 'fp64')]):
                out.append((name, make, k, flavour, store))
    return out


def run_id(r):
    return '%s-%s-%s' % (r[0], r[3], r[4])


STEP_FLAGS = {'plain': dict(),
              'topic': dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0),       # FLAGS of test_kernel_buckets_gpu
              'fix_W': dict(fix_W=True)}


# ---- the dense weighted step ---------------------------------------------------------------------------------------------
def mask01(n, d, frac, seed):
    return (np.random.RandomState(seed).rand(n, d) < frac).astype(np.float64)


def dense_cases():
    """(id, n, d, k, mask factory, environment, expected routes, flags name)"""
    n, d = 203, 141
    out = []
    for frac in (0.05, 0.11, 0.13, 0.5):
        sparse_mask = frac <= 0.12
        mk = lambda frac=frac: mask01(n, d, frac, int(frac * 100))
        out.append(('density=%.2f-bits' % frac, n, d, 5, mk, {},
                    dict(mask_bits=True, mask_cols=sparse_mask, nw_from_mask=sparse_mask), 'plain'))
        out.append(('density=%.2f-bits-nocols' % frac, n, d, 5, mk, {'RRI_WMCORR_COLS': '0'},
                    dict(mask_bits=True, mask_cols=False, nw_from_mask=False), 'plain'))
        out.append(('density=%.2f-bits-nw-from-pass' % frac, n, d, 5, mk, {'RRI_WNW_MASK': '0'},
                    dict(mask_bits=True, mask_cols=sparse_mask, nw_from_mask=False), 'plain'))
    out.append(('weights-stored', n, d, 5, lambda: np.random.RandomState(3).randint(0, 17, size=(n, d)) / 8.0, {},
                dict(mask_bits=False, mask_cols=False, nw_from_mask=False), 'plain'))
    out.append(('density=0.50-stored-01', n, d, 5, lambda: mask01(n, d, 0.5, 50), {'RRI_MASK_BITS': '0'},
                dict(mask_bits=False, mask_cols=False, nw_from_mask=False), 'plain'))
    for nn in (2048, 2049):
        out.append(('nrb=%d-%s' % (64 + nn - 2048, 'wtrow_small' if nn == 2048 else 'wreduce'), nn, 37, 3,
                    lambda nn=nn: mask01(nn, 37, 0.3, nn), {}, dict(mask_bits=True, wtrow_small=nn == 2048, nrb=64 + nn - 2048),
                    'plain'))

    def with_empty():
        M = mask01(n, d, 0.3, 77)
        M[17, :] = 0
        M[:, 64] = 0
        return M
    out.append(('zero-row-zero-column', n, d, 5, with_empty, {}, dict(mask_bits=True), 'plain'))
    out.append(('mask-of-ones', n, d, 5, lambda: np.ones((n, d)), {}, dict(mask_bits=True, mask_cols=False), 'plain'))
    out.append(('density=0.11-bits-topic', n, d, 5, lambda: mask01(n, d, 0.11, 11), {}, dict(mask_bits=True, mask_cols=True), 'topic'))
    out.append(('density=0.50-bits-topic', n, d, 5, lambda: mask01(n, d, 0.5, 50), {}, dict(mask_bits=True, mask_cols=False), 'topic'))
    out.append(('density=0.11-bits-fix_W', n, d, 5, lambda: mask01(n, d, 0.11, 11), {}, dict(mask_bits=True), 'fix_W'))
    out.append(('density=0.50-bits-fix_W', n, d, 5, lambda: mask01(n, d, 0.5, 50), {}, dict(mask_bits=True), 'fix_W'))
    return out


# the smallest shapes whose read-only pass has npanels >= 2 and more than 1024 workgroups (no interleaved row chunks)
BIG = {'fp64': (36100, 600), 'fp32': (36100, 1030)}


# ---- reference and bound of the stored residual ---------------------------------------------------------------------------
class StepBound(object):
    def __init__(self, Xs, M, store, tables):
        self.X, self.M = Xs, M
        self.u = U32 if store == 'fp32' else U64
        self.tab_u = self.u if (tables and store == 'fp32') else 0.0
        self.B = None

    def resid(self, W, T):
        return self.M * (self.X - W @ T)

    def rebuild(self, W, T):
        self.B = self.u * np.abs(self.resid(W, T))

    def correct(self, a, b, W, T):
        """E <- E - M .* a b^T has been applied and (W, T) are the factors E now belongs to"""
        self.B = self.B + self.u * (np.abs(self.resid(W, T)) + self.B)
        if self.tab_u:
            self.B = self.B + (2 * self.tab_u + self.tab_u ** 2) * self.M * np.outer(np.abs(a), np.abs(b))

    @staticmethod
    def f64(terms, k):
        return C64 * (terms + k + 2) * U64

    def T_sums(self, W, T, t):
        """float64 (wR, nw) of topic t and the bounds of the device's"""
        n, k = W.shape
        w = np.abs(W[:, t])
        E = self.resid(W, T)
        big = self.M * (np.abs(self.X) + np.abs(W) @ np.abs(T))
        nw = (w ** 2) @ self.M
        wR = W[:, t] @ E + T[t] * nw
        terms = (self.M != 0).sum(axis=0)          # entries outside the mask are exact zeros in either sum
        err_nw = (2 * self.tab_u + self.f64(terms, 0)) * nw
        err_a = w @ self.B + self.tab_u * (w @ (np.abs(E) + self.B)) + self.f64(terms, k) * (w @ big)
        return wR, nw, SAFETY * (err_a + np.abs(T[t]) * err_nw), SAFETY * err_nw

    @staticmethod
    def T_row(wR, nw, b_wR, b_nw, reg_l1, reg_l2, s, ub, eps):
        """float64 T row of the step from the sums (wR, nw) and the bound of the row a device takes from sums within (b_wR, b_nw)
        of them (the bounds carry SAFETY already): x = max(wR - reg_l1, 0) / (nw + reg_l2 + eps) [clipped at ub], |dx| <= (|d wR| +
        x |d nw|) / (den + eps) -- an entry whose nw is tiny has a bound as large as it deserves; with the sum constraint
        y = s x / sum(x), |dy_j| <= s (|dx_j| + x_j sum|dx| / sum(x)) / sum(x).  Returns (row, bound, sum(x) before the scaling)."""
        num, den = wR - reg_l1, nw + reg_l2
        ok = den > 0
        x = np.where(ok, np.maximum(num, 0) / np.where(ok, den + eps, 1.0), 0.0)
        if ub is not None:
            x = np.minimum(x, ub)
        dx = np.where(ok, (b_wR + x * b_nw) / np.where(ok, den + eps, 1.0), 0.0)
        nx = float(x.sum())
        if s is not None:
            return s * x / nx, s * (dx + x * dx.sum() / nx) / nx, nx
        return x, dx, nx

    def W_column(self, W, T, t, reg_l1, reg_l2, ub, eps):
        """float64 W[:, t] of the W half from (W, T) and the bound of the device's: x = max(num, 0) / (den + eps) [clipped at ub]
        with num = E t + w nt - reg_l1, den = nt + reg_l2; |dx| <= (|d num| + x |d den|) / (den + eps), the clips are 1-Lipschitz"""
        n, k = W.shape
        d = T.shape[1]
        tr = np.abs(T[t])
        E = self.resid(W, T)
        big = self.M * (np.abs(self.X) + np.abs(W) @ np.abs(T))
        nt = self.M @ (tr ** 2)
        num = E @ T[t] + W[:, t] * nt - reg_l1
        den = nt + reg_l2
        x = np.where(den > 0, np.maximum(num, 0) / (den + eps), 0.0)
        if ub is not None:
            x = np.minimum(x, ub)
        terms = (self.M != 0).sum(axis=1)
        err_nt = (2 * self.tab_u + self.f64(terms, 0)) * nt
        err_num = (self.B @ tr + self.tab_u * ((np.abs(E) + self.B) @ tr) + self.f64(terms, k) * (big @ tr)
                   + np.abs(W[:, t]) * err_nt)
        return x, SAFETY * (err_num + x * err_nt) / np.where(den > 0, den + eps, 1.0)


def pattern_problem(A, store):
    """(X as stored in float64, M = the pattern with explicit zeros counted) of the scipy CSR matrix A"""
    Xs = np.asarray(A.toarray().astype(STORES[store]), dtype=np.float64)
    M = np.zeros(A.shape)
    M[np.repeat(np.arange(A.shape[0]), np.diff(A.indptr)), A.indices] = 1.0
    return Xs, M


def planted(A, k, seed=0):
    """the pattern of A with X = W* T* + noise on it (explicit zeros stay zeros) and a start within 5 % of (W*, T*) -- 1 % at
    large k: every topic stays alive through the sweeps, without resets, and the residual is not all cancellation"""
    rs = np.random.RandomState(seed + 1)
    n, d = A.shape
    Ws, Ts = 0.1 + rs.rand(n, k), 0.1 + rs.rand(k, d)
    rows = np.repeat(np.arange(n), np.diff(A.indptr))
    vals = np.einsum('ij,ji->i', Ws[rows], Ts[:, A.indices]) + 0.01 * rs.rand(A.nnz)
    B = A.copy()
    B.data = np.where(A.data == 0, 0.0, vals)
    off = 0.05 if k <= 8 else 0.01
    return B, Ws * (1 + off * rs.rand(n, k)), Ts * (1 + off * rs.rand(k, d))


def planted_dense(n, d, k, M, seed=0):
    rs = np.random.RandomState(seed + 5)
    Ws, Ts = 0.1 + rs.rand(n, k), 0.1 + rs.rand(k, d)
    X = (Ws @ Ts + 0.01 * rs.rand(n, d)) * (M > 0)
    return X, Ws * (1 + 0.05 * rs.rand(n, k)), Ts * (1 + 0.05 * rs.rand(k, d))


def emulate(Xs, M, W, T, store, tables, flags=None, sweeps=2, skip=None):
    """The stored residual in numpy, no device: E = M .* (Xs - W T) kept in the storage type through `sweeps` sweeps of float64
    topic steps (closed forms on the float64 sums, so the factors are the reference's), every correction applied as the device
    applies it (factors through tables of the storage type when `tables`, one stored rounding per correction).  flags: the
    set_params options that shape a step (t_row_sum, project_T_each_iter, w_row_sum, fix_W, reg_*).  Yields a dict before every
    topic step (the emulated E, the table-rounded w, the float64 sums and their bounds) and fills in the T row and W column of
    the step, their emulated counterparts and their bounds afterwards.  skip = (sweep, t, i, j): that entry misses that T-row
    correction."""
    flags = flags or {}
    dt = STORES[store]
    k = W.shape[1]
    regs = [flags.get(r, 0.0) for r in ('reg_w_l1', 'reg_w_l2', 'reg_t_l1', 'reg_t_l2')]
    no_regs = sum(abs(r) for r in regs) == 0
    fix_W = bool(flags.get('fix_W'))
    s_T = flags.get('t_row_sum') if flags.get('project_T_each_iter') else None
    sb = StepBound(Xs, M, store, tables)
    tab = (lambda v: v.astype(np.float32).astype(np.float64)) if (tables and store == 'fp32') else (lambda v: v)
    E = None
    eps = float(np.spacing(10))
    for sweep in range(sweeps):
        for t in range(k):
            if t == 0:
                sb.rebuild(W, T)
                E = sb.resid(W, T).astype(dt)
            wR_ref, nw_ref, b_wR, b_nw = sb.T_sums(W, T, t)
            Ef = E.astype(np.float64)
            step = dict(sweep=sweep, t=t, E=Ef, w=tab(W[:, t]), trow=T[t], M=M, wR=wR_ref, nw=nw_ref, b_wR=b_wR, b_nw=b_nw)
            yield step
            told = T[t].copy()
            T = T.copy()
            T[t], bT, nx = sb.T_row(wR_ref, nw_ref, b_wR, b_nw, regs[2], regs[3], s_T, flags.get('t_row_sum'), eps)
            nw_emu = (step['w'] ** 2) @ M
            step.update(trow_new=T[t], b_trow=bT, trow_emu=sb.T_row(step['w'] @ Ef + told * nw_emu, nw_emu, b_wR, b_nw, regs[2], regs[3],
                                                                   s_T, flags.get('t_row_sum'), eps)[0])
            scale = nx if (fix_W and no_regs) else 1.0
            wold = W[:, t].copy()
            dtv = scale * T[t] - told
            dE = np.outer(tab(wold), tab(dtv)) * M
            if skip is not None and skip[:2] == (sweep, t):
                dE[skip[2], skip[3]] = 0.0
            step['dt'] = dtv
            E = (E.astype(np.float64) - dE).astype(dt)
            W = W.copy()
            W[:, t] = scale * wold
            sb.correct(wold, dtv, W, T)
            if fix_W:
                continue
            x, bx = sb.W_column(W, T, t, regs[0], regs[1], flags.get('w_row_sum'), eps)
            nt = M @ (tab(T[t]) ** 2)                 # the W column as the device takes it, from the emulated E
            num = E.astype(np.float64) @ tab(T[t]) + wold * nt - regs[0]
            x_emu = np.where(nt + regs[1] > 0, np.maximum(num, 0) / (nt + regs[1] + eps), 0.0)
            if flags.get('w_row_sum') is not None:
                x_emu = np.minimum(x_emu, flags['w_row_sum'])
            step.update(x=x, bx=bx, x_emu=x_emu)
            W = W.copy()
            W[:, t] = x
            E = (E.astype(np.float64) - np.outer(tab(x - wold), tab(T[t])) * M).astype(dt)
            sb.correct(x - wold, T[t], W, T)


def bucket_claims(name, L, store, csrx):
    """asserts that the layout L (sp_layout, or what a handle reported) is the bucket the case id `name` is named for"""
    c = L[0 if name.endswith('-csr') else 1]
    head = name.rsplit('-', 1)[0]
    lps_of = lambda avg: 64 if avg >= 768 else 32 if avg >= 384 else 16 if avg >= 192 else 8
    if head.startswith('lps='):
        assert c['lps'] == int(head[4:]), (name, c['lps'], c['avg'])
    elif head.startswith('avg='):
        assert c['avg'] == int(head[4:]) and c['lps'] == lps_of(c['avg']), (name, c['avg'], c['lps'])
    elif head.startswith('seglen-'):
        lengths = set(int(v) for v in head.split('-')[1:])
        assert lengths <= set(c['seg_len'].ravel().tolist()), (name, sorted(set(c['seg_len'].ravel().tolist())))
        assert {4 * c['lps'] * 8 - 1, 4 * c['lps'] * 8, 4 * c['lps'] * 8 + 1} <= lengths, (name, c['lps'])
    elif head.startswith('bw='):
        cap = sp_block_cap(store, csrx)
        want = {'bw=cap': 1, 'bw=cap+1': 2, 'bw=2cap+1': 3}[head]
        assert c['nblk'] == want and c['bw'] <= cap, (name, c['nblk'], c['bw'])
        if want == 1:
            assert c['bw'] == cap == c['gdim']
        else:
            assert 0 < c['gdim'] - (want - 1) * c['bw'] < c['bw'], 'the last block is the narrower one'
    elif head.startswith('items-'):
        per_block = np.bincount([w[0] for w in c['work']], minlength=c['nblk'])
        assert per_block.max() >= 2 and per_block.min() == 1, (name, per_block)
        inner = [w for i, w in enumerate(c['work']) if i > 0 and c['work'][i - 1][0] == w[0]]
        assert any(c['seg_len'][b, s0] == 0 for b, s0, _ in inner), 'no item boundary on an empty segment'
    elif head.startswith('empty-zeros-heavy'):
        for cp in L:
            assert (cp['seg_len'].sum(axis=0) == 0).any(), 'no segment without entries'
        col = L[1 if name.endswith('-csr') else 0]['seg_len'].sum(axis=0)
        assert col.max() >= col.sum() / 3.0 - 1, (name, col.max(), col.sum())
