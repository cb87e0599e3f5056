"""Frozen rows: the float64 numpy restatement of a sweep of the stacked problem [X_O; X_H] in which the rows W_O are never
updated (nmf.py:415-476 through the oracle's own pieces), the same sweep from the statistics of the frozen rows, and the
generators of the cases that tests/test_frozen_cpu.py and tests/test_frozen_gpu.py share."""
import numpy as np

from oracle import rri_oracle as orc

FLAVOURS = {
    'plain': dict(),
    'tm': dict(project_T_each_iter=True, t_row_sum=1.0, w_row_sum=1.0),
    'pen': dict(reg_w_l1=0.02, reg_w_l2=0.3, reg_t_l1=0.01, reg_t_l2=0.2),
}


def relfro(a, b):
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b))) / (nb if nb > 0 else 1.0)


class Stacked(object):
    """The stacked problem: Xo, Wo frozen, Xh, Wh, T live.  sweep() runs the reference's topic loop with the rows Wo left
    alone -- the T row of topic t from ALL rows, its column of W on the rows H only, the column check on the whole column --
    and counts the resets it met (max_resid_document among the rows H; W[:, t] = 0 reaches Wo)."""

    def __init__(self, Xo, Wo, Xh, Wh, T, reset_topic_method=None, n_resets=0, **flags):
        self.Xo, self.Xh = np.array(Xo, dtype=np.float64), np.array(Xh, dtype=np.float64)
        self.Wo, self.Wh, self.T = np.array(Wo, dtype=np.float64), np.array(Wh, dtype=np.float64), np.array(T, dtype=np.float64)
        self.flags = dict(project_T_each_iter=False, t_row_sum=None, w_row_sum=None, reg_w_l1=0, reg_w_l2=0, reg_t_l1=0, reg_t_l2=0)
        self.flags.update(flags)
        self.method, self.left, self.resets = reset_topic_method, n_resets, 0

    def _reset(self, t):
        Rp = np.maximum(self.Xh - self.Wh.dot(self.T), 0)
        mi = int(np.argmax((Rp ** 2).sum(1)))
        self.T[t, :] = Rp[mi, :]
        self.Wh[:, t] = 0
        self.Wh[mi, t] = 1.0
        self.Wo[:, t] = 0
        self.left -= 1
        self.resets += 1

    def sweep(self, n_sweeps=1):
        f = self.flags
        k = self.T.shape[0]
        X = np.vstack([self.Xo, self.Xh])
        no_regs = abs(f['reg_w_l1']) + abs(f['reg_w_l2']) + abs(f['reg_t_l1']) + abs(f['reg_t_l2']) == 0
        for _ in range(n_sweeps):
            for t in range(k):
                W = np.vstack([self.Wo, self.Wh])
                wR, nw = orc.residual_products_T(X, W, self.T, t, None)
                s = f['t_row_sum'] if f['project_T_each_iter'] else None
                self.T[t, :], nt1 = orc.qf_min(-(wR - f['reg_t_l1']), nw + f['reg_t_l2'], s=s, ub=f['t_row_sum'])
                if no_regs:
                    self.Wh[:, t] = self.Wh[:, t] * nt1
                if np.sum(self.T[t, :]) > 1e-10 or self.method is None:
                    if f['t_row_sum'] and f['project_T_each_iter'] and np.abs(np.sum(self.T[t, :]) - f['t_row_sum']) > 1e-15:
                        self.T[t, :] = orc.proj_simplex(self.T[t, :], s=f['t_row_sum'])
                elif self.left > 0:
                    self._reset(t)
                Rt, nt = orc.residual_products_W(self.Xh, self.Wh, self.T, t, None)
                self.Wh[:, t], _ = orc.qf_min(-(Rt - f['reg_w_l1']), nt + f['reg_w_l2'], s=None, ub=f['w_row_sum'])
                total = np.sum(self.Wh[:, t]) + np.sum(self.Wo[:, t])
                if not (total > 1e-10 or self.method is None) and self.left > 0:
                    self._reset(t)
                    total = np.sum(self.Wh[:, t]) + np.sum(self.Wo[:, t])
                assert total > 0, 'W[:, t] sums to 0'
        return self.Wh, self.T

    def stats(self):
        return stats_of(self.Xo, self.Wo)

    def objective(self):
        X, W = np.vstack([self.Xo, self.Xh]), np.vstack([self.Wo, self.Wh])
        return 0.5 * float(((X - W.dot(self.T)) ** 2).sum())


def stats_of(X, W):
    """(B, A, s, c) of the rows X with the factors W"""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    return W.T.dot(X), W.T.dot(W), W.sum(0), float((X ** 2).sum())


def frozen_sweep(B, A, s, Xh, Wh, T, n_sweeps=1, **flags):
    """the same sweep from the statistics alone (the form of rri_frozen.hpp), for inputs that meet no reset"""
    f = dict(project_T_each_iter=False, t_row_sum=None, w_row_sum=None, reg_w_l1=0, reg_w_l2=0, reg_t_l1=0, reg_t_l2=0)
    f.update(flags)
    Wh, T = np.array(Wh, dtype=np.float64), np.array(T, dtype=np.float64)
    no_regs = abs(f['reg_w_l1']) + abs(f['reg_w_l2']) + abs(f['reg_t_l1']) + abs(f['reg_t_l2']) == 0
    for _ in range(n_sweeps):
        for t in range(T.shape[0]):
            w = Wh[:, t]
            g = w.dot(Wh) + A[t]
            nw = g[t]
            g[t] = 0.0
            wR = w.dot(Xh) + B[t] - g.dot(T)
            sproj = f['t_row_sum'] if f['project_T_each_iter'] else None
            T[t, :], nt1 = orc.qf_min(-(wR - f['reg_t_l1']), nw + f['reg_t_l2'], s=sproj, ub=f['t_row_sum'])
            if no_regs:
                Wh[:, t] = Wh[:, t] * nt1
            assert np.sum(T[t, :]) > 1e-10
            if f['t_row_sum'] and f['project_T_each_iter'] and np.abs(np.sum(T[t, :]) - f['t_row_sum']) > 1e-15:
                T[t, :] = orc.proj_simplex(T[t, :], s=f['t_row_sum'])
            Rt, nt = orc.residual_products_W(Xh, Wh, T, t, None)
            Wh[:, t], _ = orc.qf_min(-(Rt - f['reg_w_l1']), nt + f['reg_w_l2'], s=None, ub=f['w_row_sum'])
            assert np.sum(Wh[:, t]) + s[t] > 1e-10
    return Wh, T


def planted_factors(n, d, k, seed, density=0.4):
    """non-negative factors of a planted rank-k matrix: every topic holds a share of the rows and of the columns"""
    rs = np.random.RandomState(seed)
    dens = min(density, 3.0 / k)       # large k: topics that overlap little, so that none is explained away by the others
    Wp = (0.2 + rs.rand(n, k)) * (rs.rand(n, k) < dens)
    Tp = (0.2 + rs.rand(k, d)) * (rs.rand(k, d) < dens)
    Wp[np.arange(n), np.arange(n) % k] += 0.5      # no topic without rows, no row without a topic
    Tp[np.arange(d) % k, np.arange(d)] += 0.5
    return Wp, Tp


def planted(n, d, k, seed, density=0.4):
    """a non-negative matrix of planted rank k with a little noise, entries of order one"""
    Wp, Tp = planted_factors(n, d, k, seed, density)
    return Wp.dot(Tp) + 0.01 * np.random.RandomState(seed + 7).rand(n, d)


def make_case(n_o, n_h, d, k, seed, flavour='plain', integer=False):
    """Xo (n_o x d), Wo, Xh (n_h x d), Wh, T and the flags of `flavour`.  X has planted rank k and the starting factors are the
    planted ones disturbed by a fifth, so that every topic stays alive through the sweeps (no reset); integer: X rounded to
    small counts (exact in float32, and a CSR-resident X keeps their zeros out of its pattern)"""
    rs = np.random.RandomState(1000 + seed)
    Wp, Tp = planted_factors(n_o + n_h, d, k, seed)
    X = Wp.dot(Tp) + 0.01 * rs.rand(n_o + n_h, d)
    if integer:
        X = np.floor(2.0 * X / X.mean() + 0.5)
        X[:, 0] += 1.0          # no empty row
    W = Wp * (0.8 + 0.4 * rs.rand(*Wp.shape)) + 0.02 * rs.rand(*Wp.shape)
    T = Tp * (0.8 + 0.4 * rs.rand(*Tp.shape)) + 0.02 * rs.rand(*Tp.shape)
    flags = dict(FLAVOURS[flavour])
    if flags.get('t_row_sum'):
        T /= T.sum(1, keepdims=True)
    return X[:n_o], W[:n_o].copy(), X[n_o:], W[n_o:].copy(), T, flags
