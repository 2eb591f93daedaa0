"""NumPy twin of the projected theta model (ProjectedThetaModel.H, StochasticProjectedThetaModel.H),
for tests/test_projected.py (CPU) and tests/test_gpu_projected.py.

Built only from oracle.py's F, CSR J and B with dense NumPy: it never uses the device's exports.
The Gram products are exactly rounded (``math.fsum`` over the products), so a bound on the
device's summation error needs no allowance for the twin's own.  ``gram`` also returns the sum of
the absolute products, the scale of that bound.
"""
import math

import numpy as np

from helpers import mask_fix
from iemic import config as cf
from iemic.config import PAR_INDEX
from stoch_ref import forcing_column, noise

EPS = 2.0 ** -52


def gram(V, W, d=None, exact=True):
    """(G, A): G[a, b] = fsum_i V[i, a] d[i] W[i, b] with (V d) rounded first, as the device forms
    it, and A[a, b] = sum_i |V[i, a] d[i] W[i, b]|; exact=False: G by a plain matrix product"""
    V = np.asarray(V, dtype=np.float64).reshape(len(V), -1)
    W = np.asarray(W, dtype=np.float64).reshape(len(W), -1)
    Vd = V if d is None else V * np.asarray(d, dtype=np.float64)[:, None]
    if not exact:
        return Vd.T @ W, None
    G = np.zeros((V.shape[1], W.shape[1]))
    for a in range(V.shape[1]):
        for b in range(W.shape[1]):
            G[a, b] = math.fsum(Vd[:, a] * W[:, b])
    return G, np.abs(Vd).T @ np.abs(W)


def csr_rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def csr_mm(rowptr, col, val, V):
    rows = csr_rows(rowptr)
    return np.stack([np.bincount(rows, weights=val * V[col, b], minlength=len(rowptr) - 1)
                     for b in range(V.shape[1])], axis=1)


class ProjectedTwin:
    """The projected steppers' model surface on the CPU oracle.  L: the land mask to use (the
    device's own, (l+2, m+2, n+2)); default: the configuration's, fixed up as the device does.
    exact=False: plain matrix products in place of the exactly rounded ones (a large k)."""

    def __init__(self, orc, cfg, L=None, exact=True):
        self.exact = exact
        if L is None:
            L = mask_fix(orc, cfg, cf.landmask(cfg).reshape(cfg.l + 2, cfg.m + 2, cfg.n + 2))
        self.cfg, self.L = cfg, L
        self.o = orc.Oracle(cfg.ref_dict(), L, cfg.par_list())
        o = self.o
        self.x = np.zeros(o.N)
        self.rows = csr_rows(o.rowptr)
        self.diag = np.flatnonzero(o.col == self.rows)
        self.G = None
        self.inits = 0

    # the stepper's surface -----------------------------------------------------------
    def preProcess(self):
        pass

    def setState(self, x):
        self.x = np.array(x, dtype=np.float64)

    def getState(self):
        return self.x.copy()

    def projSetBasis(self, V):
        self.V = np.array(V, dtype=np.float64)
        self.k = self.V.shape[1]
        self.y = self.projRestrictState()

    def projRestrictState(self):
        return gram(self.V, self.x, exact=self.exact)[0][:, 0]

    def projSetState(self, y):
        self.y = np.array(y, dtype=np.float64)
        self.x = self.V @ self.y

    def projInitStep(self, dt, theta):
        o = self.o
        self.dt, self.theta = dt, theta
        self.G = None
        self.inits += 1
        self.xn = self.x.copy()
        self.yn = self.projRestrictState()
        self.Fn = gram(self.V, o.rhs(self.x), exact=self.exact)[0][:, 0]
        val, B = o.jacobian(self.x)
        self.B = B
        self.VMV = gram(self.V, self.V, B, exact=self.exact)[0]
        val = val.copy()
        val[self.diag] += np.where(B != 0, -(B / dt) / theta, 0.0)
        self.val2 = val
        self.W = csr_mm(o.rowptr, o.col, val, self.V)
        self.VAV = gram(self.V, self.W, exact=self.exact)[0]

    def projStochasticInitStep(self, dt, theta, sigma, pert):
        self.projInitStep(dt, theta)
        if sigma == 0.0:
            return
        c = self.cfg
        par = {name: self.o.get_par(idx) for name, idx in PAR_INDEX.items()}
        top = self.L[c.l, 1:c.m + 1, 1:c.n + 1]
        field, _ = noise(c, forcing_column(c, top, par), top, self.o.rowintcon, dt, sigma, pert)
        self.noise_field = field
        self.G = gram(self.V, field, exact=self.exact)[0][:, 0]

    def projRHS(self):
        dt, th = self.dt, self.theta
        f = gram(self.V, self.o.rhs(self.x), exact=self.exact)[0][:, 0]
        r = (dt * (1 - th)) * self.Fn + (dt * th) * f + self.VMV @ (self.yn - self.y)
        return r if self.G is None else r + self.G

    def projSolve(self, r):
        return np.linalg.solve(self.VAV, np.asarray(r) / self.dt / self.theta)

    def projNewtonStep(self):
        from types import SimpleNamespace
        dy = self.projSolve(self.projRHS())
        self.projSetState(self.y - dy)
        return SimpleNamespace(norm_dx=float(np.max(np.abs(dy))), norm_f1=float(np.linalg.norm(self.projRHS())))

    def projRestore(self):
        self.x = self.xn.copy()

    def projGet(self, what):
        return {"y": self.y, "y_n": self.yn, "F_n": self.Fn, "VMV": self.VMV, "VAV": self.VAV,
                "G": np.zeros(self.k) if self.G is None else self.G}[what].copy()
