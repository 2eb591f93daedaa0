"""NumPy restatement of the stochastic theta model, for tests/test_stochastic.py (CPU) and
tests/test_gpu_stochastic.py.

* ``forcing_column``: the ocean's stochastic forcing operator, i.e. the salinity part of
  ``forcing`` (forcing.F90:106-189) with par(SPER) = 0, which ``stochastic_forcing``
  (forcing.F90:220-265) stores one entry per surface cell.  Evaluated in the reference's order of
  operations with the C library's cos (math.cos: NumPy's vectorised cos may differ in the last
  bit), so the device's column is compared bit for bit.  Ocean-only, idealized profile or an
  inserted emip / adapted_emip; spert is the default field (the constant SRES).
* ``forcing_triple``: the matrix THCM::computeForcing makes of it (THCM.C:836-940).
* ``noise``: G = (sqrt(dt) sigma) (coF pert[j]) on the surface S rows of the ocean cells but the
  integral condition's, as a full vector, and the mask of the rows that carry it.
* ``StochasticTwin``: tests/test_transient.py's TwinModel with ``stochasticInitStep``.
"""
import math

import numpy as np

from iemic.config import PAR_INDEX
from test_transient import TwinModel

SS = 5


def qint(field, cos_y, wet):
    """forcing.F90:536-548 -> THCM.C:2704-2737, the reference's sequential order"""
    lf = ls = 0.0
    m, n = wet.shape
    for j in range(m):
        for i in range(n):
            lf = field[j, i] * cos_y[j] * wet[j, i] + lf
            ls = cos_y[j] * wet[j, i] + ls
    return lf / ls


def forcing_column(c, land_top, par, emip=None, aemip=None):
    """coF[j, i]: Frc(find_row2(i, j, l, SS)) of ``forcing`` with par(SPER) = 0.
    land_top: the top layer of the land mask, (m, n); par: name -> value; emip / aemip: inserted
    n*m fields (setEmip 'E' / 'A'; emip is masked with the ocean cells on insertion)."""
    n, m = c.n, c.m
    if c.coupled_s:
        return np.zeros((m, n))
    ymin, ymax = c.ymin * math.pi / 180.0, c.ymax * math.pi / 180.0
    dy = (ymax - ymin) / m
    y = [(j - 0.5) * dy + ymin for j in range(1, m + 1)]
    cos_y = np.array([math.cos(v) for v in y])
    if c.forcing_type == 2:
        salf = [math.cos(math.pi * (v - ymin) / (ymax - ymin)) for v in y]
    elif c.forcing_type == 1:
        salf = [(math.cos(math.pi * v / ymax) + par["Flux Perturbation"] * v / ymax) / math.cos(v) for v in y]
    else:
        salf = [math.cos(math.pi * v / ymax) + par["Flux Perturbation"] * v / ymax for v in y]
    wet = (1 - np.asarray(land_top).reshape(m, n)).astype(np.float64)
    if emip is None:
        emip = np.array(salf)[:, None] * wet
    else:
        emip = np.asarray(emip, dtype=np.float64).reshape(m, n) * wet
    aem = np.zeros((m, n)) if aemip is None else np.asarray(aemip, dtype=np.float64).reshape(m, n) * wet
    spert = np.full((m, n), float(c.sres))
    salcor = asalcor = spertcor = 0.0
    if c.sres == 0:
        salcor, asalcor, spertcor = qint(emip, cos_y, wet), qint(aem, cos_y, wet), qint(spert, cos_y, wet)
    fac = float(1 - c.sres) + c.sres * par["Nonlinear Factor"]
    gamma = par["Combined Forcing"] * par["Salinity Forcing"] * fac
    hmtp = par["Salinity Homotopy"]
    return (gamma * (1 - hmtp) * (emip - salcor) + gamma * hmtp * (aem - asalcor)
            + 0.0 * fac * (spert - spertcor))


def surface_rows(c):
    """global row of the S unknown of every surface cell, (m, n)"""
    j, i = np.meshgrid(np.arange(c.m), np.arange(c.n), indexing="ij")
    return 6 * (((c.l - 1) * c.m + j) * c.n + i) + SS


def forcing_triple(c, coF, rowintcon):
    """THCM::computeForcing's matrix: (rows, cols, vals) sorted by row, the integral-condition
    row left out (rowintcon < 0: none), land-cell values kept; empty with coupled_S"""
    rows = surface_rows(c).reshape(-1)
    cols = np.repeat(np.arange(c.m), c.n).astype(np.int32)
    keep = (rows != rowintcon) if not c.coupled_s else np.zeros(rows.size, dtype=bool)
    return rows[keep].astype(np.int64), cols[keep], np.asarray(coF, dtype=np.float64).reshape(-1)[keep]


def noise(c, coF, land_top, rowintcon, dt, sigma, pert):
    """(G, hit): the full-length noise vector of a step and the rows that carry it"""
    rows = surface_rows(c)
    hit2 = (np.asarray(land_top).reshape(c.m, c.n) == 0) & (rows != rowintcon)
    g = (np.sqrt(dt) * sigma) * (coF * np.asarray(pert, dtype=np.float64)[:, None])
    G = np.zeros(c.nrows)
    G[rows[hit2]] = g[hit2]
    hit = np.zeros(c.nrows, dtype=bool)
    hit[rows[hit2]] = True
    return G, hit


class StochasticTwin(TwinModel):
    """TwinModel with StochasticThetaModel's initStep and residual (StochasticThetaModel.H:52-83)"""

    def __init__(self, orc, cfg, lin_tol=1e-6):
        super().__init__(orc, cfg, lin_tol)
        self.cfg = cfg
        self.G = None
        self.steps_seen = []                     # (dt, pert) of every stochasticInitStep

    def par(self):
        return {name: self.o.get_par(idx) for name, idx in PAR_INDEX.items()}

    def land_top(self):
        c = self.cfg
        return self.L[c.l, 1:c.m + 1, 1:c.n + 1]

    def thetaInitStep(self, dt, theta):
        self.G = None
        super().thetaInitStep(dt, theta)

    def stochasticInitStep(self, dt, theta, sigma, pert):
        self.thetaInitStep(dt, theta)
        self.steps_seen.append((dt, np.array(pert, dtype=np.float64)))
        if sigma == 0.0:
            return
        coF = forcing_column(self.cfg, self.land_top(), self.par())
        self.G, self.hit = noise(self.cfg, coF, self.land_top(), self.o.rowintcon, dt, sigma, pert)

    def _ftheta(self, B):
        f = super()._ftheta(B)
        if self.G is not None:
            f[self.hit] = f[self.hit] + self.G[self.hit]
        return f
