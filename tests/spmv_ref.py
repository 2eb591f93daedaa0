"""Plain numpy reference of the compressed SpMV's world (spmv.hip k_spmv7c / k_spmv7, the
dynamics defect k_spmv_dyn, active_set.hip's active list and tile descriptors), restated from
the oracle's CSR alone.  No GPU, nothing shared with the kernels.

Orders.  The reference order of a cell is (k m + j) n + i, row 6 cell + unknown.  One rank owns
the cells in the order lc = (j l + k) n + i (a "grid row" is one (j, k), n cells along i); the
ext layout puts HALO = 2 latitude rows before and after them, and a component-planar vector
holds unknown v of ext cell e at e + v ps, ps = n l (m + 4).

Grids (grid(n, periodic)): natl8's physics (SRES = 0, so the integral-condition row exists) on
n x 14 x 3 cells with a land mask made for the tiles of 64 cells along i: whole and partial
tiles, tiles whose only active lane is the first or the last, runs that start late or end
early in a tile (the staging pieces the kernel skips), holes, empty tiles.

Error bounds.  A sum of p products computed in floating point, in any order, with or without
fused multiply-adds, differs from the exact sum by at most gamma_p sum |a_i x_i|, gamma_p =
p u / (1 - p u) <= (p + 1) u, u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms,
2nd ed., section 3.1).  Terms whose coefficient is zero contribute nothing and round nothing, so
p counts the non-zero coefficients of the row.  The defect rr - sum adds one more rounding:
(p + 2) u (|rr| + sum |a_i z_i|).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from helpers import mask_fix
from iemic import config as cf
from krylov_ref import csr_operator

NUN, HALO, TILE = 6, 2, 64
M, L = 14, 3
U53 = 2.0 ** -53
GRIDS = ((130, True), (130, False), (65, True), (64, True), (63, False))
# one more, beside the five of the design: active runs that end or start exactly at the lanes
# where a staging piece begins to be skipped (see classify: last lane 19, first lane 23 / 44; 23
# and 40 together), at the lanes whose own 48 bytes straddle two pieces (21 and 42, as the last
# and as the first lane), and one lane inside those (22, 41)
EDGES = (64, False, "edges")
ALL_GRIDS = GRIDS + (EDGES,)
EDGE_SPANS = ((0, 19), (0, 21), (21, 42), (23, 40), (42, 63), (44, 63), (22, 41))
SEED2 = 99                          # the second state's seed (another Jacobian, same mask)


def grid_id(g):
    return f"n{g[0]}{'p' if g[1] else ''}{g[2] if len(g) > 2 else ''}"


# ---- the grids ---------------------------------------------------------------------------
def wet_columns(n, design=None):
    """{j: wet i} of the design, the same on every layer; spans clipped to the grid"""
    def span(a, b):
        return set(range(max(a, 0), min(b, n - 1) + 1))
    rows = {}
    if design == "edges":                     # one span per pair of rows, no land rows between
        for q, (a, b) in enumerate(EDGE_SPANS):
            rows[2 * q] = rows[2 * q + 1] = span(a, b)
        return rows
    for j in (0, 1):
        rows[j] = span(0, n - 1)
    for j in (3, 4):
        rows[j] = span(0, 1) | span(n - 2, n - 1)
    for j in (6, 7):
        rows[j] = span(63, 64)
    for j in (9, 10):
        rows[j] = span(10, 12) | span(30, 40) | span(100, 101)
    for j in (12, 13):
        rows[j] = span(50, 70)
    return rows


def config(n, periodic):
    return dataclasses.replace(cf.preset("natl8", mixing=0), name=f"tiles{n}", n=n, m=M, l=L,
                               periodic=periodic)


def landmask(n, periodic, design=None):
    """the mask handed to the device and (after mask_fix) to the oracle: (l + 2, m + 2, n + 2);
    layer index 1 is the bottom one (config._fix_inversions), turned to land under the shelf"""
    Lm = np.full((L + 2, M + 2, n + 2), cf.LAND, dtype=np.int32)
    for j, cols in wet_columns(n, design).items():
        for i in cols:
            Lm[1:L + 1, j + 1, i + 1] = cf.OCEAN
    for j in (9, 10) if design is None else ():
        Lm[1, j + 1, 1:min(35, n) + 1] = cf.LAND
    if periodic:
        cf._perio_borders(Lm)
    return Lm


_GRID = {}


def grid(orc, n, periodic, design=None):
    """the grid's configuration, masks, oracle, the two states and their Jacobians (computed
    once and shared; the arrays are read-only)"""
    key = (n, bool(periodic), design)
    if key not in _GRID:
        c = config(n, periodic)
        L0 = landmask(n, periodic, design)
        Lf = mask_fix(orc, c, L0)
        o = orc.Oracle(c.ref_dict(), Lf, c.par_list())
        x1 = cf.synthetic_state(c, Lf, amp_ts=1e-3)
        x2 = cf.synthetic_state(c, Lf, seed=SEED2, amp_ts=1e-3)
        ov1, _ = o.jacobian(x1)
        ov2, _ = o.jacobian(x2)
        for a in (L0, Lf, x1, x2, ov1, ov2):
            a.setflags(write=False)
        _GRID[key] = dict(c=c, n=n, periodic=bool(periodic), L0=L0, L=Lf, o=o, x=(x1, x2), ov=(ov1, ov2),
                          fixed=int(np.count_nonzero(L0[1:-1, 1:-1, 1:-1] != Lf[1:-1, 1:-1, 1:-1])))
    return _GRID[key]


# ---- orders ------------------------------------------------------------------------------
def owned_to_ref(n):
    """reference cell of every owned cell lc = (j l + k) n + i"""
    lc = np.arange(n * M * L)
    i, k, j = lc % n, (lc // n) % L, lc // (n * L)
    return (k * M + j) * n + i


def to_planar(n, v_ref, halo_fill):
    """reference-order vector -> component-planar ext vector (6 ps doubles); the halo rows take
    halo_fill (an array of 6 ps doubles, or a scalar)"""
    ps = n * L * (M + 2 * HALO)
    out = np.empty(NUN * ps)
    out[:] = halo_fill
    P = out.reshape(NUN, ps)
    V = np.asarray(v_ref).reshape(-1, NUN)[owned_to_ref(n)]          # owned order
    P[:, HALO * L * n: HALO * L * n + n * M * L] = V.T
    return out


def from_planar(n, p):
    """owned cells of a component-planar ext vector -> (owned cell, unknown)"""
    ps = n * L * (M + 2 * HALO)
    P = np.asarray(p).reshape(NUN, ps)
    return P[:, HALO * L * n: HALO * L * n + n * M * L].T


# ---- identity rows, active cells, tiles --------------------------------------------------
def identity_rows(o, ov):
    """the block GS's rule: a single non-zero, 1 on the diagonal; never the integral condition"""
    rows = np.repeat(np.arange(o.N), np.diff(o.rowptr))
    diag = o.col == rows
    off = np.add.reduceat(((ov != 0) & ~diag).astype(np.int64), o.rowptr[:-1])
    d = np.add.reduceat(np.where(diag, ov, 0.0), o.rowptr[:-1])
    kn = (off == 0) & (d == 1.0)
    if o.rowintcon >= 0:
        kn[o.rowintcon] = False
    return kn


@dataclasses.dataclass
class Tiles:
    active: np.ndarray          # per owned cell
    act: np.ndarray             # the active list (owned cells, ascending)
    ric: int                    # compressed row of the integral condition, -1
    atl: np.ndarray             # (natile, 8) int32 records, as ActiveSet::atl
    klass: dict                 # class -> count over every (grid row, tile), empty ones included


def tiles(n, kn, rowintcon):
    """active flags, list and the tile records (tile, lo | hi << 8, a0, na, mask low, mask high,
    0, 0) from the identity-row flags kn (reference order)"""
    active = (~kn.reshape(-1, NUN)).any(axis=1)[owned_to_ref(n)]
    act = np.flatnonzero(active)
    cmap = np.cumsum(active) - 1
    tpr = -(-n // TILE)
    pad = np.zeros((M * L, tpr * TILE), dtype=bool)
    pad[:, :n] = active.reshape(M * L, n)
    lanes = pad.reshape(M * L, tpr, TILE)
    first = cmap.reshape(M * L, n)
    recs = []
    kl = dict.fromkeys(CLASSES, 0)
    for row in range(M * L):
        for ti in range(tpr):
            b = lanes[row, ti]
            nc = min(TILE, n - ti * TILE)
            on = np.flatnonzero(b)
            for name in classify(b, nc):
                kl[name] += 1
            if on.size == 0:
                continue
            lo, hi = int(on[0]), int(on[-1])
            mask = int(sum(1 << int(q) for q in on))
            a0 = int(first[row, ti * TILE + lo])
            recs.append((row * tpr + ti, lo | (hi << 8), a0, on.size, _i32(mask), _i32(mask >> 32), 0, 0))
    ric = -1
    if rowintcon >= 0:
        cell = rowintcon // NUN
        lc = int(np.flatnonzero(owned_to_ref(n) == cell)[0])
        if active[lc]:
            ric = NUN * int(cmap[lc]) + rowintcon % NUN
    return Tiles(active, act.astype(np.int32), ric, np.array(recs, dtype=np.int32).reshape(-1, 8), kl)


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


CLASSES = ("full", "partial", "lane0", "lane63", "end<=19", "start23-43", "start>=44", "holes", "empty")


def classify(b, nc):
    """the classes of one tile from its 64 active-lane flags b and its cell count nc.  The
    kernel stages each neighbour row in three pieces of 1 KiB (21 1/3 cells of 48 bytes) and
    skips piece h when it ends at or before (lo - 1) 48 bytes or starts at or after (hi + 2) 48
    bytes: pieces 1 and 2 for hi <= 19, piece 0 for lo >= 23, pieces 0 and 1 for lo >= 44."""
    on = np.flatnonzero(b)
    if on.size == 0:
        return ["empty"]
    lo, hi = int(on[0]), int(on[-1])
    out = []
    if on.size == TILE:
        out.append("full")
    if nc < TILE:
        out.append("partial")
    if on.size == 1 and lo == 0:
        out.append("lane0")
    if on.size == 1 and lo == TILE - 1:
        out.append("lane63")
    if hi <= 19:
        out.append("end<=19")
    if 23 <= lo < 44:
        out.append("start23-43")
    if lo >= 44:
        out.append("start>=44")
    if on.size < hi - lo + 1:
        out.append("holes")
    return out


# ---- y = J x and its bound ---------------------------------------------------------------
@dataclasses.dataclass
class Product:
    y: np.ndarray               # J x in longdouble
    bound: np.ndarray           # per row: the largest |error| a correct float64 kernel can have
    mag: np.ndarray             # sum |a_ij| |x_j|


def product(o, ov, x, extra=None):
    """y = J x in longdouble and the per-row bound (p + 1) u sum |a x|, p the row's non-zero
    coefficients; extra (per row, |rr| of the defect): (p + 2) u (extra + sum |a x|)"""
    y = csr_operator(o.rowptr, o.col, ov, np.longdouble)(x)
    mag = csr_operator(o.rowptr, o.col, np.abs(ov), np.longdouble)(np.abs(x)).astype(np.float64)
    p = np.add.reduceat((ov != 0).astype(np.int64), o.rowptr[:-1])
    if extra is None:
        return Product(y, (p + 1) * U53 * mag, mag)
    return Product(y, (p + 2) * U53 * (np.abs(extra) + mag), mag)


def ratio(got, ref, bound):
    """|got - ref| / bound per row in float64; a row with bound 0 (no non-zero term) must be
    exact: 0 then, inf otherwise; a NaN in got gives inf"""
    err = np.abs(np.asarray(got).astype(np.longdouble) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def defect_expected(n, o, ov, kn, act, z_ref, rr_ref):
    """the dynamics defect on the active cells' U/V/W/P rows: (expected (nact, 4) longdouble, 0
    on identity rows; bound (nact, 4), 0 on identity rows: they must be exactly 0)"""
    pr = product(o, ov, z_ref, extra=rr_ref)
    cells = owned_to_ref(n)[act]
    rows = (NUN * cells)[:, None] + np.arange(4)[None, :]
    ident = kn[rows]
    exp = np.where(ident, np.longdouble(0), np.asarray(rr_ref, dtype=np.longdouble)[rows] - pr.y[rows])
    return exp, np.where(ident, 0.0, pr.bound[rows])
