"""The T/S aggregation multigrid of the block Gauss-Seidel preconditioner (ts_mg.hip,
ts_mg_setup.hip) restated as matrix algebra: every level is one scipy.sparse matrix over its
(variable, cell) unknowns, the transfers are aggregation matrices, the coarse operators the
triple products P^T A P, the smoother a block solve on the water columns of one colour.  No
stencil arrays, no level walk shared with the kernels or with the C twin (oracle/prec_oracle.c);
only numpy and scipy.  The one rule carried over from the twin is the integral-condition row
(level0_operator).

Unknown u of a level with n x m x l cells: u = var ncl + (j n + i) l + k, var 0 (T) / 1 (S),
ncl = n m l -- the halo-free (component, j, i, k) order the test hook copies the device's
levels in.
"""
import numpy as np
import scipy.sparse as sp

NUN, TT, SS = 6, 4, 5
OCEAN = 0


# ---- level structure (the documented one-rank rule of mg_levels) -----------------------------

def cr_ok(n, m, l):
    """a level the whole-problem cyclic reduction takes"""
    return n * m * l <= 1024 and 2 * m * l <= 192 and n >= 2


def level_sizes(n, m, l):
    """[(n_q, m_q)]: coarsen ((n+1)/2, (m+1)/2) while the level has more than 128 cells, stop
    early at the first level q > 0 that cr_ok takes, always at least one coarse level"""
    sizes = [(n, m)]
    while len(sizes) < 12:
        a, b = sizes[-1]
        q = len(sizes) - 1
        if q > 0 and (a * b * l <= 128 or cr_ok(a, b, l)):
            break
        if a == 1 and b == 1:
            break
        sizes.append(((a + 1) // 2, (b + 1) // 2))
    if len(sizes) < 2:
        raise ValueError("no coarse level")
    return sizes


def lanes(l):
    return 16 if l <= 16 else (32 if l <= 32 else 64)


def ncolours(n, periodic):
    return 4 if periodic and n % 2 == 1 else 2


def expected_plan(n, m, l, periodic, sweeps=1):
    """what the device's plan hook must report on one rank: level sizes, colours, the levels
    visited by the fused launches (an intermediate level of two colours, one sweep), the lane
    count and the coarsest level's assembly (0 device inverse, 1 cyclic reduction, 2 host)"""
    sizes = level_sizes(n, m, l)
    nlev = len(sizes)
    cols = [ncolours(a, periodic) for a, _ in sizes]
    fused = [int(0 < q < nlev - 1 and sweeps == 1 and cols[q] == 2) for q in range(nlev)]
    cn, cm = sizes[-1]
    ncl = cn * cm * l
    kind = 1 if (cr_ok(cn, cm, l) and ncl > 128) else (0 if 2 * ncl <= 192 else 2)
    return dict(nlev=nlev, sizes=sizes, colours=cols, fused=fused, lanes=lanes(l), kind=kind,
                sweeps=sweeps, hr=0, par=[0] * nlev)


# ---- helpers on a level's unknowns ------------------------------------------------------------

def _decode(u, n, m, l):
    ncl = n * m * l
    var = u // ncl
    t = u % ncl
    return var, t // (n * l), (t // l) % n, t % l          # var, j, i, k


def _filter(A, keep):
    A = A.tocoo()
    k = keep(A.row, A.col) & (A.data != 0.0)
    return sp.csr_matrix((A.data[k], (A.row[k], A.col[k])), shape=A.shape)


def level0_operator(rowptr, col, val, landm, n, m, l, periodic, rowintcon, int_sign, intc):
    """A0: the T/S block of the Jacobian on the active unknowns.  Known unknowns (land: their
    rows are identity rows) have zero rows and columns.  The integral-condition row (an S row
    whose Jacobian row is the integral over the basin) is replaced by the diagonal entry
    int_sign * intc[row] alone -- the rule of prec_oracle.c mg_build; its column stays.  Only the
    couplings the multigrid keeps: the 2x2 cell block, the same variable at -+i, -+j, -+k, and
    T <-> S at k -+ 1.  Returns (A0, active)."""
    N = NUN * n * m * l
    J = sp.csr_matrix((np.asarray(val, dtype=np.float64), np.asarray(col), np.asarray(rowptr)), shape=(N, N))
    ncl = n * m * l
    u = np.arange(2 * ncl)
    var, j, i, k = _decode(u, n, m, l)
    rows = NUN * ((k * m + j) * n + i) + TT + var
    A = J[rows][:, rows].tocsr()
    ocean = np.asarray(landm)[1:-1, 1:-1, 1:-1] == OCEAN             # (l, m, n)
    active = ocean[k, j, i]
    # the identity rows of the Jacobian say the same (the integral condition's row is no such row)
    Jl = J.tolil()
    for uu in np.nonzero(~active)[0][:64]:
        r = rows[uu]
        assert Jl.rows[r] == [r] or all(Jl[r, c] == 0.0 for c in Jl.rows[r] if c != r), "land row not an identity row"
    ic = -1
    if rowintcon >= 0:
        hit = np.nonzero(rows == rowintcon)[0]
        if hit.size:
            ic = int(hit[0])

    def keep(r, c):
        vr, jr, ir, kr = _decode(r, n, m, l)
        vc, jc, ic_, kc = _decode(c, n, m, l)
        di = ic_ - ir
        di = np.where(periodic, (di + n) % n, di) if periodic else di
        one_i = ((di == 1) | (di == n - 1)) if periodic else (np.abs(di) == 1)
        same_i = di == 0
        dj, dk = jc - jr, kc - kr
        cell = same_i & (dj == 0) & (dk == 0)
        face = ((one_i & (dj == 0) & (dk == 0)) | (same_i & (np.abs(dj) == 1) & (dk == 0)) |
                (same_i & (dj == 0) & (np.abs(dk) == 1)))
        vert = same_i & (dj == 0) & (np.abs(dk) == 1)
        ok = cell | ((vr == vc) & face) | ((vr != vc) & vert)
        return ok & active[r] & active[c] & (r != ic)

    A = _filter(A, keep).tolil()
    if ic >= 0:
        A[ic, ic] = int_sign * intc[rowintcon]
    return A.tocsr(), active


def aggregation(nf, mf, nc, mc, l, active):
    """P: piecewise constant over 2x2 horizontal cells, same k, same variable; rows only for
    the active fine unknowns"""
    u = np.nonzero(active)[0]
    var, j, i, k = _decode(u, nf, mf, l)
    cu = var * (nc * mc * l) + ((j // 2) * nc + i // 2) * l + k
    return sp.csr_matrix((np.ones(u.size), (u, cu)), shape=(2 * nf * mf * l, 2 * nc * mc * l))


def galerkin(A, P, nc, mc, l):
    """P^T A P; a coarse unknown whose diagonal comes out 0 is inactive: its row and the 2x2
    cross terms of its cell are zeroed"""
    Ac = (P.T @ A @ P).tocsr()
    ncl = nc * mc * l
    active = Ac.diagonal() != 0.0

    def keep(r, c):
        cross = (r % ncl == c % ncl) & (r != c)
        return active[r] & ~(cross & ~active[c])
    return _filter(Ac, keep), active


class Level:
    """one level: its operator split A = V + H (V: entries inside a water column, H: between
    columns), the colour of every column, dense column blocks of V for the relaxation"""

    def __init__(self, A, active, n, m, l, periodic):
        self.A, self.active, self.n, self.m, self.l = A, active, n, m, l
        ncl = n * m * l
        self.N = 2 * ncl
        u = np.arange(self.N)
        var, j, i, k = _decode(u, n, m, l)
        colid = j * n + i
        self.H = _filter(A, lambda r, c: colid[r] != colid[c])
        V = _filter(A, lambda r, c: colid[r] == colid[c]).tocoo()
        # unknown (var, k) of column c at w = var l + k
        self.idx = (np.arange(2)[None, :, None] * ncl + np.arange(n * m)[:, None, None] * l +
                    np.arange(l)[None, None, :]).reshape(n * m, 2 * l)
        w = var * l + k
        self.Vd = np.zeros((n * m, 2 * l, 2 * l))
        np.add.at(self.Vd, (colid[V.row], w[V.row], w[V.col]), V.data)
        ina = ~active[self.idx]                              # identity rows: the value stays 0
        cc, ww = np.nonzero(ina)
        self.Vd[cc, ww, ww] = 1.0
        self.ina = ina
        jj, ii = np.arange(n * m) // n, np.arange(n * m) % n
        colour = (ii + jj) % 2
        self.ncol = ncolours(n, periodic)
        if self.ncol == 4:
            colour = np.where(ii == n - 1, 2 + jj % 2, colour)
        self.cols = [np.nonzero(colour == h)[0] for h in range(self.ncol)]

    def relax(self, h, b, z):
        """z[S] = V[S,S]^-1 (b[S] - (H z)[S]) on the columns S of colour h"""
        S = self.cols[h]
        if S.size == 0:
            return
        ix = self.idx[S]
        r = (b - self.H @ z)[ix]
        r[self.ina[S]] = 0.0
        z[ix] = np.linalg.solve(self.Vd[S], r[:, :, None])[:, :, 0]


class TsMgRef:
    """levels, operators and transfers of one Jacobian; vcycles() applies cycles V-cycles"""

    def __init__(self, rowptr, col, val, landm, n, m, l, periodic, rowintcon, int_sign, intc):
        self.n, self.m, self.l, self.periodic = n, m, l, bool(periodic)
        self.sizes = level_sizes(n, m, l)
        A, act = level0_operator(rowptr, col, val, landm, n, m, l, self.periodic, rowintcon, int_sign, intc)
        self.active0 = act
        self.levels, self.P = [], []
        for q, (a, b) in enumerate(self.sizes):
            self.levels.append(Level(A, act, a, b, l, self.periodic))
            if q + 1 < len(self.sizes):
                ca, cb = self.sizes[q + 1]
                P = aggregation(a, b, ca, cb, l, act)
                self.P.append(P)
                A, act = galerkin(A, P, ca, cb, l)
        # the coarsest level is solved directly; inactive unknowns are identity rows
        C = self.levels[-1]
        Ad = C.A.toarray()
        ina = np.nonzero(~C.active)[0]
        Ad[ina, ina] = 1.0
        self.coarse_dense = Ad
        self._trace = None

    @property
    def A(self):
        return [L.A for L in self.levels]

    def coarse_inverse(self):
        return np.linalg.inv(self.coarse_dense)

    def _cycle(self, q, b, z, sweeps):
        L = self.levels[q]
        if q == len(self.levels) - 1:
            z[:] = np.linalg.solve(self.coarse_dense, b)
        else:
            for _ in range(sweeps):
                for h in range(L.ncol):
                    L.relax(h, b, z)
            P = self.P[q]
            bc = P.T @ (b - L.A @ z)
            zc = np.zeros(bc.size)
            self._cycle(q + 1, bc, zc, sweeps)
            z += P @ zc
            for _ in range(sweeps):
                for h in range(L.ncol - 1, -1, -1):
                    L.relax(h, b, z)
        if self._trace is not None:
            self._trace["b"][q] = b.copy()
            self._trace["z"][q] = z.copy()

    def vcycles(self, b, cycles=1, sweeps=1, trace=False):
        """cycles V-cycles on A0 z = b from z = 0 (b on the level-0 unknowns, 0 on the inactive
        ones; sweeps pre- and post-sweeps per level) -> z, or with trace (z, dict(A, b, z, cinv)):
        every level's operator, the right-hand side and final iterate of the last cycle, and the
        coarsest level's inverse"""
        b = np.where(self.active0, np.asarray(b, dtype=np.float64), 0.0)
        z = np.zeros(b.size)
        for cyc in range(cycles):
            nl = len(self.levels)
            self._trace = dict(b=[None] * nl, z=[None] * nl) if trace and cyc + 1 == cycles else None
            self._cycle(0, b, z, sweeps)
        if not trace:
            return z
        t, self._trace = self._trace, None
        t["A"] = self.A
        t["cinv"] = self.coarse_inverse()
        return z, t


# ---- the preconditioner's vectors (reference order: row = 6 ((k m + j) n + i) + var) ----------

def ts_rows(n, m, l):
    """Jacobian row of every level-0 unknown"""
    var, j, i, k = _decode(np.arange(2 * n * m * l), n, m, l)
    return NUN * ((k * m + j) * n + i) + TT + var


def ts_only(r):
    """r with U, V, W and P zeroed"""
    r = np.array(r, dtype=np.float64)
    r.reshape(-1, NUN)[:, :TT] = 0.0
    return r


def apply_ts(ref, rowptr, col, val, r, cycles=1, sweeps=1, trace=False):
    """the block Gauss-Seidel apply on a right-hand side r that is zero on U, V, W and P,
    restricted to T and S (the dynamics iterate is then 0): known rows return r, the others see
    r - J[:, known] r[known] -> z on the T/S rows in reference order (0 elsewhere)"""
    n, m, l = ref.n, ref.m, ref.l
    rows = ts_rows(n, m, l)
    N = NUN * n * m * l
    J = sp.csr_matrix((np.asarray(val, dtype=np.float64), np.asarray(col), np.asarray(rowptr)), shape=(N, N))
    rk = np.zeros(N)
    known = rows[~ref.active0]
    rk[known] = r[known]
    b = (r - J @ rk)[rows]
    out = ref.vcycles(b, cycles, sweeps, trace)
    zt = out[0] if trace else out
    z = np.zeros(N)
    z[rows] = np.where(ref.active0, zt, r[rows])
    return (z, out[1]) if trace else z


# ---- the cases of tests/test_ts_mg_ref.py and tests/test_gpu_ts_mg.py ---------------------------

CASES = ("natl8", "natl8_l8", "gateway16", "2dmoc", "2dmoc_run", "box6", "natl8_l20", "natl8_l40")


# rounding floor of the reference against the C twin, max|z_TS - twin| / max|twin_TS| at
# (1 cycle, 2 cycles), as tests/test_ts_mg_ref.py measured it (its docstring has the table)
FLOOR = {"natl8": (5.2e-15, 1.0e-14), "natl8_l8": (1.9e-14, 9.4e-15), "gateway16": (4.1e-14, 8.3e-15),
         "2dmoc": (5.7e-15, 4.0e-15), "2dmoc_run": (1.3e-14, 3.2e-14), "box6": (4.6e-15, 1.1e-14),
         "natl8_l20": (1.5e-14, 4.9e-14), "natl8_l40": (7.8e-13, 1.3e-12)}


def case_config(name):
    """(configuration, land mask before the pressure-row fix-up) of a case: the smallest grids
    that reach each path of the multigrid (Mixing = 1, as the default-apply parity test)"""
    import dataclasses

    from helpers import golden_landm
    from iemic import config as cf
    if name.startswith("natl8_l"):
        l = int(name[len("natl8_l"):])
        c = cf.preset("natl8", mixing=1).with_(name=name, l=l, refine_l=l)
    elif name == "box6":
        # 2dmoc's physics at 6 x 16 x 16: the intermediate level 3 x 8 is periodic with odd n
        c = dataclasses.replace(cf.preset("2dmoc", mixing=1), name=name, n=6, m=16, l=16)
    else:
        c = cf.preset(name, mixing=1)
    generated = name.startswith("natl8_l") or name == "box6"
    L0 = cf.init_landmask(c, cf.landmask(c)) if generated else golden_landm(name)
    return c, L0
