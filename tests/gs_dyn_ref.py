"""What one dynamics pass of the block Gauss-Seidel preconditioner (gs_dyn.hip dyn_solve; its
CPU twin oracle/prec_oracle.c dyn_solve) claims to solve, stated as sparse equations: the pass
is never re-run here, its output is multiplied by a matrix and the rows are checked.  numpy and
scipy only; float64 matrices, residuals formed in np.longdouble (64-bit mantissa: a product of
two doubles and the row sums are rounded at 5e-20, so what is measured is the rounding of the
code under test, not of this file).

Unknown of the Jacobian: row = 6 cell + var, cell = (k m + j) n + i, var 0..5 = u v w p T S.

Identity rows (k_known's rule, recomputed here from the CSR): the diagonal entry is exactly 1,
every other entry of the row is exactly 0, and the row is not the integral-condition row.  They
take z = r.  The other U/V/W/P rows are the active dynamics rows D.

M_D, the matrix of one pass: the Jacobian's entries between active dynamics rows and columns,
keeping only
  U/V row at (i,j,k):  the U and V columns of the same point (the 2x2 block D) and the P columns
                       of the four corner cells (i+e, j+f, k), e,f in {0,1}           (Guv)
  W row at (i,j,k):    the P columns of the cell and of the cell above, for k < l-1    (Gw)
  P row at (i,j,k):    the U/V columns of the points (i+a, j+b, k), a,b in {-1,0}      (Duv),
                       the W columns of the cell and of the cell below                 (Dw)
(i wraps where the grid is periodic, j never).  A_DD keeps every entry between active dynamics
rows and columns (what dyn_defect applies), A_Dk the entries from active dynamics rows to
identity columns of any variable: rr_D = r_D - A_Dk r.

A pass returns z_D with M_D z_D = rr_D row by row, except on rows known from structure alone
(excepted_rows).  The rules, derived from the twin's dyn_solve:

 R1 the closing P row.  Step 5 fixes w_k from the P row of every cell whose own W is active and
    whose coefficient a = M[P_c, W_c] is not 0, so those rows hold by construction.  The other
    active P rows of a water column -- in every fixture exactly one, the top level, whose W is
    the identity row w = 0 at the surface -- are closed only by the Schur equation of the
    column.  A pinned column has pbar = 0 instead of that equation: its closing row is
    excepted.  A pass without the Schur solve has pbar = 0 in every column: the closing row of
    every water column is excepted.
 R2 in place of each excepted closing row the pass satisfies p = 0 at the column's top active
    P level (ptil starts from 0 there and pbar = 0): M(schur) holds that unit row instead, and
    pin_violation returns max |p| over them, which must be exactly 0.
 R3 rows the pass leaves without an equation (all empty in every fixture used; the CPU test
    checks that): an active U/V point whose active part of D is singular; an active W row at
    k = l-1, or whose own P is an identity row or has g0 = M[W_c, P_c] = 0; an active W row
    whose P above is an identity row while its own is active (adding pbar to one of the two
    only); a water column with more or fewer than one closing row.  no_equation_rows lists
    them; they are part of excepted_rows.

The water columns (ij_of_col) and their pin flags come from the twin's BlockGS.schur().

row_backward_error: per row |rhs - M z| / (|M||z| + |rhs|abs), rows with a zero denominator
must have a zero numerator (else inf); the maximum per row kind over the active rows that are
not excepted.  The kinds are u, v, w, p and s: "p" are the P rows that the w recursion closes,
"s" the closing P rows of the columns that are not excepted.  The s rows are the one place where
the pass is not a row-local computation: they hold through the 2-D Schur system, which one
global elimination solves (band LU in the twin, block cyclic reduction on the device), and
such a solve is backward stable in the norm, not row by row.  Measured on the twin: with a unit
impulse as right-hand side the s rows far from the impulse consist of rounding residue only
(numerator and denominator both 1e-16 .. 1e-31) and their row-wise ratio is 1.0e+00 in natl8,
gateway16, 2dmoc and global4, while every other row kind stays below 2e-14.  So the s rows are
measured in the maximum norm over their set, max |rhs - M z| / max (|M||z| + |rhs|abs): an
impulse at a seam, a wall or a pinned column makes the rows next to it the largest of the set,
which is what those right-hand sides are for.  Where the right-hand side fills every row of a
type (DENSE: the dense vectors and the vectors on one row type) no s row is residue, and the
row-wise measure of the issue is kept for them as well, as the kind "sr".
"""
import dataclasses

import numpy as np
import scipy.sparse as sp

NUN, UU, VV, WW, PP = 6, 0, 1, 2, 3
TYPES = ("u", "v", "w", "p", "s")
KINDS = TYPES + ("sr",)                   # what a right-hand side that fills its rows is judged by
DENSE = ("dense3", "dense4", "w_only", "p_only", "uv_only")
LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not extended precision on this machine"


def _coo(N, row, col, val, keep):
    return sp.csr_matrix((val[keep], (row[keep], col[keep])), shape=(N, N))


def _mv(M, x, absolute=False):
    """M x in extended precision (|M||x| with absolute), M scipy CSR"""
    M = M.tocsr()
    M.sort_indices()
    d = M.data.astype(LD)
    xv = np.asarray(x, dtype=LD)[M.indices]
    prod = np.abs(d) * np.abs(xv) if absolute else d * xv
    out = np.zeros(M.shape[0], dtype=LD)
    cnt = np.diff(M.indptr)
    ne = cnt > 0
    if prod.size:
        out[ne] = np.add.reduceat(prod, M.indptr[:-1][ne])
    return out


class DynRef:
    def __init__(self, rowptr, col, val, n, m, l, periodic, rowintcon):
        self.n, self.m, self.l, self.periodic = n, m, l, bool(periodic)
        N = self.N = NUN * n * m * l
        rowptr = np.asarray(rowptr, dtype=np.int64)
        col = np.asarray(col, dtype=np.int64)
        val = np.asarray(val, dtype=np.float64)
        assert len(rowptr) == N + 1
        row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
        # identity rows, k_known's rule
        off = np.bincount(row, weights=((col != row) & (val != 0.0)).astype(float), minlength=N)
        dg1 = np.bincount(row, weights=((col == row) & (val == 1.0)).astype(float), minlength=N)
        self.known = (off == 0) & (dg1 > 0) & (np.arange(N) != rowintcon)
        var = np.arange(N) % NUN
        self.var = var
        self.active = (var <= PP) & ~self.known
        act = self.active
        vr, vc = row % NUN, col % NUN
        ir, jr, kr = self._ijk(row // NUN)
        ic, jc, kc = self._ijk(col // NUN)
        dd = act[row] & act[col] & (val != 0.0)
        di = (ic - ir) % n if self.periodic else ic - ir        # column east of the row by di
        de = (ir - ic) % n if self.periodic else ir - ic        # column west of the row by de
        dj, dk = jc - jr, kc - kr
        same = (ir == ic) & (jr == jc)
        uvrow, uvcol = vr <= VV, vc <= VV
        keep = uvrow & uvcol & same & (dk == 0)
        keep |= uvrow & (vc == PP) & (di >= 0) & (di <= 1) & (dj >= 0) & (dj <= 1) & (dk == 0)
        keep |= (vr == WW) & (vc == PP) & same & (dk >= 0) & (dk <= 1) & (kr < l - 1)
        keep |= (vr == PP) & uvcol & (de >= 0) & (de <= 1) & (dj <= 0) & (dj >= -1) & (dk == 0)
        keep |= (vr == PP) & (vc == WW) & same & (dk <= 0) & (dk >= -1)
        self.A_DD = _coo(N, row, col, val, dd)
        self.M_D = _coo(N, row, col, val, dd & keep)
        self.A_Dk = _coo(N, row, col, val, act[row] & self.known[col] & (val != 0.0))
        self._structure()

    def _ijk(self, cell):
        return cell % self.n, (cell // self.n) % self.m, cell // (self.n * self.m)

    def row_of(self, i, j, k, var):
        return NUN * ((k * self.m + j) * self.n + i) + var

    # ---- structure: closing rows, top P levels, rows without an equation ---------------------
    def _structure(self):
        n, m, l = self.n, self.m, self.l
        act, M = self.active, self.M_D
        pa = act[PP::NUN].reshape(l, m, n)                      # active P of the cell
        wa = act[WW::NUN].reshape(l, m, n)
        cells = np.arange(n * m * l)
        a = np.asarray(M[NUN * cells + PP, NUN * cells + WW]).reshape(l, m, n)
        g0 = np.asarray(M[NUN * cells + WW, NUN * cells + PP]).reshape(l, m, n)
        self.pa, self.wa = pa, wa
        self.closing = pa & ~(wa & (a != 0.0))                 # P rows the w recursion leaves open
        top = np.full((m, n), -1)
        for k in range(l):
            top[pa[k]] = k
        self.top = top                                          # top active P level, -1: no water
        bad = []
        # active W rows without an equation, or that a column shift pbar breaks
        w_noeq = wa & ((np.arange(l)[:, None, None] == l - 1) | ~pa | (g0 == 0.0))
        pa_above = np.concatenate([pa[1:], np.zeros((1, m, n), bool)])
        w_noeq |= wa & pa & ~pa_above & (np.arange(l)[:, None, None] < l - 1)
        bad += [int(NUN * c + WW) for c in np.nonzero(w_noeq.reshape(-1))[0]]
        # U/V points whose active block of D is singular
        for c in np.nonzero(act[UU::NUN] | act[VV::NUN])[0]:
            ru, rv = NUN * c + UU, NUN * c + VV
            if act[ru] and act[rv]:
                sing = M[ru, ru] * M[rv, rv] - M[ru, rv] * M[rv, ru] == 0.0
            else:
                r = ru if act[ru] else rv
                sing = M[r, r] == 0.0
            if sing:
                bad += [int(r) for r in (ru, rv) if act[r]]
        # water columns without exactly one closing row
        ncl = self.closing.sum(axis=0)
        for j, i in zip(*np.nonzero((top >= 0) & (ncl != 1))):
            bad += [int(self.row_of(i, j, k, PP)) for k in range(l) if pa[k, j, i]]
        self.no_equation_rows = np.array(sorted(set(bad)), dtype=np.int64)

    def columns(self, schur, pinned, ij_of_col):
        """(j*n+i) of the water columns whose closing row the pass leaves open (R1)"""
        ij = np.asarray(ij_of_col, dtype=np.int64)
        return ij[np.asarray(pinned, dtype=bool)] if schur else ij

    def closing_rows(self, schur, pinned, ij_of_col):
        rows = []
        for q in self.columns(schur, pinned, ij_of_col):
            i, j = q % self.n, q // self.n
            rows += [self.row_of(i, j, k, PP) for k in np.nonzero(self.closing[:, j, i])[0]]
        return np.array(rows, dtype=np.int64)

    def top_rows(self, schur, pinned, ij_of_col):
        """the P rows on which the pass has p = 0 instead (R2)"""
        q = self.columns(schur, pinned, ij_of_col)
        i, j = q % self.n, q // self.n
        return self.row_of(i, j, self.top[j, i], PP).astype(np.int64)

    def excepted_rows(self, schur, pinned, ij_of_col):
        """sorted rows on which M_D z = rr is not claimed: structure only (R1, R3)"""
        return np.union1d(self.closing_rows(schur, pinned, ij_of_col), self.no_equation_rows)

    def M(self, schur, pinned, ij_of_col):
        """M_D with the excepted closing rows replaced by the unit rows p_top = 0 (R2)"""
        cl = self.closing_rows(schur, pinned, ij_of_col)
        tp = self.top_rows(schur, pinned, ij_of_col)
        keep = np.ones(self.N)
        keep[cl] = 0.0
        # one closing row per column (else the column is in no_equation_rows): row q of cl and
        # of tp belong to the same column
        same = len(cl) == len(tp)
        E = sp.csr_matrix((np.ones(len(tp)), (cl, tp)) if same else ([], ([], [])), shape=(self.N, self.N))
        return (sp.diags(keep) @ self.M_D + E).tocsr()

    # ---- right-hand side and residuals -----------------------------------------------------
    def rr_of(self, r):
        """(rr_D, |r_D| + |A_Dk||r|) in extended precision, 0 off the active dynamics rows"""
        r = np.asarray(r, dtype=np.float64)
        rr = np.where(self.active, r.astype(LD) - _mv(self.A_Dk, r), LD(0))
        ra = np.where(self.active, np.abs(r).astype(LD) + _mv(self.A_Dk, r, True), LD(0))
        return rr, ra

    def per_type(self, num, den, excepted):
        """max per row kind of num / den over the active rows that are not excepted; "p": the P
        rows the w recursion closes, row by row; "s": the closing P rows, which the Schur solve
        closes all at once, in the maximum norm over that set, "sr" the same rows row by row
        (module docstring); "live": the number of judged rows with a nonzero denominator"""
        ok = self.active.copy()
        ok[np.asarray(excepted, dtype=np.int64)] = False
        cl = np.zeros(self.N, dtype=bool)
        cl[NUN * np.nonzero(self.closing.reshape(-1))[0] + PP] = True
        err = _ratio(num, den)
        out = {t: float(np.max(err[ok & ~cl & (self.var == v)], initial=0.0)) for v, t in enumerate(TYPES[:4])}
        sel = ok & cl
        out["s"] = float(_ratio(np.array([np.max(num[sel], initial=LD(0))]),
                                np.array([np.max(den[sel], initial=LD(0))]))[0])
        out["sr"] = float(np.max(err[sel], initial=0.0))        # the same rows, row by row
        # rows that are judged and carry something: a case with none of them tests nothing
        out["live"] = int(np.count_nonzero(ok & (den > 0)))
        return out

    def row_backward_error(self, M, z, rhs, excepted, rhs_abs=None):
        num = np.abs(np.asarray(rhs, dtype=LD) - _mv(M, z))
        den = _mv(M, z, True) + (np.abs(np.asarray(rhs, dtype=LD)) if rhs_abs is None else rhs_abs)
        return self.per_type(num, den, excepted)

    def pin_violation(self, z, schur, pinned, ij_of_col):
        tp = self.top_rows(schur, pinned, ij_of_col)
        return float(np.max(np.abs(np.asarray(z)[tp]), initial=0.0))

    def defect(self, z, rr):
        """d = rr_D - A_DD z_D, extended precision"""
        return np.where(self.active, rr - _mv(self.A_DD, z), LD(0))

    def recurrence_error(self, M, zk, zk1, w, rr, rr_abs, excepted):
        """the step M (z_{k+1} - z_k) = w (rr_D - A_DD z_k), every term's magnitude in the
        denominator: |M|(|z_{k+1}| + |z_k|) + w (|rr|abs + |A_DD||z_k|).  The two iterates come
        from separate applications, so their difference carries the rounding of each, which
        is relative to the iterate and not to the step."""
        w = LD(w)
        num = np.abs(w * self.defect(zk, rr) - _mv(M, zk1) + _mv(M, zk))
        den = _mv(M, zk1, True) + _mv(M, zk, True) + abs(w) * (rr_abs + _mv(self.A_DD, zk, True))
        return self.per_type(num, den, excepted)

    def dmask(self, z):
        return np.where(self.active, np.asarray(z, dtype=np.float64), 0.0)


def _ratio(num, den):
    out = np.zeros(len(num), dtype=np.float64)
    nz = den > 0
    out[nz] = (num[nz] / den[nz]).astype(np.float64)
    out[~nz & (num > 0)] = np.inf
    return out


def worst(e):
    return max(e[t] for t in KINDS)


def fmt(e):
    return " ".join(f"{t} {e[t]:.1e}" for t in KINDS if t in e)


def merge(a, b, kinds=TYPES):
    return {**a, **{t: max(a.get(t, 0.0), b[t]) for t in kinds}}


def kinds_of(label):
    return KINDS if label in DENSE else TYPES


def schur_rule(schur_passes, it, dyn_iters):
    """does pass it (0-based) of dyn_iters solve the Schur system (gs_pass_schur)"""
    k = schur_passes
    return it == 0 or k <= 0 or k >= dyn_iters or (k >= 2 and (it < k - 1 or it == dyn_iters - 1))


# ---- the cases ----------------------------------------------------------------------------------

FIXTURES = ["test6x6x4", "natl8", "natl8_l8", "odd7x8x4", "gateway16", "2dmoc", "global4"]


def case_config(name, mixing):
    """(configuration, land mask before the pressure-row fix-up)"""
    from helpers import golden_landm
    from iemic import config as cf
    if name == "natl8_l8":
        c = cf.preset("natl8", mixing=mixing).with_(name=name, l=8, refine_l=8)
        return c, cf.init_landmask(c, cf.landmask(c))
    if name == "odd7x8x4":          # natl8 without its last longitude: odd n, not periodic
        c = dataclasses.replace(cf.preset("natl8", mixing=mixing), n=7)
        return c, np.delete(golden_landm("natl8"), 8, axis=2)
    return cf.preset(name, mixing=mixing), golden_landm(name)


_PROBLEMS = {}


def problem(orc, name, mixing):
    """(cfg, land mask, oracle, state, Jacobian values, DynRef, ij_of_col, pinned, rhs_cases) of a
    case, built once per session and left unchanged"""
    if (name, mixing) not in _PROBLEMS:
        from helpers import mask_fix
        from iemic import config as cf
        c, L0 = case_config(name, mixing)
        L = mask_fix(orc, c, L0)
        o = orc.Oracle(c.ref_dict(), L, c.par_list())
        x = cf.synthetic_state(c, L, amp_ts=1e-3)
        ov, _ = o.jacobian(x)
        ref = DynRef(o.rowptr, o.col, ov, c.n, c.m, c.l, c.periodic, o.rowintcon)
        _, ij, pin = orc.BlockGS(o, ov, 3).schur()
        _PROBLEMS[(name, mixing)] = (c, L0, o, x, ov, ref, ij, pin, rhs_cases(c, ref, pin, ij))
    return _PROBLEMS[(name, mixing)]


def limit(name, mixing):
    """what a planted error must exceed to count as noticed: the loosest of the per-kind bounds"""
    return max(bound(name, mixing, t) for t in KINDS)


def check(e, name, mixing, kinds, what=""):
    """every kind of e within its own bound"""
    for t in kinds:
        assert e[t] <= bound(name, mixing, t), (what, t, e[t], bound(name, mixing, t))


def rhs_cases(cfg, ref, pinned, ij_of_col):
    """[(label, r)]: dense vectors, vectors on one row type only, and unit impulses at cells
    chosen from the active-row flags: the first and last longitude and latitude that hold water,
    a water cell beside land, the bottom and the top level of one column, a pinned column, and
    an identity row that couples into the dynamics rows."""
    from iemic import config as cf
    n, m, l = ref.n, ref.m, ref.l
    d3, d4 = cf.synthetic_vector(cfg, seed=3), cf.synthetic_vector(cfg, seed=4)
    var = ref.var
    out = [("dense3", d3), ("dense4", d4), ("w_only", np.where(var == WW, d3, 0.0)),
           ("p_only", np.where(var == PP, d4, 0.0)), ("uv_only", np.where(var <= VV, d3, 0.0))]
    pa = ref.pa
    kk, jj, ii = np.nonzero(pa)

    ij = np.asarray(ij_of_col)
    pinned = np.asarray(pinned, dtype=bool)
    is_pin = np.isin(jj * n + ii, ij[pinned])

    def first(mask):
        """the first cell of the mask, of a column that is not pinned where there is one (the
        pass ignores the right-hand side of a pinned column's closing row)"""
        t = np.nonzero(mask & ~is_pin)[0]
        if not t.size:
            t = np.nonzero(mask)[0]
        return (int(ii[t[0]]), int(jj[t[0]]), int(kk[t[0]])) if t.size else None

    land_nb = np.zeros_like(pa)
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        nb = np.roll(pa, (-dj, -di), axis=(1, 2))
        if di and not ref.periodic:          # beyond the grid is a wall, not a land cell
            nb[:, :, -1 if di > 0 else 0] = True
        if dj:
            nb[:, -1 if dj > 0 else 0, :] = True
        land_nb |= pa & ~nb
    free = ij[~pinned]
    deep = int(free[np.argmax([pa[:, q // n, q % n].sum() for q in free])])
    # the deepest pinned column, its impulse one level below the top: the top P row is the
    # column's excepted closing row, whose right-hand side the pass never reads
    pcols = ij[pinned]
    pin = int(pcols[np.argmax([pa[:, q // n, q % n].sum() for q in pcols])])
    pin_k = np.nonzero(pa[:, pin // n, pin % n])[0]
    cells = {
        "i_min": first(ii == ii.min()), "i_max": first(ii == ii.max()),
        "j_min": first(jj == jj.min()), "j_max": first(jj == jj.max()),
        "land_nb": first(land_nb[kk, jj, ii]),
        "bottom": (deep % n, deep // n, int(np.nonzero(pa[:, deep // n, deep % n])[0][0])),
        "top": (deep % n, deep // n, int(ref.top[deep // n, deep % n])),
        "pinned": (pin % n, pin // n, int(pin_k[-2] if len(pin_k) > 1 else pin_k[-1])),
    }
    for label, cell in cells.items():
        if cell is None:
            continue
        for v in (UU, WW, PP):
            row = ref.row_of(*cell, v)
            if ref.active[row]:
                e = np.zeros(ref.N)
                e[row] = 1.0
                out.append((f"{label}_{'uvwp'[v]}", e))
    kcols = np.nonzero(np.diff(ref.A_Dk.tocsc().indptr))[0]
    if kcols.size:
        e = np.zeros(ref.N)
        e[kcols[len(kcols) // 2]] = 1.0
        out.append(("identity", e))
    for _, r in out:
        r.setflags(write=False)
    return out


# The twin's backward error of one pass with the Schur solve (tests/test_gs_dyn_ref.py measures
# and asserts it within a factor of 2): per (fixture, Mixing), the maximum over rhs_cases of the
# per-kind error ("sr" over the DENSE cases only).  Filled from that test's output; rounded up
# to two digits.
TWIN = {
    ("test6x6x4", 0): dict(u=3.0e-16, v=2.8e-16, w=7.7e-17, p=1.7e-16, s=2.0e-15, sr=2.5e-15),
    ("test6x6x4", 1): dict(u=3.0e-16, v=2.8e-16, w=7.7e-17, p=1.7e-16, s=2.0e-15, sr=2.5e-15),
    ("natl8", 0): dict(u=4.4e-16, v=4.6e-16, w=8.1e-17, p=1.7e-16, s=1.3e-15, sr=2.3e-15),
    ("natl8", 1): dict(u=4.4e-16, v=4.6e-16, w=8.1e-17, p=1.7e-16, s=1.3e-15, sr=2.3e-15),
    ("natl8_l8", 0): dict(u=4.2e-16, v=2.3e-16, w=6.3e-16, p=1.6e-16, s=1.8e-15, sr=3.5e-15),
    ("natl8_l8", 1): dict(u=4.2e-16, v=2.3e-16, w=6.3e-16, p=1.6e-16, s=1.8e-15, sr=3.5e-15),
    ("odd7x8x4", 0): dict(u=4.8e-16, v=5.9e-16, w=1.1e-16, p=1.4e-16, s=1.5e-15, sr=9.1e-15),
    ("odd7x8x4", 1): dict(u=4.8e-16, v=5.9e-16, w=1.1e-16, p=1.4e-16, s=1.5e-15, sr=9.1e-15),
    ("gateway16", 0): dict(u=6.0e-16, v=5.8e-16, w=1.3e-15, p=1.7e-16, s=7.7e-15, sr=2.8e-13),
    ("gateway16", 1): dict(u=6.0e-16, v=5.8e-16, w=1.3e-15, p=1.7e-16, s=7.7e-15, sr=2.8e-13),
    ("2dmoc", 0): dict(u=3.6e-16, v=3.4e-16, w=1.3e-16, p=1.4e-16, s=5.4e-15, sr=1.1e-14),
    ("2dmoc", 1): dict(u=3.6e-16, v=3.4e-16, w=1.3e-16, p=1.4e-16, s=5.4e-15, sr=1.1e-14),
    ("global4", 0): dict(u=1.1e-15, v=1.3e-15, w=1.2e-14, p=2.0e-16, s=9.6e-13, sr=1.1e-11),
    ("global4", 1): dict(u=1.1e-15, v=1.3e-15, w=1.2e-14, p=2.0e-16, s=9.6e-13, sr=1.1e-11),
}


def bound(name, mixing, t):
    """what the device may show: 100 x the twin's figure (band LU with partial pivoting there,
    block cyclic reduction without pivoting across blocks here), never looser than the 1e-8 of
    the twin comparison"""
    return min(1e-8, 100.0 * TWIN[(name, mixing)][t])
