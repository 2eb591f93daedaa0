"""ctypes binding of the device library's test hooks (i-emic_amd/csrc/test_hooks.h): the
block cyclic reduction, the batched Gauss-Jordan inverse and the band LU of the
preconditioner, each driven on its own, the T/S multigrid's plan, levels and fusion
switch, and the active set, the compressed SpMV and the dynamics defect.  Not part of the
public ABI (include/iemic.h)."""
import ctypes as C

import numpy as np

from iemic import _lib

PLAN_LEN = 128
EINVAL = -22
_PD, _PI = C.POINTER(C.c_double), C.POINTER(C.c_int)
_bound = None


def hooks():
    global _bound
    if _bound is None:
        L = _lib.lib()
        vp, i = C.c_void_p, C.c_int
        L.iemic_test_cr_solve.restype = i
        L.iemic_test_cr_solve.argtypes = [vp, i, i, i, i, _PD, _PD, _PD, _PD, _PI, i, _PD, _PD, _PD, _PI, _PI]
        L.iemic_test_cr_refactor.restype = i
        L.iemic_test_cr_refactor.argtypes = [vp, i, i, i, i] + [_PD] * 8
        L.iemic_test_cr_inverse.restype = i
        L.iemic_test_cr_inverse.argtypes = [vp, i, i, i, i, i, _PD, _PD, _PI]
        L.iemic_test_band_inverse.restype = i
        L.iemic_test_band_inverse.argtypes = [vp, i, i, i, _PD, _PI, _PD, _PI, _PI]
        L.iemic_test_coupled_prec.restype = i
        L.iemic_test_coupled_prec.argtypes = [vp, _PD, _PD, i]
        L.iemic_test_ts_mg_plan.restype = i
        L.iemic_test_ts_mg_plan.argtypes = [vp, _PI]
        L.iemic_test_ts_mg_level.restype = i
        L.iemic_test_ts_mg_level.argtypes = [vp, i] + [_PD] * 5
        L.iemic_test_ts_mg_nofuse.restype = i
        L.iemic_test_ts_mg_nofuse.argtypes = [vp, i]
        L.iemic_test_active_set.restype = i
        L.iemic_test_active_set.argtypes = [vp, C.POINTER(C.c_int64), _PI, _PI]
        L.iemic_test_spmv_c.restype = i
        L.iemic_test_spmv_c.argtypes = [vp, _PD, _PD, _PD, _PI]
        L.iemic_test_dyn_defect.restype = i
        L.iemic_test_dyn_defect.argtypes = [vp, C.c_int64, _PD, _PD, _PD]
        _bound = L
    return _bound


def coupled_prec(cm, r, use_prec):
    """cpl_prec of a iemic.coupled.CoupledModel on a host vector [ocean | atmosphere] -> z"""
    r = np.ascontiguousarray(r, dtype=np.float64)
    assert r.size == cm.N
    z = np.full(cm.N, np.nan)
    rc = hooks().iemic_test_coupled_prec(cm._h, _d(r), _d(z), int(use_prec))
    if rc:
        raise RuntimeError(f"iemic_test_coupled_prec: {rc} {last_error()}")
    return z


def last_error():
    msg = _lib.lib().iemic_last_error()
    return msg.decode() if msg else ""


def _d(a):
    return None if a is None else a.ctypes.data_as(_PD)


def _colmajor(B):
    """(n, m, m) blocks [i][row][col] -> the device's column-major blocks, flat"""
    return np.ascontiguousarray(np.transpose(np.asarray(B, dtype=np.float64), (0, 2, 1))).reshape(-1)


class Plan:
    """the hook's plan array: level counts and, per apply step, (rc, nwg, ncls, levels)"""

    def __init__(self, p):
        self.nlev, self.lt, self.tM, self.ncomp, self.nsteps = (int(v) for v in p[:5])
        q = [tuple(int(v) for v in p[5 + 4 * k: 9 + 4 * k]) for k in range(2 * self.nsteps)]
        self.down, self.up = q[:self.nsteps], q[self.nsteps:]

    def __repr__(self):
        return (f"Plan(nlev={self.nlev}, lt={self.lt}, tM={self.tM}, ncomp={self.ncomp}, "
                f"down={self.down}, up={self.up})")


def cr_solve(h, n, m, periodic, tail_max, b, D=None, L=None, R=None, S9=None, col_of_ij=None, want_xT=False):
    """-> (rc, x (nsolve, n m), xT or None, info, Plan).  b: (nsolve, n m) or None (plan only)."""
    nm = n * m
    nsolve = 0 if b is None else np.asarray(b).reshape(-1, nm).shape[0]
    bb = None if b is None else np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    x = np.full(max(nsolve, 1) * nm, np.nan)
    xT = np.full(max(nsolve, 1) * nm, np.nan) if want_xT else None
    info = C.c_int(-1)
    plan = np.zeros(PLAN_LEN, dtype=np.int32)
    blocks = [None if B is None else _colmajor(B) for B in (D, L, R)]
    s9 = None if S9 is None else np.ascontiguousarray(S9, dtype=np.float64).reshape(-1)
    col = None if col_of_ij is None else np.ascontiguousarray(col_of_ij, dtype=np.int32).reshape(-1)
    rc = hooks().iemic_test_cr_solve(h, n, m, int(periodic), int(tail_max), _d(blocks[0]), _d(blocks[1]),
                                     _d(blocks[2]), _d(s9), None if col is None else col.ctypes.data_as(_PI),
                                     nsolve, _d(bb), _d(x), _d(xT), C.byref(info), plan.ctypes.data_as(_PI))
    return (rc, x.reshape(max(nsolve, 1), nm)[:nsolve], None if xT is None else xT.reshape(-1, nm)[:nsolve],
            info.value, Plan(plan))


def cr_refactor(h, n, m, periodic, tail_max, first, second, b):
    """factor `first` = (D, L, R), solve b; factor `second` on the same SchurCR, solve b -> (rc, x)"""
    a = [_colmajor(B) for B in first] + [_colmajor(B) for B in second]
    bb = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    x = np.full(n * m, np.nan)
    rc = hooks().iemic_test_cr_refactor(h, n, m, int(periodic), int(tail_max), *[_d(v) for v in a], _d(bb), _d(x))
    return rc, x


def cr_inverse(h, A, s0, sstep, count):
    """A: (nsrc, m, m) -> (rc, X (count, m, m), info): X[k] = inverse of A[s0 + k sstep]"""
    A = np.asarray(A, dtype=np.float64)
    nsrc, m = A.shape[0], A.shape[1]
    a = _colmajor(A)
    X = np.full(count * m * m, np.nan)
    info = C.c_int(-1)
    rc = hooks().iemic_test_cr_inverse(h, m, count, s0, sstep, nsrc, _d(a), _d(X), C.byref(info))
    return rc, np.transpose(X.reshape(count, m, m), (0, 2, 1)), info.value


def band_inverse(h, N, bl, bu, ab, prefill=np.nan):
    """ab: (N, 2 bl + bu + 1) rows -> (rc, ab factored, piv, X (N, N), info, stage_o)"""
    ab = np.array(ab, dtype=np.float64)
    piv = np.full(max(N, 1), -1, dtype=np.int32)
    X = np.full((max(N, 1), max(N, 1)), prefill, dtype=np.float64)
    info, so = C.c_int(-1), C.c_int(-1)
    rc = hooks().iemic_test_band_inverse(h, N, bl, bu, _d(ab), piv.ctypes.data_as(_PI), _d(X), C.byref(info),
                                         C.byref(so))
    return rc, ab, piv, X, info.value, so.value


def ts_mg_plan(h):
    """the T/S multigrid of context h as it was last set up: dict(nlev, lanes, sweeps, hr, kind,
    sizes [(n, m)], par, colours, fused), keys as ts_mg_ref.expected_plan"""
    plan = np.zeros(PLAN_LEN, dtype=np.int32)
    rc = hooks().iemic_test_ts_mg_plan(h, plan.ctypes.data_as(_PI))
    if rc:
        raise RuntimeError(f"iemic_test_ts_mg_plan: {rc} {last_error()}")
    nlev = int(plan[0])
    lv = [[int(v) for v in plan[5 + 5 * q: 10 + 5 * q]] for q in range(nlev)]
    return dict(nlev=nlev, lanes=int(plan[1]), sweeps=int(plan[2]), hr=int(plan[3]), kind=int(plan[4]),
                sizes=[(e[0], e[1]) for e in lv], par=[e[2] for e in lv], colours=[e[3] for e in lv],
                fused=[e[4] for e in lv])


def ts_mg_level(h, q, n, m, l, coarsest):
    """level q (n x m x l cells) after the last apply -> off (16, ncl), diag (4, ncl), b (2 ncl),
    z (2 ncl), cinv ((2 ncl, 2 ncl) or None); cell (j n + i) l + k.  NaN-filled first, so an
    entry the hook does not write cannot pass for a value."""
    ncl = n * m * l
    off, diag = np.full(16 * ncl, np.nan), np.full(4 * ncl, np.nan)
    b, z = np.full(2 * ncl, np.nan), np.full(2 * ncl, np.nan)
    cinv = np.full(4 * ncl * ncl, np.nan) if coarsest else None
    rc = hooks().iemic_test_ts_mg_level(h, q, _d(off), _d(diag), _d(b), _d(z), _d(cinv))
    if rc:
        raise RuntimeError(f"iemic_test_ts_mg_level: {rc} {last_error()}")
    return off.reshape(16, ncl), diag.reshape(4, ncl), b, z, None if cinv is None else cinv.reshape(2 * ncl, 2 * ncl)


def active_set(h):
    """the active set of context h's block GS set-up -> (nact, natile, ric, act (nact,),
    atl (natile, 8)); act: owned cells, atl: the compressed SpMV's tile records"""
    cnt = np.zeros(3, dtype=np.int64)
    p64 = cnt.ctypes.data_as(C.POINTER(C.c_int64))
    rc = hooks().iemic_test_active_set(h, p64, None, None)
    if rc:
        raise RuntimeError(f"iemic_test_active_set: {rc} {last_error()}")
    nact, natile, ric = (int(v) for v in cnt)
    act = np.full(max(nact, 1), -1, dtype=np.int32)
    atl = np.full(8 * max(natile, 1), -1, dtype=np.int32)
    rc = hooks().iemic_test_active_set(h, p64, act.ctypes.data_as(_PI), atl.ctypes.data_as(_PI))
    if rc:
        raise RuntimeError(f"iemic_test_active_set: {rc} {last_error()}")
    return nact, natile, ric, act[:nact], atl[:8 * natile].reshape(natile, 8)


def spmv_c(h, x, nact):
    """k_spmv7c and k_spmv7 on the same device x (reference order) -> (yc (6 nact,), y
    (reference order), guard_changed); NaN where a kernel wrote nothing"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    yc, y = np.full(6 * nact, np.nan), np.full(x.size, np.nan)
    g = C.c_int(-1)
    rc = hooks().iemic_test_spmv_c(h, _d(x), _d(yc), _d(y), C.byref(g))
    if rc:
        raise RuntimeError(f"iemic_test_spmv_c: {rc} {last_error()}")
    return yc, y, g.value


def dyn_defect(h, z, rr):
    """spmv_dyn_defect on component-planar z, rr (6 x ext cells) -> d, NaN where unwritten"""
    z = np.ascontiguousarray(z, dtype=np.float64)
    rr = np.ascontiguousarray(rr, dtype=np.float64)
    assert z.size == rr.size
    d = np.full(z.size, np.nan)
    rc = hooks().iemic_test_dyn_defect(h, z.size, _d(z), _d(rr), _d(d))
    if rc:
        raise RuntimeError(f"iemic_test_dyn_defect: {rc} {last_error()}")
    return d


def ts_mg_nofuse(h, on):
    rc = hooks().iemic_test_ts_mg_nofuse(h, int(bool(on)))
    if rc:
        raise RuntimeError(f"iemic_test_ts_mg_nofuse: {rc} {last_error()}")
