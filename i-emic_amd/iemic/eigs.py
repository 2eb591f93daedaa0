"""Linear stability of a steady state: the eigenvalues of ``J x = lambda B x`` nearest a shift.

The reference's drivers answer this with a JDQZ generalised eigenvalue solver built on the
model's ``applyMatrix`` / ``applyMassMat`` / ``applyPrecon`` (``src/utils/JDQZInterface.H``,
``run_ocean.C:82-97``) and run by ``Continuation::eigenSolver`` (Continuation.H:1108-1131).
JDQZ is an external library; this is an original solver behind the same seam: shift-invert
Arnoldi on ``(J - sigma B)^-1 B`` with thick (Krylov-Schur) restarts (csrc/eigs.hip;
iemic/krylov_schur.py holds the restart's host algebra), whose eigenvalues
``theta = 1 / (lambda - sigma)`` are largest for the ``lambda`` nearest the real shift.  ``B`` is
singular (zero on the W, P, land and integral-condition rows); the operator maps the infinite
eigenvalues to zero, so they never appear.  A perturbation grows like ``exp(lambda t)``: the
state is stable iff every finite ``lambda`` has a negative real part.

The device side does the Arnoldi steps, the restart's pass over the basis, the Ritz vectors and
the true residuals; the small eigenproblem of the Rayleigh matrix is solved here with
``numpy.linalg.eig``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from . import krylov_schur as ks
from ._lib import IemicError, check, lib, ptr

__all__ = ["EigResult", "EigenSolver", "ritz_groups", "rayleigh_groups", "eigs"]

MAX_RITZ_COLUMNS = 16       # iemic_eigs_ritz forms at most 16 vectors in its one pass


@dataclass
class EigResult:
    """The wanted eigenpairs, sorted by ``|lambda - sigma|`` ascending, a conjugate pair adjacent
    with the positive imaginary part first.  ``vecs[i]`` is ``(re, im, sign)``: the eigenvector of
    ``lam[i]`` is ``re + sign * 1j * im`` (device vectors; ``im`` is None for a real pair; the two
    members of a pair share their vectors).  ``residual`` is the true relative residual
    ``||(J - sigma B) x - (lambda - sigma) B x|| / ||(J - sigma B) x||`` measured on the device,
    ``estimate`` the Arnoldi estimate ``|h_{j+1,j}| |e_j^T y| / |theta|`` the stopping test used
    (after a restart its general form ``|g . y| / |theta|``, g the last row of ``H``).  ``steps`` is
    the number of inner solves over the whole run, ``restarts`` the number of thick restarts
    performed; ``H`` is the final Rayleigh matrix, Hessenberg only when ``restarts`` is 0."""
    sigma: float
    lam: np.ndarray
    vecs: list
    residual: np.ndarray
    estimate: np.ndarray
    converged: np.ndarray
    steps: int
    breakdown: bool
    solve_iters: list = field(default_factory=list)
    solve_unconverged: int = 0          # inner solves that missed the FGMRES tolerance
    H: np.ndarray = None                # the final (j + 1) x j Rayleigh matrix (j = steps without restarts)
    ops: object = None
    restarts: int = 0                   # thick restarts performed

    def to_host(self, i: int) -> np.ndarray:
        """eigenvector i as a complex host vector in the reference row order (this rank's rows)"""
        re, im, sign = self.vecs[i]
        x = self.ops.to_host(re).astype(np.complex128)
        if im is not None:
            x += sign * 1j * self.ops.to_host(im)
        return x

    @property
    def stable(self) -> bool:
        """no returned eigenvalue has a non-negative real part (of the pairs nearest the shift)"""
        return bool(np.all(self.lam.real < 0))


def ritz_groups(H: np.ndarray, j: int, k: int):
    """The wanted Ritz pairs of the leading j x j block of H ((j + 1) x j or larger): the k
    largest |theta|, a conjugate pair never split (then k + 1).  Returns a list of groups
    ``(theta, y, estimate, multiplicity)`` sorted by |theta| descending, y of unit 2-norm; a
    complex group stands for theta and its conjugate and carries the member with imag < 0,
    whose lambda = sigma + 1 / theta has the positive imaginary part."""
    th, Y = np.linalg.eig(H[:j, :j])
    hn = abs(H[j, j - 1]) if H.shape[0] > j else 0.0
    groups, i = [], 0
    while i < j:
        if th[i].imag != 0.0 and i + 1 < j and th[i + 1] == np.conj(th[i]):
            q = i if th[i].imag < 0 else i + 1
            groups.append((th[q], Y[:, q], 2))
            i += 2
        else:
            groups.append((complex(th[i].real, 0.0) if th[i].imag == 0.0 else th[i], Y[:, i], 1))
            i += 1
    groups.sort(key=lambda g: -abs(g[0]))
    out, n = [], 0
    for t, y, cnt in groups:
        if n >= k:
            break
        est = hn * abs(y[j - 1]) / abs(t) if abs(t) > 0 else np.inf
        out.append((t, y / np.linalg.norm(y), est, cnt))
        n += cnt
    return out


def rayleigh_groups(R: np.ndarray, j: int, k: int):
    """``ritz_groups`` for a Rayleigh matrix R that need not be Hessenberg (after a thick
    restart its last row g is full): the same groups with the estimate ``|g . y| / |theta|``,
    which for a Hessenberg matrix is ritz_groups' own."""
    return [(t, y, ks.general_estimate(R, j, t, y), cnt) for t, y, _, cnt in ritz_groups(R, j, k)]


def eigs(oc, k: int = 6, sigma: float = 0.0, m: int = 40, tol: float = 1e-8, seed: int = 1,
         restarts: int = 0, keep: int = None) -> EigResult:
    """``Ocean.eigs``: see there."""
    k, m, restarts = int(k), int(m), int(restarts)
    if k < 1:
        raise IemicError(f"Ocean.eigs: k = {k} eigenvalues wanted, need at least 1")
    if k > m:
        raise IemicError(f"Ocean.eigs: k = {k} exceeds the basis size m = {m}")
    if k + 1 > MAX_RITZ_COLUMNS:
        raise IemicError(f"Ocean.eigs: k = {k} exceeds {MAX_RITZ_COLUMNS - 1} (one Ritz-vector pass)")
    if restarts < 0:
        raise IemicError(f"Ocean.eigs: restarts = {restarts}, need at least 0")
    if restarts > 0:
        keep = ks.default_keep(k, m) if keep is None else int(keep)
        if not k <= keep <= min(ks.MAX_KEEP, m - 1):
            raise IemicError(f"Ocean.eigs: keep = {keep} directions across a restart, need k = {k} <= keep <= "
                             f"min({ks.MAX_KEEP}, m - 1 = {m - 1})")
    L, h = lib(), oc._h
    kr = oc._krylov()
    check(L.iemic_eigs_begin(h, float(sigma), m, int(seed) & (2 ** 64 - 1), C.byref(kr)), "iemic_eigs_begin")
    oc._recomp_prec = True              # the preconditioner now belongs to J - sigma B
    try:
        H = np.zeros((m + 1, m))
        hcol = np.zeros(m + 2)
        iters, unconv, steps, broke, groups, nrest = [], 0, 0, False, [], 0
        while True:
            # steps: the length of the decomposition (the solves since the last restart + its p)
            for j in range(steps, m):
                info = _lib.EigsInfo()
                rc = L.iemic_eigs_step(h, C.byref(kr), ptr(hcol), C.byref(info))
                if rc != _lib.IEMIC_ENOCONV:
                    check(rc, "iemic_eigs_step")
                else:
                    unconv += 1
                oc.last_solve = info.solve
                if oc.solve_hook is not None:
                    oc.solve_hook(info.solve)
                H[:j + 2, j] = hcol[:j + 2]
                iters.append(int(info.solve.iters))
                steps, broke = j + 1, bool(info.breakdown)
                if steps >= k or broke:
                    # until the first restart H is Hessenberg and the estimate today's, bit for bit
                    groups = ritz_groups(H, steps, k) if nrest == 0 else rayleigh_groups(H, steps, k)
                    if broke or all(g[2] <= tol for g in groups):
                        break
            if broke or steps < m or nrest >= restarts or all(g[2] <= tol for g in groups):
                break
            # thick restart: keep the `keep` largest Ritz values' invariant subspace and go on
            Q, R = ks.restart(H, steps, keep)
            p = Q.shape[1]
            check(L.iemic_eigs_restart(h, p, ptr(Q)), "iemic_eigs_restart")
            H[:] = 0.0
            H[:p + 1, :p] = R
            steps, nrest = p, nrest + 1
        if not groups:
            groups = ritz_groups(H, steps, k)
        # one pass over the basis for every wanted vector: Re (and Im) columns of the groups
        cols = []
        for t, y, est, cnt in groups:
            cols.append(y.real)
            if cnt == 2:
                cols.append(y.imag)
        Y = np.ascontiguousarray(np.stack(cols, axis=1), dtype=np.float64)        # steps x p
        ops = oc.vec_ops()
        from .ocean import DeviceVec
        xs = [DeviceVec(oc) for _ in cols]
        arr = (C.c_void_p * len(xs))(*[x.p for x in xs])
        check(L.iemic_eigs_ritz(h, steps, len(xs), ptr(Y), arr), "iemic_eigs_ritz")
        lam, vecs, res, ests = [], [], [], []
        out2 = np.zeros(2)
        q = 0
        for t, y, est, cnt in groups:
            lm = sigma + 1.0 / t
            re, im = xs[q], (xs[q + 1] if cnt == 2 else None)
            q += cnt
            check(L.iemic_eigs_residual(h, lm.real, lm.imag if cnt == 2 else 0.0, re.p, im.p if im else None,
                                        ptr(out2)), "iemic_eigs_residual")
            r = out2[0] / out2[1] if out2[1] > 0 else np.inf
            for sign in ((1.0, -1.0) if cnt == 2 else (1.0,)):
                lam.append(complex(lm.real, sign * lm.imag) if cnt == 2 else complex(lm.real, 0.0))
                vecs.append((re, im, sign))
                res.append(r)
                ests.append(est)
        ests = np.array(ests)
        return EigResult(sigma=float(sigma), lam=np.array(lam), vecs=vecs, residual=np.array(res), estimate=ests,
                         converged=(ests <= tol) | broke, steps=len(iters), breakdown=broke, solve_iters=iters,
                         solve_unconverged=unconv, H=H[:steps + 1, :steps].copy(), ops=ops, restarts=nrest)
    finally:
        L.iemic_eigs_end(h)


class EigenSolver:
    """What ``Continuation.eigen_solver`` expects (the role of the JDQZ solver handed to
    ``Continuation::setEigenSolver``): ``solve()`` analyses the model's current state."""

    def __init__(self, model, **kw):
        self.model = model
        self.kw = kw

    def solve(self) -> EigResult:
        return self.model.eigs(**self.kw)
