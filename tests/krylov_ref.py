"""A plain numpy reference of right-preconditioned restarted GMRES, to pin the device FGMRES.

For a fixed linear right preconditioner M and x0 = 0 the k-th iterate minimises
||b - A x|| over x in M K_k(A M, b): it is defined by (A, M, b) alone, so any correct
implementation -- whatever its orthogonalisation (DCGS2, DGKS) or summation order -- must
reproduce it to rounding.  This one is written for clarity, not speed: Arnoldi by classical
Gram-Schmidt applied twice, a dense least-squares solve on the Hessenberg matrix at every
step, restarts from the true residual, all in float64 or longdouble.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


def csr_operator(rowptr, col, val, dtype=np.float64):
    """y = A x for the CSR triple, accumulated in dtype (row sums by np.add.reduceat)."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    v = np.asarray(val).astype(dtype)
    start = rowptr[:-1]
    empty = rowptr[1:] == start
    # reduceat needs every start inside the array; rows without entries are zeroed after
    safe = np.minimum(start, max(len(v) - 1, 0))

    def apply(x):
        y = np.add.reduceat(v * np.asarray(x, dtype=dtype)[col], safe)
        y[empty] = 0
        return y

    return apply


def _as_callable(A):
    if callable(A):
        return A
    return lambda x: A @ x          # scipy CSR (or a dense matrix)


@dataclass
class GmresRef:
    x_cycles: list = field(default_factory=list)   # iterate after each cycle
    x_steps: list = field(default_factory=list)    # iterate after every step (all cycles)
    rho: list = field(default_factory=list)        # ||b - A x_k|| / ||b|| of those iterates
    givens: list = field(default_factory=list)     # the Givens (implicit) estimate of the same
    H: list = field(default_factory=list)          # the (k+1) x k Hessenberg matrix of each cycle


def _nrm(v):
    return np.sqrt(v @ v)


def fgmres_ref(A, M, b, m, restarts=0, dtype=np.float64) -> GmresRef:
    """Right-preconditioned GMRES(m), x0 = 0, restarts + 1 cycles of m steps.

    A: callable or a matrix with @; M: callable or None (identity); dtype: np.float64 or
    np.longdouble -- the vectors, the Hessenberg matrix and the Givens rotations are kept in
    it (A and M see and return whatever they support; their output is cast).  No stopping
    test: every cycle runs its m steps unless Arnoldi breaks down (h_{j+1,j} = 0)."""
    Af = _as_callable(A)
    T = dtype
    op = lambda v: np.asarray(Af(v)).astype(T)
    if M is None:
        prec = lambda v: v.copy()
    else:
        prec = lambda v: np.asarray(M(np.asarray(v, dtype=np.float64))).astype(T)
    b = np.asarray(b).astype(T)
    n = len(b)
    bnorm = _nrm(b)
    out = GmresRef()
    x = np.zeros(n, dtype=T)
    r = b.copy()
    for _ in range(restarts + 1):
        beta = _nrm(r)
        if not beta > 0:
            break
        V = np.zeros((m + 1, n), dtype=T)
        Z = np.zeros((m, n), dtype=T)
        H = np.zeros((m + 1, m), dtype=T)
        V[0] = r / beta
        # Givens recurrence for the implicit estimate
        R = np.zeros((m + 1, m), dtype=T)
        cs = np.zeros(m, dtype=T)
        sn = np.zeros(m, dtype=T)
        g = np.zeros(m + 1, dtype=T)
        g[0] = beta
        k = 0
        xk = x
        for j in range(m):
            Z[j] = prec(V[j])
            w = op(Z[j])
            Q = V[:j + 1]
            h = Q @ w
            w = w - h @ Q
            h2 = Q @ w
            w = w - h2 @ Q
            H[:j + 1, j] = h + h2
            hn = _nrm(w)
            H[j + 1, j] = hn
            k = j + 1
            # implicit estimate
            R[:j + 2, j] = H[:j + 2, j]
            for i in range(j):
                a0, a1 = R[i, j], R[i + 1, j]
                R[i, j] = cs[i] * a0 + sn[i] * a1
                R[i + 1, j] = -sn[i] * a0 + cs[i] * a1
            d = np.sqrt(R[j, j] ** 2 + R[j + 1, j] ** 2)
            cs[j], sn[j] = (R[j, j] / d, R[j + 1, j] / d) if d > 0 else (T(1), T(0))
            R[j, j], R[j + 1, j] = d, 0
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            # the iterate of this step: min || beta e1 - H_k y || by a small dense solve
            y = _lstsq(H[:k + 1, :k], beta, T)
            xk = x + y @ Z[:k]
            out.x_steps.append(xk)
            out.rho.append(_nrm(b - op(xk)) / bnorm)
            out.givens.append(abs(g[j + 1]) / bnorm)
            if not hn > 0:
                break
            V[j + 1] = w / hn
        out.H.append(H[:k + 1, :k].copy())
        x = xk
        out.x_cycles.append(x)
        r = b - op(x)
    return out


def _lstsq(Hk, beta, T):
    """argmin_y || beta e1 - Hk y ||_2 in dtype T: a fresh QR of the small upper Hessenberg
    matrix by Givens rotations and a back substitution (numpy's LAPACK drivers are float64
    only)."""
    k1, k = Hk.shape
    Rm = Hk.astype(T).copy()
    rhs = np.zeros(k1, dtype=T)
    rhs[0] = beta
    for i in range(k):
        a0, a1 = Rm[i, i], Rm[i + 1, i]
        d = np.sqrt(a0 * a0 + a1 * a1)
        if not d > 0:
            continue
        c, s = a0 / d, a1 / d
        ri, ri1 = Rm[i].copy(), Rm[i + 1].copy()
        Rm[i] = c * ri + s * ri1
        Rm[i + 1] = -s * ri + c * ri1
        rhs[i], rhs[i + 1] = c * rhs[i] + s * rhs[i + 1], -s * rhs[i] + c * rhs[i + 1]
    y = np.zeros(k, dtype=T)
    for i in range(k - 1, -1, -1):
        y[i] = (rhs[i] - Rm[i, i + 1:k] @ y[i + 1:k]) / Rm[i, i]
    return y


def krylov_lstsq_residual(A, b, k, dtype=np.longdouble):
    """min ||b - A x|| / ||b|| over x in K_k(A, b), by a route that shares nothing with the
    Hessenberg machinery: an explicitly orthonormalised basis Q_k of the Krylov space (each
    new direction A q orthogonalised twice against all earlier ones), then a dense float64
    least-squares problem min_y ||b - (A Q_k) y||.  Returns (relative residual, x)."""
    Af = _as_callable(A)
    T = dtype
    b = np.asarray(b).astype(T)
    Q = np.zeros((k, len(b)), dtype=T)
    Q[0] = b / _nrm(b)
    for j in range(1, k):
        w = np.asarray(Af(Q[j - 1])).astype(T)
        for _ in range(2):
            w = w - (Q[:j] @ w) @ Q[:j]
        Q[j] = w / _nrm(w)
    AQ = np.stack([np.asarray(Af(q)).astype(T) for q in Q], axis=1)
    y, *_ = np.linalg.lstsq(AQ.astype(np.float64), b.astype(np.float64), rcond=None)
    x = y.astype(T) @ Q
    return _nrm(b - np.asarray(Af(x)).astype(T)) / _nrm(b), x
