"""Plain numpy references of right-preconditioned restarted GMRES and of IDR(s), to pin the
device FGMRES and IDR(s) solvers.

For a fixed linear right preconditioner M and x0 = 0 the k-th iterate minimises
||b - A x|| over x in M K_k(A M, b): it is defined by (A, M, b) alone, so any correct
implementation -- whatever its orthogonalisation (DCGS2, DGKS) or summation order -- must
reproduce it to rounding.  This one is written for clarity, not speed: Arnoldi by classical
Gram-Schmidt applied twice, a dense least-squares solve on the Hessenberg matrix at every
step, restarts from the true residual, all in float64 or longdouble.

IDR(s) (idrs_ref) has no such minimisation property, but with x0 = 0, a fixed shadow space P
and a fixed rule for omega its k-th iterate is again a function of (A, M, b, P) alone: the
residuals of cycle j lie in the Sonneveld space G_j, r_k is orthogonal to the first k shadow
vectors, and both fix it.  idr_shadow_raw restates the device's shadow-space numbers.
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


# ---- IDR(s) --------------------------------------------------------------------------------
IDR_SEED_OCEAN = 20261015
IDR_SEED_COUPLED = 20261017
IDR_CAP = 1e-8                  # a step whose float64-longdouble spread exceeds this is not compared


def idr_steps(s):
    """the steps that enter each branch of the device's IDR(s): 1 (jj = 0, first column), s (last
    column of the first cycle), s + 1 (first omega step), s + 2 (first gamma step, all s columns
    of G), 2 s + 1 (last gamma step), 2 s + 2 (second omega step)"""
    return sorted({1, s, s + 1, s + 2, 2 * s + 1, 2 * s + 2})


def idr_kinds(ref, ks):
    """{(kind, omega steps taken so far)} of the steps ks of an IdrRef; a comparison is complete
    with IDR_KINDS in it"""
    return {(ref.kind[k - 1], sum(q <= k for q, *_ in ref.omega)) for k in ks}


IDR_KINDS = {("first", 0), ("omega", 1), ("gamma", 1), ("omega", 2)}


def idr_shadow_raw(rows, s, seed):
    """The uniform [-1, 1] numbers of the device's shadow space before it is orthonormalised,
    (len(rows), s): splitmix64 of rows * 16 + q + 1 started from `seed`, in uint64
    wrap-around arithmetic; the top 53 bits make the double."""
    u = np.uint64
    rows = np.asarray(rows, dtype=np.int64).astype(np.uint64)
    out = np.empty((len(rows), s))
    for q in range(s):
        z = u(0x9E3779B97F4A7C15) * (rows * u(16) + u(q + 1)) + u(seed)
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        z = z ^ (z >> u(31))
        out[:, q] = 2.0 * ((z >> u(11)).astype(np.float64) * (1.0 / 9007199254740992.0)) - 1.0
    return out


@dataclass
class IdrRef:
    x_steps: list = field(default_factory=list)    # iterate after every update of x
    rho: list = field(default_factory=list)        # ||b - A x_k|| / ||b|| of those iterates
    rec: list = field(default_factory=list)        # the recursively updated ||r_k|| / ||b||
    r_steps: list = field(default_factory=list)    # the recursively updated r_k
    kind: list = field(default_factory=list)       # per step: "first", "gamma" or "omega"
    omega: list = field(default_factory=list)      # per omega step: (step, rho, rule fired, omega)
    v: list = field(default_factory=list)          # per gamma step: (step, v, scale of its rounding)
    P: np.ndarray = None                           # the orthonormalised shadow space (n, s)


def idrs_ref(A, M, b, P, s, steps, angle=0.7, dtype=np.float64) -> IdrRef:
    """Bi-orthogonal IDR(s) (van Gijzen and Sonneveld, ACM TOMS 38(1), 2011, algorithm 1) with
    x0 = 0, right preconditioned: v = r - G gamma, t = M v, u_k = omega t + U gamma,
    g_k = A u_k, then g_k (and u_k) made orthogonal to p_1 .. p_{k-1} one after another,
    r -= beta g_k, x += beta u_k; after s such steps v = M r, t = A v, omega by the 'maintain
    the convergence' rule (omega = t.r / t.t, scaled by angle / rho when
    rho = |t.r| / (|t| |r|) < angle), r -= omega t, x += omega v.  The first cycle starts from
    G = U = 0, M = I and omega = 1, so its u_k is M r.

    P: (n, s), orthonormalised here in order (Gram-Schmidt, twice) in dtype.  Every update of x
    is one step; `steps` of them are taken, or fewer when mu_kk = 0 or t = 0 (breakdown).
    A, M: as for fgmres_ref."""
    Af = _as_callable(A)
    T = dtype
    op = lambda v: np.asarray(Af(v)).astype(T)
    if M is None:
        prec = lambda v: v.copy()
    else:
        prec = lambda v: np.asarray(M(np.asarray(v, dtype=np.float64))).astype(T)
    b = np.asarray(b).astype(T)
    n = len(b)
    Q = np.asarray(P).astype(T).copy()
    assert Q.shape == (n, s)
    for j in range(s):
        for _ in range(2):
            Q[:, j] -= Q[:, :j] @ (Q[:, :j].T @ Q[:, j])
        Q[:, j] /= _nrm(Q[:, j])
    out = IdrRef(P=Q)
    bnorm = _nrm(b)
    x = np.zeros(n, dtype=T)
    r = b.copy()
    G = np.zeros((n, s), dtype=T)
    U = np.zeros((n, s), dtype=T)
    Mu = np.eye(s, dtype=T)
    om = T(1)
    cycle = 0

    def record(kind):
        out.x_steps.append(x.copy())
        out.r_steps.append(r.copy())
        out.rho.append(_nrm(b - op(x)) / bnorm)
        out.rec.append(_nrm(r) / bnorm)
        out.kind.append(kind)
        return len(out.x_steps) >= steps

    while True:
        f = Q.T @ r
        rn0 = _nrm(r)                 # f is updated recursively: its rounding is of this size
        for k in range(s):
            # gamma: the lower-triangular system Mu(k:s, k:s) gamma = f(k:s)
            c = np.zeros(s - k, dtype=T)
            for i in range(s - k):
                c[i] = (f[k + i] - Mu[k + i, k:k + i] @ c[:i]) / Mu[k + i, k + i]
            v = r - G[:, k:] @ c
            if cycle > 0:
                scale = rn0 + sum(abs(c[i]) * _nrm(G[:, k + i]) for i in range(s - k))
                out.v.append((len(out.x_steps) + 1, v, scale))
            t = prec(v)
            u = om * t + U[:, k:] @ c
            g = op(u)
            for i in range(k):
                alpha = (Q[:, i] @ g) / Mu[i, i]
                g = g - alpha * G[:, i]
                u = u - alpha * U[:, i]
            G[:, k], U[:, k] = g, u
            Mu[k:, k] = Q[:, k:].T @ g
            if Mu[k, k] == 0:
                return out
            beta = f[k] / Mu[k, k]
            r = r - beta * g
            x = x + beta * u
            if k + 1 < s:
                f[:k + 1] = 0
                f[k + 1:] = f[k + 1:] - beta * Mu[k + 1:, k]
            if record("gamma" if cycle > 0 else "first"):
                return out
        cycle += 1
        v = prec(r)
        t = op(v)
        nt, nr, ts = _nrm(t), _nrm(r), t @ r
        if not nt > 0 or not nr > 0:
            return out
        rho = abs(ts / (nt * nr))
        om = ts / (nt * nt)
        fired = bool(rho < angle)
        if fired:
            om = om * angle / rho
        r = r - om * t
        x = x + om * v
        out.omega.append((len(out.x_steps) + 1, float(rho), fired, float(om)))
        if record("omega"):
            return out
