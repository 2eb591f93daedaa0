"""CPU references for the dense solvers of the preconditioner (tests/test_gpu_dense.py).

cr_ref            plain float64 block cyclic reduction, written from the recurrences in the
                  header of csrc/schur_cr.hip: odd/even elimination, the periodic wrap, the
                  direct coupling kept for odd counts, the merged periodic pair.  No tail, no
                  composed steps, no packing; np.linalg.inv per block.  The rounding yardstick.
refined_solve     sparse LU + three refinement steps with the residual in np.longdouble:
                  the high-precision solution.
refined_inverse   the same for a dense inverse.
builders          the manufactured test matrices and the case tables shared by the CPU checks
                  (tests/test_cr_ref.py) and the GPU tests.
"""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.linalg import lapack

EPS = float(np.finfo(np.float64).eps)


# ---------------------------------------------------------------- block cyclic reduction
def cr_ref(D, L, R, b, periodic):
    """x of L_i x_{i-1} + D_i x_i + R_i x_{i+1} = b_i.  D, L, R: (n, m, m); b: (n, m)."""
    n = len(D)
    D, L, R, b = (np.array(v, dtype=np.float64) for v in (D, L, R, b))
    if n == 1:
        return (np.linalg.inv(D[0]) @ b[0])[None, :]
    if n == 2 and periodic:                       # both couplings reach the same block
        R[0] = L[0] + R[0]
        L[1] = L[1] + R[1]
        periodic = False
    ne = (n + 1) // 2
    Dinv = {o: np.linalg.inv(D[o]) for o in range(1, n, 2)}
    m = D.shape[1]
    Dn, Ln, Rn = (np.zeros((ne, m, m)) for _ in range(3))
    bn = np.zeros((ne, m))
    for q in range(ne):
        e = 2 * q
        lnb = e - 1 if e > 0 else (n - 1 if periodic else None)
        rnb = e + 1 if e + 1 < n else (0 if periodic else None)
        Dn[q], bn[q] = D[e], b[e]
        if lnb is not None:
            if lnb & 1:
                X = L[e] @ Dinv[lnb]
                Dn[q] = Dn[q] - X @ R[lnb]
                Ln[q] = -(X @ L[lnb])
                bn[q] = bn[q] - X @ b[lnb]
            else:
                Ln[q] = L[e]                      # odd count: two even blocks adjacent across the wrap
        if rnb is not None:
            if rnb & 1:
                X = R[e] @ Dinv[rnb]
                Dn[q] = Dn[q] - X @ L[rnb]
                Rn[q] = -(X @ R[rnb])
                bn[q] = bn[q] - X @ b[rnb]
            else:
                Rn[q] = R[e]
    xe = cr_ref(Dn, Ln, Rn, bn, periodic)
    x = np.zeros((n, m))
    x[0::2] = xe
    for o in range(1, n, 2):
        r = b[o] - L[o] @ x[o - 1]
        if o + 1 < n or periodic:
            r = r - R[o] @ x[(o + 1) % n]
        x[o] = Dinv[o] @ r
    return x


def assemble(D, L, R, periodic):
    """the block tridiagonal (periodic) matrix as CSR; n = 1: D alone"""
    n, m = len(D), D.shape[1]
    rows = []
    for i in range(n):
        row = [None] * n
        row[i] = sp.csr_matrix(D[i])
        if n > 1:
            for B, j in ((L[i], i - 1), (R[i], i + 1)):
                if not periodic and (j < 0 or j >= n):
                    continue
                j %= n
                row[j] = sp.csr_matrix(B) if row[j] is None else row[j] + sp.csr_matrix(B)
        rows.append(row)
    A = sp.bmat(rows, format="csr")
    A.sort_indices()
    return A


def _residual_ld(A, x, b):
    """b - A x with products and sums in np.longdouble (A: CSR without empty rows)"""
    p = A.data.astype(np.longdouble) * np.asarray(x, dtype=np.longdouble)[A.indices]
    return np.asarray(b, dtype=np.longdouble) - np.add.reduceat(p, A.indptr[:-1])


def refined_solve(A, b, steps=3):
    A = sp.csr_matrix(A)
    lu = spla.splu(A.tocsc())
    x = lu.solve(np.asarray(b, dtype=np.float64)).astype(np.longdouble)
    for _ in range(steps):
        r = _residual_ld(A, x, b)
        x = x + lu.solve(r.astype(np.float64)).astype(np.longdouble)
    return x


def refined_inverse(A, steps=3):
    """dense inverse, refined with residuals in np.longdouble (returned as longdouble)"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    lu = sla.lu_factor(A)
    X = sla.lu_solve(lu, np.eye(n)).astype(np.longdouble)
    AL, I = A.astype(np.longdouble), np.eye(n, dtype=np.longdouble)
    for _ in range(steps):
        X = X + sla.lu_solve(lu, (I - AL @ X).astype(np.float64)).astype(np.longdouble)
    return X


def rel_err(x, xs):
    """||x - x*||inf / ||x*||inf over all entries"""
    xs = np.asarray(xs, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(x, dtype=np.longdouble) - xs)) / np.max(np.abs(xs)))


def bound(err_ref, size):
    """the tolerance rule of the GPU tests"""
    return max(10.0 * err_ref, 8.0 * size * EPS)


def build_blocks(n, m, seed):
    """Dense D, L, R with entries uniform in (-1, 1) -- the couplings as large as D's
    off-diagonal entries, so a dropped or misplaced block moves the answer at first order --
    and D's diagonal shifted to 1.3 x the largest absolute row sum of the whole block row:
    block diagonal dominance, which keeps every level of the reduction well conditioned."""
    rng = np.random.default_rng(seed)
    D, L, R = (rng.uniform(-1.0, 1.0, (n, m, m)) for _ in range(3))
    idx = np.arange(m)
    D[:, idx, idx] = 0.0
    shift = 1.3 * (np.abs(D).sum(2) + np.abs(L).sum(2) + np.abs(R).sum(2)).max()
    D[:, idx, idx] = shift * rng.choice([-1.0, 1.0], (n, m))
    if n == 1:
        L[:] = 0.0
        R[:] = 0.0
    return D, L, R


def build_rhs(A, seed, k=1):
    """b = A x0 with |x0| in [0.5, 1.5]: every entry of the solution is of size 1"""
    rng = np.random.default_rng(seed + 7919)
    x0 = rng.uniform(0.5, 1.5, (k, A.shape[0])) * rng.choice([-1.0, 1.0], (k, A.shape[0]))
    return np.stack([A @ v for v in x0])


@functools.lru_cache(maxsize=None)
def cr_system(n, m, periodic, seed=0):
    """(D, L, R, A, b (n m), x* longdouble, err_ref) -- computed once, read-only"""
    D, L, R = build_blocks(n, m, 1000 * n + 10 * m + periodic + seed)
    A = assemble(D, L, R, periodic)
    b = build_rhs(A, n + m + seed)[0]
    xs = refined_solve(A, b)
    xr = cr_ref(D, L, R, b.reshape(n, m), periodic).reshape(-1)
    for a in (D, L, R, b, xs):
        a.setflags(write=False)
    return D, L, R, A, b, xs, rel_err(xr, xs)


# (n, m, periodic, tail_max) of every cyclic-reduction solve of the GPU tests
CHAIN_N = (1, 2, 3, 4, 5, 6, 7, 12, 13, 23, 45, 96)
CR_CHAIN = [(n, 5, per, tm) for n in CHAIN_N for per in (0, 1) for tm in (1, 0)]
# tail placed at level 1 / 2 / 3 (m = 5: level sizes 225 115 60 30 ... and 480 240 120 60 ...)
CR_TAILPOS = [(45, 5, per, tm) for per in (0, 1) for tm in (115, 60, 30)] + \
             [(96, 5, per, tm) for per in (0, 1) for tm in (240, 120, 60)]
CR_RC4 = [(n, m, per, 1) for (n, m) in ((6, 128), (6, 129), (6, 192), (7, 33)) for per in (0, 1)]
# rc = 8 needs >= 448 workgroups in the step: outputs x ceil(m / 8).  The two-level down step
# has about n / 2 outputs, so m = 33 (5 chunks) needs n >= 180 (the issue's n = 96 gives 240
# workgroups and rc = 4 on the way down); m = 96 / 97 (12 / 13 chunks) are there at n = 80.
CR_RC8 = [(180, 33, 1, 0), (80, 96, 1, 0), (80, 97, 1, 0), (80, 97, 0, 0)]
CR_INVLEV = [(5, m, per, 1) for m in (100, 170) for per in (0, 1)]
CR_TAILEDGE = [(8, 128, 1, 0), (7, 33, 1, 0), (7, 33, 0, 0)]
CR_CASES = CR_CHAIN + CR_TAILPOS + CR_RC4 + CR_RC8 + CR_INVLEV + CR_TAILEDGE


# ---------------------------------------------------------------- 9-point rows (k_cr_expand)
def build_s9(n, m, periodic, seed):
    """Random 9-point rows S9[c, (dj+1)*3 + (di+1)], c = i m + j, with a land pattern: about a
    third of the columns (one whole longitude among them) have col_of_ij < 0.  As in the
    pinned Schur matrix no water row couples to a land column.  -> (S9, col_of_ij (m, n), A)"""
    rng = np.random.default_rng(seed)
    p = 0.3 if n <= 2 else max(0.1, (1.0 / 3 - 1.0 / n) / (1 - 1.0 / n))
    land = rng.uniform(size=(n, m)) < p
    if n > 2:
        land[n // 2, :] = True
    S9 = rng.uniform(-1.0, 1.0, (n * m, 9))
    S9[:, 4] = 0.0
    S9[:, 4] = 1.3 * np.abs(S9).sum(1).max() * rng.choice([-1.0, 1.0], n * m)
    col = np.where(land.T, -1, np.arange(n * m).reshape(n, m).T).astype(np.int32)     # (m, n)
    A = sp.lil_matrix((n * m, n * m))
    for i in range(n):
        for j in range(m):
            c = i * m + j
            if land[i, j]:
                A[c, c] = 1.0
                continue
            for o in range(9):
                di, dj = o % 3 - 1, o // 3 - 1
                ti, tj = i + di, j + dj
                if tj < 0 or tj >= m:
                    continue
                if ti < 0 or ti >= n:
                    if not periodic:
                        continue
                    ti %= n
                if land[ti, tj]:
                    S9[c, o] = 0.0
                    continue
                A[c, ti * m + tj] += S9[c, o]
    A = A.tocsr()
    A.sort_indices()
    return S9, col, A, land


# ---------------------------------------------------------------- Gauss-Jordan blocks
GJ_M = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 160, 161, 191, 192)
GJ_KINDS = ("random", "perm", "tie")


def gj_blocks(m, kind, nsrc=5):
    """nsrc m x m matrices.
    random: uniform entries + a diagonal shift (well conditioned)
    perm:   a random permutation with no fixed point + 0.1 noise off its support and a zero
            diagonal: every step must pivot
    tie:    random, but column 0 holds the same largest magnitude in two rows, and the higher
            of the two rows is scaled by 1e6 elsewhere: taking it as the first pivot adds
            1e6-sized multiples to every row (six digits lost); the lower row must win"""
    seed = {"random": 1, "perm": 2, "tie": 3}[kind] * 1000 + m
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nsrc):
        if kind == "perm" and m > 1:
            while True:
                p = rng.permutation(m)
                if not np.any(p == np.arange(m)):
                    break
            A = 0.1 * rng.uniform(-1.0, 1.0, (m, m)) / max(1.0, m / 8.0)
            A[np.arange(m), np.arange(m)] = 0.0
            A[np.arange(m), p] = rng.choice([-1.0, 1.0], m) * rng.uniform(1.0, 2.0, m)
        else:
            A = rng.uniform(-1.0, 1.0, (m, m))
            A[np.arange(m), np.arange(m)] += 0.5 * np.sqrt(m) * rng.choice([-1.0, 1.0], m)
            if kind == "tie" and m > 2:
                lo, hi = sorted(rng.choice(m, 2, replace=False))
                A[:, 0] = rng.uniform(-0.5, 0.5, m)
                A[hi, 1:] *= 1e6
                A[lo, 0], A[hi, 0] = 2.0, -2.0
        out.append(A)
    return np.stack(out)


# ---------------------------------------------------------------- band matrices
# (N, bl, bu, seed); the seeds are those for which LAPACK's pivots show a pivot row below its
# panel of 16 columns and two steps of one panel choosing rows below it (test_cr_ref.py)
BAND_CASES = [(1, 1, 1, 0), (15, 3, 3, 0), (16, 3, 3, 0), (17, 3, 3, 4), (33, 5, 2, 0), (33, 2, 7, 3),
              (100, 17, 17, 0), (257, 40, 40, 0), (500, 230, 230, 0), (500, 240, 240, 0)]
BAND_STAGE_O = {(500, 240, 240): 0}
BAND_NBP = 16


def build_band(N, bl, bu, seed):
    """dense N x N with uniform (-1, 1) entries inside the band, the diagonal no larger than the
    rest (pivots move)"""
    rng = np.random.default_rng(100000 + 1000 * N + 10 * bl + bu + 7 * seed)
    A = rng.uniform(-1.0, 1.0, (N, N))
    i, j = np.indices((N, N))
    A[(j - i > bu) | (i - j > bl)] = 0.0
    return A


def band_rows(A, bl, bu):
    """the device layout: row i holds A(i, j) at j - i + bl, width 2 bl + bu + 1"""
    N = A.shape[0]
    ab = np.zeros((N, 2 * bl + bu + 1))
    for i in range(N):
        for j in range(max(0, i - bl), min(N, i + bu + 1)):
            ab[i, j - i + bl] = A[i, j]
    return ab


def band_lapack(A, bl, bu):
    """dgbtrf of A -> (lu (2 bl + bu + 1, N), piv 0-based, info)"""
    N = A.shape[0]
    ab = np.zeros((2 * bl + bu + 1, N), order="F")
    for j in range(N):
        for i in range(max(0, j - bu), min(N, j + bl + 1)):
            ab[bl + bu + i - j, j] = A[i, j]
    lu, piv, info = lapack.dgbtrf(ab, bl, bu)
    return lu, piv, info


def band_u_rows(lu, bl, bu):
    """LAPACK's U in the device layout (row i, columns i .. i + bl + bu at offset bl ..)"""
    N = lu.shape[1]
    U = np.zeros((N, bl + bu + 1))
    for i in range(N):
        for j in range(i, min(N, i + bl + bu + 1)):
            U[i, j - i] = lu[bl + bu + i - j, j]
    return U


def band_pivot_facts(piv, N):
    """(a pivot row lies below its panel, two steps of one panel chose rows below it,
    two steps of one panel chose the same row below it)"""
    below = two = shared = False
    for k0 in range(0, N, BAND_NBP):
        nbk = min(BAND_NBP, N - k0)
        rows = [int(p) for p in piv[k0:k0 + nbk] if p >= k0 + nbk]
        below |= len(rows) >= 1
        two |= len(rows) >= 2
        shared |= len(rows) != len(set(rows))
    return below, two, shared


@functools.lru_cache(maxsize=None)
def band_system(N, bl, bu, seed):
    """(A, lu, piv, X* longdouble, err_ref of dgbtrs on the identity)"""
    A = build_band(N, bl, bu, seed)
    lu, piv, info = band_lapack(A, bl, bu)
    assert info == 0
    Xl, info = lapack.dgbtrs(lu, bl, bu, np.eye(N), piv)
    assert info == 0
    Xs = refined_inverse(A)
    for a in (A, lu, piv, Xs):
        a.setflags(write=False)
    return A, lu, piv, Xs, rel_err(Xl, Xs)
