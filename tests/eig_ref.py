"""CPU references for the stability analysis (csrc/eigs.hip, iemic/eigs.py), written without
the code under test.

* ``arnoldi_twin``: a numpy twin of the shift-invert Arnoldi loop over the oracle's J and B,
  run with any solve: the deflated dense inverse below (exact) or the oracle's preconditioned ``BlockGS.fgmres``
  (inexact, at the inner tolerance the GPU test uses).
* ``dense_reference``: the eigenvalues of ``(J - sigma B)^-1 diag(B)`` mapped by
  ``lambda = sigma + 1 / theta``, keeping ``|theta| > 1e-12``.  (Dense QZ on (J, B) is not
  accurate enough on this ill-scaled J to serve as the reference.)
* ``deflated_inverse``: the "exact" inverse both of the above use.  THCM's Jacobian is singular:
  natl8 has two null vectors, the pressure modes the block Gauss-Seidel preconditioner pins.
  Right and left null vectors live in the P rows, where B = 0, so ``B v`` is always in the range
  of ``J - sigma B`` and a null component of the solution is annihilated by the next ``B``: the
  finite eigenvalues are well defined, but a plain dense LU divides by a pivot of rounding size
  and returns four spurious |theta| ~ 1e7.  The inverse here is the pseudo-inverse from the SVD
  with the singular values below 1e-11 of the largest dropped (natl8: 4.7e-15 and 1.4e-16 against
  a next-smallest of 2.1e-3).
* ``make_fixture``: what tests/golden/eigs_natl8.npz holds (natl8 at both shifts, and the
  inexact twin's gateway16 run); ``python tests/eig_ref.py`` rewrites it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "eigs_natl8.npz")

NAME = "natl8"
K, M, TOL = 6, 40, 1e-8
INNER_TOL = 1e-10           # "FGMRES tolerance" of the GPU runs: 100 times tighter than TOL
SEED = 1
SIGMAS = (0.0, 0.02)        # 0 and a positive shift of the order of the smallest |lambda| (0.0206)


def system(orc, name=NAME):
    """(cfg, oracle, L, x, val, B, diag positions) of `name` at cf.synthetic_state"""
    from iemic import config as cf
    from helpers import mask_fix
    c = cf.preset(name)
    L = mask_fix(orc, c, cf.landmask(c).reshape(c.l + 2, c.m + 2, c.n + 2))
    o = orc.Oracle(c.ref_dict(), L, c.par_list())
    x = cf.synthetic_state(c, L)
    val, B = o.jacobian(x)
    rows = np.repeat(np.arange(o.N), np.diff(o.rowptr))
    diag = np.flatnonzero(o.col == rows)
    assert diag.size == o.N
    return c, o, L, x, val, B, diag


def shifted_val(val, B, diag, sigma):
    """val with -(sigma B) added on the diagonal where B != 0; every other entry keeps its bits"""
    out = val.copy()
    hit = B != 0
    out[diag[hit]] = val[diag[hit]] + -(sigma * B[hit])
    return out


def csr(o, val):
    import scipy.sparse as sp
    return sp.csr_matrix((val, o.col, o.rowptr), shape=(o.N, o.N))


def deflated_inverse(Js):
    """(pseudo-inverse of Js without its numerical null space, the null space's dimension)"""
    U, s, Vt = np.linalg.svd(Js)
    keep = s > 1e-11 * s[0]
    return (Vt[keep].T / s[keep]) @ U[:, keep].T, int(np.count_nonzero(~keep))


def dense_reference(Jinv, B, sigma):
    """finite eigenvalues from the shift-inverted matrix: (lambda, theta), |theta| descending"""
    th = np.linalg.eigvals(Jinv * B[None, :])
    th = th[np.abs(th) > 1e-12]
    th = th[np.argsort(-np.abs(th), kind="stable")]
    return sigma + 1.0 / th, th


def start_vector(N, seed=SEED):
    """the device's start vector: the shadow-space hash of the global row, normalised"""
    from krylov_ref import idr_shadow_raw
    v = idr_shadow_raw(np.arange(N), 1, seed)[:, 0]
    return v / np.linalg.norm(v)


def not_p_rows(N):
    """1 on the U, V, W, T, S rows, 0 on the P rows: the weights of the loop's inner products.
    An iterative inner solve leaves an arbitrary multiple of the Jacobian's null vectors (P rows
    only) in every w; measured in the plain 2-norm that multiple enters H and shows up as a
    spurious converged Ritz value whose vector has B x = 0 (seen with the CPU twin on gateway16
    in one run of three).  B vanishes on the P rows, so the operator never reads them: Arnoldi
    with the P rows left out of every dot product is Arnoldi on the same operator restricted
    to the other rows, with the same non-zero eigenvalues, and cannot see the null vectors."""
    q = np.ones(N)
    q[3::6] = 0.0
    return q


def wanted(H, j, k):
    """the k largest-|theta| Ritz pairs of H[:j, :j], a conjugate pair kept whole:
    [(theta with imag <= 0, so that lambda = sigma + 1 / theta has imag >= 0, unit y, estimate,
    multiplicity 1 | 2)], |theta| descending"""
    th, Y = np.linalg.eig(H[:j, :j])
    hn = abs(H[j, j - 1])
    done, groups = np.zeros(j, dtype=bool), []
    for i in range(j):
        if done[i]:
            continue
        done[i] = True
        if abs(th[i].imag) > 0:
            mate = [q for q in range(j) if not done[q] and th[q] == np.conj(th[i])]
            assert mate, "a complex Ritz value of a real matrix without its conjugate"
            done[mate[0]] = True
            q = i if th[i].imag < 0 else mate[0]
            groups.append((th[q], Y[:, q], 2))
        else:
            groups.append((complex(th[i].real), Y[:, i], 1))
    groups.sort(key=lambda g: -abs(g[0]))
    out, n = [], 0
    for t, y, cnt in groups:
        if n >= k:
            break
        y = y / np.linalg.norm(y)
        out.append((t, y, hn * abs(y[j - 1]) / abs(t), cnt))
        n += cnt
    return out


def arnoldi_twin(solve, B, v0, sigma, k=K, m=M, tol=TOL):
    """-> dict(lam, X (columns), estimate, steps, breakdown): lam sorted by |lam - sigma|
    ascending, a conjugate pair adjacent with the positive imaginary part first"""
    N = v0.size
    V = np.zeros((m + 1, N))
    H = np.zeros((m + 1, m))
    Q = not_p_rows(N)
    V[0] = v0 / np.linalg.norm(Q * v0)
    steps, broke, g = 0, False, []
    for j in range(m):
        w = solve(B * V[j])
        for _ in range(2):                          # two classical Gram-Schmidt passes
            h = V[:j + 1] @ (Q * w)
            w = w - V[:j + 1].T @ h
            H[:j + 1, j] += h
        hn = np.linalg.norm(Q * w)
        H[j + 1, j] = hn
        steps = j + 1
        if hn <= 1e-14 * np.linalg.norm(H[:j + 2, j]):
            broke = True
        else:
            V[j + 1] = w / hn
        if steps >= k or broke:
            g = wanted(H, steps, k)
            if broke or all(e[2] <= tol for e in g):
                break
    lam, X, est = [], [], []
    for t, y, e, cnt in g:
        lm = sigma + 1.0 / t
        x = V[:steps].T @ y
        for s in ((1, -1) if cnt == 2 else (1,)):
            lam.append(complex(lm.real, s * lm.imag))
            X.append(x if s == 1 else np.conj(x))
            est.append(e)
    return dict(lam=np.array(lam), X=np.array(X).T, estimate=np.array(est), steps=steps, breakdown=broke)


def true_residual(A, B, sigma, lam, x):
    """||(J - sigma B) x - (lam - sigma) B x|| / ||(J - sigma B) x||, A = J - sigma B (any matvec)"""
    a = A @ x
    return np.linalg.norm(a - (lam - sigma) * (B * x)) / np.linalg.norm(a)


def true_residual_extended(o, val_s, B, sigma, lam, x):
    """true_residual of the same fp64 data in numpy's extended precision (val_s: the CSR values
    of J - sigma B).  A pair converged to 1e-10 has a residual ten orders below its two terms,
    so fp64's rounding of the matrix product alone, a few u |J| |x| (about 3e-15 of ||a|| on
    natl8), is 1e-5 of it: a reference for a 1e-6 relative comparison needs the wider format.
    With u = 2^-64 the same rounding is below 1e-8 of such a residual."""
    ld, cld = np.longdouble, np.clongdouble
    assert np.finfo(ld).eps <= 2.0 ** -63, "numpy's longdouble is no wider than fp64 here"
    rowptr = np.asarray(o.rowptr, dtype=np.int64)
    assert np.all(np.diff(rowptr) > 0)
    prod = np.asarray(val_s).astype(ld) * np.asarray(x).astype(cld)[np.asarray(o.col)]
    a = np.add.reduceat(prod, rowptr[:-1])
    mu = cld(complex(lam)) - ld(sigma)
    r = a - mu * (B.astype(ld) * np.asarray(x).astype(cld))
    nrm = lambda v: np.sqrt(np.sum(v.real * v.real + v.imag * v.imag))
    return float(nrm(r) / nrm(a))


def nearest_deviation(lam, ref, sigma):
    """per lam: min over the reference of |lam - ref| / |ref - sigma|"""
    return np.array([np.min(np.abs(l - ref) / np.abs(ref - sigma)) for l in lam])


def inexact_solver(orc, o, val_s, tol=INNER_TOL):
    gs = orc.BlockGS(o, val_s, 3, dyn_iters=4, dyn_omega=0.95, ts_mg=1)
    its = []

    def solve(b):
        x, it, rel, _ = gs.fgmres(b, tol=tol, m=500, maxit=500)
        its.append(it)
        return x

    return solve, its


def run_case(orc, sigma, sysd=None):
    """both twins and the dense reference at one shift"""
    c, o, L, x, val, B, diag = sysd or system(orc)
    vs = shifted_val(val, B, diag, sigma)
    As = csr(o, vs)
    Js = As.toarray()
    Jinv, nnull = deflated_inverse(Js)
    lam_ref, th_ref = dense_reference(Jinv, B, sigma)
    v0 = start_vector(o.N)
    ex = arnoldi_twin(lambda b: Jinv @ b, B, v0, sigma)
    solve, its = inexact_solver(orc, o, vs)
    ix = arnoldi_twin(solve, B, v0, sigma)
    for r in (ex, ix):
        r["residual"] = np.array([true_residual(As, B, sigma, l, r["X"][:, q]) for q, l in enumerate(r["lam"])])
        r["deviation"] = nearest_deviation(r["lam"], lam_ref, sigma)
    ix["iters"] = its
    return dict(sigma=sigma, lam_ref=lam_ref, exact=ex, inexact=ix, nnull=nnull)


def make_fixture(orc):
    out = {"sigmas": np.array(SIGMAS), "k": K, "m": M, "tol": TOL, "inner_tol": INNER_TOL, "seed": SEED}
    sysd = system(orc)
    for q, s in enumerate(SIGMAS):
        r = run_case(orc, s, sysd)
        n = len(r["exact"]["lam"])
        out[f"s{q}_lam_dense"] = r["lam_ref"][:max(n, 16)]
        for kind in ("exact", "inexact"):
            t = r[kind]
            out[f"s{q}_{kind}_lam"] = t["lam"]
            out[f"s{q}_{kind}_steps"] = t["steps"]
            out[f"s{q}_{kind}_worst_residual"] = t["residual"].max()
            out[f"s{q}_{kind}_worst_deviation"] = t["deviation"].max()
    out.update(gateway_case(orc))
    return out


GW_NAME, GW_SIGMA, GW_K = "gateway16", 0.02, 4


def gateway_case(orc):
    """gateway16 (N = 24,576: no dense reference fits): the inexact-solve twin alone, k = 4"""
    c, o, L, x, val, B, diag = system(orc, GW_NAME)
    vs = shifted_val(val, B, diag, GW_SIGMA)
    As = csr(o, vs)
    solve, its = inexact_solver(orc, o, vs)
    r = arnoldi_twin(solve, B, start_vector(o.N), GW_SIGMA, k=GW_K)
    res = np.array([true_residual(As, B, GW_SIGMA, l, r["X"][:, q]) for q, l in enumerate(r["lam"])])
    return {"gw_sigma": GW_SIGMA, "gw_k": GW_K, "gw_lam": r["lam"], "gw_steps": r["steps"],
            "gw_estimate": r["estimate"], "gw_worst_residual": res.max()}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "i-emic_amd"))
    sys.path.insert(0, HERE)
    from oracle import oracle as orc
    fx = make_fixture(orc)
    np.savez(FIXTURE, **fx)
    for key, v in fx.items():
        print(key, v)
