"""CPU reference for the thick-restarted (Krylov-Schur) stability analysis (csrc/eigs.hip,
iemic/eigs.py, iemic/krylov_schur.py), written without the code under test.

* ``restarted_twin``: ``eig_ref.arnoldi_twin`` with thick restarts over the oracle's J and B, run
  with the exact deflated inverse or with the oracle's inexact solve.  Where the package builds
  its orthonormal basis of the kept invariant subspace from a QR of eigenvectors, the twin takes
  the leading columns of an ordered real Schur form (``scipy.linalg.schur`` with a modulus
  threshold, which cannot split a conjugate pair): another route to the same subspace.
* ``make_fixture``: what tests/golden/eigs_restart_natl8.npz holds; ``python
  tests/eig_restart_ref.py`` rewrites it.  Per shift: ``m_small``, the smallest even m >= k + 4 at
  which the unrestarted exact twin has not converged all wanted pairs in m steps (asserted here,
  and at most half the unrestarted step count of eigs_natl8.npz), the restarted twins' results
  at that m, and ``R``, twice the restart count the inexact twin needed.
"""
import os
import sys

import numpy as np

import eig_ref as er

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "eigs_restart_natl8.npz")

MAX_KEEP = 16
MAX_RESTARTS = 400          # of the twins, when the fixture is written


def default_keep(k, m):
    return min(k + 3, m - 1, MAX_KEEP)


def wanted_general(R, j, k):
    """eig_ref.wanted with the estimate of a full last row: |R[j, :j] . y| / |theta|"""
    return [(t, y, abs(R[j, :j] @ y) / abs(t), cnt) for t, y, _, cnt in er.wanted(R, j, k)]


def schur_restart(R, j, keep):
    """(Q, [[S], [b^T]]): the `keep` largest-modulus eigenvalues of G = R[:j, :j] (a pair whole:
    one more, or one fewer at the cap min(16, j - 1)) ordered first in a real Schur form G = Z T Z^T"""
    import scipy.linalg as sla
    G = R[:j, :j]
    mod = np.sort(np.abs(np.linalg.eigvals(G)))[::-1]
    cap = min(MAX_KEEP, j - 1)
    p = keep
    split = lambda q: abs(mod[q - 1] - mod[q]) <= 1e-12 * mod[q - 1]     # a pair shares its modulus
    if split(p):
        p = p + 1 if p + 1 <= cap and not split(p + 1) else p - 1
    assert 1 <= p <= cap and not split(p)
    thresh = np.sqrt(mod[p - 1] * mod[p])
    T, Z, sdim = sla.schur(G, output="real", sort=lambda re, im: np.hypot(re, im) > thresh)
    assert sdim == p, (sdim, p)
    Q = np.ascontiguousarray(Z[:, :p])
    out = np.zeros((p + 1, p))
    out[:p] = T[:p, :p]
    out[p] = R[j, :j] @ Q
    return Q, out


def restarted_twin(solve, B, v0, sigma, k, m, tol, restarts, keep=None):
    """-> dict(lam, X (columns), estimate, steps (inner solves), restarts, breakdown): lam sorted
    as eig_ref.arnoldi_twin's"""
    keep = default_keep(k, m) if keep is None else keep
    N = v0.size
    V = np.zeros((m + 1, N))
    R = np.zeros((m + 1, m))
    W = er.not_p_rows(N)
    V[0] = v0 / np.linalg.norm(W * v0)
    j, solves, nrest, broke, g = 0, 0, 0, False, []
    while True:
        done = False
        while j < m:
            w = solve(B * V[j])
            solves += 1
            for _ in range(2):                          # two classical Gram-Schmidt passes
                h = V[:j + 1] @ (W * w)
                w = w - V[:j + 1].T @ h
                R[:j + 1, j] += h
            hn = np.linalg.norm(W * w)
            R[j + 1, j] = hn
            if hn <= 1e-14 * np.linalg.norm(R[:j + 2, j]):
                broke = True
            else:
                V[j + 1] = w / hn
            j += 1
            if j >= k or broke:
                g = wanted_general(R, j, k)
                if broke or all(e[2] <= tol for e in g):
                    done = True
                    break
        if done or nrest >= restarts:
            break
        Q, S = schur_restart(R, j, keep)
        p = Q.shape[1]
        last = V[j].copy()
        V[:p] = Q.T @ V[:j]
        V[p] = last
        V[p + 1:] = 0.0
        R[:] = 0.0
        R[:p + 1, :p] = S
        j, nrest = p, nrest + 1
    lam, X, est = [], [], []
    for t, y, e, cnt in g:
        lm = sigma + 1.0 / t
        x = V[:j].T @ y
        for s in ((1, -1) if cnt == 2 else (1,)):
            lam.append(complex(lm.real, s * lm.imag))
            X.append(x if s == 1 else np.conj(x))
            est.append(e)
    return dict(lam=np.array(lam), X=np.array(X).T, estimate=np.array(est), steps=solves, restarts=nrest,
                breakdown=broke)


def smallest_unconverged_m(solve, B, v0, sigma):
    """the smallest even m >= k + 4 at which the unrestarted exact twin misses tol on a wanted pair"""
    m = er.K + 4
    m += m % 2
    while True:
        r = er.arnoldi_twin(solve, B, v0, sigma, m=m)
        if not r["breakdown"] and np.any(r["estimate"] > er.TOL):
            return m, float(r["estimate"].max())
        m += 2


def run_case(orc, q, sysd, base):
    """both restarted twins at shift q; base: eigs_natl8.npz"""
    c, o, L, x, val, B, diag = sysd
    sigma = er.SIGMAS[q]
    vs = er.shifted_val(val, B, diag, sigma)
    As = er.csr(o, vs)
    Jinv, _ = er.deflated_inverse(As.toarray())
    lam_ref = base[f"s{q}_lam_dense"]
    v0 = er.start_vector(o.N)
    exact = lambda b: Jinv @ b
    m_small, worst = smallest_unconverged_m(exact, B, v0, sigma)
    assert worst > er.TOL, "the unrestarted exact twin converged at m_small"
    assert 2 * m_small <= int(base[f"s{q}_exact_steps"]), (m_small, int(base[f"s{q}_exact_steps"]))
    ex = restarted_twin(exact, B, v0, sigma, er.K, m_small, er.TOL, MAX_RESTARTS)
    solve, its = er.inexact_solver(orc, o, vs)
    ix = restarted_twin(solve, B, v0, sigma, er.K, m_small, er.TOL, MAX_RESTARTS)
    for r in (ex, ix):
        assert np.all(r["estimate"] <= er.TOL) and r["restarts"] >= 1 and not r["breakdown"]
        r["residual"] = np.array([er.true_residual(As, B, sigma, l, r["X"][:, i]) for i, l in enumerate(r["lam"])])
        r["deviation"] = er.nearest_deviation(r["lam"], lam_ref, sigma)
    return dict(m_small=m_small, unrestarted_worst_estimate=worst, exact=ex, inexact=ix)


def make_fixture(orc):
    with np.load(er.FIXTURE, allow_pickle=False) as z:
        base = {key: z[key] for key in z.files}
    out = {"sigmas": np.array(er.SIGMAS), "k": er.K, "tol": er.TOL, "inner_tol": er.INNER_TOL, "seed": er.SEED}
    sysd = er.system(orc)
    for q in range(len(er.SIGMAS)):
        r = run_case(orc, q, sysd, base)
        out[f"s{q}_m_small"] = r["m_small"]
        out[f"s{q}_unrestarted_worst_estimate"] = r["unrestarted_worst_estimate"]
        out[f"s{q}_R"] = 2 * r["inexact"]["restarts"]
        for kind in ("exact", "inexact"):
            t = r[kind]
            out[f"s{q}_{kind}_lam"] = t["lam"]
            out[f"s{q}_{kind}_steps"] = t["steps"]
            out[f"s{q}_{kind}_restarts"] = t["restarts"]
            out[f"s{q}_{kind}_worst_residual"] = t["residual"].max()
            out[f"s{q}_{kind}_worst_deviation"] = t["deviation"].max()
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "i-emic_amd"))
    sys.path.insert(0, HERE)
    from oracle import oracle as orc
    fx = make_fixture(orc)
    np.savez(FIXTURE, **fx)
    for key, v in fx.items():
        print(key, v)
