"""The host algebra of the thick restart (iemic/krylov_schur.py, iemic.eigs.rayleigh_groups) on a
dense matrix, without the device library: a seeded numpy Arnoldi is restarted with the package's
functions until its k = 4 dominant Ritz values are numpy.linalg.eigvals' dominant eigenvalues.

A = X D X^-1, n = 200, X = I + 0.1 randn / sqrt(n) (condition number about 1.5), D block diagonal:
10, 8 +- 3i, 7 (the four wanted: one pair among them), 6 +- 2i, nine real values 5.5 .. 3.0, the
pair 2.5 +- 1.5i, and the rest inside radius 2.  Where the boundary falls is decided by the Ritz
values of the moment, not by D, so every restart is checked for the rule (no pair split, at
most one away from keep, never above the cap) and the cases are those in which both moves
occur: m = 12, keep = 5 grows to 6 in some restarts, m = 12, keep = 6 never moves, and m = 20 with
keep at the cap of 16 shrinks to 15 in some.

Bounds.  u = 2^-53, |.| the Frobenius norm, j the length before the restart, p after.
  Q^T Q = I: Householder QR of a j x p matrix, |Q^T Q - I| <= 10 j p u (Higham, Accuracy and
    Stability, Thm 19.4 with its constant taken as 10).
  E = A V' - V' S - v b^T has three parts.
    (a) The Arnoldi relation itself, carried through exactly by the orthonormal Q: per column one
        product fl(A v) (gamma_n |A|), two Gram-Schmidt passes of n-long dots and (j+1)-long
        updates (2 (gamma_n + gamma_{j+1}) |A|) and the scaling (u |A|): (3 n + 2 j + 3) u |A|, so
        sqrt(j) (3 n + 2 j + 3) u |A| over j columns.  Columns inherited from an earlier restart
        carry that restart's E instead, which the same bound covers; so (a) is taken once per
        restart so far.
    (b) The span of Q is invariant only up to numpy.linalg.eig's residual: with C the real columns
        the package orthogonalises, G C = C L + F, |F| <= 10 j u |G| sqrt(p) (backward stability of
        the QR algorithm, constant 10), and (I - Q Q^T) G Q = (I - Q Q^T) F R^-1 is at most
        |F| / sigma_min(C).  sigma_min(C) is computed here from numpy.linalg.eig of the same G.
    (c) This test's own products A V', V' S, V_j Q in fp64: (gamma_n + 2 gamma_j) |A| sqrt(p).
  Eigenvalues: Bauer-Fike, |theta - lambda| <= kappa(X) |r|, |r| = estimate |theta|, plus the dense
    solver's kappa(X) n u |A|; twice that for the second-order terms (as tests/test_eig_ref.py).
"""
import numpy as np
import pytest

from iemic import eigs as ie
from iemic import krylov_schur as ks

U = 2.0 ** -53
N, K, TOL = 200, 4, 1e-11


def matrix():
    rng = np.random.default_rng(2024)
    blocks = [10.0, (8.0, 3.0), 7.0, (6.0, 2.0), 5.5, 5.0, 4.5, 4.0, 3.8, 3.6, 3.4, 3.2, 3.0, (2.5, 1.5)]
    D = np.zeros((N, N))
    i = 0
    for b in blocks:
        if isinstance(b, tuple):
            D[i:i + 2, i:i + 2] = [[b[0], b[1]], [-b[1], b[0]]]
            i += 2
        else:
            D[i, i] = b
            i += 1
    D[i, i] = 1.0
    i += 1
    while i < N:                                    # the rest: pairs of modulus below 2
        r, a = rng.uniform(0.1, 1.9), rng.uniform(0, np.pi)
        D[i:i + 2, i:i + 2] = r * np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
        i += 2
    X = np.eye(N) + 0.1 * rng.standard_normal((N, N)) / np.sqrt(N)
    return X @ D @ np.linalg.inv(X), np.linalg.cond(X), rng.standard_normal(N)


def extend(A, V, R, j0, m):
    """Arnoldi steps j0 .. m - 1: two classical Gram-Schmidt passes against all j + 1 vectors"""
    for j in range(j0, m):
        w = A @ V[:, j]
        for _ in range(2):
            h = V[:, :j + 1].T @ w
            w = w - V[:, :j + 1] @ h
            R[:j + 1, j] += h
        R[j + 1, j] = np.linalg.norm(w)
        V[:, j + 1] = w / R[j + 1, j]


def sigma_min_of_kept(G, p):
    """sigma_min of the real columns (Re, Im per pair) of the p dominant eigenvectors of G"""
    th, Y = np.linalg.eig(G)
    idx = np.argsort(-np.abs(th), kind="stable")[:p]
    cols = []
    for i in idx:
        if th[i].imag == 0:
            cols.append(Y[:, i].real)
        elif th[i].imag > 0:
            cols += [Y[:, i].real, Y[:, i].imag]
    assert len(cols) == p, "the p dominant Ritz values split a pair"
    return np.linalg.svd(np.stack(cols, axis=1), compute_uv=False)[-1]


@pytest.mark.parametrize("m,keep,sizes_want", [(12, 5, {5, 6}), (12, 6, {6}), (20, 16, {15, 16})])
def test_restart_until_converged(m, keep, sizes_want):
    A, condX, v0 = matrix()
    nA = np.linalg.norm(A)
    lam = np.linalg.eigvals(A)
    lam = lam[np.argsort(-np.abs(lam), kind="stable")]
    V, R = np.zeros((N, m + 1)), np.zeros((m + 1, m))
    V[:, 0] = v0 / np.linalg.norm(v0)
    extend(A, V, R, 0, m)
    sizes, worst, groups = [], 0.0, []
    for nrest in range(1, 61):
        Q, Rn = ks.restart(R, m, keep)
        p = Q.shape[1]
        sizes.append(p)
        assert Q.shape == (m, p) and Rn.shape == (p + 1, p)
        assert abs(p - keep) <= 1 and p <= min(ks.MAX_KEEP, m - 1)
        assert np.linalg.norm(Q.T @ Q - np.eye(p)) <= 10 * m * p * U
        # the kept Ritz values are the p dominant ones of G, pairs whole
        th = np.linalg.eigvals(R[:m, :m])
        th = th[np.argsort(-np.abs(th), kind="stable")]
        kept = np.linalg.eigvals(Rn[:p])
        assert np.all(np.min(np.abs(kept[:, None] - th[None, :p]), axis=1) <= 1e-9 * np.abs(th[0]))
        assert p == m - 1 or abs(abs(th[p - 1]) - abs(th[p])) > 1e-9 * abs(th[p]), "a pair was split"
        smin = sigma_min_of_kept(R[:m, :m], p)
        Vn = V[:, :m] @ Q
        v = V[:, m].copy()
        E = A @ Vn - Vn @ Rn[:p] - np.outer(v, Rn[p])
        bound = U * (nrest * np.sqrt(m) * (3 * N + 2 * m + 3) * nA
                     + 10 * m * np.linalg.norm(R[:m, :m]) * np.sqrt(p) / smin
                     + (N + 2 * m) * nA * np.sqrt(p))
        worst = max(worst, np.linalg.norm(E) / bound)
        assert np.linalg.norm(E) <= bound
        V[:, :p], V[:, p], V[:, p + 1:] = Vn, v, 0.0
        R[:] = 0.0
        R[:p + 1, :p] = Rn
        extend(A, V, R, p, m)
        groups = ie.rayleigh_groups(R, m, K)
        if all(g[2] <= TOL for g in groups):
            break
    print(f"m {m} keep {keep}: {nrest} restarts, kept sizes {sorted(set(sizes))}, worst |E| / bound {worst:.3f}")
    assert all(g[2] <= TOL for g in groups), "not converged in 60 restarts"
    assert set(sizes) == sizes_want
    got = []
    for t, y, est, cnt in groups:
        got += [t, np.conj(t)] if cnt == 2 else [t]
    assert len(got) == K
    for t in got:
        d = np.abs(lam[:K] - t)
        assert d.min() <= 2 * condX * (TOL * abs(t) + N * U * nA)
    assert sorted(int(np.argmin(np.abs(lam[:K] - t))) for t in got) == list(range(K))


def test_general_estimate_on_a_hessenberg_matrix():
    """g = h_{j+1,j} e_j: |g . y| / |theta| is |h_{j+1,j}| |y_j| / |theta| up to the rounding of one
    complex modulus taken before or after the product (4 u relative)"""
    rng = np.random.default_rng(5)
    j = 12
    H = np.triu(rng.standard_normal((j + 1, j)), -1)
    a, b = ie.ritz_groups(H, j, 6), ie.rayleigh_groups(H, j, 6)
    assert len(a) == len(b) >= 3
    for (t0, y0, e0, c0), (t1, y1, e1, c1) in zip(a, b):
        assert t0 == t1 and c0 == c1 and np.array_equal(y0, y1)
        assert abs(e0 - e1) <= 4 * U * e0
    assert ks.general_estimate(H, j, 0.0, a[0][1]) == np.inf


def test_selection_rules():
    th = np.array([5.0, 3 + 1j, 3 - 1j, 2.0, 1 + 1j, 1 - 1j, 0.5])
    assert list(ks.select_kept(th, 1, 6)) == [0]
    assert sorted(ks.select_kept(th, 2, 6)) == [0, 1, 2]            # grown by one
    assert sorted(ks.select_kept(th, 2, 2)) == [0]                  # shrunk by one at the cap
    assert sorted(ks.select_kept(th, 5, 6)) == [0, 1, 2, 3, 4, 5]
    assert ks.default_keep(6, 40) == 9 and ks.default_keep(6, 8) == 7 and ks.default_keep(15, 64) == 16
    for keep, cap in ((0, 3), (4, 3), (3, 7)):
        with pytest.raises(ValueError, match="select_kept"):
            ks.select_kept(th, keep, cap)
    with pytest.raises(ValueError, match="does not fit"):
        ks.select_kept(np.array([1 + 1j, 1 - 1j, 0.1]), 1, 1)
