"""The host algebra of the thick (Krylov-Schur) restart of ``iemic.eigs``: numpy only, no device.

After j steps an Arnoldi run holds ``A V_j = V_j G + v_{j+1} g^T`` with the (j + 1) x j Rayleigh
matrix ``R = [[G], [g^T]]``: upper Hessenberg with ``g = h_{j+1,j} e_j`` until the first restart,
full afterwards.  For an orthonormal Q (j x p) whose span is invariant under G, ``G Q = Q S``
with ``S = Q^T G Q``, and multiplying the decomposition by Q gives

    A (V_j Q) = (V_j Q) S + v_{j+1} (Q^T g)^T,

a decomposition of the same kind of length p: the basis ``[V_j Q, v_{j+1}]`` is orthonormal, the
new Rayleigh matrix is ``[[S], [b^T]]`` with ``b = Q^T g``, and the next Arnoldi step
orthogonalises against all p + 1 vectors and appends a full column.  The Ritz values of S are
the kept Ritz values of G; what the dropped directions carried is gone, nothing else changes.

A Ritz pair (theta, y) of the leading block has the residual ``A V y - theta V y = v_{j+1} (g . y)``,
so its estimate is ``|g . y| / |theta|``, which for a Hessenberg matrix is the familiar
``|h_{j+1,j}| |e_j^T y| / |theta|``.
"""
from __future__ import annotations

import numpy as np

__all__ = ["MAX_KEEP", "default_keep", "general_estimate", "select_kept", "invariant_basis", "compress", "restart"]

MAX_KEEP = 16               # iemic_eigs_restart compresses onto at most 16 vectors in its one pass


def default_keep(k: int, m: int) -> int:
    """k + 3, capped so that keep < m and keep <= MAX_KEEP"""
    return min(k + 3, m - 1, MAX_KEEP)


def general_estimate(R: np.ndarray, j: int, theta: complex, y: np.ndarray) -> float:
    """``|R[j, :j] . y| / |theta|`` for a pair (theta, y) of R[:j, :j], y of unit norm"""
    if not abs(theta) > 0:
        return np.inf
    return float(abs(R[j, :j] @ y) / abs(theta))


def select_kept(th: np.ndarray, keep: int, cap: int) -> np.ndarray:
    """Indices into th (the eigenvalues of a real matrix) of the `keep` largest |theta|, a
    conjugate pair never split: one more when the keep-th and the next are a pair, one fewer
    when that would exceed `cap`.  Sorted by |theta| descending, the members of a pair adjacent."""
    n = len(th)
    if not 1 <= keep <= cap < n:
        raise ValueError(f"select_kept: needs 1 <= keep = {keep} <= cap = {cap} < {n} Ritz values")
    done, groups = np.zeros(n, dtype=bool), []
    for i in range(n):
        if done[i]:
            continue
        done[i] = True
        if th[i].imag != 0.0:
            mate = [q for q in range(n) if not done[q] and th[q] == np.conj(th[i])]
            if not mate:
                raise ValueError("select_kept: a complex Ritz value without its conjugate")
            done[mate[0]] = True
            groups.append((i, mate[0]))
        else:
            groups.append((i,))
    groups.sort(key=lambda g: -abs(th[g[0]]))
    sel = []
    for g in groups:
        if len(sel) >= keep:
            break
        sel.extend(g)
    if len(sel) > cap:
        sel = sel[:-2]
    if not sel:
        raise ValueError("select_kept: the leading conjugate pair does not fit under the cap")
    return np.array(sel, dtype=int)


def invariant_basis(sel: np.ndarray, th: np.ndarray, Y: np.ndarray) -> np.ndarray:
    """An orthonormal real basis Q (j x p) of the invariant subspace spanned by the eigenvectors
    Y[:, sel] of the eigenvalues th[sel] of a real matrix (pairs whole): the Householder QR factor
    of their real parts and, from the member of a pair with imag > 0, imaginary parts."""
    cols = []
    for i in sel:
        if th[i].imag == 0.0:
            cols.append(Y[:, i].real)
        elif th[i].imag > 0.0:
            cols.append(Y[:, i].real)
            cols.append(Y[:, i].imag)
    Q, _ = np.linalg.qr(np.stack(cols, axis=1))
    return np.ascontiguousarray(Q)


def compress(R: np.ndarray, j: int, Q: np.ndarray) -> np.ndarray:
    """the restarted Rayleigh matrix ``[[Q^T G Q], [(Q^T g)^T]]``, (p + 1) x p"""
    p = Q.shape[1]
    out = np.empty((p + 1, p))
    out[:p] = Q.T @ R[:j, :j] @ Q
    out[p] = R[j, :j] @ Q
    return out


def restart(R: np.ndarray, j: int, keep: int, cap: int = MAX_KEEP):
    """(Q, the restarted Rayleigh matrix) for the `keep` largest Ritz values of R[:j, :j]"""
    th, Y = np.linalg.eig(R[:j, :j])
    sel = select_kept(th, keep, min(cap, j - 1))
    Q = invariant_basis(sel, th, Y)
    return Q, compress(R, j, Q)
