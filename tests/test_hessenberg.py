"""The Hessenberg/Givens least-squares code shared by the three Arnoldi loops
(i-emic_amd/csrc/hessenberg.h) against numpy, on the host alone: tests/emul/
hessenberg_driver.cpp includes the header, is built here with g++ (no contraction, as
tests/emul is) and fed seeded random upper-Hessenberg columns.

Matrices: m in {1, 2, 5, 12}, entries uniform in (-1, 1) with 4 added to the diagonal, beta = 1.
The diagonal keeps sigma_min(H) well above 1, so ||y|| < beta and the backward error of the
Givens reduction, O(k eps ||H|| ||y||), stays inside the residual bound 50 eps ||H||.

For every k <= m, after k pushed columns:
  - ||beta e1 - H y||_2 (evaluated in long double) equals the |g[k]| push_column returned to
    50 eps ||H||_2, H the (k + 1) x k matrix;
  - y equals numpy.linalg.lstsq on that matrix to 10 x numpy's own spread: the largest
    relative distance, over all these matrices, between numpy's float64 lstsq and the same
    least-squares problem solved in long double (Givens, 64-bit mantissa).  Measured spread:
    4.1e-15 relative (max-norm; numpy's lstsq at m = 12, k = 8), so the bound is 4.1e-14.
    The header's distance to numpy's lstsq is 4.1e-15 in that one case (numpy's own error)
    and at most 1.1e-15 in every other.  The spread is measured again at every run and must
    not exceed the recorded figure (NUMPY_SPREAD).
Special cases: a breakdown column (hn == 0: residual exactly 0, sn == 0, y the exact solve),
and a column with x0 == x1 == 0 (cs = 1, sn = 0).
"""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emul", "hessenberg_driver.cpp")
HDR = os.path.join(os.path.dirname(HERE), "i-emic_amd", "csrc", "hessenberg.h")
EPS = np.finfo(np.float64).eps
SIZES = (1, 2, 5, 12)

# numpy's float64-against-long-double spread as measured (docstring), rounded up: the lstsq
# bound is 10 x the spread and must not loosen if a later numpy does worse
NUMPY_SPREAD = 4.2e-15


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hess") / "hessenberg_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, SRC], check=True)

    def run(m, beta, cols):
        """cols[q] = (col[0..q], hn).  Returns per column (res, cs, sn, y[0..q])."""
        words = [str(m), str(len(cols)), float(beta).hex()]
        for col, hn in cols:
            words += [float(v).hex() for v in col] + [float(hn).hex()]
        r = subprocess.run([exe], input=" ".join(words), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = []
        for line in r.stdout.splitlines():
            v = [float.fromhex(w) for w in line.split()]
            out.append((v[0], v[1], v[2], np.array(v[3:])))
        assert len(out) == len(cols)
        return out
    return run


def hbar(m, seed=20261019):
    """(m + 1) x m upper Hessenberg, uniform(-1, 1) with the diagonal shifted by 4."""
    rng = np.random.default_rng(seed + m)
    H = np.triu(rng.uniform(-1.0, 1.0, (m + 1, m)), -1)
    H[np.arange(m), np.arange(m)] += 4.0
    return H


def columns(H):
    return [(H[:q + 1, q], H[q + 1, q]) for q in range(H.shape[1])]


def lstsq_longdouble(H, beta):
    """min ||beta e1 - H y|| by Givens rotations and back substitution in long double."""
    k = H.shape[1]
    R = H.astype(np.longdouble).copy()
    g = np.zeros(k + 1, np.longdouble)
    g[0] = beta
    for q in range(k):
        a, b = R[q, q], R[q + 1, q]
        d = np.sqrt(a * a + b * b)
        c, s = a / d, b / d
        rq, rn = R[q, :].copy(), R[q + 1, :].copy()
        R[q, :], R[q + 1, :] = c * rq + s * rn, -s * rq + c * rn
        g[q], g[q + 1] = c * g[q], -s * g[q]
    y = np.zeros(k, np.longdouble)
    for i in range(k - 1, -1, -1):
        y[i] = (g[i] - R[i, i + 1:k] @ y[i + 1:]) / R[i, i]
    return y


@pytest.fixture(scope="module")
def cases():
    """Every (m, k): the matrix, numpy's float64 lstsq, the long double solution; and numpy's
    spread over all of them."""
    out, spread = {}, 0.0
    for m in SIZES:
        H = hbar(m)
        for k in range(1, m + 1):
            Hk = H[:k + 1, :k]
            e1 = np.zeros(k + 1)
            e1[0] = 1.0
            y64 = np.linalg.lstsq(Hk, e1, rcond=None)[0]
            yld = lstsq_longdouble(Hk, 1.0)
            spread = max(spread, float(np.max(np.abs(y64 - yld)) / np.max(np.abs(yld))))
            out[(m, k)] = (Hk, y64, yld)
    return out, spread


@pytest.mark.parametrize("m", SIZES)
def test_residual_and_solution(driver, cases, m):
    table, spread = cases
    got = driver(m, 1.0, columns(hbar(m)))
    assert 0.0 < spread <= NUMPY_SPREAD
    for k in range(1, m + 1):
        Hk, y64, _ = table[(m, k)]
        res, _, _, y = got[k - 1]
        e1 = np.zeros(k + 1, np.longdouble)
        e1[0] = 1.0
        true_res = float(np.sqrt(np.sum((e1 - Hk.astype(np.longdouble) @ y.astype(np.longdouble)) ** 2)))
        bound = 50 * EPS * np.linalg.norm(Hk, 2)
        dist = float(np.max(np.abs(y - y64)) / np.max(np.abs(y64)))
        print(f"m={m} k={k} res={res:.6e} |res-true|={abs(res - true_res):.2e} bound={bound:.2e} "
              f"y-dist={dist:.2e} numpy-spread={spread:.2e}")
        assert abs(res - true_res) <= bound
        assert dist <= 10 * spread


def test_breakdown_column(driver):
    """hn == 0 in the last column: the Krylov space is invariant, the residual is exactly 0 and
    y solves the square system."""
    m = 5
    H = hbar(m)
    H[m, m - 1] = 0.0
    res, cs, sn, y = driver(m, 1.0, columns(H))[-1]
    assert res == 0.0 and sn == 0.0 and abs(cs) == 1.0
    e1 = np.zeros(m)
    e1[0] = 1.0
    ref = np.linalg.solve(H[:m, :m], e1)
    assert np.max(np.abs(y - ref)) <= 50 * EPS * np.linalg.cond(H[:m, :m]) * np.max(np.abs(ref))


@pytest.mark.parametrize("q", (0, 2))
def test_zero_column_gives_identity_rotation(driver, q):
    """x0 == x1 == 0 when rotation q is formed: cs = 1, sn = 0, no division by d = 0."""
    m = 5
    H = hbar(m)
    H[:, q] = 0.0
    res, cs, sn, _ = driver(m, 1.0, columns(H)[:q + 1])[q]
    assert cs == 1.0 and sn == 0.0 and res == 0.0


def test_header_is_host_only():
    with open(HDR) as f:
        text = f.read()
    assert "#include <hip" not in text and '#include "common.h"' not in text
