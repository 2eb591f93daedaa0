"""The CPU reference GMRES (tests/krylov_ref.py) checked against itself: the GPU tests of
tests/test_gpu_krylov.py compare the device FGMRES with it to 1e-12 (residual) and 1e-11
(iterate), so its own rounding error must be far below that."""
import numpy as np
import pytest

from helpers import golden_landm, mask_fix
from iemic import config as cf
from krylov_ref import csr_operator, fgmres_ref, krylov_lstsq_residual

KS = (1, 2, 5, 8, 13, 21)


def oracle_system(orc, name):
    """The oracle's J at the synthetic state and b = J . synthetic_vector(seed=5)."""
    c = cf.preset(name, mixing=0)
    L = mask_fix(orc, c, golden_landm(name))
    o = orc.Oracle(c.ref_dict(), L, c.par_list())
    ov, _ = o.jacobian(cf.synthetic_state(c, L, amp_ts=1e-3))
    b = o.spmv(ov, cf.synthetic_vector(c, seed=5))
    return c, L, o, ov, b


@pytest.mark.parametrize("name", ["test6x6x4", "natl8"])
def test_reference_gmres(oracle_lib, name):
    """float64 and longdouble runs of the reference agree 100 times closer than the bounds the
    GPU is held to (1e-13 on x, 1e-14 on rho: the spread measured on these grids is 2.2e-15 and
    1.6e-16), the Givens estimate is the true residual, and for k <= 8 the residual is the one
    of a dense least-squares problem over an explicitly orthonormalised Krylov basis."""
    c, L, o, ov, b = oracle_system(oracle_lib, name)
    A64 = csr_operator(o.rowptr, o.col, ov, np.float64)
    AL = csr_operator(o.rowptr, o.col, ov, np.longdouble)
    # the numpy CSR product is the oracle's
    v = cf.synthetic_vector(c, seed=11)
    scale = o.spmv(np.abs(ov), np.abs(v))
    assert np.all(np.abs(A64(v) - o.spmv(ov, v)) <= 1e-15 * scale)
    r64 = fgmres_ref(A64, None, b, max(KS), 0, np.float64)
    rL = fgmres_ref(AL, None, b, max(KS), 0, np.longdouble)
    assert len(r64.rho) == len(rL.rho) == max(KS)
    for k in KS:
        x64, xL = r64.x_steps[k - 1], rL.x_steps[k - 1]
        dx = float(np.linalg.norm((x64 - xL).astype(np.float64)) / np.linalg.norm(xL.astype(np.float64)))
        drho = float(abs(r64.rho[k - 1] - rL.rho[k - 1]) / rL.rho[k - 1])
        print(f"{name} k={k}: rho {float(rL.rho[k - 1]):.6e} spread x {dx:.2e} rho {drho:.2e}")
        assert rL.rho[k - 1] >= 1e-3          # far above rounding: relative errors mean something
        assert dx <= 1e-13 and drho <= 1e-14
        # the Givens estimate is the true residual (the basis is orthonormal)
        assert abs(rL.givens[k - 1] - rL.rho[k - 1]) <= 1e-13 * rL.rho[k - 1]
    # monotone: a minimal residual never grows with the space
    assert all(r64.rho[i + 1] <= r64.rho[i] * (1 + 1e-14) for i in range(len(r64.rho) - 1))
    for k in (1, 2, 5, 8):
        rho_d, x_d = krylov_lstsq_residual(AL, b, k)
        assert abs(rho_d - rL.rho[k - 1]) <= 1e-12 * rL.rho[k - 1], (k, rho_d, rL.rho[k - 1])
    # the restarted iterate: cycle c of GMRES(5) from the true residual is one cycle on b - A x
    rr = fgmres_ref(AL, None, b, 5, 2, np.longdouble)
    assert len(rr.x_cycles) == 3
    x1 = rr.x_cycles[0]
    again = fgmres_ref(AL, None, b - AL(x1), 5, 0, np.longdouble)
    assert np.array_equal(rr.x_cycles[1], x1 + again.x_cycles[0])
    assert rr.rho[14] < rr.rho[9] < rr.rho[4]


def test_reference_gmres_preconditioned(oracle_lib):
    """With a fixed linear M (a diagonal scaling) the preconditioned reference solves the same
    minimisation as the plain one on A M: x_k = M y_k."""
    c, L, o, ov, b = oracle_system(oracle_lib, "test6x6x4")
    AL = csr_operator(o.rowptr, o.col, ov, np.longdouble)
    d = (1.0 + 0.5 * np.cos(np.arange(c.nrows))).astype(np.longdouble)
    M = lambda v: np.asarray(v, dtype=np.float64) * d.astype(np.float64)
    ML = lambda v: v * d.astype(np.float64).astype(np.longdouble)
    a = fgmres_ref(AL, M, b, 8, 0, np.longdouble)
    p = fgmres_ref(lambda v: AL(ML(v)), None, b, 8, 0, np.longdouble)
    for k in (1, 5, 8):
        assert abs(a.rho[k - 1] - p.rho[k - 1]) <= 1e-13 * p.rho[k - 1]
        xp = ML(p.x_steps[k - 1])
        assert np.linalg.norm((a.x_steps[k - 1] - xp).astype(float)) <= 1e-13 * np.linalg.norm(xp.astype(float))
