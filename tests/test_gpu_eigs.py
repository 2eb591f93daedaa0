"""Linear stability analysis on the GPU model (csrc/eigs.hip, iemic/eigs.py).

* the shifted Jacobian J - sigma B is numpy's val + -(sigma * B) on the diagonal bit for bit, built
  here from the unshifted Jacobian and B of the same model, through both Jacobian buffers;
* k_eig_ritz against V[:j].T @ Y and k_eig_residual against numpy, through test hooks, inside
  bounds derived from the arithmetic (below), not measured;
* end to end against the CPU fixture tests/golden/eigs_natl8.npz (tests/eig_ref.py, written
  without the code under test): the eigenvalues against the dense reference, inside 10 times
  the inexact-solve twin's own worst deviation from it, and every pair's true residual
  recomputed in numpy from the oracle's J and B inside 10 times that twin's worst residual;
* the same seed twice gives the same bits; two in-process latitude bands give the one-rank
  eigenvalues and step count; every misuse is refused by name.

Bounds.  u = 2^-53.
  k_eig_ritz: X_q = sum_i Y[i, q] V_i is a chain of j fused multiply-adds, so
    |err| <= gamma_j (|V|^T |Y|), gamma_j = j u / (1 - j u); twice that for the rounding of the
    numpy reference itself.
  k_eig_residual: with b x rounded once, r_r = a_r - (mu_r b x_r - mu_i b x_i) carries at most
    e_r = 4 u (|a_r| + |mu_r b x_r| + |mu_i b x_i|) (four roundings, each at most u times the
    running magnitude), likewise e_i; a term t = r_r^2 + r_i^2 is then off by at most
    2 |r_r| e_r + 2 |r_i| e_i + 3 u t, and the sum of NL terms by NL u sum(t).  The reference is
    evaluated in long double, whose own error is 2^-11 of these.
"""
import ctypes as C

import numpy as np
import pytest

import eig_ref as er
from iemic import _lib
from iemic import config as cf
from test_gpu_transient import csr_rows, owned_rows, run_bands

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_PD = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def Ocean():
    from iemic.ocean import Ocean
    return Ocean


@pytest.fixture(scope="module")
def fixture():
    with np.load(er.FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def small(Ocean):
    """a context for the kernel hooks (their shapes are their own)"""
    oc = Ocean(cf.preset("test6x6x4", mixing=0))
    yield oc
    oc.close()


def hooks():
    L = _lib.lib()
    vp, i, i64, d = C.c_void_p, C.c_int, C.c_int64, C.c_double
    L.iemic_test_eig_ritz.restype = i
    L.iemic_test_eig_ritz.argtypes = [vp, i, i, i64, i64, _PD, _PD, _PD]
    L.iemic_test_eig_residual.restype = i
    L.iemic_test_eig_residual.argtypes = [vp, i64, _PD, _PD, _PD, _PD, _PD, d, d, _PD]
    return L


def _d(a):
    return None if a is None else a.ctypes.data_as(_PD)


def model(Ocean, name, **kw):
    c = cf.preset(name)
    oc = Ocean(c, **kw)
    L = oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    return c, oc, L


def shifted(rowptr, col, val, B, sigma):
    """val with -(sigma B) added on the diagonal where B != 0; every other entry keeps its bits"""
    Bn = B[csr_rows(rowptr)]
    hit = (col == csr_rows(rowptr)) & (Bn != 0)
    want = val.copy()
    want[hit] = val[hit] + -(sigma * Bn[hit])
    return want


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- the shifted Jacobian ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["natl8", "gateway16"])
@pytest.mark.parametrize("sigma", [0.0, 0.5, 10.0])
def test_shifted_jacobian_bitwise(Ocean, name, sigma):
    c, oc, L = model(Ocean, name)
    oc.setState(cf.synthetic_state(c, L))
    oc.computeJacobian()
    rowptr, col, val = oc.exportCSR()
    B = oc.diagB()
    assert np.count_nonzero(B) > 0
    want = shifted(rowptr, col, val, B, sigma)
    assert np.count_nonzero(want != val) == (np.count_nonzero(B) if sigma else 0)
    for second_buffer in (False, True):
        if second_buffer:       # with the preconditioner set up, the Jacobian goes to the second buffer
            oc.buildPreconditioner(force=True)
        oc.shiftedJacobian(sigma)
        rp2, col2, val2 = oc.exportCSR()
        assert np.array_equal(rp2, rowptr) and np.array_equal(col2, col)
        assert np.array_equal(bits(val2), bits(want))
        assert np.array_equal(bits(oc.diagB()), bits(B))
        oc.computeJacobian()
        assert np.array_equal(bits(oc.exportCSR()[2]), bits(val))
    oc.close()


# ---- k_eig_ritz ------------------------------------------------------------------------------
@pytest.mark.parametrize("NL,pad", [(864, 0), (864, 96), (1536, 0), (1536, 7)])
@pytest.mark.parametrize("j", [1, 7, 64])
@pytest.mark.parametrize("p", [1, 2, 5, 16])
def test_ritz_kernel(small, NL, pad, j, p):
    rng = np.random.default_rng(1000 * j + 10 * p + pad)
    ldv = NL + pad
    V = rng.standard_normal((j, ldv)) * np.exp(rng.uniform(-3, 3, (j, 1)))
    Y = rng.standard_normal((j, p))
    X = np.zeros((p, NL))
    rc = hooks().iemic_test_eig_ritz(small._h, j, p, NL, ldv, _d(V), _d(Y), _d(X))
    assert rc == 0, _lib.lib().iemic_last_error()
    ref = V[:, :NL].T @ Y
    gamma = j * U / (1 - j * U)
    bound = 2 * gamma * (np.abs(V[:, :NL]).T @ np.abs(Y))
    err = np.abs(X.T - ref)
    print(f"NL {NL} ldv {ldv} j {j} p {p}: worst err / bound {np.max(err / bound):.3f}")
    assert np.all(np.isfinite(X))
    assert np.all(err <= bound)


def test_ritz_hook_refuses_bad_shapes(small):
    V, Y, X = np.zeros((65, 8)), np.zeros((65, 17)), np.zeros((17, 8))
    for j, p, N, ldv in ((0, 1, 8, 8), (65, 1, 8, 8), (1, 0, 8, 8), (1, 17, 8, 8), (1, 1, 8, 7)):
        assert hooks().iemic_test_eig_ritz(small._h, j, p, N, ldv, _d(V), _d(Y), _d(X)) == -22


# ---- k_eig_residual --------------------------------------------------------------------------
def residual_reference(ar, ai, xr, xi, B, mu_r, mu_i):
    ld = np.longdouble
    z = np.zeros_like(ar)
    ai_, xi_ = (z if ai is None else ai), (z if xi is None else xi)
    a_r, a_i, x_r, x_i, b = (v.astype(ld) for v in (ar, ai_, xr, xi_, B))
    m_r, m_i = ld(mu_r), ld(mu_i)
    rr = a_r - (m_r * b * x_r - m_i * b * x_i)
    ri = a_i - (m_r * b * x_i + m_i * b * x_r)
    t = rr * rr + ri * ri
    ta = a_r * a_r + a_i * a_i
    e_r = 4 * U * (np.abs(a_r) + np.abs(m_r * b * x_r) + np.abs(m_i * b * x_i))
    e_i = 4 * U * (np.abs(a_i) + np.abs(m_r * b * x_i) + np.abs(m_i * b * x_r))
    n = len(ar)
    bound_r = np.sum(2 * np.abs(rr) * e_r + 2 * np.abs(ri) * e_i) + (n + 3) * U * np.sum(t)
    bound_a = (n + 3) * U * np.sum(ta)
    return float(np.sum(t)), float(np.sum(ta)), float(bound_r), float(bound_a)


@pytest.mark.parametrize("NL", [864, 5001])
@pytest.mark.parametrize("cplx", [False, True])
def test_residual_kernel(small, NL, cplx):
    rng = np.random.default_rng(7 + NL + cplx)
    ar, xr, ai, xi = (rng.standard_normal(NL) for _ in range(4))
    B = -rng.uniform(0.0, 2.0, NL) * (rng.uniform(size=NL) < 0.43)      # <= 0, about 57 % zeros
    mu_r, mu_i = -0.0375, (0.0123 if cplx else 0.0)
    if not cplx:
        ai = xi = None
    out, out2 = np.zeros(2), np.zeros(2)
    for o in (out, out2):
        rc = hooks().iemic_test_eig_residual(small._h, NL, _d(ar), _d(ai), _d(xr), _d(xi), _d(B), mu_r, mu_i, _d(o))
        assert rc == 0, _lib.lib().iemic_last_error()
    sr, sa, br, ba = residual_reference(ar, ai, xr, xi, B, mu_r, mu_i)
    print(f"NL {NL} complex {cplx}: |err| / bound {abs(out[0] - sr) / br:.3f}, {abs(out[1] - sa) / ba:.3f}")
    assert abs(out[0] - sr) <= br and abs(out[1] - sa) <= ba
    assert np.array_equal(bits(out), bits(out2))


# ---- end to end --------------------------------------------------------------------------------
SOLVER = {"FGMRES tolerance": er.INNER_TOL, "FGMRES iterations": 500, "FGMRES restarts": 0}


def check_order(lam, sigma):
    d = np.abs(lam - sigma)
    assert np.all(np.diff(d) >= -1e-12 * d[:-1])
    i = 0
    while i < len(lam):
        if lam[i].imag != 0:
            assert lam[i].imag > 0 and lam[i + 1] == np.conj(lam[i])
            i += 2
        else:
            i += 1


def run_natl8(Ocean, sigma, **kw):
    c, oc, L = model(Ocean, er.NAME, solver_params=SOLVER, **kw)
    oc.setState(cf.synthetic_state(c, L))
    r = oc.eigs(k=er.K, sigma=sigma, m=er.M, tol=er.TOL, seed=er.SEED)
    return c, oc, L, r


@pytest.fixture(scope="module")
def oracle_natl8(oracle_lib):
    return er.system(oracle_lib)


@pytest.fixture(scope="module")
def natl8_runs(Ocean, oracle_natl8):
    """both shifts once: (result, the residuals recomputed in numpy from the oracle's J and B,
    the same in numpy's extended precision)"""
    co, o, Lo, xo, val, B, diag = oracle_natl8
    out, live = [], []
    for sigma in er.SIGMAS:
        c, oc, L, r = run_natl8(Ocean, sigma)
        assert np.array_equal(L, Lo)
        As = er.csr(o, er.shifted_val(val, B, diag, sigma))
        res = np.array([er.true_residual(As, B, sigma, r.lam[i], r.to_host(i)) for i in range(len(r.lam))])
        vs = er.shifted_val(val, B, diag, sigma)
        resx = np.array([er.true_residual_extended(o, vs, B, sigma, r.lam[i], r.to_host(i))
                         for i in range(len(r.lam))])
        out.append((r, res, resx))
        live.append(oc)
    yield out
    out.clear()
    for oc in live:
        oc.close()


@pytest.mark.parametrize("q", range(len(er.SIGMAS)))
def test_end_to_end_natl8(fixture, natl8_runs, q):
    sigma = er.SIGMAS[q]
    r, res, _ = natl8_runs[q]
    dense = fixture[f"s{q}_lam_dense"]
    twin_dev = float(fixture[f"s{q}_inexact_worst_deviation"])
    twin_res = float(fixture[f"s{q}_inexact_worst_residual"])
    n = len(fixture[f"s{q}_inexact_lam"])
    print(f"sigma {sigma}: {r.steps} steps (twin {int(fixture[f's{q}_inexact_steps'])}), inner "
          f"{min(r.solve_iters)}..{max(r.solve_iters)}, unconverged solves {r.solve_unconverged}")
    assert len(r.lam) == n and not r.breakdown and r.solve_unconverged == 0
    check_order(r.lam, sigma)
    dev = np.abs(r.lam[:, None] - dense[None, :]) / np.abs(dense[None, :] - sigma)
    near = np.argmin(dev, axis=1)
    gpu_dev = dev[np.arange(n), near]
    print(f"  deviation from the dense reference {gpu_dev} (twin's worst {twin_dev:.3e})")
    assert sorted(near) == list(range(n)), "not the n eigenvalues nearest the shift"
    assert np.all(gpu_dev <= 10 * twin_dev)
    print(f"  residual numpy {res}\n  residual device {r.residual}\n  estimate {r.estimate} "
          f"(twin's worst residual {twin_res:.3e})")
    assert np.all(r.converged) and np.all(r.estimate <= er.TOL)
    assert np.all(res <= 10 * twin_res)


@pytest.mark.parametrize("q", range(len(er.SIGMAS)))
def test_reported_residuals_agree_with_numpy(natl8_runs, q):
    """The residuals the library reports against the numpy ones, to 1e-6 relative.

    The pairs converged to below 1e-10 have residuals ten orders below their two terms, so the
    rounding of a = (J - sigma B) x in fp64, a few u ||(|J| |x|)|| / ||a|| ~ 3e-15 here, is up to
    7e-5 of the residual: two fp64 evaluations with different summation orders cannot agree
    to 1e-6 (measured with both in fp64: 4.5e-5 at sigma = 0, 7.2e-5 at sigma = 0.02).  The
    library therefore forms the products in double-double, and the numpy side is evaluated
    in extended precision from the same fp64 J, B, lambda and x (eig_ref.true_residual_extended).
    The fp64 numpy residual is printed beside them."""
    r, res, resx = natl8_runs[q]
    print(f"sigma {er.SIGMAS[q]}: |device - numpy| {np.abs(r.residual - resx)}, relative "
          f"{np.abs(r.residual - resx) / resx}\n  fp64 numpy against extended, relative {np.abs(res - resx) / resx}")
    assert np.all(np.abs(r.residual - resx) <= 1e-6 * resx)


def test_end_to_end_gateway16(Ocean, fixture, oracle_lib):
    sigma, k = float(fixture["gw_sigma"]), int(fixture["gw_k"])
    assert sigma > 0
    c, oc, L = model(Ocean, er.GW_NAME, solver_params=SOLVER)
    oc.setState(cf.synthetic_state(c, L))
    r = oc.eigs(k=k, sigma=sigma, m=er.M, tol=er.TOL, seed=er.SEED)
    co, o, Lo, xo, val, B, diag = er.system(oracle_lib, er.GW_NAME)
    assert np.array_equal(L, Lo)
    As = er.csr(o, er.shifted_val(val, B, diag, sigma))
    res = np.array([er.true_residual(As, B, sigma, r.lam[i], r.to_host(i)) for i in range(len(r.lam))])
    twin_res = float(fixture["gw_worst_residual"])
    print(f"gateway16 sigma {sigma}: {r.steps} steps (twin {int(fixture['gw_steps'])}), lambda {r.lam} "
          f"(twin {fixture['gw_lam']})\n  residual numpy {res} device {r.residual} estimate {r.estimate} "
          f"(twin's worst residual {twin_res:.3e}), inner {min(r.solve_iters)}..{max(r.solve_iters)}, "
          f"{r.solve_unconverged} inner solves flagged unconverged")
    assert len(r.lam) in (k, k + 1)
    check_order(r.lam, sigma)
    assert np.all(r.estimate <= er.TOL) and np.all(r.converged)
    assert np.all(res <= 10 * twin_res)
    oc.close()


def test_same_seed_same_bits_and_two_bands(Ocean, fixture):
    q = 1
    sigma = er.SIGMAS[q]
    c, a, L, ra = run_natl8(Ocean, sigma)
    a.close()
    c, b, L, rb = run_natl8(Ocean, sigma)
    b.close()
    assert ra.steps == rb.steps
    assert np.array_equal(bits(ra.lam.view(np.float64)), bits(rb.lam.view(np.float64)))
    assert np.array_equal(bits(ra.residual), bits(rb.residual))
    L0 = cf.landmask(c)
    x = cf.synthetic_state(c, L)

    def fn(rank, group):
        from iemic.ocean import Ocean as Oc
        oc = Oc(c, landm=L0, local_group=group, rank=rank, nranks=2, npx=1, solver_params=SOLVER)
        oc.setState(x)
        r = oc.eigs(k=er.K, sigma=sigma, m=er.M, tol=er.TOL, seed=er.SEED)
        out = dict(lam=r.lam, steps=r.steps, residual=r.residual, lay=oc.layout(),
                   x0=r.to_host(0))
        del r
        oc.close()
        return out

    res = run_bands(2, fn)
    tol = 10 * float(fixture[f"s{q}_inexact_worst_deviation"])
    x0 = np.zeros(c.nrows, dtype=np.complex128)
    for r in res:
        dev = np.abs(r["lam"] - ra.lam) / np.abs(ra.lam - sigma)
        print(f"bands: {r['steps']} steps (one rank {ra.steps}), deviation from one rank {dev}")
        assert r["steps"] == ra.steps and len(r["lam"]) == len(ra.lam)
        assert np.all(dev <= tol)
        rows = owned_rows(c, r["lay"])
        x0[rows] = r["x0"][rows]
    # the bands' pieces of the first eigenvector make one vector of unit norm over the rows the
    # loop's inner product counts
    assert abs(np.linalg.norm(er.not_p_rows(c.nrows) * x0) - 1.0) <= 1e-10


# ---- refusals ------------------------------------------------------------------------------------
def test_refusals(Ocean):
    c, oc, L = model(Ocean, "natl8")
    oc.setState(cf.synthetic_state(c, L))
    lib, kr = _lib.lib(), oc._krylov()
    hcol, info = np.zeros(_lib.EIGS_MAX_M + 2), _lib.EigsInfo()

    def nothing_ran():
        # no Jacobian was assembled and no run exists: the refusal came before any launch
        with pytest.raises(_lib.IemicError, match=r"rc=-71.*no Jacobian assembled"):
            oc.exportCSR()
        assert lib.iemic_eigs_step(oc._h, C.byref(kr), _d(hcol), C.byref(info)) == -71
        assert b"iemic_eigs_begin" in lib.iemic_last_error()

    nothing_ran()                                               # iemic_eigs_step before begin
    with pytest.raises(_lib.IemicError, match=r"rc=-22.*m must be at least 1"):
        _lib.check(lib.iemic_eigs_begin(oc._h, 0.0, 0, 1, C.byref(kr)), "iemic_eigs_begin")
    nothing_ran()
    with pytest.raises(_lib.IemicError, match=r"rc=-22.*IEMIC_EIGS_MAX_M = 64"):
        oc.eigs(k=6, m=_lib.EIGS_MAX_M + 1)
    nothing_ran()
    with pytest.raises(_lib.IemicError, match=r"k = 7 exceeds the basis size m = 6"):
        oc.eigs(k=7, m=6)
    nothing_ran()
    with pytest.raises(_lib.IemicError, match=r"rc=-22.*sigma must be finite"):
        oc.eigs(sigma=float("nan"))
    nothing_ran()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(_lib.IemicError, match=r"rc=-22.*iemic_shifted_jacobian.*sigma must be finite"):
            oc.shiftedJacobian(bad)
    nothing_ran()
    # after m steps
    _lib.check(lib.iemic_eigs_begin(oc._h, 0.02, 2, 1, C.byref(kr)), "iemic_eigs_begin")
    for j in range(2):
        assert lib.iemic_eigs_step(oc._h, C.byref(kr), _d(hcol), C.byref(info)) in (0, _lib.IEMIC_ENOCONV)
        assert info.step == j and np.all(np.isfinite(hcol[:j + 2])) and hcol[j + 1] > 0
    assert lib.iemic_eigs_step(oc._h, C.byref(kr), _d(hcol), C.byref(info)) == -71
    assert b"all m steps" in lib.iemic_last_error()
    assert lib.iemic_eigs_end(oc._h) == 0
    assert lib.iemic_eigs_step(oc._h, C.byref(kr), _d(hcol), C.byref(info)) == -71
    oc.close()
