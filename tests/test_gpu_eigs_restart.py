"""Thick (Krylov-Schur) restarts of the stability analysis on the GPU (csrc/eigs.hip's
k_eig_compress and eigs_restart, iemic_eigs_restart, Ocean.eigs(restarts=, keep=)).

* k_eig_compress through its hook, in place, against V[:j].T @ Q computed from the saved input,
  inside a bound derived from the arithmetic (below); the moved column bitwise; every entry the
  kernel must not touch (columns p + 1 .. j, rows >= N) bitwise.  Every case overwrites columns it
  still has to read (p < j), so a kernel that stored before it had read a row's j + 1 values
  would fail.
* end to end against the CPU fixture tests/golden/eigs_restart_natl8.npz (tests/eig_restart_ref.py,
  written without the code under test): at m_small the unrestarted run does not converge (the
  control), the restarted one does, inside 10 times the restarted inexact twin's own worst
  deviation from the dense reference and worst true residual (the factor and its reason are
  tests/test_gpu_eigs.py's: the twin and the GPU differ in the solver's rounding and in the
  last restart's Ritz values, not in method);
* a run that converges before step m is the same bits whatever `restarts` is; the same seed
  twice gives the same bits; two in-process latitude bands give the one-rank steps, restarts
  and, to the fixture's tolerance, eigenvalues; every misuse is refused by name.

Bound.  u = 2^-53.  k_eig_compress: column q is a chain of j fused multiply-adds, so
  |err| <= gamma_j (|V|^T |Q|), gamma_j = j u / (1 - j u); twice that for the rounding of the
  numpy reference itself (as k_eig_ritz in tests/test_gpu_eigs.py).
"""
import ctypes as C

import numpy as np
import pytest

import eig_ref as er
import eig_restart_ref as err
from iemic import _lib
from iemic import config as cf
from test_gpu_eigs import SOLVER, _PD, _d, bits, check_order, model
from test_gpu_transient import run_bands

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def Ocean():
    from iemic.ocean import Ocean
    return Ocean


@pytest.fixture(scope="module")
def fixture():
    out = {}
    for path in (er.FIXTURE, err.FIXTURE):
        with np.load(path, allow_pickle=False) as z:
            out.update({("base_" if path == er.FIXTURE else "") + k: z[k] for k in z.files})
    return out


@pytest.fixture(scope="module")
def small(Ocean):
    oc = Ocean(cf.preset("test6x6x4", mixing=0))
    yield oc
    oc.close()


def hook():
    L = _lib.lib()
    L.iemic_test_eig_compress.restype = C.c_int
    L.iemic_test_eig_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, _PD, _PD]
    return L.iemic_test_eig_compress


# ---- k_eig_compress ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,pad", [(864, 0), (864, 96), (1536, 7), (5001, 0), (5001, 7)])
@pytest.mark.parametrize("j,p", [(j, p) for j in (2, 7, 64) for p in (1, 5, 16) if p < j])
def test_compress_kernel(small, N, pad, j, p):
    rng = np.random.default_rng(1000 * j + 10 * p + pad + N)
    ldv = N + pad
    V0 = rng.standard_normal((j + 1, ldv)) * np.exp(rng.uniform(-3, 3, (j + 1, 1)))
    Q = rng.standard_normal((j, p))
    V = V0.copy()
    rc = hook()(small._h, j, p, N, ldv, _d(V), _d(Q))
    assert rc == 0, _lib.lib().iemic_last_error()
    ref = V0[:j, :N].T @ Q
    gamma = j * U / (1 - j * U)
    bound = 2 * gamma * (np.abs(V0[:j, :N]).T @ np.abs(Q))
    errv = np.abs(V[:p, :N].T - ref)
    print(f"N {N} ldv {ldv} j {j} p {p}: worst err / bound {np.max(errv / bound):.3f}")
    assert np.all(np.isfinite(V))
    assert np.all(errv <= bound)
    assert np.array_equal(bits(V[p, :N]), bits(V0[j, :N])), "column p is not the old column j"
    assert np.array_equal(bits(V[p + 1:, :N]), bits(V0[p + 1:, :N])), "a column behind p was written"
    assert np.array_equal(bits(V[:, N:]), bits(V0[:, N:])), "a row >= N was written"


def test_compress_hook_refuses_bad_shapes(small):
    V, Q = np.zeros((66, 8)), np.zeros((65, 17))
    for j, p, N, ldv in ((1, 1, 8, 8), (65, 1, 8, 8), (4, 0, 8, 8), (20, 17, 8, 8), (4, 4, 8, 8), (4, 5, 8, 8),
                         (4, 1, 8, 7), (4, 1, 0, 8)):
        assert hook()(small._h, j, p, N, ldv, _d(V), _d(Q)) == -22
    assert not V.any()


# ---- end to end --------------------------------------------------------------------------------
def run_natl8(Ocean, sigma, m, restarts, **kw):
    c, oc, L = model(Ocean, er.NAME, solver_params=SOLVER, **kw)
    oc.setState(cf.synthetic_state(c, L))
    solves = []
    oc.solve_hook = solves.append
    r = oc.eigs(k=er.K, sigma=sigma, m=m, tol=er.TOL, seed=er.SEED, restarts=restarts)
    return c, oc, L, r, len(solves)


@pytest.fixture(scope="module")
def oracle_natl8(oracle_lib):
    return er.system(oracle_lib)


@pytest.mark.parametrize("q", range(len(er.SIGMAS)))
def test_end_to_end_natl8_restarted(Ocean, fixture, oracle_natl8, q):
    sigma = er.SIGMAS[q]
    m, R = int(fixture[f"s{q}_m_small"]), int(fixture[f"s{q}_R"])
    assert m % 2 == 0 and er.K + 4 <= m <= int(fixture[f"base_s{q}_exact_steps"]) // 2
    # the control: today's unrestarted run is a dead end at m_small
    c, oc, L, r0, n0 = run_natl8(Ocean, sigma, m, 0)
    oc.close()
    print(f"sigma {sigma}, m {m}: unrestarted estimates {r0.estimate}")
    assert r0.steps == m == n0 and r0.restarts == 0 and not np.all(r0.converged)
    c, oc, L, r, nsolves = run_natl8(Ocean, sigma, m, R)
    dense = fixture[f"base_s{q}_lam_dense"]
    twin_dev = float(fixture[f"s{q}_inexact_worst_deviation"])
    twin_res = float(fixture[f"s{q}_inexact_worst_residual"])
    n = len(fixture[f"s{q}_inexact_lam"])
    print(f"  restarted: {r.steps} inner solves, {r.restarts} restarts (twin {int(fixture[f's{q}_inexact_steps'])}, "
          f"{int(fixture[f's{q}_inexact_restarts'])}; allowed {R}), unconverged solves {r.solve_unconverged}")
    assert 1 <= r.restarts <= R and r.steps == nsolves == len(r.solve_iters)
    assert r.H.shape[0] == r.H.shape[1] + 1 and r.H.shape[1] <= m
    assert len(r.lam) == n and not r.breakdown and r.solve_unconverged == 0
    check_order(r.lam, sigma)
    assert np.all(r.converged) and np.all(r.estimate <= er.TOL)
    dev = np.abs(r.lam[:, None] - dense[None, :]) / np.abs(dense[None, :] - sigma)
    near = np.argmin(dev, axis=1)
    gpu_dev = dev[np.arange(n), near]
    print(f"  deviation from the dense reference {gpu_dev} (twin's worst {twin_dev:.3e})")
    assert sorted(near) == list(range(n)), "not the n eigenvalues nearest the shift"
    assert np.all(gpu_dev <= 10 * twin_dev)
    co, o, Lo, xo, val, B, diag = oracle_natl8
    assert np.array_equal(L, Lo)
    As = er.csr(o, er.shifted_val(val, B, diag, sigma))
    res = np.array([er.true_residual(As, B, sigma, r.lam[i], r.to_host(i)) for i in range(n)])
    print(f"  residual numpy {res}\n  residual device {r.residual}\n  estimate {r.estimate} "
          f"(twin's worst residual {twin_res:.3e})")
    assert np.all(res <= 10 * twin_res)
    del r
    oc.close()


def test_no_restart_triggered_same_bits(Ocean):
    sigma = er.SIGMAS[1]
    c, a, L, ra, _ = run_natl8(Ocean, sigma, er.M, 0)
    a.close()
    c, b, L, rb, _ = run_natl8(Ocean, sigma, er.M, 3)
    b.close()
    assert ra.steps == rb.steps < er.M and ra.restarts == rb.restarts == 0
    for x, y in ((ra.lam.view(np.float64), rb.lam.view(np.float64)), (ra.residual, rb.residual),
                 (ra.estimate, rb.estimate), (ra.H, rb.H)):
        assert np.array_equal(bits(x), bits(y))


def test_same_seed_same_bits_and_two_bands(Ocean, fixture):
    q = 1
    sigma = er.SIGMAS[q]
    m, R = int(fixture[f"s{q}_m_small"]), int(fixture[f"s{q}_R"])
    c, a, L, ra, _ = run_natl8(Ocean, sigma, m, R)
    a.close()
    c, b, L, rb, _ = run_natl8(Ocean, sigma, m, R)
    b.close()
    assert ra.restarts >= 1 and np.all(ra.converged)
    assert (ra.steps, ra.restarts) == (rb.steps, rb.restarts)
    assert np.array_equal(bits(ra.lam.view(np.float64)), bits(rb.lam.view(np.float64)))
    assert np.array_equal(bits(ra.residual), bits(rb.residual))
    L0 = cf.landmask(c)
    x = cf.synthetic_state(c, L)

    def fn(rank, group):
        from iemic.ocean import Ocean as Oc
        oc = Oc(c, landm=L0, local_group=group, rank=rank, nranks=2, npx=1, solver_params=SOLVER)
        oc.setState(x)
        r = oc.eigs(k=er.K, sigma=sigma, m=m, tol=er.TOL, seed=er.SEED, restarts=R)
        out = dict(lam=r.lam, steps=r.steps, restarts=r.restarts, converged=r.converged)
        del r
        oc.close()
        return out

    tol = 10 * float(fixture[f"s{q}_inexact_worst_deviation"])
    for r in run_bands(2, fn):
        dev = np.abs(r["lam"] - ra.lam) / np.abs(ra.lam - sigma)
        print(f"bands: {r['steps']} solves, {r['restarts']} restarts (one rank {ra.steps}, {ra.restarts}), "
              f"deviation from one rank {dev}")
        assert (r["steps"], r["restarts"]) == (ra.steps, ra.restarts) and len(r["lam"]) == len(ra.lam)
        assert np.all(r["converged"]) and np.all(dev <= tol)


# ---- refusals and state --------------------------------------------------------------------------
def test_refusals_and_state(Ocean):
    c, oc, L = model(Ocean, "natl8")
    oc.setState(cf.synthetic_state(c, L))
    lib, kr = _lib.lib(), oc._krylov()
    hcol, info = np.zeros(_lib.EIGS_MAX_M + 2), _lib.EigsInfo()
    m, p = 6, 2
    Q = np.zeros((m, 17))
    Q[0, 0] = Q[1, 1] = 1.0
    Qp = np.ascontiguousarray(Q[:, :p])
    step = lambda: lib.iemic_eigs_step(oc._h, C.byref(kr), _d(hcol), C.byref(info))

    assert lib.iemic_eigs_restart(oc._h, p, _d(Qp)) == -71                  # before begin
    assert b"iemic_eigs_begin" in lib.iemic_last_error()
    with pytest.raises(_lib.IemicError, match=r"rc=-71.*no Jacobian assembled"):
        oc.exportCSR()                                                      # nothing ran
    _lib.check(lib.iemic_eigs_begin(oc._h, 0.02, m, 1, C.byref(kr)), "iemic_eigs_begin")
    for j in range(m):
        assert step() in (0, _lib.IEMIC_ENOCONV)
    assert step() == -71 and b"all m steps" in lib.iemic_last_error()
    nan = Qp.copy()
    nan[m - 1, p - 1] = np.nan
    for pp, q, text in ((0, Qp, b"at least 1"), (m, Q[:, :m].copy(), b"smaller than the number of steps"),
                        (17, Q, b"exceeds 16"), (p, nan, b"non-finite"), (p, None, b"null")):
        assert lib.iemic_eigs_restart(oc._h, pp, _d(q)) == -22
        assert text in lib.iemic_last_error(), (pp, lib.iemic_last_error())
        # nothing was launched and nothing changed: the run is still at its last step
        assert step() == -71 and b"all m steps" in lib.iemic_last_error()
    assert lib.iemic_eigs_restart(oc._h, p, _d(Qp)) == 0, lib.iemic_last_error()
    for j in range(p, m):
        assert step() in (0, _lib.IEMIC_ENOCONV)
        assert info.step == j and np.all(np.isfinite(hcol[:j + 2])) and hcol[j + 1] > 0
    assert step() == -71 and b"all m steps" in lib.iemic_last_error()
    assert lib.iemic_eigs_end(oc._h) == 0
    assert lib.iemic_eigs_restart(oc._h, p, _d(Qp)) == -71
    oc.close()
