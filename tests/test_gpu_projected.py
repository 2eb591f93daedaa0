"""The projected theta model on the GPU (csrc/projected.hip, k_spmm7 in csrc/spmv.hip,
iemic.transient).

 1. every column of the block product J V has applyMatrix's bits, for J and the shifted Jacobian;
 2. the block Gram products against exactly rounded references, within n 2^-52 sum |V d W| (a bound
    that holds for any summation order), bitwise reproducible, no dropped tail;
 3. the init step and the residual against the NumPy twin (tests/proj_ref.py, oracle only);
 4. the k x k solve against numpy.linalg.solve; a singular V^T J2 V refused by name;
 5. the fused Newton iteration equals the composed one, bit for bit;
 6. the noise G = V^T (the full model's noise field); sigma = 0 and a plain init step disarm it;
 7. three adaptive steps of the stochastic stepper against the twin under the same stepper class;
 8. two in-process latitude bands;
 9. the refusals, by name;
10. no preconditioner is built and no Krylov solver runs.
"""
import ctypes as C

import numpy as np
import pytest

from iemic import _lib
from iemic import config as cf
from iemic.config import PAR_INDEX
from iemic.transient import StochasticProjectedThetaStepper, StochasticThetaStepper
from proj_ref import EPS, ProjectedTwin, csr_mm, gram
from stoch_ref import forcing_column, noise
from test_gpu_transient import SOLVER, model, run_bands
from test_transient import PARAMS, transient_config

pytestmark = pytest.mark.gpu

_PD = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def Ocean():
    from iemic.ocean import Ocean
    return Ocean


def hooks():
    L = _lib.lib()
    L.iemic_test_spmm.restype = C.c_int
    L.iemic_test_spmm.argtypes = [C.c_void_p, C.c_int, C.c_int, _PD, _PD]
    L.iemic_test_gram.restype = C.c_int
    L.iemic_test_gram.argtypes = [C.c_void_p, C.c_int, C.c_int, _PD, _PD, _PD, _PD]
    return L


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def cols(V):
    """N x k -> the hooks' column-major copy"""
    return np.ascontiguousarray(np.asarray(V, dtype=np.float64).reshape(len(V), -1).T)


def spmm(oc, V, kbmax=0):
    Vc = cols(V)
    W = np.full_like(Vc, np.nan)
    _lib.check(hooks().iemic_test_spmm(oc._h, Vc.shape[0], kbmax, _lib.ptr(Vc), _lib.ptr(W)), "iemic_test_spmm")
    return W.T


def dev_gram(oc, V, W, d=None):
    Vc, Wc = cols(V), cols(W)
    G = np.zeros((Vc.shape[0], Wc.shape[0]))
    dd = None if d is None else _lib.ptr(np.ascontiguousarray(d, dtype=np.float64))
    _lib.check(hooks().iemic_test_gram(oc._h, Vc.shape[0], Wc.shape[0], _lib.ptr(Vc), dd, _lib.ptr(Wc), _lib.ptr(G)),
               "iemic_test_gram")
    return G


def basis(N, k, seed=1):
    return np.random.default_rng(seed).standard_normal((N, k))


# ---- 1. the block product ---------------------------------------------------------------------
@pytest.mark.parametrize("name,ks", [("natl8", (1, 2, 3, 5, 8, 9)), ("gateway16", (1, 2, 3, 5, 8, 9)),
                                     ("global4", (5, 9))])
def test_spmm_columns_bitwise(Ocean, name, ks):
    c, oc, L = model(Ocean, name)
    if name == "natl8":
        assert oc.rowintcon >= 0                       # the dense row is exercised
    if name == "global4":
        assert c.n == 96                               # two tiles per grid row, the second half full
    oc.setState(cf.synthetic_state(c, L))
    V = basis(c.nrows, max(ks))
    for shifted in (False, True):
        if shifted:
            oc.thetaInitStep(1e-3, 0.75)
            oc.thetaJacobian()
        else:
            oc.computeJacobian()
        want = np.stack([oc.applyMatrix(V[:, b]).copy() for b in range(max(ks))], axis=1)
        assert np.all(np.isfinite(want)) and np.count_nonzero(want) > 0
        for k in ks:
            for kb in (0, 2, 1) if k == max(ks) else (0,):
                W = spmm(oc, V[:, :k], kb)
                assert np.array_equal(bits(W), bits(want[:, :k])), (name, shifted, k, kb)
    oc.close()


# ---- 2. the Gram products -----------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("natl8", 6), ("gateway16", 6), ("global4", 5)])
def test_gram_against_exact_sums(Ocean, name, k):
    """global4 has 262,656 rows: k_gram's 256 row blocks take a second grid-stride pass and the
    last one is short (k = 5: one tile of the result is part-filled, and the fsums stay quick)"""
    c, oc, L = model(Ocean, name)
    N = c.nrows
    if name == "global4":
        assert N > 256 * 256 * 4 and N % (256 * 256) != 0
    V = basis(N, k, seed=2)
    V[:, 1] = 0.0
    V[:, 4] = 0.0
    V[oc.owned_rows()[-1], 4] = 1.0                    # a unit vector on the last owned row
    oc.setState(cf.synthetic_state(c, L))
    oc.projSetBasis(V)
    oc.thetaInitStep(1e-3, 0.75)
    oc.thetaJacobian()
    B = oc.diagB()
    W = spmm(oc, V)
    x = oc.getState()
    for what, (w, d) in {"VBV": (V, B), "VJ2V": (W, None), "Vx": (x, None), "VV": (V, None)}.items():
        got = dev_gram(oc, V, w, d)
        want, scale = gram(V, w, d)
        err = np.abs(got - want)
        print(f"{name} {what}: max err / bound {np.max(err / np.maximum(N * EPS * scale, 1e-300)):.3f}")
        assert np.all(err <= N * EPS * scale), what
        assert np.array_equal(bits(dev_gram(oc, V, w, d)), bits(got)), what
    G = dev_gram(oc, V, V)
    assert G[4, 4] == 1.0 and not G[1].any() and not G[:, 1].any()
    assert G[4, 0] == V[oc.owned_rows()[-1], 0]
    oc.close()


# ---- 3. init step and residual against the twin ---------------------------------------------------
def setup_pair(Ocean, oracle_lib, name, ortho, k=5, cfg=None):
    if cfg is None:
        c, oc, L = model(Ocean, name)
    else:
        c = cfg
        oc = Ocean(c, solver_params=SOLVER)
        L = oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    tw = ProjectedTwin(oracle_lib, c, L=L)
    V = basis(c.nrows, k, seed=4) * np.array([1.0, 3.0, 0.5, 2.0, 1.0, 1.5, 0.7, 1.0][:k])
    V[:, 1] += 0.5 * V[:, 0]
    if ortho:
        V = np.linalg.qr(V)[0]
    for m in (oc, tw):
        m.projSetBasis(V)
    return c, oc, tw, L, V


def absmv(tw, X):
    return csr_mm(tw.o.rowptr, tw.o.col, np.abs(tw.val2), np.abs(X))


@pytest.mark.parametrize("name", ["natl8", "gateway16"])
@pytest.mark.parametrize("dt,theta", [(1e-3, 0.75), (0.128, 1.0)])
@pytest.mark.parametrize("ortho", [False, True])
def test_init_step_and_residual_against_twin(Ocean, oracle_lib, name, dt, theta, ortho):
    c, oc, tw, L, V = setup_pair(Ocean, oracle_lib, name, ortho)
    N, k = c.nrows, V.shape[1]
    xn = cf.synthetic_state(c, L)
    y = gram(V, xn + 0.25 * cf.synthetic_state(c, L, seed=99))[0][:, 0] * 0.01
    for m in (oc, tw):
        m.setState(xn)
        m.projInitStep(dt, theta)
    nb = N * EPS
    e_yn = nb * gram(V, xn)[1][:, 0]
    e_Fn = nb * gram(V, tw.o.rhs(xn))[1][:, 0]
    e_VMV = nb * gram(V, V, tw.B)[1]
    # V^T (J2 V): the Gram bound plus the SpMV's 1e-13 |J2| |V| of test_gpu_parity.py under |V|^T
    e_VAV = nb * gram(V, tw.W)[1] + np.abs(V).T @ (1e-13 * absmv(tw, V))
    for what, e in (("y_n", e_yn), ("F_n", e_Fn), ("VMV", e_VMV), ("VAV", e_VAV)):
        got, want = oc.projGet(what), tw.projGet(what)
        print(f"{name} dt {dt} ortho {ortho} {what}: max err / bound {np.max(np.abs(got - want) / np.maximum(e, 1e-300)):.3f}")
        assert np.all(np.abs(got - want) <= e), what
    e_x = k * EPS * (np.abs(V) @ np.abs(y))            # the state V y carries k roundings per row
    if not ortho:                                      # y_n is the restriction of the state, not y
        for m in (oc, tw):
            m.projSetState(y)
            m.projInitStep(dt, theta)
        got, want = oc.projGet("y_n"), tw.projGet("y_n")
        assert np.all(np.abs(got - want) <= nb * gram(V, V @ y)[1][:, 0] + 2 * np.abs(V).T @ e_x)
        assert np.array_equal(oc.projGet("y"), y) and np.max(np.abs(got - y)) > 1e-3 * np.max(np.abs(y))
        for m in (oc, tw):
            m.setState(xn)
            m.projInitStep(dt, theta)
    for m in (oc, tw):
        m.projSetState(y)
    got, want = oc.projRHS(), tw.projRHS()
    x = V @ y
    F = tw.o.rhs(x)
    a, b = dt * (1 - theta), dt * theta
    # Both sides form the state V y with k roundings of 2^-53 per row, so the two states differ by at
    # most e_x, and F(x + d) - F(x) = J(x) d to first order: the two F differ by at most |J| e_x.
    val, _ = tw.o.jacobian(x)
    e_F = csr_mm(tw.o.rowptr, tw.o.col, np.abs(val), e_x[:, None])[:, 0]
    e_f = nb * gram(V, F)[1][:, 0] + np.abs(V).T @ e_F
    dy = np.abs(tw.yn - y)
    # r = a F_n + b f + sum_j VMV_ij (y_n - y)_j: the inputs' bounds carried through, and each term
    # passes through at most k + 4 roundings of 2^-53 on either side (the subtraction, the product,
    # k - 1 additions of the row sum, the scalings by a and b, the two final additions)
    parts = [a * e_Fn, b * nb * gram(V, F)[1][:, 0], b * (np.abs(V).T @ e_F), e_VMV @ dy, np.abs(tw.VMV) @ e_yn]
    e_r = (a * e_Fn + b * e_f + e_VMV @ dy + np.abs(tw.VMV) @ e_yn
           + (k + 4) * EPS * (np.abs(a * tw.Fn) + np.abs(b * gram(V, F)[0][:, 0]) + np.abs(tw.VMV) @ dy))
    print(f"{name} dt {dt} ortho {ortho} r: max err / bound {np.max(np.abs(got - want) / e_r):.3e}; the bound's parts "
          f"(F_n, V^T F, |J| e_x, VMV, y_n, roundings) as fractions: "
          + " ".join(f"{np.max(p / e_r):.2f}" for p in parts + [e_r - sum(parts)]))
    assert np.all(np.abs(got - want) <= e_r)
    # the prolonged state
    assert np.all(np.abs(oc.getState() - x) <= e_x)
    oc.close()


# ---- 4. the solve ------------------------------------------------------------------------------------
def test_solve_against_numpy(Ocean):
    c, oc, L = model(Ocean, "natl8")
    k = 5
    oc.setState(cf.synthetic_state(c, L))
    oc.projSetBasis(basis(c.nrows, k, seed=6))
    for dt, theta in ((1e-3, 0.75), (0.128, 1.0)):
        oc.projInitStep(dt, theta)
        A = oc.projGet("VAV")
        r = oc.projRHS()
        dy = oc.projSolve(r)
        ref = np.linalg.solve(A, r / dt / theta)
        cond = np.linalg.cond(A, np.inf)
        gap, bound = np.max(np.abs(dy - ref)), 32 * k * EPS * cond * np.max(np.abs(ref))
        print(f"dt {dt}: cond {cond:.3e} gap {gap:.3e} bound {bound:.3e}")
        assert gap <= bound
    oc.close()


def test_singular_vav_refused(Ocean):
    c, oc, L = model(Ocean, "natl8")
    V = basis(c.nrows, 4, seed=7)
    V[:, 3] = V[:, 1]
    oc.setState(cf.synthetic_state(c, L))
    oc.projSetBasis(V)
    with pytest.raises(_lib.IemicError, match=r"rc=-34.*singular: pivot 3 of 4 is zero"):
        oc.projInitStep(1e-3, 0.75)
    with pytest.raises(_lib.IemicError, match=r"rc=-71.*iemic_proj_init_step"):
        oc.projRHS()
    oc.close()


# ---- 5. fused equals composed -----------------------------------------------------------------------
def test_fused_step_equals_composed(Ocean):
    c = transient_config()
    a, b = Ocean(c, solver_params=SOLVER), Ocean(c, solver_params=SOLVER)
    L = a.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    V = basis(c.nrows, 5, seed=8)
    y0 = 1e-3 * np.arange(1.0, 6.0)
    pert = StochasticThetaStepper.noise_block(11, 1, c.m)
    for oc in (a, b):
        oc.setState(cf.synthetic_state(c, L, amp_ts=1e-3))
        oc.projSetBasis(V)
        oc.projSetState(y0)
        oc.projStochasticInitStep(1e-3, 0.75, 0.5, pert)
    x0 = a.getState()
    r_first = None
    for it in range(2):
        info = a.projNewtonStep()
        r = b.projRHS()
        r_first = r.copy() if r_first is None else r_first
        dy = b.projSolve(r)
        b.projSetState(b.projGet("y") - dy)
        r1 = b.projRHS()
        assert np.array_equal(bits(a.projGet("y")), bits(b.projGet("y")))
        assert np.array_equal(bits(a.projGet("r")), bits(r1))
        assert np.array_equal(bits(a.getState()), bits(b.getState()))
        assert info.norm_dx == np.max(np.abs(dy)) and info.norm_dx > 0
        assert abs(info.norm_f1 - np.linalg.norm(r1)) <= 4 * EPS * np.linalg.norm(r1)
    a.projRestore()
    assert np.array_equal(bits(a.projGet("y")), bits(y0)) and not np.array_equal(bits(b.projGet("y")), bits(y0))
    ra = a.projRHS()                                   # consistent with the restored state: the first residual
    assert np.array_equal(bits(ra), bits(r_first))
    assert np.array_equal(bits(a.getState()), bits(x0)) and not np.array_equal(bits(b.getState()), bits(x0))
    a.close()
    b.close()


# ---- 6. the noise ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["natl8", "gateway16"])
def test_noise_is_the_restricted_field(Ocean, name):
    dt, theta, sigma = 1e-3, 0.75, 0.37
    c, oc, L = model(Ocean, name)
    V = basis(c.nrows, 5, seed=9)
    pert = StochasticThetaStepper.noise_block(11, 2, c.m)
    xn = cf.synthetic_state(c, L)
    y = 1e-3 * np.arange(1.0, 6.0)
    oc.setState(xn)
    oc.projSetBasis(V)
    par = {n_: oc.getPar(n_) for n_ in PAR_INDEX}
    top = L[c.l, 1:c.m + 1, 1:c.n + 1]
    field, hit = noise(c, forcing_column(c, top, par), top, oc.rowintcon, dt, sigma, pert)

    def residual(init):
        oc.setState(xn)
        init()
        oc.projSetState(y)
        return oc.projRHS().copy()

    plain = residual(lambda: oc.projInitStep(dt, theta))
    assert not oc.projGet("G").any()
    noisy = residual(lambda: oc.projStochasticInitStep(dt, theta, sigma, pert))
    G = oc.projGet("G")
    want, scale = gram(V, field)
    assert hit.sum() > 0 and np.all(G != 0)
    assert np.all(np.abs(G - want[:, 0]) <= c.nrows * EPS * scale[:, 0])
    assert np.array_equal(bits(noisy), bits(plain + G))
    assert np.array_equal(bits(residual(lambda: oc.projStochasticInitStep(dt, theta, 0.0, pert))), bits(plain))
    residual(lambda: oc.projStochasticInitStep(dt, theta, sigma, pert))
    assert np.array_equal(bits(residual(lambda: oc.projInitStep(dt, theta))), bits(plain))
    oc.close()


# ---- 7. the stepper ------------------------------------------------------------------------------------
def test_stepper_against_twin(Ocean, oracle_lib):
    """Three adaptive steps from rest on test_oceantransient.xml's model, k = 5, sigma = 0.5 and a
    fixed pert_source, against the twin driven by the same stepper class: equal dt sequences and
    Newton counts, and ||y_gpu - y_twin||_inf <= (time steps taken, rejected ones included) *
    (Newton tolerance): both sides solve each reduced time step to that tolerance."""
    c, oc, tw, L, V = setup_pair(Ocean, oracle_lib, None, ortho=True, cfg=transient_config())
    p = dict(PARAMS, **{"sigma": 0.5, "number of time steps": 3})

    def source(block, m):
        return StochasticThetaStepper.noise_block(11, block, m)

    tw.cfg = c
    runs = []
    for m in (oc, tw):
        m.setState(np.zeros(c.nrows))
        st = StochasticProjectedThetaStepper(m, V, p, pert_source=source)
        assert st.run() == 0
        runs.append(st)
    g, t = runs
    for r, q in zip(g.history, t.history):
        print(f"step {r.step} dt {r.dt:g} steps() {r.newton_steps}/{q.newton_steps} |y| {r.norm_x:.12e} twin {q.norm_x:.12e}")
    assert [r.dt for r in g.history] == [r.dt for r in t.history] and g.rejected == t.rejected
    assert [r.newton_steps for r in g.history] == [r.newton_steps for r in t.history]
    assert g.draws == t.draws == 3 + len(g.rejected)
    taken = len(g.history) + len(g.rejected)
    gap = np.max(np.abs(g.y - t.y))
    print(f"||y_gpu - y_twin||_inf = {gap:.3e} (bound {taken * g.tol:.1e}), ||y|| = {np.linalg.norm(g.y):.6e}")
    assert np.linalg.norm(g.y) > 0 and gap <= taken * g.tol
    oc.close()


# ---- 8. two latitude bands -----------------------------------------------------------------------------
def test_two_latitude_bands(Ocean):
    dt, theta, k = 1e-3, 0.75, 5
    c = cf.preset("gateway16")
    one = Ocean(c)
    L0 = cf.landmask(c)
    L = one.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    N = c.nrows
    V = basis(N, k, seed=10)
    x = cf.synthetic_state(c, L)
    y = 1e-3 * np.arange(1.0, 6.0)

    def run(oc):
        oc.setState(x)
        oc.projSetBasis(V)
        F0 = oc.computeRHS().copy()
        oc.projInitStep(dt, theta)
        W = spmm(oc, V)                                   # J2 V: the init step left J2
        B = oc.diagB()
        oc.projSetState(y)
        F1 = oc.computeRHS().copy()
        out = dict(W=W, VAV=oc.projGet("VAV"), VMV=oc.projGet("VMV"), r=oc.projRHS().copy(), rows=oc.owned_rows(),
                   B=B, F0=F0, F1=F1, yn=oc.projGet("y_n"), Fn=oc.projGet("F_n"))
        oc.close()
        return out

    ref = run(one)
    res = run_bands(2, lambda r, group: run(Ocean(c, landm=L0, local_group=group, rank=r, nranks=2, npx=1)))
    W = np.full((N, k), np.nan)
    for r in res:
        W[r["rows"]] = r["W"][r["rows"]]
    assert np.array_equal(bits(W), bits(ref["W"]))
    nb = N * EPS
    # W is the same on one rank and on two, bit for bit, so both sides' VAV are sums of the same
    # products: each within bound 2 of the exactly rounded sum (likewise VMV)
    xVAV, sVAV = gram(V, ref["W"])
    xVMV, sVMV = gram(V, V, ref["B"])
    e_VAV, e_VMV = nb * sVAV, nb * sVMV
    for r in res + [ref]:
        assert np.all(np.abs(r["VAV"] - xVAV) <= e_VAV) and np.all(np.abs(r["VMV"] - xVMV) <= e_VMV)
    # r: each side's Gram products within bound 2 of the exact sums, so twice the bounds between them,
    # carried through r = a F_n + b V^T F + VMV (y_n - y) with (k + 4) roundings of its terms
    a, b = dt * (1 - theta), dt * theta
    dy = np.abs(ref["yn"] - y)
    e_r = 2 * (a * nb * gram(V, ref["F0"])[1][:, 0] + b * nb * gram(V, ref["F1"])[1][:, 0] + e_VMV @ dy
               + np.abs(ref["VMV"]) @ (nb * gram(V, x)[1][:, 0]))
    e_r += (k + 4) * EPS * (np.abs(a * ref["Fn"]) + np.abs(b * gram(V, ref["F1"])[0][:, 0]) + np.abs(ref["VMV"]) @ dy)
    print(f"bands: r max err / bound {np.max(np.abs(res[0]['r'] - ref['r']) / e_r):.3f}")
    assert np.all(np.abs(res[0]["r"] - ref["r"]) <= e_r)
    for key in ("VAV", "VMV", "r"):
        assert np.array_equal(bits(res[0][key]), bits(res[1][key])), key


# ---- 9. refusals -----------------------------------------------------------------------------------------
def test_refusals_by_name(Ocean):
    c, oc, L = model(Ocean, "natl8")
    lib = _lib.lib()
    oc.setState(cf.synthetic_state(c, L))
    for call, fn in (("iemic_proj_restrict_state", oc.projRestrictState), ("iemic_proj_set_state", lambda: oc.projSetState([1.0])),
                     ("iemic_proj_init_step", lambda: oc.projInitStep(1e-3, 0.75)), ("iemic_proj_rhs", oc.projRHS),
                     ("iemic_proj_solve", lambda: oc.projSolve([1.0])), ("iemic_proj_newton_step", oc.projNewtonStep),
                     ("iemic_proj_restore", oc.projRestore),
                     ("iemic_proj_init_step", lambda: oc.projStochasticInitStep(1e-3, 0.75, 1.0, np.zeros(c.m))),
                     ("iemic_proj_get", lambda: oc.projGet("y"))):
        with pytest.raises(_lib.IemicError, match=rf"rc=-71.*{call}: no basis set \(iemic_proj_set_basis\)"):
            fn()
    V = basis(c.nrows, 3, seed=11)
    Vc = cols(V)
    for k in (0, 65, -1):
        assert lib.iemic_proj_set_basis(oc._h, _lib.ptr(Vc), k) == -22 and b"k = " in lib.iemic_last_error()
    assert lib.iemic_proj_set_basis(oc._h, None, 3) == -22 and b"V is NULL" in lib.iemic_last_error()
    bad = V.copy()
    bad[7, 2] = np.inf
    with pytest.raises(_lib.IemicError, match=r"rc=-22.*V\[7, 2\] is not finite"):
        oc.projSetBasis(bad)
    with pytest.raises(_lib.IemicError, match="V has shape"):
        oc.projSetBasis(V[:-1])
    oc.projSetBasis(V)
    for call, fn in (("iemic_proj_rhs", oc.projRHS), ("iemic_proj_solve", lambda: oc.projSolve(np.ones(3))),
                     ("iemic_proj_newton_step", oc.projNewtonStep), ("iemic_proj_restore", oc.projRestore)):
        with pytest.raises(_lib.IemicError, match=rf"rc=-71.*{call}: no time step initialised \(iemic_proj_init_step\)"):
            fn()
    good = np.zeros(c.m)
    nanp = good.copy()
    nanp[2] = np.nan
    for dt, theta, word in ((1e-3, 0.0, "theta"), (1e-3, 1.5, "theta"), (1e-3, float("nan"), "theta"), (0.0, 0.75, "dt"),
                            (-1.0, 0.75, "dt")):
        with pytest.raises(_lib.IemicError, match=rf"rc=-22.*{word}"):
            oc.projInitStep(dt, theta)
        with pytest.raises(_lib.IemicError, match=rf"rc=-22.*{word}"):
            oc.projStochasticInitStep(dt, theta, 1.0, good)
    for sigma, pert, word in ((-1.0, good, "sigma"), (float("inf"), good, "sigma"), (1.0, nanp, r"pert\[2\]")):
        with pytest.raises(_lib.IemicError, match=rf"rc=-22.*{word}"):
            oc.projStochasticInitStep(1e-3, 0.75, sigma, pert)
    assert lib.iemic_proj_init_step_noise(oc._h, 1e-3, 0.75, 1.0, None) == -22 and b"pert" in lib.iemic_last_error()
    with pytest.raises(_lib.IemicError, match="pert has 7 entries"):
        oc.projStochasticInitStep(1e-3, 0.75, 1.0, np.zeros(c.m - 1))
    with pytest.raises(_lib.IemicError, match="y has 2 entries"):
        oc.projSetState(np.zeros(2))
    with pytest.raises(_lib.IemicError, match=r"rc=-22.*unknown quantity 'z'"):
        oc.projGet("z")
    with pytest.raises(_lib.IemicError, match=r"rc=-71.*no time step initialised"):
        oc.projRHS()                                   # nothing was initialised by the refused calls
    ms = C.c_double()
    oc.computeJacobian()
    for k in (0, 65):
        assert lib.iemic_time_spmm(oc._h, k, 1, C.byref(ms)) == -22 and b"iemic_time_spmm: k = " in lib.iemic_last_error()
    assert oc.time_spmm(5, nrep=1) > 0.0
    oc.projClear()
    with pytest.raises(_lib.IemicError, match=r"rc=-71.*no basis set"):
        oc.projInitStep(1e-3, 0.75)
    oc.close()


# ---- 10. no preconditioner, no Krylov solver ---------------------------------------------------------------
def solver_calls(oc):
    """(krylov_solve calls, prec_compute calls) of the context since its creation, counted inside
    the library, whichever entry point made them"""
    L = _lib.lib()
    L.iemic_test_solver_calls.restype = C.c_int
    L.iemic_test_solver_calls.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    out = (C.c_int64 * 2)()
    _lib.check(L.iemic_test_solver_calls(oc._h, out), "iemic_test_solver_calls")
    return out[0], out[1]


def test_no_preconditioner_and_no_krylov(Ocean):
    c = transient_config()
    oc = Ocean(c, solver_params=SOLVER)
    L = oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    x0 = cf.synthetic_state(c, L, amp_ts=1e-3)
    oc.setState(x0)
    V = np.linalg.qr(basis(c.nrows, 5, seed=12))[0]
    assert oc.active_cells() == 0 and solver_calls(oc) == (0, 0)   # nothing set up, nothing solved
    st = StochasticProjectedThetaStepper(oc, V, dict(PARAMS, **{"sigma": 0.5, "noise seed": 3, "number of time steps": 2}))
    assert st.run() == 0 and len(st.history) == 2
    assert oc.active_cells() == 0 and solver_calls(oc) == (0, 0)
    # the counters do count: one full-space Newton iteration sets up once and solves once
    oc.setState(x0)
    oc.preProcess()
    oc.thetaInitStep(1e-3, 0.75)
    oc.thetaNewtonStep()
    assert solver_calls(oc) == (1, 1)
    # with a preconditioner set up, a projected run leaves it as it is, bit for bit
    na = oc.active_cells()
    assert na > 0
    x = oc.getState()
    z = oc.applyPrecon(x).copy()
    st2 = StochasticProjectedThetaStepper(oc, V, dict(PARAMS, **{"sigma": 0.5, "noise seed": 3, "number of time steps": 1}))
    assert st2.run() == 0
    assert oc.active_cells() == na and solver_calls(oc) == (1, 1)
    assert np.array_equal(bits(oc.applyPrecon(x)), bits(z))
    oc.close()
