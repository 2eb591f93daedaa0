"""The ocean's IDR(s) (csrc/idrs.hip) against the plain numpy IDR(s) of tests/krylov_ref.py.

With x0 = 0, the shadow space of k_idr_random (restated by idr_shadow_raw) and the 'maintain
the convergence' rule for omega, the k-th iterate of bi-orthogonal IDR(s) is a function of
(A, M, b) alone.  The device is run with tolerance 0 and "FGMRES iterations" = k, so that it
returns exactly its k-th iterate, at the k that enter each branch of the loop; the iteration
count, the iterate, the true residual and the recursive (implicit) residual are compared.
A solver that merely converges -- with a wrong omega, a gamma loop one index off, a dropped
bi-orthogonalisation term -- fails here.

Tolerances are 100 x the spread between two correct references (float64 / longdouble, and with
a preconditioner M / M perturbed by 1e-9), at least 1e-12: test_idr_reference_spread recomputes
the spreads and holds the constants to them.
"""
import numpy as np
import pytest

from krylov_ref import IDR_CAP as CAP
from krylov_ref import IDR_KINDS, IDR_SEED_OCEAN, idr_kinds, idr_shadow_raw, idrs_ref
from krylov_ref import idr_steps as steps_of
from test_gpu_krylov import RHO_MIN, Ocean, bits, context, rel, relres, solve, system  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [("test6x6x4", 1), ("test6x6x4", 4), ("test6x6x4", 8), ("gateway16", 4)]
# Preconditioner 0: the default angle and 0.999 (fires at both omega steps).  1e-6 (never
# fires) is compared with the block Gauss-Seidel preconditioner only: the plain
# minimal-residual omega of the unpreconditioned operator is nearly zero and two correct
# references part by 2e-2 at the second omega step (tests/test_krylov_ref.py).
ANGLES = {0: (0.7, 0.999), 2: (0.7, 0.999, 1e-6)}

# 100 x the largest measured spread (test_idr_reference_spread's docstring), by the part of
# the iteration a step lies in: k = 1, the rest of the first cycle with its omega step
# (k <= s + 1), the second cycle (k <= 2 s + 2)
TOL = {0: ((2.9e-12, 1e-12), (7.9e-11, 7.6e-11), (9.9e-10, 1.9e-9)),         # (iterate, residual)
       2: ((1.3e-5, 4.4e-5), (1.7e-5, 1.2e-6), (3.7e-6, 8.1e-6))}
# steps whose float64-longdouble spread is over the cap, per (grid, s, preconditioner, angle):
# the residual there is 5e-12 and 1e-12 of ||b||, the iteration has converged to rounding
DROPPED = {("test6x6x4", 8, 2, 0.7): (17, 18)}


def kept(name, s, prec, angle):
    return [k for k in steps_of(s) if k not in DROPPED.get((name, s, prec, angle), ())]


def tol_of(prec, s, k):
    """(iterate, residual)"""
    return TOL[prec][0 if k == 1 else 1 if k <= s + 1 else 2]


_CTX, _REF = {}, {}


def ctx(Ocean, oracle_lib, name, prec):
    """one context per (grid, preconditioner) for the module; with the block GS built"""
    if (name, prec) not in _CTX:
        oc = context(Ocean, system(oracle_lib, name), Preconditioner=prec, Solver="IDR")
        if prec:
            oc.buildPreconditioner()
        _CTX[name, prec] = oc
    return _CTX[name, prec]


def perturbation(n):
    return 1.0 + 1e-9 * np.where(np.random.default_rng(7).random(n) < 0.5, -1.0, 1.0)


def reference(s_, oc, name, s, prec, angle, dtype=np.longdouble, perturbed=False, steps=None):
    """idrs_ref on the oracle's Jacobian; computed once per case and left unchanged"""
    steps = steps or 2 * s + 2
    key = (name, s, prec, angle, np.dtype(dtype).name, perturbed, steps)
    if key not in _REF:
        A = s_["AL"] if dtype == np.longdouble else s_["A64"]
        M = None
        if prec:
            M = oc.applyPrecon
            if perturbed:
                xi = perturbation(s_["c"].nrows)
                M = lambda v: oc.applyPrecon(v) * xi
        P = idr_shadow_raw(np.arange(s_["c"].nrows), s, IDR_SEED_OCEAN)
        _REF[key] = idrs_ref(A, M, s_["b"], P, s, steps, angle, dtype)
    return _REF[key]


def spread(base, other, k):
    dx = rel(other.x_steps[k - 1], base.x_steps[k - 1])
    dr = float(abs(other.rho[k - 1] - base.rho[k - 1]) / base.rho[k - 1])
    return dx, dr


def idr_opts(s, k, angle, **more):
    return {"Solver": "IDR", "IDR s": s, "IDR angle": angle, "IDR replace residuals": False,
            "FGMRES tolerance": 0.0, "FGMRES iterations": k, "FGMRES restarts": 0, **more}


def check_steps(s_, oc, ref, name, s, prec, angle, ks, label, **more):
    """the device's k-th iterate for every k of ks; every figure is printed before anything is
    asserted.  Residuals are compared relatively where the reference's is at least RHO_MIN."""
    bad, infos = [], {}
    for k in ks:
        x, info = solve(oc, s_["b"], **idr_opts(s, k, angle, **more))
        infos[k] = info
        xr, rho, rec = ref.x_steps[k - 1], float(ref.rho[k - 1]), float(ref.rec[k - 1])
        e_x = rel(x, xr)
        e_true = abs(relres(s_, x) - rho) / rho
        e_impl = abs(info.implicit_rel_res - rec) / rec
        t, tr = tol_of(prec, s, k)
        print(f"{label} k={k} {ref.kind[k - 1]}: iters {info.iters} rho {rho:.6e} x {e_x:.2e} "
              f"true {e_true:.2e} implicit {e_impl:.2e} reorth {info.reorth} (tol {t:.1e} {tr:.1e})")
        if info.iters != k:
            bad.append((k, "iters", info.iters))
        if not e_x <= t:
            bad.append((k, "iterate", e_x))
        if rho >= RHO_MIN and not e_true <= tr:
            bad.append((k, "true residual", e_true))
        if rec >= RHO_MIN and not e_impl <= tr:
            bad.append((k, "implicit residual", e_impl))
    assert not bad, bad
    return infos


def expect_fired(ref, angle):
    """what the angle setting is there to force; asserted on the reference so that the case
    cannot go vacuous"""
    fired = [f for _, _, f, _ in ref.omega]
    assert len(fired) == 2
    if angle == 0.999:
        assert fired == [True, True], ref.omega
    if angle == 1e-6:
        assert fired == [False, False], ref.omega
    return fired


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("name,s", CASES)
def test_idr_iterates(oracle_lib, Ocean, name, s, prec):
    """idrs at k = 1, s, s + 1, s + 2, 2 s + 1, 2 s + 2 and the angle settings of ANGLES against
    the longdouble reference.  Preconditioner 2: M = applyPrecon of the same context (idrs
    calls prec_apply on full-length vectors, the route applyPrecon takes).
    864 rows: one partial 256-thread block per reduction slot; 24,576 rows: 96 blocks."""
    s_ = system(oracle_lib, name)
    oc = ctx(Ocean, oracle_lib, name, prec)
    kinds = set()
    for angle in ANGLES[prec]:
        ref = reference(s_, oc, name, s, prec, angle)
        fired = expect_fired(ref, angle)
        print(f"{name} s={s} prec {prec} angle {angle}: omega steps (k, rho, fired, omega) {ref.omega}")
        ks = kept(name, s, prec, angle)
        kinds |= idr_kinds(ref, ks)
        check_steps(s_, oc, ref, name, s, prec, angle, ks, f"{name} s={s} prec {prec} angle {angle} fired {fired}")
    # a step of each kind is compared in every (grid, s, preconditioner) case
    assert IDR_KINDS <= kinds


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("name,s", CASES)
def test_idr_reference_spread(oracle_lib, Ocean, name, s, prec):
    """How far two correct IDR(s) runs are apart at the compared steps: (a) the float64 and the
    longdouble reference, (b) with Preconditioner 2, two longdouble references whose M differs
    by a fixed 1e-9 relative diagonal factor (applyPrecon is linear to about 1e-9 only).
    100 x the larger must stay within TOL, and no kept step's float64-longdouble spread may
    exceed the cap of 1e-8 (the cap is on the method's own instability; the spread from M is
    the preconditioner's and as large at k = 1 as later).
    Measured (iterate, residual), maximum over the grids, s and angles:
                                               k = 1             first cycle       second cycle
      Preconditioner 0  float64 vs longdouble  2.9e-14, 1.6e-15  7.9e-13, 7.5e-13  9.8e-12, 1.8e-11
      Preconditioner 2  float64 vs longdouble  1.9e-14, 6.4e-14  5.4e-13, 4.7e-15  4.0e-9, 2.1e-14
      Preconditioner 2  perturbed M            1.3e-7, 4.4e-7    1.7e-7, 1.1e-8    3.7e-8, 8.0e-8
    (gateway16 carries the perturbed-M figures of k = 1 and the first cycle; test6x6x4: 5.3e-9,
    5.0e-8 and 1.3e-8, 1.1e-8).  Over the cap and dropped: k = 17, 18 of test6x6x4, s = 8,
    Preconditioner 2, angle 0.7 (4.2e-8, 2.2e-8 at residuals of 5e-12 and 1e-12).
    The device's own distance from the longdouble reference on the MI355X: Preconditioner 0
    within the float64 reference's; Preconditioner 2 at most 3.7e-9 on the iterate."""
    s_ = system(oracle_lib, name)
    oc = ctx(Ocean, oracle_lib, name, prec)
    bad = []
    for angle in ANGLES[prec]:
        base = reference(s_, oc, name, s, prec, angle)
        others = [("float64", reference(s_, oc, name, s, prec, angle, np.float64))]
        if prec:
            others.append(("perturbed", reference(s_, oc, name, s, prec, angle, perturbed=True)))
        for k in kept(name, s, prec, angle):
            for tag, other in others:
                dx, dr = spread(base, other, k)
                if base.rho[k - 1] < RHO_MIN:
                    dr = 0.0
                print(f"{name} s={s} prec {prec} angle {angle} k={k} {base.kind[k - 1]} {tag}: "
                      f"rho {float(base.rho[k - 1]):.3e} spread x {dx:.2e} rho {dr:.2e}")
                if tag == "float64" and max(dx, dr) > CAP:
                    bad.append((angle, k, tag, "over the cap", dx, dr))
                if 100 * dx > tol_of(prec, s, k)[0] or 100 * dr > tol_of(prec, s, k)[1]:
                    bad.append((angle, k, tag, "tolerance does not cover", dx, dr))
    assert not bad, bad


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("name,s", [("test6x6x4", 4), ("gateway16", 4)])
def test_idr_residual_replacement(oracle_lib, Ocean, name, s, prec):
    """"IDR replace residuals" with tolerance 0: tolb / mp is 0, so trueres is set at every
    step and r = b - A x replaces r at each omega step whose residual is below ||b||.  In
    exact arithmetic nothing changes: the same iterates, and last_solve.reorth counts the omega
    steps (up to k) at which the reference's ||r|| < ||b||."""
    s_ = system(oracle_lib, name)
    oc = ctx(Ocean, oracle_lib, name, prec)
    ref = reference(s_, oc, name, s, prec, 0.7)
    ks = kept(name, s, prec, 0.7)
    infos = check_steps(s_, oc, ref, name, s, prec, 0.7, ks, f"{name} s={s} prec {prec} replace",
                        **{"IDR replace residuals": True})
    om = [q for q, *_ in ref.omega]
    assert all(abs(float(ref.rec[q - 1]) - 1.0) > 1e-6 for q in om)         # no count on a knife edge
    if prec:
        assert all(ref.rec[q - 1] < 1 for q in om)                          # both replace
    for k in ks:
        want = sum(1 for q in om if q <= k and ref.rec[q - 1] < 1)
        assert infos[k].reorth == want, (k, infos[k].reorth, want)
    x, info = solve(oc, s_["b"], **idr_opts(s, ks[-1], 0.7))
    assert info.reorth == 0


def crossing(ref, s, omega):
    """the first step k >= 2 whose recursive residual is a new minimum by a factor 2 and that
    is (omega) an omega step, or else a column of a cycle that is not its last"""
    for k in range(2, len(ref.rec) + 1):
        col = (k - 1) % (s + 1)
        if (col == s) != omega or (not omega and col == s - 1):
            continue
        lo = min(ref.rec[:k - 1])
        if ref.rec[k - 1] < 0.5 * lo:
            return k, float(np.sqrt(ref.rec[k - 1] * lo))
    return None


@pytest.mark.parametrize("omega", [False, True], ids=["in-cycle", "omega-step"])
@pytest.mark.parametrize("name", ["test6x6x4", "gateway16"])
def test_idr_converges_one_matvec_late(oracle_lib, Ocean, name, omega):
    """The convergence test of a step rides in the next step's multi-dot.  A tolerance at the
    geometric mean of two reference residuals rec_k < min(rec_1 .. rec_{k-1}) (a factor 2
    apart at least, so rounding cannot move the crossing) must stop the device with
    iters == k and the k-th iterate: inside a cycle that is the `done` path, whose pending
    step is computed but not applied; at an omega step the test at the top of the next cycle.
    Block Gauss-Seidel preconditioner (the unpreconditioned residuals grow at first)."""
    s, prec = 4, 2
    s_ = system(oracle_lib, name)
    oc = ctx(Ocean, oracle_lib, name, prec)
    ref = reference(s_, oc, name, s, prec, 0.7, steps=3 * (s + 1))
    hit = crossing(ref, s, omega)
    print(f"{name}: rec", " ".join(f"{float(r):.2e}" for r in ref.rec), "crossing", hit)
    assert hit is not None
    k, tol = hit
    x, info = solve(oc, s_["b"], **idr_opts(s, 1000, 0.7, **{"FGMRES tolerance": tol}))
    e_x = rel(x, ref.x_steps[k - 1])
    e_impl = abs(info.implicit_rel_res - float(ref.rec[k - 1])) / float(ref.rec[k - 1])
    print(f"{name}: stop at k={k} tol {tol:.3e}: iters {info.iters} x {e_x:.2e} implicit {e_impl:.2e}")
    assert info.iters == k
    t, tr = tol_of(prec, s, k)
    assert e_x <= t
    assert ref.rec[k - 1] < RHO_MIN or e_impl <= tr      # as everywhere: residuals above RHO_MIN only
    assert info.converged == 1


@pytest.mark.parametrize("prec", [0, 2])
def test_idr_zero_rhs(oracle_lib, Ocean, prec):
    """b = 0: converged, no iteration, x = 0 (after a solve that left another x behind)."""
    s_ = system(oracle_lib, "test6x6x4")
    oc = ctx(Ocean, oracle_lib, "test6x6x4", prec)
    x, _ = solve(oc, s_["b"], **idr_opts(4, 5, 0.7))
    assert np.any(x != 0)
    x, info = solve(oc, np.zeros_like(s_["b"]), **idr_opts(4, 5, 0.7))
    assert info.converged == 1 and info.iters == 0
    np.testing.assert_array_equal(bits(x), bits(np.zeros_like(x)))
