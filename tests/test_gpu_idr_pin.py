"""IDR(s) of the ocean and of the coupled model, bitwise against recorded iterates.

csrc/idrs_core.h holds the one IDR(s) loop that idrs (csrc/idrs.hip) and iemic_coupled_solve
(csrc/coupled_krylov.hip) run over their two vector spaces.  The CPU references of
test_gpu_idr.py and test_gpu_coupled_krylov.py allow 1e-12 and more; a change of the order in
which the host reads the reductions must not move a bit.  tests/golden/idr_parent_iterates.npz
holds what the two separate solvers returned before they were folded, recorded by record()
twice in separate processes on an MI355X (the two recordings agreed bitwise): x, iters, reorth
and implicit_rel_res with tolerance 0, Preconditioner 0, angle 0.7 and the step cap at
k = 1, s + 1, s + 2, 2 s + 3 (a gamma step, the first omega step, the step after it, the second
cycle), for the ocean on natl8 (s = 1, 4) and the coupled model on coupled_natl8s (s = 1, 4, 8;
s = 4 with residual replacement as well).  The right-hand sides are stored with the iterates.

The guards and the stopping rule that the coupled solve took over from the ocean's are
checked at the end.
"""
import os

import numpy as np
import pytest

import test_gpu_coupled_krylov as ck
import test_gpu_krylov as ok
from test_gpu_krylov import Ocean, bits  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "idr_parent_iterates.npz")
OCEAN, COUPLED = "natl8", "coupled_natl8s"


def caps(s):
    return (1, s + 1, s + 2, 2 * s + 3)


# (key, model, s, k, replace)
CASES = ([(f"ocean_s{s}_k{k}", "ocean", s, k, False) for s in (1, 4) for k in caps(s)]
         + [(f"coupled_s{s}_k{k}", "coupled", s, k, False) for s in (1, 4, 8) for k in caps(s)]
         + [(f"coupled_s4_k{k}_replace", "coupled", 4, k, True) for k in caps(4)])


def opts(s, k, replace):
    return {"Solver": "IDR", "IDR s": s, "IDR angle": 0.7, "IDR replace residuals": replace, "Preconditioner": 0,
            "FGMRES tolerance": 0.0, "FGMRES iterations": k, "FGMRES restarts": 0}


_MODELS = {}


def model(which, orc, Ocean):
    """(the model, its solve, the right-hand side of the reference tests); once per module"""
    if which not in _MODELS:
        if which == "ocean":
            s_ = ok.system(orc, OCEAN)
            _MODELS[which] = (ok.context(Ocean, s_, Preconditioner=0, Solver="IDR"), ok.solve, s_["b"])
        else:
            s_ = ck.system(COUPLED)
            _MODELS[which] = (ck.fresh(COUPLED)[-1], ck.solve, s_["b"])
    return _MODELS[which]


def run(which, orc, Ocean, b, s, k, replace):
    m, solve, _ = model(which, orc, Ocean)
    x, info = solve(m, b, **opts(s, k, replace))
    return x, np.array([info.iters, info.reorth, info.implicit_rel_res], dtype=np.float64)


def record(orc, Ocean):
    """every case's (x, [iters, reorth, implicit_rel_res]) and the two right-hand sides"""
    out = {f"b_{w}": np.array(model(w, orc, Ocean)[2]) for w in ("ocean", "coupled")}
    for key, which, s, k, replace in CASES:
        out[f"{key}_x"], out[f"{key}_info"] = run(which, orc, Ocean, out[f"b_{which}"], s, k, replace)
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("key,which,s,k,replace", CASES, ids=[c[0] for c in CASES])
def test_idr_iterate_is_the_recorded_one(oracle_lib, Ocean, golden, key, which, s, k, replace):
    """x bitwise, iters, reorth and implicit_rel_res equal to the recording."""
    x, info = run(which, oracle_lib, Ocean, golden[f"b_{which}"], s, k, replace)
    gx, gi = golden[f"{key}_x"], golden[f"{key}_info"]
    print(f"{key}: iters {info[0]:.0f} ({gi[0]:.0f}) reorth {info[1]:.0f} ({gi[1]:.0f}) implicit {info[2]!r} "
          f"({gi[2]!r}) differing entries of x {int(np.count_nonzero(bits(x) != bits(gx)))}")
    assert gi[0] == k and np.all(np.isfinite(gx)) and np.any(gx != 0)
    assert np.array_equal(x, gx)
    assert info[0] == gi[0] and info[1] == gi[1] and info[2] == gi[2]


def test_recorded_right_hand_sides_are_the_reference_tests(oracle_lib, Ocean, golden):
    """The recording used the right-hand sides of the reference tests; they are rebuilt on the
    host, so they are compared to rounding only (the solves above take the stored ones)."""
    for w in ("ocean", "coupled"):
        b = model(w, oracle_lib, Ocean)[2]
        assert np.allclose(golden[f"b_{w}"], b, rtol=1e-12, atol=1e-12 * np.max(np.abs(b)))


# ---- the coupled solve's guards and stopping rule ------------------------------------------------
def test_coupled_idr_guards(oracle_lib, Ocean):
    """A NaN in the right-hand side is an error with a message, not a zero return with NaN
    results; b = 0 converges at once with x = 0."""
    from iemic import _lib
    cm, solve, b = model("coupled", oracle_lib, Ocean)
    bad = np.array(b)
    bad[bad.size // 3] = np.nan
    with pytest.raises(_lib.IemicError) as e:
        solve(cm, bad, **opts(4, 10, False))
    print("NaN right-hand side:", e.value)
    assert "rc=-34" in str(e.value) and "non-finite" in str(e.value)      # IEMIC_ERANGE, with its message
    x, info = solve(cm, np.zeros_like(b), **opts(4, 10, False))
    assert info.converged == 1 and info.iters == 0
    np.testing.assert_array_equal(bits(x), bits(np.zeros_like(x)))
    x, info = solve(cm, b, **opts(4, 1, False))           # the model still solves
    assert info.iters == 1 and np.all(np.isfinite(x))


def test_coupled_idr_stops_at_the_tolerance(oracle_lib, Ocean):
    """The counterpart of test_gpu_idr.py's test_idr_converges_one_matvec_late on
    coupled_natl8s, s = 4, Preconditioner 0.  k: the step of the first two cycles (the steps
    whose tolerance test_gpu_coupled_krylov.py derives) at which the reference's implicit
    residual drops furthest below all earlier ones, the start ||r|| = ||b|| among them (the
    unpreconditioned residuals grow at first); at least 10 % below, so that rounding cannot move
    the crossing.  A tolerance at the geometric mean of the two stops the solve with
    iters == k and the k-th iterate: the test of step k rides in the multi-dot after the next
    operator application, and that pending step is discarded."""
    s = 4
    s_ = ck.system(COUPLED)
    cm = model("coupled", oracle_lib, Ocean)[0]
    ref = ck.idr_reference(s_, s, 0, 0.7)
    rec = [1.0] + [float(r) for r in ref.rec]
    k = max(range(2, 2 * s + 3), key=lambda q: min(rec[:q]) / rec[q])
    lo = min(rec[:k])
    tol = float(np.sqrt(rec[k] * lo))
    print("rec", " ".join(f"{r:.3e}" for r in rec[1:]), f"-> k={k} ({ref.kind[k - 1]}) tol {tol:.3e}")
    assert rec[k] < 0.9 * lo
    x, info = ck.solve(cm, s_["b"], **{**opts(s, 1000, False), "FGMRES tolerance": tol})
    e_x = ck.rel(x, ref.x_steps[k - 1])
    print(f"stop at k={k}: iters {info.iters} x {e_x:.2e} implicit {info.implicit_rel_res:.3e}")
    assert info.iters == k
    assert e_x <= ck.tol_idr(COUPLED, 0, s, k)[0]
    assert info.implicit_rel_res <= tol
