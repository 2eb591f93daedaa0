"""The fused Newton iterations of the steady and the theta model, bitwise against a recording.

csrc/newton.hip holds the one Newton iteration (newton_iterate) that iemic_newton_step and
iemic_theta_newton_step run over their two models.  The launches, their order and the points at
which the host waits are those of the two separate functions it replaced, so no bit may move:
tests/golden/newton_parent_steps.npz holds what those two functions returned, recorded by
record() twice in separate processes on an MI355X.  The two recordings agreed bitwise in every
field, so every field is pinned bitwise: per step the state, norm_f0, norm_f1, norm_dx (theta
only), solve.iters, solve.converged and the return status.  The file holds this project's own
output only; the inputs are the synthetic state of test_gpu_transient.py on natl8.

Cases (natl8, test_transient.transient_config):
* steady, one rank: two consecutive Newton steps, with the benchmark's solver configuration
  (FGMRES, block GS) and with Solver = IDR;
* theta, one rank: thetaInitStep at (dt, theta) = (1e-3, 0.75) and (0.128, 1.0), then two
  Newton iterations, the preconditioner-recompute flag on for the first and off for the second
  (both arms of refactor || !gs.ready);
* theta, two in-process latitude bands: one iteration (norm_dx passes through the max over the
  ranks).

Beside the pin: the steady twin of test_gpu_transient.py's test_fused_step_equals_composed, and
the device vectors' normInf on natl8 (one rank and two bands) against numpy, NaN included.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from iemic import _lib
from iemic import config as cf
from test_gpu_transient import SOLVER, run_bands
from test_transient import transient_config

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newton_parent_steps.npz")

# bench.py's defaults for the flagship Newton step (its --tol, --krylov, --restarts; the block GS
# settings it passes are the model's defaults)
BENCH = {"Preconditioner": 2, "FGMRES tolerance": 1e-8, "FGMRES iterations": 90, "FGMRES restarts": 20,
         "Orthogonalization": "DCGS2", "Solver": "FGMRES"}
IDR = {**BENCH, "Solver": "IDR", "IDR s": 4}
THETA = ((1e-3, 0.75), (0.128, 1.0))
FIELDS = ("norm_f0", "norm_f1", "norm_dx", "iters", "converged", "status")


@pytest.fixture(scope="module")
def Ocean():
    from iemic.ocean import Ocean
    return Ocean


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def start(Ocean, sp, **kw):
    """(config, model at the synthetic state of test_gpu_transient.py, that state)"""
    c = transient_config()
    oc = Ocean(c, landm=cf.landmask(c), solver_params=sp, **kw)
    x = cf.synthetic_state(c, oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2), amp_ts=1e-3)
    oc.setState(x)
    return c, oc, x


def steady_step(oc):
    """newtonStep(allow_unconverged=True), keeping the status it hides"""
    k, info = oc._krylov(), _lib.NewtonInfo()
    rc = _lib.lib().iemic_newton_step(oc._h, C.byref(k), C.byref(info))
    return rc, info


def theta_step(oc, refactor):
    """thetaNewtonStep with the recompute flag spelled out, keeping the status it hides"""
    k, info = oc._krylov(), _lib.ThetaInfo()
    rc = _lib.lib().iemic_theta_newton_step(oc._h, C.byref(k), int(refactor), C.byref(info))
    return rc, info


def entry(out, key, rc, info, x):
    assert rc in (0, _lib.IEMIC_ENOCONV), (key, rc)
    out[f"{key}_x"] = np.array(x)
    out[f"{key}_info"] = np.array([info.norm_f0, info.norm_f1, getattr(info, "norm_dx", 0.0), info.solve.iters,
                                   info.solve.converged, rc], dtype=np.float64)


def run_steady(Ocean, tag, sp):
    out = {}
    _, oc, _ = start(Ocean, sp)
    for step in (1, 2):
        rc, info = steady_step(oc)
        entry(out, f"steady_{tag}_step{step}", rc, info, oc.getState())
    oc.close()
    return out


def run_theta(Ocean, q):
    out = {}
    _, oc, _ = start(Ocean, SOLVER)
    oc.thetaInitStep(*THETA[q])
    for step, refactor in ((1, 1), (2, 0)):
        rc, info = theta_step(oc, refactor)
        entry(out, f"theta{q}_step{step}", rc, info, oc.getState())
    oc.close()
    return out


def run_theta_bands(Ocean):
    def fn(r, group):
        _, oc, _ = start(Ocean, SOLVER, local_group=group, rank=r, nranks=2, npx=1)
        oc.thetaInitStep(*THETA[0])
        rc, info = theta_step(oc, 1)
        x = oc.getState().copy()             # the rows this band owns, zero elsewhere
        oc.close()
        return rc, info, x

    out = {}
    for r, (rc, info, x) in enumerate(run_bands(2, fn)):
        entry(out, f"theta_bands_rank{r}", rc, info, x)
    return out


RUNS = {"steady_fgmres": lambda Oc: run_steady(Oc, "fgmres", BENCH),
        "steady_idr": lambda Oc: run_steady(Oc, "idr", IDR),
        "theta0": lambda Oc: run_theta(Oc, 0),
        "theta1": lambda Oc: run_theta(Oc, 1),
        "theta_bands": run_theta_bands}


def record(Ocean):
    """every case's steps: <key>_x (state) and <key>_info (FIELDS)"""
    out = {}
    for run in RUNS.values():
        out.update(run(Ocean))
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("case", list(RUNS))
def test_newton_steps_are_the_recorded_ones(Ocean, golden, case):
    """State bitwise; norm_f0, norm_f1, norm_dx, solve.iters, solve.converged and the status
    equal to the recording, in every step of the case."""
    got = RUNS[case](Ocean)
    assert got and set(got) <= set(golden)
    for key in sorted(k[:-2] for k in got if k.endswith("_x")):
        x, info, gx, gi = got[f"{key}_x"], got[f"{key}_info"], golden[f"{key}_x"], golden[f"{key}_info"]
        print(f"{key}: " + " ".join(f"{f} {float(a)!r} ({float(b)!r})" for f, a, b in zip(FIELDS, info, gi))
              + f" differing entries of x {int(np.count_nonzero(bits(x) != bits(gx)))}")
        assert np.all(np.isfinite(gx)) and np.any(gx != 0) and gi[0] > 0
        assert np.array_equal(bits(x), bits(gx))
        assert np.array_equal(bits(info), bits(gi))


def test_recording_covers_the_cases(golden):
    """Nothing recorded is left unchecked, the solves of the recording did work, and the theta
    cases saw both arms of the preconditioner rule (a set-up takes the first step only)."""
    keys = {k[:-2] for k in golden if k.endswith("_x")}
    assert keys == ({f"steady_{t}_step{s}" for t in ("fgmres", "idr") for s in (1, 2)}
                    | {f"theta{q}_step{s}" for q in (0, 1) for s in (1, 2)}
                    | {f"theta_bands_rank{r}" for r in (0, 1)})
    for k in keys:
        assert golden[f"{k}_info"][3] > 0, k
    # the two bands report the same norms: sums and the max over the ranks
    assert np.array_equal(bits(golden["theta_bands_rank0_info"]), bits(golden["theta_bands_rank1_info"]))


def test_fused_steady_step_equals_composed(Ocean):
    """newtonStep on one context; on a second rhs, jacobian, prec_compute, solve(-F),
    setState(x + dx), rhs: state and both norms to the 1e-10 relative of the theta twin."""
    _, a, x = start(Ocean, SOLVER)
    _, b, _ = start(Ocean, SOLVER)
    info = a.newtonStep()
    f0 = b.computeRHS().copy()
    b.computeJacobian()
    b.buildPreconditioner(force=True)
    dx = b.solve(-f0).copy()
    b.setState(x + dx)
    f1 = b.computeRHS().copy()
    xa, xb = a.getState(), b.getState()
    print(f"|F0| {info.norm_f0:.6e} |F1| {info.norm_f1:.6e} iters {info.solve.iters} / {b.last_solve.iters} "
          f"state diff {np.linalg.norm(xa - xb) / np.linalg.norm(xb):.2e}")
    assert info.solve.converged == 1 and b.last_solve.converged == 1
    assert np.linalg.norm(dx) > 0
    assert np.linalg.norm(xa - xb) <= 1e-10 * np.linalg.norm(xb)
    assert abs(info.norm_f0 - np.linalg.norm(f0)) <= 1e-10 * np.linalg.norm(f0)
    assert abs(info.norm_f1 - np.linalg.norm(f1)) <= 1e-10 * np.linalg.norm(f1)
    a.close()
    b.close()


def norm_inf_vectors(n):
    """mixed signs and magnitudes; the largest entry negative; then the same with one NaN"""
    v = np.random.default_rng(7).standard_normal(n) * 10.0 ** np.random.default_rng(8).uniform(-30, 30, n)
    v[n // 3] = -2.0 * np.max(np.abs(v))
    w = v.copy()
    w[(2 * n) // 3] = np.nan
    return v, w


def test_norm_inf_one_rank(Ocean):
    """normInf of a device vector is np.max(np.abs(v)) exactly (a max rounds nothing), and NaN
    when one entry is NaN."""
    c, oc, _ = start(Ocean, SOLVER)
    ops = oc.vec_ops()
    v, w = norm_inf_vectors(c.nrows)
    assert ops.norm_inf(ops.from_host(v)) == np.max(np.abs(v))
    assert math.isnan(ops.norm_inf(ops.from_host(w)))
    oc.close()


def test_norm_inf_two_bands(Ocean):
    """The same on two latitude bands: the maximum sits in one band, the NaN in one band (each
    band in turn), and every rank reports the global value."""
    c = transient_config()
    v, _ = norm_inf_vectors(c.nrows)
    # a row of the southernmost and one of the northernmost latitude: one in each band
    nan_rows = [6 * ((1 * c.m + j) * c.n + c.n // 2) + 4 for j in (0, c.m - 1)]

    def fn(r, group):
        _, oc, _ = start(Ocean, SOLVER, local_group=group, rank=r, nranks=2, npx=1)
        ops = oc.vec_ops()
        res = [ops.norm_inf(ops.from_host(v))]
        for q in nan_rows:
            w = v.copy()
            w[q] = np.nan
            res.append(ops.norm_inf(ops.from_host(w)))
        rows = set(oc.owned_rows().tolist())
        oc.close()
        return res, int(np.argmax(np.abs(v))) in rows, [q in rows for q in nan_rows]

    out = run_bands(2, fn)
    assert sorted(o[1] for o in out) == [False, True]
    assert sorted(o[2] for o in out) == [[False, True], [True, False]]
    for res, _, _ in out:
        assert res[0] == np.max(np.abs(v))
        assert math.isnan(res[1]) and math.isnan(res[2])
