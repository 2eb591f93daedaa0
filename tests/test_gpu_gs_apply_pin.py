"""The block Gauss-Seidel apply, bitwise against a recording of the unit it was split from.

csrc/prec_gs.hip was one unit; it is now four: gs_setup.hip (set-up), gs_dyn.hip (the dynamics
pass), ts_sweeps.hip (the plain T/S sweeps) and prec_gs.hip (the apply, as named steps).  Every
kernel kept its body and its launch, and the apply kept the order, the arguments and the condition
of every launch, exchange, all-reduce and stream join, so no bit may move:
tests/golden/gs_apply_parent.npz holds applyPrecon's output for a seeded dense right-hand side
(config.synthetic_vector, seed 3) as the one-unit library computed it, recorded by record() twice
in separate processes on an MI355X.  The two recordings agreed bitwise in every case, the band
cases included (the reductions on these paths run in a fixed order), so every case is pinned by
int64-view equality.  The file holds this project's own output only.

Cases (the masks of test_gpu_parity.py and test_gpu_dist.py), by the branch they reach:
* compact / generic / four: ts_mg = 0 on natl8 (even n: colour-compacted sweeps), on natl8 without
  its last longitude (7 x 8 x 4: the generic two-colour sweeps) and on 2dmoc (periodic, n = 3: four
  colours); compact_dyn4: the sweeps after four dynamics passes (every pass writes the AoS output);
* default: multigrid, dyn_iters 4, dyn_omega 0.95, default Schur passes, on natl8 (Mixing = 1),
  natl8_l8 and gateway16;
* schur0, schur1: every pass / the first only with the Schur solve;
* dyn1: one pass;  mr: the minimal-residual correction;  ts_at1: the T/S multigrid on the side
  stream after the first pass, joined at the end;
* fgmres, fgmres_sweeps: one FGMRES solve with DCGS2 on natl8 -- x, iters and both residuals --
  which applies the preconditioner to compressed input, unstaged (the first vector) and staged;
* bands_default, bands_mr, bands_sweeps: natl8 as two in-process latitude bands (the halo-row path
  of the fixed-step passes, and the two exchange fallbacks);
* split2x2: gateway16 on 2 x 2 ranks (npx > 1 turns the halo-row path off).
"""
import dataclasses
import os

import numpy as np
import pytest

from helpers import golden_landm
from iemic import config as cf
from test_gpu_transient import run_bands

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gs_apply_parent.npz")

SWEEPS = {"Preconditioner": 2, "TS sweeps": 3, "Dyn iterations": 1, "TS multigrid cycles": 0}
FGMRES = {"Preconditioner": 2, "FGMRES tolerance": 1e-8, "FGMRES iterations": 90, "FGMRES restarts": 20,
          "Orthogonalization": "DCGS2", "Solver": "FGMRES"}
# case -> (grid, Mixing, solver parameters, (nranks, npx))
APPLY = {
    "compact": ("natl8", 0, SWEEPS, None),
    "generic": ("natl8_odd", 0, SWEEPS, None),
    "four": ("2dmoc", 0, SWEEPS, None),
    "compact_dyn4": ("natl8", 0, {"Preconditioner": 2, "TS sweeps": 3, "TS multigrid cycles": 0}, None),
    "default_natl8": ("natl8", 1, {"Preconditioner": 2}, None),
    "default_natl8_l8": ("natl8_l8", 1, {"Preconditioner": 2}, None),
    "default_gateway16": ("gateway16", 1, {"Preconditioner": 2}, None),
    "schur0": ("natl8", 1, {"Preconditioner": 2, "Schur passes": 0}, None),
    "schur1": ("natl8", 1, {"Preconditioner": 2, "Schur passes": 1}, None),
    "dyn1": ("natl8", 1, {"Preconditioner": 2, "Dyn iterations": 1}, None),
    "mr": ("natl8", 1, {"Preconditioner": 2, "Dyn minimal residual": True}, None),
    "ts_at1": ("natl8", 1, {"Preconditioner": 2, "TS after dyn pass": 1}, None),
    "bands_default": ("natl8", 0, {"Preconditioner": 2}, (2, 1)),
    "bands_mr": ("natl8", 0, {"Preconditioner": 2, "Dyn minimal residual": True}, (2, 1)),
    "bands_sweeps": ("natl8", 0, {"Preconditioner": 2, "TS sweeps": 3, "TS multigrid cycles": 0}, (2, 1)),
    "split2x2": ("gateway16", 0, {"Preconditioner": 2}, (4, 2)),
}
SOLVES = {"fgmres": FGMRES, "fgmres_sweeps": {**FGMRES, "TS sweeps": 3, "TS multigrid cycles": 0}}
CASES = list(APPLY) + list(SOLVES)


@pytest.fixture(scope="module")
def Ocean():
    from iemic.ocean import Ocean
    return Ocean


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def grid(name, mixing):
    """(config, land mask) of the parity tests' grids"""
    if name == "natl8_l8":
        c = cf.preset("natl8", mixing=mixing).with_(name=name, l=8, refine_l=8)
        return c, cf.init_landmask(c, cf.landmask(c))
    if name == "natl8_odd":
        return dataclasses.replace(cf.preset("natl8", mixing=mixing), n=7), np.delete(golden_landm("natl8"), 8, axis=2)
    return cf.preset(name, mixing=mixing), golden_landm(name)


def ready(Ocean, name, mixing, sp, **kw):
    """(config, model with the Jacobian of the synthetic state and its preconditioner)"""
    c, L0 = grid(name, mixing)
    oc = Ocean(c, landm=L0, solver_params=sp, **kw)
    x = cf.synthetic_state(c, oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2), amp_ts=1e-3)
    oc.setState(x)
    oc.computeJacobian()
    oc.buildPreconditioner(force=True)
    return c, oc


def owned_rows(c, lay):
    k, j, i, v = np.meshgrid(np.arange(c.l), np.arange(lay["jb0"], lay["jb1"]), np.arange(lay["ib0"], lay["ib1"]),
                             np.arange(6), indexing="ij")
    return (6 * ((k * c.m + j) * c.n + i) + v).reshape(-1)


def run_apply(Ocean, case):
    """applyPrecon of the seeded right-hand side; subdomains: the owned rows gathered"""
    name, mixing, sp, split = APPLY[case]
    if split is None:
        c, oc = ready(Ocean, name, mixing, sp)
        z = oc.applyPrecon(cf.synthetic_vector(c, seed=3)).copy()
        oc.close()
        return {f"{case}_z": z}
    nranks, npx = split

    def fn(r, group):
        c, oc = ready(Ocean, name, mixing, sp, local_group=group, rank=r, nranks=nranks, npx=npx)
        z = oc.applyPrecon(cf.synthetic_vector(c, seed=3)).copy()
        rows = owned_rows(c, oc.layout())
        oc.close()
        return rows, z

    c, _ = grid(name, mixing)
    z, seen = np.zeros(c.nrows), np.zeros(c.nrows, dtype=np.int64)
    for rows, zr in run_bands(nranks, fn):
        z[rows] = zr[rows]
        seen[rows] += 1
    assert np.all(seen == 1)
    return {f"{case}_z": z}


def run_solve(Ocean, case):
    """one FGMRES solve of J dx = -F: the solution, iters, the implicit and the explicit residual"""
    c, oc = ready(Ocean, "natl8", 0, SOLVES[case])
    b = -oc.computeRHS().copy()
    x = np.array(oc.solve(b))
    s = oc.last_solve
    oc.close()
    return {f"{case}_z": x, f"{case}_info": np.array([s.iters, s.converged, s.implicit_rel_res, s.explicit_rel_res],
                                                     dtype=np.float64)}


def run(Ocean, case):
    return run_apply(Ocean, case) if case in APPLY else run_solve(Ocean, case)


def record(Ocean):
    """every case's output: <case>_z, and <case>_info for the solves"""
    out = {}
    for case in CASES:
        out.update(run(Ocean, case))
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("case", CASES)
def test_apply_is_the_recorded_one(Ocean, golden, case):
    """Every entry of the output (and of the solve's iters and residuals) bitwise equal to the
    recording."""
    got = run(Ocean, case)
    assert got and set(got) <= set(golden)
    for key in sorted(got):
        a, g = got[key], golden[key]
        print(f"{key}: differing entries {int(np.count_nonzero(bits(a) != bits(g)))} of {g.size}, "
              f"max |a - g| {float(np.max(np.abs(a - g))):.3e}, max |g| {float(np.max(np.abs(g))):.3e}")
        assert np.all(np.isfinite(g)) and np.any(g != 0)
        assert np.array_equal(bits(a), bits(g))


def test_recording_covers_the_cases(golden):
    """Nothing recorded is left unchecked; the solves converged after more than one step (so they
    applied the preconditioner unstaged and staged); and the options the cases vary changed the
    output, so each reached its branch."""
    assert set(golden) == {f"{k}_z" for k in CASES} | {f"{k}_info" for k in SOLVES}
    for k in SOLVES:
        assert golden[f"{k}_info"][0] > 1 and golden[f"{k}_info"][1] == 1, k
    for k in ("schur0", "schur1", "dyn1", "mr", "ts_at1"):
        assert not np.array_equal(bits(golden[f"{k}_z"]), bits(golden["default_natl8_z"])), k
    assert not np.array_equal(bits(golden["compact_dyn4_z"]), bits(golden["compact_z"]))
    assert not np.array_equal(bits(golden["bands_mr_z"]), bits(golden["bands_default_z"]))
    assert not np.array_equal(bits(golden["bands_sweeps_z"]), bits(golden["bands_default_z"]))
