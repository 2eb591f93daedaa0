"""One fused theta Newton iteration at 2 degrees beside one plain Newton step at the same state.

    python scripts/theta_step.py [--dt 1e-3] [--theta 0.75] [--reps 3] [--noise SIGMA]

The state is the bench's near-solution branch state (bench_data/global2_cf05.npz, Mixing 1,
Combined Forcing 0.5), reset from the host before every step; both steps refactor the
preconditioner (iemic_newton_step always does).  Prints one JSON line: the medians of the total
and per-phase wall times of Ocean.newtonStep and Ocean.thetaNewtonStep and their FGMRES counts.
Not a gate: the theta step solves another operator (J - B / dt / theta is more diagonally
dominant the smaller dt is), so its Krylov count differs from the steady Newton step's.
--noise SIGMA adds a third step to the alternation: the theta iteration with the stochastic
model's noise armed (Ocean.stochasticInitStep with one fixed block of normals), whose residual
kernel reads the noise field; its right-hand side differs, so its Krylov count may too.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "i-emic_amd"))

from iemic import config as cf          # noqa: E402
from iemic.ocean import Ocean           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--theta", type=float, default=0.75)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.0)
    a = ap.parse_args()
    c = cf.preset("global2", mixing=1)
    with np.load(os.path.join(ROOT, "bench_data", "global2_cf05.npz"), allow_pickle=False) as d:
        x0 = d["x"].astype(np.float64)
    oc = Ocean(c)
    fields = ("t_total_ms", "t_jac_ms", "t_rhs_ms", "t_prec_ms", "t_solve_ms")
    out = {"config": "global2", "dt": a.dt, "theta": a.theta, "reps": a.reps}
    runs = {"newton": [], "theta": []}
    if a.noise > 0.0:
        from iemic.transient import StochasticThetaStepper
        runs["theta_noise"] = []
        out["sigma"] = a.noise
        pert = StochasticThetaStepper.noise_block(1, 0, c.m)
    for rep in range(a.reps + 1):                         # the two alternate; the first pair warms up
        for name in runs:
            oc.setState(x0)
            if name == "newton":
                info = oc.newtonStep(allow_unconverged=True)
            else:
                oc.preProcess()
                if name == "theta":
                    oc.thetaInitStep(a.dt, a.theta)
                else:
                    oc.stochasticInitStep(a.dt, a.theta, a.noise, pert)
                info = oc.thetaNewtonStep()
            if rep:
                runs[name].append(info)
    for name, r in runs.items():
        out[name] = {f: statistics.median(getattr(i, f) for i in r) for f in fields}
        out[name]["total_ms_samples"] = [round(i.t_total_ms, 2) for i in r]
        out[name]["fgmres_iters"] = r[-1].solve.iters
        out[name]["converged"] = r[-1].solve.converged
    oc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
