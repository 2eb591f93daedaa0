"""What one evaluation of the rare-event score function costs at 2 degrees, beside the same quantity
composed from the device vector algebra (two lincomb and two norm, as the reference composes it).

    python scripts/score_cost.py [--reps 5] [--inner 20]

Both ways end with their results on the host (the score is compared with a level after every time
step), so host wall time around `inner` evaluations is what is reported, min - max over `reps`, in
microseconds per evaluation.  Prints one JSON line.  Reporting only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "i-emic_amd"))

from iemic import config as cf          # noqa: E402
from iemic.ocean import Ocean           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    c = cf.preset("global2", mixing=1)
    oc = Ocean(c)
    L = oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    s1 = cf.synthetic_state(c, L, seed=1)
    s2 = cf.synthetic_state(c, L, seed=2)
    x = cf.synthetic_state(c, L, seed=3)
    ops = oc.vec_ops()
    out = {"config": "global2", "rows": int(c.nrows), "reps": a.reps, "inner": a.inner}
    for var, name in ((-1, "default"), (1, "ocean")):
        oc.scoreSet(s1, s2, None, var)
        nrm, _ = oc.scoreGet()
        xv, v1, v2 = ops.from_host(x), ops.from_host(s1), ops.from_host(s2)

        def fused():
            return oc.score(xv)

        def composed():
            d1 = ops.norm(ops.lincomb(1.0, xv, -1.0, v1)) / nrm
            d2 = ops.norm(ops.lincomb(1.0, xv, -1.0, v2)) / nrm
            return d1, d2

        if var < 0:                      # the composed form has no per-variable norm
            f, g = fused(), composed()
            out["d1_fused_composed"] = [f[1], g[0]]
        for label, fn in (("fused", fused), ("composed", composed)) if var < 0 else (("fused", fused),):
            fn()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    fn()
                ts.append((time.perf_counter() - t0) / a.inner * 1e6)
            out[f"{name}_{label}_us"] = [round(min(ts), 1), round(max(ts), 1)]
    oc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
