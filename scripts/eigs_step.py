"""The cost of a stability analysis at 2 degrees: shift-invert Arnoldi at the bench state.

    python scripts/eigs_step.py [--k 6] [--m 40] [--sigma 1.0] [--inner 1e-10] [--tol 1e-8]

The state is the bench's near-solution branch state (bench_data/global2_cf05.npz, Mixing 1,
Combined Forcing 0.5).  Drives the C ABI as Ocean.eigs does (iemic/eigs.py) and prints one JSON
line: the total time, the set-up (shifted Jacobian + preconditioner + start vector), the medians
per Arnoldi step of the inner solve, the orthogonalisation and k_eig_scale_bmul, the inner FGMRES
counts, and the Ritz-vector pass: one iemic_eigs_ritz call for all p vectors beside p calls of
one vector each, which read the basis p times as p k_lincomb passes would.  Not a gate.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "i-emic_amd"))

from iemic import _lib, config as cf            # noqa: E402
from iemic.eigs import ritz_groups              # noqa: E402
from iemic.ocean import DeviceVec, Ocean        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--m", type=int, default=40)
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--inner", type=float, default=1e-10)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    c = cf.preset("global2", mixing=1)
    with np.load(os.path.join(ROOT, "bench_data", "global2_cf05.npz"), allow_pickle=False) as d:
        x0 = d["x"].astype(np.float64)
    oc = Ocean(c, solver_params={"FGMRES tolerance": a.inner})
    oc.setState(x0)
    L, h, kr = _lib.lib(), oc._h, oc._krylov()
    T0 = time.perf_counter()
    _lib.check(L.iemic_eigs_begin(h, a.sigma, a.m, 1, C.byref(kr)), "iemic_eigs_begin")
    t_begin = (time.perf_counter() - T0) * 1e3
    H, hcol, infos, groups, unconv = np.zeros((a.m + 1, a.m)), np.zeros(a.m + 2), [], [], 0
    for j in range(a.m):
        info = _lib.EigsInfo()
        rc = L.iemic_eigs_step(h, C.byref(kr), _lib.ptr(hcol), C.byref(info))
        if rc == _lib.IEMIC_ENOCONV:
            unconv += 1
        else:
            _lib.check(rc, "iemic_eigs_step")
        H[:j + 2, j] = hcol[:j + 2]
        infos.append(info)
        if j + 1 >= a.k or info.breakdown:
            groups = ritz_groups(H, j + 1, a.k)
            if info.breakdown or all(g[2] <= a.tol for g in groups):
                break
    steps = len(infos)
    cols = []
    for t, y, est, cnt in groups:
        cols += [y.real, y.imag] if cnt == 2 else [y.real]
    Y = np.ascontiguousarray(np.stack(cols, axis=1))
    p = Y.shape[1]
    xs = [DeviceVec(oc) for _ in range(p)]
    arr = (C.c_void_p * p)(*[x.p for x in xs])

    def timed(fn):
        fn()                                            # warm
        s = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            s.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(s)

    def one_pass():
        _lib.check(L.iemic_eigs_ritz(h, steps, p, _lib.ptr(Y), arr), "iemic_eigs_ritz")

    def p_passes():
        for q in range(p):
            yq = np.ascontiguousarray(Y[:, q:q + 1])
            one = (C.c_void_p * 1)(xs[q].p)
            _lib.check(L.iemic_eigs_ritz(h, steps, 1, _lib.ptr(yq), one), "iemic_eigs_ritz")

    t_ritz, t_sep = timed(one_pass), timed(p_passes)
    res, out2, q = [], np.zeros(2), 0
    for t, y, est, cnt in groups:
        lm = a.sigma + 1.0 / t
        _lib.check(L.iemic_eigs_residual(h, lm.real, lm.imag if cnt == 2 else 0.0, xs[q].p,
                                         xs[q + 1].p if cnt == 2 else None, _lib.ptr(out2)), "iemic_eigs_residual")
        res.append(out2[0] / out2[1])
        q += cnt
    total = (time.perf_counter() - T0) * 1e3
    L.iemic_eigs_end(h)
    lay = oc.layout()
    med = lambda f: statistics.median(getattr(i, f) for i in infos)      # noqa: E731
    out = {"config": "global2", "rows": oc.N, "k": a.k, "m": a.m, "sigma": a.sigma, "inner_tol": a.inner,
           "tol": a.tol, "steps": steps, "total_ms": round(total, 1), "begin_ms": round(t_begin, 1),
           "step_ms": round(med("t_total_ms"), 2), "solve_ms": round(med("t_solve_ms"), 2),
           "orth_ms": round(med("t_orth_ms"), 3), "scale_bmul_ms": round(med("t_scale_ms"), 3),
           "fgmres_iters": [int(i.solve.iters) for i in infos], "inner_unconverged": unconv,
           "ritz_p": p, "ritz_one_pass_ms": round(t_ritz, 3), "ritz_p_passes_ms": round(t_sep, 3),
           "ritz_bytes": (steps + p) * lay["own_rows"] * 8,
           "lambda": [[float(s.real), float(s.imag)] for s in (a.sigma + 1.0 / g[0] for g in groups)],
           "estimate": [float(g[2]) for g in groups], "residual": [float(v) for v in res],
           "basis_bytes": (a.m + 3) * lay["ext_rows"] * 8}
    del xs
    oc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
