"""The cost of one thick restart's pass over the basis at 2 degrees.

    python scripts/eigs_restart_cost.py [--j 64] [--p 16] [--reps 5]

On the 2 degree grid's layout (the bench's branch state, bench_data/global2_cf05.npz) and a basis
of j + 1 vectors, times by events k_eig_compress (in place, one pass) beside what it replaces:
iemic_eigs_ritz's kernel into p scratch vectors, p copies back and the copy of v_{j+1} behind
them.  One untimed repetition of each comes first.  Prints one JSON line: the medians, the
samples and the algorithmic bytes of both.  Not a gate.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "i-emic_amd"))

from iemic import _lib, config as cf            # noqa: E402
from iemic.ocean import Ocean                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--j", type=int, default=64)
    ap.add_argument("--p", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    c = cf.preset("global2", mixing=1)
    with np.load(os.path.join(ROOT, "bench_data", "global2_cf05.npz"), allow_pickle=False) as d:
        x0 = d["x"].astype(np.float64)
    oc = Ocean(c)
    oc.setState(x0)
    L = _lib.lib()
    L.iemic_test_eig_compress_cost.restype = C.c_int
    L.iemic_test_eig_compress_cost.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    n = a.reps + 1
    ms = np.zeros(2 * n)
    _lib.check(L.iemic_test_eig_compress_cost(oc._h, a.j, a.p, n, _lib.ptr(ms)), "iemic_test_eig_compress_cost")
    comp, alt = ms[1:n], ms[n + 1:]
    NL = oc.N
    out = {"grid": "global2", "rows": int(NL), "j": a.j, "p": a.p,
           "compress_ms": statistics.median(comp), "compress_samples_ms": [round(float(v), 4) for v in comp],
           "compress_bytes": (a.j + 1 + a.p + 1) * NL * 8,
           "ritz_and_copies_ms": statistics.median(alt), "ritz_and_copies_samples_ms": [round(float(v), 4) for v in alt],
           "ritz_and_copies_bytes": (a.j + a.p + 2 * a.p + 2) * NL * 8}
    out["compress_GBps"] = out["compress_bytes"] / out["compress_ms"] / 1e6
    out["ritz_and_copies_GBps"] = out["ritz_and_copies_bytes"] / out["ritz_and_copies_ms"] / 1e6
    print(json.dumps(out))
    oc.close()


if __name__ == "__main__":
    main()
