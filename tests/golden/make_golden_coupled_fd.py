"""Recorded reference runs of tests/test_coupled.py::test_ocean_block_matches_fortran_fd.

Runs the reference's own THCM Fortran (oracle/_ref/libthcm_ref.so, built by oracle/ref/Makefile
where the reference tree is present) at the synthetic state of coupled_natl8 / coupled_natl8s
with the atmosphere fields of test_coupled.fd_runs inserted (the fixture's fields and unit
perturbations of them) and stores each run's right-hand side B as "<fixture>__<run>" in
tests/golden/coupled_fd.npz.

Usage:  python tests/golden/make_golden_coupled_fd.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "i-emic_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from iemic import config as cf  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from test_coupled import fd_runs  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main() -> None:
    orc.build(ref=True)
    out = {}
    for name in ("coupled_natl8", "coupled_natl8s"):
        c, g, _, runs = fd_runs(name)
        L = cf.landmask(c)
        for k, atmos in runs.items():
            r = orc.run_reference(c.ref_dict(), L, c.par_list(), [g["synthetic_x"]], use_landm=False,
                                  atmos=atmos)
            out[f"{name}__{k}"] = r["B0"]
        print(name, "done", len(runs), "runs", flush=True)
    np.savez_compressed(os.path.join(OUT, "coupled_fd.npz"), **out)


if __name__ == "__main__":
    main()
