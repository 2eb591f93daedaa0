"""Golden surface fluxes from the reference's own Fortran (tests/test_fluxes.py).

Loads oracle/_ref/libthcm_ref.so in a fresh process per case (THCM is a singleton), sets the
case up through the thcmref_* entry points as make_golden_coupled.py does, and calls
m_probe's get_salflux / get_temflux (probe.F90:200-355, what THCM::getFluxes calls) at the
case's synthetic state.  Cases:

  flux_coupled_natl8   "Coupled Temperature" = 1, atmosphere fields of coupled_natl8.npz
  flux_coupled_natl8s  "Coupled Salinity" = 1 too, fields of coupled_natl8s.npz
  flux_natl8_emip      ocean-only natl8 (SRES = 0) with a seeded random emip inserted
                       through m_inserts' insert_emip (inserts.F90:164-182)

Each npz holds only arrays: the nine flux fields [9][n*m] in the order of THCM's enum, the
correction get_salflux returns (times COMB*SALT) and, for the last case, the inserted field.

Usage (needs the reference build):  python tests/golden/make_golden_flux.py
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "i-emic_amd"))

from iemic import config as cf  # noqa: E402
from oracle import oracle as orc  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEED_EMIP = 20261019
CASES = {"flux_coupled_natl8": "coupled_natl8", "flux_coupled_natl8s": "coupled_natl8s",
         "flux_natl8_emip": "natl8"}

# the set-up half of oracle.oracle's reference runner, then the probe calls
_SCRIPT = orc._REF_SCRIPT.split("deps = np.zeros(7)")[0] + r'''
nm = cfg.n * cfg.m
vp = C.c_void_p
if "emip" in d.files:
    e = np.ascontiguousarray(d["emip"], dtype=np.float64)
    lib._QMm_insertsPinsert_emip.argtypes = [vp]
    lib._QMm_insertsPinsert_emip(e.ctypes.data)
x = np.ascontiguousarray(d["x0"], dtype=np.float64)
fl = np.zeros((9, nm))
corr = C.c_double(0.0)
lib._QMm_probePget_salflux.argtypes = [vp, vp, vp, vp, vp]
lib._QMm_probePget_salflux(x.ctypes.data, fl[0].ctypes.data, C.addressof(corr), fl[1].ctypes.data,
                           fl[2].ctypes.data)
lib._QMm_probePget_temflux.argtypes = [vp] * 7
lib._QMm_probePget_temflux(x.ctypes.data, *[fl[q].ctypes.data for q in range(3, 9)])
np.savez(sys.argv[3], fluxes=fl, correction=np.array(corr.value))
'''


def random_emip(c, landm_local: np.ndarray) -> np.ndarray:
    """seeded random field times the ocean mask of the top layer"""
    L = landm_local.reshape(c.l + 2, c.m + 2, c.n + 2)
    wet = 1 - L[c.l, 1:c.m + 1, 1:c.n + 1].reshape(-1)
    return np.random.default_rng(SEED_EMIP).standard_normal(c.n * c.m) * wet


def run(case: str) -> dict:
    name = CASES[case]
    c = cf.preset(name, mixing=0)
    with np.load(os.path.join(OUT, f"{name}.npz"), allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    d = c.ref_dict()
    ints = [d[k] for k in ["n", "m", "l", "periodic", "itopo", "flat", "rd_mask", "tres", "sres", "iza",
                           "ite", "its", "rd_spertm", "coupled_T", "coupled_S", "forcing_type", "ih",
                           "vmix", "tap", "rho_mixing", "coriolis_on"]]
    dbls = [d[k] for k in ["xmin_deg", "xmax_deg", "ymin_deg", "ymax_deg", "hdim", "qz", "alphaT", "alphaS"]]
    arrs = dict(cfg_int=np.array(ints, dtype=np.int64), cfg_dbl=np.array(dbls),
                maskfile=np.frombuffer(d["maskfile"].encode().ljust(256, b"\0"), dtype=np.uint8),
                landm=g["landm_local"].astype(np.int32), use_landm=np.array(1),
                pars=np.array(list(c.par_list()), dtype=np.float64).reshape(-1, 2),
                nstates=np.array(1), x0=g["synthetic_x"])
    extra = {}
    if "atm_t" in g:
        for k in ("atm_t", "atm_q", "atm_a", "atm_p", "atm_pars"):
            arrs[k] = g[k]
    else:
        extra["emip"] = arrs["emip"] = random_emip(c, g["landm_local"])
    with tempfile.TemporaryDirectory() as td:
        inp, outp, script = (os.path.join(td, f) for f in ("in.npz", "out.npz", "run.py"))
        np.savez(inp, **arrs)
        with open(script, "w") as f:
            f.write(_SCRIPT)
        subprocess.run([sys.executable, script, orc.LIB_REF, inp, outp], check=True, cwd=td, timeout=600,
                       stdout=subprocess.DEVNULL)
        with np.load(outp, allow_pickle=False) as z:
            out = {k: z[k] for k in z.files}
    out.update(extra)
    return out


if __name__ == "__main__":
    if not orc.reference_available():
        sys.exit("reference library not built (make -C oracle ref)")
    for case in CASES:
        out = run(case)
        np.savez(os.path.join(OUT, f"{case}.npz"), **out)
        print(case, {k: float(np.abs(v).max()) for k, v in out.items()})
