"""The theta stepper surface of the C++ host class (i-emic_amd/csrc/ocean.hpp: thetaInitStep,
thetaNewtonStep, thetaRestore) driven by tests/cpp/theta_driver.cpp: builds on the CPU; on the
GPU two fixed time steps on natl8 give the norms of the same run through the Python stepper."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from iemic import config as cf

DRIVER = os.path.join(ROOT, "tests", "_build", "theta_driver")


@pytest.fixture(scope="module")
def driver():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "i-emic_amd"), "-j8"], check=True,
                   stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "theta.mk"], check=True,
                   stdout=subprocess.DEVNULL)
    return DRIVER


def test_driver_builds(driver):
    assert os.access(driver, os.X_OK)


def write_problem(path, c, L, x):
    """the problem file of tests/cpp/ocean_driver.cpp"""
    pars = c.par_list()
    with open(path, "wb") as f:
        f.write(struct.pack("11i", c.n, c.m, c.l, int(c.periodic), c.tres, c.sres,
                            c.forcing_type, c.inhomogeneous_mixing, c.coriolis, c.int_sign,
                            len(pars)))
        f.write(struct.pack("8d", c.xmin, c.xmax, c.ymin, c.ymax, c.hdim, c.qz, c.alpha_t,
                            c.alpha_s))
        for idx, v in pars:
            f.write(struct.pack("=id", idx, v))
        f.write(np.ascontiguousarray(L, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(x, dtype=np.float64).tobytes())


@pytest.mark.gpu
def test_cpp_theta_two_steps(driver, tmp_path):
    from iemic.ocean import Ocean
    from iemic.transient import ThetaStepper
    dt, theta, tol, maxit = 1e-3, 0.75, 1e-4, 10
    c = cf.preset("natl8", mixing=0)          # the drivers create their context with Mixing 0
    c.start_params["Combined Forcing"] = 1.0
    c.start_params["Salinity Forcing"] = 0.1
    L0 = cf.landmask(c)
    x = np.zeros(c.nrows)
    inp = str(tmp_path / "in.bin")
    write_problem(inp, c, L0, x)
    p = subprocess.run([driver, inp, repr(dt), repr(theta), "2", repr(tol), str(maxit)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    got = [(int(a), int(b), float(n)) for a, b, n in
           re.findall(r"step (\d+) newton (\d+) normx (\S+)", p.stdout)]
    assert len(got) == 2, p.stdout
    oc = Ocean(c, landm=L0, solver_params={"FGMRES tolerance": 1e-6})
    oc.setState(x)
    st = ThetaStepper(oc, {"time step": dt, "theta": theta, "Newton tolerance": tol,
                           "maximum Newton iterations": maxit, "number of time steps": 2,
                           "adaptive time steps": False, "HDF5 output frequency": 0})
    assert st.run() == 0
    print(p.stdout)
    for (step, k, norm), r in zip(got, st.history):
        print(f"python step {r.step} newton {r.newton_steps} normx {r.norm_x:.17g}")
        assert (step, k) == (r.step, r.newton_steps)
        assert abs(norm - r.norm_x) <= 1e-12 * r.norm_x
    assert st.history[0].norm_x > 0.1
    oc.close()
