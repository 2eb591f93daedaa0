"""The theta time stepper's logic (iemic.transient.ThetaStepper) on a CPU twin of the GPU model.

The twin offers the stepper's model surface over the oracle: F and J from
oracle.Oracle, the shifted Jacobian J - B / dt / theta on the CSR diagonal, and the solve by
the oracle's block Gauss-Seidel FGMRES with the GPU's default preconditioner settings.  Like
the GPU model it sets the preconditioner up once per time step (at the first solve after
preProcess) and reuses it, as the operator of that first shifted Jacobian, in the step's later
Newton iterations.

The run is the reference's regression src/tests/trns_ocean.C:41-62: test_oceantransient.xml
(natl8 with Combined Forcing 1.0 and Salinity Forcing 0.1) from the zero state with
timestepper_params.xml.  TABLE holds, per accepted time step, dt, Newton::steps() and ||x||
of a twin run that refactored in every Newton iteration (its total of 30 Newton steps is the
number the reference's test asserts); between linear tolerances 1e-6 and 1e-10 its norms move
by at most 6.6e-10, and 1e-7 is the bound here.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from iemic import config as cf
from iemic.transient import ThetaStepper
from helpers import mask_fix

# test/ocean/timestepper_params.xml
PARAMS = {"adaptive time steps": True, "minimum time step": 1.0e-6, "maximum time step": 1.0,
          "time step increase": 2.0, "time step decrease": 2.0, "time step": 1.0e-3,
          "maximum time (in y)": 10.0, "theta": 0.75, "number of time steps": 10,
          "HDF5 output frequency": 0, "Newton tolerance": 1e-4,
          "minimum desired Newton iterations": 4, "maximum desired Newton iterations": 4,
          "maximum Newton iterations": 10}

# step: (dt, Newton::steps(), ||x|| after the step)
TABLE = [(1e-3, 1, 0.410442364), (2e-3, 2, 1.184471829), (4e-3, 3, 2.644188770),
         (8e-3, 3, 5.054150394), (1.6e-2, 4, 8.938396139), (1.6e-2, 3, 12.221394604),
         (3.2e-2, 4, 17.434781029), (3.2e-2, 3, 21.632458843), (6.4e-2, 3, 28.079651045),
         (0.128, 4, 37.038309608)]


def transient_config():
    """test/ocean/test_oceantransient.xml"""
    c = cf.preset("natl8")
    c.start_params["Combined Forcing"] = 1.0
    c.start_params["Salinity Forcing"] = 0.1
    return c


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class TwinModel:
    """The stepper's model surface on the CPU oracle."""

    def __init__(self, orc, cfg, lin_tol=1e-6):
        L = cf.landmask(cfg).reshape(cfg.l + 2, cfg.m + 2, cfg.n + 2)
        self.orc = orc
        self.L = mask_fix(orc, cfg, L)
        self.o = orc.Oracle(cfg.ref_dict(), self.L, cfg.par_list())
        o = self.o
        self.x = np.zeros(o.N)
        rows = np.repeat(np.arange(o.N), np.diff(o.rowptr))
        self.diag = np.flatnonzero(o.col == rows)
        assert self.diag.size == o.N
        self.lin_tol = lin_tol
        self.refactor = True
        self.gs = None
        self.setups = 0
        self.solves = 0

    def getState(self):
        return self.x.copy()

    def preProcess(self):
        self.refactor = True

    def thetaInitStep(self, dt, theta):
        self.dt, self.theta = dt, theta
        self.xn = self.x.copy()
        self.Fn = self.o.rhs(self.x)

    def thetaRestore(self):
        self.x = self.xn.copy()

    def _ftheta(self, B):
        dt, th = self.dt, self.theta
        return (dt * th) * self.o.rhs(self.x) + (dt * (1 - th)) * self.Fn + B * (self.xn - self.x)

    def thetaNewtonStep(self):
        o, dt, th = self.o, self.dt, self.theta
        val, B = o.jacobian(self.x)
        val = val.copy()
        val[self.diag] += np.where(B != 0, -(B / dt) / th, 0.0)
        if self.refactor:
            self.gs = self.orc.BlockGS(o, val, 3, dyn_iters=4, dyn_omega=0.95, ts_mg=1)
            self.refactor = False
            self.setups += 1
        b = np.ascontiguousarray(self._ftheta(B) / dt / th)
        # BlockGS.fgmres with the current matrix in place of the set-up one
        dx = np.zeros(o.N)
        rel = C.c_double()
        hist = np.zeros(601)
        self.gs.lib.orc_fgmres_gs(o.N // 6, o.rowptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                  o.col.ctypes.data_as(C.POINTER(C.c_int)), _pd(val), self.gs.h, _pd(b),
                                  _pd(dx), self.lin_tol, 300, 600, C.byref(rel), _pd(hist))
        self.solves += 1
        self.x = self.x - dx
        return SimpleNamespace(norm_dx=float(np.max(np.abs(dx))),
                               norm_f1=float(np.linalg.norm(self._ftheta(B))))


@pytest.fixture(scope="module")
def twin_run(oracle_lib):
    m = TwinModel(oracle_lib, transient_config())
    st = ThetaStepper(m, PARAMS)
    status = st.run()
    return m, st, status


def test_trns_ocean_on_the_twin(twin_run):
    m, st, status = twin_run
    for r in st.history:
        print(f"step {r.step} dt {r.dt:g} steps() {r.newton_steps} |x| {r.norm_x:.9f}")
    assert status == 0
    assert [r.dt for r in st.history] == [t[0] for t in TABLE]
    assert [r.newton_steps for r in st.history] == [t[1] for t in TABLE]
    assert st.total_newton_steps() == 30
    for r, t in zip(st.history, TABLE):
        assert abs(r.norm_x - t[2]) <= 1e-7, (r.step, r.norm_x, t[2])
    assert [r.step for r in st.history] == list(range(1, 11))
    assert st.rejected == []


def test_preconditioner_once_per_time_step(twin_run):
    m, st, _ = twin_run
    assert m.setups == 10
    assert m.solves == sum(t[1] + 1 for t in TABLE)


def test_history_in_years(twin_run):
    _, st, _ = twin_run
    y = 737.2685 / 365.0
    t = 0.0
    for r in st.history:
        t += r.dt
        assert r.dt_y == r.dt * y and r.time_y == t * y


def test_failed_newton_halves_dt_and_restores(oracle_lib):
    c = transient_config()
    m = TwinModel(oracle_lib, c)
    m.x = cf.synthetic_state(c, m.L, amp_ts=1e-3)
    xn = m.x.copy()
    p = dict(PARAMS, **{"maximum Newton iterations": 1, "number of time steps": 1,
                        "minimum time step": 2.5e-4})
    st = ThetaStepper(m, p)
    assert st.run() == 1                     # 1e-3, 5e-4, 2.5e-4: then the minimum is reached
    assert st.rejected == [1e-3, 5e-4, 2.5e-4]
    assert st.history == [] and st.total_newton_steps() == 0
    assert np.array_equal(m.getState(), xn)


def test_failed_newton_without_adaptivity(oracle_lib):
    m = TwinModel(oracle_lib, transient_config())
    p = dict(PARAMS, **{"maximum Newton iterations": 1, "adaptive time steps": False})
    st = ThetaStepper(m, p)
    assert st.run() == 1
    assert st.rejected == [1e-3] and st.dt == 1e-3
    assert np.array_equal(m.getState(), np.zeros(m.o.N))


@pytest.mark.parametrize("theta", [0.0, 1.5])
def test_theta_refused_by_name(theta):
    with pytest.raises(ValueError, match='"theta"'):
        ThetaStepper(object(), dict(PARAMS, theta=theta))


def test_zero_time_step_refused_by_name():
    with pytest.raises(ValueError, match='"time step"'):
        ThetaStepper(object(), dict(PARAMS, **{"time step": 0.0}))


class ScriptedModel:
    """Converges in the first Newton iteration of every time step."""

    def __init__(self):
        self.calls = []

    def preProcess(self):
        self.calls.append("pre")

    def thetaInitStep(self, dt, theta):
        self.calls.append(("init", dt, theta))

    def thetaNewtonStep(self):
        self.calls.append("newton")
        return SimpleNamespace(norm_dx=1e-9, norm_f1=1e-9)

    def thetaRestore(self):
        self.calls.append("restore")

    def getState(self):
        return np.ones(4)


def test_steps_counts_the_loop_index():
    m = ScriptedModel()
    st = ThetaStepper(m, dict(PARAMS, **{"number of time steps": 3}))
    assert st.run() == 0
    assert st.total_newton_steps() == 0
    assert [r.newton_steps for r in st.history] == [0, 0, 0]
    assert [r.dt for r in st.history] == [1e-3, 2e-3, 4e-3]      # 0 < 4 desired: dt doubles
    assert m.calls == ["pre", ("init", 1e-3, 0.75), "newton", "pre", ("init", 2e-3, 0.75), "newton",
                       "pre", ("init", 4e-3, 0.75), "newton"]


def test_cap_counts_the_cap():
    class Never(ScriptedModel):
        def thetaNewtonStep(self):
            return SimpleNamespace(norm_dx=1.0, norm_f1=1.0)

    st = ThetaStepper(Never(), dict(PARAMS, **{"adaptive time steps": False}))
    assert st.run() == 1
    assert st.newton_steps == 10 and not st.converged
