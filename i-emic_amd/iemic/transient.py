"""The deterministic theta time stepper over the GPU ocean model.

Restates the loop ``TransientFactory(ocean, params)`` builds in the reference
(src/transient/TransientFactory.H): ``AdaptiveTransient`` (AdaptiveTransient.H:88-171)
running ``Newton`` (Newton.H:76-123) on ``ThetaModel<Ocean>`` (ThetaModel.H).  The theta
model itself -- x_n and F_n, the residual F_theta(x) = dt theta F(x) + dt (1 - theta) F_n +
B (x_n - x), the shifted Jacobian J - B / dt / theta and the scaled solve -- lives in the
device library (csrc/theta.hip); this module is the stepping logic, which drives its model
only through

    preProcess()                     the preconditioner is refactored at the step's first solve
    thetaInitStep(dt, theta)         x_n <- state, F_n <- F(x_n)
    thetaNewtonStep() -> info        one Newton iteration; info.norm_dx = ||dx||_inf,
                                     info.norm_f1 = ||F_theta||_2 after the update
    thetaRestore()                   state <- x_n
    getState()

(and ``postProcess`` / ``saveStateToFile`` where the model has them), so a CPU model with the
same surface can stand in for ``iemic.ocean.Ocean``.  Parameter names and defaults are the
reference's (AdaptiveTransient.H:60-68, Newton.H:50-51, ThetaModel.H:37,
Transient.hpp:138-145).

``StochasticThetaStepper`` is the same loop on ``StochasticThetaModel<Ocean>``
(StochasticThetaModel.H): every step starts with ``stochasticInitStep(dt, theta, sigma, pert)``
in place of ``thetaInitStep``, with m fresh standard normals.

``ProjectedThetaStepper`` and ``StochasticProjectedThetaStepper`` are the loop on
``ProjectedThetaModel<Ocean>`` and ``StochasticProjectedThetaModel<Ocean>``
(ProjectedThetaModel.H, StochasticProjectedThetaModel.H; TransientFactory.H:115-133 builds them
when a "space" V is given, ``load_space`` reads it): the state is confined to x = V y and the
stepper works on the small vector y.  A time step's Newton system is the k x k matrix
V^T (J - B / dt / theta) V, factored once per step in the device library (csrc/projected.hip);
no preconditioner is set up and no Krylov solver runs.  The model surface is

    projSetState(y)                  state <- V y, small state <- y
    projInitStep(dt, theta)          y_n, F_n, V^T B V, V^T J2 V and its factors
    projStochasticInitStep(dt, theta, sigma, pert)
    projNewtonStep() -> info         one Newton iteration on y; info.norm_dx = ||dy||_inf,
                                     info.norm_f1 = ||r||_2 after the update
    projRestore()                    state as at the init step
    projRestrictState(), projGet("y")

The theta = 0 branch of the reference's projected model is left out, as theta = 0 is
everywhere here.  The rare-event drivers over these steppers (naive Monte Carlo, GPA, AMS, TAMS) and
their score functions are in ``iemic.rare_event``; CoupledThetaModel is not restated.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass

import numpy as np

DEFAULTS = {
    # Transient.hpp:138-145 ("time step (in y)" and "maximum time (in y)" override when given)
    "time step": 0.01, "maximum time": 1000.0, "timescale in days": 737.2685,
    # ThetaModel.H:37
    "theta": 1.0,
    # Newton.H:50-51
    "Newton tolerance": 1e-8, "maximum Newton iterations": 20,
    # AdaptiveTransient.H:60-68
    "adaptive time steps": False, "minimum desired Newton iterations": 3,
    "maximum desired Newton iterations": 3, "minimum time step": 1.0e-8,
    "maximum time step": 1.0, "time step increase": 2.0, "time step decrease": 2.0,
    "number of time steps": 10, "HDF5 output frequency": 1,
}
_DERIVED = ("timescale in years", "time step (in y)", "maximum time (in y)")


@dataclass
class TransientRecord:
    """One accepted time step: a line of the reference's tdata.txt
    (AdaptiveTransient::writeData, AdaptiveTransient.H:175-214), with the nondimensional
    time step beside the one in years."""
    time_y: float
    step: int
    dt_y: float
    norm_x: float
    newton_steps: int
    dt: float


class ThetaStepper:
    """AdaptiveTransient<ThetaModel<Model>>: ``run()`` steps the model from its current state."""

    defaults = DEFAULTS

    def __init__(self, model, params=None):
        p = dict(self.defaults)
        for k, v in (params or {}).items():
            if k not in self.defaults and k not in _DERIVED:
                raise KeyError(f"{type(self).__name__}: unknown parameter {k!r}")
            p[k] = v
        self.model = model
        self.params = p
        self.theta = float(p["theta"])
        if not (0.0 < self.theta <= 1.0):
            raise ValueError(f'ThetaStepper: "theta" = {self.theta} is outside (0, 1]: theta = 0 divides '
                             "by the mass matrix, which is zero on the W, P, land and "
                             "integral-condition rows")
        self.in_years = float(p.get("timescale in years", float(p["timescale in days"]) / 365.0))
        # Transient.hpp:144-145 converts to years and back; a value given without its "(in y)"
        # form is taken as it stands, so it is not moved by that round trip's rounding
        self.dt = (float(p["time step (in y)"]) / self.in_years if "time step (in y)" in p
                   else float(p["time step"]))
        self.tmax = (float(p["maximum time (in y)"]) / self.in_years if "maximum time (in y)" in p
                     else float(p["maximum time"]))
        if not self.dt > 0.0:
            raise ValueError(f'ThetaStepper: "time step" = {self.dt} must be positive')
        self.tol = float(p["Newton tolerance"])
        self.max_newton = int(p["maximum Newton iterations"])
        self.adaptive = bool(p["adaptive time steps"])
        self.min_wanted = int(p["minimum desired Newton iterations"])
        self.max_wanted = int(p["maximum desired Newton iterations"])
        self.dt_min = float(p["minimum time step"])
        self.dt_max = float(p["maximum time step"])
        self.increase = float(p["time step increase"])
        self.decrease = float(p["time step decrease"])
        self.nsteps = int(p["number of time steps"])
        self.output = int(p["HDF5 output frequency"])
        self.time = 0.0
        self.time_steps = 0
        self.history: list[TransientRecord] = []
        self.rejected: list[float] = []          # the time steps of the failed Newton runs
        self._total = 0
        # the last Newton run (Newton.H's converged(), steps(), normF(), normdx())
        self.converged = False
        self.newton_steps = 0
        self.normF = -1.0
        self.normdx = math.nan

    def total_newton_steps(self) -> int:
        """The sum over the accepted time steps of Newton::steps(): the loop index at the
        return (Newton.H:92-110), so a run that converges in its k-th iteration counts k - 1
        and one that hits the cap counts the cap."""
        return self._total

    def _newton(self) -> None:
        """Newton::run (Newton.H:76-123) on the initialised theta step."""
        self.converged = False
        self.normF = -1.0
        self.newton_steps = 0
        while self.newton_steps < self.max_newton:
            info = self.model.thetaNewtonStep()
            self.normdx, self.normF = float(info.norm_dx), float(info.norm_f1)
            if self.normdx < self.tol and self.normF < self.tol:
                self.converged = True
                return
            if self.normdx > 1e2:
                return
            self.newton_steps += 1

    def _init_step(self) -> None:
        """The model call that starts a time step (ThetaModel::initStep), also after a rejected one."""
        self.model.thetaInitStep(self.dt, self.theta)

    def _restore(self) -> None:
        """AdaptiveTransient.H:107 after a failed Newton run"""
        self.model.thetaRestore()

    def _norm_x(self) -> float:
        """||x|| of an accepted step, tdata.txt's column"""
        return float(np.linalg.norm(self.model.getState()))

    def step(self, x, dt: float):
        """One time step of length dt from the state x -> the new state: the time-step function
        ``get_time_step`` builds (TransientFactory.H:55-67: setState, initStep, Newton::run), which
        returns Newton's last iterate, converged or not (``converged`` says which).  x is a
        ``DeviceVec`` of the model (the result is a new one; nothing goes through the host) or a
        host vector (the result is one too).  Mirrors ``ProjectedThetaStepper.step``."""
        m = self.model
        host = isinstance(x, np.ndarray)
        if host:
            m.setState(x)
        else:
            m.vec_ops().set_state(x)
        self.dt = float(dt)
        m.preProcess()
        self._init_step()
        self._newton()
        return m.getState().copy() if host else m.vec_ops().state()

    def run(self) -> int:
        """AdaptiveTransient::run (AdaptiveTransient.H:88-171).  Returns 0, or 1 when a Newton
        run failed at the minimum time step or with adaptivity off."""
        m = self.model
        self.time, self.time_steps = 0.0, 0
        while self.time < self.tmax and (self.nsteps < 0 or self.time_steps < self.nsteps):
            m.preProcess()
            self._init_step()
            self._newton()
            if not self.converged:
                self._restore()
                self.rejected.append(self.dt)
                if self.dt == self.dt_min or not self.adaptive:
                    return 1
                self.dt = max(self.dt / self.decrease, self.dt_min)
                continue
            self.time_steps += 1
            self.time += self.dt
            if hasattr(m, "postProcess"):
                m.postProcess()
            if self.output > 0 and self.time_steps % self.output == 0:
                m.saveStateToFile(f"transient_{self.time:.8g}.h5")
            self.history.append(TransientRecord(
                self.time * self.in_years, self.time_steps, self.dt * self.in_years,
                self._norm_x(), self.newton_steps, self.dt))
            if self.adaptive and self.newton_steps < self.min_wanted:
                self.dt = min(self.dt * self.increase, self.dt_max)
            elif self.adaptive and self.newton_steps > self.max_wanted:
                self.dt = max(self.dt / self.decrease, self.dt_min)
            self._total += self.newton_steps
        return 0


class StochasticThetaStepper(ThetaStepper):
    """AdaptiveTransient<StochasticThetaModel<Model>>: the theta stepper with noise on the
    salinity flux.  The model adds ``stochasticInitStep(dt, theta, sigma, pert)`` to the surface
    ThetaStepper drives and says how many latitudes it has (``cfg.m``); nothing else of the loop
    changes, so a step the adaptive loop rejects starts again with a new draw, as the reference's
    ``initStep`` does.

    Parameters beside ThetaStepper's: "sigma" (StochasticThetaModel.H:35, default 1.0, >= 0) and
    "noise seed" (StochasticBase; 0 takes a seed from the OS, and ``noise_seed`` holds the one in
    use either way).  ``draws`` counts the blocks drawn: accepted plus rejected steps.

    The noise of block b is ``noise_block(noise_seed, b, m)``: m standard normals from NumPy's
    counter-based Philox generator, keyed by the seed, its counter set to the block.  A block
    depends on (seed, b) alone: not on the blocks before it, the time steps taken or the number of
    ranks (every rank draws the same m values; the device keeps the latitudes it owns).  This is
    NOT the reference's stream and cannot be: there every process seeds its own ``mt19937_64``
    and draws for the columns it holds, so the noise changes with the number of processes, and
    ``std::normal_distribution`` is implementation-defined, so it changes with the C++ library.

    ``pert_source(block, m)``, if given, replaces the generator (a rare-event driver that chooses
    its noise; the tests).  What it returns must be m finite numbers."""

    defaults = dict(DEFAULTS, **{"sigma": 1.0, "noise seed": 0})

    def __init__(self, model, params=None, pert_source=None):
        super().__init__(model, params)
        self.sigma = float(self.params["sigma"])
        if not (math.isfinite(self.sigma) and self.sigma >= 0.0):
            raise ValueError(f'StochasticThetaStepper: "sigma" = {self.sigma} must be finite and >= 0')
        seed = int(self.params["noise seed"])
        if seed < 0:
            raise ValueError(f'StochasticThetaStepper: "noise seed" = {seed} must be >= 0')
        if seed == 0 and pert_source is None:
            while seed == 0:
                seed = int.from_bytes(os.urandom(8), "little")
        self.noise_seed = seed
        self.pert_source = pert_source
        self.draws = 0

    @staticmethod
    def noise_block(seed: int, block: int, m: int) -> np.ndarray:
        """Block ``block`` of the stream of ``seed``: m standard normals."""
        bits = np.random.Philox(key=int(seed), counter=[0, int(block), 0, 0])
        return np.random.Generator(bits).standard_normal(int(m))

    def _pert(self) -> np.ndarray:
        m = int(self.model.cfg.m)
        if self.pert_source is not None:
            pert = np.asarray(self.pert_source(self.draws, m), dtype=np.float64).reshape(-1)
        else:
            pert = self.noise_block(self.noise_seed, self.draws, m)
        if pert.size != m:
            raise ValueError(f"StochasticThetaStepper: pert has {pert.size} entries, the model has "
                             f"{m} latitudes")
        if not np.all(np.isfinite(pert)):
            raise ValueError(f"StochasticThetaStepper: pert[{int(np.flatnonzero(~np.isfinite(pert))[0])}] "
                             "is not finite")
        self.draws += 1
        return pert

    def _init_step(self) -> None:
        """StochasticThetaModel::initStep (StochasticThetaModel.H:52-72)"""
        self.model.stochasticInitStep(self.dt, self.theta, self.sigma, self._pert())


class ProjectedThetaStepper(ThetaStepper):
    """The time stepper on ProjectedThetaModel<Model> with the space V (N x k, 1 <= k <= 64, not
    necessarily orthonormal): ``step(y, dt)`` is the time-step function ``get_time_step`` builds
    (TransientFactory.H:55-67: setState, initStep, Newton::run on the small vector), and ``run()``
    is ThetaStepper's loop with its parameters over it, from y = V^T state of the model's current
    state.  ``y`` holds the small state; the history's norm_x is ||y||_2.  A rejected step puts
    the model's state back (``projRestore``) and leaves y as it was."""

    def __init__(self, model, V, params=None, **kw):
        super().__init__(model, params, **kw)
        V = np.asarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[1] < 1:
            raise ValueError(f"{type(self).__name__}: V must be an N x k array, not of shape {V.shape} "
                             "(the model says how many columns it takes: the device library 64)")
        self.k = V.shape[1]
        model.projSetBasis(V)
        self.y = np.asarray(model.projRestrictState(), dtype=np.float64).copy()

    def _proj_init(self) -> None:
        self.model.projInitStep(self.dt, self.theta)

    def _init_step(self) -> None:
        """get_time_step's setState and initStep (TransientFactory.H:63-64)"""
        self.model.projSetState(self.y)
        self._proj_init()

    def _newton(self) -> None:
        """Newton::run (Newton.H:76-123) on the small vector of the initialised step"""
        self.converged = False
        self.normF = -1.0
        self.newton_steps = 0
        while self.newton_steps < self.max_newton:
            info = self.model.projNewtonStep()
            self.normdx, self.normF = float(info.norm_dx), float(info.norm_f1)
            if self.normdx < self.tol and self.normF < self.tol:
                self.converged = True
                self.y = np.asarray(self.model.projGet("y"), dtype=np.float64).copy()
                return
            if self.normdx > 1e2:
                return
            self.newton_steps += 1

    def _restore(self) -> None:
        self.model.projRestore()

    def _norm_x(self) -> float:
        return float(np.linalg.norm(self.y))

    def step(self, y, dt: float) -> np.ndarray:
        """One time step of length dt from the small state y -> the new small state (Newton's
        last iterate, converged or not: ``converged`` says which, as Newton::run returns x)."""
        self.y = np.array(y, dtype=np.float64).reshape(-1)
        if self.y.size != self.k:
            raise ValueError(f"{type(self).__name__}: y has {self.y.size} entries, V has {self.k} columns")
        self.dt = float(dt)
        self._init_step()
        self._newton()
        if not self.converged:
            self.y = np.asarray(self.model.projGet("y"), dtype=np.float64).copy()
        return self.y.copy()


class StochasticProjectedThetaStepper(ProjectedThetaStepper, StochasticThetaStepper):
    """The same on StochasticProjectedThetaModel<Model>: every step starts with
    ``projStochasticInitStep(dt, theta, sigma, pert)``.  "sigma", "noise seed", ``pert_source``, the
    Philox blocks and ``draws`` are StochasticThetaStepper's, unchanged: a rejected step draws again."""

    defaults = StochasticThetaStepper.defaults

    def __init__(self, model, V, params=None, pert_source=None):
        # ProjectedThetaStepper's constructor hands pert_source on to StochasticThetaStepper's
        super().__init__(model, V, params, pert_source=pert_source)

    def _proj_init(self) -> None:
        """StochasticProjectedThetaModel::initStep (StochasticProjectedThetaModel.H:71-92)"""
        self.model.projStochasticInitStep(self.dt, self.theta, self.sigma, self._pert())


def load_space(path: str, nrows: int = None) -> np.ndarray:
    """The "space" parameter's file (TransientFactory.H:177-196): a Matrix Market *array* file, as
    ``EpetraExt::MatrixMarketFileToMultiVector`` reads it (real, general, column-major values, one
    per line) -> an N x k array.  nrows, if given, is the model's row count, which N must equal.
    A coordinate file, another field or symmetry, a size line that is not two positive integers
    and a wrong number of values are refused by name."""
    with open(path) as f:
        head = f.readline().split()
        if len(head) < 5 or head[0] != "%%MatrixMarket" or head[1].lower() != "matrix":
            raise ValueError(f"load_space: {path} is not a Matrix Market matrix file")
        fmt, field, sym = (h.lower() for h in head[2:5])
        if fmt != "array":
            raise ValueError(f'load_space: {path} is in "{fmt}" format; the space must be an "array" file')
        if field not in ("real", "double", "integer") or sym != "general":
            raise ValueError(f'load_space: {path} holds a "{field} {sym}" matrix; "real general" is needed')
        line = f.readline()
        while line and (line.startswith("%") or not line.strip()):
            line = f.readline()
        size = line.split()
        if len(size) != 2 or not all(t.isdigit() for t in size) or int(size[0]) < 1 or int(size[1]) < 1:
            raise ValueError(f"load_space: {path}: the size line {line.strip()!r} is not 'rows columns'")
        n, k = int(size[0]), int(size[1])
        if nrows is not None and n != int(nrows):
            raise ValueError(f"load_space: {path} has {n} rows, the model has {int(nrows)}")
        if k > 64:
            raise ValueError(f"load_space: {path} has {k} columns, at most 64 are supported")
        vals = np.array(f.read().split(), dtype=np.float64)
    if vals.size != n * k:
        raise ValueError(f"load_space: {path} holds {vals.size} values, its size line says {n} x {k}")
    return np.ascontiguousarray(vals.reshape(k, n).T)
