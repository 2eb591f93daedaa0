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
in place of ``thetaInitStep``, with m fresh standard normals.  The projected stochastic model,
AMS / TAMS / GPA, their score functions and CoupledThetaModel are not restated.
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
                m.thetaRestore()
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
                float(np.linalg.norm(m.getState())), self.newton_steps, self.dt))
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
