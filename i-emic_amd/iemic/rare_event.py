"""Rare-event drivers over a time-step function: naive Monte Carlo, GPA, AMS and TAMS.

Restates the reference's ``Transient<T>`` (src/transient/Transient.hpp, TransientDecl.hpp), the HDF5
``read`` / ``write`` of Transient.cpp, the score functions of ScoreFunctions.C and the rare-event
overloads of TransientFactory.H:104-198.  The drivers estimate the probability that a trajectory of
a noisy model leaves the neighbourhood of one steady state (A, score 0) and reaches another (B,
score 1) within "maximum time", and (AMS) the mean first-passage time.  A driver sees its model only
through

    time_step(x, dt) -> x'          one noisy time step (``get_time_step``, TransientFactory.H:55-67)
    dist_fun(x) -> score in [0, 1]  the score function

so the same code runs a two-variable SDE on the host, the projected model (x a small NumPy vector)
and the full model (x a ``DeviceVec``; the score then comes from one device pass, ``Ocean.score``).

The methods keep the reference's control flow line for line, including what looks accidental: the
time loops are ``t = dt; while t <= tmax: ...; t += dt`` (dt = 0.01, tmax = 2: 199 steps, not 200);
every experiment that shares the minimal ``max_distance`` is eliminated in the same iteration and
their number is recorded in ``ell``; a branch copies the donor's lists up to the first ``dlist``
entry that is not below the level; every tenth iteration drops the snapshots below the global
minimum; ``tams`` sets ``experiment.time = tlist[-1]``; alpha = (converged / N) prod (1 - l / N).

Deliberate departures from the reference:

1. *Random numbers.*  ``std::uniform_int_distribution`` over ``mt19937_64`` is
   implementation-defined and cannot be reproduced.  ``randint`` and ``randreal`` draw from a NumPy
   Philox generator keyed by "ams seed"; a seed of 0 takes one from the OS and ``ams_seed`` holds the
   one in use.  The reference declares ``int randreal(double, double)`` and its lambda takes ``int``
   bounds, so GPA's resampling value is truncated to an integer; here it is a real uniform in
   [0, sum).
2. *Extinction.*  When every unconverged experiment shares one ``max_distance`` and nothing is left
   to branch from, the reference spins through the remaining iterations doing nothing.  Here the
   loop ends and ``extinct`` is set; the estimate is what the formula gives.  (The loop also ends,
   without ``extinct``, once every experiment has converged.)
3. *MFPT with no return or no transition.*  With ``num_t2 == 0`` or ``converged == 0`` the reference
   divides by zero.  Here ``mfpt`` is nan, a warning is logged and ``probability`` stays -1.
4. *Optional sol3.*  The reference's projected factory dereferences a null ``sol3``; here
   ``sol3=None`` is accepted (the distance factor is 0.5).
5. *Noise on restart.*  The restart file also holds the stochastic stepper's ``draws`` counter
   (dataset ``data/noise draws``) and ``data/time steps``, so a resumed run continues the noise
   stream; the reference reseeds and replays the stream's start.
6. *GPA's likelihood ratio.*  A particle resampled with probability proportional to the weight w it
   had before the interval must be corrected by eta / w.  The reference (Transient.hpp:714-716)
   divides by the weight computed after the interval instead, so its product misses the first
   weight (1) and contains the last one: its estimate is that of E[1_B / W(final score)], about
   exp(-beta) times the transition probability when trajectories that reached B stay there (0.062
   against 0.156 on the reference's double well with beta = 1; the reference has no GPA test).
   Here the ratio divides by the weight the selection used.

Snapshots.  In the projected case a trajectory's state is the small vector and ``xlist`` holds
copies.  In the full space the state is a ``DeviceVec``; ``xlist`` holds device copies while their
total stays under "snapshot device memory (GB)" (default 8), and host arrays beyond that, which are
uploaded when branched from (``DeviceStates``).  Readers of the mismatching restart file get an
error, not a printed line.
"""
from __future__ import annotations

import copy
import logging
import math
import os
from typing import Callable, List, Optional

import numpy as np

log = logging.getLogger("iemic.rare_event")

__all__ = ["AMSExperiment", "GPAExperiment", "Transient", "HostStates", "DeviceStates", "mem2string",
           "default_score_function", "ocean_score_function", "projected_default_score_function",
           "projected_ocean_score_function", "transient_factory", "get_time_step"]


class AMSExperiment:
    """Transient.hpp:13-47"""

    def __init__(self, x0=None):
        self.x0 = x0
        self.xlist: list = []
        self.dlist: List[float] = []
        self.tlist: List[float] = []
        self.max_distance = 0.0
        self.time = 0.0
        self.initial_time = 0.0
        self.return_time = 0.0
        self.initialized = False
        self.converged = False


class GPAExperiment:
    """Transient.hpp:49-56"""

    def __init__(self, x=None):
        self.x = x
        self.weight = 1.0
        self.probability = 1.0
        self.distance = 0.0
        self.converged = False


def mem2string(mem) -> str:
    """Transient.cpp:19-33"""
    value, unit = float(int(mem)), "B"
    for u in ("kB", "MB", "GB", "TB"):
        if abs(value) > 1.0e3:
            value *= 1.0e-3
            unit = u
    return f"{value:.2f} {unit}"


class HostStates:
    """How a driver keeps, hands back and files the states of a host model (NumPy vectors):
    ``snapshot`` copies, ``restore`` hands the stored copy to the time step (which does not write
    into its argument)."""

    def snapshot(self, x):
        return np.array(x, dtype=np.float64, copy=True)

    def restore(self, s):
        return s

    def to_host(self, s) -> np.ndarray:
        return np.asarray(s, dtype=np.float64).reshape(-1)

    def from_host(self, a):
        return np.array(a, dtype=np.float64, copy=True)


class _DeviceSnapshot:
    """A device copy that counts against the snapshot budget for as long as anything holds it."""
    __slots__ = ("vec", "store")

    def __init__(self, vec, store):
        self.vec = vec
        self.store = store
        store.live += 1

    def __del__(self):
        self.store.live -= 1


class DeviceStates:
    """The same for the full model: a state is a ``DeviceVec``.  A snapshot is a device copy
    (``vec_ops().copy``) while the live copies stay under ``budget_gb``; beyond that it is a host
    array, uploaded when a trajectory restarts from it."""

    def __init__(self, model, budget_gb: float = 8.0):
        self.ops = model.vec_ops()
        self.bytes_per = 8 * int(model.N)
        self.budget = float(budget_gb) * 1.0e9
        self.live = 0
        self.on_host = 0                        # snapshots that went to the host

    def snapshot(self, x):
        if (self.live + 1) * self.bytes_per <= self.budget:
            return _DeviceSnapshot(self.ops.copy(x), self)
        self.on_host += 1
        return self.ops.to_host(x).copy()

    def restore(self, s):
        if isinstance(s, _DeviceSnapshot):
            return s.vec
        if isinstance(s, np.ndarray):
            return self.ops.from_host(s)
        return s                                # a DeviceVec (the caller's x0)

    def to_host(self, s) -> np.ndarray:
        if isinstance(s, np.ndarray):
            return s
        return self.ops.to_host(s.vec if isinstance(s, _DeviceSnapshot) else s).copy()

    def from_host(self, a):
        return self.snapshot(self.ops.from_host(np.asarray(a, dtype=np.float64)))


class Transient:
    """Transient<T> (TransientDecl.hpp, Transient.hpp).  ``states`` says how states are kept
    (``HostStates`` by default, ``DeviceStates`` for the full model); ``stepper``, if set, is the
    stochastic stepper behind ``time_step``, whose ``draws`` counter goes into the restart file."""

    def __init__(self, time_step: Callable, dist_fun: Optional[Callable] = None, x0=None,
                 vector_length: Optional[int] = None, states=None):
        self.time_step = time_step
        self.dist_fun = dist_fun
        self.method = "TAMS" if dist_fun is not None else "Transient"
        self.x0 = x0
        self.vector_length = 0 if vector_length is None else int(vector_length)
        self.states = HostStates() if states is None else states
        self.stepper = None
        self.mfpt = -1.0
        self.probability = -1.0
        self.extinct = False
        self.ams_seed = 0
        self._rng = None
        self.its = 0
        self.time_steps = 0
        self.time_steps_previous_write = 0
        self.ell: List[int] = []
        self.experiments: list = []
        self.set_parameters({})

    # ---- parameters (Transient.hpp:134-172) ---------------------------------------------------
    def set_parameters(self, params) -> None:
        p = params
        self.method = p.get("method", self.method)
        self.dt = float(p.get("time step", 0.01))
        self.tmax = float(p.get("maximum time", 1000.0))

        self.in_days = float(p.get("timescale in days", 737.2685))
        self.in_years = float(p.get("timescale in years", self.in_days / 365.))
        self.dt = float(p.get("time step (in y)", self.dt * self.in_years)) / self.in_years
        self.tmax = float(p.get("maximum time (in y)", self.tmax * self.in_years)) / self.in_years

        # GPA parameters
        self.tstep = float(p.get("GPA time step", 1.0))
        self.beta = float(p.get("beta", 1.0))

        # (T)AMS + GPA parameters
        self.bdist = float(p.get("B distance", 0.05))
        self.dist_tol = float(p.get("distance tolerance", 0.0005))
        self.num_exp = int(p.get("number of experiments", 1000))

        # AMS parameters
        self.adist = float(p.get("A distance", 0.05))
        self.cdist = float(p.get("C distance", 2 * self.adist))
        self.num_init_exp = int(p.get("number of initial experiments", self.num_exp))
        if self.num_init_exp < self.num_exp:
            self.num_init_exp = self.num_exp

        # (T)AMS parameters
        self.maxit = int(p.get("maximum iterations", self.num_exp * 10))

        # Writing parameters
        self.read_file = p.get("read file", "")
        self.write_file = p.get("write file", "")
        self.write_final = bool(p.get("write final state", True))
        self.write_steps = int(p.get("write steps", -1))
        self.write_time_steps = int(p.get("write time steps", -1))

    # ---- random numbers (departure 1) -----------------------------------------------------------
    def set_random_engine(self, seed: int) -> None:
        seed = int(seed)
        if seed < 0:
            raise ValueError(f'Transient: "ams seed" = {seed} must be >= 0')
        while seed == 0:
            seed = int.from_bytes(os.urandom(8), "little")
        self.ams_seed = seed
        self._rng = np.random.Generator(np.random.Philox(key=seed))

    def _engine(self):
        if self._rng is None:
            log.warning("Random engine not initialized.")
            self.set_random_engine(0)
        return self._rng

    def randint(self, a: int, b: int) -> int:
        """uniform integer in [a, b], both ends included"""
        return int(self._engine().integers(int(a), int(b) + 1))

    def randreal(self, a: float, b: float) -> float:
        """uniform real in [a, b)"""
        return float(a) + (float(b) - float(a)) * float(self._engine().random())

    # ---- the trajectories -------------------------------------------------------------------------
    def time_step_helper(self, x, dt):
        self.time_steps += 1
        return self.time_step(x, dt)

    def transient(self, x, dt, tmax):
        t = dt
        while t <= tmax:
            x = self.time_step_helper(x, dt)
            t += dt
        return x

    def transient_max_distance(self, x, dt, tmax, max_distance):
        lim = max_distance - self.bdist
        t = dt
        while t <= tmax:
            x = self.time_step_helper(x, dt)
            if self.dist_fun(x) > lim:
                return t
            t += dt
        return -1

    def transient_start(self, x0, dt, tmax, experiment: AMSExperiment) -> None:
        x = x0
        experiment.initial_time = 0.0
        t = dt
        while t <= tmax:
            x = self.time_step_helper(x, dt)
            dist = self.dist_fun(x)
            if dist > self.cdist:
                experiment.xlist.append(self.states.snapshot(x))
                experiment.dlist.append(dist)
                experiment.tlist.append(0)
                experiment.max_distance = dist
                experiment.initial_time = t
                experiment.initialized = True
                break
            t += dt

    def transient_ams(self, dt, tmax, experiment: AMSExperiment) -> None:
        x = self.states.restore(experiment.xlist[-1])
        t = experiment.tlist[-1] + dt
        tend = t + tmax
        max_distance = experiment.max_distance
        while t <= tend:
            x = self.time_step_helper(x, dt)
            dist = self.dist_fun(x)
            if dist < self.adist:
                if experiment.return_time < dt / 2.0:
                    experiment.return_time = t
                break
            elif dist > 1 - self.bdist:
                experiment.converged = True
                experiment.xlist.append(self.states.snapshot(x))
                experiment.tlist.append(t)
                experiment.dlist.append(1.0)
                max_distance = 1.0
                break
            if dist > max_distance + self.dist_tol:
                experiment.xlist.append(self.states.snapshot(x))
                experiment.tlist.append(t)
                experiment.dlist.append(dist)
                max_distance = dist
            t += dt
        experiment.max_distance = max_distance
        experiment.time = t

    def transient_tams(self, dt, tmax, experiment: AMSExperiment) -> None:
        x = self.states.restore(experiment.xlist[-1])
        t = experiment.tlist[-1] + dt
        max_distance = experiment.max_distance
        while t <= tmax:
            x = self.time_step_helper(x, dt)
            dist = self.dist_fun(x)
            if dist > 1 - self.bdist:
                experiment.converged = True
                experiment.xlist.append(self.states.snapshot(x))
                experiment.tlist.append(t)
                experiment.dlist.append(1.0)
                max_distance = 1.0
                break
            if dist > max_distance + self.dist_tol:
                experiment.xlist.append(self.states.snapshot(x))
                experiment.tlist.append(t)
                experiment.dlist.append(dist)
                max_distance = dist
            t += dt
        experiment.time = experiment.tlist[-1]
        experiment.max_distance = max_distance

    def transient_gpa(self, dt, tmax, experiment: GPAExperiment) -> None:
        x = self.states.restore(experiment.x)
        dist = -1
        t = dt
        while t <= tmax:
            x = self.time_step_helper(x, dt)
            dist = self.dist_fun(x)
            if dist > 1 - self.bdist:
                experiment.converged = True
            t += dt
        experiment.distance = dist
        experiment.x = x

    # ---- the methods ----------------------------------------------------------------------------------
    def naive(self, x0) -> None:
        experiments = [GPAExperiment() for _ in range(self.num_exp)]
        converged = 0
        for i in range(self.num_exp):
            experiments[i].x = x0
            experiments[i].converged = False
            self.transient_gpa(self.dt, self.tmax, experiments[i])
            if experiments[i].converged:
                converged += 1
        self.probability = converged / self.num_exp
        log.info("Transition probability T=%s: %s", _g(self.tmax), _g(self.probability))

    def ams_elimination(self, method: str, experiments: List[AMSExperiment], dt, tmax) -> float:
        converged = 0
        reactive_experiments = [experiments[i] for i in range(self.num_exp)]
        unconverged_experiments: List[AMSExperiment] = []
        unused_experiments: List[AMSExperiment] = []
        minimal_experiments: List[AMSExperiment] = []

        for exp in reactive_experiments:
            if not exp.converged:
                unconverged_experiments.append(exp)
            else:
                converged += 1
            unused_experiments.append(exp)

        # AMSExperiment::sort: the largest max_distance first, the minimal ones at the back
        unconverged_experiments.sort(key=lambda e: -e.max_distance)

        for _ in range(self.its, self.maxit):
            minimal_experiments = []
            if len(unconverged_experiments) > 0 and len(unused_experiments) > 0:
                minimal_exp = unconverged_experiments[-1]
                exp = unconverged_experiments[-1]
                while len(unconverged_experiments) > 0 and exp.max_distance == minimal_exp.max_distance:
                    minimal_experiments.append(exp)
                    unconverged_experiments.pop()
                    unused_experiments.remove(exp)
                    if len(unconverged_experiments) > 0:
                        exp = unconverged_experiments[-1]

            if len(minimal_experiments) == 0 or len(unused_experiments) == 0:
                # departure 2: the reference continues, and nothing can change any more
                if len(minimal_experiments) > 0:
                    self.extinct = True
                    log.warning("%s: all %d unconverged trajectories share the max distance %s and "
                                "none is left to branch from: extinct", method, len(minimal_experiments),
                                _g(minimal_experiments[0].max_distance))
                    unconverged_experiments.extend(minimal_experiments)
                    unused_experiments.extend(minimal_experiments)
                break

            self.ell.append(len(minimal_experiments))
            if self.ell[-1] == 1:
                log.info("Eliminating 1 trajectory.")
            else:
                log.info("Eliminating %d trajectories.", self.ell[-1])

            self.its += 1

            for exp in minimal_experiments:
                max_distance = exp.max_distance
                rnd_idx = self.randint(0, len(unused_experiments) - 1)
                while unused_experiments[rnd_idx].max_distance <= exp.max_distance:
                    rnd_idx = self.randint(0, len(unused_experiments) - 1)

                rnd_exp = unused_experiments[rnd_idx]
                if len(rnd_exp.dlist) == 0:
                    raise RuntimeError(f"Experiment {rnd_idx} has size 0.")

                same_distance_idx = 0
                while same_distance_idx < len(rnd_exp.dlist) and rnd_exp.dlist[same_distance_idx] < exp.max_distance:
                    same_distance_idx += 1

                if same_distance_idx == len(rnd_exp.dlist):
                    raise RuntimeError(f"Distance larger than {_g(exp.max_distance)} not found in experiment "
                                       f"with max distance {_g(rnd_exp.max_distance)}.")

                exp.xlist = list(rnd_exp.xlist[:same_distance_idx + 1])
                exp.dlist = list(rnd_exp.dlist[:same_distance_idx + 1])
                exp.tlist = list(rnd_exp.tlist[:same_distance_idx + 1])

                if method == "AMS":
                    self.transient_ams(dt, tmax, exp)
                elif method == "TAMS":
                    self.transient_tams(dt, tmax, exp)
                else:
                    raise ValueError(f"Method {method} does not exist.")

                if exp.converged:
                    converged += 1
                else:
                    unconverged_experiments.append(exp)

                log.info("%s: %d / %d, %d / %d converged with max distance %s -> %s and t=%s for experiment %d",
                         method, self.its, self.maxit, converged, self.num_exp, _g(max_distance),
                         _g(exp.max_distance), _g(exp.initial_time + exp.time),
                         _index(reactive_experiments, exp))

            for exp in minimal_experiments:
                unused_experiments.append(exp)

            unconverged_experiments.sort(key=lambda e: -e.max_distance)

            # Cleanup
            min_max_distance = 1.0
            for exp in reactive_experiments:
                min_max_distance = min(min_max_distance, exp.max_distance)

            if self.its % 10 == 0:
                log.info("Starting cleanup")
                for exp in unused_experiments:
                    min_max_idx = 0
                    while min_max_idx < len(exp.dlist) and exp.dlist[min_max_idx] < min_max_distance:
                        min_max_idx += 1
                    if min_max_idx > 0:
                        exp.xlist = exp.xlist[min_max_idx:]
                        exp.dlist = exp.dlist[min_max_idx:]
                        exp.tlist = exp.tlist[min_max_idx:]
                log.info("Finished cleanup")

            self.write_helper(experiments, self.its)
        log.info("")

        if self.write_final:
            self.write(self.write_file, experiments)

        alpha = converged / self.num_exp
        for l in self.ell:
            alpha *= 1.0 - l / self.num_exp
        return alpha

    def ams(self, x0) -> None:
        log.info("Using AMS with an estimated memory usage of: %s",
                 mem2string(int(1.0 / self.dist_tol * self.num_exp * self.vector_length * 8)))

        experiments = [AMSExperiment(x0) for _ in range(self.num_init_exp)]
        self.experiments = experiments

        self.its = 0
        self.time_steps = 0
        self.ell = []
        self.extinct = False

        if self.read_file != "":
            self.read(self.read_file, experiments)

        converged = 0
        tmax = 100 * self.tmax
        self.time_steps_previous_write = 0

        for i in range(self.num_init_exp):
            if experiments[i].initialized:
                continue

            self.transient_start(x0, self.dt, tmax, experiments[i])

            if len(experiments[i].xlist) == 0:
                raise RuntimeError("Initialization failed")

            self.transient_ams(self.dt, tmax, experiments[i])

            # Erase data that we do not need for later experiments
            if i >= self.num_exp:
                experiments[i].xlist = []
                experiments[i].dlist = []
                experiments[i].tlist = []

            if experiments[i].converged:
                converged += 1

            log.info("Initialization: %d / %d, %d / %d converged with t=%s", i + 1, self.num_init_exp, converged,
                     self.num_init_exp, _g(experiments[i].initial_time + experiments[i].time))

            self.write_helper(experiments, i + 1)
        log.info("")

        alpha = self.ams_elimination("AMS", experiments, self.dt, tmax)

        total_tr = 0.0
        total_t1 = 0.0
        total_t2 = 0.0
        num_t1 = self.num_init_exp
        num_t2 = 0
        converged = 0
        for i in range(self.num_exp):
            exp = experiments[i]
            total_tr += exp.time
            converged += int(exp.converged)

        for exp in experiments:
            total_t1 += exp.initial_time
            total_t2 += exp.return_time
            if exp.return_time > self.dt / 2.0:
                num_t2 += 1

        self.alpha = alpha
        log.info("Alpha: %s", _g(alpha))
        if num_t2 == 0 or converged == 0 or alpha == 0.0:
            # departure 3: the reference divides by zero here
            self.mfpt = math.nan
            log.warning("Mean first passage time undefined: %d returns to A, %d of %d experiments reached B",
                        num_t2, converged, self.num_exp)
            return
        meann = 1.0 / alpha - 1.0
        self.mfpt = meann * (total_t1 / num_t1 + total_t2 / num_t2) + total_t1 / num_t1 + total_tr / converged
        log.info("Mean first passage time: %s", _g(self.mfpt))

        self.probability = 1.0 - math.exp(-1.0 / self.mfpt * self.tmax)
        log.info("Transition probability T=%s: %s", _g(self.tmax), _g(self.probability))

    def tams(self, x0) -> None:
        log.info("Using TAMS with an estimated memory usage of: %s",
                 mem2string(int(self.tmax / self.dt * self.num_exp * self.vector_length * 8)))

        experiments = [AMSExperiment(x0) for _ in range(self.num_exp)]
        self.experiments = experiments

        self.its = 0
        self.time_steps = 0
        self.ell = []
        self.extinct = False

        if self.read_file != "":
            self.read(self.read_file, experiments)

        converged = 0
        self.time_steps_previous_write = 0

        start = None                            # one stored copy of x0, shared as the reference shares x0
        for i in range(self.num_exp):
            if experiments[i].initialized:
                continue

            if start is None:
                start = self.states.snapshot(x0)
            experiments[i].xlist.append(start)
            experiments[i].dlist.append(0)
            experiments[i].tlist.append(0)

            self.transient_tams(self.dt, self.tmax, experiments[i])

            experiments[i].initialized = True

            if experiments[i].converged:
                converged += 1

            log.info("Initialization: %d / %d, %d / %d converged with t=%s", i + 1, self.num_exp, converged,
                     self.num_exp, _g(experiments[i].time))

            self.write_helper(experiments, i + 1)
        log.info("")

        self.probability = self.ams_elimination("TAMS", experiments, self.dt, self.tmax)

        log.info("Transition probability T=%s: %s", _g(self.tmax), _g(self.probability))

    def gpa(self, x0) -> None:
        log.info("Using GPA with an estimated memory usage of: %s",
                 mem2string(int(self.num_exp * self.vector_length * 8)))

        experiments = [GPAExperiment() for _ in range(self.num_exp)]
        self.time_steps = 0

        def W(x):
            return math.exp(self.beta * x)

        for i in range(self.num_exp):
            experiments[i].x = x0
            experiments[i].weight = 1.0
            experiments[i].probability = 1.0
            experiments[i].distance = 0.0
            experiments[i].converged = False

        t = self.tstep
        while t <= self.tmax:
            # Compute the mean weight
            total = 0.0
            for i in range(self.num_exp):
                total += experiments[i].weight
            eta = 1.0 / self.num_exp * total

            old_experiments = [copy.copy(e) for e in experiments]

            # Sample based on the weights
            for i in range(self.num_exp):
                val = self.randreal(0.0, total)
                cumsum = 0.0
                for j in range(self.num_exp):
                    cumsum += old_experiments[j].weight
                    if cumsum >= val:
                        experiments[i] = copy.copy(old_experiments[j])
                        break
                    if j == self.num_exp - 1:
                        raise RuntimeError(f"Particle not found with sum {_g(total)} and random value {_g(val)}")

            # Step until the next tstep and recompute weights
            converged = 0
            for i in range(self.num_exp):
                selected_with = experiments[i].weight       # departure 6
                self.transient_gpa(self.dt, self.tstep, experiments[i])
                experiments[i].weight = W(experiments[i].distance)
                experiments[i].probability *= eta / selected_with
                if experiments[i].converged:
                    converged += 1

            log.info("GPA: %d / %d converged with t=%s and eta=%s", converged, self.num_exp, _g(t), _g(eta))
            t += self.tstep
        log.info("")

        self.probability = 0.0
        for i in range(self.num_exp):
            if experiments[i].converged:
                self.probability += experiments[i].probability
        self.probability /= self.num_exp

        log.info("Transition probability T=%s: %s", _g(self.tmax), _g(self.probability))

    def run(self, x0=None) -> int:
        x0 = self.x0 if x0 is None else x0
        if self.method == "AMS":
            self.ams(x0)
        elif self.method == "TAMS":
            self.tams(x0)
        elif self.method == "GPA":
            self.gpa(x0)
        elif self.method == "Naive":
            self.naive(x0)
        elif self.method == "Transient":
            self.transient(x0, self.dt, self.tmax)
        else:
            log.error("Method %s does not exist.", self.method)
            return -1
        return 0

    def get_probability(self) -> float:
        return self.probability

    def get_mfpt(self) -> float:
        return self.mfpt

    # ---- the restart file (Transient.cpp:39-214 through iemic.h5) ------------------------------------
    def write_helper(self, experiments, its: int) -> None:
        if self.write_file == "":
            return
        if self.write_steps > 0 and its % self.write_steps == 0:
            self.time_steps_previous_write = self.time_steps
            self.write(self.write_file, experiments)
            return
        if self.write_time_steps > 0 and self.time_steps - self.time_steps_previous_write >= self.write_time_steps:
            self.time_steps_previous_write = self.time_steps
            self.write(self.write_file, experiments)
            return

    def write(self, name: str, experiments: List[AMSExperiment]) -> None:
        if name == "":
            return
        from . import h5
        log.info("Writing current state to %s", name)
        if len(experiments) == 0 or len(experiments[0].xlist) == 0:
            return

        def i32(v):
            return np.array(int(v), dtype=np.int32)

        def multivector(s):
            v = self.states.to_host(s)
            return {"Values": np.asarray(v, dtype=np.float64).reshape(1, -1), "GlobalLength": i32(v.size),
                    "NumVectors": i32(1), "__type__": np.array([b"Epetra_MultiVector"], dtype="S19")}

        groups = {}
        for i, e in enumerate(experiments):
            size = len(e.dlist)
            g = {"size": i32(size), "max distance": np.array(float(e.max_distance)), "time": np.array(float(e.time)),
                 "initial time": np.array(float(e.initial_time)), "return time": np.array(float(e.return_time)),
                 "converged": i32(e.converged), "initialized": i32(e.initialized)}
            if size > 0:
                g["xlist"] = {str(j): multivector(s) for j, s in enumerate(e.xlist)}
                g["dlist"] = np.asarray(e.dlist, dtype=np.float64)
                g["tlist"] = np.asarray(e.tlist, dtype=np.float64)
            groups[str(i)] = g
        data = {"its": i32(self.its), "num exp": i32(self.num_exp), "num init exp": i32(self.num_init_exp),
                "ell size": i32(len(self.ell)), "time steps": np.array(int(self.time_steps), dtype=np.int64)}
        if self.ell:
            data["ell"] = np.asarray(self.ell, dtype=np.int32)
        if self.stepper is not None and hasattr(self.stepper, "draws"):
            data["noise draws"] = np.array(int(self.stepper.draws), dtype=np.int64)
        tmp = name + ".tmp"
        h5.write(tmp, {"experiments": groups, "data": data})
        os.replace(tmp, name)

    def read(self, name: str, experiments: List[AMSExperiment]) -> None:
        if name == "":
            return
        from . import h5
        log.info("Reading state from %s", name)
        if len(experiments) == 0:
            return
        t = h5.read(name)

        def scalar(path):
            if path not in t:
                raise ValueError(f"Transient.read: {name} holds no {path}")
            return t[path][0].reshape(-1)[0]

        num_exp = int(scalar("/data/num exp"))
        if self.num_exp != num_exp:
            raise ValueError(f"Transient.read: Number of experiments is {self.num_exp} instead of {num_exp}")
        num_init_exp = int(scalar("/data/num init exp"))
        if len(experiments) != num_exp and len(experiments) < num_init_exp:
            raise ValueError(f"Transient.read: Number of experiments is {len(experiments)} instead of "
                             f"{num_exp} or {num_init_exp}")
        self.its = int(scalar("/data/its"))
        ell_size = int(scalar("/data/ell size"))
        if ell_size > 0:
            self.ell = [int(v) for v in t["/data/ell"][0].reshape(-1)]
            if len(self.ell) != ell_size:
                raise ValueError(f"Transient.read: ell holds {len(self.ell)} entries, ell size says {ell_size}")
        # departure 5: the step count and the noise stream go on where the file left them
        if "/data/time steps" in t:
            self.time_steps = int(scalar("/data/time steps"))
        if "/data/noise draws" in t and self.stepper is not None and hasattr(self.stepper, "draws"):
            self.stepper.draws = int(scalar("/data/noise draws"))

        for i, e in enumerate(experiments):
            g = f"/experiments/{i}"
            size = int(scalar(f"{g}/size"))
            e.max_distance = float(scalar(f"{g}/max distance"))
            e.time = float(scalar(f"{g}/time"))
            e.initial_time = float(scalar(f"{g}/initial time"))
            e.return_time = float(scalar(f"{g}/return time"))
            e.converged = bool(scalar(f"{g}/converged"))
            e.initialized = bool(scalar(f"{g}/initialized"))
            if size > 0:
                e.xlist = []
                for j in range(size):
                    path = f"{g}/xlist/{j}/Values"
                    if path not in t:
                        raise ValueError(f"Transient.read: {name} holds no {path}")
                    v = np.asarray(t[path][0], dtype=np.float64).reshape(-1)
                    if self.vector_length and v.size != self.vector_length:
                        raise ValueError(f"Transient.read: {path} has {v.size} entries, the model's states "
                                         f"have {self.vector_length}")
                    e.xlist.append(self.states.from_host(v))
                e.dlist = [float(v) for v in t[f"{g}/dlist"][0].reshape(-1)]
                e.tlist = [float(v) for v in t[f"{g}/tlist"][0].reshape(-1)]
                if len(e.dlist) != size or len(e.tlist) != size:
                    raise ValueError(f"Transient.read: {g} holds {len(e.dlist)} distances and {len(e.tlist)} "
                                     f"times, size says {size}")


def _g(v) -> str:
    """a number as the reference's stream prints it (six significant digits)"""
    return f"{v:.6g}"


def _index(seq, item) -> int:
    for i, s in enumerate(seq):
        if s is item:
            return i
    return len(seq)


# ---- score functions (ScoreFunctions.C) ----------------------------------------------------------------
def _dist(f: float, d1: float, d2: float) -> float:
    return f - f * math.exp(-0.5 * (d1 / 0.25) ** 2.) + (1.0 - f) * math.exp(-0.5 * (d2 / 0.25) ** 2.)


def _host_score(norm, sol1, sol2, sol3):
    sol1 = np.asarray(sol1, dtype=np.float64).reshape(-1)
    sol2 = np.asarray(sol2, dtype=np.float64).reshape(-1)
    nrm = norm(sol1 - sol2)
    if not (nrm > 0.0 and math.isfinite(nrm)):
        raise ValueError(f"score function: ||sol1 - sol2|| = {nrm} must be positive and finite")
    dist_factor = 0.5
    if sol3 is not None:
        dist_factor = norm(sol1 - np.asarray(sol3, dtype=np.float64).reshape(-1)) / nrm
    log.info("distance factor = %s", _g(dist_factor))

    def score(x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        d1 = norm(x - sol1) / nrm
        d2 = norm(x - sol2) / nrm
        return _dist(dist_factor, d1, d2)
    score.nrm, score.dist_factor = nrm, dist_factor
    return score


def _device_score(model, sol1, sol2, sol3, var):
    model.scoreSet(sol1, sol2, sol3, var)
    nrm, dist_factor = model.scoreGet()
    log.info("distance factor = %s", _g(dist_factor))
    ops = model.vec_ops()

    def score(x=None):
        """x: a DeviceVec, a stored device snapshot, a host vector, or None for the model's state"""
        if isinstance(x, _DeviceSnapshot):
            x = x.vec
        elif isinstance(x, np.ndarray):
            x = ops.from_host(x)
        return model.score(x)[0]
    score.nrm, score.dist_factor = nrm, dist_factor
    return score


def default_score_function(model, sol1, sol2, sol3=None):
    """get_default_score_function (ScoreFunctions.C:32-66): distances over all rows.  With a model
    the score is evaluated on the device (``Ocean.scoreSet`` with var = -1, one pass per
    evaluation); ``model=None`` gives the same function on host vectors."""
    log.info("Using the default score function")
    if model is None:
        return _host_score(lambda v: float(np.linalg.norm(v)), sol1, sol2, sol3)
    return _device_score(model, sol1, sol2, sol3, -1)


def ocean_score_function(model, sol1, sol2, sol3=None):
    """get_ocean_score_function (ScoreFunctions.C:114-190): distances over the v rows
    (GID % 6 == 1, land rows included).  ``model=None``: on host vectors."""
    log.info("Using the ocean score function")
    if model is None:
        return _host_score(lambda v: float(np.linalg.norm(v[1::6])), sol1, sol2, sol3)
    return _device_score(model, sol1, sol2, sol3, 1)


def _projected_score(y1, y2, y3, M):
    M = np.asarray(M, dtype=np.float64)
    k = np.asarray(y1).size
    if M.shape != (k, k):
        raise ValueError(f"projected score function: the Gram matrix has shape {M.shape}, the small vectors "
                         f"have {k} entries")

    def norm(y):
        return math.sqrt(float(y @ (M @ y)))
    return _host_score(norm, y1, y2, y3)


def projected_default_score_function(y1, y2, y3, VV):
    """get_projected_default_score_function (ScoreFunctions.C:68-112) on the restricted states:
    ||y|| = sqrt(y^T VV y) with VV = V^T V, which is ||V y||_2 also when V is not orthonormal."""
    log.info("Using the default projected score function")
    return _projected_score(y1, y2, y3, VV)


def projected_ocean_score_function(y1, y2, y3, VvvV):
    """get_projected_ocean_score_function (ScoreFunctions.C:192-248): the same with
    VvvV = V^T diag(e_v) V, the v rows of V y."""
    log.info("Using the projected ocean score function")
    return _projected_score(y1, y2, y3, VvvV)


# ---- the factory (TransientFactory.H:55-67, :104-198) ---------------------------------------------------
def get_time_step(stepper):
    """x, dt -> the state after one time step: setState, initStep, Newton::run, and Newton's last
    iterate whether it converged or not"""
    return stepper.step


def transient_factory(model, params, sol1, sol2, sol3=None, V=None) -> Transient:
    """TransientFactory(model, pars, sol1, sol2, sol3[, V]).  "space" in params names a Matrix Market
    file V is loaded from (``load_space``).  With V: ``StochasticProjectedThetaStepper``, sol1..3
    restricted with V, the projected score function chosen by params["dof"] == 6, x0 the restricted
    sol1 and ``vector_length`` k.  Without: ``StochasticThetaStepper``, the device score function
    and x0 = sol1 on the device.  sol3 may be None (departure 4)."""
    from .transient import StochasticProjectedThetaStepper, StochasticThetaStepper, load_space, _DERIVED
    params = dict(params)
    space = params.get("space", "")
    if V is None and space != "":
        V = load_space(space, model.N)
    sp = {k: v for k, v in params.items() if k in StochasticThetaStepper.defaults or k in _DERIVED}
    ocean = params.get("dof", 1) == 6
    if V is not None:
        stepper = StochasticProjectedThetaStepper(model, V, sp)

        def restrict(s):
            if s is None:
                return None
            model.setState(np.asarray(s, dtype=np.float64))
            return np.array(model.projRestrictState(), dtype=np.float64)
        y1, y2, y3 = restrict(sol1), restrict(sol2), restrict(sol3)
        if ocean:
            score_fun = projected_ocean_score_function(y1, y2, y3, model.projGramVV(1))
        else:
            score_fun = projected_default_score_function(y1, y2, y3, model.projGramVV(-1))
        tr = Transient(get_time_step(stepper), score_fun, y1, stepper.k)
    else:
        stepper = StochasticThetaStepper(model, sp)
        score_fun = (ocean_score_function if ocean else default_score_function)(model, sol1, sol2, sol3)
        states = DeviceStates(model, float(params.get("snapshot device memory (GB)", 8.0)))
        x0 = states.ops.from_host(np.asarray(sol1, dtype=np.float64))
        tr = Transient(get_time_step(stepper), score_fun, x0, int(model.N), states=states)
    tr.stepper = stepper
    tr.set_parameters(params)
    tr.set_random_engine(int(params.get("ams seed", 0)))
    return tr
