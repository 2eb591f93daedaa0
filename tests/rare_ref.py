"""The reference's own rare-event test problem (src/tests/test_ams.C) and independent estimates of
what the drivers of iemic.rare_event should find on it.  Nothing here imports the code under test.

    dx0 = (x0 - x0^3) dt + sqrt(dt) sigma xi0
    dx1 =      -2 x1  dt + sqrt(dt) sigma xi1          explicit Euler (theta = 0)

sigma = 1, dt = 0.01, maximum time 2, B distance 0.05, sol1 = (-1, 0), sol2 = (1, 0), sol3 = (0, 0)
and the default score function of ScoreFunctions.C.  The time loop is the reference's
``t = dt; while t <= tmax: t += dt``: 199 steps.

P_REF is the transition probability by a vectorised naive Monte Carlo of exactly this process and
score, 400,000 trajectories of 199 steps: 0.15623 +- 0.00057 (one standard error) when the feature
was specified, and 0.15651 +- 0.00057 by ``naive_probability()`` with the seed below (the two runs
agree within their errors; the tests use the first, as specified); the reference's tests expect
0.157.  MFPT_REF is the mean first-passage time from sol1 to score > 1 - B distance by
``naive_mfpt()``: 6.890 +- 0.042 over 20,000 trajectories, none unfinished at t = 200.
"""
import math

import numpy as np

SIGMA, DT, TMAX, BDIST = 1.0, 0.01, 2.0, 0.05
SOL1, SOL2, SOL3 = np.array([-1.0, 0.0]), np.array([1.0, 0.0]), np.array([0.0, 0.0])

P_REF = 0.1562          # naive Monte Carlo, 400,000 trajectories: 0.15623 +- 0.00057
MFPT_REF = 6.89         # naive_mfpt(): 6.890 +- 0.042


def loop_steps(dt=DT, tmax=TMAX) -> int:
    """the number of passes of the reference's time loop"""
    n, t = 0, dt
    while t <= tmax:
        n += 1
        t += dt
    return n


def scores(X) -> np.ndarray:
    """get_default_score_function on the rows of X (n x 2)"""
    nrm = np.linalg.norm(SOL1 - SOL2)
    f = np.linalg.norm(SOL1 - SOL3) / nrm
    d1 = np.linalg.norm(X - SOL1, axis=1) / nrm
    d2 = np.linalg.norm(X - SOL2, axis=1) / nrm
    return f - f * np.exp(-0.5 * (d1 / 0.25) ** 2) + (1.0 - f) * np.exp(-0.5 * (d2 / 0.25) ** 2)


def euler(X, xi, dt=DT, sigma=SIGMA):
    """one step of all rows of X with the normals xi (same shape)"""
    F = np.stack([X[:, 0] - X[:, 0] ** 3, -2.0 * X[:, 1]], axis=1)
    return X + dt * F + math.sqrt(dt) * sigma * xi


def naive_probability(ntraj=400_000, seed=20261021, chunk=100_000):
    """(p, standard error): the share of trajectories from sol1 whose score exceeds 1 - B distance
    at one of the loop's steps"""
    rng = np.random.Generator(np.random.Philox(key=seed))
    hits = 0
    for lo in range(0, ntraj, chunk):
        n = min(chunk, ntraj - lo)
        X = np.tile(SOL1, (n, 1))
        hit = np.zeros(n, dtype=bool)
        for _ in range(loop_steps()):
            X = euler(X, rng.standard_normal((n, 2)))
            hit |= scores(X) > 1.0 - BDIST
        hits += int(hit.sum())
    p = hits / ntraj
    return p, math.sqrt(p * (1.0 - p) / ntraj)


def naive_mfpt(ntraj=20_000, seed=20261021, tcap=200.0):
    """(mean, standard error, unfinished): the first time the score of a trajectory from sol1 exceeds
    1 - B distance, over ntraj trajectories; the ones still under way at tcap count with tcap
    (20,000 trajectories, tcap 200: none unfinished)"""
    rng = np.random.Generator(np.random.Philox(key=seed))
    X = np.tile(SOL1, (ntraj, 1))
    T = np.full(ntraj, np.nan)
    alive = np.arange(ntraj)
    t = DT
    while alive.size and t <= tcap:
        X = euler(X, rng.standard_normal((alive.size, 2)))
        done = scores(X) > 1.0 - BDIST
        T[alive[done]] = t
        alive, X = alive[~done], X[~done]
        t += DT
    T[alive] = tcap
    return float(T.mean()), float(T.std(ddof=1) / math.sqrt(ntraj)), int(alive.size)


class DoubleWell:
    """``time_step(x, dt)`` of the process for one trajectory at a time: the normals of step b are
    block b of a Philox stream keyed by the seed, as iemic.transient's stochastic steppers draw."""

    def __init__(self, seed: int, sigma: float = SIGMA):
        self.seed, self.sigma, self.draws = int(seed), float(sigma), 0
        self._buf, self._at = None, 0

    def _normals(self):
        if self._buf is None or self._at == len(self._buf):
            bits = np.random.Philox(key=self.seed, counter=[0, self.draws, 0, 0])
            self._buf, self._at = np.random.Generator(bits).standard_normal((4096, 2)), 0
        xi = self._buf[self._at]
        self._at += 1
        self.draws += 1
        return xi

    def __call__(self, x, dt):
        xi = self._normals()
        s = math.sqrt(dt) * self.sigma
        return np.array([x[0] + dt * (x[0] - x[0] ** 3) + s * xi[0], x[1] + dt * (-2.0 * x[1]) + s * xi[1]])


if __name__ == "__main__":
    print("steps", loop_steps())
    print("p = %.5f +- %.5f" % naive_probability())
    print("mfpt = %.4f +- %.4f (%d unfinished)" % naive_mfpt())
