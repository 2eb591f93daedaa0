"""The rare-event drivers of iemic.rare_event on the host (no GPU).

1. exact bookkeeping on scripted trajectories and scripted donor choices: ties, the branch point,
   ell and the alpha product, the clean-up, extinction, the MFPT guard, the parameters, the loop
   count, the restart file;
2. the score-function builders against direct NumPy expressions;
3. the reference's double well (src/tests/test_ams.C) against independent naive estimates
   (tests/rare_ref.py): TAMS, naive Monte Carlo, GPA and the AMS mean first-passage time.

Measured on 2026-10-21 with the seeds below ("ams seed" = "noise seed" = 1 .. 8, N = 200):
TAMS mean 0.1587 (runs 0.132 .. 0.194), naive mean 0.1581, GPA mean 0.1196 with a standard
deviation of 0.0539 between the runs (standard error of the mean 0.0191; its outer loop covers 190
of the 199 steps); AMS (seed 1) MFPT 7.33 against 6.89 by naive first passage.  With the
reference's likelihood ratio taken literally GPA gave 0.062 (rare_event's departure 6).
"""
import logging
import math

import numpy as np
import pytest

import rare_ref as rr
from iemic import h5
from iemic.rare_event import (AMSExperiment, Transient, default_score_function, mem2string, ocean_score_function,
                              projected_default_score_function, projected_ocean_score_function)

SEEDS = range(1, 9)


# ---- 1. bookkeeping ---------------------------------------------------------------------------------
class Script:
    """Deterministic trajectories: launch L (a call whose argument is not the previous call's result:
    a start from x0 or from a stored snapshot) follows ``tables[L]``, one score per step, the last
    one repeated.  A state is (launch, steps since the launch, score)."""

    def __init__(self, tables):
        self.tables, self.launches, self._last = tables, 0, None

    def step(self, x, dt):
        if x is not self._last:
            launch, n = self.launches, 0
            self.launches += 1
        else:
            launch, n = int(x[0]), int(x[1])
        tab = self.tables[launch]
        self._last = np.array([launch, n + 1, tab[min(n, len(tab) - 1)]])
        return self._last

    @staticmethod
    def dist(x):
        return float(x[2])


X0 = np.array([-1.0, 0.0, 0.0])


def scripted(tables, picks, params):
    sc = Script(tables)
    tr = Transient(sc.step, sc.dist, X0, vector_length=3)
    tr.set_parameters(dict({"time step": 1.0, "maximum time": 5.0, "distance tolerance": 0.0005}, **params))
    it = iter(picks)
    tr.randint = lambda a, b: next(it)
    return tr, sc


TABLES = [[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.2, 0.4, 0.5, 0.6], [0.5, 0.96],      # the four initial ones
          [0.45, 0.97],        # experiment 1 from experiment 2's t = 2
          [0.5, 0.5, 0.55, 0.5],  # experiment 0 from experiment 3's t = 1
          [0.6],               # experiment 0 from experiment 2's t = 4
          [0.97],              # experiment 0 from experiment 3's t = 2
          [0.99]]              # experiment 2 from experiment 1's t = 4


def test_ties_branch_point_ell_and_alpha():
    tr, sc = scripted(TABLES, [0, 1, 0, 0, 1], {"number of experiments": 4, "method": "TAMS"})
    assert tr.run() == 0
    e = tr.experiments
    # experiments 0 and 1 tie at 0.3 and go together; then 0 alone at 0.55; then 0 and 2 tie at 0.6
    assert tr.ell == [2, 1, 2] and tr.its == 3 and not tr.extinct
    assert tr.probability == 4 / 4 * (1 - 2 / 4) * (1 - 1 / 4) * (1 - 2 / 4) == tr.get_probability()
    assert all(x.converged and x.max_distance == 1.0 for x in e)
    assert sc.launches == 9 and tr.time_steps == 15 + 2 + 2 + 4 + 1 + 1 + 1
    # experiment 1 took experiment 2's list up to the first entry >= 0.3 (0.4 at t = 2), then went on
    assert e[1].dlist == [0, 0.2, 0.4, 0.45, 1.0] and e[1].tlist == [0, 1.0, 2.0, 3.0, 4.0]
    assert [tuple(x[:2]) for x in e[1].xlist] == [(-1, 0), (2, 1), (2, 2), (4, 1), (4, 2)]
    # experiment 2 ended on experiment 1's whole list (first entry >= 0.6 is its last) and one step
    assert e[2].dlist == [0, 0.2, 0.4, 0.45, 1.0, 1.0] and e[2].tlist == [0, 1.0, 2.0, 3.0, 4.0, 5.0]
    assert e[0].dlist == [0, 0.5, 1.0, 1.0] and e[0].tlist == [0, 1.0, 2.0, 3.0]
    # tams: time is the last recorded time
    assert [x.time for x in e] == [3.0, 4.0, 5.0, 2.0]
    # snapshots are shared between donor and receiver, not re-copied, and are copies of the states
    assert e[2].xlist[1] is e[1].xlist[1]


def test_branch_keeps_the_eliminated_level_not_the_donor_maximum():
    """after a branch the running maximum is the eliminated experiment's own max_distance, as in
    transient_tams (:276): a score above it is recorded even when the donor's prefix ends higher"""
    tr, sc = scripted(TABLES, [0, 1, 0, 0, 1], {"number of experiments": 4, "method": "TAMS",
                                                "maximum iterations": 1})
    tr.run()
    e = tr.experiments
    assert tr.its == 1 and tr.ell == [2]
    assert e[0].dlist == [0, 0.5, 0.5, 0.55] and e[0].tlist == [0, 1.0, 2.0, 4.0] and e[0].max_distance == 0.55
    assert e[0].time == 4.0 and not e[0].converged
    assert tr.probability == 2 / 4 * (1 - 2 / 4)


def prepared(d, t=None):
    e = AMSExperiment(X0)
    e.dlist = list(d)
    e.tlist = list(range(len(d))) if t is None else list(t)
    e.xlist = [np.array([-2.0, j, v]) for j, v in enumerate(d)]
    e.max_distance = max(d)
    e.initialized = True
    return e


def test_cleanup_every_tenth_iteration_drops_the_prefix_below_the_global_minimum():
    for its0, cleaned in ((9, True), (8, False)):
        tr, sc = scripted([[0.35]], [0], {"number of experiments": 3, "maximum iterations": its0 + 1,
                                          "maximum time": 4.0, "write final state": False})
        exps = [prepared([0, 0.1, 0.2]), prepared([0, 0.15, 0.3, 0.5]), prepared([0, 0.25, 0.4, 0.7])]
        tr.its = its0
        alpha = tr.ams_elimination("TAMS", exps, tr.dt, tr.tmax)
        assert tr.its == its0 + 1 and tr.ell == [1] and alpha == 0.0
        if cleaned:       # the global minimum is now 0.35
            assert [x.dlist for x in exps] == [[0.35], [0.5], [0.4, 0.7]]
            assert [x.tlist for x in exps] == [[3], [3], [2, 3]]
            assert [[v[2] for v in x.xlist] for x in exps] == [[0.35], [0.5], [0.4, 0.7]]
        else:
            assert [x.dlist for x in exps] == [[0, 0.15, 0.3, 0.35], [0, 0.15, 0.3, 0.5], [0, 0.25, 0.4, 0.7]]


def test_extinction_ends_the_loop(caplog):
    tr, sc = scripted([[0.1, 0.2], [0.1, 0.2], [0.1, 0.2]], [], {"number of experiments": 3, "method": "TAMS"})
    with caplog.at_level(logging.WARNING, logger="iemic.rare_event"):
        tr.run()
    assert tr.extinct and tr.its == 0 and tr.ell == [] and tr.probability == 0.0
    assert tr.time_steps == 15 and "extinct" in caplog.text
    # not extinct, and the loop ends, once all have converged
    tr, sc = scripted([[0.96]] * 2, [], {"number of experiments": 2, "method": "TAMS"})
    tr.run()
    assert not tr.extinct and tr.probability == 1.0 and tr.its == 0


def test_mfpt_guard(caplog):
    # every experiment leaves C (0.2 > 0.1) and returns to A (0.01 < 0.05); none reaches B
    tr, sc = scripted([[0.2], [0.01]] * 3, [], {"number of experiments": 3, "method": "AMS", "maximum iterations": 0})
    with caplog.at_level(logging.WARNING, logger="iemic.rare_event"):
        tr.run()
    assert math.isnan(tr.mfpt) and tr.probability == -1.0 and "undefined" in caplog.text
    assert [x.initial_time for x in tr.experiments] == [1.0] * 3
    assert [x.return_time for x in tr.experiments] == [1.0] * 3      # tlist restarts at 0 after the start
    # every experiment reaches B and none returns: num_t2 == 0
    tr, sc = scripted([[0.2], [0.96]] * 2, [], {"number of experiments": 2, "method": "AMS"})
    tr.run()
    assert math.isnan(tr.get_mfpt()) and tr.get_probability() == -1.0 and tr.alpha == 1.0


def test_ams_mfpt_formula():
    """two experiments: one returns to A at t = 2 after leaving C at t = 1, one reaches B at t = 3
    after leaving C at t = 2; no iterations"""
    tr, sc = scripted([[0.2], [0.3, 0.01], [0.01, 0.2], [0.5, 0.6, 0.96]], [],
                      {"number of experiments": 2, "method": "AMS", "maximum iterations": 0})
    tr.run()
    a, b = tr.experiments
    assert (a.initial_time, a.return_time, a.time, a.converged) == (1.0, 2.0, 2.0, False)
    assert (b.initial_time, b.return_time, b.time, b.converged) == (2.0, 0.0, 3.0, True)
    alpha = 1 / 2
    want = (1 / alpha - 1) * (3.0 / 2 + 2.0 / 1) + 3.0 / 2 + 5.0 / 1
    assert tr.alpha == alpha and tr.mfpt == want
    assert tr.probability == 1.0 - math.exp(-1.0 / want * 5.0)


def test_parameters():
    tr = Transient(lambda x, dt: x)
    assert tr.method == "Transient"
    tr = Transient(lambda x, dt: x, lambda x: 0.0)
    assert tr.method == "TAMS"
    assert (tr.dt, tr.tmax, tr.tstep, tr.beta, tr.bdist, tr.dist_tol, tr.num_exp, tr.adist, tr.cdist,
            tr.num_init_exp, tr.maxit) == (0.01, 1000.0, 1.0, 1.0, 0.05, 0.0005, 1000, 0.05, 0.1, 1000, 10000)
    assert (tr.read_file, tr.write_file, tr.write_final, tr.write_steps, tr.write_time_steps) == ("", "", True, -1, -1)
    tr.set_parameters({"number of experiments": 50, "number of initial experiments": 20, "A distance": 0.1})
    assert tr.num_init_exp == 50 and tr.maxit == 500 and tr.cdist == 0.2
    tr.set_parameters({"number of experiments": 50, "number of initial experiments": 70})
    assert tr.num_init_exp == 70
    in_years = 737.2685 / 365.
    tr.set_parameters({"time step (in y)": 0.5, "maximum time (in y)": 10.0, "time step": 7.0})
    assert tr.dt == 0.5 / in_years and tr.tmax == 10.0 / in_years
    tr.set_parameters({"timescale in years": 2.0, "time step (in y)": 0.5, "maximum time": 3.0})
    assert tr.dt == 0.25 and tr.tmax == 3.0 * 2.0 / 2.0
    tr.set_parameters({"timescale in days": 730.0, "maximum time (in y)": 4.0})
    assert tr.tmax == 2.0 and tr.dt == 0.01 * 2.0 / 2.0
    tr.set_parameters({"method": "nonsense"})
    assert tr.run(X0) == -1
    assert mem2string(999) == "999.00 B" and mem2string(1.5e6) == "1.50 MB" and mem2string(3.2e13) == "32.00 TB"


def test_the_time_loop_takes_199_steps():
    calls = []
    tr = Transient(lambda x, dt: calls.append(dt) or x, lambda x: 0.0, X0)
    tr.set_parameters({"time step": 0.01, "maximum time": 2.0, "method": "Transient"})
    tr.run()
    assert len(calls) == tr.time_steps == 199 == rr.loop_steps() and set(calls) == {0.01}
    tr.set_parameters({"time step": 0.01, "maximum time": 2.0, "method": "Naive", "number of experiments": 3})
    tr.run()
    assert tr.time_steps == 199 * 4 and tr.probability == 0.0


def test_random_numbers_are_philox_keyed_by_the_seed():
    a, b = Transient(None), Transient(None)
    a.set_random_engine(7)
    b.set_random_engine(7)
    ia = [a.randint(0, 9) for _ in range(200)]
    assert ia == [b.randint(0, 9) for _ in range(200)] and set(ia) == set(range(10))
    ra = [a.randreal(0.0, 3.5) for _ in range(200)]
    assert all(0.0 <= v < 3.5 for v in ra) and len({int(v) == v for v in ra}) == 1 and not float(ra[0]).is_integer()
    assert a.randint(4, 4) == 4
    c = Transient(None)
    c.set_random_engine(0)
    assert c.ams_seed != 0
    want = np.random.Generator(np.random.Philox(key=7))
    assert ia[0] == int(want.integers(0, 10))


# ---- the restart file -----------------------------------------------------------------------------------
def well(method, seed, **kw):
    step = rr.DoubleWell(seed)
    tr = Transient(step, default_score_function(None, rr.SOL1, rr.SOL2, rr.SOL3), rr.SOL1.copy(), vector_length=2)
    tr.stepper = step
    tr.set_parameters(dict({"time step": rr.DT, "maximum time": rr.TMAX, "B distance": rr.BDIST, "method": method,
                            "number of experiments": 200, "maximum iterations": 10000}, **kw))
    tr.set_random_engine(seed)
    return tr


def same_experiments(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for f in ("max_distance", "time", "initial_time", "return_time", "initialized", "converged"):
            assert getattr(x, f) == getattr(y, f), f
        assert x.dlist == y.dlist and x.tlist == y.tlist and len(x.xlist) == len(y.xlist)
        assert all(np.array_equal(p, q) for p, q in zip(x.xlist, y.xlist))


@pytest.mark.parametrize("method", ["TAMS", "AMS"])
def test_write_read_resume(tmp_path, caplog, method):
    name = str(tmp_path / "out_data.h5")
    one = well(method, 42, **{"number of experiments": 20, "maximum iterations": 10, "write file": name})
    one.run()
    assert one.its == 10 and len(one.ell) == 10
    t = h5.read(name)
    assert int(t["/data/its"][0]) == 10 and int(t["/data/num exp"][0]) == 20 and int(t["/data/ell size"][0]) == 10
    assert int(t["/data/noise draws"][0]) == one.stepper.draws == one.time_steps == int(t["/data/time steps"][0])
    assert t["/experiments/3/xlist/0/Values"][0].shape == (1, 2) and int(t["/experiments/3/xlist/0/NumVectors"][0]) == 1
    assert t["/experiments/3/dlist"][0].dtype == np.float64 and t["/data/ell"][0].dtype == np.int32
    # a round trip gives the experiments back field by field
    back = well(method, 42, **{"number of experiments": 20})
    exps = [AMSExperiment(rr.SOL1) for _ in range(20)]
    back.read(name, exps)
    same_experiments(exps, one.experiments)
    assert back.its == 10 and back.ell == one.ell and back.time_steps == one.time_steps
    assert back.stepper.draws == one.stepper.draws
    # resumed with the same limit nothing is left to do; with a larger one the count goes on from 10
    for maxit in (10, 14):
        two = well(method, 43, **{"number of experiments": 20, "maximum iterations": maxit, "read file": name})
        with caplog.at_level(logging.INFO, logger="iemic.rare_event"):
            caplog.clear()
            two.run()
        assert "Initialization" not in caplog.text and f"{method}: {maxit + 1} /" not in caplog.text
        assert two.its == maxit and two.ell[:10] == one.ell and len(two.ell) == maxit
        assert (f"{method}: 11 / 14" in caplog.text) == (maxit == 14)
        assert two.time_steps >= one.time_steps and two.stepper.draws == two.time_steps
    # the refusals are errors
    with pytest.raises(ValueError, match="Number of experiments is 30 instead of 20"):
        well(method, 1, **{"number of experiments": 30, "read file": name}).run()
    bad = well(method, 1, **{"number of experiments": 20})
    bad.vector_length = 3
    with pytest.raises(ValueError, match="has 2 entries, the model's states have 3"):
        bad.read(name, [AMSExperiment(rr.SOL1) for _ in range(20)])


def test_write_helper_schedule(tmp_path):
    name = str(tmp_path / "w.h5")
    tr = well("TAMS", 3, **{"number of experiments": 4, "write file": name, "write steps": 3,
                            "write final state": False})
    written = []
    tr.write = lambda n, e: written.append((n, tr.time_steps))
    exps = [AMSExperiment()]
    for its in range(1, 8):
        tr.time_steps += 100
        tr.write_helper(exps, its)
    assert [w[1] for w in written] == [300, 600] and tr.time_steps_previous_write == 600
    tr.set_parameters({"write file": name, "write time steps": 250})
    written.clear()
    tr.time_steps = tr.time_steps_previous_write = 0
    for its in range(1, 8):
        tr.time_steps += 100
        tr.write_helper(exps, its)
    assert [w[1] for w in written] == [300, 600]
    tr.set_parameters({"write time steps": 250})                # no file: nothing
    written.clear()
    tr.write_helper(exps, 3)
    assert not written


def test_restart_file_with_hundreds_of_experiments(tmp_path):
    """more members than one symbol node holds (128): "experiments" with 300 children and an "xlist"
    with 150; past 4096 the writer refuses by name"""
    name = str(tmp_path / "many.h5")
    tr = well("TAMS", 1, **{"number of experiments": 300})
    exps = []
    for i in range(300):
        e = prepared([0.001 * j + i for j in range(150 if i == 7 else 2)])
        e.xlist = [np.array([float(i), float(j)]) for j in range(len(e.dlist))]
        exps.append(e)
    tr.write(name, exps)
    back = [AMSExperiment() for _ in range(300)]
    tr.read(name, back)
    same_experiments(back, exps)
    with pytest.raises(h5.H5Error, match="more than 4096 members"):
        h5.write(str(tmp_path / "big.h5"), {"g": {str(i): np.array(i) for i in range(4097)}})
    # up to 128 members the bytes are what they were: one symbol node under the node
    h5.write(name, {"g": {str(i): np.array(i) for i in range(128)}})
    raw = open(name, "rb").read()
    assert raw.count(b"SNOD") == 2 and raw.count(b"TREE") == 2


# ---- 2. score functions -----------------------------------------------------------------------------------
def direct(d1, d2, f):
    return f - f * math.exp(-0.5 * (d1 / 0.25) ** 2) + (1 - f) * math.exp(-0.5 * (d2 / 0.25) ** 2)


def test_score_functions_against_numpy():
    rng = np.random.default_rng(5)
    N, k = 6 * 20, 4
    s1, s2, s3, x = rng.standard_normal((4, N))
    for build, rows in ((default_score_function, slice(None)), (ocean_score_function, slice(1, None, 6))):
        for third in (s3, None):
            fn = build(None, s1, s2, third)
            nrm = np.linalg.norm((s1 - s2)[rows])
            f = 0.5 if third is None else np.linalg.norm((s1 - s3)[rows]) / nrm
            assert fn.nrm == nrm and fn.dist_factor == f
            want = direct(np.linalg.norm((x - s1)[rows]) / nrm, np.linalg.norm((x - s2)[rows]) / nrm, f)
            assert abs(fn(x) - want) <= 4 * np.finfo(float).eps
            assert fn(s1) == direct(0.0, 1.0, f) and abs(fn(s2) - direct(1.0, 0.0, f)) < 1e-15
    # the ocean score ignores every other variable
    fn = ocean_score_function(None, s1, s2, s3)
    y = x + 1.0
    y[1::6] = x[1::6]
    assert fn(y) == fn(x) and default_score_function(None, s1, s2, s3)(y) != default_score_function(None, s1, s2, s3)(x)
    # projected: V is not orthonormal, so the norm is sqrt(y^T V^T V y) = ||V y||, not ||y||
    V = rng.standard_normal((N, k)) * np.array([1.0, 3.0, 0.5, 2.0])
    V[:, 1] += 0.5 * V[:, 0]
    y1, y2, y3, y = rng.standard_normal((4, k))
    D = np.zeros(N)
    D[1::6] = 1.0
    for build, M, full in ((projected_default_score_function, V.T @ V, lambda z: np.linalg.norm(V @ z)),
                           (projected_ocean_score_function, V.T @ (D[:, None] * V), lambda z: np.linalg.norm((V @ z)[1::6]))):
        for third in (y3, None):
            fn = build(y1, y2, third, M)
            nrm = full(y1 - y2)
            f = 0.5 if third is None else full(y1 - y3) / nrm
            assert abs(fn.nrm - nrm) <= 1e-13 * nrm and abs(fn.dist_factor - f) <= 1e-13
            want = direct(full(y - y1) / nrm, full(y - y2) / nrm, f)
            assert abs(fn(y) - want) <= 1e-12
            plain = direct(np.linalg.norm(y - y1) / np.linalg.norm(y1 - y2), np.linalg.norm(y - y2) / np.linalg.norm(y1 - y2), f)
            assert abs(fn(y) - plain) > 1e-3
    with pytest.raises(ValueError, match="must be positive"):
        default_score_function(None, s1, s1, s3)
    with pytest.raises(ValueError, match="Gram matrix has shape"):
        projected_default_score_function(y1, y2, y3, np.eye(k + 1))


# ---- 3. the double well ---------------------------------------------------------------------------------------
def test_the_step_function_is_the_vectorised_process():
    step = rr.DoubleWell(9)
    x = rr.SOL1.copy()
    xi = np.random.Generator(np.random.Philox(key=9, counter=[0, 0, 0, 0])).standard_normal((4096, 2))
    for b in range(5):
        want = rr.euler(x[None, :], xi[b][None, :])[0]
        x = step(x, rr.DT)
        assert np.allclose(x, want, rtol=0, atol=1e-15)
    fn = default_score_function(None, rr.SOL1, rr.SOL2, rr.SOL3)
    assert abs(fn(x) - rr.scores(x[None, :])[0]) <= 1e-15 and fn.dist_factor == 0.5


@pytest.mark.slow
def test_tams_probability():
    """one run with N = 200 has a standard deviation of about p sqrt(-ln p / N) = 0.015, the mean of
    eight about 0.0053: within 0.02 of the naive estimate"""
    runs = []
    for s in SEEDS:
        tr = well("TAMS", s)
        tr.run()
        assert not tr.extinct and all(e.converged for e in tr.experiments)
        runs.append(tr.probability)
    print("TAMS", np.round(runs, 4), "mean", np.mean(runs))
    assert abs(np.mean(runs) - rr.P_REF) <= 0.02


def test_naive_probability():
    """8 x 200 trajectories: within 4 sqrt(p (1 - p) / 1600) = 0.036"""
    runs = []
    for s in SEEDS:
        tr = well("Naive", s)
        tr.run()
        assert tr.time_steps == 200 * 199
        runs.append(tr.probability)
    print("naive", np.round(runs, 4), "mean", np.mean(runs))
    assert abs(np.mean(runs) - rr.P_REF) <= 0.036


@pytest.mark.slow
def test_gpa_probability():
    """beta = 1, GPA time step 0.1: the mean of the eight runs within four of its standard errors
    (measured from the runs themselves), capped at 0.04"""
    runs = []
    for s in SEEDS:
        tr = well("GPA", s, **{"beta": 1.0, "GPA time step": 0.1})
        tr.run()
        runs.append(tr.probability)
    se = np.std(runs, ddof=1) / math.sqrt(len(runs))
    print("GPA", np.round(runs, 4), "mean", np.mean(runs), "std", np.std(runs, ddof=1), "se", se)
    assert abs(np.mean(runs) - rr.P_REF) <= min(4 * se, 0.04)


@pytest.mark.slow
def test_ams_mean_first_passage_time():
    """N = 200: within 25 % of the naive first-passage estimate (the reference's own tests expect
    7 +- 1 and 6.3 +- 1 for the same process)"""
    tr = well("AMS", 1)
    tr.run()
    print("AMS mfpt", tr.mfpt, "naive", rr.MFPT_REF, "alpha", tr.alpha, "its", tr.its)
    assert abs(tr.mfpt - rr.MFPT_REF) <= 0.25 * rr.MFPT_REF
    assert tr.probability == 1.0 - math.exp(-tr.tmax / tr.mfpt) or abs(tr.probability - (1.0 - math.exp(-tr.tmax / tr.mfpt))) < 1e-15
