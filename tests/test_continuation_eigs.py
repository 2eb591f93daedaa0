"""The continuation driver's eigen-solver hook (iemic.continuation; Continuation.H:278-280,
:912-914, :1097-1131) on the analytic model of tests/test_continuation.py: with
"eigenvalue analysis" = 'P' the solver runs once per accepted step, between createTangent and
postProcess, and its result is in that step's StepRecord; with 'E' once per reached destination;
with 'N' never, and the history equals a run without the attribute."""
import numpy as np
import pytest

from iemic.continuation import Continuation
from test_continuation import ToyModel

PARAMS = {"destination 0": 2.0, "initial step size": 0.05, "maximum number of steps": 500,
          "destination tolerance": 1e-9, "Newton tolerance": 1e-10}


class Model(ToyModel):
    """x^3 + x = lam, logging the calls that neighbour the eigen-solver"""

    def __init__(self, log):
        super().__init__(lambda x, l: x ** 3 + x - l, lambda x, l: np.diag(3 * x ** 2 + 1), 2)
        self.log = log

    def preProcess(self):
        self.log.append("pre")

    def postProcess(self):
        self.log.append("post")


class Stub:
    def __init__(self, model, log):
        self.model, self.log, self.calls = model, log, 0

    def solve(self):
        self.calls += 1
        self.log.append("eig")
        return ("eig", self.calls, self.model.lam)


def run(mode, solver=True, **extra):
    log = []
    m = Model(log)
    cont = Continuation(m, dict(PARAMS, **({"eigenvalue analysis": mode} if mode else {}), **extra))
    stub = Stub(m, log)
    if solver:
        cont.eigen_solver = stub
    assert cont.run() == 0
    return cont, stub, log


def test_every_converged_point():
    cont, stub, log = run("P")
    assert len(cont.history) > 3
    assert stub.calls == len(cont.history)
    for q, rec in enumerate(cont.history):
        assert rec.eig == ("eig", q + 1, rec.par)
    # the reference's neighbours: after the corrector's createTangent, before postProcess; a
    # rejected step (preProcess without postProcess) does not reach the solver
    s = "".join({"pre": "a", "eig": "e", "post": "z"}[w] for w in log)
    assert s.count("ez") == stub.calls and s.count("e") == stub.calls
    assert "ae" in s and "az" not in s


def test_every_destination():
    cont, stub, log = run("E", **{"destination 0": 1.0, "destination 1": 2.0})
    assert stub.calls == 2
    got = [rec for rec in cont.history if rec.eig is not None]
    assert len(got) == 2
    assert [abs(rec.eig[2] - d) < 1e-9 for rec, d in zip(got, (1.0, 2.0))] == [True, True]


def test_none_changes_nothing():
    base, _, _ = run(None, solver=False)
    cont, stub, log = run("N")
    assert stub.calls == 0 and "eig" not in log
    assert cont.history == base.history
    assert all(rec.eig is None for rec in cont.history)


def test_solver_not_set_warns_and_unknown_mode_is_refused():
    with pytest.warns(UserWarning, match="eigen solver not set"):
        cont, _, _ = run("P", solver=False)
    assert all(rec.eig is None for rec in cont.history)
    with pytest.raises(ValueError, match="eigenvalue analysis"):
        Continuation(Model([]), dict(PARAMS, **{"eigenvalue analysis": "X"}))
