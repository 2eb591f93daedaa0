"""The projected theta steppers' logic (iemic.transient.ProjectedThetaStepper,
StochasticProjectedThetaStepper, load_space) without a GPU.

* the two stepper classes on a scripted model: the order of setState / initStep / Newton / restore,
  a rejected step drawing again, unknown parameters refused;
* the NumPy twin's own consistency (tests/proj_ref.py): with k = N and V = I the projected Newton
  iteration is the full theta model's of test_transient.py (off the pressure null space);
* load_space: a round trip through a Matrix Market array file, and the refusals by name.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from iemic.transient import (ProjectedThetaStepper, StochasticProjectedThetaStepper, StochasticThetaStepper,
                             load_space)
from proj_ref import ProjectedTwin, gram
from test_transient import PARAMS, TwinModel, transient_config


class Scripted:
    """Converges in the first Newton iteration unless `fail` steps are still to be rejected."""

    cfg = SimpleNamespace(m=8)

    def __init__(self, fail=0):
        self.calls = []
        self.fail = fail
        self.y = np.zeros(3)

    def preProcess(self):
        self.calls.append("pre")

    def projSetBasis(self, V):
        self.calls.append(("basis", V.shape))

    def projRestrictState(self):
        return np.array([1.0, 2.0, 2.0])

    def projSetState(self, y):
        self.calls.append(("set", tuple(y)))
        self.y = np.array(y)

    def projInitStep(self, dt, theta):
        self.calls.append(("init", dt, theta))

    def projStochasticInitStep(self, dt, theta, sigma, pert):
        self.calls.append(("sinit", dt, theta, sigma, tuple(pert)))

    def projNewtonStep(self):
        self.calls.append("newton")
        if self.fail > 0:
            self.fail -= 1
            return SimpleNamespace(norm_dx=1e3, norm_f1=1.0)
        self.y = self.y + 1.0
        return SimpleNamespace(norm_dx=1e-9, norm_f1=1e-9)

    def projRestore(self):
        self.calls.append("restore")

    def projGet(self, what):
        assert what == "y"
        return self.y


V3 = np.eye(5, 3)


def test_step_and_restore_order():
    m = Scripted(fail=1)
    st = ProjectedThetaStepper(m, V3, dict(PARAMS, **{"number of time steps": 2}))
    assert m.calls == [("basis", (5, 3))] and np.array_equal(st.y, [1.0, 2.0, 2.0])
    assert st.run() == 0
    y0, y1 = (1.0, 2.0, 2.0), (2.0, 3.0, 3.0)
    assert m.calls[1:] == ["pre", ("set", y0), ("init", 1e-3, 0.75), "newton", "restore",
                           "pre", ("set", y0), ("init", 5e-4, 0.75), "newton",
                           "pre", ("set", y1), ("init", 1e-3, 0.75), "newton"]
    assert st.rejected == [1e-3] and [r.dt for r in st.history] == [5e-4, 1e-3]
    # the history's norm_x is ||y||_2
    assert st.history[0].norm_x == np.linalg.norm(y1) and st.history[1].norm_x == np.linalg.norm([3.0, 4.0, 4.0])


def test_step_function():
    m = Scripted()
    st = ProjectedThetaStepper(m, V3, PARAMS)
    y = st.step([0.5, 0.5, 0.5], 0.25)
    assert np.array_equal(y, [1.5, 1.5, 1.5]) and st.converged and st.newton_steps == 0
    assert m.calls[1:] == [("set", (0.5, 0.5, 0.5)), ("init", 0.25, 0.75), "newton"]
    with pytest.raises(ValueError, match="y has 2 entries"):
        st.step([1.0, 2.0], 0.25)


def test_rejected_step_draws_again():
    m = Scripted(fail=1)
    blocks = []

    def source(block, mm):
        blocks.append(block)
        return np.full(mm, float(block))

    st = StochasticProjectedThetaStepper(m, V3, dict(PARAMS, **{"sigma": 0.5, "number of time steps": 2}),
                                         pert_source=source)
    assert st.run() == 0
    inits = [c for c in m.calls if isinstance(c, tuple) and c[0] == "sinit"]
    assert [(c[1], c[3], c[4][0]) for c in inits] == [(1e-3, 0.5, 0.0), (5e-4, 0.5, 1.0), (1e-3, 0.5, 2.0)]
    assert blocks == [0, 1, 2] and st.draws == 3 and st.rejected == [1e-3]
    assert "restore" in m.calls and not any(isinstance(c, tuple) and c[0] == "init" for c in m.calls)


def test_philox_blocks_are_the_full_steppers():
    m = Scripted()
    st = StochasticProjectedThetaStepper(m, V3, dict(PARAMS, **{"noise seed": 11, "number of time steps": 1}))
    assert st.run() == 0 and st.noise_seed == 11
    sinit = [c for c in m.calls if isinstance(c, tuple) and c[0] == "sinit"][0]
    assert np.array_equal(sinit[4], StochasticThetaStepper.noise_block(11, 0, 8))


def test_unknown_parameters_and_bad_bases_refused():
    with pytest.raises(KeyError, match="unknown parameter 'sigma'"):
        ProjectedThetaStepper(Scripted(), V3, dict(PARAMS, sigma=1.0))
    with pytest.raises(KeyError, match="unknown parameter 'space dimension'"):
        StochasticProjectedThetaStepper(Scripted(), V3, dict(PARAMS, **{"space dimension": 3}))
    with pytest.raises(ValueError, match='"theta"'):
        ProjectedThetaStepper(Scripted(), V3, dict(PARAMS, theta=0.0))
    with pytest.raises(ValueError, match='"sigma"'):
        StochasticProjectedThetaStepper(Scripted(), V3, dict(PARAMS, sigma=-1.0))
    with pytest.raises(ValueError, match="N x k"):
        ProjectedThetaStepper(Scripted(), np.zeros(5), PARAMS)


def test_exact_gram():
    rng = np.random.default_rng(3)
    V, W, d = rng.standard_normal((200, 3)), rng.standard_normal((200, 2)), rng.standard_normal(200)
    G, A = gram(V, W, d)
    assert G.shape == (3, 2) and np.all(np.abs(G - (V * d[:, None]).T @ W) <= 200 * 2.0 ** -52 * A)
    assert np.all(A >= np.abs(G))


def test_identity_basis_is_the_full_theta_step(oracle_lib):
    """k = N, V = I: y = x, VMV = B, VAV = J2, so the projected Newton iteration is ThetaModel's: the
    first iteration from rest on test_oceantransient.xml's model against test_transient.py's
    TwinModel at linear tolerance 1e-10.  (Later iterations differ by design: the projected model
    keeps the Jacobian of the init step, ProjectedThetaModel::computeJacobian being empty, where
    ThetaModel assembles a new one.)  J2 has the two constant-pressure null vectors that the full
    model's preconditioner pins, so a dense solve needs them out of the basis: the identity column
    of the largest entry of each null vector is dropped, which pins that pressure to zero and
    leaves every other unknown of the step as it is.  The solve is the twin's own
    numpy.linalg.solve.  The P rows, defined up to the null vectors, are left out of the comparison;
    the others agree within 100 times the linear tolerance of ||dx||."""
    c = transient_config()
    m = ProjectedTwin(oracle_lib, c, exact=False)
    N = m.o.N
    m.projSetBasis(np.eye(N))
    m.projInitStep(1e-3, 0.75)
    assert np.array_equal(m.VMV, np.diag(m.B))
    _, sv, vt = np.linalg.svd(m.VAV)
    assert sv[-2] < 1e-12 * sv[0] < 1e-6 * sv[0] < sv[-3]          # exactly two null vectors
    drop = []
    for v in vt[-2:]:
        assert np.all(np.abs(v[np.arange(N) % 6 != 3]) < 1e-10)    # pressure only
        drop.append(next(int(i) for i in np.argsort(-np.abs(v)) if i not in drop))
    keepcols = np.setdiff1d(np.arange(N), drop)
    st = ProjectedThetaStepper(m, np.eye(N)[:, keepcols], PARAMS)
    assert st.k == N - 2
    m.projSetState(np.zeros(N - 2))
    m.projInitStep(1e-3, 0.75)
    assert np.linalg.cond(m.VAV) < 1e12
    a = m.projNewtonStep()
    t = TwinModel(oracle_lib, c, lin_tol=1e-10)
    t.thetaInitStep(1e-3, 0.75)
    b = t.thetaNewtonStep()
    keep = np.arange(N) % 6 != 3
    gap = np.abs(m.x - t.x)[keep].max()
    print(f"dropped columns {drop}; |dx| off P {np.abs(m.x)[keep].max():.6e} / {np.abs(t.x)[keep].max():.6e}  "
          f"|F| {a.norm_f1:.6e} / {b.norm_f1:.6e}  gap off the P rows {gap:.2e}")
    assert np.array_equal(m.x[keepcols], m.y) and not m.x[drop].any()
    assert gap <= 1e-8 * b.norm_dx
    assert abs(a.norm_f1 - b.norm_f1) <= 1e-6 * b.norm_f1


def write_mm(path, V, header="%%MatrixMarket matrix array real general"):
    with open(path, "w") as f:
        f.write(header + "\n% a comment\n")
        f.write(f"{V.shape[0]} {V.shape[1]}\n")
        for v in V.T.reshape(-1):
            f.write(f"{float(v)!r}\n")


def test_load_space_round_trip(tmp_path):
    V = np.random.default_rng(5).standard_normal((12, 3))
    p = str(tmp_path / "space.mtx")
    write_mm(p, V)
    got = load_space(p, nrows=12)
    assert got.shape == (12, 3) and got.flags["C_CONTIGUOUS"] and np.array_equal(got, V)
    assert np.array_equal(load_space(p), V)


def test_load_space_refusals(tmp_path):
    V = np.arange(12.0).reshape(4, 3)
    p = str(tmp_path / "space.mtx")
    write_mm(p, V, "%%MatrixMarket matrix coordinate real general")
    with pytest.raises(ValueError, match='"coordinate" format'):
        load_space(p)
    write_mm(p, V, "%%MatrixMarket matrix array complex general")
    with pytest.raises(ValueError, match='"complex general"'):
        load_space(p)
    write_mm(p, V, "%%MatrixMarket matrix array real symmetric")
    with pytest.raises(ValueError, match='"real symmetric"'):
        load_space(p)
    write_mm(p, V, "not a header at all")
    with pytest.raises(ValueError, match="not a Matrix Market"):
        load_space(p)
    write_mm(p, V)
    with pytest.raises(ValueError, match="has 4 rows, the model has 6"):
        load_space(p, nrows=6)
    with open(p, "a") as f:
        f.write("1.0\n")
    with pytest.raises(ValueError, match="holds 13 values.*4 x 3"):
        load_space(p)
    with open(p, "w") as f:
        f.write("%%MatrixMarket matrix array real general\n4 3 7\n")
    with pytest.raises(ValueError, match="size line"):
        load_space(p)
    write_mm(p, np.zeros((2, 65)))
    with pytest.raises(ValueError, match="65 columns"):
        load_space(p)
