"""The CPU reference of the thick-restarted stability analysis (tests/eig_restart_ref.py), checked
without the code under test: at m_small the unrestarted exact twin is a dead end, the restarted
twins (exact and inexact solves) converge the same six eigenvalues the unrestarted m = 40 run
finds, and the committed fixture tests/golden/eigs_restart_natl8.npz is what they give."""
import numpy as np
import pytest

import eig_ref as er
import eig_restart_ref as err


@pytest.fixture(scope="module")
def made(oracle_lib):
    return err.make_fixture(oracle_lib)


@pytest.fixture(scope="module")
def fixture():
    with np.load(err.FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def base():
    with np.load(er.FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("q", range(len(er.SIGMAS)))
def test_restarted_twins_find_the_unrestarted_eigenvalues(made, base, q):
    m = int(made[f"s{q}_m_small"])
    assert m % 2 == 0 and er.K + 4 <= m and 2 * m <= int(base[f"s{q}_exact_steps"])
    assert made[f"s{q}_unrestarted_worst_estimate"] > er.TOL
    want = base[f"s{q}_exact_lam"]
    for kind in ("exact", "inexact"):
        lam = made[f"s{q}_{kind}_lam"]
        print(f"sigma {er.SIGMAS[q]} {kind}: m {m}, {made[f's{q}_{kind}_steps']} solves, "
              f"{made[f's{q}_{kind}_restarts']} restarts, worst deviation {made[f's{q}_{kind}_worst_deviation']:.3e}, "
              f"worst residual {made[f's{q}_{kind}_worst_residual']:.3e}")
        assert lam.shape == want.shape and made[f"s{q}_{kind}_restarts"] >= 1
        # both runs stop on estimates <= tol: each is within its own recorded deviation of the dense reference
        both = float(base[f"s{q}_exact_worst_deviation"]) + made[f"s{q}_{kind}_worst_deviation"]
        assert np.all(np.abs(lam - want) <= both * np.abs(want - er.SIGMAS[q]))
    assert made[f"s{q}_R"] == 2 * made[f"s{q}_inexact_restarts"]


@pytest.mark.parametrize("q", range(len(er.SIGMAS)))
def test_fixture_is_current(made, fixture, q):
    """python tests/eig_restart_ref.py rewrites it"""
    assert (int(fixture["k"]), float(fixture["tol"]), float(fixture["inner_tol"]), int(fixture["seed"])) == \
        (er.K, er.TOL, er.INNER_TOL, er.SEED)
    assert int(fixture[f"s{q}_m_small"]) == made[f"s{q}_m_small"] and int(fixture[f"s{q}_R"]) == made[f"s{q}_R"]
    for kind in ("exact", "inexact"):
        for key in ("steps", "restarts"):
            assert int(fixture[f"s{q}_{kind}_{key}"]) == made[f"s{q}_{kind}_{key}"]
        want = fixture[f"s{q}_{kind}_lam"]
        assert np.all(np.abs(want - made[f"s{q}_{kind}_lam"]) <= 1e-10 * np.abs(want - er.SIGMAS[q]))
        for key in ("worst_residual", "worst_deviation"):
            rec = float(fixture[f"s{q}_{kind}_{key}"])
            assert 0.5 * rec <= made[f"s{q}_{kind}_{key}"] <= 2.0 * rec, (key, rec)
