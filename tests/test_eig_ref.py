"""The CPU references of the stability analysis (tests/eig_ref.py), checked against each other
without the code under test: the exact-solve Arnoldi twin against the dense reference, the
ordering contract, and the committed fixture tests/golden/eigs_natl8.npz that
tests/test_gpu_eigs.py measures the GPU against.

natl8 (N = 1536) at cf.synthetic_state, k = 6, m = 40, tol = 1e-8, sigma in {0, 0.02}: both twins
converge all six wanted eigenvalues (29 steps at sigma = 0, 34 at 0.02).

The bound on the exact twin's eigenvalues is first-order perturbation theory, not a measured
number: a Ritz pair of A = (J - sigma B)^-1 B with residual ||A x - theta x|| = est |theta| lies
within kappa est |theta| of an eigenvalue, kappa = 1 / |y^H x| the eigenvalue's condition number
from the dense left and right eigenvectors; the dense eigenvalue itself carries up to
kappa N u ||A||.  In lambda = sigma + 1 / theta, relative to |lambda - sigma|, that is
kappa (est + N u ||A|| / |theta|); twice that allows for the second-order terms.
"""
import numpy as np
import pytest

import eig_ref as er

U = 2.0 ** -53


@pytest.fixture(scope="module")
def cases(oracle_lib):
    sysd = er.system(oracle_lib)
    return sysd, [er.run_case(oracle_lib, s, sysd) for s in er.SIGMAS]


@pytest.fixture(scope="module")
def fixture():
    with np.load(er.FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_jacobian_null_space_is_the_pressure_modes(cases):
    """why the reference deflates: two null vectors, and B vanishes on them"""
    sysd, rs = cases
    assert [r["nnull"] for r in rs] == [2, 2]


@pytest.mark.parametrize("q", range(len(er.SIGMAS)))
def test_exact_twin_matches_dense(cases, q):
    import scipy.linalg as sla
    (c, o, L, x, val, B, diag), rs = cases
    r, sigma = rs[q], er.SIGMAS[q]
    ex = r["exact"]
    n = len(ex["lam"])
    print(f"sigma {sigma}: {ex['steps']} steps, estimates {ex['estimate']}, residuals {ex['residual']}")
    assert not ex["breakdown"] and ex["steps"] <= er.M
    assert n in (er.K, er.K + 1)
    assert np.all(ex["estimate"] <= er.TOL), "a wanted pair is unconverged at m = 40 with exact solves"
    # the condition numbers of the n eigenvalues nearest the shift
    Js = er.csr(o, er.shifted_val(val, B, diag, sigma)).toarray()
    A = er.deflated_inverse(Js)[0] * B[None, :]
    th, VL, VR = sla.eig(A, left=True, right=True)
    idx = np.argsort(-np.abs(th), kind="stable")[:n]
    kappa = 1.0 / np.abs(np.sum(np.conj(VL[:, idx]) * VR[:, idx], axis=0))
    lam_ref = sigma + 1.0 / th[idx]
    normA = np.linalg.norm(A, 2)
    hit = set()
    for i, lam in enumerate(ex["lam"]):
        d = np.abs(lam - lam_ref) / np.abs(lam_ref - sigma)
        p = int(np.argmin(d))
        bound = 2.0 * kappa[p] * (ex["estimate"][i] + o.N * U * normA / abs(th[idx][p]))
        print(f"  lambda {lam:.12g}: deviation {d[p]:.3e}, bound {bound:.3e} (kappa {kappa[p]:.2f})")
        assert d[p] <= bound
        hit.add(p)
    assert hit == set(range(n)), "the twin's eigenvalues are not the n nearest the shift"


@pytest.mark.parametrize("q", range(len(er.SIGMAS)))
@pytest.mark.parametrize("kind", ["exact", "inexact"])
def test_order_and_pairs(cases, q, kind):
    _, rs = cases
    lam, sigma = rs[q][kind]["lam"], er.SIGMAS[q]
    d = np.abs(lam - sigma)
    assert np.all(np.diff(d) >= -1e-12 * d[:-1])
    i = 0
    while i < len(lam):
        if lam[i].imag != 0:
            assert lam[i].imag > 0 and i + 1 < len(lam) and lam[i + 1] == np.conj(lam[i])
            i += 2
        else:
            i += 1


@pytest.mark.parametrize("q", range(len(er.SIGMAS)))
def test_inexact_twin_converges_all(cases, q):
    ix = cases[1][q]["inexact"]
    print(f"sigma {er.SIGMAS[q]}: {ix['steps']} steps, worst residual {ix['residual'].max():.3e}, "
          f"worst deviation {ix['deviation'].max():.3e}, inner steps {min(ix['iters'])}..{max(ix['iters'])}")
    assert np.all(ix["estimate"] <= er.TOL)
    assert ix["steps"] == cases[1][q]["exact"]["steps"]


@pytest.mark.parametrize("q", range(len(er.SIGMAS)))
def test_fixture_is_current(cases, fixture, q):
    """tests/golden/eigs_natl8.npz is what the twins give (python tests/eig_ref.py rewrites it)"""
    r = cases[1][q]
    assert list(fixture["sigmas"]) == list(er.SIGMAS)
    assert (int(fixture["k"]), int(fixture["m"]), float(fixture["tol"]), float(fixture["inner_tol"]),
            int(fixture["seed"])) == (er.K, er.M, er.TOL, er.INNER_TOL, er.SEED)
    for kind in ("exact", "inexact"):
        t = r[kind]
        assert int(fixture[f"s{q}_{kind}_steps"]) == t["steps"]
        want = fixture[f"s{q}_{kind}_lam"]
        assert want.shape == t["lam"].shape
        # the recorded digits against a rerun on another host's BLAS: far inside the GPU test's band
        assert np.all(np.abs(want - t["lam"]) <= 1e-10 * np.abs(want - er.SIGMAS[q]))
        for key, v in (("worst_residual", t["residual"].max()), ("worst_deviation", t["deviation"].max())):
            rec = float(fixture[f"s{q}_{kind}_{key}"])
            assert 0.5 * rec <= v <= 2.0 * rec, (key, rec, v)
