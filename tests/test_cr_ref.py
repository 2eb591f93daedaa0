"""The CPU references of tests/cr_ref.py against each other, and the conditions the GPU tests
(tests/test_gpu_dense.py) put on their manufactured inputs: every case has err_ref <= 1e-11
and, for the solves, a solution whose entries are all of size 1 -- so the relative bound of
the GPU tests cannot hide a wrong block."""
import numpy as np
import pytest

import cr_ref as R

ERR_REF_MAX = 1e-11


@pytest.mark.parametrize("periodic", [0, 1])
@pytest.mark.parametrize("n", sorted({c[0] for c in R.CR_CASES}))
def test_cr_ref_agrees_with_refined_solve(n, periodic):
    """the plain cyclic reduction reproduces the refined sparse-LU solution at a small m, for
    every block count of the GPU table (merge, odd counts with the wrap coupling, n = 1)"""
    m = 4
    D, L, Rb, A, b, xs, err = R.cr_system(n, m, periodic, seed=5)
    assert err <= 8 * m * R.EPS, err
    # and the reference notices a coupling: dropping one block moves the answer at first order
    if n > 2:
        L2 = np.array(L)
        L2[n // 2] = 0.0
        x2 = R.cr_ref(D, L2, Rb, np.asarray(b).reshape(n, m), periodic).reshape(-1)
        assert R.rel_err(x2, xs) > 1e-3


def test_refined_solve_is_high_precision():
    D, L, Rb, A, b, xs, _ = R.cr_system(13, 5, 1)
    r = R._residual_ld(A, xs, b)
    assert float(np.max(np.abs(r))) <= 4 * float(np.finfo(np.longdouble).eps) * float(np.max(np.abs(b))) * 20


@pytest.mark.parametrize("case", sorted({c[:3] for c in R.CR_CASES}), ids=lambda c: "n%d-m%d-p%d" % c)
def test_cr_inputs_meet_conditions(case):
    n, m, per = case
    D, L, Rb, A, b, xs, err = R.cr_system(n, m, per)
    ax = np.abs(np.asarray(xs, dtype=np.float64))
    assert err <= ERR_REF_MAX, err
    assert 0.25 <= ax.min() and ax.max() <= 4.0, (ax.min(), ax.max())
    # the couplings are as large as D's off-diagonal entries
    off = np.abs(D[:, ~np.eye(m, dtype=bool)]).mean() if m > 1 else 0.5
    if n > 1:
        assert 0.5 * off <= np.abs(L).mean() <= 2 * off and 0.5 * off <= np.abs(Rb).mean() <= 2 * off


@pytest.mark.parametrize("n,per", [(2, 1), (3, 1), (6, 0), (6, 1)])
def test_s9_inputs_meet_conditions(n, per):
    m = 7
    S9, col, A, land = R.build_s9(n, m, per, 40 + n + per)
    assert 0.15 <= land.mean() <= 0.6 and (n <= 2 or land.all(axis=1).any())
    b = R.build_rhs(A, n)[0]
    xs = np.asarray(R.refined_solve(A, b), dtype=np.float64)
    assert np.array_equal(xs[land.reshape(-1)], b[land.reshape(-1)])
    assert 0.25 <= np.abs(xs).min() and np.abs(xs).max() <= 4.0


@pytest.mark.parametrize("m", R.GJ_M)
@pytest.mark.parametrize("kind", R.GJ_KINDS)
def test_gj_inputs_meet_conditions(m, kind):
    A = R.gj_blocks(m, kind)
    for a in A:
        Xs = R.refined_inverse(a)
        assert R.rel_err(np.linalg.inv(a), Xs) <= ERR_REF_MAX
        if kind == "perm" and m > 1:
            assert not np.any(np.diag(a))
        if kind == "tie" and m > 2:
            c0 = np.abs(a[:, 0])
            assert np.sum(c0 == c0.max()) == 2


@pytest.mark.parametrize("case", R.BAND_CASES, ids=lambda c: "N%d-bl%d-bu%d" % c[:3])
def test_band_inputs_meet_conditions(case):
    """err_ref of LAPACK's band solve, and the pivot pattern the seeds were picked for: a
    pivot row below its panel, two steps of one panel choosing rows below it, and (wherever a
    panel has rows below it) two steps choosing the same row, which share a staging slot"""
    N, bl, bu, seed = case
    A, lu, piv, Xs, err = R.band_system(N, bl, bu, seed)
    assert err <= ERR_REF_MAX, err
    assert np.count_nonzero(np.diff(np.sort(np.abs(A[A != 0])))== 0) == 0     # no ties
    if N > R.BAND_NBP:
        assert R.band_pivot_facts(piv, N) == (True, True, True)
    # the reference layout helpers invert each other
    ab = R.band_rows(A, bl, bu)
    i = np.arange(N)
    assert np.array_equal(ab[:, bl], A[i, i])
