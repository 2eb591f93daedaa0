"""The dense solvers of the preconditioner, each on its own, against high-precision references:
block cyclic reduction (csrc/schur_cr.hip with cr_plan.hip and cr_factor.hip), its batched Gauss-Jordan
inverse (k_cr_inv, csrc/cr_inv.hip) and
the band LU with explicit inverse (csrc/band_lu.hip), through the test hooks of
csrc/test_hooks.hip (tests/dense_hooks.py).

Tolerance rule, the same everywhere: with x* the refined solution (tests/cr_ref.py),
err = ||x - x*||inf / ||x*||inf over all entries, err_dev of the device and err_ref of the
float64 CPU yardstick (cr_ref / np.linalg.inv / LAPACK dgbtrs):
    err_dev <= max(10 err_ref, 8 m eps)          (N for m in the band cases)
Yardstick and device do the same eliminations in float64 and differ in summation order, the
explicit tail inverse and the composed operators: one order of magnitude.  A wrong term costs
about ten.  Every test prints err_ref, err_dev and their ratio before it asserts.

Measured on the MI355X (gfx950).  One row per case; a Gauss-Jordan case is its seven
inversions (two with s0 = 1, sstep = 2, five with s0 = 0, sstep = 1) and shows the one
nearest its bound; a cyclic-reduction case solved by several tests shows the same.

family  case                               err_ref   err_dev   ratio   bound
------  ---------------------------------  --------  --------  ------  --------
gj      m=1 random                         4.76e-17  4.76e-17    1.00  1.78e-15
gj      m=1 perm                           8.86e-17  8.86e-17    1.00  1.78e-15
gj      m=1 tie                            5.35e-17  5.35e-17    1.00  1.78e-15
gj      m=2 random                         8.39e-17  8.39e-17    1.00  3.55e-15
gj      m=2 perm                           8.09e-17  8.09e-17    1.00  3.55e-15
gj      m=2 tie                            3.50e-16  3.50e-16    1.00  3.55e-15
gj      m=15 random                        1.58e-15  2.36e-15    1.49  2.66e-14
gj      m=15 perm                          1.35e-16  3.09e-16    2.29  2.66e-14
gj      m=15 tie                           1.12e-15  2.36e-15    2.11  2.66e-14
gj      m=16 random                        1.28e-15  7.93e-15    6.20  2.84e-14
gj      m=16 perm                          2.04e-16  4.52e-16    2.22  2.84e-14
gj      m=16 tie                           2.10e-14  2.39e-14    1.14  2.10e-13
gj      m=17 random                        2.87e-15  1.81e-15    0.63  3.02e-14
gj      m=17 perm                          1.71e-16  4.84e-16    2.83  3.02e-14
gj      m=17 tie                           4.69e-15  3.06e-15    0.65  4.69e-14
gj      m=31 random                        1.44e-15  1.25e-14    8.68  5.51e-14
gj      m=31 perm                          2.78e-16  6.64e-16    2.39  5.51e-14
gj      m=31 tie                           7.14e-15  1.66e-14    2.32  7.14e-14
gj      m=32 random                        7.45e-15  3.79e-14    5.09  7.45e-14
gj      m=32 perm                          4.11e-16  9.06e-16    2.20  5.68e-14
gj      m=32 tie                           8.91e-15  8.21e-15    0.92  8.91e-14
gj      m=33 random                        1.72e-15  2.47e-15    1.44  5.86e-14
gj      m=33 perm                          4.98e-16  5.21e-16    1.05  5.86e-14
gj      m=33 tie                           2.39e-14  6.58e-14    2.75  2.39e-13
gj      m=63 random                        3.58e-15  4.93e-15    1.38  1.12e-13
gj      m=63 perm                          2.94e-16  7.31e-16    2.49  1.12e-13
gj      m=63 tie                           5.68e-14  3.88e-14    0.68  5.68e-13
gj      m=64 random                        1.25e-15  5.64e-15    4.51  1.14e-13
gj      m=64 perm                          3.33e-16  8.58e-16    2.58  1.14e-13
gj      m=64 tie                           1.94e-15  2.46e-15    1.27  1.14e-13
gj      m=65 random                        7.80e-14  3.72e-13    4.77  7.80e-13
gj      m=65 perm                          4.53e-16  8.90e-16    1.96  1.15e-13
gj      m=65 tie                           1.67e-14  1.71e-14    1.02  1.67e-13
gj      m=96 random                        2.15e-14  2.61e-14    1.21  2.15e-13
gj      m=96 perm                          5.55e-16  1.24e-15    2.23  1.71e-13
gj      m=96 tie                           7.66e-14  8.40e-14    1.10  7.66e-13
gj      m=97 random                        2.33e-15  6.37e-15    2.73  1.72e-13
gj      m=97 perm                          6.87e-16  1.03e-15    1.50  1.72e-13
gj      m=97 tie                           4.52e-15  6.55e-15    1.45  1.72e-13
gj      m=128 random                       3.80e-14  4.61e-14    1.21  3.80e-13
gj      m=128 perm                         5.34e-16  1.59e-15    2.98  2.27e-13
gj      m=128 tie                          2.77e-14  5.64e-14    2.04  2.77e-13
gj      m=129 random                       1.27e-14  1.30e-14    1.02  2.29e-13
gj      m=129 perm                         4.45e-16  1.49e-15    3.35  2.29e-13
gj      m=129 tie                          5.86e-15  1.24e-14    2.12  2.29e-13
gj      m=160 random                       1.75e-14  1.35e-14    0.77  2.84e-13
gj      m=160 perm                         5.82e-16  1.97e-15    3.38  2.84e-13
gj      m=160 tie                          1.42e-14  7.47e-14    5.26  2.84e-13
gj      m=161 random                       1.04e-14  5.62e-14    5.40  2.86e-13
gj      m=161 perm                         5.17e-16  1.83e-15    3.54  2.86e-13
gj      m=161 tie                          2.04e-14  2.02e-14    0.99  2.86e-13
gj      m=191 random                       4.37e-15  1.60e-14    3.66  3.39e-13
gj      m=191 perm                         7.99e-16  1.88e-15    2.35  3.39e-13
gj      m=191 tie                          2.59e-14  2.38e-13    9.19  3.39e-13
gj      m=192 random                       1.83e-14  2.22e-14    1.21  3.41e-13
gj      m=192 perm                         6.20e-16  1.64e-15    2.65  3.41e-13
gj      m=192 tie                          8.05e-15  3.17e-14    3.94  3.41e-13
cr      n=1 m=5 per=0 tail_max=1           1.78e-16  7.76e-17    0.44  8.88e-15
cr      n=1 m=5 per=0 tail_max=0           1.78e-16  7.76e-17    0.44  8.88e-15
cr      n=1 m=5 per=1 tail_max=1           1.47e-16  1.40e-16    0.95  8.88e-15
cr      n=1 m=5 per=1 tail_max=0           1.47e-16  1.40e-16    0.95  8.88e-15
cr      n=2 m=5 per=0 tail_max=1           3.14e-16  1.60e-16    0.51  8.88e-15
cr      n=2 m=5 per=0 tail_max=0           3.14e-16  1.66e-16    0.53  8.88e-15
cr      n=2 m=5 per=1 tail_max=1           2.00e-16  1.78e-16    0.89  8.88e-15
cr      n=2 m=5 per=1 tail_max=0           2.00e-16  2.00e-16    1.00  8.88e-15
cr      n=3 m=5 per=0 tail_max=1           1.84e-16  1.84e-16    1.00  8.88e-15
cr      n=3 m=5 per=0 tail_max=0           1.84e-16  2.65e-16    1.44  8.88e-15
cr      n=3 m=5 per=1 tail_max=1           2.39e-16  3.90e-16    1.63  8.88e-15
cr      n=3 m=5 per=1 tail_max=0           2.39e-16  2.70e-16    1.13  8.88e-15
cr      n=4 m=5 per=0 tail_max=1           2.47e-16  1.65e-16    0.67  8.88e-15
cr      n=4 m=5 per=0 tail_max=0           2.47e-16  2.07e-16    0.84  8.88e-15
cr      n=4 m=5 per=1 tail_max=1           2.06e-16  2.82e-16    1.37  8.88e-15
cr      n=4 m=5 per=1 tail_max=0           2.06e-16  2.14e-16    1.04  8.88e-15
cr      n=5 m=5 per=0 tail_max=1           2.84e-16  2.84e-16    1.00  8.88e-15
cr      n=5 m=5 per=0 tail_max=0           2.84e-16  2.84e-16    1.00  8.88e-15
cr      n=5 m=5 per=1 tail_max=1           3.79e-16  2.25e-16    0.59  8.88e-15
cr      n=5 m=5 per=1 tail_max=0           3.79e-16  3.46e-16    0.91  8.88e-15
cr      n=6 m=5 per=0 tail_max=1           2.96e-16  3.96e-16    1.34  8.88e-15
cr      n=6 m=5 per=0 tail_max=0           2.96e-16  3.95e-16    1.33  8.88e-15
cr      n=6 m=5 per=1 tail_max=1           2.71e-16  4.09e-16    1.51  8.88e-15
cr      n=6 m=5 per=1 tail_max=0           2.71e-16  4.09e-16    1.51  8.88e-15
cr      n=7 m=5 per=0 tail_max=1           4.78e-16  4.78e-16    1.00  8.88e-15
cr      n=7 m=5 per=0 tail_max=0           4.78e-16  4.88e-16    1.02  8.88e-15
cr      n=7 m=5 per=1 tail_max=1           3.32e-16  2.70e-16    0.81  8.88e-15
cr      n=7 m=5 per=1 tail_max=0           3.32e-16  3.62e-16    1.09  8.88e-15
cr      n=12 m=5 per=0 tail_max=1          3.60e-16  3.71e-16    1.03  8.88e-15
cr      n=12 m=5 per=0 tail_max=0          3.60e-16  3.95e-16    1.10  8.88e-15
cr      n=12 m=5 per=1 tail_max=1          3.17e-16  4.59e-16    1.45  8.88e-15
cr      n=12 m=5 per=1 tail_max=0          3.17e-16  4.30e-16    1.36  8.88e-15
cr      n=13 m=5 per=0 tail_max=1          4.67e-16  3.59e-16    0.77  8.88e-15
cr      n=13 m=5 per=0 tail_max=0          4.67e-16  4.59e-16    0.98  8.88e-15
cr      n=13 m=5 per=1 tail_max=1          2.79e-16  3.16e-16    1.13  8.88e-15
cr      n=13 m=5 per=1 tail_max=0          2.79e-16  2.96e-16    1.06  8.88e-15
cr      n=23 m=5 per=0 tail_max=1          5.14e-16  4.70e-16    0.91  8.88e-15
cr      n=23 m=5 per=0 tail_max=0          5.14e-16  4.35e-16    0.85  8.88e-15
cr      n=23 m=5 per=1 tail_max=1          3.02e-16  4.40e-16    1.46  8.88e-15
cr      n=23 m=5 per=1 tail_max=0          3.02e-16  5.34e-16    1.77  8.88e-15
cr      n=45 m=5 per=0 tail_max=1          5.11e-16  4.51e-16    0.88  8.88e-15
cr      n=45 m=5 per=0 tail_max=0          5.11e-16  4.23e-16    0.83  8.88e-15
cr      n=45 m=5 per=1 tail_max=1          4.80e-16  5.25e-16    1.09  8.88e-15
cr      n=45 m=5 per=1 tail_max=0          4.80e-16  5.25e-16    1.09  8.88e-15
cr      n=96 m=5 per=0 tail_max=1          4.80e-16  6.30e-16    1.31  8.88e-15
cr      n=96 m=5 per=0 tail_max=0          4.80e-16  4.86e-16    1.01  8.88e-15
cr      n=96 m=5 per=1 tail_max=1          4.72e-16  5.94e-16    1.26  8.88e-15
cr      n=96 m=5 per=1 tail_max=0          4.72e-16  6.14e-16    1.30  8.88e-15
cr      n=45 m=5 per=0 tail_max=115        5.11e-16  4.56e-16    0.89  8.88e-15
cr      n=45 m=5 per=0 tail_max=60         5.11e-16  4.77e-16    0.93  8.88e-15
cr      n=45 m=5 per=0 tail_max=30         5.11e-16  6.19e-16    1.21  8.88e-15
cr      n=45 m=5 per=1 tail_max=115        4.80e-16  5.71e-16    1.19  8.88e-15
cr      n=45 m=5 per=1 tail_max=60         4.80e-16  6.73e-16    1.40  8.88e-15
cr      n=45 m=5 per=1 tail_max=30         4.80e-16  4.42e-16    0.92  8.88e-15
cr      n=96 m=5 per=0 tail_max=240        4.80e-16  6.30e-16    1.31  8.88e-15
cr      n=96 m=5 per=0 tail_max=120        4.80e-16  7.79e-16    1.62  8.88e-15
cr      n=96 m=5 per=0 tail_max=60         4.80e-16  7.79e-16    1.62  8.88e-15
cr      n=96 m=5 per=1 tail_max=240        4.72e-16  5.60e-16    1.19  8.88e-15
cr      n=96 m=5 per=1 tail_max=120        4.72e-16  5.80e-16    1.23  8.88e-15
cr      n=96 m=5 per=1 tail_max=60         4.72e-16  5.98e-16    1.27  8.88e-15
cr      n=6 m=128 per=0 tail_max=1         9.09e-16  1.63e-15    1.79  2.27e-13
cr      n=6 m=128 per=1 tail_max=1         8.49e-16  1.96e-15    2.31  2.27e-13
cr      n=6 m=129 per=0 tail_max=1         9.81e-16  1.49e-15    1.52  2.29e-13
cr      n=6 m=129 per=1 tail_max=1         8.90e-16  1.69e-15    1.90  2.29e-13
cr      n=6 m=192 per=0 tail_max=1         9.91e-16  1.87e-15    1.89  3.41e-13
cr      n=6 m=192 per=1 tail_max=1         1.02e-15  1.72e-15    1.69  3.41e-13
cr      n=7 m=33 per=0 tail_max=1          6.18e-16  8.12e-16    1.31  5.86e-14
cr      n=7 m=33 per=1 tail_max=1          6.14e-16  7.14e-16    1.16  5.86e-14
cr      n=180 m=33 per=1 tail_max=0        8.48e-16  9.25e-16    1.09  5.86e-14
cr      n=80 m=96 per=1 tail_max=0         9.96e-16  1.98e-15    1.99  1.71e-13
cr      n=80 m=97 per=1 tail_max=0         9.21e-16  1.66e-15    1.80  1.72e-13
cr      n=80 m=97 per=0 tail_max=0         1.11e-15  1.61e-15    1.45  1.72e-13
cr      n=5 m=100 per=0 tail_max=1         8.12e-16  1.49e-15    1.83  1.78e-13
cr      n=5 m=100 per=1 tail_max=1         7.90e-16  1.47e-15    1.86  1.78e-13
cr      n=5 m=170 per=0 tail_max=1         9.69e-16  1.71e-15    1.76  3.02e-13
cr      n=5 m=170 per=1 tail_max=1         1.08e-15  1.67e-15    1.55  3.02e-13
cr      n=8 m=128 per=1 tail_max=0         9.03e-16  2.07e-15    2.29  2.27e-13
cr      n=7 m=33 per=1 tail_max=0          6.14e-16  7.14e-16    1.16  5.86e-14
cr      n=7 m=33 per=0 tail_max=0          6.18e-16  7.14e-16    1.16  5.86e-14
expand  n=2 m=9 per=1 tail_max=1           1.43e-16  2.06e-16    1.44  1.60e-14
expand  n=3 m=9 per=1 tail_max=1           2.81e-16  1.95e-16    0.69  1.60e-14
expand  n=6 m=9 per=0 tail_max=1           2.58e-16  2.55e-16    0.99  1.60e-14
expand  n=6 m=9 per=1 tail_max=1           2.02e-16  5.07e-16    2.51  1.60e-14
expand  n=6 m=9 per=1 tail_max=0           2.02e-16  4.16e-16    2.06  1.60e-14
expand  n=40 m=33 per=1 tail_max=0         8.80e-16  5.56e-16    0.63  5.86e-14
band    N=1 bl=1 bu=1                      6.88e-17  6.88e-17    1.00  1.78e-15
band    N=15 bl=3 bu=3                     4.22e-16  4.18e-16    0.99  2.66e-14
band    N=16 bl=3 bu=3                     3.48e-15  5.58e-16    0.16  3.48e-14
band    N=17 bl=3 bu=3                     4.14e-15  1.37e-15    0.33  4.14e-14
band    N=33 bl=5 bu=2                     3.56e-15  2.52e-16    0.07  5.86e-14
band    N=33 bl=2 bu=7                     2.96e-16  3.38e-15   11.42  5.86e-14
band    N=100 bl=17 bu=17                  4.14e-15  2.33e-15    0.56  1.78e-13
band    N=257 bl=40 bu=40                  1.95e-14  2.22e-14    1.14  4.57e-13
band    N=500 bl=230 bu=230                3.46e-14  4.54e-14    1.31  8.88e-13
band    N=500 bl=240 bu=240                3.34e-14  3.15e-14    0.94  8.88e-13

Findings recorded with the table:
* k_band_lu loaded and stored panel entries right of a row's band (t - r > bl + bu) from the
  neighbouring rows, so every band narrower than the panel (bl + bu < 15) was factorised wrong.
  Before the fix the cases (15,3,3), (16,3,3), (17,3,3), (33,5,2), (33,2,7) chose other pivots
  than LAPACK from about step 10 on (e.g. N = 15: 11 where LAPACK takes 13); production widths
  (bl + bu >= 18) never reach the branch and are bitwise unchanged.
* One-level fallback of cr_build_steps: enumerating n = 2..64, periodic 0 and 1, tail_max = 1,
  no plan holds a one-level step where two levels were left; the fallback is unreachable there.
* rc = 8 on the way down needs >= 448 workgroups: (96, 33) gives 240, so (180, 33) stands in.
* k_band_inv_pan's STAGE = true variant is never instantiated, and is not tested.
* Value-only mutants (scratch builds): k_cr_pk without its last column group fails 14 tests
  here (rc4, rc8, m = 100 / 170 / 128, reuse); +1.0 for one s2 of the next-level D GEMM fails 79
  (every solve with more than one level); k_band_lu without the last U12 term fails 7 band
  cases; pivot ties broken toward the higher row fail the 17 "tie" Gauss-Jordan cases and no
  test of the suite before this module.
"""
import numpy as np
import pytest

import cr_ref as R
import dense_hooks as H
from helpers import golden_landm
from iemic import config as cf

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def h():
    """any single-rank context serves: the test6x6x4 ocean"""
    from iemic.ocean import Ocean
    oc = Ocean(cf.preset("test6x6x4", mixing=0), landm=golden_landm("test6x6x4"))
    yield oc._h
    oc.close()


def report(what, err_ref, err_dev, size):
    print(f"DENSE {what}: err_ref {err_ref:.2e} err_dev {err_dev:.2e} ratio "
          f"{err_dev / err_ref if err_ref > 0 else float('inf'):.2f} bound {R.bound(err_ref, size):.2e}")


def solve_case(h, n, m, per, tm, **kw):
    D, L, Rb, A, b, xs, err_ref = R.cr_system(n, m, per)
    rc, x, xT, info, plan = H.cr_solve(h, n, m, per, tm, b[None, :], D, L, Rb, **kw)
    assert rc == 0, H.last_error()
    assert info == 0
    err_dev = R.rel_err(x[0], xs)
    report(f"cr n={n} m={m} per={per} tail_max={tm} {plan}", err_ref, err_dev, m)
    assert err_dev <= R.bound(err_ref, m), (err_dev, err_ref)
    return x[0], xT, plan


# ------------------------------------------------------------------ A. Gauss-Jordan
@pytest.mark.parametrize("kind", R.GJ_KINDS)
@pytest.mark.parametrize("m", R.GJ_M)
def test_gauss_jordan(h, m, kind):
    A = R.gj_blocks(m, kind)
    Xs = [R.refined_inverse(a) for a in A]
    err_ref = [R.rel_err(np.linalg.inv(a), xs) for a, xs in zip(A, Xs)]
    for s0, sstep, count in ((1, 2, 2), (0, 1, 5)):
        rc, X, info = H.cr_inverse(h, A, s0, sstep, count)
        assert rc == 0, H.last_error()
        assert info == 0
        for k in range(count):
            s = s0 + k * sstep
            err_dev = R.rel_err(X[k], Xs[s])
            report(f"gj m={m} {kind} s0={s0} block {s}", err_ref[s], err_dev, m)
            assert err_dev <= R.bound(err_ref[s], m), (s, err_dev, err_ref[s])
            nrm = np.abs(X[k]).sum(1).max() * np.abs(A[s]).sum(1).max()
            res = lambda Y: float(np.abs(Y.astype(np.longdouble) @ A[s].astype(np.longdouble)
                                         - np.eye(m)).sum(1).max()) / nrm
            assert res(X[k]) <= R.bound(res(np.linalg.inv(A[s])), m)


@pytest.mark.parametrize("m", [17, 97, 192])
@pytest.mark.parametrize("what", ["zero_row", "nan"])
def test_gauss_jordan_singular_and_nonfinite(h, m, what):
    """a singular / non-finite block sets info and the kernel returns; its batch mates stay right"""
    A = R.gj_blocks(m, "random").copy()
    if what == "zero_row":
        A[2, m // 2, :] = 0.0
    else:
        A[2, m // 3, m // 2] = np.nan
    rc, X, info = H.cr_inverse(h, A, 0, 1, 5)
    assert rc == 0, H.last_error()
    assert info == 1
    for s in (0, 1, 3, 4):
        Xs = R.refined_inverse(A[s])
        assert R.rel_err(X[s], Xs) <= R.bound(R.rel_err(np.linalg.inv(A[s]), Xs), m)


def test_gauss_jordan_refuses_193(h):
    A = np.eye(193)[None].repeat(2, 0)
    rc, X, info = H.cr_inverse(h, A, 0, 1, 2)
    assert rc == H.EINVAL and "192" in H.last_error()
    assert np.isnan(X).all()


# ------------------------------------------------------------------ B. cyclic reduction
@pytest.mark.parametrize("case", R.CR_CHAIN, ids=lambda c: "n%d-m%d-p%d-t%d" % c)
def test_cr_level_chains(h, case):
    n, m, per, tm = case
    x, _, plan = solve_case(h, n, m, per, tm)
    if tm == 1:                       # every level through k_cr_pk, the last block k_cr_final
        assert plan.tM == 0 and sum(s[3] for s in plan.down) == plan.nlev == sum(s[3] for s in plan.up)
    else:                             # n m <= 1024: the whole problem is the tail
        assert (plan.tM, plan.lt, plan.nsteps) == ((n * m, 0, 0) if n > 1 else (0, 0, 0))


@pytest.mark.parametrize("case", R.CR_TAILPOS, ids=lambda c: "n%d-m%d-p%d-t%d" % c)
def test_cr_tail_placement(h, case):
    n, m, per, tm = case
    _, _, plan = solve_case(h, n, m, per, tm)
    want = {115: (1, [1]), 60: (2, [2]), 30: (3, [2, 1])} if n == 45 else \
           {240: (1, [1]), 120: (2, [2]), 60: (3, [2, 1])}
    lt, spans = want[tm]
    assert plan.lt == lt and plan.tM == tm
    assert [s[3] for s in plan.down] == spans and [s[3] for s in plan.up] == spans[::-1]


@pytest.mark.parametrize("case", R.CR_RC4, ids=lambda c: "n%d-m%d-p%d-t%d" % c)
def test_cr_packed_rc4(h, case):
    _, _, plan = solve_case(h, *case)
    assert plan.tM == 0 and all(s[0] == 4 for s in plan.down + plan.up)


@pytest.mark.parametrize("case", R.CR_RC8, ids=lambda c: "n%d-m%d-p%d-t%d" % c)
def test_cr_packed_rc8(h, case):
    _, _, plan = solve_case(h, *case)
    assert any(s[0] == 8 for s in plan.down) and any(s[0] == 8 for s in plan.up)


@pytest.mark.parametrize("case", R.CR_INVLEV + R.CR_TAILEDGE, ids=lambda c: "n%d-m%d-p%d-t%d" % c)
def test_cr_inverse_classes_and_tail_edges(h, case):
    n, m, per, tm = case
    _, _, plan = solve_case(h, n, m, per, tm)
    if tm == 0:
        assert plan.tM == n * m and (n * m == 1024 or (n * m) % 4)


def test_cr_tail_above_1024_refused(h):
    """cr_init accepts tail_max > 1024 (the multigrid's explicit inverse), cr_solve has no
    kernel for such a tail: a host refusal"""
    n, m = 8, 150
    D, L, Rb, A, b, xs, _ = R.cr_system(n, m, 1)
    rc, x, _, info, plan = H.cr_solve(h, n, m, 1, 2048, b[None, :], D, L, Rb)
    assert plan.tM == 1200 and info == 0
    assert rc == H.EINVAL and "1200" in H.last_error()
    assert np.isnan(x).all()


def spans(h, n, per):
    """the plan of (n, m = 5, tail_max = 1); no solve"""
    rc, _, _, _, plan = H.cr_solve(h, n, 5, per, 1, None, *R.build_blocks(n, 5, n))
    assert rc == 0, H.last_error()
    return plan


def test_cr_one_level_fallback_enumeration(h):
    """n = 2..64, both periodic values, tail_max = 1: where does cr_build_steps take a
    one-level step although two levels were left?  The smallest such case is solved."""
    hits = []
    for per in (0, 1):
        for n in range(2, 65):
            plan = spans(h, n, per)
            left = plan.nlev
            for s in plan.down:
                if s[3] == 1 and left >= 2:
                    hits.append((n, per))
                    break
                left -= s[3]
    print("DENSE fallback: one-level steps with two levels available at (n, periodic):", hits)
    if hits:
        n, per = min(hits)
        solve_case(h, n, 5, per, 1)


@pytest.mark.parametrize("case", [(1, 5, 1, 1), (1, 5, 0, 0), (12, 5, 1, 0), (45, 5, 1, 1), (45, 5, 0, 60),
                                  (180, 33, 1, 0)], ids=lambda c: "n%d-m%d-p%d-t%d" % c)
def test_cr_transposed_solution(h, case):
    n, m, per, tm = case
    x, xT, plan = solve_case(h, n, m, per, tm, want_xT=True)
    assert np.array_equal(bits(xT[0].reshape(m, n)), bits(x.reshape(n, m).T))


@pytest.mark.parametrize("case", [(45, 5, 1, 1), (45, 5, 1, 60), (12, 5, 1, 0), (80, 97, 1, 0)],
                         ids=lambda c: "n%d-m%d-p%d-t%d" % c)
def test_cr_reuse(h, case):
    n, m, per, tm = case
    D, L, Rb, A, b, xs, err_ref = R.cr_system(n, m, per)
    b3 = np.stack([b, R.build_rhs(A, 99)[0], b])
    rc, x, _, info, _ = H.cr_solve(h, n, m, per, tm, b3, D, L, Rb)
    assert rc == 0 and info == 0, H.last_error()
    assert np.array_equal(bits(x[2]), bits(x[0]))
    xs2 = R.refined_solve(A, b3[1])
    assert R.rel_err(x[1], xs2) <= R.bound(R.rel_err(
        R.cr_ref(D, L, Rb, b3[1].reshape(n, m), per).reshape(-1), xs2), m)
    # another matrix first, then this one on the same SchurCR: bitwise a fresh one's answer
    other = R.build_blocks(n, m, 4242 + n)
    rc, xr = H.cr_refactor(h, n, m, per, tm, other, (D, L, Rb), b)
    assert rc == 0, H.last_error()
    assert np.array_equal(bits(xr), bits(x[0]))


@pytest.mark.parametrize("case", [(2, 1, 1), (3, 1, 1), (6, 0, 1), (6, 1, 1), (6, 1, 0), (40, 1, 0)],
                         ids=lambda c: "n%d-p%d-t%d" % c)
def test_cr_expand_from_nine_point_rows(h, case):
    n, per, tm = case
    m = 33 if n == 40 else 9
    S9, col, A, land = R.build_s9(n, m, per, 40 + n + per)
    b = R.build_rhs(A, n)[0]
    xs = R.refined_solve(A, b)
    rc, x, _, info, plan = H.cr_solve(h, n, m, per, tm, b[None, :], S9=S9, col_of_ij=col)
    assert rc == 0 and info == 0, H.last_error()
    xr = np.linalg.solve(A.toarray(), b)
    err_ref, err_dev = R.rel_err(xr, xs), R.rel_err(x[0], xs)
    report(f"expand n={n} m={m} per={per} tail_max={tm}", err_ref, err_dev, m)
    assert err_dev <= R.bound(err_ref, m)
    lf = land.reshape(-1)
    assert lf.any() and np.array_equal(bits(x[0][lf]), bits(b[lf]))


def test_cr_singular_odd_block(h):
    n, m = 6, 5
    D, L, Rb, A, b, xs, _ = R.cr_system(n, m, 1)
    D = np.array(D)
    D[3, 2, :] = 0.0
    rc, x, _, info, _ = H.cr_solve(h, n, m, 1, 1, b[None, :], D, L, Rb)
    assert info == 1
    assert rc == H.EINVAL and "singular block" in H.last_error()


# ------------------------------------------------------------------ C. band LU and inverse
@pytest.mark.parametrize("case", R.BAND_CASES, ids=lambda c: "N%d-bl%d-bu%d" % c[:3])
def test_band_lu_inverse(h, case):
    N, bl, bu, seed = case
    A, lu, piv, Xs, err_ref = R.band_system(N, bl, bu, seed)
    rc, ab, dpiv, X, info, so = H.band_inverse(h, N, bl, bu, R.band_rows(A, bl, bu))
    assert rc == 0, H.last_error()
    assert info == 0
    assert so == R.BAND_STAGE_O.get((N, bl, bu), 1)
    below, two, shared = R.band_pivot_facts(dpiv, N)
    print(f"DENSE band N={N} bl={bl} bu={bu} stage_o={so} pivot below panel {below}, two in a panel {two}, "
          f"shared row {shared}")
    assert np.array_equal(dpiv, piv)
    if N > R.BAND_NBP:
        assert below and two
    U = R.band_u_rows(lu, bl, bu)
    eu = float(np.max(np.abs(ab[:, bl:] - U)) / np.max(np.abs(U)))
    err_dev = R.rel_err(X, Xs)
    report(f"band N={N} bl={bl} bu={bu} (U differs from LAPACK's by {eu:.2e})", err_ref, err_dev, N)
    assert eu <= R.bound(0.0, N)
    assert not np.isnan(X).any()
    assert err_dev <= R.bound(err_ref, N), (err_dev, err_ref)
    nrm = np.abs(X).sum(1).max() * np.abs(A).sum(1).max()
    Xl = np.asarray(Xs, dtype=np.float64)
    res = lambda Y: float(np.abs(Y @ A - np.eye(N)).sum(1).max()) / nrm
    assert res(X) <= max(10 * res(Xl), 8 * N * R.EPS)


def test_band_singular(h):
    N, bl, bu = 33, 5, 2
    A = np.array(R.band_system(N, bl, bu, 0)[0])
    A[:, 20] = 0.0
    rc, ab, piv, X, info, so = H.band_inverse(h, N, bl, bu, R.band_rows(A, bl, bu), prefill=-7.25)
    assert rc == 0, H.last_error()
    assert info == 21
    assert np.all(X == -7.25)


@pytest.mark.parametrize("shape", [(500, 420, 420), (0, 1, 1), (8, -1, 2)])
def test_band_out_of_range_refused(h, shape):
    """above the LDS of a workgroup (and nonsense shapes): refused on the host, nothing runs"""
    N, bl, bu = shape
    rc, ab, piv, X, info, so = H.band_inverse(h, N, bl, bu, np.zeros((max(N, 1), 2 * abs(bl) + abs(bu) + 1)),
                                              prefill=3.5)
    assert rc == H.EINVAL
    assert np.all(X == 3.5)
