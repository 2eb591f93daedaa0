"""The sparse-equation reference of the dynamics pass (tests/gs_dyn_ref.py) against the CPU twin
(oracle/prec_oracle.c), without a GPU: the twin's output satisfies the reference's equations, the
excepted rows are few and follow from structure, the reference notices small planted errors, and
the damped defect-correction recurrence holds between the twin's outputs.

Backward error of one twin pass with the Schur solve, max over gs_dyn_ref.rhs_cases, per
(fixture, Mixing) and row kind ("sr": the s rows row by row, over the cases of gs_dyn_ref.DENSE
only).  gs_dyn_ref.TWIN holds these figures rounded up; this test asserts that the twin stays within
twice of them (the figures are rounding residue, which another compiler may move a little) and
that every bound derived from them is at most 1e-8:

    fixture     Mixing        u        v        w        p        s       sr
    test6x6x4   0       3.0e-16  2.8e-16  7.7e-17  1.7e-16  2.0e-15  2.5e-15
    test6x6x4   1       3.0e-16  2.8e-16  7.7e-17  1.7e-16  2.0e-15  2.5e-15
    natl8       0       4.4e-16  4.6e-16  8.1e-17  1.7e-16  1.3e-15  2.3e-15
    natl8       1       4.4e-16  4.6e-16  8.1e-17  1.7e-16  1.3e-15  2.3e-15
    natl8_l8    0       4.2e-16  2.3e-16  6.3e-16  1.6e-16  1.8e-15  3.5e-15
    natl8_l8    1       4.2e-16  2.3e-16  6.3e-16  1.6e-16  1.8e-15  3.5e-15
    odd7x8x4    0       4.8e-16  5.9e-16  1.1e-16  1.4e-16  1.5e-15  9.1e-15
    odd7x8x4    1       4.8e-16  5.9e-16  1.1e-16  1.4e-16  1.5e-15  9.1e-15
    gateway16   0       6.0e-16  5.8e-16  1.3e-15  1.7e-16  7.7e-15  2.8e-13
    gateway16   1       6.0e-16  5.8e-16  1.3e-15  1.7e-16  7.7e-15  2.8e-13
    2dmoc       0       3.6e-16  3.4e-16  1.3e-16  1.4e-16  5.4e-15  1.1e-14
    2dmoc       1       3.6e-16  3.4e-16  1.3e-16  1.4e-16  5.4e-15  1.1e-14
    global4     0       1.1e-15  1.3e-15  1.2e-14  2.0e-16  9.6e-13  1.1e-11
    global4     1       1.1e-15  1.3e-15  1.2e-14  2.0e-16  9.6e-13  1.1e-11

No fixture has a row without an equation (gs_dyn_ref rule R3): test_excepted_set checks it.
"""
import numpy as np
import pytest

import gs_dyn_ref as R

_orc = None
OMEGA = 0.95
CASES = [(name, mixing) for name in R.FIXTURES for mixing in (0, 1)]


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    global _orc
    _orc = oracle_lib


def problem(name, mixing):
    c, L0, o, x, ov, ref, ij, pin, rhs = R.problem(_orc, name, mixing)
    return c, o, ov, ref, ij, pin, rhs


def twin(name, mixing, r, **kw):
    c, o, ov, *_ = problem(name, mixing)
    return _orc.BlockGS(o, ov, 3, **kw).apply(r)


@pytest.mark.parametrize("name,mixing", CASES)
def test_twin_satisfies_equations(name, mixing):
    c, o, ov, ref, ij, pin, rhs = problem(name, mixing)
    M = ref.M(True, pin, ij)
    exc = ref.excepted_rows(True, pin, ij)
    P = _orc.BlockGS(o, ov, 3, dyn_iters=1)
    worst = {}
    for label, r in rhs:
        z = P.apply(r)
        rr, ra = ref.rr_of(r)
        e = ref.row_backward_error(M, ref.dmask(z), rr, exc, ra)
        worst = R.merge(worst, e, R.kinds_of(label))
        assert np.all(np.isfinite(z))
        assert e["live"] > 0 and np.any(ref.dmask(z)), f"{label} reaches no judged row"
        assert np.array_equal(z[ref.known], r[ref.known]), label
        assert ref.pin_violation(z, True, pin, ij) == 0.0, label
    print(f"twin {name} mixing={mixing}: " + " ".join(f"{t} {worst[t]:.1e}" for t in R.KINDS))
    for t in R.KINDS:
        assert worst[t] <= 2.0 * R.TWIN[(name, mixing)][t], (t, worst[t])
        assert R.bound(name, mixing, t) <= 1e-8


@pytest.mark.parametrize("name,mixing", CASES)
def test_excepted_set(name, mixing):
    """structure only: one P row per pinned column (Schur pass) or per water column (pass without
    the Schur solve), nothing else, and no row without an equation"""
    c, o, ov, ref, ij, pin, rhs = problem(name, mixing)
    assert ref.no_equation_rows.size == 0, ref.no_equation_rows
    assert pin.sum() >= 1 and len(ij) == np.count_nonzero(ref.top >= 0)
    if name == "gateway16":
        assert pin.sum() > 2            # several basins
    for schur, ncols in ((True, int(pin.sum())), (False, len(ij))):
        exc = ref.excepted_rows(schur, pin, ij)
        assert len(exc) == ncols and len(set(exc.tolist())) == ncols
        assert np.all(exc % R.NUN == R.PP) and np.all(ref.active[exc])
        cols = sorted(int((row // R.NUN) % (c.n * c.m)) for row in exc)
        assert cols == sorted(int(q) for q in ref.columns(schur, pin, ij))
        # the closing row is the column's top active level, where the pass leaves p = 0
        assert np.array_equal(np.sort(exc), np.sort(ref.top_rows(schur, pin, ij)))


def _seed3(name, mixing):
    c, o, ov, ref, ij, pin, rhs = problem(name, mixing)
    r = rhs[0][1]
    rr, ra = ref.rr_of(r)
    return ref, ij, pin, r, rr, ra, twin(name, mixing, r, dyn_iters=1)


_limit = R.limit


@pytest.mark.parametrize("name,mixing", [("natl8", 0), ("gateway16", 1), ("global4", 1)])
def test_reference_can_fail(name, mixing):
    ref, ij, pin, r, rr, ra, z = _seed3(name, mixing)
    M, exc = ref.M(True, pin, ij), ref.excepted_rows(True, pin, ij)
    lim = _limit(name, mixing)
    kinds = R.worst
    err = lambda v: kinds(ref.row_backward_error(M, ref.dmask(v), rr, exc, ra))
    assert err(z) <= lim
    # one W entry scaled by 1 + 1e-6
    wrows = np.nonzero(ref.active & (ref.var == R.WW))[0]
    zw = z.copy()
    zw[wrows[np.argmax(np.abs(z[wrows]))]] *= 1.0 + 1e-6
    # one U entry beside land: an active U point with an identity U point (or the grid's edge) beside it
    ua = ref.active[R.UU::R.NUN].reshape(ref.l, ref.m, ref.n)
    inner = np.ones_like(ua)
    for ax, sh in ((1, 1), (1, -1), (2, 1), (2, -1)):
        nb = np.roll(ua, sh, axis=ax)
        if ax == 1 or not ref.periodic:
            nb[(slice(None),) * ax + (0 if sh > 0 else -1,)] = False
        inner &= nb
    beside = R.NUN * np.nonzero((ua & ~inner).reshape(-1))[0] + R.UU
    assert beside.size
    zu = z.copy()
    zu[beside[np.argmax(np.abs(z[beside]))]] *= 1.0 + 1e-6
    # p shifted by a constant in one column that is not pinned
    q = int(ij[~pin][len(ij[~pin]) // 2])
    i, j = q % ref.n, q // ref.n
    prow = np.array([ref.row_of(i, j, k, R.PP) for k in range(ref.l) if ref.pa[k, j, i]])
    zp = z.copy()
    zp[prow] += 1e-6 * np.max(np.abs(z[ref.var == R.PP]))
    for label, v in (("w", zw), ("u", zu), ("p column", zp)):
        print(f"{name} planted {label}: {err(v):.1e} (clean {err(z):.1e}, limit {lim:.1e})")
        assert err(v) > lim, label
    # a pass without the Schur solve, judged by the with-Schur equations
    z2 = twin(name, mixing, r, dyn_iters=2, dyn_omega=OMEGA, schur_passes=1)
    e = kinds(ref.recurrence_error(M, ref.dmask(z), ref.dmask(z2), OMEGA, rr, ra, exc))
    print(f"{name} pass without Schur against the Schur equations: {e:.1e}")
    assert e > lim
    e = ref.recurrence_error(ref.M(False, pin, ij), ref.dmask(z), ref.dmask(z2), OMEGA, rr, ra,
                             ref.excepted_rows(False, pin, ij))
    R.check(e, name, mixing, R.KINDS)


@pytest.mark.parametrize("name,mixing", [("natl8", 1), ("gateway16", 1), ("global4", 1)])
def test_recurrence_on_twin(name, mixing):
    """M_k (z_{k+1} - z_k) = w (rr_D - A_DD z_k) off the excepted rows of pass k, for every pass a
    Schur pass (0), the first only (1) and the default rule (2: the first and the last); every row
    kind within its own bound of the single pass (a step is one pass on the right-hand side d)"""
    c, o, ov, ref, ij, pin, rhs = problem(name, mixing)
    r = rhs[0][1]
    rr, ra = ref.rr_of(r)
    z = {(sp_k, k): ref.dmask(twin(name, mixing, r, dyn_iters=k, dyn_omega=OMEGA, schur_passes=sp_k))
         for sp_k in (0, 1, 2) for k in (1, 2, 3, 4)}
    steps = [(sp_k, k, (sp_k, k), sp_k == 0) for sp_k in (0, 1) for k in (1, 2, 3)]
    # the default's last pass is a Schur pass on the iterate of three passes, the first only solving
    steps.append((2, 3, (1, 3), True))
    for sp_k, k, prev, schur in steps:
        assert schur == R.schur_rule(sp_k, k, k + 1)
        e = ref.recurrence_error(ref.M(schur, pin, ij), z[prev], z[(sp_k, k + 1)], OMEGA, rr, ra,
                                 ref.excepted_rows(schur, pin, ij))
        print(f"twin recurrence {name} schur_passes={sp_k} pass {k + 1}: {R.fmt(e)}")
        R.check(e, name, mixing, R.KINDS, (sp_k, k))
        assert ref.pin_violation(z[(sp_k, k + 1)] - z[prev], schur, pin, ij) == 0.0
