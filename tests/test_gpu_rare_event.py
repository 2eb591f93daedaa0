"""The rare-event score function on the GPU (csrc/score.hip) and the drivers of iemic.rare_event over
the GPU steppers.

1. k_sqdist2's two sums against exact rational sums, within (n + 3) 2^-52 sum (x - a)^2: one
   rounding of the difference, one of the square or FMA, and any summation order (test_gpu_projected's
   argument); bitwise reproducible; the resident state equals a copy of it;
2. on a grid with land: var = 1 does not see the other variables; two latitude bands;
3. iemic_score_set's refusals by name, scoreGet against NumPy;
4. projGramVV against exactly rounded Gram products;
5. TAMS end to end, projected and in the full space;
6. no preconditioner set-up and no Krylov solve in a projected run; an existing set-up untouched.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from iemic import _lib
from iemic import config as cf
from iemic.rare_event import transient_factory
from iemic.transient import StochasticThetaStepper
from proj_ref import EPS, gram
from test_gpu_projected import basis, bits, solver_calls
from test_gpu_transient import SOLVER, model, run_bands
from test_transient import PARAMS, transient_config

pytestmark = pytest.mark.gpu

_PD = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def Ocean():
    from iemic.ocean import Ocean
    return Ocean


def sqdist2(oc, var, x, a, b):
    L = _lib.lib()
    L.iemic_test_sqdist2.restype = C.c_int
    L.iemic_test_sqdist2.argtypes = [C.c_void_p, C.c_int, _PD, _PD, _PD, _PD]
    out = np.zeros(2)
    vs = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (x, a, b)]
    _lib.check(L.iemic_test_sqdist2(oc._h, var, None if vs[0] is None else _lib.ptr(vs[0]), _lib.ptr(vs[1]),
                                    _lib.ptr(vs[2]), _lib.ptr(out)), "iemic_test_sqdist2")
    return out


def exact_sq(x, a, rows):
    """sum over rows of (x - a)^2, exactly"""
    return sum((Fraction(float(p)) - Fraction(float(q))) ** 2 for p, q in zip(x[rows], a[rows]))


def rows_of(N, var):
    return slice(None) if var < 0 else slice(var, N, 6)


def within(got, want: Fraction, n):
    """|got - want| <= (n + 3) 2^-52 want, in exact arithmetic"""
    return abs(Fraction(float(got)) - want) <= (n + 3) * Fraction(2) ** -52 * want


# ---- 1. the two sums ----------------------------------------------------------------------------------
@pytest.mark.parametrize("var", [-1, 0, 1, 5])
def test_sqdist2_against_exact_sums(Ocean, var):
    """test6x6x4: 864 rows, 144 cells: fewer entries than one pass of the grid, a last block with a
    partial wave (864 = 3 * 256 + 96; 144 < 256), and rows no thread beyond the count may touch"""
    c, oc, L = model(Ocean, "test6x6x4")
    N = c.nrows
    assert N == 864
    rng = np.random.default_rng(100 + var)
    x, a, b = rng.standard_normal((3, N)) * np.array([[1.0], [3.0], [0.25]])
    rows = rows_of(N, var)
    n = len(x[rows])
    got = sqdist2(oc, var, x, a, b)
    for g, ref in zip(got, (a, b)):
        want = exact_sq(x, ref, rows)
        print(f"var {var}: {g!r}, err / bound {float(abs(Fraction(float(g)) - want) / ((n + 3) * Fraction(2) ** -52 * want)):.3f}")
        assert within(g, want, n)
    assert np.array_equal(bits(sqdist2(oc, var, x, a, b)), bits(got))
    # the resident state (x = NULL) is the same as a copy of it
    oc.setState(x)
    assert np.array_equal(bits(sqdist2(oc, var, None, a, b)), bits(got))
    # through the public entry points: d = sqrt(sum) / nrm, dist in the documented order
    oc.scoreSet(a, b, None, var)
    nrm, f = oc.scoreGet()
    s12 = sqdist2(oc, var, a, b, b)[0]
    assert nrm == math.sqrt(s12) and f == 0.5
    dist, d1, d2 = oc.score()
    assert d1 == math.sqrt(got[0]) / nrm and d2 == math.sqrt(got[1]) / nrm
    assert dist == f - f * math.exp(-0.5 * (d1 / 0.25) ** 2.) + (1.0 - f) * math.exp(-0.5 * (d2 / 0.25) ** 2.)
    v = oc.vec_ops().from_host(x)
    assert oc.score(v) == (dist, d1, d2) and oc.score(oc.vec_ops().state()) == (dist, d1, d2)
    oc.scoreSet(a, b, x, var)
    assert oc.scoreGet() == (nrm, math.sqrt(sqdist2(oc, var, a, b, x)[1]) / nrm)
    oc.close()


# ---- 2. land, and two bands -------------------------------------------------------------------------------
def test_ocean_score_ignores_the_other_variables(Ocean):
    c, oc, L = model(Ocean, "natl8")
    N = c.nrows
    land = L[1:c.l + 1, 1:c.m + 1, 1:c.n + 1].reshape(-1) != 0
    assert land.any() and not land.all()
    rng = np.random.default_rng(7)
    s1, s2, s3, x = rng.standard_normal((4, N))        # land rows too: the reference's loop counts them
    oc.scoreSet(s1, s2, s3, 1)
    oc.setState(x)
    ref = oc.score()
    y = x + rng.standard_normal(N)
    y[1::6] = x[1::6]
    oc.setState(y)
    assert oc.score() == ref
    v = rng.standard_normal(N // 6)
    z = x.copy()
    z[1::6] += np.where(land, v, 0.0)                  # v on land cells alone does move it
    oc.setState(z)
    assert oc.score() != ref
    nrm = np.linalg.norm((s1 - s2)[1::6])
    got = oc.scoreGet()
    tol = (N // 6 + 3) * EPS                           # the sums' bound; the roots halve it
    assert abs(got[0] - nrm) <= tol * nrm and abs(got[1] - np.linalg.norm((s1 - s3)[1::6]) / nrm) <= 2 * tol * got[1]
    oc.close()


@pytest.mark.parametrize("var", [-1, 1])
def test_two_latitude_bands(Ocean, var):
    c = cf.preset("natl8")
    L0 = cf.landmask(c)
    N = c.nrows
    x, a, b = np.random.default_rng(8).standard_normal((3, N))

    def run(r, group):
        oc = Ocean(c, landm=L0, local_group=group, rank=r, nranks=2, npx=1)
        oc.setState(x)
        out = sqdist2(oc, var, None, a, b)
        oc.scoreSet(a, b, None, var)
        sc = oc.score()
        oc.close()
        return dict(out=out, sc=sc)

    res = run_bands(2, run)
    rows = rows_of(N, var)
    n = len(x[rows])
    for r in res:
        for g, ref in zip(r["out"], (a, b)):
            assert within(g, exact_sq(x, ref, rows), n)
    assert np.array_equal(bits(res[0]["out"]), bits(res[1]["out"])) and res[0]["sc"] == res[1]["sc"]


# ---- 3. refusals -------------------------------------------------------------------------------------------
def test_score_refusals_by_name(Ocean):
    c, oc, L = model(Ocean, "natl8")
    N = c.nrows
    s1, s2 = np.random.default_rng(9).standard_normal((2, N))
    for fn in (oc.score, oc.scoreGet):
        with pytest.raises(_lib.IemicError, match=r"rc=-71.*no score function set \(iemic_score_set\)"):
            fn()
    with pytest.raises(_lib.IemicError, match=r"rc=-34.*sol1 and sol2 coincide"):
        oc.scoreSet(s1, s1)
    same_v = s1 + 1.0
    same_v[1::6] = s1[1::6]
    with pytest.raises(_lib.IemicError, match=r"rc=-34.*coincide"):
        oc.scoreSet(s1, same_v, None, 1)               # they differ, but not on the v rows
    oc.scoreSet(s1, same_v, None, -1)
    for k, name in enumerate(("sol1", "sol2", "sol3")):
        vs = [s1.copy(), s2.copy(), s1 + s2]
        vs[k][11] = np.nan if k != 1 else np.inf
        with pytest.raises(_lib.IemicError, match=rf"rc=-22.*{name}\[11\] is not finite"):
            oc.scoreSet(*vs)
    for var in (-2, 6):
        with pytest.raises(_lib.IemicError, match=r"rc=-22.*var = "):
            oc.scoreSet(s1, s2, None, var)
    with pytest.raises(_lib.IemicError, match="sol2 has 5 entries"):
        oc.scoreSet(s1, s2[:5])
    with pytest.raises(_lib.IemicError, match=r"rc=-71.*no score function set"):
        oc.score()                                     # a refused set leaves none behind
    oc.scoreSet(s1, s2)
    oc.scoreClear()
    with pytest.raises(_lib.IemicError, match=r"rc=-71"):
        oc.score()
    with pytest.raises(_lib.IemicError, match=r"rc=-71.*iemic_proj_gram_vv: no basis set"):
        oc.projGramVV()
    oc.close()


# ---- 4. the projected scores' Gram matrices ------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 5])
def test_proj_gram_vv(Ocean, k):
    c, oc, L = model(Ocean, "natl8")
    N = c.nrows
    V = basis(N, k, seed=20 + k) * np.array([1.0, 3.0, 0.5, 2.0, 1.5][:k])
    if k > 1:
        V[:, 1] += 0.5 * V[:, 0]
    oc.projSetBasis(V)
    for var in (-1, 1):
        d = None
        if var >= 0:
            d = np.zeros(N)
            d[var::6] = 1.0
        want, scale = gram(V, V, d)
        got = oc.projGramVV(var)
        assert got.shape == (k, k) and np.all(np.abs(got - want) <= N * EPS * scale), var
        assert np.array_equal(bits(oc.projGramVV(var)), bits(got))
        assert np.max(np.abs(got - np.eye(k))) > 0.1   # not orthonormal
    with pytest.raises(_lib.IemicError, match=r"rc=-22.*var = 6"):
        oc.projGramVV(6)
    oc.close()


# ---- 5. end to end -------------------------------------------------------------------------------------------
DT = 1.0e-3
STEP = {k: v for k, v in PARAMS.items() if k != "maximum time (in y)"}
# sigma = 20 and seed 6: with the model's own noise level the four trajectories stay so close that an
# eliminated one only ever copies a donor's whole list and no time is left to step; at this level (found
# by trying 0.5 .. 20 with seeds 5 and 6 on the GPU) both runs restart from a stored snapshot and step on
RARE = dict(STEP, **{"time step": DT, "maximum time": 5.5 * DT, "sigma": 20.0, "dof": 1, "method": "TAMS",
                     "number of experiments": 4, "maximum iterations": 3, "distance tolerance": 0.0005,
                     "adaptive time steps": False})


def record(Ocean):
    """one noisy trajectory of eight steps from rest on test_oceantransient.xml's model: sol1 is rest,
    sol2 its end, and the basis spans its states after 2, 5 and 8 steps (orthonormalised, so that
    the restriction of a state in the span is its coordinate vector and scores move)"""
    c = transient_config()
    oc = Ocean(c, solver_params=SOLVER)
    st = StochasticThetaStepper(oc, {k: v for k, v in dict(STEP, **{"sigma": 0.5, "noise seed": 77}).items()})
    ops = oc.vec_ops()
    x = ops.from_host(np.zeros(c.nrows))
    states = []
    for _ in range(8):
        x = st.step(x, DT)
        states.append(ops.to_host(x).copy())
    oc.close()
    V = np.linalg.qr(np.stack([states[1], states[4], states[7]], axis=1))[0]
    return c, np.zeros(c.nrows), states[7], V


@pytest.fixture(scope="module")
def recorded(Ocean):
    return record(Ocean)


def tams(Ocean, recorded, projected, seed=6, budget=8.0):
    c, sol1, sol2, V = recorded
    oc = Ocean(c, solver_params=SOLVER)
    p = dict(RARE, **{"ams seed": seed, "noise seed": seed, "snapshot device memory (GB)": budget})
    tr = transient_factory(oc, p, sol1, sol2, None, V if projected else None)
    calls0 = solver_calls(oc)
    assert tr.run() == 0
    return oc, tr, calls0


def check_run(tr):
    e = tr.experiments
    conv = sum(x.converged for x in e)
    print("ell", tr.ell, "its", tr.its, "converged", conv, "steps", tr.time_steps, "p", tr.probability,
          "max", [round(x.max_distance, 4) for x in e], "len", [len(x.xlist) for x in e])
    # it did something: an elimination with a branch, and recorded trajectories
    assert tr.its >= 1 and len(tr.ell) == tr.its and not tr.extinct
    assert max(len(x.xlist) for x in e) > 1
    alpha = conv / 4
    for l in tr.ell:
        alpha *= 1.0 - l / 4
    assert tr.probability == alpha
    assert tr.time_steps == tr.stepper.draws and tr.time_steps > 4 * 5      # steps after a branch
    ts = [0.0]
    for _ in range(6):
        ts.append(ts[-1] + tr.dt)
    for x in e:
        assert len(x.xlist) == len(x.dlist) == len(x.tlist) and all(t in ts for t in x.tlist)
        assert x.tlist == sorted(set(x.tlist)) and x.time == x.tlist[-1]
        d = x.dlist if not x.converged else x.dlist[:-1]
        assert all(q > p + tr.dist_tol for p, q in zip(d, d[1:]))
        # (an unconverged one keeps its own level when a donor's whole list was copied and no time is left)
        assert (x.dlist[-1] == 1.0 and x.max_distance == 1.0) if x.converged else x.max_distance < 1.0
        # every stored snapshot scores what the list says; TAMS records the start as 0 without scoring
        # it and a converged entry as 1
        for s, dist, t in zip(x.xlist, x.dlist, x.tlist):
            if t != 0 and dist != 1.0:
                assert tr.dist_fun(s) == dist


def same_runs(a, b):
    assert a.ell == b.ell and a.its == b.its and a.probability == b.probability and a.time_steps == b.time_steps
    for x, y in zip(a.experiments, b.experiments):
        assert (x.dlist, x.tlist, x.max_distance, x.time, x.converged) == (y.dlist, y.tlist, y.max_distance, y.time,
                                                                           y.converged)
        for s, t in zip(x.xlist, y.xlist):
            assert np.array_equal(bits(a.states.to_host(s)), bits(b.states.to_host(t)))


def test_tams_projected(Ocean, recorded):
    oc, tr, calls0 = tams(Ocean, recorded, True)
    check_run(tr)
    assert tr.vector_length == 3 and all(isinstance(s, np.ndarray) and s.shape == (3,) for x in tr.experiments for s in x.xlist)
    # 6. nothing set up a preconditioner or ran a Krylov solver
    assert solver_calls(oc) == calls0 == (0, 0) and oc.active_cells() == 0
    oc2, tr2, _ = tams(Ocean, recorded, True)
    same_runs(tr, tr2)
    oc.close()
    oc2.close()


def test_tams_full_space(Ocean, recorded):
    oc, tr, _ = tams(Ocean, recorded, False)
    check_run(tr)
    assert tr.vector_length == recorded[0].nrows and tr.states.on_host == 0 and tr.states.live > 0
    oc2, tr2, _ = tams(Ocean, recorded, False)
    same_runs(tr, tr2)
    # no room on the device: the snapshots go to the host and come back when branched from
    oc3, tr3, _ = tams(Ocean, recorded, False, budget=0.0)
    assert tr3.states.live == 0 and tr3.states.on_host > 0
    assert all(isinstance(s, np.ndarray) for x in tr3.experiments for s in x.xlist)
    same_runs(tr, tr3)
    for o in (oc, oc2, oc3):
        o.close()


def test_projected_run_leaves_a_preconditioner_as_it_is(Ocean, recorded):
    c, sol1, sol2, V = recorded
    oc = Ocean(c, solver_params=SOLVER)
    L = oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    oc.setState(cf.synthetic_state(c, L, amp_ts=1e-3))
    oc.preProcess()
    oc.thetaInitStep(1e-3, 0.75)
    oc.thetaNewtonStep()
    assert solver_calls(oc) == (1, 1)
    x = oc.getState().copy()
    z = oc.applyPrecon(x).copy()
    tr = transient_factory(oc, dict(RARE, **{"ams seed": 5, "noise seed": 5}), sol1, sol2, None, V)
    assert tr.run() == 0
    assert solver_calls(oc) == (1, 1)
    assert np.array_equal(bits(oc.applyPrecon(x)), bits(z))
    oc.close()


def test_factory_picks_the_ocean_scores(Ocean, recorded):
    """params["dof"] == 6: the v rows alone, on the device and projected"""
    c, sol1, sol2, V = recorded
    oc = Ocean(c, solver_params=SOLVER)
    nv = c.nrows // 6
    nrm = np.linalg.norm((sol1 - sol2)[1::6])
    p = dict(RARE, **{"dof": 6, "ams seed": 5, "noise seed": 5})
    full = transient_factory(oc, p, sol1, sol2)
    assert full.dist_fun.nrm == oc.scoreGet()[0] and full.dist_fun.dist_factor == 0.5
    assert abs(full.dist_fun.nrm - nrm) <= (nv + 3) * EPS * nrm
    at_b = 0.5 - 0.5 * math.exp(-0.5 * (1.0 / 0.25) ** 2.) + 0.5
    assert abs(full.dist_fun(sol2) - at_b) <= 1e-12 and full.dist_fun(full.x0) == full.dist_fun(sol1)
    proj = transient_factory(oc, p, sol1, sol2, None, V)
    M = oc.projGramVV(1)
    y2 = V.T @ sol2
    # the restriction's rounding: N 2^-52 sum |V| |x| <= N^1.5 2^-52 |x| = 1.3e-11 |x|
    assert abs(proj.dist_fun.nrm - math.sqrt(y2 @ M @ y2)) <= 1e-10 * proj.dist_fun.nrm
    assert abs(proj.dist_fun.nrm - np.linalg.norm((V @ y2)[1::6])) <= 1e-10 * proj.dist_fun.nrm
    assert proj.vector_length == 3 and not np.any(proj.x0)
    oc.close()
