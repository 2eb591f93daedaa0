"""The stochastic theta model on the GPU (csrc/stochastic.hip, iemic.transient).

* the forcing operator (computeForcing / getForcing) is the NumPy restatement of
  forcing.F90:106-189 with SPER = 0 (tests/stoch_ref.py, pinned to the oracle by
  tests/test_stochastic.py) bit for bit, with an inserted emip and with HMTP != 0 too, and
  leaves the model's forcing and SPER alone;
* the residual with noise is ((dt theta) F + (dt (1 - theta)) F_n + B (x_n - x)) + G bit for bit,
  the rows without noise keep the plain residual's bits;
* sigma = 0 and a plain thetaInitStep give the plain residual;
* the fused Newton iteration works on the residual with noise;
* two in-process latitude bands with the same pert give the one-rank residual and operator;
* three steps of StochasticThetaStepper reproduce the CPU twin's run;
* the refusals, by name.
"""
import ctypes as C

import numpy as np
import pytest

from iemic import _lib
from iemic import config as cf
from iemic.config import PAR_INDEX
from iemic.transient import StochasticThetaStepper
from stoch_ref import forcing_column, forcing_triple, noise, surface_rows
from test_gpu_transient import SOLVER, model, run_bands
from test_stochastic import SEED, SIGMA
from test_transient import PARAMS, transient_config

pytestmark = pytest.mark.gpu

# the CPU twin's three steps with sigma = SIGMA, "noise seed" = SEED (tests/test_stochastic.py's
# three_steps on one thread): dt, Newton::steps(), ||x||
TWIN = [(1e-3, 1, 0.410273444042), (2e-3, 2, 1.184316839953), (4e-3, 3, 2.638332234034)]


@pytest.fixture(scope="module")
def Ocean():
    from iemic.ocean import Ocean
    return Ocean


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def land_top(oc, c):
    return oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)[c.l, 1:c.m + 1, 1:c.n + 1]


def restated(oc, c, emip=None, aemip=None):
    par = {name: oc.getPar(name) for name in PAR_INDEX}
    return forcing_column(c, land_top(oc, c), par, emip=emip, aemip=aemip)


@pytest.mark.parametrize("name", ["natl8", "gateway16"])
@pytest.mark.parametrize("variant", ["profile", "emip", "hmtp"])
def test_get_forcing_bitwise(Ocean, name, variant):
    c, oc, L = model(Ocean, name)
    emip = aemip = None
    if variant == "emip":
        emip = np.random.default_rng(7).standard_normal(c.n * c.m)
        oc.setEmip(emip)
    if variant == "hmtp":
        aemip = np.random.default_rng(8).standard_normal(c.n * c.m)
        oc.setEmip(aemip, "A")
        oc.setPar("Salinity Homotopy", 0.3)
    oc.setPar("Salinity Perturbation", 0.25)
    oc.setState(cf.synthetic_state(c, L))
    F = oc.computeRHS().copy()
    oc.computeForcing()
    rows, cols, vals = oc.getForcing()
    want = forcing_triple(c, restated(oc, c, emip, aemip), oc.rowintcon)
    assert rows.dtype == np.int64 and np.array_equal(rows, want[0])
    assert np.array_equal(cols, want[1])
    assert np.array_equal(bits(vals), bits(want[2]))
    assert np.all(np.diff(rows) > 0)
    land = land_top(oc, c).reshape(-1) != 0
    srow = surface_rows(c).reshape(-1)
    if name == "natl8":
        assert oc.rowintcon >= 0 and oc.rowintcon not in rows and rows.size == c.n * c.m - 1
        assert land.any() and np.all(np.isin(srow[land], rows))
        assert np.all(vals[np.isin(rows, srow[land])] != 0)
    else:
        assert oc.rowintcon < 0 and rows.size == c.n * c.m
    # the model's own forcing and SPER are untouched
    assert np.array_equal(bits(oc.computeRHS()), bits(F))
    assert oc.getPar("Salinity Perturbation") == 0.25
    oc.close()


def test_coupled_salinity_gives_an_empty_operator(Ocean):
    oc = Ocean(cf.preset("coupled_natl8s"), analyze_jacobian=False)
    oc.computeForcing()
    rows, cols, vals = oc.getForcing()
    assert rows.size == 0 and cols.size == 0 and vals.size == 0
    oc.close()


def residual_setup(Ocean, name, dt, theta):
    """test_gpu_transient.py's test_theta_residual_bitwise set-up: x_n, x, and the plain residual
    in numpy from F, F_n and B of the same model"""
    c, oc, L = model(Ocean, name)
    xn = cf.synthetic_state(c, L)
    x = xn + 0.25 * cf.synthetic_state(c, L, seed=99)
    oc.setState(xn)
    Fn = oc.computeRHS().copy()
    oc.computeJacobian()
    B = oc.diagB()
    oc.setState(x)
    F = oc.computeRHS().copy()
    plain = (dt * theta) * F + (dt * (1 - theta)) * Fn + B * (xn - x)
    return c, oc, xn, x, plain


@pytest.mark.parametrize("name", ["natl8", "gateway16"])
@pytest.mark.parametrize("dt,theta", [(1e-3, 0.75), (0.128, 1.0)])
@pytest.mark.parametrize("sigma", [1.0, 0.37])
def test_residual_with_noise_bitwise(Ocean, name, dt, theta, sigma):
    c, oc, xn, x, plain = residual_setup(Ocean, name, dt, theta)
    pert = StochasticThetaStepper.noise_block(11, 2, c.m)
    oc.setState(xn)
    oc.stochasticInitStep(dt, theta, sigma, pert)
    oc.setState(x)
    got = oc.thetaRHS().copy()
    G, hit = noise(c, restated(oc, c), land_top(oc, c), oc.rowintcon, dt, sigma, pert)
    # G is added on the rows that carry it and nowhere else: numpy's plain + G over the whole
    # vector would turn the plain residual's -0.0 entries (rows whose every term is a signed
    # zero, such as W rows under the surface) into +0.0, which the model does not do
    want = plain.copy()
    want[hit] = plain[hit] + G[hit]
    bad = np.flatnonzero(bits(got) != bits(want))
    print(f"{name} dt {dt} theta {theta} sigma {sigma}: {hit.sum()} rows with noise, {bad.size} rows differ "
          f"({np.count_nonzero(hit[bad])} of them with noise), -0.0 entries of the plain residual: "
          f"{np.count_nonzero(np.signbit(plain) & (plain == 0))}")
    assert hit.sum() > 0 and np.all(G[hit] != 0) and not np.any(G[~hit])
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(got, plain + G)               # and as values (-0.0 == +0.0) the full sum
    assert np.array_equal(bits(got[~hit]), bits(plain[~hit]))
    assert np.all(got[hit] != plain[hit])
    # land and integral-condition rows carry no noise
    srow = surface_rows(c).reshape(-1)
    land = srow[land_top(oc, c).reshape(-1) != 0]
    assert not hit[land].any() and np.array_equal(bits(got[land]), bits(plain[land]))
    if name == "natl8":
        assert oc.rowintcon >= 0 and not hit[oc.rowintcon]
        assert bits(got[oc.rowintcon:oc.rowintcon + 1])[0] == bits(plain[oc.rowintcon:oc.rowintcon + 1])[0]
    assert set(np.flatnonzero(hit) % 6) == {5}
    oc.close()


@pytest.mark.parametrize("name", ["natl8", "gateway16"])
def test_sigma_zero_and_disarming(Ocean, name):
    dt, theta = 1e-3, 0.75
    c, oc, xn, x, plain = residual_setup(Ocean, name, dt, theta)
    pert = StochasticThetaStepper.noise_block(11, 3, c.m)
    oc.setState(xn)
    oc.thetaInitStep(dt, theta)
    oc.setState(x)
    ref = oc.thetaRHS().copy()
    assert np.array_equal(bits(ref), bits(plain))
    oc.setState(xn)
    oc.stochasticInitStep(dt, theta, 0.0, pert)
    oc.setState(x)
    assert np.array_equal(bits(oc.thetaRHS()), bits(ref))
    oc.setState(xn)
    oc.stochasticInitStep(dt, theta, 1.0, pert)
    oc.setState(x)
    assert not np.array_equal(bits(oc.thetaRHS()), bits(ref))
    oc.setState(xn)
    oc.thetaInitStep(dt, theta)                       # a plain step disarms the noise
    oc.setState(x)
    assert np.array_equal(bits(oc.thetaRHS()), bits(ref))
    oc.close()


def test_changed_forcing_is_picked_up(Ocean):
    """the operator is computed again when the forcing changed since the last compute"""
    dt, theta = 1e-3, 0.75
    c, oc, L = model(Ocean, "natl8")
    pert = np.ones(c.m)
    x = cf.synthetic_state(c, L)
    oc.setState(x)
    oc.stochasticInitStep(dt, theta, 1.0, pert)
    a = oc.thetaRHS().copy()
    oc.setPar("Salinity Forcing", 2.0 * oc.getPar("Salinity Forcing"))
    oc.stochasticInitStep(dt, theta, 1.0, pert)
    b = oc.thetaRHS().copy()
    oc.thetaInitStep(dt, theta)
    plain = oc.thetaRHS().copy()
    G, hit = noise(c, restated(oc, c), land_top(oc, c), oc.rowintcon, dt, 1.0, pert)
    want = plain.copy()
    want[hit] = plain[hit] + G[hit]
    assert np.array_equal(bits(b), bits(want))
    assert not np.array_equal(a[hit], b[hit])
    oc.close()


def test_fused_step_sees_the_noise(Ocean):
    dt, theta = 1e-3, 0.75
    c = transient_config()
    a, b = Ocean(c, solver_params=SOLVER), Ocean(c, solver_params=SOLVER)
    L = a.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    x = cf.synthetic_state(c, L, amp_ts=1e-3)
    pert = StochasticThetaStepper.noise_block(11, 4, c.m)
    for oc in (a, b):
        oc.setState(x)
        oc.preProcess()
    a.stochasticInitStep(dt, theta, 1.0, pert)
    b.thetaInitStep(dt, theta)
    f0 = a.thetaRHS().copy()
    assert not np.array_equal(bits(f0), bits(b.thetaRHS()))
    ia, ib = a.thetaNewtonStep(), b.thetaNewtonStep()
    assert ia.solve.converged == 1 and ib.solve.converged == 1
    # test_fused_step_equals_composed's tolerance
    assert abs(ia.norm_f0 - np.linalg.norm(f0)) <= 1e-10 * np.linalg.norm(f0)
    xa, xb = a.getState(), b.getState()
    d = np.abs(xa - xb).reshape(-1, 6)
    print(f"|F0| with noise {ia.norm_f0:.6e}, without {ib.norm_f0:.6e}; max state gap on S rows {d[:, 5].max():.3e}")
    assert ia.norm_f0 != ib.norm_f0
    assert d[:, 5].max() > 1e-6 * np.abs(xb).max()
    a.close()
    b.close()


def test_rank_independence(Ocean):
    """natl8 as two in-process latitude bands with the same pert: the residual gathered from the
    bands is the one-rank residual bit for bit, and the operators concatenate to the one-rank one."""
    dt, theta, sigma = 1e-3, 0.75, 1.0
    c = transient_config()
    pert = StochasticThetaStepper.noise_block(11, 5, c.m)
    one = Ocean(c, solver_params=SOLVER)
    L0 = cf.landmask(c)
    L = one.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    xn = cf.synthetic_state(c, L, amp_ts=1e-3)
    x = xn + 0.25 * cf.synthetic_state(c, L, seed=99, amp_ts=1e-3)
    one.setState(xn)
    one.stochasticInitStep(dt, theta, sigma, pert)
    one.setState(x)
    ref = one.thetaRHS().copy()
    one.thetaInitStep(dt, theta)
    assert not np.array_equal(bits(one.thetaRHS()), bits(ref))
    one.computeForcing()
    triple = one.getForcing()
    one.close()

    def fn(r, group):
        oc = Ocean(c, landm=L0, local_group=group, rank=r, nranks=2, npx=1, solver_params=SOLVER)
        oc.setState(xn)
        oc.stochasticInitStep(dt, theta, sigma, pert)
        oc.setState(x)
        f = oc.thetaRHS().copy()
        oc.computeForcing()
        t = oc.getForcing()
        rows = oc.owned_rows()
        oc.close()
        return dict(f=f, rows=rows, triple=t)

    res = run_bands(2, fn)
    got = np.full(c.nrows, np.nan)
    for r in res:
        got[r["rows"]] = r["f"][r["rows"]]
    assert np.array_equal(bits(got), bits(ref))
    for q in range(3):
        cat = np.concatenate([r["triple"][q] for r in res])
        assert cat.dtype == triple[q].dtype and np.array_equal(cat.view(np.int64 if q != 1 else np.int32),
                                                               triple[q].view(np.int64 if q != 1 else np.int32))
    assert all(r["triple"][0].size > 0 for r in res)


def test_stepper_on_the_device(Ocean):
    """Three steps of StochasticThetaStepper from rest on test_oceantransient.xml's model with
    sigma = 0.5, where the twin's Newton runs still converge in 1, 2 and 3 steps (TWIN above, from
    tests/test_stochastic.py's run).  Same dt sequence and Newton counts; the norms within 1e-7,
    the gap test_gpu_transient.py's test_trns_ocean allows between the device and the twin's table
    for the noise-free run."""
    c = transient_config()
    oc = Ocean(c, solver_params=SOLVER)
    oc.setState(np.zeros(c.nrows))
    st = StochasticThetaStepper(oc, dict(PARAMS, **{"sigma": SIGMA, "noise seed": SEED,
                                                   "number of time steps": 3}))
    status = st.run()
    for r, t in zip(st.history, TWIN):
        print(f"step {r.step} dt {r.dt:g} steps() {r.newton_steps} |x| {r.norm_x:.12f} twin {t[2]:.12f} "
              f"diff {r.norm_x - t[2]:+.2e}")
    assert status == 0 and st.rejected == [] and st.draws == 3
    assert [r.dt for r in st.history] == [t[0] for t in TWIN]
    assert [r.newton_steps for r in st.history] == [t[1] for t in TWIN]
    for r, t in zip(st.history, TWIN):
        assert abs(r.norm_x - t[2]) <= 1e-7, (r.step, r.norm_x, t[2])
    oc.close()


def test_refusals_by_name(Ocean):
    c, oc, L = model(Ocean, "natl8")
    lib = _lib.lib()
    nnz = C.c_int64(-1)
    assert lib.iemic_forcing_export(oc._h, None, None, None, C.byref(nnz)) == -71        # IEMIC_ESTATE
    assert b"iemic_forcing_compute" in lib.iemic_last_error()
    with pytest.raises(_lib.IemicError, match=r"rc=-71.*iemic_forcing_compute"):
        oc.getForcing()
    assert lib.iemic_theta_init_step_noise(oc._h, 1e-3, 0.75, 1.0, None) == -22          # IEMIC_EINVAL
    assert b"pert" in lib.iemic_last_error()
    good = np.zeros(c.m)
    bad = good.copy()
    bad[2] = np.nan
    for sigma, pert, word in ((-1.0, good, "sigma"), (float("nan"), good, "sigma"), (float("inf"), good, "sigma"),
                              (1.0, bad, r"pert\[2\]")):
        with pytest.raises(_lib.IemicError, match=rf"rc=-22.*{word}"):
            oc.stochasticInitStep(1e-3, 0.75, sigma, pert)
    with pytest.raises(_lib.IemicError, match="pert has 7 entries"):
        oc.stochasticInitStep(1e-3, 0.75, 1.0, np.zeros(c.m - 1))
    for dt, theta, word in ((1e-3, 0.0, "theta"), (0.0, 0.75, "dt")):
        with pytest.raises(_lib.IemicError, match=rf"rc=-22.*{word}"):
            oc.stochasticInitStep(dt, theta, 1.0, good)
    # nothing was initialised by the refused calls
    with pytest.raises(_lib.IemicError, match=r"rc=-71.*iemic_theta_init_step"):
        oc.thetaRHS()
    oc.close()
