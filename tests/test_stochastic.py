"""The stochastic theta model on the CPU: iemic.transient.StochasticThetaStepper on a twin of the
GPU model, the NumPy restatement of the forcing column pinned to the oracle, the noise
generator, and the refusals.

The twin (tests/stoch_ref.py) is test_transient.py's TwinModel with StochasticThetaModel's
initStep and residual (StochasticThetaModel.H:52-83) in NumPy.  Its forcing column is a
restatement of forcing.F90:106-189, which tests/test_gpu_stochastic.py compares with the device
bit for bit; so that this is not the code compared with itself, the column's ocean entries are
pinned here to the oracle's residual, which was written without it: with SPER = 0 the forcing is
the only term of a surface S row that depends on SALT (gamma = COMB SALT (1 - SRES + SRES BIOT)
multiplies all of it and nothing else), so F(SALT = 0) - F(SALT = s) on those rows is the column
at SALT = s.  Measured here: the identity holds to 1 ulp of the larger residual on natl8 (SRES =
0) and on gateway16 (SRES = 1: the restoring term of the matrix carries BIOT but not SALT).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import iemic
from iemic import config as cf
from iemic.config import PAR_INDEX
from iemic.transient import StochasticThetaStepper, ThetaStepper
from stoch_ref import StochasticTwin, forcing_column, forcing_triple, noise, surface_rows
from test_transient import PARAMS, TABLE, transient_config

# noise level and seed of the three-step runs (also tests/test_gpu_stochastic.py's device run)
SIGMA, SEED = 0.5, 20261021


def test_lazy_export():
    assert iemic.StochasticThetaStepper is StochasticThetaStepper
    assert issubclass(StochasticThetaStepper, ThetaStepper)


# ---- the twin ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sigma0_run(oracle_lib):
    m = StochasticTwin(oracle_lib, transient_config())
    st = StochasticThetaStepper(m, dict(PARAMS, **{"sigma": 0.0, "noise seed": 3}))
    return m, st, st.run()


def test_sigma_zero_is_the_deterministic_table(sigma0_run):
    m, st, status = sigma0_run
    assert status == 0
    assert [r.dt for r in st.history] == [t[0] for t in TABLE]
    assert [r.newton_steps for r in st.history] == [t[1] for t in TABLE]
    for r, t in zip(st.history, TABLE):
        assert abs(r.norm_x - t[2]) <= 1e-7, (r.step, r.norm_x, t[2])      # test_transient.py's bound
    assert st.draws == 10 and len(m.steps_seen) == 10 and st.noise_seed == 3


def three_steps(orc, seed, sigma=SIGMA):
    m = StochasticTwin(orc, transient_config())
    st = StochasticThetaStepper(m, dict(PARAMS, **{"sigma": sigma, "noise seed": seed,
                                                   "number of time steps": 3}))
    assert st.run() == 0
    return m, st


@pytest.fixture(scope="module")
def noisy_runs(oracle_lib):
    """The twin's linear solver (the oracle's FGMRES) sums with OpenMP, so two of its runs differ
    in the last bits (1e-15 seen here) unless it runs on one thread; bitwise-identical histories
    are asked of the stepper and its noise, so the three runs take one thread."""
    gomp = C.CDLL("libgomp.so.1")
    nthreads = gomp.omp_get_max_threads()
    gomp.omp_set_num_threads(1)
    try:
        return three_steps(oracle_lib, SEED), three_steps(oracle_lib, SEED), three_steps(oracle_lib, SEED + 1)
    finally:
        gomp.omp_set_num_threads(nthreads)


def test_fixed_seed_reproduces_and_seeds_differ(noisy_runs):
    (ma, a), (mb, b), (mc, c) = noisy_runs
    for r in a.history:
        print(f"step {r.step} dt {r.dt:g} steps() {r.newton_steps} |x| {r.norm_x:.12f}")
    assert a.history == b.history
    assert np.array_equal(ma.getState(), mb.getState())
    assert a.draws == 3 + len(a.rejected)
    assert a.history[0].norm_x != c.history[0].norm_x
    # the noise moved the state: the deterministic first step ends within 1e-7 of TABLE[0]'s norm
    assert abs(a.history[0].norm_x - TABLE[0][2]) > 1e-5


def test_noise_lives_on_surface_salinity_rows_of_ocean_cells(oracle_lib):
    c = transient_config()
    m = StochasticTwin(oracle_lib, c)
    assert m.o.rowintcon >= 0
    pert = StochasticThetaStepper.noise_block(5, 0, c.m)
    m.stochasticInitStep(1e-3, 0.75, 1.0, pert)
    land = m.land_top().reshape(-1) != 0
    rows = surface_rows(c).reshape(-1)
    assert land.any() and not m.hit[rows[land]].any() and not m.hit[m.o.rowintcon]
    assert m.hit.sum() == (~land).sum() - 1 and np.all(m.hit[rows[~land & (rows != m.o.rowintcon)]])
    assert np.all(m.G[~m.hit] == 0) and np.all(m.G[m.hit] != 0)
    B = m.o.jacobian(m.x)[1]
    with_noise, G, hit = m._ftheta(B), m.G, m.hit
    m.thetaInitStep(1e-3, 0.75)                                            # disarms
    plain = m._ftheta(B)
    assert m.G is None
    assert np.array_equal(with_noise[~hit].view(np.int64), plain[~hit].view(np.int64))
    assert np.array_equal(with_noise[hit], plain[hit] + G[hit])


# ---- the forcing column against the oracle ---------------------------------------------------
@pytest.mark.parametrize("name", ["natl8", "gateway16"])
def test_forcing_column_pinned_to_the_oracle(oracle_lib, name):
    """natl8: SRES = 0, what the issue asks for; gateway16 (SRES = 1) holds as well."""
    c = cf.preset(name)
    m = StochasticTwin(oracle_lib, c)
    if name == "natl8":
        assert c.sres == 0 and m.o.rowintcon >= 0
    assert m.o.get_par(PAR_INDEX["Salinity Perturbation"]) == 0.0
    par = m.par()
    s = par["Salinity Forcing"]
    assert s != 0.0
    coF = forcing_column(c, m.land_top(), par)
    x = cf.synthetic_state(c, m.L)
    Fs = m.o.rhs(x)
    m.o.set_par(PAR_INDEX["Salinity Forcing"], 0.0)
    F0 = m.o.rhs(x)
    m.o.set_par(PAR_INDEX["Salinity Forcing"], s)
    rows = surface_rows(c)
    ocean = (m.land_top() == 0) & (rows != m.o.rowintcon)
    r = rows[ocean]
    gap = np.abs((F0[r] - Fs[r]) - coF[ocean])
    ulp = np.spacing(np.maximum(np.abs(F0[r]), np.abs(Fs[r])))
    print(f"{name}: {r.size} ocean entries, max gap {gap.max():.3e} = {np.max(gap / ulp):.2f} ulp of the "
          f"residuals, max |coF| {np.abs(coF[ocean]).max():.3e}")
    assert np.abs(coF[ocean]).max() > 1e-3
    # each residual is rounded to half an ulp and so is their difference: 2 ulp of the larger
    assert np.all(gap <= 2 * ulp)
    # nothing else of F moved with SALT
    other = np.ones(c.nrows, dtype=bool)
    other[rows.reshape(-1)] = False
    assert np.array_equal(F0[other], Fs[other])


def test_forcing_triple_shape():
    c = cf.preset("natl8")
    coF = np.arange(1.0, c.n * c.m + 1).reshape(c.m, c.n)
    ric = int(surface_rows(c)[c.m - 1, c.n - 1])
    rows, cols, vals = forcing_triple(c, coF, ric)
    assert rows.size == c.n * c.m - 1 and np.all(np.diff(rows) > 0) and ric not in rows
    assert rows[0] == 6 * ((c.l - 1) * c.m * c.n) + 5 and cols[0] == 0 and cols[-1] == c.m - 1
    assert np.array_equal(vals, coF.reshape(-1)[:-1])
    G, hit = noise(c, coF, np.zeros((c.m, c.n), dtype=int), ric, 0.25, 2.0, np.ones(c.m))
    assert hit.sum() == rows.size and np.array_equal(G[rows], 1.0 * vals)      # sqrt(0.25) * 2 = 1


# ---- the generator ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 20261021, 2**63 + 12345])
def test_generator_moments(seed):
    """10^5 standard normals in blocks of m = 8: the mean of N has standard deviation 1 / sqrt(N)
    and the sample variance sqrt(2 / N); five of each"""
    m, nb = 8, 12500
    v = np.concatenate([StochasticThetaStepper.noise_block(seed, b, m) for b in range(nb)])
    N = v.size
    assert N == 100000
    print(f"seed {seed}: mean {v.mean():+.3e} (bound {5 / np.sqrt(N):.3e}), "
          f"variance - 1 {v.var() - 1:+.3e} (bound {5 * np.sqrt(2 / N):.3e})")
    assert abs(v.mean()) <= 5 / np.sqrt(N)
    assert abs(v.var() - 1) <= 5 * np.sqrt(2 / N)


class ScriptedStochastic:
    """Converges in the first Newton iteration of every time step but those listed in `fail`
    (indices of stochasticInitStep calls)."""

    def __init__(self, m=8, fail=()):
        self.cfg = SimpleNamespace(m=m)
        self.fail = set(fail)
        self.inits = []

    def preProcess(self):
        pass

    def stochasticInitStep(self, dt, theta, sigma, pert):
        self.inits.append((dt, theta, sigma, np.array(pert)))

    def thetaNewtonStep(self):
        bad = (len(self.inits) - 1) in self.fail
        return SimpleNamespace(norm_dx=1.0 if bad else 1e-9, norm_f1=1.0 if bad else 1e-9)

    def thetaRestore(self):
        pass

    def getState(self):
        return np.ones(4)


def test_blocks_depend_on_seed_and_index_alone():
    seed, m = 77, 8
    a = StochasticThetaStepper.noise_block(seed, 5, m)
    assert np.array_equal(a, StochasticThetaStepper.noise_block(seed, 5, m))
    assert not np.array_equal(a, StochasticThetaStepper.noise_block(seed, 6, m))
    assert not np.array_equal(a, StochasticThetaStepper.noise_block(seed + 1, 5, m))
    assert not np.array_equal(a[:4], StochasticThetaStepper.noise_block(seed, 5, 4)[::-1])
    mod = ScriptedStochastic(m)
    st = StochasticThetaStepper(mod, dict(PARAMS, **{"noise seed": seed, "number of time steps": 6}))
    assert st.run() == 0 and st.draws == 6
    for b, (_, _, sigma, pert) in enumerate(mod.inits):
        assert sigma == 1.0                                              # the default
        assert np.array_equal(pert, StochasticThetaStepper.noise_block(seed, b, m))
    fresh = StochasticThetaStepper(ScriptedStochastic(m), dict(PARAMS, **{"noise seed": seed}))
    fresh.draws = 5
    assert np.array_equal(fresh._pert(), mod.inits[5][3])


def test_seed_zero_draws_one_and_records_it():
    a = StochasticThetaStepper(ScriptedStochastic(), dict(PARAMS, **{"noise seed": 0}))
    b = StochasticThetaStepper(ScriptedStochastic(), PARAMS)
    assert a.noise_seed > 0 and b.noise_seed > 0 and a.noise_seed != b.noise_seed


def test_rejected_step_draws_again():
    mod = ScriptedStochastic(fail=(1,))
    p = dict(PARAMS, **{"maximum Newton iterations": 1, "number of time steps": 3, "noise seed": 9,
                        "sigma": 0.25})
    st = StochasticThetaStepper(mod, p)
    assert st.run() == 0
    assert len(st.history) == 3 and st.rejected == [2e-3]
    assert st.draws == len(st.history) + len(st.rejected) == len(mod.inits) == 4
    dts = [i[0] for i in mod.inits]
    assert dts == [1e-3, 2e-3, 1e-3, 2e-3]                 # the rejected 2e-3 is halved, then doubles
    assert not np.array_equal(mod.inits[1][3], mod.inits[2][3])
    assert np.array_equal(mod.inits[2][3], StochasticThetaStepper.noise_block(9, 2, 8))
    assert all(i[2] == 0.25 for i in mod.inits)


def test_pert_source_replaces_the_generator():
    seen = []

    def src(block, m):
        seen.append((block, m))
        return np.full(m, float(block))

    mod = ScriptedStochastic(m=5)
    st = StochasticThetaStepper(mod, dict(PARAMS, **{"number of time steps": 2}), pert_source=src)
    assert st.run() == 0 and seen == [(0, 5), (1, 5)]
    assert np.array_equal(mod.inits[1][3], np.ones(5))


# ---- refusals ----------------------------------------------------------------------------------
def test_negative_sigma_refused_by_name():
    with pytest.raises(ValueError, match='"sigma"'):
        StochasticThetaStepper(ScriptedStochastic(), dict(PARAMS, sigma=-1.0))
    with pytest.raises(ValueError, match='"sigma"'):
        StochasticThetaStepper(ScriptedStochastic(), dict(PARAMS, sigma=float("nan")))


def test_nan_pert_refused_by_name():
    def src(block, m):
        v = np.zeros(m)
        v[3] = np.nan
        return v

    mod = ScriptedStochastic()
    st = StochasticThetaStepper(mod, PARAMS, pert_source=src)
    with pytest.raises(ValueError, match=r"pert\[3\] is not finite"):
        st.run()
    assert mod.inits == []


def test_wrong_length_pert_refused_by_name():
    mod = ScriptedStochastic(m=8)
    st = StochasticThetaStepper(mod, PARAMS, pert_source=lambda block, m: np.zeros(m + 1))
    with pytest.raises(ValueError, match="pert has 9 entries"):
        st.run()
    assert mod.inits == []


def test_unknown_parameter_refused():
    with pytest.raises(KeyError, match="noise sed"):
        StochasticThetaStepper(ScriptedStochastic(), dict(PARAMS, **{"noise sed": 1}))
    with pytest.raises(KeyError):
        ThetaStepper(ScriptedStochastic(), dict(PARAMS, sigma=1.0))      # the plain stepper has no noise
