"""Surface fluxes (THCM::getFluxes), the HDF5 flux groups and inserted forcing fields.

The pin is the reference's own fixture tests/golden/ocean_reference.h5: its SalinityFlux,
TemperatureFlux and SensibleHeatFlux were computed by the reference's Fortran
(probe.F90:200-355) at the state the file holds.  Bound 1e-12 * max|group|: about ten flops
per cell plus the 256-term correction sum (256 eps ~ 6e-14), and the largest cancellation,
Biot * S / gamma ~ 4915 S against ~10 giving ~0.28, costs about two more digits.

The coupled branches and an inserted emip are pinned by tests/golden/flux_*.npz, recorded
from the reference's Fortran by tests/golden/make_golden_flux.py; same bound, same reasoning.
"""
import math
import os
import threading

import numpy as np
import pytest

from helpers import GOLDEN, golden, golden_landm
from iemic import config as cf
from iemic import h5

REF_H5 = os.path.join(GOLDEN, "ocean_reference.h5")
PINNED = ("SalinityFlux", "TemperatureFlux", "SensibleHeatFlux")
ZERO = ("OceanAtmosSalFlux", "OceanSeaIceSalFlux", "ShortwaveFlux", "LatentHeatFlux", "SeaIceHeatFlux")
ORDER = ("SalinityFlux", "OceanAtmosSalFlux", "OceanSeaIceSalFlux", "TemperatureFlux", "ShortwaveFlux",
         "SensibleHeatFlux", "LatentHeatFlux", "SeaIceHeatFlux", "SeaIceMask")
gpu = pytest.mark.gpu


def fixture():
    return {k: np.asarray(v) for k, (v, _) in h5.read(REF_H5).items()}


def check_group(name, got, want):
    gap = float(np.max(np.abs(got - want)))
    bound = 1e-12 * float(np.max(np.abs(want)))
    print(f"{name}: max gap {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound, (name, gap, bound)


# ---- numpy restatement of the ocean-only formulas ------------------------------------
def qint(field, cos_y, wet):
    """forcing.F90:536-548 -> THCM.C:2704-2737, the reference's sequential order"""
    lf = ls = 0.0
    m, n = wet.shape
    for j in range(m):
        for i in range(n):
            lf = field[j, i] * cos_y[j] * wet[j, i] + lf
            ls = cos_y[j] * wet[j, i] + ls
    return lf / ls


def nondim(c):
    """QTnd and Ooa (usrc.F90:126, 1191-1200)"""
    dz = 1.0 / c.l
    ze = (c.l - 0.5) * dz - 1.0
    if c.qz > 1.0:
        dfz = c.qz / (math.tanh(c.qz) * math.cosh(c.qz * (ze + 1)) ** 2)
    else:
        dfz = 1.0 + (1.0 - c.qz) * (1.0 - 2.0 * ze)
    qtnd = 6.37e6 / (0.1 * 4.2e3 * 1.024e3 * c.hdim * (dz * dfz))
    return qtnd, 1.25 * (0.94 * 1.3e-3) * 1000.0 * 8.5 * qtnd


def uncoupled_fluxes(c, par, x, land_top, emip=None):
    """get_salflux / get_temflux with coupled_T = coupled_S = 0 and forcing type 2 or 0:
    (SalinityFlux, TemperatureFlux, SensibleHeatFlux, correction * gamma)"""
    n, m, l = c.n, c.m, c.l
    ymin, ymax = math.radians(c.ymin), math.radians(c.ymax)
    y = (np.arange(m) + 0.5) * ((ymax - ymin) / m) + ymin
    prof = np.cos(np.pi * (y - ymin) / (ymax - ymin)) if c.forcing_type == 2 else np.cos(np.pi * y / ymax)
    wet = 1 - land_top.reshape(m, n)
    top = x.reshape(l, m, n, 6)[l - 1]
    T, S = top[:, :, 4], top[:, :, 5]
    bi, comb = par["Nonlinear Factor"], par["Combined Forcing"]
    gamma, etabi = comb * par["Salinity Forcing"], comb * par["Temperature Forcing"]
    tatm = np.repeat(prof[:, None], n, axis=1)
    if emip is None:
        emip = tatm * wet
    qtnd, ooa = nondim(c)
    sal = wet * ((1 - c.sres) + c.sres * bi) * emip - c.sres * bi * S / gamma
    corr = qint(sal, np.cos(y), wet)
    sal = sal - corr
    tem = np.where(wet == 1, ((1 - c.tres) + c.tres * bi) * tatm - c.tres * bi * T / etabi, 0.0)
    qsh = np.where(wet == 1, -(ooa * (T - tatm)) / qtnd, 0.0)
    return sal.reshape(-1), tem.reshape(-1), qsh.reshape(-1), corr * gamma


def file_pars(t):
    return {k.split("/", 2)[2]: float(v.reshape(-1)[0]) for k, v in t.items() if k.startswith("/Parameters/")}


# ---- 8. CPU -----------------------------------------------------------------------------
def test_fixture_fluxes_numpy_restatement():
    """the ocean-only formulas in numpy at the fixture's state and parameters reproduce the
    fixture's three non-zero groups at 1e-12 * max|group| (land cells included)"""
    t = fixture()
    c = cf.preset("gateway16")
    sal, tem, qsh, _ = uncoupled_fluxes(c, file_pars(t), t["/State/Values"][0], t["/MaskGlobal/Surface"])
    check_group("SalinityFlux", sal, t["/SalinityFlux/Values"][0])
    check_group("TemperatureFlux", tem, t["/TemperatureFlux/Values"][0])
    check_group("SensibleHeatFlux", qsh, t["/SensibleHeatFlux/Values"][0])
    for name in ZERO:
        assert not np.any(t[f"/{name}/Values"]), name


def test_h5_int_vector_roundtrip(tmp_path):
    """an Epetra_IntVector group (Values int32, GlobalLength, __type__) reads back as written"""
    v = (np.arange(37, dtype=np.int32) * 7) % 3
    tree = {"MaskLocal": {"Values": v, "GlobalLength": np.array(v.size, dtype=np.int32),
                          "__type__": np.array([b"Epetra_IntVector"], dtype="S17")}}
    p = str(tmp_path / "iv.h5")
    h5.write(p, tree)
    t = h5.read(p)
    assert t["/MaskLocal/Values"][0].dtype == np.int32
    np.testing.assert_array_equal(t["/MaskLocal/Values"][0], v)
    assert int(np.asarray(t["/MaskLocal/GlobalLength"][0]).reshape(-1)[0]) == v.size
    assert bytes(t["/MaskLocal/__type__"][0][0]) == b"Epetra_IntVector"


# ---- GPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gateway():
    """the gateway16 ocean at the fixture's state and parameters, its fluxes and residual"""
    from iemic.ocean import Ocean
    c = cf.preset("gateway16")
    oc = Ocean(c, landm=golden_landm("gateway16"))
    assert oc.loadStateFromFile(REF_H5) == 0
    fl = oc.getFluxes()
    F = oc.computeRHS().copy()
    yield dict(c=c, oc=oc, fl=fl, F=F, t=fixture())
    oc.close()


@gpu
def test_fixture_parity(gateway):
    """1. getFluxes() at the reference's state equals the reference's fixture on all 256
    entries of the three non-zero groups; the other five groups are exactly zero"""
    fl, t = gateway["fl"], gateway["t"]
    assert gateway["oc"].getPar("Combined Forcing") == 0.020000184160660548
    for name in PINNED:
        check_group(name, fl[name], t[f"/{name}/Values"][0])
    for name in ZERO:
        assert fl[name].shape == (256,) and not np.any(fl[name]), name
    assert not np.any(fl["SeaIceMask"])
    assert np.isfinite(fl["Correction"])


@gpu
def test_residual_at_reference_solution(gateway):
    """2. the reference's converged state is a solution here: ||F||_2 <= 1e-5, and the u, v, w
    and p rows each <= 1e-8"""
    F = gateway["F"]
    norms = [float(np.linalg.norm(F[v::6])) for v in range(6)]
    print("||F||", float(np.linalg.norm(F)), dict(zip("uvwpTS", norms)))
    assert np.linalg.norm(F) <= 1e-5
    for v in range(4):
        assert norms[v] <= 1e-8, ("uvwp"[v], norms[v])


@gpu
def test_file_round_trip(gateway, tmp_path):
    """3. a saved file has the fixture's layout: the same dataset paths, shapes, dtypes and
    __type__ strings, the fixture's masks, and flux groups equal to getFluxes().  The
    fixture predates the Grid group and names its parameters as the reference then did
    (FPER, Time, no SPL2): outside Grid the path sets are equal once the parameter names are
    mapped (FPER is Flux Perturbation; Time is not a THCM parameter)."""
    oc, t, fl = gateway["oc"], gateway["t"], gateway["fl"]
    p = str(tmp_path / "ocean.h5")
    oc.saveStateToFile(p)
    s = {k: np.asarray(v) for k, (v, _) in h5.read(p).items()}
    ours = {k for k in s if not k.startswith(("/Grid/", "/Parameters/"))}
    theirs = {k for k in t if not k.startswith("/Parameters/")}
    assert ours == theirs, (sorted(ours - theirs), sorted(theirs - ours))
    pmap = {"/Parameters/FPER": "/Parameters/Flux Perturbation"}
    tp = {pmap.get(k, k) for k in t if k.startswith("/Parameters/")} - {"/Parameters/Time"}
    sp = {k for k in s if k.startswith("/Parameters/")} - {"/Parameters/SPL2"}
    assert sp == tp, (sorted(sp - tp), sorted(tp - sp))
    for k in sorted(theirs):
        assert s[k].shape == t[k].shape, k
        if t[k].dtype.kind == "S":
            assert s[k].dtype.kind == "S" and bytes(s[k].reshape(-1)[0]) == bytes(t[k].reshape(-1)[0]), k
        else:
            assert s[k].dtype == t[k].dtype, k
    for k in ("/MaskGlobal/Surface", "/MaskGlobal/Global", "/MaskLocal/Values"):
        np.testing.assert_array_equal(s[k], t[k], err_msg=k)
    for name in ORDER[:8]:
        np.testing.assert_array_equal(s[f"/{name}/Values"][0], fl[name], err_msg=name)
    q = str(tmp_path / "bare.h5")
    oc.saveStateToFile(q, save_salinity_flux=False, save_temperature_flux=False, save_mask=False)
    assert {k.split("/")[1] for k in h5.read(q)} == {"State", "Parameters", "Grid"}


def natl8_ocean(**kw):
    from iemic.ocean import Ocean
    c = cf.preset("natl8", mixing=0).with_(**kw)
    L = golden_landm("natl8")
    oc = Ocean(c, landm=L, solver_params={"FGMRES tolerance": 1e-10})
    oc.setState(cf.synthetic_state(c, L, amp_ts=1e-3))
    return c, oc


@gpu
@pytest.mark.parametrize("case", ["natl8", "gateway16"])
def test_inserted_emip_equals_profile(case, gateway):
    """4. setEmip(getEmip("E")) leaves F bitwise unchanged (natl8, SRES = 0: through the qint
    correction; gateway16, SRES = 1), and setEmip(None) after another field restores it"""
    if case == "natl8":
        c, oc = natl8_ocean()
        F0 = oc.computeRHS().copy()
    else:
        c, oc, F0 = gateway["c"], gateway["oc"], gateway["F"]
    e = oc.getEmip("E")
    assert np.any(e)
    oc.setEmip(e)
    np.testing.assert_array_equal(oc.computeRHS(), F0)
    np.testing.assert_array_equal(oc.getEmip("E"), e)
    other = e + np.random.default_rng(4).standard_normal(e.size)
    oc.setEmip(other)
    assert not np.array_equal(oc.computeRHS(), F0)
    oc.setEmip(None)
    np.testing.assert_array_equal(oc.computeRHS(), F0)
    # adapted_emip and spert: zero / SRES fields by default, and inert while their
    # parameters (Salinity Homotopy, Salinity Perturbation) are zero
    assert not np.any(oc.getEmip("A")) and np.all(oc.getEmip("P") == c.sres)
    oc.setEmip(oc.getEmip("A"), "A")
    oc.setEmip(oc.getEmip("P"), "P")
    np.testing.assert_array_equal(oc.computeRHS(), F0)
    oc.setEmip(None, "A")
    oc.setEmip(None, "P")
    if case == "natl8":
        oc.close()


@gpu
def test_inserted_tatm_equals_profile():
    """4. natl8 with TRES = 0: TemperatureFlux is then tatm itself on the ocean cells
    (probe.F90:342); inserted through setTatm it gives F bitwise (the land cells' entries are
    masked out of qint and of F)"""
    c, oc = natl8_ocean(tres=0)
    F0 = oc.computeRHS().copy()
    tatm = oc.getFluxes()["TemperatureFlux"]
    assert np.any(tatm)
    oc.setTatm(tatm)
    np.testing.assert_array_equal(oc.computeRHS(), F0)
    oc.setTatm(2.0 * tatm)
    assert not np.array_equal(oc.computeRHS(), F0)
    oc.setTatm(None)
    np.testing.assert_array_equal(oc.computeRHS(), F0)
    oc.close()


@gpu
def test_mixed_boundary_condition_restart(tmp_path):
    """5. spin up with restoring salinity (SRES = 1), save, continue under the diagnosed flux
    with SRES = 0: the loaded emip is the saved SalinityFlux times the ocean mask, and the
    salinity forcing in F is gamma (emip - qint(emip)) assembled in numpy from the file.  The
    forcing's part of F is taken as F(Salinity Forcing = 0) - F (the forcing is the only place
    the parameter enters an SRES = 0 ocean), to 1e-13 of its maximum."""
    from iemic.ocean import IemicError, Ocean
    c1, oc1 = natl8_ocean(sres=1)
    for _ in range(2):
        oc1.newtonStep()
    p = str(tmp_path / "spinup.h5")
    oc1.saveStateToFile(p)
    saved = oc1.getFluxes()["SalinityFlux"]
    L = oc1.landmask().reshape(c1.l + 2, c1.m + 2, c1.n + 2)
    wet = 1 - L[c1.l, 1:c1.m + 1, 1:c1.n + 1]
    with pytest.raises(IemicError):
        oc1.loadStateFromFile(p, load_salinity_flux=True)          # SRES = 1
    with pytest.raises(IemicError):
        oc1.loadStateFromFile(p, load_temperature_flux=True)       # TRES = 1
    oc1.close()

    c2 = c1.with_(sres=0)
    oc2 = Ocean(c2, landm=golden_landm("natl8"))
    assert oc2.loadStateFromFile(p, load_salinity_flux=True) == 0
    t = {k: np.asarray(v) for k, (v, _) in h5.read(p).items()}
    flux = t["/SalinityFlux/Values"][0]
    np.testing.assert_array_equal(flux, saved)
    emip = flux * wet.reshape(-1)
    np.testing.assert_array_equal(oc2.getEmip("E"), emip)
    ymin, ymax = math.radians(c2.ymin), math.radians(c2.ymax)
    y = (np.arange(c2.m) + 0.5) * ((ymax - ymin) / c2.m) + ymin
    gamma0 = oc2.getPar("Combined Forcing") * oc2.getPar("Salinity Forcing")
    want = gamma0 * (emip.reshape(c2.m, c2.n) - qint(emip.reshape(c2.m, c2.n), np.cos(y), wet)) * wet
    F = oc2.computeRHS().copy()
    oc2.setPar("Salinity Forcing", 0.0)
    F0 = oc2.computeRHS().copy()
    got = (F0 - F).reshape(c2.l, c2.m, c2.n, 6)[c2.l - 1, :, :, 5].copy()
    ri = oc2.rowintcon
    assert ri >= 0
    cell = ri // 6 - (c2.l - 1) * c2.m * c2.n
    got.reshape(-1)[cell] = want.reshape(-1)[cell]                  # the integral condition's row
    gap = float(np.max(np.abs(got - want)))
    print("forcing gap", gap, "max", float(np.max(np.abs(want))))
    assert np.max(np.abs(want)) > 0
    assert gap <= 1e-13 * np.max(np.abs(want))
    # a missing group, and the coupled refusals
    q = str(tmp_path / "noflux.h5")
    oc2.saveStateToFile(q, save_salinity_flux=False)
    with pytest.raises(IemicError):
        oc2.loadStateFromFile(q, load_salinity_flux=True)
    oc2.close()
    from test_coupled import landm_of
    cc = cf.preset("coupled_natl8s")
    oc3 = Ocean(cc.with_(sres=0, tres=0), landm=landm_of("coupled_natl8s"), analyze_jacobian=False)
    with pytest.raises(IemicError):
        oc3.loadStateFromFile(p, load_salinity_flux=True)          # coupled salinity
    with pytest.raises(IemicError):
        oc3.loadStateFromFile(p, load_temperature_flux=True)       # coupled temperature
    oc3.close()


@gpu
@pytest.mark.parametrize("case", ["flux_coupled_natl8", "flux_coupled_natl8s", "flux_natl8_emip"])
def test_fluxes_against_reference_fortran(case):
    """6. the coupled branches (coupled T; coupled T and S) and an ocean-only SRES = 0 case
    with an inserted non-profile emip against the reference's Fortran (flux_*.npz), all
    nine fields and the correction at 1e-12 * max|field|"""
    from iemic.ocean import Ocean
    from test_coupled import atm_args, landm_of
    name = {"flux_coupled_natl8": "coupled_natl8", "flux_coupled_natl8s": "coupled_natl8s",
            "flux_natl8_emip": "natl8"}[case]
    ref = golden(case)
    g = golden(name)
    c = cf.preset(name, mixing=0)
    oc = Ocean(c, landm=landm_of(name), analyze_jacobian=False)
    if "atm_t" in g:
        t, q, a, pars = atm_args(g)
        oc.setAtmosphere(t, q, a, g["atm_p"], pars)
    else:
        oc.setEmip(ref["emip"])
    oc.setState(g["synthetic_x"])
    fl = oc.getFluxes()
    oc.close()
    for q, key in enumerate(ORDER):
        want = ref["fluxes"][q]
        if np.any(want):
            check_group(f"{case}/{key}", fl[key], want)
        else:
            assert not np.any(fl[key]), key
    assert abs(fl["Correction"] - float(ref["correction"])) <= 1e-12 * abs(float(ref["correction"]))
    assert np.any(ref["fluxes"][0]) and np.any(ref["fluxes"][3])
    if "atm_t" in g:
        assert np.any(ref["fluxes"][4]) and np.any(ref["fluxes"][6])    # shortwave, latent


def owned_rows(c, lay):
    k = np.arange(c.l)[:, None, None, None]
    j = np.arange(lay["jb0"], lay["jb1"])[None, :, None, None]
    i = np.arange(lay["ib0"], lay["ib1"])[None, None, :, None]
    return (6 * ((k * c.m + j) * c.n + i) + np.arange(6)[None, None, None, :]).reshape(-1)


@gpu
@pytest.mark.parametrize("npx", [2, 1])
def test_decomposition_invariance(gateway, npx):
    """7. two in-process ranks (2 x 1 and 1 x 2): getFluxes() and the correction are bitwise
    the single-rank result on every rank, and so is F with an inserted emip"""
    from iemic import _lib
    from iemic.ocean import Ocean
    c, oc = gateway["c"], gateway["oc"]
    emip = np.random.default_rng(7).standard_normal(c.n * c.m)
    oc.setEmip(emip)
    F1 = oc.computeRHS().copy()
    oc.setEmip(None)
    nranks = 2
    group = _lib.lib().iemic_local_group_new(nranks)
    res = [None] * nranks

    def work(r):
        try:
            o = Ocean(c, landm=golden_landm("gateway16"), local_group=group, rank=r, nranks=nranks, npx=npx)
            o.loadStateFromFile(REF_H5)
            fl = o.getFluxes()
            o.setEmip(emip)
            F = o.computeRHS().copy()
            res[r] = dict(fl=fl, F=F, lay=o.layout())
            o.close()
        except Exception as e:  # noqa: BLE001
            res[r] = dict(err=repr(e))

    th = [threading.Thread(target=work, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    _lib.lib().iemic_local_group_free(group)
    assert not [r["err"] for r in res if "err" in r], res
    F = np.zeros(c.nrows)
    for r in res:
        assert (r["lay"]["npx"], r["lay"]["npy"]) == ((2, 1) if npx == 2 else (1, 2))
        for key in ORDER:
            np.testing.assert_array_equal(r["fl"][key], gateway["fl"][key], err_msg=key)
        assert r["fl"]["Correction"] == gateway["fl"]["Correction"]
        rows = owned_rows(c, r["lay"])
        F[rows] = r["F"][rows]
    np.testing.assert_array_equal(F, F1)
