"""The T/S aggregation multigrid on the device (ts_mg.hip, ts_mg_setup.hip) against the
matrix-algebra reference tests/ts_mg_ref.py, on every path of the V-cycle and of the set-up, one
rank.  The preconditioner is applied to a right-hand side that is nonzero on the T and S rows
only: the dynamics iterate is then exactly 0 and z(T, S) is the multigrid's result alone.

    case        grid                       reaches
    natl8       8x8x4, land                two levels, device inverse (128 unknowns), P = 16
    natl8_l8    8x8x8                      host-assembled coarsest (256 unknowns)
    gateway16   16x16x16, periodic, land   fused intermediate level; CR coarsest, 4 blocks of 128
    2dmoc       3x6x6, periodic            four colours on level 0; coarse n = 2 wrap
    2dmoc_run   4x32x16, periodic          fused periodic n = 2 level; coarsest n = 1 self-wrap; host
    box6        6x16x16, periodic          odd periodic intermediate level 3x8x16 (four colours, unfused)
    natl8_l20   8x8x20                     P = 32; CR coarsest (4x4x20)
    natl8_l40   8x8x40                     P = 64; fused level at 640 threads; CR coarsest (2x2x40)

Every test first asserts through the plan hook that the device is on the path the reference's
own level rule (ts_mg_ref.expected_plan) gives for the case.  The bar is the project's
max|z - ref| <= 1e-8 max|ref|, here in the T/S norm alone; the rounding floor of the reference
itself (ts_mg_ref.FLOOR, measured against the C twin by tests/test_ts_mg_ref.py) is at most
1.4e-12.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import dense_hooks as dh
import ts_mg_ref as R
from helpers import mask_fix
from iemic import config as cf

pytestmark = pytest.mark.gpu

BAR = 1e-8
_live = {}


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    _live.clear()


def device(name, cycles=1, sweeps=1):
    """the case's context with the preconditioner built, its reference and right-hand side;
    built once per (case, cycles, sweeps), the reference once per case"""
    from iemic.ocean import Ocean
    key = (name, cycles, sweeps)
    if key in _live:
        return _live[key]
    c, L0 = R.case_config(name)
    oc = Ocean(c, landm=L0, solver_params={"Preconditioner": 2, "TS multigrid cycles": cycles,
                                           "Multigrid sweeps": sweeps})
    L = oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    oc.setState(cf.synthetic_state(c, L, amp_ts=1e-3))
    oc.computeJacobian()
    oc.buildPreconditioner(force=True)
    if ("ref", name) not in _live:
        rowptr, col, val = oc.exportCSR()
        ref = R.TsMgRef(rowptr, col, val, L, c.n, c.m, c.l, c.periodic, oc.rowintcon, c.int_sign,
                        oc.getIntCondCoeff())
        r = R.ts_only(cf.synthetic_vector(c, seed=3))
        r.setflags(write=False)
        _live[("ref", name)] = (ref, (rowptr, col, val), r)
    _live[key] = (c, oc) + _live[("ref", name)]
    return _live[key]


def reference(name, cycles=1, sweeps=1):
    """(z, trace) of the reference, computed once and left unchanged"""
    key = ("z", name, cycles, sweeps)
    if key not in _live:
        ref, csr, r = _live[("ref", name)]
        z, t = R.apply_ts(ref, *csr, r, cycles=cycles, sweeps=sweeps, trace=True)
        z.setflags(write=False)
        _live[key] = (z, t)
    return _live[key]


def assert_plan(c, oc, sweeps=1):
    want = R.expected_plan(c.n, c.m, c.l, c.periodic, sweeps)
    got = dh.ts_mg_plan(oc._h)
    assert got == want, (got, want)
    return got


def ts(z):
    return np.asarray(z).reshape(-1, R.NUN)[:, R.TT:]


def check_apply(name, cycles, sweeps):
    c, oc, ref, csr, r = device(name, cycles, sweeps)
    assert_plan(c, oc, sweeps)
    z = oc.applyPrecon(r)
    zr, _ = reference(name, cycles, sweeps)
    assert np.all(np.isfinite(z))
    assert np.all(z.reshape(-1, R.NUN)[:, :R.TT] == 0.0), "z is not 0 on U, V, W, P"
    d = np.max(np.abs(ts(z - zr))) / np.max(np.abs(ts(zr)))
    floor = R.FLOOR[name][min(cycles, 2) - 1] if sweeps == 1 else float("nan")
    print(f"ts_mg {name} cycles={cycles} sweeps={sweeps}: device-reference {d:.2e} (CPU floor {floor:.1e})")
    assert d <= BAR, d
    return z


@pytest.mark.parametrize("name", R.CASES)
def test_default_apply(name):
    """(a) one cycle, one sweep"""
    check_apply(name, 1, 1)


def stencil_matrix(off, diag, n, m, l, periodic):
    """the device's level arrays as a sparse matrix over u = var ncl + (j n + i) l + k: diag
    (TT, TS, ST, SS), off[8 R + q] of row R: q 0..5 the same variable at -i, +i, -j, +j, -k, +k,
    q 6, 7 the other variable at -k, +k; a coupling to outside the level must be 0"""
    ncl = n * m * l
    t = np.arange(ncl)
    j, i, k = t // (n * l), (t // l) % n, t % l
    rows, cols, vals = [], [], []
    for Rv in range(2):
        rows += [Rv * ncl + t, Rv * ncl + t]
        cols += [Rv * ncl + t, (1 - Rv) * ncl + t]
        vals += [diag[3 * Rv], diag[1 + Rv]]
        for q in range(8):
            d = q if q < 6 else q - 2
            ii = i + (d == 1) - (d == 0)
            jj = j + (d == 3) - (d == 2)
            kk = k + (d == 5) - (d == 4)
            if periodic:
                ii = ii % n
            inside = (ii >= 0) & (ii < n) & (jj >= 0) & (jj < m) & (kk >= 0) & (kk < l)
            v = off[8 * Rv + q]
            assert np.all(v[~inside] == 0.0), f"coupling {q} of row {Rv} leaves the level"
            var = Rv if q < 6 else 1 - Rv
            rows.append((Rv * ncl + t)[inside])
            cols.append((var * ncl + (jj * n + ii) * l + kk)[inside])
            vals.append(v[inside])
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * ncl, 2 * ncl))
    A.eliminate_zeros()
    return A


@pytest.mark.parametrize("name", R.CASES)
def test_levels(name):
    """(b) after the default apply: every level's operator, right-hand side and iterate, the
    coarsest inverse against the reference's and against the device's own operator"""
    c, oc, ref, csr, r = device(name)
    plan = assert_plan(c, oc)
    oc.applyPrecon(r)
    _, t = reference(name)
    nlev = plan["nlev"]
    for q, (n, m) in enumerate(plan["sizes"]):
        off, diag, b, z, cinv = dh.ts_mg_level(oc._h, q, n, m, c.l, q == nlev - 1)
        assert all(np.all(np.isfinite(v)) for v in (off, diag, b, z))
        A = stencil_matrix(off, diag, n, m, c.l, c.periodic)
        Ar = t["A"][q]
        amax = np.max(np.abs(Ar.data))
        da = abs(A - Ar).max() / amax
        db = np.max(np.abs(b - t["b"][q])) / np.max(np.abs(t["b"][q]))
        dz = np.max(np.abs(z - t["z"][q])) / np.max(np.abs(t["z"][q]))
        print(f"ts_mg {name} level {q} ({n}x{m}x{c.l}): A {da:.2e} b {db:.2e} z {dz:.2e}")
        assert da <= 1e-12, (q, da)
        assert db <= BAR, (q, db)
        assert dz <= BAR, (q, dz)
        if q == nlev - 1:
            Ad = A.toarray()
            ina = np.nonzero(Ad.diagonal() == 0.0)[0]
            Ad[ina, ina] = 1.0
            assert np.all(np.isfinite(cinv))
            di = np.max(np.abs(cinv - t["cinv"])) / np.max(np.abs(t["cinv"]))
            dI = np.max(np.abs(cinv @ Ad - np.eye(Ad.shape[0])))
            print(f"ts_mg {name} coarsest kind {plan['kind']}: cinv {di:.2e} cinv A - I {dI:.2e}")
            assert di <= 1e-10, di
            assert dI <= 1e-9, dI


@pytest.mark.parametrize("name", ["natl8", "gateway16", "2dmoc", "box6"])
def test_two_cycles(name):
    """(c) the second cycle: a full pre-sweep on level 0 and the full-residual restriction"""
    z2 = check_apply(name, 2, 1)
    z1, _ = reference(name, 1, 1)
    assert np.max(np.abs(ts(z2 - z1))) > 1e-6 * np.max(np.abs(ts(z1)))


@pytest.mark.parametrize("name", ["gateway16", "2dmoc_run", "box6"])
def test_two_sweeps(name):
    """(d) two sweeps per level: the unfused visit of every coarse level"""
    check_apply(name, 1, 2)


@pytest.mark.parametrize("name", ["gateway16", "2dmoc_run", "natl8_l40"])
def test_fused_equals_unfused(name):
    """(e) k_mg_dn / k_mg_up against the launches they fuse, on the same factors.  The source
    arithmetic is the same operation for operation, but the unit is compiled with contraction
    on, so the pair is not bitwise equal everywhere: measured 0 differing entries on gateway16
    and 2dmoc_run (P = 16), 560 of 15360 on natl8_l40 (P = 64), the largest 2.84e-14.  The
    comment above k_mg_dn says so now, and the pair is held to the bar of (a)."""
    c, oc, ref, csr, r = device(name)
    plan = assert_plan(c, oc)
    assert any(plan["fused"])
    zf = oc.applyPrecon(r)
    dh.ts_mg_nofuse(oc._h, True)
    try:
        assert not any(dh.ts_mg_plan(oc._h)["fused"])
        zu = oc.applyPrecon(r)
    finally:
        dh.ts_mg_nofuse(oc._h, False)
    ndiff = int(np.count_nonzero(zf != zu))
    print(f"ts_mg {name} fused vs unfused: {ndiff} of {zf.size} entries differ, "
          f"max {np.max(np.abs(zf - zu)):.2e}")
    assert np.all(zf.reshape(-1, R.NUN)[:, :R.TT] == zu.reshape(-1, R.NUN)[:, :R.TT])
    assert np.max(np.abs(ts(zf - zu))) <= BAR * np.max(np.abs(ts(zu)))
    zr, _ = reference(name)
    assert np.max(np.abs(ts(zu - zr))) <= BAR * np.max(np.abs(ts(zr)))
    assert dh.ts_mg_plan(oc._h) == plan


@pytest.mark.parametrize("name", ["gateway16", "global4"])
def test_full_rhs_per_variable(oracle_lib, name):
    """(f) the whole default preconditioner on the full right-hand side against the C twin, each
    of the six variables in its own max norm"""
    from helpers import golden_landm
    from iemic.ocean import Ocean
    c = cf.preset(name, mixing=1)
    L0 = golden_landm(name)
    oc = Ocean(c, landm=L0, solver_params={"Preconditioner": 2})
    sp_ = oc.solver_params
    L = mask_fix(oracle_lib, c, L0)
    o = oracle_lib.Oracle(c.ref_dict(), L, c.par_list())
    x = cf.synthetic_state(c, L, amp_ts=1e-3)
    oc.setState(x)
    oc.computeJacobian()
    oc.buildPreconditioner(force=True)
    ov, _ = o.jacobian(x)
    P = oracle_lib.BlockGS(o, ov, 3, dyn_iters=sp_["Dyn iterations"], dyn_omega=sp_["Dyn damping"],
                           ts_mg=sp_["TS multigrid cycles"], schur_passes=sp_["Schur passes"])
    r = cf.synthetic_vector(c, seed=3)
    z, zc = oc.applyPrecon(r).reshape(-1, R.NUN), P.apply(r).reshape(-1, R.NUN)
    assert np.all(np.isfinite(z))
    d = [np.max(np.abs(z[:, v] - zc[:, v])) / np.max(np.abs(zc[:, v])) for v in range(R.NUN)]
    print(f"block GS {name} per variable (U V W P T S): " + " ".join(f"{v:.2e}" for v in d))
    for v in range(R.NUN):
        assert d[v] <= BAR, (v, d)
