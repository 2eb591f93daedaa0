"""The T/S multigrid's entry launch on its packed operand (k_mg_entry_p, TsMg::ep) against the
launch that reads the slot-major Jacobian (k_mg_entry), which the test hook
iemic_test_ts_mg_nopack switches back on.  Both form rr_TS - A_TS,D z_D with the same operands
in the same order and run the same colour-0 line solve, so everything here is compared bit for
bit, no tolerance.

    case        grid                     reaches
    natl8       8x8x4, land              one partial tile per row (nx < 16)
    gateway16   16x16x16, periodic, land one whole tile per row, four mask words, x wrap
    natl24      24x24x4 (natl8's mask    two tiles per row, the second half empty (nx = 24 is
                refined 3x)              no multiple of 16), coast lines inside both tiles
    gateway16, two latitude bands        level 0 with halo rows (the pack covers owned rows)

The entry hook seeds the planar right-hand side and the dynamics iterate with random numbers
on every row, identity and halo rows included, and NaN bit patterns in level 0's b and z.
"""
import ctypes as C

import numpy as np
import pytest

import dense_hooks as dh
import ts_mg_ref as R
from iemic import config as cf

pytestmark = pytest.mark.gpu

_PD = C.POINTER(C.c_double)
_live = {}


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    _live.clear()


def hooks():
    L = dh.hooks()
    L.iemic_test_ts_mg_nopack.restype = C.c_int
    L.iemic_test_ts_mg_nopack.argtypes = [C.c_void_p, C.c_int]
    L.iemic_test_ts_mg_entry.restype = C.c_int
    L.iemic_test_ts_mg_entry.argtypes = [C.c_void_p, C.c_int64, _PD, _PD, _PD, _PD, C.POINTER(C.c_int64)]
    return L


def nopack(oc, on):
    rc = hooks().iemic_test_ts_mg_nopack(oc._h, int(on))
    assert rc == 0, dh.last_error()


def case(name):
    if name == "natl24":
        c = cf.preset("natl8", mixing=1).with_(name=name, n=24, m=24, refine=3)
        return c, cf.init_landmask(c, cf.landmask(c))
    return R.case_config(name)


def states(c, L):
    return (cf.synthetic_state(c, L, amp_ts=1e-3), cf.synthetic_state(c, L, seed=11, amp_ts=2e-3))


def device(name):
    """the case's context, the preconditioner set up at the first of two states"""
    from iemic.ocean import Ocean
    if name not in _live:
        c, L0 = case(name)
        oc = Ocean(c, landm=L0, solver_params={"Preconditioner": 2, "TS multigrid cycles": 1})
        L = oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
        xs = states(c, L)
        oc.setState(xs[0])
        oc.computeJacobian()
        oc.buildPreconditioner(force=True)
        _live[name] = (c, oc, xs)
    return _live[name]


def entry(c, oc, seed):
    """(b, z, pack doubles) of level 0 after the entry launch alone, from seeded rr and z_D"""
    NE = oc.layout()["ext_rows"]
    rng = np.random.default_rng(seed)
    rr, zd = rng.uniform(-1.0, 1.0, NE), rng.uniform(-1.0, 1.0, NE)
    ncl = c.n * c.m * c.l
    b, z = np.full(2 * ncl, np.nan), np.full(2 * ncl, np.nan)
    npk = C.c_int64(0)
    rc = hooks().iemic_test_ts_mg_entry(oc._h, NE, dh._d(rr), dh._d(zd), dh._d(b), dh._d(z), C.byref(npk))
    assert rc == 0, dh.last_error()
    return b, z, npk.value


def both(c, oc, seed):
    nopack(oc, True)
    try:
        old = entry(c, oc, seed)
    finally:
        nopack(oc, False)
    return old, entry(c, oc, seed)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


CASES = ("natl8", "gateway16", "natl24")


@pytest.mark.parametrize("name", CASES)
def test_entry_bitwise(name):
    """level 0's b and z after the entry launch: packed == slot-major, bit for bit"""
    c, oc, _ = device(name)
    (b0, z0, _), (b1, z1, npk) = both(c, oc, 5)
    assert np.all(np.isfinite(b0)) and np.all(np.isfinite(z0)), "the entry left cells unwritten"
    assert np.any(b0 != 0.0) and np.any(z0 != 0.0)
    np.testing.assert_array_equal(bits(b1), bits(b0))
    np.testing.assert_array_equal(bits(z1), bits(z0))
    wet = int(np.count_nonzero(b0.reshape(2, -1).any(axis=0)))
    print(f"entry pack {name}: {npk} doubles for {wet} cells with a T/S right-hand side "
          f"of {c.n * c.m * c.l}")
    # 20 terms per active cell, each tile's run rounded up to a 128-byte line
    tiles = -(-c.n // 16) * c.m
    assert 20 * wet <= npk <= 20 * c.n * c.m * c.l + 16 * tiles


@pytest.mark.parametrize("name", CASES)
def test_pack_follows_the_jacobian(name):
    """a second Jacobian in the same context: the pack is that Jacobian's"""
    from iemic.ocean import Ocean
    c, L0 = case(name)
    oc = Ocean(c, landm=L0, solver_params={"Preconditioner": 2, "TS multigrid cycles": 1})
    L = oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
    got = []
    for x in states(c, L):
        oc.setState(x)
        oc.computeJacobian()
        oc.buildPreconditioner(force=True)
        old, new = both(c, oc, 7)
        np.testing.assert_array_equal(bits(new[0]), bits(old[0]))
        np.testing.assert_array_equal(bits(new[1]), bits(old[1]))
        got.append(new[0])
    oc.close()
    assert np.any(got[0] != got[1]), "the two Jacobians give the same right-hand side"


@pytest.mark.parametrize("name", CASES)
def test_apply_bitwise(name):
    """iemic_prec_apply with and without the pack"""
    c, oc, _ = device(name)
    r = cf.synthetic_vector(c, seed=3)
    z1 = oc.applyPrecon(r)
    nopack(oc, True)
    try:
        z0 = oc.applyPrecon(r)
    finally:
        nopack(oc, False)
    assert np.all(np.isfinite(z0)) and np.any(z0.reshape(-1, R.NUN)[:, R.TT:] != 0.0)
    np.testing.assert_array_equal(bits(z1), bits(z0))


def test_apply_bitwise_two_bands():
    """two latitude bands (level 0 keeps halo rows): the apply with and without the pack"""
    from iemic.ocean import Ocean
    from test_gpu_dist import _run_bands
    c, L0 = case("gateway16")
    r = cf.synthetic_vector(c, seed=3)

    def fn(rk, group):
        oc = Ocean(c, landm=L0, local_group=group, rank=rk, nranks=2, npx=1,
                   solver_params={"Preconditioner": 2, "TS multigrid cycles": 1})
        L = oc.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
        oc.setState(states(c, L)[0])
        oc.computeJacobian()
        oc.buildPreconditioner(force=True)
        z1 = oc.applyPrecon(r).copy()
        nopack(oc, True)
        z0 = oc.applyPrecon(r).copy()
        nopack(oc, False)
        oc.close()
        return dict(z0=z0, z1=z1)

    for q in _run_bands(2, fn):
        assert np.all(np.isfinite(q["z0"])) and np.any(q["z0"] != 0.0)
        np.testing.assert_array_equal(bits(q["z1"]), bits(q["z0"]))
