"""The block GS set-up with its two factorisations side by side (gs_setup.hip gs_factor: the
Schur cyclic reduction on the context's stream, the T/S multigrid set-up on the side stream)
against the same set-up in serial order (a context created under IEMIC_SERIAL_SETUP=1).

Both orders issue the same launches on the same data in the same per-chain order, so the
factors -- and every apply and solve that uses them -- must be bitwise equal: no tolerance.

Coarsest T/S level of each fixture (ts_mg_setup.hip mg_levels: 2x2 coarsening until the level has
at most 128 cells, stopping early at the first level of at most 1024 cells whose longitude blocks
2 m l fit 192 unknowns):
  natl8      8 x  8 x  4 -> 4 x 4 x 4  =  64 cells, 128 unknowns: the dense device inverse
                                         (mg_coarse_dev, one k_cr_inv workgroup)
  gateway16 16 x 16 x 16 -> 4 x 4 x 16 = 256 cells (8 x 8 x 16 has blocks of 256 > 192): the
                                         whole-problem cyclic reduction, 4 blocks of 128
  global4   96 x 38 x 12 -> 12 x 5 x 12 = 720 cells: the cyclic reduction, 12 blocks of 120
So the side stream carries a second SchurCR factorisation on gateway16 and global4, and the
single-workgroup inverse with its own pivot flag on natl8.
"""
import os

import numpy as np
import pytest

from helpers import golden_landm
from iemic import config as cf

pytestmark = pytest.mark.gpu

NAMES = ("natl8", "gateway16", "global4")
SEEDS = (20261015, 77)              # the two states of the repeated set-up
ENV = "IEMIC_SERIAL_SETUP"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def make(name, serial):
    """a context whose creation saw IEMIC_SERIAL_SETUP=1 (serial) or no such variable"""
    from iemic.ocean import Ocean
    old = os.environ.pop(ENV, None)
    try:
        if serial:
            os.environ[ENV] = "1"
        return Ocean(cf.preset(name, mixing=0), landm=golden_landm(name))
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


def set_up(oc, x):
    oc.setState(x)
    oc.computeJacobian()
    oc.buildPreconditioner(force=True)


_CASE = {}


def case(name):
    """the two contexts, the two states, the fixed vector, and the serial context's apply for
    each state (computed once, shared, read-only)"""
    if name not in _CASE:
        ser, par = make(name, True), make(name, False)
        c = ser.cfg
        L = ser.landmask().reshape(c.l + 2, c.m + 2, c.n + 2)
        xs = [cf.synthetic_state(c, L, seed=s, amp_ts=1e-3) for s in SEEDS]
        r = cf.synthetic_vector(c, seed=11)
        ref = []
        for x in xs:
            set_up(ser, x)
            z = ser.applyPrecon(r).copy()
            assert np.all(np.isfinite(z)) and np.any(z != 0.0)
            z.setflags(write=False)
            ref.append(z)
        assert not np.array_equal(ref[0], ref[1]), "the two states give the same preconditioner"
        _CASE[name] = dict(ser=ser, par=par, xs=xs, r=r, ref=ref)
    return _CASE[name]


@pytest.mark.parametrize("name", NAMES)
def test_apply_bitwise(name):
    s = case(name)
    set_up(s["par"], s["xs"][0])
    z = s["par"].applyPrecon(s["r"])
    nd = int(np.count_nonzero(bits(z) != bits(s["ref"][0])))
    print(f"{name}: {nd} of {z.size} entries differ")
    assert nd == 0


@pytest.mark.parametrize("name", NAMES)
def test_repeated_setup(name):
    """three set-ups in a row on alternating states in the default context, an apply after
    each: a missing join or a scratch buffer shared by the two chains would leave factors of
    the other state (or half-written ones) behind"""
    s = case(name)
    nd = []
    for k in (0, 1, 0):
        set_up(s["par"], s["xs"][k])
        z = s["par"].applyPrecon(s["r"])
        nd.append(int(np.count_nonzero(bits(z) != bits(s["ref"][k]))))
    print(f"{name}: differing entries per set-up {nd}")
    assert nd == [0, 0, 0]


def test_solve_bitwise():
    """one FGMRES solve to 1e-8 on global4 in both contexts: the Newton path's own sequence
    (set-up, then the solve's applies on the same streams)"""
    s = case("global4")
    out = []
    for oc in (s["ser"], s["par"]):
        set_up(oc, s["xs"][0])
        b = oc.applyMatrix(cf.synthetic_vector(oc.cfg, seed=5)).copy()
        oc.solver_params.update({"FGMRES tolerance": 1e-8, "FGMRES iterations": 90, "FGMRES restarts": 20})
        dx = oc.solve(b).copy()
        out.append((b, dx, oc.last_solve.iters, oc.last_solve.converged, oc.last_solve.explicit_rel_res))
    (b0, x0, it0, cv0, rr0), (b1, x1, it1, cv1, rr1) = out
    print(f"global4: iterations {it0} / {it1}, relative residual {rr0:.3e} / {rr1:.3e}")
    assert np.array_equal(bits(b0), bits(b1))
    assert cv0 == 1 and cv1 == 1
    assert it0 == it1
    assert np.array_equal(bits(x0), bits(x1))
