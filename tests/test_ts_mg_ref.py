"""The matrix-algebra reference of the T/S multigrid (tests/ts_mg_ref.py) against the oracle's
C twin (oracle/prec_oracle.c), on the CPU.  The two are float64 formulations of the same
V-cycle in different operation order (sparse triple products and dense column solves here, stencil
arrays and block Thomas there), so their distance is the rounding floor of each case: what a
comparison of the device's result with the reference can be expected to resolve.

Rounding floor max|z_TS - twin| / max|twin_TS| measured per case (right-hand side
synthetic_vector(seed=3) on the T and S rows only, state synthetic_state(amp_ts=1e-3)):

    case         cycles = 1   cycles = 2
    natl8         5.2e-15   1.0e-14
    natl8_l8      1.9e-14   9.4e-15
    gateway16     4.1e-14   8.3e-15
    2dmoc         5.7e-15   4.0e-15
    2dmoc_run     1.3e-14   3.2e-14
    box6          4.6e-15   1.1e-14
    natl8_l20     1.5e-14   4.9e-14
    natl8_l40     7.8e-13   1.3e-12

(ts_mg_ref.FLOOR holds the same figures for the device tests to print beside theirs.)  Every
floor must stay at or below FLOOR_MAX = 1e-10: two orders below the 1e-8 bar at which
tests/test_gpu_ts_mg.py compares the device with this reference.
"""
import functools

import numpy as np
import pytest

import ts_mg_ref as R
from helpers import mask_fix
from iemic import config as cf

FLOOR_MAX = 1e-10
_orc = None


@functools.lru_cache(maxsize=None)
def problem(name):
    """(cfg, oracle, Jacobian values, reference, T/S-only right-hand side) of a case, built once"""
    c, L0 = R.case_config(name)
    L = mask_fix(_orc, c, L0)
    o = _orc.Oracle(c.ref_dict(), L, c.par_list())
    x = cf.synthetic_state(c, L, amp_ts=1e-3)
    ov, _ = o.jacobian(x)
    ref = R.TsMgRef(o.rowptr, o.col, ov, L, c.n, c.m, c.l, c.periodic, o.rowintcon, c.int_sign,
                    o.intcond_coeff())
    r = R.ts_only(cf.synthetic_vector(c, seed=3))
    r.setflags(write=False)
    return c, o, ov, ref, r


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_lib):
    global _orc
    _orc = oracle_lib


def ts_norm(z):
    return np.max(np.abs(np.asarray(z).reshape(-1, R.NUN)[:, R.TT:]))


@pytest.mark.parametrize("cycles", [1, 2])
@pytest.mark.parametrize("name", R.CASES)
def test_reference_matches_twin(name, cycles):
    c, o, ov, ref, r = problem(name)
    zc = _orc.BlockGS(o, ov, 3, ts_mg=cycles).apply(r)
    assert np.all(zc.reshape(-1, R.NUN)[:, :R.TT] == 0.0), "the twin's dynamics iterate is not 0"
    z = R.apply_ts(ref, o.rowptr, o.col, ov, r, cycles=cycles)
    floor = ts_norm(z - zc) / ts_norm(zc)
    print(f"floor {name} cycles={cycles}: {floor:.2e}")
    assert np.all(np.isfinite(z)) and ts_norm(zc) > 0.0
    assert floor <= FLOOR_MAX, floor


@pytest.mark.parametrize("name", R.CASES)
def test_level_structure(name):
    """the case reaches the path the table of tests/test_gpu_ts_mg.py claims for it"""
    c, o, ov, ref, r = problem(name)
    p = R.expected_plan(c.n, c.m, c.l, c.periodic)
    want = {
        "natl8": dict(sizes=[(8, 8), (4, 4)], kind=0, lanes=16, colours=[2, 2], fused=[0, 0]),
        "natl8_l8": dict(sizes=[(8, 8), (4, 4)], kind=2, lanes=16, colours=[2, 2], fused=[0, 0]),
        "gateway16": dict(sizes=[(16, 16), (8, 8), (4, 4)], kind=1, lanes=16, colours=[2, 2, 2], fused=[0, 1, 0]),
        "2dmoc": dict(sizes=[(3, 6), (2, 3)], kind=0, lanes=16, colours=[4, 2], fused=[0, 0]),
        "2dmoc_run": dict(sizes=[(4, 32), (2, 16), (1, 8)], kind=2, lanes=16, colours=[2, 2, 4], fused=[0, 1, 0]),
        "box6": dict(sizes=[(6, 16), (3, 8), (2, 4)], kind=2, lanes=16, colours=[2, 4, 2], fused=[0, 0, 0]),
        "natl8_l20": dict(sizes=[(8, 8), (4, 4)], kind=1, lanes=32, colours=[2, 2], fused=[0, 0]),
        "natl8_l40": dict(sizes=[(8, 8), (4, 4), (2, 2)], kind=1, lanes=64, colours=[2, 2, 2], fused=[0, 1, 0]),
    }[name]
    for k, v in want.items():
        assert p[k] == v, (k, p[k], v)
    assert [(L.n, L.m) for L in ref.levels] == want["sizes"]
    # every level keeps an active unknown, and the wrap couples the first and last longitude
    for q, L in enumerate(ref.levels):
        assert L.active.any()
        if c.periodic and L.n > 2:
            ncl = L.n * L.m * L.l
            u = np.arange(2 * ncl)
            i = (u % ncl // L.l) % L.n
            A = L.A.tocoo()
            assert np.any((i[A.row] == 0) & (i[A.col] == L.n - 1)), f"level {q} has no wrap coupling"


@pytest.mark.parametrize("name", R.CASES)
def test_two_sweeps_reference(name):
    """sweeps = 2 has no twin: one V-cycle with two sweeps reduces |b - A0 z| at least as much
    as with one, and the cycle is linear in b to 1e-12"""
    c, o, ov, ref, r = problem(name)
    A0 = ref.levels[0].A
    rows = R.ts_rows(c.n, c.m, c.l)
    b = np.where(ref.active0, r[rows], 0.0)
    res = {s: np.linalg.norm(b - A0 @ ref.vcycles(b, 1, s)) for s in (1, 2)}
    print(f"residual {name}: |b| {np.linalg.norm(b):.3e} sweeps 1 {res[1]:.3e} sweeps 2 {res[2]:.3e}")
    assert res[2] <= res[1], res
    b2 = np.where(ref.active0, R.ts_only(cf.synthetic_vector(c, seed=4))[rows], 0.0)
    z = ref.vcycles(2.5 * b + b2, 1, 2)
    zl = 2.5 * ref.vcycles(b, 1, 2) + ref.vcycles(b2, 1, 2)
    assert np.max(np.abs(z - zl)) <= 1e-12 * np.max(np.abs(zl))
