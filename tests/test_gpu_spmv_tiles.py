"""The compressed SpMV k_spmv7c with its coefficient pack k_spmv_pack, the tile descriptors of
act_tiles, the full SpMV k_spmv7 and the dynamics defect k_spmv_dyn with its pack k_dyn_pack,
each called on its own through the test hooks (iemic_test_active_set, iemic_test_spmv_c,
iemic_test_dyn_defect) and compared with the longdouble reference of tests/spmv_ref.py.

The five grids (n x 14 x 3, at most 5,460 cells) are the smallest whose 64-cell tiles reach
every branch: whole tiles, last tiles of 1, 2 and 63 cells, a single active lane 0 or 63, active
runs that end by lane 19 or start at lane 23 / 44 (staging pieces skipped), holes in the mask,
empty tiles, an active list that ends inside a block of 64, and the integral-condition row in
a cell with no other live row (tests/test_spmv_ref.py asserts that the grids keep doing so).
A sixth grid (64 x 14 x 3, "edges") puts the ends of the active runs on those lanes exactly (last
19, first 23 / 44), on the lanes whose own 48 bytes lie in two staging pieces (21 and 42, as the
last and as the first lane) and one lane inside them (22, 41).  With the staged window cut by
one cell on either side (a deliberate, memory-safe change of k_spmv7c's blo / bhi, not kept)
this grid and three of the five fail the bitwise and the longdouble tests.

Tolerances are derived, not measured (spmv_ref's docstring): (p + 1) 2^-53 sum |a x| for a row
of p non-zero coefficients (the integral-condition row included: p its non-zero
coefficients), (p + 2) 2^-53 (|rr| + sum |a z|) for the defect.

Every device call of a grid is made once, when its record is built: set-up at the first state,
the three hooks, a second Jacobian (another state, the preconditioner not rebuilt) and the two
hooks again.  The tests assert on the record, so they do not depend on their order.
"""
import numpy as np
import pytest

import dense_hooks as dh
import spmv_ref as R
from iemic import config as cf

pytestmark = pytest.mark.gpu

GRID_IDS = [R.grid_id(g) for g in R.ALL_GRIDS]
_REC = {}


@pytest.fixture(scope="module", autouse=True)
def _records():
    yield
    for r in _REC.values():
        r["oc"].close()
    _REC.clear()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def record(orc, g):
    from iemic.ocean import Ocean
    if g in _REC:
        return _REC[g]
    s = R.grid(orc, *g)
    c, n, o = s["c"], s["n"], s["o"]
    oc = Ocean(c, landm=s["L0"], solver_params={"Preconditioner": 2, "TS multigrid cycles": 0, "TS sweeps": 1})
    x = cf.synthetic_vector(c, seed=11)
    assert np.all(x != 0.0)
    z, rr = cf.synthetic_vector(c, seed=21), cf.synthetic_vector(c, seed=22)
    assert np.all(z.reshape(-1, 6)[:, 4:] != 0.0)             # the W row reads T and S
    NE = oc.layout()["ext_rows"]
    assert NE == 6 * n * R.L * (R.M + 2 * R.HALO)
    # the halo rows carry other random numbers: no coefficient may reach them
    fill = np.random.default_rng(5).uniform(-1.0, 1.0, (2, NE))
    zP, rP = R.to_planar(n, z, fill[0]), R.to_planar(n, rr, fill[1])
    rec = dict(s=s, oc=oc, x=x, z=z, rr=rr, NE=NE, spmv=[], dyn=[], csr=[])
    for q in range(2):
        oc.setState(s["x"][q])
        oc.computeJacobian()
        if q == 0:
            oc.buildPreconditioner(force=True)
            rec["desc"] = dh.active_set(oc._h)
            rec["active_cells"] = oc.active_cells()
        rec["csr"].append(oc.exportCSR()[2].copy())
        rec["spmv"].append(dh.spmv_c(oc._h, x, rec["desc"][0]))
        rec["dyn"].append(dh.dyn_defect(oc._h, zP, rP))
    rec["desc_after"] = dh.active_set(oc._h)
    rec["kn"] = R.identity_rows(o, s["ov"][0])
    rec["tiles"] = R.tiles(n, rec["kn"], o.rowintcon)
    rec["prod"] = [R.product(o, s["ov"][q], x) for q in range(2)]
    _REC[g] = rec
    return rec


@pytest.mark.parametrize("g", R.ALL_GRIDS, ids=GRID_IDS)
def test_descriptors(oracle_lib, g):
    """nact, natile, ric, the active list and every tile record == the reference, exactly; the
    second Jacobian (same identity rows) leaves them as they are"""
    rec = record(oracle_lib, g)
    T = rec["tiles"]
    nact, natile, ric, act, atl = rec["desc"]
    assert (nact, natile, ric) == (len(T.act), len(T.atl), T.ric)
    np.testing.assert_array_equal(act, T.act)
    np.testing.assert_array_equal(atl, T.atl)
    assert rec["active_cells"] == nact
    for a, b in zip(rec["desc"], rec["desc_after"]):
        np.testing.assert_array_equal(a, b)
    # the device's Jacobians are the oracle's, so the reference speaks of the same operator
    for q in range(2):
        np.testing.assert_array_equal(rec["csr"][q], rec["s"]["ov"][q])


def compressed_rows(rec):
    """reference rows of the compressed vector's entries"""
    cells = R.owned_to_ref(rec["s"]["n"])[rec["tiles"].act]
    return ((R.NUN * cells)[:, None] + np.arange(R.NUN)[None, :]).reshape(-1)


def check_bitwise(rec, q):
    yc, y, guard = rec["spmv"][q]
    rows = compressed_rows(rec)
    assert guard == 0, "k_spmv7c wrote outside its 6 nact rows"
    assert not np.isnan(yc).any(), np.flatnonzero(np.isnan(yc))[:10]
    same = bits(yc) == bits(y[rows])
    same[rec["tiles"].ric] = True                  # the integral condition: a reduction of its own
    assert same.all(), (np.flatnonzero(~same)[:10], yc[~same][:10], y[rows][~same][:10])


def check_bound(rec, q, label):
    """both kernels against the longdouble J x of Jacobian q -> the two largest ratios"""
    yc, y, _ = rec["spmv"][q]
    pr = rec["prod"][q]
    rows = compressed_rows(rec)
    rf = R.ratio(y, pr.y, pr.bound)
    rc = R.ratio(yc, pr.y[rows], pr.bound[rows])
    ic = rec["s"]["o"].rowintcon
    print(f"{label}: k_spmv7 {rf.max():.3f} of the bound (row {rf.argmax()}), k_spmv7c {rc.max():.3f} "
          f"(compressed row {rc.argmax()}), integral condition {rf[ic]:.2e} / {rc[rec['tiles'].ric]:.2e}")
    assert rf.max() <= 1.0, (rf.argmax(), y[rf.argmax()], pr.y[rf.argmax()])
    assert rc.max() <= 1.0, (rc.argmax(), yc[rc.argmax()], pr.y[rows][rc.argmax()])
    return rf.max(), rc.max()


@pytest.mark.parametrize("g", R.ALL_GRIDS, ids=GRID_IDS)
def test_compressed_rows_bitwise_full(oracle_lib, g):
    """row 6 a + R of k_spmv7c == row 6 act[a] + R of k_spmv7 on the same device x, bit for bit
    (DESIGN.md section 3), the integral-condition entry excepted; nothing left unwritten, nothing
    written outside"""
    check_bitwise(record(oracle_lib, g), 0)


@pytest.mark.parametrize("g", R.ALL_GRIDS, ids=GRID_IDS)
def test_both_against_longdouble(oracle_lib, g):
    """k_spmv7 on every row of the grid (land included) and k_spmv7c on every compressed row
    within (p + 1) 2^-53 sum |a x| of the longdouble product.
    Largest |error| / bound measured on the MI355X (the same for k_spmv7 and k_spmv7c, which are
    bitwise equal; in brackets the integral-condition row's, again the same for both), first
    and second Jacobian alike:
      n130p 0.432 (7.65e-5)   n130 0.432 (7.65e-5)   n65p 0.469 (8.19e-5)
      n64p  0.431 (3.00e-5)   n63  0.509 (4.21e-5)   n64edges 0.507 (3.04e-5)"""
    rec = record(oracle_lib, g)
    check_bound(rec, 0, f"{R.grid_id(g)} first Jacobian")
    # land rows are identity rows: x itself, exactly
    yc, y, _ = rec["spmv"][0]
    kn = rec["kn"]
    np.testing.assert_array_equal(bits(y[kn]), bits(rec["x"][kn]))


@pytest.mark.parametrize("g", R.ALL_GRIDS, ids=GRID_IDS)
def test_compressed_follows_new_jacobian(oracle_lib, g):
    """a second Jacobian without a new set-up: the compressed SpMV (repacked by gs_refresh) is
    that Jacobian's, bitwise k_spmv7's and within the bound of the oracle's new J"""
    rec = record(oracle_lib, g)
    check_bitwise(rec, 1)
    check_bound(rec, 1, f"{R.grid_id(g)} second Jacobian")
    assert np.any(bits(rec["spmv"][1][0]) != bits(rec["spmv"][0][0]))
    # and not the first one's: some row is far from the old product
    rows = compressed_rows(rec)
    old = R.ratio(rec["spmv"][1][0], rec["prod"][0].y[rows], rec["prod"][0].bound[rows])
    assert old.max() >= 1e3


def check_defect(rec, d, q):
    """d against rr - J_q z -> |error| / bound per (active cell, U/V/W/P row); identity rows:
    exactly 0; everything else the NaN fill"""
    s, T = rec["s"], rec["tiles"]
    n = s["n"]
    exp, bound = R.defect_expected(n, s["o"], s["ov"][q], rec["kn"], T.act, rec["z"], rec["rr"])
    D = R.from_planar(n, d)                                     # (owned cell, unknown)
    got = D[T.act][:, :4]
    return R.ratio(got, exp, bound), got


@pytest.mark.parametrize("g", R.ALL_GRIDS, ids=GRID_IDS)
def test_dyn_defect(oracle_lib, g):
    """k_spmv_dyn on the packed stream of k_dyn_pack: rr - J z on the active cells' non-identity
    U/V/W/P rows within (p + 2) 2^-53 (|rr| + sum |a z|), exactly 0 on their identity rows, nothing
    written elsewhere (T/S rows, inactive cells, halo rows).  After a second Jacobian without a
    new set-up the defect is still the set-up Jacobian's (the two-buffer rule), bit for bit.
    Largest |error| / bound measured on the MI355X (after either Jacobian):
      n130p 0.446   n130 0.446   n65p 0.413   n64p 0.377   n63 0.516   n64edges 0.381"""
    rec = record(oracle_lib, g)
    T, n = rec["tiles"], rec["s"]["n"]
    assert len(T.act) % 64 != 0                                 # a partial last block
    for q in range(2):
        d = rec["dyn"][q]
        r0, got = check_defect(rec, d, 0)
        print(f"{R.grid_id(g)} defect after Jacobian {q + 1}: {r0.max():.3f} of the bound against the set-up J")
        assert not np.isnan(got).any()
        assert r0.max() <= 1.0, np.argwhere(r0 > 1.0)[:10]
        # written: the active cells' four dynamics rows, nothing else
        P = d.reshape(R.NUN, -1)
        wrote = ~np.isnan(P)
        want = np.zeros_like(wrote)
        want[:4, R.HALO * R.L * n + T.act] = True
        np.testing.assert_array_equal(wrote, want)
    np.testing.assert_array_equal(bits(rec["dyn"][1]), bits(rec["dyn"][0]))
    r1, _ = check_defect(rec, rec["dyn"][1], 1)
    assert r1.max() >= 1e3, "the defect follows the new Jacobian"
