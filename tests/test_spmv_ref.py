"""Self-test of tests/spmv_ref.py, the reference tests/test_gpu_spmv_tiles.py compares the
compressed SpMV, its tile descriptors and the dynamics defect with.  No GPU.

1. The five grids still produce every tile class the GPU tests rely on (a condition on the
   land-mask design: a later change of the mask cannot empty a case without notice).
2. The descriptors equal a second, cell-by-cell statement of them.
3. The derived error bound discriminates: a float64 product passes it, one with x shifted by a
   cell or with one coefficient dropped misses it by at least 1e3.
"""
import numpy as np
import pytest

import spmv_ref as R
from krylov_ref import csr_operator

GRID_IDS = [R.grid_id(g) for g in R.ALL_GRIDS]

# counts over every (grid row, tile) of the design, computed on the CPU oracle; nc: the cells of
# the partial last tile; fixed: cells mask_fix turns to land
#              nact  fixed nc   full partial lane0 lane63 end<=19 start23-43 start>=44 holes empty
TABLE = {
    (130, True): (1023, 0, 2, (12, 13, 6, 6, 31, 8, 12, 4, 59)),
    (130, False): (1023, 0, 2, (12, 13, 6, 6, 31, 8, 12, 4, 59)),
    (65, True): (584, 0, 1, (6, 24, 24, 6, 24, 2, 12, 10, 30)),
    (64, True): (560, 6, 64, (6, 0, 0, 0, 0, 2, 6, 10, 18)),
    (63, False): (548, 0, 63, (0, 24, 0, 0, 0, 2, 6, 10, 18)),
    R.EDGES: (865, 0, 64, (0, 0, 0, 0, 6, 12, 6, 1, 0)),
}


def system(orc, g):
    s = R.grid(orc, *g)
    if "tiles" not in s:
        s["kn"] = R.identity_rows(s["o"], s["ov"][0])
        s["tiles"] = R.tiles(s["n"], s["kn"], s["o"].rowintcon)
    return s


@pytest.mark.parametrize("g", R.ALL_GRIDS, ids=GRID_IDS)
def test_tile_classes(oracle_lib, g):
    s = system(oracle_lib, g)
    T = s["tiles"]
    nact, fixed, nc, counts = TABLE[g]
    print(g, len(T.act), s["fixed"], T.klass)
    assert len(T.act) == nact and s["fixed"] == fixed
    assert g[0] - (-(-g[0] // 64) - 1) * 64 == nc
    assert tuple(T.klass[k] for k in R.CLASSES) == counts
    assert s["o"].rowintcon >= 0 and T.ric >= 0
    # the second state keeps the identity rows: the active list outlives the second Jacobian
    assert np.array_equal(R.identity_rows(s["o"], s["ov"][1]), s["kn"])
    assert not np.array_equal(s["ov"][0], s["ov"][1])


def test_every_class_is_reached(oracle_lib):
    """the conditions the GPU tests rest on, over the five grids together"""
    tl = {g: system(oracle_lib, g)["tiles"] for g in R.GRIDS}
    for k in R.CLASSES:
        assert sum(t.klass[k] for t in tl.values()) > 0, k
    # the added grid: the first and last active lanes of spmv_ref.EDGE_SPANS (the integral
    # condition's cell adds lane 63 to one tile of the last span)
    e = system(oracle_lib, R.EDGES)["tiles"].atl[:, 1]
    assert {(int(v) & 255, int(v) >> 8) for v in e} == set(R.EDGE_SPANS) | {(22, 63)}
    # partial last tiles of 1, 2 and 63 cells, and a grid of whole tiles only
    assert {g[0] % 64 for g in R.GRIDS} == {2, 1, 0, 63}
    # the active list ends inside a block of 64 (k_spmv_dyn, k_dyn_pack) on every grid
    assert all(len(t.act) % 64 != 0 for t in tl.values())
    assert {len(t.act) % 64 for t in tl.values()} >= {63, 8}
    # an active lane above 15 and above 31 (the mask's popcount, both mask words)
    assert any(((t.atl[:, 1] >> 8) > 31).any() for t in tl.values())
    # the integral-condition row in a cell that is active through it alone (n = 130), and in
    # an ocean cell (the others)
    for g, t in tl.items():
        s = system(oracle_lib, g)
        cell = s["o"].rowintcon // R.NUN
        others = np.delete(s["kn"][R.NUN * cell: R.NUN * cell + R.NUN], s["o"].rowintcon % R.NUN)
        assert others.all() == (g[0] == 130)
        wet = int(np.count_nonzero(s["L"][1:-1, 1:-1, 1:-1] == 0))
        assert len(t.act) == wet + (1 if g[0] == 130 else 0)


@pytest.mark.parametrize("g", R.ALL_GRIDS, ids=GRID_IDS)
def test_descriptors_cell_by_cell(oracle_lib, g):
    """the same records from loops over rows, cells and lanes"""
    s = system(oracle_lib, g)
    o, ov, n, T = s["o"], s["ov"][0], s["n"], s["tiles"]
    m, l = R.M, R.L

    def identity(r):
        nz = [(int(o.col[p]), ov[p]) for p in range(o.rowptr[r], o.rowptr[r + 1]) if ov[p] != 0.0]
        return r != o.rowintcon and nz == [(r, 1.0)]

    act, recs, cm = [], [], {}
    for j in range(m):
        for k in range(l):
            for i in range(n):
                cell = (k * m + j) * n + i
                if not all(identity(6 * cell + v) for v in range(6)):
                    cm[(j, k, i)] = len(act)
                    act.append((j * l + k) * n + i)
    tpr = (n + 63) // 64
    for j in range(m):
        for k in range(l):
            for ti in range(tpr):
                on = [q for q in range(64) if (j, k, ti * 64 + q) in cm]
                if not on:
                    continue
                mask = sum(1 << q for q in on)
                words = [int(np.array(w, dtype=np.uint32).astype(np.int32)) for w in (mask & 0xFFFFFFFF, mask >> 32)]
                a0 = cm[(j, k, ti * 64 + on[0])]
                assert cm[(j, k, ti * 64 + on[-1])] == a0 + len(on) - 1
                recs.append([(j * l + k) * tpr + ti, on[0] | (on[-1] << 8), a0, len(on), *words, 0, 0])
    assert np.array_equal(T.act, np.array(act, dtype=np.int32))
    assert np.array_equal(T.atl, np.array(recs, dtype=np.int32))
    ci = o.rowintcon // 6
    key = ((ci // n) % m, ci // (n * m), ci % n)
    assert T.ric == 6 * cm[key] + o.rowintcon % 6
    # consecutive tiles tile the compressed vector
    assert T.atl[0, 2] == 0 and np.array_equal(T.atl[1:, 2], np.cumsum(T.atl[:, 3])[:-1])
    assert T.atl[:, 3].sum() == len(act)


def active_rows(s):
    cells = R.owned_to_ref(s["n"])[s["tiles"].act]
    return ((R.NUN * cells)[:, None] + np.arange(R.NUN)[None, :]).reshape(-1)


@pytest.mark.parametrize("g", R.ALL_GRIDS, ids=GRID_IDS)
def test_bound_holds_for_float64_and_discriminates(oracle_lib, g):
    from iemic import config as cf
    s = system(oracle_lib, g)
    o, ov = s["o"], s["ov"][0]
    x = cf.synthetic_vector(s["c"], seed=11)
    assert np.all(x != 0.0)
    pr = R.product(o, ov, x)
    A64 = csr_operator(o.rowptr, o.col, ov, np.float64)
    ok = R.ratio(A64(x), pr.y, pr.bound)
    rows = active_rows(s)
    # x one cell off (the cell is the fastest index of the reference order): what a tile
    # computes when its staged x is shifted by a cell
    sh = R.ratio(A64(np.roll(x, R.NUN)), pr.y, pr.bound)
    print(f"{g}: float64 product {ok.max():.3f} of the bound; x shifted by a cell: at least "
          f"{sh[rows].min():.2e} of it on the active cells' rows")
    assert ok.max() <= 1.0
    for rec in s["tiles"].atl:                      # every launched tile, each on its own rows
        a = np.arange(rec[2], rec[2] + rec[3])
        tr = ((R.NUN * R.owned_to_ref(s["n"])[s["tiles"].act[a]])[:, None] + np.arange(R.NUN)).reshape(-1)
        assert sh[tr].min() >= 1e3, rec
    # one coefficient dropped in one row: the first launched tile's first non-identity row,
    # its first off-diagonal non-zero
    r = next(int(q) for q in rows if not s["kn"][q] and q != o.rowintcon)
    p = next(p for p in range(o.rowptr[r], o.rowptr[r + 1]) if ov[p] != 0.0 and o.col[p] != r)
    v = ov.copy()
    v[p] = 0.0
    dr = R.ratio(csr_operator(o.rowptr, o.col, v, np.float64)(x), pr.y, pr.bound)
    # the same for every non-zero of every active row, without the float64 run: dropping
    # term e moves the row by |a_e x_e|
    term = np.abs(ov * x[o.col])
    rr = np.repeat(np.arange(o.N), np.diff(o.rowptr))
    on = (ov != 0) & np.isin(rr, rows)
    each = term[on] / pr.bound[rr[on]]
    print(f"{g}: row {r} without its entry at column {o.col[p]}: {dr[r]:.2e} of the bound; over all "
          f"{on.sum()} non-zeros of the active rows: at least {each.min():.2e}, "
          f"{np.mean(each >= 1e3):.4f} of them at 1e3 or more")
    assert dr[r] >= 1e3 and np.all(np.delete(dr, r) <= 1.0)
    # the largest term of every active row is always seen
    big = np.zeros(o.N)
    np.maximum.at(big, rr[on], each)
    assert big[rows].min() >= 1e3


@pytest.mark.parametrize("g", R.ALL_GRIDS, ids=GRID_IDS)
def test_planar_round_trip_and_defect(oracle_lib, g):
    """to_planar / from_planar against the index formula, and defect_expected's shape"""
    from iemic import config as cf
    s = system(oracle_lib, g)
    n, m, l = s["n"], R.M, R.L
    z = cf.synthetic_vector(s["c"], seed=21)
    ps = n * l * (m + 4)
    P = R.to_planar(n, z, np.nan)
    for (i, j, k, v) in ((0, 0, 0, 0), (n - 1, m - 1, l - 1, 5), (n // 2, 3, 1, 2)):
        assert P[(j + 2) * l * n + k * n + i + v * ps] == z[6 * ((k * m + j) * n + i) + v]
    assert np.count_nonzero(np.isnan(P)) == 6 * 4 * l * n
    assert np.array_equal(R.from_planar(n, P), z.reshape(-1, 6)[R.owned_to_ref(n)])
    rr = cf.synthetic_vector(s["c"], seed=22)
    exp, bound = R.defect_expected(n, s["o"], s["ov"][0], s["kn"], s["tiles"].act, z, rr)
    assert exp.shape == bound.shape == (len(s["tiles"].act), 4)
    assert np.all((bound == 0) == (exp == 0))
    # the two Jacobians' defects are far apart on some row: the two-buffer test can tell them apart
    exp2, _ = R.defect_expected(n, s["o"], s["ov"][1], s["kn"], s["tiles"].act, z, rr)
    with np.errstate(divide="ignore", invalid="ignore"):
        far = np.where(bound > 0, np.abs(exp2 - exp).astype(np.float64) / bound, 0.0)
    assert far.max() >= 1e3
