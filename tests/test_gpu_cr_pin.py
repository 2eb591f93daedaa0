"""The block cyclic reduction and its Gauss-Jordan inverse, bitwise against a recording of the
unit they were split from.

csrc/schur_cr.hip was one unit; it is now four: cr_inv.hip (the batched Gauss-Jordan), cr_plan.hip
(host: level geometry, the apply steps' expressions and packing, cr_init), cr_factor.hip (set-up)
and schur_cr.hip (the apply).  Every kernel kept its arithmetic and its launch, and the set-up kept
the order of its allocations and launches, so no bit may move: tests/golden/cr_parent.npz holds what
the one-unit library computed through the hooks of tests/dense_hooks.py, recorded by record() twice
in separate processes on an MI355X.  The two recordings agreed bitwise in every case (every sum of
these kernels runs in a fixed order), so every case is pinned by int64-view equality; none had to be
dropped.  The file holds this project's own output only.  The systems are tests/cr_ref.py's, seeded.

Cases:
* solve: every cr_ref.CR_CASES system -- CR_CHAIN (m = 5, every level count, both periodicities,
  tail on and off: odd counts, the periodic-pair merge, n = 1), CR_TAILPOS, CR_RC4, CR_RC8,
  CR_INVLEV, CR_TAILEDGE (every k_cr_pk<RC, CPT>, every tail position, every k_cr_inv class) --
  x, xT, the plan and info;
* expand: the six systems of test_cr_expand_from_nine_point_rows (k_cr_expand), the same;
* reuse: the test_cr_reuse systems factorised second on a SchurCR that held another matrix
  (iemic_test_cr_refactor), x;
* gj: the first "random" block of each k_cr_inv template class (m = 32 ... 192) and of m = 17 "tie",
  as the SHA-256 of the inverse's bytes (the file stays below 1 MiB), and info.
"""
import hashlib
import os

import numpy as np
import pytest

import cr_ref as R
import dense_hooks as H
from helpers import golden_landm
from iemic import config as cf

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cr_parent.npz")

EXPAND = [(2, 1, 1), (3, 1, 1), (6, 0, 1), (6, 1, 1), (6, 1, 0), (40, 1, 0)]
REUSE = [(45, 5, 1, 1), (45, 5, 1, 60), (12, 5, 1, 0), (80, 97, 1, 0)]
GJ = [(m, "random") for m in (32, 64, 96, 128, 160, 192)] + [(17, "tie")]
CASES = [("solve",) + c for c in R.CR_CASES] + [("expand",) + c for c in EXPAND] + \
        [("reuse",) + c for c in REUSE] + [("gj",) + c for c in GJ]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def h():
    """any single-rank context serves: the test6x6x4 ocean"""
    from iemic.ocean import Ocean
    oc = Ocean(cf.preset("test6x6x4", mixing=0), landm=golden_landm("test6x6x4"))
    yield oc._h
    oc.close()


def key(case):
    return "_".join(str(v) for v in case)


def plan_array(p):
    return np.array([p.nlev, p.lt, p.tM, p.ncomp, p.nsteps] + [v for s in p.down + p.up for v in s], dtype=np.int64)


def solved(case, rc, x, xT, info, plan):
    assert rc == 0, H.last_error()
    k = key(case)
    return {f"{k}_x": bits(x[0]), f"{k}_xT": bits(xT[0]), f"{k}_plan": plan_array(plan),
            f"{k}_info": np.array([info], dtype=np.int64)}


def run(h, case):
    """the arrays of one case, keyed as the recording"""
    kind, k = case[0], key(case)
    if kind == "solve":
        n, m, per, tm = case[1:]
        D, L, Rb, A, b, _, _ = R.cr_system(n, m, per)
        return solved(case, *H.cr_solve(h, n, m, per, tm, b[None, :], D, L, Rb, want_xT=True))
    if kind == "expand":
        n, per, tm = case[1:]
        m = 33 if n == 40 else 9
        S9, col, A, _ = R.build_s9(n, m, per, 40 + n + per)
        b = R.build_rhs(A, n)[0]
        return solved(case, *H.cr_solve(h, n, m, per, tm, b[None, :], S9=S9, col_of_ij=col, want_xT=True))
    if kind == "reuse":
        n, m, per, tm = case[1:]
        D, L, Rb, A, b, _, _ = R.cr_system(n, m, per)
        rc, x = H.cr_refactor(h, n, m, per, tm, R.build_blocks(n, m, 4242 + n), (D, L, Rb), b)
        assert rc == 0, H.last_error()
        return {f"{k}_x": bits(x)}
    m, what = case[1:]
    rc, X, info = H.cr_inverse(h, R.gj_blocks(m, what), 0, 1, 1)
    assert rc == 0, H.last_error()
    sha = hashlib.sha256(np.ascontiguousarray(X[0]).tobytes()).digest()
    return {f"{k}_sha": np.frombuffer(sha, dtype=np.uint8).copy(), f"{k}_info": np.array([info], dtype=np.int64)}


def record(h):
    """every case's arrays"""
    out = {}
    for case in CASES:
        out.update(run(h, case))
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@pytest.mark.parametrize("case", CASES, ids=key)
def test_cr_is_the_recorded_one(h, golden, case):
    """solution, transposed solution, plan and info (Gauss-Jordan: the inverse's hash) equal to the
    recording, bit for bit"""
    got = run(h, case)
    assert got and set(got) <= set(golden)
    for k in sorted(got):
        a, g = got[k], golden[k]
        print(f"{k}: differing entries {int(np.count_nonzero(a != g)) if a.shape == g.shape else -1} of {g.size}")
        assert a.dtype == g.dtype and np.array_equal(a, g)


def test_recording_covers_the_cases(golden):
    """nothing recorded is left unchecked, every solve was regular, and the solutions are numbers"""
    want = set()
    for case in CASES:
        want |= {f"{key(case)}_{s}" for s in {"solve": ("x", "xT", "plan", "info"), "expand": ("x", "xT", "plan", "info"),
                                              "reuse": ("x",), "gj": ("sha", "info")}[case[0]]}
    assert set(golden) == want
    for k, g in golden.items():
        if k.endswith("_info"):
            assert g[0] == 0, k
        if k.endswith("_x") or k.endswith("_xT"):
            v = g.view(np.float64)
            assert np.all(np.isfinite(v)) and np.any(v != 0), k
