"""The Krylov machinery of csrc/krylov.hip, spmv.hip and idrs.hip against independent computations.

1. FGMRES iterates: with a fixed linear preconditioner the k-th iterate is defined by
   (A, M, b) alone, so the device solver (DCGS2 or DGKS, full-length or compressed basis,
   whatever its summation order) must reproduce the plain numpy reference of
   tests/krylov_ref.py: iteration count, true residual, Givens estimate and the iterate.
2. State reused across solves on one context (the Krylov work space outlives a solve): a
   sequence of solves ends bitwise where a fresh context's single solve ends.
3. The device vector algebra (DeviceOps) against exact sums.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from helpers import golden_landm, mask_fix
from iemic import config as cf
from krylov_ref import csr_operator, fgmres_ref

pytestmark = pytest.mark.gpu

KS = (13, 8, 5, 2, 1)          # k = 1: the jj == m branch of the DCGS2 loop (no next candidate);
                               # the others: nvec mod 4 = 0..3 in the update kernels' tails
                               # and in k_dcgs_dot's groups of DCGS_DG = 4
RESTART = (5, 2)               # m = 5, 2 restarts: three cycles, 15 steps
RHO_MIN = 1e-3                 # residuals are compared relatively at or above this only

# Preconditioner 0 (issue: three orders above the reference's own float64-longdouble spread)
TOL0_RHO, TOL0_X = 1e-12, 1e-11
# Preconditioner 2: 100 x the larger measured reference spread, see
# test_preconditioned_reference_spread (which keeps these numbers honest)
TOLP_RHO, TOLP_X = 2.4e-7, 5.6e-7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _land_rows(c, L):
    Li = L[1:-1, 1:-1, 1:-1].reshape(-1)
    return np.repeat(Li != 0, 6)


@pytest.fixture(scope="module")
def Ocean():
    from iemic.ocean import Ocean
    return Ocean


_SYS = {}


def system(orc, name, seed=None):
    """The oracle's J at the synthetic state (amp_ts = 1e-3) and b = J . synthetic_vector(5);
    computed once per grid and shared."""
    key = (name, seed)
    if key not in _SYS:
        c = cf.preset(name, mixing=0)
        L0 = golden_landm(name)
        L = mask_fix(orc, c, L0)
        o = orc.Oracle(c.ref_dict(), L, c.par_list())
        x = cf.synthetic_state(c, L, amp_ts=1e-3) if seed is None else cf.synthetic_state(c, L, seed=seed, amp_ts=1e-3)
        ov, _ = o.jacobian(x)
        b = o.spmv(ov, cf.synthetic_vector(c, seed=5))
        for a in (x, ov, b):
            a.setflags(write=False)
        _SYS[key] = dict(c=c, L0=L0, L=L, o=o, x=x, ov=ov, b=b,
                         AL=csr_operator(o.rowptr, o.col, ov, np.longdouble),
                         A64=csr_operator(o.rowptr, o.col, ov, np.float64))
    return _SYS[key]


def context(Ocean, s, **sp):
    oc = Ocean(s["c"], landm=s["L0"], solver_params=sp)
    oc.setState(s["x"])
    oc.computeJacobian()
    return oc


def solve(oc, b, **sp):
    oc.solver_params.update(sp)
    x = oc.solve(b).copy()
    return x, oc.last_solve


def relres(s, x, b=None):
    b = s["b"] if b is None else b
    return np.linalg.norm(b - s["o"].spmv(s["ov"], x)) / np.linalg.norm(b)


def rel(a, ref):
    ref = np.asarray(ref)
    d = (np.asarray(a, dtype=ref.dtype) - ref).astype(np.float64)
    return float(np.linalg.norm(d) / np.linalg.norm(ref.astype(np.float64)))


def known_rows(s):
    """identity rows of J: a single entry, 1 on the diagonal (the block GS's rule)"""
    o, ov = s["o"], s["ov"]
    diag = o.col == np.repeat(np.arange(o.N), np.diff(o.rowptr))
    off = np.add.reduceat(((ov != 0) & ~diag).astype(np.int64), o.rowptr[:-1])
    d = np.add.reduceat(np.where(diag, ov, 0.0), o.rowptr[:-1])
    return (off == 0) & (d == 1.0)


def reference(s, M, reduced, dtype=np.longdouble):
    """(x_k for k = 1..13, x after the three cycles of GMRES(5)), each with its
    ||b - A x|| / ||b||.  reduced: the compressed path's statement of the problem --
    x = t on the identity rows of J (t = b there), and GMRES on b' = b - J t for the rest --
    which is another iterate than GMRES on b itself whenever t != 0."""
    A = s["AL"] if dtype == np.longdouble else s["A64"]
    b = np.asarray(s["b"]).astype(dtype)
    t = np.zeros_like(b)
    if reduced:
        kn = known_rows(s)
        t[kn] = b[kn]
    bp = b - A(t)
    one = fgmres_ref(A, M, bp, max(KS), 0, dtype)
    rst = fgmres_ref(A, M, bp, RESTART[0], RESTART[1], dtype)
    bn = np.sqrt(b @ b)
    out = {}
    for k in KS:
        x = one.x_steps[k - 1] + t
        out[k] = (x, np.sqrt((b - A(x)) @ (b - A(x))) / bn)
    x = rst.x_cycles[-1] + t
    out["restart"] = (x, np.sqrt((b - A(x)) @ (b - A(x))) / bn)
    return out


def check_iterates(s, oc, ref, tol_rho, tol_x, label, rho_all=True, **sp):
    """every k (descending) and the restarted case on one context; all figures are printed
    before anything is asserted.  A residual is compared only where the reference's is at
    least RHO_MIN (a relative error of a smaller one measures the rounding of x, not the
    solver); rho_all: every case must be such a one, otherwise at least k = 1 and 2."""
    bad = []
    cases = [(k, k, 0) for k in KS] + [("restart", RESTART[0], RESTART[1])]
    for key, m, rs in cases:
        x, info = solve(oc, s["b"], **{"FGMRES tolerance": 0.0, "FGMRES iterations": m,
                                       "FGMRES restarts": rs}, **sp)
        xr, rho = ref[key]
        rho = float(rho)
        it = m * (rs + 1)
        e_true = abs(relres(s, x) - rho) / rho
        e_impl = abs(info.implicit_rel_res - rho) / rho
        e_x = rel(x, xr)
        print(f"{label} {key}: iters {info.iters} rho {rho:.6e} true {e_true:.2e} "
              f"implicit {e_impl:.2e} x {e_x:.2e}")
        if rho < RHO_MIN and (rho_all or key in (1, 2)):
            bad.append((key, "reference rho below 1e-3", rho))
        if info.iters != it:
            bad.append((key, "iters", info.iters, it))
        if rho >= RHO_MIN and not e_true <= tol_rho:
            bad.append((key, "true residual", e_true))
        if rho >= RHO_MIN and not e_impl <= tol_rho:
            bad.append((key, "implicit residual", e_impl))
        if not e_x <= tol_x:
            bad.append((key, "iterate", e_x))
    assert not bad, bad


# The dot pass k_dcgs_dot1 walks the basis in chunks of 256 x DOT1_E = 1024 16-byte elements
# (NQ / 2 of them per vector) dealt to min(1024, chunks) workgroups:
#   test6x6x4   full basis  NQ =     864:   432 elements,   1 chunk (partial)
#   gateway16   full basis  NQ =  24,576: 12,288 elements,  12 chunks, all full
#   global4     full basis  NQ = 262,656: 131,328 elements, 129 chunks, the last with 256
#   test6x6x4   compressed  NQ =     720 (120 active cells):   360 elements, 1 chunk (partial)
#   gateway16   compressed  NQ =  20,352 (3,392 active cells): 10,176 elements, 10 chunks,
#               the last with 960 (asserted below from active_cells())
CHUNK = 1024


@pytest.mark.parametrize("orth", ["DCGS2", "DGKS"])
@pytest.mark.parametrize("name", ["test6x6x4", "gateway16", "global4"])
def test_fgmres_iterates_unpreconditioned(oracle_lib, Ocean, name, orth):
    """Preconditioner 0: the full-length basis (k_dcgs_dot1 / k_dcgs_coef / k_dcgs_update
    without staging; k_mdot / k_mupdate_norm; k_scale_copy, k_mupdate_add) against the
    longdouble reference (global4: the float64 one, 2e-15 from it and much faster)."""
    s = system(oracle_lib, name)
    nel = s["c"].nrows // 2
    assert {"test6x6x4": nel < CHUNK, "gateway16": nel == 12 * CHUNK,
            "global4": nel == 128 * CHUNK + 256}[name]
    ref = reference(s, None, False, np.float64 if name == "global4" else np.longdouble)
    oc = context(Ocean, s, Preconditioner=0)
    check_iterates(s, oc, ref, TOL0_RHO, TOL0_X, f"{name} prec 0 {orth}", Orthogonalization=orth)


@pytest.mark.parametrize("orth", ["DCGS2", "DGKS"])
@pytest.mark.parametrize("name", ["test6x6x4", "gateway16"])
def test_fgmres_iterates_block_gs(oracle_lib, Ocean, name, orth):
    """Preconditioner 2.  DCGS2: the compressed basis (k_known_part, k_cgather, the rrP
    staging of k_dcgs_update, k_spmv7c, gs_apply_c); DGKS: the same operator through
    prec_apply on full-length vectors.  The reference's M is applyPrecon of the same context
    (the unstaged apply, pinned to its CPU twin in test_gpu_parity.py), so what is compared is
    the Krylov machinery and the compressed / staged route.  The compressed path solves the
    reduced problem (x = b on J's identity rows, GMRES on b' = b - J t), whose k-th iterate is
    not that of GMRES on b: the reference states the same reduction, and the land rows of x
    are asserted to equal b bitwise, which only the reduced path gives.

    Tolerances TOLP_RHO = 2.4e-7, TOLP_X = 5.6e-7: applyPrecon is linear to ~1e-9 only, so M is
    not one operator to rounding; 100 x the larger of the two spreads measured by
    test_preconditioned_reference_spread (figures in its docstring).  The device's own distance
    from the reference on the MI355X: at most 3.1e-14 on x and 8.5e-15 on rho.

    The block GS is a strong preconditioner: the reference's rho_k is 2.7e-2, 4.2e-3, 5.7e-5,
    5.5e-7, 1.8e-10 (test6x6x4) and 9.1e-3, 2.3e-3, 5.7e-5, 4.6e-6, 1.3e-7 (gateway16) at
    k = 1, 2, 5, 8, 13, and no setting of its passes keeps rho_13 above 1e-3 on both grids.
    Residuals below 1e-3 carry the rounding of x (1e-8 relative at 1e-10) and are not
    compared; k = 1 and 2 must be, and are, above it.  The iteration count and the iterate are
    compared at every k and after the restarts."""
    s = system(oracle_lib, name)
    oc = context(Ocean, s, Preconditioner=2)
    oc.buildPreconditioner()
    cmp = orth == "DCGS2"
    ref = reference(s, oc.applyPrecon, cmp)
    nq = 6 * oc.active_cells()
    print(f"{name}: compressed basis NQ = {nq}, {nq // 2} elements, {-(-(nq // 2) // CHUNK)} chunks, "
          f"last {nq // 2 % CHUNK}")
    if name == "gateway16":
        assert nq // 2 > CHUNK and nq // 2 % CHUNK != 0    # several chunks, a partial last one
    check_iterates(s, oc, ref, TOLP_RHO, TOLP_X, f"{name} prec 2 {orth}", rho_all=False, Orthogonalization=orth)
    land = _land_rows(s["c"], s["L"])
    assert np.max(np.abs(s["b"][land])) > 0.1              # the reduced right-hand side path
    x, _ = solve(oc, s["b"], **{"FGMRES iterations": 5, "FGMRES restarts": 0})
    if cmp:
        np.testing.assert_array_equal(bits(x[land]), bits(s["b"][land]))
    else:
        assert not np.array_equal(x[land], s["b"][land])


@pytest.mark.parametrize("name", ["test6x6x4", "gateway16"])
def test_preconditioned_reference_spread(oracle_lib, Ocean, name):
    """How far two correct GMRES runs with M = applyPrecon can be apart: (a) the float64 and
    the longdouble reference, (b) two longdouble references whose M differs by a fixed 1e-9
    relative (diagonal) perturbation of its output.  100 x the larger must stay within
    TOLP_RHO / TOLP_X, the bounds test_fgmres_iterates_block_gs uses.
    Measured on the MI355X, the maximum over k in 1, 2, 5, 8, 13 and the restarted case, over
    the plain and the reduced problem (rho: the cases with rho >= 1e-3):
      test6x6x4  float64 vs longdouble  x 5.8e-15  rho 6.1e-15;  perturbed M  x 1.0e-9  rho 2.4e-9
      gateway16  float64 vs longdouble  x 3.8e-14  rho 3.7e-14;  perturbed M  x 5.5e-9  rho 1.7e-9
    The larger: x 5.52e-9, rho 2.36e-9; 100 x, rounded up: TOLP_X = 5.6e-7, TOLP_RHO = 2.4e-7."""
    s = system(oracle_lib, name)
    oc = context(Ocean, s, Preconditioner=2)
    oc.buildPreconditioner()
    M = oc.applyPrecon
    xi = 1.0 + 1e-9 * np.where(np.random.default_rng(7).random(s["c"].nrows) < 0.5, -1.0, 1.0)
    Mp = lambda v: M(v) * xi
    worst = {}
    for red in (False, True):
        base = reference(s, M, red)
        for tag, other in (("float64", reference(s, M, red, np.float64)), ("perturbed", reference(s, Mp, red))):
            dx = max(rel(other[k][0], base[k][0]) for k in base)
            dr = max(float(abs(other[k][1] - base[k][1]) / base[k][1]) for k in base if base[k][1] >= RHO_MIN)
            print(f"{name} reduced={red} {tag}: spread x {dx:.2e} rho {dr:.2e}")
            worst["x"] = max(worst.get("x", 0.0), dx)
            worst["rho"] = max(worst.get("rho", 0.0), dr)
    assert 100 * worst["x"] <= TOLP_X and 100 * worst["rho"] <= TOLP_RHO, worst


# ---- state reused across solves ---------------------------------------------------------
CONV = {"FGMRES tolerance": 1e-8, "FGMRES restarts": 20, "Solver": "FGMRES"}


def check_sequence(Ocean, s, seq, b=None, every=False, min_iters=0, prepare=None):
    """the solves of seq on one context; the last (every: each) equals, bitwise and in its
    iteration count, the same solve on a fresh context"""
    b = s["b"] if b is None else b
    oc = context(Ocean, s, Preconditioner=2)
    oc.buildPreconditioner()
    for q, sp in enumerate(seq):
        x, info = solve(oc, b, **dict(CONV, **sp))
        if not (every or q == len(seq) - 1):
            continue
        fr = context(Ocean, s, Preconditioner=2)
        fr.buildPreconditioner()
        xf, inf_f = solve(fr, b, **dict(CONV, **sp))
        res = relres(s, x, b)
        nd = int(np.count_nonzero(bits(x) != bits(xf)))
        print(f"solve {q} {sp}: iters {info.iters} (fresh {inf_f.iters}) res {res:.2e} "
              f"differing entries {nd} max |dx| {np.max(np.abs(x - xf)):.2e}")
        assert inf_f.converged == 1 and inf_f.iters > min_iters
        assert info.iters == inf_f.iters
        np.testing.assert_array_equal(bits(x), bits(xf))
        assert info.converged == 1 and res <= 1e-7
        fr.close()
    oc.close()


@pytest.mark.parametrize("first", [{"Orthogonalization": "DGKS", "Preconditioner": 2},
                                   {"Orthogonalization": "DCGS2", "Preconditioner": 1}],
                         ids=["dgks", "prec1"])
def test_reuse_stale_identity_rows(oracle_lib, Ocean, first):
    """An uncompressed solve with Krylov dimension 12 leaves identity-row values in the
    preconditioned vectors Z (the right-hand side is non-zero on land rows); a compressed solve
    with dimension 6 and then one with dimension 12 follow.  The staged applies never write
    Z's identity rows, so columns 6..11 must have been cleaned for the last solve.
    (prec1: "Preconditioner": 1 in the solve's options on a context whose block GS is built
    takes the uncompressed DCGS2 path with that same block GS through prec_apply.)"""
    s = system(oracle_lib, "gateway16")
    assert np.max(np.abs(s["b"][_land_rows(s["c"], s["L"])])) > 0.1
    cmp = {"Orthogonalization": "DCGS2", "Preconditioner": 2}
    check_sequence(Ocean, s, [dict(first, **{"FGMRES iterations": 12}),
                              dict(cmp, **{"FGMRES iterations": 6}),
                              dict(cmp, **{"FGMRES iterations": 12})], min_iters=6)


def test_reuse_grow_shrink(oracle_lib, Ocean):
    """DCGS2 with Krylov dimension 8 -> 16 -> 8: ensure_krylov reallocates Z, frees V and
    regrows the compressed basis; every solve equals a fresh context's."""
    s = system(oracle_lib, "gateway16")
    check_sequence(Ocean, s, [{"FGMRES iterations": m} for m in (8, 16, 8)], every=True)


def test_reuse_switch_solver(oracle_lib, Ocean):
    """IDR(4) -> FGMRES (DCGS2) -> IDR(4) on one context, each against a fresh one."""
    s = system(oracle_lib, "gateway16")
    idr = {"Solver": "IDR", "IDR s": 4, "FGMRES iterations": 1000, "FGMRES restarts": 0}
    check_sequence(Ocean, s, [idr, {"FGMRES iterations": 12}, idr], every=True)


def test_reuse_new_setup(oracle_lib, Ocean):
    """Solve, then another state, its Jacobian, preProcess and a solve with a larger Krylov
    dimension; the fresh context does only the second solve."""
    s, s2 = system(oracle_lib, "gateway16"), system(oracle_lib, "gateway16", seed=99)
    oc = context(Ocean, s, Preconditioner=2)
    solve(oc, s["b"], **CONV, **{"FGMRES iterations": 8})
    oc.setState(s2["x"])
    oc.computeJacobian()
    oc.preProcess()
    x, info = solve(oc, s2["b"], **CONV, **{"FGMRES iterations": 16})
    fr = context(Ocean, s2, Preconditioner=2)
    xf, inf_f = solve(fr, s2["b"], **CONV, **{"FGMRES iterations": 16})
    res = relres(s2, x)
    print(f"new set-up: iters {info.iters} (fresh {inf_f.iters}) res {res:.2e}")
    assert info.iters == inf_f.iters
    np.testing.assert_array_equal(bits(x), bits(xf))
    assert info.converged == 1 and res <= 1e-7


# ---- device vector algebra ---------------------------------------------------------------
def wide_vector(n, seed):
    """mixed signs, magnitudes 1e-150 .. 1e150"""
    r = np.random.default_rng(seed)
    return np.where(r.random(n) < 0.5, -1.0, 1.0) * 10.0 ** r.uniform(-150, 150, n)


@pytest.mark.parametrize("name", ["test6x6x4", "gateway16"])
def test_device_vector_algebra(Ocean, name):
    """DeviceOps.dot / norm / norm_inf / lincomb and the host round trip against exact sums
    (math.fsum, rationals).  864 rows: fewer than one 256-thread block per reduction slot;
    24,576 rows: 96 blocks."""
    c = cf.preset(name, mixing=0)
    oc = Ocean(c, landm=golden_landm(name))
    ops = oc.vec_ops()
    n = c.nrows
    cases = {"wide": (wide_vector(n, 1), wide_vector(n, 2)),
             "cancel": (np.random.default_rng(3).standard_normal(n), np.random.default_rng(4).standard_normal(n))}
    for tag, (x, y) in cases.items():
        x[5], x[7] = -0.0, 5e-324                     # a signed zero and a subnormal
        dx, dy = ops.from_host(x), ops.from_host(y)
        np.testing.assert_array_equal(bits(ops.to_host(dx)), bits(x))
        p = x * y
        d = ops.dot(dx, dy)
        print(f"{name} {tag}: dot error {abs(d - math.fsum(p)) / math.fsum(np.abs(p)):.2e} of sum |x y|")
        assert abs(d - math.fsum(p)) <= 1e-14 * math.fsum(np.abs(p))
        nr = math.sqrt(math.fsum(x * x))
        assert abs(ops.norm(dx) - nr) <= 1e-14 * nr
        assert ops.norm_inf(dx) == np.max(np.abs(x))
        a, b = 0.75, -1.3
        # numpy rounds a x, b y and their sum; a device compiler that contracts the second
        # product into the sum (fma) rounds a x and the exact fl(a x) + b y: one of the two
        # per entry, nothing else.  Without y, or with a zero coefficient, there is no choice.
        z = ops.to_host(ops.lincomb(a, dx, b, dy))
        plain = a * x + b * y
        ax = a * x
        fused = np.array([float(Fraction(float(u)) + Fraction(b) * Fraction(float(v))) for u, v in zip(ax, y)])
        either = (bits(z) == bits(plain)) | (bits(z) == bits(fused))
        print(f"{name} {tag}: lincomb {int(np.sum(bits(z) != bits(plain)))} entries differ from the uncontracted form")
        assert np.all(either), np.flatnonzero(~either)[:10]
        np.testing.assert_array_equal(bits(ops.to_host(ops.lincomb(a, dx))), bits(a * x))
        np.testing.assert_array_equal(bits(ops.to_host(ops.lincomb(a, dx, 0.0, dy))), bits(a * x + 0.0 * y))
        np.testing.assert_array_equal(bits(ops.to_host(ops.lincomb(0.0, dx, b, dy))), bits(0.0 * x + b * y))
        np.testing.assert_array_equal(bits(ops.to_host(ops.copy(dx))), bits(x))
    xn = cases["cancel"][0].copy()
    xn[n - 3] = np.nan
    try:
        v = ops.norm_inf(ops.from_host(xn))
    except Exception:
        v = float("nan")
    assert math.isnan(v)
