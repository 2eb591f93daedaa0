"""The device's dynamics pass (gs_dyn.hip dyn_solve: k_gs_ptil_rcol, the Schur cyclic reduction,
k_gs_uvp, k_gs_pw_t) and the defect-correction recurrence around it (gs_apply_impl), through
Ocean.applyPrecon alone, against the sparse equations of tests/gs_dyn_ref.py: the output is
multiplied by M_D and every row is checked; nothing is compared with the CPU twin's output.  The
Jacobian given to the reference is the oracle's (bit-equal to the device's,
test_gpu_parity.test_jacobian_rhs_bitexact); the water columns and pin flags are BlockGS.schur()'s.

Bound per (fixture, row kind): gs_dyn_ref.bound = min(1e-8, 100 x the twin's figure), the twin's
figures being the table of tests/test_gs_dyn_ref.py; the single pass, every recurrence step and
every minimal-residual step are held to it kind by kind.  The closing P rows are judged in the
maximum norm over their set ("s") and, for the right-hand sides that fill their rows, row by row
as well ("sr").  T and S are not judged here.

Backward error of one device pass, max over gs_dyn_ref.rhs_cases, Mixing 0 and 1 and both
"TS multigrid cycles" settings (MI355X):

    fixture            u        v        w        p        s       sr   (twin:  u        v        w        p        s       sr)
    test6x6x4    1.8e-16  2.1e-16  7.6e-17  1.2e-16  8.3e-14  3.9e-14       3.0e-16  2.8e-16  7.7e-17  1.7e-16  2.0e-15  2.5e-15
    natl8        2.0e-16  2.7e-16  1.1e-16  1.4e-16  1.5e-14  4.2e-14       4.4e-16  4.6e-16  8.1e-17  1.7e-16  1.3e-15  2.3e-15
    natl8_l8     2.0e-16  2.2e-16  6.3e-16  1.3e-16  6.3e-14  1.9e-13       4.2e-16  2.3e-16  6.3e-16  1.6e-16  1.8e-15  3.5e-15
    odd7x8x4     2.2e-16  1.8e-16  1.1e-16  1.3e-16  1.9e-14  1.7e-14       4.8e-16  5.9e-16  1.1e-16  1.4e-16  1.5e-15  9.1e-15
    gateway16    1.9e-16  2.3e-16  1.3e-15  1.7e-16  1.4e-14  4.0e-13       6.0e-16  5.8e-16  1.3e-15  1.7e-16  7.7e-15  2.8e-13
    2dmoc        1.6e-16  1.7e-16  9.1e-17  1.1e-16  5.9e-15  1.1e-14       3.6e-16  3.4e-16  1.3e-16  1.4e-16  5.4e-15  1.1e-14
    global4      2.0e-16  2.5e-16  1.1e-14  1.9e-16  2.3e-12  1.1e-11       1.1e-15  1.3e-15  1.2e-14  2.0e-16  9.6e-13  1.1e-11

The four settings of a fixture gave the same figures.  The s rows (the closing P rows, which the
Schur solve closes: gs_dyn_ref's docstring) are where the block cyclic reduction shows: up to 54 x
the twin's band LU (natl8_l8, sr), inside the margin of 100.
Recurrence steps ("Schur passes" 0, 1, 2; natl8, gateway16, global4), the largest per kind:
    u 8.3e-17 v 1.0e-16 w 1.1e-16 p 9.8e-17 s 7.8e-14 sr 1.8e-12
Two latitude bands:
    natl8: u 2.0e-16 v 2.7e-16 w 1.1e-16 p 1.4e-16 s 1.5e-14 sr 4.2e-14
    natl8 default pass 4: u 5.8e-17 v 3.4e-17 w 2.5e-17 p 2.9e-17 s 8.2e-17 sr 6.2e-16
    global4: u 2.0e-16 v 2.5e-16 w 1.1e-14 p 1.9e-16 s 2.3e-12 sr 1.1e-11
    global4 default pass 4: u 7.5e-17 v 1.0e-16 w 1.1e-16 p 5.9e-17 s 2.9e-14 sr 1.4e-12
Minimal residual (dw against 100 x the twin-driven recurrence's larger step: natl8 8.1e-13,
gateway16 3.2e-13; dq and orth against 100 x the numpy replay's):
    natl8 pass 2: w 0.947846 u 5.7e-17 v 5.2e-17 w 2.5e-17 p 4.0e-17 s 8.1e-17 sr 6.3e-16 dw 8.4e-13 dq 9.6e-14 orth 9.6e-15
    gateway16 pass 2: w 0.949317 u 6.5e-17 v 4.6e-17 w 5.3e-17 p 4.6e-17 s 1.4e-16 sr 4.4e-16 dw 2.1e-14 dq 4.7e-16 orth 4.0e-16
    gateway16 pass 3: w 0.761976 u 7.2e-17 v 4.7e-17 w 5.4e-17 p 5.6e-17 s 4.3e-17 sr 2.9e-16 dw 3.3e-14 dq 1.5e-15 orth 3.7e-16

Latitude bands (hrow, gslot, dhalo) are covered by test_two_bands, through the in-process
subdomain harness of tests/test_gpu_dist.py.
"""
import numpy as np
import pytest

import gs_dyn_ref as R

pytestmark = pytest.mark.gpu

BASE = {"Preconditioner": 2, "TS sweeps": 3}


@pytest.fixture(scope="module")
def Ocean():
    from iemic.ocean import Ocean
    return Ocean


def device(Ocean, orc, name, mixing, **params):
    """the case's Ocean with the preconditioner built at the oracle's state"""
    c, L0, o, x, ov, ref, ij, pin, rhs = R.problem(orc, name, mixing)
    oc = Ocean(c, landm=L0, solver_params={**BASE, **params})
    oc.setState(x)
    oc.computeJacobian()
    oc.buildPreconditioner(force=True)
    return oc


fmt = R.fmt


@pytest.mark.parametrize("ts_mg", [0, None], ids=["sweeps", "multigrid"])
@pytest.mark.parametrize("mixing", [0, 1])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_single_pass(oracle_lib, Ocean, name, mixing, ts_mg):
    """one pass with the Schur solve; the two T/S settings write the output by different paths
    (prec_gs.hip ApplyPlan::zaos)"""
    c, L0, o, x, ov, ref, ij, pin, rhs = R.problem(oracle_lib, name, mixing)
    params = {"Dyn iterations": 1}
    if ts_mg is not None:
        params["TS multigrid cycles"] = ts_mg
    oc = device(Ocean, oracle_lib, name, mixing, **params)
    M, exc = ref.M(True, pin, ij), ref.excepted_rows(True, pin, ij)
    worst = {}
    for label, r in rhs:
        z = oc.applyPrecon(r)
        assert np.all(np.isfinite(z)), label
        assert np.array_equal(z[ref.known].view(np.int64), r[ref.known].view(np.int64)), label
        assert ref.pin_violation(z, True, pin, ij) == 0.0, label
        rr, ra = ref.rr_of(r)
        e = ref.row_backward_error(M, ref.dmask(z), rr, exc, ra)
        worst = R.merge(worst, e, R.kinds_of(label))
        assert e["live"] > 0 and np.any(ref.dmask(z)), f"{label} reaches no judged row"
        R.check(e, name, mixing, R.kinds_of(label), label)
    print(f"device {name} mixing={mixing} ts_mg={ts_mg}: {fmt(worst)} | twin {fmt(R.TWIN[(name, mixing)])}")


@pytest.mark.parametrize("schur_passes", [0, 1, 2])
@pytest.mark.parametrize("name", ["natl8", "gateway16", "global4"])
def test_recurrence(oracle_lib, Ocean, name, schur_passes):
    """M_k (z_{k+1} - z_k) = w (rr_D - A_DD z_k) off the excepted rows of pass k, z_k the output
    with "Dyn iterations" k and the default damping; 0: every pass solves the Schur system, 1: the
    first only, 2 (the default): the first and the last, whose fourth pass follows from three
    passes of rule 1.  Every row kind within its own bound of the single pass: a step is one pass
    on the right-hand side d, itself a dense vector"""
    mixing = 1
    c, L0, o, x, ov, ref, ij, pin, rhs = R.problem(oracle_lib, name, mixing)
    r = rhs[0][1]
    rr, ra = ref.rr_of(r)

    def z_of(sp_k, k):
        oc = device(Ocean, oracle_lib, name, mixing, **{"Dyn iterations": k, "Schur passes": sp_k})
        assert oc.solver_params["Schur passes"] == sp_k and oc.solver_params["Dyn iterations"] == k
        return oc.solver_params["Dyn damping"], ref.dmask(oc.applyPrecon(r))

    if schur_passes == 2:
        assert Ocean(c, landm=L0).solver_params["Schur passes"] == 2      # the default
        steps = [((1, 3), (2, 4), True)]
    else:
        steps = [((schur_passes, k), (schur_passes, k + 1), schur_passes == 0) for k in (1, 2, 3)]
    z = {}
    for prev, nxt, schur in steps:
        for key in (prev, nxt):
            if key not in z:
                w, z[key] = z_of(*key)
        assert schur == R.schur_rule(nxt[0], nxt[1] - 1, nxt[1])
        e = ref.recurrence_error(ref.M(schur, pin, ij), z[prev], z[nxt], w, rr, ra,
                                 ref.excepted_rows(schur, pin, ij))
        print(f"device recurrence {name} schur_passes={nxt[0]} pass {nxt[1]}: {fmt(e)}")
        assert np.all(np.isfinite(z[nxt]))
        R.check(e, name, mixing, R.KINDS, (prev, nxt))
        assert ref.pin_violation(z[nxt] - z[prev], schur, pin, ij) == 0.0


class Replay:
    """the pass in numpy on the reference's matrices: a sparse LU of M on the active rows (not
    singular: the excepted rows of M are the unit rows p_top = 0, so their right-hand side is 0)"""

    def __init__(self, ref, M, exc):
        import scipy.sparse.linalg as spla
        self.ref, self.exc = ref, exc
        self.act = np.nonzero(ref.active)[0]
        self.lu = spla.splu(M[self.act][:, self.act].tocsc())

    def solve(self, b):
        b = np.asarray(b, dtype=np.float64).copy()
        b[self.exc] = 0.0
        out = np.zeros(self.ref.N)
        out[self.act] = self.lu.solve(b[self.act])
        return out

    def w_of(self, z, rr):
        """(zc, w) of the minimal-residual step from the iterate z: zc the pass on the defect d,
        q = A_DD zc, w = <d,q> / <q,q>"""
        d = np.asarray(self.ref.defect(z, rr), dtype=np.float64)
        zc = self.solve(d)
        q = self.ref.A_DD @ zc
        return zc, float((d @ q) / (q @ q))

    def iterates(self, rr, passes):
        z = self.solve(rr)
        out = [z.copy()]
        for _ in range(1, passes):
            zc, w = self.w_of(z, rr)
            z = z + w * zc
            out.append(z.copy())
        return out


def twin_mr_iterates(P1, ref, r, rr, passes):
    """the minimal-residual recurrence with the CPU twin's single pass P1 (the twin has no such
    variant): a right-hand side that is d on the active dynamics rows and 0 elsewhere makes the
    twin's rr equal to d.  Its iterates, judged against the replay's LU like the device's, are the
    baseline of dw: two independent implementations of the pass."""
    z = ref.dmask(P1.apply(r))
    out = [z.copy()]
    for _ in range(1, passes):
        d = np.asarray(ref.defect(z, rr), dtype=np.float64)
        zc = ref.dmask(P1.apply(d))
        q = ref.A_DD @ zc
        z = z + (d @ q) / (q @ q) * zc
        out.append(z.copy())
    return out


def mr_figures(ref, rep, M, exc, zk, zk1, rr, ra):
    """of a minimal-residual step zk -> zk1, with D = zk1 - zk and d = rr_D - A_DD zk:
    w     the step fitted by least squares to M D = w d on the rows that are not excepted;
    e     the recurrence's backward error per row kind with that w;
    dw    |w - w'| / |w|, w' = <d,q>/<q,q> with q = A_DD zc and zc the replay's own pass on d: the
          quotient k_mr_dots forms, from a correction the device did not compute;
    dq    |w - <d,q>/<q,q>| / |w| with q = A_DD D / w, the issue's form.  The fitted w cancels in
          it: it equals |<d - A_DD D, A_DD D>| / <A_DD D, A_DD D>, so it restates orth in another
          scaling and is no second confirmation;
    orth  |<d - A_DD D, A_DD D>| / (|d| |A_DD D|).
    The sums run over the active U/V/W/P rows: k_mr_dots sums the four U/V/W/P planes over the
    owned cells (Lay own0, nloc), and both of its operands are 0 on the identity rows."""
    d = ref.defect(zk, rr)
    D = (zk1.astype(R.LD) - zk.astype(R.LD)).astype(np.float64)
    ok = ref.active.copy()
    ok[exc] = False
    MD = R._mv(M, D)
    w = float(np.sum(MD[ok] * d[ok]) / np.sum(d[ok] * d[ok]))
    e = ref.recurrence_error(M, zk, zk1, w, rr, ra, exc)
    AD = R._mv(ref.A_DD, D)
    q = AD / R.LD(w)
    dq = abs(w - float(np.sum(d * q) / np.sum(q * q))) / abs(w)
    nrm = lambda v: np.sqrt(np.sum(v * v))
    orth = float(abs(np.sum((d - AD) * AD)) / (nrm(d) * nrm(AD)))
    dw = abs(w - rep.w_of(zk, rr)[1]) / abs(w)
    return w, e, dict(dw=dw, dq=dq, orth=orth)


@pytest.mark.parametrize("name", ["natl8", "gateway16"])
def test_minimal_residual(oracle_lib, Ocean, name):
    """"Dyn minimal residual" with 2 and 3 passes (every pass solves the Schur system): each step
    is a pass on the defect scaled by one number (every row kind within its bound), that number is
    the quotient of k_mr_dots, and the new defect is orthogonal to the change.  The bounds of dq and
    orth are 100 x the same figures of a numpy replay of the recurrence, that of dw 100 x the figure
    of the recurrence run with the twin's pass (twin_mr_iterates, the larger of its two steps),
    each at most 1e-8."""
    mixing = 1
    c, L0, o, x, ov, ref, ij, pin, rhs = R.problem(oracle_lib, name, mixing)
    r = rhs[0][1]
    rr, ra = ref.rr_of(r)
    M, exc = ref.M(True, pin, ij), ref.excepted_rows(True, pin, ij)
    rep = Replay(ref, M, exc)
    zr = rep.iterates(rr, 3)
    zt = twin_mr_iterates(oracle_lib.BlockGS(o, ov, 3, dyn_iters=1), ref, r, rr, 3)
    z = [ref.dmask(device(Ocean, oracle_lib, name, mixing,
                          **{"Dyn iterations": k, "Dyn minimal residual": True}).applyPrecon(r))
         for k in (1, 2, 3)]
    # dw's baseline is the larger of the twin's two steps: the figure is a difference of two
    # quotients that agree to 12 digits, and on the twin itself it moves between consecutive steps
    # (natl8: 4.8e-15 at pass 2, 8.1e-13 at pass 3; gateway16: 3.2e-14, 3.2e-13), so one step's
    # sample is not the reference's error
    dw0 = max(mr_figures(ref, rep, M, exc, zt[k - 1], zt[k], rr, ra)[2]["dw"] for k in (1, 2))
    for k in (1, 2):
        w0, e0, f0 = mr_figures(ref, rep, M, exc, zr[k - 1], zr[k], rr, ra)
        f0["dw"] = dw0
        w, e, f = mr_figures(ref, rep, M, exc, z[k - 1], z[k], rr, ra)
        show = lambda g: " ".join(f"{t} {v:.1e}" for t, v in g.items())
        print(f"device minimal residual {name} pass {k + 1}: w {w:.6f} {fmt(e)} {show(f)}"
              f" | replay w {w0:.6f} {fmt(e0)} {show(f0)}")
        assert w > 0.0
        R.check(e, name, mixing, R.KINDS, k)
        for t in f:
            assert f[t] <= min(1e-8, 100.0 * f0[t]), (t, f[t], f0[t])


def band_apply(Ocean, orc, name, mixing, nranks, rs, **params):
    """(damping, [z of applyPrecon(r) for r in rs]) on nranks latitude bands in one process, every
    z gathered from the owners of its rows"""
    from test_gpu_dist import _run_bands, owned_rows
    c, L0, o, x, ov, ref, ij, pin, rhs = R.problem(orc, name, mixing)

    def fn(rk, group):
        oc = Ocean(c, landm=L0, local_group=group, rank=rk, nranks=nranks, npx=1,
                   solver_params={**BASE, **params})
        oc.setState(x)
        oc.computeJacobian()
        oc.buildPreconditioner(force=True)
        z = [oc.applyPrecon(r).copy() for r in rs]
        lay, damping = oc.layout(), oc.solver_params["Dyn damping"]
        oc.close()
        return dict(lay=lay, z=z, w=damping)

    zs = [np.full(c.nrows, np.nan) for _ in rs]
    for q in _run_bands(nranks, fn):
        rows = np.array(owned_rows(c, q["lay"]))
        for z, zq in zip(zs, q["z"]):
            z[rows] = zq[rows]
    return q["w"], zs


@pytest.mark.parametrize("name", ["natl8", "global4"])
def test_two_bands(oracle_lib, Ocean, name):
    """two latitude bands in one process (the paths that compute the halo rows locally: hrow,
    gslot, and dhalo in the later passes): the single pass over the dense, single-row-type and
    impulse right-hand sides, and the default's fourth pass (a Schur pass, the first and the last
    solving) from three passes of which the first only solves"""
    mixing = 1
    c, L0, o, x, ov, ref, ij, pin, rhs = R.problem(oracle_lib, name, mixing)
    M, exc = ref.M(True, pin, ij), ref.excepted_rows(True, pin, ij)
    worst = {}
    _, zs = band_apply(Ocean, oracle_lib, name, mixing, 2, [r for _, r in rhs], **{"Dyn iterations": 1})
    for (label, r), z in zip(rhs, zs):
        assert np.all(np.isfinite(z)), label
        assert np.array_equal(z[ref.known].view(np.int64), r[ref.known].view(np.int64)), label
        assert ref.pin_violation(z, True, pin, ij) == 0.0, label
        rr, ra = ref.rr_of(r)
        e = ref.row_backward_error(M, ref.dmask(z), rr, exc, ra)
        worst = R.merge(worst, e, R.kinds_of(label))
        R.check(e, name, mixing, R.kinds_of(label), label)
    print(f"device two bands {name}: {fmt(worst)}")
    r = rhs[0][1]
    rr, ra = ref.rr_of(r)
    _, (z3,) = band_apply(Ocean, oracle_lib, name, mixing, 2, [r], **{"Dyn iterations": 3, "Schur passes": 1})
    w, (z4,) = band_apply(Ocean, oracle_lib, name, mixing, 2, [r])
    e = ref.recurrence_error(M, ref.dmask(z3), ref.dmask(z4), w, rr, ra, exc)
    print(f"device two bands {name} default pass 4: {fmt(e)}")
    assert np.all(np.isfinite(z4))
    R.check(e, name, mixing, R.KINDS, "pass 4")
