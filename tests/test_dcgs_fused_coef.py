"""The DCGS2 update pass with its coefficients formed in its own prologue (krylov.hip
k_dcgs_update<true>, the solve's launch) against the chain it replaces, k_dcgs_coef followed by
the update from the coefficient array (k_dcgs_update<false>), through iemic_test_dcgs_update.

Every workgroup of the fused launch runs the 256-thread reduction and the expressions of
k_dcgs_coef on the same summed dot rows, so everything must be bitwise equal: the new basis
vector u, the next candidate w, the planar copy rrP of w, beta and h_jj in rows 2 nv + 3 and
2 nv + 4 of hb, and the 2 nv + 5 rows stored into the host's pinned slot.

nv: 1, 3, 4, 5 around the update's unroll of 4, 90 the benchmark's cycle length, and 0, which
the solve does launch: the first step of every cycle (jj = 0 < m) updates against an empty basis
(u is only scaled by 1/beta, w loses gamma u).
N: 2 (one lane of one workgroup), 510 and 6*64*7 = 2688 on each side of one workgroup's 512
elements; 510 and 2688 are whole numbers of 6-row cells (as compressed rows come) and carry
rrP.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import golden_landm
from iemic import _lib
from iemic import config as cf

pytestmark = pytest.mark.gpu

NVS = (0, 1, 3, 4, 5, 90)
NS = (2, 510, 6 * 64 * 7)
EPS = 2.0 ** -52
_PD, _PI = C.POINTER(C.c_double), C.POINTER(C.c_int)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def hook():
    from iemic.ocean import Ocean
    oc = Ocean(cf.preset("test6x6x4", mixing=0), landm=golden_landm("test6x6x4"))
    f = _lib.lib().iemic_test_dcgs_update
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, _PD, _PD, _PD, _PD, _PD, _PI, C.c_int64, _PD]

    def run(fused, d):
        nv, N, ldq = d["nv"], d["N"], d["ldq"]
        hb, u, w = d["hb"].copy(), d["u"].copy(), d["w"].copy()
        hrows = np.full(2 * nv + 5, np.nan)
        act, ps = d["act"], d["ps"]
        rrP = None if act is None else np.full(6 * ps, np.nan)
        Q = d["Q"].reshape(-1)
        p = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(_PD)  # noqa: E731
        rc = f(oc._h, int(fused), nv, N, ldq, p(Q), p(hb), p(u), p(w), p(hrows),
               None if act is None else act.ctypes.data_as(_PI), ps, p(rrP))
        assert rc == 0, _lib.lib().iemic_last_error()
        return dict(hb=hb, u=u, w=w, hrows=hrows, rrP=rrP)

    yield run
    oc.close()


def data(nv, N, breakdown=False):
    """seeded Q, u, w and dot rows hb with u.u = |a|^2 + 0.7 (breakdown: half of |a|^2, so
    u.u - |a|^2 < 0); rows 2 nv + 3, 2 nv + 4 start as NaN"""
    rng = np.random.default_rng(1000 * nv + N + (7 if breakdown else 0))
    ldq = N + 4
    Q = np.full((max(nv, 1), ldq), np.nan)[:nv]
    Q[:, :N] = rng.uniform(-1.0, 1.0, (nv, N))
    u, w = rng.uniform(-1.0, 1.0, N), rng.uniform(-1.0, 1.0, N)
    a, b = rng.uniform(-0.1, 0.1, nv), rng.uniform(-0.1, 0.1, nv)
    hb = np.full(2 * nv + 5, np.nan)
    hb[0:2 * nv:2], hb[1:2 * nv:2] = a, b
    hb[2 * nv] = 0.5 * float(a @ a) if breakdown else float(a @ a) + 0.7
    hb[2 * nv + 1], hb[2 * nv + 2] = rng.uniform(-1.0, 1.0), rng.uniform(0.5, 1.5)
    act, ps = None, 0
    if N % 6 == 0:
        ps = N // 6 + 52
        act = np.sort(rng.choice(ps, N // 6, replace=False)).astype(np.int32)
    return dict(nv=nv, N=N, ldq=ldq, Q=np.ascontiguousarray(Q), u=u, w=w, hb=hb, act=act, ps=ps, a=a)


def compare(d, old, new):
    nv = d["nv"]
    names = ["u", "w", "hrows"] + (["rrP"] if d["act"] is not None else [])
    nd = {k: int(np.count_nonzero(bits(old[k]) != bits(new[k]))) for k in names}
    nd["hb"] = int(np.count_nonzero(bits(old["hb"]) != bits(new["hb"])))
    print(f"nv={nv} N={d['N']}: differing entries {nd}; beta={new['hb'][2 * nv + 3]!r} h_jj={new['hb'][2 * nv + 4]!r}")
    assert all(v == 0 for v in nd.values()), nd
    # the pinned slot holds the dot rows as they came and beta, h_jj as hb got them
    assert np.array_equal(bits(new["hrows"][:2 * nv + 3]), bits(d["hb"][:2 * nv + 3]))
    assert np.array_equal(bits(new["hrows"][2 * nv + 3:]), bits(new["hb"][2 * nv + 3:]))
    assert np.array_equal(bits(new["hb"][:2 * nv + 3]), bits(d["hb"][:2 * nv + 3]))
    if d["act"] is not None:
        # w's rows 6 a + R in plane R at cell act[a]; the hook's fill (all bits set) elsewhere
        exp = np.full((6, d["ps"]), -1, dtype=np.int64)
        exp[:, d["act"]] = bits(new["w"]).reshape(-1, 6).T
        assert np.array_equal(bits(new["rrP"]), exp.reshape(-1))


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("nv", NVS)
def test_fused_equals_coef_then_update(hook, nv, N):
    d = data(nv, N)
    old, new = hook(0, d), hook(1, d)
    compare(d, old, new)
    # not equal garbage: q = (u - Q a) / beta within the rounding of nv + 2 operations per
    # entry on terms summing to |u| + |a| . |Q| in magnitude, and of beta (its square is 0.7, from
    # u.u + |a|^2 <= 2.5: a relative error below 4 (nv + 2) eps, half of it in the root)
    a = d["a"].astype(np.longdouble)
    Qn = d["Q"][:, :N].astype(np.longdouble)
    beta = np.sqrt(np.longdouble(d["hb"][2 * nv]) - a @ a)
    ref = (d["u"].astype(np.longdouble) - a @ Qn) / beta
    mag = (np.abs(d["u"]) + np.abs(d["a"]) @ np.abs(d["Q"][:, :N])) / float(beta)
    bound = (nv + 2) * EPS * mag + (2 * (nv + 2) + 2) * EPS * np.abs(ref).astype(np.float64)
    err = np.abs((new["u"].astype(np.longdouble) - ref).astype(np.float64))
    print(f"nv={nv} N={N}: max error of q over its bound {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound)
    assert abs(new["hb"][2 * nv + 3] - float(beta)) <= (2 * (nv + 2) + 2) * EPS * float(beta)


def test_breakdown(hook):
    """u.u - |a|^2 < 0: beta = h_jj = 0 and zero scales on both paths, so u and w come out 0"""
    d = data(3, 510, breakdown=True)
    old, new = hook(0, d), hook(1, d)
    compare(d, old, new)
    assert new["hb"][2 * 3 + 3] == 0.0 and new["hb"][2 * 3 + 4] == 0.0
    assert not np.any(new["u"]) and not np.any(new["w"])
