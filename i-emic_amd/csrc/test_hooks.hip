/*
 * test_hooks.hip -- the dense solvers of the preconditioner, the coupled model's block
 * Gauss-Seidel preconditioner and the DCGS2 update pass driven on their own, and the T/S
 * multigrid's plan and levels read back, the active set read back and the compressed SpMV and
 * the dynamics defect driven on their own (test_hooks.h).
 * No kernels here: every hook stages host data, calls the production entry points of
 * the cyclic reduction (schur_cr.h: cr_plan.hip, cr_factor.hip, schur_cr.hip, cr_inv.hip) /
 * band_lu.hip / coupled.hip / krylov.hip / spmv.hip on the context's stream and copies back.
 */
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "coupled_internal.h"
#include "krylov_internal.h"
#include "vec_kernels.h"
#include "test_hooks.h"

using namespace iemic;

namespace {

/* LDS of one workgroup on gfx950 */
constexpr size_t LDS_MAX = 160 * 1024;

int bad(const char* what)
{
    set_error(std::string("test hook: ") + what);
    return IEMIC_EINVAL;
}

void cr_plan(const SchurCR& cr, int* plan)
{
    std::fill(plan, plan + IEMIC_TEST_PLAN_LEN, 0);
    plan[0] = cr.nlev;
    plan[1] = cr.lt;
    plan[2] = cr.tM;
    plan[3] = cr.ncomp;
    plan[4] = (int)cr.down.size();
    int k = 5;
    for (const auto* v : {&cr.down, &cr.up})
        for (const CrStep& st : *v) {
            if (k + 4 > IEMIC_TEST_PLAN_LEN) return;
            plan[k++] = st.rc;
            plan[k++] = st.nwg;
            plan[k++] = st.cls.ncls;
            plan[k++] = st.nl;
        }
}

int cr_load_blocks(iemic_ctx* c, SchurCR& cr, const double* D, const double* L, const double* R)
{
    const size_t nb = (size_t)cr.n * cr.m * cr.m;
    int rc;
    if ((rc = h2d(c, cr.dlr.p, D, sizeof(double) * nb))) return rc;
    if ((rc = h2d(c, cr.dlr.p + nb, L, sizeof(double) * nb))) return rc;
    return h2d(c, cr.dlr.p + 2 * nb, R, sizeof(double) * nb);
}

/* one solve; x (and xT) are filled with NaN bit patterns first, so an entry the solve does
 * not write cannot pass for a value left by the solve before */
int cr_solve_one(iemic_ctx* c, const SchurCR& cr, DevBuf<double>& bd, DevBuf<double>& xd, DevBuf<double>& xtd,
                 const double* b, double* x, double* xT)
{
    const size_t nm = (size_t)cr.n * cr.m;
    int rc;
    if ((rc = h2d(c, bd.p, b, sizeof(double) * nm))) return rc;
    HIP_OK(hipMemsetAsync(xd.p, 0xff, sizeof(double) * nm, c->stream));
    if (xT) HIP_OK(hipMemsetAsync(xtd.p, 0xff, sizeof(double) * nm, c->stream));
    if ((rc = cr_solve(c, cr, bd.p, xd.p, c->stream, xT ? xtd.p : nullptr))) return rc;
    if ((rc = d2h(c, x, xd.p, sizeof(double) * nm))) return rc;
    if (xT && (rc = d2h(c, xT, xtd.p, sizeof(double) * nm))) return rc;
    return 0;
}

}  // namespace

extern "C" int iemic_test_cr_solve(iemic_ctx* c, int n, int m, int periodic, int tail_max, const double* D,
                                   const double* L, const double* R, const double* S9, const int* col_of_ij,
                                   int nsolve, const double* b, double* x, double* xT, int* info, int* plan)
{
    if (!c || !info || !plan) return bad("null argument");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    if (n < 1 || m < 1 || nsolve < 0 || (int64_t)n * m > (1 << 24)) return bad("cyclic reduction shape out of range");
    if (D ? (!L || !R) : (!S9 || !col_of_ij)) return bad("neither blocks nor 9-point rows");
    if (nsolve && (!b || !x)) return bad("null right-hand side or solution");
    *info = 0;
    int rc;
    SchurCR cr;
    if ((rc = cr_init(c, cr, n, m, periodic ? 1 : 0, tail_max))) return rc;
    cr_plan(cr, plan);
    const size_t nm = (size_t)n * m;
    if (D) {
        if ((rc = cr_load_blocks(c, cr, D, L, R))) return rc;
        if ((rc = cr_factor_blocks(c, cr))) return rc;
    } else {
        DevBuf<double> s9;
        DevBuf<int> col;
        if (s9.alloc(nm * 9) || col.alloc(nm)) return IEMIC_ENOMEM;
        if ((rc = h2d(c, s9.p, S9, sizeof(double) * nm * 9))) return rc;
        if ((rc = h2d(c, col.p, col_of_ij, sizeof(int) * nm))) return rc;
        if ((rc = cr_factor(c, cr, s9.p, col.p))) return rc;
        DEV_SYNC(c);
    }
    if ((rc = d2h(c, info, cr.info.p, sizeof(int)))) return rc;
    if ((rc = cr_check(c, cr))) return rc;
    DevBuf<double> bd, xd, xtd;
    if (bd.alloc(nm) || xd.alloc(nm) || (xT && xtd.alloc(nm))) return IEMIC_ENOMEM;
    for (int k = 0; k < nsolve; k++)
        if ((rc = cr_solve_one(c, cr, bd, xd, xtd, b + k * nm, x + k * nm, xT ? xT + k * nm : nullptr))) return rc;
    return 0;
}

extern "C" int iemic_test_cr_refactor(iemic_ctx* c, int n, int m, int periodic, int tail_max, const double* D1,
                                      const double* L1, const double* R1, const double* D2, const double* L2,
                                      const double* R2, const double* b, double* x)
{
    if (!c || !D1 || !L1 || !R1 || !D2 || !L2 || !R2 || !b || !x) return bad("null argument");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    if (n < 1 || m < 1 || (int64_t)n * m > (1 << 24)) return bad("cyclic reduction shape out of range");
    int rc;
    SchurCR cr;
    if ((rc = cr_init(c, cr, n, m, periodic ? 1 : 0, tail_max))) return rc;
    const size_t nm = (size_t)n * m;
    DevBuf<double> bd, xd, xtd;
    if (bd.alloc(nm) || xd.alloc(nm)) return IEMIC_ENOMEM;
    for (int pass = 0; pass < 2; pass++) {
        if ((rc = cr_load_blocks(c, cr, pass ? D2 : D1, pass ? L2 : L1, pass ? R2 : R1))) return rc;
        if ((rc = cr_factor_blocks(c, cr))) return rc;
        if ((rc = cr_check(c, cr))) return rc;
        if ((rc = cr_solve_one(c, cr, bd, xd, xtd, b, x, nullptr))) return rc;
    }
    return 0;
}

extern "C" int iemic_test_cr_inverse(iemic_ctx* c, int m, int count, int s0, int sstep, int nsrc, const double* A,
                                     double* X, int* info)
{
    if (!c || !A || !X || !info) return bad("null argument");
    if (m < 1 || count < 1 || nsrc < 1 || s0 < 0 || sstep < 1 || (int64_t)s0 + (int64_t)(count - 1) * sstep >= nsrc ||
        count > 4096 || nsrc > 65536)
        return bad("Gauss-Jordan batch out of range");
    if (m > CR_BLOCK_MAX) {                           /* before any allocation: cr_inverse's own refusal */
        return cr_inverse(c->stream, m, count, nullptr, s0, sstep, nullptr, nullptr);
    }
    const size_t mm = (size_t)m * m;
    DevBuf<double> ad, xd;
    DevBuf<int> id;
    if (ad.alloc(nsrc * mm) || xd.alloc(count * mm) || id.alloc(1)) return IEMIC_ENOMEM;
    int rc;
    if ((rc = h2d(c, ad.p, A, sizeof(double) * nsrc * mm))) return rc;
    HIP_OK(hipMemsetAsync(xd.p, 0xff, sizeof(double) * count * mm, c->stream));
    HIP_OK(hipMemsetAsync(id.p, 0, sizeof(int), c->stream));
    if ((rc = cr_inverse(c->stream, m, count, ad.p, s0, sstep, xd.p, id.p))) return rc;
    if ((rc = d2h(c, X, xd.p, sizeof(double) * count * mm))) return rc;
    return d2h(c, info, id.p, sizeof(int));
}

extern "C" int iemic_test_band_inverse(iemic_ctx* c, int N, int bl, int bu, double* ab, int* piv, double* X,
                                       int* info, int* stage_o)
{
    if (!c || !ab || !piv || !X || !info || !stage_o) return bad("null argument");
    if (N < 1 || bl < 0 || bu < 0 || N > 4096 || bl > 4096 || bu > 4096) return bad("band shape out of range");
    /* the two LDS sizes as band_lu_inverse computes them */
    const int NBP = BAND_NBP;
    const size_t lb = sizeof(double) * ((size_t)(NBP + bl) * (NBP + 1) + (size_t)2 * NBP * (bl + bu));
    const int so = lb <= 150 * 1024 ? 1 : 0;
    const size_t lbu = so ? lb : lb - sizeof(double) * (size_t)NBP * (bl + bu);
    const int ring = std::max(bl + NBP + 1, bl + bu + 1);
    const size_t li = (size_t)(ring + 2 * NBP) * 16 * sizeof(double);
    *stage_o = so;
    if (lbu > LDS_MAX || li > LDS_MAX) return bad("band too wide for the LDS of the band kernels");
    const int W = 2 * bl + bu + 1;
    const size_t npan = (size_t)(N + NBP - 1) / NBP;
    DevBuf<double> abd, xd, lpan;
    DevBuf<int> pd, id, cd;
    if (abd.alloc((size_t)N * W) || xd.alloc((size_t)N * N) || lpan.alloc(npan * (NBP + bl) * NBP) || pd.alloc(N) ||
        id.alloc(1) || cd.alloc(N))
        return IEMIC_ENOMEM;
    std::vector<int> cols(N);
    for (int q = 0; q < N; q++) cols[q] = q;
    int rc;
    if ((rc = h2d(c, cd.p, cols.data(), sizeof(int) * N))) return rc;
    if ((rc = h2d(c, abd.p, ab, sizeof(double) * N * W))) return rc;
    if ((rc = h2d(c, xd.p, X, sizeof(double) * N * N))) return rc;      /* the caller's prefill */
    HIP_OK(hipMemsetAsync(pd.p, 0xff, sizeof(int) * N, c->stream));
    if ((rc = band_lu_inverse(c, abd.p, N, bl, bu, pd.p, id.p, lpan.p, cd.p, xd.p, info))) return rc;
    if ((rc = d2h(c, ab, abd.p, sizeof(double) * N * W))) return rc;
    if ((rc = d2h(c, piv, pd.p, sizeof(int) * N))) return rc;
    return d2h(c, X, xd.p, sizeof(double) * N * N);
}

extern "C" int iemic_test_dcgs_update(iemic_ctx* c, int fused, int nv, int64_t N, int64_t ldq, const double* Q,
                                      double* hb, double* u, double* w, double* hrows, const int* act, int64_t ps,
                                      double* rrP)
{
    if (!c || !hb || !u || !w || !hrows || (nv > 0 && !Q)) return bad("null argument");
    if (nv < 0 || nv > MAX_KRYLOV || N < 2 || (N & 1) || N > (1 << 24) || ldq < N || (ldq & 1)) return bad("DCGS2 shape out of range");
    if (act && (!rrP || N % NUN || ps < N / NUN || ps > (1 << 24))) return bad("planar right-hand side out of range");
    const int nr = 2 * nv + 5;
    const int64_t ncell = N / NUN;
    if (act)
        for (int64_t a = 0; a < ncell; a++)
            if (act[a] < 0 || act[a] >= ps) return bad("active cell outside the planes");
    DevBuf<double> qd, hd, cd, ud, wd, rd;
    DevBuf<int> ad;
    if ((nv && qd.alloc((size_t)nv * ldq)) || hd.alloc(nr) || cd.alloc(RED_ROWS) || ud.alloc(N) || wd.alloc(N) ||
        (act && (ad.alloc(ncell) || rd.alloc((size_t)NUN * ps))))
        return IEMIC_ENOMEM;
    int rc;
    if (nv && (rc = h2d(c, qd.p, Q, sizeof(double) * nv * ldq))) return rc;
    if ((rc = h2d(c, hd.p, hb, sizeof(double) * nr))) return rc;
    if ((rc = h2d(c, ud.p, u, sizeof(double) * N))) return rc;
    if ((rc = h2d(c, wd.p, w, sizeof(double) * N))) return rc;
    HIP_OK(hipMemsetAsync(cd.p, 0xff, sizeof(double) * RED_ROWS, c->stream));
    if (act) {
        if ((rc = h2d(c, ad.p, act, sizeof(int) * ncell))) return rc;
        HIP_OK(hipMemsetAsync(rd.p, 0xff, sizeof(double) * NUN * ps, c->stream));
    }
    /* the solve's pinned slot 0: the rows arrive there by the kernels' own stores */
    std::memset(c->h_red, 0xff, sizeof(double) * nr);
    if ((rc = dcgs_update(c, fused != 0, qd.p, ldq, nv, hd.p, cd.p, c->h_red, ud.p, wd.p, N, act ? ad.p : nullptr, 0,
                          ps, act ? rd.p : nullptr)))
        return rc;
    if ((rc = d2h(c, hb, hd.p, sizeof(double) * nr))) return rc;
    if ((rc = d2h(c, u, ud.p, sizeof(double) * N))) return rc;
    if ((rc = d2h(c, w, wd.p, sizeof(double) * N))) return rc;
    if (act && (rc = d2h(c, rrP, rd.p, sizeof(double) * NUN * ps))) return rc;
    std::memcpy(hrows, c->h_red, sizeof(double) * nr);
    return 0;
}

extern "C" int iemic_test_coupled_prec(iemic_coupled* cm, const double* r_host, double* z_host, int use_prec)
{
    if (!cm || !r_host || !z_host) return bad("null argument");
    iemic_ctx* oc = cm->oc;
    iemic_atmos* a = cm->at;
    if (hipSetDevice(oc->device) != hipSuccess) return IEMIC_EDEVICE;
    if (!oc->jac_valid || !a->jac_valid) {
        set_error("test hook: no Jacobian assembled");
        return IEMIC_ESTATE;
    }
    StreamGuard guard{oc};
    int rc;
    if (use_prec) {
        if (!oc->gs.ready && (rc = prec_compute(oc, nullptr))) return rc;
        if (!a->prec_valid && (rc = atm_prec_compute(a))) return rc;
    }
    const int64_t NC = cm->NC;
    std::vector<double> packed;
    pack_host(cm, r_host, packed);
    DevBuf<double> dr, dz;
    if (dr.alloc(NC) || dz.alloc(NC)) return IEMIC_ENOMEM;
    if ((rc = h2d(oc, dr.p, packed.data(), sizeof(double) * NC))) return rc;
    HIP_OK(hipMemsetAsync(dz.p, 0xff, sizeof(double) * NC, oc->stream));
    if ((rc = cpl_prec(cm, dr.p, dz.p, use_prec))) return rc;
    if ((rc = d2h(oc, packed.data(), dz.p, sizeof(double) * NC))) return rc;
    unpack_host(cm, packed, z_host);
    return 0;
}

extern "C" int iemic_test_ts_mg_plan(iemic_ctx* c, int* plan)
{
    if (!c || !plan) return bad("null argument");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    if (!c->gs.ready || c->gs.ts_mg <= 0) return bad("no T/S multigrid set up");
    std::fill(plan, plan + IEMIC_TEST_PLAN_LEN, 0);
    TsMgProbe p;
    int rc;
    if ((rc = ts_mg_probe(c, 0, &p))) return bad("no T/S multigrid levels");
    plan[0] = p.nlev;
    plan[1] = p.lanes;
    plan[2] = p.sweeps;
    plan[3] = p.hr;
    plan[4] = p.ckind;
    for (int q = 0; q < p.nlev && 10 + 5 * q <= IEMIC_TEST_PLAN_LEN; q++) {
        TsMgProbe l;
        if ((rc = ts_mg_probe(c, q, &l))) return rc;
        int* e = plan + 5 + 5 * q;
        e[0] = l.n;
        e[1] = l.m;
        e[2] = l.par;
        e[3] = l.colours;
        e[4] = l.fused;
    }
    return 0;
}

extern "C" int iemic_test_ts_mg_level(iemic_ctx* c, int q, double* off, double* diag, double* b, double* z,
                                      double* cinv)
{
    if (!c || !off || !diag || !b || !z) return bad("null argument");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    if (!c->gs.ready || c->gs.ts_mg <= 0) return bad("no T/S multigrid set up");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    TsMgProbe p;
    if (ts_mg_probe(c, q, &p)) return bad("no such T/S multigrid level");
    if (p.halo) return bad("the level's layout has a halo");
    if (p.cinv && !cinv) return bad("null argument");
    const size_t ncl = (size_t)p.n * p.m * c->l;
    int rc;
    if ((rc = d2h(c, off, p.off, sizeof(double) * 16 * ncl))) return rc;
    if ((rc = d2h(c, diag, p.diag, sizeof(double) * 4 * ncl))) return rc;
    if ((rc = d2h(c, b, p.b, sizeof(double) * 2 * ncl))) return rc;
    if ((rc = d2h(c, z, p.z, sizeof(double) * 2 * ncl))) return rc;
    if (p.cinv && (rc = d2h(c, cinv, p.cinv, sizeof(double) * 4 * ncl * ncl))) return rc;
    return 0;
}

extern "C" int iemic_test_ts_mg_nofuse(iemic_ctx* c, int on)
{
    if (!c) return bad("null argument");
    c->gs.mg.nofuse = on != 0;
    return 0;
}

extern "C" int iemic_test_ts_mg_nopack(iemic_ctx* c, int on)
{
    if (!c) return bad("null argument");
    c->gs.mg.nopack = on != 0;
    return 0;
}

extern "C" int iemic_test_ts_mg_entry(iemic_ctx* c, int64_t NE, const double* rr, const double* zd, double* b,
                                      double* z, int64_t* pack_doubles)
{
    if (!c || !rr || !zd || !b || !z) return bad("null argument");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    if (!c->gs.ready || c->gs.ts_mg <= 0) return bad("no T/S multigrid set up");
    if (NE != c->sub.nerows() || (size_t)NE > c->gs.rrP.n) return bad("vector length");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    StreamGuard guard{c};
    TsMgProbe p;
    if (ts_mg_probe(c, 0, &p)) return bad("no T/S multigrid levels");
    if (p.halo) return bad("the level's layout has a halo");
    DevBuf<double> keep, zdd;
    if (keep.alloc(NE) || zdd.alloc(NE)) return IEMIC_ENOMEM;
    int rc;
    /* the preconditioner's planar right-hand side is put back afterwards */
    HIP_OK(hipMemcpyAsync(keep.p, c->gs.rrP.p, sizeof(double) * NE, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = h2d(c, c->gs.rrP.p, rr, sizeof(double) * NE))) return rc;
    if ((rc = h2d(c, zdd.p, zd, sizeof(double) * NE))) return rc;
    const size_t ncl = (size_t)p.n * p.m * c->l;
    HIP_OK(hipMemsetAsync(const_cast<double*>(p.b), 0xff, sizeof(double) * 2 * ncl, c->stream));
    HIP_OK(hipMemsetAsync(const_cast<double*>(p.z), 0xff, sizeof(double) * 2 * ncl, c->stream));
    if ((rc = ts_mg_entry(c, zdd.p))) return rc;
    HIP_OK(hipGetLastError());
    if ((rc = d2h(c, b, p.b, sizeof(double) * 2 * ncl))) return rc;
    if ((rc = d2h(c, z, p.z, sizeof(double) * 2 * ncl))) return rc;
    HIP_OK(hipMemcpyAsync(c->gs.rrP.p, keep.p, sizeof(double) * NE, hipMemcpyDeviceToDevice, c->stream));
    if (pack_doubles) *pack_doubles = c->gs.mg.epn;
    return dev_wait(c, nullptr, __func__);
}

extern "C" int iemic_test_eig_ritz(iemic_ctx* c, int j, int p, int64_t N, int64_t ldv, const double* V,
                                   const double* Y, double* X)
{
    if (!c || !V || !Y || !X) return bad("null argument");
    if (j < 1 || j > IEMIC_EIGS_MAX_M || p < 1 || p > 16 || N < 1 || N > (1 << 24) || ldv < N)
        return bad("Ritz shape out of range");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    DevBuf<double> vd, xd;
    if (vd.alloc((size_t)j * ldv) || xd.alloc((size_t)p * N)) return IEMIC_ENOMEM;
    int rc;
    if ((rc = h2d(c, vd.p, V, sizeof(double) * j * ldv))) return rc;
    HIP_OK(hipMemsetAsync(xd.p, 0xff, sizeof(double) * p * N, c->stream));
    double* xs[16] = {};
    for (int q = 0; q < p; q++) xs[q] = xd.p + (int64_t)q * N;
    if ((rc = eigs_ritz(c, vd.p, ldv, j, p, Y, xs, N))) return rc;
    return d2h(c, X, xd.p, sizeof(double) * p * N);
}

extern "C" int iemic_test_eig_compress(iemic_ctx* c, int j, int p, int64_t N, int64_t ldv, double* V, const double* Q)
{
    if (!c || !V || !Q) return bad("null argument");
    if (j < 2 || j > IEMIC_EIGS_MAX_M || p < 1 || p > 16 || p >= j || N < 1 || N > (1 << 24) || ldv < N)
        return bad("compression shape out of range");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    DevBuf<double> vd;
    if (vd.alloc((size_t)(j + 1) * ldv)) return IEMIC_ENOMEM;
    int rc;
    if ((rc = h2d(c, vd.p, V, sizeof(double) * (j + 1) * ldv))) return rc;
    if ((rc = eigs_compress(c, vd.p, ldv, j, p, Q, N))) return rc;
    return d2h(c, V, vd.p, sizeof(double) * (j + 1) * ldv);
}

extern "C" int iemic_test_eig_compress_cost(iemic_ctx* c, int j, int p, int nrep, double* ms)
{
    if (!c || !ms) return bad("null argument");
    if (j < 2 || j > IEMIC_EIGS_MAX_M || p < 1 || p > 16 || p >= j || nrep < 1 || nrep > 100)
        return bad("compression shape out of range");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    StreamGuard guard{c};
    const int64_t NE = c->sub.nerows();
    const Owned w = owned(c);
    DevBuf<double> vd, xd;
    if (vd.alloc((size_t)(j + 1) * NE) || xd.alloc((size_t)p * NE)) return IEMIC_ENOMEM;
    int rc;
    /* every entry 0x3f3f3f3f3f3f3f3f = 4.8e-4 and Q the leading columns of the identity: the
     * basis stays what it is however often the pass is repeated */
    HIP_OK(hipMemsetAsync(vd.p, 0x3f, sizeof(double) * (j + 1) * NE, c->stream));
    if ((rc = dev_zero(c, xd.p, (int64_t)p * NE))) return rc;
    std::vector<double> Q((size_t)j * p, 0.0);
    for (int q = 0; q < p; q++) Q[(size_t)q * p + q] = 1.0;
    double* xs[16] = {};
    for (int q = 0; q < p; q++) xs[q] = xd.p + (int64_t)q * NE + w.o;
    EventPair ev;
    if (ev.create()) return IEMIC_EDEVICE;
    for (int r = 0; r < 2 * nrep; r++) {
        const bool alt = r >= nrep;
        HIP_OK(hipEventRecord(ev.a, c->stream));
        if (!alt) {
            if ((rc = eigs_compress(c, vd.p + w.o, NE, j, p, Q.data(), w.n))) return rc;
        } else {
            if ((rc = eigs_ritz(c, vd.p + w.o, NE, j, p, Q.data(), xs, w.n))) return rc;
            for (int q = 0; q < p; q++)
                HIP_OK(hipMemcpyAsync(vd.p + (int64_t)q * NE + w.o, xs[q], sizeof(double) * w.n,
                                      hipMemcpyDeviceToDevice, c->stream));
            HIP_OK(hipMemcpyAsync(vd.p + (int64_t)p * NE + w.o, vd.p + (int64_t)j * NE + w.o, sizeof(double) * w.n,
                                  hipMemcpyDeviceToDevice, c->stream));
        }
        HIP_OK(hipEventRecord(ev.b, c->stream));
        HIP_OK(hipEventSynchronize(ev.b));
        float t = 0.f;
        HIP_OK(hipEventElapsedTime(&t, ev.a, ev.b));
        ms[r] = t;
    }
    return 0;
}

extern "C" int iemic_test_eig_residual(iemic_ctx* c, int64_t N, const double* ar, const double* ai, const double* xr,
                                       const double* xi, const double* B, double mu_r, double mu_i, double* out2)
{
    if (!c || !ar || !xr || !B || !out2 || (ai == nullptr) != (xi == nullptr)) return bad("null argument");
    if (N < 1 || N > (1 << 24)) return bad("residual length out of range");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    const int nvec = ai ? 5 : 3;
    DevBuf<double> d;
    if (d.alloc((size_t)nvec * N)) return IEMIC_ENOMEM;
    const double* src[5] = {ar, xr, B, ai, xi};
    int rc;
    for (int q = 0; q < nvec; q++)
        if ((rc = h2d(c, d.p + (int64_t)q * N, src[q], sizeof(double) * N))) return rc;
    return eigs_residual_sums(c, d.p, ai ? d.p + 3 * N : nullptr, d.p + N, ai ? d.p + 4 * N : nullptr, d.p + 2 * N,
                              mu_r, mu_i, N, out2);
}

extern "C" int iemic_test_active_set(iemic_ctx* c, int64_t* counts, int* act, int* atl)
{
    if (!c || !counts) return bad("null argument");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    const ActiveSet& as = c->gs.act;
    if (!c->gs.ready || c->gs.kind != 2 || !as.act.p || !as.atl.p) return bad("no block Gauss-Seidel set up");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    counts[0] = as.nact;
    counts[1] = as.natile;
    counts[2] = as.ric;
    int rc;
    if (act && (rc = d2h(c, act, as.act.p, sizeof(int) * as.nact))) return rc;
    if (atl && (rc = d2h(c, atl, as.atl.p, sizeof(int) * 8 * as.natile))) return rc;
    return 0;
}

extern "C" int iemic_test_spmv_c(iemic_ctx* c, const double* x, double* yc, double* y, int* guard_changed)
{
    if (!c || !x || !yc || !y || !guard_changed) return bad("null argument");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    StreamGuard guard{c};
    const BlockGS& gs = c->gs;
    int rc;
    /* what fgmres does before its first SpMV, and its test for the compressed basis */
    if ((rc = gs_refresh(c))) return rc;
    if (!(gs.ready && gs.kind == 2 && gs.act.nact > 0 && gs.act.cmap.p && gs.act.cmp_ok && gs.act.spc.p && gs.act.atl.p)) {
        set_error("test hook: a solve would not take the compressed SpMV");
        return IEMIC_ESTATE;
    }
    constexpr size_t G = 64;                 /* guard doubles on either side of the compressed result */
    const size_t NE = (size_t)c->sub.nerows(), NC = (size_t)NUN * gs.act.nact;
    DevBuf<double> xd, yd, ycd;
    if (xd.alloc(NE) || yd.alloc(NE) || ycd.alloc(NC + 2 * G)) return IEMIC_ENOMEM;
    /* x as iemic_spmv stages it: reference order -> ext layout (halo 0), then the exchange */
    std::vector<double> e(NE, 0.0);
    c->su.ref_to_ext(x, e.data());
    if ((rc = h2d(c, xd.p, e.data(), sizeof(double) * NE))) return rc;
    if ((rc = halo_exchange(c, xd.p, 1))) return rc;
    HIP_OK(hipMemsetAsync(yd.p, 0xff, sizeof(double) * NE, c->stream));
    HIP_OK(hipMemsetAsync(ycd.p, 0xff, sizeof(double) * (NC + 2 * G), c->stream));
    if ((rc = spmv_kernel_c(c, xd.p, ycd.p + G))) return rc;
    if ((rc = spmv_kernel(c, xd.p, yd.p))) return rc;
    std::vector<double> hc(NC + 2 * G);
    if ((rc = d2h(c, hc.data(), ycd.p, sizeof(double) * hc.size()))) return rc;
    if ((rc = d2h(c, e.data(), yd.p, sizeof(double) * NE))) return rc;
    std::vector<unsigned char> fill(sizeof(double) * G, 0xff);
    *guard_changed = (std::memcmp(hc.data(), fill.data(), fill.size()) != 0 ||
                      std::memcmp(hc.data() + G + NC, fill.data(), fill.size()) != 0) ? 1 : 0;
    std::memcpy(yc, hc.data() + G, sizeof(double) * NC);
    c->su.ext_to_ref(e.data(), y);
    return 0;
}

extern "C" int iemic_test_dyn_defect(iemic_ctx* c, int64_t NE, const double* z, const double* rr, double* d)
{
    if (!c || !z || !rr || !d) return bad("null argument");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    const BlockGS& gs = c->gs;
    if (!gs.ready || gs.kind != 2 || !gs.knP.p || !gs.act.vp) return bad("no block Gauss-Seidel set up");
    if (NE != c->sub.nerows()) return bad("vector length");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    StreamGuard guard{c};
    /* buffers of the hook's own: the preconditioner's work vectors are left as they are */
    DevBuf<double> zd, rd, dd;
    if (zd.alloc(NE) || rd.alloc(NE) || dd.alloc(NE)) return IEMIC_ENOMEM;
    int rc;
    if ((rc = h2d(c, zd.p, z, sizeof(double) * NE))) return rc;
    if ((rc = h2d(c, rd.p, rr, sizeof(double) * NE))) return rc;
    HIP_OK(hipMemsetAsync(dd.p, 0xff, sizeof(double) * NE, c->stream));
    if ((rc = spmv_dyn_defect(c, zd.p, rd.p, gs.knP.p, dd.p, false))) return rc;
    HIP_OK(hipGetLastError());
    return d2h(c, d, dd.p, sizeof(double) * NE);
}

/* columns of host vectors in the reference order -> ext columns ld apart on the device, halo
 * rows exchanged (collective on several ranks) */
static int put_columns(iemic_ctx* c, const double* H, int k, double* D, int64_t ld)
{
    std::vector<double> e((size_t)ld);
    for (int b = 0; b < k; b++) {
        std::fill(e.begin(), e.end(), 0.0);
        c->su.ref_to_ext(H + (int64_t)b * c->nrows, e.data());
        int rc = h2d(c, D + (int64_t)b * ld, e.data(), sizeof(double) * (size_t)ld);
        if (!rc) rc = halo_exchange(c, D + (int64_t)b * ld, HALO);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int iemic_test_spmm(iemic_ctx* c, int k, int kbmax, const double* V, double* W)
{
    if (!c || !V || !W) return bad("null argument");
    if (k < 1 || k > SPMM_MAX_K) return bad("k out of range");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    StreamGuard guard{c};
    const int64_t ld = c->sub.nerows();
    DevBuf<double> vd, wd;
    if (vd.alloc((size_t)ld * k) || wd.alloc((size_t)ld * k)) return IEMIC_ENOMEM;
    int rc = put_columns(c, V, k, vd.p, ld);
    if (rc) return rc;
    HIP_OK(hipMemsetAsync(wd.p, 0xff, sizeof(double) * (size_t)ld * k, c->stream));
    if ((rc = spmm_kernel(c, vd.p, ld, k, wd.p, ld, kbmax))) return rc;
    std::vector<double> e((size_t)ld);
    for (int b = 0; b < k; b++) {
        if ((rc = d2h(c, e.data(), wd.p + (int64_t)b * ld, sizeof(double) * (size_t)ld))) return rc;
        c->su.ext_to_ref(e.data(), W + (int64_t)b * c->nrows);
    }
    return 0;
}

extern "C" int iemic_test_spmm_kb(iemic_ctx* c, int kbmax)
{
    if (!c) return bad("null argument");
    if (kbmax != 0 && kbmax != 1 && kbmax != 2 && kbmax != 4) return bad("kbmax must be 0, 1, 2 or 4");
    c->pj.kbmax = kbmax;
    return 0;
}

extern "C" int iemic_test_gram(iemic_ctx* c, int ka, int kb, const double* V, const double* d, const double* W,
                               double* G)
{
    if (!c || !V || !W || !G) return bad("null argument");
    if (ka < 1 || kb < 1 || ka > c->pj.k || kb > c->pj.k) return bad("set a basis of at least max(ka, kb) columns first");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    StreamGuard guard{c};
    const int64_t ld = c->sub.nerows();
    DevBuf<double> vd, wd, dd;
    if (vd.alloc((size_t)ld * ka) || wd.alloc((size_t)ld * kb) || (d && dd.alloc((size_t)ld))) return IEMIC_ENOMEM;
    int rc = put_columns(c, V, ka, vd.p, ld);
    if (!rc) rc = put_columns(c, W, kb, wd.p, ld);
    if (!rc && d) rc = put_columns(c, d, 1, dd.p, ld);
    if (rc) return rc;
    const Owned o = owned(c);
    return proj_gram(c, vd.p + o.o, ld, ka, d ? dd.p + o.o : nullptr, wd.p + o.o, ld, kb, G);
}

extern "C" int iemic_test_sqdist2(iemic_ctx* c, int var, const double* x, const double* a, const double* b, double* out2)
{
    if (!c || !a || !b || !out2) return bad("null argument");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    StreamGuard guard{c};
    const int64_t ld = c->sub.nerows();
    DevBuf<double> xd, ad, bd;
    if ((x && xd.alloc((size_t)ld)) || ad.alloc((size_t)ld) || bd.alloc((size_t)ld)) return IEMIC_ENOMEM;
    int rc = x ? put_columns(c, x, 1, xd.p, ld) : 0;
    if (!rc) rc = put_columns(c, a, 1, ad.p, ld);
    if (!rc) rc = put_columns(c, b, 1, bd.p, ld);
    if (rc) return rc;
    return score_sqdist2(c, var, x ? xd.p : c->d_x.p, ad.p, bd.p, out2);
}

extern "C" int iemic_test_gram_cost(iemic_ctx* c, int k, int nrep, double* ms)
{
    if (!c || !ms || nrep < 1) return bad("null argument");
    if (k < 1 || k > c->pj.k) return bad("set a basis of at least k columns first");
    if (c->sub.nranks != 1) return bad("a single-rank context is needed");
    if (hipSetDevice(c->device) != hipSuccess) return IEMIC_EDEVICE;
    StreamGuard guard{c};
    const int64_t ld = c->sub.nerows();
    const Owned o = owned(c);
    const Projected& p = c->pj;
    std::vector<double> G((size_t)k * k);
    EventPair ev;
    if (ev.create()) return IEMIC_EDEVICE;
    int rc = proj_gram(c, p.V.p + o.o, ld, k, nullptr, p.W.p + o.o, ld, k, G.data());   /* warm */
    if (rc) return rc;
    float t = 0;
    HIP_OK(hipEventRecord(ev.a, c->stream));
    for (int r = 0; r < nrep; r++)
        if ((rc = proj_gram(c, p.V.p + o.o, ld, k, nullptr, p.W.p + o.o, ld, k, G.data()))) return rc;
    HIP_OK(hipEventRecord(ev.b, c->stream));
    DEV_WAIT_EVENT(c, ev.b);
    HIP_OK(hipEventElapsedTime(&t, ev.a, ev.b));
    ms[0] = t / nrep;
    /* what it replaces: one multi-dot pair per column of W, its k results fetched */
    HIP_OK(hipEventRecord(ev.a, c->stream));
    for (int r = 0; r < nrep; r++)
        for (int b = 0; b < k; b++)
            if ((rc = mdot_host(c, p.V.p + o.o, ld, k, p.W.p + (int64_t)b * ld + o.o, G.data() + (size_t)b * k))) return rc;
    HIP_OK(hipEventRecord(ev.b, c->stream));
    DEV_WAIT_EVENT(c, ev.b);
    HIP_OK(hipEventElapsedTime(&t, ev.a, ev.b));
    ms[1] = t / nrep;
    /* the same launches with one fetch: k multi-dot pairs into the rows of one result array */
    DevBuf<double> res;
    if (res.alloc((size_t)k * k)) return IEMIC_ENOMEM;
    HIP_OK(hipEventRecord(ev.a, c->stream));
    for (int r = 0; r < nrep; r++) {
        for (int b = 0; b < k; b++) {
            hipLaunchKernelGGL(k_mdot, dim3(RED_BLOCKS, k), dim3(256), 0, c->stream, p.V.p + o.o, ld, k,
                               p.W.p + (int64_t)b * ld + o.o, o.n, c->d_part.p);
            hipLaunchKernelGGL(k_mdot_final, dim3(k), dim3(256), 0, c->stream, c->d_part.p, RED_BLOCKS, k,
                               res.p + (size_t)b * k);
        }
        if ((rc = d2h(c, G.data(), res.p, sizeof(double) * k * k))) return rc;
    }
    HIP_OK(hipEventRecord(ev.b, c->stream));
    DEV_WAIT_EVENT(c, ev.b);
    HIP_OK(hipEventElapsedTime(&t, ev.a, ev.b));
    ms[2] = t / nrep;
    return 0;
}

extern "C" int iemic_test_solver_calls(iemic_ctx* c, int64_t* out)
{
    if (!c || !out) return bad("null argument");
    out[0] = c->ncalls[0];
    out[1] = c->ncalls[1];
    return 0;
}
