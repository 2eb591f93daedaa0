/*
 * prec_gs.hip -- block Gauss-Seidel preconditioner for the THCM Jacobian (prec = 2): the apply.
 *
 * Replaces the reference's TRIOS::BlockPreconditioner with MRILU/ML sub-solves
 * (src/trios/TRIOS_BlockPreconditioner.C, after de Niet & Wubs)
 * by a fully GPU-resident variant of the same block structure.  Unknowns are split into
 *   known   identity rows (land, rigid lid, closed boundaries): z = r
 *   dyn     U/V (horizontal momentum), W (hydrostatic rows), P (continuity rows)
 *   ts      T/S (heat and salt)
 * and solved in the order known -> dyn -> ts (block lower triangular: the buoyancy and
 * momentum couplings from T/S into the dynamics are the dropped upper part):
 *   1. ptil : hydrostatic rows  Gw ptil = r_w, column-wise top-down with p_top = 0
 *   2. uv*  : D^-1 (r_uv - Guv ptil), D = per-point 2x2 U/V (Coriolis) block
 *   3. pbar : depth-integrated continuity per water column, 2-D Schur complement
 *             S = Mz2 Duv D^-1 Guv Mz1^T (9-point, corner-staggered), null space pinned
 *             (one column per checkerboard colour and basin), solved exactly by block
 *             cyclic reduction over longitudes (schur_cr.hip)
 *   4. uv   : uv* - D^-1 Guv Mz1^T pbar,  p = ptil + Mz1^T pbar
 *   5. w    : continuity rows Dw w = r_p - Duv uv, column-wise bottom-up
 *   6. ts   : A_ts ts = r_ts - B_ts,uv uv - B_ts,w w, by symmetric red-black Gauss-Seidel
 *             sweeps with 2x2 T/S cell blocks (parity of i+j+k)
 * Every step is a structured-grid kernel over cells or water columns reading the
 * stencil-ELL Jacobian in place; the only dense objects are the m x m blocks of the
 * Schur cyclic reduction (O(n m^2) doubles, 40 MB at 2 degrees).
 * The set-up is gs_setup.hip, steps 1-5 (one dynamics pass) gs_dyn.hip, step 6 ts_sweeps.hip or
 * the multigrid of ts_mg.hip; this unit has the right-hand side and the order of the passes.
 */
#include "gs_internal.h"

namespace iemic {

namespace {

/* The output z = r on identity rows (zall: and 0 on the others -- the T/S sweeps iterate
 * on z; otherwise the last dynamics pass and the T/S multigrid write every active row);
 * rr = r - A(:, known) r(known) on the others (slot bitmask), to the planar rrP and
 * (rr != null, the T/S sweeps) AoS.  The planar iterate zP is 0 on the identity rows and on
 * T/S (zeroed when the preconditioner is computed, never written there) and the first pass
 * writes its active dynamics rows before reading them, so the apply does not touch it here:
 * the identity rows' couplings are in rr, every kernel of the passes reads zP on the active
 * rows and the dynamics defect is rr - A zP over all its slots */
__global__ void k_gs_rr(const double* __restrict__ val, const uint8_t* __restrict__ known,
                        const uint64_t* __restrict__ kmask, const double* __restrict__ r,
                        double* __restrict__ z, double* __restrict__ rr, int zall,
                        double* __restrict__ rrP, Lay L)
{
    LAY_ALIASES;
    OWNED_CELL;
    double acc[NUN];
    bool kn[NUN];
#pragma unroll
    for (int R = 0; R < NUN; R++) {
        const int64_t row = NUN * cell + R;
        acc[R] = r[row];
        kn[R] = known[row] != 0;
        if (kn[R] || zall) z[row] = kn[R] ? acc[R] : 0.0;
    }
    uint64_t b[2] = {kmask[2 * cell], kmask[2 * cell + 1]};
    if (b[0] | b[1]) {
        for (int h = 0; h < 2; h++)
            while (b[h]) {
                const int s = 64 * h + __builtin_ctzll(b[h]);
                b[h] &= b[h] - 1;
                int R = 0;
                while (s >= ROW_BEGIN[R + 1]) R++;
                int ii = i + SLOTS[s].di, jj = j + SLOTS[s].dj;
                const int kk = k + SLOTS[s].dk;
                hnb(ii, jj, n, m, periodic);
                const int64_t col = NUN * ecell(L, ii, jj, kk) + SLOTS[s].var;
                acc[R] -= val[(int64_t)s * ncell + lc] * r[col];
            }
    }
#pragma unroll
    for (int R = 0; R < NUN; R++) {
        const double v = kn[R] ? 0.0 : acc[R];
        if (rr) rr[NUN * cell + R] = v;
        rrP[PL(cell, R)] = v;
    }
}

/* k_gs_rr for a compressed input (FGMRES's Arnoldi vectors, krylov.hip): r is zero on every
 * identity row (land cells are not stored, the identity rows of active cells are 0), so the
 * identity-column couplings vanish and rr = r on the active rows; the output z is 0 on the
 * identity rows (zall: on every row) */
__global__ void k_gs_rr_c(const uint8_t* __restrict__ known, const int* __restrict__ cmap,
                          const double* __restrict__ rc, double* __restrict__ z, double* __restrict__ rr,
                          int zall, double* __restrict__ rrP, Lay L)
{
    LAY_ALIASES;
    OWNED_CELL;
    const int cm = cmap[lc];
#pragma unroll
    for (int R = 0; R < NUN; R++) {
        const int64_t row = NUN * cell + R;
        const bool kn = known[row] != 0;
        const double v = (kn || cm < 0) ? 0.0 : rc[(int64_t)NUN * cm + R];
        if (kn || zall) z[row] = 0.0;
        if (rr) rr[row] = v;
        rrP[PL(cell, R)] = v;
    }
}

}  // namespace

/* the T/S block solve: right-hand side rr_TS - A_TS,D z_D from the dynamics iterate zd (the
 * planar zP for the multigrid, the AoS output for the sweeps), then ts_mg V-cycles
 * (ts_mg.hip: out, side) or ts_sweeps symmetric red-black sweeps (ts_sweeps.hip), result into
 * z(T, S) of the output z */
static int ts_solve(iemic_ctx* c, const double* zd, double* z, bool out, bool side = false)
{
    if (c->gs.ts_mg > 0) return ts_mg_solve(c, zd, z, out, side);
    return ts_sweeps_solve(c, z);
}

/* GPU time of the apply's parts (HIP events on the library stream, nrep back-to-back
 * launches each, zero data): us[0] one Schur solve (cyclic reduction), us[1] one T/S block
 * solve (right-hand side + V-cycle), us[2] one dynamics pass (column kernels + Schur solve),
 * us[3] one dynamics defect.  Diagnostics for DESIGN.md's per-part table (one rank). */
int gs_time_parts(iemic_ctx* c, int nrep, double* us)
{
    BlockGS& gs = c->gs;
    if (!gs.ready || gs.kind != 2 || nrep < 1) {
        set_error("gs_time_parts: the block GS preconditioner is not computed");
        return IEMIC_ESTATE;
    }
    if (c->sub.nranks > 1) {   /* parts 2 and 3 exchange halos: not callable on one rank alone */
        set_error("gs_time_parts: one-rank diagnostic, the context has " + std::to_string(c->sub.nranks) + " ranks");
        return IEMIC_EINVAL;
    }
    hipStream_t s = c->stream;
    EventPair ev;
    if (ev.create()) return IEMIC_EDEVICE;
    const hipEvent_t e0 = ev.a, e1 = ev.b;
    double* z = c->d_tmp2.p;
    HIP_OK(hipMemsetAsync(c->d_tmp1.p, 0, sizeof(double) * c->sub.nerows(), s));
    HIP_OK(hipMemsetAsync(z, 0, sizeof(double) * c->sub.nerows(), s));
    HIP_OK(hipMemsetAsync(gs.rr.p, 0, sizeof(double) * c->sub.nerows(), s));
    HIP_OK(hipMemsetAsync(gs.rrP.p, 0, sizeof(double) * c->sub.nerows(), s));
    HIP_OK(hipMemsetAsync(gs.zP.p, 0, sizeof(double) * c->sub.nerows(), s));
    HIP_OK(hipMemsetAsync(gs.colv_own.p, 0, sizeof(double) * c->n * c->m, s));
    int rc = 0;
    for (int part = 0; part < 4 && !rc; part++) {
        auto once = [&]() -> int {
            switch (part) {
            case 0: return cr_solve(c, gs.cr, gs.colv_own.p, gs.colv2.p, s);
            case 1: return ts_solve(c, gs.ts_mg > 0 ? gs.zP.p : z, z, true);
            case 2: return dyn_solve(c, gs.rrP.p, gs.zP.p);
            default: return spmv_dyn_defect(c, gs.zP.p, c->d_tmp1.p, gs.knP.p, gs.dres.p ? gs.dres.p : c->d_tmp1.p);
            }
        };
        if ((rc = once())) break;                  /* warm */
        HIP_OK(hipEventRecord(e0, s));
        for (int q = 0; q < nrep && !rc; q++) rc = once();
        HIP_OK(hipEventRecord(e1, s));
        HIP_OK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        us[part] = 1e3 * ms / nrep;
    }
    return rc;
}

/* ---- the apply: the steps of gs_apply_impl, in its order ----------------------------- */

namespace {

/* what one apply derives from BlockGS and Sub */
struct ApplyPlan {
    bool band;                       /* subdomains: exchanges and all-reduces                */
    /* the T/S block is solved with the right-hand side rr_TS - A_TS,D z_D of the dynamics
     * iterate after ts_at passes (default: after the last; the CPU twin: orc_gs_apply); the
     * later passes neither read nor write the T/S rows */
    int ts_at;
    /* early T/S on one rank: its V-cycles run on the side stream beside the remaining
     * dynamics passes (both chains are latency-bound, so they overlap) */
    bool par;
    /* the dynamics passes iterate on the planar zP; the output z (AoS) gets their final
     * values from the last pass (every pass for the T/S sweeps, which read z's AoS rows) */
    bool aos_all;
    /* latitude bands: the last pass also updated the iterate's south halo row U/V (k_gs_uvp),
     * all the T/S right-hand side reads of it beyond the band (A_TS,D couples U/V at j - 1 and
     * W in the column): no exchange (the fixed-step passes only) */
    bool ts_local;
    /* latitude bands: the defect on the two halo rows too (from a 2-deep halo of the U/V/W/P
     * planes), so that the pass needs no exchange of it (2 -> 1 exchange batch per pass) */
    bool dhalo;
    /* the AoS output of a pass: z on the last pass (aos_all: on every pass), else none */
    double* zaos(double* z, bool last) const { return (last || aos_all) ? z : nullptr; }
};

}  // namespace

static ApplyPlan apply_plan(const iemic_ctx* c)
{
    const BlockGS& gs = c->gs;
    ApplyPlan P;
    P.band = c->sub.nranks > 1;
    P.ts_at = (!gs.dyn_mr && gs.ts_at >= 1 && gs.ts_at < gs.dyn_iters) ? gs.ts_at : gs.dyn_iters;
    P.par = P.ts_at < gs.dyn_iters && !P.band && gs.ts_mg > 0;
    P.aos_all = gs.ts_mg <= 0;
    P.ts_local = P.band && c->sub.npx == 1 && gs.ts_mg > 0 && !gs.dyn_mr && P.ts_at == gs.dyn_iters &&
                 gs.dyn_iters > 1;
    P.dhalo = P.band && c->sub.npx == 1 && gs.act.dvh.p;
    return P;
}

/* z on the identity rows and the right-hand side rr of the passes (k_gs_rr, k_gs_rr_c) */
static int apply_rhs(iemic_ctx* c, const ApplyPlan& P, const double* r, double* z, bool cmp, bool staged)
{
    BlockGS& gs = c->gs;
    const Lay L = lay_of(c->sub);
    const unsigned gc = blocks_for(c->sub.nloc);
    hipStream_t s = c->stream;
    int rc;
    /* the halo rows of r hold the neighbours' identity-row values the couplings need (a
     * compressed r is zero on every identity row: no couplings, no exchange) */
    if (cmp) {
        /* staged: the update pass wrote rrP (its land entries stay 0 since the set-up, the
         * identity rows of z were zeroed per set-up: Krylov::zclean) */
        if (!staged || P.aos_all)
            hipLaunchKernelGGL(k_gs_rr_c, dim3(gc), dim3(256), 0, s, gs.known.p, gs.act.cmap.p, r, z,
                               P.aos_all ? gs.rr.p : nullptr, P.aos_all ? 1 : 0, gs.rrP.p, L);
    } else {
        if (P.band && (rc = halo_exchange(c, const_cast<double*>(r), 1))) return rc;
        hipLaunchKernelGGL(k_gs_rr, dim3(gc), dim3(256), 0, s, gs.act.vp, gs.known.p, gs.kmask.p,
                           r, z, P.aos_all ? gs.rr.p : nullptr, P.aos_all ? 1 : 0, gs.rrP.p, L);
    }
    return 0;
}

/* the T/S step: the neighbours' dynamics iterate where the right-hand side reads it, then
 * the block solve */
static int apply_ts(iemic_ctx* c, const ApplyPlan& P, double* z)
{
    BlockGS& gs = c->gs;
    double* zP = gs.zP.p;
    int rc;
    if (P.band && !P.ts_local && (P.ts_at < gs.dyn_iters || gs.dyn_iters > 1)) {
        rc = gs.ts_mg > 0 ? halo_exchange_planar(c, zP, NUN, c->sub.next, 1) : halo_exchange(c, z, 1);
        if (rc) return rc;
    }
    return ts_solve(c, gs.ts_mg > 0 ? zP : z, z, P.ts_at == gs.dyn_iters, P.par);
}

/* defect correction on the dynamics block: z_D += w M_D^-1 (rr_D - A_DD z_D), with the
 * minimal-residual w (dyn_mr) */
static int apply_mr_passes(iemic_ctx* c, const ApplyPlan& P, double* z)
{
    BlockGS& gs = c->gs;
    const int64_t ps = c->sub.next;
    double* zP = gs.zP.p;
    int rc;
    if (gs.dyn_iters <= 1) return 0;
    if (P.band && (rc = halo_exchange_planar(c, zP, NUN, ps, 1))) return rc;
    if ((rc = spmv_dyn_defect(c, zP, gs.rrP.p, gs.knP.p, gs.dres.p))) return rc;
    for (int it = 1; it < gs.dyn_iters; it++) {
        const bool last = it + 1 == gs.dyn_iters;
        if ((rc = dyn_solve(c, gs.dres.p, gs.zc.p))) return rc;
        if (P.band && (rc = halo_exchange_planar(c, gs.zc.p, NUN, ps, 1))) return rc;
        if ((rc = spmv_dyn_defect(c, gs.zc.p, gs.dzero.p, gs.knP.p, gs.dq.p))) return rc;
        if ((rc = dyn_mr_step(c, !last, P.zaos(z, last)))) return rc;
    }
    return 0;
}

/* the same with the fixed w = dyn_omega; the T/S step follows pass ts_at where that is not the last */
static int apply_fixed_passes(iemic_ctx* c, const ApplyPlan& P, double* z)
{
    BlockGS& gs = c->gs;
    const int64_t ps = c->sub.next;
    double* zP = gs.zP.p;
    int rc;
    for (int it = 1; it < gs.dyn_iters; it++) {
        const bool last = it + 1 == gs.dyn_iters;
        if (P.band && (rc = P.dhalo ? halo_exchange_planar(c, zP, 4, ps, 2) : halo_exchange_planar(c, zP, NUN, ps, 1)))
            return rc;   /* w, p of the neighbours */
        if ((rc = spmv_dyn_defect(c, zP, gs.rrP.p, gs.knP.p, gs.dres.p, P.dhalo))) return rc;
        const bool schur = gs_pass_schur(gs, it);
        if ((rc = dyn_solve(c, gs.dres.p, gs.zc.p, zP, gs.dyn_omega, P.zaos(z, last), P.dhalo, schur)))
            return rc;   /* z += w zc */
        if (it + 1 == P.ts_at && it + 1 < gs.dyn_iters && (rc = apply_ts(c, P, z))) return rc;
    }
    return 0;
}

static int gs_apply_impl(iemic_ctx* c, const double* r, double* z, bool cmp, bool staged)
{
    BlockGS& gs = c->gs;
    int rc = gs_refresh(c);
    if (rc) return rc;
    const ApplyPlan P = apply_plan(c);
    if ((rc = apply_rhs(c, P, r, z, cmp, staged))) return rc;
    if ((rc = dyn_solve(c, gs.rrP.p, gs.zP.p, nullptr, 0.0, P.zaos(z, gs.dyn_iters == 1)))) return rc;
    if (P.ts_at == 1 && gs.dyn_iters > 1 && (rc = apply_ts(c, P, z))) return rc;
    if ((rc = gs.dyn_mr ? apply_mr_passes(c, P, z) : apply_fixed_passes(c, P, z))) return rc;
    if (P.ts_at == gs.dyn_iters && (rc = apply_ts(c, P, z))) return rc;
    if (P.ts_at < gs.dyn_iters && gs.ts_mg > 0) {
        if (P.par) HIP_OK(OnSide::wait(c));                        /* join */
        if ((rc = ts_mg_out(c, z))) return rc;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int gs_apply(iemic_ctx* c, const double* r, double* z) { return gs_apply_impl(c, r, z, false, false); }
int gs_apply_c(iemic_ctx* c, const double* rc, double* z, bool staged) { return gs_apply_impl(c, rc, z, true, staged); }

}  // namespace iemic
