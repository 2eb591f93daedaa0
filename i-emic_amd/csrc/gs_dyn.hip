/*
 * gs_dyn.hip -- the dynamics pass of the block Gauss-Seidel preconditioner (prec_gs.hip has the
 * overview): z(U/V/W/P) from a right-hand side rr, both component-planar, in three kernels
 * around the Schur solve, and the minimal-residual step of the defect correction.
 *   1. ptil : hydrostatic rows  Gw ptil = r_w, column-wise top-down with p_top = 0
 *   2. uv*  : D^-1 (r_uv - Guv ptil), D = per-point 2x2 U/V (Coriolis) block
 *   3. pbar : depth-integrated continuity per water column, 2-D Schur complement
 *             S = Mz2 Duv D^-1 Guv Mz1^T (9-point, corner-staggered), null space pinned
 *             (one column per checkerboard colour and basin), solved exactly by block
 *             cyclic reduction over longitudes (schur_cr.hip)
 *   4. uv   : uv* - D^-1 Guv Mz1^T pbar,  p = ptil + Mz1^T pbar
 *   5. w    : continuity rows Dw w = r_p - Duv uv, column-wise bottom-up
 *
 * ---- the Schur right-hand side as a linear form in rr ----------------------------------
 * Steps 1-3a (ptil, uv*, the depth-weighted continuity defect) are linear in rr, so the
 * Schur right-hand side of water column (i, j) is a fixed combination of rr over its
 * neighbourhood: W rows of the 3 x 3 columns around it (through ptil, which the U/V points
 * of its four corners read), U/V rows of those corners, its own P rows.  The coefficients
 * are formed at set-up (gs_setup.hip: k_rcol_uvp, k_rcol_w), so the apply evaluates ptil and the
 * right-hand side in one column kernel (k_gs_ptil_rcol) and the U/V points only once, after
 * the Schur solve (k_gs_uvp): two launches fewer per dynamics pass.
 * Layout: rcol[(e * l + k) * ncolb + t], t = band column (j - jb0) * nx + (i - ib0);
 * e < 9: rr_W at column (i + e % 3 - 1, j + e / 3 - 1), level k; e = 9 + q4 / 13 + q4: rr_U
 * / rr_V at corner q4 = (i - (q4 & 1), j - (q4 >> 1)); e = 17: rr_P at (i, j, k)
 * (RC_NE = 18 coefficients per level).
 */
#include "gs_internal.h"

namespace iemic {

namespace {

/* Column kernels, transposed: one workgroup of 1024 threads per tile of COL_TI = 1024 / LP
 * consecutive columns of one latitude row (LP = power of two >= l), thread = (column, level)
 * with the column fastest, so every per-cell load of a wave runs along i in 128-byte runs
 * (the slot-major Jacobian rows and the planar dynamics vectors contiguously: with the
 * interleaved AoS vectors at a 48-byte cell stride the U/V and p/w kernels took 12.3 and
 * 12.6 against 7.2 and 6.9 us, scripts/ab/soa_probe.sh);
 * the column recurrences meet in LDS, where each thread composes the affine maps of the
 * levels it depends on (at most l steps of LDS reads).  At 2 degrees (LP = 16) 64-column
 * tiles, 232 workgroups: 16-column tiles (928 of 256 threads) measured 2 ms slower per
 * Newton step (scripts/ab_probe.py). */
template <int LP>
constexpr int col_ti() { return 1024 / LP; }

/* hr: the grid also covers the halo rows jl = -1 and jl = mb (latitude bands: the pass
 * recomputes the neighbours' edge values it reads instead of exchanging them) */
template <int LP>
__device__ __forceinline__ bool col_tile(const Lay& L, int& il, int& jl, int& k, bool& on, int hr = 0)
{
    constexpr int TI = col_ti<LP>();
    const int tpr = (L.nx + TI - 1) / TI;
    const int w = xcd_block(tpr * ((int)(L.nloc / ((int64_t)L.l * L.nx)) + 2 * hr));
    if (w < 0) return false;
    jl = w / tpr - hr;
    il = (w % tpr) * TI + (int)threadIdx.x % TI;
    k = (int)threadIdx.x / TI;
    on = k < L.l && il < L.nx;
    return true;
}

/* Duv uv at a P cell: sum over the 4 U/V corners (P row slots 54..61) */
/* pl: owned index (Jacobian column) of the P cell */
__device__ __forceinline__ double duv_uv(const double* __restrict__ val, const uint8_t* __restrict__ knP,
                                         const double* __restrict__ z, int i, int j, int k,
                                         int64_t pl, const Lay& L)
{
    /* branch-free: a corner outside the domain reads the cell itself with weight 0 */
    const int n = L.n, m = L.m, periodic = L.periodic;
    const int64_t ncell = L.nloc, pc = pl;
    double acc = 0.0;
#pragma unroll
    for (int q4 = 0; q4 < 4; q4++) {
        int qi = i - (q4 & 1), qj = j - ((q4 >> 1) & 1);
        const bool in = hnb(qi, qj, n, m, periodic);
        if (!in) { qi = i; qj = j; }
        const int64_t qc = ecell(L, qi, qj, k);
        const uint8_t ku = knP[PL(qc, UU)], kv = knP[PL(qc, VV)];
        const double au = val[(int64_t)(S_PU + q4) * ncell + pc], av = val[(int64_t)(S_PV + q4) * ncell + pc];
        const double zu = z[PL(qc, UU)], zv = z[PL(qc, VV)];
        acc += (in && !ku) ? au * zu : 0.0;
        acc += (in && !kv) ? av * zv : 0.0;
    }
    return acc;
}

/* 4b/5. p = ptil + pbar and the continuity rows bottom-up, w_k = A_k + B_k w_k-1 (the
 * transposed column layout of k_gs_ptil_rcol); zo += omega (p, w) in the correction passes */
template <int LP>
__global__ void __launch_bounds__(1024) k_gs_pw_t(const double* __restrict__ val,
                                                  const uint8_t* __restrict__ knP,
                                                  const double* __restrict__ pbar,
                                                  double* __restrict__ z, Lay L,
                                                  const double* __restrict__ rr,
                                                  double* __restrict__ zo, double omega,
                                                  double* __restrict__ zaos)
{
    constexpr int TI = col_ti<LP>();
    __shared__ double sA[LP][TI], sB[LP][TI];
    int il, jl, k;
    bool on;
    if (!col_tile<LP>(L, il, jl, k, on)) return;    /* whole idle workgroups */
    const int ii = (int)threadIdx.x % TI;
    const int i = L.ib0 + il, j = L.jb0 + jl;
    const int64_t ncell = L.nloc;
    double A = 0.0, B = 0.0, pb = 0.0, zp = 0.0;
    bool pa = false, wa = false;
    int64_t cell = 0;
    if (on) {
        cell = ecell(L, i, j, k);
        const uint8_t kp = knP[PL(cell, PP)], kw = knP[PL(cell, WW)];
        pa = !kp;
        wa = !kw;
    }
    if (pa) {
        /* an inactive P row (land) reads nothing: its (A, B) = (0, 0) */
        const double a = val[(int64_t)S_PW0 * ncell + (cell - L.own0)];
        const double b = val[(int64_t)S_PWM * ncell + (cell - L.own0)];
        const double rhs = rr[PL(cell, PP)] - duv_uv(val, knP, z, i, j, k, cell - L.own0, L);
        pb = pbar[(int64_t)j * L.n + i];
        zp = z[PL(cell, PP)];
        if (wa && a != 0.0) {
            A = rhs / a;
            B = -b / a;
        }
    }
    if (k < LP) {
        sA[k][ii] = A;
        sB[k][ii] = B;
    }
    __syncthreads();
    if (!on) return;
    double w = 0.0;
    for (int kk = 0; kk <= k; kk++) w = sA[kk][ii] + sB[kk][ii] * w;
    const double pn = zp + pb, wn = pa ? w : 0.0;
    if (pa) z[PL(cell, PP)] = pn;
    if (wa) z[PL(cell, WW)] = wn;
    double fp = pn, fw = wn;
    if (zo) {
        if (pa) zo[PL(cell, PP)] = fp = zo[PL(cell, PP)] + omega * pn;
        if (wa) zo[PL(cell, WW)] = fw = zo[PL(cell, WW)] + omega * wn;
    }
    /* the last pass: the final P/W rows into the preconditioner output (AoS) */
    if (zaos) {
        if (pa) zaos[NUN * cell + PP] = fp;
        if (wa) zaos[NUN * cell + WW] = fw;
    }
}

/* 1 + 3a. ptil (top-down: p_k = A_k + B_k p_k+1) and the column's Schur right-hand side
 * sum_e rcol_e rr_e (summed over the levels in a fixed order), written as k_gs_pcol wrote it */
/* gsl (latitude bands): the tiles of the halo rows jl = -1, mb (inside the grid) compute
 * ptil there too, with the W row's couplings from the halo-filled gslot (the owned Jacobian
 * has no halo rows), so that the U/V kernel needs no exchange of ptil */
/* RC = false: ptil only (a pass without the Schur solve needs no right-hand side for it) */
template <int LP, bool RC = true>
__global__ void __launch_bounds__(1024) k_gs_ptil_rcol(const double* __restrict__ val,
                                                       const uint8_t* __restrict__ knP,
                                                       const double* __restrict__ rcol,
                                                       const double* __restrict__ rr,
                                                       double* __restrict__ z,
                                                       const int* __restrict__ ocol,
                                                       double* __restrict__ colv_own, Lay L,
                                                       const double* __restrict__ gsl)
{
    LAY_ALIASES;
    constexpr int TI = col_ti<LP>();
    __shared__ double sA[LP][TI], sB[LP][TI], sv[LP][TI];
    int il, jl, k;
    bool on;
    if (!col_tile<LP>(L, il, jl, k, on, gsl ? 1 : 0)) return;    /* whole idle workgroups */
    const int ii = (int)threadIdx.x % TI;
    const int i = L.ib0 + il, j = L.jb0 + jl;
    const int mbl = (int)(L.nloc / ((int64_t)l * L.nx));
    if (jl < 0 || jl >= mbl) {
        /* a halo row: ptil only (rows outside the grid: whole idle workgroups) */
        if (j < 0 || j >= m) return;
        double A = 0.0, B = 0.0;
        bool pa = false;
        int64_t cell = 0;
        if (on) {
            cell = ecell(L, i, j, k);
            pa = !knP[PL(cell, PP)];
            if (pa && k < l - 1 && !knP[PL(cell, WW)]) {
                const double g0 = gsl[GSL * cell + 8], g1 = gsl[GSL * cell + 9];
                if (g0 != 0.0) {
                    A = rr[PL(cell, WW)] / g0;
                    B = -g1 / g0;
                }
            }
        }
        if (k < LP) {
            sA[k][ii] = A;
            sB[k][ii] = B;
        }
        __syncthreads();
        if (!on) return;
        double p = 0.0;
        for (int kk = l - 1; kk >= k; kk--) p = sA[kk][ii] + sB[kk][ii] * p;
        if (pa) z[PL(cell, PP)] = p;
        return;
    }
    const int64_t ncell = L.nloc;
    const int ncolb = (int)(L.nloc / l);
    const int t = jl * L.nx + il;
    double A = 0.0, B = 0.0, v = 0.0;
    bool pa = false;
    int64_t cell = 0;
    if (on) {
        cell = ecell(L, i, j, k);
        const uint8_t kp = knP[PL(cell, PP)], kw = knP[PL(cell, WW)];
        pa = !kp;
        if constexpr (RC) {
            int64_t nc9[9];
#pragma unroll
            for (int e = 0; e < 9; e++) {
                int i2 = i + e % 3 - 1, j2 = j + e / 3 - 1;
                if (!hnb(i2, j2, n, m, periodic)) { i2 = i; j2 = j; }
                nc9[e] = ecell(L, i2, j2, k);
            }
            const double* R = rcol + (int64_t)k * ncolb + t;
            const int64_t es = (int64_t)l * ncolb;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
            for (int e = 0; e < 9; e++) a0 += R[e * es] * rr[PL(nc9[e], WW)];
            if (pa) {
                /* the corner and own-P coefficients vanish on an inactive P row (land): not read */
#pragma unroll
                for (int q4 = 0; q4 < 4; q4++) {
                    /* corner q4 = (i - (q4 & 1), j - (q4 >> 1)): neighbour (1 - (q4 >> 1)) * 3 + 1 - (q4 & 1) */
                    const int64_t qc = nc9[(1 - ((q4 >> 1) & 1)) * 3 + 1 - (q4 & 1)];
                    a1 += R[(9 + q4) * es] * rr[PL(qc, UU)];
                    a2 += R[(13 + q4) * es] * rr[PL(qc, VV)];
                }
                a2 += R[17 * es] * rr[PL(cell, PP)];
            }
            v = a0 + (a1 + a2);
        }
        if (pa) {
            if (k < l - 1 && !kw) {
                const double g0 = val[(int64_t)S_WP0 * ncell + (cell - L.own0)];
                const double g1 = val[(int64_t)S_WP1 * ncell + (cell - L.own0)];
                if (g0 != 0.0) {
                    A = rr[PL(cell, WW)] / g0;
                    B = -g1 / g0;
                }
            }
        }
    }
    if (k < LP) {
        sA[k][ii] = A;
        sB[k][ii] = B;
        if constexpr (RC) sv[k][ii] = v;
    }
    __syncthreads();
    if (!on) return;
    double p = 0.0;
    for (int kk = l - 1; kk >= k; kk--) p = sA[kk][ii] + sB[kk][ii] * p;
    if (pa) z[PL(cell, PP)] = p;
    if (RC && k == 0) {
        const int q = ocol[j * n + i];
        double s = 0.0;
        for (int kk = 0; kk < l; kk++) s += sv[kk][ii];
        if (q >= 0) colv_own[q] = s;
        else if (q != -1) colv_own[-2 - q] = 0.0;
    }
}

/* Minimal-residual defect correction: with d the defect and q = -A_DD zc the change a
 * full correction zc would make to it, the step w = argmin ||d + w q|| = -(d.q)/(q.q).
 * Block partials in a fixed order (deterministic), summed by one thread. */
/* over the owned cells of the planar U/V/W/P planes (fixed grid-stride order) */
__global__ void __launch_bounds__(256) k_mr_dots(const double* __restrict__ d, const double* __restrict__ q,
                                                 Lay L, double* __restrict__ part)
{
    __shared__ double s0[256], s1[256];
    double a = 0.0, b = 0.0;
    const int64_t n = 4 * L.nloc;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = PL(L.own0 + t % L.nloc, t / L.nloc);
        const double qv = q[e];
        a += d[e] * qv;
        b += qv * qv;
    }
    s0[threadIdx.x] = a;
    s1[threadIdx.x] = b;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s0[threadIdx.x] += s0[threadIdx.x + w];
            s1[threadIdx.x] += s1[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s0[0];
        part[gridDim.x + blockIdx.x] = s1[0];
    }
}
__global__ void k_mr_sum(double* __restrict__ part, int nb)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a = 0.0, b = 0.0;
    for (int e = 0; e < nb; e++) {
        a += part[e];
        b += part[nb + e];
    }
    part[2 * nb] = a;
    part[2 * nb + 1] = b;
}
/* z += w zc, and (upd) d += w q, on the active U/V/W/P rows (planar); zaos: the final
 * values into the preconditioner output (AoS) */
__global__ void k_mr_update(const uint8_t* __restrict__ knP, const double* __restrict__ sums,
                            const double* __restrict__ zc, const double* __restrict__ q,
                            double* __restrict__ z, double* __restrict__ d, Lay L, int upd,
                            double* __restrict__ zaos)
{
    OWNED_CELL;
    const double w = sums[1] > 0.0 ? -sums[0] / sums[1] : 0.0;
#pragma unroll
    for (int R = UU; R <= PP; R++) {
        const int64_t e = PL(cell, R);
        if (knP[e]) continue;
        const double zn = z[e] + w * zc[e];
        z[e] = zn;
        if (upd) d[e] += w * q[e];
        if (zaos) zaos[NUN * cell + R] = zn;
    }
}

/* 2 + 4. uv = D^-1 (rr_uv - Guv (ptil + Mz1^T pbar)) in one pass once pbar is known (the
 * Schur right-hand side came from rcol, so uv* is never formed); zo += omega uv */
/* gsl (latitude bands): threads past the owned cells compute the south halo row's U/V
 * points too (their P couplings from the halo-filled gslot), into z only, so that the p/w
 * kernel needs no exchange of uv */
/* alist: the threads run over the active cells (nown of them; ActiveSet::act), the land
 * cells' U/V points being identity rows */
__global__ void k_gs_uvp(const double* __restrict__ val, const uint8_t* __restrict__ knP,
                         const double* __restrict__ uvinv, const double* __restrict__ rr,
                         const double* __restrict__ pbar, double* __restrict__ z, Lay L,
                         double* __restrict__ zo, double omega, double* __restrict__ zaos,
                         const double* __restrict__ gsl, const int* __restrict__ alist, int64_t nown)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ncell = L.nloc;
    const int n = L.n, m = L.m, periodic = L.periodic;
    int i, j, k;
    int64_t cell, lc = 0;
    const bool halo = t >= nown;
    if (!halo) {
        lc = alist ? (int64_t)alist[t] : t;
        cell = L.own0 + lc;
        lc_ijk(L, lc, i, j, k);
    } else {
        const int64_t q = t - nown;                  /* south halo row, (k, i) */
        if (!gsl || q >= (int64_t)L.l * L.nx || L.jb0 == 0) return;
        i = L.ib0 + (int)(q % L.nx);
        k = (int)(q / L.nx);
        j = L.jb0 - 1;
        cell = ecell(L, i, j, k);
    }
    const uint8_t ku = knP[PL(cell, UU)], kv = knP[PL(cell, VV)];
    const bool ua = !ku, va = !kv;
    if (!ua && !va) return;                 /* land: none of the point's operands is read */
    double gu = 0.0, gv = 0.0;
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
        int pi = i + (g4 & 1), pj = j + ((g4 >> 1) & 1);
        const bool in = hnb(pi, pj, n, m, periodic);
        if (!in) { pi = i; pj = j; }
        const int64_t pc = ecell(L, pi, pj, k);
        const uint8_t kp = knP[PL(pc, PP)];
        const double p = z[PL(pc, PP)] + pbar[(int64_t)pj * n + pi];
        const double au = halo ? gsl[GSL * cell + g4] : val[(int64_t)(S_UP + g4) * ncell + lc];
        const double av = halo ? gsl[GSL * cell + 4 + g4] : val[(int64_t)(S_VP + g4) * ncell + lc];
        const bool use = in && !kp;
        gu += use ? au * p : 0.0;
        gv += use ? av * p : 0.0;
    }
    const double* D = uvinv + 4 * cell;
    const double d0 = D[0], d1 = D[1], d2 = D[2], d3 = D[3];
    const double r0 = rr[PL(cell, UU)], r1 = rr[PL(cell, VV)];
    const double ru = ua ? r0 - gu : 0.0;
    const double rv = va ? r1 - gv : 0.0;
    const double nu = d0 * ru + d1 * rv, nv = d2 * ru + d3 * rv;
    if (ua) z[PL(cell, UU)] = nu;
    if (va) z[PL(cell, VV)] = nv;
    if (halo) {
        /* the pass iterate's south halo row too (the T/S right-hand side reads its U/V) */
        if (zo && ua) zo[PL(cell, UU)] += omega * nu;
        if (zo && va) zo[PL(cell, VV)] += omega * nv;
        return;
    }
    double fu = nu, fv = nv;
    if (zo) {
        if (ua) zo[PL(cell, UU)] = fu = zo[PL(cell, UU)] + omega * nu;
        if (va) zo[PL(cell, VV)] = fv = zo[PL(cell, VV)] + omega * nv;
    }
    /* the last pass: the final U/V rows into the preconditioner output (AoS) */
    if (zaos) {
        if (ua) zaos[NUN * cell + UU] = fu;
        if (va) zaos[NUN * cell + VV] = fv;
    }
}

}  // namespace

/* does dynamics pass it (0 .. dyn_iters - 1) solve the Schur system?  schur_passes k: the first
 * k - 1 passes and the last (k = 1: the first only; 0 or >= dyn_iters: every pass).  The twin
 * at 2 degrees: every pass 203 FGMRES steps; the first and the last 203; the first two 207;
 * the first and the third 205; the first only 300 (profiles/r06_prec_study.md) */
bool gs_pass_schur(const BlockGS& gs, int it)
{
    const int k = gs.schur_passes, n = gs.dyn_iters;
    return it == 0 || k <= 0 || k >= n || (k >= 2 && (it < k - 1 || it == n - 1));
}

/* dynamics block: z(U/V/W/P) from the right-hand side rr (steps 1-5 of the header), both
 * component-planar (BlockGS::zP); zo: when given, zo += omega z on the active U/V/W/P rows
 * once z is final (the defect correction's update, fused into the pass's last kernels where
 * the column scans run); zaos: the pass's final values (zo's when given) also into the
 * preconditioner output (AoS), on the last pass */
/* rr_halo: rr's halo rows already hold the neighbours' values (the bands' defect computed
 * them itself, spmv_dyn_defect) */
/* schur = false: pbar = 0 (no Schur right-hand side reduction, no Schur solve; the passes
 * gs_pass_schur leaves out) */
int dyn_solve(iemic_ctx* c, const double* rr, double* z, double* zo, double omega, double* zaos, bool rr_halo,
              bool schur)
{
    BlockGS& gs = c->gs;
    const Lay L = lay_of(c->sub);
    hipStream_t s = c->stream;
    const bool band = c->sub.nranks > 1;
    int rc = 0;
    const int64_t ncolb = c->sub.nloc / c->l;                        /* water columns of the band */
    const int Pl = mg_lanes(c->l);                               /* l <= 64 (gs_compute) */
    /* transposed column kernels: 1024 / Pl columns of one row per workgroup of 1024 threads */
    const int cti = 1024 / Pl;
    const unsigned gct = xcd_grid(((c->sub.nx + cti - 1) / cti) * (ncolb / c->sub.nx));
    const dim3 bct(1024u);
    const int64_t ps = c->sub.next;
    /* ptil and the Schur right-hand side in one column pass (rcol), the U/V points once
     * after the Schur solve, then p and w */
    /* latitude bands: after the one exchange of rr, the pass computes ptil on both halo rows
     * and the U/V points of the south one itself (the halo-filled gslot holds their
     * couplings) instead of exchanging ptil and uv (3 -> 1 exchange batch per pass) */
    const bool hrow = band && c->sub.npx == 1;
    const double* gsl = hrow ? gs.gslot.p : nullptr;
    const unsigned gcth = hrow ? xcd_grid(((c->sub.nx + cti - 1) / cti) * (ncolb / c->sub.nx + 2)) : gct;
    if (band && !rr_halo && (rc = halo_exchange_planar(c, const_cast<double*>(rr), NUN, ps, 1))) return rc;   /* rr around the band */
    with_lanes(Pl, [&](auto p) {
        auto kp = schur ? k_gs_ptil_rcol<LANES_OF(p), true> : k_gs_ptil_rcol<LANES_OF(p), false>;
        hipLaunchKernelGGL(kp, dim3(gcth), bct, 0, s, gs.act.vp, gs.knP.p, gs.rcol.p, rr, z, gs.ocol.p,
                           gs.colv_own.p, L, gsl);
    });
    if (band && !hrow && (rc = halo_exchange_planar(c, z, NUN, ps, 1))) return rc;   /* ptil above the band */
    const double* sb = gs.colv_own.p;
    const double* pbT = schur ? gs.colvT.p : gs.colvZ.p;
    if (band && schur) {
        HIP_OK(hipMemcpyAsync(gs.colv.p, gs.colv_own.p, sizeof(double) * c->n * c->m,
                              hipMemcpyDeviceToDevice, s));
        if ((rc = allreduce_sum(c, gs.colv.p, c->n * c->m))) return rc;
        sb = gs.colv.p;
    }
    if (schur && (rc = cr_solve(c, gs.cr, sb, gs.colv2.p, s, gs.colvT.p))) return rc;
    const bool al = gs.act.act.p && gs.act.nact > 0;
    const int64_t nown = al ? gs.act.nact : c->sub.nloc;
    const unsigned gcu = blocks_for(nown + (hrow ? (int64_t)c->l * c->sub.nx : 0));
    hipLaunchKernelGGL(k_gs_uvp, dim3(gcu), dim3(256), 0, s, gs.act.vp, gs.knP.p, gs.uvinv.p,
                       rr, pbT, z, L, zo, omega, zaos, gsl, al ? gs.act.act.p : nullptr, nown);
    if (band && !hrow && (rc = halo_exchange_planar(c, z, NUN, ps, 1))) return rc;   /* uv below the band */
    with_lanes(Pl, [&](auto p) {
        hipLaunchKernelGGL(k_gs_pw_t<LANES_OF(p)>, dim3(gct), bct, 0, s, gs.act.vp, gs.knP.p,
                           pbT, z, L, rr, zo, omega, zaos);
    });
    return 0;
}

/* one minimal-residual step of the defect correction: w from the defect BlockGS::dres and
 * q = BlockGS::dq (summed over the ranks), zP += w zc, and (upd) dres += w q; zaos: as in
 * dyn_solve */
int dyn_mr_step(iemic_ctx* c, bool upd, double* zaos)
{
    BlockGS& gs = c->gs;
    const Lay L = lay_of(c->sub);
    hipStream_t s = c->stream;
    int rc;
    hipLaunchKernelGGL(k_mr_dots, dim3(MR_NB), dim3(256), 0, s, gs.dres.p, gs.dq.p, L, gs.dmr.p);
    hipLaunchKernelGGL(k_mr_sum, dim3(1), dim3(64), 0, s, gs.dmr.p, MR_NB);
    if (c->sub.nranks > 1 && (rc = allreduce_sum(c, gs.dmr.p + 2 * MR_NB, 2))) return rc;
    hipLaunchKernelGGL(k_mr_update, dim3(blocks_for(c->sub.nloc)), dim3(256), 0, s, gs.knP.p, gs.dmr.p + 2 * MR_NB,
                       gs.zc.p, gs.dq.p, gs.zP.p, gs.dres.p, L, upd ? 1 : 0, zaos);
    return 0;
}

}  // namespace iemic
