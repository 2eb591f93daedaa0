/*
 * prec_gs.hip -- block Gauss-Seidel preconditioner for the THCM Jacobian (prec = 2).
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
 */
#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <vector>

#include "gs_internal.h"

namespace iemic {

namespace {

/* ---- structure ------------------------------------------------------------------- */

/* identity rows: diagonal slot exactly 1, every other slot exactly 0 */
__global__ void k_known(const double* __restrict__ val, Lay L, int64_t rowintcon,
                        uint8_t* __restrict__ known)
{
    OWNED_CELL;
    for (int r = 0; r < NUN; r++) {
        bool id = val[(int64_t)ROW_BEGIN[r] * ncell + lc] == 1.0;
        for (int s = ROW_BEGIN[r] + 1; id && s < ROW_BEGIN[r + 1]; s++)
            id = val[(int64_t)s * ncell + lc] == 0.0;
        known[NUN * cell + r] = (id && NUN * cell + r != rowintcon) ? 1 : 0;
    }
}

/* 2x2 inverse of [[a b][c d]] restricted to the active unknowns (ia, ib) */
__device__ __forceinline__ void inv2(double a, double b, double c, double d, bool ia, bool ib,
                                     double* out)
{
    out[0] = out[1] = out[2] = out[3] = 0.0;
    if (ia && ib) {
        const double det = a * d - b * c;
        if (det != 0.0) {
            const double q = 1.0 / det;
            out[0] = d * q; out[1] = -b * q; out[2] = -c * q; out[3] = a * q;
        }
    } else if (ia) {
        if (a != 0.0) out[0] = 1.0 / a;
    } else if (ib) {
        if (d != 0.0) out[3] = 1.0 / d;
    }
}

/* per-cell factors: U/V and T/S 2x2 inverses, depth-integration weight of the P row */
__global__ void k_cell_factors(const double* __restrict__ val, const uint8_t* __restrict__ known,
                               Lay L, int64_t rowintcon, int int_sign,
                               const double* __restrict__ intc, double* __restrict__ uvinv,
                               double* __restrict__ tsinv, double* __restrict__ pw,
                               double* __restrict__ tsdiag, int64_t next)
{
    OWNED_CELL;
    auto V = [&](int s) { return val[(int64_t)s * ncell + lc]; };
    const uint8_t* kn = known + NUN * cell;
    inv2(V(S_UU0), V(S_UV0), V(S_VU0), V(S_VV0), !kn[UU], !kn[VV], uvinv + 4 * cell);
    double sdiag = V(S_SS0), sofft = V(S_ST0);
    if (NUN * cell + SS == rowintcon) {
        sdiag = int_sign * intc[NUN * cell + SS];
        sofft = 0.0;
    }
    inv2(V(S_TT0), V(S_TS0), sofft, sdiag, !kn[TT], !kn[SS], tsinv + 4 * cell);
    {
        /* the 2x2 T/S block the sweeps invert, restricted to the active unknowns */
        const bool ta = !kn[TT], sa = !kn[SS];
        tsdiag[cell] = ta ? V(S_TT0) : 0.0;
        tsdiag[next + cell] = ta && sa ? V(S_TS0) : 0.0;
        tsdiag[2 * next + cell] = ta && sa ? sofft : 0.0;
        tsdiag[3 * next + cell] = sa ? sdiag : 0.0;
    }
    /* depth integral of the continuity rows: weight 1/a_k with a_k the coefficient of
     * the row's own W (or -1/b_k with b_k that of W(k-1) when the own W is an identity) */
    double w = 0.0;
    if (!kn[PP]) {
        const int64_t nm = L.nx;                /* k - 1 is one row of nx cells back */
        const bool w_own = !kn[WW];
        const bool w_below = k > 0 && !known[NUN * (cell - nm) + WW];
        if (w_own && V(S_PW0) != 0.0) w = 1.0 / V(S_PW0);
        else if (w_below && V(S_PWM) != 0.0) w = -1.0 / V(S_PWM);
        else w = 1.0;
    }
    pw[cell] = w;
}

/* Schur entry S[c][c'] for c' = column (i+di, j+dj): S9[c*9 + (dj+1)*3 + (di+1)], c = i*m + j.
 * Only the rows of this band's columns are built (the bands' rows are summed over the
 * ranks afterwards); corner U/V points one latitude row below the band are read from the
 * halo-filled per-cell arrays (known, uvinv, gslot). */
__global__ void k_schur_build(const double* __restrict__ val, const uint8_t* __restrict__ known,
                              const double* __restrict__ uvinv, const double* __restrict__ gslot,
                              const double* __restrict__ pw, const int* __restrict__ col_of_ij,
                              const uint8_t* __restrict__ pinned, Lay L, int jb1,
                              double* __restrict__ S9)
{
    LAY_ALIASES;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)L.nx * (jb1 - L.jb0) * 9) return;
    const int q = (int)(t / 9), o = (int)(t % 9);
    const int di = o % 3 - 1, dj = o / 3 - 1;
    const int i = L.ib0 + q % L.nx, j = L.jb0 + q / L.nx;
    const int c = col_of_ij[j * n + i];
    if (c < 0) return;
    double* row = S9 + (int64_t)c * 9;
    if (pinned[c]) {
        if (o == 4) row[4] = 1.0;
        return;
    }
    int ti = i + di, tj = j + dj;
    if (!hnb(ti, tj, n, m, periodic)) return;
    const int c2 = col_of_ij[tj * n + ti];
    if (c2 < 0 || pinned[c2]) return;
    const int64_t ncell = L.nloc;
    double s = 0.0;
    for (int k = 0; k < l; k++) {
        const int64_t pc = ecell(L, i, j, k);
        if (known[NUN * pc + PP]) continue;
        const int64_t tc = ecell(L, ti, tj, k);
        if (known[NUN * tc + PP]) continue;
        double acc = 0.0;
        /* corners q = (i+a, j+b), a,b in {0,-1}; P row slot index q4 = (0,0),(-1,0),(0,-1),(-1,-1) */
        for (int q4 = 0; q4 < 4; q4++) {
            const int a = -(q4 & 1), b = -((q4 >> 1) & 1);
            const int e = di - a, f = dj - b;
            if (e < 0 || e > 1 || f < 0 || f > 1) continue;
            int qi = i + a, qj = j + b;
            if (!hnb(qi, qj, n, m, periodic)) continue;
            const int64_t qc = ecell(L, qi, qj, k);
            const bool ua = !known[NUN * qc + UU], va = !known[NUN * qc + VV];
            if (!ua && !va) continue;
            const double du = ua ? val[(int64_t)(S_PU + q4) * ncell + (pc - L.own0)] : 0.0;
            const double dv = va ? val[(int64_t)(S_PV + q4) * ncell + (pc - L.own0)] : 0.0;
            const double* Di = uvinv + 4 * qc;
            const double yu = du * Di[0] + dv * Di[2];
            const double yv = du * Di[1] + dv * Di[3];
            const int g4 = e + 2 * f;                      /* (0,0),(1,0),(0,1),(1,1) */
            const double gu = ua ? gslot[GSL * qc + g4] : 0.0;
            const double gv = va ? gslot[GSL * qc + 4 + g4] : 0.0;
            acc += yu * gu + yv * gv;
        }
        s += pw[pc] * acc;
    }
    row[o] = s;
}

/* per owned cell: the U and V rows' couplings to the 4 P corners (slots 20..23, 42..45)
 * and the W row's to P(k), P(k+1) (slots 47, 48) */
__global__ void k_gslot_pack(const double* __restrict__ val, Lay L, double* __restrict__ gslot)
{
    OWNED_CELL;
    for (int g = 0; g < 4; g++) {
        gslot[GSL * cell + g] = val[(int64_t)(S_UP + g) * ncell + lc];
        gslot[GSL * cell + 4 + g] = val[(int64_t)(S_VP + g) * ncell + lc];
    }
    gslot[GSL * cell + 8] = val[(int64_t)S_WP0 * ncell + lc];
    gslot[GSL * cell + 9] = val[(int64_t)S_WP1 * ncell + lc];
}

/* identity-row flags <-> doubles (for the halo exchange of the flags) */
__global__ void k_u8_to_d(const uint8_t* __restrict__ a, double* __restrict__ b, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        b[q] = a[q];
}
__global__ void k_d_to_u8(const double* __restrict__ b, uint8_t* __restrict__ a, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        a[q] = b[q] != 0.0 ? 1 : 0;
}

/* ---- apply ------------------------------------------------------------------------ */

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

/* per owned water column (i, j): 1 in flags[j n + i] if a P row of it is active, 1 in
 * flags[n m + j n + i] if a U or V row is (the host's Schur structure input; band_flags did
 * this on a host copy of all the flags) */
__global__ void k_band_flags(const uint8_t* __restrict__ known, Lay L, double* __restrict__ flags)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ncol = L.nloc / L.l;
    if (t >= ncol) return;
    const int il = (int)(t % L.nx), jl = (int)(t / L.nx);
    bool p = false, uv = false;
    for (int k = 0; k < L.l; k++) {
        const int64_t cell = L.own0 + ((int64_t)jl * L.l + k) * L.nx + il;
        p |= !known[NUN * cell + PP];
        uv |= !known[NUN * cell + UU] || !known[NUN * cell + VV];
    }
    const int64_t q = (int64_t)(L.jb0 + jl) * L.n + L.ib0 + il;
    if (p) flags[q] = 1.0;
    if (uv) flags[(int64_t)L.n * L.m + q] = 1.0;
}

/* the identity-row flags in the planar layout */
__global__ void k_known_planar(const uint8_t* __restrict__ known, uint8_t* __restrict__ knP, int64_t next)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= next) return;
#pragma unroll
    for (int R = 0; R < NUN; R++) knP[e + R * next] = known[NUN * e + R];
}

/* per cell: bitmask of the slots (104 bits) through which an active row couples to an
 * identity-row column (coast, sea floor, rigid lid); empty for most interior cells */
__global__ void k_knownmask(const double* __restrict__ val, const uint8_t* __restrict__ known,
                            uint64_t* __restrict__ kmask, Lay L, int jb1)
{
    LAY_ALIASES;
    OWNED_CELL;
    uint64_t b0 = 0, b1 = 0;
    int R = 0;
    for (int s = 0; s < NSLOT; s++) {
        while (s >= ROW_BEGIN[R + 1]) R++;
        if (known[NUN * cell + R] || val[(int64_t)s * ncell + lc] == 0.0) continue;
        int ii = i + SLOTS[s].di, jj = j + SLOTS[s].dj;
        const int kk = k + SLOTS[s].dk;
        if (kk < 0 || kk >= l || !hnb(ii, jj, n, m, periodic)) continue;
        if (jj < L.jb0 - 1 || jj > jb1) continue;   /* beyond the exchanged halo row */
        if (known[NUN * ecell(L, ii, jj, kk) + SLOTS[s].var]) {
            if (s < 64) b0 |= (uint64_t)1 << s;
            else b1 |= (uint64_t)1 << (s - 64);
        }
    }
    kmask[2 * cell] = b0;
    kmask[2 * cell + 1] = b1;
}

/* T/S off-diagonal couplings of active rows to active T/S columns, compacted:
 * per row (T, S) 6 same-variable neighbours (-i,+i,-j,+j,-k,+k) + the other variable at
 * k-1, k+1; zero where the column is an identity row, outside, or the row is inactive. */
constexpr int TS_NC = 16;
__global__ void k_ts_compact(const double* __restrict__ val, const uint8_t* __restrict__ known,
                             double* __restrict__ tsoff, Lay L, int64_t next, int64_t rowintcon)
{
    LAY_ALIASES;
    OWNED_CELL;
    for (int R = TT; R <= SS; R++) {
        const int base = ROW_BEGIN[R];
        const int other = R == TT ? SS : TT;
        const bool act = !known[NUN * cell + R] && NUN * cell + R != rowintcon;
        /* slots base+1..base+6: same var (-i,+i,-j,+j,-k,+k); base+18, base+19: other var k-1, k+1 */
        const int sl[8] = {base + 1, base + 2, base + 3, base + 4, base + 5, base + 6, base + 18, base + 19};
        for (int q = 0; q < 8; q++) {
            double v = 0.0;
            if (act) {
                const int s = sl[q];
                int ii = i + SLOTS[s].di, jj = j + SLOTS[s].dj;
                const int kk = k + SLOTS[s].dk;
                if (kk >= 0 && kk < l && hnb(ii, jj, n, m, periodic) &&
                    !known[NUN * ecell(L, ii, jj, kk) + (q < 6 ? R : other)])
                    v = val[(int64_t)s * ncell + lc];
            }
            tsoff[(int64_t)((R - TT) * 8 + q) * next + cell] = v;
        }
    }
}

__device__ __forceinline__ double duv_uv(const double* __restrict__ val, const uint8_t* __restrict__ knP,
                                         const double* __restrict__ z, int i, int j, int k,
                                         int64_t pl, const Lay& L);
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
/* logical workgroup of block b for nwg workgroups launched as xcd_grid(nwg) blocks: the
 * XCDs (blocks dealt round robin, b % 8) get contiguous runs of workgroups, so tiles of
 * neighbouring latitude rows, which read each other's rows, share an L2; -1: idle block */
__device__ __forceinline__ int xcd_block(int nwg)
{
    const int per = (nwg + 7) >> 3;
    const int w = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    return w < nwg ? w : -1;
}

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

/* ---- the Schur right-hand side as a linear form in rr ----------------------------------
 * Steps 1-3a (ptil, uv*, the depth-weighted continuity defect) are linear in rr, so the
 * Schur right-hand side of water column (i, j) is a fixed combination of rr over its
 * neighbourhood: W rows of the 3 x 3 columns around it (through ptil, which the U/V points
 * of its four corners read), U/V rows of those corners, its own P rows.  The coefficients
 * are formed at set-up (k_rcol_uvp, k_rcol_w), so the apply evaluates ptil and the
 * right-hand side in one column kernel (k_gs_ptil_rcol) and the U/V points only once, after
 * the Schur solve (k_gs_uvp): two launches fewer per dynamics pass.
 * Layout: rcol[(e * l + k) * ncolb + t], t = band column (j - jb0) * nx + (i - ib0);
 * e < 9: rr_W at column (i + e % 3 - 1, j + e / 3 - 1), level k; e = 9 + q4 / 13 + q4: rr_U
 * / rr_V at corner q4 = (i - (q4 & 1), j - (q4 >> 1)); e = 17: rr_P at (i, j, k). */
constexpr int RC_NE = 18;

/* U/V and P coefficients, thread per (band column, level): with w_k the depth weight,
 * a the P row's couplings to its corners and D the corner's 2x2 U/V inverse, the column's
 * entry sum_k w_k (Duv uv* - rr_p) has d/d rr_U(q) = [ua] (cu d0 + cv d2), d/d rr_V(q) =
 * [va] (cu d1 + cv d3), cu = w_k a_U [in, ua], cv = w_k a_V [in, va]; d/d rr_P = -w_k. */
__global__ void k_rcol_uvp(const double* __restrict__ val, const uint8_t* __restrict__ known,
                           const double* __restrict__ uvinv, const double* __restrict__ pw,
                           double* __restrict__ rcol, Lay L)
{
    LAY_ALIASES;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int ncolb = (int)(L.nloc / l);
    if (g >= (int64_t)ncolb * l) return;
    const int t = (int)(g / l), k = (int)(g % l);
    const int i = L.ib0 + t % L.nx, j = L.jb0 + t / L.nx;
    const int64_t cell = ecell(L, i, j, k), pl = cell - L.own0, ncell = L.nloc;
    const bool pa = !known[NUN * cell + PP];
    const double w = pa ? pw[cell] : 0.0;
    /* coefficient e of level k: R[e * l * ncolb] */
    double* R = rcol + (int64_t)k * ncolb + t;
    const int64_t es = (int64_t)l * ncolb;
    for (int q4 = 0; q4 < 4; q4++) {
        int qi = i - (q4 & 1), qj = j - ((q4 >> 1) & 1);
        double cu_r = 0.0, cv_r = 0.0;
        if (pa && hnb(qi, qj, n, m, periodic)) {
            const int64_t qc = ecell(L, qi, qj, k);
            const bool ua = !known[NUN * qc + UU], va = !known[NUN * qc + VV];
            const double cu = ua ? w * val[(int64_t)(S_PU + q4) * ncell + pl] : 0.0;
            const double cv = va ? w * val[(int64_t)(S_PV + q4) * ncell + pl] : 0.0;
            const double* D = uvinv + 4 * qc;
            cu_r = ua ? cu * D[0] + cv * D[2] : 0.0;
            cv_r = va ? cu * D[1] + cv * D[3] : 0.0;
        }
        R[(9 + q4) * es] = cu_r;
        R[(13 + q4) * es] = cv_r;
    }
    R[17 * es] = pa ? -w : 0.0;
}

/* W coefficients, thread per (band column, neighbour column c'): with D_k the entry's
 * derivative in ptil(c', k) (through every corner U/V point of the column that reads
 * P(c', k)), and ptil(c', k) = A_k + B_k ptil(c', k+1), A_k = rr_W / g0, B_k = -g1 / g0 on
 * the active hydrostatic rows (0, 0 elsewhere), the coefficient of rr_W(c', k') is
 * S_k' / g0_k' with S_k' = S_k'-1 B_k'-1 + D_k'.  Reads the U/V coefficients of k_rcol_uvp. */
__global__ void k_rcol_w(const uint8_t* __restrict__ known, const double* __restrict__ gslot,
                         double* __restrict__ rcol, Lay L)
{
    LAY_ALIASES;
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int ncolb = (int)(L.nloc / l);
    if (g >= (int64_t)ncolb * 9) return;
    const int t = (int)(g / 9), e = (int)(g % 9);
    const int i = L.ib0 + t % L.nx, j = L.jb0 + t / L.nx;
    const int di = e % 3 - 1, dj = e / 3 - 1;
    /* coefficient e of level k: R[(e * l + k) * ncolb] */
    double* R = rcol + t;
    const int64_t ks = ncolb;
    int gi = i + di, gj = j + dj;
    if (!hnb(gi, gj, n, m, periodic)) {
        for (int k = 0; k < l; k++) R[((int64_t)e * l + k) * ks] = 0.0;
        return;
    }
    double S = 0.0, Bprev = 0.0;
    for (int k = 0; k < l; k++) {
        const int64_t gc = ecell(L, gi, gj, k);
        const bool pa = !known[NUN * gc + PP], wa = !known[NUN * gc + WW];
        double D = 0.0;
        if (pa) {
            for (int q4 = 0; q4 < 4; q4++) {
                const int a = -(q4 & 1), b = -((q4 >> 1) & 1);
                const int ex = di - a, fy = dj - b;          /* c' as a P corner of q */
                if (ex < 0 || ex > 1 || fy < 0 || fy > 1) continue;
                int qi = i + a, qj = j + b;
                if (!hnb(qi, qj, n, m, periodic)) continue;
                const int64_t qc = ecell(L, qi, qj, k);
                const int g4 = ex + 2 * fy;
                D -= R[((int64_t)(9 + q4) * l + k) * ks] * gslot[GSL * qc + g4] +
                     R[((int64_t)(13 + q4) * l + k) * ks] * gslot[GSL * qc + 4 + g4];
            }
        }
        const double g0 = gslot[GSL * gc + 8], g1 = gslot[GSL * gc + 9];
        const bool act = pa && k < l - 1 && wa && g0 != 0.0;
        S = S * Bprev + D;
        R[((int64_t)e * l + k) * ks] = act ? S / g0 : 0.0;
        Bprev = act ? -g1 / g0 : 0.0;
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
constexpr int MR_NB = 256;
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

/* 6a. T/S right-hand side: rr_ts - B_ts,(u,v,w) z;  z_ts = 0 */
__global__ void k_gs_bts(const double* __restrict__ val, const uint8_t* __restrict__ known,
                         const double* __restrict__ rr, double* __restrict__ z, double* __restrict__ bts,
                         Lay L)
{
    LAY_ALIASES;
    OWNED_CELL;
    for (int R = TT; R <= SS; R++) {
        const int64_t row = NUN * cell + R;
        if (known[row]) continue;
        double acc = rr[row];
        for (int s = ROW_BEGIN[R]; s < ROW_BEGIN[R + 1]; s++) {
            const int var = SLOTS[s].var;
            if (var == TT || var == SS) continue;
            const double v = val[(int64_t)s * ncell + lc];
            if (v == 0.0) continue;
            int ii = i + SLOTS[s].di, jj = j + SLOTS[s].dj;
            const int kk = k + SLOTS[s].dk;
            if (kk < 0 || kk >= l || !hnb(ii, jj, n, m, periodic)) continue;
            const int64_t col = NUN * ecell(L, ii, jj, kk) + var;
            if (!known[col]) acc -= v * z[col];
        }
        bts[row] = acc;
        z[row] = 0.0;
    }
}

/* colour of a cell for the T/S sweeps: parity of i+j+k (global j); on a periodic grid with
 * odd n the wrap pairs (n-1, 0) would share a colour, so column i = n-1 gets colours 2/3 */
__device__ __forceinline__ int ts_color(int i, int j, int k, int n, int periodic)
{
    if (periodic && (n & 1) && i == n - 1) return 2 + ((j + k) & 1);
    return (i + j + k) & 1;
}

/* 6b. one red-black half sweep on the T/S block with 2x2 cell blocks (compact couplings;
 * generic layout, used for odd n) */
__global__ void __launch_bounds__(256) k_gs_ts_half(const double* __restrict__ tsoff,
                                                    const uint8_t* __restrict__ known,
                                                    const double* __restrict__ tsinv,
                                                    const double* __restrict__ bts,
                                                    double* __restrict__ z, Lay L, int64_t next,
                                                    int color)
{
    LAY_ALIASES;
    OWNED_CELL;
    if (ts_color(i, j, k, n, periodic) != color) return;
    const bool ta = !known[NUN * cell + TT], sa = !known[NUN * cell + SS];
    if (!ta && !sa) return;
    /* neighbour cells (clamped where the coupling is zero anyway) */
    int im = i - 1, ip = i + 1;
    if (periodic) { if (im < 0) im = n - 1; if (ip >= n) ip = 0; }
    else { if (im < 0) im = i; if (ip >= n) ip = i; }
    const int jm = j > 0 ? j - 1 : j, jp = j < m - 1 ? j + 1 : j;
    const int km = k > 0 ? k - 1 : k, kp = k < l - 1 ? k + 1 : k;
    const int64_t nb[6] = {ecell(L, im, j, k), ecell(L, ip, j, k), ecell(L, i, jm, k),
                           ecell(L, i, jp, k), ecell(L, i, j, km), ecell(L, i, j, kp)};
    double res[2];
#pragma unroll
    for (int R = 0; R < 2; R++) {
        const int var = TT + R, oth = SS - R;
        const double* a = tsoff + (int64_t)(R * 8) * next + cell;
        double acc = bts[NUN * cell + var];
#pragma unroll
        for (int q = 0; q < 6; q++) acc -= a[(int64_t)q * next] * z[NUN * nb[q] + var];
        acc -= a[(int64_t)6 * next] * z[NUN * nb[4] + oth];
        acc -= a[(int64_t)7 * next] * z[NUN * nb[5] + oth];
        res[R] = acc;
    }
    const double* D = tsinv + 4 * cell;
    if (ta) z[NUN * cell + TT] = D[0] * res[0] + D[1] * res[1];
    if (sa) z[NUN * cell + SS] = D[2] * res[0] + D[3] * res[1];
}

/* Even n: the owned cells of one colour are lc = 2q + ((j+k+c)&1) (lc = (row)*n + i with
 * row = (j-jb0)*l + k), so every per-cell T/S array can be stored per colour and read
 * contiguously by a half sweep:  tsc[(c*16 + e)*half + q] couplings,
 * tic[(c*4 + e)*half + q] 2x2 inverses, bc[(c*2 + v)*half + q] right-hand sides;
 * zt / zs: T and S iterates by ext cell (halo entries stay 0). */
__global__ void k_ts_pack(const double* __restrict__ tsoff, const double* __restrict__ tsinv,
                          double* __restrict__ tsc, double* __restrict__ tic, Lay L, int64_t next)
{
    OWNED_CELL;
    const int64_t half = ncell / 2;
    const int c = (i + j + k) & 1;
    const int64_t q = lc >> 1;
    for (int e = 0; e < TS_NC; e++) tsc[(int64_t)(c * TS_NC + e) * half + q] = tsoff[(int64_t)e * next + cell];
    for (int e = 0; e < 4; e++) tic[(int64_t)(c * 4 + e) * half + q] = tsinv[4 * cell + e];
}

/* T/S right-hand side bts = rr_TS - A_TS,D z_D into the colour layout and bts; zt = zs = 0.
 * One wave per (64 cells, T or S row): the row's 10 dynamics slots unrolled at compile
 * time, neighbour indices clamped as in the SpMV (the ELL holds zeros outside the domain),
 * identity-row columns (their couplings are in rr already) skipped by the slot bitmask
 * kmask instead of a byte gather per slot.  Dealt to the XCDs in contiguous runs. */
__global__ void __launch_bounds__(128) k_gs_bts2(const double* __restrict__ val, const uint8_t* __restrict__ known,
                                                 const uint64_t* __restrict__ kmask,
                                                 const double* __restrict__ rr, const double* __restrict__ z,
                                                 double* __restrict__ bc, double* __restrict__ zt,
                                                 double* __restrict__ zs, Lay L, double* __restrict__ bts,
                                                 int nblk)
{
    LAY_ALIASES;
    const int per = (nblk + 7) >> 3;
    const int tile = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (tile >= nblk) return;
    const int64_t lc = (int64_t)tile * 64 + (threadIdx.x & 63);
    if (lc >= L.nloc) return;
    const int R = TT + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int i, j, k;
    lc_ijk(L, lc, i, j, k);
    const int64_t cell = L.own0 + lc;
    int nc[3][9];
    nb_cells(sub_of(L), i - L.ib0, j, k, nc);
    const int64_t row = NUN * cell + R;
    double acc = 0.0;
    if (!known[row]) {
        const uint64_t kb = kmask[2 * cell + 1];
        acc = R == TT ? bts_row<TT>(val, z, lc, L.nloc, nc, kb, rr[row])
                      : bts_row<SS>(val, z, lc, L.nloc, nc, kb, rr[row]);
    }
    const int64_t half = L.nloc / 2;
    const int c = (i + j + k) & 1;
    bc[(int64_t)(c * 2 + (R - TT)) * half + (lc >> 1)] = acc;
    bts[row] = acc;
    if (R == TT) zt[cell] = 0.0;
    else zs[cell] = 0.0;
}

__global__ void __launch_bounds__(256) k_gs_ts_half_c(const double* __restrict__ tsc,
                                                      const double* __restrict__ tic,
                                                      const double* __restrict__ bc,
                                                      double* __restrict__ zt, double* __restrict__ zs,
                                                      Lay L, int c)
{
    LAY_ALIASES;
    const int64_t half = L.nloc / 2;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= half) return;
    const int nx = L.nx;
    const int64_t row = (2 * q) / nx;                /* (j - jb0) * l + k */
    const int k = (int)(row % l), j = L.jb0 + (int)(row / l);
    const int64_t lc = 2 * q + ((j + k + c) & 1);    /* ib0 even: local parity = global */
    const int il = (int)(lc - row * nx);
    const int64_t cell = L.own0 + lc;
    const int64_t r = row + (int64_t)HALO * l;
    const int64_t ln = (int64_t)l * nx;
    const int64_t nb[6] = {xnb_cell(r, il - 1, n, L.ib0, nx, L.hx, periodic, L.xb),
                           xnb_cell(r, il + 1, n, L.ib0, nx, L.hx, periodic, L.xb),
                           j > 0 ? cell - ln : cell, j < m - 1 ? cell + ln : cell,
                           k > 0 ? cell - nx : cell, k < l - 1 ? cell + nx : cell};
    const double* a = tsc + (int64_t)(c * TS_NC) * half + q;
    double rt = bc[(int64_t)(c * 2) * half + q], rs = bc[(int64_t)(c * 2 + 1) * half + q];
#pragma unroll
    for (int e = 0; e < 6; e++) {
        rt -= a[(int64_t)e * half] * zt[nb[e]];
        rs -= a[(int64_t)(8 + e) * half] * zs[nb[e]];
    }
    rt -= a[(int64_t)6 * half] * zs[nb[4]] + a[(int64_t)7 * half] * zs[nb[5]];
    rs -= a[(int64_t)14 * half] * zt[nb[4]] + a[(int64_t)15 * half] * zt[nb[5]];
    const double* D = tic + (int64_t)(c * 4) * half + q;
    zt[cell] = D[0] * rt + D[half] * rs;
    zs[cell] = D[2 * half] * rt + D[3 * half] * rs;
}

/* z(T,S) = zt, zs on the active rows */
__global__ void k_ts_scatter(const uint8_t* __restrict__ known, const double* __restrict__ zt,
                             const double* __restrict__ zs, double* __restrict__ z, Lay L)
{
    OWNED_CELL;
    if (!known[NUN * cell + TT]) z[NUN * cell + TT] = zt[cell];
    if (!known[NUN * cell + SS]) z[NUN * cell + SS] = zs[cell];
}

/* ---- host: structure from the identity-row pattern ------------------------------ */

/* flags[j*n+i] = 1 for an active water column (any active P), flags[n*m + j*n+i] = 1
 * for an active U/V point, over the band's latitude rows */
/* Schur structure of the whole grid from the global flags (identical on every rank) */
int build_structure(iemic_ctx* c, const std::vector<double>& flags)
{
    BlockGS& gs = c->gs;
    const int n = c->n, m = c->m;
    const int periodic = c->cfg.periodic;
    std::vector<int> colid((size_t)n * m, -1);
    std::vector<uint8_t> act((size_t)n * m, 0), uva((size_t)n * m, 0);
    for (size_t q = 0; q < (size_t)n * m; q++) {
        act[q] = flags[q] != 0.0;
        uva[q] = flags[(size_t)n * m + q] != 0.0;
    }
    auto wrap = [&](int& i, int& j) {
        if (j < 0 || j >= m) return false;
        if (i < 0 || i >= n) {
            if (!periodic) return false;
            i = (i + n) % n;
        }
        return true;
    };
    /* band ordering: i folded (periodic: 0, n-1, 1, n-2, ...), j fastest */
    std::vector<int> ipos(n);
    if (periodic) {
        int a = 0, b = n - 1, q = 0;
        while (a <= b) {
            ipos[a] = q++;
            if (a != b) ipos[b] = q++;
            a++; b--;
        }
    } else {
        for (int i = 0; i < n; i++) ipos[i] = i;
    }
    std::vector<std::pair<int64_t, int>> ord;
    for (int j = 0; j < m; j++)
        for (int i = 0; i < n; i++)
            if (act[(size_t)j * n + i]) ord.push_back({(int64_t)ipos[i] * m + j, j * n + i});
    std::sort(ord.begin(), ord.end());
    const int ncol = (int)ord.size();
    /* Schur index of column (i, j): c = i*m + j (the cyclic reduction's block order); the
     * band order above only fixes which column of a null-space set is pinned (its first),
     * the same choice as the CPU twin */
    const int NC = n * m;
    std::vector<int> ij_of_col(NC);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < m; j++) ij_of_col[(size_t)i * m + j] = j * n + i;
    for (int q = 0; q < ncol; q++) {
        const int ij = ord[q].second;
        colid[ij] = (ij % n) * m + ij / n;
    }
    /* couplings: columns sharing an active U/V corner */
    std::vector<std::vector<int>> adj(NC);
    for (int q = 0; q < ncol; q++) {
        const int ij0 = ord[q].second;
        const int i = ij0 % n, j = ij0 / n, cq = colid[ij0];
        for (int dj = -1; dj <= 1; dj++)
            for (int di = -1; di <= 1; di++) {
                int ti = i + di, tj = j + dj;
                if (!wrap(ti, tj)) continue;
                const int q2 = colid[(size_t)tj * n + ti];
                if (q2 < 0 || q2 == cq) continue;
                bool shared = false;
                for (int a = -1; a <= 0 && !shared; a++)
                    for (int b = -1; b <= 0 && !shared; b++) {
                        /* corner (i+a, j+b) must also be a corner of (ti,tj): e = di-a in {0,1} */
                        const int e = di - a, f = dj - b;
                        if (e < 0 || e > 1 || f < 0 || f > 1) continue;
                        int qi = i + a, qj = j + b;
                        if (!wrap(qi, qj)) continue;
                        if (uva[(size_t)qj * n + qi]) shared = true;
                    }
                if (shared) adj[cq].push_back(q2);
            }
    }
    /* null space of the B-grid pressure Schur: constant on each connected set of
     * same-colour columns linked diagonally through an active U/V corner (checkerboard
     * modes, local ones around islands and straits included) -> one pin per set */
    std::vector<uint8_t> pin(NC, 0);
    std::vector<int> comp(NC, -1);
    for (int q = 0; q < ncol; q++) {
        const int s0 = colid[ord[q].second];       /* band order: first column of its set */
        if (comp[s0] >= 0) continue;
        std::vector<int> stack{s0};
        comp[s0] = s0;
        pin[s0] = 1;
        while (!stack.empty()) {
            const int cq = stack.back();
            stack.pop_back();
            for (int q2 : adj[cq]) {
                int di = q2 / m - cq / m;
                const int dj = q2 % m - cq % m;
                if (di > 1) di -= n;
                if (di < -1) di += n;
                if (di == 0 || dj == 0) continue; /* other colour */
                if (comp[q2] < 0) { comp[q2] = s0; stack.push_back(q2); }
            }
        }
    }
    std::vector<int> own(NC, -1), ocol((size_t)n * m, -1);
    for (int q = 0; q < ncol; q++) {
        const int ij = ord[q].second;
        if (c->su.owns(ij % n, ij / n)) {
            own[colid[ij]] = colid[ij];
            ocol[ij] = pin[colid[ij]] ? -2 - colid[ij] : colid[ij];
        }
    }
    int rc = 0;
    rc |= gs.col_of_ij.alloc((size_t)n * m);
    rc |= gs.ij_of_col.alloc(NC);
    rc |= gs.pinned.alloc(NC);
    rc |= gs.S9.alloc((size_t)9 * NC);
    rc |= gs.colv2.alloc(NC);
    rc |= gs.colvT.alloc(NC);
    rc |= gs.colvZ.alloc(NC);
    rc |= gs.colv_own.alloc(NC);
    rc |= gs.colv.alloc(NC);
    rc |= gs.own_pos.alloc(NC);
    rc |= gs.ocol.alloc((size_t)n * m);
    if (rc) {
        set_error("block GS: out of device memory");
        return IEMIC_ENOMEM;
    }
    if ((rc = h2d(c, gs.col_of_ij.p, colid.data(), sizeof(int) * colid.size()))) return rc;
    if ((rc = h2d(c, gs.ij_of_col.p, ij_of_col.data(), sizeof(int) * NC))) return rc;
    HIP_OK(hipMemsetAsync(gs.colvZ.p, 0, sizeof(double) * NC, c->stream));
    if ((rc = h2d(c, gs.pinned.p, pin.data(), NC))) return rc;
    if ((rc = h2d(c, gs.own_pos.p, own.data(), sizeof(int) * NC))) return rc;
    if ((rc = h2d(c, gs.ocol.p, ocol.data(), sizeof(int) * ocol.size()))) return rc;
    /* entries of inactive and foreign columns stay 0 (the rhs of the reduced solve) */
    HIP_OK(hipMemsetAsync(gs.colv_own.p, 0, sizeof(double) * NC, c->stream));
    HIP_OK(hipMemsetAsync(gs.colv2.p, 0, sizeof(double) * NC, c->stream));
    if ((rc = cr_init(c, gs.cr, n, m, periodic))) return rc;
    gs.flags_h = flags;
    return 0;
}

}  // namespace

/* colour-compacted T/S sweeps: the owned cells of one colour are every other cell of a
 * row (even n, nx and ib0) */
static bool ts_compact(const iemic_ctx* c) { return (c->n & 1) == 0 && (c->sub.nx & 1) == 0 && (c->sub.ib0 & 1) == 0; }

/* the T/S block solve: right-hand side rr_TS - A_TS,D z_D from the dynamics iterate zd (the
 * planar zP for the multigrid, the AoS output for the sweeps), then ts_mg V-cycles
 * (ts_mg.hip: out, side) or ts_sweeps symmetric red-black sweeps, result into z(T, S) of the
 * output z */
static int ts_solve(iemic_ctx* c, const double* zd, double* z, bool out, bool side = false)
{
    BlockGS& gs = c->gs;
    if (gs.ts_mg > 0) return ts_mg_solve(c, zd, z, out, side);
    const Lay L = lay_of(c->sub);
    const int n = c->n;
    hipStream_t s = c->stream;
    const unsigned gc = (unsigned)((c->sub.nloc + 255) / 256);
    const int nsw = std::max(1, gs.ts_sweeps);
    if (ts_compact(c)) {
        /* colour-compacted symmetric red-black sweeps */
        const int nblk = (int)((c->sub.nloc + 63) / 64);
        hipLaunchKernelGGL(k_gs_bts2, dim3(8u * (unsigned)((nblk + 7) / 8)), dim3(128), 0, s, gs.act.vp,
                           gs.known.p, gs.kmask.p, gs.rr.p, z, gs.sw.bc.p, gs.sw.zt.p, gs.sw.zs.p, L, gs.sw.bts.p, nblk);
        const unsigned gh = (unsigned)((c->sub.nloc / 2 + 255) / 256);
        const int seq[4] = {0, 1, 1, 0};
        for (int sw = 0; sw < nsw; sw++)
            for (int h = 0; h < 4; h++)
                hipLaunchKernelGGL(k_gs_ts_half_c, dim3(gh), dim3(256), 0, s, gs.sw.tsc.p, gs.sw.tic.p, gs.sw.bc.p,
                                   gs.sw.zt.p, gs.sw.zs.p, L, seq[h]);
        hipLaunchKernelGGL(k_ts_scatter, dim3(gc), dim3(256), 0, s, gs.known.p, gs.sw.zt.p, gs.sw.zs.p, z, L);
    } else {
        /* symmetric sweeps: colours forward then backward */
        hipLaunchKernelGGL(k_gs_bts, dim3(gc), dim3(256), 0, s, gs.act.vp, gs.known.p, gs.rr.p, z,
                           gs.sw.bts.p, L);
        const bool four = c->cfg.periodic && (n & 1);
        const int seq2[4] = {0, 1, 1, 0}, seq4[8] = {0, 1, 2, 3, 3, 2, 1, 0};
        const int* seq = four ? seq4 : seq2;
        const int ns = four ? 8 : 4;
        for (int sw = 0; sw < nsw; sw++)
            for (int h = 0; h < ns; h++)
                hipLaunchKernelGGL(k_gs_ts_half, dim3(gc), dim3(256), 0, s, gs.sw.tsoff.p, gs.known.p,
                                   gs.sw.tsinv.p, gs.sw.bts.p, z, L, c->sub.next, seq[h]);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

/* ---- set-up: the steps of gs_compute, in its order ---------------------------------- */

/* per-cell arrays span the ext layout; the halo entries stay 0 (and the halo rows are
 * identity rows), which is what makes the bands block-Jacobi coupled */
static int gs_reserve_cells(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    const int64_t NE = c->sub.nerows(), next = c->sub.next;
    if (gs.known.n >= (size_t)NE) return 0;
    int rc = 0;
    rc |= gs.known.alloc(NE);
    rc |= gs.uvinv.alloc((size_t)4 * next);
    rc |= gs.sw.tsinv.alloc((size_t)4 * next);
    rc |= gs.pw.alloc(next);
    rc |= gs.rr.alloc(NE);
    rc |= gs.sw.bts.alloc(NE);
    rc |= gs.kmask.alloc((size_t)2 * next);
    rc |= gs.sw.tsoff.alloc((size_t)TS_NC * next);
    rc |= gs.sw.tsc.alloc((size_t)TS_NC * c->sub.nloc);
    rc |= gs.sw.tic.alloc((size_t)4 * c->sub.nloc);
    rc |= gs.sw.bc.alloc((size_t)2 * c->sub.nloc);
    rc |= gs.sw.zt.alloc(next);
    rc |= gs.sw.zs.alloc(next);
    rc |= gs.tsdiag.alloc((size_t)4 * next);
    rc |= gs.knP.alloc(NE);
    rc |= gs.zP.alloc(NE);
    rc |= gs.rrP.alloc(NE);
    if (rc) {
        set_error("block GS: out of device memory");
        return IEMIC_ENOMEM;
    }
    for (DevBuf<double>* bptr : {&gs.uvinv, &gs.sw.tsinv, &gs.pw, &gs.rr, &gs.sw.bts, &gs.sw.tsoff, &gs.sw.zt,
                                 &gs.sw.zs, &gs.tsdiag, &gs.zP, &gs.rrP})
        HIP_OK(hipMemsetAsync(bptr->p, 0, sizeof(double) * bptr->n, c->stream));
    HIP_OK(hipMemsetAsync(gs.kmask.p, 0, sizeof(uint64_t) * gs.kmask.n, c->stream));
    gs.flags_h.clear();
    return 0;
}

/* the identity-row flags of this Jacobian (AoS and planar), the neighbours' of the adjacent
 * latitude rows in the halo; the planar iterate zeroed */
static int gs_identity_flags(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    const int64_t NE = c->sub.nerows(), next = c->sub.next;
    const unsigned gN = (unsigned)std::min<int64_t>((NE + 255) / 256, 4096);
    int rc;
    HIP_OK(hipMemsetAsync(gs.known.p, 1, NE, c->stream));     /* outer halo rows: identity */
    /* the planar iterate: 0 on the rows no pass writes (identity rows of this Jacobian, T/S) */
    HIP_OK(hipMemsetAsync(gs.zP.p, 0, sizeof(double) * NE, c->stream));
    hipLaunchKernelGGL(k_known, dim3(blocks_for(c->sub.nloc)), dim3(256), 0, c->stream, c->d_val.p, lay_of(c->sub),
                       (int64_t)c->rowintcon, gs.known.p);
    HIP_OK(hipGetLastError());
    if (c->sub.nranks > 1) {
        /* the neighbours' flags of the adjacent latitude rows */
        hipLaunchKernelGGL(k_u8_to_d, dim3(gN), dim3(256), 0, c->stream, gs.known.p, gs.rr.p, NE);
        if ((rc = halo_exchange_w(c, gs.rr.p, NUN, 1))) return rc;
        hipLaunchKernelGGL(k_d_to_u8, dim3(gN), dim3(256), 0, c->stream, gs.rr.p, gs.known.p, NE);
    }
    hipLaunchKernelGGL(k_known_planar, dim3((unsigned)((next + 255) / 256)), dim3(256), 0, c->stream,
                       gs.known.p, gs.knP.p, next);
    return 0;
}

/* global column / U/V-point flags: the Schur structure is that of the whole grid */
static int gs_global_structure(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    int rc;
    const size_t nf = (size_t)2 * c->n * c->m;
    if (gs.flags_d.reserve(nf)) return IEMIC_ENOMEM;
    HIP_OK(hipMemsetAsync(gs.flags_d.p, 0, sizeof(double) * nf, c->stream));
    hipLaunchKernelGGL(k_band_flags, dim3((unsigned)((c->sub.nloc / c->l + 255) / 256)), dim3(256), 0, c->stream,
                       gs.known.p, lay_of(c->sub), gs.flags_d.p);
    if ((rc = allreduce_sum(c, gs.flags_d.p, (int)nf))) return rc;
    std::vector<double> flags(nf);
    if ((rc = d2h(c, flags.data(), gs.flags_d.p, sizeof(double) * nf))) return rc;
    if (flags != gs.flags_h)
        if ((rc = build_structure(c, flags))) return rc;
    return 0;
}

/* the cells' 2x2 inverses, depth weights and P couplings, with the neighbours' in the halo */
static int gs_cell_factors(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    const Lay L = lay_of(c->sub);
    const int64_t next = c->sub.next;
    const unsigned gc = blocks_for(c->sub.nloc);
    int rc;
    if (gs.gslot.n < (size_t)GSL * next) {
        if (gs.gslot.alloc((size_t)GSL * next)) return IEMIC_ENOMEM;
        HIP_OK(hipMemsetAsync(gs.gslot.p, 0, sizeof(double) * gs.gslot.n, c->stream));
    }
    hipLaunchKernelGGL(k_cell_factors, dim3(gc), dim3(256), 0, c->stream, c->d_val.p, gs.known.p,
                       L, (int64_t)c->rowintcon, c->cfg.int_sign, c->d_intc.p, gs.uvinv.p,
                       gs.sw.tsinv.p, gs.pw.p, gs.tsdiag.p, next);
    hipLaunchKernelGGL(k_gslot_pack, dim3(gc), dim3(256), 0, c->stream, c->d_val.p, L, gs.gslot.p);
    if (c->sub.nranks > 1) {
        if ((rc = halo_exchange_w(c, gs.uvinv.p, 4, 1))) return rc;
        if ((rc = halo_exchange_w(c, gs.gslot.p, GSL, 1))) return rc;
    }
    return 0;
}

/* the Schur right-hand side as a linear form in rr (k_gs_ptil_rcol), the identity-column
 * slot masks and the compact T/S couplings */
static int gs_apply_tables(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    const Lay L = lay_of(c->sub);
    const int64_t next = c->sub.next;
    const unsigned gc = blocks_for(c->sub.nloc);
    if (c->l <= 64) {
        const int64_t ncolb = c->sub.nloc / c->l;
        if (gs.rcol.reserve((size_t)(ncolb * RC_NE * c->l))) return IEMIC_ENOMEM;
        hipLaunchKernelGGL(k_rcol_uvp, dim3(blocks_for(ncolb * c->l)), dim3(256), 0, c->stream, c->d_val.p,
                           gs.known.p, gs.uvinv.p, gs.pw.p, gs.rcol.p, L);
        hipLaunchKernelGGL(k_rcol_w, dim3(blocks_for(ncolb * 9)), dim3(256), 0, c->stream, gs.known.p,
                           gs.gslot.p, gs.rcol.p, L);
    }
    hipLaunchKernelGGL(k_knownmask, dim3(gc), dim3(256), 0, c->stream, c->d_val.p, gs.known.p,
                       gs.kmask.p, L, c->sub.jb1);
    hipLaunchKernelGGL(k_ts_compact, dim3(gc), dim3(256), 0, c->stream, c->d_val.p, gs.known.p,
                       gs.sw.tsoff.p, L, next, (int64_t)c->rowintcon);
    if (ts_compact(c))
        hipLaunchKernelGGL(k_ts_pack, dim3(gc), dim3(256), 0, c->stream, gs.sw.tsoff.p, gs.sw.tsinv.p,
                           gs.sw.tsc.p, gs.sw.tic.p, L, next);
    return 0;
}

/* the Schur matrix: every band builds the rows of its own columns, the sum over the ranks
 * is the whole matrix, factorised by cyclic reduction on every rank.  Stream-ordered on one
 * rank (no host synchronisation); cr_check(gs.cr) follows */
static int gs_schur_factor(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    int rc;
    const int NC = c->n * c->m;
    HIP_OK(hipMemsetAsync(gs.S9.p, 0, sizeof(double) * 9 * (size_t)NC, c->stream));
    const int64_t nt = (int64_t)c->sub.nx * c->sub.mb * 9;
    hipLaunchKernelGGL(k_schur_build, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_val.p, gs.known.p, gs.uvinv.p, gs.gslot.p, gs.pw.p, gs.col_of_ij.p,
                       gs.pinned.p, lay_of(c->sub), c->sub.jb1, gs.S9.p);
    if ((rc = allreduce_sum(c, gs.S9.p, 9 * NC))) return rc;
    return cr_factor(c, gs.cr, gs.S9.p, gs.col_of_ij.p);
}

/* The two factorisations of the set-up.  Both are dependent chains of small launches (the
 * register Gauss-Jordan levels fill at most 96 of 256 CUs) that read only the Jacobian, the
 * identity flags, the cell factors and the compact T/S couplings, and write only their own
 * arrays: the Schur chain S9 and gs.cr, the T/S chain gs.mg (its levels' arrays and its own
 * SchurCR gs.mg.cr); neither touches the context's reduction buffers.  One rank: the Schur
 * chain is enqueued on the stream, then the T/S set-up runs with c->stream naming the side
 * stream (forked after the apply tables; its host waits -- the coarsest level's pivot flag
 * -- wait for the side stream alone, with the Schur chain already in the queue), the stream
 * joins, and the Schur pivot flag is read after both.  Subdomains: both chains communicate
 * (the all-reduce of S9, the T/S halo rows and the global coarsest problem), and the host
 * and in-process transports synchronise the stream c->stream names, so the order stays
 * serial there, the same on every rank.  IEMIC_SERIAL_SETUP=1 keeps it serial on one rank
 * too (the same launches in the same per-chain order: the factors are bitwise the same). */
static int gs_factor(iemic_ctx* c, int sweeps)
{
    BlockGS& gs = c->gs;
    int rc;
    if (c->serial_setup || c->sub.nranks > 1) {
        if ((rc = gs_schur_factor(c))) return rc;
        if ((rc = cr_check(c, gs.cr))) return rc;
        return ts_mg_setup(c, sweeps);
    }
    HIP_OK(OnSide::fork(c));
    if ((rc = gs_schur_factor(c))) return rc;     /* nothing on the side stream yet */
    OnSide on(c, false);
    rc = ts_mg_setup(c, sweeps);
    /* join, also on the error path: no work of this set-up stays on the side stream */
    const hipError_t e = on.join(true);
    if (e != hipSuccess && !rc) {
        set_error(std::string("block GS set-up join: ") + hipGetErrorString(e));
        rc = IEMIC_EDEVICE;
    }
    if (rc) return rc;
    return cr_check(c, gs.cr);
}

int gs_compute(iemic_ctx* c, const iemic_krylov* opt)
{
    BlockGS& gs = c->gs;
    gs.ready = 0;
    gs.ts_sweeps = opt ? std::max(0, opt->ts_sweeps) : 3;
    const int64_t NE = c->sub.nerows();
    if (c->l > 64) {
        set_error("block GS: more than 64 levels per column (the column kernels hold a column in one workgroup)");
        return IEMIC_EINVAL;
    }
    int rc = 0;
    if ((rc = gs_reserve_cells(c))) return rc;
    if ((rc = gs_identity_flags(c))) return rc;
    bool act_changed = false;
    if ((rc = act_build(c, &act_changed))) return rc;
    if (act_changed)
        /* the defect (k_spmv_dyn) writes the active cells only: the others' rows 0 */
        for (DevBuf<double>* bptr : {&gs.dres, &gs.dq})
            if (bptr->p) HIP_OK(hipMemsetAsync(bptr->p, 0, sizeof(double) * bptr->n, c->stream));
    if ((rc = gs_global_structure(c))) return rc;
    if ((rc = gs_cell_factors(c))) return rc;
    if ((rc = act_pack_streams(c))) return rc;
    /* the staged applies write rrP on the active cells only, and leave z's identity rows */
    HIP_OK(hipMemsetAsync(gs.rrP.p, 0, sizeof(double) * gs.rrP.n, c->stream));
    c->kr.zclean = 0;
    if ((rc = gs_apply_tables(c))) return rc;
    gs.ts_mg = opt ? std::max(0, opt->ts_mg) : 0;
    if ((rc = gs_factor(c, opt ? std::max(1, opt->mg_sweeps) : 1))) return rc;
    gs.dyn_iters = opt ? std::max(1, opt->dyn_iters) : 1;
    gs.dyn_mr = opt ? (opt->dyn_mr != 0) : 0;
    gs.dyn_omega = opt && opt->dyn_omega > 0.0 ? opt->dyn_omega : 1.0;
    gs.ts_at = opt ? std::max(0, opt->ts_at) : 0;
    gs.schur_passes = opt ? std::max(0, opt->schur_passes) : 0;
    if (gs.dyn_iters > 1 && gs.dres.n < (size_t)NE) {
        if (gs.dres.alloc(NE) || gs.zc.alloc(NE) || gs.dq.alloc(NE) || gs.dzero.alloc(NE) ||
            gs.dmr.alloc(2 * MR_NB + 2))
            return IEMIC_ENOMEM;
        for (DevBuf<double>* bptr : {&gs.dres, &gs.zc, &gs.dq, &gs.dzero})
            HIP_OK(hipMemsetAsync(bptr->p, 0, sizeof(double) * NE, c->stream));
    }
    HIP_OK(hipGetLastError());
    gs.ready = 1;
    return 0;
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
/* does dynamics pass it (0 .. dyn_iters - 1) solve the Schur system?  schur_passes k: the first
 * k - 1 passes and the last (k = 1: the first only; 0 or >= dyn_iters: every pass).  The twin
 * at 2 degrees: every pass 203 FGMRES steps; the first and the last 203; the first two 207;
 * the first and the third 205; the first only 300 (profiles/r06_prec_study.md) */
static bool gs_pass_schur(const BlockGS& gs, int it)
{
    const int k = gs.schur_passes, n = gs.dyn_iters;
    return it == 0 || k <= 0 || k >= n || (k >= 2 && (it < k - 1 || it == n - 1));
}

static int dyn_solve(iemic_ctx* c, const double* rr, double* z, double* zo = nullptr, double omega = 0.0,
                     double* zaos = nullptr, bool rr_halo = false, bool schur = true)
{
    BlockGS& gs = c->gs;
    const Lay L = lay_of(c->sub);
    const unsigned gc = (unsigned)((c->sub.nloc + 255) / 256);
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
    const unsigned gcu = (unsigned)((nown + (hrow ? (int64_t)c->l * c->sub.nx : 0) + 255) / 256);
    hipLaunchKernelGGL(k_gs_uvp, dim3(gcu), dim3(256), 0, s, gs.act.vp, gs.knP.p, gs.uvinv.p,
                       rr, pbT, z, L, zo, omega, zaos, gsl, al ? gs.act.act.p : nullptr, nown);
    if (band && !hrow && (rc = halo_exchange_planar(c, z, NUN, ps, 1))) return rc;   /* uv below the band */
    with_lanes(Pl, [&](auto p) {
        hipLaunchKernelGGL(k_gs_pw_t<LANES_OF(p)>, dim3(gct), bct, 0, s, gs.act.vp, gs.knP.p,
                           pbT, z, L, rr, zo, omega, zaos);
    });
    return 0;
}

int spmv_dyn_defect(iemic_ctx* c, const double* z, const double* r, const uint8_t* knP, double* d, bool halo = false);

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

static int gs_apply_impl(iemic_ctx* c, const double* r, double* z, bool cmp, bool staged = false);
int gs_apply(iemic_ctx* c, const double* r, double* z) { return gs_apply_impl(c, r, z, false); }
int gs_apply_c(iemic_ctx* c, const double* rc, double* z, bool staged) { return gs_apply_impl(c, rc, z, true, staged); }

static int gs_apply_impl(iemic_ctx* c, const double* r, double* z, bool cmp, bool staged)
{
    BlockGS& gs = c->gs;
    const Lay L = lay_of(c->sub);
    const unsigned gc = (unsigned)((c->sub.nloc + 255) / 256);
    hipStream_t s = c->stream;
    const bool band = c->sub.nranks > 1;
    const int64_t ps = c->sub.next;
    double* zP = gs.zP.p;
    int rc = gs_refresh(c);
    if (rc) return rc;
    /* the T/S block is solved with the right-hand side rr_TS - A_TS,D z_D of the dynamics
     * iterate after ts_at passes (default: after the last; the CPU twin: orc_gs_apply); the
     * later passes neither read nor write the T/S rows */
    const int ts_at = (!gs.dyn_mr && gs.ts_at >= 1 && gs.ts_at < gs.dyn_iters) ? gs.ts_at : gs.dyn_iters;
    /* early T/S on one rank: its V-cycles run on the side stream beside the remaining
     * dynamics passes (both chains are latency-bound, so they overlap) */
    const bool par = ts_at < gs.dyn_iters && !band && gs.ts_mg > 0;
    /* the dynamics passes iterate on the planar zP; the output z (AoS) gets their final
     * values from the last pass (every pass for the T/S sweeps, which read z's AoS rows) */
    const bool aos_all = gs.ts_mg <= 0;
    auto zaos_of = [&](bool last) { return (last || aos_all) ? z : nullptr; };
    /* latitude bands: the last pass also updated the iterate's south halo row U/V (k_gs_uvp),
     * all the T/S right-hand side reads of it beyond the band (A_TS,D couples U/V at j - 1 and
     * W in the column): no exchange (the fixed-step passes only) */
    const bool ts_local = band && c->sub.npx == 1 && gs.ts_mg > 0 && !gs.dyn_mr && ts_at == gs.dyn_iters &&
                          gs.dyn_iters > 1;
    auto ts = [&]() -> int {
        if (band && !ts_local && (ts_at < gs.dyn_iters || gs.dyn_iters > 1)) {
            rc = gs.ts_mg > 0 ? halo_exchange_planar(c, zP, NUN, ps, 1) : halo_exchange(c, z, 1);
            if (rc) return rc;
        }
        return ts_solve(c, gs.ts_mg > 0 ? zP : z, z, ts_at == gs.dyn_iters, par);
    };
    /* the halo rows of r hold the neighbours' identity-row values the couplings need (a
     * compressed r is zero on every identity row: no couplings, no exchange) */
    if (cmp) {
        /* staged: the update pass wrote rrP (its land entries stay 0 since the set-up, the
         * identity rows of z were zeroed per set-up: Krylov::zclean) */
        if (!staged || aos_all)
            hipLaunchKernelGGL(k_gs_rr_c, dim3(gc), dim3(256), 0, s, gs.known.p, gs.act.cmap.p, r, z,
                               aos_all ? gs.rr.p : nullptr, aos_all ? 1 : 0, gs.rrP.p, L);
    } else {
        if (band && (rc = halo_exchange(c, const_cast<double*>(r), 1))) return rc;
        hipLaunchKernelGGL(k_gs_rr, dim3(gc), dim3(256), 0, s, gs.act.vp, gs.known.p, gs.kmask.p,
                           r, z, aos_all ? gs.rr.p : nullptr, aos_all ? 1 : 0, gs.rrP.p, L);
    }
    if ((rc = dyn_solve(c, gs.rrP.p, zP, nullptr, 0.0, zaos_of(gs.dyn_iters == 1)))) return rc;
    if (ts_at == 1 && gs.dyn_iters > 1 && (rc = ts())) return rc;
    /* defect correction on the dynamics block: z_D += w M_D^-1 (rr_D - A_DD z_D), with the
     * minimal-residual w (dyn_mr) or the fixed w = dyn_omega */
    if (gs.dyn_mr && gs.dyn_iters > 1) {
        if (band && (rc = halo_exchange_planar(c, zP, NUN, ps, 1))) return rc;
        if ((rc = spmv_dyn_defect(c, zP, gs.rrP.p, gs.knP.p, gs.dres.p))) return rc;
        for (int it = 1; it < gs.dyn_iters; it++) {
            const bool last = it + 1 == gs.dyn_iters;
            if ((rc = dyn_solve(c, gs.dres.p, gs.zc.p))) return rc;
            if (band && (rc = halo_exchange_planar(c, gs.zc.p, NUN, ps, 1))) return rc;
            if ((rc = spmv_dyn_defect(c, gs.zc.p, gs.dzero.p, gs.knP.p, gs.dq.p))) return rc;
            hipLaunchKernelGGL(k_mr_dots, dim3(MR_NB), dim3(256), 0, s, gs.dres.p, gs.dq.p, L, gs.dmr.p);
            hipLaunchKernelGGL(k_mr_sum, dim3(1), dim3(64), 0, s, gs.dmr.p, MR_NB);
            if (band && (rc = allreduce_sum(c, gs.dmr.p + 2 * MR_NB, 2))) return rc;
            hipLaunchKernelGGL(k_mr_update, dim3(gc), dim3(256), 0, s, gs.knP.p, gs.dmr.p + 2 * MR_NB,
                               gs.zc.p, gs.dq.p, zP, gs.dres.p, L, last ? 0 : 1, zaos_of(last));
        }
    }
    /* latitude bands: the defect on the two halo rows too (from a 2-deep halo of the U/V/W/P
     * planes), so that the pass needs no exchange of it (2 -> 1 exchange batch per pass) */
    const bool dhalo = band && c->sub.npx == 1 && gs.act.dvh.p;
    for (int it = 1; !gs.dyn_mr && it < gs.dyn_iters; it++) {
        const bool last = it + 1 == gs.dyn_iters;
        if (band && (rc = dhalo ? halo_exchange_planar(c, zP, 4, ps, 2) : halo_exchange_planar(c, zP, NUN, ps, 1)))
            return rc;   /* w, p of the neighbours */
        if ((rc = spmv_dyn_defect(c, zP, gs.rrP.p, gs.knP.p, gs.dres.p, dhalo))) return rc;
        const bool schur = gs_pass_schur(gs, it);
        if ((rc = dyn_solve(c, gs.dres.p, gs.zc.p, zP, gs.dyn_omega, zaos_of(last), dhalo, schur)))
            return rc;   /* z += w zc */
        if (it + 1 == ts_at && it + 1 < gs.dyn_iters && (rc = ts())) return rc;
    }
    if (ts_at == gs.dyn_iters && (rc = ts())) return rc;
    if (ts_at < gs.dyn_iters && gs.ts_mg > 0) {
        if (par) HIP_OK(OnSide::wait(c));                        /* join */
        if ((rc = ts_mg_out(c, z))) return rc;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace iemic
