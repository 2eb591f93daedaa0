/*
 * gs_setup.hip -- set-up of the block Gauss-Seidel preconditioner (prec_gs.hip has the overview):
 * the identity-row pattern and the Schur structure it implies, the per-cell factors, the tables
 * the apply reads (rcol, kmask, the compact T/S couplings), the Schur matrix and its cyclic
 * reduction, and the T/S multigrid's set-up beside it.  gs_compute lists the steps in order.
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

/* ---- the Schur right-hand side as a linear form in rr: its coefficients rcol -----------
 * (gs_dyn.hip has the derivation and the layout; k_gs_ptil_rcol evaluates the form) */

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
                if (!hnb(ti, tj, n, m, periodic)) continue;
                const int q2 = colid[(size_t)tj * n + ti];
                if (q2 < 0 || q2 == cq) continue;
                bool shared = false;
                for (int a = -1; a <= 0 && !shared; a++)
                    for (int b = -1; b <= 0 && !shared; b++) {
                        /* corner (i+a, j+b) must also be a corner of (ti,tj): e = di-a in {0,1} */
                        const int e = di - a, f = dj - b;
                        if (e < 0 || e > 1 || f < 0 || f > 1) continue;
                        int qi = i + a, qj = j + b;
                        if (!hnb(qi, qj, n, m, periodic)) continue;
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
    rc |= ts_sweeps_reserve(c);
    rc |= gs.tsdiag.alloc((size_t)4 * next);
    rc |= gs.knP.alloc(NE);
    rc |= gs.zP.alloc(NE);
    rc |= gs.rrP.alloc(NE);
    if (rc) {
        set_error("block GS: out of device memory");
        return IEMIC_ENOMEM;
    }
    for (DevBuf<double>* bptr : {&gs.uvinv, &gs.sw.tsinv, &gs.pw, &gs.rr, &gs.sw.bts, &gs.sw.tsoff, &gs.tsdiag,
                                 &gs.zP, &gs.rrP})
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
    const unsigned gN = (unsigned)std::min<int64_t>(blocks_for(NE), 4096);
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
    hipLaunchKernelGGL(k_known_planar, dim3(blocks_for(next)), dim3(256), 0, c->stream,
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
    hipLaunchKernelGGL(k_band_flags, dim3(blocks_for(c->sub.nloc / c->l)), dim3(256), 0, c->stream,
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
    ts_sweeps_pack(c);
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
    hipLaunchKernelGGL(k_schur_build, dim3(blocks_for(nt)), dim3(256), 0, c->stream,
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

}  // namespace iemic
