/*
 * band_lu.hip -- LU factorisation and explicit inverse of a band matrix on the device
 * (the global coarsest problem of the T/S multigrid, ts_mg_setup.hip).
 */
#include <algorithm>

#include "common.h"

namespace iemic {

namespace {

/* Band LU with partial pivoting (LAPACK gbtrf semantics), one workgroup of 1024 threads,
 * right-looking and blocked by panels of NBP columns: the panel is factorised in LDS
 * (partial pivoting, full panel-row interchanges), row swaps and U12 = L11^-1 A12 follow,
 * and the trailing window is updated once per panel (A22 -= L21 U12) instead of once per
 * column.  U stays in the band (row i holds columns [i-bl, i+bl+bu] at offset
 * j - i + bl); the panel multipliers go to lpan[panel][NBP + bl][NBP], so a solve applies,
 * panel by panel, the panel's interchanges and then its multipliers. */
constexpr int NBP = BAND_NBP;

__global__ void __launch_bounds__(1024) k_band_lu(double* __restrict__ ab, int ncol, int bl, int bu,
                                                  int* __restrict__ piv, int* __restrict__ info,
                                                  double* __restrict__ lpan, int stage_o)
{
    extern __shared__ double lds[];
    const int W = 2 * bl + bu + 1;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwave = nthr >> 6;
    /* panel rows padded to PS = NBP + 1 doubles: lanes walking a column hit distinct banks */
    constexpr int PS = NBP + 1;
    double* P = lds;                              /* (NBP + bl) x PS panel           */
    double* U = lds + (NBP + bl) * PS;            /* NBP x (bl + bu) block row U12   */
    double* Uo = U + NBP * (bl + bu);             /* NBP x (bl + bu) pivot rows below */
    __shared__ int s_lp[NBP], s_slot[NBP];
    __shared__ double s_best;
    __shared__ int s_info;
    if (tid == 0) s_info = 0;
    auto A = [&](int i, int j) -> double& { return ab[(int64_t)i * W + (j - i + bl)]; };
    for (int k0 = 0; k0 < ncol; k0 += NBP) {
        const int nbk = min(NBP, ncol - k0);
        const int pend = min(k0 + nbk - 1 + bl, ncol - 1);
        const int nprow = pend - k0 + 1;
        /* load the panel */
        for (int e = tid; e < nprow * NBP; e += nthr) {
            const int r = e / NBP, t = e % NBP;
            /* columns right of row r's band (t - r > bl + bu, a band narrower than the panel)
             * are not stored: zero, not the neighbouring rows' entries */
            P[r * PS + t] = (t < nbk && r <= t + bl && t - r <= bl + bu) ? A(k0 + r, k0 + t) : 0.0;
        }
        __syncthreads();
        /* factorise the panel: wavefront 0 finds the pivot and interchanges the panel
         * rows; then one thread per row below scales its multiplier and updates the rest
         * of its row (two workgroup barriers per column) */
        for (int t = 0; t < nbk; t++) {
            const int rlast = min(t + bl, nprow - 1);
            if (wave == 0) {
                double best = -1.0;
                int bi = t;
                for (int r = t + lane; r <= rlast; r += 64) {
                    const double v = fabs(P[r * PS + t]);
                    if (v > best) { best = v; bi = r; }
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const double ob = __shfl_down(best, off, 64);
                    const int oi = __shfl_down(bi, off, 64);
                    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
                }
                best = __shfl(best, 0, 64);
                const int rp = __shfl(bi, 0, 64);
                if (best == 0.0) {
                    if (lane == 0) {
                        s_lp[t] = t;
                        piv[k0 + t] = k0 + t;
                        s_best = 0.0;
                        if (s_info == 0) s_info = k0 + t + 1;
                    }
                } else {
                    if (rp != t && lane < nbk) {
                        const double x = P[t * PS + lane];
                        P[t * PS + lane] = P[rp * PS + lane];
                        P[rp * PS + lane] = x;
                    }
                    if (lane == 0) { s_lp[t] = rp; piv[k0 + t] = k0 + rp; s_best = best; }
                }
            }
            __syncthreads();
            if (s_best == 0.0) {
                __syncthreads();
                continue;
            }
            const double pivot = P[t * PS + t];
            for (int r = t + 1 + tid; r <= rlast; r += nthr) {
                const double l = P[r * PS + t] / pivot;
                P[r * PS + t] = l;
                for (int cc = t + 1; cc < nbk; cc++) P[r * PS + cc] -= l * P[t * PS + cc];
            }
            __syncthreads();
        }
        /* U11 back to the band; the multipliers (L11, L21 with the panel's row
         * interchanges applied, LAPACK getrf convention) go to the panel store */
        double* Lp = lpan + (int64_t)(k0 / NBP) * (NBP + bl) * NBP;
        for (int e = tid; e < (NBP + bl) * NBP; e += nthr) {
            const int r = e / NBP, t = e % NBP;
            const bool in = r < nprow && t < nbk;
            if (in && r <= t && t - r <= bl + bu) A(k0 + r, k0 + t) = P[r * PS + t];
            Lp[e] = (in && r > t) ? P[r * PS + t] : 0.0;
        }
        /* A12 (the panel rows right of the panel) and the rows below the panel that were
         * chosen as pivots (distinct ones, slot s_slot[t]) are staged in LDS with coalesced
         * loads; per column (one thread each) the interchanges in pivot order and
         * U12 = L11^-1 A12 then run on LDS only, and the pivot rows are written back */
        const int jlo = k0 + nbk, jhi = min(k0 + nbk - 1 + bl + bu, ncol - 1);
        const int ncu = jhi - jlo + 1;
        const int LW = bl + bu;
        if (tid == 0)
            for (int t = 0; t < nbk; t++) {
                int sl = -1;
                if (s_lp[t] >= nbk) {
                    sl = t;
                    for (int u = 0; u < t; u++)
                        if (s_lp[u] == s_lp[t]) { sl = s_slot[u]; break; }
                }
                s_slot[t] = sl;
            }
        for (int e = tid; e < nbk * ncu; e += nthr) {
            const int t = e / ncu, jj = e % ncu, j = jlo + jj;
            U[t * LW + jj] = (j <= k0 + t + bl + bu) ? A(k0 + t, j) : 0.0;
        }
        __syncthreads();
        for (int e = tid; e < nbk * ncu; e += nthr) {
            const int t = e / ncu, jj = e % ncu;
            if (stage_o && s_slot[t] == t) Uo[t * LW + jj] = A(k0 + s_lp[t], jlo + jj);
        }
        __syncthreads();
        for (int jj = tid; jj < ncu; jj += nthr) {
            const int j = jlo + jj;
            for (int t = 0; t < nbk; t++) {
                const int rp = s_lp[t];
                if (rp == t || j > k0 + t + bl + bu) continue;
                double& x = U[t * LW + jj];
                double& y = rp < nbk ? U[rp * LW + jj] : (stage_o ? Uo[s_slot[t] * LW + jj] : A(k0 + rp, j));
                const double tmp = x; x = y; y = tmp;
            }
            double u[NBP];
            for (int t = 0; t < nbk; t++) {
                double v = U[t * LW + jj];
                for (int q = 0; q < t; q++) v -= P[t * PS + q] * u[q];
                u[t] = v;
                U[t * LW + jj] = v;
                if (j <= k0 + t + bl + bu) A(k0 + t, j) = v;
            }
        }
        __syncthreads();
        for (int e = tid; e < nbk * ncu; e += nthr) {
            const int t = e / ncu, jj = e % ncu;
            if (stage_o && s_slot[t] == t) A(k0 + s_lp[t], jlo + jj) = Uo[t * LW + jj];
        }
        __syncthreads();
        /* A22 -= L21 U12 over rows k0+nbk .. pend: 4x4 register tiles (lanes along the
         * columns, so the 16 global loads of a tile are coalesced across the wavefront and
         * issued together before the rank-NBP update) */
        {
            const int nr2 = nprow - nbk;
            const int tr = (nr2 + 3) / 4, tc = (ncu + 3) / 4;
            for (int e = tid; e < tr * tc; e += nthr) {
                const int r0 = nbk + 4 * (e / tc), j0 = 4 * (e % tc);
                double a[4][4];
#pragma unroll
                for (int x = 0; x < 4; x++)
#pragma unroll
                    for (int y = 0; y < 4; y++) {
                        const int r = r0 + x, jj = j0 + y;
                        a[x][y] = (r < nprow && jj < ncu) ? A(k0 + r, jlo + jj) : 0.0;
                    }
                for (int t = 0; t < nbk; t++) {
                    double lv[4], uv[4];
#pragma unroll
                    for (int x = 0; x < 4; x++) lv[x] = r0 + x < nprow ? P[(r0 + x) * PS + t] : 0.0;
#pragma unroll
                    for (int y = 0; y < 4; y++) uv[y] = j0 + y < ncu ? U[t * (bl + bu) + j0 + y] : 0.0;
#pragma unroll
                    for (int x = 0; x < 4; x++)
#pragma unroll
                        for (int y = 0; y < 4; y++) a[x][y] -= lv[x] * uv[y];
                }
#pragma unroll
                for (int x = 0; x < 4; x++)
#pragma unroll
                    for (int y = 0; y < 4; y++) {
                        const int r = r0 + x, jj = j0 + y;
                        if (r < nprow && jj < ncu) A(k0 + r, jlo + jj) = a[x][y];
                    }
            }
        }
        __syncthreads();
    }
    if (tid == 0) *info = s_info;
}

/* Columns cols[q0 .. q0+NB) of the inverse, X = U^-1 L^-1 P, one workgroup of 256
 * threads per block of NB right-hand sides (unit vectors); cols ascending.  Column q of
 * the slab is X[row * nq + q] (row-major ncol x nq).  Thread t owns slab column t % NB
 * and every 256/NB-th row of the active window; the window lives in LDS as a ring buffer:
 *   forward  (P, L^-1): rows k..k+bl      y is written to X
 *   backward (U^-1)   : rows i+1..i+bl+bu x overwrites y in X
 * Two barriers per elimination step; the factors are read from L2. */
template <int NB, bool STAGE>
__global__ void __launch_bounds__(256) k_band_inv_pan(const double* __restrict__ ab,
                                                      const double* __restrict__ lpan,
                                                      const int* __restrict__ piv, int ncol,
                                                      int bl, int bu, const int* __restrict__ cols,
                                                      int nq, double* __restrict__ Xs)
{
    extern __shared__ double lds[];
    constexpr int G = 256 / NB;              /* row groups */
    const int W = 2 * bl + bu + 1;
    const int col = threadIdx.x % NB, grp = threadIdx.x / NB;
    const int q0 = blockIdx.x * NB;
    const int q = q0 + col;
    const bool on = q < nq;
    const int c0 = cols[q0];
    const int c = on ? cols[q] : -1;
    const int R1 = bl + NBP + 1, R2 = bl + bu + 1;
    double* red = lds;                       /* NBP x NB panel sums                     */
    double* win = lds + NBP * NB;            /* ring buffer                             */
    /* STAGE: the panel's multipliers (forward) / U rows (backward) are copied to LDS with
     * coalesced loads once per panel, so the inner loops read LDS instead of chains of
     * dependent global loads */
    double* ysh = win + (size_t)max(R1, R2) * NB;   /* NBP x NB forward results of a panel */
    double* stg = ysh + NBP * NB;
    /* ---- forward ---- */
    const int kst = (max(0, c0 - bl - NBP + 1) / NBP) * NBP;
    for (int r = kst + grp; r <= min(kst + NBP - 1 + bl, ncol - 1); r += G)
        win[(r % R1) * NB + col] = (r == c) ? 1.0 : 0.0;
    for (int k0 = kst; k0 < ncol; k0 += NBP) {
        const int nbk = min(NBP, ncol - k0);
        const int pend = min(k0 + nbk - 1 + bl, ncol - 1);
        const int nprow = pend - k0 + 1;
        const double* Lg = lpan + (int64_t)(k0 / NBP) * (NBP + bl) * NBP;
        if (STAGE)
            for (int e = threadIdx.x; e < nprow * NBP; e += 256) stg[e] = Lg[e];
        const double* Lp = STAGE ? stg : Lg;
        const int kb = k0 % R1;                  /* ring slot of row k0 */
        auto slot = [&](int r) { const int v = kb + r; return v >= R1 ? v - R1 : v; };  /* r < R1 */
        __syncthreads();
        if (grp == 0) {
            /* interchanges, then the unit-lower L11 solve, one column per lane */
            for (int t = 0; t < nbk; t++) {
                const int rp = piv[k0 + t] - k0;
                if (rp != t) {
                    double* a = win + slot(t) * NB + col;
                    double* b = win + slot(rp) * NB + col;
                    const double x = *a; *a = *b; *b = x;
                }
            }
            double y[NBP];
#pragma unroll
            for (int t = 0; t < NBP; t++) {
                if (t < nbk) {
                    double v = win[slot(t) * NB + col];
#pragma unroll
                    for (int u = 0; u < t; u++) v -= Lp[t * NBP + u] * y[u];
                    y[t] = v;
                    win[slot(t) * NB + col] = v;
                }
            }
        }
        __syncthreads();
        /* rows below the panel: -= L21 y (panel values held in registers) */
        {
            double y[NBP];
#pragma unroll
            for (int t = 0; t < NBP; t++) y[t] = t < nbk ? win[slot(t) * NB + col] : 0.0;
            for (int r = nbk + grp; r < nprow; r += G) {
                const double* lr = Lp + r * NBP;
                double a0 = 0.0, a1 = 0.0;
#pragma unroll
                for (int t = 0; t < NBP; t += 2) {
                    a0 += lr[t] * y[t];
                    a1 += lr[t + 1] * y[t + 1];
                }
                win[slot(r) * NB + col] -= a0 + a1;
            }
        }
        /* panel rows are final: y -> X */
        for (int t = grp; t < nbk; t += G)
            if (on) Xs[(int64_t)(k0 + t) * nq + q] = win[slot(t) * NB + col];
        __syncthreads();
        for (int r = pend + 1 + grp; r <= min(k0 + 2 * NBP - 1 + bl, ncol - 1); r += G)
            win[(r % R1) * NB + col] = (r == c) ? 1.0 : 0.0;
    }
    if (grp == 0 && on)
        for (int r = 0; r < kst; r++) Xs[(int64_t)r * nq + q] = 0.0;
    /* ---- backward, panels from the bottom: ring of R2 = bl + bu + 1 rows ---- */
    __syncthreads();
    const int npan = (ncol + NBP - 1) / NBP;
    const int WU = bl + bu + 1;              /* staged U row: columns i .. i+bl+bu */
    for (int pn = npan - 1; pn >= 0; pn--) {
        const int i0 = pn * NBP, i1 = min(ncol, i0 + NBP);
        const int nr = i1 - i0;
        if (STAGE) {
            for (int e = threadIdx.x; e < nr * WU; e += 256) {
                const int rr = e / WU, jj = e % WU;
                const int i = i0 + rr;
                stg[e] = (i + jj < ncol) ? ab[(int64_t)i * W + bl + jj] : 0.0;
            }
            __syncthreads();
        }
        /* t_i = sum_{j >= i1} U_ij x_j for the panel rows (rows x column per thread);
         * the forward results y_i of the panel rows are fetched alongside */
        for (int e = grp; e < nr; e += G) {
            ysh[e * NB + col] = on ? Xs[(int64_t)(i0 + e) * nq + q] : 0.0;
            const int i = i0 + e;
            const int jend = min(i + bl + bu, ncol - 1);
            double s0 = 0.0, s1 = 0.0;
            const double* ur = STAGE ? stg + e * WU - i : ab + (int64_t)i * W + (bl - i);
            /* x_j sits at ring slot j % R2: walk the slots with a wrap instead of a modulo */
            int js = i1 % R2;
            int j = i1;
            for (; j + 1 <= jend; j += 2) {
                const int js1 = js + 1 == R2 ? 0 : js + 1;
                s0 += ur[j] * win[js * NB + col];
                s1 += ur[j + 1] * win[js1 * NB + col];
                js = js1 + 1 == R2 ? 0 : js1 + 1;
            }
            if (j <= jend) s0 += ur[j] * win[js * NB + col];
            red[e * NB + col] = s0 + s1;
        }
        __syncthreads();
        if (grp == 0) {
            for (int i = i1 - 1; i >= i0; i--) {
                const double* ar = STAGE ? stg + (i - i0) * WU - i : ab + (int64_t)i * W + (bl - i);
                double t = red[(i - i0) * NB + col];
                const int jend = min(i1 - 1, i + bl + bu);
                int js = (i + 1) % R2;
                for (int j = i + 1; j <= jend; j++) {
                    t += ar[j] * win[js * NB + col];
                    js = js + 1 == R2 ? 0 : js + 1;
                }
                const double yv = ysh[(i - i0) * NB + col];
                const double x = (yv - t) / ar[i];
                win[(i % R2) * NB + col] = x;
                if (on) Xs[(int64_t)i * nq + q] = x;
            }
        }
        __syncthreads();
    }
}

}  // namespace

/* ab (N rows of 2 bl + bu + 1, LAPACK gbtrf layout) is factorised in place (pivots piv,
 * panel multipliers lpan: ceil(N / BAND_NBP) panels of (BAND_NBP + bl) x BAND_NBP) and the
 * columns cols[0 .. N) of its inverse are written row-major to X.  *info != 0: a zero pivot
 * (its column + 1, from the device flag info_d), X is not written. */
int band_lu_inverse(iemic_ctx* c, double* ab, int N, int bl, int bu, int* piv, int* info_d, double* lpan,
                    const int* cols, double* X, int* info)
{
    int rc;
    const size_t lb = sizeof(double) * ((size_t)(NBP + bl) * (NBP + 1) + (size_t)2 * NBP * (bl + bu));
    const int stage_o = lb <= 150 * 1024 ? 1 : 0;
    const size_t lbu = stage_o ? lb : lb - sizeof(double) * (size_t)NBP * (bl + bu);
    HIP_OK(hipFuncSetAttribute((const void*)k_band_lu, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lbu));
    hipLaunchKernelGGL(k_band_lu, dim3(1), dim3(1024), lbu, c->stream, ab, N, bl, bu, piv, info_d, lpan, stage_o);
    *info = 0;
    HIP_OK(hipGetLastError());
    if ((rc = d2h(c, info, info_d, sizeof(int)))) return rc;
    if (*info != 0) return 0;
    const int ring = std::max(bl + NBP + 1, bl + bu + 1);
    const size_t li = (size_t)(ring + 2 * NBP) * 16 * sizeof(double);
    HIP_OK(hipFuncSetAttribute((const void*)k_band_inv_pan<16, false>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)li));
    hipLaunchKernelGGL((k_band_inv_pan<16, false>), dim3((unsigned)((N + 15) / 16)), dim3(256), li, c->stream,
                       (const double*)ab, (const double*)lpan, (const int*)piv, N, bl, bu, cols, N, X);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace iemic
