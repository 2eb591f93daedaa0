/*
 * eigs.hip -- linear stability of the resident state: shift-invert Arnoldi for J x = lambda B x.
 *
 * The seam is the generalised eigenvalue solver the reference's drivers build on the model's
 * applyMatrix / applyMassMat / applyPrecon (src/utils/JDQZInterface.H; run_ocean.C:82-97) and
 * run from Continuation::eigenSolver (Continuation.H:1108-1131).  JDQZ is an external library,
 * so nothing is restated here: this is an original solver behind that seam.
 *
 *   operator      A = (J - sigma B)^-1 B, sigma real; B = diag(iemic_diag_b) <= 0, zero on the
 *                 W, P, land and integral-condition rows, so A maps the infinite eigenvalues to 0
 *   eigenvalues   theta = 1 / (lambda - sigma): the largest |theta| are the lambda nearest sigma
 *   shifted_jacobian   assemble_jacobian + k_shift_diag, as theta_jacobian does for J2
 *   eigs_step     t = B v_j (from the previous step's k_eig_scale_bmul), w = A v_j by
 *                 krylov_solve, two classical Gram-Schmidt passes (mdot_host + k_lincomb) in
 *                 the inner product that leaves the P rows out (k_eig_drop_p),
 *                 h_{j+1,j} = ||w||, v_{j+1} = w / h_{j+1,j} and t = B v_{j+1} in one kernel
 *   eigs_ritz     all p Ritz vectors in one pass over the basis (k_eig_ritz)
 *   eigs_restart  thick (Krylov-Schur) restart: the basis compressed onto p kept directions in
 *                 place, in one pass (k_eig_compress), the residual vector moved behind them
 *   eigs_residual ||(J - sigma B) x - (lambda - sigma) B x|| and ||(J - sigma B) x|| in one pass
 *                 over two SpMV outputs (k_eig_residual), the products and the difference in
 *                 double-double (k_spmv_dd, k_eig_intcond_dd)
 *
 * The small Hessenberg eigenproblem is the caller's (iemic/eigs.py).  Not
 * parity-with-Fortran code: built with the default contraction, except k_shift_diag, whose
 * sum is pinned bit for bit by tests/test_gpu_eigs.py, and the double-double helpers, whose
 * error terms need each product rounded on its own.
 */
#include <algorithm>
#include <chrono>
#include <cmath>

#include "common.h"
#include "krylov_internal.h"
#include "mass_slots.h"
#include "vec_kernels.h"

namespace iemic {

/* val[diagonal slot of row v][lc] += -(sigma B) for v = U, V, T, S (blockIdx.y) of every
 * assembled cell: lanes along the cells, so each plane is written in contiguous 512-byte wave
 * stores.  Rows with B = 0 (land, the integral condition) keep their bits.  The product is
 * rounded before the sum (no FMA): the shifted diagonal is numpy's val + -(sigma * B). */
__global__ void __launch_bounds__(256) k_shift_diag(const double* __restrict__ B, double* __restrict__ val,
                                                    int64_t own0, int64_t nloc, double sigma)
{
#pragma clang fp contract(off)
    const int64_t lc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lc >= nloc) return;
    const int r = blockIdx.y;
    const int var = r == 0 ? THETA_VAR[0] : r == 1 ? THETA_VAR[1] : r == 2 ? THETA_VAR[2] : THETA_VAR[3];
    const int slot = r == 0 ? THETA_SLOT[0] : r == 1 ? THETA_SLOT[1] : r == 2 ? THETA_SLOT[2] : THETA_SLOT[3];
    const double b = B[NUN * (own0 + lc) + var];
    if (b == 0.0) return;
    double* d = val + (int64_t)slot * nloc + lc;
    const double sb = sigma * b;
    *d = *d + -sb;
}

/* the start vector: entry of global row g = idr_shadow_entry(g, 0, seed), whatever rank owns it
 * (owned cells are ordered (j, k, i), i fastest; the reference row is 6 ((k m + j) n + i) + var) */
__global__ void __launch_bounds__(256) k_eig_start(double* __restrict__ w, int n, int m, int l, int jb0, int ib0,
                                                   int nx, int64_t nloc, uint64_t seed)
{
    const int64_t lc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lc >= nloc) return;
    const int i = ib0 + (int)(lc % nx), k = (int)((lc / nx) % l), j = jb0 + (int)(lc / ((int64_t)nx * l));
    const uint64_t g = (uint64_t)NUN * (((uint64_t)k * m + j) * n + i);
    for (int v = 0; v < NUN; v++) w[NUN * lc + v] = idr_shadow_entry(g + v, 0, seed);
}

/* t = w without its P rows (N rows from a cell boundary).  The dot products of the Arnoldi loop
 * leave the P rows out: an iterative solve returns w plus an arbitrary multiple of the
 * Jacobian's null vectors, the pressure modes, which live in the P rows alone; in the plain
 * 2-norm that multiple enters H and can surface as a spurious converged Ritz value with B x = 0.
 * B is zero on the P rows, so the operator never reads them, and Arnoldi in this semi-inner
 * product is Arnoldi on the same operator restricted to the other rows: the same non-zero
 * eigenvalues, blind to the null vectors.  The basis keeps its P rows (the Ritz vectors need
 * them); only the reductions read the masked copy. */
__global__ void __launch_bounds__(256) k_eig_drop_p(const double* __restrict__ w, double* __restrict__ t, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        t[q] = (q % NUN == PP) ? 0.0 : w[q];
}

/* v = s w and t = B v: one read of w and of B, the new basis vector and the next solve's
 * right-hand side */
__global__ void __launch_bounds__(256) k_eig_scale_bmul(const double* __restrict__ w, const double* __restrict__ B,
                                                        double s, double* __restrict__ v, double* __restrict__ t,
                                                        int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        const double x = s * w[q];
        v[q] = x;
        t[q] = B[q] * x;
    }
}

/* X_q = sum_i Y[i][q] V_i for all q < P at once: one pass over the m basis rows.  A block takes
 * tiles of 512 rows, a lane the rows tid and tid + 256 of the tile, so every V_i is read in
 * contiguous 512-byte wave loads and each broadcast read of Y from LDS feeds two rows; the 2 P
 * accumulators stay in registers.  The basis loop is unrolled by four: eight loads are in
 * flight before the first FMA.  Y: m x P row-major (the host pads p to P with zero columns);
 * columns q >= p are not stored.  Algorithmic bytes (m + p) N 8. */
constexpr int RITZ_MAX_P = 16;
struct RitzOut {
    double* x[RITZ_MAX_P];
};
template <int P>
__global__ void __launch_bounds__(256) k_eig_ritz(const double* __restrict__ V, int64_t ldv, int m,
                                                  const double* __restrict__ Y, RitzOut out, int p, int64_t N)
{
    __shared__ double ys[IEMIC_EIGS_MAX_M * P];
    for (int i = threadIdx.x; i < m * P; i += blockDim.x) ys[i] = Y[i];
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * 512; base < N; base += (int64_t)gridDim.x * 512) {
        const int64_t q0 = base + threadIdx.x, q1 = q0 + 256;
        const bool in0 = q0 < N, in1 = q1 < N;
        double a0[P], a1[P];
#pragma unroll
        for (int q = 0; q < P; q++) a0[q] = a1[q] = 0.0;
        int i = 0;
        for (; i + 4 <= m; i += 4) {
            const double* v = V + (int64_t)i * ldv;
            double x0[4], x1[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                x0[u] = in0 ? v[u * ldv + q0] : 0.0;
                x1[u] = in1 ? v[u * ldv + q1] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int q = 0; q < P; q++) {
                    const double y = ys[(i + u) * P + q];
                    a0[q] += y * x0[u];
                    a1[q] += y * x1[u];
                }
        }
        for (; i < m; i++) {
            const double x0 = in0 ? V[(int64_t)i * ldv + q0] : 0.0;
            const double x1 = in1 ? V[(int64_t)i * ldv + q1] : 0.0;
#pragma unroll
            for (int q = 0; q < P; q++) {
                const double y = ys[i * P + q];
                a0[q] += y * x0;
                a1[q] += y * x1;
            }
        }
#pragma unroll
        for (int q = 0; q < P; q++)
            if (q < p) {
                if (in0) out.x[q][q0] = a0[q];
                if (in1) out.x[q][q1] = a1[q];
            }
    }
}

/* The thick restart's pass over the basis, in place: V_q <- sum_{i<j} Q[i][q] V_i for q < p and
 * V_p <- V_j, columns p + 1 .. j untouched.  Row r of the result depends on row r of the basis
 * alone, and a row belongs to one lane of one block: the lane reads its j + 1 values of the
 * row (the sums, then V_j) before it stores any of the p + 1, so the overlap of outputs and
 * inputs is harmless.  V is therefore not __restrict__, and the stores stay behind the loads.
 * Otherwise k_eig_ritz's shape: tiles of 512 rows, a lane two rows 256 apart, Q (j x P
 * row-major, padded with zero columns) in LDS, 2 P accumulators in registers, contiguous
 * 512-byte wave loads and stores.  Only rows < N are touched.  Needs p < j (so column p is
 * one of the j + 1).  Algorithmic bytes (j + 1 + p + 1) N 8. */
template <int P>
__global__ void __launch_bounds__(256) k_eig_compress(double* V, int64_t ldv, int j, const double* __restrict__ Q,
                                                      int p, int64_t N)
{
    __shared__ double qs[IEMIC_EIGS_MAX_M * P];
    for (int i = threadIdx.x; i < j * P; i += blockDim.x) qs[i] = Q[i];
    __syncthreads();
    for (int64_t base = (int64_t)blockIdx.x * 512; base < N; base += (int64_t)gridDim.x * 512) {
        const int64_t q0 = base + threadIdx.x, q1 = q0 + 256;
        const bool in0 = q0 < N, in1 = q1 < N;
        double a0[P], a1[P];
#pragma unroll
        for (int q = 0; q < P; q++) a0[q] = a1[q] = 0.0;
        int i = 0;
        for (; i + 4 <= j; i += 4) {
            const double* v = V + (int64_t)i * ldv;
            double x0[4], x1[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                x0[u] = in0 ? v[u * ldv + q0] : 0.0;
                x1[u] = in1 ? v[u * ldv + q1] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int q = 0; q < P; q++) {
                    const double y = qs[(i + u) * P + q];
                    a0[q] += y * x0[u];
                    a1[q] += y * x1[u];
                }
        }
        for (; i < j; i++) {
            const double x0 = in0 ? V[(int64_t)i * ldv + q0] : 0.0;
            const double x1 = in1 ? V[(int64_t)i * ldv + q1] : 0.0;
#pragma unroll
            for (int q = 0; q < P; q++) {
                const double y = qs[i * P + q];
                a0[q] += y * x0;
                a1[q] += y * x1;
            }
        }
        const double l0 = in0 ? V[(int64_t)j * ldv + q0] : 0.0;
        const double l1 = in1 ? V[(int64_t)j * ldv + q1] : 0.0;
#pragma unroll
        for (int q = 0; q < P; q++)
            if (q < p) {
                if (in0) V[(int64_t)q * ldv + q0] = a0[q];
                if (in1) V[(int64_t)q * ldv + q1] = a1[q];
            }
        if (in0) V[(int64_t)p * ldv + q0] = l0;
        if (in1) V[(int64_t)p * ldv + q1] = l1;
    }
}

/* ---- the true residual, compensated ----------------------------------------------------------
 * A pair converged to 1e-10 has a residual a - mu B x ten orders below its two terms: formed in
 * plain fp64, the rounding of a = (J - sigma B) x alone (a few u |J| |x|) is 1e-5 of it.  So the
 * products of iemic_eigs_residual are formed in double-double (unevaluated sums hi + lo, two_prod
 * by FMA): k_spmv_dd is the SpMV of spmv.hip's k_spmv7 on the same coefficient planes, same
 * neighbour rules, with a double-double accumulator per row, and k_eig_residual subtracts in
 * double-double before it rounds.  The sums of squares have no cancellation and stay fp64.
 * The error-free transformations are built without contraction: a product fused into the sum
 * that follows it would no longer be the term whose rounding error the next line recovers.
 * Called once per returned pair, so k_spmv_dd is the plain one-lane-per-cell form: coefficient
 * planes read in contiguous wave loads, x gathered from global memory. */
struct dd {
    double h, l;
};
__device__ __forceinline__ dd two_sum(double a, double b)
{
#pragma clang fp contract(off)
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd quick_sum(double a, double b)   /* |a| >= |b| */
{
#pragma clang fp contract(off)
    const double s = a + b;
    return {s, b - (s - a)};
}
__device__ __forceinline__ dd two_prod(double a, double b)
{
#pragma clang fp contract(off)
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
__device__ __forceinline__ dd dd_add(dd a, dd b)
{
#pragma clang fp contract(off)
    const dd s = two_sum(a.h, b.h);
    return quick_sum(s.h, s.l + (a.l + b.l));
}
__device__ __forceinline__ dd dd_sub(dd a, dd b) { return dd_add(a, dd{-b.h, -b.l}); }
__device__ __forceinline__ dd dd_mul(dd a, dd b)
{
#pragma clang fp contract(off)
    const dd p = two_prod(a.h, b.h);
    return quick_sum(p.h, p.l + (a.h * b.l + a.l * b.h));
}

/* y = (J - sigma B) x on the owned cells, y = yh + yl: a lane per cell, its six rows in turn
 * (x's halo rows must be current; the integral-condition row is k_eig_intcond_dd's) */
__global__ void __launch_bounds__(256) k_spmv_dd(SubLay X, const double* __restrict__ val,
                                                 const double* __restrict__ x, double* __restrict__ yh,
                                                 double* __restrict__ yl, int64_t own0, int64_t nloc)
{
    const int64_t lc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lc >= nloc) return;
    const int nx = X.nx, l = X.l;
    const int64_t row = lc / nx;
    const int il = (int)(lc - row * nx), k = (int)(row % l), j = X.jb0 + (int)(row / l);
    const int jj[3] = {j > 0 ? j - 1 : j, j, j < X.m - 1 ? j + 1 : j};
    const int kk[3] = {k > 0 ? k - 1 : k, k, k < l - 1 ? k + 1 : k};
    const int64_t q0 = NUN * (own0 + lc);
#pragma unroll
    for (int R = 0; R < NUN; R++) {
        dd acc{0.0, 0.0};
#pragma unroll
        for (int s = ROW_BEGIN[R]; s < ROW_BEGIN[R + 1]; s++) {
            const Slot sl = SLOTS[s];
            const int64_t r = ((int64_t)jj[sl.dj + 1] - X.jb0 + HALO) * l + kk[sl.dk + 1];
            const int64_t cell = sl.di == 0 ? r * nx + il
                                            : xnb_cell(r, il + sl.di, X.n, X.ib0, nx, X.hx, X.periodic, X.xb);
            acc = dd_add(acc, two_prod(val[(int64_t)s * nloc + lc], x[NUN * cell + sl.var]));
        }
        yh[q0 + R] = acc.h;
        yl[q0 + R] = acc.l;
    }
}

/* the dense integral-condition row in double-double: out4 = {hi, lo} of coef . xr and of
 * coef . xi (block 1; zeros without xi).  One block a vector, a fixed order: deterministic. */
__global__ void __launch_bounds__(256) k_eig_intcond_dd(const double* __restrict__ coef,
                                                        const double* __restrict__ xr,
                                                        const double* __restrict__ xi, int64_t N,
                                                        double* __restrict__ out4)
{
    __shared__ double sh[256], sl[256];
    const double* x = blockIdx.x ? xi : xr;
    dd acc{0.0, 0.0};
    if (x)
        for (int64_t q = threadIdx.x; q < N; q += blockDim.x) acc = dd_add(acc, two_prod(coef[q], x[q]));
    sh[threadIdx.x] = acc.h;
    sl[threadIdx.x] = acc.l;
    __syncthreads();
    if (threadIdx.x == 0) {
        dd t{0.0, 0.0};
        for (int i = 0; i < (int)blockDim.x; i++) t = dd_add(t, dd{sh[i], sl[i]});
        out4[2 * blockIdx.x] = t.h;
        out4[2 * blockIdx.x + 1] = t.l;
    }
}
/* its entry of the owner's output: sign * (hi + lo), for the real and the imaginary product */
__global__ void k_eig_intcond_put(const double* __restrict__ in4, double sign, double* yh_r, double* yl_r,
                                  double* yh_i, double* yl_i)
{
    const dd r = two_sum(in4[0], in4[1]), i = two_sum(in4[2], in4[3]);
    *yh_r = sign * r.h;
    *yl_r = sign * r.l;
    if (yh_i) {
        *yh_i = sign * i.h;
        *yl_i = sign * i.l;
    }
}

/* block partials of sum |a - mu B x|^2 (partial[blk]) and sum |a|^2 (partial[gridDim.x + blk]) in
 * complex arithmetic, one pass: r_r = a_r - (mu_r B x_r - mu_i B x_i), r_i = a_i - (mu_r B x_i +
 * mu_i B x_r), the difference in double-double (a = a?h + a?l, the low parts optional; mu_r =
 * mu_rh + mu_rl, the unrounded lambda_r - sigma).  ai = xi = null: a real pair.  Reduced as
 * k_mdot: 64-lane shuffles, block_sum, then k_mdot_final's fixed second stage, so the same input
 * gives the same bits. */
struct ResidualIn {
    const double *ar, *ai, *alr, *ali, *xr, *xi, *B;
    double mu_rh, mu_rl, mu_i;
};
__global__ void __launch_bounds__(256) k_eig_residual(ResidualIn in, int64_t N, double* __restrict__ partial)
{
    __shared__ double sm_r[8], sm_a[8];
    const dd mr{in.mu_rh, in.mu_rl}, mi{in.mu_i, 0.0};
    double sr = 0.0, sa = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        const double b = in.B[q];
        const dd bxr = two_prod(b, in.xr[q]);
        const dd bxi = in.xi ? two_prod(b, in.xi[q]) : dd{0.0, 0.0};
        const dd pr{in.ar[q], in.alr ? in.alr[q] : 0.0};
        const dd pi{in.ai ? in.ai[q] : 0.0, in.ali ? in.ali[q] : 0.0};
        const dd dr = dd_sub(pr, dd_sub(dd_mul(mr, bxr), dd_mul(mi, bxi)));
        const dd di = dd_sub(pi, dd_add(dd_mul(mr, bxi), dd_mul(mi, bxr)));
        const double rr = dr.h + dr.l, ri = di.h + di.l;
        sr += rr * rr + ri * ri;
        sa += pr.h * pr.h + pi.h * pi.h;
    }
    const double tr = block_sum(sr, sm_r);
    const double ta = block_sum(sa, sm_a);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = tr;
        partial[gridDim.x + blockIdx.x] = ta;
    }
}

static int bad_sigma(const char* who)
{
    set_error(std::string(who) + ": the shift sigma must be finite");
    return IEMIC_EINVAL;
}

/* The shift goes into the buffer assemble_jacobian just filled, with ActiveSet::coef_stale set,
 * exactly as theta_jacobian's: the compressed SpMV's stream (gs_refresh) and the next
 * prec_compute read J - sigma B.  At sigma = 0 nothing is launched. */
int shifted_jacobian(iemic_ctx* c, double sigma)
{
    if (!std::isfinite(sigma)) return bad_sigma("iemic_shifted_jacobian");
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    if ((rc = assemble_jacobian(c, c->d_x.p))) return rc;
    if (sigma == 0.0) return 0;
    hipLaunchKernelGGL(k_shift_diag, dim3((unsigned)((c->sub.nloc + 255) / 256), THETA_ROWS), dim3(256), 0,
                       c->stream, c->d_B.p, c->d_val.p, (int64_t)c->sub.own0, (int64_t)c->sub.nloc, sigma);
    HIP_OK(hipGetLastError());
    return 0;
}

int eigs_end(iemic_ctx* c)
{
    Eigs& eg = c->eg;
    eg.V.free();
    eg.t.free();
    eg.w.free();
    eg.lo.free();
    eg.active = eg.m = eg.j = eg.broke = 0;
    return 0;
}

static int eig_drop_p(iemic_ctx* c, const double* w, double* t, int64_t NL)
{
    hipLaunchKernelGGL(k_eig_drop_p, dim3(grid_for(NL)), dim3(256), 0, c->stream, w, t, NL);
    HIP_OK(hipGetLastError());
    return 0;
}

int eigs_begin(iemic_ctx* c, double sigma, int m, uint64_t seed, const iemic_krylov* opt)
{
    if (m < 1) {
        set_error("iemic_eigs_begin: the basis size m must be at least 1");
        return IEMIC_EINVAL;
    }
    if (m > IEMIC_EIGS_MAX_M) {
        set_error("iemic_eigs_begin: the basis size m exceeds IEMIC_EIGS_MAX_M = " +
                  std::to_string(IEMIC_EIGS_MAX_M));
        return IEMIC_EINVAL;
    }
    if (!std::isfinite(sigma)) return bad_sigma("iemic_eigs_begin");
    Eigs& eg = c->eg;
    eigs_end(c);
    int rc = shifted_jacobian(c, sigma);
    if (rc) return rc;
    if (opt->prec > 0 && (rc = prec_compute(c, opt))) return rc;
    const int64_t NE = c->sub.nerows();
    const auto [o, NL, G] = owned(c);
    if (eg.V.alloc((size_t)(m + 1) * NE) || eg.t.alloc(NE) || eg.w.alloc(NE)) {
        eigs_end(c);
        set_error("iemic_eigs_begin: out of device memory for the Arnoldi basis");
        return IEMIC_ENOMEM;
    }
    /* the halo rows of the basis and the work vectors are never written: zero, not garbage */
    if ((rc = dev_zero(c, eg.V.p, (int64_t)(m + 1) * NE))) return rc;
    if ((rc = dev_zero(c, eg.t.p, NE))) return rc;
    if ((rc = dev_zero(c, eg.w.p, NE))) return rc;
    const Sub& s = c->sub;
    hipLaunchKernelGGL(k_eig_start, dim3((unsigned)((s.nloc + 255) / 256)), dim3(256), 0, c->stream, eg.w.p + o,
                       s.n, s.m, s.l, s.jb0, s.ib0, s.nx, (int64_t)s.nloc, seed);
    HIP_OK(hipGetLastError());
    double ww = 0.0;
    if ((rc = eig_drop_p(c, eg.w.p + o, eg.t.p + o, NL))) return rc;
    if ((rc = mdot_host(c, eg.t.p + o, 0, 1, eg.t.p + o, &ww))) return rc;
    const double nrm = sqrt0(ww);
    if (!std::isfinite(nrm) || !(nrm > 0.0)) {
        set_error("iemic_eigs_begin: the start vector has no finite positive norm");
        return IEMIC_ERANGE;
    }
    hipLaunchKernelGGL(k_eig_scale_bmul, dim3(G), dim3(256), 0, c->stream, eg.w.p + o, c->d_B.p + o,
                       1.0 / nrm, eg.V.p + o, eg.t.p + o, NL);
    HIP_OK(hipGetLastError());
    eg.sigma = sigma;
    eg.m = m;
    eg.j = 0;
    eg.broke = 0;
    eg.active = 1;
    return 0;
}

/* w -= sum_i h_i V_i (i < nv) by k_lincomb, 16 basis vectors a launch */
static int eig_subtract(iemic_ctx* c, const double* V, int64_t ldv, int nv, const double* h, double* w, int64_t o,
                        int64_t NL)
{
    for (int i0 = 0; i0 < nv; i0 += 16) {
        LinComb L{};
        L.a = 1.0;
        for (int i = i0; i < std::min(nv, i0 + 16); i++) {
            L.c[L.nv] = -h[i];
            L.X[L.nv] = V + (int64_t)i * ldv + o;
            L.nv++;
        }
        hipLaunchKernelGGL(k_lincomb, dim3(grid_for(NL)), dim3(256), 0, c->stream, L, w + o, NL);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int eigs_step(iemic_ctx* c, const iemic_krylov* opt, double* hcol, iemic_eigs_info* info)
{
    Eigs& eg = c->eg;
    if (!eg.active) {
        set_error("iemic_eigs_step: no run in progress (iemic_eigs_begin)");
        return IEMIC_ESTATE;
    }
    if (eg.broke || eg.j >= eg.m) {
        set_error(eg.broke ? "iemic_eigs_step: the run ended at a breakdown (invariant Krylov space)"
                           : "iemic_eigs_step: all m steps of the run are taken");
        return IEMIC_ESTATE;
    }
    iemic_eigs_info inf{};
    const auto T0 = std::chrono::steady_clock::now();
    const int j = eg.j;
    const int64_t NE = c->sub.nerows();
    const auto [o, NL, G] = owned(c);
    inf.step = j;
    auto t0 = std::chrono::steady_clock::now();
    int rc = krylov_solve(c, eg.t.p, eg.w.p, opt, &inf.solve);
    if (rc) return rc;
    DEV_SYNC(c);
    inf.t_solve_ms = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    double h[IEMIC_EIGS_MAX_M + 2], h2[IEMIC_EIGS_MAX_M + 2];
    /* t is free until the next right-hand side: it holds w without its P rows for the dots */
    double* wq = eg.t.p + o;
    if ((rc = eig_drop_p(c, eg.w.p + o, wq, NL))) return rc;
    if ((rc = mdot_host(c, eg.V.p + o, NE, j + 1, wq, h))) return rc;
    if ((rc = eig_subtract(c, eg.V.p, NE, j + 1, h, eg.w.p, o, NL))) return rc;
    if ((rc = eig_drop_p(c, eg.w.p + o, wq, NL))) return rc;
    if ((rc = mdot_host(c, eg.V.p + o, NE, j + 1, wq, h2))) return rc;
    if ((rc = eig_subtract(c, eg.V.p, NE, j + 1, h2, eg.w.p, o, NL))) return rc;
    double ww = 0.0;
    if ((rc = eig_drop_p(c, eg.w.p + o, wq, NL))) return rc;
    if ((rc = mdot_host(c, wq, 0, 1, wq, &ww))) return rc;
    const double hn = sqrt0(ww);
    double col2 = hn * hn;
    bool finite = std::isfinite(hn);
    for (int i = 0; i <= j; i++) {
        hcol[i] = h[i] + h2[i];
        finite = finite && std::isfinite(hcol[i]);
        col2 += hcol[i] * hcol[i];
    }
    hcol[j + 1] = hn;
    if (!finite) {
        set_error("iemic_eigs_step: non-finite value in the Hessenberg column (operator or solver output)");
        return IEMIC_ERANGE;
    }
    inf.t_orth_ms = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (hn <= 1e-14 * std::sqrt(col2)) {
        inf.breakdown = eg.broke = 1;
    } else {
        hipLaunchKernelGGL(k_eig_scale_bmul, dim3(G), dim3(256), 0, c->stream, eg.w.p + o, c->d_B.p + o,
                           1.0 / hn, eg.V.p + (int64_t)(j + 1) * NE + o, eg.t.p + o, NL);
        HIP_OK(hipGetLastError());
        DEV_SYNC(c);
    }
    inf.t_scale_ms = ms_since(t0);
    eg.j = j + 1;
    inf.t_total_ms = ms_since(T0);
    if (info) *info = inf;
    return inf.solve.converged ? 0 : IEMIC_ENOCONV;
}

template <int P>
static void ritz_launch(iemic_ctx* c, const double* V, int64_t ldv, int j, const double* Yd, const RitzOut& out,
                        int p, int64_t N)
{
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((N + 511) / 512, 2048));
    hipLaunchKernelGGL(k_eig_ritz<P>, dim3(g), dim3(256), 0, c->stream, V, ldv, j, Yd, out, p, N);
}

int eigs_ritz(iemic_ctx* c, const double* V, int64_t ldv, int j, int p, const double* Y, double* const* xs,
              int64_t N)
{
    if (j < 1 || j > IEMIC_EIGS_MAX_M || p < 1 || p > RITZ_MAX_P || !V || !Y || !xs || N < 0) {
        set_error("iemic_eigs_ritz: needs 1 <= j <= IEMIC_EIGS_MAX_M basis vectors and 1 <= p <= 16 outputs");
        return IEMIC_EINVAL;
    }
    const int P = p <= 1 ? 1 : p <= 2 ? 2 : p <= 4 ? 4 : p <= 8 ? 8 : 16;
    /* Y padded to P columns, through the pinned staging area */
    std::vector<double> yp((size_t)j * P, 0.0);
    for (int i = 0; i < j; i++)
        for (int q = 0; q < p; q++) yp[(size_t)i * P + q] = Y[(size_t)i * p + q];
    int rc = upload_coeffs(c, yp.data(), j * P);
    if (rc) return rc;
    const double* Yd = c->d_hbuf.p + RED_ROWS;
    RitzOut out{};
    for (int q = 0; q < p; q++) {
        if (!xs[q]) {
            set_error("iemic_eigs_ritz: null output vector");
            return IEMIC_EINVAL;
        }
        out.x[q] = xs[q];
    }
    switch (P) {
    case 1: ritz_launch<1>(c, V, ldv, j, Yd, out, p, N); break;
    case 2: ritz_launch<2>(c, V, ldv, j, Yd, out, p, N); break;
    case 4: ritz_launch<4>(c, V, ldv, j, Yd, out, p, N); break;
    case 8: ritz_launch<8>(c, V, ldv, j, Yd, out, p, N); break;
    default: ritz_launch<16>(c, V, ldv, j, Yd, out, p, N); break;
    }
    HIP_OK(hipGetLastError());
    DEV_SYNC(c);   /* the staging area is free again on return */
    return 0;
}

template <int P>
static void compress_launch(iemic_ctx* c, double* V, int64_t ldv, int j, const double* Qd, int p, int64_t N)
{
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((N + 511) / 512, 2048));
    hipLaunchKernelGGL(k_eig_compress<P>, dim3(g), dim3(256), 0, c->stream, V, ldv, j, Qd, p, N);
}

int eigs_compress(iemic_ctx* c, double* V, int64_t ldv, int j, int p, const double* Q, int64_t N)
{
    if (j < 2 || j > IEMIC_EIGS_MAX_M || p < 1 || p > RITZ_MAX_P || p >= j || !V || !Q || N < 0 || ldv < N) {
        set_error("eigs_compress: needs 1 <= p < j <= IEMIC_EIGS_MAX_M, p <= 16 and ldv >= N");
        return IEMIC_EINVAL;
    }
    const int P = p <= 1 ? 1 : p <= 2 ? 2 : p <= 4 ? 4 : p <= 8 ? 8 : 16;
    /* Q padded to P columns, through the pinned staging area */
    std::vector<double> qp((size_t)j * P, 0.0);
    for (int i = 0; i < j; i++)
        for (int q = 0; q < p; q++) qp[(size_t)i * P + q] = Q[(size_t)i * p + q];
    int rc = upload_coeffs(c, qp.data(), j * P);
    if (rc) return rc;
    const double* Qd = c->d_hbuf.p + RED_ROWS;
    switch (P) {
    case 1: compress_launch<1>(c, V, ldv, j, Qd, p, N); break;
    case 2: compress_launch<2>(c, V, ldv, j, Qd, p, N); break;
    case 4: compress_launch<4>(c, V, ldv, j, Qd, p, N); break;
    case 8: compress_launch<8>(c, V, ldv, j, Qd, p, N); break;
    default: compress_launch<16>(c, V, ldv, j, Qd, p, N); break;
    }
    HIP_OK(hipGetLastError());
    DEV_SYNC(c);   /* the staging area is free again on return */
    return 0;
}

/* Thick restart: A V_j = V_j G + v_{j+1} g^T becomes A V' = V' S + v_{j+1} b^T with V' = V_j Q,
 * S = Q^T G Q and b = Q^T g, for Q whose span is invariant under G (the caller's algebra).  The
 * next right-hand side is rebuilt from the moved vector: iemic_eigs_ritz and
 * iemic_eigs_residual may have used the work vectors since the last step. */
int eigs_restart(iemic_ctx* c, int p, const double* Q)
{
    Eigs& eg = c->eg;
    if (!eg.active) {
        set_error("iemic_eigs_restart: no run in progress (iemic_eigs_begin)");
        return IEMIC_ESTATE;
    }
    if (eg.broke) {
        set_error("iemic_eigs_restart: the run ended at a breakdown (invariant Krylov space)");
        return IEMIC_ESTATE;
    }
    const int j = eg.j;
    if (p < 1) {
        set_error("iemic_eigs_restart: p must be at least 1");
        return IEMIC_EINVAL;
    }
    if (p > RITZ_MAX_P) {
        set_error("iemic_eigs_restart: p exceeds 16 (one compression pass)");
        return IEMIC_EINVAL;
    }
    if (p >= j) {
        set_error("iemic_eigs_restart: p must be smaller than the number of steps taken, j = " + std::to_string(j));
        return IEMIC_EINVAL;
    }
    if (!Q) {
        set_error("iemic_eigs_restart: Q is null");
        return IEMIC_EINVAL;
    }
    for (int i = 0; i < j * p; i++)
        if (!std::isfinite(Q[i])) {
            set_error("iemic_eigs_restart: non-finite entry in Q");
            return IEMIC_EINVAL;
        }
    const int64_t NE = c->sub.nerows();
    const auto [o, NL, G] = owned(c);
    int rc = eigs_compress(c, eg.V.p + o, NE, j, p, Q, NL);
    if (rc) return rc;
    /* t = B v_p; w takes the copy k_eig_scale_bmul writes (the next solve overwrites it) */
    hipLaunchKernelGGL(k_eig_scale_bmul, dim3(G), dim3(256), 0, c->stream, eg.V.p + (int64_t)p * NE + o,
                       c->d_B.p + o, 1.0, eg.w.p + o, eg.t.p + o, NL);
    HIP_OK(hipGetLastError());
    DEV_SYNC(c);
    eg.j = p;
    return 0;
}

static int residual_sums(iemic_ctx* c, const ResidualIn& in, int64_t N, double* out2)
{
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((N + 255) / 256, RED_BLOCKS));
    hipLaunchKernelGGL(k_eig_residual, dim3(nb), dim3(256), 0, c->stream, in, N, c->d_part.p);
    hipLaunchKernelGGL(k_mdot_final, dim3(2), dim3(256), 0, c->stream, c->d_part.p, nb, 2, c->d_hbuf.p);
    HIP_OK(hipGetLastError());
    int rc = allreduce_sum(c, c->d_hbuf.p, 2);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(c->h_red, c->d_hbuf.p, sizeof(double) * 2, hipMemcpyDeviceToHost, c->stream));
    DEV_SYNC(c);
    out2[0] = c->h_red[0];
    out2[1] = c->h_red[1];
    return 0;
}

int eigs_residual_sums(iemic_ctx* c, const double* ar, const double* ai, const double* xr, const double* xi,
                       const double* B, double mu_r, double mu_i, int64_t N, double* out2)
{
    return residual_sums(c, ResidualIn{ar, ai, nullptr, nullptr, xr, xi, B, mu_r, 0.0, mu_i}, N, out2);
}

int eigs_residual(iemic_ctx* c, double lam_re, double lam_im, double* xr, double* xi, double* out2)
{
    Eigs& eg = c->eg;
    if (!eg.active) {
        set_error("iemic_eigs_residual: no run in progress (iemic_eigs_begin)");
        return IEMIC_ESTATE;
    }
    if (!xr || !out2) return IEMIC_EINVAL;
    if (!c->jac_valid) {
        set_error("iemic_eigs_residual: no Jacobian assembled");
        return IEMIC_ESTATE;
    }
    const int64_t NE = c->sub.nerows(), nloc = c->sub.nloc;
    const auto [o, NL, G] = owned(c);
    if (eg.lo.reserve((size_t)2 * NE)) {
        set_error("iemic_eigs_residual: out of device memory for the products' low parts");
        return IEMIC_ENOMEM;
    }
    int rc = halo_exchange(c, xr, 1);
    if (rc) return rc;
    if (xi && (rc = halo_exchange(c, xi, 1))) return rc;
    double *ahr = c->d_tmp1.p, *ahi = c->d_tmp2.p, *alr = eg.lo.p, *ali = eg.lo.p + NE;
    const unsigned grid = (unsigned)((nloc + 255) / 256);
    hipLaunchKernelGGL(k_spmv_dd, dim3(grid), dim3(256), 0, c->stream, sub_lay(c->sub), c->d_val.p, xr, ahr, alr,
                       (int64_t)c->sub.own0, nloc);
    if (xi)
        hipLaunchKernelGGL(k_spmv_dd, dim3(grid), dim3(256), 0, c->stream, sub_lay(c->sub), c->d_val.p, xi, ahi, ali,
                           (int64_t)c->sub.own0, nloc);
    HIP_OK(hipGetLastError());
    if (c->su.rowintcon_ref >= 0) {
        /* the dense row, as spmv_intcond: intSign * coeff . x summed over the ranks (hi and lo
         * parts each), into the owner's entry */
        double* d4 = c->d_hbuf.p + 2;
        hipLaunchKernelGGL(k_eig_intcond_dd, dim3(2), dim3(256), 0, c->stream, c->d_intc.p + o, xr + o,
                           xi ? xi + o : nullptr, NL, d4);
        HIP_OK(hipGetLastError());
        if ((rc = allreduce_sum(c, d4, 4))) return rc;
        if (c->rowintcon >= 0) {
            const int64_t q = c->rowintcon;
            hipLaunchKernelGGL(k_eig_intcond_put, dim3(1), dim3(1), 0, c->stream, d4, (double)c->cfg.int_sign,
                               ahr + q, alr + q, xi ? ahi + q : nullptr, xi ? ali + q : nullptr);
            HIP_OK(hipGetLastError());
        }
    }
    /* mu = lambda - sigma unrounded: two_sum on the host */
    const double mh = lam_re - eg.sigma, bb = mh - lam_re;
    const double ml = (lam_re - (mh - bb)) + (-eg.sigma - bb);
    double s[2];
    rc = residual_sums(c, ResidualIn{ahr + o, xi ? ahi + o : nullptr, alr + o, xi ? ali + o : nullptr, xr + o,
                                     xi ? xi + o : nullptr, c->d_B.p + o, mh, ml, lam_im},
                       NL, s);
    if (rc) return rc;
    out2[0] = sqrt0(s[0]);
    out2[1] = sqrt0(s[1]);
    return 0;
}

}  // namespace iemic
