/*
 * ts_mg.hip -- T/S aggregation multigrid of the block Gauss-Seidel preconditioner
 * (prec_gs.hip's overview, step 6 with ts_mg > 0).
 *
 * The T/S block is an advection-diffusion operator whose smooth error modes Gauss-Seidel
 * sweeps barely touch.  Its coarse spaces aggregate 2x2 horizontal neighbours over the
 * full depth (each level is again an n x m x l grid with the fine coupling pattern:
 * 6 same-variable face couplings, T<->S at k-1/k+1, a 2x2 cell block), built by Galerkin
 * summation with piecewise-constant transfers.  Aggregates stay inside a latitude band.
 * One V-cycle: z-line relaxation by horizontal colour on every level (colours forward
 * before the coarse correction, backward after it), a dense inverse on the coarsest.
 *
 * Level layout (level 0 included, packed once per Jacobian): columns k-contiguous,
 *     cell = ((jl + hj) * n + i) * l + k,
 * so the P lanes of a column (lane = level k) read one contiguous run of every array and
 * a horizontal neighbour is again one whole run (one 128-B line per array at l = 16);
 * with hj = 1 halo row on each side and hi = 1 halo column (the row width is n + 2 hi) on
 * level 0 when the y / x direction is split over ranks (refreshed by exchanges).
 * The z-lines are factorised at set-up (block Thomas, k_mg_fac: F = -A'^-1 B, A'^-1,
 * Cp = A'^-1 C per cell), so a relaxation is two affine parallel scans over the lanes
 * without a division.  Launch fusion (the apply is latency-bound):
 *   - the T/S right-hand side and the first colour of level 0 (k_mg_entry),
 *   - each restriction and the first colour of the coarse level (k_mg_rc): from a zero
 *     iterate that colour's lines see zero neighbours,
 *   - the prolongation into the first post-smoothing colour (k_mg_zl, corr): a line solve
 *     never reads its own old value, so the coarse correction is only needed on the
 *     neighbours not yet relaxed, and it is added where they are read,
 *   - after one forward sweep from zero with two colours, the residual of the last colour
 *     is zero and that of the first is -H z(last colour) (restriction shortcut: 16 instead
 *     of 72 doubles per fine-cell pair),
 *   - the last colour launches of the final level-0 sweep write z(T, S) straight into the
 *     preconditioner output.
 * This unit is the apply (the V-cycle kernels and their driver); the set-up -- levels,
 * Galerkin operators, line factors, the coarsest inverse -- is ts_mg_setup.hip. */
#include <algorithm>
#include <vector>

#include "ts_mg_internal.h"

namespace iemic {

namespace {

/* 3b. y = X b (X row-major nr x nc), one wavefront per row */
__global__ void __launch_bounds__(256) k_gemv(const double* __restrict__ X, int nr, int nc,
                                              const double* __restrict__ b, double* __restrict__ y)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= nr) return;
    const double* xr = X + (int64_t)row * nc;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int c = lane;
    for (; c + 192 < nc; c += 256) {
        s0 += xr[c] * b[c];
        s1 += xr[c + 64] * b[c + 64];
        s2 += xr[c + 128] * b[c + 128];
        s3 += xr[c + 192] * b[c + 192];
    }
    for (; c < nc; c += 64) s0 += xr[c] * b[c];
    double s = (s0 + s1) + (s2 + s3);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) y[row] = s;
}

/* y = X b for a dense row-major N x N inverse (N <= 64 NL), one wave per row: every load
 * of the row is issued before the first multiply, b staged in LDS, eight independent
 * accumulators and a fixed shuffle tree (deterministic) */
template <int NL>
__global__ void __launch_bounds__(256) k_gemv_w(const double* __restrict__ X, int N, const double* __restrict__ b,
                                                double* __restrict__ y)
{
    __shared__ double vb[64 * NL];
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const double* A = X + (size_t)(r < N ? r : 0) * N;
    double a[NL];
#pragma unroll
    for (int u = 0; u < NL; u++) {
        const int c = lane + 64 * u;
        a[u] = c < N ? __builtin_nontemporal_load(A + c) : 0.0;
    }
    for (int c = threadIdx.x; c < N; c += 256) vb[c] = b[c];
    __syncthreads();
    if (r >= N) return;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < NL; u++) {
        const int c = lane + 64 * u;
        if (c < N) acc[u & 7] += a[u] * vb[c];
    }
    double v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) y[r] = v;
}

/* the same neighbour, branch-free for the apply: outside the level's (visible) band the
 * cell itself (every coupling to outside is 0: k_ts_compact / k_mg_galerkin), so the loads
 * of all neighbours issue together */
__device__ __forceinline__ void mg_nbc(const TsLev& V, int q, int& i, int& jl, int& k)
{
    switch (q) {
    case 0: i = i > -V.visi ? i - 1 : (V.periodic ? V.n - 1 : i); break;
    case 1: i = i < V.n - 1 + V.visi ? i + 1 : (V.periodic ? 0 : i); break;
    case 2: jl = jl > -V.vis ? jl - 1 : jl; break;
    case 3: jl = jl < V.mb - 1 + V.vis ? jl + 1 : jl; break;
    case 4: k = k > 0 ? k - 1 : k; break;
    default: k = k < V.l - 1 ? k + 1 : k; break;
    }
}
/* off-diagonal part of row (T, S) of cell (i,jl,k) applied to the iterate */
__device__ __forceinline__ void mg_offmul(const TsLev& V, int i, int jl, int k, int64_t c,
                                          double& at, double& as)
{
    const int64_t cs = V.cstr;
    at = as = 0.0;
#pragma unroll
    for (int q = 0; q < 6; q++) {
        int ii = i, jj = jl, kk = k;
        mg_nbc(V, q, ii, jj, kk);
        const int64_t nc = mg_cell(V, ii, jj, kk);
        at += V.off[(int64_t)q * cs + c] * V.z[nc];
        as += V.off[(int64_t)(8 + q) * cs + c] * V.z[cs + nc];
        if (q == 4) {
            at += V.off[6 * cs + c] * V.z[cs + nc];
            as += V.off[14 * cs + c] * V.z[nc];
        } else if (q == 5) {
            at += V.off[7 * cs + c] * V.z[cs + nc];
            as += V.off[15 * cs + c] * V.z[nc];
        }
    }
}
/* colour of water column (i, jl): parity of i + j (global j on level 0); on a periodic
 * level with odd n the wrap pair (n-1, 0) would share a colour, so column n-1 gets 2 / 3 */
__host__ __device__ __forceinline__ int mg_ncolour(const TsLev& V) { return (V.periodic && (V.n & 1)) ? 4 : 2; }
__device__ __forceinline__ int mg_lcolour(const TsLev& V, int i, int jl)
{
    if (V.periodic && (V.n & 1) && i == V.n - 1) return 2 + ((jl + V.jpar) & 1);
    return (i + jl + V.jpar) & 1;
}
/* g-th owned column of a colour: row jl holds i = 2h + ((colour + jl + jpar) & 1), h <
 * ceil(n'/2), n' = n - 1 on an odd periodic level (whose last column has colour 2 or 3).
 * hr (bands' level 0): the rows run from -1 to mb, the halo row -1 when hr & 1, mb when
 * hr & 2 (the parity of a negative jl is that of the global row too) */
__device__ __forceinline__ bool mg_column(const TsLev& V, int colour, int g, int& i, int& jl, int hr = 0)
{
    const int np = (V.periodic && (V.n & 1)) ? V.n - 1 : V.n;
    const int rows = V.mb + (hr ? 2 : 0), j0 = hr ? -1 : 0;
    if (colour < 2) {
        const int per_row = (np + 1) / 2;
        if (g >= per_row * rows) return false;
        jl = g / per_row + j0;
        i = 2 * (g % per_row) + ((colour + jl + V.jpar) & 1);
    } else {
        if (g >= rows) return false;
        jl = g + j0;
        i = V.n - 1;
        if (((jl + V.jpar) & 1) != colour - 2) return false;
    }
    if ((jl < 0 && !(hr & 1)) || (jl >= V.mb && !(hr & 2))) return false;
    return i < np || colour >= 2;
}
__host__ __device__ __forceinline__ int64_t mg_columns_of(const TsLev& V, int colour, int hr = 0)
{
    const int np = (V.periodic && (V.n & 1)) ? V.n - 1 : V.n;
    const int rows = V.mb + (hr ? 2 : 0);
    return colour < 2 ? (int64_t)((np + 1) / 2) * rows : rows;
}

/* Line solve of one column, lane = level k (< l when on): g = A'^-1 r, then the forward
 * recurrence dp_k = F_k dp_{k-1} + g_k and the backward x_k = dp_k - Cp_k x_{k+1} as affine
 * Hillis-Steele scans over the P lanes (log2 P shuffle steps of 2x2 algebra each, no
 * division: the pivots were inverted at set-up).  The factor loads are issued first. */
/* the 12 line factors of a lane (0 when !on), loadable ahead of the right-hand side */
struct LineFac {
    double a0, a1, a2, a3, i0, i1, i2, i3, q0, q1, q2, q3;
};
__device__ __forceinline__ LineFac line_fac(const double* __restrict__ f, int64_t cs, bool on)
{
    LineFac F{};
    if (on) {
        F.a0 = f[0]; F.a1 = f[cs]; F.a2 = f[2 * cs]; F.a3 = f[3 * cs];
        F.i0 = f[4 * cs]; F.i1 = f[5 * cs]; F.i2 = f[6 * cs]; F.i3 = f[7 * cs];
        F.q0 = -f[8 * cs]; F.q1 = -f[9 * cs]; F.q2 = -f[10 * cs]; F.q3 = -f[11 * cs];
    }
    return F;
}
template <int P>
__device__ __forceinline__ void line_run(const LineFac& F, int k, double rt, double rs, double& xt, double& xs);
template <int P>
__device__ __forceinline__ void line_solve(const double* __restrict__ f, int64_t cs, bool on, int k,
                                           double rt, double rs, double& xt, double& xs)
{
    line_run<P>(line_fac(f, cs, on), k, rt, rs, xt, xs);
}
template <int P>
__device__ __forceinline__ void line_run(const LineFac& F, int k, double rt, double rs, double& xt, double& xs)
{
    double a0 = F.a0, a1 = F.a1, a2 = F.a2, a3 = F.a3;
    const double i0 = F.i0, i1 = F.i1, i2 = F.i2, i3 = F.i3;
    double q0 = F.q0, q1 = F.q1, q2 = F.q2, q3 = F.q3;
    double ct = i0 * rt + i1 * rs, cv = i2 * rt + i3 * rs;
#pragma unroll
    for (int d = 1; d < P; d <<= 1) {
        const double b0 = __shfl_up(a0, d, P), b1 = __shfl_up(a1, d, P);
        const double b2 = __shfl_up(a2, d, P), b3 = __shfl_up(a3, d, P);
        const double dt = __shfl_up(ct, d, P), dv = __shfl_up(cv, d, P);
        if (k >= d) {
            const double nt = ct + (a0 * dt + a1 * dv), nv = cv + (a2 * dt + a3 * dv);
            const double n0 = a0 * b0 + a1 * b2, n1 = a0 * b1 + a1 * b3;
            const double n2 = a2 * b0 + a3 * b2, n3 = a2 * b1 + a3 * b3;
            ct = nt; cv = nv; a0 = n0; a1 = n1; a2 = n2; a3 = n3;
        }
    }
#pragma unroll
    for (int d = 1; d < P; d <<= 1) {
        const double b0 = __shfl_down(q0, d, P), b1 = __shfl_down(q1, d, P);
        const double b2 = __shfl_down(q2, d, P), b3 = __shfl_down(q3, d, P);
        const double dt = __shfl_down(ct, d, P), dv = __shfl_down(cv, d, P);
        if (k + d < P) {
            const double nt = ct + (q0 * dt + q1 * dv), nv = cv + (q2 * dt + q3 * dv);
            const double n0 = q0 * b0 + q1 * b2, n1 = q0 * b1 + q1 * b3;
            const double n2 = q2 * b0 + q3 * b2, n3 = q2 * b1 + q3 * b3;
            ct = nt; cv = nv; q0 = n0; q1 = n1; q2 = n2; q3 = n3;
        }
    }
    xt = ct;
    xs = cv;
}

/* z-line relaxation of one colour: every column of it solves its 2x2-block tridiagonal T/S
 * system along k with the horizontal couplings taken from the current iterate.  corr: the
 * first post-smoothing colour launch, neighbours not yet relaxed in this sweep (smaller
 * colour) read with their aggregate's coarse correction C.z added.  zout (level 0, final
 * sweep): the active T/S rows of the preconditioner output (ext layout) get the result. */
/* the line solve of column (i, jl) of the given colour from the current iterate (level k of
 * this lane; on: k < l); corr: neighbours of a smaller colour read with their aggregate's
 * coarse correction C.z added.  Returns the cell index (0 when !on). */
template <int P>
__device__ __forceinline__ int64_t zl_col(const TsLev& V, int i, int jl, int k, bool on, int colour,
                                          const TsLev& C, int corr, double& xt, double& xs)
{
    const int64_t cs = V.cstr;
    int64_t c = 0;
    double rt = 0.0, rs = 0.0;
    if (on) {
        c = mg_cell(V, i, jl, k);
        rt = V.b[c];
        rs = V.b[cs + c];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            int ii = i, jj = jl, kk = k;
            mg_nbc(V, q, ii, jj, kk);
            const int64_t nc = mg_cell(V, ii, jj, kk);
            double zt = V.z[nc], zs = V.z[cs + nc];
            if (corr && mg_lcolour(V, ii, jj) < colour) {
                const int64_t p = mg_cell(C, ii >> 1, jj >> 1, k);
                zt += C.z[p];
                zs += C.z[C.cstr + p];
            }
            rt -= V.off[(int64_t)q * cs + c] * zt;
            rs -= V.off[(int64_t)(8 + q) * cs + c] * zs;
        }
    }
    line_solve<P>(V.fac + c, cs, on, k, rt, rs, xt, xs);
    return c;
}

template <int P>
__device__ __forceinline__ void zl_one(const TsLev& V, int colour, int g, int k, const TsLev& C, int corr,
                                       double* __restrict__ zout, int hr)
{
    int i, jl;
    if (!mg_column(V, colour, g, i, jl, hr)) return;       /* whole column groups exit */
    const int64_t cs = V.cstr;
    const bool on = k < V.l;
    double xt, xs;
    const int64_t c = zl_col<P>(V, i, jl, k, on, colour, C, corr, xt, xs);
    if (!on) return;
    V.z[c] = xt;
    V.z[cs + c] = xs;
    if (zout && jl >= 0 && jl < V.mb) {
        const int64_t e = NUN * ((((int64_t)jl + HALO) * V.l + k) * V.n + i);
        if (V.diag[c] != 0.0) zout[e + TT] = xt;
        if (V.diag[3 * cs + c] != 0.0) zout[e + SS] = xs;
    }
}
template <int P>
__global__ void __launch_bounds__(256) k_mg_zl(TsLev V, int colour, TsLev C, int corr,
                                              double* __restrict__ zout, int hr)
{
    zl_one<P>(V, colour, (blockIdx.x * blockDim.x + threadIdx.x) / P, threadIdx.x % P, C, corr, zout, hr);
}

/* Restriction F -> C (coarse rhs = sum of the children's residuals, fixed order
 * (c00 + c10) + (c01 + c11)) and, when relax, the coarse level's colour-0 lines from the
 * zero iterate (zero neighbours), the other coarse cells' iterate set to 0.  P lanes per
 * coarse column (lane = level k), every lane reads its four children's level k.
 * shortcut: F was relaxed once, colour 0 then 1, from a zero iterate, so the residual of
 * colour 1 is 0 and that of colour 0 is -H z (its horizontal neighbours). */
template <int P>
__device__ __forceinline__ void rc_one(const TsLev& F, const TsLev& C, int g, int k, int shortcut, int relax)
{
    if (g >= C.n * C.mb) return;
    const int I = g % C.n, J = g / C.n;
    const bool on = k < C.l;
    const int64_t fs = F.cstr, cs = C.cstr;
    const int64_t t = on ? mg_cell(C, I, J, k) : 0;
    double bt = 0.0, bs = 0.0;
    if (shortcut) {
        /* the two colour-0 children (a + b + jpar even), clamped into the level and weighted
         * 0 outside it, so that all their loads issue at once; (c00 + c10) + (c01 + c11)
         * with the colour-1 terms 0 is their plain sum */
        double rr[2][2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int a = h ? 1 - F.jpar : F.jpar, b = h;
            const int i0 = 2 * I + a, j0 = 2 * J + b;
            const bool in = on && i0 < F.n && j0 < F.mb;
            const int i = min(i0, F.n - 1), jl = min(j0, F.mb - 1), kc = on ? k : 0;
            const int64_t c = mg_cell(F, i, jl, kc);
            double at = 0.0, as = 0.0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                int ii = i, jj = jl, kk = kc;
                mg_nbc(F, q, ii, jj, kk);
                const int64_t nc = mg_cell(F, ii, jj, kk);
                at += F.off[(int64_t)q * fs + c] * F.z[nc];
                as += F.off[(int64_t)(8 + q) * fs + c] * F.z[fs + nc];
            }
            rr[h][0] = in ? -at : 0.0;
            rr[h][1] = in ? -as : 0.0;
        }
        bt = rr[0][0] + rr[1][0];
        bs = rr[0][1] + rr[1][1];
    } else if (on) {
        double r[4][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
#pragma unroll
        for (int ch = 0; ch < 4; ch++) {
            const int i = 2 * I + (ch & 1), jl = 2 * J + (ch >> 1);
            if (i >= F.n || jl >= F.mb) continue;
            const int64_t c = mg_cell(F, i, jl, k);
            double at, as;
            mg_offmul(F, i, jl, k, c, at, as);
            const double zt = F.z[c], zs = F.z[fs + c];
            at += F.diag[c] * zt + F.diag[fs + c] * zs;
            as += F.diag[2 * fs + c] * zt + F.diag[3 * fs + c] * zs;
            r[ch][0] = F.b[c] - at;
            r[ch][1] = F.b[fs + c] - as;
        }
        bt = (r[0][0] + r[1][0]) + (r[2][0] + r[3][0]);
        bs = (r[0][1] + r[1][1]) + (r[2][1] + r[3][1]);
    }
    if (on) {
        C.b[t] = bt;
        C.b[cs + t] = bs;
    }
    if (!relax) return;
    if (mg_lcolour(C, I, J) == 0) {
        double xt, xs;
        line_solve<P>(C.fac + t, cs, on, k, bt, bs, xt, xs);
        if (on) {
            C.z[t] = xt;
            C.z[cs + t] = xs;
        }
    } else if (on) {
        C.z[t] = 0.0;
        C.z[cs + t] = 0.0;
    }
}
template <int P>
__global__ void __launch_bounds__(256) k_mg_rc(TsLev F, TsLev C, int shortcut, int relax)
{
    rc_one<P>(F, C, (blockIdx.x * blockDim.x + threadIdx.x) / P, threadIdx.x % P, shortcut, relax);
}

/* ---- fused coarse-level visits (two colours, no halos, one sweep): one launch per 2 x 2
 * aggregate instead of two dependent launches, each workgroup recomputing the colour-1
 * lines its aggregate's colour-0 cells border (10 line solves for 2 + 2 outputs; the
 * coarse levels are latency-bound, their arrays L2-resident).  Groups of P lanes: g < 8
 * the line of neighbour q = g & 3 of colour-0 child h = g >> 2, g = 8, 9 the aggregate's
 * own colour-1 children.  The arithmetic is that of the unfused launches in the source,
 * operation for operation (the sums in the same order), but this unit is compiled with
 * floating-point contraction on, and the compiler forms its fused multiply-adds kernel by
 * kernel: the iterates of the two routes agree to rounding, not bit for bit (measured on
 * 8x8x40, P = 64: 560 of 15360 entries of z differ, by at most 3e-14; none at P = 16;
 * tests/test_gpu_ts_mg.py test_fused_equals_unfused holds the pair to the 1e-8 bar). */
template <int P>
__device__ __forceinline__ void mg_child0(const TsLev& F, int I, int J, int h, int& i, int& jl, bool& in)
{
    const int a = h ? 1 - F.jpar : F.jpar;          /* (a + h + jpar) even: colour 0 */
    in = 2 * I + a < F.n && 2 * J + h < F.mb;
    i = min(2 * I + a, F.n - 1);
    jl = min(2 * J + h, F.mb - 1);
}

/* down leg at level F (first visit, colour 0 relaxed from zero): colour-1 lines, the
 * restriction of the residual (zero on colour 1, -H z on colour 0: k_mg_rc's shortcut) and,
 * when relax, the coarse level's colour-0 lines from zero -- k_mg_zl(colour 1) + k_mg_rc */
template <int P>
__global__ void __launch_bounds__(10 * P) k_mg_dn(TsLev F, TsLev C, int relax)
{
    __shared__ double xv[8][2][P];
    const int g = threadIdx.x / P, k = threadIdx.x % P;
    const int I = blockIdx.x % C.n, J = blockIdx.x / C.n;
    const bool on = k < F.l;
    const int64_t fs = F.cstr, cs = C.cstr;
    const int64_t t = on ? mg_cell(C, I, J, k) : 0;
    /* group 0's operands of the restriction and the coarse line, loaded before the lines */
    double po[2][8];
    LineFac cf{};
    if (g == 0) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            int i, jl;
            bool in;
            mg_child0<P>(F, I, J, h, i, jl, in);
            const int64_t c = mg_cell(F, i, jl, on ? k : 0);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                po[h][q] = F.off[(int64_t)q * fs + c];
                po[h][4 + q] = F.off[(int64_t)(8 + q) * fs + c];
            }
        }
        cf = line_fac(C.fac + t, cs, on && relax && mg_lcolour(C, I, J) == 0);
    }
    if (g < 8) {
        const int h = g >> 2, q = g & 3;
        int i, jl;
        bool in;
        mg_child0<P>(F, I, J, h, i, jl, in);
        double xt = 0.0, xs = 0.0;
        if (in) {
            int ii = i, jj = jl, kk = on ? k : 0;
            mg_nbc(F, q, ii, jj, kk);
            if (ii == i && jj == jl) {                 /* clamped: the child itself, weight 0 */
                if (on) {
                    const int64_t c = mg_cell(F, i, jl, k);
                    xt = F.z[c];
                    xs = F.z[fs + c];
                }
            } else {
                zl_col<P>(F, ii, jj, k, on, 1, F, 0, xt, xs);
            }
        }
        xv[g][0][k] = xt;
        xv[g][1][k] = xs;
    } else {
        const int h = g - 8, a = h ? F.jpar : 1 - F.jpar;   /* colour 1 */
        const int i = 2 * I + a, jl = 2 * J + h;
        if (i < F.n && jl < F.mb) {
            double xt, xs;
            const int64_t c = zl_col<P>(F, i, jl, k, on, 1, F, 0, xt, xs);
            if (on) {
                F.z[c] = xt;
                F.z[fs + c] = xs;
            }
        }
    }
    __syncthreads();
    if (g != 0) return;
    double rr[2][2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        int i, jl;
        bool in;
        mg_child0<P>(F, I, J, h, i, jl, in);
        double at = 0.0, as = 0.0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            at += po[h][q] * xv[4 * h + q][0][k];
            as += po[h][4 + q] * xv[4 * h + q][1][k];
        }
        rr[h][0] = (on && in) ? -at : 0.0;
        rr[h][1] = (on && in) ? -as : 0.0;
    }
    const double bt = rr[0][0] + rr[1][0], bs = rr[0][1] + rr[1][1];
    if (on) {
        C.b[t] = bt;
        C.b[cs + t] = bs;
    }
    if (!relax) return;
    if (mg_lcolour(C, I, J) == 0) {
        double xt, xs;
        line_run<P>(cf, k, bt, bs, xt, xs);
        if (on) {
            C.z[t] = xt;
            C.z[cs + t] = xs;
        }
    } else if (on) {
        C.z[t] = 0.0;
        C.z[cs + t] = 0.0;
    }
}

/* up leg at level F (one sweep, colours 1 then 0): the colour-1 lines with the coarse
 * correction C.z added to their colour-0 neighbours, then the colour-0 lines from the new
 * colour-1 values -- k_mg_zl(1, corr) + k_mg_zl(0); the result goes to zu (not F.z, which
 * the neighbouring workgroups still read) */
template <int P>
__global__ void __launch_bounds__(10 * P) k_mg_up(TsLev F, TsLev C, double* __restrict__ zu)
{
    __shared__ double xv[8][2][P];
    const int g = threadIdx.x / P, k = threadIdx.x % P;
    const int I = blockIdx.x % C.n, J = blockIdx.x / C.n;
    const bool on = k < F.l;
    const int64_t fs = F.cstr;
    /* groups 0, 1: their colour-0 child's operands, loaded before the colour-1 lines */
    int64_t c0 = 0;
    bool in0 = false;
    double b0t = 0.0, b0s = 0.0, po[8];
    LineFac ff{};
    if (g < 2) {
        int i, jl;
        mg_child0<P>(F, I, J, g, i, jl, in0);
        if (in0 && on) {
            c0 = mg_cell(F, i, jl, k);
            b0t = F.b[c0];
            b0s = F.b[fs + c0];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                po[q] = F.off[(int64_t)q * fs + c0];
                po[4 + q] = F.off[(int64_t)(8 + q) * fs + c0];
            }
        }
        ff = line_fac(F.fac + c0, fs, in0 && on);
    }
    if (g < 8) {
        const int h = g >> 2, q = g & 3;
        int i, jl;
        bool in;
        mg_child0<P>(F, I, J, h, i, jl, in);
        double xt = 0.0, xs = 0.0;
        if (in) {
            int ii = i, jj = jl, kk = on ? k : 0;
            mg_nbc(F, q, ii, jj, kk);
            if (ii == i && jj == jl) {                 /* clamped: the child's old value, weight 0 */
                if (on) {
                    const int64_t c = mg_cell(F, i, jl, k);
                    xt = F.z[c];
                    xs = F.z[fs + c];
                }
            } else {
                zl_col<P>(F, ii, jj, k, on, 1, C, 1, xt, xs);
            }
        }
        xv[g][0][k] = xt;
        xv[g][1][k] = xs;
    } else {
        const int h = g - 8, a = h ? F.jpar : 1 - F.jpar;
        const int i = 2 * I + a, jl = 2 * J + h;
        if (i < F.n && jl < F.mb) {
            double xt, xs;
            const int64_t c = zl_col<P>(F, i, jl, k, on, 1, C, 1, xt, xs);
            if (on) {
                zu[c] = xt;
                zu[fs + c] = xs;
            }
        }
    }
    __syncthreads();
    if (g >= 2 || !in0) return;                        /* whole groups */
    /* colour-0 child h = g: its line from the four new colour-1 neighbours (k_mg_zl colour 0) */
    const int h = g;
    double rt = b0t, rs = b0s;
    if (on) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            rt -= po[q] * xv[4 * h + q][0][k];
            rs -= po[4 + q] * xv[4 * h + q][1][k];
        }
    }
    double xt, xs;
    line_run<P>(ff, k, rt, rs, xt, xs);
    if (on) {
        zu[c0] = xt;
        zu[fs + c0] = xs;
    }
}

/* Level-0 entry: the T/S right-hand side rr_TS - A_TS,D z_D of a tile of TI columns of one
 * latitude row (Jacobian slots read along i, coalesced; identity-row columns skipped by
 * the slot bitmask), transposed through LDS into the k-contiguous level layout, then the
 * tile's colour-0 lines relaxed from the zero iterate and the other columns' iterate set
 * to 0 (one launch instead of rhs + first colour).  This is the route from the slot-major
 * Jacobian: the reference of k_mg_entry_p below (TsMg::nopack). */
template <int P>
__global__ void __launch_bounds__(256) k_mg_entry(const double* __restrict__ val, const uint8_t* __restrict__ knP,
                                                 const uint64_t* __restrict__ kmask,
                                                 const double* __restrict__ rr, const double* __restrict__ z,
                                                 Lay L, TsLev V)
{
    LAY_ALIASES;
    __shared__ double sb[2][64][MG_TI + 1];
    const int nx = L.nx;
    const int tiles = (nx + MG_TI - 1) / MG_TI;
    const int jl = blockIdx.x / tiles, i0 = (blockIdx.x % tiles) * MG_TI;
    const int j = L.jb0 + jl;
    const SubLay X = sub_of(L);
    for (int e = threadIdx.x; e < 2 * l * MG_TI; e += blockDim.x) {
        const int R = TT + e / (l * MG_TI);
        const int k = (e / MG_TI) % l, ii = e % MG_TI, i = i0 + ii;
        double acc = 0.0;
        if (i < nx) {
            const int64_t lc = ((int64_t)jl * l + k) * nx + i;
            const int64_t cell = L.own0 + lc;
            const int64_t row = PL(cell, R);
            if (!knP[row]) {
                int nc[3][9];
                nb_cells(X, i, j, k, nc);
                const uint64_t kb = kmask[2 * cell + 1];
                acc = R == TT ? bts_row<TT>(val, z, lc, L.nloc, nc, kb, rr[row], 1, L.ps)
                              : bts_row<SS>(val, z, lc, L.nloc, nc, kb, rr[row], 1, L.ps);
            }
        }
        sb[R - TT][k][ii] = acc;
    }
    __syncthreads();
    const int grp = threadIdx.x / P, k = threadIdx.x % P, ng = blockDim.x / P;
    const bool on = k < l;
    for (int ii = grp; ii < MG_TI; ii += ng) {
        const int i = i0 + ii;
        if (i >= nx) break;
        const int64_t c = on ? mg_cell(V, i, jl, k) : 0;
        const double bt = on ? sb[0][k][ii] : 0.0, bs = on ? sb[1][k][ii] : 0.0;
        if (on) {
            V.b[c] = bt;
            V.b[V.cstr + c] = bs;
        }
        if (mg_lcolour(V, i, jl) == 0) {
            double xt, xs;
            line_solve<P>(V.fac + c, V.cstr, on, k, bt, bs, xt, xs);
            if (on) {
                V.z[c] = xt;
                V.z[V.cstr + c] = xs;
            }
        } else if (on) {
            V.z[c] = 0.0;
            V.z[V.cstr + c] = 0.0;
        }
    }
}

/* The same launch on the packed operand (TsMg::ep, ts_mg_internal.h): the same tile, a thread
 * per cell of it forms both rows -- they read the same ten entries of z_D -- from the tile's
 * own contiguous run: a wave's load of one term is one run of its active lanes' doubles, no
 * line holds a land cell or another tile's, and no load waits for a slot mask (the masked
 * slots are stored as the 0.0 bts_row takes for them).  A lane finds its place in the run
 * from the tile's active-cell mask (popcount).  The loads of a cell are written before its
 * first sum.  (Loading the first colour-0 column's line factors ahead of all that holds 24
 * more registers through the sums, 98 VGPRs against 64, gains nothing and makes the
 * compiler contract the line solve differently: DESIGN.md §4.)  The sums are
 * bts_row's, term by term in its order, identity rows 0, and the line solve is the same
 * line_solve: level 0's b and z come out bitwise as from k_mg_entry. */
template <int P>
__global__ void __launch_bounds__(256) k_mg_entry_p(const double* __restrict__ ep, const uint64_t* __restrict__ etl,
                                                   int nw, const uint8_t* __restrict__ knP,
                                                   const double* __restrict__ rr, const double* __restrict__ z,
                                                   Lay L, TsLev V)
{
    LAY_ALIASES;
    __shared__ double sb[2][64][MG_TI + 1];
    const int nx = L.nx;
    const int tiles = (nx + MG_TI - 1) / MG_TI;
    const int jl = blockIdx.x / tiles, i0 = (blockIdx.x % tiles) * MG_TI;
    const int j = L.jb0 + jl;
    const SubLay X = sub_of(L);
    const uint64_t* e = etl + (int64_t)blockIdx.x * (2 + nw);
    const int64_t na = (int64_t)e[1];
    const double* run = ep + (int64_t)e[0];
    const int grp = threadIdx.x / P, kl = threadIdx.x % P, ng = blockDim.x / P;
    const bool on = kl < l;
    for (int q = threadIdx.x; q < l * MG_TI; q += blockDim.x) {
        const int k = q / MG_TI, ii = q % MG_TI;
        double at = 0.0, as = 0.0;
        if ((e[2 + (q >> 6)] >> (q & 63)) & 1) {
            const double* p = run + mg_entry_rank(e, q);
            double vt[MG_NE], vs[MG_NE], zz[MG_NE];
#pragma unroll
            for (int d = 0; d < MG_NE; d++) {
                vt[d] = p[d * na];
                vs[d] = p[(MG_NE + d) * na];
            }
            const int i = i0 + ii;
            const int64_t cell = L.own0 + ((int64_t)jl * l + k) * nx + i;
            int nc[3][9];
            nb_cells(X, i, j, k, nc);
#pragma unroll
            for (int d = 0; d < MG_NE; d++) {
                const Slot sl = SLOTS[MG_ES.s[0][d]];
                zz[d] = z[(int64_t)nc[sl.di + 1][(sl.dk + 1) * 3 + (sl.dj + 1)] + L.ps * sl.var];
            }
            const int64_t rt = PL(cell, TT), rs = PL(cell, SS);
            const uint8_t idt = knP[rt], ids = knP[rs];
            at = rr[rt];
            as = rr[rs];
#pragma unroll
            for (int d = 0; d < MG_NE; d++) {
                at -= vt[d] * zz[d];
                as -= vs[d] * zz[d];
            }
            if (idt) at = 0.0;
            if (ids) as = 0.0;
        }
        sb[0][k][ii] = at;
        sb[1][k][ii] = as;
    }
    __syncthreads();
    for (int ii = grp; ii < MG_TI; ii += ng) {
        const int i = i0 + ii;
        if (i >= nx) break;
        const int64_t c = on ? mg_cell(V, i, jl, kl) : 0;
        const double bt = on ? sb[0][kl][ii] : 0.0, bs = on ? sb[1][kl][ii] : 0.0;
        if (on) {
            V.b[c] = bt;
            V.b[V.cstr + c] = bs;
        }
        if (mg_lcolour(V, i, jl) == 0) {
            double xt, xs;
            line_solve<P>(V.fac + c, V.cstr, on, kl, bt, bs, xt, xs);
            if (on) {
                V.z[c] = xt;
                V.z[V.cstr + c] = xs;
            }
        } else if (on) {
            V.z[c] = 0.0;
            V.z[V.cstr + c] = 0.0;
        }
    }
}

/* fine iterate += coarse correction of its aggregate (active unknowns; level 0 of a band
 * group only, where the first post-smoothing colour reads neighbours across the band edge) */
__global__ void k_mg_prolong(TsLev F, TsLev C)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)F.n * F.mb * F.l) return;
    const int k = (int)(t % F.l), i = (int)((t / F.l) % F.n), jl = (int)(t / ((int64_t)F.l * F.n));
    const int64_t c = mg_cell(F, i, jl, k), p = mg_cell(C, i >> 1, jl >> 1, k);
    if (F.diag[c] != 0.0) F.z[c] += C.z[p];
    if (F.diag[3 * F.cstr + c] != 0.0) F.z[F.cstr + c] += C.z[C.cstr + p];
}

/* level-0 iterate -> z(T, S) of the preconditioner output on the active rows (when the
 * T/S block was solved before the last dynamics pass, whose defects see z(T, S) = 0) */
__global__ void k_mg_out(TsLev V, double* __restrict__ zout)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)V.n * V.mb * V.l) return;
    const int k = (int)(t % V.l), i = (int)((t / V.l) % V.n), jl = (int)(t / ((int64_t)V.l * V.n));
    const int64_t c = mg_cell(V, i, jl, k);
    const int64_t e = NUN * ((((int64_t)jl + HALO) * V.l + k) * V.n + i);
    if (V.diag[c] != 0.0) zout[e + TT] = V.z[c];
    if (V.diag[3 * V.cstr + c] != 0.0) zout[e + SS] = V.z[V.cstr + c];
}

}  // namespace

/* global index of local coarsest cell t (rank offsets I0, J0 in the GX-wide coarse grid) */
__device__ __forceinline__ int64_t mg_gq(int64_t t, int nc, int l, int GX, int I0, int J0)
{
    const int k = (int)(t % l), i = (int)((t / l) % nc), jl = (int)(t / ((int64_t)l * nc));
    return 2 * ((((int64_t)J0 + jl) * GX + I0 + i) * l + k);
}
/* local coarsest rhs (T block, S block) -> its entries of the global vector */
__global__ void k_mg_gput(const double* __restrict__ b, int64_t ncl, int nc, int l, int GX, int I0, int J0,
                          double* __restrict__ g)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncl) return;
    const int64_t q = mg_gq(t, nc, l, GX, I0, J0);
    g[q] = b[t];
    g[q + 1] = b[ncl + t];
}
/* own rows of the global solution -> local (T block, S block) */
__global__ void k_mg_gget(const double* __restrict__ y, int64_t ncl, int nc, int l, int GX, int I0, int J0,
                          double* __restrict__ z)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncl) return;
    const int64_t q = mg_gq(t, nc, l, GX, I0, J0);
    z[t] = y[q];
    z[ncl + t] = y[q + 1];
}

/* ---- T/S multigrid: host side ------------------------------------------------------ */
/* refresh the level-0 iterate's halo columns (phase x, owned rows) and halo rows (phase
 * y, whole rows with their halo columns) -- the subdomains coupled in the T/S smoother */
static int mg_halo(iemic_ctx* c, const TsLev& V)
{
    if (!V.vis && !V.visi) return 0;
    const int64_t W = V.n + 2 * V.hi, L = V.l;
    const int w = c->sub.nb[0], e = c->sub.nb[1], so = c->sub.nb[2], no = c->sub.nb[3];
    std::vector<Msg> x, y;
    for (double* z : {V.z, V.z + V.cstr}) {
        if (V.visi) {
            auto col = [&](int64_t i) { return Seg{z, (V.hj * W + V.hi + i) * L, V.mb, L, W * L}; };
            push_pair(x, w, e, col(0), col(V.n), col(V.n - 1), col(-1));
        }
        if (V.vis) {
            auto row = [&](int64_t jl) { return Seg{z, (V.hj + jl) * W * L, 1, W * L, W * L}; };
            push_pair(y, so, no, row(0), row(V.mb), row(V.mb - 1), row(-1));
        }
    }
    int rc = run_msgs(c, x);
    if (rc) return rc;
    return run_msgs(c, y);
}

/* the bands' level 0 (mg_hr): the iterate's 2 rows next to each neighbour band, and with b
 * its right-hand side's edge row -- for the halo-row line solves */
static int mg_halo2(iemic_ctx* c, const TsLev& V, bool with_b)
{
    const int64_t RW = (int64_t)V.n * V.l;
    const int so = c->sub.nb[2], no = c->sub.nb[3];
    std::vector<Msg> y;
    for (double* z : {V.z, V.z + V.cstr}) {
        auto rows = [&](int jl) { return Seg{z, (V.hj + jl) * RW, 1, 2 * RW, 2 * RW}; };
        push_pair(y, so, no, rows(0), rows(V.mb), rows(V.mb - 2), rows(-2));
    }
    if (with_b)
        for (double* b : {V.b, V.b + V.cstr}) {
            auto row = [&](int jl) { return Seg{b, (V.hj + jl) * RW, 1, RW, RW}; };
            push_pair(y, so, no, row(0), row(V.mb), row(V.mb - 1), row(-1));
        }
    return run_msgs(c, y);
}

/* one colour launch of the z-line smoother (C: first post-smoothing sweep, zout: final;
 * hr: the halo rows' lines too, mg_column) */
static int mg_zl(iemic_ctx* c, const TsLev& V, int colour, const TsLev* C, double* zout, int hr = 0)
{
    hipStream_t s = c->stream;
    const int P = mg_lanes(V.l);
    const unsigned g = (unsigned)((mg_columns_of(V, colour, hr) * P + 63) / 64);
    if (!g) return 0;
    const TsLev Cv = C ? *C : V;
    const int corr = C ? 1 : 0;
    with_lanes(P, [&](auto p) {
        hipLaunchKernelGGL(k_mg_zl<LANES_OF(p)>, dim3(g), dim3(64), 0, s, V, colour, Cv, corr, zout, hr);
    });
    return 0;
}

/* the coarsest level: z = A^-1 b (dense), or the bands' global coarsest problem */
static int mg_coarsest(iemic_ctx* c, int q)
{
    BlockGS& gs = c->gs;
    hipStream_t s = c->stream;
    int rc;
    const int N = 2 * gs.mg.n[q] * gs.mg.m[q] * c->l;
    if (gs.mg.glob) {
        /* gather the bands' right-hand sides, own rows of X b */
        const int64_t ncl = N / 2;
        if ((rc = dev_zero(c, gs.mg.gvec.p, gs.mg.gN))) return rc;
        hipLaunchKernelGGL(k_mg_gput, dim3(blocks_for(ncl)), dim3(256), 0, s, gs.mg.b[q].p, ncl,
                           gs.mg.n[q], c->l, gs.mg.gGX, gs.mg.gI0, gs.mg.gJ0, gs.mg.gvec.p);
        if ((rc = allreduce_sum(c, gs.mg.gvec.p, gs.mg.gN))) return rc;
        hipLaunchKernelGGL(k_gemv, dim3((unsigned)((gs.mg.gN + 3) / 4)), dim3(256), 0, s, gs.mg.gX.p,
                           gs.mg.gN, gs.mg.gN, gs.mg.gvec.p, gs.mg.gtmp.p);
        hipLaunchKernelGGL(k_mg_gget, dim3(blocks_for(ncl)), dim3(256), 0, s, gs.mg.gtmp.p, ncl,
                           gs.mg.n[q], c->l, gs.mg.gGX, gs.mg.gI0, gs.mg.gJ0, gs.mg.z[q].p);
        return 0;
    }
    if (N <= 1024)
        hipLaunchKernelGGL(k_gemv_w<16>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, (const double*)gs.mg.cinv.p,
                           N, (const double*)gs.mg.b[q].p, gs.mg.z[q].p);
    else if (N <= 2048)
        hipLaunchKernelGGL(k_gemv_w<32>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, (const double*)gs.mg.cinv.p,
                           N, (const double*)gs.mg.b[q].p, gs.mg.z[q].p);
    else
        hipLaunchKernelGGL(k_gemv, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, gs.mg.cinv.p, N, N,
                           gs.mg.b[q].p, gs.mg.z[q].p);
    return 0;
}

/* One V-cycle from level q.  first: the level's iterate started at 0 and its colour-0 lines
 * were relaxed by the launch that formed its right-hand side (k_mg_entry / k_mg_rc).
 * zout: the last level-0 sweep writes z(T, S) into the preconditioner output. */
/* a coarse level visited by the fused launches (k_mg_dn / k_mg_up): two colours, one
 * sweep, no halo on it or on its coarse level (one rank, or the bands' band-local levels) */
static bool mg_fused(iemic_ctx* c, int q)
{
    BlockGS& gs = c->gs;
    if (q < 1 || q + 1 >= gs.mg.nlev || std::max(1, gs.mg.sweeps) != 1 || !gs.mg.zu[q].p || gs.mg.nofuse)
        return false;
    const TsLev V = mg_view(c, q), C = mg_view(c, q + 1);
    return mg_ncolour(V) == 2 && !V.hj && !V.hi && !V.vis && !V.visi && !C.hj && !C.hi && C.l == V.l;
}
/* level q as its coarse-correction source: the iterate after its post-smoothing */
static TsLev mg_final(iemic_ctx* c, int q)
{
    TsLev V = mg_view(c, q);
    if (mg_fused(c, q)) V.z = c->gs.mg.zu[q].p;
    return V;
}

static int mg_vcycle(iemic_ctx* c, int q, bool first, double* zout)
{
    BlockGS& gs = c->gs;
    hipStream_t s = c->stream;
    int rc;
    const TsLev V = mg_view(c, q);
    const int nc = mg_ncolour(V), nu = std::max(1, gs.mg.sweeps);
    if (first && !zout && mg_fused(c, q)) {
        /* one launch down (colour 1 + restriction + the coarse colour 0), one launch up */
        const int qc = gs.mg.nlev - 1;
        const TsLev C = mg_view(c, q + 1);
        const int P = mg_lanes(V.l);
        const unsigned g = (unsigned)(C.n * C.mb);
        const int relax = q + 1 < qc ? 1 : 0;
        with_lanes(P, [&](auto p) {
            hipLaunchKernelGGL(k_mg_dn<LANES_OF(p)>, dim3(g), dim3(10 * LANES_OF(p)), 0, s, V, C, relax);
        });
        if (q + 1 == qc) {
            if ((rc = mg_coarsest(c, q + 1))) return rc;
        } else if ((rc = mg_vcycle(c, q + 1, true, nullptr))) {
            return rc;
        }
        const TsLev Cf = mg_final(c, q + 1);
        double* zu = gs.mg.zu[q].p;
        with_lanes(P, [&](auto p) {
            hipLaunchKernelGGL(k_mg_up<LANES_OF(p)>, dim3(g), dim3(10 * LANES_OF(p)), 0, s, V, Cf, zu);
        });
        return 0;
    }
    /* the bands' level 0, one sweep of two colours from the entry kernel: one exchange of 2
     * rows before each colour-1 launch, which relaxes the halo rows' colour-1 lines too
     * (the neighbour's own lines, operation for operation), so that the restriction and the
     * last colour-0 launch read them without another exchange (4 -> 2 batches per V-cycle) */
    const bool hrel = q == 0 && gs.mg.hr && V.hj == 2 && nu == 1 && nc == 2 && first;
    const int hr = hrel ? ((c->sub.nb[2] >= 0 ? 1 : 0) | (c->sub.nb[3] >= 0 ? 2 : 0)) : 0;
    for (int sw = 0; sw < nu; sw++)
        for (int h = (sw == 0 && first) ? 1 : 0; h < nc; h++) {
            if ((rc = hrel ? mg_halo2(c, V, true) : mg_halo(c, V))) return rc;
            if ((rc = mg_zl(c, V, h, nullptr, nullptr, hrel && h == 1 ? hr : 0))) return rc;
        }
    const int qc = gs.mg.nlev - 1;
    const TsLev C = mg_view(c, q + 1);
    if (!hrel && (rc = mg_halo(c, V))) return rc;
    {
        const int P = mg_lanes(V.l);
        const int shortcut = (first && nu == 1 && nc == 2) ? 1 : 0;
        const int relax = q + 1 < qc ? 1 : 0;
        const unsigned g = (unsigned)(((int64_t)C.n * C.mb * P + 63) / 64);
        with_lanes(P, [&](auto p) {
            hipLaunchKernelGGL(k_mg_rc<LANES_OF(p)>, dim3(g), dim3(64), 0, s, V, C, shortcut, relax);
        });
    }
    if (q + 1 == qc) {
        if ((rc = mg_coarsest(c, q + 1))) return rc;
    } else if ((rc = mg_vcycle(c, q + 1, true, nullptr))) {
        return rc;
    }
    const TsLev Cf = mg_final(c, q + 1);
    /* coarse correction: added where the first post-smoothing colours read it, or (level 0
     * of a band group, whose lines also read the neighbour bands' rows) explicitly */
    const bool corr = V.hj == 0 && V.hi == 0;
    if (!corr)
        hipLaunchKernelGGL(k_mg_prolong, dim3(blocks_for((int64_t)V.n * V.mb * V.l)), dim3(256), 0, s, V, Cf);
    for (int sw = 0; sw < nu; sw++)
        for (int h = nc - 1; h >= 0; h--) {
            if (hrel) {
                if (h == 1 && (rc = mg_halo2(c, V, false))) return rc;
            } else if ((rc = mg_halo(c, V))) {
                return rc;
            }
            if ((rc = mg_zl(c, V, h, corr && sw == 0 ? &Cf : nullptr, sw + 1 == nu ? zout : nullptr,
                            hrel && h == 1 ? hr : 0)))
                return rc;
        }
    return 0;
}

/* The T/S block solve by ts_mg V-cycles: the right-hand side rr_TS - A_TS,D z_D from the
 * planar dynamics iterate zd (k_mg_entry), then the V-cycles, the result into z(T, S) of the
 * output z only when out (else later by ts_mg_out).  side: the V-cycles (which read and
 * write only the multigrid's own buffers once the entry kernel has formed the right-hand
 * side) run on the side stream, forked after the entry kernel; gs_apply joins before
 * ts_mg_out. */
/* the entry launch: from the packed operand of the last set-up (every decomposition: it
 * forms the owned rows only), or from the Jacobian when the test hook asks (TsMg::nopack) */
int ts_mg_entry(iemic_ctx* c, const double* zd)
{
    BlockGS& gs = c->gs;
    const Lay L = lay_of(c->sub);
    hipStream_t s = c->stream;
    const TsLev V0 = mg_view(c, 0);
    const unsigned ge = (unsigned)(((c->sub.nx + MG_TI - 1) / MG_TI) * V0.mb);
    with_lanes(mg_lanes(c->l), [&](auto p) {
        if (gs.mg.nopack)
            hipLaunchKernelGGL(k_mg_entry<LANES_OF(p)>, dim3(ge), dim3(256), 0, s, gs.act.vp, gs.knP.p,
                               gs.kmask.p, gs.rrP.p, zd, L, V0);
        else
            hipLaunchKernelGGL(k_mg_entry_p<LANES_OF(p)>, dim3(ge), dim3(256), 0, s, (const double*)gs.mg.ep.p,
                               (const uint64_t*)gs.mg.etl.p, mg_entry_words(c->l), gs.knP.p, gs.rrP.p, zd, L, V0);
    });
    return 0;
}

int ts_mg_solve(iemic_ctx* c, const double* zd, double* z, bool out, bool side)
{
    BlockGS& gs = c->gs;
    int rc;
    if ((rc = ts_mg_entry(c, zd))) return rc;
    auto cycles = [&]() {
        int rc = 0;
        for (int cyc = 0; cyc < gs.ts_mg && !rc; cyc++)
            rc = mg_vcycle(c, 0, cyc == 0, out && cyc + 1 == gs.ts_mg ? z : nullptr);
        return rc;
    };
    if (side) {
        OnSide on(c);
        HIP_OK(on.err);
        if ((rc = cycles())) return rc;
        HIP_OK(on.join(false));
    } else if ((rc = cycles())) {
        return rc;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

/* the plan and level q for the test hooks (common.h TsMgProbe) */
int ts_mg_probe(iemic_ctx* c, int q, TsMgProbe* o)
{
    const TsMg& mg = c->gs.mg;
    *o = TsMgProbe{};
    if (c->gs.ts_mg <= 0 || mg.nlev < 2 || q < 0 || q >= mg.nlev) return IEMIC_EINVAL;
    const TsLev V = mg_final(c, q);
    o->nlev = mg.nlev;
    o->lanes = mg_lanes(c->l);
    o->sweeps = std::max(1, mg.sweeps);
    o->hr = mg.hr;
    o->ckind = mg.ckind;
    o->n = V.n;
    o->m = V.mb;
    o->par = V.jpar;
    o->colours = mg_ncolour(V);
    o->fused = mg_fused(c, q) ? 1 : 0;
    o->halo = (V.hj || V.hi) ? 1 : 0;
    o->off = V.off;
    o->diag = V.diag;
    o->b = V.b;
    o->z = V.z;
    o->cinv = q == mg.nlev - 1 ? mg.cinv.p : nullptr;
    return 0;
}

/* level-0 iterate -> z(T, S) of the preconditioner output (k_mg_out), after an early solve */
int ts_mg_out(iemic_ctx* c, double* z)
{
    const TsLev V0 = mg_view(c, 0);
    hipLaunchKernelGGL(k_mg_out, dim3(blocks_for((int64_t)V0.n * V0.mb * V0.l)), dim3(256), 0, c->stream, V0, z);
    return 0;
}

}  // namespace iemic
