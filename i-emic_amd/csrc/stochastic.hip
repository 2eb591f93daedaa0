/*
 * stochastic.hip -- the stochastic theta model's device side, on the resident state.
 *
 * Restates what StochasticThetaModel<Ocean> (src/transient/StochasticThetaModel.H) adds to
 * ThetaModel<Ocean>, and the ocean's stochastic forcing operator under it:
 *   stochastic_forcing (forcing.F90:220-265)   one entry per surface cell, the S forcing with
 *   + THCM::computeForcing (THCM.C:836-940)    par(SPER) = 0, in column j        -> k_stoch_forcing
 *   initStep (:52-72)     G = (sqrt(dt) sigma) (B_f pert), the product first   -> k_stoch_noise
 *   computeRHS (:79-83)   F_theta + G                                          -> k_stheta_residual
 * B_f has one entry per row, so G lives on the surface S rows only and is kept as a surface
 * field, one double per owned (i, j), never as a full-length vector.  Two departures from the
 * reference: G is zero on land cells (there it would land on identity rows),
 * and pert is m values in the global latitude index, the same on every rank.
 * Compiled with -ffp-contract=off like the assembly and theta.hip: the forcing column is
 * forcing_cell's S entry and the residual is theta.hip's expression, bit for bit.
 */
#include <cmath>

#include "common.h"

namespace iemic {

/* coF[(j - jb0) nx + (i - ib0)] = forcing_cell's f[SS] of the owned surface cell (i, j, l); the
 * caller passes the geometry with par[P_SPER] = 0 (a copy: the context's par is not touched).
 * Lanes along i.  "Coupled Salinity": the reference's operator is empty, the column zero. */
__global__ void __launch_bounds__(256) k_stoch_forcing(Geo g, const double* __restrict__ ftab,
                                                       const double* __restrict__ qcor,
                                                       double* __restrict__ coF, int ns)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ns) return;
    if (g.coupled_s) {
        coF[q] = 0.0;
        return;
    }
    const int i = g.ib0 + q % g.nx + 1, j = g.jb0 + q / g.nx + 1;
    double f[NUN];
    forcing_cell(g, ftab, qcor, i, j, g.l, f);
    coF[q] = f[SS];
}

/* G[q] = scale (coF[q] pert[j]) on the owned surface cells, scale = sqrt(dt) sigma from the host:
 * the one-entry row product is rounded first, then scaled (Apply, then Scale).  Zero on land
 * cells and on the integral-condition row (ext row rowintcon, -1: none or not owned), which
 * THCM::computeForcing leaves out of the operator. */
__global__ void __launch_bounds__(256) k_stoch_noise(Geo g, const double* __restrict__ coF,
                                                     const double* __restrict__ pert, double scale,
                                                     int64_t rowintcon, double* __restrict__ G, int ns)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ns) return;
    const int il = q % g.nx, jl = q / g.nx;
    const int i = g.ib0 + il + 1, j = g.jb0 + jl + 1;
    const int64_t row = NUN * (own0(g) + ((int64_t)jl * g.l + (g.l - 1)) * g.nx + il) + SS;
    double v = 0.0;
    if (LM(g, i, j, g.l) == OCEAN && row != rowintcon) v = scale * (coF[q] * pert[j - 1]);
    G[q] = v;
}

/* k_theta_residual (theta.hip) term for term, followed by + G on the surface S rows:
 * out = (dt theta) F + (dt (1 - theta)) F_n + B (x_n - x) [+ G], outb = out / dt / theta, over the
 * owned slab.  Row q is variable q % 6 of owned-local cell lc = q / 6 = (jl l + k) nx + il; the
 * top layer's S rows read G[jl nx + il].  A zero of G (land, the integral condition) is not
 * added: x + 0.0 would turn a -0.0 into +0.0. */
__global__ void __launch_bounds__(256) k_stheta_residual(double a, const double* __restrict__ F, double bn,
                                                         const double* __restrict__ Fn, const double* __restrict__ B,
                                                         const double* __restrict__ xn, const double* __restrict__ x,
                                                         const double* __restrict__ G, int nx, int l,
                                                         double dt, double theta, double* __restrict__ out,
                                                         double* __restrict__ outb, int64_t N)
{
    const unsigned nxl = (unsigned)nx * (unsigned)l, top = (unsigned)nx * (unsigned)(l - 1);
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        double v = a * F[q] + bn * Fn[q] + B[q] * (xn[q] - x[q]);
        const unsigned lc = (unsigned)(q / NUN);
        if ((int)(q - (int64_t)NUN * lc) == SS) {
            const unsigned jl = lc / nxl, r = lc - jl * nxl;
            if (r >= top) {
                const double gq = G[jl * (unsigned)nx + (r - top)];
                if (gq != 0.0) v = v + gq;
            }
        }
        out[q] = v;
        outb[q] = v / dt / theta;
    }
}

static int stoch_alloc(iemic_ctx* c)
{
    Stoch& st = c->st;
    const size_t ns = (size_t)c->sub.nx * c->sub.mb;
    if (st.coF.n == ns && st.G.n == ns && st.pert.n == (size_t)c->m) return 0;
    st.gen = -1;
    st.armed = 0;
    if (st.coF.alloc(ns) || st.G.alloc(ns) || st.pert.alloc((size_t)c->m)) {
        set_error("stochastic forcing: out of device memory");
        return IEMIC_ENOMEM;
    }
    return 0;
}

/* Ocean::computeForcing: the forcing column of the current parameters and inserted fields.
 * d_frc and the context's par are read-only here: SPER is zero in the kernel's copy of Geo. */
int stoch_forcing(iemic_ctx* c)
{
    int rc = stoch_alloc(c);
    if (rc) return rc;
    const int ns = c->sub.nx * c->sub.mb;
    Geo g = c->geo();
    g.par[P_SPER] = 0.0;
    hipLaunchKernelGGL(k_stoch_forcing, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, g,
                       c->d_ftab.p, c->d_qcor.p, c->st.coF.p, ns);
    HIP_OK(hipGetLastError());
    c->st.gen = c->frc_gen;
    return 0;
}

/* Ocean::getForcing: the reference's ndim x m matrix, owned entries in row order.  Land cells keep
 * the values the reference stores; the integral-condition row (SRES = 0) and, with "Coupled
 * Salinity", every row are left out.  rows / cols / vals may be null (the count alone). */
int stoch_export(iemic_ctx* c, int64_t* rows, int* cols, double* vals, int64_t* nnz)
{
    const int nx = c->sub.nx, mb = c->sub.mb;
    std::vector<double> coF((size_t)nx * mb);
    const int rc = d2h(c, coF.data(), c->st.coF.p, sizeof(double) * coF.size());
    if (rc) return rc;
    int64_t v = 0;
    if (!c->cfg.coupled_s)
        for (int jl = 0; jl < mb; jl++)
            for (int il = 0; il < nx; il++) {
                const int i = c->sub.ib0 + il, j = c->sub.jb0 + jl;
                const int64_t row = NUN * c->su.ref_cell(i, j, c->l - 1) + SS;
                if (row == c->su.rowintcon_ref) continue;
                if (rows) rows[v] = row;
                if (cols) cols[v] = j;
                if (vals) vals[v] = coF[(size_t)jl * nx + il];
                v++;
            }
    *nnz = v;
    return 0;
}

/* StochasticThetaModel::initStep after ThetaModel's (the caller ran theta_init_step): the forcing
 * column again if the forcing changed since it was computed, G of this step, and the noise armed
 * for theta_rhs.  sigma = 0 arms nothing: the residual stays k_theta_residual's. */
int stoch_arm(iemic_ctx* c, double sigma, const double* pert)
{
    c->st.armed = 0;
    if (sigma == 0.0) return 0;
    const int rc = stoch_noise(c, c->th.dt, sigma, pert);
    if (rc) return rc;
    c->st.armed = 1;
    return 0;
}

/* Stoch::G of a step of length dt, nothing armed: stoch_arm's field, which the projected model
 * restricts (projected.hip).  The full model's noise is disarmed: the field is shared. */
int stoch_noise(iemic_ctx* c, double dt, double sigma, const double* pert)
{
    Stoch& st = c->st;
    st.armed = 0;
    int rc = stoch_alloc(c);
    if (rc) return rc;
    if (st.gen != c->frc_gen && (rc = stoch_forcing(c))) return rc;
    if ((rc = h2d(c, st.pert.p, pert, sizeof(double) * (size_t)c->m))) return rc;
    const int ns = c->sub.nx * c->sub.mb;
    hipLaunchKernelGGL(k_stoch_noise, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, c->geo(),
                       st.coF.p, st.pert.p, std::sqrt(dt) * sigma, (int64_t)c->rowintcon, st.G.p, ns);
    HIP_OK(hipGetLastError());
    return 0;
}

/* StochasticThetaModel::computeRHS: theta_rhs's launch while noise is armed */
int stoch_theta_residual(iemic_ctx* c)
{
    Theta& th = c->th;
    const auto [o, NL, G] = owned(c);
    hipLaunchKernelGGL(k_stheta_residual, dim3(G), dim3(256), 0, c->stream, th.dt * th.theta, c->d_F.p + o,
                       th.dt * (1 - th.theta), th.Fold.p + o, c->d_B.p + o, th.xold.p + o, c->d_x.p + o,
                       c->st.G.p, c->sub.nx, c->l, th.dt, th.theta, th.Ft.p + o, th.b.p + o, NL);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace iemic
