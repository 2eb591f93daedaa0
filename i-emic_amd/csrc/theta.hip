/*
 * theta.hip -- the theta time stepper's device side, on the resident state.
 *
 * Restates what ThetaModel<Ocean> (src/transient/ThetaModel.H) lays over the Ocean model:
 *   initStep (:64-74)         x_n <- state, F_n <- F(x_n)                -> theta_init_step
 *   computeRHS (:87-113)      F_theta(x) = dt theta F(x) + dt (1 - theta) F_n + B (x_n - x)
 *                                                                       -> k_theta_residual
 *   computeJacobian (:118-146) J2 = J + diag(-B / dt / theta)           -> k_theta_shift
 *   solve (:150-164)          J2 dx = F_theta / dt / theta: the scaled copy is the
 *                             residual kernel's second output
 *   Newton.H:97               x <- x - dx, with ||dx||_inf              -> k_theta_update
 * Compiled with -ffp-contract=off like the assembly: the shifted diagonal and the residual are
 * the reference's expressions evaluated in the reference's order, bit for bit.
 */
#include <algorithm>

#include "common.h"
#include "mass_slots.h"

namespace iemic {

/* val[diagonal slot of row v][lc] += -B / dt / theta for v = U, V, T, S (blockIdx.y) of every
 * assembled cell: lanes along the cells, so each plane is written in contiguous 512-byte
 * wave stores.  Rows with B = 0 (land, the integral condition) are not touched. */
__global__ void __launch_bounds__(256) k_theta_shift(const double* __restrict__ B, double* __restrict__ val,
                                                     int64_t own0, int64_t nloc, double dt, double theta)
{
    const int64_t lc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lc >= nloc) return;
    const int r = blockIdx.y;
    const int var = r == 0 ? THETA_VAR[0] : r == 1 ? THETA_VAR[1] : r == 2 ? THETA_VAR[2] : THETA_VAR[3];
    const int slot = r == 0 ? THETA_SLOT[0] : r == 1 ? THETA_SLOT[1] : r == 2 ? THETA_SLOT[2] : THETA_SLOT[3];
    const double b = B[NUN * (own0 + lc) + var];
    if (b == 0.0) return;
    double* d = val + (int64_t)slot * nloc + lc;
    *d = *d + -b / dt / theta;
}

/* out = (dt theta) F + (dt (1 - theta)) F_n + B (x_n - x), summed left to right, and
 * outb = out / dt / theta, over the owned slab (a = dt theta, bn = dt (1 - theta)) */
__global__ void __launch_bounds__(256) k_theta_residual(double a, const double* __restrict__ F, double bn,
                                                        const double* __restrict__ Fn, const double* __restrict__ B,
                                                        const double* __restrict__ xn, const double* __restrict__ x,
                                                        double dt, double theta, double* __restrict__ out,
                                                        double* __restrict__ outb, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        const double v = a * F[q] + bn * Fn[q] + B[q] * (xn[q] - x[q]);
        out[q] = v;
        outb[q] = v / dt / theta;
    }
}

/* x -= dx over the owned slab; part[block] = max |dx| (reduced as k_vec_absmax: NaN propagates) */
__global__ void __launch_bounds__(256) k_theta_update(double* __restrict__ x, const double* __restrict__ dx,
                                                      int64_t N, double* __restrict__ part)
{
    __shared__ double sm[4];
    double v = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        const double d = dx[q];
        x[q] = x[q] - d;
        v = nanmax(v, fabs(d));
    }
    v = block_nanmax(v, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

static int theta_ready(iemic_ctx* c, const char* who)
{
    if (c->th.init) return 0;
    set_error(std::string(who) + ": no time step initialised (iemic_theta_init_step)");
    return IEMIC_ESTATE;
}

/* ThetaModel::initStep (ThetaModel.H:64-74); the preconditioner flag of its preProcess is the
 * caller's (`refactor` of iemic_theta_newton_step) */
int theta_init_step(iemic_ctx* c, double dt, double theta)
{
    if (!(theta > 0.0) || !(theta <= 1.0)) {
        set_error("iemic_theta_init_step: theta must lie in (0, 1] (theta = 0 divides by the mass matrix, "
                  "which is zero on the W, P, land and integral-condition rows)");
        return IEMIC_EINVAL;
    }
    if (!(dt > 0.0)) {
        set_error("iemic_theta_init_step: the time step dt must be positive");
        return IEMIC_EINVAL;
    }
    Theta& th = c->th;
    const size_t NE = (size_t)c->sub.nerows();
    if (th.xold.n != NE) {
        th.init = 0;
        if (th.xold.alloc(NE) || th.Fold.alloc(NE) || th.Ft.alloc(NE) || th.b.alloc(NE)) {
            set_error("iemic_theta_init_step: out of device memory");
            return IEMIC_ENOMEM;
        }
        for (DevBuf<double>* v : {&th.xold, &th.Fold, &th.Ft, &th.b}) {
            const int rz = dev_zero(c, v->p, (int64_t)NE);
            if (rz) return rz;
        }
    }
    th.init = 0;
    c->st.armed = 0;                 /* a plain step carries no noise (stoch_arm arms after this) */
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    if ((rc = assemble_rhs(c, c->d_x.p, c->d_F.p))) return rc;
    if ((rc = assemble_diagB(c))) return rc;
    HIP_OK(hipMemcpyAsync(th.xold.p, c->d_x.p, sizeof(double) * NE, hipMemcpyDeviceToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(th.Fold.p, c->d_F.p, sizeof(double) * NE, hipMemcpyDeviceToDevice, c->stream));
    th.dt = dt;
    th.theta = theta;
    th.init = 1;
    return 0;
}

/* ThetaModel::computeRHS (ThetaModel.H:87-113); with noise armed for the step,
 * StochasticThetaModel::computeRHS (stochastic.hip) */
int theta_rhs(iemic_ctx* c)
{
    int rc = theta_ready(c, "iemic_theta_rhs");
    if (rc) return rc;
    Theta& th = c->th;
    if ((rc = halo_exchange(c, c->d_x.p, HALO))) return rc;
    if ((rc = assemble_rhs(c, c->d_x.p, c->d_F.p))) return rc;
    if (c->st.armed) return stoch_theta_residual(c);
    const auto [o, NL, G] = owned(c);
    hipLaunchKernelGGL(k_theta_residual, dim3(G), dim3(256), 0, c->stream, th.dt * th.theta, c->d_F.p + o,
                       th.dt * (1 - th.theta), th.Fold.p + o, c->d_B.p + o, th.xold.p + o, c->d_x.p + o, th.dt,
                       th.theta, th.Ft.p + o, th.b.p + o, NL);
    HIP_OK(hipGetLastError());
    return 0;
}

/* ThetaModel::computeJacobian (ThetaModel.H:118-146).  The shift goes into the buffer
 * assemble_jacobian just filled (after its swap with ActiveSet::vold) and before anything
 * repacks from it: ActiveSet::coef_stale is set, so the compressed SpMV's stream
 * (gs_refresh) and the next prec_compute read the shifted values. */
int theta_jacobian(iemic_ctx* c)
{
    int rc = theta_ready(c, "iemic_theta_jacobian");
    if (rc) return rc;
    return theta_jacobian_at(c, c->th.dt, c->th.theta);
}

/* the same for a step the caller holds (the projected model's, projected.hip) */
int theta_jacobian_at(iemic_ctx* c, double dt, double theta)
{
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    if ((rc = assemble_jacobian(c, c->d_x.p))) return rc;
    hipLaunchKernelGGL(k_theta_shift, dim3((unsigned)((c->sub.nloc + 255) / 256), THETA_ROWS), dim3(256), 0,
                       c->stream, c->d_B.p, c->d_val.p, (int64_t)c->sub.own0, (int64_t)c->sub.nloc, dt, theta);
    HIP_OK(hipGetLastError());
    return 0;
}

/* Newton.H:95-97: x <- x - dx and this rank's ||dx||_inf */
int theta_update(iemic_ctx* c, const double* dx, double* absmax)
{
    const Owned w = owned(c);
    const int nb = (int)std::min<int64_t>((w.n + 255) / 256, RED_BLOCKS);
    hipLaunchKernelGGL(k_theta_update, dim3(nb), dim3(256), 0, c->stream, c->d_x.p + w.o, dx + w.o, w.n,
                       c->d_part.p);
    HIP_OK(hipGetLastError());
    c->jac_valid = 0;
    return part_nanmax(c, nb, absmax);
}

/* AdaptiveTransient.H:107: the state goes back to x_n after a failed Newton run */
int theta_restore(iemic_ctx* c)
{
    int rc = theta_ready(c, "iemic_theta_restore");
    if (rc) return rc;
    const Owned w = owned(c);
    HIP_OK(hipMemcpyAsync(c->d_x.p + w.o, c->th.xold.p + w.o, sizeof(double) * w.n, hipMemcpyDeviceToDevice,
                          c->stream));
    c->jac_valid = 0;
    return 0;
}

}  // namespace iemic
