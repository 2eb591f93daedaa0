/*
 * newton.hip -- the C ABI's solve side: the operator (F, J, SpMV), the preconditioner and the
 * linear solves, the Newton iteration, and the entry points of the theta stepper (theta.hip), of
 * its stochastic model (stochastic.hip), of the projected theta model (projected.hip) and of the
 * linear stability analysis (eigs.hip).
 *
 * One iteration of transient/Newton.H:92-99 is written once, newton_iterate, over the two
 * models that run it: the steady model (F(x) = 0, iemic_newton_step) and the theta model of a
 * time step (F_theta(x) = 0, iemic_theta_newton_step).  A model is a plain struct that says
 * where its residual lives and how its Jacobian, its right-hand side and its update are made;
 * the schedule, the points at which the host waits for the device, the timing and the
 * convergence status are the iteration's.
 */
#include <chrono>
#include <cmath>

#include "capi_internal.h"

using namespace iemic;

extern "C" int iemic_jacobian(iemic_ctx* c)
{
    CTX_CHECK(c);
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    if ((rc = assemble_jacobian(c, c->d_x.p))) return rc;
    DEV_SYNC(c);
    return 0;
}

extern "C" int iemic_rhs(iemic_ctx* c, double* F)
{
    CTX_CHECK(c);
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    if ((rc = assemble_rhs(c, c->d_x.p, c->d_F.p))) return rc;
    if (F) return get_ref(c, c->d_F.p, F);
    DEV_SYNC(c);
    return 0;
}

extern "C" int iemic_diag_b(iemic_ctx* c, double* B)
{
    CTX_CHECK(c);
    if (!c->jac_valid) return IEMIC_ESTATE;
    return get_ref(c, c->d_B.p, B);
}

extern "C" int iemic_export_csr(iemic_ctx* c, int64_t* rowptr, int* col, double* val)
{
    CTX_CHECK(c);
    if (!c->jac_valid) {
        set_error("iemic_export_csr: no Jacobian assembled");
        return IEMIC_ESTATE;
    }
    std::vector<double> v((size_t)NSLOT * c->sub.nloc);
    int rc = d2h(c, v.data(), c->d_val.p, sizeof(double) * v.size());
    if (rc) return rc;
    c->su.to_csr(v.data(), rowptr, col, val);
    return 0;
}

extern "C" int iemic_spmv(iemic_ctx* c, const double* x, double* y)
{
    CTX_CHECK(c);
    int rc = put_ref(c, x, c->d_tmp1.p);
    if (rc) return rc;
    if ((rc = spmv(c, c->d_tmp1.p, c->d_tmp2.p, c->stream))) return rc;
    return get_ref(c, c->d_tmp2.p, y);
}

extern "C" int iemic_spmv_dev(iemic_ctx* c, double* x, double* y, void*)
{
    CTX_CHECK(c);
    return spmv(c, x, y, c->stream);
}

extern "C" int iemic_prec_compute(iemic_ctx* c, const iemic_krylov* opt)
{
    CTX_CHECK(c);
    int rc = prec_compute(c, opt);
    if (rc) return rc;
    DEV_SYNC(c);
    return 0;
}

extern "C" int iemic_prec_apply(iemic_ctx* c, const double* r, double* z)
{
    CTX_CHECK(c);
    int rc = put_ref(c, r, c->d_tmp1.p);
    if (rc) return rc;
    if ((rc = prec_apply(c, c->d_tmp1.p, c->d_tmp2.p))) return rc;
    return get_ref(c, c->d_tmp2.p, z);
}

extern "C" int iemic_solve_dev(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt,
                               iemic_solve_info* info)
{
    CTX_CHECK(c);
    if (!opt) return IEMIC_EINVAL;
    return krylov_solve(c, b, x, opt, info);
}

extern "C" int iemic_solve(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt,
                           iemic_solve_info* info)
{
    CTX_CHECK(c);
    if (!opt || !b || !x) return IEMIC_EINVAL;
    DevBuf<double> db, dx;
    if (db.alloc(c->sub.nerows()) || dx.alloc(c->sub.nerows())) return IEMIC_ENOMEM;
    int rc = put_ref(c, b, db.p);
    if (rc) return rc;
    if ((rc = krylov_solve(c, db.p, dx.p, opt, info))) return rc;
    return get_ref(c, dx.p, x);
}

namespace iemic {
__global__ void k_newton_update(double* __restrict__ x, const double* __restrict__ dx, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        x[q] += dx[q];
}
__global__ void k_neg(const double* __restrict__ a, double* __restrict__ b, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        b[q] = -a[q];
}
}  // namespace iemic

namespace {

/* F(x) = 0 on the resident state: J dx = -F, x += dx */
struct SteadyModel {
    using Info = iemic_newton_info;
    const double* F(iemic_ctx* c) const { return c->d_F.p; }
    int rhs(iemic_ctx* c) const
    {
        const int rc = halo_exchange(c, c->d_x.p, HALO);
        return rc ? rc : assemble_rhs(c, c->d_x.p, c->d_F.p);
    }
    int jacobian(iemic_ctx* c) const { return assemble_jacobian(c, c->d_x.p); }
    bool refactor(const iemic_ctx*) const { return true; }
    /* -F into d_tmp1: launched between the preconditioner's timing and the solve's */
    const double* solve_rhs(iemic_ctx* c) const
    {
        const auto [o, NL, G] = owned(c);
        hipLaunchKernelGGL(k_neg, dim3(G), dim3(256), 0, c->stream, c->d_F.p + o, c->d_tmp1.p + o, NL);
        return c->d_tmp1.p;
    }
    int update(iemic_ctx* c, const double* dx, Info&) const
    {
        const auto [o, NL, G] = owned(c);
        hipLaunchKernelGGL(k_newton_update, dim3(G), dim3(256), 0, c->stream, c->d_x.p + o, dx + o, NL);
        return 0;
    }
};

/* F_theta(x) = 0 of the initialised time step: J2 dx = F_theta / dt / theta (ThetaModel.H:150-164,
 * the scaled copy Theta::b is made with the residual), x -= dx.  The preconditioner of the time
 * step is kept unless the caller asks for a new one or none is set up. */
struct ThetaModel {
    using Info = iemic_theta_info;
    int refactor_asked;
    const double* F(iemic_ctx* c) const { return c->th.Ft.p; }
    int rhs(iemic_ctx* c) const { return theta_rhs(c); }
    int jacobian(iemic_ctx* c) const { return theta_jacobian(c); }
    bool refactor(const iemic_ctx* c) const { return refactor_asked || !c->gs.ready; }
    const double* solve_rhs(iemic_ctx* c) const { return c->th.b.p; }
    /* the host waits for the device inside: ||dx||_inf comes back, then the max over the ranks */
    int update(iemic_ctx* c, const double* dx, Info& inf) const
    {
        const int rc = theta_update(c, dx, &inf.norm_dx);
        return rc ? rc : host_max(c, &inf.norm_dx);
    }
};

/* one iteration of transient/Newton.H:92-99: F, J, the preconditioner, the solve for dx, the
 * update, F again.  Only the two residuals, the Jacobian, the preconditioner and the solve are
 * timed; each timed part ends with the host waiting for the device. */
template <class Model>
int newton_iterate(iemic_ctx* c, const iemic_krylov* opt, const Model& M, typename Model::Info* info)
{
    typename Model::Info inf{};
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    auto T0 = clk::now();
    auto t = clk::now();
    int rc = M.rhs(c);
    if (rc) return rc;
    DEV_SYNC(c);
    inf.t_rhs_ms += ms(t);
    inf.norm_f0 = std::sqrt(dot(c, M.F(c), M.F(c), 0));   /* NaN stays NaN */
    t = clk::now();
    if ((rc = M.jacobian(c))) return rc;
    DEV_SYNC(c);
    inf.t_jac_ms = ms(t);
    t = clk::now();
    if (opt->prec > 0 && M.refactor(c)) {
        if ((rc = prec_compute(c, opt))) return rc;
        DEV_SYNC(c);
    }
    inf.t_prec_ms = ms(t);
    const double* b = M.solve_rhs(c);
    t = clk::now();
    if ((rc = krylov_solve(c, b, c->d_tmp2.p, opt, &inf.solve))) return rc;
    DEV_SYNC(c);
    inf.t_solve_ms = ms(t);
    if ((rc = M.update(c, c->d_tmp2.p, inf))) return rc;
    t = clk::now();
    if ((rc = M.rhs(c))) return rc;
    DEV_SYNC(c);
    inf.t_rhs_ms += ms(t);
    inf.norm_f1 = std::sqrt(dot(c, M.F(c), M.F(c), 0));   /* NaN stays NaN */
    c->jac_valid = 1;
    inf.t_total_ms = ms(T0);
    if (info) *info = inf;
    /* Newton.H applies the update whatever the solver reported; the caller learns that the
     * solve missed its tolerance from a distinct status */
    return inf.solve.converged ? 0 : IEMIC_ENOCONV;
}

}  // namespace

/* transient/Newton.H:92-99: F, J, solve J dx = -F, x += dx, F */
extern "C" int iemic_newton_step(iemic_ctx* c, const iemic_krylov* opt, iemic_newton_info* info)
{
    CTX_CHECK(c);
    if (!opt) return IEMIC_EINVAL;
    return newton_iterate(c, opt, SteadyModel{}, info);
}

/* ---- the theta time stepper (theta.hip) ------------------------------------------------ */
/* ThetaModel::initStep (ThetaModel.H:64-74) */
extern "C" int iemic_theta_init_step(iemic_ctx* c, double dt, double theta)
{
    CTX_CHECK(c);
    return theta_init_step(c, dt, theta);
}

/* ThetaModel::computeRHS (ThetaModel.H:87-113) */
extern "C" int iemic_theta_rhs(iemic_ctx* c, double* F)
{
    CTX_CHECK(c);
    int rc = theta_rhs(c);
    if (rc) return rc;
    if (F) return get_ref(c, c->th.Ft.p, F);
    DEV_SYNC(c);
    return 0;
}

/* ThetaModel::computeJacobian (ThetaModel.H:118-146) */
extern "C" int iemic_theta_jacobian(iemic_ctx* c)
{
    CTX_CHECK(c);
    int rc = theta_jacobian(c);
    if (rc) return rc;
    DEV_SYNC(c);
    return 0;
}

/* AdaptiveTransient.H:107 after a failed Newton run: the model is set back to x_n */
extern "C" int iemic_theta_restore(iemic_ctx* c)
{
    CTX_CHECK(c);
    return theta_restore(c);
}

/* one iteration of Newton.H:92-99 on the theta model: F_theta, J2, solve J2 dx = F_theta / dt /
 * theta (ThetaModel.H:150-164), x -= dx, F_theta */
extern "C" int iemic_theta_newton_step(iemic_ctx* c, const iemic_krylov* opt, int refactor,
                                       iemic_theta_info* info)
{
    CTX_CHECK(c);
    if (!opt) return IEMIC_EINVAL;
    return newton_iterate(c, opt, ThetaModel{refactor}, info);
}

/* ---- the stochastic theta model (stochastic.hip) ----------------------------------------- */
/* Ocean::computeForcing (THCM::computeForcing, THCM.C:836-940) */
extern "C" int iemic_forcing_compute(iemic_ctx* c)
{
    CTX_CHECK(c);
    return stoch_forcing(c);
}

/* Ocean::getForcing: the entries of the last iemic_forcing_compute */
extern "C" int iemic_forcing_export(iemic_ctx* c, int64_t* rows, int* cols, double* vals, int64_t* nnz)
{
    CTX_CHECK(c);
    if (!nnz) {
        set_error("iemic_forcing_export: nnz is NULL");
        return IEMIC_EINVAL;
    }
    if (c->st.gen < 0) {
        set_error("iemic_forcing_export: no forcing operator computed (iemic_forcing_compute)");
        return IEMIC_ESTATE;
    }
    return stoch_export(c, rows, cols, vals, nnz);
}

/* StochasticThetaModel::initStep (StochasticThetaModel.H:52-72) with the caller's normals */
extern "C" int iemic_theta_init_step_noise(iemic_ctx* c, double dt, double theta, double sigma,
                                           const double* pert)
{
    CTX_CHECK(c);
    if (!pert) {
        set_error("iemic_theta_init_step_noise: pert is NULL (m standard normals, one per latitude)");
        return IEMIC_EINVAL;
    }
    if (!std::isfinite(sigma) || sigma < 0.0) {
        set_error("iemic_theta_init_step_noise: sigma must be finite and >= 0");
        return IEMIC_EINVAL;
    }
    for (int j = 0; j < c->m; j++)
        if (!std::isfinite(pert[j])) {
            set_error("iemic_theta_init_step_noise: pert[" + std::to_string(j) + "] is not finite");
            return IEMIC_EINVAL;
        }
    const int rc = theta_init_step(c, dt, theta);
    return rc ? rc : stoch_arm(c, sigma, pert);
}

/* ---- the projected theta model (projected.hip) -------------------------------------------- */
/* ProjectedThetaModel's constructor (ProjectedThetaModel.H:38-65): the space V */
extern "C" int iemic_proj_set_basis(iemic_ctx* c, const double* V, int k)
{
    CTX_CHECK(c);
    return proj_set_basis(c, V, k);
}

extern "C" int iemic_proj_clear(iemic_ctx* c)
{
    CTX_CHECK(c);
    DEV_SYNC(c);
    return proj_clear(c);
}

/* ProjectedThetaModel::restrict (ProjectedThetaModel.H:196-206) of the state */
extern "C" int iemic_proj_restrict_state(iemic_ctx* c, double* y)
{
    CTX_CHECK(c);
    if (!y) return IEMIC_EINVAL;
    return proj_restrict_state(c, y);
}

/* ProjectedThetaModel::setState (ProjectedThetaModel.H:114-118) */
extern "C" int iemic_proj_set_state(iemic_ctx* c, const double* y)
{
    CTX_CHECK(c);
    if (!y) return IEMIC_EINVAL;
    return proj_set_state(c, y);
}

/* ProjectedThetaModel::initStep (ProjectedThetaModel.H:70-112) */
extern "C" int iemic_proj_init_step(iemic_ctx* c, double dt, double theta)
{
    CTX_CHECK(c);
    return proj_init_step(c, dt, theta);
}

/* StochasticProjectedThetaModel::initStep (StochasticProjectedThetaModel.H:71-92) with the
 * caller's normals: iemic_theta_init_step_noise's checks */
extern "C" int iemic_proj_init_step_noise(iemic_ctx* c, double dt, double theta, double sigma, const double* pert)
{
    CTX_CHECK(c);
    if (!pert) {
        set_error("iemic_proj_init_step_noise: pert is NULL (m standard normals, one per latitude)");
        return IEMIC_EINVAL;
    }
    if (!std::isfinite(sigma) || sigma < 0.0) {
        set_error("iemic_proj_init_step_noise: sigma must be finite and >= 0");
        return IEMIC_EINVAL;
    }
    for (int j = 0; j < c->m; j++)
        if (!std::isfinite(pert[j])) {
            set_error("iemic_proj_init_step_noise: pert[" + std::to_string(j) + "] is not finite");
            return IEMIC_EINVAL;
        }
    const int rc = proj_init_step(c, dt, theta);
    return rc ? rc : proj_arm(c, sigma, pert);
}

/* ProjectedThetaModel::computeRHS (ProjectedThetaModel.H:125-155) */
extern "C" int iemic_proj_rhs(iemic_ctx* c, double* r)
{
    CTX_CHECK(c);
    return proj_rhs(c, r);
}

/* ProjectedThetaModel::solve (ProjectedThetaModel.H:163-193) */
extern "C" int iemic_proj_solve(iemic_ctx* c, const double* r, double* dy)
{
    CTX_CHECK(c);
    if (!r || !dy) return IEMIC_EINVAL;
    return proj_solve(c, r, dy);
}

/* one iteration of Newton.H:94-99 on the small state */
extern "C" int iemic_proj_newton_step(iemic_ctx* c, iemic_proj_info* info)
{
    CTX_CHECK(c);
    return proj_newton_step(c, info);
}

/* AdaptiveTransient.H:107 after a failed Newton run */
extern "C" int iemic_proj_restore(iemic_ctx* c)
{
    CTX_CHECK(c);
    return proj_restore(c);
}

/* the model's small vectors and matrices (smallState_, oldState_, oldRhs_, rhs_, G_, VMV_, VAVmat_) */
extern "C" int iemic_proj_get(iemic_ctx* c, const char* what, double* out)
{
    CTX_CHECK(c);
    if (!what || !out) return IEMIC_EINVAL;
    const Projected& p = c->pj;
    if (p.k < 1) {
        set_error("iemic_proj_get: no basis set (iemic_proj_set_basis)");
        return IEMIC_ESTATE;
    }
    const std::string w(what);
    const std::vector<double>* v = w == "y" ? &p.y : w == "y_n" ? &p.yn : w == "F_n" ? &p.Fn : w == "r" ? &p.r
                                 : w == "G" ? &p.G : w == "VMV" ? &p.VMV : w == "VAV" ? &p.VAV : nullptr;
    if (!v) {
        set_error("iemic_proj_get: unknown quantity '" + w + "' (y, y_n, F_n, r, G, VMV, VAV)");
        return IEMIC_EINVAL;
    }
    std::copy(v->begin(), v->end(), out);
    return 0;
}

/* ---- linear stability analysis (eigs.hip): the JDQZInterface seam ------------------------ */
/* Ocean::computeJacobian + the operator-side shift of JDQZInterface.H (alpha A - beta B) */
extern "C" int iemic_shifted_jacobian(iemic_ctx* c, double sigma)
{
    CTX_CHECK(c);
    int rc = shifted_jacobian(c, sigma);
    if (rc) return rc;
    DEV_SYNC(c);
    return 0;
}

/* JDQZ's construction on the model (run_ocean.C:82-97) */
extern "C" int iemic_eigs_begin(iemic_ctx* c, double sigma, int m, uint64_t seed, const iemic_krylov* opt)
{
    CTX_CHECK(c);
    if (!opt) return IEMIC_EINVAL;
    return eigs_begin(c, sigma, m, seed, opt);
}

/* one operator application of the eigen-iteration: applyMassMat, then the shifted solve */
extern "C" int iemic_eigs_step(iemic_ctx* c, const iemic_krylov* opt, double* hcol, iemic_eigs_info* info)
{
    CTX_CHECK(c);
    if (!opt || !hcol) return IEMIC_EINVAL;
    return eigs_step(c, opt, hcol, info);
}

/* the eigenvectors JDQZ hands to Utils::saveEigenvectors (Continuation.H:1116-1120) */
extern "C" int iemic_eigs_ritz(iemic_ctx* c, int j, int p, const double* Y, void** xvecs)
{
    CTX_CHECK(c);
    if (!c->eg.active || j > c->eg.j + (c->eg.broke ? 0 : 1)) {
        set_error("iemic_eigs_ritz: the run holds fewer than j basis vectors (iemic_eigs_begin, iemic_eigs_step)");
        return IEMIC_ESTATE;
    }
    if (!xvecs || p < 1 || p > 16) {
        set_error("iemic_eigs_ritz: needs 1 <= p <= 16 output vectors");
        return IEMIC_EINVAL;
    }
    const Owned w = owned(c);
    double* xs[16];
    for (int q = 0; q < p; q++) xs[q] = xvecs[q] ? (double*)xvecs[q] + w.o : nullptr;
    return eigs_ritz(c, c->eg.V.p + w.o, c->sub.nerows(), j, p, Y, xs, w.n);
}

/* JDQZ's restart from jmax back to jmin search directions, here on an Arnoldi decomposition */
extern "C" int iemic_eigs_restart(iemic_ctx* c, int p, const double* Q)
{
    CTX_CHECK(c);
    return eigs_restart(c, p, Q);
}

/* the residual JDQZ reports per converged pair, measured on the operator itself */
extern "C" int iemic_eigs_residual(iemic_ctx* c, double lam_re, double lam_im, double* x_re, double* x_im,
                                   double out[2])
{
    CTX_CHECK(c);
    return eigs_residual(c, lam_re, lam_im, x_re, x_im, out);
}

extern "C" int iemic_eigs_end(iemic_ctx* c)
{
    CTX_CHECK(c);
    DEV_SYNC(c);
    return eigs_end(c);
}
