/*
 * projected.hip -- the projected theta model's device side and its small host algebra.
 *
 * Restates ProjectedThetaModel<Ocean> (src/transient/ProjectedThetaModel.H) and what
 * StochasticProjectedThetaModel<Ocean> (StochasticProjectedThetaModel.H) adds, on the resident
 * state confined to x = V y:
 *   restrict (:196-206)     y = V^T x                                   -> proj_gram, one column
 *   prolongate (:209-215)   x = V y                                     -> k_lincomb, 16 columns a launch
 *   initStep (:70-112)      y_n, F_n, VMV = V^T B V, VAV = V^T J2 V, LU -> proj_init_step
 *   computeRHS (:125-155)   r = dt (1 - theta) F_n + dt theta V^T F + VMV (y_n - y) [+ G]  -> proj_rhs
 *   solve (:163-193)        VAV dy = r / dt / theta                     -> proj_solve
 *   Newton.H:94-99          dy, y -= dy, x = V y, F, r                  -> proj_newton_step
 *   StochasticProjected initStep (:71-92)  G = V^T (sqrt(dt) sigma B_f pert)  -> proj_arm
 * The hot path is J2 V (spmv.hip's k_spmm7 on the shifted Jacobian theta.hip leaves in d_val)
 * and the block Gram products (k_gram).  Nothing here sets up a preconditioner or calls a Krylov
 * solver.  On several ranks every rank holds its rows of V; the small quantities come out of
 * all-reduces and are identical on every rank, so the host algebra is replicated.
 * Default contraction: no test needs these bits to match a restated expression.
 */
#include <chrono>
#include <cmath>
#include <cstring>

#include "common.h"
#include "vec_kernels.h"

namespace iemic {

/* partial[(a kb + b) gridDim.x + blk] = sum over the block's rows of V(q, a) d(q) W(q, b) for the
 * GRAM_T x GRAM_T tile (a0.., b0..) of blockIdx.y: a thread keeps the tile in registers, so a row
 * of V and W is read once per tile of columns, not once per entry.  d null: no weights.  The
 * rows of a thread are fixed by the grid (grid-stride), the lanes are summed by shuffles and the
 * waves in order: the same bits on every run.  k_mdot_final sums the partials. */
__global__ void __launch_bounds__(256) k_gram(const double* __restrict__ V, int64_t ldv, int ka,
                                              const double* __restrict__ d, const double* __restrict__ W,
                                              int64_t ldw, int kb, int64_t N, double* __restrict__ partial)
{
    __shared__ double sm[4][GRAM_T * GRAM_T];
    const int tb = (kb + GRAM_T - 1) / GRAM_T;
    const int a0 = (int)(blockIdx.y / tb) * GRAM_T, b0 = (int)(blockIdx.y % tb) * GRAM_T;
    double acc[GRAM_T][GRAM_T];
#pragma unroll
    for (int i = 0; i < GRAM_T; i++)
#pragma unroll
        for (int j = 0; j < GRAM_T; j++) acc[i][j] = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        double va[GRAM_T], wb[GRAM_T];
#pragma unroll
        for (int i = 0; i < GRAM_T; i++) va[i] = a0 + i < ka ? V[(int64_t)(a0 + i) * ldv + q] : 0.0;
#pragma unroll
        for (int j = 0; j < GRAM_T; j++) wb[j] = b0 + j < kb ? W[(int64_t)(b0 + j) * ldw + q] : 0.0;
        if (d) {
            const double dq = d[q];
#pragma unroll
            for (int i = 0; i < GRAM_T; i++) va[i] *= dq;
        }
#pragma unroll
        for (int i = 0; i < GRAM_T; i++)
#pragma unroll
            for (int j = 0; j < GRAM_T; j++) acc[i][j] += va[i] * wb[j];
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < GRAM_T; i++)
#pragma unroll
        for (int j = 0; j < GRAM_T; j++) {
            double v = acc[i][j];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) sm[wid][i * GRAM_T + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < GRAM_T * GRAM_T) {
        const int i = threadIdx.x / GRAM_T, j = threadIdx.x - i * GRAM_T;
        if (a0 + i < ka && b0 + j < kb) {
            double t = 0.0;
            for (int w = 0; w < 4; w++) t += sm[w][threadIdx.x];
            partial[((int64_t)(a0 + i) * kb + (b0 + j)) * gridDim.x + blockIdx.x] = t;
        }
    }
}

/* w[row of surface cell q] = G[q]: the step's noise field (Stoch::G, one double per owned (i, j))
 * on the surface S rows of an ext vector the caller zeroed */
__global__ void __launch_bounds__(256) k_proj_noise_rows(const double* __restrict__ G, int nx, int l, int64_t own0,
                                                         double* __restrict__ w, int ns)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= ns) return;
    const int il = q % nx, jl = q / nx;
    w[NUN * (own0 + ((int64_t)jl * l + (l - 1)) * nx + il) + SS] = G[q];
}

static int proj_ready(iemic_ctx* c, const char* who, bool step)
{
    if (c->pj.k < 1) {
        set_error(std::string(who) + ": no basis set (iemic_proj_set_basis)");
        return IEMIC_ESTATE;
    }
    if (step && !c->pj.init) {
        set_error(std::string(who) + ": no time step initialised (iemic_proj_init_step)");
        return IEMIC_ESTATE;
    }
    return 0;
}

int proj_alloc(iemic_ctx* c, int k)
{
    Projected& p = c->pj;
    const size_t NE = (size_t)c->sub.nerows();
    p.k = 0;
    p.init = p.armed = p.r_valid = 0;
    if (p.V.alloc(NE * k) || p.W.alloc(NE * k) || p.xold.alloc(NE) ||
        p.part.alloc((size_t)k * k * GRAM_BLOCKS) || p.res.alloc((size_t)k * k)) {
        proj_clear(c);
        set_error("iemic_proj_set_basis: out of device memory");
        return IEMIC_ENOMEM;
    }
    for (std::vector<double>* v : {&p.y, &p.yold, &p.yn, &p.Fn, &p.G, &p.r}) v->assign((size_t)k, 0.0);
    for (std::vector<double>* v : {&p.VMV, &p.VAV, &p.LU}) v->assign((size_t)k * k, 0.0);
    p.piv.assign((size_t)k, 0);
    int rc = dev_zero(c, p.V.p, (int64_t)(NE * k));
    if (!rc) rc = dev_zero(c, p.W.p, (int64_t)(NE * k));
    if (rc) return rc;
    p.k = k;
    return 0;
}

int proj_clear(iemic_ctx* c)
{
    Projected& p = c->pj;
    p.k = 0;
    p.init = p.armed = p.r_valid = 0;
    for (DevBuf<double>* b : {&p.V, &p.W, &p.xold, &p.part, &p.res}) b->free();
    return 0;
}

int proj_gram(iemic_ctx* c, const double* V, int64_t ldv, int ka, const double* d, const double* W, int64_t ldw,
              int kb, double* G)
{
    Projected& p = c->pj;
    if ((size_t)ka * kb > p.res.n || ka < 1 || kb < 1) {
        set_error("proj_gram: the result does not fit the basis' work space");
        return IEMIC_EINVAL;
    }
    const int64_t N = c->sub.nlrows();
    const int nb = (int)std::min<int64_t>((N + 255) / 256, GRAM_BLOCKS);
    const int ta = (ka + GRAM_T - 1) / GRAM_T, tb = (kb + GRAM_T - 1) / GRAM_T;
    hipLaunchKernelGGL(k_gram, dim3(nb, ta * tb), dim3(256), 0, c->stream, V, ldv, ka, d, W, ldw, kb, N, p.part.p);
    hipLaunchKernelGGL(k_mdot_final, dim3(ka * kb), dim3(256), 0, c->stream, p.part.p, nb, ka * kb, p.res.p);
    HIP_OK(hipGetLastError());
    int rc = allreduce_sum(c, p.res.p, ka * kb);
    if (rc) return rc;
    return d2h(c, G, p.res.p, sizeof(double) * ka * kb);
}

/* V^T w for one ext vector w */
static int proj_restrict(iemic_ctx* c, const double* w, double* out)
{
    const Owned o = owned(c);
    return proj_gram(c, c->pj.V.p + o.o, c->sub.nerows(), c->pj.k, nullptr, w + o.o, 0, 1, out);
}

/* state = V y on the owned rows, 16 columns a launch in column order */
static int proj_prolongate(iemic_ctx* c, const double* y)
{
    const Projected& p = c->pj;
    const Owned o = owned(c);
    const int64_t ld = c->sub.nerows();
    for (int b = 0; b < p.k; b += 16) {
        LinComb L{};
        L.a = b == 0 ? 0.0 : 1.0;
        for (int q = b; q < p.k && q < b + 16; q++) {
            L.c[L.nv] = y[q];
            L.X[L.nv] = p.V.p + (int64_t)q * ld + o.o;
            L.nv++;
        }
        hipLaunchKernelGGL(k_lincomb, dim3(o.grid), dim3(256), 0, c->stream, L, c->d_x.p + o.o, o.n);
    }
    HIP_OK(hipGetLastError());
    c->jac_valid = 0;
    return 0;
}

int proj_set_basis(iemic_ctx* c, const double* V, int k)
{
    if (k < 1 || k > SPMM_MAX_K) {
        set_error("iemic_proj_set_basis: k = " + std::to_string(k) + " is outside 1 .. " + std::to_string(SPMM_MAX_K));
        return IEMIC_EINVAL;
    }
    if (!V) {
        set_error("iemic_proj_set_basis: V is NULL");
        return IEMIC_EINVAL;
    }
    const int64_t N = c->nrows;
    for (int b = 0; b < k; b++)
        for (int64_t q = 0; q < N; q++)
            if (!std::isfinite(V[(int64_t)b * N + q])) {
                set_error("iemic_proj_set_basis: V[" + std::to_string(q) + ", " + std::to_string(b) + "] is not finite");
                return IEMIC_EINVAL;
            }
    int rc = proj_alloc(c, k);
    if (rc) return rc;
    Projected& p = c->pj;
    const int64_t ld = c->sub.nerows();
    std::vector<double> e((size_t)ld);
    for (int b = 0; b < k && !rc; b++) {
        std::fill(e.begin(), e.end(), 0.0);
        c->su.ref_to_ext(V + (int64_t)b * N, e.data());
        rc = h2d(c, p.V.p + (int64_t)b * ld, e.data(), sizeof(double) * (size_t)ld);
        if (!rc) rc = halo_exchange(c, p.V.p + (int64_t)b * ld, HALO);
    }
    if (!rc) rc = proj_restrict(c, c->d_x.p, p.y.data());
    if (rc) proj_clear(c);
    return rc;
}

int proj_restrict_state(iemic_ctx* c, double* y)
{
    int rc = proj_ready(c, "iemic_proj_restrict_state", false);
    if (rc) return rc;
    return proj_restrict(c, c->d_x.p, y);
}

int proj_set_state(iemic_ctx* c, const double* y)
{
    int rc = proj_ready(c, "iemic_proj_set_state", false);
    if (rc) return rc;
    Projected& p = c->pj;
    for (int a = 0; a < p.k; a++)
        if (!std::isfinite(y[a])) {
            set_error("iemic_proj_set_state: y[" + std::to_string(a) + "] is not finite");
            return IEMIC_EINVAL;
        }
    std::copy(y, y + p.k, p.y.begin());
    p.r_valid = 0;
    return proj_prolongate(c, p.y.data());
}

/* LU = P VAV with partial pivoting (row-major; unit lower factor below the diagonal); a zero or
 * non-finite pivot is returned by its index, -1: none */
static int proj_factor(Projected& p)
{
    const int k = p.k;
    p.LU = p.VAV;
    double* A = p.LU.data();
    for (int j = 0; j < k; j++) {
        int pr = j;
        double big = std::fabs(A[j * k + j]);
        for (int i = j + 1; i < k; i++)
            if (std::fabs(A[i * k + j]) > big) {
                big = std::fabs(A[i * k + j]);
                pr = i;
            }
        p.piv[j] = pr;
        if (pr != j)
            for (int q = 0; q < k; q++) std::swap(A[j * k + q], A[pr * k + q]);
        const double d = A[j * k + j];
        if (d == 0.0 || !std::isfinite(d)) return j;
        for (int i = j + 1; i < k; i++) {
            const double m = A[i * k + j] / d;
            A[i * k + j] = m;
            for (int q = j + 1; q < k; q++) A[i * k + q] -= m * A[j * k + q];
        }
    }
    return -1;
}

int proj_init_step(iemic_ctx* c, double dt, double theta)
{
    int rc = proj_ready(c, "iemic_proj_init_step", false);
    if (rc) return rc;
    if (!(theta > 0.0) || !(theta <= 1.0)) {
        set_error("iemic_proj_init_step: theta must lie in (0, 1] (the theta = 0 branch, which factors V^T B V, "
                  "is not restated)");
        return IEMIC_EINVAL;
    }
    if (!(dt > 0.0) || !std::isfinite(dt)) {
        set_error("iemic_proj_init_step: the time step dt must be positive");
        return IEMIC_EINVAL;
    }
    Projected& p = c->pj;
    const int k = p.k;
    const int64_t ld = c->sub.nerows();
    const Owned o = owned(c);
    p.init = p.armed = p.r_valid = 0;
    /* oldState_ = restrict(state_): of the large state */
    if ((rc = proj_restrict(c, c->d_x.p, p.yn.data()))) return rc;
    HIP_OK(hipMemcpyAsync(p.xold.p, c->d_x.p, sizeof(double) * (size_t)ld, hipMemcpyDeviceToDevice, c->stream));
    p.yold = p.y;
    /* oldRhs_ = restrict(F(state)) */
    if ((rc = halo_exchange(c, c->d_x.p, HALO))) return rc;
    if ((rc = assemble_rhs(c, c->d_x.p, c->d_F.p))) return rc;
    if ((rc = proj_restrict(c, c->d_F.p, p.Fn.data()))) return rc;
    /* VMV = V^T (B V) */
    if ((rc = assemble_diagB(c))) return rc;
    if ((rc = proj_gram(c, p.V.p + o.o, ld, k, c->d_B.p + o.o, p.V.p + o.o, ld, k, p.VMV.data()))) return rc;
    /* ThetaModel::computeJacobian, applyMatrix(V), VAV = V^T (J2 V) */
    if ((rc = theta_jacobian_at(c, dt, theta))) return rc;
    c->jac_valid = 1;
    if ((rc = spmm_kernel(c, p.V.p, ld, k, p.W.p, ld, p.kbmax))) return rc;
    if ((rc = proj_gram(c, p.V.p + o.o, ld, k, nullptr, p.W.p + o.o, ld, k, p.VAV.data()))) return rc;
    for (size_t e = 0; e < p.VAV.size(); e++)
        if (!std::isfinite(p.VAV[e])) {
            set_error("iemic_proj_init_step: V^T J2 V[" + std::to_string(e / k) + ", " + std::to_string(e % k) +
                      "] is not finite");
            return IEMIC_ERANGE;
        }
    const int bad = proj_factor(p);
    if (bad >= 0) {
        set_error("iemic_proj_init_step: V^T J2 V is singular: pivot " + std::to_string(bad) + " of " + std::to_string(k) +
                  " is " + (p.LU[(size_t)bad * k + bad] == 0.0 ? "zero" : "not finite") +
                  " (linearly dependent columns of V?)");
        return IEMIC_ERANGE;
    }
    p.dt = dt;
    p.theta = theta;
    p.init = 1;
    return 0;
}

/* StochasticProjectedThetaModel::initStep after ProjectedThetaModel's (the caller ran
 * proj_init_step): G = V^T of the full model's noise field of this step */
int proj_arm(iemic_ctx* c, double sigma, const double* pert)
{
    Projected& p = c->pj;
    p.armed = 0;
    p.r_valid = 0;
    std::fill(p.G.begin(), p.G.end(), 0.0);
    if (sigma == 0.0) return 0;
    int rc = stoch_noise(c, p.dt, sigma, pert);
    if (rc) return rc;
    /* column 0 of the scratch W: zero but for the surface S rows */
    const int64_t ld = c->sub.nerows();
    if ((rc = dev_zero(c, p.W.p, ld))) return rc;
    const int ns = c->sub.nx * c->sub.mb;
    hipLaunchKernelGGL(k_proj_noise_rows, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, c->st.G.p,
                       c->sub.nx, c->l, (int64_t)c->sub.own0, p.W.p, ns);
    HIP_OK(hipGetLastError());
    if ((rc = proj_restrict(c, p.W.p, p.G.data()))) return rc;
    p.armed = 1;
    return 0;
}

int proj_rhs(iemic_ctx* c, double* r)
{
    int rc = proj_ready(c, "iemic_proj_rhs", true);
    if (rc) return rc;
    Projected& p = c->pj;
    const int k = p.k;
    if ((rc = halo_exchange(c, c->d_x.p, HALO))) return rc;
    if ((rc = assemble_rhs(c, c->d_x.p, c->d_F.p))) return rc;
    std::vector<double> f((size_t)k);
    if ((rc = proj_restrict(c, c->d_F.p, f.data()))) return rc;
    const double a = p.dt * (1 - p.theta), b = p.dt * p.theta;
    for (int i = 0; i < k; i++) {
        double m = 0.0;
        for (int j = 0; j < k; j++) m += p.VMV[(size_t)i * k + j] * (p.yn[j] - p.y[j]);
        double v = a * p.Fn[i] + b * f[i];
        v = v + m;
        if (p.armed) v = v + p.G[i];
        p.r[i] = v;
    }
    p.r_valid = 1;
    if (r) std::copy(p.r.begin(), p.r.end(), r);
    return 0;
}

int proj_solve(iemic_ctx* c, const double* r, double* dy)
{
    int rc = proj_ready(c, "iemic_proj_solve", true);
    if (rc) return rc;
    const Projected& p = c->pj;
    const int k = p.k;
    const double* A = p.LU.data();
    std::vector<double> z((size_t)k);
    for (int i = 0; i < k; i++) z[i] = r[i] / p.dt / p.theta;
    for (int j = 0; j < k; j++) {
        std::swap(z[j], z[p.piv[j]]);
        for (int i = j + 1; i < k; i++) z[i] -= A[i * k + j] * z[j];
    }
    for (int i = k - 1; i >= 0; i--) {
        double s = z[i];
        for (int q = i + 1; q < k; q++) s -= A[i * k + q] * z[q];
        z[i] = s / A[i * k + i];
    }
    std::copy(z.begin(), z.end(), dy);
    return 0;
}

int proj_newton_step(iemic_ctx* c, iemic_proj_info* info)
{
    int rc = proj_ready(c, "iemic_proj_newton_step", true);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    Projected& p = c->pj;
    const int k = p.k;
    if (!p.r_valid && (rc = proj_rhs(c, nullptr))) return rc;
    std::vector<double> dy((size_t)k);
    if ((rc = proj_solve(c, p.r.data(), dy.data()))) return rc;
    iemic_proj_info inf{};
    for (int i = 0; i < k; i++) {
        inf.norm_dx = nanmax(inf.norm_dx, std::fabs(dy[i]));
        p.y[i] = p.y[i] - dy[i];
    }
    if ((rc = proj_prolongate(c, p.y.data()))) return rc;
    if ((rc = proj_rhs(c, nullptr))) return rc;
    double s = 0.0;
    for (int i = 0; i < k; i++) s += p.r[i] * p.r[i];
    inf.norm_f1 = std::sqrt(s);
    inf.t_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (info) *info = inf;
    return 0;
}

int proj_restore(iemic_ctx* c)
{
    int rc = proj_ready(c, "iemic_proj_restore", true);
    if (rc) return rc;
    const Owned w = owned(c);
    HIP_OK(hipMemcpyAsync(c->d_x.p + w.o, c->pj.xold.p + w.o, sizeof(double) * w.n, hipMemcpyDeviceToDevice,
                          c->stream));
    c->pj.y = c->pj.yold;
    c->jac_valid = 0;
    c->pj.r_valid = 0;
    return 0;
}

}  // namespace iemic
