/*
 * coupled_krylov.hip -- the Krylov solvers of the coupled model on packed vectors
 * [ocean owned rows | atmosphere]: iemic_coupled_solve with coupled_fgmres and IDR(s).
 *
 * IDR(s) is idrs_run (idrs_core.h), the loop the ocean's idrs runs (idrs.hip), over
 * CoupledSpace below.  The solvers share the element-wise vector kernels (vec_kernels.h) and
 * the Hessenberg code (hessenberg.h) with the ocean's, but not their reductions: the dots here
 * reduce over KB = 512 blocks with an LDS tree, and coupled_fgmres runs CGS2 with the
 * coefficients left on the device.  Operator and preconditioner: coupled.hip.
 */
#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <vector>

#include "common.h"
#include "coupled_internal.h"
#include "hessenberg.h"
#include "idrs_core.h"
#include "vec_kernels.h"

using namespace iemic;

namespace iemic {
namespace {

/* ---- packed-vector Krylov kernels that have no ocean twin ------------------------------ */
/* part[v*KB + b] = partial of V_v . w (v < nv), part[nv*KB + b] = w . w */
__global__ void __launch_bounds__(256) k_cdots(const double* __restrict__ V, int64_t ld, int nv,
                                               const double* __restrict__ w, int64_t N, double* __restrict__ part)
{
    __shared__ double sm[256];
    const int v = blockIdx.y;
    const double* a = v < nv ? V + (int64_t)v * ld : w;
    double s = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x)
        s += a[q] * w[q];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) sm[threadIdx.x] += sm[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(int64_t)v * KB + blockIdx.x] = sm[0];
}
__global__ void k_cfinal(const double* __restrict__ part, int nvec, double* __restrict__ out)
{
    __shared__ double sm[256];
    const int v = blockIdx.x;
    double s = 0.0;
    for (int q = threadIdx.x; q < KB; q += blockDim.x) s += part[(int64_t)v * KB + q];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) sm[threadIdx.x] += sm[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0 && v < nvec) out[v] = sm[0];
}
/* y = a*y + sum_v c_v X_v */
__global__ void k_cupdate(const double* __restrict__ X, int64_t ld, int nv, const double* __restrict__ c, double a,
                          double* __restrict__ y, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x) {
        double s = a * y[q];
        for (int v = 0; v < nv; v++) s += c[v] * X[(int64_t)v * ld + q];
        y[q] = s;
    }
}
/* IDR shadow space: uniform in [-1, 1] from splitmix64 over the packed row index */
__global__ void k_cidr_random(double* __restrict__ P, int64_t ld, int s, int64_t N)
{
    const int64_t q0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q0 >= N) return;
    for (int q = 0; q < s; q++) P[(int64_t)q * ld + q0] = idr_shadow_entry((uint64_t)q0, q, 20261017ull);
}
/* y -= sum_v c_v X_v with the coefficients in device memory (CGS2 pass without a host trip) */
__global__ void k_cupdate_m(const double* __restrict__ X, int64_t ld, int nv, const double* __restrict__ c,
                            double* __restrict__ y, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x) {
        double s = y[q];
        for (int v = 0; v < nv; v++) s += -c[v] * X[(int64_t)v * ld + q];
        y[q] = s;
    }
}
/* y *= 1 / sqrt(nrm2) from the device-resident squared norm (unchanged when it is not > 0) */
__global__ void k_cscale_dev(const double* __restrict__ nrm2, double* __restrict__ y, int64_t N)
{
    const double n2 = *nrm2;
    if (!(n2 > 0.0)) return;
    const double s = 1.0 / sqrt(n2);
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x)
        y[q] = s * y[q];
}

}  // namespace
}  // namespace iemic

namespace {
/* dots of packed vectors: the ocean's owned rows on every rank, the (replicated) atmosphere
 * on rank 0 only, summed over the ranks -- the same values on every rank.  out[v] = V_v . w
 * (v < nv), out[nv] = w . w, left on the device */
int cdot_dev(iemic_coupled* cm, const double* V, int64_t ld, int nv, const double* w, double* out)
{
    hipStream_t s = cm->oc->stream;
    const int64_t N = cm->oc->sub.rank == 0 ? cm->NC : cm->NL;
    hipLaunchKernelGGL(k_cdots, dim3(KB, nv + 1), dim3(256), 0, s, V, ld, nv, w, N, cm->part.p);
    hipLaunchKernelGGL(k_cfinal, dim3(nv + 1), dim3(256), 0, s, (const double*)cm->part.p, nv + 1, out);
    if (cm->oc->sub.nranks > 1) return allreduce_sum(cm->oc, out, nv + 1);
    return 0;
}

/* the same on the host: out[0..nv], and out[nv] returned (NaN when the reduction failed) */
double cdot_host(iemic_coupled* cm, const double* V, int64_t ld, int nv, const double* w, double* out)
{
    int rc = cdot_dev(cm, V, ld, nv, w, cm->hb.p);
    if (!rc) {
        (void)hipMemcpyAsync(cm->h_red, cm->hb.p, sizeof(double) * (nv + 1), hipMemcpyDeviceToHost, cm->oc->stream);
        rc = dev_wait(cm->oc, nullptr, "coupled dots");
    }
    for (int i = 0; i <= nv; i++) out[i] = rc ? std::nan("") : cm->h_red[i];
    return out[nv];
}

/* the packed vectors as idrs_run takes them (idrs_core.h), right preconditioned by the block
 * Gauss-Seidel preconditioner; storage in cm->V (and cm->Z, which coupled_fgmres sizes with it) */
struct CoupledSpace {
    iemic_coupled* cm;
    int prec_on;
    int64_t ld;                                  /* NC */
    hipStream_t stream;
    unsigned GR;
    int work(int nvec, double*& base)
    {
        if (cm->mk < nvec) {
            if (cm->V.alloc((size_t)(nvec + 1) * ld) || cm->Z.alloc((size_t)nvec * ld)) {
                set_error("coupled IDR(s): out of device memory");
                return IEMIC_ENOMEM;
            }
            cm->mk = nvec;
        }
        base = cm->V.p;
        return 0;
    }
    void shadow(double* P, int s)
    {
        hipLaunchKernelGGL(k_cidr_random, dim3((unsigned)((ld + 255) / 256)), dim3(256), 0, stream, P, ld, s, ld);
    }
    /* V_v . w from one cdot_dev (whose slot nv holds w . w), ea . ea from a second one into
     * slot nv unless it is that w . w; one copy and one wait */
    int mdot(const double* V, int nv, const double* w, double* out, const double* ea = nullptr,
             const double* eb = nullptr)
    {
        assert(ea == eb);
        int rc = 0;
        if (nv > 0 && (rc = cdot_dev(cm, V, ld, nv, w, cm->hb.p))) return rc;
        if (ea && (nv == 0 || ea != w) && (rc = cdot_dev(cm, nullptr, 0, 0, ea, cm->hb.p + nv))) return rc;
        const int nout = nv + (ea ? 1 : 0);
        HIP_OK(hipMemcpyAsync(cm->h_red, cm->hb.p, sizeof(double) * nout, hipMemcpyDeviceToHost, stream));
        if ((rc = dev_wait(cm->oc, nullptr, "coupled dots"))) return rc;
        std::copy(cm->h_red, cm->h_red + nout, out);
        return 0;
    }
    int norm2(const double* a, double* out) { return mdot(nullptr, 0, nullptr, out, a, a); }
    void lincomb(double a, double* y, const Coefs& cs, const Vecs& xs)
    {
        hipLaunchKernelGGL(k_lincomb, dim3(GR), dim3(256), 0, stream, make_lc(a, cs, xs, 0), y, ld);
    }
    void lincomb2(double a1, double* y1, const Coefs& c1, const Vecs& x1, double a2, double* y2, const Coefs& c2,
                  const Vecs& x2)
    {
        hipLaunchKernelGGL(k_lincomb2, dim3(GR), dim3(256), 0, stream, make_lc(a1, c1, x1, 0), y1, make_lc(a2, c2, x2, 0),
                           y2, ld);
    }
    void scale(double* y, double a)
    {
        hipLaunchKernelGGL(k_scale_copy, dim3(GR), dim3(256), 0, stream, (const double*)y, a, y, ld);
    }
    void axpby(double a, const double* x, double b, const double* y, double* out)
    {
        hipLaunchKernelGGL(k_axpby, dim3(GR), dim3(256), 0, stream, a, x, b, y, out, ld);
    }
    int copy(double* dst, const double* src)
    {
        HIP_OK(hipMemcpyAsync(dst, src, sizeof(double) * ld, hipMemcpyDeviceToDevice, stream));
        return 0;
    }
    int prec(const double* in, double* out) { return cpl_prec(cm, in, out, prec_on); }
    int apply(const double* in, double* out) { return cpl_apply(cm, in, out); }
};

/* r = b - A x on packed device vectors (w: scratch); returns ||r|| */
double coupled_residual(iemic_coupled* cm, const double* b, const double* x, double* w, double* r, int* rc)
{
    std::vector<double> tmp(1);
    if ((*rc = cpl_apply(cm, x, w))) return 0.0;
    hipLaunchKernelGGL(k_axpby, dim3(blocks_for(cm->NC)), dim3(256), 0, cm->oc->stream, 1.0, b, -1.0, (const double*)w,
                       r, cm->NC);
    return std::sqrt(std::max(cdot_host(cm, nullptr, 0, 0, r, tmp.data()), 0.0));
}

/* CoupledModel::FGMRESSolve (353-432): right-preconditioned FGMRES(m) with restarts on the
 * packed coupled vector, classical Gram-Schmidt with one re-orthogonalisation pass.  b, x:
 * device packed vectors; x starts at 0.  Leaves r = b - A x in cm->r and its norm over
 * bnorm in inf.explicit_rel_res. */
int coupled_fgmres(iemic_coupled* cm, const double* b, double* x, const iemic_krylov* opt, double bnorm,
                   iemic_solve_info& inf)
{
    hipStream_t s = cm->oc->stream;
    const int m = std::max(1, std::min(opt->krylov_dim, MAX_KRYLOV - 1));
    const int64_t NC = cm->NC;
    int rc = 0;
    if (cm->mk < m) {
        if (cm->V.alloc((size_t)(m + 1) * NC) || cm->Z.alloc((size_t)m * NC)) {
            set_error("iemic_coupled_solve: out of device memory for the Krylov basis");
            return IEMIC_ENOMEM;
        }
        cm->mk = m;
    }
    double* V = cm->V.p;
    double* Z = cm->Z.p;
    double* w = cm->w.p;
    double* r = cm->r.p;
    const unsigned G = blocks_for(NC);
    Hessenberg hess(m);
    std::vector<double> h(m + 2), y(m);
    double beta = bnorm, res = 1.0;
    int it = 0;
    HIP_OK(hipMemcpyAsync(r, b, sizeof(double) * NC, hipMemcpyDeviceToDevice, s));
    for (int cycle = 0; cycle <= opt->max_restarts; cycle++) {
        hipLaunchKernelGGL(k_scale_copy, dim3(G), dim3(256), 0, s, (const double*)r, 1.0 / beta, V, NC);
        hess.reset(beta);
        /* step jj enqueued: preconditioner, operator, CGS2 with the coefficients on the
         * device, the new vector scaled on the device, its coefficients copied into half
         * jj & 1 of the pinned h_red; the host enqueues step jj + 1 before it reads step jj
         * (the work of a step after the last one of a cycle is discarded) */
        const size_t HH = 2 * MAX_KRYLOV + 8;
        auto enqueue = [&](int jj) -> int {
            double* vj = V + (int64_t)jj * NC;
            double* zj = Z + (int64_t)jj * NC;
            double* vn = V + (int64_t)(jj + 1) * NC;
            int rc2;
            if ((rc2 = cpl_prec(cm, vj, zj, opt->prec > 0))) return rc2;
            if ((rc2 = cpl_apply(cm, zj, vn))) return rc2;
            double* hc0 = cm->hc.p + (size_t)(jj & 1) * HH;
            double* hc1 = hc0 + (jj + 1);
            double* hcn = hc0 + 2 * (jj + 1);
            for (int pass = 0; pass < 2; pass++) {
                double* hv = pass ? hc1 : hc0;
                if ((rc2 = cdot_dev(cm, V, NC, jj + 1, vn, hv))) return rc2;
                hipLaunchKernelGGL(k_cupdate_m, dim3(G), dim3(256), 0, s, (const double*)V, NC, jj + 1,
                                   (const double*)hv, vn, NC);
            }
            if ((rc2 = cdot_dev(cm, nullptr, 0, 0, vn, hcn))) return rc2;
            hipLaunchKernelGGL(k_cscale_dev, dim3(G), dim3(256), 0, s, (const double*)hcn, vn, NC);
            HIP_OK(hipMemcpyAsync(cm->h_red + (size_t)(jj & 1) * HH, hc0, sizeof(double) * (2 * (jj + 1) + 1),
                                  hipMemcpyDeviceToHost, s));
            HIP_OK(hipEventRecord(cm->ev[jj & 1], s));
            return 0;
        };
        int j = 0;
        if ((rc = enqueue(0))) return rc;
        for (; j < m; j++) {
            if (j + 1 < m && (rc = enqueue(j + 1))) return rc;
            DEV_WAIT_EVENT(cm->oc, cm->ev[j & 1]);
            const double* hr = cm->h_red + (size_t)(j & 1) * HH;
            for (int i = 0; i <= j; i++) h[i] = hr[i] + hr[j + 1 + i];
            const double hn2 = hr[2 * (j + 1)];
            if (!std::isfinite(hn2)) {
                (void)dev_wait(cm->oc, nullptr, "coupled fgmres");
                set_error("coupled FGMRES: non-finite value in the Krylov basis");
                return IEMIC_ERANGE;
            }
            const double hn = std::sqrt(std::max(hn2, 0.0));
            res = hess.push_column(j, h.data(), hn) / bnorm;
            it++;
            if (res <= opt->tol || hn == 0.0) {
                j++;
                break;
            }
        }
        hess.solve(j, y.data());
        if (j > 0) {
            (void)hipMemcpyAsync(cm->hb.p + MAX_KRYLOV + 4, y.data(), sizeof(double) * j, hipMemcpyHostToDevice, s);
            hipLaunchKernelGGL(k_cupdate, dim3(G), dim3(256), 0, s, (const double*)Z, NC, j,
                               (const double*)(cm->hb.p + MAX_KRYLOV + 4), 1.0, x, NC);
        }
        beta = coupled_residual(cm, b, x, w, r, &rc);
        if (rc) return rc;
        if (res <= opt->tol || cycle == opt->max_restarts) break;
    }
    inf.iters = it;
    inf.implicit_rel_res = res;
    inf.explicit_rel_res = beta / bnorm;
    return 0;
}
}  // namespace

/* CoupledModel::solve (274-432) on host vectors [ocean (reference order) | atmosphere]:
 * x0 = 0, FGMRES or IDR(s) (opt->method) on the packed vector, explicit residual at the
 * end.  The Jacobians must be current (iemic_coupled_jacobian); opt->prec > 0 selects the
 * block Gauss-Seidel preconditioner with the ocean's block preconditioner (computed here)
 * inside. */
extern "C" int iemic_coupled_solve(iemic_coupled* cm, const double* b_host, double* x_host,
                                   const iemic_krylov* opt, iemic_solve_info* info)
{
    if (!cm || !b_host || !x_host || !opt) return IEMIC_EINVAL;
    iemic_ctx* oc = cm->oc;
    iemic_atmos* a = cm->at;
    if (hipSetDevice(oc->device) != hipSuccess) return IEMIC_EDEVICE;
    if (!oc->jac_valid || !a->jac_valid) {
        set_error("iemic_coupled_solve: no Jacobian assembled");
        return IEMIC_ESTATE;
    }
    StreamGuard guard{oc};
    auto T0 = std::chrono::steady_clock::now();
    const int64_t NA = cm->NA, NC = cm->NC;
    int rc = 0;
    if (opt->prec > 0) {
        if ((rc = prec_compute(oc, opt))) return rc;
        if ((rc = atm_prec_compute(a))) return rc;
    }
    /* b, x to packed device vectors */
    std::vector<double> packed;
    pack_host(cm, b_host, packed);
    DevBuf<double> db, dxv;
    if (db.alloc(NC) || dxv.alloc(NC)) return IEMIC_ENOMEM;
    if ((rc = h2d(oc, db.p, packed.data(), sizeof(double) * NC))) return rc;
    HIP_OK(hipMemsetAsync(dxv.p, 0, sizeof(double) * NC, oc->stream));
    iemic_solve_info inf{};
    std::vector<double> tmp(1);
    const double bnorm = std::sqrt(std::max(cdot_host(cm, nullptr, 0, 0, db.p, tmp.data()), 0.0));
    if (!std::isfinite(bnorm)) return nonfinite();
    if (!(bnorm > 0)) {
        inf.converged = 1;
        if (info) *info = inf;
        std::fill(x_host, x_host + oc->nrows + NA, 0.0);
        return 0;
    }
    if (opt->method == 1) {
        CoupledSpace sp{cm, opt->prec > 0, NC, oc->stream, blocks_for(NC)};
        if ((rc = idrs_run(sp, db.p, dxv.p, opt, bnorm, inf))) return rc;
        inf.explicit_rel_res = coupled_residual(cm, db.p, dxv.p, cm->w.p, cm->r.p, &rc) / bnorm;
        if (rc) return rc;
    } else {
        if ((rc = coupled_fgmres(cm, db.p, dxv.p, opt, bnorm, inf))) return rc;
    }
    inf.converged = inf.implicit_rel_res <= opt->tol && inf.explicit_rel_res <= 10.0 * opt->tol;
    inf.t_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count();
    if ((rc = d2h(oc, packed.data(), dxv.p, sizeof(double) * NC))) return rc;
    unpack_host(cm, packed, x_host);
    if (info) *info = inf;
    return 0;
}
