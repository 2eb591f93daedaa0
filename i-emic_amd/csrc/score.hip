/*
 * score.hip -- the rare-event score function's distances on the device.
 *
 * Restates what the score functions of src/transient/ScoreFunctions.C evaluate after every time
 * step of every trajectory (get_default_score_function :53-65, get_ocean_score_function :163-189):
 *   d1 = ||x - sol1||_v / nrm,  d2 = ||x - sol2||_v / nrm,
 *   dist = f - f exp(-1/2 (d1 / 0.25)^2) + (1 - f) exp(-1/2 (d2 / 0.25)^2),
 * ||.||_v the 2-norm over the rows of one variable (the ocean score: v, GID % 6 == 1) or over all
 * rows (the default score).  The reference forms each distance as a copy, an update and a norm;
 * here one launch reads x, sol1 and sol2 once and leaves both sums of squares (k_sqdist2), then
 * one all-reduce of two values and one fetch.  Land rows count, as the reference's loop over
 * GID % dof counts them; halo rows do not.  The weights of the projected ocean score's
 * V^T diag(e_v) V (get_projected_ocean_score_function :204-213) are made here too.
 * Default contraction: the tests hold the sums to a bound that covers either rounding.
 */
#include <cmath>

#include "common.h"
#include "vec_kernels.h"

namespace iemic {

/* partial[blk] = sum (x - a)^2, partial[gridDim.x + blk] = sum (x - b)^2 over the block's share of
 * the n entries first + stride q (q < n): stride 1 walks rows, stride NUN the cells of one variable.
 * The entries of a thread are fixed by the grid (grid-stride), the lanes are summed by shuffles and
 * the waves in order: the same bits on every run.  k_mdot_final sums the partials. */
__global__ void __launch_bounds__(256) k_sqdist2(const double* __restrict__ x, const double* __restrict__ a,
                                                 const double* __restrict__ b, int64_t n, int stride, int first,
                                                 double* __restrict__ partial)
{
    __shared__ double sma[4], smb[4];
    double sa = 0.0, sb = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n;
         q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = first + stride * q;
        const double xr = x[r];
        const double da = xr - a[r], db = xr - b[r];
        sa += da * da;
        sb += db * db;
    }
    const double ta = block_sum(sa, sma), tb = block_sum(sb, smb);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = ta;
        partial[gridDim.x + blockIdx.x] = tb;
    }
}

/* w[q] = 1 on the rows of variable var, 0 elsewhere (q over the owned rows) */
__global__ void k_var_weights(double* __restrict__ w, int64_t N, int var)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        w[q] = (int)(q % NUN) == var ? 1.0 : 0.0;
}

static int score_buffers(iemic_ctx* c)
{
    Score& s = c->sc;
    if (s.part.reserve(2 * (size_t)GRAM_BLOCKS) || s.res.reserve(2)) {
        set_error("iemic_score: out of device memory");
        return IEMIC_ENOMEM;
    }
    return 0;
}

int score_sqdist2(iemic_ctx* c, int var, const double* x, const double* a, const double* b, double* out2)
{
    if (var < -1 || var >= NUN) {
        set_error("iemic_score: var = " + std::to_string(var) + " is outside -1 .. " + std::to_string(NUN - 1));
        return IEMIC_EINVAL;
    }
    int rc = score_buffers(c);
    if (rc) return rc;
    Score& s = c->sc;
    const Owned o = owned(c);
    const int64_t n = var < 0 ? o.n : o.n / NUN;
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, GRAM_BLOCKS));
    hipLaunchKernelGGL(k_sqdist2, dim3(nb), dim3(256), 0, c->stream, x + o.o, a + o.o, b + o.o, n, var < 0 ? 1 : NUN,
                       var < 0 ? 0 : var, s.part.p);
    hipLaunchKernelGGL(k_mdot_final, dim3(2), dim3(256), 0, c->stream, s.part.p, nb, 2, s.res.p);
    HIP_OK(hipGetLastError());
    if ((rc = allreduce_sum(c, s.res.p, 2))) return rc;
    return d2h(c, out2, s.res.p, sizeof(double) * 2);
}

/* sol1, sol2, sol3 (or null): ext vectors on the device; the context keeps copies of the first two */
int score_set(iemic_ctx* c, const double* sol1, const double* sol2, const double* sol3, int var)
{
    Score& s = c->sc;
    s.set = 0;
    const size_t NE = (size_t)c->sub.nerows();
    if (s.s1.reserve(NE) || s.s2.reserve(NE)) {
        set_error("iemic_score_set: out of device memory");
        return IEMIC_ENOMEM;
    }
    double q[2];
    /* ||sol1 - sol2||^2 and, with sol3, ||sol1 - sol3||^2 in the same launch */
    int rc = score_sqdist2(c, var, sol1, sol2, sol3 ? sol3 : sol2, q);
    if (rc) return rc;
    if (!(q[0] > 0.0) || !std::isfinite(q[0]) || !std::isfinite(q[1])) {
        set_error(!(q[0] == 0.0) ? "iemic_score_set: ||sol1 - sol2|| is not finite"
                                 : "iemic_score_set: sol1 and sol2 coincide on the score's rows (nrm = 0)");
        return IEMIC_ERANGE;
    }
    HIP_OK(hipMemcpyAsync(s.s1.p, sol1, sizeof(double) * NE, hipMemcpyDeviceToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(s.s2.p, sol2, sizeof(double) * NE, hipMemcpyDeviceToDevice, c->stream));
    s.var = var;
    s.nrm = std::sqrt(q[0]);
    s.dist_factor = sol3 ? std::sqrt(q[1]) / s.nrm : 0.5;
    s.set = 1;
    return 0;
}

int score_eval(iemic_ctx* c, const double* v, double* dist, double* d1, double* d2)
{
    const Score& s = c->sc;
    if (!s.set) {
        set_error("iemic_score: no score function set (iemic_score_set)");
        return IEMIC_ESTATE;
    }
    double q[2];
    const int rc = score_sqdist2(c, s.var, v ? v : c->d_x.p, s.s1.p, s.s2.p, q);
    if (rc) return rc;
    const double e1 = std::sqrt(q[0]) / s.nrm, e2 = std::sqrt(q[1]) / s.nrm, f = s.dist_factor;
    if (d1) *d1 = e1;
    if (d2) *d2 = e2;
    if (dist) *dist = f - f * std::exp(-0.5 * std::pow(e1 / 0.25, 2.)) + (1.0 - f) * std::exp(-0.5 * std::pow(e2 / 0.25, 2.));
    return 0;
}

int score_clear(iemic_ctx* c)
{
    Score& s = c->sc;
    s.set = 0;
    for (DevBuf<double>* b : {&s.s1, &s.s2, &s.part, &s.res}) b->free();
    return 0;
}

int proj_gram_vv(iemic_ctx* c, int var, double* out)
{
    const Projected& p = c->pj;
    if (p.k < 1) {
        set_error("iemic_proj_gram_vv: no basis set (iemic_proj_set_basis)");
        return IEMIC_ESTATE;
    }
    if (var < -1 || var >= NUN) {
        set_error("iemic_proj_gram_vv: var = " + std::to_string(var) + " is outside -1 .. " + std::to_string(NUN - 1));
        return IEMIC_EINVAL;
    }
    const Owned o = owned(c);
    const int64_t ld = c->sub.nerows();
    DevBuf<double> w;
    if (var >= 0) {
        if (w.alloc((size_t)o.n)) {
            set_error("iemic_proj_gram_vv: out of device memory");
            return IEMIC_ENOMEM;
        }
        hipLaunchKernelGGL(k_var_weights, dim3(o.grid), dim3(256), 0, c->stream, w.p, o.n, var);
        HIP_OK(hipGetLastError());
    }
    /* proj_gram ends with a fetch: the stream is idle when w is released */
    return proj_gram(c, p.V.p + o.o, ld, p.k, var >= 0 ? w.p : nullptr, p.V.p + o.o, ld, p.k, out);
}

}  // namespace iemic
