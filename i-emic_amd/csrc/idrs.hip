/*
 * idrs.hip -- IDR(s) on the ocean's ext-layout vectors, the alternative to krylov.hip's FGMRES
 * (iemic_krylov::method = 1).  The method itself is idrs_run (idrs_core.h), shared with the
 * coupled model (coupled_krylov.hip); here are the ocean's vector space -- owned rows at
 * offset o of stride-NE vectors in the Krylov basis storage, mdot_host, prec_apply, spmv --
 * and the explicit residual at the end.  Work space, multi-dot and guards: krylov_internal.h;
 * vector kernels: vec_kernels.h.
 */
#include <chrono>

#include "common.h"
#include "idrs_core.h"
#include "vec_kernels.h"

namespace iemic {

/* the IDR shadow space P: s vectors uniform in [-1, 1] from splitmix64 over the global
 * row index (identical for every band split), orthonormalised by idrs_run (IDRSolver::createP) */
__global__ void k_idr_random(double* __restrict__ P, int64_t ldp, int s, int64_t NL, int64_t row0,
                             int n, int m, int l, int jb0, int ib0, int nx)
{
    const int64_t lr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lr >= NL) return;
    /* owned row -> global reference row 6((k m + j) n + i) + v */
    const int64_t lc = lr / NUN;
    const int v = (int)(lr % NUN);
    const int i = ib0 + (int)(lc % nx), k = (int)((lc / nx) % l), j = jb0 + (int)(lc / ((int64_t)nx * l));
    const uint64_t g = (uint64_t)(NUN * (((int64_t)k * m + j) * n + i) + v);
    for (int q = 0; q < s; q++) P[(int64_t)q * ldp + row0 + lr] = idr_shadow_entry(g, q, 20261015ull);
}

/* the ocean's vectors as idrs_run takes them (idrs_core.h) */
struct OceanSpace {
    iemic_ctx* c;
    int prec_on;
    int64_t ld, o, NL;                           /* stride NE; first owned row, owned rows */
    unsigned GR;
    hipStream_t stream;
    int work(int nvec, double*& base)
    {
        int rc = ensure_krylov(c, nvec);
        base = c->kr.V.p;
        return rc;
    }
    void shadow(double* P, int s)
    {
        hipLaunchKernelGGL(k_idr_random, dim3((unsigned)((NL + 255) / 256)), dim3(256), 0, c->stream, P, ld, s, NL,
                           o, c->n, c->m, c->l, c->sub.jb0, c->sub.ib0, c->sub.nx);
    }
    int mdot(const double* V, int nv, const double* w, double* out, const double* ea = nullptr,
             const double* eb = nullptr)
    {
        return mdot_host(c, V + o, ld, nv, w + o, out, ea ? ea + o : nullptr, eb ? eb + o : nullptr);
    }
    int norm2(const double* a, double* out) { return dot_owned(c, a, a, out); }
    /* y = a y + sum c_i x_i on the owned rows; lincomb2: two of them in one pass */
    void lincomb(double a, double* y, const Coefs& cs, const Vecs& xs)
    {
        hipLaunchKernelGGL(k_lincomb, dim3(GR), dim3(256), 0, c->stream, make_lc(a, cs, xs, o), y + o, NL);
    }
    void lincomb2(double a1, double* y1, const Coefs& c1, const Vecs& x1, double a2, double* y2, const Coefs& c2,
                  const Vecs& x2)
    {
        hipLaunchKernelGGL(k_lincomb2, dim3(GR), dim3(256), 0, c->stream, make_lc(a1, c1, x1, o), y1 + o,
                           make_lc(a2, c2, x2, o), y2 + o, NL);
    }
    void scale(double* y, double a)
    {
        hipLaunchKernelGGL(k_scale_copy, dim3(GR), dim3(256), 0, c->stream, y + o, a, y + o, NL);
    }
    void axpby(double a, const double* x, double b, const double* y, double* out)
    {
        hipLaunchKernelGGL(k_axpby, dim3(GR), dim3(256), 0, c->stream, a, x + o, b, y + o, out + o, NL);
    }
    int copy(double* dst, const double* src)
    {
        HIP_OK(hipMemcpyAsync(dst, src, sizeof(double) * ld, hipMemcpyDeviceToDevice, c->stream));
        return 0;
    }
    int prec(const double* in, double* out) { return prec_on ? prec_apply(c, in, out) : copy(out, in); }
    int apply(double* in, double* out) { return spmv(c, in, out, c->stream); }    /* fills in's halo */
};

int idrs(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt, iemic_solve_info* info)
{
    iemic_solve_info inf{};
    auto T0 = std::chrono::steady_clock::now();
    const Owned w = owned(c);
    OceanSpace sp{c, opt->prec > 0, c->sub.nerows(), w.o, w.n, w.grid, c->stream};
    int rc = dev_zero(c, x, sp.ld);
    if (rc) return rc;
    const double normb = sqrt0(dot(c, b, b, 0));
    if (!std::isfinite(normb)) return nonfinite();
    if (!(normb > 0.0)) {
        inf.converged = 1;
        if (info) *info = inf;
        return 0;
    }
    if ((rc = idrs_run(sp, b, x, opt, normb, inf))) return rc;
    /* explicit residual (the shadow space is no longer needed: scratch) */
    double* t = c->kr.V.p;
    if ((rc = spmv(c, x, t, c->stream))) return rc;
    sp.axpby(1.0, b, -1.0, t, t);
    const double e2v = dot(c, t, t, 0);
    inf.explicit_rel_res = sqrt0(e2v) / normb;
    inf.converged = inf.converged && inf.explicit_rel_res <= 2.0 * opt->tol;
    inf.t_total_ms = ms_since(T0);
    inf.t_orth_ms = std::max(0.0, inf.t_total_ms - inf.t_prec_ms - inf.t_spmv_ms);
    HIP_OK(hipGetLastError());
    if (info) *info = inf;
    return 0;
}

}  // namespace iemic
