/*
 * idrs_core.h -- IDR(s) (src/idrsolver/IDRSolver.H:109-340, van Gijzen & Sonneveld), written
 * once for the two vector spaces it runs on: the ocean's ext-layout vectors (OceanSpace,
 * idrs.hip) and the coupled model's packed vectors (CoupledSpace, coupled_krylov.hip).  Host
 * code only: every kernel, reduction and launch grid belongs to the space.
 *
 * A Space is a plain struct (no virtual calls) with
 *   int work(int nvec, double*& base)   storage of nvec vectors, stride ld (set by work)
 *   void shadow(P, s)                   s random shadow vectors, not yet orthonormal
 *   int mdot(V, nv, w, out, ea, eb)     out[i] = V_i . w (i < nv, stride ld) and, with ea,
 *                                       out[nv] = ea . eb: host values, one synchronisation
 *   int norm2(a, out)                   a . a likewise
 *   void lincomb / lincomb2 / scale / axpby   the element-wise updates
 *   int prec / apply / copy             z = M^-1 r, y = A x, dst = src
 *   hipStream_t stream                  where all of it runs (the step's timing events go there)
 * The convergence test runs one operator application late (r.r rides in the P'G multi-dot),
 * so a step costs one host synchronisation, and a converged solve spends one prec + apply
 * whose updates are not applied.
 */
#ifndef IEMIC_IDRS_CORE_H
#define IEMIC_IDRS_CORE_H

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "krylov_internal.h"

namespace iemic {

using Coefs = std::vector<double>;
using Vecs = std::vector<const double*>;

/* the events around a step's preconditioner (0, 1) and operator application (2) */
struct StepEvents {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~StepEvents()
    {
        for (hipEvent_t q : e)
            if (q) (void)hipEventDestroy(q);
    }
};

/* b, x: vectors of the space, x = 0 on entry; normb = ||b|| > 0.  Sets inf.iters, reorth,
 * implicit_rel_res and converged (the implicit test ||r|| <= tol ||b|| alone: the caller adds
 * its explicit residual) and adds the steps' t_prec_ms, t_spmv_ms, n_spmv.  After the return
 * the work storage is free for the caller. */
template <class Space>
int idrs_run(Space& sp, const double* b, double* x, const iemic_krylov* opt, double normb, iemic_solve_info& inf)
{
    const int s = std::max(1, std::min(opt->idr_s > 0 ? opt->idr_s : 4, 8));
    const double angle = opt->idr_angle > 0.0 ? opt->idr_angle : 0.7;
    const double mp = 1e-13;
    const int maxit = std::max(1, opt->krylov_dim * (opt->max_restarts + 1));
    /* vectors: P (s) | U (s) | G (s) | t | r | v */
    double* base = nullptr;
    int rc = sp.work(3 * s + 3, base);
    if (rc) return rc;
    const int64_t ld = sp.ld;
    double* P = base;
    double* U = base + (int64_t)s * ld;
    double* G = base + (int64_t)2 * s * ld;
    double* t = base + (int64_t)3 * s * ld;
    double* r = t + ld;                          /* t, r adjacent: one multi-dot for omega */
    double* v = r + ld;
    auto Ui = [&](int i) { return U + (int64_t)i * ld; };
    auto Gi = [&](int i) { return G + (int64_t)i * ld; };
    auto Pi = [&](int i) { return P + (int64_t)i * ld; };
    /* shadow space (createP: random, orthonormalised in order) */
    sp.shadow(P, s);
    for (int j = 0; j < s; j++) {
        Coefs al(j + 1);
        if (j > 0 && (rc = sp.mdot(P, j, Pi(j), al.data()))) return rc;
        Coefs cs;
        Vecs xs;
        for (int k = 0; k < j; k++) { cs.push_back(-al[k]); xs.push_back(Pi(k)); }
        if (j > 0) sp.lincomb(1.0, Pi(j), cs, xs);
        double nn = 0.0;
        if ((rc = sp.norm2(Pi(j), &nn))) return rc;
        nn = sqrt0(nn);
        if (!(nn > 0.0)) return nonfinite();
        sp.scale(Pi(j), 1.0 / nn);
    }
    if ((rc = sp.copy(r, b))) return rc;
    const double tolb = opt->tol * normb;
    double normr = normb;
    Coefs f(s, 0.0), gamma(s, 0.0), d(s + 2, 0.0);
    std::vector<Coefs> M(s, Coefs(s, 0.0));
    double om = 1.0;
    int jj = 0, iter = 0;
    bool trueres = false;
    StepEvents ev;
    for (hipEvent_t& q : ev.e) HIP_OK(hipEventCreate(&q));
    auto prec = [&](const double* in, double* out) -> int {
        HIP_OK(hipEventRecord(ev.e[0], sp.stream));
        int r2 = sp.prec(in, out);
        HIP_OK(hipEventRecord(ev.e[1], sp.stream));
        return r2;
    };
    auto apply = [&](double* in, double* out) -> int {
        int r2 = sp.apply(in, out);
        HIP_OK(hipEventRecord(ev.e[2], sp.stream));
        return r2;
    };
    auto times = [&]() {                          /* after a synchronisation: e[2] is done */
        float a1 = 0.f, a2 = 0.f;
        (void)hipEventElapsedTime(&a1, ev.e[0], ev.e[1]);
        (void)hipEventElapsedTime(&a2, ev.e[1], ev.e[2]);
        inf.t_prec_ms += a1;
        inf.t_spmv_ms += a2;
        inf.n_spmv++;
    };
    auto set_normr = [&](double rr) -> int {
        normr = sqrt0(rr);
        return std::isfinite(normr) ? 0 : nonfinite();
    };
    /* the norm of the r just updated, when residual replacement needs it at once */
    auto replace_norm = [&]() -> int {
        double rr = 0.0;
        int r2 = sp.norm2(r, &rr);
        if (!r2) r2 = set_normr(rr);
        if (!r2 && normr > tolb / mp) trueres = true;
        return r2;
    };
    /* one host synchronisation per inner step: the multi-dot after the operator also returns
     * r.r of the previous update, whose convergence check therefore comes one application late
     * (wasted only on the final step: the pending step's updates are not applied) */
    bool done = false;
    while (!done && iter < maxit) {
        if ((rc = sp.mdot(P, s, r, d.data(), r, r))) return rc;                 /* f = P' r, r.r */
        std::copy(d.begin(), d.begin() + s, f.begin());
        if ((rc = set_normr(d[s]))) return rc;
        if (normr <= tolb) break;
        for (int k = 0; k < s; k++) {
            if (jj > 0) {
                /* gamma from the lower-triangular M(k:s, k:s); v = r - G(:, k:s) gamma */
                Coefs cs{1.0};
                Vecs xs{r};
                for (int i = k; i < s; i++) {
                    double gi = f[i];
                    for (int j = k; j < i; j++) gi -= M[i][j] * gamma[j];
                    gamma[i] = gi / M[i][i];
                    cs.push_back(-gamma[i]);
                    xs.push_back(Gi(i));
                }
                sp.lincomb(0.0, v, cs, xs);                                      /* v = r - G gamma */
                if ((rc = prec(v, t))) return rc;
                /* U(:,k) = om t + U(:, k:s) gamma */
                cs.assign(1, om);
                xs.assign(1, t);
                for (int i = k; i < s; i++) { cs.push_back(gamma[i]); xs.push_back(Ui(i)); }
                sp.lincomb(0.0, Ui(k), cs, xs);
            } else {
                if ((rc = prec(r, Ui(k)))) return rc;                         /* initial space */
            }
            if ((rc = apply(Ui(k), Gi(k)))) return rc;                        /* G(:,k) = A U(:,k) */
            /* bi-orthogonalise against P(:, 0:k) (the modified Gram-Schmidt of the reference
             * restated as one multi-dot + forward substitution) and the new column of M; the
             * same launch returns r.r after the previous step's update */
            if ((rc = sp.mdot(P, s, Gi(k), d.data(), r, r))) return rc;
            times();
            if (k > 0) {
                if ((rc = set_normr(d[s]))) return rc;
                if (normr <= tolb) {
                    done = true;
                    break;
                }
            }
            Coefs al(k, 0.0);
            for (int i = 0; i < k; i++) {
                double a = d[i];
                for (int j = 0; j < i; j++) a -= al[j] * M[i][j];
                al[i] = a / M[i][i];
            }
            for (int i = k; i < s; i++) {
                double mik = d[i];
                for (int j = 0; j < k; j++) mik -= al[j] * M[i][j];
                M[i][k] = mik;
            }
            if (k > 0) {
                Coefs cs;
                Vecs xg, xu;
                for (int i = 0; i < k; i++) { cs.push_back(-al[i]); xg.push_back(Gi(i)); xu.push_back(Ui(i)); }
                sp.lincomb2(1.0, Gi(k), cs, xg, 1.0, Ui(k), cs, xu);
            }
            if (!std::isfinite(M[k][k])) return nonfinite();
            if (M[k][k] == 0.0) {
                set_error("IDR(s): breakdown (M[k][k] == 0)");
                return IEMIC_ERANGE;
            }
            const double beta = f[k] / M[k][k];
            sp.lincomb2(1.0, r, {-beta}, {Gi(k)}, 1.0, x, {beta}, {Ui(k)});      /* r -= beta G, x += beta U */
            if (opt->idr_replace && (rc = replace_norm())) return rc;
            for (int i = k + 1; i < s; i++) f[i] -= beta * M[i][k];
            iter++;
            if (iter >= maxit) break;
        }
        if (done || iter >= maxit) break;
        jj++;
        /* first residual of G_{j+1}: v = M^-1 r, t = A v, omega, r -= om t, x += om v */
        if ((rc = prec(r, v))) return rc;
        if ((rc = apply(v, t))) return rc;
        double tt_tr[3];
        if ((rc = sp.mdot(t, 2, t, tt_tr, r, r))) return rc;                    /* t.t, r.t, r.r */
        times();
        if ((rc = set_normr(tt_tr[2]))) return rc;
        if (normr <= tolb) break;
        const double nt = sqrt0(tt_tr[0]), ts = tt_tr[1];
        if (!(nt > 0.0) || !std::isfinite(ts)) return nonfinite();
        const double rho = std::fabs(ts / (nt * normr));
        om = ts / (nt * nt);
        if (rho < angle) om = om * angle / rho;                                 /* calc_omega */
        sp.lincomb2(1.0, r, {-om}, {t}, 1.0, x, {om}, {v});
        if (opt->idr_replace) {
            if ((rc = replace_norm())) return rc;
            if (trueres && normr < normb) {
                /* residual replacement: r = b - A x */
                if ((rc = sp.apply(x, r))) return rc;
                sp.axpby(1.0, b, -1.0, r, r);
                trueres = false;
                inf.reorth++;
            }
        }
        iter++;
    }
    double rr = 0.0;                                                            /* the final r */
    if (!done && ((rc = sp.norm2(r, &rr)) || (rc = set_normr(rr)))) return rc;
    inf.iters = iter;
    inf.implicit_rel_res = normr / normb;
    inf.converged = normr <= tolb;
    return 0;
}

}  // namespace iemic

#endif
