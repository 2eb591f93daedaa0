/*
 * krylov_internal.h -- what the ocean's Krylov units share (krylov.hip, idrs.hip): the small
 * numeric guards and the helpers of krylov.hip that IDR(s) calls.  idrs_core.h takes the guards (sqrt0, nonfinite) from here, also for the
 * coupled model; included by nothing else.
 */
#ifndef IEMIC_KRYLOV_INTERNAL_H
#define IEMIC_KRYLOV_INTERNAL_H

#include <algorithm>
#include <chrono>
#include <cmath>

#include "common.h"

namespace iemic {

/* sqrt of a squared norm that rounding may have driven below zero; NaN stays NaN */
inline double sqrt0(double v) { return v > 0.0 ? std::sqrt(v) : (v == v ? 0.0 : v); }

/* krylov.hip */
/* a NaN/Inf reaching the Hessenberg column would pass for a breakdown (res = 0): stop loudly */
int nonfinite();
double ms_since(std::chrono::steady_clock::time_point t0);
/* dot products of nvec vectors V_i (stride ldv) with w, and (ea != null) ea . eb as
 * out[nvec], in one launch pair and one host synchronisation */
/* V, w, ea, eb point at the first owned row; length nlrows; sums over the ranks */
int mdot_host(iemic_ctx* c, const double* V, int64_t ldv, int nvec, const double* w, double* out,
              const double* ea = nullptr, const double* eb = nullptr);
/* the Krylov work space: Z (m x N) and w, r always; the full-length basis V ((m+1) x N) unless
 * the basis is compressed, then Vc ((m+1) x nc) and the full-length t, b' */
int ensure_krylov(iemic_ctx* c, int m, int64_t nc = 0);
/* coefficients -> device through the pinned staging area (the previous use of the area
 * has completed: every caller synchronised the stream since) */
int upload_coeffs(iemic_ctx* c, const double* h, int n);
/* the DCGS2 update pass of one Arnoldi step on the context's stream, from the summed dot
 * rows hb (2 nv + 5 doubles): fused (coefficients formed in the update's prologue, as the
 * solve runs it) or as k_dcgs_coef + the update from its coefficient array coef (RED_ROWS
 * doubles; the reference of test_hooks.hip).  hrows: the host's pinned slot, or null */
int dcgs_update(iemic_ctx* c, bool fused, const double* Q, int64_t ldq, int nv, double* hb, double* coef,
                double* hrows, double* u, double* w, int64_t N, const int* act, int64_t own0, int64_t ps,
                double* rrP);

}  // namespace iemic

#endif
