/*
 * hessenberg.h -- the least-squares problem of a GMRES cycle: the Hessenberg matrix reduced
 * to triangular form by Givens rotations as its columns arrive, the rotated right-hand side
 * g, and the back substitution.  Shared by the three Arnoldi loops (krylov.hip: DGKS and
 * DCGS2; coupled_krylov.hip), which differ only in how they produce a column.
 *
 * Plain C++, no HIP include: it compiles on the host alone (tests/emul/hessenberg_driver.cpp).
 *
 * Rounding: krylov.o is built with floating-point contraction allowed and coupled_krylov.o
 * without; both must keep the bits they had when each loop carried its own copy.  Every
 * member therefore turns contraction off for its own body (`#pragma clang fp contract(off)`
 * at block scope, not at the top of the file: a file-scope pragma would also reach the device
 * kernels that follow the include in krylov.hip).  This is what was done, and it leaves the
 * ocean solve bitwise equal: the host objects target baseline x86-64, which has no fused
 * multiply-add, so contraction never applied to these loops.
 */
#ifndef IEMIC_HESSENBERG_H
#define IEMIC_HESSENBERG_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace iemic {

struct Hessenberg {
    int m;                           /* columns; H is (m + 1) x m, row-major            */
    std::vector<double> H, cs, sn, g;
    explicit Hessenberg(int m_) : m(m_), H((size_t)(m_ + 1) * m_, 0.0), cs(m_), sn(m_), g(m_ + 1) {}

    /* a cycle starts from a residual of norm beta: g = beta e_1 */
    void reset(double beta)
    {
        std::fill(g.begin(), g.end(), 0.0);
        g[0] = beta;
    }

    /* column q = [col[0..q]; hn]: the rotations 0..q-1 applied, rotation q formed and applied
     * to the column and to g.  Returns |g[q+1]|, the residual norm of the least-squares
     * problem over the columns 0..q. */
    double push_column(int q, const double* col, double hn)
    {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        for (int i = 0; i <= q; i++) H[(size_t)i * m + q] = col[i];
        H[(size_t)(q + 1) * m + q] = hn;
        for (int i = 0; i < q; i++) {
            const double x0 = H[(size_t)i * m + q], x1 = H[(size_t)(i + 1) * m + q];
            H[(size_t)i * m + q] = cs[i] * x0 + sn[i] * x1;
            H[(size_t)(i + 1) * m + q] = -sn[i] * x0 + cs[i] * x1;
        }
        const double x0 = H[(size_t)q * m + q], x1 = H[(size_t)(q + 1) * m + q];
        const double d = std::sqrt(x0 * x0 + x1 * x1);
        cs[q] = d > 0 ? x0 / d : 1.0;
        sn[q] = d > 0 ? x1 / d : 0.0;
        H[(size_t)q * m + q] = d;
        H[(size_t)(q + 1) * m + q] = 0.0;
        g[q + 1] = -sn[q] * g[q];
        g[q] = cs[q] * g[q];
        return std::fabs(g[q + 1]);
    }

    /* y[0..k) = R \ g over the first k columns */
    void solve(int k, double* y) const
    {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        for (int i = k - 1; i >= 0; i--) {
            double t = g[i];
            for (int q = i + 1; q < k; q++) t -= H[(size_t)i * m + q] * y[q];
            y[i] = t / H[(size_t)i * m + i];
        }
    }
};

}  // namespace iemic

#endif
