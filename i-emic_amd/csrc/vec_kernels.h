/*
 * vec_kernels.h -- the vector kernels that the Krylov units share: the block reduction, the
 * multi-dot pair, the IDR(s) shadow-space hash, scale/copy, axpby and the linear combinations
 * of up to 16 vectors.
 * Included by spmv.hip, krylov.hip and idrs.hip (the ocean's vectors, default compiler flags)
 * and by coupled.hip and coupled_krylov.hip (the packed coupled vectors, built without
 * floating-point contraction).
 *
 * Every __global__ function here is `static`.  The two groups of units compile these
 * kernels with different contraction settings and each must keep the bits it has, so every
 * including unit gets its own copy of all six, built with its own flags.  With external
 * linkage the link would either fail or silently pick one copy for both groups.  Do not
 * remove the `static`.  A unit that launches only some of them (spmv.hip the multi-dot
 * pair and k_scale_copy, coupled.hip k_axpby) still emits all six: the unlaunched copies
 * are known and harmless, a few KB of code object each.
 *
 * k_zero is not here: dev_zero (common.h) launches it from every unit, it does no
 * arithmetic, and its one external definition stays in krylov.hip.
 *
 * The launch grids stay with the callers (grid_for in common.h, blocks_for in
 * coupled_internal.h): the loops are grid-stride and element-wise.
 */
#ifndef IEMIC_VEC_KERNELS_H
#define IEMIC_VEC_KERNELS_H

#include <vector>

#include "common.h"

namespace iemic {

/* ---- reductions ---------------------------------------------------------------------- */
__device__ __forceinline__ double block_sum(double v, double* sm)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) sm[wid] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x >> 6); w++) t += sm[w];
    return t;
}

/* partial[i * gridDim.x + blk] = sum over the block's range of V_i . w, i < nvec;
 * with extra != null, row i == nvec is extra . w (or extra . extra_w) in the same launch */
static __global__ void __launch_bounds__(256) k_mdot(const double* __restrict__ V, int64_t ldv, int nvec,
                                              const double* __restrict__ w, int64_t N,
                                              double* __restrict__ partial,
                                              const double* __restrict__ extra = nullptr,
                                              const double* __restrict__ extra_w = nullptr)
{
    __shared__ double sm[8];
    const int i = blockIdx.y;
    if (i > nvec || (i == nvec && !extra)) return;
    const double* vi = i == nvec ? extra : V + (int64_t)i * ldv;
    const double* wi = (i == nvec && extra_w) ? extra_w : w;
    double s = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        s += vi[q] * wi[q];
    double t = block_sum(s, sm);
    if (threadIdx.x == 0) partial[(int64_t)i * gridDim.x + blockIdx.x] = t;
}
/* out[i] = sum_b partial[i*nb + b]  (fixed order: deterministic) */
static __global__ void k_mdot_final(const double* __restrict__ partial, int nb, int nvec,
                             double* __restrict__ out)
{
    __shared__ double sm[8];
    const int i = blockIdx.x;
    if (i >= nvec) return;
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) s += partial[(int64_t)i * nb + b];
    double t = block_sum(s, sm);
    if (threadIdx.x == 0) out[i] = t;
}

/* ---- the IDR(s) shadow space -------------------------------------------------------------- */
/* entry q of row g: uniform in [-1, 1], splitmix64 of (g, q) from the space's seed.  The callers
 * (k_idr_random, k_cidr_random) map their threads to g */
__device__ __forceinline__ double idr_shadow_entry(uint64_t g, int q, uint64_t seed)
{
    uint64_t z = 0x9E3779B97F4A7C15ull * (g * 16 + (uint64_t)q + 1) + seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return 2.0 * ((double)(z >> 11) * (1.0 / 9007199254740992.0)) - 1.0;
}

/* ---- BLAS-1 -------------------------------------------------------------------------- */
/* b = s a */
static __global__ void k_scale_copy(const double* __restrict__ a, double s, double* __restrict__ b, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        b[q] = s * a[q];
}
static __global__ void k_axpby(double a, const double* __restrict__ x, double b, const double* __restrict__ y,
                        double* __restrict__ out, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        out[q] = a * x[q] + b * y[q];
}

/* y = a y + sum_i c_i X_i (i < nv <= 16), coefficients by value */
struct LinComb {
    int nv;
    double a;
    double c[16];
    const double* X[16];
};
/* y may also be one of the X (the IDR update of U(:,k) reads U(:,k)): no __restrict__ */
static __global__ void __launch_bounds__(256) k_lincomb(LinComb L, double* y, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        double acc = L.a == 0.0 ? 0.0 : L.a * y[q];
        for (int i = 0; i < L.nv; i++) acc += L.c[i] * L.X[i][q];
        y[q] = acc;
    }
}
/* two independent combinations in one pass (y1 = a1 y1 + sum c_i X_i, y2 likewise) */
static __global__ void __launch_bounds__(256) k_lincomb2(LinComb L1, double* y1, LinComb L2, double* y2, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        double a1 = L1.a == 0.0 ? 0.0 : L1.a * y1[q];
        for (int i = 0; i < L1.nv; i++) a1 += L1.c[i] * L1.X[i][q];
        double a2 = L2.a == 0.0 ? 0.0 : L2.a * y2[q];
        for (int i = 0; i < L2.nv; i++) a2 += L2.c[i] * L2.X[i][q];
        y1[q] = a1;
        y2[q] = a2;
    }
}
/* the combination's terms c_i (x_i + o): o the offset of the first row the launch covers */
static inline LinComb make_lc(double a, const std::vector<double>& cs, const std::vector<const double*>& xs, int64_t o)
{
    LinComb L{};
    L.a = a;
    for (size_t q = 0; q < cs.size() && q < 16; q++) {
        L.c[L.nv] = cs[q];
        L.X[L.nv] = xs[q] + o;
        L.nv++;
    }
    return L;
}

}  // namespace iemic

#endif
