/*
 * cr_inv.hip -- batched Gauss-Jordan inverse of m x m column-major blocks (m <= CR_BLOCK_MAX)
 * in registers, one workgroup per block: the odd blocks of every cyclic-reduction level
 * (cr_factor.hip) and, on its own, the T/S multigrid's small dense coarsest operator
 * (ts_mg_setup.hip).
 */
#include "common.h"

namespace iemic {

namespace {

/* Gauss-Jordan inverse with partial pivoting of src block (s0 + blockIdx.x * sstep) into
 * dst block blockIdx.x (m x m column-major, m <= TR RA, m <= 32 RB), in place in registers:
 * 32 TR threads as a TR x 32 grid, thread (tr, tc) holds rows tr + TR x and columns
 * tc + 32 y.  Rows are never swapped: step k takes the unused row p with the largest
 * |a(p, k)|, scales it, eliminates column k from every other row, and column k -- dead in
 * the eliminated matrix -- keeps column p of the inverse's row-permuted form (the in-place
 * trick), so the result is written out through the two permutations (row p_k of the
 * storage is row k of the inverse, storage column k is its column p_k).  The step loop is
 * unrolled over blocks of TR steps, so the register column of k is a compile-time index;
 * the pivot row's register row is selected under a branch on its row lane.
 * One barrier per step (round 6; two before): the owners of column k + 1 write it to LDS and
 * search its pivot right after their step-k update, and every thread takes the pivot row's
 * entries of its own columns from the lane of thread (p's row lane, its column lane) -- the
 * threads of one column lane are TR consecutive lanes of one wave -- by a cross-lane read
 * instead of a second LDS round.  Same operations in the same order: the inverse is bitwise
 * the two-barrier kernel's.  A zero pivot sets *info. */
template <int TR, int RA, int RB>
__device__ __forceinline__ void cr_inv_pivot(const double* cv, unsigned used, int m, int k, int tr,
                                             double* __restrict__ pcol, int* __restrict__ s_p,
                                             int* __restrict__ piv_row, int* __restrict__ step_of,
                                             int* __restrict__ info)
{
    double best = -1.0;
    int bi = m;
#pragma unroll
    for (int x = 0; x < RA; x++) {
        const int i = tr + TR * x;
        const double v = cv[x];
        if (i < m) pcol[i] = v;
        /* a NaN candidate counts as 0, so some unused row is always taken and step_of /
         * piv_row stay a permutation (the zero pivot sets *info) */
        const double av = (i < m && !((used >> x) & 1u)) ? (v == v ? fabs(v) : 0.0) : -1.0;
        if (av > best) { best = av; bi = i; }
    }
#pragma unroll
    for (int o = 1; o < TR; o <<= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (tr == 0) {
        if (!(best > 0.0)) *info = 1;
        *s_p = bi;
        piv_row[k] = bi;
        step_of[bi < m ? bi : 0] = k;
    }
}

template <int TR, int RA, int RB>
__global__ void __launch_bounds__(32 * TR) k_cr_inv(const double* __restrict__ src, int s0, int sstep,
                                                     double* __restrict__ dst, int m, int* __restrict__ info)
{
    const size_t mm = (size_t)m * m;
    const double* A = src + (size_t)(s0 + blockIdx.x * sstep) * mm;
    double* X = dst + (size_t)blockIdx.x * mm;
    const int t = threadIdx.x, tr = t % TR, tc = t / TR;
    const int lbase = (t & 63) - tr;                    /* lane of thread (0, tc) in this wave */
    __shared__ double pcol[2][TR * RA];
    __shared__ int s_p[2];
    __shared__ int piv_row[TR * RA], step_of[TR * RA];
    double a[RA][RB];
#pragma unroll
    for (int x = 0; x < RA; x++)
#pragma unroll
        for (int y = 0; y < RB; y++) {
            const int i = tr + TR * x, j = tc + 32 * y;
            a[x][y] = (i < m && j < m) ? A[i + (size_t)j * m] : 0.0;
        }
    unsigned used = 0;                                 /* bit x: row tr + TR x was a pivot */
    if (tc == 0) {                                     /* column 0: LDS and its pivot */
        double cv[RA];
#pragma unroll
        for (int x = 0; x < RA; x++) cv[x] = a[x][0];
        cr_inv_pivot<TR, RA, RB>(cv, used, m, 0, tr, pcol[0], &s_p[0], piv_row, step_of, info);
    }
#pragma unroll
    for (int kbr = 0; kbr < RA; kbr++) {
        const int yk = kbr * TR / 32;                   /* register column of k (compile time) */
        const int ykn = ((kbr + 1) * TR / 32) < RB ? (kbr + 1) * TR / 32 : RB - 1;   /* of the next block's first */
        for (int kk = 0; kk < TR; kk++) {
            const int k = kbr * TR + kk;
            if (k >= m) break;
            const int sel = k & 1, kc = k & 31;
            __syncthreads();                            /* column k and its pivot in LDS */
            const int p = __builtin_amdgcn_readfirstlane(s_p[sel]);
            const int pr = p % TR, pa = p / TR;
            if (tr == pr) used |= 1u << pa;
            /* the pivot row's entries of this thread's columns: thread (pr, tc)'s registers */
            double prw[RB];
#pragma unroll
            for (int y = 0; y < RB; y++) {
                double mine = a[0][y];
#pragma unroll
                for (int x = 1; x < RA; x++)
                    if (x == pa) mine = a[x][y];
                prw[y] = __shfl(mine, lbase + pr, 64);
            }
            /* scale row p, eliminate column k from the other rows; column k keeps the
             * inverse's column (1 / piv in row p, -a(i, k) / piv elsewhere) */
            const double piv = pcol[sel][p];
            const double inv = piv != 0.0 ? 1.0 / piv : 0.0;
            double pr_s[RB];
#pragma unroll
            for (int y = 0; y < RB; y++) {
                const int j = tc + 32 * y;
                pr_s[y] = j < m ? prw[y] * inv : 0.0;
            }
            const bool colk = tc == kc;
#pragma unroll
            for (int x = 0; x < RA; x++) {
                const int i = tr + TR * x;
                const double f = i < m ? pcol[sel][i] : 0.0;
#pragma unroll
                for (int y = 0; y < RB; y++) {
                    if (y == yk && colk) a[x][y] = -f * inv;
                    else a[x][y] -= f * pr_s[y];
                }
            }
            if (tr == pr) {
#pragma unroll
                for (int x = 0; x < RA; x++)
                    if (x == pa)
#pragma unroll
                        for (int y = 0; y < RB; y++) a[x][y] = (y == yk && colk) ? inv : pr_s[y];
            }
            /* column k + 1 (updated above) to LDS and its pivot, by its owners */
            if (k + 1 < m && tc == ((k + 1) & 31)) {
                double cv[RA];
#pragma unroll
                for (int x = 0; x < RA; x++) cv[x] = kk + 1 < TR ? a[x][yk] : a[x][ykn];
                cr_inv_pivot<TR, RA, RB>(cv, used, m, k + 1, tr, pcol[sel ^ 1], &s_p[sel ^ 1], piv_row,
                                         step_of, info);
            }
        }
    }
    __syncthreads();
    /* storage (i, k) = inverse (step_of[i], piv_row[k]) */
#pragma unroll
    for (int x = 0; x < RA; x++)
#pragma unroll
        for (int y = 0; y < RB; y++) {
            const int i = tr + TR * x, j = tc + 32 * y;
            if (i < m && j < m) X[step_of[i] + (size_t)piv_row[j] * m] = a[x][y];
        }
}

}  // namespace

/* the inverses of src blocks s0 + k sstep (k < count) into dst blocks k, one workgroup each */
int cr_inverse(hipStream_t s, int m, int count, const double* src, int s0, int sstep, double* dst, int* info)
{
    if (count <= 0) return 0;
#define CR_INV(TR, RA, RB)                                                                           \
    hipLaunchKernelGGL((k_cr_inv<TR, RA, RB>), dim3(count), dim3(32 * TR), 0, s, src, s0, sstep, dst, m, info)
    if (m <= 32) CR_INV(16, 2, 1);
    else if (m <= 64) CR_INV(16, 4, 2);
    else if (m <= 96) CR_INV(16, 6, 3);
    else if (m <= 128) CR_INV(32, 4, 4);
    else if (m <= 160) CR_INV(32, 5, 5);
    else if (m <= CR_BLOCK_MAX) CR_INV(32, 6, 6);
    else {
        set_error("Schur cyclic reduction: more than " + std::to_string(CR_BLOCK_MAX) + " latitudes");
        return IEMIC_EINVAL;
    }
    static_assert(CR_BLOCK_MAX == 32 * 6, "the largest register class holds the largest block");
#undef CR_INV
    HIP_OK(hipGetLastError());
    return 0;
}

/* the inverse of one block on the device */
int cr_inverse_dev(hipStream_t s, int m, const double* src, double* dst, int* info)
{
    return cr_inverse(s, m, 1, src, 0, 1, dst, info);
}

}  // namespace iemic
