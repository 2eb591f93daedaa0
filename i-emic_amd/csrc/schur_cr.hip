/*
 * schur_cr.hip -- exact solve of the 2-D (barotropic) Schur complement of the block
 * Gauss-Seidel preconditioner by block cyclic reduction over longitudes.
 *
 * The pinned Schur matrix S (prec_gs.hip, step 3; the depth-averaged pressure problem that
 * TRIOS::BlockPreconditioner solves iteratively with AztecOO/ML, TRIOS_BlockPreconditioner.C:
 * 1479-1611 SolveLower1 and 2113-2173 Compute) couples water column (i, j) only to
 * (i+di, j+dj), |di|, |dj| <= 1.  Numbered c = i*m + j it is block tridiagonal in i with
 * m x m blocks (periodic in i for a periodic grid):
 *     L_i x_{i-1} + D_i x_i + R_i x_{i+1} = b_i .
 * Cyclic reduction eliminates the odd blocks of every level,
 *     D'_e = D_e - L_e D_{e-1}^-1 R_{e-1} - R_e D_{e+1}^-1 L_{e+1},
 *     L'_e = -L_e D_{e-1}^-1 L_{e-1},  R'_e = -R_e D_{e+1}^-1 R_{e+1},
 * halving the block count per level (ceil(log2 n) levels, a direct coupling kept where an
 * odd count leaves two even blocks adjacent across the periodic wrap, the two couplings of
 * a periodic pair merged), down to one m x m block.  Set-up per level: one Gauss-Jordan
 * inverse per odd block (one workgroup each) and two batched GEMM launches; the apply is one
 * GEMV launch per level down and one per level up.  The deepest levels (the first level of
 * at most 1024 unknowns and below) form a dense tail: its explicit inverse is built at set-up
 * by running those levels on the identity, and the apply replaces their 2 (nlev - lt) + 1
 * launches with one GEMV (9 -> 1 at 2 degrees).  Cost: O(n m^3) set-up flops spread over
 * n/2 workgroups per level and O(n m^2) apply bytes -- against the O(ncol^2) dense inverse
 * and the single-workgroup band LU it replaces.  Land columns are identity rows; pivoting
 * happens inside the diagonal blocks only (tested against the band LU with partial
 * pivoting of the CPU twin, oracle/prec_oracle.c).
 *
 * Every m x m block is stored column-major: a(r, c) at [r + c*m].
 *
 * This unit is the apply (k_cr_pk, k_cr_tail, cr_solve).  The plan -- levels, storage, the apply
 * steps and their packing -- is cr_plan.hip, the set-up cr_factor.hip, the Gauss-Jordan
 * inverse cr_inv.hip; schur_cr.h holds the state, cr_internal.h what the four share.
 */
#include "cr_internal.h"

namespace iemic {

namespace {

/* dense tail, apply: x = Tinv b (row-major, M <= CR_TAIL_MAX), one wave per row, b staged
 * in LDS; every load of the row is issued before the first multiply (up to 32 per lane,
 * eight independent accumulators), then a fixed shuffle tree (deterministic) */
__global__ void __launch_bounds__(256) k_cr_tail(const double* __restrict__ Tinv, const double* __restrict__ b,
                                                 double* __restrict__ x, int M, double* __restrict__ xT, int nT, int m)
{
    __shared__ double vb[CR_TAIL_MAX];
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const double* A = Tinv + (size_t)(r < M ? r : 0) * M;
    constexpr int NL = CR_TAIL_MAX / 64;
    double a[NL];
#pragma unroll
    for (int u = 0; u < NL; u++) {
        const int c = lane + 64 * u;
        a[u] = c < M ? A[c] : 0.0;
    }
    for (int c = threadIdx.x; c < M; c += 256) vb[c] = b[c];
    __syncthreads();
    if (r >= M) return;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < NL; u++) {
        const int c = lane + 64 * u;
        if (c < M) acc[u & 7] += a[u] * vb[c];
    }
    double v = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) {
        x[r] = v;
        if (xT) xT[(int64_t)(r % m) * nT + r / m] = v;   /* a tail holding the whole problem */
    }
}

/* Apply step (packed, CrStep): workgroup w computes rows [r0, r0 + RC) of one output block,
 * y = sum_t A_t v_t (+ v_id), its nA scaled matrix terms read from its own run of P
 * (term, column, row; thread = (row, column group) with the row fastest; default load
 * policy: non-temporal loads measured 44 against 39 us per solve).  The class
 * bounds are kernel arguments, so the matrix loads are issued before the vector references
 * arrive; the vectors are staged in LDS meanwhile.  Per row the column groups' partial sums
 * meet by a fixed shuffle tree inside each wave and in LDS across the four waves
 * (deterministic). */
template <int RC, int CPT>
__global__ void __launch_bounds__(256) k_cr_pk(const double* __restrict__ P, const CrCls cls,
                                               const CrWg* __restrict__ wgs, int m, const double* __restrict__ b,
                                               double* __restrict__ x, double* __restrict__ bv,
                                               double* __restrict__ xv, double* __restrict__ xT, int nT)
{
    constexpr int G = 256 / RC;
    __shared__ double vs[CR_MT + 1][CR_BLOCK_MAX];
    __shared__ double red[4][RC];
    const int w = blockIdx.x;
    int k = 0;
#pragma unroll
    for (int q = 1; q < CR_NCLS; q++)
        if (q < cls.ncls && w >= cls.w0[q]) k = q;
    const int nA = cls.nA[k];
    const double* __restrict__ Pw = P + cls.p0[k] + (int64_t)(w - cls.w0[k]) * nA * m * RC;
    const int t = threadIdx.x, g = t / RC, rr = t % RC;
    double a[CR_MT][CPT];
#pragma unroll
    for (int q = 0; q < CR_MT; q++)
#pragma unroll
        for (int u = 0; u < CPT; u++) {
            const int c = g + G * u;
            a[q][u] = (q < nA && c < m) ? Pw[((int64_t)q * m + c) * RC + rr] : 0.0;
        }
    const CrWg& d = wgs[w];
    const int nv = d.nv;
    const double* base[4] = {b, x, bv, xv};
    {
        /* (vector, element) pairs dealt over the lanes, all loads before the first store */
        constexpr int SPT = ((CR_MT + 1) * CR_BLOCK_MAX + 255) / 256;
        const int tot = nv * m;
        double v[SPT];
        int qv[SPT], cv[SPT], refs[CR_MT];
#pragma unroll
        for (int q = 0; q < CR_MT; q++) refs[q] = d.vref[q];
#pragma unroll
        for (int i = 0; i < SPT; i++) {
            const int e = t + 256 * i;
            qv[i] = e < tot ? e / m : 0;
            cv[i] = e < tot ? e - qv[i] * m : -1;
            int ref = refs[0];
#pragma unroll
            for (int q = 1; q < CR_MT; q++)
                if (qv[i] == q) ref = refs[q];
            v[i] = cv[i] >= 0 ? base[cr_vref_base(ref)][cr_vref_off(ref) + cv[i]] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < SPT; i++)
            if (cv[i] >= 0) vs[qv[i]][cv[i]] = v[i];
    }
    __syncthreads();
    const int r = d.r0 + rr;
    double acc = (d.hasid && g == 0 && r < m) ? vs[nv - 1][r] : 0.0;
#pragma unroll
    for (int q = 0; q < CR_MT; q++) {
        if (q >= nA) break;
        double p = 0.0;
#pragma unroll
        for (int u = 0; u < CPT; u++) {
            const int c = g + G * u;
            if (c < m) p += a[q][u] * vs[q][c];
        }
        acc += p;
    }
    /* lanes of one row within a wave are RC apart */
#pragma unroll
    for (int o = 32; o >= RC; o >>= 1) acc += __shfl_xor(acc, o, 64);
    const int lane = t & 63, wave = t >> 6;
    if (lane < RC) red[wave][lane] = acc;
    __syncthreads();
    if (t < RC && r < m) {
        const double sum = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        double* const ys[4] = {nullptr, x, bv, xv};
        const int yb = cr_vref_base(d.yref), yo = cr_vref_off(d.yref);
        ys[yb][yo + r] = sum;
        /* the solution also transposed (row j of block i at j * n + i) for its consumers,
         * whose lanes run along i */
        if (xT && yb == 1) xT[(int64_t)r * nT + yo / m] = sum;
    }
}

}  // namespace

/* one apply step: the k_cr_pk instance of its chunk size and of m's columns per thread */
static void cr_step(const SchurCR& cr, const CrStep& st, const double* b, double* x, hipStream_t s,
                    double* xT = nullptr)
{
    const int m = cr.m;
    double* bv = const_cast<double*>(cr.bv.p);
    double* xv = const_cast<double*>(cr.xv.p);
    const dim3 g((unsigned)st.nwg), blk(256);
    const int nT = cr.N[0];
#define CR_PK(RC, CPT) hipLaunchKernelGGL((k_cr_pk<RC, CPT>), g, blk, 0, s, (const double*)st.P.p, st.cls, \
                                          (const CrWg*)st.wg.p, m, b, x, bv, xv, xT, nT)
    if (st.rc == 16) {
        if (m <= 80) CR_PK(16, 5);
        else CR_PK(16, 12);
    } else if (st.rc == 8) {
        if (m <= 96) CR_PK(8, 3);
        else CR_PK(8, 6);
    } else {
        if (m <= 128) CR_PK(4, 2);
        else CR_PK(4, 3);
    }
#undef CR_PK
}

/* x = S^-1 b (b, x: n*m, c = i*m + j): the levels above the tail in packed apply steps of one
 * or two levels each way (k_cr_pk), the tail (levels >= lt, tM = N[lt] m unknowns) one dense
 * GEMV (k_cr_tail); without a tail the last block by k_cr_final */
int cr_solve(iemic_ctx* c, const SchurCR& cr, const double* b, double* x, hipStream_t s, double* xT)
{
    (void)c;
    if (cr.tM > CR_TAIL_MAX) {             /* k_cr_tail holds b and a row in arrays of that size */
        set_error("Schur cyclic reduction: a dense tail of " + std::to_string(cr.tM) + " unknowns (more than " +
                  std::to_string(CR_TAIL_MAX) + ") has no apply kernel");
        return IEMIC_EINVAL;
    }
    auto bvec = [&](int l) { return l == 0 ? b : cr.bv.p + cr.v_off[l]; };
    auto xvec = [&](int l) { return l == 0 ? x : cr.xv.p + cr.v_off[l]; };
    const int le = cr.tM ? cr.lt : cr.nlev;
    for (const CrStep& st : cr.down) cr_step(cr, st, b, x, s);
    if (cr.tM)
        hipLaunchKernelGGL(k_cr_tail, dim3((cr.tM + 3) / 4), dim3(256), 0, s, (const double*)cr.tinv.p, bvec(le),
                           xvec(le), cr.tM, le == 0 ? xT : nullptr, cr.N[0], cr.m);
    else
        cr_final(cr, bvec(le), xvec(le), 1, s);
    for (const CrStep& st : cr.up) cr_step(cr, st, b, x, s, xT);
    if (xT && le == 0 && !cr.tM)           /* one block (n = 1): the transposed order is x's */
        HIP_OK(hipMemcpyAsync(xT, x, sizeof(double) * cr.m, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace iemic
