/*
 * cr_internal.h -- what the cyclic reduction's own units share (cr_plan.hip, cr_factor.hip,
 * schur_cr.hip, cr_inv.hip) and no other unit includes: the level geometry, the layout of
 * SchurCR::ap, the apply's vector references, the plan's output record and the row-chunk
 * fragment of the batched level kernels.  Each fact is written down here once.
 */
#ifndef IEMIC_CR_INTERNAL_H
#define IEMIC_CR_INTERNAL_H

#include "common.h"

namespace iemic {

/* ---- level geometry.  Level (N blocks, per: periodic) eliminates its odd blocks.  An even
 * block e has the neighbours lnb and rnb (wrapped; lex / rex: they exist); lo / ro: the
 * neighbour is odd, so it is eliminated -- otherwise (an odd count leaves two even blocks
 * adjacent across the periodic wrap) the direct coupling is kept */
struct CrEven {
    bool lex, rex;
    int lnb, rnb;
    bool lo, ro;
};
__host__ __device__ __forceinline__ CrEven cr_even(int N, int per, int e)
{
    CrEven g;
    g.lex = e > 0 || per;
    g.rex = e + 1 < N || per;
    g.lnb = e > 0 ? e - 1 : N - 1;
    g.rnb = (e + 1) % N;
    g.lo = g.lex && (g.lnb & 1);
    g.ro = g.rex && (g.rnb & 1);
    return g;
}
/* an odd block b: its left neighbour b - 1 always exists, its right one rn (even) if rex */
struct CrOdd {
    bool rex;
    int rn;
};
__host__ __device__ __forceinline__ CrOdd cr_odd(int N, int per, int b)
{
    return {b + 1 < N || per, (b + 1) % N};
}

/* ---- SchurCR::ap, level l < nlev: the five operator families, block k of a family at
 * family + k mm.  XL_q = L_e Dinv, XR_q = R_e Dinv of the even blocks e = 2q (ne of each),
 * Dinv_p, YL_p = Dinv L_o, YR_p = Dinv R_o of the odd blocks o = 2p + 1 (no of each).
 * Level nlev: the last block's inverse alone (cr_last) */
struct CrOps {
    double *XL, *XR, *Dinv, *YL, *YR;
    size_t mm;
};
inline size_t cr_ops_blocks(int Nl) { return 2 * (size_t)((Nl + 1) / 2) + 3 * (size_t)(Nl / 2); }
inline CrOps cr_ops(const SchurCR& cr, int l)
{
    const size_t mm = (size_t)cr.m * cr.m, ne = (cr.N[l] + 1) / 2, no = cr.N[l] / 2;
    double* ap = cr.ap.p + cr.ap_off[l];
    return {ap, ap + ne * mm, ap + 2 * ne * mm, ap + (2 * ne + no) * mm, ap + (2 * ne + 2 * no) * mm, mm};
}
inline double* cr_last(const SchurCR& cr) { return cr.ap.p + cr.ap_off[cr.nlev]; }

/* ---- a vector of the apply as one int (CrWg): base 0 the solve's right-hand side b, 1 its
 * solution x, 2 / 3 the internal level vectors bv / xv, and the offset of the block in it */
__host__ __device__ __forceinline__ int cr_vref(int base, int64_t off) { return (base << 28) | (int)off; }
__host__ __device__ __forceinline__ int cr_vref_base(int ref) { return ref >> 28; }
__host__ __device__ __forceinline__ int cr_vref_off(int ref) { return ref & 0x0fffffff; }

/* ---- the plan (cr_plan.hip).  One output block of a (composite) apply step:
 * y = sum_t s_t A_t v_t (A_t null: identity); vectors and output as (base, offset) of cr_vref */
struct CrOut {
    int yb, nt;
    int64_t yo;
    double s[CR_MT];
    const double* A[CR_MT];
    int vb[CR_MT];
    int64_t vo[CR_MT];
};
/* ---- dense tail: k_cr_tail stages b and a row in arrays of this size (cr_init's default
 * tail_max) */
constexpr int CR_TAIL_MAX = 1024;

/* ---- the batched level kernels k_cr_fwd / k_cr_bwd / k_cr_final (cr_factor.hip: they build
 * the tail's inverse, and k_cr_final is the last block of a solve without a tail; the packed
 * apply steps have their own chunk, CrStep::rc).  Rows [r0, r0 + CR_RC) of
 * y = y0 + s0 (A0 v0 + A1 v1 + A2 v2) for m x m column-major blocks (m <= CR_RC * CR_CPT):
 * thread = (row, column group), CR_RC rows x CR_G groups, each thread CR_CPT columns per
 * block.  The block entries are loaded into registers BEFORE the vectors arrive in LDS
 * (crf_load, then the caller's vector loads and barrier, then crf_finish), so both memory
 * latencies overlap; the groups' partial sums are added in LDS in a fixed order
 * (deterministic).  CR_RB right-hand sides per workgroup (blockIdx.y groups): the blocks are
 * read once per CR_RB columns instead of once per column. */
constexpr int CR_RC = 16, CR_G = 256 / CR_RC, CR_CPT = 12, CR_RB = 8;
static_assert(CR_RC * CR_CPT >= CR_BLOCK_MAX, "a row chunk's column groups cover the largest block");
struct CrFrag {
    double a[3][CR_CPT];
};
__device__ __forceinline__ void crf_load(CrFrag& f, const double* __restrict__ A0, const double* __restrict__ A1,
                                         const double* __restrict__ A2, int m, int r0)
{
    const int t = threadIdx.x, g = t / CR_RC, r = r0 + t % CR_RC;
    const double* A[3] = {A0, A1, A2};
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int u = 0; u < CR_CPT; u++) {
            const int c = g + CR_G * u;
            f.a[q][u] = (A[q] && r < m && c < m) ? A[q][r + (size_t)c * m] : 0.0;
        }
}
__device__ __forceinline__ void crf_finish(const CrFrag& f, const double* v0, const double* v1, const double* v2,
                                           double s0, const double* __restrict__ y0, double* __restrict__ y,
                                           int m, int r0, double* red)
{
    const int t = threadIdx.x, g = t / CR_RC, r = r0 + t % CR_RC;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int u = 0; u < CR_CPT; u++) {
        const int c = g + CR_G * u;
        if (c < m) {
            a0 += f.a[0][u] * v0[c];
            a1 += f.a[1][u] * v1[c];
            a2 += f.a[2][u] * v2[c];
        }
    }
    red[t] = (a0 + a1) + a2;
    __syncthreads();
    if (t < CR_RC && r < m) {
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < CR_G; q++) sum += red[q * CR_RC + t];
        y[r] = (y0 ? y0[r] : 0.0) + s0 * sum;
    }
}
/* x = Dfin b for nrhs right-hand sides m apart (k_cr_final; cr_factor.hip) */
void cr_final(const SchurCR& cr, const double* b, double* x, int nrhs, hipStream_t s);

}  // namespace iemic

#endif
