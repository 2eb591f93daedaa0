/*
 * schur_cr.h -- block cyclic reduction of a block tridiagonal (periodic) system: the state
 * SchurCR, what its members need, and the entry points (cr_plan.hip: cr_init; cr_factor.hip:
 * set-up; schur_cr.hip: the apply; cr_inv.hip: the batched Gauss-Jordan inverse).  Its users:
 * the block GS's 2-D Schur complement (BlockGS::cr), the T/S multigrid's coarsest level
 * (TsMg::cr) and the atmosphere's two solvers.  Included by common.h, after DevBuf.
 *
 * m x m blocks, column-major; level l has N[l] blocks (N[nlev] = 1).
 */
#ifndef IEMIC_SCHUR_CR_H
#define IEMIC_SCHUR_CR_H

namespace iemic {

/* the largest block: k_cr_inv's register classes, k_cr_pk's staged vectors */
constexpr int CR_BLOCK_MAX = 192;

struct CrGemm {                      /* C = C0 + C0b + s1 A1 B1 + s2 A2 B2                 */
    double* C;
    const double *C0, *C0b, *A1, *B1, *A2, *B2;
    double s1, s2;
};
/* matrix terms of one output block of an apply step, y = sum_t s_t A_t v_t */
constexpr int CR_MT = 8;
/* C = sum_k s_k A_k B_k (B_k null: s_k A_k; A_k null: s_k I), a composite operator */
struct CrComp {
    double* C;
    int nt;
    const double* A[4];
    const double* B[4];
    double s[4];
};
/* Packed apply step.  The matrix terms of every (output block, row chunk of rc rows) --
 * one workgroup -- are copied at set-up, scaled, into one contiguous run of the step's
 * buffer P: term-major, then column, then the chunk's rc rows, so a wave reads 512
 * contiguous bytes per load and no two workgroups share a cache line.  The workgroups are
 * sorted by their number of matrix terms into at most CR_NCLS classes, whose bounds travel
 * as kernel arguments: a workgroup finds its run in P without a memory load and issues its
 * matrix loads at once; only the vector references (CrWg) come from memory. */
constexpr int CR_NCLS = 8;
struct CrCls {
    int ncls;
    int w0[CR_NCLS + 1];             /* first workgroup of each class (w0[ncls] = nwg)     */
    int nA[CR_NCLS];                 /* matrix terms per workgroup of the class            */
    int64_t p0[CR_NCLS];             /* first double of the class in P                     */
};
struct CrWg {                        /* vectors of one workgroup                           */
    int yref, r0;                    /* output (cr_vref, cr_internal.h), first row         */
    int nv, hasid;                   /* vector terms; the last is the identity (scale 1)   */
    int vref[CR_MT];                 /* cr_vref                                            */
};
struct CrPack {                      /* set-up copy: P[dst + c rc + rr] = s A[r0 + rr, c]  */
    const double* A;
    double s;
    int64_t dst;
    int r0;
};
struct CrStep {                      /* one apply launch                                  */
    int nwg = 0, rc = 16;            /* workgroups, rows per chunk                        */
    int nl = 1;                      /* levels the step spans (1 or 2)                    */
    CrCls cls{};
    DevBuf<CrWg> wg;
    DevBuf<double> P;
    DevBuf<CrPack> jobs;
    int njobs = 0;
};
struct SchurCR {
    int n = 0, m = 0, periodic = 0, nlev = 0;
    std::vector<CrStep> down, up;    /* apply steps above the tail: one or two levels each */
    DevBuf<double> cmat;             /* composite operators                              */
    DevBuf<CrComp> cdesc;            /* their products (set-up)                          */
    int ncomp = 0;
    std::vector<int> N, per, merge;  /* blocks, periodic coupling, periodic pair merged   */
    std::vector<size_t> dlr_off;     /* level l: D, L, R blocks (3 N[l])                  */
    std::vector<size_t> ap_off;      /* level l: XL, XR (evens), Dinv, YL, YR (odds)       */
                                     /* (cr_ops, cr_internal.h); level nlev: the last      */
                                     /* block's inverse                                   */
    std::vector<size_t> v_off;       /* level vectors b_l, x_l (l >= 1)                   */
    std::vector<int> g_off, g_cnt;   /* GEMM descriptor ranges: 3 per level               */
    int lt = 0, tM = 0;              /* dense tail: levels >= lt as one explicit inverse  */
    std::vector<size_t> tb_off;      /* tail set-up: batched level vectors, tM columns    */
    DevBuf<double> dlr, ap, bv, xv;
    DevBuf<double> tinv, tb, tx;     /* tail inverse (row-major tM x tM), set-up batches  */
    DevBuf<CrGemm> gd;
    DevBuf<int> info;
};
/* level sizes, storage, descriptors and apply steps for n blocks of m <= CR_BLOCK_MAX (host,
 * once per grid).  tail_max: the dense tail starts at the first level of at most tail_max
 * unknowns (0: the apply's default, 1024; n m: the whole problem, whose inverse cr.tinv is
 * then built) */
int cr_init(iemic_ctx* c, SchurCR& cr, int n, int m, int periodic, int tail_max = 0);
/* set-up from the 9-point rows / from level-0 blocks already in cr.dlr (stream-ordered);
 * cr_check reads the singular-block flag back */
int cr_factor(iemic_ctx* c, SchurCR& cr, const double* S9, const int* col_of_ij);
int cr_factor_blocks(iemic_ctx* c, SchurCR& cr);
int cr_check(iemic_ctx* c, SchurCR& cr);
/* x = S^-1 b; xT: the solution also as j * n + i */
int cr_solve(iemic_ctx* c, const SchurCR& cr, const double* b, double* x, hipStream_t s, double* xT = nullptr);
/* Gauss-Jordan inverses of m x m column-major blocks (m <= CR_BLOCK_MAX), *info set on a
 * zero pivot: one block; src blocks s0 + k sstep (k < count) into dst blocks k */
int cr_inverse_dev(hipStream_t s, int m, const double* src, double* dst, int* info);
int cr_inverse(hipStream_t s, int m, int count, const double* src, int s0, int sstep, double* dst, int* info);

}  // namespace iemic

#endif
