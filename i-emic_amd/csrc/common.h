/*
 * common.h -- device context shared by the assembly, Krylov and preconditioner units.
 */
#ifndef IEMIC_COMMON_H
#define IEMIC_COMMON_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/iemic.h"
#include "stencil.h"
#include "host_setup.h"
#include "decomp.h"

namespace iemic {

void set_error(const std::string& s);

/* Workgroups dealt to the 8 XCDs in contiguous runs.  xcd_grid: blocks launched for nwg
 * workgroups.  xcd_block: logical workgroup of block b of such a grid: the XCDs (blocks dealt
 * round robin, b % 8) get contiguous runs of workgroups, so tiles of neighbouring latitude
 * rows, which read each other's rows, share an L2; -1: idle block */
static inline unsigned xcd_grid(int64_t nwg) { return 8u * (unsigned)((nwg + 7) / 8); }
__device__ __forceinline__ int xcd_block(int nwg)
{
    const int per = (nwg + 7) >> 3;
    const int w = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    return w < nwg ? w : -1;
}

#define HIP_OK(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            ::iemic::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));     \
            return IEMIC_EDEVICE;                                                      \
        }                                                                              \
    } while (0)

template <typename T> struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    /* grow-only: at least count elements (the contents are lost when it grows) */
    int reserve(size_t count) { return n < count ? alloc(count) : 0; }
    int alloc(size_t count)
    {
        free();
        n = count;
        if (count == 0) return 0;
        if (hipMalloc(&p, count * sizeof(T)) != hipSuccess) {
            p = nullptr;
            n = 0;
            return IEMIC_ENOMEM;
        }
        return 0;
    }
    void free()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            free();
            p = o.p; n = o.n;
            o.p = nullptr; o.n = 0;
        }
        return *this;
    }
    ~DevBuf() { free(); }
};

}  // namespace iemic

#include "schur_cr.h"              /* SchurCR (holds DevBufs), embedded in TsMg and BlockGS */

namespace iemic {

/* T/S aggregation multigrid of the block GS (ts_mg.hip, ts_mg_setup.hip; BlockGS::mg, which no
 * other unit names): 2x2 horizontal aggregates, full depth, band-local; level q has n[q] x m[q] x l
 * cells in the k-contiguous level layout (ts_mg_internal.h TsLev; level 0 packed from tsoff/tsdiag) with
 * 16 couplings, the 2x2 block, the z-line factors (12), rhs and iterate */
struct TsMg {
    static constexpr int MAX = 12;
    int sweeps = 1, nlev = 0;
    int n[MAX] = {}, m[MAX] = {};
    int par[MAX] = {};               /* colour parity of the level's cell (0, 0): global   */
                                     /* column + row offset of the subdomain's aggregates  */
    DevBuf<double> off[MAX], diag[MAX], fac[MAX], b[MAX], z[MAX];
    DevBuf<double> zu[MAX];          /* fused up leg (k_mg_up): the post-smoothed iterate      */
    DevBuf<double> cinv;             /* coarsest level: dense inverse (2 ncl)^2          */
    /* subdomains: the coarsest T/S level solved globally (all ranks' coarsest cells plus
     * the cross-subdomain couplings; band LU + inverse on the device, on every rank) */
    int glob = 0, gN = 0, gGX = 0, gI0 = 0, gJ0 = 0;
    DevBuf<double> gX, gband, gvec, gtmp, glpan;
    DevBuf<int> gpiv, ginfo, gcols;
    DevBuf<double> cdense;           /* coarsest dense operator (device assembly)        */
    /* one rank: the coarsest level is the first of <= CR_CELLS cells whose columns of
     * one longitude fit a cyclic-reduction block (2 mb l <= CR_BLOCK_MAX); its inverse (cinv,
     * in the level's unknown order) comes from a whole-problem cyclic reduction over
     * longitudes (schur_cr.h, the explicit "tail" inverse) */
    static constexpr int CR_CELLS = 1024;
    int crd = 0;
    int ckind = 0;                   /* how cinv was assembled: 0 device, 1 cyclic reduction, 2 host */
    bool nofuse = false;             /* test hook only: no level takes the fused launches    */
    /* the entry kernel's operand A_TS,D (k_mg_entry_p): the T/S rows' couplings to the dynamics
     * unknowns of the active cells, one contiguous run per tile, the identity-column slots
     * stored as 0 (k_mg_entry_pack, once per set-up from the set-up's Jacobian); etl: per
     * tile the run's start, its active cells and their mask (ts_mg_internal.h), rebuilt when
     * the active set changes (egen against ActiveSet::gen) */
    DevBuf<double> ep;
    DevBuf<uint64_t> etl;
    int64_t egen = -1, epn = 0;      /* epn: doubles of ep in use                             */
    bool nopack = false;             /* test hook only: the entry reads the slot-major Jacobian */
    int hr = 0;                      /* bands: level 0 has 2 halo rows, and its colour-1   */
                                     /* lines on them are relaxed here too (mg_vcycle)      */
    SchurCR cr;
    DevBuf<int> cinfo;               /* its Gauss-Jordan pivot flag                      */
};
/* stores sweeps; with BlockGS::ts_mg > 0: levels, Galerkin operators, z-line factors and the
 * coarsest inverse (once per Jacobian), ts_mg = 0 where the grid has no coarse level */
int ts_mg_setup(iemic_ctx* c, int sweeps);
/* BlockGS::ts_mg V-cycles on rr_TS - A_TS,D zd; z(T, S) is written when out, else by
 * ts_mg_out.  side: the V-cycles on iemic_ctx::side, ev_join recorded after them */
int ts_mg_solve(iemic_ctx* c, const double* zd, double* z, bool out, bool side);
int ts_mg_out(iemic_ctx* c, double* z);
/* the solve's first launch alone: level 0's right-hand side from BlockGS::rrP and zd, its
 * colour-0 lines relaxed (from the pack, or from the Jacobian when TsMg::nopack) */
int ts_mg_entry(iemic_ctx* c, const double* zd);
/* test_hooks.hip: the V-cycle's plan and level q as the apply leaves it (device pointers; z is
 * the iterate the level hands upward, cinv only on the coarsest level; halo: the level's
 * layout pads its rows or columns) */
struct TsMgProbe {
    int nlev, lanes, sweeps, hr, ckind;
    int n, m, par, colours, fused, halo;
    const double *off, *diag, *b, *z, *cinv;
};
int ts_mg_probe(iemic_ctx* c, int q, TsMgProbe* o);

/* band_lu.hip: band LU with partial pivoting and the explicit inverse, panels of BAND_NBP
 * columns (lpan: ceil(N / BAND_NBP) x (BAND_NBP + bl) x BAND_NBP multipliers) */
constexpr int BAND_NBP = 16;
int band_lu_inverse(iemic_ctx* c, double* ab, int N, int bl, int bu, int* piv, int* info_d, double* lpan,
                    const int* cols, double* X, int* info);

/* The compressed active-cell set and the coefficient streams packed from the Jacobian
 * (active_set.hip; BlockGS::act).  This is the part of the block GS that krylov.hip, spmv.hip and
 * assembly.hip may read; beside it they read only BlockGS::ready, kind, known, rrP, dyn_iters
 * and dyn_mr. */
struct ActiveSet {
    /* owned cells with a non-identity row (the rest: land, all six rows identity), ascending:
     * FGMRES keeps its Arnoldi basis on these cells only (krylov.hip) */
    DevBuf<int> act;
    DevBuf<int> cmap;                /* per owned cell: its index in act, -1 (land)        */
    int64_t ric = -1;                /* compressed row of the integral condition (owned)   */
    DevBuf<uint8_t> actf;            /* per owned cell: 1 active (k_cell_active)           */
    int64_t nact = 0;
    std::vector<uint8_t> act_h;      /* the per-cell flags the list was built from        */
    int64_t gen = 0;                 /* counts the rebuilds of the list (act_build)       */
    /* the compressed SpMV (spmv.hip k_spmv7c): the active cells' 104 coefficients blocked
     * per tile (k_spmv_pack: no coefficient line holds a land cell or another tile's), and
     * the grid tiles that hold an active cell (8 ints each: tile, first | last active lane
     * << 8, first active cell, active cells, 64-bit active-lane mask, 0, 0) */
    DevBuf<double> spc;
    DevBuf<int> atl;
    DevBuf<int> apos;                /* per active cell: its tile's index in atl            */
    int natile = 0;
    DevBuf<double> dvh;              /* bands: U/V/W/P coefficients of the two halo rows  */
    DevBuf<double> dvb;              /* the active cells' U/V/W/P coefficients, blocked:  */
                                     /* [act / 64][slot][act % 64] (the defect's stream)  */
    /* the Jacobian the apply reads: the set-up one (gs_refresh).  A Jacobian assembled
     * while the block GS is set up goes into the other buffer (assemble_jacobian swaps
     * iemic_ctx::d_val with vold), so the preconditioner stays the operator of its set-up
     * Jacobian on every rank, as the reference's extracted blocks do */
    const double* vp = nullptr;
    DevBuf<double> vold;
    /* a Jacobian was assembled since the set-up: the compressed SpMV's stream spc and the
     * identity-row check are redone before the next apply or solve (gs_refresh) */
    int coef_stale = 0;
    int cmp_ok = 0;                  /* the active list matches the Jacobian's identity rows */
    DevBuf<double> chk;              /* gs_refresh: identity-row mismatches (1 double)     */
};
/* the list, cmap, ric and the tiles from BlockGS::known; *changed: the list was rebuilt */
int act_build(iemic_ctx* c, bool* changed);
/* set-up: dvh, dvb and spc from the Jacobian just assembled, which vp keeps */
int act_pack_streams(iemic_ctx* c);
/* repack the coefficient copies after a new Jacobian (ActiveSet::coef_stale) */
int gs_refresh(iemic_ctx* c);

/* the plain T/S sweeps of the block GS (ts_sweeps.hip, ts_mg = 0); the multigrid's level 0 is
 * packed from tsoff */
struct TsSweeps {
    DevBuf<double> tsinv;            /* 2x2 T/S inverses per cell                       */
    DevBuf<double> tsoff;            /* compact T/S off-diagonal couplings, 16 x ncell  */
    DevBuf<double> tsc, tic, bc;     /* the same per colour (even n), T/S rhs per colour */
    DevBuf<double> zt, zs;           /* T/S iterates                                     */
    DevBuf<double> bts;              /* T/S right-hand side (AoS)                        */
};

/* Preconditioner state (prec.hip: block Jacobi; gs_setup.hip, prec_gs.hip: block Gauss-Seidel). */
struct BlockGS {
    int ready = 0;
    int kind = 0;                    /* 1: block-Jacobi, 2: block Gauss-Seidel           */
    int ts_sweeps = 3;               /* symmetric red-black sweeps on the T/S block     */
    DevBuf<double> dinv;             /* block-Jacobi: 6x6 inverses, slot-major          */
    TsMg mg;
    ActiveSet act;
    TsSweeps sw;
    /* structure (rebuilt when the identity-row pattern changes) */
    DevBuf<double> flags_d;          /* the same flags on the device (k_band_flags)       */
    std::vector<double> flags_h;     /* global (active column, U/V point) flags the      */
                                     /* structure was built for                         */
    DevBuf<int> own_pos;             /* Schur index -> itself for this band's active     */
                                     /* columns, -1 otherwise                           */
    DevBuf<int> ocol;                /* (j*n+i) -> this band's Schur rhs entry, -2 - entry */
                                     /* for a pinned column (written 0), -1 for none     */
    DevBuf<double> gslot;            /* per cell: U/V rows' P couplings (8) and the W row's */
                                     /* P couplings (2), halo-filled                     */
    DevBuf<double> rcol;             /* per owned water column: the Schur right-hand side */
                                     /* as a linear form in rr (18 x l coefficients)     */
    DevBuf<uint8_t> known;           /* per row: identity row (z = r)                   */
    DevBuf<int> col_of_ij;           /* (j*n+i) -> Schur index i*m+j, or -1 (no water)   */
    DevBuf<int> ij_of_col;           /* Schur index -> j*n+i                            */
    DevBuf<uint8_t> pinned;          /* Schur index pinned to 0 (null-space pins)       */
    /* numeric factors */
    DevBuf<double> uvinv;            /* 2x2 U/V inverses per cell                       */
    DevBuf<double> tsdiag;           /* fine 2x2 T/S blocks (active entries; k_cell_factors, */
                                     /* read by the multigrid's level 0)                 */
    DevBuf<double> pw;               /* per P row: weight of the depth integral         */
    DevBuf<uint64_t> kmask;          /* per cell: slots coupling to identity columns     */
    DevBuf<double> S9;               /* Schur rows, 9 couplings per column (i*m+j)       */
    SchurCR cr;                      /* its cyclic-reduction factors                     */
    int dyn_iters = 1;               /* defect-correction passes on the dynamics block   */
    DevBuf<double> dres, zc;         /* dynamics defect and correction (ext rows)        */
    DevBuf<double> dq, dzero, dmr;   /* MR passes: -A_DD zc, a zero vector, dot partials  */
    int dyn_mr = 0;                  /* 1: minimal-residual step length per correction   */
    double dyn_omega = 1.0;          /* fixed step of the correction passes (dyn_mr = 0) */
    int ts_at = 0;                   /* T/S rhs after this many passes (0: after all)     */
    int schur_passes = 0;            /* passes solving the Schur system: first k-1 + last (0: all) */
    int ts_mg = 1;                   /* T/S multigrid V-cycles per apply (0: the sweeps)  */
    /* the dynamics passes work on component-planar copies (plane q = unknown q of every ext
     * cell, plane stride next): known flags, iterate and right-hand side; dres, zc, dq and
     * dzero are planar too.  The AoS rr is kept for the T/S sweeps (ts_mg = 0) */
    DevBuf<uint8_t> knP;
    DevBuf<double> zP, rrP;
    DevBuf<double> colvT;            /* the Schur solution transposed (j * n + i)          */
    DevBuf<double> colvZ;            /* zeros of colvT's size: pbar of a pass without Schur  */
    DevBuf<double> rr, colv, colv2, colv_own; /* work: Schur rhs (colv_own; bands:       */
                                     /* summed into colv), solution colv2               */
};

struct Krylov {
    int m = 0;                       /* allocated basis size                            */
    DevBuf<double> V, Z;             /* (m+1) x N and m x N                             */
    DevBuf<double> w, r;
    /* DCGS2 with the block GS: the Arnoldi basis compressed to the active cells
     * (ActiveSet::act, 6 nact rows per vector), the preconditioner input rf (full, zero on
     * the land cells) and, for a right-hand side with land-cell entries, t and b' */
    int mc = 0;
    int64_t nc = 0;
    DevBuf<double> Vc, rf, t, bp;
    int zclean = 0;                  /* leading columns of Z that are zero on the identity  */
                                     /* rows of the current set-up                        */
};

/* The theta time stepper's state (theta.hip; ThetaModel.H's timestep_, theta_, oldState_,
 * oldRhs_): vectors in the ext layout, allocated at the first iemic_theta_init_step */
struct Theta {
    double theta = 1.0, dt = 0.0;
    int init = 0;                    /* a step is initialised (xold, Fold current)        */
    DevBuf<double> xold, Fold;       /* x_n and F(x_n)                                    */
    DevBuf<double> Ft, b;            /* F_theta(x) and F_theta / dt / theta (the solve's rhs) */
};

/* The stochastic theta model's state (stochastic.hip; StochasticThetaModel.H's B_ and G_), surface
 * fields of the owned cells, [(j - jb0) nx + (i - ib0)], allocated at the first use */
struct Stoch {
    DevBuf<double> coF;              /* the forcing column: forcing_cell's f[SS] with SPER = 0 */
    DevBuf<double> G;                /* the noise of the armed step                        */
    DevBuf<double> pert;             /* its m normals, global latitude index               */
    int64_t gen = -1;                /* iemic_ctx::frc_gen when coF was computed (-1: never) */
    int armed = 0;                   /* theta_rhs adds G (iemic_theta_init_step_noise)     */
};

/* The projected theta model (projected.hip; ProjectedThetaModel.H's V_, smallState_, oldState_,
 * oldRhs_, VMV_, VAVmat_ / VAVsolver_ and StochasticProjectedThetaModel.H's G_): the state is
 * confined to x = V y.  V is fixed for the life of the basis and its halo is exchanged once, when
 * it is set; the small quantities live on the host, identical on every rank. */
constexpr int SPMM_MAX_K = 64;       /* most columns of a basis / a block product         */
constexpr int SPMM_KB = 4;           /* columns per k_spmm7 launch (measured)  */
constexpr int GRAM_T = 4;            /* k_gram: a workgroup's GRAM_T x GRAM_T result tile  */
constexpr int GRAM_BLOCKS = 256;     /* its row blocks: the partials of one entry          */
struct Projected {
    int k = 0;                       /* columns of V (0: no basis)                        */
    int init = 0;                    /* a step is initialised                             */
    int armed = 0;                   /* proj_rhs adds G (iemic_proj_init_step_noise)      */
    int r_valid = 0;                 /* r is the residual at the current small state      */
    int kbmax = 0;                   /* test hook only: columns per k_spmm7 launch (0: SPMM_KB) */
    double dt = 0.0, theta = 1.0;
    DevBuf<double> V, W;             /* k x nerows each: the basis and J2 V / scratch      */
    DevBuf<double> xold;             /* the state at the init step (proj_restore)         */
    DevBuf<double> part, res;        /* k_gram's partials (k^2 GRAM_BLOCKS) and results (k^2) */
    std::vector<double> y, yn, Fn;   /* small state, V^T x_n, V^T F(x_n)                   */
    std::vector<double> yold;        /* the small state at the init step (proj_restore)   */
    std::vector<double> VMV, VAV, LU;/* V^T B V, V^T J2 V (row-major k x k) and its factors */
    std::vector<int> piv;
    std::vector<double> G, r;        /* the step's noise V^T (B_f pert ...), the residual  */
};

/* The rare-event score function's reference states (score.hip; ScoreFunctions.C's sol1, sol2, nrm
 * and dist_factor): device copies in the ext layout, kept from iemic_score_set to iemic_score_clear */
struct Score {
    int set = 0;
    int var = -1;                    /* 0..5: the rows NUN cell + var; -1: every owned row   */
    double nrm = 0.0;                /* ||sol1 - sol2||_v                                   */
    double dist_factor = 0.5;        /* ||sol1 - sol3||_v / nrm, 0.5 without sol3           */
    DevBuf<double> s1, s2;           /* sol1, sol2                                          */
    DevBuf<double> part, res;        /* k_sqdist2's partials (2 GRAM_BLOCKS) and the two sums */
};

/* A shift-invert Arnoldi run (eigs.hip): the basis of (J - sigma B)^-1 B and its work vectors,
 * ext layout, allocated by eigs_begin and freed by eigs_end */
struct Eigs {
    int active = 0;                  /* a run is in progress (V, t, w current)            */
    int m = 0, j = 0;                /* basis size of the run, steps taken                */
    int broke = 0;                   /* the last step found an invariant subspace         */
    double sigma = 0.0;
    DevBuf<double> V;                /* (m + 1) x nerows                                  */
    DevBuf<double> t, w;             /* B v_j (the solve's rhs) and the solve's output    */
    DevBuf<double> lo;               /* 2 x nerows: the low parts of eigs_residual's products */
};

constexpr int RED_BLOCKS = 1024;     /* partial-sum blocks of the reductions            */
/* the larger of a running maximum v and the next value a; a NaN on either side wins (it is
 * taken, and nothing is larger than it afterwards) */
__host__ __device__ inline double nanmax(double v, double a) { return (a > v || a != a) ? a : v; }
/* nanmax of v over a block of 256 threads, in thread 0 (sm: 4 doubles of LDS) */
__device__ inline double block_nanmax(double v, double* sm)
{
    for (int o = 32; o > 0; o >>= 1) v = nanmax(v, __shfl_down(v, o, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = sm[0];
        for (int w = 1; w < 4; w++) v = nanmax(v, sm[w]);
    }
    return v;
}
constexpr int MAX_KRYLOV = 1000;     /* largest Krylov dimension                        */
/* reduction rows (DCGS2: 2 per basis vector + 3 sums + beta, h_jj; the coefficient area
 * d_hbuf[RED_ROWS..] holds 2 per basis vector and 1/beta, gamma at DCGS_SCAL) */
constexpr int RED_ROWS = 2 * MAX_KRYLOV + 8;
constexpr int DCGS_SCAL = 2 * MAX_KRYLOV + 2;

}  // namespace iemic

struct iemic_ctx {
    iemic_grid cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;      /* second stream (one rank): the early T/S V-cycles,  */
                                     /* the T/S set-up beside the Schur factorisation      */
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int serial_setup = 0;            /* IEMIC_SERIAL_SETUP=1 at creation: gs_compute keeps the  */
                                     /* Schur and T/S set-up chains on one stream            */
    int n = 0, m = 0, l = 0;
    int64_t ncell = 0, nrows = 0;    /* global cells / rows                               */
    int64_t rowintcon = -1;          /* ext row of the integral condition if owned        */
    double int_correction = 0.0;     /* THCM::intCorrection_ (setIntCondCorrection)      */
    void* comm = nullptr;            /* ncclComm_t when nranks > 1 over RCCL              */
    void* group = nullptr;           /* in-process rank group (test facility), else null  */
    iemic_transport tp{};            /* host transport (tp.send != null), else RCCL/group  */
    iemic::DevBuf<double> d_stage;   /* packed strided messages (RCCL)                    */
    std::vector<double> h_stage;     /* host-staged messages (group / host transport)     */
    int64_t stat[4] = {0, 0, 0, 0};  /* exchange batches, messages, bytes sent, all-reduces */
    /* fail-fast (comm.hip): every host wait of an RCCL context (stream / event + async-error
     * polling, then ncclCommAbort) and every barrier of the in-process group is bounded by
     * this (IEMIC_COMM_TIMEOUT or 300 s at creation); the first all-reduce and halo batch
     * name their batch (bits of comm_checked: 1 all-reduce, 2 halo) */
    double comm_timeout_s = 300.0;
    int comm_checked = 0;
    iemic::host::Setup su;           /* grid tables, parameters, effective mask */
    const iemic::Sub& sub = su;      /* this rank's Decomp2D subdomain and ext layout: su's record (decomp.h) */
    /* device tables */
    iemic::DevBuf<int> d_landm;
    iemic::DevBuf<double> d_tab;     /* cos_y | cos_yv | tan_yv | sin_yv | amh_y | bmh_y |
                                        amh_yv | bmh_yv | bmhy_yv | dfzT | dfzW          */
    iemic::DevBuf<double> d_ftab;    /* forcing tables wfun(yv), temfun(y), salfun(y), spert */
    iemic::DevBuf<double> d_frc;     /* Frc (forcing.F90), before boundaries zeroing     */
    iemic::DevBuf<double> d_qcor;    /* qint corrections                                 */
    iemic::DevBuf<double> d_intc;    /* intcond coefficients (THCM.C:2549)               */
    iemic::DevBuf<double> d_atm;     /* coupled: tatm | qatm | albe (n*m each, surface)  */
    /* inserted forcing fields emip | adapted_emip | spert | tatm (n*m each; allocated at the
     * first insert) and which of them are set (Geo::ins_*, null otherwise) */
    iemic::DevBuf<double> d_ins;
    int ins_on[4] = {0, 0, 0, 0};
    /* state and operator */
    iemic::DevBuf<double> d_x, d_F, d_B, d_val; /* d_val: NSLOT x ncell                    */
    iemic::DevBuf<double> d_tmp1, d_tmp2, d_red;
    /* reduction buffers (allocated at create): partial sums, results, pinned host copy */
    iemic::DevBuf<double> d_part, d_hbuf;
    double* h_red = nullptr;
    int jac_valid = 0;
    int refs = 1;                    /* the handle + dependents (atmosphere, coupled model) */
    iemic::BlockGS gs;
    iemic::Krylov kr;
    iemic::Theta th;
    iemic::Stoch st;
    int64_t ncalls[2] = {0, 0};      /* krylov_solve and prec_compute calls since creation  */
    int64_t frc_gen = 0;             /* counts compute_forcing: what Stoch::coF was made from */
    iemic::Eigs eg;
    iemic::Projected pj;
    iemic::Score sc;
    iemic::Geo geo() const;
    iemic_ctx() = default;
    iemic_ctx(const iemic_ctx&) = delete;
    iemic_ctx& operator=(const iemic_ctx&) = delete;
    ~iemic_ctx();
};

namespace iemic {
/* the host waits for the stream (e null) or an event: bounded under RCCL (comm.hip) */
int dev_wait(iemic_ctx* c, hipEvent_t e, const char* what);
#define DEV_SYNC(c)                                                     \
    do {                                                                \
        const int rs_ = ::iemic::dev_wait((c), nullptr, __func__);      \
        if (rs_) return rs_;                                            \
    } while (0)
#define DEV_WAIT_EVENT(c, e)                                            \
    do {                                                                \
        const int rs_ = ::iemic::dev_wait((c), (e), __func__);          \
        if (rs_) return rs_;                                            \
    } while (0)
/* Stream-ordered copies: every transfer goes through the context's stream and is complete
 * on return (the stream is non-blocking, so the legacy null stream must never be used). */
inline int h2d(iemic_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!bytes) return 0;
    HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    DEV_SYNC(c);
    return 0;
}
inline int d2h(iemic_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!bytes) return 0;
    HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    DEV_SYNC(c);
    return 0;
}
/* nanmax of d_part[0 .. nb), the block maxima a kernel left there, on the host */
inline int part_nanmax(iemic_ctx* c, int nb, double* mx)
{
    std::vector<double> part(nb);
    const int rc = d2h(c, part.data(), c->d_part.p, sizeof(double) * nb);
    if (rc) return rc;
    *mx = 0.0;
    for (double v : part) *mx = nanmax(*mx, v);
    return 0;
}
/* blocks of 256 threads for an element-wise kernel over N rows (grid-stride beyond 2048) */
inline unsigned grid_for(int64_t N)
{
    int64_t b = (N + 255) / 256;
    return (unsigned)std::min<int64_t>(b, 2048);
}
/* the owned slab of an ext vector, rows [o, o + n), and the grid of an element-wise launch
 * over it.  (Reductions into d_part take their own grids, capped by RED_BLOCKS.) */
struct Owned {
    int64_t o, n;
    unsigned grid;
};
inline Owned owned(const iemic_ctx* c)
{
    const int64_t n = c->sub.nlrows();
    return {NUN * c->sub.own0, n, grid_for(n)};
}
/* p[0 .. n) = 0 by a kernel of the library.  Used instead of hipMemsetAsync on the solve
 * path: the HIP runtime dispatches a memset as its own blit kernel, and rocprofv3's kernel
 * tracer (rocprofiler-sdk 7.2) faulted inside its dispatch intercept when several host
 * threads issued those concurrently (eight in-process band ranks) */
__global__ void k_zero(double* __restrict__ p, int64_t n);
inline int dev_zero(iemic_ctx* c, double* p, int64_t n);
/* two timing events, destroyed on every return path */
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    int create()
    {
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return IEMIC_EDEVICE;
        return 0;
    }
    ~EventPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};
/* Drains the stream when an entry point returns, also on error paths, so no kernel of
 * this context is still in flight when control goes back to the caller. */
inline int dev_zero(iemic_ctx* c, double* p, int64_t n)
{
    if (n <= 0) return 0;
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_zero, dim3(g), dim3(256), 0, c->stream, p, n);
    HIP_OK(hipGetLastError());
    return 0;
}
struct StreamGuard {
    iemic_ctx* c;
    ~StreamGuard() { if (c && c->stream) (void)dev_wait(c, nullptr, "return"); }
};
/* A scope whose work goes to the side stream.  The constructor forks (ev_fork on the stream,
 * the side stream waits for it; err) and makes c->stream name the side stream, which all that
 * reads c->stream follows (h2d, d2h, dev_zero, dev_wait, run_msgs, allreduce_sum,
 * StreamGuard); the destructor puts the stream back on every return path.  fork_now = false:
 * the caller forked earlier (OnSide::fork) and has put work on the stream since, which the
 * side stream is not to wait for.  join: the stream is put back, ev_join follows the side
 * stream's work and, when wait_now, the stream waits for it (else a later OnSide::wait).  A
 * record or wait that fails is returned after the host has waited for the side stream
 * instead, so none of the scope's work is left running unordered. */
struct OnSide {
    iemic_ctx* c;
    hipStream_t main;
    hipError_t err;
    static hipError_t fork(iemic_ctx* c)
    {
        const hipError_t e = hipEventRecord(c->ev_fork, c->stream);
        return e != hipSuccess ? e : hipStreamWaitEvent(c->side, c->ev_fork, 0);
    }
    static hipError_t wait(iemic_ctx* c)
    {
        const hipError_t e = hipStreamWaitEvent(c->stream, c->ev_join, 0);
        if (e != hipSuccess) (void)hipStreamSynchronize(c->side);
        return e;
    }
    explicit OnSide(iemic_ctx* c_, bool fork_now = true)
        : c(c_), main(c_->stream), err(fork_now ? fork(c_) : hipSuccess)
    {
        c->stream = c->side;
    }
    OnSide(const OnSide&) = delete;
    OnSide& operator=(const OnSide&) = delete;
    ~OnSide() { c->stream = main; }
    hipError_t join(bool wait_now)
    {
        c->stream = main;
        const hipError_t e = hipEventRecord(c->ev_join, c->side);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(c->side);
            return e;
        }
        return wait_now ? wait(c) : hipSuccess;
    }
};

/* comm.hip: sums over the ranks (no-op for one rank) and halo exchanges.  A message is
 * nblk blocks of len doubles, stride doubles apart, from base + off; one exchange is a
 * list of messages in two phases (x, then y: the y messages carry the x halo, so the
 * corner cells arrive too), each run as one batch by the transport. */
struct Seg {
    double* base;
    int64_t off, nblk, len, stride;
};
struct Msg {
    bool send;
    int peer;
    Seg s;
};
/* the exchange with a pair of opposite neighbours (lo: west / south, hi: east / north; < 0:
 * none) in the order by which the ranks' batches pair up: send lo, receive hi, send hi,
 * receive lo */
inline void push_pair(std::vector<Msg>& ops, int lo, int hi, const Seg& lo_send, const Seg& hi_recv,
                      const Seg& hi_send, const Seg& lo_recv)
{
    if (lo >= 0) ops.push_back({true, lo, lo_send});
    if (hi >= 0) ops.push_back({false, hi, hi_recv});
    if (hi >= 0) ops.push_back({true, hi, hi_send});
    if (lo >= 0) ops.push_back({false, lo, lo_recv});
}
int allreduce_sum(iemic_ctx* c, double* dev, int count);
int comm_size(const iemic_ctx* c, int* size, int* kind);
/* depth latitude rows and x columns of the ext layout (width doubles per cell) */
int halo_exchange(iemic_ctx* c, double* ext_vec, int depth);
int halo_exchange_w(iemic_ctx* c, double* ext_cells, int width, int depth);
/* the two phases of an exchange of arrays of the ext layout (appended to x / y) */
int halo_exchange_planar(iemic_ctx* c, double* v, int nplanes, int64_t ps, int depth);
void halo_plan_ext(const iemic_ctx* c, double* v, int width, int depth, std::vector<Msg>& x,
                   std::vector<Msg>& y);
int run_msgs(iemic_ctx* c, const std::vector<Msg>& ops);
int comm_init(iemic_ctx* c, const unsigned char* id, int rank, int nranks);
/* collective check at creation that every rank's exchange plans pair up (the k-th message
 * a sends to b has the size of the k-th b receives from a): a mismatch is an error naming
 * the pair, before any exchange could hang */
int comm_verify_plans(iemic_ctx* c);
/* drop one reference to the context (iemic_destroy, a dependent's destroy); the last one
 * frees it */
void ctx_release(iemic_ctx* c);
int comm_unique_id(unsigned char* id128);
void* local_group_new(int nranks);
void local_group_free(void* g);
void local_group_join(iemic_ctx* c, void* g);
void local_group_leave(iemic_ctx* c);
void comm_destroy(iemic_ctx* c);

/* assembly.hip */
int assemble_jacobian(iemic_ctx* c, const double* x_dev);
int assemble_rhs(iemic_ctx* c, const double* x_dev, double* F_dev);
/* d_B = the diagonal mass matrix of the owned cells (state independent) */
int assemble_diagB(iemic_ctx* c);
int compute_forcing(iemic_ctx* c);
/* the nine surface flux fields of the state x_dev (planar, [9][n*m], whole on every rank)
 * and the salinity correction times gamma, on the host */
int surface_fluxes(iemic_ctx* c, const double* x_dev, double* out9, double* scorr);
int intcond_correction(iemic_ctx* c, const double* x_dev);
/* spmv.hip, krylov.hip, idrs.hip */
/* y = J x on the owned rows; x (ext layout) gets its halo rows exchanged first */
int spmv(iemic_ctx* c, double* x, double* y, hipStream_t s);
int spmv_kernel(iemic_ctx* c, const double* x, double* y);
/* the block GS dynamics defect d = r - A_DD z on the active U/V/W/P rows (component-planar);
 * halo: on the bands' two halo rows too */
int spmv_dyn_defect(iemic_ctx* c, const double* z, const double* r, const uint8_t* knP, double* d, bool halo = false);
double dot(iemic_ctx* c, const double* a, const double* b, int64_t n);
int dot_owned(iemic_ctx* c, const double* a, const double* b, double* out);
int idrs(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt, iemic_solve_info* info);
/* opt->method: 0 FGMRES, 1 IDR(s) */
int krylov_solve(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt,
                 iemic_solve_info* info);
int fgmres(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt,
           iemic_solve_info* info);
/* theta.hip: the theta method on the resident state (ThetaModel.H:64-164) */
int theta_init_step(iemic_ctx* c, double dt, double theta);
/* F_theta(state) into Theta::Ft, scaled by 1 / dt / theta into Theta::b */
int theta_rhs(iemic_ctx* c);
/* J(state) with -B / dt / theta on the diagonal of the U, V, T and S rows */
int theta_jacobian(iemic_ctx* c);
/* the same with the caller's dt and theta, no initialised step needed */
int theta_jacobian_at(iemic_ctx* c, double dt, double theta);
/* state -= dx on the owned rows; *absmax: this rank's max |dx| (NaN propagates) */
int theta_update(iemic_ctx* c, const double* dx, double* absmax);
int theta_restore(iemic_ctx* c);
/* stochastic.hip: the stochastic theta model (StochasticThetaModel.H) on top of theta.hip */
/* Stoch::coF of the current forcing (d_frc and par untouched) */
int stoch_forcing(iemic_ctx* c);
/* Stoch::coF as the reference's matrix: owned entries in row order (pointers may be null) */
int stoch_export(iemic_ctx* c, int64_t* rows, int* cols, double* vals, int64_t* nnz);
/* after theta_init_step: coF again if the forcing changed, G = (sqrt(dt) sigma) (coF pert[j]),
 * noise armed (sigma = 0: nothing armed) */
int stoch_arm(iemic_ctx* c, double sigma, const double* pert);
/* Stoch::G = (sqrt(dt) sigma) (coF pert[j]) alone; disarms the full model's noise */
int stoch_noise(iemic_ctx* c, double dt, double sigma, const double* pert);
/* theta_rhs's residual launch while noise is armed: F_theta + G into Theta::Ft, scaled into Theta::b */
int stoch_theta_residual(iemic_ctx* c);
/* eigs.hip: shift-invert Arnoldi for J x = lambda B x on the resident state */
/* J(state) with -(sigma B) on the diagonal of the U, V, T and S rows (sigma = 0: J untouched) */
int shifted_jacobian(iemic_ctx* c, double sigma);
int eigs_begin(iemic_ctx* c, double sigma, int m, uint64_t seed, const iemic_krylov* opt);
int eigs_step(iemic_ctx* c, const iemic_krylov* opt, double* hcol, iemic_eigs_info* info);
int eigs_end(iemic_ctx* c);
/* xs[q] = sum_i Y[i p + q] V_i (i < j, q < p <= 16) over N rows, one pass over V (stride ldv);
 * Y: host, j x p row-major; V and xs point at the first row the launch covers */
int eigs_ritz(iemic_ctx* c, const double* V, int64_t ldv, int j, int p, const double* Y, double* const* xs,
              int64_t N);
/* V[:, q] <- sum_i Q[i p + q] V[:, i] (i < j, q < p) and V[:, p] <- V[:, j] over N rows, in place,
 * one pass (stride ldv); Q: host, j x p row-major; 1 <= p < j, p <= 16; V points at the first row */
int eigs_compress(iemic_ctx* c, double* V, int64_t ldv, int j, int p, const double* Q, int64_t N);
/* thick restart of the run in progress on Q (j x p): the basis compressed, t = B v_p, j <- p */
int eigs_restart(iemic_ctx* c, int p, const double* Q);
/* out2 = sum |a - mu B x|^2, sum |a|^2 over N rows (a, x complex; ai = xi = null: real),
 * summed over the ranks; pointers at the first row */
int eigs_residual_sums(iemic_ctx* c, const double* ar, const double* ai, const double* xr, const double* xi,
                       const double* B, double mu_r, double mu_i, int64_t N, double* out2);
/* the two norms of iemic_eigs_residual for ext vectors xr, xi (their halo rows are updated) */
int eigs_residual(iemic_ctx* c, double lam_re, double lam_im, double* xr, double* xi, double* out2);
/* spmv.hip: W(:, b) = J V(:, b), b < k <= SPMM_MAX_K, columns ldv / ldw apart (ext layout, halo rows
 * current), in blocks of kbmax columns per launch (0: SPMM_KB); column b has spmv_kernel's bits */
int spmm_kernel(iemic_ctx* c, const double* V, int64_t ldv, int k, double* W, int64_t ldw, int kbmax = 0);
/* projected.hip: the projected theta model (ProjectedThetaModel.H, StochasticProjectedThetaModel.H) */
/* G (ka x kb, row-major, host) = V^T diag(d) W over the owned rows, summed over the ranks; V, d, W
 * point at the first owned row (d null: no weights); deterministic (two stages, no atomics) */
int proj_gram(iemic_ctx* c, const double* V, int64_t ldv, int ka, const double* d, const double* W, int64_t ldw,
              int kb, double* G);
/* device buffers for a basis of k columns (Projected::V, W, part, res), the small vectors sized */
int proj_alloc(iemic_ctx* c, int k);
int proj_set_basis(iemic_ctx* c, const double* V, int k);
int proj_clear(iemic_ctx* c);
int proj_restrict_state(iemic_ctx* c, double* y);
int proj_set_state(iemic_ctx* c, const double* y);
int proj_init_step(iemic_ctx* c, double dt, double theta);
int proj_arm(iemic_ctx* c, double sigma, const double* pert);
int proj_rhs(iemic_ctx* c, double* r);
int proj_solve(iemic_ctx* c, const double* r, double* dy);
int proj_newton_step(iemic_ctx* c, iemic_proj_info* info);
int proj_restore(iemic_ctx* c);
/* score.hip: the score function's two distances in one pass */
/* out2 = sum (x - a)^2, sum (x - b)^2 over the owned rows of variable var (-1: all of them), summed
 * over the ranks; x, a, b ext vectors; deterministic (two stages, no atomics) */
int score_sqdist2(iemic_ctx* c, int var, const double* x, const double* a, const double* b, double* out2);
int score_set(iemic_ctx* c, const double* sol1, const double* sol2, const double* sol3, int var);
int score_eval(iemic_ctx* c, const double* v, double* dist, double* d1, double* d2);
int score_clear(iemic_ctx* c);
/* out (k x k, row-major, host) = V^T diag(e_var) V of the projected model's basis (var -1: V^T V) */
int proj_gram_vv(iemic_ctx* c, int var, double* out);
/* prec.hip */
int prec_compute(iemic_ctx* c, const iemic_krylov* opt);
int prec_apply(iemic_ctx* c, const double* r, double* z);
/* the solvers' stagnation safeguard: the block GS's correction passes take minimal-residual steps
 * from now on; 0: nothing to switch */
int prec_safeguard(iemic_ctx* c);
/* the block GS: set-up (gs_setup.hip) and apply (prec_gs.hip) */
int gs_compute(iemic_ctx* c, const iemic_krylov* opt);
int gs_apply(iemic_ctx* c, const double* r, double* z);
/* the block GS apply from a compressed input (6 rows per ActiveSet::act cell, zero land rows) */
/* staged: rc is already in the block GS's planar right-hand side (k_dcgs_update) */
int gs_apply_c(iemic_ctx* c, const double* rc, double* z, bool staged = false);
/* prec_gs.hip: GPU microseconds of the block GS apply's four parts (one rank) */
int gs_time_parts(iemic_ctx* c, int nrep, double* us);
/* y = J x written compressed (rows of the active cells only; x full, halo current) */
int spmv_kernel_c(iemic_ctx* c, const double* x, double* yc, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
}  // namespace iemic

#endif
