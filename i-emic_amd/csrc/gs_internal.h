/*
 * gs_internal.h -- what the units of the block Gauss-Seidel preconditioner share
 * (prec_gs.hip, gs_setup.hip, gs_dyn.hip, ts_sweeps.hip, ts_mg.hip, ts_mg_setup.hip, active_set.hip):
 * the Jacobian's slot indices, the subdomain layout seen by their kernels, the launch helpers
 * and the entries they call in each other.  Included by nothing else.
 */
#ifndef IEMIC_GS_INTERNAL_H
#define IEMIC_GS_INTERNAL_H

#include <type_traits>

#include "common.h"

namespace iemic {

namespace {

/* slot indices (see SLOTS in stencil.h) */
constexpr int S_UU0 = 0, S_UV0 = 7;                 /* U row: U self, V self            */
constexpr int S_UP = 20;                            /* U row: P (0,0),(1,0),(0,1),(1,1) */
constexpr int S_VV0 = 24, S_VU0 = 31;               /* V row: V self, U self            */
constexpr int S_VP = 42;                            /* V row: P, same order             */
constexpr int S_WP0 = 47, S_WP1 = 48;               /* W row: P(k), P(k+1)              */
constexpr int S_PU = 54, S_PV = 58;                 /* P row: U/V (0,0),(-1,0),(0,-1),(-1,-1) */
constexpr int S_PW0 = 62, S_PWM = 63;               /* P row: W(k), W(k-1)              */
constexpr int S_TT0 = 64, S_TS0 = 81;               /* T row: T self, S self            */
constexpr int S_SS0 = 84, S_ST0 = 101;              /* S row: S self, T self            */
constexpr int GSL = 10;                             /* gslot doubles per cell           */
constexpr int RC_NE = 18;                           /* rcol coefficients per level (gs_dyn.hip) */
constexpr int MR_NB = 256;                          /* blocks of the minimal-residual dots */
constexpr int TS_NC = 16;                           /* compact T/S couplings per cell (tsoff) */

/* subdomain layout seen by the kernels (stencil.h ext layout, Decomp2D): n, m global;
 * owned columns [ib0, ib0 + nx), rows from jb0; per-cell arrays are indexed by ext cell,
 * the Jacobian by owned cell (ext cell - own0: the owned cells are one slab) */
struct Lay {
    int n, m, l, periodic, jb0, ib0, nx, hx;
    int64_t nloc, own0, xb;
    int64_t ps;                      /* plane stride of the planar dynamics vectors (next) */
};
/* unknown v of ext cell e in a component-planar vector */
#define PL(e, v) ((e) + (int64_t)(v) * L.ps)
/* ext cell of global (i, j, k) (i in the grid after hnb's wrap; the x halo when split) */
__device__ __forceinline__ int64_t ecell(const Lay& L, int i, int j, int k)
{
    const int64_t r = ((int64_t)j - L.jb0 + HALO) * L.l + k;
    return xcell(r, xlocal(i, L.n, L.ib0, L.nx, L.hx, L.hx ? L.periodic : 0), L.nx, L.hx, L.xb);
}
__device__ __forceinline__ void lc_ijk(const Lay& L, int64_t lc, int& i, int& j, int& k)
{
    i = L.ib0 + (int)(lc % L.nx);
    k = (int)((lc / L.nx) % L.l);
    j = L.jb0 + (int)(lc / ((int64_t)L.nx * L.l));
}
__device__ __forceinline__ SubLay sub_of(const Lay& L)
{
    SubLay X;
    X.n = L.n; X.m = L.m; X.l = L.l; X.periodic = L.periodic;
    X.jb0 = L.jb0; X.ib0 = L.ib0; X.nx = L.nx; X.hx = L.hx; X.xb = L.xb;
    return X;
}
#define LAY_ALIASES const int n = L.n, m = L.m, l = L.l, periodic = L.periodic; (void)n; (void)m; (void)l; (void)periodic
/* thread -> owned cell: lc (Jacobian column), cell (ext), (i, j, k) */
#define OWNED_CELL                                                                       \
    const int64_t lc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;                   \
    if (lc >= L.nloc) return;                                                            \
    const int64_t cell = L.own0 + lc;                                                    \
    const int64_t ncell = L.nloc;                                                        \
    int i, j, k;                                                                         \
    lc_ijk(L, lc, i, j, k);                                                              \
    (void)i; (void)j; (void)k; (void)ncell
/* wrap / reject a horizontal neighbour; returns false when outside the domain */
__host__ __device__ __forceinline__ bool hnb(int& i, int& j, int n, int m, int periodic)
{
    if (j < 0 || j >= m) return false;
    if (i < 0 || i >= n) {
        if (!periodic) return false;
        i = (i + n) % n;
    }
    return true;
}

/* one T or S row of rr_TS - A_TS,D z_D (k_gs_bts2, k_mg_entry): the row's 10 dynamics slots
 * unrolled at compile time, neighbour indices clamped as in the SpMV (the ELL holds zeros
 * outside the domain), identity-row columns (their couplings are in rr already) skipped by
 * the slot bitmask kmask instead of a byte gather per slot */
template <int R>
__device__ __forceinline__ double bts_row(const double* __restrict__ val, const double* __restrict__ z,
                                          int64_t lc, int64_t nloc, const int (*nc)[9],
                                          uint64_t kbits, double acc, int64_t zcell = NUN, int64_t zvar = 1)
{
    /* z(cell, var) = z[zcell cell + zvar var]: (NUN, 1) AoS, (1, plane stride) planar */
    constexpr int B = RowInfo<R>::B, NS = RowInfo<R>::NS;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const Slot sl = SLOTS[B + s];
        if (sl.var == TT || sl.var == SS) continue;
        /* identity-row columns (coupling already in rr) weigh 0: no branch, so the loads of
         * all the row's slots issue together (default load policy: non-temporal loads made
         * the T/S solve 6.5 us slower, scripts/ab_probe.py) */
        const double v = ((kbits >> (B + s - 64)) & 1) ? 0.0 : val[(int64_t)(B + s) * nloc + lc];
        const int cidx = nc[sl.di + 1][(sl.dk + 1) * 3 + (sl.dj + 1)];
        acc -= v * z[zcell * (int64_t)cidx + zvar * sl.var];
    }
    return acc;
}

}  // namespace

/* the record plus the plane stride of the planar dynamics vectors (next) */
static Lay lay_of(const Sub& S)
{
    Lay L;
    L.n = S.n; L.m = S.m; L.l = S.l; L.periodic = S.periodic; L.jb0 = S.jb0;
    L.ib0 = S.ib0; L.nx = S.nx; L.hx = S.hx; L.xb = S.xb;
    L.nloc = S.nloc; L.own0 = S.own0; L.ps = S.next;
    return L;
}
static unsigned blocks_for(int64_t n) { return (unsigned)((n + 255) / 256); }

/* lanes per z-line (one per level, a power of two >= l; the smoother needs l <= 64) */
static int mg_lanes(int l) { return l <= 16 ? 16 : (l <= 32 ? 32 : 64); }
/* f(std::integral_constant<int, P>) for the lane count P of mg_lanes: the one place where
 * the kernels' compile-time lane count is chosen */
template <typename F>
static inline void with_lanes(int P, F&& f)
{
    switch (P) {
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
    }
}
#define LANES_OF(p) (decltype(p)::value)

/* the entries the units call in each other: not among the library's dynamic symbols */
#pragma GCC visibility push(hidden)
/* gs_dyn.hip: one dynamics pass, z(U/V/W/P) from rr (both component-planar) */
int dyn_solve(iemic_ctx* c, const double* rr, double* z, double* zo = nullptr, double omega = 0.0,
              double* zaos = nullptr, bool rr_halo = false, bool schur = true);
/* does pass it of BlockGS::dyn_iters solve the Schur system (BlockGS::schur_passes)? */
bool gs_pass_schur(const BlockGS& gs, int it);
/* the minimal-residual step from BlockGS::dres and dq: zP += w zc, (upd) dres += w dq */
int dyn_mr_step(iemic_ctx* c, bool upd, double* zaos);
/* ts_sweeps.hip: its buffers, its colour pack (set-up), and the T/S solve by plain sweeps */
int ts_sweeps_reserve(iemic_ctx* c);
void ts_sweeps_pack(iemic_ctx* c);
int ts_sweeps_solve(iemic_ctx* c, double* z);
#pragma GCC visibility pop

}  // namespace iemic

#endif
