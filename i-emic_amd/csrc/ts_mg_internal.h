/*
 * ts_mg_internal.h -- what the two units of the T/S multigrid share (ts_mg.hip: the apply,
 * ts_mg_setup.hip: the set-up): a level as the kernels see it, its cell index, and the walk
 * over one row of the coarsest level's operator.  Included by nothing else.
 */
#ifndef IEMIC_TS_MG_INTERNAL_H
#define IEMIC_TS_MG_INTERNAL_H

#include "gs_internal.h"

namespace iemic {

namespace {

struct TsLev {
    int n, mb, l, periodic;          /* periodic: the level wraps in x (one x part)        */
    int hj, hi;                      /* halo rows / columns of the layout (level 0, split)  */
    int vis, visi;                   /* halo rows / columns the smoother / residual read    */
    int jpar;                        /* colour parity of (0, 0) (global i + j, level 0)     */
    int64_t cstr;                    /* array stride (mb + 2 hj) (n + 2 hi) l              */
    const double* off;               /* 16 x cstr: T row q 0..7, S row q 8..15            */
    const double* diag;              /* 4 x cstr: 2x2 block (TT, TS, ST, SS)              */
    const double* fac;               /* 12 x cstr: line factors F | A'^-1 | Cp            */
    double* b;                       /* 2 x cstr: right-hand side (T, S)                  */
    double* z;                       /* 2 x cstr: iterate (T, S)                          */
};
__host__ __device__ __forceinline__ int64_t mg_cell(const TsLev& V, int i, int jl, int k)
{
    return (((int64_t)jl + V.hj) * (V.n + 2 * V.hi) + i + V.hi) * V.l + k;
}

/* decode of a halo-free level's cell index t = (jl n + i) l + k */
__host__ __device__ __forceinline__ void mg_decode(int64_t t, int n, int l, int& i, int& jl, int& k)
{
    k = (int)(t % l);
    i = (int)((t / l) % n);
    jl = (int)(t / ((int64_t)l * n));
}

/* Row (cell (i, jl, k), variable R: 0 T, 1 S) of the coarsest level's operator on its cn x cm
 * x l grid, entry by entry in the one order every assembly of it accumulates in: the 2x2
 * block's own entry dself, its cross entry dcross, then the 8 couplings off8[qq ostr] (0 .. 5:
 * the same variable at -i, +i, -j, +j, -k, +k; 6, 7: the other variable at -k, +k), zeros and
 * neighbours outside the grid skipped, x wrapping when wrap.  f(ii, jj, kk, var, dir, v) gets
 * the column's cell and variable, the direction (-1: the cell itself) and the value; where
 * the entry lands is the caller's business. */
template <class F>
__host__ __device__ __forceinline__ void mg_coarse_row(int R, int i, int jl, int k, int cn, int cm, int l, bool wrap,
                                                       double dself, double dcross, const double* off8,
                                                       int64_t ostr, F&& f)
{
    f(i, jl, k, R, -1, dself);
    f(i, jl, k, 1 - R, -1, dcross);
    for (int qq = 0; qq < 8; qq++) {
        const double v = off8[qq * ostr];
        if (v == 0.0) continue;
        const int dir = qq < 6 ? qq : qq - 2;
        int ii = i, jj = jl, kk = k;
        switch (dir) {
        case 0: ii--; break;
        case 1: ii++; break;
        case 2: jj--; break;
        case 3: jj++; break;
        case 4: kk--; break;
        default: kk++; break;
        }
        if (jj < 0 || jj >= cm || kk < 0 || kk >= l) continue;
        if (ii < 0 || ii >= cn) {
            if (!wrap) continue;
            ii = (ii + cn) % cn;
        }
        f(ii, jj, kk, qq < 6 ? R : 1 - R, dir, v);
    }
}

}  // namespace

/* intermediate levels (1 ..) that carry the x halo under x splits */
constexpr int MG_XHALO_LEVELS = 99;
static TsLev mg_view(iemic_ctx* c, int q)
{
    BlockGS& gs = c->gs;
    TsLev V{};
    V.l = c->l;
    V.n = gs.mg.n[q];
    V.mb = gs.mg.m[q];
    /* subdomains: the level-0 smoother and residual see the neighbours' edge rows and
     * columns (halo rows / columns in the layout, exchanged before every relaxation); with
     * an x split the intermediate levels see the neighbours' edge columns too (a cut across
     * the zonal flow would otherwise make them block Jacobi), the coarsest is
     * the global problem; colours by the global i + j parity of the level's aggregates, so
     * that all subdomains relax the same colour in the same launch and a cell's neighbours
     * across a cut have the other colour; the x wrap only with one x part */
    const int qc = gs.mg.nlev - 1;
    V.periodic = c->cfg.periodic && c->sub.npx == 1;
    V.hj = (q == 0 && c->sub.npy > 1) ? (gs.mg.hr ? 2 : 1) : 0;
    V.hi = (q < qc && q <= MG_XHALO_LEVELS && c->sub.npx > 1) ? 1 : 0;
    V.vis = V.hj;
    V.visi = V.hi;
    V.jpar = gs.mg.par[q];
    V.cstr = (int64_t)(V.mb + 2 * V.hj) * (V.n + 2 * V.hi) * V.l;
    V.off = gs.mg.off[q].p;
    V.diag = gs.mg.diag[q].p;
    V.fac = gs.mg.fac[q].p;
    V.b = gs.mg.b[q].p;
    V.z = gs.mg.z[q].p;
    return V;
}

}  // namespace iemic

#endif
