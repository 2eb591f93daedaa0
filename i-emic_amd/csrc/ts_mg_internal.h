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

/* The entry kernel's tile (k_mg_entry, k_mg_entry_p): MG_TI columns of one latitude row over
 * the full depth, cell q = k MG_TI + ii of the tile.  Its packed operand A_TS,D (TsMg::ep,
 * k_mg_entry_pack): the T and S rows' slots whose columns are dynamics unknowns, listed here
 * once from the slot table in the rows' own order (the order bts_row accumulates in). */
constexpr int MG_TI = 16;
struct EntrySlots {
    int n[2];                        /* dynamics slots of the T row, of the S row            */
    int s[2][20];                    /* their indices in SLOTS                               */
};
constexpr EntrySlots entry_slots()
{
    EntrySlots E{};
    for (int R = 0; R < 2; R++)
        for (int s = ROW_BEGIN[TT + R]; s < ROW_BEGIN[TT + R + 1]; s++)
            if (SLOTS[s].var != TT && SLOTS[s].var != SS) E.s[R][E.n[R]++] = s;
    return E;
}
constexpr EntrySlots MG_ES = entry_slots();
constexpr int MG_NE = MG_ES.n[0];    /* terms per row (10)                                   */
/* the two rows read the same columns in the same order, so one gather of z serves both */
constexpr bool entry_slots_match()
{
    if (MG_ES.n[0] != MG_ES.n[1]) return false;
    for (int d = 0; d < MG_ES.n[0]; d++) {
        const Slot a = SLOTS[MG_ES.s[0][d]], b = SLOTS[MG_ES.s[1][d]];
        if (a.di != b.di || a.dj != b.dj || a.dk != b.dk || a.var != b.var) return false;
    }
    return true;
}
static_assert(entry_slots_match(), "the T and S rows' dynamics slots differ");
/* a tile's descriptor in TsMg::etl, 2 + nw 64-bit words: the first double of its run in ep,
 * its active cells na, the active-cell mask (bit q & 63 of word q >> 6).  The run holds term
 * d of row R (0 T, 1 S) of the r-th active cell at (R MG_NE + d) na + r, and starts on a
 * 128-byte line that no other tile shares. */
__host__ __device__ __forceinline__ int mg_entry_words(int l) { return (MG_TI * l + 63) / 64; }
__device__ __forceinline__ int mg_entry_rank(const uint64_t* __restrict__ e, int q)
{
    const int w = q >> 6, bit = q & 63;
    int r = __popcll(e[2 + w] & (((uint64_t)1 << bit) - 1));
    for (int u = 0; u < w; u++) r += __popcll(e[2 + u]);
    return r;
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
