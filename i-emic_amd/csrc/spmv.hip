/*
 * spmv.hip -- the stencil-ELL SpMV of the ocean Jacobian.
 *
 *  - k_spmv7 replaces Epetra_CrsMatrix::Apply (Ocean::applyMatrix, src/ocean/Ocean.C:1352-1357)
 *    on the maximal graph: one workgroup per 64-cell tile of a grid row stages the x values
 *    of the tile's neighbourhood in LDS and four waves share the 104 slot-major coefficient
 *    rows (read non-temporally); columns are implicit in the cell index and slot.  The dense
 *    integral-condition row (SRES = 0, THCM.C:2121-2198) is a separate fused dot
 *    (vec_kernels.h's multi-dot pair).
 *  - k_spmv7c: the same on the active cells only, written compressed (FGMRES's basis).
 *  - k_spmv_dyn: the U/V/W/P rows only (the dynamics defect of the block GS).
 */
#include <algorithm>
#include <cstdlib>

#include <hip/hip_ext.h>

#include "common.h"
#include "vec_kernels.h"

namespace iemic {

/* ---- k_spmv7: LDS-staged x, slot-balanced waves ----------------------------------------
 * One workgroup (4 waves) per tile of up to 64 cells along i of one (j, k) grid row.  The
 * x values of the tile's neighbourhood -- the six (dj, dk) grid rows the slot table reaches
 * ((0,0), (+-1,0), (0,+-1), (+1,-1)), cells i0-1 .. i0+64, all six unknowns -- are copied
 * into LDS with contiguous loads, so the 104 gathers per cell become LDS reads.  The 104
 * slots are split into four runs of 26 (one per wave: U+V, V+W, W+P+T, T+S) instead of one
 * wave per equation (24/22/7/11/20/20), so the waves of a tile finish together; their row
 * partials meet in LDS and the 384 results of the tile are stored contiguously. */
constexpr int SP7_T = 64;
__host__ __device__ constexpr int sp7_row(int s)
{
    return s < 24 ? 0 : s < 46 ? 1 : s < 53 ? 2 : s < 64 ? 3 : s < 84 ? 4 : 5;
}
__host__ __device__ constexpr int sp7_combo(int dj, int dk)
{
    return dk == 0 ? (dj + 1) : (dk == -1 ? (dj == 0 ? 3 : 5) : 4);  /* (-1,0)0 (0,0)1 (1,0)2 (0,-1)3 (0,1)4 (1,-1)5 */
}
/* the coefficient stream is read once per SpMV: non-temporal loads (in-solve 43.4 us vs
 * 45.9 us with the default policy at 2 degrees) */
template <int S0, int S1>
__device__ __forceinline__ void sp7_load(const double* __restrict__ val, int64_t nloc, int64_t lc, bool act,
                                         double* v)
{
    /* an inactive lane's v is left undefined (its sums are never stored): no merge point
     * that would wait for the loads before the staging's are issued */
    if (act) {
#pragma unroll
        for (int s = S0; s < S1; s++) v[s - S0] = __builtin_nontemporal_load(val + (int64_t)s * nloc + lc);
    }
}
template <int S0, int S1>
__device__ __forceinline__ void sp7_compute(const double* v, const double* xs, int c, double* acc)
{
#pragma unroll
    for (int s = S0; s < S1; s++) {
        const Slot sl = SLOTS[s];
        const int q = sp7_combo(sl.dj, sl.dk);
        acc[sp7_row(s) - sp7_row(S0)] += v[s - S0] * xs[(q * (SP7_T + 2) + (c + 1 + sl.di)) * NUN + sl.var];
    }
}
/* the full SpMV (FGMRES's compressed basis uses k_spmv7c below) */
__global__ void __launch_bounds__(256) k_spmv7(SubLay X, const double* __restrict__ val,
                                               const double* __restrict__ x,
                                               double* __restrict__ y, int nloc, int ntile, int tpr)
{
    __shared__ double xs[6 * (SP7_T + 2) * NUN];
    __shared__ double red[4][3][SP7_T];
    const int l = X.l, nx = X.nx;
    const int per = (ntile + 7) >> 3;
    const int tile = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (tile >= ntile) return;
    const int row = tile / tpr, i0 = (tile - row * tpr) * SP7_T;
    const int k = row % l, jl = row / l, j = X.jb0 + jl;
    const int nc = min(SP7_T, nx - i0);
    const int lc0 = row * nx + i0;
    const int t = threadIdx.x, c = t & 63;
    const int g = __builtin_amdgcn_readfirstlane(t >> 6);   /* wave-uniform: scalar branches */
    const bool act = c < nc;
    const int64_t lc = lc0 + c;
    double acc[3] = {0.0, 0.0, 0.0};
    double v[26];
    /* the coefficient loads first (one predicated block), then the x staging's loads, all
     * issued before the first LDS store: one memory latency per tile instead of one per
     * staging round (the staging loop waited for each load before its store) */
    if (g == 0) sp7_load<0, 26>(val, nloc, lc, act, v);
    else if (g == 1) sp7_load<26, 52>(val, nloc, lc, act, v);
    else if (g == 2) sp7_load<52, 78>(val, nloc, lc, act, v);
    else sp7_load<78, 104>(val, nloc, lc, act, v);
    /* stage x: 6 grid rows x (nc + 2) cells x 6 unknowns, contiguous runs (the two end
     * cells: the neighbour columns, from the x halo when the x direction is split) */
    {
        const int jm = j > 0 ? j - 1 : j, jp = j < X.m - 1 ? j + 1 : j;
        const int km = k > 0 ? k - 1 : k, kp = k < l - 1 ? k + 1 : k;
        const int rj[6] = {jm, j, jp, j, j, jp}, rk[6] = {k, k, k, km, kp, km};
        /* element e of the LDS image is (q (SP7_T + 2) + p) NUN + var: constant divisors */
        constexpr int PR = (SP7_T + 2) * NUN;
        constexpr int SPT = (6 * PR + 255) / 256;
        const int lim = (nc + 2) * NUN;
        double xv[SPT];
        int xo[SPT];
#pragma unroll
        for (int u = 0; u < SPT; u++) {
            const int e = t + 256 * u;
            const int q = e / PR, w = e - q * PR;
            xo[u] = -1;
            if (e < 6 * PR && w < lim) {
                const int p = w / NUN, var = w - p * NUN;
                const int64_t r = (int64_t)(rj[q] - X.jb0 + HALO) * l + rk[q];
                const int64_t cell = (p == 0 || p == nc + 1)
                                         ? xnb_cell(r, i0 + p - 1, X.n, X.ib0, nx, X.hx, X.periodic, X.xb)
                                         : r * nx + i0 + p - 1;
                xo[u] = e;
                xv[u] = x[NUN * cell + var];
            }
        }
#pragma unroll
        for (int u = 0; u < SPT; u++)
            if (xo[u] >= 0) xs[xo[u]] = xv[u];
    }
    __syncthreads();
    if (g == 0) sp7_compute<0, 26>(v, xs, c, acc);
    else if (g == 1) sp7_compute<26, 52>(v, xs, c, acc);
    else if (g == 2) sp7_compute<52, 78>(v, xs, c, acc);
    else sp7_compute<78, 104>(v, xs, c, acc);
#pragma unroll
    for (int q = 0; q < 3; q++) red[g][q][c] = acc[q];
    __syncthreads();
    /* rows of the groups: g0 {U,V} g1 {V,W} g2 {W,P,T} g3 {T,S}; first row of group g */
    for (int o = t; o < nc * NUN; o += 256) {
        const int cc = o / NUN, R = o - cc * NUN;
        double v;
        switch (R) {
        case 0: v = red[0][0][cc]; break;
        case 1: v = red[0][1][cc] + red[1][0][cc]; break;
        case 2: v = red[1][1][cc] + red[2][0][cc]; break;
        case 3: v = red[2][1][cc]; break;
        case 4: v = red[2][2][cc] + red[3][0][cc]; break;
        default: v = red[3][1][cc]; break;
        }
        y[NUN * ((int64_t)HALO * l * nx + lc0) + o] = v;
    }
}

/* k_spmm7<KB>: W(:, b) = J V(:, b) for KB columns per launch (the projected theta model's J2 V,
 * projected.hip), on the uncompressed slot-major Jacobian.  k_spmv7's tiling: a lane loads its 26
 * coefficients once and uses them against KB staged neighbourhoods, so the coefficient stream is
 * read once per KB columns instead of once per column (104 * 8 / KB + 96 bytes per cell and
 * column).  Column b is at x + b ldx / y + b ldy, ext layout, halo current.
 * LDS: KB images of 6 * 66 * 6 doubles (19,008 B each); the waves' row partials go into the
 * start of each column's image once every wave has read it, so KB = 4 takes 76,032 B and two
 * workgroups stay resident on a CU's 160 KiB.
 * Every column is formed by sp7_compute from the same v and the same image layout and combined
 * by the same sums as in k_spmv7: column b of W has the bits of k_spmv7 on column b. */
template <int KB>
__global__ void __launch_bounds__(256) k_spmm7(SubLay X, const double* __restrict__ val,
                                               const double* __restrict__ x, int64_t ldx,
                                               double* __restrict__ y, int64_t ldy, int nloc, int ntile, int tpr)
{
    constexpr int PR = (SP7_T + 2) * NUN, IMG = 6 * PR;
    constexpr int SPT = (IMG + 255) / 256;
    static_assert(4 * 3 * SP7_T <= IMG, "the row partials of a column fit in its image");
    __shared__ double xs[KB * IMG];
    const int l = X.l, nx = X.nx;
    const int per = (ntile + 7) >> 3;
    const int tile = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (tile >= ntile) return;
    const int row = tile / tpr, i0 = (tile - row * tpr) * SP7_T;
    const int k = row % l, jl = row / l, j = X.jb0 + jl;
    const int nc = min(SP7_T, nx - i0);
    const int lc0 = row * nx + i0;
    const int t = threadIdx.x, c = t & 63;
    const int g = __builtin_amdgcn_readfirstlane(t >> 6);   /* wave-uniform: scalar branches */
    const bool act = c < nc;
    const int64_t lc = lc0 + c;
    double acc[KB][3];
#pragma unroll
    for (int b = 0; b < KB; b++) acc[b][0] = acc[b][1] = acc[b][2] = 0.0;
    double v[26];
    if (g == 0) sp7_load<0, 26>(val, nloc, lc, act, v);
    else if (g == 1) sp7_load<26, 52>(val, nloc, lc, act, v);
    else if (g == 2) sp7_load<52, 78>(val, nloc, lc, act, v);
    else sp7_load<78, 104>(val, nloc, lc, act, v);
    /* stage the KB neighbourhoods: k_spmv7's image, the source offsets computed once */
    {
        const int jm = j > 0 ? j - 1 : j, jp = j < X.m - 1 ? j + 1 : j;
        const int km = k > 0 ? k - 1 : k, kp = k < l - 1 ? k + 1 : k;
        const int rj[6] = {jm, j, jp, j, j, jp}, rk[6] = {k, k, k, km, kp, km};
        const int lim = (nc + 2) * NUN;
        int64_t src[SPT];
        int xo[SPT];
#pragma unroll
        for (int u = 0; u < SPT; u++) {
            const int e = t + 256 * u;
            const int q = e / PR, w = e - q * PR;
            xo[u] = -1;
            src[u] = 0;
            if (e < IMG && w < lim) {
                const int p = w / NUN, var = w - p * NUN;
                const int64_t r = (int64_t)(rj[q] - X.jb0 + HALO) * l + rk[q];
                const int64_t cell = (p == 0 || p == nc + 1)
                                         ? xnb_cell(r, i0 + p - 1, X.n, X.ib0, nx, X.hx, X.periodic, X.xb)
                                         : r * nx + i0 + p - 1;
                xo[u] = e;
                src[u] = NUN * cell + var;
            }
        }
        double xv[KB][SPT];
#pragma unroll
        for (int b = 0; b < KB; b++)
#pragma unroll
            for (int u = 0; u < SPT; u++)
                if (xo[u] >= 0) xv[b][u] = x[(int64_t)b * ldx + src[u]];
#pragma unroll
        for (int b = 0; b < KB; b++)
#pragma unroll
            for (int u = 0; u < SPT; u++)
                if (xo[u] >= 0) xs[b * IMG + xo[u]] = xv[b][u];
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < KB; b++) {
        if (g == 0) sp7_compute<0, 26>(v, xs + b * IMG, c, acc[b]);
        else if (g == 1) sp7_compute<26, 52>(v, xs + b * IMG, c, acc[b]);
        else if (g == 2) sp7_compute<52, 78>(v, xs + b * IMG, c, acc[b]);
        else sp7_compute<78, 104>(v, xs + b * IMG, c, acc[b]);
    }
    __syncthreads();                    /* every image is read: its start now holds red[4][3][64] */
#pragma unroll
    for (int b = 0; b < KB; b++)
#pragma unroll
        for (int q = 0; q < 3; q++) xs[b * IMG + (g * 3 + q) * SP7_T + c] = acc[b][q];
    __syncthreads();
    /* rows of the groups as in k_spmv7: g0 {U,V} g1 {V,W} g2 {W,P,T} g3 {T,S} */
#pragma unroll
    for (int b = 0; b < KB; b++) {
        const double* red = xs + b * IMG;
        for (int o = t; o < nc * NUN; o += 256) {
            const int cc = o / NUN, R = o - cc * NUN;
            double vv;
            switch (R) {
            case 0: vv = red[(0 * 3 + 0) * SP7_T + cc]; break;
            case 1: vv = red[(0 * 3 + 1) * SP7_T + cc] + red[(1 * 3 + 0) * SP7_T + cc]; break;
            case 2: vv = red[(1 * 3 + 1) * SP7_T + cc] + red[(2 * 3 + 0) * SP7_T + cc]; break;
            case 3: vv = red[(2 * 3 + 1) * SP7_T + cc]; break;
            case 4: vv = red[(2 * 3 + 2) * SP7_T + cc] + red[(3 * 3 + 0) * SP7_T + cc]; break;
            default: vv = red[(3 * 3 + 1) * SP7_T + cc]; break;
            }
            y[(int64_t)b * ldy + NUN * ((int64_t)HALO * l * nx + lc0) + o] = vv;
        }
    }
}

/* k_spmv7c: the in-solve SpMV of FGMRES's compressed basis (round 6).  k_spmv7 reads the
 * slot-major Jacobian, whose 128-byte coefficient lines hold 16 cells: the lines of mixed land /
 * water runs are fetched whole (at 2 degrees 128.9 MB of coefficient lines for 100.7 MB of
 * active coefficients; round 5's land-skipping variant moved 147 MB per launch, 1.25x).
 *  - Coefficients: ActiveSet::spc holds the active cells' 104 slots blocked per tile -- the na
 *    active cells of a tile (consecutive in the compressed order, from a0) as one contiguous
 *    run of 104 na doubles, slot s of the tile's r-th active cell at 104 a0 + s na + r -- so a
 *    workgroup streams one run that no land cell and no other tile shares (PMC: 117.1 MB per
 *    launch against 117.7 MB algorithmic; slot-major packing over the active list: 124.9 MB,
 *    3.4 us slower).
 *  - Tiles: only the 64-cell tiles (one grid row) that hold an active cell are launched
 *    (ActiveSet::atl: tile, first / last active lane, a0, na and the 64-bit active-lane mask, so
 *    a lane finds its compressed index by a popcount instead of a dependent load), dealt to
 *    the 8 XCDs in contiguous runs.
 *  - x: the six (dj, dk) neighbour rows' interior cells are contiguous runs in x and in the
 *    LDS image, copied by LDS-DMA (global_load_lds_dwordx4, no VGPR destination: 94 instead
 *    of 104 VGPRs, 5 waves per SIMD instead of 4; 32.5 -> 29.2 us), pieces beyond the active
 *    cells' reach skipped; the two end cells of each row by plain loads.
 * Same sums in the same order as k_spmv7: the compressed rows are bitwise its rows. */
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) void glb_void;
__global__ void __launch_bounds__(256) k_spmv7c(SubLay X, const double* __restrict__ spc,
                                                const double* __restrict__ x, double* __restrict__ y,
                                                const int4* __restrict__ atl, int natile, int tpr)
{
    __shared__ double xs[6 * (SP7_T + 2) * NUN];
    __shared__ double red[4][3][SP7_T];
    __shared__ int lof[SP7_T];
    const int l = X.l, nx = X.nx;
    const int per = (natile + 7) >> 3;
    const int pos = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (pos >= natile) return;
    const int4 td = atl[2 * pos], tm = atl[2 * pos + 1];
    const int tile = td.x, clo = td.y & 255, chi = td.y >> 8, a0 = td.z;
    /* the tile's active lanes: a 64-bit mask, so a lane finds its compressed index without a
     * dependent load (cm = a0 + active lanes below it) */
    const uint64_t amask = (uint64_t)(uint32_t)tm.x | ((uint64_t)(uint32_t)tm.y << 32);
    const int row = tile / tpr, i0 = (tile - row * tpr) * SP7_T;
    const int k = row % l, jl = row / l, j = X.jb0 + jl;
    const int nc = min(SP7_T, nx - i0);
    const int t = threadIdx.x, c = t & 63;
    const int g = __builtin_amdgcn_readfirstlane(t >> 6);   /* wave-uniform: scalar branches */
    const bool act = (amask >> c) & 1;
    const int cm = act ? a0 + __builtin_popcountll(amask & ((1ull << c) - 1)) : -1;
    if (g == 0 && act) lof[cm - a0] = c;                    /* active cell -> its lane */
    double acc[3] = {0.0, 0.0, 0.0};
    double v[26];
    /* coefficient loads, then the staging loads, all issued before the first LDS store */
    const double* vb = spc + (int64_t)NSLOT * a0;
    const int64_t vs = td.w, vo = cm - a0;
    if (g == 0) sp7_load<0, 26>(vb, vs, vo, act, v);
    else if (g == 1) sp7_load<26, 52>(vb, vs, vo, act, v);
    else if (g == 2) sp7_load<52, 78>(vb, vs, vo, act, v);
    else sp7_load<78, 104>(vb, vs, vo, act, v);
    {
        /* the interior cells i0 .. i0 + nc - 1 of each of the six grid rows are one contiguous
         * run of nc * 48 bytes in x and in the LDS image: copied by LDS-DMA in 1 KiB pieces (a
         * wave-instruction of 16 bytes per lane, no VGPR destination), the pieces outside the
         * active cells' reach skipped; the two end cells of each row (the neighbour columns,
         * from the x halo when the x direction is split) by 72 plain loads */
        const int jm = j > 0 ? j - 1 : j, jp = j < X.m - 1 ? j + 1 : j;
        const int km = k > 0 ? k - 1 : k, kp = k < l - 1 ? k + 1 : k;
        const int rj[6] = {jm, j, jp, j, j, jp}, rk[6] = {k, k, k, km, kp, km};
        const int lane = t & 63, nb = nc * NUN * 8;
        const int blo = max(0, (clo - 1) * NUN * 8), bhi = min(nb, (chi + 2) * NUN * 8);
        for (int u = g; u < 18; u += 4) {
            const int q = u / 3, h = u - 3 * q;
            if (h * 1024 >= bhi || (h + 1) * 1024 <= blo) continue;        /* wave-uniform */
            const int byte = h * 1024 + lane * 16;
            const int64_t r = (int64_t)(rj[q] - X.jb0 + HALO) * l + rk[q];
            if (byte < nb)
                __builtin_amdgcn_global_load_lds((glb_void*)(x + NUN * (r * nx + i0) + byte / 8),
                                                 (lds_void*)(xs + (q * (SP7_T + 2) + 1) * NUN + h * 128), 16, 0, 0);
    }
        if (t < 72) {
            const int q = t / 12, side = (t / NUN) & 1, var = t - NUN * (t / NUN);
            const int p = side ? nc + 1 : 0;
            const int64_t r = (int64_t)(rj[q] - X.jb0 + HALO) * l + rk[q];
            const int64_t cell = xnb_cell(r, i0 + p - 1, X.n, X.ib0, nx, X.hx, X.periodic, X.xb);
            xs[(q * (SP7_T + 2) + p) * NUN + var] = x[NUN * cell + var];
    }
    }
    __syncthreads();
    if (act) {
        if (g == 0) sp7_compute<0, 26>(v, xs, c, acc);
        else if (g == 1) sp7_compute<26, 52>(v, xs, c, acc);
        else if (g == 2) sp7_compute<52, 78>(v, xs, c, acc);
        else sp7_compute<78, 104>(v, xs, c, acc);
    }
#pragma unroll
    for (int q = 0; q < 3; q++) red[g][q][c] = acc[q];
    __syncthreads();
    /* rows of the groups: g0 {U,V} g1 {V,W} g2 {W,P,T} g3 {T,S}; the tile's active cells are
     * consecutive in the compressed vector, so its rows [6 cm(clo), 6 cm(chi) + 6) are one
     * contiguous run: thread o writes entry o of it */
    const int na = td.w;
    for (int o = t; o < na * NUN; o += 256) {
        const int ac = o / NUN, R = o - ac * NUN;
        const int cc = lof[ac];
        double vv;
        switch (R) {
        case 0: vv = red[0][0][cc]; break;
        case 1: vv = red[0][1][cc] + red[1][0][cc]; break;
        case 2: vv = red[1][1][cc] + red[2][0][cc]; break;
        case 3: vv = red[2][1][cc]; break;
        case 4: vv = red[2][2][cc] + red[3][0][cc]; break;
        default: vv = red[3][1][cc]; break;
        }
        y[(int64_t)NUN * a0 + o] = vv;
    }
}

/* Dynamics defect of the block GS (prec_gs.hip's correction passes around gs_dyn.hip): d = rr - A z on the active U/V/W/P rows,
 * 0 on the others.  z is the pass iterate, 0 on the identity rows (whose couplings are in
 * rr, the block right-hand side) and on T/S, so rr - A z equals rr_D - A_DD z_D of the
 * block iteration.  One workgroup per 64 cells; the 64 slots of the four rows are split
 * evenly over the waves (U | U+V | V+W | W+P, 16 each), the gathers read z directly, and
 * the rows' partials meet in LDS.  z, rr, the flags and d are all component-planar (plane
 * stride ps: unit-stride along i; round 4 read r as 48-byte AoS records).  Skipping the W
 * row's four T/S slots (z(T, S) = 0) measured slower (24.7 against 22.5 us: the waves'
 * balance), so they are read. */
/* on[q]: row sp7_row(S0) + q of the cell is active; an identity row's coefficients are
 * neither loaded nor used (about half the cells are land at 2 degrees).  (Non-temporal
 * coefficient loads measured 35.6 against 26.1 us per defect, scripts/ab_probe.py.) */
/* The loads of each row are issued in one predicated block (per-slot predicates made the
 * compiler wait for every load before the next: 64 vmcnt(0) per wave), then the products
 * are summed in slot order. */
template <int S0, int S1>
__device__ __forceinline__ void dyn_partial(const double* __restrict__ val, const double* __restrict__ z,
                                            int64_t vs, const int (*nc)[9], const bool* on,
                                            int64_t ps, double* acc)
{
    constexpr int NS = S1 - S0;
    double v[NS], zz[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) v[s] = zz[s] = 0.0;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        if (!on[q]) continue;
#pragma unroll
        for (int s = S0; s < S1; s++) {
            const Slot sl = SLOTS[s];
            if (sp7_row(s) - sp7_row(S0) != q) continue;
            const int cidx = nc[sl.di + 1][(sl.dk + 1) * 3 + (sl.dj + 1)];
            v[s - S0] = val[(int64_t)s * vs];
            zz[s - S0] = z[(int64_t)cidx + ps * sl.var];
        }
    }
#pragma unroll
    for (int s = S0; s < S1; s++) {
        const int q = sp7_row(s) - sp7_row(S0);
        if (on[q]) acc[q] += v[s - S0] * zz[s - S0];
    }
}
/* hv (latitude bands): tiles past the owned ones compute the defect on the two halo rows
 * too (their coefficients exchanged once per Jacobian, ActiveSet::dvh; z with a 2-deep halo),
 * so that the next dynamics pass needs no exchange of d.  hs / hn: the south / north halo row
 * exists (a neighbour band).  alist: the owned tiles run over the active cells only (the
 * compressed basis' list, ActiveSet::act; about half the cells are land at 2 degrees): d of the
 * other cells stays 0 (gs_compute zeroes it whenever the list changes). */
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) k_spmv_dyn(SubLay X, const double* __restrict__ val,
                                                  const double* __restrict__ z,
                                                  const double* __restrict__ r,
                                                  const uint8_t* __restrict__ knP,
                                                  double* __restrict__ d, int64_t nloc, int nblk, int64_t ps,
                                                  const double* __restrict__ hv, int nhb, int hs, int hn,
                                                  const int* __restrict__ alist, int64_t nown,
                                                  const double* __restrict__ vb)
{
    __shared__ double red[4][2][64];
    __shared__ int64_t us[64];
    __shared__ int oks[64];
    const int ntot = nblk + nhb;
    const int per = (ntot + 7) >> 3;
    const int tile = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (tile >= ntot) return;
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t row = (int64_t)X.l * X.nx;             /* cells of one latitude row */
    const int64_t e0 = (int64_t)HALO * row;              /* ext cell of owned cell 0 */
    /* u: the cell relative to owned cell 0 (the halo rows at -row .. -1 and nloc .. nloc + row - 1) */
    const bool halo = tile >= nblk;
    int64_t h, u;
    bool act;
    if (!halo) {
        h = (int64_t)tile * 64 + c;
        act = h < nown;
        u = !act ? 0 : (alist ? (int64_t)alist[h] : h);
    } else {
        h = (int64_t)(tile - nblk) * 64 + c;             /* halo index: south row, then north */
        const bool south = h < row;
        act = h < 2 * row && (south ? hs : hn);
        u = south ? h - row : nloc + h - row;
    }
    if (g == 0) {
        us[c] = u;
        oks[c] = act ? 1 : 0;
    }
    double acc[2] = {0.0, 0.0};
    if (act) {
        const int64_t q = u + row;                       /* >= 0 */
        const int il = (int)(q % X.nx), k = (int)((q / X.nx) % X.l);
        const int j = X.jb0 - 1 + (int)(q / row);
        int nc[3][9];
        nb_cells(X, il, j, k, nc);
        /* the wave's two rows: g0 {U, -} g1 {U, V} g2 {V, W} g3 {W, P} */
        const int64_t cell = e0 + u;
        const int v0 = g == 0 ? 0 : g - 1;
        const bool on[2] = {!knP[cell + ps * v0], g > 0 && !knP[cell + ps * (v0 + 1)]};
        /* vb: the active cells' coefficients blocked per tile (h = tile 64 + c) */
        const double* vp = halo ? hv + h : (vb ? vb + (int64_t)tile * 4096 + c : val + u);
        const int64_t vs = halo ? 2 * row : (vb ? 64 : nloc);
        if (g == 0) dyn_partial<0, 16>(vp, z, vs, nc, on, ps, acc);
        else if (g == 1) dyn_partial<16, 32>(vp, z, vs, nc, on, ps, acc);
        else if (g == 2) dyn_partial<32, 48>(vp, z, vs, nc, on, ps, acc);
        else dyn_partial<48, 64>(vp, z, vs, nc, on, ps, acc);
    }
    red[g][0][c] = acc[0];
    red[g][1][c] = acc[1];
    __syncthreads();
    /* rows of the waves: g0 {U} g1 {U,V} g2 {V,W} g3 {W,P}; thread = (row, cell), the
     * cell fastest (planar stores) */
    const int R = threadIdx.x >> 6, cc = threadIdx.x & 63;
    if (!oks[cc]) return;
    const double sum = R == 0 ? red[0][0][cc] + red[1][0][cc]
                     : R == 1 ? red[1][1][cc] + red[2][0][cc]
                     : R == 2 ? red[2][1][cc] + red[3][0][cc]
                              : red[3][1][cc];
    const int64_t cell = e0 + us[cc], e = cell + ps * R;
    d[e] = knP[e] ? 0.0 : r[e] - sum;
}

int spmv_dyn_defect(iemic_ctx* c, const double* z, const double* r, const uint8_t* knP, double* d, bool halo)
{
    const BlockGS& gs = c->gs;
    const bool al = gs.act.act.p && gs.act.nact > 0;
    const int64_t nown = al ? gs.act.nact : c->sub.nloc;
    const int nblk = (int)((nown + 63) / 64);
    const int64_t row = (int64_t)c->l * c->sub.nx;
    const bool hv = halo && gs.act.dvh.p;
    const int nhb = hv ? (int)((2 * row + 63) / 64) : 0;
    const unsigned grid = xcd_grid(nblk + nhb);
    hipLaunchKernelGGL(k_spmv_dyn, dim3(grid), dim3(256), 0, c->stream, sub_lay(c->sub), gs.act.vp, z, r, knP, d,
                       c->sub.nloc, nblk, (int64_t)c->sub.next, hv ? gs.act.dvh.p : nullptr, nhb,
                       hv && c->sub.nb[2] >= 0 ? 1 : 0, hv && c->sub.nb[3] >= 0 ? 1 : 0,
                       al ? gs.act.act.p : nullptr, nown, al && gs.act.dvb.p ? gs.act.dvb.p : nullptr);
    return 0;
}

static int spmv_intcond(iemic_ctx* c, const double* x, double* yr);
/* the SpMV kernel(s) alone: x's halo rows must be current */
int spmv_kernel(iemic_ctx* c, const double* x, double* y)
{
    if (!c->jac_valid) {
        set_error("spmv: no Jacobian assembled");
        return IEMIC_ESTATE;
    }
    hipStream_t s = c->stream;
    if (c->sub.nloc >= INT32_MAX) {
        set_error("spmv: more than 2^31 cells per rank");
        return IEMIC_EINVAL;
    }
    const int tpr = (c->sub.nx + SP7_T - 1) / SP7_T;
    const int ntile = (int)(c->sub.nloc / c->sub.nx) * tpr;
    const unsigned grid = xcd_grid(ntile);
    hipLaunchKernelGGL(k_spmv7, dim3(grid), dim3(256), 0, s, sub_lay(c->sub), c->d_val.p, x, y, (int)c->sub.nloc, ntile,
                       tpr);
    return spmv_intcond(c, x, c->rowintcon >= 0 ? y + c->rowintcon : nullptr);
}

/* the dense integral-condition row: *yr = intSign * coeff . x (summed over the ranks; yr its
 * entry of this rank's output, if it owns it) */
static int spmv_intcond(iemic_ctx* c, const double* x, double* yr)
{
    hipStream_t s = c->stream;
    if (c->su.rowintcon_ref >= 0) {
        /* dense intcond row: y[rowintcon] = intSign * coeff . x (summed over the ranks) */
        const Owned w = owned(c);
        hipLaunchKernelGGL(k_mdot, dim3(RED_BLOCKS, 1), dim3(256), 0, s, c->d_intc.p + w.o, (int64_t)0, 1,
                           x + w.o, w.n, c->d_red.p);
        hipLaunchKernelGGL(k_mdot_final, dim3(1), dim3(256), 0, s, c->d_red.p, RED_BLOCKS, 1,
                           c->d_red.p + RED_BLOCKS);
        int rc = allreduce_sum(c, c->d_red.p + RED_BLOCKS, 1);
        if (rc) return rc;
        if (c->rowintcon >= 0)
            hipLaunchKernelGGL(k_scale_copy, dim3(1), dim3(1), 0, s, c->d_red.p + RED_BLOCKS,
                               (double)c->cfg.int_sign, yr, (int64_t)1);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

/* ev0 / ev1 (optional): the kernel's own start and end (hipExtLaunchKernelGGL records them
 * from the dispatch itself, so FGMRES times the SpMV kernel alone, as the trace does) */
int spmv_kernel_c(iemic_ctx* c, const double* x, double* yc, hipEvent_t ev0, hipEvent_t ev1)
{
    const BlockGS& gs = c->gs;
    if (!c->jac_valid || !gs.act.cmap.p || !gs.act.spc.p || !gs.act.atl.p || gs.act.coef_stale) {
        set_error("spmv: no Jacobian, no active-cell map or stale packed coefficients");
        return IEMIC_ESTATE;
    }
    hipStream_t s = c->stream;
    const int tpr = (c->sub.nx + SP7_T - 1) / SP7_T;
    const unsigned grid = xcd_grid(gs.act.natile);
    if (gs.act.natile > 0)
        hipExtLaunchKernelGGL(k_spmv7c, dim3(grid), dim3(256), 0, s, ev0, ev1, 0, sub_lay(c->sub),
                              (const double*)gs.act.spc.p, x, yc, (const int4*)gs.act.atl.p, gs.act.natile, tpr);
    double* yr = nullptr;
    if (c->rowintcon >= 0) {
        if (c->gs.act.ric < 0) {
            set_error("spmv: the integral-condition row lies in an inactive cell");
            return IEMIC_EINVAL;
        }
        yr = yc + c->gs.act.ric;
    }
    return spmv_intcond(c, x, yr);
}

/* W[b ldw + rowintcon] = s res[b], b < k: the dense row's entries of the block product */
__global__ void k_intcond_put(const double* __restrict__ res, double s, double* __restrict__ w, int64_t ldw, int k)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < k) w[(int64_t)b * ldw] = s * res[b];
}

template <int KB>
static void spmm_launch(iemic_ctx* c, const double* V, int64_t ldv, double* W, int64_t ldw, int ntile, int tpr)
{
    hipLaunchKernelGGL(k_spmm7<KB>, dim3(xcd_grid(ntile)), dim3(256), 0, c->stream, sub_lay(c->sub), c->d_val.p, V, ldv, W,
                       ldw, (int)c->sub.nloc, ntile, tpr);
}

/* W(:, b) = J V(:, b), b < k, on the owned rows: full blocks of kbmax columns (4, 2 or 1; 0: the
 * default), then the remainder in narrower blocks; the columns' halo rows must be current.
 * The dense integral-condition row follows spmv_intcond: one multi-dot of the k columns
 * against d_intc (the partials in d_part), one all-reduce of k values. */
int spmm_kernel(iemic_ctx* c, const double* V, int64_t ldv, int k, double* W, int64_t ldw, int kbmax)
{
    if (!c->jac_valid) {
        set_error("spmm: no Jacobian assembled");
        return IEMIC_ESTATE;
    }
    if (c->sub.nloc >= INT32_MAX) {
        set_error("spmm: more than 2^31 cells per rank");
        return IEMIC_EINVAL;
    }
    if (k < 1 || k > SPMM_MAX_K) {
        set_error("spmm: the number of columns must lie in 1 .. " + std::to_string(SPMM_MAX_K));
        return IEMIC_EINVAL;
    }
    const int kb = kbmax == 1 || kbmax == 2 || kbmax == 4 ? kbmax : SPMM_KB;
    const int tpr = (c->sub.nx + SP7_T - 1) / SP7_T;
    const int ntile = (int)(c->sub.nloc / c->sub.nx) * tpr;
    int b = 0;
    if (kb == 4)
        for (; b + 4 <= k; b += 4) spmm_launch<4>(c, V + b * ldv, ldv, W + b * ldw, ldw, ntile, tpr);
    if (kb >= 2)
        for (; b + 2 <= k; b += 2) spmm_launch<2>(c, V + b * ldv, ldv, W + b * ldw, ldw, ntile, tpr);
    for (; b < k; b++) spmm_launch<1>(c, V + b * ldv, ldv, W + b * ldw, ldw, ntile, tpr);
    HIP_OK(hipGetLastError());
    if (c->su.rowintcon_ref >= 0) {
        const Owned w = owned(c);
        double* part = c->d_part.p;
        double* res = part + (size_t)RED_BLOCKS * k;
        hipLaunchKernelGGL(k_mdot, dim3(RED_BLOCKS, k), dim3(256), 0, c->stream, V + w.o, ldv, k, c->d_intc.p + w.o, w.n,
                           part);
        hipLaunchKernelGGL(k_mdot_final, dim3(k), dim3(256), 0, c->stream, part, RED_BLOCKS, k, res);
        int rc = allreduce_sum(c, res, k);
        if (rc) return rc;
        if (c->rowintcon >= 0)
            hipLaunchKernelGGL(k_intcond_put, dim3(1), dim3(64), 0, c->stream, res, (double)c->cfg.int_sign,
                               W + c->rowintcon, ldw, k);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

int spmv(iemic_ctx* c, double* x, double* y, hipStream_t)
{
    int rc = halo_exchange(c, x, 1);
    if (rc) return rc;
    return spmv_kernel(c, x, y);
}

}  // namespace iemic
