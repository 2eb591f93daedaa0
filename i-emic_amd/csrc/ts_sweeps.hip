/*
 * ts_sweeps.hip -- the plain T/S sweeps of the block Gauss-Seidel preconditioner (ts_mg = 0;
 * step 6 of prec_gs.hip's overview): the T/S right-hand side rr_ts - B_ts,(u,v,w) z from the
 * dynamics iterate, then symmetric red-black Gauss-Seidel sweeps with 2x2 T/S cell blocks.  Even
 * n: the sweeps run on per-colour copies of the couplings (TsSweeps::tsc, tic, bc, zt, zs),
 * packed at set-up; otherwise on the generic layout, with two colours or (periodic, odd n) four.
 */
#include <algorithm>

#include "gs_internal.h"

namespace iemic {

namespace {

/* 6a. T/S right-hand side: rr_ts - B_ts,(u,v,w) z;  z_ts = 0 */
__global__ void k_gs_bts(const double* __restrict__ val, const uint8_t* __restrict__ known,
                         const double* __restrict__ rr, double* __restrict__ z, double* __restrict__ bts,
                         Lay L)
{
    LAY_ALIASES;
    OWNED_CELL;
    for (int R = TT; R <= SS; R++) {
        const int64_t row = NUN * cell + R;
        if (known[row]) continue;
        double acc = rr[row];
        for (int s = ROW_BEGIN[R]; s < ROW_BEGIN[R + 1]; s++) {
            const int var = SLOTS[s].var;
            if (var == TT || var == SS) continue;
            const double v = val[(int64_t)s * ncell + lc];
            if (v == 0.0) continue;
            int ii = i + SLOTS[s].di, jj = j + SLOTS[s].dj;
            const int kk = k + SLOTS[s].dk;
            if (kk < 0 || kk >= l || !hnb(ii, jj, n, m, periodic)) continue;
            const int64_t col = NUN * ecell(L, ii, jj, kk) + var;
            if (!known[col]) acc -= v * z[col];
        }
        bts[row] = acc;
        z[row] = 0.0;
    }
}

/* colour of a cell for the T/S sweeps: parity of i+j+k (global j); on a periodic grid with
 * odd n the wrap pairs (n-1, 0) would share a colour, so column i = n-1 gets colours 2/3 */
__device__ __forceinline__ int ts_color(int i, int j, int k, int n, int periodic)
{
    if (periodic && (n & 1) && i == n - 1) return 2 + ((j + k) & 1);
    return (i + j + k) & 1;
}

/* 6b. one red-black half sweep on the T/S block with 2x2 cell blocks (compact couplings;
 * generic layout, used for odd n) */
__global__ void __launch_bounds__(256) k_gs_ts_half(const double* __restrict__ tsoff,
                                                    const uint8_t* __restrict__ known,
                                                    const double* __restrict__ tsinv,
                                                    const double* __restrict__ bts,
                                                    double* __restrict__ z, Lay L, int64_t next,
                                                    int color)
{
    LAY_ALIASES;
    OWNED_CELL;
    if (ts_color(i, j, k, n, periodic) != color) return;
    const bool ta = !known[NUN * cell + TT], sa = !known[NUN * cell + SS];
    if (!ta && !sa) return;
    /* neighbour cells (clamped where the coupling is zero anyway) */
    int im = i - 1, ip = i + 1;
    if (periodic) { if (im < 0) im = n - 1; if (ip >= n) ip = 0; }
    else { if (im < 0) im = i; if (ip >= n) ip = i; }
    const int jm = j > 0 ? j - 1 : j, jp = j < m - 1 ? j + 1 : j;
    const int km = k > 0 ? k - 1 : k, kp = k < l - 1 ? k + 1 : k;
    const int64_t nb[6] = {ecell(L, im, j, k), ecell(L, ip, j, k), ecell(L, i, jm, k),
                           ecell(L, i, jp, k), ecell(L, i, j, km), ecell(L, i, j, kp)};
    double res[2];
#pragma unroll
    for (int R = 0; R < 2; R++) {
        const int var = TT + R, oth = SS - R;
        const double* a = tsoff + (int64_t)(R * 8) * next + cell;
        double acc = bts[NUN * cell + var];
#pragma unroll
        for (int q = 0; q < 6; q++) acc -= a[(int64_t)q * next] * z[NUN * nb[q] + var];
        acc -= a[(int64_t)6 * next] * z[NUN * nb[4] + oth];
        acc -= a[(int64_t)7 * next] * z[NUN * nb[5] + oth];
        res[R] = acc;
    }
    const double* D = tsinv + 4 * cell;
    if (ta) z[NUN * cell + TT] = D[0] * res[0] + D[1] * res[1];
    if (sa) z[NUN * cell + SS] = D[2] * res[0] + D[3] * res[1];
}

/* Even n: the owned cells of one colour are lc = 2q + ((j+k+c)&1) (lc = (row)*n + i with
 * row = (j-jb0)*l + k), so every per-cell T/S array can be stored per colour and read
 * contiguously by a half sweep:  tsc[(c*16 + e)*half + q] couplings,
 * tic[(c*4 + e)*half + q] 2x2 inverses, bc[(c*2 + v)*half + q] right-hand sides;
 * zt / zs: T and S iterates by ext cell (halo entries stay 0). */
__global__ void k_ts_pack(const double* __restrict__ tsoff, const double* __restrict__ tsinv,
                          double* __restrict__ tsc, double* __restrict__ tic, Lay L, int64_t next)
{
    OWNED_CELL;
    const int64_t half = ncell / 2;
    const int c = (i + j + k) & 1;
    const int64_t q = lc >> 1;
    for (int e = 0; e < TS_NC; e++) tsc[(int64_t)(c * TS_NC + e) * half + q] = tsoff[(int64_t)e * next + cell];
    for (int e = 0; e < 4; e++) tic[(int64_t)(c * 4 + e) * half + q] = tsinv[4 * cell + e];
}

/* T/S right-hand side bts = rr_TS - A_TS,D z_D into the colour layout; zt = zs = 0.
 * One wave per (64 cells, T or S row): the row's 10 dynamics slots unrolled at compile
 * time, neighbour indices clamped as in the SpMV (the ELL holds zeros outside the domain),
 * identity-row columns (their couplings are in rr already) skipped by the slot bitmask
 * kmask instead of a byte gather per slot.  Dealt to the XCDs in contiguous runs. */
__global__ void __launch_bounds__(128) k_gs_bts2(const double* __restrict__ val, const uint8_t* __restrict__ known,
                                                 const uint64_t* __restrict__ kmask,
                                                 const double* __restrict__ rr, const double* __restrict__ z,
                                                 double* __restrict__ bc, double* __restrict__ zt,
                                                 double* __restrict__ zs, Lay L, int nblk)
{
    LAY_ALIASES;
    const int tile = xcd_block(nblk);
    if (tile < 0) return;
    const int64_t lc = (int64_t)tile * 64 + (threadIdx.x & 63);
    if (lc >= L.nloc) return;
    const int R = TT + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int i, j, k;
    lc_ijk(L, lc, i, j, k);
    const int64_t cell = L.own0 + lc;
    int nc[3][9];
    nb_cells(sub_of(L), i - L.ib0, j, k, nc);
    const int64_t row = NUN * cell + R;
    double acc = 0.0;
    if (!known[row]) {
        const uint64_t kb = kmask[2 * cell + 1];
        acc = R == TT ? bts_row<TT>(val, z, lc, L.nloc, nc, kb, rr[row])
                      : bts_row<SS>(val, z, lc, L.nloc, nc, kb, rr[row]);
    }
    const int64_t half = L.nloc / 2;
    const int c = (i + j + k) & 1;
    bc[(int64_t)(c * 2 + (R - TT)) * half + (lc >> 1)] = acc;
    if (R == TT) zt[cell] = 0.0;
    else zs[cell] = 0.0;
}

__global__ void __launch_bounds__(256) k_gs_ts_half_c(const double* __restrict__ tsc,
                                                      const double* __restrict__ tic,
                                                      const double* __restrict__ bc,
                                                      double* __restrict__ zt, double* __restrict__ zs,
                                                      Lay L, int c)
{
    LAY_ALIASES;
    const int64_t half = L.nloc / 2;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= half) return;
    const int nx = L.nx;
    const int64_t row = (2 * q) / nx;                /* (j - jb0) * l + k */
    const int k = (int)(row % l), j = L.jb0 + (int)(row / l);
    const int64_t lc = 2 * q + ((j + k + c) & 1);    /* ib0 even: local parity = global */
    const int il = (int)(lc - row * nx);
    const int64_t cell = L.own0 + lc;
    const int64_t r = row + (int64_t)HALO * l;
    const int64_t ln = (int64_t)l * nx;
    const int64_t nb[6] = {xnb_cell(r, il - 1, n, L.ib0, nx, L.hx, periodic, L.xb),
                           xnb_cell(r, il + 1, n, L.ib0, nx, L.hx, periodic, L.xb),
                           j > 0 ? cell - ln : cell, j < m - 1 ? cell + ln : cell,
                           k > 0 ? cell - nx : cell, k < l - 1 ? cell + nx : cell};
    const double* a = tsc + (int64_t)(c * TS_NC) * half + q;
    double rt = bc[(int64_t)(c * 2) * half + q], rs = bc[(int64_t)(c * 2 + 1) * half + q];
#pragma unroll
    for (int e = 0; e < 6; e++) {
        rt -= a[(int64_t)e * half] * zt[nb[e]];
        rs -= a[(int64_t)(8 + e) * half] * zs[nb[e]];
    }
    rt -= a[(int64_t)6 * half] * zs[nb[4]] + a[(int64_t)7 * half] * zs[nb[5]];
    rs -= a[(int64_t)14 * half] * zt[nb[4]] + a[(int64_t)15 * half] * zt[nb[5]];
    const double* D = tic + (int64_t)(c * 4) * half + q;
    zt[cell] = D[0] * rt + D[half] * rs;
    zs[cell] = D[2 * half] * rt + D[3 * half] * rs;
}

/* z(T,S) = zt, zs on the active rows */
__global__ void k_ts_scatter(const uint8_t* __restrict__ known, const double* __restrict__ zt,
                             const double* __restrict__ zs, double* __restrict__ z, Lay L)
{
    OWNED_CELL;
    if (!known[NUN * cell + TT]) z[NUN * cell + TT] = zt[cell];
    if (!known[NUN * cell + SS]) z[NUN * cell + SS] = zs[cell];
}

}  // namespace

/* colour-compacted T/S sweeps: the owned cells of one colour are every other cell of a
 * row (even n, nx and ib0) */
static bool ts_compact(const iemic_ctx* c) { return (c->n & 1) == 0 && (c->sub.nx & 1) == 0 && (c->sub.ib0 & 1) == 0; }

/* set-up, with the other per-cell arrays (gs_reserve_cells): the per-colour arrays and the
 * iterates, whose halo entries stay 0; nonzero: out of device memory */
int ts_sweeps_reserve(iemic_ctx* c)
{
    TsSweeps& sw = c->gs.sw;
    int rc = 0;
    rc |= sw.tsc.alloc((size_t)TS_NC * c->sub.nloc);
    rc |= sw.tic.alloc((size_t)4 * c->sub.nloc);
    rc |= sw.bc.alloc((size_t)2 * c->sub.nloc);
    rc |= sw.zt.alloc(c->sub.next);
    rc |= sw.zs.alloc(c->sub.next);
    if (rc) return rc;
    for (DevBuf<double>* bptr : {&sw.zt, &sw.zs})
        HIP_OK(hipMemsetAsync(bptr->p, 0, sizeof(double) * bptr->n, c->stream));
    return 0;
}

/* set-up: the couplings and the 2x2 inverses per colour, where the sweeps are colour-compacted */
void ts_sweeps_pack(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    if (ts_compact(c))
        hipLaunchKernelGGL(k_ts_pack, dim3(blocks_for(c->sub.nloc)), dim3(256), 0, c->stream, gs.sw.tsoff.p,
                           gs.sw.tsinv.p, gs.sw.tsc.p, gs.sw.tic.p, lay_of(c->sub), c->sub.next);
}

/* the T/S block solve by BlockGS::ts_sweeps symmetric red-black sweeps: right-hand side from
 * the dynamics rows of the output z (AoS), result into its T/S rows */
int ts_sweeps_solve(iemic_ctx* c, double* z)
{
    BlockGS& gs = c->gs;
    const Lay L = lay_of(c->sub);
    const int n = c->n;
    hipStream_t s = c->stream;
    const unsigned gc = blocks_for(c->sub.nloc);
    const int nsw = std::max(1, gs.ts_sweeps);
    if (ts_compact(c)) {
        /* colour-compacted symmetric red-black sweeps */
        const int nblk = (int)((c->sub.nloc + 63) / 64);
        hipLaunchKernelGGL(k_gs_bts2, dim3(xcd_grid(nblk)), dim3(128), 0, s, gs.act.vp,
                           gs.known.p, gs.kmask.p, gs.rr.p, z, gs.sw.bc.p, gs.sw.zt.p, gs.sw.zs.p, L, nblk);
        const unsigned gh = blocks_for(c->sub.nloc / 2);
        const int seq[4] = {0, 1, 1, 0};
        for (int sw = 0; sw < nsw; sw++)
            for (int h = 0; h < 4; h++)
                hipLaunchKernelGGL(k_gs_ts_half_c, dim3(gh), dim3(256), 0, s, gs.sw.tsc.p, gs.sw.tic.p, gs.sw.bc.p,
                                   gs.sw.zt.p, gs.sw.zs.p, L, seq[h]);
        hipLaunchKernelGGL(k_ts_scatter, dim3(gc), dim3(256), 0, s, gs.known.p, gs.sw.zt.p, gs.sw.zs.p, z, L);
    } else {
        /* symmetric sweeps: colours forward then backward */
        hipLaunchKernelGGL(k_gs_bts, dim3(gc), dim3(256), 0, s, gs.act.vp, gs.known.p, gs.rr.p, z,
                           gs.sw.bts.p, L);
        const bool four = c->cfg.periodic && (n & 1);
        const int seq2[4] = {0, 1, 1, 0}, seq4[8] = {0, 1, 2, 3, 3, 2, 1, 0};
        const int* seq = four ? seq4 : seq2;
        const int ns = four ? 8 : 4;
        for (int sw = 0; sw < nsw; sw++)
            for (int h = 0; h < ns; h++)
                hipLaunchKernelGGL(k_gs_ts_half, dim3(gc), dim3(256), 0, s, gs.sw.tsoff.p, gs.known.p,
                                   gs.sw.tsinv.p, gs.sw.bts.p, z, L, c->sub.next, seq[h]);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace iemic
