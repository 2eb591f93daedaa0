/*
 * ts_mg_setup.hip -- set-up of the T/S aggregation multigrid (ts_mg.hip has the apply and
 * describes the method and the level layout), once per Jacobian: level 0 packed from the
 * compact T/S couplings, the Galerkin chain, the z-line factors, and the coarsest level's
 * inverse by one of three routes (ts_mg_setup) -- a whole-problem cyclic reduction over the
 * longitudes, a dense inverse on the device, or through the host, which with subdomains
 * also builds their global coarsest problem (mg_global_setup).
 */
#include <algorithm>
#include <cmath>
#include <vector>

#include "ts_mg_internal.h"

namespace iemic {

namespace {

/* neighbour q (-i,+i,-j,+j,-k,+k) of (i,jl,k): false outside the level's (visible) band */
__device__ __forceinline__ bool mg_nb(const TsLev& V, int q, int& i, int& jl, int& k)
{
    switch (q) {
    case 0: i--; break;
    case 1: i++; break;
    case 2: jl--; break;
    case 3: jl++; break;
    case 4: k--; break;
    default: k++; break;
    }
    if (jl < -V.vis || jl >= V.mb + V.vis || k < 0 || k >= V.l) return false;
    if (i < -V.visi || i >= V.n + V.visi) {
        if (!V.periodic) return false;
        i = (i + V.n) % V.n;
    }
    return true;
}
/* level 0: the compact T/S couplings and 2x2 blocks (ext layout) into the level layout */
__global__ void k_mg_pack0(const double* __restrict__ tsoff, const double* __restrict__ tsdiag, Lay L,
                           int64_t next, TsLev V, double* __restrict__ off, double* __restrict__ diag)
{
    OWNED_CELL;
    const int64_t c = mg_cell(V, i - L.ib0, j - L.jb0, k);
#pragma unroll
    for (int e = 0; e < 16; e++) off[(int64_t)e * V.cstr + c] = tsoff[(int64_t)e * next + cell];
#pragma unroll
    for (int e = 0; e < 4; e++) diag[(int64_t)e * V.cstr + c] = tsdiag[(int64_t)e * next + cell];
}

/* the entry kernel's operand (ts_mg_internal.h): one thread per (tile, cell of the tile); an
 * active cell writes its 2 MG_NE terms, a slot that couples to an identity column (kmask) as
 * the 0.0 bts_row puts in its place */
__global__ void k_mg_entry_pack(const double* __restrict__ val, const uint64_t* __restrict__ kmask,
                                const uint64_t* __restrict__ etl, int nw, Lay L, int64_t nt,
                                double* __restrict__ ep)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    const int tc = MG_TI * L.l, tiles = (L.nx + MG_TI - 1) / MG_TI;
    const int q = (int)(t % tc);
    const int64_t tile = t / tc;
    const uint64_t* e = etl + tile * (2 + nw);
    if (!((e[2 + (q >> 6)] >> (q & 63)) & 1)) return;
    const int64_t na = (int64_t)e[1];
    double* p = ep + (int64_t)e[0] + mg_entry_rank(e, q);
    const int jl = (int)(tile / tiles), i = (int)(tile % tiles) * MG_TI + q % MG_TI, k = q / MG_TI;
    const int64_t lc = ((int64_t)jl * L.l + k) * L.nx + i;
    const uint64_t kb = kmask[2 * (L.own0 + lc) + 1];
#pragma unroll
    for (int R = 0; R < 2; R++)
#pragma unroll
        for (int d = 0; d < MG_NE; d++) {
            const int s = MG_ES.s[R][d];
            p[(R * MG_NE + d) * na] = ((kb >> (s - 64)) & 1) ? 0.0 : val[(int64_t)s * L.nloc + lc];
        }
}

/* Galerkin coarse operator: sum of the children's blocks and couplings; couplings inside
 * the aggregate go to the coarse 2x2 block */
__global__ void k_mg_galerkin(TsLev F, TsLev C, double* __restrict__ off, double* __restrict__ diag)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)C.n * C.mb * C.l) return;
    const int k = (int)(t % C.l), I = (int)((t / C.l) % C.n), J = (int)(t / ((int64_t)C.l * C.n));
    const int64_t fs = F.cstr;
    double o[16], d[4] = {0.0, 0.0, 0.0, 0.0};
    for (int e = 0; e < 16; e++) o[e] = 0.0;
    for (int b = 0; b < 2; b++)
        for (int a = 0; a < 2; a++) {
            const int i = 2 * I + a, jl = 2 * J + b;
            if (i >= F.n || jl >= F.mb) continue;
            const int64_t c = mg_cell(F, i, jl, k);
            for (int e = 0; e < 4; e++) d[e] += F.diag[(int64_t)e * fs + c];
            for (int R = 0; R < 2; R++)
                for (int q = 0; q < 8; q++) {
                    const double v = F.off[(int64_t)(8 * R + q) * fs + c];
                    if (v == 0.0) continue;
                    int ii = i, jj = jl, kk = k;
                    if (!mg_nb(F, q < 6 ? q : q - 2, ii, jj, kk)) continue;
                    if (q < 6 && ii >= 0 && ii < F.n && jj >= 0 && jj < F.mb && (ii >> 1) == I && (jj >> 1) == J &&
                        kk == k)
                        d[3 * R] += v;                    /* same variable, same aggregate */
                    else
                        o[8 * R + q] += v;
                }
        }
    const bool at = d[0] != 0.0, as = d[3] != 0.0;
    if (!at) { d[1] = d[2] = 0.0; for (int q = 0; q < 8; q++) o[q] = 0.0; }
    if (!as) { d[1] = d[2] = 0.0; for (int q = 8; q < 16; q++) o[q] = 0.0; }
    /* the level's layout (a level with an x halo pads its rows) */
    const int64_t cs = C.cstr, cc = mg_cell(C, I, J, k);
    for (int e = 0; e < 16; e++) off[(int64_t)e * cs + cc] = o[e];
    for (int e = 0; e < 4; e++) diag[(int64_t)e * cs + cc] = d[e];
}

/* z-line factors of every owned column (one thread each, serial block Thomas along k, the
 * CPU twin's mg_zline arithmetic): A'_k = A_k - B_k Cp_{k-1}, F_k = -A'_k^-1 B_k, Cp_k =
 * A'_k^-1 C_k; inactive unknowns (zero diagonal) are identity rows whose A'^-1 and F rows
 * are zeroed, so their line values come out 0 whatever the right-hand side */
__global__ void k_mg_fac(TsLev V, double* __restrict__ fac)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= V.n * V.mb) return;
    const int i = t % V.n, jl = t / V.n;
    const int64_t cs = V.cstr;
    double P0 = 0.0, P1 = 0.0, P2 = 0.0, P3 = 0.0;
    for (int k = 0; k < V.l; k++) {
        const int64_t c = mg_cell(V, i, jl, k);
        double Am[4] = {V.diag[c], V.diag[cs + c], V.diag[2 * cs + c], V.diag[3 * cs + c]};
        double Bm[4] = {V.off[4 * cs + c], V.off[6 * cs + c], V.off[14 * cs + c], V.off[12 * cs + c]};
        double Cm[4] = {V.off[5 * cs + c], V.off[7 * cs + c], V.off[15 * cs + c], V.off[13 * cs + c]};
        const bool at = Am[0] != 0.0, as = Am[3] != 0.0;
        if (!at) { Am[0] = 1.0; Am[1] = Am[2] = 0.0; Bm[0] = Bm[1] = 0.0; Cm[0] = Cm[1] = 0.0; }
        if (!as) { Am[3] = 1.0; Am[1] = Am[2] = 0.0; Bm[2] = Bm[3] = 0.0; Cm[2] = Cm[3] = 0.0; }
        if (k == 0) Bm[0] = Bm[1] = Bm[2] = Bm[3] = 0.0;
        else {
            const double a0 = Am[0] - (Bm[0] * P0 + Bm[1] * P2), a1 = Am[1] - (Bm[0] * P1 + Bm[1] * P3);
            const double a2 = Am[2] - (Bm[2] * P0 + Bm[3] * P2), a3 = Am[3] - (Bm[2] * P1 + Bm[3] * P3);
            Am[0] = a0; Am[1] = a1; Am[2] = a2; Am[3] = a3;
        }
        const double det = Am[0] * Am[3] - Am[1] * Am[2];
        const double qd = det != 0.0 ? 1.0 / det : 0.0;
        double I0 = Am[3] * qd, I1 = -Am[1] * qd, I2 = -Am[2] * qd, I3 = Am[0] * qd;
        P0 = I0 * Cm[0] + I1 * Cm[2]; P1 = I0 * Cm[1] + I1 * Cm[3];
        P2 = I2 * Cm[0] + I3 * Cm[2]; P3 = I2 * Cm[1] + I3 * Cm[3];
        double F0 = -(I0 * Bm[0] + I1 * Bm[2]), F1 = -(I0 * Bm[1] + I1 * Bm[3]);
        double F2 = -(I2 * Bm[0] + I3 * Bm[2]), F3 = -(I2 * Bm[1] + I3 * Bm[3]);
        if (!at) { I0 = I1 = F0 = F1 = 0.0; }
        if (!as) { I2 = I3 = F2 = F3 = 0.0; }
        const double v[12] = {F0, F1, F2, F3, I0, I1, I2, I3, P0, P1, P2, P3};
#pragma unroll
        for (int e = 0; e < 12; e++) fac[(int64_t)e * cs + c] = v[e];
    }
}

}  // namespace

/* Gauss-Jordan inverse with partial pivoting (host, large coarsest levels); unknowns
 * without any coupling (inactive) get an identity row */
static void dense_inverse(std::vector<double>& A, int N, std::vector<double>& X)
{
    X.assign((size_t)N * N, 0.0);
    for (int i = 0; i < N; i++) {
        X[(size_t)i * N + i] = 1.0;
        bool any = false;
        for (int j = 0; j < N; j++) any |= A[(size_t)i * N + j] != 0.0;
        if (!any) A[(size_t)i * N + i] = 1.0;
    }
    for (int k = 0; k < N; k++) {
        int p = k;
        for (int i = k + 1; i < N; i++)
            if (std::fabs(A[(size_t)i * N + k]) > std::fabs(A[(size_t)p * N + k])) p = i;
        if (p != k)
            for (int j = 0; j < N; j++) {
                std::swap(A[(size_t)p * N + j], A[(size_t)k * N + j]);
                std::swap(X[(size_t)p * N + j], X[(size_t)k * N + j]);
            }
        const double d = A[(size_t)k * N + k];
        const double q = d != 0.0 ? 1.0 / d : 0.0;
        for (int j = 0; j < N; j++) {
            A[(size_t)k * N + j] *= q;
            X[(size_t)k * N + j] *= q;
        }
        for (int i = 0; i < N; i++) {
            if (i == k) continue;
            const double f = A[(size_t)i * N + k];
            if (f == 0.0) continue;
            for (int j = 0; j < N; j++) {
                A[(size_t)i * N + j] -= f * A[(size_t)k * N + j];
                X[(size_t)i * N + j] -= f * X[(size_t)k * N + j];
            }
        }
    }
}

/* the global coarse grid: rank (px, py)'s coarsest grid at column offset ioff[px], row offset
 * joff[py] of GX x GY cells; band half-widths and row width of its matrix */
struct MgGlob {
    std::vector<int> ioff, joff;
    int GX, GY, I0, J0, NG, bl, bu, W;
};
static int mg_global_grid(iemic_ctx* c, MgGlob& G)
{
    BlockGS& gs = c->gs;
    const Sub& S = c->sub;
    const int P = S.nranks, l = c->l, qc = gs.mg.nlev - 1;
    int rc;
    /* coarsest columns / rows of every rank: offsets of its rank column / row */
    std::vector<double> dims(2 * P, 0.0);
    dims[2 * S.rank] = gs.mg.n[qc];
    dims[2 * S.rank + 1] = gs.mg.m[qc];
    {
        DevBuf<double> rb;
        if (rb.alloc(2 * P)) return IEMIC_ENOMEM;
        if ((rc = h2d(c, rb.p, dims.data(), sizeof(double) * 2 * P))) return rc;
        if ((rc = allreduce_sum(c, rb.p, 2 * P))) return rc;
        if ((rc = d2h(c, dims.data(), rb.p, sizeof(double) * 2 * P))) return rc;
    }
    G.ioff.assign(S.npx + 1, 0);
    G.joff.assign(S.npy + 1, 0);
    for (int px = 0; px < S.npx; px++) G.ioff[px + 1] = G.ioff[px] + (int)dims[2 * px];
    for (int py = 0; py < S.npy; py++) G.joff[py + 1] = G.joff[py] + (int)dims[2 * (py * S.npx) + 1];
    G.GX = G.ioff[S.npx];
    G.GY = G.joff[S.npy];
    G.I0 = G.ioff[S.px];
    G.J0 = G.joff[S.py];
    G.NG = 2 * G.GX * G.GY * l;
    G.bl = 2 * l * G.GX + 1;
    G.bu = G.bl;
    G.W = 2 * G.bl + G.bu + 1;
    return 0;
}

/* this rank's rows of the global band matrix H; *ok = false: an entry outside the band */
static int mg_global_rows(iemic_ctx* c, const MgGlob& G, const std::vector<double>& off,
                          const std::vector<double>& dg, std::vector<double>& H, bool* okp)
{
    BlockGS& gs = c->gs;
    const int l = c->l, qc = gs.mg.nlev - 1;
    const int nc = gs.mg.n[qc], cm = gs.mg.m[qc], mb = c->sub.mb;
    const int64_t ncl = (int64_t)nc * cm * l;
    int rc;
    H.assign((size_t)G.NG * G.W, 0.0);
    const bool wrap = c->cfg.periodic != 0;
    auto gidx = [&](int J, int I, int k, int var) { return 2 * ((J * G.GX + I) * l + k) + var; };
    auto gwrap = [&](int I) { return I < 0 ? I + G.GX : (I >= G.GX ? I - G.GX : I); };
    auto add = [&](int row, int col, double v) {
        const int d = col - row;
        if (d < -G.bl || d > G.bu) return false;
        H[(size_t)row * G.W + (d + G.bl)] += v;
        return true;
    };
    bool ok = true;
    const bool lwrap = wrap && c->sub.npx == 1;           /* the local level wraps in x */
    for (int64_t t = 0; t < ncl; t++) {
        int i, jl, k;
        mg_decode(t, nc, l, i, jl, k);
        for (int R = 0; R < 2; R++) {
            const int row = gidx(G.J0 + jl, G.I0 + i, k, R);
            mg_coarse_row(R, i, jl, k, nc, cm, l, lwrap, dg[(3 * R) * ncl + t], dg[(1 + R) * ncl + t],
                          &off[(8 * R) * ncl + t], ncl, [&](int ii, int jj, int kk, int var, int, double v) {
                              ok &= add(row, gidx(G.J0 + jj, G.I0 + ii, kk, var), v);
                          });
        }
    }
    /* cross-subdomain couplings: level-0 T/S couplings of the first / last latitude row (-j /
     * +j) and the first / last column (-i / +i), summed into the edge aggregates */
    {
        const int64_t nx = c->sub.nx, slab = (int64_t)l * nx;
        std::vector<double> e((size_t)slab * mb);
        for (int dir = 0; dir < 4; dir++) {
            if (c->sub.nb[dir] < 0) continue;
            const int q = dir == 0 ? 0 : dir == 1 ? 1 : dir == 2 ? 2 : 3;   /* -i, +i, -j, +j */
            for (int R = 0; R < 2; R++) {
                /* the owned rows of coupling q of row R (ext layout: one slab) */
                const double* src = gs.sw.tsoff.p + (int64_t)(R * 8 + q) * c->sub.next + c->sub.own0;
                if ((rc = d2h(c, e.data(), src, sizeof(double) * e.size()))) return rc;
                for (int jl = 0; jl < mb; jl++)
                    for (int k = 0; k < l; k++)
                        for (int il = 0; il < nx; il++) {
                            const bool edge = dir == 0 ? il == 0 : dir == 1 ? il == nx - 1 : dir == 2 ? jl == 0 : jl == mb - 1;
                            if (!edge) continue;
                            const double v = e[((int64_t)jl * l + k) * nx + il];
                            if (v == 0.0) continue;
                            const int Is = G.I0 + (il >> qc), Js = G.J0 + (jl >> qc);
                            const int Id = dir == 0 ? gwrap(G.I0 - 1) : dir == 1 ? gwrap(G.ioff[c->sub.px + 1]) : Is;
                            const int Jd = dir == 2 ? G.J0 - 1 : dir == 3 ? G.joff[c->sub.py + 1] : Js;
                            ok &= add(gidx(Js, Is, k, R), gidx(Jd, Id, k, R), v);
                        }
            }
        }
    }
    *okp = ok;
    if (!ok) return 0;
    /* own rows without entries (inactive unknowns) become identity rows */
    for (int jl = 0; jl < cm; jl++)
        for (int i = 0; i < nc; i++)
            for (int k = 0; k < l; k++)
                for (int R = 0; R < 2; R++) {
                    const int row = gidx(G.J0 + jl, G.I0 + i, k, R);
                    bool any = false;
                    for (int d = 0; d < G.W; d++) any |= H[(size_t)row * G.W + d] != 0.0;
                    if (!any) H[(size_t)row * G.W + G.bl] = 1.0;
                }
    return 0;
}

/* Subdomains: the coarsest T/S level as one global problem.  The ranks' coarsest grids
 * tile a GX x GY coarse grid (rank (px, py) at column offset ioff[px], row offset joff[py]);
 * unknown (J, I, k, var) is 2((J GX + I) l + k) + var, a band matrix of half-width
 * 2 l GX + 1 (+ the periodic wrap inside a row).  Every rank writes its own rows -- its
 * local coarsest operator plus the couplings of its edge aggregates to the neighbours'
 * edge aggregates, taken from the level-0 couplings across the subdomain edges (the
 * Galerkin sum of piecewise-constant aggregates) -- the rows are summed over the ranks,
 * and every rank factorises and inverts the whole matrix (band_lu.hip). */
static int mg_global_setup(iemic_ctx* c, const std::vector<double>& off, const std::vector<double>& dg)
{
    BlockGS& gs = c->gs;
    gs.mg.glob = 0;
    if (c->sub.nranks <= 1 || c->l > 64) return 0;
    int rc;
    MgGlob G;
    if ((rc = mg_global_grid(c, G))) return rc;
    const int NG = G.NG, bl = G.bl, bu = G.bu, W = G.W;
    {
        /* LDS of the band kernels (same rules as the Schur band) */
        const size_t lb = sizeof(double) * ((size_t)(BAND_NBP + bl) * (BAND_NBP + 1) + (size_t)BAND_NBP * (bl + bu));
        const size_t li = sizeof(double) * (size_t)(std::max(bl + BAND_NBP + 1, bl + bu + 1) + 2 * BAND_NBP) * 16;
        if (lb > 150 * 1024 || li > 150 * 1024 || (int64_t)NG * W > INT32_MAX) return 0;   /* stay local */
    }
    std::vector<double> H;
    bool ok = true;
    if ((rc = mg_global_rows(c, G, off, dg, H, &ok))) return rc;
    if (!ok) return 0;                        /* outside the assumed band: stay local */
    const size_t npan = (size_t)(NG + BAND_NBP - 1) / BAND_NBP;
    if (gs.mg.gband.n < (size_t)NG * W) {
        if (gs.mg.gband.alloc((size_t)NG * W) || gs.mg.gX.alloc((size_t)NG * NG) ||
            gs.mg.gvec.alloc(NG) || gs.mg.gtmp.alloc(NG) || gs.mg.gpiv.alloc(NG) ||
            gs.mg.ginfo.alloc(1) || gs.mg.gcols.alloc(NG) ||
            gs.mg.glpan.alloc(npan * (BAND_NBP + bl) * BAND_NBP))
            return IEMIC_ENOMEM;
        std::vector<int> cols(NG);
        for (int q = 0; q < NG; q++) cols[q] = q;
        if ((rc = h2d(c, gs.mg.gcols.p, cols.data(), sizeof(int) * NG))) return rc;
    }
    if ((rc = h2d(c, gs.mg.gband.p, H.data(), sizeof(double) * H.size()))) return rc;
    if ((rc = allreduce_sum(c, gs.mg.gband.p, (int)((size_t)NG * W)))) return rc;
    int info = 0;
    if ((rc = band_lu_inverse(c, gs.mg.gband.p, NG, bl, bu, gs.mg.gpiv.p, gs.mg.ginfo.p, gs.mg.glpan.p,
                              gs.mg.gcols.p, gs.mg.gX.p, &info)))
        return rc;
    if (info != 0) return 0;                  /* singular global coarse problem: local */
    gs.mg.gN = NG;
    gs.mg.gGX = G.GX;
    gs.mg.gI0 = G.I0;
    gs.mg.gJ0 = G.J0;
    gs.mg.glob = 1;
    return 0;
}

/* the coarsest level's dense operator, row-major A[row * N + col] (one thread per row),
 * inactive rows -> identity rows */
__global__ void k_mg_coarse_dense(const double* __restrict__ off, const double* __restrict__ dg, int64_t ncl,
                                  int cn, int cm, int l, int periodic, double* __restrict__ A)
{
    const int64_t rowq = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (rowq >= 2 * ncl) return;
    const int R = (int)(rowq / ncl);
    const int64_t t = rowq % ncl;
    const int64_t N = 2 * ncl;
    double* Ar = A + rowq * N;
    int i, jl, k;
    mg_decode(t, cn, l, i, jl, k);
    mg_coarse_row(R, i, jl, k, cn, cm, l, periodic != 0, dg[(3 * R) * ncl + t], dg[(1 + R) * ncl + t],
                  off + (8 * R) * ncl + t, ncl, [&](int ii, int jj, int kk, int var, int, double v) {
                      Ar[var * ncl + ((int64_t)jj * cn + ii) * l + kk] += v;
                  });
    bool any = false;
    for (int64_t c = 0; c < N; c++) any |= Ar[c] != 0.0;
    if (!any) Ar[rowq] = 1.0;
}

/* the coarsest level's operator as cyclic-reduction blocks over longitudes (one rank, no
 * halo): block i holds the unknowns (jl l + k) 2 + var of longitude i; D_i couples them
 * within the longitude (2x2 cell block, -+j, -+k, the T/S cross couplings along k), L_i / R_i
 * to longitude i -+ 1 (wrapping when periodic).  Inactive unknowns become identity rows.
 * One thread per (cell, var) row: no write races. */
__global__ void k_mg_cr_expand(TsLev V, int mc, int periodic, double* __restrict__ D, double* __restrict__ Lb,
                               double* __restrict__ Rb)
{
    const int64_t ncl = (int64_t)V.n * V.mb * V.l;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= 2 * ncl) return;
    const int R = (int)(q / ncl);
    const int64_t t = q % ncl;
    int i, jl, k;
    mg_decode(t, V.n, V.l, i, jl, k);
    const int64_t cs = V.cstr, c = mg_cell(V, i, jl, k);
    const size_t mm = (size_t)mc * mc;
    auto idx = [&](int j2, int k2, int var) { return (j2 * V.l + k2) * 2 + var; };
    const int r = idx(jl, k, R);
    double* Di = D + (size_t)i * mm;
    const double dself = V.diag[(int64_t)(3 * R) * cs + c];
    if (dself == 0.0) {
        Di[r + (size_t)r * mc] = 1.0;
        return;
    }
    /* a -i / +i entry goes to this longitude's L / R block (at the edge the walk drops it
     * unless periodic), every other one to D */
    mg_coarse_row(R, i, jl, k, V.n, V.mb, V.l, periodic != 0, dself, V.diag[(int64_t)(1 + R) * cs + c],
                  V.off + (int64_t)(8 * R) * cs + c, cs, [&](int, int jj, int kk, int var, int dir, double v) {
                      double* B = dir == 0 ? Lb + (size_t)i * mm : dir == 1 ? Rb + (size_t)i * mm : Di;
                      B[r + (size_t)idx(jj, kk, var) * mc] += v;
                  });
}

/* the whole-problem inverse of the cyclic reduction (row-major, longitude-block order) in
 * the level's unknown order var ncl + cell, row-major -- what the coarse GEMV applies */
__global__ void k_mg_cr_perm(const double* __restrict__ T, TsLev V, int N, double* __restrict__ X)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)N * N) return;
    const int64_t ncl = N / 2;
    const int rq = (int)(e / N), cq = (int)(e % N);
    auto cr_of = [&](int u) {
        const int var = (int)(u / ncl);
        int i, jl, k;
        mg_decode(u % ncl, V.n, V.l, i, jl, k);
        return (int64_t)i * (2 * V.mb * V.l) + (jl * V.l + k) * 2 + var;
    };
    X[e] = T[cr_of(rq) * N + cr_of(cq)];
}

/* level sizes, colour parities and the levels' arrays (first set-up); ts_mg = 0 where the
 * grid has no coarse level */
static int mg_levels(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    const int l = c->l;
    int rc;
    /* latitude bands, one sweep: level 0 keeps 2 halo rows (mg_vcycle) */
    gs.mg.hr = c->sub.npy > 1 && c->sub.npx == 1 && std::max(1, gs.mg.sweeps) == 1;
    /* coarsen 2x2 horizontally until the level has <= 128 cells (<= 256 unknowns); the
     * number of levels is that of the largest subdomain, the same on every rank, so the
     * coarsest grids of the ranks tile the global coarsest problem */
    int N = (c->n + c->sub.npx - 1) / c->sub.npx, M = (c->m + c->sub.npy - 1) / c->sub.npy, q = 0;
    int n = c->sub.nx, m = c->sub.mb;
    gs.mg.n[0] = n;
    gs.mg.m[0] = m;
    gs.mg.crd = 0;
    /* one rank: stop at the first level of <= TsMg::CR_CELLS cells that the whole-problem
     * cyclic reduction takes (blocks of one longitude, 2 m l <= CR_BLOCK_MAX unknowns, >= 2
     * longitudes): an exact coarse solve, one GEMV per V-cycle instead of the last
     * levels' ~9 latency-bound launches */
    auto cr_ok = [&](int nn, int mm) {
        return c->sub.nranks == 1 && (int64_t)nn * mm * l <= TsMg::CR_CELLS && 2 * mm * l <= CR_BLOCK_MAX && nn >= 2;
    };
    while (q + 1 < TsMg::MAX && (q == 0 || (int64_t)N * M * l > 128) && (N > 1 || M > 1) &&
           !(q > 0 && cr_ok(n, m))) {
        N = (N + 1) / 2;
        M = (M + 1) / 2;
        n = (n + 1) / 2;
        m = (m + 1) / 2;
        q++;
        gs.mg.n[q] = n;
        gs.mg.m[q] = m;
    }
    if (q == 0) {
        gs.ts_mg = 0;            /* a single water column per band: plain sweeps */
        return 0;
    }
    gs.mg.crd = cr_ok(n, m) && (int64_t)n * m * l > 128 ? 1 : 0;
    if (gs.mg.crd && (rc = cr_init(c, gs.mg.cr, n, 2 * m * l, c->cfg.periodic, 2 * n * m * l))) return rc;
    if ((int64_t)n * m * l > 1024) {
        set_error("block GS: T/S multigrid coarsest level too large");
        return IEMIC_EINVAL;
    }
    gs.mg.nlev = q + 1;
    /* global offsets of this subdomain's aggregates on every level: the x parts to the
     * west / the y parts to the south, each coarsened like this one (decomp.h part_of) */
    for (int lv = 0; lv <= q; lv++) {
        auto coarse = [&](int v) {
            for (int t = 0; t < lv; t++) v = (v + 1) / 2;
            return v;
        };
        int io = 0, jo = 0, off, cnt;
        for (int px = 0; px < c->sub.px; px++) {
            part_of(c->n, c->sub.npx, px, off, cnt);
            io += coarse(cnt);
        }
        for (int py = 0; py < c->sub.py; py++) {
            part_of(c->m, c->sub.npy, py, off, cnt);
            jo += coarse(cnt);
        }
        gs.mg.par[lv] = (io + jo) & 1;
    }
    for (int lv = 0; lv <= q; lv++) {
        const size_t cs = (size_t)mg_view(c, lv).cstr;
        if (gs.mg.off[lv].alloc(16 * cs) || gs.mg.diag[lv].alloc(4 * cs) || gs.mg.fac[lv].alloc(12 * cs) ||
            gs.mg.b[lv].alloc(2 * cs) || gs.mg.z[lv].alloc(2 * cs) || gs.mg.zu[lv].alloc(2 * cs))
            return IEMIC_ENOMEM;
        for (DevBuf<double>* bptr : {&gs.mg.off[lv], &gs.mg.diag[lv], &gs.mg.fac[lv], &gs.mg.b[lv], &gs.mg.z[lv],
                                     &gs.mg.zu[lv]})
            HIP_OK(hipMemsetAsync(bptr->p, 0, sizeof(double) * bptr->n, c->stream));
    }
    const size_t NC = (size_t)2 * n * m * l;
    if (gs.mg.cinv.alloc(NC * NC)) return IEMIC_ENOMEM;
    return 0;
}

/* level 0 from the compact couplings, the Galerkin chain, the z-line factors; bands: level
 * 0's of the neighbours' edge rows */
static int mg_operators(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    hipStream_t s = c->stream;
    int rc;
    {
        const TsLev V0 = mg_view(c, 0);
        hipLaunchKernelGGL(k_mg_pack0, dim3(blocks_for(c->sub.nloc)), dim3(256), 0, s, gs.sw.tsoff.p, gs.tsdiag.p,
                           lay_of(c->sub), c->sub.next, V0, gs.mg.off[0].p, gs.mg.diag[0].p);
    }
    for (int q = 1; q < gs.mg.nlev; q++) {
        TsLev F = mg_view(c, q - 1);
        const TsLev C = mg_view(c, q);
        /* the coarse operator keeps the couplings across a cut where the coarse level has a
         * halo there (x splits, intermediate levels); the coarsest stays local (its global
         * problem adds the cross couplings itself, mg_global_setup) */
        F.vis = C.hj;
        F.visi = C.hi;
        hipLaunchKernelGGL(k_mg_galerkin, dim3(blocks_for((int64_t)C.n * C.mb * C.l)), dim3(256), 0, s, F, C,
                           gs.mg.off[q].p, gs.mg.diag[q].p);
    }
    for (int q = 0; q + 1 < gs.mg.nlev; q++) {
        const TsLev V = mg_view(c, q);
        hipLaunchKernelGGL(k_mg_fac, dim3(blocks_for((int64_t)V.n * V.mb)), dim3(256), 0, s, V, gs.mg.fac[q].p);
    }
    HIP_OK(hipGetLastError());
    if (gs.mg.hr) {
        /* level 0's couplings, blocks and line factors of the neighbours' edge rows (the
         * halo-row line solves of mg_vcycle) */
        const TsLev V = mg_view(c, 0);
        const int64_t RW = (int64_t)V.n * V.l;
        const int so = c->sub.nb[2], no = c->sub.nb[3];
        std::vector<Msg> y;
        double* const arr[3] = {gs.mg.off[0].p, gs.mg.diag[0].p, gs.mg.fac[0].p};
        const int ncomp[3] = {16, 4, 12};
        for (int q = 0; q < 3; q++) {
            auto row = [&](int jl) { return Seg{arr[q], (V.hj + jl) * RW, ncomp[q], RW, V.cstr}; };
            push_pair(y, so, no, row(0), row(V.mb), row(V.mb - 1), row(-1));
        }
        if ((rc = run_msgs(c, y))) return rc;
    }
    return 0;
}

/* coarsest level, one rank (TsMg::crd): cyclic reduction over the level's longitudes */
static int mg_coarse_cr(iemic_ctx* c, int qc, int64_t ncl, int N)
{
    BlockGS& gs = c->gs;
    hipStream_t s = c->stream;
    const int l = c->l;
    int rc;
    /* cyclic reduction over the level's longitudes: blocks of one longitude, unknown
     * (jl l + k) 2 + var; the whole problem is its tail, whose explicit inverse is
     * permuted into the level's (var, cell) order for the coarse GEMV */
    SchurCR& cr = gs.mg.cr;
    const int mc = cr.m;
    const size_t mm = (size_t)mc * mc;
    HIP_OK(hipMemsetAsync(cr.dlr.p, 0, sizeof(double) * 3 * (size_t)cr.n * mm, s));
    const TsLev C = mg_view(c, qc);
    hipLaunchKernelGGL(k_mg_cr_expand, dim3(blocks_for(2 * ncl)), dim3(256), 0, s, C, mc, cr.periodic,
                       cr.dlr.p, cr.dlr.p + (size_t)cr.n * mm, cr.dlr.p + 2 * (size_t)cr.n * mm);
    if ((rc = cr_factor_blocks(c, cr))) return rc;
    if ((rc = cr_check(c, cr))) {
        set_error("block GS: singular coarsest T/S operator");
        return rc;
    }
    hipLaunchKernelGGL(k_mg_cr_perm, dim3(blocks_for((int64_t)N * N)), dim3(256), 0, s,
                       (const double*)cr.tinv.p, C, N, gs.mg.cinv.p);
    HIP_OK(hipGetLastError());
    return 0;
}

/* coarsest level of at most CR_BLOCK_MAX unknowns, one rank: its dense operator assembled and
 * inverted on the device (Gauss-Jordan with pivoting in one workgroup, cr_inv.hip) */
static int mg_coarse_dev(iemic_ctx* c, int qc, int64_t ncl, int N)
{
    BlockGS& gs = c->gs;
    hipStream_t s = c->stream;
    const int l = c->l;
    int rc;
    DevBuf<double>& A = gs.mg.cdense;
    if (A.reserve((size_t)N * N)) return IEMIC_ENOMEM;
    if (!gs.mg.cinfo.p && gs.mg.cinfo.alloc(1)) return IEMIC_ENOMEM;
    HIP_OK(hipMemsetAsync(A.p, 0, sizeof(double) * N * N, s));
    HIP_OK(hipMemsetAsync(gs.mg.cinfo.p, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_mg_coarse_dense, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, s,
                       (const double*)gs.mg.off[qc].p, (const double*)gs.mg.diag[qc].p, ncl,
                       gs.mg.n[qc], gs.mg.m[qc], l, c->cfg.periodic && c->sub.npx == 1, A.p);
    /* k_cr_inv reads column-major: it inverts A^T and writes the result column-major,
     * which is A^-1 row-major -- the layout k_gemv applies */
    if ((rc = cr_inverse_dev(s, N, A.p, gs.mg.cinv.p, gs.mg.cinfo.p))) return rc;
    int info = 0;
    if ((rc = d2h(c, &info, gs.mg.cinfo.p, sizeof(int)))) return rc;
    if (info) {
        set_error("block GS: singular coarsest T/S operator");
        return IEMIC_EINVAL;
    }
    return 0;
}

/* larger coarsest levels and the subdomains' global coarsest problem: through the host */
static int mg_coarse_host(iemic_ctx* c, int qc, int64_t ncl, int N)
{
    BlockGS& gs = c->gs;
    const int l = c->l;
    int rc;
    std::vector<double> off(16 * ncl), dg(4 * ncl);
    if ((rc = d2h(c, off.data(), gs.mg.off[qc].p, sizeof(double) * off.size()))) return rc;
    if ((rc = d2h(c, dg.data(), gs.mg.diag[qc].p, sizeof(double) * dg.size()))) return rc;
    std::vector<double> A((size_t)N * N, 0.0), X;
    const int cn = gs.mg.n[qc], cm = gs.mg.m[qc];
    const bool wrap = c->cfg.periodic && c->sub.npx == 1;
    for (int64_t t = 0; t < ncl; t++) {
        int i, jl, k;
        mg_decode(t, cn, l, i, jl, k);
        for (int R = 0; R < 2; R++) {
            double* Ar = &A[(R * ncl + t) * N];
            mg_coarse_row(R, i, jl, k, cn, cm, l, wrap, dg[(3 * R) * ncl + t], dg[(1 + R) * ncl + t],
                          &off[(8 * R) * ncl + t], ncl, [&](int ii, int jj, int kk, int var, int, double v) {
                              Ar[var * ncl + ((int64_t)jj * cn + ii) * l + kk] += v;
                          });
        }
    }
    dense_inverse(A, N, X);
    if ((rc = h2d(c, gs.mg.cinv.p, X.data(), sizeof(double) * X.size()))) return rc;
    return mg_global_setup(c, off, dg);
}

/* The entry kernel's packed operand from the set-up's Jacobian (ActiveSet::vp) and the slot
 * masks: reads nothing else, so under gs_factor's overlap it runs on the side stream with the
 * rest of this set-up.  The tiles' descriptors follow the active set (host, from its flags)
 * and are rebuilt only when that changes.  Owned rows only, whatever the decomposition: the
 * entry kernel forms no other row (a band's halo rows arrive by mg_halo2). */
static int mg_entry_pack(iemic_ctx* c)
{
    TsMg& mg = c->gs.mg;
    const ActiveSet& as = c->gs.act;
    const int nx = c->sub.nx, mb = c->sub.mb, l = c->l;
    const int tiles = (nx + MG_TI - 1) / MG_TI, nw = mg_entry_words(l), S = 2 + nw;
    int rc;
    if (mg.egen != as.gen || !mg.etl.p) {
        std::vector<uint64_t> d((size_t)tiles * mb * S, 0);
        int64_t base = 0;
        for (int jl = 0; jl < mb; jl++)
            for (int ti = 0; ti < tiles; ti++) {
                uint64_t* e = &d[((size_t)jl * tiles + ti) * S];
                int64_t na = 0;
                for (int k = 0; k < l; k++)
                    for (int ii = 0; ii < MG_TI && ti * MG_TI + ii < nx; ii++)
                        if (as.act_h[((size_t)jl * l + k) * nx + ti * MG_TI + ii]) {
                            const int q = k * MG_TI + ii;
                            e[2 + (q >> 6)] |= (uint64_t)1 << (q & 63);
                            na++;
                        }
                e[0] = (uint64_t)base;
                e[1] = (uint64_t)na;
                base += (2 * MG_NE * na + 15) / 16 * 16;
            }
        if (mg.etl.reserve(d.size() + 1) || mg.ep.reserve((size_t)base + 16)) return IEMIC_ENOMEM;
        if ((rc = h2d(c, mg.etl.p, d.data(), sizeof(uint64_t) * d.size()))) return rc;
        mg.epn = base;
        mg.egen = as.gen;
    }
    const int64_t nt = (int64_t)tiles * mb * MG_TI * l;
    hipLaunchKernelGGL(k_mg_entry_pack, dim3(blocks_for(nt)), dim3(256), 0, c->stream, c->gs.act.vp,
                       (const uint64_t*)c->gs.kmask.p, (const uint64_t*)mg.etl.p, nw, lay_of(c->sub), nt, mg.ep.p);
    HIP_OK(hipGetLastError());
    return 0;
}

/* levels, Galerkin operators, z-line factors and the coarsest inverse (once per Jacobian) */
int ts_mg_setup(iemic_ctx* c, int sweeps)
{
    BlockGS& gs = c->gs;
    int rc;
    gs.mg.sweeps = sweeps;
    if (gs.ts_mg <= 0) return 0;
    if (c->l > 64) {             /* the z-line smoother runs one lane per level */
        gs.ts_mg = 0;
        return 0;
    }
    /* latitude bands: level 0's halo rows (hr, mg_levels) follow the sweep count, which a live
     * context may change between set-ups; the levels are then laid out again.  One rank: hr
     * is 0 whatever the sweeps, so nothing changes there */
    if (gs.mg.nlev && gs.mg.hr != (c->sub.npy > 1 && c->sub.npx == 1 && std::max(1, sweeps) == 1)) gs.mg.nlev = 0;
    if (gs.mg.nlev == 0) {
        if ((rc = mg_levels(c))) return rc;
        if (gs.ts_mg == 0) return 0;
    }
    if ((rc = mg_entry_pack(c))) return rc;
    if ((rc = mg_operators(c))) return rc;
    const int qc = gs.mg.nlev - 1;
    const int64_t ncl = (int64_t)gs.mg.n[qc] * gs.mg.m[qc] * c->l;
    const int N = (int)(2 * ncl);
    gs.mg.ckind = gs.mg.crd ? 1 : (N <= CR_BLOCK_MAX && c->sub.nranks <= 1) ? 0 : 2;
    if (gs.mg.ckind == 1) return mg_coarse_cr(c, qc, ncl, N);
    if (gs.mg.ckind == 0) return mg_coarse_dev(c, qc, ncl, N);
    return mg_coarse_host(c, qc, ncl, N);
}

}  // namespace iemic
