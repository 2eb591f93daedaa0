/*
 * active_set.hip -- the compressed active-cell set of the block Gauss-Seidel set-up and the
 * coefficient streams packed from the Jacobian (BlockGS::act): what FGMRES's compressed
 * basis, the compressed SpMV and the dynamics defect (krylov.hip, spmv.hip) read.
 */
#include <algorithm>
#include <vector>

#include "gs_internal.h"

namespace iemic {

namespace {

/* 1 per owned cell (owned index lc) with a non-identity row */
__global__ void k_cell_active(const uint8_t* __restrict__ known, Lay L, uint8_t* __restrict__ act)
{
    OWNED_CELL;
    bool a = false;
#pragma unroll
    for (int r = 0; r < NUN; r++) a |= !known[NUN * cell + r];
    act[lc] = a ? 1 : 0;
}

}  // namespace

/* dvb[(h / 64) 4096 + s 64 + h % 64] = val[s nloc + act[h]] (0 past the last active cell) */
__global__ void k_dyn_pack(const double* __restrict__ val, const int* __restrict__ act, int64_t nact,
                           int64_t nloc, double* __restrict__ dvb, int64_t n)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t blk = t >> 12, s = (t >> 6) & 63, l = t & 63, h = blk * 64 + l;
    dvb[t] = h < nact ? val[s * nloc + act[h]] : 0.0;
}

/* the compressed SpMV's stream (spmv.hip k_spmv7c): the active cells of tile pos (a0 ..
 * a0 + na - 1) hold one contiguous run spc[104 a0 ..), slot s of active cell a at
 * 104 a0 + s na + (a - a0) */
__global__ void k_spmv_pack(const double* __restrict__ val, const int* __restrict__ act,
                                const int* __restrict__ apos, const int4* __restrict__ atl, int64_t nact,
                                int64_t nloc, double* __restrict__ spc)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)NSLOT * nact) return;
    const int64_t s = t / nact, a = t - s * nact;
    const int4 td = atl[2 * apos[a]];
    spc[(int64_t)NSLOT * td.z + s * td.w + (a - td.z)] = val[s * nloc + act[a]];
}

/* gs_refresh: *nd += 1 for every owned row whose identity flag (k_known's rule) in the
 * current Jacobian differs from the set-up's */
__global__ void k_known_diff(const double* __restrict__ val, Lay L, int64_t rowintcon,
                             const uint8_t* __restrict__ known, double* __restrict__ nd)
{
    OWNED_CELL;
    int diff = 0;
    for (int r = 0; r < NUN; r++) {
        bool id = val[(int64_t)ROW_BEGIN[r] * ncell + lc] == 1.0;
        for (int s = ROW_BEGIN[r] + 1; id && s < ROW_BEGIN[r + 1]; s++)
            id = val[(int64_t)s * ncell + lc] == 0.0;
        const uint8_t k = (id && NUN * cell + r != rowintcon) ? 1 : 0;
        diff += k != known[NUN * cell + r];
    }
    if (diff) atomicAdd(nd, (double)diff);
}

/* the compressed SpMV's tiles (k_spmv7c): 64 cells along i of one grid row, those holding
 * an active cell: tile, first | last active lane << 8, the first active cell a0, the active
 * cells na, the 64-bit active-lane mask (8 ints each); apos: per active cell its tile */
static int act_tiles(iemic_ctx* c, const std::vector<uint8_t>& h, const std::vector<int>& cm)
{
    ActiveSet& as = c->gs.act;
    int rc;
    const int nx = c->sub.nx, tpr = (nx + 63) / 64;
    const int64_t nrow = c->sub.nloc / nx;
    std::vector<int> tl, ap((size_t)as.nact, 0);
    for (int64_t row = 0; row < nrow; row++)
        for (int ti = 0; ti < tpr; ti++) {
            const int i0 = ti * 64, nc = std::min(64, nx - i0);
            int lo = -1, hi = -1;
            uint64_t mask = 0;
            for (int cc = 0; cc < nc; cc++)
                if (h[row * nx + i0 + cc]) {
                    if (lo < 0) lo = cc;
                    hi = cc;
                    mask |= (uint64_t)1 << cc;
                }
            if (lo < 0) continue;
            const int a0 = cm[row * nx + i0 + lo], na = cm[row * nx + i0 + hi] - a0 + 1;
            for (int a = a0; a < a0 + na; a++) ap[a] = (int)(tl.size() / 8);
            tl.insert(tl.end(), {(int)(row * tpr + ti), lo | (hi << 8), a0, na, (int)(uint32_t)mask,
                                 (int)(uint32_t)(mask >> 32), 0, 0});
        }
    as.natile = (int)(tl.size() / 8);
    if (as.atl.reserve(tl.size() + 8)) return IEMIC_ENOMEM;
    if (!tl.empty() && (rc = h2d(c, as.atl.p, tl.data(), sizeof(int) * tl.size()))) return rc;
    if (as.apos.reserve(ap.size() + 1)) return IEMIC_ENOMEM;
    if (!ap.empty() && (rc = h2d(c, as.apos.p, ap.data(), sizeof(int) * ap.size()))) return rc;
    return 0;
}

/* the active-cell list of the compressed Arnoldi basis from the identity-row flags
 * (BlockGS::known), with cmap, ric and the tiles; rebuilt when the flags change (*changed) */
int act_build(iemic_ctx* c, bool* changed)
{
    BlockGS& gs = c->gs;
    ActiveSet& as = gs.act;
    int rc;
    *changed = false;
    if (as.actf.reserve(c->sub.nloc)) return IEMIC_ENOMEM;
    hipLaunchKernelGGL(k_cell_active, dim3(blocks_for(c->sub.nloc)), dim3(256), 0, c->stream, gs.known.p,
                       lay_of(c->sub), as.actf.p);
    std::vector<uint8_t> h((size_t)c->sub.nloc);
    if ((rc = d2h(c, h.data(), as.actf.p, h.size()))) return rc;
    if (h == as.act_h) return 0;
    std::vector<int> list;
    list.reserve(h.size());
    for (int64_t q = 0; q < c->sub.nloc; q++)
        if (h[q]) list.push_back((int)q);
    as.nact = (int64_t)list.size();
    if (as.act.reserve(list.size() + 1)) return IEMIC_ENOMEM;
    if (!list.empty() && (rc = h2d(c, as.act.p, list.data(), sizeof(int) * list.size()))) return rc;
    std::vector<int> cm((size_t)c->sub.nloc, -1);
    for (size_t q = 0; q < list.size(); q++) cm[list[q]] = (int)q;
    if (as.cmap.reserve(cm.size())) return IEMIC_ENOMEM;
    if ((rc = h2d(c, as.cmap.p, cm.data(), sizeof(int) * cm.size()))) return rc;
    as.ric = -1;
    if (c->rowintcon >= 0) {
        const int64_t cell = c->rowintcon / NUN - c->sub.own0;
        if (cell >= 0 && cell < c->sub.nloc && cm[cell] >= 0) as.ric = (int64_t)NUN * cm[cell] + c->rowintcon % NUN;
    }
    if ((rc = act_tiles(c, h, cm))) return rc;
    as.act_h.swap(h);
    as.gen++;
    *changed = true;
    return 0;
}

/* latitude bands: the U/V/W/P rows' coefficients (slots 0 .. 63) of the two halo rows, from
 * the neighbour bands' first / last owned row (ActiveSet::dvh: slot-major, the south row's
 * cells, then the north row's) */
static int dyn_halo_coefs(iemic_ctx* c)
{
    ActiveSet& as = c->gs.act;
    const int64_t row = (int64_t)c->l * c->sub.nx, nloc = c->sub.nloc;
    constexpr int NDS = 64;
    if (as.dvh.n < (size_t)(NDS * 2 * row)) {
        if (as.dvh.alloc((size_t)(NDS * 2 * row))) return IEMIC_ENOMEM;
        HIP_OK(hipMemsetAsync(as.dvh.p, 0, sizeof(double) * as.dvh.n, c->stream));
    }
    double* v = c->d_val.p;
    const int so = c->sub.nb[2], no = c->sub.nb[3];
    std::vector<Msg> y;
    push_pair(y, so, no, Seg{v, 0, NDS, row, nloc}, Seg{as.dvh.p, row, NDS, row, 2 * row},
              Seg{v, nloc - row, NDS, row, nloc}, Seg{as.dvh.p, 0, NDS, row, 2 * row});
    return run_msgs(c, y);
}

/* the defect's coefficient stream: the active cells' 64 U/V/W/P slots, blocked per 64 active
 * cells, so a workgroup reads one contiguous 32 KB run and no land lines */
static int act_pack_dvb(iemic_ctx* c)
{
    ActiveSet& as = c->gs.act;
    if (as.nact <= 0 || !as.act.p) return 0;
    const int64_t nb = (as.nact + 63) / 64;
    if (as.dvb.reserve((size_t)(nb * 64 * 64))) return IEMIC_ENOMEM;
    hipLaunchKernelGGL(k_dyn_pack, dim3(blocks_for(nb * 64 * 64)), dim3(256), 0, c->stream, c->d_val.p,
                       (const int*)as.act.p, as.nact, c->sub.nloc, as.dvb.p, nb * 64 * 64);
    HIP_OK(hipGetLastError());
    return 0;
}

/* The compressed SpMV's coefficient stream (k_spmv7c): the active cells' 104 slots of the
 * current Jacobian, packed at every set-up and by gs_refresh after every later Jacobian */
static int gs_pack_spc(iemic_ctx* c)
{
    ActiveSet& as = c->gs.act;
    if (as.nact <= 0 || !as.act.p) return 0;
    if (as.spc.reserve((size_t)(NSLOT * as.nact))) return IEMIC_ENOMEM;
    hipLaunchKernelGGL(k_spmv_pack, dim3(blocks_for(NSLOT * as.nact)), dim3(256), 0, c->stream, c->d_val.p,
                       (const int*)as.act.p, (const int*)as.apos.p, (const int4*)as.atl.p, as.nact, c->sub.nloc,
                       as.spc.p);
    HIP_OK(hipGetLastError());
    return 0;
}

/* set-up: every stream packed from the Jacobian just assembled, which the apply reads from
 * now on (a later one is assembled into the other buffer) */
int act_pack_streams(iemic_ctx* c)
{
    ActiveSet& as = c->gs.act;
    int rc;
    if (c->sub.nranks > 1 && c->sub.npx == 1 && (rc = dyn_halo_coefs(c))) return rc;
    if ((rc = act_pack_dvb(c))) return rc;
    if ((rc = gs_pack_spc(c))) return rc;
    as.vp = c->d_val.p;
    as.coef_stale = 0;
    as.cmp_ok = 1;
    return 0;
}

/* A Jacobian assembled while the block GS is set up (Ocean::solve reuses the preconditioner
 * until preProcess flags a rebuild, Ocean.C:790-801, 1360-1374).  The preconditioner stays the
 * operator of the set-up Jacobian, as TRIOS::BlockPreconditioner's extracted blocks do: the
 * assembly wrote into the second Jacobian buffer (assemble_jacobian) and the apply reads the
 * set-up one through ActiveSet::vp, together with the copies made from it (gslot, dvh, dvb).
 * What follows the new Jacobian: the compressed SpMV's stream, and whether the set-up's land
 * cells are still identity rows (else the compressed basis would drop live rows: summed over
 * the ranks, so every rank takes the same branch). */
int gs_refresh(iemic_ctx* c)
{
    BlockGS& gs = c->gs;
    ActiveSet& as = gs.act;
    if (!as.coef_stale || !gs.ready || gs.kind != 2) return 0;
    as.coef_stale = 0;
    if (as.chk.reserve(1)) return IEMIC_ENOMEM;
    HIP_OK(hipMemsetAsync(as.chk.p, 0, sizeof(double), c->stream));
    hipLaunchKernelGGL(k_known_diff, dim3((unsigned)((c->sub.nloc + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_val.p, lay_of(c->sub), (int64_t)c->rowintcon, gs.known.p, as.chk.p);
    int rc = allreduce_sum(c, as.chk.p, 1);
    if (rc) return rc;
    double nd = 0.0;
    if ((rc = d2h(c, &nd, as.chk.p, sizeof(double)))) return rc;
    if (nd != 0.0) as.cmp_ok = 0;
    return gs_pack_spc(c);
}

}  // namespace iemic
