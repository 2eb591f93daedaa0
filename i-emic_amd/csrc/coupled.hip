/*
 * coupled.hip -- the coupled ocean + atmosphere block system on the device (SURVEY.md §8f
 * row 2, BASELINE config C4): its operator and preconditioner.
 *
 *   CoupledModel (src/coupledmodel/CoupledModel.C) with CouplingBlock (CouplingBlock.H)
 *     -> iemic_coupled_*: synchronize (218-233), computeRHS / computeJacobian (236-271),
 *     applyMatrix (436-470) and the forward block Gauss-Seidel applyPrecon 'F' (544-585);
 *     the solve (274-432) is coupled_krylov.hip, the atmosphere atmos.hip
 *   Ocean::getBlock(atmos) (Ocean.C:1538-1667), Atmosphere::getBlock(ocean)
 *     (Atmosphere.C:502-613) -> the coupling kernels below (applied matrix-free)
 *
 * The coupled Krylov vectors are packed [ocean owned rows | atmosphere]; one process (the
 * coupled grid is small: 4 degrees).
 */
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "stencil.h"
#include "coupled_internal.h"
#include "vec_kernels.h"

using namespace iemic;

namespace iemic {
namespace {

/* ---- coupling (applied matrix-free) -------------------------------------------------- */
struct CplPar {
    int n, m, l;
    int ib0, jb0, nx, mb;  /* the ocean subdomain's owned columns / rows (Decomp2D)  */
    int64_t own0;          /* first owned ext cell of the ocean                    */
    double dTFQ;           /* nuq tdim/qdim dqso (1 - M)  (Atmosphere.C:547)        */
    double pfac;           /* (1/A)(tdim/qdim) dqso        (Atmosphere.C:596-597)   */
    double Ooa, aft, dqft; /* Ocean.C:1613-1627: Ooa, -comb sunp albed, lvsc eta qdim */
    int ct, cs;            /* coupled_T, coupled_S                                  */
    double nus;            /* Ocean.C:1639-1651: -dQFS = nus, -dPFS = nus Pd        */
    int64_t sint_row;      /* packed row of the ocean's integral condition, or -1   */
};

/* SST of the ocean state: T at (i, j, l-1) (Ocean::interfaceT -> Atmosphere::synchronize),
 * the subdomain's owned surface cells into the n*m surface (the other entries untouched:
 * on several ranks zeroed before and summed after) */
__global__ void k_sst(CplPar K, const double* __restrict__ xo_ext, double* __restrict__ sst)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K.nx * K.mb) return;
    const int il = e % K.nx, jl = e / K.nx;
    const int64_t cell = ((int64_t)(jl + HALO) * K.l + (K.l - 1)) * K.nx + il;
    sst[(int64_t)(K.jb0 + jl) * K.n + K.ib0 + il] = xo_ext[NUN * cell + TT];
}
/* surface T of a packed ocean vector (owned rows) into the n*m surface, owned cells */
__global__ void k_surf_t(CplPar K, const double* __restrict__ xo_packed, double* __restrict__ out)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K.nx * K.mb) return;
    const int il = e % K.nx, jl = e / K.nx;
    const int64_t lc = ((int64_t)jl * K.l + (K.l - 1)) * K.nx + il;
    out[(int64_t)(K.jb0 + jl) * K.n + K.ib0 + il] = xo_packed[NUN * lc + TT];
}
/* Atmosphere::interfaceT/Q/A/P (449-493, getP 1160-1225): the surface fields the ocean
 * needs; P dimensional, Pdist (Eo0 + eta qdim P) over water */
__global__ void k_atm_fields(AtmPar P, AtmGeo G, const double* __restrict__ xa, double* __restrict__ out, int nm)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nm) return;
    out[q] = xa[ANUN * q + AT];
    out[nm + q] = xa[ANUN * q + AQ];
    out[2 * nm + q] = xa[ANUN * q + AA];
    out[3 * nm + q] = G.surf[q] == 0 ? G.pdist[q] * (P.Eo0 + P.eta * P.qdim * xa[G.rowP]) : 0.0;
}

/* y_o(surface T rows) += C_oa x_a  (Ocean::getBlock(atmos): -dTFT, -dAFT, -dQFT; with
 * coupled_S the surface S rows: -dQFS, -dPFS) */
__global__ void k_cpl_oa(CplPar K, const int* __restrict__ surf, const double* __restrict__ suno,
                         const double* __restrict__ pdist, int rowP, const double* __restrict__ xa,
                         double* __restrict__ yo_packed)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= K.nx * K.mb) return;
    const int il = e % K.nx, jl = e / K.nx, j = K.jb0 + jl;
    const int q = j * K.n + K.ib0 + il;
    if (surf[q]) return;
    const int64_t lc = ((int64_t)jl * K.l + (K.l - 1)) * K.nx + il;   /* owned-local cell */
    const double S = suno[j + 1];
    const double dTFT = K.Ooa * (1.0 - 0.0);
    const double dAFT = K.aft * S * (1.0 - 0.0);
    const double dQFT = K.dqft * (1.0 - 0.0);
    if (K.ct) {
        double z = 0.0;
        z += -dTFT * xa[ANUN * q + AT];
        z += -dAFT * xa[ANUN * q + AA];
        z += -dQFT * xa[ANUN * q + AQ];
        yo_packed[NUN * lc + TT] += z;
    }
    if (K.cs && NUN * lc + SS != K.sint_row) {
        const double dQFS = -K.nus * (1.0 - 0.0);
        const double dPFS = -K.nus * pdist[q] * (1.0 - 0.0);
        double z = 0.0;
        z += -dQFS * xa[ANUN * q + AQ];
        z += -dPFS * xa[rowP];
        yo_packed[NUN * lc + SS] += z;
    }
}
/* surface T of cell q: from the gathered n*m surface (several ranks) or straight from the
 * packed ocean vector (one rank) */
__device__ __forceinline__ double surf_t(const CplPar& K, const double* __restrict__ tsurf,
                                         const double* __restrict__ xo_packed, int q)
{
    if (tsurf) return tsurf[q];
    const int i = q % K.n, j = q / K.n;
    return xo_packed[NUN * (((int64_t)j * K.l + (K.l - 1)) * K.n + i) + TT];
}
/* y_a += C_ao x_o on the T and q rows (Atmosphere::getBlock(ocean)) */
__global__ void k_cpl_ao(CplPar K, AtmGeo G, const double* __restrict__ tsurf, const double* __restrict__ xo_packed,
                         double* __restrict__ ya)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= K.n * K.m) return;
    if (G.surf[q]) return;
    const double t = surf_t(K, tsurf, xo_packed, q);
    if (ANUN * q + AT != G.rowint) ya[ANUN * q + AT] += (1.0 - 0.0) * t;
    if (ANUN * q + AQ != G.rowint) ya[ANUN * q + AQ] += K.dTFQ * t;
}
/* partials of sum_q intc_q T_o(q) (the precipitation row's SST dependence) */
__global__ void __launch_bounds__(256) k_cpl_pdot(CplPar K, const double* __restrict__ pint,
                                                  const double* __restrict__ tsurf,
                                                  const double* __restrict__ xo_packed, double* __restrict__ part)
{
    __shared__ double sm[256];
    double s = 0.0;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < K.n * K.m; q += gridDim.x * blockDim.x)
        s += pint[q] * surf_t(K, tsurf, xo_packed, q);
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) sm[threadIdx.x] += sm[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sm[0];
}
__global__ void k_cpl_pfin(CplPar K, AtmGeo G, const double* __restrict__ part, double* __restrict__ ya, double sgn)
{
    if (threadIdx.x || blockIdx.x) return;
    double a = 0.0;
    for (int q = 0; q < AR_BLOCKS; q++) a += part[q];
    ya[G.rowP] += sgn * K.pfac * a;
}

}  // namespace
}  // namespace iemic

/* =========================== coupled model ============================================ */
namespace {
CplPar cpl_par(const iemic_coupled* cm)
{
    const iemic_ctx* oc = cm->oc;
    const iemic_atmos* a = cm->at;
    const host::Setup& su = oc->su;
    CplPar K{};
    K.n = oc->n; K.m = oc->m; K.l = oc->l;
    K.ib0 = oc->sub.ib0; K.jb0 = oc->sub.jb0; K.nx = oc->sub.nx; K.mb = oc->sub.mb;
    K.own0 = oc->sub.own0;
    const AtmPar& P = a->P;
    K.dTFQ = P.nuq * P.tdim / P.qdim * P.dqso * (1.0 - 0.0);
    K.pfac = (1.0 / P.total_area) * (P.tdim / P.qdim) * P.dqso * (1.0 - 0.0);
    K.Ooa = su.Ooa;
    K.aft = -su.par[P_COMB] * su.par[P_SUNP] * P.da;
    K.dqft = su.lvsc * su.eta_a * su.qdim_a;
    K.ct = oc->cfg.coupled_t;
    K.cs = oc->cfg.coupled_s;
    K.nus = su.nus;
    K.sint_row = oc->rowintcon >= 0 ? oc->rowintcon - NUN * oc->sub.own0 : -1;
    return K;
}

/* CoupledModel::synchronize (218-233): ocean <- atmosphere fields + CommPars
 * (Ocean::synchronize(atmos)), atmosphere <- SST (Atmosphere::synchronize(ocean)) */
int cpl_sync(iemic_coupled* cm)
{
    iemic_ctx* oc = cm->oc;
    iemic_atmos* a = cm->at;
    const int nm = a->n * a->m;
    hipStream_t s = oc->stream;
    hipLaunchKernelGGL(k_atm_fields, dim3((nm + 255) / 256), dim3(256), 0, s, a->P, atm_geo(a), (const double*)a->d_x.p,
                       oc->d_atm.p, nm);
    double pars[18];
    iemic_atmos_commpars(a, pars);
    /* the ocean Jacobian depends on the CommPars only through lin's latent-heat term */
    if (!cm->synced || !std::equal(pars, pars + 18, cm->pars)) oc->jac_valid = 0;
    std::copy(pars, pars + 18, cm->pars);
    cm->synced = 1;
    oc->su.set_atmos(pars);
    int rc = compute_forcing(oc);
    if (rc) return rc;
    /* the atmosphere (replicated on every rank) sees the whole surface: each rank writes its
     * owned cells, the sum over the ranks fills the rest */
    if (oc->sub.nranks > 1) HIP_OK(hipMemsetAsync(a->d_sst.p, 0, sizeof(double) * nm, s));
    hipLaunchKernelGGL(k_sst, dim3((nm + 255) / 256), dim3(256), 0, s, cpl_par(cm), (const double*)oc->d_x.p,
                       a->d_sst.p);
    HIP_OK(hipGetLastError());
    if (oc->sub.nranks > 1 && (rc = allreduce_sum(oc, a->d_sst.p, nm))) return rc;
    return 0;
}

/* the surface T of a packed ocean vector for the atmosphere rows: null on one rank (the
 * coupling kernels read the vector), else the n*m surface summed over the ranks */
int cpl_surf(iemic_coupled* cm, const double* xo_packed, const double** tsurf)
{
    iemic_ctx* oc = cm->oc;
    *tsurf = nullptr;
    if (oc->sub.nranks <= 1) return 0;
    const int nm = oc->n * oc->m;
    hipStream_t s = oc->stream;
    double* t = cm->tsurf.p;
    HIP_OK(hipMemsetAsync(t, 0, sizeof(double) * nm, s));
    hipLaunchKernelGGL(k_surf_t, dim3((nm + 255) / 256), dim3(256), 0, s, cpl_par(cm), xo_packed, t);
    HIP_OK(hipGetLastError());
    int rc = allreduce_sum(oc, t, nm);
    if (rc) return rc;
    *tsurf = t;
    return 0;
}
}  // namespace

namespace iemic {
/* y = [J_o C_oa; C_ao J_a] x on packed vectors [ocean owned rows | atmosphere] */
int cpl_apply(iemic_coupled* cm, const double* x, double* y)
{
    iemic_ctx* oc = cm->oc;
    iemic_atmos* a = cm->at;
    hipStream_t s = oc->stream;
    const int64_t o = NUN * oc->sub.own0, NL = cm->NL;
    const int nm = a->n * a->m;
    const CplPar K = cpl_par(cm);
    HIP_OK(hipMemcpyAsync(cm->xo.p + o, x, sizeof(double) * NL, hipMemcpyDeviceToDevice, s));
    int rc = spmv(oc, cm->xo.p, cm->yo.p, s);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(y, cm->yo.p + o, sizeof(double) * NL, hipMemcpyDeviceToDevice, s));
    if ((rc = atm_spmv_dev(a, x + NL, y + NL))) return rc;
    hipLaunchKernelGGL(k_cpl_oa, dim3((nm + 255) / 256), dim3(256), 0, s, K, (const int*)a->d_surf.p,
                       (const double*)(oc->d_tab.p + 9 * (oc->m + 2) + 2 * (oc->l + 2)), (const double*)a->d_pdist.p,
                       a->rowP, x + NL, y);
    const double* ts = nullptr;
    if ((rc = cpl_surf(cm, x, &ts))) return rc;
    hipLaunchKernelGGL(k_cpl_ao, dim3((nm + 255) / 256), dim3(256), 0, s, K, atm_geo(a), ts, x, y + NL);
    hipLaunchKernelGGL(k_cpl_pdot, dim3(AR_BLOCKS), dim3(256), 0, s, K, (const double*)a->d_pint.p, ts, x,
                       a->d_red.p + 3 * AR_BLOCKS);
    hipLaunchKernelGGL(k_cpl_pfin, dim3(1), dim3(64), 0, s, K, atm_geo(a), (const double*)a->d_red.p + 3 * AR_BLOCKS,
                       y + NL, 1.0);
    HIP_OK(hipGetLastError());
    return 0;
}

/* forward block Gauss-Seidel (CoupledModel.C:544-585, 'F'): z_o = M_o^-1 r_o;
 * z_a = M_a^-1 (r_a - C_ao z_o) */
int cpl_prec(iemic_coupled* cm, const double* r, double* z, int use_prec)
{
    iemic_ctx* oc = cm->oc;
    iemic_atmos* a = cm->at;
    hipStream_t s = oc->stream;
    const int64_t o = NUN * oc->sub.own0, NL = cm->NL, NA = cm->NA;
    const int nm = a->n * a->m;
    if (!use_prec) {
        HIP_OK(hipMemcpyAsync(z, r, sizeof(double) * (NL + NA), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    HIP_OK(hipMemcpyAsync(cm->ro.p + o, r, sizeof(double) * NL, hipMemcpyDeviceToDevice, s));
    int rc = prec_apply(oc, cm->ro.p, cm->zo.p);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(z, cm->zo.p + o, sizeof(double) * NL, hipMemcpyDeviceToDevice, s));
    /* b_a = r_a - C_ao z_o */
    double* b = cm->tmpa.p;
    HIP_OK(hipMemsetAsync(b, 0, sizeof(double) * NA, s));
    const CplPar K = cpl_par(cm);
    const double* ts = nullptr;
    if ((rc = cpl_surf(cm, z, &ts))) return rc;
    hipLaunchKernelGGL(k_cpl_ao, dim3((nm + 255) / 256), dim3(256), 0, s, K, atm_geo(a), ts, (const double*)z, b);
    hipLaunchKernelGGL(k_cpl_pdot, dim3(AR_BLOCKS), dim3(256), 0, s, K, (const double*)a->d_pint.p, ts,
                       (const double*)z, a->d_red.p + 3 * AR_BLOCKS);
    hipLaunchKernelGGL(k_cpl_pfin, dim3(1), dim3(64), 0, s, K, atm_geo(a), (const double*)a->d_red.p + 3 * AR_BLOCKS,
                       b, 1.0);
    hipLaunchKernelGGL(k_axpby, dim3(blocks_for(NA)), dim3(256), 0, s, 1.0, r + NL, -1.0, (const double*)b, b, NA);
    if ((rc = atm_prec_apply(a, b, z + NL))) return rc;
    HIP_OK(hipGetLastError());
    return 0;
}

void pack_host(const iemic_coupled* cm, const double* ref_vec, std::vector<double>& packed)
{
    const iemic_ctx* oc = cm->oc;
    const int64_t NL = cm->NL, NA = cm->NA, o = NUN * oc->sub.own0;
    std::vector<double> ext((size_t)oc->sub.nerows(), 0.0);
    oc->su.ref_to_ext(ref_vec, ext.data());
    packed.resize((size_t)(NL + NA));
    std::copy(ext.begin() + o, ext.begin() + o + NL, packed.begin());
    std::copy(ref_vec + oc->nrows, ref_vec + oc->nrows + NA, packed.begin() + NL);
}

void unpack_host(const iemic_coupled* cm, const std::vector<double>& packed, double* ref_vec)
{
    const iemic_ctx* oc = cm->oc;
    const int64_t NL = cm->NL, o = NUN * oc->sub.own0;
    std::vector<double> ext((size_t)oc->sub.nerows(), 0.0);
    std::copy(packed.begin(), packed.begin() + NL, ext.begin() + o);
    oc->su.ext_to_ref(ext.data(), ref_vec);
    std::copy(packed.begin() + NL, packed.end(), ref_vec + oc->nrows);
}
}  // namespace iemic

extern "C" int iemic_coupled_create(iemic_coupled** out, iemic_ctx* oc, iemic_atmos* a)
{
    if (!out || !oc || !a || a->oc != oc) return IEMIC_EINVAL;
    int rc = coupled_check(oc);
    if (rc) return rc;
    if (hipSetDevice(oc->device) != hipSuccess) return IEMIC_EDEVICE;
    iemic_coupled* cm = new iemic_coupled();
    cm->oc = oc;
    cm->at = a;
    cm->NL = oc->sub.nlrows();
    cm->NA = a->dim;
    cm->NC = cm->NL + cm->NA;
    const int64_t NE = oc->sub.nerows();
    rc = 0;
    rc |= cm->xo.alloc(NE);
    rc |= cm->yo.alloc(NE);
    rc |= cm->ro.alloc(NE);
    rc |= cm->zo.alloc(NE);
    rc |= cm->tmpa.alloc(cm->NA);
    rc |= cm->tsurf.alloc((size_t)oc->n * oc->m);
    rc |= cm->w.alloc(cm->NC);
    rc |= cm->r.alloc(cm->NC);
    rc |= cm->part.alloc((size_t)KB * (MAX_KRYLOV + 2));
    rc |= cm->hb.alloc((size_t)2 * MAX_KRYLOV + 8);
    rc |= cm->hc.alloc((size_t)2 * (2 * MAX_KRYLOV + 8));
    for (hipEvent_t& e : cm->ev)
        if (!rc && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) rc = 1;
    if (!rc && hipHostMalloc(&cm->h_red, sizeof(double) * 2 * (2 * MAX_KRYLOV + 8)) != hipSuccess) rc = 1;
    if (rc) {
        delete cm;
        set_error("iemic_coupled_create: out of device memory");
        return IEMIC_ENOMEM;
    }
    for (DevBuf<double>* b : {&cm->xo, &cm->yo, &cm->ro, &cm->zo})
        (void)hipMemsetAsync(b->p, 0, sizeof(double) * b->n, oc->stream);
    (void)hipStreamSynchronize(oc->stream);
    oc->refs++;
    a->refs++;
    *out = cm;
    return 0;
}

extern "C" void iemic_coupled_destroy(iemic_coupled* cm)
{
    if (!cm) return;
    iemic_ctx* oc = cm->oc;
    iemic_atmos* a = cm->at;
    (void)hipSetDevice(oc->device);
    (void)hipStreamSynchronize(oc->stream);
    delete cm;
    atmos_release(a);
    ctx_release(oc);
}

extern "C" int iemic_coupled_synchronize(iemic_coupled* cm)
{
    if (!cm) return IEMIC_EINVAL;
    if (hipSetDevice(cm->oc->device) != hipSuccess) return IEMIC_EDEVICE;
    int rc = cpl_sync(cm);
    if (rc) return rc;
    DEV_SYNC(cm->oc);
    return 0;
}

/* CoupledModel::computeRHS (260-271): synchronize, then each model's F (device copies
 * stay in the contexts; host copies if pointers are given: ocean in reference order) */
extern "C" int iemic_coupled_rhs(iemic_coupled* cm, double* F_ocean, double* F_atmos)
{
    if (!cm) return IEMIC_EINVAL;
    int rc = iemic_coupled_synchronize(cm);
    if (!rc) rc = iemic_rhs(cm->oc, F_ocean);
    if (!rc) rc = iemic_atmos_rhs(cm->at, F_atmos);
    return rc;
}

/* CoupledModel::computeJacobian (236-257): synchronize, each model's Jacobian; the
 * coupling blocks are applied matrix-free from the synchronized parameters */
extern "C" int iemic_coupled_jacobian(iemic_coupled* cm)
{
    if (!cm) return IEMIC_EINVAL;
    int rc = iemic_coupled_synchronize(cm);
    if (!rc) rc = iemic_jacobian(cm->oc);
    if (!rc) rc = iemic_atmos_jacobian(cm->at);
    return rc;
}

/* CoupledModel::applyMatrix (436-470) on host vectors [ocean (reference order) | atmosphere] */
extern "C" int iemic_coupled_spmv(iemic_coupled* cm, const double* x, double* y)
{
    if (!cm || !x || !y) return IEMIC_EINVAL;
    iemic_ctx* oc = cm->oc;
    if (hipSetDevice(oc->device) != hipSuccess) return IEMIC_EDEVICE;
    if (!oc->jac_valid || !cm->at->jac_valid) {
        set_error("iemic_coupled_spmv: no Jacobian assembled");
        return IEMIC_ESTATE;
    }
    const int64_t NL = cm->NL, NA = cm->NA;
    std::vector<double> packed;
    pack_host(cm, x, packed);
    DevBuf<double> dx, dy;
    if (dx.alloc(NL + NA) || dy.alloc(NL + NA)) return IEMIC_ENOMEM;
    int rc = h2d(oc, dx.p, packed.data(), sizeof(double) * (NL + NA));
    if (!rc) rc = cpl_apply(cm, dx.p, dy.p);
    if (!rc) rc = d2h(oc, packed.data(), dy.p, sizeof(double) * (NL + NA));
    if (rc) return rc;
    unpack_host(cm, packed, y);
    return 0;
}

