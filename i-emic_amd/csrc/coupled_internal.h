/*
 * coupled_internal.h -- what the units of the coupled ocean + atmosphere model share
 * (atmos.hip, coupled.hip, coupled_krylov.hip): the two handles behind iemic_atmos_* and
 * iemic_coupled_*, the atmosphere's parameter blocks as its kernels take them, and the
 * functions that cross the three files.  All three units are built without floating-point
 * contraction.  Included by nothing else.
 */
#ifndef IEMIC_COUPLED_INTERNAL_H
#define IEMIC_COUPLED_INTERNAL_H

#include <algorithm>
#include <vector>

#include "common.h"
#include "stencil.h"

namespace iemic {
/* atmosphere unknowns per surface cell (T, q, A), ELL slots per row, blocks of its reductions */
constexpr int AT = 0, AQ = 1, AA = 2, ANUN = 3, ASL = 7;
constexpr int AR_BLOCKS = 64;
/* partial-sum blocks of the packed-vector dots (coupled_krylov.hip) */
constexpr int KB = 512;
}  // namespace iemic

/* scalar parameters and coefficients (AtmosLocal::setParameters 106-171, setup 174-245) */
struct AtmPar {
    double comb, sunp, lonf, humf, latf, albf, tdif;
    double Ad, bmua, amua, Phv, nuq, eta, qdim, tdim, dqso, dqsi, Po0, Eo0, Ei0, Cs, lvscale;
    double a0, da, tauf, tauc, Ooa, Tm, Tr, Pa, epm, epr, epa, t0o, t0i;
    double total_area;
};

struct iemic_atmos {
    iemic_ctx* oc = nullptr;             /* the ocean context: device, stream, surface mask  */
    int refs = 1;                        /* the handle + coupled models built on it          */
    iemic_atmos_params prm{};
    int n = 0, m = 0, periodic = 0, dim = 0, rowint = 0, rowP = 0;
    AtmPar P{};
    double eta0 = 0, hdimq = 0, rhoo = 0, rhoa = 0, r0dim = 0, udim = 0;   /* for nuq */
    std::vector<int> surf;               /* (j, i): 1 land                                   */
    std::vector<double> tab;             /* per j (1..m): datc*cosdx2i, t4, t6, cosdx2i, q4, */
                                         /* q6, suna, suno (8 (m+1))                         */
    std::vector<double> pdist, pint;     /* n*m                                              */
    iemic::DevBuf<double> d_tab, d_pdist, d_pint, d_x, d_sst, d_F, d_val, d_red, d_tmp, d_y;
    iemic::DevBuf<int> d_surf, d_col;
    /* preconditioner: 9-point T and q operators, their cyclic reductions, work vectors */
    iemic::DevBuf<double> d_s9t, d_s9q, d_bt, d_bq, d_zt, d_zq;
    iemic::DevBuf<double> d_w, d_g, d_pred;          /* S_q^-1 (q-P column), P Schur partials + scalar   */
    iemic::DevBuf<int> d_colij;
    iemic::SchurCR crT, crQ;
    int jac_valid = 0, prec_valid = 0;
};

struct iemic_coupled {
    iemic_ctx* oc = nullptr;
    iemic_atmos* at = nullptr;
    int64_t NL = 0, NA = 0, NC = 0;      /* ocean owned rows, atmosphere rows, packed total  */
    iemic::DevBuf<double> xo, yo, ro, zo;       /* ocean ext-layout scratch                         */
    iemic::DevBuf<double> V, Z, w, r, tmpa, part, hb;
    iemic::DevBuf<double> hc;                   /* FGMRES: the step's CGS2 coefficients and norm    */
    iemic::DevBuf<double> tsurf;            /* n*m surface T of a packed vector (several ranks)  */
    int mk = 0;
    int synced = 0;
    double pars[18] = {};                /* CommPars of the last synchronisation            */
    double* h_red = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};  /* FGMRES: a step's coefficients in h_red         */
    ~iemic_coupled()
    {
        if (h_red) (void)hipHostFree(h_red);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

namespace iemic {

/* ---- per-cell atmosphere rows (computeJacobian 585-746 + boundaries 1429-1479) ------- */
struct AtmGeo {
    int n, m, periodic, dim, rowint, rowP;
    const double* tab;
    const double* pdist;
    const int* surf;
};

/* launch grid of the element-wise kernels on packed vectors */
inline unsigned blocks_for(int64_t N) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((N + 255) / 256, 4096)); }

/* atmos.hip */
AtmGeo atm_geo(const iemic_atmos* a);
int coupled_check(iemic_ctx* c);
void atmos_release(iemic_atmos* a);
/* y = J_a x (device vectors of length dim) */
int atm_spmv_dev(iemic_atmos* a, const double* x, double* y);
int atm_prec_compute(iemic_atmos* a);
int atm_prec_apply(iemic_atmos* a, const double* r, double* z);

/* coupled.hip */
/* y = [J_o C_oa; C_ao J_a] x on packed vectors [ocean owned rows | atmosphere] */
int cpl_apply(iemic_coupled* cm, const double* x, double* y);
/* forward block Gauss-Seidel: z_o = M_o^-1 r_o; z_a = M_a^-1 (r_a - C_ao z_o) */
int cpl_prec(iemic_coupled* cm, const double* r, double* z, int use_prec);
/* host vectors [ocean (reference order) | atmosphere] <-> packed [ocean owned rows |
 * atmosphere]; unpack_host writes this rank's owned ocean rows and the atmosphere */
void pack_host(const iemic_coupled* cm, const double* ref_vec, std::vector<double>& packed);
void unpack_host(const iemic_coupled* cm, const std::vector<double>& packed, double* ref_vec);

}  // namespace iemic

#endif
