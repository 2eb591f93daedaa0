/*
 * capi_diag.hip -- the C ABI's host-side diagnostics of the state, evaluated on the host as the
 * reference does (integral-condition coefficients, the sum over the ranks, the overturning
 * streamfunction, the integral checks), the surface fluxes, and the inserted forcing fields
 * (emip, tatm).  Built with capi.hip's flags: the host arithmetic is the reference's.
 */
#include <algorithm>
#include <cmath>

#include "capi_internal.h"

using namespace iemic;

/* THCM::getIntCondCoeff (THCM.C:2549-2577): the integral-condition coefficients */
extern "C" int iemic_get_intcond_coeff(iemic_ctx* c, double* out)
{
    CTX_CHECK(c);
    if (!out) return IEMIC_EINVAL;
    return get_ref(c, c->d_intc.p, out);
}

namespace iemic {
int host_state(iemic_ctx* c, std::vector<double>& x)
{
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    x.assign((size_t)c->sub.nerows(), 0.0);
    return d2h(c, x.data(), c->d_x.p, sizeof(double) * x.size());
}
int host_sum(iemic_ctx* c, std::vector<double>& v)
{
    if (c->sub.nranks <= 1) return 0;
    DevBuf<double> d;
    if (d.alloc(v.size())) return IEMIC_ENOMEM;
    int rc = h2d(c, d.p, v.data(), sizeof(double) * v.size());
    if (!rc) rc = allreduce_sum(c, d.p, (int)v.size());
    if (!rc) rc = d2h(c, v.data(), d.p, sizeof(double) * v.size());
    return rc;
}
int host_max(iemic_ctx* c, double* mx)
{
    if (c->sub.nranks <= 1) return 0;
    std::vector<double> all((size_t)c->sub.nranks, 0.0);
    all[(size_t)c->sub.rank] = *mx;
    int rc = host_sum(c, all);
    if (rc) return rc;
    *mx = 0.0;
    for (double v : all) *mx = nanmax(*mx, v);
    return 0;
}
}  // namespace iemic

/* Epetra_Comm::SumAll over the context's ranks (host buffer, in place) */
extern "C" int iemic_allreduce_sum(iemic_ctx* c, double* buf, int64_t count)
{
    CTX_CHECK(c);
    if (count < 0 || (count > 0 && !buf) || count > INT32_MAX) return IEMIC_EINVAL;
    if (c->sub.nranks <= 1 || count == 0) return 0;
    std::vector<double> v(buf, buf + count);
    int rc = host_sum(c, v);
    if (!rc) std::copy(v.begin(), v.end(), buf);
    return rc;
}

/* Ocean::getPsiM (Ocean.C:872-886): the meridional overturning streamfunction of the
 * state, OceanGrid::recomputePsiM (OceanGrid.C:270-346: v of usol integrated over x, times
 * dx) and m_thcm_utils::compute_psim (thcm_utils.F90:95-118: -cos(yv) vs dz dfzT summed up
 * from the bottom below 500 m), its extrema over (0:m, 0:l), in Sv (r0dim hdim udim 1e-6).
 * psim (optional): PsiM(j, k) at [(m+1) k + j]. */
extern "C" int iemic_psim(iemic_ctx* c, double* psim_min, double* psim_max, double* psim)
{
    CTX_CHECK(c);
    if (!psim_min || !psim_max) return IEMIC_EINVAL;
    std::vector<double> x;
    int rc = host_state(c, x);
    if (rc) return rc;
    const auto& su = c->su;
    const Geo g = su.geo(su.landm.data(), su.tab.data());
    const int n = c->n, m = c->m, l = c->l;
    std::vector<double> ps((size_t)(m + 1) * (l + 1), 0.0);
    for (int j = c->sub.jb0 + 1; j <= c->sub.jb1 && j <= m; j++) {          /* 1-based, owned */
        const double cs = std::cos(su.yv[j]);
        for (int k = 1; k <= l; k++) {
            double sum = 0.0;
            for (int i = c->sub.ib0 + 1; i <= c->sub.ib1; i++) sum += uv_arr(g, x.data(), VV, i, j, k);
            const double vs = sum * su.dx;
            const double zk = host::fz(((double)k - 0.5) * su.dz + host::zmin, su.cfg.qz);
            if (zk * su.cfg.hdim < -500.0)
                ps[(size_t)(m + 1) * k + j] = -cs * vs * su.dz * su.dfzT[k] + ps[(size_t)(m + 1) * (k - 1) + j];
        }
    }
    if ((rc = host_sum(c, ps))) return rc;
    const double transc = host::r0dim * su.cfg.hdim * host::udim * 1e-6;
    double mn = ps[0], mx = ps[0];
    for (double v : ps) {
        mn = std::min(mn, v);
        mx = std::max(mx, v);
    }
    *psim_min = mn * transc;
    *psim_max = mx * transc;
    if (psim)
        for (size_t q = 0; q < ps.size(); q++) psim[q] = ps[q] * transc;
    return 0;
}

/* Ocean::integralChecks (Ocean.C:1841-1848 -> THCM.C:2042-2118): the volume integrals of
 * the salt advection and salt diffusion operators of the state (m_integrals,
 * integrals.F90:17-89, over usol's padded fields; the advection sum covers the columns whose
 * top cell is ocean, as there).  Discrete conservation makes both vanish. */
extern "C" int iemic_integral_checks(iemic_ctx* c, double* salt_advection, double* salt_diffusion)
{
    CTX_CHECK(c);
    if (!salt_advection || !salt_diffusion) return IEMIC_EINVAL;
    std::vector<double> x;
    int rc = host_state(c, x);
    if (rc) return rc;
    const auto& su = c->su;
    const Geo g = su.geo(su.landm.data(), su.tab.data());
    const int n = c->n, m = c->m, l = c->l;
    const double dx = su.dx, dy = su.dy, dz = su.dz;
    const double* xs = x.data();
    auto u = [&](int i, int j, int k) { return uv_arr(g, xs, UU, i, j, k); };
    auto v = [&](int i, int j, int k) { return uv_arr(g, xs, VV, i, j, k); };
    auto w = [&](int i, int j, int k) { return w_arr(g, xs, i, j, k); };
    auto sa = [&](int i, int j, int k) { return ts_arr(g, xs, SS, i, j, k); };
    std::vector<double> sums(2, 0.0);
    for (int k = 1; k <= l; k++) {
        const double h1 = 1.0 / (su.dfzT[k] * su.dfzW[k]), h2 = 1.0 / (su.dfzT[k] * su.dfzW[k - 1]);
        for (int j = c->sub.jb0 + 1; j <= c->sub.jb1 && j <= m; j++) {
            const double cay = std::cos(su.y[j]), c1 = std::cos(su.yv[j]), c2 = std::cos(su.yv[j - 1]);
            for (int i = c->sub.ib0 + 1; i <= c->sub.ib1; i++) {
                if (LM(g, i, j, l) == OCEAN)
                    sums[0] += (u(i, j, k) + u(i, j - 1, k)) * (sa(i + 1, j, k) + sa(i, j, k)) / (4 * dx) -
                               (u(i - 1, j, k) + u(i - 1, j - 1, k)) * (sa(i, j, k) + sa(i - 1, j, k)) / (4 * dx) +
                               (v(i, j, k) + v(i - 1, j, k)) * (sa(i, j + 1, k) + sa(i, j, k)) * std::cos(su.yv[j]) / (4 * dy) -
                               (v(i, j - 1, k) + v(i - 1, j - 1, k)) * (sa(i, j, k) + sa(i, j - 1, k)) *
                                   std::cos(su.yv[j - 1]) / (4 * dy) +
                               w(i, j, k) * (sa(i, j, k + 1) + sa(i, j, k)) * std::cos(su.y[j]) / (2 * dz * su.dfzW[k]) -
                               w(i, j, k - 1) * (sa(i, j, k) + sa(i, j, k - 1)) * std::cos(su.y[j]) /
                                   (2 * dz * su.dfzW[k - 1]);
                if (LM(g, i, j, k) == OCEAN)
                    sums[1] += std::cos(su.y[j]) * su.dfzT[k] *
                               ((sa(i + 1, j, k) + sa(i - 1, j, k) - 2 * sa(i, j, k)) / (dx * dx * cay * cay) +
                                (c1 * sa(i, j + 1, k) + c2 * sa(i, j - 1, k) - (c1 + c2) * sa(i, j, k)) / (dy * dy * cay) +
                                (h1 * sa(i, j, k + 1) + h2 * sa(i, j, k - 1) - (h1 + h2) * sa(i, j, k)) / (dz * dz));
            }
        }
    }
    if ((rc = host_sum(c, sums))) return rc;
    *salt_advection = sums[0];
    *salt_diffusion = sums[1];
    return 0;
}

/* ---- surface fluxes and inserted forcing fields ------------------------------------- */
/* THCM::getFluxes (THCM.C:1559-1593; m_probe get_salflux / get_temflux, probe.F90:200-355),
 * what Ocean::additionalExports writes (Ocean.C:1904-1929): out = [9][n*m] in the order of
 * THCM's enum (_Sal, _QSOA, _QSOS, _Temp, _QSW, _QSH, _QLH, _QTOS, _MSI), (j, i) with i
 * fastest; each rank writes the surface cells it owns.  scorr (THCM::scorr_): the salinity
 * correction times COMB*SALT, the same on every rank. */
extern "C" int iemic_get_fluxes(iemic_ctx* c, const double* x, double* out, double* scorr)
{
    CTX_CHECK(c);
    if (!out || !scorr) return IEMIC_EINVAL;
    const double* xd = c->d_x.p;
    int rc = 0;
    if (x) {
        if ((rc = put_ref(c, x, c->d_tmp1.p))) return rc;
        xd = c->d_tmp1.p;
    }
    const size_t nm = (size_t)c->n * c->m;
    std::vector<double> all((size_t)NFLUX * nm);
    if ((rc = surface_fluxes(c, xd, all.data(), scorr))) return rc;
    for (int f = 0; f < NFLUX; f++)
        for (int j = c->sub.jb0; j < c->sub.jb1; j++)
            for (int i = c->sub.ib0; i < c->sub.ib1; i++) {
                const size_t q = f * nm + (size_t)j * c->n + i;
                out[q] = all[q];
            }
    return 0;
}

namespace {
int ins_slot(char mode) { return mode == 'E' ? 0 : mode == 'A' ? 1 : mode == 'P' ? 2 : -1; }
/* slot of iemic_ctx::d_ins <- field (null: back to the profile), then forcing again */
int insert_field(iemic_ctx* c, int slot, const double* field, bool mask)
{
    const int n = c->n, m = c->m, l = c->l;
    const size_t nm = (size_t)n * m;
    if (!field) {
        c->ins_on[slot] = 0;
        return compute_forcing(c);
    }
    if (!c->d_ins.p) {
        if (c->d_ins.alloc(4 * nm)) {
            set_error("insert: out of device memory");
            return IEMIC_ENOMEM;
        }
        int rc = dev_zero(c, c->d_ins.p, (int64_t)(4 * nm));
        if (rc) return rc;
    }
    std::vector<double> v(field, field + nm);
    if (mask)
        for (int j = 1; j <= m; j++)
            for (int i = 1; i <= n; i++)
                v[(size_t)(j - 1) * n + (i - 1)] *= (double)(1 - c->su.landm[((size_t)l * (m + 2) + j) * (n + 2) + i]);
    int rc = h2d(c, c->d_ins.p + slot * nm, v.data(), sizeof(double) * nm);
    if (rc) return rc;
    c->ins_on[slot] = 1;
    return compute_forcing(c);
}
}  // namespace

/* THCM::setEmip (THCM.C:1486-1514; m_inserts insert_emip / insert_adapted_emip /
 * insert_emip_pert, inserts.F90:164-224, each masked with 1 - landm(i,j,l)): mode 'E' emip,
 * 'A' adapted_emip, 'P' spert, as whole n*m surface fields on every rank.  From then on the
 * forcing uses the field in place of the idealized profile (the reference's its = 0); NULL
 * restores the profile. */
extern "C" int iemic_set_emip(iemic_ctx* c, char mode, const double* field_nm)
{
    CTX_CHECK(c);
    const int slot = ins_slot(mode);
    if (slot < 0) {
        set_error("iemic_set_emip: mode must be 'E', 'A' or 'P'");
        return IEMIC_EINVAL;
    }
    return insert_field(c, slot, field_nm, true);
}

/* THCM::getEmip (THCM.C:1530-1556; m_probe get_emip / get_adapted_emip / get_emip_pert,
 * probe.F90:140-197): the field the forcing uses; 'E' comes back times 1 - landm(i,j,l) */
extern "C" int iemic_get_emip(iemic_ctx* c, char mode, double* out_nm)
{
    CTX_CHECK(c);
    const int slot = ins_slot(mode);
    if (slot < 0 || !out_nm) {
        set_error("iemic_get_emip: mode must be 'E', 'A' or 'P'");
        return IEMIC_EINVAL;
    }
    const int n = c->n, m = c->m, l = c->l;
    const size_t nm = (size_t)n * m;
    if (c->ins_on[slot]) {
        int rc = d2h(c, out_nm, c->d_ins.p + slot * nm, sizeof(double) * nm);
        if (rc) return rc;
    } else {
        const std::vector<double> t = c->su.forcing_tables();
        for (int j = 1; j <= m; j++)
            for (int i = 1; i <= n; i++) {
                const size_t q = (size_t)(j - 1) * n + (i - 1);
                const int lm = c->su.landm[((size_t)l * (m + 2) + j) * (n + 2) + i];
                out_nm[q] = slot == 0 ? t[2 * (m + 2) + j] * (1 - lm) : slot == 1 ? 0.0 : t[3 * (m + 2) + q];
            }
    }
    if (slot == 0)
        for (int j = 1; j <= m; j++)
            for (int i = 1; i <= n; i++)
                out_nm[(size_t)(j - 1) * n + (i - 1)] *= (double)(1 - c->su.landm[((size_t)l * (m + 2) + j) * (n + 2) + i]);
    return 0;
}

/* THCM::setTatm (THCM.C:1466-1483; m_inserts insert_tatm, inserts.F90:227-245, unmasked):
 * the atmospheric temperature / heat flux the ocean-only forcing uses in place of the
 * idealized profile (the reference's ite = 0); NULL restores the profile.  A context with
 * coupled_t = 1 takes its tatm from iemic_set_atmosphere. */
extern "C" int iemic_set_tatm(iemic_ctx* c, const double* field_nm)
{
    CTX_CHECK(c);
    if (c->cfg.coupled_t) {
        set_error("iemic_set_tatm: the context has coupled_t = 1 (tatm comes from the atmosphere)");
        return IEMIC_EINVAL;
    }
    return insert_field(c, 3, field_nm, false);
}
