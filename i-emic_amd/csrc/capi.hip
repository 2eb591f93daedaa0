/*
 * capi.hip -- the C ABI (include/iemic.h): the context and what is set on and read from it:
 * the error string, the fatal-signal trace, creation and destruction, parameters and the
 * atmosphere's fields, the layout getters, the state.  The rest of the ABI's ocean entry points:
 * capi_diag.hip (host diagnostics and inserted forcing fields), newton.hip (operator, solves,
 * the Newton iteration, theta and eigs), capi_vec.hip (device vectors), capi_time.hip (timing
 * probes); atmos.hip and coupled.hip hold their models'.
 *
 * iemic_create restates the serial set-up of the THCM constructor
 * (src/ocean/THCM.C:178-798): init_ (usrc.F90:6-139: border handling of the land mask,
 * grid (grid.F90), QTnd/QSnd, stpnt + vmix_par, forcing), rowintcon and intcond
 * coefficients (THCM.C:661-717, thcm_utils.F90:285-312), then the Ocean mask-fix cycle
 * (Ocean.C:496-569, analyzeJacobian1 at the zero state).  The 1-D metric tables (cos, tan,
 * sin of the y grid, stretching derivatives) are evaluated once on the host with the same
 * libm the reference uses, so every per-cell expression evaluated on the device is
 * bit-identical to the reference; all per-cell and per-row work runs on the GPU.
 */
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "capi_internal.h"

namespace iemic {
static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
}  // namespace iemic

using namespace iemic;

extern "C" const char* iemic_last_error(void) { return g_err.c_str(); }

/* Fatal-signal trace: on SIGSEGV / SIGBUS / SIGILL / SIGFPE the library writes the native
 * backtrace of the faulting thread to stderr (backtrace_symbols_fd: no allocation), then
 * restores the handler that was installed before (Python's faulthandler, a profiler's, or the
 * default) and lets the fault recur into it, so the process still ends as it would have.
 * Installed once, at the first context creation; IEMIC_SEGV_TRACE=0 leaves the handlers alone. */
namespace {
constexpr int kTraceSigs[4] = {SIGSEGV, SIGBUS, SIGILL, SIGFPE};
struct sigaction g_prev_act[4];

void fatal_trace(int sig, siginfo_t* si, void*)
{
    static const char hdr[] = "\niemic: fatal signal in the process; native backtrace of the faulting thread:\n";
    (void)!write(2, hdr, sizeof(hdr) - 1);
    void* fr[64];
    const int n = backtrace(fr, 64);
    backtrace_symbols_fd(fr, n, 2);
    for (int q = 0; q < 4; q++)
        if (kTraceSigs[q] == sig) sigaction(sig, &g_prev_act[q], nullptr);
    /* a fault raised by the hardware recurs when the instruction is re-executed on return;
     * a signal sent by a process is re-sent */
    if (!si || si->si_code <= 0) raise(sig);
}

void install_fatal_trace()
{
    static std::once_flag once;
    std::call_once(once, [] {
        const char* e = std::getenv("IEMIC_SEGV_TRACE");
        if (e && e[0] == '0') return;
        void* warm[2];
        (void)backtrace(warm, 2);            /* loads the unwinder outside any handler */
        struct sigaction sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.sa_sigaction = fatal_trace;
        sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
        sigemptyset(&sa.sa_mask);
        for (int q = 0; q < 4; q++) sigaction(kTraceSigs[q], &sa, &g_prev_act[q]);
    });
}
}  // namespace

extern "C" int iemic_abi_version(void) { return IEMIC_ABI_VERSION; }

extern "C" int iemic_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

Geo iemic_ctx::geo() const
{
    Geo g = su.geo(d_landm.p, d_tab.p, d_atm.p);
    const size_t nm = (size_t)n * m;
    g.ins_emip = ins_on[0] ? d_ins.p : nullptr;
    g.ins_aemip = ins_on[1] ? d_ins.p + nm : nullptr;
    g.ins_spert = ins_on[2] ? d_ins.p + 2 * nm : nullptr;
    g.ins_tatm = ins_on[3] ? d_ins.p + 3 * nm : nullptr;
    return g;
}

iemic_ctx::~iemic_ctx()
{
    if (stream) (void)hipStreamSynchronize(stream);
    if (h_red) (void)hipHostFree(h_red);
    h_red = nullptr;
    if (side) (void)hipStreamSynchronize(side);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (side) (void)hipStreamDestroy(side);
    if (stream) (void)hipStreamDestroy(stream);
    stream = side = nullptr;
    if (group) iemic::local_group_leave(this);   /* the group outlives its last context */
    /* device buffers are members: released after this body, with the stream drained */
}

namespace {

int upload_forcing_tables(iemic_ctx* c)
{
    std::vector<double> t = c->su.forcing_tables();
    HIP_OK(hipMemcpyAsync(c->d_ftab.p, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice,
                          c->stream));
    DEV_SYNC(c);
    return compute_forcing(c);
}

int upload_landm(iemic_ctx* c)
{
    int rc = h2d(c, c->d_landm.p, c->su.landm.data(), sizeof(int) * c->su.landm.size());
    if (rc) return rc;
    std::vector<double> ic = c->su.intcond_coeff();
    return h2d(c, c->d_intc.p, ic.data(), sizeof(double) * ic.size());
}

/* Ocean::analyzeJacobian1 (Ocean.C:273-340) + THCM::getLandMask(fix) (THCM.C:1298-1330):
 * P rows with at most 2 entries |v| > 1e-10 (and not a land identity row) become land.
 * Each rank inspects its band; the fixes are summed over the ranks so every rank applies
 * the same mask. */
int mask_fix(iemic_ctx* c)
{
    const int n = c->n, m = c->m;
    HIP_OK(hipMemsetAsync(c->d_tmp1.p, 0, sizeof(double) * c->sub.nerows(), c->stream));
    const int pb = ROW_BEGIN[PP], pn = ROW_BEGIN[PP + 1] - ROW_BEGIN[PP];
    std::vector<double> pv((size_t)pn * c->sub.nloc);
    DevBuf<double> dflag;
    if (c->sub.nranks > 1 && dflag.alloc(c->ncell)) return IEMIC_ENOMEM;
    std::vector<double> flag;
    for (int cyc = 0; cyc < std::max(1, c->cfg.max_mask_fixes); cyc++) {
        int rc = assemble_jacobian(c, c->d_tmp1.p);
        if (rc) return rc;
        if ((rc = d2h(c, pv.data(), c->d_val.p + (size_t)pb * c->sub.nloc, sizeof(double) * pv.size())))
            return rc;
        flag.assign(c->ncell, 0.0);
        for (int64_t lc = 0; lc < c->sub.nloc; lc++) {
            int i, j, k;
            c->su.owned_ijk(lc, i, j, k);
            if (NUN * c->su.ref_cell(i, j, k) + PP == c->su.rowintcon_ref) continue;
            double sum = 0.0;
            int el = 0;
            for (int s = 0; s < pn; s++) {
                double v = pv[(size_t)s * c->sub.nloc + lc];
                sum += v;
                if (std::fabs(v) > 1e-10) el++;
            }
            if (sum == 1) continue;
            if (el <= 2) flag[c->su.ref_cell(i, j, k)] = 1.0;
        }
        if (c->sub.nranks > 1) {
            if ((rc = h2d(c, dflag.p, flag.data(), sizeof(double) * c->ncell))) return rc;
            if ((rc = allreduce_sum(c, dflag.p, (int)c->ncell))) return rc;
            if ((rc = d2h(c, flag.data(), dflag.p, sizeof(double) * c->ncell))) return rc;
        }
        int nfix = 0;
        for (int64_t q = 0; q < c->ncell; q++)
            if (flag[q] != 0.0) {
                const int i = (int)(q % n) + 1, j = (int)((q / n) % m) + 1, k = (int)(q / ((int64_t)n * m)) + 1;
                c->su.landm[((size_t)k * (m + 2) + j) * (n + 2) + i] = LAND;
                nfix++;
            }
        if (nfix == 0) break;
        int rc2 = upload_landm(c);
        if (rc2) return rc2;
        rc2 = upload_forcing_tables(c);
        if (rc2) return rc2;
    }
    c->jac_valid = 0;
    return 0;
}

}  // namespace

extern "C" int iemic_comm_unique_id(unsigned char* id128)
{
    if (!id128) return IEMIC_EINVAL;
    return comm_unique_id(id128);
}

extern "C" int iemic_decomp2d(int n, int m, int nranks, int* npx, int* npy)
{
    if (nranks < 1 || !npx || !npy) return IEMIC_EINVAL;
    decomp2d(n, m, nranks, *npx, *npy);
    return 0;
}

struct CreateArgs {
    const iemic_dist* dist = nullptr;       /* RCCL                                       */
    void* group = nullptr;                  /* in-process rank group                      */
    const iemic_transport* tp = nullptr;    /* host transport                             */
    int rank = 0, nranks = 1, npx = 1;
};
static int create_impl(iemic_ctx** out, const iemic_grid* grid, const int* landm, const CreateArgs& a);

extern "C" int iemic_create_dist(iemic_ctx** out, const iemic_grid* grid, const int* landm,
                                 const iemic_dist* dist)
{
    CreateArgs a;
    if (dist) {
        a.dist = dist;
        a.rank = dist->rank;
        a.nranks = dist->nranks;
        a.npx = dist->npx;
    }
    return create_impl(out, grid, landm, a);
}

extern "C" int iemic_create_transport(iemic_ctx** out, const iemic_grid* grid, const int* landm, int rank,
                                      int nranks, int npx, const iemic_transport* tp)
{
    if (!tp || !tp->send || !tp->recv || !tp->allreduce_sum) return IEMIC_EINVAL;
    CreateArgs a;
    a.tp = tp;
    a.rank = rank;
    a.nranks = nranks;
    a.npx = npx;
    return create_impl(out, grid, landm, a);
}

extern "C" void* iemic_local_group_new(int nranks) { return local_group_new(nranks); }
extern "C" void iemic_local_group_free(void* group) { local_group_free(group); }
extern "C" int iemic_create_local_2d(iemic_ctx** out, const iemic_grid* grid, const int* landm,
                                     void* group, int rank, int nranks, int npx)
{
    if (!group) return IEMIC_EINVAL;
    CreateArgs a;
    a.group = group;
    a.rank = rank;
    a.nranks = nranks;
    a.npx = npx;
    return create_impl(out, grid, landm, a);
}
extern "C" int iemic_create_local(iemic_ctx** out, const iemic_grid* grid, const int* landm,
                                  void* group, int rank, int nranks)
{
    return iemic_create_local_2d(out, grid, landm, group, rank, nranks, 1);
}

static int create_impl(iemic_ctx** out, const iemic_grid* grid, const int* landm, const CreateArgs& a)
{
    if (!out || !grid || !landm) return IEMIC_EINVAL;
    *out = nullptr;
    install_fatal_trace();
    int ndev = iemic_device_count();
    if (ndev <= 0) {
        set_error("iemic_create: no HIP device available (the library never runs on the CPU)");
        return IEMIC_ENODEV;
    }
    if (grid->vmix < 0 || grid->vmix > 2) {
        set_error("iemic_create: Mixing must be 0, 1 or 2");
        return IEMIC_EINVAL;
    }
    if (grid->n < 3 || grid->m < 2 || grid->l < 2) {
        set_error("iemic_create: grid too small");
        return IEMIC_EINVAL;
    }
    Sub sub;
    if (const char* why = sub_init(sub, grid->n, grid->m, grid->l, grid->periodic, a.rank, a.nranks, a.npx)) {
        set_error(std::string("iemic_create: ") + why);
        return IEMIC_EINVAL;
    }
    iemic_ctx* c = new iemic_ctx();
    if (const char* e = std::getenv("IEMIC_COMM_TIMEOUT")) {
        const double v = std::atof(e);
        if (v > 0.0) c->comm_timeout_s = v;
    }
    if (const char* e = std::getenv("IEMIC_SERIAL_SETUP")) c->serial_setup = std::atoi(e) != 0;
    c->cfg = *grid;
    c->device = std::min(std::max(grid->device, 0), ndev - 1);
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        set_error("iemic_create: cannot initialise the HIP device");
        delete c;
        return IEMIC_EDEVICE;
    }
    c->n = grid->n; c->m = grid->m; c->l = grid->l;
    c->ncell = (int64_t)c->n * c->m * c->l;
    c->nrows = NUN * c->ncell;
    c->su.init(*grid, landm, sub);
    const int n = c->n, m = c->m, l = c->l;
    const size_t nl = (size_t)(n + 2) * (m + 2) * (l + 2);
    c->su.vmix_init();
    c->rowintcon = c->su.rowintcon;
    int rc = 0;
    if (a.group) local_group_join(c, a.group);
    else if (a.tp) c->tp = *a.tp;
    else if (sub.nranks > 1 && (rc = comm_init(c, a.dist->id, sub.rank, sub.nranks))) {
        delete c;
        return rc;
    }
    if (sub.nranks > 1 && (rc = comm_verify_plans(c))) {
        comm_destroy(c);
        delete c;
        return rc;
    }
    const int64_t NE = c->sub.nerows();
    rc |= c->d_landm.alloc(nl);
    rc |= c->d_ftab.alloc((size_t)3 * (m + 2) + (size_t)n * m);
    rc |= c->d_frc.alloc(NE);
    rc |= c->d_qcor.alloc(8);
    rc |= c->d_intc.alloc(NE);
    rc |= c->d_atm.alloc((size_t)4 * n * m);
    rc |= c->d_x.alloc(NE);
    rc |= c->d_F.alloc(NE);
    rc |= c->d_B.alloc(NE);
    rc |= c->d_val.alloc((size_t)NSLOT * c->sub.nloc);
    rc |= c->d_tmp1.alloc(NE);
    rc |= c->d_tmp2.alloc(NE);
    rc |= c->d_red.alloc(2048);
    rc |= c->d_part.alloc((size_t)RED_BLOCKS * RED_ROWS);
    rc |= c->d_hbuf.alloc((size_t)2 * RED_ROWS);
    /* coherent: the DCGS2 update (dcgs_rows_out) writes the Hessenberg rows straight into it */
    if (!rc && hipHostMalloc(&c->h_red, sizeof(double) * 2 * RED_ROWS, hipHostMallocCoherent) != hipSuccess) rc = 1;
    if (rc) {
        set_error("iemic_create: out of device memory");
        delete c;
        return IEMIC_ENOMEM;
    }
    for (DevBuf<double>* b : {&c->d_x, &c->d_F, &c->d_B, &c->d_frc, &c->d_tmp1, &c->d_tmp2, &c->d_atm})
        (void)hipMemsetAsync(b->p, 0, sizeof(double) * b->n, c->stream);
    if (c->d_tab.alloc(c->su.tab.size()) ||
        h2d(c, c->d_tab.p, c->su.tab.data(), sizeof(double) * c->su.tab.size()) != 0) {
        set_error("iemic_create: cannot upload metric tables");
        delete c;
        return IEMIC_EDEVICE;
    }
    if ((rc = upload_landm(c))) {
        delete c;
        return rc;
    }
    if ((rc = upload_forcing_tables(c))) {
        delete c;
        return rc;
    }
    if (grid->analyze_jacobian) {
        if ((rc = mask_fix(c))) {
            delete c;
            return rc;
        }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
        set_error("iemic_create: device error during set-up");
        delete c;
        return IEMIC_EDEVICE;
    }
    *out = c;
    return 0;
}

extern "C" int iemic_create(iemic_ctx** out, const iemic_grid* grid, const int* landm)
{
    return iemic_create_dist(out, grid, landm, nullptr);
}

namespace iemic {
void ctx_release(iemic_ctx* c)
{
    if (!c || --c->refs > 0) return;
    (void)hipSetDevice(c->device);
    comm_destroy(c);
    delete c; /* ~iemic_ctx drains the stream before any buffer is released */
}
}  // namespace iemic

/* the context lives on while an atmosphere or coupled model built on it exists */
extern "C" void iemic_destroy(iemic_ctx* c) { ctx_release(c); }

namespace iemic {
int put_ref(iemic_ctx* c, const double* ref, double* dev)
{
    std::vector<double> e((size_t)c->sub.nerows(), 0.0);
    c->su.ref_to_ext(ref, e.data());
    return h2d(c, dev, e.data(), sizeof(double) * e.size());
}
int get_ref(iemic_ctx* c, const double* dev, double* ref)
{
    std::vector<double> e((size_t)c->sub.nerows());
    int rc = d2h(c, e.data(), dev, sizeof(double) * e.size());
    if (rc) return rc;
    c->su.ext_to_ref(e.data(), ref);
    return 0;
}

/* reference-ordered global device vector -> ext layout (owned rows) */
__global__ void k_ref_to_ext(const double* __restrict__ ref, double* __restrict__ ext, int n, int m,
                             int l, int jb0, int ib0, int nx, int64_t nloc)
{
    const int64_t lc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (lc >= nloc) return;
    const int i = ib0 + (int)(lc % nx), k = (int)((lc / nx) % l), j = jb0 + (int)(lc / ((int64_t)nx * l));
    const int64_t e = NUN * ((int64_t)HALO * l * nx + lc), r = NUN * (((int64_t)k * m + j) * n + i);
    for (int v = 0; v < NUN; v++) ext[e + v] = ref[r + v];
}
}  // namespace iemic

/* Ocean::synchronize(atmos) (Ocean.C:1443-1472): THCM::setAtmosphereT/Q/A/P (inserted
 * into tatm/qatm/albe/patm, inserts.F90:12-100) and set_atmos_parameters (usrc.F90:237-293:
 * CommPars -> qdim, eta, dqso, eo0, albe0, albed, nus, lvsc; then forcing and lin).  The
 * fields are n*m surface vectors, (j, i) with i fastest; p (patm, dimensional) enters
 * the salinity flux with "Coupled Salinity" = 1. */
extern "C" int iemic_set_atmosphere(iemic_ctx* c, const double* t, const double* q, const double* a,
                                    const double* p, const double* commpars)
{
    CTX_CHECK(c);
    if (!c->cfg.coupled_t && !c->cfg.coupled_s) {
        set_error("iemic_set_atmosphere: the context was created with coupled_t = coupled_s = 0");
        return IEMIC_EINVAL;
    }
    if (!t || !q || !a || !commpars) return IEMIC_EINVAL;
    const size_t nm = (size_t)c->n * c->m;
    int rc = h2d(c, c->d_atm.p, t, sizeof(double) * nm);
    if (!rc) rc = h2d(c, c->d_atm.p + nm, q, sizeof(double) * nm);
    if (!rc) rc = h2d(c, c->d_atm.p + 2 * nm, a, sizeof(double) * nm);
    if (!rc && p) rc = h2d(c, c->d_atm.p + 3 * nm, p, sizeof(double) * nm);
    if (rc) return rc;
    c->su.set_atmos(commpars);
    c->jac_valid = 0;
    return compute_forcing(c);
}

/* getdeps (usrc.F90:201-219): Ooa, Os, nus, eta, lvsc, qdim, pQSnd */
extern "C" int iemic_get_deps(iemic_ctx* c, double* out7)
{
    if (!c || !out7) return IEMIC_EINVAL;
    const host::Setup& su = c->su;
    const double v[7] = {su.Ooa, su.Os, su.nus, su.eta_a, su.lvsc, su.qdim_a,
                         su.par[P_COMB] * su.par[P_SALT] * su.qsnd};
    for (int i = 0; i < 7; i++) out7[i] = v[i];
    return 0;
}

/* THCM::getSunO (THCM.C:1517-1527, m_probe get_suno): suno(j) on the n*m surface */
extern "C" int iemic_get_suno(iemic_ctx* c, double* out_nm)
{
    if (!c || !out_nm) return IEMIC_EINVAL;
    const host::Setup& su = c->su;
    const double* suno = su.tab.data() + 9 * (su.m + 2) + 2 * (su.l + 2);
    for (int j = 0; j < su.m; j++)
        for (int i = 0; i < su.n; i++) out_nm[(size_t)j * su.n + i] = suno[j + 1];
    return 0;
}

extern "C" int iemic_set_par(iemic_ctx* c, int idx, double value)
{
    CTX_CHECK(c);
    if (idx < 1 || idx > 30) {
        set_error("iemic_set_par: index out of range 1..30");
        return IEMIC_EINVAL;
    }
    c->su.par[idx] = value;       /* setparcs_ (usrc.F90:163-181): par, then forcing + lin */
    c->jac_valid = 0;
    int rc = upload_forcing_tables(c);
    if (rc) return rc;
    DEV_SYNC(c);
    return 0;
}

extern "C" int iemic_get_par(iemic_ctx* c, int idx, double* value)
{
    if (!c || !value || idx < 1 || idx > 30) return IEMIC_EINVAL;
    *value = c->su.par[idx];
    return 0;
}

extern "C" int iemic_nrows(const iemic_ctx* c) { return c ? (int)c->nrows : IEMIC_EINVAL; }
extern "C" int iemic_rowintcon(const iemic_ctx* c) { return c ? c->su.rowintcon_ref : IEMIC_EINVAL; }
extern "C" int iemic_landm(const iemic_ctx* c, int* out)
{
    if (!c || !out) return IEMIC_EINVAL;
    std::memcpy(out, c->su.landm.data(), sizeof(int) * c->su.landm.size());
    return 0;
}
extern "C" int iemic_layout(const iemic_ctx* c, int64_t* out)
{
    if (!c || !out) return IEMIC_EINVAL;
    const Sub& S = c->sub;
    const int64_t v[12] = {S.nerows(), NUN * S.own0, S.nlrows(), S.jb0, S.jb1, S.rank,
                           S.nranks,   S.ib0,        S.ib1,      S.npx, S.npy, S.hx};
    std::copy(v, v + 12, out);
    return 0;
}

extern "C" int iemic_active_cells(const iemic_ctx* c, int64_t* nact)
{
    if (!c || !nact) return IEMIC_EINVAL;
    *nact = c->gs.ready && c->gs.kind == 2 ? c->gs.act.nact : 0;
    return 0;
}

/* communication counters since the last call (halo batches, messages and bytes sent,
 * all-reduces), reset by the call */
extern "C" int iemic_comm_stats(iemic_ctx* c, int64_t* out4)
{
    if (!c || !out4) return IEMIC_EINVAL;
    for (int q = 0; q < 4; q++) {
        out4[q] = c->stat[q];
        c->stat[q] = 0;
    }
    return 0;
}

extern "C" int iemic_set_comm_timeout(iemic_ctx* c, double seconds)
{
    if (!c || !(seconds > 0.0)) return IEMIC_EINVAL;
    c->comm_timeout_s = seconds;
    return 0;
}

/* the ranks the communicator reports (RCCL: ncclCommCount) and the transport kind */
extern "C" int iemic_comm_size(const iemic_ctx* c, int* size, int* kind)
{
    if (!c || !size || !kind) return IEMIC_EINVAL;
    return comm_size(c, size, kind);
}

/* Maximal-graph rows owned by this context (THCM.C:2288-2521) */
extern "C" int64_t iemic_graph_nnz(const iemic_ctx* c)
{
    if (!c) return IEMIC_EINVAL;
    return c->su.to_csr(nullptr, nullptr, nullptr, nullptr);
}

extern "C" int iemic_set_state(iemic_ctx* c, const double* x)
{
    CTX_CHECK(c);
    if (!x) return IEMIC_EINVAL;
    int rc = put_ref(c, x, c->d_x.p);
    if (rc) return rc;
    c->jac_valid = 0;
    return 0;
}
extern "C" int iemic_set_intcond_correction(iemic_ctx* c, const double* x)
{
    CTX_CHECK(c);
    const double* xd = c->d_x.p;
    if (x) {
        int rc = put_ref(c, x, c->d_tmp1.p);
        if (rc) return rc;
        xd = c->d_tmp1.p;
    }
    return intcond_correction(c, xd);
}
extern "C" int iemic_get_intcond_correction(iemic_ctx* c, double* corr)
{
    CTX_CHECK(c);
    if (!corr) return IEMIC_EINVAL;
    *corr = c->int_correction;
    return 0;
}
extern "C" int iemic_set_state_dev(iemic_ctx* c, const double* x_dev)
{
    CTX_CHECK(c);
    if (!x_dev) return IEMIC_EINVAL;
    hipLaunchKernelGGL(k_ref_to_ext, dim3((unsigned)((c->sub.nloc + 255) / 256)), dim3(256), 0, c->stream,
                       x_dev, c->d_x.p, c->n, c->m, c->l, c->sub.jb0, c->sub.ib0, c->sub.nx, c->sub.nloc);
    HIP_OK(hipGetLastError());
    c->jac_valid = 0;
    return 0;
}
extern "C" int iemic_get_state(iemic_ctx* c, double* x)
{
    CTX_CHECK(c);
    return get_ref(c, c->d_x.p, x);
}
