/*
 * capi.hip -- the C ABI (include/iemic.h): context set-up and the Newton step.
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
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "common.h"

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

#define CTX_CHECK(c)                                   \
    if (!(c)) return IEMIC_EINVAL;                     \
    if (hipSetDevice((c)->device) != hipSuccess) {     \
        set_error("hipSetDevice failed");              \
        return IEMIC_EDEVICE;                          \
    }                                                  \
    StreamGuard stream_guard_{(c)}

namespace {
/* host reference-ordered global vector -> ext layout on the device (owned rows; halo 0) */
int put_ref(iemic_ctx* c, const double* ref, double* dev)
{
    std::vector<double> e((size_t)c->sub.nerows(), 0.0);
    c->su.ref_to_ext(ref, e.data());
    return h2d(c, dev, e.data(), sizeof(double) * e.size());
}
/* ext layout on the device -> owned rows of a host reference-ordered global vector */
int get_ref(iemic_ctx* c, const double* dev, double* ref)
{
    std::vector<double> e((size_t)c->sub.nerows());
    int rc = d2h(c, e.data(), dev, sizeof(double) * e.size());
    if (rc) return rc;
    c->su.ext_to_ref(e.data(), ref);
    return 0;
}
}  // namespace

namespace iemic {
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

/* ---- diagnostics of the state (host side, as in the reference) --------------------- */
/* THCM::getIntCondCoeff (THCM.C:2549-2577): the integral-condition coefficients */
extern "C" int iemic_get_intcond_coeff(iemic_ctx* c, double* out)
{
    CTX_CHECK(c);
    if (!out) return IEMIC_EINVAL;
    return get_ref(c, c->d_intc.p, out);
}

namespace {
/* the current state on the host in the ext layout with its HALO rows refreshed (the
 * reference's Solve2Assembly import before usol) */
int host_state(iemic_ctx* c, std::vector<double>& x)
{
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    x.assign((size_t)c->sub.nerows(), 0.0);
    return d2h(c, x.data(), c->d_x.p, sizeof(double) * x.size());
}
/* sum of a host array over the ranks */
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
/* max over the ranks (NaN propagates): each rank's value in its own slot, summed */
int host_max(iemic_ctx* c, double* mx)
{
    if (c->sub.nranks <= 1) return 0;
    std::vector<double> all((size_t)c->sub.nranks, 0.0);
    all[(size_t)c->sub.rank] = *mx;
    int rc = host_sum(c, all);
    if (rc) return rc;
    *mx = 0.0;
    for (double v : all) *mx = (v > *mx || v != v) ? v : *mx;
    return 0;
}
}  // namespace

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

extern "C" int iemic_jacobian(iemic_ctx* c)
{
    CTX_CHECK(c);
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    if ((rc = assemble_jacobian(c, c->d_x.p))) return rc;
    DEV_SYNC(c);
    return 0;
}

extern "C" int iemic_rhs(iemic_ctx* c, double* F)
{
    CTX_CHECK(c);
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    if ((rc = assemble_rhs(c, c->d_x.p, c->d_F.p))) return rc;
    if (F) return get_ref(c, c->d_F.p, F);
    DEV_SYNC(c);
    return 0;
}

extern "C" int iemic_diag_b(iemic_ctx* c, double* B)
{
    CTX_CHECK(c);
    if (!c->jac_valid) return IEMIC_ESTATE;
    return get_ref(c, c->d_B.p, B);
}

extern "C" int iemic_export_csr(iemic_ctx* c, int64_t* rowptr, int* col, double* val)
{
    CTX_CHECK(c);
    if (!c->jac_valid) {
        set_error("iemic_export_csr: no Jacobian assembled");
        return IEMIC_ESTATE;
    }
    std::vector<double> v((size_t)NSLOT * c->sub.nloc);
    int rc = d2h(c, v.data(), c->d_val.p, sizeof(double) * v.size());
    if (rc) return rc;
    c->su.to_csr(v.data(), rowptr, col, val);
    return 0;
}

extern "C" int iemic_spmv(iemic_ctx* c, const double* x, double* y)
{
    CTX_CHECK(c);
    int rc = put_ref(c, x, c->d_tmp1.p);
    if (rc) return rc;
    if ((rc = spmv(c, c->d_tmp1.p, c->d_tmp2.p, c->stream))) return rc;
    return get_ref(c, c->d_tmp2.p, y);
}

extern "C" int iemic_spmv_dev(iemic_ctx* c, double* x, double* y, void*)
{
    CTX_CHECK(c);
    return spmv(c, x, y, c->stream);
}

extern "C" int iemic_prec_compute(iemic_ctx* c, const iemic_krylov* opt)
{
    CTX_CHECK(c);
    int rc = prec_compute(c, opt);
    if (rc) return rc;
    DEV_SYNC(c);
    return 0;
}

extern "C" int iemic_prec_apply(iemic_ctx* c, const double* r, double* z)
{
    CTX_CHECK(c);
    int rc = put_ref(c, r, c->d_tmp1.p);
    if (rc) return rc;
    if ((rc = prec_apply(c, c->d_tmp1.p, c->d_tmp2.p))) return rc;
    return get_ref(c, c->d_tmp2.p, z);
}

extern "C" int iemic_solve_dev(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt,
                               iemic_solve_info* info)
{
    CTX_CHECK(c);
    if (!opt) return IEMIC_EINVAL;
    return krylov_solve(c, b, x, opt, info);
}

extern "C" int iemic_solve(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt,
                           iemic_solve_info* info)
{
    CTX_CHECK(c);
    if (!opt || !b || !x) return IEMIC_EINVAL;
    DevBuf<double> db, dx;
    if (db.alloc(c->sub.nerows()) || dx.alloc(c->sub.nerows())) return IEMIC_ENOMEM;
    int rc = put_ref(c, b, db.p);
    if (rc) return rc;
    if ((rc = krylov_solve(c, db.p, dx.p, opt, info))) return rc;
    return get_ref(c, dx.p, x);
}

namespace iemic {
__global__ void k_newton_update(double* __restrict__ x, const double* __restrict__ dx, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        x[q] += dx[q];
}
__global__ void k_neg(const double* __restrict__ a, double* __restrict__ b, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x)
        b[q] = -a[q];
}
}  // namespace iemic

/* transient/Newton.H:92-99: F, J, solve J dx = -F, x += dx, F */
extern "C" int iemic_newton_step(iemic_ctx* c, const iemic_krylov* opt, iemic_newton_info* info)
{
    CTX_CHECK(c);
    if (!opt) return IEMIC_EINVAL;
    iemic_newton_info inf{};
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    auto T0 = clk::now();
    const int64_t o = NUN * c->sub.own0, NL = c->sub.nlrows();
    const unsigned G = (unsigned)std::min<int64_t>((NL + 255) / 256, 2048);
    auto t = clk::now();
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    if ((rc = assemble_rhs(c, c->d_x.p, c->d_F.p))) return rc;
    DEV_SYNC(c);
    inf.t_rhs_ms += ms(t);
    inf.norm_f0 = std::sqrt(dot(c, c->d_F.p, c->d_F.p, 0));   /* NaN stays NaN */
    t = clk::now();
    if ((rc = assemble_jacobian(c, c->d_x.p))) return rc;
    DEV_SYNC(c);
    inf.t_jac_ms = ms(t);
    t = clk::now();
    if (opt->prec > 0) {
        if ((rc = prec_compute(c, opt))) return rc;
        DEV_SYNC(c);
    }
    inf.t_prec_ms = ms(t);
    hipLaunchKernelGGL(k_neg, dim3(G), dim3(256), 0, c->stream, c->d_F.p + o, c->d_tmp1.p + o, NL);
    t = clk::now();
    if ((rc = krylov_solve(c, c->d_tmp1.p, c->d_tmp2.p, opt, &inf.solve))) return rc;
    DEV_SYNC(c);
    inf.t_solve_ms = ms(t);
    hipLaunchKernelGGL(k_newton_update, dim3(G), dim3(256), 0, c->stream, c->d_x.p + o, c->d_tmp2.p + o, NL);
    t = clk::now();
    if ((rc = halo_exchange(c, c->d_x.p, HALO))) return rc;
    if ((rc = assemble_rhs(c, c->d_x.p, c->d_F.p))) return rc;
    DEV_SYNC(c);
    inf.t_rhs_ms += ms(t);
    inf.norm_f1 = std::sqrt(dot(c, c->d_F.p, c->d_F.p, 0));   /* NaN stays NaN */
    c->jac_valid = 1;
    inf.t_total_ms = ms(T0);
    if (info) *info = inf;
    /* Newton.H applies the update whatever the solver reported; the caller learns that the
     * solve missed its tolerance from a distinct status */
    return inf.solve.converged ? 0 : IEMIC_ENOCONV;
}

/* ---- the theta time stepper (theta.hip) ------------------------------------------------ */
/* ThetaModel::initStep (ThetaModel.H:64-74) */
extern "C" int iemic_theta_init_step(iemic_ctx* c, double dt, double theta)
{
    CTX_CHECK(c);
    return theta_init_step(c, dt, theta);
}

/* ThetaModel::computeRHS (ThetaModel.H:87-113) */
extern "C" int iemic_theta_rhs(iemic_ctx* c, double* F)
{
    CTX_CHECK(c);
    int rc = theta_rhs(c);
    if (rc) return rc;
    if (F) return get_ref(c, c->th.Ft.p, F);
    DEV_SYNC(c);
    return 0;
}

/* ThetaModel::computeJacobian (ThetaModel.H:118-146) */
extern "C" int iemic_theta_jacobian(iemic_ctx* c)
{
    CTX_CHECK(c);
    int rc = theta_jacobian(c);
    if (rc) return rc;
    DEV_SYNC(c);
    return 0;
}

/* AdaptiveTransient.H:107 after a failed Newton run: the model is set back to x_n */
extern "C" int iemic_theta_restore(iemic_ctx* c)
{
    CTX_CHECK(c);
    return theta_restore(c);
}

/* one iteration of Newton.H:92-99 on the theta model: F_theta, J2, solve J2 dx = F_theta / dt /
 * theta (ThetaModel.H:150-164), x -= dx, F_theta */
extern "C" int iemic_theta_newton_step(iemic_ctx* c, const iemic_krylov* opt, int refactor,
                                       iemic_theta_info* info)
{
    CTX_CHECK(c);
    if (!opt) return IEMIC_EINVAL;
    iemic_theta_info inf{};
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
    auto T0 = clk::now();
    auto t = clk::now();
    int rc = theta_rhs(c);
    if (rc) return rc;
    DEV_SYNC(c);
    inf.t_rhs_ms += ms(t);
    inf.norm_f0 = std::sqrt(dot(c, c->th.Ft.p, c->th.Ft.p, 0));   /* NaN stays NaN */
    t = clk::now();
    if ((rc = theta_jacobian(c))) return rc;
    DEV_SYNC(c);
    inf.t_jac_ms = ms(t);
    t = clk::now();
    if (opt->prec > 0 && (refactor || !c->gs.ready)) {
        if ((rc = prec_compute(c, opt))) return rc;
        DEV_SYNC(c);
    }
    inf.t_prec_ms = ms(t);
    t = clk::now();
    if ((rc = krylov_solve(c, c->th.b.p, c->d_tmp2.p, opt, &inf.solve))) return rc;
    DEV_SYNC(c);
    inf.t_solve_ms = ms(t);
    if ((rc = theta_update(c, c->d_tmp2.p, &inf.norm_dx))) return rc;
    if ((rc = host_max(c, &inf.norm_dx))) return rc;
    t = clk::now();
    if ((rc = theta_rhs(c))) return rc;
    DEV_SYNC(c);
    inf.t_rhs_ms += ms(t);
    inf.norm_f1 = std::sqrt(dot(c, c->th.Ft.p, c->th.Ft.p, 0));
    c->jac_valid = 1;
    inf.t_total_ms = ms(T0);
    if (info) *info = inf;
    /* as iemic_newton_step: the update is applied whatever the solver reported */
    return inf.solve.converged ? 0 : IEMIC_ENOCONV;
}

/* ---- linear stability analysis (eigs.hip): the JDQZInterface seam ------------------------ */
/* Ocean::computeJacobian + the operator-side shift of JDQZInterface.H (alpha A - beta B) */
extern "C" int iemic_shifted_jacobian(iemic_ctx* c, double sigma)
{
    CTX_CHECK(c);
    int rc = shifted_jacobian(c, sigma);
    if (rc) return rc;
    DEV_SYNC(c);
    return 0;
}

/* JDQZ's construction on the model (run_ocean.C:82-97) */
extern "C" int iemic_eigs_begin(iemic_ctx* c, double sigma, int m, uint64_t seed, const iemic_krylov* opt)
{
    CTX_CHECK(c);
    if (!opt) return IEMIC_EINVAL;
    return eigs_begin(c, sigma, m, seed, opt);
}

/* one operator application of the eigen-iteration: applyMassMat, then the shifted solve */
extern "C" int iemic_eigs_step(iemic_ctx* c, const iemic_krylov* opt, double* hcol, iemic_eigs_info* info)
{
    CTX_CHECK(c);
    if (!opt || !hcol) return IEMIC_EINVAL;
    return eigs_step(c, opt, hcol, info);
}

/* the eigenvectors JDQZ hands to Utils::saveEigenvectors (Continuation.H:1116-1120) */
extern "C" int iemic_eigs_ritz(iemic_ctx* c, int j, int p, const double* Y, void** xvecs)
{
    CTX_CHECK(c);
    if (!c->eg.active || j > c->eg.j + (c->eg.broke ? 0 : 1)) {
        set_error("iemic_eigs_ritz: the run holds fewer than j basis vectors (iemic_eigs_begin, iemic_eigs_step)");
        return IEMIC_ESTATE;
    }
    if (!xvecs || p < 1 || p > 16) {
        set_error("iemic_eigs_ritz: needs 1 <= p <= 16 output vectors");
        return IEMIC_EINVAL;
    }
    const int64_t o = NUN * c->sub.own0;
    double* xs[16];
    for (int q = 0; q < p; q++) xs[q] = xvecs[q] ? (double*)xvecs[q] + o : nullptr;
    return eigs_ritz(c, c->eg.V.p + o, c->sub.nerows(), j, p, Y, xs, c->sub.nlrows());
}

/* the residual JDQZ reports per converged pair, measured on the operator itself */
extern "C" int iemic_eigs_residual(iemic_ctx* c, double lam_re, double lam_im, double* x_re, double* x_im,
                                   double out[2])
{
    CTX_CHECK(c);
    return eigs_residual(c, lam_re, lam_im, x_re, x_im, out);
}

extern "C" int iemic_eigs_end(iemic_ctx* c)
{
    CTX_CHECK(c);
    DEV_SYNC(c);
    return eigs_end(c);
}

/* ---- device vectors: the Epetra_Vector algebra Continuation.H applies through Utils
 * (dot / norm / update over the solve map), on vectors in the ext layout; the owned rows
 * are one contiguous slab, reductions are summed over the ranks ------------------------ */
namespace iemic {
__global__ void k_vec_update(double a, const double* __restrict__ x, double b, const double* __restrict__ y,
                             double cz, double* __restrict__ z, int64_t N)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        double v = a * x[q];
        if (y) v += b * y[q];
        if (cz != 0.0) v += cz * z[q];
        z[q] = v;
    }
}
__global__ void __launch_bounds__(256) k_vec_absmax(const double* __restrict__ x, int64_t N,
                                                    double* __restrict__ part)
{
    __shared__ double sm[4];
    double v = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        const double a = fabs(x[q]);
        v = (a > v || a != a) ? a : v;                  /* NaN propagates */
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_down(v, o, 64);
        v = (u > v || u != u) ? u : v;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sm[0];
        for (int w = 1; w < 4; w++) t = (sm[w] > t || sm[w] != sm[w]) ? sm[w] : t;
        part[blockIdx.x] = t;
    }
}
}  // namespace iemic

extern "C" int iemic_vec_alloc(iemic_ctx* c, double** v)
{
    CTX_CHECK(c);
    if (!v) return IEMIC_EINVAL;
    *v = nullptr;
    if (hipMalloc((void**)v, sizeof(double) * c->sub.nerows()) != hipSuccess) {
        *v = nullptr;
        set_error("iemic_vec_alloc: out of device memory");
        return IEMIC_ENOMEM;
    }
    HIP_OK(hipMemsetAsync(*v, 0, sizeof(double) * c->sub.nerows(), c->stream));
    return 0;
}

extern "C" int iemic_vec_free(iemic_ctx* c, double* v)
{
    CTX_CHECK(c);
    if (v) HIP_OK(hipFree(v));
    return 0;
}

extern "C" int iemic_vec_update(iemic_ctx* c, double a, const double* x, double b, const double* y, double cz,
                                double* z)
{
    CTX_CHECK(c);
    if (!x || !z) return IEMIC_EINVAL;
    const int64_t o = NUN * c->sub.own0, NL = c->sub.nlrows();
    const unsigned G = (unsigned)std::min<int64_t>((NL + 255) / 256, 2048);
    hipLaunchKernelGGL(k_vec_update, dim3(G), dim3(256), 0, c->stream, a, x + o, b, y ? y + o : nullptr, cz,
                       z + o, NL);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int iemic_vec_dot(iemic_ctx* c, const double* x, const double* y, double* out)
{
    CTX_CHECK(c);
    if (!x || !y || !out) return IEMIC_EINVAL;
    return dot_owned(c, x, y, out);
}

extern "C" int iemic_vec_norm_inf(iemic_ctx* c, const double* x, double* out)
{
    CTX_CHECK(c);
    if (!x || !out) return IEMIC_EINVAL;
    const int64_t o = NUN * c->sub.own0, NL = c->sub.nlrows();
    const int nb = (int)std::min<int64_t>((NL + 255) / 256, RED_BLOCKS);
    hipLaunchKernelGGL(k_vec_absmax, dim3(nb), dim3(256), 0, c->stream, x + o, NL, c->d_part.p);
    HIP_OK(hipGetLastError());
    std::vector<double> part(nb);
    int rc = d2h(c, part.data(), c->d_part.p, sizeof(double) * nb);
    if (rc) return rc;
    double mx = 0.0;
    for (double v : part) mx = (v > mx || v != v) ? v : mx;
    if ((rc = host_max(c, &mx))) return rc;
    *out = mx;
    return 0;
}

extern "C" int iemic_vec_from_ref(iemic_ctx* c, const double* ref, double* v)
{
    CTX_CHECK(c);
    if (!ref || !v) return IEMIC_EINVAL;
    return put_ref(c, ref, v);
}

extern "C" int iemic_vec_to_ref(iemic_ctx* c, const double* v, double* ref)
{
    CTX_CHECK(c);
    if (!ref || !v) return IEMIC_EINVAL;
    return get_ref(c, v, ref);
}

/* set = 0: v = state; set = 1: state = v (owned rows; halos are refreshed before use) */
extern "C" int iemic_state_vec(iemic_ctx* c, double* v, int set)
{
    CTX_CHECK(c);
    if (!v) return IEMIC_EINVAL;
    const int64_t o = NUN * c->sub.own0;
    if (set) {
        HIP_OK(hipMemcpyAsync(c->d_x.p + o, v + o, sizeof(double) * c->sub.nlrows(), hipMemcpyDeviceToDevice,
                              c->stream));
        c->jac_valid = 0;
    } else {
        HIP_OK(hipMemcpyAsync(v + o, c->d_x.p + o, sizeof(double) * c->sub.nlrows(), hipMemcpyDeviceToDevice,
                              c->stream));
    }
    return 0;
}

/* F(state) into the device vector F (owned rows) */
extern "C" int iemic_rhs_vec(iemic_ctx* c, double* F)
{
    CTX_CHECK(c);
    if (!F) return IEMIC_EINVAL;
    int rc = halo_exchange(c, c->d_x.p, HALO);
    if (rc) return rc;
    if ((rc = assemble_rhs(c, c->d_x.p, c->d_F.p))) return rc;
    const int64_t o = NUN * c->sub.own0;
    if (F != c->d_F.p)
        HIP_OK(hipMemcpyAsync(F + o, c->d_F.p + o, sizeof(double) * c->sub.nlrows(), hipMemcpyDeviceToDevice,
                              c->stream));
    return 0;
}

/* mean duration of the SpMV kernel alone (no halo exchange), HIP events on its stream */
extern "C" int iemic_time_spmv(iemic_ctx* c, int nrep, double* ms_per_launch)
{
    CTX_CHECK(c);
    if (!c->jac_valid || nrep < 1) return IEMIC_ESTATE;
    EventPair ev;
    if (ev.create()) {
        set_error("hipEventCreate failed");
        return IEMIC_EDEVICE;
    }
    hipEvent_t e0 = ev.a, e1 = ev.b;
    int rc = spmv(c, c->d_x.p, c->d_tmp2.p, c->stream); /* warm, fills the halo */
    if (rc) return rc;
    HIP_OK(hipEventRecord(e0, c->stream));
    for (int r = 0; r < nrep; r++) {
        rc = spmv_kernel(c, c->d_x.p, c->d_tmp2.p);
        if (rc) return rc;
    }
    HIP_OK(hipEventRecord(e1, c->stream));
    DEV_WAIT_EVENT(c, e1);
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_launch = ms / nrep;
    return 0;
}

extern "C" int iemic_time_prec(iemic_ctx* c, int nrep, double* ms_per_apply, double* host_ms_per_apply)
{
    CTX_CHECK(c);
    if (!c->gs.ready || nrep < 1 || !ms_per_apply || !host_ms_per_apply) return IEMIC_ESTATE;
    EventPair ev;
    if (ev.create()) {
        set_error("hipEventCreate failed");
        return IEMIC_EDEVICE;
    }
    hipEvent_t e0 = ev.a, e1 = ev.b;
    HIP_OK(hipMemsetAsync(c->d_tmp1.p, 0, sizeof(double) * c->sub.nerows(), c->stream));
    int rc = prec_apply(c, c->d_tmp1.p, c->d_tmp2.p);   /* warm */
    if (rc) return rc;
    DEV_SYNC(c);
    const auto t0 = std::chrono::steady_clock::now();
    HIP_OK(hipEventRecord(e0, c->stream));
    for (int r = 0; r < nrep && !rc; r++) rc = prec_apply(c, c->d_tmp1.p, c->d_tmp2.p);
    HIP_OK(hipEventRecord(e1, c->stream));
    const double host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    DEV_WAIT_EVENT(c, e1);
    if (rc) return rc;
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    *ms_per_apply = ms / nrep;
    *host_ms_per_apply = host / nrep;
    return 0;
}

namespace iemic {
int gs_time_parts(iemic_ctx* c, int nrep, double* us);
}
/* GPU microseconds of the block GS apply's parts (gs_time_parts): Schur solve, T/S block
 * solve, one dynamics pass, one dynamics defect */
extern "C" int iemic_time_prec_parts(iemic_ctx* c, int nrep, double* us4)
{
    CTX_CHECK(c);
    if (!us4) return IEMIC_EINVAL;
    return gs_time_parts(c, nrep, us4);
}

/* streaming read of a scratch buffer (evicts the Infinity Cache without leaving dirty
 * lines behind, which a memset would); the store never happens for finite data */
__global__ void k_flush_read(const double2* __restrict__ a, int64_t n2, double* __restrict__ sink)
{
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2;
         i += (int64_t)gridDim.x * blockDim.x) {
        const double2 v = a[i];
        s += v.x + v.y;
    }
    if (s == 1.2345e300) sink[0] = s;
}

/* Cold-cache SpMV timing: before every launch the stream reads `flush_bytes` of the
 * device buffer `flush` (larger than the 256 MiB Infinity Cache), so each launch reads the
 * Jacobian from HBM as it does inside FGMRES (where the basis passes evict it); only the
 * SpMV launches sit between the events. */
extern "C" int iemic_time_spmv_cold(iemic_ctx* c, int nrep, void* flush, int64_t flush_bytes,
                                    double* ms_per_launch)
{
    CTX_CHECK(c);
    if (!c->jac_valid || nrep < 1 || !flush || flush_bytes <= 0) return IEMIC_EINVAL;
    EventPair ev;
    if (ev.create()) {
        set_error("hipEventCreate failed");
        return IEMIC_EDEVICE;
    }
    hipEvent_t e0 = ev.a, e1 = ev.b;
    int rc = spmv(c, c->d_x.p, c->d_tmp2.p, c->stream);
    if (rc) return rc;
    double tot = 0.0;
    for (int r = 0; r < nrep; r++) {
        hipLaunchKernelGGL(k_flush_read, dim3(4096), dim3(256), 0, c->stream, (const double2*)flush,
                           flush_bytes / 16, c->d_tmp1.p);
        HIP_OK(hipEventRecord(e0, c->stream));
        if ((rc = spmv_kernel(c, c->d_x.p, c->d_tmp2.p))) return rc;
        HIP_OK(hipEventRecord(e1, c->stream));
        DEV_WAIT_EVENT(c, e1);
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        tot += ms;
    }
    *ms_per_launch = tot / nrep;
    return 0;
}
