/*
 * capi_time.hip -- the C ABI's timing probes (what bench.py and the profiling scripts read):
 * the SpMV kernel warm and cold, the block product of the projected model, the preconditioner
 * apply and its parts.
 */
#include <chrono>

#include "capi_internal.h"

using namespace iemic;

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

/* mean duration of the block product J V of k columns alone (spmm_kernel: the k_spmm7 launches
 * and, with SRES = 0, the dense row's multi-dot), HIP events on its stream; the columns are
 * copies of the state, halo rows filled by the warm-up SpMV */
extern "C" int iemic_time_spmm(iemic_ctx* c, int k, int nrep, double* ms_per_product)
{
    CTX_CHECK(c);
    if (!c->jac_valid || nrep < 1 || !ms_per_product) return IEMIC_ESTATE;
    if (k < 1 || k > SPMM_MAX_K) {
        set_error("iemic_time_spmm: k = " + std::to_string(k) + " is outside 1 .. " + std::to_string(SPMM_MAX_K));
        return IEMIC_EINVAL;
    }
    const size_t NE = (size_t)c->sub.nerows();
    DevBuf<double> V, W;
    if (V.alloc(NE * k) || W.alloc(NE * k)) {
        set_error("iemic_time_spmm: out of device memory");
        return IEMIC_ENOMEM;
    }
    EventPair ev;
    if (ev.create()) {
        set_error("hipEventCreate failed");
        return IEMIC_EDEVICE;
    }
    int rc = spmv(c, c->d_x.p, c->d_tmp2.p, c->stream); /* fills the state's halo */
    if (rc) return rc;
    for (int b = 0; b < k; b++)
        HIP_OK(hipMemcpyAsync(V.p + b * NE, c->d_x.p, sizeof(double) * NE, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = spmm_kernel(c, V.p, (int64_t)NE, k, W.p, (int64_t)NE, c->pj.kbmax))) return rc;   /* warm */
    HIP_OK(hipEventRecord(ev.a, c->stream));
    for (int r = 0; r < nrep; r++)
        if ((rc = spmm_kernel(c, V.p, (int64_t)NE, k, W.p, (int64_t)NE, c->pj.kbmax))) return rc;
    HIP_OK(hipEventRecord(ev.b, c->stream));
    DEV_WAIT_EVENT(c, ev.b);
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, ev.a, ev.b));
    *ms_per_product = ms / nrep;
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
