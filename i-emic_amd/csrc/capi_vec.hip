/*
 * capi_vec.hip -- the C ABI's device vectors: the Epetra_Vector algebra Continuation.H applies
 * through Utils (dot / norm / update over the solve map), on vectors in the ext layout; the
 * owned rows are one contiguous slab, reductions are summed over the ranks.
 */
#include <algorithm>

#include "capi_internal.h"

using namespace iemic;

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
         q += (int64_t)gridDim.x * blockDim.x)
        v = nanmax(v, fabs(x[q]));                      /* NaN propagates */
    v = block_nanmax(v, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
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
    const auto [o, NL, G] = owned(c);
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
    const Owned w = owned(c);
    const int nb = (int)std::min<int64_t>((w.n + 255) / 256, RED_BLOCKS);
    hipLaunchKernelGGL(k_vec_absmax, dim3(nb), dim3(256), 0, c->stream, x + w.o, w.n, c->d_part.p);
    HIP_OK(hipGetLastError());
    double mx = 0.0;
    int rc = part_nanmax(c, nb, &mx);
    if (!rc) rc = host_max(c, &mx);
    if (rc) return rc;
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
    const Owned w = owned(c);
    if (set) {
        HIP_OK(hipMemcpyAsync(c->d_x.p + w.o, v + w.o, sizeof(double) * w.n, hipMemcpyDeviceToDevice, c->stream));
        c->jac_valid = 0;
    } else {
        HIP_OK(hipMemcpyAsync(v + w.o, c->d_x.p + w.o, sizeof(double) * w.n, hipMemcpyDeviceToDevice, c->stream));
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
    const Owned w = owned(c);
    if (F != c->d_F.p)
        HIP_OK(hipMemcpyAsync(F + w.o, c->d_F.p + w.o, sizeof(double) * w.n, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}
