/*
 * capi_internal.h -- what the units of the C ABI share (capi.hip, capi_diag.hip, capi_vec.hip,
 * capi_time.hip, newton.hip): the entry check of every call that takes a context, and the
 * host-side transfers between the reference's row order and the ext layout.  Included by
 * nothing else.
 */
#ifndef IEMIC_CAPI_INTERNAL_H
#define IEMIC_CAPI_INTERNAL_H

#include "common.h"

#define CTX_CHECK(c)                                   \
    if (!(c)) return IEMIC_EINVAL;                     \
    if (hipSetDevice((c)->device) != hipSuccess) {     \
        set_error("hipSetDevice failed");              \
        return IEMIC_EDEVICE;                          \
    }                                                  \
    StreamGuard stream_guard_{(c)}

namespace iemic {
/* capi.hip */
/* host reference-ordered global vector -> ext layout on the device (owned rows; halo 0) */
int put_ref(iemic_ctx* c, const double* ref, double* dev);
/* ext layout on the device -> owned rows of a host reference-ordered global vector */
int get_ref(iemic_ctx* c, const double* dev, double* ref);
/* capi_diag.hip */
/* the current state on the host in the ext layout with its HALO rows refreshed (the
 * reference's Solve2Assembly import before usol) */
int host_state(iemic_ctx* c, std::vector<double>& x);
/* sum of a host array over the ranks */
int host_sum(iemic_ctx* c, std::vector<double>& v);
/* max over the ranks (NaN propagates): each rank's value in its own slot, summed */
int host_max(iemic_ctx* c, double* mx);
}  // namespace iemic

#endif
