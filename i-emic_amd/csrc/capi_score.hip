/*
 * capi_score.hip -- the C ABI of the rare-event score function (score.hip): the reference states
 * come in as host vectors in the reference's row order, the evaluated vector is a device vector
 * or the resident state.
 */
#include <cmath>

#include "capi_internal.h"

using namespace iemic;

static int finite_ref(const iemic_ctx* c, const double* v, const char* name)
{
    for (int64_t q = 0; q < c->nrows; q++)
        if (!std::isfinite(v[q])) {
            set_error(std::string("iemic_score_set: ") + name + "[" + std::to_string(q) + "] is not finite");
            return IEMIC_EINVAL;
        }
    return 0;
}

/* get_default_score_function / get_ocean_score_function up to the returned lambda
 * (ScoreFunctions.C:40-51, :145-161): nrm and dist_factor; sol3 may be NULL */
extern "C" int iemic_score_set(iemic_ctx* c, const double* sol1, const double* sol2, const double* sol3, int var)
{
    CTX_CHECK(c);
    c->sc.set = 0;                                     /* a refused call leaves no score function set */
    if (!sol1 || !sol2) {
        set_error("iemic_score_set: sol1 or sol2 is NULL");
        return IEMIC_EINVAL;
    }
    if (var < -1 || var >= NUN) {
        set_error("iemic_score_set: var = " + std::to_string(var) + " is outside -1 .. " + std::to_string(NUN - 1));
        return IEMIC_EINVAL;
    }
    int rc = finite_ref(c, sol1, "sol1");
    if (!rc) rc = finite_ref(c, sol2, "sol2");
    if (!rc && sol3) rc = finite_ref(c, sol3, "sol3");
    if (rc) return rc;
    const size_t NE = (size_t)c->sub.nerows();
    DevBuf<double> d1, d2, d3;
    if (d1.alloc(NE) || d2.alloc(NE) || (sol3 && d3.alloc(NE))) {
        set_error("iemic_score_set: out of device memory");
        return IEMIC_ENOMEM;
    }
    if ((rc = put_ref(c, sol1, d1.p)) || (rc = put_ref(c, sol2, d2.p)) || (sol3 && (rc = put_ref(c, sol3, d3.p))))
        return rc;
    rc = score_set(c, d1.p, d2.p, sol3 ? d3.p : nullptr, var);
    DEV_SYNC(c);                                       /* the copies out of d1, d2 are done */
    return rc;
}

extern "C" int iemic_score_get(iemic_ctx* c, double* nrm, double* dist_factor)
{
    CTX_CHECK(c);
    if (!c->sc.set) {
        set_error("iemic_score_get: no score function set (iemic_score_set)");
        return IEMIC_ESTATE;
    }
    if (nrm) *nrm = c->sc.nrm;
    if (dist_factor) *dist_factor = c->sc.dist_factor;
    return 0;
}

/* the returned lambda (ScoreFunctions.C:53-65, :163-189) on a device vector, or on the state */
extern "C" int iemic_score(iemic_ctx* c, const double* v, double* dist, double* d1, double* d2)
{
    CTX_CHECK(c);
    return score_eval(c, v, dist, d1, d2);
}

extern "C" int iemic_score_clear(iemic_ctx* c)
{
    CTX_CHECK(c);
    DEV_SYNC(c);
    return score_clear(c);
}

/* dot(V, V) / dot(Vvvec, Vvvec) of the projected score functions (ScoreFunctions.C:77, :204-213) */
extern "C" int iemic_proj_gram_vv(iemic_ctx* c, int var, double* out)
{
    CTX_CHECK(c);
    if (!out) return IEMIC_EINVAL;
    return proj_gram_vv(c, var, out);
}
