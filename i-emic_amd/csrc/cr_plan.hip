/*
 * cr_plan.hip -- the plan of the block cyclic reduction (schur_cr.hip), host code, once per
 * grid: level sizes and storage, the GEMM descriptors of the set-up (cr_factor.hip), the
 * dense tail, and the apply steps -- the level operations as block expressions, composed two
 * levels at a time, packed into the workgroup descriptors k_cr_pk reads.
 */
#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "cr_internal.h"

namespace iemic {

/* ---- apply steps: the level operations as block expressions, composed two levels at a time.
 * Composing level l with level l + 1 (the down step b_l -> b_{l+2}, the
 * up step x_{l+2} -> x_l) halves the apply launches; the merged coefficients are materialised
 * once per factorisation (k_cr_comp). */
namespace {
/* A quantity (a block of a level vector) is a sum over leaves -- blocks of the right-hand
 * sides b_l or solutions x_l of other levels -- of coefficient matrices, each a sum of signed
 * products of at most two level operators */
using Leaf = std::tuple<int, int, int>;          /* (0: b / 1: x, level, block) */
struct Prod {
    double s;
    const double* A;                             /* null: identity */
    const double* B;                             /* null: none     */
};
using Expr = std::map<Leaf, std::vector<Prod>>;

/* b_{l+1}[q] over b_l (k_cr_fwd) */
Expr fwd_expr(const SchurCR& cr, int l, int q)
{
    const CrOps o = cr_ops(cr, l);
    const int e = 2 * q;
    const CrEven g = cr_even(cr.N[l], cr.per[l], e);
    Expr E;
    E[Leaf{0, l, e}].push_back({1.0, nullptr, nullptr});
    if (g.lo) E[Leaf{0, l, g.lnb}].push_back({-1.0, o.XL + q * o.mm, nullptr});
    if (g.ro) E[Leaf{0, l, g.rnb}].push_back({-1.0, o.XR + q * o.mm, nullptr});
    return E;
}
/* x_l[t] over x_{l+1} and b_l (k_cr_bwd; even blocks are copies) */
Expr bwd_expr(const SchurCR& cr, int l, int t)
{
    Expr E;
    if ((t & 1) == 0) {
        E[Leaf{1, l + 1, t / 2}].push_back({1.0, nullptr, nullptr});
        return E;
    }
    const CrOps o = cr_ops(cr, l);
    const int p = t / 2;
    const CrOdd g = cr_odd(cr.N[l], cr.per[l], t);
    E[Leaf{0, l, t}].push_back({1.0, o.Dinv + p * o.mm, nullptr});
    E[Leaf{1, l + 1, p}].push_back({-1.0, o.YL + p * o.mm, nullptr});
    if (g.rex) E[Leaf{1, l + 1, g.rn / 2}].push_back({-1.0, o.YR + p * o.mm, nullptr});
    return E;
}
/* dst += s M E  (E's coefficients single operators) */
void add_mul(Expr& dst, double s, const double* M, const Expr& E)
{
    for (const auto& kv : E)
        for (const Prod& p : kv.second) {
            Prod q{s * p.s, p.A, nullptr};
            if (M) {
                if (p.A) { q.A = M; q.B = p.A; }
                else q.A = M;
            }
            dst[kv.first].push_back(q);
        }
}
/* E with every leaf of (kind, level) replaced by sub(block) */
template <class F>
Expr substitute(const Expr& E, int kind, int level, F sub)
{
    Expr R;
    for (const auto& kv : E) {
        if (std::get<0>(kv.first) != kind || std::get<1>(kv.first) != level) {
            for (const Prod& p : kv.second) R[kv.first].push_back(p);
            continue;
        }
        const Expr S = sub(std::get<2>(kv.first));
        for (const Prod& p : kv.second) {
            if (p.B) return Expr{};              /* not composable (never: single operators) */
            add_mul(R, p.s, p.A, S);
        }
    }
    return R;
}
struct OutSpec {
    int kind, level, block;                      /* the output quantity */
    Expr e;
};
}  // namespace

/* the outputs of the apply step(s) for levels [l0, l0 + nl) (nl = 1 or 2), down or up */
static std::vector<OutSpec> step_outputs(const SchurCR& cr, int l0, int nl, bool down)
{
    std::vector<OutSpec> out;
    if (down) {
        if (nl == 1) {
            for (int q = 0; q < cr.N[l0 + 1]; q++) out.push_back({0, l0 + 1, q, fwd_expr(cr, l0, q)});
            return out;
        }
        for (int r = 0; r < cr.N[l0 + 2]; r++)
            out.push_back({0, l0 + 2, r, substitute(fwd_expr(cr, l0 + 1, r), 0, l0 + 1,
                                                    [&](int q) { return fwd_expr(cr, l0, q); })});
        for (int q = 1; q < cr.N[l0 + 1]; q += 2) out.push_back({0, l0 + 1, q, fwd_expr(cr, l0, q)});
        return out;
    }
    if (nl == 1) {
        for (int t = 0; t < cr.N[l0]; t++) out.push_back({1, l0, t, bwd_expr(cr, l0, t)});
        return out;
    }
    for (int t = 0; t < cr.N[l0]; t++)
        out.push_back({1, l0, t, substitute(bwd_expr(cr, l0, t), 1, l0 + 1,
                                            [&](int q) { return bwd_expr(cr, l0 + 1, q); })});
    return out;
}

/* the packed form of one apply step (CrStep): 8 rows per chunk (16 measured 1.3 ms slower per
 * Newton step at 2 degrees, scripts/ab/cr_rc8.sh), fewer where the step would have < 448
 * workgroups (the small steps of the deep levels would leave CUs idle), the workgroups
 * sorted by matrix-term count into classes, the set-up copy jobs */
static int cr_pack_step(iemic_ctx* c, const SchurCR& cr, const std::vector<CrOut>& outs, CrStep& st)
{
    const int m = cr.m;
    int rcw = 8;
    while (rcw > 4 && (int64_t)outs.size() * ((m + rcw - 1) / rcw) < 448) rcw /= 2;
    const int nch = (m + rcw - 1) / rcw;
    struct W { int nA, o, ch; };
    std::vector<W> ws;
    for (int o = 0; o < (int)outs.size(); o++) {
        int nA = 0, nid = 0;
        for (int t = 0; t < outs[o].nt; t++) {
            if (outs[o].A[t]) nA++;
            else if (outs[o].s[t] != 1.0 || ++nid > 1) {
                set_error("Schur cyclic reduction: unexpected identity term in an apply step");
                return IEMIC_EINVAL;
            }
        }
        for (int ch = 0; ch < nch; ch++) ws.push_back({nA, o, ch});
    }
    std::stable_sort(ws.begin(), ws.end(), [](const W& a, const W& b) { return a.nA > b.nA; });
    CrCls cls{};
    std::vector<CrWg> wg(ws.size());
    std::vector<CrPack> jobs;
    int64_t pos = 0;
    for (size_t w = 0; w < ws.size(); w++) {
        const W& q = ws[w];
        if (w == 0 || q.nA != ws[w - 1].nA) {
            if (cls.ncls == CR_NCLS) {
                set_error("Schur cyclic reduction: too many term classes in an apply step");
                return IEMIC_EINVAL;
            }
            cls.w0[cls.ncls] = (int)w;
            cls.nA[cls.ncls] = q.nA;
            cls.p0[cls.ncls] = pos;
            cls.ncls++;
        }
        const CrOut& o = outs[q.o];
        CrWg& d = wg[w];
        d.yref = cr_vref(o.yb, o.yo);
        d.r0 = q.ch * rcw;
        int v = 0, id = -1;
        for (int t = 0; t < o.nt; t++) {
            if (!o.A[t]) {
                id = t;
                continue;
            }
            d.vref[v++] = cr_vref(o.vb[t], o.vo[t]);
            jobs.push_back({o.A[t], o.s[t], pos, d.r0});
            pos += (int64_t)m * rcw;
        }
        d.hasid = id >= 0;
        if (id >= 0) d.vref[v++] = cr_vref(o.vb[id], o.vo[id]);
        d.nv = v;
    }
    cls.w0[cls.ncls] = (int)ws.size();
    st.nwg = (int)ws.size();
    st.rc = rcw;
    st.cls = cls;
    st.njobs = (int)jobs.size();
    if (st.wg.alloc(wg.size()) || st.P.alloc(std::max<int64_t>(pos, 1)) || st.jobs.alloc(std::max<size_t>(jobs.size(), 1))) {
        set_error("Schur cyclic reduction: out of device memory");
        return IEMIC_ENOMEM;
    }
    int rc = h2d(c, st.wg.p, wg.data(), sizeof(CrWg) * wg.size());
    if (!rc && !jobs.empty()) rc = h2d(c, st.jobs.p, jobs.data(), sizeof(CrPack) * jobs.size());
    return rc;
}

/* apply steps (descriptors) and the composite operators they need; two levels per step
 * where the composed step stays within CR_MT terms */
static int cr_build_steps(iemic_ctx* c, SchurCR& cr)
{
    const int m = cr.m;
    const size_t mm = (size_t)m * m;
    const int le = cr.tM ? cr.lt : cr.nlev;
    struct Plan { int l0, nl; std::vector<OutSpec> dn, up; };
    std::vector<Plan> plan;
    for (int l = 0; l < le;) {
        Plan P{l, std::min(2, le - l), {}, {}};
        P.dn = step_outputs(cr, l, P.nl, true);
        P.up = step_outputs(cr, l, P.nl, false);
        bool ok = true;
        for (const auto* v : {&P.dn, &P.up})
            for (const OutSpec& o : *v) {
                ok &= (int)o.e.size() <= CR_MT;
                for (const auto& kv : o.e) ok &= kv.second.size() <= 4;
            }
        if (!ok && P.nl == 2) {                  /* fall back to one level */
            P.nl = 1;
            P.dn = step_outputs(cr, l, 1, true);
            P.up = step_outputs(cr, l, 1, false);
        }
        l += P.nl;
        plan.push_back(std::move(P));
    }
    /* composite operators: coefficients that are not a single signed operator */
    std::vector<CrComp> comps;
    auto is_single = [](const std::vector<Prod>& v) { return v.size() == 1 && !v[0].B; };
    for (const Plan& P : plan)
        for (const auto* v : {&P.dn, &P.up})
            for (const OutSpec& o : *v)
                for (const auto& kv : o.e)
                    if (!is_single(kv.second)) comps.push_back(CrComp{});
    cr.ncomp = (int)comps.size();
    if (cr.ncomp && (cr.cmat.alloc(comps.size() * mm) || cr.cdesc.alloc(comps.size()))) {
        set_error("Schur cyclic reduction: out of device memory");
        return IEMIC_ENOMEM;
    }
    auto vref = [&](int kind, int level, int block, int& base, int64_t& off) {
        if (level == 0) { base = kind; off = (int64_t)block * m; }
        else { base = 2 + kind; off = (int64_t)cr.v_off[level] + (int64_t)block * m; }
    };
    size_t ic = 0;
    cr.down.clear();
    cr.up.clear();
    cr.down.resize(plan.size());
    cr.up.resize(plan.size());
    for (size_t ip = 0; ip < plan.size(); ip++) {
        const Plan& P = plan[ip];
        for (int dir = 0; dir < 2; dir++) {
            const std::vector<OutSpec>& specs = dir == 0 ? P.dn : P.up;
            std::vector<CrOut> outs;
            for (const OutSpec& o : specs) {
                CrOut d{};
                vref(o.kind, o.level, o.block, d.yb, d.yo);
                for (const auto& kv : o.e) {
                    const int t = d.nt++;
                    vref(std::get<0>(kv.first), std::get<1>(kv.first), std::get<2>(kv.first), d.vb[t], d.vo[t]);
                    if (is_single(kv.second)) {
                        d.s[t] = kv.second[0].s;
                        d.A[t] = kv.second[0].A;
                    } else {
                        CrComp& cc = comps[ic];
                        cc.C = cr.cmat.p + ic * mm;
                        cc.nt = (int)kv.second.size();
                        for (int k = 0; k < cc.nt; k++) {
                            cc.A[k] = kv.second[k].A;
                            cc.B[k] = kv.second[k].B;
                            cc.s[k] = kv.second[k].s;
                        }
                        d.s[t] = 1.0;
                        d.A[t] = cc.C;
                        ic++;
                    }
                }
                outs.push_back(d);
            }
            /* down steps top-first in plan order; up steps applied bottom-first (reverse) */
            CrStep& st = dir == 0 ? cr.down[ip] : cr.up[plan.size() - 1 - ip];
            st.nl = P.nl;
            int rc;
            if ((rc = cr_pack_step(c, cr, outs, st))) return rc;
        }
    }
    if (cr.ncomp) {
        int rc;
        if ((rc = h2d(c, cr.cdesc.p, comps.data(), sizeof(CrComp) * comps.size()))) return rc;
    }
    return 0;
}


/* ---- cr_init, step by step */

/* levels: blocks, periodic coupling and pair merge per level, and where each level's D/L/R
 * blocks, operators and vectors start; -> the doubles of cr.dlr, cr.ap and of cr.bv / cr.xv */
struct CrSizes {
    size_t nd, na, nv;
};
static CrSizes cr_levels(SchurCR& cr, int n, int m, int periodic)
{
    cr.n = n; cr.m = m; cr.periodic = periodic;
    cr.N.clear(); cr.per.clear(); cr.merge.clear();
    int N = n, P = periodic;
    while (N > 1) {
        const int mg = (N == 2 && P) ? 1 : 0;
        if (mg) P = 0;
        cr.N.push_back(N); cr.per.push_back(P); cr.merge.push_back(mg);
        N = (N + 1) / 2;
    }
    cr.N.push_back(1); cr.per.push_back(0); cr.merge.push_back(0);
    cr.nlev = (int)cr.N.size() - 1;
    const size_t mm = (size_t)m * m;
    cr.dlr_off.assign(cr.nlev + 1, 0);
    cr.ap_off.assign(cr.nlev + 1, 0);
    cr.v_off.assign(cr.nlev + 1, 0);
    CrSizes z{0, 0, 0};
    for (int l = 0; l <= cr.nlev; l++) {
        cr.dlr_off[l] = z.nd;
        z.nd += 3 * (size_t)cr.N[l] * mm;
        cr.ap_off[l] = z.na;
        z.na += l < cr.nlev ? cr_ops_blocks(cr.N[l]) * mm : mm;
        cr.v_off[l] = z.nv;
        if (l > 0) z.nv += (size_t)cr.N[l] * m;
    }
    return z;
}

static int cr_buffers(SchurCR& cr, const CrSizes& z)
{
    int rc = 0;
    rc |= cr.dlr.alloc(z.nd);
    rc |= cr.ap.alloc(z.na);
    rc |= cr.bv.alloc(std::max<size_t>(z.nv, 1));
    rc |= cr.xv.alloc(std::max<size_t>(z.nv, 1));
    rc |= cr.info.alloc(1);
    if (rc) {
        set_error("Schur cyclic reduction: out of device memory");
        return IEMIC_ENOMEM;
    }
    return 0;
}

/* the set-up's GEMM descriptors: per level the periodic-pair merge (g0), the X/Y products (g1)
 * and the next level's blocks (g2) */
static int cr_gemm_descriptors(iemic_ctx* c, SchurCR& cr)
{
    const size_t mm = (size_t)cr.m * cr.m;
    std::vector<CrGemm> g;
    cr.g_off.assign(3 * cr.nlev, 0);
    cr.g_cnt.assign(3 * cr.nlev, 0);
    auto blk = [&](int l, int which, int b) { return cr.dlr.p + cr.dlr_off[l] + ((size_t)which * cr.N[l] + b) * mm; };
    for (int l = 0; l < cr.nlev; l++) {
        const int Nl = cr.N[l], per = cr.per[l], ne = (Nl + 1) / 2, no = Nl / 2;
        const CrOps o = cr_ops(cr, l);
        auto XL = [&](int q) { return o.XL + q * mm; };
        auto XR = [&](int q) { return o.XR + q * mm; };
        auto DI = [&](int p) { return o.Dinv + p * mm; };
        auto YL = [&](int p) { return o.YL + p * mm; };
        auto YR = [&](int p) { return o.YR + p * mm; };
        const auto D = [&](int b) { return blk(l, 0, b); };
        const auto Lb = [&](int b) { return blk(l, 1, b); };
        const auto Rb = [&](int b) { return blk(l, 2, b); };
        cr.g_off[3 * l] = (int)g.size();
        if (cr.merge[l]) {
            g.push_back({Rb(0), Lb(0), Rb(0), nullptr, nullptr, nullptr, nullptr, 0.0, 0.0});
            g.push_back({Lb(1), Lb(1), Rb(1), nullptr, nullptr, nullptr, nullptr, 0.0, 0.0});
        }
        cr.g_cnt[3 * l] = (int)g.size() - cr.g_off[3 * l];
        cr.g_off[3 * l + 1] = (int)g.size();
        for (int q = 0; q < ne; q++) {
            const int e = 2 * q;
            const CrEven v = cr_even(Nl, per, e);
            if (v.lo) g.push_back({XL(q), nullptr, nullptr, Lb(e), DI(v.lnb / 2), nullptr, nullptr, 1.0, 0.0});
            if (v.ro) g.push_back({XR(q), nullptr, nullptr, Rb(e), DI(v.rnb / 2), nullptr, nullptr, 1.0, 0.0});
        }
        for (int p = 0; p < no; p++) {
            g.push_back({YL(p), nullptr, nullptr, DI(p), Lb(2 * p + 1), nullptr, nullptr, 1.0, 0.0});
            g.push_back({YR(p), nullptr, nullptr, DI(p), Rb(2 * p + 1), nullptr, nullptr, 1.0, 0.0});
        }
        cr.g_cnt[3 * l + 1] = (int)g.size() - cr.g_off[3 * l + 1];
        cr.g_off[3 * l + 2] = (int)g.size();
        for (int q = 0; q < ne; q++) {
            const int e = 2 * q;
            const CrEven v = cr_even(Nl, per, e);
            CrGemm dg{blk(l + 1, 0, q), D(e), nullptr, nullptr, nullptr, nullptr, nullptr, -1.0, -1.0};
            if (v.lo) { dg.A1 = XL(q); dg.B1 = Rb(v.lnb); }
            if (v.ro) { dg.A2 = XR(q); dg.B2 = Lb(v.rnb); }
            if (!dg.A1 && dg.A2) { dg.A1 = dg.A2; dg.B1 = dg.B2; dg.A2 = dg.B2 = nullptr; }
            g.push_back(dg);
            if (v.lo) g.push_back({blk(l + 1, 1, q), nullptr, nullptr, XL(q), Lb(v.lnb), nullptr, nullptr, -1.0, 0.0});
            else g.push_back({blk(l + 1, 1, q), v.lex ? Lb(e) : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0});
            if (v.ro) g.push_back({blk(l + 1, 2, q), nullptr, nullptr, XR(q), Rb(v.rnb), nullptr, nullptr, -1.0, 0.0});
            else g.push_back({blk(l + 1, 2, q), v.rex ? Rb(e) : nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0});
        }
        cr.g_cnt[3 * l + 2] = (int)g.size() - cr.g_off[3 * l + 2];
    }
    if (cr.gd.alloc(std::max<size_t>(g.size(), 1))) {
        set_error("Schur cyclic reduction: out of device memory");
        return IEMIC_ENOMEM;
    }
    return g.empty() ? 0 : h2d(c, cr.gd.p, g.data(), sizeof(CrGemm) * g.size());
}

/* dense tail: the first level of at most tail_max unknowns (default 1024; 2048: no gain,
 * DESIGN.md) and its descendants become one explicit inverse (built at set-up by solving the
 * tail for the identity), so the apply spends one GEMV launch instead of 2 (nlev - lt) + 1 */
static int cr_tail(SchurCR& cr, int tail_max)
{
    if (tail_max <= 0) tail_max = CR_TAIL_MAX;
    cr.lt = cr.nlev;
    cr.tM = 0;
    for (int l = 0; l < cr.nlev; l++)
        if (cr.N[l] > 1 && (int64_t)cr.N[l] * cr.m <= tail_max) {
            cr.lt = l;
            cr.tM = cr.N[l] * cr.m;
            break;
        }
    if (!cr.tM) return 0;
    cr.tb_off.assign(cr.nlev - cr.lt + 1, 0);
    size_t nt = 0;
    for (int l = cr.lt; l <= cr.nlev; l++) {
        cr.tb_off[l - cr.lt] = nt;
        nt += (size_t)cr.N[l] * cr.m * cr.tM;
    }
    if (cr.tinv.alloc((size_t)cr.tM * cr.tM) || cr.tb.alloc(nt) || cr.tx.alloc(nt)) {
        set_error("Schur cyclic reduction: out of device memory");
        return IEMIC_ENOMEM;
    }
    return 0;
}

int cr_init(iemic_ctx* c, SchurCR& cr, int n, int m, int periodic, int tail_max)
{
    if (m > CR_BLOCK_MAX) {
        set_error("Schur cyclic reduction: more than " + std::to_string(CR_BLOCK_MAX) + " latitudes");
        return IEMIC_EINVAL;
    }
    int rc;
    if ((rc = cr_buffers(cr, cr_levels(cr, n, m, periodic)))) return rc;
    if ((rc = cr_gemm_descriptors(c, cr))) return rc;
    if ((rc = cr_tail(cr, tail_max))) return rc;
    return cr_build_steps(c, cr);
}

}  // namespace iemic
