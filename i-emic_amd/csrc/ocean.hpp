/*
 * ocean.hpp -- header-only C++ host class over the C ABI (include/iemic.h), with the
 * method names and argument meaning of the reference's Ocean model
 * (src/ocean/Ocean.H; the calls Continuation and transient/Newton make)
 * and an Epetra-shaped vector (Update / Scale / PutScalar / Norm2 / Dot / GlobalLength).
 *
 *   reference                                  here
 *   Ocean::computeRHS()            Ocean.C:1267    computeRHS()      -> iemic_rhs
 *   Ocean::computeJacobian()       Ocean.C:1287    computeJacobian() -> iemic_jacobian
 *   Ocean::solve(rhs)              Ocean.C:1060    solve(rhs)        -> iemic_prec_compute + iemic_solve
 *   Ocean::applyMatrix(in, out)    Ocean.C:1352    applyMatrix       -> iemic_spmv
 *   Ocean::getState/getSolution/getRHS('C'|'V')    Ocean.C:1302-1318
 *   Ocean::setPar/getPar(std::string, double)      THCM::par2int names (THCM.C:1754-1807)
 *   Ocean::preProcess / postProcess                Ocean.C:790-801
 *
 * Errors throw std::runtime_error carrying iemic_last_error() (the reference throws via
 * its ERROR macro).  No CPU fallback exists: construction throws without a GPU.
 */
#ifndef IEMIC_OCEAN_HPP
#define IEMIC_OCEAN_HPP

#include <array>
#include <cmath>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/iemic.h"

namespace iemic {

inline void check(int rc, const char* what)
{
    if (rc != 0)
        throw std::runtime_error(std::string(what) + " failed (rc=" + std::to_string(rc) +
                                 "): " + iemic_last_error());
}

/* Epetra_Vector-shaped host vector in the reference's global row order. */
class Vector {
  public:
    explicit Vector(size_t n = 0, double v = 0.0) : v_(n, v) {}
    size_t GlobalLength() const { return v_.size(); }
    double* data() { return v_.data(); }
    const double* data() const { return v_.data(); }
    double& operator[](size_t i) { return v_[i]; }
    double operator[](size_t i) const { return v_[i]; }
    void PutScalar(double a) { std::fill(v_.begin(), v_.end(), a); }
    void Scale(double a) { for (double& x : v_) x *= a; }
    /* this = a*X + b*this  (Epetra_MultiVector::Update) */
    void Update(double a, const Vector& X, double b)
    {
        for (size_t i = 0; i < v_.size(); i++) v_[i] = a * X.v_[i] + b * v_[i];
    }
    double Dot(const Vector& X) const
    {
        double s = 0.0;
        for (size_t i = 0; i < v_.size(); i++) s += v_[i] * X.v_[i];
        return s;
    }
    double Norm2() const { return std::sqrt(Dot(*this)); }

  private:
    std::vector<double> v_;
};

class Ocean {
  public:
    /* grid: the THCM ParameterList subset; landm: (n+2)(m+2)(l+2) global mask */
    Ocean(const iemic_grid& grid, const std::vector<int>& landm)
    {
        if (iemic_abi_version() != IEMIC_ABI_VERSION)
            throw std::runtime_error("libiemic_amd was built from another iemic.h (ABI version " +
                                     std::to_string(iemic_abi_version()) + ", header " +
                                     std::to_string(IEMIC_ABI_VERSION) + ")");
        check(iemic_create(&ctx_, &grid, landm.data()), "iemic_create");
        N_ = (size_t)iemic_nrows(ctx_);
        nm_ = (size_t)grid.n * grid.m;
        m_ = (size_t)grid.m;
        state_ = std::make_shared<Vector>(N_);
        rhs_ = std::make_shared<Vector>(N_);
        sol_ = std::make_shared<Vector>(N_);
        /* Belos defaults of Ocean::getDefaultInitParameters (Ocean.C:2232-2237) */
        krylov_ = iemic_krylov{1e-8, 500, 0, 2, 12, 0, 4, /*method FGMRES*/ 0, 1, 1, 0.95, 0, 4, 0.7, 0, 0, /*Schur passes*/ 2};
    }
    ~Ocean() { iemic_destroy(ctx_); }
    Ocean(const Ocean&) = delete;
    Ocean& operator=(const Ocean&) = delete;

    /* ---- Model interface -------------------------------------------------------- */
    void computeRHS() { check(iemic_rhs(ctx_, rhs_->data()), "computeRHS"); }
    void computeJacobian() { check(iemic_jacobian(ctx_), "computeJacobian"); }
    void applyMatrix(const Vector& in, Vector& out)
    {
        check(iemic_spmv(ctx_, in.data(), out.data()), "applyMatrix");
    }
    void buildPreconditioner(bool force = false)
    {
        if (recompPrec_ || force) {
            check(iemic_prec_compute(ctx_, &krylov_), "buildPreconditioner");
            recompPrec_ = false;
        }
    }
    void applyPrecon(const Vector& in, Vector& out)
    {
        check(iemic_prec_apply(ctx_, in.data(), out.data()), "applyPrecon");
    }
    /* J sol = rhs (Ocean::solve); the solution is in getSolution() */
    void solve(const Vector& rhs)
    {
        buildPreconditioner();
        check(iemic_solve(ctx_, rhs.data(), sol_->data(), &krylov_, &lastSolve_), "solve");
    }
    void preProcess() { recompPrec_ = true; }
    void postProcess() {}

    /* ---- state (mode 'C' = copy, 'V' = view of the host mirror) ----------------- */
    void setState(const Vector& x)
    {
        *state_ = x;
        check(iemic_set_state(ctx_, x.data()), "setState");
    }
    std::shared_ptr<Vector> getState(char mode)
    {
        check(iemic_get_state(ctx_, state_->data()), "getState");
        return mode == 'V' ? state_ : std::make_shared<Vector>(*state_);
    }
    std::shared_ptr<Vector> getRHS(char mode)
    {
        return mode == 'V' ? rhs_ : std::make_shared<Vector>(*rhs_);
    }
    std::shared_ptr<Vector> getSolution(char mode)
    {
        return mode == 'V' ? sol_ : std::make_shared<Vector>(*sol_);
    }

    /* ---- parameters (THCM::par2int names) ---------------------------------------- */
    void setPar(const std::string& name, double v) { check(iemic_set_par(ctx_, parIndex(name), v), "setPar"); }
    double getPar(const std::string& name)
    {
        double v = 0.0;
        check(iemic_get_par(ctx_, parIndex(name), &v), "getPar");
        return v;
    }
    static int parIndex(const std::string& name)
    {
        static const std::map<std::string, int> idx = {
            {"AL_T", 1}, {"Rayleigh-Number", 2}, {"Vertical Ekman-Number", 3},
            {"Horizontal Ekman-Number", 4}, {"Rossby-Number", 5}, {"MIXP", 6}, {"RESC", 7},
            {"SPL1", 8}, {"Salinity Homotopy", 9}, {"Solar Forcing", 10},
            {"Horizontal Peclet-Number", 11}, {"Vertical Peclet-Number", 12}, {"P_VC", 13},
            {"LAMB", 14}, {"Salinity Forcing", 15}, {"Wind Forcing", 16},
            {"Temperature Forcing", 17}, {"Nonlinear Factor", 18}, {"Combined Forcing", 19},
            {"ARCL", 20}, {"NLES", 21}, {"IFRICB", 22}, {"CONT", 23}, {"Energy", 24},
            {"ALPC", 25}, {"CMPR", 26}, {"Flux Perturbation", 27},
            {"Salinity Perturbation", 28}, {"MKAP", 29}, {"SPL2", 30}};
        auto it = idx.find(name);
        if (it == idx.end()) throw std::runtime_error("invalid THCM parameter: " + name);
        return it->second;
    }

    /* ---- surface fluxes and inserted forcing fields (n*m, (j, i) with i fastest) ---- */
    /* THCM::getFluxes (THCM.C:1559-1593): the nine fields in the order of THCM's enum
     * (_Sal, _QSOA, _QSOS, _Temp, _QSW, _QSH, _QLH, _QTOS, _MSI) of the current state;
     * scorr (optional): the salinity correction times COMB*SALT */
    std::vector<std::vector<double>> getFluxes(double* scorr = nullptr)
    {
        const size_t nm = nm_;
        std::vector<double> all(9 * nm, 0.0);
        double sc = 0.0;
        check(iemic_get_fluxes(ctx_, nullptr, all.data(), &sc), "getFluxes");
        if (scorr) *scorr = sc;
        std::vector<std::vector<double>> out;
        for (int f = 0; f < 9; f++) out.emplace_back(all.begin() + f * nm, all.begin() + (f + 1) * nm);
        return out;
    }
    /* THCM::setEmip / getEmip (THCM.C:1486-1514, 1530-1556): mode 'E', 'A' or 'P'; an empty
     * field restores the idealized profile */
    void setEmip(const std::vector<double>& field, char mode = 'E')
    {
        check(iemic_set_emip(ctx_, mode, field.empty() ? nullptr : field.data()), "setEmip");
    }
    std::vector<double> getEmip(char mode = 'E')
    {
        std::vector<double> out(nm_, 0.0);
        check(iemic_get_emip(ctx_, mode, out.data()), "getEmip");
        return out;
    }
    /* THCM::setTatm (THCM.C:1466-1483) */
    void setTatm(const std::vector<double>& field)
    {
        check(iemic_set_tatm(ctx_, field.empty() ? nullptr : field.data()), "setTatm");
    }

    /* ---- Belos settings (names of Ocean's solver ParameterList) ----------------- */
    iemic_krylov& solverParameters() { return krylov_; }
    const iemic_solve_info& lastSolve() const { return lastSolve_; }

    /* device-resident Newton step (transient/Newton.H:92-99 shape).  The update is applied
     * even when the linear solve missed its tolerance (IEMIC_ENOCONV, a warning), as the
     * reference's Newton / Continuation go on with the unconverged correction unless
     * rejectFailedNewton is set: the caller reads info.solve.converged.  Errors throw. */
    iemic_newton_info newtonStep()
    {
        iemic_newton_info info{};
        const int rc = iemic_newton_step(ctx_, &krylov_, &info);
        if (rc != IEMIC_ENOCONV) check(rc, "newtonStep");
        return info;
    }

    /* ---- the theta time stepper: what ThetaModel<Ocean> lays over the model -------- */
    /* ThetaModel::initStep (ThetaModel.H:64-74): x_n <- state, F_n <- F(x_n), and its
     * preProcess: the preconditioner is refactored at the step's first solve */
    void thetaInitStep(double dt, double theta)
    {
        check(iemic_theta_init_step(ctx_, dt, theta), "thetaInitStep");
        preProcess();
    }
    /* ThetaModel::computeRHS (ThetaModel.H:87-113): F_theta in getRHS() */
    void thetaRHS() { check(iemic_theta_rhs(ctx_, rhs_->data()), "thetaRHS"); }
    /* ThetaModel::computeJacobian (ThetaModel.H:118-146): solve, applyMatrix and
     * buildPreconditioner then act on J - B / dt / theta */
    void thetaJacobian() { check(iemic_theta_jacobian(ctx_), "thetaJacobian"); }
    void thetaRestore() { check(iemic_theta_restore(ctx_), "thetaRestore"); }
    /* one iteration of Newton.H:92-99 on the theta model, on the device; the update is
     * applied even when the linear solve missed its tolerance (info.solve.converged) */
    iemic_theta_info thetaNewtonStep()
    {
        iemic_theta_info info{};
        const int rc = iemic_theta_newton_step(ctx_, &krylov_, recompPrec_ ? 1 : 0, &info);
        if (rc != IEMIC_ENOCONV) check(rc, "thetaNewtonStep");
        recompPrec_ = false;
        lastSolve_ = info.solve;
        return info;
    }

    /* ---- the stochastic theta model: what StochasticThetaModel<Ocean> adds ----------- */
    /* Ocean::computeForcing: the stochastic forcing operator of the current parameters */
    void computeForcing() { check(iemic_forcing_compute(ctx_), "computeForcing"); }
    /* Ocean::getForcing: the operator's entries (row, column = latitude j, value), sorted by row */
    struct Forcing {
        std::vector<int64_t> rows;
        std::vector<int> cols;
        std::vector<double> vals;
    };
    Forcing getForcing()
    {
        int64_t nnz = 0;
        check(iemic_forcing_export(ctx_, nullptr, nullptr, nullptr, &nnz), "getForcing");
        Forcing f{std::vector<int64_t>((size_t)nnz), std::vector<int>((size_t)nnz), std::vector<double>((size_t)nnz)};
        check(iemic_forcing_export(ctx_, f.rows.data(), f.cols.data(), f.vals.data(), &nnz), "getForcing");
        return f;
    }
    /* StochasticThetaModel::initStep (StochasticThetaModel.H:52-72): thetaInitStep, then the
     * step's noise G = (sqrt(dt) sigma) (B_f pert) armed for thetaRHS / thetaNewtonStep; pert: m
     * standard normals, one per latitude (the caller's generator) */
    void stochasticInitStep(double dt, double theta, double sigma, const std::vector<double>& pert)
    {
        if (pert.size() != m_)
            throw std::runtime_error("stochasticInitStep: pert has " + std::to_string(pert.size()) +
                                     " entries, the grid has " + std::to_string(m_) + " latitudes");
        check(iemic_theta_init_step_noise(ctx_, dt, theta, sigma, pert.data()), "stochasticInitStep");
        preProcess();
    }

    /* ---- the projected theta model: what ProjectedThetaModel<Ocean> and
     * StochasticProjectedThetaModel<Ocean> lay over the model (the state confined to x = V y; the
     * k x k Newton system is factored on the host, no preconditioner, no Krylov solver) -------- */
    /* the constructor's V (ProjectedThetaModel.H:38-65): k columns of nrows() doubles, column-major,
     * 1 <= k <= IEMIC_PROJ_MAX_K, not necessarily orthonormal */
    void projSetBasis(const std::vector<double>& V, int k)
    {
        if (k < 1 || V.size() != (size_t)k * N_)
            throw std::runtime_error("projSetBasis: V has " + std::to_string(V.size()) + " entries, k x nrows = " +
                                     std::to_string((size_t)(k < 0 ? 0 : k) * N_));
        check(iemic_proj_set_basis(ctx_, V.data(), k), "projSetBasis");
        k_ = (size_t)k;
    }
    void projClear()
    {
        check(iemic_proj_clear(ctx_), "projClear");
        k_ = 0;
    }
    /* restrict (ProjectedThetaModel.H:196-206) of the state */
    std::vector<double> projRestrictState()
    {
        std::vector<double> y(k_ ? k_ : 1);
        check(iemic_proj_restrict_state(ctx_, y.data()), "projRestrictState");
        return y;
    }
    /* setState (ProjectedThetaModel.H:114-118): state = V y */
    void projSetState(const std::vector<double>& y)
    {
        if (k_ && y.size() != k_) throw std::runtime_error("projSetState: y has " + std::to_string(y.size()) + " entries");
        check(iemic_proj_set_state(ctx_, y.data()), "projSetState");
    }
    /* initStep (ProjectedThetaModel.H:70-112); with noise StochasticProjectedThetaModel.H:71-92 */
    void projInitStep(double dt, double theta) { check(iemic_proj_init_step(ctx_, dt, theta), "projInitStep"); }
    void projStochasticInitStep(double dt, double theta, double sigma, const std::vector<double>& pert)
    {
        if (pert.size() != m_)
            throw std::runtime_error("projStochasticInitStep: pert has " + std::to_string(pert.size()) +
                                     " entries, the grid has " + std::to_string(m_) + " latitudes");
        check(iemic_proj_init_step_noise(ctx_, dt, theta, sigma, pert.data()), "projStochasticInitStep");
    }
    /* computeRHS (ProjectedThetaModel.H:125-155) and solve (:163-193) */
    std::vector<double> projRHS()
    {
        std::vector<double> r(k_ ? k_ : 1);
        check(iemic_proj_rhs(ctx_, r.data()), "projRHS");
        return r;
    }
    std::vector<double> projSolve(const std::vector<double>& r)
    {
        std::vector<double> dy(k_ ? k_ : 1);
        if (r.size() != dy.size()) throw std::runtime_error("projSolve: r has " + std::to_string(r.size()) + " entries");
        check(iemic_proj_solve(ctx_, r.data(), dy.data()), "projSolve");
        return dy;
    }
    /* one iteration of Newton.H:94-99 on the small state */
    iemic_proj_info projNewtonStep()
    {
        iemic_proj_info info{};
        check(iemic_proj_newton_step(ctx_, &info), "projNewtonStep");
        return info;
    }
    /* the state and the small state as at the init step */
    void projRestore() { check(iemic_proj_restore(ctx_), "projRestore"); }
    /* "y", "y_n", "F_n", "r", "G" (k) or "VMV", "VAV" (k x k, row-major) */
    std::vector<double> projGet(const std::string& what)
    {
        const size_t k = k_ ? k_ : 1;
        std::vector<double> out(what == "VMV" || what == "VAV" ? k * k : k);
        check(iemic_proj_get(ctx_, what.c_str(), out.data()), "projGet");
        return out;
    }

    /* ---- the rare-event score function (ScoreFunctions.C): d1 = ||x - sol1||_v / nrm and d2 from
     * one pass over x, sol1 and sol2; var = -1 the default score (all rows), var = 1 the ocean
     * score (the v rows) --------------------------------------------------------------------- */
    /* sol1, sol2, sol3 (empty: none, the distance factor is 0.5): nrows() doubles each */
    void scoreSet(const std::vector<double>& sol1, const std::vector<double>& sol2, const std::vector<double>& sol3,
                  int var = -1)
    {
        if (sol1.size() != N_ || sol2.size() != N_ || (!sol3.empty() && sol3.size() != N_))
            throw std::runtime_error("scoreSet: sol1, sol2 and sol3 must have nrows() = " + std::to_string(N_) +
                                     " entries");
        check(iemic_score_set(ctx_, sol1.data(), sol2.data(), sol3.empty() ? nullptr : sol3.data(), var), "scoreSet");
    }
    /* {nrm, distance factor} */
    std::array<double, 2> scoreGet()
    {
        std::array<double, 2> out{};
        check(iemic_score_get(ctx_, &out[0], &out[1]), "scoreGet");
        return out;
    }
    /* {dist, d1, d2} of the device vector v (iemic_vec_alloc), or of the resident state */
    std::array<double, 3> score(const double* v = nullptr)
    {
        std::array<double, 3> out{};
        check(iemic_score(ctx_, v, &out[0], &out[1], &out[2]), "score");
        return out;
    }
    /* V^T V (var = -1) or V^T diag(e_var) V of the basis, k x k row-major */
    std::vector<double> projGramVV(int var = -1)
    {
        const size_t k = k_ ? k_ : 1;
        std::vector<double> out(k * k);
        check(iemic_proj_gram_vv(ctx_, var, out.data()), "projGramVV");
        return out;
    }

    /* ---- linear stability analysis: the calls a JDQZInterface-shaped eigen-solver makes
     * (src/utils/JDQZInterface.H); the Hessenberg eigen-decomposition is the caller's
     * (INTEGRATION.md shows it with LAPACKE_dhseqr / dtrevc) ------------------------- */
    /* J - sigma B at the state: solve, applyMatrix and buildPreconditioner then act on it;
     * computeJacobian restores J */
    void shiftedJacobian(double sigma) { check(iemic_shifted_jacobian(ctx_, sigma), "shiftedJacobian"); }
    /* a shift-invert Arnoldi run on (J - sigma B)^-1 B: at most m <= IEMIC_EIGS_MAX_M steps */
    void eigsBegin(double sigma, int m, uint64_t seed = 1)
    {
        check(iemic_eigs_begin(ctx_, sigma, m, seed, &krylov_), "eigsBegin");
        recompPrec_ = false;
    }
    /* one step: hcol receives column info.step of the Hessenberg matrix (step + 2 doubles); an
     * inner solve that missed its tolerance shows in info.solve.converged */
    iemic_eigs_info eigsStep(double* hcol)
    {
        iemic_eigs_info info{};
        const int rc = iemic_eigs_step(ctx_, &krylov_, hcol, &info);
        if (rc != IEMIC_ENOCONV) check(rc, "eigsStep");
        lastSolve_ = info.solve;
        return info;
    }
    /* xvecs[q] = sum_i Y[i p + q] v_i, i < j: p device vectors from iemic_vec_alloc */
    void eigsRitz(int j, int p, const double* Y, void** xvecs)
    {
        check(iemic_eigs_ritz(ctx_, j, p, Y, xvecs), "eigsRitz");
    }
    /* thick restart on Q (j x p row-major, orthonormal, invariant under the caller's Rayleigh
     * matrix): the basis becomes [V_j Q, v_{j+1}], j <- p, and eigsStep goes on from there */
    void eigsRestart(int p, const double* Q) { check(iemic_eigs_restart(ctx_, p, Q), "eigsRestart"); }
    /* out = ||(J - sigma B) x - (lambda - sigma) B x||, ||(J - sigma B) x|| */
    void eigsResidual(double lamRe, double lamIm, double* xRe, double* xIm, double out[2])
    {
        check(iemic_eigs_residual(ctx_, lamRe, lamIm, xRe, xIm, out), "eigsResidual");
    }
    void eigsEnd() { check(iemic_eigs_end(ctx_), "eigsEnd"); }

    size_t nrows() const { return N_; }
    iemic_ctx* handle() { return ctx_; }

  private:
    iemic_ctx* ctx_ = nullptr;
    size_t N_ = 0, nm_ = 0, m_ = 0, k_ = 0;   /* k_: columns of the projected model's basis */
    std::shared_ptr<Vector> state_, rhs_, sol_;
    iemic_krylov krylov_{};
    iemic_solve_info lastSolve_{};
    bool recompPrec_ = true;
};

}  // namespace iemic
#endif
