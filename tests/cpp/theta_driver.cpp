// theta_driver.cpp -- C++ host check of the theta stepper surface of i-emic_amd/csrc/ocean.hpp
// (thetaInitStep / thetaNewtonStep / thetaRestore, what ThetaModel<Ocean> binds).  Reads the
// problem file of tests/cpp/ocean_driver.cpp (written by tests/test_cpp_theta.py), then
//   theta_driver <in> <dt> <theta> <nsteps> <tol> <maxit>
// runs nsteps fixed time steps from the file's state, each a Newton run as Newton.H:76-123,
// and prints one line per time step: step, Newton::steps(), ||x||_2, ||dx||_inf, ||F_theta||_2.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../i-emic_amd/csrc/ocean.hpp"

template <typename T> static void rd(FILE* f, T* p, size_t n)
{
    if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
}

int main(int argc, char** argv)
{
    if (argc < 7) { fprintf(stderr, "usage: theta_driver <in> <dt> <theta> <nsteps> <tol> <maxit>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const double dt = atof(argv[2]), theta = atof(argv[3]), tol = atof(argv[5]);
    const int nsteps = atoi(argv[4]), maxit = atoi(argv[6]);
    int hdr[11];
    rd(f, hdr, 11);
    double dv[8];
    rd(f, dv, 8);
    iemic_grid g{};
    g.n = hdr[0]; g.m = hdr[1]; g.l = hdr[2]; g.periodic = hdr[3]; g.tres = hdr[4];
    g.sres = hdr[5]; g.forcing_type = hdr[6]; g.ih = hdr[7]; g.coriolis_on = hdr[8];
    g.int_sign = hdr[9];
    g.xmin = dv[0]; g.xmax = dv[1]; g.ymin = dv[2]; g.ymax = dv[3]; g.hdim = dv[4]; g.qz = dv[5];
    g.alpha_t = dv[6]; g.alpha_s = dv[7];
    g.vmix = 0; g.int_i = -1; g.int_j = -1; g.analyze_jacobian = 1; g.max_mask_fixes = 5;
    g.device = 0;
    const int npar = hdr[10];
    std::vector<std::pair<int, double>> pars(npar);
    for (int q = 0; q < npar; q++) {
        rd(f, &pars[q].first, 1);
        rd(f, &pars[q].second, 1);
    }
    const size_t nl = (size_t)(g.n + 2) * (g.m + 2) * (g.l + 2);
    std::vector<int> landm(nl);
    rd(f, landm.data(), nl);
    const size_t N = (size_t)6 * g.n * g.m * g.l;
    iemic::Vector x(N);
    rd(f, x.data(), N);
    fclose(f);
    try {
        iemic::Ocean ocean(g, landm);
        for (auto& p : pars) iemic::check(iemic_set_par(ocean.handle(), p.first, p.second), "set_par");
        ocean.solverParameters().tol = 1e-6;
        ocean.setState(x);
        for (int step = 1; step <= nsteps; step++) {
            ocean.thetaInitStep(dt, theta);
            int k = 0;
            bool converged = false;
            iemic_theta_info info{};
            for (; k < maxit; k++) {
                info = ocean.thetaNewtonStep();
                if (info.norm_dx < tol && info.norm_f1 < tol) { converged = true; break; }
                if (info.norm_dx > 1e2) break;
            }
            if (!converged) {
                ocean.thetaRestore();
                fprintf(stderr, "error: Newton did not converge in time step %d\n", step);
                return 1;
            }
            printf("step %d newton %d normx %.17g normdx %.17g normF %.17g\n", step, k,
                   ocean.getState('V')->Norm2(), info.norm_dx, info.norm_f1);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
