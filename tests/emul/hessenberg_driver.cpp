// Stand-alone driver of i-emic_amd/csrc/hessenberg.h for tests/test_hessenberg.py (host
// compiler only, nothing from HIP).  Reads from stdin, numbers as C99 hex floats:
//     m k beta
//     k columns, column q as q + 2 numbers: col[0..q] hn
// and prints one line per pushed column q:
//     |g[q+1]| cs[q] sn[q] y[0..q]        (y = solve(q + 1) after the push)
#include <cstdio>
#include <vector>

#include "../../i-emic_amd/csrc/hessenberg.h"

int main()
{
    int m = 0, k = 0;
    double beta = 0.0;
    if (std::scanf("%d %d %la", &m, &k, &beta) != 3 || m < 1 || k < 0 || k > m) return 2;
    iemic::Hessenberg hs(m);
    hs.reset(beta);
    std::vector<double> col(m + 1), y(m);
    for (int q = 0; q < k; q++) {
        double hn = 0.0;
        for (int i = 0; i <= q; i++)
            if (std::scanf("%la", &col[i]) != 1) return 2;
        if (std::scanf("%la", &hn) != 1) return 2;
        const double res = hs.push_column(q, col.data(), hn);
        hs.solve(q + 1, y.data());
        std::printf("%a %a %a", res, hs.cs[q], hs.sn[q]);
        for (int i = 0; i <= q; i++) std::printf(" %a", y[i]);
        std::printf("\n");
    }
    return 0;
}
