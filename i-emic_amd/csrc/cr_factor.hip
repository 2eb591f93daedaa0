/*
 * cr_factor.hip -- set-up of the block cyclic reduction (schur_cr.hip): the level-0 blocks from
 * the 9-point rows, per level the Gauss-Jordan inverses of the odd blocks (cr_inv.hip) and the
 * batched GEMMs of cr_init's descriptors, the composite operators and packed runs of the apply
 * steps, and the dense tail's inverse, built by running the tail's levels on the identity with
 * the batched level kernels.  Stream-ordered, no host synchronisation.
 */
#include "cr_internal.h"

namespace iemic {

namespace {

constexpr int CR_MAXM = 512;                    /* the level kernels' vectors in LDS */

/* level-0 blocks from the 9-point rows S9[c*9 + (dj+1)*3 + (di+1)], c = i*m + j; inactive
 * columns (no water) become identity rows.  One thread per row (i, j): no write races. */
__global__ void k_cr_expand(const double* __restrict__ S9, const int* __restrict__ col_of_ij, int n,
                            int m, int periodic, double* __restrict__ D, double* __restrict__ Lb,
                            double* __restrict__ Rb)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n * m) return;
    const int i = c / m, j = c % m;
    const size_t mm = (size_t)m * m;
    double* Di = D + (size_t)i * mm;
    if (col_of_ij[j * n + i] < 0) {
        Di[j + (size_t)j * m] = 1.0;
        return;
    }
    for (int o = 0; o < 9; o++) {
        const double v = S9[(size_t)c * 9 + o];
        if (v == 0.0) continue;
        const int di = o % 3 - 1, dj = o / 3 - 1;
        int ti = i + di;
        const int tj = j + dj;
        if (tj < 0 || tj >= m) continue;
        if (ti < 0 || ti >= n) {
            if (!periodic) continue;
            ti = (ti + n) % n;
        }
        double* B = ti == i ? Di : (di < 0 ? Lb + (size_t)i * mm : Rb + (size_t)i * mm);
        B[j + (size_t)tj * m] += v;
    }
}

/* pa[q] = (A B)(r0 + tr, c0 + tc + 8 q), q < 4: one 32 x 32 tile of the product of two m x m
 * column-major blocks by 256 threads (tr = t & 31, tc = t >> 5), k in steps of 32 through LDS */
__device__ __forceinline__ void cr_tile_product(const double* __restrict__ A, const double* __restrict__ B, int m,
                                                int r0, int c0, double (&As)[32][33], double (&Bs)[32][33],
                                                double (&pa)[4])
{
    const int t = threadIdx.x, tr = t & 31, tc = t >> 5;
#pragma unroll
    for (int q = 0; q < 4; q++) pa[q] = 0.0;
    for (int k0 = 0; k0 < m; k0 += 32) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = t + 256 * q;
            const int rr = e & 31, kk = e >> 5;
            As[kk][rr] = (r0 + rr < m && k0 + kk < m) ? A[(r0 + rr) + (size_t)(k0 + kk) * m] : 0.0;
            const int kb = e & 31, cc = e >> 5;
            Bs[cc][kb] = (k0 + kb < m && c0 + cc < m) ? B[(k0 + kb) + (size_t)(c0 + cc) * m] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < 32; kk++) {
            const double a = As[kk][tr];
#pragma unroll
            for (int q = 0; q < 4; q++) pa[q] += a * Bs[tc + 8 * q][kk];
        }
        __syncthreads();
    }
}

/* C = C0 + C0b + s1 A1 B1 + s2 A2 B2 for a batch of m x m column-major blocks: one 32x32
 * tile of one descriptor per workgroup (blockIdx.y = descriptor) */
__global__ void __launch_bounds__(256) k_cr_gemm(const CrGemm* __restrict__ dd, int m)
{
    const CrGemm d = dd[blockIdx.y];
    const int T = (m + 31) / 32;
    const int r0 = (blockIdx.x % T) * 32, c0 = (blockIdx.x / T) * 32;
    const int t = threadIdx.x, tr = t & 31, tc = t >> 5;
    __shared__ double As[32][33], Bs[32][33];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int prod = 0; prod < 2; prod++) {
        const double* A = prod ? d.A2 : d.A1;
        const double* B = prod ? d.B2 : d.B1;
        if (!A) continue;
        const double s = prod ? d.s2 : d.s1;
        double pa[4];
        cr_tile_product(A, B, m, r0, c0, As, Bs, pa);
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] += s * pa[q];
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int r = r0 + tr, c = c0 + tc + 8 * q;
        if (r >= m || c >= m) continue;
        const size_t idx = r + (size_t)c * m;
        double v = acc[q];
        if (d.C0) v += d.C0[idx];
        if (d.C0b) v += d.C0b[idx];
        d.C[idx] = v;
    }
}

/* composite operators C = sum_k s_k A_k B_k: one 32x32 tile of one descriptor per workgroup */
__global__ void __launch_bounds__(256) k_cr_comp(const CrComp* __restrict__ dd, int m)
{
    const CrComp d = dd[blockIdx.y];
    const int T = (m + 31) / 32;
    const int r0 = (blockIdx.x % T) * 32, c0 = (blockIdx.x / T) * 32;
    const int t = threadIdx.x, tr = t & 31, tc = t >> 5;
    __shared__ double As[32][33], Bs[32][33];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int term = 0; term < d.nt; term++) {
        const double* A = d.A[term];
        const double* B = d.B[term];
        const double sc = d.s[term];
        if (!A) {                                           /* identity */
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (r0 + tr == c0 + tc + 8 * q && r0 + tr < m) acc[q] += sc;
            continue;
        }
        if (!B) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int rr = r0 + tr, cc = c0 + tc + 8 * q;
                if (rr < m && cc < m) acc[q] += sc * A[rr + (size_t)cc * m];
            }
            continue;
        }
        double pa[4];
        cr_tile_product(A, B, m, r0, c0, As, Bs, pa);
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] += sc * pa[q];
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int rr = r0 + tr, cc = c0 + tc + 8 * q;
        if (rr < m && cc < m) d.C[rr + (size_t)cc * m] = acc[q];
    }
}

/* set-up copy of the matrix terms into the packed layout, one job per workgroup */
__global__ void __launch_bounds__(256) k_cr_pack(const CrPack* __restrict__ jobs, double* __restrict__ P, int m, int rc)
{
    const CrPack j = jobs[blockIdx.x];
    for (int e = threadIdx.x; e < m * rc; e += 256) {
        const int c = e / rc, rr = e - c * rc, r = j.r0 + rr;
        P[j.dst + e] = r < m ? j.s * j.A[r + (size_t)c * m] : 0.0;
    }
}

/* level down, one row chunk of one even block per workgroup (blockIdx.x = q * nch + chunk):
 * b'_q = b_e - XL_q b_{e-1} - XR_q b_{e+1} (odd neighbours only), e = 2q */
__global__ void __launch_bounds__(256) k_cr_fwd(const double* __restrict__ bl, double* __restrict__ bn,
                                                const double* __restrict__ XL, const double* __restrict__ XR,
                                                int N, int per, int m, int nch, int64_t sl, int64_t sn, int nrhs)
{
    __shared__ double vl[CR_MAXM], vr[CR_MAXM], red[256];
    const int q = blockIdx.x / nch, r0 = (blockIdx.x % nch) * CR_RC, e = 2 * q;
    const CrEven g = cr_even(N, per, e);
    const size_t mm = (size_t)m * m;
    CrFrag f;
    crf_load(f, g.lo ? XL + q * mm : nullptr, g.ro ? XR + q * mm : nullptr, nullptr, m, r0);
    const int r1 = min(nrhs, (int)(blockIdx.y + 1) * CR_RB);
    for (int rh = blockIdx.y * CR_RB; rh < r1; rh++) {
        const double* b = bl + rh * sl;
        for (int c = threadIdx.x; c < m; c += 256) {
            vl[c] = g.lo ? b[(size_t)g.lnb * m + c] : 0.0;
            vr[c] = g.ro ? b[(size_t)g.rnb * m + c] : 0.0;
        }
        __syncthreads();
        crf_finish(f, vl, vr, vl, -1.0, b + (size_t)e * m, bn + rh * sn + (size_t)q * m, m, r0, red);
    }
}

/* level up, one row chunk of one odd block per workgroup (blockIdx.x = p * nch + chunk):
 * x_o = Dinv b_o - YL x_{o-1} - YR x_{o+1}, o = 2p + 1; the even blocks are copied from
 * the level below (x_{o-1} by block o, the last even block of an odd count by block N-2) */
__global__ void __launch_bounds__(256) k_cr_bwd(const double* __restrict__ bl, const double* __restrict__ xn,
                                                double* __restrict__ xl, const double* __restrict__ Dinv,
                                                const double* __restrict__ YL, const double* __restrict__ YR,
                                                int N, int per, int m, int nch, int64_t sl, int64_t sn, int nrhs)
{
    __shared__ double vb[CR_MAXM], vl[CR_MAXM], vr[CR_MAXM], red[256];
    const int p = blockIdx.x / nch, r0 = (blockIdx.x % nch) * CR_RC, b = 2 * p + 1;
    const CrOdd g = cr_odd(N, per, b);
    const size_t mm = (size_t)m * m;
    CrFrag f;
    crf_load(f, Dinv + p * mm, YL + p * mm, g.rex ? YR + p * mm : nullptr, m, r0);
    const int r1 = min(nrhs, (int)(blockIdx.y + 1) * CR_RB);
    for (int rh = blockIdx.y * CR_RB; rh < r1; rh++) {
        const double* bq = bl + rh * sl;
        const double* xq = xn + rh * sn;
        double* xo = xl + rh * sl;
        for (int c = threadIdx.x; c < m; c += 256) {
            vb[c] = bq[(size_t)b * m + c];
            vl[c] = -xq[(size_t)p * m + c];
            vr[c] = g.rex ? -xq[(size_t)(g.rn / 2) * m + c] : 0.0;
        }
        if (threadIdx.x < CR_RC && r0 + threadIdx.x < m) {
            const int r = r0 + threadIdx.x;
            xo[(size_t)(b - 1) * m + r] = xq[(size_t)p * m + r];
            if (b == N - 2) xo[(size_t)(N - 1) * m + r] = xq[(size_t)((N - 1) / 2) * m + r];
        }
        __syncthreads();
        crf_finish(f, vb, vl, vr, 1.0, nullptr, xo + (size_t)b * m, m, r0, red);
    }
}

/* the last level: x = Dfin b, one row chunk per workgroup */
__global__ void __launch_bounds__(256) k_cr_final(const double* __restrict__ Dfin, const double* __restrict__ b,
                                                  double* __restrict__ x, int m, int nrhs)
{
    __shared__ double vb[CR_MAXM], red[256];
    CrFrag f;
    crf_load(f, Dfin, nullptr, nullptr, m, blockIdx.x * CR_RC);
    const int r1 = min(nrhs, (int)(blockIdx.y + 1) * CR_RB);
    for (int rh = blockIdx.y * CR_RB; rh < r1; rh++) {
        for (int c = threadIdx.x; c < m; c += 256) vb[c] = b[(size_t)rh * m + c];
        __syncthreads();
        crf_finish(f, vb, vb, vb, 1.0, nullptr, x + (size_t)rh * m, m, blockIdx.x * CR_RC, red);
    }
}

/* dense tail, set-up: the identity as tM right-hand sides of the tail's first level */
__global__ void k_cr_eye(double* __restrict__ B, int M)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (int64_t)M * M) B[e] = (e / M == e % M) ? 1.0 : 0.0;
}

/* T = X^T for the M x M column-major X (32 x 32 tiles through LDS) */
__global__ void k_cr_transpose(const double* __restrict__ X, double* __restrict__ T, int M)
{
    __shared__ double t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int y = ty; y < 32; y += 8)
        if (r0 + tx < M && c0 + y < M) t[y][tx] = X[(r0 + tx) + (size_t)(c0 + y) * M];
    __syncthreads();
    for (int y = ty; y < 32; y += 8)
        if (c0 + tx < M && r0 + y < M) T[(r0 + y) * (size_t)M + c0 + tx] = t[tx][y];
}

}  // namespace

/* one level down / up for nrhs right-hand sides (level vectors N[l] m apart) */
static void cr_down(const SchurCR& cr, int l, const double* bl, double* bn, int nrhs, hipStream_t s)
{
    const int m = cr.m, nch = (m + CR_RC - 1) / CR_RC, Nl = cr.N[l], ne = (Nl + 1) / 2;
    const CrOps o = cr_ops(cr, l);
    hipLaunchKernelGGL(k_cr_fwd, dim3(ne * nch, (nrhs + CR_RB - 1) / CR_RB), dim3(256), 0, s, bl, bn,
                       (const double*)o.XL, (const double*)o.XR, Nl, cr.per[l], m, nch, (int64_t)Nl * m,
                       (int64_t)cr.N[l + 1] * m, nrhs);
}
static void cr_up(const SchurCR& cr, int l, const double* bl, const double* xn, double* xl, int nrhs, hipStream_t s)
{
    const int m = cr.m, nch = (m + CR_RC - 1) / CR_RC, Nl = cr.N[l], no = Nl / 2;
    const CrOps o = cr_ops(cr, l);
    hipLaunchKernelGGL(k_cr_bwd, dim3(no * nch, (nrhs + CR_RB - 1) / CR_RB), dim3(256), 0, s, bl, xn, xl,
                       (const double*)o.Dinv, (const double*)o.YL, (const double*)o.YR, Nl, cr.per[l], m, nch,
                       (int64_t)Nl * m, (int64_t)cr.N[l + 1] * m, nrhs);
}
void cr_final(const SchurCR& cr, const double* b, double* x, int nrhs, hipStream_t s)
{
    hipLaunchKernelGGL(k_cr_final, dim3((cr.m + CR_RC - 1) / CR_RC, (nrhs + CR_RB - 1) / CR_RB), dim3(256), 0, s,
                       (const double*)cr_last(cr), b, x, cr.m, nrhs);
}

/* set-up from the 9-point rows (stream-ordered, no host synchronisation) */
int cr_factor(iemic_ctx* c, SchurCR& cr, const double* S9, const int* col_of_ij)
{
    hipStream_t s = c->stream;
    const int m = cr.m;
    const size_t mm = (size_t)m * m;
    HIP_OK(hipMemsetAsync(cr.dlr.p, 0, sizeof(double) * 3 * (size_t)cr.n * mm, s));
    const int nm = cr.n * m;
    hipLaunchKernelGGL(k_cr_expand, dim3((nm + 255) / 256), dim3(256), 0, s, S9, col_of_ij, cr.n, m,
                       cr.periodic, cr.dlr.p, cr.dlr.p + (size_t)cr.n * mm, cr.dlr.p + 2 * (size_t)cr.n * mm);
    return cr_factor_blocks(c, cr);
}

/* set-up from level-0 blocks already in cr.dlr (D, L, R: 3 n column-major m x m blocks) */
int cr_factor_blocks(iemic_ctx* c, SchurCR& cr)
{
    hipStream_t s = c->stream;
    int rc;
    const int m = cr.m;
    const int T = (m + 31) / 32;
    HIP_OK(hipMemsetAsync(cr.info.p, 0, sizeof(int), s));
    for (int l = 0; l < cr.nlev; l++) {
        if (cr.g_cnt[3 * l])
            hipLaunchKernelGGL(k_cr_gemm, dim3(T * T, cr.g_cnt[3 * l]), dim3(256), 0, s, cr.gd.p + cr.g_off[3 * l], m);
        if ((rc = cr_inverse(s, m, cr.N[l] / 2, cr.dlr.p + cr.dlr_off[l], 1, 2, cr_ops(cr, l).Dinv, cr.info.p)))
            return rc;
        hipLaunchKernelGGL(k_cr_gemm, dim3(T * T, cr.g_cnt[3 * l + 1]), dim3(256), 0, s,
                           cr.gd.p + cr.g_off[3 * l + 1], m);
        hipLaunchKernelGGL(k_cr_gemm, dim3(T * T, cr.g_cnt[3 * l + 2]), dim3(256), 0, s,
                           cr.gd.p + cr.g_off[3 * l + 2], m);
    }
    if ((rc = cr_inverse(s, m, 1, cr.dlr.p + cr.dlr_off[cr.nlev], 0, 1, cr_last(cr), cr.info.p)))
        return rc;
    if (cr.ncomp)                          /* the composite operators of the apply steps */
        hipLaunchKernelGGL(k_cr_comp, dim3(T * T, cr.ncomp), dim3(256), 0, s, cr.cdesc.p, m);
    for (const auto* v : {&cr.down, &cr.up})   /* the apply steps' packed operators */
        for (const CrStep& st : *v)
            if (st.njobs)
                hipLaunchKernelGGL(k_cr_pack, dim3(st.njobs), dim3(256), 0, s, (const CrPack*)st.jobs.p, st.P.p, m,
                                   st.rc);
    if (cr.tM) {                           /* the tail's inverse, column r = tail solve of e_r */
        const int M = cr.tM;
        auto tb = [&](int l) { return cr.tb.p + cr.tb_off[l - cr.lt]; };
        auto tx = [&](int l) { return cr.tx.p + cr.tb_off[l - cr.lt]; };
        hipLaunchKernelGGL(k_cr_eye, dim3((unsigned)(((int64_t)M * M + 255) / 256)), dim3(256), 0, s, tb(cr.lt), M);
        for (int l = cr.lt; l < cr.nlev; l++) cr_down(cr, l, tb(l), tb(l + 1), M, s);
        cr_final(cr, tb(cr.nlev), tx(cr.nlev), M, s);
        for (int l = cr.nlev - 1; l >= cr.lt; l--) cr_up(cr, l, tb(l), tx(l + 1), tx(l), M, s);
        hipLaunchKernelGGL(k_cr_transpose, dim3((M + 31) / 32, (M + 31) / 32), dim3(256), 0, s,
                           (const double*)tx(cr.lt), cr.tinv.p, M);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int cr_check(iemic_ctx* c, SchurCR& cr)
{
    int info = 0, rc;
    if ((rc = d2h(c, &info, cr.info.p, sizeof(int)))) return rc;
    if (info) {
        set_error("block GS: singular block in the Schur cyclic reduction");
        return IEMIC_EINVAL;
    }
    return 0;
}

}  // namespace iemic
