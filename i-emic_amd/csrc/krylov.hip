/*
 * krylov.hip -- the flexible GMRES driver of the ocean and its reductions.
 *
 *  - fgmres restates Belos BlockGmresSolMgr as configured by Ocean::initializeBelos
 *    (Ocean.C:961-1020): flexible (right) preconditioning, x0 = 0, residual relative to
 *    ||b|| (the preconditioned initial residual for right preconditioning), classical
 *    Gram-Schmidt with one full re-orthogonalisation pass (DGKS-like), Givens updates of
 *    the least-squares problem (hessenberg.h), restarts, and the explicit residual check of
 *    Ocean::solve (Ocean.C:1140-1150).
 *  - The operator is spmv.hip's, IDR(s) is idrs.hip; the element-wise vector kernels and the
 *    multi-dot pair are vec_kernels.h's.
 */
#include <algorithm>
#include <cstdlib>
#include <chrono>
#include <cmath>

#include <hip/hip_ext.h>

#include "common.h"
#include "hessenberg.h"
#include "krylov_internal.h"
#include "vec_kernels.h"

namespace iemic {

/* ---- reductions / DCGS2 -------------------------------------------------------------- */
/* dev_zero's kernel (common.h): the one definition with external linkage */
__global__ void k_zero(double* __restrict__ p, int64_t n)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x)
        p[q] = 0.0;
}

/* w -= sum_i h_i V_i and partial[blk] = block's sum of the new w^2 (grid = RED_BLOCKS) */
__global__ void __launch_bounds__(256) k_mupdate_norm(const double* __restrict__ V, int64_t ldv,
                                                      int nvec, const double* __restrict__ h,
                                                      double* __restrict__ w, int64_t N,
                                                      double* __restrict__ partial)
{
    __shared__ double hs[1024];
    __shared__ double sm[8];
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) hs[i] = h[i];
    __syncthreads();
    double ss = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        double acc = w[q];
        int i = 0;
        for (; i + 4 <= nvec; i += 4) {
            const double* v = V + (int64_t)i * ldv + q;
            acc -= hs[i] * v[0];
            acc -= hs[i + 1] * v[ldv];
            acc -= hs[i + 2] * v[2 * ldv];
            acc -= hs[i + 3] * v[3 * ldv];
        }
        for (; i < nvec; i++) acc -= hs[i] * V[(int64_t)i * ldv + q];
        w[q] = acc;
        ss += acc * acc;
    }
    const double t = block_sum(ss, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

/* sum NV values over the block; result valid in thread 0 (sm: NV*(blockDim/64) doubles) */
template <int NV>
__device__ __forceinline__ void block_sum_n(double* v, double* sm)
{
#pragma unroll
    for (int q = 0; q < NV; q++)
        for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o, 64);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < NV; q++) sm[q * nw + wid] = v[q];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int q = 0; q < NV; q++) {
            double t = 0.0;
            for (int w = 0; w < nw; w++) t += sm[q * nw + w];
            v[q] = t;
        }
}

/* DCGS2 dot pass: rows 2i, 2i+1 = Q_i.u, Q_i.w (i < nvec); rows 2nvec..2nvec+2 = u.u, u.w,
 * w.w.  Block (bx, by), by < ceil(nvec / DG), handles DG basis vectors against u and w over
 * chunk bx; by == nq the three self products.  The group index varies fastest in the block
 * order, so the groups of one chunk run together on one XCD and u, w come from its L2
 * after the first;
 * every lane reads two consecutive elements (16-byte loads; N even, 16-byte aligned).
 * partial[row * nbx + bx].  (scripts/orth_probe.hip: DG = 4 in this order 5.5 TB/s at 89
 * vectors against 4.5 for DG = 8 with the group index slowest.) */
constexpr int DCGS_DG = 4;
static_assert(RED_BLOCKS % 8 == 0, "k_dcgs_dot deals chunks to the 8 XCDs");
__global__ void __launch_bounds__(256) k_dcgs_dot(const double* __restrict__ V, int64_t ldv, int nvec,
                                                  const double* __restrict__ u,
                                                  const double* __restrict__ w, int64_t N,
                                                  double* __restrict__ partial, int nbx)
{
    constexpr int DG = DCGS_DG;
    __shared__ double sm[4 * 2 * DG];
    const int nq = (nvec + DG - 1) / DG;
    /* XCD-aware order (workgroups are dealt to the 8 XCDs round robin): the nq + 1 groups of
     * chunk bx run on XCD bx % 8, launched together, so u and w of the chunk are read from
     * HBM once and from that XCD's L2 by the other groups (nbx % 8 == 0) */
    const int G = nq + 1, sb = blockIdx.x / (8 * G), rem = blockIdx.x % (8 * G);
    const int by = rem / 8, bx = sb * 8 + rem % 8;
    const int64_t N2 = N / 2;
    const int64_t stride = (int64_t)nbx * blockDim.x;
    const int64_t e0 = (int64_t)bx * blockDim.x + threadIdx.x;
    const double2* u2 = reinterpret_cast<const double2*>(u);
    const double2* w2 = reinterpret_cast<const double2*>(w);
    if (by < nq) {
        const int i0 = DG * by;
        const int nv = min(DG, nvec - i0);
        double acc[2 * DG];
#pragma unroll
        for (int t = 0; t < 2 * DG; t++) acc[t] = 0.0;
        const double* q0 = V + (int64_t)i0 * ldv;
        for (int64_t e = e0; e < N2; e += stride) {
            const double2 ue = u2[e], we = w2[e];
#pragma unroll
            for (int t = 0; t < DG; t++) {
                if (t < nv) {
                    const double2 qe = reinterpret_cast<const double2*>(q0 + (int64_t)t * ldv)[e];
                    acc[2 * t] += qe.x * ue.x + qe.y * ue.y;
                    acc[2 * t + 1] += qe.x * we.x + qe.y * we.y;
                }
            }
        }
        block_sum_n<2 * DG>(acc, sm);
        if (threadIdx.x == 0)
            for (int t = 0; t < 2 * nv; t++) partial[(int64_t)(2 * i0 + t) * nbx + bx] = acc[t];
    } else {
        double acc[3] = {0, 0, 0};
        for (int64_t e = e0; e < N2; e += stride) {
            const double2 ue = u2[e], we = w2[e];
            acc[0] += ue.x * ue.x + ue.y * ue.y;
            acc[1] += ue.x * we.x + ue.y * we.y;
            acc[2] += we.x * we.x + we.y * we.y;
        }
        block_sum_n<3>(acc, sm);
        if (threadIdx.x == 0)
            for (int t = 0; t < 3; t++) partial[(int64_t)(2 * nvec + t) * nbx + bx] = acc[t];
    }
}

/* DCGS2 dot pass, one read of everything: a workgroup holds its chunk of u and w in
 * registers (DOT1_E 16-byte elements per lane) and streams every basis vector past them once;
 * each vector's two sums are reduced across the wave and accumulated per wave in LDS
 * (4 x (2 nvec + 3) doubles, dynamic).  Chunks are dealt to the nbx <= RED_BLOCKS workgroups
 * round robin.  partial[row * nbx + bx] as k_dcgs_dot. */
/* 16-byte non-temporal load: the DCGS2 passes stream the basis (up to 1 GB at 2 degrees,
 * past the Infinity Cache) once per pass, and keeping it out of the caches leaves them to
 * u, w and the partial sums (dot pass 84.2 -> 73.7 us, update 84.0 -> 81.7 us,
 * scripts/ab/dcgs_nt.sh) */
__device__ __forceinline__ double2 ldnt2(const double2* p)
{
    typedef double d2v __attribute__((ext_vector_type(2)));
    const d2v v = __builtin_nontemporal_load(reinterpret_cast<const d2v*>(p));
    return make_double2(v.x, v.y);
}
constexpr int DOT1_E = 4;
__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ void __launch_bounds__(256) k_dcgs_dot1(const double* __restrict__ V, int64_t ldv, int nvec,
                                                   const double* __restrict__ u,
                                                   const double* __restrict__ w, int64_t N,
                                                   double* __restrict__ partial, int nbx)
{
    constexpr int E = DOT1_E;
    extern __shared__ double acc_s[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int R = 2 * nvec + 3;
    double* my = acc_s + wid * R;
    for (int t = lane; t < R; t += 64) my[t] = 0.0;
    __syncthreads();
    const int64_t N2 = N / 2, CH = 256 * E;
    const int64_t nch = (N2 + CH - 1) / CH;
    const double2* u2 = reinterpret_cast<const double2*>(u);
    const double2* w2 = reinterpret_cast<const double2*>(w);
    double suu = 0.0, suw = 0.0, sww = 0.0;
    for (int64_t ch = blockIdx.x; ch < nch; ch += nbx) {
        const int64_t e0 = ch * CH + threadIdx.x;
        double2 ue[E], we[E];
#pragma unroll
        for (int k = 0; k < E; k++) {
            const int64_t e = e0 + (int64_t)k * 256;
            ue[k] = e < N2 ? u2[e] : make_double2(0.0, 0.0);
            we[k] = e < N2 ? w2[e] : make_double2(0.0, 0.0);
            suu += ue[k].x * ue[k].x + ue[k].y * ue[k].y;
            suw += ue[k].x * we[k].x + ue[k].y * we[k].y;
            sww += we[k].x * we[k].x + we[k].y * we[k].y;
        }
        /* out-of-range lanes read element 0 of the vector (their u, w are zero) */
        int64_t ex[E];
#pragma unroll
        for (int k = 0; k < E; k++) {
            const int64_t e = e0 + (int64_t)k * 256;
            ex[k] = e < N2 ? e : 0;
        }
        double2 qn[E];
        if (nvec > 0) {
#pragma unroll
            for (int k = 0; k < E; k++) qn[k] = ldnt2(reinterpret_cast<const double2*>(V) + ex[k]);
        }
        for (int i = 0; i < nvec; i++) {
            double2 q[E];
#pragma unroll
            for (int k = 0; k < E; k++) q[k] = qn[k];
            if (i + 1 < nvec) {
                const double2* qv = reinterpret_cast<const double2*>(V + (int64_t)(i + 1) * ldv);
#pragma unroll
                for (int k = 0; k < E; k++) qn[k] = ldnt2(qv + ex[k]);
            }
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int k = 0; k < E; k++) {
                a += q[k].x * ue[k].x + q[k].y * ue[k].y;
                b += q[k].x * we[k].x + q[k].y * we[k].y;
            }
            a = wave_sum(a);
            b = wave_sum(b);
            if (lane == 0) {
                my[2 * i] += a;
                my[2 * i + 1] += b;
            }
        }
    }
    suu = wave_sum(suu);
    suw = wave_sum(suw);
    sww = wave_sum(sww);
    if (lane == 0) {
        my[2 * nvec] += suu;
        my[2 * nvec + 1] += suw;
        my[2 * nvec + 2] += sww;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < R; t += blockDim.x)
        partial[(int64_t)t * nbx + blockIdx.x] = acc_s[t] + acc_s[R + t] + acc_s[2 * R + t] + acc_s[3 * R + t];
}

/* DCGS2 coefficients on the device (no host round trip before the update pass): from the
 * summed dot rows hb = [Q^T u, Q^T w interleaved | u.u, u.w, w.w], beta = sqrt(u.u - |a|^2),
 * h_jj = (u.w - a.b) / beta, gamma = h_jj / beta; the update's coefficients are a and
 * b - gamma a, its scales 1/beta and gamma.  A breakdown (beta = 0) gives zero scales; the
 * host stops on it.  One 256-thread workgroup: the strided partial sums and block_sum_n<2>
 * fix the summation order, so every workgroup that runs this on the same hb gets the same
 * bits. */
struct DcgsScal {
    double bt, hjj, inv_beta, gamma;
};
__device__ __forceinline__ DcgsScal dcgs_scal(const double* __restrict__ hb, int nv)
{
    __shared__ double sm[2 * 4];
    __shared__ double tot[2];
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nv; i += blockDim.x) {
        const double a = hb[2 * i], b = hb[2 * i + 1];
        v[0] += a * a;
        v[1] += a * b;
    }
    block_sum_n<2>(v, sm);
    if (threadIdx.x == 0) {
        tot[0] = v[0];
        tot[1] = v[1];
    }
    __syncthreads();
    const double beta2 = hb[2 * nv] - tot[0];
    const double bt = beta2 > 0.0 ? sqrt(beta2) : 0.0;
    const bool ok = bt > 0.0 && bt <= 1.79e308;
    const double hjj = ok ? (hb[2 * nv + 1] - tot[1]) / bt : 0.0;
    const double gamma = ok ? hjj / bt : 0.0;
    return DcgsScal{bt, hjj, ok ? 1.0 / bt : 0.0, gamma};
}
/* beta, h_jj appended to hb (rows 2nv+3, 2nv+4) for the host's Hessenberg column, and the
 * rows straight into its pinned (coherent) slot: no device-to-host copy launch per Arnoldi
 * step.  One workgroup calls this, all its threads. */
__device__ __forceinline__ void dcgs_rows_out(double* __restrict__ hb, int nv, const DcgsScal& sc,
                                              double* __restrict__ hrows)
{
    if (threadIdx.x == 0) {
        hb[2 * nv + 3] = sc.bt;
        hb[2 * nv + 4] = sc.hjj;
    }
    if (hrows) {
        for (int i = threadIdx.x; i < 2 * nv + 3; i += blockDim.x) hrows[i] = hb[i];
        if (threadIdx.x == 0) {
            hrows[2 * nv + 3] = sc.bt;
            hrows[2 * nv + 4] = sc.hjj;
        }
    }
}
/* The coefficients as a launch of their own: coef = [a | b - gamma a], coef[DCGS_SCAL..] =
 * 1/beta, gamma.  The solve runs it only where no update pass follows (the last step of a
 * full cycle); it is also the reference the fused update is tested against. */
__global__ void __launch_bounds__(256) k_dcgs_coef(double* __restrict__ hb, int nv, double* __restrict__ coef,
                                                   double* __restrict__ hrows)
{
    const DcgsScal sc = dcgs_scal(hb, nv);
    for (int i = threadIdx.x; i < nv; i += blockDim.x) {
        const double a = hb[2 * i], b = hb[2 * i + 1];
        coef[i] = a;
        coef[nv + i] = b - a * sc.gamma;
    }
    if (threadIdx.x == 0) {
        coef[DCGS_SCAL] = sc.inv_beta;
        coef[DCGS_SCAL + 1] = sc.gamma;
    }
    dcgs_rows_out(hb, nv, sc, hrows);
}

/* DCGS2 update pass, one read of Q:  q_j = (u - Q a) * inv_beta,
 * w = (w - Q c - gamma * u) * inv_beta; u is overwritten by q_j.  Scaling the next candidate
 * w by the same 1/beta (lagged normalisation) keeps every candidate at the scale of a
 * normalised Arnoldi vector, so its norm never compounds the earlier subdiagonals (no
 * overflow / false breakdown over long cycles). */
/* FUSED: every workgroup forms a, c, inv_beta and gamma itself from the summed dot rows hb
 * (dcgs_scal: the bits of k_dcgs_coef, no workgroup depends on another), so no coefficient
 * launch sits between the dot pass and this one; workgroup 0 writes beta, h_jj and the
 * host's rows (hb rows 2nv+3.. are read by no workgroup).  !FUSED: hb is the ready
 * coefficient array of k_dcgs_coef (coef = [a (nvec) | c (nvec)], scales at DCGS_SCAL). */
/* rrP (the compressed basis with the block GS): the new candidate w -- the next step's
 * preconditioner input -- also goes straight into the block GS's planar right-hand side
 * (rows 2e, 2e + 1 of w are unknowns R, R + 1 of active cell act[2e / 6]), so the apply
 * skips its entry kernel k_gs_rr_c */
template <bool FUSED>
__global__ void __launch_bounds__(256) k_dcgs_update(const double* __restrict__ V, int64_t ldv,
                                                     int nvec, double* __restrict__ hb,
                                                     double* __restrict__ hrows,
                                                     double* __restrict__ u, double* __restrict__ w,
                                                     int64_t N, const int* __restrict__ act = nullptr,
                                                     int64_t own0 = 0, int64_t ps = 0,
                                                     double* __restrict__ rrP = nullptr)
{
    /* two consecutive elements per lane (16-byte loads; N even), four basis vectors per step */
    constexpr int UN = 4;
    __shared__ double cs[2 * 1024];
    double inv_beta, gamma;
    if (FUSED) {
        const DcgsScal sc = dcgs_scal(hb, nvec);
        for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
            const double a = hb[2 * i], b = hb[2 * i + 1];
            cs[i] = a;
            cs[nvec + i] = b - a * sc.gamma;
        }
        if (blockIdx.x == 0) dcgs_rows_out(hb, nvec, sc, hrows);
        inv_beta = sc.inv_beta;
        gamma = sc.gamma;
    } else {
        for (int i = threadIdx.x; i < 2 * nvec; i += blockDim.x) cs[i] = hb[i];
        inv_beta = hb[DCGS_SCAL];
        gamma = hb[DCGS_SCAL + 1];
    }
    __syncthreads();
    const double* a = cs;
    const double* cc = cs + nvec;
    const int64_t N2 = N / 2;
    double2* u2 = reinterpret_cast<double2*>(u);
    double2* w2 = reinterpret_cast<double2*>(w);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < N2;
         e += (int64_t)gridDim.x * blockDim.x) {
        double sux = 0.0, suy = 0.0, swx = 0.0, swy = 0.0;
        int i = 0;
        for (; i + UN <= nvec; i += UN) {
            double2 q[UN];
#pragma unroll
            for (int k = 0; k < UN; k++) q[k] = ldnt2(reinterpret_cast<const double2*>(V + (int64_t)(i + k) * ldv) + e);
#pragma unroll
            for (int k = 0; k < UN; k++) {
                sux += a[i + k] * q[k].x;
                suy += a[i + k] * q[k].y;
                swx += cc[i + k] * q[k].x;
                swy += cc[i + k] * q[k].y;
            }
        }
        for (; i < nvec; i++) {
            const double2 q = ldnt2(reinterpret_cast<const double2*>(V + (int64_t)i * ldv) + e);
            sux += a[i] * q.x;
            suy += a[i] * q.y;
            swx += cc[i] * q.x;
            swy += cc[i] * q.y;
        }
        const double2 ue = u2[e], we = w2[e];
        u2[e] = make_double2((ue.x - sux) * inv_beta, (ue.y - suy) * inv_beta);
        const double2 wn = make_double2((we.x - swx - gamma * ue.x) * inv_beta, (we.y - swy - gamma * ue.y) * inv_beta);
        w2[e] = wn;
        if (rrP) {
            const int64_t a = e / 3, R = 2 * e - 6 * a, cell = own0 + act[a];
            rrP[cell + R * ps] = wn.x;
            rrP[cell + (R + 1) * ps] = wn.y;
        }
    }
}

/* the update pass of one Arnoldi step on the context's stream: fused (the solve), or
 * k_dcgs_coef and the update from its coefficient array (the test hook's reference).  hb:
 * the summed dot rows, coef: RED_ROWS doubles, hrows: the host's pinned slot or null */
int dcgs_update(iemic_ctx* c, bool fused, const double* Q, int64_t ldq, int nv, double* hb, double* coef,
                double* hrows, double* u, double* w, int64_t N, const int* act, int64_t own0, int64_t ps,
                double* rrP)
{
    const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (N / 2 + 255) / 256)));
    if (fused) {
        hipLaunchKernelGGL(k_dcgs_update<true>, g, dim3(256), 0, c->stream, Q, ldq, nv, hb, hrows, u, w, N, act,
                           own0, ps, rrP);
    } else {
        hipLaunchKernelGGL(k_dcgs_coef, dim3(1), dim3(256), 0, c->stream, hb, nv, coef, hrows);
        hipLaunchKernelGGL(k_dcgs_update<false>, g, dim3(256), 0, c->stream, Q, ldq, nv, coef, (double*)nullptr, u,
                           w, N, act, own0, ps, rrP);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

/* x += sum_i y_i Z_i */
__global__ void __launch_bounds__(256) k_mupdate_add(const double* __restrict__ Z, int64_t ldz, int nvec,
                                                     const double* __restrict__ y,
                                                     double* __restrict__ x, int64_t N)
{
    __shared__ double ys[1024];
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) ys[i] = y[i];
    __syncthreads();
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < N;
         q += (int64_t)gridDim.x * blockDim.x) {
        double acc = x[q];
        for (int i = 0; i < nvec; i++) acc += ys[i] * Z[(int64_t)i * ldz + q];
        x[q] = acc;
    }
}

/* dot products of nvec vectors V_i (stride ldv) with w, and (ea != null) ea . eb as
 * out[nvec], in one launch pair and one host synchronisation */
/* V, w, ea, eb point at the first owned row; length nlrows; sums over the ranks */
int mdot_host(iemic_ctx* c, const double* V, int64_t ldv, int nvec, const double* w,
              double* out, const double* ea, const double* eb)
{
    const int64_t N = c->sub.nlrows();
    const int nout = nvec + (ea ? 1 : 0);
    hipLaunchKernelGGL(k_mdot, dim3(RED_BLOCKS, nout), dim3(256), 0, c->stream, V, ldv, nvec, w, N,
                       c->d_part.p, ea, eb);
    hipLaunchKernelGGL(k_mdot_final, dim3(nout), dim3(256), 0, c->stream, c->d_part.p, RED_BLOCKS,
                       nout, c->d_hbuf.p);
    int rc = allreduce_sum(c, c->d_hbuf.p, nout);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(c->h_red, c->d_hbuf.p, sizeof(double) * nout, hipMemcpyDeviceToHost,
                          c->stream));
    DEV_SYNC(c);
    for (int i = 0; i < nout; i++) out[i] = c->h_red[i];
    return 0;
}

/* a . b over the owned rows of two ext vectors, summed over the ranks (error code) */
int dot_owned(iemic_ctx* c, const double* a, const double* b, double* out)
{
    const int64_t o = owned(c).o;
    return mdot_host(c, a + o, 0, 1, b + o, out);
}

/* a . b over the owned rows of two ext vectors, summed over the ranks */
double dot(iemic_ctx* c, const double* a, const double* b, int64_t)
{
    const int64_t o = owned(c).o;
    double r = 0.0;
    if (mdot_host(c, a + o, 0, 1, b + o, &r)) return NAN;
    return r;
}

/* One Gram-Schmidt pass over the nvec basis vectors: h = V^T w, ww0 = w.w (before),
 * w -= V h, ww1 = w.w (after).  The coefficients stay on the device between the two
 * launches; one device-to-host copy + synchronisation returns h, ww0, ww1. */
static int orth_pass(iemic_ctx* c, const double* V, int64_t ldv, int nvec, double* w, double* h,
                     double* ww0, double* ww1)
{
    const int64_t N = c->sub.nlrows();
    hipLaunchKernelGGL(k_mdot, dim3(RED_BLOCKS, nvec + 1), dim3(256), 0, c->stream, V, ldv, nvec,
                       w, N, c->d_part.p, (const double*)w);
    hipLaunchKernelGGL(k_mdot_final, dim3(nvec + 1), dim3(256), 0, c->stream, c->d_part.p,
                       RED_BLOCKS, nvec + 1, c->d_hbuf.p);
    int rc = allreduce_sum(c, c->d_hbuf.p, nvec + 1);   /* coefficients summed before use */
    if (rc) return rc;
    hipLaunchKernelGGL(k_mupdate_norm, dim3(RED_BLOCKS), dim3(256), 0, c->stream, V, ldv, nvec,
                       c->d_hbuf.p, w, N, c->d_part.p);
    hipLaunchKernelGGL(k_mdot_final, dim3(1), dim3(256), 0, c->stream, c->d_part.p, RED_BLOCKS, 1,
                       c->d_hbuf.p + nvec + 1);
    if ((rc = allreduce_sum(c, c->d_hbuf.p + nvec + 1, 1))) return rc;
    HIP_OK(hipMemcpyAsync(c->h_red, c->d_hbuf.p, sizeof(double) * (nvec + 2), hipMemcpyDeviceToHost,
                          c->stream));
    DEV_SYNC(c);
    for (int i = 0; i < nvec; i++) h[i] = c->h_red[i];
    *ww0 = c->h_red[nvec];
    *ww1 = c->h_red[nvec + 1];
    return 0;
}

/* the Krylov work space: Z (m x N) and w, r always; the full-length basis V ((m+1) x N) unless
 * the basis is compressed, then Vc ((m+1) x nc) and the full-length t, b' */
int ensure_krylov(iemic_ctx* c, int m, int64_t nc)
{
    Krylov& k = c->kr;
    const int64_t N = c->sub.nerows();
    int rc = 0;
    if (k.m < m || !k.Z.p) {
        k.zclean = 0;
        k.V.free();                  /* sized by m: reallocated below when needed */
        rc |= k.Z.alloc((size_t)m * N);
        rc |= k.w.alloc(N);
        rc |= k.r.alloc(N);
        if (rc) {
            set_error("fgmres: out of device memory for the Krylov basis");
            return IEMIC_ENOMEM;
        }
        k.m = m;
    }
    if (!nc && !k.V.p) {
        if (k.V.alloc((size_t)(k.m + 1) * N)) {
            set_error("fgmres: out of device memory for the Krylov basis");
            return IEMIC_ENOMEM;
        }
    }
    if (nc && (k.mc < m || k.nc < nc || !k.Vc.p)) {
        rc |= k.Vc.alloc((size_t)(m + 1) * nc);
        if (!k.t.p) rc |= k.t.alloc(N) | k.bp.alloc(N);
        if (rc) {
            set_error("fgmres: out of device memory for the Krylov basis");
            return IEMIC_ENOMEM;
        }
        k.mc = m;
        k.nc = nc;
    }
    return 0;
}

/* the compressed Arnoldi basis: rows of the active cells act[] (6 per cell), in order */
__global__ void k_cgather(const double* __restrict__ full, const int* __restrict__ act, int64_t nc,
                          int64_t own0, double s, double* __restrict__ cmp)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nc;
         q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t cl = q / NUN;
        cmp[q] = s * full[NUN * (own0 + act[cl]) + (q - NUN * cl)];
    }
}
/* t = v on the identity rows (known), 0 elsewhere (owned rows) */
__global__ void k_known_part(const double* __restrict__ v, const uint8_t* __restrict__ known, int64_t n0,
                             int64_t nl, double* __restrict__ t)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nl;
         q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = n0 + q;
        t[r] = known[r] ? v[r] : 0.0;
    }
}

/* coefficients -> device through the pinned staging area (the previous use of the area
 * has completed: every caller synchronised the stream since) */
int upload_coeffs(iemic_ctx* c, const double* h, int n)
{
    if (n > RED_ROWS) {
        set_error("upload_coeffs: too many coefficients");
        return IEMIC_EINVAL;
    }
    double* st = c->h_red + RED_ROWS;
    for (int i = 0; i < n; i++) st[i] = h[i];
    HIP_OK(hipMemcpyAsync(c->d_hbuf.p + RED_ROWS, st, sizeof(double) * n,
                          hipMemcpyHostToDevice, c->stream));
    return 0;
}

/* a NaN/Inf reaching the Hessenberg column would pass for a breakdown (res = 0): stop loudly */
int nonfinite()
{
    set_error("FGMRES: non-finite value in the Krylov basis (operator or preconditioner output)");
    return IEMIC_ERANGE;
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

/* a restart cycle of at least STAG_MIN steps that cut the true residual by less than
 * 1 / STAG_RATIO counts as stagnation (a converging cycle at the 2-degree bench state cuts it
 * by ~1e-3, one at the 1-degree continuation tolerance by ~30) */
constexpr double STAG_RATIO = 0.25;
constexpr int STAG_MIN = 20;

int fgmres(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt, iemic_solve_info* info)
{
    /* vectors are ext-layout (stride NE); kernels touch the owned rows [o, o + NL) */
    const int m = std::max(1, std::min(opt->krylov_dim, MAX_KRYLOV));
    const Owned ow = owned(c);         /* o, NL are named: the DCGS2 loop's lambda captures them */
    const int64_t NE = c->sub.nerows(), o = ow.o, NL = ow.n;
    /* DCGS2 with the block GS: the Arnoldi basis on the active cells only.  Identity rows of J
     * (all rows of a land cell, some of an ocean cell) are identity rows of the preconditioner
     * too, so with a right-hand side that is zero on them every Krylov vector is exactly zero
     * there: the basis skips the land cells (48 % of the rows at 2 degrees), the block GS
     * reads it without the identity-column couplings and the SpMV writes only the active
     * cells.  A right-hand side with identity-row entries is first reduced: x_k = b_k,
     * b' = b - J t (t = b on the identity rows), zero on them. */
    const BlockGS& gs = c->gs;
    int rc = opt->prec > 0 ? gs_refresh(c) : 0;
    if (rc) return rc;
    const bool cmp = opt->orth == 0 && opt->prec == 2 && gs.ready && gs.kind == 2 && gs.act.nact > 0 && gs.act.cmap.p &&
                     gs.act.cmp_ok && gs.act.spc.p && gs.act.atl.p;
    const int64_t NC = cmp ? NUN * gs.act.nact : 0;
    rc = ensure_krylov(c, m, NC);
    if (rc) return rc;
    /* the staged applies (gs_apply_c after an update pass) leave the identity rows of the
     * preconditioned vectors Z alone: zero them once per set-up, the other solvers may have
     * left values there.  kr.zclean counts the leading columns already zeroed: a solve with a
     * larger m than the one that cleaned zeroes the columns in between */
    if (cmp && c->kr.zclean < m) {
        const int z0 = c->kr.zclean;
        if ((rc = dev_zero(c, c->kr.Z.p + (int64_t)z0 * NE, (int64_t)(m - z0) * NE))) return rc;
        c->kr.zclean = m;
    } else if (!cmp) {
        c->kr.zclean = 0;
    }
    iemic_solve_info inf{};
    auto T0 = std::chrono::steady_clock::now();
    double* V = cmp ? nullptr : c->kr.V.p;
    double* Vc = cmp ? c->kr.Vc.p : nullptr;
    double* Z = c->kr.Z.p;
    double* w = c->kr.w.p;
    double* r = c->kr.r.p;
    const unsigned G = ow.grid;
    const unsigned GC = grid_for(NC);
    Hessenberg hess(m);
    std::vector<double> h(m + 1), h2(m + 1), y(m);
    std::vector<double> zs(m + 1, 1.0);   /* DCGS2: scale of the stored z_j (1 for DGKS) */
    if (2 * m + 5 > RED_ROWS) {
        set_error("fgmres: Krylov dimension too large");
        return IEMIC_EINVAL;
    }
    int inf_reorth = 0;
    /* prec / SpMV timing events (two sets: the DCGS2 loop runs one iteration ahead) and the
     * DCGS2 row-copy events */
    struct Events {
        hipEvent_t e[8] = {};
        ~Events() { for (auto& x : e) if (x) (void)hipEventDestroy(x); }
    } evs;
    hipEvent_t* ev = evs.e;
    hipEvent_t* evr = evs.e + 6;
    for (int q = 0; q < 6; q++) HIP_OK(hipEventCreate(&ev[q]));
    for (int q = 6; q < 8; q++) HIP_OK(hipEventCreateWithFlags(&evs.e[q], hipEventDisableTiming));

    if ((rc = dev_zero(c, x, NE))) return rc;
    double bnorm = sqrt0(dot(c, b, b, 0));
    if (!std::isfinite(bnorm)) return nonfinite();
    if (!(bnorm > 0)) {
        inf.converged = 1;
        if (info) *info = inf;
        return 0;
    }
    const double* b_orig = b;
    bool known_rhs = false;
    if (cmp) {
        double* t = c->kr.t.p;
        hipLaunchKernelGGL(k_known_part, dim3(G), dim3(256), 0, c->stream, b, gs.known.p, o, NL, t);
        if (dot(c, t, t, 0) > 0.0) {
            known_rhs = true;
            if ((rc = spmv(c, t, w, c->stream))) return rc;
            hipLaunchKernelGGL(k_axpby, dim3(G), dim3(256), 0, c->stream, 1.0, b + o, -1.0, w + o,
                               c->kr.bp.p + o, NL);
            b = c->kr.bp.p;
        }
    }
    /* r = b (x0 = 0) */
    HIP_OK(hipMemcpyAsync(r, b, sizeof(double) * NE, hipMemcpyDeviceToDevice, c->stream));
    double beta = known_rhs ? sqrt0(dot(c, b, b, 0)) : bnorm, res = beta / bnorm, res_c0 = res;
    int it = 0;
    /* the safeguard's switch lasts for this solve only */
    struct Restore {
        iemic_ctx* c;
        int mr;
        ~Restore() { c->gs.dyn_mr = mr; }
    } restore{c, c->gs.dyn_mr};
    /* beta = 0: a right-hand side on the land rows only, solved by x = t below */
    for (int cycle = 0; beta > 0.0 && cycle <= opt->max_restarts; cycle++) {
        const int it_c0 = it;
        if (cmp)
            hipLaunchKernelGGL(k_cgather, dim3(GC), dim3(256), 0, c->stream, r, gs.act.act.p, NC, c->sub.own0,
                               1.0 / beta, Vc);
        else
            hipLaunchKernelGGL(k_scale_copy, dim3(G), dim3(256), 0, c->stream, r + o, 1.0 / beta, V + o, NL);
        hess.reset(beta);
        int j = 0;
        if (opt->orth == 1) {
            for (; j < m; j++) {
                double* vj = V + (int64_t)j * NE;
                double* zj = Z + (int64_t)j * NE;
                double* vn = V + (int64_t)(j + 1) * NE;
                /* prec and SpMV are timed with events (no extra host synchronisation) */
                HIP_OK(hipEventRecord(ev[0], c->stream));
                if (opt->prec > 0) {
                    rc = prec_apply(c, vj, zj);
                    if (rc) return rc;
                } else {
                    HIP_OK(hipMemcpyAsync(zj, vj, sizeof(double) * NE, hipMemcpyDeviceToDevice, c->stream));
                }
                HIP_OK(hipEventRecord(ev[1], c->stream));
                rc = spmv(c, zj, vn, c->stream);
                if (rc) return rc;
                HIP_OK(hipEventRecord(ev[2], c->stream));

                /* DGKS (Belos' default orthogonalisation): one classical Gram-Schmidt pass
                 * h = V^T w (with ||w||^2 in the same launch), w -= V h (with ||w||^2 fused),
                 * and a second pass only when the norm dropped below 1/sqrt(2) of its value
                 * (dep_tol, BelosDGKSOrthoManager).  One host synchronisation per pass. */
                double hn2 = 0.0;
                {
                    double ww0 = 0.0;
                    rc = orth_pass(c, V + o, NE, j + 1, vn + o, h.data(), &ww0, &hn2);
                    if (rc) return rc;
                    if (hn2 < 0.5 * ww0) {
                        double dummy = 0.0;
                        rc = orth_pass(c, V + o, NE, j + 1, vn + o, h2.data(), &dummy, &hn2);
                        if (rc) return rc;
                        for (int i = 0; i <= j; i++) h[i] += h2[i];
                        inf_reorth++;
                    }
                }
                if (!std::isfinite(hn2)) return nonfinite();
                double hn = sqrt0(hn2);
                if (hn > 0)
                    hipLaunchKernelGGL(k_scale_copy, dim3(G), dim3(256), 0, c->stream, vn + o, 1.0 / hn,
                                       vn + o, NL);
                {
                    float a1 = 0.f, a2 = 0.f;
                    (void)hipEventElapsedTime(&a1, ev[0], ev[1]);
                    (void)hipEventElapsedTime(&a2, ev[1], ev[2]);
                    inf.t_prec_ms += a1;
                    inf.t_spmv_ms += a2;
                    inf.n_spmv++;
                }
                res = hess.push_column(j, h.data(), hn) / bnorm;
                it++;
                if (res <= opt->tol || hn == 0.0) {
                    j++;
                    break;
                }
            }
        } else {
            /* DCGS2 (delayed classical Gram-Schmidt with reorthogonalisation): the new
             * vector u_j is orthogonalised once when produced and re-orthogonalised one step
             * later in the same pass over the basis that orthogonalises the next candidate;
             * normalisation is folded in.  One read pass (k_dcgs_dot) + one update pass
             * (k_dcgs_update) over the basis per iteration; the Hessenberg column j-1 is final
             * (and the residual known) at iteration j.
             * Pipelined: the update pass forms its coefficients on the device (dcgs_scal), so the
             * host enqueues iteration jj+1 (update, preconditioner, SpMV, dot pass) before it
             * waits for iteration jj's dot rows; the queue never drains on a host round trip.
             * The one speculative iteration past convergence only touches columns the
             * solution update does not read. */
            std::vector<double> htent(m + 1), col(m + 1);
            int ncolf = 0;                 /* finalised columns */
            /* the basis: compressed (Vc, stride NC, from row 0) or the ext vectors' owned rows */
            double* const Q = cmp ? Vc : V + o;
            const int64_t LQ = cmp ? NC : NE, NQ = cmp ? NC : NL;
            const int nbx1 = (int)std::min<int64_t>(RED_BLOCKS, (NQ / 2 + 256 * DOT1_E - 1) / (256 * DOT1_E));
            /* z_jj = M u_jj with u_jj of norm bt_jj: the Hessenberg column of z_jj / bt_jj is
             * the one assembled below, so the solution update divides y_jj by bt_jj */
            std::fill(zs.begin(), zs.end(), 1.0);
            /* iteration jj: prec, SpMV, dot pass, update (coefficients in its prologue, rows ->
             * pinned slot jj % 2) */
            auto enqueue = [&](int jj) -> int {
                double* u = Q + (int64_t)jj * LQ;
                double* wv = jj < m ? Q + (int64_t)(jj + 1) * LQ : nullptr;
                hipEvent_t* e = ev + 3 * (jj & 1);
                int rc2;
                if (jj < m) {
                    double* zj = Z + (int64_t)jj * NE;
                    HIP_OK(hipEventRecord(e[0], c->stream));
                    if (cmp) {
                        /* the block GS reads the compressed u (staged into its planar right-hand
                         * side by the previous update pass, jj > 0), the SpMV writes the
                         * compressed w */
                        if ((rc2 = gs_apply_c(c, u, zj, jj > 0))) return rc2;
                    } else if (opt->prec > 0) {
                        if ((rc2 = prec_apply(c, u - o, zj))) return rc2;
                    } else {
                        HIP_OK(hipMemcpyAsync(zj, u - o, sizeof(double) * NE, hipMemcpyDeviceToDevice,
                                              c->stream));
                    }
                    if (cmp) {
                        /* e[1] .. e[2]: the SpMV kernel alone (bench.py's roofline.launch_us) */
                        if ((rc2 = halo_exchange(c, zj, 1))) return rc2;
                        if ((rc2 = spmv_kernel_c(c, zj, wv, e[1], e[2]))) return rc2;
                    } else {
                        HIP_OK(hipEventRecord(e[1], c->stream));
                        if ((rc2 = spmv(c, zj, wv - o, c->stream))) return rc2;
                        HIP_OK(hipEventRecord(e[2], c->stream));
                    }
                }
                /* dot pass: a = Q^T u, b = Q^T w, u.u, u.w, w.w (Q = V_0..jj-1), summed over ranks */
                const int nv = jj;
                const double* wd = wv ? wv : u;
                hipLaunchKernelGGL(k_dcgs_dot1, dim3(nbx1), dim3(256), sizeof(double) * 4 * (2 * nv + 3),
                                   c->stream, Q, LQ, nv, u, wd, NQ, c->d_part.p, nbx1);
                hipLaunchKernelGGL(k_mdot_final, dim3(2 * nv + 3), dim3(256), 0, c->stream, c->d_part.p,
                                   nbx1, 2 * nv + 3, c->d_hbuf.p);
                if ((rc2 = allreduce_sum(c, c->d_hbuf.p, 2 * nv + 3))) return rc2;
                /* the update forms its coefficients itself and its first workgroup writes the
                 * host's rows, so the rows' event follows it; the step after a full cycle's
                 * last column has no update and gets the rows from k_dcgs_coef */
                double* hrows = c->h_red + (size_t)RED_ROWS * (jj & 1);
                if (jj < m) {
                    if ((rc2 = dcgs_update(c, true, Q, LQ, nv, c->d_hbuf.p, nullptr, hrows, u, wv, NQ,
                                           cmp ? (const int*)gs.act.act.p : nullptr, c->sub.own0,
                                           (int64_t)c->sub.next, cmp ? gs.rrP.p : nullptr)))
                        return rc2;
                } else {
                    hipLaunchKernelGGL(k_dcgs_coef, dim3(1), dim3(256), 0, c->stream, c->d_hbuf.p, nv,
                                       c->d_hbuf.p + RED_ROWS, hrows);
                }
                HIP_OK(hipEventRecord(evr[jj & 1], c->stream));
                return 0;
            };
            if ((rc = enqueue(0))) return rc;
            for (int jj = 0; jj <= m; jj++) {
                if (jj < m && (rc = enqueue(jj + 1))) return rc;
                DEV_WAIT_EVENT(c, evr[jj & 1]);
                if (jj < m) {
                    float a1 = 0.f, a2 = 0.f;
                    hipEvent_t* e = ev + 3 * (jj & 1);
                    (void)hipEventElapsedTime(&a1, e[0], e[1]);
                    (void)hipEventElapsedTime(&a2, e[1], e[2]);
                    inf.t_prec_ms += a1;
                    inf.t_spmv_ms += a2;
                    inf.n_spmv++;
                }
                const int nv = jj;
                const double* hr = c->h_red + (size_t)RED_ROWS * (jj & 1);
                const double uu = hr[2 * nv], uw = hr[2 * nv + 1];
                if (!std::isfinite(uu) || !std::isfinite(uw)) {
                    (void)dev_wait(c, nullptr, "fgmres");
                    return nonfinite();
                }
                const double bt = hr[2 * nv + 3], hjj = hr[2 * nv + 4];
                bool stop = false;
                if (jj >= 1) {
                    /* finalise column jj-1: tentative + reorthogonalisation coefficients */
                    const int q = jj - 1;
                    for (int i = 0; i < jj; i++) col[i] = htent[i] + hr[2 * i];
                    res = hess.push_column(q, col.data(), bt) / bnorm;
                    ncolf = jj;
                    it++;
                    stop = res <= opt->tol || !(bt > 0.0);
                }
                if (stop || jj == m || !(bt > 0.0)) break;
                /* the update pass (already enqueued): q_jj = (u - Q a)/bt,  w -= Q c + gamma u */
                for (int i = 0; i < nv; i++) htent[i] = hr[2 * i + 1] / bt;
                htent[nv] = hjj / bt;
                zs[jj] = bt;
            }
            /* the speculative iteration and its copy into the pinned slots finish before the
             * slots are reused as the staging area of the solution update */
            DEV_SYNC(c);
            j = ncolf;
        }
        /* y = H \ g ; x += Z y */
        int k = j;
        hess.solve(k, y.data());
        if (k > 0) {
            for (int i = 0; i < k; i++) y[i] /= zs[i];
            if ((rc = upload_coeffs(c, y.data(), k))) return rc;
            hipLaunchKernelGGL(k_mupdate_add, dim3(G), dim3(256), 0, c->stream, Z + o, NE, k,
                               c->d_hbuf.p + RED_ROWS, x + o, NL);
        }
        if (cycle == opt->max_restarts) break;
        /* r = b - J x; a cycle that converged on the implicit (Givens) estimate restarts
         * only if the true residual has not reached the tolerance */
        rc = spmv(c, x, r, c->stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_axpby, dim3(G), dim3(256), 0, c->stream, 1.0, b + o, -1.0, r + o, r + o, NL);
        beta = sqrt0(dot(c, r, r, 0));
        res = beta / bnorm;
        if (res <= opt->tol) break;
        /* stagnation: switch the preconditioner to its safe variant (FGMRES is flexible) */
        if (opt->prec == 2 && it - it_c0 >= STAG_MIN && res > STAG_RATIO * res_c0 && prec_safeguard(c))
            inf.safeguard++;
        res_c0 = res;
    }
    /* the identity-row part of a reduced right-hand side: x = x' + t */
    if (known_rhs)
        hipLaunchKernelGGL(k_axpby, dim3(G), dim3(256), 0, c->stream, 1.0, x + o, 1.0, c->kr.t.p + o, x + o, NL);
    b = b_orig;
    /* explicit residual (Ocean.C:1140-1150) */
    rc = spmv(c, x, w, c->stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_axpby, dim3(G), dim3(256), 0, c->stream, 1.0, b + o, -1.0, w + o, w + o, NL);
    double e2 = dot(c, w, w, 0);
    inf.iters = it;
    inf.reorth = inf_reorth;
    inf.implicit_rel_res = res;
    inf.explicit_rel_res = sqrt0(e2) / bnorm;
    /* converged: the Givens estimate reached the tolerance and the true residual agrees
     * with it (a loss of orthogonality shows up as a gap between the two) */
    inf.converged = res <= opt->tol && inf.explicit_rel_res <= 2.0 * opt->tol;
    inf.t_total_ms = ms_since(T0);
    /* everything that is not the (event-timed) preconditioner or SpMV: Gram-Schmidt
     * passes, reductions, host synchronisation and the Hessenberg work */
    inf.t_orth_ms = std::max(0.0, inf.t_total_ms - inf.t_prec_ms - inf.t_spmv_ms);
    HIP_OK(hipGetLastError());
    if (info) *info = inf;
    return 0;
}

}  // namespace iemic

namespace iemic {
int krylov_solve(iemic_ctx* c, const double* b, double* x, const iemic_krylov* opt, iemic_solve_info* info)
{
    c->ncalls[0]++;
    if (opt->method == 1) return idrs(c, b, x, opt, info);
    if (opt->method != 0) {
        set_error("krylov: unknown method");
        return IEMIC_EINVAL;
    }
    return fgmres(c, b, x, opt, info);
}
}  // namespace iemic
