// beta_centred.hip -- the centred update of the mean function's coefficients: exact Gibbs for beta_j with g_j = f_j + mu_j held
// fixed (gpirt_sampler_draw_beta_centred, sampler.hip; include/gpirt_hip.h has the contract, DESIGN.md section 44 the reasons).
//
// draw_beta moves beta_j under a fixed f_j, so it changes g_j, which thousands of answers per item pin down: only tiny steps are
// accepted and the linear trend wanders between f_j and mu_j as slowly as draw_f lets it.  This move changes beta_j and f_j
// together with g_j fixed.  The likelihood does not change, there is no accept step, and with X = [1, theta], S = K + eps I and
// f_j = g_j - X beta_j ~ N(0, a_j^2 S) the conditional of beta_j is Gaussian:
//       Lam_j = B / a_j^2 + diag(1 / s0^2),   b_j = (W^T f_j + B beta_j) / a_j^2 + m0 / s0^2,   B = X^T S^-1 X,   W = S^-1 X.
// On the rank-64 identity K = Phi Phi^T, Phi = V F (V the Lagrange basis at theta, Kcc = F F^T with its dead columns zeroed as
// the centred amplitude update keeps it), W = (X - Phi A^-1 Phi^T X) / eps with A = Phi^T Phi + eps I = R R^T: no factor of S.
//
// The launches, all on the caller's stream, no host read, no atomics but the error word, one writer per value:
//   launch_nu_lr_basis             V (n x 64) from theta
//   launch_gemm_splitk             Gv = V^T V, the parts added in index order
//   fstar_free_xhat (with R)       Xh = R^-1 F^T and R, one work-group (fstar_free.hip); a bad pivot raises *err
//   beta_centred_p_kernel          P = V^T X (64 x 2), one work-group per node
//   beta_centred_gx_kernel         u = Xh P, Gx = Xh^T u (64 x 2), one work-group
//   beta_centred_w_kernel          W (n x 2), one thread per row
//   beta_centred_b_kernel          B (2 x 2), one work-group
//   beta_centred_item_kernel       per item: T_j = W^T f_j, the 2 x 2 draw, the rewrite of f_j, mu_j and mu_star_j
//
// THE ORDER OF EVERY OPERATION (fma where written, nothing else contracted):
//   ROW ORDER: thread t of 256 takes the rows t, t + 256, ... ascending into one accumulator that starts at 0, then the 256
//              accumulators are added by the fixed LDS tree s = 128, 64, .., 1: acc[t] += acc[t + s] (ell_delta_kernel's).
//   P[c, 0]  = sum_i V[i, c] in row order (plain sums);  P[c, 1] = fma(V[i, c], theta_i, .) in row order
//   u[k, q]  = fma(Xh(k, i), P[i, q], .) over i = 0 .. 63 ascending from 0
//   Gx[c, q] = fma(Xh(k, c), u[k, q], .) over k = 0 .. 63 ascending from 0
//   W[i, q]  = (X[i, q] - s) / eps, s = fma(V[i, c], Gx[c, q], .) over c = 0 .. 63 ascending from 0, X[i, 0] = 1, X[i, 1] = theta_i
//   B00      = sum_i W[i, 0] in row order (plain sums);  B01 = B10 = fma(W[i, 0], theta_i, .);  B11 = fma(W[i, 1], theta_i, .)
//   T_j[q]   = fma(W[i, q], f[i, j], .) in row order
//   ia = 1 / (a_j a_j)                     one product, one division; a_j = 1.0 exactly when the amplitudes are off
//   p_q = 1 / (s0_q s0_q)                  one product, one division
//   b_q = (T_j[q] + (B_q0 beta_0 + B_q1 beta_1)) ia + m0_q p_q             products, the inner sum, the outer sum, product, product, sum
//   Lam00 = B00 ia + p_0,  Lam10 = B10 ia,  Lam11 = B11 ia + p_1
//   c00 = sqrt(Lam00),  c10 = Lam10 / c00,  c11 = sqrt(Lam11 - c10 c10)
//   y0 = b_0 / c00,  y1 = (b_1 - c10 y0) / c11,  mean_1 = y1 / c11,  mean_0 = (y0 - c10 mean_1) / c00
//   x1 = z_1 / c11,  x0 = (z_0 - c10 x1) / c00,  beta'_q = mean_q + x_q
//   mo_i = beta_0 + theta_i beta_1 (the stored mu's bits),  mu_i = beta'_0 + theta_i beta'_1,  f'_i = f_i + (mo_i - mu_i),
//   mu*_i = beta'_0 + theta*_i beta'_1.  The shift is the difference of the two ROUNDED means, not X (beta - beta'): f' + mu'
//   then differs from f + mu by the roundings of that difference and of the last sum alone, also where beta_0 and theta beta_1
//   cancel.
#include "common.h"
#include "kernels.h"

#include <cmath>

namespace gpirt {

namespace {

constexpr int BR = BETA_CENTRED_RANK;
constexpr int BT = 256;
constexpr double DMAX = 1.79769313486231570815e308;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= DMAX; }

// the fixed LDS tree over the 256 accumulators of two sums at once; the totals come back in every thread
__device__ __forceinline__ void tree2(double* s0, double* s1, int tid, double& a0, double& a1)
{
    s0[tid] = a0; s1[tid] = a1;
    __syncthreads();
#pragma unroll
    for (int s = BT / 2; s > 0; s >>= 1) {
        if (tid < s) { s0[tid] += s0[tid + s]; s1[tid] += s1[tid + s]; }
        __syncthreads();
    }
    a0 = s0[0]; a1 = s1[0];
    __syncthreads();                             // (the arrays may be filled again)
}

// One work-group per node c: P[c, 0] = sum_i V[i, c], P[c, 1] = sum_i V[i, c] theta_i in row order.
__global__ __launch_bounds__(BT) void beta_centred_p_kernel(const double* __restrict__ V, const double* __restrict__ theta,
                                                            int64_t n, double* __restrict__ P)
{
    __shared__ double s0[BT], s1[BT];
    const int tid = threadIdx.x, c = blockIdx.x;
    const double* Vc = V + (int64_t)c * n;
    double a0 = 0.0, a1 = 0.0;
    for (int64_t i = tid; i < n; i += BT) {
        const double v = Vc[i];
        a0 = a0 + v;
        a1 = fma(v, theta[i], a1);
    }
    tree2(s0, s1, tid, a0, a1);
    if (tid == 0) { P[c] = a0; P[c + BR] = a1; }
}

// One work-group of 128 threads: thread (k, q) forms u[k, q], then Gx[k, q].  Xh(k, i) is Xh[k + 64 i].
__global__ __launch_bounds__(2 * BR) void beta_centred_gx_kernel(const double* __restrict__ Xh, const double* __restrict__ P,
                                                                 double* __restrict__ Gx)
{
    __shared__ double sP[2 * BR], sU[2 * BR];
    const int t = threadIdx.x, k = t & (BR - 1), q = t >> 6;
    sP[t] = P[t];
    __syncthreads();
    double u = 0.0;
    for (int i = 0; i < BR; ++i) u = fma(Xh[k + BR * i], sP[i + BR * q], u);
    sU[t] = u;
    __syncthreads();
    double g = 0.0;
    for (int i = 0; i < BR; ++i) g = fma(Xh[i + BR * k], sU[i + BR * q], g);
    Gx[t] = g;
}

// One thread per row i: W[i, q] = (X[i, q] - sum_c V[i, c] Gx[c, q]) / eps.
__global__ __launch_bounds__(BT) void beta_centred_w_kernel(const double* __restrict__ V, const double* __restrict__ theta,
                                                            const double* __restrict__ Gx, int64_t n, double eps,
                                                            double* __restrict__ W)
{
    __shared__ double sG[2 * BR];
    if (threadIdx.x < 2 * BR) sG[threadIdx.x] = Gx[threadIdx.x];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (int c = 0; c < BR; ++c) {
        const double v = V[i + (int64_t)c * n];
        s0 = fma(v, sG[c], s0);
        s1 = fma(v, sG[c + BR], s1);
    }
    W[i] = (1.0 - s0) / eps;
    W[i + n] = (theta[i] - s1) / eps;
}

// One work-group: B = {B00, B10, B01, B11} with B10 = B01 the one sum of W[i, 0] theta_i.
__global__ __launch_bounds__(BT) void beta_centred_b_kernel(const double* __restrict__ W, const double* __restrict__ theta,
                                                            int64_t n, double* __restrict__ B)
{
    __shared__ double s0[BT], s1[BT];
    const int tid = threadIdx.x;
    double a00 = 0.0, a01 = 0.0, a11 = 0.0, unused = 0.0;
    for (int64_t i = tid; i < n; i += BT) {
        const double w0 = W[i], w1 = W[i + n], th = theta[i];
        a00 = a00 + w0;
        a01 = fma(w0, th, a01);
        a11 = fma(w1, th, a11);
    }
    tree2(s0, s1, tid, a00, a01);
    tree2(s0, s1, tid, a11, unused);
    if (tid == 0) { B[0] = a00; B[1] = a01; B[2] = a01; B[3] = a11; }
}

// One work-group per item j.  lds_rows: the rows of the item's f column kept in LDS between the reduction and the rewrite (n where
// it fits, else 0: the column is read again).  rec (status: 0 updated, 3 failed), counts (2 x m row-major: updates, failed) and
// the 2 x m / 3 x m intermediates (column j: item j) have this one writer per value.
__global__ __launch_bounds__(BT) void beta_centred_item_kernel(BetaCentredArgs a, int lds_rows)
{
    extern __shared__ __attribute__((aligned(16))) double sf[];
    __shared__ double s0[BT], s1[BT];
    __shared__ double sh[4];
    __shared__ int s_ok;
    const int tid = threadIdx.x;
    const int64_t j = blockIdx.x, n = a.n, m = a.m;
    double* fj = a.f + j * n;
    const double* W0 = a.W;
    const double* W1 = a.W + n;
    const bool keep = lds_rows > 0;
    double t0 = 0.0, t1 = 0.0;
    for (int64_t i = tid; i < n; i += BT) {
        const double fv = fj[i];
        if (keep) sf[i] = fv;
        t0 = fma(W0[i], fv, t0);
        t1 = fma(W1[i], fv, t1);
    }
    tree2(s0, s1, tid, t0, t1);
    if (tid == 0) {
        const double be0 = a.beta[0 + 2 * j], be1 = a.beta[1 + 2 * j];
        const double aj = a.amp ? a.amp[j] : 1.0;
        const double ia = 1.0 / (aj * aj);
        const double sd0 = a.ps[0 + 2 * j], sd1 = a.ps[1 + 2 * j];
        const double p0 = 1.0 / (sd0 * sd0), p1 = 1.0 / (sd1 * sd1);
        const double B00 = a.B[0], B10 = a.B[1], B01 = a.B[2], B11 = a.B[3];
        const double z0 = qnorm_as241(item_uniform(a.seed, a.t, GPIRT_ST_BETA_CENTRED, a.item0 + (uint32_t)j, 0u));
        const double z1 = qnorm_as241(item_uniform(a.seed, a.t, GPIRT_ST_BETA_CENTRED, a.item0 + (uint32_t)j, 1u));
        const double b0 = (t0 + (B00 * be0 + B01 * be1)) * ia + a.pm[0 + 2 * j] * p0;
        const double b1 = (t1 + (B10 * be0 + B11 * be1)) * ia + a.pm[1 + 2 * j] * p1;
        const double L00 = B00 * ia + p0, L10 = B10 * ia, L11 = B11 * ia + p1;
        const double c00 = sqrt(L00);
        const double c10 = L10 / c00;
        const double piv = L11 - c10 * c10;
        const double c11 = sqrt(piv);
        const double y0 = b0 / c00;
        const double y1 = (b1 - c10 * y0) / c11;
        const double mean1 = y1 / c11;
        const double mean0 = (y0 - c10 * mean1) / c00;
        const double x1 = z1 / c11;
        const double x0 = (z0 - c10 * x1) / c00;
        const double n0 = mean0 + x0, n1 = mean1 + x1;
        const bool ok = finite_d(t0) && finite_d(t1) && finite_d(L00) && finite_d(L10) && finite_d(L11) && L00 > 0.0 && piv > 0.0 &&
                        finite_d(c00) && finite_d(c10) && finite_d(c11) && c00 > 0.0 && c11 > 0.0 &&
                        finite_d(mean0) && finite_d(mean1) && finite_d(n0) && finite_d(n1);
        a.T[0 + 2 * j] = t0; a.T[1 + 2 * j] = t1;
        a.Z[0 + 2 * j] = z0; a.Z[1 + 2 * j] = z1;
        a.mean[0 + 2 * j] = mean0; a.mean[1 + 2 * j] = mean1;
        a.chol[0 + 3 * j] = c00; a.chol[1 + 3 * j] = c10; a.chol[2 + 3 * j] = c11;
        a.beta_old[0 + 2 * j] = be0; a.beta_old[1 + 2 * j] = be1;
        a.beta_new[0 + 2 * j] = ok ? n0 : be0; a.beta_new[1 + 2 * j] = ok ? n1 : be1;
        a.rec[j] = ok ? 0.0 : 3.0;
        a.counts[j] += 1;
        if (!ok) a.counts[m + j] += 1;
        if (ok) { a.beta[0 + 2 * j] = n0; a.beta[1 + 2 * j] = n1; }
        sh[0] = be0; sh[1] = be1; sh[2] = n0; sh[3] = n1;
        s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) return;                           // failed: the column, beta, mu and mu_star stay byte for byte
    const double o0 = sh[0], o1 = sh[1], n0 = sh[2], n1 = sh[3];
    double* mj = a.mu + j * n;
    for (int64_t i = tid; i < n; i += BT) {
        const double th = a.theta[i];
        const double fv = keep ? sf[i] : fj[i];
        const double mo = o0 + th * o1, mn = n0 + th * n1;          // the linear mean's bits for beta and for beta'
        fj[i] = fv + (mo - mn);
        mj[i] = mn;
    }
    double* msj = a.mu_star + j * a.N;
    for (int64_t i = tid; i < a.N; i += BT) msj[i] = n0 + a.tstar[i] * n1;
}

}  // namespace

int launch_beta_centred(hipStream_t st, const BetaCentredArgs& a)
{
    const int64_t n = a.n, m = a.m;
    if (n <= 0 || m <= 0) return 0;
    GP_TRY(launch_nu_lr_basis(st, a.theta, n, a.nodes, a.wts, a.V));
    GP_TRY(launch_gemm_splitk(st, true, false, BR, BR, n, 1.0, a.V, n, a.V, n, a.parts, BR, (int64_t)BR * BR, a.nsplit, a.Gv, BR, 0.0));
    GP_TRY(launch_fstar_free_xhat(st, a.Gv, a.F, a.eps, a.Xh, 1, a.err, false, a.R));
    hipLaunchKernelGGL(beta_centred_p_kernel, dim3(BR), dim3(BT), 0, st, a.V, a.theta, n, a.P);
    hipLaunchKernelGGL(beta_centred_gx_kernel, dim3(1), dim3(2 * BR), 0, st, a.Xh, a.P, a.Gx);
    hipLaunchKernelGGL(beta_centred_w_kernel, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, st, a.V, a.theta, a.Gx, n, a.eps, a.W);
    hipLaunchKernelGGL(beta_centred_b_kernel, dim3(1), dim3(BT), 0, st, a.W, a.theta, n, a.B);
    GP_HIP(hipGetLastError());
    // the item's f column in LDS where it fits (64 KB at n = 8192, of the 160 KB a work-group has); read again otherwise
    const int lds_rows = n <= BETA_CENTRED_LDS_ROWS ? (int)n : 0;
    const size_t lds = sizeof(double) * (size_t)lds_rows;
    if (lds > 0) GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(beta_centred_item_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (a.kev[0]) GP_HIP(hipEventRecord(a.kev[0], st));
    hipLaunchKernelGGL(beta_centred_item_kernel, dim3((unsigned)m), dim3(BT), lds, st, a, lds_rows);
    GP_HIP(hipGetLastError());
    if (a.kev[1]) GP_HIP(hipEventRecord(a.kev[1], st));
    return 0;
}

}  // namespace gpirt
