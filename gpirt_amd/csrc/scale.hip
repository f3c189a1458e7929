// scale.hip -- the collapsed scale and shift move: the linear mean's coefficients with theta summed out
// (gpirt_sampler_draw_scale, sampler.hip; include/gpirt_hip.h has the contract, DESIGN.md section 45 the reasons).
//
// Between theta_partial and theta_finish the sampler holds logpost (N x n), the log-likelihood of every respondent at every
// grid point.  Respondent i's theta is drawn from masses proportional to exp(P_i[k]) on k = 1 .. N - 1, P_i[k] = lprior_i[k] +
// logpost[k, i], so  lz_i = log sum_{k >= 1} exp(P_i[k])  is the log normaliser of exactly that law and  prod_i exp(lz_i)  the
// likelihood of the curve with theta summed out.  One call proposes ONE joint change of all m linear means on the grid, with the
// GP part hstar = fstar - mu_star held fixed, and decides it on  sum_i (lz'_i - lz_i)  plus beta's prior and the Jacobian:
//   kind 0 (scale)  eps = w z,    b1_j' = b1_j exp(-eps),      b0_j' = b0_j;   log r = sum_i dlz_i + sum_j dprior_j - m eps
//   kind 1 (shift)  delta = w z,  b0_j' = b0_j + b1_j delta,   b1_j' = b1_j;   log r = sum_i dlz_i + sum_j dprior_j
// The theta_finish that follows redraws every theta under whichever curve stands: a partially collapsed Gibbs pair.
//
// The launches, all on the caller's stream, no host read, no floating-point atomic, one writer per value:
//   scale_curve_kernel    N x m: z, the step, beta', mu2 and fstar2; the record's first entries
//   (the caller's)        logpost2 from fstar2 by the launches theta_partial makes
//   scale_logz_kernel     one work-group per respondent: lz_i, lz'_i, dlz_i, bad_i
//   scale_decide_kernel   one work-group: the sums, log u, the decision, the record, the counters
//   scale_commit_kernel, scale_commit_logpost_kernel   return at once unless the record says accepted
//
// THE ORDER OF EVERY OPERATION (the library is built without contraction: no fma anywhere in this file):
//   z       = qnorm_as241(item_uniform(seed, t, GPIRT_ST_SCALE, kind, 0)),  step = w * z
//   scale:    c = exp(-step) (the device's exp; the record holds c),  b1' = b1 * c,  b0' = b0
//   shift:    c = 1,  b0' = b0 + b1 * step (one product, one sum),  b1' = b1
//   mu2[k,j]  = b0' + x_k * b1',  x_k = -5.0 + (double)k * 0.01            draw_beta_kernel's expression and bits
//   fstar2    = fstar + (mu2 - mu_star)                                    the difference of the two ROUNDED means
//   P_i[k]    = lprior_i[k] + logpost[k, i]; lprior_i[k] = r_dnorm_log(x_k, 0, 1), or table[codes[i], k] with a population prior
//   LAYOUT:   thread t of 256 holds k = 4 t + e, e = 0 .. 3 (theta_sample_kernel's); k = 0 and k >= N are left out
//   M_i       = max over the held k (fmax: a NaN is skipped by the maximum and caught by the sum)
//   s_t       = ((0 + exp(P[4t] - M)) + exp(P[4t+1] - M)) + ..             e ascending, left-out k add exactly 0.0
//   S_i       = the adjacent-pair tree over s_0 .. s_255: for d = 1, 2, .., 128: s[t] += s[t - d] at every t with
//               (t + 1) % (2 d) == 0; S_i = s[255].  (What the last entry of theta_sample_kernel's Hillis-Steele scan holds.)
//   lz_i      = M_i + log(S_i);  lz'_i likewise from logpost2;  dlz_i = lz'_i - lz_i
//   bad_i     = 1 when lz_i or lz'_i is not finite or M_i, M'_i is not > -1e300 (theta_sample_kernel's degenerate column), else 0
//   ROW ORDER (the decide kernel): thread t of 256 takes i = t, t + 256, ... ascending into one accumulator that starts at 0,
//             then the fixed LDS tree s = 128, 64, .., 1: acc[t] += acc[t + s] (ell_delta_kernel's).   D = sum_i dlz_i so.
//   Q         = sum_j q_j in ascending j from 0, q_j = r_dnorm_log(b', pm, ps) - r_dnorm_log(b, pm, ps) of the moved coefficient
//   J         = (double)m * step for the scale, 0.0 for the shift;   log r = (D + Q) - J
//   u = item_uniform(seed, t, GPIRT_ST_SCALE, kind, 1);   accepted iff log(u) < log r and nothing failed
#include "common.h"
#include "kernels.h"

#include <cmath>

namespace gpirt {

namespace {

constexpr int SC_T = 256;
constexpr double DMAX = 1.79769313486231570815e308;
constexpr double LN_SQRT_2PI = 0.918938533204672741780329736406;

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= DMAX; }

// R's dnorm(x, mu, sd, log = TRUE) as stages.hip forms it
__device__ __forceinline__ double dnorm_log(double x, double mu, double sd)
{
    const double z = fabs((x - mu) / sd);
    return -(LN_SQRT_2PI + 0.5 * z * z + log(sd));
}

// grid (ceil(N / 256), m).  Every thread forms z, the step and c itself (the same bits everywhere); thread k = 0 of item j
// writes beta_prop[:, j], thread (0, 0) the record's first entries.
__global__ __launch_bounds__(SC_T) void scale_curve_kernel(ScaleArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * SC_T + threadIdx.x, j = blockIdx.y;
    if (k >= a.N) return;
    const double z = qnorm_as241(item_uniform(a.seed, a.t, GPIRT_ST_SCALE, (uint32_t)a.kind, 0u));
    const double step = a.width * z;
    const double b0 = a.beta[0 + 2 * j], b1 = a.beta[1 + 2 * j];
    double c = 1.0, n0 = b0, n1 = b1;
    if (a.kind == 0) { c = exp(-step); n1 = b1 * c; }
    else n0 = b0 + b1 * step;
    const double x = -5.0 + (double)k * 0.01;
    const double m2 = n0 + x * n1;
    const int64_t g = k + j * a.N;
    a.mu2[g] = m2;
    a.fstar2[g] = a.fstar[g] + (m2 - a.mu_star[g]);
    if (k == 0) {
        a.beta_prop[0 + 2 * j] = n0; a.beta_prop[1 + 2 * j] = n1;
        if (j == 0) { a.rec[SCALE_REC_KIND] = (double)a.kind; a.rec[SCALE_REC_Z] = z; a.rec[SCALE_REC_STEP] = step; a.rec[SCALE_REC_C] = c;
                      a.rec[SCALE_REC_T] = (double)a.t; a.rec[SCALE_REC_WIDTH] = a.width; }
    }
}

// the log normaliser of one column in the stated layout and order; every thread returns it, M comes back too
__device__ __forceinline__ double column_logz(const double* __restrict__ lp, const double (&pr)[4], int N, int t, double* red,
                                              double* tree, double& Mout)
{
    const int lane = t & 63, w = t >> 6;
    double P[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = t * 4 + e;
        P[e] = (k >= 1 && k < N) ? pr[e] + lp[k] : -INFINITY;
    }
    double mx = fmax(fmax(P[0], P[1]), fmax(P[2], P[3]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    double run = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = t * 4 + e;
        run += (k >= 1 && k < N) ? exp(P[e] - mx) : 0.0;
    }
    tree[t] = run;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < SC_T; d <<= 1) {
        if (((t + 1) & (2 * d - 1)) == 0) tree[t] += tree[t - d];
        __syncthreads();
    }
    const double S = tree[SC_T - 1];
    __syncthreads();                             // (red and tree are filled again for the second column)
    Mout = mx;
    return mx + log(S);
}

// One work-group per respondent, theta_sample_kernel's layout.  POP: the prior is row codes[i] of the table.
template <bool POP>
__global__ __launch_bounds__(SC_T) void scale_logz_kernel(ScaleArgs a)
{
    __shared__ double red[4];
    __shared__ double tree[SC_T];
    const int64_t i = blockIdx.x;
    const int t = threadIdx.x, N = (int)a.N;
    const double* prior = nullptr;
    if (POP) prior = a.log_prior + (int64_t)a.codes[i] * a.N;
    double pr[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = t * 4 + e;
        if (k < N) pr[e] = POP ? prior[k] : dnorm_log(-5.0 + (double)k * 0.01, 0.0, 1.0);
        else pr[e] = 0.0;
    }
    double M0, M1;
    const double lz0 = column_logz(a.logpost + i * a.N, pr, N, t, red, tree, M0);
    const double lz1 = column_logz(a.logpost2 + i * a.N, pr, N, t, red, tree, M1);
    if (t == 0) {
        a.lz[i] = lz0; a.lz_prop[i] = lz1; a.dlz[i] = lz1 - lz0;
        a.bad[i] = (finite_d(lz0) && finite_d(lz1) && M0 > -1e300 && M1 > -1e300) ? 0 : 1;
    }
}

// One work-group.  rec[SCALE_REC_STATUS]: 0 rejected, 1 accepted, 2 failed.  counts (3 x 2 row-major: calls, accepted, failed
// of the kind) have this one writer.
__global__ __launch_bounds__(SC_T) void scale_decide_kernel(ScaleArgs a)
{
    __shared__ double sd[SC_T];
    __shared__ int sc[SC_T];
    const int tid = threadIdx.x;
    double acc = 0.0;
    int bad = 0;
    for (int64_t i = tid; i < a.n; i += SC_T) { acc += a.dlz[i]; bad += a.bad[i]; }
    sd[tid] = acc; sc[tid] = bad;
    __syncthreads();
#pragma unroll
    for (int s = SC_T / 2; s > 0; s >>= 1) {
        if (tid < s) { sd[tid] += sd[tid + s]; sc[tid] += sc[tid + s]; }
        __syncthreads();
    }
    const double D = sd[0];
    bad = sc[0];
    __syncthreads();
    // the prior's terms: all threads form 256 items' at a time, the one deciding thread adds them in ascending j
    const int q = a.kind == 0 ? 1 : 0;              // the moved coefficient
    double Q = 0.0;
    int badb = 0;
    for (int64_t j0 = 0; j0 < a.m; j0 += SC_T) {
        const int64_t j = j0 + tid;
        if (j < a.m) {
            const double bo = a.beta[q + 2 * j], bn = a.beta_prop[q + 2 * j];
            const double pm = a.pm[q + 2 * j], ps = a.ps[q + 2 * j];
            sd[tid] = dnorm_log(bn, pm, ps) - dnorm_log(bo, pm, ps);
            sc[tid] = (finite_d(bn) && finite_d(a.beta_prop[(1 - q) + 2 * j])) ? 0 : 1;
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = (int)(a.m - j0 < SC_T ? a.m - j0 : SC_T);
            for (int e = 0; e < cnt; ++e) { Q += sd[e]; badb += sc[e]; }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const double step = a.rec[SCALE_REC_STEP];
    const double J = a.kind == 0 ? (double)a.m * step : 0.0;
    const double logr = (D + Q) - J;
    const double u = item_uniform(a.seed, a.t, GPIRT_ST_SCALE, (uint32_t)a.kind, 1u);
    const double logu = log(u);
    const bool failed = bad != 0 || badb != 0 || !finite_d(D) || !finite_d(Q) || !finite_d(logr);
    const bool accept = !failed && logu < logr;
    a.rec[SCALE_REC_D] = D; a.rec[SCALE_REC_Q] = Q; a.rec[SCALE_REC_J] = J; a.rec[SCALE_REC_LOGR] = logr;
    a.rec[SCALE_REC_U] = u; a.rec[SCALE_REC_LOGU] = logu; a.rec[SCALE_REC_STATUS] = failed ? 2.0 : (accept ? 1.0 : 0.0);
    a.rec[SCALE_REC_BAD] = (double)(bad + badb);
    a.counts[0 + a.kind] += 1;
    if (accept) a.counts[2 + a.kind] += 1;
    if (failed) a.counts[4 + a.kind] += 1;
}

// The curve and the means: fstar <- fstar2, mu_star <- mu2, gbar += mu2 - mu_star (when the shape block is on), mu = b0' +
// theta_i b1' (linear_mean_kernel's expression), beta <- beta'.  One thread per cell of each, nothing unless accepted.
__global__ __launch_bounds__(SC_T) void scale_commit_kernel(ScaleArgs a)
{
    if (a.rec[SCALE_REC_STATUS] != 1.0) return;
    const int64_t Nm = a.N * a.m, nm = a.n * a.m, top = Nm > nm ? Nm : nm;
    const int64_t stride = (int64_t)gridDim.x * SC_T;
    for (int64_t g = (int64_t)blockIdx.x * SC_T + threadIdx.x; g < top; g += stride) {
        if (g < Nm) {
            const double m2 = a.mu2[g];
            if (a.gbar) a.gbar[g] = a.gbar[g] + (m2 - a.mu_star[g]);
            a.fstar[g] = a.fstar2[g];
            a.mu_star[g] = m2;
        }
        if (g < nm) {
            const int64_t j = g / a.n, i = g - j * a.n;
            a.mu[g] = a.beta_prop[0 + 2 * j] + a.theta[i] * a.beta_prop[1 + 2 * j];
        }
        if (g < 2 * a.m) a.beta[g] = a.beta_prop[g];
    }
}

__global__ __launch_bounds__(SC_T) void scale_commit_logpost_kernel(const double* __restrict__ rec, double* __restrict__ lp,
                                                                    const double* __restrict__ lp2, int64_t count)
{
    if (rec[SCALE_REC_STATUS] != 1.0) return;
    const int64_t stride = (int64_t)gridDim.x * SC_T;
    for (int64_t g = (int64_t)blockIdx.x * SC_T + threadIdx.x; g < count; g += stride) lp[g] = lp2[g];
}

}  // namespace

int launch_scale_curve(hipStream_t st, const ScaleArgs& a)
{
    if (a.N <= 0 || a.m <= 0) return 0;
    hipLaunchKernelGGL(scale_curve_kernel, dim3((unsigned)((a.N + SC_T - 1) / SC_T), (unsigned)a.m), dim3(SC_T), 0, st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_scale_decide(hipStream_t st, const ScaleArgs& a)
{
    if (a.n <= 0 || a.m <= 0) return 0;
    if (a.N > 1024) { set_error("theta grid larger than 1024 points is not supported"); return GPIRT_E_ARG; }
    if (a.kev[0]) GP_HIP(hipEventRecord(a.kev[0], st));
    if (a.log_prior && a.codes) hipLaunchKernelGGL(scale_logz_kernel<true>, dim3((unsigned)a.n), dim3(SC_T), 0, st, a);
    else hipLaunchKernelGGL(scale_logz_kernel<false>, dim3((unsigned)a.n), dim3(SC_T), 0, st, a);
    if (a.kev[1]) GP_HIP(hipEventRecord(a.kev[1], st));
    hipLaunchKernelGGL(scale_decide_kernel, dim3(1), dim3(SC_T), 0, st, a);
    if (a.kev[2]) GP_HIP(hipEventRecord(a.kev[2], st));
    const int64_t Nm = a.N * a.m, nm = a.n * a.m, top = Nm > nm ? Nm : nm;
    int64_t blocks = (top + SC_T - 1) / SC_T;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(scale_commit_kernel, dim3((unsigned)blocks), dim3(SC_T), 0, st, a);
    blocks = (a.N * a.n + SC_T - 1) / SC_T;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(scale_commit_logpost_kernel, dim3((unsigned)blocks), dim3(SC_T), 0, st, a.rec, a.logpost, a.logpost2, a.N * a.n);
    if (a.kev[3]) GP_HIP(hipEventRecord(a.kev[3], st));
    GP_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpirt
