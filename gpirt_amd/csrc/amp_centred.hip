// amp_centred.hip -- the centred update of the per-item GP amplitudes on the GP's rank-64 smooth part
// (gpirt_sampler_draw_amp_centred, sampler.hip; include/gpirt_hip.h has the contract, DESIGN.md section 43 the reasons).
//
// The whitened update (amp.hip) holds nu_j = L^-1 f_j / a_j fixed, and with thousands of answers per item the likelihood pins
// f_j down: a_j then moves only as fast as draw_f changes |nu_j|.  Murray & Adams (2010) pair it with a centred move that reads
// the prior density of f.  With the nugget tied to the amplitude the plain conjugate update of a_j^2 given f_j^T S^-1 f_j has n
// degrees of freedom of which n - r are nugget; this one reads the smooth part alone, by augmentation.  With V the Lagrange basis
// at theta (nu_lr.hip), Kcc = F F^T (fstar_free_factor; columns of F with squared norm <= 1e-13 are DEAD and zeroed by the host,
// r live ones remain), Phi = V F and eps the jitter, the model f_j ~ N(0, a_j^2 (K + eps I)) is the marginal of
//       xi_j ~ N(0, a_j^2 I_r),   e_j ~ N(0, eps I_n),   f_j = Phi xi_j + a_j e_j.
// One update of item j:
//   1. xi_j | f_j, a_j from its Gaussian conditional: A = Phi^T Phi + eps I = R R^T, t_j = R^-1 Phi^T f_j, w_j = t_j +
//      (a_j sqrt(eps)) z_j, xi_j = R^-T w_j; h_j = Phi xi_j, Q_j = |xi_j|^2 over the live coordinates;
//   2. k' from the exact discrete conditional of a given xi_j alone: q[k] ~ exp(log_prior[k] - r ln a_k - Q_j / (2 a_k^2));
//   3. f_j' = h_j + (a_k' / a_k)(f_j - h_j): the nugget's whitened coordinates held fixed;
//   4. accept iff log u1 < ll(f_j') - ll(f_j): the proposal carries the prior and the centred term, the likelihood is left.
//
// The launches, all on the caller's stream, no host read, no atomics but the error word, one writer per value:
//   launch_nu_lr_basis             V (n x 64) from theta
//   launch_gemm_splitk             Gv = V^T V, the parts added in index order
//   fstar_free_xhat (with R)       Xh = R^-1 F^T and R, one work-group (fstar_free.hip); a bad pivot raises *err
//   launch_gemm_splitk             T = V^T f (64 x m)
//   amp_centred_coef_kernel        per item: t, z, w, xi, Q, g = Xh^T w = F xi
//   launch_gemm_batched            H = V Gc (n x m), un-split: an element depends on its row of V and its item's g alone
//   amp_centred_update_kernel      per item: the proposal table, the draw, the pass over the rows, the decision, the rewrite
//
// THE ORDER OF EVERY SUM (coefficient kernel; lane k of the item's wavefront owns coordinate k, fma where written):
//   t_k  = fma(Xh(k, i), T_i, .) over i = 0 .. 63 ascending from 0
//   z_k  = qnorm_as241(item_uniform(seed, t, GPIRT_ST_AMP_CENTRED, item0 + j, k)), all 64 drawn, dead ones ignored
//   w_k  = t_k + (a_j sqrt_eps) z_k                        one product for the sd, one product, one sum
//   xi   = R^-T w by back-substitution, k = 63 .. 0: xi_k = w_k / R(k, k), then w_i <- w_i - R(k, i) xi_k for i < k
//   Q    = sum of xi_k xi_k over live k ascending from 0   product, then sum
//   g_i  = fma(Xh(k, i), w_k, .) over k = 0 .. 63 ascending from 0
// and of the update kernel: lq[k] = (log_prior[k] - r ln_a[k]) - Q half_inv_a2[k]; exp(lq[k] - max); a thread's points added in
// index order, a Hillis-Steele scan over the 256 thread totals (theta_sample_kernel's); k' = the first k with C_k > u0 C_last;
// the rows in ell_delta_kernel's order (thread t takes rows t, t + 256, ..., then the fixed LDS tree).
#include "common.h"
#include "kernels.h"
#include "ll_fast.h"

#include <cmath>

namespace gpirt {

namespace {

constexpr int CR = AMP_CENTRED_RANK;
constexpr int CLD = CR + 1;                  // LDS column stride (doubles): odd, rows and columns both spread over the banks
constexpr int CT = 256;
constexpr int COEF_ITEMS = CT / 64;          // one wavefront per item
constexpr double DMAX = 1.79769313486231570815e308;

// Four items per work-group, one wavefront each; Xh and R are staged once per work-group (2 x 33 KB of LDS).  Every barrier is
// met by all four wavefronts: a wavefront past the last item computes on the last item's data and stores nothing.
__global__ __launch_bounds__(CT) void amp_centred_coef_kernel(AmpCentredArgs a, double sqrt_eps)
{
    __shared__ double sX[CR * CLD];          // Xh(k, i) at sX[k + CLD i]
    __shared__ double sR[CR * CLD];          // R(i, k) at sR[i + CLD k]
    __shared__ double sT[COEF_ITEMS][CR], sW[COEF_ITEMS][CR], sXi[COEF_ITEMS][CR];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int e = t; e < CR * CR; e += CT) {
        const int r = e & (CR - 1), c = e >> 6;
        sX[r + CLD * c] = a.Xh[e];
        sR[r + CLD * c] = a.R[e];
    }
    const int64_t jw = (int64_t)blockIdx.x * COEF_ITEMS + wave;
    const bool on = jw < a.m;
    const int64_t j = on ? jw : a.m - 1;
    sT[wave][lane] = a.T[lane + CR * j];
    __syncthreads();
    double tk = 0.0;
#pragma unroll 8
    for (int i = 0; i < CR; ++i) tk = fma(sX[lane + CLD * i], sT[wave][i], tk);
    const double z = qnorm_as241(item_uniform(a.seed, a.t, GPIRT_ST_AMP_CENTRED, a.item0 + (uint32_t)j, (uint32_t)lane));
    const double sd = a.amp[j] * sqrt_eps;
    const double w = tk + sd * z;
    sW[wave][lane] = w;
    // R^T xi = w, R lower: from the last coordinate up.  The running right-hand side stays in the lanes' registers, the pivot's
    // value goes round by a shuffle; nothing here crosses a wavefront
    double rhs = w, xi = 0.0;
    for (int k = CR - 1; k >= 0; --k) {
        const double xk = __shfl(rhs, k, 64) / sR[k + CLD * k];
        if (lane == k) xi = xk;
        if (lane < k) rhs = rhs - sR[k + CLD * lane] * xk;
    }
    sXi[wave][lane] = xi;
    __syncthreads();
    double g = 0.0;
#pragma unroll 8
    for (int k = 0; k < CR; ++k) g = fma(sX[k + CLD * lane], sW[wave][k], g);
    if (!on) return;
    a.Z[lane + CR * j] = z;
    a.W[lane + CR * j] = w;
    a.Xi[lane + CR * j] = xi;
    a.Gc[lane + CR * j] = g;
    if (lane == 0) {
        double q = 0.0;
        for (int k = 0; k < CR; ++k)
            if ((a.live >> k) & 1ull) { const double x = sXi[wave][k]; q = q + x * x; }
        a.Q[j] = q;
    }
}

// One work-group per item j, on the plan of amp_update_kernel.  counts (4 x m: updates, accepted, same, failed) and rec (5 x m:
// Q, k', dll, log u1, status; status 0 rejected, 1 accepted, 2 same, 3 failed) have this one writer per value; k' is -1 and the
// two figures NaN where the update failed before a draw, dll and log u1 are NaN for `same`.
__global__ __launch_bounds__(CT) void amp_centred_update_kernel(AmpCentredArgs a)
{
    __shared__ double sd[CT];
    __shared__ int sc[CT];
    __shared__ double red[4];
    __shared__ int ired[4];
    __shared__ int s_accept;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t j = blockIdx.x, n = a.n, m = a.m;
    const int P = a.P;
    const double u0 = item_uniform(a.seed, a.t, GPIRT_ST_AMP_CENTRED, a.item0 + (uint32_t)j, 64),
                 u1 = item_uniform(a.seed, a.t, GPIRT_ST_AMP_CENTRED, a.item0 + (uint32_t)j, 65);
    const int k = a.idx[j];
    const double Q = a.Q[j];
    long long* cnt = a.counts + j;
    double* rec = a.rec + j;
    const double nan = __builtin_nan("");
    // the proposal table: thread t holds the points 4 t .. 4 t + 3, the last thread also point 1024 (P <= 1025)
    const double rr = (double)a.r;
    double C[5];
    int kk[5];
    double mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 5; ++e) {
        kk[e] = e < 4 ? 4 * tid + e : (tid == CT - 1 ? 4 * CT : P);
        if (kk[e] < P) {
            C[e] = (a.log_prior[kk[e]] - rr * a.ln_a[kk[e]]) - Q * a.half_inv_a2[kk[e]];
            mx = fmax(mx, C[e]);
        } else C[e] = -INFINITY;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) red[wv] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    double run = 0.0;
#pragma unroll
    for (int e = 0; e < 5; ++e) {
        const double v = kk[e] < P ? exp(C[e] - mx) : 0.0;
        run += v;
        C[e] = run;
    }
    sd[tid] = run;
    __syncthreads();
    for (int d = 1; d < CT; d <<= 1) {               // Hillis-Steele inclusive scan of the 256 thread totals
        const double add = tid >= d ? sd[tid - d] : 0.0;
        __syncthreads();
        sd[tid] += add;
        __syncthreads();
    }
    const double base = tid > 0 ? sd[tid - 1] : 0.0, total = sd[CT - 1];
    const double cut = u0 * total;
    int first = 0x7fffffff;
#pragma unroll
    for (int e = 4; e >= 0; --e)
        if (kk[e] < P && C[e] + base > cut) first = kk[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
    if (lane == 0) ired[wv] = first;
    __syncthreads();
    const int kp = min(min(ired[0], ired[1]), min(ired[2], ired[3]));
    // a Q, a maximum or a total that is not finite and positive: no draw can be made -- failed, not an error
    if (!(fabs(Q) <= DMAX) || !(fabs(mx) <= DMAX) || !(total > 0.0) || !(total <= DMAX) || kp == 0x7fffffff) {
        if (tid == 0) {
            cnt[0] += 1; cnt[3 * m] += 1;
            rec[0] = Q; rec[m] = -1.0; rec[2 * m] = nan; rec[3 * m] = nan; rec[4 * m] = 3.0;
        }
        return;
    }
    if (kp == k) {
        if (tid == 0) {
            cnt[0] += 1; cnt[2 * m] += 1;
            rec[0] = Q; rec[m] = (double)kp; rec[2 * m] = nan; rec[3 * m] = nan; rec[4 * m] = 2.0;
        }
        return;
    }
    const double c = a.grid[kp] / a.grid[k];
    double* fj = a.f + j * n;
    const double* hj = a.H + j * n;
    const double* mj = a.mu + j * n;
    const double* yj = a.y + j * n;
    double acc = 0.0;
    int bad = 0;
    auto cell = [&](double hv, double fv, double mv, double yv) {
        const double pv = hv + c * (fv - hv);
        if (!(fabs(pv) <= DMAX) || !(fabs(hv) <= DMAX)) ++bad;               // NaN or infinite
        if (yv == yv) acc += ll_term_fast(yv * (fv + mv)) - ll_term_fast(yv * (pv + mv));
    };
    int64_t i = tid;
    for (; i + 3 * CT < n; i += 4 * CT) {                                     // four rows' loads in flight, added in row order
        const int64_t i1 = i + CT, i2 = i + 2 * CT, i3 = i + 3 * CT;
        const double h0 = hj[i], h1 = hj[i1], h2 = hj[i2], h3 = hj[i3];
        const double f0 = fj[i], f1 = fj[i1], f2 = fj[i2], f3 = fj[i3];
        const double m0 = mj[i], m1 = mj[i1], m2 = mj[i2], m3 = mj[i3];
        const double y0 = yj[i], y1 = yj[i1], y2 = yj[i2], y3 = yj[i3];
        cell(h0, f0, m0, y0); cell(h1, f1, m1, y1); cell(h2, f2, m2, y2); cell(h3, f3, m3, y3);
    }
    for (; i < n; i += CT) cell(hj[i], fj[i], mj[i], yj[i]);
    __syncthreads();                                                          // (sd still holds the scan)
    sd[tid] = acc; sc[tid] = bad;
    __syncthreads();
#pragma unroll
    for (int s = CT / 2; s > 0; s >>= 1) {
        if (tid < s) { sd[tid] += sd[tid + s]; sc[tid] += sc[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double dll = sd[0], log_u = log(u1);
        const bool failed = sc[0] != 0 || !(fabs(dll) <= DMAX);
        const bool accept = !failed && log_u < dll;
        rec[0] = Q; rec[m] = (double)kp; rec[2 * m] = dll; rec[3 * m] = log_u; rec[4 * m] = failed ? 3.0 : (accept ? 1.0 : 0.0);
        cnt[0] += 1;
        if (accept) { cnt[m] += 1; a.idx[j] = kp; a.amp[j] = a.grid[kp]; }
        if (failed) cnt[3 * m] += 1;
        s_accept = accept ? 1 : 0;
    }
    __syncthreads();
    if (!s_accept) return;
    for (i = tid; i < n; i += CT) { const double hv = hj[i]; fj[i] = hv + c * (fj[i] - hv); }
}

}  // namespace

int launch_amp_centred(hipStream_t st, const AmpCentredArgs& a)
{
    const int64_t n = a.n, m = a.m;
    if (n <= 0 || m <= 0) return 0;
    if (a.P < 2 || a.P > 4 * CT + 1) { set_error("amp_centred: P = %d points, the proposal table holds 2 .. %d", a.P, 4 * CT + 1); return GPIRT_E_ARG; }
    GP_TRY(launch_nu_lr_basis(st, a.theta, n, a.nodes, a.wts, a.V));
    GP_TRY(launch_gemm_splitk(st, true, false, CR, CR, n, 1.0, a.V, n, a.V, n, a.parts, CR, (int64_t)CR * CR, a.nsplit, a.Gv, CR, 0.0));
    GP_TRY(launch_fstar_free_xhat(st, a.Gv, a.F, a.eps, a.Xh, 1, a.err, false, a.R));
    GP_TRY(launch_gemm_splitk(st, true, false, CR, m, n, 1.0, a.V, n, a.f, n, a.parts, CR, (int64_t)CR * m, a.nsplit, a.T, CR, 0.0));
    hipLaunchKernelGGL(amp_centred_coef_kernel, dim3((unsigned)((m + COEF_ITEMS - 1) / COEF_ITEMS)), dim3(CT), 0, st, a, std::sqrt(a.eps));
    GP_HIP(hipGetLastError());
    // an un-split 64-tile product: an element of H depends on its row of V and on its item's column of Gc alone
    GP_TRY(launch_gemm_batched(st, false, false, TRI_NONE, n, m, CR, 1.0, a.V, n, 0, a.Gc, CR, 0, 0.0, a.H, n, 0, 1));
    hipLaunchKernelGGL(amp_centred_update_kernel, dim3((unsigned)m), dim3(CT), 0, st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpirt
