// ordinal.hip -- ordinal (graded) responses under the cumulative-logit model (include/gpirt_hip.h, "ordinal responses"; library
// version 139).  With g = f + mu and an item's thresholds b_1 < ... < b_{C-1} (b_0 = -inf, b_C = +inf),
//     log P(y = c | g, b) = -ll(b_c - g) [c < C] - ll(g - b_{c-1}) [c > 1] + w(b_c - b_{c-1}) [1 < c < C]
//     ll(a) = log(1 + e^-a) = ll_term_fast(a) (ll_fast.h),   w(d) = log1p(-exp(-d))
// so every cell is one or two evaluations of the term the binary kernels use, and the w term -- free of f, theta and beta --
// matters to the thresholds alone.  cat: n x m int8, column-major, 0 = missing, 1 .. C a category.
//
//   ess_ord_kernel          the elliptical slice for f (rng_ess.hip's ess_kernel_reg with the ordinal term): THE OPERATION ORDER
//                           per trial point and cell is  g = (F c + V s) + M;  t1 = ll(b_c - g) if c < C;  t2 = ll(g - b_{c-1}) if
//                           c > 1;  acc += t1; acc += t2  -- entries in ascending e, then the block's fixed tree.  With C = 2 and
//                           b_1 = 0 the arguments are 0 - g and g - 0: the binary kernel's y g up to the sign of a zero, which
//                           fabs() removes, so f and the rejection counts are the binary kernel's bit for bit.
//   ord_indicators_kernel   cat -> one-hot Y (n x C m)
//   ord_loglik_terms_kernel f* and the thresholds -> G (N x C m), padded as Gpm is
//   ord_nan_fix_kernel      what theta_nan_fix_kernel does, for the one-hot product
//   draw_beta_ord_kernel    the k = 1 pass of src/draw-beta.cpp (the slope) under the ordinal likelihood
//   ord_thresholds_kernel   exact Gibbs for each threshold on the grid inside a randomly placed window
//   ord_irf_kernel          cum[k, c, j] += sigma(f*[k, j] - b_{j,c})
//   ord_record_kernel       the indices of a kept draw into the draw buffer and the histogram
//
// ord_thresholds_kernel, THE OPERATION ORDER (gpirt_amd.ordinal.threshold_conditional is its NumPy statement).  One work-group per
// item; a lane keeps g_i = f_i + mu_i (one addition) of its rows i = tid + NTH e and their categories, 4 bits each.  For
// c = 1 .. C - 1 in order, with k = K[j, c], left = K[j, c-1] (-1 for c = 1), right = K[j, c+1] (P for c = C - 1), each already
// updated where c' < c:
//     u0, u1 = item_uniform(seed, t, GPIRT_ST_ORD, item0 + j, 2 (c - 1)) and (.., 2 (c - 1) + 1), t the draw_thresholds calls from 1
//     a  = k - (int)(u0 W)                  the window is [a, a + W)
//     lo = max(a, left + 1, 0),  hi = min(a + W - 1, right - 1, P - 1)          the candidates q = lo .. hi
//     lo == hi:  the threshold stays, `pinned` counts it, the lp row holds 0 at k's slot and -inf elsewhere
//     else for every q ascending, t_q = grid[q]:
//         a lane's sum: over its rows in ascending e, ll(t_q - g_i) where cat = c, ll(g_i - t_q) where cat = c + 1 (ONE sum)
//         S = the block's fixed tree over the lanes' sums (block_sum_256 / _512 / the 1024-thread tree of ess_kernel_reg)
//         m_q = log_prior[q] - S
//         if left >= 0:  m_q = m_q + (double)N_c     * log1p(-exp(-(t_q - grid[left])))
//         if right < P:  m_q = m_q + (double)N_{c+1} * log1p(-exp(-(grid[right] - t_q)))
//       lp[j, c, q - a] = m_q (every other slot of the row -inf).  Any m_q not finite: `failed` counts it, this threshold and the
//       item's later ones keep their bytes.  Otherwise mx = max m_q, e_q = exp(m_q - mx), the cumulative sums ascending in q, and
//       the new index is the first q whose cumulative sum exceeds u1 * total (the last candidate if rounding leaves none).
// No running factor e^-h is used: every candidate costs its own exp per cell.  The term is ll_term_fast with the DEVICE's exp and
// reciprocal estimate, log1p and exp are the device library's: the lp masses agree with the NumPy statement within a derived
// bound (tests/_ordinal_bounds.py), not bit for bit.  There is no floating-point atomic and each value has one writer: two runs
// give a byte-identical state.
#include "common.h"
#include "kernels.h"
#include "ll_fast.h"

#include <cmath>
#include <vector>

namespace gpirt {

namespace {

constexpr int ORD_MAX_TRIALS = 100000;          // rng_ess.hip's ESS_MAX_TRIALS

#define GP_LN_SQRT_2PI_ORD 0.918938533204672741780329736406

// stages.hip's two helpers of draw_beta, to the letter
__device__ __forceinline__ double ord_rnorm(double mu, double sd, double z)
{
    if (mu != mu || !isfinite(sd) || sd < 0.0) return __builtin_nan("");
    if (sd == 0.0 || !isfinite(mu)) return mu;
    return mu + sd * z;
}

__device__ __forceinline__ double ord_dnorm_log(double x, double mu, double sd)
{
    const double z = fabs((x - mu) / sd);
    return -(GP_LN_SQRT_2PI_ORD + 0.5 * z * z + log(sd));
}

// the block's sum in ess_kernel_reg's trees (red: >= 16 doubles)
template <int NTH>
__device__ __forceinline__ double ord_block_sum(double v, double* red)
{
    if (NTH == 256) return block_sum_256(v, red);
    if (NTH == 512) return block_sum_512(v, red);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7]))) +
           (((red[8] + red[9]) + (red[10] + red[11])) + ((red[12] + red[13]) + (red[14] + red[15])));
}

// One cell's terms added to acc_ in the stated order; bt[c] = b_c in LDS (c = 1 .. C - 1), c_ the cell's category (0: skipped).
// An end category has one term, an interior one two.  (Macros, not lambdas: rng_ess.hip, ESS_ARG0.)
#define ORD_TERMS(acc_, c_, g_, LL_)                                                          \
    do {                                                                                      \
        const int oc_ = (c_);                                                                 \
        if (oc_ != 0) {                                                                       \
            const double og_ = (g_);                                                          \
            const double o1_ = oc_ < C ? bt[oc_] - og_ : og_ - bt[oc_ - 1];                   \
            acc_ += LL_(o1_);                                                                 \
            if (oc_ > 1 && oc_ < C) acc_ += LL_(og_ - bt[oc_ - 1]);                           \
        }                                                                                     \
    } while (0)
#define ORD_CAT(e) ((int)((cats >> (4 * (e))) & 15ull))

// ---- the elliptical slice ---------------------------------------------------------------------------------------------------------
// ess_kernel_reg's three size classes by what a lane HOLDS in registers: 3 = F, V and M (n <= 2048: 8 entries of 256 lanes), 2 = F
// and V, mu read again from memory for every pass (n <= 8192: 16 entries of 512 lanes; with M held as well the compiler reported
// 256 registers and 52 bytes of scratch), 0 = nothing, every pass streams f, nu, mu and cat from memory in the same row order
// i = tid + NTH e (n <= 16384, 1024 lanes at most 128 registers: no 16-entry array fits without scratch there; the item's
// columns are 400 KB and stay in L2).  The sums' order is the same in all three: DESIGN section 47 has the compiler's numbers.
template <int EPT, int NTH, int HOLD>
__global__ __launch_bounds__(NTH) void ess_ord_kernel(EssOrdArgs a)
{
    __shared__ double red[16];
    __shared__ double bt[9];
    const int64_t j = blockIdx.x;
    const int64_t n = a.n;
    const int C = a.C;
    double* fj = a.f + j * n;
    const double* nj = a.nu + j * n;
    const double* mj = a.mu + j * n;
    const int8_t* cj = a.cat + j * n;
    const uint32_t item = a.item0 + (uint32_t)j;
    if (threadIdx.x < 9) bt[threadIdx.x] = (threadIdx.x >= 1 && (int)threadIdx.x < C) ? a.thr[j * (C - 1) + threadIdx.x - 1] : 0.0;
    double F[HOLD >= 2 ? EPT : 1], V[HOLD >= 2 ? EPT : 1], M[HOLD == 3 ? EPT : 1];
    static_assert(EPT <= 16, "4 bits per entry in one 64-bit word");
    uint64_t cats = 0;
    if (HOLD >= 2) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int64_t i = threadIdx.x + NTH * e;
            const bool in = i < n;
            F[HOLD >= 2 ? e : 0] = in ? fj[i] : 0.0;
            V[HOLD >= 2 ? e : 0] = in ? nj[i] : 0.0;
            if (HOLD == 3) M[HOLD == 3 ? e : 0] = in ? mj[i] : 0.0;
            cats |= (uint64_t)(in ? (cj[i] & 15) : 0) << (4 * e);
        }
    }
    // the item's number of terms, for the screen's band: N_c (1 + [1 < c < C]) summed
    double nterms = 0.0;
    for (int c = 1; c <= C; ++c) nterms += (double)a.counts[j * C + c - 1] * ((c > 1 && c < C) ? 2.0 : 1.0);
    __syncthreads();
#define ORD_M(e) (HOLD == 3 ? M[HOLD == 3 ? (e) : 0] : mj[threadIdx.x + NTH * (e)])
#define ORD_G0(e) (F[e] + ORD_M(e))
#define ORD_GP(e, c_, s_) ((F[e] * (c_) + V[e] * (s_)) + ORD_M(e))
// the lane's sum over its rows in ascending e (i = tid + NTH e), TRIAL: at the trial point (c_, s_), else at the current state
#define ORD_SUM(acc_, TRIAL, c_, s_, LL_)                                                                        \
    do {                                                                                                         \
        if (HOLD >= 2) {                                                                                         \
            _Pragma("unroll") for (int e = 0; e < (HOLD >= 2 ? EPT : 1); ++e)                                    \
                if (ORD_CAT(e) != 0) ORD_TERMS(acc_, ORD_CAT(e), (TRIAL) ? ORD_GP(e, c_, s_) : ORD_G0(e), LL_);  \
        } else {                                                                                                 \
            for (int64_t i = threadIdx.x; i < n; i += NTH)                                                       \
                ORD_TERMS(acc_, (int)cj[i], (TRIAL) ? (fj[i] * (c_) + nj[i] * (s_)) + mj[i] : fj[i] + mj[i], LL_); \
        }                                                                                                        \
    } while (0)
    uint32_t uidx = 0;
    double acc = 0.0;
    auto exact_ll0 = [&]() {
        double t = 0.0;
        ORD_SUM(t, false, 0.0, 0.0, ll_term_fast);
        return -ord_block_sum<NTH>(t, red);
    };
    const double band = LL_SCREEN_ERR * nterms;
    double ll0 = 0.0, lls0 = 0.0;
    bool have_ll0 = false;
    if (a.screen) {
        ORD_SUM(acc, false, 0.0, 0.0, ll_term_screen);
        lls0 = -ord_block_sum<NTH>(acc, red);
    } else {
        ll0 = exact_ll0();
        have_ll0 = true;
    }
    const double u = item_uniform(a.seed, a.iter, GPIRT_ST_F_ESS, item, uidx++);
    const double log_u = log(u);
    double eps_min = 0.0, eps_max = GP_2PI;
    double eps = eps_min + (eps_max - eps_min) * item_uniform(a.seed, a.iter, GPIRT_ST_F_ESS, item, uidx++);
    eps_min = eps - GP_2PI;
    int k = 0;
    bool bad = false;
    double c, s;
    for (;;) {
        c = cos(eps);
        s = sin(eps);
        int verdict = 0;                                                   // +1 accept, -1 reject, 0 undecided
        if (a.screen) {
            acc = 0.0;
            ORD_SUM(acc, true, c, s, ll_term_screen);
            const double lls = -ord_block_sum<NTH>(acc, red);
            if (!have_ll0) {
                const double d = lls - lls0;
                if (d - 2.0 * band > log_u) verdict = 1;
                else if (d + 2.0 * band < log_u) verdict = -1;
            } else {
                const double log_y = ll0 + log_u;
                if (lls - band > log_y) verdict = 1;
                else if (lls + band < log_y) verdict = -1;
            }
        }
        if (verdict == 0) {
            if (!have_ll0) { ll0 = exact_ll0(); have_ll0 = true; }
            const double log_y = ll0 + log_u;
            acc = 0.0;
            ORD_SUM(acc, true, c, s, ll_term_fast);
            const double llp = -ord_block_sum<NTH>(acc, red);
            if (llp > log_y) verdict = 1;
            else if (llp != llp || ll0 != ll0) { bad = true; break; }
        }
        if (verdict > 0) break;
        if (eps < 0.0) eps_min = eps; else eps_max = eps;
        if (eps_min == eps_max) eps = eps_min;
        else eps = eps_min + (eps_max - eps_min) * item_uniform(a.seed, a.iter, GPIRT_ST_F_ESS, item, uidx++);
        ++k;
        if (k >= ORD_MAX_TRIALS) { bad = true; break; }
    }
    if (HOLD >= 2) {
#pragma unroll
        for (int e = 0; e < (HOLD >= 2 ? EPT : 1); ++e) {
            const int64_t i = threadIdx.x + NTH * e;
            if (i < n) fj[i] = F[e] * c + V[e] * s;
        }
    } else {
        for (int64_t i = threadIdx.x; i < n; i += NTH) fj[i] = fj[i] * c + nj[i] * s;     // (the lane's own rows)
    }
    if (threadIdx.x == 0) {
        if (a.k_out) a.k_out[j] = k;
        if (bad && a.err) atomicCAS(a.err, 0, (int)GPIRT_E_NUMERIC);
    }
#undef ORD_M
#undef ORD_G0
#undef ORD_GP
#undef ORD_SUM
}

// ---- the theta product's operands ---------------------------------------------------------------------------------------------------
__global__ void ord_indicators_kernel(const int8_t* __restrict__ cat, int64_t total, int C, double* __restrict__ Y)
{
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int v = cat[g];
        for (int c = 0; c < C; ++c) Y[g + (int64_t)c * total] = (v == c + 1) ? 1.0 : 0.0;
    }
}

// counts[j, c - 1] = the item's observed cells of category c (int64): one work-group per item, integer sums
__global__ __launch_bounds__(256) void ord_counts_kernel(const int8_t* __restrict__ cat, int64_t n, int C, long long* __restrict__ counts)
{
    __shared__ int sc[8][256];
    const int64_t j = blockIdx.x;
    int loc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const int v = cat[j * n + i];
#pragma unroll
        for (int c = 0; c < 8; ++c) loc[c] += (v == c + 1) ? 1 : 0;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) sc[c][threadIdx.x] = loc[c];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int c = 0; c < 8; ++c) sc[c][threadIdx.x] += sc[c][threadIdx.x + w];
        __syncthreads();
    }
    if ((int)threadIdx.x < C) counts[j * C + threadIdx.x] = sc[threadIdx.x][0];
}

// G[k, c0 m + j] (category c = c0 + 1) = -ll(b_c - v) [c < C] - ll(v - b_{c-1}) [c > 1], v = f*[k, j]; -inf is held at -1e300 as
// loglik_terms_kernel holds it (stages.hip); NaN stays NaN.  ldg >= N: the rows beyond N are padding and are never written.
__global__ void ord_loglik_terms_kernel(const double* __restrict__ fstar, int64_t N, int64_t m, int C, const double* __restrict__ thr,
                                        double* __restrict__ G, int64_t ldg)
{
    const int64_t total = N * m;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = g % N, j = g / N;
        const double v = fstar[g];
        const double* b = thr + j * (C - 1);              // b[c - 1] = b_c
        for (int c = 1; c <= C; ++c) {
            double val = 0.0;
            if (c < C) val = -ll_term_fast(b[c - 1] - v);
            if (c > 1) val = val - ll_term_fast(v - b[c - 2]);
            if (val == -INFINITY) val = -1e300;
            G[k + ((int64_t)(c - 1) * m + j) * ldg] = val;
        }
    }
}

// every NaN entry of the log-posterior again over the observed cells alone, in item order (theta_nan_fix_kernel's rule)
__global__ void ord_nan_fix_kernel(const double* __restrict__ G, int64_t ldg, const int8_t* __restrict__ cat, int64_t n, int64_t m,
                                   double* __restrict__ lp, int64_t N, int64_t ldlp)
{
    const int64_t total = N * n;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = g % N, i = g / N;
        double* out = lp + k + i * ldlp;
        if (*out == *out) continue;
        double acc = 0.0;
        for (int64_t j = 0; j < m; ++j) {
            const int c = cat[i + j * n];
            if (c != 0) acc += G[k + ((int64_t)(c - 1) * m + j) * ldg];
        }
        *out = acc;
    }
}

// ---- the slope ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void draw_beta_ord_kernel(BetaOrdArgs a)
{
    __shared__ double red[16];
    __shared__ double bt[9];
    const int64_t j = blockIdx.x;
    const int64_t n = a.n;
    const int C = a.C;
    const double* fj = a.f + j * n;
    const int8_t* cj = a.cat + j * n;
    const uint32_t item = a.item0 + (uint32_t)j;
    if (threadIdx.x < 9) bt[threadIdx.x] = (threadIdx.x >= 1 && (int)threadIdx.x < C) ? a.thr[j * (C - 1) + threadIdx.x - 1] : 0.0;
    __syncthreads();
    const double cv0 = a.beta[0 + 2 * j];                 // the pinned intercept: read, never written
    double cv1 = a.beta[1 + 2 * j];
    const double step = a.step[1 + 2 * j];
    const double z = qnorm_as241(item_uniform(a.seed, a.iter, GPIRT_ST_BETA, item, 2u));
    const double pv1 = ord_rnorm(cv1, step, z);                                 // draw-beta.cpp:22
    const double pm = a.pm[1 + 2 * j], ps = a.ps[1 + 2 * j];
    const double pv_prior = ord_dnorm_log(pv1, pm, ps);                         // :25
    const double cv_prior = ord_dnorm_log(cv1, pm, ps);                         // :26
    double accp = 0.0, accc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const int c = cj[i];
        if (c == 0) continue;
        const double th = a.theta[i], f = fj[i];
        const double mup = cv0 + th * pv1;
        const double muc = cv0 + th * cv1;
        ORD_TERMS(accp, c, f + mup, ll_term_fast);                              // :27
        ORD_TERMS(accc, c, f + muc, ll_term_fast);                              // :28
    }
    const double pv_ll = -block_sum_256(accp, red);
    const double cv_ll = -block_sum_256(accc, red);
    const double r = pv_prior + pv_ll - cv_prior - cv_ll;                       // :29
    const double u = item_uniform(a.seed, a.iter, GPIRT_ST_BETA, item, 3u);
    if (log(u) < r) cv1 = pv1;                                                  // :30-35
    if (threadIdx.x == 0) a.beta[1 + 2 * j] = cv1;
    if (a.mu)
        for (int64_t i = threadIdx.x; i < n; i += 256) a.mu[i + j * n] = cv0 + a.theta[i] * cv1;
    if (a.mu_star)
        for (int64_t i = threadIdx.x; i < a.N; i += 256) a.mu_star[i + j * a.N] = cv0 + (-5.0 + (double)i * 0.01) * cv1;
}

// ---- the thresholds (the operation order is stated at the head of this file) ----------------------------------------------------------
// REG = false (the 16384 class, 1024 lanes at most 128 registers): g and the categories are not held but formed again from f, mu
// and cat for every candidate, rows in the same order i = tid + NTH e (held, the compiler reported 104 bytes of scratch)
template <int EPT, int NTH, bool REG>
__global__ __launch_bounds__(NTH) void ord_thresholds_kernel(OrdThrArgs a)
{
    __shared__ double red[16];
    __shared__ double lpw[GPIRT_ORD_MAX_WIDTH];
    __shared__ int sk[10];                                 // sk[c] = K[j, c]; sk[0] = -1, sk[C] = P
    __shared__ int sfail;
    const int64_t j = blockIdx.x;
    const int64_t n = a.n;
    const int C = a.C, P = a.P, W = a.W;
    const int tid = threadIdx.x;
    const uint32_t item = a.item0 + (uint32_t)j;
    const double* fj = a.f + j * n;
    const double* mj = a.mu + j * n;
    const int8_t* cj = a.cat + j * n;
    double G[REG ? EPT : 1];
    static_assert(EPT <= 16, "4 bits per entry in one 64-bit word");
    uint64_t cats = 0;
    if (REG) {
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int64_t i = tid + NTH * e;
            const bool in = i < n;
            G[REG ? e : 0] = in ? fj[i] + mj[i] : 0.0;
            cats |= (uint64_t)(in ? (cj[i] & 15) : 0) << (4 * e);
        }
    }
    if (tid <= C) sk[tid] = tid == 0 ? -1 : (tid == C ? P : a.idx[j * (C - 1) + tid - 1]);
    if (tid == 0) sfail = 0;
    __syncthreads();
    for (int c = 1; c < C; ++c) {
        const int k = sk[c], left = sk[c - 1], right = sk[c + 1];
        const int64_t row = j * (C - 1) + (c - 1);
        const double u0 = item_uniform(a.seed, a.t, GPIRT_ST_ORD, item, (uint32_t)(2 * (c - 1)));
        int off = (int)(u0 * (double)W);
        if (off > W - 1) off = W - 1;
        const int a0 = k - off;
        int lo = a0 > left + 1 ? a0 : left + 1;
        if (lo < 0) lo = 0;
        int hi = a0 + W - 1 < right - 1 ? a0 + W - 1 : right - 1;
        if (hi > P - 1) hi = P - 1;
        if (tid < W) { lpw[tid] = -INFINITY; a.lp[row * W + tid] = -INFINITY; }
        if (tid == 0) a.window[row] = a0;
        __syncthreads();
        if (lo >= hi) {                                    // one candidate: k itself
            if (tid == 0) {
                a.lp[row * W + (k - a0)] = 0.0;
                atomicAdd((unsigned long long*)&a.stat[0], 1ull);
            }
            continue;
        }
        const double nc = (double)a.counts[j * C + c - 1], nc1 = (double)a.counts[j * C + c];
        for (int q = lo; q <= hi; ++q) {
            const double tq = a.grid[q];
            double acc = 0.0;
            if (REG) {
#pragma unroll
                for (int e = 0; e < (REG ? EPT : 1); ++e) {
                    const int ce = ORD_CAT(e);
                    if (ce == c || ce == c + 1) {
                        const double arg = ce == c ? tq - G[e] : G[e] - tq;
                        acc += ll_term_fast(arg);
                    }
                }
            } else {
                for (int64_t i = tid; i < n; i += NTH) {
                    const int ce = cj[i];
                    if (ce == c || ce == c + 1) {
                        const double g = fj[i] + mj[i];
                        const double arg = ce == c ? tq - g : g - tq;
                        acc += ll_term_fast(arg);
                    }
                }
            }
            const double S = ord_block_sum<NTH>(acc, red);
            double mq = a.log_prior[q] - S;
            if (left >= 0) mq = mq + nc * log1p(-exp(-(tq - a.grid[left])));
            if (right < P) mq = mq + nc1 * log1p(-exp(-(a.grid[right] - tq)));
            if (tid == 0) { lpw[q - a0] = mq; a.lp[row * W + (q - a0)] = mq; }
        }
        __syncthreads();
        if (tid == 0) {
            bool ok = true;
            double mx = -INFINITY;
            for (int q = lo; q <= hi; ++q) {
                const double v = lpw[q - a0];
                if (!isfinite(v)) ok = false;
                if (v > mx) mx = v;
            }
            if (!ok) {
                sfail = 1;
                atomicAdd((unsigned long long*)&a.stat[1], 1ull);
            } else {
                const double u1 = item_uniform(a.seed, a.t, GPIRT_ST_ORD, item, (uint32_t)(2 * (c - 1) + 1));
                double total = 0.0;
                for (int q = lo; q <= hi; ++q) { total += exp(lpw[q - a0] - mx); lpw[q - a0] = total; }
                const double target = u1 * total;
                int pick = hi;
                for (int q = hi; q >= lo; --q)
                    if (lpw[q - a0] > target) pick = q;
                sk[c] = pick;
                a.idx[row] = pick;
                a.thr[row] = a.grid[pick];
                atomicAdd((unsigned long long*)&a.stat[2], 1ull);
            }
        }
        __syncthreads();
        if (sfail) break;
    }
}

__global__ void ord_irf_kernel(const double* __restrict__ fstar, int64_t N, int64_t m, int C, const double* __restrict__ thr,
                               double* __restrict__ cum)
{
    const int64_t total = N * m * (C - 1);
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = g % N, r = g / N;               // r = (c - 1) + (C - 1) j
        const int64_t j = r / (C - 1);
        const double x = fstar[k + j * N] - thr[r];
        cum[g] += 1.0 / (1.0 + exp(-x));
    }
}

__global__ void ord_record_kernel(const int* __restrict__ idx, int64_t rows, int P, int64_t slot, uint32_t* __restrict__ hist,
                                  int32_t* __restrict__ draws)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int k = idx[r];
        draws[slot * rows + r] = k;
        if (k >= 0 && k < P) hist[r * P + k] += 1u;        // (one writer per row)
    }
}

inline unsigned ord_grid_for(int64_t total)
{
    int64_t b = (total + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace

int launch_ess_ord(hipStream_t stream, const EssOrdArgs& a)
{
    if (a.m <= 0) return 0;
    if (a.n <= 256 * 8) hipLaunchKernelGGL((ess_ord_kernel<8, 256, 3>), dim3((unsigned)a.m), dim3(256), 0, stream, a);
    else if (a.n <= 512 * 16) hipLaunchKernelGGL((ess_ord_kernel<16, 512, 2>), dim3((unsigned)a.m), dim3(512), 0, stream, a);
    else if (a.n <= 1024 * 16) hipLaunchKernelGGL((ess_ord_kernel<16, 1024, 0>), dim3((unsigned)a.m), dim3(1024), 0, stream, a);
    else { set_error("ordinal: n = %lld respondents, the slice kernel holds at most %d", (long long)a.n, GPIRT_ORD_MAX_N); return GPIRT_E_ARG; }
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ord_indicators(hipStream_t stream, const int8_t* cat, int64_t n, int64_t m, int C, double* Y)
{
    if (n * m <= 0) return 0;
    hipLaunchKernelGGL(ord_indicators_kernel, dim3(ord_grid_for(n * m)), dim3(256), 0, stream, cat, n * m, C, Y);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ord_counts(hipStream_t stream, const int8_t* cat, int64_t n, int64_t m, int C, long long* counts)
{
    if (m <= 0) return 0;
    hipLaunchKernelGGL(ord_counts_kernel, dim3((unsigned)m), dim3(256), 0, stream, cat, n, C, counts);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ord_loglik_terms(hipStream_t stream, const double* fstar, int64_t N, int64_t m, int C, const double* thr, double* G, int64_t ldg)
{
    if (N * m <= 0) return 0;
    hipLaunchKernelGGL(ord_loglik_terms_kernel, dim3(ord_grid_for(N * m)), dim3(256), 0, stream, fstar, N, m, C, thr, G, ldg);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ord_nan_fix(hipStream_t stream, const double* G, int64_t ldg, const int8_t* cat, int64_t n, int64_t m, double* lp, int64_t N,
                       int64_t ldlp)
{
    if (N * n <= 0) return 0;
    hipLaunchKernelGGL(ord_nan_fix_kernel, dim3(ord_grid_for(N * n)), dim3(256), 0, stream, G, ldg, cat, n, m, lp, N, ldlp);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_draw_beta_ord(hipStream_t stream, const BetaOrdArgs& a)
{
    if (a.m <= 0) return 0;
    hipLaunchKernelGGL(draw_beta_ord_kernel, dim3((unsigned)a.m), dim3(256), 0, stream, a);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ord_thresholds(hipStream_t stream, const OrdThrArgs& a)
{
    if (a.m <= 0) return 0;
    if (a.W < 1 || a.W > GPIRT_ORD_MAX_WIDTH || a.C < 2 || a.C > GPIRT_ORD_MAX_C) { set_error("ordinal: bad width or category count"); return GPIRT_E_ARG; }
    if (a.n <= 256 * 8) hipLaunchKernelGGL((ord_thresholds_kernel<8, 256, true>), dim3((unsigned)a.m), dim3(256), 0, stream, a);
    else if (a.n <= 512 * 16) hipLaunchKernelGGL((ord_thresholds_kernel<16, 512, true>), dim3((unsigned)a.m), dim3(512), 0, stream, a);
    else if (a.n <= 1024 * 16) hipLaunchKernelGGL((ord_thresholds_kernel<16, 1024, false>), dim3((unsigned)a.m), dim3(1024), 0, stream, a);
    else { set_error("ordinal: n = %lld respondents, the threshold kernel holds at most %d", (long long)a.n, GPIRT_ORD_MAX_N); return GPIRT_E_ARG; }
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ord_irf(hipStream_t stream, const double* fstar, int64_t N, int64_t m, int C, const double* thr, double* cum)
{
    if (N * m <= 0) return 0;
    hipLaunchKernelGGL(ord_irf_kernel, dim3(ord_grid_for(N * m * (C - 1))), dim3(256), 0, stream, fstar, N, m, C, thr, cum);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ord_record(hipStream_t stream, const int* idx, int64_t m, int C, int P, int64_t slot, uint32_t* hist, int32_t* draws)
{
    const int64_t rows = m * (C - 1);
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(ord_record_kernel, dim3(ord_grid_for(rows)), dim3(256), 0, stream, idx, rows, P, slot, hist, draws);
    GP_HIP(hipGetLastError());
    return 0;
}

void ord_grid_fill(double hi, int P, double* out)
{
    // t_k = -hi + k h in long double, rounded once: antisymmetric bit for bit, the centre exactly 0, the end points exact
    for (int k = 0; k < P; ++k)
        out[k] = (double)(((long double)(2 * k - (P - 1)) / (long double)(P - 1)) * (long double)hi);
}

}  // namespace gpirt

using namespace gpirt;

extern "C" {

int gpirt_ordinal_check(const int8_t* cat, const double* y, int64_t n, int64_t m, int C, double hi, int P, const double* log_prior,
                        const int32_t* K0, int W, const gpirt_options* opts)
{
    if (C < 2 || C > GPIRT_ORD_MAX_C) { set_error("ordinal: C = %d categories, it must lie in 2 .. %d", C, GPIRT_ORD_MAX_C); return GPIRT_E_ARG; }
    if (n < 0 || m < 0) { set_error("ordinal: n = %lld, m = %lld", (long long)n, (long long)m); return GPIRT_E_ARG; }
    if (n > GPIRT_ORD_MAX_N) {
        set_error("ordinal: n = %lld respondents is refused, the register-resident slice and threshold kernels hold at most %d", (long long)n,
                  GPIRT_ORD_MAX_N);
        return GPIRT_E_ARG;
    }
    if (P < GPIRT_ORD_MIN_POINTS || P > GPIRT_ORD_MAX_POINTS || P % 2 == 0) {
        set_error("ordinal: P = %d grid points, it must be odd (the centre is exactly 0) and lie in %d .. %d", P, GPIRT_ORD_MIN_POINTS,
                  GPIRT_ORD_MAX_POINTS);
        return GPIRT_E_ARG;
    }
    if (!std::isfinite(hi) || !(hi > 0.0) || !(hi <= 20.0)) { set_error("ordinal: hi = %g, it must lie in (0, 20]", hi); return GPIRT_E_ARG; }
    if (W < 1 || W > GPIRT_ORD_MAX_WIDTH) { set_error("ordinal: window width W = %d, it must lie in 1 .. %d", W, GPIRT_ORD_MAX_WIDTH); return GPIRT_E_ARG; }
    if (cat)
        for (int64_t g = 0; g < n * m; ++g) {
            if (cat[g] < 0 || cat[g] > C) {
                set_error("ordinal: cat[%lld, %lld] = %d, it must lie in 0 .. C = %d (0 = missing)", (long long)(g % (n ? n : 1)),
                          (long long)(g / (n ? n : 1)), (int)cat[g], C);
                return GPIRT_E_ARG;
            }
            if (y && ((y[g] != y[g]) != (cat[g] == 0))) {
                set_error("ordinal: y[%lld, %lld] must be NaN exactly where cat is 0 (the sampler is created on ordinal.dichotomise(cat))",
                          (long long)(g % n), (long long)(g / n));
                return GPIRT_E_ARG;
            }
        }
    if (log_prior)
        for (int k = 0; k < P; ++k)
            if (!std::isfinite(log_prior[k])) { set_error("ordinal: log_prior[%d] is not finite", k); return GPIRT_E_ARG; }
    if (K0)
        for (int64_t j = 0; j < m; ++j)
            for (int c = 0; c < C - 1; ++c) {
                const int k = K0[j * (C - 1) + c];
                if (k < 0 || k >= P) {
                    set_error("ordinal: K0[%lld, %d] = %d is off the grid 0 .. P - 1 = %d", (long long)j, c + 1, k, P - 1);
                    return GPIRT_E_ARG;
                }
                if (c > 0 && k <= K0[j * (C - 1) + c - 1]) {
                    set_error("ordinal: K0[%lld, .] is not strictly increasing at c = %d", (long long)j, c + 1);
                    return GPIRT_E_ARG;
                }
            }
    if (opts) {
        if (opts->rng_kind == GPIRT_RNG_RSTREAM) {
            set_error("ordinal: rng = reference (GPIRT_RNG_RSTREAM) is refused, R's stream has no such draw");
            return GPIRT_E_ARG;
        }
        if (opts->item0 != 0) {
            set_error("ordinal: an item shard (item0 = %lld, m_total = %lld) is refused, the respondent-block theta path has no one-hot product",
                      (long long)opts->item0, (long long)opts->m_total);
            return GPIRT_E_ARG;
        }
    }
    return 0;
}

int gpirt_ordinal_grid(double hi, int P, double* out)
{
    GP_ARG(out != nullptr);
    GP_TRY(gpirt_ordinal_check(nullptr, nullptr, 0, 0, 2, hi, P, nullptr, nullptr, 1, nullptr));
    ord_grid_fill(hi, P, out);
    return 0;
}

}  // extern "C"
