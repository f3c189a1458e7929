// summary.hip -- posterior summaries of a chain, accumulated on the device one draw at a time (O(n m) memory, however
// long the chain): Welford moments of theta, beta and f, the mean predictive probability P(y = 1) of every cell (the
// held-out prediction of a missing one), and the pointwise terms of WAIC -- lppd_ij = log mean_s exp(ll_s) as a running
// logaddexp, p_waic_ij = the sample variance of ll_s (Welford).  For cell (i, j) of draw s: g = f + mu (mu = X beta, the
// sampler's own array), P(y = 1) = plogis(g) and ll = -softplus(-y g) (src/log-likelihood.cpp:25-37), in the stable form
// log1p(exp(-|a|)) + max(-a, 0).
//
// summary_accumulate_kernel is one streaming pass: f, mu and y read once, each accumulator read and written once, 16 bytes
// per lane; theta and beta (n + 2m values) ride in the same launch.  The totals are reduced in a fixed order (block partials,
// then one block), without atomics: bit-identical from run to run.
#include "common.h"
#include "kernels.h"

namespace gpirt {

namespace {

constexpr int SUM_THREADS = 256;
constexpr int SUM_MAX_BLOCKS = 2048;
constexpr int SUM_TOTAL_BLOCKS = 1024;       // fixed: the order of the totals' sums does not depend on the device

struct SumArgs {
    const double* f; const double* mu; const double* y; const double* theta; const double* beta;
    double* lse; double* ll_mean; double* ll_m2; double* p_sum; double* f_mean; double* f_m2;
    double* tb_mean; double* tb_m2;
    int64_t cells, n, m;
};

struct CellOut { double ll, p; };

// P(y = 1) and ll for one cell; exp(-|g|) serves both (|y g| = |g| for y = +-1)
__device__ __forceinline__ CellOut cell_terms(double g, double y)
{
    const double e = exp(-fabs(g));
    const double a = y * g;
    CellOut o;
    o.p = g >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
    o.ll = -(log1p(e) + fmax(-a, 0.0));
    return o;
}

__device__ __forceinline__ void welford(double& mean, double& m2, double x, double d)
{
    const double delta = x - mean;
    mean += delta / d;
    m2 += delta * (x - mean);
}

// lse := log(exp(lse) + exp(ll)); the first draw sets it
__device__ __forceinline__ double logaddexp(double lse, double ll, bool first)
{
    if (first) return ll;
    return fmax(lse, ll) + log1p(exp(-fabs(lse - ll)));
}

template <bool WAIC, bool PRED, bool F>
__device__ __forceinline__ void accumulate_cell(const SumArgs& a, double fv, double muv, double yv, double& lse, double& lm,
                                                double& l2, double& ps, double& fm, double& f2, double d, bool first)
{
    if (WAIC || PRED) {
        const CellOut c = cell_terms(fv + muv, yv);
        if (WAIC) { lse = logaddexp(lse, c.ll, first); welford(lm, l2, c.ll, d); }
        if (PRED) ps += c.p;
    }
    if (F) welford(fm, f2, fv, d);
}

// draw d (1-based) of the chain: cells as pairs (double2 loads / stores; every array is 16-byte aligned), an odd last cell,
// then the n + 2m values of theta and beta
template <bool WAIC, bool PRED, bool F>
__global__ __launch_bounds__(SUM_THREADS) void summary_accumulate_kernel(SumArgs a, int64_t draw)
{
    const double d = (double)draw;
    const bool first = draw == 1;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (WAIC || PRED || F) {
        const int64_t pairs = a.cells >> 1;
        const double2* f2p = reinterpret_cast<const double2*>(a.f);
        const double2* m2p = reinterpret_cast<const double2*>(a.mu);
        const double2* y2p = reinterpret_cast<const double2*>(a.y);
        for (int64_t q = tid; q < pairs; q += stride) {
            const double2 fv = f2p[q], mv = m2p[q], yv = y2p[q];
            double2 lse{}, lm{}, l2{}, ps{}, fm{}, fq{};
            if (WAIC) {
                lse = reinterpret_cast<const double2*>(a.lse)[q];
                lm = reinterpret_cast<const double2*>(a.ll_mean)[q];
                l2 = reinterpret_cast<const double2*>(a.ll_m2)[q];
            }
            if (PRED) ps = reinterpret_cast<const double2*>(a.p_sum)[q];
            if (F) {
                fm = reinterpret_cast<const double2*>(a.f_mean)[q];
                fq = reinterpret_cast<const double2*>(a.f_m2)[q];
            }
            accumulate_cell<WAIC, PRED, F>(a, fv.x, mv.x, yv.x, lse.x, lm.x, l2.x, ps.x, fm.x, fq.x, d, first);
            accumulate_cell<WAIC, PRED, F>(a, fv.y, mv.y, yv.y, lse.y, lm.y, l2.y, ps.y, fm.y, fq.y, d, first);
            if (WAIC) {
                reinterpret_cast<double2*>(a.lse)[q] = lse;
                reinterpret_cast<double2*>(a.ll_mean)[q] = lm;
                reinterpret_cast<double2*>(a.ll_m2)[q] = l2;
            }
            if (PRED) reinterpret_cast<double2*>(a.p_sum)[q] = ps;
            if (F) {
                reinterpret_cast<double2*>(a.f_mean)[q] = fm;
                reinterpret_cast<double2*>(a.f_m2)[q] = fq;
            }
        }
        if ((a.cells & 1) && tid == 0) {
            const int64_t c = a.cells - 1;
            double lse = 0, lm = 0, l2 = 0, ps = 0, fm = 0, fq = 0;
            if (WAIC) { lse = a.lse[c]; lm = a.ll_mean[c]; l2 = a.ll_m2[c]; }
            if (PRED) ps = a.p_sum[c];
            if (F) { fm = a.f_mean[c]; fq = a.f_m2[c]; }
            accumulate_cell<WAIC, PRED, F>(a, a.f[c], a.mu[c], a.y[c], lse, lm, l2, ps, fm, fq, d, first);
            if (WAIC) { a.lse[c] = lse; a.ll_mean[c] = lm; a.ll_m2[c] = l2; }
            if (PRED) a.p_sum[c] = ps;
            if (F) { a.f_mean[c] = fm; a.f_m2[c] = fq; }
        }
    }
    const int64_t tb = a.n + 2 * a.m;
    for (int64_t i = tid; i < tb; i += stride) {
        const double x = i < a.n ? a.theta[i] : a.beta[i - a.n];
        double mean = a.tb_mean[i], m2 = a.tb_m2[i];
        welford(mean, m2, x, d);
        a.tb_mean[i] = mean; a.tb_m2[i] = m2;
    }
}

// out[i] = src[i] * scale + shift, NaN where the response is missing (y != nullptr)
__global__ __launch_bounds__(SUM_THREADS) void summary_finish_kernel(const double* __restrict__ src, const double* __restrict__ y,
                                                                     int64_t count, double scale, double shift,
                                                                     double* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = src[i] * scale + shift;
        out[i] = (y && y[i] != y[i]) ? (double)NAN : v;
    }
}

template <int K>
__device__ void block_sum(double (&v)[K], double (*sh)[SUM_THREADS])
{
    const int t = threadIdx.x;
    for (int k = 0; k < K; ++k) sh[k][t] = v[k];
    __syncthreads();
    for (int w = SUM_THREADS / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int k = 0; k < K; ++k) sh[k][t] += sh[k][t + w];
        __syncthreads();
    }
    for (int k = 0; k < K; ++k) v[k] = sh[k][0];
}

// totals over the observed cells, block partials.  pass 0: [sum lppd_ij, sum p_waic_ij, n_obs, sum elpd_ij];
// pass 1: [sum (elpd_ij - mean)^2] with mean = tot[GPIRT_SUM_T_ELPD_MEAN] of pass 0
__global__ __launch_bounds__(SUM_THREADS) void summary_totals_kernel(const double* __restrict__ lse, const double* __restrict__ m2,
                                                                     const double* __restrict__ y, int64_t cells, double log_s,
                                                                     double inv_s1, int pass, const double* __restrict__ tot,
                                                                     double* __restrict__ part)
{
    __shared__ double sh[4][SUM_THREADS];
    double v[4] = { 0.0, 0.0, 0.0, 0.0 };
    const double mean = pass ? tot[GPIRT_SUM_T_ELPD_MEAN] : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
        if (y[i] != y[i]) continue;
        const double lppd = lse[i] - log_s, pw = m2[i] * inv_s1, e = lppd - pw;
        if (pass == 0) { v[0] += lppd; v[1] += pw; v[2] += 1.0; v[3] += e; }
        else { const double dv = e - mean; v[0] += dv * dv; }
    }
    block_sum<4>(v, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) part[(int64_t)blockIdx.x * 4 + k] = v[k];
}

// one block: the partials in block order, then the derived totals (include/gpirt_hip.h GPIRT_SUM_T_*)
__global__ __launch_bounds__(SUM_THREADS) void summary_reduce_kernel(const double* __restrict__ part, int nblocks, int pass,
                                                                     double draws, double* __restrict__ tot)
{
    __shared__ double sh[4][SUM_THREADS];
    double v[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (int b = threadIdx.x; b < nblocks; b += SUM_THREADS)
        for (int k = 0; k < 4; ++k) v[k] += part[(int64_t)b * 4 + k];
    block_sum<4>(v, sh);
    if (threadIdx.x != 0) return;
    if (pass == 0) {
        tot[GPIRT_SUM_T_LPPD] = v[0];
        tot[GPIRT_SUM_T_P_WAIC] = v[1];
        tot[GPIRT_SUM_T_ELPD_WAIC] = v[0] - v[1];
        tot[GPIRT_SUM_T_WAIC] = -2.0 * (v[0] - v[1]);
        tot[GPIRT_SUM_T_N_OBS] = v[2];
        tot[GPIRT_SUM_T_DRAWS] = draws;
        tot[GPIRT_SUM_T_ELPD_MEAN] = v[3] / v[2];
    } else {
        const double nobs = tot[GPIRT_SUM_T_N_OBS];
        tot[GPIRT_SUM_T_ELPD_SS] = v[0];
        tot[GPIRT_SUM_T_SE_ELPD_WAIC] = sqrt(nobs * (v[0] / (nobs - 1.0)));     // loo: sqrt(N var(elpd_i)), ddof = 1
    }
}

int grid_cap(int64_t work)
{
    const int64_t b = (work + SUM_THREADS - 1) / SUM_THREADS;
    return (int)(b < 1 ? 1 : (b > SUM_MAX_BLOCKS ? SUM_MAX_BLOCKS : b));
}

template <bool W, bool P, bool F>
void launch_acc(hipStream_t st, const SumArgs& a, int64_t draw)
{
    const int64_t work = (W || P || F) ? (a.cells >> 1) : a.n + 2 * a.m;
    const int64_t tb = a.n + 2 * a.m;
    hipLaunchKernelGGL((summary_accumulate_kernel<W, P, F>), dim3(grid_cap(work > tb ? work : tb)), dim3(SUM_THREADS), 0, st, a,
                       draw);
}

}  // namespace

int summary_alloc(SummaryState* s, int64_t n, int64_t m, int parts)
{
    const size_t cells = (size_t)(n * m), tb = (size_t)(n + 2 * m);
    auto get = [&](double** p, size_t count) -> int {
        GP_HIP(hipMalloc(p, count * sizeof(double)));
        s->allocs.push_back(*p);
        GP_HIP(hipMemset(*p, 0, count * sizeof(double)));
        return 0;
    };
    s->n = n; s->m = m; s->parts = parts; s->draws = 0;
    GP_TRY(get(&s->tb_mean, tb)); GP_TRY(get(&s->tb_m2, tb));
    if (parts & GPIRT_SUM_WAIC) { GP_TRY(get(&s->lse, cells)); GP_TRY(get(&s->ll_mean, cells)); GP_TRY(get(&s->ll_m2, cells)); }
    if (parts & GPIRT_SUM_PRED) GP_TRY(get(&s->p_sum, cells));
    if (parts & GPIRT_SUM_F) { GP_TRY(get(&s->f_mean, cells)); GP_TRY(get(&s->f_m2, cells)); }
    GP_TRY(get(&s->out, cells > tb ? cells : tb));
    GP_TRY(get(&s->part, (size_t)SUM_TOTAL_BLOCKS * 4));
    GP_TRY(get(&s->tot, GPIRT_SUM_NTOTALS));
    return 0;
}

void summary_free(SummaryState* s)
{
    for (void* p : s->allocs) hipFree(p);
    *s = SummaryState{};
}

int launch_summary_accumulate(hipStream_t st, SummaryState* s, const double* theta, const double* beta, const double* f,
                              const double* mu, const double* y)
{
    if ((((uintptr_t)f | (uintptr_t)mu | (uintptr_t)y) & 15) != 0) {
        set_error("summary: f, mu and y must be 16-byte aligned");
        return GPIRT_E_ARG;
    }
    SumArgs a{};
    a.f = f; a.mu = mu; a.y = y; a.theta = theta; a.beta = beta;
    a.lse = s->lse; a.ll_mean = s->ll_mean; a.ll_m2 = s->ll_m2; a.p_sum = s->p_sum; a.f_mean = s->f_mean; a.f_m2 = s->f_m2;
    a.tb_mean = s->tb_mean; a.tb_m2 = s->tb_m2;
    a.cells = s->n * s->m; a.n = s->n; a.m = s->m;
    const int64_t draw = s->draws + 1;
    const bool w = s->parts & GPIRT_SUM_WAIC, p = s->parts & GPIRT_SUM_PRED, fo = s->parts & GPIRT_SUM_F;
    switch ((w ? 4 : 0) | (p ? 2 : 0) | (fo ? 1 : 0)) {
        case 0: launch_acc<false, false, false>(st, a, draw); break;
        case 1: launch_acc<false, false, true>(st, a, draw); break;
        case 2: launch_acc<false, true, false>(st, a, draw); break;
        case 3: launch_acc<false, true, true>(st, a, draw); break;
        case 4: launch_acc<true, false, false>(st, a, draw); break;
        case 5: launch_acc<true, false, true>(st, a, draw); break;
        case 6: launch_acc<true, true, false>(st, a, draw); break;
        default: launch_acc<true, true, true>(st, a, draw); break;
    }
    GP_HIP(hipGetLastError());
    s->draws = draw;
    return 0;
}

int summary_array(const SummaryState* s, const char* name, const double** src, int64_t* count, double* scale, double* shift,
                  bool* masked)
{
    const double S = (double)s->draws;
    const double nan = (double)NAN;
    const double mean_scale = s->draws >= 1 ? 1.0 : nan, var_scale = s->draws >= 2 ? 1.0 / (S - 1.0) : nan;
    const int64_t cells = s->n * s->m;
    struct E { const char* k; const double* p; int64_t c; double sc, sh; bool mask; int part; } tab[] = {
        { "p_yes", s->p_sum, cells, s->draws >= 1 ? 1.0 / S : nan, 0.0, false, GPIRT_SUM_PRED },
        { "lppd", s->lse, cells, mean_scale, s->draws >= 1 ? -log(S) : nan, true, GPIRT_SUM_WAIC },
        { "p_waic", s->ll_m2, cells, var_scale, 0.0, true, GPIRT_SUM_WAIC },
        { "f_mean", s->f_mean, cells, mean_scale, 0.0, false, GPIRT_SUM_F },
        { "f_var", s->f_m2, cells, var_scale, 0.0, false, GPIRT_SUM_F },
        { "theta_mean", s->tb_mean, s->n, mean_scale, 0.0, false, 0 },
        { "theta_var", s->tb_m2, s->n, var_scale, 0.0, false, 0 },
        { "beta_mean", s->tb_mean ? s->tb_mean + s->n : nullptr, 2 * s->m, mean_scale, 0.0, false, 0 },
        { "beta_var", s->tb_m2 ? s->tb_m2 + s->n : nullptr, 2 * s->m, var_scale, 0.0, false, 0 },
    };
    for (const E& e : tab) {
        if (strcmp(e.k, name) != 0) continue;
        if (!s->parts || (e.part && !(s->parts & e.part))) {
            set_error("summary '%s' was not enabled (gpirt_sampler_summary_enable)", name);
            return GPIRT_E_ARG;
        }
        *src = e.p; *count = e.c; *scale = e.sc; *shift = e.sh; *masked = e.mask;
        return 0;
    }
    set_error("unknown summary '%s'", name);
    return GPIRT_E_ARG;
}

int launch_summary_finish(hipStream_t st, const SummaryState* s, const char* name, const double* y, double** d_out,
                          int64_t* count)
{
    const double* src; double scale, shift; bool masked;
    GP_TRY(summary_array(s, name, &src, count, &scale, &shift, &masked));
    hipLaunchKernelGGL(summary_finish_kernel, dim3(grid_cap(*count)), dim3(SUM_THREADS), 0, st, src, masked ? y : nullptr,
                       *count, scale, shift, s->out);
    GP_HIP(hipGetLastError());
    *d_out = s->out;
    return 0;
}

int launch_summary_totals(hipStream_t st, const SummaryState* s, const double* y)
{
    if (!(s->parts & GPIRT_SUM_WAIC)) {
        set_error("summary totals need GPIRT_SUM_WAIC");
        return GPIRT_E_ARG;
    }
    const double S = (double)s->draws;
    const double log_s = s->draws >= 1 ? log(S) : (double)NAN, inv_s1 = s->draws >= 2 ? 1.0 / (S - 1.0) : (double)NAN;
    const int64_t cells = s->n * s->m;
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(summary_totals_kernel, dim3(SUM_TOTAL_BLOCKS), dim3(SUM_THREADS), 0, st, s->lse, s->ll_m2, y, cells,
                           log_s, inv_s1, pass, s->tot, s->part);
        GP_HIP(hipGetLastError());
        hipLaunchKernelGGL(summary_reduce_kernel, dim3(1), dim3(SUM_THREADS), 0, st, s->part, SUM_TOTAL_BLOCKS, pass, S, s->tot);
        GP_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace gpirt
