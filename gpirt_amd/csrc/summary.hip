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
//
// GPIRT_SUM_DIAG adds, in the same pass, the split-half and batch-means accumulators of split-R-hat and a batch-means ESS
// (summary_diag_accumulate_kernel).  Every accumulator of a chain lives in ONE device block (header, arrays, y, the IRF sum),
// and chains_combine pools C such blocks -- Chan's formula, a logaddexp over chains, the theta -> -theta reflection applied
// to the means -- into a state of C S draws that the finish and totals kernels read as they read one chain's
// (include/gpirt_hip.h).
#include "common.h"
#include "kernels.h"

#include <algorithm>

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

// GPIRT_SUM_DIAG: which accumulators draw d touches depends on d only (uniform over the grid).  half: 0 none, 1 or 2 (hd = the
// draw's count within that half); batch: 0 past the a b batched draws, 1 add to the batch sum, 2 add and close batch bk of
// size bd (its mean enters the Welford of the batch means, the sum restarts at 0).  The pointers are the draw's half's.
struct DiagArgs {
    double *t_hm, *t_h2, *t_bs, *t_bmm, *t_bm2;      // theta / beta (n + 2m)
    double *f_hm, *f_h2, *f_bs, *f_bmm, *f_bm2;      // f (n x m; with F)
    double hd, bd, bk;
    int half, batch;
};

__device__ __forceinline__ void diag_value(const DiagArgs& g, double x, double& hm, double& h2, double& bs, double& bmm,
                                           double& bm2)
{
    if (g.half) welford(hm, h2, x, g.hd);
    if (g.batch == 2) { welford(bmm, bm2, (bs + x) / g.bd, g.bk); bs = 0.0; }
    else if (g.batch == 1) bs += x;
}

template <bool DIAG>
__device__ __forceinline__ void diag_load2(const DiagArgs& g, double* hmp, double* h2p, double* bsp, double* bmmp,
                                           double* bm2p, int64_t q, double2& hm, double2& h2, double2& bs, double2& bmm,
                                           double2& bm2)
{
    if (!DIAG) return;
    if (g.half) { hm = reinterpret_cast<const double2*>(hmp)[q]; h2 = reinterpret_cast<const double2*>(h2p)[q]; }
    if (g.batch) bs = reinterpret_cast<const double2*>(bsp)[q];
    if (g.batch == 2) { bmm = reinterpret_cast<const double2*>(bmmp)[q]; bm2 = reinterpret_cast<const double2*>(bm2p)[q]; }
}

template <bool DIAG>
__device__ __forceinline__ void diag_store2(const DiagArgs& g, double* hmp, double* h2p, double* bsp, double* bmmp,
                                            double* bm2p, int64_t q, const double2& hm, const double2& h2, const double2& bs,
                                            const double2& bmm, const double2& bm2)
{
    if (!DIAG) return;
    if (g.half) { reinterpret_cast<double2*>(hmp)[q] = hm; reinterpret_cast<double2*>(h2p)[q] = h2; }
    if (g.batch) reinterpret_cast<double2*>(bsp)[q] = bs;
    if (g.batch == 2) { reinterpret_cast<double2*>(bmmp)[q] = bmm; reinterpret_cast<double2*>(bm2p)[q] = bm2; }
}

// one value of an array without a vector form (the odd last cell, theta and beta)
template <bool DIAG>
__device__ __forceinline__ void diag_scalar(const DiagArgs& g, double* hmp, double* h2p, double* bsp, double* bmmp, double* bm2p,
                                            int64_t i, double x)
{
    if (!DIAG) return;
    double hm = 0, h2 = 0, bs = 0, bmm = 0, bm2 = 0;
    if (g.half) { hm = hmp[i]; h2 = h2p[i]; }
    if (g.batch) bs = bsp[i];
    if (g.batch == 2) { bmm = bmmp[i]; bm2 = bm2p[i]; }
    diag_value(g, x, hm, h2, bs, bmm, bm2);
    if (g.half) { hmp[i] = hm; h2p[i] = h2; }
    if (g.batch) bsp[i] = bs;
    if (g.batch == 2) { bmmp[i] = bmm; bm2p[i] = bm2; }
}

// summary_accumulate_kernel with the GPIRT_SUM_DIAG accumulators (split halves, batch means) added in the same pass -- f's
// only with F --, so f is still read once.  (The kernel above is kept as it was: its instances' code does not move.)
template <bool WAIC, bool PRED, bool F, bool DIAG>
__device__ __forceinline__ void accumulate_body(const SumArgs& a, const DiagArgs& g, int64_t draw)
{
    const double d = (double)draw;
    const bool first = draw == 1;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    constexpr bool FD = DIAG && F;
    if (WAIC || PRED || F) {
        const int64_t pairs = a.cells >> 1;
        const double2* f2p = reinterpret_cast<const double2*>(a.f);
        const double2* m2p = reinterpret_cast<const double2*>(a.mu);
        const double2* y2p = reinterpret_cast<const double2*>(a.y);
        for (int64_t q = tid; q < pairs; q += stride) {
            const double2 fv = f2p[q], mv = m2p[q], yv = y2p[q];
            double2 lse{}, lm{}, l2{}, ps{}, fm{}, fq{};
            double2 hm{}, h2{}, bs{}, bmm{}, bm2{};
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
            diag_load2<FD>(g, g.f_hm, g.f_h2, g.f_bs, g.f_bmm, g.f_bm2, q, hm, h2, bs, bmm, bm2);
            accumulate_cell<WAIC, PRED, F>(a, fv.x, mv.x, yv.x, lse.x, lm.x, l2.x, ps.x, fm.x, fq.x, d, first);
            accumulate_cell<WAIC, PRED, F>(a, fv.y, mv.y, yv.y, lse.y, lm.y, l2.y, ps.y, fm.y, fq.y, d, first);
            if (FD) {
                diag_value(g, fv.x, hm.x, h2.x, bs.x, bmm.x, bm2.x);
                diag_value(g, fv.y, hm.y, h2.y, bs.y, bmm.y, bm2.y);
            }
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
            diag_store2<FD>(g, g.f_hm, g.f_h2, g.f_bs, g.f_bmm, g.f_bm2, q, hm, h2, bs, bmm, bm2);
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
            diag_scalar<FD>(g, g.f_hm, g.f_h2, g.f_bs, g.f_bmm, g.f_bm2, c, a.f[c]);
        }
    }
    const int64_t tb = a.n + 2 * a.m;
    for (int64_t i = tid; i < tb; i += stride) {
        const double x = i < a.n ? a.theta[i] : a.beta[i - a.n];
        double mean = a.tb_mean[i], m2 = a.tb_m2[i];
        welford(mean, m2, x, d);
        a.tb_mean[i] = mean; a.tb_m2[i] = m2;
        diag_scalar<DIAG>(g, g.t_hm, g.t_h2, g.t_bs, g.t_bmm, g.t_bm2, i, x);
    }
}

// the same pass with the GPIRT_SUM_DIAG accumulators
template <bool WAIC, bool PRED, bool F>
__global__ __launch_bounds__(SUM_THREADS) void summary_diag_accumulate_kernel(SumArgs a, DiagArgs g, int64_t draw)
{
    accumulate_body<WAIC, PRED, F, true>(a, g, draw);
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

template <bool W, bool P, bool F>
void launch_diag_acc(hipStream_t st, const SumArgs& a, const DiagArgs& g, int64_t draw)
{
    const int64_t work = (W || P || F) ? (a.cells >> 1) : a.n + 2 * a.m;
    const int64_t tb = a.n + 2 * a.m;
    hipLaunchKernelGGL((summary_diag_accumulate_kernel<W, P, F>), dim3(grid_cap(work > tb ? work : tb)), dim3(SUM_THREADS), 0,
                       st, a, g, draw);
}

int64_t isqrt(int64_t S)
{
    int64_t b = (int64_t)sqrt((double)S);
    while (b > 1 && b * b > S) --b;
    while ((b + 1) * (b + 1) <= S) ++b;
    return b < 1 ? 1 : b;
}

// DiagArgs of draw d (1-based) of a chain of S planned draws
DiagArgs diag_step(const SummaryState* s, int64_t d)
{
    DiagArgs g{};
    const int64_t S = s->planned, hN = S / 2, b = isqrt(S), nb = S / b;
    if (d <= hN) { g.half = 1; g.hd = (double)d; }
    else if (d > S - hN) { g.half = 2; g.hd = (double)(d - (S - hN)); }
    if (d <= nb * b) { g.batch = d % b == 0 ? 2 : 1; g.bd = (double)b; g.bk = (double)(d / b); }
    const int h0 = g.half == 2 ? DG_H2_MEAN : DG_H1_MEAN, h1 = g.half == 2 ? DG_H2_M2 : DG_H1_M2;
    g.t_hm = s->dtb[h0]; g.t_h2 = s->dtb[h1]; g.t_bs = s->dtb[DG_BSUM]; g.t_bmm = s->dtb[DG_BM_MEAN]; g.t_bm2 = s->dtb[DG_BM_M2];
    g.f_hm = s->df[h0]; g.f_h2 = s->df[h1]; g.f_bs = s->df[DG_BSUM]; g.f_bmm = s->df[DG_BM_MEAN]; g.f_bm2 = s->df[DG_BM_M2];
    return g;
}

// ---- GPIRT_SUM_THETA_HIST / GPIRT_SUM_IRF_BAND: the histograms of a draw -------------------------------------------------
constexpr int NG = GPIRT_NGRID;

struct HistArgs {
    const double* theta; const double* fstar; const double* edges;
    uint32_t *th_all, *th_half, *th_off;     // th_half: the draw's DIAG half (nullptr: in neither, or no DIAG)
    uint32_t *band, *band_nan;
    double* psum;
    int64_t n, nm;
};

__device__ __forceinline__ double plogis(double x)
{
    const double e = exp(-fabs(x));
    return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// One lane owns one f* cell, or one respondent, of the draw: every counter it increments is its own -- no atomics, the same
// counts from run to run.  A cell's value goes in bin #{b : e_b <= x} (a binary search over the 255 edges in LDS); the bins
// are bin-major with the cell fastest, so neighbouring grid points, which mostly share a bin, share cache lines.
template <bool TH, bool BAND>
__global__ __launch_bounds__(SUM_THREADS) void summary_hist_accumulate_kernel(HistArgs a)
{
    __shared__ double e[GPIRT_IRF_BINS];
    if (BAND) {
        for (int b = threadIdx.x; b < GPIRT_IRF_BINS - 1; b += SUM_THREADS) e[b] = a.edges[b];
        __syncthreads();
    }
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (BAND)
        for (int64_t c = tid; c < a.nm; c += stride) {
            const double x = a.fstar[c];
            a.psum[c] += plogis(x);
            if (x != x) { a.band_nan[c] += 1u; continue; }
            int b = 0;
            for (int step = GPIRT_IRF_BINS / 2; step > 0; step >>= 1)
                if (b + step <= GPIRT_IRF_BINS - 1 && e[b + step - 1] <= x) b += step;
            a.band[(int64_t)b * a.nm + c] += 1u;
        }
    if (TH)
        for (int64_t i = tid; i < a.n; i += stride) {
            const double t = a.theta[i];
            const double k = rint((t + 5.0) * 100.0);
            if (!(k >= 0.0 && k <= (double)(NG - 1) && -5.0 + k * 0.01 == t)) { a.th_off[i] += 1u; continue; }
            const int64_t at = i * NG + (int64_t)k;
            a.th_all[at] += 1u;
            if (a.th_half) a.th_half[at] += 1u;
        }
}

template <bool TH, bool BAND>
void launch_hist_t(hipStream_t st, const HistArgs& a)
{
    const int64_t work = BAND ? (a.nm > a.n ? a.nm : a.n) : a.n;
    hipLaunchKernelGGL((summary_hist_accumulate_kernel<TH, BAND>), dim3(grid_cap(work)), dim3(SUM_THREADS), 0, st, a);
}

// the histogram launch of draw d (1-based), after the moments' own
int launch_hist(hipStream_t st, const SummaryState* s, const double* theta, const double* fstar, int64_t d)
{
    const bool th = s->parts & GPIRT_SUM_THETA_HIST, band = s->parts & GPIRT_SUM_IRF_BAND;
    if (!th && !band) return 0;
    HistArgs a{};
    a.theta = theta; a.fstar = fstar; a.edges = s->edges;
    a.th_all = s->th_hist[0]; a.th_off = s->th_off; a.band = s->band; a.band_nan = s->band_nan; a.psum = s->psum;
    a.n = s->n; a.nm = (int64_t)NG * s->m;
    if (th && (s->parts & GPIRT_SUM_DIAG)) {              // DIAG's halves: draws 1..floor(S/2) and the last floor(S/2)
        const int64_t S = s->planned, hN = S / 2;
        if (d <= hN) a.th_half = s->th_hist[1];
        else if (d > S - hN) a.th_half = s->th_hist[2];
    }
    if (th && band) launch_hist_t<true, true>(st, a);
    else if (th) launch_hist_t<true, false>(st, a);
    else launch_hist_t<false, true>(st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

}  // namespace

SumLayout summary_layout(int64_t n, int64_t m, int parts)
{
    SumLayout L;
    const int64_t cells = n * m, tb = n + 2 * m;
    int64_t at = SUM_HEADER_WORDS;
    auto take = [&](int64_t count) { const int64_t o = at; at += (count + 1) & ~(int64_t)1; return o; };
    L.tb_mean = take(tb); L.tb_m2 = take(tb);
    if (parts & GPIRT_SUM_WAIC) { L.lse = take(cells); L.ll_mean = take(cells); L.ll_m2 = take(cells); L.y = take(cells); }
    if (parts & GPIRT_SUM_PRED) L.p_sum = take(cells);
    if (parts & GPIRT_SUM_F) { L.f_mean = take(cells); L.f_m2 = take(cells); }
    L.irf = take((int64_t)GPIRT_NGRID * m);
    if (parts & GPIRT_SUM_DIAG) {
        for (int k = 0; k < 7; ++k) L.dtb[k] = take(tb);
        if (parts & GPIRT_SUM_F)
            for (int k = 0; k < 7; ++k) L.df[k] = take(cells);
    }
    L.total = at;
    return L;
}

QntLayout quantile_layout(int64_t n, int64_t m, int parts)
{
    QntLayout Q;
    int64_t at = summary_layout(n, m, parts).total;
    auto take_u32 = [&](int64_t count) { const int64_t o = at; const int64_t w = (count + 1) / 2; at += (w + 1) & ~(int64_t)1; return o; };
    if (parts & GPIRT_SUM_THETA_HIST) {
        Q.th_hist[0] = take_u32(n * NG);
        if (parts & GPIRT_SUM_DIAG) { Q.th_hist[1] = take_u32(n * NG); Q.th_hist[2] = take_u32(n * NG); }
        Q.th_off = take_u32(n);
    }
    if (parts & GPIRT_SUM_IRF_BAND) {
        const int64_t nm = (int64_t)NG * m;
        Q.psum = at; at += (nm + 1) & ~(int64_t)1;
        Q.band_nan = take_u32(nm);
        Q.band = take_u32(nm * GPIRT_IRF_BINS);
    }
    Q.total = at;
    return Q;
}

// logit(b / 256) = log1p((2b - 256) / (256 - b)): log(b) - log(256 - b) cancels near b = 128 (up to 109 ulp off at b = 125);
// this form stays within 4 ulp of the correctly rounded edge
void irf_band_edges(double* out)
{
    const double B = (double)GPIRT_IRF_BINS;
    for (int b = 1; b < GPIRT_IRF_BINS; ++b) out[b - 1] = log1p((2.0 * b - B) / (B - b));
}

int summary_alloc(SummaryState* s, int64_t n, int64_t m, int parts, int64_t planned)
{
    const size_t cells = (size_t)(n * m), tb = (size_t)(n + 2 * m);
    auto get = [&](double** p, size_t count) -> int {
        GP_HIP(hipMalloc(p, count * sizeof(double)));
        s->allocs.push_back(*p);
        GP_HIP(hipMemset(*p, 0, count * sizeof(double)));
        return 0;
    };
    s->n = n; s->m = m; s->parts = parts; s->draws = 0; s->planned = planned;
    s->lay = summary_layout(n, m, parts);
    s->qlay = quantile_layout(n, m, parts);
    GP_TRY(get(&s->block, (size_t)s->qlay.total));
    auto at = [&](int64_t off) { return off < 0 ? nullptr : s->block + off; };
    auto atu = [&](int64_t off) { return off < 0 ? nullptr : reinterpret_cast<uint32_t*>(s->block + off); };
    const SumLayout& L = s->lay;
    s->tb_mean = at(L.tb_mean); s->tb_m2 = at(L.tb_m2);
    s->lse = at(L.lse); s->ll_mean = at(L.ll_mean); s->ll_m2 = at(L.ll_m2); s->y = at(L.y);
    s->p_sum = at(L.p_sum); s->f_mean = at(L.f_mean); s->f_m2 = at(L.f_m2); s->irf = at(L.irf);
    for (int k = 0; k < 7; ++k) { s->dtb[k] = at(L.dtb[k]); s->df[k] = at(L.df[k]); }
    const QntLayout& Q = s->qlay;
    for (int k = 0; k < 3; ++k) s->th_hist[k] = atu(Q.th_hist[k]);
    s->th_off = atu(Q.th_off); s->band = atu(Q.band); s->band_nan = atu(Q.band_nan); s->psum = at(Q.psum);
    if (parts & GPIRT_SUM_IRF_BAND) {
        double e[GPIRT_IRF_BINS - 1];
        irf_band_edges(e);
        GP_TRY(get(&s->edges, GPIRT_IRF_BINS));
        GP_HIP(hipMemcpy(s->edges, e, sizeof(e), hipMemcpyHostToDevice));
    }
    GP_TRY(get(&s->out, cells > tb ? cells : tb));
    GP_TRY(get(&s->part, (size_t)SUM_TOTAL_BLOCKS * 4));
    GP_TRY(get(&s->tot, GPIRT_SUM_NTOTALS));
    // the clears above are the null stream's, which is not ordered against a hipStreamNonBlocking stream (the handle
    // gpirt_mcmc makes for itself): drained here, or the first kernel that writes s->out on such a stream can have its
    // last blocks cleared under it (seen once: the tail of the pooled lppd read back as zeros)
    GP_HIP(hipStreamSynchronize(nullptr));
    return 0;
}

void summary_free(SummaryState* s)
{
    for (void* p : s->allocs) hipFree(p);
    *s = SummaryState{};
}

int launch_summary_accumulate(hipStream_t st, SummaryState* s, const double* theta, const double* beta, const double* f,
                              const double* mu, const double* y, const double* fstar)
{
    if ((((uintptr_t)f | (uintptr_t)mu | (uintptr_t)y) & 15) != 0) {
        set_error("summary: f, mu and y must be 16-byte aligned");
        return GPIRT_E_ARG;
    }
    if ((s->parts & GPIRT_SUM_IRF_BAND) && !fstar) {
        set_error("summary: GPIRT_SUM_IRF_BAND needs f*");
        return GPIRT_E_ARG;
    }
    const bool diag = s->parts & GPIRT_SUM_DIAG;
    if (diag && s->draws >= s->planned) {
        set_error("summary: all %lld planned draws are in (gpirt_sampler_summary_enable_planned)", (long long)s->planned);
        return GPIRT_E_ARG;
    }
    SumArgs a{};
    a.f = f; a.mu = mu; a.y = y; a.theta = theta; a.beta = beta;
    a.lse = s->lse; a.ll_mean = s->ll_mean; a.ll_m2 = s->ll_m2; a.p_sum = s->p_sum; a.f_mean = s->f_mean; a.f_m2 = s->f_m2;
    a.tb_mean = s->tb_mean; a.tb_m2 = s->tb_m2;
    a.cells = s->n * s->m; a.n = s->n; a.m = s->m;
    const int64_t draw = s->draws + 1;
    const bool w = s->parts & GPIRT_SUM_WAIC, p = s->parts & GPIRT_SUM_PRED, fo = s->parts & GPIRT_SUM_F;
    if (draw == 1 && s->y)       // the missing cells travel with the block (gpirt_chains_combine masks by them)
        GP_HIP(hipMemcpyAsync(s->y, y, sizeof(double) * (size_t)(s->n * s->m), hipMemcpyDeviceToDevice, st));
    if (diag) {
        const DiagArgs g = diag_step(s, draw);
        switch ((w ? 4 : 0) | (p ? 2 : 0) | (fo ? 1 : 0)) {
            case 0: launch_diag_acc<false, false, false>(st, a, g, draw); break;
            case 1: launch_diag_acc<false, false, true>(st, a, g, draw); break;
            case 2: launch_diag_acc<false, true, false>(st, a, g, draw); break;
            case 3: launch_diag_acc<false, true, true>(st, a, g, draw); break;
            case 4: launch_diag_acc<true, false, false>(st, a, g, draw); break;
            case 5: launch_diag_acc<true, false, true>(st, a, g, draw); break;
            case 6: launch_diag_acc<true, true, false>(st, a, g, draw); break;
            default: launch_diag_acc<true, true, true>(st, a, g, draw); break;
        }
        GP_HIP(hipGetLastError());
        GP_TRY(launch_hist(st, s, theta, fstar, draw));
        s->draws = draw;
        return 0;
    }
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
    GP_TRY(launch_hist(st, s, theta, fstar, draw));
    s->draws = draw;
    return 0;
}

int summary_seal(hipStream_t st, SummaryState* s, const double* irf_sum, int64_t N)
{
    int64_t hdr[SUM_HEADER_WORDS];
    hdr[0] = s->n; hdr[1] = s->m; hdr[2] = s->parts; hdr[3] = s->planned; hdr[4] = s->draws; hdr[5] = SUM_LAYOUT_VERSION;
    hdr[6] = N; hdr[7] = 0;
    GP_HIP(hipMemcpyAsync(s->block, hdr, SUM_HEADER_WORDS * sizeof(int64_t), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(s->irf, irf_sum, sizeof(double) * (size_t)(N * s->m), hipMemcpyDeviceToDevice, st));
    GP_HIP(hipStreamSynchronize(st));       // hdr is on this stack
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

int summary_hist_get(hipStream_t st, const SummaryState* s, const char* name, double* h_out, int64_t count, bool* found)
{
    const int64_t nh = s->n * NG, nm = (int64_t)NG * s->m;
    const struct { const char* k; const void* p; int64_t c; bool u32; } tab[] = {
        { "theta_hist", s->th_hist[0], nh, true }, { "theta_hist_h1", s->th_hist[1], nh, true },
        { "theta_hist_h2", s->th_hist[2], nh, true }, { "theta_off_grid", s->th_off, s->n, true },
        { "irf_p_mean", s->psum, nm, false }, { "irf_band", s->band, nm * GPIRT_IRF_BINS, true },
        { "irf_nan", s->band_nan, nm, true },
    };
    *found = false;
    for (const auto& e : tab) {
        if (strcmp(e.k, name) != 0) continue;
        *found = true;
        if (!e.p) {
            set_error("summary '%s' was not enabled (GPIRT_SUM_THETA_HIST, GPIRT_SUM_IRF_BAND; the halves need GPIRT_SUM_DIAG)", name);
            return GPIRT_E_ARG;
        }
        GP_ARG(count <= e.c);
        if (e.u32) {
            std::vector<uint32_t> tmp((size_t)count);
            GP_HIP(hipMemcpyAsync(tmp.data(), e.p, sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToHost, st));
            GP_HIP(hipStreamSynchronize(st));
            for (int64_t i = 0; i < count; ++i) h_out[i] = (double)tmp[(size_t)i];
        } else {                                  // the mean of plogis(f*) over the draws
            GP_HIP(hipMemcpyAsync(h_out, e.p, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, st));
            GP_HIP(hipStreamSynchronize(st));
            const double T = (double)s->draws;
            for (int64_t i = 0; i < count; ++i) h_out[i] = s->draws >= 1 ? h_out[i] / T : (double)NAN;
        }
        return 0;
    }
    return 0;
}

// ---- several chains: gpirt_chains_combine ----------------------------------------------------------------------------
namespace {

struct CombArgs {
    const double* const* st;          // C state blocks (SumLayout)
    const double* sgn;                // C signs: -1 reflects the chain's theta and beta slope means
    SumLayout L;
    int C, parts;
    int64_t n, tb, cells;
    double S, b, a, N;                // draws per chain, batch size and count, half length
    double *tb_mean, *tb_m2, *lse, *ll_mean, *ll_m2, *p_sum, *f_mean, *f_m2;    // the pooled accumulators (draws C S)
    double *rhat, *ess, *mcse;        // tb values, then (DIAG and F) the cells
};

// (mean, M2) of cnt draws += (mc, m2c) of S more: Chan et al.'s pairwise update, the first chain taken as it is
__device__ __forceinline__ void chan(double& mean, double& m2, double& cnt, double mc, double m2c, double S)
{
    if (cnt == 0.0) { mean = mc; m2 = m2c; cnt = S; return; }
    const double nn = cnt + S, delta = mc - mean;
    mean += delta * (S / nn);
    m2 += m2c + delta * delta * (cnt * S / nn);
    cnt = nn;
}

// split-R-hat, batch-means ESS and MCSE of one value (include/gpirt_hip.h GPIRT_SUM_DIAG), chains in order
__device__ __forceinline__ void diag_of(const CombArgs& a, const int64_t* off, int64_t m2off, int64_t i, bool flip, double& rhat,
                                        double& ess, double& mcse)
{
    double hc = 0.0, hmean = 0.0, hss = 0.0, w = 0.0, lam = 0.0, sig = 0.0;
    for (int c = 0; c < a.C; ++c) {
        const double* base = a.st[c];
        const double sg = flip ? a.sgn[c] : 1.0;
        hc += 1.0; welford(hmean, hss, sg * base[off[DG_H1_MEAN] + i], hc);
        hc += 1.0; welford(hmean, hss, sg * base[off[DG_H2_MEAN] + i], hc);
        w += base[off[DG_H1_M2] + i] / (a.N - 1.0) + base[off[DG_H2_M2] + i] / (a.N - 1.0);
        lam += base[m2off + i] / (a.S - 1.0);
        sig += base[off[DG_BM_M2] + i] * (a.b / (a.a - 1.0));
    }
    const double M = 2.0 * a.C, B = a.N / (M - 1.0) * hss, W = w / M;
    const double varp = (a.N - 1.0) / a.N * W + B / a.N;
    if (a.S < 4.0) rhat = (double)NAN;
    else if (W > 0.0) rhat = sqrt(varp / W);
    else rhat = B > 0.0 ? (double)INFINITY : (double)NAN;
    if (a.a < 2.0 || a.S < 2.0) { ess = (double)NAN; mcse = (double)NAN; return; }
    const double CS = a.C * a.S, lm = lam / a.C, sm = sig / a.C;
    ess = CS * lm / sm;
    mcse = sqrt(sm / CS);
}

template <bool DIAG>
__global__ __launch_bounds__(SUM_THREADS) void chains_combine_kernel(CombArgs a)
{
    const bool anycell = a.parts & (GPIRT_SUM_WAIC | GPIRT_SUM_PRED | GPIRT_SUM_F);
    const int64_t total = a.tb + (anycell ? a.cells : 0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < a.tb) {
            const bool flip = i < a.n || ((i - a.n) & 1);          // theta, and row 1 (the slope) of the 2 x m beta
            double mean = 0.0, m2 = 0.0, cnt = 0.0;
            for (int c = 0; c < a.C; ++c) {
                const double* base = a.st[c];
                chan(mean, m2, cnt, (flip ? a.sgn[c] : 1.0) * base[a.L.tb_mean + i], base[a.L.tb_m2 + i], a.S);
            }
            a.tb_mean[i] = mean; a.tb_m2[i] = m2;
            if (DIAG) diag_of(a, a.L.dtb, a.L.tb_m2, i, flip, a.rhat[i], a.ess[i], a.mcse[i]);
            continue;
        }
        const int64_t q = i - a.tb;
        if (a.parts & GPIRT_SUM_WAIC) {
            double lse = 0.0, mean = 0.0, m2 = 0.0, cnt = 0.0;
            for (int c = 0; c < a.C; ++c) {
                const double* base = a.st[c];
                lse = logaddexp(lse, base[a.L.lse + q], c == 0);
                chan(mean, m2, cnt, base[a.L.ll_mean + q], base[a.L.ll_m2 + q], a.S);
            }
            a.lse[q] = lse; a.ll_mean[q] = mean; a.ll_m2[q] = m2;
        }
        if (a.parts & GPIRT_SUM_PRED) {
            double ps = 0.0;
            for (int c = 0; c < a.C; ++c) ps += a.st[c][a.L.p_sum + q];
            a.p_sum[q] = ps;
        }
        if (a.parts & GPIRT_SUM_F) {
            double mean = 0.0, m2 = 0.0, cnt = 0.0;
            for (int c = 0; c < a.C; ++c) chan(mean, m2, cnt, a.st[c][a.L.f_mean + q], a.st[c][a.L.f_m2 + q], a.S);
            a.f_mean[q] = mean; a.f_m2[q] = m2;
            if (DIAG) diag_of(a, a.L.df, a.L.f_m2, q, false, a.rhat[i], a.ess[i], a.mcse[i]);
        }
    }
}

// dots[c] = sum_i thetabar_c,i thetabar_0,i over the n theta means, one block per chain, in a fixed order
__global__ __launch_bounds__(SUM_THREADS) void chains_dot_kernel(const double* const* st, int64_t off, int64_t n,
                                                                  double* __restrict__ dots)
{
    __shared__ double sh[1][SUM_THREADS];
    const double* x = st[blockIdx.x] + off;
    const double* x0 = st[0] + off;
    double v[1] = { 0.0 };
    for (int64_t i = threadIdx.x; i < n; i += SUM_THREADS) v[0] += x[i] * x0[i];
    block_sum<1>(v, sh);
    if (threadIdx.x == 0) dots[blockIdx.x] = v[0];
}

// the summed IRF sums, a reflected chain's reversed along the grid (k -> N - 1 - k)
__global__ __launch_bounds__(SUM_THREADS) void chains_irf_kernel(const double* const* st, const double* __restrict__ sgn, int C,
                                                                  int64_t off, int64_t N, int64_t m, double* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N * m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = i % N, j = i / N;
        double v = 0.0;
        for (int c = 0; c < C; ++c) v += st[c][off + (sgn[c] < 0.0 ? (N - 1 - k) + j * N : i)];
        out[i] = v;
    }
}

constexpr int DG_SCAL_BLOCKS = 256;

// per-block scalars (GPIRT_DIAG_*) of a range of values: partials [max rhat, min ess, # rhat > 1.01, # NaN rhat, # NaN ess]
__global__ __launch_bounds__(SUM_THREADS) void diag_scalars_kernel(const double* __restrict__ rhat, const double* __restrict__ ess,
                                                                   int64_t count, int fold, double* __restrict__ part)
{
    __shared__ double sh[GPIRT_DIAG_NSCALARS][SUM_THREADS];
    double v[GPIRT_DIAG_NSCALARS] = { -(double)INFINITY, (double)INFINITY, 0.0, 0.0, 0.0 };
    if (fold) {                                           // one block: the partials of the first pass
        for (int64_t b = threadIdx.x; b < count; b += SUM_THREADS) {
            const double* p = part + b * GPIRT_DIAG_NSCALARS;
            v[0] = fmax(v[0], p[0]); v[1] = fmin(v[1], p[1]); v[2] += p[2]; v[3] += p[3]; v[4] += p[4];
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
            const double r = rhat[i], e = ess[i];
            if (r != r) v[3] += 1.0; else { v[0] = fmax(v[0], r); if (r > 1.01) v[2] += 1.0; }
            if (e != e) v[4] += 1.0; else v[1] = fmin(v[1], e);
        }
    }
    const int t = threadIdx.x;
    for (int k = 0; k < GPIRT_DIAG_NSCALARS; ++k) sh[k][t] = v[k];
    __syncthreads();
    for (int w = SUM_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
            sh[0][t] = fmax(sh[0][t], sh[0][t + w]);
            sh[1][t] = fmin(sh[1][t], sh[1][t + w]);
            for (int k = 2; k < GPIRT_DIAG_NSCALARS; ++k) sh[k][t] += sh[k][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        double* o = fold ? part + (int64_t)DG_SCAL_BLOCKS * GPIRT_DIAG_NSCALARS : part + (int64_t)blockIdx.x * GPIRT_DIAG_NSCALARS;
        for (int k = 0; k < GPIRT_DIAG_NSCALARS; ++k) o[k] = sh[k][0];
    }
}

// the pooled outputs of gpirt_summary: the checks of gpirt_mcmc_summary with the parts the states carry
int pooled_args_ok(const gpirt_summary* p, int have)
{
    const int parts = p->parts;
    GP_ARG((parts & ~(GPIRT_SUM_THETA_BETA | GPIRT_SUM_F | GPIRT_SUM_PRED | GPIRT_SUM_WAIC)) == 0 && p->reserved == 0);
    GP_ARG((parts & ~have) == 0);
    GP_ARG(!((p->h_p_yes) && !(parts & GPIRT_SUM_PRED)));
    GP_ARG(!((p->h_lppd || p->h_p_waic) && !(parts & GPIRT_SUM_WAIC)));
    GP_ARG(!((p->h_f_mean || p->h_f_var) && !(parts & GPIRT_SUM_F)));
    return 0;
}

struct DevFree {
    std::vector<void*> p;
    ~DevFree() { for (void* q : p) hipFree(q); }
};

constexpr int POOLED_PARTS = GPIRT_SUM_THETA_BETA | GPIRT_SUM_F | GPIRT_SUM_PRED | GPIRT_SUM_WAIC;
constexpr int STATE_PARTS = POOLED_PARTS | GPIRT_SUM_DIAG | GPIRT_SUM_THETA_HIST | GPIRT_SUM_IRF_BAND;

// the C headers of d_states (identical) into hd; checks that they are this library's
int read_headers(hipStream_t st, int C, const void* const* d_states, std::vector<int64_t>& hd)
{
    hd.assign((size_t)C * SUM_HEADER_WORDS, 0);
    for (int c = 0; c < C; ++c) {
        GP_ARG(d_states[c] && ((uintptr_t)d_states[c] & 15) == 0);
        GP_HIP(hipMemcpyAsync(&hd[(size_t)c * SUM_HEADER_WORDS], d_states[c], SUM_HEADER_WORDS * sizeof(int64_t),
                              hipMemcpyDeviceToHost, st));
    }
    GP_HIP(hipStreamSynchronize(st));
    const int64_t* h0 = hd.data();
    for (int c = 1; c < C; ++c)
        if (memcmp(h0, &hd[(size_t)c * SUM_HEADER_WORDS], SUM_HEADER_WORDS * sizeof(int64_t)) != 0) {
            set_error("chain %d's state header (n, m, parts, planned draws, draws, layout) differs from chain 0's", c);
            return GPIRT_E_ARG;
        }
    if (h0[5] != SUM_LAYOUT_VERSION || h0[6] != GPIRT_NGRID || h0[0] <= 0 || h0[1] <= 0 || h0[4] < 0 ||
        (h0[2] & ~(int64_t)STATE_PARTS) != 0 || !(h0[2] & GPIRT_SUM_THETA_BETA)) {
        set_error("not a summary state block of this library (layout %lld)", (long long)h0[5]);
        return GPIRT_E_ARG;
    }
    return 0;
}

// The chains' signs, gpirt_chains_combine's decision: forced, or chain c >= 1 reflected when sum_i thetabar_c,i thetabar_0,i
// < 0 (align); sg holds C ones on entry.  d_st: the C block pointers on the device, d_dot C doubles of workspace.
int chain_signs(hipStream_t st, int C, const double* const* d_st, int64_t tb_mean, int64_t n, const int* signs, int align,
                double* d_dot, std::vector<double>& sg)
{
    if (signs) {
        for (int c = 0; c < C; ++c) {
            GP_ARG(signs[c] == 1 || signs[c] == -1);
            sg[(size_t)c] = (double)signs[c];
        }
    } else if (align && C > 1) {
        hipLaunchKernelGGL(chains_dot_kernel, dim3(C), dim3(SUM_THREADS), 0, st, d_st, tb_mean, n, d_dot);
        GP_HIP(hipGetLastError());
        std::vector<double> dots((size_t)C);
        GP_HIP(hipMemcpyAsync(dots.data(), d_dot, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        for (int c = 1; c < C; ++c) sg[(size_t)c] = dots[(size_t)c] < 0.0 ? -1.0 : 1.0;
    }
    return 0;
}

}  // namespace

int chains_combine(gpirt_handle_t h, int C, const void* const* d_states, const int* signs, int align, double* h_irfs,
                   gpirt_summary* pooled, gpirt_diag* diag, int* signs_out)
{
    GP_ARG(h && C >= 1 && d_states);
    hipStream_t st = h->stream;
    std::vector<int64_t> hd;
    GP_TRY(read_headers(st, C, d_states, hd));       // states with THETA_HIST / IRF_BAND too: their arrays come last
    const int64_t* h0 = hd.data();
    const int64_t n = h0[0], m = h0[1], planned = h0[3], draws = h0[4];
    const int parts = (int)h0[2];
    const bool dg = parts & GPIRT_SUM_DIAG, fo = parts & GPIRT_SUM_F;
    if (dg && draws != planned) {
        set_error("diagnostics need all %lld planned draws (%lld are in)", (long long)planned, (long long)draws);
        return GPIRT_E_ARG;
    }
    if (pooled) GP_TRY(pooled_args_ok(pooled, parts & POOLED_PARTS));
    if (diag) {
        GP_ARG(dg);
        GP_ARG(diag->reserved[0] == 0 && diag->reserved[1] == 0 && diag->reserved[2] == 0 && diag->reserved[3] == 0);
        GP_ARG(fo || !(diag->h_f_rhat || diag->h_f_ess || diag->h_f_mcse));
    }
    const SumLayout L = summary_layout(n, m, parts);
    const int64_t cells = n * m, tb = n + 2 * m, N = GPIRT_NGRID;
    std::vector<double> sg((size_t)C, 1.0);
    DevFree tmp;
    double* d_ptrs = nullptr;                    // C block pointers, C signs, C dots
    GP_HIP(hipMalloc(&d_ptrs, sizeof(double) * 3 * (size_t)C));
    tmp.p.push_back(d_ptrs);
    const double* const* d_st = reinterpret_cast<const double* const*>(d_ptrs);
    double* d_sg = d_ptrs + C;
    double* d_dot = d_ptrs + 2 * C;
    GP_HIP(hipMemcpyAsync(d_ptrs, d_states, sizeof(void*) * (size_t)C, hipMemcpyHostToDevice, st));
    GP_TRY(chain_signs(st, C, d_st, L.tb_mean, n, signs, align, d_dot, sg));
    if (signs_out)
        for (int c = 0; c < C; ++c) signs_out[c] = sg[(size_t)c] < 0.0 ? -1 : 1;
    GP_HIP(hipMemcpyAsync(d_sg, sg.data(), sizeof(double) * (size_t)C, hipMemcpyHostToDevice, st));

    SummaryState P;                              // the pooled accumulators: a chain of C S draws
    struct Free { SummaryState* s; ~Free() { summary_free(s); } } pfree{ &P };
    GP_TRY(summary_alloc(&P, n, m, parts & POOLED_PARTS));
    P.draws = (int64_t)C * draws;
    const int64_t nd = dg ? tb + (fo ? cells : 0) : 0;
    double* d_diag = nullptr;
    if (dg) {
        GP_HIP(hipMalloc(&d_diag, sizeof(double) * (size_t)(3 * nd + (DG_SCAL_BLOCKS + 1) * GPIRT_DIAG_NSCALARS)));
        tmp.p.push_back(d_diag);
    }
    CombArgs a{};
    a.st = d_st; a.sgn = d_sg; a.L = L; a.C = C; a.parts = parts; a.n = n; a.tb = tb; a.cells = cells;
    const int64_t S = dg ? planned : draws, b = dg ? isqrt(planned) : 1;
    a.S = (double)S; a.b = (double)b; a.a = (double)(S / b); a.N = (double)(S / 2);
    a.tb_mean = P.tb_mean; a.tb_m2 = P.tb_m2; a.lse = P.lse; a.ll_mean = P.ll_mean; a.ll_m2 = P.ll_m2; a.p_sum = P.p_sum;
    a.f_mean = P.f_mean; a.f_m2 = P.f_m2;
    if (dg) { a.rhat = d_diag; a.ess = d_diag + nd; a.mcse = d_diag + 2 * nd; }
    const bool anycell = parts & (GPIRT_SUM_WAIC | GPIRT_SUM_PRED | GPIRT_SUM_F);
    const int64_t work = tb + (anycell ? cells : 0);
    if (dg) hipLaunchKernelGGL(chains_combine_kernel<true>, dim3(grid_cap(work)), dim3(SUM_THREADS), 0, st, a);
    else hipLaunchKernelGGL(chains_combine_kernel<false>, dim3(grid_cap(work)), dim3(SUM_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());

    const double* y0 = L.y >= 0 ? static_cast<const double*>(d_states[0]) + L.y : nullptr;
    auto fetch = [&](const char* name, double* h_out) -> int {
        if (!h_out) return 0;
        double* d = nullptr; int64_t cnt = 0;
        GP_TRY(launch_summary_finish(st, &P, name, y0, &d, &cnt));
        GP_HIP(hipMemcpyAsync(h_out, d, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));          // P.out is reused by the next array
        return 0;
    };
    if (pooled) {
        for (int k = 0; k < GPIRT_SUM_NTOTALS; ++k) pooled->totals[k] = (double)NAN;
        pooled->totals[GPIRT_SUM_T_DRAWS] = (double)P.draws;
        GP_TRY(fetch("p_yes", pooled->h_p_yes)); GP_TRY(fetch("lppd", pooled->h_lppd)); GP_TRY(fetch("p_waic", pooled->h_p_waic));
        GP_TRY(fetch("f_mean", pooled->h_f_mean)); GP_TRY(fetch("f_var", pooled->h_f_var));
        GP_TRY(fetch("theta_mean", pooled->h_theta_mean)); GP_TRY(fetch("theta_var", pooled->h_theta_var));
        GP_TRY(fetch("beta_mean", pooled->h_beta_mean)); GP_TRY(fetch("beta_var", pooled->h_beta_var));
        if (pooled->parts & GPIRT_SUM_WAIC) {
            GP_TRY(launch_summary_totals(st, &P, y0));
            GP_HIP(hipMemcpyAsync(pooled->totals, P.tot, sizeof(double) * GPIRT_SUM_NTOTALS, hipMemcpyDeviceToHost, st));
        }
    }
    if (diag) {
        const struct { double* p; int64_t at, cnt; } outs[] = {
            { diag->h_theta_rhat, 0, n }, { diag->h_theta_ess, nd, n }, { diag->h_theta_mcse, 2 * nd, n },
            { diag->h_beta_rhat, n, 2 * m }, { diag->h_beta_ess, nd + n, 2 * m }, { diag->h_beta_mcse, 2 * nd + n, 2 * m },
            { diag->h_f_rhat, tb, cells }, { diag->h_f_ess, nd + tb, cells }, { diag->h_f_mcse, 2 * nd + tb, cells },
        };
        for (const auto& o : outs)
            if (o.p) GP_HIP(hipMemcpyAsync(o.p, d_diag + o.at, sizeof(double) * (size_t)o.cnt, hipMemcpyDeviceToHost, st));
        double* part = d_diag + 3 * nd;
        const int64_t range[GPIRT_DIAG_NBLOCKS][2] = { { 0, n }, { n, 2 * m }, { tb, fo ? cells : 0 } };
        for (int blk = 0; blk < GPIRT_DIAG_NBLOCKS; ++blk) {
            double* sc = diag->scalars[blk];
            const int64_t cnt = range[blk][1];
            if (cnt == 0) {
                sc[GPIRT_DIAG_MAX_RHAT] = sc[GPIRT_DIAG_MIN_ESS] = (double)NAN;
                sc[GPIRT_DIAG_N_RHAT_HIGH] = sc[GPIRT_DIAG_N_RHAT_NAN] = sc[GPIRT_DIAG_N_ESS_NAN] = 0.0;
                continue;
            }
            const double* r = d_diag + range[blk][0];
            hipLaunchKernelGGL(diag_scalars_kernel, dim3(DG_SCAL_BLOCKS), dim3(SUM_THREADS), 0, st, r, r + nd, cnt, 0, part);
            hipLaunchKernelGGL(diag_scalars_kernel, dim3(1), dim3(SUM_THREADS), 0, st, r, r + nd, (int64_t)DG_SCAL_BLOCKS, 1, part);
            GP_HIP(hipGetLastError());
            GP_HIP(hipMemcpyAsync(sc, part + (int64_t)DG_SCAL_BLOCKS * GPIRT_DIAG_NSCALARS, sizeof(double) * GPIRT_DIAG_NSCALARS,
                                  hipMemcpyDeviceToHost, st));
            GP_HIP(hipStreamSynchronize(st));
            if (sc[GPIRT_DIAG_N_RHAT_NAN] == (double)cnt) sc[GPIRT_DIAG_MAX_RHAT] = (double)NAN;
            if (sc[GPIRT_DIAG_N_ESS_NAN] == (double)cnt) sc[GPIRT_DIAG_MIN_ESS] = (double)NAN;
        }
        if (diag->reflected)
            for (int c = 0; c < C; ++c) diag->reflected[c] = sg[(size_t)c] < 0.0 ? 1 : 0;
    }
    if (h_irfs) {
        double* d_irf = nullptr;                 // N x m: more than P.out holds when n < N
        GP_HIP(hipMalloc(&d_irf, sizeof(double) * (size_t)(N * m)));
        tmp.p.push_back(d_irf);
        hipLaunchKernelGGL(chains_irf_kernel, dim3(grid_cap(N * m)), dim3(SUM_THREADS), 0, st, d_st, d_sg, C, L.irf, N, m, d_irf);
        GP_HIP(hipGetLastError());
        GP_HIP(hipMemcpyAsync(h_irfs, d_irf, sizeof(double) * (size_t)(N * m), hipMemcpyDeviceToHost, st));
    }
    GP_HIP(hipStreamSynchronize(st));
    if (h_irfs) {
        const double inv = 1.0 / ((double)C * (double)S);
        for (int64_t i = 0; i < N * m; ++i) h_irfs[i] = 1.0 / (1.0 + exp(-(h_irfs[i] * inv)));
    }
    return 0;
}

// ---- quantiles: gpirt_summary_quantiles ------------------------------------------------------------------------------
namespace {

struct QArgs {
    const double* const* st;          // C state blocks
    const double* sgn;                // C signs: -1 reverses the chain's grid index (k -> NG - 1 - k)
    QntLayout Q;
    int C, nprobs;
    int64_t n, nm, T, hN;             // pooled draws C S, half length floor(S / 2)
    const int64_t* rank;              // nprobs + 1: max(ceil(q T), 1) of each prob, then the median's
    const double* tq;                 // nprobs: q T
    const int64_t* order;             // nprobs: the probabilities' indices in ascending order of q T
    double *theta_q, *median, *mode, *hist, *bulk, *tail, *rhat, *off;     // device, nullptr: not wanted
    double *irf_q, *p_mean, *part;
};

constexpr int QPER = (NG + SUM_THREADS - 1) / SUM_THREADS;     // grid points a lane scans, contiguous

__device__ __forceinline__ uint32_t th_count(const QArgs& a, int c, int64_t off, int64_t i, int k)
{
    const uint32_t* h = reinterpret_cast<const uint32_t*>(a.st[c] + off) + i * NG;
    return h[a.sgn[c] < 0.0 ? NG - 1 - k : k];
}

// Half (c, off)'s count at index t of the ranked variable: grid point t (s2 < 0), or the folded distance d = 2t + (s2 & 1)
// from the median s2 / 2 in half-grid units -- grid points (s2 + d) / 2 and (s2 - d) / 2, one point at d = 0
__device__ __forceinline__ long long split_count(const QArgs& a, int c, int64_t off, int64_t i, int t, int s2)
{
    if (s2 < 0) return th_count(a, c, off, i, t);
    const int kp = (s2 + 1) / 2 + t, km = s2 / 2 - t;
    long long v = kp < NG ? (long long)th_count(a, c, off, i, kp) : 0;
    if (km >= 0 && km != kp) v += th_count(a, c, off, i, km);
    return v;
}

// cum[k] = v[0] + ... + v[k] over the NG entries (LDS): each lane sums QPER contiguous entries, a Hillis-Steele scan of
// the lane sums, then the lane's entries; every lane returns with cum complete
__device__ __forceinline__ void scan_counts(const long long* v, long long* cum, long long* sh)
{
    const int t = threadIdx.x, k0 = t * QPER;
    long long run = 0;
    for (int u = 0; u < QPER; ++u)
        if (k0 + u < NG) run += v[k0 + u];
    sh[t] = run;
    __syncthreads();
    for (int w = 1; w < SUM_THREADS; w <<= 1) {
        const long long add = t >= w ? sh[t - w] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    long long base = t ? sh[t - 1] : 0;
    for (int u = 0; u < QPER; ++u)
        if (k0 + u < NG) { base += v[k0 + u]; cum[k0 + u] = base; }
    __syncthreads();
}

// the block's sum of x in a fixed order (block_sum's tree), in every lane
__device__ __forceinline__ double block_total(double x, double (*sh)[SUM_THREADS])
{
    const int t = threadIdx.x;
    sh[0][t] = x;
    __syncthreads();
    for (int w = SUM_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) sh[0][t] += sh[0][t + w];
        __syncthreads();
    }
    const double v = sh[0][0];
    __syncthreads();                  // sh is written again by the next sum
    return v;
}

// Rank-normalised split-R-hat of respondent i from the 2C halves' counts (s2 < 0: bulk; else the tail, folded about
// s2 / 2): ranks with ties averaged over the T' split draws, r = cum_(t-1) + (count_t + 1) / 2, z = Phi^-1((r - 3/8) /
// (T' + 1/4)); each half's mean and variance (ddof 1) from its counts, streamed from the blocks; the BDA3 formula of
// diag_of with its W = 0 rules.
__device__ __forceinline__ double rank_rhat(const QArgs& a, int64_t i, int s2, long long* sc, long long* cum, double* z, long long* shl,
                            double (*shd)[SUM_THREADS])
{
    for (int t = threadIdx.x; t < NG; t += SUM_THREADS) {
        long long v = 0;
        for (int c = 0; c < a.C; ++c) v += split_count(a, c, a.Q.th_hist[1], i, t, s2) + split_count(a, c, a.Q.th_hist[2], i, t, s2);
        sc[t] = v;
    }
    __syncthreads();
    scan_counts(sc, cum, shl);
    const double Tp = (double)(2 * a.C * a.hN);
    for (int t = threadIdx.x; t < NG; t += SUM_THREADS) {
        const double r = (double)(cum[t] - sc[t]) + ((double)sc[t] + 1.0) * 0.5;
        z[t] = sc[t] ? normcdfinv((r - 0.375) / (Tp + 0.25)) : 0.0;
    }
    __syncthreads();
    const double N = (double)a.hN;
    double hc = 0.0, hmean = 0.0, hss = 0.0, w = 0.0;
    for (int c = 0; c < a.C; ++c)
        for (int h = 1; h <= 2; ++h) {
            const int64_t off = a.Q.th_hist[h];
            double s = 0.0;
            for (int t = threadIdx.x; t < NG; t += SUM_THREADS) s += (double)split_count(a, c, off, i, t, s2) * z[t];
            const double mean = block_total(s, shd) / N;
            double q = 0.0;
            for (int t = threadIdx.x; t < NG; t += SUM_THREADS) {
                const double d = z[t] - mean;
                q += (double)split_count(a, c, off, i, t, s2) * d * d;
            }
            w += block_total(q, shd) / (N - 1.0);
            hc += 1.0; welford(hmean, hss, mean, hc);
        }
    if (a.hN < 2) return (double)NAN;                      // S < 4
    const double M = 2.0 * a.C, B = N / (M - 1.0) * hss, W = w / M;
    const double varp = (N - 1.0) / N * W + B / N;
    if (W > 0.0) return sqrt(varp / W);
    return B > 0.0 ? (double)INFINITY : (double)NAN;
}

// One work-group per respondent: the pooled counts, their quantiles, median, mode and (with the halves) the bulk and tail
// R-hat.  LDS: the pooled and split counts, their prefix sums and the scores, about 45 KB; the 2C halves stream from the
// blocks, so C does not bound it.
__global__ __launch_bounds__(SUM_THREADS) void quantile_theta_kernel(QArgs a)
{
    __shared__ long long cnt[NG], cum[NG], sc[NG], scum[NG], shl[SUM_THREADS];
    __shared__ double z[NG], shd[1][SUM_THREADS];
    __shared__ int shk[SUM_THREADS], kq[2];
    const int64_t i = blockIdx.x;
    const int t = threadIdx.x;
    for (int k = t; k < NG; k += SUM_THREADS) {
        long long v = 0;
        for (int c = 0; c < a.C; ++c) v += th_count(a, c, a.Q.th_hist[0], i, k);
        cnt[k] = v;
        if (a.hist) a.hist[i * NG + k] = (double)v;
    }
    double offc = 0.0;
    for (int c = 0; c < a.C; ++c) offc += (double)reinterpret_cast<const uint32_t*>(a.st[c] + a.Q.th_off)[i];
    if (t == 0) a.off[i] = offc;
    if (offc > 0.0) {                                       // a draw off the grid: no quantity of this respondent is exact
        for (int p = t; p < a.nprobs; p += SUM_THREADS)
            if (a.theta_q) a.theta_q[p + (int64_t)a.nprobs * i] = (double)NAN;
        if (t == 0) {
            if (a.median) a.median[i] = (double)NAN;
            if (a.mode) a.mode[i] = (double)NAN;
            if (a.rhat) { a.rhat[i] = (double)NAN; if (a.bulk) a.bulk[i] = (double)NAN; if (a.tail) a.tail[i] = (double)NAN; }
        }
        return;
    }
    __syncthreads();
    scan_counts(cnt, cum, shl);
    // order statistics: grid point k holds ranks cum_(k-1) + 1 .. cum_k
    const int64_t rlo = (a.T + 1) / 2, rhi = a.T / 2 + 1;   // R's median: the two middle order statistics
    long long best = -1;
    int bk = 0;
    for (int k = t; k < NG; k += SUM_THREADS) {
        const long long lo = k ? cum[k - 1] : 0, hi = cum[k];
        if (cnt[k] > best) { best = cnt[k]; bk = k; }
        if (lo == hi) continue;
        const double v = -5.0 + (double)k * 0.01;
        if (a.theta_q)
            for (int p = 0; p < a.nprobs; ++p)
                if (lo < a.rank[p] && a.rank[p] <= hi) a.theta_q[p + (int64_t)a.nprobs * i] = v;
        if (a.median && lo < a.rank[a.nprobs] && a.rank[a.nprobs] <= hi) a.median[i] = v;
        if (lo < rlo && rlo <= hi) kq[0] = k;
        if (lo < rhi && rhi <= hi) kq[1] = k;
    }
    shl[t] = best; shk[t] = bk;                             // the mode: the largest count, the lowest grid point on a tie
    __syncthreads();
    for (int w = SUM_THREADS / 2; w > 0; w >>= 1) {
        if (t < w && (shl[t + w] > shl[t] || (shl[t + w] == shl[t] && shk[t + w] < shk[t]))) { shl[t] = shl[t + w]; shk[t] = shk[t + w]; }
        __syncthreads();
    }
    if (t == 0 && a.mode) a.mode[i] = -5.0 + (double)shk[0] * 0.01;
    __syncthreads();
    if (!a.rhat) return;
    const double bulk = rank_rhat(a, i, -1, sc, scum, z, shl, shd);
    const double tail = rank_rhat(a, i, kq[0] + kq[1], sc, scum, z, shl, shd);
    if (t == 0) {
        if (a.bulk) a.bulk[i] = bulk;
        if (a.tail) a.tail[i] = tail;
        a.rhat[i] = (bulk != bulk || tail != tail) ? (double)NAN : fmax(bulk, tail);
    }
}

// the block's min (mx = false) or max of x, in every lane
__device__ __forceinline__ double block_extreme(double x, bool mx, double (*sh)[SUM_THREADS])
{
    const int t = threadIdx.x;
    sh[0][t] = x;
    __syncthreads();
    for (int w = SUM_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) sh[0][t] = mx ? fmax(sh[0][t], sh[0][t + w]) : fmin(sh[0][t], sh[0][t + w]);
        __syncthreads();
    }
    const double v = sh[0][0];
    __syncthreads();
    return v;
}

// One lane per f* cell: E[P], then ONE pass over the pooled band (a reflected chain's cell read at the mirrored grid
// point), each bin of each chain read once, that resolves the probabilities in ascending order of q T (a.order) -- the
// first bin with a draw whose cumulative count reaches t -- and counts the cell's draws.  Block partials: the NaN draws,
// the least and the most draws of a cell (bins + NaN).
__global__ __launch_bounds__(SUM_THREADS) void quantile_irf_kernel(QArgs a)
{
    __shared__ double sh[1][SUM_THREADS];
    double nan_all = 0.0, cnt_min = (double)INFINITY, cnt_max = -(double)INFINITY;
    const double T = (double)a.T;
    for (int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; cell < a.nm; cell += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = cell % NG, mirror = cell - k + (NG - 1 - k);
        double nanc = 0.0, ps = 0.0;
        for (int c = 0; c < a.C; ++c) {
            const int64_t src = a.sgn[c] < 0.0 ? mirror : cell;
            nanc += (double)reinterpret_cast<const uint32_t*>(a.st[c] + a.Q.band_nan)[src];
            ps += a.st[c][a.Q.psum + src];
        }
        nan_all += nanc;
        if (a.p_mean) a.p_mean[cell] = ps / T;
        int pi = 0;                                          // the next probability, in ascending order of q T
        double cum = 0.0;
        for (int b = 0; b < GPIRT_IRF_BINS; ++b) {
            double cb = 0.0;
            for (int c = 0; c < a.C; ++c)
                cb += (double)reinterpret_cast<const uint32_t*>(a.st[c] + a.Q.band)[(int64_t)b * a.nm + (a.sgn[c] < 0.0 ? mirror : cell)];
            if (cb > 0.0)
                for (; pi < a.nprobs && cum + cb >= a.tq[a.order[pi]]; ++pi) {
                    const int64_t p = a.order[pi];
                    if (a.irf_q)
                        a.irf_q[p + (int64_t)a.nprobs * cell] =
                            nanc == 0.0 ? ((double)b + (a.tq[p] - cum) / cb) / (double)GPIRT_IRF_BINS : (double)NAN;
                }
            cum += cb;
        }
        for (; pi < a.nprobs; ++pi)
            if (a.irf_q) a.irf_q[a.order[pi] + (int64_t)a.nprobs * cell] = (double)NAN;
        cnt_min = fmin(cnt_min, cum + nanc);
        cnt_max = fmax(cnt_max, cum + nanc);
    }
    const double v0 = block_total(nan_all, sh), v1 = block_extreme(cnt_min, false, sh), v2 = block_extreme(cnt_max, true, sh);
    if (threadIdx.x == 0) { a.part[3 * (int64_t)blockIdx.x] = v0; a.part[3 * (int64_t)blockIdx.x + 1] = v1; a.part[3 * (int64_t)blockIdx.x + 2] = v2; }
}

}  // namespace

int summary_quantiles(gpirt_handle_t h, int C, const void* const* d_states, const int* signs, int align, gpirt_quantiles* q)
{
    GP_ARG(h && C >= 1 && d_states && q);
    GP_ARG(q->reserved0 == 0 && q->reserved[0] == 0 && q->reserved[1] == 0 && q->reserved[2] == 0 && q->reserved[3] == 0);
    GP_ARG(q->nprobs >= 0 && (q->nprobs == 0 || q->probs));
    for (int p = 0; p < q->nprobs; ++p) GP_ARG(q->probs[p] >= 0.0 && q->probs[p] <= 1.0);
    hipStream_t st = h->stream;
    std::vector<int64_t> hd;
    GP_TRY(read_headers(st, C, d_states, hd));
    const int64_t n = hd[0], m = hd[1], planned = hd[3], draws = hd[4];
    const int parts = (int)hd[2];
    const bool th = parts & GPIRT_SUM_THETA_HIST, band = parts & GPIRT_SUM_IRF_BAND, dg = parts & GPIRT_SUM_DIAG;
    const bool rh = th && dg;
    GP_ARG(th || !(q->theta_q || q->theta_median || q->theta_mode || q->theta_hist));
    GP_ARG(rh || !(q->theta_rhat_bulk || q->theta_rhat_tail || q->theta_rhat));
    GP_ARG(band || !(q->irf_q || q->irf_p_mean));
    if (dg && draws != planned) {
        set_error("the R-hat needs all %lld planned draws (%lld are in)", (long long)planned, (long long)draws);
        return GPIRT_E_ARG;
    }
    if (draws < 1) { set_error("quantiles need draws (the states hold none)"); return GPIRT_E_ARG; }
    const int64_t T = (int64_t)C * draws;
    if (T >= ((int64_t)1 << 32)) { set_error("C S = %lld draws: the pooled counts are limited to 2^32", (long long)T); return GPIRT_E_ARG; }
    const SumLayout L = summary_layout(n, m, parts);
    const QntLayout Q = quantile_layout(n, m, parts);
    const int64_t nm = (int64_t)NG * m, np = q->nprobs;

    DevFree tmp;
    auto dalloc = [&](double** p, int64_t count) -> int {
        GP_HIP(hipMalloc(p, sizeof(double) * (size_t)(count < 1 ? 1 : count)));
        tmp.p.push_back(*p);
        return 0;
    };
    double* d_ptrs = nullptr;                    // C block pointers, C signs, C dots
    GP_TRY(dalloc(&d_ptrs, 3 * (int64_t)C));
    const double* const* d_st = reinterpret_cast<const double* const*>(d_ptrs);
    GP_HIP(hipMemcpyAsync(d_ptrs, d_states, sizeof(void*) * (size_t)C, hipMemcpyHostToDevice, st));
    std::vector<double> sg((size_t)C, 1.0);
    GP_TRY(chain_signs(st, C, d_st, L.tb_mean, n, signs, align, d_ptrs + 2 * C, sg));
    GP_HIP(hipMemcpyAsync(d_ptrs + C, sg.data(), sizeof(double) * (size_t)C, hipMemcpyHostToDevice, st));

    std::vector<int64_t> rk((size_t)np + 1);     // max(ceil(q T), 1), then the median's; q T
    std::vector<double> tq((size_t)np + 1, 0.0);
    for (int64_t p = 0; p <= np; ++p) {
        const double qq = p < np ? q->probs[p] : 0.5;
        const int64_t r = (int64_t)ceil(qq * (double)T);
        rk[(size_t)p] = r < 1 ? 1 : r;
        tq[(size_t)p] = qq * (double)T;
    }
    std::vector<int64_t> order((size_t)np + 1);
    for (int64_t p = 0; p <= np; ++p) order[(size_t)p] = p;
    std::stable_sort(order.begin(), order.begin() + np, [&](int64_t x, int64_t y) { return tq[(size_t)x] < tq[(size_t)y]; });
    double *d_rk = nullptr, *d_tq = nullptr, *d_order = nullptr;
    GP_TRY(dalloc(&d_rk, np + 1)); GP_TRY(dalloc(&d_tq, np + 1)); GP_TRY(dalloc(&d_order, np + 1));
    GP_HIP(hipMemcpyAsync(d_rk, rk.data(), sizeof(int64_t) * (size_t)(np + 1), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(d_tq, tq.data(), sizeof(double) * (size_t)(np + 1), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(d_order, order.data(), sizeof(int64_t) * (size_t)(np + 1), hipMemcpyHostToDevice, st));

    QArgs a{};
    a.st = d_st; a.sgn = d_ptrs + C; a.Q = Q; a.C = C; a.nprobs = (int)np;
    a.n = n; a.nm = nm; a.T = T; a.hN = planned / 2;
    a.rank = reinterpret_cast<const int64_t*>(d_rk); a.tq = d_tq; a.order = reinterpret_cast<const int64_t*>(d_order);
    struct Out { double* host; double** dev; int64_t count; };
    std::vector<Out> outs;
    auto want = [&](double* host, double** dev, int64_t count, bool always) -> int {
        if (!host && !always) return 0;
        GP_TRY(dalloc(dev, count));
        if (host) outs.push_back({ host, dev, count });
        return 0;
    };
    std::vector<double> off_h, rhat_h, part_h;
    if (th) {
        GP_TRY(want(np ? q->theta_q : nullptr, &a.theta_q, np * n, false));
        GP_TRY(want(q->theta_median, &a.median, n, false));
        GP_TRY(want(q->theta_mode, &a.mode, n, false));
        GP_TRY(want(q->theta_hist, &a.hist, NG * n, false));
        off_h.resize((size_t)n);
        GP_TRY(want(off_h.data(), &a.off, n, true));
        if (rh) {
            GP_TRY(want(q->theta_rhat_bulk, &a.bulk, n, false));
            GP_TRY(want(q->theta_rhat_tail, &a.tail, n, false));
            rhat_h.resize((size_t)n);
            GP_TRY(want(rhat_h.data(), &a.rhat, n, true));
        }
        hipLaunchKernelGGL(quantile_theta_kernel, dim3((unsigned)n), dim3(SUM_THREADS), 0, st, a);
        GP_HIP(hipGetLastError());
    }
    if (band) {
        GP_TRY(want(np ? q->irf_q : nullptr, &a.irf_q, np * nm, false));
        GP_TRY(want(q->irf_p_mean, &a.p_mean, nm, false));
        const int blocks = grid_cap(nm);
        part_h.resize(3 * (size_t)blocks);
        GP_TRY(want(part_h.data(), &a.part, 3 * (int64_t)blocks, true));
        hipLaunchKernelGGL(quantile_irf_kernel, dim3(blocks), dim3(SUM_THREADS), 0, st, a);
        GP_HIP(hipGetLastError());
    }
    for (const Out& o : outs)
        GP_HIP(hipMemcpyAsync(o.host, *o.dev, sizeof(double) * (size_t)o.count, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));

    double* sc = q->scalars;
    sc[GPIRT_QNT_DRAWS] = (double)T;
    sc[GPIRT_QNT_MAX_RHAT] = (double)NAN;
    sc[GPIRT_QNT_N_RHAT_HIGH] = sc[GPIRT_QNT_N_RHAT_NAN] = 0.0;
    if (rh && q->theta_rhat) memcpy(q->theta_rhat, rhat_h.data(), sizeof(double) * (size_t)n);
    if (rh)
        for (double r : rhat_h) {
            if (r != r) { sc[GPIRT_QNT_N_RHAT_NAN] += 1.0; continue; }
            if (!(sc[GPIRT_QNT_MAX_RHAT] >= r)) sc[GPIRT_QNT_MAX_RHAT] = r;
            if (r > 1.01) sc[GPIRT_QNT_N_RHAT_HIGH] += 1.0;
        }
    double off = 0.0, nan = 0.0;
    for (double v : off_h) off += v;
    double cmin = band ? (double)INFINITY : (double)NAN, cmax = band ? -(double)INFINITY : (double)NAN;
    for (size_t b = 0; b < part_h.size(); b += 3) {
        nan += part_h[b];
        cmin = fmin(cmin, part_h[b + 1]);
        cmax = fmax(cmax, part_h[b + 2]);
    }
    sc[GPIRT_QNT_THETA_OFF_GRID] = th ? off : (double)NAN;
    sc[GPIRT_QNT_IRF_NAN] = band ? nan : (double)NAN;
    sc[GPIRT_QNT_IRF_COUNT_MIN] = cmin;
    sc[GPIRT_QNT_IRF_COUNT_MAX] = cmax;
    if (q->reflected)
        for (int c = 0; c < C; ++c) q->reflected[c] = sg[(size_t)c] < 0.0 ? 1 : 0;
    return 0;
}

}  // namespace gpirt
