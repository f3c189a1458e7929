// amp.hip -- per-item GP amplitudes (gpirt_sampler_amp_*, sampler.hip): item j's prior is f_j ~ N(0, a_j^2 (K + 0.001 I)), i.e.
// a_j times the unit model.  The kernels: the scaling of draw_f's prior draw nu_j = a_j L z_j, the one-launch update of every
// item's amplitude on a grid (a prior-whitened Metropolis step, Murray & Adams 2010, section 2.2: nu_j = L^-1 f_j / a_j is
// held fixed, a proposal moves f_j' = (a_k' / a_k) f_j and the likelihood decides), and the recorder of the indices.  Below them
// the argument check on the host.
//
// The log-likelihood term is ll_term_fast (ll_fast.h), a cell's contribution t(y (f + mu)) - t(y (f' + mu)) is formed as that
// difference of two terms, and the order of the additions is ell_delta_kernel's (ell.hip).
#include "common.h"
#include "kernels.h"
#include "ll_fast.h"

#include <cmath>

namespace gpirt {

namespace {

constexpr int AMP_THREADS = 256;

// nu_ij <- a_j nu_ij: one product per value, one writer each
__global__ __launch_bounds__(AMP_THREADS) void amp_scale_kernel(double* __restrict__ nu, const double* __restrict__ amp, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * AMP_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t j = blockIdx.y;
    nu[i + j * n] = amp[j] * nu[i + j * n];
}

// One work-group per item j.  Every thread forms the proposal from the item's two uniforms; thread t sums its rows
// i = t, t + 256, ... in ascending order, four loads in flight, then the fixed LDS tree; thread 0 decides; on accept the same
// work-group rewrites its column.  idx, amp, counts (4 x m: updates, accepted, out_of_range, failed) and rec (5 x m: dll,
// log_ratio, log_u, status, nonfinite; status 0 rejected, 1 accepted, 2 out of range, 3 failed) have this one writer per value.
__global__ __launch_bounds__(AMP_THREADS) void amp_update_kernel(AmpUpdateArgs a)
{
    __shared__ double sd[AMP_THREADS];
    __shared__ int sc[AMP_THREADS];
    __shared__ int s_accept;
    const int tid = threadIdx.x;
    const int64_t j = blockIdx.x, n = a.n;
    const double u0 = item_uniform(a.seed, a.t, GPIRT_ST_AMP, a.item0 + (uint32_t)j, 0),
                 u1 = item_uniform(a.seed, a.t, GPIRT_ST_AMP, a.item0 + (uint32_t)j, 1);
    const int k = a.idx[j], w = a.width[j];
    int q = (int)floor(u0 * (double)(2 * w));
    if (q > 2 * w - 1) q = 2 * w - 1;
    const int kp = k + (q < w ? q - w : q - w + 1);
    const int64_t m = a.m;
    long long* cnt = a.counts + j;                                            // (4 x m and 5 x m, row-major: stride m)
    double* rec = a.rec + j;
    if (kp < 0 || kp >= a.P) {                                                // (the proposal is symmetric: nothing else runs)
        if (tid == 0) {
            cnt[0] += 1; cnt[2 * m] += 1;
            rec[0] = __builtin_nan(""); rec[m] = __builtin_nan(""); rec[2 * m] = __builtin_nan(""); rec[3 * m] = 2.0; rec[4 * m] = 0.0;
        }
        return;
    }
    const double c = a.grid[kp] / a.grid[k];
    double* fj = a.f + j * n;
    const double* mj = a.mu + j * n;
    const double* yj = a.y + j * n;
    double acc = 0.0;
    int bad = 0;
    auto cell = [&](double fv, double mv, double yv) {
        const double pv = c * fv;
        if (!(fabs(pv) <= 1.79769313486231570815e308)) ++bad;             // NaN or infinite
        if (yv == yv) acc += ll_term_fast(yv * (fv + mv)) - ll_term_fast(yv * (pv + mv));
    };
    int64_t i = tid;
    for (; i + 3 * AMP_THREADS < n; i += 4 * AMP_THREADS) {               // four rows' loads in flight, added in row order
        const int64_t i1 = i + AMP_THREADS, i2 = i + 2 * AMP_THREADS, i3 = i + 3 * AMP_THREADS;
        const double f0 = fj[i], f1 = fj[i1], f2 = fj[i2], f3 = fj[i3];
        const double m0 = mj[i], m1 = mj[i1], m2 = mj[i2], m3 = mj[i3];
        const double y0 = yj[i], y1 = yj[i1], y2 = yj[i2], y3 = yj[i3];
        cell(f0, m0, y0); cell(f1, m1, y1); cell(f2, m2, y2); cell(f3, m3, y3);
    }
    for (; i < n; i += AMP_THREADS) cell(fj[i], mj[i], yj[i]);
    sd[tid] = acc; sc[tid] = bad;
    __syncthreads();
#pragma unroll
    for (int s = AMP_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) { sd[tid] += sd[tid + s]; sc[tid] += sc[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double dll = sd[0], log_u = log(u1);
        const double ratio = dll + (a.log_prior[kp] - a.log_prior[k]);
        const bool failed = sc[0] != 0 || !(fabs(dll) <= 1.79769313486231570815e308);
        const bool accept = !failed && log_u < ratio;
        rec[0] = dll; rec[m] = ratio; rec[2 * m] = log_u; rec[3 * m] = failed ? 3.0 : (accept ? 1.0 : 0.0); rec[4 * m] = (double)sc[0];
        cnt[0] += 1;
        if (accept) { cnt[m] += 1; a.idx[j] = kp; a.amp[j] = a.grid[kp]; }
        if (failed) cnt[3 * m] += 1;
        s_accept = accept ? 1 : 0;
    }
    __syncthreads();
    if (!s_accept) return;
    for (i = tid; i < n; i += AMP_THREADS) fj[i] = c * fj[i];
}

// draws[slot, j] = k_j, hist[k_j, j] += 1: thread j is the one writer of column j
__global__ __launch_bounds__(AMP_THREADS) void amp_record_kernel(const int* __restrict__ idx, int64_t m, int P, int64_t slot,
                                                                 uint32_t* __restrict__ hist, int32_t* __restrict__ draws)
{
    const int64_t j = (int64_t)blockIdx.x * AMP_THREADS + threadIdx.x;
    if (j >= m) return;
    const int k = idx[j];
    draws[slot * m + j] = k;
    if (k >= 0 && k < P) hist[(int64_t)k * m + j] += 1u;
}

}  // namespace

int launch_amp_scale(hipStream_t st, double* nu, const double* amp, int64_t n, int64_t m)
{
    if (n <= 0 || m <= 0) return 0;
    hipLaunchKernelGGL(amp_scale_kernel, dim3((unsigned)((n + AMP_THREADS - 1) / AMP_THREADS), (unsigned)m), dim3(AMP_THREADS), 0, st,
                       nu, amp, n);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_amp_update(hipStream_t st, const AmpUpdateArgs& a)
{
    if (a.n <= 0 || a.m <= 0) return 0;
    hipLaunchKernelGGL(amp_update_kernel, dim3((unsigned)a.m), dim3(AMP_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_amp_record(hipStream_t st, const int* idx, int64_t m, int P, int64_t slot, uint32_t* hist, int32_t* draws)
{
    hipLaunchKernelGGL(amp_record_kernel, dim3((unsigned)((m + AMP_THREADS - 1) / AMP_THREADS)), dim3(AMP_THREADS), 0, st, idx, m, P,
                       slot, hist, draws);
    GP_HIP(hipGetLastError());
    return 0;
}

int amp_nearest_one(const double* grid, int P)
{
    int best = 0;
    long double dist = fabsl(logl((long double)grid[0]));
    for (int k = 1; k < P; ++k) {
        const long double d = fabsl(logl((long double)grid[k]));
        if (d < dist) { dist = d; best = k; }
    }
    return best;
}

}  // namespace gpirt

using namespace gpirt;

extern "C" {

int gpirt_amp_check(double lo, double hi, int P, const double* log_prior, int width, const int* k0, int64_t m,
                    const gpirt_options* opts)
{
    if (P < 2 || P > GPIRT_AMP_MAX_POINTS) {
        set_error("amplitude grid: P = %d points, it must lie in 2 .. %d", P, GPIRT_AMP_MAX_POINTS);
        return GPIRT_E_ARG;
    }
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo >= GPIRT_AMP_MIN) || !(hi <= GPIRT_AMP_MAX) || !(lo < hi)) {
        set_error("amplitude grid: lo = %g, hi = %g, they must satisfy %g <= lo < hi <= %g", lo, hi, (double)GPIRT_AMP_MIN,
                  (double)GPIRT_AMP_MAX);
        return GPIRT_E_ARG;
    }
    std::vector<double> grid((size_t)P);
    ell_grid_fill(lo, hi, P, grid.data());
    for (int k = 1; k < P; ++k)
        if (!(grid[(size_t)k] > grid[(size_t)k - 1])) {
            set_error("amplitude grid: %d points between %.17g and %.17g are not strictly increasing in fp64", P, lo, hi);
            return GPIRT_E_ARG;
        }
    if (log_prior)
        for (int k = 0; k < P; ++k)
            if (!std::isfinite(log_prior[k])) { set_error("amplitude: log_prior[%d] is not finite", k); return GPIRT_E_ARG; }
    if (width < 1 || width > P - 1) {
        set_error("amplitude: width = %d, it must lie in 1 .. P - 1 = %d", width, P - 1);
        return GPIRT_E_ARG;
    }
    if (m < 0) { set_error("amplitude: m = %lld items", (long long)m); return GPIRT_E_ARG; }
    if (k0)
        for (int64_t j = 0; j < m; ++j)
            if (k0[j] < 0 || k0[j] >= P) {
                set_error("amplitude: starting index k0[%lld] = %d, it must lie in 0 .. P - 1 = %d", (long long)j, k0[j], P - 1);
                return GPIRT_E_ARG;
            }
    if (opts) {
        if (opts->rng_kind == GPIRT_RNG_RSTREAM) {
            set_error("amplitude: rng = reference (GPIRT_RNG_RSTREAM) is refused, R's stream has no such draw");
            return GPIRT_E_ARG;
        }
        if (opts->kernel_fp32) {
            set_error("amplitude: kernel_fp32 is refused, the single-precision build is the default kernel's alone");
            return GPIRT_E_ARG;
        }
        if (opts->item0 != 0 || (opts->m_total > 0 && m > 0 && opts->m_total != m)) {
            set_error("amplitude: an item shard (item0 = %lld, m_total = %lld) is refused, the amplitudes are kept for all items of one sampler",
                      (long long)opts->item0, (long long)opts->m_total);
            return GPIRT_E_ARG;
        }
    }
    return 0;
}

}  // extern "C"
