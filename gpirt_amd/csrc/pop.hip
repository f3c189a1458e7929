// pop.hip -- the population prior for theta (gpirt_sampler_pop_*, sampler.hip): respondent i carries a group code g_i and group
// g's prior is row g of a G x N table of log masses on the theta grid, which theta_sample_kernel<true> (stages.hip) adds in
// place of N(0, 1).  The kernels: the groups' sufficient statistics in exact integers, the one-launch exact Gibbs update of
// every group's (mu_g, sd_g) on two grids with the rebuild of the group's row, and the recorder of the indices.  Below them the
// host tables (the default row, a normal row, the grids, the grid normaliser lse) and the argument check.
//
// The order of every fp64 operation of the update is the header's ("a population prior for theta"); this file is compiled with
// -ffp-contract=off as every other, so each product and sum is rounded on its own and gpirt_amd/pop.py step_exact holds the bits.
#include "common.h"
#include "kernels.h"

#include <cmath>
#include <thread>
#include <vector>

namespace gpirt {

namespace {

constexpr int POP_THREADS = 256;
constexpr int POP_CENTRE = (GPIRT_NGRID - 1) / 2;

// Per group n_g, S1 = sum (k_i - 500), S2 = sum (k_i - 500)^2 over the members on the grid, and the members off it.  Integer
// atomics in LDS, then one global atomic per value and work-group: integer addition is associative, the bits do not depend on
// the order.  stats is 4 x G row-major and zeroed in front of the launch.
__global__ __launch_bounds__(POP_THREADS) void pop_stats_kernel(const double* __restrict__ theta, const int32_t* __restrict__ codes,
                                                                int64_t n, int G, unsigned long long* __restrict__ stats)
{
    __shared__ unsigned long long acc[4 * GPIRT_POP_MAX_GROUPS];
    const int tid = threadIdx.x;
    if (tid < 4 * GPIRT_POP_MAX_GROUPS) acc[tid] = 0ull;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * POP_THREADS + tid; i < n; i += (int64_t)gridDim.x * POP_THREADS) {
        const int g = codes[i];
        if (g < 0 || g >= G) continue;                                        // (refused at the entry: never taken)
        const int k = grid_index(theta[i]);
        if (k < 0) { atomicAdd(&acc[3 * GPIRT_POP_MAX_GROUPS + g], 1ull); continue; }
        const long long d = (long long)k - POP_CENTRE;
        atomicAdd(&acc[g], 1ull);
        atomicAdd(&acc[GPIRT_POP_MAX_GROUPS + g], (unsigned long long)d);     // (two's complement: the sum wraps to the signed one)
        atomicAdd(&acc[2 * GPIRT_POP_MAX_GROUPS + g], (unsigned long long)(d * d));
    }
    __syncthreads();
    if (tid < 4 * GPIRT_POP_MAX_GROUPS) {
        const int r = tid / GPIRT_POP_MAX_GROUPS, g = tid % GPIRT_POP_MAX_GROUPS;
        if (g < G && acc[tid] != 0ull) atomicAdd(&stats[r * G + g], acc[tid]);
    }
}

// lp[0 .. 3] are the log masses of the points 4 tid .. 4 tid + 3 (-inf at and beyond P).  Subtract the maximum, exp, inclusive
// scan, (C - C_0) / (C_last - C_0) against u: theta_sample_kernel's layout and its rule, the first index whose CDF exceeds u.
// Returns that index in every thread, -1 where no point does (C_last = C_0, or a NaN).
__device__ int pop_grid_draw(double lp[4], int P, double u, double* red, double* scan, int* ired)
{
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double mx = fmax(fmax(lp[0], lp[1]), fmax(lp[2], lp[3]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
    if (lane == 0) red[w] = mx;
    __syncthreads();
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    double run = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = t * 4 + e;
        const double v = (k < P) ? exp(lp[e] - mx) : 0.0;
        run += v;
        lp[e] = run;
    }
    scan[t] = run;
    __syncthreads();
    for (int d = 1; d < POP_THREADS; d <<= 1) {                             // Hillis-Steele inclusive scan of the thread totals
        const double add = (t >= d) ? scan[t - d] : 0.0;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    const double base = (t > 0) ? scan[t - 1] : 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) lp[e] += base;
    if (t == 0) red[0] = lp[0];                                             // C_0
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (t * 4 + e == P - 1) red[1] = lp[e];                             // C_last
    __syncthreads();
    const double c0 = red[0], range = red[1] - red[0];
    int first = 0x7fffffff;
#pragma unroll
    for (int e = 3; e >= 0; --e) {
        const int k = t * 4 + e;
        if (k < P) {
            const double cdf = (lp[e] - c0) / range;
            if (cdf > u) first = k;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
    if (lane == 0) ired[w] = first;
    __syncthreads();
    first = min(min(ired[0], ired[1]), min(ired[2], ired[3]));
    __syncthreads();
    return first == 0x7fffffff ? -1 : first;
}

// One work-group per group g = blockIdx.x + 1 (group 0 is the anchor).  mu given sd, sd given the new mu, then the group's row.
// idx, lp_mu, lp_sd, the row and counts (4 x G: calls, updated, skipped, failed) have this one writer per value.
__global__ __launch_bounds__(POP_THREADS) void pop_update_kernel(PopUpdateArgs p)
{
    __shared__ double red[8];
    __shared__ double scan[POP_THREADS];
    __shared__ int ired[4];
    const int tid = threadIdx.x;
    const int g = (int)blockIdx.x + 1, G = p.G;
    long long* cnt = p.counts + g;
    if (tid == 0) cnt[0] += 1;
    if (p.stats[3 * G + g] != 0) {                                            // a member off the grid: the group stays
        if (tid == 0) cnt[2 * G] += 1;
        return;
    }
    const double fn = (double)p.stats[g], fS1 = (double)p.stats[G + g], fS2 = (double)p.stats[2 * G + g];
    const double c = 0.01;
    const double A = (fS2 * c) * c;
    const int b0 = p.idx[2 * g + 1];                                          // (mu's old index is not read: Gibbs)
    const double u0 = item_uniform(p.seed, p.t, GPIRT_ST_POP, (uint32_t)g, 0), u1 = item_uniform(p.seed, p.t, GPIRT_ST_POP, (uint32_t)g, 1);
    double lp[4];
    // mu given sd_b0
    {
        const double s = p.sd[b0];
        const double den = 2.0 * (s * s);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int a = tid * 4 + e;
            if (a < p.P_mu) {
                const double m = p.mu[a];
                const double B = ((2.0 * m) * fS1) * c;
                const double C = (fn * m) * m;
                const double Q = (A - B) + C;
                lp[e] = (p.hyper_mu[a] - Q / den) - fn * p.lse[(int64_t)a * p.P_sd + b0];
                p.lp_mu[(int64_t)g * p.P_mu + a] = lp[e];
            } else lp[e] = -INFINITY;
        }
    }
    const int a1 = pop_grid_draw(lp, p.P_mu, u0, red, scan, ired);
    if (a1 < 0) {                                                             // (uniform over the work-group)
        if (tid == 0) cnt[3 * G] += 1;
        return;
    }
    // sd given mu_a1
    {
        const double m = p.mu[a1];
        const double B = ((2.0 * m) * fS1) * c;
        const double C = (fn * m) * m;
        const double Q = (A - B) + C;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int b = tid * 4 + e;
            if (b < p.P_sd) {
                const double s = p.sd[b];
                const double den = 2.0 * (s * s);
                lp[e] = (p.hyper_sd[b] - Q / den) - fn * p.lse[(int64_t)a1 * p.P_sd + b];
                p.lp_sd[(int64_t)g * p.P_sd + b] = lp[e];
            } else lp[e] = -INFINITY;
        }
    }
    const int b1 = pop_grid_draw(lp, p.P_sd, u1, red, scan, ired);
    if (b1 < 0) {                                                             // (mu's index is not kept either: the pair moves or stays)
        if (tid == 0) cnt[3 * G] += 1;
        return;
    }
    if (tid == 0) { p.idx[2 * g] = a1; p.idx[2 * g + 1] = b1; cnt[G] += 1; }
    const double m = p.mu[a1], s = p.sd[b1];
    double* row = p.log_prior + (int64_t)g * p.N;
    for (int k = tid; k < p.N; k += POP_THREADS) {
        const double z = ((-5.0 + (double)k * 0.01) - m) / s;
        row[k] = -(0.5 * z * z);
    }
}

__global__ void pop_record_kernel(const int* __restrict__ idx, int G, int P_mu, int P_sd, int64_t slot, uint32_t* __restrict__ hist_mu,
                                  uint32_t* __restrict__ hist_sd, int32_t* __restrict__ draws)
{
    const int g = threadIdx.x;
    if (g >= G) return;
    const int a = idx[2 * g], b = idx[2 * g + 1];
    draws[slot * 2 * G + 2 * g] = a;
    draws[slot * 2 * G + 2 * g + 1] = b;
    if (a >= 0 && a < P_mu) hist_mu[(int64_t)a * G + g] += 1u;
    if (b >= 0 && b < P_sd) hist_sd[(int64_t)b * G + g] += 1u;
}

}  // namespace

int launch_pop_stats(hipStream_t st, const double* theta, const int32_t* codes, int64_t n, int G, long long* stats)
{
    GP_HIP(hipMemsetAsync(stats, 0, sizeof(long long) * 4 * (size_t)G, st));
    if (n <= 0) return 0;
    int64_t blocks = (n + POP_THREADS - 1) / POP_THREADS;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(pop_stats_kernel, dim3((unsigned)blocks), dim3(POP_THREADS), 0, st, theta, codes, n, G,
                       (unsigned long long*)stats);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_pop_update(hipStream_t st, const PopUpdateArgs& a)
{
    if (a.G < 2) return 0;
    hipLaunchKernelGGL(pop_update_kernel, dim3((unsigned)(a.G - 1)), dim3(POP_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_pop_record(hipStream_t st, const int* idx, int G, int P_mu, int P_sd, int64_t slot, uint32_t* hist_mu, uint32_t* hist_sd,
                      int32_t* draws)
{
    hipLaunchKernelGGL(pop_record_kernel, dim3(1), dim3(64), 0, st, idx, G, P_mu, P_sd, slot, hist_mu, hist_sd, draws);
    GP_HIP(hipGetLastError());
    return 0;
}

// r_dnorm_log(ts, 0.0, 1.0) of stages.hip: (ts - 0.0) / 1.0 and + log(1.0) change no bit, and nothing is contracted
void pop_default_row(double* row)
{
    const double ln_sqrt_2pi = 0.918938533204672741780329736406;          // stages.hip GP_LN_SQRT_2PI
    for (int k = 0; k < GPIRT_NGRID; ++k) {
        const double z = fabs(-5.0 + (double)k * 0.01);
        row[k] = -(ln_sqrt_2pi + 0.5 * z * z);
    }
}

void pop_normal_row(double mu, double sd, double* row)
{
    for (int k = 0; k < GPIRT_NGRID; ++k) {
        const double z = ((-5.0 + (double)k * 0.01) - mu) / sd;
        row[k] = -(0.5 * z * z);
    }
}

void pop_grids_fill(double mu_hi, int P_mu, double sd_lo, double sd_hi, int P_sd, double* mu, double* sd)
{
    // mu_a = mu_hi (2a - (P - 1)) / (P - 1) in long double, rounded once: antisymmetric bit for bit, the end points exact
    for (int a = 0; a < P_mu; ++a)
        mu[a] = (double)(((long double)(2 * a - (P_mu - 1)) / (long double)(P_mu - 1)) * (long double)mu_hi);
    ell_grid_fill(sd_lo, sd_hi, P_sd, sd);
}

void pop_lse_fill(const double* mu, int P_mu, const double* sd, int P_sd, double* lse)
{
    // every entry is a sum of its own in a fixed order: the rows go to up to 8 host threads, the bits do not depend on how
    auto rows = [=](int first, int step) {
        for (int a = first; a < P_mu; a += step)
            for (int b = 0; b < P_sd; ++b) {
                const long double m = (long double)mu[a], den = 2.0L * ((long double)sd[b] * (long double)sd[b]);
                long double sum = 0.0L;
                for (int k = 0; k < GPIRT_NGRID; ++k) {
                    const long double d = (long double)(-5.0 + (double)k * 0.01) - m;
                    sum += expl(-(d * d) / den);
                }
                lse[(size_t)a * (size_t)P_sd + (size_t)b] = (double)logl(sum);
            }
    };
    const int nt = (int64_t)P_mu * P_sd < 4096 ? 1 : (P_mu < 8 ? P_mu : 8);
    if (nt <= 1) { rows(0, 1); return; }
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(rows, t, nt);
    rows(0, nt);
    for (std::thread& t : pool) t.join();
}

}  // namespace gpirt

using namespace gpirt;

extern "C" {

int gpirt_pop_check(const int32_t* codes, int64_t n, int G, const double* log_prior, int64_t rows, int sampled, double mu_hi,
                    int P_mu, double sd_lo, double sd_hi, int P_sd, const double* log_hyper_mu, const double* log_hyper_sd,
                    const int* a0, const int* b0, const gpirt_options* opts)
{
    if (G < 1 || G > GPIRT_POP_MAX_GROUPS) {
        set_error("population prior: G = %d groups, it must lie in 1 .. %d", G, GPIRT_POP_MAX_GROUPS);
        return GPIRT_E_ARG;
    }
    if (n < 0) { set_error("population prior: n = %lld respondents", (long long)n); return GPIRT_E_ARG; }
    if (codes) {
        int64_t members[GPIRT_POP_MAX_GROUPS] = {};
        for (int64_t i = 0; i < n; ++i) {
            if (codes[i] < 0 || codes[i] >= G) {
                set_error("population prior: codes[%lld] = %d, it must lie in 0 .. G - 1 = %d (every respondent has a prior: -1 is not allowed)",
                          (long long)i, (int)codes[i], G - 1);
                return GPIRT_E_ARG;
            }
            members[codes[i]] += 1;
        }
        for (int g = 0; g < G; ++g)
            if (members[g] == 0) { set_error("population prior: group %d has no member", g); return GPIRT_E_ARG; }
    }
    if (log_prior)
        for (int64_t r = 0; r < rows; ++r)
            for (int k = 0; k < GPIRT_NGRID; ++k)
                if (!std::isfinite(log_prior[r * GPIRT_NGRID + k])) {
                    set_error("population prior: log_prior[%lld, %d] is not finite", (long long)r, k);
                    return GPIRT_E_ARG;
                }
    if (sampled) {
        if (P_mu < 2 || P_mu > GPIRT_POP_MAX_POINTS || P_sd < 2 || P_sd > GPIRT_POP_MAX_POINTS) {
            set_error("population prior: P_mu = %d and P_sd = %d points, each must lie in 2 .. %d", P_mu, P_sd, GPIRT_POP_MAX_POINTS);
            return GPIRT_E_ARG;
        }
        if (!std::isfinite(mu_hi) || !(mu_hi > 0.0) || !(mu_hi <= 5.0)) {
            set_error("population prior: mu_hi = %g, it must lie in (0, 5]: the means stay on the theta grid's range", mu_hi);
            return GPIRT_E_ARG;
        }
        if (!std::isfinite(sd_lo) || !std::isfinite(sd_hi) || !(sd_lo >= GPIRT_POP_SD_MIN) || !(sd_lo < sd_hi) || !(sd_hi <= GPIRT_POP_SD_MAX)) {
            set_error("population prior: sd_lo = %g, sd_hi = %g, they must satisfy %g <= sd_lo < sd_hi <= %g", sd_lo, sd_hi,
                      (double)GPIRT_POP_SD_MIN, (double)GPIRT_POP_SD_MAX);
            return GPIRT_E_ARG;
        }
        std::vector<double> mu((size_t)P_mu), sd((size_t)P_sd);
        pop_grids_fill(mu_hi, P_mu, sd_lo, sd_hi, P_sd, mu.data(), sd.data());
        for (int a = 1; a < P_mu; ++a)
            if (!(mu[(size_t)a] > mu[(size_t)a - 1])) {
                set_error("population prior: %d mu points up to %.17g are not strictly increasing in fp64", P_mu, mu_hi);
                return GPIRT_E_ARG;
            }
        for (int b = 1; b < P_sd; ++b)
            if (!(sd[(size_t)b] > sd[(size_t)b - 1])) {
                set_error("population prior: %d sd points between %.17g and %.17g are not strictly increasing in fp64", P_sd, sd_lo, sd_hi);
                return GPIRT_E_ARG;
            }
        if (log_hyper_mu)
            for (int a = 0; a < P_mu; ++a)
                if (!std::isfinite(log_hyper_mu[a])) { set_error("population prior: log_hyper_mu[%d] is not finite", a); return GPIRT_E_ARG; }
        if (log_hyper_sd)
            for (int b = 0; b < P_sd; ++b)
                if (!std::isfinite(log_hyper_sd[b])) { set_error("population prior: log_hyper_sd[%d] is not finite", b); return GPIRT_E_ARG; }
        for (int g = 1; g < G; ++g) {
            if (a0 && (a0[g] < 0 || a0[g] >= P_mu)) {
                set_error("population prior: starting index a0[%d] = %d, it must lie in 0 .. P_mu - 1 = %d", g, a0[g], P_mu - 1);
                return GPIRT_E_ARG;
            }
            if (b0 && (b0[g] < 0 || b0[g] >= P_sd)) {
                set_error("population prior: starting index b0[%d] = %d, it must lie in 0 .. P_sd - 1 = %d", g, b0[g], P_sd - 1);
                return GPIRT_E_ARG;
            }
        }
    }
    if (opts) {
        if (sampled && opts->rng_kind == GPIRT_RNG_RSTREAM) {
            set_error("population prior: the sampled mode is refused under rng = reference (GPIRT_RNG_RSTREAM), R's stream has no such draw");
            return GPIRT_E_ARG;
        }
        if (opts->item0 != 0) {                                 // (m_total != m is the sampler's to see: sampler.hip pop_refusals)
            set_error("population prior: an item shard (item0 = %lld, m_total = %lld) is refused, the respondent-block theta path "
                      "would need the codes of its respondents", (long long)opts->item0, (long long)opts->m_total);
            return GPIRT_E_ARG;
        }
    }
    return 0;
}

int gpirt_pop_default_row(double* row) { GP_ARG(row != nullptr); pop_default_row(row); return 0; }

int gpirt_pop_normal_row(double mu, double sd, double* row)
{
    GP_ARG(row != nullptr);
    if (!std::isfinite(mu) || !std::isfinite(sd) || !(sd > 0.0)) { set_error("population prior: a normal row needs a finite mu and sd > 0"); return GPIRT_E_ARG; }
    pop_normal_row(mu, sd, row);
    return 0;
}

int gpirt_pop_grids(double mu_hi, int P_mu, double sd_lo, double sd_hi, int P_sd, double* mu, double* sd)
{
    GP_ARG(mu && sd);
    GP_TRY(gpirt_pop_check(nullptr, 0, 1, nullptr, 0, 1, mu_hi, P_mu, sd_lo, sd_hi, P_sd, nullptr, nullptr, nullptr, nullptr, nullptr));
    pop_grids_fill(mu_hi, P_mu, sd_lo, sd_hi, P_sd, mu, sd);
    return 0;
}

int gpirt_pop_lse(const double* mu, int P_mu, const double* sd, int P_sd, double* lse)
{
    GP_ARG(mu && sd && lse && P_mu >= 1 && P_sd >= 1);
    for (int b = 0; b < P_sd; ++b)
        if (!(sd[b] > 0.0) || !std::isfinite(sd[b])) { set_error("population prior: sd[%d] = %g", b, sd[b]); return GPIRT_E_ARG; }
    pop_lse_fill(mu, P_mu, sd, P_sd, lse);
    return 0;
}

}  // extern "C"
