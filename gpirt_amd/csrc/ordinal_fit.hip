// ordinal_fit.hip -- fit output for the ordinal (graded) model, accumulated on the device one draw at a time (include/gpirt_hip.h,
// "ordinal model fit"; library version 142): pointwise WAIC, per-cell category predictions and the
// first-order posterior predictive check.  With g = f + mu, an item's thresholds b_1 < ... < b_{C-1} and d_c = g - b_c,
//     E_c = exp(-|d_c|)                                   one per threshold; it serves e_c and both ll terms
//     e_c = P(y > c) = d_c >= 0 ? 1 / (1 + E_c) : E_c / (1 + E_c)                  (summary.hip's cell_terms)
//     ll(b_c - g) = log1p(E_c) + max(d_c, 0),   ll(g - b_c) = log1p(E_c) + max(-d_c, 0)
//     logP(c) = v:  v = 0;  c < C: v = -ll(b_c - g);  c > 1: v = v - ll(g - b_{c-1});  1 < c < C: v = v + w_c,
//     w_c = log1p(-exp(-(b_c - b_{c-1})))                 at most C - 2 per item, formed once per work-group
// exp and log1p are the device library's precise forms.  No category probability is formed as a difference of two sigmas.
//
// ofit_cell_kernel<WAIC, PRED, PPC> is one streaming pass over 256 respondents x a strip of OFIT_STRIP items per work-group
// (ppc_replicate_kernel's geometry): f, mu and cat are read once, lanes along the respondents (coalesced).  The strip's thresholds
// and w values are staged in LDS once.  A lane owns one respondent over the strip.
//   WAIC  the cell's lse (a logaddexp; the first draw sets it) and the Welford pair of logP(cat): read and written once, one owner.
//   PRED  sum e_c of every cell, missing ones included, in C - 1 planes of n x m: read and written once, one owner.
//   PPC   rep = 1 + #{c : u < e_c}, u = item_uniform(seed, iteration, GPIRT_ST_ORD_PPC, item0 + j, i), for an observed cell with a
//         finite g; per cell -2 logP(cat), -2 logP(rep) and, where rep != cat, logP(cat) - logP(rep).
// THE ORDER OF EVERY fp64 SUM.  A row partial: the lane adds its cells in ascending item order within the strip.  A column
// partial: the wave's fixed shuffle tree (offsets 32, 16, .., 1), one LDS slot per wave, then (w0 + w1) + (w2 + w3).  The integer
// partials are packed (score 12 bits, agreeing cells 10, non-finite cells 10; the replicate's category counts 8 bits each in one
// 64-bit word per wave) and travel through the same tree.  ofit_units_kernel: item k adds its row blocks' partials in ascending
// block order, respondent i its strips' partials in ascending strip order; it decides the integer comparisons and updates the
// unit's accumulators (one thread per unit).  ofit_total_kernel: thread t adds the items' sums of the draw for items t, t + 256,
// ... ascending, then block_sum_256's tree.  The WAIC totals: 1024 blocks of 256 threads, thread partials over a grid-stride loop in
// ascending cell order, an LDS tree per block, then one block over the 1024 partials in the same way (summary.hip's totals).
// There is no floating-point atomic anywhere and every value has one writer: two runs give a byte-identical state, and the
// geometry is fixed, so the sums do not depend on the device.
//
// A unit (item, respondent, the whole matrix) with a non-finite g in an observed cell in a draw counts that draw in `nonfinite` and
// leaves it out of every sum of the unit, the item's category counts included (ppc.hip's rule).  A non-finite g in a missing cell
// touches nothing but that cell's PRED sums.
#include "common.h"
#include "kernels.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace gpirt {

namespace {

constexpr int OFIT_THREADS = 256;
constexpr int OFIT_STRIP = 32;
constexpr int OFIT_TOTAL_BLOCKS = 1024;
constexpr int OFIT_MAXC = GPIRT_ORD_MAX_C;          // 8
constexpr uint32_t OK_SCORE = 1u, OK_AGREE = 1u << 12, OK_NONFINITE = 1u << 22;
constexpr uint32_t OK_SCORE_MASK = 4095u, OK_MASK10 = 1023u;
constexpr int64_t OFIT_TAG = 0x5449464F;            // "OFIT"
constexpr double OFIT_MISSING_M2 = -1.0;

struct OfitArgs {
    const double* f; const double* mu; const int8_t* cat; const double* thr;
    int64_t n, m;
    int C, first;
    double draw;
    uint64_t seed; uint32_t iter, item0;
    double *lse, *mean, *m2, *pred;
    double* rowd; uint32_t* rowi;        // [strip][3][n], [strip][n]: Delta, -2 sum logP(cat), -2 sum logP(rep); the packed counts
    double* cold; uint32_t* coli;        // [row block][3][m], [row block][m]
    uint32_t* colc;                      // [row block][m][8]: the replicate's cells per category
    int8_t* rep;                         // n x m: the last draw's replicate (0: missing or non-finite)
};

#define OFIT_EACH(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6)
#define OFIT_DECL(q) [[maybe_unused]] double d##q = 0.0, E##q = 0.0, e##q = 0.0;
#define OFIT_FORM(q)                                                                \
    if (q < C - 1) {                                                                \
        d##q = g - bt[jj][q + 1];                                                   \
        E##q = exp(-fabs(d##q));                                                    \
        e##q = d##q >= 0.0 ? 1.0 / (1.0 + E##q) : E##q / (1.0 + E##q);              \
    }
#define OFIT_PRED_ADD(q) if (q < C - 1) a.pred[(int64_t)q * cells + at] += e##q;
#define OFIT_PICK(q) if (c == q + 1) { dd = d##q; EE = E##q; }
#define OFIT_COUNT(q) if (q < C - 1 && u < e##q) ++rep;
static_assert(OFIT_MAXC == 8, "OFIT_EACH names the seven thresholds");

template <bool WAIC, bool PRED, bool PPC>
__global__ __launch_bounds__(OFIT_THREADS) void ofit_cell_kernel(OfitArgs a)
{
    constexpr bool ALL = PRED || PPC;              // every threshold's E_c is needed (else the category's own two)
    __shared__ double bt[OFIT_STRIP][OFIT_MAXC];   // bt[jj][c] = b_c, c = 1 .. C - 1
    __shared__ double wt[OFIT_STRIP][OFIT_MAXC];   // wt[jj][c] = w_c, c = 2 .. C - 1
    __shared__ double sd[4][OFIT_STRIP][3];
    __shared__ uint32_t si[4][OFIT_STRIP];
    __shared__ unsigned long long sc[4][OFIT_STRIP];
    const int rb = blockIdx.x, strip = blockIdx.y;
    const int64_t i = (int64_t)rb * OFIT_THREADS + threadIdx.x;
    const bool live = i < a.n;
    const int64_t j0 = (int64_t)strip * OFIT_STRIP;
    const int w = (int)(a.m - j0 < OFIT_STRIP ? a.m - j0 : OFIT_STRIP);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int C = a.C;
    const int64_t cells = a.n * a.m;
    {
        static_assert(OFIT_THREADS == OFIT_STRIP * OFIT_MAXC, "one staged value per thread");
        const int jj = threadIdx.x >> 3, c = threadIdx.x & 7;
        double b = 0.0, wc = 0.0;
        if (jj < w && c >= 1 && c < C) {
            const double* tj = a.thr + (j0 + jj) * (C - 1);
            b = tj[c - 1];
            if (c >= 2) wc = log1p(-exp(-(b - tj[c - 2])));
        }
        bt[jj][c] = b; wt[jj][c] = wc;
    }
    __syncthreads();
    double rD = 0.0, rO = 0.0, rR = 0.0;
    uint32_t rI = 0;
    for (int jj = 0; jj < w; ++jj) {
        double cD = 0.0, cO = 0.0, cR = 0.0;
        uint32_t cI = 0;
        unsigned long long cK = 0;
        if (live) {
            const int64_t at = i + (j0 + jj) * a.n;
            const int cv = a.cat[at];
            if (PRED || cv != 0) {
                const double g = a.f[at] + a.mu[at];
                // the seven thresholds' values as named scalars (an indexed array went to scratch): q = c - 1
                OFIT_EACH(OFIT_DECL)
                if constexpr (ALL) { OFIT_EACH(OFIT_FORM) }
                if constexpr (PRED) { OFIT_EACH(OFIT_PRED_ADD) }
                // d_c and E_c of threshold c = 1 .. C - 1
                auto dE = [&](int c, double& dd, double& EE) {
                    if constexpr (ALL) {
                        dd = d0; EE = E0;
                        OFIT_EACH(OFIT_PICK)
                    } else {
                        dd = g - bt[jj][c];
                        EE = exp(-fabs(dd));
                    }
                };
                auto logp = [&](int c) -> double {
                    double v = 0.0, dd, EE;
                    if (c < C) { dE(c, dd, EE); v = -(log1p(EE) + fmax(dd, 0.0)); }
                    if (c > 1) { dE(c - 1, dd, EE); v = v - (log1p(EE) + fmax(-dd, 0.0)); }
                    if (c > 1 && c < C) v = v + wt[jj][c];
                    return v;
                };
                if (cv != 0) {
                    const double lpc = logp(cv);
                    if constexpr (WAIC) {
                        const double lse = a.lse[at];
                        double mean = a.mean[at], m2 = a.m2[at];
                        a.lse[at] = a.first ? lpc : fmax(lse, lpc) + log1p(exp(-fabs(lse - lpc)));
                        const double delta = lpc - mean;
                        mean += delta / a.draw;
                        m2 += delta * (lpc - mean);
                        a.mean[at] = mean; a.m2[at] = m2;
                    }
                    if constexpr (PPC) {
                        int8_t rep8 = 0;
                        if (!isfinite(g)) cI = OK_NONFINITE;
                        else {
                            const double u = item_uniform(a.seed, a.iter, GPIRT_ST_ORD_PPC, (uint32_t)(a.item0 + j0 + jj), (uint32_t)i);
                            int rep = 1;
                            OFIT_EACH(OFIT_COUNT)
                            const double lpr = rep == cv ? lpc : logp(rep);
                            cO = -2.0 * lpc;
                            cR = -2.0 * lpr;
                            if (rep != cv) cD = lpc - lpr;
                            cI = (uint32_t)rep * OK_SCORE + (rep == cv ? OK_AGREE : 0u);
                            cK = 1ull << (8 * (rep - 1));
                            rep8 = (int8_t)rep;
                        }
                        a.rep[at] = rep8;
                    }
                } else if constexpr (PPC) a.rep[at] = 0;
            } else if constexpr (PPC) a.rep[at] = 0;
        }
        if constexpr (PPC) {
            rD += cD; rO += cO; rR += cR; rI += cI;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                cD += __shfl_down(cD, off, 64);
                cO += __shfl_down(cO, off, 64);
                cR += __shfl_down(cR, off, 64);
                cI += __shfl_down(cI, off, 64);
                cK += __shfl_down(cK, off, 64);       // (at most 64 cells of a wave in a field of 8 bits)
            }
            if (lane == 0) { sd[wv][jj][0] = cD; sd[wv][jj][1] = cO; sd[wv][jj][2] = cR; si[wv][jj] = cI; sc[wv][jj] = cK; }
        }
    }
    if constexpr (PPC) {
        if (live) {
            const int64_t base = (int64_t)strip * 3 * a.n + i;
            a.rowd[base] = rD; a.rowd[base + a.n] = rO; a.rowd[base + 2 * a.n] = rR;
            a.rowi[(int64_t)strip * a.n + i] = rI;
        }
        __syncthreads();
        if ((int)threadIdx.x < w) {
            const int jj = threadIdx.x;
            const int64_t base = (int64_t)rb * 3 * a.m + j0 + jj;
#pragma unroll
            for (int q = 0; q < 3; ++q)
                a.cold[base + q * a.m] = (sd[0][jj][q] + sd[1][jj][q]) + (sd[2][jj][q] + sd[3][jj][q]);
            a.coli[(int64_t)rb * a.m + j0 + jj] = (si[0][jj] + si[1][jj]) + (si[2][jj] + si[3][jj]);
            uint32_t* kc = a.colc + ((int64_t)rb * a.m + j0 + jj) * OFIT_MAXC;
#pragma unroll
            for (int c = 0; c < OFIT_MAXC; ++c) {
                uint32_t t = 0;
                for (int v = 0; v < 4; ++v) t += (uint32_t)((sc[v][jj] >> (8 * c)) & 255ull);
                kc[c] = t;
            }
        }
    }
}

struct OfitUnitArgs {
    const double* rowd; const uint32_t* rowi; const double* cold; const uint32_t* coli; const uint32_t* colc;
    int64_t n, m, stride;
    int C, strips, rblocks;
    uint64_t* units;                     // [OFIT_NUNIT][stride]
    uint64_t* cats;                      // [OFIT_NCAT][m x C]
    double* unit_d; uint64_t* unit_i;    // [3][m] each: the items' sums of this draw, for the total
    double* last_delta; int64_t* last_score; int64_t* last_counts;      // the last draw: units, units, m x C
};

// one draw of unit k; returns whether it entered the unit's sums
__device__ __forceinline__ bool ofit_update(const OfitUnitArgs& a, int64_t k, uint64_t R, uint64_t agree, uint64_t nonfinite, double D,
                                            double O, double Rp)
{
    uint64_t* acc = a.units;
    const int64_t stride = a.stride;
    a.last_delta[k] = D; a.last_score[k] = (int64_t)R;
    if (acc[OFIT_U_N_OBS * stride + k] == 0) return false;
    if (nonfinite) { acc[OFIT_U_NONFINITE * stride + k] += 1; return false; }
    const uint64_t T = acc[OFIT_U_OBS_SCORE * stride + k];
    acc[OFIT_U_REP_SUM * stride + k] += R;
    acc[OFIT_U_REP_SUMSQ * stride + k] += R * R;
    acc[OFIT_U_SCORE_GE * stride + k] += R >= T ? 1 : 0;
    acc[OFIT_U_SCORE_GT * stride + k] += R > T ? 1 : 0;
    acc[OFIT_U_DEV_GE * stride + k] += D >= 0.0 ? 1 : 0;
    acc[OFIT_U_AGREE * stride + k] += agree;
    double* dacc = reinterpret_cast<double*>(acc);
    dacc[OFIT_U_DEV_OBS * stride + k] += O;
    dacc[OFIT_U_DEV_REP * stride + k] += Rp;
    return true;
}

// unit k < m: item k, the row blocks' partials in order; else respondent k - m, the strips' partials in order
__global__ __launch_bounds__(OFIT_THREADS) void ofit_units_kernel(OfitUnitArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.m + a.n) return;
    double D = 0.0, O = 0.0, Rp = 0.0;
    uint64_t R = 0, agree = 0, nonfinite = 0;
    if (k < a.m) {
        uint64_t cnt[OFIT_MAXC] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int rb = 0; rb < a.rblocks; ++rb) {
            const int64_t base = (int64_t)rb * 3 * a.m + k;
            D += a.cold[base]; O += a.cold[base + a.m]; Rp += a.cold[base + 2 * a.m];
            const uint32_t pk = a.coli[(int64_t)rb * a.m + k];
            R += pk & OK_SCORE_MASK; agree += (pk >> 12) & OK_MASK10; nonfinite += (pk >> 22) & OK_MASK10;
            const uint32_t* kc = a.colc + ((int64_t)rb * a.m + k) * OFIT_MAXC;
#pragma unroll
            for (int c = 0; c < OFIT_MAXC; ++c) cnt[c] += kc[c];
        }
        a.unit_d[k] = D; a.unit_d[a.m + k] = O; a.unit_d[2 * a.m + k] = Rp;
        a.unit_i[k] = R; a.unit_i[a.m + k] = agree; a.unit_i[2 * a.m + k] = nonfinite;
        const bool in = ofit_update(a, k, R, agree, nonfinite, D, O, Rp);
        const int64_t mc = a.m * a.C;
#pragma unroll
        for (int c = 0; c < OFIT_MAXC; ++c)
            if (c < a.C) {
                const int64_t at = k * a.C + c;
                a.last_counts[at] = (int64_t)cnt[c];
                if (in) {
                    const uint64_t obs = a.cats[OFIT_K_OBS * mc + at], r = cnt[c];
                    a.cats[OFIT_K_REP_SUM * mc + at] += r;
                    a.cats[OFIT_K_REP_SUMSQ * mc + at] += r * r;
                    a.cats[OFIT_K_GE * mc + at] += r >= obs ? 1 : 0;
                    a.cats[OFIT_K_GT * mc + at] += r > obs ? 1 : 0;
                }
            }
    } else {
        const int64_t i = k - a.m;
        for (int s = 0; s < a.strips; ++s) {
            const int64_t base = (int64_t)s * 3 * a.n + i;
            D += a.rowd[base]; O += a.rowd[base + a.n]; Rp += a.rowd[base + 2 * a.n];
            const uint32_t pk = a.rowi[(int64_t)s * a.n + i];
            R += pk & OK_SCORE_MASK; agree += (pk >> 12) & OK_MASK10; nonfinite += (pk >> 22) & OK_MASK10;
        }
        ofit_update(a, k, R, agree, nonfinite, D, O, Rp);
    }
}

// the whole matrix: the items' sums of this draw, thread t taking items t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(OFIT_THREADS) void ofit_total_kernel(OfitUnitArgs a)
{
    __shared__ double sm[4];
    __shared__ unsigned long long cnt[3];
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    double v[3] = { 0.0, 0.0, 0.0 };
    unsigned long long c[3] = { 0, 0, 0 };
    for (int64_t j = threadIdx.x; j < a.m; j += OFIT_THREADS)
        for (int q = 0; q < 3; ++q) { v[q] += a.unit_d[q * a.m + j]; c[q] += a.unit_i[q * a.m + j]; }
    __syncthreads();
    for (int q = 0; q < 3; ++q) atomicAdd(&cnt[q], c[q]);        // integers: any order gives the same sum
    double t[3];
    for (int q = 0; q < 3; ++q) t[q] = block_sum_256(v[q], sm);
    __syncthreads();
    if (threadIdx.x == 0) ofit_update(a, a.m + a.n, cnt[0], cnt[1], cnt[2], t[0], t[1], t[2]);
}

// n_obs and obs_score of every item and respondent and the items' observed cells per category (once, at enable) ...
__global__ __launch_bounds__(OFIT_THREADS) void ofit_observed_kernel(const int8_t* __restrict__ cat, int64_t n, int64_t m, int C,
                                                                     int64_t stride, uint64_t* units, uint64_t* cats)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m + n) return;
    uint64_t obs = 0, score = 0;
    uint64_t cnt[OFIT_MAXC] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    const int64_t first = k < m ? k * n : k - m, step = k < m ? 1 : n, count = k < m ? n : m;
    for (int64_t q = 0; q < count; ++q) {
        const int v = cat[first + q * step];
        obs += v != 0 ? 1 : 0;
        score += (uint64_t)v;
#pragma unroll
        for (int c = 0; c < OFIT_MAXC; ++c) cnt[c] += v == c + 1 ? 1 : 0;
    }
    units[OFIT_U_N_OBS * stride + k] = obs;
    units[OFIT_U_OBS_SCORE * stride + k] = score;
    if (k < m)
#pragma unroll
        for (int c = 0; c < OFIT_MAXC; ++c)
            if (c < C) cats[OFIT_K_OBS * m * C + k * C + c] = cnt[c];
}

// ... and of the whole matrix, from the items'
__global__ void ofit_observed_total_kernel(int64_t n, int64_t m, int64_t stride, uint64_t* units)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t obs = 0, score = 0;
    for (int64_t j = 0; j < m; ++j) { obs += units[OFIT_U_N_OBS * stride + j]; score += units[OFIT_U_OBS_SCORE * stride + j]; }
    units[OFIT_U_N_OBS * stride + m + n] = obs;
    units[OFIT_U_OBS_SCORE * stride + m + n] = score;
}

__device__ void ofit_block_sum4(double (&v)[4], double (*sh)[OFIT_THREADS])
{
    const int t = threadIdx.x;
    for (int k = 0; k < 4; ++k) sh[k][t] = v[k];
    __syncthreads();
    for (int w = OFIT_THREADS / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int k = 0; k < 4; ++k) sh[k][t] += sh[k][t + w];
        __syncthreads();
    }
    for (int k = 0; k < 4; ++k) v[k] = sh[k][0];
}

// totals over the observed cells, block partials.  pass 0: [sum lppd_ij, sum p_waic_ij, n_obs, sum elpd_ij]; pass 1:
// [sum (elpd_ij - mean)^2] with mean = tot[4] of pass 0 (summary.hip's summary_totals_kernel; a missing cell is marked by its m2)
__global__ __launch_bounds__(OFIT_THREADS) void ofit_waic_part_kernel(const double* __restrict__ lse, const double* __restrict__ m2,
                                                                      int64_t cells, double log_s, double inv_s1, int pass,
                                                                      const double* __restrict__ tot,
                                                                      double* __restrict__ part)
{
    __shared__ double sh[4][OFIT_THREADS];
    double v[4] = { 0.0, 0.0, 0.0, 0.0 };
    const double mean = pass ? tot[4] : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
        if (m2[i] == OFIT_MISSING_M2) continue;           // a missing cell
        const double lppd = lse[i] - log_s, pw = m2[i] * inv_s1, e = lppd - pw;
        if (pass == 0) { v[0] += lppd; v[1] += pw; v[2] += 1.0; v[3] += e; }
        else { const double dv = e - mean; v[0] += dv * dv; }
    }
    ofit_block_sum4(v, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) part[(int64_t)blockIdx.x * 4 + k] = v[k];
}

// one block: the partials in block order; tot: lppd, p_waic, n_obs, sum elpd, mean elpd, sum of squares
__global__ __launch_bounds__(OFIT_THREADS) void ofit_waic_reduce_kernel(const double* __restrict__ part, int nblocks, int pass,
                                                                        double* __restrict__ tot)
{
    __shared__ double sh[4][OFIT_THREADS];
    double v[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (int b = threadIdx.x; b < nblocks; b += OFIT_THREADS)
        for (int k = 0; k < 4; ++k) v[k] += part[(int64_t)b * 4 + k];
    ofit_block_sum4(v, sh);
    if (threadIdx.x != 0) return;
    if (pass == 0) { tot[0] = v[0]; tot[1] = v[1]; tot[2] = v[2]; tot[3] = v[3]; tot[4] = v[3] / v[2]; }
    else tot[5] = v[0];
}

// pooling, chain b into the pooled block a (na and nb draws): elementwise, one owner per element
__global__ __launch_bounds__(OFIT_THREADS) void ofit_pool_waic_kernel(double* __restrict__ lse, double* __restrict__ mean,
                                                                      double* __restrict__ m2, const double* __restrict__ lse_b,
                                                                      const double* __restrict__ mean_b, const double* __restrict__ m2_b,
                                                                      int64_t cells, double na, double nb)
{
    const double nt = na + nb;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
        if (nb == 0.0 || m2[i] == OFIT_MISSING_M2) continue;
        if (na == 0.0) { lse[i] = lse_b[i]; mean[i] = mean_b[i]; m2[i] = m2_b[i]; continue; }
        const double x = lse[i], y = lse_b[i];
        lse[i] = fmax(x, y) + log1p(exp(-fabs(x - y)));
        const double delta = mean_b[i] - mean[i];
        mean[i] = mean[i] + delta * (nb / nt);
        m2[i] = (m2[i] + m2_b[i]) + (delta * delta) * (na * nb / nt);
    }
}

__global__ __launch_bounds__(OFIT_THREADS) void ofit_pool_add_f64_kernel(double* __restrict__ a, const double* __restrict__ b, int64_t count)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) a[i] += b[i];
}

__global__ __launch_bounds__(OFIT_THREADS) void ofit_pool_add_u64_kernel(uint64_t* __restrict__ a, const uint64_t* __restrict__ b, int64_t count)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) a[i] += b[i];
}

inline unsigned ofit_grid_for(int64_t total)
{
    int64_t b = (total + OFIT_THREADS - 1) / OFIT_THREADS;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// a missing cell's ll_m2 is OFIT_MISSING_M2 (an observed cell's is >= 0 or NaN): the block itself tells which cells the totals and
// the pooling take, and no accumulate ever touches a missing cell's WAIC words
__global__ __launch_bounds__(OFIT_THREADS) void ofit_mark_missing_kernel(const int8_t* __restrict__ cat, int64_t cells, double* __restrict__ m2)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x)
        if (cat[i] == 0) m2[i] = OFIT_MISSING_M2;
}

const char* const kUnitNames[OFIT_NUNIT] = { "n_obs", "obs_score", "score_ge", "score_gt", "rep_score_sum", "rep_score_sumsq",
                                             "agree_sum", "dev_ge", "nonfinite", "dev_obs_sum", "dev_rep_sum" };
const char* const kCatNames[OFIT_NCAT] = { "obs_count", "rep_count_sum", "rep_count_sumsq", "count_ge", "count_gt" };

int ofit_read_header(hipStream_t st, const void* d_block, int64_t* hdr, const char* who, int idx)
{
    GP_HIP(hipMemcpyAsync(hdr, d_block, sizeof(int64_t) * OFIT_HEADER_WORDS, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] != OFIT_TAG || hdr[1] != OFIT_LAYOUT_VERSION || hdr[2] <= 0 || hdr[3] <= 0 || hdr[4] < 2 || hdr[4] > OFIT_MAXC ||
        hdr[5] <= 0 || (hdr[5] & ~(int64_t)GPIRT_OFIT_ALL) || hdr[6] < 0) {
        set_error("%s: state %d is not an ordinal fit state block of layout %d", who, idx, OFIT_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    return 0;
}

int ofit_waic_totals(hipStream_t st, const double* lse, const double* m2, int64_t cells, int64_t draws, double* part,
                     double* tot, gpirt_ordinal_fit* out)
{
    const double S = (double)draws;
    const double log_s = std::log(S), inv_s1 = 1.0 / (S - 1.0);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(ofit_waic_part_kernel, dim3(OFIT_TOTAL_BLOCKS), dim3(OFIT_THREADS), 0, st, lse, m2, cells, log_s, inv_s1,
                           pass, tot, part);
        GP_HIP(hipGetLastError());
        hipLaunchKernelGGL(ofit_waic_reduce_kernel, dim3(1), dim3(OFIT_THREADS), 0, st, part, OFIT_TOTAL_BLOCKS, pass, tot);
        GP_HIP(hipGetLastError());
    }
    double h[8];
    GP_HIP(hipMemcpyAsync(h, tot, sizeof(h), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    out->lppd = h[0]; out->p_waic = h[1];
    out->elpd_waic = h[0] - h[1];
    out->waic = -2.0 * (h[0] - h[1]);
    out->se_elpd_waic = std::sqrt(h[2] * (h[5] / (h[2] - 1.0)));      // loo: sqrt(N var(elpd_i)), ddof = 1
    out->n_obs = (int64_t)h[2];
    return 0;
}

}  // namespace

OfitLayout ofit_layout(int64_t n, int64_t m, int C, int parts)
{
    OfitLayout L{};
    L.cells = n * m;
    L.stride = (n + m + 1 + 1) & ~(int64_t)1;
    int64_t at = OFIT_HEADER_WORDS;
    L.lse = L.mean = L.m2 = L.pred = L.units = L.cats = -1;
    if (parts & GPIRT_OFIT_WAIC) { L.lse = at; L.mean = at + L.cells; L.m2 = at + 2 * L.cells; at += 3 * L.cells; }
    if (parts & GPIRT_OFIT_PRED) { L.pred = at; at += (int64_t)(C - 1) * L.cells; }
    if (parts & GPIRT_OFIT_PPC) { L.units = at; at += (int64_t)OFIT_NUNIT * L.stride; L.cats = at; at += (int64_t)OFIT_NCAT * m * C; }
    L.words = at;
    return L;
}

int64_t ofit_state_words(const OfitState* p) { return p->L.words; }

void ofit_free(OfitState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = OfitState{};
}

int ofit_seal(hipStream_t st, OfitState* p)
{
    int64_t hdr[OFIT_HEADER_WORDS] = { OFIT_TAG, OFIT_LAYOUT_VERSION, p->n, p->m, p->C, p->parts, p->draws, p->item0 };
    GP_HIP(hipMemcpyAsync(p->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));       // hdr is on this stack
    return 0;
}

int ofit_alloc(hipStream_t st, OfitState* p, int64_t n, int64_t m, int C, int parts, int64_t item0, const int8_t* cat)
{
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes ? bytes : 8));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes ? bytes : 8, st));
        return 0;
    };
    p->n = n; p->m = m; p->C = C; p->parts = parts; p->item0 = item0; p->draws = 0;
    p->L = ofit_layout(n, m, C, parts);
    p->strips = (int)((m + OFIT_STRIP - 1) / OFIT_STRIP);
    p->rblocks = (int)((n + OFIT_THREADS - 1) / OFIT_THREADS);
    const size_t N = (size_t)n, M = (size_t)m, U = (size_t)(n + m + 1);
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)p->L.words));
    if (parts & GPIRT_OFIT_PPC) {
        GP_TRY(get((void**)&p->rowd, sizeof(double) * (size_t)p->strips * 3 * N));
        GP_TRY(get((void**)&p->rowi, sizeof(uint32_t) * (size_t)p->strips * N));
        GP_TRY(get((void**)&p->cold, sizeof(double) * (size_t)p->rblocks * 3 * M));
        GP_TRY(get((void**)&p->coli, sizeof(uint32_t) * (size_t)p->rblocks * M));
        GP_TRY(get((void**)&p->colc, sizeof(uint32_t) * (size_t)p->rblocks * M * OFIT_MAXC));
        GP_TRY(get((void**)&p->unit_d, sizeof(double) * 3 * M));
        GP_TRY(get((void**)&p->unit_i, sizeof(uint64_t) * 3 * M));
        GP_TRY(get((void**)&p->rep, N * M));
        GP_TRY(get((void**)&p->last_delta, sizeof(double) * U));
        GP_TRY(get((void**)&p->last_score, sizeof(int64_t) * U));
        GP_TRY(get((void**)&p->last_counts, sizeof(int64_t) * M * (size_t)C));
        uint64_t* units = p->block + p->L.units;
        hipLaunchKernelGGL(ofit_observed_kernel, dim3((unsigned)((n + m + OFIT_THREADS - 1) / OFIT_THREADS)), dim3(OFIT_THREADS), 0, st,
                           cat, n, m, C, p->L.stride, units, p->block + p->L.cats);
        GP_HIP(hipGetLastError());
        hipLaunchKernelGGL(ofit_observed_total_kernel, dim3(1), dim3(64), 0, st, n, m, p->L.stride, units);
        GP_HIP(hipGetLastError());
    }
    if (parts & GPIRT_OFIT_WAIC) {
        hipLaunchKernelGGL(ofit_mark_missing_kernel, dim3(ofit_grid_for(n * m)), dim3(OFIT_THREADS), 0, st, cat, n * m,
                           reinterpret_cast<double*>(p->block) + p->L.m2);
        GP_HIP(hipGetLastError());
    }
    p->on = true;
    return ofit_seal(st, p);
}

int launch_ofit_accumulate(hipStream_t st, OfitState* p, const double* f, const double* mu, const int8_t* cat, const double* thr,
                           uint64_t seed, uint32_t iter)
{
    OfitArgs a{};
    double* blk = reinterpret_cast<double*>(p->block);
    a.f = f; a.mu = mu; a.cat = cat; a.thr = thr; a.n = p->n; a.m = p->m; a.C = p->C;
    a.first = p->draws == 0 ? 1 : 0; a.draw = (double)(p->draws + 1);
    a.seed = seed; a.iter = iter; a.item0 = (uint32_t)p->item0;
    if (p->parts & GPIRT_OFIT_WAIC) { a.lse = blk + p->L.lse; a.mean = blk + p->L.mean; a.m2 = blk + p->L.m2; }
    if (p->parts & GPIRT_OFIT_PRED) a.pred = blk + p->L.pred;
    a.rowd = p->rowd; a.rowi = p->rowi; a.cold = p->cold; a.coli = p->coli; a.colc = p->colc; a.rep = p->rep;
    const dim3 grid((unsigned)p->rblocks, (unsigned)p->strips), block(OFIT_THREADS);
    switch (p->parts) {
        case 1: hipLaunchKernelGGL((ofit_cell_kernel<true, false, false>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((ofit_cell_kernel<false, true, false>), grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL((ofit_cell_kernel<true, true, false>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((ofit_cell_kernel<false, false, true>), grid, block, 0, st, a); break;
        case 5: hipLaunchKernelGGL((ofit_cell_kernel<true, false, true>), grid, block, 0, st, a); break;
        case 6: hipLaunchKernelGGL((ofit_cell_kernel<false, true, true>), grid, block, 0, st, a); break;
        case 7: hipLaunchKernelGGL((ofit_cell_kernel<true, true, true>), grid, block, 0, st, a); break;
        default: set_error("ordinal fit: parts = %d", p->parts); return GPIRT_E_ARG;
    }
    GP_HIP(hipGetLastError());
    if (p->parts & GPIRT_OFIT_PPC) {
        OfitUnitArgs u{};
        u.rowd = p->rowd; u.rowi = p->rowi; u.cold = p->cold; u.coli = p->coli; u.colc = p->colc;
        u.n = p->n; u.m = p->m; u.stride = p->L.stride; u.C = p->C; u.strips = p->strips; u.rblocks = p->rblocks;
        u.units = p->block + p->L.units; u.cats = p->block + p->L.cats; u.unit_d = p->unit_d; u.unit_i = p->unit_i;
        u.last_delta = p->last_delta; u.last_score = p->last_score; u.last_counts = p->last_counts;
        hipLaunchKernelGGL(ofit_units_kernel, dim3((unsigned)((p->n + p->m + OFIT_THREADS - 1) / OFIT_THREADS)), dim3(OFIT_THREADS), 0, st, u);
        GP_HIP(hipGetLastError());
        hipLaunchKernelGGL(ofit_total_kernel, dim3(1), dim3(OFIT_THREADS), 0, st, u);
        GP_HIP(hipGetLastError());
    }
    p->draws += 1;
    return 0;
}

// one raw accumulator of a state block on the device, by name
int ofit_block_get(hipStream_t st, const void* d_block, const char* name, void* h_out, int64_t bytes)
{
    int64_t hdr[OFIT_HEADER_WORDS];
    GP_TRY(ofit_read_header(st, d_block, hdr, "gpirt_ordinal_fit_get", 0));
    const int64_t n = hdr[2], m = hdr[3];
    const int C = (int)hdr[4], parts = (int)hdr[5];
    const OfitLayout L = ofit_layout(n, m, C, parts);
    const uint64_t* blk = static_cast<const uint64_t*>(d_block);
    int64_t off = -1, want = 0;
    const char* part = nullptr;
    int need = 0;
    if (strcmp(name, "draws") == 0) {
        if (bytes != 8) { set_error("ordinal fit: 'draws' holds 8 bytes, %lld were asked for", (long long)bytes); return GPIRT_E_ARG; }
        memcpy(h_out, &hdr[6], 8);
        return 0;
    }
    if (strcmp(name, "lse") == 0) { off = L.lse; want = 8 * L.cells; part = "waic"; need = GPIRT_OFIT_WAIC; }
    else if (strcmp(name, "ll_mean") == 0) { off = L.mean; want = 8 * L.cells; part = "waic"; need = GPIRT_OFIT_WAIC; }
    else if (strcmp(name, "ll_m2") == 0) { off = L.m2; want = 8 * L.cells; part = "waic"; need = GPIRT_OFIT_WAIC; }
    else if (strcmp(name, "pred_sum") == 0) { off = L.pred; want = 8 * (int64_t)(C - 1) * L.cells; part = "pred"; need = GPIRT_OFIT_PRED; }
    else {
        const bool item = strncmp(name, "item_", 5) == 0, resp = strncmp(name, "respondent_", 11) == 0, tot = strncmp(name, "total_", 6) == 0;
        const bool cat = strncmp(name, "cat_", 4) == 0;
        part = "ppc"; need = GPIRT_OFIT_PPC;
        if (item || resp || tot) {
            const char* fld = name + (item ? 5 : resp ? 11 : 6);
            for (int k = 0; k < OFIT_NUNIT; ++k)
                if (strcmp(kUnitNames[k], fld) == 0) {
                    off = (parts & GPIRT_OFIT_PPC) ? L.units + (int64_t)k * L.stride + (item ? 0 : resp ? m : m + n) : -1;
                    want = 8 * (item ? m : resp ? n : 1);
                }
        } else if (cat) {
            for (int k = 0; k < OFIT_NCAT; ++k)
                if (strcmp(kCatNames[k], name + 4) == 0) {
                    off = (parts & GPIRT_OFIT_PPC) ? L.cats + (int64_t)k * m * C : -1;
                    want = 8 * m * C;
                }
        }
        if (want == 0) { set_error("unknown ordinal fit array '%s'", name); return GPIRT_E_ARG; }
    }
    if (!(parts & need)) {
        set_error("ordinal fit: '%s' belongs to the %s part, which is not enabled (parts = %d)", name, part, parts);
        return GPIRT_E_ARG;
    }
    if (bytes != want) { set_error("ordinal fit: '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes); return GPIRT_E_ARG; }
    GP_HIP(hipMemcpyAsync(h_out, blk + off, (size_t)want, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

// the last counted draw of a sampler's state: "rep", "delta", "score", "counts_rep"; 1 if the name is none of them
int ofit_last_get(hipStream_t st, OfitState* p, const char* name, void* h_out, int64_t bytes)
{
    const void* dev = nullptr;
    int64_t want = 0;
    const int64_t U = p->n + p->m + 1;
    if (strcmp(name, "rep") == 0) { dev = p->rep; want = p->n * p->m; }
    else if (strcmp(name, "delta") == 0) { dev = p->last_delta; want = 8 * U; }
    else if (strcmp(name, "score") == 0) { dev = p->last_score; want = 8 * U; }
    else if (strcmp(name, "counts_rep") == 0) { dev = p->last_counts; want = 8 * p->m * p->C; }
    else return 1;
    if (!(p->parts & GPIRT_OFIT_PPC)) {
        set_error("ordinal fit: '%s' belongs to the ppc part, which is not enabled (parts = %d)", name, p->parts);
        return GPIRT_E_ARG;
    }
    if (bytes != want) { set_error("ordinal fit: '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes); return GPIRT_E_ARG; }
    GP_HIP(hipMemcpyAsync(h_out, dev, (size_t)want, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

// the totals of a state block on the device (one chain's or a pooled one)
int ofit_block_totals(hipStream_t st, const void* d_block, gpirt_ordinal_fit* out)
{
    int64_t hdr[OFIT_HEADER_WORDS];
    GP_TRY(ofit_read_header(st, d_block, hdr, "gpirt_ordinal_fit_totals", 0));
    for (int64_t r : out->reserved)
        if (r) { set_error("gpirt_ordinal_fit: reserved words must be 0"); return GPIRT_E_ARG; }
    const double nan = (double)NAN;
    const int64_t n = hdr[2], m = hdr[3];
    const int C = (int)hdr[4], parts = (int)hdr[5];
    const OfitLayout L = ofit_layout(n, m, C, parts);
    out->n = n; out->m = m; out->categories = C; out->parts = parts; out->draws = hdr[6]; out->n_obs = 0;
    out->lppd = out->p_waic = out->elpd_waic = out->waic = out->se_elpd_waic = nan;
    if (parts & GPIRT_OFIT_WAIC) {
        double *part = nullptr, *tot = nullptr;
        GP_HIP(hipMalloc((void**)&part, sizeof(double) * OFIT_TOTAL_BLOCKS * 4));
        if (hipMalloc((void**)&tot, sizeof(double) * 8) != hipSuccess) { hipFree(part); set_error("ordinal fit: hipMalloc failed"); return GPIRT_E_ALLOC; }
        hipMemsetAsync(tot, 0, sizeof(double) * 8, st);
        const double* blk = static_cast<const double*>(d_block);
        const int rc = ofit_waic_totals(st, blk + L.lse, blk + L.m2, L.cells, hdr[6], part, tot, out);
        hipFree(part); hipFree(tot);
        GP_TRY(rc);
    } else if (parts & GPIRT_OFIT_PPC) {
        uint64_t nobs = 0;
        GP_HIP(hipMemcpyAsync(&nobs, static_cast<const uint64_t*>(d_block) + L.units + OFIT_U_N_OBS * L.stride + m + n, 8, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        out->n_obs = (int64_t)nobs;
    }
    return 0;
}

int ofit_combine(gpirt_handle_t h, const void* const* d_states, int chains, void* d_out)
{
    GP_ARG(h && chains >= 1 && d_states && d_out);
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    hipStream_t st = h->stream;
    int64_t h0[OFIT_HEADER_WORDS], hc[OFIT_HEADER_WORDS];
    GP_TRY(ofit_read_header(st, d_states[0], h0, "gpirt_ordinal_fit_combine", 0));
    const int64_t n = h0[2], m = h0[3];
    const int C = (int)h0[4], parts = (int)h0[5];
    const OfitLayout L = ofit_layout(n, m, C, parts);
    if (d_out != d_states[0]) GP_HIP(hipMemcpyAsync(d_out, d_states[0], sizeof(uint64_t) * (size_t)L.words, hipMemcpyDeviceToDevice, st));
    uint64_t* po = static_cast<uint64_t*>(d_out);
    double* pd = static_cast<double*>(d_out);
    int64_t draws = h0[6];
    for (int c = 1; c < chains; ++c) {
        GP_TRY(ofit_read_header(st, d_states[c], hc, "gpirt_ordinal_fit_combine", c));
        if (hc[2] != n || hc[3] != m || hc[4] != C || hc[5] != parts || hc[7] != h0[7]) {
            set_error("gpirt_ordinal_fit_combine: state %d has another n, m, C, parts or item0 than state 0", c);
            return GPIRT_E_ARG;
        }
        const uint64_t* pu = static_cast<const uint64_t*>(d_states[c]);
        const double* pb = static_cast<const double*>(d_states[c]);
        if (parts & GPIRT_OFIT_WAIC)
            hipLaunchKernelGGL(ofit_pool_waic_kernel, dim3(ofit_grid_for(L.cells)), dim3(OFIT_THREADS), 0, st, pd + L.lse, pd + L.mean,
                               pd + L.m2, pb + L.lse, pb + L.mean, pb + L.m2, L.cells, (double)draws, (double)hc[6]);
        if (parts & GPIRT_OFIT_PRED)
            hipLaunchKernelGGL(ofit_pool_add_f64_kernel, dim3(ofit_grid_for((C - 1) * L.cells)), dim3(OFIT_THREADS), 0, st, pd + L.pred,
                               pb + L.pred, (int64_t)(C - 1) * L.cells);
        if (parts & GPIRT_OFIT_PPC) {
            // the counts from score_ge to nonfinite, the two deviance sums in chain order; n_obs, obs_score and obs_count are the data's
            const int64_t i0 = L.units + (int64_t)OFIT_U_SCORE_GE * L.stride, ni = (int64_t)(OFIT_U_NONFINITE - OFIT_U_SCORE_GE + 1) * L.stride;
            hipLaunchKernelGGL(ofit_pool_add_u64_kernel, dim3(ofit_grid_for(ni)), dim3(OFIT_THREADS), 0, st, po + i0, pu + i0, ni);
            const int64_t d0 = L.units + (int64_t)OFIT_U_DEV_OBS * L.stride, nd = 2 * L.stride;
            hipLaunchKernelGGL(ofit_pool_add_f64_kernel, dim3(ofit_grid_for(nd)), dim3(OFIT_THREADS), 0, st, pd + d0, pb + d0, nd);
            const int64_t k0 = L.cats + (int64_t)OFIT_K_REP_SUM * m * C, nk = (int64_t)(OFIT_NCAT - 1) * m * C;
            hipLaunchKernelGGL(ofit_pool_add_u64_kernel, dim3(ofit_grid_for(nk)), dim3(OFIT_THREADS), 0, st, po + k0, pu + k0, nk);
        }
        GP_HIP(hipGetLastError());
        draws += hc[6];
    }
    h0[6] = draws;
    GP_HIP(hipMemcpyAsync(d_out, h0, sizeof(h0), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace gpirt
