// groups.hip -- group posteriors (include/gpirt_hip.h, "group posteriors"): the respondents come in
// groups, and per counted draw the device forms joint functionals of the groups -- how far apart they lie on theta, how much they
// overlap, who their medians are, on which items they take opposite sides and who votes least with their own group.
//
// Part A (theta alone, exact integers up to the fp64 statistics):
//   grp_hist_kernel     the (G + 1) x 1001 histogram by integer LDS atomics, flushed by integer global atomics; the off-grid word
//   grp_latent_kernel   ONE work-group: a wave per row scans the row into its prefix sums and folds c1, c2 and med2; a wave per pair
//                       sums U2 and ov over k (integers, wave shuffles); one thread per pair and per row owns the fp64 statistics
//                       and their accumulators
//   grp_share_kernel    one thread per respondent: the median shares from the prefix sums; one thread per cell of the density
//                       accumulators
// Part B (the n x m pass, twice over f and mu, once over y):
//   grp_votes_kernel    GV_ROWS respondents x GV_STRIP items per work-group, lanes along i, a strip's loads before its arithmetic,
//                       rint(p 2^44) into a (copy, item, group) table in LDS by integer atomics, one 64-bit integer global atomic
//                       per occupied entry
//   grp_items_kernel    one thread per (group, item) -- side, support, rice -- and per (pair, item) -- gap, split --, each with its
//                       accumulators; n_split by integer atomics, one per wave
//   grp_loyalty_kernel  256 respondents x GL_COLS items per work-group with the items' flags in LDS (contested = any pair's split;
//                       the first row of work-groups stores it and counts c_g, one integer atomic per strip and group); a
//                       lane's terms in a register, one 64-bit integer global atomic per (respondent, strip); uncontested
//                       items are never loaded
//   grp_loy_update_kernel  one thread per respondent: the draw's loyalty and the observed counts into their accumulators
// Both skip words are complete before any kernel that touches an accumulator runs.  Every accumulator cell has one owner; there
// is no floating-point atomic, and every integer sum is independent of the order of arrival: the state is byte-identical from
// run to run.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace gpirt {

namespace {

constexpr int GR_THREADS = 256;
constexpr int GR_MAXG = GPIRT_GROUPS_MAX_G;
constexpr int GR_MAXP = GR_MAXG * (GR_MAXG - 1) / 2;
constexpr int GR_K = GPIRT_NGRID;                  // 1001 grid points
constexpr int GR_KP = GR_K + 1;                    // a row of prefix sums: less[k], k = 0 .. 1001 (the last one is n_g)
constexpr int GR_CENTRE = (GPIRT_NGRID - 1) / 2;
constexpr int GR_SUB = 4;                          // row sub-blocks of a work-group of the histogram and the votes kernel
constexpr int GV_ROWS = GR_THREADS * GR_SUB;
constexpr int GV_STRIP = 8;                        // items per work-group of grp_votes_kernel
constexpr int GV_COPIES = 8;                       // copies of the LDS table, by lane & 7: an eighth of the same-address adds
constexpr int GL_COLS = 32;                        // items per work-group of grp_loyalty_kernel
constexpr double GR_FIX = 17592186044416.0;        // 2^44
static_assert(GR_K == 1001 && GR_K <= 64 * 16, "a lane of the scanning wave owns 16 grid points");
static_assert((int64_t)GPIRT_GROUPS_MAX_N * (int64_t)(1ll << 44) < (1ll << 60), "e stays below 2^60");
static_assert(GPIRT_GROUPS_MAX_M <= 0xFFFF, "obs_with and obs_n share a 32-bit word");
static_assert(GR_MAXP <= 64 && 64 + GR_MAXG + 1 <= GR_THREADS, "the owners of grp_latent_kernel and grp_loy_update_kernel");

const char* const kGrpRaw[GPIRT_GROUPS_NARRAYS] = {
    "dens_sum", "dens_sq", "medhist", "order", "ov_sum", "d_undefined", "mean_sum", "mean_sq", "sd_sum", "sd_sq", "a_sum", "a_sq",
    "ovl_sum", "ovl_sq", "d_sum", "d_sq", "median_cover", "median_share", "split_count", "nsplit_sum", "nsplit_sq", "support_sum",
    "support_sq", "rice_sum", "rice_sq", "gap_sum", "gap_sq", "loy_sum", "loy_sq", "loy_undefined", "obs_with_sum", "obs_n_sum" };

inline int64_t grp_pairs(int64_t G) { return G * (G - 1) / 2; }
inline int grp_raw_width(int k)
{
    return (k == GPIRT_GROUPS_MEDHIST || k == GPIRT_GROUPS_ORDER || k == GPIRT_GROUPS_D_UNDEFINED || k == GPIRT_GROUPS_MEDIAN_COVER ||
            k == GPIRT_GROUPS_SPLIT_COUNT || k == GPIRT_GROUPS_LOY_UNDEFINED) ? 4 : 8;
}
inline bool grp_raw_double(int k)
{
    return (k >= GPIRT_GROUPS_MEAN_SUM && k <= GPIRT_GROUPS_D_SQ) || k == GPIRT_GROUPS_MEDIAN_SHARE ||
           (k >= GPIRT_GROUPS_SUPPORT_SUM && k <= GPIRT_GROUPS_LOY_SQ);
}
inline int64_t grp_raw_count(int k, int64_t n, int64_t m, int64_t G)
{
    const int64_t P = grp_pairs(G), G1 = G + 1;
    switch (k) {
        case GPIRT_GROUPS_DENS_SUM: case GPIRT_GROUPS_DENS_SQ: return G1 * GR_K;
        case GPIRT_GROUPS_MEDHIST: return G1 * GPIRT_GROUPS_MED_BINS;
        case GPIRT_GROUPS_ORDER: return 6 * P;
        case GPIRT_GROUPS_MEAN_SUM: case GPIRT_GROUPS_MEAN_SQ: case GPIRT_GROUPS_SD_SUM: case GPIRT_GROUPS_SD_SQ: return G1;
        case GPIRT_GROUPS_MEDIAN_COVER: case GPIRT_GROUPS_MEDIAN_SHARE: case GPIRT_GROUPS_LOY_SUM: case GPIRT_GROUPS_LOY_SQ:
        case GPIRT_GROUPS_OBS_WITH_SUM: case GPIRT_GROUPS_OBS_N_SUM: return n;
        case GPIRT_GROUPS_SPLIT_COUNT: case GPIRT_GROUPS_GAP_SUM: case GPIRT_GROUPS_GAP_SQ: return P * m;
        case GPIRT_GROUPS_SUPPORT_SUM: case GPIRT_GROUPS_SUPPORT_SQ: case GPIRT_GROUPS_RICE_SUM: case GPIRT_GROUPS_RICE_SQ: return G * m;
        case GPIRT_GROUPS_LOY_UNDEFINED: return G;
        default: return P;
    }
}

struct GrpSizes { int64_t n[GR_MAXG + 1]; };

// ---- part A ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GR_THREADS) void grp_hist_kernel(const double* __restrict__ theta, const signed char* __restrict__ grp,
                                                              int64_t n, int G, uint32_t* __restrict__ hist, int* __restrict__ ctl)
{
    __shared__ uint32_t sh[(GR_MAXG + 1) * GR_K];
    const int t = threadIdx.x, cells = (G + 1) * GR_K;
    for (int k = t; k < cells; k += GR_THREADS) sh[k] = 0;
    __syncthreads();
    for (int sub = 0; sub < GR_SUB; ++sub) {
        const int64_t i = ((int64_t)blockIdx.x * GR_SUB + sub) * GR_THREADS + t;
        const int g = i < n ? grp[i] : -1;
        if (g < 0 || g >= G) continue;               // left out: theta is never read
        const int k = grid_index(theta[i]);
        if (k < 0) { ctl[0] = 1; continue; }         // (every writer stores the same word)
        atomicAdd(&sh[g * GR_K + k], 1u);
        atomicAdd(&sh[G * GR_K + k], 1u);
    }
    __syncthreads();
    for (int k = t; k < cells; k += GR_THREADS) {
        const uint32_t v = sh[k];
        if (v) atomicAdd(&hist[k], v);
    }
}

struct GrpLatentArgs {
    const uint32_t* hist;                          // the draw's [G + 1][1001]
    uint32_t* less;                                // out: [G + 1][1002]
    const int* ctl;
    int64_t* hdr;
    GrpSizes sz;
    int G;
    uint64_t* ov_sum;
    uint32_t *medhist, *order, *d_undef;
    double *mean_sum, *mean_sq, *sd_sum, *sd_sq, *a_sum, *a_sq, *ovl_sum, *ovl_sq, *d_sum, *d_sq;
    int64_t* lat_last;                             // c1, c2, med2 (G + 1 each), w, ov (P each)
    double* stat_last;                             // mean, var, sd (G + 1 each), a, overlap, d (P each)
};

__device__ __forceinline__ void grp_moments(int64_t c1, int64_t c2, int64_t ng, double* mean, double* var)
{
    *mean = (double)c1 / (double)ng;
    *var = (double)(ng * c2 - c1 * c1) / (double)(ng * ng);
}

__global__ __launch_bounds__(GR_THREADS) void grp_latent_kernel(GrpLatentArgs a)
{
    __shared__ uint32_t less[(GR_MAXG + 1) * GR_KP];
    __shared__ int64_t c1[GR_MAXG + 1], c2[GR_MAXG + 1], med2[GR_MAXG + 1];
    __shared__ unsigned long long red[GR_MAXP][2];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, G = a.G, G1 = G + 1, P = G * (G - 1) / 2;
    if (a.ctl[0] != 0) {                              // (the same for every thread) skipped whole: nothing is touched
        if (t == 0) a.hdr[6] += 1;
        return;
    }
    for (int g = wv; g < G1; g += GR_THREADS / 64) {
        const int64_t ng = a.sz.n[g];
        const uint32_t q1 = (uint32_t)((ng + 1) / 2), q2 = (uint32_t)(ng / 2 + 1);
        uint32_t h[16], s = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = lane * 16 + q;
            h[q] = k < GR_K ? a.hist[g * GR_K + k] : 0u;
            s += h[q];
        }
        uint32_t inc = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = __shfl_up(inc, off, 64);
            if (lane >= off) inc += v;
        }
        uint32_t run = inc - s;
        long long s1 = 0, s2 = 0, md = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int k = lane * 16 + q;
            if (k <= GR_K) { less[g * GR_KP + k] = run; a.less[g * GR_KP + k] = run; }
            if (k < GR_K && h[q]) {
                const long long tt = k - GR_CENTRE;
                s1 += tt * (long long)h[q];
                s2 += tt * tt * (long long)h[q];
                if (run < q1 && q1 <= run + h[q]) md += k;
                if (run < q2 && q2 <= run + h[q]) md += k;
            }
            run += h[q];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s1 += __shfl_down(s1, off, 64);
            s2 += __shfl_down(s2, off, 64);
            md += __shfl_down(md, off, 64);
        }
        if (lane == 0) { c1[g] = s1; c2[g] = s2; med2[g] = md; }
    }
    __syncthreads();
    {
        int p = 0;
        for (int g = 0; g < G; ++g)
            for (int h = g + 1; h < G; ++h, ++p) {
                if ((p & (GR_THREADS / 64 - 1)) != wv) continue;          // a wave owns whole pairs: no sum across waves
                const unsigned long long ng = (unsigned long long)a.sz.n[g], nh = (unsigned long long)a.sz.n[h];
                unsigned long long u2 = 0, ov = 0;
                for (int k = lane; k < GR_K; k += 64) {
                    const unsigned long long Hg = less[g * GR_KP + k + 1] - less[g * GR_KP + k];
                    const unsigned long long Hh = less[h * GR_KP + k + 1] - less[h * GR_KP + k];
                    u2 += Hg * (2ull * less[h * GR_KP + k] + Hh);
                    const unsigned long long x = Hg * nh, y = Hh * ng;
                    ov += x < y ? x : y;
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    u2 += __shfl_down(u2, off, 64);
                    ov += __shfl_down(ov, off, 64);
                }
                if (lane == 0) { red[p][0] = u2; red[p][1] = ov; }
            }
    }
    __syncthreads();
    if (t < P) {
        int g = 0, h = 0, p = 0;
        for (int gg = 0; gg < G; ++gg)
            for (int hh = gg + 1; hh < G; ++hh, ++p)
                if (p == t) { g = gg; h = hh; }
        const int64_t ng = a.sz.n[g], nh = a.sz.n[h];
        const unsigned long long u2 = red[t][0], ov = red[t][1];
        const int64_t w = (int64_t)u2 - ng * nh;
        const int64_t lhs = c1[g] * nh, rhs = c1[h] * ng;
        a.order[(lhs > rhs ? 0 : lhs == rhs ? 1 : 2) * P + t] += 1u;
        a.order[(med2[g] > med2[h] ? 3 : med2[g] == med2[h] ? 4 : 5) * P + t] += 1u;
        a.ov_sum[t] += ov;
        double mg, vg, mh, vh;
        grp_moments(c1[g], c2[g], ng, &mg, &vg);
        grp_moments(c1[h], c2[h], nh, &mh, &vh);
        const double nn = (double)(ng * nh);
        const double av = (double)w / nn, ol = (double)(int64_t)ov / nn;
        a.a_sum[t] += av; a.a_sq[t] += av * av;
        a.ovl_sum[t] += ol; a.ovl_sq[t] += ol * ol;
        const double pooled = ((double)ng * vg + (double)nh * vh) / ((double)ng + (double)nh);
        double d = __longlong_as_double(0x7ff8000000000000LL);
        if (pooled == 0.0) a.d_undef[t] += 1u;
        else {
            d = (mg - mh) / sqrt(pooled);
            a.d_sum[t] += d; a.d_sq[t] += d * d;
        }
        a.lat_last[3 * G1 + t] = w; a.lat_last[3 * G1 + P + t] = (int64_t)ov;
        a.stat_last[3 * G1 + t] = av; a.stat_last[3 * G1 + P + t] = ol; a.stat_last[3 * G1 + 2 * P + t] = d;
    }
    if (t >= 64 && t < 64 + G1) {
        const int g = t - 64;
        double mean, var;
        grp_moments(c1[g], c2[g], a.sz.n[g], &mean, &var);
        const double sd = sqrt(var);
        a.mean_sum[g] += mean; a.mean_sq[g] += mean * mean;
        a.sd_sum[g] += sd; a.sd_sq[g] += sd * sd;
        a.medhist[(int64_t)g * GPIRT_GROUPS_MED_BINS + med2[g]] += 1u;
        a.lat_last[g] = c1[g]; a.lat_last[G1 + g] = c2[g]; a.lat_last[2 * G1 + g] = med2[g];
        a.stat_last[g] = mean; a.stat_last[G1 + g] = var; a.stat_last[2 * G1 + g] = sd;
    }
    if (t == 0) a.hdr[5] += 1;
}

__global__ __launch_bounds__(GR_THREADS) void grp_share_kernel(const double* __restrict__ theta, const signed char* __restrict__ grp,
                                                               int64_t n, int G, const uint32_t* __restrict__ less, GrpSizes sz,
                                                               const int* __restrict__ ctl, uint32_t* __restrict__ cover,
                                                               double* __restrict__ share, uint64_t* __restrict__ dens_sum,
                                                               uint64_t* __restrict__ dens_sq, uint32_t* __restrict__ hist_last)
{
    const int64_t i = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x;
    if (ctl[0] != 0) return;                         // (the same for every thread)
    if (i < (int64_t)(G + 1) * GR_K) {               // thread e owns cell e of the density accumulators
        const int g = (int)(i / GR_K), k = (int)(i - (int64_t)g * GR_K);
        const unsigned long long H = less[g * GR_KP + k + 1] - less[g * GR_KP + k];
        dens_sum[i] += H;
        dens_sq[i] += H * H;
        hist_last[i] = (uint32_t)H;
    }
    if (i >= n) return;
    const int g = grp[i];
    if (g < 0 || g >= G) return;
    const int k = grid_index(theta[i]);
    if (k < 0) return;                               // (cannot be: the draw would have been skipped)
    const uint32_t ls = less[g * GR_KP + k], eq = less[g * GR_KP + k + 1] - ls;
    const uint32_t q1 = (uint32_t)((sz.n[g] + 1) / 2), q2 = (uint32_t)(sz.n[g] / 2 + 1);
    const int c = ((ls < q1 && q1 <= ls + eq) ? 1 : 0) + ((ls < q2 && q2 <= ls + eq) ? 1 : 0);
    if (c == 0) return;
    cover[i] += 1u;
    share[i] += (double)c / (double)(2u * eq);
}

// ---- part B ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GR_THREADS) void grp_votes_kernel(const double* __restrict__ f, const double* __restrict__ mu,
                                                               int64_t n, int64_t m, const signed char* __restrict__ grp, int G,
                                                               unsigned long long* __restrict__ e, int* __restrict__ bad)
{
    __shared__ unsigned long long sc[GV_COPIES][GV_STRIP][GR_MAXG];
    const int t = threadIdx.x, cp = t & (GV_COPIES - 1);
    for (int k = t; k < GV_COPIES * GV_STRIP * GR_MAXG; k += GR_THREADS) (&sc[0][0][0])[k] = 0ull;
    __syncthreads();
    const int64_t j0 = (int64_t)blockIdx.y * GV_STRIP;
    const int w = (int)(m - j0 < GV_STRIP ? m - j0 : GV_STRIP);
    for (int sub = 0; sub < GR_SUB; ++sub) {
        const int64_t i = ((int64_t)blockIdx.x * GR_SUB + sub) * GR_THREADS + t;
        const int g = i < n ? grp[i] : -1;
        if (g < 0 || g >= G) continue;               // (no barrier inside this loop)
        double gv[GV_STRIP];
#pragma unroll
        for (int jj = 0; jj < GV_STRIP; ++jj) {
            gv[jj] = 0.0;
            if (jj < w) {
                const int64_t at = i + (j0 + jj) * n;
                gv[jj] = f[at] + mu[at];
            }
        }
#pragma unroll
        for (int jj = 0; jj < GV_STRIP; ++jj) {
            if (jj >= w) continue;
            const double x = gv[jj];
            if (!(x == x)) { *bad = 1; continue; }   // (every writer stores the same word)
            const double ex = exp(-fabs(x));
            const double p = x >= 0.0 ? 1.0 / (1.0 + ex) : ex / (1.0 + ex);
            atomicAdd(&sc[cp][jj][g], (unsigned long long)rint(p * GR_FIX));
        }
    }
    __syncthreads();
    for (int k = t; k < w * G; k += GR_THREADS) {
        const int jj = k / G, g = k - jj * G;
        unsigned long long v = 0;
#pragma unroll
        for (int c = 0; c < GV_COPIES; ++c) v += sc[c][jj][g];
        if (v) atomicAdd(&e[(int64_t)g * m + j0 + jj], v);
    }
}

struct GrpItemArgs {
    const uint64_t* e;
    const int* ctl;
    int64_t* hdr;
    GrpSizes sz;
    int64_t m;
    int G;
    uint32_t* cnt;                                  // the draw's n_split [P], then c_g [G]
    uint32_t* split_count;
    double *support_sum, *support_sq, *rice_sum, *rice_sq, *gap_sum, *gap_sq;
    uint64_t* e_last;
    signed char* flags;                             // side [G][m], split [P][m]; grp_loyalty_kernel adds contested [m]
};

// the item's side and support of group g from e: what the group's owner and every pair's owner of the item form alike
__device__ __forceinline__ void grp_side(uint64_t ev, int64_t ng, int* sd, double* s)
{
    const int64_t diff = (int64_t)(2 * ev) - (ng << 44);
    *sd = diff > 0 ? 1 : diff < 0 ? -1 : 0;
    *s = (double)ev / ((double)ng * GR_FIX);
}

// blockIdx.y < G: thread j owns (group, item) -- side, support, rice; else (pair, item) -- gap, split and the pair's n_split
__global__ __launch_bounds__(GR_THREADS) void grp_items_kernel(GrpItemArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, G = a.G, role = blockIdx.y;
    const int64_t m = a.m;
    if (a.ctl[1] != 0) {                             // (the same for every thread) skipped whole: nothing is touched
        if (j == 0 && role == 0) a.hdr[8] += 1;
        return;
    }
    const bool live = j < m;
    if (role < G) {
        if (!live) return;
        const int64_t at = (int64_t)role * m + j;
        const uint64_t ev = a.e[at];
        int sd;
        double s;
        grp_side(ev, a.sz.n[role], &sd, &s);
        const double rice = fabs(2.0 * s - 1.0);
        a.support_sum[at] += s; a.support_sq[at] += s * s;
        a.rice_sum[at] += rice; a.rice_sq[at] += rice * rice;
        a.e_last[at] = ev;
        a.flags[at] = (signed char)sd;
        return;
    }
    const int p = role - G;
    int g = 0, h = 0, q = 0;
    for (int gg = 0; gg < G; ++gg)
        for (int hh = gg + 1; hh < G; ++hh, ++q)
            if (q == p) { g = gg; h = hh; }
    bool split = false;
    if (live) {
        int sg, sh;
        double s0, s1;
        grp_side(a.e[(int64_t)g * m + j], a.sz.n[g], &sg, &s0);
        grp_side(a.e[(int64_t)h * m + j], a.sz.n[h], &sh, &s1);
        split = sg * sh == -1;
        const int64_t at = (int64_t)p * m + j;
        const double gap = s0 - s1;
        a.gap_sum[at] += gap; a.gap_sq[at] += gap * gap;
        a.split_count[at] += split ? 1u : 0u;
        a.flags[(int64_t)G * m + at] = split ? 1 : 0;
    }
    const unsigned long long b = __ballot(split);
    if (lane == 0 && b) atomicAdd(&a.cnt[p], (uint32_t)__popcll(b));
}

// work-groups with blockIdx.x == 0 also own their strip's contested flags and its part of c_g
__global__ __launch_bounds__(GR_THREADS) void grp_loyalty_kernel(const double* __restrict__ f, const double* __restrict__ mu,
                                                                 const double* __restrict__ y, int64_t n, int64_t m,
                                                                 const signed char* __restrict__ grp, int G,
                                                                 signed char* __restrict__ flags, int P,
                                                                 const int* __restrict__ ctl, unsigned long long* __restrict__ loy,
                                                                 uint32_t* __restrict__ obs, uint32_t* __restrict__ cnt)
{
    __shared__ signed char sside[GL_COLS][GR_MAXG];
    __shared__ signed char scont[GL_COLS];
    if (ctl[1] != 0) return;                         // (the same for every thread)
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * GR_THREADS + t, j0 = (int64_t)blockIdx.y * GL_COLS;
    if (t < 64) {                                    // the first wave, whole: its ballots count c_g
        const int64_t j = j0 + t;
        const bool have = t < GL_COLS && j < m;
        bool cont = false;
        if (have) for (int p = 0; p < P; ++p) cont = cont || flags[(int64_t)(G + p) * m + j] != 0;
        if (t < GL_COLS) scont[t] = cont ? 1 : 0;
        if (have && blockIdx.x == 0) flags[(int64_t)(G + P) * m + j] = cont ? 1 : 0;
        for (int g = 0; g < GR_MAXG; ++g) {
            const signed char sd = (have && g < G) ? flags[(int64_t)g * m + j] : 0;
            if (t < GL_COLS) sside[t][g] = sd;
            if (blockIdx.x == 0 && g < G) {
                const unsigned long long b = __ballot(cont && sd != 0);
                if (t == 0 && b) atomicAdd(&cnt[P + g], (uint32_t)__popcll(b));
            }
        }
    }
    __syncthreads();
    const int g = i < n ? grp[i] : -1;
    if (g < 0 || g >= G) return;
    unsigned long long acc = 0;
    uint32_t ob = 0;
    for (int jj = 0; jj < GL_COLS; ++jj) {
        if (!scont[jj]) continue;                    // (uniform: an uncontested item is never loaded)
        const int sd = sside[jj][g];
        if (sd == 0) continue;
        const int64_t at = i + (j0 + jj) * n;
        const double x = f[at] + mu[at], yv = y[at];
        const double ex = exp(-fabs(x));
        const double p = x >= 0.0 ? 1.0 / (1.0 + ex) : ex / (1.0 + ex);
        const double q = x >= 0.0 ? ex / (1.0 + ex) : 1.0 / (1.0 + ex);
        acc += (unsigned long long)rint((sd > 0 ? p : q) * GR_FIX);
        if (yv == yv) ob += 0x10000u + (((yv > 0.0) == (sd > 0)) ? 1u : 0u);
    }
    if (acc) atomicAdd(&loy[i], acc);
    if (ob) atomicAdd(&obs[i], ob);
}

struct GrpLoyArgs {
    const signed char* grp;
    const int* ctl;
    int64_t* hdr;
    int64_t n;
    int G;
    const uint32_t* cnt;
    const uint64_t* loy;
    const uint32_t* obs;
    uint64_t *nsplit_sum, *nsplit_sq, *obs_with_sum, *obs_n_sum;
    uint32_t* loy_undef;
    double *loy_sum, *loy_sq;
    uint64_t* loy_last;
    uint32_t* obs_last;
    int64_t* cnt_last;
};

__global__ __launch_bounds__(GR_THREADS) void grp_loy_update_kernel(GrpLoyArgs a)
{
    if (a.ctl[1] != 0) return;                       // (the same for every thread; grp_items_kernel counted the skip)
    const int64_t i = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x;
    const int G = a.G, P = G * (G - 1) / 2;
    if (i == 0) a.hdr[7] += 1;
    if (i < P) {
        const uint64_t ns = a.cnt[i];
        a.nsplit_sum[i] += ns; a.nsplit_sq[i] += ns * ns;
        a.cnt_last[i] = (int64_t)ns;
    }
    if (i >= 64 && i < 64 + G) {
        const int g = (int)i - 64;
        const uint32_t c = a.cnt[P + g];
        a.cnt_last[P + g] = c;
        if (c == 0) a.loy_undef[g] += 1u;
    }
    if (i >= a.n) return;
    const int g = a.grp[i];
    if (g < 0 || g >= G) return;
    const uint64_t lv = a.loy[i];
    const uint32_t ob = a.obs[i];
    a.loy_last[i] = lv; a.obs_last[i] = ob;
    a.obs_with_sum[i] += ob & 0xFFFFu; a.obs_n_sum[i] += ob >> 16;
    const uint32_t c = a.cnt[P + g];
    if (c == 0) return;
    const double l = (double)lv / ((double)c * GR_FIX);
    a.loy_sum[i] += l; a.loy_sq[i] += l * l;
}

inline unsigned grp_grid(int64_t work, int64_t per = GR_THREADS) { return (unsigned)std::max<int64_t>((work + per - 1) / per, 1); }
inline size_t grp_pad(size_t bytes) { return (bytes + 15) / 16 * 16; }

// a state block on the host
struct HostGrp {
    std::vector<uint64_t> w;
    int64_t n = 0, m = 0, G = 0;
    GrpLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    const signed char* groups() const { return reinterpret_cast<const signed char*>(w.data() + L.groups); }
    template <class T> T* arr(int k) { return reinterpret_cast<T*>(w.data() + L.off[k]); }
    template <class T> const T* arr(int k) const { return reinterpret_cast<const T*>(w.data() + L.off[k]); }
};

int grp_read(hipStream_t st, const void* d_state, HostGrp& r, int c)
{
    int64_t hdr[GRP_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] != GRP_TAG || hdr[1] != GRP_LAYOUT_VERSION || hdr[2] < 1 || hdr[2] > GPIRT_GROUPS_MAX_N || hdr[3] < 1 ||
        hdr[3] > GPIRT_GROUPS_MAX_M || hdr[4] < 2 || hdr[4] > GPIRT_GROUPS_MAX_G) {
        set_error("gpirt_groups_combine: state %d is not a group posterior state block of layout %d", c, GRP_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[2]; r.m = hdr[3]; r.G = hdr[4];
    r.L = grp_layout(r.n, r.m, r.G);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

// theta -> -theta: the grid axes reversed, the odd sums negated, > and < swapped
void grp_reflect(HostGrp& r)
{
    const int64_t G1 = r.G + 1, P = grp_pairs(r.G);
    for (int64_t g = 0; g < G1; ++g) {
        for (int k : { GPIRT_GROUPS_DENS_SUM, GPIRT_GROUPS_DENS_SQ }) {
            uint64_t* row = r.arr<uint64_t>(k) + g * GR_K;
            std::reverse(row, row + GR_K);
        }
        uint32_t* row = r.arr<uint32_t>(GPIRT_GROUPS_MEDHIST) + g * GPIRT_GROUPS_MED_BINS;
        std::reverse(row, row + GPIRT_GROUPS_MED_BINS);
        double* ms = r.arr<double>(GPIRT_GROUPS_MEAN_SUM);
        ms[g] = -ms[g];
    }
    uint32_t* ord = r.arr<uint32_t>(GPIRT_GROUPS_ORDER);
    for (int64_t p = 0; p < P; ++p) {
        std::swap(ord[p], ord[2 * P + p]);
        std::swap(ord[3 * P + p], ord[5 * P + p]);
        double* as = r.arr<double>(GPIRT_GROUPS_A_SUM);
        double* ds = r.arr<double>(GPIRT_GROUPS_D_SUM);
        as[p] = -as[p]; ds[p] = -ds[p];
    }
}

}  // namespace

GrpLayout grp_layout(int64_t n, int64_t m, int64_t G)
{
    GrpLayout L{};
    int64_t at = GRP_HEADER_WORDS + GRP_SIZE_WORDS;
    L.groups = at;
    at += (n + 15) / 16 * 2;
    for (int k = 0; k < GPIRT_GROUPS_NARRAYS; ++k) {
        L.off[k] = at;
        at += (grp_raw_count(k, n, m, G) * grp_raw_width(k) + 15) / 16 * 2;      // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int64_t groups_state_words(const GroupsState* s) { return grp_layout(s->n, s->m, s->G).words; }

int groups_check(int64_t n, int64_t m, int G, const int32_t* groups, int top, int64_t* sizes)
{
    if (n < 1 || n > GPIRT_GROUPS_MAX_N) {
        set_error("groups: n = %lld respondents, 1..%d are taken", (long long)n, GPIRT_GROUPS_MAX_N);
        return GPIRT_E_ARG;
    }
    if (m < 1 || m > GPIRT_GROUPS_MAX_M) {
        set_error("groups: m = %lld items, 1..%d are taken", (long long)m, GPIRT_GROUPS_MAX_M);
        return GPIRT_E_ARG;
    }
    if (G < 2 || G > GPIRT_GROUPS_MAX_G || !groups) {
        set_error("groups: %d groups given, 2..%d are taken", G, GPIRT_GROUPS_MAX_G);
        return GPIRT_E_ARG;
    }
    if (top < 1 || top > GPIRT_GROUPS_MAX_TOP) {
        set_error("groups: top = %d is outside 1..%d", top, GPIRT_GROUPS_MAX_TOP);
        return GPIRT_E_ARG;
    }
    int64_t cnt[GR_MAXG + 1] = {};
    for (int64_t i = 0; i < n; ++i) {
        if (groups[i] < -1 || groups[i] >= G) {
            set_error("groups: the code %d of respondent %lld is outside -1..%d", (int)groups[i], (long long)i, G - 1);
            return GPIRT_E_ARG;
        }
        if (groups[i] >= 0) { cnt[groups[i]] += 1; cnt[G] += 1; }
    }
    for (int g = 0; g < G; ++g)
        if (cnt[g] == 0) { set_error("groups: group %d has no member", g); return GPIRT_E_ARG; }
    if (sizes) for (int g = 0; g <= GR_MAXG; ++g) sizes[g] = cnt[g];
    return 0;
}

void groups_free(GroupsState* s)
{
    for (void* q : s->allocs) hipFree(q);
    *s = GroupsState{};
}

int groups_alloc(hipStream_t st, GroupsState* s, int64_t n, int64_t m, int G, const int32_t* groups, int top)
{
    GP_TRY(groups_check(n, m, G, groups, top, s->sizes));
    const int64_t P = grp_pairs(G), G1 = G + 1;
    const GrpLayout L = grp_layout(n, m, G);
    s->n = n; s->m = m; s->G = G; s->top = top;
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        s->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    GP_TRY(get((void**)&s->block, sizeof(uint64_t) * (size_t)L.words));
    // the draw's scratch in one piece (one memset per draw): ctl, cnt, hist, e, loy, obs
    const size_t b_ctl = 16, b_cnt = grp_pad(4 * (size_t)(P + G)), b_hist = grp_pad(4 * (size_t)(G1 * GR_K)),
                 b_e = grp_pad(8 * (size_t)(G * m)), b_loy = grp_pad(8 * (size_t)n), b_obs = grp_pad(4 * (size_t)n);
    char* sc = nullptr;
    GP_TRY(get((void**)&sc, b_ctl + b_cnt + b_hist + b_e + b_loy + b_obs));
    s->ctl = reinterpret_cast<int*>(sc); sc += b_ctl;
    s->cnt = reinterpret_cast<uint32_t*>(sc); sc += b_cnt;
    s->hist = reinterpret_cast<uint32_t*>(sc); sc += b_hist;
    s->e = reinterpret_cast<uint64_t*>(sc); sc += b_e;
    s->loy = reinterpret_cast<uint64_t*>(sc); sc += b_loy;
    s->obs = reinterpret_cast<uint32_t*>(sc);
    GP_TRY(get((void**)&s->less, 4 * (size_t)(G1 * GR_KP)));
    GP_TRY(get((void**)&s->hist_last, 4 * (size_t)(G1 * GR_K)));
    GP_TRY(get((void**)&s->lat_last, 8 * (size_t)(3 * G1 + 2 * P)));
    GP_TRY(get((void**)&s->stat_last, 8 * (size_t)(3 * G1 + 3 * P)));
    GP_TRY(get((void**)&s->e_last, 8 * (size_t)(G * m)));
    GP_TRY(get((void**)&s->side_last, (size_t)((G + P + 1) * m)));
    GP_TRY(get((void**)&s->cnt_last, 8 * (size_t)(P + G)));
    GP_TRY(get((void**)&s->loy_last, 8 * (size_t)n));
    GP_TRY(get((void**)&s->obs_last, 4 * (size_t)n));
    std::vector<int64_t> head((size_t)L.off[0], 0);
    const int64_t hdr[GRP_HEADER_WORDS] = { GRP_TAG, GRP_LAYOUT_VERSION, n, m, G, 0, 0, 0, 0 };
    std::copy_n(hdr, GRP_HEADER_WORDS, head.begin());
    for (int g = 0; g <= GR_MAXG; ++g) head[(size_t)(GRP_HEADER_WORDS + g)] = s->sizes[g];
    signed char* gb = reinterpret_cast<signed char*>(head.data() + L.groups);
    for (int64_t i = 0; i < n; ++i) gb[i] = (signed char)groups[i];
    GP_HIP(hipMemcpyAsync(s->block, head.data(), sizeof(int64_t) * head.size(), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // head is this call's
    s->on = true;
    return 0;
}

int launch_groups_accumulate(hipStream_t st, GroupsState* s, const double* theta, const double* f, const double* mu, const double* y)
{
    GP_ARG(theta && f && mu && y);
    const int64_t n = s->n, m = s->m;
    const int G = s->G, P = (int)grp_pairs(G), G1 = G + 1;
    const GrpLayout L = grp_layout(n, m, G);
    const signed char* grp = reinterpret_cast<const signed char*>(s->block + L.groups);
    int64_t* hdr = reinterpret_cast<int64_t*>(s->block);
    auto u64 = [&](int k) { return s->block + L.off[k]; };
    auto u32 = [&](int k) { return reinterpret_cast<uint32_t*>(s->block + L.off[k]); };
    auto f64 = [&](int k) { return reinterpret_cast<double*>(s->block + L.off[k]); };
    GrpSizes sz{};
    for (int g = 0; g <= GR_MAXG; ++g) sz.n[g] = s->sizes[g];
    const size_t scratch = reinterpret_cast<char*>(s->obs) + grp_pad(4 * (size_t)n) - reinterpret_cast<char*>(s->ctl);
    GP_HIP(hipMemsetAsync(s->ctl, 0, scratch, st));
    // part A
    hipLaunchKernelGGL(grp_hist_kernel, dim3(grp_grid(n, GV_ROWS)), dim3(GR_THREADS), 0, st, theta, grp, n, G, s->hist, s->ctl);
    GrpLatentArgs a{};
    a.hist = s->hist; a.less = s->less; a.ctl = s->ctl; a.hdr = hdr; a.sz = sz; a.G = G;
    a.ov_sum = u64(GPIRT_GROUPS_OV_SUM);
    a.medhist = u32(GPIRT_GROUPS_MEDHIST); a.order = u32(GPIRT_GROUPS_ORDER); a.d_undef = u32(GPIRT_GROUPS_D_UNDEFINED);
    a.mean_sum = f64(GPIRT_GROUPS_MEAN_SUM); a.mean_sq = f64(GPIRT_GROUPS_MEAN_SQ);
    a.sd_sum = f64(GPIRT_GROUPS_SD_SUM); a.sd_sq = f64(GPIRT_GROUPS_SD_SQ);
    a.a_sum = f64(GPIRT_GROUPS_A_SUM); a.a_sq = f64(GPIRT_GROUPS_A_SQ);
    a.ovl_sum = f64(GPIRT_GROUPS_OVL_SUM); a.ovl_sq = f64(GPIRT_GROUPS_OVL_SQ);
    a.d_sum = f64(GPIRT_GROUPS_D_SUM); a.d_sq = f64(GPIRT_GROUPS_D_SQ);
    a.lat_last = s->lat_last; a.stat_last = s->stat_last;
    hipLaunchKernelGGL(grp_latent_kernel, dim3(1), dim3(GR_THREADS), 0, st, a);
    hipLaunchKernelGGL(grp_share_kernel, dim3(grp_grid(std::max<int64_t>(n, (int64_t)G1 * GR_K))), dim3(GR_THREADS), 0, st, theta, grp, n,
                       G, s->less, sz, s->ctl, u32(GPIRT_GROUPS_MEDIAN_COVER), f64(GPIRT_GROUPS_MEDIAN_SHARE),
                       u64(GPIRT_GROUPS_DENS_SUM), u64(GPIRT_GROUPS_DENS_SQ), s->hist_last);
    GP_HIP(hipGetLastError());
    // part B
    hipLaunchKernelGGL(grp_votes_kernel, dim3(grp_grid(n, GV_ROWS), grp_grid(m, GV_STRIP)), dim3(GR_THREADS), 0, st, f, mu, n, m, grp, G,
                       reinterpret_cast<unsigned long long*>(s->e), s->ctl + 1);
    GrpItemArgs b{};
    b.e = s->e; b.ctl = s->ctl; b.hdr = hdr; b.sz = sz; b.m = m; b.G = G; b.cnt = s->cnt;
    b.split_count = u32(GPIRT_GROUPS_SPLIT_COUNT);
    b.support_sum = f64(GPIRT_GROUPS_SUPPORT_SUM); b.support_sq = f64(GPIRT_GROUPS_SUPPORT_SQ);
    b.rice_sum = f64(GPIRT_GROUPS_RICE_SUM); b.rice_sq = f64(GPIRT_GROUPS_RICE_SQ);
    b.gap_sum = f64(GPIRT_GROUPS_GAP_SUM); b.gap_sq = f64(GPIRT_GROUPS_GAP_SQ);
    b.e_last = s->e_last; b.flags = s->side_last;
    hipLaunchKernelGGL(grp_items_kernel, dim3(grp_grid(m), (unsigned)(G + P)), dim3(GR_THREADS), 0, st, b);
    hipLaunchKernelGGL(grp_loyalty_kernel, dim3(grp_grid(n), grp_grid(m, GL_COLS)), dim3(GR_THREADS), 0, st, f, mu, y, n, m, grp, G,
                       s->side_last, P, s->ctl, reinterpret_cast<unsigned long long*>(s->loy), s->obs, s->cnt);
    GrpLoyArgs c{};
    c.grp = grp; c.ctl = s->ctl; c.hdr = hdr; c.n = n; c.G = G; c.cnt = s->cnt; c.loy = s->loy; c.obs = s->obs;
    c.nsplit_sum = u64(GPIRT_GROUPS_NSPLIT_SUM); c.nsplit_sq = u64(GPIRT_GROUPS_NSPLIT_SQ);
    c.obs_with_sum = u64(GPIRT_GROUPS_OBS_WITH_SUM); c.obs_n_sum = u64(GPIRT_GROUPS_OBS_N_SUM);
    c.loy_undef = u32(GPIRT_GROUPS_LOY_UNDEFINED);
    c.loy_sum = f64(GPIRT_GROUPS_LOY_SUM); c.loy_sq = f64(GPIRT_GROUPS_LOY_SQ);
    c.loy_last = s->loy_last; c.obs_last = s->obs_last; c.cnt_last = s->cnt_last;
    hipLaunchKernelGGL(grp_loy_update_kernel, dim3(grp_grid(n)), dim3(GR_THREADS), 0, st, c);
    GP_HIP(hipGetLastError());
    return 0;
}

int groups_get(hipStream_t st, GroupsState* s, const char* name, void* h_out, int64_t bytes)
{
    const int64_t n = s->n, m = s->m, G = s->G, P = grp_pairs(G), G1 = G + 1;
    const GrpLayout L = grp_layout(n, m, G);
    auto copy = [&](const void* src, void* dst, int64_t nb) -> int {
        GP_HIP(hipMemcpyAsync(dst, src, (size_t)nb, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    struct Last { const char* name; const void* src; int64_t bytes; };
    const Last last[] = {
        { "counts", s->block + 5, 32 },
        { "group_size", s->block + GRP_HEADER_WORDS, 8 * (GR_MAXG + 1) },
        { "groups", s->block + L.groups, n },
        { "hist", s->hist_last, 4 * G1 * GR_K },
        { "c1", s->lat_last, 8 * G1 }, { "c2", s->lat_last + G1, 8 * G1 }, { "med2", s->lat_last + 2 * G1, 8 * G1 },
        { "w", s->lat_last + 3 * G1, 8 * P }, { "ov", s->lat_last + 3 * G1 + P, 8 * P },
        { "latent_stats", s->stat_last, 8 * (3 * G1 + 3 * P) },
        { "e", s->e_last, 8 * G * m },
        { "side", s->side_last, G * m }, { "split", s->side_last + G * m, P * m }, { "contested", s->side_last + (G + P) * m, m },
        { "n_split", s->cnt_last, 8 * P }, { "c_g", s->cnt_last + P, 8 * G },
        { "loy", s->loy_last, 8 * n },
    };
    for (const Last& l : last)
        if (strcmp(l.name, name) == 0) { GP_ARG(bytes == l.bytes); return copy(l.src, h_out, bytes); }
    if (strcmp(name, "obs_with") == 0 || strcmp(name, "obs_n") == 0) {
        GP_ARG(bytes == 4 * n);
        std::vector<uint32_t> pk((size_t)n);
        GP_TRY(copy(s->obs_last, pk.data(), 4 * n));
        uint32_t* out = static_cast<uint32_t*>(h_out);
        for (int64_t i = 0; i < n; ++i) out[i] = name[4] == 'w' ? (pk[(size_t)i] & 0xFFFFu) : (pk[(size_t)i] >> 16);
        return 0;
    }
    for (int k = 0; k < GPIRT_GROUPS_NARRAYS; ++k)
        if (strcmp(kGrpRaw[k], name) == 0) {
            GP_ARG(bytes == grp_raw_count(k, n, m, G) * grp_raw_width(k));
            return copy(s->block + L.off[k], h_out, bytes);
        }
    set_error("unknown groups field '%s'", name);
    return GPIRT_E_ARG;
}

int groups_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_groups* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_GROUPS_MAX_TOP) {
        set_error("groups: top = %lld is outside 1..%d", (long long)out->top, GPIRT_GROUPS_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) {
        GP_ARG(d_states[c]);
        if (signs && signs[c] != 1 && signs[c] != -1) {
            set_error("groups: sign %d is %d, not +1 or -1", c, signs[c]);
            return GPIRT_E_ARG;
        }
    }
    HostGrp pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostGrp& r = c == 0 ? pooled : one;
        GP_TRY(grp_read(h->stream, d_states[c], r, c));
        if (c > 0 && (r.n != pooled.n || r.m != pooled.m || r.G != pooled.G ||
                      !std::equal(r.groups(), r.groups() + r.n, pooled.groups()))) {
            set_error("gpirt_groups_combine: state %d has another n, m or groups than state 0", c);
            return GPIRT_E_ARG;
        }
        if (signs && signs[c] < 0) grp_reflect(r);
        if (c == 0) continue;
        for (int q = 5; q <= 8; ++q) pooled.hdr()[q] += one.hdr()[q];
        for (int k = 0; k < GPIRT_GROUPS_NARRAYS; ++k) {
            const int64_t cnt = grp_raw_count(k, r.n, r.m, r.G);
            if (grp_raw_double(k)) for (int64_t g = 0; g < cnt; ++g) pooled.arr<double>(k)[g] += one.arr<double>(k)[g];     // in chain order
            else if (grp_raw_width(k) == 4) for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
            else for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint64_t>(k)[g] += one.arr<uint64_t>(k)[g];
        }
    }
    const HostGrp& r = pooled;
    const int64_t n = r.n, m = r.m, G = r.G, P = grp_pairs(G), top = out->top;
    out->n = n; out->m = m; out->G = G; out->pairs = P; out->chains = chains;
    out->latent_draws = r.hdr()[5]; out->latent_skipped = r.hdr()[6]; out->votes_draws = r.hdr()[7]; out->votes_skipped = r.hdr()[8];
    for (int g = 0; g <= GR_MAXG; ++g) out->group_size[g] = r.hdr()[GRP_HEADER_WORDS + g];
    out->included = out->group_size[G];
    for (int k = 0; k < GPIRT_GROUPS_NARRAYS; ++k)
        if (out->raw[k]) memcpy(out->raw[k], r.w.data() + r.L.off[k], (size_t)(grp_raw_count(k, n, m, G) * grp_raw_width(k)));
    const double nan = (double)NAN, V = (double)out->votes_draws;
    if (out->most_split_items || out->most_split_p) {
        const uint32_t* sc = r.arr<uint32_t>(GPIRT_GROUPS_SPLIT_COUNT);
        std::vector<int64_t> idx((size_t)m);
        for (int64_t p = 0; p < P; ++p) {
            for (int64_t j = 0; j < m; ++j) idx[(size_t)j] = j;
            std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return sc[p * m + x] > sc[p * m + y]; });
            for (int64_t t = 0; t < top; ++t) {
                const bool have = t < m;
                if (out->most_split_items) out->most_split_items[p * top + t] = have ? idx[(size_t)t] : -1;
                if (out->most_split_p)
                    out->most_split_p[p * top + t] = have && out->votes_draws > 0 ? (double)sc[p * m + idx[(size_t)t]] / V : nan;
            }
        }
    }
    if (out->least_loyal || out->least_loyal_loyalty) {
        const double* ls = r.arr<double>(GPIRT_GROUPS_LOY_SUM);
        const uint32_t* lu = r.arr<uint32_t>(GPIRT_GROUPS_LOY_UNDEFINED);
        std::vector<int64_t> idx;
        std::vector<double> val((size_t)n, nan);
        for (int64_t i = 0; i < n; ++i) {
            const int g = r.groups()[i];
            if (g < 0) continue;
            const int64_t den = out->votes_draws - (int64_t)lu[g];
            if (den <= 0) continue;
            val[(size_t)i] = ls[i] / (double)den;
            idx.push_back(i);
        }
        std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return val[(size_t)x] < val[(size_t)y]; });
        for (int64_t t = 0; t < top; ++t) {
            const bool have = (size_t)t < idx.size();
            if (out->least_loyal) out->least_loyal[t] = have ? idx[(size_t)t] : -1;
            if (out->least_loyal_loyalty) out->least_loyal_loyalty[t] = have ? val[(size_t)idx[(size_t)t]] : nan;
        }
    }
    return 0;
}

}  // namespace gpirt
