// ppc_dif.hip -- group-wise item fit of the posterior predictive checks (include/gpirt_hip.h, "group-wise item fit"; DESIGN.md
// section 22): per draw the respondents fall into cells (group, bin of theta), and per (cell, item) the yes answers of the data
// (T) and of the replicate (R) are counted beside what the model expects there (E, V) -- the Mantel-Haenszel odds ratio and the
// standardised P-difference of every focal group against group 0, a yes count and a chi-square per group.
//
// dif_assign_kernel (one work-group): every respondent's cell from theta's grid index and the group code, the cells' occupancy
// (integer LDS atomics) and the word that tells of a theta off the grid.
// dif_tables_kernel: a pass of its own over the n x m cells, lanes along i (coalesced), DF_ROWS respondents x DF_STRIP items per
// work-group.  It forms the PPC's replicate again (the same p, the same uniform) and adds N | T << 16 | R << 32, rint(p 2^44)
// and rint(p q 2^44) into a (strip, cell) table in LDS with integer atomics, then flushes the table's occupied entries into the
// draw's global tables with integer atomics.  Every term is an integer, so no order of arrival changes a sum.
// dif_update_kernel: 32 lanes per item, lane b owns bin b of every group.  It reads and clears the draw's tables, keeps the
// cells' accumulators, lays every statistic's per-bin terms out in LDS, sums each series in increasing b (one lane a series)
// and decides.  Each accumulator word is owned by one lane: no global floating-point atomics, bit-identical from run to run.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <strings.h>

namespace gpirt {

namespace {

constexpr int DF_THREADS = 256;
constexpr int DF_SUB = 4;                          // row sub-blocks of a work-group of dif_tables_kernel
constexpr int DF_ROWS = DF_THREADS * DF_SUB;       // 1024 respondents: N, T, R of a work-group fit their 16 bits
constexpr int DF_STRIP = 8;                        // items per work-group
constexpr int DF_CELLS = 128;                      // >= GPIRT_DIF_MAX_G * GPIRT_BINS_MAX_B = 124
constexpr int DF_CENTRE = (GPIRT_NGRID - 1) / 2;
constexpr int DU_THREADS = 128;
constexpr int DU_ITEMS = DU_THREADS / 32;          // items per work-group of dif_update_kernel
constexpr int DU_GS = 5, DU_FS = 7;                // series per group and per focal group
constexpr int DU_MAXK = DU_GS * GPIRT_DIF_MAX_G + DU_FS * (GPIRT_DIF_MAX_G - 1);
constexpr double DIF_FIX = 17592186044416.0;       // 2^44
constexpr double DIF_UNFIX = 1.0 / DIF_FIX;
static_assert(GPIRT_DIF_MAX_G * GPIRT_BINS_MAX_B <= DF_CELLS && DF_CELLS < DIF_NONE, "a cell is one byte");
static_assert(GPIRT_BINS_MAX_B <= 32, "one lane of a 32-lane group per bin");

const char* const kDifCell[GPIRT_DIF_CELL_NFIELDS] = { "obs_rate", "rep_rate", "exp_rate" };
const char* const kDifGroup[GPIRT_DIF_GROUP_NFIELDS] = { "ppp_yes", "ppp_yes_mid", "ppp_chi2", "ppp_chi2_mid", "chi2_obs_mean",
                                                         "chi2_rep_mean" };
const char* const kDifFocal[GPIRT_DIF_FOCAL_NFIELDS] = { "mh_log_or_obs_mean", "mh_log_or_rep_mean", "mh_delta_obs_mean", "ppp_mh",
                                                         "ppp_mh_mid", "mh_undefined", "std_obs_mean", "std_rep_mean", "std_undefined" };
const char* const kDifRaw[DIF_NARRAYS] = { "sum_n", "sum_t", "sum_r", "sum_e", "occ_sum", "yes_ge", "yes_gt", "chi_ge", "chi_gt",
                                           "mh_ge", "mh_gt", "mh_undefined_count", "std_undefined_count", "chi_obs_sum",
                                           "chi_rep_sum", "mh_log_obs_sum", "mh_log_rep_sum", "std_obs_sum", "std_rep_sum" };

struct DifCuts { int h; int d[GPIRT_BINS_MAX_H]; };

inline int dif_raw_width(int k) { return (k >= DIF_YES_GE && k <= DIF_STD_UNDEF) ? 4 : 8; }
inline bool dif_raw_double(int k) { return k == DIF_SUM_E || k >= DIF_CHI_OBS; }
inline int64_t dif_raw_count(int k, int64_t m, int64_t G, int64_t B) { return k <= DIF_SUM_E ? G * B * m : k == DIF_OCC ? G * B : G * m; }

__global__ __launch_bounds__(DF_THREADS) void dif_assign_kernel(const double* __restrict__ theta, const signed char* __restrict__ grp,
                                                                int64_t n, DifCuts c, int B, unsigned char* __restrict__ cell,
                                                                uint32_t* __restrict__ occ, int* __restrict__ ctl)
{
    __shared__ uint32_t cnt[DF_CELLS];
    __shared__ int bad;
    const int t = threadIdx.x;
    if (t < DF_CELLS) cnt[t] = 0;
    if (t == 0) bad = 0;
    __syncthreads();
    for (int64_t i = t; i < n; i += DF_THREADS) {
        const int k = grid_index(theta[i]);
        const int g = grp[i];
        unsigned char v = DIF_NONE;
        if (k < 0) bad = 1;                  // several lanes may store here: all store the same 1, and a barrier follows
        else if (g >= 0) {
            const int a = k >= DF_CENTRE ? k - DF_CENTRE : DF_CENTRE - k;
            int l = 0;
            for (int q = 0; q < c.h; ++q) l += a >= c.d[q] ? 1 : 0;
            v = (unsigned char)(g * B + (k >= DF_CENTRE ? c.h + l : c.h - l));
            atomicAdd(&cnt[v], 1u);
        }
        cell[i] = v;
    }
    __syncthreads();
    if (t < DF_CELLS) occ[t] = cnt[t];
    if (t == 0) { ctl[0] = bad; ctl[1] = 0; }
}

struct DifTabArgs {
    const double* f; const double* mu; const double* y;
    int64_t n, m;
    uint64_t seed; uint32_t iter, item0;
    const unsigned char* cell; int GB;
    unsigned long long* tab;              // [3][GB][m]
    int* bad;
};

__global__ __launch_bounds__(DF_THREADS) void dif_tables_kernel(DifTabArgs a)
{
    __shared__ unsigned long long sc[3][DF_STRIP][DF_CELLS];
    const int t = threadIdx.x;
    for (int k = t; k < 3 * DF_STRIP * DF_CELLS; k += DF_THREADS) (&sc[0][0][0])[k] = 0ull;
    __syncthreads();
    const int64_t j0 = (int64_t)blockIdx.y * DF_STRIP;
    const int w = (int)(a.m - j0 < DF_STRIP ? a.m - j0 : DF_STRIP);
    for (int sub = 0; sub < DF_SUB; ++sub) {
        const int64_t i = ((int64_t)blockIdx.x * DF_SUB + sub) * DF_THREADS + t;
        const int c = i < a.n ? a.cell[i] : DIF_NONE;
        if (c == DIF_NONE) continue;       // (no barrier inside this loop)
        double yv[DF_STRIP], gv[DF_STRIP];
#pragma unroll
        for (int jj = 0; jj < DF_STRIP; ++jj) {
            yv[jj] = (double)NAN; gv[jj] = 0.0;
            if (jj < w) {
                const int64_t at = i + (j0 + jj) * a.n;
                yv[jj] = a.y[at]; gv[jj] = a.f[at] + a.mu[at];
            }
        }
#pragma unroll
        for (int jj = 0; jj < DF_STRIP; ++jj) {
            const double g = gv[jj];
            if (!(yv[jj] == yv[jj])) continue;                    // not observed (or beyond the strip)
            if (!isfinite(g)) { *a.bad = 1; continue; }           // (every writer stores the same word)
            const double e = exp(-fabs(g));
            const double p = g >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
            const double q = g >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
            const double u = item_uniform(a.seed, a.iter, GPIRT_ST_PPC, (uint32_t)(a.item0 + j0 + jj), (uint32_t)i);
            const unsigned long long pk = 1ull | (yv[jj] > 0.0 ? 1ull << 16 : 0ull) | (u < p ? 1ull << 32 : 0ull);
            atomicAdd(&sc[0][jj][c], pk);
            atomicAdd(&sc[1][jj][c], (unsigned long long)rint(p * DIF_FIX));
            atomicAdd(&sc[2][jj][c], (unsigned long long)rint(p * q * DIF_FIX));
        }
    }
    __syncthreads();
    const int64_t C = (int64_t)a.GB * a.m;
    for (int k = t; k < w * a.GB; k += DF_THREADS) {
        const int jj = k / a.GB, c = k - jj * a.GB;
        const unsigned long long pk = sc[0][jj][c];
        if (pk == 0ull) continue;
        const int64_t at = (int64_t)c * a.m + j0 + jj;
        atomicAdd(&a.tab[at], pk);
        atomicAdd(&a.tab[C + at], sc[1][jj][c]);
        atomicAdd(&a.tab[2 * C + at], sc[2][jj][c]);
    }
}

struct DifUpdateArgs {
    uint64_t* tab; uint64_t* tab_last; double* stat_last;
    const unsigned char* cell_cur; unsigned char* cell_last;
    const uint32_t* occ_cur; const int* ctl;
    int64_t n, m;
    int G, B;
    int64_t* hdr;                                     // the block's header: [3] dif_draws, [4] dif_skipped
    uint64_t* sum_n; uint64_t* sum_t; uint64_t* sum_r; double* sum_e; uint64_t* occ;
    uint32_t* cnt;                                    // DIF_YES_GE ..: consecutive arrays of cstride uint32
    double* dsum;                                     // DIF_CHI_OBS ..: consecutive arrays of dstride doubles
    int64_t cstride, dstride;
};

__global__ __launch_bounds__(DU_THREADS) void dif_update_kernel(DifUpdateArgs a)
{
    __shared__ double term[DU_ITEMS][DU_MAXK][32];
    __shared__ double tot[DU_ITEMS][DU_MAXK];
    const int t = threadIdx.x, b = t & 31, li = t >> 5, G = a.G, B = a.B;
    const int64_t gid = (int64_t)blockIdx.x * DU_THREADS + t;
    const int64_t j = (int64_t)blockIdx.x * DU_ITEMS + li;
    const bool skip = a.ctl[0] != 0 || a.ctl[1] != 0;
    if (gid == 0) a.hdr[skip ? 4 : 3] += 1;           // (nobody else in this launch reads the header)
    const bool have = j < a.m && b < B;
    const int64_t C = (int64_t)G * B * a.m;
    uint32_t N[GPIRT_DIF_MAX_G], T[GPIRT_DIF_MAX_G], R[GPIRT_DIF_MAX_G];
    uint64_t Ef[GPIRT_DIF_MAX_G], Vf[GPIRT_DIF_MAX_G];
#pragma unroll
    for (int g = 0; g < GPIRT_DIF_MAX_G; ++g) {
        N[g] = T[g] = R[g] = 0; Ef[g] = Vf[g] = 0;
        if (have && g < G) {
            const int64_t at = ((int64_t)g * B + b) * a.m + j;
            const uint64_t pk = a.tab[at];
            Ef[g] = a.tab[C + at]; Vf[g] = a.tab[2 * C + at];
            a.tab[at] = 0; a.tab[C + at] = 0; a.tab[2 * C + at] = 0;      // the next draw starts from zero, counted or not
            N[g] = (uint32_t)(pk & 0xFFFFu); T[g] = (uint32_t)((pk >> 16) & 0xFFFFu); R[g] = (uint32_t)((pk >> 32) & 0xFFFFu);
            if (!skip) { a.tab_last[at] = pk; a.tab_last[C + at] = Ef[g]; a.tab_last[2 * C + at] = Vf[g]; }
        }
    }
    if (skip) return;                                  // (the same for every thread of the launch)
    for (int64_t i = gid; i < a.n; i += (int64_t)gridDim.x * DU_THREADS) a.cell_last[i] = a.cell_cur[i];
    if (gid < G * B) a.occ[gid] += a.occ_cur[gid];
    const int K = DU_GS * G + DU_FS * (G - 1);
    for (int k = 0; k < K; ++k) term[li][k][b] = 0.0;
    if (have) {
#pragma unroll
        for (int g = 0; g < GPIRT_DIF_MAX_G; ++g) {
            if (g >= G) break;
            const int64_t at = ((int64_t)g * B + b) * a.m + j;
            const double E = (double)Ef[g] * DIF_UNFIX, V = (double)Vf[g] * DIF_UNFIX;
            a.sum_n[at] += N[g]; a.sum_t[at] += T[g]; a.sum_r[at] += R[g];
            a.sum_e[at] += E;
            double* s = &term[li][DU_GS * g][b];
            if (N[g] > 0 && V > 0.0) {
                const double dT = (double)T[g] - E, dR = (double)R[g] - E;
                s[0] = dT * dT / V;
                s[32] = dR * dR / V;
            }
            s[64] = (double)R[g]; s[96] = (double)T[g]; s[128] = R[g] != T[g] ? 1.0 : 0.0;
            if (g > 0 && N[0] > 0 && N[g] > 0) {
                double* q = &term[li][DU_GS * G + DU_FS * (g - 1)][b];
                const double nb = (double)(N[0] + N[g]), n0 = (double)N[0], nf = (double)N[g];
                q[0] = (double)((uint64_t)T[0] * (uint64_t)(N[g] - T[g])) / nb;
                q[32] = (double)((uint64_t)(N[0] - T[0]) * (uint64_t)T[g]) / nb;
                q[64] = (double)((uint64_t)R[0] * (uint64_t)(N[g] - R[g])) / nb;
                q[96] = (double)((uint64_t)(N[0] - R[0]) * (uint64_t)R[g]) / nb;
                q[128] = nf * ((double)T[g] / nf - (double)T[0] / n0);
                q[160] = nf * ((double)R[g] / nf - (double)R[0] / n0);
                q[192] = nf;
            }
        }
    }
    __syncthreads();
    for (int k = b; k < K; k += 32) {                  // one lane a series: its terms in increasing b
        double s = 0.0;
        for (int q = 0; q < B; ++q) s += term[li][k][q];
        tot[li][k] = s;
    }
    __syncthreads();
    if (!(j < a.m && b < G)) return;
    const int g = b;
    const int64_t at = (int64_t)g * a.m + j, GM = (int64_t)G * a.m;
    auto cnt = [&](int arr) -> uint32_t& { return a.cnt[(int64_t)(arr - DIF_YES_GE) * a.cstride + at]; };
    auto dsum = [&](int arr) -> double& { return a.dsum[(int64_t)(arr - DIF_CHI_OBS) * a.dstride + at]; };
    const double* s = &tot[li][DU_GS * g];
    const double x2T = s[0], x2R = s[1], Rg = s[2], Tg = s[3];
    const bool tie = s[4] == 0.0;
    cnt(DIF_YES_GE) += Rg >= Tg ? 1u : 0u;
    cnt(DIF_YES_GT) += Rg > Tg ? 1u : 0u;
    cnt(DIF_CHI_GE) += (tie || x2R >= x2T) ? 1u : 0u;
    cnt(DIF_CHI_GT) += (!tie && x2R > x2T) ? 1u : 0u;
    dsum(DIF_CHI_OBS) += x2T;
    dsum(DIF_CHI_REP) += x2R;
    const double nan = (double)NAN;
    double st[DIF_NSTATS] = { nan, nan, nan, nan, nan, nan, x2T, x2R };
    if (g > 0) {
        const double* q = &tot[li][DU_GS * G + DU_FS * (g - 1)];
        const double numT = q[0], denT = q[1], numR = q[2], denR = q[3];
        st[0] = numT; st[1] = denT; st[2] = numR; st[3] = denR;
        if (numT == 0.0 || denT == 0.0 || numR == 0.0 || denR == 0.0) cnt(DIF_MH_UNDEF) += 1u;
        else {
            const double lhs = numR * denT, rhs = numT * denR;
            cnt(DIF_MH_GE) += lhs >= rhs ? 1u : 0u;
            cnt(DIF_MH_GT) += lhs > rhs ? 1u : 0u;
            dsum(DIF_MH_LOG_OBS) += log(numT / denT);
            dsum(DIF_MH_LOG_REP) += log(numR / denR);
        }
        if (q[6] > 0.0) {
            st[4] = q[4] / q[6]; st[5] = q[5] / q[6];
            dsum(DIF_STD_OBS) += st[4];
            dsum(DIF_STD_REP) += st[5];
        } else cnt(DIF_STD_UNDEF) += 1u;
    }
    for (int k = 0; k < DIF_NSTATS; ++k) a.stat_last[(int64_t)k * GM + at] = st[k];
}

// a state block on the host
struct HostDif {
    std::vector<uint64_t> w;
    int64_t n = 0, m = 0, B = 0, G = 0, item0 = 0;
    int h = 0;
    DifLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    const int64_t* cuts() const { return hdr() + DIF_HEADER_WORDS; }
    const int64_t* gw() const { return hdr() + DIF_HEADER_WORDS + DIF_CUT_WORDS; }
    const signed char* groups() const { return reinterpret_cast<const signed char*>(w.data() + L.groups); }
    template <class T> T* arr(int k) { return reinterpret_cast<T*>(w.data() + L.off[k]); }
    template <class T> const T* arr(int k) const { return reinterpret_cast<const T*>(w.data() + L.off[k]); }
};

int dif_read(hipStream_t st, const void* d_state, HostDif& r, const char* who, int c)
{
    int64_t hdr[DIF_HEADER_WORDS + DIF_CUT_WORDS + DIF_GROUP_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    const int64_t G = hdr[DIF_HEADER_WORDS + DIF_CUT_WORDS];
    if (hdr[7] != DIF_TAG || hdr[2] != DIF_LAYOUT_VERSION || hdr[0] <= 0 || hdr[0] > GPIRT_DIF_MAX_N || hdr[1] <= 0 || hdr[3] < 0 ||
        hdr[4] < 0 || hdr[6] < 3 || hdr[6] > GPIRT_BINS_MAX_B || hdr[6] % 2 == 0 || G < 2 || G > GPIRT_DIF_MAX_G) {
        set_error("%s: state %d is not a group-wise PPC state block of layout %d", who, c, DIF_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[0]; r.m = hdr[1]; r.item0 = hdr[5]; r.B = hdr[6]; r.h = (int)((hdr[6] - 1) / 2); r.G = G;
    r.L = dif_layout(r.n, r.m, r.G, r.B);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

double dif_cell_field(const HostDif& r, int fld, int64_t at)
{
    const uint64_t sN = r.arr<uint64_t>(DIF_SUM_N)[at];
    if (!sN) return (double)NAN;
    switch (fld) {
        case 0: return (double)r.arr<uint64_t>(DIF_SUM_T)[at] / (double)sN;
        case 1: return (double)r.arr<uint64_t>(DIF_SUM_R)[at] / (double)sN;
        case 2: return r.arr<double>(DIF_SUM_E)[at] / (double)sN;
        default: break;
    }
    return (double)NAN;
}

double dif_group_field(const HostDif& r, int fld, int64_t at)
{
    const int64_t S = r.hdr()[3];
    if (S < 1) return (double)NAN;
    const double dS = (double)S;
    auto c = [&](int k) { return (double)r.arr<uint32_t>(k)[at]; };
    switch (fld) {
        case 0: return c(DIF_YES_GE) / dS;
        case 1: return (c(DIF_YES_GE) + c(DIF_YES_GT)) / (2.0 * dS);
        case 2: return c(DIF_CHI_GE) / dS;
        case 3: return (c(DIF_CHI_GE) + c(DIF_CHI_GT)) / (2.0 * dS);
        case 4: return r.arr<double>(DIF_CHI_OBS)[at] / dS;
        case 5: return r.arr<double>(DIF_CHI_REP)[at] / dS;
        default: break;
    }
    return (double)NAN;
}

double dif_focal_field(const HostDif& r, int fld, int64_t at)
{
    const double nan = (double)NAN;
    if (at < r.m) return nan;                          // group 0
    const int64_t S = r.hdr()[3];
    auto c = [&](int k) { return (double)r.arr<uint32_t>(k)[at]; };
    const int64_t Sm = S - (int64_t)r.arr<uint32_t>(DIF_MH_UNDEF)[at], Ss = S - (int64_t)r.arr<uint32_t>(DIF_STD_UNDEF)[at];
    switch (fld) {
        case 0: return Sm > 0 ? r.arr<double>(DIF_MH_LOG_OBS)[at] / (double)Sm : nan;
        case 1: return Sm > 0 ? r.arr<double>(DIF_MH_LOG_REP)[at] / (double)Sm : nan;
        case 2: return Sm > 0 ? -2.35 * (r.arr<double>(DIF_MH_LOG_OBS)[at] / (double)Sm) : nan;
        case 3: return Sm > 0 ? c(DIF_MH_GE) / (double)Sm : nan;
        case 4: return Sm > 0 ? (c(DIF_MH_GE) + c(DIF_MH_GT)) / (2.0 * (double)Sm) : nan;
        case 5: return c(DIF_MH_UNDEF);
        case 6: return Ss > 0 ? r.arr<double>(DIF_STD_OBS)[at] / (double)Ss : nan;
        case 7: return Ss > 0 ? r.arr<double>(DIF_STD_REP)[at] / (double)Ss : nan;
        case 8: return c(DIF_STD_UNDEF);
        default: break;
    }
    return nan;
}

void dif_fill(const HostDif& r, gpirt_ppc_dif* out)
{
    const int64_t m = r.m, B = r.B, G = r.G, C = G * B * m, GM = G * m;
    out->n = r.n; out->m = m; out->B = B; out->dif_draws = r.hdr()[3]; out->dif_skipped = r.hdr()[4];
    out->G = (int)G; out->h = r.h;
    for (int q = 0; q <= GPIRT_BINS_MAX_H; ++q) out->cuts[q] = q < r.h ? (int)r.cuts()[q] : 0;
    for (int g = 0; g < GPIRT_DIF_MAX_G; ++g) out->group_size[g] = r.gw()[1 + g];
    for (int fld = 0; fld < GPIRT_DIF_CELL_NFIELDS; ++fld)
        if (out->cell[fld]) for (int64_t at = 0; at < C; ++at) out->cell[fld][at] = dif_cell_field(r, fld, at);
    if (out->occupancy)
        for (int64_t c = 0; c < G * B; ++c)
            out->occupancy[c] = r.hdr()[3] > 0 ? (double)r.arr<uint64_t>(DIF_OCC)[c] / (double)r.hdr()[3] : (double)NAN;
    for (int fld = 0; fld < GPIRT_DIF_GROUP_NFIELDS; ++fld)
        if (out->group[fld]) for (int64_t at = 0; at < GM; ++at) out->group[fld][at] = dif_group_field(r, fld, at);
    for (int fld = 0; fld < GPIRT_DIF_FOCAL_NFIELDS; ++fld)
        if (out->focal[fld]) for (int64_t at = 0; at < GM; ++at) out->focal[fld][at] = dif_focal_field(r, fld, at);
    for (int k = 0; k < DIF_NARRAYS; ++k)
        if (out->raw[k]) memcpy(out->raw[k], r.w.data() + r.L.off[k], (size_t)(dif_raw_count(k, m, G, B) * dif_raw_width(k)));
    if (!out->flagged_items && !out->flagged_groups && !out->flagged_ppp_mh_mid) return;
    // the (focal group, item) pairs by decreasing |ppp_mh_mid - 0.5|, ties to the lowest (group, item): a stable sort
    struct E { double dist, mid; int64_t g, j; };
    std::vector<E> es;
    for (int64_t at = m; at < GM; ++at) {
        const double mid = dif_focal_field(r, 4, at);
        if (mid == mid) es.push_back(E{ fabs(mid - 0.5), mid, at / m, at % m });
    }
    std::stable_sort(es.begin(), es.end(), [](const E& x, const E& y) { return x.dist > y.dist; });
    for (int t = 0; t < out->top; ++t) {
        const bool have = (size_t)t < es.size();
        if (out->flagged_items) out->flagged_items[t] = have ? es[(size_t)t].j : -1;
        if (out->flagged_groups) out->flagged_groups[t] = have ? es[(size_t)t].g : -1;
        if (out->flagged_ppp_mh_mid) out->flagged_ppp_mh_mid[t] = have ? es[(size_t)t].mid : (double)NAN;
    }
}

// theta -> -theta: cell (g, b, j) becomes (g, B - 1 - b, j), and so does occ_sum
void dif_reflect(HostDif& r)
{
    const int64_t m = r.m, B = r.B, G = r.G;
    auto rows = [&](auto* p, int64_t width) {
        for (int64_t g = 0; g < G; ++g)
            for (int64_t b = 0; b < B / 2; ++b)
                std::swap_ranges(p + (g * B + b) * width, p + (g * B + b + 1) * width, p + (g * B + B - 1 - b) * width);
    };
    for (int k = DIF_SUM_N; k <= DIF_SUM_R; ++k) rows(r.arr<uint64_t>(k), m);
    rows(r.arr<double>(DIF_SUM_E), m);
    rows(r.arr<uint64_t>(DIF_OCC), 1);
}

}  // namespace

DifLayout dif_layout(int64_t n, int64_t m, int64_t G, int64_t B)
{
    DifLayout L{};
    int64_t at = DIF_HEADER_WORDS + DIF_CUT_WORDS + DIF_GROUP_WORDS;
    L.groups = at;
    at += (n + 15) / 16 * 2;
    for (int k = 0; k < DIF_NARRAYS; ++k) {
        L.off[k] = at;
        const int64_t bytes = dif_raw_count(k, m, G, B) * dif_raw_width(k);
        at += (bytes + 15) / 16 * 2;                                  // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int64_t dif_state_words(const DifState* p) { return dif_layout(p->n, p->m, p->G, p->B).words; }

int dif_check_groups(int64_t n, int G, const int32_t* groups, int64_t* sizes)
{
    if (n > GPIRT_DIF_MAX_N) {
        set_error("group-wise PPC: n = %lld is beyond %d respondents", (long long)n, GPIRT_DIF_MAX_N);
        return GPIRT_E_ARG;
    }
    if (G < 2 || G > GPIRT_DIF_MAX_G || !groups) {
        set_error("group-wise PPC: %d groups given, 2..%d are taken", G, GPIRT_DIF_MAX_G);
        return GPIRT_E_ARG;
    }
    int64_t cnt[GPIRT_DIF_MAX_G] = {};
    for (int64_t i = 0; i < n; ++i) {
        if (groups[i] < -1 || groups[i] >= G) {
            set_error("group-wise PPC: the code %d of respondent %lld is outside -1..%d", (int)groups[i], (long long)i, G - 1);
            return GPIRT_E_ARG;
        }
        if (groups[i] >= 0) cnt[groups[i]] += 1;
    }
    for (int g = 0; g < G; ++g)
        if (cnt[g] == 0) { set_error("group-wise PPC: group %d has no member", g); return GPIRT_E_ARG; }
    if (sizes) for (int g = 0; g < GPIRT_DIF_MAX_G; ++g) sizes[g] = cnt[g];
    return 0;
}

void dif_free(DifState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = DifState{};
}

int dif_alloc(hipStream_t st, DifState* p, int64_t n, int64_t m, int64_t item0, int G, const int32_t* groups, int h, const int* cuts)
{
    int64_t sizes[GPIRT_DIF_MAX_G];
    GP_TRY(dif_check_groups(n, G, groups, sizes));
    GP_TRY(bin_check_cuts(h, cuts));
    const int64_t B = 2 * h + 1, C = (int64_t)G * B * m;
    const DifLayout L = dif_layout(n, m, G, B);
    p->n = n; p->m = m; p->item0 = item0; p->G = G; p->h = h; p->B = (int)B;
    for (int q = 0; q < h; ++q) p->cuts[q] = cuts[q];
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->cell_cur, (size_t)n));
    GP_TRY(get((void**)&p->cell_last, (size_t)n));
    GP_TRY(get((void**)&p->occ, sizeof(uint32_t) * DF_CELLS));
    GP_TRY(get((void**)&p->ctl, sizeof(int) * 4));
    GP_TRY(get((void**)&p->tab, sizeof(uint64_t) * 3 * (size_t)C));
    GP_TRY(get((void**)&p->tab_last, sizeof(uint64_t) * 3 * (size_t)C));
    GP_TRY(get((void**)&p->stat_last, sizeof(double) * DIF_NSTATS * (size_t)G * (size_t)m));
    std::vector<int64_t> head((size_t)(L.off[0]), 0);
    const int64_t hdr[DIF_HEADER_WORDS] = { n, m, DIF_LAYOUT_VERSION, 0, 0, item0, B, DIF_TAG };
    std::copy_n(hdr, DIF_HEADER_WORDS, head.begin());
    for (int q = 0; q < h; ++q) head[(size_t)(DIF_HEADER_WORDS + q)] = cuts[q];
    head[DIF_HEADER_WORDS + DIF_CUT_WORDS] = G;
    for (int g = 0; g < GPIRT_DIF_MAX_G; ++g) head[(size_t)(DIF_HEADER_WORDS + DIF_CUT_WORDS + 1 + g)] = sizes[g];
    signed char* gb = reinterpret_cast<signed char*>(head.data() + L.groups);
    for (int64_t i = 0; i < n; ++i) gb[i] = (signed char)groups[i];
    GP_HIP(hipMemcpyAsync(p->block, head.data(), sizeof(int64_t) * head.size(), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // head is this call's: nothing below may leave with the copy pending
    p->on = true;
    return 0;
}

int launch_dif_accumulate(hipStream_t st, DifState* p, const double* f, const double* mu, const double* y, uint64_t seed,
                          uint32_t iter, const double* theta)
{
    GP_ARG(theta);
    const DifLayout L = dif_layout(p->n, p->m, p->G, p->B);
    DifCuts c{};
    c.h = p->h;
    for (int q = 0; q < p->h; ++q) c.d[q] = p->cuts[q];
    hipLaunchKernelGGL(dif_assign_kernel, dim3(1), dim3(DF_THREADS), 0, st, theta,
                       reinterpret_cast<const signed char*>(p->block + L.groups), p->n, c, p->B, p->cell_cur, p->occ, p->ctl);
    GP_HIP(hipGetLastError());
    DifTabArgs t{};
    t.f = f; t.mu = mu; t.y = y; t.n = p->n; t.m = p->m; t.seed = seed; t.iter = iter; t.item0 = (uint32_t)p->item0;
    t.cell = p->cell_cur; t.GB = p->G * p->B; t.tab = reinterpret_cast<unsigned long long*>(p->tab); t.bad = p->ctl + 1;
    const dim3 grid((unsigned)((p->n + DF_ROWS - 1) / DF_ROWS), (unsigned)((p->m + DF_STRIP - 1) / DF_STRIP));
    hipLaunchKernelGGL(dif_tables_kernel, grid, dim3(DF_THREADS), 0, st, t);
    GP_HIP(hipGetLastError());
    DifUpdateArgs a{};
    a.tab = p->tab; a.tab_last = p->tab_last; a.stat_last = p->stat_last;
    a.cell_cur = p->cell_cur; a.cell_last = p->cell_last; a.occ_cur = p->occ; a.ctl = p->ctl;
    a.n = p->n; a.m = p->m; a.G = p->G; a.B = p->B;
    a.hdr = reinterpret_cast<int64_t*>(p->block);
    auto at = [&](int k) { return p->block + L.off[k]; };
    a.sum_n = at(DIF_SUM_N); a.sum_t = at(DIF_SUM_T); a.sum_r = at(DIF_SUM_R);
    a.sum_e = reinterpret_cast<double*>(at(DIF_SUM_E)); a.occ = at(DIF_OCC);
    a.cnt = reinterpret_cast<uint32_t*>(at(DIF_YES_GE)); a.dsum = reinterpret_cast<double*>(at(DIF_CHI_OBS));
    a.cstride = (L.off[DIF_YES_GT] - L.off[DIF_YES_GE]) * 2; a.dstride = L.off[DIF_CHI_REP] - L.off[DIF_CHI_OBS];
    hipLaunchKernelGGL(dif_update_kernel, dim3((unsigned)((p->m + DU_ITEMS - 1) / DU_ITEMS)), dim3(DU_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

int dif_get(hipStream_t st, DifState* p, const char* name, void* h_out, int64_t bytes)
{
    const int64_t n = p->n, m = p->m, B = p->B, G = p->G, C = G * B * m, GM = G * m;
    const DifLayout L = dif_layout(n, m, G, B);
    auto copy = [&](const void* src, void* dst, int64_t nb) -> int {
        GP_HIP(hipMemcpyAsync(dst, src, (size_t)nb, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 16); return copy(p->block + 3, h_out, bytes); }
    if (strcmp(name, "cuts") == 0) { GP_ARG(bytes == 8 * p->h); return copy(p->block + DIF_HEADER_WORDS, h_out, bytes); }
    if (strcmp(name, "groups") == 0) { GP_ARG(bytes == n); return copy(p->block + L.groups, h_out, bytes); }
    if (strcmp(name, "group_size") == 0) {
        GP_ARG(bytes == 8 * GPIRT_DIF_MAX_G);
        return copy(p->block + DIF_HEADER_WORDS + DIF_CUT_WORDS + 1, h_out, bytes);
    }
    if (strcmp(name, "cell") == 0) { GP_ARG(bytes == n); return copy(p->cell_last, h_out, bytes); }
    if (strcmp(name, "stats") == 0) { GP_ARG(bytes == 8 * DIF_NSTATS * GM); return copy(p->stat_last, h_out, bytes); }
    if (strlen(name) == 2 && name[0] == 't') {                        // the last counted draw's tables
        if (name[1] == 'E' || name[1] == 'V') { GP_ARG(bytes == 8 * C); return copy(p->tab_last + (name[1] == 'V' ? 2 : 1) * C, h_out, bytes); }
        const char* ints = "NTR";
        if (const char* q = strchr(ints, name[1])) {
            GP_ARG(bytes == 4 * C);
            std::vector<uint64_t> pk((size_t)C);
            GP_TRY(copy(p->tab_last, pk.data(), 8 * C));
            int32_t* out = static_cast<int32_t*>(h_out);
            for (int64_t at = 0; at < C; ++at) out[at] = (int32_t)((pk[(size_t)at] >> (16 * (q - ints))) & 0xFFFFu);
            return 0;
        }
    }
    int cell = -1, group = -1, focal = -1;
    for (int k = 0; k < GPIRT_DIF_CELL_NFIELDS; ++k) if (strcmp(kDifCell[k], name) == 0) cell = k;
    for (int k = 0; k < GPIRT_DIF_GROUP_NFIELDS; ++k) if (strcmp(kDifGroup[k], name) == 0) group = k;
    for (int k = 0; k < GPIRT_DIF_FOCAL_NFIELDS; ++k) if (strcmp(kDifFocal[k], name) == 0) focal = k;
    const bool occ = strcmp(name, "occupancy") == 0;
    if (cell < 0 && group < 0 && focal < 0 && !occ) {
        for (int k = 0; k < DIF_NARRAYS; ++k)
            if (strcasecmp(kDifRaw[k], name) == 0) {
                GP_ARG(bytes == dif_raw_count(k, m, G, B) * dif_raw_width(k));
                return copy(p->block + L.off[k], h_out, bytes);
            }
        set_error("unknown group-wise PPC field '%s'", name);
        return GPIRT_E_ARG;
    }
    GP_ARG(bytes == 8 * (cell >= 0 ? C : occ ? G * B : GM));
    HostDif r;
    GP_TRY(dif_read(st, p->block, r, "gpirt_sampler_ppc_dif_get", 0));
    double* out = static_cast<double*>(h_out);
    if (cell >= 0) for (int64_t at = 0; at < C; ++at) out[at] = dif_cell_field(r, cell, at);
    else if (group >= 0) for (int64_t at = 0; at < GM; ++at) out[at] = dif_group_field(r, group, at);
    else if (focal >= 0) for (int64_t at = 0; at < GM; ++at) out[at] = dif_focal_field(r, focal, at);
    else for (int64_t c = 0; c < G * B; ++c) out[c] = r.hdr()[3] > 0 ? (double)r.arr<uint64_t>(DIF_OCC)[c] / (double)r.hdr()[3] : (double)NAN;
    return 0;
}

int dif_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ppc_dif* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved0 == 0 && out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_DIF_MAX_TOP) {
        set_error("group-wise PPC: top = %d is outside 1..%d", out->top, GPIRT_DIF_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) {
        GP_ARG(d_states[c]);
        if (signs) GP_ARG(signs[c] == 1 || signs[c] == -1);
    }
    HostDif pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostDif& r = c == 0 ? pooled : one;
        GP_TRY(dif_read(h->stream, d_states[c], r, "gpirt_ppc_dif_combine", c));
        if (c > 0 && (r.n != pooled.n || r.m != pooled.m || r.item0 != pooled.item0 || r.B != pooled.B || r.G != pooled.G ||
                      !std::equal(r.cuts(), r.cuts() + DIF_CUT_WORDS, pooled.cuts()) ||
                      !std::equal(r.groups(), r.groups() + r.n, pooled.groups()))) {
            set_error("gpirt_ppc_dif_combine: state %d has another n, m, item0, groups or cuts than state 0", c);
            return GPIRT_E_ARG;
        }
        if (signs && signs[c] < 0) dif_reflect(r);
        if (c == 0) continue;
        pooled.hdr()[3] += one.hdr()[3];
        pooled.hdr()[4] += one.hdr()[4];
        for (int k = 0; k < DIF_NARRAYS; ++k) {
            const int64_t cnt = dif_raw_count(k, r.m, r.G, r.B);
            if (dif_raw_double(k)) for (int64_t g = 0; g < cnt; ++g) pooled.arr<double>(k)[g] += one.arr<double>(k)[g];      // in chain order
            else if (dif_raw_width(k) == 4) for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
            else for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint64_t>(k)[g] += one.arr<uint64_t>(k)[g];
        }
    }
    dif_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
