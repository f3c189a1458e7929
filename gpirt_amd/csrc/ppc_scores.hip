// ppc_scores.hip -- the score-based posterior predictive checks (include/gpirt_hip.h, "score-based PPC"):
// the distribution of the respondents' scores, every item's correlation with the rest score and the item fit within groups of
// the rest score, for the data and for the PPC's replicate of every draw.
//
// pps_rows_kernel (pass A): one streaming pass over f, mu and y, lanes along i (coalesced), 256 respondents x PA_STRIP items per
// work-group.  It forms the PPC's replicate again (the same p, the same uniform); a wave's 64 answers to one item become ONE
// 64-bit word of the bit plane repw[j][W] by a wave vote, written with an ordinary store (the bits of rows >= n and of missing
// cells are zero).  It also leaves each respondent's strip partial (rep count | observed << 16) and the word that tells of a
// non-finite g in an observed cell.
// pps_scores_kernel: a respondent's score from its strip partials, and the histogram (integer atomics).
// pps_cols_kernel (pass B): reads repw and the scores, and f, mu and y once more for p; PB_ROWS respondents x PB_STRIP items per
// work-group.  Per item the sums A, B, Cq, D (registers, then a fixed shuffle tree and integer LDS atomics), per (group, item)
// Nr | R << 32 and the fixed-point Er, Vr under the replicate's grouping and Eo, Vo under the data's (integer LDS atomics), then
// flushed into the draw's global tables with integer atomics.  Every term is an integer, so no order of arrival changes a sum.
// pps_update_kernel: one thread per item owns the item's and its K cells' accumulators: it reads and clears the draw's tables,
// forms r and the two X2 (k ascending) and decides.  pps_hist_kernel (one work-group): the histogram's and the CDF's decisions
// and the spread of the scores.  No floating-point atomics: bit-identical from run to run.
// The DATA instances run once at enable with the plane of Y in place of the replicate's and X in place of Xr: the same code counts
// the constants (x_obs, hist_obs, sums_obs, r_obs, tNo, tT, var_obs).
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <strings.h>

namespace gpirt {

namespace {

constexpr int PA_THREADS = 256;
constexpr int PA_STRIP = 32;                       // items per work-group of pass A
constexpr int PB_THREADS = 256;
constexpr int PB_SUB = 4;                          // row sub-blocks of a work-group of pass B
constexpr int PB_ROWS = PB_THREADS * PB_SUB;       // 1024 respondents
constexpr int PB_STRIP = 8;                        // items per work-group
constexpr int PU_THREADS = 128;
constexpr int PH_THREADS = 256;
constexpr int PPS_NTAB = 5;                        // Nr | R << 32, Er, Vr, Eo, Vo
constexpr double PPS_FIX = 17592186044416.0;       // 2^44
constexpr double PPS_UNFIX = 1.0 / PPS_FIX;
static_assert(GPIRT_SCORES_MAX_M < 65536 && GPIRT_SCORES_MAX_N < 65536, "a strip partial packs two 16-bit counts");

// type: 'q' 8-byte integer, 'u' uint32, 'd' double; kind: 'h' m + 1, 's' 4 m, 'v' 2, '1' 1, 'i' m, 'c' K m
struct PpsArr { const char* name; char type; char kind; };
const PpsArr kPpsArr[PPS_NARRAYS] = {
    { "hist_obs", 'q', 'h' }, { "sums_obs", 'q', 's' }, { "var_obs", 'q', 'v' }, { "r_obs", 'd', 'i' }, { "tNo", 'u', 'c' }, { "tT", 'u', 'c' },
    { "hist_sum", 'q', 'h' }, { "hist_sumsq", 'q', 'h' }, { "hist_ge", 'u', 'h' }, { "hist_gt", 'u', 'h' }, { "cdf_ge", 'u', 'h' }, { "cdf_gt", 'u', 'h' },
    { "var_ge", 'u', '1' }, { "var_gt", 'u', '1' }, { "var_rep_sum", 'q', '1' },
    { "r_ge", 'u', 'i' }, { "r_gt", 'u', 'i' }, { "r_undefined_count", 'u', 'i' }, { "r_rep_sum", 'd', 'i' }, { "r_rep_sumsq", 'd', 'i' },
    { "cell_ge", 'u', 'c' }, { "cell_gt", 'u', 'c' }, { "cell_empty", 'u', 'c' }, { "sum_nr", 'q', 'c' }, { "sum_r", 'q', 'c' }, { "sum_eo", 'd', 'c' }, { "sum_er", 'd', 'c' },
    { "chi_ge", 'u', 'i' }, { "chi_gt", 'u', 'i' }, { "chi_obs_sum", 'd', 'i' }, { "chi_rep_sum", 'd', 'i' } };
const char* const kPpsHist[GPIRT_SCORES_HIST_NFIELDS] = { "score_hist_obs", "score_hist_rep_mean", "score_hist_rep_sd", "ppp_hist",
                                                          "ppp_hist_mid", "ppp_cdf", "ppp_cdf_mid" };
const char* const kPpsVar[3] = { "score_var_obs", "score_var_rep_mean", "ppp_var" };
const char* const kPpsItem[GPIRT_SCORES_ITEM_NFIELDS] = { "r_rep_mean", "r_rep_sd", "ppp_r", "ppp_r_mid", "r_undefined", "ppp_chi2",
                                                          "ppp_chi2_mid", "chi2_obs_mean", "chi2_rep_mean" };
const char* const kPpsCell[GPIRT_SCORES_CELL_NFIELDS] = { "obs_rate", "rep_rate", "exp_rate", "ppp_cell", "ppp_cell_mid" };

inline int pps_width(int k) { return kPpsArr[k].type == 'u' ? 4 : 8; }
inline int64_t pps_count(int k, int64_t m, int64_t K)
{
    switch (kPpsArr[k].kind) {
        case 'h': return m + 1;
        case 's': return 4 * m;
        case 'v': return 2;
        case '1': return 1;
        case 'i': return m;
        default: return K * m;
    }
}

struct PpsCuts { int K; int c[GPIRT_SCORES_MAX_K - 1]; };

__device__ __forceinline__ int pps_group(const PpsCuts& c, int w)
{
    int k = 0;
#pragma unroll
    for (int q = 0; q < GPIRT_SCORES_MAX_K - 1; ++q) k += (q < c.K - 1 && w >= c.c[q]) ? 1 : 0;
    return k;
}

struct PpsRowArgs {
    const double* f; const double* mu; const double* y;
    int64_t n, m, W;
    uint64_t seed; uint32_t iter, item0;
    unsigned long long* repw;             // [m][W]
    uint32_t* xpart;                      // [strips][n]
    int* bad;
};

template <bool DATA>
__global__ __launch_bounds__(PA_THREADS) void pps_rows_kernel(PpsRowArgs a)
{
    const int rb = blockIdx.x, strip = blockIdx.y;
    const int64_t i = (int64_t)rb * PA_THREADS + threadIdx.x;
    const bool live = i < a.n;
    const int64_t j0 = (int64_t)strip * PA_STRIP;
    const int w = (int)(a.m - j0 < PA_STRIP ? a.m - j0 : PA_STRIP);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t word = (int64_t)rb * (PA_THREADS / 64) + wv;
    uint32_t part = 0;
    for (int jj = 0; jj < w; ++jj) {
        bool bit = false;
        if (live) {
            const int64_t c = i + (j0 + jj) * a.n;
            const double yv = a.y[c];
            if (yv == yv) {                                   // an observed cell
                part += 1u << 16;
                if constexpr (DATA) bit = yv > 0.0;
                else {
                    const double g = a.f[c] + a.mu[c];
                    if (!isfinite(g)) *a.bad = 1;             // (every writer stores the same word)
                    else {
                        const double e = exp(-fabs(g));
                        const double p = g >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
                        const double u = item_uniform(a.seed, a.iter, GPIRT_ST_PPC, (uint32_t)(a.item0 + j0 + jj), (uint32_t)i);
                        bit = u < p;
                    }
                }
            }
        }
        part += bit ? 1u : 0u;
        const unsigned long long v = __ballot(bit ? 1 : 0);   // (every lane of the wave is here: the trip count is uniform)
        if (lane == 0 && word < a.W) a.repw[(j0 + jj) * a.W + word] = v;
    }
    if (live) a.xpart[(int64_t)strip * a.n + i] = part;
}

struct PpsScoreArgs {
    const uint32_t* xpart; int64_t n; int strips; const int* bad;
    int32_t* x; unsigned char* live; uint32_t* hist;
};

template <bool DATA>
__global__ __launch_bounds__(PA_THREADS) void pps_scores_kernel(PpsScoreArgs a)
{
    if (!DATA && *a.bad) return;                               // (the same for every thread of the launch)
    const int64_t i = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
    if (i >= a.n) return;
    uint32_t s = 0;
    for (int q = 0; q < a.strips; ++q) s += a.xpart[(int64_t)q * a.n + i];
    const int32_t X = (int32_t)(s & 0xFFFFu);
    a.x[i] = X;
    if constexpr (DATA) a.live[i] = (s >> 16) ? 1 : 0;
    if (DATA ? (s >> 16) != 0 : a.live[i] != 0) atomicAdd(&a.hist[X], 1u);
}

struct PpsColArgs {
    const double* f; const double* mu; const double* y;
    int64_t n, m, W;
    const unsigned long long* repw;
    const int32_t* x;                     // the grouping score of the plane: Xr (X in the DATA instance)
    const int32_t* x_obs;
    PpsCuts c;
    unsigned long long* tab;              // [PPS_NTAB][K][m]
    unsigned long long* isum;             // [4][m]
    const int* bad;
};

template <bool DATA>
__global__ __launch_bounds__(PB_THREADS) void pps_cols_kernel(PpsColArgs a)
{
    __shared__ unsigned long long sc[PPS_NTAB][PB_STRIP][GPIRT_SCORES_MAX_K];
    __shared__ unsigned long long si[PB_STRIP][4];
    if (!DATA && *a.bad) return;                               // (the same for every thread of the launch)
    const int t = threadIdx.x;
    for (int k = t; k < PPS_NTAB * PB_STRIP * GPIRT_SCORES_MAX_K; k += PB_THREADS) (&sc[0][0][0])[k] = 0ull;
    if (t < PB_STRIP * 4) (&si[0][0])[t] = 0ull;
    __syncthreads();
    const int64_t j0 = (int64_t)blockIdx.y * PB_STRIP;
    const int w = (int)(a.m - j0 < PB_STRIP ? a.m - j0 : PB_STRIP);
    const int K = a.c.K;
    uint32_t sA[PB_STRIP], sB[PB_STRIP], sD[PB_STRIP];
    unsigned long long sQ[PB_STRIP];
#pragma unroll
    for (int jj = 0; jj < PB_STRIP; ++jj) { sA[jj] = sB[jj] = sD[jj] = 0; sQ[jj] = 0; }
    for (int sub = 0; sub < PB_SUB; ++sub) {
        const int64_t i = ((int64_t)blockIdx.x * PB_SUB + sub) * PB_THREADS + t;
        if (i >= a.n) continue;            // (no barrier and no shuffle inside this loop)
        const int xr = a.x[i];
        [[maybe_unused]] const int xo = DATA ? xr : a.x_obs[i];
        const int64_t wd = i >> 6;
        const int sh = (int)(i & 63);
#pragma unroll
        for (int jj = 0; jj < PB_STRIP; ++jj) {
            if (jj >= w) continue;
            const int64_t at = i + (j0 + jj) * a.n;
            const double yv = a.y[at];
            if (!(yv == yv)) continue;                         // not observed
            const uint32_t rep = (uint32_t)((a.repw[(j0 + jj) * a.W + wd] >> sh) & 1ull);
            const uint32_t wr = (uint32_t)xr - rep;
            const int kr = pps_group(a.c, (int)wr);
            sA[jj] += rep; sB[jj] += wr; sD[jj] += rep * wr; sQ[jj] += (unsigned long long)wr * wr;
            atomicAdd(&sc[0][jj][kr], 1ull | ((unsigned long long)rep << 32));
            if constexpr (!DATA) {
                const double g = a.f[at] + a.mu[at];           // finite: pass A has looked at every observed cell
                const double e = exp(-fabs(g));
                const double p = g >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
                const double q = g >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
                const unsigned long long ef = (unsigned long long)rint(p * PPS_FIX), vf = (unsigned long long)rint(p * q * PPS_FIX);
                const int ko = pps_group(a.c, xo - (yv > 0.0 ? 1 : 0));
                atomicAdd(&sc[1][jj][kr], ef);
                atomicAdd(&sc[2][jj][kr], vf);
                atomicAdd(&sc[3][jj][ko], ef);
                atomicAdd(&sc[4][jj][ko], vf);
            }
        }
    }
    // the item sums: a fixed shuffle tree per wave (integers), then one LDS atomic per wave and sum
#pragma unroll
    for (int jj = 0; jj < PB_STRIP; ++jj) {
        unsigned long long v[4] = { sA[jj], sB[jj], sQ[jj], sD[jj] };
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
            if ((t & 63) == 0 && v[q]) atomicAdd(&si[jj][q], v[q]);
        }
    }
    __syncthreads();
    const int64_t C = (int64_t)K * a.m;
    for (int k = t; k < w * K; k += PB_THREADS) {
        const int jj = k / K, kk = k - jj * K;
        const int64_t at = (int64_t)kk * a.m + j0 + jj;
#pragma unroll
        for (int q = 0; q < PPS_NTAB; ++q) {
            const unsigned long long v = sc[q][jj][kk];
            if (v) atomicAdd(&a.tab[q * C + at], v);
        }
    }
    if (t < w * 4) {
        const int jj = t >> 2, q = t & 3;
        const unsigned long long v = si[jj][q];
        if (v) atomicAdd(&a.isum[(int64_t)q * a.m + j0 + jj], v);
    }
}

// r = NUM / sqrt(VA VC) from the five integer sums; false when VA = 0 or VC = 0
__host__ __device__ inline bool pps_r(int64_t N, int64_t A, int64_t B, int64_t Cq, int64_t D, double* r)
{
    const int64_t NUM = N * D - A * B, VA = N * A - A * A, VC = N * Cq - B * B;
    if (VA == 0 || VC == 0) return false;
    const double den = sqrt((double)VA * (double)VC);
    *r = (double)NUM / den;
    return true;
}

__device__ __forceinline__ double pps_x2_term(uint32_t Cn, uint64_t E, uint64_t V)
{
    const double d = (double)((int64_t)((uint64_t)Cn << 44) - (int64_t)E) * PPS_UNFIX;
    const double v = (double)(int64_t)V * PPS_UNFIX;
    const double dd = d * d;
    return dd / v;
}

struct PpsUpdateArgs {
    uint64_t* tab; uint64_t* tab_last; uint64_t* isum; uint64_t* isum_last;
    double* r_last; double* chi_last;
    const int* bad;
    int64_t m; int K;
    uint64_t* block; PpsLayout L;
};

template <bool DATA>
__global__ __launch_bounds__(PU_THREADS) void pps_update_kernel(PpsUpdateArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * PU_THREADS + threadIdx.x;
    const bool skip = !DATA && *a.bad != 0;
    int64_t* hdr = reinterpret_cast<int64_t*>(a.block);
    if (!DATA && j == 0) hdr[skip ? 6 : 5] += 1;               // (nobody else in this launch reads the header)
    if (skip || j >= a.m) return;                              // (a skipped draw has left the tables at zero)
    const int64_t m = a.m, C = (int64_t)a.K * m;
    auto u32 = [&](int k) { return reinterpret_cast<uint32_t*>(a.block + a.L.off[k]); };
    auto u64 = [&](int k) { return a.block + a.L.off[k]; };
    auto f64 = [&](int k) { return reinterpret_cast<double*>(a.block + a.L.off[k]); };
    int64_t S[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        S[q] = (int64_t)a.isum[q * m + j];
        a.isum[q * m + j] = 0;                                 // the next draw starts from zero
        if (DATA) reinterpret_cast<int64_t*>(u64(PPS_SUMS_OBS))[q * m + j] = S[q];
        else a.isum_last[q * m + j] = (uint64_t)S[q];
    }
    int64_t N = 0;
    double x2T = 0.0, x2R = 0.0;
    for (int k = 0; k < a.K; ++k) {
        const int64_t at = (int64_t)k * m + j;
        uint64_t v[PPS_NTAB];
#pragma unroll
        for (int q = 0; q < PPS_NTAB; ++q) {
            v[q] = a.tab[q * C + at];
            a.tab[q * C + at] = 0;
            if (!DATA) a.tab_last[q * C + at] = v[q];
        }
        const uint32_t Nr = (uint32_t)(v[0] & 0xFFFFFFFFull), R = (uint32_t)(v[0] >> 32);
        N += Nr;
        if constexpr (DATA) { u32(PPS_TNO)[at] = Nr; u32(PPS_TT)[at] = R; }
        else {
            const uint32_t No = u32(PPS_TNO)[at], T = u32(PPS_TT)[at];
            u64(PPS_SUM_NR)[at] += Nr; u64(PPS_SUM_R)[at] += R;
            f64(PPS_SUM_EO)[at] += (double)(int64_t)v[3] * PPS_UNFIX;
            f64(PPS_SUM_ER)[at] += (double)(int64_t)v[1] * PPS_UNFIX;
            if (Nr > 0 && No > 0) {
                const uint64_t lhs = (uint64_t)R * No, rhs = (uint64_t)T * Nr;
                u32(PPS_CELL_GE)[at] += lhs >= rhs ? 1u : 0u;
                u32(PPS_CELL_GT)[at] += lhs > rhs ? 1u : 0u;
            } else u32(PPS_CELL_EMPTY)[at] += 1u;
            if (v[4] > 0) x2T += pps_x2_term(T, v[3], v[4]);
            if (v[2] > 0) x2R += pps_x2_term(R, v[1], v[2]);
        }
    }
    double r = (double)NAN;
    const bool ok = pps_r(N, S[0], S[1], S[2], S[3], &r);
    if constexpr (DATA) { f64(PPS_R_OBS)[j] = ok ? r : (double)NAN; return; }
    a.r_last[j] = ok ? r : (double)NAN;
    const double r0 = f64(PPS_R_OBS)[j];
    if (!ok || !(r0 == r0)) u32(PPS_R_UNDEF)[j] += 1u;
    else {
        u32(PPS_R_GE)[j] += r >= r0 ? 1u : 0u;
        u32(PPS_R_GT)[j] += r > r0 ? 1u : 0u;
        f64(PPS_R_REP_SUM)[j] += r;
        const double rr = r * r;
        f64(PPS_R_REP_SUMSQ)[j] += rr;
    }
    u32(PPS_CHI_GE)[j] += x2R >= x2T ? 1u : 0u;
    u32(PPS_CHI_GT)[j] += x2R > x2T ? 1u : 0u;
    f64(PPS_CHI_OBS)[j] += x2T;
    f64(PPS_CHI_REP)[j] += x2R;
    a.chi_last[j] = x2T; a.chi_last[m + j] = x2R;
}

struct PpsHistArgs {
    uint32_t* hist; int64_t* hist_last; const int* bad;
    int64_t m;
    uint64_t* block; PpsLayout L;
};

// one work-group: thread t owns the scores [t c, (t + 1) c), c = ceil((m + 1) / 256)
template <bool DATA>
__global__ __launch_bounds__(PH_THREADS) void pps_hist_kernel(PpsHistArgs a)
{
    __shared__ unsigned long long crep[PH_THREADS], cobs[PH_THREADS];
    __shared__ unsigned long long mom[2];
    if (!DATA && *a.bad) return;                               // (the same for every thread; the histogram was left at zero)
    const int t = threadIdx.x;
    const int64_t len = a.m + 1, c = (len + PH_THREADS - 1) / PH_THREADS;
    const int64_t lo = (int64_t)t * c < len ? (int64_t)t * c : len, hi = lo + c < len ? lo + c : len;
    int64_t* hobs = reinterpret_cast<int64_t*>(a.block + a.L.off[PPS_HIST_OBS]);
    if (t < 2) mom[t] = 0;
    unsigned long long sr = 0, so = 0, s1 = 0, s2 = 0;
    for (int64_t s = lo; s < hi; ++s) {
        const unsigned long long h = a.hist[s];
        sr += h; s1 += (unsigned long long)s * h; s2 += (unsigned long long)(s * s) * h;
        if (!DATA) so += (unsigned long long)hobs[s];
    }
    crep[t] = sr; cobs[t] = so;
    __syncthreads();
    atomicAdd(&mom[0], s1);                                    // integers: any order gives the same sum
    atomicAdd(&mom[1], s2);
    unsigned long long br = 0, bo = 0;
    for (int q = 0; q < t; ++q) { br += crep[q]; bo += cobs[q]; }
    auto u32 = [&](int k) { return reinterpret_cast<uint32_t*>(a.block + a.L.off[k]); };
    auto u64 = [&](int k) { return a.block + a.L.off[k]; };
    for (int64_t s = lo; s < hi; ++s) {
        const unsigned long long h = a.hist[s];
        a.hist[s] = 0;                                         // the next draw starts from zero
        br += h;
        if constexpr (DATA) hobs[s] = (int64_t)h;
        else {
            const unsigned long long ho = (unsigned long long)hobs[s];
            bo += ho;
            a.hist_last[s] = (int64_t)h;
            u64(PPS_HIST_SUM)[s] += h; u64(PPS_HIST_SUMSQ)[s] += h * h;
            u32(PPS_HIST_GE)[s] += h >= ho ? 1u : 0u; u32(PPS_HIST_GT)[s] += h > ho ? 1u : 0u;
            u32(PPS_CDF_GE)[s] += br >= bo ? 1u : 0u; u32(PPS_CDF_GT)[s] += br > bo ? 1u : 0u;
        }
    }
    __syncthreads();
    if (t != PH_THREADS - 1) return;
    // thread 255's running sum holds every score: n_s
    const int64_t ns = (int64_t)br, Vn = ns * (int64_t)mom[1] - (int64_t)mom[0] * (int64_t)mom[0];
    int64_t* vobs = reinterpret_cast<int64_t*>(u64(PPS_VAR_OBS));
    if constexpr (DATA) { vobs[0] = Vn; vobs[1] = ns; }
    else {
        u32(PPS_VAR_GE)[0] += Vn >= vobs[0] ? 1u : 0u;
        u32(PPS_VAR_GT)[0] += Vn > vobs[0] ? 1u : 0u;
        u64(PPS_VAR_REP_SUM)[0] += (uint64_t)Vn;
    }
}

// a state block on the host
struct HostPps {
    std::vector<uint64_t> w;
    int64_t n = 0, m = 0, K = 0;
    PpsLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    const int64_t* cuts() const { return hdr() + PPS_HEADER_WORDS; }
    template <class T> T* arr(int k) { return reinterpret_cast<T*>(w.data() + L.off[k]); }
    template <class T> const T* arr(int k) const { return reinterpret_cast<const T*>(w.data() + L.off[k]); }
    int64_t S() const { return hdr()[5]; }
};

int pps_read(hipStream_t st, const void* d_state, HostPps& r, const char* who, int c)
{
    int64_t hdr[PPS_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] != PPS_TAG || hdr[1] != PPS_LAYOUT_VERSION || hdr[2] <= 0 || hdr[2] > GPIRT_SCORES_MAX_N || hdr[3] < 2 ||
        hdr[3] > GPIRT_SCORES_MAX_M || hdr[4] < 2 || hdr[4] > GPIRT_SCORES_MAX_K || hdr[5] < 0 || hdr[6] < 0) {
        set_error("%s: state %d is not a score-based PPC state block of layout %d", who, c, PPS_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[2]; r.m = hdr[3]; r.K = hdr[4];
    r.L = pps_layout(r.m, r.K);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

double pps_hist_field(const HostPps& r, int fld, int64_t s)
{
    const int64_t S = r.S();
    const double nan = (double)NAN, dS = (double)S;
    auto c = [&](int k) { return (double)r.arr<uint32_t>(k)[s]; };
    if (fld == 0) return (double)r.arr<int64_t>(PPS_HIST_OBS)[s];
    if (S < 1) return nan;
    switch (fld) {
        case 1: return (double)r.arr<uint64_t>(PPS_HIST_SUM)[s] / dS;
        case 2: {
            if (S < 2) return nan;
            // S sum H^2 - (sum H)^2 >= 0, exact in 128 bits, rounded once
            const unsigned __int128 a = (unsigned __int128)(uint64_t)S * r.arr<uint64_t>(PPS_HIST_SUMSQ)[s];
            const unsigned __int128 b = (unsigned __int128)r.arr<uint64_t>(PPS_HIST_SUM)[s] * r.arr<uint64_t>(PPS_HIST_SUM)[s];
            const double q = (double)(a - b) / (dS * (double)(S - 1));
            return sqrt(q);
        }
        case 3: return c(PPS_HIST_GE) / dS;
        case 4: return (c(PPS_HIST_GE) + c(PPS_HIST_GT)) / (2.0 * dS);
        case 5: return c(PPS_CDF_GE) / dS;
        case 6: return (c(PPS_CDF_GE) + c(PPS_CDF_GT)) / (2.0 * dS);
        default: break;
    }
    return nan;
}

double pps_var_field(const HostPps& r, int fld)
{
    const int64_t S = r.S(), ns = r.arr<int64_t>(PPS_VAR_OBS)[1];
    const double nan = (double)NAN;
    if (ns < 1) return nan;
    const double n2 = (double)ns * (double)ns;
    switch (fld) {
        case 0: return (double)r.arr<int64_t>(PPS_VAR_OBS)[0] / n2;
        case 1: return S >= 1 ? (double)r.arr<uint64_t>(PPS_VAR_REP_SUM)[0] / ((double)S * n2) : nan;
        case 2: return S >= 1 ? (double)r.arr<uint32_t>(PPS_VAR_GE)[0] / (double)S : nan;
        default: break;
    }
    return nan;
}

double pps_item_field(const HostPps& r, int fld, int64_t j)
{
    const int64_t S = r.S();
    const double nan = (double)NAN, dS = (double)S;
    auto c = [&](int k) { return (double)r.arr<uint32_t>(k)[j]; };
    const int64_t Sr = S - (int64_t)r.arr<uint32_t>(PPS_R_UNDEF)[j];
    const double sum = r.arr<double>(PPS_R_REP_SUM)[j];
    switch (fld) {
        case 0: return Sr >= 1 ? sum / (double)Sr : nan;
        case 1: {
            if (Sr < 2) return nan;
            const double mean = sum / (double)Sr, sm = sum * mean;
            const double v = (r.arr<double>(PPS_R_REP_SUMSQ)[j] - sm) / (double)(Sr - 1);
            return v > 0.0 ? sqrt(v) : 0.0;
        }
        case 2: return Sr >= 1 ? c(PPS_R_GE) / (double)Sr : nan;
        case 3: return Sr >= 1 ? (c(PPS_R_GE) + c(PPS_R_GT)) / (2.0 * (double)Sr) : nan;
        case 4: return c(PPS_R_UNDEF);
        case 5: return S >= 1 ? c(PPS_CHI_GE) / dS : nan;
        case 6: return S >= 1 ? (c(PPS_CHI_GE) + c(PPS_CHI_GT)) / (2.0 * dS) : nan;
        case 7: return S >= 1 ? r.arr<double>(PPS_CHI_OBS)[j] / dS : nan;
        case 8: return S >= 1 ? r.arr<double>(PPS_CHI_REP)[j] / dS : nan;
        default: break;
    }
    return nan;
}

double pps_cell_field(const HostPps& r, int fld, int64_t at)
{
    const int64_t S = r.S();
    const double nan = (double)NAN;
    const uint32_t No = r.arr<uint32_t>(PPS_TNO)[at];
    const int64_t Sc = S - (int64_t)r.arr<uint32_t>(PPS_CELL_EMPTY)[at];
    auto c = [&](int k) { return (double)r.arr<uint32_t>(k)[at]; };
    switch (fld) {
        case 0: return No > 0 ? (double)r.arr<uint32_t>(PPS_TT)[at] / (double)No : nan;
        case 1: {
            const uint64_t sn = r.arr<uint64_t>(PPS_SUM_NR)[at];
            return sn > 0 ? (double)r.arr<uint64_t>(PPS_SUM_R)[at] / (double)sn : nan;
        }
        case 2: return (S >= 1 && No > 0) ? r.arr<double>(PPS_SUM_EO)[at] / ((double)S * (double)No) : nan;
        case 3: return Sc >= 1 ? c(PPS_CELL_GE) / (double)Sc : nan;
        case 4: return Sc >= 1 ? (c(PPS_CELL_GE) + c(PPS_CELL_GT)) / (2.0 * (double)Sc) : nan;
        default: break;
    }
    return nan;
}

int64_t pps_group_edge(const HostPps& r, bool hi, int64_t k)
{
    if (!hi) return k == 0 ? 0 : r.cuts()[k - 1];
    return k == r.K - 1 ? r.m - 1 : r.cuts()[k] - 1;
}

void pps_fill(const HostPps& r, gpirt_ppc_scores* out)
{
    const int64_t m = r.m, K = r.K;
    out->n = r.n; out->m = m; out->K = (int)K; out->score_draws = r.hdr()[5]; out->score_skipped = r.hdr()[6];
    out->n_scored = r.arr<int64_t>(PPS_VAR_OBS)[1];
    for (int q = 0; q < GPIRT_SCORES_MAX_K; ++q) out->cuts[q] = q < K - 1 ? (int)r.cuts()[q] : 0;
    for (int fld = 0; fld < GPIRT_SCORES_HIST_NFIELDS; ++fld)
        if (out->hist[fld]) for (int64_t s = 0; s <= m; ++s) out->hist[fld][s] = pps_hist_field(r, fld, s);
    if (out->var) for (int fld = 0; fld < 3; ++fld) out->var[fld] = pps_var_field(r, fld);
    for (int fld = 0; fld < GPIRT_SCORES_ITEM_NFIELDS; ++fld)
        if (out->item[fld]) for (int64_t j = 0; j < m; ++j) out->item[fld][j] = pps_item_field(r, fld, j);
    for (int fld = 0; fld < GPIRT_SCORES_CELL_NFIELDS; ++fld)
        if (out->cell[fld]) for (int64_t at = 0; at < K * m; ++at) out->cell[fld][at] = pps_cell_field(r, fld, at);
    for (int k = 0; k < PPS_NARRAYS; ++k)
        if (out->raw[k]) memcpy(out->raw[k], r.w.data() + r.L.off[k], (size_t)(pps_count(k, m, K) * pps_width(k)));
    for (int64_t k = 0; k < K; ++k) {
        if (out->group_lo) out->group_lo[k] = pps_group_edge(r, false, k);
        if (out->group_hi) out->group_hi[k] = pps_group_edge(r, true, k);
    }
    if (!out->worst_items && !out->worst_ppp_chi2_mid) return;
    // the items by increasing ppp_chi2_mid, ties to the lowest j: a stable sort
    struct E { double mid; int64_t j; };
    std::vector<E> es;
    for (int64_t j = 0; j < m; ++j) {
        const double mid = pps_item_field(r, 6, j);
        if (mid == mid) es.push_back(E{ mid, j });
    }
    std::stable_sort(es.begin(), es.end(), [](const E& x, const E& y) { return x.mid < y.mid; });
    for (int t = 0; t < out->top; ++t) {
        const bool have = (size_t)t < es.size();
        if (out->worst_items) out->worst_items[t] = have ? es[(size_t)t].j : -1;
        if (out->worst_ppp_chi2_mid) out->worst_ppp_chi2_mid[t] = have ? es[(size_t)t].mid : (double)NAN;
    }
}

PpsCuts pps_cuts(const PpsState* p)
{
    PpsCuts c{};
    c.K = p->K;
    for (int q = 0; q < p->K - 1; ++q) c.c[q] = p->cuts[q];
    return c;
}

template <bool DATA>
int pps_launch(hipStream_t st, PpsState* p, const double* f, const double* mu, const double* y, uint64_t seed, uint32_t iter)
{
    const PpsLayout L = pps_layout(p->m, p->K);
    if (!DATA) GP_HIP(hipMemsetAsync(p->ctl, 0, sizeof(int), st));
    PpsRowArgs r{};
    r.f = f; r.mu = mu; r.y = y; r.n = p->n; r.m = p->m; r.W = p->W; r.seed = seed; r.iter = iter; r.item0 = (uint32_t)p->item0;
    r.repw = reinterpret_cast<unsigned long long*>(p->repw); r.xpart = p->xpart; r.bad = p->ctl;
    const unsigned rblocks = (unsigned)((p->n + PA_THREADS - 1) / PA_THREADS);
    hipLaunchKernelGGL((pps_rows_kernel<DATA>), dim3(rblocks, (unsigned)p->strips), dim3(PA_THREADS), 0, st, r);
    GP_HIP(hipGetLastError());
    PpsScoreArgs s{};
    s.xpart = p->xpart; s.n = p->n; s.strips = p->strips; s.bad = p->ctl; s.x = DATA ? p->x_obs : p->xr; s.live = p->live;
    s.hist = p->hist_cur;
    hipLaunchKernelGGL((pps_scores_kernel<DATA>), dim3(rblocks), dim3(PA_THREADS), 0, st, s);
    GP_HIP(hipGetLastError());
    PpsColArgs c{};
    c.f = f; c.mu = mu; c.y = y; c.n = p->n; c.m = p->m; c.W = p->W;
    c.repw = reinterpret_cast<const unsigned long long*>(p->repw); c.x = DATA ? p->x_obs : p->xr; c.x_obs = p->x_obs;
    c.c = pps_cuts(p); c.tab = reinterpret_cast<unsigned long long*>(p->tab); c.isum = reinterpret_cast<unsigned long long*>(p->isum);
    c.bad = p->ctl;
    const dim3 grid((unsigned)((p->n + PB_ROWS - 1) / PB_ROWS), (unsigned)((p->m + PB_STRIP - 1) / PB_STRIP));
    hipLaunchKernelGGL((pps_cols_kernel<DATA>), grid, dim3(PB_THREADS), 0, st, c);
    GP_HIP(hipGetLastError());
    PpsUpdateArgs u{};
    u.tab = p->tab; u.tab_last = p->tab_last; u.isum = p->isum; u.isum_last = p->isum_last; u.r_last = p->r_last;
    u.chi_last = p->chi_last; u.bad = p->ctl; u.m = p->m; u.K = p->K; u.block = p->block; u.L = L;
    hipLaunchKernelGGL((pps_update_kernel<DATA>), dim3((unsigned)((p->m + PU_THREADS - 1) / PU_THREADS)), dim3(PU_THREADS), 0, st, u);
    GP_HIP(hipGetLastError());
    PpsHistArgs h{};
    h.hist = p->hist_cur; h.hist_last = p->hist_last; h.bad = p->ctl; h.m = p->m; h.block = p->block; h.L = L;
    hipLaunchKernelGGL((pps_hist_kernel<DATA>), dim3(1), dim3(PH_THREADS), 0, st, h);
    GP_HIP(hipGetLastError());
    return 0;
}

}  // namespace

PpsLayout pps_layout(int64_t m, int64_t K)
{
    PpsLayout L{};
    int64_t at = PPS_HEADER_WORDS + PPS_CUT_WORDS;
    for (int k = 0; k < PPS_NARRAYS; ++k) {
        L.off[k] = at;
        const int64_t bytes = pps_count(k, m, K) * pps_width(k);
        at += (bytes + 15) / 16 * 2;                                  // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int64_t pps_state_words(const PpsState* p) { return pps_layout(p->m, p->K).words; }

int pps_check(int64_t n, int64_t m, int K, const int* cuts)
{
    if (m < 2 || m > GPIRT_SCORES_MAX_M) {
        set_error("score-based PPC: m = %lld is outside 2..%d items", (long long)m, GPIRT_SCORES_MAX_M);
        return GPIRT_E_ARG;
    }
    if (n < 1 || n > GPIRT_SCORES_MAX_N) {
        set_error("score-based PPC: n = %lld is beyond %d respondents", (long long)n, GPIRT_SCORES_MAX_N);
        return GPIRT_E_ARG;
    }
    if (K < 2 || K > GPIRT_SCORES_MAX_K || !cuts) {
        set_error("score-based PPC: %d score groups given, 2..%d are taken (K - 1 cuts)", K, GPIRT_SCORES_MAX_K);
        return GPIRT_E_ARG;
    }
    for (int q = 0; q < K - 1; ++q)
        if (cuts[q] < 1 || cuts[q] > m - 1 || (q > 0 && cuts[q] <= cuts[q - 1])) {
            set_error("score-based PPC: the cuts must be increasing integers in 1..%lld (cut %d is %d)", (long long)(m - 1), q + 1, cuts[q]);
            return GPIRT_E_ARG;
        }
    return 0;
}

void pps_free(PpsState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = PpsState{};
}

int pps_alloc(hipStream_t st, PpsState* p, int64_t n, int64_t m, int64_t item0, const double* y, int K, const int* cuts)
{
    GP_TRY(pps_check(n, m, K, cuts));
    const PpsLayout L = pps_layout(m, K);
    p->n = n; p->m = m; p->item0 = item0; p->K = K; p->W = (n + 63) / 64; p->strips = (int)((m + PA_STRIP - 1) / PA_STRIP);
    for (int q = 0; q < K - 1; ++q) p->cuts[q] = cuts[q];
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    const size_t N = (size_t)n, M = (size_t)m, C = (size_t)K * M;
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->repw, sizeof(uint64_t) * M * (size_t)p->W));
    GP_TRY(get((void**)&p->xpart, sizeof(uint32_t) * (size_t)p->strips * N));
    GP_TRY(get((void**)&p->x_obs, sizeof(int32_t) * N));
    GP_TRY(get((void**)&p->xr, sizeof(int32_t) * N));
    GP_TRY(get((void**)&p->live, N));
    GP_TRY(get((void**)&p->hist_cur, sizeof(uint32_t) * (M + 1)));
    GP_TRY(get((void**)&p->hist_last, sizeof(int64_t) * (M + 1)));
    GP_TRY(get((void**)&p->ctl, sizeof(int) * 4));
    GP_TRY(get((void**)&p->tab, sizeof(uint64_t) * PPS_NTAB * C));
    GP_TRY(get((void**)&p->tab_last, sizeof(uint64_t) * PPS_NTAB * C));
    GP_TRY(get((void**)&p->isum, sizeof(uint64_t) * 4 * M));
    GP_TRY(get((void**)&p->isum_last, sizeof(uint64_t) * 4 * M));
    GP_TRY(get((void**)&p->r_last, sizeof(double) * M));
    GP_TRY(get((void**)&p->chi_last, sizeof(double) * 2 * M));
    int64_t head[PPS_HEADER_WORDS + PPS_CUT_WORDS] = { PPS_TAG, PPS_LAYOUT_VERSION, n, m, K, 0, 0, 0 };
    for (int q = 0; q < K - 1; ++q) head[PPS_HEADER_WORDS + q] = cuts[q];
    GP_HIP(hipMemcpyAsync(p->block, head, sizeof(head), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // head is this call's: nothing below may leave with the copy pending
    GP_TRY(pps_launch<true>(st, p, nullptr, nullptr, y, 0, 0));       // the constants
    p->on = true;
    return 0;
}

int launch_pps_accumulate(hipStream_t st, PpsState* p, const double* f, const double* mu, const double* y, uint64_t seed,
                          uint32_t iter)
{
    return pps_launch<false>(st, p, f, mu, y, seed, iter);
}

int pps_get(hipStream_t st, PpsState* p, const char* name, void* h_out, int64_t bytes)
{
    const int64_t n = p->n, m = p->m, K = p->K, C = K * m;
    const PpsLayout L = pps_layout(m, K);
    auto copy = [&](const void* src, void* dst, int64_t nb) -> int {
        GP_HIP(hipMemcpyAsync(dst, src, (size_t)nb, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 16); return copy(p->block + 5, h_out, bytes); }
    if (strcmp(name, "cuts") == 0) { GP_ARG(bytes == 8 * (K - 1)); return copy(p->block + PPS_HEADER_WORDS, h_out, bytes); }
    if (strcmp(name, "x_obs") == 0) { GP_ARG(bytes == 4 * n); return copy(p->x_obs, h_out, bytes); }
    if (strcmp(name, "xr") == 0) { GP_ARG(bytes == 4 * n); return copy(p->xr, h_out, bytes); }
    if (strcmp(name, "hist") == 0) { GP_ARG(bytes == 8 * (m + 1)); return copy(p->hist_last, h_out, bytes); }
    if (strcmp(name, "sums") == 0) { GP_ARG(bytes == 8 * 4 * m); return copy(p->isum_last, h_out, bytes); }
    if (strcmp(name, "r") == 0) { GP_ARG(bytes == 8 * m); return copy(p->r_last, h_out, bytes); }
    if (strcmp(name, "chi") == 0) { GP_ARG(bytes == 8 * 2 * m); return copy(p->chi_last, h_out, bytes); }
    static const char* const kTab[4] = { "tEr", "tVr", "tEo", "tVo" };
    for (int q = 0; q < 4; ++q)
        if (strcmp(name, kTab[q]) == 0) { GP_ARG(bytes == 8 * C); return copy(p->tab_last + (q + 1) * C, h_out, bytes); }
    if (strcmp(name, "tNr") == 0 || strcmp(name, "tR") == 0) {
        GP_ARG(bytes == 4 * C);
        std::vector<uint64_t> pk((size_t)C);
        GP_TRY(copy(p->tab_last, pk.data(), 8 * C));
        uint32_t* out = static_cast<uint32_t*>(h_out);
        const int sh = name[1] == 'R' ? 32 : 0;
        for (int64_t at = 0; at < C; ++at) out[at] = (uint32_t)((pk[(size_t)at] >> sh) & 0xFFFFFFFFull);
        return 0;
    }
    for (int k = 0; k < PPS_NARRAYS; ++k)
        if (strcmp(kPpsArr[k].name, name) == 0) {
            GP_ARG(bytes == pps_count(k, m, K) * pps_width(k));
            return copy(p->block + L.off[k], h_out, bytes);
        }
    int hist = -1, var = -1, item = -1, cell = -1;
    for (int k = 0; k < GPIRT_SCORES_HIST_NFIELDS; ++k) if (strcmp(kPpsHist[k], name) == 0) hist = k;
    for (int k = 0; k < 3; ++k) if (strcmp(kPpsVar[k], name) == 0) var = k;
    for (int k = 0; k < GPIRT_SCORES_ITEM_NFIELDS; ++k) if (strcmp(kPpsItem[k], name) == 0) item = k;
    for (int k = 0; k < GPIRT_SCORES_CELL_NFIELDS; ++k) if (strcmp(kPpsCell[k], name) == 0) cell = k;
    const bool lo = strcmp(name, "group_lo") == 0, hi = strcmp(name, "group_hi") == 0;
    if (hist < 0 && var < 0 && item < 0 && cell < 0 && !lo && !hi) {
        set_error("unknown score-based PPC field '%s'", name);
        return GPIRT_E_ARG;
    }
    GP_ARG(bytes == 8 * (hist >= 0 ? m + 1 : var >= 0 ? 1 : item >= 0 ? m : cell >= 0 ? C : K));
    HostPps r;
    GP_TRY(pps_read(st, p->block, r, "gpirt_sampler_ppc_scores_get", 0));
    double* out = static_cast<double*>(h_out);
    if (hist >= 0) for (int64_t s = 0; s <= m; ++s) out[s] = pps_hist_field(r, hist, s);
    else if (var >= 0) out[0] = pps_var_field(r, var);
    else if (item >= 0) for (int64_t j = 0; j < m; ++j) out[j] = pps_item_field(r, item, j);
    else if (cell >= 0) for (int64_t at = 0; at < C; ++at) out[at] = pps_cell_field(r, cell, at);
    else for (int64_t k = 0; k < K; ++k) static_cast<int64_t*>(h_out)[k] = pps_group_edge(r, hi, k);
    return 0;
}

int pps_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_scores* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_SCORES_MAX_TOP) {
        set_error("score-based PPC: top = %d is outside 1..%d", out->top, GPIRT_SCORES_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    HostPps pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostPps& r = c == 0 ? pooled : one;
        GP_TRY(pps_read(h->stream, d_states[c], r, "gpirt_ppc_scores_combine", c));
        if (c == 0) continue;
        // the constants (hist_obs .. tT) lie between the cuts and the first accumulator: another response matrix shows there
        if (r.n != pooled.n || r.m != pooled.m || r.K != pooled.K ||
            memcmp(r.w.data() + PPS_HEADER_WORDS, pooled.w.data() + PPS_HEADER_WORDS,
                   sizeof(uint64_t) * (size_t)(r.L.off[PPS_HIST_SUM] - PPS_HEADER_WORDS)) != 0) {
            set_error("gpirt_ppc_scores_combine: state %d has another n, m, K, cuts or response matrix than state 0", c);
            return GPIRT_E_ARG;
        }
        pooled.hdr()[5] += one.hdr()[5];
        pooled.hdr()[6] += one.hdr()[6];
        for (int k = PPS_HIST_SUM; k < PPS_NARRAYS; ++k) {
            const int64_t cnt = pps_count(k, r.m, r.K);
            if (kPpsArr[k].type == 'd') for (int64_t g = 0; g < cnt; ++g) pooled.arr<double>(k)[g] += one.arr<double>(k)[g];      // in chain order
            else if (kPpsArr[k].type == 'u') for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
            else for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint64_t>(k)[g] += one.arr<uint64_t>(k)[g];
        }
    }
    pps_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
