// acf.hip -- autocorrelation ESS without stored draws (include/gpirt_hip.h, "autocorrelation ESS"): per
// tracked value the lag products s_k = sum_t d_t d_{t-k}, k = 0 .. L, of each split half, kept one draw at a time from a ring of
// the last L + 1 draws, and at the end Geyer's initial monotone sequence over the 2C half-chains.
//
//   acf_ll_kernel       one pass over y, f and mu, lanes along i: work-group (b, q) owns 256 rows x 32 columns; a lane's row
//                       sum stays in a register, each column's 256 rows are summed by a fixed tree (wave shuffles, then the four
//                       waves through LDS) into the work-group's own partial
//   acf_fold_kernel     item_ll[j] and resp_ll[i]: the partials in work-group order; acf_total_kernel: item_ll in item order
//   acf_gather_kernel   thread p: the draw's value -> d_t into the ring's slot, the running sum, head[t]; the first draw sets the
//                       centre
//   acf_lag_kernel<T>   thread (p, chunk of 16 lags): s[k][p] += d_t d_{t-k} in place, reads coalesced across p, 8 bytes per lane;
//                       T = int64 for theta's section, double for the rest; the lag range depends on the draw number only
//   acf_tail_kernel<T>  at a half's last draw: tail[k][p] from the ring, backwards
//   acf_finish_kernel   thread p over the chains' blocks: gamma, W, var+, rho_k, Geyer's pairs, the outputs
//   acf_block_kernel, acf_top_kernel   the block folds (min / max / counts: order-free) and the `top` smallest ess
// No atomics anywhere; every accumulator cell has one owner and every floating-point sum a fixed order.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace gpirt {

namespace {

constexpr int ACF_THREADS = 256;
constexpr int ACF_LL_COLS = 32;                  // columns of a work-group of the log-likelihood pass
constexpr int ACF_KCHUNK = 16;                   // lags per thread of the lag kernel

const char* const kAcfRaw[GPIRT_ACF_NARRAYS] = { "s", "sum", "head", "tail", "centre", "nonfinite", "ring" };

inline int64_t acf_raw_words(int k, int64_t P, int64_t L)
{
    switch (k) {
        case GPIRT_ACF_S: case GPIRT_ACF_HEAD: case GPIRT_ACF_TAIL: return 2 * (L + 1) * P;
        case GPIRT_ACF_SUM: return 2 * P;
        case GPIRT_ACF_RING: return (L + 1) * P;
        default: return P;
    }
}

struct AcfDims {
    int64_t n, m, P, Pi, nbeta, o_item, o_resp, o_total;      // Pi: theta's values (the integer section), then beta, then ll
};

AcfDims acf_dims(int64_t n, int64_t m, int parts)
{
    AcfDims d{};
    d.n = n; d.m = m;
    d.Pi = (parts & GPIRT_ACF_THETA) ? n : 0;
    d.nbeta = (parts & GPIRT_ACF_BETA) ? 2 * m : 0;
    d.o_item = d.Pi + d.nbeta;
    d.o_resp = d.o_item + m;
    d.o_total = d.o_resp + n;
    d.P = (parts & GPIRT_ACF_LL) ? d.o_total + 1 : d.o_item;
    return d;
}

// ---- the log-likelihood series ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ACF_THREADS) void acf_ll_kernel(const double* __restrict__ f, const double* __restrict__ mu,
                                                             const double* __restrict__ y, int64_t n, int64_t m,
                                                             double* __restrict__ cpart, double* __restrict__ rpart)
{
    __shared__ double sh[ACF_LL_COLS][4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * ACF_THREADS + t;
    const int64_t j0 = (int64_t)blockIdx.y * ACF_LL_COLS, j1 = j0 + ACF_LL_COLS < m ? j0 + ACF_LL_COLS : m;
    double row = 0.0;
    for (int64_t j = j0; j < j1; ++j) {
        double c = 0.0;
        if (i < n) {
            const int64_t at = i + j * n;
            const double yv = y[at];
            if (yv == yv) {
                const double g = f[at] + mu[at];
                const double a = yv * g;
                c = -(log1p(exp(-fabs(g))) + fmax(-a, 0.0));
            }
        }
        row += c;
        double v = c;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) sh[j - j0][w] = v;
    }
    if (i < n) rpart[(int64_t)blockIdx.y * n + i] = row;
    __syncthreads();
    if (t < j1 - j0) cpart[(int64_t)blockIdx.x * m + j0 + t] = (sh[t][0] + sh[t][1]) + (sh[t][2] + sh[t][3]);
}

__global__ __launch_bounds__(ACF_THREADS) void acf_fold_kernel(const double* __restrict__ cpart, const double* __restrict__ rpart,
                                                               int64_t n, int64_t m, int nb, int nq, double* __restrict__ item,
                                                               double* __restrict__ resp)
{
    const int64_t e = (int64_t)blockIdx.x * ACF_THREADS + threadIdx.x;
    if (e < m) {
        double acc = 0.0;
        for (int b = 0; b < nb; ++b) acc += cpart[(int64_t)b * m + e];
        item[e] = acc;
    } else if (e < m + n) {
        const int64_t i = e - m;
        double acc = 0.0;
        for (int q = 0; q < nq; ++q) acc += rpart[(int64_t)q * n + i];
        resp[i] = acc;
    }
}

__global__ __launch_bounds__(ACF_THREADS) void acf_total_kernel(const double* __restrict__ item, int64_t m, double* __restrict__ total)
{
    __shared__ double sh[ACF_THREADS];
    double acc = 0.0;
    for (int64_t j0 = 0; j0 < m; j0 += ACF_THREADS) {
        __syncthreads();
        if (j0 + threadIdx.x < m) sh[threadIdx.x] = item[j0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = (int)(m - j0 < ACF_THREADS ? m - j0 : ACF_THREADS);
            for (int q = 0; q < cnt; ++q) acc += sh[q];
        }
    }
    if (threadIdx.x == 0) *total = acc;
}

// ---- one draw into the ring and the running sums ---------------------------------------------------------------------------
struct AcfBlock {
    int64_t* hdr;
    uint64_t *s, *sum, *head, *tail, *ring;       // 8-byte cells: int64 for p < Pi, double from there on
    double* centre;
    int64_t* nonfinite;
};

AcfBlock acf_block(uint64_t* block, const AcfLayout& L)
{
    AcfBlock b;
    b.hdr = reinterpret_cast<int64_t*>(block);
    b.s = block + L.off[GPIRT_ACF_S];
    b.sum = block + L.off[GPIRT_ACF_SUM];
    b.head = block + L.off[GPIRT_ACF_HEAD];
    b.tail = block + L.off[GPIRT_ACF_TAIL];
    b.ring = block + L.off[GPIRT_ACF_RING];
    b.centre = reinterpret_cast<double*>(block + L.off[GPIRT_ACF_CENTRE]);
    b.nonfinite = reinterpret_cast<int64_t*>(block + L.off[GPIRT_ACF_NONFINITE]);
    return b;
}

// half: 0 (the middle draw of an odd S: only `last` and the header's count), 1 or 2; t = the draw's number within the half
__global__ __launch_bounds__(ACF_THREADS) void acf_gather_kernel(AcfBlock b, AcfDims d, const double* __restrict__ theta,
                                                                 const double* __restrict__ beta, double* __restrict__ last,
                                                                 int half, int64_t t, int64_t L, int first)
{
    const int64_t p = (int64_t)blockIdx.x * ACF_THREADS + threadIdx.x;
    if (p == 0) b.hdr[9] += 1;
    if (p >= d.P) return;
    double x;
    if (p < d.Pi) { x = theta[p]; last[p] = x; }
    else if (p < d.o_item) { x = beta[p - d.Pi]; last[p] = x; }
    else x = last[p];                                                 // the fold kernels' item_ll, resp_ll, total_ll
    if (!half) return;
    const int64_t R = L + 1, slot = (t - 1) % R, hp = (int64_t)(half - 1);
    if (p < d.Pi) {
        const double k = rint((x + 5.0) * 100.0);
        const bool ok = k >= 0.0 && k <= (double)(GPIRT_NGRID - 1) && -5.0 + k * 0.01 == x;
        const int64_t dv = ok ? (int64_t)k - (GPIRT_NGRID - 1) / 2 : 0;
        if (!ok) b.nonfinite[p] += 1;
        reinterpret_cast<int64_t*>(b.ring)[slot * d.P + p] = dv;
        int64_t* sum = reinterpret_cast<int64_t*>(b.sum) + hp * d.P + p;
        const int64_t sv = *sum + dv;
        *sum = sv;
        if (t <= L) reinterpret_cast<int64_t*>(b.head)[(hp * R + t) * d.P + p] = sv;
    } else {
        const bool ok = fabs(x) <= DBL_MAX;
        double c;
        if (first) { c = ok ? x : 0.0; b.centre[p] = c; }
        else c = b.centre[p];
        const double dv = ok ? x - c : 0.0;
        if (!ok) b.nonfinite[p] += 1;
        reinterpret_cast<double*>(b.ring)[slot * d.P + p] = dv;
        double* sum = reinterpret_cast<double*>(b.sum) + hp * d.P + p;
        const double sv = *sum + dv;
        *sum = sv;
        if (t <= L) reinterpret_cast<double*>(b.head)[(hp * R + t) * d.P + p] = sv;
    }
}

// s[k][p] += d_t d_{t-k} for the values p0 <= p < p1 and the lags of chunk blockIdx.y, k <= kmax = min(L, t - 1)
template <typename T>
__global__ __launch_bounds__(ACF_THREADS) void acf_lag_kernel(const T* __restrict__ ring, T* __restrict__ s, int64_t P, int64_t p0,
                                                              int64_t p1, int64_t t, int64_t R, int64_t kmax)
{
    const int64_t p = p0 + (int64_t)blockIdx.x * ACF_THREADS + threadIdx.x;
    if (p >= p1) return;
    const int64_t k0 = (int64_t)blockIdx.y * ACF_KCHUNK, k1 = k0 + ACF_KCHUNK - 1 < kmax ? k0 + ACF_KCHUNK - 1 : kmax;
    const T x0 = ring[((t - 1) % R) * P + p];
    int64_t slot = (t - 1 - k0) % R;
    for (int64_t k = k0; k <= k1; ++k) {
        const T prod = x0 * ring[slot * P + p];
        s[k * P + p] += prod;
        slot = slot == 0 ? R - 1 : slot - 1;
    }
}

// the half's last draw (t = H): tail[k][p] = d_H + d_{H-1} + ... + d_{H-k+1}
template <typename T>
__global__ __launch_bounds__(ACF_THREADS) void acf_tail_kernel(const T* __restrict__ ring, T* __restrict__ tail, int64_t P, int64_t p0,
                                                               int64_t p1, int64_t H, int64_t R, int64_t L)
{
    const int64_t p = p0 + (int64_t)blockIdx.x * ACF_THREADS + threadIdx.x;
    if (p >= p1) return;
    T acc = 0;
    for (int64_t k = 1; k <= L; ++k) {
        acc += ring[((H - k) % R) * P + p];
        tail[k * P + p] = acc;
    }
}

// ---- the finish ------------------------------------------------------------------------------------------------------------
struct AcfFinish {
    const uint64_t* const* blocks;    // C
    const int* signs;                 // C
    int64_t off[GPIRT_ACF_NARRAYS];
    AcfDims d;
    int64_t H, L;
    int C;
    double* value;                    // [NVALUE][P]
    int64_t* flag;                    // [NFLAG][P]
    double* acf;                      // [L + 1][P]
};

__device__ __forceinline__ double acf_cell(const uint64_t* a, int64_t at, bool integer)
{
    return integer ? (double)reinterpret_cast<const int64_t*>(a)[at] : reinterpret_cast<const double*>(a)[at];
}

// mean over the 2C half-chains of gamma_k (in half-chain order)
__device__ __forceinline__ double acf_gamma_mean(const AcfFinish& a, int64_t p, int64_t k, bool integer, bool flips)
{
    const int64_t P = a.d.P, R = a.L + 1;
    const double Hd = (double)a.H;
    double acc = 0.0;
    for (int c = 0; c < 2 * a.C; ++c) {
        const uint64_t* blk = a.blocks[c >> 1];
        const int64_t hp = c & 1;
        const double sg = flips ? (double)a.signs[c >> 1] : 1.0;
        const double sum = sg * acf_cell(blk + a.off[GPIRT_ACF_SUM], hp * P + p, integer);
        const double sk = acf_cell(blk + a.off[GPIRT_ACF_S], (hp * R + k) * P + p, integer);
        const double hd = sg * acf_cell(blk + a.off[GPIRT_ACF_HEAD], (hp * R + k) * P + p, integer);
        const double tl = sg * acf_cell(blk + a.off[GPIRT_ACF_TAIL], (hp * R + k) * P + p, integer);
        const double dbar = sum / Hd;
        const double cross = dbar * ((sum - tl) + (sum - hd));
        const double sq = ((double)(a.H - k) * dbar) * dbar;
        acc += ((sk - cross) + sq) / Hd;
    }
    return acc / (double)(2 * a.C);
}

__global__ __launch_bounds__(ACF_THREADS) void acf_finish_kernel(AcfFinish a)
{
    const int64_t p = (int64_t)blockIdx.x * ACF_THREADS + threadIdx.x;
    const int64_t P = a.d.P;
    if (p >= P) return;
    const bool integer = p < a.d.Pi;
    const bool flips = integer || (p < a.d.o_item && ((p - a.d.Pi) & 1));
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double Hd = (double)a.H;
    const int M = 2 * a.C;
    // the half means, their mean and variance (two passes), the non-finite count
    double msum = 0.0;
    int64_t bad = 0;
    for (int c = 0; c < M; ++c) {
        const uint64_t* blk = a.blocks[c >> 1];
        const double sg = flips ? (double)a.signs[c >> 1] : 1.0;
        const double cen = sg * reinterpret_cast<const double*>(blk + a.off[GPIRT_ACF_CENTRE])[p];
        const double sum = sg * acf_cell(blk + a.off[GPIRT_ACF_SUM], (int64_t)(c & 1) * P + p, integer);
        msum += cen + sum / Hd;
        if (!(c & 1)) bad += reinterpret_cast<const int64_t*>(blk + a.off[GPIRT_ACF_NONFINITE])[p];
    }
    const double mean = msum / (double)M;
    double dev = 0.0;
    for (int c = 0; c < M; ++c) {
        const uint64_t* blk = a.blocks[c >> 1];
        const double sg = flips ? (double)a.signs[c >> 1] : 1.0;
        const double cen = sg * reinterpret_cast<const double*>(blk + a.off[GPIRT_ACF_CENTRE])[p];
        const double sum = sg * acf_cell(blk + a.off[GPIRT_ACF_SUM], (int64_t)(c & 1) * P + p, integer);
        const double e = (cen + sum / Hd) - mean;
        dev += e * e;
    }
    const double B = dev / (double)(M - 1);
    const double g0 = acf_gamma_mean(a, p, 0, integer, flips);
    const double W = g0 * Hd / (Hd - 1.0);
    const double varp = W * (Hd - 1.0) / Hd + B;
    const bool constant = !(fabs(W) <= DBL_MAX) || !(fabs(varp) <= DBL_MAX) || W == 0.0 || varp == 0.0;
    a.value[GPIRT_ACF_V_MEAN * P + p] = mean;
    a.value[GPIRT_ACF_V_SD * P + p] = sqrt(varp);
    a.flag[GPIRT_ACF_F_NONFINITE * P + p] = bad;
    a.flag[GPIRT_ACF_F_CONSTANT * P + p] = constant ? 1 : 0;
    if (constant) {
        for (int q = 0; q <= GPIRT_ACF_V_RHO1; ++q) a.value[(int64_t)q * P + p] = nan;
        a.flag[GPIRT_ACF_F_LAG_USED * P + p] = 0;
        a.flag[GPIRT_ACF_F_TRUNCATED * P + p] = 0;
        if (a.acf) for (int64_t k = 0; k <= a.L; ++k) a.acf[k * P + p] = nan;
        return;
    }
    if (a.acf) a.acf[p] = 1.0;
    double even = 1.0, prev = 0.0, psum = 0.0, rho1 = nan;
    bool open = true;                                  // Geyer's sequence still runs
    int64_t lag_used = 0;
    for (int64_t k = 1; k <= a.L; ++k) {
        const double rho = 1.0 - (W - acf_gamma_mean(a, p, k, integer, flips)) / varp;
        if (a.acf) a.acf[k * P + p] = rho;
        if (k == 1) rho1 = rho;
        if (k & 1) {
            if (open) {
                double pj = even + rho;
                if (!(pj > 0.0)) open = false;
                else {
                    if (k > 1 && prev < pj) pj = prev;
                    psum += pj;
                    prev = pj;
                    lag_used = k;
                }
            }
        } else even = rho;
    }
    const double N = (double)M * Hd;
    double tau = -1.0 + 2.0 * psum;
    const double floor_ = 1.0 / log10(N);
    if (tau < floor_) tau = floor_;
    const double ess = N / tau;
    a.value[GPIRT_ACF_V_ESS * P + p] = ess;
    a.value[GPIRT_ACF_V_TAU * P + p] = tau;
    a.value[GPIRT_ACF_V_MCSE * P + p] = sqrt(varp / ess);
    a.value[GPIRT_ACF_V_RHAT * P + p] = sqrt(varp / W);
    a.value[GPIRT_ACF_V_RHO1 * P + p] = rho1;
    a.flag[GPIRT_ACF_F_LAG_USED * P + p] = lag_used;
    a.flag[GPIRT_ACF_F_TRUNCATED * P + p] = open ? 1 : 0;
}

// work-group b: block b's values [lo, hi): min ess, max tau, max rhat over the values that are not NaN, the counts
__global__ __launch_bounds__(ACF_THREADS) void acf_block_kernel(const double* __restrict__ value, const int64_t* __restrict__ flag, int64_t P,
                                                                const int64_t* __restrict__ bounds, double* __restrict__ stat,
                                                                int64_t* __restrict__ count)
{
    __shared__ double sh[3][ACF_THREADS];
    __shared__ int64_t shc[2][ACF_THREADS];
    const int t = threadIdx.x, b = blockIdx.x;
    const int64_t lo = bounds[b], hi = bounds[b + 1];
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double mn = nan, mt = nan, mr = nan;
    int64_t ntr = 0, nn = 0;
    for (int64_t p = lo + t; p < hi; p += ACF_THREADS) {
        const double e = value[GPIRT_ACF_V_ESS * P + p], ta = value[GPIRT_ACF_V_TAU * P + p], r = value[GPIRT_ACF_V_RHAT * P + p];
        if (e == e && !(mn <= e)) mn = e;
        if (ta == ta && !(mt >= ta)) mt = ta;
        if (r == r && !(mr >= r)) mr = r;
        if (!(e == e)) ++nn;
        ntr += flag[GPIRT_ACF_F_TRUNCATED * P + p];
    }
    sh[0][t] = mn; sh[1][t] = mt; sh[2][t] = mr; shc[0][t] = ntr; shc[1][t] = nn;
    __syncthreads();
    for (int w = ACF_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
            const double e = sh[0][t + w], ta = sh[1][t + w], r = sh[2][t + w];
            if (e == e && !(sh[0][t] <= e)) sh[0][t] = e;
            if (ta == ta && !(sh[1][t] >= ta)) sh[1][t] = ta;
            if (r == r && !(sh[2][t] >= r)) sh[2][t] = r;
            shc[0][t] += shc[0][t + w];
            shc[1][t] += shc[1][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        for (int q = 0; q < 3; ++q) stat[b * GPIRT_ACF_NBSTAT + q] = sh[q][0];
        count[b * GPIRT_ACF_NBCOUNT + GPIRT_ACF_C_TRUNCATED] = shc[0][0];
        count[b * GPIRT_ACF_NBCOUNT + GPIRT_ACF_C_NAN] = shc[1][0];
    }
}

// (e, p) orders before (e', p') when e < e', or e == e' and p < p'
__device__ __forceinline__ bool acf_before(double e, int64_t p, double e2, int64_t p2)
{
    return e < e2 || (e == e2 && p < p2);
}

// one work-group: the `top` values with the smallest ess in that order (a NaN ess never enters); missing places: NaN and -1
__global__ __launch_bounds__(ACF_THREADS) void acf_top_kernel(const double* __restrict__ ess, int64_t P, int top, double* __restrict__ we,
                                                              int64_t* __restrict__ wp)
{
    __shared__ double shk[ACF_THREADS];
    __shared__ int64_t shi[ACF_THREADS];
    const int t = threadIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double pk = -__longlong_as_double(0x7ff0000000000000LL);          // -inf: everything comes after it
    int64_t pid = -1;
    for (int r = 0; r < top; ++r) {
        double bk = nan;
        int64_t bid = -1;
        if (r == 0 || pid >= 0) {
            for (int64_t e = t; e < P; e += ACF_THREADS) {
                const double v = ess[e];
                if (!(v == v)) continue;
                if (r > 0 && !acf_before(pk, pid, v, e)) continue;    // already taken
                if (bid < 0 || acf_before(v, e, bk, bid)) { bk = v; bid = e; }
            }
        }
        __syncthreads();
        shk[t] = bk; shi[t] = bid;
        __syncthreads();
        for (int w = ACF_THREADS / 2; w > 0; w >>= 1) {
            if (t < w && shi[t + w] >= 0 && (shi[t] < 0 || acf_before(shk[t + w], shi[t + w], shk[t], shi[t]))) {
                shk[t] = shk[t + w]; shi[t] = shi[t + w];
            }
            __syncthreads();
        }
        pk = shk[0]; pid = shi[0];
        if (t == 0) { we[r] = pid >= 0 ? pk : nan; wp[r] = pid; }
    }
}

struct DevBuf {
    std::vector<void*> p;
    ~DevBuf() { for (void* q : p) hipFree(q); }
    int get(void** q, size_t bytes)
    {
        GP_HIP(hipMalloc(q, bytes ? bytes : 16));
        p.push_back(*q);
        return 0;
    }
};

inline unsigned acf_grid(int64_t work) { return (unsigned)std::max<int64_t>((work + ACF_THREADS - 1) / ACF_THREADS, 1); }

}  // namespace

AcfLayout acf_layout(int64_t P, int64_t L)
{
    AcfLayout A{};
    int64_t at = ACF_HEADER_WORDS;
    for (int k = 0; k < GPIRT_ACF_NARRAYS; ++k) {
        A.off[k] = at;
        at += (acf_raw_words(k, P, L) + 1) / 2 * 2;                   // whole 16-byte pieces
    }
    A.words = at;
    return A;
}

int acf_check(int64_t n, int64_t m, int parts, int64_t planned, int64_t max_lag, int64_t* L_out, int64_t* P_out)
{
    if (n < 1 || m < 1) {
        set_error("ACF: n = %lld and m = %lld must be at least 1", (long long)n, (long long)m);
        return GPIRT_E_ARG;
    }
    if (parts <= 0 || (parts & ~(GPIRT_ACF_THETA | GPIRT_ACF_BETA | GPIRT_ACF_LL))) {
        set_error("ACF: parts = %d, it must be a non-empty mask of GPIRT_ACF_THETA | GPIRT_ACF_BETA | GPIRT_ACF_LL", parts);
        return GPIRT_E_ARG;
    }
    const int64_t H = planned / 2;
    if (planned < 1 || H < 4) {
        set_error("ACF: %lld planned draws give halves of %lld draws, fewer than 4 (no planned draws?)", (long long)planned,
                  (long long)(planned < 0 ? 0 : H));
        return GPIRT_E_ARG;
    }
    const int64_t cap = std::min<int64_t>(H - 1, GPIRT_ACF_MAX_LAG);
    if (max_lag < 0 || max_lag > cap) {
        set_error("ACF: max_lag = %lld, it must lie in 1 .. min(H - 1, %d) = %lld for halves of H = %lld draws (or be 0 for the default)",
                  (long long)max_lag, GPIRT_ACF_MAX_LAG, (long long)cap, (long long)H);
        return GPIRT_E_ARG;
    }
    if (L_out) *L_out = max_lag ? max_lag : std::min<int64_t>(H - 1, GPIRT_ACF_DEFAULT_LAG);
    if (P_out) *P_out = acf_dims(n, m, parts).P;
    return 0;
}

void acf_free(AcfState* s)
{
    if (s->block) hipFree(s->block);
    if (s->last) hipFree(s->last);
    if (s->cpart) hipFree(s->cpart);
    if (s->rpart) hipFree(s->rpart);
    *s = AcfState{};
}

int acf_alloc(hipStream_t st, AcfState* s, int64_t n, int64_t m, int parts, int64_t planned, int64_t L)
{
    const AcfDims d = acf_dims(n, m, parts);
    const AcfLayout A = acf_layout(d.P, L);
    s->n = n; s->m = m; s->parts = parts; s->S = planned; s->H = planned / 2; s->L = L; s->P = d.P; s->draws = 0;
    GP_HIP(hipMalloc((void**)&s->block, sizeof(uint64_t) * (size_t)A.words));
    GP_HIP(hipMalloc((void**)&s->last, sizeof(double) * (size_t)d.P));
    GP_HIP(hipMemsetAsync(s->block, 0, sizeof(uint64_t) * (size_t)A.words, st));
    GP_HIP(hipMemsetAsync(s->last, 0, sizeof(double) * (size_t)d.P, st));
    if (parts & GPIRT_ACF_LL) {
        const int64_t nb = (n + ACF_THREADS - 1) / ACF_THREADS, nq = (m + ACF_LL_COLS - 1) / ACF_LL_COLS;
        GP_HIP(hipMalloc((void**)&s->cpart, sizeof(double) * (size_t)(nb * m)));
        GP_HIP(hipMalloc((void**)&s->rpart, sizeof(double) * (size_t)(nq * n)));
    }
    const int64_t hdr[ACF_HEADER_WORDS] = { ACF_TAG, ACF_LAYOUT_VERSION, n, m, parts, planned, planned / 2, L, d.P, 0 };
    GP_HIP(hipMemcpyAsync(s->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));            // hdr is this call's
    s->on = true;
    return 0;
}

int launch_acf_accumulate(hipStream_t st, AcfState* s, const double* theta, const double* beta, const double* f, const double* mu,
                          const double* y)
{
    if (s->draws >= s->S) {
        set_error("ACF: all %lld planned draws are in (gpirt_sampler_acf_enable)", (long long)s->S);
        return GPIRT_E_ARG;
    }
    const AcfDims d = acf_dims(s->n, s->m, s->parts);
    const AcfLayout A = acf_layout(d.P, s->L);
    const AcfBlock b = acf_block(s->block, A);
    const int64_t draw = s->draws + 1, H = s->H, L = s->L, R = L + 1, P = d.P;
    int half = 0;
    int64_t t = 0;
    if (draw <= H) { half = 1; t = draw; }
    else if (draw > s->S - H) { half = 2; t = draw - (s->S - H); }
    if (s->parts & GPIRT_ACF_LL) {
        const int nb = (int)((s->n + ACF_THREADS - 1) / ACF_THREADS), nq = (int)((s->m + ACF_LL_COLS - 1) / ACF_LL_COLS);
        hipLaunchKernelGGL(acf_ll_kernel, dim3(nb, nq), dim3(ACF_THREADS), 0, st, f, mu, y, s->n, s->m, s->cpart, s->rpart);
        hipLaunchKernelGGL(acf_fold_kernel, dim3(acf_grid(s->n + s->m)), dim3(ACF_THREADS), 0, st, s->cpart, s->rpart, s->n, s->m, nb, nq,
                           s->last + d.o_item, s->last + d.o_resp);
        hipLaunchKernelGGL(acf_total_kernel, dim3(1), dim3(ACF_THREADS), 0, st, s->last + d.o_item, s->m, s->last + d.o_total);
    }
    hipLaunchKernelGGL(acf_gather_kernel, dim3(acf_grid(P)), dim3(ACF_THREADS), 0, st, b, d, theta, beta, s->last, half, t, L,
                       draw == 1 ? 1 : 0);
    if (half) {
        const int64_t hp = half - 1, kmax = std::min<int64_t>(L, t - 1);
        const unsigned chunks = (unsigned)(kmax / ACF_KCHUNK + 1);
        if (d.Pi > 0)
            hipLaunchKernelGGL(acf_lag_kernel<int64_t>, dim3(acf_grid(d.Pi), chunks), dim3(ACF_THREADS), 0, st,
                               reinterpret_cast<const int64_t*>(b.ring), reinterpret_cast<int64_t*>(b.s) + hp * R * P, P, (int64_t)0, d.Pi, t, R,
                               kmax);
        if (P > d.Pi)
            hipLaunchKernelGGL(acf_lag_kernel<double>, dim3(acf_grid(P - d.Pi), chunks), dim3(ACF_THREADS), 0, st,
                               reinterpret_cast<const double*>(b.ring), reinterpret_cast<double*>(b.s) + hp * R * P, P, d.Pi, P, t, R, kmax);
        if (t == H) {
            if (d.Pi > 0)
                hipLaunchKernelGGL(acf_tail_kernel<int64_t>, dim3(acf_grid(d.Pi)), dim3(ACF_THREADS), 0, st,
                                   reinterpret_cast<const int64_t*>(b.ring), reinterpret_cast<int64_t*>(b.tail) + hp * R * P, P, (int64_t)0, d.Pi,
                                   H, R, L);
            if (P > d.Pi)
                hipLaunchKernelGGL(acf_tail_kernel<double>, dim3(acf_grid(P - d.Pi)), dim3(ACF_THREADS), 0, st,
                                   reinterpret_cast<const double*>(b.ring), reinterpret_cast<double*>(b.tail) + hp * R * P, P, d.Pi, P, H, R, L);
        }
    }
    GP_HIP(hipGetLastError());
    s->draws = draw;
    return 0;
}

int acf_get(hipStream_t st, AcfState* s, const char* name, void* h_out, int64_t bytes)
{
    const AcfLayout A = acf_layout(s->P, s->L);
    auto copy = [&](const void* src) -> int {
        GP_HIP(hipMemcpyAsync(h_out, src, (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 64); return copy(s->block + 2); }
    if (strcmp(name, "last") == 0) { GP_ARG(bytes == 8 * s->P); return copy(s->last); }
    for (int k = 0; k < GPIRT_ACF_NARRAYS; ++k)
        if (strcmp(kAcfRaw[k], name) == 0) {
            GP_ARG(bytes == 8 * acf_raw_words(k, s->P, s->L));
            return copy(s->block + A.off[k]);
        }
    set_error("unknown acf field '%s'", name);
    return GPIRT_E_ARG;
}

int acf_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_acf* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_ACF_MAX_TOP) {
        set_error("ACF: top = %lld, it must lie in 1 .. %d", (long long)out->top, GPIRT_ACF_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) {
        GP_ARG(d_states[c]);
        if (signs && signs[c] != 1 && signs[c] != -1) {
            set_error("ACF: sign %d is %d, not +1 or -1", c, signs[c]);
            return GPIRT_E_ARG;
        }
    }
    hipStream_t st = h->stream;
    int64_t h0[ACF_HEADER_WORDS] = {}, hc[ACF_HEADER_WORDS];
    for (int c = 0; c < chains; ++c) {
        GP_HIP(hipMemcpyAsync(hc, d_states[c], sizeof(hc), hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        if (hc[0] != ACF_TAG || hc[1] != ACF_LAYOUT_VERSION || acf_check(hc[2], hc[3], (int)hc[4], hc[5], hc[7], nullptr, nullptr) != 0 ||
            hc[7] < 1 || hc[6] != hc[5] / 2 || hc[8] != acf_dims(hc[2], hc[3], (int)hc[4]).P) {
            set_error("gpirt_acf_combine: state %d is not an ACF state block of layout %d", c, ACF_LAYOUT_VERSION);
            return GPIRT_E_ARG;
        }
        if (c == 0) memcpy(h0, hc, sizeof(h0));
        else if (memcmp(h0 + 2, hc + 2, sizeof(int64_t) * 7) != 0) {
            set_error("gpirt_acf_combine: state %d has another n, m, parts, S or L than state 0", c);
            return GPIRT_E_ARG;
        }
        if (hc[9] != hc[5]) {
            set_error("gpirt_acf_combine: state %d holds %lld of its %lld planned draws", c, (long long)hc[9], (long long)hc[5]);
            return GPIRT_E_ARG;
        }
    }
    const int64_t n = h0[2], m = h0[3], S = h0[5], H = h0[6], L = h0[7], P = h0[8];
    const int parts = (int)h0[4], top = (int)out->top;
    const AcfLayout A = acf_layout(P, L);
    DevBuf buf;
    const uint64_t** d_ptrs = nullptr;
    int* d_signs = nullptr;
    double *d_value = nullptr, *d_acf = nullptr, *d_stat = nullptr, *d_we = nullptr;
    int64_t *d_flag = nullptr, *d_count = nullptr, *d_bounds = nullptr, *d_wp = nullptr;
    GP_TRY(buf.get((void**)&d_ptrs, sizeof(void*) * (size_t)chains));
    GP_TRY(buf.get((void**)&d_signs, sizeof(int) * (size_t)chains));
    GP_TRY(buf.get((void**)&d_value, sizeof(double) * (size_t)(GPIRT_ACF_NVALUE * P)));
    GP_TRY(buf.get((void**)&d_flag, sizeof(int64_t) * (size_t)(GPIRT_ACF_NFLAG * P)));
    if (out->acf) GP_TRY(buf.get((void**)&d_acf, sizeof(double) * (size_t)((L + 1) * P)));
    GP_TRY(buf.get((void**)&d_stat, sizeof(double) * GPIRT_ACF_NBLOCK * GPIRT_ACF_NBSTAT));
    GP_TRY(buf.get((void**)&d_count, sizeof(int64_t) * GPIRT_ACF_NBLOCK * GPIRT_ACF_NBCOUNT));
    GP_TRY(buf.get((void**)&d_bounds, sizeof(int64_t) * (GPIRT_ACF_NBLOCK + 1)));
    GP_TRY(buf.get((void**)&d_we, sizeof(double) * (size_t)top));
    GP_TRY(buf.get((void**)&d_wp, sizeof(int64_t) * (size_t)top));
    std::vector<int> sg((size_t)chains, 1);
    if (signs) for (int c = 0; c < chains; ++c) sg[(size_t)c] = signs[c];
    const AcfDims d = acf_dims(n, m, parts);
    const bool ll = parts & GPIRT_ACF_LL;
    const int64_t bounds[GPIRT_ACF_NBLOCK + 1] = { 0, d.Pi, d.o_item, ll ? d.o_resp : d.o_item, ll ? d.o_total : d.o_item, P };
    GP_HIP(hipMemcpyAsync(d_ptrs, d_states, sizeof(void*) * (size_t)chains, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(d_signs, sg.data(), sizeof(int) * (size_t)chains, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(d_bounds, bounds, sizeof(bounds), hipMemcpyHostToDevice, st));
    AcfFinish a{};
    a.blocks = d_ptrs; a.signs = d_signs; a.d = d; a.H = H; a.L = L; a.C = chains;
    for (int k = 0; k < GPIRT_ACF_NARRAYS; ++k) a.off[k] = A.off[k];
    a.value = d_value; a.flag = d_flag; a.acf = d_acf;
    hipLaunchKernelGGL(acf_finish_kernel, dim3(acf_grid(P)), dim3(ACF_THREADS), 0, st, a);
    hipLaunchKernelGGL(acf_block_kernel, dim3(GPIRT_ACF_NBLOCK), dim3(ACF_THREADS), 0, st, d_value, d_flag, P, d_bounds, d_stat, d_count);
    hipLaunchKernelGGL(acf_top_kernel, dim3(1), dim3(ACF_THREADS), 0, st, d_value + (int64_t)GPIRT_ACF_V_ESS * P, P, top, d_we, d_wp);
    GP_HIP(hipGetLastError());
    auto back = [&](void* dst, const void* src, size_t bytes) -> int {
        if (dst) GP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        return 0;
    };
    for (int q = 0; q < GPIRT_ACF_NVALUE; ++q) GP_TRY(back(out->value[q], d_value + (int64_t)q * P, sizeof(double) * (size_t)P));
    for (int q = 0; q < GPIRT_ACF_NFLAG; ++q) GP_TRY(back(out->flag[q], d_flag + (int64_t)q * P, sizeof(int64_t) * (size_t)P));
    GP_TRY(back(out->acf, d_acf, sizeof(double) * (size_t)((L + 1) * P)));
    GP_TRY(back(out->block_stat, d_stat, sizeof(out->block_stat)));
    GP_TRY(back(out->block_count, d_count, sizeof(out->block_count)));
    std::vector<int64_t> wp((size_t)top);
    GP_TRY(back(wp.data(), d_wp, sizeof(int64_t) * (size_t)top));
    GP_TRY(back(out->worst_ess, d_we, sizeof(double) * (size_t)top));
    GP_HIP(hipStreamSynchronize(st));
    for (int r = 0; r < top; ++r) {
        int blk = -1;
        int64_t idx = -1;
        if (wp[(size_t)r] >= 0) {
            for (blk = GPIRT_ACF_NBLOCK - 1; blk > 0 && wp[(size_t)r] < bounds[blk]; --blk) {}
            idx = wp[(size_t)r] - bounds[blk];
        }
        if (out->worst_block) out->worst_block[r] = blk;
        if (out->worst_index) out->worst_index[r] = idx;
    }
    out->n = n; out->m = m; out->parts = parts; out->S = S; out->H = H; out->L = L; out->P = P; out->chains = chains;
    return 0;
}

}  // namespace gpirt
