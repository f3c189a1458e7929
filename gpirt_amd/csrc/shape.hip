// shape.hip -- shape posteriors of the item response curves (include/gpirt_hip.h, "IRF shape posteriors"):
// per draw and item, from the draw's smooth curve g = k*^T S^-1 f + mu* (the sampler's "gbar", stored by draw_fstar's epilogue),
// where the curve peaks, whether it is monotone within a tolerance, where it crosses P = 1/2, how steep it is and how much
// Fisher information it carries -- accumulated one draw at a time without stored draws.
//
// shape_item_kernel: one work-group of 256 lanes per item column.  The column (1001 doubles, contiguous) is read once, lanes
// along k, into LDS; lane t then owns k = 4t .. 4t + 3.  The prefix max / min that the largest fall and rise need are a wave
// scan of the lanes' aggregates plus an LDS combine of the four waves; every other quantity is a max, a min, an integer sum or
// an argmax with the lowest-k tie rule, reduced by wave shuffles and the same LDS combine -- order-independent, so exact.
// Lane 0 classifies the draw and bumps the item's cells; the information I[k, j] goes out lanes along k.
// shape_ti_kernel: TI[k] = sum_j I[k, j] in ascending j, one lane per k (coalesced across k), and the reliability's terms.
// shape_rel_kernel: one work-group adds the terms in a fixed order and keeps the draw counters.
// Every accumulator cell is owned by one lane: no atomics, bit-identical from run to run.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <climits>

namespace gpirt {

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_N = GPIRT_NGRID;                 // 1001 grid points
constexpr int SH_PAD = 1024;                      // ... padded to four per lane
constexpr int TI_THREADS = 64;                    // shape_ti_kernel: one wave per work-group, so that 16 CUs share the reads
constexpr int SH_CENTRE = (GPIRT_NGRID - 1) / 2;  // the grid index of theta = 0
static_assert(SH_N <= SH_PAD && SH_PAD == 4 * SH_THREADS, "lane t owns k = 4t .. 4t + 3");

const char* const kShapeRaw[GPIRT_SHAPE_NARRAYS] = { "cls", "peak_hist", "valley_hist", "cross_first_hist", "cross_last_hist",
                                                     "cross_count", "draws", "nonfinite", "slope", "info_sum", "ti_sum",
                                                     "ti_sumsq", "rel" };

// bytes per element and elements of raw array k
inline int shape_raw_width(int k) { return k <= GPIRT_SHAPE_NONFINITE ? 4 : 8; }
inline int64_t shape_raw_count(int k, int64_t m)
{
    switch (k) {
        case GPIRT_SHAPE_CLS: return (int64_t)GPIRT_SHAPE_MAX_TOLS * 4 * m;
        case GPIRT_SHAPE_PEAK_HIST: case GPIRT_SHAPE_VALLEY_HIST: case GPIRT_SHAPE_CROSS_FIRST_HIST:
        case GPIRT_SHAPE_CROSS_LAST_HIST: case GPIRT_SHAPE_INFO_SUM: return (int64_t)SH_N * m;
        case GPIRT_SHAPE_CROSS_COUNT: case GPIRT_SHAPE_SLOPE: return 4 * m;
        case GPIRT_SHAPE_DRAWS: case GPIRT_SHAPE_NONFINITE: return m;
        case GPIRT_SHAPE_TI_SUM: case GPIRT_SHAPE_TI_SUMSQ: return SH_N;
        default: return 2;                        // GPIRT_SHAPE_REL
    }
}

struct ShapeArgs {
    const double* g;                              // N x m, ld N
    int64_t m;
    int klo, khi, n_tols;
    double tols[GPIRT_SHAPE_MAX_TOLS];
    uint32_t *cls, *peak, *valley, *cfirst, *clast, *ccount, *draws, *nonfinite;
    double *slope, *info_sum, *info;
    unsigned char* bad;
};

__global__ __launch_bounds__(SH_THREADS) void shape_item_kernel(ShapeArgs a)
{
    __shared__ double g[SH_PAD];
    __shared__ double w_max[4], w_min[4];                         // the waves' aggregates for the scan
    __shared__ double r_dd[4], r_du[4], r_bv[4], r_cv[4], r_smax[4], r_smin[4];
    __shared__ int r_bk[4], r_ck[4], r_cnt[4], r_first[4], r_last[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int64_t j = blockIdx.x;
    const double* col = a.g + j * SH_N;
    int nf = 0;
    for (int k = t; k < SH_N; k += SH_THREADS) {
        const double v = col[k];
        g[k] = v;
        nf |= isfinite(v) ? 0 : 1;
    }
    if (__syncthreads_or(nf)) {                                   // (the barrier also publishes g)
        if (t == 0) { a.nonfinite[j] += 1u; a.bad[j] = 1; }
        return;
    }
    const double inf = (double)INFINITY;
    const int k0 = 4 * t;
    const int lo = k0 > a.klo ? k0 : a.klo, hi = k0 + 3 < a.khi ? k0 + 3 : a.khi;     // this lane's part of W (empty: lo > hi)
    // the lane's aggregate, then the exclusive prefix over the lanes before it
    double tmax = -inf, tmin = inf;
    for (int k = lo; k <= hi; ++k) { tmax = fmax(tmax, g[k]); tmin = fmin(tmin, g[k]); }
    double imax = tmax, imin = tmin;
    for (int off = 1; off < 64; off <<= 1) {
        const double u = __shfl_up(imax, off, 64), v = __shfl_up(imin, off, 64);
        if (lane >= off) { imax = fmax(imax, u); imin = fmin(imin, v); }
    }
    if (lane == 63) { w_max[wv] = imax; w_min[wv] = imin; }
    double emax = __shfl_up(imax, 1, 64), emin = __shfl_up(imin, 1, 64);
    if (lane == 0) { emax = -inf; emin = inf; }
    __syncthreads();
    for (int q = 0; q < wv; ++q) { emax = fmax(emax, w_max[q]); emin = fmin(emin, w_min[q]); }
    // the lane's own k in order: the largest fall and rise, the extremes (first occurrence), the crossings, the slopes
    double dd = 0.0, du = 0.0, bv = -inf, cv = inf, smax = -inf, smin = inf;
    int bk = INT_MAX, ck = INT_MAX, cnt = 0, first = INT_MAX, last = -1;
    for (int k = lo; k <= hi; ++k) {
        const double v = g[k];
        emax = fmax(emax, v); emin = fmin(emin, v);
        dd = fmax(dd, emax - v); du = fmax(du, v - emin);
        if (v > bv) { bv = v; bk = k; }
        if (v < cv) { cv = v; ck = k; }
        if (k < a.khi) {
            const double nx = g[k + 1];
            if ((v >= 0.0) != (nx >= 0.0)) { ++cnt; first = first < k ? first : k; last = k; }
            const double d = nx - v;
            smax = fmax(smax, d); smin = fmin(smin, d);
        }
    }
    for (int off = 32; off; off >>= 1) {
        dd = fmax(dd, __shfl_xor(dd, off, 64)); du = fmax(du, __shfl_xor(du, off, 64));
        smax = fmax(smax, __shfl_xor(smax, off, 64)); smin = fmin(smin, __shfl_xor(smin, off, 64));
        const double ob = __shfl_xor(bv, off, 64), oc = __shfl_xor(cv, off, 64);
        const int obk = __shfl_xor(bk, off, 64), ock = __shfl_xor(ck, off, 64);
        if (ob > bv || (ob == bv && obk < bk)) { bv = ob; bk = obk; }
        if (oc < cv || (oc == cv && ock < ck)) { cv = oc; ck = ock; }
        cnt += __shfl_xor(cnt, off, 64);
        const int of = __shfl_xor(first, off, 64), ol = __shfl_xor(last, off, 64);
        first = first < of ? first : of; last = last > ol ? last : ol;
    }
    if (lane == 0) {
        r_dd[wv] = dd; r_du[wv] = du; r_bv[wv] = bv; r_cv[wv] = cv; r_smax[wv] = smax; r_smin[wv] = smin;
        r_bk[wv] = bk; r_ck[wv] = ck; r_cnt[wv] = cnt; r_first[wv] = first; r_last[wv] = last;
    }
    __syncthreads();
    if (t == 0) {
        for (int q = 1; q < 4; ++q) {
            dd = fmax(dd, r_dd[q]); du = fmax(du, r_du[q]); smax = fmax(smax, r_smax[q]); smin = fmin(smin, r_smin[q]);
            if (r_bv[q] > bv || (r_bv[q] == bv && r_bk[q] < bk)) { bv = r_bv[q]; bk = r_bk[q]; }
            if (r_cv[q] < cv || (r_cv[q] == cv && r_ck[q] < ck)) { cv = r_cv[q]; ck = r_ck[q]; }
            cnt += r_cnt[q];
            first = first < r_first[q] ? first : r_first[q]; last = last > r_last[q] ? last : r_last[q];
        }
        const int64_t m = a.m;
        a.draws[j] += 1u;
        a.bad[j] = 0;
        a.peak[j * SH_N + bk] += 1u;                              // bk, ck in [klo, khi]: W is never empty
        a.valley[j * SH_N + ck] += 1u;
        for (int q = 0; q < a.n_tols; ++q) {
            const double tol = a.tols[q];
            const int c = dd <= tol ? (du <= tol ? GPIRT_SHAPE_CLS_FLAT : GPIRT_SHAPE_CLS_INCREASING)
                                    : (du <= tol ? GPIRT_SHAPE_CLS_DECREASING : GPIRT_SHAPE_CLS_NONMONOTONE);
            a.cls[((int64_t)q * 4 + c) * m + j] += 1u;
        }
        a.ccount[(int64_t)(cnt < 3 ? cnt : 3) * m + j] += 1u;
        if (cnt >= 1) { a.cfirst[j * SH_N + first] += 1u; a.clast[j * SH_N + last] += 1u; }     // pair indices in [klo, khi - 1]
        const double vmax = smax / 0.01, vmin = smin / 0.01;
        a.slope[j] += vmax; a.slope[m + j] += vmax * vmax;
        a.slope[2 * m + j] += vmin; a.slope[3 * m + j] += vmin * vmin;
    }
    for (int k = t; k < SH_N; k += SH_THREADS) {
        const double gp = k == 0 ? (g[1] - g[0]) / 0.01 : k == SH_N - 1 ? (g[SH_N - 1] - g[SH_N - 2]) / 0.01 : (g[k + 1] - g[k - 1]) / 0.02;
        const double e = exp(-fabs(g[k])), ope = 1.0 + e;
        const double I = (e / (ope * ope)) * (gp * gp);
        a.info[j * SH_N + k] = I;
        a.info_sum[j * SH_N + k] += I;
    }
}

// grid: SH_PAD / TI_THREADS work-groups, one lane per k
__global__ __launch_bounds__(TI_THREADS) void shape_ti_kernel(const double* __restrict__ info, const unsigned char* __restrict__ bad,
                                                              int64_t m, const double* __restrict__ w, double* __restrict__ ti,
                                                              double* __restrict__ term, double* __restrict__ ti_sum,
                                                              double* __restrict__ ti_sumsq, int* __restrict__ ctl)
{
    const int t = threadIdx.x;
    int b = 0;
    for (int64_t j = t; j < m; j += TI_THREADS) b |= bad[j];
    const int skip = __syncthreads_or(b);                         // the same in every work-group
    if (blockIdx.x == 0 && t == 0) ctl[0] = skip;
    if (skip) return;
    const int k = blockIdx.x * TI_THREADS + t;
    if (k >= SH_N) { term[k] = 0.0; return; }                     // k < SH_PAD: term holds SH_PAD doubles
    double s = 0.0;
    int64_t j = 0;
    for (; j + 8 <= m; j += 8) {                                  // eight loads in flight, added in ascending j
        double v[8];
        for (int q = 0; q < 8; ++q) v[q] = info[(j + q) * SH_N + k];
        for (int q = 0; q < 8; ++q) s += v[q];
    }
    for (; j < m; ++j) s += info[j * SH_N + k];
    ti[k] = s;
    ti_sum[k] += s;
    ti_sumsq[k] += s * s;
    term[k] = w[k] * (s / (s + 1.0));
}

__global__ __launch_bounds__(SH_THREADS) void shape_rel_kernel(const double* __restrict__ term, const int* __restrict__ ctl,
                                                               double* __restrict__ rel, int64_t* __restrict__ hdr)
{
    __shared__ double part[SH_THREADS];
    const int t = threadIdx.x;
    if (ctl[0]) {
        if (t == 0) hdr[11] += 1;                                 // info_skipped
        return;
    }
    part[t] = ((term[4 * t] + term[4 * t + 1]) + term[4 * t + 2]) + term[4 * t + 3];
    __syncthreads();
    if (t == 0) {
        double rho = 0.0;
        for (int q = 0; q < SH_THREADS; ++q) rho += part[q];
        rel[0] += rho;
        rel[1] += rho * rho;
        hdr[10] += 1;                                             // info_draws
    }
}

// a state block on the host
struct HostShape {
    std::vector<uint64_t> w;
    int64_t n = 0, m = 0;
    ShapeLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    template <class T> T* arr(int k) { return reinterpret_cast<T*>(w.data() + L.off[k]); }
};

int shape_read(hipStream_t st, const void* d_state, HostShape& r, const char* who, int c)
{
    int64_t hdr[SHAPE_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] != SHAPE_TAG || hdr[1] != SHAPE_LAYOUT_VERSION || hdr[2] <= 0 || hdr[3] <= 0 || hdr[4] < 1 || hdr[4] > SH_CENTRE ||
        hdr[5] < 1 || hdr[5] > GPIRT_SHAPE_MAX_TOLS || hdr[10] < 0 || hdr[11] < 0) {
        set_error("%s: state %d is not a shape state block of layout %d", who, c, SHAPE_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[2]; r.m = hdr[3];
    r.L = shape_layout(r.m);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

// theta -> -theta on the accumulators (include/gpirt_hip.h): exact, W being symmetric
void shape_reflect(HostShape& r)
{
    const int64_t m = r.m;
    uint32_t *peak = r.arr<uint32_t>(GPIRT_SHAPE_PEAK_HIST), *valley = r.arr<uint32_t>(GPIRT_SHAPE_VALLEY_HIST);
    uint32_t *cf = r.arr<uint32_t>(GPIRT_SHAPE_CROSS_FIRST_HIST), *cl = r.arr<uint32_t>(GPIRT_SHAPE_CROSS_LAST_HIST);
    double* info = r.arr<double>(GPIRT_SHAPE_INFO_SUM);
    for (int64_t j = 0; j < m; ++j) {
        std::reverse(peak + j * SH_N, peak + (j + 1) * SH_N);
        std::reverse(valley + j * SH_N, valley + (j + 1) * SH_N);
        std::reverse(info + j * SH_N, info + (j + 1) * SH_N);
        // pair indices k -> 999 - k (cell 1000 is never a pair's), and the first crossing becomes the last
        std::reverse(cf + j * SH_N, cf + j * SH_N + (SH_N - 1));
        std::reverse(cl + j * SH_N, cl + j * SH_N + (SH_N - 1));
        std::swap_ranges(cf + j * SH_N, cf + (j + 1) * SH_N, cl + j * SH_N);
    }
    std::reverse(r.arr<double>(GPIRT_SHAPE_TI_SUM), r.arr<double>(GPIRT_SHAPE_TI_SUM) + SH_N);
    std::reverse(r.arr<double>(GPIRT_SHAPE_TI_SUMSQ), r.arr<double>(GPIRT_SHAPE_TI_SUMSQ) + SH_N);
    uint32_t* cls = r.arr<uint32_t>(GPIRT_SHAPE_CLS);
    for (int q = 0; q < GPIRT_SHAPE_MAX_TOLS; ++q)
        std::swap_ranges(cls + ((int64_t)q * 4 + GPIRT_SHAPE_CLS_INCREASING) * m, cls + ((int64_t)q * 4 + GPIRT_SHAPE_CLS_INCREASING + 1) * m,
                         cls + ((int64_t)q * 4 + GPIRT_SHAPE_CLS_DECREASING) * m);
    double* sl = r.arr<double>(GPIRT_SHAPE_SLOPE);
    for (int64_t j = 0; j < m; ++j) {
        const double mx = sl[j], mn = sl[2 * m + j];
        sl[j] = -mn; sl[2 * m + j] = -mx;
        std::swap(sl[m + j], sl[3 * m + j]);
    }
}

void shape_fill(HostShape& r, gpirt_shape* out)
{
    const int64_t* h = r.hdr();
    out->k_half = (int)h[4]; out->n_tols = (int)h[5];
    for (int q = 0; q < GPIRT_SHAPE_MAX_TOLS; ++q) memcpy(&out->tols[q], &h[6 + q], sizeof(double));
    out->n = r.n; out->m = r.m; out->info_draws = h[10]; out->info_skipped = h[11];
    for (int k = 0; k < GPIRT_SHAPE_NARRAYS; ++k)
        if (out->raw[k]) memcpy(out->raw[k], r.w.data() + r.L.off[k], (size_t)(shape_raw_count(k, r.m) * shape_raw_width(k)));
}

}  // namespace

ShapeLayout shape_layout(int64_t m)
{
    ShapeLayout L{};
    int64_t at = SHAPE_HEADER_WORDS;
    for (int k = 0; k < GPIRT_SHAPE_NARRAYS; ++k) {
        L.off[k] = at;
        const int64_t bytes = shape_raw_count(k, m) * shape_raw_width(k);
        at += (bytes + 15) / 16 * 2;                                  // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int shape_check(int k_half, const double* tols, int n_tols)
{
    if (k_half < 1 || k_half > SH_CENTRE) {
        set_error("shape posteriors: the window's half width is %d grid steps, 1..%d are taken (window in [0.01, 5.0])", k_half, SH_CENTRE);
        return GPIRT_E_ARG;
    }
    if (n_tols < 1 || n_tols > GPIRT_SHAPE_MAX_TOLS || !tols) {
        set_error("shape posteriors: %d tolerances given, 1..%d are taken", n_tols, GPIRT_SHAPE_MAX_TOLS);
        return GPIRT_E_ARG;
    }
    for (int q = 0; q < n_tols; ++q)
        if (!(tols[q] >= 0.0) || !std::isfinite(tols[q])) {
            set_error("shape posteriors: a tolerance must be finite and >= 0 (logits)");
            return GPIRT_E_ARG;
        }
    return 0;
}

void shape_free(ShapeState* p)
{
    order_free(&p->order);
    for (void* q : p->allocs) hipFree(q);
    *p = ShapeState{};
}

int shape_alloc(hipStream_t st, ShapeState* p, int64_t n, int64_t m, int k_half, const double* tols, int n_tols)
{
    GP_TRY(shape_check(k_half, tols, n_tols));
    const ShapeLayout L = shape_layout(m);
    p->n = n; p->m = m; p->k_half = k_half; p->n_tols = n_tols;
    for (int q = 0; q < n_tols; ++q) p->tols[q] = tols[q];
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    const size_t cells = (size_t)SH_N * (size_t)m;
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->gbar, sizeof(double) * (cells + 1)));
    GP_TRY(get((void**)&p->info, sizeof(double) * cells));
    GP_TRY(get((void**)&p->ti, sizeof(double) * SH_PAD));
    GP_TRY(get((void**)&p->term, sizeof(double) * SH_PAD));
    GP_TRY(get((void**)&p->w, sizeof(double) * SH_PAD + 16));         // the weights, then ctl (one int) behind them
    GP_TRY(get((void**)&p->bad, (size_t)m));
    // the N(0, 1) density on the grid, normalised: theta_k the double -5 + 0.01 k, the sum in ascending k
    std::vector<double> w(SH_PAD, 0.0);
    double sum = 0.0;
    for (int k = 0; k < SH_N; ++k) {
        const double th = -5.0 + (double)k * 0.01;
        w[(size_t)k] = exp(-(th * th) / 2.0);
        sum += w[(size_t)k];
    }
    for (int k = 0; k < SH_N; ++k) w[(size_t)k] /= sum;
    int64_t hdr[SHAPE_HEADER_WORDS] = { SHAPE_TAG, SHAPE_LAYOUT_VERSION, n, m, k_half, n_tols };
    for (int q = 0; q < GPIRT_SHAPE_MAX_TOLS; ++q) memcpy(&hdr[6 + q], &p->tols[q], sizeof(double));
    GP_HIP(hipMemcpyAsync(p->w, w.data(), sizeof(double) * SH_PAD, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // w and hdr are this call's: nothing below may leave with the copies pending
    p->on = true;
    return 0;
}

int launch_shape_accumulate(hipStream_t st, ShapeState* p, const double* gbar)
{
    const ShapeLayout L = shape_layout(p->m);
    ShapeArgs a{};
    a.g = gbar; a.m = p->m; a.klo = SH_CENTRE - p->k_half; a.khi = SH_CENTRE + p->k_half; a.n_tols = p->n_tols;
    for (int q = 0; q < GPIRT_SHAPE_MAX_TOLS; ++q) a.tols[q] = p->tols[q];
    auto u32 = [&](int k) { return reinterpret_cast<uint32_t*>(p->block + L.off[k]); };
    auto f64 = [&](int k) { return reinterpret_cast<double*>(p->block + L.off[k]); };
    a.cls = u32(GPIRT_SHAPE_CLS); a.peak = u32(GPIRT_SHAPE_PEAK_HIST); a.valley = u32(GPIRT_SHAPE_VALLEY_HIST);
    a.cfirst = u32(GPIRT_SHAPE_CROSS_FIRST_HIST); a.clast = u32(GPIRT_SHAPE_CROSS_LAST_HIST);
    a.ccount = u32(GPIRT_SHAPE_CROSS_COUNT); a.draws = u32(GPIRT_SHAPE_DRAWS); a.nonfinite = u32(GPIRT_SHAPE_NONFINITE);
    a.slope = f64(GPIRT_SHAPE_SLOPE); a.info_sum = f64(GPIRT_SHAPE_INFO_SUM); a.info = p->info; a.bad = p->bad;
    int* ctl = reinterpret_cast<int*>(p->w + SH_PAD);
    hipLaunchKernelGGL(shape_item_kernel, dim3((unsigned)p->m), dim3(SH_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(shape_ti_kernel, dim3(SH_PAD / TI_THREADS), dim3(TI_THREADS), 0, st, p->info, p->bad, p->m, p->w, p->ti,
                       p->term, f64(GPIRT_SHAPE_TI_SUM), f64(GPIRT_SHAPE_TI_SUMSQ), ctl);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(shape_rel_kernel, dim3(1), dim3(SH_THREADS), 0, st, p->term, ctl, f64(GPIRT_SHAPE_REL),
                       reinterpret_cast<int64_t*>(p->block));
    GP_HIP(hipGetLastError());
    if (p->order.on) GP_TRY(launch_order_accumulate(st, p, gbar));    // the pair block, on the same curves and bad[]
    return 0;
}

int shape_get(hipStream_t st, ShapeState* p, const char* name, void* h_out, int64_t bytes)
{
    const int64_t m = p->m;
    const ShapeLayout L = shape_layout(m);
    auto copy = [&](const void* src) -> int {
        GP_HIP(hipMemcpyAsync(h_out, src, (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 16); return copy(p->block + 10); }
    if (strcmp(name, "tols") == 0) { GP_ARG(bytes == 8 * GPIRT_SHAPE_MAX_TOLS); return copy(p->block + 6); }
    if (strcmp(name, "info") == 0) { GP_ARG(bytes == 8 * (int64_t)SH_N * m); return copy(p->info); }
    if (strcmp(name, "ti") == 0) { GP_ARG(bytes == 8 * (int64_t)SH_N); return copy(p->ti); }
    for (int k = 0; k < GPIRT_SHAPE_NARRAYS; ++k)
        if (strcmp(kShapeRaw[k], name) == 0) {
            GP_ARG(bytes == shape_raw_count(k, m) * shape_raw_width(k));
            return copy(p->block + L.off[k]);
        }
    set_error("unknown shape field '%s'", name);
    return GPIRT_E_ARG;
}

int shape_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_shape* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    for (int c = 0; c < chains; ++c) {
        GP_ARG(d_states[c]);
        if (signs) GP_ARG(signs[c] == 1 || signs[c] == -1);
    }
    HostShape pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostShape& r = c == 0 ? pooled : one;
        GP_TRY(shape_read(h->stream, d_states[c], r, "gpirt_shape_combine", c));
        if (c > 0 && (r.m != pooled.m || !std::equal(r.hdr() + 4, r.hdr() + 10, pooled.hdr() + 4))) {
            set_error("gpirt_shape_combine: state %d has another m, window or other tolerances than state 0", c);
            return GPIRT_E_ARG;
        }
        if (signs && signs[c] < 0) shape_reflect(r);
        if (c == 0) continue;
        pooled.hdr()[10] += one.hdr()[10];
        pooled.hdr()[11] += one.hdr()[11];
        for (int k = 0; k < GPIRT_SHAPE_NARRAYS; ++k) {
            const int64_t cnt = shape_raw_count(k, r.m);
            if (shape_raw_width(k) == 4) for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
            else for (int64_t g = 0; g < cnt; ++g) pooled.arr<double>(k)[g] += one.arr<double>(k)[g];      // in chain order
        }
    }
    shape_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
