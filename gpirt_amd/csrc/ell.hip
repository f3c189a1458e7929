// ell.hip -- the kernel's length scale as a parameter of the chain (gpirt_sampler_draw_ell, sampler.hip): the grid and its
// checks on the host, and the three kernels that decide and commit one prior-whitened Metropolis update (Murray & Adams 2010,
// section 2.2: nu = L(ell)^-1 f is held fixed, f' = L(ell') nu is what the likelihood sees).  Below them the three kernels of
// the centred update (gpirt_sampler_draw_ell_centred: f is held fixed and the GP prior N(f_j; 0, S(ell)) decides): the
// quadratic-form difference per item, the log-determinant difference, the decision.
//
// The log-likelihood term t(a) = log(1 + exp(-a)) is ll_term_fast (ll_fast.h): max(-a, 0) + log1p(exp(-|a|)) with the
// logarithm as 2 atanh(s).  Against the exact value it is within 2 ulp of the term (tests/test_ll_fast.py), i.e. at most
// 2 * 2^-52 * t(a) absolute per term; a cell's contribution t(y (f + mu)) - t(y (f' + mu)) is formed as that difference of two
// terms, cell by cell, never as a difference of two sums.
#include "common.h"
#include "kernels.h"
#include "ll_fast.h"

#include <cmath>

namespace gpirt {

namespace {

constexpr int ELL_THREADS = 256;

// One work-group per item j: thread t sums its rows i = t, t + 256, ... in ascending order, then a fixed LDS tree.  delta[j]
// and nonfin[j] (rows whose f' is not finite, observed or not: an accepted f' becomes f whole) have this one writer.
__global__ __launch_bounds__(ELL_THREADS) void ell_delta_kernel(const double* __restrict__ f, const double* __restrict__ fp,
                                                                const double* __restrict__ mu, const double* __restrict__ y,
                                                                int64_t n, double* __restrict__ delta, int* __restrict__ nonfin)
{
    __shared__ double sd[ELL_THREADS];
    __shared__ int sc[ELL_THREADS];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * n;
    const double* fj = f + base;
    const double* pj = fp + base;
    const double* mj = mu + base;
    const double* yj = y + base;
    double acc = 0.0;
    int bad = 0;
    auto cell = [&](double fv, double pv, double mv, double yv) {
        if (!(fabs(pv) <= 1.79769313486231570815e308)) ++bad;             // NaN or infinite
        if (yv == yv) acc += ll_term_fast(yv * (fv + mv)) - ll_term_fast(yv * (pv + mv));
    };
    int64_t i = tid;
    for (; i + 3 * ELL_THREADS < n; i += 4 * ELL_THREADS) {               // four rows' loads in flight, added in row order
        const int64_t i1 = i + ELL_THREADS, i2 = i + 2 * ELL_THREADS, i3 = i + 3 * ELL_THREADS;
        const double f0 = fj[i], f1 = fj[i1], f2 = fj[i2], f3 = fj[i3];
        const double p0 = pj[i], p1 = pj[i1], p2 = pj[i2], p3 = pj[i3];
        const double m0 = mj[i], m1 = mj[i1], m2 = mj[i2], m3 = mj[i3];
        const double y0 = yj[i], y1 = yj[i1], y2 = yj[i2], y3 = yj[i3];
        cell(f0, p0, m0, y0); cell(f1, p1, m1, y1); cell(f2, p2, m2, y2); cell(f3, p3, m3, y3);
    }
    for (; i < n; i += ELL_THREADS) cell(fj[i], pj[i], mj[i], yj[i]);
    sd[tid] = acc; sc[tid] = bad;
    __syncthreads();
#pragma unroll
    for (int s = ELL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) { sd[tid] += sd[tid + s]; sc[tid] += sc[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { delta[blockIdx.x] = sd[0]; nonfin[blockIdx.x] = sc[0]; }
}

// One work-group, one deciding thread: dll = delta[0] + ... + delta[m - 1] in ascending j, log_ratio = dll + lp_diff, accept iff
// log_u < log_ratio.  A factor that reported a non-positive minor or a hang-guard expiry (info[0], info[1]), a non-finite f' or
// dll: failed, never accepted.  rec = {dll, log_ratio, log_u, accept, nonfinite}; flag = 0 rejected, 1 accepted, 2 failed,
// 3 the hang guard expired (the host factors once more and decides again).
__global__ __launch_bounds__(ELL_THREADS) void ell_decide_kernel(const double* __restrict__ delta, const int* __restrict__ nonfin,
                                                                 int64_t m, double lp_diff, double log_u,
                                                                 const int* __restrict__ info, double* __restrict__ rec,
                                                                 int* __restrict__ flag)
{
    // all threads fetch 1024 items at a time into LDS, the one deciding thread adds them in ascending j: the order of the
    // additions is the serial one, the loads are not
    __shared__ double sd[4 * ELL_THREADS];
    __shared__ int sc[4 * ELL_THREADS];
    double dll = 0.0;
    long long bad = 0;
    for (int64_t j0 = 0; j0 < m; j0 += 4 * ELL_THREADS) {
        const int cnt = (int)(m - j0 < 4 * ELL_THREADS ? m - j0 : 4 * ELL_THREADS);
        for (int q = threadIdx.x; q < cnt; q += ELL_THREADS) { sd[q] = delta[j0 + q]; sc[q] = nonfin[j0 + q]; }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int q = 0; q < cnt; ++q) { dll += sd[q]; bad += sc[q]; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double ratio = dll + lp_diff;
    const bool failed = info[0] != 0 || info[1] != 0 || bad != 0 || !(fabs(dll) <= 1.79769313486231570815e308);
    const bool accept = !failed && log_u < ratio;
    rec[0] = dll; rec[1] = ratio; rec[2] = log_u; rec[3] = accept ? 1.0 : 0.0; rec[4] = (double)bad;
    *flag = info[1] != 0 ? 3 : failed ? 2 : (accept ? 1 : 0);
}

// f <- f' when the decision on the device says so: enqueued behind it, the copy does not wait for the host
__global__ __launch_bounds__(ELL_THREADS) void ell_commit_kernel(const int* __restrict__ flag, double* __restrict__ f,
                                                                 const double* __restrict__ fp, int64_t count)
{
    if (*flag != 1) return;
    const int64_t stride = (int64_t)gridDim.x * ELL_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * ELL_THREADS + threadIdx.x; i < count; i += stride) f[i] = fp[i];
}

// ---- the centred update: log p(f | ell') - log p(f | ell) = -0.5 sum_j (|nu'_j|^2 - |nu_j|^2) - m (log det L' - log det L) ----
// One work-group per item j, ell_delta_kernel's order: dq[j] = sum_i (nu'_ij - nu_ij) (nu'_ij + nu_ij), each cell that product
// (never a difference of two sums of squares); nonfin[j] = the rows whose nu' is not finite.  One writer each.
__global__ __launch_bounds__(ELL_THREADS) void ell_quad_kernel(const double* __restrict__ nu, const double* __restrict__ nup,
                                                               int64_t n, double* __restrict__ dq, int* __restrict__ nonfin)
{
    __shared__ double sd[ELL_THREADS];
    __shared__ int sc[ELL_THREADS];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * n;
    const double* aj = nu + base;
    const double* pj = nup + base;
    double acc = 0.0;
    int bad = 0;
    auto cell = [&](double av, double pv) {
        if (!(fabs(pv) <= 1.79769313486231570815e308)) ++bad;             // NaN or infinite
        acc += (pv - av) * (pv + av);
    };
    int64_t i = tid;
    for (; i + 3 * ELL_THREADS < n; i += 4 * ELL_THREADS) {               // four rows' loads in flight, added in row order
        const int64_t i1 = i + ELL_THREADS, i2 = i + 2 * ELL_THREADS, i3 = i + 3 * ELL_THREADS;
        const double a0 = aj[i], a1 = aj[i1], a2 = aj[i2], a3 = aj[i3];
        const double p0 = pj[i], p1 = pj[i1], p2 = pj[i2], p3 = pj[i3];
        cell(a0, p0); cell(a1, p1); cell(a2, p2); cell(a3, p3);
    }
    for (; i < n; i += ELL_THREADS) cell(aj[i], pj[i]);
    sd[tid] = acc; sc[tid] = bad;
    __syncthreads();
#pragma unroll
    for (int s = ELL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) { sd[tid] += sd[tid + s]; sc[tid] += sc[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { dq[blockIdx.x] = sd[0]; nonfin[blockIdx.x] = sc[0]; }
}

// One work-group: out[0] = dld = sum_i (log L'_ii - log L_ii), the diagonals at stride ldl + 1 (L: the saved buffer, L': the
// factor buffer); thread t takes its rows i = t, t + 256, ... ascending, four loads in flight, then the fixed tree.
// out[1] = the diagonal entries of either factor that are non-positive or non-finite (their terms are left out of the sum).
__global__ __launch_bounds__(ELL_THREADS) void ell_logdet_kernel(const double* __restrict__ Lold, const double* __restrict__ Lnew,
                                                                 int64_t n, int64_t ldl, double* __restrict__ out)
{
    __shared__ double sd[ELL_THREADS];
    __shared__ int sc[ELL_THREADS];
    const int tid = threadIdx.x;
    const int64_t step = ldl + 1;
    double acc = 0.0;
    int bad = 0;
    auto row = [&](double lo, double ln) {
        const bool ok_o = lo > 0.0 && lo <= 1.79769313486231570815e308, ok_n = ln > 0.0 && ln <= 1.79769313486231570815e308;
        if (ok_o && ok_n) acc += log(ln) - log(lo);
        else bad += (ok_o ? 0 : 1) + (ok_n ? 0 : 1);
    };
    int64_t i = tid;
    for (; i + 3 * ELL_THREADS < n; i += 4 * ELL_THREADS) {
        const int64_t i1 = i + ELL_THREADS, i2 = i + 2 * ELL_THREADS, i3 = i + 3 * ELL_THREADS;
        const double o0 = Lold[i * step], o1 = Lold[i1 * step], o2 = Lold[i2 * step], o3 = Lold[i3 * step];
        const double n0 = Lnew[i * step], n1 = Lnew[i1 * step], n2 = Lnew[i2 * step], n3 = Lnew[i3 * step];
        row(o0, n0); row(o1, n1); row(o2, n2); row(o3, n3);
    }
    for (; i < n; i += ELL_THREADS) row(Lold[i * step], Lnew[i * step]);
    sd[tid] = acc; sc[tid] = bad;
    __syncthreads();
#pragma unroll
    for (int s = ELL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) { sd[tid] += sd[tid + s]; sc[tid] += sc[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { out[0] = sd[0]; out[1] = (double)sc[0]; }
}

// One work-group, one deciding thread, as ell_decide_kernel: dq = dq[0] + ... + dq[m - 1] in ascending j, log_ratio =
// (-0.5 dq - m dld) + lp_diff with every product and sum rounded on its own, accept iff log_u < log_ratio.  Failed, never
// accepted: a factor that reported a non-positive minor or a hang-guard expiry, a non-finite nu', diagonal entry, dq or dld.
// rec = {dq, dld, log_ratio, log_u, accept, nonfinite}; flag as ell_decide_kernel's.
__global__ __launch_bounds__(ELL_THREADS) void ell_decide_centred_kernel(const double* __restrict__ dqj, const int* __restrict__ nonfin,
                                                                         int64_t m, const double* __restrict__ ld, double lp_diff,
                                                                         double log_u, const int* __restrict__ info,
                                                                         double* __restrict__ rec, int* __restrict__ flag)
{
    __shared__ double sd[4 * ELL_THREADS];
    __shared__ int sc[4 * ELL_THREADS];
    double dq = 0.0;
    long long bad = 0;
    for (int64_t j0 = 0; j0 < m; j0 += 4 * ELL_THREADS) {
        const int cnt = (int)(m - j0 < 4 * ELL_THREADS ? m - j0 : 4 * ELL_THREADS);
        for (int q = threadIdx.x; q < cnt; q += ELL_THREADS) { sd[q] = dqj[j0 + q]; sc[q] = nonfin[j0 + q]; }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int q = 0; q < cnt; ++q) { dq += sd[q]; bad += sc[q]; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double dld = ld[0];
    bad += (long long)ld[1];
    const double half = __dmul_rn(-0.5, dq), dets = __dmul_rn((double)m, dld);
    const double ratio = __dadd_rn(__dsub_rn(half, dets), lp_diff);
    const bool failed = info[0] != 0 || info[1] != 0 || bad != 0 || !(fabs(dq) <= 1.79769313486231570815e308) ||
                        !(fabs(dld) <= 1.79769313486231570815e308);
    const bool accept = !failed && log_u < ratio;
    rec[0] = dq; rec[1] = dld; rec[2] = ratio; rec[3] = log_u; rec[4] = accept ? 1.0 : 0.0; rec[5] = (double)bad;
    *flag = info[1] != 0 ? 3 : failed ? 2 : (accept ? 1 : 0);
}

}  // namespace

int launch_ell_delta(hipStream_t st, const double* f, const double* fp, const double* mu, const double* y, int64_t n, int64_t m,
                     double* delta, int* nonfin)
{
    hipLaunchKernelGGL(ell_delta_kernel, dim3((unsigned)m), dim3(ELL_THREADS), 0, st, f, fp, mu, y, n, delta, nonfin);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ell_decide(hipStream_t st, const double* delta, const int* nonfin, int64_t m, double lp_diff, double log_u,
                      const int* info, double* rec, int* flag)
{
    hipLaunchKernelGGL(ell_decide_kernel, dim3(1), dim3(ELL_THREADS), 0, st, delta, nonfin, m, lp_diff, log_u, info, rec, flag);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ell_commit(hipStream_t st, const int* flag, double* f, const double* fp, int64_t count)
{
    int64_t blocks = (count + ELL_THREADS - 1) / ELL_THREADS;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(ell_commit_kernel, dim3((unsigned)blocks), dim3(ELL_THREADS), 0, st, flag, f, fp, count);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ell_quad(hipStream_t st, const double* nu, const double* nup, int64_t n, int64_t m, double* dq, int* nonfin)
{
    hipLaunchKernelGGL(ell_quad_kernel, dim3((unsigned)m), dim3(ELL_THREADS), 0, st, nu, nup, n, dq, nonfin);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ell_logdet(hipStream_t st, const double* Lold, const double* Lnew, int64_t n, int64_t ldl, double* out)
{
    hipLaunchKernelGGL(ell_logdet_kernel, dim3(1), dim3(ELL_THREADS), 0, st, Lold, Lnew, n, ldl, out);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ell_decide_centred(hipStream_t st, const double* dq, const int* nonfin, int64_t m, const double* ld, double lp_diff,
                              double log_u, const int* info, double* rec, int* flag)
{
    hipLaunchKernelGGL(ell_decide_centred_kernel, dim3(1), dim3(ELL_THREADS), 0, st, dq, nonfin, m, ld, lp_diff, log_u, info, rec, flag);
    GP_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- host: the grid and its checks -----------------------------
int ell_grid_check(double lo, double hi, int P)
{
    if (P < 2 || P > GPIRT_ELL_MAX_POINTS) {
        set_error("length-scale grid: P = %d points, it must lie in 2 .. %d", P, GPIRT_ELL_MAX_POINTS);
        return GPIRT_E_ARG;
    }
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo >= GPIRT_LENGTH_SCALE_MIN) || !(hi <= GPIRT_LENGTH_SCALE_MAX) || !(lo < hi)) {
        set_error("length-scale grid: lo = %g, hi = %g, they must satisfy %g <= lo < hi <= %g", lo, hi,
                  (double)GPIRT_LENGTH_SCALE_MIN, (double)GPIRT_LENGTH_SCALE_MAX);
        return GPIRT_E_ARG;
    }
    return 0;
}

void ell_grid_fill(double lo, double hi, int P, double* out)
{
    const long double ratio = (long double)hi / (long double)lo;
    for (int k = 0; k < P; ++k)
        out[k] = (double)((long double)lo * powl(ratio, (long double)k / (long double)(P - 1)));
    out[0] = lo; out[P - 1] = hi;
}

}  // namespace gpirt

using namespace gpirt;

extern "C" {

int gpirt_ell_grid(double lo, double hi, int P, double* out)
{
    GP_TRY(ell_grid_check(lo, hi, P));
    GP_ARG(out != nullptr);
    ell_grid_fill(lo, hi, P, out);
    for (int k = 1; k < P; ++k)
        if (!(out[k] > out[k - 1])) {
            set_error("length-scale grid: %d points between %.17g and %.17g are not strictly increasing in fp64", P, lo, hi);
            return GPIRT_E_ARG;
        }
    return 0;
}

int gpirt_ell_check(double lo, double hi, int P, const double* log_prior, int width, int k0, const gpirt_kernel* kern,
                    const gpirt_options* opts, int64_t m)
{
    std::vector<double> grid((size_t)(P > 0 && P <= GPIRT_ELL_MAX_POINTS ? P : 1));
    GP_TRY(gpirt_ell_grid(lo, hi, P, grid.data()));
    if (log_prior)
        for (int k = 0; k < P; ++k)
            if (!std::isfinite(log_prior[k])) { set_error("length scale: log_prior[%d] is not finite", k); return GPIRT_E_ARG; }
    if (width < 1 || width > P - 1) {
        set_error("length scale: width = %d, it must lie in 1 .. P - 1 = %d", width, P - 1);
        return GPIRT_E_ARG;
    }
    if (k0 < -1 || k0 >= P) {
        set_error("length scale: starting index k0 = %d, it must lie in 0 .. P - 1 = %d (-1: the handle's length scale)", k0, P - 1);
        return GPIRT_E_ARG;
    }
    int rank = 0;
    if (opts) {
        if (opts->rng_kind == GPIRT_RNG_RSTREAM) {
            set_error("length scale: rng = reference (GPIRT_RNG_RSTREAM) is refused, R's stream has no such draw");
            return GPIRT_E_ARG;
        }
        if (opts->kernel_fp32) {
            set_error("length scale: kernel_fp32 is refused, the single-precision build is the default kernel's alone");
            return GPIRT_E_ARG;
        }
        if (opts->item0 != 0 || (opts->m_total > 0 && m > 0 && opts->m_total != m)) {
            set_error("length scale: an item shard (item0 = %lld, m_total = %lld) is refused, the likelihood change runs over all items",
                      (long long)opts->item0, (long long)opts->m_total);
            return GPIRT_E_ARG;
        }
        rank = opts->fstar_fused ? opts->kstar_rank : 0;
    }
    if (kern) {
        KernelSpec spec;
        GP_TRY(kernel_spec_from(kern, &spec));
        bool on_grid = false;
        for (int k = 0; k < P; ++k) on_grid = on_grid || grid[(size_t)k] == spec.length_scale;
        if (!on_grid) {
            set_error("length scale: the handle's length_scale = %.17g is not a point of the grid (%d points, %.17g .. %.17g)",
                      spec.length_scale, P, lo, hi);
            return GPIRT_E_ARG;
        }
        if (rank != 0) {
            // the certificate grows as the length scale shrinks: passing at ell_0 = lo covers the whole grid
            KernelSpec at_lo = spec;
            at_lo.length_scale = lo; at_lo.inv_ell = 1.0 / lo;
            GP_TRY(kernel_rank_check(at_lo, rank, nullptr, nullptr));
        }
    }
    return 0;
}

}  // extern "C"
