// ordinal_score.hip -- scoring respondents who were not in the fit under ordinal (graded) responses, their category predictions and
// the item to ask them next (include/gpirt_hip.h, "scoring new respondents under ordinal responses"; library
// version 144).  cat_new: n_new x m int8, 0 = missing, 1 .. C a category, over the sampler's items and categories.
//
// Part A.  Per counted draw, with that draw's f* (it carries mu*; the intercept is pinned at 0) and thresholds b_{j,c},
//     T[k, r] = sum over r's observed cells of  -ll(b_c - f*[k,j]) [c < C]  - ll(f*[k,j] - b_{c-1}) [c > 1],   c = cat_new[r, j]
// is exactly the product theta_product_ord (sampler.hip) forms for the chain's respondents, so launch_oscore_accumulate CALLS its
// launchers -- launch_ord_loglik_terms, launch_gemm with K = C m against the one-hot launch_ord_indicators(cat_new), and
// launch_ord_nan_fix -- on the block's own operands: its own table G, never the chain's (the chain's table holds whatever curve
// draw_theta or a proposal last put there).  The w term that draw_theta may drop is free of theta but not of the draw:
//     Wc[r] = sum over r's observed cells with 1 < c < C of  log1p(-exp(-(b_c - b_{c-1})))
// oscore_wtab_kernel builds the m x C table of w from the thresholds, oscore_wc_kernel sums it per respondent in ascending item order
// (one thread owns a respondent), and the accumulate kernel adds it to l AFTER the normaliser: l = M + log Z - lse_prior + Wc[r].  It
// never enters T: the grid weights do not see it.
//
// The NaN contract is score.hip's: a NaN cell of f* skips the draw only for the respondents who answered that item.  The product is
// formed from a cleaned copy of f* (NaN -> 0, the item marked), oscore_flag_kernel flags the respondents with cat_new != 0 at a marked
// item; they are counted in nonfinite and nothing else of theirs is touched.  +-inf is left as it is: the table holds such a term
// at -1e300, which is finite.
//
// oscore_accumulate_kernel is score_accumulate_kernel's geometry: one wave per respondent, four respondents per 256-lane work-group,
// lanes stride k (k = lane + 64 i, i < 16), the 16 values of a lane in registers, max and sum through the xor butterfly whose partners
// add the same two numbers in either order.  No LDS, no scratch, no atomics; lane 0 keeps the respondent's scalars.
//
// Part B (predict).  The WEIGHTS instantiation leaves the draw's weights in W (Np x n_new) and the go-flag "no NaN in this f*":
//   oscore_operands_kernel  B = [P_1 | ... | P_C | Hc] (Np x (C + 1) m), one (k, j) a thread.  From ONE E_c = exp(-|f* - b_c|) per
//                           threshold: l_c = log1p(E_c), up_c = l_c + max(f* - b_c, 0) = ll(b_c - f*), lo_c = l_c + max(b_c - f*, 0)
//                           = ll(f* - b_c);  logP_c = -up_c [c < C] - lo_{c-1} [c > 1] + w_c [1 < c < C];  P_c = exp(logP_c) -- never
//                           a difference of two sigmas;  Hc = -sum_c P_c logP_c in ascending c, a term with P_c = 0 left out
//   launch_gemm             W^T B (n_new x (C + 1) m) on the fp64 matrix cores, conditional on the go-flag (one kernel, a fixed
//                           order); K runs over all Np rows, the padding rows of both operands are zero
//   oscore_epilogue_kernel  one thread per (r, j): q_c = the C products, h(q) = -sum_c q_c log q_c (q_c clamped to <= 1, 0 log 0 = 0,
//                           ascending c), info = h(q) - the Hc product; prob_sum[c][j][r] += q_c, info_sum[j][r] += info.  Each cell
//                           has one owner; one lane keeps pred_draws / pred_skipped in the header.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace gpirt {

namespace {

constexpr int NG = GPIRT_NGRID;
constexpr int64_t NP = (NG + 127) / 128 * 128;       // 1024
constexpr int OS_THREADS = 256;
constexpr int OS_WAVES = OS_THREADS / 64;
constexpr int OS_PER_LANE = (NG + 63) / 64;          // 16
static_assert(OS_PER_LANE * 64 >= NG, "a wave covers the grid");

struct OscoreLayout { int64_t draws, nonfinite, n_obs, lpd_acc, ll_sum, post_sum, words; };
OscoreLayout oscore_layout(int64_t n)
{
    OscoreLayout L;
    L.draws = OSCORE_HEADER_WORDS; L.nonfinite = L.draws + n; L.n_obs = L.nonfinite + n;
    L.lpd_acc = L.n_obs + n; L.ll_sum = L.lpd_acc + n; L.post_sum = L.ll_sum + n;
    L.words = L.post_sum + n * NG;
    return L;
}

struct OspredLayout { int64_t mask, prob_sum, info_sum, words; };
OspredLayout ospred_layout(int64_t n, int64_t m, int C)
{
    OspredLayout L;
    L.mask = OSCORE_HEADER_WORDS;
    L.prob_sum = L.mask + (n * m + 63) / 64;
    L.info_sum = L.prob_sum + (int64_t)C * n * m;
    L.words = L.info_sum + n * m;
    return L;
}

inline unsigned os_grid_for(int64_t total)
{
    int64_t b = (total + 255) / 256;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// flags: [0] any NaN in this draw's f*, [1 .. m] the item holds one, then bad[n_new]: the respondent answered such an item
__global__ __launch_bounds__(256) void oscore_clean_kernel(const double* __restrict__ fstar, int64_t N, int64_t m,
                                                           double* __restrict__ clean, int* __restrict__ flags)
{
    const int64_t total = N * m;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const double v = fstar[g];
        const bool nan = v != v;
        clean[g] = nan ? 0.0 : v;
        if (nan) { flags[0] = 1; flags[1 + g / N] = 1; }
    }
}

__global__ __launch_bounds__(256) void oscore_flag_kernel(const int8_t* __restrict__ cat, int64_t n, int64_t m, int* __restrict__ flags)
{
    if (flags[0] == 0) return;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    int bad = 0;
    for (int64_t j = 0; j < m; ++j)
        if (flags[1 + j] != 0 && cat[r + j * n] != 0) bad = 1;
    flags[1 + m + r] = bad;
}

// wtab[j C + c - 1] = w(b_c - b_{c-1}) = log1p(-exp(-(b_c - b_{c-1}))) for 1 < c < C, 0 for the two end categories
__global__ __launch_bounds__(256) void oscore_wtab_kernel(const double* __restrict__ thr, int64_t m, int C, double* __restrict__ wtab)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= m * C) return;
    const int64_t j = g / C;
    const int c = (int)(g - j * C) + 1;
    double w = 0.0;
    if (c > 1 && c < C) {
        const double* b = thr + j * (C - 1);               // b[c - 1] = b_c
        w = log1p(-exp(-(b[c - 1] - b[c - 2])));
    }
    wtab[g] = w;
}

// Wc[r]: r's observed interior cells in ascending item order, one owner per respondent
__global__ __launch_bounds__(256) void oscore_wc_kernel(const int8_t* __restrict__ cat, int64_t n, int64_t m, int C,
                                                        const double* __restrict__ wtab, double* __restrict__ Wc)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    double acc = 0.0;
    for (int64_t j = 0; j < m; ++j) {
        const int c = cat[r + j * n];
        if (c > 1 && c < C) acc += wtab[j * C + c - 1];
    }
    Wc[r] = acc;
}

struct OscoreArgs {
    const double* T;            // N x n_new, the product
    const double* logprior;     // N
    const double* Wc;           // n_new
    const int* bad;             // n_new
    double lse_prior;
    int64_t n;
    int64_t* draws; int64_t* nonfinite;
    double* lpd_acc; double* ll_sum; double* post_sum;
    // WEIGHTS instantiation only: this draw's w_k to W[r ldw + k], and go = "no NaN in this draw's f*"
    double* W; int64_t ldw; const int* nan_flag; int* go;
};

__device__ __forceinline__ double os_wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ double os_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <bool WEIGHTS>
__global__ __launch_bounds__(OS_THREADS) void oscore_accumulate_kernel(OscoreArgs a)
{
    const int lane = (int)(threadIdx.x & 63);
    const int64_t r = (int64_t)blockIdx.x * OS_WAVES + (threadIdx.x >> 6);
    if (WEIGHTS && blockIdx.x == 0 && threadIdx.x == 0) *a.go = (*a.nan_flag == 0) ? 1 : 0;
    if (r >= a.n) return;                                // (a whole wave: nothing below waits for another wave)
    const double* __restrict__ T = a.T + r * NG;
    double* __restrict__ post = a.post_sum + r * NG;
    double lp[OS_PER_LANE];
    bool ok = a.bad[r] == 0;
#pragma unroll
    for (int i = 0; i < OS_PER_LANE; ++i) {
        const int k = lane + 64 * i;
        if (k < NG) {
            lp[i] = a.logprior[k] + T[k];
            ok = ok && isfinite(lp[i]);
        } else lp[i] = -INFINITY;
    }
    if (!__all(ok)) {                                    // this draw is skipped for r alone, nothing else of r changes
        if (lane == 0) a.nonfinite[r] += 1;
        return;
    }
    double M = lp[0];
#pragma unroll
    for (int i = 1; i < OS_PER_LANE; ++i) M = fmax(M, lp[i]);
    M = os_wave_max(M);
    double Z = 0.0;
#pragma unroll
    for (int i = 0; i < OS_PER_LANE; ++i) {
        lp[i] = exp(lp[i] - M);                          // (beyond the grid: exp(-inf) = 0)
        Z += lp[i];
    }
    Z = os_wave_sum(Z);
#pragma unroll
    for (int i = 0; i < OS_PER_LANE; ++i) {
        const int k = lane + 64 * i;
        if (k < NG) {
            const double w = lp[i] / Z;
            post[k] += w;
            if (WEIGHTS) a.W[r * a.ldw + k] = w;
        }
    }
    if (lane == 0) {
        const double l = ((M + log(Z)) - a.lse_prior) + a.Wc[r];
        const double acc = a.lpd_acc[r];
        const double hi = fmax(acc, l), lo = fmin(acc, l);
        a.lpd_acc[r] = lo == -INFINITY ? hi : hi + log1p(exp(lo - hi));
        a.ll_sum[r] += l;
        a.draws[r] += 1;
    }
}

// B[k + ((c - 1) m + j) ldb] = P_c, B[k + (C m + j) ldb] = Hc for k < N; rows N .. ldb - 1 are never written (zero since the allocation)
__global__ __launch_bounds__(256) void oscore_operands_kernel(const double* __restrict__ fclean, int64_t N, int64_t m, int C,
                                                              const double* __restrict__ thr, const double* __restrict__ wtab,
                                                              double* __restrict__ B, int64_t ldb, const int* __restrict__ go)
{
    if (*go == 0) return;
    const int64_t total = N * m;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t j = g / N, k = g - j * N;
        const double v = fclean[g];
        const double* b = thr + j * (C - 1);               // b[c - 1] = b_c
        const double* wj = wtab + j * C;
        double lo_prev = 0.0, H = 0.0;
        for (int c = 1; c <= C; ++c) {
            double up = 0.0, lo = 0.0;
            if (c < C) {
                const double d = v - b[c - 1];
                const double E = exp(-fabs(d));
                const double l1 = log1p(E);
                up = l1 + fmax(d, 0.0);
                lo = l1 + fmax(-d, 0.0);
            }
            double lp = 0.0;
            if (c < C) lp = -up;
            if (c > 1) lp = lp - lo_prev;
            if (c > 1 && c < C) lp = lp + wj[c - 1];
            const double P = exp(lp);
            B[k + ((int64_t)(c - 1) * m + j) * ldb] = P;
            if (P > 0.0) H = H - P * lp;
            lo_prev = lo;
        }
        B[k + ((int64_t)C * m + j) * ldb] = H;
    }
}

__global__ __launch_bounds__(256) void oscore_epilogue_kernel(const double* __restrict__ Cm, int64_t n, int64_t m, int C,
                                                              double* __restrict__ prob_sum, double* __restrict__ info_sum,
                                                              int64_t* __restrict__ counters, const int* __restrict__ go)
{
    const bool run = *go != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[run ? 0 : 1] += 1;         // pred_draws / pred_skipped
    if (!run) return;
    const int64_t total = n * m;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        double h = 0.0;
        for (int c = 0; c < C; ++c) {
            const double q = Cm[g + (int64_t)c * total];
            prob_sum[g + (int64_t)c * total] += q;
            const double qc = fmin(q, 1.0);
            if (qc > 0.0) h = h - qc * log(qc);
        }
        info_sum[g] += h - Cm[g + (int64_t)C * total];
    }
}

// log dnorm(theta*_k) as draw_theta adds it (score.hip's score_logprior: no transcendental, so the host table is its bits)
void oscore_logprior(double* lp, double* lse)
{
    long double s = 0.0L;
    double mx = -INFINITY;
    const double ln_sqrt_2pi = 0.918938533204672741780329736406;
    for (int k = 0; k < NG; ++k) {
        const double z = fabs(-5.0 + (double)k * 0.01);
        lp[k] = -(ln_sqrt_2pi + 0.5 * z * z);
        mx = std::max(mx, lp[k]);
    }
    for (int k = 0; k < NG; ++k) s += expl((long double)lp[k] - (long double)mx);
    *lse = (double)((long double)mx + logl(s));
}

double os_logaddexp(double a, double b)
{
    const double hi = std::max(a, b), lo = std::min(a, b);
    return lo == -INFINITY ? hi : hi + log1p(exp(lo - hi));
}

// a block's header on the host: refuses anything but a block of the tag
int oscore_read_header(hipStream_t st, const void* d_block, int64_t tag, int64_t* hdr, const char* who, int c)
{
    GP_HIP(hipMemcpyAsync(hdr, d_block, sizeof(int64_t) * OSCORE_HEADER_WORDS, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] != tag || hdr[1] != OSCORE_LAYOUT_VERSION || hdr[2] < 1 || hdr[2] > GPIRT_SCORE_MAX_N || hdr[3] < 1 || hdr[4] < 2 ||
        hdr[4] > GPIRT_ORD_MAX_C || hdr[5] != NG || hdr[6] < 0 || hdr[7] < 0) {
        set_error("%s: state %d is not an ordinal %s state block of layout %d", who, c, tag == OSCORE_TAG ? "score" : "predict",
                  OSCORE_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    return 0;
}

}  // namespace

int64_t oscore_state_words(const OscoreState* s) { return oscore_layout(s->n).words; }
int64_t oscore_pred_state_words(const OscoreState* s) { return ospred_layout(s->n, s->m, s->C).words; }

int oscore_alloc(hipStream_t st, OscoreState* s, const int8_t* h_cat, int64_t n_new, int64_t m, int C, bool predict)
{
    // every refusal before anything is touched
    if (!h_cat || n_new < 1 || n_new > GPIRT_SCORE_MAX_N) {
        set_error("ordinal scoring: n_new = %lld is outside 1..%d", (long long)n_new, GPIRT_SCORE_MAX_N);
        return GPIRT_E_ARG;
    }
    for (int64_t g = 0; g < n_new * m; ++g)
        if (h_cat[g] < 0 || h_cat[g] > C) {
            set_error("ordinal scoring: cat_new[%lld, %lld] = %d, it must lie in 0 .. C = %d (0 = missing)", (long long)(g % n_new),
                      (long long)(g / n_new), (int)h_cat[g], C);
            return GPIRT_E_ARG;
        }
    const int64_t N = NG;
    s->n = n_new; s->m = m; s->C = C;
    const OscoreLayout L = oscore_layout(n_new);
    auto get = [&](void** p, size_t bytes, bool zero) -> int {
        GP_HIP(hipMalloc(p, bytes));
        s->allocs.push_back(*p);
        if (zero) GP_HIP(hipMemsetAsync(*p, 0, bytes, st));
        return 0;
    };
    const size_t Cm = (size_t)C * (size_t)m;
    GP_TRY(get((void**)&s->block, sizeof(uint64_t) * (size_t)L.words, true));
    GP_TRY(get((void**)&s->cat, (size_t)(n_new * m), false));
    GP_TRY(get((void**)&s->Y, sizeof(double) * (size_t)n_new * Cm, false));
    GP_TRY(get((void**)&s->G, sizeof(double) * ((size_t)NP * Cm + 2), true));               // the padding rows stay zero
    GP_TRY(get((void**)&s->T, sizeof(double) * (size_t)(N * n_new + 2), true));
    GP_TRY(get((void**)&s->fclean, sizeof(double) * (size_t)(N * m + 2), true));
    GP_TRY(get((void**)&s->flags, sizeof(int) * (size_t)(1 + m + n_new), true));
    GP_TRY(get((void**)&s->logprior, sizeof(double) * (size_t)N, false));
    GP_TRY(get((void**)&s->wtab, sizeof(double) * Cm, true));
    GP_TRY(get((void**)&s->Wc, sizeof(double) * (size_t)n_new, true));
    // the header, the observed cells and lpd_acc = -inf in front of the zeroed sums
    std::vector<uint64_t> head((size_t)L.post_sum, 0);
    int64_t* hi = reinterpret_cast<int64_t*>(head.data());
    double* hd = reinterpret_cast<double*>(head.data());
    hi[0] = OSCORE_TAG; hi[1] = OSCORE_LAYOUT_VERSION; hi[2] = n_new; hi[3] = m; hi[4] = C; hi[5] = N;
    for (int64_t r = 0; r < n_new; ++r) {
        int64_t c = 0;
        for (int64_t j = 0; j < m; ++j) c += h_cat[r + j * n_new] != 0;
        hi[L.n_obs + r] = c;
        hd[L.lpd_acc + r] = -INFINITY;
    }
    double lp[NG];
    oscore_logprior(lp, &s->lse_prior);
    GP_HIP(hipMemcpyAsync(s->block, head.data(), sizeof(uint64_t) * head.size(), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(s->logprior, lp, sizeof(lp), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(s->cat, h_cat, (size_t)(n_new * m), hipMemcpyHostToDevice, st));
    GP_TRY(launch_ord_indicators(st, s->cat, n_new, m, C, s->Y));
    std::vector<uint64_t> phead;
    if (predict) {
        const OspredLayout P = ospred_layout(n_new, m, C);
        GP_TRY(get((void**)&s->pblock, sizeof(uint64_t) * (size_t)P.words, true));
        GP_TRY(get((void**)&s->W, sizeof(double) * (size_t)(NP * n_new), true));           // the padding rows stay zero
        GP_TRY(get((void**)&s->B, sizeof(double) * (size_t)NP * (Cm + (size_t)m), true));  // ... and these
        GP_TRY(get((void**)&s->Cm, sizeof(double) * (size_t)n_new * (Cm + (size_t)m), true));
        GP_TRY(get((void**)&s->go, sizeof(int) * 4, true));
        phead.assign((size_t)P.prob_sum, 0);
        int64_t* pi = reinterpret_cast<int64_t*>(phead.data());
        pi[0] = OSPRED_TAG; pi[1] = OSCORE_LAYOUT_VERSION; pi[2] = n_new; pi[3] = m; pi[4] = C; pi[5] = N;
        for (int64_t g = 0; g < n_new * m; ++g)
            if (h_cat[g] != 0) phead[(size_t)(P.mask + (g >> 6))] |= (uint64_t)1 << (g & 63);
        GP_HIP(hipMemcpyAsync(s->pblock, phead.data(), sizeof(uint64_t) * phead.size(), hipMemcpyHostToDevice, st));
    }
    GP_HIP(hipStreamSynchronize(st));        // head, phead, lp are this call's; h_cat is the caller's
    s->pred_on = predict;
    s->on = true;
    return 0;
}

void oscore_free(OscoreState* s)
{
    for (void* p : s->allocs) hipFree(p);
    *s = OscoreState{};
}

int launch_oscore_accumulate(gpirt_handle_t h, hipStream_t st, OscoreState* s, const double* fstar, const double* thr)
{
    const int64_t N = NG, n = s->n, m = s->m;
    const int C = s->C;
    GP_HIP(hipMemsetAsync(s->flags, 0, sizeof(int) * (size_t)(1 + m + n), st));
    hipLaunchKernelGGL(oscore_clean_kernel, dim3(os_grid_for(N * m)), dim3(256), 0, st, fstar, N, m, s->fclean, s->flags);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(oscore_flag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->cat, n, m, s->flags);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(oscore_wtab_kernel, dim3((unsigned)((m * C + 255) / 256)), dim3(256), 0, st, thr, m, C, s->wtab);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(oscore_wc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->cat, n, m, C, s->wtab, s->Wc);
    GP_HIP(hipGetLastError());
    // the product, as theta_product_ord launches it (sampler.hip), on the block's own operands
    GP_TRY(launch_ord_loglik_terms(st, s->fclean, N, m, C, thr, s->G, NP));
    GP_TRY(launch_gemm(h, st, false, true, TRI_NONE, N, n, (int64_t)C * m, 1.0, s->G, NP, s->Y, n, 0.0, s->T, N, NP));
    GP_TRY(launch_ord_nan_fix(st, s->G, NP, s->cat, n, m, s->T, N, N));
    const OscoreLayout L = oscore_layout(n);
    OscoreArgs a{};
    a.T = s->T; a.logprior = s->logprior; a.Wc = s->Wc; a.bad = s->flags + 1 + m; a.lse_prior = s->lse_prior; a.n = n;
    a.draws = reinterpret_cast<int64_t*>(s->block + L.draws);
    a.nonfinite = reinterpret_cast<int64_t*>(s->block + L.nonfinite);
    a.lpd_acc = reinterpret_cast<double*>(s->block + L.lpd_acc);
    a.ll_sum = reinterpret_cast<double*>(s->block + L.ll_sum);
    a.post_sum = reinterpret_cast<double*>(s->block + L.post_sum);
    const dim3 grid((unsigned)((n + OS_WAVES - 1) / OS_WAVES));
    if (!s->pred_on) {
        hipLaunchKernelGGL(oscore_accumulate_kernel<false>, grid, dim3(OS_THREADS), 0, st, a);
        GP_HIP(hipGetLastError());
        return 0;
    }
    a.W = s->W; a.ldw = NP; a.nan_flag = s->flags; a.go = s->go;
    hipLaunchKernelGGL(oscore_accumulate_kernel<true>, grid, dim3(OS_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    const OspredLayout P = ospred_layout(n, m, C);
    hipLaunchKernelGGL(oscore_operands_kernel, dim3(os_grid_for(N * m)), dim3(256), 0, st, s->fclean, N, m, C, thr, s->wtab, s->B, NP,
                       s->go);
    GP_HIP(hipGetLastError());
    GP_TRY(launch_gemm(h, st, true, false, TRI_NONE, n, (int64_t)(C + 1) * m, NP, 1.0, s->W, NP, s->B, NP, 0.0, s->Cm, n, 0, s->go));
    hipLaunchKernelGGL(oscore_epilogue_kernel, dim3(os_grid_for(n * m)), dim3(256), 0, st, s->Cm, n, m, C,
                       reinterpret_cast<double*>(s->pblock + P.prob_sum), reinterpret_cast<double*>(s->pblock + P.info_sum),
                       reinterpret_cast<int64_t*>(s->pblock + 6), s->go);
    GP_HIP(hipGetLastError());
    return 0;
}

int oscore_get(hipStream_t st, OscoreState* s, const char* name, void* h_out, int64_t bytes)
{
    const int64_t n = s->n, m = s->m;
    const int C = s->C;
    const OscoreLayout L = oscore_layout(n);
    const OspredLayout P = ospred_layout(n, m, C);
    auto fetch = [&](const void* src, int64_t want) -> int {
        if (bytes != want) {
            set_error("ordinal scoring: '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes);
            return GPIRT_E_ARG;
        }
        GP_HIP(hipMemcpyAsync(h_out, src, (size_t)want, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    const struct { const char* name; const void* src; int64_t bytes; } raw[] = {
        { "draws", s->block + L.draws, 8 * n }, { "nonfinite", s->block + L.nonfinite, 8 * n }, { "n_obs", s->block + L.n_obs, 8 * n },
        { "lpd_acc", s->block + L.lpd_acc, 8 * n }, { "ll_sum", s->block + L.ll_sum, 8 * n },
        { "post_sum", s->block + L.post_sum, 8 * n * NG }, { "product", s->T, 8 * n * NG }, { "wc", s->Wc, 8 * n },
        { "w_table", s->wtab, 8 * m * C },
    };
    for (const auto& e : raw)
        if (strcmp(e.name, name) == 0) return fetch(e.src, e.bytes);
    static const char* const pred_names[] = { "prob_sum", "info_sum", "counts", "weights", "operands" };
    int which = -1;
    for (int d = 0; d < 5; ++d) if (strcmp(name, pred_names[d]) == 0) which = d;
    if (which < 0) { set_error("unknown ordinal score field '%s'", name); return GPIRT_E_ARG; }
    if (!s->pred_on) {
        set_error("ordinal scoring: '%s' needs the prediction part, which is not enabled (gpirt_sampler_ordinal_score_enable with predict = 1)", name);
        return GPIRT_E_ARG;
    }
    if (which == 0) return fetch(s->pblock + P.prob_sum, 8 * (int64_t)C * n * m);
    if (which == 1) return fetch(s->pblock + P.info_sum, 8 * n * m);
    if (which == 2) return fetch(s->pblock + 6, 16);
    if (which == 4) {                                     // B of the last counted draw: N x (C + 1) m out of the Np-row buffer
        const int64_t cols = (int64_t)(C + 1) * m;
        GP_ARG(bytes == 8 * cols * NG);
        GP_HIP(hipMemcpy2DAsync(h_out, 8 * (size_t)NG, s->B, 8 * (size_t)NP, 8 * (size_t)NG, (size_t)cols, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    GP_ARG(bytes == 8 * n * NG);                          // W of the last counted draw: N x n_new out of the Np x n_new buffer
    GP_HIP(hipMemcpy2DAsync(h_out, 8 * (size_t)NG, s->W, 8 * (size_t)NP, 8 * (size_t)NG, (size_t)n, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

int oscore_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, void* h_out, int64_t bytes)
{
    GP_ARG(h && chains >= 1 && d_states && h_out);
    const char* me = "gpirt_ordinal_score_combine";
    for (int c = 0; c < chains; ++c) {
        GP_ARG(d_states[c]);
        if (signs) GP_ARG(signs[c] == 1 || signs[c] == -1);
    }
    hipStream_t st = h->stream;
    std::vector<uint64_t> one;
    uint64_t* pooled = static_cast<uint64_t*>(h_out);
    OscoreLayout L{};
    int64_t hdr0[OSCORE_HEADER_WORDS];
    for (int c = 0; c < chains; ++c) {
        int64_t hdr[OSCORE_HEADER_WORDS];
        GP_TRY(oscore_read_header(st, d_states[c], OSCORE_TAG, hdr, me, c));
        if (c == 0) {
            memcpy(hdr0, hdr, sizeof(hdr));
            L = oscore_layout(hdr[2]);
            if (bytes != 8 * L.words) { set_error("%s: the pooled block holds %lld bytes, %lld were given", me, (long long)(8 * L.words), (long long)bytes); return GPIRT_E_ARG; }
            one.resize((size_t)L.words);
        } else if (hdr[2] != hdr0[2] || hdr[3] != hdr0[3] || hdr[4] != hdr0[4]) {
            set_error("%s: state %d has another n_new, m or C than state 0", me, c);
            return GPIRT_E_ARG;
        }
        uint64_t* dst = c == 0 ? pooled : one.data();
        GP_HIP(hipMemcpyAsync(dst, d_states[c], sizeof(uint64_t) * (size_t)L.words, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        const int64_t n = hdr0[2];
        double* post = reinterpret_cast<double*>(dst + L.post_sum);
        if (signs && signs[c] < 0)                       // theta -> -theta: post_sum[r][k] <-> post_sum[r][1000 - k]
            for (int64_t i = 0; i < n; ++i) std::reverse(post + i * NG, post + (i + 1) * NG);
        if (c == 0) continue;
        int64_t* pi = reinterpret_cast<int64_t*>(pooled);
        double* pd = reinterpret_cast<double*>(pooled);
        const int64_t* oi = reinterpret_cast<const int64_t*>(one.data());
        const double* od = reinterpret_cast<const double*>(one.data());
        for (int64_t i = 0; i < n; ++i) {
            if (oi[L.n_obs + i] != pi[L.n_obs + i]) {
                set_error("%s: state %d was built on another cat_new than state 0", me, c);
                return GPIRT_E_ARG;
            }
            pi[L.draws + i] += oi[L.draws + i];
            pi[L.nonfinite + i] += oi[L.nonfinite + i];
            pd[L.ll_sum + i] += od[L.ll_sum + i];
            pd[L.lpd_acc + i] = os_logaddexp(pd[L.lpd_acc + i], od[L.lpd_acc + i]);
        }
        for (int64_t k = 0; k < n * NG; ++k) pd[L.post_sum + k] += od[L.post_sum + k];
    }
    return 0;
}

int oscore_pred_combine(gpirt_handle_t h, int chains, const void* const* d_states, void* h_out, int64_t bytes)
{
    GP_ARG(h && chains >= 1 && d_states && h_out);
    const char* me = "gpirt_ordinal_score_predict_combine";
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    hipStream_t st = h->stream;
    std::vector<uint64_t> one;
    uint64_t* pooled = static_cast<uint64_t*>(h_out);
    OspredLayout L{};
    int64_t hdr0[OSCORE_HEADER_WORDS];
    for (int c = 0; c < chains; ++c) {
        int64_t hdr[OSCORE_HEADER_WORDS];
        GP_TRY(oscore_read_header(st, d_states[c], OSPRED_TAG, hdr, me, c));
        if (c == 0) {
            memcpy(hdr0, hdr, sizeof(hdr));
            L = ospred_layout(hdr[2], hdr[3], (int)hdr[4]);
            if (bytes != 8 * L.words) { set_error("%s: the pooled block holds %lld bytes, %lld were given", me, (long long)(8 * L.words), (long long)bytes); return GPIRT_E_ARG; }
            one.resize((size_t)L.words);
        } else if (hdr[2] != hdr0[2] || hdr[3] != hdr0[3] || hdr[4] != hdr0[4]) {
            set_error("%s: state %d has another n_new, m or C than state 0", me, c);
            return GPIRT_E_ARG;
        }
        uint64_t* dst = c == 0 ? pooled : one.data();
        GP_HIP(hipMemcpyAsync(dst, d_states[c], sizeof(uint64_t) * (size_t)L.words, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        if (c == 0) continue;
        if (!std::equal(one.begin() + L.mask, one.begin() + L.prob_sum, pooled + L.mask)) {
            set_error("%s: state %d was built on another cat_new than state 0", me, c);
            return GPIRT_E_ARG;
        }
        int64_t* pi = reinterpret_cast<int64_t*>(pooled);
        const int64_t* oi = reinterpret_cast<const int64_t*>(one.data());
        pi[6] += oi[6];
        pi[7] += oi[7];
        double* pd = reinterpret_cast<double*>(pooled);
        const double* od = reinterpret_cast<const double*>(one.data());
        for (int64_t g = L.prob_sum; g < L.words; ++g) pd[g] += od[g];        // prob_sum and info_sum lie side by side
    }
    return 0;
}

}  // namespace gpirt
