// score.hip -- scoring respondents who were not in the fit, one f* draw at a time (include/gpirt_hip.h, "scoring new
// respondents").  For a new respondent r with answers y_new[r, :] and the grid theta*_k = -5 + 0.01 k,
//     T[k, r] = sum_j over observed cells of -log(1 + exp(-+ f*[k, j]))
// is exactly the product draw_theta forms for the respondents of the chain, so launch_score_accumulate CALLS that product
// (theta_fixed.hip: exact fixed point on the int8 matrix cores; gemm_f64.hip: the fp64 GEMM, behind the fixed-point form's
// own hand-over flag or instead of it with GPIRT_THETA_FIXED=2) on the state's own packed y_new, and score_accumulate_kernel
// turns every column of T into a normalised grid posterior and a log marginal likelihood and accumulates them.
//
// The product is a GEMM with a 0/1 operand: 0 * NaN = NaN would spread ONE non-finite f* cell over every respondent, whether
// they answered that item or not.  The contract skips a draw only for the respondents who did, so score_clean_kernel copies
// f* with NaN replaced by 0 and marks the item; score_flag_kernel, which does nothing unless a cell was marked, flags the
// respondents who answered a marked item (for them lp[k] IS NaN at that k).  +-inf and |f*| > 709 are left as they are: the
// product holds the overflowed term at -1e300 (stages.hip loglik_terms_kernel), which is finite.
//
// score_accumulate_kernel: one wave per respondent, four respondents per 256-lane work-group, lanes stride k (k = lane +
// 64 i, i < 16 covers the 1001 points), so the reads of the N x n_new product and the read-modify-write of post_sum[r][.]
// are coalesced along k.  The 16 values of a lane stay in registers (fully unrolled: no scratch, no LDS).  Max and sum go
// through a lane-local loop in k order and the xor butterfly, whose partners add the same two numbers in either order: every
// lane holds the same bits, and neither the grid size nor the other waves enter.  The non-finite decision (a wave vote) is
// made before any accumulator of the respondent is written; lane 0 keeps the respondent's scalars.  No atomics.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace gpirt {

namespace {

constexpr int NG = GPIRT_NGRID;
constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_PER_LANE = (NG + 63) / 64;          // 16
static_assert(SC_PER_LANE * 64 >= NG, "a wave covers the grid");

struct ScoreLayout { int64_t draws, nonfinite, n_obs, lpd_acc, ll_sum, post_sum, words; };
ScoreLayout score_layout(int64_t n)
{
    ScoreLayout L;
    L.draws = SCORE_HEADER_WORDS; L.nonfinite = L.draws + n; L.n_obs = L.nonfinite + n;
    L.lpd_acc = L.n_obs + n; L.ll_sum = L.lpd_acc + n; L.post_sum = L.ll_sum + n;
    L.words = L.post_sum + n * NG;
    return L;
}

// flags: [0] any NaN in this draw's f*, [1 .. m] the item holds one, then bad[n_new]: the respondent answered such an item
__global__ __launch_bounds__(256) void score_clean_kernel(const double* __restrict__ fstar, int64_t N, int64_t m,
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

__global__ __launch_bounds__(256) void score_flag_kernel(const double* __restrict__ Ypm, int64_t n, int64_t m,
                                                         int* __restrict__ flags)
{
    if (flags[0] == 0) return;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t total = n * m;
    int bad = 0;
    for (int64_t j = 0; j < m; ++j)
        if (flags[1 + j] != 0 && (Ypm[r + j * n] != 0.0 || Ypm[r + j * n + total] != 0.0)) bad = 1;
    flags[1 + m + r] = bad;
}

struct ScoreArgs {
    const double* T;            // N x n_new, the product
    const double* logprior;     // N
    const int* bad;             // n_new
    double lse_prior;           // logsumexp_k(logprior)
    int64_t n;
    int64_t* draws; int64_t* nonfinite;
    double* lpd_acc; double* ll_sum; double* post_sum;
    // WEIGHTS instantiation only (predict.hip): this draw's w_k to W[r ldw + k], and go = "no NaN in this draw's f*"
    double* W; int64_t ldw; const int* nan_flag; int* go;
};

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// WEIGHTS = false is the scorer as it always was; true also keeps what it used to throw away: the value added to post_sum
// goes to W as well (the same register, so the score block's bits do not depend on the flag), and one lane of the launch
// turns flags[0] into the go-flag of the prediction's conditional launches.
template <bool WEIGHTS>
__global__ __launch_bounds__(SC_THREADS) void score_accumulate_kernel(ScoreArgs a)
{
    const int lane = (int)(threadIdx.x & 63);
    const int64_t r = (int64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
    if (WEIGHTS && blockIdx.x == 0 && threadIdx.x == 0) *a.go = (*a.nan_flag == 0) ? 1 : 0;
    if (r >= a.n) return;                                // (a whole wave: nothing below waits for another wave)
    const double* __restrict__ T = a.T + r * NG;
    double* __restrict__ post = a.post_sum + r * NG;
    double lp[SC_PER_LANE];
    bool ok = a.bad[r] == 0;
#pragma unroll
    for (int i = 0; i < SC_PER_LANE; ++i) {
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
    for (int i = 1; i < SC_PER_LANE; ++i) M = fmax(M, lp[i]);
    M = wave_max(M);
    double Z = 0.0;
#pragma unroll
    for (int i = 0; i < SC_PER_LANE; ++i) {
        lp[i] = exp(lp[i] - M);                          // (beyond the grid: exp(-inf) = 0)
        Z += lp[i];
    }
    Z = wave_sum(Z);
#pragma unroll
    for (int i = 0; i < SC_PER_LANE; ++i) {
        const int k = lane + 64 * i;
        if (k < NG) {
            const double w = lp[i] / Z;
            post[k] += w;
            if (WEIGHTS) a.W[r * a.ldw + k] = w;
        }
    }
    if (lane == 0) {
        const double l = M + log(Z) - a.lse_prior;
        const double acc = a.lpd_acc[r];
        const double hi = fmax(acc, l), lo = fmin(acc, l);
        a.lpd_acc[r] = lo == -INFINITY ? hi : hi + log1p(exp(lo - hi));
        a.ll_sum[r] += l;
        a.draws[r] += 1;
    }
}

// log dnorm(theta*_k) as draw_theta adds it (stages.hip r_dnorm_log: no transcendental, so the host table is its bits)
void score_logprior(double* lp, double* lse)
{
    long double s = 0.0L;
    double mx = -INFINITY;
    const double ln_sqrt_2pi = 0.918938533204672741780329736406;          // stages.hip GP_LN_SQRT_2PI
    for (int k = 0; k < NG; ++k) {
        const double z = fabs(-5.0 + (double)k * 0.01);
        lp[k] = -(ln_sqrt_2pi + 0.5 * z * z);
        mx = std::max(mx, lp[k]);
    }
    for (int k = 0; k < NG; ++k) s += expl((long double)lp[k] - (long double)mx);
    *lse = (double)((long double)mx + logl(s));
}

// a state block on the host
struct HostScore {
    int64_t n = 0, m = 0;
    ScoreLayout L{};
    std::vector<uint64_t> words;
    int64_t* i64(int64_t at) { return reinterpret_cast<int64_t*>(words.data() + at); }
    double* f64(int64_t at) { return reinterpret_cast<double*>(words.data() + at); }
};

int score_read_header(hipStream_t st, const void* d_block, HostScore& r, const char* who, int c)
{
    int64_t hdr[SCORE_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_block, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] < 1 || hdr[0] > GPIRT_SCORE_MAX_N || hdr[1] < 1 || hdr[2] != SCORE_LAYOUT_VERSION || hdr[3] != NG ||
        hdr[4] != 0 || hdr[5] != 0 || hdr[6] != 0 || hdr[7] != 0) {
        set_error("%s: state %d is not a score state block of layout %d", who, c, SCORE_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[0]; r.m = hdr[1];
    r.L = score_layout(r.n);
    return 0;
}

int score_read(hipStream_t st, const void* d_block, HostScore& r, const char* who, int c)
{
    GP_TRY(score_read_header(st, d_block, r, who, c));
    r.words.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.words.data(), d_block, sizeof(uint64_t) * (size_t)r.L.words, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

double score_logaddexp(double a, double b)
{
    const double hi = std::max(a, b), lo = std::min(a, b);
    return lo == -INFINITY ? hi : hi + log1p(exp(lo - hi));
}

// the finished values of one respondent from its accumulators (the header's table); sums run in k order
struct ScoreRow { double mean, sd, map, lpd, ll; };
ScoreRow score_finish(const double* post, int64_t draws, double lpd_acc, double ll_sum, double* grid /* NG, may be null */,
                      const double* probs, int nprobs, double* q_out, int64_t q_stride)
{
    ScoreRow o{ (double)NAN, (double)NAN, (double)NAN, (double)NAN, (double)NAN };
    if (draws < 1) {
        if (grid) for (int k = 0; k < NG; ++k) grid[k] = (double)NAN;
        for (int p = 0; p < nprobs; ++p) q_out[(int64_t)p * q_stride] = (double)NAN;
        return o;
    }
    const double S = (double)draws;
    double mean = 0.0, best = -1.0;
    int kbest = 0;
    for (int k = 0; k < NG; ++k) {
        const double g = post[k] / S;
        if (grid) grid[k] = g;
        mean += (-5.0 + (double)k * 0.01) * g;
        if (g > best) { best = g; kbest = k; }
    }
    double var = 0.0;
    for (int k = 0; k < NG; ++k) {
        const double d = (-5.0 + (double)k * 0.01) - mean;
        var += d * d * (post[k] / S);
    }
    for (int p = 0; p < nprobs; ++p) {
        double cum = 0.0;
        int k = 0;
        for (; k < NG - 1; ++k) { cum += post[k] / S; if (cum >= probs[p]) break; }
        q_out[(int64_t)p * q_stride] = -5.0 + (double)k * 0.01;
    }
    o.mean = mean; o.sd = sqrt(var); o.map = -5.0 + (double)kbest * 0.01;
    o.lpd = lpd_acc - log(S); o.ll = ll_sum / S;
    return o;
}

void score_fill(HostScore& r, gpirt_score* out)
{
    const int64_t n = r.n;
    const int64_t* draws = r.i64(r.L.draws);
    out->n_new = n; out->m = r.m;
    std::vector<double> lpd((size_t)n), qtmp((size_t)std::max(out->nprobs, 1));
    for (int64_t i = 0; i < n; ++i) {
        const ScoreRow o = score_finish(r.f64(r.L.post_sum) + i * NG, draws[i], r.f64(r.L.lpd_acc)[i], r.f64(r.L.ll_sum)[i],
                                        out->grid_post ? out->grid_post + i * NG : nullptr, out->probs, out->nprobs,
                                        out->theta_quantiles ? out->theta_quantiles + i : qtmp.data(),
                                        out->theta_quantiles ? n : 1);
        lpd[(size_t)i] = o.lpd;
        if (out->theta_mean) out->theta_mean[i] = o.mean;
        if (out->theta_sd) out->theta_sd[i] = o.sd;
        if (out->theta_map) out->theta_map[i] = o.map;
        if (out->lpd) out->lpd[i] = o.lpd;
        if (out->loglik_mean) out->loglik_mean[i] = o.ll;
    }
    if (out->draws) memcpy(out->draws, draws, sizeof(int64_t) * (size_t)n);
    if (out->nonfinite) memcpy(out->nonfinite, r.i64(r.L.nonfinite), sizeof(int64_t) * (size_t)n);
    if (out->n_obs) memcpy(out->n_obs, r.i64(r.L.n_obs), sizeof(int64_t) * (size_t)n);
    if (out->lpd_acc) memcpy(out->lpd_acc, r.f64(r.L.lpd_acc), sizeof(double) * (size_t)n);
    if (out->ll_sum) memcpy(out->ll_sum, r.f64(r.L.ll_sum), sizeof(double) * (size_t)n);
    if (out->post_sum) memcpy(out->post_sum, r.f64(r.L.post_sum), sizeof(double) * (size_t)(n * NG));
    // sum_r lpd and sqrt(n_new var_r lpd) (ddof 1), in respondent order; NaN as soon as one respondent has no draw
    double tot = 0.0;
    for (int64_t i = 0; i < n; ++i) tot += lpd[(size_t)i];
    double ss = 0.0;
    const double mean = tot / (double)n;
    for (int64_t i = 0; i < n; ++i) ss += (lpd[(size_t)i] - mean) * (lpd[(size_t)i] - mean);
    out->lpd_total = tot;
    out->se_lpd_total = n >= 2 ? sqrt((double)n * (ss / (double)(n - 1))) : (double)NAN;
}

}  // namespace

int64_t score_state_words(const ScoreState* s) { return score_layout(s->n).words; }

int score_alloc(hipStream_t st, ScoreState* s, const double* h_y_new, int64_t n_new, int64_t m)
{
    // every refusal before anything is touched
    if (!h_y_new || n_new < 1 || n_new > GPIRT_SCORE_MAX_N) {
        set_error("scoring: n_new = %lld is outside 1..%d", (long long)n_new, GPIRT_SCORE_MAX_N);
        return GPIRT_E_ARG;
    }
    for (int64_t g = 0; g < n_new * m; ++g) {
        const double v = h_y_new[g];
        if (!(v == 1.0 || v == -1.0 || v != v)) { set_error("scoring: y_new must be +1, -1 or NaN (a missing response)"); return GPIRT_E_ARG; }
    }
    const int64_t N = NG, Np = (N + 127) / 128 * 128;
    s->n = n_new; s->m = m; s->tfd = tf_dims(n_new, m, N);
    const ScoreLayout L = score_layout(n_new);
    auto get = [&](void** p, size_t bytes, bool zero) -> int {
        GP_HIP(hipMalloc(p, bytes));
        s->allocs.push_back(*p);
        if (zero) GP_HIP(hipMemsetAsync(*p, 0, bytes, st));
        return 0;
    };
    double* d_y = nullptr;
    GP_TRY(get((void**)&s->block, sizeof(uint64_t) * (size_t)L.words, true));
    GP_TRY(get((void**)&s->Ypm, sizeof(double) * (size_t)(n_new * 2 * m), false));
    GP_TRY(get((void**)&s->Gpm, sizeof(double) * (size_t)(Np * 2 * m + 2), true));       // the padding rows stay zero
    GP_TRY(get((void**)&s->y8, tf_y8_bytes(s->tfd) + 16, false));
    GP_TRY(get((void**)&s->gq, tf_gq_bytes(s->tfd) + 16, false));
    GP_TRY(get((void**)&s->aux, tf_aux_bytes(s->tfd) + 16, true));
    GP_TRY(get((void**)&s->T, sizeof(double) * (size_t)(N * n_new + 2), true));
    GP_TRY(get((void**)&s->fclean, sizeof(double) * (size_t)(N * m + 2), true));
    GP_TRY(get((void**)&s->flags, sizeof(int) * (size_t)(1 + m + n_new), true));
    GP_TRY(get((void**)&s->logprior, sizeof(double) * (size_t)N, false));
    GP_TRY(get((void**)&d_y, sizeof(double) * (size_t)(n_new * m), false));
    // the header, the observed cells and lpd_acc = -inf in front of the zeroed sums
    std::vector<uint64_t> head((size_t)L.post_sum, 0);
    int64_t* hi = reinterpret_cast<int64_t*>(head.data());
    double* hd = reinterpret_cast<double*>(head.data());
    hi[0] = n_new; hi[1] = m; hi[2] = SCORE_LAYOUT_VERSION; hi[3] = N;
    for (int64_t r = 0; r < n_new; ++r) {
        int64_t c = 0;
        for (int64_t j = 0; j < m; ++j) c += h_y_new[r + j * n_new] == h_y_new[r + j * n_new];
        hi[L.n_obs + r] = c;
        hd[L.lpd_acc + r] = -INFINITY;
    }
    s->answered.assign((size_t)((n_new * m + 63) / 64), 0);                  // (host only: what a predict state block carries)
    for (int64_t g = 0; g < n_new * m; ++g)
        if (h_y_new[g] == h_y_new[g]) s->answered[(size_t)(g >> 6)] |= (uint64_t)1 << (g & 63);
    double lp[NG];
    score_logprior(lp, &s->lse_prior);
    GP_HIP(hipMemcpyAsync(s->block, head.data(), sizeof(uint64_t) * head.size(), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(s->logprior, lp, sizeof(lp), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(d_y, h_y_new, sizeof(double) * (size_t)(n_new * m), hipMemcpyHostToDevice, st));
    GP_TRY(launch_indicators(st, d_y, n_new, m, s->Ypm));
    GP_TRY(launch_tf_indicators(st, d_y, n_new, n_new, m, s->tfd, s->y8));
    GP_HIP(hipStreamSynchronize(st));        // head, lp are this call's; d_y is not needed again
    GP_HIP(hipFree(d_y));
    s->allocs.pop_back();
    s->on = true;
    return 0;
}

void score_free(ScoreState* s)
{
    pred_free(&s->pred);
    for (void* p : s->allocs) hipFree(p);
    *s = ScoreState{};
}

int launch_score_accumulate(gpirt_handle_t h, hipStream_t st, ScoreState* s, const double* fstar)
{
    const int64_t N = NG, n = s->n, m = s->m, Np = (N + 127) / 128 * 128;
    GP_HIP(hipMemsetAsync(s->flags, 0, sizeof(int) * (size_t)(1 + m + n), st));
    int64_t blocks = (N * m + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(score_clean_kernel, dim3((unsigned)blocks), dim3(256), 0, st, fstar, N, m, s->fclean, s->flags);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(score_flag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->Ypm, n, m, s->flags);
    GP_HIP(hipGetLastError());
    // the product, as do_theta_partial launches it (sampler.hip), on the state's own buffers
    const int* only_if = nullptr;
    if (h->cfg.theta_fixed == 1) {
        GP_TRY(launch_theta_fixed(st, s->fclean, N, n, m, s->tfd, s->y8, s->gq, s->aux, s->T, N, false, nullptr));
        only_if = tf_overflow(s->aux, s->tfd);
    }
    GP_TRY(launch_loglik_terms(st, s->fclean, N, m, s->Gpm, Np, only_if));
    GP_TRY(launch_gemm(h, st, false, true, TRI_NONE, N, n, 2 * m, 1.0, s->Gpm, Np, s->Ypm, n, 0.0, s->T, N, Np, only_if));
    const ScoreLayout L = score_layout(n);
    ScoreArgs a{};
    a.T = s->T; a.logprior = s->logprior; a.bad = s->flags + 1 + m; a.lse_prior = s->lse_prior; a.n = n;
    a.draws = reinterpret_cast<int64_t*>(s->block + L.draws);
    a.nonfinite = reinterpret_cast<int64_t*>(s->block + L.nonfinite);
    a.lpd_acc = reinterpret_cast<double*>(s->block + L.lpd_acc);
    a.ll_sum = reinterpret_cast<double*>(s->block + L.ll_sum);
    a.post_sum = reinterpret_cast<double*>(s->block + L.post_sum);
    const dim3 grid((unsigned)((n + SC_WAVES - 1) / SC_WAVES));
    if (!s->pred.on) {
        hipLaunchKernelGGL(score_accumulate_kernel<false>, grid, dim3(SC_THREADS), 0, st, a);
        GP_HIP(hipGetLastError());
        return 0;
    }
    a.W = s->pred.W; a.ldw = Np; a.nan_flag = s->flags; a.go = s->pred.go;
    hipLaunchKernelGGL(score_accumulate_kernel<true>, grid, dim3(SC_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    return launch_pred_accumulate(h, st, s);
}

int score_get(hipStream_t st, ScoreState* s, const char* name, void* h_out, int64_t bytes)
{
    const int64_t n = s->n;
    const ScoreLayout L = score_layout(n);
    const char* blk = reinterpret_cast<const char*>(s->block);
    auto fetch = [&](void* dst, const void* src, int64_t nbytes) -> int {
        GP_HIP(hipMemcpyAsync(dst, src, (size_t)nbytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "product") == 0) {                  // T of the last accumulate call (N x n_new, k fastest)
        GP_ARG(bytes == 8 * n * NG);
        return fetch(h_out, s->T, bytes);
    }
    const struct { const char* name; int64_t word, bytes; } raw[] = {
        { "draws", L.draws, 8 * n }, { "nonfinite", L.nonfinite, 8 * n }, { "n_obs", L.n_obs, 8 * n },
        { "lpd_acc", L.lpd_acc, 8 * n }, { "ll_sum", L.ll_sum, 8 * n }, { "post_sum", L.post_sum, 8 * n * NG },
    };
    for (const auto& e : raw)
        if (strcmp(e.name, name) == 0) {
            GP_ARG(bytes == e.bytes);
            return fetch(h_out, blk + 8 * e.word, e.bytes);
        }
    const bool grid = strcmp(name, "grid_post") == 0;
    static const char* const derived[] = { "theta_mean", "theta_sd", "theta_map", "lpd", "loglik_mean" };
    int which = -1;
    for (int d = 0; d < 5; ++d) if (strcmp(name, derived[d]) == 0) which = d;
    if (!grid && which < 0) { set_error("unknown score field '%s'", name); return GPIRT_E_ARG; }
    GP_ARG(bytes == (grid ? 8 * n * NG : 8 * n));
    HostScore r;
    GP_TRY(score_read(st, s->block, r, "gpirt_sampler_score_get", 0));
    double* out = static_cast<double*>(h_out);
    for (int64_t i = 0; i < n; ++i) {
        const ScoreRow o = score_finish(r.f64(r.L.post_sum) + i * NG, r.i64(r.L.draws)[i], r.f64(r.L.lpd_acc)[i],
                                        r.f64(r.L.ll_sum)[i], grid ? out + i * NG : nullptr, nullptr, 0, nullptr, 0);
        if (!grid) out[i] = which == 0 ? o.mean : which == 1 ? o.sd : which == 2 ? o.map : which == 3 ? o.lpd : o.ll;
    }
    return 0;
}

int score_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_score* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved0 == 0 && out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    GP_ARG(out->nprobs >= 0 && (out->nprobs == 0 || out->probs));
    for (int p = 0; p < out->nprobs; ++p) GP_ARG(out->probs[p] >= 0.0 && out->probs[p] <= 1.0);
    for (int c = 0; c < chains; ++c) {
        GP_ARG(d_states[c]);
        if (signs) GP_ARG(signs[c] == 1 || signs[c] == -1);
    }
    HostScore pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostScore& r = c == 0 ? pooled : one;
        GP_TRY(score_read(h->stream, d_states[c], r, "gpirt_score_combine", c));
        if (c > 0 && (r.n != pooled.n || r.m != pooled.m)) {
            set_error("gpirt_score_combine: state %d has another n_new or m than state 0", c);
            return GPIRT_E_ARG;
        }
        const int64_t n = r.n;
        if (signs && signs[c] < 0)                       // theta -> -theta: post_sum[r][k] <-> post_sum[r][1000 - k]
            for (int64_t i = 0; i < n; ++i) std::reverse(r.f64(r.L.post_sum) + i * NG, r.f64(r.L.post_sum) + (i + 1) * NG);
        if (c == 0) continue;
        for (int64_t i = 0; i < n; ++i) {
            pooled.i64(pooled.L.draws)[i] += one.i64(one.L.draws)[i];
            pooled.i64(pooled.L.nonfinite)[i] += one.i64(one.L.nonfinite)[i];
            pooled.f64(pooled.L.ll_sum)[i] += one.f64(one.L.ll_sum)[i];
            pooled.f64(pooled.L.lpd_acc)[i] = score_logaddexp(pooled.f64(pooled.L.lpd_acc)[i], one.f64(one.L.lpd_acc)[i]);
            if (one.i64(one.L.n_obs)[i] != pooled.i64(pooled.L.n_obs)[i]) {
                set_error("gpirt_score_combine: state %d was built on another y_new than state 0", c);
                return GPIRT_E_ARG;
            }
        }
        for (int64_t k = 0; k < n * NG; ++k) pooled.f64(pooled.L.post_sum)[k] += one.f64(one.L.post_sum)[k];
    }
    score_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
