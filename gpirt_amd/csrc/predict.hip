// predict.hip -- the unseen answers of respondents who were not in the fit, and the item to ask them next (include/gpirt_hip.h,
// "predicting new respondents' unseen answers").  An add-on to a score state (score.hip): the scorer's
// WEIGHTS instantiation leaves this draw's normalised grid weights in W (Np x n_new, k fastest, the padding rows zero) and the
// go-flag "no NaN in this draw's f*"; from there on three launches per draw, all of which do nothing in a skipped draw:
//   pred_operands_kernel   B = [P | H] (Np x 2m) from the cleaned f*: plogis and its binary entropy, one cell a thread
//   launch_gemm            C (n_new x 2m) = W^T B on the fp64 matrix cores, conditional on the go-flag (so never split-K: one
//                          kernel, a fixed order).  K runs over all Np rows: the padding rows of BOTH operands are zero and add
//                          exact zeros, and a K range that is a multiple of the K-step lets interior tiles take the
//                          branch-free main loop
//   pred_epilogue_kernel   q = C[:, j], Hbar = C[:, m + j], g = h(q) - Hbar; pred_sum += q, info_sum += g.  Every thread owns
//                          its cells (r fastest: coalesced in C and in both sums), no atomics; one lane keeps the two counters
//                          in the block's header.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace gpirt {

namespace {

constexpr int NG = GPIRT_NGRID;
constexpr int64_t NP = (NG + 127) / 128 * 128;       // 1024

struct PredLayout { int64_t mask, pred_sum, info_sum, words; };
PredLayout pred_layout(int64_t n, int64_t m)
{
    PredLayout L;
    L.mask = PRED_HEADER_WORDS;
    L.pred_sum = L.mask + (n * m + 63) / 64;
    L.info_sum = L.pred_sum + n * m;
    L.words = L.info_sum + n * m;
    return L;
}

// B[k + j ldb] = P, B[k + (m + j) ldb] = H for k < N; rows N .. ldb - 1 are never written (zero since the allocation)
__global__ __launch_bounds__(256) void pred_operands_kernel(const double* __restrict__ fclean, int64_t N, int64_t m,
                                                            double* __restrict__ B, int64_t ldb, const int* __restrict__ go)
{
    if (*go == 0) return;
    const int64_t total = N * m;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t j = g / N, k = g - j * N;
        const double f = fclean[g];
        const double a = fabs(f);
        const double e = exp(-a);
        const double l = log1p(e);
        const double s = e / (1.0 + e);
        B[k + j * ldb] = f >= 0.0 ? 1.0 / (1.0 + e) : s;
        B[k + (m + j) * ldb] = e == 0.0 ? 0.0 : l + a * s;
    }
}

__device__ __forceinline__ double binary_entropy(double q)
{
    q = fmin(fmax(q, 0.0), 1.0);
    const double a = q > 0.0 ? q * log(q) : 0.0;
    const double b = q < 1.0 ? (1.0 - q) * log1p(-q) : 0.0;
    return -(a + b);
}

__global__ __launch_bounds__(256) void pred_epilogue_kernel(const double* __restrict__ C, int64_t n, int64_t m,
                                                            double* __restrict__ pred_sum, double* __restrict__ info_sum,
                                                            int64_t* __restrict__ counters, const int* __restrict__ go)
{
    const bool run = *go != 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[run ? 0 : 1] += 1;         // pred_draws / pred_skipped
    if (!run) return;
    const int64_t total = n * m;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const double q = C[g], hbar = C[g + total];
        pred_sum[g] += q;
        info_sum[g] += binary_entropy(q) - hbar;
    }
}

struct HostPred {
    int64_t n = 0, m = 0;
    PredLayout L{};
    std::vector<uint64_t> words;
    int64_t* i64(int64_t at) { return reinterpret_cast<int64_t*>(words.data() + at); }
    double* f64(int64_t at) { return reinterpret_cast<double*>(words.data() + at); }
};

int pred_read(hipStream_t st, const void* d_block, HostPred& r, const char* who, int c)
{
    int64_t hdr[PRED_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_block, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] < 1 || hdr[0] > GPIRT_SCORE_MAX_N || hdr[1] < 1 || hdr[2] != PRED_LAYOUT_VERSION || hdr[3] != NG || hdr[4] < 0 ||
        hdr[5] < 0 || hdr[6] != 0 || hdr[7] != PRED_TAG) {
        set_error("%s: state %d is not a predict state block of layout %d", who, c, PRED_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[0]; r.m = hdr[1];
    r.L = pred_layout(r.n, r.m);
    r.words.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.words.data(), d_block, sizeof(uint64_t) * (size_t)r.L.words, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

// sum / pred_draws (NaN everywhere without a draw)
void pred_mean(const double* sum, int64_t count, int64_t draws, double* out)
{
    const double S = (double)draws;
    for (int64_t g = 0; g < count; ++g) out[g] = draws > 0 ? sum[g] / S : (double)NAN;
}

void pred_fill(HostPred& r, gpirt_score_predict* out)
{
    const int64_t n = r.n, m = r.m, draws = r.i64(4)[0];
    const int top = out->top;
    out->n_new = n; out->m = m; out->pred_draws = draws; out->pred_skipped = r.i64(5)[0];
    if (out->pred_sum) memcpy(out->pred_sum, r.f64(r.L.pred_sum), sizeof(double) * (size_t)(n * m));
    if (out->info_sum) memcpy(out->info_sum, r.f64(r.L.info_sum), sizeof(double) * (size_t)(n * m));
    if (out->p_yes) pred_mean(r.f64(r.L.pred_sum), n * m, draws, out->p_yes);
    std::vector<double> info_own;
    double* info = out->info;
    if (!info) { info_own.resize((size_t)(n * m)); info = info_own.data(); }
    pred_mean(r.f64(r.L.info_sum), n * m, draws, info);
    if (!out->next_items && !out->next_info) return;
    // the unanswered items of r by decreasing info, ties to the lowest j: top passes of a strict ">" scan in j order
    const uint64_t* mask = r.words.data() + r.L.mask;
    std::vector<char> taken((size_t)m);
    for (int64_t i = 0; i < n; ++i) {
        std::fill(taken.begin(), taken.end(), 0);
        for (int t = 0; t < top; ++t) {
            int64_t best = -1;
            for (int64_t j = 0; j < m; ++j) {
                const int64_t g = i + j * n;
                if (taken[(size_t)j] || ((mask[g >> 6] >> (g & 63)) & 1) || info[g] != info[g]) continue;
                if (best < 0 || info[g] > info[i + best * n]) best = j;
            }
            if (best >= 0) taken[(size_t)best] = 1;
            if (out->next_items) out->next_items[i + (int64_t)t * n] = best;
            if (out->next_info) out->next_info[i + (int64_t)t * n] = best >= 0 ? info[i + best * n] : (double)NAN;
        }
    }
}

}  // namespace

int64_t pred_state_words(int64_t n_new, int64_t m) { return pred_layout(n_new, m).words; }

void pred_free(PredState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = PredState{};
}

int pred_alloc(hipStream_t st, ScoreState* s)
{
    PredState* p = &s->pred;
    const int64_t n = s->n, m = s->m;
    const PredLayout L = pred_layout(n, m);
    p->n = n; p->m = m;
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->W, sizeof(double) * (size_t)(NP * n)));                // the padding rows stay zero
    GP_TRY(get((void**)&p->B, sizeof(double) * (size_t)(NP * 2 * m)));            // ... and these
    GP_TRY(get((void**)&p->C, sizeof(double) * (size_t)(n * 2 * m)));
    GP_TRY(get((void**)&p->go, sizeof(int) * 4));
    std::vector<uint64_t> head((size_t)L.pred_sum, 0);
    int64_t* hi = reinterpret_cast<int64_t*>(head.data());
    hi[0] = n; hi[1] = m; hi[2] = PRED_LAYOUT_VERSION; hi[3] = NG; hi[7] = PRED_TAG;
    std::copy(s->answered.begin(), s->answered.end(), head.begin() + L.mask);
    GP_HIP(hipMemcpyAsync(p->block, head.data(), sizeof(uint64_t) * head.size(), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // head is this call's
    p->on = true;
    return 0;
}

int launch_pred_accumulate(gpirt_handle_t h, hipStream_t st, ScoreState* s)
{
    PredState* p = &s->pred;
    const int64_t N = NG, n = p->n, m = p->m;
    const PredLayout L = pred_layout(n, m);
    int64_t blocks = (N * m + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pred_operands_kernel, dim3((unsigned)blocks), dim3(256), 0, st, s->fclean, N, m, p->B, NP, p->go);
    GP_HIP(hipGetLastError());
    GP_TRY(launch_gemm(h, st, true, false, TRI_NONE, n, 2 * m, NP, 1.0, p->W, NP, p->B, NP, 0.0, p->C, n, 0, p->go));
    blocks = (n * m + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pred_epilogue_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p->C, n, m,
                       reinterpret_cast<double*>(p->block + L.pred_sum), reinterpret_cast<double*>(p->block + L.info_sum),
                       reinterpret_cast<int64_t*>(p->block + 4), p->go);
    GP_HIP(hipGetLastError());
    return 0;
}

int pred_get(hipStream_t st, ScoreState* s, const char* name, void* h_out, int64_t bytes)
{
    PredState* p = &s->pred;
    const int64_t n = p->n, m = p->m;
    const PredLayout L = pred_layout(n, m);
    const char* blk = reinterpret_cast<const char*>(p->block);
    if (strcmp(name, "weights") == 0) {                   // W of the last counted draw: N x n_new out of the Np x n_new buffer
        GP_ARG(bytes == 8 * n * NG);
        GP_HIP(hipMemcpy2DAsync(h_out, 8 * (size_t)NG, p->W, 8 * (size_t)NP, 8 * (size_t)NG, (size_t)n, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const bool counts = strcmp(name, "counts") == 0;
    const bool sum = strcmp(name, "pred_sum") == 0 || strcmp(name, "p_yes") == 0;
    const bool mean = strcmp(name, "p_yes") == 0 || strcmp(name, "info") == 0;
    if (!counts && !sum && strcmp(name, "info_sum") != 0 && strcmp(name, "info") != 0) {
        set_error("unknown predict field '%s'", name);
        return GPIRT_E_ARG;
    }
    GP_ARG(bytes == (counts ? 16 : 8 * n * m));
    int64_t cnt[2];
    GP_HIP(hipMemcpyAsync(cnt, blk + 8 * 4, sizeof(cnt), hipMemcpyDeviceToHost, st));
    if (!counts) GP_HIP(hipMemcpyAsync(h_out, blk + 8 * (sum ? L.pred_sum : L.info_sum), (size_t)bytes, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (counts) memcpy(h_out, cnt, sizeof(cnt));
    else if (mean) pred_mean(static_cast<const double*>(h_out), n * m, cnt[0], static_cast<double*>(h_out));
    return 0;
}

int pred_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_score_predict* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved0 == 0 && out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_PREDICT_MAX_TOP) {
        set_error("prediction: top = %d is outside 1..%d", out->top, GPIRT_PREDICT_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    HostPred pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostPred& r = c == 0 ? pooled : one;
        GP_TRY(pred_read(h->stream, d_states[c], r, "gpirt_score_predict_combine", c));
        if (c == 0) continue;
        if (r.n != pooled.n || r.m != pooled.m) {
            set_error("gpirt_score_predict_combine: state %d has another n_new or m than state 0", c);
            return GPIRT_E_ARG;
        }
        if (!std::equal(one.words.begin() + one.L.mask, one.words.begin() + one.L.pred_sum, pooled.words.begin() + pooled.L.mask)) {
            set_error("gpirt_score_predict_combine: state %d was built on another y_new than state 0", c);
            return GPIRT_E_ARG;
        }
        pooled.i64(4)[0] += one.i64(4)[0];
        pooled.i64(5)[0] += one.i64(5)[0];
        const int64_t cells = 2 * r.n * r.m;               // pred_sum and info_sum lie side by side
        for (int64_t g = 0; g < cells; ++g) pooled.f64(pooled.L.pred_sum)[g] += one.f64(one.L.pred_sum)[g];
    }
    pred_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
