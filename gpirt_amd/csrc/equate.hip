// equate.hip -- two forms at once (include/gpirt_hip.h, "Two-form score equating"): per draw the joint
// distribution J[s, t] = sum_k w_k P(S_X = s | theta_k) P(S_Y = t | theta_k) of the sum scores on two disjoint forms X and Y for
// the N(0, 1) population, from it the two score distributions, the equipercentile equivalents of each form's scores on the other
// form's scale and the correlation of the two scores -- accumulated one draw at a time without stored draws.
//
// The recursion is sumscore.hip's, run once per form through its launchers (no second recursion lives here):
//   launch_sumscore_table   x 2: (p, q) of each form's columns; a NaN in a column of EITHER form raises the one skip word, and both
//                           tables are done before any row kernel reads it
//   launch_sumscore_rows    x 2: A_X with its weighted copy w_k A_X (the row kernel's `joint` output on a buffer zeroed for the
//                           draw: 0 + w_k A is w_k A rounded once) and T_X, V_X; A_Y, T_Y, V_Y (no weighted copy)
//   launch_sumscore_pi      x 2: pi_X and pi_Y in sumscore_pi_kernel's order, straight into last_pix / pix_sum / pix_sumsq
//   equate_fin_kernel       one work-group: the five sums of the correlation in ascending k, the two CDFs (one lane each, in LDS),
//                           then one lane per score searches the other form's CDF; the counters; the go-flag of the product
//   launch_gemm             last_joint ((M_Y + 1) x (M_X + 1), t fastest) = A_Y^T-image times the weighted A_X image over k, ONE
//                           conditional product on the fp64 matrix cores (run_if: never split-K, a fixed order).  K = 1024: rows
//                           1001 .. 1023 of both operands are zero since the allocation and add exact zeros
//   equate_add_kernel       joint_sum += last_joint, one owner per cell
// Every kernel reads the skip word before it touches anything: a skipped draw changes the counter `skipped` alone.  No atomics.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace gpirt {

namespace {

constexpr int EQ_N = GPIRT_NGRID;                 // 1001 grid points
constexpr int EQ_NP = 1024;                       // ... padded to the product's K step
constexpr int EQ_FIN_THREADS = 256;
constexpr int EQ_MAXS = GPIRT_EQUATE_MAX_ITEMS + 1;   // scores of one form
static_assert(5 * EQ_NP >= 2 * EQ_MAXS, "the finishing kernel's LDS holds five grid vectors, then two CDFs");
static_assert(EQ_NP % 128 == 0 && EQ_NP >= EQ_N, "K is a whole number of the product's K steps");

const char* const kEquateRaw[GPIRT_EQUATE_NARRAYS] = { "joint_sum", "pix_sum", "pix_sumsq", "piy_sum", "piy_sumsq", "eyx_sum", "eyx_sumsq",
                                                       "exy_sum", "exy_sumsq", "corr", "corr_terms", "mask_x", "mask_y", "w",
                                                       "last_joint", "last_pix", "last_piy", "last_eyx", "last_exy" };

inline int64_t eq_raw_bytes(int k, int64_t m, int64_t Mx, int64_t My)
{
    switch (k) {
        case GPIRT_EQUATE_JOINT_SUM: case GPIRT_EQUATE_LAST_JOINT: return 8 * (Mx + 1) * (My + 1);
        case GPIRT_EQUATE_PIX_SUM: case GPIRT_EQUATE_PIX_SUMSQ: case GPIRT_EQUATE_LAST_PIX: case GPIRT_EQUATE_EYX_SUM:
        case GPIRT_EQUATE_EYX_SUMSQ: case GPIRT_EQUATE_LAST_EYX: return 8 * (Mx + 1);
        case GPIRT_EQUATE_PIY_SUM: case GPIRT_EQUATE_PIY_SUMSQ: case GPIRT_EQUATE_LAST_PIY: case GPIRT_EQUATE_EXY_SUM:
        case GPIRT_EQUATE_EXY_SUMSQ: case GPIRT_EQUATE_LAST_EXY: return 8 * (My + 1);
        case GPIRT_EQUATE_CORR: return 16;
        case GPIRT_EQUATE_CORR_TERMS: return 40;
        case GPIRT_EQUATE_W: return 8 * (int64_t)EQ_N;
        default: return m;                        // the two masks: a byte per item
    }
}

// e[s] for every score s of form A on form B's scale (include/gpirt_hip.h): P = F_A[s - 1] + pi_A[s] / 2, t* the smallest t with
// F_B[t] > P, e = t* - 0.5 + (P - F_B[t* - 1]) / pi_B[t*]; no such t: M_B + 0.5 and one more clamped cell.  F_A, F_B in LDS.
__device__ __forceinline__ int equate_search(const double* FA, const double* __restrict__ piA, int MA, const double* FB,
                                             const double* __restrict__ piB, int MB, double* __restrict__ last, double* __restrict__ sum,
                                             double* __restrict__ sumsq)
{
    int clamped = 0;
    for (int s = threadIdx.x; s <= MA; s += EQ_FIN_THREADS) {
        const double P = (s > 0 ? FA[s - 1] : 0.0) + piA[s] / 2.0;
        int lo = 0, hi = MB + 1;                                  // the answer lies in [lo, hi]; hi = MB + 1: none
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (FB[mid] > P) hi = mid; else lo = mid + 1;
        }
        double e;
        if (lo > MB) {
            e = (double)MB + 0.5;
            ++clamped;
        } else {
            e = ((double)lo - 0.5) + (P - (lo > 0 ? FB[lo - 1] : 0.0)) / piB[lo];
        }
        last[s] = e;
        sum[s] += e;
        sumsq[s] += e * e;
    }
    return clamped;
}

__global__ __launch_bounds__(EQ_FIN_THREADS) void equate_fin_kernel(
    const double* __restrict__ pix, const double* __restrict__ piy, int Mx, int My, const double* __restrict__ TX,
    const double* __restrict__ VX, const double* __restrict__ TY, const double* __restrict__ VY, const double* __restrict__ w,
    int* __restrict__ ctl, double* __restrict__ eyx_sum, double* __restrict__ eyx_sumsq, double* __restrict__ exy_sum,
    double* __restrict__ exy_sumsq, double* __restrict__ last_eyx, double* __restrict__ last_exy, double* __restrict__ corr,
    double* __restrict__ corr_terms, int64_t* __restrict__ hdr)
{
    __shared__ double sh[5 * EQ_NP];
    __shared__ int cnt[EQ_FIN_THREADS];
    const int t = threadIdx.x;
    if (ctl[0]) {
        if (t == 0) { hdr[7] += 1; ctl[1] = 0; }                  // skipped; the product does not run
        return;
    }
    // the correlation's five sums, ascending k
    for (int k = t; k < EQ_N; k += EQ_FIN_THREADS) {
        const double tx = TX[k], vx = VX[k], ty = TY[k], vy = VY[k], wk = w[k];
        sh[k] = wk * tx;
        sh[EQ_NP + k] = wk * (vx + tx * tx);
        sh[2 * EQ_NP + k] = wk * ty;
        sh[3 * EQ_NP + k] = wk * (vy + ty * ty);
        sh[4 * EQ_NP + k] = wk * (tx * ty);
    }
    __syncthreads();
    if (t == 0) {
        double ax = 0.0, bx = 0.0, ay = 0.0, by = 0.0, c = 0.0;
        for (int k = 0; k < EQ_N; ++k) {
            ax += sh[k]; bx += sh[EQ_NP + k]; ay += sh[2 * EQ_NP + k]; by += sh[3 * EQ_NP + k]; c += sh[4 * EQ_NP + k];
        }
        corr_terms[0] = ax; corr_terms[1] = bx; corr_terms[2] = ay; corr_terms[3] = by; corr_terms[4] = c;
        hdr[6] += 1;                                              // draws
        ctl[1] = 1;                                               // the product runs
        const double vx = bx - ax * ax, vy = by - ay * ay;
        if (vx > 0.0 && vy > 0.0) {
            const double r = (c - ax * ay) / sqrt(vx * vy);
            corr[0] += r;
            corr[1] += r * r;
            hdr[8] += 1;                                          // corr_draws
        } else {
            hdr[9] += 1;                                          // corr_skipped
        }
    }
    __syncthreads();
    // the two CDFs in ascending score: one lane each, in place over the copies of pi
    double* FX = sh;
    double* FY = sh + EQ_MAXS;
    for (int s = t; s <= Mx; s += EQ_FIN_THREADS) FX[s] = pix[s];
    for (int s = t; s <= My; s += EQ_FIN_THREADS) FY[s] = piy[s];
    __syncthreads();
    if (t == 0 || t == 64) {
        double* F = t == 0 ? FX : FY;
        const int M = t == 0 ? Mx : My;
        double acc = 0.0;
        for (int s = 0; s <= M; ++s) { acc += F[s]; F[s] = acc; }
    }
    __syncthreads();
    int clamped = equate_search(FX, pix, Mx, FY, piy, My, last_eyx, eyx_sum, eyx_sumsq);
    clamped += equate_search(FY, piy, My, FX, pix, Mx, last_exy, exy_sum, exy_sumsq);
    cnt[t] = clamped;
    __syncthreads();
    if (t == 0) {
        int all = 0;
        for (int i = 0; i < EQ_FIN_THREADS; ++i) all += cnt[i];
        hdr[10] += all;                                           // eq_clamped
    }
}

__global__ __launch_bounds__(256) void equate_add_kernel(const double* __restrict__ last_joint, int64_t cells, const int* __restrict__ ctl,
                                                         double* __restrict__ joint_sum)
{
    if (ctl[0]) return;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < cells; g += (int64_t)gridDim.x * 256) joint_sum[g] += last_joint[g];
}

// a state block on the host
struct HostEquate {
    std::vector<uint64_t> w;
    int64_t m = 0, Mx = 0, My = 0;
    EquateLayout L{};
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    double* f64(int k) { return reinterpret_cast<double*>(w.data() + L.off[k]); }
    const unsigned char* bytes(int k) const { return reinterpret_cast<const unsigned char*>(w.data() + L.off[k]); }
};

int equate_read(hipStream_t st, const void* d_state, HostEquate& r, const char* who, int c)
{
    int64_t hdr[EQUATE_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    bool ok = hdr[0] == EQUATE_TAG && hdr[1] == EQUATE_LAYOUT_VERSION && hdr[2] > 0 && hdr[3] >= 1 && hdr[4] >= 1 &&
              hdr[3] <= GPIRT_EQUATE_MAX_ITEMS && hdr[4] <= GPIRT_EQUATE_MAX_ITEMS && hdr[3] + hdr[4] <= hdr[2] && hdr[5] == EQ_N;
    for (int q = 6; q <= 10; ++q) ok = ok && hdr[q] >= 0;
    if (!ok) {
        set_error("%s: state %d is not an equating state block of layout %d", who, c, EQUATE_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.m = hdr[2]; r.Mx = hdr[3]; r.My = hdr[4];
    r.L = equate_layout(r.m, r.Mx, r.My);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

void equate_fill(HostEquate& r, gpirt_equate* out)
{
    const int64_t* h = r.hdr();
    out->m = r.m; out->Mx = r.Mx; out->My = r.My;
    out->draws = h[6]; out->skipped = h[7]; out->corr_draws = h[8]; out->corr_skipped = h[9]; out->eq_clamped = h[10];
    for (int k = 0; k < GPIRT_EQUATE_NARRAYS; ++k)
        if (out->raw[k]) memcpy(out->raw[k], r.w.data() + r.L.off[k], (size_t)eq_raw_bytes(k, r.m, r.Mx, r.My));
}

}  // namespace

EquateLayout equate_layout(int64_t m, int64_t Mx, int64_t My)
{
    EquateLayout L{};
    int64_t at = EQUATE_HEADER_WORDS;
    for (int k = 0; k < GPIRT_EQUATE_NARRAYS; ++k) {
        L.off[k] = at;
        at += (eq_raw_bytes(k, m, Mx, My) + 15) / 16 * 2;             // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int equate_check(int64_t m, const unsigned char* mask_x, const unsigned char* mask_y, int64_t* Mx_out, int64_t* My_out)
{
    if (!mask_x || !mask_y) {
        set_error("score equating: both forms need a mask of m bytes");
        return GPIRT_E_ARG;
    }
    int64_t Mx = 0, My = 0;
    for (int64_t j = 0; j < m; ++j) {
        Mx += mask_x[j] ? 1 : 0;
        My += mask_y[j] ? 1 : 0;
        if (mask_x[j] && mask_y[j]) {
            set_error("score equating: the forms overlap (column %lld is in both); the scores factorise given theta only for "
                      "disjoint forms", (long long)j);
            return GPIRT_E_ARG;
        }
    }
    if (Mx < 1 || My < 1) {
        set_error("score equating: form %s is empty (no item of the %lld is in it)", Mx < 1 ? "x" : "y", (long long)m);
        return GPIRT_E_ARG;
    }
    if (Mx > GPIRT_EQUATE_MAX_ITEMS || My > GPIRT_EQUATE_MAX_ITEMS) {
        set_error("score equating: form %s has %lld items, at most %d are taken", Mx > GPIRT_EQUATE_MAX_ITEMS ? "x" : "y",
                  (long long)(Mx > GPIRT_EQUATE_MAX_ITEMS ? Mx : My), GPIRT_EQUATE_MAX_ITEMS);
        return GPIRT_E_ARG;
    }
    if (Mx_out) *Mx_out = Mx;
    if (My_out) *My_out = My;
    return 0;
}

void equate_free(EquateState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = EquateState{};
}

int equate_alloc(hipStream_t st, EquateState* p, int64_t m, const unsigned char* mask_x, const unsigned char* mask_y)
{
    int64_t Mx = 0, My = 0;
    GP_TRY(equate_check(m, mask_x, mask_y, &Mx, &My));
    const EquateLayout L = equate_layout(m, Mx, My);
    p->m = m; p->Mx = Mx; p->My = My;
    p->steps_x = sumscore_steps(Mx);
    p->steps_y = sumscore_steps(My);
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->tab_x, 2 * sizeof(double) * (size_t)EQ_N * (size_t)p->steps_x));
    GP_TRY(get((void**)&p->tab_y, 2 * sizeof(double) * (size_t)EQ_N * (size_t)p->steps_y));
    GP_TRY(get((void**)&p->AX, sizeof(double) * (size_t)EQ_NP * (size_t)(Mx + 1)));       // rows 1001 .. 1023 stay zero
    GP_TRY(get((void**)&p->WX, sizeof(double) * (size_t)EQ_NP * (size_t)(Mx + 1)));
    GP_TRY(get((void**)&p->AY, sizeof(double) * (size_t)EQ_NP * (size_t)(My + 1)));
    GP_TRY(get((void**)&p->TV, sizeof(double) * 4 * EQ_NP));
    GP_TRY(get((void**)&p->cols_x, sizeof(int) * (size_t)Mx));
    GP_TRY(get((void**)&p->cols_y, sizeof(int) * (size_t)My));
    GP_TRY(get((void**)&p->ctl, 16));
    std::vector<int> cx, cy;
    std::vector<unsigned char> bx((size_t)m), by((size_t)m);
    for (int64_t j = 0; j < m; ++j) {
        bx[(size_t)j] = mask_x[j] ? 1 : 0;
        by[(size_t)j] = mask_y[j] ? 1 : 0;
        if (bx[(size_t)j]) cx.push_back((int)j);
        if (by[(size_t)j]) cy.push_back((int)j);
    }
    std::vector<double> w(EQ_N);
    sumscore_grid_weights(w.data());
    const int64_t hdr[EQUATE_HEADER_WORDS] = { EQUATE_TAG, EQUATE_LAYOUT_VERSION, m, Mx, My, EQ_N };
    GP_HIP(hipMemcpyAsync(p->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->block + L.off[GPIRT_EQUATE_MASK_X], bx.data(), (size_t)m, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->block + L.off[GPIRT_EQUATE_MASK_Y], by.data(), (size_t)m, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->block + L.off[GPIRT_EQUATE_W], w.data(), sizeof(double) * EQ_N, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->cols_x, cx.data(), sizeof(int) * (size_t)Mx, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->cols_y, cy.data(), sizeof(int) * (size_t)My, hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // the host vectors are this call's: nothing may leave with the copies pending
    p->on = true;
    return 0;
}

int launch_equate_accumulate(gpirt_handle_t h, hipStream_t st, EquateState* p, const double* fstar)
{
    const EquateLayout L = equate_layout(p->m, p->Mx, p->My);
    auto f64 = [&](int k) { return reinterpret_cast<double*>(p->block + L.off[k]); };
    const int Mx = (int)p->Mx, My = (int)p->My;
    const double* w = f64(GPIRT_EQUATE_W);
    double *TX = p->TV, *VX = p->TV + EQ_NP, *TY = p->TV + 2 * EQ_NP, *VY = p->TV + 3 * EQ_NP;
    GP_HIP(hipMemsetAsync(p->ctl, 0, 2 * sizeof(int), st));
    GP_HIP(hipMemsetAsync(p->WX, 0, sizeof(double) * (size_t)EQ_N * (size_t)(Mx + 1), st));    // the row kernel ADDS w_k A to it
    GP_TRY(launch_sumscore_table(st, fstar, p->cols_x, Mx, (int)p->steps_x, p->tab_x, p->ctl));
    GP_TRY(launch_sumscore_table(st, fstar, p->cols_y, My, (int)p->steps_y, p->tab_y, p->ctl));
    GP_TRY(launch_sumscore_rows(st, p->tab_x, Mx, (int)p->steps_x, w, p->ctl, p->AX, p->WX, TX, VX));
    GP_TRY(launch_sumscore_rows(st, p->tab_y, My, (int)p->steps_y, w, p->ctl, p->AY, nullptr, TY, VY));
    GP_TRY(launch_sumscore_pi(st, p->AX, w, Mx, p->ctl, f64(GPIRT_EQUATE_LAST_PIX), f64(GPIRT_EQUATE_PIX_SUM), f64(GPIRT_EQUATE_PIX_SUMSQ)));
    GP_TRY(launch_sumscore_pi(st, p->AY, w, My, p->ctl, f64(GPIRT_EQUATE_LAST_PIY), f64(GPIRT_EQUATE_PIY_SUM), f64(GPIRT_EQUATE_PIY_SUMSQ)));
    hipLaunchKernelGGL(equate_fin_kernel, dim3(1), dim3(EQ_FIN_THREADS), 0, st, f64(GPIRT_EQUATE_LAST_PIX), f64(GPIRT_EQUATE_LAST_PIY),
                       Mx, My, TX, VX, TY, VY, w, p->ctl, f64(GPIRT_EQUATE_EYX_SUM), f64(GPIRT_EQUATE_EYX_SUMSQ),
                       f64(GPIRT_EQUATE_EXY_SUM), f64(GPIRT_EQUATE_EXY_SUMSQ), f64(GPIRT_EQUATE_LAST_EYX), f64(GPIRT_EQUATE_LAST_EXY),
                       f64(GPIRT_EQUATE_CORR), f64(GPIRT_EQUATE_CORR_TERMS), reinterpret_cast<int64_t*>(p->block));
    GP_HIP(hipGetLastError());
    // last_joint[s (M_Y + 1) + t] = sum_k A_Y[k, t] (w_k A_X[k, s]): column-major (M_Y + 1) x (M_X + 1), both operands stored
    // score-contiguous per grid point (the row kernel's layout), K over all 1024 rows
    GP_TRY(launch_gemm(h, st, false, true, TRI_NONE, My + 1, Mx + 1, EQ_NP, 1.0, p->AY, My + 1, p->WX, Mx + 1, 0.0,
                       f64(GPIRT_EQUATE_LAST_JOINT), My + 1, 0, p->ctl + 1));
    const int64_t cells = (int64_t)(Mx + 1) * (My + 1);
    int64_t blocks = (cells + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(equate_add_kernel, dim3((unsigned)blocks), dim3(256), 0, st, f64(GPIRT_EQUATE_LAST_JOINT), cells, p->ctl,
                       f64(GPIRT_EQUATE_JOINT_SUM));
    GP_HIP(hipGetLastError());
    return 0;
}

int equate_get(hipStream_t st, EquateState* p, const char* name, void* h_out, int64_t bytes)
{
    const EquateLayout L = equate_layout(p->m, p->Mx, p->My);
    auto copy = [&](const void* src) -> int {
        GP_HIP(hipMemcpyAsync(h_out, src, (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 40); return copy(p->block + 6); }
    for (int k = 0; k < GPIRT_EQUATE_NARRAYS; ++k)
        if (strcmp(kEquateRaw[k], name) == 0) {
            GP_ARG(bytes == eq_raw_bytes(k, p->m, p->Mx, p->My));
            return copy(p->block + L.off[k]);
        }
    set_error("unknown equate field '%s'", name);
    return GPIRT_E_ARG;
}

int equate_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_equate* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    HostEquate pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostEquate& r = c == 0 ? pooled : one;
        GP_TRY(equate_read(h->stream, d_states[c], r, "gpirt_equate_combine", c));
        if (c == 0) continue;
        if (r.m != pooled.m || r.Mx != pooled.Mx || r.My != pooled.My ||
            memcmp(r.bytes(GPIRT_EQUATE_MASK_X), pooled.bytes(GPIRT_EQUATE_MASK_X), (size_t)r.m) != 0 ||
            memcmp(r.bytes(GPIRT_EQUATE_MASK_Y), pooled.bytes(GPIRT_EQUATE_MASK_Y), (size_t)r.m) != 0 ||
            memcmp(r.f64(GPIRT_EQUATE_W), pooled.f64(GPIRT_EQUATE_W), sizeof(double) * EQ_N) != 0) {
            set_error("gpirt_equate_combine: state %d has another m, other forms or other grid weights than state 0", c);
            return GPIRT_E_ARG;
        }
        for (int q = 6; q <= 10; ++q) pooled.hdr()[q] += one.hdr()[q];
        for (int k = 0; k <= GPIRT_EQUATE_CORR; ++k) {                 // the sums, in chain order
            const int64_t cnt = eq_raw_bytes(k, r.m, r.Mx, r.My) / 8;
            double *a = pooled.f64(k), *b = one.f64(k);
            for (int64_t g = 0; g < cnt; ++g) a[g] += b[g];
        }
        for (int k : { GPIRT_EQUATE_CORR_TERMS, GPIRT_EQUATE_LAST_JOINT, GPIRT_EQUATE_LAST_PIX, GPIRT_EQUATE_LAST_PIY,
                       GPIRT_EQUATE_LAST_EYX, GPIRT_EQUATE_LAST_EXY })  // the last state's last draw
            memcpy(pooled.f64(k), one.f64(k), (size_t)eq_raw_bytes(k, r.m, r.Mx, r.My));
    }
    equate_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
