// sumscore.hip -- posteriors of the sum score S = number of yes answers on a form of M items (include/gpirt_hip.h, "Sum-score
// posteriors"): per draw the Poisson-binomial P(S = s | theta_k) at every grid point by the
// Lord-Wingersky recursion, from it the score distribution, the joint of (theta_k, s), the test characteristic curve and the
// sum score's reliability -- accumulated one draw at a time without stored draws.
//
// sumscore_table_kernel: p = 1 / (1 + exp(-f*)) and q = 1 / (1 + exp(+f*)) of the form's columns, read lanes along k (f* is
//   stored k-contiguous) and turned through LDS so that the table is j-contiguous per grid point: tab[k][jj] = (p, q), padded to a
//   multiple of 32 steps with (0, 1), the step that changes nothing.  A NaN in a form column raises the draw's skip word.
// sumscore_row_kernel<R>: one wave per grid point.  Lane l owns the scores s = l R .. l R + R - 1 in R registers (R = 17 / 33 /
//   65 for M + 1 <= 1088 / 2112 / 4160); a step is A[s] <- A[s] q + A[s - 1] p on every register, the one value that crosses
//   between lanes coming by a shift of the wave by one lane.  p and q are the same for the whole wave: they come through the scalar
//   cache eight steps at a time.  T[k] = sum p and V[k] = sum p q are added on the way in ascending j.  The row goes out through
//   LDS, lanes along s: last[k, .] and joint_sum[k, .] += w_k A.
// sumscore_pi_kernel: pi[s] = sum_k w_k A[k, s] in ascending k, lanes along s, sixteen loads in flight.
// sumscore_fin_kernel: one work-group: the TCC sums, the reliability's three sums in ascending k, the header's counters.
// The skip word is read by every kernel before it touches anything: a skipped draw changes the counter `skipped` alone.
// Every accumulator cell is owned by one lane: no atomics, bit-identical from run to run.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace gpirt {

namespace {

constexpr int SS_N = GPIRT_NGRID;                 // 1001 grid points
constexpr int SS_PAD = 1024;
constexpr int SS_TILE_K = 64, SS_TILE_J = 32;     // the table kernel's tile
constexpr int SS_STEP_PAD = SS_TILE_J;            // the table's steps per grid point are a multiple of this (and of SS_CHUNK)
constexpr int SS_CHUNK = 8;                       // steps whose (p, q) the row kernel fetches at once
constexpr int SS_PI_THREADS = 64, SS_PI_FLIGHT = 16;
constexpr int SS_FIN_THREADS = 256;
static_assert(SS_STEP_PAD % SS_CHUNK == 0, "the row kernel walks the padded table in whole chunks");

const char* const kSumscoreRaw[GPIRT_SUMSCORE_NARRAYS] = { "joint_sum", "pi_sum", "pi_sumsq", "tcc_sum", "tcc_sumsq", "var_sum",
                                                           "rel", "mask", "w", "last", "last_pi" };

inline int64_t ss_raw_bytes(int k, int64_t m, int64_t M)
{
    switch (k) {
        case GPIRT_SUMSCORE_JOINT_SUM: case GPIRT_SUMSCORE_LAST: return 8 * (int64_t)SS_N * (M + 1);
        case GPIRT_SUMSCORE_PI_SUM: case GPIRT_SUMSCORE_PI_SUMSQ: case GPIRT_SUMSCORE_LAST_PI: return 8 * (M + 1);
        case GPIRT_SUMSCORE_TCC_SUM: case GPIRT_SUMSCORE_TCC_SUMSQ: case GPIRT_SUMSCORE_VAR_SUM: case GPIRT_SUMSCORE_W: return 8 * (int64_t)SS_N;
        case GPIRT_SUMSCORE_REL: return 16;
        default: return m;                        // GPIRT_SUMSCORE_MASK: a byte per item
    }
}

// grid: (ceil(1001 / 64), steps / 32), 256 lanes
__global__ __launch_bounds__(256) void sumscore_table_kernel(const double* __restrict__ fstar, const int* __restrict__ cols, int M,
                                                             int steps, double2* __restrict__ tab, int* __restrict__ ctl)
{
    __shared__ double2 tile[SS_TILE_K][SS_TILE_J + 1];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int k = blockIdx.x * SS_TILE_K + lane, j0 = blockIdx.y * SS_TILE_J;
    int bad = 0;
    for (int i = 0; i < SS_TILE_J / 4; ++i) {
        const int jl = wv + 4 * i, jj = j0 + jl;
        double2 pq = make_double2(0.0, 1.0);                      // beyond the form: the step that changes nothing
        if (jj < M && k < SS_N) {
            const double f = fstar[(int64_t)cols[jj] * SS_N + k];
            bad |= (f != f) ? 1 : 0;
            pq.x = 1.0 / (1.0 + exp(-f));                         // each on its own: q is never 1 - p
            pq.y = 1.0 / (1.0 + exp(f));
        }
        tile[lane][jl] = pq;
    }
    if (bad) ctl[0] = 1;                                          // (every writer writes the same word)
    __syncthreads();
    const int jl = t & (SS_TILE_J - 1);
    for (int i = 0; i < SS_TILE_K / 8; ++i) {
        const int kl = (t >> 5) + 8 * i, kk = blockIdx.x * SS_TILE_K + kl;
        if (kk < SS_N) tab[(int64_t)kk * steps + j0 + jl] = tile[kl][jl];
    }
}

// the value of the lane below (0 in lane 0): a shift of the whole wave by one lane, two 32-bit halves
__device__ __forceinline__ double from_lane_below(double x)
{
    const int lo = __double2loint(x), hi = __double2hiint(x);
    const int l2 = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, false);    // wave_shr:1
    const int h2 = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(h2, l2);
}

// grid: 1001 work-groups of one wave
template <int R>
__global__ __launch_bounds__(64) void sumscore_row_kernel(const double2* __restrict__ tab, int M, int steps, const double* __restrict__ w,
                                                          const int* __restrict__ ctl, double* __restrict__ last,
                                                          double* __restrict__ joint, double* __restrict__ T, double* __restrict__ V)
{
    __shared__ double row[R * 64];
    if (ctl[0]) return;
    const int lane = threadIdx.x, k = blockIdx.x;
    double A[R];
#pragma unroll
    for (int r = 0; r < R; ++r) A[r] = 0.0;
    if (lane == 0) A[0] = 1.0;
    const double2* __restrict__ pq = tab + (int64_t)k * steps;
    double Tk = 0.0, Vk = 0.0;
    for (int j = 0; j < steps; j += SS_CHUNK) {
        double2 c[SS_CHUNK];
#pragma unroll
        for (int u = 0; u < SS_CHUNK; ++u) c[u] = pq[j + u];
#pragma unroll
        for (int u = 0; u < SS_CHUNK; ++u) {
            const double p = c[u].x, q = c[u].y;
            const double up = from_lane_below(A[R - 1]);
#pragma unroll
            for (int r = R - 1; r >= 1; --r) A[r] = A[r] * q + A[r - 1] * p;
            A[0] = A[0] * q + up * p;
            Tk += p;
            Vk += p * q;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) row[lane * R + r] = A[r];
    __syncthreads();
    const double wk = w[k];
    const int64_t at = (int64_t)k * (M + 1);
    for (int s = lane; s <= M; s += 64) {                         // s <= M < 64 R
        const double a = row[s];
        last[at + s] = a;
        if (joint) joint[at + s] += wk * a;                       // (NULL: a caller that keeps no weighted copy, equate.hip's form Y)
    }
    if (lane == 0) { T[k] = Tk; V[k] = Vk; }
}

// grid: ceil((M + 1) / 64) work-groups of one wave, one lane per score
__global__ __launch_bounds__(SS_PI_THREADS) void sumscore_pi_kernel(const double* __restrict__ last, const double* __restrict__ w, int M,
                                                                    const int* __restrict__ ctl, double* __restrict__ last_pi,
                                                                    double* __restrict__ pi_sum, double* __restrict__ pi_sumsq)
{
    if (ctl[0]) return;
    const int s = blockIdx.x * SS_PI_THREADS + threadIdx.x;
    if (s > M) return;
    const int64_t ld = (int64_t)M + 1;
    double acc = 0.0;
    int k = 0;
    for (; k + SS_PI_FLIGHT <= SS_N; k += SS_PI_FLIGHT) {         // sixteen loads in flight, added in ascending k
        double v[SS_PI_FLIGHT];
#pragma unroll
        for (int q = 0; q < SS_PI_FLIGHT; ++q) v[q] = last[(int64_t)(k + q) * ld + s];
#pragma unroll
        for (int q = 0; q < SS_PI_FLIGHT; ++q) acc += w[k + q] * v[q];
    }
    for (; k < SS_N; ++k) acc += w[k] * last[(int64_t)k * ld + s];
    last_pi[s] = acc;
    pi_sum[s] += acc;
    pi_sumsq[s] += acc * acc;
}

__global__ __launch_bounds__(SS_FIN_THREADS) void sumscore_fin_kernel(const double* __restrict__ T, const double* __restrict__ V,
                                                                      const double* __restrict__ w, const int* __restrict__ ctl,
                                                                      double* __restrict__ tcc_sum, double* __restrict__ tcc_sumsq,
                                                                      double* __restrict__ var_sum, double* __restrict__ rel,
                                                                      int64_t* __restrict__ hdr)
{
    __shared__ double ta[SS_PAD], tb[SS_PAD], tc[SS_PAD];
    const int t = threadIdx.x;
    if (ctl[0]) {
        if (t == 0) hdr[6] += 1;                                  // skipped
        return;
    }
    for (int k = t; k < SS_N; k += SS_FIN_THREADS) {
        const double Tk = T[k], Vk = V[k], wk = w[k];
        tcc_sum[k] += Tk;
        tcc_sumsq[k] += Tk * Tk;
        var_sum[k] += Vk;
        ta[k] = wk * Vk;
        tb[k] = wk * (Vk + Tk * Tk);
        tc[k] = wk * Tk;
    }
    __syncthreads();
    if (t == 0) {
        double a = 0.0, b = 0.0, c = 0.0;
        for (int k = 0; k < SS_N; ++k) { a += ta[k]; b += tb[k]; c += tc[k]; }      // ascending k
        hdr[5] += 1;                                              // draws
        const double den = b - c * c;
        if (den > 0.0) {
            const double rho = 1.0 - a / den;
            rel[0] += rho;
            rel[1] += rho * rho;
            hdr[7] += 1;                                          // rel_draws
        } else {
            hdr[8] += 1;                                          // rel_skipped
        }
    }
}

// a state block on the host
struct HostSumscore {
    std::vector<uint64_t> w;
    int64_t m = 0, M = 0;
    SumscoreLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    double* f64(int k) { return reinterpret_cast<double*>(w.data() + L.off[k]); }
    const unsigned char* mask() const { return reinterpret_cast<const unsigned char*>(w.data() + L.off[GPIRT_SUMSCORE_MASK]); }
};

int sumscore_read(hipStream_t st, const void* d_state, HostSumscore& r, const char* who, int c)
{
    int64_t hdr[SUMSCORE_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] != SUMSCORE_TAG || hdr[1] != SUMSCORE_LAYOUT_VERSION || hdr[2] <= 0 || hdr[3] < 1 || hdr[3] > hdr[2] ||
        hdr[3] > GPIRT_SUMSCORE_MAX_ITEMS || hdr[4] != SS_N || hdr[5] < 0 || hdr[6] < 0 || hdr[7] < 0 || hdr[8] < 0) {
        set_error("%s: state %d is not a sum-score state block of layout %d", who, c, SUMSCORE_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.m = hdr[2]; r.M = hdr[3];
    r.L = sumscore_layout(r.m, r.M);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

// theta -> -theta on the accumulators (include/gpirt_hip.h): the k axis of everything indexed by k; pi and rel are kept
void sumscore_reflect(HostSumscore& r)
{
    const int64_t ld = r.M + 1;
    for (int k : { GPIRT_SUMSCORE_JOINT_SUM, GPIRT_SUMSCORE_LAST }) {
        double* a = r.f64(k);
        for (int lo = 0, hi = SS_N - 1; lo < hi; ++lo, --hi) std::swap_ranges(a + lo * ld, a + (lo + 1) * ld, a + hi * ld);
    }
    for (int k : { GPIRT_SUMSCORE_TCC_SUM, GPIRT_SUMSCORE_TCC_SUMSQ, GPIRT_SUMSCORE_VAR_SUM }) std::reverse(r.f64(k), r.f64(k) + SS_N);
}

void sumscore_fill(HostSumscore& r, gpirt_sumscore* out)
{
    const int64_t* h = r.hdr();
    out->m = r.m; out->M = r.M; out->draws = h[5]; out->skipped = h[6]; out->rel_draws = h[7]; out->rel_skipped = h[8];
    for (int k = 0; k < GPIRT_SUMSCORE_NARRAYS; ++k)
        if (out->raw[k]) memcpy(out->raw[k], r.w.data() + r.L.off[k], (size_t)ss_raw_bytes(k, r.m, r.M));
}

}  // namespace

SumscoreLayout sumscore_layout(int64_t m, int64_t M)
{
    SumscoreLayout L{};
    int64_t at = SUMSCORE_HEADER_WORDS;
    for (int k = 0; k < GPIRT_SUMSCORE_NARRAYS; ++k) {
        L.off[k] = at;
        at += (ss_raw_bytes(k, m, M) + 15) / 16 * 2;                  // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

void sumscore_grid_weights(double* w)
{
    // the N(0, 1) density on the grid, normalised: theta_k the double -5 + 0.01 k, everything else in long double, the sum in
    // ascending k, rounded once
    long double e[SS_N], sum = 0.0L;
    for (int k = 0; k < SS_N; ++k) {
        const long double th = (long double)(-5.0 + (double)k * 0.01);
        e[k] = expl(-(th * th) / 2.0L);
        sum += e[k];
    }
    for (int k = 0; k < SS_N; ++k) w[k] = (double)(e[k] / sum);
}

int sumscore_check(int64_t m, const unsigned char* mask, int64_t* M_out)
{
    int64_t M = 0;
    if (mask) { for (int64_t j = 0; j < m; ++j) M += mask[j] ? 1 : 0; }
    else M = m;
    if (M < 1) {
        set_error("sum-score posteriors: the form is empty (no item of the %lld is in it)", (long long)m);
        return GPIRT_E_ARG;
    }
    if (M > GPIRT_SUMSCORE_MAX_ITEMS) {
        set_error("sum-score posteriors: the form has M = %lld items, at most %d are taken", (long long)M, GPIRT_SUMSCORE_MAX_ITEMS);
        return GPIRT_E_ARG;
    }
    if (M_out) *M_out = M;
    return 0;
}

int64_t sumscore_steps(int64_t M) { return (M + SS_STEP_PAD - 1) / SS_STEP_PAD * SS_STEP_PAD; }

void sumscore_free(SumscoreState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = SumscoreState{};
}

int sumscore_alloc(hipStream_t st, SumscoreState* p, int64_t m, const unsigned char* mask)
{
    int64_t M = 0;
    GP_TRY(sumscore_check(m, mask, &M));
    const SumscoreLayout L = sumscore_layout(m, M);
    p->m = m; p->M = M;
    p->steps = sumscore_steps(M);
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->tab, 2 * sizeof(double) * (size_t)SS_N * (size_t)p->steps));
    GP_TRY(get((void**)&p->T, sizeof(double) * SS_PAD));
    GP_TRY(get((void**)&p->V, sizeof(double) * SS_PAD));
    GP_TRY(get((void**)&p->cols, sizeof(int) * (size_t)M));
    GP_TRY(get((void**)&p->ctl, 16));
    std::vector<int> cols;
    std::vector<unsigned char> bytes((size_t)m, 1);
    for (int64_t j = 0; j < m; ++j) {
        if (mask) bytes[(size_t)j] = mask[j] ? 1 : 0;
        if (bytes[(size_t)j]) cols.push_back((int)j);
    }
    std::vector<double> w(SS_N);
    sumscore_grid_weights(w.data());
    const int64_t hdr[SUMSCORE_HEADER_WORDS] = { SUMSCORE_TAG, SUMSCORE_LAYOUT_VERSION, m, M, SS_N };
    GP_HIP(hipMemcpyAsync(p->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->block + L.off[GPIRT_SUMSCORE_MASK], bytes.data(), (size_t)m, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->block + L.off[GPIRT_SUMSCORE_W], w.data(), sizeof(double) * SS_N, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->cols, cols.data(), sizeof(int) * (size_t)M, hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // the host vectors are this call's: nothing may leave with the copies pending
    p->on = true;
    return 0;
}

int launch_sumscore_table(hipStream_t st, const double* fstar, const int* cols, int M, int steps, double* tab, int* ctl)
{
    hipLaunchKernelGGL(sumscore_table_kernel, dim3((SS_N + SS_TILE_K - 1) / SS_TILE_K, (unsigned)(steps / SS_TILE_J)), dim3(256), 0, st,
                       fstar, cols, M, steps, reinterpret_cast<double2*>(tab), ctl);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_sumscore_rows(hipStream_t st, const double* tab_, int M, int steps, const double* w, const int* ctl, double* last,
                         double* joint, double* T, double* V)
{
    const double2* tab = reinterpret_cast<const double2*>(tab_);
    if (M + 1 <= 17 * 64)
        hipLaunchKernelGGL(sumscore_row_kernel<17>, dim3(SS_N), dim3(64), 0, st, tab, M, steps, w, ctl, last, joint, T, V);
    else if (M + 1 <= 33 * 64)
        hipLaunchKernelGGL(sumscore_row_kernel<33>, dim3(SS_N), dim3(64), 0, st, tab, M, steps, w, ctl, last, joint, T, V);
    else
        hipLaunchKernelGGL(sumscore_row_kernel<65>, dim3(SS_N), dim3(64), 0, st, tab, M, steps, w, ctl, last, joint, T, V);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_sumscore_pi(hipStream_t st, const double* last, const double* w, int M, const int* ctl, double* last_pi, double* pi_sum,
                       double* pi_sumsq)
{
    hipLaunchKernelGGL(sumscore_pi_kernel, dim3((unsigned)((M + 1 + SS_PI_THREADS - 1) / SS_PI_THREADS)), dim3(SS_PI_THREADS), 0, st,
                       last, w, M, ctl, last_pi, pi_sum, pi_sumsq);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_sumscore_accumulate(hipStream_t st, SumscoreState* p, const double* fstar)
{
    const SumscoreLayout L = sumscore_layout(p->m, p->M);
    auto f64 = [&](int k) { return reinterpret_cast<double*>(p->block + L.off[k]); };
    const int M = (int)p->M, steps = (int)p->steps;
    const double* w = f64(GPIRT_SUMSCORE_W);
    GP_HIP(hipMemsetAsync(p->ctl, 0, sizeof(int), st));
    GP_TRY(launch_sumscore_table(st, fstar, p->cols, M, steps, p->tab, p->ctl));
    double *last = f64(GPIRT_SUMSCORE_LAST), *joint = f64(GPIRT_SUMSCORE_JOINT_SUM);
    GP_TRY(launch_sumscore_rows(st, p->tab, M, steps, w, p->ctl, last, joint, p->T, p->V));
    GP_TRY(launch_sumscore_pi(st, last, w, M, p->ctl, f64(GPIRT_SUMSCORE_LAST_PI), f64(GPIRT_SUMSCORE_PI_SUM), f64(GPIRT_SUMSCORE_PI_SUMSQ)));
    hipLaunchKernelGGL(sumscore_fin_kernel, dim3(1), dim3(SS_FIN_THREADS), 0, st, p->T, p->V, w, p->ctl, f64(GPIRT_SUMSCORE_TCC_SUM),
                       f64(GPIRT_SUMSCORE_TCC_SUMSQ), f64(GPIRT_SUMSCORE_VAR_SUM), f64(GPIRT_SUMSCORE_REL),
                       reinterpret_cast<int64_t*>(p->block));
    GP_HIP(hipGetLastError());
    return 0;
}

int sumscore_get(hipStream_t st, SumscoreState* p, const char* name, void* h_out, int64_t bytes)
{
    const SumscoreLayout L = sumscore_layout(p->m, p->M);
    auto copy = [&](const void* src) -> int {
        GP_HIP(hipMemcpyAsync(h_out, src, (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 32); return copy(p->block + 5); }
    if (strcmp(name, "tcc") == 0) { GP_ARG(bytes == 8 * (int64_t)SS_N); return copy(p->T); }
    if (strcmp(name, "var") == 0) { GP_ARG(bytes == 8 * (int64_t)SS_N); return copy(p->V); }
    for (int k = 0; k < GPIRT_SUMSCORE_NARRAYS; ++k)
        if (strcmp(kSumscoreRaw[k], name) == 0) {
            GP_ARG(bytes == ss_raw_bytes(k, p->m, p->M));
            return copy(p->block + L.off[k]);
        }
    set_error("unknown sumscore field '%s'", name);
    return GPIRT_E_ARG;
}

int sumscore_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_sumscore* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    for (int c = 0; c < chains; ++c) {
        GP_ARG(d_states[c]);
        if (signs) GP_ARG(signs[c] == 1 || signs[c] == -1);
    }
    HostSumscore pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostSumscore& r = c == 0 ? pooled : one;
        GP_TRY(sumscore_read(h->stream, d_states[c], r, "gpirt_sumscore_combine", c));
        if (c > 0 && (r.m != pooled.m || r.M != pooled.M || memcmp(r.mask(), pooled.mask(), (size_t)r.m) != 0 ||
                      memcmp(r.f64(GPIRT_SUMSCORE_W), pooled.f64(GPIRT_SUMSCORE_W), sizeof(double) * SS_N) != 0)) {
            set_error("gpirt_sumscore_combine: state %d has another m, another form or other grid weights than state 0", c);
            return GPIRT_E_ARG;
        }
        if (signs && signs[c] < 0) sumscore_reflect(r);
        if (c == 0) continue;
        for (int q = 5; q <= 8; ++q) pooled.hdr()[q] += one.hdr()[q];
        for (int k = 0; k <= GPIRT_SUMSCORE_REL; ++k) {               // the sums, in chain order
            const int64_t cnt = ss_raw_bytes(k, r.m, r.M) / 8;
            double *a = pooled.f64(k), *b = one.f64(k);
            for (int64_t g = 0; g < cnt; ++g) a[g] += b[g];
        }
        for (int k : { GPIRT_SUMSCORE_LAST, GPIRT_SUMSCORE_LAST_PI })  // the last chain's last draw
            memcpy(pooled.f64(k), one.f64(k), (size_t)ss_raw_bytes(k, r.m, r.M));
    }
    sumscore_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
