// ppc_pairs.hip -- pairwise item checks of the posterior predictive checks (include/gpirt_hip.h, "pairwise item checks";
// DESIGN.md section 18): for every pair of items the 2 x 2 table of the replicate over the co-observed respondents against
// the data's -- the joint yes count, the agreement and the odds ratio -- accumulated one draw at a time without stored draws.
//
// The counts are products of 0 / 1 matrices, exact on the int8 matrix cores (as theta_fixed.hip's digit planes are):
//     r11 = rep^T rep,  r1 = rep^T O          (m x m each, depth n, int32)
// with rep[i, j] = [yrep_ij = +1][y_ij observed] the bytes ppc_replicate_kernel<true> leaves and O[i, j] = [y_ij observed].
// Operands are stored in the "fragment order" of theta_fixed.hip, the 1 KiB one v_mfma_i32_32x32x32_i8 consumes, with
// k = the respondent:
//     X8 [j / 32][k / 32][lane = (j % 32) + 32 ((k % 32) / 16)][k % 16]        bytes 0 / 1
// the items zero-padded to a multiple of 128 (a work-group's tile), k to a multiple of 256 (whole chunks of PC_KS k-steps).
// pair_counts_kernel: a work-group owns 128 x 128 of X^T [X | O]; wave w the 64 x 64 at (w / 2, w % 2) = 2 x 2 accumulator
// tiles.  Four item blocks of each operand, PC_KS k-steps deep, lie in one of two LDS stages (32 KiB each); the next chunk
// travels global -> registers under this chunk's 16 MFMAs per wave and registers -> the other stage behind them, one barrier
// per chunk.  Of X^T X only the work-group tiles on and below the diagonal are computed; the ones below are stored twice.
// pair_update_kernel: one thread per ordered pair (a, b) makes the six decisions in integers and updates its accumulators:
// no atomics, bit-identical from run to run.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace gpirt {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int PC_KS = 4;                          // k-steps (of 32 respondents) per LDS stage
constexpr int PC_TILE = 128;                      // items per side of a work-group's tile
constexpr int PC_STAGE = 8 * PC_KS * 1024;        // four item blocks of each operand, bytes
static_assert(2 * PC_STAGE <= 64 * 1024, "two stages in the LDS a work-group may ask for");
static_assert(256 % (32 * PC_KS) == 0, "ppc_replicate_kernel's 256 respondents are whole chunks");

const char* const kPairFields[GPIRT_PAIRS_NFIELDS] = {
    "n_co", "obs_n11", "obs_n10", "obs_n01", "obs_n00", "rep_n11_mean", "rep_n11_var", "rep_n10_mean", "rep_n01_mean",
    "rep_n00_mean", "agree_obs", "agree_rep_mean", "log_or_obs", "ppp_n11", "ppp_n11_mid", "ppp_agree", "ppp_agree_mid",
    "ppp_or", "ppp_or_mid" };
const char* const kPairCounts[6] = { "n11_ge", "n11_gt", "agree_ge", "agree_gt", "or_ge", "or_gt" };

__device__ __forceinline__ uint32_t pack4(int b0, int b1, int b2, int b3)
{
    return (uint32_t)b0 | ((uint32_t)b1 << 8) | ((uint32_t)b2 << 16) | ((uint32_t)b3 << 24);
}

// O8 and Y8 (once, at enable): one thread per 16-byte piece
__global__ __launch_bounds__(256) void pair_bytes_kernel(const double* __restrict__ y, int64_t n, int64_t m, int64_t iblocks,
                                                         int64_t ksteps, uint4* __restrict__ O8, uint4* __restrict__ Y8)
{
    const int64_t total = iblocks * ksteps * 64;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int lane = (int)(t & 63);
        const int64_t ks = (t >> 6) % ksteps, ib = (t >> 6) / ksteps;
        const int64_t j = ib * 32 + (lane & 31), i0 = ks * 32 + 16 * (lane >> 5);
        int o[16], p[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            double v = (double)NAN;
            if (j < m && i0 + q < n) v = y[i0 + q + j * n];
            o[q] = v == v ? 1 : 0;
            p[q] = v > 0.0 ? 1 : 0;
        }
        O8[t] = make_uint4(pack4(o[0], o[1], o[2], o[3]), pack4(o[4], o[5], o[6], o[7]), pack4(o[8], o[9], o[10], o[11]),
                           pack4(o[12], o[13], o[14], o[15]));
        Y8[t] = make_uint4(pack4(p[0], p[1], p[2], p[3]), pack4(p[4], p[5], p[6], p[7]), pack4(p[8], p[9], p[10], p[11]),
                           pack4(p[12], p[13], p[14], p[15]));
    }
}

struct PairCountArgs {
    const unsigned char* X8;             // the planes of X (one, or two with `cur`)
    const unsigned char* O8;
    const int* cur;                      // non-null: X is the plane *cur does NOT name (this draw's replicate)
    const int* skip;                     // non-null and *skip != 0: this draw is skipped, nothing is written
    int64_t plane, ksteps, m;
    int nab;                             // work-group tiles per side
    int* x11; int* x1;                   // X^T X and X^T O, m x m, (a, b) at [a m + b]; x1 may be null (grid.y = nab then)
};

// register v of lane l of an accumulator tile: item a = (v & 3) + 8 (v >> 2) + 4 (l >> 5) of the first operand's block,
// item b = l & 31 of the second's
__device__ __forceinline__ void pair_store_tile(const v16i& acc, int* __restrict__ out, int64_t m, int64_t a0, int64_t b0,
                                                int lane, bool mirror)
{
    const int64_t b = b0 + (lane & 31);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int64_t a = a0 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
        if (a < m && b < m) {
            out[a * m + b] = acc[v];
            if (mirror) out[b * m + a] = acc[v];
        }
    }
}

__global__ __launch_bounds__(256) void pair_counts_kernel(PairCountArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pc_lds[];
    const int ab = (int)blockIdx.x, by = (int)blockIdx.y;
    const bool second = by >= a.nab;                 // the X^T O half
    const int bb = second ? by - a.nab : by;
    if (!second && bb > ab) return;                   // X^T X: the mirror of a tile below the diagonal
    if (a.skip && *a.skip) return;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wa = wave >> 1, wb = wave & 1;
    const unsigned char* X = a.X8 + (a.cur ? (int64_t)(*a.cur ^ 1) * a.plane : 0);
    const unsigned char* B = second ? a.O8 : X;
    const int64_t ksteps = a.ksteps;
    const int nchunks = (int)(ksteps / PC_KS);
    // block q < 4: item block 4 ab + q of X; q >= 4: item block 4 bb + q - 4 of the second operand; a chunk of a block is
    // PC_KS KiB in a row
    const unsigned char* src[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        src[q] = X + ((int64_t)(4 * ab + q) * ksteps) * 1024 + tid * 16;
        src[4 + q] = B + ((int64_t)(4 * bb + q) * ksteps) * 1024 + tid * 16;
    }
    v16i acc[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[r][c][v] = 0;
    v4i nx[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) nx[q] = *reinterpret_cast<const v4i*>(src[q]);
#pragma unroll
    for (int q = 0; q < 8; ++q) *reinterpret_cast<v4i*>(pc_lds + q * (PC_KS * 1024) + tid * 16) = nx[q];
    __syncthreads();
    for (int c = 0; c < nchunks; ++c) {
        const unsigned char* st = pc_lds + (c & 1) * PC_STAGE + lane * 16;
        const bool more = c + 1 < nchunks;
        if (more) {
            const int64_t adv = (int64_t)(c + 1) * PC_KS * 1024;
#pragma unroll
            for (int q = 0; q < 8; ++q) nx[q] = *reinterpret_cast<const v4i*>(src[q] + adv);
        }
#pragma unroll
        for (int ks = 0; ks < PC_KS; ++ks) {
            const v4i a0 = *reinterpret_cast<const v4i*>(st + ((2 * wa) * PC_KS + ks) * 1024);
            const v4i a1 = *reinterpret_cast<const v4i*>(st + ((2 * wa + 1) * PC_KS + ks) * 1024);
            const v4i b0 = *reinterpret_cast<const v4i*>(st + ((4 + 2 * wb) * PC_KS + ks) * 1024);
            const v4i b1 = *reinterpret_cast<const v4i*>(st + ((5 + 2 * wb) * PC_KS + ks) * 1024);
            acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) {
            unsigned char* sn = pc_lds + ((c + 1) & 1) * PC_STAGE + tid * 16;     // (last read in chunk c - 1, before its barrier)
#pragma unroll
            for (int q = 0; q < 8; ++q) *reinterpret_cast<v4i*>(sn + q * (PC_KS * 1024)) = nx[q];
        }
        __syncthreads();
    }
    int* out = second ? a.x1 : a.x11;
    const bool mirror = !second && bb < ab;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
            pair_store_tile(acc[r][c], out, a.m, (int64_t)ab * PC_TILE + (2 * wa + r) * 32, (int64_t)bb * PC_TILE + (2 * wb + c) * 32,
                            lane, mirror);
}

struct PairUpdateArgs {
    const int* r11; const int* r1;
    const int* n_co; const int* o11; const int* o1;
    uint64_t* sum_n11; uint64_t* sumsq_n11; uint64_t* sum_n1;
    uint32_t* cnt[6];                    // n11_ge, n11_gt, agree_ge, agree_gt, or_ge, or_gt
    int64_t* hdr;                        // the block's header: [3] pair_draws, [4] pair_skipped
    int* ctl;                            // [0] the plane of the last counted draw, [1] this draw holds a non-finite g
    int64_t m;
};

__global__ __launch_bounds__(256) void pair_update_kernel(PairUpdateArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = a.ctl[1] != 0;
    if (idx == 0) {                                   // (nobody else in this launch reads ctl[0] or the header)
        if (bad) a.hdr[4] += 1;
        else { a.hdr[3] += 1; a.ctl[0] ^= 1; }
    }
    if (bad || idx >= a.m * a.m) return;
    const int64_t pa = idx / a.m, pb = idx - pa * a.m, tr = pb * a.m + pa;
    const uint64_t nco = (uint64_t)a.n_co[idx];
    if (pa == pb || nco == 0) return;
    const uint64_t r11 = (uint64_t)a.r11[idx], r1 = (uint64_t)a.r1[idx];
    const uint64_t r10 = r1 - r11, r01 = (uint64_t)a.r1[tr] - r11, r00 = nco - r11 - r10 - r01;
    const uint64_t o11 = (uint64_t)a.o11[idx];
    const uint64_t o10 = (uint64_t)a.o1[idx] - o11, o01 = (uint64_t)a.o1[tr] - o11, o00 = nco - o11 - o10 - o01;
    a.sum_n11[idx] += r11;
    a.sumsq_n11[idx] += r11 * r11;
    a.sum_n1[idx] += r1;
    // both sides <= (n + 1)^4 < 2^64 for n <= 65534
    const uint64_t lhs = (2 * r11 + 1) * (2 * r00 + 1) * ((2 * o10 + 1) * (2 * o01 + 1));
    const uint64_t rhs = (2 * o11 + 1) * (2 * o00 + 1) * ((2 * r10 + 1) * (2 * r01 + 1));
    a.cnt[0][idx] += r11 >= o11 ? 1u : 0u;
    a.cnt[1][idx] += r11 > o11 ? 1u : 0u;
    a.cnt[2][idx] += r11 + r00 >= o11 + o00 ? 1u : 0u;
    a.cnt[3][idx] += r11 + r00 > o11 + o00 ? 1u : 0u;
    a.cnt[4][idx] += lhs >= rhs ? 1u : 0u;
    a.cnt[5][idx] += lhs > rhs ? 1u : 0u;
}

int launch_counts(hipStream_t st, const PairState* p, const unsigned char* X8, bool planes, int* x11, int* x1)
{
    PairCountArgs a{};
    a.X8 = X8; a.O8 = p->O8; a.cur = planes ? p->ctl : nullptr; a.skip = planes ? p->ctl + 1 : nullptr;
    a.plane = p->plane; a.ksteps = p->ksteps; a.m = p->m; a.nab = (int)(p->iblocks / 4);
    a.x11 = x11; a.x1 = x1;
    hipLaunchKernelGGL(pair_counts_kernel, dim3((unsigned)a.nab, (unsigned)(x1 ? 2 * a.nab : a.nab)), dim3(256), 2 * PC_STAGE, st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

// a state block on the host
struct HostPairs {
    std::vector<uint64_t> w;
    int64_t n = 0, m = 0;
    PairLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    template <class T> T* arr(int k) { return reinterpret_cast<T*>(w.data() + L.off[k]); }
    template <class T> const T* arr(int k) const { return reinterpret_cast<const T*>(w.data() + L.off[k]); }
};

int pair_read(hipStream_t st, const void* d_state, HostPairs& r, const char* who, int c)
{
    int64_t hdr[PAIR_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[7] != PAIR_TAG || hdr[2] != PAIR_LAYOUT_VERSION || hdr[0] <= 0 || hdr[0] > GPIRT_PAIRS_MAX_N || hdr[1] <= 0 ||
        hdr[3] < 0 || hdr[4] < 0) {
        set_error("%s: state %d is not a pairwise PPC state block of layout %d", who, c, PAIR_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[0]; r.m = hdr[1];
    r.L = pair_layout(r.m);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

// finished field `fld` of the ordered pair (a, b)
double pair_field(const HostPairs& r, int fld, int64_t a, int64_t b)
{
    const int64_t m = r.m, idx = a * m + b, tr = b * m + a, S = r.hdr()[3];
    const double nan = (double)NAN;
    const int64_t nco = r.arr<int32_t>(PAIR_N_CO)[idx];
    if (fld == GPIRT_PAIRS_N_CO) return (double)nco;
    if (a == b || nco == 0) return nan;
    const int64_t o11 = r.arr<int32_t>(PAIR_O11)[idx];
    const int64_t o10 = r.arr<int32_t>(PAIR_O1)[idx] - o11, o01 = r.arr<int32_t>(PAIR_O1)[tr] - o11, o00 = nco - o11 - o10 - o01;
    const uint64_t s11 = r.arr<uint64_t>(PAIR_SUM_N11)[idx], s1ab = r.arr<uint64_t>(PAIR_SUM_N1)[idx], s1ba = r.arr<uint64_t>(PAIR_SUM_N1)[tr];
    auto cnt = [&](int k) { return (double)r.arr<uint32_t>(k)[idx]; };
    const double dS = (double)S;
    switch (fld) {
        case GPIRT_PAIRS_OBS_N11: return (double)o11;
        case GPIRT_PAIRS_OBS_N10: return (double)o10;
        case GPIRT_PAIRS_OBS_N01: return (double)o01;
        case GPIRT_PAIRS_OBS_N00: return (double)o00;
        case GPIRT_PAIRS_AGREE_OBS: return (double)(o11 + o00) / (double)nco;
        case GPIRT_PAIRS_LOG_OR_OBS:
            return std::log((double)((2 * o11 + 1) * (2 * o00 + 1)) / (double)((2 * o10 + 1) * (2 * o01 + 1)));
        default: break;
    }
    if (S < 1) return nan;
    switch (fld) {
        case GPIRT_PAIRS_REP_N11_MEAN: return (double)s11 / dS;
        case GPIRT_PAIRS_REP_N11_VAR: {
            if (S < 2) return nan;
            const unsigned __int128 x = (unsigned __int128)(uint64_t)S * r.arr<uint64_t>(PAIR_SUMSQ_N11)[idx];
            const unsigned __int128 y = (unsigned __int128)s11 * s11;
            return (double)(x - y) / (dS * (double)(S - 1));
        }
        case GPIRT_PAIRS_REP_N10_MEAN: return (double)(s1ab - s11) / dS;
        case GPIRT_PAIRS_REP_N01_MEAN: return (double)(s1ba - s11) / dS;
        case GPIRT_PAIRS_REP_N00_MEAN: return (double)((uint64_t)S * (uint64_t)nco + s11 - s1ab - s1ba) / dS;
        case GPIRT_PAIRS_AGREE_REP_MEAN:
            return (double)((uint64_t)S * (uint64_t)nco + 2 * s11 - s1ab - s1ba) / (double)((uint64_t)S * (uint64_t)nco);
        case GPIRT_PAIRS_PPP_N11: return cnt(PAIR_N11_GE) / dS;
        case GPIRT_PAIRS_PPP_N11_MID: return (cnt(PAIR_N11_GE) + cnt(PAIR_N11_GT)) / (2.0 * dS);
        case GPIRT_PAIRS_PPP_AGREE: return cnt(PAIR_AGREE_GE) / dS;
        case GPIRT_PAIRS_PPP_AGREE_MID: return (cnt(PAIR_AGREE_GE) + cnt(PAIR_AGREE_GT)) / (2.0 * dS);
        case GPIRT_PAIRS_PPP_OR: return cnt(PAIR_OR_GE) / dS;
        case GPIRT_PAIRS_PPP_OR_MID: return (cnt(PAIR_OR_GE) + cnt(PAIR_OR_GT)) / (2.0 * dS);
        default: break;
    }
    return nan;
}

void pair_fill_field(const HostPairs& r, int fld, double* out)
{
    for (int64_t a = 0; a < r.m; ++a)
        for (int64_t b = 0; b < r.m; ++b) out[a * r.m + b] = pair_field(r, fld, a, b);
}

void pair_fill(const HostPairs& r, gpirt_ppc_pairs* out)
{
    const int64_t m = r.m, P = m * m;
    out->n = r.n; out->m = m; out->pair_draws = r.hdr()[3]; out->pair_skipped = r.hdr()[4];
    for (int fld = 0; fld < GPIRT_PAIRS_NFIELDS; ++fld)
        if (out->field[fld]) pair_fill_field(r, fld, out->field[fld]);
    if (out->sum_n11) std::copy_n(r.arr<uint64_t>(PAIR_SUM_N11), P, out->sum_n11);
    if (out->sumsq_n11) std::copy_n(r.arr<uint64_t>(PAIR_SUMSQ_N11), P, out->sumsq_n11);
    if (out->sum_n1) std::copy_n(r.arr<uint64_t>(PAIR_SUM_N1), P, out->sum_n1);
    for (int k = 0; k < 6; ++k)
        if (out->count[k]) std::copy_n(r.arr<uint32_t>(PAIR_N11_GE + k), P, out->count[k]);
    if (!out->extreme_pairs && !out->extreme_ppp_or_mid && !out->extreme_log_or_obs) return;
    // the pairs a < b by decreasing |ppp_or_mid - 0.5|, ties to the lowest (a, b): a stable sort of the pairs in (a, b) order
    struct E { double key, mid; int64_t a, b; };
    std::vector<E> es;
    for (int64_t a = 0; a < m; ++a)
        for (int64_t b = a + 1; b < m; ++b) {
            const double mid = pair_field(r, GPIRT_PAIRS_PPP_OR_MID, a, b);
            if (mid == mid) es.push_back(E{ std::fabs(mid - 0.5), mid, a, b });
        }
    std::stable_sort(es.begin(), es.end(), [](const E& x, const E& y) { return x.key > y.key; });
    for (int t = 0; t < out->top; ++t) {
        const bool have = (size_t)t < es.size();
        if (out->extreme_pairs) {
            out->extreme_pairs[2 * t] = have ? es[(size_t)t].a : -1;
            out->extreme_pairs[2 * t + 1] = have ? es[(size_t)t].b : -1;
        }
        if (out->extreme_ppp_or_mid) out->extreme_ppp_or_mid[t] = have ? es[(size_t)t].mid : (double)NAN;
        if (out->extreme_log_or_obs)
            out->extreme_log_or_obs[t] = have ? pair_field(r, GPIRT_PAIRS_LOG_OR_OBS, es[(size_t)t].a, es[(size_t)t].b) : (double)NAN;
    }
}

}  // namespace

PairLayout pair_layout(int64_t m)
{
    PairLayout L{};
    const int64_t P = m * m;
    int64_t at = PAIR_HEADER_WORDS;
    for (int k = 0; k < PAIR_NARRAYS; ++k) {
        L.off[k] = at;
        const bool wide = k >= PAIR_SUM_N11 && k <= PAIR_SUM_N1;
        at += wide ? (P + 1) / 2 * 2 : (P + 3) / 4 * 2;           // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int64_t pair_state_words(int64_t m) { return pair_layout(m).words; }

void pair_free(PairState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = PairState{};
}

int pair_alloc(hipStream_t st, PairState* p, int64_t n, int64_t m, int64_t item0, const double* y)
{
    if (n > GPIRT_PAIRS_MAX_N) {
        set_error("pairwise PPC: n = %lld is beyond %d respondents (the odds-ratio products would leave 64 bits)", (long long)n,
                  GPIRT_PAIRS_MAX_N);
        return GPIRT_E_ARG;
    }
    const PairLayout L = pair_layout(m);
    p->n = n; p->m = m; p->item0 = item0;
    p->iblocks = (m + PC_TILE - 1) / PC_TILE * (PC_TILE / 32);
    p->ksteps = (n + 255) / 256 * 8;
    p->plane = p->iblocks * p->ksteps * 1024;
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->O8, (size_t)p->plane));
    GP_TRY(get((void**)&p->Y8, (size_t)p->plane));
    GP_TRY(get((void**)&p->rep8, 2 * (size_t)p->plane));          // (the item blocks past the last strip stay zero)
    GP_TRY(get((void**)&p->r11, sizeof(int) * (size_t)(m * m)));
    GP_TRY(get((void**)&p->r1, sizeof(int) * (size_t)(m * m)));
    GP_TRY(get((void**)&p->ctl, sizeof(int) * 4));
    const int64_t hdr[PAIR_HEADER_WORDS] = { n, m, PAIR_LAYOUT_VERSION, 0, 0, item0, 0, PAIR_TAG };
    GP_HIP(hipMemcpyAsync(p->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // hdr is this call's: nothing below may leave with the copy pending
    int64_t blocks = (p->iblocks * p->ksteps * 64 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(pair_bytes_kernel, dim3((unsigned)blocks), dim3(256), 0, st, y, n, m, p->iblocks, p->ksteps,
                       reinterpret_cast<uint4*>(p->O8), reinterpret_cast<uint4*>(p->Y8));
    GP_HIP(hipGetLastError());
    int* tab = reinterpret_cast<int*>(p->block);
    GP_TRY(launch_counts(st, p, p->Y8, false, tab + 2 * L.off[PAIR_O11], tab + 2 * L.off[PAIR_O1]));
    GP_TRY(launch_counts(st, p, p->O8, false, tab + 2 * L.off[PAIR_N_CO], nullptr));
    p->on = true;
    return 0;
}

int launch_pair_accumulate(hipStream_t st, PairState* p)
{
    const PairLayout L = pair_layout(p->m);
    GP_TRY(launch_counts(st, p, p->rep8, true, p->r11, p->r1));
    PairUpdateArgs u{};
    int* tab = reinterpret_cast<int*>(p->block);
    u.r11 = p->r11; u.r1 = p->r1;
    u.n_co = tab + 2 * L.off[PAIR_N_CO]; u.o11 = tab + 2 * L.off[PAIR_O11]; u.o1 = tab + 2 * L.off[PAIR_O1];
    u.sum_n11 = p->block + L.off[PAIR_SUM_N11]; u.sumsq_n11 = p->block + L.off[PAIR_SUMSQ_N11]; u.sum_n1 = p->block + L.off[PAIR_SUM_N1];
    for (int k = 0; k < 6; ++k) u.cnt[k] = reinterpret_cast<uint32_t*>(p->block + L.off[PAIR_N11_GE + k]);
    u.hdr = reinterpret_cast<int64_t*>(p->block); u.ctl = p->ctl; u.m = p->m;
    hipLaunchKernelGGL(pair_update_kernel, dim3((unsigned)((p->m * p->m + 255) / 256)), dim3(256), 0, st, u);
    GP_HIP(hipGetLastError());
    return 0;
}

int pair_get(hipStream_t st, PairState* p, const char* name, void* h_out, int64_t bytes)
{
    const int64_t n = p->n, m = p->m, P = m * m;
    const PairLayout L = pair_layout(m);
    if (strcmp(name, "r11") == 0 || strcmp(name, "r1") == 0) {
        GP_ARG(bytes == 4 * P);
        GP_HIP(hipMemcpyAsync(h_out, name[2] == '1' ? p->r11 : p->r1, (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    if (strcmp(name, "rep") == 0) {               // the plane of the last counted draw, out of the operand layout
        GP_ARG(bytes == n * m);
        int cur = 0;
        GP_HIP(hipMemcpyAsync(&cur, p->ctl, sizeof(int), hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        std::vector<unsigned char> raw((size_t)p->plane);
        GP_HIP(hipMemcpyAsync(raw.data(), p->rep8 + (int64_t)(cur & 1) * p->plane, raw.size(), hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        signed char* out = static_cast<signed char*>(h_out);
        for (int64_t j = 0; j < m; ++j)
            for (int64_t i = 0; i < n; ++i)
                out[i + j * n] = (signed char)raw[(size_t)((((j >> 5) * p->ksteps + (i >> 5)) * 64 + (j & 31) + 32 * ((i & 31) >> 4)) * 16 + (i & 15))];
        return 0;
    }
    if (strcmp(name, "counts") == 0) {
        GP_ARG(bytes == 16);
        GP_HIP(hipMemcpyAsync(h_out, p->block + 3, 16, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    int fld = -1, raw = -1;
    for (int k = 0; k < GPIRT_PAIRS_NFIELDS; ++k) if (strcmp(kPairFields[k], name) == 0) fld = k;
    if (strcmp(name, "sum_n11") == 0) raw = PAIR_SUM_N11;
    if (strcmp(name, "sumsq_n11") == 0) raw = PAIR_SUMSQ_N11;
    if (strcmp(name, "sum_n1") == 0) raw = PAIR_SUM_N1;
    for (int k = 0; k < 6; ++k) if (strcmp(kPairCounts[k], name) == 0) raw = PAIR_N11_GE + k;
    if (fld < 0 && raw < 0) { set_error("unknown pairwise PPC field '%s'", name); return GPIRT_E_ARG; }
    if (raw >= 0) {
        GP_ARG(bytes == (raw <= PAIR_SUM_N1 ? 8 : 4) * P);
        GP_HIP(hipMemcpyAsync(h_out, p->block + L.off[raw], (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    GP_ARG(bytes == 8 * P);
    HostPairs r;
    GP_TRY(pair_read(st, p->block, r, "gpirt_sampler_ppc_pairs_get", 0));
    pair_fill_field(r, fld, static_cast<double*>(h_out));
    return 0;
}

int pair_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_pairs* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved0 == 0 && out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_PAIRS_MAX_TOP) {
        set_error("pairwise PPC: top = %d is outside 1..%d", out->top, GPIRT_PAIRS_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    HostPairs pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostPairs& r = c == 0 ? pooled : one;
        GP_TRY(pair_read(h->stream, d_states[c], r, "gpirt_ppc_pairs_combine", c));
        if (c == 0) continue;
        if (r.n != pooled.n || r.m != pooled.m) {
            set_error("gpirt_ppc_pairs_combine: state %d has another n or m than state 0", c);
            return GPIRT_E_ARG;
        }
        // n_co, o11 and o1 lie side by side
        if (!std::equal(one.w.begin() + one.L.off[PAIR_N_CO], one.w.begin() + one.L.off[PAIR_SUM_N11], pooled.w.begin() + pooled.L.off[PAIR_N_CO])) {
            set_error("gpirt_ppc_pairs_combine: state %d was accumulated on another response matrix than state 0 (n_co, o11 or o1 differ)", c);
            return GPIRT_E_ARG;
        }
        pooled.hdr()[3] += one.hdr()[3];
        pooled.hdr()[4] += one.hdr()[4];
        const int64_t P = r.m * r.m;
        for (int k = PAIR_SUM_N11; k <= PAIR_SUM_N1; ++k)
            for (int64_t g = 0; g < P; ++g) pooled.arr<uint64_t>(k)[g] += one.arr<uint64_t>(k)[g];
        for (int k = PAIR_N11_GE; k <= PAIR_OR_GT; ++k)
            for (int64_t g = 0; g < P; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
    }
    pair_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
