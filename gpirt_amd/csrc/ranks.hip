// ranks.hip -- rank posteriors accumulated on the device, one theta draw at a time (include/gpirt_hip.h, "rank posteriors";
// DESIGN.md section 15).  Every sampled theta is a grid point -5 + 0.01 k (the fact summary.hip's theta histograms rest on),
// so a draw's ranks follow from a 1001-bin count and a prefix sum: less_i = #{k_j < k_i}, eq_i = #{k_j = k_i},
// R2_i = 2 less_i + eq_i + 1 (twice the mid-rank).  A draw with any respondent off the grid (NaN included) is skipped whole.
//
// rank_accumulate_kernel: every work-group counts ALL n indices into 1001 LDS bins (integer LDS atomics: the order of
// arrival cannot change a count), scans them, and then updates the 256 respondents it owns -- one lane per respondent and
// per accumulator row, so there are no global atomics.  The skip decision (any off-grid index) is made from the LDS flag
// before any accumulator is touched, identically in every work-group.  All outputs are integers or per-respondent double
// sums in draw order (pivot_share: one correctly rounded division and one addition per draw), so the launch geometry
// cannot change a bit of the result.  Work-group 0 counts the draw in the block's header and leaves a `valid` word and the
// draw's indices (uint16, zero padded to the counters' leading dimension) for the pairwise pass.
//
// rank_pairwise_kernel: lt[i, j] += (k_i < k_j), one read-modify-write pass over the n x ld uint32 counters per draw
// (ld = n rounded up to 4, so every row starts on 16 bytes).  A work-group of 256 lanes owns 32 rows x 1024 columns: a lane
// keeps its four k_j in registers, the 32 k_i of the strip sit in LDS, and every access is one 16-byte load or store, lanes
// along the contiguous dimension.  The store is UNCONDITIONAL: skipping it where nothing was incremented could save
// traffic only if all 32 counters of a 128-byte line were skipped together, and the respondents are in no order of theta,
// so a line's counters behave like independent coin flips (probability 2^-32 for an interior pair of strips); a per-lane
// branch would cost divergence and save nothing at the memory.  The pass moves at most 8 n ld bytes per draw.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace gpirt {

namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_BINS = 1024;            // 1001 bins, padded to 4 per lane
constexpr int PW_ROWS = 32;              // rows of a pairwise tile
constexpr int PW_COLS = RK_THREADS * 4;  // columns of a pairwise tile: four counters (16 bytes) a lane

struct RankArgs {
    const double* theta;
    int64_t n;
    int64_t B, w, pad;                   // the histogram's bins over R2 (rank_bins)
    int np;
    int piv[GPIRT_RANK_MAX_PIVOTS_CLOSED];
    int64_t* hdr;                        // the block's header: [1] draws, [2] skipped
    uint64_t* sum; uint64_t* sumsq;      // [n]
    double* share; uint32_t* cover;      // [np][n]
    uint32_t* hist;                      // [n][B]
    uint16_t* kidx; uint32_t* ctl;       // the draw's indices and ctl[0] = 1 if the draw counted, for the pairwise pass
};

__global__ __launch_bounds__(RK_THREADS) void rank_accumulate_kernel(RankArgs a)
{
    __shared__ uint32_t cnt[RK_BINS];        // eq: the count of each grid index
    __shared__ uint32_t less[RK_BINS];       // its exclusive prefix sum
    __shared__ uint32_t part[RK_THREADS];
    __shared__ int bad;
    const int t = threadIdx.x;
    for (int b = t; b < RK_BINS; b += RK_THREADS) cnt[b] = 0;
    if (t == 0) bad = 0;
    __syncthreads();
    for (int64_t i = t; i < a.n; i += RK_THREADS) {
        const int k = grid_index(a.theta[i]);
        if (k < 0) bad = 1;                  // several lanes may store here: all store the same 1, and a barrier follows
        else atomicAdd(&cnt[k], 1u);
    }
    __syncthreads();
    if (bad) {                               // decided before any accumulator is touched
        if (blockIdx.x == 0 && t == 0) { a.hdr[2] += 1; a.ctl[0] = 0u; }
        return;
    }
    // exclusive scan: four bins a lane, then the lanes' sums
    const uint32_t c0 = cnt[4 * t], c1 = cnt[4 * t + 1], c2 = cnt[4 * t + 2], c3 = cnt[4 * t + 3];
    part[t] = c0 + c1 + c2 + c3;
    __syncthreads();
    for (int off = 1; off < RK_THREADS; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const uint32_t base = t > 0 ? part[t - 1] : 0u;
    less[4 * t] = base; less[4 * t + 1] = base + c0; less[4 * t + 2] = base + c0 + c1; less[4 * t + 3] = base + c0 + c1 + c2;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * RK_THREADS + t;
    if (i < a.n) {
        const int k = grid_index(a.theta[i]);
        const uint64_t ls = less[k], eq = cnt[k];
        const uint64_t R2 = 2 * ls + eq + 1;
        a.sum[i] += R2;
        a.sumsq[i] += R2 * R2;
        a.hist[i * a.B + ((int64_t)R2 - 2 + a.pad) / a.w] += 1u;
        for (int p = 0; p < a.np; ++p) {
            const uint64_t q = (uint64_t)a.piv[p];
            if (ls < q && q <= ls + eq) {
                a.cover[(int64_t)p * a.n + i] += 1u;
                a.share[(int64_t)p * a.n + i] += 1.0 / (double)eq;
            }
        }
        a.kidx[i] = (uint16_t)k;
    }
    if (blockIdx.x == 0 && t == 0) { a.hdr[1] += 1; a.ctl[0] = 1u; }
}

__global__ __launch_bounds__(RK_THREADS) void rank_pairwise_kernel(const uint16_t* __restrict__ kidx, const uint32_t* __restrict__ ctl,
                                                                   int64_t n, int64_t ld, uint32_t* __restrict__ lt)
{
    __shared__ uint32_t ki[PW_ROWS];
    if (ctl[0] == 0u) return;                // a skipped draw: nothing changes
    const int t = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.y * PW_ROWS;
    const int rows = (int)(n - i0 < PW_ROWS ? n - i0 : PW_ROWS);
    if (t < rows) ki[t] = kidx[i0 + t];
    __syncthreads();
    const int64_t j0 = (int64_t)blockIdx.x * PW_COLS + 4 * t;
    if (j0 >= ld) return;                    // ld is a multiple of 4: j0 .. j0 + 3 < ld; kidx is zero beyond n (k_i < 0 never holds)
    const ushort4 kv = *reinterpret_cast<const ushort4*>(kidx + j0);
    const uint32_t k0 = kv.x, k1 = kv.y, k2 = kv.z, k3 = kv.w;
    uint4* row = reinterpret_cast<uint4*>(lt + i0 * ld + j0);
    const int64_t step = ld / 4;
    auto bump = [&](uint4 v, uint32_t k) {
        v.x += k < k0 ? 1u : 0u; v.y += k < k1 ? 1u : 0u; v.z += k < k2 ? 1u : 0u; v.w += k < k3 ? 1u : 0u;
        return v;
    };
    // four rows at a time, every load issued into a local before the first store: the compiler cannot prove that the rows
    // do not alias, so a load-add-store loop would leave one 16-byte load in flight per lane
    int r = 0;
    for (; r + 4 <= rows; r += 4) {
        const uint4 v0 = row[r * step], v1 = row[(r + 1) * step], v2 = row[(r + 2) * step], v3 = row[(r + 3) * step];
        row[r * step] = bump(v0, ki[r]);
        row[(r + 1) * step] = bump(v1, ki[r + 1]);
        row[(r + 2) * step] = bump(v2, ki[r + 2]);
        row[(r + 3) * step] = bump(v3, ki[r + 3]);
    }
    for (; r < rows; ++r) row[r * step] = bump(row[r * step], ki[r]);
}

struct RankLayout { int64_t sum, sumsq, share, cover, hist, lt, words; };

RankLayout rank_layout(int64_t n, int np, int64_t B, int64_t ld, bool pairwise)
{
    RankLayout L{};
    int64_t at = RANK_HEADER_WORDS;
    L.sum = at; at += n;
    L.sumsq = at; at += n;
    L.share = at; at += (int64_t)np * n;
    L.cover = at; at += ((int64_t)np * n + 1) / 2;
    L.hist = at; at += (n * B + 1) / 2;
    at = (at + 1) & ~(int64_t)1;             // the pairwise counters start on 16 bytes
    L.lt = at;
    if (pairwise) at += n * ld / 2;
    L.words = at;
    return L;
}

int64_t rank_ld(int64_t n) { return (n + 3) & ~(int64_t)3; }

// a state block on the host: the words in front of the pairwise counters, and those counters dense (n x n)
struct HostRank {
    int64_t n = 0, draws = 0, skipped = 0, B = 0, w = 0, pad = 0;
    int np = 0;
    bool pairwise = false;
    RankLayout L{};
    std::vector<uint64_t> words;
    std::vector<uint32_t> lt;
    uint64_t* sum() { return words.data() + L.sum; }
    uint64_t* sumsq() { return words.data() + L.sumsq; }
    double* share() { return reinterpret_cast<double*>(words.data() + L.share); }
    uint32_t* cover() { return reinterpret_cast<uint32_t*>(words.data() + L.cover); }
    uint32_t* hist() { return reinterpret_cast<uint32_t*>(words.data() + L.hist); }
    const int64_t* piv() const { return reinterpret_cast<const int64_t*>(words.data()) + 8; }
};

// the header alone: the counts, the bins, the layout; r.words then holds the RANK_HEADER_WORDS header words only
int rank_read_header(hipStream_t st, const void* d_block, HostRank& r, const char* who, int c)
{
    int64_t hdr[RANK_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_block, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    int64_t B, w, pad;
    const bool plausible = hdr[0] >= 1 && hdr[0] <= GPIRT_RANK_MAX_N && hdr[3] == RANK_LAYOUT_VERSION;
    if (plausible) rank_bins(hdr[0], &B, &w, &pad);
    if (!plausible || hdr[1] < 0 || hdr[2] < 0 || hdr[4] != B || hdr[5] != w || hdr[6] < 1 ||
        hdr[6] > GPIRT_RANK_MAX_PIVOTS_CLOSED || (hdr[7] != 0 && hdr[7] != 1)) {
        set_error("%s: state %d is not a rank state block of layout %d", who, c, RANK_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[0]; r.draws = hdr[1]; r.skipped = hdr[2]; r.B = B; r.w = w; r.pad = pad; r.np = (int)hdr[6];
    r.pairwise = hdr[7] != 0;
    r.L = rank_layout(r.n, r.np, B, rank_ld(r.n), r.pairwise);
    r.words.assign(RANK_HEADER_WORDS, 0);
    memcpy(r.words.data(), hdr, sizeof(hdr));
    r.lt.clear();
    return 0;
}

int rank_read(hipStream_t st, const void* d_block, HostRank& r, bool with_lt, const char* who, int c)
{
    GP_TRY(rank_read_header(st, d_block, r, who, c));
    const int64_t ld = rank_ld(r.n);
    r.words.resize((size_t)r.L.lt);
    GP_HIP(hipMemcpyAsync(r.words.data(), d_block, sizeof(uint64_t) * (size_t)r.L.lt, hipMemcpyDeviceToHost, st));
    r.lt.clear();
    if (with_lt && r.pairwise) {
        r.lt.resize((size_t)(r.n * r.n));
        const char* src = static_cast<const char*>(d_block) + sizeof(uint64_t) * (size_t)r.L.lt;
        GP_HIP(hipMemcpy2DAsync(r.lt.data(), sizeof(uint32_t) * (size_t)r.n, src, sizeof(uint32_t) * (size_t)ld,
                                sizeof(uint32_t) * (size_t)r.n, (size_t)r.n, hipMemcpyDeviceToHost, st));
    }
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

// the theta -> -theta reflection of a chain's accumulators, exactly: R2 -> 2n + 2 - R2, pivot q <-> n + 1 - q, lt -> lt^T
void rank_reflect(HostRank& r)
{
    const int64_t n = r.n;
    const uint64_t S = (uint64_t)r.draws, c = (uint64_t)(2 * n + 2);
    uint64_t *s1 = r.sum(), *s2 = r.sumsq();
    for (int64_t i = 0; i < n; ++i) {
        // sum (c - R2)^2 = S c^2 - 2 c sum R2 + sum R2^2: below 2^64, and exact modulo 2^64 term by term
        const uint64_t a = s1[i];
        s2[i] = S * c * c - 2 * c * a + s2[i];
        s1[i] = S * c - a;
        std::reverse(r.hist() + i * r.B, r.hist() + (i + 1) * r.B);
    }
    for (int p = 0; p < r.np / 2; ++p) {     // the closed set is sorted: position p holds q, np - 1 - p holds n + 1 - q
        const int o = r.np - 1 - p;
        std::swap_ranges(r.share() + (int64_t)p * n, r.share() + (int64_t)(p + 1) * n, r.share() + (int64_t)o * n);
        std::swap_ranges(r.cover() + (int64_t)p * n, r.cover() + (int64_t)(p + 1) * n, r.cover() + (int64_t)o * n);
    }
    if (!r.lt.empty())
        for (int64_t i = 0; i < n; ++i)
            for (int64_t j = i + 1; j < n; ++j) std::swap(r.lt[(size_t)(i * n + j)], r.lt[(size_t)(j * n + i)]);
}

double rank_mean_of(uint64_t s1, int64_t S) { return S >= 1 ? (double)s1 / (2.0 * (double)S) : (double)NAN; }

double rank_var_of(uint64_t s1, uint64_t s2, int64_t S)
{
    if (S < 2) return (double)NAN;
    // S sum R2^2 - (sum R2)^2 >= 0, exact in 128 bits, rounded once
    const unsigned __int128 a = (unsigned __int128)(uint64_t)S * s2;
    const unsigned __int128 b = (unsigned __int128)s1 * s1;
    return (double)(a - b) / (4.0 * (double)S * (double)(S - 1));
}

// the finished values of a (pooled) block; lt moves out last
void rank_fill(HostRank& r, gpirt_ranks* out)
{
    const int64_t n = r.n, S = r.draws;
    out->draws = S; out->skipped = r.skipped; out->B = r.B; out->w = r.w;
    out->rank_bin_width = 0.5 * (double)r.w;
    out->n_pivots = r.np;
    for (int p = 0; p < GPIRT_RANK_MAX_PIVOTS_CLOSED; ++p) out->pivots[p] = p < r.np ? r.piv()[p] : 0;
    for (int64_t i = 0; i < n; ++i) {
        if (out->rank2_sum) out->rank2_sum[i] = r.sum()[i];
        if (out->rank2_sumsq) out->rank2_sumsq[i] = r.sumsq()[i];
        if (out->rank_mean) out->rank_mean[i] = rank_mean_of(r.sum()[i], S);
        if (out->rank_var) out->rank_var[i] = rank_var_of(r.sum()[i], r.sumsq()[i], S);
    }
    if (out->rank_hist) memcpy(out->rank_hist, r.hist(), sizeof(uint32_t) * (size_t)(n * r.B));
    if (out->pivot_cover) memcpy(out->pivot_cover, r.cover(), sizeof(uint32_t) * (size_t)(r.np * n));
    if (out->pivot_share) memcpy(out->pivot_share, r.share(), sizeof(double) * (size_t)(r.np * n));
    if (out->p_pivot)
        for (int64_t k = 0; k < r.np * n; ++k) out->p_pivot[k] = S >= 1 ? r.share()[k] / (double)S : (double)NAN;
    if (out->rank_q)
        for (int p = 0; p < out->nprobs; ++p) {
            // the ceil(q S)-th smallest (the first for q S < 1), as the upper edge of its bin in rank units
            const double want = ceil(out->probs[p] * (double)S);
            const uint64_t need = want < 1.0 ? 1 : (uint64_t)want;
            for (int64_t i = 0; i < n; ++i) {
                double v = (double)NAN;
                if (S >= 1) {
                    const uint32_t* h = r.hist() + i * r.B;
                    uint64_t cum = 0;
                    int64_t b = 0;
                    for (; b < r.B - 1; ++b) { cum += h[b]; if (cum >= need) break; }
                    v = 0.5 * (double)(2 - r.pad + (b + 1) * r.w - 1);
                }
                out->rank_q[(int64_t)p * n + i] = v;
            }
        }
    if (out->lt && !r.lt.empty()) memcpy(out->lt, r.lt.data(), sizeof(uint32_t) * r.lt.size());
}

}  // namespace

void rank_bins(int64_t n, int64_t* B, int64_t* w, int64_t* pad)
{
    const int64_t span = 2 * n - 1;          // R2 runs over 2 .. 2n
    int64_t ww = 1;
    while ((span + ww - 1) / ww > 1025) ww += 2;
    int64_t b = (span + ww - 1) / ww;
    if (b % 2 == 0) b += 1;                  // B odd and w odd: B w - span is even, the padding splits evenly
    *B = b; *w = ww; *pad = (b * ww - span) / 2;
}

int rank_close_pivots(int64_t n, const int64_t* pivots, int n_pivots, int64_t* closed)
{
    std::vector<int64_t> q;
    if (n_pivots == 0) {                     // "median"
        q.push_back((n + 1) / 2);
        q.push_back(n + 1 - (n + 1) / 2);
    }
    for (int p = 0; p < n_pivots; ++p) { q.push_back(pivots[p]); q.push_back(n + 1 - pivots[p]); }
    std::sort(q.begin(), q.end());
    q.erase(std::unique(q.begin(), q.end()), q.end());
    for (size_t p = 0; p < q.size(); ++p) closed[p] = q[p];
    return (int)q.size();
}

int64_t rank_state_words(const RankState* s)
{
    return rank_layout(s->n, s->np, s->B, s->ld, s->pairwise).words;
}

int rank_alloc(hipStream_t st, RankState* s, int64_t n, const int64_t* pivots, int n_pivots, int pairwise)
{
    if (n > GPIRT_RANK_MAX_N) {
        set_error("rank posteriors: n = %lld is beyond %d respondents", (long long)n, GPIRT_RANK_MAX_N);
        return GPIRT_E_ARG;
    }
    if (n_pivots < 0 || n_pivots > GPIRT_RANK_MAX_PIVOTS || (n_pivots > 0 && !pivots)) {
        set_error("rank posteriors: %d pivots given, at most %d are taken", n_pivots, GPIRT_RANK_MAX_PIVOTS);
        return GPIRT_E_ARG;
    }
    for (int p = 0; p < n_pivots; ++p)
        if (pivots[p] < 1 || pivots[p] > n) {
            set_error("rank posteriors: pivot %lld is outside 1..%lld", (long long)pivots[p], (long long)n);
            return GPIRT_E_ARG;
        }
    s->n = n; s->pairwise = pairwise != 0; s->ld = rank_ld(n);
    rank_bins(n, &s->B, &s->w, &s->pad);
    s->np = rank_close_pivots(n, pivots, n_pivots, s->piv);
    const RankLayout L = rank_layout(n, s->np, s->B, s->ld, s->pairwise);
    auto get = [&](void** p, size_t bytes) -> int {
        GP_HIP(hipMalloc(p, bytes));
        s->allocs.push_back(*p);
        GP_HIP(hipMemsetAsync(*p, 0, bytes, st));
        return 0;
    };
    GP_TRY(get((void**)&s->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&s->kidx, sizeof(uint16_t) * (size_t)(s->ld + 8)));
    GP_TRY(get((void**)&s->ctl, 16));
    int64_t hdr[RANK_HEADER_WORDS] = { n, 0, 0, RANK_LAYOUT_VERSION, s->B, s->w, s->np, s->pairwise ? 1 : 0 };
    for (int p = 0; p < s->np; ++p) hdr[8 + p] = s->piv[p];
    GP_HIP(hipMemcpyAsync(s->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // hdr is on this stack
    s->on = true;
    return 0;
}

void rank_free(RankState* s)
{
    for (void* p : s->allocs) hipFree(p);
    *s = RankState{};
}

int launch_rank_accumulate(hipStream_t st, RankState* s, const double* theta)
{
    const RankLayout L = rank_layout(s->n, s->np, s->B, s->ld, s->pairwise);
    uint64_t* blk = s->block;
    RankArgs a{};
    a.theta = theta; a.n = s->n; a.B = s->B; a.w = s->w; a.pad = s->pad; a.np = s->np;
    for (int p = 0; p < s->np; ++p) a.piv[p] = (int)s->piv[p];
    a.hdr = reinterpret_cast<int64_t*>(blk);
    a.sum = blk + L.sum; a.sumsq = blk + L.sumsq;
    a.share = reinterpret_cast<double*>(blk + L.share);
    a.cover = reinterpret_cast<uint32_t*>(blk + L.cover);
    a.hist = reinterpret_cast<uint32_t*>(blk + L.hist);
    a.kidx = s->kidx; a.ctl = s->ctl;
    hipLaunchKernelGGL(rank_accumulate_kernel, dim3((unsigned)((s->n + RK_THREADS - 1) / RK_THREADS)), dim3(RK_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    if (s->pairwise) {
        const dim3 grid((unsigned)((s->ld + PW_COLS - 1) / PW_COLS), (unsigned)((s->n + PW_ROWS - 1) / PW_ROWS));
        hipLaunchKernelGGL(rank_pairwise_kernel, grid, dim3(RK_THREADS), 0, st, s->kidx, s->ctl, s->n, s->ld,
                           reinterpret_cast<uint32_t*>(blk + L.lt));
        GP_HIP(hipGetLastError());
    }
    return 0;
}

int rank_get(hipStream_t st, RankState* s, const char* name, void* h_out, int64_t bytes)
{
    // the header, then only the array asked for (the histogram alone is n B words: 32 MB at 8192)
    HostRank r;
    GP_TRY(rank_read_header(st, s->block, r, "gpirt_sampler_rank_get", 0));
    const int64_t n = r.n, P = r.np, S = r.draws, ld = rank_ld(n);
    const char* blk = reinterpret_cast<const char*>(s->block);
    auto fetch = [&](void* dst, int64_t word, int64_t nbytes) -> int {
        GP_HIP(hipMemcpyAsync(dst, blk + 8 * word, (size_t)nbytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) {
        GP_ARG(bytes == 8 * 5);
        int64_t* c = static_cast<int64_t*>(h_out);
        c[0] = r.draws; c[1] = r.skipped; c[2] = r.B; c[3] = r.w; c[4] = r.np;
        return 0;
    }
    if (strcmp(name, "pivots") == 0) {
        GP_ARG(bytes == 8 * P);
        memcpy(h_out, r.piv(), (size_t)bytes);
        return 0;
    }
    if (strcmp(name, "lt") == 0) {
        if (!r.pairwise) { set_error("rank posteriors: the pairwise counters are not enabled"); return GPIRT_E_ARG; }
        GP_ARG(bytes == 4 * n * n);
        GP_HIP(hipMemcpy2DAsync(h_out, sizeof(uint32_t) * (size_t)n, blk + 8 * r.L.lt, sizeof(uint32_t) * (size_t)ld,
                                sizeof(uint32_t) * (size_t)n, (size_t)n, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const struct { const char* name; int64_t word, bytes; } raw[] = {
        { "rank2_sum", r.L.sum, 8 * n }, { "rank2_sumsq", r.L.sumsq, 8 * n }, { "rank_hist", r.L.hist, 4 * n * r.B },
        { "pivot_cover", r.L.cover, 4 * P * n }, { "pivot_share", r.L.share, 8 * P * n },
    };
    for (const auto& e : raw)
        if (strcmp(e.name, name) == 0) {
            GP_ARG(bytes == e.bytes);
            return fetch(h_out, e.word, e.bytes);
        }
    double* out = static_cast<double*>(h_out);
    if (strcmp(name, "rank_mean") == 0 || strcmp(name, "rank_var") == 0) {
        GP_ARG(bytes == 8 * n);
        std::vector<uint64_t> s12((size_t)(2 * n));              // rank2_sum and rank2_sumsq lie side by side
        GP_TRY(fetch(s12.data(), r.L.sum, 16 * n));
        const bool mean = name[5] == 'm';
        for (int64_t i = 0; i < n; ++i)
            out[i] = mean ? rank_mean_of(s12[(size_t)i], S) : rank_var_of(s12[(size_t)i], s12[(size_t)(n + i)], S);
        return 0;
    }
    if (strcmp(name, "p_pivot") == 0) {
        GP_ARG(bytes == 8 * P * n);
        GP_TRY(fetch(out, r.L.share, 8 * P * n));
        for (int64_t k = 0; k < P * n; ++k) out[k] = S >= 1 ? out[k] / (double)S : (double)NAN;
        return 0;
    }
    set_error("unknown rank field '%s'", name);
    return GPIRT_E_ARG;
}

int rank_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ranks* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    GP_ARG(out->nprobs >= 0 && (out->nprobs == 0 || out->probs));
    for (int p = 0; p < out->nprobs; ++p) GP_ARG(out->probs[p] >= 0.0 && out->probs[p] <= 1.0);
    for (int c = 0; c < chains; ++c) {
        GP_ARG(d_states[c]);
        if (signs) GP_ARG(signs[c] == 1 || signs[c] == -1);
    }
    HostRank pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostRank& r = c == 0 ? pooled : one;
        GP_TRY(rank_read(h->stream, d_states[c], r, out->lt != nullptr, "gpirt_rank_combine", c));
        if (out->lt && !r.pairwise) {
            set_error("gpirt_rank_combine: state %d holds no pairwise counters", c);
            return GPIRT_E_ARG;
        }
        if (c > 0 && (r.n != pooled.n || r.np != pooled.np || memcmp(r.piv(), pooled.piv(), sizeof(int64_t) * (size_t)r.np) != 0)) {
            set_error("gpirt_rank_combine: state %d has another n or other pivots than state 0", c);
            return GPIRT_E_ARG;
        }
        if (signs && signs[c] < 0) rank_reflect(r);
        if (c == 0) continue;
        const int64_t n = pooled.n;
        for (int64_t i = 0; i < n; ++i) { pooled.sum()[i] += one.sum()[i]; pooled.sumsq()[i] += one.sumsq()[i]; }
        for (int64_t k = 0; k < n * pooled.B; ++k) pooled.hist()[k] += one.hist()[k];
        for (int64_t k = 0; k < pooled.np * n; ++k) {
            pooled.cover()[k] += one.cover()[k];
            pooled.share()[k] += one.share()[k];               // the shares, in chain order
        }
        for (size_t k = 0; k < pooled.lt.size(); ++k) pooled.lt[k] += one.lt[k];
        pooled.draws += one.draws;
        pooled.skipped += one.skipped;
    }
    rank_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
