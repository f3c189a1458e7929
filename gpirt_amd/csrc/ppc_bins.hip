// ppc_bins.hip -- theta-binned item fit of the posterior predictive checks (include/gpirt_hip.h, "theta-binned item fit";
// DESIGN.md section 19): per draw the respondents are grouped by the bin of their theta, and per (bin, item) the yes answers of
// the data (T) and of the replicate (R) are compared with each other and with what the model expects there (E, V) -- the
// empirical item response function and a chi-square per item, accumulated one draw at a time without stored draws.
//
// bin_assign_kernel (one work-group): the bin of every respondent from theta's grid index, n_b (integer LDS atomics: the order
// of arrival cannot change a count) and the word that tells of a theta off the grid.
// ppc_replicate_kernel<*, true> (ppc.hip): the ONE pass over the n x m cells -- f, mu and y are read once, for the PPC, the
// pairs and the bins together -- leaves N, T, R, E, V per (block of 256 respondents, item, bin).
// bin_update_kernel: 32 lanes per item, lane b owns bin b.  It adds the row blocks' partial tables in block order, keeps the
// cell's accumulators, and the item's X2(T) and X2(R) are summed over the lanes in increasing b by every lane alike.  Each
// accumulator word is owned by one lane: no global atomics, bit-identical from run to run.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <strings.h>

namespace gpirt {

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_ITEMS = BN_THREADS / 32;         // items per work-group of bin_update_kernel
constexpr int BN_CENTRE = (GPIRT_NGRID - 1) / 2;  // the grid index of theta = 0
static_assert(GPIRT_BINS_MAX_B <= 32, "one lane of a 32-lane group per bin");

const char* const kBinCell[GPIRT_BINS_CELL_NFIELDS] = { "obs_rate", "rep_rate", "exp_rate", "z_mean", "ppp_cell", "ppp_cell_mid", "n_mean" };
const char* const kBinItem[GPIRT_BINS_ITEM_NFIELDS] = { "ppp_chi2", "ppp_chi2_mid", "chi2_obs_mean", "chi2_rep_mean" };
const char* const kBinBin[GPIRT_BINS_BIN_NFIELDS] = { "occupancy", "bin_lo", "bin_hi" };
const char* const kBinRaw[BIN_NARRAYS] = { "sum_n", "sum_t", "sum_r", "sum_e", "sum_z", "cell_ge", "cell_gt", "cell_empty",
                                           "chi_ge", "chi_gt", "chi_obs_sum", "chi_rep_sum", "occ_sum" };

struct BinCuts { int h; int d[GPIRT_BINS_MAX_H]; };

// bytes per element and elements of raw array k
inline int bin_raw_width(int k) { return (k >= BIN_CELL_GE && k <= BIN_CHI_GT) ? 4 : 8; }
inline int64_t bin_raw_count(int k, int64_t m, int64_t B) { return k <= BIN_CELL_EMPTY ? B * m : k == BIN_OCC ? B : m; }

__global__ __launch_bounds__(BN_THREADS) void bin_assign_kernel(const double* __restrict__ theta, int64_t n, BinCuts c,
                                                                unsigned char* __restrict__ bin, uint32_t* __restrict__ nb,
                                                                int* __restrict__ ctl)
{
    __shared__ uint32_t cnt[32];
    __shared__ int bad;
    const int t = threadIdx.x;
    if (t < 32) cnt[t] = 0;
    if (t == 0) bad = 0;
    __syncthreads();
    for (int64_t i = t; i < n; i += BN_THREADS) {
        const int k = grid_index(theta[i]);
        unsigned char b = BIN_NONE;
        if (k < 0) bad = 1;                  // several lanes may store here: all store the same 1, and a barrier follows
        else {
            const int a = k >= BN_CENTRE ? k - BN_CENTRE : BN_CENTRE - k;
            int l = 0;
            for (int q = 0; q < c.h; ++q) l += a >= c.d[q] ? 1 : 0;
            b = (unsigned char)(k >= BN_CENTRE ? c.h + l : c.h - l);
            atomicAdd(&cnt[b], 1u);
        }
        bin[i] = b;
    }
    __syncthreads();
    if (t < 32) nb[t] = cnt[t];
    if (t == 0) { ctl[0] = bad; ctl[1] = 0; }
}

struct BinUpdateArgs {
    const uint32_t* part_i; const double* part_e; const double* part_v;      // [row block][m][B]
    int rblocks, B;
    int64_t n, m;
    const int* ctl; const uint32_t* nb;
    const unsigned char* bin_cur; unsigned char* bin_last;
    int32_t* tab_i; double* tab_d;                    // the last counted draw's tables
    int64_t* hdr;                                     // the block's header: [3] bin_draws, [4] bin_skipped
    uint64_t* sum_n; uint64_t* sum_t; uint64_t* sum_r; double* sum_e; double* sum_z;
    uint32_t* cell_ge; uint32_t* cell_gt; uint32_t* cell_empty;
    uint32_t* chi_ge; uint32_t* chi_gt; double* chi_obs; double* chi_rep;
    uint64_t* occ;
};

__global__ __launch_bounds__(BN_THREADS) void bin_update_kernel(BinUpdateArgs a)
{
    const int t = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * BN_THREADS + t;
    const bool skip = a.ctl[0] != 0 || a.ctl[1] != 0;
    if (gid == 0) a.hdr[skip ? 4 : 3] += 1;           // (nobody else in this launch reads the header)
    if (skip) return;
    for (int64_t i = gid; i < a.n; i += (int64_t)gridDim.x * BN_THREADS) a.bin_last[i] = a.bin_cur[i];
    if (gid < a.B) a.occ[gid] += a.nb[gid];
    const int b = t & 31;
    const int64_t j = (int64_t)blockIdx.x * BN_ITEMS + (t >> 5);
    const bool have = j < a.m && b < a.B;
    uint32_t N = 0, T = 0, R = 0;
    double E = 0.0, V = 0.0;
    if (have)
        for (int rb = 0; rb < a.rblocks; ++rb) {
            const int64_t at = ((int64_t)rb * a.m + j) * a.B + b;
            const uint32_t pk = a.part_i[at];
            N += pk & 1023u; T += (pk >> 10) & 1023u; R += (pk >> 20) & 1023u;
            E += a.part_e[at]; V += a.part_v[at];
        }
    double termT = 0.0, termR = 0.0;
    int same = 1;
    if (have) {
        const int64_t C = (int64_t)a.B * a.m, at = (int64_t)b * a.m + j;
        a.tab_i[at] = (int32_t)N; a.tab_i[C + at] = (int32_t)T; a.tab_i[2 * C + at] = (int32_t)R;
        a.tab_d[at] = E; a.tab_d[C + at] = V;
        if (N == 0) a.cell_empty[at] += 1u;
        else {
            a.cell_ge[at] += R >= T ? 1u : 0u;
            a.cell_gt[at] += R > T ? 1u : 0u;
            a.sum_n[at] += N; a.sum_t[at] += T; a.sum_r[at] += R;
            a.sum_e[at] += E;
            same = R == T ? 1 : 0;
            if (V > 0.0) {
                const double dT = (double)T - E, dR = (double)R - E;
                a.sum_z[at] += dT / sqrt(V);
                termT = dT * dT / V;
                termR = dR * dR / V;
            }
        }
    }
    // the item's chi-squares: the bins' terms in increasing b (a bin that does not enter holds 0), by every lane of the group
    double x2T = 0.0, x2R = 0.0;
    int all_same = 1;
    for (int q = 0; q < a.B; ++q) {
        x2T += __shfl(termT, q, 32);
        x2R += __shfl(termR, q, 32);
        all_same &= __shfl(same, q, 32);
    }
    if (have && b == 0) {
        a.chi_ge[j] += (all_same || x2R >= x2T) ? 1u : 0u;
        a.chi_gt[j] += (!all_same && x2R > x2T) ? 1u : 0u;
        a.chi_obs[j] += x2T;
        a.chi_rep[j] += x2R;
    }
}

// a state block on the host
struct HostBins {
    std::vector<uint64_t> w;
    int64_t n = 0, m = 0, B = 0, item0 = 0;
    int h = 0;
    BinLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    const int64_t* cuts() const { return hdr() + BIN_HEADER_WORDS; }
    template <class T> T* arr(int k) { return reinterpret_cast<T*>(w.data() + L.off[k]); }
    template <class T> const T* arr(int k) const { return reinterpret_cast<const T*>(w.data() + L.off[k]); }
};

int bin_read(hipStream_t st, const void* d_state, HostBins& r, const char* who, int c)
{
    int64_t hdr[BIN_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[7] != BIN_TAG || hdr[2] != BIN_LAYOUT_VERSION || hdr[0] <= 0 || hdr[1] <= 0 || hdr[3] < 0 || hdr[4] < 0 ||
        hdr[6] < 3 || hdr[6] > GPIRT_BINS_MAX_B || hdr[6] % 2 == 0) {
        set_error("%s: state %d is not a theta-binned PPC state block of layout %d", who, c, BIN_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[0]; r.m = hdr[1]; r.item0 = hdr[5]; r.B = hdr[6]; r.h = (int)((hdr[6] - 1) / 2);
    r.L = bin_layout(r.m, r.B);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

double bin_cell_field(const HostBins& r, int fld, int64_t at)
{
    const double nan = (double)NAN;
    const int64_t S = r.hdr()[3];
    const uint64_t sN = r.arr<uint64_t>(BIN_SUM_N)[at];
    const int64_t Sc = S - (int64_t)r.arr<uint32_t>(BIN_CELL_EMPTY)[at];      // the draws in which the cell held someone
    switch (fld) {
        case GPIRT_BINS_CELL_OBS_RATE: return sN ? (double)r.arr<uint64_t>(BIN_SUM_T)[at] / (double)sN : nan;
        case GPIRT_BINS_CELL_REP_RATE: return sN ? (double)r.arr<uint64_t>(BIN_SUM_R)[at] / (double)sN : nan;
        case GPIRT_BINS_CELL_EXP_RATE: return sN ? r.arr<double>(BIN_SUM_E)[at] / (double)sN : nan;
        case GPIRT_BINS_CELL_Z_MEAN: return Sc > 0 ? r.arr<double>(BIN_SUM_Z)[at] / (double)Sc : nan;
        case GPIRT_BINS_CELL_PPP_CELL: return Sc > 0 ? (double)r.arr<uint32_t>(BIN_CELL_GE)[at] / (double)Sc : nan;
        case GPIRT_BINS_CELL_PPP_CELL_MID:
            return Sc > 0 ? ((double)r.arr<uint32_t>(BIN_CELL_GE)[at] + (double)r.arr<uint32_t>(BIN_CELL_GT)[at]) / (2.0 * (double)Sc) : nan;
        case GPIRT_BINS_CELL_N_MEAN: return S > 0 ? (double)sN / (double)S : nan;
        default: break;
    }
    return nan;
}

double bin_item_field(const HostBins& r, int fld, int64_t j)
{
    const int64_t S = r.hdr()[3];
    if (S < 1) return (double)NAN;
    const double dS = (double)S;
    switch (fld) {
        case GPIRT_BINS_ITEM_PPP_CHI2: return (double)r.arr<uint32_t>(BIN_CHI_GE)[j] / dS;
        case GPIRT_BINS_ITEM_PPP_CHI2_MID: return ((double)r.arr<uint32_t>(BIN_CHI_GE)[j] + (double)r.arr<uint32_t>(BIN_CHI_GT)[j]) / (2.0 * dS);
        case GPIRT_BINS_ITEM_CHI2_OBS_MEAN: return r.arr<double>(BIN_CHI_OBS)[j] / dS;
        case GPIRT_BINS_ITEM_CHI2_REP_MEAN: return r.arr<double>(BIN_CHI_REP)[j] / dS;
        default: break;
    }
    return (double)NAN;
}

// the edge of bin b towards -inf (hi = false) or +inf, in theta
double bin_edge(const HostBins& r, int64_t b, bool hi)
{
    const int64_t h = r.h;
    auto cut = [&](int64_t l) { return l > h ? 5.0 : (double)r.cuts()[l - 1] / 100.0; };     // l = 1 .. h + 1
    if (b == h) return hi ? cut(1) : -cut(1);
    if (b > h) return hi ? cut(b - h + 1) : cut(b - h);
    return hi ? -cut(h - b) : -cut(h - b + 1);
}

double bin_bin_field(const HostBins& r, int fld, int64_t b)
{
    const int64_t S = r.hdr()[3];
    switch (fld) {
        case GPIRT_BINS_BIN_OCCUPANCY: return S > 0 ? (double)r.arr<uint64_t>(BIN_OCC)[b] / (double)S : (double)NAN;
        case GPIRT_BINS_BIN_LO: return bin_edge(r, b, false);
        case GPIRT_BINS_BIN_HI: return bin_edge(r, b, true);
        default: break;
    }
    return (double)NAN;
}

void bin_fill(const HostBins& r, gpirt_ppc_bins* out)
{
    const int64_t m = r.m, B = r.B, C = B * m;
    out->n = r.n; out->m = m; out->B = B; out->bin_draws = r.hdr()[3]; out->bin_skipped = r.hdr()[4];
    out->h = r.h;
    for (int q = 0; q <= GPIRT_BINS_MAX_H; ++q) out->cuts[q] = q < r.h ? (int)r.cuts()[q] : 0;
    for (int fld = 0; fld < GPIRT_BINS_CELL_NFIELDS; ++fld)
        if (out->cell[fld]) for (int64_t at = 0; at < C; ++at) out->cell[fld][at] = bin_cell_field(r, fld, at);
    for (int fld = 0; fld < GPIRT_BINS_ITEM_NFIELDS; ++fld)
        if (out->item[fld]) for (int64_t j = 0; j < m; ++j) out->item[fld][j] = bin_item_field(r, fld, j);
    for (int fld = 0; fld < GPIRT_BINS_BIN_NFIELDS; ++fld)
        if (out->bin[fld]) for (int64_t b = 0; b < B; ++b) out->bin[fld][b] = bin_bin_field(r, fld, b);
    if (out->sum_n) std::copy_n(r.arr<uint64_t>(BIN_SUM_N), C, out->sum_n);
    if (out->sum_t) std::copy_n(r.arr<uint64_t>(BIN_SUM_T), C, out->sum_t);
    if (out->sum_r) std::copy_n(r.arr<uint64_t>(BIN_SUM_R), C, out->sum_r);
    if (out->sum_e) std::copy_n(r.arr<double>(BIN_SUM_E), C, out->sum_e);
    if (out->sum_z) std::copy_n(r.arr<double>(BIN_SUM_Z), C, out->sum_z);
    for (int k = 0; k < 3; ++k)
        if (out->cell_count[k]) std::copy_n(r.arr<uint32_t>(BIN_CELL_GE + k), C, out->cell_count[k]);
    for (int k = 0; k < 2; ++k)
        if (out->chi_count[k]) std::copy_n(r.arr<uint32_t>(BIN_CHI_GE + k), m, out->chi_count[k]);
    if (out->chi_obs_sum) std::copy_n(r.arr<double>(BIN_CHI_OBS), m, out->chi_obs_sum);
    if (out->chi_rep_sum) std::copy_n(r.arr<double>(BIN_CHI_REP), m, out->chi_rep_sum);
    if (out->occ_sum) std::copy_n(r.arr<uint64_t>(BIN_OCC), B, out->occ_sum);
    if (!out->worst_items && !out->worst_ppp_chi2_mid && !out->worst_chi2_obs_mean) return;
    // the items by increasing ppp_chi2_mid, ties to the lowest j: a stable sort of the items in order
    struct E { double mid; int64_t j; };
    std::vector<E> es;
    for (int64_t j = 0; j < m; ++j) {
        const double mid = bin_item_field(r, GPIRT_BINS_ITEM_PPP_CHI2_MID, j);
        if (mid == mid) es.push_back(E{ mid, j });
    }
    std::stable_sort(es.begin(), es.end(), [](const E& x, const E& y) { return x.mid < y.mid; });
    for (int t = 0; t < out->top; ++t) {
        const bool have = (size_t)t < es.size();
        if (out->worst_items) out->worst_items[t] = have ? es[(size_t)t].j : -1;
        if (out->worst_ppp_chi2_mid) out->worst_ppp_chi2_mid[t] = have ? es[(size_t)t].mid : (double)NAN;
        if (out->worst_chi2_obs_mean)
            out->worst_chi2_obs_mean[t] = have ? bin_item_field(r, GPIRT_BINS_ITEM_CHI2_OBS_MEAN, es[(size_t)t].j) : (double)NAN;
    }
}

// theta -> -theta: cell (b, j) becomes (B - 1 - b, j), and so does occ_sum
void bin_reflect(HostBins& r)
{
    const int64_t m = r.m, B = r.B;
    auto rows = [&](auto* p, int64_t width) {
        for (int64_t b = 0; b < B / 2; ++b) std::swap_ranges(p + b * width, p + (b + 1) * width, p + (B - 1 - b) * width);
    };
    for (int k = BIN_SUM_N; k <= BIN_SUM_R; ++k) rows(r.arr<uint64_t>(k), m);
    for (int k = BIN_SUM_E; k <= BIN_SUM_Z; ++k) rows(r.arr<double>(k), m);
    for (int k = BIN_CELL_GE; k <= BIN_CELL_EMPTY; ++k) rows(r.arr<uint32_t>(k), m);
    rows(r.arr<uint64_t>(BIN_OCC), 1);
}

}  // namespace

BinLayout bin_layout(int64_t m, int64_t B)
{
    BinLayout L{};
    int64_t at = BIN_HEADER_WORDS + BIN_CUT_WORDS;
    for (int k = 0; k < BIN_NARRAYS; ++k) {
        L.off[k] = at;
        const int64_t bytes = bin_raw_count(k, m, B) * bin_raw_width(k);
        at += (bytes + 15) / 16 * 2;                                  // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int64_t bin_state_words(int64_t m, int64_t B) { return bin_layout(m, B).words; }

int bin_check_cuts(int h, const int* cuts)
{
    if (h < 1 || h > GPIRT_BINS_MAX_H || !cuts) {
        set_error("theta-binned PPC: %d cuts given, 1..%d are taken", h, GPIRT_BINS_MAX_H);
        return GPIRT_E_ARG;
    }
    for (int q = 0; q < h; ++q)
        if (cuts[q] < 1 || cuts[q] > BN_CENTRE - 1 || (q > 0 && cuts[q] <= cuts[q - 1])) {
            set_error("theta-binned PPC: the cuts must be increasing integers in 1..%d (hundredths of theta)", BN_CENTRE - 1);
            return GPIRT_E_ARG;
        }
    return 0;
}

void bin_free(BinState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = BinState{};
}

int bin_alloc(hipStream_t st, BinState* p, int64_t n, int64_t m, int64_t item0, int rblocks, int h, const int* cuts)
{
    GP_TRY(bin_check_cuts(h, cuts));
    const int64_t B = 2 * h + 1, C = B * m;
    const BinLayout L = bin_layout(m, B);
    p->n = n; p->m = m; p->item0 = item0; p->h = h; p->B = (int)B; p->rblocks = rblocks;
    for (int q = 0; q < h; ++q) p->cuts[q] = cuts[q];
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    const size_t parts = (size_t)rblocks * (size_t)C;
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->bin_cur, (size_t)n));
    GP_TRY(get((void**)&p->bin_last, (size_t)n));
    GP_TRY(get((void**)&p->nb, sizeof(uint32_t) * 32));
    GP_TRY(get((void**)&p->ctl, sizeof(int) * 4));
    GP_TRY(get((void**)&p->part_i, sizeof(uint32_t) * parts));
    GP_TRY(get((void**)&p->part_e, sizeof(double) * parts));
    GP_TRY(get((void**)&p->part_v, sizeof(double) * parts));
    GP_TRY(get((void**)&p->tab_i, sizeof(int32_t) * 3 * (size_t)C));
    GP_TRY(get((void**)&p->tab_d, sizeof(double) * 2 * (size_t)C));
    int64_t hdr[BIN_HEADER_WORDS + BIN_CUT_WORDS] = { n, m, BIN_LAYOUT_VERSION, 0, 0, item0, B, BIN_TAG };
    for (int q = 0; q < h; ++q) hdr[BIN_HEADER_WORDS + q] = cuts[q];
    GP_HIP(hipMemcpyAsync(p->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // hdr is this call's: nothing below may leave with the copy pending
    p->on = true;
    return 0;
}

int launch_bin_assign(hipStream_t st, BinState* p, const double* theta)
{
    BinCuts c{};
    c.h = p->h;
    for (int q = 0; q < p->h; ++q) c.d[q] = p->cuts[q];
    hipLaunchKernelGGL(bin_assign_kernel, dim3(1), dim3(BN_THREADS), 0, st, theta, p->n, c, p->bin_cur, p->nb, p->ctl);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_bin_update(hipStream_t st, BinState* p)
{
    const BinLayout L = bin_layout(p->m, p->B);
    BinUpdateArgs a{};
    a.part_i = p->part_i; a.part_e = p->part_e; a.part_v = p->part_v;
    a.rblocks = p->rblocks; a.B = p->B; a.n = p->n; a.m = p->m;
    a.ctl = p->ctl; a.nb = p->nb; a.bin_cur = p->bin_cur; a.bin_last = p->bin_last;
    a.tab_i = p->tab_i; a.tab_d = p->tab_d;
    a.hdr = reinterpret_cast<int64_t*>(p->block);
    auto at = [&](int k) { return p->block + L.off[k]; };
    a.sum_n = at(BIN_SUM_N); a.sum_t = at(BIN_SUM_T); a.sum_r = at(BIN_SUM_R);
    a.sum_e = reinterpret_cast<double*>(at(BIN_SUM_E)); a.sum_z = reinterpret_cast<double*>(at(BIN_SUM_Z));
    a.cell_ge = reinterpret_cast<uint32_t*>(at(BIN_CELL_GE)); a.cell_gt = reinterpret_cast<uint32_t*>(at(BIN_CELL_GT));
    a.cell_empty = reinterpret_cast<uint32_t*>(at(BIN_CELL_EMPTY));
    a.chi_ge = reinterpret_cast<uint32_t*>(at(BIN_CHI_GE)); a.chi_gt = reinterpret_cast<uint32_t*>(at(BIN_CHI_GT));
    a.chi_obs = reinterpret_cast<double*>(at(BIN_CHI_OBS)); a.chi_rep = reinterpret_cast<double*>(at(BIN_CHI_REP));
    a.occ = at(BIN_OCC);
    hipLaunchKernelGGL(bin_update_kernel, dim3((unsigned)((p->m + BN_ITEMS - 1) / BN_ITEMS)), dim3(BN_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

int bin_get(hipStream_t st, BinState* p, const char* name, void* h_out, int64_t bytes)
{
    const int64_t n = p->n, m = p->m, B = p->B, C = B * m;
    const BinLayout L = bin_layout(m, B);
    auto copy = [&](const void* src) -> int {
        GP_HIP(hipMemcpyAsync(h_out, src, (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 16); return copy(p->block + 3); }
    if (strcmp(name, "cuts") == 0) { GP_ARG(bytes == 8 * p->h); return copy(p->block + BIN_HEADER_WORDS); }
    if (strcmp(name, "bin") == 0) { GP_ARG(bytes == n); return copy(p->bin_last); }
    if (strlen(name) == 2 && name[0] == 't') {                        // the last counted draw's tables
        const char* ints = "NTR";
        if (const char* q = strchr(ints, name[1])) { GP_ARG(bytes == 4 * C); return copy(p->tab_i + (q - ints) * C); }
        if (name[1] == 'E' || name[1] == 'V') { GP_ARG(bytes == 8 * C); return copy(p->tab_d + (name[1] == 'V' ? C : 0)); }
    }
    for (int k = 0; k < BIN_NARRAYS; ++k)
        if (strcasecmp(kBinRaw[k], name) == 0) {
            GP_ARG(bytes == bin_raw_count(k, m, B) * bin_raw_width(k));
            return copy(p->block + L.off[k]);
        }
    int cell = -1, item = -1, bin = -1;
    for (int k = 0; k < GPIRT_BINS_CELL_NFIELDS; ++k) if (strcmp(kBinCell[k], name) == 0) cell = k;
    for (int k = 0; k < GPIRT_BINS_ITEM_NFIELDS; ++k) if (strcmp(kBinItem[k], name) == 0) item = k;
    for (int k = 0; k < GPIRT_BINS_BIN_NFIELDS; ++k) if (strcmp(kBinBin[k], name) == 0) bin = k;
    if (cell < 0 && item < 0 && bin < 0) { set_error("unknown theta-binned PPC field '%s'", name); return GPIRT_E_ARG; }
    GP_ARG(bytes == 8 * (cell >= 0 ? C : item >= 0 ? m : B));
    HostBins r;
    GP_TRY(bin_read(st, p->block, r, "gpirt_sampler_ppc_bins_get", 0));
    double* out = static_cast<double*>(h_out);
    if (cell >= 0) for (int64_t at = 0; at < C; ++at) out[at] = bin_cell_field(r, cell, at);
    else if (item >= 0) for (int64_t j = 0; j < m; ++j) out[j] = bin_item_field(r, item, j);
    else for (int64_t b = 0; b < B; ++b) out[b] = bin_bin_field(r, bin, b);
    return 0;
}

int bin_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ppc_bins* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_BINS_MAX_TOP) {
        set_error("theta-binned PPC: top = %d is outside 1..%d", out->top, GPIRT_BINS_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) {
        GP_ARG(d_states[c]);
        if (signs) GP_ARG(signs[c] == 1 || signs[c] == -1);
    }
    HostBins pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostBins& r = c == 0 ? pooled : one;
        GP_TRY(bin_read(h->stream, d_states[c], r, "gpirt_ppc_bins_combine", c));
        if (c > 0 && (r.n != pooled.n || r.m != pooled.m || r.item0 != pooled.item0 || r.B != pooled.B ||
                      !std::equal(r.cuts(), r.cuts() + BIN_CUT_WORDS, pooled.cuts()))) {
            set_error("gpirt_ppc_bins_combine: state %d has another n, m, item0 or cuts than state 0", c);
            return GPIRT_E_ARG;
        }
        if (signs && signs[c] < 0) bin_reflect(r);
        if (c == 0) continue;
        pooled.hdr()[3] += one.hdr()[3];
        pooled.hdr()[4] += one.hdr()[4];
        for (int k = 0; k < BIN_NARRAYS; ++k) {
            const int64_t cnt = bin_raw_count(k, r.m, r.B);
            const bool dbl = (k >= BIN_SUM_E && k <= BIN_SUM_Z) || (k >= BIN_CHI_OBS && k <= BIN_CHI_REP);
            if (dbl) for (int64_t g = 0; g < cnt; ++g) pooled.arr<double>(k)[g] += one.arr<double>(k)[g];      // in chain order
            else if (bin_raw_width(k) == 4) for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
            else for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint64_t>(k)[g] += one.arr<uint64_t>(k)[g];
        }
    }
    bin_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
