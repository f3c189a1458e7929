// ppc_person.hip -- the person fit of the posterior predictive checks (include/gpirt_hip.h, "person fit in the PPC"; DESIGN.md
// section 28): every respondent's Guttman errors, the standardised log-likelihood lz and the person response function (the yes
// rate within groups of the items' easiness), for the data and for the PPC's replicate of every draw.
//
// prs_strips_kernel: one streaming pass over f, mu and y, lanes along i (coalesced columns, visited through `order`), 256
// respondents x one STRIP per work-group: at most 32 positions of the item order, all of ONE group.  It forms the PPC's replicate
// again (the same p, the same uniform) and leaves per (strip, respondent) the packed counts ones | observed << 8 | G_s << 16,
// the fixed-point E and V and the three lz sums (the strip's observed cells in ascending position), and the word that tells of a
// non-finite g in an observed cell.
// prs_finish_kernel: one thread per respondent walks the strips in ascending order, joins the Guttman count G = sum G_s +
// sum_{s < s'} z_s o_s' (z the zeros, o the ones of a strip), builds the K cells group by group, adds the strips' lz sums in
// order, forms the statistics and decides.  It owns every accumulator of its respondent: no atomics, byte-identical states.
// The DATA instances run once at enable with Y in place of the replicate: the same code counts the constants (x_obs, g_obs,
// q_obs, tN, tT).
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace gpirt {

namespace {

constexpr int PS_THREADS = 256;
constexpr int PF_THREADS = 128;
constexpr double PRS_FIX = 17592186044416.0;       // 2^44
constexpr double PRS_UNFIX = 1.0 / PRS_FIX;
static_assert(PRS_STRIP <= 32, "a strip partial packs two 8-bit counts and G_s <= 16 x 16");
static_assert(GPIRT_PERSON_MAX_M < 65536, "PrsStrips::lo");

// type: 'q' 8-byte integer, 'u' uint32, 'd' double; kind: 'n' n, 'c' K n
struct PrsArr { const char* name; char type; char kind; };
const PrsArr kPrsArr[PRS_NARRAYS] = {
    { "x_obs", 'q', 'n' }, { "g_obs", 'q', 'n' }, { "q_obs", 'q', 'n' }, { "tN", 'u', 'c' }, { "tT", 'u', 'c' },
    { "g_ge", 'u', 'n' }, { "g_gt", 'u', 'n' }, { "g_undefined_count", 'u', 'n' }, { "g_rep_sum", 'q', 'n' }, { "gn_rep_sum", 'd', 'n' },
    { "lz_undefined_count", 'u', 'n' }, { "lz_obs_sum", 'd', 'n' }, { "lz_rep_sum", 'd', 'n' }, { "lz_rep_sumsq", 'd', 'n' },
    { "sum_r", 'q', 'c' }, { "sum_e", 'd', 'c' }, { "cell_ge", 'u', 'c' }, { "cell_gt", 'u', 'c' },
    { "chi_ge", 'u', 'n' }, { "chi_gt", 'u', 'n' }, { "chi_obs_sum", 'd', 'n' }, { "chi_rep_sum", 'd', 'n' } };
const char* const kPrsResp[GPIRT_PERSON_RESP_NFIELDS] = {
    "guttman_obs", "guttman_norm_obs", "guttman_rep_mean", "guttman_norm_rep_mean", "ppp_guttman", "ppp_guttman_mid", "guttman_undefined",
    "lz_obs_mean", "lz_rep_mean", "lz_rep_sd", "lz_undefined", "ppp_chi2", "ppp_chi2_mid", "chi2_obs_mean", "chi2_rep_mean" };
const char* const kPrsCell[GPIRT_PERSON_CELL_NFIELDS] = { "obs_rate", "rep_rate", "exp_rate", "ppp_cell", "ppp_cell_mid" };
constexpr int PRS_RESP_MID = 5;                    // ppp_guttman_mid

inline int prs_width(int k) { return kPrsArr[k].type == 'u' ? 4 : 8; }
inline int64_t prs_count(int k, int64_t n, int64_t K) { return kPrsArr[k].kind == 'n' ? n : K * n; }

struct PrsStripArgs {
    const double* f; const double* mu; const double* y;
    const int32_t* order;
    int64_t n;
    uint64_t seed; uint32_t iter, item0;
    PrsStrips st;
    uint32_t* part_c;                     // [strips][n]
    int64_t* part_ev;                     // [strips][2][n]
    double* part_lz;                      // [strips][3][n]
    int* bad;
};

template <bool DATA>
__global__ __launch_bounds__(PS_THREADS) void prs_strips_kernel(PrsStripArgs a)
{
    const int s = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * PS_THREADS + threadIdx.x;
    if (i >= a.n) return;                                          // (no barrier and no shuffle in this kernel)
    const int lo = a.st.lo[s], len = a.st.len[s];
    uint32_t ones = 0, zeros = 0, G = 0;
    int64_t E = 0, V = 0;
    double Wo = 0.0, Wr = 0.0, Vl = 0.0;
    for (int t = 0; t < len; ++t) {
        const int64_t j = a.order[lo + t];
        const int64_t c = i + j * a.n;
        const double yv = a.y[c];
        if (!(yv == yv)) continue;                                 // not observed
        bool bit;
        if constexpr (DATA) bit = yv > 0.0;
        else {
            const double g = a.f[c] + a.mu[c];
            if (!isfinite(g)) { *a.bad = 1; continue; }            // (every writer stores the same word; the draw is skipped)
            const double e = exp(-fabs(g));
            const double p = g >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
            const double q = g >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
            const double u = item_uniform(a.seed, a.iter, GPIRT_ST_PPC, (uint32_t)(a.item0 + j), (uint32_t)i);
            bit = u < p;
            const double pq = p * q;
            E += (int64_t)rint(p * PRS_FIX);
            V += (int64_t)rint(pq * PRS_FIX);
            const double yo = (yv > 0.0 ? 1.0 : 0.0) - p, yr = (bit ? 1.0 : 0.0) - p;
            const double to = yo * g, tr = yr * g, tv = (pq * g) * g;
            Wo += to; Wr += tr; Vl += tv;
        }
        if (bit) { ones += 1; G += zeros; } else zeros += 1;
    }
    const int64_t at = (int64_t)s * a.n + i;
    a.part_c[at] = ones | ((ones + zeros) << 8) | (G << 16);
    if constexpr (!DATA) {
        a.part_ev[2 * at - i] = E;                                 // [s][0][i]
        a.part_ev[2 * at - i + a.n] = V;                           // [s][1][i]
        const int64_t b = 3 * at - 2 * i;                          // [s][0][i]
        a.part_lz[b] = Wo; a.part_lz[b + a.n] = Wr; a.part_lz[b + 2 * a.n] = Vl;
    }
}

__device__ __forceinline__ double prs_x2_term(uint32_t Cn, int64_t E, int64_t V)
{
    const double d = (double)((int64_t)((uint64_t)Cn << 44) - E) * PRS_UNFIX;
    const double v = (double)V * PRS_UNFIX;
    const double dd = d * d;
    return dd / v;
}

struct PrsFinishArgs {
    const uint32_t* part_c; const int64_t* part_ev; const double* part_lz;
    const int* bad;
    int64_t n; int K;
    PrsStrips st;
    uint64_t* block; PrsLayout L;
    int64_t* xgq_last; uint32_t* tr_last; int64_t* tev_last; double* lz_last; double* chi_last;
};

template <bool DATA>
__global__ __launch_bounds__(PF_THREADS) void prs_finish_kernel(PrsFinishArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * PF_THREADS + threadIdx.x;
    const bool skip = !DATA && *a.bad != 0;                        // (the same for every thread of the launch)
    int64_t* hdr = reinterpret_cast<int64_t*>(a.block);
    if (!DATA && i == 0) hdr[skip ? 6 : 5] += 1;                   // (nobody else in this launch reads the header)
    if (skip || i >= a.n) return;
    const int64_t n = a.n, C = (int64_t)a.K * n;
    auto u32 = [&](int k) { return reinterpret_cast<uint32_t*>(a.block + a.L.off[k]); };
    auto u64 = [&](int k) { return a.block + a.L.off[k]; };
    auto i64 = [&](int k) { return reinterpret_cast<int64_t*>(a.block + a.L.off[k]); };
    auto f64 = [&](int k) { return reinterpret_cast<double*>(a.block + a.L.off[k]); };
    int64_t N = 0;
    if constexpr (!DATA) for (int k = 0; k < a.K; ++k) N += u32(PRS_TN)[(int64_t)k * n + i];
    [[maybe_unused]] const bool live = N > 0;
    int64_t X = 0, G = 0, Z = 0, Nd = 0;
    double Wo = 0.0, Wr = 0.0, Vl = 0.0, x2T = 0.0, x2R = 0.0;
    for (int k = 0; k < a.K; ++k) {
        uint32_t cn = 0, cr = 0;
        int64_t E = 0, V = 0;
        for (int s = a.st.first[k]; s < a.st.first[k + 1]; ++s) {
            const int64_t at = (int64_t)s * n + i;
            const uint32_t pk = a.part_c[at];
            const int64_t o = pk & 0xFFu, cnt = (pk >> 8) & 0xFFu;
            G += (int64_t)(pk >> 16) + Z * o;
            Z += cnt - o; X += o; Nd += cnt;
            cn += (uint32_t)cnt; cr += (uint32_t)o;
            if constexpr (!DATA) {
                E += a.part_ev[2 * at - i]; V += a.part_ev[2 * at - i + n];
                const int64_t b = 3 * at - 2 * i;
                Wo += a.part_lz[b]; Wr += a.part_lz[b + n]; Vl += a.part_lz[b + 2 * n];
            }
        }
        const int64_t at = (int64_t)k * n + i;
        if constexpr (DATA) { u32(PRS_TN)[at] = cn; u32(PRS_TT)[at] = cr; }
        else {
            a.tr_last[at] = cr; a.tev_last[at] = E; a.tev_last[C + at] = V;
            const uint32_t T = u32(PRS_TT)[at];
            if (cn > 0) {
                u64(PRS_SUM_R)[at] += cr;
                f64(PRS_SUM_E)[at] += (double)E * PRS_UNFIX;
                u32(PRS_CELL_GE)[at] += cr >= T ? 1u : 0u;
                u32(PRS_CELL_GT)[at] += cr > T ? 1u : 0u;
            }
            if (V > 0) { x2T += prs_x2_term(T, E, V); x2R += prs_x2_term(cr, E, V); }
        }
    }
    const int64_t Q = X * (Nd - X);
    if constexpr (DATA) { i64(PRS_X_OBS)[i] = X; i64(PRS_G_OBS)[i] = G; i64(PRS_Q_OBS)[i] = Q; return; }
    a.xgq_last[i] = X; a.xgq_last[n + i] = G; a.xgq_last[2 * n + i] = Q;
    a.lz_last[i] = Wo; a.lz_last[n + i] = Wr; a.lz_last[2 * n + i] = Vl;
    a.chi_last[i] = x2T; a.chi_last[n + i] = x2R;
    if (!live) return;                                             // a respondent without an observed cell: nothing moves
    const int64_t Go = i64(PRS_G_OBS)[i], Qo = i64(PRS_Q_OBS)[i];
    if (Qo == 0 || Q == 0) u32(PRS_G_UNDEF)[i] += 1u;
    else {
        const int64_t lhs = G * Qo, rhs = Go * Q;                  // below 2^46 each
        u32(PRS_G_GE)[i] += lhs >= rhs ? 1u : 0u;
        u32(PRS_G_GT)[i] += lhs > rhs ? 1u : 0u;
        u64(PRS_G_REP_SUM)[i] += (uint64_t)G;
        f64(PRS_GN_REP_SUM)[i] += (double)G / (double)Q;
    }
    if (!(isfinite(Vl) && Vl > 0.0) || !isfinite(Wo) || !isfinite(Wr)) u32(PRS_LZ_UNDEF)[i] += 1u;
    else {
        const double sd = sqrt(Vl), zo = Wo / sd, zr = Wr / sd;
        f64(PRS_LZ_OBS_SUM)[i] += zo;
        f64(PRS_LZ_REP_SUM)[i] += zr;
        const double zz = zr * zr;
        f64(PRS_LZ_REP_SUMSQ)[i] += zz;
    }
    u32(PRS_CHI_GE)[i] += x2R >= x2T ? 1u : 0u;
    u32(PRS_CHI_GT)[i] += x2R > x2T ? 1u : 0u;
    f64(PRS_CHI_OBS)[i] += x2T;
    f64(PRS_CHI_REP)[i] += x2R;
}

// a state block on the host
struct HostPrs {
    std::vector<uint64_t> w;
    int64_t n = 0, m = 0, K = 0;
    PrsLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    const int64_t* cuts() const { return hdr() + PRS_HEADER_WORDS; }
    const int32_t* order() const { return reinterpret_cast<const int32_t*>(w.data() + L.order); }
    template <class T> T* arr(int k) { return reinterpret_cast<T*>(w.data() + L.off[k]); }
    template <class T> const T* arr(int k) const { return reinterpret_cast<const T*>(w.data() + L.off[k]); }
    int64_t S() const { return hdr()[5]; }
    int64_t nobs(int64_t i) const
    {
        int64_t N = 0;
        for (int64_t k = 0; k < K; ++k) N += arr<uint32_t>(PRS_TN)[k * n + i];
        return N;
    }
};

int prs_read(hipStream_t st, const void* d_state, HostPrs& r, const char* who, int c)
{
    int64_t hdr[PRS_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] != PRS_TAG || hdr[1] != PRS_LAYOUT_VERSION || hdr[2] <= 0 || hdr[2] > GPIRT_PERSON_MAX_N || hdr[3] < 2 ||
        hdr[3] > GPIRT_PERSON_MAX_M || hdr[4] < 2 || hdr[4] > GPIRT_PERSON_MAX_K || hdr[5] < 0 || hdr[6] < 0) {
        set_error("%s: state %d is not a person-fit state block of layout %d", who, c, PRS_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[2]; r.m = hdr[3]; r.K = hdr[4];
    r.L = prs_layout(r.n, r.m, r.K);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

double prs_resp_field(const HostPrs& r, int fld, int64_t i)
{
    const double nan = (double)NAN;
    if (r.nobs(i) == 0) return nan;
    const int64_t S = r.S();
    const double dS = (double)S;
    auto c = [&](int k) { return (double)r.arr<uint32_t>(k)[i]; };
    const int64_t Sg = S - (int64_t)r.arr<uint32_t>(PRS_G_UNDEF)[i], Sl = S - (int64_t)r.arr<uint32_t>(PRS_LZ_UNDEF)[i];
    const int64_t Qo = r.arr<int64_t>(PRS_Q_OBS)[i];
    switch (fld) {
        case 0: return (double)r.arr<int64_t>(PRS_G_OBS)[i];
        case 1: return Qo > 0 ? (double)r.arr<int64_t>(PRS_G_OBS)[i] / (double)Qo : nan;
        case 2: return Sg >= 1 ? (double)r.arr<uint64_t>(PRS_G_REP_SUM)[i] / (double)Sg : nan;
        case 3: return Sg >= 1 ? r.arr<double>(PRS_GN_REP_SUM)[i] / (double)Sg : nan;
        case 4: return Sg >= 1 ? c(PRS_G_GE) / (double)Sg : nan;
        case 5: return Sg >= 1 ? (c(PRS_G_GE) + c(PRS_G_GT)) / (2.0 * (double)Sg) : nan;
        case 6: return c(PRS_G_UNDEF);
        case 7: return Sl >= 1 ? r.arr<double>(PRS_LZ_OBS_SUM)[i] / (double)Sl : nan;
        case 8: return Sl >= 1 ? r.arr<double>(PRS_LZ_REP_SUM)[i] / (double)Sl : nan;
        case 9: {
            if (Sl < 2) return nan;
            const double sum = r.arr<double>(PRS_LZ_REP_SUM)[i], mean = sum / (double)Sl, sm = sum * mean;
            const double v = (r.arr<double>(PRS_LZ_REP_SUMSQ)[i] - sm) / (double)(Sl - 1);
            return v > 0.0 ? sqrt(v) : 0.0;
        }
        case 10: return c(PRS_LZ_UNDEF);
        case 11: return S >= 1 ? c(PRS_CHI_GE) / dS : nan;
        case 12: return S >= 1 ? (c(PRS_CHI_GE) + c(PRS_CHI_GT)) / (2.0 * dS) : nan;
        case 13: return S >= 1 ? r.arr<double>(PRS_CHI_OBS)[i] / dS : nan;
        case 14: return S >= 1 ? r.arr<double>(PRS_CHI_REP)[i] / dS : nan;
        default: break;
    }
    return nan;
}

double prs_cell_field(const HostPrs& r, int fld, int64_t at)
{
    const int64_t S = r.S();
    const double nan = (double)NAN, dS = (double)S;
    const uint32_t tN = r.arr<uint32_t>(PRS_TN)[at];
    if (tN == 0) return nan;
    auto c = [&](int k) { return (double)r.arr<uint32_t>(k)[at]; };
    if (fld == 0) return (double)r.arr<uint32_t>(PRS_TT)[at] / (double)tN;
    if (S < 1) return nan;
    switch (fld) {
        case 1: return (double)r.arr<uint64_t>(PRS_SUM_R)[at] / (dS * (double)tN);
        case 2: return r.arr<double>(PRS_SUM_E)[at] / (dS * (double)tN);
        case 3: return c(PRS_CELL_GE) / dS;
        case 4: return (c(PRS_CELL_GE) + c(PRS_CELL_GT)) / (2.0 * dS);
        default: break;
    }
    return nan;
}

int64_t prs_group_edge(const HostPrs& r, bool hi, int64_t k)
{
    if (!hi) return k == 0 ? 0 : r.cuts()[k - 1];
    return k == r.K - 1 ? r.m - 1 : r.cuts()[k] - 1;
}

void prs_fill(const HostPrs& r, gpirt_ppc_person* out)
{
    const int64_t n = r.n, m = r.m, K = r.K;
    out->n = n; out->m = m; out->K = (int)K; out->person_draws = r.hdr()[5]; out->person_skipped = r.hdr()[6];
    int64_t ns = 0;
    for (int64_t i = 0; i < n; ++i) ns += r.nobs(i) > 0 ? 1 : 0;
    out->n_scored = ns;
    for (int q = 0; q < GPIRT_PERSON_MAX_K; ++q) out->cuts[q] = q < K - 1 ? (int)r.cuts()[q] : 0;
    for (int fld = 0; fld < GPIRT_PERSON_RESP_NFIELDS; ++fld)
        if (out->resp[fld]) for (int64_t i = 0; i < n; ++i) out->resp[fld][i] = prs_resp_field(r, fld, i);
    for (int fld = 0; fld < GPIRT_PERSON_CELL_NFIELDS; ++fld)
        if (out->cell[fld]) for (int64_t at = 0; at < K * n; ++at) out->cell[fld][at] = prs_cell_field(r, fld, at);
    for (int k = 0; k < PRS_NARRAYS; ++k)
        if (out->raw[k]) memcpy(out->raw[k], r.w.data() + r.L.off[k], (size_t)(prs_count(k, n, K) * prs_width(k)));
    for (int64_t k = 0; k < K; ++k) {
        if (out->group_lo) out->group_lo[k] = prs_group_edge(r, false, k);
        if (out->group_hi) out->group_hi[k] = prs_group_edge(r, true, k);
    }
    if (out->group_items) memcpy(out->group_items, r.order(), sizeof(int32_t) * (size_t)m);
    if (!out->worst_respondents && !out->worst_ppp_guttman_mid) return;
    // the respondents by increasing ppp_guttman_mid, ties to the lowest i: a stable sort
    struct E { double mid; int64_t i; };
    std::vector<E> es;
    for (int64_t i = 0; i < n; ++i) {
        const double mid = prs_resp_field(r, PRS_RESP_MID, i);
        if (mid == mid) es.push_back(E{ mid, i });
    }
    std::stable_sort(es.begin(), es.end(), [](const E& x, const E& y) { return x.mid < y.mid; });
    for (int t = 0; t < out->top; ++t) {
        const bool have = (size_t)t < es.size();
        if (out->worst_respondents) out->worst_respondents[t] = have ? es[(size_t)t].i : -1;
        if (out->worst_ppp_guttman_mid) out->worst_ppp_guttman_mid[t] = have ? es[(size_t)t].mid : (double)NAN;
    }
}

// the strips of the header: each group's positions in runs of PRS_STRIP from the group's first position on
PrsStrips prs_strips(int64_t m, int K, const int* cuts)
{
    PrsStrips s{};
    for (int k = 0; k < K; ++k) {
        const int lo = k == 0 ? 0 : cuts[k - 1], hi = k == K - 1 ? (int)m : cuts[k];
        s.first[k] = s.ns;
        for (int at = lo; at < hi; at += PRS_STRIP) {
            s.lo[s.ns] = (uint16_t)at;
            s.len[s.ns] = (uint8_t)std::min(PRS_STRIP, hi - at);
            s.ns += 1;
        }
    }
    for (int k = K; k <= GPIRT_PERSON_MAX_K; ++k) s.first[k] = s.ns;
    return s;
}

template <bool DATA>
int prs_launch(hipStream_t st, PrsState* p, const double* f, const double* mu, const double* y, uint64_t seed, uint32_t iter)
{
    if (!DATA) GP_HIP(hipMemsetAsync(p->ctl, 0, sizeof(int), st));
    PrsStripArgs a{};
    a.f = f; a.mu = mu; a.y = y; a.order = p->order; a.n = p->n; a.seed = seed; a.iter = iter; a.item0 = (uint32_t)p->item0;
    a.st = p->strips; a.part_c = p->part_c; a.part_ev = p->part_ev; a.part_lz = p->part_lz; a.bad = p->ctl;
    const unsigned rblocks = (unsigned)((p->n + PS_THREADS - 1) / PS_THREADS);
    hipLaunchKernelGGL((prs_strips_kernel<DATA>), dim3(rblocks, (unsigned)p->strips.ns), dim3(PS_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    PrsFinishArgs u{};
    u.part_c = p->part_c; u.part_ev = p->part_ev; u.part_lz = p->part_lz; u.bad = p->ctl; u.n = p->n; u.K = p->K; u.st = p->strips;
    u.block = p->block; u.L = prs_layout(p->n, p->m, p->K);
    u.xgq_last = p->xgq_last; u.tr_last = p->tr_last; u.tev_last = p->tev_last; u.lz_last = p->lz_last; u.chi_last = p->chi_last;
    hipLaunchKernelGGL((prs_finish_kernel<DATA>), dim3((unsigned)((p->n + PF_THREADS - 1) / PF_THREADS)), dim3(PF_THREADS), 0, st, u);
    GP_HIP(hipGetLastError());
    return 0;
}

}  // namespace

PrsLayout prs_layout(int64_t n, int64_t m, int64_t K)
{
    PrsLayout L{};
    int64_t at = PRS_HEADER_WORDS + PRS_CUT_WORDS;
    L.order = at;
    at += (4 * m + 15) / 16 * 2;
    for (int k = 0; k < PRS_NARRAYS; ++k) {
        L.off[k] = at;
        const int64_t bytes = prs_count(k, n, K) * prs_width(k);
        at += (bytes + 15) / 16 * 2;                                  // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int64_t prs_state_words(const PrsState* p) { return prs_layout(p->n, p->m, p->K).words; }

int prs_check(int64_t n, int64_t m, int K, const int32_t* order, const int* cuts)
{
    if (m < 2 || m > GPIRT_PERSON_MAX_M) {
        set_error("person fit: m = %lld is outside 2..%d items", (long long)m, GPIRT_PERSON_MAX_M);
        return GPIRT_E_ARG;
    }
    if (n < 1 || n > GPIRT_PERSON_MAX_N) {
        set_error("person fit: n = %lld is beyond %d respondents", (long long)n, GPIRT_PERSON_MAX_N);
        return GPIRT_E_ARG;
    }
    if (K < 2 || K > GPIRT_PERSON_MAX_K || !cuts) {
        set_error("person fit: %d item groups given, 2..%d are taken (K - 1 cuts)", K, GPIRT_PERSON_MAX_K);
        return GPIRT_E_ARG;
    }
    if (!order) {
        set_error("person fit: no item order given (a permutation of 0..%lld, the easiest item first)", (long long)(m - 1));
        return GPIRT_E_ARG;
    }
    std::vector<char> seen((size_t)m, 0);
    for (int64_t t = 0; t < m; ++t) {
        const int64_t j = order[t];
        if (j < 0 || j >= m || seen[(size_t)j]) {
            set_error("person fit: the order is not a permutation of 0..%lld (entry %lld is %lld: %s)", (long long)(m - 1), (long long)t,
                      (long long)j, (j < 0 || j >= m) ? "out of range" : "a repeat");
            return GPIRT_E_ARG;
        }
        seen[(size_t)j] = 1;
    }
    for (int q = 0; q < K - 1; ++q)
        if (cuts[q] < 1 || cuts[q] > m - 1 || (q > 0 && cuts[q] <= cuts[q - 1])) {
            set_error("person fit: the cuts must be increasing integers in 1..%lld (cut %d is %d)", (long long)(m - 1), q + 1, cuts[q]);
            return GPIRT_E_ARG;
        }
    return 0;
}

void prs_free(PrsState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = PrsState{};
}

int prs_alloc(hipStream_t st, PrsState* p, int64_t n, int64_t m, int64_t item0, const double* y, int K, const int32_t* order,
              const int* cuts)
{
    GP_TRY(prs_check(n, m, K, order, cuts));
    const PrsLayout L = prs_layout(n, m, K);
    p->n = n; p->m = m; p->item0 = item0; p->K = K;
    for (int q = 0; q < K - 1; ++q) p->cuts[q] = cuts[q];
    p->strips = prs_strips(m, K, cuts);
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    const size_t N = (size_t)n, C = (size_t)K * N, NS = (size_t)p->strips.ns;
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->order, sizeof(int32_t) * (size_t)m));
    GP_TRY(get((void**)&p->part_c, sizeof(uint32_t) * NS * N));
    GP_TRY(get((void**)&p->part_ev, sizeof(int64_t) * NS * 2 * N));
    GP_TRY(get((void**)&p->part_lz, sizeof(double) * NS * 3 * N));
    GP_TRY(get((void**)&p->ctl, sizeof(int) * 4));
    GP_TRY(get((void**)&p->xgq_last, sizeof(int64_t) * 3 * N));
    GP_TRY(get((void**)&p->tr_last, sizeof(uint32_t) * C));
    GP_TRY(get((void**)&p->tev_last, sizeof(int64_t) * 2 * C));
    GP_TRY(get((void**)&p->lz_last, sizeof(double) * 3 * N));
    GP_TRY(get((void**)&p->chi_last, sizeof(double) * 2 * N));
    int64_t head[PRS_HEADER_WORDS + PRS_CUT_WORDS] = { PRS_TAG, PRS_LAYOUT_VERSION, n, m, K, 0, 0, 0 };
    for (int q = 0; q < K - 1; ++q) head[PRS_HEADER_WORDS + q] = cuts[q];
    GP_HIP(hipMemcpyAsync(p->block, head, sizeof(head), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->block + L.order, order, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->order, order, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // head and order are the caller's: nothing below may leave with a copy pending
    GP_TRY(prs_launch<true>(st, p, nullptr, nullptr, y, 0, 0));       // the constants
    p->on = true;
    return 0;
}

int launch_prs_accumulate(hipStream_t st, PrsState* p, const double* f, const double* mu, const double* y, uint64_t seed,
                          uint32_t iter)
{
    return prs_launch<false>(st, p, f, mu, y, seed, iter);
}

int prs_get(hipStream_t st, PrsState* p, const char* name, void* h_out, int64_t bytes)
{
    const int64_t n = p->n, m = p->m, K = p->K, C = K * n;
    const PrsLayout L = prs_layout(n, m, K);
    auto copy = [&](const void* src, void* dst, int64_t nb) -> int {
        GP_HIP(hipMemcpyAsync(dst, src, (size_t)nb, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 16); return copy(p->block + 5, h_out, bytes); }
    if (strcmp(name, "cuts") == 0) { GP_ARG(bytes == 8 * (K - 1)); return copy(p->block + PRS_HEADER_WORDS, h_out, bytes); }
    if (strcmp(name, "order") == 0 || strcmp(name, "group_items") == 0) { GP_ARG(bytes == 4 * m); return copy(p->block + L.order, h_out, bytes); }
    static const char* const kXgq[3] = { "xr", "gr", "qr" };
    for (int q = 0; q < 3; ++q)
        if (strcmp(name, kXgq[q]) == 0) { GP_ARG(bytes == 8 * n); return copy(p->xgq_last + q * n, h_out, bytes); }
    if (strcmp(name, "tR") == 0) { GP_ARG(bytes == 4 * C); return copy(p->tr_last, h_out, bytes); }
    if (strcmp(name, "tE") == 0) { GP_ARG(bytes == 8 * C); return copy(p->tev_last, h_out, bytes); }
    if (strcmp(name, "tV") == 0) { GP_ARG(bytes == 8 * C); return copy(p->tev_last + C, h_out, bytes); }
    if (strcmp(name, "lz") == 0) { GP_ARG(bytes == 8 * 3 * n); return copy(p->lz_last, h_out, bytes); }
    if (strcmp(name, "chi") == 0) { GP_ARG(bytes == 8 * 2 * n); return copy(p->chi_last, h_out, bytes); }
    for (int k = 0; k < PRS_NARRAYS; ++k)
        if (strcmp(kPrsArr[k].name, name) == 0) {
            GP_ARG(bytes == prs_count(k, n, K) * prs_width(k));
            return copy(p->block + L.off[k], h_out, bytes);
        }
    int resp = -1, cell = -1;
    for (int k = 0; k < GPIRT_PERSON_RESP_NFIELDS; ++k) if (strcmp(kPrsResp[k], name) == 0) resp = k;
    for (int k = 0; k < GPIRT_PERSON_CELL_NFIELDS; ++k) if (strcmp(kPrsCell[k], name) == 0) cell = k;
    const bool lo = strcmp(name, "group_lo") == 0, hi = strcmp(name, "group_hi") == 0;
    if (resp < 0 && cell < 0 && !lo && !hi) {
        set_error("unknown person-fit field '%s'", name);
        return GPIRT_E_ARG;
    }
    GP_ARG(bytes == 8 * (resp >= 0 ? n : cell >= 0 ? C : K));
    HostPrs r;
    GP_TRY(prs_read(st, p->block, r, "gpirt_sampler_ppc_person_get", 0));
    double* out = static_cast<double*>(h_out);
    if (resp >= 0) for (int64_t i = 0; i < n; ++i) out[i] = prs_resp_field(r, resp, i);
    else if (cell >= 0) for (int64_t at = 0; at < C; ++at) out[at] = prs_cell_field(r, cell, at);
    else for (int64_t k = 0; k < K; ++k) static_cast<int64_t*>(h_out)[k] = prs_group_edge(r, hi, k);
    return 0;
}

int prs_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_person* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_PERSON_MAX_TOP) {
        set_error("person fit: top = %d is outside 1..%d", out->top, GPIRT_PERSON_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    HostPrs pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostPrs& r = c == 0 ? pooled : one;
        GP_TRY(prs_read(h->stream, d_states[c], r, "gpirt_ppc_person_combine", c));
        if (c == 0) continue;
        // the cuts, the order and the constants (x_obs .. tT) lie between the header and the first accumulator
        if (r.n != pooled.n || r.m != pooled.m || r.K != pooled.K ||
            memcmp(r.w.data() + PRS_HEADER_WORDS, pooled.w.data() + PRS_HEADER_WORDS,
                   sizeof(uint64_t) * (size_t)(r.L.off[PRS_G_GE] - PRS_HEADER_WORDS)) != 0) {
            set_error("gpirt_ppc_person_combine: state %d has another n, m, K, order, cuts or response matrix than state 0", c);
            return GPIRT_E_ARG;
        }
        pooled.hdr()[5] += one.hdr()[5];
        pooled.hdr()[6] += one.hdr()[6];
        for (int k = PRS_G_GE; k < PRS_NARRAYS; ++k) {
            const int64_t cnt = prs_count(k, r.n, r.K);
            if (kPrsArr[k].type == 'd') for (int64_t g = 0; g < cnt; ++g) pooled.arr<double>(k)[g] += one.arr<double>(k)[g];      // in chain order
            else if (kPrsArr[k].type == 'u') for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
            else for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint64_t>(k)[g] += one.arr<uint64_t>(k)[g];
        }
    }
    prs_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
