// ppc.hip -- posterior predictive checks accumulated on the device, one draw at a time, in O(n + m) memory
// (include/gpirt_hip.h, "posterior predictive checks").  For the state after an iteration,
// g = f + mu, p = plogis(g) (the arithmetic of summary.hip's cell_terms), the replicate yrep = +1 if u < p else -1 with
// u = item_uniform(seed, iter, GPIRT_ST_PPC, item0 + j, i), and per item, per respondent and for the whole matrix:
// R = #{yrep = +1}, D(y) and D(yrep) = 2 sum softplus(-y g), Delta = sum over flipped cells of y g (= (D(yrep) - D(y)) / 2
// exactly in algebra, exactly 0 when nothing flipped), the correctly classified cells.
//
// ppc_replicate_kernel is one streaming pass: f, mu and y read once (lanes along i: coalesced).  A lane owns one respondent
// over a strip of PPC_STRIP items and keeps its row partials in registers; a column's partials go through a wave reduction
// (fixed shuffle tree) and four LDS slots per work-group.  The per-strip row partials and the per-row-block column partials
// land in a scratch array of (strips x n) + (row blocks x m) records; ppc_units_kernel sums them in fixed order, decides
// the >= / > comparisons and updates the accumulators, ppc_total_kernel does the same for the whole matrix from the items'
// sums.  No floating-point atomics: bit-identical from run to run; the geometry (256 rows x 32 items per work-group) is
// fixed, so the sums do not depend on the device either.
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace gpirt {

namespace {

constexpr int PPC_THREADS = 256;
constexpr int PPC_STRIP = 32;            // items per work-group: 32 row blocks x 32 strips = 1024 work-groups at 8192 x 1024
// packed counts of a partial (at most 256 cells of a column per work-group, PPC_STRIP of a row): 10 bits each
constexpr uint32_t PK_R = 1u, PK_CORRECT = 1u << 10, PK_NONFINITE = 1u << 20, PK_MASK = 1023u;

struct PpcArgs {
    const double* f; const double* mu; const double* y;
    int64_t n, m;
    uint64_t seed; uint32_t iter, item0;
    double* rowd; uint32_t* rowi;        // [strip][3][n], [strip][n]: Delta, D(y), D(yrep); the packed counts
    double* cold; uint32_t* coli;        // [row block][3][m], [row block][m]
    // the pairwise checks (ppc_pairs.hip; read by the BYTES instance only): the replicate's 0 / 1 bytes in the product's
    // operand layout, written into the plane *cur does NOT name, and the word that tells of a non-finite g in an observed cell
    unsigned char* rep8; const int* cur; int64_t plane, ksteps; int* bad;
    // the theta-binned item fit (ppc_bins.hip; read by the BINS instances only): this draw's bin of every respondent, the
    // partial tables [row block][item][bin] and the word that tells of a non-finite g in an observed cell
    const unsigned char* bin; int B; uint32_t* bpi; double* bpe; double* bpv; int* bbad;
};

// the BINS instances' staging area: a work-group's 256 cells of one item (E's and V's terms, the flags 1 = observed,
// 2 = y = +1, 4 = rep = 1), the respondents' bins, and the four waves' partial sums per bin
struct PpcBinStage {
    double e[PPC_THREADS], v[PPC_THREADS];
    unsigned char flag[PPC_THREADS], bin[PPC_THREADS];
    double pe[4][32], pv[4][32];
    uint32_t pi[4][32];
};
__device__ __forceinline__ PpcBinStage* ppc_bin_stage()
{
    __shared__ PpcBinStage ppc_bs;
    return &ppc_bs;
}

// the BYTES instance's staging area, [PPC_STRIP][PPC_THREADS] bytes of dynamic LDS (the plain instance asks for none and
// never names it)
constexpr int PPC_STAGE_BYTES = PPC_STRIP * PPC_THREADS;
__device__ __forceinline__ unsigned char* ppc_byte_stage()
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ppc_sb[];
    return ppc_sb;
}

// BYTES: the same pass also leaves rep[i, j] = [yrep = +1] of the observed cells as bytes for pair_counts_kernel -- strip s is
// item block s of that layout, a work-group's 256 respondents are its k-steps 8 rb .. 8 rb + 7 -- through 8 KiB of dynamic LDS, so that
// the stores are the layout's 16-byte pieces.  The instance without BYTES is the kernel as it was before the pairs existed.
// BINS: the same pass also leaves, per item and bin of theta, N, T, R, E and V over the work-group's 256 respondents (ppc_bins.hip):
// a lane stages its cell's p and p q in LDS; lane b < B of every wave then sums the cells of bin b among its wave's 64 rows
// in row order, and lane 32 + b of wave 0 adds the four waves' sums in wave order: every double in a fixed order, g read once.
// The instances without BINS are the kernels as they were before the bins existed.
template <bool BYTES, bool BINS>
__global__ __launch_bounds__(PPC_THREADS) void ppc_replicate_kernel(PpcArgs a)
{
    __shared__ double sd[4][PPC_STRIP][3];
    __shared__ uint32_t si[4][PPC_STRIP];
    const int rb = blockIdx.x, strip = blockIdx.y;
    const int64_t i = (int64_t)rb * PPC_THREADS + threadIdx.x;
    const bool live = i < a.n;
    const int64_t j0 = (int64_t)strip * PPC_STRIP;
    const int w = (int)(a.m - j0 < PPC_STRIP ? a.m - j0 : PPC_STRIP);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double rD = 0.0, rO = 0.0, rR = 0.0;
    uint32_t rI = 0;
    if constexpr (BINS) ppc_bin_stage()->bin[threadIdx.x] = live ? a.bin[i] : BIN_NONE;     // (the loop's first barrier follows)
    for (int jj = 0; jj < w; ++jj) {
        double cD = 0.0, cO = 0.0, cR = 0.0;
        uint32_t cI = 0;
        [[maybe_unused]] double bE = 0.0, bV = 0.0;
        [[maybe_unused]] unsigned bF = 0;
        if (live) {
            const int64_t c = i + (j0 + jj) * a.n;
            const double yv = a.y[c], g = a.f[c] + a.mu[c];
            if (yv == yv) {                                   // an observed cell
                if (!isfinite(g)) cI = PK_NONFINITE;
                else {
                    const double e = exp(-fabs(g));
                    const double p = g >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
                    const double l1 = log1p(e);
                    const double u = item_uniform(a.seed, a.iter, GPIRT_ST_PPC, (uint32_t)(a.item0 + j0 + jj), (uint32_t)i);
                    const double yr = u < p ? 1.0 : -1.0;
                    cO = 2.0 * (l1 + fmax(-yv * g, 0.0));
                    cR = 2.0 * (l1 + fmax(-yr * g, 0.0));
                    if (yr != yv) cD = yv * g;
                    cI = (yr > 0.0 ? PK_R : 0u) + (((g > 0.0) == (yv > 0.0)) ? PK_CORRECT : 0u);
                    if constexpr (BINS) {
                        const double q = g >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
                        bE = p; bV = p * q;
                        bF = 1u | (yv > 0.0 ? 2u : 0u) | (yr > 0.0 ? 4u : 0u);
                    }
                }
            }
        }
        rD += cD; rO += cO; rR += cR; rI += cI;
        if constexpr (BYTES) {
            ppc_byte_stage()[jj * PPC_THREADS + threadIdx.x] = (unsigned char)(cI & PK_R);
            if (cI & PK_NONFINITE) *a.bad = 1;                // (every writer stores the same word)
        }
        if constexpr (BINS) {
            PpcBinStage* bs = ppc_bin_stage();
            if (cI & PK_NONFINITE) *a.bbad = 1;
            bs->e[threadIdx.x] = bE; bs->v[threadIdx.x] = bV; bs->flag[threadIdx.x] = (unsigned char)bF;
            __syncthreads();
            if (lane < a.B) {
                double E = 0.0, V = 0.0;
                uint32_t pk = 0;
                for (int r = wv * 64; r < wv * 64 + 64; ++r) {
                    const unsigned fl = bs->flag[r];
                    if (bs->bin[r] == lane && (fl & 1u)) {
                        E += bs->e[r]; V += bs->v[r];
                        pk += 1u + ((fl >> 1) & 1u) * PK_CORRECT + ((fl >> 2) & 1u) * PK_NONFINITE;      // N | T << 10 | R << 20
                    }
                }
                bs->pe[wv][lane] = E; bs->pv[wv][lane] = V; bs->pi[wv][lane] = pk;
            }
            __syncthreads();
            if (wv == 0 && lane >= 32 && lane - 32 < a.B) {
                const int b = lane - 32;
                const int64_t at = ((int64_t)rb * a.m + j0 + jj) * a.B + b;
                a.bpe[at] = ((bs->pe[0][b] + bs->pe[1][b]) + bs->pe[2][b]) + bs->pe[3][b];
                a.bpv[at] = ((bs->pv[0][b] + bs->pv[1][b]) + bs->pv[2][b]) + bs->pv[3][b];
                a.bpi[at] = bs->pi[0][b] + bs->pi[1][b] + bs->pi[2][b] + bs->pi[3][b];
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cD += __shfl_down(cD, off, 64);
            cO += __shfl_down(cO, off, 64);
            cR += __shfl_down(cR, off, 64);
            cI += __shfl_down(cI, off, 64);
        }
        if (lane == 0) { sd[wv][jj][0] = cD; sd[wv][jj][1] = cO; sd[wv][jj][2] = cR; si[wv][jj] = cI; }
    }
    if (live) {
        const int64_t base = (int64_t)strip * 3 * a.n + i;
        a.rowd[base] = rD; a.rowd[base + a.n] = rO; a.rowd[base + 2 * a.n] = rR;
        a.rowi[(int64_t)strip * a.n + i] = rI;
    }
    __syncthreads();
    if ((int)threadIdx.x < w) {
        const int jj = threadIdx.x;
        const int64_t base = (int64_t)rb * 3 * a.m + j0 + jj;
#pragma unroll
        for (int q = 0; q < 3; ++q)
            a.cold[base + q * a.m] = (sd[0][jj][q] + sd[1][jj][q]) + (sd[2][jj][q] + sd[3][jj][q]);
        a.coli[(int64_t)rb * a.m + j0 + jj] = (si[0][jj] + si[1][jj]) + (si[2][jj] + si[3][jj]);
    }
    if constexpr (BYTES) {
        // piece p = (k-step kk of the work-group, lane L = item jj + 32 x the half of the k-step): 16 respondents of one item
        unsigned char* dst = a.rep8 + (int64_t)(*a.cur ^ 1) * a.plane + ((int64_t)strip * a.ksteps + (int64_t)rb * 8) * 1024;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int p = (int)threadIdx.x + q * PPC_THREADS, kk = p >> 6, L = p & 63, jj = L & 31;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (jj < w) v = *reinterpret_cast<const uint4*>(ppc_byte_stage() + jj * PPC_THREADS + kk * 32 + (L >> 5) * 16);
            *reinterpret_cast<uint4*>(dst + (int64_t)p * 16) = v;
        }
    }
}

struct PpcUnitArgs {
    const double* rowd; const uint32_t* rowi; const double* cold; const uint32_t* coli;
    int64_t n, m, stride;
    int strips, rblocks;
    uint64_t* acc;                       // the accumulators (behind the block's header): [array][stride]
    double* unit_d; uint64_t* unit_i;    // [3][m] each: the items' sums of this draw, for the total
};

// one draw of unit k: a non-finite g counts the draw out, a unit without observed cells keeps every count at 0
__device__ __forceinline__ void ppc_update(uint64_t* acc, int64_t stride, int64_t k, uint64_t R, uint64_t correct,
                                           uint64_t nonfinite, double D, double O, double Rp)
{
    if (acc[PPC_N_OBS * stride + k] == 0) return;
    if (nonfinite) { acc[PPC_NONFINITE * stride + k] += 1; return; }
    const uint64_t T = acc[PPC_OBS_YES * stride + k];
    acc[PPC_SUM_R * stride + k] += R;
    acc[PPC_SUM_R2 * stride + k] += R * R;
    acc[PPC_YES_GE * stride + k] += R >= T ? 1 : 0;
    acc[PPC_YES_GT * stride + k] += R > T ? 1 : 0;
    acc[PPC_DEV_GE * stride + k] += D >= 0.0 ? 1 : 0;
    acc[PPC_CORRECT * stride + k] += correct;
    double* dacc = reinterpret_cast<double*>(acc);
    dacc[PPC_DEV_OBS * stride + k] += O;
    dacc[PPC_DEV_REP * stride + k] += Rp;
}

// unit k < m: item k, the row blocks' partials in order; else respondent k - m, the strips' partials in order
__global__ __launch_bounds__(PPC_THREADS) void ppc_units_kernel(PpcUnitArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.m + a.n) return;
    double D = 0.0, O = 0.0, Rp = 0.0;
    uint64_t R = 0, correct = 0, nonfinite = 0;
    if (k < a.m) {
        for (int rb = 0; rb < a.rblocks; ++rb) {
            const int64_t base = (int64_t)rb * 3 * a.m + k;
            D += a.cold[base]; O += a.cold[base + a.m]; Rp += a.cold[base + 2 * a.m];
            const uint32_t pk = a.coli[(int64_t)rb * a.m + k];
            R += pk & PK_MASK; correct += (pk >> 10) & PK_MASK; nonfinite += (pk >> 20) & PK_MASK;
        }
        a.unit_d[k] = D; a.unit_d[a.m + k] = O; a.unit_d[2 * a.m + k] = Rp;
        a.unit_i[k] = R; a.unit_i[a.m + k] = correct; a.unit_i[2 * a.m + k] = nonfinite;
    } else {
        const int64_t i = k - a.m;
        for (int s = 0; s < a.strips; ++s) {
            const int64_t base = (int64_t)s * 3 * a.n + i;
            D += a.rowd[base]; O += a.rowd[base + a.n]; Rp += a.rowd[base + 2 * a.n];
            const uint32_t pk = a.rowi[(int64_t)s * a.n + i];
            R += pk & PK_MASK; correct += (pk >> 10) & PK_MASK; nonfinite += (pk >> 20) & PK_MASK;
        }
    }
    ppc_update(a.acc, a.stride, k, R, correct, nonfinite, D, O, Rp);
}

// the whole matrix: the items' sums of this draw, thread t taking items t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(PPC_THREADS) void ppc_total_kernel(PpcUnitArgs a)
{
    __shared__ double sm[4];
    __shared__ unsigned long long cnt[3];
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    double v[3] = { 0.0, 0.0, 0.0 };
    unsigned long long c[3] = { 0, 0, 0 };
    for (int64_t j = threadIdx.x; j < a.m; j += PPC_THREADS)
        for (int q = 0; q < 3; ++q) { v[q] += a.unit_d[q * a.m + j]; c[q] += a.unit_i[q * a.m + j]; }
    __syncthreads();
    for (int q = 0; q < 3; ++q) atomicAdd(&cnt[q], c[q]);        // integers: any order gives the same sum
    double t[3];
    for (int q = 0; q < 3; ++q) t[q] = block_sum_256(v[q], sm);
    __syncthreads();
    if (threadIdx.x == 0) ppc_update(a.acc, a.stride, a.m + a.n, cnt[0], cnt[1], cnt[2], t[0], t[1], t[2]);
}

// n_obs and obs_yes of every item and respondent (once, at enable) ...
__global__ __launch_bounds__(PPC_THREADS) void ppc_observed_kernel(const double* __restrict__ y, int64_t n, int64_t m,
                                                                   int64_t stride, uint64_t* acc)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m + n) return;
    uint64_t obs = 0, yes = 0;
    const int64_t first = k < m ? k * n : k - m, step = k < m ? 1 : n, count = k < m ? n : m;
    for (int64_t q = 0; q < count; ++q) {
        const double v = y[first + q * step];
        obs += v == v ? 1 : 0;
        yes += v > 0.0 ? 1 : 0;
    }
    acc[PPC_N_OBS * stride + k] = obs;
    acc[PPC_OBS_YES * stride + k] = yes;
}

// ... and of the whole matrix, from the items'
__global__ void ppc_observed_total_kernel(int64_t n, int64_t m, int64_t stride, uint64_t* acc)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t obs = 0, yes = 0;
    for (int64_t j = 0; j < m; ++j) { obs += acc[PPC_N_OBS * stride + j]; yes += acc[PPC_OBS_YES * stride + j]; }
    acc[PPC_N_OBS * stride + m + n] = obs;
    acc[PPC_OBS_YES * stride + m + n] = yes;
}

const char* const kFieldNames[GPIRT_PPC_NFIELDS] = {
    "n_obs", "obs_yes", "rep_yes_mean", "rep_yes_var", "yes_ge", "yes_gt", "dev_obs_mean", "dev_rep_mean", "dev_ge",
    "correct_mean", "nonfinite", "draws", "rep_yes_sum", "rep_yes_sumsq", "correct_sum" };

// field `fld` of unit k from a state block on the host (the header's draws may be a pooled count)
double ppc_field(const uint64_t* blk, int fld, int64_t k)
{
    const int64_t n = (int64_t)blk[0], m = (int64_t)blk[1], draws = (int64_t)blk[2];
    const int64_t stride = ppc_stride(n, m);
    const uint64_t* acc = blk + PPC_HEADER_WORDS;
    auto u = [&](int arr) { return acc[(int64_t)arr * stride + k]; };
    auto d = [&](int arr) { double x; memcpy(&x, &acc[(int64_t)arr * stride + k], sizeof(x)); return x; };
    const uint64_t nobs = u(PPC_N_OBS);
    const int64_t S = draws - (int64_t)u(PPC_NONFINITE);       // the draws that entered
    const double nan = (double)NAN;
    const bool mean_ok = nobs > 0 && S >= 1;
    switch (fld) {
        case GPIRT_PPC_N_OBS: return (double)nobs;
        case GPIRT_PPC_OBS_YES: return (double)u(PPC_OBS_YES);
        case GPIRT_PPC_REP_YES_MEAN: return mean_ok ? (double)u(PPC_SUM_R) / (double)S : nan;
        case GPIRT_PPC_REP_YES_VAR: {
            if (!(nobs > 0 && S >= 2)) return nan;
            // S sum R^2 - (sum R)^2 >= 0, exact in 128 bits, rounded once
            const unsigned __int128 a = (unsigned __int128)(uint64_t)S * u(PPC_SUM_R2);
            const unsigned __int128 b = (unsigned __int128)u(PPC_SUM_R) * u(PPC_SUM_R);
            return (double)(a - b) / ((double)S * (double)(S - 1));
        }
        case GPIRT_PPC_YES_GE: return (double)u(PPC_YES_GE);
        case GPIRT_PPC_YES_GT: return (double)u(PPC_YES_GT);
        case GPIRT_PPC_DEV_OBS_MEAN: return mean_ok ? d(PPC_DEV_OBS) / (double)S : nan;
        case GPIRT_PPC_DEV_REP_MEAN: return mean_ok ? d(PPC_DEV_REP) / (double)S : nan;
        case GPIRT_PPC_DEV_GE: return (double)u(PPC_DEV_GE);
        case GPIRT_PPC_CORRECT_MEAN: return mean_ok ? (double)u(PPC_CORRECT) / (double)S : nan;
        case GPIRT_PPC_NONFINITE: return (double)u(PPC_NONFINITE);
        case GPIRT_PPC_DRAWS: return (double)draws;
        case GPIRT_PPC_REP_YES_SUM: return (double)u(PPC_SUM_R);
        case GPIRT_PPC_REP_YES_SUMSQ: return (double)u(PPC_SUM_R2);
        case GPIRT_PPC_CORRECT_SUM: return (double)u(PPC_CORRECT);
    }
    return nan;
}

}  // namespace

int64_t ppc_stride(int64_t n, int64_t m) { return (n + m + 1 + 1) & ~(int64_t)1; }
int64_t ppc_state_words(int64_t n, int64_t m) { return PPC_HEADER_WORDS + (int64_t)PPC_NARRAYS * ppc_stride(n, m); }

int ppc_alloc(hipStream_t st, PpcState* s, int64_t n, int64_t m, int64_t item0, const double* y)
{
    auto get = [&](void** p, size_t bytes) -> int {
        GP_HIP(hipMalloc(p, bytes ? bytes : 8));
        s->allocs.push_back(*p);
        GP_HIP(hipMemsetAsync(*p, 0, bytes ? bytes : 8, st));
        return 0;
    };
    s->n = n; s->m = m; s->item0 = item0; s->draws = 0;
    s->stride = ppc_stride(n, m);
    s->strips = (int)((m + PPC_STRIP - 1) / PPC_STRIP);
    s->rblocks = (int)((n + PPC_THREADS - 1) / PPC_THREADS);
    const size_t N = (size_t)n, M = (size_t)m;
    GP_TRY(get((void**)&s->block, sizeof(uint64_t) * (size_t)ppc_state_words(n, m)));
    GP_TRY(get((void**)&s->rowd, sizeof(double) * (size_t)s->strips * 3 * N));
    GP_TRY(get((void**)&s->rowi, sizeof(uint32_t) * (size_t)s->strips * N));
    GP_TRY(get((void**)&s->cold, sizeof(double) * (size_t)s->rblocks * 3 * M));
    GP_TRY(get((void**)&s->coli, sizeof(uint32_t) * (size_t)s->rblocks * M));
    GP_TRY(get((void**)&s->unit_d, sizeof(double) * 3 * M));
    GP_TRY(get((void**)&s->unit_i, sizeof(uint64_t) * 3 * M));
    uint64_t* acc = s->block + PPC_HEADER_WORDS;
    hipLaunchKernelGGL(ppc_observed_kernel, dim3((unsigned)((n + m + PPC_THREADS - 1) / PPC_THREADS)), dim3(PPC_THREADS), 0, st,
                       y, n, m, s->stride, acc);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(ppc_observed_total_kernel, dim3(1), dim3(64), 0, st, n, m, s->stride, acc);
    GP_HIP(hipGetLastError());
    s->on = true;
    return ppc_seal(st, s);
}

void ppc_free(PpcState* s)
{
    pair_free(&s->pairs);
    bin_free(&s->bins);
    dif_free(&s->dif);
    pps_free(&s->scores);
    prs_free(&s->person);
    rsd_free(&s->resid);
    for (void* p : s->allocs) hipFree(p);
    *s = PpcState{};
}

int launch_ppc_accumulate(hipStream_t st, PpcState* s, const double* f, const double* mu, const double* y, uint64_t seed,
                          uint32_t iter, const double* theta)
{
    PpcArgs a{};
    a.f = f; a.mu = mu; a.y = y; a.n = s->n; a.m = s->m; a.seed = seed; a.iter = iter; a.item0 = (uint32_t)s->item0;
    a.rowd = s->rowd; a.rowi = s->rowi; a.cold = s->cold; a.coli = s->coli;
    const dim3 grid((unsigned)s->rblocks, (unsigned)s->strips);
    const bool bins = s->bins.on;
    if (bins) {
        BinState* b = &s->bins;
        GP_ARG(theta);
        GP_TRY(launch_bin_assign(st, b, theta));
        a.bin = b->bin_cur; a.B = b->B; a.bpi = b->part_i; a.bpe = b->part_e; a.bpv = b->part_v; a.bbad = b->ctl + 1;
    }
    if (s->pairs.on) {
        PairState* p = &s->pairs;
        a.rep8 = p->rep8; a.cur = p->ctl; a.plane = p->plane; a.ksteps = p->ksteps; a.bad = p->ctl + 1;
        GP_HIP(hipMemsetAsync(p->ctl + 1, 0, sizeof(int), st));
        if (bins) hipLaunchKernelGGL((ppc_replicate_kernel<true, true>), grid, dim3(PPC_THREADS), PPC_STAGE_BYTES, st, a);
        else hipLaunchKernelGGL((ppc_replicate_kernel<true, false>), grid, dim3(PPC_THREADS), PPC_STAGE_BYTES, st, a);
    } else if (bins)
        hipLaunchKernelGGL((ppc_replicate_kernel<false, true>), grid, dim3(PPC_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((ppc_replicate_kernel<false, false>), grid, dim3(PPC_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    PpcUnitArgs u{};
    u.rowd = s->rowd; u.rowi = s->rowi; u.cold = s->cold; u.coli = s->coli;
    u.n = s->n; u.m = s->m; u.stride = s->stride; u.strips = s->strips; u.rblocks = s->rblocks;
    u.acc = s->block + PPC_HEADER_WORDS; u.unit_d = s->unit_d; u.unit_i = s->unit_i;
    hipLaunchKernelGGL(ppc_units_kernel, dim3((unsigned)((s->n + s->m + PPC_THREADS - 1) / PPC_THREADS)), dim3(PPC_THREADS), 0,
                       st, u);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(ppc_total_kernel, dim3(1), dim3(PPC_THREADS), 0, st, u);
    GP_HIP(hipGetLastError());
    s->draws += 1;
    if (s->pairs.on) GP_TRY(launch_pair_accumulate(st, &s->pairs));
    if (bins) GP_TRY(launch_bin_update(st, &s->bins));
    if (s->dif.on) GP_TRY(launch_dif_accumulate(st, &s->dif, f, mu, y, seed, iter, theta));     // (ppc_dif.hip: launches of its own)
    if (s->scores.on) GP_TRY(launch_pps_accumulate(st, &s->scores, f, mu, y, seed, iter));       // (ppc_scores.hip: likewise)
    if (s->person.on) GP_TRY(launch_prs_accumulate(st, &s->person, f, mu, y, seed, iter));       // (ppc_person.hip: likewise)
    if (s->resid.on) GP_TRY(launch_rsd_accumulate(st, &s->resid, f, mu, y, seed, iter));         // (ppc_resid.hip: likewise)
    return 0;
}

int ppc_seal(hipStream_t st, PpcState* s)
{
    int64_t hdr[PPC_HEADER_WORDS] = { s->n, s->m, s->draws, PPC_LAYOUT_VERSION, s->item0, 0, 0, 0 };
    GP_HIP(hipMemcpyAsync(s->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));       // hdr is on this stack
    return 0;
}

int ppc_field_index(const char* name)
{
    for (int k = 0; k < GPIRT_PPC_NFIELDS; ++k)
        if (strcmp(kFieldNames[k], name) == 0) return k;
    return -1;
}

int ppc_fetch(hipStream_t st, PpcState* s, std::vector<uint64_t>& host)
{
    GP_TRY(ppc_seal(st, s));
    host.resize((size_t)ppc_state_words(s->n, s->m));
    GP_HIP(hipMemcpyAsync(host.data(), s->block, sizeof(uint64_t) * host.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

void ppc_fill(const uint64_t* blk, int fld, bool respondents, double* out, int64_t count)
{
    const int64_t m = (int64_t)blk[1];
    for (int64_t k = 0; k < count; ++k) out[k] = ppc_field(blk, fld, respondents ? m + k : k);
}

void ppc_fill_totals(const uint64_t* blk, double* out)
{
    const int64_t n = (int64_t)blk[0], m = (int64_t)blk[1];
    for (int fld = 0; fld < GPIRT_PPC_NFIELDS; ++fld) out[fld] = ppc_field(blk, fld, m + n);
}

void ppc_fill_struct(const uint64_t* blk, gpirt_ppc* out)
{
    const int64_t n = (int64_t)blk[0], m = (int64_t)blk[1];
    for (int fld = 0; fld < GPIRT_PPC_NFIELDS; ++fld) {
        if (out->item[fld]) ppc_fill(blk, fld, false, out->item[fld], m);
        if (out->respondent[fld]) ppc_fill(blk, fld, true, out->respondent[fld], n);
    }
    ppc_fill_totals(blk, out->totals);
}

int ppc_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    hipStream_t st = h->stream;
    std::vector<uint64_t> pooled, one;
    for (int c = 0; c < chains; ++c) {
        int64_t hdr[PPC_HEADER_WORDS];
        GP_HIP(hipMemcpyAsync(hdr, d_states[c], sizeof(hdr), hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        if (hdr[0] <= 0 || hdr[1] <= 0 || hdr[2] < 0 || hdr[3] != PPC_LAYOUT_VERSION) {
            set_error("gpirt_ppc_combine: state %d is not a PPC state block of layout %d", c, PPC_LAYOUT_VERSION);
            return GPIRT_E_ARG;
        }
        const size_t words = (size_t)ppc_state_words(hdr[0], hdr[1]);
        std::vector<uint64_t>& dst = c == 0 ? pooled : one;
        if (c > 0 && ((int64_t)pooled[0] != hdr[0] || (int64_t)pooled[1] != hdr[1] || (int64_t)pooled[4] != hdr[4])) {
            set_error("gpirt_ppc_combine: state %d has another n, m or item0 than state 0", c);
            return GPIRT_E_ARG;
        }
        dst.resize(words);
        GP_HIP(hipMemcpyAsync(dst.data(), d_states[c], sizeof(uint64_t) * words, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        if (c == 0) continue;
        const int64_t stride = ppc_stride(hdr[0], hdr[1]), units = hdr[0] + hdr[1] + 1;
        uint64_t* pa = pooled.data() + PPC_HEADER_WORDS;
        const uint64_t* oa = one.data() + PPC_HEADER_WORDS;
        for (int64_t k = 0; k < units; ++k) {
            if (pa[PPC_N_OBS * stride + k] != oa[PPC_N_OBS * stride + k] || pa[PPC_OBS_YES * stride + k] != oa[PPC_OBS_YES * stride + k]) {
                set_error("gpirt_ppc_combine: state %d was accumulated on another response matrix than state 0", c);
                return GPIRT_E_ARG;
            }
            for (int arr = PPC_SUM_R; arr <= PPC_NONFINITE; ++arr) pa[arr * stride + k] += oa[arr * stride + k];
            for (int arr = PPC_DEV_OBS; arr <= PPC_DEV_REP; ++arr) {       // the double sums, in chain order
                double x, y2;
                memcpy(&x, &pa[arr * stride + k], 8); memcpy(&y2, &oa[arr * stride + k], 8);
                x += y2;
                memcpy(&pa[arr * stride + k], &x, 8);
            }
        }
        pooled[2] += (uint64_t)hdr[2];
    }
    ppc_fill_struct(pooled.data(), out);
    return 0;
}

}  // namespace gpirt
