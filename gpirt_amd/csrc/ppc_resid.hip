// ppc_resid.hip -- residual correlations of the posterior predictive checks (include/gpirt_hip.h, "residual correlations in the
// PPC"): per draw the residual correlation of every item pair, the infit of every item, each item's share
// in the dependence and three global statistics, for the data and for that draw's replicate, accumulated without stored draws.
//
// The terms dt_obs, dt_rep (in [-2^22, 2^22]) and wt (in [0, 2^20]) are integers in units of 2^-22, split in three balanced
// base-256 digits.  resid_terms_kernel reads f, mu and y once (lanes along respondents, RT_ITEMS items per work-group), forms the
// PPC's replicate again bit for bit and leaves the nine int8 digit planes in the operand layout of ppc_pairs.hip
//     X8 [j / 32][k / 32][lane = (j % 32) + 32 ((k % 32) / 16)][k % 16]
// through LDS, so that the stores are the layout's 16-byte pieces.  resid_products_kernel: a work-group owns 128 x 128 pairs of
// ONE of S_obs, S_rep and V and runs through its digit-plane pairs (u, v) -- nine for S, three for V = W^T O --, each a pass of
// ppc_pairs.hip's pipeline (two LDS stages of RP_KS k-steps, the next chunk travelling global -> registers under this chunk's 16
// MFMAs per wave and registers -> the other stage behind them, one barrier per chunk); after each pass the int32 tile is joined
// into the int64 one with the weight 256^(u + v), in registers: the int32 partials never go to memory.  The depth of S_obs and of
// S_rep is split in two halves, each a work-group of its own whose int64 tile resid_update_kernel adds to the other's (integer
// sums: exact in any order), so that a tile's 9 passes become two work-groups of 4.5 beside V's 3.  Of S only the tiles on and
// below the diagonal are computed: with ALL nine ordered plane pairs summed on a tile, X_u^T X_v and its mirror X_v^T X_u are both
// there, so no transposed tile is needed, and the work is the 4.5 full products of the triangular scheme; the owner stores both
// triangles.  resid_update_kernel: one thread per ordered pair (the diagonal cell is the item's infit) decides on the integers and
// owns its sums.  resid_items_kernel: one wave per item, lane l summing b = l, l + 64, ... in ascending order and lane 0 the 64
// lane sums in lane order; resid_global_kernel sums the items' parts in the same order over a.  No atomics anywhere.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace gpirt {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int RP_KS = 4;                          // k-steps (of 32 respondents) per LDS stage
constexpr int RP_TILE = 128;                      // items per side of a work-group's tile
constexpr int RP_STAGE = 8 * RP_KS * 1024;        // four item blocks of each operand, bytes
constexpr int RT_THREADS = 256;                   // respondents per work-group of the terms kernel: 8 k-steps
constexpr int RT_ITEMS = 16;                      // items per work-group of the terms kernel: half an item block
constexpr int RSD_SETS = 2, RSD_PLANES = 9;
constexpr double RSD_UNIT = 4194304.0;            // 2^22
static_assert(2 * RP_STAGE <= 64 * 1024, "two stages in the LDS a work-group may ask for");
static_assert(RT_THREADS % (32 * RP_KS) == 0, "the terms kernel's 256 respondents are whole chunks");
static_assert((int64_t)GPIRT_RESID_MAX_N * 128 * 128 < ((int64_t)1 << 31), "a digit-plane product fits int32");
// sum over the nine plane pairs of |d_u| |d_v| 256^(u + v) <= (128 + 128 x 256 + 64 x 65536)^2 per respondent
static_assert((long double)GPIRT_RESID_MAX_N * (128.0L + 128.0L * 256.0L + 64.0L * 65536.0L) * (128.0L + 128.0L * 256.0L + 64.0L * 65536.0L) <
                  9.2e18L, "every partial sum of the joined products fits int64");

const char* const kResidPair[GPIRT_RESID_NPAIR] = { "n_co", "rc_obs_mean", "rc_rep_mean", "rc_rep_sd", "ppp_rc", "ppp_rc_mid", "undefined" };
const char* const kResidItem[GPIRT_RESID_NITEM] = { "infit_obs_mean", "infit_rep_mean", "infit_rep_sd", "ppp_infit", "ppp_infit_mid",
                                                    "ss_obs_mean", "ss_rep_mean", "ppp_ss", "ppp_ss_mid" };
const char* const kResidRaw[RSD_NARRAYS] = { "n_co_int", "undefined_count", "rc_ge", "rc_gt", "rc_obs_sum", "rc_rep_sum", "rc_rep_sumsq",
                                             "ss_undefined", "ss_ge", "ss_gt", "ss_obs_sum", "ss_rep_sum", "global" };

__device__ __forceinline__ uint32_t pack4(int b0, int b1, int b2, int b3)
{
    return (uint32_t)b0 | ((uint32_t)b1 << 8) | ((uint32_t)b2 << 16) | ((uint32_t)b3 << 24);
}

// O8 (once, at enable): one thread per 16-byte piece
__global__ __launch_bounds__(256) void resid_observed_kernel(const double* __restrict__ y, int64_t n, int64_t m, int64_t iblocks,
                                                             int64_t ksteps, uint4* __restrict__ O8)
{
    const int64_t total = iblocks * ksteps * 64;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int lane = (int)(t & 63);
        const int64_t ks = (t >> 6) % ksteps, ib = (t >> 6) / ksteps;
        const int64_t j = ib * 32 + (lane & 31), i0 = ks * 32 + 16 * (lane >> 5);
        int o[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            double v = (double)NAN;
            if (j < m && i0 + q < n) v = y[i0 + q + j * n];
            o[q] = v == v ? 1 : 0;
        }
        O8[t] = make_uint4(pack4(o[0], o[1], o[2], o[3]), pack4(o[4], o[5], o[6], o[7]), pack4(o[8], o[9], o[10], o[11]),
                           pack4(o[12], o[13], o[14], o[15]));
    }
}

struct ResidTermArgs {
    const double* f; const double* mu; const double* y;
    int64_t n, m;
    uint64_t seed; uint32_t iter, item0;
    signed char* dig; const int* cur;    // the planes of the set *cur does NOT name are written
    int64_t plane, ksteps;
    int* bad;                            // raised by a NaN g in an observed cell
};

// x in [-2^22, 2^22] = d0 + 256 d1 + 65536 d2, d0 and d1 in [-128, 127], |d2| <= 64
__device__ __forceinline__ void resid_split(int x, signed char* d0, signed char* d1, signed char* d2)
{
    const int a0 = ((x + 128) & 255) - 128, x1 = (x - a0) >> 8;
    const int a1 = ((x1 + 128) & 255) - 128;
    *d0 = (signed char)a0; *d1 = (signed char)a1; *d2 = (signed char)((x1 - a1) >> 8);
}

__global__ __launch_bounds__(RT_THREADS) void resid_terms_kernel(ResidTermArgs a)
{
    __shared__ __attribute__((aligned(16))) signed char st[RSD_PLANES][RT_ITEMS][RT_THREADS];
    const int rb = blockIdx.x, strip = blockIdx.y, tid = (int)threadIdx.x;
    const int64_t i = (int64_t)rb * RT_THREADS + tid;
    const int64_t j0 = (int64_t)strip * RT_ITEMS;
    for (int jj = 0; jj < RT_ITEMS; ++jj) {
        int dobs = 0, drep = 0, wt = 0;
        const int64_t j = j0 + jj;
        if (i < a.n && j < a.m) {
            const int64_t c = i + j * a.n;
            const double yv = a.y[c];
            if (yv == yv) {                                   // an observed cell
                const double g = a.f[c] + a.mu[c];
                if (g != g) *a.bad = 1;                       // (every writer stores the same word)
                else {
                    const double e = exp(-fabs(g));
                    const double p = g >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
                    const double q = g >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);
                    const double u = item_uniform(a.seed, a.iter, GPIRT_ST_PPC, (uint32_t)(a.item0 + j), (uint32_t)i);
                    dobs = (int)rint((yv > 0.0 ? q : -p) * RSD_UNIT);
                    drep = (int)rint((u < p ? q : -p) * RSD_UNIT);
                    wt = (int)rint((p * q) * RSD_UNIT);
                }
            }
        }
        resid_split(dobs, &st[0][jj][tid], &st[1][jj][tid], &st[2][jj][tid]);
        resid_split(drep, &st[3][jj][tid], &st[4][jj][tid], &st[5][jj][tid]);
        resid_split(wt, &st[6][jj][tid], &st[7][jj][tid], &st[8][jj][tid]);
    }
    __syncthreads();
    // thread = (k-step kk of the work-group, half of the k-step, item jj): one 16-byte piece of every plane
    const int kk = tid >> 5, half = (tid >> 4) & 1, jj = tid & 15;
    const int64_t piece = (((int64_t)(strip >> 1) * a.ksteps + (int64_t)rb * 8 + kk) * 64 + (strip & 1) * 16 + jj + 32 * half) * 16;
    signed char* dst = a.dig + (int64_t)(*a.cur ^ 1) * RSD_PLANES * a.plane + piece;
#pragma unroll
    for (int pl = 0; pl < RSD_PLANES; ++pl)
        *reinterpret_cast<uint4*>(dst + pl * a.plane) = *reinterpret_cast<const uint4*>(&st[pl][jj][kk * 32 + half * 16]);
}

// operand kinds of a job: 0, 1, 2 = the three planes of d_obs, d_rep, w in the set of this draw; 3 = O8 (one plane); a job
// covers the chunks [c0, c0 + nc) of the depth
struct ResidJob { int a_kind, b_kind, lower, c0, nc; int64_t* out; };
constexpr int RSD_MAX_JOBS = 5;
struct ResidProdArgs {
    ResidJob job[RSD_MAX_JOBS];
    const signed char* dig; const signed char* O8;
    const int* cur;                      // non-null: this draw's set is the one *cur does NOT name
    const int* skip;                     // non-null and *skip != 0: this draw is skipped, nothing is written
    int64_t plane, ksteps, m;
};

// register v of lane l of an accumulator tile: item a = (v & 3) + 8 (v >> 2) + 4 (l >> 5) of the first operand's block,
// item b = l & 31 of the second's
__global__ __launch_bounds__(256) void resid_products_kernel(ResidProdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rp_lds[];
    const int ab = (int)blockIdx.x, bb = (int)blockIdx.y;
    const ResidJob job = a.job[blockIdx.z];
    if (job.lower && bb > ab) return;                 // the mirror of a tile below the diagonal
    if (a.skip && *a.skip) return;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wa = wave >> 1, wb = wave & 1;
    const signed char* set = a.dig + (a.cur ? (int64_t)(*a.cur ^ 1) * RSD_PLANES * a.plane : 0);
    const signed char* A = job.a_kind < 3 ? set + (int64_t)job.a_kind * 3 * a.plane : a.O8;
    const signed char* B = job.b_kind < 3 ? set + (int64_t)job.b_kind * 3 * a.plane : a.O8;
    const int nA = job.a_kind < 3 ? 3 : 1, nB = job.b_kind < 3 ? 3 : 1;
    const int64_t ksteps = a.ksteps;
    const int nchunks = job.nc;
    const int64_t first = (int64_t)job.c0 * RP_KS * 1024 + tid * 16;
    int64_t tot[2][2][16];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int v = 0; v < 16; ++v) tot[r][c][v] = 0;
    for (int u = 0; u < nA; ++u)
        for (int w = 0; w < nB; ++w) {
            // block q < 4: item block 4 ab + q of plane u of A; q >= 4: item block 4 bb + q - 4 of plane w of B; a chunk of a
            // block is RP_KS KiB in a row
            const signed char* src[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                src[q] = A + (int64_t)u * a.plane + ((int64_t)(4 * ab + q) * ksteps) * 1024 + first;
                src[4 + q] = B + (int64_t)w * a.plane + ((int64_t)(4 * bb + q) * ksteps) * 1024 + first;
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
            // (stage 0 was last read in the pass before, whose last chunk ended on a barrier)
#pragma unroll
            for (int q = 0; q < 8; ++q) *reinterpret_cast<v4i*>(rp_lds + q * (RP_KS * 1024) + tid * 16) = nx[q];
            __syncthreads();
            for (int c = 0; c < nchunks; ++c) {
                const unsigned char* st = rp_lds + (c & 1) * RP_STAGE + lane * 16;
                const bool more = c + 1 < nchunks;
                if (more) {
                    const int64_t adv = (int64_t)(c + 1) * RP_KS * 1024;
#pragma unroll
                    for (int q = 0; q < 8; ++q) nx[q] = *reinterpret_cast<const v4i*>(src[q] + adv);
                }
#pragma unroll
                for (int ks = 0; ks < RP_KS; ++ks) {
                    const v4i a0 = *reinterpret_cast<const v4i*>(st + ((2 * wa) * RP_KS + ks) * 1024);
                    const v4i a1 = *reinterpret_cast<const v4i*>(st + ((2 * wa + 1) * RP_KS + ks) * 1024);
                    const v4i b0 = *reinterpret_cast<const v4i*>(st + ((4 + 2 * wb) * RP_KS + ks) * 1024);
                    const v4i b1 = *reinterpret_cast<const v4i*>(st + ((5 + 2 * wb) * RP_KS + ks) * 1024);
                    acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
                }
                if (more) {
                    unsigned char* sn = rp_lds + ((c + 1) & 1) * RP_STAGE + tid * 16;     // (last read in chunk c - 1, before its barrier)
#pragma unroll
                    for (int q = 0; q < 8; ++q) *reinterpret_cast<v4i*>(sn + q * (RP_KS * 1024)) = nx[q];
                }
                __syncthreads();
            }
            const int64_t weight = (int64_t)1 << (8 * (u + w));
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int v = 0; v < 16; ++v) tot[r][c][v] += (int64_t)acc[r][c][v] * weight;
        }
    const bool mirror = job.lower && bb < ab;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int64_t pb = (int64_t)bb * RP_TILE + (2 * wb + c) * 32 + (lane & 31);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int64_t pa = (int64_t)ab * RP_TILE + (2 * wa + r) * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
                if (pa < a.m && pb < a.m) {
                    job.out[pa * a.m + pb] = tot[r][c][v];
                    if (mirror) job.out[pb * a.m + pa] = tot[r][c][v];
                }
            }
        }
}

struct ResidUpdateArgs {
    const int64_t* s_obs; const int64_t* s_rep; const int64_t* v; const int64_t* n_co;
    uint32_t* undef; uint32_t* ge; uint32_t* gt;
    double* sum_obs; double* sum_rep; double* sumsq_rep;
    double* r_obs; double* r_rep;
    int64_t* hdr;                        // the block's header: [3] resid_draws, [4] resid_skipped
    int* ctl;                            // [0] the set of the last counted draw, [1] this draw holds a NaN g
    int64_t m;
};

__global__ __launch_bounds__(256) void resid_update_kernel(ResidUpdateArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool bad = a.ctl[1] != 0;
    if (idx == 0) {                                   // (nobody else in this launch reads ctl[0] or the header)
        if (bad) a.hdr[4] += 1;
        else { a.hdr[3] += 1; a.ctl[0] ^= 1; }
    }
    if (bad || idx >= a.m * a.m) return;
    const int64_t pa = idx / a.m, pb = idx - pa * a.m, tr = pb * a.m + pa;
    double ro = (double)NAN, rr = (double)NAN;
    if (a.n_co[idx] > 0) {
        const int64_t vab = a.v[idx], vba = a.v[tr];
        if (vab == 0 || vba == 0) a.undef[idx] += 1;
        else {
            const double den = pa == pb ? (double)vab * RSD_UNIT : sqrt((double)vab * (double)vba) * RSD_UNIT;
            const int64_t P = a.m * a.m;
            const int64_t so = a.s_obs[idx] + a.s_obs[P + idx], sr = a.s_rep[idx] + a.s_rep[P + idx];      // the halves of the depth
            ro = (double)so / den;
            rr = (double)sr / den;
            a.sum_obs[idx] += ro;
            a.sum_rep[idx] += rr;
            a.sumsq_rep[idx] += rr * rr;
            a.ge[idx] += sr >= so ? 1u : 0u;
            a.gt[idx] += sr > so ? 1u : 0u;
        }
    }
    a.r_obs[idx] = ro;
    a.r_rep[idx] = rr;
}

struct ResidItemArgs {
    const double* r_obs; const double* r_rep;
    uint32_t* ss_undef; uint32_t* ss_ge; uint32_t* ss_gt; double* ss_obs; double* ss_rep;
    double* part;                        // [RSD_ITEM_PARTS][m]: t_obs, t_rep, u_obs, u_rep, M+_obs, M+_rep, M_obs, M_rep, #t, #u
    uint64_t* global; double* stats;
    const int* ctl;
    int64_t m;
};

// lane l's eight partial values in, the sums of the 64 lanes in lane order (sums) and their maxima out, on lane 0
__device__ __forceinline__ void resid_join_lanes(double (*sh)[64], int lane, double* val)
{
#pragma unroll
    for (int q = 0; q < RSD_ITEM_PARTS; ++q) sh[q][lane] = val[q];
    __syncthreads();
    if (lane != 0) return;
    for (int q = 0; q < RSD_ITEM_PARTS; ++q) {
        const bool is_max = q >= 4 && q < 8;
        double x = sh[q][0];
        for (int l = 1; l < 64; ++l) x = is_max ? fmax(x, sh[q][l]) : x + sh[q][l];
        val[q] = x;
    }
}

// one wave per item a: row a of r (r is symmetric bit for bit), lane l taking b = l, l + 64, ... in ascending order
__global__ __launch_bounds__(64) void resid_items_kernel(ResidItemArgs a)
{
    __shared__ double sh[RSD_ITEM_PARTS][64];
    if (a.ctl[1] != 0) return;
    const int64_t ia = blockIdx.x, m = a.m;
    const int lane = (int)threadIdx.x;
    const double ninf = -(double)INFINITY;
    double val[RSD_ITEM_PARTS] = { 0.0, 0.0, 0.0, 0.0, ninf, ninf, ninf, ninf, 0.0, 0.0 };
    for (int64_t b = lane; b < m; b += 64) {
        if (b == ia) continue;
        const double ro = a.r_obs[ia * m + b];
        if (ro != ro) continue;                       // undefined in this draw (the replicate's is NaN with it)
        const double rr = a.r_rep[ia * m + b];
        const double so = ro * ro, sr = rr * rr;
        val[0] += so; val[1] += sr; val[8] += 1.0;
        if (b > ia) {
            val[2] += so; val[3] += sr; val[9] += 1.0;
            val[4] = fmax(val[4], ro); val[5] = fmax(val[5], rr);
            val[6] = fmax(val[6], fabs(ro)); val[7] = fmax(val[7], fabs(rr));
        }
    }
    resid_join_lanes(sh, lane, val);
    if (lane != 0) return;
#pragma unroll
    for (int q = 0; q < RSD_ITEM_PARTS; ++q) a.part[q * m + ia] = val[q];
    if (val[8] == 0.0) a.ss_undef[ia] += 1;
    else {
        a.ss_obs[ia] += val[0];
        a.ss_rep[ia] += val[1];
        a.ss_ge[ia] += val[1] >= val[0] ? 1u : 0u;
        a.ss_gt[ia] += val[1] > val[0] ? 1u : 0u;
    }
}

// the whole matrix from the items' parts: lane l taking a = l, l + 64, ... in ascending order, lane 0 the 64 lanes in order
__global__ __launch_bounds__(64) void resid_global_kernel(ResidItemArgs a)
{
    __shared__ double sh[RSD_ITEM_PARTS][64];
    if (a.ctl[1] != 0) return;
    const int lane = (int)threadIdx.x;
    const int64_t m = a.m;
    const double ninf = -(double)INFINITY;
    double val[RSD_ITEM_PARTS] = { 0.0, 0.0, 0.0, 0.0, ninf, ninf, ninf, ninf, 0.0, 0.0 };
    for (int64_t ia = lane; ia < m; ia += 64) {
        val[2] += a.part[2 * m + ia]; val[3] += a.part[3 * m + ia]; val[9] += a.part[9 * m + ia];
#pragma unroll
        for (int q = 4; q < 8; ++q) val[q] = fmax(val[q], a.part[q * m + ia]);
    }
    resid_join_lanes(sh, lane, val);
    if (lane != 0) return;
    double* gd = reinterpret_cast<double*>(a.global);
    const double stat[8] = { val[2], val[4], val[6], val[3], val[5], val[7], val[9], 0.0 };      // Q, M+, M: data, replicate
#pragma unroll
    for (int q = 0; q < 8; ++q) a.stats[q] = stat[q];
    if (val[9] == 0.0) { a.global[13] += 1; return; }
    gd[0] += stat[0]; gd[1] += stat[3]; gd[2] += stat[3] * stat[3];
    gd[3] += stat[1]; gd[4] += stat[4];
    gd[5] += stat[2]; gd[6] += stat[5];
    for (int k = 0; k < 3; ++k) {
        a.global[7 + 2 * k] += stat[3 + k] >= stat[k] ? 1 : 0;
        a.global[8 + 2 * k] += stat[3 + k] > stat[k] ? 1 : 0;
    }
}

int launch_products(hipStream_t st, const RsdState* p, bool draw)
{
    ResidProdArgs a{};
    a.dig = p->dig; a.O8 = p->O8; a.plane = p->plane; a.ksteps = p->ksteps; a.m = p->m;
    const unsigned nab = (unsigned)(p->iblocks / 4);
    const int nchunks = (int)(p->ksteps / RP_KS), half = nchunks / 2;      // (ksteps is a multiple of 8: nchunks is even)
    const int64_t P = p->m * p->m;
    unsigned jobs = 1;
    if (draw) {
        // the nine passes of S_obs and of S_rep in two halves of the depth each, beside the three of V: five jobs of 4.5, 4.5,
        // 4.5, 4.5 and 3 passes per tile in place of 9, 9 and 3; resid_update_kernel adds the halves
        a.cur = p->ctl; a.skip = p->ctl + 1;
        a.job[0] = ResidJob{ 0, 0, 1, 0, half, p->s_obs };
        a.job[1] = ResidJob{ 0, 0, 1, half, nchunks - half, p->s_obs + P };
        a.job[2] = ResidJob{ 1, 1, 1, 0, half, p->s_rep };
        a.job[3] = ResidJob{ 1, 1, 1, half, nchunks - half, p->s_rep + P };
        a.job[4] = ResidJob{ 2, 3, 0, 0, nchunks, p->v };
        jobs = RSD_MAX_JOBS;
    } else
        a.job[0] = ResidJob{ 3, 3, 1, 0, nchunks, reinterpret_cast<int64_t*>(p->block + rsd_layout(p->m).off[RSD_N_CO]) };
    hipLaunchKernelGGL(resid_products_kernel, dim3(nab, nab, jobs), dim3(256), 2 * RP_STAGE, st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

// a state block on the host
struct HostResid {
    std::vector<uint64_t> w;
    int64_t n = 0, m = 0;
    RsdLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    template <class T> T* arr(int k) { return reinterpret_cast<T*>(w.data() + L.off[k]); }
    template <class T> const T* arr(int k) const { return reinterpret_cast<const T*>(w.data() + L.off[k]); }
};

int resid_read(hipStream_t st, const void* d_state, HostResid& r, const char* who, int c)
{
    int64_t hdr[RSD_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[7] != RSD_TAG || hdr[2] != RSD_LAYOUT_VERSION || hdr[0] <= 0 || hdr[0] > GPIRT_RESID_MAX_N || hdr[1] < 2 ||
        hdr[1] > GPIRT_RESID_MAX_M || hdr[3] < 0 || hdr[4] < 0) {
        set_error("%s: state %d is not a residual PPC state block of layout %d", who, c, RSD_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[0]; r.m = hdr[1];
    r.L = rsd_layout(r.m);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

struct ResidFin { double obs_mean, rep_mean, rep_sd, ppp, ppp_mid; };

// the finished values of one statistic from its sums and counts over D draws
ResidFin resid_finish(double so, double sr, double sq, uint64_t ge, uint64_t gt, int64_t D)
{
    const double nan = (double)NAN;
    ResidFin f{ nan, nan, nan, nan, nan };
    if (D < 1) return f;
    const double dD = (double)D;
    f.obs_mean = so / dD;
    f.rep_mean = sr / dD;
    if (D >= 2) {
        const double var = (sq - sr * f.rep_mean) / (double)(D - 1);
        f.rep_sd = var > 0.0 ? std::sqrt(var) : 0.0;
    }
    f.ppp = (double)ge / dD;
    f.ppp_mid = ((double)ge + (double)gt) / (2.0 * dD);
    return f;
}

ResidFin resid_cell(const HostResid& r, int64_t idx)
{
    const int64_t D = r.hdr()[3] - (int64_t)r.arr<uint32_t>(RSD_UNDEF)[idx];
    return resid_finish(r.arr<double>(RSD_RC_OBS_SUM)[idx], r.arr<double>(RSD_RC_REP_SUM)[idx], r.arr<double>(RSD_RC_REP_SUMSQ)[idx],
                        r.arr<uint32_t>(RSD_RC_GE)[idx], r.arr<uint32_t>(RSD_RC_GT)[idx], D);
}

double resid_pair_field(const HostResid& r, int fld, int64_t a, int64_t b)
{
    const int64_t idx = a * r.m + b;
    const int64_t nco = r.arr<int64_t>(RSD_N_CO)[idx];
    if (fld == GPIRT_RESID_P_N_CO) return (double)nco;
    if (a == b || nco == 0) return (double)NAN;
    if (fld == GPIRT_RESID_P_UNDEFINED) return (double)r.arr<uint32_t>(RSD_UNDEF)[idx];
    const ResidFin f = resid_cell(r, idx);
    switch (fld) {
        case GPIRT_RESID_P_RC_OBS_MEAN: return f.obs_mean;
        case GPIRT_RESID_P_RC_REP_MEAN: return f.rep_mean;
        case GPIRT_RESID_P_RC_REP_SD: return f.rep_sd;
        case GPIRT_RESID_P_PPP_RC: return f.ppp;
        case GPIRT_RESID_P_PPP_RC_MID: return f.ppp_mid;
        default: break;
    }
    return (double)NAN;
}

double resid_item_field(const HostResid& r, int fld, int64_t a)
{
    const int64_t idx = a * r.m + a;
    if (r.arr<int64_t>(RSD_N_CO)[idx] == 0) return (double)NAN;
    if (fld <= GPIRT_RESID_I_PPP_INFIT_MID) {
        const ResidFin f = resid_cell(r, idx);
        switch (fld) {
            case GPIRT_RESID_I_INFIT_OBS_MEAN: return f.obs_mean;
            case GPIRT_RESID_I_INFIT_REP_MEAN: return f.rep_mean;
            case GPIRT_RESID_I_INFIT_REP_SD: return f.rep_sd;
            case GPIRT_RESID_I_PPP_INFIT: return f.ppp;
            default: return f.ppp_mid;
        }
    }
    const int64_t D = r.hdr()[3] - (int64_t)r.arr<uint32_t>(RSD_SS_UNDEF)[a];
    const ResidFin f = resid_finish(r.arr<double>(RSD_SS_OBS_SUM)[a], r.arr<double>(RSD_SS_REP_SUM)[a], 0.0, r.arr<uint32_t>(RSD_SS_GE)[a],
                                    r.arr<uint32_t>(RSD_SS_GT)[a], D);
    switch (fld) {
        case GPIRT_RESID_I_SS_OBS_MEAN: return f.obs_mean;
        case GPIRT_RESID_I_SS_REP_MEAN: return f.rep_mean;
        case GPIRT_RESID_I_PPP_SS: return f.ppp;
        default: return f.ppp_mid;
    }
}

void resid_scalars(const HostResid& r, double* out)
{
    const uint64_t* g = r.arr<uint64_t>(RSD_GLOBAL);
    const double* gd = r.arr<double>(RSD_GLOBAL);
    const int64_t D = r.hdr()[3] - (int64_t)g[13];
    const ResidFin fr = resid_finish(gd[0], gd[1], gd[2], g[7], g[8], D);
    const ResidFin mx = resid_finish(gd[3], gd[4], 0.0, g[9], g[10], D);
    const ResidFin am = resid_finish(gd[5], gd[6], 0.0, g[11], g[12], D);
    out[GPIRT_RESID_S_FROB_OBS_MEAN] = fr.obs_mean; out[GPIRT_RESID_S_FROB_REP_MEAN] = fr.rep_mean; out[GPIRT_RESID_S_FROB_REP_SD] = fr.rep_sd;
    out[GPIRT_RESID_S_PPP_FROB] = fr.ppp; out[GPIRT_RESID_S_PPP_FROB_MID] = fr.ppp_mid;
    out[GPIRT_RESID_S_MAX_OBS_MEAN] = mx.obs_mean; out[GPIRT_RESID_S_MAX_REP_MEAN] = mx.rep_mean;
    out[GPIRT_RESID_S_PPP_MAX] = mx.ppp; out[GPIRT_RESID_S_PPP_MAX_MID] = mx.ppp_mid;
    out[GPIRT_RESID_S_ABSMAX_OBS_MEAN] = am.obs_mean; out[GPIRT_RESID_S_ABSMAX_REP_MEAN] = am.rep_mean;
    out[GPIRT_RESID_S_PPP_ABSMAX] = am.ppp; out[GPIRT_RESID_S_PPP_ABSMAX_MID] = am.ppp_mid;
}

void resid_fill_pair(const HostResid& r, int fld, double* out)
{
    for (int64_t a = 0; a < r.m; ++a)
        for (int64_t b = 0; b < r.m; ++b) out[a * r.m + b] = resid_pair_field(r, fld, a, b);
}

void resid_fill_item(const HostResid& r, int fld, double* out)
{
    for (int64_t a = 0; a < r.m; ++a) out[a] = resid_item_field(r, fld, a);
}

void resid_fill(const HostResid& r, gpirt_ppc_resid* out)
{
    const int64_t m = r.m;
    out->n = r.n; out->m = m; out->resid_draws = r.hdr()[3]; out->resid_skipped = r.hdr()[4];
    out->global_undefined = (int64_t)r.arr<uint64_t>(RSD_GLOBAL)[13];
    for (int fld = 0; fld < GPIRT_RESID_NPAIR; ++fld)
        if (out->pair[fld]) resid_fill_pair(r, fld, out->pair[fld]);
    for (int fld = 0; fld < GPIRT_RESID_NITEM; ++fld)
        if (out->item[fld]) resid_fill_item(r, fld, out->item[fld]);
    for (int k = 0; k < RSD_NARRAYS; ++k)
        if (out->raw[k]) memcpy(out->raw[k], r.w.data() + r.L.off[k], (size_t)r.L.bytes[k]);
    resid_scalars(r, out->scalar);
    // a stable sort of the candidates in index order by ascending mid-p: ties go to the lowest (a, b), the lowest a
    struct E { double mid; int64_t a, b; };
    if (out->worst_pairs || out->worst_ppp_rc_mid || out->worst_rc_obs_mean) {
        std::vector<E> es;
        for (int64_t a = 0; a < m; ++a)
            for (int64_t b = a + 1; b < m; ++b) {
                const double mid = resid_pair_field(r, GPIRT_RESID_P_PPP_RC_MID, a, b);
                if (mid == mid) es.push_back(E{ mid, a, b });
            }
        std::stable_sort(es.begin(), es.end(), [](const E& x, const E& y) { return x.mid < y.mid; });
        for (int t = 0; t < out->top; ++t) {
            const bool have = (size_t)t < es.size();
            if (out->worst_pairs) {
                out->worst_pairs[2 * t] = have ? es[(size_t)t].a : -1;
                out->worst_pairs[2 * t + 1] = have ? es[(size_t)t].b : -1;
            }
            if (out->worst_ppp_rc_mid) out->worst_ppp_rc_mid[t] = have ? es[(size_t)t].mid : (double)NAN;
            if (out->worst_rc_obs_mean)
                out->worst_rc_obs_mean[t] = have ? resid_pair_field(r, GPIRT_RESID_P_RC_OBS_MEAN, es[(size_t)t].a, es[(size_t)t].b) : (double)NAN;
        }
    }
    if (out->worst_items || out->worst_ppp_ss_mid) {
        std::vector<E> es;
        for (int64_t a = 0; a < m; ++a) {
            const double mid = resid_item_field(r, GPIRT_RESID_I_PPP_SS_MID, a);
            if (mid == mid) es.push_back(E{ mid, a, a });
        }
        std::stable_sort(es.begin(), es.end(), [](const E& x, const E& y) { return x.mid < y.mid; });
        for (int t = 0; t < out->top; ++t) {
            const bool have = (size_t)t < es.size();
            if (out->worst_items) out->worst_items[t] = have ? es[(size_t)t].a : -1;
            if (out->worst_ppp_ss_mid) out->worst_ppp_ss_mid[t] = have ? es[(size_t)t].mid : (double)NAN;
        }
    }
}

// plane `pl` of the set `set` out of the operand layout: out[i + j n]
void resid_unpack(const RsdState* p, const std::vector<signed char>& raw, int pl, signed char* out)
{
    const signed char* src = raw.data() + (size_t)pl * (size_t)p->plane;
    for (int64_t j = 0; j < p->m; ++j)
        for (int64_t i = 0; i < p->n; ++i)
            out[i + j * p->n] = src[(size_t)((((j >> 5) * p->ksteps + (i >> 5)) * 64 + (j & 31) + 32 * ((i & 31) >> 4)) * 16 + (i & 15))];
}

}  // namespace

RsdLayout rsd_layout(int64_t m)
{
    RsdLayout L{};
    const int64_t P = m * m;
    int64_t at = RSD_HEADER_WORDS;
    for (int k = 0; k < RSD_NARRAYS; ++k) {
        const int64_t count = k <= RSD_RC_REP_SUMSQ ? P : k == RSD_GLOBAL ? RSD_GLOBAL_WORDS : m;
        const bool narrow = (k >= RSD_UNDEF && k <= RSD_RC_GT) || (k >= RSD_SS_UNDEF && k <= RSD_SS_GT);
        L.off[k] = at;
        L.bytes[k] = count * (narrow ? 4 : 8);
        at += narrow ? (count + 3) / 4 * 2 : (count + 1) / 2 * 2;       // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int64_t rsd_state_words(int64_t m) { return rsd_layout(m).words; }

void rsd_free(RsdState* p)
{
    for (void* q : p->allocs) hipFree(q);
    *p = RsdState{};
}

int rsd_alloc(hipStream_t st, RsdState* p, int64_t n, int64_t m, int64_t item0, const double* y)
{
    if (n > GPIRT_RESID_MAX_N) {
        set_error("residual PPC: n = %lld is beyond %d respondents (a digit-plane product would leave 32 bits)", (long long)n,
                  GPIRT_RESID_MAX_N);
        return GPIRT_E_ARG;
    }
    if (m < 2 || m > GPIRT_RESID_MAX_M) {
        set_error("residual PPC: m = %lld is outside 2..%d items", (long long)m, GPIRT_RESID_MAX_M);
        return GPIRT_E_ARG;
    }
    const RsdLayout L = rsd_layout(m);
    p->n = n; p->m = m; p->item0 = item0;
    p->iblocks = (m + RP_TILE - 1) / RP_TILE * (RP_TILE / 32);
    p->ksteps = (n + RT_THREADS - 1) / RT_THREADS * (RT_THREADS / 32);
    p->plane = p->iblocks * p->ksteps * 1024;
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        p->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    const size_t P = (size_t)(m * m);
    GP_TRY(get((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&p->O8, (size_t)p->plane));
    GP_TRY(get((void**)&p->dig, (size_t)(RSD_SETS * RSD_PLANES) * (size_t)p->plane));      // (what no strip covers stays zero)
    GP_TRY(get((void**)&p->s_obs, 2 * 8 * P));       // (two halves of the depth each)
    GP_TRY(get((void**)&p->s_rep, 2 * 8 * P));
    GP_TRY(get((void**)&p->v, 8 * P));
    GP_TRY(get((void**)&p->r_obs, 8 * P));
    GP_TRY(get((void**)&p->r_rep, 8 * P));
    GP_TRY(get((void**)&p->item_part, 8 * (size_t)RSD_ITEM_PARTS * (size_t)m));
    GP_TRY(get((void**)&p->stats, 8 * 8));
    GP_TRY(get((void**)&p->ctl, sizeof(int) * 4));
    const int64_t hdr[RSD_HEADER_WORDS] = { n, m, RSD_LAYOUT_VERSION, 0, 0, item0, 0, RSD_TAG };
    GP_HIP(hipMemcpyAsync(p->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // hdr is this call's: nothing below may leave with the copy pending
    int64_t blocks = (p->iblocks * p->ksteps * 64 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(resid_observed_kernel, dim3((unsigned)blocks), dim3(256), 0, st, y, n, m, p->iblocks, p->ksteps,
                       reinterpret_cast<uint4*>(p->O8));
    GP_HIP(hipGetLastError());
    GP_TRY(launch_products(st, p, false));
    p->on = true;
    return 0;
}

int launch_rsd_accumulate(hipStream_t st, RsdState* p, const double* f, const double* mu, const double* y, uint64_t seed, uint32_t iter)
{
    const RsdLayout L = rsd_layout(p->m);
    const int64_t m = p->m;
    GP_HIP(hipMemsetAsync(p->ctl + 1, 0, sizeof(int), st));
    ResidTermArgs t{};
    t.f = f; t.mu = mu; t.y = y; t.n = p->n; t.m = m; t.seed = seed; t.iter = iter; t.item0 = (uint32_t)p->item0;
    t.dig = p->dig; t.cur = p->ctl; t.plane = p->plane; t.ksteps = p->ksteps; t.bad = p->ctl + 1;
    hipLaunchKernelGGL(resid_terms_kernel, dim3((unsigned)(p->ksteps / 8), (unsigned)((m + RT_ITEMS - 1) / RT_ITEMS)), dim3(RT_THREADS), 0,
                       st, t);
    GP_HIP(hipGetLastError());
    GP_TRY(launch_products(st, p, true));
    ResidUpdateArgs u{};
    u.s_obs = p->s_obs; u.s_rep = p->s_rep; u.v = p->v; u.n_co = reinterpret_cast<const int64_t*>(p->block + L.off[RSD_N_CO]);
    u.undef = reinterpret_cast<uint32_t*>(p->block + L.off[RSD_UNDEF]);
    u.ge = reinterpret_cast<uint32_t*>(p->block + L.off[RSD_RC_GE]);
    u.gt = reinterpret_cast<uint32_t*>(p->block + L.off[RSD_RC_GT]);
    u.sum_obs = reinterpret_cast<double*>(p->block + L.off[RSD_RC_OBS_SUM]);
    u.sum_rep = reinterpret_cast<double*>(p->block + L.off[RSD_RC_REP_SUM]);
    u.sumsq_rep = reinterpret_cast<double*>(p->block + L.off[RSD_RC_REP_SUMSQ]);
    u.r_obs = p->r_obs; u.r_rep = p->r_rep;
    u.hdr = reinterpret_cast<int64_t*>(p->block); u.ctl = p->ctl; u.m = m;
    hipLaunchKernelGGL(resid_update_kernel, dim3((unsigned)((m * m + 255) / 256)), dim3(256), 0, st, u);
    GP_HIP(hipGetLastError());
    ResidItemArgs it{};
    it.r_obs = p->r_obs; it.r_rep = p->r_rep;
    it.ss_undef = reinterpret_cast<uint32_t*>(p->block + L.off[RSD_SS_UNDEF]);
    it.ss_ge = reinterpret_cast<uint32_t*>(p->block + L.off[RSD_SS_GE]);
    it.ss_gt = reinterpret_cast<uint32_t*>(p->block + L.off[RSD_SS_GT]);
    it.ss_obs = reinterpret_cast<double*>(p->block + L.off[RSD_SS_OBS_SUM]);
    it.ss_rep = reinterpret_cast<double*>(p->block + L.off[RSD_SS_REP_SUM]);
    it.part = p->item_part; it.global = p->block + L.off[RSD_GLOBAL]; it.stats = p->stats; it.ctl = p->ctl; it.m = m;
    hipLaunchKernelGGL(resid_items_kernel, dim3((unsigned)m), dim3(64), 0, st, it);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(resid_global_kernel, dim3(1), dim3(64), 0, st, it);
    GP_HIP(hipGetLastError());
    return 0;
}

int rsd_get(hipStream_t st, RsdState* p, const char* name, void* h_out, int64_t bytes)
{
    const int64_t n = p->n, m = p->m, P = m * m;
    const RsdLayout L = rsd_layout(m);
    auto copy = [&](const void* src) -> int {
        GP_HIP(hipMemcpyAsync(h_out, src, (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    const char* const tabs[5] = { "s_obs", "s_rep", "v", "r_obs", "r_rep" };
    const void* const tab_ptr[5] = { p->s_obs, p->s_rep, p->v, p->r_obs, p->r_rep };
    for (int k = 0; k < 5; ++k)
        if (strcmp(name, tabs[k]) == 0) {
            GP_ARG(bytes == 8 * P);
            GP_TRY(copy(tab_ptr[k]));
            if (k < 2) {                              // S: the sum of the two halves of the depth
                std::vector<int64_t> second((size_t)P);
                GP_HIP(hipMemcpyAsync(second.data(), static_cast<const int64_t*>(tab_ptr[k]) + P, (size_t)bytes, hipMemcpyDeviceToHost, st));
                GP_HIP(hipStreamSynchronize(st));
                for (int64_t g = 0; g < P; ++g) static_cast<int64_t*>(h_out)[g] += second[(size_t)g];
            }
            return 0;
        }
    if (strcmp(name, "stats") == 0) { GP_ARG(bytes == 64); return copy(p->stats); }
    const int term = strcmp(name, "d_obs") == 0 ? 0 : strcmp(name, "d_rep") == 0 ? 1 : strcmp(name, "w") == 0 ? 2 : -1;
    if (term >= 0 || strcmp(name, "digits") == 0) {       // the set of the last counted draw, out of the operand layout
        GP_ARG(bytes == (term >= 0 ? 4 : RSD_PLANES) * n * m);
        int cur = 0;
        GP_HIP(hipMemcpyAsync(&cur, p->ctl, sizeof(int), hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        const int npl = term >= 0 ? 3 : RSD_PLANES;
        std::vector<signed char> raw((size_t)npl * (size_t)p->plane);
        GP_HIP(hipMemcpyAsync(raw.data(), p->dig + ((int64_t)(cur & 1) * RSD_PLANES + (term >= 0 ? 3 * term : 0)) * p->plane, raw.size(),
                              hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        if (term < 0) {
            for (int pl = 0; pl < RSD_PLANES; ++pl) resid_unpack(p, raw, pl, static_cast<signed char*>(h_out) + (int64_t)pl * n * m);
            return 0;
        }
        std::vector<signed char> d((size_t)(3 * n * m));
        for (int pl = 0; pl < 3; ++pl) resid_unpack(p, raw, pl, d.data() + (int64_t)pl * n * m);
        int32_t* out = static_cast<int32_t*>(h_out);
        for (int64_t c = 0; c < n * m; ++c) out[c] = (int32_t)d[(size_t)c] + 256 * (int32_t)d[(size_t)(n * m + c)] + 65536 * (int32_t)d[(size_t)(2 * n * m + c)];
        return 0;
    }
    for (int k = 0; k < RSD_NARRAYS; ++k)
        if (strcmp(kResidRaw[k], name) == 0) { GP_ARG(bytes == L.bytes[k]); return copy(p->block + L.off[k]); }
    int pf = -1, itf = -1;
    for (int k = 0; k < GPIRT_RESID_NPAIR; ++k) if (strcmp(kResidPair[k], name) == 0) pf = k;
    for (int k = 0; k < GPIRT_RESID_NITEM; ++k) if (strcmp(kResidItem[k], name) == 0) itf = k;
    const bool scalars = strcmp(name, "scalars") == 0, counts = strcmp(name, "counts") == 0;
    if (pf < 0 && itf < 0 && !scalars && !counts) { set_error("unknown residual PPC field '%s'", name); return GPIRT_E_ARG; }
    GP_ARG(bytes == (pf >= 0 ? 8 * P : itf >= 0 ? 8 * m : scalars ? 8 * GPIRT_RESID_NSCALAR : 24));
    HostResid r;
    GP_TRY(resid_read(st, p->block, r, "gpirt_sampler_ppc_resid_get", 0));
    if (pf >= 0) resid_fill_pair(r, pf, static_cast<double*>(h_out));
    else if (itf >= 0) resid_fill_item(r, itf, static_cast<double*>(h_out));
    else if (scalars) resid_scalars(r, static_cast<double*>(h_out));
    else {
        int64_t* out = static_cast<int64_t*>(h_out);
        out[0] = r.hdr()[3]; out[1] = r.hdr()[4]; out[2] = (int64_t)r.arr<uint64_t>(RSD_GLOBAL)[13];
    }
    return 0;
}

int rsd_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_resid* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved0 == 0 && out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_RESID_MAX_TOP) {
        set_error("residual PPC: top = %d is outside 1..%d", out->top, GPIRT_RESID_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    HostResid pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostResid& r = c == 0 ? pooled : one;
        GP_TRY(resid_read(h->stream, d_states[c], r, "gpirt_ppc_resid_combine", c));
        if (c == 0) continue;
        if (r.n != pooled.n || r.m != pooled.m || r.hdr()[5] != pooled.hdr()[5]) {
            set_error("gpirt_ppc_resid_combine: state %d has another n, m or item0 than state 0", c);
            return GPIRT_E_ARG;
        }
        const int64_t m = r.m, P = m * m;
        if (!std::equal(one.arr<int64_t>(RSD_N_CO), one.arr<int64_t>(RSD_N_CO) + P, pooled.arr<int64_t>(RSD_N_CO))) {
            set_error("gpirt_ppc_resid_combine: state %d was accumulated on another response matrix than state 0 (n_co differs)", c);
            return GPIRT_E_ARG;
        }
        pooled.hdr()[3] += one.hdr()[3];
        pooled.hdr()[4] += one.hdr()[4];
        for (int k = RSD_UNDEF; k <= RSD_RC_GT; ++k)
            for (int64_t g = 0; g < P; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
        for (int k = RSD_RC_OBS_SUM; k <= RSD_RC_REP_SUMSQ; ++k)           // the double sums, in chain order
            for (int64_t g = 0; g < P; ++g) pooled.arr<double>(k)[g] += one.arr<double>(k)[g];
        for (int k = RSD_SS_UNDEF; k <= RSD_SS_GT; ++k)
            for (int64_t g = 0; g < m; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
        for (int k = RSD_SS_OBS_SUM; k <= RSD_SS_REP_SUM; ++k)
            for (int64_t g = 0; g < m; ++g) pooled.arr<double>(k)[g] += one.arr<double>(k)[g];
        for (int g = 0; g < 7; ++g) pooled.arr<double>(RSD_GLOBAL)[g] += one.arr<double>(RSD_GLOBAL)[g];
        for (int g = 7; g < RSD_GLOBAL_WORDS; ++g) pooled.arr<uint64_t>(RSD_GLOBAL)[g] += one.arr<uint64_t>(RSD_GLOBAL)[g];
    }
    resid_fill(pooled, out);
    return 0;
}

}  // namespace gpirt
