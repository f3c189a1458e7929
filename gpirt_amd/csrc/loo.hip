// loo.hip -- PSIS-LOO without stored draws (include/gpirt_hip.h, "PSIS-LOO"): per observed cell the K = M + 1
// largest keys kappa = -y (f + mu) of all pooled draws, kept one draw at a time, the sums of the importance ratios of everything
// else, and at the end a generalised Pareto fit of the tail per cell.
//
//   loo_accumulate_kernel   one streaming pass over the cells, one thread per cell: f, mu, the y byte and the heap's root are read;
//                           a draw that does not beat the root costs one compare and the two evicted sums; one that does replaces
//                           the root and sifts down (until K keys are in: append and sift up).  The heap lives in global memory,
//                           slot-major (slot z of cell c at [z cells + c]): adjacent lanes touch adjacent cells at every level.
//   loo_merge_kernel        pooling: the other state's kept keys enter the pooled heap in slot order by the same rule
//   loo_finish_kernel       one wave per cell: the keys to LDS (8 K bytes), a bitonic sort whose every comparator moves the
//                           smaller key down (so the slots beyond K act as +inf without being stored), exp(key - kmax) in place,
//                           then Zhang and Stephens' fit with one lane per grid point, the softmax over the grid and every sum in
//                           a fixed lane order
//   loo_totals_kernel / loo_reduce_kernel   block partials, then one block in block order (two passes: sums, then the squared
//                           deviations from the mean), as summary.hip's totals
//   loo_item_kernel, loo_respondent_kernel, loo_top_kernel   the column / row sums and the `top` largest k
// No atomics anywhere; every accumulator cell has one owner.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

namespace gpirt {

namespace {

constexpr int LOO_THREADS = 256;
constexpr int LOO_MAX_BLOCKS = 2048;
constexpr int LOO_TOTAL_BLOCKS = 1024;            // fixed: the order of the totals' sums does not depend on the device
constexpr int LOO_FIN_BLOCKS = 4096;
constexpr int LOO_NPART = 9;
constexpr int LOO_TOP_BLOCKS = 128;
constexpr int LOO_MAXK = GPIRT_LOO_MAX_TAIL + 1;

const char* const kLooRaw[GPIRT_LOO_NARRAYS] = { "keys", "evicted_sum", "evicted_sumsq", "p_sum", "count", "nonfinite", "y" };

inline int64_t loo_raw_bytes(int k, int64_t cells, int64_t M)
{
    switch (k) {
        case GPIRT_LOO_KEYS: return 8 * (M + 1) * cells;
        case GPIRT_LOO_COUNT: case GPIRT_LOO_NONFINITE: return 4 * cells;
        case GPIRT_LOO_Y: return cells;
        default: return 8 * cells;
    }
}

struct LooArrays {
    double* keys; double* es; double* es2; double* ps; int* count; int* nonfinite; signed char* y;
};

LooArrays loo_arrays(uint64_t* block, const LooLayout& L)
{
    LooArrays a;
    a.keys = reinterpret_cast<double*>(block + L.off[GPIRT_LOO_KEYS]);
    a.es = reinterpret_cast<double*>(block + L.off[GPIRT_LOO_EVICTED_SUM]);
    a.es2 = reinterpret_cast<double*>(block + L.off[GPIRT_LOO_EVICTED_SUMSQ]);
    a.ps = reinterpret_cast<double*>(block + L.off[GPIRT_LOO_P_SUM]);
    a.count = reinterpret_cast<int*>(block + L.off[GPIRT_LOO_COUNT]);
    a.nonfinite = reinterpret_cast<int*>(block + L.off[GPIRT_LOO_NONFINITE]);
    a.y = reinterpret_cast<signed char*>(block + L.off[GPIRT_LOO_Y]);
    return a;
}

int loo_grid(int64_t work)
{
    const int64_t b = (work + LOO_THREADS - 1) / LOO_THREADS;
    return (int)(b < 1 ? 1 : (b > LOO_MAX_BLOCKS ? LOO_MAX_BLOCKS : b));
}

// ---- the heap of one cell: keys[z * cells + c], z = 0 .. hs - 1, the smallest in slot 0 ------------------------------------
__device__ __forceinline__ void loo_sift_up(double* __restrict__ keys, int64_t cells, int64_t c, int pos, double v)
{
    while (pos > 0) {
        const int par = (pos - 1) >> 1;
        const double kp = keys[(int64_t)par * cells + c];
        if (!(v < kp)) break;
        keys[(int64_t)pos * cells + c] = kp;
        pos = par;
    }
    keys[(int64_t)pos * cells + c] = v;
}

__device__ __forceinline__ void loo_sift_down(double* __restrict__ keys, int64_t cells, int64_t c, int K, double v)
{
    int pos = 0;
    for (;;) {
        const int l = 2 * pos + 1;
        if (l >= K) break;
        int ch = l;
        double kc = keys[(int64_t)l * cells + c];
        if (l + 1 < K) {
            const double kr = keys[(int64_t)(l + 1) * cells + c];
            if (kr < kc) { kc = kr; ch = l + 1; }
        }
        if (!(kc < v)) break;
        keys[(int64_t)pos * cells + c] = kc;
        pos = ch;
    }
    keys[(int64_t)pos * cells + c] = v;
}

// one key into the heap of hs keys: appended while hs < K; else it beats the root (which leaves) or is refused.  r and r^2 of
// whichever key is not kept go to the evicted sums.  r_key: 1 + exp(key) if the caller has it, 0 if not.
__device__ __forceinline__ void loo_enter(double* __restrict__ keys, int64_t cells, int64_t c, int K, int& hs, double key,
                                          double r_key, double& es, double& es2)
{
    if (hs < K) {
        loo_sift_up(keys, cells, c, hs, key);
        ++hs;
        return;
    }
    const double root = keys[c];
    double r = r_key;
    if (key > root) {
        r = 1.0 + exp(root);
        loo_sift_down(keys, cells, c, K, key);
    } else if (r == 0.0) {
        r = 1.0 + exp(key);
    }
    es += r;
    es2 += r * r;
}

__global__ __launch_bounds__(LOO_THREADS) void loo_accumulate_kernel(const double* __restrict__ f, const double* __restrict__ mu,
                                                                     LooArrays a, int64_t cells, int K, int64_t* __restrict__ hdr)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (tid == 0) hdr[6] += 1;
    for (int64_t c = tid; c < cells; c += stride) {
        const int yv = a.y[c];
        if (!yv) continue;
        const double g = f[c] + mu[c];
        const double key = -((double)yv * g);
        if (!(fabs(g) <= DBL_MAX) || key > GPIRT_LOO_KEY_MAX) {
            a.nonfinite[c] += 1;
            continue;
        }
        const double r = 1.0 + exp(key);
        a.ps[c] += 1.0 / r;
        const int cnt = a.count[c];
        int hs = cnt < K ? cnt : K;
        if (hs == K) {
            double es = a.es[c], es2 = a.es2[c];
            loo_enter(a.keys, cells, c, K, hs, key, r, es, es2);
            a.es[c] = es;
            a.es2[c] = es2;
        } else {
            loo_sift_up(a.keys, cells, c, hs, key);
        }
        a.count[c] = cnt + 1;
    }
}

__global__ __launch_bounds__(LOO_THREADS) void loo_merge_kernel(LooArrays d, LooArrays s, int64_t cells, int K, int64_t* __restrict__ hd,
                                                                const int64_t* __restrict__ hs_)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (tid == 0) { hd[6] += hs_[6]; hd[7] += hs_[7]; }
    for (int64_t c = tid; c < cells; c += stride) {
        if (!d.y[c]) continue;
        const int cd = d.count[c], cs = s.count[c];
        int hs = cd < K ? cd : K;
        const int ns = cs < K ? cs : K;
        double es = d.es[c] + s.es[c], es2 = d.es2[c] + s.es2[c];
        for (int z = 0; z < ns; ++z) loo_enter(d.keys, cells, c, K, hs, s.keys[(int64_t)z * cells + c], 0.0, es, es2);
        d.es[c] = es;
        d.es2[c] = es2;
        d.ps[c] += s.ps[c];
        d.count[c] = cd + cs;
        d.nonfinite[c] += s.nonfinite[c];
    }
}

// ---- finishing: one wave per cell ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void loo_cmpx(double* sk, int i, int j, int K)
{
    if (j < K) {
        const double a = sk[i], b = sk[j];
        if (b < a) { sk[i] = b; sk[j] = a; }
    }
}

// the 64 lanes' values added in lane order; every lane gets the sum
__device__ __forceinline__ double loo_lane_sum(double* red, int lane, double v)
{
    __syncthreads();
    red[lane] = v;
    __syncthreads();
    double s = 0.0;
    for (int l = 0; l < 64; ++l) s += red[l];
    return s;
}

// status: 0 missing, 1 incomplete, 2 unsmoothed, 3 smoothed
__global__ __launch_bounds__(64) void loo_finish_kernel(LooArrays a, int64_t cells, int K, int64_t T, double* __restrict__ out,
                                                        signed char* __restrict__ status)
{
    __shared__ double sk[LOO_MAXK];
    __shared__ double red[64];
    __shared__ double lj[64];
    const int lane = threadIdx.x;
    const int M = K - 1;
    const double dM = (double)M;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    int P = 1;
    while (P < K) P <<= 1;
    for (int64_t c = blockIdx.x; c < cells; c += gridDim.x) {
        const int yv = a.y[c];
        const bool done = yv && (int64_t)a.count[c] == T && a.nonfinite[c] == 0;
        if (!done) {                                                  // (uniform over the wave)
            if (lane == 0) {
                for (int q = 0; q < GPIRT_LOO_NPOINTWISE; ++q) out[(int64_t)q * cells + c] = nan;
                status[c] = yv ? 1 : 0;
            }
            continue;
        }
        __syncthreads();                                              // the last cell's reads of sk are over
        for (int z = lane; z < K; z += 64) sk[z] = a.keys[(int64_t)z * cells + c];
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            const int hk = k >> 1;
            for (int t = lane; t < (P >> 1); t += 64) {               // the flip: i against its mirror in the block of k
                const int blk = t / hk, off = t - blk * hk;
                loo_cmpx(sk, blk * k + off, blk * k + k - 1 - off, K);
            }
            __syncthreads();
            for (int jj = hk >> 1; jj > 0; jj >>= 1) {
                for (int t = lane; t < (P >> 1); t += 64) {
                    const int blk = t / jj, off = t - blk * jj;
                    const int i = 2 * jj * blk + off;
                    loo_cmpx(sk, i, i + jj, K);
                }
                __syncthreads();
            }
        }
        const double kc = sk[0], kmax = sk[K - 1];
        __syncthreads();
        for (int z = lane; z < K; z += 64) sk[z] = exp(sk[z] - kmax);
        __syncthreads();
        const double ec = sk[0], emk = exp(-kmax);
        const double xM = sk[M] - ec;
        bool smooth = M >= 5 && xM > 0.0;
        double kfit = nan, sigma = nan;
        if (smooth) {
            const int mgrid = 30 + (int)floor(sqrt(dM));
            const double xstar = sk[(M + 2) / 4] - ec;
            double th = 0.0;
            if (lane < mgrid) {
                th = 1.0 / xM + (1.0 - sqrt((double)mgrid / ((double)(lane + 1) - 0.5))) / (3.0 * xstar);
                double acc = 0.0;
                for (int z = 1; z <= M; ++z) acc += log1p(-th * (sk[z] - ec));
                const double kj = acc / dM;
                lj[lane] = dM * (log(-th / kj) - kj - 1.0);
            }
            __syncthreads();
            double tw = 0.0;
            if (lane < mgrid) {
                const double l = lj[lane];
                double s = 0.0;
                for (int i = 0; i < mgrid; ++i) s += exp(lj[i] - l);
                tw = th * (1.0 / s);
            }
            const double that = loo_lane_sum(red, lane, tw);         // (the lanes beyond mgrid add +0)
            double part = 0.0;
            for (int z = 1 + lane; z <= M; z += 64) part += log1p(-that * (sk[z] - ec));
            const double k0 = loo_lane_sum(red, lane, part) / dM;
            sigma = -k0 / that;
            kfit = (k0 * dM + 5.0) / (dM + 10.0);
            if (!(fabs(kfit) <= DBL_MAX) || !(fabs(sigma) <= DBL_MAX)) { smooth = false; kfit = nan; }
        }
        double sw = 0.0, sw2 = 0.0, swr = 0.0;
        for (int z = 1 + lane; z <= M; z += 64) {
            const double rho = emk + sk[z];
            double wt = rho;
            if (smooth) {
                double q = sigma * expm1(-kfit * log1p(-((double)z - 0.5) / dM)) / kfit + ec;
                if (q > 1.0) q = 1.0;
                wt = emk + q;
            }
            sw += wt;
            sw2 += wt * wt;
            swr += wt / rho;
        }
        const double SW = loo_lane_sum(red, lane, sw);
        const double SW2 = loo_lane_sum(red, lane, sw2);
        const double SWR = loo_lane_sum(red, lane, swr);
        if (lane == 0) {
            const double rc = 1.0 + exp(kc);
            const double E = a.es[c] + rc, E2 = a.es2[c] + rc * rc;
            const double W = E * emk + SW;
            const double elpd = log((double)(T - M) + SWR) - log(W) - kmax;
            const double neff = W * W / ((E2 * emk) * emk + SW2);
            const double lppd = log(a.ps[c] / (double)T);
            out[(int64_t)GPIRT_LOO_PW_PARETO_K * cells + c] = kfit;
            out[(int64_t)GPIRT_LOO_PW_ELPD_LOO * cells + c] = elpd;
            out[(int64_t)GPIRT_LOO_PW_N_EFF * cells + c] = neff;
            out[(int64_t)GPIRT_LOO_PW_LPPD * cells + c] = lppd;
            out[(int64_t)GPIRT_LOO_PW_P_LOO * cells + c] = lppd - elpd;
            out[(int64_t)GPIRT_LOO_PW_LOO_P_YES * cells + c] = yv > 0 ? exp(elpd) : 1.0 - exp(elpd);
            status[c] = smooth ? 3 : 2;
        }
    }
}

// ---- totals ---------------------------------------------------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void loo_block_sum(double (&v)[NV], double (*sh)[LOO_THREADS])
{
    const int t = threadIdx.x;
    for (int k = 0; k < NV; ++k) sh[k][t] = v[k];
    __syncthreads();
    for (int w = LOO_THREADS / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int k = 0; k < NV; ++k) sh[k][t] += sh[k][t + w];
        __syncthreads();
    }
    for (int k = 0; k < NV; ++k) v[k] = sh[k][0];
}

// pass 0: [sum elpd, sum p_loo, sum lppd, n_obs, k_good, k_bad, k_very_bad, unsmoothed, incomplete]; pass 1: [sum (elpd - mean)^2]
__global__ __launch_bounds__(LOO_THREADS) void loo_totals_kernel(const double* __restrict__ out, const signed char* __restrict__ status,
                                                                 int64_t cells, double thr, int pass, const double* __restrict__ tot,
                                                                 double* __restrict__ part)
{
    __shared__ double sh[LOO_NPART][LOO_THREADS];
    double v[LOO_NPART] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    const double mean = pass ? tot[GPIRT_LOO_T_ELPD_MEAN] : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
        const int st = status[i];
        if (st < 2) {
            if (st == 1 && pass == 0) v[8] += 1.0;
            continue;
        }
        const double e = out[(int64_t)GPIRT_LOO_PW_ELPD_LOO * cells + i];
        if (pass) { const double dv = e - mean; v[0] += dv * dv; continue; }
        v[0] += e;
        v[1] += out[(int64_t)GPIRT_LOO_PW_P_LOO * cells + i];
        v[2] += out[(int64_t)GPIRT_LOO_PW_LPPD * cells + i];
        v[3] += 1.0;
        if (st == 2) { v[7] += 1.0; continue; }
        const double k = out[(int64_t)GPIRT_LOO_PW_PARETO_K * cells + i];
        if (k <= thr) v[4] += 1.0; else if (k <= 1.0) v[5] += 1.0; else v[6] += 1.0;
    }
    loo_block_sum<LOO_NPART>(v, sh);
    if (threadIdx.x == 0)
        for (int k = 0; k < LOO_NPART; ++k) part[(int64_t)blockIdx.x * LOO_NPART + k] = v[k];
}

// one block: the partials in block order, then the derived totals (include/gpirt_hip.h GPIRT_LOO_T_*)
__global__ __launch_bounds__(LOO_THREADS) void loo_reduce_kernel(const double* __restrict__ part, int nblocks, int pass, double thr,
                                                                 double* __restrict__ tot)
{
    __shared__ double sh[LOO_NPART][LOO_THREADS];
    double v[LOO_NPART] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int b = threadIdx.x; b < nblocks; b += LOO_THREADS)
        for (int k = 0; k < LOO_NPART; ++k) v[k] += part[(int64_t)b * LOO_NPART + k];
    loo_block_sum<LOO_NPART>(v, sh);
    if (threadIdx.x != 0) return;
    if (pass == 0) {
        tot[GPIRT_LOO_T_ELPD_LOO] = v[0];
        tot[GPIRT_LOO_T_P_LOO] = v[1];
        tot[GPIRT_LOO_T_LPPD] = v[2];
        tot[GPIRT_LOO_T_LOOIC] = -2.0 * v[0];
        tot[GPIRT_LOO_T_N_OBS] = v[3];
        tot[GPIRT_LOO_T_K_THRESHOLD] = thr;
        tot[GPIRT_LOO_T_K_GOOD] = v[4];
        tot[GPIRT_LOO_T_K_BAD] = v[5];
        tot[GPIRT_LOO_T_K_VERY_BAD] = v[6];
        tot[GPIRT_LOO_T_UNSMOOTHED] = v[7];
        tot[GPIRT_LOO_T_CELLS_INCOMPLETE] = v[8];
        tot[GPIRT_LOO_T_ELPD_MEAN] = v[0] / v[3];
    } else {
        const double nobs = tot[GPIRT_LOO_T_N_OBS];
        const double se = sqrt(nobs * (v[0] / (nobs - 1.0)));           // loo: sqrt(N var(elpd_i)), ddof = 1
        tot[GPIRT_LOO_T_SE_ELPD_LOO] = se;
        tot[GPIRT_LOO_T_SE_LOOIC] = 2.0 * se;
    }
}

// item j: the finished cells of column j, strided partials and a tree in a fixed order
__global__ __launch_bounds__(LOO_THREADS) void loo_item_kernel(const double* __restrict__ elpd, const signed char* __restrict__ status,
                                                               int64_t n, double* __restrict__ item)
{
    __shared__ double sh[1][LOO_THREADS];
    const int64_t j = blockIdx.x;
    double v[1] = { 0.0 };
    for (int64_t i = threadIdx.x; i < n; i += LOO_THREADS)
        if (status[j * n + i] >= 2) v[0] += elpd[j * n + i];
    loo_block_sum<1>(v, sh);
    if (threadIdx.x == 0) item[j] = v[0];
}

// respondent i: the finished cells of row i in ascending column order
__global__ __launch_bounds__(LOO_THREADS) void loo_respondent_kernel(const double* __restrict__ elpd,
                                                                     const signed char* __restrict__ status, int64_t n, int64_t m,
                                                                     double* __restrict__ resp)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (int64_t j = 0; j < m; ++j)
        if (status[j * n + i] >= 2) acc += elpd[j * n + i];
    resp[i] = acc;
}

// (k, id) orders before (k', id') when k > k', or k == k' and id < id'
__device__ __forceinline__ bool loo_before(double k, int64_t id, double k2, int64_t id2)
{
    return k > k2 || (k == k2 && id < id2);
}

// block b: the `top` first entries, in that order, among its slice of `count` entries (k[e], id = ids ? ids[e] : e; a NaN k and a
// negative id never enter) -> ck / cid [b * top ..]; missing places hold NaN and -1.  Stage 1 runs it over the cells in slices,
// stage 2 with one block over stage 1's candidates.
__global__ __launch_bounds__(LOO_THREADS) void loo_top_kernel(const double* __restrict__ k, const int64_t* __restrict__ ids, int64_t count,
                                                              int top, double* __restrict__ ck, int64_t* __restrict__ cid)
{
    __shared__ double shk[LOO_THREADS];
    __shared__ int64_t shi[LOO_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (count + gridDim.x - 1) / gridDim.x;
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < count ? lo + per : count;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double pk = __longlong_as_double(0x7ff0000000000000LL);           // +inf: everything comes after it
    int64_t pid = -1;
    for (int r = 0; r < top; ++r) {
        double bk = nan;
        int64_t bid = -1;
        if (r == 0 || pid >= 0) {
            for (int64_t e = lo + t; e < hi; e += LOO_THREADS) {
                const double v = k[e];
                const int64_t id = ids ? ids[e] : e;
                if (!(v == v) || id < 0) continue;
                if (r > 0 && !loo_before(pk, pid, v, id)) continue;   // already taken
                if (bid < 0 || loo_before(v, id, bk, bid)) { bk = v; bid = id; }
            }
        }
        __syncthreads();
        shk[t] = bk; shi[t] = bid;
        __syncthreads();
        for (int w = LOO_THREADS / 2; w > 0; w >>= 1) {
            if (t < w && shi[t + w] >= 0 && (shi[t] < 0 || loo_before(shk[t + w], shi[t + w], shk[t], shi[t]))) {
                shk[t] = shk[t + w]; shi[t] = shi[t + w];
            }
            __syncthreads();
        }
        pk = shk[0]; pid = shi[0];
        if (t == 0) { ck[(int64_t)blockIdx.x * top + r] = pid >= 0 ? pk : nan; cid[(int64_t)blockIdx.x * top + r] = pid; }
    }
}

struct DevBuf {
    std::vector<void*> p;
    ~DevBuf() { for (void* q : p) hipFree(q); }
    int get(void** q, size_t bytes)
    {
        GP_HIP(hipMalloc(q, bytes ? bytes : 16));
        p.push_back(*q);
        return 0;
    }
};

int loo_read_header(hipStream_t st, const void* d_state, int64_t* hdr, const char* who, int c)
{
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(int64_t) * LOO_HEADER_WORDS, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    const bool ok = hdr[0] == LOO_TAG && hdr[1] == LOO_LAYOUT_VERSION && hdr[2] > 0 && hdr[3] > 0 && hdr[4] >= 1 && hdr[5] >= 0 &&
                    hdr[5] <= GPIRT_LOO_MAX_TAIL && hdr[5] < hdr[4] && hdr[6] >= 0 && hdr[7] >= 1;
    if (!ok) {
        set_error("%s: state %d is not a LOO state block of layout %d", who, c, LOO_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    return 0;
}

// the pointwise outputs, totals, sums and worst cells of one (pooled) block into out
int loo_finish(gpirt_handle_t h, uint64_t* block, const int64_t* hdr, gpirt_loo* out)
{
    hipStream_t st = h->stream;
    const int64_t n = hdr[2], m = hdr[3], T = hdr[4], M = hdr[5], cells = n * m;
    const int K = (int)M + 1, top = (int)out->top;
    const LooLayout L = loo_layout(n, m, M);
    const LooArrays a = loo_arrays(block, L);
    DevBuf buf;
    double *d_out = nullptr, *d_part = nullptr, *d_tot = nullptr, *d_item = nullptr, *d_resp = nullptr, *d_ck = nullptr, *d_wk = nullptr;
    int64_t *d_cid = nullptr, *d_wid = nullptr;
    signed char* d_status = nullptr;
    const int tblocks = (int)std::min<int64_t>(LOO_TOP_BLOCKS, (cells + 4095) / 4096);
    GP_TRY(buf.get((void**)&d_out, sizeof(double) * (size_t)cells * GPIRT_LOO_NPOINTWISE));
    GP_TRY(buf.get((void**)&d_status, (size_t)cells));
    GP_TRY(buf.get((void**)&d_part, sizeof(double) * LOO_TOTAL_BLOCKS * LOO_NPART));
    GP_TRY(buf.get((void**)&d_tot, sizeof(double) * GPIRT_LOO_NTOTALS));
    GP_TRY(buf.get((void**)&d_item, sizeof(double) * (size_t)m));
    GP_TRY(buf.get((void**)&d_resp, sizeof(double) * (size_t)n));
    GP_TRY(buf.get((void**)&d_ck, sizeof(double) * (size_t)tblocks * (size_t)top));
    GP_TRY(buf.get((void**)&d_cid, sizeof(int64_t) * (size_t)tblocks * (size_t)top));
    GP_TRY(buf.get((void**)&d_wk, sizeof(double) * (size_t)top));
    GP_TRY(buf.get((void**)&d_wid, sizeof(int64_t) * (size_t)top));
    GP_HIP(hipMemsetAsync(d_tot, 0, sizeof(double) * GPIRT_LOO_NTOTALS, st));
    const int fblocks = (int)std::min<int64_t>(LOO_FIN_BLOCKS, cells);
    hipLaunchKernelGGL(loo_finish_kernel, dim3(fblocks), dim3(64), 0, st, a, cells, K, T, d_out, d_status);
    GP_HIP(hipGetLastError());
    const double thr = std::min(1.0 - 1.0 / std::log10((double)T), 0.7);
    for (int pass = 0; pass < 2; ++pass) {
        hipLaunchKernelGGL(loo_totals_kernel, dim3(LOO_TOTAL_BLOCKS), dim3(LOO_THREADS), 0, st, d_out, d_status, cells, thr, pass, d_tot,
                           d_part);
        hipLaunchKernelGGL(loo_reduce_kernel, dim3(1), dim3(LOO_THREADS), 0, st, d_part, LOO_TOTAL_BLOCKS, pass, thr, d_tot);
    }
    GP_HIP(hipGetLastError());
    const double* d_elpd = d_out + (int64_t)GPIRT_LOO_PW_ELPD_LOO * cells;
    hipLaunchKernelGGL(loo_item_kernel, dim3((unsigned)m), dim3(LOO_THREADS), 0, st, d_elpd, d_status, n, d_item);
    hipLaunchKernelGGL(loo_respondent_kernel, dim3((unsigned)((n + LOO_THREADS - 1) / LOO_THREADS)), dim3(LOO_THREADS), 0, st, d_elpd,
                       d_status, n, m, d_resp);
    hipLaunchKernelGGL(loo_top_kernel, dim3(tblocks), dim3(LOO_THREADS), 0, st, d_out + (int64_t)GPIRT_LOO_PW_PARETO_K * cells,
                       (const int64_t*)nullptr, cells, top, d_ck, d_cid);
    hipLaunchKernelGGL(loo_top_kernel, dim3(1), dim3(LOO_THREADS), 0, st, d_ck, d_cid, (int64_t)tblocks * top, top, d_wk, d_wid);
    GP_HIP(hipGetLastError());
    auto back = [&](void* dst, const void* src, size_t bytes) -> int {
        if (dst) GP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        return 0;
    };
    for (int q = 0; q < GPIRT_LOO_NPOINTWISE; ++q) GP_TRY(back(out->pointwise[q], d_out + (int64_t)q * cells, sizeof(double) * (size_t)cells));
    for (int k = 0; k < GPIRT_LOO_NARRAYS; ++k) GP_TRY(back(out->raw[k], block + L.off[k], (size_t)loo_raw_bytes(k, cells, M)));
    GP_TRY(back(out->item_elpd_loo, d_item, sizeof(double) * (size_t)m));
    GP_TRY(back(out->respondent_elpd_loo, d_resp, sizeof(double) * (size_t)n));
    GP_TRY(back(out->worst_index, d_wid, sizeof(int64_t) * (size_t)top));
    GP_TRY(back(out->worst_k, d_wk, sizeof(double) * (size_t)top));
    GP_TRY(back(out->totals, d_tot, sizeof(double) * GPIRT_LOO_NTOTALS));
    GP_HIP(hipStreamSynchronize(st));
    int64_t now[LOO_HEADER_WORDS];
    GP_HIP(hipMemcpy(now, block, sizeof(now), hipMemcpyDeviceToHost));
    out->n = n; out->m = m; out->T = T; out->M = M; out->draws = now[6]; out->chains = now[7];
    return 0;
}

}  // namespace

LooLayout loo_layout(int64_t n, int64_t m, int64_t M)
{
    LooLayout L{};
    int64_t at = LOO_HEADER_WORDS;
    for (int k = 0; k < GPIRT_LOO_NARRAYS; ++k) {
        L.off[k] = at;
        at += (loo_raw_bytes(k, n * m, M) + 15) / 16 * 2;             // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

int loo_tail_length(int64_t T, int tail, int64_t* M_out)
{
    if (T < 1) {
        set_error("LOO: the planned number of draws must be at least 1 (got %lld)", (long long)T);
        return GPIRT_E_ARG;
    }
    int64_t M;
    if (tail != 0) {
        if (tail < 5 || tail > GPIRT_LOO_MAX_TAIL) {
            set_error("LOO: tail = %d, it must lie in 5 .. %d (or be 0 for the rule)", tail, GPIRT_LOO_MAX_TAIL);
            return GPIRT_E_ARG;
        }
        M = tail;
        if (M >= T) {
            set_error("LOO: a tail of %lld keys and the cutoff need more than the %lld planned draws", (long long)M, (long long)T);
            return GPIRT_E_ARG;
        }
    } else {
        int64_t c = (int64_t)std::ceil(3.0 * std::sqrt((double)T));   // ceil(3 sqrt(T)): the smallest c with c^2 >= 9 T
        while (c * c >= 9 * T && c > 0) --c;
        while (c * c < 9 * T) ++c;
        M = std::min(T / 5, c);
    }
    if (M > GPIRT_LOO_MAX_TAIL) {
        set_error("LOO: %lld planned draws give a tail of %lld keys, more than GPIRT_LOO_MAX_TAIL = %d; pass tail=", (long long)T,
                  (long long)M, GPIRT_LOO_MAX_TAIL);
        return GPIRT_E_ARG;
    }
    if (M_out) *M_out = M;
    return 0;
}

void loo_free(LooState* p)
{
    if (p->block) hipFree(p->block);
    *p = LooState{};
}

int loo_alloc(hipStream_t st, LooState* p, int64_t n, int64_t m, int64_t T, int64_t M, const double* d_y)
{
    const int64_t cells = n * m;
    const LooLayout L = loo_layout(n, m, M);
    GP_HIP(hipMalloc((void**)&p->block, sizeof(uint64_t) * (size_t)L.words));
    p->n = n; p->m = m; p->T = T; p->M = M;
    GP_HIP(hipMemsetAsync(p->block, 0, sizeof(uint64_t) * (size_t)L.words, st));
    std::vector<double> y((size_t)cells);
    GP_HIP(hipMemcpyAsync(y.data(), d_y, sizeof(double) * (size_t)cells, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    std::vector<signed char> yb((size_t)cells);
    for (int64_t c = 0; c < cells; ++c) yb[(size_t)c] = y[(size_t)c] != y[(size_t)c] ? 0 : (y[(size_t)c] > 0.0 ? 1 : -1);
    const int64_t hdr[LOO_HEADER_WORDS] = { LOO_TAG, LOO_LAYOUT_VERSION, n, m, T, M, 0, 1 };
    GP_HIP(hipMemcpyAsync(p->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipMemcpyAsync(p->block + L.off[GPIRT_LOO_Y], yb.data(), (size_t)cells, hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // the host vectors are this call's: nothing may leave with the copies pending
    p->on = true;
    return 0;
}

int launch_loo_accumulate(hipStream_t st, LooState* p, const double* f, const double* mu)
{
    const int64_t cells = p->n * p->m;
    const LooArrays a = loo_arrays(p->block, loo_layout(p->n, p->m, p->M));
    hipLaunchKernelGGL(loo_accumulate_kernel, dim3(loo_grid(cells)), dim3(LOO_THREADS), 0, st, f, mu, a, cells, (int)p->M + 1,
                       reinterpret_cast<int64_t*>(p->block));
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_loo_merge(hipStream_t st, uint64_t* into, const uint64_t* from, int64_t n, int64_t m, int64_t M)
{
    const LooLayout L = loo_layout(n, m, M);
    const LooArrays d = loo_arrays(into, L), s = loo_arrays(const_cast<uint64_t*>(from), L);
    hipLaunchKernelGGL(loo_merge_kernel, dim3(loo_grid(n * m)), dim3(LOO_THREADS), 0, st, d, s, n * m, (int)M + 1,
                       reinterpret_cast<int64_t*>(into), reinterpret_cast<const int64_t*>(from));
    GP_HIP(hipGetLastError());
    return 0;
}

int loo_get(hipStream_t st, LooState* p, const char* name, void* h_out, int64_t bytes)
{
    const LooLayout L = loo_layout(p->n, p->m, p->M);
    auto copy = [&](const void* src) -> int {
        GP_HIP(hipMemcpyAsync(h_out, src, (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 48); return copy(p->block + 2); }
    for (int k = 0; k < GPIRT_LOO_NARRAYS; ++k)
        if (strcmp(kLooRaw[k], name) == 0) {
            GP_ARG(bytes == loo_raw_bytes(k, p->n * p->m, p->M));
            return copy(p->block + L.off[k]);
        }
    set_error("unknown loo field '%s'", name);
    return GPIRT_E_ARG;
}

int loo_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_loo* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_LOO_MAX_TOP) {
        set_error("LOO: top = %lld, it must lie in 1 .. %d", (long long)out->top, GPIRT_LOO_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    hipStream_t st = h->stream;
    int64_t h0[LOO_HEADER_WORDS], hc[LOO_HEADER_WORDS];
    GP_TRY(loo_read_header(st, d_states[0], h0, "gpirt_loo_combine", 0));
    if (chains == 1) return loo_finish(h, static_cast<uint64_t*>(const_cast<void*>(d_states[0])), h0, out);
    const int64_t n = h0[2], m = h0[3], M = h0[5], cells = n * m;
    const LooLayout L = loo_layout(n, m, M);
    std::vector<signed char> y0((size_t)cells), yc((size_t)cells);
    GP_HIP(hipMemcpy(y0.data(), static_cast<const uint64_t*>(d_states[0]) + L.off[GPIRT_LOO_Y], (size_t)cells, hipMemcpyDeviceToHost));
    for (int c = 1; c < chains; ++c) {
        GP_TRY(loo_read_header(st, d_states[c], hc, "gpirt_loo_combine", c));
        bool same = hc[2] == n && hc[3] == m && hc[4] == h0[4] && hc[5] == M;
        if (same) {
            GP_HIP(hipMemcpy(yc.data(), static_cast<const uint64_t*>(d_states[c]) + L.off[GPIRT_LOO_Y], (size_t)cells, hipMemcpyDeviceToHost));
            same = memcmp(y0.data(), yc.data(), (size_t)cells) == 0;
        }
        if (!same) {
            set_error("gpirt_loo_combine: state %d has another n, m, T, M or y than state 0", c);
            return GPIRT_E_ARG;
        }
    }
    DevBuf buf;
    uint64_t* pooled = nullptr;
    GP_TRY(buf.get((void**)&pooled, sizeof(uint64_t) * (size_t)L.words));
    GP_HIP(hipMemcpyAsync(pooled, d_states[0], sizeof(uint64_t) * (size_t)L.words, hipMemcpyDeviceToDevice, st));
    for (int c = 1; c < chains; ++c) GP_TRY(launch_loo_merge(st, pooled, static_cast<const uint64_t*>(d_states[c]), n, m, M));
    return loo_finish(h, pooled, h0, out);
}

}  // namespace gpirt
