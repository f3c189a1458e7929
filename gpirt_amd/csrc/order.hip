// order.hip -- item-pair order posteriors of the item response curves (include/gpirt_hip.h, "Item-pair IRF order posteriors";
// DESIGN.md section 25): per counted draw and pair of items, from the shape block's smooth curves gbar, whether curve a lies
// above curve b on the whole window, below it, or crosses it, how deep the crossing is, which item is easier under N(0, 1),
// and how many pairs cross in the draw -- accumulated one draw at a time on top of the shape block (shape.hip), whose window,
// tolerances, grid weights and bad[] flags it reads.
//
// order_easiness_kernel: one work-group of 256 lanes per item; lane t adds its k = 4t .. 4t + 3 in order, lane 0 adds the 256
// partial sums in ascending t.
// order_pair_kernel<T>: one work-group per tile (A, B), A <= B, of T x T pairs.  The window is walked in chunks of OR_KC grid
// points; a chunk of the two item groups is staged in LDS transposed ([k][item], rows padded by two doubles), read from gbar in
// runs of OR_KC contiguous doubles per item.  Lane (ta, tb) of 16 x 16 owns the R x R pairs a = A T + R ta + i, b = B T + R tb + j
// (R = T / 16) in registers: per grid point one subtraction, one max and one min per pair (the min is -U[b, a] exactly).  The
// epilogue classifies the lane's pairs and bumps both triangles' cells -- in a diagonal tile every lane bumps only its own
// (a, b), so every cell has one owner -- and the tile's crossing pairs (a < b) are counted into the tile's partials.
// order_finish_kernel: one work-group adds the tiles' partials (integers) and keeps the set counts and the draw counters.
// Every work-group of all three reads bad[] first and leaves without a store when any item's curve was not finite.
// No atomics, one owner per cell: bit-identical from run to run.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace gpirt {

namespace {

constexpr int OR_THREADS = 256;
constexpr int OR_N = GPIRT_NGRID;
constexpr int OR_CENTRE = (GPIRT_NGRID - 1) / 2;
constexpr int OR_KC = 32;                          // grid points per LDS chunk
#ifndef GPIRT_ORDER_TILE
#define GPIRT_ORDER_TILE 64                        // tile width T (DESIGN.md section 25 has the measurement)
#endif
constexpr int OR_T = GPIRT_ORDER_TILE;
constexpr int OR_TOLS = GPIRT_SHAPE_MAX_TOLS;
static_assert(OR_T % 16 == 0 && OR_T >= 16 && OR_T <= 64, "a lane of 16 x 16 owns (T / 16)^2 pairs");
static_assert(4 * OR_THREADS >= OR_N, "lane t owns k = 4t .. 4t + 3");

const char* const kOrderRaw[GPIRT_ORDER_NARRAYS] = { "above", "cross", "easier", "depth_sum", "easiness", "set_counts" };

inline int order_raw_width(int k) { return k <= GPIRT_ORDER_EASIER ? 4 : 8; }
inline int64_t order_raw_count(int k, int64_t m, int n_tols)
{
    switch (k) {
        case GPIRT_ORDER_ABOVE: case GPIRT_ORDER_CROSS: return (int64_t)n_tols * m * m;
        case GPIRT_ORDER_EASIER: case GPIRT_ORDER_DEPTH_SUM: return m * m;
        case GPIRT_ORDER_EASINESS: return 2 * m;
        default: return 3 * OR_TOLS;               // GPIRT_ORDER_SET_COUNTS
    }
}

inline int64_t order_tiles(int64_t m)
{
    const int64_t nT = (m + OR_T - 1) / OR_T;
    return nT * (nT + 1) / 2;
}

// any item's curve not finite in this draw?  (the same answer in every work-group; the barrier is the callers' first)
__device__ __forceinline__ int order_skip(const unsigned char* __restrict__ bad, int64_t m)
{
    int b = 0;
    for (int64_t j = threadIdx.x; j < m; j += OR_THREADS) b |= bad[j];
    return __syncthreads_or(b);
}

__global__ __launch_bounds__(OR_THREADS) void order_easiness_kernel(const double* __restrict__ g, const unsigned char* __restrict__ bad,
                                                                    const double* __restrict__ w, int64_t m,
                                                                    double* __restrict__ e_out, double* __restrict__ easiness)
{
    __shared__ double part[OR_THREADS];
    if (order_skip(bad, m)) return;
    const int t = threadIdx.x;
    const int64_t j = blockIdx.x;
    const double* col = g + j * OR_N;
    double s = 0.0;
    for (int k = 4 * t; k < 4 * t + 4 && k < OR_N; ++k) s += w[k] / (1.0 + exp(-col[k]));
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        double e = 0.0;
        for (int q = 0; q < OR_THREADS; ++q) e += part[q];
        e_out[j] = e;
        easiness[j] += e;
        easiness[m + j] += e * e;
    }
}

struct OrderArgs {
    const double* g;                              // N x m, ld N
    const unsigned char* bad;
    const double* e;                              // this draw's easiness
    int64_t m;
    int klo, khi, n_tols;
    double tols[OR_TOLS];
    uint32_t *above, *cross, *easier;
    double *depth, *u;
    uint32_t* tile_part;                          // [tiles][OR_TOLS]
};

// the ordered cell (x, y): U = U[x, y], V = U[y, x] (so the minimum of g_x - g_y over W is -V); returns the tolerances at which
// the pair crosses as a bit mask
__device__ __forceinline__ unsigned order_cell(const OrderArgs& a, int64_t x, int64_t y, double U, double V, double ex, double ey)
{
    const int64_t m = a.m, at = x * m + y;
    unsigned mask = 0;
#pragma unroll
    for (int q = 0; q < OR_TOLS; ++q) {
        if (q < a.n_tols) {
            const double tol = a.tols[q];
            const bool hi = U > tol, lo = -V < -tol;
            if (hi && lo) { a.cross[(int64_t)q * m * m + at] += 1u; mask |= 1u << q; }
            else if (hi) a.above[(int64_t)q * m * m + at] += 1u;
        }
    }
    if (ex > ey) a.easier[at] += 1u;
    a.depth[at] += fmin(fmax(U, 0.0), fmax(V, 0.0));
    a.u[at] = U;
    return mask;
}

template <int T>
__global__ __launch_bounds__(OR_THREADS) void order_pair_kernel(OrderArgs a)
{
    constexpr int R = T / 16, LD = T + 2;
    __shared__ double sA[OR_KC * LD], sB[OR_KC * LD];
    __shared__ int red[OR_THREADS / 64][OR_TOLS];
    const int64_t m = a.m;
    if (order_skip(a.bad, m)) return;
    const int t = threadIdx.x;
    // the tile: the blocks count the pairs (A, B), A <= B, row by row
    const int nT = (int)((m + T - 1) / T);
    int rest = (int)blockIdx.x, A = 0;
    while (rest >= nT - A) { rest -= nT - A; ++A; }
    const int B = A + rest;
    const bool diag = A == B;
    const int ta = t & 15, tb = t >> 4;
    const int64_t a0 = (int64_t)A * T + R * ta, b0 = (int64_t)B * T + R * tb;
    const double inf = (double)INFINITY;
    double up[R][R], dn[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) { up[i][j] = -inf; dn[i][j] = inf; }

    for (int k0 = a.klo; k0 <= a.khi; k0 += OR_KC) {
        const int kc = a.khi - k0 + 1 < OR_KC ? a.khi - k0 + 1 : OR_KC;
        __syncthreads();                                          // the last chunk has been read
        for (int idx = t; idx < T * OR_KC; idx += OR_THREADS) {
            const int item = idx / OR_KC, kk = idx % OR_KC;
            const int64_t ja = (int64_t)A * T + item, jb = (int64_t)B * T + item;
            double va = 0.0, vb = 0.0;
            if (kk < kc) {                                        // k0 + kk <= khi <= 1000
                if (ja < m) va = a.g[ja * OR_N + k0 + kk];
                if (jb < m) vb = a.g[jb * OR_N + k0 + kk];
            }
            sA[kk * LD + item] = va;
            sB[kk * LD + item] = vb;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kc; ++kk) {
            double ga[R], gb[R];
#pragma unroll
            for (int i = 0; i < R; ++i) { ga[i] = sA[kk * LD + R * ta + i]; gb[i] = sB[kk * LD + R * tb + i]; }
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const double d = ga[i] - gb[j];
                    up[i][j] = fmax(up[i][j], d);
                    dn[i][j] = fmin(dn[i][j], d);
                }
        }
    }

    double ea[R], eb[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        ea[i] = a0 + i < m ? a.e[a0 + i] : 0.0;
        eb[i] = b0 + i < m ? a.e[b0 + i] : 0.0;
    }
    int cnt[OR_TOLS];
#pragma unroll
    for (int q = 0; q < OR_TOLS; ++q) cnt[q] = 0;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int64_t x = a0 + i, y = b0 + j;
            if (x >= m || y >= m) continue;
            const double U = up[i][j], V = -dn[i][j];             // U[x, y] and U[y, x]
            if (diag) {
                if (x == y) continue;                             // (u's diagonal stays 0)
                const unsigned mask = order_cell(a, x, y, U, V, ea[i], eb[j]);
                if (x < y) {
#pragma unroll
                    for (int q = 0; q < OR_TOLS; ++q) cnt[q] += (int)((mask >> q) & 1u);
                }
            } else {
                const unsigned mask = order_cell(a, x, y, U, V, ea[i], eb[j]);
                order_cell(a, y, x, V, U, eb[j], ea[i]);
#pragma unroll
                for (int q = 0; q < OR_TOLS; ++q) cnt[q] += (int)((mask >> q) & 1u);
            }
        }
#pragma unroll
    for (int q = 0; q < OR_TOLS; ++q)
        for (int off = 32; off; off >>= 1) cnt[q] += __shfl_xor(cnt[q], off, 64);
    if ((t & 63) == 0) {
#pragma unroll
        for (int q = 0; q < OR_TOLS; ++q) red[t >> 6][q] = cnt[q];
    }
    __syncthreads();
    if (t < OR_TOLS) {
        int s = 0;
        for (int v = 0; v < OR_THREADS / 64; ++v) s += red[v][t];
        a.tile_part[(int64_t)blockIdx.x * OR_TOLS + t] = (uint32_t)s;
    }
}

__global__ __launch_bounds__(OR_THREADS) void order_finish_kernel(const unsigned char* __restrict__ bad, int64_t m, int64_t tiles,
                                                                  int n_tols, const uint32_t* __restrict__ tile_part,
                                                                  int64_t* __restrict__ ncross, uint64_t* __restrict__ set_counts,
                                                                  int64_t* __restrict__ hdr)
{
    __shared__ unsigned long long red[OR_THREADS / 64][OR_TOLS];
    const int t = threadIdx.x;
    if (order_skip(bad, m)) {
        if (t == 0) hdr[11] += 1;                                 // skipped
        return;
    }
    unsigned long long s[OR_TOLS];
#pragma unroll
    for (int q = 0; q < OR_TOLS; ++q) s[q] = 0;
    for (int64_t i = t; i < tiles; i += OR_THREADS) {
#pragma unroll
        for (int q = 0; q < OR_TOLS; ++q) s[q] += tile_part[i * OR_TOLS + q];
    }
#pragma unroll
    for (int q = 0; q < OR_TOLS; ++q)
        for (int off = 32; off; off >>= 1) s[q] += __shfl_xor(s[q], off, 64);
    if ((t & 63) == 0) {
#pragma unroll
        for (int q = 0; q < OR_TOLS; ++q) red[t >> 6][q] = s[q];
    }
    __syncthreads();
    if (t < OR_TOLS) {
        unsigned long long nc = 0;
        for (int v = 0; v < OR_THREADS / 64; ++v) nc += red[v][t];
        if (t >= n_tols) nc = 0;
        ncross[t] = (int64_t)nc;
        if (t < n_tols) {
            set_counts[t] += nc == 0 ? 1u : 0u;                   // iio_draws
            set_counts[OR_TOLS + t] += nc;
            set_counts[2 * OR_TOLS + t] += nc * nc;
        }
    }
    if (t == 0) hdr[10] += 1;                                     // draws
}

// a state block on the host
struct HostOrder {
    std::vector<uint64_t> w;
    int64_t n = 0, m = 0;
    int n_tols = 0;
    OrderLayout L{};
    const int64_t* hdr() const { return reinterpret_cast<const int64_t*>(w.data()); }
    int64_t* hdr() { return reinterpret_cast<int64_t*>(w.data()); }
    template <class T> T* arr(int k) { return reinterpret_cast<T*>(w.data() + L.off[k]); }
};

int order_read(hipStream_t st, const void* d_state, HostOrder& r, int c)
{
    int64_t hdr[ORDER_HEADER_WORDS];
    GP_HIP(hipMemcpyAsync(hdr, d_state, sizeof(hdr), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (hdr[0] != ORDER_TAG || hdr[1] != ORDER_LAYOUT_VERSION || hdr[2] <= 0 || hdr[3] < 2 || hdr[3] > GPIRT_ORDER_MAX_M ||
        hdr[4] < 1 || hdr[4] > OR_CENTRE || hdr[5] < 1 || hdr[5] > OR_TOLS || hdr[10] < 0 || hdr[11] < 0) {
        set_error("gpirt_shape_order_combine: state %d is not an order state block of layout %d", c, ORDER_LAYOUT_VERSION);
        return GPIRT_E_ARG;
    }
    r.n = hdr[2]; r.m = hdr[3]; r.n_tols = (int)hdr[5];
    r.L = order_layout(r.m, r.n_tols);
    r.w.resize((size_t)r.L.words);
    GP_HIP(hipMemcpyAsync(r.w.data(), d_state, sizeof(uint64_t) * r.w.size(), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

OrderLayout order_layout(int64_t m, int n_tols)
{
    OrderLayout L{};
    int64_t at = ORDER_HEADER_WORDS;
    for (int k = 0; k < GPIRT_ORDER_NARRAYS; ++k) {
        L.off[k] = at;
        const int64_t bytes = order_raw_count(k, m, n_tols) * order_raw_width(k);
        at += (bytes + 15) / 16 * 2;                                  // whole 16-byte pieces
    }
    L.words = at;
    return L;
}

void order_free(OrderState* o)
{
    for (void* q : o->allocs) hipFree(q);
    *o = OrderState{};
}

int order_alloc(hipStream_t st, ShapeState* p)
{
    const int64_t m = p->m;
    if (m < 2 || m > GPIRT_ORDER_MAX_M) {
        set_error("order posteriors: m = %lld items, 2..%d are taken", (long long)m, GPIRT_ORDER_MAX_M);
        return GPIRT_E_ARG;
    }
    OrderState* o = &p->order;
    const OrderLayout L = order_layout(m, p->n_tols);
    auto get = [&](void** q, size_t bytes) -> int {
        GP_HIP(hipMalloc(q, bytes));
        o->allocs.push_back(*q);
        GP_HIP(hipMemsetAsync(*q, 0, bytes, st));
        return 0;
    };
    GP_TRY(get((void**)&o->block, sizeof(uint64_t) * (size_t)L.words));
    GP_TRY(get((void**)&o->u, sizeof(double) * (size_t)(m * m)));
    GP_TRY(get((void**)&o->e, sizeof(double) * (size_t)m));
    GP_TRY(get((void**)&o->ncross, sizeof(int64_t) * OR_TOLS));
    GP_TRY(get((void**)&o->tile_part, sizeof(uint32_t) * OR_TOLS * (size_t)order_tiles(m)));
    int64_t hdr[ORDER_HEADER_WORDS] = { ORDER_TAG, ORDER_LAYOUT_VERSION, p->n, m, p->k_half, p->n_tols };
    for (int q = 0; q < OR_TOLS; ++q) memcpy(&hdr[6 + q], &p->tols[q], sizeof(double));
    GP_HIP(hipMemcpyAsync(o->block, hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));        // hdr is this call's
    o->on = true;
    return 0;
}

int launch_order_accumulate(hipStream_t st, ShapeState* p, const double* gbar)
{
    OrderState* o = &p->order;
    const int64_t m = p->m, tiles = order_tiles(m);
    const OrderLayout L = order_layout(m, p->n_tols);
    auto u32 = [&](int k) { return reinterpret_cast<uint32_t*>(o->block + L.off[k]); };
    auto f64 = [&](int k) { return reinterpret_cast<double*>(o->block + L.off[k]); };
    hipLaunchKernelGGL(order_easiness_kernel, dim3((unsigned)m), dim3(OR_THREADS), 0, st, gbar, p->bad, p->w, m, o->e,
                       f64(GPIRT_ORDER_EASINESS));
    GP_HIP(hipGetLastError());
    OrderArgs a{};
    a.g = gbar; a.bad = p->bad; a.e = o->e; a.m = m;
    a.klo = OR_CENTRE - p->k_half; a.khi = OR_CENTRE + p->k_half; a.n_tols = p->n_tols;
    for (int q = 0; q < OR_TOLS; ++q) a.tols[q] = p->tols[q];
    a.above = u32(GPIRT_ORDER_ABOVE); a.cross = u32(GPIRT_ORDER_CROSS); a.easier = u32(GPIRT_ORDER_EASIER);
    a.depth = f64(GPIRT_ORDER_DEPTH_SUM); a.u = o->u; a.tile_part = o->tile_part;
    hipLaunchKernelGGL(order_pair_kernel<OR_T>, dim3((unsigned)tiles), dim3(OR_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    hipLaunchKernelGGL(order_finish_kernel, dim3(1), dim3(OR_THREADS), 0, st, p->bad, m, tiles, p->n_tols, o->tile_part, o->ncross,
                       o->block + L.off[GPIRT_ORDER_SET_COUNTS], reinterpret_cast<int64_t*>(o->block));
    GP_HIP(hipGetLastError());
    return 0;
}

int order_get(hipStream_t st, ShapeState* p, const char* name, void* h_out, int64_t bytes)
{
    OrderState* o = &p->order;
    const int64_t m = p->m;
    const OrderLayout L = order_layout(m, p->n_tols);
    auto copy = [&](const void* src) -> int {
        GP_HIP(hipMemcpyAsync(h_out, src, (size_t)bytes, hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        return 0;
    };
    if (strcmp(name, "counts") == 0) { GP_ARG(bytes == 16); return copy(o->block + 10); }
    if (strcmp(name, "u") == 0) { GP_ARG(bytes == 8 * m * m); return copy(o->u); }
    if (strcmp(name, "e") == 0) { GP_ARG(bytes == 8 * m); return copy(o->e); }
    if (strcmp(name, "ncross") == 0) { GP_ARG(bytes == 8 * OR_TOLS); return copy(o->ncross); }
    for (int k = 0; k < GPIRT_ORDER_NARRAYS; ++k)
        if (strcmp(kOrderRaw[k], name) == 0) {
            GP_ARG(bytes == order_raw_count(k, m, p->n_tols) * order_raw_width(k));
            return copy(o->block + L.off[k]);
        }
    set_error("unknown order field '%s'", name);
    return GPIRT_E_ARG;
}

int order_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_shape_order* out)
{
    GP_ARG(h && chains >= 1 && d_states && out);
    GP_ARG(out->reserved[0] == 0 && out->reserved[1] == 0 && out->reserved[2] == 0 && out->reserved[3] == 0);
    if (out->top < 1 || out->top > GPIRT_ORDER_MAX_TOP) {
        set_error("gpirt_shape_order_combine: top = %d is outside 1..%d", out->top, GPIRT_ORDER_MAX_TOP);
        return GPIRT_E_ARG;
    }
    for (int c = 0; c < chains; ++c) GP_ARG(d_states[c]);
    HostOrder pooled, one;
    for (int c = 0; c < chains; ++c) {
        HostOrder& r = c == 0 ? pooled : one;
        GP_TRY(order_read(h->stream, d_states[c], r, c));
        if (c == 0) continue;
        if (r.m != pooled.m || !std::equal(r.hdr() + 4, r.hdr() + 10, pooled.hdr() + 4)) {
            set_error("gpirt_shape_order_combine: state %d has another m, window or other tolerances than state 0", c);
            return GPIRT_E_ARG;
        }
        pooled.hdr()[10] += one.hdr()[10];
        pooled.hdr()[11] += one.hdr()[11];
        for (int k = 0; k < GPIRT_ORDER_NARRAYS; ++k) {
            const int64_t cnt = order_raw_count(k, r.m, r.n_tols);
            if (order_raw_width(k) == 4) for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint32_t>(k)[g] += one.arr<uint32_t>(k)[g];
            else if (k == GPIRT_ORDER_SET_COUNTS) for (int64_t g = 0; g < cnt; ++g) pooled.arr<uint64_t>(k)[g] += one.arr<uint64_t>(k)[g];
            else for (int64_t g = 0; g < cnt; ++g) pooled.arr<double>(k)[g] += one.arr<double>(k)[g];      // in chain order
        }
    }
    const int64_t* hd = pooled.hdr();
    const int64_t m = pooled.m;
    out->k_half = (int)hd[4]; out->n_tols = pooled.n_tols;
    for (int q = 0; q < OR_TOLS; ++q) memcpy(&out->tols[q], &hd[6 + q], sizeof(double));
    out->n = pooled.n; out->m = m; out->draws = hd[10]; out->skipped = hd[11];
    for (int k = 0; k < GPIRT_ORDER_NARRAYS; ++k)
        if (out->raw[k])
            memcpy(out->raw[k], pooled.w.data() + pooled.L.off[k], (size_t)(order_raw_count(k, m, pooled.n_tols) * order_raw_width(k)));
    // the pairs a < b that cross most often at the largest tolerance; scanned in (a, b) order, so a tie keeps the lowest pair
    int qmax = 0;
    for (int q = 1; q < pooled.n_tols; ++q) if (out->tols[q] > out->tols[qmax]) qmax = q;
    const uint32_t* cross = pooled.arr<uint32_t>(GPIRT_ORDER_CROSS) + (int64_t)qmax * m * m;
    struct Top { uint32_t c; int64_t a, b; };
    std::vector<Top> top;
    const size_t want = (size_t)out->top;
    for (int64_t a = 0; a < m; ++a)
        for (int64_t b = a + 1; b < m; ++b) {
            const uint32_t c = cross[a * m + b];
            if (top.size() == want && c <= top.back().c) continue;
            size_t at = top.size();
            while (at > 0 && top[at - 1].c < c) --at;
            top.insert(top.begin() + (std::ptrdiff_t)at, Top{ c, a, b });
            if (top.size() > want) top.pop_back();
        }
    out->n_worst = (int64_t)top.size();
    for (size_t i = 0; i < want; ++i) {
        if (out->worst_a) out->worst_a[i] = i < top.size() ? top[i].a : -1;
        if (out->worst_b) out->worst_b[i] = i < top.size() ? top[i].b : -1;
    }
    return 0;
}

}  // namespace gpirt
