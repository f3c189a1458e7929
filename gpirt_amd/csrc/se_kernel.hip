// se_kernel.hip -- the covariance K(x1, x2) (src/covariance-function.cpp:3-14) with the +jitter diagonal of
// src/gpirtMCMC.cpp:16,77,96 fused in: the reference's squared exponential exp(-d^2 / 2) and, chosen per handle
// (gpirt_kernel_set), the squared exponential with a length scale and the Matern 5/2 and 3/2 forms.
//
// HBM-write bound (8 n1 n2 bytes out, 8 (n1+n2) bytes in): each work-group produces a 128-row x
// 32-column tile; a lane owns two consecutive rows, so every store instruction writes one
// contiguous 1 KiB segment of a column.  The `lower` variant visits only the 128 x 128 tiles on or
// below the block diagonal -- all the blocked Cholesky ever reads -- halving bytes and exp() work.
//
// se_tile is instantiated per family.  KF_DEFAULT is the reference's kernel with the expression it has always had (the bits of
// K and of everything behind it do not move for a handle whose kernel was never set); the other three scale |d| by 1 / ell,
// formed once on the host.  In one dimension |a - b| needs no square root: the Matern forms cost one fabs, the products of a
// short polynomial and the same exp() as the squared exponential, all under the write bound.
//
// Host side, below the launches: the argument checks of gpirt_kernel and the rank certificate of gpirt_kernel_check.
#include "common.h"
#include "kernels.h"

#include <cmath>

namespace gpirt {

namespace {

constexpr int TR = 128;   // tile rows
constexpr int TC = 32;    // tile columns

constexpr int KF_DEFAULT = -1;         // GPIRT_KERNEL_SE at length scale 1: exp(-0.5 d d) as written
#define GP_SQRT5 2.2360679774997896964
#define GP_SQRT3 1.7320508075688772935

// k(|d| / ell) for one entry; -ffp-contract=off (Makefile): every product and sum below rounds once, in this order
template <int FAM>
__device__ __forceinline__ double kernel_value(double d, double inv_ell)
{
    if (FAM == KF_DEFAULT) return exp(-0.5 * d * d);
    if (FAM == GPIRT_KERNEL_SE) {
        const double r = d * inv_ell;
        return exp(-0.5 * r * r);
    }
    const double r = fabs(d) * inv_ell;
    if (FAM == GPIRT_KERNEL_MATERN52) {
        const double a = GP_SQRT5 * r;
        return ((1.0 + a) + (a * a) * (1.0 / 3.0)) * exp(-a);
    }
    const double a = GP_SQRT3 * r;     // GPIRT_KERNEL_MATERN32
    return (1.0 + a) * exp(-a);
}

template <int FAM>
__device__ __forceinline__ void se_tile(const double* __restrict__ x1, int64_t n1,
                                        const double* __restrict__ x2, int64_t n2,
                                        double* __restrict__ out, int64_t ld, double jitter, double inv_ell,
                                        int64_t i0, int64_t j0, bool lower_only, bool fp32 = false)
{
    const int t = threadIdx.x;
    const int64_t r = i0 + (t & 63) * 2;
    const bool in0 = r < n1, in1 = (r + 1) < n1;
    const double a0 = in0 ? x1[r] : 0.0;
    const double a1 = in1 ? x1[r + 1] : 0.0;
    const bool vec = in1 && ((ld & 1) == 0) && ((((uintptr_t)out) & 15) == 0);
#pragma unroll
    for (int p = 0; p < TC / 4; ++p) {
        const int64_t c = j0 + (t >> 6) + 4 * p;
        if (c >= n2) break;
        const double b = x2[c];
        const double d0 = a0 - b, d1 = a1 - b;
        double v0, v1;
        if (FAM == KF_DEFAULT && fp32) {      // config C5: single-precision kernel build feeding the fp64 factorisation
            v0 = (double)expf((float)(-0.5 * d0 * d0));
            v1 = (double)expf((float)(-0.5 * d1 * d1));
        } else {
            v0 = kernel_value<FAM>(d0, inv_ell);
            v1 = kernel_value<FAM>(d1, inv_ell);
        }
        if (r == c) v0 += jitter;
        if (r + 1 == c) v1 += jitter;
        if (lower_only) {                 // strict upper part of a diagonal tile: exact zeros
            if (r < c) v0 = 0.0;
            if (r + 1 < c) v1 = 0.0;
        }
        double* o = out + r + c * ld;
        if (vec) {
            *reinterpret_cast<double2*>(o) = make_double2(v0, v1);
        } else {
            if (in0) o[0] = v0;
            if (in1) o[1] = v1;
        }
    }
}

template <int FAM>
__global__ __launch_bounds__(256) void se_kernel_full(const double* __restrict__ x1, int64_t n1,
                                                      const double* __restrict__ x2, int64_t n2,
                                                      double* __restrict__ out, int64_t ld,
                                                      double jitter, double inv_ell, int rblocks)
{
    const int64_t bi = blockIdx.x % rblocks, bj = blockIdx.x / rblocks;
    se_tile<FAM>(x1, n1, x2, n2, out, ld, jitter, inv_ell, bi * TR, bj * TC, false);
}

// blockIdx.x enumerates (lower block pair, 32-column strip) ; pairs are 128 x 128
template <int FAM>
__global__ __launch_bounds__(256) void se_kernel_lower(const double* __restrict__ x, int64_t n,
                                                       double* __restrict__ out, int64_t ld,
                                                       double jitter, double inv_ell, bool fp32)
{
    const int strip = blockIdx.x & 3;
    const int t = blockIdx.x >> 2;
    int r = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    while (r * (r + 1) / 2 > t) --r;
    const int bi = r, bj = t - r * (r + 1) / 2;
    se_tile<FAM>(x, n, x, n, out, ld, jitter, inv_ell, (int64_t)bi * TR, (int64_t)bj * 128 + strip * TC, bi == bj, fp32);
}

// the instantiation a spec selects (an unknown family never gets here: kernel_spec_from refuses it)
int family_index(const KernelSpec& k)
{
    return k.is_default() ? KF_DEFAULT : k.family;
}

}  // namespace

int launch_se_kernel(hipStream_t stream, KernelSpec kern, const double* x1, int64_t n1, const double* x2, int64_t n2,
                     double* out, int64_t ld, double jitter)
{
    if (n1 <= 0 || n2 <= 0) return 0;
    const int rblocks = (int)((n1 + TR - 1) / TR);
    const int64_t cblocks = (n2 + TC - 1) / TC;
    const dim3 grid((unsigned)(rblocks * cblocks)), block(256);
#define GP_FULL(F) hipLaunchKernelGGL(se_kernel_full<F>, grid, block, 0, stream, x1, n1, x2, n2, out, ld, jitter, kern.inv_ell, rblocks)
    switch (family_index(kern)) {
    case KF_DEFAULT: GP_FULL(KF_DEFAULT); break;
    case GPIRT_KERNEL_SE: GP_FULL(GPIRT_KERNEL_SE); break;
    case GPIRT_KERNEL_MATERN52: GP_FULL(GPIRT_KERNEL_MATERN52); break;
    case GPIRT_KERNEL_MATERN32: GP_FULL(GPIRT_KERNEL_MATERN32); break;
    default: set_error("unknown kernel family %d", kern.family); return GPIRT_E_ARG;
    }
#undef GP_FULL
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_se_kernel_lower(hipStream_t stream, KernelSpec kern, const double* x, int64_t n, double* out, int64_t ld,
                           double jitter, bool fp32)
{
    if (n <= 0) return 0;
    if (fp32 && !kern.is_default()) {
        set_error("the single-precision kernel build (kernel_fp32) needs the default kernel");
        return GPIRT_E_ARG;
    }
    const int64_t nb = (n + 127) / 128;
    const int64_t pairs = nb * (nb + 1) / 2;
    const dim3 grid((unsigned)(pairs * 4)), block(256);
#define GP_LOWER(F) hipLaunchKernelGGL(se_kernel_lower<F>, grid, block, 0, stream, x, n, out, ld, jitter, kern.inv_ell, fp32)
    switch (family_index(kern)) {
    case KF_DEFAULT: GP_LOWER(KF_DEFAULT); break;
    case GPIRT_KERNEL_SE: GP_LOWER(GPIRT_KERNEL_SE); break;
    case GPIRT_KERNEL_MATERN52: GP_LOWER(GPIRT_KERNEL_MATERN52); break;
    case GPIRT_KERNEL_MATERN32: GP_LOWER(GPIRT_KERNEL_MATERN32); break;
    default: set_error("unknown kernel family %d", kern.family); return GPIRT_E_ARG;
    }
#undef GP_LOWER
    GP_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- host: gpirt_kernel, the rank certificate -------------------
int kernel_spec_from(const gpirt_kernel* k, KernelSpec* out)
{
    if (!k) { set_error("bad argument: the kernel is NULL"); return GPIRT_E_ARG; }
    if (k->family < GPIRT_KERNEL_SE || k->family > GPIRT_KERNEL_MATERN32) {
        set_error("kernel: family %d is not one of GPIRT_KERNEL_SE (0), GPIRT_KERNEL_MATERN52 (1), GPIRT_KERNEL_MATERN32 (2)", k->family);
        return GPIRT_E_ARG;
    }
    if (k->reserved0 != 0 || k->reserved[0] != 0 || k->reserved[1] != 0 || k->reserved[2] != 0 || k->reserved[3] != 0) {
        set_error("kernel: the reserved words must be 0");
        return GPIRT_E_ARG;
    }
    const double ell = k->length_scale;
    if (!std::isfinite(ell) || !(ell >= GPIRT_LENGTH_SCALE_MIN) || !(ell <= GPIRT_LENGTH_SCALE_MAX)) {
        set_error("kernel: length_scale = %g, it must be finite and lie in %g .. %g (the lower limit is the spacing of the theta grid)",
                  ell, (double)GPIRT_LENGTH_SCALE_MIN, (double)GPIRT_LENGTH_SCALE_MAX);
        return GPIRT_E_ARG;
    }
    if (out) { out->family = k->family; out->length_scale = ell; out->inv_ell = 1.0 / ell; }
    return 0;
}

void cheb_nodes_basis(int r, std::vector<double>& nodes, std::vector<double>& V)
{
    const int64_t N = GPIRT_NGRID;
    const long double pi = 3.141592653589793238462643383279502884L;
    std::vector<long double> w((size_t)r);
    nodes.resize((size_t)r); V.assign((size_t)(N * r), 0.0);
    for (int k = 0; k < r; ++k) {
        const long double a = (2 * k + 1) * pi / (2 * r);
        w[(size_t)k] = ((k & 1) ? -1.0L : 1.0L) * sinl(a);
        nodes[(size_t)k] = (double)(5.0L * cosl(a));
    }
    for (int64_t j = 0; j < N; ++j) {
        const long double t = (long double)(-5.0 + (double)j * 0.01);     // src/gpirtMCMC.cpp:35
        int hit = -1;
        long double den = 0.0L;
        for (int k = 0; k < r; ++k) {
            const long double d = t - (long double)nodes[(size_t)k];     // the nodes as the device will see them
            if (d == 0.0L) { hit = k; break; }
            den += w[(size_t)k] / d;
        }
        for (int k = 0; k < r; ++k) {
            long double v;
            if (hit >= 0) v = (k == hit) ? 1.0L : 0.0L;
            else v = (w[(size_t)k] / (t - (long double)nodes[(size_t)k])) / den;
            V[(size_t)(j + k * N)] = (double)v;
        }
    }
}

namespace {

long double kernel_value_ld(const KernelSpec& kern, long double a, long double b)
{
    const long double r = fabsl(a - b) / (long double)kern.length_scale;
    if (kern.family == GPIRT_KERNEL_SE) return expl(-0.5L * r * r);
    if (kern.family == GPIRT_KERNEL_MATERN52) {
        const long double q = sqrtl(5.0L) * r;
        return (1.0L + q + q * q / 3.0L) * expl(-q);
    }
    const long double q = sqrtl(3.0L) * r;
    return (1.0L + q) * expl(-q);
}

// max over theta and theta* on the grid of |sum_k K(theta, c_k) V[theta*][k] - K(theta, theta*)|, long double, V as fp64
double rank_certificate(const KernelSpec& kern, int r)
{
    const int64_t N = GPIRT_NGRID;
    std::vector<double> nodes, V;
    cheb_nodes_basis(r, nodes, V);
    std::vector<long double> Vt((size_t)(N * r)), U((size_t)(N * r)), kd((size_t)N);      // Vt[j][k], U[i][k]; K on the grid by |i - j|
    for (int64_t j = 0; j < N; ++j)
        for (int k = 0; k < r; ++k) Vt[(size_t)(j * r + k)] = (long double)V[(size_t)(j + k * N)];
    std::vector<double> ts((size_t)N);
    for (int64_t i = 0; i < N; ++i) ts[(size_t)i] = -5.0 + (double)i * 0.01;
    for (int64_t i = 0; i < N; ++i)
        for (int k = 0; k < r; ++k) U[(size_t)(i * r + k)] = kernel_value_ld(kern, (long double)ts[(size_t)i], (long double)nodes[(size_t)k]);
    long double worst = 0.0L;
    for (int64_t i = 0; i < N; ++i) {
        const long double* u = &U[(size_t)(i * r)];
        for (int64_t j = 0; j < N; ++j) {
            const long double* v = &Vt[(size_t)(j * r)];
            long double acc = 0.0L;
            for (int k = 0; k < r; ++k) acc += u[k] * v[k];
            const long double e = fabsl(acc - kernel_value_ld(kern, (long double)ts[(size_t)i], (long double)ts[(size_t)j]));
            if (e > worst) worst = e;
        }
    }
    return (double)worst;
}

}  // namespace

int kernel_rank_check(const KernelSpec& kern, int kstar_rank, double* cert_out, int* min_rank_out)
{
    if (cert_out) *cert_out = 0.0;
    if (min_rank_out) *min_rank_out = 0;
    if (kstar_rank == 0) return 0;
    if (kstar_rank < 16 || kstar_rank > 128 || (kstar_rank % 16) != 0) {
        set_error("kstar_rank must be 0 or a multiple of 16 in 16..128");
        return GPIRT_E_ARG;
    }
    const double cert = rank_certificate(kern, kstar_rank);
    if (cert_out) *cert_out = cert;
    if (kern.family != GPIRT_KERNEL_SE) {
        set_error("kstar_rank = %d is refused: a Matern kernel is not analytic at r = 0 and has no rank form that is exact to rounding "
                  "(certificate max |K(theta, c) V^T - K(theta, theta*)| = %.3g); use kstar_rank = 0", kstar_rank, cert);
        return GPIRT_E_ARG;
    }
    KernelSpec unit;
    static const double line = rank_certificate(unit, 48);            // "exact to rounding": (SE, 1.0, r = 48) by the same routine
    if (cert <= line) return 0;
    int min_rank = 0;
    for (int r = 16; r <= 128 && !min_rank; r += 16)
        if (r != kstar_rank && rank_certificate(kern, r) <= line) min_rank = r;
    if (min_rank_out) *min_rank_out = min_rank;
    if (min_rank)
        set_error("kstar_rank = %d is refused under the squared exponential with length_scale = %g: its certificate max |K(theta, c) V^T - "
                  "K(theta, theta*)| = %.3g exceeds %.3g, that of (length_scale 1, r = 48); the smallest rank that passes is %d",
                  kstar_rank, kern.length_scale, cert, line, min_rank);
    else
        set_error("kstar_rank = %d is refused under the squared exponential with length_scale = %g: its certificate max |K(theta, c) V^T - "
                  "K(theta, theta*)| = %.3g exceeds %.3g, that of (length_scale 1, r = 48), and no rank up to 128 passes; use kstar_rank = 0",
                  kstar_rank, kern.length_scale, cert, line);
    return GPIRT_E_ARG;
}

}  // namespace gpirt
