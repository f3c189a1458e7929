// nu_lr.hip -- draw_f's product nu = L z WITHOUT the blocks of L below its 512-column diagonal parts (item-keyed RNG).
//
// S = K(theta, theta) + jitter I is a smooth kernel matrix plus a multiple of the identity, so for a row i below a block of
// columns P the factor is   L[i, P] = K(theta_i, theta_P) L_PP^-T   (the jitter sits on the diagonal only), and with the
// r = 64 Chebyshev nodes c on [-5, 5] and the Lagrange basis V[i][k] = l_k(theta_i) (cheb_nodes_basis: 1e-15 per entry for
// the unit squared exponential; kernel_rank_check's certificate for any other handle kernel)
//       K(theta_i, .) = sum_k V[i][k] K(c_k, .)      =>      L[i, P] = V[i, :] Bt[:, P],    Bt = K(c, theta) L^-T   (64 x n).
// Bt is what the bordered factorisation leaves in the 64 node rows below L (sampler.hip: node_off), for free.  With the n
// columns cut into parts P of 512:
//       nu[P, :] = L[P, P] Z[P, :]  +  V[P, :] sum_{Q < P} Bt[:, Q] Z[Q, :]
// -- the dense 512 x 512 lower-triangular diagonal parts, a 64 x 512 x m product per part, a running sum over the parts in
// part order, and a 512 x 64 x m product per part: 6.5e9 flop at 8192 x 1024 instead of n^2 m = 6.9e10.  rs_lr.hip uses the
// same structure in single precision with coefficients rebuilt from theta, as a predictor; here it is fp64 with the factor's
// own rows and IS the product (to rounding: DESIGN.md has the measured bound).
//
// Every launch is an un-split 64-tile product of launch_gemm_batched or the element-wise scan below: what produces one
// element of nu depends on its row, its item's column of Z and the factor, not on m, item0 or how many parts ride together
// (an item shard's nu is bit-identical to the same columns of the full problem).  Ordinary work-groups on the caller's
// stream: no flags, no spinning, no hand-off between work-groups.
#include "common.h"
#include "kernels.h"

namespace gpirt {

namespace {

constexpr int NR = NU_LR_RANK;
constexpr int NB_ROWS = 32, NB_G = 8;        // nu_basis_kernel: rows per work-group, threads per row

// V[i + k n] = l_k(theta_i), barycentric form in fp64.  ONE formula whether theta_i is a grid value or not (a theta on a
// node gets that node's unit vector); theta clamped to the nodes' interval and a NaN set to 0 only so that the row is finite
// -- the product is not taken with such a theta (the sampler's theta_ok)
__global__ __launch_bounds__(256) void nu_basis_kernel(const double* __restrict__ theta, int64_t n, const double* __restrict__ nodes,
                                                       const double* __restrict__ wts, double* __restrict__ V)
{
    // 32 rows per work-group, eight threads to a row with eight nodes each (a thread per row spent 20 us at n = 8192 on its
    // 128 fp64 divisions); the eight partial sums of a row are added in group order
    __shared__ double c[NR], w[NR], part[NB_G][NB_ROWS];
    __shared__ int hitk[NB_ROWS];
    const int tid = threadIdx.x;
    if (tid < NR) { c[tid] = nodes[tid]; w[tid] = wts[tid]; }
    if (tid < NB_ROWS) hitk[tid] = -1;
    __syncthreads();
    const int r = tid % NB_ROWS, g = tid / NB_ROWS;
    const int64_t i = (int64_t)blockIdx.x * NB_ROWS + r;
    const bool live = i < n;
    double t = live ? theta[i] : 0.0;
    t = t < -5.0 ? -5.0 : (t > 5.0 ? 5.0 : t);
    if (!(t == t)) t = 0.0;
    double q[NR / NB_G], s = 0.0;
#pragma unroll
    for (int j = 0; j < NR / NB_G; ++j) {
        const int k = g * (NR / NB_G) + j;
        const double d = t - c[k];
        if (d == 0.0) { hitk[r] = k; q[j] = 0.0; } else { q[j] = w[k] / d; s += q[j]; }
    }
    part[g][r] = s;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int u = 0; u < NB_G; ++u) tot += part[u][r];
    const int hit = hitk[r];
    if (!live) return;
#pragma unroll
    for (int j = 0; j < NR / NB_G; ++j) {
        const int k = g * (NR / NB_G) + j;
        V[i + (int64_t)k * n] = (hit >= 0) ? (k == hit ? 1.0 : 0.0) : q[j] / tot;
    }
}

// T[q] <- T[0] + ... + T[q], q = 1 .. nslab - 1, in slab order (slab = the 64 x m record of one part), element by element
__global__ __launch_bounds__(256) void nu_scan_kernel(double* __restrict__ T, int64_t slab, int nslab)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= slab) return;
    double run = T[e];
    int q = 1;
    for (; q + 4 <= nslab; q += 4) {
        double t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = T[(int64_t)(q + u) * slab + e];
#pragma unroll
        for (int u = 0; u < 4; ++u) { run += t[u]; T[(int64_t)(q + u) * slab + e] = run; }
    }
    for (; q < nslab; ++q) { run += T[(int64_t)q * slab + e]; T[(int64_t)q * slab + e] = run; }
}

}  // namespace

// the 64 nodes of cheb_nodes_basis(64) and their barycentric weights (host, once per sampler)
void nu_lr_nodes(std::vector<double>& nodes, std::vector<double>& wts)
{
    std::vector<double> V;
    cheb_nodes_basis(NR, nodes, V);
    wts.resize((size_t)NR);
    const long double pi = 3.141592653589793238462643383279502884L;
    for (int k = 0; k < NR; ++k) wts[(size_t)k] = (double)(((k & 1) ? -1.0L : 1.0L) * sinl((2 * k + 1) * pi / (2 * NR)));
}

int64_t nu_lr_slabs(int64_t n) { const int64_t parts = (n + NU_LR_PART - 1) / NU_LR_PART; return parts > 1 ? parts - 1 : 1; }

int launch_nu_lr_basis(hipStream_t stream, const double* theta, int64_t n, const double* nodes, const double* wts, double* V)
{
    hipLaunchKernelGGL(nu_basis_kernel, dim3((unsigned)((n + NB_ROWS - 1) / NB_ROWS)), dim3(NB_ROWS * NB_G), 0, stream, theta, n, nodes, wts, V);
    GP_HIP(hipGetLastError());
    return 0;
}

// NU (n x m, ld n) = L Z as above.  L: the factor (ld ldl), Bt: its 64 node rows (ld ldl), V: n x 64 (ld n), Z: n x m (ld n),
// T: nu_lr_slabs(n) slabs of 64 x m.  n a multiple of 64; the last part may be shorter than 512.
int launch_nu_lr(hipStream_t stream, const NuLrArgs& a, double* flops, double* bytes)
{
    constexpr int64_t PC = NU_LR_PART;
    const int64_t n = a.n, m = a.m, ldl = a.ldl;
    if (n <= 0 || m <= 0) return 0;
    if ((n % 64) != 0) { set_error("nu_lr: n must be a multiple of 64"); return GPIRT_E_ARG; }
    const int64_t full = n / PC, rem = n % PC, parts = full + (rem ? 1 : 0);
    const int64_t slab = (int64_t)NR * m;
    const int nslab = (int)(parts - 1);                  // (the last part's record has no rows below it)
    // T_P = Bt[:, P] Z[P, :]: every part that has rows below it is a full one
    if (nslab > 0) {
        GP_TRY(launch_gemm_batched(stream, false, false, TRI_NONE, NR, m, PC, 1.0, a.Bt, ldl, PC * ldl, a.Z, n, PC, 0.0, a.T, NR, slab, nslab));
        if (nslab > 1) {
            hipLaunchKernelGGL(nu_scan_kernel, dim3((unsigned)((slab + 255) / 256)), dim3(256), 0, stream, a.T, slab, nslab);
            GP_HIP(hipGetLastError());
        }
    }
    // the diagonal parts, dense
    if (full > 0)
        GP_TRY(launch_gemm_batched(stream, false, false, TRI_A_LOWER, PC, m, PC, 1.0, a.L, ldl, PC * (ldl + 1), a.Z, n, PC, 0.0, a.NU, n, PC, (int)full));
    if (rem > 0)
        GP_TRY(launch_gemm_batched(stream, false, false, TRI_A_LOWER, rem, m, rem, 1.0, a.L + full * PC * (ldl + 1), ldl, 0, a.Z + full * PC, n, 0, 0.0,
                                   a.NU + full * PC, n, 0, 1));
    // += V[P, :] (T_0 + ... + T_{P-1}), P >= 1
    if (full > 1)
        GP_TRY(launch_gemm_batched(stream, false, false, TRI_NONE, PC, m, NR, 1.0, a.V + PC, n, PC, a.T, NR, slab, 1.0, a.NU + PC, n, PC, (int)(full - 1)));
    if (rem > 0 && full > 0)
        GP_TRY(launch_gemm_batched(stream, false, false, TRI_NONE, rem, m, NR, 1.0, a.V + full * PC, n, 0, a.T + (full - 1) * slab, NR, 0, 1.0,
                                   a.NU + full * PC, n, 0, 1));
    // algorithmic work: the triangles of the diagonal parts, the two rank-64 products per part below the first
    const double dn = (double)n, dm = (double)m, tri = (double)full * (double)(PC * PC) + (double)(rem * rem);
    if (flops) *flops = tri * dm + 2.0 * (double)NR * dm * (nslab > 0 ? (double)(nslab * PC) + (double)(n - PC) : 0.0);
    if (bytes) *bytes = 8.0 * (0.5 * tri + 2.0 * (double)NR * dn + 2.0 * dn * dm + 3.0 * dn * dm + 3.0 * (double)(slab * (nslab > 0 ? nslab : 0)));
    return 0;
}

}  // namespace gpirt
