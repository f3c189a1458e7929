// nu_lr.hip -- draw_f's product nu = L z WITHOUT the blocks of L below its diagonal parts (item-keyed RNG).
//
// S = K(theta, theta) + jitter I is a smooth kernel matrix plus a multiple of the identity, so for a row i below a block of
// columns P the factor is   L[i, P] = K(theta_i, theta_P) L_PP^-T   (the jitter sits on the diagonal only), and with the
// r = 64 Chebyshev nodes c on [-5, 5] and the Lagrange basis V[i][k] = l_k(theta_i) (cheb_nodes_basis: 1e-15 per entry for
// the unit squared exponential; kernel_rank_check's certificate for any other handle kernel)
//       K(theta_i, .) = sum_k V[i][k] K(c_k, .)      =>      L[i, P] = V[i, :] Bt[:, P],    Bt = K(c, theta) L^-T   (64 x n).
// Bt is what the bordered factorisation leaves in the 64 node rows below L (sampler.hip: node_off), for free.  The identity
// holds for every row block strictly below every column block, so the n columns may be cut into parts P of any multiple of
// 64: w = 64, 128, 256 or 512 (GPIRT_NU_SUB, default NU_LR_SUB; the structured FACTOR's parts are at least as wide, up to
// NU_LR_PART = 512, and the w-wide diagonal blocks lie inside them):
//       nu[P, :] = L[P, P] Z[P, :]  +  V[P, :] sum_{Q < P} Bt[:, Q] Z[Q, :]
// -- the dense w x w lower-triangular diagonal parts and two rank-64 products, n m (w + 256) flop: 3.2e9 at 8192 x 1024 and
// w = 128 (6.4e9 at 512) instead of n^2 m = 6.9e10.  Four launches:
//   nu_basis_kernel      V at theta
//   records              slab Q + 1 <- Bt[:, Q] Z[Q, :] for every part with rows below it (batched, K = w)
//   nu_scan_kernel       running sums over the slabs in part order: slab P = sum_{Q < P} T_Q; slab 0 is zero, always
//   consumer             nu[P, :] = L[P, P] Z[P, :] + V[P, :] slab_P, both products in ONE accumulator per 64-tile
//                        (launch_gemm_batched_dual): nu is written once and never read back
// (a ragged last part, a multiple of 64 rows, is a second consumer launch).  rs_lr.hip uses the same structure in single
// precision with coefficients rebuilt from theta, as a predictor; here it is fp64 with the factor's own rows and IS the
// product (to rounding: DESIGN.md has the measured bound).
//
// Every launch is an un-split 64-tile product or the element-wise scan below.  The summation order of an element of nu is
// fixed -- the triangle's K range ascending, then the 64 node terms ascending -- and depends on its row, its item's column of
// Z, the factor and w, not on m, item0 or how many parts ride together (an item shard's nu is bit-identical to the same
// columns of the full problem).  Ordinary work-groups on the caller's stream: no flags, no spinning, no atomics, no hand-off
// between work-groups.
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

// slabs of 64 x m in T: the zero slab and one record per part but the last at the narrowest width (so that GPIRT_NU_SUB can change
// on a live sampler)
int64_t nu_lr_slabs(int64_t n) { const int64_t parts = (n + NU_LR_SUB_MIN - 1) / NU_LR_SUB_MIN; return parts > 1 ? parts : 1; }

int launch_nu_lr_basis(hipStream_t stream, const double* theta, int64_t n, const double* nodes, const double* wts, double* V)
{
    hipLaunchKernelGGL(nu_basis_kernel, dim3((unsigned)((n + NB_ROWS - 1) / NB_ROWS)), dim3(NB_ROWS * NB_G), 0, stream, theta, n, nodes, wts, V);
    GP_HIP(hipGetLastError());
    return 0;
}

// NU (n x m, ld n) = L Z as above, in parts of w = a.sub columns.  L: the factor (ld ldl), Bt: its 64 node rows (ld ldl), V: n x 64
// (ld n), Z: n x m (ld n), T: nu_lr_slabs(n) slabs of 64 x m whose slab 0 holds zeros (the owner zeroes it once; nothing here
// writes it).  n a multiple of 64; the last part may be shorter than w.
int launch_nu_lr(hipStream_t stream, const NuLrArgs& a, double* flops, double* bytes)
{
    const int64_t n = a.n, m = a.m, ldl = a.ldl;
    const int64_t w = a.sub ? a.sub : NU_LR_SUB;
    if (!nu_lr_sub_ok((int)w)) { set_error("nu_lr: the part width (GPIRT_NU_SUB) is %d; it must be 64, 128, 256 or 512", (int)w); return GPIRT_E_ARG; }
    if (n <= 0 || m <= 0) return 0;
    if ((n % 64) != 0) { set_error("nu_lr: n must be a multiple of 64"); return GPIRT_E_ARG; }
    const int64_t full = n / w, rem = n % w, parts = full + (rem ? 1 : 0);
    const int64_t slab = (int64_t)NR * m;
    const int nrec = (int)(parts - 1);                   // (the last part's record has no rows below it)
    // slab Q + 1 <- T_Q = Bt[:, Q] Z[Q, :]: every part that has rows below it is a full one; then the running sums in part
    // order, so that slab P holds sum_{Q < P} T_Q (slab 0: zero)
    if (nrec > 0) {
        GP_TRY(launch_gemm_batched(stream, false, false, TRI_NONE, NR, m, w, 1.0, a.Bt, ldl, w * ldl, a.Z, n, w, 0.0, a.T + slab, NR, slab, nrec));
        if (nrec > 1) {
            hipLaunchKernelGGL(nu_scan_kernel, dim3((unsigned)((slab + 255) / 256)), dim3(256), 0, stream, a.T + slab, slab, nrec);
            GP_HIP(hipGetLastError());
        }
    }
    // nu[P, :] = L[P, P] Z[P, :] + V[P, :] slab_P: the triangle's K range, then the 64 node terms, in one accumulator
    if (full > 0)
        GP_TRY(launch_gemm_batched_dual(stream, TRI_A_LOWER, w, m, w, a.L, ldl, w * (ldl + 1), a.Z, n, w, NR, a.V, n, w, a.T, NR, slab, a.NU, n, w,
                                        (int)full));
    if (rem > 0)
        GP_TRY(launch_gemm_batched_dual(stream, TRI_A_LOWER, rem, m, rem, a.L + full * w * (ldl + 1), ldl, 0, a.Z + full * w, n, 0, NR, a.V + full * w, n,
                                        0, a.T + full * slab, NR, 0, a.NU + full * w, n, 0, 1));
    // what ran: the triangles of the diagonal parts, the records' rank-64 product and the consumer's (every part, the first
    // against the zero slab); the slabs are written by the records, read and written by the scan and read by the consumer
    const double dn = (double)n, dm = (double)m, tri = (double)full * (double)(w * w) + (double)(rem * rem);
    const double rec = (double)nrec, sl = (double)slab;
    if (flops) *flops = tri * dm + 2.0 * (double)NR * dm * (rec * (double)w + dn);
    if (bytes) *bytes = 8.0 * (0.5 * tri + 2.0 * (double)NR * dn + 2.0 * dn * dm + dn * dm + sl * (rec + (nrec > 1 ? 2.0 * rec : 0.0) + (double)parts));
    return 0;
}

}  // namespace gpirt
