// fstar_free.hip -- the rank-64 draw_fstar's C = S^-1 U (n x 64) from theta alone, WITHOUT the transposed solve through L.
//
// S = K(theta, theta) + eps I, U = K(theta, c), c the 64 Chebyshev nodes of cheb_nodes_basis(64).  With V[i][k] = l_k(theta_i)
// (nu_lr.hip's basis, n x 64) and Kcc = K(c, c) the same rank-64 fact draw_f's structured product rests on gives
//       K(theta, theta) = V Kcc V^T,      U = V Kcc        (1e-15 per entry under a kernel that passes the certificate).
// Let Kcc = F F^T (F 64 x 64: a property of the kernel alone, from the host, fstar_free_factor) and Y = V F.  Then
//       S = Y Y^T + eps I,     C = S^-1 Y F^T = Y (Y^T Y + eps I)^-1 F^T = V M,
//       M = F (F^T (V^T V) F + eps I)^-1 F^T                   (64 x 64, symmetric; the inner matrix has cond <= cond(S))
// -- one 64 x 64 x n Gram product, one 64 x 64 factorisation and solve in one work-group, one n x 64 x 64 product, and no
// dependence on the factor: the chain starts as soon as the basis at theta exists, not when the last pivot block of the
// factorisation does.  With A = F^T (V^T V) F + eps I = R R^T and X = R^-1 F^T the small matrix is M = X^T X.
//
// G = B^T B is NOT taken from the closed form Kcc - eps M: that difference is not positive semi-definite in floating point
// (s = 1 - sqrt(v^T G v) is then wrong by 1e-5 where the quadratic form is near 0); the caller keeps the product over the
// node rows the bordered factorisation leaves.
//
// Ordinary work-groups on the caller's stream: no flags, no spinning.  Nothing here depends on m, item0 or the shard.
#include <float.h>

#include "common.h"
#include "kernels.h"
#include "potf2.h"
#include "solve64.h"

namespace gpirt {

namespace {

constexpr int FR = FSTAR_FREE_RANK;
constexpr int FLD = FR + 1;                        // LDS column stride (doubles): odd, so rows and columns both spread over the banks
constexpr size_t FF_LDS = sizeof(double) * (3 * FR * FLD + 2 * FR);

// acc[ii][jj] = sum_k opA(4 ti + ii, k) opB(k, 4 tj + jj), k in index order.  Column-major 64 x 64 blocks with stride FLD:
// TA: opA(i, k) = A[k + FLD i] (A^T), else A[i + FLD k];  TB: opB(k, j) = B[j + FLD k] (B^T), else B[k + FLD j]
template <bool TA, bool TB>
__device__ __forceinline__ void mm64(const double* __restrict__ A, const double* __restrict__ B, int ti, int tj, double (&acc)[4][4])
{
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = 0.0;
#pragma unroll 4
    for (int k = 0; k < FR; ++k) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = TA ? A[k + FLD * (4 * ti + u)] : A[(4 * ti + u) + FLD * k];
            b[u] = TB ? B[(4 * tj + u) + FLD * k] : B[k + FLD * (4 * tj + u)];
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = fma(a[ii], b[jj], acc[ii][jj]);
    }
}

__device__ __forceinline__ void put64(double* __restrict__ D, int ti, int tj, const double (&acc)[4][4])
{
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) D[(4 * ti + ii) + FLD * (4 * tj + jj)] = acc[ii][jj];
}

// M = F (F^T Gv F + eps I)^-1 F^T, one work-group of 256 threads.  Gv, F, M: 64 x 64, column-major, dense.
// Thread (ti, tj) = (t & 15, t >> 4) owns the 4 x 4 tile at rows 4 ti, columns 4 tj of every 64 x 64 matrix.  The Cholesky
// factorisation and the forward substitution keep their matrix in those register tiles and pass one column / one row a step
// through LDS (two buffers in turn: one barrier a step).
// A pivot that is not positive and finite raises *err (the sampler's numeric error word) and M is left all NaN.
__global__ __launch_bounds__(256) void fstar_free_small_kernel(const double* __restrict__ Gv, const double* __restrict__ F, double eps,
                                                               double* __restrict__ M, int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) double ff_lds[];
    double* P = ff_lds;                      // Gv, then the Cholesky factor R of A (lower)
    double* Q = ff_lds + FR * FLD;           // F
    double* W = ff_lds + 2 * FR * FLD;       // Gv F, then X = R^-1 F^T
    double* line = ff_lds + 3 * FR * FLD;    // 2 x 64: the step's column of A / row of X
    const int t = threadIdx.x, ti = t & 15, tj = t >> 4;
    for (int e = t; e < FR * FR; e += 256) {
        const int i = e & (FR - 1), j = e >> 6;
        P[i + FLD * j] = Gv[e];
        Q[i + FLD * j] = F[e];
    }
    __syncthreads();
    double acc[4][4], a[4][4];
    mm64<false, false>(P, Q, ti, tj, acc);                   // W = Gv F
    put64(W, ti, tj, acc);
    __syncthreads();
    mm64<true, false>(Q, W, ti, tj, a);                      // A = F^T (Gv F) + eps I, in the register tiles
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (ti == tj) a[u][u] += eps;
    // Cholesky, right-looking: column k goes through LDS, every thread scales it and updates its own tile.  Only the lower
    // triangle means anything (what the tiles hold above it is never read).
    bool bad = false;
    for (int kb = 0; kb < FR / 4; ++kb) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = 4 * kb + kk;
            double* col = line + (k & 1) * FR;
            if (tj == kb) {
#pragma unroll
                for (int u = 0; u < 4; ++u) col[4 * ti + u] = a[u][kk];
            }
            __syncthreads();
            double d = col[k];                                           // (the same value in every thread)
            if (!(d > 0.0) || !(d <= 1.79769313486231570815e308)) { bad = true; d = 1.0; }
            const double r = sqrt(d), inv = 1.0 / r;
            double li[4], lj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { li[u] = col[4 * ti + u] * inv; lj[u] = col[4 * tj + u] * inv; }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    if (tj > kb || (tj == kb && jj > kk)) a[ii][jj] -= li[ii] * lj[jj];
            if (tj == kb) {
#pragma unroll
                for (int u = 0; u < 4; ++u) a[u][kk] = (4 * ti + u == k) ? r : li[u];
            }
        }
    }
    if (bad) {
        if (t == 0 && err) atomicCAS(err, 0, (int)GPIRT_E_NUMERIC);
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int e = t; e < FR * FR; e += 256) M[e] = nan;
        return;
    }
    put64(P, ti, tj, a);                                     // R
    // X = R^-1 F^T, right-looking: row k of X is final once divided by R(k, k); it goes through LDS and every thread takes
    // R(i, k) x_k off its rows i > k
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) a[ii][jj] = Q[(4 * tj + jj) + FLD * (4 * ti + ii)];       // F^T
    __syncthreads();
    for (int kb = 0; kb < FR / 4; ++kb) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = 4 * kb + kk;
            double* row = line + (k & 1) * FR;
            if (ti == kb) {
                const double rkk = P[k + FLD * k];
#pragma unroll
                for (int u = 0; u < 4; ++u) { a[kk][u] = a[kk][u] / rkk; row[4 * tj + u] = a[kk][u]; }
            }
            __syncthreads();
            double rk[4], xr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { rk[u] = P[(4 * ti + u) + FLD * k]; xr[u] = row[4 * tj + u]; }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    if (ti > kb || (ti == kb && ii > kk)) a[ii][jj] -= rk[ii] * xr[jj];
        }
    }
    put64(W, ti, tj, a);                                     // X(k, j) at W[k + FLD j]
    __syncthreads();
    mm64<true, false>(W, W, ti, tj, acc);                    // M = X^T X: M(i, j) = sum_k X(k, i) X(k, j), the same sum for (j, i)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) M[(4 * ti + ii) + FR * (4 * tj + jj)] = acc[ii][jj];
}

// Xh = R^-1 F^T with R R^T = F^T Gv F + eps I for `gridDim.x` matrices Gv 64 x 64 apart, one work-group each (factor_lr.hip:
// a part's X-hat; the first half of the kernel above, which it leaves as it is).  The two products as above; A is then
// factored in LDS by the factorisation's own 64 x 64 Cholesky (potf2.h) and each wavefront solves R x = f for 16 rows f of F
// with its substitution core (solve64.h): x is column i of Xh for row i of F.
// A pivot that is not positive raises *err (the sampler's numeric error word).
// prefix: the slots of Gv hold the parts' own Grams and work-group P first adds those of slots 1 .. P itself, element by
// element in slot order from zero -- flr_scan_kernel's sums, so its bits, without its launch (slot 0 is not read: G_0 = 0).
// Rout (the centred amplitude update, amp_centred.hip; nullptr for everybody else, whose code it leaves as it was): R itself,
// 64 x 64 column-major with zeros above the diagonal, stored before its diagonal blocks are inverted in place.
constexpr size_t FX_LDS = sizeof(double) * (3 * FR * FLD + 2 * 4 * FR);
static_assert(FR * S64_LS <= 2 * FR * FLD, "the staged factor takes the place of Gv and Gv F");
__device__ __forceinline__ void fstar_free_xhat_body(const double* __restrict__ Gv, const double* __restrict__ F, double eps,
                                                     double* __restrict__ Xh, int* __restrict__ err, const bool prefix,
                                                     double* __restrict__ Rout = nullptr, const bool chain = false)
{
    extern __shared__ __attribute__((aligned(16))) double ff_lds[];
    __shared__ int sfail, sinfo;
    double* Q = ff_lds;                      // F
    double* P = ff_lds + FR * FLD;           // Gv
    double* W = ff_lds + 2 * FR * FLD;       // Gv F
    double* sM = P;                          // A, then R, with solve64.h's stride (over P and W, both dead by then)
    double* sP = ff_lds + 3 * FR * FLD;      // potf2_64_body's two panels
    const int t = threadIdx.x, ti = t & 15, tj = t >> 4;
    const int lane = t & 63, wave = t >> 6, i = lane & 15, g = lane >> 4;
    // (a link of the fused structured factor's chain, 16 work-groups that share their SIMDs with draw_beta's waves: ahead of them at issue)
    if (prefix || chain) __builtin_amdgcn_s_setprio(3);
    Xh += (int64_t)blockIdx.x * FR * FR;
    for (int e = t; e < FR * FR; e += 256) {
        const int r = e & (FR - 1), c = e >> 6;
        double gv;
        if (prefix) {
            gv = 0.0;
            for (int q = 1; q <= (int)blockIdx.x; ++q) gv += Gv[(int64_t)q * FR * FR + e];
        } else {
            gv = Gv[(int64_t)blockIdx.x * FR * FR + e];
        }
        P[r + FLD * c] = gv;
        Q[r + FLD * c] = F[e];
    }
    if (t == 0) sinfo = 0;
    __syncthreads();
    double acc[4][4], a[4][4];
    mm64<false, false>(P, Q, ti, tj, acc);                   // W = Gv F
    put64(W, ti, tj, acc);
    __syncthreads();
    mm64<true, false>(Q, W, ti, tj, a);                      // A = F^T (Gv F) + eps I
    __syncthreads();                                         // (every thread has read P and W: A goes over them)
#pragma unroll
    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int r = 4 * ti + ii, c = 4 * tj + jj;
            sM[c * S64_LS + r] = r >= c ? a[ii][jj] + (r == c ? eps : 0.0) : 0.0;
        }
    d4 X[4];                                                 // this lane's row of F
#pragma unroll
    for (int J = 0; J < 4; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) X[J][r] = Q[(wave * 16 + i) + FLD * (16 * J + 4 * g + r)];
    __syncthreads();
    potf2_64_body(sM, S64_LS, FR, 0, &sinfo, sP, &sfail);
    if (t == 0 && sfail != 0x7fffffff && err) atomicCAS(err, 0, (int)GPIRT_E_NUMERIC);
    if (Rout) {
        Rout += (int64_t)blockIdx.x * FR * FR;
        for (int e = t; e < FR * FR; e += 256) Rout[e] = sM[(e >> 6) * S64_LS + (e & (FR - 1))];
        __syncthreads();                                     // (read before wave 0 inverts the diagonal blocks)
    }
    invert_diag16(sM);
    solve64_lower_inv(X, sM);
#pragma unroll
    for (int J = 0; J < 4; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) Xh[(16 * J + 4 * g + r) + FR * (wave * 16 + i)] = X[J][r];
}

__global__ __launch_bounds__(256) void fstar_free_xhat_kernel(const double* __restrict__ Gv, const double* __restrict__ F, double eps,
                                                              double* __restrict__ Xh, int* __restrict__ err)
{
    fstar_free_xhat_body(Gv, F, eps, Xh, err, false);
}

__global__ __launch_bounds__(256) void fstar_free_xhat_r_kernel(const double* __restrict__ Gv, const double* __restrict__ F, double eps,
                                                                double* __restrict__ Xh, double* __restrict__ R, int* __restrict__ err)
{
    fstar_free_xhat_body(Gv, F, eps, Xh, err, false, R);
}

// The prefix form runs on the fused structured factor's chain while the sampler's side stream fills the chip with
// draw_beta_kernel (stages.hip: 104 registers, four waves on every SIMD, which leaves 96 of a SIMD's 512 registers free).
// Held to 96 registers (five waves a SIMD; the rest spills to scratch) its 16 work-groups start beside those waves; with
// the 146 it would otherwise take they wait until the first draw_beta work-groups retire, 0.15 ms later.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5)))
void fstar_free_xhat_prefix_kernel(const double* __restrict__ Gv, const double* __restrict__ F, double eps, double* __restrict__ Xh, int* __restrict__ err)
{
    fstar_free_xhat_body(Gv, F, eps, Xh, err, true);
}

// the prefix form's place on the chain -- its register cap, its priority -- for slots that already hold the prefix (factor_lr.hip's
// two-level sum for parts narrower than 512)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5)))
void fstar_free_xhat_chain_kernel(const double* __restrict__ Gv, const double* __restrict__ F, double eps, double* __restrict__ Xh, int* __restrict__ err)
{
    fstar_free_xhat_body(Gv, F, eps, Xh, err, false, nullptr, true);
}

}  // namespace

// F (64 x 64, column-major) with K(c, c) = F F^T for the handle's kernel at the nodes of nu_lr_nodes: Kcc in long double, a
// cyclic Jacobi eigendecomposition in long double (Kcc's small eigenvalues lie far below fp64's rounding of its large ones),
// negative eigenvalues clipped to 0, F = Q sqrt(Lambda) rounded to fp64.  Host only; a squared-exponential kernel.
void fstar_free_factor(const KernelSpec& kern, std::vector<double>& F)
{
    std::vector<double> nodes, wts;
    nu_lr_nodes(nodes, wts);
    std::vector<long double> A((size_t)(FR * FR)), Q((size_t)(FR * FR), 0.0L);
    for (int i = 0; i < FR; ++i) {
        Q[(size_t)(i + FR * i)] = 1.0L;
        for (int j = 0; j < FR; ++j) {
            const long double r = fabsl((long double)nodes[(size_t)i] - (long double)nodes[(size_t)j]) / (long double)kern.length_scale;
            A[(size_t)(i + FR * j)] = expl(-0.5L * r * r);
        }
    }
    auto at = [&](std::vector<long double>& X, int i, int j) -> long double& { return X[(size_t)(i + FR * j)]; };
    for (int sweep = 0; sweep < 60; ++sweep) {
        long double off = 0.0L, diag = 0.0L;
        for (int i = 0; i < FR; ++i)
            for (int j = 0; j < FR; ++j) (i == j ? diag : off) += at(A, i, j) * at(A, i, j);
        if (sqrtl(off) <= LDBL_EPSILON * sqrtl(diag)) break;
        for (int p = 0; p < FR - 1; ++p)
            for (int q = p + 1; q < FR; ++q) {
                const long double apq = at(A, p, q);
                if (apq == 0.0L) continue;
                const long double th = (at(A, q, q) - at(A, p, p)) / (2.0L * apq);
                const long double tt = th != 0.0L ? (th > 0.0L ? 1.0L : -1.0L) / (fabsl(th) + sqrtl(th * th + 1.0L)) : 1.0L;
                const long double c = 1.0L / sqrtl(tt * tt + 1.0L), s = tt * c;
                for (int i = 0; i < FR; ++i) {                    // A <- A J
                    const long double x = at(A, i, p), y = at(A, i, q);
                    at(A, i, p) = c * x - s * y; at(A, i, q) = s * x + c * y;
                }
                for (int i = 0; i < FR; ++i) {                    // A <- J^T A
                    const long double x = at(A, p, i), y = at(A, q, i);
                    at(A, p, i) = c * x - s * y; at(A, q, i) = s * x + c * y;
                }
                for (int i = 0; i < FR; ++i) {                    // Q <- Q J
                    const long double x = at(Q, i, p), y = at(Q, i, q);
                    at(Q, i, p) = c * x - s * y; at(Q, i, q) = s * x + c * y;
                }
            }
    }
    F.resize((size_t)(FR * FR));
    for (int k = 0; k < FR; ++k) {
        const long double lam = at(A, k, k);
        const long double sq = lam > 0.0L ? sqrtl(lam) : 0.0L;
        for (int i = 0; i < FR; ++i) F[(size_t)(i + FR * k)] = (double)(at(Q, i, k) * sq);
    }
}

// Cu (n x 64, ld n) = V M with M = F (F^T (V^T V) F + eps I)^-1 F^T.  V: n x 64 (ld n), the basis at theta; F: 64 x 64;
// work: 2 x 64 x 64 doubles (V^T V, then M behind it); parts: nsplit x 64 x 64 doubles for the split-K Gram product.
int launch_fstar_free(hipStream_t stream, const double* V, int64_t n, const double* F, double eps, double* work, double* parts,
                      int nsplit, double* Cu, int* err)
{
    if (n <= 0) return 0;
    double* Gv = work;
    double* M = work + FR * FR;
    GP_TRY(launch_gemm_splitk(stream, true, false, FR, FR, n, 1.0, V, n, V, n, parts, FR, (int64_t)FR * FR, nsplit, Gv, FR, 0.0));
    GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fstar_free_small_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FF_LDS));
    hipLaunchKernelGGL(fstar_free_small_kernel, dim3(1), dim3(256), FF_LDS, stream, Gv, F, eps, M, err);
    GP_HIP(hipGetLastError());
    // an un-split 64-tile product: an element of Cu depends on its row of V and on M alone
    return launch_gemm_batched(stream, false, false, TRI_NONE, n, FR, FR, 1.0, V, n, 0, M, FR, 0, 0.0, Cu, n, 0, 1);
}

// Xh[q] = R_q^-1 F^T with R_q R_q^T = F^T Gv[q] F + eps I for `batch` matrices Gv[q] (64 x 64 each, 4096 doubles apart), one
// work-group per matrix.  prefix: matrix q is the sum of the slots 1 .. q of Gv, formed by its work-group (see the kernel);
// chain: the prefix form's register cap and priority without its sum
int launch_fstar_free_xhat(hipStream_t stream, const double* Gv, const double* F, double eps, double* Xh, int batch, int* err, bool prefix,
                           double* R, bool chain)
{
    if (batch <= 0) return 0;
    if (chain && (prefix || R)) { set_error("fstar_free_xhat: the chain form takes the slots as they stand and keeps no R"); return GPIRT_E_ARG; }
    if (R) {
        if (prefix) { set_error("fstar_free_xhat: R is not kept in the prefix form"); return GPIRT_E_ARG; }
        GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fstar_free_xhat_r_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FX_LDS));
        hipLaunchKernelGGL(fstar_free_xhat_r_kernel, dim3((unsigned)batch), dim3(256), FX_LDS, stream, Gv, F, eps, Xh, R, err);
        GP_HIP(hipGetLastError());
        return 0;
    }
    auto* kernel = prefix ? fstar_free_xhat_prefix_kernel : chain ? fstar_free_xhat_chain_kernel : fstar_free_xhat_kernel;
    GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FX_LDS));
    hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(256), FX_LDS, stream, Gv, F, eps, Xh, err);
    GP_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpirt
