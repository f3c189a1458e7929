// factor_lr.hip -- what the fast preset's steady iteration reads of the factor L of S = K(theta, theta) + eps I, from theta
// alone: the 512-column diagonal parts L[P, P] (nu_lr.hip's structured nu = L z) and the 64 node rows Bt = K(c, theta) L^-T
// below the factor (nu_lr.hip's records, draw_fstar's G = B^T B).  The triangle of L below the parts is NOT computed.
//
// With V[i][k] = l_k(theta_i) (nu_lr.hip's basis, n x 64), Kcc = K(c, c) = F F^T (fstar_free.hip) and K(theta, theta) =
// V Kcc V^T the Schur complement of S in front of the part P = [p, p + w) is, by the Woodbury step of fstar_free.hip on the
// leading block,
//       S_PP - S_{P,<p} S_{<p,<p}^-1 S_{<p,P} = eps I + V[P] (eps F (H_P + eps I)^-1 F^T) V[P]^T,   H_P = F^T G_P F,
// G_P = V[<p]^T V[<p] the Gram of the basis rows in front of the part (G_0 = 0).  With A_P = H_P + eps I = R_P R_P^T,
// Xh_P = R_P^-1 F^T (64 x 64) and X_P = Xh_P V[P]^T (64 x w):
//       S_PP = eps (I + X_P^T X_P)              (a sum of positive terms: every pivot of its factor is >= sqrt(eps))
//       L_PP = chol(S_PP)
//       Bt[:, P] = eps Xh_P^T (X_P L_PP^-T)
// The parts depend on each other through the running Gram alone: behind an element-wise prefix over the parts' Grams in part
// order all parts are factored side by side, eight rounds of 64 columns, the 64 rows of X_P riding along as a border that
// leaves the factorisation as X_P L_PP^-T (the bordered trick of potrf.hip at part scale).  1.5e9 flop at n = 8192 instead of
// n^3 / 3 = 1.8e11, and a pivot chain of 8 links instead of 128.
//
// Ordinary work-groups on the caller's stream, every sum in a fixed order: no atomics, no flags, no spinning.  Nothing here
// depends on m, item0 or the shard.
#include "common.h"
#include "kernels.h"
#include "potf2.h"
#include "solve64.h"

namespace gpirt {

namespace {

constexpr int NR = NU_LR_RANK;
constexpr int64_t PC = NU_LR_PART;
constexpr int NBLK = (int)(PC / 64);                 // 64-column rounds of a full part
static_assert(NR == 64, "potf2.h and solve64.h are written for 64 x 64");

// G[0] <- 0, G[q] <- g[1] + ... + g[q] for the Grams g[q] found in slot q (q = 1 .. nslot - 1), in slot order, element by
// element (nu_scan_kernel's pattern): slot P then holds the Gram of the basis rows in front of part P
__global__ __launch_bounds__(256) void flr_scan_kernel(double* __restrict__ G, int nslot)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= NR * NR) return;
    double run = 0.0;
    G[e] = 0.0;
    for (int q = 1; q < nslot; ++q) { run += G[(int64_t)q * NR * NR + e]; G[(int64_t)q * NR * NR + e] = run; }
}

// Round k of the parts' factorisation, all parts side by side.  Work-group (rb, q) belongs to part q, whose pivot block D is
// the 64 x 64 block at column c0 = 512 q + 64 k of L's diagonal.  EVERY work-group of the part factors D itself, in LDS
// (potf2.h; eps is added to its diagonal here: the product in front wrote eps X^T X) -- nothing passes between work-groups,
// and nobody writes D in this launch -- and then solves its own 64 rows B <- B D^-T with the substitution core of the
// factorisation's panels (solve64.h, 16 rows a wavefront):  rb == 0: the border, the 64 rows of X at the pivot's columns (and
// it keeps D's factor in Dw, which flr_diag_kernel puts in place behind the last round);  rb >= 1: rows c0 + 64 rb of the part.
// A pivot that is not positive raises *err (the sampler's numeric error word).
__global__ __launch_bounds__(256) void flr_panel_kernel(double* __restrict__ L, int64_t ldl, int64_t n, double* __restrict__ X,
                                                        double* __restrict__ Dw, int k, double eps, int* __restrict__ err)
{
    __shared__ __attribute__((aligned(16))) double sM[NR * S64_LS];
    __shared__ __attribute__((aligned(16))) double sP[2 * 4 * NR];
    __shared__ int sfail, sinfo;
    const int64_t p0 = (int64_t)blockIdx.y * PC;
    const int nb = (int)(((n - p0) < PC ? (n - p0) : PC) / 64);         // 64-column blocks of this part
    const int rb = (int)blockIdx.x;
    if (k >= nb || rb > nb - 1 - k) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int64_t c0 = p0 + 64 * (int64_t)k;
    const double* D = L + c0 * (ldl + 1);
    double* B = (rb == 0 ? X + (int64_t)NR * c0 : L + c0 * (ldl + 1) + 64 * (int64_t)rb) + wave * 16 + i;      // this lane's row
    const int64_t ldb = rb == 0 ? NR : ldl;
    d4 Xv[4];
#pragma unroll
    for (int J = 0; J < 4; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) Xv[J][r] = B[(16 * J + 4 * g + r) * ldb];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int idx = t + 256 * q;
        const int r = idx & (NR - 1), c = idx >> 6;
        sM[c * S64_LS + r] = r >= c ? D[r + c * ldl] + (r == c ? eps : 0.0) : 0.0;
    }
    if (t == 0) sinfo = 0;
    __syncthreads();
    potf2_64_body(sM, S64_LS, NR, 0, &sinfo, sP, &sfail);
    if (t == 0 && sfail != 0x7fffffff && err) atomicCAS(err, 0, (int)GPIRT_E_NUMERIC);
    if (rb == 0) {
        double* out = Dw + ((int64_t)blockIdx.y * NBLK + k) * NR * NR;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int idx = t + 256 * q;
            out[idx] = sM[(idx >> 6) * S64_LS + (idx & (NR - 1))];
        }
    }
    __syncthreads();
    invert_diag16(sM);
    solve64_lower_inv(Xv, sM);
#pragma unroll
    for (int J = 0; J < 4; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) B[(16 * J + 4 * g + r) * ldb] = Xv[J][r];
}

// the pivot blocks' factors from Dw into L's diagonal (the strict upper triangle inside a block: zero)
__global__ __launch_bounds__(256) void flr_diag_kernel(double* __restrict__ L, int64_t ldl, int64_t n, const double* __restrict__ Dw)
{
    const int k = (int)blockIdx.x;
    const int64_t c0 = (int64_t)blockIdx.y * PC + 64 * (int64_t)k;
    if (c0 >= n) return;
    const double* in = Dw + ((int64_t)blockIdx.y * NBLK + k) * NR * NR;
    double* D = L + c0 * (ldl + 1);
    for (int idx = threadIdx.x; idx < NR * NR; idx += 256) D[(idx & (NR - 1)) + (int64_t)(idx >> 6) * ldl] = in[idx];
}

}  // namespace

int64_t factor_lr_parts(int64_t n) { return (n + PC - 1) / PC; }

// The diagonal parts into a.L (lower triangles; the strict upper triangle inside a part is zero, nothing below the parts is
// written) and the node rows into a.Bt.  V: n x 64 (ld n), rewritten with the basis at theta; G, Xh: factor_lr_parts(n) x
// 64 x 64; X: 64 x n; D: factor_lr_parts(n) x 8 x 64 x 64.  n a multiple of 64; the last part may be shorter than 512.
// h (may be null): the handle whose profiler books the syrk-lower launches -- S_PP under class 1, the in-part updates
// under class 2.
int launch_factor_lr(gpirt_handle_t h, hipStream_t stream, const FactorLrArgs& a)
{
    const int64_t n = a.n, ldl = a.ldl;
    if (n <= 0) return 0;
    if ((n % 64) != 0) { set_error("factor_lr: n must be a multiple of 64"); return GPIRT_E_ARG; }
    const int64_t full = n / PC, rem = n % PC;
    const int parts = (int)(full + (rem ? 1 : 0));
    const int64_t sG = (int64_t)NR * NR, sX = (int64_t)NR * PC, sL = PC * (ldl + 1);
    auto syrk = [&](int cls, bool ta, int64_t M, double alpha, const double* A, int64_t lda, int64_t sA, double beta, double* C, int batch) -> int {
        if (M <= 0 || batch <= 0) return 0;
        ProfPair pp;
        if (h) GP_TRY(prof_pair_begin(h, stream, pp));
        GP_TRY(launch_gemm_batched(stream, ta, !ta, TRI_SYRK_LOWER, M, M, NR, alpha, A, lda, sA, A, lda, sA, beta, C, ldl, sL, batch));
        // the lower triangle of C written (and read, where it is updated), the M x 64 operand read once
        const double tri = 0.5 * (double)M * (double)(M + 1) * (double)batch;
        if (h) GP_TRY(prof_pair_end(h, stream, pp, cls, 2.0 * NR * tri, 8.0 * ((beta != 0.0 ? 2.0 : 1.0) * tri + (double)(M * NR) * (double)batch)));
        return 0;
    };
    GP_TRY(launch_nu_lr_basis(stream, a.theta, n, a.nodes, a.wts, a.V));
    // the Grams of every part but the last (all full) into slots 1 .. parts - 1, then the prefix: slot P = G_P
    if (parts > 1)
        GP_TRY(launch_gemm_batched(stream, true, false, TRI_NONE, NR, NR, PC, 1.0, a.V, n, PC, a.V, n, PC, 0.0, a.G + sG, NR, sG, parts - 1));
    hipLaunchKernelGGL(flr_scan_kernel, dim3((unsigned)((NR * NR + 255) / 256)), dim3(256), 0, stream, a.G, parts);
    GP_HIP(hipGetLastError());
    GP_TRY(launch_fstar_free_xhat(stream, a.G, a.F, a.eps, a.Xh, parts, a.err));
    // X_P = Xh_P V[P]^T, then eps X_P^T X_P into the parts of L (flr_panel_kernel adds eps I)
    if (full > 0) GP_TRY(launch_gemm_batched(stream, false, true, TRI_NONE, NR, PC, NR, 1.0, a.Xh, NR, sG, a.V, n, PC, 0.0, a.X, NR, sX, (int)full));
    if (rem > 0) GP_TRY(launch_gemm_batched(stream, false, true, TRI_NONE, NR, rem, NR, 1.0, a.Xh + full * sG, NR, 0, a.V + full * PC, n, 0, 0.0, a.X + full * sX, NR, 0, 1));
    GP_TRY(syrk(1, true, PC, a.eps, a.X, NR, sX, 0.0, a.L, (int)full));
    GP_TRY(syrk(1, true, rem, a.eps, a.X + full * sX, NR, 0, 0.0, a.L + full * sL, 1));
    // the parts' factorisation with X_P as the border: a round factors the pivot blocks and solves the rows below them, then
    // takes the new columns' products off what lies to their right (the part's trailing triangle, the border's columns)
    const int rounds = full > 0 ? NBLK : (int)(rem / 64);
    for (int k = 0; k < rounds; ++k) {
        hipLaunchKernelGGL(flr_panel_kernel, dim3((unsigned)(rounds - k), (unsigned)parts), dim3(256), 0, stream, a.L, ldl, n, a.X, a.D, k, a.eps, a.err);
        GP_HIP(hipGetLastError());
        const int64_t c = 64 * (int64_t)k, c1 = c + 64;
        auto update = [&](int64_t w, int64_t part0, int batch) -> int {
            const int64_t Mt = w - c1;
            if (Mt <= 0 || batch <= 0) return 0;
            double* Lp = a.L + part0 * sL;
            double* Xp = a.X + part0 * sX;
            GP_TRY(syrk(2, false, Mt, -1.0, Lp + c1 + c * ldl, ldl, batch > 1 ? sL : 0, 1.0, Lp + c1 * (ldl + 1), batch));
            return launch_gemm_batched(stream, false, true, TRI_NONE, NR, Mt, NR, -1.0, Xp + NR * c, NR, batch > 1 ? sX : 0, Lp + c1 + c * ldl, ldl,
                                       batch > 1 ? sL : 0, 1.0, Xp + NR * c1, NR, batch > 1 ? sX : 0, batch);
        };
        GP_TRY(update(PC, 0, (int)full));
        GP_TRY(update(rem, full, 1));
    }
    hipLaunchKernelGGL(flr_diag_kernel, dim3((unsigned)rounds, (unsigned)parts), dim3(256), 0, stream, a.L, ldl, n, a.D);
    GP_HIP(hipGetLastError());
    // Bt[:, P] = eps Xh_P^T (X_P L_PP^-T)
    if (full > 0) GP_TRY(launch_gemm_batched(stream, true, false, TRI_NONE, NR, PC, NR, a.eps, a.Xh, NR, sG, a.X, NR, sX, 0.0, a.Bt, ldl, PC * ldl, (int)full));
    if (rem > 0) GP_TRY(launch_gemm_batched(stream, true, false, TRI_NONE, NR, rem, NR, a.eps, a.Xh + full * sG, NR, 0, a.X + full * sX, NR, 0, 0.0,
                                            a.Bt + full * PC * ldl, ldl, 0, 1));
    return 0;
}

}  // namespace gpirt
