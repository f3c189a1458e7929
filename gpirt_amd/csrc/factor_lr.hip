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
//
// Two schedules of the same sums (GPIRT_FLR_FUSE): 1, the default, one launch per round
// (flr_round_kernel: 12 launches at n = 8192); 2, a panel launch and two product launches per round (29 launches).
//
// The identities hold for any cut into multiples of 64, and the steady iteration reads no more of L than diagonal parts as
// wide as draw_f's product takes them (GPIRT_NU_SUB, 128 by default): FactorLrArgs::part = 64, 128, 256 or 512 is the width
// of the parts built here (GPIRT_FLR_NARROW), part / 64 rounds instead of eight -- 7 launches at
// n = 8192 and part = 128.  At 512 every launch is what it was; below it the prefix over the Grams is flr_scan2_kernel's.
#include "common.h"
#include "kernels.h"
#include "potf2.h"
#include "solve64.h"

namespace gpirt {

namespace {

constexpr int NR = NU_LR_RANK;
// The part width PC and NBLK = PC / 64, the 64-column rounds of a full part, are launch arguments (`part`: 64, 128, 256 or
// NU_LR_PART = 512, FactorLrArgs::part): whoever reads no more of L than w-wide diagonal parts is given w-wide parts,
// part / 64 rounds instead of eight.
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

// The same prefix for parts narrower than 512 columns, where the slots are many (n / part: 64 at n = 8192 and part = 128) and a
// serial sum per element is a chain of that many dependent adds behind as many loads.  Two levels in a fixed order, no atomics:
// with c = 512 / part slots a group (the parts of one 512-column stretch), g[p] the Gram of part p (found in slot p + 1),
//       H_j = g[j c] + ... + g[j c + c - 1]          (from zero, ascending: the Gram of stretch j)
//       G_P = (H_0 + ... + H_{J-1}) + (g[J c] + ... + g[P - 1]),   J = P / c        (both sums from zero, ascending)
// A work-group holds 256 / ng elements of all groups, thread (element, group): it loads its group's c Grams (all loads in
// flight together), leaves H_j in LDS, and behind the barrier -- every slot has been read by then: slot j c + c belongs to the
// next group's thread -- adds the groups in front and writes its c slots.  ng: the groups' count rounded up to a power of two.
constexpr int FLR_SCAN_THREADS = 256;
constexpr int FLR_SCAN_CMAX = NU_LR_PART / NU_LR_SUB_MIN;        // 8 slots a group at the narrowest width
__global__ __launch_bounds__(FLR_SCAN_THREADS) void flr_scan2_kernel(double* __restrict__ G, int nslot, int c, int ng)
{
    extern __shared__ double sH[];                               // [group][element of the work-group]
    const int el_per = FLR_SCAN_THREADS / ng;
    const int el = threadIdx.x % el_per, j = threadIdx.x / el_per;
    const int e = blockIdx.x * el_per + el;                      // (NR * NR is a multiple of el_per: no element is left over)
    double g[FLR_SCAN_CMAX];
    double h = 0.0;
#pragma unroll
    for (int r = 0; r < FLR_SCAN_CMAX; ++r) {
        const int slot = j * c + r + 1;                          // g[j c + r]
        g[r] = (r < c && slot < nslot) ? G[(int64_t)slot * NR * NR + e] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < FLR_SCAN_CMAX; ++r)
        if (r < c) h += g[r];
    sH[j * el_per + el] = h;
    __syncthreads();
    double run = 0.0;
    for (int jj = 0; jj < j; ++jj) run += sH[jj * el_per + el];
    double tail = 0.0;
#pragma unroll
    for (int r = 0; r < FLR_SCAN_CMAX; ++r) {
        const int slot = j * c + r;                              // G_P for P = j c + r
        if (r < c && slot < nslot) G[(int64_t)slot * NR * NR + e] = run + tail;
        tail += g[r];
    }
}

// Round k of the parts' factorisation, all parts side by side.  Work-group (rb, q) belongs to part q, whose pivot block D is
// the 64 x 64 block at column c0 = part q + 64 k of L's diagonal.  EVERY work-group of the part factors D itself, in LDS
// (potf2.h; eps is added to its diagonal here: the product in front wrote eps X^T X) -- nothing passes between work-groups,
// and nobody writes D in this launch -- and then solves its own 64 rows B <- B D^-T with the substitution core of the
// factorisation's panels (solve64.h, 16 rows a wavefront):  rb == 0: the border, the 64 rows of X at the pivot's columns (and
// it keeps D's factor in Dw, which flr_diag_kernel puts in place behind the last round);  rb >= 1: rows c0 + 64 rb of the part.
// A pivot that is not positive raises *err (the sampler's numeric error word).
__global__ __launch_bounds__(256) void flr_panel_kernel(double* __restrict__ L, int64_t ldl, int64_t n, double* __restrict__ X,
                                                        double* __restrict__ Dw, int k, double eps, int* __restrict__ err, int part)
{
    const int64_t PC = part;
    const int NBLK = part / 64;
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
__global__ __launch_bounds__(256) void flr_diag_kernel(double* __restrict__ L, int64_t ldl, int64_t n, const double* __restrict__ Dw, int part)
{
    const int64_t PC = part;
    const int NBLK = part / 64;
    const int k = (int)blockIdx.x;
    const int64_t c0 = (int64_t)blockIdx.y * PC + 64 * (int64_t)k;
    if (c0 >= n) return;
    const double* in = Dw + ((int64_t)blockIdx.y * NBLK + k) * NR * NR;
    double* D = L + c0 * (ldl + 1);
    for (int idx = threadIdx.x; idx < NR * NR; idx += 256) D[(idx & (NR - 1)) + (int64_t)(idx >> 6) * ldl] = in[idx];
}

// ---- one launch per round (GPIRT_FLR_FUSE = 1) ---------------------------------------------------------------------------
// flr_round_kernel, launch k = 0 .. rounds - 1, all parts side by side: the round's panel work AND the update by the panel of
// the round before, which the launches above run as two products of their own behind every panel launch.  Tiles are 64 x 64;
// part q has nb block columns; its border is the 64 rows of X_P.  Work items of part q in launch k (blockIdx.y, in this order):
//   column items   rb = 0: the border's columns of block column k;  rb = 1 .. nb - 1 - k: tile (k + rb, k)
//   border tiles   j = k + 1 .. nb - 1
//   trailing tiles (i, j), k < j <= i < nb
//   the placer     (k >= 1) pivot factor k - 1 from Dw into tile (k - 1, k - 1), the strict upper triangle zero
// Every tile item first takes panel k - 1 off its tile -- C(i, j) -= L(i, k - 1) L(j, k - 1)^T, for the border X(:, j) -=
// X(:, k - 1) L(j, k - 1)^T -- one K = 64 product, accumulated in ascending k by the fp64 MFMA from a zero accumulator and
// applied as alpha * acc + beta * c exactly as gemm_f64.hip's 64-tile kernel does: the same bits.  In launch 0 there is no
// panel in front: the item forms its tile as eps X_i^T X_j with X_b = Xh_P V[P_b]^T computed by itself (the border items write
// X, nobody reads it).  A column item also forms the pivot block D itself, from tile (k, k) with the same update (launch 0:
// eps X_k^T X_k), factors it in LDS and solves its own 64 rows, as flr_panel_kernel does.
//
// THE PIVOT TILE HAS NO OWNER: tile (k, k) is read by the column items of launch k and written by nobody in that launch; in
// the launches before k it is an ordinary trailing tile, in launch k + 1 the placer overwrites it and nobody reads it.  Panel
// k - 1 (tiles (i, k - 1), border columns k - 1) was written by launch k - 1 and is only read in launch k; every other tile
// is read and written by its one item.  So no two work-groups of a launch touch the same memory unless both only read it,
// and the launches follow each other in stream order: no flag, no spinning, no atomics beyond the error word.  In a part's
// last round (k = nb - 1) the border item is the only reader of the pivot tile and puts the factor in place itself, behind
// the barrier that ends its reads -- nothing is left to place after the last launch.
//
// The grid is (parts, items): blockIdx.x, the part, runs fastest, so the column items of all parts -- the round's critical
// path: update, factorisation, solve -- are dispatched first and the tiles that only take the update fill in behind them.
// LDS: two 64 x 64 operand images (36 KB each; the staged pivot block and the item's own rows later lie over them) and
// potf2_64_body's panels, 76 KB: two work-groups a compute unit, as the 192 registers allow.
constexpr int FT = 72;                                // row stride (doubles) of an operand image [k][row]
constexpr size_t FLR_LDS = sizeof(double) * (2 * NR * FT + 2 * 4 * NR);
static_assert(S64_LS <= FT, "the staged pivot block and the item's own rows take the place of the operand images");

// image s[kc * FT + r] = G[r + kc * ld] of a 64 x 64 block (all loads in flight before the first LDS write)
__device__ __forceinline__ void flr_stage(double* __restrict__ s, const double* __restrict__ G, int64_t ld)
{
    const int r = threadIdx.x & 63, c = threadIdx.x >> 6;
    double v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = G[r + (int64_t)(c + 4 * q) * ld];
#pragma unroll
    for (int q = 0; q < 16; ++q) s[(c + 4 * q) * FT + r] = v[q];
}

// acc = sum_k tA[k][m] tB[k][n] over k = 0 .. 63 in gemm_f64.hip's order: 16 MFMA steps of 4, step s takes k = 4 s + (lane >> 4);
// wave (wm, wn) owns the 32 x 32 quarter, acc[tn][tm][r] belongs to m = 32 wm + 16 tm + (lane & 15), n = 32 wn + 16 tn + (lane >> 4) + 4 r
__device__ __forceinline__ void flr_mma(const double* __restrict__ tA, const double* __restrict__ tB, d4 (&acc)[2][2])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const int kq = kk * 4 + l4;
        double a[2], b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            a[t] = tA[kq * FT + wm * 32 + t * 16 + l15];
            b[t] = tB[kq * FT + wn * 32 + t * 16 + l15];
        }
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) acc[tn][tm] = __builtin_amdgcn_mfma_f64_16x16x4f64(b[tn], a[tm], acc[tn][tm], 0, 0, 0);
    }
}

// f(m, n, value) for the 16 elements of the tile this lane holds
template <class Fn>
__device__ __forceinline__ void flr_each(const d4 (&acc)[2][2], Fn f)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) f(wm * 32 + tm * 16 + l15, wn * 32 + tn * 16 + l4 + 4 * r, acc[tn][tm][r]);
}

// c <- the lane's 16 elements of C (64 x 64, leading dimension ldc; lower: only where m >= n), asked for ahead of the product
__device__ __forceinline__ void flr_load_c(d4 (&c)[2][2], const double* __restrict__ C, int64_t ldc, bool lower)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) {
                const int m = wm * 32 + tm * 16 + l15, nn = wn * 32 + tn * 16 + l4 + 4 * r;
                c[tn][tm][r] = (!lower || m >= nn) ? C[m + (int64_t)nn * ldc] : 0.0;
            }
}

// acc <- alpha * acc + beta * c, gemm_epilogue's two statements
__device__ __forceinline__ void flr_axpby(d4 (&acc)[2][2], double alpha, double beta, const d4 (&c)[2][2])
{
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) {
                double v = alpha * acc[tn][tm][r];
                v += beta * c[tn][tm][r];
                acc[tn][tm][r] = v;
            }
}

template <bool FIRST>
__global__ __launch_bounds__(256) void flr_round_kernel(double* __restrict__ L, int64_t ldl, int64_t n, double* __restrict__ X,
                                                        double* __restrict__ Dw, const double* __restrict__ Xh, const double* __restrict__ V,
                                                        int k, double eps, int* __restrict__ err, int part)
{
    const int64_t PC = part;
    const int NBLK = part / 64;
    extern __shared__ __attribute__((aligned(16))) double flr_lds[];
    __shared__ int sfail, sinfo;
    double* tA = flr_lds;                    // operand image A[k][m]
    double* tB = flr_lds + NR * FT;          // operand image B[k][n]
    double* sP = flr_lds + 2 * NR * FT;      // potf2_64_body's two panels
    double* sM = tA;                         // the pivot block, with solve64.h's stride (over A, dead by then)
    double* sT = tB;                         // the column item's own rows on their way into the solve's layout (over B)
    const int q = (int)blockIdx.x;
    const int64_t p0 = (int64_t)q * PC;
    const int nb = (int)(((n - p0) < PC ? (n - p0) : PC) / 64);         // 64-column blocks of this part
    const int rem = nb - k;
    if (rem <= 0) return;
    int it = (int)blockIdx.y;
    // the chain runs beside the side stream's chip-filling kernels (the Z prefill, a held-back draw_beta): its waves win the issue
    // arbitration, the column items (the round's critical path; potf2_64_body raises it too) ahead of the round's other tiles
    if (it < rem) __builtin_amdgcn_s_setprio(3); else __builtin_amdgcn_s_setprio(2);
    const int t = threadIdx.x;
    double* Lp = L + p0 * (ldl + 1);
    double* Xp = X + (int64_t)NR * p0;
    auto tile = [&](int i, int j) -> double* { return Lp + 64 * (int64_t)i + 64 * (int64_t)j * ldl; };
    auto xcol = [&](int j) -> double* { return Xp + (int64_t)NR * 64 * j; };
    // launch 0: X_b = Xh_P V[P_b]^T for block column b (alpha = 1, beta = 0: the accumulator itself); Xh_P stays in tA
    auto xblock = [&](int b, d4 (&acc)[2][2]) {
        flr_stage(tB, V + p0 + 64 * (int64_t)b, n);
        __syncthreads();
        flr_mma(tA, tB, acc);
        __syncthreads();
    };
    auto image = [&](double* s, const d4 (&acc)[2][2]) { flr_each(acc, [&](int m, int nn, double v) { s[m * FT + nn] = v; }); };
    if (FIRST) flr_stage(tA, Xh + (int64_t)q * NR * NR, NR);

    if (it >= rem) {
        it -= rem;
        d4 acc[2][2];
        if (it < rem - 1) {
            // a border tile: columns of block column j of X
            const int j = k + 1 + it;
            if (FIRST) {
                xblock(j, acc);
            } else {
                d4 c[2][2];
                flr_stage(tA, xcol(k - 1), NR);
                flr_stage(tB, tile(j, k - 1), ldl);
                flr_load_c(c, xcol(j), NR, false);
                __syncthreads();
                flr_mma(tA, tB, acc);
                flr_axpby(acc, -1.0, 1.0, c);
            }
            double* C = xcol(j);
            flr_each(acc, [&](int m, int nn, double v) { C[m + (int64_t)NR * nn] = v; });
            return;
        }
        it -= rem - 1;
        if (it < rem * (rem - 1) / 2) {
            // a trailing tile (i, j), k < j <= i
            int a = 0;
            while ((a + 1) * (a + 2) / 2 <= it) ++a;
            const int i = k + 1 + a, j = k + 1 + (it - a * (a + 1) / 2);
            double* C = tile(i, j);
            if (FIRST) {
                d4 xi[2][2];
                xblock(i, xi);
                if (i != j) {
                    d4 xj[2][2];
                    xblock(j, xj);
                    image(tB, xj);
                } else {
                    image(tB, xi);
                }
                image(tA, xi);
                __syncthreads();
                flr_mma(tA, tB, acc);
                flr_each(acc, [&](int m, int nn, double v) { if (i != j || m >= nn) C[m + (int64_t)nn * ldl] = eps * v; });
            } else {
                d4 c[2][2];
                flr_stage(tA, tile(i, k - 1), ldl);
                flr_stage(tB, tile(j, k - 1), ldl);
                flr_load_c(c, C, ldl, i == j);
                __syncthreads();
                flr_mma(tA, tB, acc);
                flr_axpby(acc, -1.0, 1.0, c);
                flr_each(acc, [&](int m, int nn, double v) { if (i != j || m >= nn) C[m + (int64_t)nn * ldl] = v; });
            }
            return;
        }
        it -= rem * (rem - 1) / 2;
        if (!FIRST && it == 0) {
            // the placer: pivot factor k - 1 into L's diagonal
            const double* in = Dw + ((int64_t)q * NBLK + (k - 1)) * NR * NR;
            double* D = tile(k - 1, k - 1);
            for (int idx = t; idx < NR * NR; idx += 256) D[(idx & (NR - 1)) + (int64_t)(idx >> 6) * ldl] = in[idx];
        }
        return;
    }

    // ---- a column item: its own 64 rows B, the pivot block D, B <- B D^-T
    const int rb = it;
    const int lane = t & 63, wave = t >> 6;
    const int i = lane & 15, g = lane >> 4;
    double* B = rb == 0 ? xcol(k) : tile(k + rb, k);
    const int64_t ldb = rb == 0 ? NR : ldl;
    d4 own[2][2], piv[2][2];
    if (FIRST) {
        if (rb == 0) {
            xblock(0, own);                              // X_0: the border's own rows
            image(tB, own);
            __syncthreads();
            flr_mma(tB, tB, piv);
        } else {
            d4 xi[2][2], x0[2][2];
            xblock(rb, xi);
            xblock(0, x0);
            image(tA, xi);
            image(tB, x0);
            __syncthreads();
            flr_mma(tA, tB, own);
            flr_mma(tB, tB, piv);
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) own[a][b][r] = eps * own[a][b][r];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) piv[a][b][r] = eps * piv[a][b][r];
    } else {
        flr_stage(tA, rb == 0 ? xcol(k - 1) : tile(k + rb, k - 1), ldb);
        flr_stage(tB, tile(k, k - 1), ldl);
        d4 cown[2][2], cpiv[2][2];
        flr_load_c(cown, B, ldb, false);
        flr_load_c(cpiv, tile(k, k), ldl, true);
        __syncthreads();
        flr_mma(tA, tB, own);
        flr_mma(tB, tB, piv);
        flr_axpby(own, -1.0, 1.0, cown);
        flr_axpby(piv, -1.0, 1.0, cpiv);
    }
    __syncthreads();                                     // (every wave has read the images: D and the rows go over them)
    flr_each(own, [&](int m, int nn, double v) { sT[nn * S64_LS + m] = v; });
    flr_each(piv, [&](int m, int nn, double v) { sM[nn * S64_LS + m] = m >= nn ? v + (m == nn ? eps : 0.0) : 0.0; });
    if (t == 0) sinfo = 0;
    __syncthreads();
    d4 Xv[4];
#pragma unroll
    for (int J = 0; J < 4; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) Xv[J][r] = sT[(16 * J + 4 * g + r) * S64_LS + wave * 16 + i];
    potf2_64_body(sM, S64_LS, NR, 0, &sinfo, sP, &sfail);
    if (t == 0 && sfail != 0x7fffffff && err) atomicCAS(err, 0, (int)GPIRT_E_NUMERIC);
    if (rb == 0) {
        double* out = Dw + ((int64_t)q * NBLK + k) * NR * NR;
        double* D = tile(k, k);
        const bool last = (k == nb - 1);                 // the part's last round: this item is the pivot tile's only reader
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) {
            const int idx = t + 256 * qq;
            const double v = sM[(idx >> 6) * S64_LS + (idx & (NR - 1))];
            out[idx] = v;
            if (last) D[(idx & (NR - 1)) + (int64_t)(idx >> 6) * ldl] = v;
        }
    }
    __syncthreads();
    invert_diag16(sM);
    solve64_lower_inv(Xv, sM);
    double* Bl = B + wave * 16 + i;                      // this lane's row
#pragma unroll
    for (int J = 0; J < 4; ++J)
#pragma unroll
        for (int r = 0; r < 4; ++r) Bl[(16 * J + 4 * g + r) * ldb] = Xv[J][r];
}

}  // namespace

int64_t factor_lr_parts(int64_t n, int part) { const int64_t PC = part ? part : NU_LR_PART; return (n + PC - 1) / PC; }

// The diagonal parts into a.L (lower triangles; the strict upper triangle inside a part is zero, nothing below the parts is
// written) and the node rows into a.Bt.  V: n x 64 (ld n), rewritten with the basis at theta; G, Xh: factor_lr_parts(n, part)
// x 64 x 64; X: 64 x n; D: n / 64 x 64 x 64.  n a multiple of 64; the last part may be shorter than a.part.
// h (may be null): the handle whose profiler books the syrk-lower launches -- S_PP under class 1, the in-part updates
// under class 2 (the fused rounds: round 0 under class 1, the rounds behind it under class 2, each with the flops and bytes
// of the syrk-lower it contains) -- and whose GPIRT_FLR_FUSE picks the schedule (null: the fused rounds).
int launch_factor_lr(gpirt_handle_t h, hipStream_t stream, const FactorLrArgs& a)
{
    const int64_t n = a.n, ldl = a.ldl;
    if (n <= 0) return 0;
    if ((n % 64) != 0) { set_error("factor_lr: n must be a multiple of 64"); return GPIRT_E_ARG; }
    const int part = a.part ? a.part : NU_LR_PART;
    if (part != 64 && part != 128 && part != 256 && part != 512) { set_error("factor_lr: the part width must be 64, 128, 256 or 512 (got %d)", a.part); return GPIRT_E_ARG; }
    const int64_t PC = part;
    const int NBLK = part / 64;
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
    const bool fuse = !h || h->cfg.flr_fuse != 2;
    if (parts > 1)
        GP_TRY(launch_gemm_batched(stream, true, false, TRI_NONE, NR, NR, PC, 1.0, a.V, n, PC, a.V, n, PC, 0.0, a.G + sG, NR, sG, parts - 1));
    const int rounds = full > 0 ? NBLK : (int)(rem / 64);
    // the prefix over the Grams: parts narrower than 512 take the two-level order of flr_scan2_kernel in both schedules
    const bool narrow = part < NU_LR_PART;
    if (narrow) {                                         // (a single part too: slot 0 <- 0, which nobody else writes)
        const int c = NU_LR_PART / part;
        const int64_t groups = (parts + c - 1) / c;
        if (groups > FLR_SCAN_THREADS) { set_error("factor_lr: n = %lld is too large for parts %d wide", (long long)n, part); return GPIRT_E_ARG; }
        int ng = 1;
        while (ng < groups) ng *= 2;
        const int el_per = FLR_SCAN_THREADS / ng;
        hipLaunchKernelGGL(flr_scan2_kernel, dim3((unsigned)(NR * NR / el_per)), dim3(FLR_SCAN_THREADS), sizeof(double) * FLR_SCAN_THREADS, stream, a.G, parts, c, ng);
        GP_HIP(hipGetLastError());
    }
    if (fuse) {
        // One launch per round (flr_round_kernel): the prefix over the Grams rides in the X-hat kernel, X_P, eps X_P^T X_P and
        // each round's update in the round kernels, the diagonal is placed as the rounds go.  The same sums in the same order.
        // (behind flr_scan2_kernel the slots already hold the prefix: the same kernel without its own sum)
        GP_TRY(launch_fstar_free_xhat(stream, a.G, a.F, a.eps, a.Xh, parts, a.err, !narrow, nullptr, narrow));
        GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(flr_round_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FLR_LDS));
        GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(flr_round_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FLR_LDS));
        for (int k = 0; k < rounds; ++k) {
            const int r0 = rounds - k;                                  // blocks left in the longest part (the first)
            const unsigned items = (unsigned)(r0 + (r0 - 1) + r0 * (r0 - 1) / 2 + (k > 0 ? 1 : 0));
            // booked as the syrk-lower the launch contains: S_PP (class 1) in round 0, the update by panel k - 1 (class 2) behind it
            double flops = 0.0, bytes = 0.0;
            for (int q = 0; q < parts; ++q) {
                const int64_t M = (q < full ? PC : rem) - 64 * (int64_t)k;
                if (M <= 0) continue;
                const double tri = 0.5 * (double)M * (double)(M + 1);
                flops += 2.0 * NR * tri;
                bytes += 8.0 * ((k > 0 ? 2.0 : 1.0) * tri + (double)(M * NR));
            }
            ProfPair pp;
            if (h) GP_TRY(prof_pair_begin(h, stream, pp));
            if (k == 0) hipLaunchKernelGGL(flr_round_kernel<true>, dim3((unsigned)parts, items), dim3(256), FLR_LDS, stream, a.L, ldl, n, a.X, a.D, a.Xh, a.V, k, a.eps, a.err, part);
            else        hipLaunchKernelGGL(flr_round_kernel<false>, dim3((unsigned)parts, items), dim3(256), FLR_LDS, stream, a.L, ldl, n, a.X, a.D, a.Xh, a.V, k, a.eps, a.err, part);
            GP_HIP(hipGetLastError());
            if (h) GP_TRY(prof_pair_end(h, stream, pp, k == 0 ? 1 : 2, flops, bytes));
        }
        // Bt[:, P] = eps Xh_P^T (X_P L_PP^-T): the batched product of the launches below (its sums, its bits)
        if (full > 0) GP_TRY(launch_gemm_batched(stream, true, false, TRI_NONE, NR, PC, NR, a.eps, a.Xh, NR, sG, a.X, NR, sX, 0.0, a.Bt, ldl, PC * ldl, (int)full));
        if (rem > 0) GP_TRY(launch_gemm_batched(stream, true, false, TRI_NONE, NR, rem, NR, a.eps, a.Xh + full * sG, NR, 0, a.X + full * sX, NR, 0, 0.0,
                                                a.Bt + full * PC * ldl, ldl, 0, 1));
        return 0;
    }
    // GPIRT_FLR_FUSE = 2: a panel launch and two product launches per round (library version 131)
    if (!narrow) {
        hipLaunchKernelGGL(flr_scan_kernel, dim3((unsigned)((NR * NR + 255) / 256)), dim3(256), 0, stream, a.G, parts);
        GP_HIP(hipGetLastError());
    }
    GP_TRY(launch_fstar_free_xhat(stream, a.G, a.F, a.eps, a.Xh, parts, a.err));
    // X_P = Xh_P V[P]^T, then eps X_P^T X_P into the parts of L (flr_panel_kernel adds eps I)
    if (full > 0) GP_TRY(launch_gemm_batched(stream, false, true, TRI_NONE, NR, PC, NR, 1.0, a.Xh, NR, sG, a.V, n, PC, 0.0, a.X, NR, sX, (int)full));
    if (rem > 0) GP_TRY(launch_gemm_batched(stream, false, true, TRI_NONE, NR, rem, NR, 1.0, a.Xh + full * sG, NR, 0, a.V + full * PC, n, 0, 0.0, a.X + full * sX, NR, 0, 1));
    GP_TRY(syrk(1, true, PC, a.eps, a.X, NR, sX, 0.0, a.L, (int)full));
    GP_TRY(syrk(1, true, rem, a.eps, a.X + full * sX, NR, 0, 0.0, a.L + full * sL, 1));
    // the parts' factorisation with X_P as the border: a round factors the pivot blocks and solves the rows below them, then
    // takes the new columns' products off what lies to their right (the part's trailing triangle, the border's columns)
    for (int k = 0; k < rounds; ++k) {
        hipLaunchKernelGGL(flr_panel_kernel, dim3((unsigned)(rounds - k), (unsigned)parts), dim3(256), 0, stream, a.L, ldl, n, a.X, a.D, k, a.eps, a.err, part);
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
    hipLaunchKernelGGL(flr_diag_kernel, dim3((unsigned)rounds, (unsigned)parts), dim3(256), 0, stream, a.L, ldl, n, a.D, part);
    GP_HIP(hipGetLastError());
    // Bt[:, P] = eps Xh_P^T (X_P L_PP^-T)
    if (full > 0) GP_TRY(launch_gemm_batched(stream, true, false, TRI_NONE, NR, PC, NR, a.eps, a.Xh, NR, sG, a.X, NR, sX, 0.0, a.Bt, ldl, PC * ldl, (int)full));
    if (rem > 0) GP_TRY(launch_gemm_batched(stream, true, false, TRI_NONE, NR, rem, NR, a.eps, a.Xh + full * sG, NR, 0, a.X + full * sX, NR, 0, 0.0,
                                            a.Bt + full * PC * ldl, ldl, 0, 1));
    return 0;
}

}  // namespace gpirt
