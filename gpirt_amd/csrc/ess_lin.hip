// ess_lin.hip -- the elliptical slice kernel of the 512 x 16 class (2048 < n <= 8192, item RNG) with y packed and mu recomputed
// (GPIRT_ESS_PACK=1), and the kernel that packs y.  A file of its own for its compiler option (Makefile):
// with machine LICM on, the coefficients of exp, log, cos, sin and ll_term_fast are hoisted out of the slice loop into vector
// register pairs that stay live through every pass -- 182 registers, or 116 bytes of scratch under a 128-register limit; with it
// off the kernel takes 111 and two work-groups share a CU.
#include "common.h"
#include "kernels.h"
#include "ll_fast.h"

namespace gpirt {

namespace {

template <bool FAST>
__device__ __forceinline__ double ll_t(double a) { return FAST ? ll_term_fast(a) : ll_term(a); }

// ess_kernel_reg<16, 512> reads f, nu, mu and y and holds all four, 237 registers: one work-group per CU, whose loads and
// passes do not overlap.  Here the lane holds F and V alone.  y is one word per (item, lane), built once (ess_pack_kernel): bit e
// = row tid + 512 e is observed, bit 16 + e = it is negative.  mu is formed again in every pass from theta (in LDS, loaded
// once per work-group) and the item's two coefficients, M = b0 + theta b1 as one multiply and one add -- the bits draw_beta
// and linear_mean_kernel store (the build is -ffp-contract=off).  Then (F c + V s) + M, the sign by an exclusive or on bit 63
// (y is +1 or -1: the product is exact), the term of a row that does not count cleared to +0.0 by an and (the sums start at
// +0.0 and no partial sum is -0.0, so adding +0.0 is skipping the row: stages.hip, draw_beta_reg_kernel).  Same rows per
// lane, same order of e, same block_sum_512: every sum, hence every decision, k and f', is ess_kernel_reg's bit for bit.
// A work-group strides over items blockIdx.x, blockIdx.x + gridDim.x, ...
constexpr int EL_NTH = 512, EL_EPT = 16, EL_ROWS = EL_NTH * EL_EPT;
constexpr size_t EL_LDS = sizeof(double) * (size_t)(16 + EL_ROWS);      // the reduction's scratch, then theta
constexpr int EL_MAX_TRIALS = 100000;             // rng_ess.hip's ESS_MAX_TRIALS

__global__ __launch_bounds__(256) void ess_pack_kernel(const double* __restrict__ y, int64_t n, int64_t m, uint32_t* __restrict__ out)
{
    const int64_t total = m * EL_NTH;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = g / EL_NTH, t = g - j * EL_NTH;
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < EL_EPT; ++e) {
            const int64_t i = t + EL_NTH * e;
            if (i < n) {
                const double yy = y[j * n + i];
                w |= (uint32_t)(yy == yy) << e;
                w |= (uint32_t)(yy < 0.0) << (16 + e);
            }
        }
        out[g] = w;
    }
}

// a value every lane holds alike, moved to scalar registers (the vector registers go to the rows)
__device__ __forceinline__ double el_uniform(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
// x with its sign flipped where row e is negative / x where row e counts, +0.0 where it does not
__device__ __forceinline__ double el_flip(double x, uint32_t pk, int e)
{
    return __hiloint2double(__double2hiint(x) ^ (int)((pk << (15 - e)) & 0x80000000u), __double2loint(x));
}
__device__ __forceinline__ double el_keep(double x, uint32_t pk, int e)
{
    const int k = -(int)((pk >> e) & 1u);
    return __hiloint2double(__double2hiint(x) & k, __double2loint(x) & k);
}
// EL_COEF: the coefficients and the mask word of one pass behind an empty asm, so that every pass forms M and its arguments anew
// (nothing of a screened pass is kept alive for the full-precision pass that rarely follows)
#define EL_COEF(c_, s_) double cc = (c_), ss = (s_), b0 = be0, b1 = be1; uint32_t pk = ypk; \
    asm volatile("" : "+s"(cc), "+s"(ss), "+s"(b0), "+s"(b1), "+v"(pk))
#define EL_M(e) (b0 + th[EL_NTH * (e)] * b1)
#define EL_ARG0(e) el_flip(F[e] + EL_M(e), pk, e)
#define EL_ARGP(e) el_flip((F[e] * cc + V[e] * ss) + EL_M(e), pk, e)
// acc <- this lane's sum of fn over the current state (ARG0) or the trial point (ARGP)
#define EL_PASS0(fn, every)                                                                     \
    {                                                                                           \
        EL_COEF(0.0, 0.0);                                                                      \
        acc = 0.0;                                                                              \
        _Pragma("unroll") for (int e = 0; e < EL_EPT; ++e) {                                    \
            acc += el_keep(fn(EL_ARG0(e)), pk, e);                                              \
            if ((e & (every - 1)) == every - 1) __builtin_amdgcn_sched_barrier(0);              \
        }                                                                                       \
    }
#define EL_PASSP(fn, track, every)                                                              \
    {                                                                                           \
        EL_COEF(c, s);                                                                          \
        acc = 0.0;                                                                              \
        _Pragma("unroll") for (int e = 0; e < EL_EPT; ++e) {                                    \
            const double arg = EL_ARGP(e);                                                      \
            acc += el_keep(fn(arg), pk, e);                                                     \
            if (track) overflows |= (int)(arg < -709.0) & (int)(pk >> e);                       \
            if ((e & (every - 1)) == every - 1) __builtin_amdgcn_sched_barrier(0);              \
        }                                                                                       \
    }

template <bool FAST>
__global__ __launch_bounds__(EL_NTH) __attribute__((amdgpu_waves_per_eu(FAST ? 4 : 2, FAST ? 4 : 2))) void ess_kernel_lin(EssArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double el_lds[];
    double* red = el_lds;
    const int tid = (int)threadIdx.x;
    const int n = (int)a.n;
    for (int i = tid; i < EL_ROWS; i += EL_NTH) el_lds[16 + i] = i < n ? a.theta[i] : 0.0;
    __syncthreads();
    const double* th = el_lds + 16 + tid;
    const double band = el_uniform(LL_SCREEN_ERR * (double)n);
    const bool lazy = a.screen && FAST;
    for (int64_t j = blockIdx.x; j < a.m; j += gridDim.x) {
        double* fj = a.f + j * a.n;
        const double* nj = a.nu + j * a.n;
        const uint32_t item = a.item0 + (uint32_t)j;
        const uint32_t ypk = a.ypk[j * EL_NTH + tid];
        const double be0 = el_uniform(a.beta[0 + 2 * j]), be1 = el_uniform(a.beta[1 + 2 * j]);
        // the slice level's uniform and the first angle, in front of the loads: log's coefficients are dead before the rows arrive
        uint32_t uidx = 0;
        const double u = item_uniform(a.seed, a.iter, GPIRT_ST_F_ESS, item, uidx++);
        const double log_u = el_uniform(log(u));
        double eps_min = 0.0, eps_max = GP_2PI;
        double eps = el_uniform(eps_min + (eps_max - eps_min) * item_uniform(a.seed, a.iter, GPIRT_ST_F_ESS, item, uidx++));
        eps_min = el_uniform(eps - GP_2PI);                                    // :36
        __builtin_amdgcn_sched_barrier(0);
        double F[EL_EPT], V[EL_EPT];
        {
            // (a row past the end reads the last one: its terms are cleared and it is never stored.  The rows' indices are formed
            // anew for every item, not carried through the loop: sixteen addresses per array were 260 bytes of scratch)
            unsigned t2 = (unsigned)tid;
            asm volatile("" : "+v"(t2));
#pragma unroll
            for (int e = 0; e < EL_EPT; ++e) {
                const unsigned i = t2 + EL_NTH * e, ic = i < (unsigned)n ? i : (unsigned)n - 1u;
                F[e] = fj[ic];
                V[e] = nj[ic];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        double acc;
        double ll0 = 0.0, lls0 = 0.0;
        bool have_ll0 = false;
        if (lazy) {
            EL_PASS0(ll_term_screen, 4);
            lls0 = el_uniform(-block_sum_512(acc, red));
        } else {
            EL_PASS0(ll_t<FAST>, 1);
            ll0 = el_uniform(-block_sum_512(acc, red));
            have_ll0 = true;
        }
        int k = 0;
        bool bad = false;
        double c, s;
        for (;;) {
            c = el_uniform(cos(eps));
            s = el_uniform(sin(eps));
            int verdict = 0;                                                   // +1 accept, -1 reject, 0 undecided
            if (a.screen) {
                int overflows = 0;
                EL_PASSP(ll_term_screen, !FAST, 4);
                const double lls = el_uniform(-block_sum_512(acc, red));
                if (!have_ll0) {
                    const double d = lls - lls0;
                    if (d - 2.0 * band > log_u) verdict = 1;
                    else if (d + 2.0 * band < log_u) verdict = -1;
                } else {
                    const double log_y = ll0 + log_u;
                    if (lls - band > log_y) verdict = 1;
                    else if (lls + band < log_y) verdict = -1;
                }
                if (!FAST) { if (__syncthreads_or(overflows & 1)) verdict = 0; }
            }
            if (verdict == 0) {
                if (!have_ll0) {
                    EL_PASS0(ll_t<FAST>, 1);
                    ll0 = el_uniform(-block_sum_512(acc, red));
                    have_ll0 = true;
                }
                const double log_y = ll0 + log_u;                              // draw-f.cpp:28-29
                int overflows = 0;
                EL_PASSP(ll_t<FAST>, false, 1);                                  // :43
                (void)overflows;
                const double llp = el_uniform(-block_sum_512(acc, red));
                if (llp > log_y) verdict = 1;                                  // :45-47
                else if (llp != llp || ll0 != ll0) { bad = true; break; }
            }
            if (verdict > 0) break;
            if (eps < 0.0) eps_min = eps; else eps_max = eps;                  // :50-55
            if (eps_min == eps_max) eps = eps_min;
            else eps = el_uniform(eps_min + (eps_max - eps_min) * item_uniform(a.seed, a.iter, GPIRT_ST_F_ESS, item, uidx++));
            ++k;
            if (k >= EL_MAX_TRIALS) { bad = true; break; }
        }
        {
            unsigned t2 = (unsigned)tid;
            asm volatile("" : "+v"(t2));
#pragma unroll
            for (int e = 0; e < EL_EPT; ++e) {
                const unsigned i = t2 + EL_NTH * e;
                if (i < (unsigned)n) fj[i] = F[e] * c + V[e] * s;
            }
        }
        if (tid == 0) {
            if (a.k_out) a.k_out[j] = k;
            if (bad && a.err) atomicCAS(a.err, 0, (int)GPIRT_E_NUMERIC);
        }
    }
}
#undef EL_COEF
#undef EL_M
#undef EL_ARG0
#undef EL_ARGP
#undef EL_PASS0
#undef EL_PASSP

}  // namespace

int launch_ess_lin(hipStream_t stream, const EssArgs& a)
{
    if (a.m <= 0) return 0;
    if (a.U || !ess_pack_eligible(a.n) || !a.ypk || !a.theta || !a.beta) { set_error("launch_ess_lin: the packed slice kernel takes the item RNG and 2048 < n <= 8192"); return GPIRT_E_ARG; }
    const bool fast = a.ll_exact != 1;
    const unsigned grid = a.grid > 0 && a.grid < a.m ? (unsigned)a.grid : (unsigned)a.m;
    // (dynamic LDS: theta at n = 8192 is 64 KB, above the static limit; two work-groups share a CU's 160 KB)
    void (*kern)(EssArgs) = fast ? ess_kernel_lin<true> : ess_kernel_lin<false>;
    GP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)EL_LDS));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(EL_NTH), EL_LDS, stream, a);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_ess_pack(hipStream_t stream, const double* y, int64_t n, int64_t m, uint32_t* out)
{
    if (m <= 0) return 0;
    int64_t blocks = (m * EL_NTH + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(ess_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, y, n, m, out);
    GP_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpirt
