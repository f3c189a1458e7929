// carry.hip -- the consistent step's carry stage (gpirt_sampler_carry_f, gpirt_sampler_step_consistent; sampler.hip) and the
// prior check's reduction (gpirt_sampler_prior_quad).
//
// WHAT THE CARRY IS.  The reference's iteration moves theta and keeps f (quirk Q3 of SURVEY.md): after draw_theta, f[i, :] is
// still the GP's value at respondent i's OLD position, while mu, L and everything built on them belong to the new one.  The
// carry runs behind draw_theta (theta_finish or theta_commit) and in front of draw_beta and makes (theta, f) consistent:
//   - given the curve on the grid, theta's draw is the reference's own: nothing of draw_theta changes;
//   - f then becomes that curve at the new theta plus the model's nugget: with k_i = grid_index(theta_i) (kernels.h),
//       g = fstar[k_i, j] - mu_star[k_i, j]     one fp64 subtraction; mu_star is the one draw_fstar added, still in place
//       f_ij = g                                 nugget = 0
//       f_ij = g + sd_j z_ij                     nugget = 1: one multiplication and one addition, no FMA
//     sd_j = a_j 0.031622776601683794 (the correctly rounded sqrt(0.001), the jitter's square root; a_j the item's amplitude,
//     1.0 exactly when amplitudes are off), z_ij = qnorm_as241(item_uniform(seed, iter + 1, GPIRT_ST_CARRY, item0 + j, i)).
//     Nothing else draws from GPIRT_ST_CARRY and the carry draws from nothing else: every existing stage keeps its uniforms,
//     and the values are keyed by the GLOBAL item, so an item shard carries its columns to the same bits.
// It is exact up to two named approximations:
//   (1) f* is the reference's conditional mean plus INDEPENDENT noise of sd s = 1 - sqrt(q), about 1e-6 (quirk Q2), not a joint
//       draw over the grid;
//   (2) the nugget is redrawn from its prior, not tilted by the likelihood; its sd is 0.03 logits.
// The next draw_f is an exact update of f | theta, y, so neither accumulates.
// WHAT IT IS NOT: a change of the reference's chain.  gpirt_sampler_step, gpirt_run and gpirt_mcmc* never call it.
//
// All respondents are carried, moved or not: one that stayed gets the predictive value at its own point and a fresh nugget.  A
// row with k_i < 0 (NaN, a starting value off the grid) keeps its f byte for byte and is counted in off_grid.  A non-finite
// fstar cell is carried as draw_fstar left it and counted in nonfinite.  One writer per cell; the two counters are integer
// atomics (one per work-group that has something to add): two runs give a byte-identical f.
//
// SHAPE.  f is column-major n x m: a thread owns ONE row i of a 256-row tile and walks CARRY_COLS columns of it, so every store
// instruction of a wave is 512 contiguous bytes and k_i, the row's only dependence on theta, is computed once and kept in a
// register for all the thread's columns.  The two gathered loads hit one 8 KB column of fstar / mu_star each (cache-resident).
// The cost is the Philox block and the AS241 evaluation per value, fp64 VALU work of a few hundred instructions against 8 bytes
// stored: VALU-bound by a wide margin (MI355X: 8.4e6 values at 8192 x 1024 are 67 MB, 11 us at 6 TB/s).  Such a kernel needs
// enough independent work per SIMD to fill its issue slots, not waves to hide memory: 256 threads (one wave per SIMD), no LDS
// but two counter words.  The compiler keeps AS241's fp64 coefficients in registers (143 VGPRs with the column loop unrolled
// by two, 126 without; item_fill_kernel: 94), so 3 work-groups share a CU, each wave with two columns' independent Philox /
// Horner chains in flight -- with fp64 VALU instructions at 4 cycles of issue per wave that is issue-bound, and a fourth wave
// per SIMD (no unrolling) would add nothing an idle issue slot is waiting for.  CARRY_COLS = 8 gives 32 x 128 = 4096
// work-groups at the metric size, five rounds of the chip.  Unlike item_fill_kernel, the yardstick it is measured against
// (tools/carry_cost.py), no 64-bit division by n finds a value's item.
#include "common.h"
#include "kernels.h"

namespace gpirt {

namespace {

constexpr int CARRY_THREADS = 256;
constexpr int CARRY_COLS = 8;
constexpr double CARRY_SQRT_JITTER = 0.031622776601683794;      // sqrt(GPIRT_JITTER), correctly rounded

__global__ __launch_bounds__(CARRY_THREADS) void carry_f_kernel(CarryArgs a)
{
    __shared__ unsigned int s_cnt[2];                  // this work-group's off-grid rows / non-finite cells
    const int tid = threadIdx.x;
    if (tid < 2) s_cnt[tid] = 0u;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * CARRY_THREADS + tid;
    const int64_t j0 = (int64_t)blockIdx.y * CARRY_COLS;
    const int64_t j1 = j0 + CARRY_COLS < a.m ? j0 + CARRY_COLS : a.m;
    if (i < a.n) {
        const int k = grid_index(a.theta[i]);
        if (k < 0) {
            if (blockIdx.y == 0) atomicAdd(&s_cnt[0], 1u);                    // (a row is counted once, by its first column tile)
        } else {
            unsigned int bad = 0u;
#pragma unroll 2
            for (int64_t j = j0; j < j1; ++j) {
                const double fs = a.fstar[k + j * a.N];
                const double g = __dsub_rn(fs, a.mu_star[k + j * a.N]);
                if (!(fabs(fs) <= 1.79769313486231570815e308)) ++bad;        // NaN or infinite
                double v = g;
                if (a.nugget) {
                    const double sd = a.amp ? __dmul_rn(a.amp[j], CARRY_SQRT_JITTER) : CARRY_SQRT_JITTER;
                    const double z = qnorm_as241(item_uniform(a.seed, a.iter, GPIRT_ST_CARRY, a.item0 + (uint32_t)j, (uint32_t)i));
                    v = __dadd_rn(g, __dmul_rn(sd, z));
                }
                a.f[i + j * a.n] = v;
            }
            if (bad) atomicAdd(&s_cnt[1], bad);
        }
    }
    __syncthreads();
    // counters (CarryArgs): the life's pair, this call's pair (zero when the launch starts), and the pair of the NEXT call, which
    // nothing else touches in this launch and one thread zeroes -- so a call is one launch, with no memset in front of it
    if (tid < 2 && s_cnt[tid]) {
        atomicAdd(a.counters + tid, (unsigned long long)s_cnt[tid]);
        atomicAdd(a.counters + 2 + 2 * a.slot + tid, (unsigned long long)s_cnt[tid]);
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < 2) a.counters[2 + 2 * (1 - a.slot) + tid] = 0ull;
}

// One work-group per item j, ell_quad_kernel's order: q[j] = sum_i nu_ij^2 -- thread t takes its rows t, t + 256, ... ascending,
// four loads in flight, added in row order, then the fixed LDS tree.  One writer per value, no atomics.
__global__ __launch_bounds__(CARRY_THREADS) void prior_quad_kernel(const double* __restrict__ nu, int64_t n, double* __restrict__ q)
{
    __shared__ double sd[CARRY_THREADS];
    const int tid = threadIdx.x;
    const double* aj = nu + (int64_t)blockIdx.x * n;
    double acc = 0.0;
    int64_t i = tid;
    for (; i + 3 * CARRY_THREADS < n; i += 4 * CARRY_THREADS) {
        const double a0 = aj[i], a1 = aj[i + CARRY_THREADS], a2 = aj[i + 2 * CARRY_THREADS], a3 = aj[i + 3 * CARRY_THREADS];
        acc += a0 * a0; acc += a1 * a1; acc += a2 * a2; acc += a3 * a3;
    }
    for (; i < n; i += CARRY_THREADS) acc += aj[i] * aj[i];
    sd[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s = CARRY_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) sd[tid] += sd[tid + s];
        __syncthreads();
    }
    if (tid == 0) q[blockIdx.x] = sd[0];
}

}  // namespace

int launch_carry_f(hipStream_t st, const CarryArgs& a)
{
    if (a.n <= 0 || a.m <= 0) return 0;
    const dim3 grid((unsigned)((a.n + CARRY_THREADS - 1) / CARRY_THREADS), (unsigned)((a.m + CARRY_COLS - 1) / CARRY_COLS));
    hipLaunchKernelGGL(carry_f_kernel, grid, dim3(CARRY_THREADS), 0, st, a);
    GP_HIP(hipGetLastError());
    return 0;
}

int launch_prior_quad(hipStream_t st, const double* nu, int64_t n, int64_t m, double* q)
{
    if (m <= 0) return 0;
    hipLaunchKernelGGL(prior_quad_kernel, dim3((unsigned)m), dim3(CARRY_THREADS), 0, st, nu, n, q);
    GP_HIP(hipGetLastError());
    return 0;
}

}  // namespace gpirt
