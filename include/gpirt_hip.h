/*
 * gpirt_hip.h -- C ABI of libgpirt_hip.so: the MI355X (gfx950) implementation of the per-iteration
 * GP linear algebra of duckmayr/gpirt's gpirtMCMC(), behind the reference's own boundary.
 *
 * Boundary being replaced (paths relative to the upstream repository):
 *   R/RcppExports.R:4-6      .Call(`_gpirt_gpirtMCMC`, y, theta, S, B, prior_means, prior_sds, steps)
 *   src/RcppExports.cpp:16-30  SEXP _gpirt_gpirtMCMC(SEXP x 7)  (Rcpp glue, RNGScope, BEGIN/END_RCPP)
 *   src/gpirtMCMC.cpp:5-9    Rcpp::List gpirtMCMC(const arma::mat& y, arma::vec theta, int, int, ...)
 *   src/gpirt.h:4-28         internal prototypes K / draw_f / draw_fstar / draw_theta / draw_beta / ll_bar
 *
 * Conventions: plain pointers and sizes only; every matrix is column-major fp64 (Armadillo / R
 * layout); y holds -1 / +1 / NaN; int64_t sizes; `void* stream` is a hipStream_t (NULL = the
 * handle's stream).  Pointers named d_* are DEVICE pointers, h_* are HOST pointers.
 * Every function returns 0 on success; >0 = LAPACK-style potrf info (order of the leading minor
 * that is not positive definite -- what makes arma::chol throw "decomposition failed",
 * src/gpirtMCMC.cpp:17); <0 = GPIRT_E_* .  gpirt_last_error() describes the last failure of the
 * calling thread.  No function throws across the boundary.
 *
 * The library has NO CPU fallback: without a usable gfx950 device every compute entry fails with
 * GPIRT_E_NODEVICE.
 */
#ifndef GPIRT_HIP_H
#define GPIRT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPIRT_NGRID 1001           /* theta_star = regspace(-5, 0.01, 5): src/gpirtMCMC.cpp:35 */
#define GPIRT_JITTER 0.001         /* S.diag() += 0.001: src/gpirtMCMC.cpp:16,77,96 */

enum {
    GPIRT_OK          = 0,
    GPIRT_E_ARG       = -1,   /* bad argument (NULL pointer, negative size, ...) */
    GPIRT_E_HIP       = -2,   /* a HIP runtime call failed */
    GPIRT_E_NODEVICE  = -3,   /* no gfx950 device visible */
    GPIRT_E_ALLOC     = -4,   /* device or host allocation failed */
    GPIRT_E_RNG       = -5,   /* R-stream replay ran out of pre-generated uniforms */
    GPIRT_E_INTERRUPT = -6,   /* the tick callback asked to stop */
    GPIRT_E_NUMERIC   = -7    /* non-finite state (e.g. ESS did not terminate) */
};

/* RNG contracts:
 *  GPIRT_RNG_RSTREAM  exact replay of R's Mersenne-Twister/inversion stream in the reference's
 *                     consumption order (item-sequential draw_f);
 *  GPIRT_RNG_ITEM     counter-based Philox4x32-10 sub-streams keyed by (seed, iteration, stage,
 *                     item): same algorithm, items independent, batched trmm legal. */
enum { GPIRT_RNG_RSTREAM = 0, GPIRT_RNG_ITEM = 1 };

/* stage ids of the GPIRT_RNG_ITEM contract */
enum {
    GPIRT_ST_INIT_F = 1, GPIRT_ST_INIT_BETA = 2, GPIRT_ST_F_Z = 3, GPIRT_ST_F_ESS = 4,
    GPIRT_ST_FSTAR = 5, GPIRT_ST_THETA = 6, GPIRT_ST_BETA = 7,
    GPIRT_ST_PPC = 8,     /* the replicate of the posterior predictive checks (below); no stage of the chain draws from it */
    GPIRT_ST_AMP_CENTRED = 13,  /* the centred amplitude update (gpirt_sampler_draw_amp_centred): item index item0 + j, index 0 .. 63 the normals of the augmentation, 64 / 65 the two uniforms; nothing else draws from it */
    GPIRT_ST_BETA_CENTRED = 14, /* the two normals per item of the centred beta update (gpirt_sampler_draw_beta_centred): item index item0 + j, index 0 / 1; nothing else draws from it */
    GPIRT_ST_SCALE = 15,  /* the collapsed scale and shift move (gpirt_sampler_draw_scale): item index the kind (0 scale, 1 shift), index 0 the normal's uniform, 1 the decision's; nothing else draws from it */
    GPIRT_ST_AMP = 10,    /* the two uniforms per item of an amplitude update (gpirt_sampler_draw_amp): item index item0 + j, index 0 / 1; nothing else draws from it */
    GPIRT_ST_POP = 12,    /* the two uniforms per group of a population-prior update (gpirt_sampler_draw_pop): item index g, index 0 (mu) / 1 (sd); nothing else draws from it */
    GPIRT_ST_CARRY = 11,  /* the nugget of the consistent step's carry (gpirt_sampler_carry_f): item index item0 + j, index i; nothing else draws from it */
    GPIRT_ST_ORD = 16,    /* the two uniforms per threshold of an ordinal threshold update (gpirt_sampler_draw_thresholds): item index item0 + j, index 2 (c - 1) the window's placement, 2 (c - 1) + 1 the draw; nothing else draws from it */
    GPIRT_ST_ORD_PPC = 17, /* the replicate of the ordinal model's posterior predictive check (gpirt_sampler_ordinal_fit_accumulate): item index item0 + j, index i; nothing else draws from it */
    GPIRT_ST_ELL = 9      /* the two uniforms of a length-scale update: item index 0 the whitened one's (gpirt_sampler_draw_ell), item index 1 the centred one's (gpirt_sampler_draw_ell_centred); nothing else draws from it */
};

typedef struct gpirt_handle_s*  gpirt_handle_t;
typedef struct gpirt_sampler_s* gpirt_sampler_t;

/* ---------------------------------------------------------------- library / handle ------ */
int         gpirt_version(void);    /* 142: fit output for the ordinal model accumulated on the device -- pointwise WAIC, category predictions, the first-order PPC (GPIRT_ST_ORD_PPC, gpirt_ordinal_fit, gpirt_sampler_ordinal_fit_*, gpirt_ordinal_fit_get, gpirt_ordinal_fit_totals, gpirt_ordinal_fit_combine); 138: draw_f's structured product in parts of its own width with the rank-64 term accumulated in the launch of the diagonal parts (GPIRT_NU_SUB; nu changes in rounding only, no change to the interface); 133: a consistent step beside the reference's -- f carried to the new theta plus the model's nugget, and the prior check (GPIRT_ST_CARRY, gpirt_sampler_carry_f, gpirt_sampler_step_consistent, gpirt_carry, gpirt_sampler_carry_stats, gpirt_sampler_prior_quad); 128: draw_f's nu = L z from L's diagonal parts and 64 node rows (GPIRT_NU_LR, gpirt_sampler_nu_lr_draws, gpirt_sampler_nu_lr_rows; gpirt_sampler_ldl has the layouts); 127: group posteriors -- separation, overlap, party-line votes (gpirt_groups, gpirt_groups_check, gpirt_sampler_groups_*, gpirt_groups_combine); 126: a centred length-scale update beside the whitened one (gpirt_sampler_draw_ell_centred, gpirt_sampler_ell_width_centred, gpirt_ell_centred, gpirt_sampler_ell_centred_stats); 125: the kernel's length scale as a parameter of the chain (GPIRT_ST_ELL, gpirt_ell_grid, gpirt_ell_check, gpirt_sampler_ell_*, gpirt_sampler_draw_ell); 124: the covariance kernel is a property of the handle -- squared exponential with a length scale, Matern 5/2, Matern 3/2 (gpirt_kernel, gpirt_kernel_default, gpirt_kernel_check, gpirt_kernel_set, gpirt_kernel_get); 119: gpirt_mcmc_run and gpirt_run replace the thirteen whole-call entries that versions 106 to 118 added one per analysis, each the one before with one more parameter (in that order: quantiles, ppc, ranks, score, predict, pairs, bins, shape, sumscore, dif, equate, loo, order -- the fields of gpirt_run); gpirt_mcmc, gpirt_mcmc_summary and gpirt_mcmc_chains are unchanged; 110: predicting new respondents' unseen answers, next-item information (gpirt_sampler_score_predict_*, gpirt_score_predict_combine); 109: scoring new respondents (gpirt_sampler_score_*, gpirt_score_combine); 108: rank posteriors (gpirt_sampler_rank_*, gpirt_rank_combine); 107: posterior predictive checks (gpirt_sampler_ppc_*, gpirt_ppc_combine); 106: quantiles (gpirt_summary_quantiles); 105: several chains, split-R-hat / ESS / MCSE (GPIRT_SUM_DIAG, gpirt_chains_combine, gpirt_mcmc_chains); 104: posterior summaries (gpirt_sampler_summary_*, gpirt_mcmc_summary); 103: gpirt_debug_poison_allocs, y outside {+1, -1, NaN} refused; 102: gpirt_potrf_subpanel_width(n) takes the order of the matrix; 101: named gpirt_options fields, gpirt_fast_options */
const char* gpirt_last_error(void);
int         gpirt_device_count(int* count);
/* device < 0: current device.  stream is a hipStream_t; NULL is HIP's default (null) stream. */
int         gpirt_create(gpirt_handle_t* h, int device, void* stream);
/* same, but the handle creates and owns a non-blocking stream of its own */
int         gpirt_create_own_stream(gpirt_handle_t* h, int device);
int         gpirt_destroy(gpirt_handle_t h);
int         gpirt_synchronize(gpirt_handle_t h);
int         gpirt_set_stream(gpirt_handle_t h, void* stream);
/* The library's switches (README.md: GPIRT_PANEL, GPIRT_LOOKAHEAD, GPIRT_DEFER, GPIRT_TRSM_INV, GPIRT_LL_EXACT,
 * GPIRT_BORDERED, GPIRT_EARLY_INV, GPIRT_PREP_EARLY; GPIRT_NBO / GPIRT_NBP read-only).  The environment
 * is read ONCE per process; every handle starts from those values and a caller may change them per handle here (drains
 * the handle's stream; takes effect from the next call on).  Nothing in the library reads the environment per call. */
int         gpirt_config_get(gpirt_handle_t h, const char* name, int* value);
int         gpirt_config_set(gpirt_handle_t h, const char* name, int value);
/* Hang-guard fallbacks taken on this handle so far: a factorisation whose persistent sub-panel kernel gave up on a
 * progress counter (its work-groups were not co-resident within the spin bound, e.g. beside a foreign tenant of the GPU)
 * is repeated ONCE from the intact theta with the launch-per-step panel (GPIRT_PANEL=2's path) by gpirt_factor,
 * gpirt_sampler_check and gpirt_mcmc; only a failure of the repeat is an error. */
int         gpirt_guard_fallbacks(gpirt_handle_t h, int* count);
/* Debug: the nth factorisation enqueued on h from now (nth >= 1; 0 disarms) ends the way a guard expiry leaves it -- guard
 * word raised, result unfinished -- without spinning any kernel.  h == NULL arms the handle the NEXT gpirt_mcmc call
 * creates for itself (that call reports its fallbacks through gpirt_debug_last_mcmc_fallbacks). */
int         gpirt_debug_trip_guard(gpirt_handle_t h, int nth);
/* Tests only: a pass of the R-stream replay's draw_f resolves up to three items: the anchor, the next
 * item at one of 15 places its predecessor's uniform count selects, the one after at one of 16.  limit > 0 clamps both
 * candidate counts to min(15 | 16, limit) (0: the full 15 / 16), so that passes which end early -- a predecessor's slice loop
 * consumed more than the slot holds candidates for, the next pass starts at the first unresolved item -- are exercised at
 * will.  There is no host fallback: the anchor is device-side state. */
int         gpirt_debug_rs_cand_limit(gpirt_handle_t h, int limit);
/* Tests only: the R-stream replay's draw_f predicts every item's start in R's stream on a single-precision copy of L and
 * verifies all items exactly afterwards; every > 0 makes the predictor wrong on purpose at every
 * every-th item, so the verification's discard-and-resume path runs.  The draws must not change. */
int         gpirt_debug_rs_mispredict(gpirt_handle_t h, int every);
/* Tests only: on != 0 fills every floating buffer a sampler created on h allocates, and every floating workspace h or its side
 * handle grows, with 0xFF bytes (a quiet NaN in fp64 and fp32) at allocation, so that a kernel reading memory nothing wrote
 * shows in the results.  Integer, flag, ticket and counter buffers are never poisoned.  0 switches it off for later allocations. */
int         gpirt_debug_poison_allocs(gpirt_handle_t h, int on);
/* Debug: pass number `pass` (0-based; < 0: none) of every R-stream draw_f on this handle leaves the in-kernel time stamps of
 * its two kernels in the sampler's "rs_trace" array (gpirt_sampler_get, 128 64-bit words, 100 MHz): tools/rs_trace.py. */
int         gpirt_debug_rs_trace(gpirt_handle_t h, int pass);
int         gpirt_debug_last_mcmc_fallbacks(void);
/* Peak fp64 MFMA rate of this device measured by a back-to-back v_mfma_f64_16x16x4_f64 loop
 * (TFLOP/s); used to calibrate the roofline. */
int         gpirt_calibrate_mfma_f64(gpirt_handle_t h, double* tflops);

/* ---------------------------------------------------------------- the covariance kernel -- */
/* K(a, b) = k(|a - b| / length_scale) with k(0) = 1 for every family, S = K(theta, theta) + GPIRT_JITTER I:
 *   GPIRT_KERNEL_SE        k(r) = exp(-r^2 / 2)                          (the reference's, at length_scale = 1)
 *   GPIRT_KERNEL_MATERN52  k(r) = (1 + a + a^2 / 3) exp(-a), a = sqrt(5) r
 *   GPIRT_KERNEL_MATERN32  k(r) = (1 + a) exp(-a),           a = sqrt(3) r
 * length_scale is finite, GPIRT_LENGTH_SCALE_MIN (the spacing of the theta grid) <= length_scale <= GPIRT_LENGTH_SCALE_MAX.
 * There is NO signal variance: draw_fstar's standard deviation is the reference's s = 1 - sqrt(q) (src/draw-fstar.cpp:20),
 * which is a statement about a prior with k(0) = 1 and means nothing for any other k(0).
 *
 * The kernel is a property of the HANDLE (like the switches of gpirt_config_set); gpirt_options and gpirt_run do not know it.
 * gpirt_se_kernel, gpirt_factor and gpirt_draw_fstar read the handle's kernel, and so does every sampler created on the handle
 * afterwards (a sampler keeps the kernel it was created under).  gpirt_mcmc, gpirt_mcmc_summary, gpirt_mcmc_chains and
 * gpirt_mcmc_run create a handle of their own: they run the default kernel.  A handle that was never set, or was set to
 * (GPIRT_KERNEL_SE, 1.0), computes bit for bit what it did before version 124.
 *
 * gpirt_kernel_check touches no device.  It validates k (GPIRT_E_ARG with a message: family outside 0..2, length_scale not
 * finite or outside its range, a non-zero reserved word, kstar_rank not 0 or a multiple of 16 in 16..128) and decides whether
 * gpirt_options.kstar_rank = kstar_rank may be used with it.  The Chebyshev nodes c and the basis V of the rank form do not
 * depend on the kernel; the interpolation error does.  The certificate is max |K(theta, c) V^T - K(theta, theta*)| over theta
 * and theta* on the whole grid, in long double with V rounded to fp64 as the device holds it (*cert_out; 0 for
 * kstar_rank = 0).  A rank is accepted exactly when its certificate is no larger than that of (GPIRT_KERNEL_SE, 1.0, r = 48)
 * from the same routine -- the line gpirt_options.kstar_rank draws for "exact to rounding".  A refusal is GPIRT_E_ARG, its
 * message names the certificate and the smallest allowed rank that passes, which is also *min_rank_out (0: none does).  The
 * Matern kernels are not analytic at r = 0 (the interpolation converges algebraically only): every kstar_rank > 0 is refused
 * for them, *min_rank_out = 0.  cert_out and min_rank_out may be NULL.
 * gpirt_sampler_create applies the same check to a handle whose kernel is not the default (under the default kernel every
 * allowed rank is accepted, as before: r = 16 and r = 32 are the documented approximations); and kernel_fp32 needs the
 * default kernel (GPIRT_E_ARG otherwise).
 * gpirt_kernel_set drains the handle's stream; it is refused (GPIRT_E_ARG) while samplers created on the handle are alive. */
#define GPIRT_KERNEL_SE        0
#define GPIRT_KERNEL_MATERN52  1
#define GPIRT_KERNEL_MATERN32  2
#define GPIRT_LENGTH_SCALE_MIN 0.01
#define GPIRT_LENGTH_SCALE_MAX 1000.0
typedef struct gpirt_kernel {
    int      family;          /* GPIRT_KERNEL_* */
    int      reserved0;       /* must be 0 */
    double   length_scale;
    int64_t  reserved[4];     /* must be 0 */
} gpirt_kernel;
void gpirt_kernel_default(gpirt_kernel* k);                   /* GPIRT_KERNEL_SE, 1.0 */
int  gpirt_kernel_check(const gpirt_kernel* k, int kstar_rank, double* cert_out, int* min_rank_out);
int  gpirt_kernel_set(gpirt_handle_t h, const gpirt_kernel* k);
int  gpirt_kernel_get(gpirt_handle_t h, gpirt_kernel* k);

/* ---------------------------------------------------------------- operators ------------- */
/* K(): src/covariance-function.cpp:3-14 under the handle's kernel (above).  d_out (n1 x n2, leading dimension ld) =
 * k(|x1_i - x2_j| / length_scale), by default exp(-0.5 (x1_i - x2_j)^2); `jitter` is added where i == j
 * (src/gpirtMCMC.cpp:16; pass 0 for K(theta, theta_star), src/draw-fstar.cpp:17). */
int gpirt_se_kernel(gpirt_handle_t h, const double* d_x1, int64_t n1, const double* d_x2,
                    int64_t n2, double* d_out, int64_t ld, double jitter);

/* arma::chol(S, "lower"): src/gpirtMCMC.cpp:17,78,97.  In place on d_A (n x n, lda): on exit the
 * lower triangle holds L and the strict upper triangle is zero.  Blocked right-looking
 * factorisation, trailing update on fp64 MFMA.  Returns info (>0) if S is not positive definite. */
int gpirt_potrf_lower(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda);

/* Fused K(theta,theta) + jitter + chol: src/gpirtMCMC.cpp:15-17,76-78,95-97.  d_L n x n. */
int gpirt_factor(gpirt_handle_t h, const double* d_theta, int64_t n, double* d_L, int64_t ldl);

/* The same factorisation in pieces, for a host that distributes it over several GPUs (one process each): outer panel
 * p = columns [p W, min((p + 1) W, n)), W = gpirt_potrf_panel_width().  With 1-D block-cyclic ownership of the outer
 * panels the owner of p calls panel_factor once its columns carry the updates of every panel q < p, the finished
 * panel travels to the other ranks through panel_copy (rows [pW, n) of the panel <-> a dense (n - pW) x w buffer the
 * host broadcasts), and every rank applies it to the block columns c > p it owns with panel_update.  The pieces are
 * the launches gpirt_potrf_lower itself makes, so the assembled factor is bit-identical to it.  Nothing here
 * synchronises; gpirt_potrf_begin clears the info word and gpirt_potrf_finish drains the stream and returns it. */
int64_t gpirt_potrf_panel_width(void);
int gpirt_potrf_begin(gpirt_handle_t h);
int gpirt_potrf_panel_factor(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p);
int gpirt_potrf_panel_update(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, int64_t c);
int gpirt_potrf_panel_copy(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, double* d_buf, int to_buf);
int gpirt_potrf_finish(gpirt_handle_t h);
/* The same pieces by HALVES of an outer panel, for a host that pipelines its broadcasts: an outer panel is factored as a
 * first sub-panel of gpirt_potrf_subpanel_width(n) columns (GPIRT_NBP, or chosen by the order n of the matrix) and the rest, and the next panel's first columns take the panel's
 * update as two products (first sub-panel, then the rest -- the same rule launch_potrf_lower follows on one GPU), so
 *   half: 0 = the panel's first sub-panel, 1 = the rest of it, 2 = the whole panel        (factor / copy)
 *   part: 0 = what needs only panel p's first sub-panel, 1 = everything else, 2 = all     (update)
 * let the next owner start on a panel's first half while its second half is still being factored or travelling.
 * Factoring / updating by halves launches exactly what the whole-panel calls launch, in the same order: L is the same
 * bit for bit.  copy_part moves the part's columns, rows from the part's first row down (dense, ld = that row count);
 * buf_doubles is the capacity of d_buf in doubles: a part that does not fit is refused (GPIRT_E_ARG), never truncated
 * (half 1 is W - H columns wide, wider than half 0 whenever GPIRT_NBP < GPIRT_NBO / 2). */
int64_t gpirt_potrf_subpanel_width(int64_t n);
int gpirt_potrf_panel_factor_part(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, int half);
int gpirt_potrf_panel_update_part(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, int64_t c, int part);
int gpirt_potrf_panel_copy_part(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, int half, double* d_buf,
                                int64_t buf_doubles, int to_buf);
/* Debug aid for hosts that enqueue collectives between the pieces: *busy = bit mask of the handle's INTERNAL streams that
 * still have work in flight (0 = every piece has joined the handle's stream, as each must before it returns). */
int gpirt_debug_streams_busy(gpirt_handle_t h, int* busy);
/* One term of ll() (src/log-likelihood.cpp:20,34), log(1 + exp(-a)), elementwise for the n device values d_a:
 * fast = 0 the formula as written through the device library's exp and log (ll_bar, draw_beta, draw_theta and every
 * R-stream replay use it), fast = 1 the form of csrc/ll_fast.h that the elliptical-slice kernel of the item-keyed RNG
 * evaluates (within 3 ulp of the exact value; GPIRT_LL_EXACT=1 makes that kernel use the written form too), fast = 2 the
 * single-precision SCREEN that kernel tries first at every trial point: it only decides an accept test whose sum is
 * further from the slice level than the screen's error bound (4e-6 per row), everything closer is repeated in full
 * precision, so the decisions and the draws are the full-precision ones (GPIRT_ESS_SCREEN=2 switches the screen off). */
/* In-kernel time stamps of ONE sub-panel launch of the factorisation as it runs inside the schedule (100 MHz wall clock:
 * [row block relative to the launch][step 0..39][slot 0..7], the layout tools/micro/panel_bench.hip prints).
 * host_out == NULL arms it for the launch that starts at column k0 (count = entries to allocate, >= 40 * 8 * row blocks;
 * count = 0 disarms and frees); otherwise copies `count` entries out.  tools/panel_trace_insitu.py. */
int gpirt_debug_panel_trace(gpirt_handle_t h, int64_t k0, long long* host_out, int64_t count);
int gpirt_debug_ll_term(gpirt_handle_t h, const double* d_a, int64_t n, double* d_out, int fast);
/* The log-posterior of draw_theta before the prior (GPIRT_NGRID x n, column i = respondent i): the product
 * sum_j [y_ij = +-1] -log(1 + exp(-+ f*_gj)) as gpirt_draw_theta and the sampler form it -- in exact fixed point on the int8
 * matrix cores (csrc/theta_fixed.hip; every term rounded once to 54 bits of its grid row's range, the sums exact), or with
 * GPIRT_THETA_FIXED=2 as the fp64 GEMM.  *fell_back = 1 when the fixed-point form handed over to the fp64 product on its
 * own (|f*| > 709 or non-finite somewhere: the formula as written overflows there).  Synchronises the handle's stream. */
int gpirt_debug_theta_logpost(gpirt_handle_t h, const double* d_y, const double* d_fstar, int64_t n, int64_t m,
                              double* d_logpost_out, int* fell_back);
/* The same product with in-kernel stamps: six 64-bit words per work-group of the int8 kernel (the first 1024 of them) --
 * shader clock (s_memtime) and 100 MHz wall clock (s_memrealtime) at its start, after its main loop and at its end; what the
 * clock the chip holds under this kernel and the share of its prologue and epilogue are read from (tools/theta_clock.py). */
int gpirt_debug_theta_clock(gpirt_handle_t h, const double* d_y, const double* d_fstar, int64_t n, int64_t m,
                            long long* host_stamps, int64_t count);

/* rmvnorm()'s product `cholS * res` (src/mvnormal.h:10) for all item columns at once:
 * d_out (n x m) = L * Z with L lower triangular; the strict upper triangle of d_L must hold zeros
 * (as gpirt_potrf_lower / arma::chol leave it). */
int gpirt_trmm_lz(gpirt_handle_t h, const double* d_L, int64_t n, int64_t ldl, const double* d_Z,
                  int64_t m, int64_t ldz, double* d_out, int64_t ldo);

/* solve(trimatl(L), B) (trans = 0) and solve(trimatu(L.t()), B) (trans = 1):
 * src/draw-fstar.cpp:7,19.  In place on d_B (n x nrhs, ldb). */
int gpirt_trsm_lower(gpirt_handle_t h, const double* d_L, int64_t n, int64_t ldl, double* d_B,
                     int64_t nrhs, int64_t ldb, int trans);

/* General fp64 MFMA GEMM used by every stage: C = alpha * op(A) op(B) + beta * C.
 * ta/tb: 0 = as stored, 1 = transposed.  C is M x N. */
int gpirt_gemm(gpirt_handle_t h, int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha,
               const double* d_A, int64_t lda, const double* d_B, int64_t ldb, double beta,
               double* d_C, int64_t ldc);

/* ll_bar() for every column: src/log-likelihood.cpp:25-37.  d_out[j] = ll_bar(f_j, y_j, mu_j).
 * d_mu may be NULL (then this is ll(), :12-23). */
int gpirt_ll_bar(gpirt_handle_t h, const double* d_f, const double* d_y, const double* d_mu,
                 int64_t n, int64_t m, double* d_out);

/* draw_f(): src/draw-f.cpp:64-73 under GPIRT_RNG_ITEM: Z ~ N(0,1) from (seed, iter) sub-streams,
 * nu = L Z as one trmm, then one elliptical-slice update per column (ess(), :21-60).
 * In place on d_f (n x m).  d_k_out (m ints, may be NULL) receives the rejection counts.  d_y holds +1, -1 or NaN (a missing
 * response); any other value is refused with GPIRT_E_ARG before d_f is touched. */
int gpirt_draw_f(gpirt_handle_t h, double* d_f, const double* d_y, const double* d_L, int64_t ldl,
                 const double* d_mu, int64_t n, int64_t m, uint64_t seed, uint32_t iter,
                 int* d_k_out);

/* Library version 143.  gpirt_draw_f for a linear mean given by its parts: mu[i + j n] = d_beta[2 j] + d_theta[i] * d_beta[2 j + 1]
 * (one multiply, one add).  y is packed to two bits a cell and the slice kernel forms mu itself (csrc/ess_lin.hip, DESIGN.md
 * section 51); f, the rejection counts and the error code are gpirt_draw_f's on that mu, bit for bit.  2048 < n <= 8192, any
 * other n is GPIRT_E_ARG.  Inside a sampler the same kernel runs under GPIRT_ESS_PACK (gpirt_config_set): 1 (the default)
 * where the sampler knows that mu is b0 + theta b1 of the theta and beta in place (written last by draw_beta or at
 * initialisation; any entry that writes theta, beta or mu another way sends the next draw_f to the kernel that reads mu and
 * y), one work-group per item; 3 the same with two work-groups per CU striding over the items; 2 never.
 * gpirt_sampler_ess_pack_draws: how many draws of this sampler took the packed kernel. */
int gpirt_draw_f_linear(gpirt_handle_t h, double* d_f, const double* d_y, const double* d_L, int64_t ldl,
                        const double* d_theta, const double* d_beta, int64_t n, int64_t m, uint64_t seed,
                        uint32_t iter, int* d_k_out);
int gpirt_sampler_ess_pack_draws(gpirt_sampler_t s, int64_t* draws);

/* draw_fstar(): src/draw-fstar.cpp:10-31 under GPIRT_RNG_ITEM.  d_out (N x m), N = GPIRT_NGRID.
 * fused = 0: alpha = L^-T L^-1 f as in the reference (double_solve, :3-8);
 * fused = 1: mean = (L^-1 kstar)^T (L^-1 f), algebraically identical, one trsm fewer.
 * d_s_out (N) and d_mean_out (N x m) may be NULL. */
int gpirt_draw_fstar(gpirt_handle_t h, const double* d_f, const double* d_theta, const double* d_L,
                     int64_t ldl, const double* d_mu_star, int64_t n, int64_t m, uint64_t seed,
                     uint32_t iter, int fused, double* d_out, double* d_s_out, double* d_mean_out);

/* draw_theta(): src/draw-theta.cpp:3-37 under GPIRT_RNG_ITEM, as one fp64 MFMA GEMM over the
 * +1 / -1 indicator matrices of y.  stabilise = 1 subtracts the column maximum before exp. */
int gpirt_draw_theta(gpirt_handle_t h, const double* d_y, const double* d_fstar, int64_t n,
                     int64_t m, uint64_t seed, uint32_t iter, int stabilise, double* d_theta_out,
                     int* d_degenerate);

/* draw_beta(): src/draw-beta.cpp:3-41 under GPIRT_RNG_ITEM.  In place on d_beta (2 x m). */
int gpirt_draw_beta(gpirt_handle_t h, double* d_beta, const double* d_theta, const double* d_y,
                    const double* d_f, const double* d_prior_means, const double* d_prior_sds,
                    const double* d_step_sizes, int64_t n, int64_t m, uint64_t seed, uint32_t iter);
/* Library version 141: the same draws from two leaner kernels.  draw_beta under the item RNG at n <= 8192
 * keeps an item's f and theta in registers and decides each accept test by a single-precision screen of the two log-likelihood
 * sums wherever their difference is further from log u than the screen's error band (4e-6 n per sum); inside the band, with an
 * observed row's argument below -709, or with a NaN in the comparison, the test is the full-precision expression of version 140,
 * same sums in the same order.  beta, mu and mu_star are bit for bit those of version 140.  GPIRT_BETA_SCREEN (gpirt_config_set):
 * 1 this (the default), 2 always the kernel of version 140.  gpirt_draw_beta first checks that y holds +1, -1 and NaN only (one
 * small launch and a stream synchronisation) and takes the kernel of version 140 when it does not.
 * gpirt_draw_beta_paths, for tests: gpirt_draw_beta that also records which path took each decision.  d_path (2 x m ints, device):
 * entry k + 2 j = 0 when the screen decided coefficient k of item j, 1 when full precision did; the kernel of version 140
 * leaves d_path as it was.
 * The normal fills (gpirt_item_normals, draw_f's N(0,1) draws) evaluate the tail branch of AS241 (|u - 0.5| > 0.425) on a
 * compacted list per 1024 elements instead of under a mask in every wavefront; every value is bit for bit that of version 140.
 * GPIRT_ZFILL_COMPACT (gpirt_config_set): 1 this (the default), 2 the kernel of version 140. */
int gpirt_draw_beta_paths(gpirt_handle_t h, double* d_beta, const double* d_theta, const double* d_y,
                          const double* d_f, const double* d_prior_means, const double* d_prior_sds,
                          const double* d_step_sizes, int64_t n, int64_t m, uint64_t seed, uint32_t iter, int* d_path);

/* The item-RNG primitives, exported so hosts and tests can address the same sub-streams. */
int gpirt_item_uniforms(gpirt_handle_t h, uint64_t seed, uint32_t iter, uint32_t stage,
                        uint32_t item0, int64_t n_items, int64_t n_index, double* d_out);
int gpirt_item_normals(gpirt_handle_t h, uint64_t seed, uint32_t iter, uint32_t stage,
                       uint32_t item0, int64_t n_items, int64_t n_index, double* d_out);

/* ---------------------------------------------------------------- R's RNG on the host --- */
/* set.seed(seed) + unif_rand()/norm_rand() of R's default Mersenne-Twister/inversion generator.
 * Host code (R does this itself before the call: theta_init <- rnorm(n), R/gpirtMCMC.R:95-97). */
typedef struct gpirt_rstream_s* gpirt_rstream_t;
int gpirt_rstream_create(gpirt_rstream_t* r, uint32_t seed);
int gpirt_rstream_from_state(gpirt_rstream_t* r, const uint32_t mt[624], int mti);
int gpirt_rstream_get_state(gpirt_rstream_t r, uint32_t mt[624], int* mti);
int gpirt_rstream_destroy(gpirt_rstream_t r);
int gpirt_rstream_unif(gpirt_rstream_t r, double* h_out, int64_t n);
int gpirt_rstream_norm(gpirt_rstream_t r, double* h_out, int64_t n);

/* ---------------------------------------------------------------- sampler --------------- */
typedef int (*gpirt_tick_fn)(void* ctx, int iter, int total);  /* nonzero return = stop */

typedef struct gpirt_options {
    int      rng_kind;        /* GPIRT_RNG_RSTREAM or GPIRT_RNG_ITEM */
    uint64_t seed;            /* GPIRT_RNG_ITEM key */
    int      theta_stabilise; /* 1 = subtract the row maximum before exp in draw_theta */
    int      fstar_fused;     /* see gpirt_draw_fstar */
    int      device;          /* < 0: current device */
    int      reserved0;       /* must be 0 (round 1 reserved this slot for a hipGraph replay switch that was never
                               * built: the host enqueues one iteration in 0.40 ms against 8.3 ms on the device,
                               * tools/host_time_probe.py, so a graph has nothing to win; the slot keeps the layout) */
    /* item sharding (one process per GPU): this rank owns item columns [item0, item0 + m) of a
     * global problem with m_total items; y / priors / outputs passed in are the LOCAL columns. */
    int64_t  item0;
    int64_t  m_total;
    int      reserved1;       /* must be 0 */
    int      kernel_fp32;     /* 1: K(theta, theta) is built with single-precision exp() before the fp64 factorisation
                               * (BASELINE config C5; parity then only statistical) */
    int      kstar_rank;      /* r (16..128, multiple of 16; needs fstar_fused): draw_fstar works with the rank-r Chebyshev
                               * factorisation K(theta, theta*) = K(theta, c) V^T of src/draw-fstar.cpp:17 and solves r + m
                               * right-hand sides instead of 1001 + m; 0 = every grid column is solved.  max |K(theta, c) V^T -
                               * K(theta, theta*)| over the grid, in long double with V as stored (tests/test_stage_exact_cpu.py):
                               *   r = 16: 4.6e-3    r = 32: 3.8e-8    r = 48: 8.7e-15    r = 64 .. 128: 1.1e-16 .. 1.3e-16
                               * r = 16 and r = 32 are APPROXIMATIONS of K* (f* moves by that error times ||S^-1 f||_1); from
                               * r = 48 on the form is exact to rounding.  At r = 16 the error lifts ||L^-1 k*|| above 1 at
                               * about a fifth of the grid points: s = 1 - sqrt(q) < 0 there and R::rnorm's rule makes f* NaN
                               * (tests/test_gpu_fstar_ranks.py): r = 16 is not usable for a chain */
    int      reserved[4];     /* must be 0.  (Up to version 100 kernel_fp32 and kstar_rank were the unnamed slots
                               * reserved[1] and reserved[2] of an int reserved[8] at this offset: same layout, same size.) */
    int      factor_structured; /* 0 or 1 (version 131; up to 130 the last slot of an int reserved[5]: same layout, same size).
                               * 1: where the sampler's steady iteration reads nothing else of the factor (the conditions of
                               * gpirt_sampler_factor_lr_count below) a factorisation builds only L's 512-column diagonal parts
                               * and the 64 node rows, from theta; the dense factor is formed on demand.  0: every
                               * factorisation is the dense one, bit for bit as before. */
} gpirt_options;

/* The reference's contract: GPIRT_RNG_RSTREAM (draw-for-draw replay of R's stream), draw_theta and draw_fstar as
 * written.  NOTE: these defaults REQUIRE an R stream -- gpirt_sampler_create / gpirt_mcmc called with opts == NULL
 * (or with unmodified defaults) and rs == NULL fail with GPIRT_E_ARG ("GPIRT_RNG_RSTREAM needs an R stream state");
 * a host without R's RNG state sets rng_kind = GPIRT_RNG_ITEM (and a seed) explicitly. */
void gpirt_default_options(gpirt_options* o);
/* The throughput preset -- what bench.py times as its headline and what BASELINE.json's metric is quoted on: the item-keyed
 * RNG (seed = 1: set your own), theta_stabilise = 1, fstar_fused = 1, kstar_rank = 64, factor_structured = 1 (from n = 2048
 * on a factorisation then builds L's diagonal parts and node rows alone, from theta: f within 1e-10 max(1, max|f|) and f* within
 * 1e-9 max|f*| of the dense factor's, theta and beta the same draws).  Same sampler, every form
 * algebraically identical to the reference's (DESIGN.md sections 4-5: f* within 1e-9 of the as-written form relative to
 * max|f*| at 8192 x 1024, checked in every bench.py run); draws are NOT those of R's stream (gpirt_default_options is
 * that contract).  One call away from the drop-in: the R shim selects it with options(gpirt.hip.preset = "fast"). */
void gpirt_fast_options(gpirt_options* o);

/* Whole-call drop-in for .gpirtMCMC (src/gpirtMCMC.cpp:5-117), all pointers HOST:
 *   h_y            n x m   responses (never modified)
 *   h_theta0       n       initial theta (copied, R semantics)
 *   h_prior_means / h_prior_sds / h_step_sizes   2 x m
 *   h_theta_draws  (S+1) x n, h_beta_draws 2 x m x (S+1), h_f_draws n x m x (S+1), h_irfs 1001 x m
 * R-stream mode: rs carries R's Mersenne-Twister state in and out (GetRNGstate/PutRNGstate of
 * Rcpp::RNGScope, src/RcppExports.cpp:19); ignored for GPIRT_RNG_ITEM.
 * tick may be NULL; it is called once per iteration before the draws (Rprintf +
 * checkUserInterrupt, src/gpirtMCMC.cpp:64-66,83-85). */
int gpirt_mcmc(const double* h_y, int64_t n, int64_t m, const double* h_theta0,
               int sample_iterations, int burn_iterations, const double* h_prior_means,
               const double* h_prior_sds, const double* h_step_sizes, const gpirt_options* opts,
               gpirt_rstream_t rs, gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws,
               double* h_beta_draws, double* h_f_draws, double* h_irfs);

/* ------------------------------------------------------ posterior summaries ------------- */
/* Summaries of a chain accumulated on the device, one draw at a time, in O(n m) memory however long the chain (the stored
 * f draws of gpirt_mcmc take n m 8 bytes per iteration).  Parts (bits of `parts`):
 *   GPIRT_SUM_THETA_BETA  theta_mean / theta_var (n), beta_mean / beta_var (2 x m); always on when any part is
 *   GPIRT_SUM_F           f_mean / f_var (n x m)
 *   GPIRT_SUM_PRED        p_yes (n x m): mean over the draws of P(y = 1) = plogis(f + mu); for a missing cell the
 *                         held-out prediction
 *   GPIRT_SUM_WAIC        lppd, p_waic (n x m; NaN where y is missing) and the totals below
 * For cell (i, j) of draw s, ll = -softplus(-y g) with g = f + mu (src/log-likelihood.cpp:25-37);
 * lppd_ij = log(mean_s exp(ll_s)) (a running logaddexp), p_waic_ij = var_s(ll_s) (ddof = 1, Welford).  Every variance and
 * p_waic is NaN with fewer than two draws.  A draw is the state at the end of a sampling iteration (slot s >= 1 of the
 * stored draws); burn-in and the initial state never enter. */
#define GPIRT_SUM_THETA_BETA 1
#define GPIRT_SUM_F          2
#define GPIRT_SUM_PRED       4
#define GPIRT_SUM_WAIC       8
/* totals[] over the observed cells (GPIRT_SUM_WAIC): sums of lppd_ij and p_waic_ij, elpd_waic = lppd - p_waic,
 * waic = -2 elpd_waic, se_elpd_waic = sqrt(n_obs var(elpd_ij)) (ddof = 1, as the loo package), n_obs, draws, and the
 * mean and sum of squared deviations of elpd_ij (what shards combine exactly by Chan's formula) */
#define GPIRT_SUM_T_LPPD         0
#define GPIRT_SUM_T_P_WAIC       1
#define GPIRT_SUM_T_ELPD_WAIC    2
#define GPIRT_SUM_T_WAIC         3
#define GPIRT_SUM_T_SE_ELPD_WAIC 4
#define GPIRT_SUM_T_N_OBS        5
#define GPIRT_SUM_T_DRAWS        6
#define GPIRT_SUM_T_ELPD_MEAN    7
#define GPIRT_SUM_T_ELPD_SS      8
#define GPIRT_SUM_NTOTALS        9

/* What gpirt_mcmc_summary returns besides the IRFs: the parts wanted, a HOST pointer per output (NULL: not wanted; a
 * pointer to a part that is off is refused) and the totals (written when GPIRT_SUM_WAIC is on). */
typedef struct gpirt_summary {
    int      parts;
    int      reserved;        /* must be 0 */
    double*  h_p_yes;         /* n x m */
    double*  h_lppd;          /* n x m */
    double*  h_p_waic;        /* n x m */
    double*  h_f_mean;        /* n x m */
    double*  h_f_var;         /* n x m */
    double*  h_theta_mean;    /* n */
    double*  h_theta_var;     /* n */
    double*  h_beta_mean;     /* 2 x m */
    double*  h_beta_var;      /* 2 x m */
    double   totals[GPIRT_SUM_NTOTALS];
} gpirt_summary;

/* gpirt_mcmc with summaries: same inputs, the same chain (draws, IRFs and R's stream bit-identical to gpirt_mcmc's);
 * h_theta_draws, h_beta_draws and h_f_draws may each be NULL (not stored), h_irfs is required.  GPIRT_RNG_ITEM: each draw
 * is added from its checkpoint once that is verified, so a hang-guard rollback never counts an iteration twice. */
int gpirt_mcmc_summary(const double* h_y, int64_t n, int64_t m, const double* h_theta0,
                       int sample_iterations, int burn_iterations, const double* h_prior_means,
                       const double* h_prior_sds, const double* h_step_sizes, const gpirt_options* opts,
                       gpirt_rstream_t rs, gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws,
                       double* h_beta_draws, double* h_f_draws, double* h_irfs, gpirt_summary* summary);

/* ------------------------------------------------------ several chains, convergence diagnostics ------------- */
/* GPIRT_SUM_DIAG: per theta (n), beta (2 x m) and, with GPIRT_SUM_F, f cell (n x m), the accumulators of split-R-hat and a
 * batch-means ESS for a chain of S planned draws (gpirt_sampler_summary_enable_planned; the only way to turn it on):
 * Welford moments of half 1 (draws 1..floor(S/2)) and half 2 (draws S-floor(S/2)+1..S; with S odd the middle draw is in
 * neither), and of the means of a = floor(S/b) batches of b = floor(sqrt(S)) draws (draws 1..a b).  The ESS is the
 * batch-means one, NOT the rank-normalised ESS of Vehtari et al. (2021): rank normalisation needs every draw.
 * Split-R-hat (BDA3) over M = 2C half-chains of N = floor(S/2) draws: B = N/(M-1) sum_j (xbar_j - xbar)^2,
 * W = mean_j s_j^2 (ddof 1), var+ = (N-1)/N W + B/N, Rhat = sqrt(var+ / W); W = 0 gives +inf if B > 0 and NaN otherwise,
 * S < 4 gives NaN.  ESS = C S mean_c(lambda_c^2) / mean_c(sigma_c^2) with lambda_c^2 the chain's variance (ddof 1) and
 * sigma_c^2 = b/(a-1) sum_k (Ybar_ck - Ybar_c)^2 (Ybar_c: the mean of the chain's batch means); MCSE of the pooled mean =
 * sqrt(mean_c(sigma_c^2) / (C S)); a < 2 gives NaN.  Batch means all equal (mean_c(sigma_c^2) = 0) give MCSE 0 and
 * ESS = x / 0: +inf where the chains vary (mean_c(lambda_c^2) > 0), NaN where every draw is equal. */
#define GPIRT_SUM_DIAG       16
/* chain c's GPIRT_RNG_ITEM seed: chain 0 uses seed; chain c >= 1 the splitmix64 finaliser of seed + c GAMMA:
 * z = (z ^ (z >> 30)) M1; z = (z ^ (z >> 27)) M2; z ^ (z >> 31) */
#define GPIRT_CHAIN_SEED_GAMMA 0x9E3779B97F4A7C15ULL
#define GPIRT_CHAIN_SEED_M1    0xBF58476D1CE4E5B9ULL
#define GPIRT_CHAIN_SEED_M2    0x94D049BB133111EBULL
uint64_t gpirt_chain_seed(uint64_t seed, int c);

/* per-block scalars of gpirt_diag: blocks theta, beta, f; NaN values are left out of the max / min and counted apart
 * (a block whose every value is NaN, or f without GPIRT_SUM_F, has NaN max / min) */
#define GPIRT_DIAG_THETA      0
#define GPIRT_DIAG_BETA       1
#define GPIRT_DIAG_F          2
#define GPIRT_DIAG_NBLOCKS    3
#define GPIRT_DIAG_MAX_RHAT   0
#define GPIRT_DIAG_MIN_ESS    1
#define GPIRT_DIAG_N_RHAT_HIGH 2   /* R-hat > 1.01 (+inf included) */
#define GPIRT_DIAG_N_RHAT_NAN 3
#define GPIRT_DIAG_N_ESS_NAN  4
#define GPIRT_DIAG_NSCALARS   5
typedef struct gpirt_diag {
    double*  h_theta_rhat;    /* n; every pointer may be NULL (not wanted) */
    double*  h_theta_ess;
    double*  h_theta_mcse;
    double*  h_beta_rhat;     /* 2 x m */
    double*  h_beta_ess;
    double*  h_beta_mcse;
    double*  h_f_rhat;        /* n x m (needs GPIRT_SUM_F) */
    double*  h_f_ess;
    double*  h_f_mcse;
    int*     reflected;       /* C flags: 1 where the chain was reflected (theta -> -theta) */
    double   scalars[GPIRT_DIAG_NBLOCKS][GPIRT_DIAG_NSCALARS];
    int64_t  reserved[4];     /* must be 0 */
} gpirt_diag;

/* The accumulators of a sampler's summaries live in ONE contiguous, 16-byte-aligned device block: a header of 8 int64
 * (n, m, parts, planned S, draws done, layout version, grid points, 0), then the arrays, a copy of y (GPIRT_SUM_WAIC: the
 * missing cells) and of the chain's IRF sum (1001 x m).  It can be copied anywhere -- another process, another GPU -- and
 * combined there.  summary_state refreshes the header and the IRF sum and returns the block (valid until the summaries are
 * enabled again or the sampler is destroyed). */
int gpirt_sampler_summary_enable_planned(gpirt_sampler_t s, int parts, int64_t planned_draws);
int gpirt_summary_state_bytes(int64_t n, int64_t m, int parts, int64_t* bytes);
int gpirt_sampler_summary_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
/* Combine C chains' state blocks (device pointers on h's device; headers identical, GPIRT_SUM_DIAG states complete):
 * pooled moments (Chan's formula in chain order), p_yes, lppd (logaddexp over chains), p_waic and the totals as
 * gpirt_mcmc_summary fills `pooled` (pooled->parts: a subset of the states' parts); the diagnostics into diag (needs
 * GPIRT_SUM_DIAG; may be NULL); the pooled IRFs plogis(sum_c irf_sum_c / (C S)) into h_irfs (1001 x m, may be NULL).
 * Reflection theta -> -theta (a mode of the likelihood with symmetric priors): signs (C values of +1 / -1) forces it;
 * signs == NULL and align != 0 reflects chain c >= 1 when sum_i thetabar_c,i thetabar_0,i < 0.  A reflected chain enters
 * with its theta means and beta slope (row 1) means negated and its IRF sum reversed along the grid; f, p_yes and WAIC are
 * unchanged.  No atomics: bit-identical from run to run. */
int gpirt_chains_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, int align,
                         double* h_irfs, gpirt_summary* pooled, gpirt_diag* diag);
/* C chains one after another on one handle (GPIRT_RNG_ITEM only), each the gpirt_mcmc_summary loop with
 * seed = gpirt_chain_seed(opts->seed, c) and column c of h_theta0 (n x C), then gpirt_chains_combine with align.  The
 * draws (each may be NULL) are chain-major: chain c's gpirt_mcmc layout at offset c (S+1) n, c 2 m (S+1), c n m (S+1).
 * tick sees (c total + it, C total), total = S + B. */
int gpirt_mcmc_chains(const double* h_y, int64_t n, int64_t m, const double* h_theta0, int chains,
                      int sample_iterations, int burn_iterations, const double* h_prior_means,
                      const double* h_prior_sds, const double* h_step_sizes, const gpirt_options* opts, int align,
                      gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws, double* h_beta_draws, double* h_f_draws,
                      double* h_irfs, gpirt_summary* pooled, gpirt_diag* diag);

/* ------------------------------------------------------ quantiles: theta intervals, IRF bands, rank R-hat --- */
/* Two more parts of a summary state (gpirt_sampler_summary_enable(_planned), gpirt_summary_state_bytes; NOT of
 * gpirt_summary.parts, which has no place for their outputs).  Their arrays follow every other array of the state block.
 * GPIRT_SUM_THETA_HIST: per respondent, uint32 counts over the GPIRT_NGRID grid points of all draws (a theta draw is a grid
 * point, -5 + 0.01 k); with GPIRT_SUM_DIAG also the counts of half 1 and half 2 (DIAG's halves).  A draw whose theta is not
 * bit for bit -5 + 0.01 k, k = rint((theta + 5) 100), NaN included, goes in no histogram and is counted per respondent.
 * GPIRT_SUM_IRF_BAND: per f* cell (grid point k, item j), uint32 counts over GPIRT_IRF_BINS bins that cut the probability
 * scale evenly -- x goes in bin #{b : e_b <= x} with the 255 edges e_b = logit(b / 256) of gpirt_irf_band_edges --, a NaN
 * count per cell, and the running sum of plogis(f*) (the posterior mean IRF E[P], not plogis(E f*)). */
#define GPIRT_SUM_THETA_HIST 32
#define GPIRT_SUM_IRF_BAND   128
#define GPIRT_IRF_BINS       256
/* the GPIRT_IRF_BINS - 1 edges e_b = logit(b / 256), b = 1..255, in fp64, increasing (out[0] = e_1) */
int gpirt_irf_band_edges(double* out);

/* per-call scalars of gpirt_quantiles */
#define GPIRT_QNT_MAX_RHAT       0   /* over the respondents whose R-hat is not NaN (NaN if none) */
#define GPIRT_QNT_N_RHAT_HIGH    1   /* R-hat > 1.01 (+inf included) */
#define GPIRT_QNT_N_RHAT_NAN     2
#define GPIRT_QNT_THETA_OFF_GRID 3   /* theta draws not on the grid, over every chain and respondent (should be 0) */
#define GPIRT_QNT_IRF_NAN        4   /* f* draws that were NaN, over every chain and cell */
#define GPIRT_QNT_DRAWS          5   /* T = C S */
#define GPIRT_QNT_IRF_COUNT_MIN  6   /* the least and the most draws a pooled f* cell holds (bins + NaN): T both when */
#define GPIRT_QNT_IRF_COUNT_MAX  7   /* no draw was lost or counted twice */
#define GPIRT_QNT_NSCALARS       8
/* What gpirt_summary_quantiles / gpirt_mcmc_run return: a HOST pointer per output (NULL: not wanted; an output
 * whose part the states lack is refused).  T = C S pooled draws, a reflected chain entering with its grid index
 * reversed (k -> 1000 - k, for theta and for f*'s grid axis).
 * theta_q (nprobs x n): the ceil(q T)-th smallest pooled draw (1-based; q = 0: the smallest; q T, here and below, is
 * the fp64 product), theta_median the same for q = 0.5, theta_mode the most frequent grid point (the lowest on a
 * tie), theta_hist (1001 x n) the pooled counts;
 * NaN (the histogram: as counted) for a respondent with a draw off the grid.  (Needs GPIRT_SUM_THETA_HIST.)
 * theta_rhat_bulk / _tail / theta_rhat (n; needs GPIRT_SUM_DIAG too): the rank-normalised split-R-hat of Vehtari et al.
 * (2021), exact from the half histograms.  Bulk: the 2C halves' T' = 2C floor(S/2) draws ranked with ties averaged,
 * z = Phi^-1((r - 3/8) / (T' + 1/4)), the BDA3 R-hat of GPIRT_SUM_DIAG on z.  Tail: the same on |theta - median| (R's
 * median of all T draws).  theta_rhat = max(bulk, tail), NaN if either is.
 * irf_q (nprobs x 1001 x m; needs GPIRT_SUM_IRF_BAND): in probability, t = q T, b = the first bin with a draw whose
 * cumulative count is >= t (one pass over a cell's bins, the probabilities in ascending order), (b + (t - cum_(b-1)) / count_b) / 256: within 1 / 256 of the ceil(q T)-th smallest
 * plogis(f*) draw (NaN for a cell with a NaN draw).  irf_p_mean (1001 x m): the mean of plogis(f*) over the T draws
 * (NaN for a cell with a NaN draw: the NaN enters the sum).
 * reflected: C flags, as gpirt_diag's. */
typedef struct gpirt_quantiles {
    int            nprobs;
    int            reserved0;       /* must be 0 */
    const double*  probs;           /* nprobs values in [0, 1] */
    double*        theta_q;
    double*        theta_median;    /* n */
    double*        theta_mode;      /* n */
    double*        theta_hist;      /* 1001 x n */
    double*        theta_rhat_bulk; /* n */
    double*        theta_rhat_tail; /* n */
    double*        theta_rhat;      /* n */
    double*        irf_q;
    double*        irf_p_mean;      /* 1001 x m */
    int*           reflected;       /* C */
    double         scalars[GPIRT_QNT_NSCALARS];
    int64_t        reserved[4];     /* must be 0 */
} gpirt_quantiles;
/* Quantiles of C >= 1 chains' state blocks (as gpirt_chains_combine: device pointers on h's device, identical headers;
 * states with GPIRT_SUM_DIAG complete).  The reflection is gpirt_chains_combine's decision for the same states, signs and
 * align.  C S must be < 2^32.  No atomics: bit-identical from run to run. */
int gpirt_summary_quantiles(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, int align,
                            gpirt_quantiles* q);

/* ------------------------------------------------------ posterior predictive checks: items, respondents, the whole matrix --- */
/* Does the model fit these items and these respondents?  For sampling draw s, the state after that iteration's step gives
 *   g_ij = f_ij + mu_ij,  p_ij = plogis(g_ij)  (the arithmetic of GPIRT_SUM_PRED: e = exp(-|g|), p = 1 / (1 + e) for
 *   g >= 0 and e / (1 + e) otherwise),  O = the observed cells, those whose y_ij is not NaN.
 * The replicate is yrep_ij = +1 if u_ij < p_ij, else -1, with
 *   u_ij = the item-RNG uniform of (seed, iter, GPIRT_ST_PPC, item0 + j, i)
 * -- what gpirt_item_uniforms(h, seed, iter, GPIRT_ST_PPC, item0, m, n, .) writes at [i + j n].  iter is the sampler's
 * completed-iteration counter at the time of the call, seed the chain's opts->seed (chain c of several:
 * gpirt_chain_seed(seed, c)).  The uniforms are keyed by the GLOBAL item index and the respondent: they depend neither on
 * the launch geometry nor on a sharding of the items.  The replicate uses the counter-based generator under BOTH RNG
 * contracts: with GPIRT_RNG_RSTREAM it consumes nothing of R's stream, and under either contract the chain is untouched.
 * Per unit -- item j over i in O_j, respondent i over j in O_i, and the whole matrix over O -- and draw:
 *   R = #{yrep = +1},  T = #{y = +1} (fixed; counted on the device at enable),
 *   D(z) = 2 sum softplus(-z g), the deviance of z = y or z = yrep, softplus(a) = log1p(exp(-|a|)) + max(a, 0),
 *   Delta = sum over the cells with yrep != y of y g.  softplus(a) - softplus(-a) = a, so D(yrep) - D(y) = 2 Delta in exact
 *   algebra; D(yrep) >= D(y) is DECIDED as Delta >= 0: exactly 0 when nothing flipped, no cancellation of two large sums,
 *   correct = #{(g > 0) == (y = +1)}, the correctly classified cells (PCP and APRE follow from it).
 * Fields of a unit (GPIRT_PPC_*; every one a double on the way out, counts included):
 *   n_obs, obs_yes = T, rep_yes_mean and rep_yes_var = the mean and the variance (ddof 1) of R over the draws, from the
 *   exact integer sums rep_yes_sum = sum R and rep_yes_sumsq = sum R^2 (uint64): mean = sum R / S,
 *   var = (S sum R^2 - (sum R)^2) / (S (S - 1)) with the numerator exact and rounded once;
 *   yes_ge = #{s : R >= T}, yes_gt = #{s : R > T} (the host derives ppp_yes = yes_ge / S and the mid-p value
 *   (yes_ge + yes_gt) / 2S); dev_obs_mean, dev_rep_mean = the means of D(y), D(yrep); dev_ge = #{s : Delta >= 0};
 *   correct_mean = correct_sum / S; nonfinite; draws.
 * A non-finite g in an observed cell makes that draw count in `nonfinite` of its row, its column and the whole matrix, and
 * enter NO other accumulator of those three units; S above is the unit's draws - nonfinite, the draws that entered.  A
 * unit with no observed cell has NaN means and every count 0; so has a mean with S = 0, and the variance with S < 2.
 * No floating-point atomics: every double sum is reduced in a fixed order (rows in blocks of 256 in order, items in
 * strips of 32 in order, draws in order), so two runs give bit-identical states.
 * Pooling C chains adds the integer sums and counts and adds the double sums in chain order.  The reflection
 * theta -> -theta maps f(theta) to f(-theta) and leaves f_ij + mu_ij of every cell as it is: every PPC output is unchanged
 * by it, so the pooling takes no signs and no alignment. */
#define GPIRT_PPC_N_OBS          0
#define GPIRT_PPC_OBS_YES        1
#define GPIRT_PPC_REP_YES_MEAN   2
#define GPIRT_PPC_REP_YES_VAR    3
#define GPIRT_PPC_YES_GE         4
#define GPIRT_PPC_YES_GT         5
#define GPIRT_PPC_DEV_OBS_MEAN   6
#define GPIRT_PPC_DEV_REP_MEAN   7
#define GPIRT_PPC_DEV_GE         8
#define GPIRT_PPC_CORRECT_MEAN   9
#define GPIRT_PPC_NONFINITE      10
#define GPIRT_PPC_DRAWS          11   /* every draw accumulated (pooled: over the chains) */
#define GPIRT_PPC_REP_YES_SUM    12
#define GPIRT_PPC_REP_YES_SUMSQ  13
#define GPIRT_PPC_CORRECT_SUM    14
#define GPIRT_PPC_NFIELDS        15
/* HOST pointers per field (NULL: not wanted): item[fld] m values, respondent[fld] n values; totals[fld] is always written */
typedef struct gpirt_ppc {
    double*  item[GPIRT_PPC_NFIELDS];
    double*  respondent[GPIRT_PPC_NFIELDS];
    double   totals[GPIRT_PPC_NFIELDS];
    int64_t  reserved[4];     /* must be 0 */
} gpirt_ppc;
/* Stage API.  ppc_enable(on != 0) allocates and zeroes the accumulators and counts n_obs and obs_yes (0 frees them);
 * ppc_accumulate adds the replicate of the CURRENT state as one draw (call it after the step of a sampling iteration);
 * ppc_get finishes one field by name -- "item_" or "respondent_" and the lower-case name of a GPIRT_PPC_* field, e.g.
 * "item_yes_ge" (count <= m or n) --, ppc_totals writes the GPIRT_PPC_NFIELDS fields of the whole matrix.
 * The accumulators live in ONE device block of 8-byte words, apart from the summaries' block: a header of 8 int64 (n, m,
 * draws done, layout version, item0, 0, 0, 0), then 11 arrays of n + m + 1 words (padded to an even count), unit k =
 * item k, respondent k - m, the whole matrix last: uint64 n_obs, obs_yes, sum R, sum R^2, yes_ge, yes_gt, dev_ge, correct
 * sum, nonfinite, then the double sums of D(y) and D(yrep).  ppc_state refreshes the header and returns the block (valid
 * until ppc_enable is called again or the sampler is destroyed); gpirt_ppc_combine pools C such blocks (device pointers
 * on h's device; the same n, m, item0 and response matrix). */
int gpirt_sampler_ppc_enable(gpirt_sampler_t s, int on);
int gpirt_sampler_ppc_accumulate(gpirt_sampler_t s);
int gpirt_sampler_ppc_get(gpirt_sampler_t s, const char* name, double* h_out, int64_t count);
int gpirt_sampler_ppc_totals(gpirt_sampler_t s, double* h_totals);
int gpirt_sampler_ppc_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_ppc_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc* out);

/* ------------------------------------------------------ rank posteriors: rank intervals, pivots, pairwise order --------- */
/* Who is where in the order?  Joint functionals of one theta draw, accumulated without storing it (library version 108).
 * Per draw: the grid index k_i of every respondent, k = rint((theta + 5) 100) where theta is bit for bit -5 + 0.01 k (the
 * rule of GPIRT_SUM_THETA_HIST).  If ANY respondent is off the grid (NaN included) the whole draw is skipped: `skipped`
 * rises by one and nothing else changes.  Otherwise, with S the number of counted draws so far,
 *   less_i = #{j : k_j < k_i},  eq_i = #{j : k_j = k_i} (i itself included),
 *   R2_i = 2 less_i + eq_i + 1 in [2, 2n]: twice the mid-rank, rank 1 the smallest theta.
 * Per respondent: rank2_sum = sum R2 and rank2_sumsq = sum R2^2 (uint64); rank_mean = rank2_sum / (2 S),
 *   rank_var = (S sum R2^2 - (sum R2)^2) / (4 S (S - 1)) (ddof 1; the numerator exact in 128 bits, rounded once; NaN for S < 2).
 *   rank_hist: n x B uint32 (respondent-major) over R2, symmetric under R2 -> 2n + 2 - R2: w = the smallest odd width with
 *   ceil((2n - 1) / w) <= 1025, B = ceil((2n - 1) / w), plus one if that is even (B w is odd), pad = (B w - (2n - 1)) / 2,
 *   bin = (R2 - 2 + pad) / w.  For n <= 512, w = 1 and the histogram is the exact distribution of twice the mid-rank.
 *   rank_q[p]: the max(1, ceil(probs[p] S))-th smallest R2 of the S draws, reported as its bin's upper edge in rank units,
 *   (2 - pad + (bin + 1) w - 1) / 2; rank_bin_width = w / 2.
 * Pivots: up to GPIRT_RANK_MAX_PIVOTS ordinal positions q in 1..n (none given: the median, (n + 1) / 2 for odd n, n / 2 and
 *   n / 2 + 1 for even n); the library closes the set under q <-> n + 1 - q and keeps it sorted (at most 32 positions).
 *   Respondent i covers q in a draw when less_i < q <= less_i + eq_i.  pivot_cover[q][i] (uint32) counts those draws,
 *   pivot_share[q][i] (double) adds 1.0 / eq_i for each of them, in draw order; p_pivot = pivot_share / S.
 * Pairwise (optional): lt[i][j] = #{draws : k_i < k_j}, uint32, n x n, zero diagonal; P(theta_i < theta_j) = lt / S, ties
 *   are S - lt[i][j] - lt[j][i].  MEMORY: 4 n^2 bytes per chain on the device, 268 MB at n = 8192, 1.07 GB at 16384.
 * All accumulators are integers or per-respondent double sums in draw order: neither the launch geometry nor the device
 * can change a bit of them, and two runs give bit-identical states.  Nothing is drawn: the chain is untouched under both
 * RNG contracts.  n <= GPIRT_RANK_MAX_N.
 * Pooling C chains (gpirt_rank_combine) adds the integers and adds the shares in chain order.  A chain with sign -1 (the
 * theta -> -theta reflection gpirt_chains_combine decided, or the caller's) is reflected EXACTLY first:
 *   rank2_sum -> S (2n + 2) - rank2_sum,  rank2_sumsq -> sum (2n + 2 - R2)^2 = S (2n + 2)^2 - 2 (2n + 2) rank2_sum + rank2_sumsq,
 *   rank_hist's bins reversed, pivot q <-> n + 1 - q, lt -> lt^T.  signs = NULL reflects nothing. */
#define GPIRT_RANK_MAX_PIVOTS         16      /* positions the caller may give */
#define GPIRT_RANK_MAX_PIVOTS_CLOSED  32      /* ... and their closure under q <-> n + 1 - q */
#define GPIRT_RANK_MAX_N              16384
/* HOST pointers (NULL: not wanted).  P = n_pivots on the way out (the closed set), B and w as above. */
typedef struct gpirt_ranks {
    const double* probs;          /* in: nprobs probabilities in [0, 1] for rank_q */
    int       nprobs;
    int       n_pivots;           /* in (gpirt_mcmc_run): the positions given in pivots[], 0 = the median; out: P */
    int64_t   pivots[GPIRT_RANK_MAX_PIVOTS_CLOSED];     /* in: the first n_pivots; out: the closed set, sorted */
    int       pairwise;           /* in (gpirt_mcmc_run): keep lt */
    int       reserved0;          /* must be 0 */
    double*   rank_mean;          /* n */
    double*   rank_var;           /* n */
    double*   rank_q;             /* nprobs x n */
    double*   p_pivot;            /* P x n */
    double*   pivot_share;        /* P x n */
    uint64_t* rank2_sum;          /* n */
    uint64_t* rank2_sumsq;        /* n */
    uint32_t* rank_hist;          /* n x B */
    uint32_t* pivot_cover;        /* P x n */
    uint32_t* lt;                 /* n x n (the states must hold the pairwise counters) */
    int64_t   draws, skipped, B, w;       /* out: counted and skipped draws (pooled: over the chains), the bins */
    double    rank_bin_width;             /* out: w / 2 */
    int64_t   reserved[4];        /* must be 0 */
} gpirt_ranks;
/* Stage API.  rank_enable(pivots, n_pivots, pairwise) allocates and zeroes the accumulators (pivots = NULL and
 * n_pivots < 0: frees them; n_pivots = 0: the median); more than GPIRT_RANK_MAX_PIVOTS positions or one outside 1..n is
 * GPIRT_E_ARG.  rank_accumulate adds the CURRENT theta as one draw (call it after the step of a sampling iteration).
 * rank_get copies one array by name to the host, `bytes` its exact size: "rank2_sum", "rank2_sumsq" (uint64, n),
 * "rank_hist" (uint32, n x B), "pivot_cover" (uint32, P x n), "pivot_share", "p_pivot" (double, P x n), "rank_mean",
 * "rank_var" (double, n), "pivots" (int64, P), "lt" (uint32, n x n, dense), "counts" (int64: draws, skipped, B, w, P).
 * rank_state returns the ONE device block, apart from the summaries' and the PPC's (valid until rank_enable is called again
 * or the sampler is destroyed): a header of 40 int64 -- n, counted draws, skipped draws, layout version (1), B, w, P, the
 * pairwise flag, then the closed pivots in 32 words -- then uint64 rank2_sum[n], rank2_sumsq[n], double pivot_share[P][n],
 * uint32 pivot_cover[P][n] and rank_hist[n][B] (each padded to 8 bytes) and, with the flag, on a 16-byte boundary uint32
 * lt[n][ld], ld = n rounded up to 4 (padding 0).  gpirt_rank_combine pools C such blocks (device pointers on h's device;
 * the same n and pivots; with out->lt every state must hold lt) into out, whose probs / nprobs it reads. */
int gpirt_sampler_rank_enable(gpirt_sampler_t s, const int64_t* pivots, int n_pivots, int pairwise);
int gpirt_sampler_rank_accumulate(gpirt_sampler_t s);
int gpirt_sampler_rank_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_rank_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_rank_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ranks* out);

/* ------------------------------------------------------ scoring new respondents: theta posterior and predictive density -- */
/* What does the fitted model say about a respondent who was NOT in the fit (library version 109)?  y_new is n_new x m,
 * column-major, coded +1 / -1 / NaN, over the SAME m item columns as the sampler's y (after unanimous items were dropped),
 * 1 <= n_new <= GPIRT_SCORE_MAX_N; any other value or size is GPIRT_E_ARG before anything is touched.  Per counted draw of
 * f* (which carries mu*) and new respondent r, with N = GPIRT_NGRID and theta*_k = -5 + 0.01 k:
 *   T[k, r]  = sum_j over observed cells of -log(1 + exp(-+ f*[k, j])), the product gpirt_debug_theta_logpost documents: in
 *     exact fixed point on the int8 matrix cores (with its own hand-over to the fp64 product when |f*| > 709 or f* is not
 *     finite), or with GPIRT_THETA_FIXED=2 as the fp64 GEMM.  In the fp64 form a term that overflows (the formula as
 *     written gives -inf for |f*| > ~709.8) is held at -1e300, which is finite.  A NaN cell f*[k, j] makes T[k, r] NaN for
 *     the respondents who answered item j and ONLY for them (the library keeps it out of the product and flags them).
 *   lp[k]    = logprior[k] + T[k, r], logprior[k] = log dnorm(theta*_k) = -(log sqrt(2 pi) + 0.5 theta*_k^2) as draw_theta adds it.
 *   M = max_k lp[k], Z = sum_k exp(lp[k] - M), w_k = exp(lp[k] - M) / Z: always stabilised, whatever theta_stabilise says.
 *   post_sum[r][k] += w_k: the Rao-Blackwellised grid posterior, the mean over draws of P(theta_new = theta*_k | f*, y_new).
 *   l = M + log Z - logsumexp_k(logprior): the log of sum_k pi_k prod_j P(y_rj | theta*_k) under the normalised grid prior pi.
 *   lpd_acc[r] = logaddexp(lpd_acc[r], l) (from -inf, as WAIC's lppd), ll_sum[r] += l, draws[r] += 1.
 * If any lp[k] of respondent r is not finite in a draw, that draw is skipped for r alone: nonfinite[r] += 1 and nothing
 * else of r changes.  A respondent with no observed cell has T = 0: its posterior is the prior and l = 0.
 * Finished on the host from the integers and sums (sums over k in k order; NaN where draws[r] = 0):
 *   grid_post = post_sum / draws[r];  theta_mean = sum_k theta*_k grid_post[k],  theta_sd = sqrt(sum_k (theta*_k - mean)^2
 *   grid_post[k]);  theta_quantiles[p] = the smallest grid point whose cumulative grid_post is >= probs[p] (the last one if
 *   none is);  theta_map = the lowest grid point of maximal grid_post;  lpd = lpd_acc - log draws[r];  loglik_mean =
 *   ll_sum / draws[r];  lpd_total = sum_r lpd,  se_lpd_total = sqrt(n_new var_r lpd) (ddof 1; NaN for n_new < 2).
 * Nothing is drawn: the chain, the IRFs and R's stream position are what they are without scoring, under both RNG
 * contracts.  All accumulators are per-respondent sums in draw order formed by one wave in a fixed order: two runs give
 * bit-identical states.
 * Pooling C chains (gpirt_score_combine) adds the counters, adds post_sum and ll_sum in chain order and combines lpd_acc by
 * logaddexp in chain order.  A chain with sign -1 (the theta -> -theta reflection gpirt_chains_combine decided, or the
 * caller's) enters with post_sum[r][k] <-> post_sum[r][1000 - k]; l is taken as it is (the prior is symmetric, so l does not
 * depend on the labelling).  signs = NULL reflects nothing. */
#define GPIRT_SCORE_MAX_N  16384
/* HOST pointers (NULL: not wanted). */
typedef struct gpirt_score {
    const double* probs;          /* in: nprobs probabilities in [0, 1] for theta_quantiles */
    int       nprobs;
    int       reserved0;          /* must be 0 */
    double*   grid_post;          /* n_new x GPIRT_NGRID (k fastest) */
    double*   theta_mean;         /* n_new */
    double*   theta_sd;           /* n_new */
    double*   theta_quantiles;    /* nprobs x n_new */
    double*   theta_map;          /* n_new */
    double*   lpd;                /* n_new */
    double*   loglik_mean;        /* n_new */
    double*   post_sum;           /* n_new x GPIRT_NGRID */
    double*   lpd_acc;            /* n_new */
    double*   ll_sum;             /* n_new */
    int64_t*  n_obs;              /* n_new */
    int64_t*  draws;              /* n_new */
    int64_t*  nonfinite;          /* n_new */
    int64_t   n_new, m;           /* out */
    double    lpd_total, se_lpd_total;    /* out */
    int64_t   reserved[4];        /* must be 0 */
} gpirt_score;
/* Stage API.  score_enable(h_y_new, n_new) packs y_new (a HOST array) and allocates the state (h_y_new = NULL or n_new = 0:
 * scoring off, the state freed).  score_accumulate adds the CURRENT f* as one draw (call it after the step of a sampling
 * iteration).  score_get copies one array by name to the host, `bytes` its exact size: "draws", "nonfinite", "n_obs" (int64,
 * n_new), "lpd_acc", "ll_sum", "lpd", "loglik_mean", "theta_mean", "theta_sd", "theta_map" (double, n_new), "post_sum",
 * "grid_post" (double, n_new x N) and "product" (double, N x n_new, k fastest: T of the last score_accumulate).
 * score_state returns the ONE device block, apart from the summaries', the PPC's and the ranks' (valid until score_enable is
 * called again or the sampler is destroyed): a header of 8 int64 -- n_new, m, layout version (1), N, 0, 0, 0, 0 -- then int64
 * draws[n_new], nonfinite[n_new], n_obs[n_new], double lpd_acc[n_new] (-inf before the first draw), ll_sum[n_new] and
 * post_sum[n_new][N].  gpirt_score_combine pools C such blocks (device pointers on h's device; the same n_new, m and
 * n_obs) into out, whose probs / nprobs it reads.  Item shards are refused by score_enable: a new respondent's product runs
 * over all items. */
int gpirt_sampler_score_enable(gpirt_sampler_t s, const double* h_y_new, int64_t n_new);
int gpirt_sampler_score_accumulate(gpirt_sampler_t s);
int gpirt_sampler_score_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_score_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_score_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_score* out);

/* ---------------------------------------------- predicting new respondents' unseen answers and ranking the next item to ask -- */
/* How would a respondent who was NOT in the fit answer item j, and which unanswered item is expected to say most about their
 * theta (library version 110)?  An add-on to scoring: it can only be enabled on a sampler whose score_enable is on, and it
 * accumulates inside the same score_accumulate call.  Both answers are joint functionals of ONE draw -- that draw's grid
 * weights times that draw's f* --, so neither grid_post nor the IRFs determine them; they are accumulated draw by draw without
 * storing f*.  With N = GPIRT_NGRID, theta*_k = -5 + 0.01 k and w_k respondent r's normalised weights of this draw exactly as
 * the scoring block above defines them:
 * Per cell f = f*[k, j], with a = |f|, e = exp(-a), l = log1p(e), s = e / (1 + e):
 *   P[k, j] = f >= 0 ? 1 / (1 + e) : s          plogis(f), stable in both tails
 *   H[k, j] = e == 0 ? 0 : l + a s              the binary entropy of P in nats: symmetric in f, log 2 at 0, exactly 0 once
 *                                               exp(-|f|) underflows (+-inf included)
 * Per draw and respondent r, for EVERY item j (the respondent's own answered items included; the caller masks what they like):
 *   q[r, j]    = sum_k w_k P[k, j]              P(y_rj = +1 | this draw, y_new[r, :])
 *   Hbar[r, j] = sum_k w_k H[k, j]
 *   g[r, j]    = h(q) - Hbar                    the mutual information between the unseen answer and theta_r under this draw;
 *                                               h(q) = -(q log q + (1 - q) log1p(-q)) with q clamped to [0, 1] for the entropy
 *                                               only and 0 log 0 = 0; g is NOT clamped (it is >= 0 up to rounding)
 *   pred_sum[r, j] += q,  info_sum[r, j] += g.
 * The two sums over k are one fp64 matrix-core product C (n_new x 2m) = W^T [P | H] in a fixed order.
 * A draw whose f* holds ANY NaN cell is skipped whole for prediction: pred_skipped += 1 and nothing else changes (scoring
 * itself still skips only the respondents who answered the marked item).  In a NaN-free draw every respondent's
 * log-posterior is finite (an overflowed term is held at -1e300), so ONE counter pred_draws serves all respondents.  +-inf
 * cells are fine: P is 0 or 1 and H is 0.
 * Finished on the host: p_yes = pred_sum / pred_draws, info = info_sum / pred_draws (nats), NaN everywhere if pred_draws = 0;
 * next_items[r, t], t < top (1 <= top <= GPIRT_PREDICT_MAX_TOP, the Python default is 5), holds r's UNANSWERED items by
 * decreasing info, ties to the lowest j (an item whose info is NaN is never listed), padded with -1; next_info[r, t] their
 * info, NaN where padded.
 * Pooling C chains (gpirt_score_predict_combine) adds pred_sum, info_sum, pred_draws and pred_skipped in chain order and
 * refuses blocks with another n_new, m or answered-mask.  The theta -> -theta reflection changes nothing here (both sums
 * run over the whole grid), so there is no signs argument.
 * Nothing is drawn: the chain, the IRFs, R's stream position and THE SCORE STATE BLOCK are bit for bit what they are without
 * prediction.  The accumulation order is fixed (each cell is owned by one thread, no atomics): two runs give bit-identical
 * states.  Item shards stay refused, as for score_enable.
 * Device memory per state: pred_sum and info_sum 16 n_new m bytes and the per-draw product C as much again, the per-draw
 * weights 8 Np n_new bytes (Np = 1024), the operand tables 16 Np m bytes: at n_new = 16384, m = 1024 about 268 MB + 268 MB +
 * 134 MB + 17 MB. */
#define GPIRT_PREDICT_MAX_TOP  16
/* HOST pointers (NULL: not wanted); every n_new x . array is column-major (r fastest), as y_new is. */
typedef struct gpirt_score_predict {
    int       top;                /* in: 1..GPIRT_PREDICT_MAX_TOP */
    int       reserved0;          /* must be 0 */
    double*   p_yes;              /* n_new x m */
    double*   info;               /* n_new x m */
    int64_t*  next_items;         /* n_new x top */
    double*   next_info;          /* n_new x top */
    double*   pred_sum;           /* n_new x m */
    double*   info_sum;           /* n_new x m */
    int64_t   n_new, m;           /* out */
    int64_t   pred_draws, pred_skipped;   /* out */
    int64_t   reserved[4];        /* must be 0 */
} gpirt_score_predict;
/* Stage API.  score_predict_enable(on != 0) allocates and zeroes the state on a sampler with score_enable on (GPIRT_E_ARG
 * without; on = 0 frees it; score_enable called again frees it too).  From then on every score_accumulate also adds the draw
 * to the prediction.  score_predict_get copies one array by name to the host, `bytes` its exact size: "pred_sum", "info_sum",
 * "p_yes", "info" (double, n_new x m), "counts" (int64: pred_draws, pred_skipped) and "weights" (double, N x n_new, k
 * fastest: W of the last draw that counted).  score_predict_state returns the ONE device block, apart from the score block:
 * a header of 8 int64 -- n_new, m, layout version (1), N, pred_draws, pred_skipped, 0, the tag 0x44455250 ("PRED": a score
 * block's header starts alike) --, the answered-mask of y_new
 * packed 64 cells a word (cell g = r + j n_new: bit g % 64 of word g / 64; ceil(n_new m / 64) words), then double
 * pred_sum[m][n_new] and info_sum[m][n_new]. */
int gpirt_sampler_score_predict_enable(gpirt_sampler_t s, int on);
int gpirt_sampler_score_predict_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_score_predict_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_score_predict_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_score_predict* out);

/* ------------------------------------------------------------- pairwise item checks: joint counts and odds ratios of item pairs -- */
/* Does the model's one latent dimension hold (library version 111)?  Given theta, answers to different items are independent;
 * a second dimension or a pair of near-duplicate items leaves every item's yes count well replicated and shows only in how
 * items co-occur.  The check is the posterior predictive distribution of each item pair's 2 x 2 table and of its odds ratio.
 * An add-on to the PPC: it can only be enabled on a sampler whose ppc_enable is on, and it accumulates inside the same
 * ppc_accumulate call, from the same replicate.  With n respondents and m items:
 *   O[i, j]   = 1 where y_ij is observed
 *   Y[i, j]   = [y_ij = +1]
 *   rep[i, j] = [yrep_ij = +1] O[i, j], yrep EXACTLY the replicate ppc_accumulate forms for that draw: the same p arithmetic
 *               and the same uniform item_uniform(seed, iter, GPIRT_ST_PPC, item0 + j, i).  No second stream, nothing else drawn.
 * Constants, formed once at enable: n_co = O^T O, o11 = Y^T Y, o1 = Y^T O.  Per draw: r11 = rep^T rep, r1 = rep^T O.  All are
 * m x m and exact int32 counts (products of 0 / 1 bytes on the int8 matrix cores).
 * For x in {o, r} the 2 x 2 table of the pair (a, b), a != b, over the co-observed respondents is
 *   t11 = x11[a, b],  t10 = x1[a, b] - x11[a, b],  t01 = x1[b, a] - x11[a, b],  t00 = n_co[a, b] - t11 - t10 - t01.
 * Per COUNTED draw and ordered pair with n_co > 0, everything in integers:
 *   sum_n11 += r11,  sumsq_n11 += r11^2,  sum_n1[a, b] += r1[a, b] (not symmetric)                    uint64
 *   n11_ge / n11_gt     += [r11 >= / > o11]                                                           uint32
 *   agree_ge / agree_gt += [r11 + r00 >= / > o11 + o00]
 *   or_ge / or_gt       += [lhs >= / > rhs], the odds ratios with the half-count correction compared by cross-multiplication,
 *                          without a division:  lhs = (2 r11 + 1)(2 r00 + 1)(2 o10 + 1)(2 o01 + 1),
 *                                               rhs = (2 o11 + 1)(2 o00 + 1)(2 r10 + 1)(2 r01 + 1);
 *                          both are <= (n + 1)^4, exact in uint64 for n <= GPIRT_PAIRS_MAX_N = 65534 (ppc_pairs_enable returns
 *                          GPIRT_E_ARG above that).
 * The diagonal and the pairs with n_co = 0 keep every counter at 0 and finish as NaN (n_co itself is reported everywhere).
 * A draw with a non-finite g in ANY observed cell is skipped whole for the pairs: pair_skipped += 1 and nothing else changes
 * (as pred_skipped works); the PPC's own per-unit `nonfinite` rule is untouched.  Otherwise pair_draws += 1.
 * Finished on the host as m x m doubles, pair (a, b) at [a m + b], with S = pair_draws (GPIRT_PAIRS_* below):
 *   n_co; obs_n11, obs_n10, obs_n01, obs_n00;
 *   rep_n11_mean = sum_n11 / S and rep_n11_var = (S sumsq_n11 - sum_n11^2) / (S (S - 1)), the numerator in exact integers,
 *   rounded once (NaN for S < 2);
 *   rep_n10_mean, rep_n01_mean, rep_n00_mean: (sum_n1[a, b] - sum_n11) / S, (sum_n1[b, a] - sum_n11) / S and
 *   (S n_co + sum_n11 - sum_n1[a, b] - sum_n1[b, a]) / S, each numerator an exact integer;
 *   agree_obs = (o11 + o00) / n_co and agree_rep_mean = (S n_co + 2 sum_n11 - sum_n1[a, b] - sum_n1[b, a]) / (S n_co);
 *   log_or_obs = log(((2 o11 + 1)(2 o00 + 1)) / ((2 o10 + 1)(2 o01 + 1))): one division of two exact integers, one log;
 *   ppp_n11, ppp_agree, ppp_or = ge / S and their mid-p forms ppp_*_mid = (ge + gt) / 2S.  Everything NaN for S = 0.
 *   extreme: the `top` pairs a < b by decreasing |ppp_or_mid - 0.5|, ties to the lowest (a, b) (a pair whose ppp_or_mid is NaN
 *   is never listed); 1 <= top <= GPIRT_PAIRS_MAX_TOP, the Python default is 20: their indices, ppp_or_mid and log_or_obs,
 *   padded with -1 / NaN.
 * Pooling C chains (gpirt_ppc_pairs_combine) adds every array and both counters and refuses blocks with another n, m or
 * n_co (o11 and o1 are compared too).  The theta -> -theta reflection changes nothing, so there is no signs argument.
 * There are no atomics: each ordered pair is owned by one thread, so two runs give a bit-identical state.  Nothing is drawn:
 * the chain, the IRFs, R's stream position and THE PPC STATE BLOCK are bit for bit what they are without the pairs.  Item
 * shards stay refused, as for ppc_enable.
 * Device memory per state: 48 bytes of accumulators per ordered pair (3 uint64 + 6 uint32), 12 of constants and 8 of per-draw
 * tables: about 71 MB at m = 1024 and 1.1 GB at m = 4096.  The n x m int8 operands are extra: O, Y and two planes of rep,
 * padded to 128 items and 256 respondents (34 MB at 8192 x 1024). */
#define GPIRT_PAIRS_MAX_TOP  64
#define GPIRT_PAIRS_MAX_N    65534
#define GPIRT_PAIRS_N_CO            0
#define GPIRT_PAIRS_OBS_N11         1
#define GPIRT_PAIRS_OBS_N10         2
#define GPIRT_PAIRS_OBS_N01         3
#define GPIRT_PAIRS_OBS_N00         4
#define GPIRT_PAIRS_REP_N11_MEAN    5
#define GPIRT_PAIRS_REP_N11_VAR     6
#define GPIRT_PAIRS_REP_N10_MEAN    7
#define GPIRT_PAIRS_REP_N01_MEAN    8
#define GPIRT_PAIRS_REP_N00_MEAN    9
#define GPIRT_PAIRS_AGREE_OBS       10
#define GPIRT_PAIRS_AGREE_REP_MEAN  11
#define GPIRT_PAIRS_LOG_OR_OBS      12
#define GPIRT_PAIRS_PPP_N11         13
#define GPIRT_PAIRS_PPP_N11_MID     14
#define GPIRT_PAIRS_PPP_AGREE       15
#define GPIRT_PAIRS_PPP_AGREE_MID   16
#define GPIRT_PAIRS_PPP_OR          17
#define GPIRT_PAIRS_PPP_OR_MID      18
#define GPIRT_PAIRS_NFIELDS         19
/* HOST pointers (NULL: not wanted); every m x m array holds the pair (a, b) at [a m + b]. */
typedef struct gpirt_ppc_pairs {
    int        top;                            /* in: 1..GPIRT_PAIRS_MAX_TOP */
    int        reserved0;                      /* must be 0 */
    double*    field[GPIRT_PAIRS_NFIELDS];     /* m x m each */
    uint64_t*  sum_n11;                        /* m x m */
    uint64_t*  sumsq_n11;
    uint64_t*  sum_n1;
    uint32_t*  count[6];                       /* m x m each: n11_ge, n11_gt, agree_ge, agree_gt, or_ge, or_gt */
    int64_t*   extreme_pairs;                  /* top x 2: a, b */
    double*    extreme_ppp_or_mid;             /* top */
    double*    extreme_log_or_obs;             /* top */
    int64_t    n, m;                           /* out */
    int64_t    pair_draws, pair_skipped;       /* out */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_ppc_pairs;
/* Stage API.  ppc_pairs_enable(on != 0) allocates and zeroes the state on a sampler with ppc_enable on (GPIRT_E_ARG without,
 * and for n > GPIRT_PAIRS_MAX_N; on = 0 frees it; ppc_enable called again frees it too) and forms the constants.  From then on
 * every ppc_accumulate also adds the draw to the pairs.  ppc_pairs_get copies one array by name to the host, `bytes` its exact
 * size: every finished field by the lower-case name of its GPIRT_PAIRS_* index (double, m x m), "sum_n11", "sumsq_n11",
 * "sum_n1" (uint64), "n11_ge", "n11_gt", "agree_ge", "agree_gt", "or_ge", "or_gt" (uint32), "counts" (int64: pair_draws,
 * pair_skipped), and of the last COUNTED draw "rep" (int8, n x m, column-major as y is) and "r11", "r1" (int32, m x m).
 * ppc_pairs_state returns the ONE device block, apart from the PPC block: a header of 8 int64 -- n, m, layout version (1),
 * pair_draws, pair_skipped, item0, 0, the tag 0x52494150 ("PAIR") --, then the constant tables int32 n_co, o11, o1, then the
 * accumulators uint64 sum_n11, sumsq_n11, sum_n1 and uint32 n11_ge, n11_gt, agree_ge, agree_gt, or_ge, or_gt; every array is
 * m x m and starts on a 16-byte boundary. */
int gpirt_sampler_ppc_pairs_enable(gpirt_sampler_t s, int on);
int gpirt_sampler_ppc_pairs_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ppc_pairs_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_ppc_pairs_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_pairs* out);

/* ------------------------------------------------------------- theta-binned item fit: empirical IRFs and chi-square per item -- */
/* Does an item's response function have the right SHAPE along theta (library version 112)?  An item's yes count is reproduced by
 * almost any model with an intercept; whether the curve is right in the tails shows only when the respondents are grouped by
 * where a draw puts them on the theta axis and, group by group, the yes answers are compared with what the model expects there
 * (Yen's Q1 / Orlando and Thissen's S-X2 as posterior predictive discrepancies, Sinharay 2006).  An add-on to the PPC as the
 * pairs are: enabled on a sampler whose ppc_enable is on, accumulated inside the same ppc_accumulate call from the same
 * replicate; O, Y and rep as in the pairs section, p the PPC's p = plogis(g), q = plogis(-g) by the same arithmetic with the
 * branches swapped (e = exp(-|g|); g >= 0: p = 1 / (1 + e), q = e / (1 + e); else p = e / (1 + e), q = 1 / (1 + e)).
 * Cuts and bins.  The cuts are h integers 1 <= d_1 < ... < d_h <= 499, 1 <= h <= GPIRT_BINS_MAX_H = 15: hundredths of theta,
 * the positive cut points.  They give B = 2h + 1 <= 31 bins.  A respondent whose theta is the grid point k (bit for bit
 * -5 + 0.01 k, the rule of the rank posteriors and the theta histograms) has a = |k - 500|, l = #{t : a >= d_t} and
 *   bin = h + l if k >= 500, else h - l.
 * Bin h is the centre bin |theta| < d_1 / 100; theta -> -theta maps bin b to B - 1 - b exactly.  The Python default is
 * (14, 43, 76, 122): nine bins of equal N(0, 1) probability, snapped to the grid.
 * Per draw and (bin b, item j), over the cells i in b with y_ij observed: the exact integers N = #cells, T = #{y = +1},
 * R = #{rep = 1} and, in fp64, E = sum p_ij, V = sum p_ij q_ij; n_b = #{i in b}.
 * Per COUNTED draw:
 *   cell (b, j) with N > 0:  cell_ge / cell_gt += [R >= / > T] (uint32); sum_N, sum_T, sum_R += N, T, R (uint64); sum_E += E;
 *                            sum_z += (T - E) / sqrt(V), added only where V > 0 (double);
 *                with N = 0: cell_empty += 1 (uint32) and nothing else;
 *   item j:  X2(C) = sum_b ((double)C_b - E_b)^2 / V_b over the bins with N_b > 0 and V_b > 0, summed in increasing b.
 *            If R_b = T_b in every bin -- decided on the integers, before any floating point -- the draw counts in chi_ge and
 *            not in chi_gt; otherwise chi_ge / chi_gt += [X2(R) >= / > X2(T)] (uint32).  chi_obs_sum += X2(T),
 *            chi_rep_sum += X2(R) (double), in every counted draw;
 *   bin b:   occ_sum[b] += n_b (uint64).
 * A draw is skipped whole for the bins when any theta is off the grid (NaN included) or g is non-finite in any observed cell:
 * bin_skipped += 1 and nothing else changes; any other draw adds 1 to bin_draws.  The PPC's and the pairs' own rules are
 * untouched.
 * Finished on the host with S = bin_draws, B x m arrays with cell (b, j) at [b m + j] (GPIRT_BINS_CELL_*):
 *   obs_rate = sum_T / sum_N (the empirical IRF), rep_rate = sum_R / sum_N, exp_rate = sum_E / sum_N,
 *   z_mean = sum_z / (S - cell_empty), ppp_cell = cell_ge / (S - cell_empty), ppp_cell_mid = (cell_ge + cell_gt) / 2 (S - cell_empty),
 *   n_mean = sum_N / S;
 * per item (GPIRT_BINS_ITEM_*): ppp_chi2 = chi_ge / S, ppp_chi2_mid = (chi_ge + chi_gt) / 2S, chi2_obs_mean = chi_obs_sum / S,
 * chi2_rep_mean = chi_rep_sum / S; per bin (GPIRT_BINS_BIN_*): occupancy = occ_sum / S and the bin's edges in theta bin_lo,
 * bin_hi (bin h + l, l >= 1: [d_l, d_(l+1)) / 100 with the last one closed at 5; bin h - l its mirror image; the centre bin
 * (-d_1, d_1) / 100).  Everything is NaN where its denominator is 0.
 *   worst: the `top` (1..GPIRT_BINS_MAX_TOP, the Python default is 20) items by increasing ppp_chi2_mid, ties to the lowest j,
 *   NaN never listed: their indices, ppp_chi2_mid and chi2_obs_mean, padded with -1 / NaN.
 * Determinism: no floating-point atomics; every double is reduced in a fixed order (the 64 rows of a wave in row order, the four
 * waves of a 256-row block in order, the row blocks in order, the bins in increasing b), so two runs give a bit-identical state
 * block.  The only atomics are integer LDS (vector) atomics that count n_b.
 * Pooling C chains (gpirt_ppc_bins_combine) adds the integers and adds the doubles in chain order; a chain with sign -1 enters
 * with its bin axis reversed (cell (b, j) as (B - 1 - b, j), occ_sum too), which is exact by the symmetry above.  signs = NULL:
 * all +1.  Blocks with another n, m, item0 or cuts are refused.
 * Nothing is drawn: with the bins on, the chain, the IRFs, R's stream position, the PPC state block and the pairs state block are
 * bit for bit what they are without.  Item shards stay refused, as for ppc_enable.
 * Device memory per state: 52 B m bytes of accumulators, 28 B m of the last draw's tables and 20 B m per block of 256
 * respondents of per-draw partial tables (at 8192 x 1024: 0.7 MB + 5.9 MB for B = 9, 2.5 MB + 20 MB for B = 31). */
#define GPIRT_BINS_MAX_H     15
#define GPIRT_BINS_MAX_B     31
#define GPIRT_BINS_MAX_TOP   64
#define GPIRT_BINS_CELL_OBS_RATE       0
#define GPIRT_BINS_CELL_REP_RATE       1
#define GPIRT_BINS_CELL_EXP_RATE       2
#define GPIRT_BINS_CELL_Z_MEAN         3
#define GPIRT_BINS_CELL_PPP_CELL       4
#define GPIRT_BINS_CELL_PPP_CELL_MID   5
#define GPIRT_BINS_CELL_N_MEAN         6
#define GPIRT_BINS_CELL_NFIELDS        7
#define GPIRT_BINS_ITEM_PPP_CHI2       0
#define GPIRT_BINS_ITEM_PPP_CHI2_MID   1
#define GPIRT_BINS_ITEM_CHI2_OBS_MEAN  2
#define GPIRT_BINS_ITEM_CHI2_REP_MEAN  3
#define GPIRT_BINS_ITEM_NFIELDS        4
#define GPIRT_BINS_BIN_OCCUPANCY       0
#define GPIRT_BINS_BIN_LO              1
#define GPIRT_BINS_BIN_HI              2
#define GPIRT_BINS_BIN_NFIELDS         3
/* HOST pointers (NULL: not wanted). */
typedef struct gpirt_ppc_bins {
    int        top;                            /* in: 1..GPIRT_BINS_MAX_TOP */
    int        h;                              /* in (gpirt_mcmc_run): the number of cuts; out: the states' */
    int        cuts[GPIRT_BINS_MAX_H + 1];     /* in (gpirt_mcmc_run) / out: d_1 .. d_h, the rest 0 */
    double*    cell[GPIRT_BINS_CELL_NFIELDS];  /* B x m each */
    double*    item[GPIRT_BINS_ITEM_NFIELDS];  /* m each */
    double*    bin[GPIRT_BINS_BIN_NFIELDS];    /* B each */
    uint64_t*  sum_n;                          /* B x m */
    uint64_t*  sum_t;
    uint64_t*  sum_r;
    double*    sum_e;
    double*    sum_z;
    uint32_t*  cell_count[3];                  /* B x m each: cell_ge, cell_gt, cell_empty */
    uint32_t*  chi_count[2];                   /* m each: chi_ge, chi_gt */
    double*    chi_obs_sum;                    /* m */
    double*    chi_rep_sum;
    uint64_t*  occ_sum;                        /* B */
    int64_t*   worst_items;                    /* top */
    double*    worst_ppp_chi2_mid;             /* top */
    double*    worst_chi2_obs_mean;            /* top */
    int64_t    n, m, B;                        /* out */
    int64_t    bin_draws, bin_skipped;         /* out */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_ppc_bins;
/* Stage API.  ppc_bins_enable(h, cuts, on != 0) allocates and zeroes the state on a sampler with ppc_enable on (GPIRT_E_ARG
 * without, and for cuts that break the rule above; on = 0 frees it, cuts may then be NULL; ppc_enable called again frees it too).
 * From then on every ppc_accumulate also adds the draw to the bins.  ppc_bins_get copies one array by name to the host, `bytes`
 * its exact size: every finished array by the lower-case name above (double; B x m, m or B), "cuts" (int64, h), the raw
 * "sum_n", "sum_t", "sum_r", "occ_sum" (uint64), "sum_e", "sum_z", "chi_obs_sum", "chi_rep_sum" (double), "cell_ge", "cell_gt",
 * "cell_empty", "chi_ge", "chi_gt" (uint32), "counts" (int64: bin_draws, bin_skipped) and, of the last COUNTED draw, "bin"
 * (uint8, n), "tN", "tT", "tR" (int32, B x m) and "tE", "tV" (double, B x m).
 * ppc_bins_state returns the ONE device block, apart from the PPC's and the pairs': a header of 8 int64 -- n, m, layout version
 * (1), bin_draws, bin_skipped, item0, B, the tag 0x534E4942 ("BINS") --, then 16 int64 that hold the cuts d_1 .. d_h (the rest
 * 0), then uint64 sum_n, sum_t, sum_r, double sum_e, sum_z, uint32 cell_ge, cell_gt, cell_empty (B x m each), uint32 chi_ge,
 * chi_gt, double chi_obs_sum, chi_rep_sum (m each) and uint64 occ_sum (B); every array starts on a 16-byte boundary. */
int gpirt_sampler_ppc_bins_enable(gpirt_sampler_t s, int h, const int* cuts, int on);
int gpirt_sampler_ppc_bins_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ppc_bins_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_ppc_bins_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ppc_bins* out);

/* ------------------------------------------------------ IRF shape posteriors: monotonicity, peaks, information --------- */
/* The posterior mean curve and its pointwise bands do not say what SHAPE an item's response curve has: whether it is monotone,
 * where it peaks, where it crosses P = 1/2, how steep it is, how much Fisher information it carries.  Those are joint
 * functionals of one curve in one draw.  The stored f* is white noise around the draw's smooth curve (draw_fstar draws every
 * grid point independently about the conditional mean), so the curve of a draw is that mean itself,
 *   g[k, j] = (k*^T S^-1 f)[k, j] + mu*[k, j],   k = 0 .. 1000 (theta_k = -5 + 0.01 k),
 * the one fp64 sum draw_fstar's epilogue forms anyway.  With the shape accumulators on, the epilogue also stores it in the
 * sampler array "gbar" (N x m, leading dimension 1001; gpirt_sampler_get / _set / _devptr know it): the mu* that draw_fstar
 * used, not the one draw_beta leaves later in the step.
 * The window W = [k_lo, k_hi] = [500 - k_half, 500 + k_half], 1 <= k_half <= 500, is symmetric about theta = 0.  Per draw and
 * item j, all in fp64 on the same g:
 *   extremes   kmax / kmin = argmax / argmin of g over W, the lowest k on ties (+0 and -0 tie): peak_hist[kmax, j] += 1,
 *              valley_hist[kmin, j] += 1;
 *   monotone   DD = max over k <= l in W of g[k] - g[l] (the largest fall: prefix max minus g, maximised), DU = max over
 *              k <= l in W of g[l] - g[k] (the largest rise); both are >= 0 and, being max, min and ONE subtraction, have the
 *              same bits in any evaluation order.  For each of the n_tols <= GPIRT_SHAPE_MAX_TOLS tolerances t >= 0 (logits) the
 *              draw is GPIRT_SHAPE_CLS_FLAT (DD <= t and DU <= t), _INCREASING (DD <= t < DU), _DECREASING (DU <= t < DD) or
 *              _NONMONOTONE (both > t): cls[t, class, j] += 1;
 *   crossings  sgn(x) = (x >= 0); c = #{k in [k_lo, k_hi - 1] : sgn(g[k]) != sgn(g[k + 1])}; cross_count[min(c, 3), j] += 1 and,
 *              for c >= 1, cross_first_hist[k, j] += 1 at the lowest such k and cross_last_hist[k, j] += 1 at the highest;
 *   slopes     d_k = g[k + 1] - g[k], k in [k_lo, k_hi - 1]; slope_max = (max d_k) / 0.01, slope_min = (min d_k) / 0.01; their
 *              sums and sums of squares per item in draw order (slope[0..3, j]: max sum, max sumsq, min sum, min sumsq);
 *   information, over the WHOLE grid: I[k, j] = (e / ((1 + e) (1 + e))) (g' g'), e = exp(-|g[k]|),
 *              g' = (g[k + 1] - g[k - 1]) / 0.02, at the ends (g[1] - g[0]) / 0.01 and (g[1000] - g[999]) / 0.01;
 *              info_sum[k, j] += I.
 * An item whose column holds ANY non-finite g (inside W or not) is skipped for that draw in all of the above: nonfinite[j] += 1;
 * otherwise draws[j] += 1.
 * Per draw, over all items: TI[k] = sum_j I[k, j] in ascending j; ti_sum[k] += TI, ti_sumsq[k] += TI TI; the marginal
 * reliability rho = sum_k w_k TI_k / (TI_k + 1) (prior variance 1), w_k = exp(-theta_k theta_k / 2) / sum of the same with
 * theta_k the double -5 + 0.01 k, the sum in ascending k; rho is reduced in a fixed order (lane t of 256 adds its terms
 * k = 4t .. 4t + 3 in order, the 256 partial sums are added in ascending t); rel[0] += rho, rel[1] += rho rho.  A draw in which any item
 * was skipped adds 1 to info_skipped and nothing to ti_sum, ti_sumsq and rel; any other adds 1 to info_draws.
 * Every accumulator cell is owned by one thread: no atomics, a fixed order, bit-identical state blocks from run to run.
 * Arrays indexed [k, j] are stored item-major: cell (k, j) at [j 1001 + k].  cls is [GPIRT_SHAPE_MAX_TOLS][4][m] (the slots
 * beyond n_tols stay 0), cross_count [4][m], slope [4][m].
 * Pooling C chains (gpirt_shape_combine) adds the integers and adds the doubles in chain order.  A chain with sign -1 (theta ->
 * -theta) is reflected ON ITS ACCUMULATORS, exactly because W is symmetric: the k axis of the four histograms, of info_sum,
 * ti_sum and ti_sumsq is reversed (k -> 1000 - k; the crossing histograms hold pair indices: k -> 999 - k), cross_first_hist
 * and cross_last_hist swap, increasing and decreasing swap, (slope_max, slope_min) becomes (-slope_min, -slope_max) (sums
 * negated and swapped, sums of squares swapped), rel is kept.  The argmax / argmin tie rule (the lowest k) is applied BEFORE the
 * reflection: a reflected chain's tied draw lands on the mirror image of its lowest tied k, not on the lowest tied k of the
 * mirrored curve.  signs = NULL: all +1.  Blocks with another m, k_half or other tolerances are refused.
 * Nothing is drawn: with the accumulators on, the chain, the IRFs, R's stream position and every other block's state are bit for
 * bit what they are without.
 * Device memory per state at m = 1024: four uint32 histograms and info_sum, 24 MB, plus 8 MB each for gbar and the draw's I. */
#define GPIRT_SHAPE_MAX_TOLS          4
#define GPIRT_SHAPE_CLS_FLAT          0
#define GPIRT_SHAPE_CLS_INCREASING    1
#define GPIRT_SHAPE_CLS_DECREASING    2
#define GPIRT_SHAPE_CLS_NONMONOTONE   3
/* the raw arrays of a state block, in the block's order */
#define GPIRT_SHAPE_CLS               0       /* uint32 [4][4][m] */
#define GPIRT_SHAPE_PEAK_HIST         1       /* uint32 [m][1001] */
#define GPIRT_SHAPE_VALLEY_HIST       2
#define GPIRT_SHAPE_CROSS_FIRST_HIST  3
#define GPIRT_SHAPE_CROSS_LAST_HIST   4
#define GPIRT_SHAPE_CROSS_COUNT       5       /* uint32 [4][m] */
#define GPIRT_SHAPE_DRAWS             6       /* uint32 [m] */
#define GPIRT_SHAPE_NONFINITE         7       /* uint32 [m] */
#define GPIRT_SHAPE_SLOPE             8       /* double [4][m] */
#define GPIRT_SHAPE_INFO_SUM          9       /* double [m][1001] */
#define GPIRT_SHAPE_TI_SUM            10      /* double [1001] */
#define GPIRT_SHAPE_TI_SUMSQ          11      /* double [1001] */
#define GPIRT_SHAPE_REL               12      /* double [2]: sum rho, sum rho^2 */
#define GPIRT_SHAPE_NARRAYS           13
/* HOST pointers (NULL: not wanted): the pooled raw arrays, each of the size and type named above. */
typedef struct gpirt_shape {
    int        k_half;                         /* in (gpirt_mcmc_run): 1..500; out: the states' */
    int        n_tols;                         /* in (gpirt_mcmc_run): 1..GPIRT_SHAPE_MAX_TOLS; out: the states' */
    double     tols[GPIRT_SHAPE_MAX_TOLS];     /* in (gpirt_mcmc_run) / out: the first n_tols, each >= 0 and finite */
    void*      raw[GPIRT_SHAPE_NARRAYS];
    int64_t    n, m;                           /* out */
    int64_t    info_draws, info_skipped;       /* out */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_shape;
/* Stage API.  shape_enable(k_half, tols, n_tols, on != 0) allocates and zeroes the state and the "gbar" array (GPIRT_E_ARG with a
 * message for k_half outside 1..500, n_tols outside 1..GPIRT_SHAPE_MAX_TOLS, a negative or non-finite tolerance; on = 0 frees
 * both, tols may then be NULL).  "gbar" holds a curve from the next draw_fstar on (zeros until then).  shape_accumulate adds the
 * CURRENT gbar as one draw (call it after the step of a sampling iteration).  shape_get copies one array by name to the host,
 * `bytes` its exact size: the lower-case names of the raw arrays ("cls", "peak_hist", "valley_hist", "cross_first_hist",
 * "cross_last_hist", "cross_count", "draws", "nonfinite", "slope", "info_sum", "ti_sum", "ti_sumsq", "rel"), "counts" (int64:
 * info_draws, info_skipped), "tols" (double, GPIRT_SHAPE_MAX_TOLS) and, of the last draw, "info" (double [m][1001], stale for
 * a skipped item) and "ti" (double [1001], stale after a skipped draw).
 * shape_state returns the ONE device block (valid until shape_enable is called again or the sampler goes): a header of 16 int64
 * -- the tag 0x50414853 ("SHAP"), the layout version (1), n, m, k_half, n_tols, the four tolerances' bits, info_draws,
 * info_skipped, 0, 0, 0, 0 -- then the raw arrays in the order above, every array starting on a 16-byte boundary;
 * gpirt_shape_state_bytes gives its size. */
int gpirt_sampler_shape_enable(gpirt_sampler_t s, int k_half, const double* tols, int n_tols, int on);
int gpirt_sampler_shape_accumulate(gpirt_sampler_t s);
int gpirt_sampler_shape_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_shape_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_shape_state_bytes(int64_t m, int64_t* bytes);
int gpirt_shape_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_shape* out);

/* ------------------------------------------------------ Sum-score posteriors: score table, TCC, reliability ------------ */
/* Everything above looks at one item, a pair of items or one respondent with a known answer pattern.  The statistic an IRT user
 * meets first is the SUM SCORE S = the number of yes answers on a set of items: which score distribution the model implies,
 * what theta is given only that somebody scored s, the expected score along theta (the test characteristic curve, TCC), how
 * reliable the score is.  Each is a joint functional of ALL items' curves in one draw (the score given theta is a
 * Poisson-binomial over the items; forming it from the mean curves gives the wrong spread: a mean of a product is not a
 * product of means), and none can be had by enumerating answer patterns beyond some twenty items.  Library version 114.
 * A FORM is a non-empty set of item columns: all m, or those a mask of m bytes names; M is its size, 1 <= M <=
 * GPIRT_SUMSCORE_MAX_ITEMS.  Per draw, over the grid theta*_k = -5 + 0.01 k (k = 0 .. 1000), from the draw's f* (N x m, carrying
 * mu*), the form's items taken in ascending column j, all in fp64:
 *   p[k, j] = 1 / (1 + exp(-f*[k, j])),  q[k, j] = 1 / (1 + exp(+f*[k, j])): each formed on its own, q is never 1 - p, so that
 *             both keep their relative accuracy in the tails; f* = +-inf gives exactly 0 and 1 (so does |f*| = 800: exp overflows
 *             to inf, 1 / inf = 0);
 *   A[k, .]   starts as A[k, 0] = 1, A[k, s > 0] = 0; for each item A[k, s] <- A[k, s] q + A[k, s - 1] p (two products, one sum).
 *             The result is A[k, s] = P(S = s | theta*_k, this draw), s = 0 .. M (the Lord-Wingersky recursion);
 *   w_k       the N(0, 1) density on the grid, normalised: theta_k the double -5 + 0.01 k, exp(-theta_k theta_k / 2) and the sum
 *             (ascending k) in long double on the host, the quotient rounded ONCE to double and stored in the state;
 *   pi[s]     = sum_k w_k A[k, s], ascending k: the draw's score distribution for a N(0, 1) population;
 *   T[k]      = sum_j p[k, j] (the TCC), V[k] = sum_j p[k, j] q[k, j] (the score's variance at theta_k), ascending j;
 *   rho       = 1 - (sum_k w_k V[k]) / (sum_k w_k (V[k] + T[k] T[k]) - (sum_k w_k T[k])^2), the three sums in ascending k: the
 *             reliability of the sum score, the model-based counterpart of Cronbach's alpha.
 * A draw whose f* holds a NaN in a form column is skipped WHOLE (`skipped` += 1, nothing else changes; the decision is made on
 * the device before anything is touched); a NaN in a column outside the form is ignored.  Every other draw adds 1 to `draws`.  A
 * counted draw whose total variance (rho's denominator) is not > 0 adds nothing to rel and 1 to `rel_skipped`; any other adds 1
 * to `rel_draws`.
 * The accumulators:
 *   joint_sum[k, s] += w_k A[k, s]       (1001 x (M + 1), cell (k, s) at [k (M + 1) + s])
 *   pi_sum[s] += pi[s], pi_sumsq[s] += pi[s] pi[s];  tcc_sum[k] += T[k], tcc_sumsq[k] += T[k] T[k], var_sum[k] += V[k];
 *   rel[0] += rho, rel[1] += rho rho;  last = A and last_pi = pi of the last counted draw.
 * THE JOINT, NOT THE RATIO.  For somebody new with theta ~ N(0, 1) of whom only the score s is known,
 * p(theta_k | s, data) is proportional to E_draws[w_k A[k, s]]: the block keeps the joint and it is normalised ONCE at the end.
 * This differs on purpose from the scorer above, which keeps the mean of per-draw normalised posteriors.  Nothing is normalised
 * per draw, and pooling chains is plain addition.
 * NO RESCALING.  Every A[k, s] is a sum of non-negative products of factors <= 1, and a partial product is never smaller than a
 * final one: whatever underflows on the way belongs to a probability below the smallest normal double.  There is no cancellation
 * anywhere, so the error is relative (a few M eps) plus an absolute floor of (M + 1) 2^-1021.
 * Every accumulator cell is owned by one thread: no atomics, a fixed order, bit-identical state blocks from run to run.
 * Pooling C chains (gpirt_sumscore_combine) adds the doubles and the counters in chain order.  A chain with sign -1 (theta ->
 * -theta) enters with the k axis of joint_sum, tcc_sum, tcc_sumsq, var_sum (and last) reversed; pi_sum, pi_sumsq and rel are kept
 * as they are (a reflected chain's sums over k ran in the other order; as with the shape posteriors they are not redone).  last
 * and last_pi are the last state's.  signs = NULL: all +1.  States with another m, another form or other grid weights are
 * refused.
 * Nothing is drawn: with the accumulators on, the chain, the IRFs, R's stream position and every other block's state are bit for
 * bit what they are without.
 * Device memory per state at M = 1024: joint_sum and last 8.2 MB each, the draw's (p, q) table 16.4 MB. */
#define GPIRT_SUMSCORE_MAX_ITEMS      4096
/* the raw arrays of a state block, in the block's order */
#define GPIRT_SUMSCORE_JOINT_SUM      0       /* double [1001][M + 1] */
#define GPIRT_SUMSCORE_PI_SUM         1       /* double [M + 1] */
#define GPIRT_SUMSCORE_PI_SUMSQ       2       /* double [M + 1] */
#define GPIRT_SUMSCORE_TCC_SUM        3       /* double [1001] */
#define GPIRT_SUMSCORE_TCC_SUMSQ      4       /* double [1001] */
#define GPIRT_SUMSCORE_VAR_SUM        5       /* double [1001] */
#define GPIRT_SUMSCORE_REL            6       /* double [2]: sum rho, sum rho^2 */
#define GPIRT_SUMSCORE_MASK           7       /* unsigned char [m]: 1 where the item is in the form */
#define GPIRT_SUMSCORE_W              8       /* double [1001]: the grid weights */
#define GPIRT_SUMSCORE_LAST           9       /* double [1001][M + 1] */
#define GPIRT_SUMSCORE_LAST_PI        10      /* double [M + 1] */
#define GPIRT_SUMSCORE_NARRAYS        11
/* HOST pointers (NULL: not wanted): the pooled raw arrays, each of the size and type named above. */
typedef struct gpirt_sumscore {
    const unsigned char* items;                /* in (gpirt_mcmc_run): m bytes, non-zero = in the form; NULL: all m items */
    void*      raw[GPIRT_SUMSCORE_NARRAYS];
    int64_t    m, M;                           /* out */
    int64_t    draws, skipped, rel_draws, rel_skipped;   /* out */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_sumscore;
/* Stage API.  sumscore_enable(items_mask, on != 0) allocates and zeroes the state for the form the mask names (m bytes, non-zero
 * = in the form; NULL: all m items); GPIRT_E_ARG with a message for an empty form and for M > GPIRT_SUMSCORE_MAX_ITEMS, the old
 * state is then kept; on = 0 frees it.  sumscore_accumulate adds the CURRENT f* (the sampler array "fstar") as one draw.
 * sumscore_get copies one array by name to the host, `bytes` its exact size: the lower-case names of the raw arrays
 * ("joint_sum", "pi_sum", "pi_sumsq", "tcc_sum", "tcc_sumsq", "var_sum", "rel", "mask", "w", "last", "last_pi"), "counts" (int64:
 * draws, skipped, rel_draws, rel_skipped) and, of the last counted draw, "tcc" and "var" (double [1001]).
 * sumscore_state returns the ONE device block (valid until sumscore_enable is called again or the sampler goes): a header of 16
 * int64 -- the tag 0x43534d53 ("SMSC"), the layout version (1), m, M, N = 1001, draws, skipped, rel_draws, rel_skipped, 0 ... --
 * then the raw arrays in the order above, every array starting on a 16-byte boundary; gpirt_sumscore_state_bytes gives its
 * size.  gpirt_sumscore_grid_weights writes the 1001 weights w_k (host only; no device is needed). */
int gpirt_sampler_sumscore_enable(gpirt_sampler_t s, const unsigned char* items_mask, int on);
int gpirt_sampler_sumscore_accumulate(gpirt_sampler_t s);
int gpirt_sampler_sumscore_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_sumscore_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_sumscore_state_bytes(int64_t m, int64_t M, int64_t* bytes);
int gpirt_sumscore_grid_weights(double* h_w);
int gpirt_sumscore_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_sumscore* out);

/* ------------------------------------------------------------- group-wise item fit (DIF): Mantel-Haenszel per item ------------ */
/* Given theta, does an answer still depend on WHO the respondent is (library version 115)?  Differential item functioning: the
 * respondents are stratified by the bin of a draw's theta (the cuts, the bins and grid_index's rule of the theta-binned item fit
 * above) and, stratum by stratum, a focal group's answers to an item are compared with the reference group's -- the
 * Mantel-Haenszel common odds ratio (Holland and Thayer 1988) and the standardised P-difference (Dorans and Kulick 1986) as
 * posterior predictive discrepancies.  A third add-on to the PPC: enabled on a sampler whose ppc_enable is on, accumulated inside
 * the same ppc_accumulate call by a pass of its own that forms the PPC's replicate again, bit for bit (the same expression for p,
 * the same item_uniform(seed, iter, GPIRT_ST_PPC, item0 + j, i)); nothing is drawn.
 * Groups.  One code per respondent: -1 = left out, 0 = the reference group, 1 .. G - 1 the focal groups,
 * 2 <= G <= GPIRT_DIF_MAX_G = 4, every group with at least one member; n <= GPIRT_DIF_MAX_N = 65534.  A respondent's cell in a
 * draw is c = group B + bin (uint8; 255 = left out or theta off the grid).
 * Per draw and (group g, bin b, item j), over the observed cells of the respondents in (g, b): the integers N = #cells,
 * T = #{y = +1}, R = #{rep = 1}, and E = sum rint(p 2^44), V = sum rint(p q 2^44) as uint64 (below 2^60): every term rounded once,
 * the sums exact, so the tables do not depend on the order of summation and integer atomics (LDS and global) form them
 * deterministically.  E and V below stand for (double)E_fix 2^-44 and (double)V_fix 2^-44.
 * Per COUNTED draw, every statistic in fp64 from those integer tables, without contraction -- conversions, products, divisions and
 * additions only, summed in increasing b --, so the same tables give the same bits anywhere:
 *   cell (g, b, j): sum_n, sum_t, sum_r += N, T, R (uint64); sum_e += E (double); occ_sum[g, b] += #{i in (g, b)};
 *   group g, item j: R_g = sum_b R, T_g = sum_b T: yes_ge / yes_gt += [R_g >= / > T_g];
 *            X2_g(C) = sum_b ((double)C - E)^2 / V over the bins with N > 0 and V > 0.  If R = T in every bin of the group the
 *            draw counts in chi_ge and not in chi_gt, else chi_ge / chi_gt += [X2_g(R) >= / > X2_g(T)]; chi_obs_sum += X2_g(T),
 *            chi_rep_sum += X2_g(R);
 *   focal f = 1 .. G - 1 against group 0, item j, over the bins with N_0 > 0 and N_f > 0, n_b = N_0 + N_f, for C in {T, R}:
 *            num(C) = sum_b (double)(C_0 (N_f - C_f)) / n_b, den(C) = sum_b (double)((N_0 - C_0) C_f) / n_b, alpha = num / den.
 *            If any of num(T), den(T), num(R), den(R) is 0: mh_undefined += 1 and nothing else of the MH block; otherwise
 *            mh_ge / mh_gt += [num(R) den(T) >= / > num(T) den(R)], mh_log_obs_sum += log(num(T) / den(T)),
 *            mh_log_rep_sum += log(num(R) / den(R)).
 *            STD(C) = (sum_b N_f (C_f / N_f - C_0 / N_0)) / sum_b N_f; without a common bin std_undefined += 1, otherwise
 *            std_obs_sum += STD(T), std_rep_sum += STD(R).
 * A draw is skipped whole when any theta is off the grid or g is non-finite in an observed cell of a grouped respondent:
 * dif_skipped += 1 and nothing else changes; any other draw adds 1 to dif_draws.  The host never synchronises for it.
 * Finished on the host with S = dif_draws (NaN where a denominator is 0): G x B x m arrays, cell (g, b, j) at [(g B + b) m + j]
 * (GPIRT_DIF_CELL_*): obs_rate = sum_t / sum_n, rep_rate = sum_r / sum_n, exp_rate = sum_e / sum_n; occupancy = occ_sum / S
 * (G x B); G x m arrays (GPIRT_DIF_GROUP_*): ppp_yes = yes_ge / S, ppp_yes_mid = (yes_ge + yes_gt) / 2S, ppp_chi2, ppp_chi2_mid
 * likewise, chi2_obs_mean, chi2_rep_mean; G x m arrays whose row 0 is NaN (GPIRT_DIF_FOCAL_*), with S' = S - mh_undefined and
 * S" = S - std_undefined: mh_log_or_obs_mean = mh_log_obs_sum / S', mh_log_or_rep_mean, mh_delta_obs_mean = -2.35
 * mh_log_or_obs_mean (the ETS delta scale), ppp_mh = mh_ge / S', ppp_mh_mid = (mh_ge + mh_gt) / 2S', mh_undefined,
 * std_obs_mean = std_obs_sum / S", std_rep_mean, std_undefined.
 *   flagged: the `top` (1..GPIRT_DIF_MAX_TOP, the Python default is 20) (focal group, item) pairs by decreasing
 *   |ppp_mh_mid - 0.5|, ties to the lowest (group, item), NaN never listed: items, groups, ppp_mh_mid, padded with -1 / NaN.
 * Determinism: no floating-point atomics anywhere; the only atomics add integers.  Two runs give a byte-identical state block.
 * Pooling C chains (gpirt_ppc_dif_combine) adds the integers and adds the doubles in chain order; a chain with sign -1 enters with
 * the bin axis of the (group, bin, item) tables and of occ_sum reversed (exact: the bins are symmetric); every counter and
 * per-draw sum is kept as the chain decided it.  Blocks with another n, m, item0, G, group vector or cuts are refused.
 * With the block on, the chain, the IRFs, R's stream position and the PPC, pairs and bins state blocks are bit for bit what they
 * are without.  Item shards stay refused.
 * The raw arrays (GPIRT_DIF_NRAW, in the state block's order): uint64 sum_n, sum_t, sum_r, double sum_e (G B m), uint64 occ_sum
 * (G B), uint32 yes_ge, yes_gt, chi_ge, chi_gt, mh_ge, mh_gt, mh_undefined_count, std_undefined_count (G m), double chi_obs_sum, chi_rep_sum,
 * mh_log_obs_sum, mh_log_rep_sum, std_obs_sum, std_rep_sum (G m; the rows of group 0 of the focal arrays stay 0). */
#define GPIRT_DIF_MAX_G      4
#define GPIRT_DIF_MAX_N      65534
#define GPIRT_DIF_MAX_TOP    64
#define GPIRT_DIF_CELL_NFIELDS   3      /* obs_rate, rep_rate, exp_rate */
#define GPIRT_DIF_GROUP_NFIELDS  6      /* ppp_yes, ppp_yes_mid, ppp_chi2, ppp_chi2_mid, chi2_obs_mean, chi2_rep_mean */
#define GPIRT_DIF_FOCAL_NFIELDS  9      /* mh_log_or_obs_mean, mh_log_or_rep_mean, mh_delta_obs_mean, ppp_mh, ppp_mh_mid,
                                           mh_undefined, std_obs_mean, std_rep_mean, std_undefined */
#define GPIRT_DIF_NRAW           19
/* HOST pointers (NULL: not wanted). */
typedef struct gpirt_ppc_dif {
    int        top;                            /* in: 1..GPIRT_DIF_MAX_TOP */
    int        G;                              /* in (gpirt_mcmc_run): the number of groups; out: the states' */
    int        h;                              /* in (gpirt_mcmc_run): the number of cuts; out: the states' */
    int        cuts[GPIRT_BINS_MAX_H + 1];     /* in (gpirt_mcmc_run) / out: d_1 .. d_h, the rest 0 */
    int        reserved0;                      /* must be 0 */
    const int32_t* groups;                     /* in (gpirt_mcmc_run): n codes in -1 .. G - 1 */
    double*    cell[GPIRT_DIF_CELL_NFIELDS];   /* G x B x m each */
    double*    occupancy;                      /* G x B */
    double*    group[GPIRT_DIF_GROUP_NFIELDS]; /* G x m each */
    double*    focal[GPIRT_DIF_FOCAL_NFIELDS]; /* G x m each, row 0 NaN */
    void*      raw[GPIRT_DIF_NRAW];            /* the raw arrays, in the order and with the types above */
    int64_t*   flagged_items;                  /* top */
    int64_t*   flagged_groups;                 /* top */
    double*    flagged_ppp_mh_mid;             /* top */
    int64_t    n, m, B;                        /* out */
    int64_t    dif_draws, dif_skipped;         /* out */
    int64_t    group_size[GPIRT_DIF_MAX_G];    /* out: the members of each group (0 beyond G) */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_ppc_dif;
/* Stage API.  ppc_dif_enable(G, groups, h, cuts, on != 0) allocates and zeroes the state on a sampler with ppc_enable on
 * (GPIRT_E_ARG, with a message, without it, for n > GPIRT_DIF_MAX_N, for G outside 2..4, a code outside -1 .. G - 1, an empty group
 * and for cuts that break the bins' rule; on = 0 frees it, groups and cuts may then be NULL; ppc_enable called again frees it
 * too).  From then on every ppc_accumulate also adds the draw to the block.  ppc_dif_get copies one array by name to the host,
 * `bytes` its exact size: every finished array by the lower-case name above (double), the raw arrays by theirs, "counts" (int64:
 * dif_draws, dif_skipped), "cuts" (int64, h), "groups" (int8, n), "group_size" (int64, 4) and, of the last COUNTED draw, "cell"
 * (uint8, n), "tN", "tT", "tR" (int32, G x B x m), "tE", "tV" (the raw uint64 fixed-point sums, G x B x m) and "stats" (double,
 * 8 x G x m: num(T), den(T), num(R), den(R), STD(T), STD(R) -- NaN for group 0, the STDs NaN without a common bin --, X2_g(T), X2_g(R)).
 * ppc_dif_state returns the ONE device block of its own: a header of 8 int64 -- n, m, layout version (1), dif_draws, dif_skipped,
 * item0, B, the tag 0x31464944 ("DIF1") --, 16 int64 with the cuts d_1 .. d_h (the rest 0), 8 int64 G, group_size[0..3], 0, 0, 0,
 * the n group codes as int8, then the raw arrays in the order above; every array starts on a 16-byte boundary. */
int gpirt_sampler_ppc_dif_enable(gpirt_sampler_t s, int G, const int32_t* groups, int h, const int* cuts, int on);
int gpirt_sampler_ppc_dif_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ppc_dif_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_ppc_dif_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ppc_dif* out);

/* ------------------------------------------------- score-based PPC: score distribution, item-rest fit by score group --------- */
/* The three discrepancies Sinharay, Johnson and Stern (2006) name first for a one-dimensional model, on the MANIFEST score
 * (library version 120): the observed-score distribution, every item's correlation with the rest of the test, and the item fit
 * within groups of the rest score (the grouping of Orlando and Thissen's S-X2; the theta-binned fit above groups on each draw's
 * latent theta instead, which is what makes it conservative).  A fourth add-on to the PPC: enabled on a sampler whose ppc_enable
 * is on, accumulated inside the same ppc_accumulate call by passes of its own that form the PPC's replicate again, bit for bit
 * (the same expression for p, the same item_uniform(seed, iter, GPIRT_ST_PPC, item0 + j, i)); nothing is drawn.  Stage API only:
 * gpirt_run has no field for it yet.
 * n respondents, m items, 2 <= m <= GPIRT_SCORES_MAX_M = 4096, n <= GPIRT_SCORES_MAX_N = 65534, 2 <= K <= GPIRT_SCORES_MAX_K = 16
 * score groups; item shards are refused.  O = the observed cells, Y = [y = +1] and rep = [yrep = +1] on O.
 * Scores are raw counts over each respondent's own observed items: X_i = sum_j Y_ij (constant, counted on the device at enable),
 * Xr_i = sum_j rep_ij per draw; the rest scores of a cell W_ij = X_i - Y_ij and Wr_ij = Xr_i - rep_ij.  Respondents without an
 * observed cell are left out of everything; n_s is the number of the others.
 * Cuts: ascending integers c_1 < ... < c_{K-1} in 1 .. m - 1; the group of a rest score w is #{k : c_k <= w}, so group k holds
 * the rest scores group_lo[k] = c_k (0 for k = 0) to group_hi[k] = c_{k+1} - 1 (m - 1 for k = K - 1).
 * A draw with a non-finite g = f + mu in an observed cell is skipped whole -- score_skipped += 1 and nothing else changes, which
 * is decided before any accumulator is touched; a NaN in a missing cell is ignored.  Every other draw adds 1 to score_draws.
 * 1. Score distribution.  H[s] = #{i : score_i = s}, s = 0 .. m, over the n_s respondents, for the data (hist_obs) and per draw
 *    for the replicate; C[s] = H[0] + ... + H[s].  Per counted draw and s: hist_sum += H_rep, hist_sumsq += H_rep^2 (uint64),
 *    hist_ge / hist_gt += [H_rep >= / > H_obs], cdf_ge / cdf_gt += [C_rep >= / > C_obs] (uint32).  The spread of the scores
 *    Vn = n_s S2 - S1^2 with S1 = sum_i X_i, S2 = sum_i X_i^2: an exact int64 (S2 <= 65534 x 4096^2 < 2^41, both terms < 2^57);
 *    var_obs = (Vn_obs, n_s); var_ge / var_gt += [Vn_rep >= / > Vn_obs], var_rep_sum += Vn_rep (uint64).
 * 2. Item-rest correlation.  Per item j over i in O_j: N = #O_j, A = sum Y, B = sum W, Cq = sum W^2, D = sum Y W -- integers,
 *    B <= 65534 x 4096 < 2^28, Cq < 2^40 -- and NUM = N D - A B, VA = N A - A^2, VC = N Cq - B^2 exactly in int64 (every product
 *    is below 2^57).  r = (double)NUM / sqrt((double)VA * (double)VC): each conversion rounded once, sqrt and the division
 *    IEEE.  r_obs at enable (NaN when VA = 0 or VC = 0); r_rep per draw from rep and Wr.  When VA = 0 or VC = 0 in the replicate,
 *    or r_obs is NaN, the draw counts in r_undefined_count[j] and enters nothing else of item j's correlation; otherwise
 *    r_ge / r_gt += [r_rep >= / > r_obs], r_rep_sum += r_rep, r_rep_sumsq += r_rep r_rep (doubles, in draw order).
 * 3. Item fit by rest-score group.  Per (group k, item j): the data's cells are grouped by W_ij -- constant, so tNo[k, j] = #cells
 *    and tT[k, j] = #{Y = 1} are counted at enable --, the replicate's cells by Wr_ij, which gives Nr and R per draw.  Given theta
 *    item j's answer is independent of the REST score, so E = sum p is the expectation within a group (it would not be under a
 *    grouping by the total score).  Both groupings get E = sum rint(p 2^44) and V = sum rint(p q 2^44) over their cells (Eo, Vo
 *    and Er, Vr; int64, below 2^60): every term rounded once, the sums exact and independent of the order of summation.
 *    Per counted draw: sum_nr += Nr, sum_r += R (uint64), sum_eo += (double)Eo 2^-44, sum_er += (double)Er 2^-44 (in draw order);
 *    when Nr > 0 and No > 0 cell_ge / cell_gt += [R No >= / > T Nr] (integer cross-multiplication), otherwise cell_empty += 1.
 *    Item statistic for C = T with (Eo, Vo) and for C = R with (Er, Vr): d = (double)(C 2^44 - E) 2^-44, v = (double)V 2^-44,
 *    X2 = sum over k ascending with V > 0 of d d / v (no contraction).  chi_ge / chi_gt += [X2(R) >= / > X2(T)], chi_obs_sum +=
 *    X2(T), chi_rep_sum += X2(R).
 * Finished on the host with S = score_draws (NaN where a denominator is 0; a mean over zero draws is NaN):
 *   m + 1 values each (GPIRT_SCORES_HIST_*): score_hist_obs, score_hist_rep_mean = hist_sum / S, score_hist_rep_sd =
 *   sqrt((S hist_sumsq - hist_sum^2) / (S (S - 1))) (the numerator exact in 128 bits), ppp_hist = hist_ge / S, ppp_hist_mid =
 *   (hist_ge + hist_gt) / 2S, ppp_cdf, ppp_cdf_mid;
 *   3 values (var): score_var_obs = Vn_obs / n_s^2, score_var_rep_mean = var_rep_sum / (S n_s^2), ppp_var = var_ge / S;
 *   m values each (GPIRT_SCORES_ITEM_*), with S' = S - r_undefined_count: r_rep_mean = r_rep_sum / S', r_rep_sd =
 *   sqrt(max((r_rep_sumsq - r_rep_sum r_rep_mean) / (S' - 1), 0)) for S' >= 2, ppp_r = r_ge / S', ppp_r_mid, r_undefined,
 *   ppp_chi2 = chi_ge / S, ppp_chi2_mid, chi2_obs_mean, chi2_rep_mean;
 *   K x m values each, cell (k, j) at [k m + j] (GPIRT_SCORES_CELL_*): obs_rate = tT / tNo, rep_rate = sum_r / sum_nr, exp_rate =
 *   sum_eo / (S tNo), and with S" = S - cell_empty: ppp_cell = cell_ge / S", ppp_cell_mid;
 *   group_lo, group_hi (int64, K); worst: the `top` (1..GPIRT_SCORES_MAX_TOP, the Python default is 20) items with the smallest
 *   ppp_chi2_mid, ties to the lowest j, NaN never listed, padded with -1 / NaN.
 * Determinism: no floating-point atomics anywhere; the only atomics add integers.  Two runs give a byte-identical state block.
 * Pooling C chains (gpirt_ppc_scores_combine) adds the integers and adds the doubles in chain order.  It takes no signs: theta ->
 * -theta leaves f + mu of every cell as it is.  Blocks with another n, m, K, cuts or response matrix (the constants differ) than
 * state 0 are refused.  With the block on, the chain, the IRFs and the PPC, pairs, bins and dif state blocks are bit for bit what
 * they are without.
 * The raw arrays (GPIRT_SCORES_NRAW, in the state block's order).  Constants: int64 hist_obs (m + 1), int64 sums_obs (4 x m: A, B,
 * Cq, D), int64 var_obs (2), double r_obs (m), uint32 tNo, tT (K m).  Accumulators: uint64 hist_sum, hist_sumsq, uint32 hist_ge,
 * hist_gt, cdf_ge, cdf_gt (m + 1); uint32 var_ge, var_gt, uint64 var_rep_sum (1); uint32 r_ge, r_gt, r_undefined_count, double
 * r_rep_sum, r_rep_sumsq (m); uint32 cell_ge, cell_gt, cell_empty, uint64 sum_nr, sum_r, double sum_eo, sum_er (K m); uint32
 * chi_ge, chi_gt, double chi_obs_sum, chi_rep_sum (m). */
#define GPIRT_SCORES_MAX_M       4096
#define GPIRT_SCORES_MAX_N       65534
#define GPIRT_SCORES_MAX_K       16
#define GPIRT_SCORES_MAX_TOP     64
#define GPIRT_SCORES_HIST_NFIELDS  7    /* score_hist_obs, score_hist_rep_mean, score_hist_rep_sd, ppp_hist, ppp_hist_mid, ppp_cdf,
                                           ppp_cdf_mid */
#define GPIRT_SCORES_ITEM_NFIELDS  9    /* r_rep_mean, r_rep_sd, ppp_r, ppp_r_mid, r_undefined, ppp_chi2, ppp_chi2_mid,
                                           chi2_obs_mean, chi2_rep_mean */
#define GPIRT_SCORES_CELL_NFIELDS  5    /* obs_rate, rep_rate, exp_rate, ppp_cell, ppp_cell_mid */
#define GPIRT_SCORES_NRAW          31
/* HOST pointers (NULL: not wanted). */
typedef struct gpirt_ppc_scores {
    int        top;                              /* in: 1..GPIRT_SCORES_MAX_TOP */
    int        K;                                /* out: the states' number of groups */
    int        cuts[GPIRT_SCORES_MAX_K];         /* out: c_1 .. c_{K-1}, the rest 0 */
    double*    hist[GPIRT_SCORES_HIST_NFIELDS];  /* m + 1 each */
    double*    var;                              /* 3: score_var_obs, score_var_rep_mean, ppp_var */
    double*    item[GPIRT_SCORES_ITEM_NFIELDS];  /* m each */
    double*    cell[GPIRT_SCORES_CELL_NFIELDS];  /* K x m each */
    void*      raw[GPIRT_SCORES_NRAW];           /* the raw arrays, in the order and with the types above */
    int64_t*   group_lo;                         /* K */
    int64_t*   group_hi;                         /* K */
    int64_t*   worst_items;                      /* top */
    double*    worst_ppp_chi2_mid;               /* top */
    int64_t    n, m;                             /* out */
    int64_t    score_draws, score_skipped;       /* out */
    int64_t    n_scored;                         /* out: n_s, the respondents with an observed cell */
    int64_t    reserved[4];                      /* must be 0 */
} gpirt_ppc_scores;
/* Stage API.  ppc_scores_enable(K, cuts, on != 0) allocates and zeroes the state on a sampler with ppc_enable on and counts the
 * constants on the device (GPIRT_E_ARG, with a message, without ppc_enable, on an item shard, for m outside 2..4096, n > 65534, K
 * outside 2..16 and for cuts that are not K - 1 ascending integers in 1 .. m - 1; on = 0 frees it, cuts may then be NULL;
 * ppc_enable called again frees it too).  From then on every ppc_accumulate also adds the draw to the block.  ppc_scores_get
 * copies one array by name to the host, `bytes` its exact size: every finished array by the lower-case name above (double), the
 * raw arrays by theirs, "group_lo", "group_hi" (int64, K), "counts" (int64: score_draws, score_skipped), "cuts" (int64, K - 1),
 * "x_obs" (int32, n) and, of the last COUNTED draw, "xr" (int32, n), "hist" (int64, m + 1), "sums" (int64, 4 x m: A, B, Cq, D
 * of the replicate), "r" (double, m; NaN where VA = 0 or VC = 0), "tNr", "tR" (uint32, K x m), "tEo", "tVo", "tEr", "tVr" (the
 * fixed-point int64 sums, K x m) and "chi" (double, 2 x m: X2(T), X2(R)).
 * ppc_scores_state returns the ONE device block of its own: a header of 8 int64 -- the tag 0x31524353 ("SCR1"), the layout
 * version (1), n, m, K, score_draws, score_skipped, 0 --, 16 int64 with the cuts c_1 .. c_{K-1} (the rest 0), then the raw arrays in
 * the order above; every array starts on a 16-byte boundary.
 * gpirt_ppc_scores_check is ppc_scores_enable's argument check alone (0, or GPIRT_E_ARG with the message): nothing is allocated and
 * no device is touched. */
int gpirt_ppc_scores_check(int64_t n, int64_t m, int K, const int* cuts);
int gpirt_sampler_ppc_scores_enable(gpirt_sampler_t s, int K, const int* cuts, int on);
int gpirt_sampler_ppc_scores_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ppc_scores_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_ppc_scores_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_scores* out);

/* ------------------------------------------------- person fit in the PPC: Guttman errors, lz, person response function ------- */
/* The checks above judge an ITEM; for a RESPONDENT the PPC has the yes count and one deviance p-value (respondent_ppp_dev).  A
 * respondent who misses the easy items and answers the hard ones can replicate both: what goes wrong is WHICH items were answered
 * yes, in the order of their easiness.  This section adds the three standard person-fit tools in their posterior predictive form
 * (Glas and Meijer 2003): the number of Guttman errors (Meijer 1994), the standardised log-likelihood lz (Drasgow, Levine and
 * Williams 1985) and the person response function, the yes rate by item-easiness group (Sijtsma and Meijer 2001).  For a GP-IRT
 * model the curves need not be monotone, so the model does not imply a Guttman pattern: only the replicate of each draw says how
 * many errors a respondent is expected to make.  It is the score-based section transposed: respondent fit within groups of the
 * items' easiness.  A fifth add-on to the PPC (library version 121): enabled on a sampler whose ppc_enable is on, accumulated
 * inside the same ppc_accumulate call by a pass of its own that forms the PPC's replicate again, bit for bit (the same expression
 * for p, the same item_uniform(seed, iter, GPIRT_ST_PPC, item0 + j, i)); nothing is drawn.  Stage API only: gpirt_run,
 * gpirt_mcmc_run and gpirtMCMC have no field for it and stay exactly as they are.
 * n respondents, m items, column-major (cell (i, j) at i + j n), 2 <= m <= GPIRT_PERSON_MAX_M = 4096, n <= GPIRT_PERSON_MAX_N =
 * 65534, 2 <= K <= GPIRT_PERSON_MAX_K = 16 item groups; item shards are refused.  O = the observed cells, Y = [y = +1] and rep =
 * [yrep = +1] on O.  A respondent without an observed cell is left out of everything: no accumulator of its moves and every
 * finished value of its is NaN.
 * Item order and groups, given by the caller and constant for the state: `order` is a permutation of 0 .. m - 1, the easiest item
 * first; position t holds item order[t].  The cuts c_1 < ... < c_{K-1}, integers in 1 .. m - 1, act on POSITIONS: position t lies
 * in group #{k : c_k <= t}, so group k holds the positions group_lo[k] = c_k (0 for k = 0) to group_hi[k] = c_{k+1} - 1 (m - 1
 * for k = K - 1).  The STRIPS: each group's positions are cut, from the group's first position on, into runs of 32 (the last run
 * of a group may be shorter); the strips are numbered in ascending position.  They fix the order of the floating-point sums.
 * A draw with a non-finite g = f + mu in an observed cell is skipped whole -- person_skipped += 1 and nothing else changes, which
 * is decided before any accumulator is touched; a NaN in a missing cell is ignored.  Every other draw adds 1 to person_draws.
 * Per respondent i, over i's observed cells in position order (N = #O_i):
 * 1. Guttman errors.  For z in {Y, rep}: X(z) = sum z, G(z) = #{positions s < t, both observed : z_s = 0, z_t = 1}, Q(z) =
 *    X (N - X), the largest G that score allows.  x_obs, g_obs, q_obs are constants (int64), counted on the device at enable.
 *    Per counted draw: if Q_obs = 0 or Q_rep = 0, g_undefined_count += 1 and the draw enters nothing else of the Guttman check;
 *    otherwise g_ge / g_gt += [G_rep Q_obs >= / > G_obs Q_rep] (an integer cross-multiplication, every product below 2^46),
 *    g_rep_sum += G_rep (uint64) and gn_rep_sum += (double)G_rep / (double)Q_rep (in draw order).  A small p-value says that the
 *    data hold more errors than the model replicates.
 * 2. lz.  With g the cell's f + mu, e = exp(-|g|), p = 1 / (1 + e) for g >= 0 and e / (1 + e) otherwise, q the other of the two:
 *    l(z) - E[l] = sum (z - p) g exactly and Var[l] = sum p q g^2, so no logarithm is needed.  Per draw Wo = sum (Y - p) g, Wr =
 *    sum (rep - p) g, Vl = sum ((p q) g) g, every term in fp64 as written (Y and rep as 0.0 / 1.0, no contraction), the observed
 *    cells of a strip added in ascending position to 0.0, the strips' sums added in ascending strip to 0.0.  No floating-point
 *    atomics.  If Vl is not finite or not > 0, or Wo or Wr is not finite, lz_undefined_count += 1; otherwise, with sd =
 *    sqrt(Vl), lz_obs_sum += Wo / sd, lz_rep_sum += Wr / sd, lz_rep_sumsq += (Wr / sd) (Wr / sd).  The p-value of lz is the PPC's
 *    own respondent_ppp_dev -- l(rep) <= l(y) exactly when D(rep) >= D(y) -- and is not stored twice.
 * 3. Person response function.  Per (group k, respondent i): tN = #observed cells and tT = #{Y = 1} (constants, uint32, counted
 *    at enable); per draw R = #{rep = 1}, E = sum rint(p 2^44) and V = sum rint((p q) 2^44) as int64 (the score-based section's
 *    fixed point: every term rounded once, the sums exact in any order).  Per counted draw and cell with tN > 0: sum_r += R
 *    (uint64), sum_e += (double)E 2^-44, cell_ge / cell_gt += [R >= / > tT] (the same cells on both sides, so no
 *    cross-multiplication).  X2(C) = sum over k ascending with V > 0 of d d / v, d = (double)(C 2^44 - E) 2^-44, v = (double)V
 *    2^-44 (no contraction); chi_ge / chi_gt += [X2(R) >= / > X2(tT)], chi_obs_sum += X2(tT), chi_rep_sum += X2(R).
 * Finished on the host with S = person_draws (NaN where a denominator is 0 and for a respondent without an observed cell):
 *   n values each (GPIRT_PERSON_RESP_*), with S' = S - g_undefined_count and S" = S - lz_undefined_count: guttman_obs = G_obs,
 *   guttman_norm_obs = G_obs / Q_obs, guttman_rep_mean = g_rep_sum / S', guttman_norm_rep_mean = gn_rep_sum / S', ppp_guttman =
 *   g_ge / S', ppp_guttman_mid = (g_ge + g_gt) / 2S', guttman_undefined; lz_obs_mean = lz_obs_sum / S", lz_rep_mean, lz_rep_sd =
 *   sqrt(max((lz_rep_sumsq - lz_rep_sum lz_rep_mean) / (S" - 1), 0)) for S" >= 2, lz_undefined; ppp_chi2 = chi_ge / S,
 *   ppp_chi2_mid, chi2_obs_mean, chi2_rep_mean;
 *   K x n values each, cell (k, i) at [k n + i] (GPIRT_PERSON_CELL_*; NaN where tN = 0): obs_rate = tT / tN, rep_rate = sum_r /
 *   (S tN), exp_rate = sum_e / (S tN), ppp_cell = cell_ge / S, ppp_cell_mid;
 *   group_lo, group_hi (int64, K; positions), group_items (int32, m: the order itself); worst: the `top` (1 ..
 *   GPIRT_PERSON_MAX_TOP, the Python default is 20) respondents with the smallest ppp_guttman_mid, ties to the lowest i, NaN never
 *   listed, padded with -1 / NaN.
 * Determinism: every accumulator of a respondent is owned by one thread and there is no atomic at all; two runs give a
 * byte-identical state block.  Pooling C chains (gpirt_ppc_person_combine) adds the integers and adds the doubles in chain order.
 * It takes no signs: theta -> -theta leaves f + mu of every cell as it is.  Blocks whose n, m, K, order, cuts or constants differ
 * from state 0 are refused.  With the block on, the chain, the IRFs and the PPC, pairs, bins, dif and scores state blocks are bit
 * for bit what they are without.
 * The raw arrays (GPIRT_PERSON_NRAW, in the state block's order).  Constants: int64 x_obs, g_obs, q_obs (n), uint32 tN, tT (K n).
 * Accumulators: uint32 g_ge, g_gt, g_undefined_count, uint64 g_rep_sum, double gn_rep_sum (n); uint32 lz_undefined_count, double
 * lz_obs_sum, lz_rep_sum, lz_rep_sumsq (n); uint64 sum_r, double sum_e, uint32 cell_ge, cell_gt (K n); uint32 chi_ge, chi_gt,
 * double chi_obs_sum, chi_rep_sum (n).
 * Device memory per state at 8192 x 1024 with 16 groups: the block 5.0 MB (104 bytes per respondent and 32 per cell), the
 * strips' partials 17 MB at the most (44 bytes per strip and respondent, 32 to 47 strips), the last draw's arrays 3.0 MB. */
#define GPIRT_PERSON_MAX_M       4096
#define GPIRT_PERSON_MAX_N       65534
#define GPIRT_PERSON_MAX_K       16
#define GPIRT_PERSON_MAX_TOP     64
#define GPIRT_PERSON_RESP_NFIELDS  15   /* guttman_obs, guttman_norm_obs, guttman_rep_mean, guttman_norm_rep_mean, ppp_guttman,
                                           ppp_guttman_mid, guttman_undefined, lz_obs_mean, lz_rep_mean, lz_rep_sd, lz_undefined,
                                           ppp_chi2, ppp_chi2_mid, chi2_obs_mean, chi2_rep_mean */
#define GPIRT_PERSON_CELL_NFIELDS  5    /* obs_rate, rep_rate, exp_rate, ppp_cell, ppp_cell_mid */
#define GPIRT_PERSON_NRAW          22
/* HOST pointers (NULL: not wanted). */
typedef struct gpirt_ppc_person {
    int        top;                              /* in: 1..GPIRT_PERSON_MAX_TOP */
    int        K;                                /* out: the states' number of groups */
    int        cuts[GPIRT_PERSON_MAX_K];         /* out: c_1 .. c_{K-1}, the rest 0 */
    double*    resp[GPIRT_PERSON_RESP_NFIELDS];  /* n each */
    double*    cell[GPIRT_PERSON_CELL_NFIELDS];  /* K x n each */
    void*      raw[GPIRT_PERSON_NRAW];           /* the raw arrays, in the order and with the types above */
    int64_t*   group_lo;                         /* K */
    int64_t*   group_hi;                         /* K */
    int32_t*   group_items;                      /* m: the order */
    int64_t*   worst_respondents;                /* top */
    double*    worst_ppp_guttman_mid;            /* top */
    int64_t    n, m;                             /* out */
    int64_t    person_draws, person_skipped;     /* out */
    int64_t    n_scored;                         /* out: the respondents with an observed cell */
    int64_t    reserved[4];                      /* must be 0 */
} gpirt_ppc_person;
/* Stage API.  ppc_person_enable(K, order, cuts, on != 0) allocates and zeroes the state on a sampler with ppc_enable on and counts
 * the constants on the device (GPIRT_E_ARG, with a message that names the fault, without ppc_enable, on an item shard, for m
 * outside 2..4096, n > 65534, K outside 2..16, for an order that is not a permutation of 0 .. m - 1 -- the first offending entry is
 * named -- and for cuts that are not K - 1 ascending integers in 1 .. m - 1; on = 0 frees it, order and cuts may then be NULL;
 * ppc_enable called again frees it too).  From then on every ppc_accumulate also adds the draw to the block.  ppc_person_get
 * copies one array by name to the host, `bytes` its exact size: every finished array by the lower-case name above (double), the
 * raw arrays by theirs, "group_lo", "group_hi" (int64, K), "group_items" and "order" (int32, m), "counts" (int64: person_draws,
 * person_skipped), "cuts" (int64, K - 1) and, of the last COUNTED draw, "xr", "gr", "qr" (int64, n: X, G, Q of the replicate),
 * "tR" (uint32, K x n), "tE", "tV" (the fixed-point int64 sums, K x n), "lz" (double, 3 x n: Wo, Wr, Vl) and "chi" (double, 2 x
 * n: X2(tT), X2(R)).
 * ppc_person_state returns the ONE device block of its own: a header of 8 int64 -- the tag 0x31535250 ("PRS1"), the layout
 * version (1), n, m, K, person_draws, person_skipped, 0 --, 16 int64 with the cuts c_1 .. c_{K-1} (the rest 0), the order as m
 * int32, then the raw arrays in the order above; every array starts on a 16-byte boundary.
 * gpirt_ppc_person_check is ppc_person_enable's argument check alone (0, or GPIRT_E_ARG with the message): nothing is allocated
 * and no device is touched. */
int gpirt_ppc_person_check(int64_t n, int64_t m, int K, const int32_t* order, const int* cuts);
int gpirt_sampler_ppc_person_enable(gpirt_sampler_t s, int K, const int32_t* order, const int* cuts, int on);
int gpirt_sampler_ppc_person_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ppc_person_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_ppc_person_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_person* out);

/* ------------------------------------------------- residual correlations in the PPC: local dependence, infit, global tests ------- */
/* Is one dimension enough, as a single test (library version 123)?  The pairs section returns m (m - 1) / 2 p-values and nothing
 * that sums them up, and its odds ratio weighs every co-observed respondent alike.  This sixth add-on forms, per draw, the
 * residual correlation of every item pair (Yen's Q3 with the model variance as the scale), the infit mean square of every item
 * (the diagonal of the same products), each item's share t_a in the dependence and three global statistics -- the sum of squared
 * residual correlations Q, the largest correlation M+ and the largest absolute one M -- for the data and for that draw's
 * replicate, and accumulates the comparisons.  Enabled on a sampler whose ppc_enable is on; it accumulates inside the same
 * ppc_accumulate call.  2 <= m <= GPIRT_RESID_MAX_M = 4096, n <= GPIRT_RESID_MAX_N = 65534; item shards stay refused.
 * Per draw, with g = f + mu, over the observed cells (O = the 0 / 1 observed matrix; an unobserved cell is 0 in all three terms):
 *   e = exp(-|g|);  p = 1 / (1 + e), q = e / (1 + e) for g >= 0, p = e / (1 + e), q = 1 / (1 + e) for g < 0 (the PPC's own
 *   arithmetic: p is 1 / (1 + exp(-g)) and q is 1 / (1 + exp(+g)), each formed on its own; +-inf gives exactly 0 and 1)
 *   d_obs = +q where y = +1, -p where y = -1;   d_rep = the same with yrep = +1 if u < p, else -1, u the PPC's uniform
 *   item_uniform(seed, iter, GPIRT_ST_PPC, item0 + j, i): the PPC's replicate bit for bit, nothing else is drawn (at g = +-inf,
 *   where the PPC itself counts the item's draw out, the same rule gives yrep = +-1);   w = p q
 *   dt = rint(d 2^22) in [-2^22, 2^22], wt = rint(w 2^22) in [0, 2^20]: every term rounded ONCE, to units of 2^-22.
 * Each term is split in three balanced base-256 digits (d0, d1 in [-128, 127], |d2| <= 64) held as int8 planes in the operand
 * layout of the pairs section; the nine digit-plane products per statistic run on the int8 matrix cores (a product is below
 * 65534 x 128 x 128 < 2^31) and are joined with the weights 256^(u + v) into exact int64 (|S| <= 65534 x 2^44 < 2^61):
 *   S_obs[a, b] = sum_i dt_obs[i, a] dt_obs[i, b],  S_rep likewise (symmetric, units of 2^-44),
 *   V[a, b] = sum_i wt[i, a] O[i, b] (NOT symmetric, units of 2^-22),  n_co = O^T O once at enable.
 * Per COUNTED draw and ordered pair (a, b), a != b, with n_co > 0 (pair (a, b) at [a m + b]):
 *   V[a, b] V[b, a] = 0: undefined_count += 1 and the pair is left out of every sum of this draw, data and replicate alike;
 *   otherwise r = (double)S / (sqrt((double)V[a, b] * (double)V[b, a]) * 4194304.0) for S_obs and S_rep (conversion, product,
 *   square root, product, division: in this order),  rc_obs_sum += r_obs, rc_rep_sum += r_rep, rc_rep_sumsq += r_rep r_rep,
 *   rc_ge / rc_gt += [S_rep >= / > S_obs]: both share the positive denominator, so the comparison is made on the integers.
 * The DIAGONAL cell (a, a) of the same seven arrays holds item a's infit: undefined when V[a, a] = 0, otherwise
 *   infit = (double)S[a, a] / ((double)V[a, a] * 4194304.0) in place of r, the comparison again on S[a, a].
 * Per item a: t_a = sum over b != a, in ascending b, of r[a, b]^2 over the pairs defined in this draw; an item without one adds
 * 1 to ss_undefined, otherwise ss_obs_sum += t_obs, ss_rep_sum += t_rep, ss_ge / ss_gt += [t_rep >= / > t_obs] in fp64.
 * Global: u_a = sum over b > a, ascending, of r[a, b]^2; Q = sum over a, ascending, of u_a; M+ = max r, M = max |r| over the
 * defined pairs a < b.  A draw without a defined pair adds 1 to global_undefined; otherwise the 16 words `global` take
 *   [0..6] doubles frob_obs_sum, frob_rep_sum, frob_rep_sumsq, max_obs_sum, max_rep_sum, absmax_obs_sum, absmax_rep_sum,
 *   [7..12] uint64 frob_ge, frob_gt, max_ge, max_gt, absmax_ge, absmax_gt (rep >= / > obs in fp64), [13] global_undefined.
 * Every fp64 sum has one owning thread and the order stated above; there are no atomics, so two runs leave a byte-identical
 * state block and NumPy reproduces it bit for bit from the integer tables (gpirt_amd.ppc.resid_*).
 * A draw with a NaN g in an observed cell is skipped whole: resid_skipped += 1 and nothing else changes, decided on the device
 * before anything is touched.  A NaN in an unobserved cell is ignored.  Otherwise resid_draws += 1.
 * Finished on the host, S = resid_draws.  Pair arrays (m x m; NaN on the diagonal and where n_co = 0, except n_co itself), with
 * D = S - undefined_count:  n_co;  rc_obs_mean = rc_obs_sum / D, rc_rep_mean (NaN for D < 1);  rc_rep_sd = sqrt(max(0,
 * (rc_rep_sumsq - rc_rep_sum (rc_rep_sum / D)) / (D - 1))) (NaN for D < 2);  ppp_rc = rc_ge / D, ppp_rc_mid = (rc_ge + rc_gt) /
 * 2D;  undefined = undefined_count.  Item arrays (m): infit_obs_mean, infit_rep_mean, infit_rep_sd, ppp_infit, ppp_infit_mid by
 * the same formulas from the diagonal cells;  ss_obs_mean, ss_rep_mean, ppp_ss, ppp_ss_mid with D = S - ss_undefined.  Scalars,
 * D = S - global_undefined: frob_obs_mean, frob_rep_mean, frob_rep_sd, ppp_frob, ppp_frob_mid; max_obs_mean, max_rep_mean,
 * ppp_max, ppp_max_mid; absmax_obs_mean, absmax_rep_mean, ppp_absmax, ppp_absmax_mid.
 *   worst: the `top` (1..GPIRT_RESID_MAX_TOP, the Python default is 20) pairs a < b with the smallest ppp_rc_mid -- the data more
 *   correlated than the replicates: positive local dependence --, ties to the lowest (a, b), NaN never listed: their indices,
 *   ppp_rc_mid and rc_obs_mean, padded with -1 / NaN.  worst_items: the `top` items with the smallest ppp_ss_mid, ties to the
 *   lowest a.
 * Pooling C chains (gpirt_ppc_resid_combine) adds the integers and adds the doubles in chain order; blocks with another n, m or
 * item0, or another n_co, are refused.  theta -> -theta leaves f + mu as it is, so there are no signs.  Nothing is drawn: with
 * the block on, the chain, the IRFs, R's stream position and the PPC, pairs, bins, dif, scores and person state blocks are bit
 * for bit what they are without it.
 * Device memory per state: 44 bytes per ordered pair of accumulators and constants and 56 of per-draw tables (105 MB at m =
 * 1024), and 19 int8 planes of n x m padded to 256 respondents and 128 items (160 MB at 8192 x 1024). */
#define GPIRT_RESID_MAX_TOP  64
#define GPIRT_RESID_MAX_N    65534
#define GPIRT_RESID_MAX_M    4096
#define GPIRT_RESID_P_N_CO          0
#define GPIRT_RESID_P_RC_OBS_MEAN   1
#define GPIRT_RESID_P_RC_REP_MEAN   2
#define GPIRT_RESID_P_RC_REP_SD     3
#define GPIRT_RESID_P_PPP_RC        4
#define GPIRT_RESID_P_PPP_RC_MID    5
#define GPIRT_RESID_P_UNDEFINED     6
#define GPIRT_RESID_NPAIR           7
#define GPIRT_RESID_I_INFIT_OBS_MEAN  0
#define GPIRT_RESID_I_INFIT_REP_MEAN  1
#define GPIRT_RESID_I_INFIT_REP_SD    2
#define GPIRT_RESID_I_PPP_INFIT       3
#define GPIRT_RESID_I_PPP_INFIT_MID   4
#define GPIRT_RESID_I_SS_OBS_MEAN     5
#define GPIRT_RESID_I_SS_REP_MEAN     6
#define GPIRT_RESID_I_PPP_SS          7
#define GPIRT_RESID_I_PPP_SS_MID      8
#define GPIRT_RESID_NITEM             9
#define GPIRT_RESID_S_FROB_OBS_MEAN    0
#define GPIRT_RESID_S_FROB_REP_MEAN    1
#define GPIRT_RESID_S_FROB_REP_SD      2
#define GPIRT_RESID_S_PPP_FROB         3
#define GPIRT_RESID_S_PPP_FROB_MID     4
#define GPIRT_RESID_S_MAX_OBS_MEAN     5
#define GPIRT_RESID_S_MAX_REP_MEAN     6
#define GPIRT_RESID_S_PPP_MAX          7
#define GPIRT_RESID_S_PPP_MAX_MID      8
#define GPIRT_RESID_S_ABSMAX_OBS_MEAN  9
#define GPIRT_RESID_S_ABSMAX_REP_MEAN  10
#define GPIRT_RESID_S_PPP_ABSMAX       11
#define GPIRT_RESID_S_PPP_ABSMAX_MID   12
#define GPIRT_RESID_NSCALAR            13
/* the raw arrays of the state block, in its order: n_co (int64, m x m); undefined_count, rc_ge, rc_gt (uint32, m x m);
 * rc_obs_sum, rc_rep_sum, rc_rep_sumsq (double, m x m); ss_undefined, ss_ge, ss_gt (uint32, m); ss_obs_sum, ss_rep_sum (double,
 * m); global (16 words of 8 bytes) */
#define GPIRT_RESID_NRAW     13
/* HOST pointers (NULL: not wanted); every m x m array holds the pair (a, b) at [a m + b]. */
typedef struct gpirt_ppc_resid {
    int        top;                            /* in: 1..GPIRT_RESID_MAX_TOP */
    int        reserved0;                      /* must be 0 */
    double*    pair[GPIRT_RESID_NPAIR];        /* m x m each */
    double*    item[GPIRT_RESID_NITEM];        /* m each */
    void*      raw[GPIRT_RESID_NRAW];          /* the raw arrays, by their own types */
    int64_t*   worst_pairs;                    /* top x 2: a, b */
    double*    worst_ppp_rc_mid;               /* top */
    double*    worst_rc_obs_mean;              /* top */
    int64_t*   worst_items;                    /* top */
    double*    worst_ppp_ss_mid;               /* top */
    double     scalar[GPIRT_RESID_NSCALAR];    /* out */
    int64_t    n, m;                           /* out */
    int64_t    resid_draws, resid_skipped, global_undefined;     /* out */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_ppc_resid;
/* Stage API.  ppc_resid_enable(top in 1..GPIRT_RESID_MAX_TOP; 0 frees the state) allocates and zeroes the state on a sampler
 * with ppc_enable on and forms O and n_co (GPIRT_E_ARG, with a message that names the fault, without ppc_enable, on an item
 * shard, for top outside 0..64, m outside 2..4096 and n > 65534; ppc_enable called again frees it too).  From then on every
 * ppc_accumulate also adds the draw to the block.  ppc_resid_get copies one array by name to the host, `bytes` its exact size:
 * every finished pair or item array by the lower-case name above (double), "scalars" (double, 13), the raw arrays by theirs,
 * "counts" (int64: resid_draws, resid_skipped, global_undefined) and, of the last COUNTED draw, "d_obs", "d_rep", "w" (int32, n x
 * m, column-major as y is, rejoined from the digit planes), "digits" (int8, 9 x n x m: the planes of d_obs, d_rep, w, the low
 * digit first), "s_obs", "s_rep", "v" (int64, m x m), "r_obs", "r_rep" (double, m x m: the correlations, the infit on the
 * diagonal, NaN where undefined) and "stats" (double, 8: Q, M+, M of the data, Q, M+, M of the replicate, the defined pairs a <
 * b, 0).
 * ppc_resid_state returns the ONE device block of its own: a header of 8 int64 -- n, m, the layout version (1), resid_draws,
 * resid_skipped, item0, 0, the tag 0x31445352 ("RSD1") --, then the raw arrays in the order above; every array starts on a
 * 16-byte boundary. */
int gpirt_sampler_ppc_resid_enable(gpirt_sampler_t s, int top);
int gpirt_sampler_ppc_resid_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ppc_resid_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_ppc_resid_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_resid* out);

/* ------------------------------------------------------ Two-form score equating: joint table, concordance ------------- */
/* The sum-score section answers every question about ONE form's score.  This one is about TWO forms at once: how scores on
 * form X and form Y relate (IRT observed-score equating), what somebody who scored s on X scores on Y (the concordance table),
 * how well the two forms agree on a pass / fail decision, how two subscores correlate.  All follow from the joint distribution
 * of the two scores for the N(0, 1) population, per draw
 *     J[s, t] = sum_k w_k P(S_X = s | theta_k) P(S_Y = t | theta_k),
 * a product of two recursions under ONE draw integrated over theta: a mean of a product is not a product of means, so neither
 * two sum-score states (they keep the marginals) nor the IRFs determine it.  Library version 116.
 * The two FORMS are non-empty DISJOINT sets of item columns, each named by a mask of m bytes; 1 <= M_X, M_Y <=
 * GPIRT_EQUATE_MAX_ITEMS.  They must be disjoint because only then do the scores factorise given theta (anchor designs are out
 * of scope; so is true-score equating: a GP-IRT test characteristic curve need not be monotone, so it has no inverse).
 * Per draw, with the grid, the weights w_k (gpirt_sumscore_grid_weights, stored in the state), p, q and the recursion of the
 * sum-score section, each form's items in ascending column order, all in fp64:
 *   A_X[k, s], T_X[k], V_X[k] and A_Y[k, t], T_Y[k], V_Y[k]   exactly as the sum-score section forms A, T and V for each form;
 *   pi_X[s]   = sum_k w_k A_X[k, s], ascending k (the sum-score pi); pi_Y[t] likewise;
 *   J[s, t]   = sum_k (w_k A_X[k, s]) A_Y[k, t]: the weighted left operand is rounded once, the contraction is ONE product
 *               through the library's fp64 matrix-core GEMM, never split along k, so its order is fixed and the result is the
 *               same from run to run; both operands are padded along k to 1024 with zero rows, which add exact zeros.  The order
 *               of summation inside the product is the GEMM core's: any order of 1001 non-negative terms;
 *   F_X, F_Y  the cumulative sums of pi_X, pi_Y in ascending score;
 *   e_YX[s]   the equipercentile equivalent of the X score s on Y's scale (Kolen and Brennan's percentile-rank form), s = 0 ..
 *               M_X: P = F_X[s - 1] + pi_X[s] / 2 (F[-1] = 0), t* the smallest t with F_Y[t] > P,
 *               e_YX[s] = (t* - 0.5) + (P - F_Y[t* - 1]) / pi_Y[t*]; if no t qualifies e_YX[s] = M_Y + 0.5 and `eq_clamped`
 *               counts the cell.  e_XY[t], t = 0 .. M_Y, is the same with the roles swapped;
 *   r         with a_X = sum_k w_k T_X[k], b_X = sum_k w_k (V_X[k] + T_X[k] T_X[k]), a_Y and b_Y likewise and c = sum_k w_k
 *               (T_X[k] T_Y[k]), the five sums in ascending k: r = (c - a_X a_Y) / sqrt((b_X - a_X a_X) (b_Y - a_Y a_Y)), the
 *               correlation of the two scores.
 * A draw whose f* holds a NaN in a column of EITHER form is skipped WHOLE (`skipped` += 1, nothing else changes; the decision is
 * made on the device before anything is touched); a NaN in a column outside both forms is ignored; +-inf is fine (a point mass).
 * Every other draw adds 1 to `draws`.  A counted draw whose two variances b - a a are not both > 0 adds nothing to corr and 1 to
 * `corr_skipped`; any other adds 1 to `corr_draws`.
 * The accumulators:
 *   joint_sum[s, t] += J[s, t]           ((M_X + 1) x (M_Y + 1), cell (s, t) at [s (M_Y + 1) + t])
 *   pix_sum[s] += pi_X[s], pix_sumsq[s] += pi_X[s]^2;  piy_sum, piy_sumsq likewise
 *   eyx_sum[s] += e_YX[s], eyx_sumsq[s] += e_YX[s]^2 (M_X + 1);  exy_sum, exy_sumsq (M_Y + 1)
 *   corr[0] += r, corr[1] += r r;  corr_terms = (a_X, b_X, a_Y, b_Y, c) of the last counted draw
 *   last_joint, last_pix, last_piy, last_eyx, last_exy = J, pi_X, pi_Y, e_YX, e_XY of the last counted draw.
 * THE JOINT, NOT THE RATIO, as in the sum-score section: the concordance P(S_Y = t | S_X = s), its mean and quantiles, the
 * decision agreement and kappa at a pair of cut scores are linear in the joint or a ratio of it; the host computes them from the
 * pooled joint_sum, normalised once.  A row without mass gives NaN.
 * Every accumulator cell is owned by one thread: no atomics, a fixed order, byte-identical state blocks from run to run.
 * REFLECTION.  theta -> -theta changes none of these quantities: every sum runs over the whole symmetric grid.  So
 * gpirt_equate_combine takes no signs; pooling C chains adds the doubles and the counters in chain order, and the last_* arrays
 * and corr_terms are the last state's.  States with another m, other forms or other grid weights are refused.
 * Nothing is drawn: with the accumulators on, the chain, the IRFs, R's stream position and every other block's state are bit for
 * bit what they are without.
 * Device memory per state at M_X = M_Y = 1024: joint_sum and last_joint 8.4 MB each, the two A tables and the weighted copy
 * 8.4 MB each, the two (p, q) tables 16.4 MB each. */
#define GPIRT_EQUATE_MAX_ITEMS        2048
/* the raw arrays of a state block, in the block's order */
#define GPIRT_EQUATE_JOINT_SUM        0       /* double [M_X + 1][M_Y + 1] */
#define GPIRT_EQUATE_PIX_SUM          1       /* double [M_X + 1] */
#define GPIRT_EQUATE_PIX_SUMSQ        2       /* double [M_X + 1] */
#define GPIRT_EQUATE_PIY_SUM          3       /* double [M_Y + 1] */
#define GPIRT_EQUATE_PIY_SUMSQ        4       /* double [M_Y + 1] */
#define GPIRT_EQUATE_EYX_SUM          5       /* double [M_X + 1] */
#define GPIRT_EQUATE_EYX_SUMSQ        6       /* double [M_X + 1] */
#define GPIRT_EQUATE_EXY_SUM          7       /* double [M_Y + 1] */
#define GPIRT_EQUATE_EXY_SUMSQ        8       /* double [M_Y + 1] */
#define GPIRT_EQUATE_CORR             9       /* double [2]: sum r, sum r^2 */
#define GPIRT_EQUATE_CORR_TERMS       10      /* double [5]: a_X, b_X, a_Y, b_Y, c of the last counted draw */
#define GPIRT_EQUATE_MASK_X           11      /* unsigned char [m]: 1 where the item is in form X */
#define GPIRT_EQUATE_MASK_Y           12      /* unsigned char [m] */
#define GPIRT_EQUATE_W                13      /* double [1001]: the grid weights */
#define GPIRT_EQUATE_LAST_JOINT       14      /* double [M_X + 1][M_Y + 1] */
#define GPIRT_EQUATE_LAST_PIX         15      /* double [M_X + 1] */
#define GPIRT_EQUATE_LAST_PIY         16      /* double [M_Y + 1] */
#define GPIRT_EQUATE_LAST_EYX         17      /* double [M_X + 1] */
#define GPIRT_EQUATE_LAST_EXY         18      /* double [M_Y + 1] */
#define GPIRT_EQUATE_NARRAYS          19
/* HOST pointers (NULL: not wanted): the pooled raw arrays, each of the size and type named above. */
typedef struct gpirt_equate {
    const unsigned char* x;                    /* in (gpirt_mcmc_run): m bytes, non-zero = in form X */
    const unsigned char* y;                    /* in (gpirt_mcmc_run): m bytes, non-zero = in form Y */
    void*      raw[GPIRT_EQUATE_NARRAYS];
    int64_t    m, Mx, My;                      /* out */
    int64_t    draws, skipped, corr_draws, corr_skipped, eq_clamped;   /* out */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_equate;
/* Stage API.  equate_enable(mask_x, mask_y, on != 0) allocates and zeroes the state for the two forms (m bytes each, non-zero =
 * in the form); GPIRT_E_ARG with a message for a missing mask, an overlap (the first shared column is named), an empty form and
 * more than GPIRT_EQUATE_MAX_ITEMS items, the old state is then kept; on = 0 frees it.  equate_accumulate adds the CURRENT f*
 * (the sampler array "fstar") as one draw.  equate_get copies one array by name to the host, `bytes` its exact size: the
 * lower-case names of the raw arrays ("joint_sum", "pix_sum", ..., "last_exy") and "counts" (int64: draws, skipped, corr_draws,
 * corr_skipped, eq_clamped).  equate_state returns the ONE device block (valid until equate_enable is called again or the
 * sampler goes): a header of 16 int64 -- the tag 0x45545145 ("EQTE"), the layout version (1), m, M_X, M_Y, N = 1001, draws,
 * skipped, corr_draws, corr_skipped, eq_clamped, 0 ... -- then the raw arrays in the order above, every array starting on a
 * 16-byte boundary; gpirt_equate_state_bytes gives its size. */
int gpirt_sampler_equate_enable(gpirt_sampler_t s, const unsigned char* mask_x, const unsigned char* mask_y, int on);
int gpirt_sampler_equate_accumulate(gpirt_sampler_t s);
int gpirt_sampler_equate_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_equate_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_equate_state_bytes(int64_t m, int64_t Mx, int64_t My, int64_t* bytes);
int gpirt_equate_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_equate* out);

/* ------------------------------------------------------ PSIS-LOO: pointwise elpd, Pareto k, model comparison ----------- */
/* Leave-one-out cross-validation by Pareto-smoothed importance sampling (Vehtari, Gelman and Gabry 2017; Vehtari, Simpson,
 * Gelman, Yao and Gabry 2024) for every observed cell, without stored draws.  Library version 117.
 * For an observed cell (i, j) and a draw s, with the sampler's own arrays f and mu:
 *   g = f + mu (one fp64 add, as WAIC forms it), a = y g, the KEY kappa_s = -a (exact: a product with +-1 and a sign);
 *   the importance ratio r_s = 1 / p(y | draw) = 1 + exp(kappa_s), and p_s = 1 / r_s.
 * T is the number of draws that will be pooled (chains times draws per chain), fixed when the state is made.  The tail length
 * is M = min(floor(T / 5), ceil(3 sqrt(T))) unless `tail` (5 .. GPIRT_LOO_MAX_TAIL) replaces the rule; M > GPIRT_LOO_MAX_TAIL
 * and M >= T are argument errors that say so.  K = M + 1.
 * PER DRAW AND CELL a state keeps
 *   keys          the K largest keys entered so far (equal keys are interchangeable: the kept multiset is unique), as a binary
 *                 min-heap per cell, slot-major (slot z of cell c at [z cells + c], c = i + j n), the smallest kept key in slot 0;
 *   evicted_sum, evicted_sumsq   the sums of r and r^2 over every key that is not, or is no longer, kept, added in draw order at
 *                 the moment the key is refused (it does not exceed the smallest kept key) or pushed out (the smallest kept key
 *                 leaves for a larger one): the non-tail sum is never formed by subtraction;
 *   p_sum         the sum of p_s;
 *   count, nonfinite   a draw whose g is not finite in the cell, or whose key exceeds GPIRT_LOO_KEY_MAX = 700, is not entered
 *                 and adds 1 to `nonfinite`; every other draw adds 1 to `count`.  A missing cell (y NaN) keeps nothing.
 * One thread owns a cell: no atomics, a fixed order, byte-identical state blocks from run to run.
 * POOLING.  The keys kept by the next chain's state are entered into the pooled heap in slot order, by the same rule; its
 * evicted sums are added first, then r and r^2 of whatever the pooled heap refuses or pushes out; p_sum and the counters add.
 * theta -> -theta does not change g, so pooling takes no signs.  States of another n, m, T, M or y are refused.
 * FINISHING, per cell.  A cell with count == T and nonfinite == 0 is finished; any other observed cell gets NaN outputs and is
 * counted in `cells_incomplete`.
 *   1. The kept keys in ascending order: the smallest is the cutoff kappa_c, the other M are the tail kappa_(1) <= ... <=
 *      kappa_(M) = kmax.
 *   2. x_z = exp(kappa_(z) - kmax) - exp(kappa_c - kmax), the exceedances in units of exp(kmax) (the "1 +" cancels).
 *   3. M < 5 or x_M <= 0: the cell is UNSMOOTHED (pareto_k = NaN, the raw ratios are used, counted in `unsmoothed`).
 *   4. Else the generalised Pareto fit of Zhang and Stephens (2009) as PSIS uses it: mgrid = 30 + floor(sqrt(M)), x* = x at the
 *      1-based position floor(M / 4 + 0.5); for j = 1 .. mgrid
 *        theta_j = 1 / x_M + (1 - sqrt(mgrid / (j - 0.5))) / (3 x*),   k_j = mean_z log1p(-theta_j x_z),
 *        l_j = M (log(-theta_j / k_j) - k_j - 1),   w_j = 1 / sum_i exp(l_i - l_j);
 *      theta^ = sum_j theta_j w_j, k = mean_z log1p(-theta^ x_z), sigma = -k / theta^, then k <- (k M + 5) / (M + 10).
 *      A fit whose k or sigma is not finite (x* = 0: a quarter of the tail ties with the cutoff) leaves the cell unsmoothed too.
 *   5. q_z = sigma expm1(-k log1p(-(z - 1/2) / M)) / k + exp(kappa_c - kmax), capped at 1 (the largest raw ratio);
 *      w~_z = exp(-kmax) + q_z (unsmoothed: w~_z = rho_z), and the raw rho_z = exp(-kmax) + exp(kappa_(z) - kmax).
 *   6. With E = evicted_sum + r(kappa_c), E2 = evicted_sumsq + r(kappa_c)^2, W = E exp(-kmax) + sum_z w~_z:
 *        elpd_loo  = log((T - M) + sum_z w~_z / rho_z) - log(W) - kmax      (W is in units of exp(kmax));
 *        n_eff     = W^2 / ((E2 exp(-kmax)) exp(-kmax) + sum_z w~_z^2);
 *        lppd      = log(p_sum / T);   p_loo = lppd - elpd_loo;
 *        loo_p_yes = exp(elpd_loo) for a yes cell, 1 - exp(elpd_loo) for a no cell.
 *      The sums over z are 64 interleaved partial sums (z = 1 + lane, 65 + lane, ...) added in lane order.
 * TOTALS over the finished cells (block partials reduced in a fixed order): elpd_loo, se_elpd_loo = sqrt(N var) (ddof 1),
 * p_loo, looic = -2 elpd_loo, se_looic = 2 se_elpd_loo, n_obs = N, lppd, k_threshold = min(1 - 1 / log10(T), 0.7), and the
 * counts k_good (k <= threshold), k_bad (threshold < k <= 1), k_very_bad (k > 1), unsmoothed, cells_incomplete.
 * item_elpd_loo (m) and respondent_elpd_loo (n) are sums over the finished cells of a column / a row.  worst: the `top` cells
 * with the largest pareto_k, ties to the lowest column-major index; index -1 and k NaN where fewer cells have a k.
 * Nothing is drawn: with the accumulators on, the chain, the IRFs, R's stream position and every other block's state are bit
 * for bit what they are without.
 * Device memory per state: (8 K + 32) bytes per cell, plus one byte per cell for the copy of y. */
#define GPIRT_LOO_MAX_TAIL            1024
#define GPIRT_LOO_MAX_TOP             64
#define GPIRT_LOO_KEY_MAX             700.0
/* the raw arrays of a state block, in the block's order */
#define GPIRT_LOO_KEYS                0       /* double [K][n m]: the heaps, slot-major */
#define GPIRT_LOO_EVICTED_SUM         1       /* double [n m] */
#define GPIRT_LOO_EVICTED_SUMSQ       2       /* double [n m] */
#define GPIRT_LOO_P_SUM               3       /* double [n m] */
#define GPIRT_LOO_COUNT               4       /* int32 [n m] */
#define GPIRT_LOO_NONFINITE           5       /* int32 [n m] */
#define GPIRT_LOO_Y                   6       /* signed char [n m]: +1, -1, 0 for a missing cell */
#define GPIRT_LOO_NARRAYS             7
/* the pointwise outputs (double [n m] each, NaN for a missing or an incomplete cell) */
#define GPIRT_LOO_PW_PARETO_K         0
#define GPIRT_LOO_PW_ELPD_LOO         1
#define GPIRT_LOO_PW_N_EFF            2
#define GPIRT_LOO_PW_LPPD             3
#define GPIRT_LOO_PW_P_LOO            4
#define GPIRT_LOO_PW_LOO_P_YES        5
#define GPIRT_LOO_NPOINTWISE          6
/* totals */
#define GPIRT_LOO_T_ELPD_LOO          0
#define GPIRT_LOO_T_SE_ELPD_LOO       1
#define GPIRT_LOO_T_P_LOO             2
#define GPIRT_LOO_T_LOOIC             3
#define GPIRT_LOO_T_SE_LOOIC          4
#define GPIRT_LOO_T_N_OBS             5
#define GPIRT_LOO_T_LPPD              6
#define GPIRT_LOO_T_K_THRESHOLD       7
#define GPIRT_LOO_T_K_GOOD            8
#define GPIRT_LOO_T_K_BAD             9
#define GPIRT_LOO_T_K_VERY_BAD        10
#define GPIRT_LOO_T_UNSMOOTHED        11
#define GPIRT_LOO_T_CELLS_INCOMPLETE  12
#define GPIRT_LOO_T_ELPD_MEAN         13
#define GPIRT_LOO_NTOTALS             14
/* HOST pointers (NULL: not wanted). */
typedef struct gpirt_loo {
    int64_t    tail;                           /* in (gpirt_mcmc_run): 0 = the rule, else 5 .. GPIRT_LOO_MAX_TAIL */
    int64_t    top;                            /* in: 1 .. GPIRT_LOO_MAX_TOP, the length of worst_index / worst_k */
    void*      raw[GPIRT_LOO_NARRAYS];         /* the pooled raw arrays, each of the size and type named above */
    double*    pointwise[GPIRT_LOO_NPOINTWISE];
    double*    item_elpd_loo;                  /* m */
    double*    respondent_elpd_loo;            /* n */
    int64_t*   worst_index;                    /* top */
    double*    worst_k;                        /* top */
    double     totals[GPIRT_LOO_NTOTALS];      /* out */
    int64_t    n, m, T, M, draws, chains;      /* out: draws = accumulate calls pooled, chains = states pooled */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_loo;
/* Stage API.  loo_enable(planned_total_draws = T >= 1, tail = 0 or 5 .. 1024, on != 0) allocates and zeroes the state (a bad
 * tail, M > GPIRT_LOO_MAX_TAIL and M >= T are GPIRT_E_ARG with a message, the old state is then kept); on = 0 frees it.
 * loo_accumulate enters the CURRENT f + mu as one draw.  loo_get copies one array by name to the host, `bytes` its exact size:
 * "keys", "evicted_sum", "evicted_sumsq", "p_sum", "count", "nonfinite", "y" and "counts" (int64: n, m, T, M, draws, chains).
 * loo_state returns the ONE device block (valid until loo_enable is called again or the sampler goes): a header of 16 int64 --
 * the tag 0x4F4F4C50 ("PLOO"), the layout version (1), n, m, T, M, draws, chains, 0 ... -- then the raw arrays in the order
 * above, every array starting on a 16-byte boundary; gpirt_loo_state_bytes gives its size.  gpirt_loo_combine pools the states
 * in order on the device (one pooled copy beside the callers' states; none for one state) and finishes. */
int gpirt_sampler_loo_enable(gpirt_sampler_t s, int64_t planned_total_draws, int tail, int on);
int gpirt_sampler_loo_accumulate(gpirt_sampler_t s);
int gpirt_sampler_loo_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_loo_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_loo_tail_length(int64_t T, int tail, int64_t* M);
int gpirt_loo_state_bytes(int64_t n, int64_t m, int64_t M, int64_t* bytes);
int gpirt_loo_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_loo* out);

/* ------------------------------------------------------ Item-pair IRF order posteriors: dominance and crossings -------- */
/* The shape posteriors say, item by item, whether a curve is monotone.  Whether the curves of two items INTERSECT -- whether the
 * items have an invariant ordering (Sijtsma and Junker 1996) -- is a joint functional of two smooth curves gbar[:, a] and
 * gbar[:, b] of one draw.  This block sits on top of the shape block: it reads the same gbar, the same window W = [k_lo, k_hi],
 * the same tolerances and the bad[] flags the shape's item kernel writes.  2 <= m <= GPIRT_ORDER_MAX_M.
 * Per counted draw, in fp64 (comparing P_a with P_b is comparing g_a with g_b, plogis being monotone):
 *   U[a, b] = max over k in W of fl(g[k, a] - g[k, b]), a != b; the minimum over W is L = -U[b, a] exactly (fl(x - y) = -fl(y - x)).
 *   For each tolerance t and ordered pair (a, b):  cross[t, a, b] += 1 where U > t and L < -t (symmetric);
 *   above[t, a, b] += 1 where U > t and L >= -t (a above b); where U <= t and L < -t it is above[t, b, a] that gains; the
 *   remainder is tied.  depth_sum[a, b] += min(max(U, 0), max(-L, 0)): the depth of the crossing in logits, symmetric, added
 *   in draw order.  All of it is max, min, comparisons and ONE subtraction: the same bits in any order.
 *   Easiness e_j = sum over the WHOLE grid of w_k / (1 + exp(-g[k, j])), w the shape block's normalised N(0, 1) weights; lane t
 *   of 256 adds its k = 4t .. 4t + 3 in order, the 256 partial sums are added in ascending t.  easiness[0, j] += e_j,
 *   easiness[1, j] += e_j e_j; easier[a, b] += 1 where e_a > e_b (the device's own e).
 *   n_cross[t] = the unordered pairs that cross at t in this draw: set_counts[0, t] += (n_cross == 0) (iio_draws),
 *   set_counts[1, t] += n_cross, set_counts[2, t] += n_cross n_cross (uint64).
 * A draw in which ANY item's curve holds a non-finite value anywhere on the grid is skipped whole (inf - inf would poison a row
 * of pairs): skipped += 1 and nothing else changes; otherwise draws += 1.  The diagonal cells are never touched (0).
 * One owner per cell, no atomics: the state is byte-identical from run to run.  theta -> -theta changes nothing here (W and w
 * are symmetric), so pooling chains is plain addition in chain order.
 * Device memory per state: (8 n_tols + 12) m m bytes of accumulators and 8 m m for u: 38 MB + 8 MB = 46 MB at m = 1024 with
 * three tolerances, 0.60 GB + 0.13 GB = 0.74 GB at m = 4096. */
#define GPIRT_ORDER_MAX_M        4096
#define GPIRT_ORDER_MAX_TOP      64
/* the raw arrays of a state block, in the block's order */
#define GPIRT_ORDER_ABOVE        0       /* uint32 [n_tols][m][m] */
#define GPIRT_ORDER_CROSS        1       /* uint32 [n_tols][m][m] */
#define GPIRT_ORDER_EASIER       2       /* uint32 [m][m] */
#define GPIRT_ORDER_DEPTH_SUM    3       /* double [m][m] */
#define GPIRT_ORDER_EASINESS     4       /* double [2][m]: sum e, sum e^2 */
#define GPIRT_ORDER_SET_COUNTS   5       /* uint64 [3][GPIRT_SHAPE_MAX_TOLS]: iio_draws, cross_pairs_sum, cross_pairs_sumsq */
#define GPIRT_ORDER_NARRAYS      6
/* HOST pointers (NULL: not wanted): the pooled raw arrays, each of the size and type named above. */
typedef struct gpirt_shape_order {
    int        top;                            /* in: 1..GPIRT_ORDER_MAX_TOP, the length of worst_a / worst_b */
    int        k_half, n_tols;                 /* out: the states' */
    double     tols[GPIRT_SHAPE_MAX_TOLS];     /* out */
    void*      raw[GPIRT_ORDER_NARRAYS];
    int64_t*   worst_a;                        /* top: the pairs a < b with the largest cross count at the largest tolerance, */
    int64_t*   worst_b;                        /*      ties to the lowest (a, b); -1 beyond n_worst */
    int64_t    n_worst;                        /* out: min(top, m (m - 1) / 2) */
    int64_t    n, m, draws, skipped;           /* out */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_shape_order;
/* Stage API.  shape_order_enable(on != 0) allocates and zeroes the block beside a shape state that is on (GPIRT_E_ARG with a
 * message when the shape posteriors are off or m is outside 2..GPIRT_ORDER_MAX_M; on = 0 frees it).  gpirt_sampler_shape_enable
 * drops the block with the shape state it belongs to.  From then on gpirt_sampler_shape_accumulate also runs the order kernels,
 * behind the shape's own, on the same gbar.  shape_order_get copies one array by name, `bytes` its exact size: "above", "cross",
 * "easier", "depth_sum", "easiness", "set_counts", "counts" (int64: draws, skipped) and, of the last counted draw, "u" (double
 * [m][m], the diagonal 0), "e" (double [m]) and "ncross" (int64 [GPIRT_SHAPE_MAX_TOLS]).  shape_order_state returns the ONE device
 * block: a header of 16 int64 -- the tag 0x5244524F ("ORDR"), the layout version (1), n, m, k_half, n_tols, the four tolerances'
 * bits, draws, skipped, 0, 0, 0, 0 -- then the raw arrays in the order above, every array starting on a 16-byte boundary;
 * gpirt_shape_order_state_bytes gives its size.  gpirt_shape_order_combine adds the integers and adds the doubles in chain order;
 * states with another m, window or tolerances than state 0 are refused. */
int gpirt_sampler_shape_order_enable(gpirt_sampler_t s, int on);
int gpirt_sampler_shape_order_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_shape_order_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_shape_order_state_bytes(int64_t m, int n_tols, int64_t* bytes);
int gpirt_shape_order_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_shape_order* out);

/* ------------------------------------------------------ autocorrelation ESS: lag sums, Geyer tau, MCSE ---------------- */
/* The lag-window estimate of the effective sample size (Geyer's 1992 initial monotone sequence over split chains, the rule
 * Stan, `posterior` and ArviZ users know as ESS) for tracked scalar series of the chain, without stored draws: only the last
 * L + 1 draws of each value are kept, in a ring.  Library version 122.  Stage API only: gpirt_run has no field for it yet.
 * SERIES, chosen by the bit mask `parts`, in this order (P values in all):
 *   GPIRT_ACF_THETA   n values, the INTEGER section: a theta draw is a grid point -5 + 0.01 k;
 *   GPIRT_ACF_BETA    2m values in the order of the array beta (value 2j + r is row r of item j; r = 1 is the slope);
 *   GPIRT_ACF_LL      m + n + 1 values: item_ll[j], resp_ll[i], total_ll, from the sampler's own f, mu and y.
 * LOG-LIKELIHOOD.  For an observed cell g = f + mu (one fp64 add) and cell = -(log1p(exp(-|g|)) + fmax(-y g, 0)), WAIC's
 * expression; a missing cell and a row past n enter as 0.0.  Work-group (b, q) owns rows 256 b .. 256 b + 255 and columns
 * 32 q .. 32 q + 31.  Its lane of row i adds the cells of its columns in ascending j: R[q][i].  For each column the 256 rows
 * are summed by a fixed tree: in each wave of 64 rows v[l] += v[l + o] for o = 32, 16, 8, 4, 2, 1, then (w0 + w1) + (w2 + w3)
 * over the four waves: C[b][j].  resp_ll[i] = sum over q ascending of R[q][i]; item_ll[j] = sum over b ascending of C[b][j];
 * total_ll = sum over j ascending of item_ll[j].  No atomics.
 * HALVES.  S = the chain's planned draws, H = floor(S / 2); half 1 is draws 1 .. H, half 2 the last H draws; with S odd the
 * middle draw enters nothing.  Each half is a series of its own with t = 1 .. H; the ring restarts at half 2's first draw.
 * 4 <= H, 1 <= L <= min(H - 1, GPIRT_ACF_MAX_LAG); max_lag = 0 asks for L = min(H - 1, GPIRT_ACF_DEFAULT_LAG).
 * RAW ARRAYS, for half h, lag k = 0 .. L and value p (value fastest): d_t = x_t - centre[p]; for theta d_t = k_t - 500 as an
 * integer (centre 0) and every theta array but `centre` is int64; for the others centre[p] is the value at the chain's first
 * draw (0 if that is not finite) and d_t is one fp64 subtraction.  A non-finite value -- for theta also one off the grid, by
 * the rule of GPIRT_SUM_THETA_HIST: k = rint((x + 5) 100) outside 0 .. 1000 or -5 + 0.01 k != x -- adds 1 to nonfinite[p] and
 * enters as d_t = 0.
 *   s[h][k][p]    = sum_{t = k+1 .. H} d_t d_{t-k}, one product and one add per term, added in ascending t;
 *   sum[h][p]     = sum_t d_t in ascending t;
 *   head[h][k][p] = the running sum after the first k draws;
 *   tail[h][k][p] = d_H + d_{H-1} + ... + d_{H-k+1}, added in that order (written from the ring at the half's last draw);
 *   centre[p], nonfinite[p] (int64).
 * Every cell has one owner and no sum is contracted, so a sequential NumPy loop reproduces the arrays bit for bit.
 * FINISH (gpirt_acf_combine), in fp64, one thread per value, over the 2C half-chains c in the order chain 0 half 1, chain 0
 * half 2, chain 1 half 1, ...: dbar = sum / H,
 *   gamma_{k,c} = [s_k - dbar ((sum - tail_k) + (sum - head_k)) + (H - k) dbar^2] / H,
 *   W = mean_c gamma_{0,c} H / (H - 1),  var+ = W (H - 1) / H + var(centre + dbar over c, ddof 1),
 *   rho_0 = 1, rho_k = 1 - (W - mean_c gamma_{k,c}) / var+.
 * Geyer's pairs P_j = rho_{2j} + rho_{2j+1}, 2j + 1 <= L: stop at the first P_j <= 0, else P_j <- min(P_j, P_{j-1}); tau = -1 +
 * 2 sum P_j; lag_used = 2j + 1 of the last pair that entered (0: none); truncated = 1 when the lags ran out with P_j > 0;
 * tau <- max(tau, 1 / log10 N), N = 2 C H; ess = N / tau, mcse = sqrt(var+ / ess), rhat = sqrt(var+ / W), rho1 = rho_1,
 * mean = the mean over c of centre + dbar, sd = sqrt(var+).  constant = 1 when W = 0 or var+ = 0 or either is not finite:
 * ess, tau, mcse, rhat and rho1 are then NaN, lag_used and truncated 0 and the value's acf column NaN.  acf[k][p] = rho_k.
 * BLOCKS theta, beta, item_ll, resp_ll, total_ll: min_ess, max_tau, max_rhat over the values that are not NaN (NaN if none),
 * n_truncated, n_nan (values whose ess is NaN).  worst: the `top` values with the smallest ess, ties to the lowest p; block -1
 * and ess NaN where fewer values have an ess.
 * REFLECTION.  A chain with sign -1 enters with theta's sum, head and tail negated, the beta slopes' sum, head, tail and centre
 * negated; s and the log-likelihood series are untouched.  That is exactly the chain with every draw negated.
 * Nothing is drawn: with the block on, the chain, the IRFs, R's stream position and every other block's state are bit for bit
 * what they are without.  Device memory per state: 8 bytes x (7 (L + 1) P + 4 P), plus 8 (ceil(n / 256) m + ceil(m / 32) n). */
#define GPIRT_ACF_THETA               1
#define GPIRT_ACF_BETA                2
#define GPIRT_ACF_LL                  4
#define GPIRT_ACF_MAX_LAG             1024
#define GPIRT_ACF_DEFAULT_LAG         256
#define GPIRT_ACF_MAX_TOP             64
/* the raw arrays of a state block, in the block's order (8-byte elements; the theta columns of the first four are int64) */
#define GPIRT_ACF_S                   0       /* [2][L + 1][P] */
#define GPIRT_ACF_SUM                 1       /* [2][P] */
#define GPIRT_ACF_HEAD                2       /* [2][L + 1][P] */
#define GPIRT_ACF_TAIL                3       /* [2][L + 1][P] */
#define GPIRT_ACF_CENTRE              4       /* double [P] */
#define GPIRT_ACF_NONFINITE           5       /* int64 [P] */
#define GPIRT_ACF_RING                6       /* [L + 1][P]: d_t at slot (t - 1) mod (L + 1); theta's as int64 */
#define GPIRT_ACF_NARRAYS             7
/* per value */
#define GPIRT_ACF_V_ESS               0
#define GPIRT_ACF_V_TAU               1
#define GPIRT_ACF_V_MCSE              2
#define GPIRT_ACF_V_RHAT              3
#define GPIRT_ACF_V_RHO1              4
#define GPIRT_ACF_V_MEAN              5
#define GPIRT_ACF_V_SD                6
#define GPIRT_ACF_NVALUE              7
#define GPIRT_ACF_F_LAG_USED          0
#define GPIRT_ACF_F_TRUNCATED         1
#define GPIRT_ACF_F_NONFINITE         2       /* summed over the chains */
#define GPIRT_ACF_F_CONSTANT          3
#define GPIRT_ACF_NFLAG               4
/* per block */
#define GPIRT_ACF_NBLOCK              5       /* theta, beta, item_ll, resp_ll, total_ll */
#define GPIRT_ACF_B_MIN_ESS           0
#define GPIRT_ACF_B_MAX_TAU           1
#define GPIRT_ACF_B_MAX_RHAT          2
#define GPIRT_ACF_NBSTAT              3
#define GPIRT_ACF_C_TRUNCATED         0
#define GPIRT_ACF_C_NAN               1
#define GPIRT_ACF_NBCOUNT             2
/* HOST pointers (NULL: not wanted). */
typedef struct gpirt_acf {
    int64_t    top;                            /* in: 1 .. GPIRT_ACF_MAX_TOP, the length of the worst_* arrays */
    double*    value[GPIRT_ACF_NVALUE];        /* P each */
    int64_t*   flag[GPIRT_ACF_NFLAG];          /* P each */
    double*    acf;                            /* (L + 1) x P, value fastest */
    int64_t*   worst_block;                    /* top: 0 theta, 1 beta, 2 item_ll, 3 resp_ll, 4 total_ll */
    int64_t*   worst_index;                    /* top: the index inside the block */
    double*    worst_ess;                      /* top */
    double     block_stat[GPIRT_ACF_NBLOCK * GPIRT_ACF_NBSTAT];     /* out: [block][stat]; NaN for a block that is not tracked */
    int64_t    block_count[GPIRT_ACF_NBLOCK * GPIRT_ACF_NBCOUNT];   /* out: [block][count] */
    int64_t    n, m, parts, S, H, L, P, chains;                     /* out */
    int64_t    reserved[4];                    /* must be 0 */
} gpirt_acf;
/* gpirt_acf_check is the argument check alone (no device is touched): parts a non-empty subset of the three bits, H >= 4,
 * max_lag 0 or 1 .. min(H - 1, GPIRT_ACF_MAX_LAG); each refusal says which.  L_out, P_out: may be NULL.
 * Stage API.  acf_enable(parts, planned_draws, max_lag, on != 0) allocates and zeroes the state (a refused argument keeps the
 * old state); on = 0 frees it.  acf_accumulate enters the CURRENT theta, beta, f and mu as the chain's next draw; one beyond
 * the planned draws is GPIRT_E_ARG and says so.  acf_get copies one array by name to the host, `bytes` its exact size: "s",
 * "sum", "head", "tail", "centre", "nonfinite", "ring", "counts" (int64: n, m, parts, S, H, L, P, draws) and "last" (double [P]:
 * the values x_t of the last accumulate as they were read, before centring; what the log-likelihood pass is tested by).  acf_state returns the ONE device block (valid until acf_enable is called again or the sampler
 * goes): a header of 16 int64 -- the tag 0x31464341 ("ACF1"), the layout version (1), n, m, parts, S, H, L, P, draws, 0 ... --
 * then the raw arrays in the order above, each on a 16-byte boundary.  gpirt_acf_combine finishes `chains` such blocks of the
 * same n, m, parts, S and L, each with all S draws in, on the device; signs: NULL (all +1) or `chains` values of +1 / -1. */
int gpirt_acf_check(int64_t n, int64_t m, int parts, int64_t planned_draws, int64_t max_lag, int64_t* L_out, int64_t* P_out);
int gpirt_sampler_acf_enable(gpirt_sampler_t s, int parts, int64_t planned_draws, int64_t max_lag, int on);
int gpirt_sampler_acf_accumulate(gpirt_sampler_t s);
int gpirt_sampler_acf_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_acf_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_acf_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_acf* out);

/* ------------------------------------------------------ the kernel's length scale as a parameter of the chain ---------- */
/* Library version 125.  One length scale ell, shared by all items, is updated INSIDE the chain so that theta, the IRFs and
 * every analysis block average over it; the family stays the handle's, there is still no signal variance.  Stage API only:
 * gpirt_sampler_step, gpirt_mcmc_run and the whole-call entries do not know it, and a sampler on which
 * gpirt_sampler_ell_enable was never called (or was called with on = 0) computes bit for bit what it did before.
 *
 * ell lives on a fixed logarithmic grid, ell_k = lo (hi / lo)^(k / (P - 1)), k = 0 .. P - 1, 2 <= P <= GPIRT_ELL_MAX_POINTS,
 * GPIRT_LENGTH_SCALE_MIN <= lo < hi <= GPIRT_LENGTH_SCALE_MAX: computed once on the host in long double, rounded to fp64, the
 * end points exact (gpirt_ell_grid; a grid that is not strictly increasing in fp64 is refused).  The chain's state is the
 * index k.  log_prior[k] (P finite doubles) is a mass on the grid, i.e. a density with respect to log ell; NULL: the default
 * -(ln ell_k)^2 / 2, a log-normal with median 1 and log-sd 1.
 *
 * gpirt_sampler_draw_ell is the prior-whitened Metropolis step of Murray & Adams (2010, section 2.2): nu = L(ell_k)^-1 f is
 * held fixed, not f; theta, beta and mu are held fixed; L is the sampler's current factor of K(theta, theta; ell_k) + jitter.
 *   t        the number of draw_ell calls on this sampler so far, counted from 1
 *   u0, u1   item_uniform(seed, t, GPIRT_ST_ELL, 0, 0) and (.., 0, 1): what gpirt_item_uniforms(h, seed, t, 9, 0, 1, 2, .) writes
 *   j = min(floor(u0 2w), 2w - 1), d = j - w for j < w, else j - w + 1; k' = k + d (width 1 <= w <= P - 1).  k' outside
 *   0 .. P - 1: rejected and counted in out_of_range, nothing else runs (the proposal is symmetric).
 *   nu = L^-1 f (all n x m values); S under ell_k' is built and factored (ONE factorisation per update); f' = L' nu.
 *   dll = sum over observed cells of [t(y (f + mu)) - t(y (f' + mu))], t(a) = log(1 + exp(-a)) in the form of csrc/ll_fast.h,
 *   formed cell by cell as a difference of terms; per item in a fixed order (256 threads over ascending rows, a fixed tree),
 *   then over the items in ascending order: deterministic.  Cells with NaN y are skipped.
 *   accepted iff log(u1) < dll + log_prior[k'] - log_prior[k].
 *   Accepted: f <- f', k <- k', the sampler's kernel is ell_k'; L, the rows below it and the cached products are bit for bit
 *   what gpirt_sampler_factor leaves for (theta, ell_k').  Rejected, out of range or failed: f, L, the rows below it, theta,
 *   beta, mu and the sampler's kernel are byte-identical to before the call; only the counters move.  A proposal whose factor
 *   reports a non-positive minor, or whose f' or dll is not finite, is rejected and counted in `failed`: not an error.
 * A call that returns an error (a HIP error, a hang-guard expiry that could not be repaired) has not happened: it is not
 * counted, t does not advance, and updates = accepted + rejected + out_of_range + failed always.  A factor nobody has checked
 * yet (gpirt_sampler_step directly before) is checked first, a hang-guard expiry in it repaired as gpirt_sampler_check does.
 * The host reads the decision once per update (4 bytes and a stream synchronisation).  The handle's kernel
 * (gpirt_kernel_get) is not touched: it stays what new samplers of the handle start from.
 *
 * gpirt_ell_check touches no device: every refusal of gpirt_sampler_ell_enable (GPIRT_E_ARG, the message names the reason) --
 * the grid, a non-finite log_prior, width outside 1 .. P - 1, k0 outside -1 .. P - 1 (-1: the index of the handle's length
 * scale); with opts: GPIRT_RNG_RSTREAM (R's stream has no such draw), kernel_fp32, an item shard (item0 != 0 or
 * m_total != m); with kern: a length_scale that is not a point of the grid, and a kstar_rank > 0 whose gpirt_kernel_check
 * certificate fails at ell_0 = lo (the certificate grows as the length scale shrinks; a Matern family needs kstar_rank = 0).
 * kern and opts may be NULL (those checks are skipped).
 *
 * gpirt_sampler_ell_enable (after gpirt_sampler_init) applies that check to the sampler's own kernel and options, keeps the
 * tables, zeroes the counters (not t: the call count runs over the sampler's life, so enabling again never replays a pair of
 * uniforms), sets the sampler's kernel to ell_k0 and factors (nothing is factored when ell_k0 is the
 * length scale it already has).  on = 0 frees the state and leaves the sampler's kernel as it is.
 * gpirt_sampler_ell_get, by name: "grid", "log_prior" (P doubles), "index" (1 int64), "counts" (4 int64: updates, accepted,
 * out_of_range, failed) and, of the last update that reached the device, "nu", "f_prop" (n x m doubles), "delta" (m doubles)
 * and "record" (5 doubles: dll, log_ratio, log_u, accept, nonfinite); "times" (GPIRT_ELL_PARTS doubles, milliseconds of device
 * time of that update's parts with gpirt_sampler_enable_timing on, else 0: the copies f -> nu's buffer and factor buffer ->
 * saved buffer, the solve, the build and factorisation, the product, the delta, decide and commit kernels, the copy back after
 * a rejection).
 *
 * Library version 126: gpirt_sampler_draw_ell_centred, the companion move of the same paper (section 2.1): f is held fixed, not
 * nu, and the GP prior decides -- p(k | f, theta) is proportional to prod_j N(f_j; 0, S_k) exp(log_prior[k]); the likelihood
 * does not enter, since f does not move.  It needs gpirt_sampler_ell_enable, takes the same refusals and is held to the same
 * contract as gpirt_sampler_draw_ell; gpirt_sampler_draw_ell itself, its uniforms, decisions and counters are untouched by it,
 * and a sampler that never calls it computes bit for bit what it did under version 125.
 *   t_c      the number of draw_ell_centred calls on this sampler so far, counted from 1: a counter of its own, which
 *            survives gpirt_sampler_ell_enable as t does
 *   u0, u1   item_uniform(seed, t_c, GPIRT_ST_ELL, 1, 0) and (.., 1, 1): item index 1 where the whitened update has 0, so the two
 *            never share a uniform and calling one never shifts the other's stream
 *   k' = k + d by the rule above with the centred update's own width w_c: the width given to gpirt_sampler_ell_enable until
 *   gpirt_sampler_ell_width_centred sets another (gpirt_sampler_ell_width sets the whitened update's alone).  k' outside
 *   0 .. P - 1: rejected and counted in out_of_range, nothing else runs.
 *   nu = L^-1 f; S under ell_k' is built and factored (ONE factorisation and TWO solves per update that reaches the device);
 *   nu' = L'^-1 f.  There is no product and no commit copy: f does not move.
 *   dq_j = sum over ALL n rows of (nu'_ij - nu_ij) (nu'_ij + nu_ij), formed cell by cell as that product, never as a difference
 *   of two sums of squares; per item in the order of delta above (256 threads over ascending rows, a fixed tree); dq = the sum
 *   of dq_j over the items in ascending order.
 *   dld = sum_i (log L'_ii - log L_ii), each term that difference of two fp64 logarithms; one work-group, 256 threads over
 *   ascending rows, the same tree.  A diagonal entry that is non-positive or not finite counts as non-finite.
 *   log_ratio = (-0.5 dq - m dld) + (log_prior[k'] - log_prior[k]), each product and sum rounded on its own;
 *   accepted iff log(u1) < log_ratio.
 *   Accepted: k <- k', the sampler's kernel is ell_k'; f is byte-identical to before; L, the rows below it and the cached
 *   products are bit for bit what gpirt_sampler_factor leaves for (theta, ell_k').  Rejected, out of range or failed (a
 *   non-positive minor of the proposal's factor, a non-finite nu', diagonal entry, dq or dld): f, L, the rows below it, theta,
 *   beta, mu and the sampler's kernel are byte-identical to before the call; only the centred counters move.  Not an error.
 * A call that returns an error has not happened: not counted, t_c does not advance, and for the centred counters too
 * updates = accepted + rejected + out_of_range + failed always.  A hang-guard expiry in the proposal's factor is repaired once
 * (the factor again on the launch-per-step panel, then the solve, the kernels and the decision again), as above.
 * gpirt_ell's counters stay the whitened update's alone; gpirt_sampler_ell_centred_stats fills gpirt_ell_centred with the
 * centred update's.  gpirt_sampler_ell_get gains "nu_prop" (n x m doubles: nu'), "dq" (m doubles), "record_centred" (6 doubles:
 * dq, dld, log_ratio, log_u, accept, nonfinite), "counts_centred" (4 int64, as "counts") and "times_centred" (GPIRT_ELL_PARTS
 * doubles: the copies, the first solve, the build and factorisation, the second solve, the quad, logdet and decide kernels, the
 * copy back after a rejection).  "nu" is that of whichever update ran last. */
#define GPIRT_ELL_MAX_POINTS 1025
#define GPIRT_ELL_PARTS 8
typedef struct gpirt_ell {
    int64_t  points, width, index;          /* P, w, k */
    int64_t  updates, accepted, out_of_range, failed;
    int64_t  last;                          /* the last update: 0 rejected, 1 accepted, 2 out of range, 3 failed, -1 none yet */
    int64_t  last_proposed;                 /* its k' (may lie outside the grid) */
    int64_t  factorisations;                /* factorisations enqueued by the updates so far (one per update that reached the device) */
    double   length_scale, lo, hi;          /* ell_k and the grid's end points */
    double   last_u0, last_u1;
    int64_t  reserved[4];
} gpirt_ell;
typedef struct gpirt_ell_centred {
    int64_t  width;                         /* w_c */
    int64_t  updates, accepted, out_of_range, failed;
    int64_t  last;                          /* the last centred update: 0 rejected, 1 accepted, 2 out of range, 3 failed, -1 none yet */
    int64_t  last_proposed;                 /* its k' (may lie outside the grid) */
    int64_t  factorisations;                /* factorisations enqueued by the centred updates so far */
    double   last_u0, last_u1;
    int64_t  reserved[6];
} gpirt_ell_centred;
int gpirt_ell_grid(double lo, double hi, int P, double* out);
int gpirt_ell_check(double lo, double hi, int P, const double* log_prior, int width, int k0, const gpirt_kernel* kern,
                    const gpirt_options* opts, int64_t m);
int gpirt_sampler_ell_enable(gpirt_sampler_t s, double lo, double hi, int P, const double* log_prior, int width, int k0, int on);
int gpirt_sampler_draw_ell(gpirt_sampler_t s);
int gpirt_sampler_ell_width(gpirt_sampler_t s, int w);
int gpirt_sampler_ell_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ell_stats(gpirt_sampler_t s, gpirt_ell* out);
int gpirt_sampler_draw_ell_centred(gpirt_sampler_t s);
int gpirt_sampler_ell_width_centred(gpirt_sampler_t s, int w);
int gpirt_sampler_ell_centred_stats(gpirt_sampler_t s, gpirt_ell_centred* out);

/* ------------------------------------------------------ per-item GP amplitudes: fixed or sampled in the chain ---------- */
/* Library version 129.  Item j has an amplitude a_j > 0 and the prior f_j ~ N(0, a_j^2 (K(theta, theta) + 0.001 I)): the
 * amplitude multiplies the WHOLE prior, jitter included, so item j's model is exactly a_j times the unit model.  The factor L is
 * shared by all items as before and nothing is factored for an amplitude.  Where a_j enters, and nowhere else:
 *   draw_f       the prior draw of the elliptical slice is nu_j = a_j (L z_j): the product as before, then one multiplication
 *                per value;
 *   draw_fstar   the conditional mean is unchanged (a_j cancels in k*^T S^-1 f), the standard deviation is a_j s_i with the
 *                reference's s_i = 1 - sqrt(q_i) (quirk Q2) as before;
 *   gpirt_sampler_draw_ell (whitened) runs unchanged: f' = L' L^-1 f does not contain a_j;
 *   gpirt_sampler_draw_ell_centred returns GPIRT_E_ARG while amplitudes are on: its quadratic form would need 1 / a_j^2 per item.
 * Stage API only: gpirt_options, gpirt_run, gpirt_mcmc* and gpirt_sampler_step keep their layout and behaviour.  A sampler on
 * which neither gpirt_sampler_amp_set nor gpirt_sampler_amp_enable was called computes bit for bit what it did; multiplying by
 * 1.0 is exact, so a sampler whose amplitudes are all 1.0 does too.
 *
 * gpirt_sampler_amp_set(s, a): m fixed amplitudes, each finite and in [GPIRT_AMP_MIN, GPIRT_AMP_MAX]; a = NULL turns amplitudes
 * off.  After gpirt_sampler_init.  f is not rescaled: any f is a valid state under any amplitude.
 *
 * gpirt_sampler_amp_enable puts the amplitudes on the logarithmic grid of gpirt_ell_grid, a_k = lo (hi / lo)^(k / (P - 1)),
 * 2 <= P <= GPIRT_AMP_MAX_POINTS, GPIRT_AMP_MIN <= lo < hi <= GPIRT_AMP_MAX, the end points exact, with a_j = a_{k0[j]}
 * (k0 = NULL: the grid point nearest 1 in log a for every item).  log_prior: P finite values, a mass on the grid, i.e. a
 * density with respect to log a; NULL: -(ln a_k)^2 / 2, a log-normal with median 1 and log-sd 1 -- a choice, not a measurement.
 * Every item's proposal width starts at `width` (1 .. P - 1; gpirt_sampler_amp_width sets m widths).  It allocates per item the
 * index, the width, four int64 counters and the last update's record, a P x m uint32 histogram and a planned_draws x m int32
 * buffer of recorded indices, all zeroed; the call count t runs over the sampler's life.  on = 0 frees the state and turns
 * amplitudes off.  gpirt_amp_check is the argument check alone and touches no device: the grid, a non-finite log_prior, width,
 * k0 (m indices in 0 .. P - 1 or NULL); with opts: GPIRT_RNG_RSTREAM (R's stream has no such draw), kernel_fp32, an item shard
 * (item0 != 0 or m_total != m).  gpirt_sampler_amp_enable after gpirt_sampler_amp_set without turning it off, and the
 * converse, are refused.
 *
 * gpirt_sampler_draw_amp: one update of every item in ONE launch, with no host read.  It is a prior-whitened Metropolis step
 * (Murray & Adams 2010, section 2.2) per item: nu_j = L^-1 f_j / a_j is held fixed, so a proposal moves f_j' = (a_k' / a_k) f_j
 * and the likelihood decides.  theta, beta, mu and L are not touched.  For item j (one work-group of 256 threads):
 *   t        the number of draw_amp calls on this sampler so far, counted from 1
 *   u0, u1   item_uniform(seed, t, GPIRT_ST_AMP, item0 + j, 0) and (.., 1)
 *   q = min(floor(u0 2w_j), 2w_j - 1), d = q - w_j for q < w_j, else q - w_j + 1; k' = k_j + d.  k' outside 0 .. P - 1: rejected
 *   and counted in out_of_range[j], nothing else runs for the item.
 *   c = grid[k'] / grid[k_j] (one fp64 division), f'_i = c f_ij (one fp64 multiplication)
 *   dll_j = sum over observed rows of [t(y (f + mu)) - t(y (f' + mu))], t(a) = log(1 + exp(-a)) in the form of csrc/ll_fast.h,
 *   formed cell by cell as a difference of terms; thread t takes rows t, t + 256, ... in ascending order, then a fixed tree:
 *   deterministic.  Rows whose f' is not finite are counted, observed or not.
 *   accepted iff log(u1) < dll_j + (log_prior[k'] - log_prior[k_j]).  A non-finite f' or dll_j: `failed`, never accepted, not
 *   an error.
 *   Accepted: f_ij <- c f_ij (the same expression), k_j <- k', a_j <- grid[k'].  Otherwise item j's column of f is
 *   byte-identical to before; only its counters and record move.
 * Items are independent: no grid-wide barrier, no atomic, one writer per value; two runs give a byte-identical state.
 *
 * gpirt_sampler_amp_record appends the current indices to the draw buffer (GPIRT_E_ARG once planned_draws are in) and adds 1 to
 * hist[k_j, j], on the device with no host synchronisation.  gpirt_sampler_amp_get, by name: "grid", "log_prior" (P doubles),
 * "amplitude" (m doubles; the one name a sampler with gpirt_sampler_amp_set knows), "index", "width" (m int32), "counts" (4 x m
 * int64, row-major: updates, accepted, out_of_range, failed), "record" (5 x m doubles, row-major, of the last update: dll,
 * log_ratio, log_u, status, nonfinite; status 0 rejected, 1 accepted, 2 out of range -- the three figures are NaN --, 3 failed),
 * "hist" (P x m uint32, row-major), "draws" (recorded x m int32, row-major: bytes = 4 m times the records so far), "time" (1 double: milliseconds of device time of
 * the last update's launch with gpirt_sampler_enable_timing on -- one synchronisation per update then --, else 0).
 * gpirt_sampler_amp_stats: totals over the items and the pooled acceptance. */
#define GPIRT_AMP_MAX_POINTS 1025
#define GPIRT_AMP_MIN 0.01
#define GPIRT_AMP_MAX 1000.0
typedef struct gpirt_amp {
    int64_t  on;                            /* 0 off, 1 fixed (gpirt_sampler_amp_set), 2 on the grid (gpirt_sampler_amp_enable) */
    int64_t  points, m;                     /* P (0 when fixed), the items */
    int64_t  calls;                         /* t: gpirt_sampler_draw_amp calls over the sampler's life */
    int64_t  updates, accepted, out_of_range, failed;   /* summed over the items, since gpirt_sampler_amp_enable */
    int64_t  planned_draws, recorded;
    double   accept_rate;                   /* accepted / updates, NaN before the first update */
    double   lo, hi, min_amplitude, max_amplitude;
    int64_t  reserved[4];
} gpirt_amp;
int gpirt_amp_check(double lo, double hi, int P, const double* log_prior, int width, const int* k0, int64_t m,
                    const gpirt_options* opts);
int gpirt_sampler_amp_set(gpirt_sampler_t s, const double* a);
int gpirt_sampler_amp_enable(gpirt_sampler_t s, double lo, double hi, int P, const double* log_prior, int width, const int* k0,
                             int64_t planned_draws, int on);
int gpirt_sampler_draw_amp(gpirt_sampler_t s);
int gpirt_sampler_amp_width(gpirt_sampler_t s, const int* w);
int gpirt_sampler_amp_record(gpirt_sampler_t s);
int gpirt_sampler_amp_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_amp_stats(gpirt_sampler_t s, gpirt_amp* out);

/* ------------------------------------------------------ a centred amplitude update on the rank-64 smooth part ---------- */
/* Library version 135.  gpirt_sampler_draw_amp holds nu_j = L^-1 f_j / a_j fixed; with thousands of answers per item the
 * likelihood pins f_j down and a_j moves only as fast as draw_f changes |nu_j|.  gpirt_sampler_draw_amp_centred is the centred
 * move Murray & Adams (2010) pair it with.  It reads the prior density of f, so it belongs behind gpirt_sampler_step_consistent
 * (after the reference's step f sits at the old theta, quirk Q3).  It needs no factor, dense or structured: only the rank-64
 * identity K(theta, theta) = V Kcc V^T (V the Lagrange basis at theta on the 64 Chebyshev nodes, Kcc = F F^T the kernel at the
 * nodes) on which the structured draw_f and draw_fstar rest.  Stage API only: gpirt_options, gpirt_run, gpirt_mcmc*,
 * gpirt_sampler_step* and gpirt_sampler_draw_amp keep their layout and behaviour, every existing stage keeps its numbers, and a
 * sampler on which the entry is never called computes bit for bit what it did.
 *
 * Exact MCMC by augmentation.  Phi = V F (n x 64), eps = GPIRT_JITTER.  The columns of F whose squared norm (the eigenvalue of
 * Kcc) is <= 1e-13 are DEAD: zeroed on the host, they take no part; r is the count of live ones (32 at the default kernel).  The
 * model f_j ~ N(0, a_j^2 (K + eps I)) is the marginal of
 *     xi_j ~ N(0, a_j^2 I_r),   e_j ~ N(0, eps I_n),   f_j = Phi xi_j + a_j e_j
 * (its covariance a^2 (Phi Phi^T + eps I) differs from a^2 S by the rank identity's 1e-13; the move leaves that model's posterior
 * exactly invariant).  One update of item j, t the count of gpirt_sampler_draw_amp_centred calls from 1:
 *   1. augment   A = Phi^T Phi + eps I = R R^T (one work-group; a bad pivot raises the sampler's numeric error word as the
 *                theta-alone draw_fstar does), T = V^T f, t_j = (R^-1 F^T) T_j, z_j[k] = qnorm(item_uniform(seed, t,
 *                GPIRT_ST_AMP_CENTRED, item0 + j, k)), k = 0 .. 63 (dead k are drawn and ignored: the keying does not depend on
 *                r), w_j = t_j + (a_j sqrt(eps)) z_j, xi_j = R^-T w_j by back-substitution, Q_j = sum of xi^2 over live k in
 *                ascending k, g_j = F xi_j, h_j = V g_j.  csrc/amp_centred.hip fixes the order of every sum.
 *   2. propose   lq[k] = (log_prior[k] - r ln a_k) - Q_j / (2 a_k^2) with the two tables formed at enable on the host in long
 *                double; the maximum, exp and an inclusive scan C; u0 = item_uniform(.., item0 + j, 64); k' = the FIRST k with
 *                C_k > u0 C_last (not draw_theta's (C - C_0) rule: index 0 keeps its mass).  k' == k_j: counted in `same`,
 *                nothing is touched.
 *   3. move      c = grid[k'] / grid[k_j] (one division), f'_i = h_i + c (f_i - h_i) (three roundings, no FMA): the nugget's
 *                whitened coordinates are held fixed.
 *   4. accept    iff log(u1) < dll_j, u1 = item_uniform(.., item0 + j, 65), dll_j the sum over observed rows of
 *                t(y (f + mu)) - t(y (f' + mu)) cell by cell in gpirt_sampler_draw_amp's order.  The proposal carries the prior
 *                and the centred term, so only the likelihood ratio is left; the nugget is 0.03 a logits and acceptance is near
 *                1.  A non-finite f', h, Q_j or dll_j: `failed`, never accepted, not an error.  Accepted: the same work-group
 *                rewrites the column with the same expression and sets k_j, a_j; otherwise the column is byte-identical.
 * No atomics, one writer per value, items independent behind the shared 64 x 64 factorisation: two runs give a byte-identical
 * state.  The call joins a held-back draw_beta, rebuilds V from the current theta and uses the n x m scratch of draw_f's prior
 * draw for H (free between steps).  F is cached per sampler and rebuilt only when a sampled length scale's index moved.
 * On a coarse grid the move hardly moves: given xi, a has relative sd 1 / sqrt(2 r), about 0.12, so a useful grid has steps
 * under about 10 % (the default 129 points on 0.1 .. 10: 3.7 %).
 *
 * It shares grid, log_prior, index, amplitude, histogram and draw buffer with the whitened update and has its own counters and
 * last record, by name through gpirt_sampler_amp_get: "counts_centred" (4 x m int64, row-major: updates, accepted, same,
 * failed), "record_centred" (5 x m doubles, row-major: Q_j, k', dll, log u1, status; status 0 rejected, 1 accepted, 2 same --
 * dll and log u1 NaN --, 3 failed; k' = -1 where no draw could be made), "rank" (1 int32: r), "live" (64 int32: 1 live, 0
 * dead), and the last call's intermediates "centred_T", "centred_z", "centred_w", "centred_xi", "centred_g" (64 x m doubles,
 * column j item j), "centred_Q" (m doubles), "centred_H" (n x m doubles, valid until the next draw_f), "centred_Xh",
 * "centred_R", "centred_F" (64 x 64; F with its dead columns zeroed), "time_centred" (1 double, as "time").  All of them need one gpirt_sampler_draw_amp_centred first.
 * gpirt_sampler_amp_centred_stats: the totals.
 *
 * Refused with GPIRT_E_ARG, each with its reason: before gpirt_sampler_init; amplitudes not in the sampled mode;
 * GPIRT_RNG_RSTREAM; an item shard; kernel_fp32; a handle kernel that fails gpirt_kernel_check(kernel, 64) (Matern, too short
 * a length scale); a theta the sampler does not vouch for (not finite or outside [-5, 5]). */
typedef struct gpirt_amp_centred {
    int64_t  calls;                         /* t: gpirt_sampler_draw_amp_centred calls over the sampler's life */
    int64_t  rank;                          /* r of the last call (0 before the first) */
    int64_t  updates, accepted, same, failed;   /* summed over the items, since gpirt_sampler_amp_enable */
    double   accept_rate;                   /* accepted / (updates - same - failed), NaN while that is 0 */
    double   last_ms;                       /* device time of the last call with gpirt_sampler_enable_timing on, else 0 */
    int64_t  reserved[6];
} gpirt_amp_centred;
int gpirt_sampler_draw_amp_centred(gpirt_sampler_t s);
int gpirt_sampler_amp_centred_stats(gpirt_sampler_t s, gpirt_amp_centred* out);

/* ------------------------------------------------------ a centred beta update: exact Gibbs with f + mu held fixed ------ */
/* Library version 136.  gpirt_sampler_draw_beta is the reference's: one random-walk Metropolis step per coefficient of
 * mu_j = beta_0j + beta_1j theta with f_j held fixed, at step sizes the caller gives.  The likelihood reads only g_j = f_j + mu_j
 * and with thousands of answers per item pins it down, so a step that moves mu_j under a fixed f_j is accepted only when tiny, and
 * the linear trend wanders between f_j and mu_j as slowly as draw_f lets it.  gpirt_sampler_draw_beta_centred is the centred move
 * Murray & Adams (2010) and Yu & Meng (2011) pair such an update with, as gpirt_sampler_draw_ell_centred and
 * gpirt_sampler_draw_amp_centred do for their parameters: beta_j and f_j move together with g_j held fixed.  The likelihood does
 * not change at all, there is no accept step, and the conditional of beta_j is Gaussian in closed form.  It reads the prior
 * density of f, so it belongs behind gpirt_sampler_step_consistent (after the reference's step f sits at the old theta, quirk
 * Q3); it is not refused behind a plain step, which measurements need.  It needs no factor, dense or structured: only the rank-64
 * identity K(theta, theta) = Phi Phi^T, Phi = V F, which gpirt_sampler_draw_amp_centred builds (V the Lagrange basis at theta on
 * the 64 Chebyshev nodes, Kcc = F F^T with its dead columns zeroed).  Stage API only: gpirt_options, gpirt_run, gpirt_mcmc*,
 * gpirt_sampler_step* and gpirt_sampler_draw_beta keep their layout and behaviour, every existing stage keeps its uniforms, and a
 * sampler on which the entry is never called computes bit for bit what it did.
 *
 * With X = [1, theta] (n x 2), S = K(theta, theta) + eps I, eps = GPIRT_JITTER, the amplitude a_j (1.0 exactly when amplitudes
 * are off; fixed and sampled amplitudes are both taken) and the independent priors beta_kj ~ N(m0_kj, s0_kj^2) of the sampler:
 *     f_j = g_j - X beta_j ~ N(0, a_j^2 S)   =>   beta_j | g_j, theta, a_j ~ N(Lam_j^-1 b_j, Lam_j^-1)
 *     Lam_j = B / a_j^2 + diag(1 / s0_kj^2),   B = X^T S^-1 X (2 x 2, shared by all items),   W = S^-1 X (n x 2, shared)
 *     b_j   = X^T S^-1 g_j / a_j^2 + m0_j / s0_j^2 = (W^T f_j + B beta_j) / a_j^2 + m0_j / s0_j^2
 *     f_j'  = f_j + X (beta_j - beta_j'),   mu_j' = X beta_j',   g_j' = g_j.
 * One call updates every item once; t is the count of gpirt_sampler_draw_beta_centred calls over the sampler's life from 1.
 * ROW ORDER below means ell_delta_kernel's: thread t of 256 takes the rows t, t + 256, ... ascending into one accumulator
 * that starts at 0, then the fixed LDS tree s = 128, 64, .., 1 with acc[t] += acc[t + s].  The library is built without
 * contraction: fma where written, nothing else fused.
 *   1. shared    (from theta alone) the call joins a held-back draw_beta, builds V from the current theta and Gv = V^T V by the
 *                split-K product in index order, Xh = R^-1 F^T and R with A = Phi^T Phi + eps I = R R^T in one work-group (a bad
 *                pivot raises the sampler's numeric error word as the theta-alone draw_fstar does).  F and its live mask are the
 *                ones gpirt_sampler_draw_amp_centred caches per sampler, rebuilt only when a sampled length scale's index moved.
 *                P = V^T X (64 x 2): P[c, 0] = sum_i V[i, c] by plain sums, P[c, 1] by fma(V[i, c], theta_i, .), both in row
 *                order.  u = Xh P: u[k, q] = fma(Xh(k, i), P[i, q], .) over i ascending.  Gx = Xh^T u (= F A^-1 Phi^T X):
 *                Gx[c, q] = fma(Xh(k, c), u[k, q], .) over k ascending.  W[i, q] = (X[i, q] - sum_c V[i, c] Gx[c, q]) / eps, the
 *                sum over c ascending by fma from 0, then one subtraction and one division.  B00 = sum_i W[i, 0] (plain sums),
 *                B01 = B10 = fma(W[i, 0], theta_i, .), B11 = fma(W[i, 1], theta_i, .), each in row order.
 *   2. per item  (one work-group per item) T_j[k] = fma(W[i, k], f[i, j], .) in row order; ia = 1 / (a_j a_j); p_k =
 *                1 / (s0_kj s0_kj); b_k = (T_j[k] + (B_k0 beta_0j + B_k1 beta_1j)) ia + m0_kj p_k; Lam00 = B00 ia + p_0,
 *                Lam10 = B10 ia, Lam11 = B11 ia + p_1; c00 = sqrt(Lam00), c10 = Lam10 / c00, c11 = sqrt(Lam11 - c10 c10);
 *                y0 = b_0 / c00, y1 = (b_1 - c10 y0) / c11, mean_1 = y1 / c11, mean_0 = (y0 - c10 mean_1) / c00;
 *                z_k = qnorm_as241(item_uniform(seed, t, GPIRT_ST_BETA_CENTRED, item0 + j, k)), k = 0, 1; x1 = z_1 / c11,
 *                x0 = (z_0 - c10 x1) / c00; beta'_k = mean_k + x_k.
 *                A non-finite T, Lam, pivot, mean or beta', or a pivot (Lam00, Lam11 - c10 c10) that is not > 0: `failed`;
 *                the item's f column, beta, mu and mu_star then stay byte for byte.  It is not an error.
 *   3. rewrite   (the same work-group) mo_i = beta_0j + theta_i beta_1j, the bits mu[i, j] holds behind draw_beta;
 *                mu[i, j] = beta'_0 + theta_i beta'_1 and mu_star[i, j] = beta'_0 + theta*_i beta'_1, the bits the linear mean
 *                of gpirt_sampler_draw_beta gives for beta', so the state is what draw_beta would have left; f'_i = f_i +
 *                (mo_i - mu[i, j]): two products and four sums, no FMA.  The shift is the difference of the two ROUNDED means
 *                and not d_0 + theta_i d_1 with d = beta - beta': that form rounds theta_i beta_1 apart from mu's own rounding,
 *                and where beta_0 and theta_i beta_1 cancel g'_i - g_i would exceed 4 u (|f| + |mu| + |mu'|).  As it is,
 *                |g'_i - g_i| <= u |mo_i - mu_i| + u |f'_i|, within that bound in every cell.  The column of f stays in LDS
 *                between the reduction and the rewrite up to n = 8192 and is read again above.
 * No floating-point atomic, one writer per value: two runs give a byte-identical state.
 *
 * gpirt_sampler_beta_centred_get, by name, all of the last call (they need one gpirt_sampler_draw_beta_centred first, "time"
 * excepted): "W" (n x 2 doubles, column-major), "B" (4 doubles: B00, B10, B01, B11), "P", "Gx" (64 x 2, column-major), "T", "z",
 * "mean", "beta_old", "beta_new" (2 x m doubles, column j item j, as beta; beta_new of a failed item is beta_old), "chol" (3 x m:
 * c00, c10, c11 of item j in column j), "record" (m doubles: status 0 updated, 3 failed), "counts" (2 x m int64, row-major:
 * updates, failed), "time" (1 double: ms of device time of the last call with gpirt_sampler_enable_timing on, else 0),
 * "time_item" (1 double: of that, the per-item kernel's).
 * gpirt_sampler_beta_centred_stats: the totals.
 *
 * Refused with GPIRT_E_ARG, each with its reason: before gpirt_sampler_init; GPIRT_RNG_RSTREAM; an item shard; kernel_fp32; a
 * handle kernel that fails gpirt_kernel_check(kernel, 64) (Matern, too short a length scale); a theta the sampler does not vouch
 * for (not finite or outside [-5, 5]); a prior sd that is not finite and > 0. */
typedef struct gpirt_beta_centred {
    int64_t  calls;                         /* t: gpirt_sampler_draw_beta_centred calls over the sampler's life */
    int64_t  rank;                          /* the live columns of F at the last call (0 before the first) */
    int64_t  updates, failed;               /* summed over the items: every item of every call, and those that failed */
    double   last_ms;                       /* device time of the last call with gpirt_sampler_enable_timing on, else 0 */
    int64_t  reserved[6];
} gpirt_beta_centred;
int gpirt_sampler_draw_beta_centred(gpirt_sampler_t s);
int gpirt_sampler_beta_centred_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_beta_centred_stats(gpirt_sampler_t s, gpirt_beta_centred* out);

/* ------------------------------------------------------ a collapsed scale and shift move: the slopes with theta summed out -- */
/* Library version 137.  theta_finish draws theta given the curves on the grid and every update of beta is given theta, so a
 * change of theta's scale (or location) needs all n respondents and all m slopes (intercepts) to move together, and no
 * conditional update does that: each chain sits at its own scale.  Between gpirt_sampler_theta_partial and
 * gpirt_sampler_theta_finish the sampler holds logpost (N x n), from which theta is summed out in closed form.
 * gpirt_sampler_draw_scale makes ONE Metropolis proposal that moves the linear mean of every item at once and is decided on
 * prod_i Z_i, the likelihood with every theta_i summed out; the theta_finish that follows redraws every theta under whichever
 * curve stands.  That is a partially collapsed Gibbs pair in the right order: no rounding of theta, no factorisation, no new
 * model assumption.  Stage API only: gpirt_options, gpirt_run, gpirt_mcmc*, gpirt_sampler_step, gpirt_sampler_step_consistent
 * and every existing stage keep their layout, behaviour and uniforms, and a sampler that never calls
 * gpirt_sampler_scale_enable computes bit for bit what it did.
 *
 * At the call fstar[k, j] = hstar[k, j] + mu_star[k, j] with mu_star[k, j] = b0_j + x_k b1_j, x_k = -5 + 0.01 k, and
 * logpost[k, i] is the log-likelihood of respondent i's answers at fstar[k, :].  theta_finish draws theta_i from masses
 * proportional to exp(P_i[k]) on k = 1 .. N - 1 (index 0 is never drawn: the CDF there is (C - C_0) / (C_last - C_0)), with
 * P_i[k] = lprior_i[k] + logpost[k, i] and lprior_i the N(0, 1) log density at x_k or row codes[i] of the population prior's
 * table.  So   lz_i = M_i + log sum_{k=1}^{N-1} exp(P_i[k] - M_i),  M_i = max_{k >= 1} P_i[k]   is the log normaliser of
 * exactly the law theta_finish draws from.  hstar is held fixed and only the linear mean moves; t is the count of calls of
 * the kind over the sampler's life from 1, z = qnorm_as241(item_uniform(seed, t, GPIRT_ST_SCALE, kind, 0)), u =
 * item_uniform(seed, t, GPIRT_ST_SCALE, kind, 1):
 *   kind 0, scale   eps = w_scale z;    b1_j' = b1_j c, c = exp(-eps) (the device's exp; the record holds c); b0 unchanged;
 *                   log r = sum_i (lz'_i - lz_i) + sum_j [ldn(b1_j'; pm_1j, ps_1j) - ldn(b1_j; pm_1j, ps_1j)] - m eps.
 *                   -m eps is the log Jacobian of the m slopes; without it the move does not leave the prior invariant.
 *   kind 1, shift   delta = w_shift z;  b0_j' = b0_j + b1_j delta (one product, one sum); b1 unchanged: the linear mean at
 *                   x + delta, Jacobian 1;  log r = sum_i (lz'_i - lz_i) + sum_j [ldn(b0_j'; pm_0j, ps_0j) - ldn(b0_j; ..)].
 * ldn is R's dnorm(., log = TRUE) as draw_beta forms it, -(ln sqrt(2 pi) + 0.5 z^2 + log(sd)) with z = |(x - mean) / sd|.
 * Accepted iff log(u) < log r.  The library is built without contraction: no operation below is fused.
 *   the curve    mu2[k, j] = b0_j' + x_k b1_j' with x_k = -5.0 + (double)k 0.01, draw_beta's expression, so an accepted mu_star
 *                holds the bits draw_beta would write for beta'.  fstar2 = fstar + (mu2 - mu_star): the difference of the two
 *                ROUNDED means; carry_f's fstar - mu_star moves by two roundings per cell.
 *   logpost2     from fstar2 through the very launches gpirt_sampler_theta_partial makes, into its own buffer, through the
 *                same scratch: a width of 0 gives a logpost2 byte-equal to logpost.
 *   lz, lz'      one work-group per respondent in theta_sample_kernel's layout: thread t of 256 holds k = 4 t + e, e = 0 .. 3;
 *                k = 0 and k >= N are left out.  M = the maximum by fmax (a NaN is skipped there and caught by the sum).
 *                s_t = ((0 + exp(P[4t] - M)) + exp(P[4t + 1] - M)) + .., e ascending, a left-out k adding exactly 0.0.
 *                S = the adjacent-pair tree over s_0 .. s_255: for d = 1, 2, .., 128, s[t] += s[t - d] at every t with
 *                (t + 1) % (2 d) == 0, S = s[255] -- what the last entry of theta_sample_kernel's scan holds; in NumPy,
 *                s = s[0::2] + s[1::2] eight times.  lz = M + log(S); dlz = lz' - lz.
 *   the sums     D = sum_i dlz_i: thread t of 256 takes i = t, t + 256, .. ascending into an accumulator that starts at 0,
 *                then the fixed tree s = 128, 64, .., 1 with acc[t] += acc[t + s] (ell_delta_kernel's).  Q = the prior's sum
 *                in ascending j from 0, each term the difference of the two ldn.  J = (double)m eps (scale) or 0.0 (shift).
 *                log r = (D + Q) - J.
 * A call is FAILED, never accepted and counted in `failed`, when an lz_i or lz'_i is not finite, a respondent's column is
 * degenerate (M not > -1e300, theta_sample_kernel's rule), a beta' is not finite, or D, Q or log r is not finite.
 * On ACCEPT the device decides and the host reads nothing: beta, mu_star, fstar and logpost take the proposal's values, mu is
 * rewritten as b0_j' + theta_i b1_j' at the theta in place (mu = X beta as stored holds between stages), and the shape block's
 * gbar, when on, moves by the same mu2 - mu_star.  On REJECT or a failed call every array of the chain is byte for byte as
 * before; only the counters, the record and the proposal's buffers move.  No floating-point atomic, one writer per value: two
 * runs give a byte-identical state.  The call keeps the sampler's note that logpost belongs to the fstar and beta in place,
 * which gpirt_sampler_theta_partial sets and every writer of fstar, beta, f, theta or the population prior clears.
 *
 * gpirt_sampler_scale_enable(s, w_scale, w_shift) allocates the proposal's buffers (2 N m + N n + 3 n doubles) and sets the
 * widths, the sds of eps and delta.  NaN asks for the default 1 / sqrt(n) -- a choice, not a measurement: the sum over n
 * respondents has a curvature of order n m, so this is generous and gpirt_amd.scale.run retunes it.  A width of 0 is allowed
 * and proposes the state itself.  Calling it again only sets the widths.  gpirt_sampler_scale_width sets one.
 * gpirt_sampler_scale_get, by name: "record" (GPIRT_SCALE_RECORD doubles: kind, z, the step eps or delta, c, D, Q, J, log r, u,
 * log u, status (0 rejected, 1 accepted, 2 failed), the count of bad respondents and coefficients, t, the width, 0, 0), "lz",
 * "lz_prop", "dlz" (n doubles), "beta_prop" (2 x m), "mu_prop", "fstar_prop" (N x m), "logpost", "logpost_prop" (N x n, column i
 * respondent i), "counts" (6 int64, row-major 3 x 2: calls, accepted, failed of kind 0 / 1), "times" (6 doubles, ms of the last
 * call with gpirt_sampler_enable_timing on: whole, curve, product, logz, decide, commits).
 * gpirt_sampler_step_consistent_scale(s, nugget, kinds): gpirt_sampler_step_consistent with the asked-for kinds (bit 0 the
 * scale, bit 1 the shift, the scale first) between theta_partial and theta_finish; kinds = 0 is that step bit for bit.
 *
 * Refused with GPIRT_E_ARG, each with its reason: before gpirt_sampler_init or gpirt_sampler_scale_enable; GPIRT_RNG_RSTREAM; an
 * item shard or gpirt_sampler_set_theta_block in use (logpost then holds only part of the items); logpost not current; a kind
 * other than 0 or 1; a width that is not finite or < 0; a prior sd that is not finite and > 0.  Behind a plain
 * gpirt_sampler_step's stages it is not refused, which measurements need, but there f sits at the old theta (quirk Q3) and the
 * chain it is part of is not the model's. */
#define GPIRT_SCALE_RECORD 16
typedef struct gpirt_scale {
    int64_t  on;
    int64_t  calls[2], accepted[2], failed[2];  /* per kind (0 scale, 1 shift) over the sampler's life */
    double   width[2];                          /* the sds of eps and delta */
    double   last_ms[2];                        /* device time of the kind's last call with gpirt_sampler_enable_timing on, else 0 */
    int64_t  reserved[5];
} gpirt_scale;
int gpirt_sampler_scale_enable(gpirt_sampler_t s, double w_scale, double w_shift);
int gpirt_sampler_scale_width(gpirt_sampler_t s, int kind, double w);
int gpirt_sampler_draw_scale(gpirt_sampler_t s, int kind);
int gpirt_sampler_scale_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_scale_stats(gpirt_sampler_t s, gpirt_scale* out);
int gpirt_sampler_step_consistent_scale(gpirt_sampler_t s, int nugget, int kinds);

/* ------------------------------------------------------ a consistent step: f carried to the new theta, a prior check ---- */
/* Library version 133.  The reference's iteration moves theta and keeps f (quirk Q3 of SURVEY.md): behind gpirt_sampler_step
 * f[i, :] is the GP's value at respondent i's OLD position while mu, L and everything built on them belong to the new one, and
 * the prior quadratic form f_j^T S(theta)^-1 f_j / n, which is near 1 for a draw from the prior, sits two orders of magnitude
 * above it (README, "a consistent step").  Whatever reads the prior density of f after such a step reads that mismatch as
 * roughness.  The entries below are an opt-in BESIDE the reference's step: gpirt_sampler_step, gpirt_options, gpirt_run,
 * gpirt_mcmc* and every existing stage's uniforms are unchanged, and a sampler that never calls them computes bit for bit
 * what it did.
 *
 * gpirt_sampler_carry_f(s, nugget): the carry stage, behind gpirt_sampler_theta_finish (or gpirt_sampler_theta_commit) and in
 * front of gpirt_sampler_draw_beta; one launch over the n x m cells on the handle's stream (csrc/carry.hip).  Per respondent i,
 * with k_i the k for which theta_i is bit for bit -5 + 0.01 k (else -1):
 *   k_i < 0 (NaN, a starting value off the grid): the row of f stays byte for byte and is counted in off_grid;
 *   otherwise, for every local item j,
 *     g    = fstar[k_i, j] - mu_star[k_i, j]      one fp64 subtraction; mu_star is the one draw_fstar added, still in place
 *     f_ij = g                                    nugget = 0
 *     f_ij = g + sd_j z_ij                        nugget = 1: one multiplication, one addition, no FMA
 *   sd_j = a_j 0.031622776601683794 (the correctly rounded sqrt(GPIRT_JITTER); a_j the item's amplitude, 1.0 exactly when
 *   amplitudes are off), z_ij = qnorm(item_uniform(seed, iter + 1, GPIRT_ST_CARRY, item0 + j, i)) with iter the completed
 *   iterations: what gpirt_item_normals(h, seed, iter + 1, 11, item0, m, n, .) writes at [i + j n].
 * All respondents are carried, moved or not.  A non-finite fstar cell is carried as draw_fstar left it and counted in
 * nonfinite.  One writer per cell, integer atomics for the two counters alone: two runs give a byte-identical f.  Given the
 * curve on the grid, theta's draw is the reference's own; f becomes that curve at the new theta plus the model's nugget.  Exact
 * up to two named approximations: f* is the reference's conditional mean plus independent noise of sd s = 1 - sqrt(q), about
 * 1e-6 (quirk Q2), not a joint draw; and the nugget is redrawn from its prior (sd 0.03 logits), not tilted by the likelihood.
 * The next draw_f is an exact update of f | theta, y.  nugget = 0 leaves a smooth f WITHOUT the jitter's share: its quadratic
 * form is some 30 times too small; it is there for measurements, not as a step to run.
 * Refused (GPIRT_E_ARG, the reason in gpirt_last_error): before gpirt_sampler_init; GPIRT_RNG_RSTREAM (R's stream has no such
 * draw); nugget other than 0 or 1.  Item shards are NOT refused: the normals are keyed by the global item and a shard holds its
 * own columns of fstar, so a shard's columns come out bit for bit as the whole sampler's.
 *
 * gpirt_sampler_step_consistent(s, nugget): gpirt_sampler_step with the carry between theta_finish and draw_beta -- draw_f,
 * draw_fstar, theta_partial, theta_finish, carry, draw_beta, factor -- bit for bit those seven stage calls.  The carry runs on
 * the main stream in front of the (possibly held-back) draw_beta, which reads the carried f; L and theta are not touched, so
 * nothing cached from the factor goes stale, and the structured paths (which read f at draw_f and draw_fstar only) run as under
 * gpirt_sampler_step.  With gpirt_sampler_enable_timing on, gpirt_sampler_stage_times reports its six stages as before and the
 * carry's device time is gpirt_carry.last_ms, the seventh.
 *
 * gpirt_sampler_carry_stats: the counters (one 32-byte read and a stream synchronisation).
 *
 * gpirt_sampler_prior_quad(s, h_q): m doubles, q_j = || L^-1 f_j ||^2 for the sampler's current L and f -- the prior check.
 * q_j / (n a_j^2) near 1 says that f_j looks like a draw from its prior N(0, a_j^2 S) at the theta L belongs to.  It settles
 * the factor as the length-scale update does, replaces a structured factor by the dense one (gpirt_sampler_dense_factor_count
 * moves by one then, and later structured products read the dense factor's parts: equal to rounding, not bit for bit), copies f
 * to scratch, runs the forward solve there and one reduction (thread t of 256 takes rows t, t + 256, ... ascending, then a fixed
 * tree: no atomics).  f, theta, beta and the iteration counter are untouched and nothing is drawn. */
typedef struct gpirt_carry {
    int64_t  calls;                         /* carries over the sampler's life (stage calls and consistent steps) */
    int64_t  off_grid, nonfinite;           /* of the last call: rows kept (theta not a grid point), non-finite fstar cells carried */
    int64_t  total_off_grid, total_nonfinite;   /* the same summed over the sampler's life */
    double   last_ms;                       /* device time of the last carry with gpirt_sampler_enable_timing on, else 0 */
    int64_t  reserved[4];
} gpirt_carry;
int gpirt_sampler_carry_f(gpirt_sampler_t s, int nugget);
int gpirt_sampler_step_consistent(gpirt_sampler_t s, int nugget);
int gpirt_sampler_carry_stats(gpirt_sampler_t s, gpirt_carry* out);
int gpirt_sampler_prior_quad(gpirt_sampler_t s, double* h_q);

/* ------------------------------------------------------ a population prior for theta: group means and sds ------------------ */
/* Library version 134.  The reference's prior on theta is N(0, 1) for everyone (src/draw-theta.cpp:18).  Here respondent i
 * carries a group code g_i in 0 .. G - 1, 1 <= G <= GPIRT_POP_MAX_GROUPS, every group has a member and -1 is not allowed, and
 * group g's prior is a mass on the theta grid t_k = -5 + 0.01 k: row g of a G x GPIRT_NGRID table log_prior (row-major) of finite
 * doubles.  The table need not be normalised: the constant cancels in :25.  draw_theta becomes
 *   P[k] = log_prior[g_i, k] + logpost[k, i]            one fp64 addition
 * and everything behind that line -- the stabilising maximum, exp, the scan, the CDF, the draw, the degenerate count, the one
 * uniform per respondent -- is as it was (csrc/stages.hip theta_sample_kernel<true>).  A sampler on which neither entry below
 * was called runs the kernel it ran (theta_sample_kernel<false>), and a sampler whose rows are all the default row
 * (gpirt_pop_default_row: -(ln sqrt(2 pi) + 0.5 z z), z = |t_k|, the built-in prior's own bits) draws the same bits.
 * Stage API only: gpirt_options, gpirt_run, gpirt_mcmc* and gpirt_sampler_step keep their layout and behaviour.
 * WHAT KEEPS READING N(0, 1): score, predict, sumscore and shape's reliability weights read N(0, 1) for new respondents and for
 * the marginal weights -- group 0's default population.
 *
 * gpirt_sampler_pop_set(s, codes, G, log_prior): FIXED.  n codes and a G x GPIRT_NGRID table, any finite table -- a normal per
 * group (gpirt_pop_normal_row), a mixture, a flat row.  codes = NULL turns it off.  It works under both RNG contracts: theta
 * consumes the same one uniform per respondent, so R's stream position is unchanged.
 *
 * gpirt_sampler_pop_enable: SAMPLED.  Group 0 is the anchor and keeps a fixed row (anchor_row: GPIRT_NGRID finite values; NULL:
 * the default row), which is what fixes location and scale.  Each group g >= 1 has (mu_g, sd_g) on two grids,
 *   mu_a = mu_hi (2a - (P_mu - 1)) / (P_mu - 1)            long double, rounded once: antisymmetric bit for bit, so that a
 *                                                           mirror-mode chain maps index a to P_mu - 1 - a; 0 < mu_hi <= 5
 *   sd_b = gpirt_ell_grid(sd_lo, sd_hi, P_sd)[b]           logarithmic, the end points exact;
 *                                                           GPIRT_POP_SD_MIN <= sd_lo < sd_hi <= GPIRT_POP_SD_MAX
 * with 2 <= P_mu, P_sd <= GPIRT_POP_MAX_POINTS, and its row is log_prior[g, k] = -(0.5 z z), z = (t_k - mu_g) / sd_g, with
 * t_k = -5.0 + (double)k * 0.01: each of the two products, the sum, the difference, the quotient, 0.5 z and (0.5 z) z rounded on
 * its own, no contraction and no transcendental.  log_hyper_mu (P_mu finite values) and log_hyper_sd (P_sd) are masses on the
 * grids; NULL: zeros, i.e. flat in mu and flat in log sd.  a0, b0: G start indices each (entry 0 is not read); NULL: a = (P_mu -
 * 1) / 2 and the sd point nearest 1 in log sd.  planned_draws sizes the record buffer.  The P_mu x P_sd table
 *   lse[a, b] = log sum_k exp(-(t_k - mu_a)^2 / (2 sd_b^2))
 * the grid's normaliser, is formed once on the host in long double (k ascending) and rounded once (gpirt_pop_lse); it is what
 * makes the update exact for the truncated, discrete prior that draw_theta actually uses.  At P_mu = P_sd = 1024 this is 10^9
 * long-double exponentials, tens of seconds on one core.  on = 0 frees the state and turns the prior off.
 *
 * gpirt_sampler_draw_pop: every group g >= 1 by EXACT GIBBS ON THE GRIDS, with no host read: a reduction launch, then one
 * launch with one work-group of 256 threads per group.  t counts the draw_pop calls over the sampler's life, from 1.
 *   1. n_g, S1_g = sum (k_i - 500), S2_g = sum (k_i - 500)^2 over the group's members, int64, from the grid index k_i of theta_i
 *      (theta_i bit for bit -5 + 0.01 k_i); integer atomics, so the bits do not depend on the order.  A member whose theta is no
 *      grid point (NaN, a start value before the first draw) is counted in off_grid and left out of n_g; its group is not updated
 *      in this call and keeps its indices, its row and its lp rows byte for byte.
 *   2. mu given sd_b (b the group's current sd index), for a = 0 .. P_mu - 1, with c = 0.01, n = (double)n_g, S1, S2 converted
 *      likewise, m = mu_a, s = sd_b, each operation one fp64 rounding in this order:
 *        A = (S2 c) c      B = ((2 m) S1) c      C = (n m) m      Q = (A - B) + C      den = 2 (s s)
 *        lp[a] = (log_hyper_mu[a] - Q / den) - n lse[a, b]
 *      Then the maximum is subtracted, exp, the inclusive scan in theta_sample_kernel's layout (256 threads by 4 consecutive
 *      points: 3 additions in a thread, the Hillis-Steele scan of the thread totals, 1 base addition), and the new index is the
 *      first a with (C_a - C_0) / (C_last - C_0) > u0.  As in draw_theta, index 0 of a grid is therefore never drawn: the update
 *      is exact Gibbs for the masses on the points 1 .. P - 1.
 *   3. sd given the new mu: the same form over b with Q at the new m, lp[b] = (log_hyper_sd[b] - Q / den_b) - n lse[a, b], u1.
 *   4. the group's row, as stated above.
 *   u0, u1 = item_uniform(seed, t, GPIRT_ST_POP, g, 0) and (.., 1): what gpirt_item_uniforms(h, seed, t, 12, g, 1, 2, .) writes.
 *   Nothing else draws from stage 12 and stage 12 draws from nothing else, so every existing stage keeps its uniforms.
 * A draw that finds no index (C_last = C_0) is counted in failed and leaves the group as it was.  Each value has one writer and
 * there is no floating-point atomic: two runs give a byte-identical state.
 *
 * gpirt_sampler_pop_record appends the (a_g, b_g) pairs (group 0's are -1) to the draw buffer (GPIRT_E_ARG once planned_draws are
 * in) and adds 1 to hist_mu[a_g, g] and hist_sd[b_g, g], on the device.  gpirt_sampler_pop_get, by name: "codes" (n int32),
 * "log_prior" (G x GPIRT_NGRID doubles) -- the two names a sampler with gpirt_sampler_pop_set knows --, "mu_grid" (P_mu), "sd_grid"
 * (P_sd), "lse" (P_mu x P_sd, row-major), "log_hyper_mu", "log_hyper_sd", "index" (G x 2 int32), "stats" (3 x G int64, row-major:
 * n_g, S1, S2 of the last call), "off_grid" (G int64, of the last call), "lp_mu" (G x P_mu), "lp_sd" (G x P_sd: the last call's
 * rows, row 0 unused), "counts" (4 x G int64, row-major: calls, updated, skipped, failed), "hist_mu" (P_mu x G uint32), "hist_sd"
 * (P_sd x G uint32), "draws" (recorded x G x 2 int32), "time" (1 double: milliseconds of device time of the last draw_pop's
 * launches with gpirt_sampler_enable_timing on -- one synchronisation per call then --, else 0).  gpirt_sampler_pop_stats: totals.
 *
 * gpirt_pop_check is the argument check alone and touches no device (codes, log_prior, the hyperpriors, a0, b0 may be NULL: not
 * checked then; rows: the rows of log_prior to check; the grids are checked with sampled != 0).  Refused, GPIRT_E_ARG with the
 * reason: the sampled mode under GPIRT_RNG_RSTREAM (R's stream has no such draw); an item shard (item0 != 0 or m_total != m) or
 * gpirt_sampler_set_theta_block in use (the block path would need the codes of its respondents; and
 * gpirt_sampler_set_theta_block is refused while a population prior is on); before gpirt_sampler_init; gpirt_sampler_pop_enable
 * after gpirt_sampler_pop_set without turning it off, and the converse; a non-finite table entry; a code outside 0 .. G - 1; a
 * group without a member; G or a grid size out of range; mu_hi outside (0, 5]; sd_lo not in [GPIRT_POP_SD_MIN, sd_hi) or sd_hi
 * above GPIRT_POP_SD_MAX.  gpirt_sampler_copy_state is refused while a population prior is on (it is not copied). */
#define GPIRT_POP_MAX_GROUPS 8
#define GPIRT_POP_MAX_POINTS 1024
#define GPIRT_POP_SD_MIN 0.05
#define GPIRT_POP_SD_MAX 10.0
typedef struct gpirt_pop {
    int64_t  on;                            /* 0 off, 1 fixed (gpirt_sampler_pop_set), 2 sampled (gpirt_sampler_pop_enable) */
    int64_t  groups, n;                     /* G, the respondents */
    int64_t  points_mu, points_sd;          /* 0 when fixed */
    int64_t  calls;                         /* t: gpirt_sampler_draw_pop calls over the sampler's life */
    int64_t  updates, updated, skipped, failed;   /* summed over the groups g >= 1, since gpirt_sampler_pop_enable */
    int64_t  off_grid;                      /* members off the grid in the last call, summed over all groups */
    int64_t  planned_draws, recorded;
    double   mu_hi, sd_lo, sd_hi;
    double   last_ms;
    int64_t  reserved[4];
} gpirt_pop;
int gpirt_pop_check(const int32_t* codes, int64_t n, int G, const double* log_prior, int64_t rows, int sampled, double mu_hi,
                    int P_mu, double sd_lo, double sd_hi, int P_sd, const double* log_hyper_mu, const double* log_hyper_sd,
                    const int* a0, const int* b0, const gpirt_options* opts);
int gpirt_pop_default_row(double* row);                             /* GPIRT_NGRID doubles */
int gpirt_pop_normal_row(double mu, double sd, double* row);        /* GPIRT_NGRID doubles: -(0.5 z z), the update's expression */
int gpirt_pop_grids(double mu_hi, int P_mu, double sd_lo, double sd_hi, int P_sd, double* mu, double* sd);
int gpirt_pop_lse(const double* mu, int P_mu, const double* sd, int P_sd, double* lse);   /* P_mu x P_sd, row-major */
int gpirt_sampler_pop_set(gpirt_sampler_t s, const int32_t* codes, int G, const double* log_prior);
int gpirt_sampler_pop_enable(gpirt_sampler_t s, const int32_t* codes, int G, const double* anchor_row, double mu_hi, int P_mu,
                             double sd_lo, double sd_hi, int P_sd, const double* log_hyper_mu, const double* log_hyper_sd,
                             const int* a0, const int* b0, int64_t planned_draws, int on);
int gpirt_sampler_draw_pop(gpirt_sampler_t s);
int gpirt_sampler_pop_record(gpirt_sampler_t s);
int gpirt_sampler_pop_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_pop_stats(gpirt_sampler_t s, gpirt_pop* out);

/* ------------------------------------------------------ ordinal (graded) responses: thresholds sampled in the chain --- */
/* Library version 139.  The cumulative-logit (graded response) model on the same f: with g = f + mu and an item's thresholds
 * b_1 < ... < b_{C-1} (b_0 = -inf, b_C = +inf),
 *   P(y = c | g, b) = sigma(b_c - g) - sigma(b_{c-1} - g) = sigma(b_c - g) sigma(g - b_{c-1}) (1 - e^-(b_c - b_{c-1}))
 *   log P = -ll(b_c - g) [c < C] - ll(g - b_{c-1}) [c > 1] + w(b_c - b_{c-1}) [1 < c < C],  ll(a) = log(1 + e^-a), w(d) = log1p(-e^-d)
 * Stage API only: gpirt_run, gpirt_mcmc* and gpirt_options are unchanged, and a sampler on which gpirt_sampler_ordinal_enable was
 * never called launches exactly the kernels it launched before.
 *
 * cat is n x m int8, column-major: 0 = missing, 1 .. C a category, 2 <= C <= GPIRT_ORD_MAX_C, the same C for every item (an item
 * need not use every category).  The sampler is created on the dichotomised matrix (gpirt_amd.ordinal.dichotomise); enable
 * refuses unless its y is NaN exactly where cat is 0, and while ordinal is on nothing of the chain reads y.  The thresholds live on
 * the grid t_k = hi (2k - (P - 1)) / (P - 1) (gpirt_ordinal_grid: long double, rounded once; P odd, the centre exactly 0, the end
 * points exact; GPIRT_ORD_MIN_POINTS <= P <= GPIRT_ORD_MAX_POINTS, 0 < hi <= 20); the state is the int32 index K[j, c], c = 1 ..
 * C - 1, strictly increasing in c (row-major m x (C - 1)).  log_prior: P finite log masses (NULL: -t^2 / 18, sd 3).  K0: the start
 * (NULL: k_c = ((2 (P - 1) c + C) / (2 C), integer division -- for C = 2 the centre; gpirt_amd.ordinal.init_thresholds starts from the data).
 * The intercept is pinned: enable sets beta[0, :] = 0 and refreshes mu and mu_star; location is the thresholds'.
 *
 * While ordinal is on, gpirt_sampler_step (and _step_consistent) run draw_f with the ordinal slice kernel (the same uniforms of
 * GPIRT_ST_F_ESS, bracket rule, trial cap and failure behaviour; with C = 2 and the one threshold at the centre it is the binary
 * kernel bit for bit), draw_fstar unchanged, theta_partial as the fp64 product of the N x C m table
 *   G[k, (c - 1) m + j] = -ll(b_c - f*_kj) [c < C] - ll(f*_kj - b_{c-1}) [c > 1]
 * with the one-hot n x C m indicators (the int8 fixed-point product is not extended), theta_finish unchanged (the population prior
 * composes), and draw_beta as the reference's MH step for the SLOPE alone (GPIRT_ST_BETA indices 2 and 3, the binary kernel's).
 * gpirt_sampler_draw_thresholds is a call of its own after the step: exact Gibbs for each threshold on the grid points of a
 * randomly placed window [a, a + W), a = k - (int)(u0 W), that lie strictly between the neighbouring thresholds -- a set that does
 * not depend on k, so the move leaves the posterior invariant.  csrc/ordinal.hip states the order of every operation.
 * gpirt_sampler_ordinal_record appends K to the draw buffer (planned_draws x m x (C - 1) int32) and adds to the histogram
 * (m x (C - 1) x P uint32); gpirt_sampler_ordinal_accumulate_irf adds sigma(f*[k, j] - b_{j,c}) = P(y > c | theta_k) to cum
 * (m x (C - 1) x GPIRT_NGRID doubles, k fastest).
 * gpirt_sampler_ordinal_get, by name: "cat" (n x m int8), "grid", "log_prior" (P doubles), "index" (m x (C - 1) int32),
 * "thresholds" (m x (C - 1) doubles), "counts" (m x C int64: observed cells per category), "lp" (m x (C - 1) x W doubles: the last
 * update's masses by window slot, -inf outside the candidates; W is that update's width, gpirt_ordinal.lp_width -- a
 * gpirt_sampler_ordinal_width since then does not change how it is read), "window" (m x (C - 1) int32: the last windows' a), "hist", "draws"
 * (recorded x m x (C - 1)), "cum", "pinned", "failed", "updates" (1 int64 each).
 *
 * Refused while ordinal is on, GPIRT_E_ARG with the reason: every entry that evaluates the binary likelihood or reads y (the
 * summaries' WAIC / pred parts, the PPC and its add-ons, LOO, score and predict, sumscore, equate, groups, the ACF's
 * log-likelihood series, the whitened draw_ell, both draw_amp updates, draw_scale), draw_beta_centred (it moves the pinned
 * intercept), gpirt_sampler_set_theta_block, gpirt_sampler_copy_state, gpirt_sampler_set of "y" (its missing cells were checked
 * against cat) and of "beta" with a non-zero intercept; and gpirt_sampler_ordinal_enable itself after any of
 * those blocks, under GPIRT_RNG_RSTREAM, on an item shard, with theta_block in use, with GPIRT_LL_EXACT=1 (the ordinal kernels have
 * the fast term alone), before gpirt_sampler_init, for n > GPIRT_ORD_MAX_N, and for every bad argument gpirt_ordinal_check names
 * (it is the argument check alone and touches no device; NULL pointers are not checked).  cat = NULL turns ordinal off and
 * frees its state; beta and the chain's state stay as they are. */
#define GPIRT_ORD_MAX_C 8
#define GPIRT_ORD_MIN_POINTS 9
#define GPIRT_ORD_MAX_POINTS 1001
#define GPIRT_ORD_MAX_WIDTH 64
#define GPIRT_ORD_MAX_N 16384
typedef struct gpirt_ordinal {
    int64_t  on;                            /* 0 off, 1 on */
    int64_t  n, m, categories, points, width;
    int64_t  calls;                         /* t: gpirt_sampler_draw_thresholds calls over the sampler's life */
    int64_t  pinned, failed, updates;       /* thresholds with one candidate / a non-finite mass / drawn, since enable */
    int64_t  planned_draws, recorded, irf_draws;
    double   hi;
    double   last_ms;                       /* device time of the last draw_thresholds with gpirt_sampler_enable_timing on, else 0 */
    int64_t  lp_width;                      /* the W of the last update: the slots per row of "lp" (the enable's W before the first) */
    int64_t  reserved[3];
} gpirt_ordinal;
int gpirt_ordinal_check(const int8_t* cat, const double* y, int64_t n, int64_t m, int C, double hi, int P, const double* log_prior,
                        const int32_t* K0, int W, const gpirt_options* opts);
int gpirt_ordinal_grid(double hi, int P, double* out);
int gpirt_sampler_ordinal_enable(gpirt_sampler_t s, const int8_t* cat, int C, double hi, int P, const double* log_prior,
                                 const int32_t* K0, int W, int64_t planned_draws);
int gpirt_sampler_draw_thresholds(gpirt_sampler_t s);
int gpirt_sampler_ordinal_width(gpirt_sampler_t s, int W);
int gpirt_sampler_ordinal_record(gpirt_sampler_t s);
int gpirt_sampler_ordinal_accumulate_irf(gpirt_sampler_t s);
int gpirt_sampler_ordinal_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ordinal_stats(gpirt_sampler_t s, gpirt_ordinal* out);

/* ------------------------------------------------------ ordinal model fit: WAIC, category predictions, PPC ------------ */
/* Library version 142.  Fit output for the ordinal model above, accumulated on the device one draw at a time so that no f draw is
 * ever stored.  Stage API only: gpirt_run, gpirt_mcmc* and gpirt_options are unchanged, every refusal above stays (the binary
 * summaries and PPC are still refused while ordinal is on), nothing is drawn from the chain's streams and a sampler that never
 * calls gpirt_sampler_ordinal_fit_enable launches exactly what it launched before.
 *
 * Per cell and draw, g = f + mu, d_c = g - b_c with the sampler's CURRENT thresholds (an accumulate after
 * gpirt_sampler_draw_thresholds sees that iteration's), E_c = exp(-|d_c|):
 *   e_c = P(y > c) = d_c >= 0 ? 1 / (1 + E_c) : E_c / (1 + E_c),     ll(a) = log1p(e^-|a|) + max(-a, 0)
 *   logP(c) = -ll(b_c - g) [c < C] - ll(g - b_{c-1}) [c > 1] + w(b_c - b_{c-1}) [1 < c < C], added in that order
 * (csrc/ordinal_fit.hip states the order of every sum; gpirt_amd.ordinal.fit_from_draws is the NumPy statement).
 *
 * parts, any subset: GPIRT_OFIT_WAIC -- per observed cell the running lse (a logaddexp, the first draw sets it) and the Welford
 * mean and M2 of logP(cat), 24 bytes per cell; a cell with a NaN draw is NaN.  GPIRT_OFIT_PRED -- per cell, missing ones
 * included, the sums of e_c, 8 (C - 1) bytes per cell (for a missing cell its held-out prediction).  GPIRT_OFIT_PPC -- each
 * observed cell replicated from one uniform, rep = 1 + #{c : u < e_c}, u = item_uniform(seed, iteration, GPIRT_ST_ORD_PPC,
 * item0 + j, i), iteration the completed-iteration counter; per item, per respondent and for the whole matrix over the observed
 * cells: n_obs, obs_score (T, the sum of cat), score_ge / score_gt (#{R >= T}, #{R > T} of the replicate's score R),
 * rep_score_sum, rep_score_sumsq, agree_sum (cells with rep == cat), dev_obs_sum, dev_rep_sum (D = -2 sum logP), dev_ge (Delta >= 0,
 * Delta = the sum over the cells with rep != cat of logP(cat) - logP(rep): exactly 0, and counted, when nothing changed), nonfinite;
 * per (item, category): obs_count, rep_count_sum, rep_count_sumsq, count_ge, count_gt.  A unit with a non-finite g in an observed
 * cell in a draw counts that draw in nonfinite and leaves it out of its sums (the item's category counts included).
 *
 * gpirt_sampler_ordinal_fit_enable: after gpirt_sampler_ordinal_enable; parts = 0 turns the block off and frees it, as does
 * gpirt_sampler_ordinal_enable(cat = NULL).  Refused, GPIRT_E_ARG with the reason: before gpirt_sampler_init, without ordinal on,
 * parts with unknown bits; gpirt_sampler_ordinal_fit_accumulate without enable; a _get of a part that is not enabled.
 * gpirt_sampler_ordinal_fit_state: ONE device block (header of 16 int64: the tag "OFIT", layout version, n, m, C, parts, draws,
 * item0; then the enabled parts' arrays).  gpirt_ordinal_fit_combine pools `chains` such blocks into d_out (as large as one of
 * them; it may be d_states[0]) in chain order: counts added, Chan's formula for the Welford pairs, a logaddexp for lse.  It takes no
 * signs: theta -> -theta with the slope leaves f + mu and the thresholds as they are.  gpirt_ordinal_fit_get and
 * gpirt_ordinal_fit_totals read any such block, one chain's or a pooled one; the sampler's entries read its own.
 * _get, by name: "draws" (1 int64); "lse", "ll_mean", "ll_m2" (n x m doubles, column-major; a missing cell: 0, 0, -1);
 * "pred_sum" ((C - 1) planes of n x m doubles); "item_<f>" (m), "respondent_<f>" (n), "total_<f>" (1) for the unit fields <f> above
 * (uint64; dev_obs_sum and dev_rep_sum doubles); "cat_<f>" (m x C uint64, row-major) for the category fields; and through the
 * sampler's entry alone, of the last counted draw: "rep" (n x m int8; 0 = missing or non-finite), "delta" and "score" (m + n + 1
 * doubles / int64: items, respondents, the whole matrix), "counts_rep" (m x C int64).
 * Limits are the ordinal model's: n <= GPIRT_ORD_MAX_N, C <= GPIRT_ORD_MAX_C, GPIRT_RNG_ITEM, no item shard. */
enum { GPIRT_OFIT_WAIC = 1, GPIRT_OFIT_PRED = 2, GPIRT_OFIT_PPC = 4, GPIRT_OFIT_ALL = 7 };
typedef struct gpirt_ordinal_fit {
    int64_t  n, m, categories, parts;
    int64_t  draws;                         /* accumulated draws (pooled: of all chains) */
    int64_t  n_obs;                         /* observed cells (0 with GPIRT_OFIT_PRED alone) */
    double   lppd, p_waic, elpd_waic, waic, se_elpd_waic;      /* NaN without GPIRT_OFIT_WAIC; se: sqrt(n_obs var(elpd_ij)), ddof 1 */
    int64_t  reserved[5];                   /* in: 0 */
} gpirt_ordinal_fit;
int gpirt_sampler_ordinal_fit_enable(gpirt_sampler_t s, int parts);
int gpirt_sampler_ordinal_fit_accumulate(gpirt_sampler_t s);
int gpirt_sampler_ordinal_fit_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ordinal_fit_totals(gpirt_sampler_t s, gpirt_ordinal_fit* out);
int gpirt_sampler_ordinal_fit_state(gpirt_sampler_t s, void** d_block, int64_t* bytes);
int gpirt_ordinal_fit_combine(gpirt_handle_t h, const void* const* d_states, int chains, void* d_out);
int gpirt_ordinal_fit_get(gpirt_handle_t h, const void* d_block, const char* name, void* h_out, int64_t bytes);
int gpirt_ordinal_fit_totals(gpirt_handle_t h, const void* d_block, gpirt_ordinal_fit* out);

/* ------------------------------------------------------ scoring new respondents under ordinal responses ---------------- */
/* Library version 144.  What "scoring new respondents" and "predicting new respondents' unseen answers" do for the binary model,
 * for the ordinal model above: the theta posterior and predictive density of respondents who were not in the fit, their category
 * probabilities on every item and the item to ask next, accumulated on the device one draw at a time.  Stage API only: gpirt_run,
 * gpirt_mcmc* and gpirt_options are unchanged, gpirt_sampler_score_enable and gpirt_sampler_score_predict_enable stay refused
 * while ordinal is on, nothing is drawn and a sampler that never calls gpirt_sampler_ordinal_score_enable launches exactly what
 * it launched before.
 *
 * cat_new: n_new x m int8, column-major, 0 = missing, 1 .. C a category, over the sampler's m items and its C; 1 <= n_new <=
 * GPIRT_SCORE_MAX_N.  Per counted draw, with that draw's f* (N = 1001 x m; it carries mu*, the intercept is pinned at 0) and the
 * sampler's CURRENT thresholds b_{j,c} (an accumulate after gpirt_sampler_draw_thresholds sees that iteration's):
 *   T[k, r] = sum over r's observed cells of  -ll(b_c - f*[k,j]) [c < C]  - ll(f*[k,j] - b_{c-1}) [c > 1],   c = cat_new[r, j]
 *   Wc[r]   = sum over r's observed cells with 1 < c < C of  log1p(-exp(-(b_c - b_{c-1}))),  ascending j
 * T is the product draw_theta forms for the chain's respondents (the same launches, on the block's own one-hot operand and table).
 * lp[k] = log dnorm(theta*_k) + T[k, r];  M = max_k lp[k],  Z = sum_k exp(lp[k] - M),  w_k = exp(lp[k] - M) / Z;
 *   l = M + log Z - logsumexp_k log dnorm(theta*_k) + Wc[r]        (the log marginal likelihood of r's answers under the draw)
 * post_sum[r][k] += w_k, lpd_acc[r] = logaddexp(lpd_acc[r], l), ll_sum[r] += l, draws[r] += 1.  Wc does not depend on theta, so the
 * weights do not see it; it changes from draw to draw, so l may not drop it.  A NaN cell of f* skips the draw for the respondents
 * who answered that item alone (nonfinite[r] += 1, nothing else of theirs is touched); +-inf terms are held at -1e300, which is
 * finite.  A respondent with no answers gets the prior and l = 0.
 *
 * predict != 0 adds, per counted draw and for every respondent and item (answered ones included),
 *   q_c[r, j] = sum_k w_k P_c[k, j],   P_c = exp(logP(c | f*[k,j], b_j)) with the w term (the stable log form above, one
 *               exp(-|f* - b_c|) per threshold; never a difference of two sigmas)
 *   info[r, j] = h(q) - sum_k w_k Hc[k, j],   h(q) = -sum_c q_c log q_c,   Hc = -sum_c P_c log P_c   (a term with P = 0 is 0)
 * into prob_sum[c][j][r] and info_sum[j][r]: the mutual information between the unseen answer and theta_r.  A draw whose f* holds a
 * NaN is skipped WHOLE for this part and counted in pred_skipped; +-inf cells are fine.  top (1..GPIRT_PREDICT_MAX_TOP) is checked
 * here and used by the callers' next-item list (r's unanswered items by decreasing info, ties to the lowest j, padded with -1).
 *
 * gpirt_sampler_ordinal_score_enable: after gpirt_sampler_ordinal_enable; cat_new = NULL or n_new = 0 frees the block, as does
 * gpirt_sampler_ordinal_enable(cat = NULL).  Refused, GPIRT_E_ARG with the reason: before gpirt_sampler_init, without ordinal on, a
 * value outside 0 .. C, n_new outside 1..GPIRT_SCORE_MAX_N, top out of range; _accumulate or _get without enable; a predict name
 * without predict.
 * _get, by name: "draws", "nonfinite", "n_obs" (n_new int64), "lpd_acc", "ll_sum" (n_new), "post_sum" (n_new x N, k fastest); of the
 * last accumulate "product" (T: N x n_new, k fastest), "wc" (n_new), "w_table" (m x C, row-major); with predict "prob_sum" (C planes
 * of n_new x m, column-major), "info_sum" (n_new x m), "counts" (2 int64: pred_draws, pred_skipped), "weights" (N x n_new) and
 * "operands" (N x (C + 1) m: [P_1 | ... | P_C | Hc]) of the last counted draw.  The finished values (grid_post = post_sum / draws,
 * theta_mean, theta_sd, theta_quantiles, theta_map, lpd = lpd_acc - log draws, loglik_mean, probs, expected, info, next_items) are
 * the binary scorer's functions of these sums (gpirt_amd.ordinal.score_result, predict_result).
 *
 * State blocks, ONE device block each, a header of 8 int64 then the arrays:
 *   gpirt_sampler_ordinal_score_state          ("OSCR", layout version, n_new, m, C, N, 0, 0), draws, nonfinite, n_obs, lpd_acc,
 *                                              ll_sum, post_sum
 *   gpirt_sampler_ordinal_score_predict_state  ("OSPR", layout version, n_new, m, C, N, pred_draws, pred_skipped), the answered-mask
 *                                              of cat_new packed 64 cells a word (cell g = r + j n_new), prob_sum, info_sum
 * gpirt_ordinal_score_combine pools `chains` score blocks in chain order into the HOST block h_out (bytes: one block's size, the same
 * layout): counters and sums added, lpd_acc by logaddexp, a chain with signs[c] = -1 entering with post_sum[r][k] <->
 * post_sum[r][1000 - k] (exact: theta -> -theta with the slope leaves f + mu and the thresholds as they are; lpd takes no sign).
 * gpirt_ordinal_score_predict_combine adds prob_sum, info_sum and the two counters; it takes no signs.  Blocks with another n_new, m,
 * C or cat_new are refused.
 * Device memory per state: 8 (n_new C m + 1024 C m + 2 * 1001 n_new + 1001 m) bytes for the one-hot operand, the table, the
 * accumulators and the product; predict adds 16 (C + 1) n_new m bytes for its sums and product (about 2.4 GB at 16384 x 1024 with
 * C = 8) and 8 * 1024 (n_new + (C + 1) m) for the weights and the operand table. */
int gpirt_sampler_ordinal_score_enable(gpirt_sampler_t s, const int8_t* cat_new, int64_t n_new, int predict, int top);
int gpirt_sampler_ordinal_score_accumulate(gpirt_sampler_t s);
int gpirt_sampler_ordinal_score_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_ordinal_score_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_sampler_ordinal_score_predict_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_ordinal_score_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, void* h_out, int64_t bytes);
int gpirt_ordinal_score_predict_combine(gpirt_handle_t h, int chains, const void* const* d_states, void* h_out, int64_t bytes);

/* ------------------------------------------------------ group posteriors: separation, overlap, party-line votes ------- */
/* Library version 127.  The respondents come in groups (parties, cohorts, arms); per counted draw the device forms joint
 * functionals of the groups and accumulates them, so that no f draw is ever stored.  Stage API only: gpirt_run is unchanged,
 * nothing is drawn, and a sampler on which gpirt_sampler_groups_enable was never called computes bit for bit what it did.
 *
 * GROUP CODES.  One int32 per respondent: -1 = left out, 0 .. G - 1 the groups; 2 <= G <= GPIRT_GROUPS_MAX_G, every group has a
 * member, n <= GPIRT_GROUPS_MAX_N, m <= GPIRT_GROUPS_MAX_M, top in 1 .. GPIRT_GROUPS_MAX_TOP.  gpirt_groups_check is that
 * check alone (no device is touched; sizes_out: GPIRT_GROUPS_MAX_G + 1 words, the group sizes n_g and at index G the number of
 * included respondents; may be NULL).  A left-out respondent takes part in nothing: its theta, f, mu and y are never looked at.
 * Row G of every per-group array of part A is the group of ALL included respondents.  The P = G (G - 1) / 2 pairs (g, h),
 * g < h, are indexed in lexicographic order.
 *
 * PART A, LATENT (theta alone; every per-draw quantity but the fp64 statistics is an integer).  k_i is theta_i's grid index
 * (theta_i bit for bit -5 + 0.01 k_i, else the respondent is off the grid), t_i = k_i - 500.  A draw with any included
 * respondent off the grid is skipped whole (latent_skipped), decided before anything is touched; else latent_draws counts it:
 *   hist[g][k]   uint32 (G + 1) x 1001: the group's respondents at grid point k
 *   c1[g], c2[g] int64: sum of t and of t^2
 *   med2[g]      k at position (n_g + 1) / 2 plus k at position n_g / 2 + 1 of the sorted group (positions from 1; integer
 *                divisions), 0 .. 2000
 *   w[p]         U2 - n_g n_h, U2 = sum_k H_g[k] (2 less_h[k] + H_h[k]), less_h[k] = sum_{k' < k} H_h[k']: twice the Mann-Whitney
 *                count of theta_g > theta_h with ties as a half
 *   ov[p]        sum_k min(H_g[k] n_h, H_h[k] n_g)
 *   the order of the means: c1[g] n_h against c1[h] n_g in int64; the order of the medians: med2[g] against med2[h]
 *   in fp64, each operation rounded on its own (-ffp-contract=off):
 *     mean_g = c1 / n_g;  var_g = (n_g c2 - c1 c1) / (n_g n_g) (numerator and denominator exact integers, converted, one
 *     division);  sd_g = sqrt(var_g);  a[p] = w / (n_g n_h);  overlap[p] = ov / (n_g n_h);
 *     d[p] = (mean_g - mean_h) / sqrt((n_g var_g + n_h var_h) / (n_g + n_h)), each n converted, products before the sum; a
 *     pooled variance of 0 counts in d_undefined and adds nothing
 *   per included respondent, within its own group: less = less_g[k_i], eq = H_g[k_i]; it covers a median position q when
 *   less < q <= less + eq, q1 = (n_g + 1) / 2, q2 = n_g / 2 + 1; c = [covers q1] + [covers q2]; median_cover += (c > 0),
 *   median_share += c / (2 eq) in fp64.
 * PART B, VOTES (the n x m pass).  Per cell of an included respondent, observed or not, g = f + mu, e = exp(-|g|),
 * p = g >= 0 ? 1 / (1 + e) : e / (1 + e), q = g >= 0 ? e / (1 + e) : 1 / (1 + e) (the PPC's expression).  A draw with a NaN g
 * in any such cell is skipped whole (votes_skipped), decided before anything is touched; +-inf is taken (p is 0 or 1); else
 * votes_draws counts it.  The two parts skip independently.
 *   e[g][j]      uint64: sum over the group's members of rint(p 2^44)
 *   side[g][j]   the sign of 2 e - n_g 2^44 (integers); pair p is split on j when side_g side_h = -1; j is contested when any
 *                pair splits on it; n_split[p] = its split items; c_g = the contested items with side_g != 0
 *   support s = (double)e / ((double)n_g 2^44), rice = |2 s - 1|, gap[p][j] = s_g - s_h
 *   loy[i]       uint64: sum over the contested items j with side_g != 0 of rint(x 2^44), x = p for side_g = +1, q for -1; the
 *                draw's loyalty is (double)loy / ((double)c_g 2^44); c_g = 0 counts in loy_undefined[g] and adds nothing
 *   obs_with[i], obs_n[i]: over the same items, the observed cells whose answer is on the group's side, and their number.
 * ACCUMULATORS (the arrays GPIRT_GROUPS_* of the state block, in this order; every fp64 cell has one owner and is added to
 * once per counted draw, the value and then its square, in draw order; no floating-point atomics anywhere).
 * POOLING (gpirt_groups_combine): integers add, fp64 sums add in chain order.  A chain with sign -1 enters part A reflected:
 * dens_sum, dens_sq and medhist reversed along their grid axis, mean_sum, a_sum and d_sum negated, the > and < order counts
 * swapped; everything else is even in theta and kept; part B takes no signs.  The struct gets the pooled arrays, the counters,
 * most_split (per pair the `top` items by split count, ties to the lowest j; -1 beyond m) with p_split = count / votes_draws,
 * and least_loyal (the `top` included respondents by loy_sum / (votes_draws - loy_undefined[g]) ascending, ties to the
 * lowest i, respondents without a defined draw left out; -1 and NaN beyond them).
 * gpirt_sampler_groups_get, by name: every array below in lower case ("dens_sum" ...), "counts" (4 int64: latent_draws,
 * latent_skipped, votes_draws, votes_skipped), "group_size" (GPIRT_GROUPS_MAX_G + 1 int64), "groups" (n int8) and, of the last
 * counted draw of its part: "hist" (uint32), "c1", "c2", "med2", "w", "ov" (int64), "latent_stats" (fp64: mean, var, sd of the
 * G + 1 rows, then a, overlap, d of the P pairs, d NaN where undefined), "e" (uint64 G x m), "side" (int8 G x m), "split" (uint8
 * P x m), "contested" (uint8 m), "n_split" (int64 P), "c_g" (int64 G), "loy" (uint64 n), "obs_with", "obs_n" (uint32 n).
 * gpirt_sampler_groups_state returns the ONE device block: 16 int64 (the tag 0x31505247 "GRP1", the layout version 1, n, m, G,
 * latent_draws, latent_skipped, votes_draws, votes_skipped, 0 ...), 16 int64 of group sizes, the codes as n int8, then the
 * arrays in order, each on a 16-byte boundary. */
#define GPIRT_GROUPS_MAX_G            8
#define GPIRT_GROUPS_MAX_N            65534
#define GPIRT_GROUPS_MAX_M            4096
#define GPIRT_GROUPS_MAX_TOP          64
#define GPIRT_GROUPS_MED_BINS         2001
#define GPIRT_GROUPS_DENS_SUM         0       /* uint64 [G + 1][1001]: sum of H */
#define GPIRT_GROUPS_DENS_SQ          1       /* uint64 [G + 1][1001]: sum of H^2 */
#define GPIRT_GROUPS_MEDHIST          2       /* uint32 [G + 1][2001] */
#define GPIRT_GROUPS_ORDER            3       /* uint32 [6][P]: mean >, =, <, median >, =, < */
#define GPIRT_GROUPS_OV_SUM           4       /* uint64 [P] */
#define GPIRT_GROUPS_D_UNDEFINED      5       /* uint32 [P] */
#define GPIRT_GROUPS_MEAN_SUM         6       /* double [G + 1] */
#define GPIRT_GROUPS_MEAN_SQ          7
#define GPIRT_GROUPS_SD_SUM           8       /* double [G + 1] */
#define GPIRT_GROUPS_SD_SQ            9
#define GPIRT_GROUPS_A_SUM            10      /* double [P] */
#define GPIRT_GROUPS_A_SQ             11
#define GPIRT_GROUPS_OVL_SUM          12      /* double [P] */
#define GPIRT_GROUPS_OVL_SQ           13
#define GPIRT_GROUPS_D_SUM            14      /* double [P] */
#define GPIRT_GROUPS_D_SQ             15
#define GPIRT_GROUPS_MEDIAN_COVER     16      /* uint32 [n] */
#define GPIRT_GROUPS_MEDIAN_SHARE     17      /* double [n] */
#define GPIRT_GROUPS_SPLIT_COUNT      18      /* uint32 [P][m] */
#define GPIRT_GROUPS_NSPLIT_SUM       19      /* uint64 [P] */
#define GPIRT_GROUPS_NSPLIT_SQ        20      /* uint64 [P] */
#define GPIRT_GROUPS_SUPPORT_SUM      21      /* double [G][m] */
#define GPIRT_GROUPS_SUPPORT_SQ       22
#define GPIRT_GROUPS_RICE_SUM         23      /* double [G][m] */
#define GPIRT_GROUPS_RICE_SQ          24
#define GPIRT_GROUPS_GAP_SUM          25      /* double [P][m] */
#define GPIRT_GROUPS_GAP_SQ           26
#define GPIRT_GROUPS_LOY_SUM          27      /* double [n] */
#define GPIRT_GROUPS_LOY_SQ           28
#define GPIRT_GROUPS_LOY_UNDEFINED    29      /* uint32 [G] */
#define GPIRT_GROUPS_OBS_WITH_SUM     30      /* uint64 [n] */
#define GPIRT_GROUPS_OBS_N_SUM        31      /* uint64 [n] */
#define GPIRT_GROUPS_NARRAYS          32
typedef struct gpirt_groups {
    int64_t    top;                                  /* in: 1 .. GPIRT_GROUPS_MAX_TOP */
    void*      raw[GPIRT_GROUPS_NARRAYS];            /* the pooled arrays, on the host, sized as above; NULL: not wanted */
    int64_t*   most_split_items;                     /* P x top */
    double*    most_split_p;                         /* P x top */
    int64_t*   least_loyal;                          /* top */
    double*    least_loyal_loyalty;                  /* top */
    int64_t    n, m, G, pairs, included, chains;     /* out */
    int64_t    latent_draws, latent_skipped, votes_draws, votes_skipped;
    int64_t    group_size[GPIRT_GROUPS_MAX_G + 1];   /* n_g; at index G the included respondents */
    int64_t    reserved[4];                          /* zero */
} gpirt_groups;
int gpirt_groups_check(int64_t n, int64_t m, int G, const int32_t* groups, int top, int64_t* sizes_out);
int gpirt_sampler_groups_enable(gpirt_sampler_t s, int G, const int32_t* groups, int top, int on);
int gpirt_sampler_groups_accumulate(gpirt_sampler_t s);
int gpirt_sampler_groups_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes);
int gpirt_sampler_groups_state(gpirt_sampler_t s, void** d_state, int64_t* bytes);
int gpirt_groups_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_groups* out);

/* ------------------------------------------------------ the chains with any of the analyses above, in one call -------- */
/* What gpirt_mcmc_run computes beside gpirt_mcmc_chains's outputs: one struct per analysis, each NULL when not wanted, each
 * filled as its section above describes.  The chains are gpirt_mcmc_chains's whatever is asked for -- draws, IRFs, pooled, diag
 * and R's stream position bit-identical; no analysis consumes anything of the chain's random numbers, and each leaves every
 * other one's results bit for bit what they are without it.  Every chain accumulates after each sampling iteration's
 * summaries: under the item RNG from the verified checkpoint (so a hang-guard rollback counts no draw twice), under R's
 * stream from the live state right after the step.  The states are pooled with the reflection signs that
 * gpirt_chains_combine decided for the same chains (align = 0 or one chain: none) where the analysis's combine takes signs. */
typedef struct gpirt_run {
    gpirt_rstream_t rs;            /* NULL: item RNG (GPIRT_RNG_ITEM); else R's stream (GPIRT_RNG_RSTREAM, chains = 1): the
                                    * chain is gpirt_mcmc_summary's -- draws, IRFs and R's stream position bit-identical */
    gpirt_quantiles* quantiles;    /* every chain also keeps GPIRT_SUM_THETA_HIST | GPIRT_SUM_IRF_BAND; gpirt_summary_quantiles
                                    * of the chains' states.  NULL: no histograms, no bands.  chains x S < 2^32 */
    gpirt_ppc* ppc;                /* the posterior predictive checks, pooled by gpirt_ppc_combine */
    gpirt_ranks* ranks;            /* the rank posteriors of every chain's theta: pivots, n_pivots and pairwise given; n <=
                                    * GPIRT_RANK_MAX_N, chains x S < 2^32 */
    const double* h_y_new;         /* scoring: n_new x m on the host, +1 / -1 / NaN; NULL and 0 without score */
    int64_t n_new;                 /* 1..GPIRT_SCORE_MAX_N */
    gpirt_score* score;            /* scoring y_new against every chain's f* */
    gpirt_score_predict* predict;  /* needs score: the prediction of y_new's unseen answers, accumulated inside the score's
                                    * accumulate; top in 1..GPIRT_PREDICT_MAX_TOP */
    gpirt_ppc_pairs* pairs;        /* needs ppc: the pairwise item checks, accumulated inside the PPC's accumulate; top in
                                    * 1..GPIRT_PAIRS_MAX_TOP, n <= GPIRT_PAIRS_MAX_N */
    gpirt_ppc_bins* bins;          /* needs ppc: the theta-binned item fit, h and cuts given; inside the PPC's accumulate as the
                                    * pairs; top in 1..GPIRT_BINS_MAX_TOP */
    gpirt_shape* shape;            /* the IRF shape posteriors, k_half, n_tols and tols given: every chain's curves gbar (which
                                    * the checkpoint then carries); chains x S < 2^32 */
    gpirt_sumscore* sumscore;      /* the sum-score posteriors of every chain's f*; items given or NULL (all m) */
    gpirt_ppc_dif* dif;            /* needs ppc: the group-wise item fit, G, groups, h and cuts given; inside the PPC's
                                    * accumulate as the pairs and the bins; top in 1..GPIRT_DIF_MAX_TOP */
    gpirt_equate* equate;          /* the two-form score equating of every chain's f*, both masks given; pooled in chain
                                    * order (no signs: see REFLECTION above) */
    gpirt_loo* loo;                /* PSIS-LOO of every chain's f + mu with T = chains x sample_iterations; each finished chain
                                    * is merged into the pooled state and freed (at most two states are alive), then the pooled
                                    * state is finished into loo */
    gpirt_shape_order* order;      /* needs shape: the item-pair order posteriors; every chain's shape accumulation also runs
                                    * the order kernels, pooled without signs; the shape block is bit for bit what it is
                                    * without; m in 2..GPIRT_ORDER_MAX_M, top in 1..GPIRT_ORDER_MAX_TOP */
    void* reserved[8];             /* must be NULL: the next analyses go here */
} gpirt_run;
/* gpirt_mcmc_chains with the analyses that run names (library version 119; run == NULL, a non-NULL reserved slot and a
 * dependant without its base are GPIRT_E_ARG).  With run->rs it needs GPIRT_RNG_RSTREAM and chains = 1, without it
 * GPIRT_RNG_ITEM.  A run with every analysis NULL and no rs is gpirt_mcmc_chains. */
int gpirt_mcmc_run(const double* h_y, int64_t n, int64_t m, const double* h_theta0, int chains,
                   int sample_iterations, int burn_iterations, const double* h_prior_means,
                   const double* h_prior_sds, const double* h_step_sizes, const gpirt_options* opts, int align,
                   gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws, double* h_beta_draws, double* h_f_draws,
                   double* h_irfs, gpirt_summary* pooled, gpirt_diag* diag, gpirt_run* run);

/* Stage-level sampler for hosts that drive the loop themselves (bench.py, multi-GPU hosts that
 * put a collective between stages).  State lives on the device.  h_y holds +1, -1 or NaN (a missing response); any
 * other value is refused with GPIRT_E_ARG (gpirt_mcmc creates its sampler here). */
int gpirt_sampler_create(gpirt_sampler_t* s, gpirt_handle_t h, const double* h_y, int64_t n,
                         int64_t m, const double* h_theta0, const double* h_prior_means,
                         const double* h_prior_sds, const double* h_step_sizes,
                         const gpirt_options* opts, gpirt_rstream_t rs);
int gpirt_sampler_destroy(gpirt_sampler_t s);
int gpirt_sampler_init(gpirt_sampler_t s);               /* src/gpirtMCMC.cpp:13-47 */
int gpirt_sampler_step(gpirt_sampler_t s);               /* one full iteration, :68-78 / :87-97 */
/* the stages of one iteration, in the reference's order */
int gpirt_sampler_draw_f(gpirt_sampler_t s);             /* :68 / :87 */
int gpirt_sampler_draw_fstar(gpirt_sampler_t s);         /* :69 / :88 */
int gpirt_sampler_theta_partial(gpirt_sampler_t s);      /* local-item part of draw_theta's log-posterior */
int gpirt_sampler_theta_finish(gpirt_sampler_t s);       /* :70 / :89 (after any cross-rank reduction) */
/* Respondent-block form of draw_theta for item-sharded runs (replaces theta_partial / all-reduce / theta_finish):
 * once, hand over this rank's block of the response matrix with ALL item columns (host, n_block x m_total,
 * column-major, same coding as y); per iteration gather every rank's f* columns into the device array
 * "fstar_full" (N x m_total, gpirt_sampler_devptr), call theta_block -- draw-theta.cpp:15-34 for the respondents
 * [i0, i0 + n_block), result in "theta_stage" (n values, zero outside the block) --, sum "theta_stage" over the
 * ranks and call theta_commit.  Draws are keyed by the global respondent index: independent of the partition. */
int gpirt_sampler_set_theta_block(gpirt_sampler_t s, const double* y_block, int64_t i0, int64_t n_block, int64_t m_total);
int gpirt_sampler_theta_block(gpirt_sampler_t s);
int gpirt_sampler_theta_commit(gpirt_sampler_t s);
int gpirt_sampler_draw_beta(gpirt_sampler_t s);          /* :71-75 / :90-94 (beta, mu, mu_star) */
int gpirt_sampler_factor(gpirt_sampler_t s);             /* :76-78 / :95-97 */
/* K(theta, theta) + jitter into "L" (lower blocks; src/gpirtMCMC.cpp:76-77) without factoring: the first step of a
 * factorisation the host distributes with the gpirt_potrf_panel_* pieces on the "L" devptr; gpirt_sampler_skip_factor
 * then closes the iteration. */
int gpirt_sampler_build_cov(gpirt_sampler_t s);
/* The pieces on this sampler's own "L" (which may carry extra rows below the n x n factor, see gpirt_sampler_ldl):
 * panel_rows = number of rows of a panel's column block that travel (n + extra - p W rows for panel p). */
int gpirt_sampler_panel_factor(gpirt_sampler_t s, int64_t p);
int gpirt_sampler_panel_update(gpirt_sampler_t s, int64_t p, int64_t c);
int gpirt_sampler_panel_copy(gpirt_sampler_t s, int64_t p, double* d_buf, int to_buf);
int gpirt_sampler_panel_rows(gpirt_sampler_t s, int64_t* rows);
/* ... and by halves of an outer panel (gpirt_potrf_panel_*_part above) */
int gpirt_sampler_panel_factor_part(gpirt_sampler_t s, int64_t p, int half);
int gpirt_sampler_panel_update_part(gpirt_sampler_t s, int64_t p, int64_t c, int part);
int gpirt_sampler_panel_copy_part(gpirt_sampler_t s, int64_t p, int half, double* d_buf, int64_t buf_doubles, int to_buf);
/* Close the iteration WITHOUT factoring: "L" arrived from elsewhere (a broadcast into the "L" devptr, the distributed
 * pieces, gpirt_sampler_set).  rows_with_L != 0: the rows below the n x n factor (gpirt_sampler_ldl) arrived with it,
 * i.e. the whole ldl x n buffer was received; 0: only the n x n factor is current and the rows are rebuilt by the
 * explicit forward solve (src/draw-fstar.cpp:19) before draw_fstar reads them.  gpirt_sampler_skip_factor(s) is
 * gpirt_sampler_adopt_factor(s, 0), the form that is safe for any host. */
int gpirt_sampler_adopt_factor(gpirt_sampler_t s, int rows_with_L);
int gpirt_sampler_skip_factor(gpirt_sampler_t s);
int gpirt_sampler_accumulate_irf(gpirt_sampler_t s);     /* :103 */
/* Posterior summaries on the stage API: summary_enable allocates and zeroes the accumulators of `parts` (0 frees them);
 * summary_accumulate adds the CURRENT state as one draw (call it after the step of a sampling iteration); summary_get
 * finishes one array ("p_yes", "lppd", "p_waic", "f_mean", "f_var", "theta_mean", "theta_var", "beta_mean", "beta_var";
 * GPIRT_SUM_THETA_HIST: "theta_hist", "theta_hist_h1", "theta_hist_h2" (1001 x n, counts as doubles; the halves need
 * GPIRT_SUM_DIAG), "theta_off_grid" (n); GPIRT_SUM_IRF_BAND: "irf_p_mean" (1001 x m), "irf_band" (1001 x m x 256: the
 * bin last), "irf_nan" (1001 x m); count <= its size) and copies it out; summary_totals writes GPIRT_SUM_NTOTALS doubles (needs GPIRT_SUM_WAIC). */
int gpirt_sampler_summary_enable(gpirt_sampler_t s, int parts);
int gpirt_sampler_summary_accumulate(gpirt_sampler_t s);
int gpirt_sampler_summary_get(gpirt_sampler_t s, const char* name, double* h_out, int64_t count);
int gpirt_sampler_summary_totals(gpirt_sampler_t s, double* h_totals);
int gpirt_sampler_iteration(gpirt_sampler_t s, int* iter);
/* Sets the completed-iteration counter (the GPIRT_RNG_ITEM sub-streams are keyed by it): lets a second sampler
 * replay a stage of another one's iteration on copied state (bench.py's in-run check of the draw_fstar forms). */
int gpirt_sampler_set_iteration(gpirt_sampler_t s, int iter);
int gpirt_sampler_check(gpirt_sampler_t s);              /* syncs; returns potrf info / GPIRT_E_* */
/* Device pointer of a named state array ("theta","f","beta","mu","mu_star","fstar","L","logpost",
 * "irf_sum","ess_k") and its element count; the pointer stays valid until destroy. */
int gpirt_sampler_devptr(gpirt_sampler_t s, const char* name, void** d_ptr, int64_t* count);
/* Leading dimension of the "L" device array.  With n % 64 == 0 the array is (n + e) x n: e rows below the factor enter
 * the factorisation as K(c, theta) (rank-r K*, e = r) or K(theta*, theta) (e = 1024: the 1001 grid points, n >= 1024)
 * and leave it as (L^-1 K(theta, .))^T -- draw_fstar's forward solve (src/draw-fstar.cpp:19) comes out of a bordered
 * factorisation.
 * gpirt_sampler_get / _set("L") always move the n x n factor.
 * Every such layout also carries 64 NODE rows, K(c_64, theta) for the 64 Chebyshev nodes of the rank-64 form, which leave
 * the factorisation as K(c_64, theta) L^-T: with r = 64 they are draw_fstar's rows (e = 64); with another rank r they come
 * first and the r rows behind them (e = 64 + r); with the grid rows they follow the 1024 (e = 1088); a sampler with
 * neither (rank 0, n < 1024) carries them alone (e = 64), and so does every sampler under GPIRT_BORDERED=2, which switches
 * off draw_fstar's rows only (f does not depend on that switch).
 *
 * draw_f of a sampler under GPIRT_RNG_ITEM forms nu = L z from them (csrc/nu_lr.hip): below a block P of 512 columns
 * L[i, P] = V[i, :] Bt[:, P] with V the Lagrange basis of the nodes at theta_i and Bt the node rows, so
 *   nu[P, :] = L[P, P] Z[P, :] + V[P, :] sum_{Q < P} Bt[:, Q] Z[Q, :]
 * -- about a tenth of the n^2 m flops.  nu then equals L z TO ROUNDING, not bit for bit: measured on the device max |nu - L z| <= 1e-11 with max |nu| = 3 (n = 8192; 2.3e-12 at n = 1088), against the 1e-9 every oracle comparison of f uses.  It does not
 * depend on the draw_fstar form, on m or on item0 (an item shard's f is bit-identical to the same columns of the full problem).
 * It runs when n % 64 == 0, n >= 2048, the handle's kernel passes gpirt_kernel_check(kernel,
 * 64) (under gpirt_sampler_ell_enable: at the grid's smallest length scale), kernel_fp32 == 0, every theta is finite and
 * inside [-5, 5] (theta_init and gpirt_sampler_set("theta") are looked at on the host; draw_theta's values are grid values),
 * and L is the factor of K(theta, theta): a gpirt_sampler_set("theta") that no factorisation, adopted factor or
 * gpirt_sampler_set("L") has followed takes the dense product, and a caller who sets both sets a matching pair.
 * Otherwise the dense product runs, as before.  GPIRT_NU_LR (gpirt_config_set): 1 this rule, 2 always dense, 3 at every
 * eligible n.  GPIRT_NU_SUB (library version 138): the width of the product's blocks P, 64, 128 (the default), 256 or 512 --
 * any cut into multiples of 64 satisfies the identity, the factor's own parts stay 512 wide, and a value outside the four is
 * GPIRT_E_ARG; the width changes nu in rounding only and can be changed between draws.
 * The operators gpirt_draw_f / gpirt_trmm_lz are given L, not theta, and keep the dense product.
 * gpirt_sampler_nu_lr_draws: how many draws of this sampler have run the structured product; gpirt_sampler_nu_lr_rows:
 * the node rows as they stand (64 x n, column-major, count = 64 n; GPIRT_E_ARG when the layout carries none). */
int gpirt_sampler_ldl(gpirt_sampler_t s, int64_t* ldl);
int gpirt_sampler_nu_lr_draws(gpirt_sampler_t s, int64_t* draws);
int gpirt_sampler_nu_lr_rows(gpirt_sampler_t s, double* h_out, int64_t count);
/* Library version 130.  The rank-64 draw_fstar (kstar_rank = 64, bordered layout) needs C = S^-1 U, U = K(theta, c_64).  With
 * the same basis V and Kcc = K(c_64, c_64) = F F^T (F from a long-double Jacobi eigendecomposition on the host, once per
 * kernel) S = (V F)(V F)^T + 0.001 I, so
 *   C = V M,   M = F (F^T (V^T V) F + 0.001 I)^-1 F^T   (64 x 64)
 * -- a 64 x 64 x n Gram product, one 64 x 64 factorisation and solve in a single work-group, an n x 64 x 64 product: nothing
 * of L, where the transposed solve through L's block inverses could not start before the factorisation's last pivot block
 * (csrc/fstar_free.hip).  G = B^T B stays the product over the node rows: s is unchanged bit for bit;
 * mean and f* change to rounding (measured in DESIGN.md section 38, inside 1e-9 max(1, max|f*|) for a theta that is not
 * degenerate; for a theta on one or two points the forward error of S x = f, 8 n u cond(S), is the bound).  It does not depend
 * on m or item0.  It runs under the conditions of the structured nu = L z above and, besides: kstar_rank = 64 in the bordered
 * layout, GPIRT_RNG_ITEM, no length-scale update (gpirt_sampler_ell_enable) in force.  Otherwise the chain through L, as
 * before.  GPIRT_FSTAR_FREE (gpirt_config_set): 1 this rule, 2 always through L, 3 at every eligible n.
 * gpirt_sampler_fstar_free_draws: how many draw_fstar calls of this sampler have used such a C. */
int gpirt_sampler_fstar_free_draws(gpirt_sampler_t s, int64_t* draws);
/* Library version 131.  With both of the above in force a steady iteration reads of L only its 512-column diagonal parts
 * L[P, P] and the 64 node rows.  A sampler created with gpirt_options.factor_structured = 1 then builds exactly those, from
 * theta (csrc/factor_lr.hip): with G_P = V[<p]^T V[<p] the Gram of the basis rows in front of part P,
 *   A_P = F^T G_P F + 0.001 I = R_P R_P^T,  Xh_P = R_P^-1 F^T,  X_P = Xh_P V[P]^T,
 *   L[P, P] = chol(0.001 (I + X_P^T X_P)),  Bt[:, P] = 0.001 Xh_P^T (X_P L[P, P]^-T)
 * -- 1.5e9 flop at n = 8192 instead of n^3 / 3 = 1.8e11; every pivot is >= sqrt(0.001).  The triangle of L below the parts is
 * NOT written.  Parts and rows equal the dense factor's to rounding (measured in DESIGN.md section 39); they do not depend on
 * m or item0 (an item shard's are bit-identical).  It runs where the structured nu = L z and C from theta alone both would
 * (their switches included), gpirt_sampler_init excepted.  GPIRT_FACTOR_LR (gpirt_config_set): 1 this rule from n = 2048,
 * 2 always the dense factor, 3 at every eligible n.
 * Whatever reads more of L first replaces it by the dense factor of K(theta_L, theta_L), theta_L the theta the structured
 * factor was built from (a gpirt_sampler_set("theta") in between does not change which matrix is factored): the dense nu = L z,
 * the solves of the other draw_fstar forms, the length-scale update, gpirt_sampler_get("L"), gpirt_sampler_devptr("L"),
 * gpirt_sampler_copy_state (on src), the factorisation in pieces.  A caller who keeps the pointer of gpirt_sampler_devptr("L")
 * across factorisations calls gpirt_sampler_dense_factor before reading through it.
 * gpirt_sampler_factor_lr_count: factorisations of this sampler that built the parts and rows alone;
 * gpirt_sampler_dense_factor_count: dense factorisations it enqueued, those on demand included;
 * gpirt_sampler_dense_factor: the dense factor now, if L holds a structured one (otherwise nothing);
 * gpirt_sampler_factor_lr_parts: the diagonal parts as they stand, WITHOUT forming the dense factor: 512 x n column-major,
 * column j holding L[p + i, j], i = 0 .. w - 1, for its part [p, p + w) (zero behind a shorter last part); count = 512 n.
 * Library version 132: the structured factor runs one launch per 64-column round (12 launches at n = 8192 instead of 29;
 * DESIGN.md section 40).  The same sums in the same order: parts and rows are bit for bit those of version 131.
 * GPIRT_FLR_FUSE (gpirt_config_set): 1 these launches (the default), 2 the launches of version 131.  No change to this interface.
 * Library version 140: draw_f's product reads diagonal parts GPIRT_NU_SUB wide and nothing else reads the parts, so the
 * structured factor builds parts of that width, width / 64 rounds instead of eight (the identities above
 * hold for any cut into multiples of 64).  GPIRT_FLR_NARROW (gpirt_config_set): 1 this from n = 2048 on (the default), 2 always
 * 512-wide parts (version 139, bit for bit), 3 at every eligible n.  Parts and node rows change in rounding only.  Whoever reads
 * wider parts than L holds -- draw_f after GPIRT_NU_SUB was raised on a live sampler, gpirt_sampler_factor_lr_parts -- first
 * replaces the factor by the structured factor of K(theta_L, theta_L) in 512-wide parts; that counts in neither counter.
 * gpirt_sampler_factor_lr_width: the width of the parts L holds, 0 for a dense L;
 * gpirt_sampler_factor_lr_blocks: those parts as they lie, nothing factored for it: width x n column-major, column j holding
 * L[p + i, j], i = 0 .. w - 1, for its part [p, p + w) (zero behind a shorter last part); count = width n; GPIRT_E_ARG when L is dense. */
int gpirt_sampler_factor_lr_count(gpirt_sampler_t s, int64_t* count);
int gpirt_sampler_dense_factor_count(gpirt_sampler_t s, int64_t* count);
int gpirt_sampler_dense_factor(gpirt_sampler_t s);
int gpirt_sampler_factor_lr_parts(gpirt_sampler_t s, double* h_out, int64_t count);
int gpirt_sampler_factor_lr_width(gpirt_sampler_t s, int* width);
int gpirt_sampler_factor_lr_blocks(gpirt_sampler_t s, double* h_out, int64_t count);
/* dst's chain state := src's (theta, f, beta, mu, mu_star, fstar, L, iteration counter); same handle, same n and m.  The kernel
 * is not part of the state: refused (GPIRT_E_ARG) when the two samplers' kernels differ, or while the length-scale update
 * (gpirt_sampler_ell_enable) is on for either -- its index and tables are not copied. */
int gpirt_sampler_copy_state(gpirt_sampler_t dst, gpirt_sampler_t src);
int gpirt_sampler_get(gpirt_sampler_t s, const char* name, double* h_out, int64_t count);
int gpirt_sampler_set(gpirt_sampler_t s, const char* name, const double* h_in, int64_t count);
int gpirt_sampler_finish_irfs(gpirt_sampler_t s, int sample_iterations, double* h_irfs); /* :106-111 */
/* Per-stage device time of the last gpirt_sampler_step (ms, hipEvents); names_out is a
 * NUL-separated list terminated by an empty string. */
int gpirt_sampler_enable_timing(gpirt_sampler_t s, int on);
int gpirt_sampler_stage_times(gpirt_sampler_t s, double* ms_out, int max_stages, int* n_stages,
                              const char** names_out);
/* Device time and launch count of the potrf trailing-update kernel accumulated since the last
 * reset (hipEvents on the launch stream); the roofline figure of bench.py. */
int gpirt_prof_trailing(gpirt_handle_t h, int reset, double* total_ms, int64_t* launches,
                        double* flops);
/* The same per class of syrk launch inside arma::chol's replacement (src/gpirtMCMC.cpp:17,78,97):
 * cls 0 = trailing update on the 128-tile kernel (what gpirt_prof_trailing reports), 1 = trailing update on the
 * 64-tile kernel, 2 = the update between the two sub-panels of an outer panel (K = gpirt_potrf_subpanel_width(n)).  flops are the
 * algorithmic ones of the lower trapezoid, 2 K (M N - N (N - 1) / 2).
 * The same instrument on two kernels of draw_f: cls 3 = nu = L Z of the item-keyed draw_f (src/mvnormal.h:10 for all m
 * columns as one triangular product: n^2 m flops), 4 = the R-stream replay's pass over L (rs3_products_kernel: bytes = the
 * lower triangle of L, 8 n (n + 1) / 2, flops = 2 x 32 candidate columns x n (n + 1) / 2).
 * And on draw_theta: cls 5 = the log-posterior product in fixed point on the int8 matrix cores (csrc/theta_fixed.hip:
 * "flops" = the int8 multiply-adds x 2 of its seven digit planes, 7 x 2 x 1001 x n x 2m). */
int gpirt_prof_syrk(gpirt_handle_t h, int cls, int reset, double* total_ms, int64_t* launches, double* flops);
/* algorithmic bytes of the same launches (call before the resetting gpirt_prof_syrk): the C trapezoid read and
 * written once, the M x K panel operand read once -- what the launch must move if nothing is re-read */
int gpirt_prof_syrk_bytes(gpirt_handle_t h, int cls, double* bytes);
int gpirt_prof_enable(gpirt_handle_t h, int on);

#ifdef __cplusplus
}
#endif
#endif /* GPIRT_HIP_H */
