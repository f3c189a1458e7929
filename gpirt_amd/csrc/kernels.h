// kernels.h -- internal launch functions of libgpirt_hip (device pointers, explicit stream).
#pragma once

#include "common.h"

namespace gpirt {

enum { TRI_NONE = 0, TRI_SYRK_LOWER = 1, TRI_A_LOWER = 2, TRI_A_UPPER = 3, TRI_SYRK_LOWER_TRAILING = 4,
       TRI_SYRK_LOWER_BACKGROUND = 5 /* deferred trailing update (GPIRT_DEFER): its own tile threshold GPIRT_BG128_MIN */ };
bool gemm_trailing_uses_128(int64_t M, int64_t N, bool background = false);
int launch_gemm_update_potf2(hipStream_t stream, int64_t M, int64_t N, int64_t K, const double* P, int64_t ldp,
                             double* C, int64_t ldc, int nb_next, int k0_next, int* info);   // does a trailing update of this shape run the 128-tile kernel?

// gemm_f64.hip
int launch_gemm(gpirt_handle_t h, hipStream_t stream, bool ta, bool tb, int tri, int64_t M,
                int64_t N, int64_t K, double alpha, const double* A, int64_t lda, const double* B,
                int64_t ldb, double beta, double* C, int64_t ldc, int64_t Mread = 0, const int* run_if = nullptr);
// run_if (plain products only): a device flag; the launch does nothing unless it is non-zero when the kernel starts.
// Mread (> M, !ta only): rows of A beyond M that exist in memory (padding up to a tile multiple) -- lets the
// last block row take the branch-free main loop; whatever those rows hold only reaches masked rows of C.

int launch_gemm_batched(hipStream_t stream, bool ta, bool tb, int tri, int64_t M, int64_t N, int64_t K, double alpha,
                        const double* A, int64_t lda, int64_t strideA, const double* B, int64_t ldb, int64_t strideB,
                        double beta, double* C, int64_t ldc, int64_t strideC, int batch);
// ... and C = A B + A2 B2 (both NN, TRI_NONE or TRI_A_LOWER on A) in one accumulator per 64-tile: A B's K range ascending, then
// the K2 terms of A2 B2 ascending; C is written once
int launch_gemm_batched_dual(hipStream_t stream, int tri, int64_t M, int64_t N, int64_t K, const double* A, int64_t lda,
                             int64_t strideA, const double* B, int64_t ldb, int64_t strideB, int64_t K2, const double* A2,
                             int64_t lda2, int64_t strideA2, const double* B2, int64_t ldb2, int64_t strideB2, double* C,
                             int64_t ldc, int64_t strideC, int batch);

// nparts consecutive trailing updates of one block column (panel q = columns [q * kpart, (q + 1) * kpart) of A / B) as one
// launch + an in-order application: bit-identical to nparts separate launches (work: nparts * M * N doubles)
int launch_syrk_panels(hipStream_t stream, int64_t M, int64_t N, int64_t kpart, int nparts, double alpha, const double* A,
                       int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, double* work);
int gemm_split_count(gpirt_handle_t h, hipStream_t stream, int tri, int64_t M, int64_t N, int64_t K);
// split-K product for small M x N with long K: parts land in Cpart (+ q * strideC, each M x N with ldc == M),
// then Cout (ldout) = beta_out * Cout + their sum
int launch_gemm_splitk(hipStream_t stream, bool ta, bool tb, int64_t M, int64_t N, int64_t K, double alpha,
                       const double* A, int64_t lda, const double* B, int64_t ldb, double* Cpart, int64_t ldc,
                       int64_t strideC, int nsplit, double* Cout, int64_t ldout, double beta_out);

// se_kernel.hip
int launch_se_kernel(hipStream_t stream, KernelSpec kern, const double* x1, int64_t n1, const double* x2, int64_t n2,
                     double* out, int64_t ld, double jitter);
// lower-triangular blocks only (upper blocks are left untouched): the potrf input.  fp32 (config C5): the default kernel only
int launch_se_kernel_lower(hipStream_t stream, KernelSpec kern, const double* x, int64_t n, double* out, int64_t ld,
                           double jitter, bool fp32 = false);
// host only (gpirt_kernel_check): the argument checks, and the rank certificate of include/gpirt_hip.h
int kernel_spec_from(const gpirt_kernel* k, KernelSpec* out);       // GPIRT_E_ARG with the message
int kernel_rank_check(const KernelSpec& kern, int kstar_rank, double* cert_out, int* min_rank_out);
// the r first-kind Chebyshev nodes on [-5, 5] rounded to fp64 and the barycentric Lagrange basis at the GPIRT_NGRID grid points
// (V[j + k N], evaluated in long double, rounded to fp64): what the rank-r draw_fstar holds on the device
void cheb_nodes_basis(int r, std::vector<double>& nodes, std::vector<double>& V);

// ell.hip: the length-scale update's own kernels (gpirt_sampler_draw_ell) and the grid on the host
// delta[j] = sum over item j's observed rows of t(y (f + mu)) - t(y (f' + mu)), nonfin[j] = its rows with a non-finite f'
int launch_ell_delta(hipStream_t st, const double* f, const double* fp, const double* mu, const double* y, int64_t n, int64_t m,
                     double* delta, int* nonfin);
// rec = {dll, log_ratio, log_u, accept, nonfinite}, flag = 0 rejected / 1 accepted / 2 failed / 3 hang guard (info: the factor's two words)
int launch_ell_decide(hipStream_t st, const double* delta, const int* nonfin, int64_t m, double lp_diff, double log_u,
                      const int* info, double* rec, int* flag);
int launch_ell_commit(hipStream_t st, const int* flag, double* f, const double* fp, int64_t count);     // f <- f' iff *flag == 1
// the centred update (gpirt_sampler_draw_ell_centred): dq[j] = sum_i (nu' - nu)(nu' + nu), nonfin[j] = item j's non-finite nu';
// out = {sum_i log L'_ii - log L_ii, the diagonal entries that are non-positive or non-finite};
// rec = {dq, dld, log_ratio, log_u, accept, nonfinite}, flag as launch_ell_decide's
int launch_ell_quad(hipStream_t st, const double* nu, const double* nup, int64_t n, int64_t m, double* dq, int* nonfin);
int launch_ell_logdet(hipStream_t st, const double* Lold, const double* Lnew, int64_t n, int64_t ldl, double* out);
int launch_ell_decide_centred(hipStream_t st, const double* dq, const int* nonfin, int64_t m, const double* ld, double lp_diff,
                              double log_u, const int* info, double* rec, int* flag);
// amp.hip: per-item GP amplitudes (gpirt_sampler_amp_*)
int launch_amp_scale(hipStream_t st, double* nu, const double* amp, int64_t n, int64_t m);              // nu_ij <- a_j nu_ij
struct AmpUpdateArgs {
    double* f; const double* mu; const double* y; int64_t n, m;
    const double* grid; const double* log_prior; int P;                 // device tables of P values
    int* idx; const int* width; double* amp;                            // m each
    long long* counts; double* rec;                                     // 4 x m, 5 x m, row-major (item j's values at stride m)
    uint64_t seed; uint32_t t; uint32_t item0;
};
// one update of every item's amplitude: one work-group per item, f rewritten in place where the item accepts
int launch_amp_update(hipStream_t st, const AmpUpdateArgs& a);
// draws[slot, j] = idx[j] (planned x m, row-major), hist[idx[j], j] += 1 (P x m, row-major)
int launch_amp_record(hipStream_t st, const int* idx, int64_t m, int P, int64_t slot, uint32_t* hist, int32_t* draws);
int amp_nearest_one(const double* grid, int P);                     // the grid point nearest 1 in log a (the first of a tie)
// amp_centred.hip: the centred amplitude update on the GP's rank-64 smooth part (gpirt_sampler_draw_amp_centred)
constexpr int AMP_CENTRED_RANK = 64;
struct AmpCentredArgs {
    double* f; const double* mu; const double* y; int64_t n, m;
    const double* theta; const double* nodes; const double* wts;        // the basis' inputs (launch_nu_lr_basis)
    const double* F; double eps;                                        // F with Kcc = F F^T, its dead columns zero; the jitter
    uint64_t live; int r;                                               // bit k: column k of F is live; r = their count
    double *V, *Gv, *parts; int nsplit;                                 // n x 64; 64 x 64; nsplit x 64 x max(64, m)
    double *Xh, *R;                                                     // 64 x 64 each: R^-1 F^T and R, R R^T = F^T V^T V F + eps I
    double *T, *Z, *W, *Xi, *Gc, *Q;                                    // 64 x m each (column j: item j), Q: m
    double* H;                                                          // n x m (ld n): h_j = V g_j
    const double *grid, *log_prior, *ln_a, *half_inv_a2; int P;         // device tables of P values
    int* idx; double* amp;                                              // m each, shared with the whitened update
    long long* counts; double* rec;                                     // 4 x m (updates, accepted, same, failed), 5 x m, row-major
    uint64_t seed; uint32_t t; uint32_t item0;
    int* err;                                                           // the sampler's numeric error word
};
// one centred update of every item's amplitude: the basis, V^T V, the small kernel, T = V^T f, the coefficients, H = V Gc, the update
int launch_amp_centred(hipStream_t st, const AmpCentredArgs& a);
// beta_centred.hip: the centred update of the mean function's coefficients, exact Gibbs with f + mu fixed (gpirt_sampler_draw_beta_centred)
constexpr int BETA_CENTRED_RANK = 64;
constexpr int64_t BETA_CENTRED_LDS_ROWS = 8192;                         // an item's f column stays in LDS up to this n (64 KB)
struct BetaCentredArgs {
    double *f, *beta, *mu, *mu_star; int64_t n, m, N;                   // the state it rewrites: n x m, 2 x m, n x m, N x m
    const double *theta, *tstar;                                        // n, N
    const double *pm, *ps;                                              // the prior's means and sds, 2 x m each
    const double* amp;                                                  // m, or nullptr: every a_j is 1.0
    const double* nodes; const double* wts;                             // the basis' inputs (launch_nu_lr_basis)
    const double* F; double eps;                                        // F with Kcc = F F^T, its dead columns zero; the jitter
    double *V, *Gv, *parts; int nsplit;                                 // n x 64; 64 x 64; nsplit x 64 x 64
    double *Xh, *R;                                                     // 64 x 64 each: R^-1 F^T and R, R R^T = F^T V^T V F + eps I
    double *P, *Gx, *W, *B;                                             // 64 x 2, 64 x 2, n x 2 (column-major), 4
    double *T, *Z, *mean, *beta_old, *beta_new, *chol, *rec;            // 2 x m each (column j: item j), chol 3 x m, rec m
    long long* counts;                                                  // 2 x m row-major: updates, failed
    uint64_t seed; uint32_t t; uint32_t item0;
    int* err;                                                           // the sampler's numeric error word
    hipEvent_t kev[2];                                                  // with timing on: recorded around the per-item kernel, else null
};
// one centred update of every item's coefficients: the basis, V^T V, the small kernel, P, Gx, W, B, the per-item kernel
int launch_beta_centred(hipStream_t st, const BetaCentredArgs& a);
// scale.hip: the collapsed scale and shift move, the linear mean's coefficients with theta summed out (gpirt_sampler_draw_scale)
enum { SCALE_REC_KIND = 0, SCALE_REC_Z, SCALE_REC_STEP, SCALE_REC_C, SCALE_REC_D, SCALE_REC_Q, SCALE_REC_J, SCALE_REC_LOGR,
       SCALE_REC_U, SCALE_REC_LOGU, SCALE_REC_STATUS, SCALE_REC_BAD, SCALE_REC_T, SCALE_REC_WIDTH, SCALE_REC_COUNT = 16 };
struct ScaleArgs {
    double *beta, *mu, *mu_star, *fstar, *logpost, *gbar; int64_t n, m, N;   // the state an accepted move rewrites (gbar: or nullptr)
    const double* theta;                                                // n
    const double *pm, *ps;                                              // the prior's means and sds, 2 x m each
    const double* log_prior; const int* codes;                          // the population prior's table and codes, or nullptr
    double *beta_prop, *mu2, *fstar2, *logpost2;                        // the proposal: 2 x m, N x m, N x m, N x n
    double *lz, *lz_prop, *dlz; int* bad;                               // n each
    double* rec;                                                        // SCALE_REC_COUNT doubles
    long long* counts;                                                  // 3 x 2 row-major: calls, accepted, failed of kind 0 / 1
    int kind; double width;
    uint64_t seed; uint32_t t;
    hipEvent_t kev[4];                                                  // with timing on: around logz, decide, the commits; else null
};
int launch_scale_curve(hipStream_t st, const ScaleArgs& a);             // z, the step, beta', mu2, fstar2
int launch_scale_decide(hipStream_t st, const ScaleArgs& a);            // lz, lz', the decision and the conditional commits
// pop.hip: the population prior for theta (gpirt_sampler_pop_*): group means and sds on two grids, and the host tables
struct PopUpdateArgs {
    const long long* stats;                                             // 4 x G, row-major: n_g, S1, S2, off_grid of this call
    const double* mu; const double* sd; int P_mu, P_sd;                 // the grids
    const double* hyper_mu; const double* hyper_sd; const double* lse;  // P_mu, P_sd, P_mu x P_sd (row-major)
    int* idx;                                                           // 2 x G: (a_g, b_g) pairs; group 0's are -1
    double* lp_mu; double* lp_sd;                                       // G x P_mu, G x P_sd: the last call's rows
    double* log_prior;                                                  // G x N: row g rebuilt
    long long* counts;                                                  // 4 x G, row-major: calls, updated, skipped, failed
    int G, N;
    uint64_t seed; uint32_t t;
};
// stats[0 .. 4G) (zeroed here) from theta's grid indices: integer atomics alone, so any order gives the same bits
int launch_pop_stats(hipStream_t st, const double* theta, const int32_t* codes, int64_t n, int G, long long* stats);
// one exact Gibbs update of (mu_g, sd_g) for every group g >= 1: one work-group of 256 threads per group
int launch_pop_update(hipStream_t st, const PopUpdateArgs& a);
// draws[slot, g] = (a_g, b_g) (planned x 2G int32), hist_mu[a_g, g] += 1 (P_mu x G), hist_sd[b_g, g] += 1 (P_sd x G)
int launch_pop_record(hipStream_t st, const int* idx, int G, int P_mu, int P_sd, int64_t slot, uint32_t* hist_mu, uint32_t* hist_sd,
                      int32_t* draws);
void pop_default_row(double* row);                                  // the N(0, 1) row as theta_sample_kernel forms it: its bits
void pop_normal_row(double mu, double sd, double* row);             // -(0.5 z z), z = (t_k - mu) / sd: the update kernel's bits
void pop_grids_fill(double mu_hi, int P_mu, double sd_lo, double sd_hi, int P_sd, double* mu, double* sd);
void pop_lse_fill(const double* mu, int P_mu, const double* sd, int P_sd, double* lse);     // long double, rounded once
// ordinal.hip: ordinal (graded) responses under the cumulative-logit model (gpirt_sampler_ordinal_*).  cat: n x m int8,
// column-major, 0 = missing; thr: m x (C - 1) threshold values, thr[j (C - 1) + c - 1] = b_{j,c}; counts: m x C int64 observed cells
struct EssOrdArgs {
    double* f; const double* nu; const double* mu; const int8_t* cat; const double* thr; const long long* counts;
    int C; int64_t n, m;
    int* k_out; int* err;                                               // as EssArgs
    uint64_t seed; uint32_t iter; uint32_t item0;
    int screen;
};
int launch_ess_ord(hipStream_t stream, const EssOrdArgs& a);          // the slice for f, item-keyed RNG only, n <= GPIRT_ORD_MAX_N
int launch_ord_indicators(hipStream_t stream, const int8_t* cat, int64_t n, int64_t m, int C, double* Y);      // Y: n x C m one-hot
int launch_ord_counts(hipStream_t stream, const int8_t* cat, int64_t n, int64_t m, int C, long long* counts);
// G[k, (c - 1) m + j] = -ll(b_c - f*) [c < C] - ll(f* - b_{c-1}) [c > 1] (N x C m, leading dimension ldg >= N)
int launch_ord_loglik_terms(hipStream_t stream, const double* fstar, int64_t N, int64_t m, int C, const double* thr, double* G, int64_t ldg);
int launch_ord_nan_fix(hipStream_t stream, const double* G, int64_t ldg, const int8_t* cat, int64_t n, int64_t m, double* lp, int64_t N,
                       int64_t ldlp);
struct BetaOrdArgs {
    double* beta; const double* theta; const int8_t* cat; const double* f; const double* thr;
    const double* pm; const double* ps; const double* step;
    int C; int64_t n, m, N; double* mu; double* mu_star;
    uint64_t seed; uint32_t iter; uint32_t item0;
};
int launch_draw_beta_ord(hipStream_t stream, const BetaOrdArgs& a);   // the slope's MH step; beta[0, :] is read and never written
struct OrdThrArgs {
    const double* f; const double* mu; const int8_t* cat; const long long* counts; int64_t n, m;
    const double* grid; const double* log_prior; int C, P, W;
    int* idx; double* thr;                                              // m x (C - 1): the state
    double* lp; int* window;                                            // m x (C - 1) x W, m x (C - 1): the last update's masses and windows
    long long* stat;                                                    // pinned, failed, updates
    uint64_t seed; uint32_t t; uint32_t item0;
};
int launch_ord_thresholds(hipStream_t stream, const OrdThrArgs& a);   // one window update of every threshold, one work-group per item
int launch_ord_irf(hipStream_t stream, const double* fstar, int64_t N, int64_t m, int C, const double* thr, double* cum);
int launch_ord_record(hipStream_t stream, const int* idx, int64_t m, int C, int P, int64_t slot, uint32_t* hist, int32_t* draws);
void ord_grid_fill(double hi, int P, double* out);                    // long double, rounded once: the centre exactly 0
// ordinal_fit.hip: fit output of the ordinal model accumulated one draw at a time (gpirt_sampler_ordinal_fit_*).  The state is ONE
// device block of 8-byte words: a header of OFIT_HEADER_WORDS int64 (the tag "OFIT", the layout version, n, m, C, parts, draws,
// item0), then the enabled parts' arrays in this order -- WAIC: double lse, ll_mean, ll_m2 [n x m] (a missing cell's ll_m2 is -1
// and its words are never touched); PRED: double [C - 1][n x m]; PPC: [OFIT_NUNIT][stride] (units: the m items, the n respondents,
// the whole matrix; stride = n + m + 1 rounded up to even; uint64 but for the two deviance sums) and uint64 [OFIT_NCAT][m][C].
constexpr int OFIT_HEADER_WORDS = 16;
constexpr int OFIT_LAYOUT_VERSION = 1;
enum { OFIT_U_N_OBS = 0, OFIT_U_OBS_SCORE, OFIT_U_SCORE_GE, OFIT_U_SCORE_GT, OFIT_U_REP_SUM, OFIT_U_REP_SUMSQ, OFIT_U_AGREE,
       OFIT_U_DEV_GE, OFIT_U_NONFINITE, OFIT_U_DEV_OBS, OFIT_U_DEV_REP, OFIT_NUNIT };
enum { OFIT_K_OBS = 0, OFIT_K_REP_SUM, OFIT_K_REP_SUMSQ, OFIT_K_GE, OFIT_K_GT, OFIT_NCAT };
struct OfitLayout { int64_t lse, mean, m2, pred, units, cats, words, cells, stride; };       // offsets in words, -1: not there
OfitLayout ofit_layout(int64_t n, int64_t m, int C, int parts);
struct OfitState {
    bool on = false;
    int64_t n = 0, m = 0, item0 = 0, draws = 0;
    int C = 0, parts = 0, strips = 0, rblocks = 0;
    OfitLayout L{};
    uint64_t* block = nullptr;
    double *rowd = nullptr, *cold = nullptr;          // a draw's partials: [strip][3][n], [row block][3][m]
    uint32_t *rowi = nullptr, *coli = nullptr, *colc = nullptr;       //   ... their packed counts; [row block][m][8] category counts
    double* unit_d = nullptr; uint64_t* unit_i = nullptr;             // the items' sums of a draw ([3][m]), for the total
    int8_t* rep = nullptr;                            // the last draw: the replicate (n x m), Delta and the score of every unit,
    double* last_delta = nullptr; int64_t *last_score = nullptr, *last_counts = nullptr;      //   the replicate's counts (m x C)
    std::vector<void*> allocs;
};
int64_t ofit_state_words(const OfitState* p);
int ofit_alloc(hipStream_t stream, OfitState* p, int64_t n, int64_t m, int C, int parts, int64_t item0, const int8_t* cat);
void ofit_free(OfitState* p);
int ofit_seal(hipStream_t stream, OfitState* p);      // refreshes the header (synchronises)
// one draw: f, mu (n x m doubles), cat (n x m int8) and thr (m x (C - 1)) on the device; iter = the completed-iteration counter
int launch_ofit_accumulate(hipStream_t stream, OfitState* p, const double* f, const double* mu, const int8_t* cat, const double* thr,
                           uint64_t seed, uint32_t iter);
int ofit_block_get(hipStream_t stream, const void* d_block, const char* name, void* h_out, int64_t bytes);
int ofit_last_get(hipStream_t stream, OfitState* p, const char* name, void* h_out, int64_t bytes);   // 1: not a last-draw name
int ofit_block_totals(hipStream_t stream, const void* d_block, gpirt_ordinal_fit* out);
int ofit_combine(gpirt_handle_t h, const void* const* d_states, int chains, void* d_out);
// ordinal_score.hip: scoring respondents who were not in the fit under ordinal responses, and their category predictions
// (gpirt_sampler_ordinal_score_*).  Two device blocks of 8-byte words, each with a header of OSCORE_HEADER_WORDS int64.
//   score:    (OSCORE_TAG, layout version, n_new, m, C, N, 0, 0), int64 draws[n_new], nonfinite[n_new], n_obs[n_new], double
//             lpd_acc[n_new] (starts at -inf), ll_sum[n_new], post_sum[n_new][N] (k fastest)
//   predict:  (OSPRED_TAG, layout version, n_new, m, C, N, pred_draws, pred_skipped -- the two counters are the epilogue kernel's),
//             the answered-mask of cat_new packed 64 cells a word (cell g = r + j n_new), double prob_sum[C][m][n_new] and
//             info_sum[m][n_new] (r fastest)
// Beside them: the one-hot Y (n_new x C m), the block's OWN table G (Np x C m, Np = 1024), the product T (N x n_new), the cleaned
// f*, the w table (m x C) and Wc (n_new) of the last draw; with predict the weights W (Np x n_new), the operand table
// B = [P_1 | ... | P_C | Hc] (Np x (C + 1) m) and the product W^T B (n_new x (C + 1) m).
constexpr int OSCORE_LAYOUT_VERSION = 1;
constexpr int OSCORE_HEADER_WORDS = 8;
constexpr int64_t OSCORE_TAG = 0x5243534F;            // "OSCR"
constexpr int64_t OSPRED_TAG = 0x5250534F;            // "OSPR"
struct OscoreState {
    bool on = false, pred_on = false;
    int64_t n = 0, m = 0;
    int C = 0;
    uint64_t *block = nullptr, *pblock = nullptr;
    int8_t* cat = nullptr;                            // device: n_new x m
    double *Y = nullptr, *G = nullptr, *T = nullptr, *fclean = nullptr, *logprior = nullptr, *wtab = nullptr, *Wc = nullptr;
    double *W = nullptr, *B = nullptr, *Cm = nullptr; // predict only
    int* flags = nullptr;                             // [0] a NaN in this draw's f*, [1 + j] in item j, [1 + m + r] r answered one
    int* go = nullptr;                                // predict: 1 when this draw's f* holds no NaN
    double lse_prior = 0.0;
    std::vector<void*> allocs;
};
int64_t oscore_state_words(const OscoreState* s);
int64_t oscore_pred_state_words(const OscoreState* s);
// refuses n_new outside 1..GPIRT_SCORE_MAX_N and a value outside 0..C before anything is allocated; h_cat_new: n_new x m, column-major
int oscore_alloc(hipStream_t stream, OscoreState* s, const int8_t* h_cat_new, int64_t n_new, int64_t m, int C, bool predict);
void oscore_free(OscoreState* s);
// one draw: fstar (N x m) and thr (m x (C - 1)) on the device
int launch_oscore_accumulate(gpirt_handle_t h, hipStream_t stream, OscoreState* s, const double* fstar, const double* thr);
int oscore_get(hipStream_t stream, OscoreState* s, const char* name, void* h_out, int64_t bytes);
// pools `chains` blocks into the host block h_out (the same layout; bytes: its size); signs (score only): -1 reverses the grid axis
int oscore_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, void* h_out, int64_t bytes);
int oscore_pred_combine(gpirt_handle_t h, int chains, const void* const* d_states, void* h_out, int64_t bytes);
// carry.hip: the consistent step's carry stage (gpirt_sampler_carry_f) and the prior check's reduction (gpirt_sampler_prior_quad)
struct CarryArgs {
    double* f; const double* theta; const double* fstar; const double* mu_star; int64_t n, m, N;       // f: n x m; fstar, mu_star: N x m
    const double* amp;                                                  // m amplitudes, or nullptr: 1.0
    // 6 words, {off_grid, nonfinite} three times: [0, 1] the sampler's life, [2 + 2 slot, ..] this call's, and the third pair is
    // zeroed by this launch for the next call (slot alternates 0 / 1 from call to call; all six start at zero)
    unsigned long long* counters; int slot;
    uint64_t seed; uint32_t iter; uint32_t item0; int nugget;
};
// f_ij <- fstar[k_i, j] - mu_star[k_i, j] (+ sd_j z_ij with nugget) for every row whose theta is a grid point: one launch
int launch_carry_f(hipStream_t st, const CarryArgs& a);
// q[j] = sum_i nu_ij^2 (nu: n x m, column-major), ell_quad_kernel's order
int launch_prior_quad(hipStream_t st, const double* nu, int64_t n, int64_t m, double* q);
int ell_grid_check(double lo, double hi, int P);                    // GPIRT_E_ARG with the message
void ell_grid_fill(double lo, double hi, int P, double* out);         // long double, rounded to fp64, the end points exact

// potrf.hip
int launch_potrf_lower(gpirt_handle_t h, hipStream_t stream, double* A, int64_t n, int64_t lda,
                       bool zero_upper, bool reset_info = true, int64_t extra_rows = 0);

int potrf_guard_reset(gpirt_handle_t h, hipStream_t stream);      // hang-guard fallback: see potrf.hip

// the same factorisation in pieces (distributed hosts): outer panel p = columns [p W, (p + 1) W)
int64_t potrf_panel_width();
int64_t potrf_subpanel_width(int64_t n);     // first sub-panel of an outer panel of an n x n factorisation (GPIRT_NBP, or by size)
// half: 0 = the panel's first sub-panel, 1 = the rest of it, 2 = the whole panel (persistent panel kernel for 0 / 1)
int potrf_panel_factor(gpirt_handle_t h, hipStream_t stream, double* A, int64_t n, int64_t lda, int64_t p, int64_t extra_rows = 0,
                       int half = 2);
// part: 2 = the whole update of block column c by panel p; 0 = what needs only the panel's first sub-panel; 1 = the rest
int potrf_panel_update(gpirt_handle_t h, hipStream_t stream, double* A, int64_t n, int64_t lda, int64_t p, int64_t c,
                       int64_t extra_rows = 0, int part = 2);
// half as for potrf_panel_factor: the columns of that part of the panel, rows from the part's first row down
// capacity: doubles the buffer holds (< 0: not checked) -- a part that does not fit is refused, never truncated
int potrf_panel_copy(hipStream_t stream, double* A, int64_t n, int64_t lda, int64_t p, double* buf, bool to_buf,
                     int64_t extra_rows = 0, int half = 2, int64_t capacity = -1);

// panel.hip: columns [K0, c1) of the Cholesky factor, all rows below, one persistent kernel
int launch_panel_ll(gpirt_handle_t h, hipStream_t stream, double* A, int64_t n, int64_t lda, int64_t K0, int64_t c1,
                    int64_t row_end = 0, unsigned long long* epoch_out = nullptr);
size_t panel_ll_smem_bytes();

// trsm.hip
int launch_trsm_lower(gpirt_handle_t h, hipStream_t stream, const double* L, int64_t n, int64_t ldl,
                      double* B, int64_t nrhs, int64_t ldb, bool trans, bool reuse_inverses = false);

// the block inverses launch_trsm_lower applies, exposed so that they can be built by ranges of 512-block pairs [p0, p1) as
// the factor's outer panels finish; *_mark tells the handle that its inverses now belong to (L, n, ldl)
int trsm_inverses_reserve(gpirt_handle_t h, hipStream_t stream, int64_t n, int64_t nrhs, bool thin);
int trsm_inverses_build(gpirt_handle_t h, hipStream_t stream, const double* L, int64_t n, int64_t ldl, bool thin,
                        int64_t p0, int64_t p1);
void trsm_inverses_mark(gpirt_handle_t h, const double* L, int64_t n, int64_t ldl, bool thin);

// rng.hip
int launch_item_uniforms(hipStream_t stream, uint64_t seed, uint32_t iter, uint32_t stage,
                         uint32_t item0, int64_t n_items, int64_t n_index, double* out, bool normal, bool compact = false);
// z (n x m) from the R stream: column j, row i <- rnorm from U[pos0 + j*stride + 2i], U[.. + 1]
int launch_rstream_normals(hipStream_t stream, const double* U, const uint64_t* d_pos,
                           int64_t col_stride, int64_t n, int64_t m, double* out);

// ess.hip
struct EssArgs {
    double* f; const double* nu; const double* y; const double* mu;
    int64_t n, m;
    int* k_out;           // rejection counts per column (may be null)
    int* err;             // device error flag (set when the slice loop hits its cap)
    // item RNG
    uint64_t seed; uint32_t iter; uint32_t item0;
    // R-stream replay (U != null): one column per launch, uniforms from U[*pos + 2n ...]
    const double* U; uint64_t* pos; uint64_t cap;
    int ll_exact;         // 1: log(1 + exp(-a)) through the library's exp and log, as written (GPIRT_LL_EXACT)
    int screen;           // 1: the register kernels decide a trial point by the single-precision screen where it can (ll_fast.h)
    // packed y and mu = b0 + theta b1 recomputed (ypk != null; item RNG, 2048 < n <= 8192: ess_kernel_lin).
    // y and mu are then not read; any other n or an R-stream replay is an argument error
    const uint32_t* ypk;  // launch_ess_pack's words, 512 per item
    const double* theta;  // [n]
    const double* beta;   // [2 m]: b0, b1 of item j at 2 j
    int grid;             // work-groups of that kernel, each striding over the items (<= 0 or > m: one per item)
};
int launch_ess(hipStream_t stream, const EssArgs& a);
// y (n x m, +1 / -1 / NaN) as ess_kernel_lin reads it: one word per (item, lane of 512), bit e = row lane + 512 e is observed,
// bit 16 + e = it is negative; rows >= n are not observed.  512 m words.  ess_pack_eligible: the n the packed kernel takes.
inline bool ess_pack_eligible(int64_t n) { return n > 2048 && n <= 8192; }
int launch_ess_pack(hipStream_t stream, const double* y, int64_t n, int64_t m, uint32_t* out);
int launch_ess_lin(hipStream_t stream, const EssArgs& a);     // (launch_ess calls it where a.ypk is set)
// R-stream replay of draw_f, three items per pass over L (rng_ess.hip; sampler.hip, do_draw_f)
constexpr int RS_KC = 512;           // columns of L per part of a candidate product (one work-group: four waves x 128 columns)
constexpr int RS_ROWS = 32;          // rows of L per work-group of a candidate product
constexpr int RS_SPEC_MIN_N = 64;    // below: item by item, four launches each
constexpr int RS3_SLOTS = 3;         // items a pass can resolve
constexpr int RS3_C1 = 15;           // slot 1: the item before consumed 0 .. 14 uniforms behind its first two
constexpr int RS3_C2 = 16;           // slot 2: the two items before consumed 0 .. 15 together
constexpr int RS3_NT = 2;            // 16-wide MFMA tiles of a pass ...
constexpr int RS3_CAND = 16 * RS3_NT;   // ... = its columns: [slot 0 | slot 1 x 15 | slot 2 x 16]
static_assert(1 + RS3_C1 == 16 && RS3_C2 == 16 * (RS3_NT - 1), "tile 0 = slots 0 and 1, the other tiles = slot 2");
constexpr int RS3_TRIALS = 8;        // trial points of a slice loop evaluated per meeting of the work-groups
constexpr int RS3_MAX_WGS = 256;     // work-groups of the slice kernel (32 R rows each, R <= 8 rows per thread)
constexpr int64_t RS3_MAX_N = (int64_t)RS3_MAX_WGS * 256;
constexpr int RS3_QSTRIDE = 4 * RS3_NT * 65;         // products: one wave's accumulators of ONE tile parity per lane in LDS (rows of 65: bank spread)
constexpr int RS3_LDS_DOUBLES = (4 * RS3_QSTRIDE > 5 * RS_KC + 16 + RS3_C2) ? 4 * RS3_QSTRIDE : 5 * RS_KC + 16 + RS3_C2;    //   the three Nrm windows of a part (5 RS_KC + 16 + RS3_C2 doubles), then the four waves' accumulators
static_assert(5 * RS_KC + 16 + RS3_C2 <= RS3_LDS_DOUBLES, "the windows must fit");
struct Rs3Args {
    const double* U; uint64_t cap;   // the window of stream uniforms
    double* Nrm;                     // Nrm[r] = rnorm(U[r], U[r + 1]) for r in [cursor at the start of draw_f, *nrm_end)
    uint64_t* anchor;                // (8 words; [3] = the predictor has stalled, [4] = rounds of 16 trial points its anchor item has already lost, rs_predict.hip)
                                     // [0] the first item no pass has resolved yet (m: all done, or the draw has failed)  [1] where
                                     //   its normals start  [2] the end of Nrm -- one 32-byte record, read once per work-group
    uint64_t* pos;                   // the cursor (start of the next unconsumed uniform)
    uint64_t* posv;                  // [m + 1]: where item j's normals start
    int* k_out;                      // [m]: rejection counts
    int* err;                        // the draw's error flag (the failing kernel also closes the anchor)
    int64_t n, m;
    const double* Lt; int64_t nkb;   // L in 1 KiB tiles of 32 rows x 4 columns (launch_rs_tiles), nkb = rs_tile_quads(n) tiles per row group
    double* part;                    // [parts][RS3_CAND][n] parts of the pass's candidate products
    const uint32_t* units;           // the products' work-groups: (row group bx) | (part by) << 16, the nfull full parts first
    int nunits, nfull;
    int lim1, lim2;                  // slots 1 / 2 take counts below these (RS3_C1 / RS3_C2; smaller only through gpirt_debug_rs_cand_limit)
    double* f; const double* y; const double* mu;      // n x m
    // the slice kernel's work-groups meet through partial[2][RS3_MAX_WGS][RS3_TRIALS + 1] and flags[2][RS3_MAX_WGS]: a
    // work-group raises its flag to the meeting's tag = tag + (meetings before it in this launch); the host hands every
    // launch a range of 2^20 tags above all earlier ones, so nothing is ever reset
    double* partial; unsigned long long* flags; uint64_t tag;
    long long* trace;                // debug (gpirt_debug_rs_trace): in-kernel time stamps of this pass, or null
    // the predicted replay (rs_predict.hip): the predictor's passes work on single-precision tiles of L and leave
    // single-precision parts; anchor[3] != 0 = the predictor has stalled
    const float* Lt32; int64_t nk8;  // L in 1 KiB tiles of 32 rows x 8 columns of floats (launch_rs32_tiles), nk8 = rs32_tile_octs(n) per row group
    float* part32;                   // [parts][RS3_CAND][n]; non-null selects the predictor's form of the slice kernel
    int mispredict;                  // debug (gpirt_debug_rs_mispredict): the predictor is off by one at every mispredict-th item
    // rs3p_decide_kernel: partial sums [work-group][17], the candidates' walk records [32][18], the ticket (monotonic)
    double* dec_part; double* dec_rec; unsigned* dec_ticket;
    uint64_t* pass_count;            // += 1 per real pass of the predictor (rs_ctl[3])
    // the predictor's structured form (rs_lr.hip): the blocks of L below the diagonal parts as V C
    int lr;                          // != 0: the units are the diagonal parts + 2 row groups of C per part (bit 31 of the unit word);
                                     //       rs_lr_apply_kernel completes part 0 of part32, the decide kernel reads that one part
    const float* Ct32;               // C in the tile layout of Lt32: RS_LR_RANK rows
    float* lrY;                      // [parts][RS3_CAND][RS_LR_RANK]: y_J = C_J z_J of the pass
    const float* V32t;               // [RS_LR_RANK][n]: the Lagrange basis at theta
};
inline int64_t rs_tile_quads(int64_t n) { return (n + 3) / 4 + 1; }
inline size_t rs_tile_doubles(int64_t n) { return (size_t)((n + RS_ROWS - 1) / RS_ROWS) * (size_t)rs_tile_quads(n) * 128; }
int launch_rs_tiles(hipStream_t stream, const double* L, int64_t n, int64_t ldl, double* Lt);
int launch_rs_unpack(hipStream_t stream, const uint32_t* raw, int64_t count, double* out);   // MT words -> unif_rand() values
int launch_rs3_begin(hipStream_t stream, const Rs3Args& a, uint64_t span);   // Nrm over [cursor, cursor + span), anchor 0
int launch_rs3_products(hipStream_t stream, const Rs3Args& a);
void rs3_unit_table(int64_t n, std::vector<uint32_t>& units, int* nfull);
int rs3_slice_wgs(int64_t n);
int rs3_slice_rows(int64_t n);
int launch_rs3_slice(hipStream_t stream, const Rs3Args& a);
// rs_predict.hip: the predicted replay (phase A on single-precision tiles of L, phase B = one fp64 product + all slice loops
// side by side + an in-order commit)
constexpr int RS_LR_RANK = 64;       // Chebyshev nodes of the predictor's structured form (rs_lr.hip)
// (whole parts of 512 columns: the structured form's units read every oct of the part that holds a row group's diagonal)
inline int64_t rs32_tile_octs(int64_t n) { return ((n + 511) / 512) * 64 + 1; }
inline size_t rs32_tile_floats(int64_t n) { return (size_t)((n + RS_ROWS - 1) / RS_ROWS) * (size_t)rs32_tile_octs(n) * 256; }
#ifndef RS3P_KC_VALUE
#define RS3P_KC_VALUE 512
#endif
constexpr int RS3P_KC = RS3P_KC_VALUE;   // columns of L per unit of the PREDICTOR's products (its own unit table: rs3p_unit_table)
void rs3p_unit_table(int64_t n, std::vector<uint32_t>& units, int* nfull);
struct RsVerifyArgs {
    const double* f; double* nu; const double* y; const double* mu;    // n x m; nu = the product's columns for items j0 .. (n x (m - j0)), f' on return
    int64_t n, m, j0;
    const double* U; uint64_t cap;
    uint64_t* posv;                  // [m + 1] predicted starts; the commit corrects the entry behind a misprediction
    const uint64_t* anchorP;         // [0] = first item the predictor has NOT reached
    int* kv; int* used; int* ierr;   // [m]: rejections, uniforms consumed behind the normals, error code of each verified item
};
int launch_rs32_tiles(hipStream_t stream, const double* L, int64_t n, int64_t ldl, float* Lt, bool diag_only = false);
// rs_lr.hip: the structured form of the predictor's pass
struct RsLrSetup {
    const double* theta; int64_t n;
    const double* nodes; const double* wts; const double* Mn;     // RS_LR_RANK nodes, barycentric weights, K(c, c)
    double eps;                       // the jitter
    const double* L; int64_t ldl;     // the dense factor (its 64 x 64 diagonal blocks are read)
    double* V64; double* Gb;          // [64 ceil(n / 64)][RS_LR_RANK]; [ceil(n / 64)][RS_LR_RANK^2]
    float* V32t; float* Ct32; int64_t nk8;
    int* bad;                         // |= 1 zero pivot, 2 negative diagonal, 4 a coefficient beyond 1e6
};
void rs_lr_nodes(std::vector<double>& nodes, std::vector<double>& wts, std::vector<double>& M);
void rs_lr_unit_table(int64_t n, std::vector<uint32_t>& units);
int launch_rs_lr_setup(hipStream_t stream, const RsLrSetup& q);
int launch_rs_lr_apply(hipStream_t stream, const Rs3Args& a);
// nu_lr.hip: draw_f's nu = L z (item-keyed RNG) from L's diagonal parts and the 64 node rows below the factor
constexpr int NU_LR_RANK = 64;       // the nodes of cheb_nodes_basis(64)
constexpr int NU_LR_PART = 512;      // columns per part of the FACTOR at its widest (factor_lr.hip, gpirt_sampler_factor_lr_parts)
constexpr int NU_LR_SUB = 128;       // columns per part of the PRODUCT (GPIRT_NU_SUB: 64, 128, 256 or 512), measured
constexpr int NU_LR_SUB_MIN = 64;    // the narrowest width: what the workspace is sized for
inline bool nu_lr_sub_ok(int w) { return w == 64 || w == 128 || w == 256 || w == 512; }
struct NuLrArgs {
    const double* L; int64_t ldl;     // the dense factor
    const double* Bt;                 // its node rows, K(c, theta) L^-T (64 x n, leading dimension ldl)
    const double* V;                  // n x 64 (leading dimension n): the Lagrange basis at theta
    const double* Z; double* NU;      // n x m each
    double* T;                        // nu_lr_slabs(n) slabs of 64 x m; slab 0 is zero and stays zero
    int64_t n, m;
    int sub;                          // the product's part width (0: NU_LR_SUB)
};
void nu_lr_nodes(std::vector<double>& nodes, std::vector<double>& wts);
int64_t nu_lr_slabs(int64_t n);
int launch_nu_lr_basis(hipStream_t stream, const double* theta, int64_t n, const double* nodes, const double* wts, double* V);
int launch_nu_lr(hipStream_t stream, const NuLrArgs& a, double* flops, double* bytes);
// fstar_free.hip: the rank-64 draw_fstar's C = S^-1 K(theta, c) = V M from theta alone (V: launch_nu_lr_basis' n x 64)
constexpr int FSTAR_FREE_RANK = NU_LR_RANK;
void fstar_free_factor(const KernelSpec& kern, std::vector<double>& F);        // host: F (64 x 64) with K(c, c) = F F^T
int launch_fstar_free(hipStream_t stream, const double* V, int64_t n, const double* F, double eps, double* work, double* parts,
                      int nsplit, double* Cu, int* err);                        // work: 2 x 64 x 64, parts: nsplit x 64 x 64
// Xh[q] = R_q^-1 F^T, R_q R_q^T = F^T Gv[q] F + eps I, for `batch` 64 x 64 matrices Gv[q] (one work-group each); prefix: matrix q
// is Gv[1] + ... + Gv[q], added by its own work-group in slot order (Gv[0] is not read)
int launch_fstar_free_xhat(hipStream_t stream, const double* Gv, const double* F, double eps, double* Xh, int batch, int* err,
                           bool prefix = false, double* R = nullptr,      // R: also R itself, 64 x 64 per matrix (not with prefix)
                           bool chain = false);                           // chain: the prefix form's kernel without its sum
// factor_lr.hip: L's diagonal parts and the 64 node rows from theta alone -- nothing below the parts is computed
struct FactorLrArgs {
    const double* theta; int64_t n;
    const double *nodes, *wts;        // nu_lr_nodes on the device
    double* V;                        // n x 64 (leading dimension n): rewritten with the basis at theta
    const double* F; double eps;      // fstar_free_factor's F on the device; the jitter
    double *G, *Xh;                   // factor_lr_parts(n, part) x 64 x 64 each: the Grams in front of the parts; R_P^-1 F^T
    double* X;                        // 64 x n: the parts' borders
    double* D;                        // n / 64 x 64 x 64: the pivot blocks' factors until the last round is through
    double* L; int64_t ldl;           // the factor's buffer: the diagonal parts are written
    double* Bt;                       // its node rows (64 x n, leading dimension ldl): written
    int* err;                         // the sampler's numeric error word
    int part;                         // the parts' width: 64, 128, 256 or 512 (0: NU_LR_PART); anything else is an argument error
};
int64_t factor_lr_parts(int64_t n, int part = 0);
int launch_factor_lr(gpirt_handle_t h, hipStream_t stream, const FactorLrArgs& a);
int launch_rs3p_products(hipStream_t stream, const Rs3Args& a);
int launch_rs3p_decide(hipStream_t stream, const Rs3Args& a);
int launch_rs_pred_start(hipStream_t stream, const uint64_t* anchor, uint64_t* anchorP, const int* k_last, int64_t m);
int launch_rs_gather(hipStream_t stream, const double* Nrm, const uint64_t* posv, const uint64_t* anchorP, int64_t n, int64_t j0,
                     int64_t m, double* Z);
int launch_rs_verify(hipStream_t stream, const RsVerifyArgs& a);
int launch_rs_commit(hipStream_t stream, const RsVerifyArgs& a, uint64_t* anchor, uint64_t* pos, uint64_t* ctl, int* err, double* f,
                     int* k_out);
int launch_ll_term_probe(hipStream_t stream, const double* a, int64_t n, double* out, int fast);     // 0 written, 1 ll_fast, 2 screen
int launch_ll_bar(hipStream_t stream, const double* f, const double* y, const double* mu, int64_t n,
                  int64_t m, double* out);

// fstar.hip
int launch_colnorm_s(hipStream_t stream, const double* tmp, int64_t n, int64_t N, int64_t ld, double* s);
int launch_lowrank_s(hipStream_t stream, const double* V, int64_t N, int r, const double* G, int64_t ldg, double* s);
struct FstarEpiArgs {
    const double* mean; const double* mu_star; const double* s; double* out;
    int64_t N, m;
    uint64_t seed; uint32_t iter; uint32_t item0;
    const double* U; uint64_t* pos; uint64_t cap; int* err;   // R-stream replay when U != null
    double* mean_out;     // optional copy of mean + mu_star
    int* off_scratch;     // N + 1 ints of device scratch for the R-stream consumption offsets
    const double* amp;    // optional per-item amplitudes (m): sd = amp[j] * s[i]; null: sd = s[i]
};
int launch_fstar_epilogue(hipStream_t stream, const FstarEpiArgs& a);

// theta.hip
int launch_indicators(hipStream_t stream, const double* y, int64_t n, int64_t m, double* Ypm /* n x 2m */);
int launch_loglik_terms(hipStream_t stream, const double* fstar, int64_t N, int64_t m, double* Gpm /* ldg x 2m */, int64_t ldg,
                        const int* run_if = nullptr);
// behind the fp64 product (lp = Gpm Ypm^T, N x n): entries that came out NaN are summed again over the observed cells alone
int launch_theta_nan_fix(hipStream_t stream, const double* Gpm, int64_t ldg, const double* Ypm /* n x 2m */, int64_t n, int64_t m,
                         double* lp, int64_t N, int64_t ldlp, const int* run_if = nullptr);
// theta_fixed.hip: the same product in exact fixed point on the int8 matrix cores
struct TfDims { int64_t mp, ksteps, iblocks, gblocks; };
TfDims tf_dims(int64_t n, int64_t m, int64_t N);
size_t tf_y8_bytes(const TfDims& d);
size_t tf_gq_bytes(const TfDims& d);
size_t tf_aux_bytes(const TfDims& d);
int* tf_overflow(void* aux, const TfDims& d);
int launch_tf_indicators(hipStream_t stream, const double* y, int64_t n, int64_t ldy, int64_t m, const TfDims& d, void* Y8);
int launch_theta_fixed(hipStream_t stream, const double* fstar, int64_t N, int64_t n, int64_t m, const TfDims& d,
                       const void* Y8, void* Gq, void* aux, double* logpost, int64_t ldlp, bool trace = false,
                       gpirt_handle_t prof = nullptr);   // prof: the handle whose event-pair profiler brackets the int8 kernel (class 5)
long long* tf_trace(void* aux, const TfDims& d);            // (a traced launch: six stamps per work-group, tf_trace_wgs() of them)
int tf_trace_wgs();
struct ThetaArgs {
    const double* logpost;   // N x n (column i = respondent i0 + i), WITHOUT the prior
    int64_t N, n;
    int64_t i0;              // global index of the first respondent (a block of a sharded run; 0 otherwise):
                             // keys the RNG and offsets theta_out, so draws do not depend on the partition
    int stabilise;
    uint64_t seed; uint32_t iter;
    const double* U; uint64_t* pos; uint64_t cap;  // R-stream replay when U != null
    double* theta_out; int* degenerate; int* err;
    // the population prior (pop.hip): a G x N table of log masses and one code per respondent; both null: N(0, 1) as before
    const double* log_prior; const int32_t* codes;
};
int launch_theta_sample(hipStream_t stream, const ThetaArgs& a);

// beta.hip
struct BetaArgs {
    double* beta; const double* theta; const double* y; const double* f;
    const double* pm; const double* ps; const double* step;
    int64_t n, m, N;
    double* mu; double* mu_star;      // refreshed with the new beta (may be null)
    uint64_t seed; uint32_t iter; uint32_t item0;
    const double* U; uint64_t* pos; const uint64_t* item_off; uint64_t cap; int* err;  // R stream
    int screen;                       // 1: draw_beta_reg_kernel where it is eligible (GPIRT_BETA_SCREEN; y must be +1, -1 or NaN)
    int* path;                        // 2 x m, tests only (null in production): path[k + 2j] = 0 the screen decided step k, 1 full precision
};
int launch_draw_beta(hipStream_t stream, const BetaArgs& a);
int launch_linear_mean(hipStream_t stream, const double* x, int64_t n, const double* beta, int64_t m, double* mu);

// api.hip: an event pair around one launch while gpirt_prof_enable is on (classes: common.h); resolved by gpirt_prof_syrk
int prof_pair_begin(gpirt_handle_t h, hipStream_t stream, ProfPair& pp);
int prof_pair_end(gpirt_handle_t h, hipStream_t stream, ProfPair& pp, int cls, double flops, double bytes);

// api.hip: turns the hang-guard record of the panel kernel (info[1..7]) into the error message and clears it
int report_panel_guard(gpirt_handle_t h, const int* info_words, hipStream_t stream);

// api.hip
int create_side_handle(gpirt_handle_t* out, int device);

// summary.hip: posterior summaries accumulated one draw at a time (gpirt_sampler_summary_*, gpirt_mcmc_summary), and the
// combination of several chains' accumulators (gpirt_chains_combine)
constexpr int SUM_LAYOUT_VERSION = 1;
constexpr int SUM_HEADER_WORDS = 8;       // int64: n, m, parts, planned S, draws, layout version, grid points, 0
// offsets in doubles from the start of a state block (-1: the part is off); every one is even (16-byte aligned)
struct SumLayout {
    int64_t tb_mean = -1, tb_m2 = -1, lse = -1, ll_mean = -1, ll_m2 = -1, y = -1, p_sum = -1, f_mean = -1, f_m2 = -1, irf = -1;
    int64_t dtb[7] = { -1, -1, -1, -1, -1, -1, -1 };    // DIAG of theta / beta: half 1 (mean, M2), half 2 (mean, M2), batch sum,
    int64_t df[7] = { -1, -1, -1, -1, -1, -1, -1 };     // batch means (mean, M2); df: the same of f (DIAG and F)
    int64_t total = 0;
};
enum { DG_H1_MEAN, DG_H1_M2, DG_H2_MEAN, DG_H2_M2, DG_BSUM, DG_BM_MEAN, DG_BM_M2 };
SumLayout summary_layout(int64_t n, int64_t m, int parts);
// GPIRT_SUM_THETA_HIST / GPIRT_SUM_IRF_BAND: their arrays follow SumLayout's (offsets in doubles, -1: off; a uint32 array
// takes half a double per count, every array padded to 16 bytes).  total: the whole block.
struct QntLayout {
    int64_t th_hist[3] = { -1, -1, -1 };    // whole chain, half 1, half 2 (DIAG): uint32 n x GPIRT_NGRID, respondent-major
    int64_t th_off = -1;                     // uint32 n: draws off the grid
    int64_t psum = -1;                       // double GPIRT_NGRID x m: sum of plogis(f*)
    int64_t band_nan = -1;                   // uint32 GPIRT_NGRID x m
    int64_t band = -1;                       // uint32 GPIRT_IRF_BINS x (GPIRT_NGRID x m): bin-major, the f* cell fastest
    int64_t total = 0;
};
QntLayout quantile_layout(int64_t n, int64_t m, int parts);
void irf_band_edges(double* out);          // GPIRT_IRF_BINS - 1 edges logit(b / 256)
struct SummaryState {
    int parts = 0;                    // GPIRT_SUM_* (0: off)
    int64_t n = 0, m = 0, draws = 0, planned = 0;
    double* block = nullptr;          // the accumulators: ONE device block (SumLayout), header first
    SumLayout lay;
    double *tb_mean = nullptr, *tb_m2 = nullptr;                          // theta (n) then beta (2 x m): Welford
    double *lse = nullptr, *ll_mean = nullptr, *ll_m2 = nullptr;          // WAIC: log sum_s exp(ll_s), Welford of ll
    double *y = nullptr;                                                  // WAIC: a copy of y (the missing cells' mask)
    double *p_sum = nullptr;                                              // PRED: sum_s P(y = 1)
    double *f_mean = nullptr, *f_m2 = nullptr;                            // F: Welford of f
    double *irf = nullptr;                                                // a copy of the sampler's irf_sum (N x m)
    double *dtb[7] = {}, *df[7] = {};                                     // DIAG (SumLayout)
    QntLayout qlay;                                                       // THETA_HIST / IRF_BAND (and the block's size)
    uint32_t *th_hist[3] = {}, *th_off = nullptr;                         // THETA_HIST: whole chain, halves; off the grid
    uint32_t *band = nullptr, *band_nan = nullptr;                        // IRF_BAND: bins, NaN draws
    double *psum = nullptr, *edges = nullptr;                             // IRF_BAND: sum of plogis(f*); the bin edges
    double *out = nullptr, *part = nullptr, *tot = nullptr;              // a finished array, block partials, the totals
    std::vector<void*> allocs;
};
// zeroed accumulators; planned: the draw count S fixed for GPIRT_SUM_DIAG (0 without it)
int summary_alloc(SummaryState* s, int64_t n, int64_t m, int parts, int64_t planned = 0);
void summary_free(SummaryState* s);
// adds one draw; f, mu, y are n x m (16-byte aligned), theta n, beta 2 x m, fstar GPIRT_NGRID x m (GPIRT_SUM_IRF_BAND)
int launch_summary_accumulate(hipStream_t stream, SummaryState* s, const double* theta, const double* beta, const double* f,
                              const double* mu, const double* y, const double* fstar = nullptr);
// GPIRT_SUM_THETA_HIST / IRF_BAND arrays of summary_get by name (*found = false: not one of theirs), copied to h_out
int summary_hist_get(hipStream_t stream, const SummaryState* s, const char* name, double* h_out, int64_t count, bool* found);
// gpirt_summary_quantiles on h's stream
int summary_quantiles(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, int align,
                      gpirt_quantiles* q);
// the finished array `name` (p_yes, lppd, p_waic, f_mean, f_var, theta_mean, theta_var, beta_mean, beta_var) into s->out
int launch_summary_finish(hipStream_t stream, const SummaryState* s, const char* name, const double* y, double** d_out,
                          int64_t* count);
// the totals (GPIRT_SUM_T_*) into s->tot
int launch_summary_totals(hipStream_t stream, const SummaryState* s, const double* y);
// the header words and the IRF sum into the block (irf_sum: the sampler's, N x m); the block is then self-contained
int summary_seal(hipStream_t stream, SummaryState* s, const double* irf_sum, int64_t N);
// gpirt_chains_combine on h's stream (arguments as in include/gpirt_hip.h)
int chains_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, int align, double* h_irfs,
                   gpirt_summary* pooled, gpirt_diag* diag, int* signs_out = nullptr);     // signs_out: the C signs it decided

// ppc.hip: posterior predictive checks accumulated one draw at a time (gpirt_sampler_ppc_*, gpirt_run.ppc).  The state is ONE
// device block of 8-byte words: a header of 8 int64 (n, m, draws, layout version, item0, 0, 0, 0), then PPC_NARRAYS arrays of
// ppc_stride(n, m) words each, unit k = item k (k < m), respondent k - m (k < m + n) or the whole matrix (k = m + n).
constexpr int PPC_LAYOUT_VERSION = 1;
constexpr int PPC_HEADER_WORDS = 8;
enum { PPC_N_OBS, PPC_OBS_YES, PPC_SUM_R, PPC_SUM_R2, PPC_YES_GE, PPC_YES_GT, PPC_DEV_GE, PPC_CORRECT, PPC_NONFINITE,   // uint64
       PPC_DEV_OBS, PPC_DEV_REP,                                                                                        // double sums
       PPC_NARRAYS };
int64_t ppc_stride(int64_t n, int64_t m);           // n + m + 1 units, padded to an even count
int64_t ppc_state_words(int64_t n, int64_t m);
// ppc_pairs.hip: the pairwise item checks (gpirt_sampler_ppc_pairs_*, gpirt_run.pairs), an add-on to a PPC state.  Its
// accumulators are ONE device block of 8-byte words of their own: a header of PAIR_HEADER_WORDS int64 (n, m, layout version,
// pair_draws, pair_skipped, item0, 0, PAIR_TAG -- the two counters are kept by pair_update_kernel), the constant tables int32
// n_co, o11, o1 (m x m, pair (a, b) at [a m + b]), then uint64 sum_n11, sumsq_n11, sum_n1 and uint32 n11_ge, n11_gt, agree_ge,
// agree_gt, or_ge, or_gt, every array padded to 16 bytes.  Beside it: the 0 / 1 byte operands O8, Y8 (built once) and two planes
// of rep8 (ctl[0] names the plane of the last counted draw; the replicate writes the other one), the per-draw tables r11 and
// r1, and the control words ctl[0] = plane, ctl[1] = this draw holds a non-finite g.
constexpr int PAIR_LAYOUT_VERSION = 1;
constexpr int PAIR_HEADER_WORDS = 8;
constexpr int64_t PAIR_TAG = 0x52494150;              // "PAIR"
enum { PAIR_N_CO, PAIR_O11, PAIR_O1, PAIR_SUM_N11, PAIR_SUMSQ_N11, PAIR_SUM_N1, PAIR_N11_GE, PAIR_N11_GT, PAIR_AGREE_GE,
       PAIR_AGREE_GT, PAIR_OR_GE, PAIR_OR_GT, PAIR_NARRAYS };
struct PairLayout { int64_t off[PAIR_NARRAYS]; int64_t words; };      // offsets in 8-byte words from the start of the block
PairLayout pair_layout(int64_t m);
struct PairState {
    bool on = false;
    int64_t n = 0, m = 0, item0 = 0;
    int64_t iblocks = 0, ksteps = 0, plane = 0;       // the operands: item blocks of 32, k-steps of 32 respondents, bytes of one
    uint64_t* block = nullptr;
    unsigned char *O8 = nullptr, *Y8 = nullptr, *rep8 = nullptr;
    int *r11 = nullptr, *r1 = nullptr;
    int* ctl = nullptr;
    std::vector<void*> allocs;
};
int64_t pair_state_words(int64_t m);
inline int64_t pair_state_words(const PairState* p) { return pair_state_words(p->m); }
int pair_alloc(hipStream_t stream, PairState* p, int64_t n, int64_t m, int64_t item0, const double* y);
void pair_free(PairState* p);
// after the replicate pass has left this draw's bytes and its non-finite word: the products, then the decisions
int launch_pair_accumulate(hipStream_t stream, PairState* p);
int pair_get(hipStream_t stream, PairState* p, const char* name, void* h_out, int64_t bytes);
int pair_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_pairs* out);

// ppc_bins.hip: the theta-binned item fit (gpirt_sampler_ppc_bins_*, gpirt_run.bins), an add-on to a PPC state.  Its
// accumulators are ONE device block of 8-byte words of their own: a header of BIN_HEADER_WORDS int64 (n, m, layout version,
// bin_draws, bin_skipped, item0, B, BIN_TAG -- the two counters are kept by bin_update_kernel), BIN_CUT_WORDS int64 with the
// cuts, then the arrays of BinLayout, cell (b, j) at [b m + j], every array padded to 16 bytes.  Beside it: this draw's bins
// (uint8 per respondent, BIN_NONE off the grid), the last counted draw's, n_b, the control words ctl[0] = a theta is off the
// grid, ctl[1] = this draw holds a non-finite g in an observed cell, the replicate pass's partial tables per block of 256
// respondents ([row block][item][bin]: the packed counts N | T << 10 | R << 20, E and V) and the last counted draw's tables.
constexpr int BIN_LAYOUT_VERSION = 1;
constexpr int BIN_HEADER_WORDS = 8;
constexpr int BIN_CUT_WORDS = 16;
constexpr int64_t BIN_TAG = 0x534E4942;               // "BINS"
constexpr unsigned char BIN_NONE = 0xFF;
enum { BIN_SUM_N, BIN_SUM_T, BIN_SUM_R,                              // uint64, B x m
       BIN_SUM_E, BIN_SUM_Z,                                         // double, B x m
       BIN_CELL_GE, BIN_CELL_GT, BIN_CELL_EMPTY,                     // uint32, B x m
       BIN_CHI_GE, BIN_CHI_GT,                                       // uint32, m
       BIN_CHI_OBS, BIN_CHI_REP,                                     // double, m
       BIN_OCC,                                                      // uint64, B
       BIN_NARRAYS };
struct BinLayout { int64_t off[BIN_NARRAYS]; int64_t words; };       // offsets in 8-byte words from the start of the block
BinLayout bin_layout(int64_t m, int64_t B);
struct BinState {
    bool on = false;
    int64_t n = 0, m = 0, item0 = 0;
    int h = 0, B = 0, rblocks = 0;
    int cuts[GPIRT_BINS_MAX_H + 1] = {};
    uint64_t* block = nullptr;
    unsigned char *bin_cur = nullptr, *bin_last = nullptr;            // [n]
    uint32_t* nb = nullptr;                                           // [32]: this draw's n_b
    int* ctl = nullptr;
    uint32_t* part_i = nullptr; double *part_e = nullptr, *part_v = nullptr;      // [row block][m][B]
    int32_t* tab_i = nullptr; double* tab_d = nullptr;                // the last counted draw: [3][B][m] N, T, R; [2][B][m] E, V
    std::vector<void*> allocs;
};
int64_t bin_state_words(int64_t m, int64_t B);
inline int64_t bin_state_words(const BinState* p) { return bin_state_words(p->m, p->B); }
int bin_check_cuts(int h, const int* cuts);          // GPIRT_E_ARG (with the message) unless 1 <= d_1 < ... < d_h <= 499, 1 <= h <= 15
int bin_alloc(hipStream_t stream, BinState* p, int64_t n, int64_t m, int64_t item0, int rblocks, int h, const int* cuts);
void bin_free(BinState* p);
// before the replicate pass: this draw's bins, n_b and ctl[0] from theta (n doubles on the device); clears ctl[1]
int launch_bin_assign(hipStream_t stream, BinState* p, const double* theta);
// after the replicate pass has left this draw's partial tables and ctl[1]: the tables, the decisions, the accumulators
int launch_bin_update(hipStream_t stream, BinState* p);
int bin_get(hipStream_t stream, BinState* p, const char* name, void* h_out, int64_t bytes);
int bin_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ppc_bins* out);

// ppc_dif.hip: the group-wise item fit (gpirt_sampler_ppc_dif_*, gpirt_run.dif), an add-on to a PPC state.  Its accumulators
// are ONE device block of 8-byte words of their own: a header of DIF_HEADER_WORDS int64 (n, m, layout version, dif_draws,
// dif_skipped, item0, B, DIF_TAG -- the two counters are kept by dif_update_kernel), DIF_CUT_WORDS int64 with the cuts,
// DIF_GROUP_WORDS int64 (G, the groups' sizes), the n group codes as int8, then the arrays of DifLayout, cell (g, b, j) at
// [(g B + b) m + j] and (g, j) at [g m + j], every array padded to 16 bytes.  Beside it: this draw's cells (uint8 per
// respondent, DIF_NONE left out or off the grid), the last counted draw's, the cells' occupancy, the control words ctl[0] = a
// theta is off the grid, ctl[1] = a non-finite g in an observed cell of a grouped respondent, this draw's tables [3][G B][m]
// (N | T << 16 | R << 32, E and V in units of 2^-44; zero between draws: dif_update_kernel clears what it has read), the last
// counted draw's tables and statistics.
constexpr int DIF_LAYOUT_VERSION = 1;
constexpr int DIF_HEADER_WORDS = 8;
constexpr int DIF_CUT_WORDS = 16;
constexpr int DIF_GROUP_WORDS = 8;
constexpr int64_t DIF_TAG = 0x31464944;               // "DIF1"
constexpr unsigned char DIF_NONE = 0xFF;
constexpr int DIF_NSTATS = 8;
enum { DIF_SUM_N, DIF_SUM_T, DIF_SUM_R,                              // uint64, G x B x m
       DIF_SUM_E,                                                    // double, G x B x m
       DIF_OCC,                                                      // uint64, G x B
       DIF_YES_GE, DIF_YES_GT, DIF_CHI_GE, DIF_CHI_GT, DIF_MH_GE, DIF_MH_GT, DIF_MH_UNDEF, DIF_STD_UNDEF,      // uint32, G x m
       DIF_CHI_OBS, DIF_CHI_REP, DIF_MH_LOG_OBS, DIF_MH_LOG_REP, DIF_STD_OBS, DIF_STD_REP,                      // double, G x m
       DIF_NARRAYS };
static_assert(DIF_NARRAYS == GPIRT_DIF_NRAW, "gpirt_ppc_dif::raw");
struct DifLayout { int64_t groups; int64_t off[DIF_NARRAYS]; int64_t words; };     // offsets in 8-byte words
DifLayout dif_layout(int64_t n, int64_t m, int64_t G, int64_t B);
struct DifState {
    bool on = false;
    int64_t n = 0, m = 0, item0 = 0;
    int G = 0, h = 0, B = 0;
    int cuts[GPIRT_BINS_MAX_H + 1] = {};
    uint64_t* block = nullptr;
    unsigned char *cell_cur = nullptr, *cell_last = nullptr;          // [n]
    uint32_t* occ = nullptr;                                          // [128]: this draw's members per cell
    int* ctl = nullptr;
    uint64_t *tab = nullptr, *tab_last = nullptr;                     // [3][G B][m]
    double* stat_last = nullptr;                                      // [DIF_NSTATS][G][m]
    std::vector<void*> allocs;
};
int dif_check_groups(int64_t n, int G, const int32_t* groups, int64_t* sizes);      // GPIRT_E_ARG with the message
int dif_alloc(hipStream_t stream, DifState* p, int64_t n, int64_t m, int64_t item0, int G, const int32_t* groups, int h,
              const int* cuts);
void dif_free(DifState* p);
// one draw: the cells from theta, the tables from f, mu, y and the PPC's uniforms, then the statistics and the accumulators
int launch_dif_accumulate(hipStream_t stream, DifState* p, const double* f, const double* mu, const double* y, uint64_t seed,
                          uint32_t iter, const double* theta);
int64_t dif_state_words(const DifState* p);
int dif_get(hipStream_t stream, DifState* p, const char* name, void* h_out, int64_t bytes);
int dif_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ppc_dif* out);

// ppc_scores.hip: the score-based checks (gpirt_sampler_ppc_scores_*), an add-on to a PPC state.  Its accumulators are ONE device
// block of 8-byte words of their own: a header of PPS_HEADER_WORDS int64 (PPS_TAG, layout version, n, m, K, score_draws,
// score_skipped, 0 -- the two counters are kept by pps_update_kernel), PPS_CUT_WORDS int64 with the cuts, then the arrays of
// PpsLayout (the constants first), (k, j) at [k m + j], every array padded to 16 bytes.  Beside it: the replicate's bit plane
// repw[j][W] (W = ceil(n / 64) words per item), the strips' row partials (rep count | observed << 16), X and the last counted
// draw's Xr, the respondents with an observed cell, this draw's histogram, the control word ctl[0] = a non-finite g in an observed
// cell, this draw's tables [5][K][m] (Nr | R << 32, Er, Vr, Eo, Vo in units of 2^-44) and item sums [4][m] (A, B, Cq, D) --
// zero between draws: pps_update_kernel clears what it has read --, and the last counted draw's tables and statistics.
constexpr int PPS_LAYOUT_VERSION = 1;
constexpr int PPS_HEADER_WORDS = 8;
constexpr int PPS_CUT_WORDS = 16;
constexpr int64_t PPS_TAG = 0x31524353;             // "SCR1"
enum { PPS_HIST_OBS, PPS_SUMS_OBS, PPS_VAR_OBS, PPS_R_OBS, PPS_TNO, PPS_TT,                                     // the constants
       PPS_HIST_SUM, PPS_HIST_SUMSQ, PPS_HIST_GE, PPS_HIST_GT, PPS_CDF_GE, PPS_CDF_GT,                          // m + 1
       PPS_VAR_GE, PPS_VAR_GT, PPS_VAR_REP_SUM,                                                              // 1
       PPS_R_GE, PPS_R_GT, PPS_R_UNDEF, PPS_R_REP_SUM, PPS_R_REP_SUMSQ,                                        // m
       PPS_CELL_GE, PPS_CELL_GT, PPS_CELL_EMPTY, PPS_SUM_NR, PPS_SUM_R, PPS_SUM_EO, PPS_SUM_ER,                  // K x m
       PPS_CHI_GE, PPS_CHI_GT, PPS_CHI_OBS, PPS_CHI_REP,                                                      // m
       PPS_NARRAYS };
static_assert(PPS_NARRAYS == GPIRT_SCORES_NRAW, "gpirt_ppc_scores::raw");
struct PpsLayout { int64_t off[PPS_NARRAYS]; int64_t words; };      // offsets in 8-byte words from the start of the block
PpsLayout pps_layout(int64_t m, int64_t K);
struct PpsState {
    bool on = false;
    int64_t n = 0, m = 0, item0 = 0, W = 0;
    int K = 0, strips = 0;
    int cuts[GPIRT_SCORES_MAX_K] = {};
    uint64_t* block = nullptr;
    uint64_t* repw = nullptr;                                         // [m][W]
    uint32_t* xpart = nullptr;                                        // [strips][n]
    int32_t *x_obs = nullptr, *xr = nullptr;                          // [n]
    unsigned char* live = nullptr;                                    // [n]
    uint32_t* hist_cur = nullptr; int64_t* hist_last = nullptr;       // [m + 1]
    int* ctl = nullptr;
    uint64_t *tab = nullptr, *tab_last = nullptr;                     // [5][K][m]
    uint64_t *isum = nullptr, *isum_last = nullptr;                   // [4][m]
    double *r_last = nullptr, *chi_last = nullptr;                    // [m], [2][m]
    std::vector<void*> allocs;
};
int pps_check(int64_t n, int64_t m, int K, const int* cuts);       // GPIRT_E_ARG with the message
int pps_alloc(hipStream_t stream, PpsState* p, int64_t n, int64_t m, int64_t item0, const double* y, int K, const int* cuts);
void pps_free(PpsState* p);
// one draw: the replicate's bit plane and row scores, the columns' tables, then the statistics and the accumulators
int launch_pps_accumulate(hipStream_t stream, PpsState* p, const double* f, const double* mu, const double* y, uint64_t seed,
                            uint32_t iter);
int64_t pps_state_words(const PpsState* p);
int pps_get(hipStream_t stream, PpsState* p, const char* name, void* h_out, int64_t bytes);
int pps_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_scores* out);

// ppc_person.hip: the person fit (gpirt_sampler_ppc_person_*), an add-on to a PPC state.  Its accumulators are ONE device block of
// 8-byte words of their own: a header of PRS_HEADER_WORDS int64 (PRS_TAG, layout version, n, m, K, person_draws, person_skipped,
// 0 -- the two counters are kept by prs_finish_kernel), PRS_CUT_WORDS int64 with the cuts, the order as m int32, then the arrays
// of PrsLayout (the constants first), (k, i) at [k n + i], every array padded to 16 bytes.  Beside it: the order once more (the
// kernels' copy), the strips' partials per (strip, respondent) -- the packed counts ones | observed << 8 | G_s << 16, E and V in
// units of 2^-44 and the three lz sums --, the control word ctl[0] = a non-finite g in an observed cell, and the last counted
// draw's tables and statistics.
constexpr int PRS_LAYOUT_VERSION = 1;
constexpr int PRS_HEADER_WORDS = 8;
constexpr int PRS_CUT_WORDS = 16;
constexpr int64_t PRS_TAG = 0x31535250;             // "PRS1"
constexpr int PRS_STRIP = 32;                       // positions per strip at the most
constexpr int PRS_MAX_STRIPS = GPIRT_PERSON_MAX_M / PRS_STRIP + GPIRT_PERSON_MAX_K;
enum { PRS_X_OBS, PRS_G_OBS, PRS_Q_OBS, PRS_TN, PRS_TT,                                                    // the constants
       PRS_G_GE, PRS_G_GT, PRS_G_UNDEF, PRS_G_REP_SUM, PRS_GN_REP_SUM,                                        // n
       PRS_LZ_UNDEF, PRS_LZ_OBS_SUM, PRS_LZ_REP_SUM, PRS_LZ_REP_SUMSQ,                                         // n
       PRS_SUM_R, PRS_SUM_E, PRS_CELL_GE, PRS_CELL_GT,                                                       // K x n
       PRS_CHI_GE, PRS_CHI_GT, PRS_CHI_OBS, PRS_CHI_REP,                                                      // n
       PRS_NARRAYS };
static_assert(PRS_NARRAYS == GPIRT_PERSON_NRAW, "gpirt_ppc_person::raw");
struct PrsLayout { int64_t order; int64_t off[PRS_NARRAYS]; int64_t words; };      // offsets in 8-byte words from the block's start
PrsLayout prs_layout(int64_t n, int64_t m, int64_t K);
// the strips of the header: strip s holds the positions lo[s] .. lo[s] + len[s] - 1 of ONE group; group k's strips are first[k] ..
// first[k + 1] - 1
struct PrsStrips { int ns; int first[GPIRT_PERSON_MAX_K + 1]; uint16_t lo[PRS_MAX_STRIPS]; uint8_t len[PRS_MAX_STRIPS]; };
struct PrsState {
    bool on = false;
    int64_t n = 0, m = 0, item0 = 0;
    int K = 0;
    int cuts[GPIRT_PERSON_MAX_K] = {};
    PrsStrips strips{};
    uint64_t* block = nullptr;
    int32_t* order = nullptr;                                         // [m]
    uint32_t* part_c = nullptr;                                       // [strips][n]
    int64_t* part_ev = nullptr;                                       // [strips][2][n]
    double* part_lz = nullptr;                                        // [strips][3][n]
    int* ctl = nullptr;
    int64_t* xgq_last = nullptr;                                      // [3][n]: X, G, Q of the replicate
    uint32_t* tr_last = nullptr;                                      // [K][n]
    int64_t* tev_last = nullptr;                                      // [2][K][n]
    double *lz_last = nullptr, *chi_last = nullptr;                   // [3][n], [2][n]
    std::vector<void*> allocs;
};
int prs_check(int64_t n, int64_t m, int K, const int32_t* order, const int* cuts);      // GPIRT_E_ARG with the message
int prs_alloc(hipStream_t stream, PrsState* p, int64_t n, int64_t m, int64_t item0, const double* y, int K, const int32_t* order,
              const int* cuts);
void prs_free(PrsState* p);
// one draw: the strips' partials from f, mu, y and the PPC's uniforms, then one thread per respondent finishes and decides
int launch_prs_accumulate(hipStream_t stream, PrsState* p, const double* f, const double* mu, const double* y, uint64_t seed,
                          uint32_t iter);
int64_t prs_state_words(const PrsState* p);
int prs_get(hipStream_t stream, PrsState* p, const char* name, void* h_out, int64_t bytes);
int prs_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_person* out);

// ppc_resid.hip: the residual correlations (gpirt_sampler_ppc_resid_*), an add-on to a PPC state.  Its accumulators are ONE device
// block of 8-byte words of their own: a header of RSD_HEADER_WORDS int64 (n, m, layout version, resid_draws, resid_skipped, item0,
// 0, RSD_TAG -- the two counters are kept by resid_update_kernel), then the arrays of RsdLayout, pair (a, b) at [a m + b], every
// array padded to 16 bytes.  Beside it: the 0 / 1 plane O8 (built once), two sets of the nine int8 digit planes (ctl[0] names
// the set of the last counted draw; the terms kernel writes the other one), the per-draw tables S_obs, S_rep, V, r_obs, r_rep, the
// items' partial sums, the last draw's global statistics and the control words ctl[0] = set, ctl[1] = this draw holds a NaN g.
constexpr int RSD_LAYOUT_VERSION = 1;
constexpr int RSD_HEADER_WORDS = 8;
constexpr int64_t RSD_TAG = 0x31445352;               // "RSD1"
constexpr int RSD_GLOBAL_WORDS = 16;
constexpr int RSD_ITEM_PARTS = 10;                    // per item and draw: t, u, M+, M for the data and the replicate, both counts
enum { RSD_N_CO, RSD_UNDEF, RSD_RC_GE, RSD_RC_GT, RSD_RC_OBS_SUM, RSD_RC_REP_SUM, RSD_RC_REP_SUMSQ,                     // m x m
       RSD_SS_UNDEF, RSD_SS_GE, RSD_SS_GT, RSD_SS_OBS_SUM, RSD_SS_REP_SUM,                                                // m
       RSD_GLOBAL, RSD_NARRAYS };
static_assert(RSD_NARRAYS == GPIRT_RESID_NRAW, "gpirt_ppc_resid::raw");
struct RsdLayout { int64_t off[RSD_NARRAYS]; int64_t bytes[RSD_NARRAYS]; int64_t words; };      // offsets in 8-byte words
RsdLayout rsd_layout(int64_t m);
struct RsdState {
    bool on = false;
    int64_t n = 0, m = 0, item0 = 0;
    int64_t iblocks = 0, ksteps = 0, plane = 0;       // the operands: item blocks of 32, k-steps of 32 respondents, bytes of one
    uint64_t* block = nullptr;
    signed char* O8 = nullptr;
    signed char* dig = nullptr;                       // [set][d_obs, d_rep, w][digit] planes
    int64_t *s_obs = nullptr, *s_rep = nullptr, *v = nullptr;          // 2 x m x m (two halves of the depth), m x m
    double *r_obs = nullptr, *r_rep = nullptr;                         // m x m
    double* item_part = nullptr;                                       // [RSD_ITEM_PARTS][m]
    double* stats = nullptr;                                           // [8]
    int* ctl = nullptr;
    std::vector<void*> allocs;
};
int64_t rsd_state_words(int64_t m);
inline int64_t rsd_state_words(const RsdState* p) { return rsd_state_words(p->m); }
int rsd_alloc(hipStream_t stream, RsdState* p, int64_t n, int64_t m, int64_t item0, const double* y);      // refusals: with a message
void rsd_free(RsdState* p);
// one draw: the digit planes from f, mu, y and the PPC's uniforms, the int8 products, then the decisions and the reductions
int launch_rsd_accumulate(hipStream_t stream, RsdState* p, const double* f, const double* mu, const double* y, uint64_t seed,
                          uint32_t iter);
int rsd_get(hipStream_t stream, RsdState* p, const char* name, void* h_out, int64_t bytes);
int rsd_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_resid* out);

struct PpcState {
    bool on = false;
    int64_t n = 0, m = 0, item0 = 0, draws = 0, stride = 0;
    int strips = 0, rblocks = 0;
    uint64_t* block = nullptr;                        // header + accumulators
    double *rowd = nullptr, *cold = nullptr;          // a draw's partials: [strip][3][n], [row block][3][m]
    uint32_t *rowi = nullptr, *coli = nullptr;        //   ... their packed counts
    double* unit_d = nullptr; uint64_t* unit_i = nullptr;     // the items' sums of a draw ([3][m]), for the total
    PairState pairs;                                  // the pairwise item checks (ppc_pairs.hip; on == false: off)
    BinState bins;                                    // the theta-binned item fit (ppc_bins.hip; on == false: off)
    DifState dif;                                     // the group-wise item fit (ppc_dif.hip; on == false: off)
    PpsState scores;                                  // the score-based checks (ppc_scores.hip; on == false: off)
    PrsState person;                                  // the person fit (ppc_person.hip; on == false: off)
    RsdState resid;                                   // the residual correlations (ppc_resid.hip; on == false: off)
    std::vector<void*> allocs;
};
// zeroed accumulators; n_obs and obs_yes from y (device, n x m) on `stream`; the header is written
int ppc_alloc(hipStream_t stream, PpcState* s, int64_t n, int64_t m, int64_t item0, const double* y);
inline int64_t ppc_state_words(const PpcState* s) { return ppc_state_words(s->n, s->m); }
void ppc_free(PpcState* s);
// adds the replicate of one draw: f, mu, y n x m on the device; iter = the completed-iteration counter of that state;
// theta (n, on the device) is read only with the bins or the group-wise fit on
int launch_ppc_accumulate(hipStream_t stream, PpcState* s, const double* f, const double* mu, const double* y, uint64_t seed,
                          uint32_t iter, const double* theta);
int ppc_seal(hipStream_t stream, PpcState* s);      // refreshes the header (synchronises)
int ppc_fetch(hipStream_t stream, PpcState* s, std::vector<uint64_t>& host);     // seals and copies the block to the host
int ppc_field_index(const char* name);              // GPIRT_PPC_* of a field name, -1 if unknown
// finished values from a block on the host
void ppc_fill(const uint64_t* blk, int fld, bool respondents, double* out, int64_t count);
void ppc_fill_totals(const uint64_t* blk, double* out);
void ppc_fill_struct(const uint64_t* blk, gpirt_ppc* out);
int ppc_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc* out);

// ranks.hip: rank posteriors accumulated one theta draw at a time (gpirt_sampler_rank_*, gpirt_run.ranks).  The state is ONE
// device block of 8-byte words: a header of RANK_HEADER_WORDS int64 (n, counted draws, skipped draws, layout version, B, w,
// the closed pivots' count, the pairwise flag, then the closed pivots, sorted, in 32 words), uint64 rank2_sum[n] and
// rank2_sumsq[n], double pivot_share[np][n], uint32 pivot_cover[np][n], uint32 rank_hist[n][B] (each padded to a whole word)
// and, with the pairwise flag, on a 16-byte boundary uint32 lt[n][ld], ld = n rounded up to 4 (the padding stays 0).  The
// header's two draw counters are kept by the kernel itself (the device decides whether a draw is skipped).
constexpr int RANK_LAYOUT_VERSION = 1;
// the rule of quantiles.grid_index and of summary_hist_accumulate_kernel: k where theta is bit for bit -5 + 0.01 k, else -1
// (ranks.hip and ppc_bins.hip)
__device__ __forceinline__ int grid_index(double t)
{
    const double k = rint((t + 5.0) * 100.0);
    if (!(k >= 0.0 && k <= (double)(GPIRT_NGRID - 1) && -5.0 + k * 0.01 == t)) return -1;
    return (int)k;
}
constexpr int RANK_HEADER_WORDS = 8 + GPIRT_RANK_MAX_PIVOTS_CLOSED;
struct RankState {
    bool on = false, pairwise = false;
    int64_t n = 0, B = 0, w = 0, pad = 0, ld = 0;
    int np = 0;
    int64_t piv[GPIRT_RANK_MAX_PIVOTS_CLOSED] = {};
    uint64_t* block = nullptr;
    uint16_t* kidx = nullptr;                         // the last draw's grid indices, zero padded to ld (+ 8)
    uint32_t* ctl = nullptr;                          // [0]: 1 if the last draw counted
    std::vector<void*> allocs;
};
void rank_bins(int64_t n, int64_t* B, int64_t* w, int64_t* pad);      // the histogram's bins over R2 = 2 .. 2n
// the sorted closure of the pivots under q <-> n + 1 - q (n_pivots = 0: the median position(s)); returns its size (<= 32)
int rank_close_pivots(int64_t n, const int64_t* pivots, int n_pivots, int64_t* closed);
int64_t rank_state_words(const RankState* s);
int rank_alloc(hipStream_t stream, RankState* s, int64_t n, const int64_t* pivots, int n_pivots, int pairwise);
void rank_free(RankState* s);
int launch_rank_accumulate(hipStream_t stream, RankState* s, const double* theta);    // theta: n doubles on the device
int rank_get(hipStream_t stream, RankState* s, const char* name, void* h_out, int64_t bytes);
int rank_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ranks* out);

// score.hip: scoring respondents who were not in the fit, one f* draw at a time (gpirt_sampler_score_*, gpirt_run.score).  The
// state is ONE device block of 8-byte words: a header of SCORE_HEADER_WORDS int64 (n_new, m, layout version, N, 0, 0, 0, 0),
// int64 draws[n_new], nonfinite[n_new], n_obs[n_new], double lpd_acc[n_new] (starts at -inf), ll_sum[n_new] and
// post_sum[n_new][N] (k fastest).  Beside it the state owns everything the product launchers need at n_new: the packed y_new
// in both forms (Ypm for the fp64 GEMM, y8 for the int8 kernel), the terms and digit planes, and the product itself.
constexpr int SCORE_LAYOUT_VERSION = 1;
constexpr int SCORE_HEADER_WORDS = 8;
// predict.hip: the new respondents' UNSEEN answers (gpirt_sampler_score_predict_*, gpirt_run.predict), an add-on to a score
// state.  Its accumulators are ONE device block of 8-byte words of their own: a header of PRED_HEADER_WORDS int64 (n_new, m,
// layout version, N, pred_draws, pred_skipped, 0, PRED_TAG -- the two counters are kept by the epilogue kernel; the tag tells
// the block from a score block, whose header starts alike), the answered-mask of
// y_new packed 64 cells a word (cell g = r + j n_new: bit g % 64 of word g / 64), double pred_sum[m][n_new] and
// info_sum[m][n_new] (r fastest).  Beside it: the last draw's weights W (Np x n_new, k fastest, Np = 1024: the padding rows
// stay zero), the operand tables B = [P | H] (Np x 2m) and the product C = W^T B (n_new x 2m).
constexpr int PRED_LAYOUT_VERSION = 1;
constexpr int PRED_HEADER_WORDS = 8;
constexpr int64_t PRED_TAG = 0x44455250;              // "PRED"
struct PredState {
    bool on = false;
    int64_t n = 0, m = 0;
    uint64_t* block = nullptr;
    double *W = nullptr, *B = nullptr, *C = nullptr;
    int* go = nullptr;                                // 1: this draw's f* holds no NaN (written by the weights' launch)
    std::vector<void*> allocs;
};
struct ScoreState {
    bool on = false;
    int64_t n = 0, m = 0;
    TfDims tfd{};
    uint64_t* block = nullptr;
    double *Ypm = nullptr, *Gpm = nullptr, *T = nullptr, *fclean = nullptr, *logprior = nullptr;
    void *y8 = nullptr, *gq = nullptr, *aux = nullptr;
    int* flags = nullptr;                             // [0] a NaN in this draw's f*, [1 + j] in item j, [1 + m + r] r answered one
    double lse_prior = 0.0;                           // logsumexp_k(logprior)
    std::vector<uint64_t> answered;                   // host: the answered-mask of y_new, packed as a predict state block holds it
    PredState pred;                                   // predicting the unseen answers (predict.hip; on == false: off)
    std::vector<void*> allocs;
};
int64_t score_state_words(const ScoreState* s);
// refuses n_new outside 1..GPIRT_SCORE_MAX_N and values other than +1, -1, NaN before anything is allocated; h_y_new is
// n_new x m, column-major
int score_alloc(hipStream_t stream, ScoreState* s, const double* h_y_new, int64_t n_new, int64_t m);
void score_free(ScoreState* s);
// the product of (y_new, f*) as draw_theta launches it (h: its configuration and the GEMM's workspace), then the accumulation
int launch_score_accumulate(gpirt_handle_t h, hipStream_t stream, ScoreState* s, const double* fstar);   // fstar: N x m on the device
int score_get(hipStream_t stream, ScoreState* s, const char* name, void* h_out, int64_t bytes);
int score_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_score* out);
// predict.hip
int64_t pred_state_words(int64_t n_new, int64_t m);
inline int64_t pred_state_words(const ScoreState* s) { return pred_state_words(s->pred.n, s->pred.m); }     // of s->pred
int pred_alloc(hipStream_t stream, ScoreState* s);    // needs s->on; the block's header and mask are written
void pred_free(PredState* p);
// after score_accumulate_kernel has stored this draw's weights and go-flag: the operands, the contraction, the epilogue
int launch_pred_accumulate(gpirt_handle_t h, hipStream_t stream, ScoreState* s);
int pred_get(hipStream_t stream, ScoreState* s, const char* name, void* h_out, int64_t bytes);
int pred_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_score_predict* out);

// shape.hip: shape posteriors of the item response curves, one curve draw at a time (gpirt_sampler_shape_*, gpirt_run.shape;
// include/gpirt_hip.h, "IRF shape posteriors").  The state is ONE device block of 8-byte words: a header of SHAPE_HEADER_WORDS
// int64 (tag, layout version, n, m, k_half, n_tols, the four tolerances' bits, info_draws, info_skipped, 0, 0, 0, 0 -- the two
// counters are kept by the kernels), then the GPIRT_SHAPE_* arrays in order, each on a 16-byte boundary.  Beside it the state
// owns gbar (N x m, ld N: what draw_fstar's epilogue stores as mean_out), the draw's information I (as gbar), TI and the
// reliability's terms (1024 each), the grid weights w and a byte per item that tells of a skipped column.
constexpr int SHAPE_LAYOUT_VERSION = 1;
constexpr int SHAPE_HEADER_WORDS = 16;
constexpr int64_t SHAPE_TAG = 0x50414853;             // "SHAP"
struct ShapeLayout { int64_t off[GPIRT_SHAPE_NARRAYS]; int64_t words; };
ShapeLayout shape_layout(int64_t m);
// order.hip: item-pair order posteriors on top of the shape block (gpirt_sampler_shape_order_*, gpirt_run.order;
// include/gpirt_hip.h, "Item-pair IRF order posteriors").  ONE device block of 8-byte words: a header of ORDER_HEADER_WORDS
// int64 (tag, layout version, n, m, k_half, n_tols, the four tolerances' bits, draws, skipped, 0, 0, 0, 0 -- the two counters
// are kept by the finishing kernel), then the GPIRT_ORDER_* arrays in order, each on a 16-byte boundary.  Beside it the work
// arrays of the last counted draw (u: m x m, e: m, ncross: GPIRT_SHAPE_MAX_TOLS int64) and the tiles' crossing partials.
constexpr int ORDER_LAYOUT_VERSION = 1;
constexpr int ORDER_HEADER_WORDS = 16;
constexpr int64_t ORDER_TAG = 0x5244524F;             // "ORDR"
struct OrderLayout { int64_t off[GPIRT_ORDER_NARRAYS]; int64_t words; };
OrderLayout order_layout(int64_t m, int n_tols);
struct OrderState {
    bool on = false;
    uint64_t* block = nullptr;
    double *u = nullptr, *e = nullptr;
    int64_t* ncross = nullptr;
    uint32_t* tile_part = nullptr;                    // [tiles][GPIRT_SHAPE_MAX_TOLS]: unordered crossing pairs of a tile
    std::vector<void*> allocs;
};
struct ShapeState {
    bool on = false;
    int64_t n = 0, m = 0;
    int k_half = 0, n_tols = 0;
    double tols[GPIRT_SHAPE_MAX_TOLS] = {};
    uint64_t* block = nullptr;
    double *gbar = nullptr, *info = nullptr, *ti = nullptr, *term = nullptr, *w = nullptr;
    unsigned char* bad = nullptr;                     // [m]: 1 where the last draw's column held a non-finite g
    std::vector<void*> allocs;
    OrderState order;                                 // the pair block (order.on: launch_shape_accumulate also runs its kernels)
};
// refuses k_half outside 1..500, n_tols outside 1..GPIRT_SHAPE_MAX_TOLS and a negative or non-finite tolerance, with a message
int shape_check(int k_half, const double* tols, int n_tols);
// the sizes of the shape block and of its pair block (s->order), in 8-byte words
inline int64_t shape_state_words(const ShapeState* s) { return shape_layout(s->m).words; }
inline int64_t order_state_words(const ShapeState* s) { return order_layout(s->m, s->n_tols).words; }
int shape_alloc(hipStream_t stream, ShapeState* s, int64_t n, int64_t m, int k_half, const double* tols, int n_tols);
void shape_free(ShapeState* s);
int launch_shape_accumulate(hipStream_t stream, ShapeState* s, const double* gbar);   // gbar: N x m (ld N) on the device
int shape_get(hipStream_t stream, ShapeState* s, const char* name, void* h_out, int64_t bytes);
int shape_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_shape* out);
// the pair block of a shape state that is on: order_alloc refuses m outside 2..GPIRT_ORDER_MAX_M with a message
int order_alloc(hipStream_t stream, ShapeState* s);
void order_free(OrderState* o);
int launch_order_accumulate(hipStream_t stream, ShapeState* s, const double* gbar);   // after the shape's kernels: reads s->bad
int order_get(hipStream_t stream, ShapeState* s, const char* name, void* h_out, int64_t bytes);
int order_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_shape_order* out);

// sumscore.hip: posteriors of the sum score on a form of M items, one f* draw at a time (gpirt_sampler_sumscore_*,
// gpirt_run.sumscore; include/gpirt_hip.h, "Sum-score posteriors").  The state is ONE device block of 8-byte words: a header of
// SUMSCORE_HEADER_WORDS int64 (tag, layout version, m, M, N = 1001, draws, skipped, rel_draws, rel_skipped, 0 ... -- the four
// counters are kept by the kernels), then the GPIRT_SUMSCORE_* arrays in order, each on a 16-byte boundary.  Beside it the state
// owns the draw's table of (p, q) (1001 x steps pairs, steps = M rounded up to 32), T and V of the draw (1024 each), the form's
// column indices and the draw's skip word.
constexpr int SUMSCORE_LAYOUT_VERSION = 1;
constexpr int SUMSCORE_HEADER_WORDS = 16;
constexpr int64_t SUMSCORE_TAG = 0x43534d53;          // "SMSC"
struct SumscoreLayout { int64_t off[GPIRT_SUMSCORE_NARRAYS]; int64_t words; };
SumscoreLayout sumscore_layout(int64_t m, int64_t M);
struct SumscoreState {
    bool on = false;
    int64_t m = 0, M = 0, steps = 0;
    uint64_t* block = nullptr;
    double *tab = nullptr, *T = nullptr, *V = nullptr;
    int *cols = nullptr, *ctl = nullptr;
    std::vector<void*> allocs;
};
// mask: m bytes (non-zero: the item is in the form) or NULL (all m); refuses an empty form and M > GPIRT_SUMSCORE_MAX_ITEMS
int sumscore_check(int64_t m, const unsigned char* mask, int64_t* M_out);
inline int64_t sumscore_state_words(const SumscoreState* s) { return sumscore_layout(s->m, s->M).words; }
void sumscore_grid_weights(double* w);                // 1001 doubles (host)
int sumscore_alloc(hipStream_t stream, SumscoreState* s, int64_t m, const unsigned char* mask);
void sumscore_free(SumscoreState* s);
int launch_sumscore_accumulate(hipStream_t stream, SumscoreState* s, const double* fstar);   // fstar: N x m (ld N) on the device
int sumscore_get(hipStream_t stream, SumscoreState* s, const char* name, void* h_out, int64_t bytes);
int sumscore_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_sumscore* out);
// one form's recursion for other blocks (equate.hip), the very kernels of launch_sumscore_accumulate: the (p, q) table of the
// form's columns (1001 x steps pairs, steps = sumscore_steps(M); a NaN raises ctl[0]), then the rows A (`last`, 1001 x (M + 1)),
// `joint` += w_k A (NULL: not kept), T and V; then pi in sumscore_pi_kernel's order.  All do nothing once ctl[0] is set.
int64_t sumscore_steps(int64_t M);
int launch_sumscore_table(hipStream_t stream, const double* fstar, const int* cols, int M, int steps, double* tab, int* ctl);
int launch_sumscore_rows(hipStream_t stream, const double* tab, int M, int steps, const double* w, const int* ctl, double* last,
                         double* joint, double* T, double* V);
int launch_sumscore_pi(hipStream_t stream, const double* last, const double* w, int M, const int* ctl, double* last_pi,
                       double* pi_sum, double* pi_sumsq);

// equate.hip: the joint distribution of the sum scores on two disjoint forms, one f* draw at a time (gpirt_sampler_equate_*,
// gpirt_run.equate; include/gpirt_hip.h, "Two-form score equating").  The state is ONE device block of 8-byte words: a header of
// EQUATE_HEADER_WORDS int64 (tag, layout version, m, M_X, M_Y, N = 1001, draws, skipped, corr_draws, corr_skipped, eq_clamped,
// 0 ... -- the five counters are kept by the kernels), then the GPIRT_EQUATE_* arrays in order, each on a 16-byte boundary.  Beside
// it the state owns each form's (p, q) table, A_X, its weighted copy and A_Y (1024 x (M + 1) each: the rows beyond 1001 are the
// product's zero padding), T and V of both forms, the forms' column indices and the control words (skip, go).
constexpr int EQUATE_LAYOUT_VERSION = 1;
constexpr int EQUATE_HEADER_WORDS = 16;
constexpr int64_t EQUATE_TAG = 0x45545145;            // "EQTE"
struct EquateLayout { int64_t off[GPIRT_EQUATE_NARRAYS]; int64_t words; };
EquateLayout equate_layout(int64_t m, int64_t Mx, int64_t My);
struct EquateState {
    bool on = false;
    int64_t m = 0, Mx = 0, My = 0, steps_x = 0, steps_y = 0;
    uint64_t* block = nullptr;
    double *tab_x = nullptr, *tab_y = nullptr, *AX = nullptr, *WX = nullptr, *AY = nullptr, *TV = nullptr;
    int *cols_x = nullptr, *cols_y = nullptr, *ctl = nullptr;
    std::vector<void*> allocs;
};
// both masks: m bytes; refuses a missing mask, an overlap (naming the first shared column), an empty form and more than
// GPIRT_EQUATE_MAX_ITEMS items in a form
int equate_check(int64_t m, const unsigned char* mask_x, const unsigned char* mask_y, int64_t* Mx_out, int64_t* My_out);
inline int64_t equate_state_words(const EquateState* s) { return equate_layout(s->m, s->Mx, s->My).words; }
int equate_alloc(hipStream_t stream, EquateState* s, int64_t m, const unsigned char* mask_x, const unsigned char* mask_y);
void equate_free(EquateState* s);
int launch_equate_accumulate(gpirt_handle_t h, hipStream_t stream, EquateState* s, const double* fstar);   // fstar: N x m (ld N)
int equate_get(hipStream_t stream, EquateState* s, const char* name, void* h_out, int64_t bytes);
int equate_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_equate* out);

// loo.hip: PSIS-LOO without stored draws (gpirt_sampler_loo_*, gpirt_run.loo; include/gpirt_hip.h, "PSIS-LOO").  The state is
// ONE device block of 8-byte words: a header of LOO_HEADER_WORDS int64 (tag, layout version, n, m, T, M, draws, chains, 0 ...
// -- draws and chains are kept by the kernels), then the GPIRT_LOO_* arrays in order, each on a 16-byte boundary: the per-cell
// min-heaps of the K = M + 1 largest keys (slot-major), the evicted sums, p_sum, the counters and a copy of y as bytes.
constexpr int LOO_LAYOUT_VERSION = 1;
constexpr int LOO_HEADER_WORDS = 16;
constexpr int64_t LOO_TAG = 0x4F4F4C50;               // "PLOO"
struct LooLayout { int64_t off[GPIRT_LOO_NARRAYS]; int64_t words; };
LooLayout loo_layout(int64_t n, int64_t m, int64_t M);
struct LooState {
    bool on = false;
    int64_t n = 0, m = 0, T = 0, M = 0;
    uint64_t* block = nullptr;
};
// M from T and `tail` (0: the rule); refuses a tail outside 5 .. GPIRT_LOO_MAX_TAIL, M > GPIRT_LOO_MAX_TAIL and M >= T
int loo_tail_length(int64_t T, int tail, int64_t* M_out);
inline int64_t loo_state_words(const LooState* s) { return loo_layout(s->n, s->m, s->M).words; }
int loo_alloc(hipStream_t stream, LooState* s, int64_t n, int64_t m, int64_t T, int64_t M, const double* d_y);   // d_y: n x m
void loo_free(LooState* s);
int launch_loo_accumulate(hipStream_t stream, LooState* s, const double* f, const double* mu);    // f, mu: n x m on the device
// `from`'s kept keys, sums and counters into `into` (both blocks of the same n, m, M: the callers check)
int launch_loo_merge(hipStream_t stream, uint64_t* into, const uint64_t* from, int64_t n, int64_t m, int64_t M);
int loo_get(hipStream_t stream, LooState* s, const char* name, void* h_out, int64_t bytes);
int loo_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_loo* out);

// acf.hip: autocorrelation ESS without stored draws (gpirt_sampler_acf_*, gpirt_acf_combine; include/gpirt_hip.h,
// "autocorrelation ESS").  The state is ONE device block of 8-byte words: a header of ACF_HEADER_WORDS int64 (tag, layout version,
// n, m, parts, S, H, L, P, draws, 0 ... -- draws is kept by the kernels), then the GPIRT_ACF_* arrays in order, each on a 16-byte
// boundary.  `last` (the draw's P values as read), cpart and rpart (the log-likelihood pass's partials) are scratch beside it.
constexpr int ACF_LAYOUT_VERSION = 1;
constexpr int ACF_HEADER_WORDS = 16;
constexpr int64_t ACF_TAG = 0x31464341;               // "ACF1"
struct AcfLayout { int64_t off[GPIRT_ACF_NARRAYS]; int64_t words; };
AcfLayout acf_layout(int64_t P, int64_t L);
struct AcfState {
    bool on = false;
    int64_t n = 0, m = 0, S = 0, H = 0, L = 0, P = 0, draws = 0;
    int parts = 0;
    uint64_t* block = nullptr;
    double *last = nullptr, *cpart = nullptr, *rpart = nullptr;
};
// the argument check of gpirt_acf_check: L from max_lag (0: the default), P from the parts
int acf_check(int64_t n, int64_t m, int parts, int64_t planned, int64_t max_lag, int64_t* L_out, int64_t* P_out);
inline int64_t acf_state_words(const AcfState* s) { return acf_layout(s->P, s->L).words; }
int acf_alloc(hipStream_t stream, AcfState* s, int64_t n, int64_t m, int parts, int64_t planned, int64_t L);
void acf_free(AcfState* s);
// the sampler's theta (n), beta (2 x m), f, mu and y (n x m) on the device; refuses a draw beyond the planned ones
int launch_acf_accumulate(hipStream_t stream, AcfState* s, const double* theta, const double* beta, const double* f, const double* mu,
                          const double* y);
int acf_get(hipStream_t stream, AcfState* s, const char* name, void* h_out, int64_t bytes);
int acf_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_acf* out);

// groups.hip: group posteriors (gpirt_sampler_groups_*, gpirt_groups_combine; include/gpirt_hip.h, "group posteriors").  The
// state is ONE device block of 8-byte words: GRP_HEADER_WORDS int64 (tag, layout version, n, m, G, latent_draws, latent_skipped,
// votes_draws, votes_skipped, 0 ... -- the counters are kept by the kernels), GRP_SIZE_WORDS int64 of group sizes (index G: the
// included respondents), the codes as n int8, then the GPIRT_GROUPS_* arrays in order, each on a 16-byte boundary.  Everything
// else is the draw's scratch and the last counted draw's tables.
constexpr int GRP_LAYOUT_VERSION = 1;
constexpr int GRP_HEADER_WORDS = 16;
constexpr int GRP_SIZE_WORDS = 16;
constexpr int64_t GRP_TAG = 0x31505247;               // "GRP1"
struct GrpLayout { int64_t groups; int64_t off[GPIRT_GROUPS_NARRAYS]; int64_t words; };
GrpLayout grp_layout(int64_t n, int64_t m, int64_t G);
struct GroupsState {
    bool on = false;
    int64_t n = 0, m = 0;
    int G = 0, top = 0;
    int64_t sizes[GPIRT_GROUPS_MAX_G + 1] = {};
    uint64_t* block = nullptr;
    // the draw's scratch: ctl[0] a theta off the grid, ctl[1] a NaN g; hist and e are zeroed before each draw
    int* ctl = nullptr;
    uint32_t *hist = nullptr, *less = nullptr, *cnt = nullptr, *obs = nullptr;    // cnt: n_split[P], then c_g[G]
    uint64_t *e = nullptr, *loy = nullptr;
    // the last counted draw's tables
    uint32_t *hist_last = nullptr, *obs_last = nullptr;
    int64_t *lat_last = nullptr, *cnt_last = nullptr;
    double* stat_last = nullptr;
    uint64_t *e_last = nullptr, *loy_last = nullptr;
    signed char* side_last = nullptr;                 // side [G][m], then split [P][m], then contested [m]
    std::vector<void*> allocs;
};
// the argument check of gpirt_groups_check; sizes: GPIRT_GROUPS_MAX_G + 1 words or NULL
int groups_check(int64_t n, int64_t m, int G, const int32_t* groups, int top, int64_t* sizes);
int64_t groups_state_words(const GroupsState* s);
int groups_alloc(hipStream_t stream, GroupsState* s, int64_t n, int64_t m, int G, const int32_t* groups, int top);
void groups_free(GroupsState* s);
// the sampler's theta (n), f, mu and y (n x m) on the device
int launch_groups_accumulate(hipStream_t stream, GroupsState* s, const double* theta, const double* f, const double* mu,
                             const double* y);
int groups_get(hipStream_t stream, GroupsState* s, const char* name, void* h_out, int64_t bytes);
int groups_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_groups* out);

// misc
// out (cols x rows, ldo) = in^T, in is rows x cols with leading dimension ldi
int launch_transpose(hipStream_t stream, const double* in, int64_t rows, int64_t cols, int64_t ldi, double* out, int64_t ldo);
int launch_axpy_irf(hipStream_t stream, double* acc, const double* fstar, int64_t count);
int launch_advance_pos(hipStream_t stream, uint64_t* pos, uint64_t delta);
// *bad = 1 if any of the `total` responses is not +1, -1 or NaN (bad is not cleared here)
int launch_check_y(hipStream_t stream, const double* y, int64_t total, int* bad);

}  // namespace gpirt
