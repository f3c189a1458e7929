// sampler.hip -- device-resident state and the per-iteration driver of gpirtMCMC()
// (src/gpirtMCMC.cpp:5-117): init, draw_f -> draw_fstar -> draw_theta -> draw_beta -> mu, mu_star
// -> K + jitter -> chol, storage of draws, IRF averaging.  One process drives one GPU; a host that
// shards item columns over several processes calls the stage entry points and puts its collective
// (RCCL through torch.distributed) between gpirt_sampler_theta_partial and _theta_finish.
//
// Two RNG contracts:
//   GPIRT_RNG_ITEM     counter-based sub-streams: all m columns of draw_f are ONE trmm + ONE
//                      elliptical-slice launch;
//   GPIRT_RNG_RSTREAM  exact replay of R's global Mersenne-Twister stream.  The stream is generated
//                      on the host one iteration ahead (a fixed, value-independent sequence), copied
//                      to the device, and consumed through a device-resident cursor, because ess()'s
//                      consumption is data dependent (k_j rejections) and sequential over items.
#include "common.h"
#include "kernels.h"
#include "rstream.h"

#include <stdlib.h>
#include <new>
#include <mutex>
#include <type_traits>
#include <string>
#include <vector>

using namespace gpirt;

namespace {

constexpr int KSPLIT = 16;       // K ranges of the split-K product B^T [B | W] in the low-rank draw_fstar

enum { ST_DRAW_F = 0, ST_FSTAR, ST_THETA_GEMM, ST_THETA_SAMPLE, ST_BETA, ST_FACTOR, ST_COUNT };
const char* const kStageNames[ST_COUNT] = { "draw_f", "draw_fstar", "theta_gemm", "theta_sample",
                                            "draw_beta", "factor" };

}  // namespace

// The length scale as a parameter of the chain (gpirt_sampler_ell_enable / gpirt_sampler_draw_ell; include/gpirt_hip.h).  The
// index k is host state: every decision is read back once per update.  Two updates move it, each with its own width, call
// count, uniforms and counters: the whitened one (gpirt_sampler_draw_ell) and the centred one (gpirt_sampler_draw_ell_centred).
enum { ELL_WHITENED = 0, ELL_CENTRED = 1 };
struct EllUpdate {
    int w = 0;
    int64_t updates = 0, accepted = 0, out_of_range = 0, failed = 0, factorisations = 0;
    int64_t last = -1, last_proposed = 0;
    double last_u0 = 0.0, last_u1 = 0.0;
    uint32_t t = 0;                   // calls of this update so far
    double part_ms[GPIRT_ELL_PARTS] = {};
};
struct EllState {
    bool on = false;
    int P = 0, k = 0;
    std::vector<double> grid, log_prior;
    EllUpdate up[2];                  // ELL_WHITENED, ELL_CENTRED
    double *Lsave = nullptr, *fprop = nullptr, *delta = nullptr, *rec = nullptr;    // device: ldl x n, n x m, m, 8
    double *nuprop = nullptr, *dq = nullptr, *ld = nullptr, *rec_c = nullptr;       // the centred update's: n x m, m, 2, 8
    int *nonfin = nullptr, *flag = nullptr;                                         // device: m, 1
    int* h_flag = nullptr;            // pinned
    hipEvent_t ev = nullptr;          // the sampler's own stream has finished whatever still reads L
    // with gpirt_sampler_enable_timing on: the device time of the last update's parts ("times" of gpirt_sampler_ell_get) --
    // the copies (f -> nu's buffer, the factor buffer saved), the solve, the build and factorisation, the product, the three
    // kernels, the copy back after a rejection (the centred update: the copies, the first solve, the build and factorisation,
    // the second solve, the quad, logdet and decide kernels, the copy back)
    hipEvent_t tev[GPIRT_ELL_PARTS + 2] = {};
};

// Per-item GP amplitudes (gpirt_sampler_amp_set / gpirt_sampler_amp_enable; include/gpirt_hip.h, amp.hip).  mode 0: off (draw_f
// and draw_fstar are the unit model's), 1: fixed, 2: on the grid.  The indices, widths, counters and records live on the device:
// an update is one launch and no host read.
struct AmpState {
    int mode = 0;
    int P = 0;
    int64_t planned = 0, recorded = 0;
    uint32_t t = 0;                   // draw_amp calls so far (it survives enabling again: no pair of uniforms is replayed)
    std::vector<double> grid, log_prior;
    double *amp = nullptr, *d_grid = nullptr, *d_log_prior = nullptr, *rec = nullptr;      // device: m, P, P, 5 x m
    int *idx = nullptr, *width = nullptr;                                                  // device: m, m
    long long* counts = nullptr;                                                           // device: 4 x m
    uint32_t* hist = nullptr;                                                              // device: P x m
    int32_t* draws = nullptr;                                                              // device: planned x m
    // with gpirt_sampler_enable_timing on: the device time of the last update's one launch ("time" of gpirt_sampler_amp_get)
    hipEvent_t tev[2] = {};
    double last_ms = 0.0;
    // The centred update (gpirt_sampler_draw_amp_centred; amp_centred.hip).  Its buffers are one allocation made by its first
    // call after an enable: a sampler that never calls it has none.  F, its live mask and r are the sampler's SmoothF (below),
    // shared with the centred beta update.
    uint32_t ct = 0;                  // draw_amp_centred calls so far (it survives enabling again, as t)
    double* cbuf = nullptr;
    AmpCentredArgs ca{};              // the device pointers into cbuf, the tables
    hipEvent_t ctev[2] = {};
    double clast_ms = 0.0;
};

// The population prior for theta (gpirt_sampler_pop_set / gpirt_sampler_pop_enable; include/gpirt_hip.h, pop.hip).  mode 0: off
// (draw_theta adds N(0, 1) in the kernel it always ran), 1: a fixed table, 2: the groups' means and sds on two grids.  The
// indices, statistics, counters and rows live on the device: an update is two launches and no host read.
struct PopState {
    int mode = 0;
    int G = 0, P_mu = 0, P_sd = 0;
    int64_t planned = 0, recorded = 0;
    uint32_t t = 0;                   // draw_pop calls so far (it survives enabling again: no pair of uniforms is replayed)
    double mu_hi = 0.0, sd_lo = 0.0, sd_hi = 0.0;
    std::vector<double> mu, sd, lse, hyper_mu, hyper_sd;
    int32_t* codes = nullptr;                                                              // device: n
    double *log_prior = nullptr, *d_mu = nullptr, *d_sd = nullptr, *d_lse = nullptr, *d_hyper_mu = nullptr, *d_hyper_sd = nullptr,
           *lp_mu = nullptr, *lp_sd = nullptr;                    // device: G x N, P_mu, P_sd, P_mu x P_sd, P_mu, P_sd, G x P_mu, G x P_sd
    int* idx = nullptr;                                                                    // device: G x 2
    long long *stats = nullptr, *counts = nullptr;                                         // device: 4 x G each
    uint32_t *hist_mu = nullptr, *hist_sd = nullptr;                                       // device: P_mu x G, P_sd x G
    int32_t* draws = nullptr;                                                              // device: planned x G x 2
    hipEvent_t tev[2] = {};           // with gpirt_sampler_enable_timing on: around the two launches of the last draw_pop
    double last_ms = 0.0;
};

// Ordinal responses (gpirt_sampler_ordinal_enable; include/gpirt_hip.h, ordinal.hip).  on == false: the binary chain, launch for
// launch what it was.  The indices, thresholds, counters and records live on the device: an update is one launch and no host read.
struct OrdState {
    bool on = false;
    int C = 0, P = 0, W = 16;
    int lp_W = 16;                    // the width the last update wrote "lp" with (enable: W), the stride gpirt_sampler_ordinal_get reads it by
    double hi = 0.0;
    int64_t planned = 0, recorded = 0, irf_draws = 0;
    uint32_t t = 0;                   // draw_thresholds calls so far (it survives enabling again: no pair of uniforms is replayed)
    std::vector<double> grid, log_prior;
    int8_t* cat = nullptr;                                                                 // device: n x m
    double *d_grid = nullptr, *d_log_prior = nullptr, *thr = nullptr, *lp = nullptr, *cum = nullptr, *Y = nullptr, *G = nullptr;
                                      // device: P, P, m x (C - 1), m x (C - 1) x GPIRT_ORD_MAX_WIDTH, m x (C - 1) x N, n x C m, Np x C m
    int *idx = nullptr, *window = nullptr;                                                 // device: m x (C - 1) each
    long long *counts = nullptr, *stat = nullptr;                                          // device: m x C; pinned, failed, updates
    uint32_t* hist = nullptr;                                                              // device: m x (C - 1) x P
    int32_t* draws = nullptr;                                                              // device: planned x m x (C - 1)
    hipEvent_t tev[2] = {};
    double last_ms = 0.0;
    OfitState fit;                    // the fit output (gpirt_sampler_ordinal_fit_enable, ordinal_fit.hip; on == false: off)
    OscoreState score;                // scoring new respondents (gpirt_sampler_ordinal_score_enable, ordinal_score.hip; on == false: off)
};

// F of the rank-64 smooth part, Kcc = F F^T (fstar_free_factor) with its DEAD columns (squared norm <= 1e-13) zeroed on the host,
// `live` their mask and r the live count, on the device for the kernel with length scale `ell`.  One per sampler, shared by the
// centred amplitude update and the centred beta update; built by the first call of either and rebuilt only when a sampled length
// scale's index moved (smooth_factor).
struct SmoothF {
    double* F = nullptr;              // device, 64 x 64 (in `allocs`)
    uint64_t live = 0;
    int r = 0;
    bool have = false;
    double ell = 0.0;
};

// The centred beta update (gpirt_sampler_draw_beta_centred; include/gpirt_hip.h, beta_centred.hip).  Its buffers are one
// allocation made by its first call: a sampler that never calls it has none.
struct BetaCentredState {
    uint32_t t = 0;                   // draw_beta_centred calls so far
    double* buf = nullptr;            // device (in `allocs`)
    BetaCentredArgs a{};              // the device pointers into buf
    int prior_ok = -1;                // the prior sds are finite and > 0 (host_tmp): -1 not looked at yet
    hipEvent_t tev[4] = {};           // with timing on: around the call, around its per-item kernel
    double last_ms = 0.0, item_ms = 0.0;
};

// The collapsed scale and shift move (gpirt_sampler_scale_enable, gpirt_sampler_draw_scale; include/gpirt_hip.h, scale.hip).
// Its buffers are allocated by gpirt_sampler_scale_enable through `allocs`: a sampler that never enables it has none.
struct ScaleState {
    bool on = false;
    uint32_t t[2] = {};               // draw_scale calls so far, per kind
    double width[2] = {};             // the proposal's sd: of eps (scale), of delta (shift)
    ScaleArgs a{};                    // the device pointers of the proposal's buffers, the vectors, the record, the counters
    int last_kind = -1;
    int prior_ok = -1;                // the prior sds are finite and > 0 (host_tmp): -1 not looked at yet
    hipEvent_t tev[7] = {};           // with timing on: the call's start, behind the curve, behind the product, logz, decide, commits
    double last_ms[2] = {};
    double times[6] = {};             // of the last timed call: whole, curve, product, logz, decide, commits
};

// The consistent step's carry and the prior check (gpirt_sampler_carry_f, gpirt_sampler_prior_quad; include/gpirt_hip.h,
// carry.hip).  Both buffers are allocated by the first call that needs them: a sampler that never calls either has neither.
struct CarryState {
    int64_t calls = 0;
    unsigned long long* counters = nullptr;   // device, 6: off_grid, nonfinite of the sampler's life, of the even calls, of the odd calls
    double* quad = nullptr;                   // device, m: the prior check's q_j
    hipEvent_t tev[2] = {};                   // with gpirt_sampler_enable_timing on: around the carry's launch
    double last_ms = 0.0;
};

struct gpirt_sampler_s {
    gpirt_handle_t h = nullptr;
    int64_t n = 0, m = 0, N = GPIRT_NGRID;
    gpirt_options opt{};
    KernelSpec kern;                  // the handle's covariance kernel when the sampler was created (gpirt_kernel_set is
                                      // refused while the sampler lives, so the two cannot part)
    RStream* rs = nullptr;            // borrowed (R-stream mode)
    // device state
    double *y = nullptr, *Ypm = nullptr, *theta = nullptr, *theta_new = nullptr, *f = nullptr,
           *Z = nullptr, *NU = nullptr, *beta = nullptr, *mu = nullptr, *mu_star = nullptr,
           *fstar = nullptr, *L = nullptr, *tstar = nullptr, *kstar = nullptr, *rhs = nullptr,
           *mean = nullptr, *s = nullptr, *Gpm = nullptr, *logpost = nullptr, *irf_sum = nullptr,
           *pm = nullptr, *ps = nullptr, *step = nullptr;
    // low-rank K* (opt.kstar_rank = r > 0): Chebyshev nodes, interpolation matrix V (N x r), split-K parts
    int kr = 0;
    double *knodes = nullptr, *kV = nullptr, *kparts = nullptr, *kP = nullptr;
    // L is stored (n + ext) x n with leading dimension ldl.  ext = kr when the low-rank K* is on and n % 64 == 0: the
    // extra rows enter the factorisation holding K(c, theta) (r x n) and leave it holding (L^-1 K(theta, c))^T -- the
    // forward solve of draw_fstar comes out of the bordered factorisation (potrf.hip) for ~1 % more work.
    // Without the low-rank K* (ext_grid): the rows are K(theta*, theta) for the 1001 grid points (padded to 1024 zero
    // rows) and come out as (L^-1 k*)^T -- the 1001-column forward solve of src/draw-fstar.cpp:19 rides through the
    // factorisation the same way.  rows_valid: the rows belong to the current (theta, L); cleared when either is set
    // from outside, rebuilt by an explicit solve on demand (rebuild_rows).
    // Every bordered layout also carries the 64 NODE rows K(c_64, theta) -> K(c_64, theta) L^-T that draw_f's structured product
    // reads (nu_lr.hip): with kr == 64 they ARE draw_fstar's rows (carried once, shared); with another rank r the node rows
    // come first and the r rank rows behind them (ext = 64 + r); with the grid rows they sit behind the 1024 (ext = 1088);
    // a sampler with neither (kr == 0, n < 1024) carries them alone (ext = 64).  node_off / rank_off: first row of each
    // below row n (node_off < 0: none).
    // Under GPIRT_BORDERED=2 draw_fstar's rows are not carried (it solves for them: fstar_rows == false, also with kr == 64),
    // the node rows still are (ext = 64): draw_f's product, and with it f, does not depend on that switch.
    int64_t ext = 0, ldl = 0, node_off = -1, rank_off = 0;
    bool ext_grid = false, rows_valid = false, fstar_rows = false;
    // draw_f's structured product: nodes and weights, the basis at theta (n x 64), the parts' records.  nu_kern_ok: the handle's
    // kernel passes the rank-64 certificate (under a length-scale update: at the grid's smallest ell); theta_ok: every theta
    // is finite and inside [-5, 5] -- a HOST-side fact, checked on the host arrays that arrive (create, set) and true by
    // construction after a draw_theta; theta_alone: theta was set from outside and no factor has followed it, so L need
    // not be the factor of K(theta, theta); nu_lr_draws: draws that ran the structured product so far
    double *nu_nodes = nullptr, *nu_wts = nullptr, *nuV = nullptr, *nuT = nullptr;
    bool nu_kern_ok = false, theta_ok = false, theta_alone = false;
    int64_t nu_lr_draws = 0;
    // Work that needs only L (not this iteration's f) runs on a stream of the sampler's own, beside draw_f's elliptical
    // slice kernel: the part of the low-rank draw_fstar that depends on the factor alone (C = L^-T B, G = B^T B).
    // haux is the main handle's side handle (h->aux, shared by the samplers of that handle, not owned) on that stream (its own trsm / split-K workspaces: several
    // samplers may share `h`).  prep_valid: C and G belong to the current L; *_pending: the main stream has not yet
    // waited for the event.
    gpirt_handle_t haux = nullptr;
    hipEvent_t ev_trmm = nullptr, ev_prep = nullptr;
    bool prep_valid = false, prep_pending = false;
    // C from theta alone (fstar_free.hip): C = V M with V = nuV and M from V^T V and F, K(c, c) = F F^T -- no solve through L.
    // ffF: F on the device (64 x 64) for the kernel with length scale ff_ell (ff_have; rebuilt wherever the host replaces
    // `kern`); ffW: V^T V and M; prep_free: the C in place (prep_valid) came from that chain, which READS nuV -- whoever
    // rewrites nuV while it is pending joins it first; fstar_free_draws: draw_fstar calls that used such a C so far
    double *ffF = nullptr, *ffW = nullptr;
    bool ff_have = false, prep_free = false;
    double ff_ell = 0.0;
    int64_t fstar_free_draws = 0;
    // The structured factor (factor_lr.hip; opt.factor_structured): where the sampler's next readers are draw_f's structured
    // product and the rank-64 draw_fstar with C from theta alone, only L's diagonal parts and the node rows are built, from
    // theta.  L_structured: that is what `L` holds -- the triangle below the parts is NOT the factor's; theta_L: the theta it
    // belongs to (ensure_dense_factor builds the dense factor from it for whoever reads more of L); flrG / flrXh / flrX: the
    // workspaces of launch_factor_lr; ev_flr: recorded where the structured factor starts (the side work waits for it)
    double *theta_L = nullptr, *flrG = nullptr, *flrXh = nullptr, *flrX = nullptr, *flrD = nullptr;
    bool L_structured = false;
    int L_part_width = 0;                 // the width of the diagonal parts a structured L holds (factor_width(): 0 for a dense L)
    hipEvent_t ev_flr = nullptr;
    int64_t factor_lr_count = 0, dense_factor_count = 0;      // structured factors / dense factorisations this sampler enqueued
    // the N(0,1) draws of the NEXT draw_f depend on (seed, iteration, item, index) only: filled on the sampler's own stream
    // while the last outer panel is factored; z_filled_iter = the iteration they belong to (0: none), ev_zfill fires when done
    uint32_t z_filled_iter = 0;
    hipEvent_t ev_zfill = nullptr;
    // draw_beta (+ mu, mu_star) needs theta and f but nothing of the factorisation that follows it: it is held back
    // (beta_deferred) until the factorisation has been enqueued and then runs on the sampler's own stream in the same idle
    // phase; beta_pending: the main stream has not yet waited for it (ev_beta).  Anything that reads or writes beta, mu,
    // mu_star, theta or f first flushes / joins it (beta_sync).
    bool beta_deferred = false, beta_pending = false;
    hipEvent_t ev_beta = nullptr;
    // respondent-block form of draw_theta for item-sharded runs (gpirt_sampler_set_theta_block): this rank's
    // block of respondents with ALL items
    int64_t blk_i0 = 0, blk_n = 0, blk_m = 0;
    double *Ypm_blk = nullptr, *Gpm_full = nullptr, *logpost_blk = nullptr, *fstar_full = nullptr, *theta_stage = nullptr;
    // the log-posterior product in fixed point (theta_fixed.hip): byte indicators (built once), digit planes of G, row scales
    TfDims tfd{}, tfd_blk{};
    double *tf_y8 = nullptr, *tf_gq = nullptr, *tf_aux = nullptr, *tf_y8_blk = nullptr, *tf_gq_blk = nullptr, *tf_aux_blk = nullptr;
    int *ess_k = nullptr, *flags = nullptr;    // flags[0] = err, flags[1] = degenerate theta count
    int *fstar_off = nullptr;                  // R-stream replay: consumption offsets of draw_fstar
    int *h_flags = nullptr;                    // pinned
    // R-stream replay
    double* U = nullptr; double* hU = nullptr; uint64_t U_cap = 0;
    uint64_t* pos = nullptr; uint64_t* h_pos = nullptr; uint64_t* beta_off = nullptr;
    uint64_t beta_total = 0;
    RStream saved{};
    bool stream_open = false;
    // The host generator runs AHEAD of the chain (stream_begin / stream_end): while the device works off an iteration the
    // host tops up a FIFO of fresh uniforms (hA, uploaded to S on cs), and the next window is put together on the device
    // from the unconsumed tail of this one + the FIFO's head -- no 65 ms rewind and no 73 ms generation between two
    // iterations (they were half of the default contract's 286 ms at 8192 x 1024).  ahead_gen / ahead_used: draws generated /
    // consumed since the generator was attached; snaps: its state every 2^16 draws, so that the state at the consumed
    // position -- what the caller's RStream must hold whenever anybody looks (rstream_sync) -- is one copy + a short skip.
    gpirt_rstream_s* rs_obj = nullptr;
    bool ahead_attached = false;
    uint64_t ahead_gen = 0, ahead_used = 0, a_len = 0;
    std::vector<std::pair<uint64_t, RStream>> snaps;
    uint32_t *hA = nullptr, *Sraw = nullptr;      // the FIFO as the host produces it: raw Mersenne-Twister words (pinned / device)
    double *S = nullptr, *U2 = nullptr;
    hipStream_t cs = nullptr;
    hipEvent_t ev_up = nullptr, ev_asm = nullptr;
    // draw_f of the replay, three items per pass over L (rng_ess.hip): Nrm = the normal that starts at every position of the
    // window, rs_part = the parts of a pass's 48 candidate products, next_item = the first item no pass has resolved yet
    bool spec_ok = false;
    uint64_t *posv = nullptr, *anchor = nullptr, *h_next = nullptr;
    unsigned long long* rs_flags = nullptr; double* rs_partial = nullptr; uint64_t rs_tag = 0;
    double* Lt = nullptr;             // L in the candidate products' tile order (rebuilt at the start of every draw_f)
    double *Nrm = nullptr, *rs_part = nullptr;
    uint32_t* rs_units = nullptr; int rs_nunits = 0, rs_nfull = 0;
    uint32_t* rs_unitsP = nullptr; int rs_nunitsP = 0, rs_nfullP = 0;     // the predictor's own units (RS3P_KC columns each)
    long long* rs_trace = nullptr;    // debug stamps of one pass (gpirt_debug_rs_trace)
    // the predicted replay (rs_predict.hip): single-precision tiles of L and parts, the predictor's own anchor / cursor / error
    // word, what the verification leaves per item, ctl = [first item not committed, mispredictions, predictor stalls, passes]
    float *Lt32 = nullptr, *rs_part32 = nullptr;
    uint64_t *anchorP = nullptr, *rs_ctl = nullptr, *rs_posP = nullptr;
    double *rs_dec_part = nullptr, *rs_dec_rec = nullptr; unsigned* rs_dec_ticket = nullptr;
    double rs_pass_rate = 0.0; uint64_t rs_pass_seen = 0;    // real predictor passes per item of the last round / the counter's last reading
    int *rs_kpred = nullptr, *rs_kv = nullptr, *rs_used = nullptr, *rs_ierr = nullptr, *rs_errP = nullptr;
    // the predictor's structured form (rs_lr.hip): nodes / weights / K(c, c), the basis at theta in both precisions, prefix Grams,
    // C as tiles, the parts' records, the units; lr_on: in use; lr_strikes: draws in a row whose structured rounds mispredicted
    double *lr_nodes = nullptr, *lr_wts = nullptr, *lr_M = nullptr, *lr_V64 = nullptr, *lr_Gb = nullptr;
    float *lr_V32t = nullptr, *lr_Ct32 = nullptr, *lr_Y = nullptr;
    int* lr_bad = nullptr; uint32_t* lr_units = nullptr; int lr_nunits = 0;
    bool lr_on = false; int lr_strikes = 0; uint64_t rs_mis_seen = 0;
    // bookkeeping
    int iter = 0;                     // completed iterations
    bool initialised = false;
    bool sticky_info = false;         // gpirt_mcmc: potrf info is not cleared between iterations
    bool factor_fresh = false;        // the L enqueued last has not been read by any stage yet (recover_factor)
    bool counted = false;             // registered in h->live_samplers (a fully created sampler)
    bool in_init = false;             // do_factor runs for gpirt_sampler_init (no prefill of Z: init fills it itself)
    bool timing = false;
    hipEvent_t ev[ST_COUNT + 1] = {};
    double stage_ms[ST_COUNT] = {};
    std::vector<void*> allocs;
    std::vector<double> host_tmp;
    SummaryState sum;                 // posterior summaries (gpirt_sampler_summary_enable; parts == 0: off)
    PpcState ppc;                     // posterior predictive checks (gpirt_sampler_ppc_enable; on == false: off)
    RankState rank;                   // rank posteriors (gpirt_sampler_rank_enable; on == false: off)
    ShapeState shape;                 // IRF shape posteriors (gpirt_sampler_shape_enable; on: draw_fstar also stores gbar)
    ScoreState score;                 // scoring new respondents (gpirt_sampler_score_enable; on == false: off)
    SumscoreState sumscore;           // sum-score posteriors (gpirt_sampler_sumscore_enable; on == false: off)
    EquateState equate;               // two-form score equating (gpirt_sampler_equate_enable; on == false: off)
    LooState loo;                     // PSIS-LOO (gpirt_sampler_loo_enable; on == false: off)
    AcfState acf;                     // autocorrelation ESS (gpirt_sampler_acf_enable; on == false: off)
    GroupsState groups;               // group posteriors (gpirt_sampler_groups_enable; on == false: off)
    EllState ell;                     // the length scale in the chain (gpirt_sampler_ell_enable; on == false: off)
    AmpState amp;                     // per-item GP amplitudes (gpirt_sampler_amp_set, gpirt_sampler_amp_enable; mode == 0: off)
    OrdState ord;                     // ordinal responses (gpirt_sampler_ordinal_enable; on == false: the binary chain)
    PopState pop;                     // the population prior for theta (gpirt_sampler_pop_set, gpirt_sampler_pop_enable; mode == 0: off)
    CarryState carry;               // the consistent step's carry and the prior check (gpirt_sampler_carry_f, gpirt_sampler_prior_quad)
    SmoothF sf;                       // F of the rank-64 smooth part with its dead columns zeroed (the two centred updates below)
    BetaCentredState bc;              // the centred beta update (gpirt_sampler_draw_beta_centred)
    ScaleState sc;                    // the collapsed scale and shift move (gpirt_sampler_scale_enable; on == false: off)
    // logpost (N x n) is theta_partial's product for the fstar, beta and population prior in place: set by theta_partial, kept
    // by gpirt_sampler_draw_scale, cleared by every writer of fstar, beta, f, theta or the population prior's table
    bool lp_current = false;
    // mu_linear: mu was last written as b0 + theta b1 (one multiply, one add) from the theta and beta that are still in place, so
    // the slice kernel may form it again instead of reading it (ess_lin.hip; DESIGN.md section 51 lists who sets and who clears
    // it).  ess_ypk: y as that kernel reads it (launch_ess_pack), built at creation and again behind a caller's write to y;
    // ess_pack_draws: draws that took that kernel so far
    bool mu_linear = false;
    uint32_t* ess_ypk = nullptr;
    bool ess_ypk_valid = false;
    int64_t ess_pack_draws = 0;
};

namespace {

// numbers = false: a double-typed buffer that holds integer words (the fixed-point indicators and counters of theta_fixed.hip),
// never poisoned (poison_fresh)
template <typename T>
int dalloc(gpirt_sampler_s* s, T** p, size_t count, bool numbers = true)
{
    void* q = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return GPIRT_E_ALLOC;
    }
    s->allocs.push_back(q);
    *p = reinterpret_cast<T*>(q);
    if (std::is_same<T, double>::value || std::is_same<T, float>::value) {
        if (numbers && poison_fresh(s->h, q, bytes, s->h->stream) != hipSuccess) {
            set_error("hipMemsetAsync(%zu bytes) failed", bytes);
            return GPIRT_E_HIP;
        }
    }
    return 0;
}

inline bool stream_mode(const gpirt_sampler_s* s) { return s->opt.rng_kind == GPIRT_RNG_RSTREAM; }

int report_degenerate_theta(gpirt_sampler_s* s, int count);

// ---- R-stream window ---------------------------------------------------------------------------
// draws [ahead_gen, ahead_gen + count) of the attached generator into dst, a state snapshot every 2^16 draws.  The host
// only runs the Mersenne-Twister recurrence (0.85 ns per word on one core: 16 ms for the 18.8 M draws of an iteration at
// 8192 x 1024); tempering and the conversion to unif_rand()'s double happen on the device (rs_unpack_kernel) -- done on the
// host they were three quarters of the 70 ms this took, more than the device needs for the whole iteration.
void ahead_generate(gpirt_sampler_s* s, uint32_t* dst, uint64_t count)
{
    constexpr uint64_t EVERY = 1ull << 16;
    while (count) {
        const uint64_t c = count < EVERY ? count : EVERY;
        s->snaps.emplace_back(s->ahead_gen, *s->rs);
        s->rs->fill_raw(dst, c);
        s->ahead_gen += c; dst += c; count -= c;
    }
}

// puts the caller's generator back to exactly the consumed position and forgets everything generated ahead
// (gone: the RStream object itself is being destroyed -- the sampler must not touch it again)
void ahead_resolve(void* owner, bool gone)
{
    gpirt_sampler_s* s = static_cast<gpirt_sampler_s*>(owner);
    if (s->ahead_attached) {
        if (s->ev_up) hipEventSynchronize(s->ev_up);          // (an upload may still be reading hA)
        size_t best = 0;
        for (size_t q = 0; q < s->snaps.size(); ++q) if (s->snaps[q].first <= s->ahead_used) best = q;
        *s->rs = s->snaps[best].second;
        s->rs->skip(s->ahead_used - s->snaps[best].first);
    }
    s->ahead_attached = false;
    s->snaps.clear();
    s->ahead_gen = s->ahead_used = s->a_len = 0;
    if (s->rs_obj) { s->rs_obj->owner = nullptr; s->rs_obj->resolve = nullptr; }
    if (gone) { s->rs_obj = nullptr; s->rs = nullptr; }
}

// gpirt_rstream_destroy: the stream object this sampler was created on is being freed
void rstream_forget(void* sampler)
{
    gpirt_sampler_s* s = static_cast<gpirt_sampler_s*>(sampler);
    s->rs_obj = nullptr; s->rs = nullptr;
}

int stream_begin(gpirt_sampler_s* s, uint64_t count)
{
    if (count > s->U_cap) { set_error("R-stream window %llu exceeds capacity %llu", (unsigned long long)count, (unsigned long long)s->U_cap); return GPIRT_E_RNG; }
    if (!s->rs) { set_error("the R stream of this sampler has been destroyed"); return GPIRT_E_ARG; }
    hipStream_t st = s->h->stream;
    if (!s->ahead_attached) {
        // the first window after creation (or after somebody looked at the generator): generate, upload
        if (s->rs_obj->owner && s->rs_obj->owner != s) rstream_sync(s->rs_obj);     // another sampler runs ahead on this stream
        s->snaps.clear();
        s->ahead_gen = s->ahead_used = s->a_len = 0;
        GP_HIP(hipEventSynchronize(s->ev_up));                // (an earlier upload may still be reading hA)
        ahead_generate(s, s->hA, count);
        GP_HIP(hipStreamWaitEvent(st, s->ev_up, 0));          // (... or unpacking Sraw on the copy stream)
        GP_HIP(hipMemcpyAsync(s->Sraw, s->hA, count * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        GP_TRY(launch_rs_unpack(st, s->Sraw, (int64_t)count, s->U));
        GP_HIP(hipEventRecord(s->ev_asm, st));
        GP_HIP(hipEventRecord(s->ev_up, st));                 // (hA and Sraw are free again when this has run)
        s->ahead_attached = true;
        s->rs_obj->owner = s; s->rs_obj->resolve = ahead_resolve;
    }                                                         // (otherwise stream_end has already put the window together)
    GP_HIP(hipMemsetAsync(s->pos, 0, sizeof(uint64_t), st));
    s->stream_open = true;
    return 0;
}

// Fills the FIFO of fresh uniforms up to one window and uploads the new part on the copy stream: host work for the time the
// device is busy.  Called with the items of draw_f enqueued (80 % of an iteration's device time is still ahead), and again
// from stream_end for whoever did not come through there.
int ahead_topup(gpirt_sampler_s* s, uint64_t count)
{
    if (!s->ahead_attached || s->a_len >= count) return 0;
    const uint64_t need = count - s->a_len;
    GP_HIP(hipEventSynchronize(s->ev_up));                    // the previous upload has left hA
    ahead_generate(s, s->hA + s->a_len, need);
    GP_HIP(hipStreamWaitEvent(s->cs, s->ev_asm, 0));          // the last assembly has finished moving S's leftover
    GP_HIP(hipMemcpyAsync(s->Sraw + s->a_len, s->hA + s->a_len, need * sizeof(uint32_t), hipMemcpyHostToDevice, s->cs));
    GP_TRY(launch_rs_unpack(s->cs, s->Sraw + s->a_len, (int64_t)need, s->S + s->a_len));
    GP_HIP(hipEventRecord(s->ev_up, s->cs));
    s->a_len = count;
    return 0;
}

// reads back the cursor, builds the next window on the device
int stream_end(gpirt_sampler_s* s, uint64_t count)
{
    hipStream_t st = s->h->stream;
    GP_HIP(hipMemcpyAsync(s->h_pos, s->pos, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    GP_HIP(hipMemcpyAsync(s->h_flags, s->flags, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    GP_TRY(ahead_topup(s, count));                            // (normally done already, beside draw_f)
    GP_HIP(hipStreamSynchronize(st));
    s->stream_open = false;
    const uint64_t used = *s->h_pos <= count ? *s->h_pos : count;
    s->ahead_used += used;
    if (s->h_flags[0] != 0 || s->h_flags[1] != 0) ahead_resolve(s, false);       // the chain stops here: hand the generator back
    if (s->h_flags[0] != 0) {
        set_error(s->h_flags[0] == GPIRT_E_RNG ? "R-stream replay ran out of pre-generated uniforms"
                  : s->h_flags[0] == GPIRT_E_HIP ? "slice sampler: the work-groups of one item did not meet within the spin bound (device hang guard)"
                  : "sampler state is not finite (elliptical slice sampler met a NaN log-likelihood or did not terminate)");
        return s->h_flags[0];
    }
    // draw_theta as written underflows to 0/0 for some respondents (quirk Q5: the reference then reads theta_star[N] out
    // of bounds): reported at the iteration it happens in, not as whatever the NaN theta breaks next
    if (s->h_flags[1] != 0) return report_degenerate_theta(s, s->h_flags[1]);
    // next window = this one's unconsumed tail + the FIFO's first `used` draws; the FIFO's leftover moves to its front
    // (through the old window buffer: the ranges overlap)
    const uint64_t tail = count - used, rem = s->a_len - used;
    GP_HIP(hipStreamWaitEvent(st, s->ev_up, 0));
    if (tail) GP_HIP(hipMemcpyAsync(s->U2, s->U + used, tail * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (used) GP_HIP(hipMemcpyAsync(s->U2 + tail, s->S, used * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (rem) {
        GP_HIP(hipMemcpyAsync(s->U, s->S + used, rem * sizeof(double), hipMemcpyDeviceToDevice, st));
        GP_HIP(hipMemcpyAsync(s->S, s->U, rem * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    GP_HIP(hipEventRecord(s->ev_asm, st));
    std::swap(s->U, s->U2);
    GP_HIP(hipEventSynchronize(s->ev_up));
    s->a_len = rem;                                           // (the host copy of the FIFO is never read again: nothing to move)
    // snapshots below the consumed position are never needed again (all but the last of them)
    size_t keep = 0;
    for (size_t q = 0; q < s->snaps.size(); ++q) if (s->snaps[q].first <= s->ahead_used) keep = q;
    if (keep) s->snaps.erase(s->snaps.begin(), s->snaps.begin() + (std::ptrdiff_t)keep);
    return 0;
}

uint64_t stream_window(const gpirt_sampler_s* s)
{
    const uint64_t n = (uint64_t)s->n, m = (uint64_t)s->m, N = (uint64_t)s->N;
    return m * (2 * n + 2) + 512 * m + 4096 + 2 * N * m + n + s->beta_total;
}

// nu = L z for ONE right-hand side -- the R-stream replay's rmvnorm (src/mvnormal.h:10).  Under R's stream item j's
// normals start where item j - 1's data-dependent slice loop stopped consuming (src/draw-f.cpp:40-58), so the m products
// of an iteration are DEPENDENT (no batching, and nothing of item j can start beside item j - 1's loop): what is left is
// to make one product cost what its bytes cost.  It is memory-bound -- the lower triangle, n^2 / 2 doubles, read once --
// so the shape is chosen for bytes in flight: 32 rows per work-group (lane = row: 256-byte row segments per column), 8
// column phases per work-group, and TRMV_SPLIT column ranges of every row block side by side (1024 work-groups at n = 8192,
// four per CU), their parts added in a fixed order.  Round 3's thread-per-row kernel (one 64-thread work-group per 64
// rows, each thread walking its whole row) kept 8192 loads in flight on the chip.
// (The strict upper triangle of L holds zeros -- gpirt_sampler_create -- so the diagonal 32 x 32 block is read whole.)
constexpr int TRMV_ROWS = 32, TRMV_SPLIT = 4;

__global__ __launch_bounds__(256) void trmv_lower_part_kernel(const double* __restrict__ L, int64_t n, int64_t ldl,
                                                              const double* __restrict__ z, double* __restrict__ part)
{
    __shared__ double sred[8][TRMV_ROWS];
    const int r = threadIdx.x & 31, ph = threadIdx.x >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * TRMV_ROWS, row = row0 + r;
    const int64_t kall = (row0 + TRMV_ROWS < n) ? row0 + TRMV_ROWS : n;        // columns that can be non-zero in these rows
    const int64_t chunk = ((kall + TRMV_SPLIT - 1) / TRMV_SPLIT + 7) / 8 * 8;
    const int64_t k0 = (int64_t)blockIdx.y * chunk, k1 = (k0 + chunk < kall) ? k0 + chunk : kall;
    double acc = 0.0;
    if (row < n) {
        const double* Lr = L + row;
        int64_t k = k0 + ph;
        for (; k + 24 < k1; k += 32) {                    // four loads in flight per lane
            const double a0 = Lr[k * ldl], a1 = Lr[(k + 8) * ldl], a2 = Lr[(k + 16) * ldl], a3 = Lr[(k + 24) * ldl];
            acc += a0 * z[k]; acc += a1 * z[k + 8]; acc += a2 * z[k + 16]; acc += a3 * z[k + 24];
        }
        for (; k < k1; k += 8) acc += Lr[k * ldl] * z[k];
    }
    sred[ph][r] = acc;
    __syncthreads();
    if (ph == 0 && row < n) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) s += sred[q][r];
        part[(int64_t)blockIdx.y * n + row] = s;
    }
}

__global__ void trmv_sum_kernel(const double* __restrict__ part, int64_t n, double* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < TRMV_SPLIT; ++q) s += part[(int64_t)q * n + i];
    out[i] = s;
}

int launch_trmv_lower(hipStream_t st, const double* L, int64_t n, int64_t ldl, const double* z, double* part, double* out)
{
    hipLaunchKernelGGL(trmv_lower_part_kernel, dim3((unsigned)((n + TRMV_ROWS - 1) / TRMV_ROWS), TRMV_SPLIT), dim3(256), 0, st,
                       L, n, ldl, z, part);
    hipLaunchKernelGGL(trmv_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, n, out);
    GP_HIP(hipGetLastError());
    return 0;
}

// does the kernel have the rank-64 form draw_f's structured product rests on (gpirt_kernel_check's certificate)?  The default
// kernel does (as every rank >= 48 is taken for it at creation); a refusal's message is not an error here
bool nu_kernel_ok(const KernelSpec& kern)
{
    if (kern.is_default()) return true;
    if (kern.family != GPIRT_KERNEL_SE) return false;          // (a Matern kernel has no such form)
    return kernel_rank_check(kern, NU_LR_RANK, nullptr, nullptr) == 0;
}

int fstar_prep(gpirt_sampler_s* s, gpirt_handle_t hh);

// F for the sampler's kernel on the device (fstar_free.hip): at creation and wherever the host replaces s->kern for good.  The
// decomposition is a property of the kernel alone: the last one is kept per process.  Drains the handle's stream.
int fstar_free_setup(gpirt_sampler_s* s)
{
    s->ff_have = false;
    if (!s->ffF || s->kern.family != GPIRT_KERNEL_SE) return 0;
    static std::mutex mu;
    static double cached_ell = 0.0;
    static std::vector<double> cached;
    std::vector<double> F;
    {
        std::lock_guard<std::mutex> lock(mu);
        if (cached.empty() || cached_ell != s->kern.length_scale) {
            fstar_free_factor(s->kern, cached);
            cached_ell = s->kern.length_scale;
        }
        F = cached;
    }
    GP_HIP(hipMemcpyAsync(s->ffF, F.data(), sizeof(double) * F.size(), hipMemcpyHostToDevice, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));                // (F leaves scope)
    s->ff_have = true; s->ff_ell = s->kern.length_scale;
    return 0;
}

// Does the rank-64 draw_fstar take C from theta alone?  What the structured nu = L z asks (the node rows carried, the kernel's
// rank-64 certificate, K built in fp64, every theta inside the nodes' interval, L the factor of K(theta, theta) as far as
// the sampler can know), and: kstar_rank = 64 in the bordered layout, the item-keyed RNG, F in place for the kernel as it
// stands, no length-scale update (F for a moving kernel is not kept).  From n = 2048 on (GPIRT_FSTAR_FREE=3: at every n;
// =2: never).  Otherwise the chain through L (fstar_prep).
// (state_only: without "L is the factor of K(theta, theta)" -- what a factorisation about to run asks, factor_lr_ok)
bool fstar_free_ok(const gpirt_sampler_s* s, bool state_only = false)
{
    const int mode = s->h->cfg.fstar_free;
    return mode != 2 && (mode == 3 || s->n >= 2048) && s->kr == NU_LR_RANK && s->fstar_rows && s->node_off >= 0 && s->nuV &&
           !stream_mode(s) && s->nu_kern_ok && !s->opt.kernel_fp32 && s->theta_ok && (state_only || !s->theta_alone) && !s->ell.on &&
           s->ffF && s->ff_have && s->kern.family == GPIRT_KERNEL_SE && s->ff_ell == s->kern.length_scale;
}

// Does the factorisation build L's diagonal parts and node rows alone, from theta (factor_lr.hip)?  Only where nothing of the
// steady iteration reads more: the option set, and what draw_f's structured product and the rank-64 draw_fstar with C from
// theta alone ask, their own switches included.  From n = 2048 on (GPIRT_FACTOR_LR=3: at every eligible n; =2: never).
bool factor_lr_ok(const gpirt_sampler_s* s)
{
    const Config& c = s->h->cfg;
    return s->opt.factor_structured && s->theta_L && c.factor_lr != 2 && (c.factor_lr == 3 || s->n >= 2048) &&
           c.nu_lr != 2 && (c.nu_lr == 3 || s->n >= 2048) && fstar_free_ok(s, true);
}

// ... and that chain on `st`: [the basis at theta,] V^T V, M in one work-group, C = V M into draw_fstar's Cu; G = B^T B from
// the node rows as fstar_prep forms it (the same launches: the same bits)
int fstar_prep_free(gpirt_sampler_s* s, hipStream_t st, bool basis)
{
    const int64_t n = s->n;
    const int r = s->kr;
    const double* Bt = s->L + n + s->rank_off;
    if (basis) GP_TRY(launch_nu_lr_basis(st, s->theta, n, s->nu_nodes, s->nu_wts, s->nuV));
    GP_TRY(launch_fstar_free(st, s->nuV, n, s->ffF, GPIRT_JITTER, s->ffW, s->kparts, KSPLIT, s->rhs + (size_t)n * r, s->flags));
    return launch_gemm_splitk(st, false, true, r, r, n, 1.0, Bt, s->ldl, Bt, s->ldl, s->kparts, r, (int64_t)r * r, KSPLIT,
                              s->kP, r, 0.0);
}
int report_degenerate_theta(gpirt_sampler_s* s, int count);
int rebuild_rows(gpirt_sampler_s* s);
int beta_sync(gpirt_sampler_s* s);
int ensure_dense_factor(gpirt_sampler_s* s);
int ensure_factor_width(gpirt_sampler_s* s, int need);

// Z may still be being filled on the sampler's own stream (do_factor's prefill of the NEXT draw_f's normals): whoever reads or
// rewrites Z, or changes the iteration the prefill was keyed by, joins it first and drops it
int z_sync(gpirt_sampler_s* s)
{
    if (s->z_filled_iter != 0 && s->ev_zfill) GP_HIP(hipStreamWaitEvent(s->h->stream, s->ev_zfill, 0));
    s->z_filled_iter = 0;
    return 0;
}

int do_draw_f(gpirt_sampler_s* s)
{
    s->lp_current = false;
    gpirt_handle_t h = s->h;
    hipStream_t st = h->stream;
    const int64_t n = s->n, m = s->m;
    const uint32_t iter = (uint32_t)(s->iter + 1);
    GP_TRY(beta_sync(s));                     // mu of the previous iteration's draw_beta
    s->factor_fresh = false;
    if (!stream_mode(s)) {
        // The structured product (nu_lr.hip) reads the node rows below L: it runs when they are carried and belong to this
        // (theta, L) -- rebuilt here by the explicit solve if they were left stale --, the kernel has the rank-64 form, K was
        // built in fp64, every theta lies in the nodes' interval and L is the factor of K(theta, theta) as far as the sampler
        // can know; from n = 2048 on (GPIRT_NU_LR=3: at every n; =2: never).  Otherwise the dense product, as before.
        const bool nu_lr = s->node_off >= 0 && s->nuV && h->cfg.nu_lr != 2 && (h->cfg.nu_lr == 3 || n >= 2048) &&
                           s->nu_kern_ok && !s->opt.kernel_fp32 && s->theta_ok && !s->theta_alone;
        if (!nu_lr) GP_TRY(ensure_dense_factor(s));               // (the dense product reads all of L)
        if (nu_lr) GP_TRY(rebuild_rows(s));
        if (nu_lr) GP_TRY(ensure_factor_width(s, h->cfg.nu_sub));  // (GPIRT_NU_SUB raised behind a factor in narrower parts)
        const bool prep = s->haux && s->kr > 0 && s->fstar_rows && s->rows_valid && !s->prep_valid;
        // The side work (what the low-rank draw_fstar needs from L alone: the last range of block inverses and the
        // 64-column transposed solve, ~0.6 ms of small DEPENDENT launches) starts at once, beside the fill and the product
        // nu = L z.  Until the end of round 3 it waited for the product with all 1024 columns ("its 256 work-groups would
        // starve it"): what starved was ONE kernel, the 392-register leaf of the block inverses, which cannot share a CU
        // with a 224-register work-group of the product and sat out its whole 1.09 ms -- the side handle now launches
        // the 256-register form of that leaf (trsm.hip, slim_leaf) and the chain is done before the slice kernel is:
        // draw_fstar no longer waits 0.33 ms for it (7.12 -> 6.88 ms per iteration; the product slows by 0.1 ms).
        // GPIRT_PREP_EARLY=2 puts it back behind the product.
        // With C from theta alone (fstar_free.hip) the side work does not wait for anything of the factor but the node rows
        // (G): four small launches behind the basis at theta, no block inverses, no solve.
        const bool free = prep && fstar_free_ok(s);
        if (prep && !free) GP_TRY(ensure_dense_factor(s));        // (fstar_prep solves through L)
        const bool early = prep && !free && !(h->cfg.prep_early == 2 && m > 128);
        if (early || (free && !nu_lr)) GP_HIP(hipEventRecord(s->ev_trmm, st));
        if (nu_lr && s->prep_pending && s->prep_free) {           // (a chain of an earlier draw may still be reading the basis)
            GP_HIP(hipStreamWaitEvent(st, s->ev_prep, 0));
            s->prep_pending = false;
        }
        if (s->z_filled_iter == iter && s->ev_zfill) {
            GP_HIP(hipStreamWaitEvent(st, s->ev_zfill, 0));       // filled behind the previous factorisation (do_factor)
            s->z_filled_iter = 0;
        } else {
            GP_TRY(z_sync(s));                                    // a prefill for ANOTHER iteration may still be writing Z
            GP_TRY(launch_item_uniforms(st, s->opt.seed, iter, GPIRT_ST_F_Z, (uint32_t)s->opt.item0, m, n, s->Z, true, s->h->cfg.zfill_compact == 1));
        }
        {
            ProfPair pp;                                          // (bench.py's roofline: class 3, n^2 m flops)
            GP_TRY(prof_pair_begin(h, st, pp));
            if (nu_lr) {
                // (class 3 with what actually ran: the diagonal parts' triangles and the rank-64 products)
                double flops = 0.0, bytes = 0.0;
                NuLrArgs q{};
                q.L = s->L; q.ldl = s->ldl; q.Bt = s->L + n + s->node_off; q.V = s->nuV; q.Z = s->Z; q.NU = s->NU; q.T = s->nuT;
                q.n = n; q.m = m; q.sub = h->cfg.nu_sub;
                GP_TRY(launch_nu_lr_basis(st, s->theta, n, s->nu_nodes, s->nu_wts, s->nuV));
                if (free) GP_HIP(hipEventRecord(s->ev_trmm, st));       // (the side chain shares this basis)
                GP_TRY(launch_nu_lr(st, q, &flops, &bytes));
                GP_TRY(prof_pair_end(h, st, pp, 3, flops, bytes));
                s->nu_lr_draws += 1;
            } else {
                GP_TRY(launch_gemm(h, st, false, false, TRI_A_LOWER, n, m, n, 1.0, s->L, s->ldl, s->Z, n, 0.0, s->NU, n));
                GP_TRY(prof_pair_end(h, st, pp, 3, (double)n * (double)n * (double)m, 8.0 * (0.5 * (double)n * (double)n + 2.0 * (double)n * (double)m)));
            }
        }
        if (s->amp.mode) GP_TRY(launch_amp_scale(st, s->NU, s->amp.amp, n, m));       // nu_j = a_j (L z_j)
        if (prep && !early && !free) GP_HIP(hipEventRecord(s->ev_trmm, st));
        if (s->ord.on) {                                          // (the ordinal slice: ordinal.hip; y is not read)
            EssOrdArgs a{};
            a.f = s->f; a.nu = s->NU; a.mu = s->mu; a.cat = s->ord.cat; a.thr = s->ord.thr; a.counts = s->ord.counts;
            a.C = s->ord.C; a.n = n; a.m = m; a.k_out = s->ess_k; a.err = s->flags;
            a.seed = s->opt.seed; a.iter = iter; a.item0 = (uint32_t)s->opt.item0;
            a.screen = h->cfg.ess_screen == 1;
            GP_TRY(launch_ess_ord(st, a));
        } else {
        EssArgs a{};
        a.f = s->f; a.nu = s->NU; a.y = s->y; a.mu = s->mu; a.n = n; a.m = m; a.k_out = s->ess_k;
        a.err = s->flags; a.seed = s->opt.seed; a.iter = iter; a.item0 = (uint32_t)s->opt.item0;
        a.ll_exact = h->cfg.ll_exact;
        a.screen = h->cfg.ess_screen == 1;
        // y packed and mu formed again from theta and beta (ess_lin.hip) where mu is known to be b0 + theta b1 of the theta and
        // beta in place; GPIRT_ESS_PACK=2, kernel_fp32 or any other n: the kernel that reads mu and y
        if (h->cfg.ess_pack != 2 && s->mu_linear && s->ess_ypk && !s->opt.kernel_fp32 && ess_pack_eligible(n)) {
            if (!s->ess_ypk_valid) { GP_TRY(launch_ess_pack(st, s->y, n, m, s->ess_ypk)); s->ess_ypk_valid = true; }
            a.ypk = s->ess_ypk; a.theta = s->theta; a.beta = s->beta;
            a.grid = h->cfg.ess_pack == 3 ? 2 * h->n_cu : 0;      // (3: two work-groups per CU stride over the items)
            s->ess_pack_draws += 1;
        }
        GP_TRY(launch_ess(st, a));
        }
        if (prep) {
            // what the low-rank draw_fstar needs from L alone, on the sampler's own stream (see `early` above)
            hipStream_t ax = s->haux->stream;
            GP_HIP(hipStreamWaitEvent(ax, s->ev_trmm, 0));
            if (free) {
                GP_TRY(fstar_prep_free(s, ax, !nu_lr));
            } else {
                s->haux->slim_leaf = early;
                const int rc_prep = fstar_prep(s, s->haux);
                s->haux->slim_leaf = false;
                GP_TRY(rc_prep);
            }
            GP_HIP(hipEventRecord(s->ev_prep, ax));
            s->prep_valid = true; s->prep_pending = true; s->prep_free = free;
        }
        return 0;
    }
    // exact R order: item j draws its n normals, then u, eps0 and one uniform per rejection
    auto plain_item = [&](int64_t j) -> int {
        GP_TRY(launch_rstream_normals(st, s->U, s->pos, 0, n, 1, s->Z));
        GP_TRY(launch_trmv_lower(st, s->L, n, s->ldl, s->Z, s->NU + n, s->NU));        // (the parts go behind NU's first column)
        EssArgs a{};
        a.f = s->f + j * n; a.nu = s->NU; a.y = s->y + j * n; a.mu = s->mu + j * n; a.n = n; a.m = 1;
        a.k_out = s->ess_k + j; a.err = s->flags; a.item0 = (uint32_t)j;
        a.U = s->U; a.pos = s->pos; a.cap = s->U_cap;
        return launch_ess(st, a);
    };
    const bool spec = s->spec_ok;
    if (!spec) {
        for (int64_t j = 0; j < m; ++j) GP_TRY(plain_item(j));
        return 0;
    }
    // Three items per pass over L (rng_ess.hip): a pass is anchored at the first item whose start is known, computes L z for
    // the one place its normals start at and for the 15 + 32 places the next two items' normals can start at, and runs the
    // three slice loops; a slice loop that ran longer than its successors' candidates reach just ends the pass early.  All of
    // it is device-side state (next_item, posv): the host enqueues ceil(m / 3) passes and a few spare ones -- a pass that finds
    // every item done leaves at once -- and reads the item counter back once.
    bool tiles64 = false;                       // (L as fp64 tiles: only the one-phase replay reads them -- built when it first runs)
    Rs3Args a{};
    a.U = s->U; a.cap = s->U_cap; a.Nrm = s->Nrm; a.anchor = s->anchor; a.pos = s->pos; a.posv = s->posv; a.k_out = s->ess_k;
    a.err = s->flags; a.n = n; a.m = m; a.Lt = s->Lt; a.nkb = rs_tile_quads(n); a.part = s->rs_part;
    a.units = s->rs_units; a.nunits = s->rs_nunits; a.nfull = s->rs_nfull;
    a.lim1 = RS3_C1; a.lim2 = RS3_C2;
    if (h->rs_cand_limit > 0) {
        if (h->rs_cand_limit < a.lim1) a.lim1 = h->rs_cand_limit;
        if (h->rs_cand_limit < a.lim2) a.lim2 = h->rs_cand_limit;
    }
    a.f = s->f; a.y = s->y; a.mu = s->mu; a.partial = s->rs_partial; a.flags = s->rs_flags;
    // the normals draw_f can reach: m items of 2n + 2 uniforms + their rejections (the window's own slack, stream_window)
    GP_TRY(launch_rs3_begin(st, a, (uint64_t)m * (2ull * (uint64_t)n + 2ull) + 512ull * (uint64_t)m + 4096ull));
    int64_t pass = 0, done = 0;
    int64_t one_phase = 0;                      // passes of the one-phase replay: the draw's progress bound counts these alone
    bool topped = false;
    // Predict + verify (rs_predict.hip; GPIRT_RS_PREDICT=2: every pass in fp64, the one-phase replay).  The predictor's
    // passes leave predicted starts; phase B computes every item at its predicted start exactly and commits, in order, what
    // the prediction did not break.  A round that commits nothing (the predictor stalled on its first item) hands the rest
    // of the draw to the one-phase replay, which always makes progress and reports genuine errors.
    bool predict = h->cfg.rs_predict != 2;
    // The structured form of the pass (rs_lr.hip): the blocks of L below the diagonal parts as V C, built from theta alone.  It
    // serves the draw's rounds until one of them finds a misprediction (the dense pass takes the rest of the draw over); three
    // such draws in a row, or a coefficient block the construction itself flags, switch it off for this sampler.
    bool lr = predict && s->lr_on, lr_missed = false;
    // (single-precision tiles of L: the structured pass reads the diagonal parts only; the whole triangle follows if the dense pass is needed)
    bool tiles32_full = !lr;
    if (predict) GP_TRY(launch_rs32_tiles(st, s->L, n, s->ldl, s->Lt32, lr));
    if (lr) {
        RsLrSetup q{};
        q.theta = s->theta; q.n = n; q.nodes = s->lr_nodes; q.wts = s->lr_wts; q.Mn = s->lr_M; q.eps = GPIRT_JITTER; q.L = s->L; q.ldl = s->ldl;
        q.V64 = s->lr_V64; q.Gb = s->lr_Gb; q.V32t = s->lr_V32t; q.Ct32 = s->lr_Ct32; q.nk8 = rs32_tile_octs(n); q.bad = s->lr_bad;
        GP_TRY(launch_rs_lr_setup(st, q));
    }
    while (done < m) {
        const int64_t left = m - done;
        int64_t count = (left + RS3_SLOTS - 1) / RS3_SLOTS + left / 40 + 2;
        // (a one-phase pass resolves >= 1 item.  A predicted round enqueues spare passes -- ~0.375 per item left + 4 -- and may
        // commit a single item behind a misprediction, so its passes do not count: a round that commits nothing hands over to
        // the one-phase replay below, hence at most m predicted rounds)
        if (one_phase > 4 * m + 64) { set_error("R-stream replay: draw_f made no progress"); return GPIRT_E_NUMERIC; }
        if (predict) {
            // (a slice loop that rejects 16 points in a row costs a pass of its own.)  How many passes a draw needs is a property
            // of the chain's state and moves slowly: the predictor counts its real passes (rs_ctl[3]) and the next draw enqueues
            // that many per item + 3 % + 4 -- a pass that finds every item predicted leaves at once, but 120 of them per draw
            // were 0.5 ms; too few only costs one more round of both phases for the items left over
            count = (left + RS3_SLOTS - 1) / RS3_SLOTS + left / 8 + 4;
            if (s->rs_pass_rate > 0.0) {
                const int64_t hint = (int64_t)(s->rs_pass_rate * 1.03 * (double)left) + 4;
                if (hint < count) count = hint;
            }
            Rs3Args ap = a;
            ap.anchor = s->anchorP; ap.pos = s->rs_posP; ap.k_out = s->rs_kpred; ap.err = s->rs_errP;
            ap.units = s->rs_unitsP; ap.nunits = s->rs_nunitsP; ap.nfull = s->rs_nfullP;
            if (!lr && !tiles32_full) { GP_TRY(launch_rs32_tiles(st, s->L, n, s->ldl, s->Lt32)); tiles32_full = true; }
            ap.lr = lr ? 1 : 0;
            if (lr) {
                ap.units = s->lr_units; ap.nunits = ap.nfull = s->lr_nunits;
                ap.Ct32 = s->lr_Ct32; ap.lrY = s->lr_Y; ap.V32t = s->lr_V32t;
            }
            ap.Lt32 = s->Lt32; ap.nk8 = rs32_tile_octs(n); ap.part32 = s->rs_part32; ap.mispredict = h->rs_mispredict;
            ap.dec_part = s->rs_dec_part; ap.dec_rec = s->rs_dec_rec; ap.dec_ticket = s->rs_dec_ticket; ap.pass_count = s->rs_ctl + 3;
            GP_TRY(launch_rs_pred_start(st, s->anchor, s->anchorP, s->ess_k, m));
            for (int64_t q = 0; q < count; ++q, ++pass) {
                s->rs_tag += 1ull << 20;
                ap.tag = s->rs_tag;
                ap.trace = (h->rs_trace_pass >= 0 && pass == h->rs_trace_pass) ? s->rs_trace : nullptr;
                ProfPair pp;                                      // (bench.py's roofline: class 4, the lower triangle as floats)
                GP_TRY(prof_pair_begin(h, st, pp));
                GP_TRY(launch_rs3p_products(st, ap));
                // (algorithmic bytes / flops of the pass: the lower triangle as floats -- or, structured, the diagonal parts' rows and C)
                const double pass_el = lr ? (double)(RS3P_KC + RS_LR_RANK) * (double)n : 0.5 * (double)n * (double)(n + 1);
                GP_TRY(prof_pair_end(h, st, pp, 4, 2.0 * RS3_CAND * pass_el, 4.0 * pass_el));
                if (lr) GP_TRY(launch_rs_lr_apply(st, ap));
                GP_TRY(launch_rs3p_decide(st, ap));
            }
            // phase B: the items [done, predicted) at their predicted starts, exactly
            const int64_t mc = m - done;
            GP_TRY(launch_rs_gather(st, s->Nrm, s->posv, s->anchorP, n, done, m, s->Z));
            GP_TRY(launch_gemm(h, st, false, false, TRI_A_LOWER, n, mc, n, 1.0, s->L, s->ldl, s->Z, n, 0.0, s->NU, n));
            RsVerifyArgs v{};
            v.f = s->f; v.nu = s->NU; v.y = s->y; v.mu = s->mu; v.n = n; v.m = m; v.j0 = done;
            v.U = s->U; v.cap = s->U_cap; v.posv = s->posv; v.anchorP = s->anchorP;
            v.kv = s->rs_kv; v.used = s->rs_used; v.ierr = s->rs_ierr;
            GP_TRY(launch_rs_verify(st, v));
            GP_TRY(launch_rs_commit(st, v, s->anchor, s->pos, s->rs_ctl, s->flags, s->f, s->ess_k));
        } else {
        if (!tiles64) { GP_TRY(launch_rs_tiles(st, s->L, n, s->ldl, s->Lt)); tiles64 = true; }
        for (int64_t q = 0; q < count; ++q, ++pass, ++one_phase) {
            s->rs_tag += 1ull << 20;
            a.tag = s->rs_tag;
            a.trace = (h->rs_trace_pass >= 0 && pass == h->rs_trace_pass) ? s->rs_trace : nullptr;
            ProfPair pp;                                          // (bench.py's roofline: class 4, the lower triangle's bytes)
            GP_TRY(prof_pair_begin(h, st, pp));
            GP_TRY(launch_rs3_products(st, a));
            GP_TRY(prof_pair_end(h, st, pp, 4, 2.0 * RS3_CAND * 0.5 * (double)n * (double)(n + 1), 8.0 * 0.5 * (double)n * (double)(n + 1)));
            GP_TRY(launch_rs3_slice(st, a));
        }
        }
        GP_HIP(hipMemcpyAsync(s->h_next, s->anchor, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        GP_HIP(hipMemcpyAsync(s->h_next + 1, s->flags, sizeof(int), hipMemcpyDeviceToHost, st));
        if (predict) GP_HIP(hipMemcpyAsync(s->h_next + 2, s->rs_ctl + 3, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (predict) GP_HIP(hipMemcpyAsync(s->h_next + 3, s->rs_ctl + 1, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (lr) GP_HIP(hipMemcpyAsync(s->h_next + 4, s->lr_bad, sizeof(int), hipMemcpyDeviceToHost, st));
        if (s->stream_open && !topped) { GP_TRY(ahead_topup(s, stream_window(s))); topped = true; }     // the next window's uniforms, while the items run
        GP_HIP(hipStreamSynchronize(st));
        if ((int)s->h_next[1] != 0) break;                    // (an error flag: stream_end / check report it)
        if (predict) {
            if (lr && (int)s->h_next[4] != 0) { s->lr_on = false; lr = false; }                  // the construction flagged itself
            if (lr && s->h_next[3] != s->rs_mis_seen) { lr = false; lr_missed = true; }          // a misprediction: dense from here
            s->rs_mis_seen = s->h_next[3];
        }
        if ((int64_t)s->h_next[0] <= done) {
            if (predict) {                                    // the predictor stalled on its first item: the one-phase replay goes on
                predict = false;
                GP_TRY(launch_advance_pos(st, s->rs_ctl + 2, 1));     // (counted: gpirt_sampler_get "rs_stats"[2])
                continue;
            }
            set_error("R-stream replay: draw_f made no progress"); return GPIRT_E_NUMERIC;
        }
        if (predict && (int64_t)s->h_next[0] > done) {
            // real passes per item of this round (the counter is monotonic: difference to the last reading)
            const uint64_t real = s->h_next[2] - s->rs_pass_seen;
            s->rs_pass_seen = s->h_next[2];
            s->rs_pass_rate = (double)real / (double)((int64_t)s->h_next[0] - done);
        }
        done = (int64_t)s->h_next[0];
    }
    if (s->lr_on) {
        s->lr_strikes = lr_missed ? s->lr_strikes + 1 : 0;
        if (s->lr_strikes >= 3) s->lr_on = false;
    }
    return 0;
}

// The factor-only part of the low-rank draw_fstar (bordered layout): B^T (r x n) sits in the rows below L;
//   Cu = L^-T B  (n x r: transpose, then the transposed solve through the block inverses of L),
//   G  = B^T B   (r x r, split-K over n).
// Runs on hh->stream with hh's workspaces: the sampler's private handle beside draw_f, or the caller's handle inline.
int fstar_prep(gpirt_sampler_s* s, gpirt_handle_t hh)
{
    hipStream_t st = hh->stream;
    const int64_t n = s->n;
    const int r = s->kr;
    double* Cu = s->rhs + (size_t)n * r;
    const double* Bt = s->L + n + s->rank_off;
    GP_TRY(launch_transpose(st, Bt, r, n, s->ldl, Cu, n));
    if (hh == s->haux && hh->inv_partial_L == s->L && hh->inv_partial_pairs > 0 && hh->trsm_winv_L != s->L) {
        // most of the block inverses were built while the last outer panel was being factored (do_factor): the rest now.
        // (inv_partial_L lives on the shared side handle: another sampler's early build in between resets it, and this
        // one then rebuilds everything below, in launch_trsm_lower.)
        GP_TRY(trsm_inverses_build(hh, st, s->L, n, s->ldl, true, hh->inv_partial_pairs, (n / 256) / 2));
        trsm_inverses_mark(hh, s->L, n, s->ldl, true);
        hh->inv_partial_L = nullptr; hh->inv_partial_pairs = 0;
    }
    // the block inverses of L are reused when this handle already holds them (built by an earlier solve against the
    // same factor) -- invalidate_factor_products() clears that whenever L changes
    GP_TRY(launch_trsm_lower(hh, st, s->L, n, s->ldl, Cu, r, n, true, true));
    return launch_gemm_splitk(st, false, true, r, r, n, 1.0, Bt, s->ldl, Bt, s->ldl, s->kparts, r, (int64_t)r * r, KSPLIT,
                              s->kP, r, 0.0);
}

int do_draw_fstar(gpirt_sampler_s* s, uint32_t iter)
{
    s->lp_current = false;
    gpirt_handle_t h = s->h;
    hipStream_t st = h->stream;
    const int64_t n = s->n, m = s->m, N = s->N;
    double* tmp = s->rhs;                    // n x N : L^-1 kstar
    double* W = s->rhs + (size_t)n * N;      // n x m : L^-1 f, then L^-T L^-1 f
    const bool fused = s->opt.fstar_fused != 0;
    GP_TRY(beta_sync(s));                     // mu_star
    s->factor_fresh = false;
    GP_TRY(rebuild_rows(s));
    if (s->kr > 0) {
        // K*^T = U V^T exactly (see gpirt_sampler_create), so with B = L^-1 U and C = L^-T B = S^-1 U:
        //   ||L^-1 k*_j||^2 = v_j^T (B^T B) v_j          (src/draw-fstar.cpp:19-20)
        //   k*_j^T S^-1 f   = v_j^T (C^T f)              (:7, :24-25)
        // Two solves with r right-hand sides each (forward, then transposed with the same block inverses)
        // replace the solve with N + m; the N x n x m product shrinks to r x n x (r + m).
        const int r = s->kr;
        double* Bu = s->rhs;                                  // n x r : U, then B
        double* Cu = s->rhs + (size_t)n * r;                  // n x r : B, then C
        const bool bordered = s->fstar_rows;
        if (bordered) {
            // C = L^-T B and G = B^T B depend on the factor alone: usually already under way on the sampler's own
            // stream since draw_f's product finished (do_draw_f); otherwise computed here
            if (!s->prep_valid) {                                 // (rows rebuilt above if they were stale)
                if (s->prep_pending) { GP_HIP(hipStreamWaitEvent(st, s->ev_prep, 0)); s->prep_pending = false; }
                s->prep_free = fstar_free_ok(s);
                if (s->prep_free) GP_TRY(fstar_prep_free(s, st, true));
                else { GP_TRY(ensure_dense_factor(s)); GP_TRY(fstar_prep(s, h)); }
                s->prep_valid = true;
            }
            else if (s->prep_pending) { GP_HIP(hipStreamWaitEvent(st, s->ev_prep, 0)); s->prep_pending = false; }
            if (s->prep_free) s->fstar_free_draws += 1;
        } else {
            GP_TRY(launch_se_kernel(st, s->kern, s->theta, n, s->knodes, r, Bu, n, 0.0));
            GP_TRY(launch_trsm_lower(h, st, s->L, n, s->ldl, Bu, r, n, false));
            GP_HIP(hipMemcpyAsync(Cu, Bu, sizeof(double) * (size_t)n * r, hipMemcpyDeviceToDevice, st));
            GP_TRY(launch_trsm_lower(h, st, s->L, n, s->ldl, Cu, r, n, true, true));
        }
        double* G = s->kP;                                    // r x r
        double* Q = s->kP + (size_t)r * r;                    // r x m
        if (!bordered)
            GP_TRY(launch_gemm_splitk(st, true, false, r, r, n, 1.0, Bu, n, Bu, n, s->kparts, r, (int64_t)r * r, KSPLIT, G, r, 0.0));
        GP_TRY(launch_gemm_splitk(st, true, false, r, m, n, 1.0, Cu, n, s->f, n, s->kparts, r, (int64_t)r * m, KSPLIT, Q, r, 0.0));
        GP_TRY(launch_lowrank_s(st, s->kV, N, r, G, r, s->s));
        GP_TRY(launch_gemm(h, st, false, false, TRI_NONE, N, m, r, 1.0, s->kV, N, Q, r, 0.0, s->mean, N));
        FstarEpiArgs a{};
        a.mean = s->mean; a.mu_star = s->mu_star; a.s = s->s; a.out = s->fstar; a.N = N; a.m = m;
        a.seed = s->opt.seed; a.iter = iter; a.item0 = (uint32_t)s->opt.item0; a.err = s->flags;
        if (stream_mode(s)) { a.U = s->U; a.pos = s->pos; a.cap = s->U_cap; a.off_scratch = s->fstar_off; }
        if (s->shape.on) a.mean_out = s->shape.gbar;          // the draw's smooth curve, for the shape posteriors
        if (s->amp.mode) a.amp = s->amp.amp;
        return launch_fstar_epilogue(st, a);
    }
    GP_HIP(hipMemcpyAsync(W, s->f, sizeof(double) * (size_t)n * m, hipMemcpyDeviceToDevice, st));
    if (s->ext_grid) {
        // tmp = L^-1 k* came out of the bordered factorisation as the rows below L (N x n): one transpose puts it
        // where the solve used to leave it; only the m item columns are still solved for                      :19
        if (!fused) GP_TRY(launch_se_kernel(st, s->kern, s->theta, n, s->tstar, N, s->kstar, n, 0.0));  // :17 (for :25)
        GP_TRY(launch_transpose(st, s->L + n, N, n, s->ldl, tmp, n));
        GP_TRY(launch_trsm_lower(h, st, s->L, n, s->ldl, W, m, n, false));                    // :7 inner
    } else {
        if (fused) {
            GP_TRY(launch_se_kernel(st, s->kern, s->theta, n, s->tstar, N, tmp, n, 0.0));               // :17
        } else {
            GP_TRY(launch_se_kernel(st, s->kern, s->theta, n, s->tstar, N, s->kstar, n, 0.0));
            GP_HIP(hipMemcpyAsync(tmp, s->kstar, sizeof(double) * (size_t)n * N, hipMemcpyDeviceToDevice, st));
        }
        GP_TRY(launch_trsm_lower(h, st, s->L, n, s->ldl, s->rhs, N + m, n, false));                // :19, :7 inner
    }
    GP_TRY(launch_colnorm_s(st, tmp, n, N, n, s->s));                                         // :20
    if (fused) {
        GP_TRY(launch_gemm(h, st, true, false, TRI_NONE, N, m, n, 1.0, tmp, n, W, n, 0.0, s->mean, N));
    } else {
        // (the block inverses of L are the forward solve's: same factor, not modified since)
        GP_TRY(launch_trsm_lower(h, st, s->L, n, s->ldl, W, m, n, true, true));                    // :7 outer
        GP_TRY(launch_gemm(h, st, true, false, TRI_NONE, N, m, n, 1.0, s->kstar, n, W, n, 0.0, s->mean, N)); // :25
    }
    FstarEpiArgs a{};
    a.mean = s->mean; a.mu_star = s->mu_star; a.s = s->s; a.out = s->fstar; a.N = N; a.m = m;
    a.seed = s->opt.seed; a.iter = iter; a.item0 = (uint32_t)s->opt.item0; a.err = s->flags;
    if (stream_mode(s)) { a.U = s->U; a.pos = s->pos; a.cap = s->U_cap; a.off_scratch = s->fstar_off; }
    if (s->shape.on) a.mean_out = s->shape.gbar;
    if (s->amp.mode) a.amp = s->amp.amp;
    return launch_fstar_epilogue(st, a);                                                      // :26-28
}

// logpost_out (N x n) from the curve fstar_in (N x m) through the sampler's scratch (tfd, tf_gq, tf_aux, Gpm): what
// theta_partial launches, also for the proposal's curve of gpirt_sampler_draw_scale (the scratch is free again once the first
// product has finished on the stream)
int theta_product(gpirt_sampler_s* s, const double* fstar_in, double* logpost_out)
{
    hipStream_t st = s->h->stream;
    const int64_t n = s->n, m = s->m, N = s->N;
    const int64_t Np = (N + 127) / 128 * 128;     // Gpm is padded to whole 128-row tiles (zero rows)
    // logpost (N x n) = G+ Y+^T + G- Y-^T   (draw-theta.cpp:15-19 summed over this rank's items): in exact fixed point on the
    // int8 matrix cores (theta_fixed.hip); the fp64 product runs behind it only under the device flag that says a row of G
    // could not be scaled (|f*| beyond exp()'s range, non-finite), or instead of it with GPIRT_THETA_FIXED=2
    const int* only_if = nullptr;
    if (s->h->cfg.theta_fixed == 1) {
        GP_TRY(launch_theta_fixed(st, fstar_in, N, n, m, s->tfd, s->tf_y8, s->tf_gq, s->tf_aux, logpost_out, N, false, s->h));
        only_if = tf_overflow(s->tf_aux, s->tfd);
    }
    GP_TRY(launch_loglik_terms(st, fstar_in, N, m, s->Gpm, Np, only_if));
    GP_TRY(launch_gemm(s->h, st, false, true, TRI_NONE, N, n, 2 * m, 1.0, s->Gpm, Np, s->Ypm, n, 0.0, logpost_out, N, Np, only_if));
    return launch_theta_nan_fix(st, s->Gpm, Np, s->Ypm, n, m, logpost_out, N, N, only_if);   // (a missing answer over a NaN f*)
}

// the ordinal counterpart (ordinal.hip): the fp64 product of the N x C m table with the one-hot indicators, K = C m, and the NaN
// fix behind it -- the int8 fixed-point product is not extended to one-hot operands
int theta_product_ord(gpirt_sampler_s* s, const double* fstar_in, double* logpost_out)
{
    hipStream_t st = s->h->stream;
    const OrdState& A = s->ord;
    const int64_t n = s->n, m = s->m, N = s->N;
    const int64_t Np = (N + 127) / 128 * 128;
    GP_TRY(launch_ord_loglik_terms(st, fstar_in, N, m, A.C, A.thr, A.G, Np));
    GP_TRY(launch_gemm(s->h, st, false, true, TRI_NONE, N, n, (int64_t)A.C * m, 1.0, A.G, Np, A.Y, n, 0.0, logpost_out, N, Np));
    return launch_ord_nan_fix(st, A.G, Np, A.cat, n, m, logpost_out, N, N);
}

int do_theta_partial(gpirt_sampler_s* s)
{
    if (s->ord.on) {
        GP_TRY(theta_product_ord(s, s->fstar, s->logpost));
        s->lp_current = true;
        return 0;
    }
    GP_TRY(theta_product(s, s->fstar, s->logpost));
    s->lp_current = true;
    return 0;
}

int do_theta_finish(gpirt_sampler_s* s)
{
    hipStream_t st = s->h->stream;
    ThetaArgs a{};
    a.logpost = s->logpost; a.N = s->N; a.n = s->n; a.stabilise = s->opt.theta_stabilise;
    a.seed = s->opt.seed; a.iter = (uint32_t)(s->iter + 1);
    a.theta_out = s->theta; a.degenerate = s->flags + 1; a.err = s->flags;
    if (stream_mode(s)) { a.U = s->U; a.pos = s->pos; a.cap = s->U_cap; }
    if (s->pop.mode) { a.log_prior = s->pop.log_prior; a.codes = s->pop.codes; }           // (the group's row in place of N(0, 1))
    GP_TRY(launch_theta_sample(st, a));
    if (stream_mode(s)) GP_TRY(launch_advance_pos(st, s->pos, (uint64_t)s->n));
    s->lp_current = false;
    s->mu_linear = false;                 // (theta moved: mu is the old theta's until draw_beta has run)
    s->theta_ok = true;                   // grid values
    return 0;
}

// draw_theta for the respondents [blk_i0, blk_i0 + blk_n) from the gathered f* of ALL items: the same product and
// the same sampling kernel as the single-GPU path, restricted to a column block of the log-posterior -- so the
// sums over items run in one GEMM in item order (bit-identical to one GPU) and what crosses the links per
// iteration is f* (N x m, 8 MB at the metric size) instead of the N x n partial log-posterior (66 MB).
int do_theta_block(gpirt_sampler_s* s)
{
    hipStream_t st = s->h->stream;
    const int64_t N = s->N, nb = s->blk_n, mt = s->blk_m;
    const int64_t Np = (N + 127) / 128 * 128;
    GP_HIP(hipMemsetAsync(s->theta_stage, 0, sizeof(double) * (size_t)s->n, st));
    if (nb == 0) return 0;
    const int* only_if = nullptr;
    if (s->h->cfg.theta_fixed == 1) {                       // (as do_theta_partial; exact sums: the same bits as one GPU's product)
        GP_TRY(launch_theta_fixed(st, s->fstar_full, N, nb, mt, s->tfd_blk, s->tf_y8_blk, s->tf_gq_blk, s->tf_aux_blk, s->logpost_blk, N, false, s->h));
        only_if = tf_overflow(s->tf_aux_blk, s->tfd_blk);
    }
    GP_TRY(launch_loglik_terms(st, s->fstar_full, N, mt, s->Gpm_full, Np, only_if));
    GP_TRY(launch_gemm(s->h, st, false, true, TRI_NONE, N, nb, 2 * mt, 1.0, s->Gpm_full, Np, s->Ypm_blk, nb, 0.0,
                       s->logpost_blk, N, Np, only_if));
    GP_TRY(launch_theta_nan_fix(st, s->Gpm_full, Np, s->Ypm_blk, nb, mt, s->logpost_blk, N, N, only_if));
    ThetaArgs a{};
    a.logpost = s->logpost_blk; a.N = N; a.n = nb; a.i0 = s->blk_i0; a.stabilise = s->opt.theta_stabilise;
    a.seed = s->opt.seed; a.iter = (uint32_t)(s->iter + 1);
    a.theta_out = s->theta_stage; a.degenerate = s->flags + 1; a.err = s->flags;
    return launch_theta_sample(st, a);
}

int launch_beta_on(gpirt_sampler_s* s, hipStream_t st)
{
    s->lp_current = false;
    s->mu_linear = !s->ord.on;                                    // (draw_beta_kernel and draw_beta_reg_kernel store mu = b0 + theta_i b1)
    if (s->ord.on) {                                              // (the slope alone: the intercept is pinned at 0)
        BetaOrdArgs a{};
        a.beta = s->beta; a.theta = s->theta; a.cat = s->ord.cat; a.f = s->f; a.thr = s->ord.thr; a.pm = s->pm; a.ps = s->ps;
        a.step = s->step; a.C = s->ord.C; a.n = s->n; a.m = s->m; a.N = s->N; a.mu = s->mu; a.mu_star = s->mu_star;
        a.seed = s->opt.seed; a.iter = (uint32_t)(s->iter + 1); a.item0 = (uint32_t)s->opt.item0;
        return launch_draw_beta_ord(st, a);
    }
    BetaArgs a{};
    a.beta = s->beta; a.theta = s->theta; a.y = s->y; a.f = s->f; a.pm = s->pm; a.ps = s->ps;
    a.step = s->step; a.n = s->n; a.m = s->m; a.N = s->N; a.mu = s->mu; a.mu_star = s->mu_star;
    a.seed = s->opt.seed; a.iter = (uint32_t)(s->iter + 1); a.item0 = (uint32_t)s->opt.item0;
    a.err = s->flags;
    a.screen = s->h->cfg.beta_screen == 1;           // (y was checked at creation: +1, -1 or NaN)
    if (stream_mode(s)) { a.U = s->U; a.pos = s->pos; a.item_off = s->beta_off; a.cap = s->U_cap; }
    GP_TRY(launch_draw_beta(st, a));
    if (stream_mode(s)) GP_TRY(launch_advance_pos(st, s->pos, s->beta_total));
    return 0;
}

// a deferred draw_beta runs NOW on the main stream; one already running on the sampler's stream is joined
int beta_sync(gpirt_sampler_s* s)
{
    if (s->beta_deferred) {
        s->beta_deferred = false;
        GP_TRY(launch_beta_on(s, s->h->stream));
    }
    if (s->beta_pending) {
        GP_HIP(hipStreamWaitEvent(s->h->stream, s->ev_beta, 0));
        s->beta_pending = false;
    }
    return 0;
}

int do_draw_beta(gpirt_sampler_s* s)
{
    const bool defer = s->h->cfg.early_inv != 2 && !stream_mode(s) && s->haux && s->ev_beta && s->initialised;
    GP_TRY(beta_sync(s));
    if (defer) { s->beta_deferred = true; return 0; }     // do_factor launches it behind the factorisation's last outer panel
    return launch_beta_on(s, s->h->stream);
}

// ---- the consistent step's carry (include/gpirt_hip.h; the kernel is carry.hip's) ---------------------------------------------
// the refusals of gpirt_sampler_carry_f and gpirt_sampler_step_consistent, each with its reason
int carry_refusals(gpirt_sampler_s* s, int nugget, const char* entry)
{
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", entry); return GPIRT_E_ARG; }
    if (stream_mode(s)) {
        set_error("carry: rng = reference (GPIRT_RNG_RSTREAM) is refused, R's stream has no such draw");
        return GPIRT_E_ARG;
    }
    if (nugget != 0 && nugget != 1) { set_error("carry: nugget = %d, it must be 0 or 1", nugget); return GPIRT_E_ARG; }
    return 0;
}

// f <- the curve at the new theta (+ the nugget), on the main stream: behind theta_finish / theta_commit, in front of draw_beta.
// mu_star is the one this iteration's draw_fstar added (draw_beta, which rewrites it, has not run yet).  timed: the launch
// between the carry's own two events (the caller reads them once the stream has passed the second).
int do_carry_f(gpirt_sampler_s* s, int nugget, bool timed)
{
    CarryState& c = s->carry;
    hipStream_t st = s->h->stream;
    // a draw_beta still held back or running on the sampler's own stream reads the f this stage rewrites (inside a step: none)
    GP_TRY(beta_sync(s));
    s->lp_current = false;
    s->mu_linear = false;
    if (!c.counters) {
        GP_TRY(dalloc(s, &c.counters, 6));
        GP_HIP(hipMemsetAsync(c.counters, 0, 6 * sizeof(unsigned long long), st));
    }
    CarryArgs a{};
    a.slot = (int)(c.calls & 1);              // (the launch adds to this call's pair and zeroes the other for the next call)
    a.f = s->f; a.theta = s->theta; a.fstar = s->fstar; a.mu_star = s->mu_star; a.n = s->n; a.m = s->m; a.N = s->N;
    a.amp = s->amp.mode ? s->amp.amp : nullptr;
    a.counters = c.counters;
    a.seed = s->opt.seed; a.iter = (uint32_t)(s->iter + 1); a.item0 = (uint32_t)s->opt.item0; a.nugget = nugget;
    if (timed) {
        for (hipEvent_t& t : c.tev) if (!t) GP_HIP(hipEventCreate(&t));
        GP_HIP(hipEventRecord(c.tev[0], st));
    }
    GP_TRY(launch_carry_f(st, a));
    if (timed) GP_HIP(hipEventRecord(c.tev[1], st));
    c.calls += 1;
    c.last_ms = 0.0;
    return 0;
}

// everything derived from the factor (C, G, cached block inverses on either handle) is stale once L changes
void invalidate_factor_products(gpirt_sampler_s* s)
{
    s->prep_valid = false;
    if (s->haux && s->haux->inv_partial_L == s->L) { s->haux->inv_partial_L = nullptr; s->haux->inv_partial_pairs = 0; }
    if (s->h->trsm_winv_L == s->L) s->h->trsm_winv_L = nullptr;
    if (s->haux && s->haux->trsm_winv_L == s->L) s->haux->trsm_winv_L = nullptr;
}

// the main stream waits for whatever the sampler's own stream still has in flight.  z_too: also a prefill of the next
// draw_f's normals, which is then dropped (every caller but do_factor, whose own prefill it would be)
int aux_join(gpirt_sampler_s* s, bool beta_too = true, bool z_too = true)
{
    hipStream_t st = s->h->stream;
    if (s->prep_pending) { GP_HIP(hipStreamWaitEvent(st, s->ev_prep, 0)); s->prep_pending = false; }
    if (beta_too) GP_TRY(beta_sync(s));
    if (z_too) GP_TRY(z_sync(s));
    return 0;
}

// S = K(theta, theta) + jitter into the lower blocks of L; with the bordered layout also K(c, theta) into the rows below
// (theta: the sampler's, or the saved theta a structured factor belongs to -- ensure_dense_factor)
int build_cov(gpirt_sampler_s* s, const double* theta = nullptr)
{
    hipStream_t st = s->h->stream;
    if (!theta) theta = s->theta;
    s->L_structured = false;              // (whatever L held is being overwritten)
    GP_TRY(launch_se_kernel_lower(st, s->kern, theta, s->n, s->L, s->ldl, GPIRT_JITTER, s->opt.kernel_fp32 != 0));
    if (s->fstar_rows && s->kr > 0) GP_TRY(launch_se_kernel(st, s->kern, s->knodes, s->kr, theta, s->n, s->L + s->n + s->rank_off, s->ldl, 0.0));
    if (s->ext_grid) GP_TRY(launch_se_kernel(st, s->kern, s->tstar, s->N, theta, s->n, s->L + s->n, s->ldl, 0.0));
    // the node rows of draw_f's structured product (nu_lr.hip); with kr == 64 they are the rows just written
    if (s->node_off >= 0 && !(s->fstar_rows && s->kr == NU_LR_RANK))
        GP_TRY(launch_se_kernel(st, s->kern, s->nu_nodes, NU_LR_RANK, theta, s->n, s->L + s->n + s->node_off, s->ldl, 0.0));
    return 0;
}

// the rows below L for the CURRENT (theta, L) by the explicit forward solve (after L or theta was set from outside)
int rebuild_rows(gpirt_sampler_s* s)
{
    if (s->ext == 0 || s->rows_valid) return 0;
    GP_TRY(ensure_dense_factor(s));       // (the solves below go through all of L)
    hipStream_t st = s->h->stream;
    const int64_t n = s->n, cols = s->ext_grid ? s->N : (s->fstar_rows ? s->kr : 0);
    double* Bu = s->rhs;
    if (cols > 0) {
        GP_TRY(launch_se_kernel(st, s->kern, s->theta, n, s->ext_grid ? s->tstar : s->knodes, cols, Bu, n, 0.0));
        GP_TRY(launch_trsm_lower(s->h, st, s->L, n, s->ldl, Bu, cols, n, false));
        GP_TRY(launch_transpose(st, Bu, n, cols, n, s->L + n + (s->ext_grid ? 0 : s->rank_off), s->ldl));
    }
    if (s->node_off >= 0 && !(s->fstar_rows && s->kr == NU_LR_RANK)) {
        // the node rows: a 64-column solve of their own in every layout (the same arithmetic whatever rides beside them)
        GP_TRY(launch_se_kernel(st, s->kern, s->theta, n, s->nu_nodes, NU_LR_RANK, Bu, n, 0.0));
        GP_TRY(launch_trsm_lower(s->h, st, s->L, n, s->ldl, Bu, NU_LR_RANK, n, false));
        GP_TRY(launch_transpose(st, Bu, n, NU_LR_RANK, n, s->L + n + s->node_off, s->ldl));
    }
    s->rows_valid = true;
    return 0;
}

// S under the sampler's kernel, built and factored in place on the main stream -- do_factor without its side work (the early
// block inverses, the Z prefill, a held-back draw_beta).  Whoever calls it has made sure nothing still reads the old factor.
// With factor_lr_ok (not for gpirt_sampler_init, whose f = L z is the dense product): the diagonal parts and the node rows
// alone, from theta (factor_lr.hip) -- theta is kept in theta_L for whoever asks for the rest of L later.
// the structured factor of K(theta, theta) in parts `part` wide on the main stream: the diagonal parts into L, the node rows below
int launch_structured_factor(gpirt_sampler_s* s, const double* theta, int part)
{
    FactorLrArgs a{};
    a.theta = theta; a.n = s->n; a.nodes = s->nu_nodes; a.wts = s->nu_wts; a.V = s->nuV; a.F = s->ffF; a.eps = GPIRT_JITTER;
    a.G = s->flrG; a.Xh = s->flrXh; a.X = s->flrX; a.D = s->flrD; a.L = s->L; a.ldl = s->ldl; a.Bt = s->L + s->n + s->node_off; a.err = s->flags;
    a.part = part;
    GP_TRY(launch_factor_lr(s->h, s->h->stream, a));
    s->L_part_width = part;
    return 0;
}

// The width of the structured factor's parts: nobody in the steady iteration reads more of L than the diagonal parts of draw_f's
// product, GPIRT_NU_SUB wide, so that is how wide they are factored, part / 64 rounds instead of eight -- from n = 2048 on
// (GPIRT_FLR_NARROW=3: at every eligible n; =2: always 512).  Whoever reads wider parts later asks ensure_factor_width first.
int factor_lr_width(const gpirt_sampler_s* s)
{
    const Config& c = s->h->cfg;
    return (c.flr_narrow != 2 && (c.flr_narrow == 3 || s->n >= 2048)) ? c.nu_sub : NU_LR_PART;
}

// the width of the diagonal parts L holds; 0: L is dense
int factor_width(const gpirt_sampler_s* s) { return s->L_structured ? s->L_part_width : 0; }

// Whoever reads diagonal parts `need` wide calls this first: a structured factor in narrower parts is replaced by the structured
// factor of K(theta_L, theta_L) in 512-wide parts, on the main stream behind whatever still reads the node rows or the basis,
// and everything derived from the factor is dropped.  Counted neither as a structured nor as a dense factorisation.
int ensure_factor_width(gpirt_sampler_s* s, int need)
{
    if (!s->L_structured || s->L_part_width >= need) return 0;
    hipStream_t st = s->h->stream;
    if (s->prep_pending) { GP_HIP(hipStreamWaitEvent(st, s->ev_prep, 0)); s->prep_pending = false; }
    invalidate_factor_products(s);
    return launch_structured_factor(s, s->theta_L, NU_LR_PART);
}

int factor_core(gpirt_sampler_s* s)
{
    hipStream_t st = s->h->stream;
    invalidate_factor_products(s);
    if (!s->in_init && factor_lr_ok(s)) {
        if (s->ev_flr) GP_HIP(hipEventRecord(s->ev_flr, st));          // (the side work of do_factor starts here)
        if (!s->sticky_info) GP_HIP(hipMemsetAsync(s->h->d_info, 0, sizeof(int), st));
        GP_HIP(hipMemcpyAsync(s->theta_L, s->theta, sizeof(double) * (size_t)s->n, hipMemcpyDeviceToDevice, st));
        GP_TRY(launch_structured_factor(s, s->theta, factor_lr_width(s)));
        s->L_structured = true;
        s->rows_valid = true;
        s->theta_alone = false;
        s->factor_lr_count += 1;
        return 0;
    }
    GP_TRY(build_cov(s));                                                                                  // :76-77
    s->rows_valid = true;
    s->theta_alone = false;
    s->dense_factor_count += 1;
    return launch_potrf_lower(s->h, st, s->L, s->n, s->ldl, false, !s->sticky_info, s->ext);               // :78
}

// Whoever reads more of L than its diagonal parts and node rows calls this first: a structured factor (factor_lr.hip) is
// replaced by the dense factorisation of K(theta_L, theta_L) -- the existing build and factorisation, on the main stream --
// and everything derived from the factor is dropped.  The rows below L then belong to theta_L as before: rows_valid stands.
int ensure_dense_factor(gpirt_sampler_s* s)
{
    if (!s->L_structured) return 0;
    hipStream_t st = s->h->stream;
    if (s->prep_pending) { GP_HIP(hipStreamWaitEvent(st, s->ev_prep, 0)); s->prep_pending = false; }      // (G = B^T B may still read the rows)
    invalidate_factor_products(s);
    GP_TRY(build_cov(s, s->theta_L));
    s->dense_factor_count += 1;
    s->factor_fresh = false;              // (a hang-guard expiry here is reported, not repaired: theta may have moved on)
    return launch_potrf_lower(s->h, st, s->L, s->n, s->ldl, false, false, s->ext);
}

int do_factor(gpirt_sampler_s* s)
{
    hipStream_t st = s->h->stream;
    GP_TRY(aux_join(s, false, true));     // nothing of the old factor may still be read when it is overwritten (a held-back
                                          // draw_beta does not read it: it is launched below, behind the factorisation)
    GP_TRY(factor_core(s));
    // The low-rank draw_fstar's transposed solve (fstar_prep) goes through the inverses of L's 1024 x 1024 diagonal blocks:
    // ~5 GFLOP to build at n = 8192, and they only need the DIAGONAL blocks, final panel by panel.  Those of every outer
    // panel but the last are built on the sampler's own stream while the last outer panel is factored (16 + 8 whole-CU
    // work-groups and small updates: most of the chip is idle then); only the last block and the solve are left behind.
    const bool early_inv = s->h->cfg.early_inv != 2;
    // Behind a structured factor (factor_lr.hip) there is no last outer panel: its batched 64-column rounds leave most of the
    // chip idle from the start, so the Z prefill and the held-back draw_beta wait for the event recorded where it began
    // (prelast_cols says nothing about it), and no block inverses are built (nobody reads them).
    const bool lr = s->L_structured && s->ev_flr;
    hipEvent_t ev_side = lr ? s->ev_flr : s->h->ev_prelast;
    const bool side_phase = lr || s->h->prelast_cols >= 2048;
    // Not when the next draw_fstar takes C from theta alone (fstar_free.hip): nobody would read them.
    if (early_inv && !s->L_structured && s->haux && s->kr > 0 && s->fstar_rows && !stream_mode(s) && s->h->prelast_cols >= 2048 && !fstar_free_ok(s)) {
        const int64_t p1 = (s->h->prelast_cols / 512) & ~(int64_t)1;
        hipStream_t ax = s->haux->stream;
        GP_HIP(hipStreamWaitEvent(ax, s->h->ev_prelast, 0));
        GP_TRY(trsm_inverses_reserve(s->haux, ax, s->n, s->kr, true));
        s->haux->trsm_winv_L = nullptr;                      // whatever the side handle held is being overwritten
        GP_TRY(trsm_inverses_build(s->haux, ax, s->L, s->n, s->ldl, true, 0, p1));
        s->haux->inv_partial_L = s->L; s->haux->inv_partial_pairs = p1;
    }
    if (early_inv && s->initialised && !s->in_init && s->haux && s->ev_zfill && !stream_mode(s) && side_phase) {
        // (not from gpirt_sampler_init, first or repeated: it fills Z itself for the initial f right behind its factorisation)
        // ... and the next draw_f's N(0,1) draws (the factorisation closes iteration s->iter + 1; the next draw_f is
        // iteration s->iter + 2).  Z was last read by this iteration's nu = L z, long finished on the main stream.
        hipStream_t ax = s->haux->stream;
        const uint32_t next_iter = (uint32_t)(s->iter + 2);
        GP_HIP(hipStreamWaitEvent(ax, ev_side, 0));
        GP_TRY(launch_item_uniforms(ax, s->opt.seed, next_iter, GPIRT_ST_F_Z, (uint32_t)s->opt.item0, s->m, s->n, s->Z, true, s->h->cfg.zfill_compact == 1));
        GP_HIP(hipEventRecord(s->ev_zfill, ax));
        s->z_filled_iter = next_iter;
    }
    if (s->beta_deferred) {
        // draw_beta of THIS iteration (do_draw_beta held it back): beside the last outer panel on the sampler's stream
        // when there is such a phase, otherwise right here on the main stream
        s->beta_deferred = false;
        if (s->haux && side_phase) {
            hipStream_t ax = s->haux->stream;
            GP_HIP(hipStreamWaitEvent(ax, ev_side, 0));                // (causally behind theta and f on the main stream)
            GP_TRY(launch_beta_on(s, ax));
            GP_HIP(hipEventRecord(s->ev_beta, ax));
            s->beta_pending = true;
        } else {
            GP_TRY(launch_beta_on(s, st));
        }
    }
    // nothing has read this L yet: a hang-guard expiry in it can still be repaired in place (a structured factor has no guard)
    s->factor_fresh = !s->L_structured;
    return 0;
}

// The factorisation enqueued last ended in a hang-guard expiry (info[1]) and nothing has consumed its L yet (factor_fresh):
// theta is intact, so K is rebuilt from it and factored once more with the launch-per-step panel -- the schedule differs,
// the products do not, and the chain goes on as if nothing had happened (L within rounding of the undisturbed factor).
// Whatever was launched behind the bad factor on the sampler's own stream and depends on it (early block inverses) is
// dropped; the Z prefill and a held-back draw_beta do not depend on L and stay.
int recover_factor(gpirt_sampler_s* s)
{
    gpirt_handle_t h = s->h;
    hipStream_t st = h->stream;
    if (s->haux) GP_HIP(hipStreamSynchronize(s->haux->stream));
    GP_TRY(potrf_guard_reset(h, st));
    s->prep_pending = false;
    invalidate_factor_products(s);
    const int saved = h->cfg.panel;
    h->cfg.panel = 2;
    int rc = build_cov(s);
    if (!rc) rc = launch_potrf_lower(h, st, s->L, s->n, s->ldl, false, true, s->ext);
    s->dense_factor_count += 1;
    h->cfg.panel = saved;
    GP_TRY(rc);
    s->rows_valid = true;
    s->theta_alone = false;
    s->factor_fresh = true;
    return 0;
}

// drains the stream and repairs a hang-guard expiry of the factorisation enqueued last (callers that drain it anyway)
int factor_guard_sync(gpirt_sampler_s* s)
{
    gpirt_handle_t h = s->h;
    GP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 8 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));
    if (h->h_info[1] != 0 && s->factor_fresh && h->cfg.panel != 2) GP_TRY(recover_factor(s));
    return 0;
}

// ---- the length scale as a parameter of the chain (include/gpirt_hip.h; the kernels are ell.hip's) ------------------------------
void ell_free(EllState* e)
{
    for (void* p : { (void*)e->Lsave, (void*)e->fprop, (void*)e->delta, (void*)e->rec, (void*)e->nuprop, (void*)e->dq, (void*)e->ld,
                     (void*)e->rec_c, (void*)e->nonfin, (void*)e->flag })
        if (p) hipFree(p);
    if (e->h_flag) hipHostFree(e->h_flag);
    if (e->ev) hipEventDestroy(e->ev);
    for (hipEvent_t t : e->tev) if (t) hipEventDestroy(t);
    // t counts the sampler's calls of each update: enabling again does not replay their uniforms
    const uint32_t calls[2] = { e->up[ELL_WHITENED].t, e->up[ELL_CENTRED].t };
    *e = EllState();
    e->up[ELL_WHITENED].t = calls[0]; e->up[ELL_CENTRED].t = calls[1];
}

// ---- per-item GP amplitudes (include/gpirt_hip.h; the kernels are amp.hip's) ---------------------------------------------------
void amp_free(AmpState* a)
{
    for (void* p : { (void*)a->amp, (void*)a->d_grid, (void*)a->d_log_prior, (void*)a->rec, (void*)a->idx, (void*)a->width,
                     (void*)a->counts, (void*)a->hist, (void*)a->draws, (void*)a->cbuf })
        if (p) hipFree(p);
    for (hipEvent_t t : a->tev) if (t) hipEventDestroy(t);
    for (hipEvent_t t : a->ctev) if (t) hipEventDestroy(t);
    const uint32_t calls = a->t, ccalls = a->ct;      // the sampler's draw_amp / draw_amp_centred calls: enabling again does not replay their uniforms
    *a = AmpState();
    a->t = calls; a->ct = ccalls;
}

// ---- ordinal responses (include/gpirt_hip.h; the kernels are ordinal.hip's) -----------------------------------------------------
void ord_free(OrdState* p)
{
    const uint32_t calls = p->t;      // the sampler's draw_thresholds calls: enabling again does not replay their uniforms
    ofit_free(&p->fit);
    oscore_free(&p->score);
    for (void* q : { (void*)p->cat, (void*)p->d_grid, (void*)p->d_log_prior, (void*)p->thr, (void*)p->lp, (void*)p->cum, (void*)p->Y,
                     (void*)p->G, (void*)p->idx, (void*)p->window, (void*)p->counts, (void*)p->stat, (void*)p->hist, (void*)p->draws })
        if (q) hipFree(q);
    for (hipEvent_t t : p->tev) if (t) hipEventDestroy(t);
    *p = OrdState{};
    p->t = calls;
}

// "<entry> is refused while ordinal responses are on: <why>"
int ord_refuse(const gpirt_sampler_s* s, const char* entry, const char* why)
{
    if (!s->ord.on) return 0;
    set_error("%s is refused while ordinal responses are on: %s", entry, why);
    return GPIRT_E_ARG;
}
#define ORD_BINARY "it evaluates the binary likelihood of y"

// ---- the population prior for theta (include/gpirt_hip.h; the kernels are pop.hip's) -------------------------------------------
void pop_free(PopState* p)
{
    for (void* q : { (void*)p->codes, (void*)p->log_prior, (void*)p->d_mu, (void*)p->d_sd, (void*)p->d_lse, (void*)p->d_hyper_mu,
                     (void*)p->d_hyper_sd, (void*)p->lp_mu, (void*)p->lp_sd, (void*)p->idx, (void*)p->stats, (void*)p->counts,
                     (void*)p->hist_mu, (void*)p->hist_sd, (void*)p->draws })
        if (q) hipFree(q);
    for (hipEvent_t t : p->tev) if (t) hipEventDestroy(t);
    const uint32_t calls = p->t;      // the sampler's draw_pop calls: enabling again does not replay their uniforms
    *p = PopState();
    p->t = calls;
}

// The main stream waits for whatever the sampler's own stream still has in flight -- the early block inverses read L, a
// deferred draw_beta writes beta and mu -- WITHOUT dropping a prefilled Z, which aux_join's z_too would: the update touches
// neither Z nor the iteration it is keyed by.
int ell_join(gpirt_sampler_s* s)
{
    GP_TRY(aux_join(s, true, false));
    if (s->haux) {
        GP_HIP(hipEventRecord(s->ell.ev, s->haux->stream));
        GP_HIP(hipStreamWaitEvent(s->h->stream, s->ell.ev, 0));
    }
    return 0;
}

void ell_set_kernel(gpirt_sampler_s* s, double ell)
{
    s->kern.length_scale = ell;
    s->kern.inv_ell = 1.0 / ell;
}

// a factor nobody has looked at yet: its info words would be lost under the next factorisation's
int ell_settle_factor(gpirt_sampler_s* s)
{
    if (!s->factor_fresh) return 0;
    gpirt_handle_t h = s->h;
    hipStream_t st = h->stream;
    GP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (h->h_info[1] != 0) {
        // a hang-guard expiry nothing has consumed: repaired in place, and the words read again, as gpirt_sampler_check does
        if (h->cfg.panel == 2) return report_panel_guard(h, h->h_info, st);
        GP_TRY(recover_factor(s));
        GP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        if (h->h_info[1] != 0) return report_panel_guard(h, h->h_info, st);
    }
    if (*h->h_info > 0) {
        set_error("chol(): decomposition failed (leading minor of order %d is not positive definite)", *h->h_info);
        return *h->h_info;
    }
    return 0;
}

// One update of the index, whitened or centred.  What the two share is here: the factor settled, the call counted only when it
// ends in one of the four outcomes, the proposal, the join, f -> nu's buffer and the factor buffer saved, nu = L^-1 f, the
// proposal's factor, the decision read back, a hang-guard expiry repaired once, everything put back unless accepted, the timing.
// They differ in their uniforms' item index, their width and counters, and in what is enqueued between the proposal's factor and
// the read of the decision.
int do_draw_ell(gpirt_sampler_s* s, int kind)
{
    EllState& e = s->ell;
    EllUpdate& c = e.up[kind];
    gpirt_handle_t h = s->h;
    hipStream_t st = h->stream;
    const int64_t n = s->n, m = s->m;
    GP_TRY(ell_settle_factor(s));
    s->lp_current = false;
    // the call is counted, and its pair of uniforms consumed, when it ends in one of the four outcomes: an update that returns
    // an error has not happened (updates = accepted + rejected + out_of_range + failed at all times)
    const uint32_t t = c.t + 1;
    const double u0 = item_uniform(s->opt.seed, t, GPIRT_ST_ELL, (uint32_t)kind, 0),        // (item index 0: whitened, 1: centred)
                 u1 = item_uniform(s->opt.seed, t, GPIRT_ST_ELL, (uint32_t)kind, 1);
    auto counted = [&]() { c.t = t; c.updates += 1; c.last_u0 = u0; c.last_u1 = u1; };
    const int w = c.w;
    int j = (int)floor(u0 * (double)(2 * w));
    if (j > 2 * w - 1) j = 2 * w - 1;
    const int kp = e.k + (j < w ? j - w : j - w + 1);
    if (kp < 0 || kp >= e.P) { counted(); c.last_proposed = kp; c.out_of_range += 1; c.last = 2; return 0; }      // (the proposal is symmetric: nothing else runs)
    GP_TRY(ell_join(s));
    GP_TRY(ensure_dense_factor(s));       // (the update saves, solves through and multiplies by all of L)
    s->factor_fresh = false;
    const bool timed = s->timing;
    if (timed)
        for (hipEvent_t& t : e.tev) if (!t) GP_HIP(hipEventCreate(&t));
    auto tick = [&](int i) { if (timed) hipEventRecord(e.tev[i], st); };
    const KernelSpec kern_before = s->kern;
    const bool rows_before = s->rows_valid;
    const size_t fbytes = sizeof(double) * (size_t)(n * m), lbytes = sizeof(double) * (size_t)(s->ldl * n);
    // everything back as it was: the saved buffer holds the factor AND the rows below it
    auto restore = [&]() -> int {
        s->kern = kern_before;
        s->rows_valid = rows_before;
        invalidate_factor_products(s);
        GP_HIP(hipMemcpyAsync(s->L, e.Lsave, lbytes, hipMemcpyDeviceToDevice, st));
        return 0;
    };
    // nu = L^-1 f (NU is free between steps), then the proposal's factor in place of the saved one
    tick(0);
    GP_HIP(hipMemcpyAsync(s->NU, s->f, fbytes, hipMemcpyDeviceToDevice, st));
    if (kind == ELL_CENTRED) GP_HIP(hipMemcpyAsync(e.nuprop, s->f, fbytes, hipMemcpyDeviceToDevice, st));
    GP_HIP(hipMemcpyAsync(e.Lsave, s->L, lbytes, hipMemcpyDeviceToDevice, st));
    tick(1);
    GP_TRY(launch_trsm_lower(h, st, s->L, n, s->ldl, s->NU, m, n, false));
    tick(2);
    ell_set_kernel(s, e.grid[(size_t)kp]);
    int rc = factor_core(s);
    c.factorisations += 1;
    tick(3);
    const double lp_diff = e.log_prior[(size_t)kp] - e.log_prior[(size_t)e.k], log_u = log(u1);
    for (int attempt = 0; !rc; ++attempt) {
        if (kind == ELL_WHITENED) {
            // f' = L' nu, the likelihood's change, the decision, f <- f' behind it
            rc = launch_gemm(h, st, false, false, TRI_A_LOWER, n, m, n, 1.0, s->L, s->ldl, s->NU, n, 0.0, e.fprop, n);
            tick(4);
            if (!rc) rc = launch_ell_delta(st, s->f, e.fprop, s->mu, s->y, n, m, e.delta, e.nonfin);
            tick(5);
            if (!rc) rc = launch_ell_decide(st, e.delta, e.nonfin, m, lp_diff, log_u, h->d_info, e.rec, e.flag);
            tick(6);
            if (!rc) rc = launch_ell_commit(st, e.flag, s->f, e.fprop, n * m);
            tick(7);
        } else {
            // nu' = L'^-1 f (f does not move: no product, no commit), the prior's change in its two parts, the decision
            if (attempt > 0 && hipMemcpyAsync(e.nuprop, s->f, fbytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
                set_error("length-scale update: copying f failed: %s", hipGetErrorString(hipGetLastError()));
                rc = GPIRT_E_HIP;
            }
            if (!rc) rc = launch_trsm_lower(h, st, s->L, n, s->ldl, e.nuprop, m, n, false);
            tick(4);
            if (!rc) rc = launch_ell_quad(st, s->NU, e.nuprop, n, m, e.dq, e.nonfin);
            tick(5);
            if (!rc) rc = launch_ell_logdet(st, e.Lsave, s->L, n, s->ldl, e.ld);
            tick(6);
            if (!rc) rc = launch_ell_decide_centred(st, e.dq, e.nonfin, m, e.ld, lp_diff, log_u, h->d_info, e.rec_c, e.flag);
            tick(7);
        }
        if (rc) break;
        // the decision: 4 bytes and a stream synchronisation, as gpirt_sampler_check's
        if (hipMemcpyAsync(e.h_flag, e.flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            set_error("length-scale update: reading the decision failed: %s", hipGetErrorString(hipGetLastError()));
            rc = GPIRT_E_HIP;
            break;
        }
        if (*e.h_flag != 3) break;
        // a hang-guard expiry in the proposal's factor (nothing was committed): once more with the launch-per-step panel
        if (attempt > 0 || h->cfg.panel == 2) {
            hipMemcpyAsync(h->h_info, h->d_info, 8 * sizeof(int), hipMemcpyDeviceToHost, st);
            hipStreamSynchronize(st);
            rc = report_panel_guard(h, h->h_info, st);
            break;
        }
        s->factor_fresh = true;
        rc = recover_factor(s);
        s->factor_fresh = false;
        c.factorisations += 1;
    }
    if (rc) { restore(); return rc; }
    // the parts' device time, once the stream has passed the last event (timing on: one more synchronisation)
    auto times = [&](bool restored) -> int {
        if (!timed) return 0;
        tick(9);
        GP_HIP(hipEventSynchronize(e.tev[9]));
        for (int i = 0; i < GPIRT_ELL_PARTS; ++i) {
            float ms = 0.f;
            if (i < 7) hipEventElapsedTime(&ms, e.tev[i], e.tev[i + 1]);
            else if (restored) hipEventElapsedTime(&ms, e.tev[8], e.tev[9]);
            c.part_ms[i] = ms;
        }
        return 0;
    };
    counted();
    c.last_proposed = kp;
    if (*e.h_flag == 1) {
        e.k = kp; c.accepted += 1; c.last = 1;
        invalidate_factor_products(s);        // (the solve for nu may have left block inverses of the OLD factor behind)
        return times(false);
    }
    if (*e.h_flag == 2) {
        c.failed += 1; c.last = 3;
        GP_HIP(hipMemsetAsync(h->d_info, 0, sizeof(int), st));       // a non-positive minor of the PROPOSAL is not the chain's
    } else {
        c.last = 0;
    }
    tick(8);                                  // (the copy back alone: from here to the last event)
    GP_TRY(restore());
    return times(true);
}

// draw_theta's CDF came out 0/0 for some respondents: the reference reads theta_star[N] out of bounds there
// (src/draw-theta.cpp:28, quirk Q5); the device wrote NaN and counted them -- the chain cannot go on.
int report_degenerate_theta(gpirt_sampler_s* s, int count)
{
    hipMemsetAsync(s->flags + 1, 0, sizeof(int), s->h->stream);
    set_error("draw_theta: exp() underflowed for %d respondent(s) (0/0 in the reference's CDF, src/draw-theta.cpp:23-34); "
              "theta_stabilise = 1 draws from the same distribution without the underflow", count);
    return GPIRT_E_NUMERIC;
}

inline void mark(gpirt_sampler_s* s, int idx)
{
    if (s->timing) hipEventRecord(s->ev[idx], s->h->stream);
}

// every word of a struct's reserved[] is zero (NULL)
template <typename T, size_t N>
bool all_zero(const T (&r)[N])
{
    for (const T& v : r)
        if (v) return false;
    return true;
}

// ---- the analysis blocks: what their stage entries and the run loop share ------------------------------------------------------
// "<what> not enabled (<entry>)" unless on; what: the subject with its verb ("the rank posteriors are", "scoring is")
int needs(bool on, const char* what, const char* entry)
{
    if (on) return 0;
    set_error("%s not enabled (%s)", what, entry);
    return GPIRT_E_ARG;
}

// One block as its entries see it: the state its functions take (order and predict: their parent's), its device block,
// whether it is on and the two parts of its refusal.
template <class St>
struct Block { St* st; void* block; bool on; const char* what; const char* entry; };
template <class St>
using BlockOf = Block<St> (*)(gpirt_sampler_t);
template <class St>
int needs(const Block<St>& b) { return needs(b.on, b.what, b.entry); }

Block<PpcState> blk_ppc(gpirt_sampler_t s)
{
    return { &s->ppc, s->ppc.block, s->ppc.on,
             "the posterior predictive checks are", "gpirt_sampler_ppc_enable" };
}
Block<PairState> blk_pairs(gpirt_sampler_t s)
{
    return { &s->ppc.pairs, s->ppc.pairs.block, s->ppc.on && s->ppc.pairs.on,
             "the pairwise item checks are", "gpirt_sampler_ppc_pairs_enable" };
}
Block<BinState> blk_bins(gpirt_sampler_t s)
{
    return { &s->ppc.bins, s->ppc.bins.block, s->ppc.on && s->ppc.bins.on,
             "the theta-binned item fit is", "gpirt_sampler_ppc_bins_enable" };
}
Block<DifState> blk_dif(gpirt_sampler_t s)
{
    return { &s->ppc.dif, s->ppc.dif.block, s->ppc.on && s->ppc.dif.on,
             "the group-wise item fit is", "gpirt_sampler_ppc_dif_enable" };
}
Block<PpsState> blk_scores(gpirt_sampler_t s)
{
    return { &s->ppc.scores, s->ppc.scores.block, s->ppc.on && s->ppc.scores.on,
             "the score-based checks are", "gpirt_sampler_ppc_scores_enable" };
}
Block<PrsState> blk_person(gpirt_sampler_t s)
{
    return { &s->ppc.person, s->ppc.person.block, s->ppc.on && s->ppc.person.on,
             "the person fit is", "gpirt_sampler_ppc_person_enable" };
}
Block<RsdState> blk_resid(gpirt_sampler_t s)
{
    return { &s->ppc.resid, s->ppc.resid.block, s->ppc.on && s->ppc.resid.on,
             "the residual correlations are", "gpirt_sampler_ppc_resid_enable" };
}
Block<RankState> blk_rank(gpirt_sampler_t s)
{
    return { &s->rank, s->rank.block, s->rank.on,
             "the rank posteriors are", "gpirt_sampler_rank_enable" };
}
Block<ShapeState> blk_shape(gpirt_sampler_t s)
{
    return { &s->shape, s->shape.block, s->shape.on,
             "the shape posteriors are", "gpirt_sampler_shape_enable" };
}
Block<ShapeState> blk_order(gpirt_sampler_t s)
{
    return { &s->shape, s->shape.order.block, s->shape.on && s->shape.order.on,
             "the order posteriors are", "gpirt_sampler_shape_order_enable" };
}
Block<SumscoreState> blk_sumscore(gpirt_sampler_t s)
{
    return { &s->sumscore, s->sumscore.block, s->sumscore.on,
             "the sum-score posteriors are", "gpirt_sampler_sumscore_enable" };
}
Block<EquateState> blk_equate(gpirt_sampler_t s)
{
    return { &s->equate, s->equate.block, s->equate.on,
             "the score equating is", "gpirt_sampler_equate_enable" };
}
Block<LooState> blk_loo(gpirt_sampler_t s)
{
    return { &s->loo, s->loo.block, s->loo.on,
             "PSIS-LOO is", "gpirt_sampler_loo_enable" };
}
Block<AcfState> blk_acf(gpirt_sampler_t s)
{
    return { &s->acf, s->acf.block, s->acf.on,
             "the autocorrelation ESS is", "gpirt_sampler_acf_enable" };
}
Block<GroupsState> blk_groups(gpirt_sampler_t s)
{
    return { &s->groups, s->groups.block, s->groups.on,
             "the group posteriors are", "gpirt_sampler_groups_enable" };
}
Block<ScoreState> blk_score(gpirt_sampler_t s)
{
    return { &s->score, s->score.block, s->score.on,
             "scoring is", "gpirt_sampler_score_enable" };
}
Block<ScoreState> blk_predict(gpirt_sampler_t s)
{
    return { &s->score, s->score.pred.block, s->score.pred.on,
             "prediction is", "gpirt_sampler_score_predict_enable" };
}

// gpirt_sampler_X_state: the block and its size once the stream has finished the last accumulate (the header's counters are
// the kernels'); seal (ppc): refreshes the header instead, which synchronises too
template <class St>
int stage_state(gpirt_sampler_t s, BlockOf<St> of, int64_t (*words)(const St*), void** d_state, int64_t* bytes,
                int (*seal)(hipStream_t, St*) = nullptr)
{
    GP_ARG(s && d_state && bytes);
    const Block<St> b = of(s);
    GP_TRY(needs(b));
    if (seal) GP_TRY(seal(s->h->stream, b.st));
    else GP_HIP(hipStreamSynchronize(s->h->stream));
    *d_state = b.block;
    *bytes = words(b.st) * (int64_t)sizeof(uint64_t);
    return 0;
}

// gpirt_sampler_X_get
template <class St>
int stage_get(gpirt_sampler_t s, BlockOf<St> of, int (*get)(hipStream_t, St*, const char*, void*, int64_t), const char* name,
              void* h_out, int64_t bytes)
{
    GP_ARG(s && name && h_out && bytes >= 0);
    const Block<St> b = of(s);
    GP_TRY(needs(b));
    return get(s->h->stream, b.st, name, h_out, bytes);
}

// What every gpirt_sampler_X_enable ends with, after the refusals that leave the old state alone: that state goes once no
// kernel runs on its accumulators any more (shape: or stores gbar), and with `on` alloc() makes the new one -- its own
// refusals first; nothing is left of a state that failed.
template <class St, class Alloc>
int stage_enable(gpirt_sampler_t s, St* st, void (*release)(St*), bool on, Alloc alloc)
{
    GP_HIP(hipStreamSynchronize(s->h->stream));
    release(st);
    if (!on) return 0;
    const int rc = alloc();
    if (rc) release(st);
    return rc;
}

// One draw as the blocks read it: the sampler's live state after a step, or a verified checkpoint slot of mcmc_run (iter:
// the completed iterations of that state, which keys the PPC's replicate).
struct DrawView { const double *theta, *beta, *f, *mu, *fstar, *gbar; uint32_t iter; };
DrawView live_view(gpirt_sampler_t s) { return { s->theta, s->beta, s->f, s->mu, s->fstar, s->shape.gbar, (uint32_t)s->iter }; }

// each block's accumulate on a view, on the main stream (the pair, bin, group, score, person and residual add-ons travel
// inside the PPC's, the prediction inside the score's, the order posteriors inside the shape's)
int acc_summary(gpirt_sampler_t s, const DrawView& v) { return launch_summary_accumulate(s->h->stream, &s->sum, v.theta, v.beta, v.f, v.mu, s->y, v.fstar); }
int acc_ppc(gpirt_sampler_t s, const DrawView& v) { return launch_ppc_accumulate(s->h->stream, &s->ppc, v.f, v.mu, s->y, s->opt.seed, v.iter, v.theta); }
int acc_rank(gpirt_sampler_t s, const DrawView& v) { return launch_rank_accumulate(s->h->stream, &s->rank, v.theta); }
int acc_score(gpirt_sampler_t s, const DrawView& v) { return launch_score_accumulate(s->h, s->h->stream, &s->score, v.fstar); }
int acc_shape(gpirt_sampler_t s, const DrawView& v) { return launch_shape_accumulate(s->h->stream, &s->shape, v.gbar); }
int acc_sumscore(gpirt_sampler_t s, const DrawView& v) { return launch_sumscore_accumulate(s->h->stream, &s->sumscore, v.fstar); }
int acc_equate(gpirt_sampler_t s, const DrawView& v) { return launch_equate_accumulate(s->h, s->h->stream, &s->equate, v.fstar); }
int acc_loo(gpirt_sampler_t s, const DrawView& v) { return launch_loo_accumulate(s->h->stream, &s->loo, v.f, v.mu); }
int acc_acf(gpirt_sampler_t s, const DrawView& v) { return launch_acf_accumulate(s->h->stream, &s->acf, v.theta, v.beta, v.f, v.mu, s->y); }
int acc_groups(gpirt_sampler_t s, const DrawView& v) { return launch_groups_accumulate(s->h->stream, &s->groups, v.theta, v.f, v.mu, s->y); }

// mcmc_run's draw: every block that is on (what the run named, enabled before the loop; the ACF and the groups are stage-only), in this
// order on the stream.  A live view needs beta_sync first (the summaries and the PPC read beta and mu).
int accumulate_run(gpirt_sampler_t s, const DrawView& v)
{
    if (s->sum.parts) GP_TRY(acc_summary(s, v));
    if (s->ppc.on) GP_TRY(acc_ppc(s, v));
    if (s->rank.on) GP_TRY(acc_rank(s, v));
    if (s->score.on) GP_TRY(acc_score(s, v));
    if (s->shape.on) GP_TRY(acc_shape(s, v));
    if (s->sumscore.on) GP_TRY(acc_sumscore(s, v));
    if (s->equate.on) GP_TRY(acc_equate(s, v));
    if (s->loo.on) GP_TRY(acc_loo(s, v));
    return 0;
}

// gpirt_sampler_X_accumulate: the block's piece on the live state; join_beta: draw_beta (beta, mu) may still be deferred to
// the sampler's own stream
template <class St>
int stage_accumulate(gpirt_sampler_t s, BlockOf<St> of, int (*piece)(gpirt_sampler_t, const DrawView&), bool join_beta = false)
{
    GP_ARG(s && s->initialised);
    GP_TRY(needs(of(s)));
    if (join_beta) GP_TRY(beta_sync(s));
    return piece(s, live_view(s));
}

// "<what>: top = <top> is outside 1..<max>"
int check_top(const char* what, int top, int max)
{
    if (top >= 1 && top <= max) return 0;
    set_error("%s: top = %d is outside 1..%d", what, top, max);
    return GPIRT_E_ARG;
}

// every answer of the new respondents (n_new x m on the host) is +1, -1 or NaN
int score_check_new(const double* h_y_new, int64_t n_new, int64_t m)
{
    for (int64_t g = 0; g < n_new * m; ++g) {
        const double v = h_y_new[g];
        if (!(v == 1.0 || v == -1.0 || v != v)) { set_error("scoring: y_new must be +1, -1 or NaN (a missing response)"); return GPIRT_E_ARG; }
    }
    return 0;
}

}  // namespace

extern "C" {

int gpirt_sampler_create(gpirt_sampler_t* out, gpirt_handle_t h, const double* h_y, int64_t n,
                         int64_t m, const double* h_theta0, const double* h_pm, const double* h_ps,
                         const double* h_step, const gpirt_options* opts, gpirt_rstream_t rs)
{
    GP_ARG(out && h && h_y && h_theta0 && h_pm && h_ps && h_step && n > 0 && m > 0);
    *out = nullptr;
    for (int64_t i = 0; i < n * m; ++i) {          // (the slice kernels fold y into f, nu and mu: rng_ess.hip)
        const double v = h_y[i];
        if (!(v == 1.0 || v == -1.0 || v != v)) { set_error("y must be +1, -1 or NaN (a missing response)"); return GPIRT_E_ARG; }
    }
    gpirt_sampler_s* s = new (std::nothrow) gpirt_sampler_s();
    if (!s) { set_error("out of host memory"); return GPIRT_E_ALLOC; }
    s->h = h; s->n = n; s->m = m; s->N = GPIRT_NGRID;
    if (opts) s->opt = *opts; else gpirt_default_options(&s->opt);
    if (s->opt.m_total <= 0) s->opt.m_total = m;
    s->kern = h->kern;
    if (!s->kern.is_default()) {
        // the single-precision build is the default kernel's (config C5); the rank form must pass the kernel's certificate
        // (gpirt_kernel_check: under the default kernel every allowed rank is taken as before, r = 16 and 32 included)
        if (s->opt.kernel_fp32) {
            set_error("kernel_fp32 needs the default kernel (squared exponential, length_scale 1): the handle's kernel is family %d, "
                      "length_scale %g", s->kern.family, s->kern.length_scale);
            delete s;
            return GPIRT_E_ARG;
        }
        if (s->opt.kstar_rank != 0 && s->opt.fstar_fused && s->opt.kstar_rank >= 16 && s->opt.kstar_rank <= 128 &&
            (s->opt.kstar_rank % 16) == 0) {           // (any other value is refused below, with the message it always had)
            const int rc_k = kernel_rank_check(s->kern, s->opt.kstar_rank, nullptr, nullptr);
            if (rc_k) { delete s; return rc_k; }
        }
    }
    if (stream_mode(s)) {
        if (!rs) { set_error("GPIRT_RNG_RSTREAM needs an R stream state"); delete s; return GPIRT_E_ARG; }
        if (s->opt.item0 != 0 || s->opt.m_total != m) {
            set_error("R-stream replay is sequential over items and cannot be sharded"); delete s; return GPIRT_E_ARG;
        }
        rstream_sync(rs);            // (another sampler may be running ahead on this stream: it hands it back first)
        s->rs = &rs->r; s->rs_obj = rs;
        rs->attached.push_back(s); rs->forget = rstream_forget;
    }
    const int64_t N = s->N;
    hipStream_t st = h->stream;
    int rc = 0;
#define GP_A(p, cnt) do { rc = dalloc(s, &(p), (size_t)(cnt)); if (rc) { gpirt_sampler_destroy(s); return rc; } } while (0)
    GP_A(s->y, n * m);       GP_A(s->Ypm, n * 2 * m);  GP_A(s->theta, n);       GP_A(s->theta_new, n);
    s->tfd = tf_dims(n, m, N);
#define GP_AI(p, cnt) do { rc = dalloc(s, &(p), (size_t)(cnt), false); if (rc) { gpirt_sampler_destroy(s); return rc; } } while (0)
    GP_AI(s->tf_y8, tf_y8_bytes(s->tfd) / 8 + 2); GP_AI(s->tf_gq, tf_gq_bytes(s->tfd) / 8 + 2); GP_AI(s->tf_aux, tf_aux_bytes(s->tfd) / 8 + 2);
#undef GP_AI
    GP_A(s->f, n * m);       GP_A(s->Z, n * m);        GP_A(s->NU, n * (m > 1 + TRMV_SPLIT ? m : 1 + TRMV_SPLIT));   GP_A(s->beta, 2 * m);   // (NU: >= 1 + TRMV_SPLIT columns, launch_trmv_lower's parts)
    s->kr = s->opt.kstar_rank;
    if (s->kr != 0 && (!s->opt.fstar_fused || s->kr < 16 || s->kr > 128 || (s->kr % 16) != 0)) {
        set_error("kstar_rank must be a multiple of 16 in 16..128 and needs fstar_fused");
        gpirt_sampler_destroy(s);
        return GPIRT_E_ARG;
    }
    if (s->opt.factor_structured != 0 && s->opt.factor_structured != 1) {
        set_error("factor_structured must be 0 or 1");
        gpirt_sampler_destroy(s);
        return GPIRT_E_ARG;
    }
    const bool bordered_ok = (n % 64) == 0 && h->cfg.bordered != 2;
    if (bordered_ok) {
        // (the node rows of nu_lr.hip in every bordered layout: see node_off)
        if (s->kr == NU_LR_RANK) { s->ext = s->kr; s->node_off = 0; s->rank_off = 0; s->fstar_rows = true; }
        else if (s->kr > 0) { s->ext = NU_LR_RANK + s->kr; s->node_off = 0; s->rank_off = NU_LR_RANK; s->fstar_rows = true; }
        else if (n >= 1024) {
            s->node_off = (N + 63) / 64 * 64;     // 1001 grid rows + 23 rows that stay zero, then the node rows
            s->ext = s->node_off + NU_LR_RANK;
            s->ext_grid = true; s->fstar_rows = true;
        } else { s->ext = NU_LR_RANK; s->node_off = 0; }
    } else if ((n % 64) == 0) { s->ext = NU_LR_RANK; s->node_off = 0; }      // GPIRT_BORDERED=2: the node rows alone
    s->ldl = n + s->ext;
    s->theta_ok = true;
    for (int64_t i = 0; i < n; ++i) s->theta_ok = s->theta_ok && h_theta0[i] >= -5.0 && h_theta0[i] <= 5.0;
    s->nu_kern_ok = nu_kernel_ok(s->kern);
    GP_A(s->mu, n * m);      GP_A(s->mu_star, N * m + 1); GP_A(s->fstar, N * m + 1); GP_A(s->L, s->ldl * n);
    GP_A(s->tstar, N + 1);   GP_A(s->rhs, n * (N + m) + 2); GP_A(s->mean, N * m + 1); GP_A(s->s, N + 1);
    GP_A(s->Gpm, ((N + 127) / 128 * 128) * 2 * m + 2); GP_A(s->logpost, N * n + 2); GP_A(s->irf_sum, N * m + 1);
    // padding rows stay zero; cleared on the handle's stream (drained below) -- a null-stream hipMemset is not
    // ordered against a non-blocking stream
    if (hipMemsetAsync(s->Gpm, 0, sizeof(double) * (size_t)(((N + 127) / 128 * 128) * 2 * m + 2), st) != hipSuccess) {
        set_error("hipMemsetAsync(Gpm) failed"); gpirt_sampler_destroy(s); return GPIRT_E_HIP;
    }
    GP_A(s->pm, 2 * m);      GP_A(s->ps, 2 * m);       GP_A(s->step, 2 * m);
    GP_A(s->ess_k, m);       GP_A(s->flags, 4);
    if (!stream_mode(s) && ess_pack_eligible(n)) {       // (y as ess_kernel_lin reads it: 512 words per item)
        rc = dalloc(s, &s->ess_ypk, (size_t)(512 * m), false);
        if (rc) { gpirt_sampler_destroy(s); return rc; }
    }
    if (!s->opt.fstar_fused) GP_A(s->kstar, n * N + 2);
    if (s->node_off >= 0) {
        GP_A(s->nu_nodes, NU_LR_RANK); GP_A(s->nu_wts, NU_LR_RANK);
        if (!stream_mode(s)) {
            GP_A(s->nuV, n * NU_LR_RANK); GP_A(s->nuT, nu_lr_slabs(n) * NU_LR_RANK * m);
            // slab 0 of the product's workspace is the zero prefix of its first part: cleared once, behind any poison fill on the
            // same stream, and never written again (nu_lr.hip)
            if (hipMemsetAsync(s->nuT, 0, sizeof(double) * (size_t)(NU_LR_RANK * m), st) != hipSuccess) {
                set_error("hipMemsetAsync(nuT) failed"); gpirt_sampler_destroy(s); return GPIRT_E_HIP;
            }
        }
        if (!stream_mode(s) && s->kr == NU_LR_RANK && s->fstar_rows) {
            GP_A(s->ffF, FSTAR_FREE_RANK * FSTAR_FREE_RANK); GP_A(s->ffW, 2 * FSTAR_FREE_RANK * FSTAR_FREE_RANK);
            if (s->opt.factor_structured) {       // (the structured factor's: only where the rank-64 chain from theta can run)
                // one 64 x 64 slot per part of the narrowest width (G, Xh) and per pivot block (D: NU_LR_SUB_MIN = 64 columns each)
                const int64_t fp = factor_lr_parts(n, NU_LR_SUB_MIN) * NU_LR_RANK * NU_LR_RANK;
                GP_A(s->theta_L, n); GP_A(s->flrG, fp); GP_A(s->flrXh, fp); GP_A(s->flrX, NU_LR_RANK * n);
                GP_A(s->flrD, factor_lr_parts(n) * (NU_LR_PART / 64) * NU_LR_RANK * NU_LR_RANK);
            }
        }
    }
    if (s->kr != 0) {
        GP_A(s->knodes, s->kr); GP_A(s->kV, N * s->kr);
        GP_A(s->kparts, (size_t)KSPLIT * s->kr * (s->kr + m)); GP_A(s->kP, (size_t)s->kr * (s->kr + m));
    }
    if (stream_mode(s)) {
        // consumption of draw_beta per item: rnorm (2 unless step == 0) + runif (1), twice
        std::vector<uint64_t> off((size_t)m);
        uint64_t acc = 0;
        for (int64_t j = 0; j < m; ++j) {
            off[(size_t)j] = acc;
            for (int k = 0; k < 2; ++k) {
                const double sd = h_step[k + 2 * j];
                acc += ((sd > 0.0 && std::isfinite(sd)) ? 2 : 0) + 1;
            }
        }
        s->beta_total = acc;
        s->U_cap = stream_window(s);
        const uint64_t init_need = (uint64_t)m * 2 * (uint64_t)n + 4 * (uint64_t)m + 2 * (uint64_t)N * m + 64;
        if (init_need > s->U_cap) s->U_cap = init_need;
        GP_A(s->U, s->U_cap);       GP_A(s->U2, s->U_cap);      GP_A(s->S, s->U_cap);      GP_A(s->Sraw, s->U_cap);
        GP_A(s->pos, 2);
        // draw_f, three items per pass (rng_ess.hip)
        // The one-phase slice kernel MEETS: its work-groups (320 threads, ~30 KB of LDS) poll each other's flags, so all of
        // them must be resident at once -- at most one per compute unit is what the launch can count on beside foreign work.
        // (The predictor's decide kernel has no such need: a ticket, nobody waits for anybody.)  On a device with fewer
        // compute units than the grid the replay falls back to the item-by-item form.
        s->spec_ok = n >= RS_SPEC_MIN_N && n <= RS3_MAX_N && rs3_slice_wgs(n) <= h->n_cu;
        if (s->spec_ok) {
            const size_t parts = (size_t)((n + RS_KC - 1) / RS_KC);
            const size_t nrm = (size_t)s->U_cap + 8 * (size_t)n + 4096;       // (the predictor's products read up to 8n + 6 + 32 + 16 PD_MAXROUND + 40 past an anchor)
            GP_A(s->Lt, rs_tile_doubles(n));
            GP_A(s->posv, m + 1);    GP_A(s->anchor, 4);    GP_A(s->rs_trace, 128);
            hipMemsetAsync(s->rs_trace, 0, 128 * sizeof(long long), st);
            GP_A(s->rs_flags, 2 * RS3_MAX_WGS);    GP_A(s->rs_partial, 2 * RS3_MAX_WGS * (RS3_TRIALS + 1));
            hipMemsetAsync(s->rs_flags, 0, sizeof(unsigned long long) * 2 * RS3_MAX_WGS, st);
            GP_A(s->Nrm, nrm);       GP_A(s->rs_part, parts * RS3_CAND * (size_t)n);
            hipMemsetAsync(s->Nrm, 0, sizeof(double) * nrm, st);              // (positions no draw has filled are read, never used)
            hipMemsetAsync(s->rs_part, 0, sizeof(double) * parts * RS3_CAND * (size_t)n, st);
            hipMemsetAsync(s->anchor, 0, 4 * sizeof(uint64_t), st);
            const size_t partsP = (size_t)((n + RS3P_KC - 1) / RS3P_KC);
            GP_A(s->Lt32, rs32_tile_floats(n));   GP_A(s->rs_part32, partsP * RS3_CAND * (size_t)n);
            // (the octs right of a row group's diagonal are never written by rs32_tile_kernel, but the structured pass reads
            // its diagonal part whole: they must hold zeros from the start)
            hipMemsetAsync(s->Lt32, 0, sizeof(float) * rs32_tile_floats(n), st);
            GP_A(s->anchorP, 8);     GP_A(s->rs_ctl, 8);     GP_A(s->rs_posP, 2);
            GP_A(s->rs_dec_part, (size_t)RS3_CAND * 8 * 17 + 8);  GP_A(s->rs_dec_rec, (size_t)RS3_CAND * 20 + 8);  GP_A(s->rs_dec_ticket, 32 * 9);      // the top word + one per row part, 128 bytes apart
            hipMemsetAsync(s->rs_dec_ticket, 0, 32 * 9 * sizeof(unsigned), st);
            GP_A(s->rs_kpred, m);    GP_A(s->rs_kv, m);      GP_A(s->rs_used, m);     GP_A(s->rs_ierr, m);    GP_A(s->rs_errP, 4);
            hipMemsetAsync(s->rs_part32, 0, sizeof(float) * partsP * RS3_CAND * (size_t)n, st);
            hipMemsetAsync(s->anchorP, 0, 8 * sizeof(uint64_t), st);
            hipMemsetAsync(s->rs_ctl, 0, 8 * sizeof(uint64_t), st);
            hipMemsetAsync(s->rs_errP, 0, 4 * sizeof(int), st);
            std::vector<uint32_t> units;
            rs3_unit_table(n, units, &s->rs_nfull);
            s->rs_nunits = (int)units.size();
            GP_A(s->rs_units, units.size());
            hipMemcpyAsync(s->rs_units, units.data(), units.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
            std::vector<uint32_t> unitsP;
            rs3p_unit_table(n, unitsP, &s->rs_nfullP);
            s->rs_nunitsP = (int)unitsP.size();
            GP_A(s->rs_unitsP, unitsP.size());
            hipMemcpyAsync(s->rs_unitsP, unitsP.data(), unitsP.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
            // the structured form of the predictor's pass (rs_lr.hip): from 4096 rows on (below, a pass over L is a few MB anyway: 2048 x 256 runs at 270 it/s with it, 298 without),
            // not with the single-precision kernel build (S then is not the kernel the basis represents, to 6e-8),
            // and only under the default kernel: rs_lr.hip builds its rank-64 basis from the unit squared exponential
            // (rs_lr_nodes' K(c, c), the setup kernel's K(theta, c)), which says nothing about any other S.  With another kernel the
            // dense predictor runs -- it reads only the fp32 copy of L.  The draws are the same either way: phase B verifies.
            s->lr_on = h->cfg.rs_lr != 2 && n >= 4096 && !s->opt.kernel_fp32 && s->kern.is_default();
            std::vector<uint32_t> unitsL;
            if (s->lr_on) {
                std::vector<double> nodes, wts, Mn;
                rs_lr_nodes(nodes, wts, Mn);
                const size_t nb = (size_t)((n + 63) / 64), lparts = (size_t)((n + RS3P_KC - 1) / RS3P_KC);
                GP_A(s->lr_nodes, RS_LR_RANK);  GP_A(s->lr_wts, RS_LR_RANK);  GP_A(s->lr_M, RS_LR_RANK * RS_LR_RANK);
                GP_A(s->lr_V64, nb * 64 * RS_LR_RANK);  GP_A(s->lr_Gb, nb * RS_LR_RANK * RS_LR_RANK);
                GP_A(s->lr_V32t, (size_t)RS_LR_RANK * (size_t)n);  GP_A(s->lr_Ct32, (size_t)(RS_LR_RANK / RS_ROWS) * (size_t)rs32_tile_octs(n) * 256);
                GP_A(s->lr_Y, lparts * RS3_CAND * RS_LR_RANK);  GP_A(s->lr_bad, 4);
                hipMemcpyAsync(s->lr_nodes, nodes.data(), sizeof(double) * RS_LR_RANK, hipMemcpyHostToDevice, st);
                hipMemcpyAsync(s->lr_wts, wts.data(), sizeof(double) * RS_LR_RANK, hipMemcpyHostToDevice, st);
                hipMemcpyAsync(s->lr_M, Mn.data(), sizeof(double) * RS_LR_RANK * RS_LR_RANK, hipMemcpyHostToDevice, st);
                hipMemsetAsync(s->lr_Ct32, 0, sizeof(float) * (size_t)(RS_LR_RANK / RS_ROWS) * (size_t)rs32_tile_octs(n) * 256, st);
                hipMemsetAsync(s->lr_Y, 0, sizeof(float) * lparts * RS3_CAND * RS_LR_RANK, st);
                hipMemsetAsync(s->lr_bad, 0, 4 * sizeof(int), st);
                rs_lr_unit_table(n, unitsL);
                s->lr_nunits = (int)unitsL.size();
                GP_A(s->lr_units, unitsL.size());
                hipMemcpyAsync(s->lr_units, unitsL.data(), unitsL.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
            }
            hipStreamSynchronize(st);                                          // (unitsP, unitsL leave scope with units below)
            hipStreamSynchronize(st);                                          // (units leaves scope)
        }
        GP_A(s->beta_off, m);
        GP_A(s->fstar_off, N + 8);
        if (hipHostMalloc(&s->hU, s->U_cap * sizeof(double), hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&s->hA, s->U_cap * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&s->h_pos, 2 * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess ||
            hipStreamCreateWithFlags(&s->cs, hipStreamNonBlocking) != hipSuccess ||
            hipHostMalloc(&s->h_next, 8 * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev_up, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev_asm, hipEventDisableTiming) != hipSuccess) {
            set_error("pinned allocation for the R-stream window failed");
            gpirt_sampler_destroy(s);
            return GPIRT_E_ALLOC;
        }
        hipMemcpyAsync(s->beta_off, off.data(), sizeof(uint64_t) * (size_t)m, hipMemcpyHostToDevice, st);
        hipStreamSynchronize(st);
    }
#undef GP_A
    if (hipHostMalloc(&s->h_flags, 4 * sizeof(int), hipHostMallocDefault) != hipSuccess) {
        set_error("pinned allocation failed"); gpirt_sampler_destroy(s); return GPIRT_E_ALLOC;
    }
    for (int i = 0; i <= ST_COUNT; ++i) hipEventCreate(&s->ev[i]);
    // uploads (host buffers are caller-owned and never modified: R semantics)
    std::vector<double> ts((size_t)N);
    for (int64_t i = 0; i < N; ++i) ts[(size_t)i] = -5.0 + (double)i * 0.01;   // src/gpirtMCMC.cpp:35
    hipMemcpyAsync(s->y, h_y, sizeof(double) * (size_t)(n * m), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(s->theta, h_theta0, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st);
    hipMemcpyAsync(s->pm, h_pm, sizeof(double) * (size_t)(2 * m), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(s->ps, h_ps, sizeof(double) * (size_t)(2 * m), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(s->step, h_step, sizeof(double) * (size_t)(2 * m), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(s->tstar, ts.data(), sizeof(double) * (size_t)N, hipMemcpyHostToDevice, st);
    std::vector<double> nodes, V;
    if (s->kr > 0) {
        // Chebyshev interpolation of  t -> exp(-(theta - t)^2 / 2)  on the grid's interval [-5, 5]:
        //   K(theta_i, t_j) = sum_k K(theta_i, c_k) V[j][k],  V = barycentric Lagrange basis at the r first-kind
        // Chebyshev points c_k, evaluated at the 1001 grid points in long double.  The integrand is entire and
        // the interval is 10 length-scales wide: r = 56 already reaches 1.3e-15 max-abs error (Lebesgue
        // constant 3.6), so K*^T (n x 1001) is replaced by its exact rank-r factorisation U V^T, U = K(theta, c).
        // Neither the nodes nor V depend on the kernel; the error does (a shorter length scale needs a higher rank, a Matern
        // kernel has no such form): gpirt_kernel_check's certificate, applied above, is computed from this same V.
        const int r = s->kr;
        cheb_nodes_basis(r, nodes, V);                                     // (se_kernel.hip)
        hipMemcpyAsync(s->knodes, nodes.data(), sizeof(double) * (size_t)r, hipMemcpyHostToDevice, st);
        hipMemcpyAsync(s->kV, V.data(), sizeof(double) * (size_t)(N * r), hipMemcpyHostToDevice, st);
    }
    if (s->node_off >= 0) {
        std::vector<double> nnodes, wts;
        nu_lr_nodes(nnodes, wts);                                           // (cheb_nodes_basis(64): with kr == 64, knodes' values)
        hipMemcpyAsync(s->nu_nodes, nnodes.data(), sizeof(double) * NU_LR_RANK, hipMemcpyHostToDevice, st);
        hipMemcpyAsync(s->nu_wts, wts.data(), sizeof(double) * NU_LR_RANK, hipMemcpyHostToDevice, st);
        hipStreamSynchronize(st);                                          // (nnodes, wts leave scope)
    }
    hipMemsetAsync(s->L, 0, sizeof(double) * (size_t)(s->ldl * n), st);    // strict upper stays zero
    hipMemsetAsync(s->irf_sum, 0, sizeof(double) * (size_t)(N * m), st);   // :42
    hipMemsetAsync(s->flags, 0, 4 * sizeof(int), st);
    hipMemsetAsync(s->ess_k, 0, sizeof(int) * (size_t)m, st);
    launch_indicators(st, s->y, n, m, s->Ypm);
    launch_tf_indicators(st, s->y, n, n, m, s->tfd, s->tf_y8);
    if (s->ess_ypk) { launch_ess_pack(st, s->y, n, m, s->ess_ypk); s->ess_ypk_valid = true; }
    if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
        set_error("sampler upload failed"); gpirt_sampler_destroy(s); return GPIRT_E_HIP;
    }
    if (fstar_free_setup(s) != 0) { gpirt_sampler_destroy(s); return GPIRT_E_HIP; }
    if (!stream_mode(s)) {
        if (!h->aux) {
            if (create_side_handle(&h->aux, h->device) != 0) { gpirt_sampler_destroy(s); return GPIRT_E_HIP; }
            h->aux->cfg = h->cfg;
        }
        s->haux = h->aux;
        s->haux->poison_allocs = h->poison_allocs;       // (gpirt_debug_poison_allocs: the side handle's workspaces too)
        if (
            hipEventCreateWithFlags(&s->ev_trmm, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev_prep, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev_zfill, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev_flr, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&s->ev_beta, hipEventDisableTiming) != hipSuccess) {
            gpirt_sampler_destroy(s);
            return GPIRT_E_HIP;
        }
    }
    // keep pm/ps on the host for the R-stream init of beta
    s->host_tmp.assign(h_pm, h_pm + 2 * m);
    s->host_tmp.insert(s->host_tmp.end(), h_ps, h_ps + 2 * m);
    h->live_samplers += 1;
    s->counted = true;
    *out = s;
    return 0;
}

int gpirt_sampler_destroy(gpirt_sampler_t s)
{
    if (!s) return 0;
    if (s->h) hipStreamSynchronize(s->h->stream);
    if (s->rs_obj && s->rs_obj->owner == s) ahead_resolve(s, false);     // the caller's generator goes back to the consumed position
    if (s->rs_obj) {
        auto& at = s->rs_obj->attached;
        for (size_t q = 0; q < at.size(); ++q) if (at[q] == s) { at.erase(at.begin() + (std::ptrdiff_t)q); break; }
    }
    if (s->cs) { hipStreamSynchronize(s->cs); hipStreamDestroy(s->cs); }
    if (s->h_next) hipHostFree(s->h_next);
    if (s->ev_up) hipEventDestroy(s->ev_up);
    if (s->ev_asm) hipEventDestroy(s->ev_asm);
    if (s->hA) hipHostFree(s->hA);
    if (s->haux) {
        hipStreamSynchronize(s->haux->stream);       // (the side handle belongs to the main handle: not destroyed here)
        if (s->haux->trsm_winv_L == s->L) s->haux->trsm_winv_L = nullptr;
        if (s->haux->inv_partial_L == s->L) { s->haux->inv_partial_L = nullptr; s->haux->inv_partial_pairs = 0; }
    }
    if (s->h && s->h->trsm_winv_L == s->L) s->h->trsm_winv_L = nullptr;
    if (s->ev_trmm) hipEventDestroy(s->ev_trmm);
    if (s->ev_prep) hipEventDestroy(s->ev_prep);
    if (s->ev_zfill) hipEventDestroy(s->ev_zfill);
    if (s->ev_flr) hipEventDestroy(s->ev_flr);
    if (s->ev_beta) hipEventDestroy(s->ev_beta);
    for (void* p : s->allocs) hipFree(p);
    summary_free(&s->sum);
    ppc_free(&s->ppc);
    rank_free(&s->rank);
    shape_free(&s->shape);
    sumscore_free(&s->sumscore);
    equate_free(&s->equate);
    loo_free(&s->loo);
    acf_free(&s->acf);
    groups_free(&s->groups);
    score_free(&s->score);
    ell_free(&s->ell);
    amp_free(&s->amp);
    pop_free(&s->pop);
    ord_free(&s->ord);
    for (hipEvent_t t : s->carry.tev) if (t) hipEventDestroy(t);      // (its two buffers are in `allocs`)
    for (hipEvent_t t : s->bc.tev) if (t) hipEventDestroy(t);         // (its buffer and the smooth part's F are in `allocs`)
    for (hipEvent_t t : s->sc.tev) if (t) hipEventDestroy(t);         // (the scale move's buffers are in `allocs`)
    if (s->hU) hipHostFree(s->hU);
    if (s->h_pos) hipHostFree(s->h_pos);
    if (s->h_flags) hipHostFree(s->h_flags);
    for (int i = 0; i <= ST_COUNT; ++i) if (s->ev[i]) hipEventDestroy(s->ev[i]);
    gpirt_handle_t h = s->h;
    const bool counted = s->counted;
    delete s;
    if (h && counted) {
        h->live_samplers -= 1;
        if (h->zombie && h->live_samplers == 0) { h->zombie = false; gpirt_destroy(h); }    // the handle outlived by its samplers
    }
    return 0;
}

// src/gpirtMCMC.cpp:13-47
int gpirt_sampler_init(gpirt_sampler_t s)
{
    GP_ARG(s != nullptr);
    gpirt_handle_t h = s->h;
    hipStream_t st = h->stream;
    const int64_t n = s->n, m = s->m, N = s->N;
    GP_TRY(aux_join(s));                  // (a repeated init: nothing of the previous chain may still be in flight)
    if (stream_mode(s)) {
        if (!s->rs) { set_error("the R stream of this sampler has been destroyed"); return GPIRT_E_ARG; }
        rstream_sync(s->rs_obj);          // init draws from the generator directly: from the consumed position
    }
    s->in_init = true;
    const int rc_f = do_factor(s);                                                // :15-17
    s->in_init = false;
    GP_TRY(rc_f);
    GP_TRY(factor_guard_sync(s));         // (init drains the stream below anyway)
    if (!stream_mode(s)) {
        GP_TRY(launch_item_uniforms(st, s->opt.seed, 0, GPIRT_ST_INIT_F, (uint32_t)s->opt.item0, m, n, s->Z, true, s->h->cfg.zfill_compact == 1));
        GP_TRY(launch_gemm(h, st, false, false, TRI_A_LOWER, n, m, n, 1.0, s->L, s->ldl, s->Z, n, 0.0, s->f, n)); // :18-21
        // beta(p, j) = R::rnorm(prior_mean, prior_sd), index = p                    :22-27
        std::vector<double> b((size_t)(2 * m));
        const double* pm = s->host_tmp.data();
        const double* ps = pm + 2 * m;
        for (int64_t j = 0; j < m; ++j)
            for (int p = 0; p < 2; ++p) {
                const double mu = pm[p + 2 * j], sd = ps[p + 2 * j];
                double v;
                if (mu != mu || !std::isfinite(sd) || sd < 0.0) v = NAN;
                else if (sd == 0.0 || !std::isfinite(mu)) v = mu;
                else v = mu + sd * qnorm_as241(item_uniform(s->opt.seed, 0, GPIRT_ST_INIT_BETA,
                                                            (uint32_t)(s->opt.item0 + j), (uint32_t)p));
                b[(size_t)(p + 2 * j)] = v;
            }
        GP_HIP(hipMemcpyAsync(s->beta, b.data(), sizeof(double) * b.size(), hipMemcpyHostToDevice, st));
        GP_HIP(hipStreamSynchronize(st));
    } else {
        // window layout: [f init: m x 2n][beta init: <= 4m][fstar: 2 N m]
        const uint64_t nf = (uint64_t)m * 2 * (uint64_t)n;
        // beta consumes on the host, directly behind the f-init block
        s->saved = *s->rs;
        s->rs->fill_unif(s->hU, nf);
        std::vector<double> b((size_t)(2 * m));
        const double* pm = s->host_tmp.data();
        const double* ps = pm + 2 * m;
        uint64_t nb = 0;
        for (int64_t j = 0; j < m; ++j)
            for (int p = 0; p < 2; ++p) {
                const double mu = pm[p + 2 * j], sd = ps[p + 2 * j];
                double v;
                if (mu != mu || !std::isfinite(sd) || sd < 0.0) v = NAN;
                else if (sd == 0.0 || !std::isfinite(mu)) v = mu;
                else { v = mu + sd * s->rs->norm(); nb += 2; }
                b[(size_t)(p + 2 * j)] = v;
            }
        const uint64_t nfs = 2 * (uint64_t)N * (uint64_t)m;
        s->rs->fill_unif(s->hU + nf, nfs);
        (void)nb;
        GP_HIP(hipMemcpyAsync(s->U, s->hU, (nf + nfs) * sizeof(double), hipMemcpyHostToDevice, st));
        GP_HIP(hipMemsetAsync(s->pos, 0, sizeof(uint64_t), st));
        GP_TRY(launch_rstream_normals(st, s->U, s->pos, 2 * n, n, m, s->Z));
        GP_TRY(launch_gemm(h, st, false, false, TRI_A_LOWER, n, m, n, 1.0, s->L, s->ldl, s->Z, n, 0.0, s->f, n));
        GP_TRY(launch_advance_pos(st, s->pos, nf));
        GP_HIP(hipMemcpyAsync(s->beta, b.data(), sizeof(double) * b.size(), hipMemcpyHostToDevice, st));
        GP_HIP(hipStreamSynchronize(st));
    }
    GP_TRY(launch_linear_mean(st, s->theta, n, s->beta, m, s->mu));               // :30-33
    s->mu_linear = true;
    GP_TRY(launch_linear_mean(st, s->tstar, N, s->beta, m, s->mu_star));          // :37-40
    GP_TRY(do_draw_fstar(s, 0));                                                  // :41
    if (stream_mode(s)) {
        // the fstar block may have consumed fewer than 2 N m uniforms (s_i <= 0): rewind exactly
        GP_HIP(hipMemcpyAsync(s->h_pos, s->pos, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        const uint64_t nf = (uint64_t)m * 2 * (uint64_t)n;
        const uint64_t used_fstar = *s->h_pos - nf;
        // host state currently sits after [f][beta][2Nm]; recompute: after [f][beta] + used_fstar
        RStream r = s->saved;
        r.skip(nf);
        const double* pm = s->host_tmp.data();
        const double* ps = pm + 2 * m;
        for (int64_t j = 0; j < m; ++j)
            for (int p = 0; p < 2; ++p) {
                const double mu = pm[p + 2 * j], sd = ps[p + 2 * j];
                if (!(mu != mu || !std::isfinite(sd) || sd < 0.0) && !(sd == 0.0 || !std::isfinite(mu))) {
                    (void)r.next32(); (void)r.next32();
                }
            }
        r.skip(used_fstar);
        *s->rs = r;
    }
    s->iter = 0;
    s->initialised = true;
    return 0;
}

int gpirt_sampler_draw_f(gpirt_sampler_t s) { GP_ARG(s && s->initialised); return do_draw_f(s); }
int gpirt_sampler_draw_fstar(gpirt_sampler_t s) { GP_ARG(s && s->initialised); return do_draw_fstar(s, (uint32_t)(s->iter + 1)); }
int gpirt_sampler_theta_partial(gpirt_sampler_t s) { GP_ARG(s && s->initialised); return do_theta_partial(s); }
int gpirt_sampler_theta_finish(gpirt_sampler_t s) { GP_ARG(s && s->initialised); return do_theta_finish(s); }

int gpirt_sampler_set_theta_block(gpirt_sampler_t s, const double* y_block, int64_t i0, int64_t n_block, int64_t m_total)
{
    GP_ARG(s && (y_block || n_block == 0) && i0 >= 0 && n_block >= 0 && i0 + n_block <= s->n && m_total >= s->m);
    if (stream_mode(s)) { set_error("the R-stream replay cannot be sharded"); return GPIRT_E_ARG; }
    if (s->fstar_full) { set_error("the theta block is already set"); return GPIRT_E_ARG; }
    GP_TRY(ord_refuse(s, "gpirt_sampler_set_theta_block", "the respondent-block theta path has no one-hot product"));
    if (s->pop.mode) {
        set_error("gpirt_sampler_set_theta_block is refused while a population prior is on: the block path would need the codes of its respondents");
        return GPIRT_E_ARG;
    }
    const int64_t N = s->N, Np = (N + 127) / 128 * 128;
    int rc = 0;
    double* yb = nullptr;
#define GP_B(p, cnt) do { rc = dalloc(s, &(p), (size_t)(cnt)); if (rc) return rc; } while (0)
    GP_B(s->Ypm_blk, n_block * 2 * m_total + 2); GP_B(s->Gpm_full, Np * 2 * m_total + 2);
    GP_B(s->logpost_blk, N * n_block + 2);       GP_B(s->fstar_full, N * m_total + 2);
    GP_B(s->theta_stage, s->n + 1);              GP_B(yb, n_block * m_total + 1);
    s->tfd_blk = tf_dims(n_block, m_total, N);
#undef GP_B
#define GP_B(p, cnt) do { rc = dalloc(s, &(p), (size_t)(cnt), false); if (rc) return rc; } while (0)
    GP_B(s->tf_y8_blk, tf_y8_bytes(s->tfd_blk) / 8 + 2); GP_B(s->tf_gq_blk, tf_gq_bytes(s->tfd_blk) / 8 + 2);
    GP_B(s->tf_aux_blk, tf_aux_bytes(s->tfd_blk) / 8 + 2);
#undef GP_B
    hipStream_t st = s->h->stream;
    GP_HIP(hipMemsetAsync(s->Gpm_full, 0, sizeof(double) * (size_t)(Np * 2 * m_total + 2), st));   // padding rows stay zero
    if (n_block > 0) {
        GP_HIP(hipMemcpyAsync(yb, y_block, sizeof(double) * (size_t)(n_block * m_total), hipMemcpyHostToDevice, st));
        GP_TRY(launch_indicators(st, yb, n_block, m_total, s->Ypm_blk));
        GP_TRY(launch_tf_indicators(st, yb, n_block, n_block, m_total, s->tfd_blk, s->tf_y8_blk));
    }
    GP_HIP(hipStreamSynchronize(st));
    s->blk_i0 = i0; s->blk_n = n_block; s->blk_m = m_total;
    return 0;
}

int gpirt_sampler_theta_block(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    if (!s->fstar_full) { set_error("gpirt_sampler_set_theta_block has not been called"); return GPIRT_E_ARG; }
    return do_theta_block(s);
}

/* theta := the staged draw (after the blocks of all ranks have been summed into "theta_stage") */
int gpirt_sampler_theta_commit(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised && s->theta_stage);
    GP_HIP(hipMemcpyAsync(s->theta, s->theta_stage, sizeof(double) * (size_t)s->n, hipMemcpyDeviceToDevice, s->h->stream));
    s->lp_current = false;
    s->mu_linear = false;
    s->theta_ok = true;                   // the ranks' blocks of grid values, summed
    return 0;
}
int gpirt_sampler_draw_beta(gpirt_sampler_t s) { GP_ARG(s && s->initialised); return do_draw_beta(s); }
int gpirt_sampler_factor(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    GP_TRY(do_factor(s));
    s->iter += 1;            // the factorisation closes an iteration (src/gpirtMCMC.cpp:78,97)
    return 0;
}

int gpirt_sampler_build_cov(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    hipStream_t st = s->h->stream;
    if (!s->sticky_info) GP_HIP(hipMemsetAsync(s->h->d_info, 0, sizeof(int), st));
    GP_TRY(aux_join(s));
    invalidate_factor_products(s);
    return build_cov(s);                                                                                   // :76-77
}

// L arrived from elsewhere (a broadcast, the distributed pieces, gpirt_sampler_set): closes the iteration without
// factoring.  rows_with_L says whether the rows below the n x n factor (bordered layout, gpirt_sampler_ldl) arrived
// with it -- the WHOLE ldl x n buffer was received, as gpirt_amd/distributed.py does.  If not (a host that moved only
// the n x n factor), they still belong to the previous (theta, L) and are rebuilt by the explicit forward solve before
// draw_fstar reads them.
int gpirt_sampler_adopt_factor(gpirt_sampler_t s, int rows_with_L)
{
    GP_ARG(s && s->initialised);
    GP_TRY(beta_sync(s));                // a held-back draw_beta belongs to the iteration that closes here
    invalidate_factor_products(s);
    s->L_structured = false;             // (L was overwritten from outside)
    s->factor_fresh = false;             // (nothing here could rebuild a factor that arrived from elsewhere)
    s->rows_valid = rows_with_L != 0;
    s->theta_alone = false;
    s->iter += 1;
    return 0;
}

int gpirt_sampler_skip_factor(gpirt_sampler_t s) { return gpirt_sampler_adopt_factor(s, 0); }

int gpirt_sampler_step(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    if (stream_mode(s)) GP_TRY(stream_begin(s, stream_window(s)));
    mark(s, 0);
    GP_TRY(do_draw_f(s));            mark(s, 1);
    GP_TRY(do_draw_fstar(s, (uint32_t)(s->iter + 1))); mark(s, 2);
    GP_TRY(do_theta_partial(s));     mark(s, 3);
    GP_TRY(do_theta_finish(s));      mark(s, 4);
    GP_TRY(do_draw_beta(s));         mark(s, 5);
    GP_TRY(do_factor(s));            mark(s, 6);
    s->iter += 1;
    if (stream_mode(s)) GP_TRY(stream_end(s, stream_window(s)));
    if (s->timing) {
        GP_HIP(hipEventSynchronize(s->ev[ST_COUNT]));
        for (int i = 0; i < ST_COUNT; ++i) {
            float ms = 0.f;
            hipEventElapsedTime(&ms, s->ev[i], s->ev[i + 1]);
            s->stage_ms[i] = ms;
        }
    }
    return 0;
}

// ---- the consistent step (include/gpirt_hip.h, "a consistent step"; carry.hip) -------------------------------------------------
int gpirt_sampler_carry_f(gpirt_sampler_t s, int nugget)
{
    GP_ARG(s != nullptr);
    GP_TRY(carry_refusals(s, nugget, "gpirt_sampler_carry_f"));
    const bool timed = s->timing;
    GP_TRY(do_carry_f(s, nugget, timed));
    if (timed) {                              // (timing on: one synchronisation, as the amplitude update's)
        GP_HIP(hipEventSynchronize(s->carry.tev[1]));
        float ms = 0.f;
        hipEventElapsedTime(&ms, s->carry.tev[0], s->carry.tev[1]);
        s->carry.last_ms = ms;
    }
    return 0;
}

// gpirt_sampler_step with the carry between theta_finish and draw_beta: the same marks, the carry between its own two events
int gpirt_sampler_step_consistent(gpirt_sampler_t s, int nugget)
{
    GP_ARG(s != nullptr);
    GP_TRY(carry_refusals(s, nugget, "gpirt_sampler_step_consistent"));
    mark(s, 0);
    GP_TRY(do_draw_f(s));            mark(s, 1);
    GP_TRY(do_draw_fstar(s, (uint32_t)(s->iter + 1))); mark(s, 2);
    GP_TRY(do_theta_partial(s));     mark(s, 3);
    GP_TRY(do_theta_finish(s));      mark(s, 4);
    GP_TRY(do_carry_f(s, nugget, s->timing));
    GP_TRY(do_draw_beta(s));         mark(s, 5);
    GP_TRY(do_factor(s));            mark(s, 6);
    s->iter += 1;
    if (s->timing) {
        GP_HIP(hipEventSynchronize(s->ev[ST_COUNT]));
        for (int i = 0; i < ST_COUNT; ++i) {
            float ms = 0.f;
            // (draw_beta's time starts behind the carry, whose own is the seventh: gpirt_carry.last_ms)
            hipEventElapsedTime(&ms, i == ST_BETA ? s->carry.tev[1] : s->ev[i], s->ev[i + 1]);
            s->stage_ms[i] = ms;
        }
        float ms = 0.f;
        hipEventElapsedTime(&ms, s->carry.tev[0], s->carry.tev[1]);
        s->carry.last_ms = ms;
    }
    return 0;
}

int gpirt_sampler_carry_stats(gpirt_sampler_t s, gpirt_carry* out)
{
    GP_ARG(s && out);
    const CarryState& c = s->carry;
    memset(out, 0, sizeof(*out));
    out->calls = c.calls; out->last_ms = c.last_ms;
    if (!c.counters) return 0;
    unsigned long long w[6];
    GP_HIP(hipMemcpyAsync(w, c.counters, sizeof(w), hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    const int last = 2 + 2 * (int)((c.calls - 1) & 1);
    out->total_off_grid = (int64_t)w[0]; out->total_nonfinite = (int64_t)w[1];
    out->off_grid = (int64_t)w[last]; out->nonfinite = (int64_t)w[last + 1];
    return 0;
}

// q_j = || L^-1 f_j ||^2: the forward solve of the centred length-scale update's first half into NU (free between steps), then
// one reduction.  Nothing of the chain moves; a structured factor is replaced by the dense one first.
int gpirt_sampler_prior_quad(gpirt_sampler_t s, double* h_q)
{
    GP_ARG(s && h_q);
    if (!s->initialised) { set_error("gpirt_sampler_prior_quad needs an initialised sampler (gpirt_sampler_init)"); return GPIRT_E_ARG; }
    gpirt_handle_t h = s->h;
    hipStream_t st = h->stream;
    const int64_t n = s->n, m = s->m;
    GP_TRY(ell_settle_factor(s));             // (a factor nobody has looked at yet: its info words read, an expired guard repaired)
    GP_TRY(aux_join(s, true, false));         // (a held-back draw_beta runs now; a prefilled Z is kept: nothing here touches it)
    GP_TRY(ensure_dense_factor(s));           // (the solve goes through all of L)
    s->factor_fresh = false;
    if (!s->carry.quad) GP_TRY(dalloc(s, &s->carry.quad, (size_t)m));
    GP_HIP(hipMemcpyAsync(s->NU, s->f, sizeof(double) * (size_t)(n * m), hipMemcpyDeviceToDevice, st));
    GP_TRY(launch_trsm_lower(h, st, s->L, n, s->ldl, s->NU, m, n, false));
    GP_TRY(launch_prior_quad(st, s->NU, n, m, s->carry.quad));
    GP_HIP(hipMemcpyAsync(h_q, s->carry.quad, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

int gpirt_sampler_accumulate_irf(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    return launch_axpy_irf(s->h->stream, s->irf_sum, s->fstar, s->N * s->m);     // :103
}

// ---- posterior summaries (summary.hip) on the stage API ---------------------------------------------------------------
int gpirt_sampler_summary_enable(gpirt_sampler_t s, int parts)
{
    GP_ARG(s && s->initialised);
    GP_ARG((parts & ~(GPIRT_SUM_THETA_BETA | GPIRT_SUM_F | GPIRT_SUM_PRED | GPIRT_SUM_WAIC | GPIRT_SUM_THETA_HIST |
                      GPIRT_SUM_IRF_BAND)) == 0);
    return gpirt_sampler_summary_enable_planned(s, parts, 0);
}

int gpirt_sampler_summary_enable_planned(gpirt_sampler_t s, int parts, int64_t planned_draws)
{
    GP_ARG(s && s->initialised);
    if (parts & (GPIRT_SUM_PRED | GPIRT_SUM_WAIC)) GP_TRY(ord_refuse(s, "gpirt_sampler_summary_enable_planned", "its WAIC and pred parts evaluate the binary likelihood of y"));
    GP_ARG((parts & ~(GPIRT_SUM_THETA_BETA | GPIRT_SUM_F | GPIRT_SUM_PRED | GPIRT_SUM_WAIC | GPIRT_SUM_DIAG |
                      GPIRT_SUM_THETA_HIST | GPIRT_SUM_IRF_BAND)) == 0);
    GP_ARG(planned_draws >= 0 && (!(parts & GPIRT_SUM_DIAG) || planned_draws >= 1));
    GP_HIP(hipStreamSynchronize(s->h->stream));        // a summary kernel still running on the old accumulators
    summary_free(&s->sum);
    if (parts == 0) return 0;
    const int rc = summary_alloc(&s->sum, s->n, s->m, parts | GPIRT_SUM_THETA_BETA, planned_draws);
    if (rc) summary_free(&s->sum);
    return rc;
}

int gpirt_summary_state_bytes(int64_t n, int64_t m, int parts, int64_t* bytes)
{
    GP_ARG(n > 0 && m > 0 && bytes);
    GP_ARG((parts & ~(GPIRT_SUM_THETA_BETA | GPIRT_SUM_F | GPIRT_SUM_PRED | GPIRT_SUM_WAIC | GPIRT_SUM_DIAG |
                      GPIRT_SUM_THETA_HIST | GPIRT_SUM_IRF_BAND)) == 0);
    *bytes = quantile_layout(n, m, parts | GPIRT_SUM_THETA_BETA).total * (int64_t)sizeof(double);
    return 0;
}

int gpirt_sampler_summary_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    GP_ARG(s && d_state && bytes);
    if (!s->sum.parts) { set_error("summaries are not enabled (gpirt_sampler_summary_enable)"); return GPIRT_E_ARG; }
    GP_TRY(summary_seal(s->h->stream, &s->sum, s->irf_sum, s->N));
    *d_state = s->sum.block;
    *bytes = s->sum.qlay.total * (int64_t)sizeof(double);
    return 0;
}

int gpirt_sampler_summary_accumulate(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    if (!s->sum.parts) { set_error("summaries are not enabled (gpirt_sampler_summary_enable)"); return GPIRT_E_ARG; }
    GP_TRY(beta_sync(s));                     // draw_beta (beta, mu) may still be deferred to the sampler's own stream
    return acc_summary(s, live_view(s));
}

int gpirt_sampler_summary_get(gpirt_sampler_t s, const char* name, double* h_out, int64_t count)
{
    GP_ARG(s && name && h_out && count >= 0);
    if (!s->sum.parts) { set_error("summaries are not enabled (gpirt_sampler_summary_enable)"); return GPIRT_E_ARG; }
    bool hist = false;
    GP_TRY(summary_hist_get(s->h->stream, &s->sum, name, h_out, count, &hist));
    if (hist) return 0;
    double* d = nullptr; int64_t c = 0;
    GP_TRY(launch_summary_finish(s->h->stream, &s->sum, name, s->y, &d, &c));
    GP_ARG(count <= c);
    GP_HIP(hipMemcpyAsync(h_out, d, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

int gpirt_sampler_summary_totals(gpirt_sampler_t s, double* h_totals)
{
    GP_ARG(s && h_totals);
    if (!s->sum.parts) { set_error("summaries are not enabled (gpirt_sampler_summary_enable)"); return GPIRT_E_ARG; }
    GP_TRY(launch_summary_totals(s->h->stream, &s->sum, s->y));
    GP_HIP(hipMemcpyAsync(h_totals, s->sum.tot, sizeof(double) * GPIRT_SUM_NTOTALS, hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

// ---- posterior predictive checks (ppc.hip) on the stage API -----------------------------------------------------------
int gpirt_sampler_ppc_enable(gpirt_sampler_t s, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_ppc_enable", ORD_BINARY));
    return stage_enable(s, &s->ppc, ppc_free, on, [&] { return ppc_alloc(s->h->stream, &s->ppc, s->n, s->m, s->opt.item0, s->y); });
}

int gpirt_sampler_ppc_accumulate(gpirt_sampler_t s) { return stage_accumulate(s, blk_ppc, acc_ppc, true); }

int gpirt_sampler_ppc_get(gpirt_sampler_t s, const char* name, double* h_out, int64_t count)
{
    GP_ARG(s && name && h_out && count >= 0);
    GP_TRY(needs(blk_ppc(s)));
    const bool item = strncmp(name, "item_", 5) == 0, resp = strncmp(name, "respondent_", 11) == 0;
    const int fld = item ? ppc_field_index(name + 5) : resp ? ppc_field_index(name + 11) : -1;
    if (fld < 0) { set_error("unknown PPC field '%s'", name); return GPIRT_E_ARG; }
    GP_ARG(count <= (item ? s->m : s->n));
    std::vector<uint64_t> host;
    GP_TRY(ppc_fetch(s->h->stream, &s->ppc, host));
    ppc_fill(host.data(), fld, resp, h_out, count);
    return 0;
}

int gpirt_sampler_ppc_totals(gpirt_sampler_t s, double* h_totals)
{
    GP_ARG(s && h_totals);
    GP_TRY(needs(blk_ppc(s)));
    std::vector<uint64_t> host;
    GP_TRY(ppc_fetch(s->h->stream, &s->ppc, host));
    ppc_fill_totals(host.data(), h_totals);
    return 0;
}

int gpirt_sampler_ppc_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_ppc, ppc_state_words, d_state, bytes, ppc_seal);
}

int gpirt_ppc_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc* out)
{
    return ppc_combine(h, chains, d_states, out);
}

// ---- pairwise item checks (ppc_pairs.hip): an add-on to the PPC state ----------------------------------------------------
int gpirt_sampler_ppc_pairs_enable(gpirt_sampler_t s, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_ppc_pairs_enable", ORD_BINARY));
    return stage_enable(s, &s->ppc.pairs, pair_free, on, [&]() -> int {
        GP_TRY(needs(blk_ppc(s)));
        return pair_alloc(s->h->stream, &s->ppc.pairs, s->n, s->m, s->opt.item0, s->y);
    });
}

int gpirt_sampler_ppc_pairs_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_pairs, pair_get, name, h_out, bytes);
}

int gpirt_sampler_ppc_pairs_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_pairs, pair_state_words, d_state, bytes);
}

int gpirt_ppc_pairs_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_pairs* out)
{
    return pair_combine(h, chains, d_states, out);
}

// ---- theta-binned item fit (ppc_bins.hip): an add-on to the PPC state ------------------------------------------------------
int gpirt_sampler_ppc_bins_enable(gpirt_sampler_t s, int h, const int* cuts, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_ppc_bins_enable", ORD_BINARY));
    return stage_enable(s, &s->ppc.bins, bin_free, on, [&]() -> int {
        GP_TRY(needs(blk_ppc(s)));
        return bin_alloc(s->h->stream, &s->ppc.bins, s->n, s->m, s->opt.item0, s->ppc.rblocks, h, cuts);
    });
}

int gpirt_sampler_ppc_bins_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_bins, bin_get, name, h_out, bytes);
}

int gpirt_sampler_ppc_bins_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_bins, bin_state_words, d_state, bytes);
}

int gpirt_ppc_bins_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ppc_bins* out)
{
    return bin_combine(h, chains, d_states, signs, out);
}

// ---- group-wise item fit (ppc_dif.hip): an add-on to the PPC state ----------------------------------------------------------
int gpirt_sampler_ppc_dif_enable(gpirt_sampler_t s, int G, const int32_t* groups, int h, const int* cuts, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_ppc_dif_enable", ORD_BINARY));
    return stage_enable(s, &s->ppc.dif, dif_free, on, [&]() -> int {
        GP_TRY(needs(blk_ppc(s)));
        return dif_alloc(s->h->stream, &s->ppc.dif, s->n, s->m, s->opt.item0, G, groups, h, cuts);
    });
}

int gpirt_sampler_ppc_dif_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_dif, dif_get, name, h_out, bytes);
}

int gpirt_sampler_ppc_dif_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_dif, dif_state_words, d_state, bytes);
}

int gpirt_ppc_dif_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ppc_dif* out)
{
    return dif_combine(h, chains, d_states, signs, out);
}

// ---- score-based checks (ppc_scores.hip): an add-on to the PPC state ---------------------------------------------------------
int gpirt_ppc_scores_check(int64_t n, int64_t m, int K, const int* cuts) { return pps_check(n, m, K, cuts); }

int gpirt_sampler_ppc_scores_enable(gpirt_sampler_t s, int K, const int* cuts, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_ppc_scores_enable", ORD_BINARY));
    return stage_enable(s, &s->ppc.scores, pps_free, on, [&]() -> int {
        GP_TRY(needs(blk_ppc(s)));
        if (s->opt.item0 != 0 || s->opt.m_total != s->m) {
            set_error("the score-based checks are not offered for item shards (a respondent's score runs over all items)");
            return GPIRT_E_ARG;
        }
        return pps_alloc(s->h->stream, &s->ppc.scores, s->n, s->m, s->opt.item0, s->y, K, cuts);
    });
}

int gpirt_sampler_ppc_scores_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_scores, pps_get, name, h_out, bytes);
}

int gpirt_sampler_ppc_scores_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_scores, pps_state_words, d_state, bytes);
}

int gpirt_ppc_scores_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_scores* out)
{
    return pps_combine(h, chains, d_states, out);
}

// ---- person fit (ppc_person.hip): an add-on to the PPC state -----------------------------------------------------------------
int gpirt_ppc_person_check(int64_t n, int64_t m, int K, const int32_t* order, const int* cuts)
{
    return prs_check(n, m, K, order, cuts);
}

int gpirt_sampler_ppc_person_enable(gpirt_sampler_t s, int K, const int32_t* order, const int* cuts, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_ppc_person_enable", ORD_BINARY));
    return stage_enable(s, &s->ppc.person, prs_free, on, [&]() -> int {
        GP_TRY(needs(blk_ppc(s)));
        if (s->opt.item0 != 0 || s->opt.m_total != s->m) {
            set_error("the person fit is not offered for item shards (a respondent's pattern runs over all items)");
            return GPIRT_E_ARG;
        }
        return prs_alloc(s->h->stream, &s->ppc.person, s->n, s->m, s->opt.item0, s->y, K, order, cuts);
    });
}

int gpirt_sampler_ppc_person_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_person, prs_get, name, h_out, bytes);
}

int gpirt_sampler_ppc_person_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_person, prs_state_words, d_state, bytes);
}

int gpirt_ppc_person_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_person* out)
{
    return prs_combine(h, chains, d_states, out);
}

// ---- residual correlations (ppc_resid.hip): an add-on to the PPC state ---------------------------------------------------------
int gpirt_sampler_ppc_resid_enable(gpirt_sampler_t s, int top)
{
    GP_ARG(s && s->initialised);
    if (top != 0) GP_TRY(ord_refuse(s, "gpirt_sampler_ppc_resid_enable", ORD_BINARY));
    return stage_enable(s, &s->ppc.resid, rsd_free, top != 0, [&]() -> int {
        GP_TRY(needs(blk_ppc(s)));
        GP_TRY(check_top("residual PPC", top, GPIRT_RESID_MAX_TOP));
        if (s->opt.item0 != 0 || s->opt.m_total != s->m) {
            set_error("the residual correlations are not offered for item shards (a pair's items may lie on two ranks)");
            return GPIRT_E_ARG;
        }
        return rsd_alloc(s->h->stream, &s->ppc.resid, s->n, s->m, s->opt.item0, s->y);
    });
}

int gpirt_sampler_ppc_resid_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_resid, rsd_get, name, h_out, bytes);
}

int gpirt_sampler_ppc_resid_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_resid, rsd_state_words, d_state, bytes);
}

int gpirt_ppc_resid_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_ppc_resid* out)
{
    return rsd_combine(h, chains, d_states, out);
}

// ---- rank posteriors (ranks.hip) on the stage API -----------------------------------------------------------------------
int gpirt_sampler_rank_enable(gpirt_sampler_t s, const int64_t* pivots, int n_pivots, int pairwise)
{
    GP_ARG(s && s->initialised);
    return stage_enable(s, &s->rank, rank_free, pivots || n_pivots >= 0,
                        [&] { return rank_alloc(s->h->stream, &s->rank, s->n, pivots, n_pivots, pairwise); });
}

int gpirt_sampler_rank_accumulate(gpirt_sampler_t s) { return stage_accumulate(s, blk_rank, acc_rank); }

int gpirt_sampler_rank_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_rank, rank_get, name, h_out, bytes);
}

int gpirt_sampler_rank_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_rank, rank_state_words, d_state, bytes);
}

int gpirt_rank_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_ranks* out)
{
    return rank_combine(h, chains, d_states, signs, out);
}

// ---- IRF shape posteriors (shape.hip) on the stage API -------------------------------------------------------------------
int gpirt_sampler_shape_enable(gpirt_sampler_t s, int k_half, const double* tols, int n_tols, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(shape_check(k_half, tols, n_tols));  // refused before the old state goes
    return stage_enable(s, &s->shape, shape_free, on,
                        [&] { return shape_alloc(s->h->stream, &s->shape, s->n, s->m, k_half, tols, n_tols); });
}

int gpirt_sampler_shape_accumulate(gpirt_sampler_t s) { return stage_accumulate(s, blk_shape, acc_shape); }

int gpirt_sampler_shape_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_shape, shape_get, name, h_out, bytes);
}

int gpirt_sampler_shape_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_shape, shape_state_words, d_state, bytes);
}

int gpirt_shape_state_bytes(int64_t m, int64_t* bytes)
{
    GP_ARG(m > 0 && bytes);
    *bytes = shape_layout(m).words * (int64_t)sizeof(uint64_t);
    return 0;
}

int gpirt_shape_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_shape* out)
{
    return shape_combine(h, chains, d_states, signs, out);
}

// ---- sum-score posteriors (sumscore.hip) on the stage API -----------------------------------------------------------------
int gpirt_sampler_sumscore_enable(gpirt_sampler_t s, const unsigned char* items_mask, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_sumscore_enable", "its scores are sums of binary answers"));
    if (on) GP_TRY(sumscore_check(s->m, items_mask, nullptr));   // refused before the old state goes
    return stage_enable(s, &s->sumscore, sumscore_free, on,
                        [&] { return sumscore_alloc(s->h->stream, &s->sumscore, s->m, items_mask); });
}

int gpirt_sampler_sumscore_accumulate(gpirt_sampler_t s) { return stage_accumulate(s, blk_sumscore, acc_sumscore); }

int gpirt_sampler_sumscore_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_sumscore, sumscore_get, name, h_out, bytes);
}

int gpirt_sampler_sumscore_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_sumscore, sumscore_state_words, d_state, bytes);
}

int gpirt_sumscore_state_bytes(int64_t m, int64_t M, int64_t* bytes)
{
    GP_ARG(m > 0 && M >= 1 && M <= m && M <= GPIRT_SUMSCORE_MAX_ITEMS && bytes);
    *bytes = sumscore_layout(m, M).words * (int64_t)sizeof(uint64_t);
    return 0;
}

int gpirt_sumscore_grid_weights(double* h_w)
{
    GP_ARG(h_w);
    sumscore_grid_weights(h_w);
    return 0;
}

int gpirt_sumscore_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_sumscore* out)
{
    return sumscore_combine(h, chains, d_states, signs, out);
}

// ---- two-form score equating (equate.hip) on the stage API ----------------------------------------------------------------
int gpirt_sampler_equate_enable(gpirt_sampler_t s, const unsigned char* mask_x, const unsigned char* mask_y, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_equate_enable", "its scores are sums of binary answers"));
    if (on) GP_TRY(equate_check(s->m, mask_x, mask_y, nullptr, nullptr));   // refused before the old state goes
    return stage_enable(s, &s->equate, equate_free, on,
                        [&] { return equate_alloc(s->h->stream, &s->equate, s->m, mask_x, mask_y); });
}

int gpirt_sampler_equate_accumulate(gpirt_sampler_t s) { return stage_accumulate(s, blk_equate, acc_equate); }

int gpirt_sampler_equate_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_equate, equate_get, name, h_out, bytes);
}

int gpirt_sampler_equate_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_equate, equate_state_words, d_state, bytes);
}

int gpirt_equate_state_bytes(int64_t m, int64_t Mx, int64_t My, int64_t* bytes)
{
    GP_ARG(m > 0 && Mx >= 1 && My >= 1 && Mx + My <= m && Mx <= GPIRT_EQUATE_MAX_ITEMS && My <= GPIRT_EQUATE_MAX_ITEMS && bytes);
    *bytes = equate_layout(m, Mx, My).words * (int64_t)sizeof(uint64_t);
    return 0;
}

int gpirt_equate_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_equate* out)
{
    return equate_combine(h, chains, d_states, out);
}

// ---- PSIS-LOO (loo.hip) on the stage API -----------------------------------------------------------------------------------
int gpirt_sampler_loo_enable(gpirt_sampler_t s, int64_t planned_total_draws, int tail, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_loo_enable", ORD_BINARY));
    int64_t M = 0;
    if (on) GP_TRY(loo_tail_length(planned_total_draws, tail, &M));   // refused before the old state goes
    return stage_enable(s, &s->loo, loo_free, on,
                        [&] { return loo_alloc(s->h->stream, &s->loo, s->n, s->m, planned_total_draws, M, s->y); });
}

int gpirt_sampler_loo_accumulate(gpirt_sampler_t s) { return stage_accumulate(s, blk_loo, acc_loo); }

int gpirt_sampler_loo_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_loo, loo_get, name, h_out, bytes);
}

int gpirt_sampler_loo_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_loo, loo_state_words, d_state, bytes);
}

int gpirt_loo_tail_length(int64_t T, int tail, int64_t* M)
{
    GP_ARG(M);
    return loo_tail_length(T, tail, M);
}

int gpirt_loo_state_bytes(int64_t n, int64_t m, int64_t M, int64_t* bytes)
{
    GP_ARG(n > 0 && m > 0 && M >= 0 && M <= GPIRT_LOO_MAX_TAIL && bytes);
    *bytes = loo_layout(n, m, M).words * (int64_t)sizeof(uint64_t);
    return 0;
}

int gpirt_loo_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_loo* out)
{
    return loo_combine(h, chains, d_states, out);
}

// ---- item-pair order posteriors (order.hip) on top of the shape block ------------------------------------------------------
int gpirt_sampler_shape_order_enable(gpirt_sampler_t s, int on)
{
    GP_ARG(s && s->initialised);
    if (on) {                                           // refused before the old block goes
        if (!s->shape.on) {
            set_error("the order posteriors need the shape posteriors (gpirt_sampler_shape_enable first)");
            return GPIRT_E_ARG;
        }
        if (s->m < 2 || s->m > GPIRT_ORDER_MAX_M) {
            set_error("order posteriors: m = %lld items, 2..%d are taken", (long long)s->m, GPIRT_ORDER_MAX_M);
            return GPIRT_E_ARG;
        }
    }
    return stage_enable(s, &s->shape.order, order_free, on, [&] { return order_alloc(s->h->stream, &s->shape); });
}

int gpirt_sampler_shape_order_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_order, order_get, name, h_out, bytes);
}

int gpirt_sampler_shape_order_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_order, order_state_words, d_state, bytes);
}

int gpirt_shape_order_state_bytes(int64_t m, int n_tols, int64_t* bytes)
{
    GP_ARG(m >= 2 && m <= GPIRT_ORDER_MAX_M && n_tols >= 1 && n_tols <= GPIRT_SHAPE_MAX_TOLS && bytes);
    *bytes = order_layout(m, n_tols).words * (int64_t)sizeof(uint64_t);
    return 0;
}

int gpirt_shape_order_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_shape_order* out)
{
    return order_combine(h, chains, d_states, out);
}

// ---- autocorrelation ESS (acf.hip) on the stage API -------------------------------------------------------------------------
int gpirt_acf_check(int64_t n, int64_t m, int parts, int64_t planned_draws, int64_t max_lag, int64_t* L_out, int64_t* P_out)
{
    return acf_check(n, m, parts, planned_draws, max_lag, L_out, P_out);
}

int gpirt_sampler_acf_enable(gpirt_sampler_t s, int parts, int64_t planned_draws, int64_t max_lag, int on)
{
    GP_ARG(s && s->initialised);
    if (on && (parts & GPIRT_ACF_LL)) GP_TRY(ord_refuse(s, "gpirt_sampler_acf_enable", "its log-likelihood series evaluates the binary likelihood of y"));
    int64_t L = 0;
    if (on) GP_TRY(acf_check(s->n, s->m, parts, planned_draws, max_lag, &L, nullptr));   // refused before the old state goes
    return stage_enable(s, &s->acf, acf_free, on,
                        [&] { return acf_alloc(s->h->stream, &s->acf, s->n, s->m, parts, planned_draws, L); });
}

int gpirt_sampler_acf_accumulate(gpirt_sampler_t s) { return stage_accumulate(s, blk_acf, acc_acf, true); }

int gpirt_sampler_acf_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_acf, acf_get, name, h_out, bytes);
}

int gpirt_sampler_acf_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_acf, acf_state_words, d_state, bytes);
}

int gpirt_acf_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_acf* out)
{
    return acf_combine(h, chains, d_states, signs, out);
}

// ---- group posteriors (groups.hip) on the stage API --------------------------------------------------------------------------
int gpirt_groups_check(int64_t n, int64_t m, int G, const int32_t* groups, int top, int64_t* sizes_out)
{
    return groups_check(n, m, G, groups, top, sizes_out);
}

int gpirt_sampler_groups_enable(gpirt_sampler_t s, int G, const int32_t* groups, int top, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_groups_enable", "its vote part evaluates the binary likelihood of y"));
    if (on) {                                         // refused before the old state goes
        if (s->opt.item0 != 0 || s->opt.m_total != s->m) {
            set_error("groups: not offered for an item shard (the vote part runs over all items)");
            return GPIRT_E_ARG;
        }
        GP_TRY(groups_check(s->n, s->m, G, groups, top, nullptr));
    }
    return stage_enable(s, &s->groups, groups_free, on,
                        [&] { return groups_alloc(s->h->stream, &s->groups, s->n, s->m, G, groups, top); });
}

int gpirt_sampler_groups_accumulate(gpirt_sampler_t s) { return stage_accumulate(s, blk_groups, acc_groups, true); }

int gpirt_sampler_groups_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_groups, groups_get, name, h_out, bytes);
}

int gpirt_sampler_groups_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_groups, groups_state_words, d_state, bytes);
}

int gpirt_groups_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_groups* out)
{
    return groups_combine(h, chains, d_states, signs, out);
}

// ---- scoring new respondents (score.hip) on the stage API ----------------------------------------------------------------
int gpirt_sampler_score_enable(gpirt_sampler_t s, const double* h_y_new, int64_t n_new)
{
    GP_ARG(s && s->initialised);
    if (h_y_new && n_new != 0) GP_TRY(ord_refuse(s, "gpirt_sampler_score_enable", ORD_BINARY));
    const bool on = h_y_new && n_new != 0;
    if (on) {                                           // every refusal before the old state is touched
        if (n_new < 1 || n_new > GPIRT_SCORE_MAX_N) {
            set_error("scoring: n_new = %lld is outside 1..%d", (long long)n_new, GPIRT_SCORE_MAX_N);
            return GPIRT_E_ARG;
        }
        if (s->opt.item0 != 0 || s->opt.m_total != s->m) {
            set_error("scoring is not offered for item shards (a new respondent's product runs over all items)");
            return GPIRT_E_ARG;
        }
        GP_TRY(score_check_new(h_y_new, n_new, s->m));
    }
    return stage_enable(s, &s->score, score_free, on, [&] { return score_alloc(s->h->stream, &s->score, h_y_new, n_new, s->m); });
}

int gpirt_sampler_score_accumulate(gpirt_sampler_t s) { return stage_accumulate(s, blk_score, acc_score); }

int gpirt_sampler_score_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_score, score_get, name, h_out, bytes);
}

int gpirt_sampler_score_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_score, score_state_words, d_state, bytes);
}

int gpirt_score_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, gpirt_score* out)
{
    return score_combine(h, chains, d_states, signs, out);
}

// ---- predicting the new respondents' unseen answers (predict.hip): an add-on to the score state --------------------------------
int gpirt_sampler_score_predict_enable(gpirt_sampler_t s, int on)
{
    GP_ARG(s && s->initialised);
    if (on) GP_TRY(ord_refuse(s, "gpirt_sampler_score_predict_enable", ORD_BINARY));
    if (on) GP_TRY(needs(blk_score(s)));
    return stage_enable(s, &s->score.pred, pred_free, on, [&] { return pred_alloc(s->h->stream, &s->score); });
}

int gpirt_sampler_score_predict_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    return stage_get(s, blk_predict, pred_get, name, h_out, bytes);
}

int gpirt_sampler_score_predict_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    return stage_state(s, blk_predict, pred_state_words, d_state, bytes);
}

int gpirt_score_predict_combine(gpirt_handle_t h, int chains, const void* const* d_states, gpirt_score_predict* out)
{
    return pred_combine(h, chains, d_states, out);
}

// ---- the length scale as a parameter of the chain -------------------------------------------------------------------------
int gpirt_sampler_ell_enable(gpirt_sampler_t s, double lo, double hi, int P, const double* log_prior, int width, int k0, int on)
{
    GP_ARG(s != nullptr);
    EllState& e = s->ell;
    if (!on) {
        GP_HIP(hipStreamSynchronize(s->h->stream));
        ell_free(&e);
        s->nu_kern_ok = nu_kernel_ok(s->kern);
        return fstar_free_setup(s);          // (the kernel stays where the chain left it)
    }
    if (!s->initialised) { set_error("gpirt_sampler_ell_enable needs an initialised sampler (gpirt_sampler_init)"); return GPIRT_E_ARG; }
    gpirt_kernel kk;
    gpirt_kernel_default(&kk);
    kk.family = s->kern.family; kk.length_scale = s->kern.length_scale;
    GP_TRY(gpirt_ell_check(lo, hi, P, log_prior, width, k0, &kk, &s->opt, s->m));
    GP_TRY(ensure_dense_factor(s));       // (the updates read all of L; from here on every factor is dense)
    GP_HIP(hipStreamSynchronize(s->h->stream));
    ell_free(&e);
    const int64_t n = s->n, m = s->m;
    auto fail = [&](int rc, const char* what) { set_error("length scale: %s failed", what); ell_free(&e); return rc; };
    if (hipMalloc((void**)&e.Lsave, sizeof(double) * (size_t)(s->ldl * n)) != hipSuccess ||
        hipMalloc((void**)&e.fprop, sizeof(double) * (size_t)(n * m)) != hipSuccess ||
        hipMalloc((void**)&e.delta, sizeof(double) * (size_t)m) != hipSuccess ||
        hipMalloc((void**)&e.rec, sizeof(double) * 8) != hipSuccess ||
        hipMalloc((void**)&e.nuprop, sizeof(double) * (size_t)(n * m)) != hipSuccess ||
        hipMalloc((void**)&e.dq, sizeof(double) * (size_t)m) != hipSuccess ||
        hipMalloc((void**)&e.ld, sizeof(double) * 2) != hipSuccess ||
        hipMalloc((void**)&e.rec_c, sizeof(double) * 8) != hipSuccess ||
        hipMalloc((void**)&e.nonfin, sizeof(int) * (size_t)m) != hipSuccess ||
        hipMalloc((void**)&e.flag, sizeof(int)) != hipSuccess) return fail(GPIRT_E_ALLOC, "hipMalloc");
    if (hipHostMalloc((void**)&e.h_flag, sizeof(int), hipHostMallocDefault) != hipSuccess) return fail(GPIRT_E_ALLOC, "the pinned allocation");
    if (hipEventCreateWithFlags(&e.ev, hipEventDisableTiming) != hipSuccess) return fail(GPIRT_E_HIP, "hipEventCreate");
    hipStream_t st = s->h->stream;
    if (hipMemsetAsync(e.fprop, 0, sizeof(double) * (size_t)(n * m), st) != hipSuccess ||
        hipMemsetAsync(e.delta, 0, sizeof(double) * (size_t)m, st) != hipSuccess ||
        hipMemsetAsync(e.rec, 0, sizeof(double) * 8, st) != hipSuccess ||
        hipMemsetAsync(e.nuprop, 0, sizeof(double) * (size_t)(n * m), st) != hipSuccess ||
        hipMemsetAsync(e.dq, 0, sizeof(double) * (size_t)m, st) != hipSuccess ||
        hipMemsetAsync(e.ld, 0, sizeof(double) * 2, st) != hipSuccess ||
        hipMemsetAsync(e.rec_c, 0, sizeof(double) * 8, st) != hipSuccess ||
        hipMemsetAsync(e.nonfin, 0, sizeof(int) * (size_t)m, st) != hipSuccess ||
        hipMemsetAsync(e.flag, 0, sizeof(int), st) != hipSuccess) return fail(GPIRT_E_HIP, "hipMemsetAsync");
    e.P = P; e.up[ELL_WHITENED].w = e.up[ELL_CENTRED].w = width;
    e.grid.resize((size_t)P); e.log_prior.resize((size_t)P);
    ell_grid_fill(lo, hi, P, e.grid.data());
    for (int k = 0; k < P; ++k) {
        const long double l = logl((long double)e.grid[(size_t)k]);
        e.log_prior[(size_t)k] = log_prior ? log_prior[k] : (double)(-(l * l) / 2.0L);
        if (k0 < 0 && e.grid[(size_t)k] == s->kern.length_scale) k0 = k;
    }
    e.k = k0;
    e.on = true;
    {
        // draw_f's structured product under a moving length scale: the certificate at the grid's smallest ell covers the grid
        KernelSpec at_lo = s->kern;
        at_lo.length_scale = lo; at_lo.inv_ell = 1.0 / lo;
        s->nu_kern_ok = nu_kernel_ok(at_lo);
    }
    if (e.grid[(size_t)k0] != s->kern.length_scale) {
        // the chain starts at ell_k0: its factor, through the same core as every other
        int rc = ell_settle_factor(s);
        if (!rc) rc = ell_join(s);
        if (!rc) {
            ell_set_kernel(s, e.grid[(size_t)k0]);
            rc = factor_core(s);
            s->factor_fresh = true;
        }
        if (rc) { ell_free(&e); return rc; }
    }
    return 0;
}

int gpirt_sampler_draw_ell(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    GP_TRY(ord_refuse(s, "gpirt_sampler_draw_ell", ORD_BINARY));
    GP_TRY(needs(s->ell.on, "the length-scale update is", "gpirt_sampler_ell_enable"));
    return do_draw_ell(s, ELL_WHITENED);
}

int gpirt_sampler_draw_ell_centred(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    GP_TRY(needs(s->ell.on, "the length-scale update is", "gpirt_sampler_ell_enable"));
    if (s->amp.mode) {
        set_error("gpirt_sampler_draw_ell_centred is refused while per-item amplitudes are on: its quadratic form would need "
                  "1 / a_j^2 per item (the whitened update does not contain a_j and runs)");
        return GPIRT_E_ARG;
    }
    return do_draw_ell(s, ELL_CENTRED);
}

static int ell_set_width(gpirt_sampler_t s, int w, int kind)
{
    GP_ARG(s != nullptr);
    GP_TRY(needs(s->ell.on, "the length-scale update is", "gpirt_sampler_ell_enable"));
    if (w < 1 || w > s->ell.P - 1) {
        set_error("length scale: width = %d, it must lie in 1 .. P - 1 = %d", w, s->ell.P - 1);
        return GPIRT_E_ARG;
    }
    s->ell.up[kind].w = w;
    return 0;
}

int gpirt_sampler_ell_width(gpirt_sampler_t s, int w)
{
    return ell_set_width(s, w, ELL_WHITENED);
}

int gpirt_sampler_ell_width_centred(gpirt_sampler_t s, int w)
{
    return ell_set_width(s, w, ELL_CENTRED);
}

int gpirt_sampler_ell_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    GP_ARG(s && name && h_out && bytes >= 0);
    EllState& e = s->ell;
    GP_TRY(needs(e.on, "the length-scale update is", "gpirt_sampler_ell_enable"));
    const int64_t nm = s->n * s->m;
    const EllUpdate &wh = e.up[ELL_WHITENED], &ce = e.up[ELL_CENTRED];
    const int64_t counts[4] = { wh.updates, wh.accepted, wh.out_of_range, wh.failed };
    const int64_t counts_c[4] = { ce.updates, ce.accepted, ce.out_of_range, ce.failed };
    const int64_t index = e.k;
    const void* host = nullptr; const void* dev = nullptr; int64_t want = 0;
    if (strcmp(name, "grid") == 0) { host = e.grid.data(); want = 8 * (int64_t)e.P; }
    else if (strcmp(name, "log_prior") == 0) { host = e.log_prior.data(); want = 8 * (int64_t)e.P; }
    else if (strcmp(name, "index") == 0) { host = &index; want = 8; }
    else if (strcmp(name, "counts") == 0) { host = counts; want = 32; }
    else if (strcmp(name, "nu") == 0) { dev = s->NU; want = 8 * nm; }
    else if (strcmp(name, "f_prop") == 0) { dev = e.fprop; want = 8 * nm; }
    else if (strcmp(name, "delta") == 0) { dev = e.delta; want = 8 * s->m; }
    else if (strcmp(name, "record") == 0) { dev = e.rec; want = 40; }
    else if (strcmp(name, "times") == 0) { host = wh.part_ms; want = 8 * GPIRT_ELL_PARTS; }
    else if (strcmp(name, "nu_prop") == 0) { dev = e.nuprop; want = 8 * nm; }
    else if (strcmp(name, "dq") == 0) { dev = e.dq; want = 8 * s->m; }
    else if (strcmp(name, "record_centred") == 0) { dev = e.rec_c; want = 48; }
    else if (strcmp(name, "counts_centred") == 0) { host = counts_c; want = 32; }
    else if (strcmp(name, "times_centred") == 0) { host = ce.part_ms; want = 8 * GPIRT_ELL_PARTS; }
    else { set_error("unknown length-scale array '%s'", name); return GPIRT_E_ARG; }
    if (bytes != want) { set_error("length scale: '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes); return GPIRT_E_ARG; }
    if (host) { memcpy(h_out, host, (size_t)want); return 0; }
    GP_HIP(hipMemcpyAsync(h_out, dev, (size_t)want, hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

int gpirt_sampler_ell_stats(gpirt_sampler_t s, gpirt_ell* out)
{
    GP_ARG(s && out);
    const EllState& e = s->ell;
    GP_TRY(needs(e.on, "the length-scale update is", "gpirt_sampler_ell_enable"));
    const EllUpdate& c = e.up[ELL_WHITENED];
    memset(out, 0, sizeof(*out));
    out->points = e.P; out->width = c.w; out->index = e.k;
    out->updates = c.updates; out->accepted = c.accepted; out->out_of_range = c.out_of_range; out->failed = c.failed;
    out->last = c.last; out->last_proposed = c.last_proposed; out->factorisations = c.factorisations;
    out->length_scale = e.grid[(size_t)e.k]; out->lo = e.grid.front(); out->hi = e.grid.back();
    out->last_u0 = c.last_u0; out->last_u1 = c.last_u1;
    return 0;
}

int gpirt_sampler_ell_centred_stats(gpirt_sampler_t s, gpirt_ell_centred* out)
{
    GP_ARG(s && out);
    const EllState& e = s->ell;
    GP_TRY(needs(e.on, "the length-scale update is", "gpirt_sampler_ell_enable"));
    const EllUpdate& c = e.up[ELL_CENTRED];
    memset(out, 0, sizeof(*out));
    out->width = c.w;
    out->updates = c.updates; out->accepted = c.accepted; out->out_of_range = c.out_of_range; out->failed = c.failed;
    out->last = c.last; out->last_proposed = c.last_proposed; out->factorisations = c.factorisations;
    out->last_u0 = c.last_u0; out->last_u1 = c.last_u1;
    return 0;
}

// ---- per-item GP amplitudes ---------------------------------------------------------------------------------------------------
static int amp_refusals(gpirt_sampler_t s, const char* entry)
{
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", entry); return GPIRT_E_ARG; }
    return gpirt_amp_check(GPIRT_AMP_MIN, GPIRT_AMP_MAX, 2, nullptr, 1, nullptr, s->m, &s->opt);      // (the options' refusals)
}

int gpirt_sampler_amp_set(gpirt_sampler_t s, const double* a)
{
    GP_ARG(s != nullptr);
    AmpState& A = s->amp;
    if (!a) {
        if (A.mode == 2) { set_error("gpirt_sampler_amp_set(NULL): the amplitudes are on the grid, gpirt_sampler_amp_enable(on = 0) turns them off"); return GPIRT_E_ARG; }
        GP_HIP(hipStreamSynchronize(s->h->stream));
        amp_free(&A);
        return 0;
    }
    if (A.mode == 2) {
        set_error("gpirt_sampler_amp_set after gpirt_sampler_amp_enable: turn the sampled amplitudes off first (on = 0)");
        return GPIRT_E_ARG;
    }
    GP_TRY(amp_refusals(s, "gpirt_sampler_amp_set"));
    const int64_t m = s->m;
    for (int64_t j = 0; j < m; ++j)
        if (!std::isfinite(a[j]) || !(a[j] >= GPIRT_AMP_MIN) || !(a[j] <= GPIRT_AMP_MAX)) {
            set_error("amplitude: a[%lld] = %g, it must be finite and lie in %g .. %g", (long long)j, a[j], (double)GPIRT_AMP_MIN,
                      (double)GPIRT_AMP_MAX);
            return GPIRT_E_ARG;
        }
    hipStream_t st = s->h->stream;
    if (!A.amp && hipMalloc((void**)&A.amp, sizeof(double) * (size_t)m) != hipSuccess) {
        set_error("amplitude: hipMalloc failed");
        return GPIRT_E_ALLOC;
    }
    GP_HIP(hipMemcpyAsync(A.amp, a, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));
    A.mode = 1;
    return 0;
}

int gpirt_sampler_amp_enable(gpirt_sampler_t s, double lo, double hi, int P, const double* log_prior, int width, const int* k0,
                             int64_t planned_draws, int on)
{
    GP_ARG(s != nullptr);
    AmpState& A = s->amp;
    if (!on) {
        if (A.mode == 1) { set_error("gpirt_sampler_amp_enable(on = 0): the amplitudes are fixed, gpirt_sampler_amp_set(NULL) turns them off"); return GPIRT_E_ARG; }
        GP_HIP(hipStreamSynchronize(s->h->stream));
        amp_free(&A);
        return 0;
    }
    if (A.mode == 1) {
        set_error("gpirt_sampler_amp_enable after gpirt_sampler_amp_set: turn the fixed amplitudes off first (gpirt_sampler_amp_set(NULL))");
        return GPIRT_E_ARG;
    }
    if (!s->initialised) { set_error("gpirt_sampler_amp_enable needs an initialised sampler (gpirt_sampler_init)"); return GPIRT_E_ARG; }
    const int64_t m = s->m;
    GP_TRY(gpirt_amp_check(lo, hi, P, log_prior, width, k0, m, &s->opt));
    if (planned_draws < 0 || planned_draws > (int64_t)1 << 31) {
        set_error("amplitude: planned_draws = %lld, it must lie in 0 .. 2^31", (long long)planned_draws);
        return GPIRT_E_ARG;
    }
    hipStream_t st = s->h->stream;
    GP_HIP(hipStreamSynchronize(st));
    amp_free(&A);
    auto fail = [&](int rc, const char* what) { set_error("amplitude: %s failed", what); amp_free(&A); return rc; };
    const size_t hist_bytes = sizeof(uint32_t) * (size_t)P * (size_t)m, draw_bytes = sizeof(int32_t) * (size_t)(planned_draws ? planned_draws : 1) * (size_t)m;
    if (hipMalloc((void**)&A.amp, sizeof(double) * (size_t)m) != hipSuccess ||
        hipMalloc((void**)&A.d_grid, sizeof(double) * (size_t)P) != hipSuccess ||
        hipMalloc((void**)&A.d_log_prior, sizeof(double) * (size_t)P) != hipSuccess ||
        hipMalloc((void**)&A.rec, sizeof(double) * 5 * (size_t)m) != hipSuccess ||
        hipMalloc((void**)&A.idx, sizeof(int) * (size_t)m) != hipSuccess ||
        hipMalloc((void**)&A.width, sizeof(int) * (size_t)m) != hipSuccess ||
        hipMalloc((void**)&A.counts, sizeof(long long) * 4 * (size_t)m) != hipSuccess ||
        hipMalloc((void**)&A.hist, hist_bytes) != hipSuccess ||
        hipMalloc((void**)&A.draws, draw_bytes) != hipSuccess) return fail(GPIRT_E_ALLOC, "hipMalloc");
    A.P = P; A.planned = planned_draws; A.recorded = 0;
    A.grid.resize((size_t)P); A.log_prior.resize((size_t)P);
    ell_grid_fill(lo, hi, P, A.grid.data());
    for (int k = 0; k < P; ++k) {
        const long double l = logl((long double)A.grid[(size_t)k]);
        A.log_prior[(size_t)k] = log_prior ? log_prior[k] : (double)(-(l * l) / 2.0L);
    }
    const int near1 = amp_nearest_one(A.grid.data(), P);
    std::vector<int> idx((size_t)m), wd((size_t)m, width);
    std::vector<double> amp((size_t)m);
    for (int64_t j = 0; j < m; ++j) {
        idx[(size_t)j] = k0 ? k0[j] : near1;
        amp[(size_t)j] = A.grid[(size_t)idx[(size_t)j]];
    }
    if (hipMemcpyAsync(A.d_grid, A.grid.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.d_log_prior, A.log_prior.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.amp, amp.data(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.idx, idx.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.width, wd.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(A.rec, 0, sizeof(double) * 5 * (size_t)m, st) != hipSuccess ||
        hipMemsetAsync(A.counts, 0, sizeof(long long) * 4 * (size_t)m, st) != hipSuccess ||
        hipMemsetAsync(A.hist, 0, hist_bytes, st) != hipSuccess ||
        hipMemsetAsync(A.draws, 0, draw_bytes, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return fail(GPIRT_E_HIP, "the upload");      // (the host vectors go out of scope)
    A.mode = 2;
    return 0;
}

int gpirt_sampler_draw_amp(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    GP_TRY(ord_refuse(s, "gpirt_sampler_draw_amp", ORD_BINARY));
    AmpState& A = s->amp;
    GP_TRY(needs(A.mode == 2, "the amplitude update is", "gpirt_sampler_amp_enable"));
    // mu of a held-back draw_beta, and nothing on the sampler's own stream may still read the f this update rewrites in place
    GP_TRY(beta_sync(s));
    AmpUpdateArgs a{};
    a.f = s->f; a.mu = s->mu; a.y = s->y; a.n = s->n; a.m = s->m;
    a.grid = A.d_grid; a.log_prior = A.d_log_prior; a.P = A.P;
    a.idx = A.idx; a.width = A.width; a.amp = A.amp; a.counts = A.counts; a.rec = A.rec;
    a.seed = s->opt.seed; a.t = A.t + 1; a.item0 = (uint32_t)s->opt.item0;
    hipStream_t st = s->h->stream;
    const bool timed = s->timing;
    if (timed) {
        for (hipEvent_t& t : A.tev) if (!t) GP_HIP(hipEventCreate(&t));
        GP_HIP(hipEventRecord(A.tev[0], st));
    }
    GP_TRY(launch_amp_update(st, a));
    A.t += 1;
    if (timed) {                              // (timing on: one synchronisation, as the length-scale update's)
        GP_HIP(hipEventRecord(A.tev[1], st));
        GP_HIP(hipEventSynchronize(A.tev[1]));
        float ms = 0.f;
        hipEventElapsedTime(&ms, A.tev[0], A.tev[1]);
        A.last_ms = ms;
    }
    return 0;
}

int gpirt_sampler_amp_width(gpirt_sampler_t s, const int* w)
{
    GP_ARG(s && w);
    AmpState& A = s->amp;
    GP_TRY(needs(A.mode == 2, "the amplitude update is", "gpirt_sampler_amp_enable"));
    for (int64_t j = 0; j < s->m; ++j)
        if (w[j] < 1 || w[j] > A.P - 1) {
            set_error("amplitude: width[%lld] = %d, it must lie in 1 .. P - 1 = %d", (long long)j, w[j], A.P - 1);
            return GPIRT_E_ARG;
        }
    GP_HIP(hipMemcpyAsync(A.width, w, sizeof(int) * (size_t)s->m, hipMemcpyHostToDevice, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

int gpirt_sampler_amp_record(gpirt_sampler_t s)
{
    GP_ARG(s != nullptr);
    AmpState& A = s->amp;
    GP_TRY(needs(A.mode == 2, "the amplitude update is", "gpirt_sampler_amp_enable"));
    if (A.recorded >= A.planned) {
        set_error("amplitude: all %lld planned draws are recorded", (long long)A.planned);
        return GPIRT_E_ARG;
    }
    GP_TRY(launch_amp_record(s->h->stream, A.idx, s->m, A.P, A.recorded, A.hist, A.draws));
    A.recorded += 1;
    return 0;
}

int gpirt_sampler_amp_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    GP_ARG(s && name && h_out && bytes >= 0);
    AmpState& A = s->amp;
    GP_TRY(needs(A.mode != 0, "per-item amplitudes are", "gpirt_sampler_amp_set, gpirt_sampler_amp_enable"));
    const int64_t m = s->m, P = A.P;
    const void* host = nullptr; const void* dev = nullptr; int64_t want = 0;
    if (strcmp(name, "amplitude") != 0) GP_TRY(needs(A.mode == 2, "the amplitude update is", "gpirt_sampler_amp_enable"));
    if (strcmp(name, "amplitude") == 0) { dev = A.amp; want = 8 * m; }
    else if (strcmp(name, "grid") == 0) { host = A.grid.data(); want = 8 * P; }
    else if (strcmp(name, "log_prior") == 0) { host = A.log_prior.data(); want = 8 * P; }
    else if (strcmp(name, "index") == 0) { dev = A.idx; want = 4 * m; }
    else if (strcmp(name, "width") == 0) { dev = A.width; want = 4 * m; }
    else if (strcmp(name, "counts") == 0) { dev = A.counts; want = 32 * m; }
    else if (strcmp(name, "record") == 0) { dev = A.rec; want = 40 * m; }
    else if (strcmp(name, "hist") == 0) { dev = A.hist; want = 4 * P * m; }
    else if (strcmp(name, "draws") == 0) { dev = A.draws; want = 4 * A.recorded * m; }
    else if (strcmp(name, "time") == 0) { host = &A.last_ms; want = 8; }
    else if (strcmp(name, "time_centred") == 0) { host = &A.clast_ms; want = 8; }
    else if (strstr(name, "centred") != nullptr || strcmp(name, "rank") == 0 || strcmp(name, "live") == 0) {
        // the centred update's (gpirt_sampler_draw_amp_centred): they exist from its first call on
        GP_TRY(needs(A.cbuf != nullptr && s->sf.have, "the centred amplitude update's arrays are", "one gpirt_sampler_draw_amp_centred call"));
        const AmpCentredArgs& c = A.ca;
        const int64_t R = AMP_CENTRED_RANK;
        int32_t small[AMP_CENTRED_RANK];
        if (strcmp(name, "rank") == 0 || strcmp(name, "live") == 0) {
            const bool one = name[0] == 'r';
            want = one ? 4 : 4 * R;
            if (bytes != want) { set_error("amplitude: '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes); return GPIRT_E_ARG; }
            if (one) small[0] = s->sf.r;
            else for (int k = 0; k < R; ++k) small[k] = (int32_t)((s->sf.live >> k) & 1ull);
            memcpy(h_out, small, (size_t)want);
            return 0;
        }
        if (strcmp(name, "counts_centred") == 0) { dev = c.counts; want = 32 * m; }
        else if (strcmp(name, "record_centred") == 0) { dev = c.rec; want = 40 * m; }
        else if (strcmp(name, "centred_T") == 0) { dev = c.T; want = 8 * R * m; }
        else if (strcmp(name, "centred_z") == 0) { dev = c.Z; want = 8 * R * m; }
        else if (strcmp(name, "centred_w") == 0) { dev = c.W; want = 8 * R * m; }
        else if (strcmp(name, "centred_xi") == 0) { dev = c.Xi; want = 8 * R * m; }
        else if (strcmp(name, "centred_g") == 0) { dev = c.Gc; want = 8 * R * m; }
        else if (strcmp(name, "centred_Q") == 0) { dev = c.Q; want = 8 * m; }
        else if (strcmp(name, "centred_H") == 0) { dev = s->NU; want = 8 * s->n * m; }
        else if (strcmp(name, "centred_Xh") == 0) { dev = c.Xh; want = 8 * R * R; }
        else if (strcmp(name, "centred_R") == 0) { dev = c.R; want = 8 * R * R; }
        else if (strcmp(name, "centred_F") == 0) { dev = s->sf.F; want = 8 * R * R; }
        else { set_error("unknown amplitude array '%s'", name); return GPIRT_E_ARG; }
    }
    else { set_error("unknown amplitude array '%s'", name); return GPIRT_E_ARG; }
    if (bytes != want) { set_error("amplitude: '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes); return GPIRT_E_ARG; }
    if (want == 0) return 0;
    if (host) { memcpy(h_out, host, (size_t)want); return 0; }
    GP_HIP(hipMemcpyAsync(h_out, dev, (size_t)want, hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

int gpirt_sampler_amp_stats(gpirt_sampler_t s, gpirt_amp* out)
{
    GP_ARG(s && out);
    const AmpState& A = s->amp;
    memset(out, 0, sizeof(*out));
    out->on = A.mode; out->m = s->m; out->calls = A.t;
    out->accept_rate = (double)NAN; out->lo = out->hi = out->min_amplitude = out->max_amplitude = (double)NAN;
    if (A.mode == 0) return 0;
    const int64_t m = s->m;
    std::vector<double> amp((size_t)m);
    std::vector<long long> cnt(A.mode == 2 ? 4 * (size_t)m : 0);
    hipStream_t st = s->h->stream;
    GP_HIP(hipMemcpyAsync(amp.data(), A.amp, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
    if (A.mode == 2) GP_HIP(hipMemcpyAsync(cnt.data(), A.counts, sizeof(long long) * 4 * (size_t)m, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    out->min_amplitude = out->max_amplitude = amp[0];
    for (int64_t j = 1; j < m; ++j) {
        if (amp[(size_t)j] < out->min_amplitude) out->min_amplitude = amp[(size_t)j];
        if (amp[(size_t)j] > out->max_amplitude) out->max_amplitude = amp[(size_t)j];
    }
    if (A.mode != 2) return 0;
    out->points = A.P; out->planned_draws = A.planned; out->recorded = A.recorded;
    out->lo = A.grid.front(); out->hi = A.grid.back();
    for (int64_t j = 0; j < m; ++j) {
        out->updates += cnt[(size_t)j]; out->accepted += cnt[(size_t)(m + j)];
        out->out_of_range += cnt[(size_t)(2 * m + j)]; out->failed += cnt[(size_t)(3 * m + j)];
    }
    if (out->updates) out->accept_rate = (double)out->accepted / (double)out->updates;
    return 0;
}

// ---- the centred amplitude update (amp_centred.hip) ----------------------------------------------------------------------------
// the buffers of the first call after an enable: one allocation, the two tables of the proposal (long double on the host, rounded
// once), the nodes and weights of the basis; counters and record zeroed.  Drains the handle's stream.
static int amp_centred_alloc(gpirt_sampler_t s)
{
    AmpState& A = s->amp;
    if (A.cbuf) return 0;
    const size_t n = (size_t)s->n, m = (size_t)s->m, P = (size_t)A.P, R = AMP_CENTRED_RANK, RR = R * R;
    const size_t wide = m > R ? m : R;
    const size_t sizes[] = { n * R, RR, (size_t)KSPLIT * R * wide, RR, RR, R * m, R * m, R * m, R * m, R * m, m, P, P, 5 * m, 4 * m, R, R };
    size_t total = 0;
    for (size_t sz : sizes) total += sz;
    if (hipMalloc((void**)&A.cbuf, sizeof(double) * total) != hipSuccess) { A.cbuf = nullptr; set_error("amplitude (centred): hipMalloc failed"); return GPIRT_E_ALLOC; }
    double* p = A.cbuf;
    auto take = [&](size_t sz) { double* q = p; p += sz; return q; };
    AmpCentredArgs& c = A.ca;
    c = AmpCentredArgs();
    c.V = take(sizes[0]); c.Gv = take(sizes[1]); c.parts = take(sizes[2]); c.Xh = take(sizes[3]); c.R = take(sizes[4]);
    c.T = take(sizes[5]); c.Z = take(sizes[6]); c.W = take(sizes[7]); c.Xi = take(sizes[8]); c.Gc = take(sizes[9]); c.Q = take(sizes[10]);
    double* ln_a = take(sizes[11]); double* hia = take(sizes[12]);
    c.ln_a = ln_a; c.half_inv_a2 = hia;
    c.rec = take(sizes[13]);
    c.counts = reinterpret_cast<long long*>(take(sizes[14]));
    double* nodes = take(sizes[15]); double* wts = take(sizes[16]);
    c.nodes = nodes; c.wts = wts;
    c.nsplit = KSPLIT;
    std::vector<double> tab(2 * P), hn, hw;
    for (size_t k = 0; k < P; ++k) {
        const long double a = (long double)A.grid[k];
        tab[k] = (double)logl(a);
        tab[P + k] = (double)(0.5L / (a * a));
    }
    nu_lr_nodes(hn, hw);
    hipStream_t st = s->h->stream;
    if (hipMemsetAsync(A.cbuf, 0, sizeof(double) * total, st) != hipSuccess ||
        hipMemcpyAsync(ln_a, tab.data(), sizeof(double) * 2 * P, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(nodes, hn.data(), sizeof(double) * R, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(wts, hw.data(), sizeof(double) * R, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        hipFree(A.cbuf); A.cbuf = nullptr;
        set_error("amplitude (centred): the upload failed");
        return GPIRT_E_HIP;
    }
    return 0;
}

// F for the sampler's current length scale with its dead columns zeroed, the live mask and r (host; cached per sampler until the
// length scale moves; the two centred updates share it).  Drains the handle's stream when it rebuilds.
static int smooth_factor(gpirt_sampler_t s)
{
    SmoothF& S = s->sf;
    if (S.have && S.ell == s->kern.length_scale) return 0;
    constexpr int R = AMP_CENTRED_RANK;
    if (!S.F) GP_TRY(dalloc(s, &S.F, (size_t)R * R, false));
    std::vector<double> F;
    fstar_free_factor(s->kern, F);
    uint64_t live = 0;
    int r = 0;
    for (int k = 0; k < R; ++k) {
        long double sq = 0.0L;
        for (int i = 0; i < R; ++i) sq += (long double)F[(size_t)(i + R * k)] * (long double)F[(size_t)(i + R * k)];
        if (sq <= 1e-13L) { for (int i = 0; i < R; ++i) F[(size_t)(i + R * k)] = 0.0; }
        else { live |= 1ull << k; r += 1; }
    }
    hipStream_t st = s->h->stream;
    S.have = false;
    GP_HIP(hipMemcpyAsync(S.F, F.data(), sizeof(double) * F.size(), hipMemcpyHostToDevice, st));
    GP_HIP(hipStreamSynchronize(st));                          // (F leaves scope)
    S.live = live; S.r = r;
    S.have = true; S.ell = s->kern.length_scale;
    return 0;
}

int gpirt_sampler_draw_amp_centred(gpirt_sampler_t s)
{
    GP_ARG(s != nullptr);
    const char* me = "gpirt_sampler_draw_amp_centred";
    GP_TRY(ord_refuse(s, "gpirt_sampler_draw_amp_centred", ORD_BINARY));
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", me); return GPIRT_E_ARG; }
    if (stream_mode(s)) { set_error("%s: rng = reference (GPIRT_RNG_RSTREAM) is refused, R's stream has no such draw", me); return GPIRT_E_ARG; }
    if (s->opt.kernel_fp32) { set_error("%s: kernel_fp32 is refused, the single-precision build is the default kernel's alone", me); return GPIRT_E_ARG; }
    if (s->opt.item0 != 0 || (s->opt.m_total > 0 && s->opt.m_total != s->m)) {
        set_error("%s: an item shard (item0 = %lld, m_total = %lld) is refused, the amplitudes are kept for all items of one sampler", me,
                  (long long)s->opt.item0, (long long)s->opt.m_total);
        return GPIRT_E_ARG;
    }
    AmpState& A = s->amp;
    if (A.mode != 2) {
        set_error("%s: the amplitudes are not in the sampled mode (gpirt_sampler_amp_enable): %s", me,
                  A.mode == 1 ? "they are fixed" : "they are off");
        return GPIRT_E_ARG;
    }
    if (!s->nu_kern_ok) {
        if (s->kern.family != GPIRT_KERNEL_SE) {
            set_error("%s: the handle's kernel is not a squared exponential, it has no rank-64 form (gpirt_kernel_check(kernel, 64))", me);
            return GPIRT_E_ARG;
        }
        const int rc = kernel_rank_check(s->kern, AMP_CENTRED_RANK, nullptr, nullptr);      // (its message names the length scale)
        if (rc) return rc;
        set_error("%s: the length-scale grid's smallest value fails gpirt_kernel_check(kernel, 64)", me);
        return GPIRT_E_ARG;
    }
    if (!s->theta_ok) {
        set_error("%s: a theta is not finite or lies outside [-5, 5], the rank-64 basis does not hold there", me);
        return GPIRT_E_ARG;
    }
    // mu of a held-back draw_beta, and nothing on the sampler's own stream may still read the f this update rewrites in place
    GP_TRY(beta_sync(s));
    s->lp_current = false;
    s->mu_linear = false;
    GP_TRY(amp_centred_alloc(s));
    GP_TRY(smooth_factor(s));
    AmpCentredArgs a = A.ca;
    a.F = s->sf.F; a.live = s->sf.live; a.r = s->sf.r;
    a.f = s->f; a.mu = s->mu; a.y = s->y; a.n = s->n; a.m = s->m;
    a.theta = s->theta; a.eps = GPIRT_JITTER;
    a.H = s->NU;                                  // draw_f's prior draw: free between steps
    a.grid = A.d_grid; a.log_prior = A.d_log_prior; a.P = A.P;
    a.idx = A.idx; a.amp = A.amp;
    a.seed = s->opt.seed; a.t = A.ct + 1; a.item0 = (uint32_t)s->opt.item0;
    a.err = s->flags;
    hipStream_t st = s->h->stream;
    const bool timed = s->timing;
    if (timed) {
        for (hipEvent_t& t : A.ctev) if (!t) GP_HIP(hipEventCreate(&t));
        GP_HIP(hipEventRecord(A.ctev[0], st));
    }
    GP_TRY(launch_amp_centred(st, a));
    A.ct += 1;
    if (timed) {                              // (timing on: one synchronisation, as the whitened update's)
        GP_HIP(hipEventRecord(A.ctev[1], st));
        GP_HIP(hipEventSynchronize(A.ctev[1]));
        float ms = 0.f;
        hipEventElapsedTime(&ms, A.ctev[0], A.ctev[1]);
        A.clast_ms = ms;
    }
    return 0;
}

int gpirt_sampler_amp_centred_stats(gpirt_sampler_t s, gpirt_amp_centred* out)
{
    GP_ARG(s && out);
    const AmpState& A = s->amp;
    memset(out, 0, sizeof(*out));
    out->calls = A.ct; out->accept_rate = (double)NAN; out->last_ms = A.clast_ms;
    if (A.mode != 2 || !A.cbuf) return 0;
    out->rank = s->sf.have ? s->sf.r : 0;
    const int64_t m = s->m;
    std::vector<long long> cnt(4 * (size_t)m);
    hipStream_t st = s->h->stream;
    GP_HIP(hipMemcpyAsync(cnt.data(), A.ca.counts, sizeof(long long) * 4 * (size_t)m, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    for (int64_t j = 0; j < m; ++j) {
        out->updates += cnt[(size_t)j]; out->accepted += cnt[(size_t)(m + j)];
        out->same += cnt[(size_t)(2 * m + j)]; out->failed += cnt[(size_t)(3 * m + j)];
    }
    const int64_t decided = out->updates - out->same - out->failed;
    if (decided > 0) out->accept_rate = (double)out->accepted / (double)decided;
    return 0;
}

// ---- the centred beta update (beta_centred.hip) ----------------------------------------------------------------------------------
// the buffers of the first call: one allocation, zeroed (counters and record too), the nodes and weights of the basis.  Drains
// the handle's stream.
static int beta_centred_alloc(gpirt_sampler_t s)
{
    BetaCentredState& Bc = s->bc;
    if (Bc.buf) return 0;
    const size_t n = (size_t)s->n, m = (size_t)s->m, R = BETA_CENTRED_RANK, RR = R * R;
    const size_t sizes[] = { n * R, RR, (size_t)KSPLIT * RR, RR, RR, 2 * R, 2 * R, 2 * n, 4, 2 * m, 2 * m, 2 * m, 2 * m, 2 * m, 3 * m, m, 2 * m, R, R };
    size_t total = 0;
    for (size_t sz : sizes) total += sz;
    double* buf = nullptr;
    GP_TRY(dalloc(s, &buf, total, false));
    double* p = buf;
    auto take = [&](size_t sz) { double* q = p; p += sz; return q; };
    BetaCentredArgs& c = Bc.a;
    c = BetaCentredArgs();
    c.V = take(sizes[0]); c.Gv = take(sizes[1]); c.parts = take(sizes[2]); c.Xh = take(sizes[3]); c.R = take(sizes[4]);
    c.P = take(sizes[5]); c.Gx = take(sizes[6]); c.W = take(sizes[7]); c.B = take(sizes[8]);
    c.T = take(sizes[9]); c.Z = take(sizes[10]); c.mean = take(sizes[11]); c.beta_old = take(sizes[12]); c.beta_new = take(sizes[13]);
    c.chol = take(sizes[14]); c.rec = take(sizes[15]);
    c.counts = reinterpret_cast<long long*>(take(sizes[16]));
    double* nodes = take(sizes[17]); double* wts = take(sizes[18]);
    c.nodes = nodes; c.wts = wts;
    c.nsplit = KSPLIT;
    std::vector<double> hn, hw;
    nu_lr_nodes(hn, hw);
    hipStream_t st = s->h->stream;
    if (hipMemsetAsync(buf, 0, sizeof(double) * total, st) != hipSuccess ||
        hipMemcpyAsync(nodes, hn.data(), sizeof(double) * R, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(wts, hw.data(), sizeof(double) * R, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        set_error("beta (centred): the upload failed");              // (the buffer stays in `allocs`; the next call tries again)
        return GPIRT_E_HIP;
    }
    Bc.buf = buf;
    return 0;
}

int gpirt_sampler_draw_beta_centred(gpirt_sampler_t s)
{
    GP_ARG(s != nullptr);
    const char* me = "gpirt_sampler_draw_beta_centred";
    GP_TRY(ord_refuse(s, "gpirt_sampler_draw_beta_centred", "it moves the intercept, which ordinal responses pin at 0"));
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", me); return GPIRT_E_ARG; }
    if (stream_mode(s)) { set_error("%s: rng = reference (GPIRT_RNG_RSTREAM) is refused, R's stream has no such draw", me); return GPIRT_E_ARG; }
    if (s->opt.kernel_fp32) { set_error("%s: kernel_fp32 is refused, the single-precision build is the default kernel's alone", me); return GPIRT_E_ARG; }
    if (s->opt.item0 != 0 || (s->opt.m_total > 0 && s->opt.m_total != s->m)) {
        set_error("%s: an item shard (item0 = %lld, m_total = %lld) is refused, the shared 2 x 2 matrix is built for all items of one sampler", me,
                  (long long)s->opt.item0, (long long)s->opt.m_total);
        return GPIRT_E_ARG;
    }
    if (!s->nu_kern_ok) {
        if (s->kern.family != GPIRT_KERNEL_SE) {
            set_error("%s: the handle's kernel is not a squared exponential, it has no rank-64 form (gpirt_kernel_check(kernel, 64))", me);
            return GPIRT_E_ARG;
        }
        const int rc = kernel_rank_check(s->kern, BETA_CENTRED_RANK, nullptr, nullptr);     // (its message names the length scale)
        if (rc) return rc;
        set_error("%s: the length-scale grid's smallest value fails gpirt_kernel_check(kernel, 64)", me);
        return GPIRT_E_ARG;
    }
    if (!s->theta_ok) {
        set_error("%s: a theta is not finite or lies outside [-5, 5], the rank-64 basis does not hold there", me);
        return GPIRT_E_ARG;
    }
    BetaCentredState& Bc = s->bc;
    if (Bc.prior_ok < 0) {                        // (the prior is the sampler's for life: looked at once)
        Bc.prior_ok = 1;
        const double* ps = s->host_tmp.data() + 2 * s->m;
        for (int64_t e = 0; e < 2 * s->m; ++e)
            if (!(ps[e] > 0.0) || !(ps[e] <= 1.79769313486231570815e308)) Bc.prior_ok = 0;
    }
    if (!Bc.prior_ok) {
        set_error("%s: a prior sd of beta is not finite and > 0, the conditional has no precision to add", me);
        return GPIRT_E_ARG;
    }
    // a held-back draw_beta writes beta, mu and mu_star, and nothing on the sampler's own stream may still read what this rewrites
    GP_TRY(beta_sync(s));
    s->lp_current = false;
    s->mu_linear = false;
    GP_TRY(beta_centred_alloc(s));
    GP_TRY(smooth_factor(s));
    BetaCentredArgs a = Bc.a;
    a.f = s->f; a.beta = s->beta; a.mu = s->mu; a.mu_star = s->mu_star; a.n = s->n; a.m = s->m; a.N = s->N;
    a.theta = s->theta; a.tstar = s->tstar; a.pm = s->pm; a.ps = s->ps;
    a.amp = s->amp.mode ? s->amp.amp : nullptr;
    a.F = s->sf.F; a.eps = GPIRT_JITTER;
    a.seed = s->opt.seed; a.t = Bc.t + 1; a.item0 = (uint32_t)s->opt.item0;
    a.err = s->flags;
    hipStream_t st = s->h->stream;
    const bool timed = s->timing;
    if (timed) {
        for (hipEvent_t& t : Bc.tev) if (!t) GP_HIP(hipEventCreate(&t));
        GP_HIP(hipEventRecord(Bc.tev[0], st));
        a.kev[0] = Bc.tev[2]; a.kev[1] = Bc.tev[3];
    }
    GP_TRY(launch_beta_centred(st, a));
    Bc.t += 1;
    if (timed) {                              // (timing on: one synchronisation, as the amplitude updates')
        GP_HIP(hipEventRecord(Bc.tev[1], st));
        GP_HIP(hipEventSynchronize(Bc.tev[1]));
        float ms = 0.f;
        hipEventElapsedTime(&ms, Bc.tev[0], Bc.tev[1]);
        Bc.last_ms = ms;
        hipEventElapsedTime(&ms, Bc.tev[2], Bc.tev[3]);
        Bc.item_ms = ms;
    }
    return 0;
}

int gpirt_sampler_beta_centred_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    GP_ARG(s && name && h_out);
    BetaCentredState& Bc = s->bc;
    if (strcmp(name, "time") == 0 || strcmp(name, "time_item") == 0) {
        if (bytes != 8) { set_error("beta (centred): '%s' holds 8 bytes, %lld were asked for", name, (long long)bytes); return GPIRT_E_ARG; }
        memcpy(h_out, name[4] ? &Bc.item_ms : &Bc.last_ms, 8);
        return 0;
    }
    GP_TRY(needs(Bc.buf != nullptr && Bc.t > 0, "the centred beta update's arrays are", "one gpirt_sampler_draw_beta_centred call"));
    const BetaCentredArgs& c = Bc.a;
    const int64_t n = s->n, m = s->m, R = BETA_CENTRED_RANK;
    const void* dev = nullptr;
    int64_t want = 0;
    if (strcmp(name, "W") == 0) { dev = c.W; want = 8 * 2 * n; }
    else if (strcmp(name, "B") == 0) { dev = c.B; want = 8 * 4; }
    else if (strcmp(name, "P") == 0) { dev = c.P; want = 8 * 2 * R; }
    else if (strcmp(name, "Gx") == 0) { dev = c.Gx; want = 8 * 2 * R; }
    else if (strcmp(name, "T") == 0) { dev = c.T; want = 8 * 2 * m; }
    else if (strcmp(name, "z") == 0) { dev = c.Z; want = 8 * 2 * m; }
    else if (strcmp(name, "mean") == 0) { dev = c.mean; want = 8 * 2 * m; }
    else if (strcmp(name, "beta_old") == 0) { dev = c.beta_old; want = 8 * 2 * m; }
    else if (strcmp(name, "beta_new") == 0) { dev = c.beta_new; want = 8 * 2 * m; }
    else if (strcmp(name, "chol") == 0) { dev = c.chol; want = 8 * 3 * m; }
    else if (strcmp(name, "record") == 0) { dev = c.rec; want = 8 * m; }
    else if (strcmp(name, "counts") == 0) { dev = c.counts; want = 8 * 2 * m; }
    else { set_error("unknown centred beta array '%s'", name); return GPIRT_E_ARG; }
    if (bytes != want) { set_error("beta (centred): '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes); return GPIRT_E_ARG; }
    hipStream_t st = s->h->stream;
    GP_HIP(hipMemcpyAsync(h_out, dev, (size_t)want, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

int gpirt_sampler_beta_centred_stats(gpirt_sampler_t s, gpirt_beta_centred* out)
{
    GP_ARG(s && out);
    const BetaCentredState& Bc = s->bc;
    memset(out, 0, sizeof(*out));
    out->calls = Bc.t; out->last_ms = Bc.last_ms;
    if (!Bc.buf) return 0;
    out->rank = s->sf.have ? s->sf.r : 0;
    const int64_t m = s->m;
    std::vector<long long> cnt(2 * (size_t)m);
    hipStream_t st = s->h->stream;
    GP_HIP(hipMemcpyAsync(cnt.data(), Bc.a.counts, sizeof(long long) * 2 * (size_t)m, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    for (int64_t j = 0; j < m; ++j) { out->updates += cnt[(size_t)j]; out->failed += cnt[(size_t)(m + j)]; }
    return 0;
}

// ---- the collapsed scale and shift move (scale.hip) ------------------------------------------------------------------------------
static const char* const SCALE_KIND_NAME[2] = { "scale", "shift" };

static int scale_width_check(const char* me, int kind, double w)
{
    if (!(w >= 0.0) || !(w <= 1.79769313486231570815e308)) {
        set_error("%s: the %s width = %g, it must be finite and >= 0", me, SCALE_KIND_NAME[kind], w);
        return GPIRT_E_ARG;
    }
    return 0;
}

// what gpirt_sampler_scale_enable and gpirt_sampler_draw_scale both refuse, each with its reason
static int scale_refusals(gpirt_sampler_t s, const char* me)
{
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", me); return GPIRT_E_ARG; }
    if (stream_mode(s)) { set_error("%s: rng = reference (GPIRT_RNG_RSTREAM) is refused, R's stream has no such draw", me); return GPIRT_E_ARG; }
    if (s->opt.item0 != 0 || (s->opt.m_total > 0 && s->opt.m_total != s->m)) {
        set_error("%s: an item shard (item0 = %lld, m_total = %lld) is refused, logpost then holds only part of the items", me,
                  (long long)s->opt.item0, (long long)s->opt.m_total);
        return GPIRT_E_ARG;
    }
    if (s->fstar_full) {
        set_error("%s is refused while gpirt_sampler_set_theta_block is in use: logpost then holds only part of the items", me);
        return GPIRT_E_ARG;
    }
    ScaleState& Sc = s->sc;
    if (Sc.prior_ok < 0) {                        // (the prior is the sampler's for life: looked at once)
        Sc.prior_ok = 1;
        const double* ps = s->host_tmp.data() + 2 * s->m;
        for (int64_t e = 0; e < 2 * s->m; ++e)
            if (!(ps[e] > 0.0) || !(ps[e] <= 1.79769313486231570815e308)) Sc.prior_ok = 0;
    }
    if (!Sc.prior_ok) {
        set_error("%s: a prior sd of beta is not finite and > 0, the move's prior ratio is not defined", me);
        return GPIRT_E_ARG;
    }
    return 0;
}

int gpirt_sampler_scale_enable(gpirt_sampler_t s, double w_scale, double w_shift)
{
    GP_ARG(s != nullptr);
    const char* me = "gpirt_sampler_scale_enable";
    GP_TRY(scale_refusals(s, me));
    // the defaults: a choice, not a measurement (the sum of n respondents' dlz has a curvature of order n)
    const double dflt = 1.0 / sqrt((double)s->n);
    if (w_scale != w_scale) w_scale = dflt;
    if (w_shift != w_shift) w_shift = dflt;
    GP_TRY(scale_width_check(me, 0, w_scale));
    GP_TRY(scale_width_check(me, 1, w_shift));
    ScaleState& Sc = s->sc;
    if (!Sc.on) {
        const size_t n = (size_t)s->n, m = (size_t)s->m, N = (size_t)s->N;
        ScaleArgs& a = Sc.a;
        a = ScaleArgs();
        GP_TRY(dalloc(s, &a.fstar2, N * m + 2));
        GP_TRY(dalloc(s, &a.mu2, N * m + 2));
        GP_TRY(dalloc(s, &a.logpost2, N * n + 2));
        GP_TRY(dalloc(s, &a.beta_prop, 2 * m));
        double* vec = nullptr;
        GP_TRY(dalloc(s, &vec, 3 * n + SCALE_REC_COUNT, false));
        a.lz = vec; a.lz_prop = vec + n; a.dlz = vec + 2 * n; a.rec = vec + 3 * n;
        GP_TRY(dalloc(s, &a.bad, n));
        GP_TRY(dalloc(s, &a.counts, 6));
        hipStream_t st = s->h->stream;
        GP_HIP(hipMemsetAsync(vec, 0, sizeof(double) * (3 * n + SCALE_REC_COUNT), st));
        GP_HIP(hipMemsetAsync(a.bad, 0, sizeof(int) * n, st));
        GP_HIP(hipMemsetAsync(a.counts, 0, sizeof(long long) * 6, st));
        Sc.on = true;
    }
    Sc.width[0] = w_scale; Sc.width[1] = w_shift;
    return 0;
}

int gpirt_sampler_scale_width(gpirt_sampler_t s, int kind, double w)
{
    GP_ARG(s != nullptr);
    const char* me = "gpirt_sampler_scale_width";
    GP_TRY(needs(s->sc.on, "the scale and shift move is", "gpirt_sampler_scale_enable"));
    if (kind != 0 && kind != 1) { set_error("%s: kind = %d, it must be 0 (scale) or 1 (shift)", me, kind); return GPIRT_E_ARG; }
    GP_TRY(scale_width_check(me, kind, w));
    s->sc.width[kind] = w;
    return 0;
}

// one proposal of the kind on the main stream; nothing is read back.  timed: its events are recorded, the caller reads them
static int do_draw_scale(gpirt_sampler_t s, int kind, const char* me, bool timed)
{
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", me); return GPIRT_E_ARG; }
    GP_TRY(needs(s->sc.on, "the scale and shift move is", "gpirt_sampler_scale_enable"));
    GP_TRY(scale_refusals(s, me));
    if (kind != 0 && kind != 1) { set_error("%s: kind = %d, it must be 0 (scale) or 1 (shift)", me, kind); return GPIRT_E_ARG; }
    // a held-back draw_beta writes beta, mu and mu_star (and with them makes logpost stale): it runs first
    GP_TRY(beta_sync(s));
    if (!s->lp_current) {
        set_error("%s: logpost is not current, the move belongs between gpirt_sampler_theta_partial and gpirt_sampler_theta_finish "
                  "(a stage that writes fstar, beta, f, theta or the population prior ran since the last theta_partial)", me);
        return GPIRT_E_ARG;
    }
    ScaleState& Sc = s->sc;
    ScaleArgs a = Sc.a;
    a.beta = s->beta; a.mu = s->mu; a.mu_star = s->mu_star; a.fstar = s->fstar; a.logpost = s->logpost;
    a.gbar = s->shape.on ? s->shape.gbar : nullptr;
    a.n = s->n; a.m = s->m; a.N = s->N; a.theta = s->theta; a.pm = s->pm; a.ps = s->ps;
    if (s->pop.mode) { a.log_prior = s->pop.log_prior; a.codes = s->pop.codes; }
    a.kind = kind; a.width = Sc.width[kind]; a.seed = s->opt.seed; a.t = Sc.t[kind] + 1;
    hipStream_t st = s->h->stream;
    if (timed) {
        for (hipEvent_t& t : Sc.tev) if (!t) GP_HIP(hipEventCreate(&t));
        GP_HIP(hipEventRecord(Sc.tev[0], st));
        for (int k = 0; k < 4; ++k) a.kev[k] = Sc.tev[3 + k];
    }
    s->mu_linear = false;                         // (an accepted move rewrites beta and mu on the device: the host cannot know)
    GP_TRY(launch_scale_curve(st, a));
    if (timed) GP_HIP(hipEventRecord(Sc.tev[1], st));
    GP_TRY(theta_product(s, a.fstar2, a.logpost2));
    if (timed) GP_HIP(hipEventRecord(Sc.tev[2], st));
    GP_TRY(launch_scale_decide(st, a));
    Sc.t[kind] += 1;
    Sc.last_kind = kind;
    return 0;                                     // (lp_current stays: logpost is the standing curve's either way)
}

static int scale_read_times(gpirt_sampler_t s)
{
    ScaleState& Sc = s->sc;
    GP_HIP(hipEventSynchronize(Sc.tev[6]));
    float ms = 0.f;
    hipEventElapsedTime(&ms, Sc.tev[0], Sc.tev[6]); Sc.times[0] = ms;
    hipEventElapsedTime(&ms, Sc.tev[0], Sc.tev[1]); Sc.times[1] = ms;
    hipEventElapsedTime(&ms, Sc.tev[1], Sc.tev[2]); Sc.times[2] = ms;
    for (int k = 0; k < 3; ++k) { hipEventElapsedTime(&ms, Sc.tev[3 + k], Sc.tev[4 + k]); Sc.times[3 + k] = ms; }
    Sc.last_ms[Sc.last_kind] = Sc.times[0];
    return 0;
}

int gpirt_sampler_draw_scale(gpirt_sampler_t s, int kind)
{
    GP_ARG(s != nullptr);
    GP_TRY(ord_refuse(s, "gpirt_sampler_draw_scale", ORD_BINARY));
    const bool timed = s->timing;
    GP_TRY(do_draw_scale(s, kind, "gpirt_sampler_draw_scale", timed));
    if (timed) GP_TRY(scale_read_times(s));      // (timing on: one synchronisation, as the centred updates')
    return 0;
}

// gpirt_sampler_step_consistent with the asked-for kinds between theta_partial and theta_finish (kinds: bit 0 scale, bit 1 shift,
// the scale first)
int gpirt_sampler_step_consistent_scale(gpirt_sampler_t s, int nugget, int kinds)
{
    GP_ARG(s != nullptr);
    if (kinds) GP_TRY(ord_refuse(s, "gpirt_sampler_step_consistent_scale", ORD_BINARY));
    const char* me = "gpirt_sampler_step_consistent_scale";
    GP_TRY(carry_refusals(s, nugget, me));
    if (kinds < 0 || kinds > 3) { set_error("%s: kinds = %d, it is a mask of 1 (scale) and 2 (shift)", me, kinds); return GPIRT_E_ARG; }
    if (kinds) {
        GP_TRY(needs(s->sc.on, "the scale and shift move is", "gpirt_sampler_scale_enable"));
        GP_TRY(scale_refusals(s, me));
    }
    mark(s, 0);
    GP_TRY(do_draw_f(s));            mark(s, 1);
    GP_TRY(do_draw_fstar(s, (uint32_t)(s->iter + 1))); mark(s, 2);
    GP_TRY(do_theta_partial(s));
    for (int kind = 0; kind < 2; ++kind)
        if (kinds & (1 << kind)) GP_TRY(do_draw_scale(s, kind, me, false));
    mark(s, 3);
    GP_TRY(do_theta_finish(s));      mark(s, 4);
    GP_TRY(do_carry_f(s, nugget, s->timing));
    GP_TRY(do_draw_beta(s));         mark(s, 5);
    GP_TRY(do_factor(s));            mark(s, 6);
    s->iter += 1;
    if (s->timing) {
        GP_HIP(hipEventSynchronize(s->ev[ST_COUNT]));
        for (int i = 0; i < ST_COUNT; ++i) {
            float ms = 0.f;
            hipEventElapsedTime(&ms, i == ST_BETA ? s->carry.tev[1] : s->ev[i], s->ev[i + 1]);
            s->stage_ms[i] = ms;                  // (the moves' time is inside theta_partial's)
        }
        float ms = 0.f;
        hipEventElapsedTime(&ms, s->carry.tev[0], s->carry.tev[1]);
        s->carry.last_ms = ms;
    }
    return 0;
}

int gpirt_sampler_scale_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    GP_ARG(s && name && h_out);
    ScaleState& Sc = s->sc;
    GP_TRY(needs(Sc.on, "the scale and shift move's arrays are", "gpirt_sampler_scale_enable"));
    const ScaleArgs& c = Sc.a;
    const int64_t n = s->n, m = s->m, N = s->N;
    const void* dev = nullptr;
    const void* host = nullptr;
    int64_t want = 0;
    if (strcmp(name, "times") == 0) { host = Sc.times; want = 8 * 6; }
    else if (strcmp(name, "counts") == 0) { dev = c.counts; want = 8 * 6; }
    else if (strcmp(name, "logpost") == 0) { dev = s->logpost; want = 8 * N * n; }
    else {
        GP_TRY(needs(Sc.last_kind >= 0, "the scale and shift move's arrays are", "one gpirt_sampler_draw_scale call"));
        if (strcmp(name, "record") == 0) { dev = c.rec; want = 8 * SCALE_REC_COUNT; }
        else if (strcmp(name, "lz") == 0) { dev = c.lz; want = 8 * n; }
        else if (strcmp(name, "lz_prop") == 0) { dev = c.lz_prop; want = 8 * n; }
        else if (strcmp(name, "dlz") == 0) { dev = c.dlz; want = 8 * n; }
        else if (strcmp(name, "beta_prop") == 0) { dev = c.beta_prop; want = 8 * 2 * m; }
        else if (strcmp(name, "mu_prop") == 0) { dev = c.mu2; want = 8 * N * m; }
        else if (strcmp(name, "fstar_prop") == 0) { dev = c.fstar2; want = 8 * N * m; }
        else if (strcmp(name, "logpost_prop") == 0) { dev = c.logpost2; want = 8 * N * n; }
        else { set_error("unknown scale array '%s'", name); return GPIRT_E_ARG; }
    }
    if (bytes != want) { set_error("scale: '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes); return GPIRT_E_ARG; }
    if (host) { memcpy(h_out, host, (size_t)want); return 0; }
    hipStream_t st = s->h->stream;
    GP_HIP(hipMemcpyAsync(h_out, dev, (size_t)want, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    return 0;
}

int gpirt_sampler_scale_stats(gpirt_sampler_t s, gpirt_scale* out)
{
    GP_ARG(s && out);
    const ScaleState& Sc = s->sc;
    memset(out, 0, sizeof(*out));
    out->on = Sc.on ? 1 : 0;
    for (int k = 0; k < 2; ++k) { out->calls[k] = Sc.t[k]; out->width[k] = Sc.width[k]; out->last_ms[k] = Sc.last_ms[k]; }
    if (!Sc.on) return 0;
    long long cnt[6];
    hipStream_t st = s->h->stream;
    GP_HIP(hipMemcpyAsync(cnt, Sc.a.counts, sizeof(cnt), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 2; ++k) { out->accepted[k] = cnt[2 + k]; out->failed[k] = cnt[4 + k]; }
    return 0;
}

// ---- the population prior for theta --------------------------------------------------------------------------------------------
static int pop_refusals(gpirt_sampler_t s, const char* entry)
{
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", entry); return GPIRT_E_ARG; }
    if (s->fstar_full) {
        set_error("%s is refused while gpirt_sampler_set_theta_block is in use: the block path would need the codes of its respondents", entry);
        return GPIRT_E_ARG;
    }
    if (s->opt.m_total > 0 && s->opt.m_total != s->m) {
        set_error("population prior: an item shard (item0 = %lld, m_total = %lld) is refused, the respondent-block theta path "
                  "would need the codes of its respondents", (long long)s->opt.item0, (long long)s->opt.m_total);
        return GPIRT_E_ARG;
    }
    return 0;
}

int gpirt_sampler_pop_set(gpirt_sampler_t s, const int32_t* codes, int G, const double* log_prior)
{
    GP_ARG(s != nullptr);
    PopState& A = s->pop;
    s->lp_current = false;
    s->mu_linear = false;
    if (!codes) {
        if (A.mode == 2) { set_error("gpirt_sampler_pop_set(NULL): the population prior is sampled, gpirt_sampler_pop_enable(on = 0) turns it off"); return GPIRT_E_ARG; }
        GP_HIP(hipStreamSynchronize(s->h->stream));
        pop_free(&A);
        return 0;
    }
    if (A.mode == 2) {
        set_error("gpirt_sampler_pop_set after gpirt_sampler_pop_enable: turn the sampled population prior off first (on = 0)");
        return GPIRT_E_ARG;
    }
    GP_ARG(log_prior != nullptr);
    GP_TRY(pop_refusals(s, "gpirt_sampler_pop_set"));
    const int64_t n = s->n, N = s->N;
    GP_TRY(gpirt_pop_check(codes, n, G, log_prior, G, 0, 0.0, 0, 0.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr, &s->opt));
    hipStream_t st = s->h->stream;
    GP_HIP(hipStreamSynchronize(st));
    pop_free(&A);
    if (hipMalloc((void**)&A.codes, sizeof(int32_t) * (size_t)n) != hipSuccess ||
        hipMalloc((void**)&A.log_prior, sizeof(double) * (size_t)G * (size_t)N) != hipSuccess) {
        set_error("population prior: hipMalloc failed");
        pop_free(&A);
        return GPIRT_E_ALLOC;
    }
    if (hipMemcpyAsync(A.codes, codes, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.log_prior, log_prior, sizeof(double) * (size_t)G * (size_t)N, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        set_error("population prior: the upload failed");
        pop_free(&A);
        return GPIRT_E_HIP;
    }
    A.G = G;
    A.mode = 1;
    return 0;
}

int gpirt_sampler_pop_enable(gpirt_sampler_t s, const int32_t* codes, int G, const double* anchor_row, double mu_hi, int P_mu,
                             double sd_lo, double sd_hi, int P_sd, const double* log_hyper_mu, const double* log_hyper_sd,
                             const int* a0, const int* b0, int64_t planned_draws, int on)
{
    GP_ARG(s != nullptr);
    PopState& A = s->pop;
    s->lp_current = false;
    s->mu_linear = false;
    if (!on) {
        if (A.mode == 1) { set_error("gpirt_sampler_pop_enable(on = 0): the population prior is fixed, gpirt_sampler_pop_set(NULL) turns it off"); return GPIRT_E_ARG; }
        GP_HIP(hipStreamSynchronize(s->h->stream));
        pop_free(&A);
        return 0;
    }
    if (A.mode == 1) {
        set_error("gpirt_sampler_pop_enable after gpirt_sampler_pop_set: turn the fixed population prior off first (gpirt_sampler_pop_set(NULL))");
        return GPIRT_E_ARG;
    }
    GP_ARG(codes != nullptr);
    GP_TRY(pop_refusals(s, "gpirt_sampler_pop_enable"));
    const int64_t n = s->n, N = s->N;
    GP_TRY(gpirt_pop_check(codes, n, G, anchor_row, anchor_row ? 1 : 0, 1, mu_hi, P_mu, sd_lo, sd_hi, P_sd, log_hyper_mu, log_hyper_sd,
                           a0, b0, &s->opt));
    if (planned_draws < 0 || planned_draws > (int64_t)1 << 31) {
        set_error("population prior: planned_draws = %lld, it must lie in 0 .. 2^31", (long long)planned_draws);
        return GPIRT_E_ARG;
    }
    hipStream_t st = s->h->stream;
    GP_HIP(hipStreamSynchronize(st));
    pop_free(&A);
    auto fail = [&](int rc, const char* what) { set_error("population prior: %s failed", what); pop_free(&A); return rc; };
    const size_t Gs = (size_t)G, Pm = (size_t)P_mu, Ps = (size_t)P_sd;
    const size_t draw_bytes = sizeof(int32_t) * (size_t)(planned_draws ? planned_draws : 1) * 2 * Gs;
    if (hipMalloc((void**)&A.codes, sizeof(int32_t) * (size_t)n) != hipSuccess ||
        hipMalloc((void**)&A.log_prior, sizeof(double) * Gs * (size_t)N) != hipSuccess ||
        hipMalloc((void**)&A.d_mu, sizeof(double) * Pm) != hipSuccess ||
        hipMalloc((void**)&A.d_sd, sizeof(double) * Ps) != hipSuccess ||
        hipMalloc((void**)&A.d_lse, sizeof(double) * Pm * Ps) != hipSuccess ||
        hipMalloc((void**)&A.d_hyper_mu, sizeof(double) * Pm) != hipSuccess ||
        hipMalloc((void**)&A.d_hyper_sd, sizeof(double) * Ps) != hipSuccess ||
        hipMalloc((void**)&A.lp_mu, sizeof(double) * Gs * Pm) != hipSuccess ||
        hipMalloc((void**)&A.lp_sd, sizeof(double) * Gs * Ps) != hipSuccess ||
        hipMalloc((void**)&A.idx, sizeof(int) * 2 * Gs) != hipSuccess ||
        hipMalloc((void**)&A.stats, sizeof(long long) * 4 * Gs) != hipSuccess ||
        hipMalloc((void**)&A.counts, sizeof(long long) * 4 * Gs) != hipSuccess ||
        hipMalloc((void**)&A.hist_mu, sizeof(uint32_t) * Pm * Gs) != hipSuccess ||
        hipMalloc((void**)&A.hist_sd, sizeof(uint32_t) * Ps * Gs) != hipSuccess ||
        hipMalloc((void**)&A.draws, draw_bytes) != hipSuccess) return fail(GPIRT_E_ALLOC, "hipMalloc");
    A.G = G; A.P_mu = P_mu; A.P_sd = P_sd; A.planned = planned_draws; A.recorded = 0;
    A.mu_hi = mu_hi; A.sd_lo = sd_lo; A.sd_hi = sd_hi;
    A.mu.resize(Pm); A.sd.resize(Ps); A.lse.resize(Pm * Ps);
    A.hyper_mu.assign(Pm, 0.0); A.hyper_sd.assign(Ps, 0.0);
    pop_grids_fill(mu_hi, P_mu, sd_lo, sd_hi, P_sd, A.mu.data(), A.sd.data());
    pop_lse_fill(A.mu.data(), P_mu, A.sd.data(), P_sd, A.lse.data());
    if (log_hyper_mu) A.hyper_mu.assign(log_hyper_mu, log_hyper_mu + Pm);
    if (log_hyper_sd) A.hyper_sd.assign(log_hyper_sd, log_hyper_sd + Ps);
    const int near1 = amp_nearest_one(A.sd.data(), P_sd);
    std::vector<int> idx(2 * Gs, -1);
    std::vector<double> table(Gs * (size_t)N);
    if (anchor_row) memcpy(table.data(), anchor_row, sizeof(double) * (size_t)N);
    else pop_default_row(table.data());
    for (int g = 1; g < G; ++g) {
        const int a = a0 ? a0[g] : (P_mu - 1) / 2, b = b0 ? b0[g] : near1;
        idx[2 * (size_t)g] = a; idx[2 * (size_t)g + 1] = b;
        pop_normal_row(A.mu[(size_t)a], A.sd[(size_t)b], table.data() + (size_t)g * (size_t)N);
    }
    if (hipMemcpyAsync(A.codes, codes, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.log_prior, table.data(), sizeof(double) * Gs * (size_t)N, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.d_mu, A.mu.data(), sizeof(double) * Pm, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.d_sd, A.sd.data(), sizeof(double) * Ps, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.d_lse, A.lse.data(), sizeof(double) * Pm * Ps, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.d_hyper_mu, A.hyper_mu.data(), sizeof(double) * Pm, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.d_hyper_sd, A.hyper_sd.data(), sizeof(double) * Ps, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.idx, idx.data(), sizeof(int) * 2 * Gs, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(A.lp_mu, 0, sizeof(double) * Gs * Pm, st) != hipSuccess ||
        hipMemsetAsync(A.lp_sd, 0, sizeof(double) * Gs * Ps, st) != hipSuccess ||
        hipMemsetAsync(A.stats, 0, sizeof(long long) * 4 * Gs, st) != hipSuccess ||
        hipMemsetAsync(A.counts, 0, sizeof(long long) * 4 * Gs, st) != hipSuccess ||
        hipMemsetAsync(A.hist_mu, 0, sizeof(uint32_t) * Pm * Gs, st) != hipSuccess ||
        hipMemsetAsync(A.hist_sd, 0, sizeof(uint32_t) * Ps * Gs, st) != hipSuccess ||
        hipMemsetAsync(A.draws, 0, draw_bytes, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return fail(GPIRT_E_HIP, "the upload");      // (the host vectors go out of scope)
    A.mode = 2;
    return 0;
}

int gpirt_sampler_draw_pop(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    PopState& A = s->pop;
    GP_TRY(needs(A.mode == 2, "the population prior's update is", "gpirt_sampler_pop_enable"));
    s->lp_current = false;
    s->mu_linear = false;
    PopUpdateArgs a{};
    a.stats = A.stats; a.mu = A.d_mu; a.sd = A.d_sd; a.P_mu = A.P_mu; a.P_sd = A.P_sd;
    a.hyper_mu = A.d_hyper_mu; a.hyper_sd = A.d_hyper_sd; a.lse = A.d_lse;
    a.idx = A.idx; a.lp_mu = A.lp_mu; a.lp_sd = A.lp_sd; a.log_prior = A.log_prior; a.counts = A.counts;
    a.G = A.G; a.N = (int)s->N; a.seed = s->opt.seed; a.t = A.t + 1;
    hipStream_t st = s->h->stream;              // (theta is written on this stream alone; nothing else writes the table)
    const bool timed = s->timing;
    if (timed) {
        for (hipEvent_t& t : A.tev) if (!t) GP_HIP(hipEventCreate(&t));
        GP_HIP(hipEventRecord(A.tev[0], st));
    }
    GP_TRY(launch_pop_stats(st, s->theta, A.codes, s->n, A.G, A.stats));
    GP_TRY(launch_pop_update(st, a));
    A.t += 1;
    if (timed) {                              // (timing on: one synchronisation, as the amplitude update's)
        GP_HIP(hipEventRecord(A.tev[1], st));
        GP_HIP(hipEventSynchronize(A.tev[1]));
        float ms = 0.f;
        hipEventElapsedTime(&ms, A.tev[0], A.tev[1]);
        A.last_ms = ms;
    }
    return 0;
}

int gpirt_sampler_pop_record(gpirt_sampler_t s)
{
    GP_ARG(s != nullptr);
    PopState& A = s->pop;
    GP_TRY(needs(A.mode == 2, "the population prior's update is", "gpirt_sampler_pop_enable"));
    if (A.recorded >= A.planned) {
        set_error("population prior: all %lld planned draws are recorded", (long long)A.planned);
        return GPIRT_E_ARG;
    }
    GP_TRY(launch_pop_record(s->h->stream, A.idx, A.G, A.P_mu, A.P_sd, A.recorded, A.hist_mu, A.hist_sd, A.draws));
    A.recorded += 1;
    return 0;
}

int gpirt_sampler_pop_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    GP_ARG(s && name && h_out && bytes >= 0);
    PopState& A = s->pop;
    GP_TRY(needs(A.mode != 0, "a population prior is", "gpirt_sampler_pop_set, gpirt_sampler_pop_enable"));
    const int64_t n = s->n, N = s->N, G = A.G, Pm = A.P_mu, Ps = A.P_sd;
    const void* host = nullptr; const void* dev = nullptr; int64_t want = 0;
    const bool both = strcmp(name, "codes") == 0 || strcmp(name, "log_prior") == 0;
    if (!both) GP_TRY(needs(A.mode == 2, "the population prior's update is", "gpirt_sampler_pop_enable"));
    if (strcmp(name, "codes") == 0) { dev = A.codes; want = 4 * n; }
    else if (strcmp(name, "log_prior") == 0) { dev = A.log_prior; want = 8 * G * N; }
    else if (strcmp(name, "mu_grid") == 0) { host = A.mu.data(); want = 8 * Pm; }
    else if (strcmp(name, "sd_grid") == 0) { host = A.sd.data(); want = 8 * Ps; }
    else if (strcmp(name, "lse") == 0) { host = A.lse.data(); want = 8 * Pm * Ps; }
    else if (strcmp(name, "log_hyper_mu") == 0) { host = A.hyper_mu.data(); want = 8 * Pm; }
    else if (strcmp(name, "log_hyper_sd") == 0) { host = A.hyper_sd.data(); want = 8 * Ps; }
    else if (strcmp(name, "index") == 0) { dev = A.idx; want = 8 * G; }
    else if (strcmp(name, "stats") == 0) { dev = A.stats; want = 24 * G; }
    else if (strcmp(name, "off_grid") == 0) { dev = A.stats + 3 * G; want = 8 * G; }
    else if (strcmp(name, "lp_mu") == 0) { dev = A.lp_mu; want = 8 * G * Pm; }
    else if (strcmp(name, "lp_sd") == 0) { dev = A.lp_sd; want = 8 * G * Ps; }
    else if (strcmp(name, "counts") == 0) { dev = A.counts; want = 32 * G; }
    else if (strcmp(name, "hist_mu") == 0) { dev = A.hist_mu; want = 4 * Pm * G; }
    else if (strcmp(name, "hist_sd") == 0) { dev = A.hist_sd; want = 4 * Ps * G; }
    else if (strcmp(name, "draws") == 0) { dev = A.draws; want = 8 * A.recorded * G; }
    else if (strcmp(name, "time") == 0) { host = &A.last_ms; want = 8; }
    else { set_error("unknown population-prior array '%s'", name); return GPIRT_E_ARG; }
    if (bytes != want) { set_error("population prior: '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes); return GPIRT_E_ARG; }
    if (want == 0) return 0;
    if (host) { memcpy(h_out, host, (size_t)want); return 0; }
    GP_HIP(hipMemcpyAsync(h_out, dev, (size_t)want, hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

int gpirt_sampler_pop_stats(gpirt_sampler_t s, gpirt_pop* out)
{
    GP_ARG(s && out);
    const PopState& A = s->pop;
    memset(out, 0, sizeof(*out));
    out->on = A.mode; out->groups = A.G; out->n = s->n; out->calls = A.t;
    out->mu_hi = out->sd_lo = out->sd_hi = (double)NAN;
    if (A.mode != 2) return 0;
    const size_t G = (size_t)A.G;
    std::vector<long long> cnt(4 * G), stats(4 * G);
    hipStream_t st = s->h->stream;
    GP_HIP(hipMemcpyAsync(cnt.data(), A.counts, sizeof(long long) * 4 * G, hipMemcpyDeviceToHost, st));
    GP_HIP(hipMemcpyAsync(stats.data(), A.stats, sizeof(long long) * 4 * G, hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    out->points_mu = A.P_mu; out->points_sd = A.P_sd; out->planned_draws = A.planned; out->recorded = A.recorded;
    out->mu_hi = A.mu_hi; out->sd_lo = A.sd_lo; out->sd_hi = A.sd_hi; out->last_ms = A.last_ms;
    for (size_t g = 0; g < G; ++g) {
        out->updates += cnt[g]; out->updated += cnt[G + g]; out->skipped += cnt[2 * G + g]; out->failed += cnt[3 * G + g];
        out->off_grid += stats[3 * G + g];
    }
    return 0;
}

// ---- ordinal responses ------------------------------------------------------------------------------------------------------------
int gpirt_sampler_ordinal_enable(gpirt_sampler_t s, const int8_t* cat, int C, double hi, int P, const double* log_prior,
                                 const int32_t* K0, int W, int64_t planned_draws)
{
    GP_ARG(s != nullptr);
    OrdState& A = s->ord;
    const char* me = "gpirt_sampler_ordinal_enable";
    if (!cat) {
        GP_HIP(hipStreamSynchronize(s->h->stream));
        s->lp_current = false;
        ord_free(&A);
        return 0;
    }
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", me); return GPIRT_E_ARG; }
    if (s->fstar_full) {
        set_error("%s is refused while gpirt_sampler_set_theta_block is in use: the respondent-block theta path has no one-hot product", me);
        return GPIRT_E_ARG;
    }
    if (s->opt.m_total > 0 && s->opt.m_total != s->m) {
        set_error("ordinal: an item shard (item0 = %lld, m_total = %lld) is refused, the respondent-block theta path has no one-hot product",
                  (long long)s->opt.item0, (long long)s->opt.m_total);
        return GPIRT_E_ARG;
    }
    if (s->h->cfg.ll_exact == 1) {
        set_error("%s is refused under GPIRT_LL_EXACT=1: the ordinal kernels have the fast term alone", me);
        return GPIRT_E_ARG;
    }
    // the analysis blocks that evaluate the binary likelihood: none may be on
    const char* blk = nullptr;
    if (s->sum.parts & (GPIRT_SUM_PRED | GPIRT_SUM_WAIC)) blk = "the summaries' WAIC / pred parts (gpirt_sampler_summary_enable)";
    else if (s->ppc.on) blk = "the posterior predictive checks (gpirt_sampler_ppc_enable)";
    else if (s->loo.on) blk = "PSIS-LOO (gpirt_sampler_loo_enable)";
    else if (s->score.on) blk = "scoring (gpirt_sampler_score_enable)";
    else if (s->sumscore.on) blk = "the sum-score posteriors (gpirt_sampler_sumscore_enable)";
    else if (s->equate.on) blk = "the score equating (gpirt_sampler_equate_enable)";
    else if (s->groups.on) blk = "the group posteriors (gpirt_sampler_groups_enable)";
    else if (s->acf.on && (s->acf.parts & GPIRT_ACF_LL)) blk = "the ACF's log-likelihood series (gpirt_sampler_acf_enable)";
    if (blk) { set_error("%s is refused while %s are on: they evaluate the binary likelihood of y", me, blk); return GPIRT_E_ARG; }
    const int64_t n = s->n, m = s->m, N = s->N, Np = (N + 127) / 128 * 128;
    if (planned_draws < 0 || planned_draws > (int64_t)1 << 31) {
        set_error("ordinal: planned_draws = %lld, it must lie in 0 .. 2^31", (long long)planned_draws);
        return GPIRT_E_ARG;
    }
    hipStream_t st = s->h->stream;
    GP_TRY(beta_sync(s));                     // (a held-back draw_beta writes beta, mu and mu_star)
    std::vector<double> hy((size_t)(n * m));
    GP_HIP(hipMemcpyAsync(hy.data(), s->y, sizeof(double) * (size_t)(n * m), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    GP_TRY(gpirt_ordinal_check(cat, hy.data(), n, m, C, hi, P, log_prior, K0, W, &s->opt));
    s->lp_current = false;
    ord_free(&A);
    auto fail = [&](int rc, const char* what) { set_error("ordinal: %s failed", what); ord_free(&A); return rc; };
    const size_t rows = (size_t)m * (size_t)(C - 1), Ps = (size_t)P;
    const size_t draw_bytes = sizeof(int32_t) * (size_t)(planned_draws ? planned_draws : 1) * rows;
    if (hipMalloc((void**)&A.cat, (size_t)(n * m)) != hipSuccess ||
        hipMalloc((void**)&A.d_grid, sizeof(double) * Ps) != hipSuccess ||
        hipMalloc((void**)&A.d_log_prior, sizeof(double) * Ps) != hipSuccess ||
        hipMalloc((void**)&A.thr, sizeof(double) * rows) != hipSuccess ||
        hipMalloc((void**)&A.lp, sizeof(double) * rows * GPIRT_ORD_MAX_WIDTH) != hipSuccess ||
        hipMalloc((void**)&A.cum, sizeof(double) * rows * (size_t)N) != hipSuccess ||
        hipMalloc((void**)&A.Y, sizeof(double) * (size_t)n * (size_t)C * (size_t)m) != hipSuccess ||
        hipMalloc((void**)&A.G, sizeof(double) * ((size_t)Np * (size_t)C * (size_t)m + 2)) != hipSuccess ||
        hipMalloc((void**)&A.idx, sizeof(int) * rows) != hipSuccess ||
        hipMalloc((void**)&A.window, sizeof(int) * rows) != hipSuccess ||
        hipMalloc((void**)&A.counts, sizeof(long long) * (size_t)m * (size_t)C) != hipSuccess ||
        hipMalloc((void**)&A.stat, sizeof(long long) * 4) != hipSuccess ||
        hipMalloc((void**)&A.hist, sizeof(uint32_t) * rows * Ps) != hipSuccess ||
        hipMalloc((void**)&A.draws, draw_bytes) != hipSuccess) return fail(GPIRT_E_ALLOC, "hipMalloc");
    A.C = C; A.P = P; A.W = W; A.lp_W = W; A.hi = hi; A.planned = planned_draws; A.recorded = 0; A.irf_draws = 0;
    A.grid.resize(Ps); A.log_prior.resize(Ps);
    ord_grid_fill(hi, P, A.grid.data());
    for (int k = 0; k < P; ++k) A.log_prior[(size_t)k] = log_prior ? log_prior[k] : -(A.grid[(size_t)k] * A.grid[(size_t)k]) / 18.0;
    std::vector<int> idx(rows);
    std::vector<double> thr(rows);
    for (int64_t j = 0; j < m; ++j)
        for (int c = 1; c < C; ++c) {
            const size_t r = (size_t)j * (size_t)(C - 1) + (size_t)(c - 1);
            idx[r] = K0 ? K0[r] : (2 * (P - 1) * c + C) / (2 * C);
            thr[r] = A.grid[(size_t)idx[r]];
        }
    if (hipMemcpyAsync(A.cat, cat, (size_t)(n * m), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.d_grid, A.grid.data(), sizeof(double) * Ps, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.d_log_prior, A.log_prior.data(), sizeof(double) * Ps, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.idx, idx.data(), sizeof(int) * rows, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(A.thr, thr.data(), sizeof(double) * rows, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(A.lp, 0, sizeof(double) * rows * GPIRT_ORD_MAX_WIDTH, st) != hipSuccess ||
        hipMemsetAsync(A.cum, 0, sizeof(double) * rows * (size_t)N, st) != hipSuccess ||
        hipMemsetAsync(A.G, 0, sizeof(double) * ((size_t)Np * (size_t)C * (size_t)m + 2), st) != hipSuccess ||
        hipMemsetAsync(A.window, 0, sizeof(int) * rows, st) != hipSuccess ||
        hipMemsetAsync(A.stat, 0, sizeof(long long) * 4, st) != hipSuccess ||
        hipMemsetAsync(A.hist, 0, sizeof(uint32_t) * rows * Ps, st) != hipSuccess ||
        hipMemsetAsync(A.draws, 0, draw_bytes, st) != hipSuccess) return fail(GPIRT_E_HIP, "the upload");
    if (launch_ord_indicators(st, A.cat, n, m, C, A.Y) != 0 || launch_ord_counts(st, A.cat, n, m, C, A.counts) != 0)
        return fail(GPIRT_E_HIP, "the indicator launch");
    // the pinned intercept: beta[0, :] = 0, mu and mu_star refreshed with draw_beta's expression
    std::vector<double> hb((size_t)(2 * m));
    if (hipMemcpyAsync(hb.data(), s->beta, sizeof(double) * (size_t)(2 * m), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return fail(GPIRT_E_HIP, "reading beta");
    for (int64_t j = 0; j < m; ++j) hb[(size_t)(2 * j)] = 0.0;
    if (hipMemcpyAsync(s->beta, hb.data(), sizeof(double) * (size_t)(2 * m), hipMemcpyHostToDevice, st) != hipSuccess ||
        launch_linear_mean(st, s->theta, n, s->beta, m, s->mu) != 0 ||
        launch_linear_mean(st, s->tstar, N, s->beta, m, s->mu_star) != 0 ||
        hipStreamSynchronize(st) != hipSuccess) return fail(GPIRT_E_HIP, "pinning the intercept");      // (the host vectors go out of scope)
    A.on = true;
    return 0;
}

int gpirt_sampler_draw_thresholds(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    OrdState& A = s->ord;
    GP_TRY(needs(A.on, "ordinal responses are", "gpirt_sampler_ordinal_enable"));
    GP_TRY(beta_sync(s));                     // mu of a held-back draw_beta
    s->lp_current = false;
    OrdThrArgs a{};
    a.f = s->f; a.mu = s->mu; a.cat = A.cat; a.counts = A.counts; a.n = s->n; a.m = s->m;
    a.grid = A.d_grid; a.log_prior = A.d_log_prior; a.C = A.C; a.P = A.P; a.W = A.W;
    a.idx = A.idx; a.thr = A.thr; a.lp = A.lp; a.window = A.window; a.stat = A.stat;
    a.seed = s->opt.seed; a.t = A.t + 1; a.item0 = (uint32_t)s->opt.item0;
    hipStream_t st = s->h->stream;
    const bool timed = s->timing;
    if (timed) {
        for (hipEvent_t& t : A.tev) if (!t) GP_HIP(hipEventCreate(&t));
        GP_HIP(hipEventRecord(A.tev[0], st));
    }
    GP_TRY(launch_ord_thresholds(st, a));
    A.t += 1;
    A.lp_W = A.W;
    if (timed) {                              // (timing on: one synchronisation, as the amplitude update's)
        GP_HIP(hipEventRecord(A.tev[1], st));
        GP_HIP(hipEventSynchronize(A.tev[1]));
        float ms = 0.f;
        hipEventElapsedTime(&ms, A.tev[0], A.tev[1]);
        A.last_ms = ms;
    }
    return 0;
}

int gpirt_sampler_ordinal_width(gpirt_sampler_t s, int W)
{
    GP_ARG(s != nullptr);
    GP_TRY(needs(s->ord.on, "ordinal responses are", "gpirt_sampler_ordinal_enable"));
    if (W < 1 || W > GPIRT_ORD_MAX_WIDTH) { set_error("ordinal: window width W = %d, it must lie in 1 .. %d", W, GPIRT_ORD_MAX_WIDTH); return GPIRT_E_ARG; }
    s->ord.W = W;                             // (from the next update on; "lp" keeps the last update's width, lp_W, until then)
    return 0;
}

int gpirt_sampler_ordinal_record(gpirt_sampler_t s)
{
    GP_ARG(s != nullptr);
    OrdState& A = s->ord;
    GP_TRY(needs(A.on, "ordinal responses are", "gpirt_sampler_ordinal_enable"));
    if (A.recorded >= A.planned) { set_error("ordinal: all %lld planned draws are recorded", (long long)A.planned); return GPIRT_E_ARG; }
    GP_TRY(launch_ord_record(s->h->stream, A.idx, s->m, A.C, A.P, A.recorded, A.hist, A.draws));
    A.recorded += 1;
    return 0;
}

int gpirt_sampler_ordinal_accumulate_irf(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    OrdState& A = s->ord;
    GP_TRY(needs(A.on, "ordinal responses are", "gpirt_sampler_ordinal_enable"));
    GP_TRY(launch_ord_irf(s->h->stream, s->fstar, s->N, s->m, A.C, A.thr, A.cum));
    A.irf_draws += 1;
    return 0;
}

int gpirt_sampler_ordinal_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    GP_ARG(s && name && h_out && bytes >= 0);
    OrdState& A = s->ord;
    GP_TRY(needs(A.on, "ordinal responses are", "gpirt_sampler_ordinal_enable"));
    const int64_t n = s->n, m = s->m, N = s->N, rows = m * (A.C - 1), P = A.P;
    const void* host = nullptr; const void* dev = nullptr; int64_t want = 0;
    if (strcmp(name, "cat") == 0) { dev = A.cat; want = n * m; }
    else if (strcmp(name, "grid") == 0) { host = A.grid.data(); want = 8 * P; }
    else if (strcmp(name, "log_prior") == 0) { host = A.log_prior.data(); want = 8 * P; }
    else if (strcmp(name, "index") == 0) { dev = A.idx; want = 4 * rows; }
    else if (strcmp(name, "thresholds") == 0) { dev = A.thr; want = 8 * rows; }
    else if (strcmp(name, "counts") == 0) { dev = A.counts; want = 8 * m * A.C; }
    else if (strcmp(name, "lp") == 0) { dev = A.lp; want = 8 * rows * A.lp_W; }
    else if (strcmp(name, "window") == 0) { dev = A.window; want = 4 * rows; }
    else if (strcmp(name, "hist") == 0) { dev = A.hist; want = 4 * rows * P; }
    else if (strcmp(name, "draws") == 0) { dev = A.draws; want = 4 * A.recorded * rows; }
    else if (strcmp(name, "cum") == 0) { dev = A.cum; want = 8 * rows * N; }
    else if (strcmp(name, "pinned") == 0) { dev = A.stat; want = 8; }
    else if (strcmp(name, "failed") == 0) { dev = A.stat + 1; want = 8; }
    else if (strcmp(name, "updates") == 0) { dev = A.stat + 2; want = 8; }
    else { set_error("unknown ordinal array '%s'", name); return GPIRT_E_ARG; }
    if (bytes != want) { set_error("ordinal: '%s' holds %lld bytes, %lld were asked for", name, (long long)want, (long long)bytes); return GPIRT_E_ARG; }
    if (want == 0) return 0;
    if (host) { memcpy(h_out, host, (size_t)want); return 0; }
    GP_HIP(hipMemcpyAsync(h_out, dev, (size_t)want, hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

int gpirt_sampler_ordinal_stats(gpirt_sampler_t s, gpirt_ordinal* out)
{
    GP_ARG(s && out);
    const OrdState& A = s->ord;
    memset(out, 0, sizeof(*out));
    out->on = A.on ? 1 : 0; out->n = s->n; out->m = s->m; out->calls = A.t; out->hi = (double)NAN;
    if (!A.on) return 0;
    long long st3[3];
    GP_HIP(hipMemcpyAsync(st3, A.stat, sizeof(st3), hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    out->categories = A.C; out->points = A.P; out->width = A.W; out->lp_width = A.lp_W; out->hi = A.hi; out->last_ms = A.last_ms;
    out->pinned = st3[0]; out->failed = st3[1]; out->updates = st3[2];
    out->planned_draws = A.planned; out->recorded = A.recorded; out->irf_draws = A.irf_draws;
    return 0;
}

// ---- ordinal model fit (ordinal_fit.hip) --------------------------------------------------------------------------------------------
int gpirt_sampler_ordinal_fit_enable(gpirt_sampler_t s, int parts)
{
    GP_ARG(s != nullptr);
    const char* me = "gpirt_sampler_ordinal_fit_enable";
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", me); return GPIRT_E_ARG; }
    OrdState& A = s->ord;
    if (parts == 0)
        return stage_enable(s, &A.fit, ofit_free, false, [] { return 0; });
    GP_TRY(needs(A.on, "ordinal responses are", "gpirt_sampler_ordinal_enable"));
    if (parts < 0 || (parts & ~GPIRT_OFIT_ALL)) {
        set_error("%s: parts = %d has bits outside GPIRT_OFIT_WAIC | GPIRT_OFIT_PRED | GPIRT_OFIT_PPC", me, parts);
        return GPIRT_E_ARG;
    }
    return stage_enable(s, &A.fit, ofit_free, true,
                        [&] { return ofit_alloc(s->h->stream, &A.fit, s->n, s->m, A.C, parts, s->opt.item0, A.cat); });
}

int gpirt_sampler_ordinal_fit_accumulate(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    OrdState& A = s->ord;
    GP_TRY(needs(A.on && A.fit.on, "the ordinal fit block is", "gpirt_sampler_ordinal_fit_enable"));
    GP_TRY(beta_sync(s));                     // mu of a held-back draw_beta
    return launch_ofit_accumulate(s->h->stream, &A.fit, s->f, s->mu, A.cat, A.thr, s->opt.seed, (uint32_t)s->iter);
}

int gpirt_sampler_ordinal_fit_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    GP_ARG(s && name && h_out && bytes >= 0);
    OrdState& A = s->ord;
    GP_TRY(needs(A.on && A.fit.on, "the ordinal fit block is", "gpirt_sampler_ordinal_fit_enable"));
    const int rc = ofit_last_get(s->h->stream, &A.fit, name, h_out, bytes);
    if (rc != 1) return rc;
    GP_TRY(ofit_seal(s->h->stream, &A.fit));
    return ofit_block_get(s->h->stream, A.fit.block, name, h_out, bytes);
}

int gpirt_sampler_ordinal_fit_totals(gpirt_sampler_t s, gpirt_ordinal_fit* out)
{
    GP_ARG(s && out);
    OrdState& A = s->ord;
    GP_TRY(needs(A.on && A.fit.on, "the ordinal fit block is", "gpirt_sampler_ordinal_fit_enable"));
    GP_TRY(ofit_seal(s->h->stream, &A.fit));
    return ofit_block_totals(s->h->stream, A.fit.block, out);
}

int gpirt_sampler_ordinal_fit_state(gpirt_sampler_t s, void** d_block, int64_t* bytes)
{
    GP_ARG(s && d_block && bytes);
    OrdState& A = s->ord;
    GP_TRY(needs(A.on && A.fit.on, "the ordinal fit block is", "gpirt_sampler_ordinal_fit_enable"));
    GP_TRY(ofit_seal(s->h->stream, &A.fit));
    *d_block = A.fit.block;
    *bytes = ofit_state_words(&A.fit) * (int64_t)sizeof(uint64_t);
    return 0;
}

int gpirt_ordinal_fit_combine(gpirt_handle_t h, const void* const* d_states, int chains, void* d_out)
{
    return ofit_combine(h, d_states, chains, d_out);
}

int gpirt_ordinal_fit_get(gpirt_handle_t h, const void* d_block, const char* name, void* h_out, int64_t bytes)
{
    GP_ARG(h && d_block && name && h_out && bytes >= 0);
    return ofit_block_get(h->stream, d_block, name, h_out, bytes);
}

int gpirt_ordinal_fit_totals(gpirt_handle_t h, const void* d_block, gpirt_ordinal_fit* out)
{
    GP_ARG(h && d_block && out);
    return ofit_block_totals(h->stream, d_block, out);
}

// ---- scoring new respondents under ordinal responses (ordinal_score.hip) ----------------------------------------------------------
int gpirt_sampler_ordinal_score_enable(gpirt_sampler_t s, const int8_t* cat_new, int64_t n_new, int predict, int top)
{
    GP_ARG(s != nullptr);
    const char* me = "gpirt_sampler_ordinal_score_enable";
    if (!s->initialised) { set_error("%s needs an initialised sampler (gpirt_sampler_init)", me); return GPIRT_E_ARG; }
    OrdState& A = s->ord;
    if (!cat_new || n_new == 0)
        return stage_enable(s, &A.score, oscore_free, false, [] { return 0; });
    GP_TRY(needs(A.on, "ordinal responses are", "gpirt_sampler_ordinal_enable"));
    if (n_new < 1 || n_new > GPIRT_SCORE_MAX_N) {        // refused before the old state goes, as every refusal here
        set_error("ordinal scoring: n_new = %lld is outside 1..%d", (long long)n_new, GPIRT_SCORE_MAX_N);
        return GPIRT_E_ARG;
    }
    if (predict) GP_TRY(check_top("ordinal scoring", top, GPIRT_PREDICT_MAX_TOP));
    for (int64_t g = 0; g < n_new * s->m; ++g)
        if (cat_new[g] < 0 || cat_new[g] > A.C) {
            set_error("ordinal scoring: cat_new[%lld, %lld] = %d, it must lie in 0 .. C = %d (0 = missing)", (long long)(g % n_new),
                      (long long)(g / n_new), (int)cat_new[g], A.C);
            return GPIRT_E_ARG;
        }
    return stage_enable(s, &A.score, oscore_free, true,
                        [&] { return oscore_alloc(s->h->stream, &A.score, cat_new, n_new, s->m, A.C, predict != 0); });
}

#define OSCORE_NEEDS(A) needs((A).on && (A).score.on, "ordinal scoring is", "gpirt_sampler_ordinal_score_enable")

int gpirt_sampler_ordinal_score_accumulate(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    OrdState& A = s->ord;
    GP_TRY(OSCORE_NEEDS(A));
    return launch_oscore_accumulate(s->h, s->h->stream, &A.score, s->fstar, A.thr);
}

int gpirt_sampler_ordinal_score_get(gpirt_sampler_t s, const char* name, void* h_out, int64_t bytes)
{
    GP_ARG(s && name && h_out && bytes >= 0);
    OrdState& A = s->ord;
    GP_TRY(OSCORE_NEEDS(A));
    return oscore_get(s->h->stream, &A.score, name, h_out, bytes);
}

int gpirt_sampler_ordinal_score_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    GP_ARG(s && d_state && bytes);
    OrdState& A = s->ord;
    GP_TRY(OSCORE_NEEDS(A));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    *d_state = A.score.block;
    *bytes = oscore_state_words(&A.score) * (int64_t)sizeof(uint64_t);
    return 0;
}

int gpirt_sampler_ordinal_score_predict_state(gpirt_sampler_t s, void** d_state, int64_t* bytes)
{
    GP_ARG(s && d_state && bytes);
    OrdState& A = s->ord;
    GP_TRY(OSCORE_NEEDS(A));
    GP_TRY(needs(A.score.pred_on, "ordinal prediction is", "gpirt_sampler_ordinal_score_enable with predict = 1"));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    *d_state = A.score.pblock;
    *bytes = oscore_pred_state_words(&A.score) * (int64_t)sizeof(uint64_t);
    return 0;
}

int gpirt_ordinal_score_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, void* h_out, int64_t bytes)
{
    return oscore_combine(h, chains, d_states, signs, h_out, bytes);
}

int gpirt_ordinal_score_predict_combine(gpirt_handle_t h, int chains, const void* const* d_states, void* h_out, int64_t bytes)
{
    return oscore_pred_combine(h, chains, d_states, h_out, bytes);
}

int gpirt_sampler_iteration(gpirt_sampler_t s, int* iter)
{
    GP_ARG(s && iter);
    *iter = s->iter;
    return 0;
}

int gpirt_sampler_set_iteration(gpirt_sampler_t s, int iter)
{
    GP_ARG(s && s->initialised && iter >= 0);
    if (stream_mode(s)) { set_error("the R-stream replay has no iteration-keyed sub-streams"); return GPIRT_E_ARG; }
    GP_TRY(aux_join(s));
    s->iter = iter;
    return 0;
}

int gpirt_sampler_check(gpirt_sampler_t s)
{
    GP_ARG(s != nullptr);
    gpirt_handle_t h = s->h;
    hipStream_t st = h->stream;
    GP_TRY(aux_join(s));                  // the flags of work still running on the sampler's own stream
    GP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
    GP_HIP(hipMemcpyAsync(s->h_flags, s->flags, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    GP_HIP(hipStreamSynchronize(st));
    if (h->h_info[1] != 0) {
        // hang-guard expiry.  Repairable in place while nothing has read the bad L (the usual case: check() right behind a
        // step) and the launch-per-step panel was not what failed; otherwise the chain has already consumed garbage.
        if (!s->factor_fresh || h->cfg.panel == 2) return report_panel_guard(h, h->h_info, st);
        GP_TRY(recover_factor(s));
        GP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
        GP_HIP(hipStreamSynchronize(st));
        if (h->h_info[1] != 0) return report_panel_guard(h, h->h_info, st);
    }
    if (*h->h_info > 0) {
        set_error("chol(): decomposition failed (leading minor of order %d is not positive definite)", *h->h_info);
        return *h->h_info;
    }
    if (s->h_flags[0] != 0) {
        set_error("sampler state is not finite (flag %d): elliptical slice sampler did not terminate or the R stream window overflowed", s->h_flags[0]);
        return s->h_flags[0];
    }
    if (s->h_flags[1] != 0) return report_degenerate_theta(s, s->h_flags[1]);
    return 0;
}

static int lookup(gpirt_sampler_t s, const char* name, void** p, int64_t* count)
{
    const int64_t n = s->n, m = s->m, N = s->N;
    struct E { const char* k; void* p; int64_t c; } tab[] = {
        { "theta", s->theta, n }, { "f", s->f, n * m }, { "beta", s->beta, 2 * m }, { "mu", s->mu, n * m },
        { "mu_star", s->mu_star, N * m }, { "fstar", s->fstar, N * m }, { "L", s->L, n * n },
        { "logpost", s->logpost, N * n }, { "irf_sum", s->irf_sum, N * m }, { "ess_k", s->ess_k, m },
        { "s", s->s, N }, { "mean", s->mean, N * m }, { "nu", s->NU, n * m }, { "z", s->Z, n * m },
        { "y", s->y, n * m }, { "rs_trace", s->rs_trace, s->rs_trace ? 128 : 0 },
        { "rs_stats", s->rs_ctl, s->rs_ctl ? 8 : 0 },     // 64-bit words: [first item not committed, mispredictions found, ...]
        { "fstar_full", s->fstar_full, s->fstar_full ? N * s->blk_m : 0 }, { "theta_stage", s->theta_stage, s->theta_stage ? n : 0 },
        { "gbar", s->shape.gbar, s->shape.on ? N * m : 0 },       // the curve draw_fstar's epilogue stored (shape posteriors on)
    };
    for (auto& e : tab)
        if (strcmp(e.k, name) == 0) { *p = e.p; *count = e.c; return 0; }
    set_error("unknown sampler array '%s'", name);
    return GPIRT_E_ARG;
}

int gpirt_sampler_devptr(gpirt_sampler_t s, const char* name, void** d_ptr, int64_t* count)
{
    GP_ARG(s && name && d_ptr && count);
    GP_TRY(lookup(s, name, d_ptr, count));
    // the caller may write through the pointer: what is derived from these arrays is taken as stale from here on (a caller
    // who writes theta, beta or mu after a later draw_beta asks for the pointer again, or uses gpirt_sampler_set)
    if (strcmp(name, "theta") == 0 || strcmp(name, "beta") == 0 || strcmp(name, "mu") == 0) s->mu_linear = false;
    if (strcmp(name, "y") == 0) s->ess_ypk_valid = false;
    if (strcmp(name, "L") == 0) {
        *count = s->ldl * s->n;           // the whole buffer (leading dimension gpirt_sampler_ldl)
        // the caller may read or overwrite any of it: the dense factor now, and a structured factor that follows is not seen
        // through this pointer until gpirt_sampler_dense_factor (or another call that needs all of L) has run
        GP_TRY(ensure_dense_factor(s));
    }
    return 0;
}

int gpirt_sampler_ldl(gpirt_sampler_t s, int64_t* ldl)
{
    GP_ARG(s && ldl);
    *ldl = s->ldl;
    return 0;
}

// ---- the factorisation in pieces on this sampler's L (distributed hosts; include/gpirt_hip.h) ---------------------
int gpirt_sampler_panel_factor(gpirt_sampler_t s, int64_t p)
{
    GP_ARG(s && s->initialised);
    GP_TRY(ensure_dense_factor(s));       // (the pieces work on, and hand out, the dense factor)
    return potrf_panel_factor(s->h, s->h->stream, s->L, s->n, s->ldl, p, s->ext);
}

int gpirt_sampler_panel_update(gpirt_sampler_t s, int64_t p, int64_t c)
{
    GP_ARG(s && s->initialised);
    GP_TRY(ensure_dense_factor(s));       // (the pieces work on, and hand out, the dense factor)
    return potrf_panel_update(s->h, s->h->stream, s->L, s->n, s->ldl, p, c, s->ext);
}

int gpirt_sampler_panel_copy(gpirt_sampler_t s, int64_t p, double* d_buf, int to_buf)
{
    GP_ARG(s && s->initialised && d_buf);
    GP_TRY(ensure_dense_factor(s));       // (the pieces work on, and hand out, the dense factor)
    return potrf_panel_copy(s->h->stream, s->L, s->n, s->ldl, p, d_buf, to_buf != 0, s->ext);
}

int gpirt_sampler_panel_rows(gpirt_sampler_t s, int64_t* rows)
{
    GP_ARG(s && rows);
    *rows = s->n + s->ext;
    return 0;
}

// draw_f's structured product (nu_lr.hip): how many draws have run it so far, and the 64 node rows below the factor as they
// stand (64 x n, column-major; GPIRT_E_ARG when the layout carries none)
int gpirt_sampler_ess_pack_draws(gpirt_sampler_t s, int64_t* draws)
{
    GP_ARG(s && draws);
    *draws = s->ess_pack_draws;
    return 0;
}

int gpirt_sampler_nu_lr_draws(gpirt_sampler_t s, int64_t* draws)
{
    GP_ARG(s && draws);
    *draws = s->nu_lr_draws;
    return 0;
}

// draw_fstar calls of this sampler that took C = S^-1 U from theta alone (fstar_free.hip) so far
int gpirt_sampler_fstar_free_draws(gpirt_sampler_t s, int64_t* draws)
{
    GP_ARG(s && draws);
    *draws = s->fstar_free_draws;
    return 0;
}

// the structured factor (factor_lr.hip): how many factorisations of this sampler built the diagonal parts and node rows alone,
// how many dense factorisations it enqueued (those of ensure_dense_factor included), the dense factor on demand, and the
// diagonal parts as they stand (no dense factor is formed for them)
int gpirt_sampler_factor_lr_count(gpirt_sampler_t s, int64_t* count)
{
    GP_ARG(s && count);
    *count = s->factor_lr_count;
    return 0;
}

int gpirt_sampler_dense_factor_count(gpirt_sampler_t s, int64_t* count)
{
    GP_ARG(s && count);
    *count = s->dense_factor_count;
    return 0;
}

int gpirt_sampler_dense_factor(gpirt_sampler_t s)
{
    GP_ARG(s && s->initialised);
    return ensure_dense_factor(s);
}

int gpirt_sampler_factor_lr_parts(gpirt_sampler_t s, double* h_out, int64_t count)
{
    GP_ARG(s && h_out && count == (int64_t)NU_LR_PART * s->n);
    GP_TRY(aux_join(s));
    GP_TRY(ensure_factor_width(s, NU_LR_PART));       // (behind a factor in narrower parts: the structured factor at 512 first)
    memset(h_out, 0, sizeof(double) * (size_t)count);
    for (int64_t p = 0; p < s->n; p += NU_LR_PART) {
        const int64_t w = s->n - p < NU_LR_PART ? s->n - p : NU_LR_PART;
        GP_HIP(hipMemcpy2DAsync(h_out + p * NU_LR_PART, (size_t)NU_LR_PART * 8, s->L + p * (s->ldl + 1), (size_t)s->ldl * 8, (size_t)w * 8, (size_t)w,
                                hipMemcpyDeviceToHost, s->h->stream));
    }
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

// the width of the diagonal parts a structured L holds (0: L is dense), and those parts as they lie: part p, w x w with w the
// width (the last may be shorter), at h_out + p * w * w with leading dimension w; count = width * n.  Nothing is factored for it.
int gpirt_sampler_factor_lr_width(gpirt_sampler_t s, int* width)
{
    GP_ARG(s && width);
    *width = factor_width(s);
    return 0;
}

int gpirt_sampler_factor_lr_blocks(gpirt_sampler_t s, double* h_out, int64_t count)
{
    GP_ARG(s && h_out);
    const int64_t W = factor_width(s);
    if (W == 0) { set_error("factor_lr_blocks: L holds the dense factor, not diagonal parts"); return GPIRT_E_ARG; }
    GP_ARG(count == W * s->n);
    GP_TRY(aux_join(s));
    memset(h_out, 0, sizeof(double) * (size_t)count);
    for (int64_t p = 0; p < s->n; p += W) {
        const int64_t w = s->n - p < W ? s->n - p : W;
        GP_HIP(hipMemcpy2DAsync(h_out + p * W, (size_t)W * 8, s->L + p * (s->ldl + 1), (size_t)s->ldl * 8, (size_t)w * 8, (size_t)w,
                                hipMemcpyDeviceToHost, s->h->stream));
    }
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

int gpirt_sampler_nu_lr_rows(gpirt_sampler_t s, double* h_out, int64_t count)
{
    GP_ARG(s && h_out && s->node_off >= 0 && count == (int64_t)NU_LR_RANK * s->n);
    GP_TRY(aux_join(s));
    GP_HIP(hipMemcpy2DAsync(h_out, (size_t)NU_LR_RANK * 8, s->L + s->n + s->node_off, (size_t)s->ldl * 8, (size_t)NU_LR_RANK * 8, (size_t)s->n,
                            hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

// ... and by halves of an outer panel (first sub-panel / the rest), for a host that pipelines the broadcasts
int gpirt_sampler_panel_factor_part(gpirt_sampler_t s, int64_t p, int half)
{
    GP_ARG(s && s->initialised);
    GP_TRY(ensure_dense_factor(s));       // (the pieces work on, and hand out, the dense factor)
    return potrf_panel_factor(s->h, s->h->stream, s->L, s->n, s->ldl, p, s->ext, half);
}

int gpirt_sampler_panel_update_part(gpirt_sampler_t s, int64_t p, int64_t c, int part)
{
    GP_ARG(s && s->initialised);
    GP_TRY(ensure_dense_factor(s));       // (the pieces work on, and hand out, the dense factor)
    return potrf_panel_update(s->h, s->h->stream, s->L, s->n, s->ldl, p, c, s->ext, part);
}

int gpirt_sampler_panel_copy_part(gpirt_sampler_t s, int64_t p, int half, double* d_buf, int64_t buf_doubles, int to_buf)
{
    GP_ARG(s && s->initialised && d_buf && buf_doubles >= 0);
    GP_TRY(ensure_dense_factor(s));       // (the pieces work on, and hand out, the dense factor)
    return potrf_panel_copy(s->h->stream, s->L, s->n, s->ldl, p, d_buf, to_buf != 0, s->ext, half, buf_doubles);
}

// dst's chain state := src's (theta, f, beta, mu, mu_star, fstar, the n x n factor, the iteration counter): lets a second
// sampler with other options replay a stage on the same state (bench.py's in-run check of the draw_fstar forms)
int gpirt_sampler_copy_state(gpirt_sampler_t dst, gpirt_sampler_t src)
{
    GP_ARG(dst && src && dst->initialised && src->initialised && dst->n == src->n && dst->m == src->m && dst->h == src->h);
    if (dst->ord.on || src->ord.on) {
        set_error("gpirt_sampler_copy_state is refused while ordinal responses are on: the categories, thresholds and records are not copied");
        return GPIRT_E_ARG;
    }
    if (dst->ell.on || src->ell.on) {
        set_error("gpirt_sampler_copy_state is not defined while the length-scale update is on (the index and its tables are not copied)");
        return GPIRT_E_ARG;
    }
    if (dst->amp.mode || src->amp.mode) {
        set_error("gpirt_sampler_copy_state is not defined while per-item amplitudes are on (they are not copied)");
        return GPIRT_E_ARG;
    }
    if (dst->pop.mode || src->pop.mode) {
        set_error("gpirt_sampler_copy_state is not defined while a population prior is on (it is not copied)");
        return GPIRT_E_ARG;
    }
    if (dst->kern.family != src->kern.family || dst->kern.length_scale != src->kern.length_scale) {
        // (only a length-scale update can part two samplers of one handle: the copied factor would not be dst's kernel's)
        set_error("gpirt_sampler_copy_state: the samplers' kernels differ (length_scale %g and %g)", dst->kern.length_scale, src->kern.length_scale);
        return GPIRT_E_ARG;
    }
    hipStream_t st = dst->h->stream;
    const int64_t n = dst->n, m = dst->m, N = dst->N;
    GP_TRY(aux_join(dst)); GP_TRY(aux_join(src));
    GP_TRY(ensure_dense_factor(src));     // (dst gets the whole factor)
    dst->L_structured = false;
    dst->lp_current = false;
    dst->mu_linear = false;
    src->factor_fresh = false;
    invalidate_factor_products(dst);
    GP_HIP(hipMemcpyAsync(dst->theta, src->theta, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
    GP_HIP(hipMemcpyAsync(dst->f, src->f, sizeof(double) * (size_t)(n * m), hipMemcpyDeviceToDevice, st));
    GP_HIP(hipMemcpyAsync(dst->beta, src->beta, sizeof(double) * (size_t)(2 * m), hipMemcpyDeviceToDevice, st));
    GP_HIP(hipMemcpyAsync(dst->mu, src->mu, sizeof(double) * (size_t)(n * m), hipMemcpyDeviceToDevice, st));
    GP_HIP(hipMemcpyAsync(dst->mu_star, src->mu_star, sizeof(double) * (size_t)(N * m), hipMemcpyDeviceToDevice, st));
    GP_HIP(hipMemcpyAsync(dst->fstar, src->fstar, sizeof(double) * (size_t)(N * m), hipMemcpyDeviceToDevice, st));
    GP_HIP(hipMemcpy2DAsync(dst->L, (size_t)dst->ldl * 8, src->L, (size_t)src->ldl * 8, (size_t)n * 8, (size_t)n,
                            hipMemcpyDeviceToDevice, st));
    dst->rows_valid = false;
    dst->theta_ok = src->theta_ok; dst->theta_alone = src->theta_alone;
    GP_TRY(rebuild_rows(dst));            // the rows below L for the copied (theta, L)
    dst->iter = src->iter;
    return 0;
}

int gpirt_sampler_get(gpirt_sampler_t s, const char* name, double* h_out, int64_t count)
{
    GP_ARG(s && name && h_out);
    void* p; int64_t c;
    GP_TRY(lookup(s, name, &p, &c));
    GP_ARG(count <= c);
    const size_t esz = strcmp(name, "ess_k") == 0 ? sizeof(int) : sizeof(double);
    GP_TRY(aux_join(s));
    if (strcmp(name, "L") == 0) GP_TRY(ensure_dense_factor(s));
    if (strcmp(name, "L") == 0 && s->ldl != s->n) {       // n x n out of the (n + ext) x n buffer
        GP_ARG(count == s->n * s->n);
        GP_HIP(hipMemcpy2DAsync(h_out, (size_t)s->n * 8, p, (size_t)s->ldl * 8, (size_t)s->n * 8, (size_t)s->n,
                                hipMemcpyDeviceToHost, s->h->stream));
    } else {
        GP_HIP(hipMemcpyAsync(h_out, p, esz * (size_t)count, hipMemcpyDeviceToHost, s->h->stream));
    }
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

int gpirt_sampler_set(gpirt_sampler_t s, const char* name, const double* h_in, int64_t count)
{
    GP_ARG(s && name && h_in);
    void* p; int64_t c;
    GP_TRY(lookup(s, name, &p, &c));
    GP_ARG(count <= c && strcmp(name, "ess_k") != 0);
    if (s->ord.on && strcmp(name, "y") == 0)
        GP_TRY(ord_refuse(s, "gpirt_sampler_set(\"y\")", "the categories were checked against y's missing cells at enable"));
    if (s->ord.on && strcmp(name, "beta") == 0)
        for (int64_t q = 0; q < count; q += 2)
            if (h_in[q] != 0.0) GP_TRY(ord_refuse(s, "gpirt_sampler_set(\"beta\") with a non-zero intercept", "the intercept is pinned at 0"));
    GP_TRY(aux_join(s));
    invalidate_factor_products(s);
    s->lp_current = false;
    if (strcmp(name, "theta") == 0 || strcmp(name, "beta") == 0 || strcmp(name, "mu") == 0) s->mu_linear = false;
    if (strcmp(name, "y") == 0) s->ess_ypk_valid = false;       // (packed again by the next draw_f that reads it)
    if (strcmp(name, "L") == 0 || strcmp(name, "theta") == 0) s->rows_valid = false;
    if (strcmp(name, "L") == 0) s->theta_alone = false;          // (taken as the factor of K(theta, theta) for the theta in place)
    if (strcmp(name, "L") == 0) {
        // (a partial write lands in the dense factor; a whole one replaces whatever L held)
        if (count < c) GP_TRY(ensure_dense_factor(s));
        s->L_structured = false;
    }
    if (strcmp(name, "theta") == 0) {
        s->theta_alone = true;
        s->theta_ok = count == s->n;
        for (int64_t i = 0; i < count; ++i) s->theta_ok = s->theta_ok && h_in[i] >= -5.0 && h_in[i] <= 5.0;
    }
    if (strcmp(name, "L") == 0 && s->ldl != s->n) {
        GP_ARG(count == s->n * s->n);
        GP_HIP(hipMemcpy2DAsync(p, (size_t)s->ldl * 8, h_in, (size_t)s->n * 8, (size_t)s->n * 8, (size_t)s->n,
                                hipMemcpyHostToDevice, s->h->stream));
    } else {
        GP_HIP(hipMemcpyAsync(p, h_in, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, s->h->stream));
    }
    GP_HIP(hipStreamSynchronize(s->h->stream));
    return 0;
}

// IRFs *= 1/S ; plogis : src/gpirtMCMC.cpp:106-111 (Q7: S = 0 gives NaN, as in the reference)
int gpirt_sampler_finish_irfs(gpirt_sampler_t s, int sample_iterations, double* h_irfs)
{
    GP_ARG(s && h_irfs);
    const int64_t cnt = s->N * s->m;
    GP_HIP(hipMemcpyAsync(h_irfs, s->irf_sum, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, s->h->stream));
    GP_HIP(hipStreamSynchronize(s->h->stream));
    const double inv = 1.0 / (double)sample_iterations;
    for (int64_t i = 0; i < cnt; ++i) h_irfs[i] = 1.0 / (1.0 + exp(-(h_irfs[i] * inv)));
    return 0;
}

int gpirt_sampler_enable_timing(gpirt_sampler_t s, int on)
{
    GP_ARG(s != nullptr);
    s->timing = on != 0;
    return 0;
}

int gpirt_sampler_stage_times(gpirt_sampler_t s, double* ms_out, int max_stages, int* n_stages,
                              const char** names_out)
{
    GP_ARG(s && ms_out && n_stages);
    static const char names[] = "draw_f\0draw_fstar\0theta_gemm\0theta_sample\0draw_beta\0factor\0";
    const int k = max_stages < ST_COUNT ? max_stages : ST_COUNT;
    for (int i = 0; i < k; ++i) ms_out[i] = s->stage_ms[i];
    *n_stages = k;
    if (names_out) *names_out = names;
    (void)kStageNames;
    return 0;
}

// Whole-call drop-in: src/gpirtMCMC.cpp:5-117 behind src/RcppExports.cpp:16-30.
long long gpirt_debug_take_mcmc_trip(void);
static int g_last_mcmc_fallbacks = 0;
int gpirt_debug_last_mcmc_fallbacks(void) { return g_last_mcmc_fallbacks; }

// What one chain of chains_run leaves behind for the combines: its states, moved out of the sampler before that goes.  The
// pair, bin and group states travel inside ppc, the prediction inside score, the order posteriors' pair block inside shape.
struct ChainKeep {
    SummaryState sum;                 // sealed: header and IRF sum
    PpcState ppc;
    RankState rank;
    ScoreState score;
    ShapeState shape;
    SumscoreState sumscore;
    EquateState equate;
    LooState loo;
};

// One chain of chains_run: run on the caller's handle, with the GPIRT_SUM_DIAG accumulators planned for the chain's S draws
// and the analyses that `run` names (never NULL; its in/out structs as they were on entry), each accumulated beside the
// summaries and handed to *keep.  The tick sees (base + it, ticks); PSIS-LOO plans its tail for all chains' `draws`.
struct ChainRun {
    gpirt_handle_t h;
    int base, ticks;
    int64_t draws;
    const gpirt_run* run;
    ChainKeep* keep;
};

// The loop of gpirt_mcmc, gpirt_mcmc_summary and each chain of gpirt_mcmc_chains (arguments checked by the callers).
// sm != NULL: the draws' pointers may be NULL (not stored) and every sampling iteration's state is added to the summaries --
// under the item RNG from its checkpoint once that is verified (start_store), so that a rollback cannot count an iteration
// twice.
static int mcmc_run(const double* h_y, int64_t n, int64_t m, const double* h_theta0, int S_it, int B_it,
                    const double* h_pm, const double* h_ps, const double* h_step, const gpirt_options* opts,
                    gpirt_rstream_t rs, gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws,
                    double* h_beta_draws, double* h_f_draws, double* h_irfs, gpirt_summary* sm, const ChainRun* cr = nullptr)
{
    gpirt_options o;
    if (opts) o = *opts; else gpirt_default_options(&o);
    gpirt_handle_t h = nullptr;
    if (cr) h = cr->h;
    else {
        GP_TRY(gpirt_create_own_stream(&h, o.device));
        const long long trip = gpirt_debug_take_mcmc_trip();
        if (trip > 0) h->trip_guard_at = trip;
    }
    auto drop_handle = [&]() { if (!cr) gpirt_destroy(h); };
    auto ticked = [&](int it, int total) -> bool {
        return tick && (cr ? tick(tick_ctx, cr->base + it, cr->ticks) : tick(tick_ctx, it, total));
    };
    gpirt_sampler_t s = nullptr;
    int rc = gpirt_sampler_create(&s, h, h_y, n, m, h_theta0, h_pm, h_ps, h_step, &o, rs);
    if (rc) { drop_handle(); return rc; }
    const int64_t N = s->N;
    const int total = S_it + B_it;
    const bool replay = stream_mode(s);
    const bool summarise = sm && sm->parts;
    // a chain of chains_run also accumulates what its run names (chains_run has checked it: predict only with score; pairs,
    // bins and dif only with ppc; order only with shape)
    const gpirt_run none{};
    const gpirt_run& run = cr ? *cr->run : none;
    std::vector<double> th((size_t)n);
    auto store_sync = [&](int slot) -> int {
        // theta_draws.row(slot), beta_draws.slice(slot), f_draws.slice(slot): :53-55, :99-101
        if (h_theta_draws) {
            GP_TRY(gpirt_sampler_get(s, "theta", th.data(), n));
            for (int64_t i = 0; i < n; ++i) h_theta_draws[slot + i * (int64_t)(S_it + 1)] = th[(size_t)i];
        }
        if (h_beta_draws) GP_TRY(gpirt_sampler_get(s, "beta", h_beta_draws + (int64_t)slot * 2 * m, 2 * m));
        if (h_f_draws) GP_TRY(gpirt_sampler_get(s, "f", h_f_draws + (int64_t)slot * n * m, n * m));
        return 0;
    };
    // the summaries out of the sampler (before it is destroyed)
    auto summary_out = [&]() -> int {
        if (cr) {                               // the chain's states outlive its sampler until the combines
            ChainKeep& k = *cr->keep;
            auto hand_over = [&](auto& kept, auto& live) -> int {      // once the stream has finished the last accumulate
                GP_HIP(hipStreamSynchronize(h->stream));
                kept = std::move(live);
                live = {};
                return 0;
            };
            GP_TRY(summary_seal(h->stream, &s->sum, s->irf_sum, N));
            k.sum = std::move(s->sum);
            s->sum = SummaryState{};
            if (s->ppc.on) {
                GP_TRY(ppc_seal(h->stream, &s->ppc));
                k.ppc = std::move(s->ppc);
                s->ppc = PpcState{};
            }
            if (s->rank.on) GP_TRY(hand_over(k.rank, s->rank));
            if (s->score.on) GP_TRY(hand_over(k.score, s->score));
            if (s->shape.on) GP_TRY(hand_over(k.shape, s->shape));
            if (s->sumscore.on) GP_TRY(hand_over(k.sumscore, s->sumscore));
            if (s->equate.on) GP_TRY(hand_over(k.equate, s->equate));
            if (s->loo.on) {
                GP_HIP(hipStreamSynchronize(h->stream));
                k.loo = s->loo;
                s->loo = LooState{};
            }
            return 0;
        }
        if (!sm) return 0;
        for (int k = 0; k < GPIRT_SUM_NTOTALS; ++k) sm->totals[k] = (double)NAN;
        sm->totals[GPIRT_SUM_T_DRAWS] = (double)s->sum.draws;
        if (!summarise) return 0;
        const struct { const char* name; double* p; int64_t c; } outs[] = {
            { "p_yes", sm->h_p_yes, n * m }, { "lppd", sm->h_lppd, n * m }, { "p_waic", sm->h_p_waic, n * m },
            { "f_mean", sm->h_f_mean, n * m }, { "f_var", sm->h_f_var, n * m }, { "theta_mean", sm->h_theta_mean, n },
            { "theta_var", sm->h_theta_var, n }, { "beta_mean", sm->h_beta_mean, 2 * m }, { "beta_var", sm->h_beta_var, 2 * m },
        };
        for (const auto& e : outs)
            if (e.p) GP_TRY(gpirt_sampler_summary_get(s, e.name, e.p, e.c));
        if (sm->parts & GPIRT_SUM_WAIC) GP_TRY(gpirt_sampler_summary_totals(s, sm->totals));
        return 0;
    };
    rc = gpirt_sampler_init(s);
    if (!rc) rc = gpirt_sampler_check(s);
    if (!rc) rc = store_sync(0);
    if (!rc && summarise)
        rc = cr ? gpirt_sampler_summary_enable_planned(s, sm->parts | GPIRT_SUM_DIAG, S_it) : gpirt_sampler_summary_enable(s, sm->parts);
    if (!rc && run.ppc) rc = gpirt_sampler_ppc_enable(s, 1);
    if (!rc && run.pairs) rc = gpirt_sampler_ppc_pairs_enable(s, 1);
    if (!rc && run.bins) rc = gpirt_sampler_ppc_bins_enable(s, run.bins->h, run.bins->cuts, 1);
    if (!rc && run.dif) rc = gpirt_sampler_ppc_dif_enable(s, run.dif->G, run.dif->groups, run.dif->h, run.dif->cuts, 1);
    if (!rc && run.ranks) rc = gpirt_sampler_rank_enable(s, run.ranks->pivots, run.ranks->n_pivots, run.ranks->pairwise);
    if (!rc && run.score) rc = gpirt_sampler_score_enable(s, run.h_y_new, run.n_new);
    if (!rc && run.predict) rc = gpirt_sampler_score_predict_enable(s, 1);
    // (gbar holds a curve from the first step's draw_fstar on; no draw is accumulated before that)
    if (!rc && run.shape) rc = gpirt_sampler_shape_enable(s, run.shape->k_half, run.shape->tols, run.shape->n_tols, 1);
    if (!rc && run.sumscore) rc = gpirt_sampler_sumscore_enable(s, run.sumscore->items, 1);
    if (!rc && run.equate) rc = gpirt_sampler_equate_enable(s, run.equate->x, run.equate->y, 1);
    if (!rc && run.order) rc = gpirt_sampler_shape_order_enable(s, 1);
    if (!rc && run.loo) rc = gpirt_sampler_loo_enable(s, cr->draws, (int)run.loo->tail, 1);

    if (replay) {
        // R-stream replay is item-sequential and drains the stream every iteration anyway (the cursor comes back to the
        // host): check, repair a hang-guard expiry in place (gpirt_sampler_check: nothing has read the new L yet) and store,
        // synchronously.
        for (int it = 0; it < total && !rc; ++it) {
            if (ticked(it, total)) { set_error("interrupted"); rc = GPIRT_E_INTERRUPT; break; }
            rc = gpirt_sampler_step(s);
            if (!rc) rc = gpirt_sampler_check(s);
            if (!rc && it >= B_it) {
                rc = gpirt_sampler_accumulate_irf(s);                          // :103
                if (!rc) rc = store_sync(it - B_it + 1);
                // the blocks read the live state and consume nothing of R's stream (the PPC's replicate is counter-based);
                // beta_sync once for all of them, also where only blocks that read neither beta nor mu are on: under R's
                // stream draw_beta is never deferred, so the call finds nothing to do
                if (!rc) rc = beta_sync(s);
                if (!rc) rc = accumulate_run(s, live_view(s));
            }
        }
        if (!rc) rc = gpirt_sampler_finish_irfs(s, S_it, h_irfs);
        if (!rc) rc = summary_out();
        g_last_mcmc_fallbacks = h->guard_fallbacks;
        gpirt_sampler_destroy(s);
        drop_handle();
        return rc;
    }

    // Item RNG: the host runs ahead of the device, errors are sticky words polled without draining the stream, and the
    // stored draws (src/gpirtMCMC.cpp:99-101; 64 MiB per stored iteration at the metric size) travel on a second stream
    // while the next iterations run.  Both hang off ONE mechanism: after every iteration the chain state is copied
    // device-to-device into one of three checkpoint slots (theta, beta, f, mu, mu*, f*, the IRF sums: ~1 % of an iteration),
    // followed by a read-back of the error words.  A checkpoint is VERIFIED once its error words have come back clean;
    // the host never enqueues iteration it before checkpoint it - 1 is verified (so it is at most two iterations ahead,
    // and a verified slot is never the one being overwritten).  Stored draws are copied out of verified checkpoints.
    // If the words come back with the panel kernel's hang guard raised (flagsync.h: its work-groups were not co-resident
    // within the spin bound -- a foreign tenant on the GPU can do that), the iterations enqueued since the last verified
    // checkpoint have consumed an unfinished factor: the state is rolled back to that checkpoint, its factor is rebuilt
    // from theta with the launch-per-step panel, the lost iterations are repeated on that panel too, and the chain goes
    // on -- the same draws as an undisturbed run (counter-based RNG keyed by the iteration; L equal to rounding).  Only a
    // second expiry without progress ends the call.
    constexpr int NS = 3;
    // every part of a slot starts on a 16-byte boundary (the summaries' kernel reads f and mu of a slot two doubles a lane)
    auto even = [](size_t c) { return (c + 1) & ~(size_t)1; };
    const size_t off_beta = even((size_t)n), off_f = off_beta + even((size_t)(2 * m)), off_mu = off_f + even((size_t)(n * m));
    const size_t off_gbar = off_mu + even((size_t)(n * m)) + 3 * even((size_t)(N * m));   // with the shapes on: gbar, last
    const size_t ck_doubles = off_gbar + (s->shape.on ? even((size_t)(N * m)) : 0);
    const size_t off_fstar = off_mu + even((size_t)(n * m)) + even((size_t)(N * m));      // the slot's f*, after mu*
    double* ck[NS] = { nullptr, nullptr, nullptr };
    hipEvent_t ev_flags[NS] = {}, ev_copied[NS] = {};
    bool copy_pending[NS] = { false, false, false };
    int copy_slot[NS] = { 0, 0, 0 };
    std::vector<double> th_stage[NS];
    hipStream_t copy_stream = nullptr;
    int* h_poll = nullptr;                                 // pinned, per slot: [potrf info + guard record (8) | flag0, flag1]
    auto fail_hip = [&](const char* what) { set_error("%s failed in gpirt_mcmc", what); return (int)GPIRT_E_HIP; };
    if (!rc) {
        bool ok = hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking) == hipSuccess &&
                  hipHostMalloc(&h_poll, NS * 16 * sizeof(int), hipHostMallocDefault) == hipSuccess;
        for (int q = 0; q < NS && ok; ++q) {
            ok = hipMalloc(&ck[q], ck_doubles * sizeof(double)) == hipSuccess &&
                 hipEventCreateWithFlags(&ev_flags[q], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&ev_copied[q], hipEventDisableTiming) == hipSuccess;
            th_stage[q].resize((size_t)n);
        }
        if (!ok) rc = fail_hip("allocation");
    }
    struct Part { double* p; size_t cnt; };
    auto parts = [&]() {
        std::vector<Part> v{ { s->theta, (size_t)n }, { s->beta, (size_t)(2 * m) }, { s->f, (size_t)(n * m) },
                             { s->mu, (size_t)(n * m) }, { s->mu_star, (size_t)(N * m) }, { s->fstar, (size_t)(N * m) },
                             { s->irf_sum, (size_t)(N * m) } };
        if (s->shape.on) v.push_back(Part{ s->shape.gbar, (size_t)(N * m) });
        return v;
    };
    auto save_ckpt = [&](int k) -> int {                    // state after k iterations -> slot k % NS, on the compute stream
        const int q = k % NS;
        hipStream_t st = h->stream;
        if (beta_sync(s) != 0) return fail_hip("draw_beta join");
        if (copy_pending[q] && hipStreamWaitEvent(st, ev_copied[q], 0) != hipSuccess) return fail_hip("hipStreamWaitEvent");
        double* d = ck[q];
        for (const Part& pt : parts()) {
            if (hipMemcpyAsync(d, pt.p, pt.cnt * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail_hip("checkpoint");
            d += even(pt.cnt);
        }
        if (hipMemcpyAsync(h_poll + 16 * q, h->d_info, 8 * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(h_poll + 16 * q + 8, s->flags, 2 * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipEventRecord(ev_flags[q], st) != hipSuccess)
            return fail_hip("flag read-back");
        return 0;
    };
    auto finish_store = [&](int q) -> int {                 // theta travels through a staging row: scatter it once it is here
        if (!copy_pending[q]) return 0;
        if (hipEventSynchronize(ev_copied[q]) != hipSuccess) return fail_hip("draw copy");
        const int slot = copy_slot[q];
        if (h_theta_draws)
            for (int64_t i = 0; i < n; ++i) h_theta_draws[slot + i * (int64_t)(S_it + 1)] = th_stage[q][(size_t)i];
        copy_pending[q] = false;
        return 0;
    };
    auto start_store = [&](int k) -> int {                  // verified checkpoint k -> draw slot k - B_it, on the copy stream
        const int q = k % NS, slot = k - B_it;
        GP_TRY(finish_store(q));
        const double* d = ck[q];
        // the blocks read the slot (the state after k iterations; theta first) on the compute stream: ordered before
        // save_ckpt(k + 3) overwrites it, which the host enqueues only once checkpoint k + 1 is verified
        GP_TRY(accumulate_run(s, DrawView{ d, d + off_beta, d + off_f, d + off_mu, d + off_fstar, d + off_gbar, (uint32_t)k }));
        if (!h_theta_draws && !h_beta_draws && !h_f_draws) return 0;
        if ((h_theta_draws && hipMemcpyAsync(th_stage[q].data(), d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, copy_stream) != hipSuccess) ||
            (h_beta_draws && hipMemcpyAsync(h_beta_draws + (int64_t)slot * 2 * m, d + off_beta, sizeof(double) * (size_t)(2 * m), hipMemcpyDeviceToHost, copy_stream) != hipSuccess) ||
            (h_f_draws && hipMemcpyAsync(h_f_draws + (int64_t)slot * n * m, d + off_f, sizeof(double) * (size_t)(n * m), hipMemcpyDeviceToHost, copy_stream) != hipSuccess) ||
            hipEventRecord(ev_copied[q], copy_stream) != hipSuccess)
            return fail_hip("draw copy");
        copy_pending[q] = true; copy_slot[q] = slot;
        return 0;
    };
    auto rollback = [&](int k) -> int {                     // chain state := verified checkpoint k, factor rebuilt on the fallback panel
        hipStream_t st = h->stream;
        if (hipStreamSynchronize(st) != hipSuccess) return fail_hip("hipStreamSynchronize");
        if (h->side) hipStreamSynchronize(h->side);
        if (s->haux) hipStreamSynchronize(s->haux->stream);
        s->beta_deferred = false; s->beta_pending = false; s->prep_pending = false; s->z_filled_iter = 0;
        const double* d = ck[k % NS];
        for (const Part& pt : parts()) {
            if (hipMemcpyAsync(pt.p, d, pt.cnt * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail_hip("rollback");
            d += even(pt.cnt);
        }
        if (hipMemsetAsync(s->flags, 0, 4 * sizeof(int), st) != hipSuccess) return fail_hip("rollback");
        s->mu_linear = false;
        s->iter = k;
        return recover_factor(s);
    };
    s->sticky_info = true;            // potrf no longer clears its info word: first failure sticks
    const int panel_mode = h->cfg.panel;
    int it = 0, verified = 0, fallback_until = 0, last_fallback = -1;
    if (!rc) rc = save_ckpt(0);
    if (!rc && hipEventSynchronize(ev_flags[0]) != hipSuccess) rc = fail_hip("hipEventSynchronize");
    while (!rc && verified < total) {
        if (it < total && verified >= it - 1) {
            if (ticked(it, total)) { set_error("interrupted"); rc = GPIRT_E_INTERRUPT; break; }
            h->cfg.panel = (it < fallback_until) ? 2 : panel_mode;          // iterations lost to a guard expiry are repeated on the fallback panel
            if (h->aux) h->aux->cfg.panel = h->cfg.panel;
            rc = gpirt_sampler_step(s);
            h->cfg.panel = panel_mode;
            if (h->aux) h->aux->cfg.panel = panel_mode;
            if (!rc && it >= B_it) rc = gpirt_sampler_accumulate_irf(s);   // :103
            if (!rc) rc = save_ckpt(it + 1);
            ++it;
            continue;
        }
        const int k = verified + 1, q = k % NS;
        if (hipEventSynchronize(ev_flags[q]) != hipSuccess) { rc = fail_hip("hipEventSynchronize"); break; }
        const int* w = h_poll + 16 * q;
        if (w[1] != 0) {
            if (panel_mode == 2 || last_fallback == verified) { rc = report_panel_guard(h, w, h->stream); break; }
            rc = rollback(verified);
            last_fallback = verified; fallback_until = it; it = verified;
            continue;
        }
        if (w[0] > 0) {
            set_error("chol(): decomposition failed (leading minor of order %d is not positive definite)", w[0]);
            rc = w[0];
        } else if (w[8] != 0) {
            set_error("sampler state is not finite (flag %d)", w[8]); rc = w[8];
        } else if (w[9] != 0) {
            rc = report_degenerate_theta(s, w[9]);
        } else {
            verified = k;
            if (k > B_it) rc = start_store(k);
        }
    }
    for (int q = 0; q < NS; ++q) { const int r2 = finish_store(q); if (!rc) rc = r2; }
    if (rc != GPIRT_E_INTERRUPT) {
        const int rc2 = gpirt_sampler_check(s);                            // final, synchronising
        if (!rc) rc = rc2;
    }
    if (copy_stream) { hipStreamSynchronize(copy_stream); hipStreamDestroy(copy_stream); }
    for (int q = 0; q < NS; ++q) {
        if (ck[q]) hipFree(ck[q]);
        if (ev_flags[q]) hipEventDestroy(ev_flags[q]);
        if (ev_copied[q]) hipEventDestroy(ev_copied[q]);
    }
    if (h_poll) hipHostFree(h_poll);
    if (!rc) rc = gpirt_sampler_finish_irfs(s, S_it, h_irfs);
    if (!rc) rc = summary_out();
    g_last_mcmc_fallbacks = h->guard_fallbacks;
    gpirt_sampler_destroy(s);
    drop_handle();
    return rc;
}

int gpirt_mcmc(const double* h_y, int64_t n, int64_t m, const double* h_theta0, int S_it, int B_it,
               const double* h_pm, const double* h_ps, const double* h_step, const gpirt_options* opts,
               gpirt_rstream_t rs, gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws,
               double* h_beta_draws, double* h_f_draws, double* h_irfs)
{
    GP_ARG(h_y && h_theta0 && h_pm && h_ps && h_step && h_theta_draws && h_beta_draws && h_f_draws && h_irfs);
    GP_ARG(n > 0 && m > 0 && S_it >= 0 && B_it >= 0);
    return mcmc_run(h_y, n, m, h_theta0, S_it, B_it, h_pm, h_ps, h_step, opts, rs, tick, tick_ctx, h_theta_draws,
                    h_beta_draws, h_f_draws, h_irfs, nullptr);
}

int gpirt_mcmc_summary(const double* h_y, int64_t n, int64_t m, const double* h_theta0, int S_it, int B_it,
                       const double* h_pm, const double* h_ps, const double* h_step, const gpirt_options* opts,
                       gpirt_rstream_t rs, gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws,
                       double* h_beta_draws, double* h_f_draws, double* h_irfs, gpirt_summary* summary)
{
    GP_ARG(h_y && h_theta0 && h_pm && h_ps && h_step && h_irfs && summary);
    GP_ARG(n > 0 && m > 0 && S_it >= 0 && B_it >= 0);
    const int parts = summary->parts;
    GP_ARG((parts & ~(GPIRT_SUM_THETA_BETA | GPIRT_SUM_F | GPIRT_SUM_PRED | GPIRT_SUM_WAIC)) == 0 && summary->reserved == 0);
    GP_ARG(!((summary->h_p_yes) && !(parts & GPIRT_SUM_PRED)));
    GP_ARG(!((summary->h_lppd || summary->h_p_waic) && !(parts & GPIRT_SUM_WAIC)));
    GP_ARG(!((summary->h_f_mean || summary->h_f_var) && !(parts & GPIRT_SUM_F)));
    GP_ARG(!((summary->h_theta_mean || summary->h_theta_var || summary->h_beta_mean || summary->h_beta_var) && parts == 0));
    return mcmc_run(h_y, n, m, h_theta0, S_it, B_it, h_pm, h_ps, h_step, opts, rs, tick, tick_ctx, h_theta_draws,
                    h_beta_draws, h_f_draws, h_irfs, summary);
}

// ---- several chains ---------------------------------------------------------------------------------------------------
uint64_t gpirt_chain_seed(uint64_t seed, int c)
{
    if (c <= 0) return seed;
    uint64_t z = seed + (uint64_t)c * GPIRT_CHAIN_SEED_GAMMA;
    z = (z ^ (z >> 30)) * GPIRT_CHAIN_SEED_M1;
    z = (z ^ (z >> 27)) * GPIRT_CHAIN_SEED_M2;
    return z ^ (z >> 31);
}

int gpirt_chains_combine(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, int align,
                         double* h_irfs, gpirt_summary* pooled, gpirt_diag* diag)
{
    return chains_combine(h, chains, d_states, signs, align, h_irfs, pooled, diag);
}

// gpirt_mcmc_chains (run == NULL) and gpirt_mcmc_run: the arguments checked as gpirt_mcmc_chains checks them, then run's
// structs; C chains one after another on one handle (chain c: seed gpirt_chain_seed(seed, c), column c of h_theta0;
// run->rs != NULL: R's stream, one chain), each state keeping pooled->parts (with DIAG planned for S; with the quantiles also
// THETA_HIST | IRF_BAND) and accumulating the run's analyses; then gpirt_chains_combine with align and every analysis's
// combine over the same states.  One loop, so every analysis's chains are gpirt_mcmc_chains's chains.
static int chains_run(const double* h_y, int64_t n, int64_t m, const double* h_theta0, int chains, int S_it, int B_it,
                      const double* h_pm, const double* h_ps, const double* h_step, const gpirt_options* opts, int align,
                      gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws, double* h_beta_draws, double* h_f_draws,
                      double* h_irfs, gpirt_summary* pooled, gpirt_diag* diag, const gpirt_run* run)
{
    const gpirt_run none{};
    if (!run) run = &none;
    gpirt_quantiles* const q = run->quantiles;
    gpirt_ppc* const ppc = run->ppc;
    gpirt_ranks* const ranks = run->ranks;
    const double* const h_y_new = run->h_y_new;
    const int64_t n_new = run->n_new;
    gpirt_score* const score = run->score;
    gpirt_score_predict* const predict = run->predict;
    gpirt_ppc_pairs* const pairs = run->pairs;
    gpirt_ppc_bins* const bins = run->bins;
    gpirt_shape* const shape = run->shape;
    gpirt_sumscore* const sumscore = run->sumscore;
    gpirt_ppc_dif* const dif = run->dif;
    gpirt_equate* const equate = run->equate;
    gpirt_loo* const loo = run->loo;
    gpirt_shape_order* const order = run->order;
    GP_ARG(h_y && h_theta0 && h_pm && h_ps && h_step && opts && pooled);
    GP_ARG(n > 0 && m > 0 && chains >= 1 && S_it >= 1 && B_it >= 0);
    // the pooled outputs are checked now, before any chain runs (the combine checks them again against the states)
    const int parts = pooled->parts | GPIRT_SUM_THETA_BETA;
    {
        GP_ARG((pooled->parts & ~(GPIRT_SUM_THETA_BETA | GPIRT_SUM_F | GPIRT_SUM_PRED | GPIRT_SUM_WAIC)) == 0 && pooled->reserved == 0);
        GP_ARG(!(pooled->h_p_yes && !(parts & GPIRT_SUM_PRED)));
        GP_ARG(!((pooled->h_lppd || pooled->h_p_waic) && !(parts & GPIRT_SUM_WAIC)));
        GP_ARG(!((pooled->h_f_mean || pooled->h_f_var) && !(parts & GPIRT_SUM_F)));
    }
    if (diag) {
        GP_ARG(all_zero(diag->reserved));
        GP_ARG((parts & GPIRT_SUM_F) || !(diag->h_f_rhat || diag->h_f_ess || diag->h_f_mcse));
    }
    if (q) {
        GP_ARG(q->reserved0 == 0 && all_zero(q->reserved));
        GP_ARG(q->nprobs >= 0 && (q->nprobs == 0 || q->probs));
        for (int p = 0; p < q->nprobs; ++p) GP_ARG(q->probs[p] >= 0.0 && q->probs[p] <= 1.0);
        GP_ARG((int64_t)chains * S_it < ((int64_t)1 << 32));
    }
    if (ppc) GP_ARG(all_zero(ppc->reserved));
    if (ranks) {
        GP_ARG(ranks->reserved0 == 0 && all_zero(ranks->reserved));
        GP_ARG(ranks->nprobs >= 0 && (ranks->nprobs == 0 || ranks->probs));
        for (int p = 0; p < ranks->nprobs; ++p) GP_ARG(ranks->probs[p] >= 0.0 && ranks->probs[p] <= 1.0);
        GP_ARG((int64_t)chains * S_it < ((int64_t)1 << 32));
        if (n > GPIRT_RANK_MAX_N) { set_error("rank posteriors: n = %lld is beyond %d respondents", (long long)n, GPIRT_RANK_MAX_N); return GPIRT_E_ARG; }
        if (ranks->n_pivots < 0 || ranks->n_pivots > GPIRT_RANK_MAX_PIVOTS) {
            set_error("rank posteriors: %d pivots given, at most %d are taken", ranks->n_pivots, GPIRT_RANK_MAX_PIVOTS);
            return GPIRT_E_ARG;
        }
        for (int p = 0; p < ranks->n_pivots; ++p)
            if (ranks->pivots[p] < 1 || ranks->pivots[p] > n) {
                set_error("rank posteriors: pivot %lld is outside 1..%lld", (long long)ranks->pivots[p], (long long)n);
                return GPIRT_E_ARG;
            }
        GP_ARG(!(ranks->lt && !ranks->pairwise));
    }
    if (score) {
        GP_ARG(score->reserved0 == 0 && all_zero(score->reserved));
        GP_ARG(score->nprobs >= 0 && (score->nprobs == 0 || score->probs));
        for (int p = 0; p < score->nprobs; ++p) GP_ARG(score->probs[p] >= 0.0 && score->probs[p] <= 1.0);
        if (!h_y_new || n_new < 1 || n_new > GPIRT_SCORE_MAX_N) {
            set_error("scoring: n_new = %lld is outside 1..%d", (long long)n_new, GPIRT_SCORE_MAX_N);
            return GPIRT_E_ARG;
        }
        GP_TRY(score_check_new(h_y_new, n_new, m));
    }
    if (predict) {
        GP_ARG(score);
        GP_ARG(predict->reserved0 == 0 && all_zero(predict->reserved));
        GP_TRY(check_top("prediction", predict->top, GPIRT_PREDICT_MAX_TOP));
    }
    if (pairs) {
        GP_ARG(ppc);
        GP_ARG(pairs->reserved0 == 0 && all_zero(pairs->reserved));
        GP_TRY(check_top("pairwise PPC", pairs->top, GPIRT_PAIRS_MAX_TOP));
        if (n > GPIRT_PAIRS_MAX_N) { set_error("pairwise PPC: n = %lld is beyond %d respondents", (long long)n, GPIRT_PAIRS_MAX_N); return GPIRT_E_ARG; }
    }
    if (bins) {
        GP_ARG(ppc);
        GP_ARG(all_zero(bins->reserved));
        GP_TRY(check_top("theta-binned PPC", bins->top, GPIRT_BINS_MAX_TOP));
        GP_TRY(bin_check_cuts(bins->h, bins->cuts));
    }
    if (shape) {
        GP_ARG(all_zero(shape->reserved));
        GP_ARG((int64_t)chains * S_it < ((int64_t)1 << 32));
        GP_TRY(shape_check(shape->k_half, shape->tols, shape->n_tols));
    }
    if (sumscore) {
        GP_ARG(all_zero(sumscore->reserved));
        GP_TRY(sumscore_check(m, sumscore->items, nullptr));
    }
    if (dif) {
        GP_ARG(ppc);
        GP_ARG(dif->reserved0 == 0 && all_zero(dif->reserved));
        GP_TRY(check_top("group-wise PPC", dif->top, GPIRT_DIF_MAX_TOP));
        GP_TRY(dif_check_groups(n, dif->G, dif->groups, nullptr));
        GP_TRY(bin_check_cuts(dif->h, dif->cuts));
    }
    if (equate) {
        GP_ARG(all_zero(equate->reserved));
        GP_TRY(equate_check(m, equate->x, equate->y, nullptr, nullptr));
    }
    if (order) {
        GP_ARG(all_zero(order->reserved));
        if (!shape) {
            set_error("gpirt_mcmc_run: the order posteriors need the shape posteriors (shape is NULL)");
            return GPIRT_E_ARG;
        }
        if (m < 2 || m > GPIRT_ORDER_MAX_M) {
            set_error("order posteriors: m = %lld items, 2..%d are taken", (long long)m, GPIRT_ORDER_MAX_M);
            return GPIRT_E_ARG;
        }
        GP_TRY(check_top("gpirt_mcmc_run", order->top, GPIRT_ORDER_MAX_TOP));
    }
    int64_t loo_M = 0;
    if (loo) {
        GP_ARG(all_zero(loo->reserved));
        GP_ARG(loo->top >= 1 && loo->top <= GPIRT_LOO_MAX_TOP && loo->tail >= 0 && loo->tail <= GPIRT_LOO_MAX_TAIL);
        GP_TRY(loo_tail_length((int64_t)chains * S_it, (int)loo->tail, &loo_M));
    }
    // what the chains read: the run with its in/out structs as they are now (the combines overwrite pivots / n_pivots, h /
    // cuts, k_half / tols)
    gpirt_ranks ranks_in = ranks ? *ranks : gpirt_ranks{};
    gpirt_ppc_bins bins_in = bins ? *bins : gpirt_ppc_bins{};
    gpirt_ppc_dif dif_in = dif ? *dif : gpirt_ppc_dif{};
    gpirt_shape shape_in = shape ? *shape : gpirt_shape{};
    gpirt_run in = *run;
    if (ranks) in.ranks = &ranks_in;
    if (bins) in.bins = &bins_in;
    if (dif) in.dif = &dif_in;
    if (shape) in.shape = &shape_in;
    gpirt_handle_t h = nullptr;
    GP_TRY(gpirt_create_own_stream(&h, opts->device));
    { const long long trip = gpirt_debug_take_mcmc_trip(); if (trip > 0) h->trip_guard_at = trip; }
    std::vector<ChainKeep> keep((size_t)chains);
    LooState& loo_pool = keep[0].loo;                                  // the pooled state: chain 0's, the others merged in
    const int total = S_it + B_it;
    int rc = 0;
    for (int c = 0; c < chains && !rc; ++c) {
        gpirt_options o = *opts;
        o.seed = gpirt_chain_seed(opts->seed, c);
        gpirt_summary sm{};
        sm.parts = parts | (q ? GPIRT_SUM_THETA_HIST | GPIRT_SUM_IRF_BAND : 0);
        ChainKeep& k = keep[(size_t)c];
        const ChainRun cr{ h, c * total, chains * total, (int64_t)chains * S_it, &in, &k };
        std::vector<double> irf_c((size_t)GPIRT_NGRID * (size_t)m);
        rc = mcmc_run(h_y, n, m, h_theta0 + (int64_t)c * n, S_it, B_it, h_pm, h_ps, h_step, &o, run->rs, tick, tick_ctx,
                      h_theta_draws ? h_theta_draws + (int64_t)c * (S_it + 1) * n : nullptr,
                      h_beta_draws ? h_beta_draws + (int64_t)c * 2 * m * (S_it + 1) : nullptr,
                      h_f_draws ? h_f_draws + (int64_t)c * n * m * (S_it + 1) : nullptr, irf_c.data(), &sm, &cr);
        if (loo && c > 0) {                                  // pooled in chain order; the chain's state goes at once
            if (!rc && k.loo.block) rc = launch_loo_merge(h->stream, loo_pool.block, k.loo.block, n, m, loo_M);
            if (hipStreamSynchronize(h->stream) != hipSuccess && !rc) { set_error("LOO merge: the stream failed"); rc = GPIRT_E_HIP; }
            loo_free(&k.loo);
        }
    }
    std::vector<const void*> st((size_t)chains);
    std::vector<int> sg((size_t)chains, 1);
    // st[] := the block that `block` picks from every chain's kept states, then `combine` on them
    auto pool = [&](auto block, auto combine) -> int {
        for (int c = 0; c < chains; ++c) st[(size_t)c] = block(keep[(size_t)c]);
        return combine(st.data());
    };
    using K = const ChainKeep&;
    using St = const void* const*;
    if (!rc) rc = pool([](K k) { return k.sum.block; }, [&](St s) { return chains_combine(h, chains, s, nullptr, align, h_irfs, pooled, diag, sg.data()); });
    if (!rc && q) rc = summary_quantiles(h, chains, st.data(), nullptr, align, q);
    if (!rc && ppc) rc = pool([](K k) { return k.ppc.block; }, [&](St s) { return ppc_combine(h, chains, s, ppc); });
    if (!rc && pairs) rc = pool([](K k) { return k.ppc.pairs.block; }, [&](St s) { return pair_combine(h, chains, s, pairs); });
    if (!rc && bins) rc = pool([](K k) { return k.ppc.bins.block; }, [&](St s) { return bin_combine(h, chains, s, sg.data(), bins); });
    if (!rc && dif) rc = pool([](K k) { return k.ppc.dif.block; }, [&](St s) { return dif_combine(h, chains, s, sg.data(), dif); });
    for (auto& k : keep) summary_free(&k.sum);
    if (!rc && ranks) rc = pool([](K k) { return k.rank.block; }, [&](St s) { return rank_combine(h, chains, s, sg.data(), ranks); });
    if (!rc && score) rc = pool([](K k) { return k.score.block; }, [&](St s) { return score_combine(h, chains, s, sg.data(), score); });
    // (no signs: both sums of the prediction run over the whole grid)
    if (!rc && predict) rc = pool([](K k) { return k.score.pred.block; }, [&](St s) { return pred_combine(h, chains, s, predict); });
    if (!rc && shape) rc = pool([](K k) { return k.shape.block; }, [&](St s) { return shape_combine(h, chains, s, sg.data(), shape); });
    // (no signs: the pair block is the same under theta -> -theta)
    if (!rc && order) rc = pool([](K k) { return k.shape.order.block; }, [&](St s) { return order_combine(h, chains, s, order); });
    if (!rc && sumscore) rc = pool([](K k) { return k.sumscore.block; }, [&](St s) { return sumscore_combine(h, chains, s, sg.data(), sumscore); });
    for (auto& k : keep) shape_free(&k.shape);
    if (!rc && equate) rc = pool([](K k) { return k.equate.block; }, [&](St s) { return equate_combine(h, chains, s, equate); });
    if (!rc && loo) {
        const void* one = loo_pool.block;
        rc = loo_combine(h, 1, &one, loo);
    }
    // the rest, block by block over the chains, not chain by chain: releasing in that order cost about 5 ms more per call at
    // 8192 x 1024 with two chains (in these frees, the samplers' and the handle's), measured with host timers
    loo_free(&loo_pool);
    for (auto& k : keep) sumscore_free(&k.sumscore);
    for (auto& k : keep) equate_free(&k.equate);
    for (auto& k : keep) ppc_free(&k.ppc);
    for (auto& k : keep) rank_free(&k.rank);
    for (auto& k : keep) score_free(&k.score);
    gpirt_destroy(h);
    return rc;
}

int gpirt_mcmc_chains(const double* h_y, int64_t n, int64_t m, const double* h_theta0, int chains, int S_it, int B_it,
                      const double* h_pm, const double* h_ps, const double* h_step, const gpirt_options* opts, int align,
                      gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws, double* h_beta_draws, double* h_f_draws,
                      double* h_irfs, gpirt_summary* pooled, gpirt_diag* diag)
{
    GP_ARG(opts);
    if (opts->rng_kind != GPIRT_RNG_ITEM) {
        set_error("gpirt_mcmc_chains needs GPIRT_RNG_ITEM (each chain keys its draws by gpirt_chain_seed)");
        return GPIRT_E_ARG;
    }
    return chains_run(h_y, n, m, h_theta0, chains, S_it, B_it, h_pm, h_ps, h_step, opts, align, tick, tick_ctx, h_theta_draws,
                      h_beta_draws, h_f_draws, h_irfs, pooled, diag, nullptr);
}

// ---- quantiles --------------------------------------------------------------------------------------------------------
int gpirt_irf_band_edges(double* out)
{
    GP_ARG(out);
    irf_band_edges(out);
    return 0;
}

int gpirt_summary_quantiles(gpirt_handle_t h, int chains, const void* const* d_states, const int* signs, int align,
                            gpirt_quantiles* q)
{
    return summary_quantiles(h, chains, d_states, signs, align, q);
}

// ---- the chains with any of the analyses ------------------------------------------------------------------------------
int gpirt_mcmc_run(const double* h_y, int64_t n, int64_t m, const double* h_theta0, int chains, int S_it, int B_it,
                   const double* h_pm, const double* h_ps, const double* h_step, const gpirt_options* opts, int align,
                   gpirt_tick_fn tick, void* tick_ctx, double* h_theta_draws, double* h_beta_draws, double* h_f_draws,
                   double* h_irfs, gpirt_summary* pooled, gpirt_diag* diag, gpirt_run* run)
{
    GP_ARG(opts && run);
    GP_ARG(all_zero(run->reserved));
    if (run->rs ? (opts->rng_kind != GPIRT_RNG_RSTREAM || chains != 1) : opts->rng_kind != GPIRT_RNG_ITEM) {
        set_error("gpirt_mcmc_run needs GPIRT_RNG_ITEM, or GPIRT_RNG_RSTREAM with rs and one chain");
        return GPIRT_E_ARG;
    }
    return chains_run(h_y, n, m, h_theta0, chains, S_it, B_it, h_pm, h_ps, h_step, opts, align, tick, tick_ctx, h_theta_draws,
                      h_beta_draws, h_f_draws, h_irfs, pooled, diag, run);
}

}  // extern "C"
