// api.hip -- handle management, R's RNG on the host, and the operator-level C ABI (include/gpirt_hip.h).
#include "common.h"
#include "kernels.h"
#include "rstream.h"

#include <stdarg.h>
#include <stdlib.h>
#include <new>
#include <vector>
#include <algorithm>

namespace gpirt {

static thread_local char g_err[512] = "";

// GPIRT_* switches: the environment is read here, once per process; handles copy the result (gpirt_create)
static int env_value(const char* name, int dflt)
{
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    return atoi(v);
}
const Config& env_config()
{
    static const Config c = [] {
        Config d;
        d.nbo = env_value("GPIRT_NBO", d.nbo);            d.nbp = env_value("GPIRT_NBP", d.nbp);
        d.lookahead = env_value("GPIRT_LOOKAHEAD", d.lookahead);
        d.panel = env_value("GPIRT_PANEL", d.panel);      d.defer = env_value("GPIRT_DEFER", d.defer);
        d.trsm_inv = env_value("GPIRT_TRSM_INV", d.trsm_inv);
        d.ll_exact = env_value("GPIRT_LL_EXACT", d.ll_exact);
        d.ess_screen = env_value("GPIRT_ESS_SCREEN", d.ess_screen);
        d.theta_fixed = env_value("GPIRT_THETA_FIXED", d.theta_fixed);
        d.bordered = env_value("GPIRT_BORDERED", d.bordered);
        d.early_inv = env_value("GPIRT_EARLY_INV", d.early_inv);
        d.prep_early = env_value("GPIRT_PREP_EARLY", d.prep_early);
        d.guard_verbose = env_value("GPIRT_GUARD_VERBOSE", d.guard_verbose);
        d.rs_predict = env_value("GPIRT_RS_PREDICT", d.rs_predict);
        d.rs_lr = env_value("GPIRT_RS_LR", d.rs_lr);
        d.nu_lr = env_value("GPIRT_NU_LR", d.nu_lr);
        d.nu_sub = env_value("GPIRT_NU_SUB", NU_LR_SUB);
        d.fstar_free = env_value("GPIRT_FSTAR_FREE", d.fstar_free);
        d.factor_lr = env_value("GPIRT_FACTOR_LR", d.factor_lr);
        d.flr_fuse = env_value("GPIRT_FLR_FUSE", d.flr_fuse);
        d.flr_narrow = env_value("GPIRT_FLR_NARROW", d.flr_narrow);
        d.beta_screen = env_value("GPIRT_BETA_SCREEN", d.beta_screen);
        d.zfill_compact = env_value("GPIRT_ZFILL_COMPACT", d.zfill_compact);
        d.ess_pack = env_value("GPIRT_ESS_PACK", d.ess_pack);
        if (d.nbo < 64) d.nbo = 1024;
        if (d.nbp != 0 && d.nbp < 64) d.nbp = 512;          // (0 = by size: potrf_subpanel_width)
        return d;
    }();
    return c;
}

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int ensure_work(gpirt_handle_t h, size_t bytes)
{
    if (bytes <= h->work_bytes) return 0;
    GP_HIP(hipStreamSynchronize(h->stream));
    if (h->d_work) GP_HIP(hipFree(h->d_work));
    h->d_work = nullptr;
    h->work_bytes = 0;
    hipError_t e = hipMalloc(&h->d_work, bytes);
    if (e != hipSuccess) { set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); return GPIRT_E_ALLOC; }
    h->work_bytes = bytes;
    GP_HIP(poison_fresh(h, h->d_work, bytes, h->stream));
    return 0;
}

static int check_device(int device)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device visible (%s): libgpirt_hip has no CPU fallback",
                  e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return GPIRT_E_NODEVICE;
    }
    if (device >= count) { set_error("device %d out of range (%d visible)", device, count); return GPIRT_E_ARG; }
    return 0;
}

// back-to-back v_mfma_f64_16x16x4_f64 with independent accumulators, operands in registers
__global__ __launch_bounds__(256) void mfma_f64_peak_kernel(double* out, int iters)
{
    d4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
    double a = 1.0 + threadIdx.x * 1e-3, b = 1.0 - threadIdx.x * 1e-3;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// The persistent panel kernel gave up on a progress counter (flagsync.h): info[1] = 1, info[2] = waiting row
// block (absolute), info[3] = awaited row block, info[4..5] = value needed, info[6..7] = value last seen.
int report_panel_guard(gpirt_handle_t h, const int* w, hipStream_t stream)
{
    unsigned long long need = 0, seen = 0;
    memcpy(&need, w + 4, sizeof(need));
    memcpy(&seen, w + 6, sizeof(seen));
    hipMemsetAsync(h->d_info + 1, 0, 7 * sizeof(int), stream);
    set_error("potrf panel kernel: a progress-counter wait expired (device hang guard): row block %d waited for "
              "counter %d to reach %llu, last saw %llu", w[2], w[3], need, seen);
    return GPIRT_E_HIP;
}

int potrf_panel_copy(hipStream_t stream, double* A, int64_t n, int64_t lda, int64_t p, double* buf, bool to_buf,
                     int64_t extra_rows, int half, int64_t capacity)
{
    const int64_t W = potrf_panel_width(), H = potrf_subpanel_width(n), P0 = p * W;
    if (p < 0 || P0 >= n || half < 0 || half > 2) { set_error("panel %lld / half %d out of range", (long long)p, half); return GPIRT_E_ARG; }
    const int64_t P1 = (P0 + W < n) ? P0 + W : n;
    const int64_t mid = (P0 + H < P1) ? P0 + H : P1;
    const int64_t K0 = (half == 1) ? mid : P0, K1 = (half == 0) ? mid : P1;     // the columns that travel
    const int64_t w = K1 - K0, rows = n + extra_rows - K0;
    if (w <= 0) return 0;
    if (capacity >= 0 && rows * w > capacity) {
        set_error("panel copy: part %d of panel %lld is %lld x %lld doubles, the buffer holds %lld", half, (long long)p,
                  (long long)rows, (long long)w, (long long)capacity);
        return GPIRT_E_ARG;
    }
    double* a = A + K0 + K0 * lda;
    if (to_buf) GP_HIP(hipMemcpy2DAsync(buf, (size_t)rows * 8, a, (size_t)lda * 8, (size_t)rows * 8, (size_t)w, hipMemcpyDeviceToDevice, stream));
    else        GP_HIP(hipMemcpy2DAsync(a, (size_t)lda * 8, buf, (size_t)rows * 8, (size_t)rows * 8, (size_t)w, hipMemcpyDeviceToDevice, stream));
    return 0;
}

}  // namespace gpirt

using namespace gpirt;

static int create_own_stream(gpirt_handle_t* out, int device, bool high_priority);
namespace gpirt {
// a handle on a high-priority stream of its own: the sampler's side work must win free slots against resident kernels
int create_side_handle(gpirt_handle_t* out, int device) { return create_own_stream(out, device, true); }
}

namespace gpirt {
int prof_pair_begin(gpirt_handle_t h, hipStream_t stream, ProfPair& pp)
{
    pp = ProfPair{nullptr, nullptr, 0.0, 0, 0.0};
    if (!h->prof.enabled) return 0;
    if (!h->prof.free_pairs.empty()) { pp = h->prof.free_pairs.back(); h->prof.free_pairs.pop_back(); }
    else { GP_HIP(hipEventCreate(&pp.e0)); GP_HIP(hipEventCreate(&pp.e1)); }
    GP_HIP(hipEventRecord(pp.e0, stream));
    return 0;
}
int prof_pair_end(gpirt_handle_t h, hipStream_t stream, ProfPair& pp, int cls, double flops, double bytes)
{
    if (!pp.e0) return 0;
    GP_HIP(hipEventRecord(pp.e1, stream));
    pp.flops = flops; pp.bytes = bytes; pp.cls = cls;
    h->prof.pending.push_back(pp);
    return 0;
}
}  // namespace gpirt

extern "C" {

int gpirt_version(void) { return 144; }   // 101: gpirt_options names kernel_fp32 / kstar_rank, gpirt_fast_options;
                                            // 102: gpirt_potrf_subpanel_width takes the order of the matrix, gpirt_debug_theta_*
                                            // 103: gpirt_debug_poison_allocs; draw_f and the sampler refuse y outside {+1, -1, NaN}
                                            // 104: posterior summaries (gpirt_sampler_summary_*, gpirt_mcmc_summary, summary.hip)
                                            // 105: several chains, split-R-hat / ESS / MCSE (GPIRT_SUM_DIAG, gpirt_chains_combine,
                                            //      gpirt_mcmc_chains, gpirt_chain_seed)
                                            // 106: quantiles -- theta histograms, IRF bands, rank-normalised R-hat
                                            //      (GPIRT_SUM_THETA_HIST, GPIRT_SUM_IRF_BAND, gpirt_summary_quantiles,
                                            //      gpirt_irf_band_edges)
                                            // 107: posterior predictive checks (ppc.hip: gpirt_sampler_ppc_*, gpirt_ppc_combine)
                                            // 108: rank posteriors (ranks.hip: gpirt_sampler_rank_*, gpirt_rank_combine)
                                            // 109: scoring new respondents (score.hip: gpirt_sampler_score_*, gpirt_score_combine)
                                            // 110: predicting new respondents' unseen answers and the next item to ask (predict.hip:
                                            //      gpirt_sampler_score_predict_*, gpirt_score_predict_combine)
                                            // 111: pairwise item checks of the PPC (ppc_pairs.hip: gpirt_sampler_ppc_pairs_*,
                                            //      gpirt_ppc_pairs_combine)
                                            // 112: theta-binned item fit of the PPC (ppc_bins.hip: gpirt_sampler_ppc_bins_*,
                                            //      gpirt_ppc_bins_combine)
                                            // 113: IRF shape posteriors (shape.hip: gpirt_sampler_shape_*, gpirt_shape_state_bytes,
                                            //      gpirt_shape_combine; the sampler array "gbar")
                                            // 114: sum-score posteriors (sumscore.hip: gpirt_sampler_sumscore_*, gpirt_sumscore_state_bytes,
                                            //      gpirt_sumscore_grid_weights, gpirt_sumscore_combine)
                                            // 115: group-wise item fit of the PPC (ppc_dif.hip: gpirt_sampler_ppc_dif_*,
                                            //      gpirt_ppc_dif_combine)
                                            // 116: two-form score equating (equate.hip: gpirt_sampler_equate_*, gpirt_equate_state_bytes,
                                            //      gpirt_equate_combine)
                                            // 117: PSIS-LOO (loo.hip: gpirt_sampler_loo_*, gpirt_loo_tail_length, gpirt_loo_state_bytes,
                                            //      gpirt_loo_combine)
                                            // 118: item-pair IRF order posteriors (order.hip: gpirt_sampler_shape_order_*,
                                            //      gpirt_shape_order_state_bytes, gpirt_shape_order_combine)
                                            // 119: gpirt_mcmc_run with a gpirt_run (sampler.hip) replaces the whole-call entries that 106 to 118
                                            //      added one per analysis, each the one before with one more parameter
                                            // 120: score-based checks of the PPC (ppc_scores.hip: gpirt_sampler_ppc_scores_*,
                                            //      gpirt_ppc_scores_check, gpirt_ppc_scores_combine)
                                            // 121: person fit of the PPC (ppc_person.hip: gpirt_sampler_ppc_person_*,
                                            //      gpirt_ppc_person_check, gpirt_ppc_person_combine)
                                            // 122: autocorrelation ESS (acf.hip: gpirt_acf_check, gpirt_sampler_acf_*, gpirt_acf_combine)
                                            // 123: residual correlations of the PPC (ppc_resid.hip: gpirt_sampler_ppc_resid_*,
                                            //      gpirt_ppc_resid_combine)
                                            // 124: the covariance kernel per handle -- squared exponential with a length scale, Matern
                                            //      5/2 and 3/2 (se_kernel.hip: gpirt_kernel_default, gpirt_kernel_check, gpirt_kernel_set,
                                            //      gpirt_kernel_get); gpirt_options, gpirt_run and the gpirt_mcmc* entries are unchanged
                                            // 125: the length scale as a parameter of the chain (ell.hip, sampler.hip: gpirt_ell_grid,
                                            //      gpirt_ell_check, gpirt_sampler_ell_*, gpirt_sampler_draw_ell); stage API only
                                            // 127: group posteriors (groups.hip: gpirt_groups_check, gpirt_sampler_groups_*,
                                            //      gpirt_groups_combine); stage API only
                                            // 128: draw_f's nu = L z from L's diagonal parts and 64 node rows below the factor (nu_lr.hip:
                                            //      GPIRT_NU_LR, gpirt_sampler_nu_lr_draws, gpirt_sampler_nu_lr_rows; every bordered layout
                                            //      carries the node rows, gpirt_sampler_ldl)
                                            // 129: per-item GP amplitudes, fixed or sampled in the chain (amp.hip, sampler.hip:
                                            //      gpirt_amp_check, gpirt_sampler_amp_*, gpirt_sampler_draw_amp); stage API only
                                            // 130: the rank-64 draw_fstar's C = S^-1 U from theta alone, without the solve through L
                                            //      (fstar_free.hip: GPIRT_FSTAR_FREE, gpirt_sampler_fstar_free_draws)
                                            // 131: gpirt_options.factor_structured (gpirt_fast_options sets it): L's diagonal parts and node
                                            //      rows alone, from theta (factor_lr.hip: GPIRT_FACTOR_LR, gpirt_sampler_factor_lr_count,
                                            //      gpirt_sampler_dense_factor_count, gpirt_sampler_dense_factor, gpirt_sampler_factor_lr_parts)
                                            // 132: the structured factor runs one launch per 64-column round (factor_lr.hip: GPIRT_FLR_FUSE; 2 = the
                                            //      launches of version 131); the same bits, no change to the interface
                                            // 133: a consistent step beside the reference's: f carried to the new theta plus the model's
                                            //      nugget, and the prior check (carry.hip, sampler.hip: GPIRT_ST_CARRY, gpirt_sampler_carry_f,
                                            //      gpirt_sampler_step_consistent, gpirt_sampler_carry_stats, gpirt_sampler_prior_quad); stage
                                            //      API only, gpirt_sampler_step and every existing stage's uniforms are unchanged
                                            // 134: a population prior for theta: a table of log masses per group, fixed or with the groups'
                                            //      means and sds sampled by exact Gibbs on two grids (pop.hip, sampler.hip: GPIRT_ST_POP,
                                            //      gpirt_pop_check, gpirt_sampler_pop_*, gpirt_sampler_draw_pop); stage API only
                                            // 135: a centred amplitude update on the GP's rank-64 smooth part beside the whitened one
                                            //      (amp_centred.hip, sampler.hip: GPIRT_ST_AMP_CENTRED, gpirt_sampler_draw_amp_centred,
                                            //      gpirt_sampler_amp_centred_stats, new names of gpirt_sampler_amp_get); stage API only
                                            // 136: a centred beta update, exact Gibbs for the mean's coefficients with f + mu held fixed
                                            //      (beta_centred.hip, sampler.hip: GPIRT_ST_BETA_CENTRED, gpirt_sampler_draw_beta_centred,
                                            //      gpirt_sampler_beta_centred_get, gpirt_sampler_beta_centred_stats); stage API only
                                            // 137: a collapsed scale and shift move on the linear mean with theta summed out (scale.hip,
                                            //      sampler.hip: GPIRT_ST_SCALE, gpirt_sampler_scale_enable, gpirt_sampler_draw_scale,
                                            //      gpirt_sampler_scale_width / _get / _stats, gpirt_sampler_step_consistent_scale); stage API only
                                            // 138: draw_f's structured product in parts of its own width, narrower than the factor's 512, with
                                            //      the rank-64 term accumulated in the launch of the diagonal parts (nu_lr.hip, gemm_f64.hip:
                                            //      GPIRT_NU_SUB = 64, 128, 256 or 512); nu changes in rounding only, no change to the interface
                                            // 139: ordinal (graded) responses under the cumulative-logit model, the thresholds sampled on a grid
                                            //      (ordinal.hip, sampler.hip: GPIRT_ST_ORD, gpirt_ordinal_check, gpirt_ordinal_grid,
                                            //      gpirt_sampler_ordinal_enable / _width / _record / _accumulate_irf / _get / _stats,
                                            //      gpirt_sampler_draw_thresholds); stage API only
                                            // 140: the structured factor's parts as narrow as draw_f's product reads them, part / 64 rounds instead
                                            //      of eight (factor_lr.hip: GPIRT_FLR_NARROW, gpirt_sampler_factor_lr_width,
                                            //      gpirt_sampler_factor_lr_blocks); the parts and node rows change in rounding only
                                            // 143: draw_f's slice kernel of 2048 < n <= 8192 with y packed and mu formed again from theta and
                                            //      beta (ess_lin.hip: GPIRT_ESS_PACK, gpirt_draw_f_linear, gpirt_sampler_ess_pack_draws); bit for bit
                                            // 144: scoring new respondents under ordinal responses: theta posterior, lpd, category predictions and
                                            //      the next item (ordinal_score.hip, sampler.hip: gpirt_sampler_ordinal_score_enable / _accumulate /
                                            //      _get / _state / _predict_state, gpirt_ordinal_score_combine, gpirt_ordinal_score_predict_combine);
                                            //      stage API only, every existing kernel's output is unchanged

const char* gpirt_last_error(void) { return g_err; }

int gpirt_device_count(int* count)
{
    GP_ARG(count != nullptr);
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *count = (e == hipSuccess) ? c : 0;
    return 0;
}

int gpirt_create(gpirt_handle_t* out, int device, void* stream)
{
    GP_ARG(out != nullptr);
    *out = nullptr;
    GP_TRY(check_device(device < 0 ? 0 : device));
    if (device >= 0) GP_HIP(hipSetDevice(device));
    int cur = 0;
    GP_HIP(hipGetDevice(&cur));
    hipDeviceProp_t prop;
    GP_HIP(hipGetDeviceProperties(&prop, cur));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; libgpirt_hip is built for gfx950 (MI355X) only", cur, prop.gcnArchName);
        return GPIRT_E_NODEVICE;
    }
    gpirt_handle_s* h = new (std::nothrow) gpirt_handle_s();
    if (!h) { set_error("out of host memory"); return GPIRT_E_ALLOC; }
    h->device = cur;
    h->cfg = env_config();
    h->n_cu = prop.multiProcessorCount;
    // stream == NULL is HIP's default (null) stream, like every hipStream_t argument
    h->stream = (hipStream_t)stream;
    h->own_stream = false;
    // Every word the kernels poll or publish (potrf info + hang-guard record, the panel kernel's progress
    // counters) is cleared ON THE HANDLE'S STREAM and the stream is drained before the handle is handed out:
    // a null-stream hipMemset is not ordered against a hipStreamNonBlocking stream (gpirt_create_own_stream),
    // so a kernel launched there could start on recycled, uncleared words or have its counters zeroed under it.
    const size_t prog_cap = 2048;        // 64-row blocks: n <= 131008 without growing
    hipError_t e = hipMalloc(&h->d_info, 64);
    if (e == hipSuccess) e = hipMalloc(&h->d_prog, 2 * prog_cap * sizeof(unsigned long long));   // row-block counters | column counters (panel.hip)
    if (e == hipSuccess) e = hipHostMalloc(&h->h_info, 64, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_info, 0, 64, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_prog, 0, 2 * prog_cap * sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        set_error("handle workspace setup failed: %s", hipGetErrorString(e));
        gpirt_destroy(h);
        return GPIRT_E_ALLOC;
    }
    h->prog_cap = prog_cap;
    *out = h;
    return 0;
}

int gpirt_destroy(gpirt_handle_t h)
{
    if (!h) return 0;
    if (h->live_samplers > 0) { h->zombie = true; return 0; }     // freed by the last sampler's destroy (common.h)
    hipStreamSynchronize(h->stream);
    if (h->d_info) hipFree(h->d_info);
    if (h->h_info) hipHostFree(h->h_info);
    if (h->d_work) hipFree(h->d_work);
    if (h->d_prog) hipFree(h->d_prog);
    if (h->d_winv) hipFree(h->d_winv);
    if (h->d_splitk) hipFree(h->d_splitk);
    if (h->d_trsm_winv) hipFree(h->d_trsm_winv);
    if (h->d_trsm_tmp) hipFree(h->d_trsm_tmp);
    if (h->d_trsm_wquad) hipFree(h->d_trsm_wquad);
    for (auto& pp : h->prof.pending) { hipEventDestroy(pp.e0); hipEventDestroy(pp.e1); }
    for (auto& pp : h->prof.free_pairs) { hipEventDestroy(pp.e0); hipEventDestroy(pp.e1); }
    if (h->side) hipStreamDestroy(h->side);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->ev_mid) hipEventDestroy(h->ev_mid);
    if (h->ev_half) hipEventDestroy(h->ev_half);
    if (h->ev_prelast) hipEventDestroy(h->ev_prelast);
    if (h->panel_trace && h->panel_trace_cap > 0) hipFree(h->panel_trace);
    if (h->aux) { hipStreamSynchronize(h->aux->stream); gpirt_destroy(h->aux); h->aux = nullptr; }
    if (h->d_defer_ws) hipFree(h->d_defer_ws);

    if (h->own_stream) hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

int gpirt_synchronize(gpirt_handle_t h)
{
    GP_ARG(h != nullptr);
    GP_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

static int create_own_stream(gpirt_handle_t* out, int device, bool high_priority)
{
    GP_ARG(out != nullptr);
    *out = nullptr;
    GP_TRY(check_device(device < 0 ? 0 : device));
    if (device >= 0) GP_HIP(hipSetDevice(device));
    hipStream_t st = nullptr;
    int lo_pri = 0, hi_pri = 0;
    hipError_t e = hipSuccess;
    if (high_priority) e = hipDeviceGetStreamPriorityRange(&lo_pri, &hi_pri);
    if (e == hipSuccess)
        e = high_priority ? hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi_pri)
                          : hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e != hipSuccess) { set_error("hipStreamCreate failed: %s", hipGetErrorString(e)); return GPIRT_E_HIP; }
    // the handle is set up ON this stream (gpirt_create clears its workspace there and drains it)
    const int rc = gpirt_create(out, device, st);
    if (rc != 0) { hipStreamDestroy(st); return rc; }
    (*out)->own_stream = true;
    return 0;
}

int gpirt_create_own_stream(gpirt_handle_t* out, int device) { return create_own_stream(out, device, false); }

// The library's switches (README.md), per handle: the value the environment gave at process start, or what a caller set
// here since.  Geometry (GPIRT_NBO / GPIRT_NBP) is per process and read-only.  Takes effect at the next call that uses it;
// samplers of the handle read it when they run, their layout switch (GPIRT_BORDERED) when they are created.
static int* config_slot(gpirt_handle_t h, const char* name, bool* read_only)
{
    struct E { const char* k; int* p; bool ro; } tab[] = {
        { "GPIRT_NBO", &h->cfg.nbo, true }, { "GPIRT_NBP", &h->cfg.nbp, true },
        { "GPIRT_LOOKAHEAD", &h->cfg.lookahead, false }, { "GPIRT_PANEL", &h->cfg.panel, false },
        { "GPIRT_DEFER", &h->cfg.defer, false }, { "GPIRT_TRSM_INV", &h->cfg.trsm_inv, false },
        { "GPIRT_LL_EXACT", &h->cfg.ll_exact, false }, { "GPIRT_ESS_SCREEN", &h->cfg.ess_screen, false }, { "GPIRT_THETA_FIXED", &h->cfg.theta_fixed, false }, { "GPIRT_BORDERED", &h->cfg.bordered, false },
        { "GPIRT_EARLY_INV", &h->cfg.early_inv, false }, { "GPIRT_PREP_EARLY", &h->cfg.prep_early, false },
        { "GPIRT_RS_PREDICT", &h->cfg.rs_predict, false },
        { "GPIRT_RS_LR", &h->cfg.rs_lr, false },
        { "GPIRT_NU_LR", &h->cfg.nu_lr, false },
        { "GPIRT_NU_SUB", &h->cfg.nu_sub, false },
        { "GPIRT_FSTAR_FREE", &h->cfg.fstar_free, false },
        { "GPIRT_FACTOR_LR", &h->cfg.factor_lr, false },
        { "GPIRT_FLR_FUSE", &h->cfg.flr_fuse, false },
        { "GPIRT_FLR_NARROW", &h->cfg.flr_narrow, false },
        { "GPIRT_BETA_SCREEN", &h->cfg.beta_screen, false },
        { "GPIRT_ZFILL_COMPACT", &h->cfg.zfill_compact, false },
        { "GPIRT_ESS_PACK", &h->cfg.ess_pack, false },
    };
    for (auto& e : tab)
        if (strcmp(e.k, name) == 0) { if (read_only) *read_only = e.ro; return e.p; }
    return nullptr;
}

int gpirt_config_get(gpirt_handle_t h, const char* name, int* value)
{
    GP_ARG(h && name && value);
    int* p = config_slot(h, name, nullptr);
    if (!p) { set_error("unknown switch '%s'", name); return GPIRT_E_ARG; }
    *value = *p;
    return 0;
}

int gpirt_config_set(gpirt_handle_t h, const char* name, int value)
{
    GP_ARG(h && name);
    bool ro = false;
    int* p = config_slot(h, name, &ro);
    if (!p) { set_error("unknown switch '%s'", name); return GPIRT_E_ARG; }
    if (ro) { set_error("%s is fixed per process (set it in the environment before the library is loaded)", name); return GPIRT_E_ARG; }
    if (p == &h->cfg.nu_sub && !nu_lr_sub_ok(value)) { set_error("GPIRT_NU_SUB must be 64, 128, 256 or 512 (got %d)", value); return GPIRT_E_ARG; }
    GP_HIP(hipStreamSynchronize(h->stream));
    *p = value;
    if (h->aux) *config_slot(h->aux, name, nullptr) = value;
    return 0;
}

// The covariance kernel (include/gpirt_hip.h, "the covariance kernel"; device code and certificate: se_kernel.hip)
void gpirt_kernel_default(gpirt_kernel* k)
{
    if (!k) return;
    memset(k, 0, sizeof(*k));
    k->family = GPIRT_KERNEL_SE;
    k->length_scale = 1.0;
}

int gpirt_kernel_check(const gpirt_kernel* k, int kstar_rank, double* cert_out, int* min_rank_out)
{
    if (cert_out) *cert_out = 0.0;
    if (min_rank_out) *min_rank_out = 0;
    KernelSpec spec;
    GP_TRY(kernel_spec_from(k, &spec));
    return kernel_rank_check(spec, kstar_rank, cert_out, min_rank_out);
}

int gpirt_kernel_set(gpirt_handle_t h, const gpirt_kernel* k)
{
    GP_ARG(h != nullptr);
    KernelSpec spec;
    GP_TRY(kernel_spec_from(k, &spec));
    if (h->live_samplers > 0) {
        set_error("gpirt_kernel_set: %d sampler(s) created on this handle are alive; a sampler keeps the kernel it was created "
                  "under -- destroy them first", h->live_samplers);
        return GPIRT_E_ARG;
    }
    GP_HIP(hipStreamSynchronize(h->stream));
    h->kern = spec;
    if (h->aux) h->aux->kern = spec;
    return 0;
}

int gpirt_kernel_get(gpirt_handle_t h, gpirt_kernel* k)
{
    GP_ARG(h && k);
    gpirt_kernel_default(k);
    k->family = h->kern.family;
    k->length_scale = h->kern.length_scale;
    return 0;
}

int gpirt_set_stream(gpirt_handle_t h, void* stream)
{
    GP_ARG(h != nullptr);
    GP_HIP(hipStreamSynchronize(h->stream));
    if (h->own_stream) { hipStreamDestroy(h->stream); h->own_stream = false; }
    h->stream = (hipStream_t)stream;
    return 0;
}

int gpirt_calibrate_mfma_f64(gpirt_handle_t h, double* tflops)
{
    GP_ARG(h != nullptr && tflops != nullptr);
    const int blocks = 256 * 8, iters = 4096;
    GP_TRY(ensure_work(h, (size_t)blocks * 256 * sizeof(double)));
    hipEvent_t e0, e1;
    GP_HIP(hipEventCreate(&e0));
    GP_HIP(hipEventCreate(&e1));
    double best = 0.0;
    for (int rep = 0; rep < 4; ++rep) {
        GP_HIP(hipEventRecord(e0, h->stream));
        hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, h->stream, h->d_work, iters);
        GP_HIP(hipEventRecord(e1, h->stream));
        GP_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        GP_HIP(hipEventElapsedTime(&ms, e0, e1));
        const double flops = (double)blocks * 4.0 * iters * 8.0 * 2048.0;   // waves * mfma * flop
        const double tf = flops / (ms * 1e-3) / 1e12;
        if (tf > best) best = tf;
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    *tflops = best;
    return 0;
}

static int finish_info(gpirt_handle_t h)
{
    GP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 8 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));
    const int info = *h->h_info;
    if (h->h_info[1] != 0) return report_panel_guard(h, h->h_info, h->stream);
    if (info > 0) set_error("chol(): decomposition failed (leading minor of order %d is not positive definite)", info);
    return info;
}

int gpirt_se_kernel(gpirt_handle_t h, const double* d_x1, int64_t n1, const double* d_x2, int64_t n2,
                    double* d_out, int64_t ld, double jitter)
{
    GP_ARG(h && d_x1 && d_x2 && d_out && n1 >= 0 && n2 >= 0 && ld >= n1);
    return launch_se_kernel(h->stream, h->kern, d_x1, n1, d_x2, n2, d_out, ld, jitter);
}

int gpirt_potrf_lower(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda)
{
    GP_ARG(h && d_A && n >= 0 && lda >= n);
    GP_TRY(launch_potrf_lower(h, h->stream, d_A, n, lda, true));
    return finish_info(h);
}

int gpirt_factor(gpirt_handle_t h, const double* d_theta, int64_t n, double* d_L, int64_t ldl)
{
    GP_ARG(h && d_theta && d_L && n >= 0 && ldl >= n);
    GP_TRY(launch_se_kernel(h->stream, h->kern, d_theta, n, d_theta, n, d_L, ldl, GPIRT_JITTER));
    GP_TRY(launch_potrf_lower(h, h->stream, d_L, n, ldl, true));
    GP_HIP(hipMemcpyAsync(h->h_info, h->d_info, 8 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));
    if (h->h_info[1] != 0 && h->cfg.panel != 2) {
        // The persistent panel kernel gave up on a progress counter (its work-groups were not co-resident in time, e.g.
        // beside a foreign tenant).  theta is intact, so K is rebuilt and factored once more with the launch-per-step
        // panel; only a failure of THAT is an error.
        GP_TRY(potrf_guard_reset(h, h->stream));
        const int saved = h->cfg.panel;
        h->cfg.panel = 2;
        int rc = launch_se_kernel(h->stream, h->kern, d_theta, n, d_theta, n, d_L, ldl, GPIRT_JITTER);
        if (!rc) rc = launch_potrf_lower(h, h->stream, d_L, n, ldl, true);
        h->cfg.panel = saved;
        GP_TRY(rc);
    }
    return finish_info(h);
}

int gpirt_guard_fallbacks(gpirt_handle_t h, int* count)
{
    GP_ARG(h && count);
    *count = h->guard_fallbacks;
    return 0;
}

// Debug: the nth factorisation from now on this handle (nth >= 1; 0 disarms) ends as a hang-guard expiry would leave it --
// guard word raised, result unfinished -- so the fallback can be tested without spinning a kernel to its bound.
// h == NULL arms the NEXT handle gpirt_mcmc creates for itself.
static long long g_trip_next_mcmc = 0;
// Tests only: the replay's speculative draw_f (rng_ess.hip) finds a candidate for rejection counts < limit only (0: all 32),
// so that the redo-one-item-the-plain-way path, which a real chain takes once in many thousand items, runs every few items.
int gpirt_debug_rs_cand_limit(gpirt_handle_t h, int limit)
{
    GP_ARG(h != nullptr && limit >= 0);
    h->rs_cand_limit = limit;
    return 0;
}

// Tests only: the predictor of the R-stream replay's draw_f (rs_predict.hip) reports one uniform too many for every
// every-th item (0: never), so that the verification's discard-and-resume path, which a real chain takes about once in
// 1e5 trial points, runs at will.  The committed draws must not change.
int gpirt_debug_rs_mispredict(gpirt_handle_t h, int every)
{
    GP_ARG(h != nullptr && every >= 0);
    h->rs_mispredict = every;
    return 0;
}

// Tests only: every floating buffer a sampler on this handle allocates from now on, and every floating workspace the handle
// (or its side handle) grows, starts as 0xFF bytes -- a quiet NaN in fp64 and fp32 (poison_fresh, common.h) -- so that a read
// of memory nothing wrote changes the numbers or raises a named error instead of depending on what the allocator hands out.
// Integer, flag, ticket and counter buffers are never poisoned.
int gpirt_debug_poison_allocs(gpirt_handle_t h, int on)
{
    GP_ARG(h != nullptr && on >= 0);
    h->poison_allocs = on ? 1 : 0;
    if (h->aux) h->aux->poison_allocs = h->poison_allocs;
    return 0;
}

// Debug: pass number `pass` of every replayed draw_f on this handle leaves in-kernel time stamps in the sampler's "rs_trace"
// array (128 64-bit words, 100 MHz wall clock: tools/rs_trace.py); pass < 0 switches it off.
int gpirt_debug_rs_trace(gpirt_handle_t h, int pass)
{
    GP_ARG(h != nullptr);
    h->rs_trace_pass = pass;
    return 0;
}

int gpirt_debug_trip_guard(gpirt_handle_t h, int nth)
{
    GP_ARG(nth >= 0);
    if (!h) { g_trip_next_mcmc = nth; return 0; }
    h->trip_guard_at = nth > 0 ? h->factor_count + nth : -1;
    return 0;
}
long long gpirt_debug_take_mcmc_trip(void) { const long long v = g_trip_next_mcmc; g_trip_next_mcmc = 0; return v; }

// ---- distributed factorisation pieces (no host synchronisation; info is read by gpirt_potrf_finish) ----------------
int64_t gpirt_potrf_panel_width(void) { return potrf_panel_width(); }

int gpirt_potrf_begin(gpirt_handle_t h)
{
    GP_ARG(h != nullptr);
    GP_HIP(hipMemsetAsync(h->d_info, 0, sizeof(int), h->stream));
    return 0;
}

int gpirt_potrf_panel_factor(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p)
{
    GP_ARG(h && d_A && n > 0 && lda >= n);
    return potrf_panel_factor(h, h->stream, d_A, n, lda, p);
}

int gpirt_potrf_panel_update(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, int64_t c)
{
    GP_ARG(h && d_A && n > 0 && lda >= n);
    return potrf_panel_update(h, h->stream, d_A, n, lda, p, c);
}

// rows [pW, n) of outer panel p <-> a dense (n - pW) x w buffer (w = the panel's column count)
int gpirt_potrf_panel_copy(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, double* d_buf, int to_buf)
{
    GP_ARG(h && d_A && d_buf && n > 0 && lda >= n && p >= 0);
    return potrf_panel_copy(h->stream, d_A, n, lda, p, d_buf, to_buf != 0, 0);
}

// the same three pieces by halves of an outer panel (its first sub-panel / the rest): the pipeline of a distributing host
int64_t gpirt_potrf_subpanel_width(int64_t n) { return potrf_subpanel_width(n); }

int gpirt_potrf_panel_factor_part(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, int half)
{
    GP_ARG(h && d_A && n > 0 && lda >= n);
    return potrf_panel_factor(h, h->stream, d_A, n, lda, p, 0, half);
}

int gpirt_potrf_panel_update_part(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, int64_t c, int part)
{
    GP_ARG(h && d_A && n > 0 && lda >= n);
    return potrf_panel_update(h, h->stream, d_A, n, lda, p, c, 0, part);
}

int gpirt_potrf_panel_copy_part(gpirt_handle_t h, double* d_A, int64_t n, int64_t lda, int64_t p, int half, double* d_buf,
                                int64_t buf_doubles, int to_buf)
{
    GP_ARG(h && d_A && d_buf && n > 0 && lda >= n && p >= 0 && buf_doubles >= 0);
    return potrf_panel_copy(h->stream, d_A, n, lda, p, d_buf, to_buf != 0, 0, half, buf_doubles);
}

// Debug aid for hosts that put collectives between the pieces: every piece must have joined the handle's stream before it
// returns (the library forks look-ahead work onto streams of its own).  *busy = bit mask of the handle's internal streams
// that still have work in flight (0 = all idle): bit 0 = the look-ahead side stream.  Does not synchronise.
int gpirt_debug_streams_busy(gpirt_handle_t h, int* busy)
{
    GP_ARG(h && busy);
    int m = 0;
    if (h->side && hipStreamQuery(h->side) == hipErrorNotReady) m |= 1;
    (void)hipGetLastError();
    *busy = m;
    return 0;
}

int gpirt_debug_panel_trace(gpirt_handle_t h, int64_t k0, long long* host_out, int64_t count)
{
    GP_ARG(h && count >= 0);
    if (!host_out) {            // arm: the sub-panel launch that starts at column k0 stamps [row block][40 steps][8 slots]
        GP_HIP(hipStreamSynchronize(h->stream));
        if (h->panel_trace_cap < count) {
            if (h->panel_trace && h->panel_trace_cap > 0) GP_HIP(hipFree(h->panel_trace));
            h->panel_trace = nullptr; h->panel_trace_cap = 0;
            GP_HIP(hipMalloc(&h->panel_trace, (size_t)count * sizeof(long long)));
            h->panel_trace_cap = count;
        }
        if (count == 0) { h->panel_trace_k0 = -1; if (h->panel_trace_cap > 0) { GP_HIP(hipFree(h->panel_trace)); h->panel_trace = nullptr; h->panel_trace_cap = 0; } return 0; }
        GP_HIP(hipMemsetAsync(h->panel_trace, 0, (size_t)count * sizeof(long long), h->stream));
        GP_HIP(hipStreamSynchronize(h->stream));
        h->panel_trace_k0 = k0;
        return 0;
    }
    GP_ARG(h->panel_trace && count <= h->panel_trace_cap);
    GP_HIP(hipDeviceSynchronize());
    GP_HIP(hipMemcpy(host_out, h->panel_trace, (size_t)count * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

int gpirt_debug_ll_term(gpirt_handle_t h, const double* d_a, int64_t n, double* d_out, int fast)
{
    GP_ARG(h && (n == 0 || (d_a && d_out)) && n >= 0);
    return launch_ll_term_probe(h->stream, d_a, n, d_out, fast);
}

int gpirt_potrf_finish(gpirt_handle_t h)
{
    GP_ARG(h != nullptr);
    return finish_info(h);
}

int gpirt_trmm_lz(gpirt_handle_t h, const double* d_L, int64_t n, int64_t ldl, const double* d_Z,
                  int64_t m, int64_t ldz, double* d_out, int64_t ldo)
{
    GP_ARG(h && d_L && d_Z && d_out && n >= 0 && m >= 0 && ldl >= n && ldz >= n && ldo >= n);
    return launch_gemm(h, h->stream, false, false, TRI_A_LOWER, n, m, n, 1.0, d_L, ldl, d_Z, ldz, 0.0, d_out, ldo);
}

int gpirt_trsm_lower(gpirt_handle_t h, const double* d_L, int64_t n, int64_t ldl, double* d_B,
                     int64_t nrhs, int64_t ldb, int trans)
{
    GP_ARG(h && d_L && d_B && n >= 0 && nrhs >= 0 && ldl >= n && ldb >= n);
    return launch_trsm_lower(h, h->stream, d_L, n, ldl, d_B, nrhs, ldb, trans != 0);
}

int gpirt_gemm(gpirt_handle_t h, int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha,
               const double* d_A, int64_t lda, const double* d_B, int64_t ldb, double beta,
               double* d_C, int64_t ldc)
{
    GP_ARG(h && d_A && d_B && d_C && M >= 0 && N >= 0 && K >= 0);
    GP_ARG(lda >= (ta ? K : M) && ldb >= (tb ? N : K) && ldc >= M);
    return launch_gemm(h, h->stream, ta != 0, tb != 0, TRI_NONE, M, N, K, alpha, d_A, lda, d_B, ldb, beta, d_C, ldc);
}

int gpirt_ll_bar(gpirt_handle_t h, const double* d_f, const double* d_y, const double* d_mu,
                 int64_t n, int64_t m, double* d_out)
{
    GP_ARG(h && d_f && d_y && d_out && n >= 0 && m >= 0);
    return launch_ll_bar(h->stream, d_f, d_y, d_mu, n, m, d_out);
}

int gpirt_item_uniforms(gpirt_handle_t h, uint64_t seed, uint32_t iter, uint32_t stage,
                        uint32_t item0, int64_t n_items, int64_t n_index, double* d_out)
{
    GP_ARG(h && d_out && n_items >= 0 && n_index >= 0);
    return launch_item_uniforms(h->stream, seed, iter, stage, item0, n_items, n_index, d_out, false);
}

int gpirt_item_normals(gpirt_handle_t h, uint64_t seed, uint32_t iter, uint32_t stage,
                       uint32_t item0, int64_t n_items, int64_t n_index, double* d_out)
{
    GP_ARG(h && d_out && n_items >= 0 && n_index >= 0);
    return launch_item_uniforms(h->stream, seed, iter, stage, item0, n_items, n_index, d_out, true, h->cfg.zfill_compact == 1);
}

int gpirt_draw_f(gpirt_handle_t h, double* d_f, const double* d_y, const double* d_L, int64_t ldl,
                 const double* d_mu, int64_t n, int64_t m, uint64_t seed, uint32_t iter, int* d_k_out)
{
    GP_ARG(h && d_f && d_y && d_L && d_mu && n >= 0 && m >= 0 && ldl >= n);
    // workspace: Z (n x m) | NU (n x m) | err, bad y
    const size_t nm = (size_t)n * (size_t)m;
    GP_TRY(ensure_work(h, (2 * nm + 8) * sizeof(double)));
    double* Z = h->d_work;
    double* NU = Z + nm;
    int* err = reinterpret_cast<int*>(NU + nm);
    GP_HIP(hipMemsetAsync(err, 0, 2 * sizeof(int), h->stream));
    // the slice kernels take y as +1, -1 or NaN (a missing response; rng_ess.hip folds y into f, nu and mu for n <= 16384):
    // anything else is refused before f is touched
    GP_TRY(launch_check_y(h->stream, d_y, (int64_t)nm, err + 1));
    GP_HIP(hipMemcpyAsync(h->h_info, err + 1, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));
    if (*h->h_info != 0) { set_error("draw_f: y must be +1, -1 or NaN (a missing response)"); return GPIRT_E_ARG; }
    GP_TRY(launch_item_uniforms(h->stream, seed, iter, GPIRT_ST_F_Z, 0, m, n, Z, true, h->cfg.zfill_compact == 1));
    GP_TRY(launch_gemm(h, h->stream, false, false, TRI_A_LOWER, n, m, n, 1.0, d_L, ldl, Z, n, 0.0, NU, n));
    EssArgs a{};
    a.f = d_f; a.nu = NU; a.y = d_y; a.mu = d_mu; a.n = n; a.m = m; a.k_out = d_k_out; a.err = err;
    a.seed = seed; a.iter = iter; a.item0 = 0; a.U = nullptr; a.pos = nullptr; a.cap = 0;
    a.ll_exact = h->cfg.ll_exact; a.screen = h->cfg.ess_screen == 1;
    GP_TRY(launch_ess(h->stream, a));
    GP_HIP(hipMemcpyAsync(h->h_info, err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));
    if (*h->h_info != 0) { set_error("draw_f: elliptical slice sampler did not terminate"); return GPIRT_E_NUMERIC; }
    return 0;
}

// gpirt_draw_f with mu = b0 + theta b1 given by its parts: y is packed and the slice kernel forms mu itself (ess_lin.hip).
// Same Z, same product, same draws as gpirt_draw_f on mu[i + j n] = beta[2 j] + theta[i] * beta[2 j + 1], bit for bit.
int gpirt_draw_f_linear(gpirt_handle_t h, double* d_f, const double* d_y, const double* d_L, int64_t ldl,
                        const double* d_theta, const double* d_beta, int64_t n, int64_t m, uint64_t seed, uint32_t iter,
                        int* d_k_out)
{
    GP_ARG(h && d_f && d_y && d_L && d_theta && d_beta && m >= 0 && ldl >= n);
    if (!ess_pack_eligible(n)) { set_error("draw_f_linear: n = %lld, the packed slice kernel takes 2048 < n <= 8192", (long long)n); return GPIRT_E_ARG; }
    // workspace: Z (n x m) | NU (n x m) | err, bad y | the packed y (512 m words)
    const size_t nm = (size_t)n * (size_t)m;
    GP_TRY(ensure_work(h, (2 * nm + 8) * sizeof(double) + 512 * (size_t)m * sizeof(uint32_t)));
    double* Z = h->d_work;
    double* NU = Z + nm;
    int* err = reinterpret_cast<int*>(NU + nm);
    uint32_t* ypk = reinterpret_cast<uint32_t*>(NU + nm + 8);
    GP_HIP(hipMemsetAsync(err, 0, 2 * sizeof(int), h->stream));
    GP_TRY(launch_check_y(h->stream, d_y, (int64_t)nm, err + 1));
    GP_HIP(hipMemcpyAsync(h->h_info, err + 1, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));
    if (*h->h_info != 0) { set_error("draw_f_linear: y must be +1, -1 or NaN (a missing response)"); return GPIRT_E_ARG; }
    GP_TRY(launch_ess_pack(h->stream, d_y, n, m, ypk));
    GP_TRY(launch_item_uniforms(h->stream, seed, iter, GPIRT_ST_F_Z, 0, m, n, Z, true, h->cfg.zfill_compact == 1));
    GP_TRY(launch_gemm(h, h->stream, false, false, TRI_A_LOWER, n, m, n, 1.0, d_L, ldl, Z, n, 0.0, NU, n));
    EssArgs a{};
    a.f = d_f; a.nu = NU; a.n = n; a.m = m; a.k_out = d_k_out; a.err = err;
    a.seed = seed; a.iter = iter; a.item0 = 0;
    a.ll_exact = h->cfg.ll_exact; a.screen = h->cfg.ess_screen == 1;
    a.ypk = ypk; a.theta = d_theta; a.beta = d_beta;
    a.grid = h->cfg.ess_pack == 3 ? 2 * h->n_cu : 0;
    GP_TRY(launch_ess(h->stream, a));
    GP_HIP(hipMemcpyAsync(h->h_info, err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));
    if (*h->h_info != 0) { set_error("draw_f_linear: elliptical slice sampler did not terminate"); return GPIRT_E_NUMERIC; }
    return 0;
}

int gpirt_draw_fstar(gpirt_handle_t h, const double* d_f, const double* d_theta, const double* d_L,
                     int64_t ldl, const double* d_mu_star, int64_t n, int64_t m, uint64_t seed,
                     uint32_t iter, int fused, double* d_out, double* d_s_out, double* d_mean_out)
{
    GP_ARG(h && d_f && d_theta && d_L && d_mu_star && d_out && n >= 0 && m >= 0 && ldl >= n);
    const int64_t N = GPIRT_NGRID;
    // workspace: tstar (N) | kstar (n x N) | rhs (n x (N+m)) | mean (N x m) | s (N)
    const size_t need = (size_t)N + (size_t)n * N + (size_t)n * (N + m) + (size_t)N * m + (size_t)N + 16;
    GP_TRY(ensure_work(h, need * sizeof(double)));
    double* tstar = h->d_work;
    double* kstar = tstar + ((N + 1) & ~1);
    double* rhs = kstar + (size_t)n * N + ((size_t)n * N & 1);
    double* mean = rhs + (size_t)n * (N + m) + (((size_t)n * (N + m)) & 1);
    double* s = mean + (size_t)N * m;
    double ts[GPIRT_NGRID];
    for (int i = 0; i < GPIRT_NGRID; ++i) ts[i] = -5.0 + (double)i * 0.01;
    GP_HIP(hipMemcpyAsync(tstar, ts, sizeof(ts), hipMemcpyHostToDevice, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));   // ts is a stack buffer
    GP_TRY(launch_se_kernel(h->stream, h->kern, d_theta, n, tstar, N, kstar, n, 0.0));              // :17
    GP_HIP(hipMemcpyAsync(rhs, kstar, sizeof(double) * (size_t)n * N, hipMemcpyDeviceToDevice, h->stream));
    GP_HIP(hipMemcpyAsync(rhs + (size_t)n * N, d_f, sizeof(double) * (size_t)n * m, hipMemcpyDeviceToDevice, h->stream));
    GP_TRY(launch_trsm_lower(h, h->stream, d_L, n, ldl, rhs, N + m, n, false));             // :19 and :7 inner
    GP_TRY(launch_colnorm_s(h->stream, rhs, n, N, n, s));                                   // :20
    double* W = rhs + (size_t)n * N;
    if (fused) {
        GP_TRY(launch_gemm(h, h->stream, true, false, TRI_NONE, N, m, n, 1.0, rhs, n, W, n, 0.0, mean, N));
    } else {
        GP_TRY(launch_trsm_lower(h, h->stream, d_L, n, ldl, W, m, n, true));                // :7 outer
        GP_TRY(launch_gemm(h, h->stream, true, false, TRI_NONE, N, m, n, 1.0, kstar, n, W, n, 0.0, mean, N)); // :25
    }
    FstarEpiArgs a{};
    a.mean = mean; a.mu_star = d_mu_star; a.s = s; a.out = d_out; a.N = N; a.m = m;
    a.seed = seed; a.iter = iter; a.item0 = 0; a.U = nullptr; a.mean_out = d_mean_out;
    GP_TRY(launch_fstar_epilogue(h->stream, a));
    if (d_s_out) GP_HIP(hipMemcpyAsync(d_s_out, s, sizeof(double) * N, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// the log-posterior (N x n, without the prior) of draw_theta in the handle's workspace: src/draw-theta.cpp:15-19
static int theta_logpost(gpirt_handle_t h, const double* d_y, const double* d_fstar, int64_t n, int64_t m, double** lp_out,
                         const int** overflow_out, long long** trace_out = nullptr)
{
    const int64_t N = GPIRT_NGRID;
    // workspace: Ypm (n x 2m) | Gpm (N x 2m, padded) | logpost (N x n) | byte indicators, digit planes, scales (theta_fixed.hip)
    const int64_t Np = (N + 127) / 128 * 128;     // rows of Gpm incl. padding to whole 128-row tiles
    const TfDims tfd = tf_dims(n, m, N);
    const size_t lp_doubles = ((size_t)N * n + 17) / 2 * 2;
    const size_t fixed_doubles = tf_y8_bytes(tfd) / 8 + tf_gq_bytes(tfd) / 8 + tf_aux_bytes(tfd) / 8 + 8;
    const size_t need = (size_t)n * 2 * m + (size_t)Np * 2 * m + lp_doubles + fixed_doubles;
    GP_TRY(ensure_work(h, need * sizeof(double)));
    double* Ypm = h->d_work;
    double* Gpm = Ypm + (size_t)n * 2 * m;
    double* lp = Gpm + (size_t)Np * 2 * m;
    double* y8 = lp + lp_doubles;                  // (an even number of doubles from the base: 16-byte aligned)
    double* gq = y8 + tf_y8_bytes(tfd) / 8;
    double* aux = gq + tf_gq_bytes(tfd) / 8;
    GP_HIP(hipMemsetAsync(Gpm, 0, sizeof(double) * (size_t)Np * 2 * m, h->stream));
    GP_TRY(launch_indicators(h->stream, d_y, n, m, Ypm));
    const int* only_if = nullptr;                  // (the product: sampler.hip do_theta_partial)
    if (h->cfg.theta_fixed == 1) {
        GP_TRY(launch_tf_indicators(h->stream, d_y, n, n, m, tfd, y8));
        GP_TRY(launch_theta_fixed(h->stream, d_fstar, N, n, m, tfd, y8, gq, aux, lp, N, trace_out != nullptr));
        only_if = tf_overflow(aux, tfd);
        if (trace_out) *trace_out = tf_trace(aux, tfd);
    }
    GP_TRY(launch_loglik_terms(h->stream, d_fstar, N, m, Gpm, Np, only_if));
    GP_TRY(launch_gemm(h, h->stream, false, true, TRI_NONE, N, n, 2 * m, 1.0, Gpm, Np, Ypm, n, 0.0, lp, N, Np, only_if));
    GP_TRY(launch_theta_nan_fix(h->stream, Gpm, Np, Ypm, n, m, lp, N, N, only_if));
    *lp_out = lp;
    if (overflow_out) *overflow_out = only_if;
    return 0;
}

int gpirt_draw_theta(gpirt_handle_t h, const double* d_y, const double* d_fstar, int64_t n,
                     int64_t m, uint64_t seed, uint32_t iter, int stabilise, double* d_theta_out,
                     int* d_degenerate)
{
    GP_ARG(h && d_y && d_fstar && d_theta_out && n >= 0 && m >= 0);
    double* lp = nullptr;
    GP_TRY(theta_logpost(h, d_y, d_fstar, n, m, &lp, nullptr));
    if (d_degenerate) GP_HIP(hipMemsetAsync(d_degenerate, 0, sizeof(int), h->stream));
    ThetaArgs a{};
    a.logpost = lp; a.N = GPIRT_NGRID; a.n = n; a.stabilise = stabilise; a.seed = seed; a.iter = iter;
    a.U = nullptr; a.theta_out = d_theta_out; a.degenerate = d_degenerate; a.err = nullptr;
    return launch_theta_sample(h->stream, a);
}

int gpirt_debug_theta_logpost(gpirt_handle_t h, const double* d_y, const double* d_fstar, int64_t n, int64_t m,
                              double* d_logpost_out, int* fell_back)
{
    GP_ARG(h && d_y && d_fstar && d_logpost_out && n >= 0 && m >= 0);
    double* lp = nullptr;
    const int* ovf = nullptr;
    GP_TRY(theta_logpost(h, d_y, d_fstar, n, m, &lp, &ovf));
    GP_HIP(hipMemcpyAsync(d_logpost_out, lp, sizeof(double) * (size_t)GPIRT_NGRID * n, hipMemcpyDeviceToDevice, h->stream));
    int flag = 0;
    if (ovf) GP_HIP(hipMemcpyAsync(&flag, ovf, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));
    if (fell_back) *fell_back = flag;
    return 0;
}

int gpirt_debug_theta_clock(gpirt_handle_t h, const double* d_y, const double* d_fstar, int64_t n, int64_t m,
                            long long* host_stamps, int64_t count)
{
    GP_ARG(h && d_y && d_fstar && host_stamps && n >= 0 && m >= 0 && count >= 0);
    if (h->cfg.theta_fixed != 1) { set_error("the stamps are those of the fixed-point product"); return GPIRT_E_ARG; }
    double* lp = nullptr;
    long long* tr = nullptr;
    GP_TRY(theta_logpost(h, d_y, d_fstar, n, m, &lp, nullptr, &tr));
    const int64_t have = (int64_t)tf_trace_wgs() * 6;
    GP_HIP(hipMemcpyAsync(host_stamps, tr, sizeof(long long) * (size_t)(count < have ? count : have), hipMemcpyDeviceToHost, h->stream));
    GP_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

// draw_beta for callers outside a sampler.  Nobody has checked this y: the register kernel (GPIRT_BETA_SCREEN=1) folds it into
// two bit masks and is only taken when every entry is +1, -1 or NaN; anything else goes to draw_beta_kernel, which multiplies.
static int draw_beta_op(gpirt_handle_t h, double* d_beta, const double* d_theta, const double* d_y,
                        const double* d_f, const double* d_pm, const double* d_ps, const double* d_step,
                        int64_t n, int64_t m, uint64_t seed, uint32_t iter, int* d_path)
{
    GP_ARG(h && d_beta && d_theta && d_y && d_f && d_pm && d_ps && d_step && n >= 0 && m >= 0);
    BetaArgs a{};
    a.beta = d_beta; a.theta = d_theta; a.y = d_y; a.f = d_f; a.pm = d_pm; a.ps = d_ps; a.step = d_step;
    a.n = n; a.m = m; a.N = GPIRT_NGRID; a.mu = nullptr; a.mu_star = nullptr;
    a.seed = seed; a.iter = iter; a.item0 = 0; a.U = nullptr; a.path = d_path;
    if (h->cfg.beta_screen == 1 && n <= 8192 && n * m > 0) {
        GP_TRY(ensure_work(h, 8 * sizeof(double)));
        int* bad = reinterpret_cast<int*>(h->d_work);
        GP_HIP(hipMemsetAsync(bad, 0, sizeof(int), h->stream));
        GP_TRY(launch_check_y(h->stream, d_y, n * m, bad));
        GP_HIP(hipMemcpyAsync(h->h_info, bad, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        GP_HIP(hipStreamSynchronize(h->stream));
        a.screen = *h->h_info == 0;
    }
    return launch_draw_beta(h->stream, a);
}

int gpirt_draw_beta(gpirt_handle_t h, double* d_beta, const double* d_theta, const double* d_y,
                    const double* d_f, const double* d_pm, const double* d_ps, const double* d_step,
                    int64_t n, int64_t m, uint64_t seed, uint32_t iter)
{
    return draw_beta_op(h, d_beta, d_theta, d_y, d_f, d_pm, d_ps, d_step, n, m, seed, iter, nullptr);
}

int gpirt_draw_beta_paths(gpirt_handle_t h, double* d_beta, const double* d_theta, const double* d_y,
                          const double* d_f, const double* d_pm, const double* d_ps, const double* d_step,
                          int64_t n, int64_t m, uint64_t seed, uint32_t iter, int* d_path)
{
    GP_ARG(d_path != nullptr);
    return draw_beta_op(h, d_beta, d_theta, d_y, d_f, d_pm, d_ps, d_step, n, m, seed, iter, d_path);
}

int gpirt_prof_enable(gpirt_handle_t h, int on)
{
    GP_ARG(h != nullptr);
    h->prof.enabled = on != 0;
    return 0;
}

static int prof_resolve(gpirt_handle_t h)
{
    if (h->prof.pending.empty()) return 0;
    GP_HIP(hipStreamSynchronize(h->stream));
    if (h->side) GP_HIP(hipStreamSynchronize(h->side));
    // class 4 (the replay's pass over L): the spare passes a draw enqueues find every item done and leave at once (a few
    // microseconds) -- they are not passes over L and stay out of the average.  The yardstick is the upper quartile of the
    // durations, not the longest: one pass that was held up (0.5 ms beside 17 us ones at n = 4096) would otherwise throw
    // every real pass out
    float longest4 = 0.f;
    {
        std::vector<float> d4;
        for (auto& pp : h->prof.pending)
            if (pp.cls == 4) { float ms = 0.f; GP_HIP(hipEventElapsedTime(&ms, pp.e0, pp.e1)); d4.push_back(ms); }
        if (!d4.empty()) { std::sort(d4.begin(), d4.end()); longest4 = d4[(d4.size() * 3) / 4]; }
    }
    for (auto& pp : h->prof.pending) {
        float ms = 0.f;
        GP_HIP(hipEventElapsedTime(&ms, pp.e0, pp.e1));
        if (pp.cls == 4 && ms < 0.25f * longest4) { h->prof.free_pairs.push_back(pp); continue; }
        h->prof.ms[pp.cls] += ms;
        h->prof.launches[pp.cls] += 1;
        h->prof.flops[pp.cls] += pp.flops;
        h->prof.bytes[pp.cls] += pp.bytes;
        h->prof.free_pairs.push_back(pp);
    }
    h->prof.pending.clear();
    return 0;
}

int gpirt_prof_syrk(gpirt_handle_t h, int cls, int reset, double* total_ms, int64_t* launches, double* flops)
{
    GP_ARG(h != nullptr && cls >= 0 && cls < PROF_CLASSES);
    GP_TRY(prof_resolve(h));
    if (total_ms) *total_ms = h->prof.ms[cls];
    if (launches) *launches = h->prof.launches[cls];
    if (flops) *flops = h->prof.flops[cls];
    if (reset) { h->prof.ms[cls] = 0.0; h->prof.launches[cls] = 0; h->prof.flops[cls] = 0.0; h->prof.bytes[cls] = 0.0; }
    return 0;
}

int gpirt_prof_syrk_bytes(gpirt_handle_t h, int cls, double* bytes)
{
    GP_ARG(h != nullptr && bytes != nullptr && cls >= 0 && cls < PROF_CLASSES);
    GP_TRY(prof_resolve(h));
    *bytes = h->prof.bytes[cls];
    return 0;
}

int gpirt_prof_trailing(gpirt_handle_t h, int reset, double* total_ms, int64_t* launches, double* flops)
{
    return gpirt_prof_syrk(h, 0, reset, total_ms, launches, flops);
}

// ---------------------------------------------------------------- R stream (host) ----------
int gpirt_rstream_create(gpirt_rstream_t* out, uint32_t seed)
{
    GP_ARG(out != nullptr);
    gpirt_rstream_s* r = new (std::nothrow) gpirt_rstream_s();
    if (!r) { set_error("out of host memory"); return GPIRT_E_ALLOC; }
    // set.seed(): Randomize() -- 50 LCG scrambles, then 625 LCG words; dummy[0] (mti) forced to 624
    for (int j = 0; j < 50; ++j) seed = 69069u * seed + 1u;
    uint32_t dummy[625];
    for (int j = 0; j < 625; ++j) { seed = 69069u * seed + 1u; dummy[j] = seed; }
    memcpy(r->r.mt, dummy + 1, sizeof(r->r.mt));
    r->r.mti = 624;
    *out = r;
    return 0;
}

int gpirt_rstream_from_state(gpirt_rstream_t* out, const uint32_t mt[624], int mti)
{
    GP_ARG(out != nullptr && mt != nullptr && mti >= 0 && mti <= 624);
    gpirt_rstream_s* r = new (std::nothrow) gpirt_rstream_s();
    if (!r) { set_error("out of host memory"); return GPIRT_E_ALLOC; }
    memcpy(r->r.mt, mt, sizeof(r->r.mt));
    r->r.mti = mti;
    *out = r;
    return 0;
}

int gpirt_rstream_get_state(gpirt_rstream_t r, uint32_t mt[624], int* mti)
{
    GP_ARG(r && mt && mti);
    rstream_sync(r);                 // a sampler replaying this stream runs ahead of the chain: back to the consumed position
    memcpy(mt, r->r.mt, sizeof(r->r.mt));
    *mti = r->r.mti;
    return 0;
}

int gpirt_rstream_destroy(gpirt_rstream_t r) { rstream_gone(r); delete r; return 0; }

int gpirt_rstream_unif(gpirt_rstream_t r, double* h_out, int64_t n)
{
    GP_ARG(r && (h_out || n == 0) && n >= 0);
    rstream_sync(r);
    for (int64_t i = 0; i < n; ++i) h_out[i] = r->r.unif();
    return 0;
}

int gpirt_rstream_norm(gpirt_rstream_t r, double* h_out, int64_t n)
{
    GP_ARG(r && (h_out || n == 0) && n >= 0);
    rstream_sync(r);
    for (int64_t i = 0; i < n; ++i) h_out[i] = r->r.norm();
    return 0;
}

void gpirt_default_options(gpirt_options* o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    // the reference's contract: R's own stream replayed draw for draw, draw_theta exactly as src/draw-theta.cpp words it
    o->rng_kind = GPIRT_RNG_RSTREAM;
    o->seed = 1;
    o->theta_stabilise = 0;
    o->fstar_fused = 0;
    o->device = -1;
    o->reserved0 = 0;
    o->item0 = 0;
    o->m_total = 0;
}

// the preset bench.py's headline is timed with (include/gpirt_hip.h)
void gpirt_fast_options(gpirt_options* o)
{
    if (!o) return;
    gpirt_default_options(o);
    o->rng_kind = GPIRT_RNG_ITEM;
    o->seed = 1;
    o->theta_stabilise = 1;
    o->fstar_fused = 1;
    o->kstar_rank = 64;
    o->factor_structured = 1;
}

}  // extern "C"
