"""ctypes binding of libgpirt_hip.so -- the C ABI declared in include/gpirt_hip.h.

The product path has NO CPU fallback: if the library is missing, or no gfx950 device is visible,
every compute entry raises.  (The CPU oracle under oracle/ is test infrastructure and is never
imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# GPIRT_HIP_LIBRARY: test hook -- another build of the same library (tests/test_gpu_fences.py loads the fenced variant)
LIB_PATH = os.environ.get("GPIRT_HIP_LIBRARY") or os.path.join(HERE, "libgpirt_hip.so")

NGRID = 1001
RNG_RSTREAM, RNG_ITEM = 0, 1
ST_INIT_F, ST_INIT_BETA, ST_F_Z, ST_F_ESS, ST_FSTAR, ST_THETA, ST_BETA = 1, 2, 3, 4, 5, 6, 7
ST_PPC = 8                        # the replicate of the posterior predictive checks (gpirt_amd.ppc)
ST_ELL = 9                        # the two uniforms of a length-scale update (gpirt_amd.ell): item index 0 whitened, 1 centred
ST_AMP = 10                       # the two uniforms per item of an amplitude update (gpirt_amd.amp): item index item0 + j
ST_CARRY = 11                     # the nugget of the consistent step's carry (gpirt_amd.consistent): item index item0 + j, index i

E_ARG, E_HIP, E_NODEVICE, E_ALLOC, E_RNG, E_INTERRUPT, E_NUMERIC = -1, -2, -3, -4, -5, -6, -7

# posterior summaries (include/gpirt_hip.h GPIRT_SUM_*): part bits, and the order of the totals
SUM_THETA_BETA, SUM_F, SUM_PRED, SUM_WAIC = 1, 2, 4, 8
SUM_PARTS = {"theta_beta": SUM_THETA_BETA, "f": SUM_F, "pred": SUM_PRED, "waic": SUM_WAIC}
SUM_DIAG = 16                     # split-R-hat / batch-means ESS accumulators (Sampler.summary_enable(..., planned_draws=S))
# quantiles (gpirt_amd.quantiles): theta histograms, IRF bands -- parts of a summary state, not of gpirt_summary.parts
SUM_THETA_HIST, SUM_IRF_BAND = 32, 128
SUM_PARTS.update(diag=SUM_DIAG, theta_hist=SUM_THETA_HIST, irf_band=SUM_IRF_BAND)     # "diag": with planned_draws only
SUM_POOLED = SUM_THETA_BETA | SUM_F | SUM_PRED | SUM_WAIC      # the parts gpirt_summary (a pooled or one chain's) can carry
IRF_BINS = 256
QNT_SCALARS = ("max_rhat", "n_rhat_high", "n_rhat_nan", "theta_off_grid", "irf_nan", "draws", "irf_count_min",
               "irf_count_max")
SUM_TOTALS = ("lppd", "p_waic", "elpd_waic", "waic", "se_elpd_waic", "n_obs", "draws", "elpd_mean", "elpd_ss")


def summary_parts(spec) -> int:
    """GPIRT_SUM_* bits from an int, one part name or an iterable of them ("theta_beta", "f", "pred", "waic")."""
    if isinstance(spec, (int, np.integer)) and not isinstance(spec, bool):
        return int(spec)
    if isinstance(spec, str):
        spec = (spec,)
    bits = 0
    for name in spec:
        if name not in SUM_PARTS:
            raise ValueError(f"unknown summary part {name!r} (one of {sorted(SUM_PARTS)})")
        bits |= SUM_PARTS[name]
    return bits


class GpirtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[gpirt {code}] {msg}")
        self.code = code


class Summary(C.Structure):
    """gpirt_summary (include/gpirt_hip.h): the parts wanted, a host pointer per output (NULL: not wanted), the totals."""
    _fields_ = [("parts", C.c_int), ("reserved", C.c_int)] + [
        (f"h_{k}", C.POINTER(C.c_double)) for k in ("p_yes", "lppd", "p_waic", "f_mean", "f_var", "theta_mean", "theta_var",
                                                     "beta_mean", "beta_var")] + [("totals", C.c_double * len(SUM_TOTALS))]


DIAG_BLOCKS = ("theta", "beta", "f")
DIAG_SCALARS = ("max_rhat", "min_ess", "n_rhat_high", "n_rhat_nan", "n_ess_nan")
CHAIN_SEED_GAMMA, CHAIN_SEED_M1, CHAIN_SEED_M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_M64 = 0xFFFFFFFFFFFFFFFF


def chain_seed(seed: int, c: int) -> int:
    """gpirt_chain_seed: chain 0 keeps `seed`; chain c >= 1 takes the splitmix64 finaliser of seed + c GAMMA."""
    seed = int(seed) & _M64
    if c <= 0:
        return seed
    z = (seed + c * CHAIN_SEED_GAMMA) & _M64
    z = ((z ^ (z >> 30)) * CHAIN_SEED_M1) & _M64
    z = ((z ^ (z >> 27)) * CHAIN_SEED_M2) & _M64
    return z ^ (z >> 31)


class Diag(C.Structure):
    """gpirt_diag (include/gpirt_hip.h): host pointers of R-hat / ESS / MCSE per block (NULL: not wanted), the reflection
    flags, the per-block scalars and reserved words."""
    _fields_ = [(f"h_{b}_{k}", C.POINTER(C.c_double)) for b in DIAG_BLOCKS for k in ("rhat", "ess", "mcse")] + [
        ("reflected", C.POINTER(C.c_int)), ("scalars", (C.c_double * len(DIAG_SCALARS)) * len(DIAG_BLOCKS)),
        ("reserved", C.c_int64 * 4)]


class Quantiles(C.Structure):
    """gpirt_quantiles (include/gpirt_hip.h): the probabilities, a host pointer per output (NULL: not wanted), the C
    reflection flags, the scalars and reserved words."""
    _fields_ = [("nprobs", C.c_int), ("reserved0", C.c_int), ("probs", C.POINTER(C.c_double))] + [
        (k, C.POINTER(C.c_double)) for k in ("theta_q", "theta_median", "theta_mode", "theta_hist", "theta_rhat_bulk",
                                             "theta_rhat_tail", "theta_rhat", "irf_q", "irf_p_mean")] + [
        ("reflected", C.POINTER(C.c_int)), ("scalars", C.c_double * len(QNT_SCALARS)), ("reserved", C.c_int64 * 4)]


# posterior predictive checks (include/gpirt_hip.h GPIRT_PPC_*): the fields of a unit, in order
PPC_FIELDS = ("n_obs", "obs_yes", "rep_yes_mean", "rep_yes_var", "yes_ge", "yes_gt", "dev_obs_mean", "dev_rep_mean", "dev_ge",
              "correct_mean", "nonfinite", "draws", "rep_yes_sum", "rep_yes_sumsq", "correct_sum")


class Ppc(C.Structure):
    """gpirt_ppc (include/gpirt_hip.h): a host pointer per field for the items (m) and the respondents (n) (NULL: not
    wanted), the whole matrix's fields and reserved words."""
    _fields_ = [("item", C.POINTER(C.c_double) * len(PPC_FIELDS)), ("respondent", C.POINTER(C.c_double) * len(PPC_FIELDS)),
                ("totals", C.c_double * len(PPC_FIELDS)), ("reserved", C.c_int64 * 4)]


# pairwise item checks (include/gpirt_hip.h GPIRT_PAIRS_*): the finished m x m fields in order, the six uint32 counters
PAIRS_FIELDS = ("n_co", "obs_n11", "obs_n10", "obs_n01", "obs_n00", "rep_n11_mean", "rep_n11_var", "rep_n10_mean",
                "rep_n01_mean", "rep_n00_mean", "agree_obs", "agree_rep_mean", "log_or_obs", "ppp_n11", "ppp_n11_mid",
                "ppp_agree", "ppp_agree_mid", "ppp_or", "ppp_or_mid")
PAIRS_SUMS = ("sum_n11", "sumsq_n11", "sum_n1")
PAIRS_COUNTS = ("n11_ge", "n11_gt", "agree_ge", "agree_gt", "or_ge", "or_gt")
PAIRS_MAX_TOP, PAIRS_MAX_N = 64, 65534


class PpcPairs(C.Structure):
    """gpirt_ppc_pairs (include/gpirt_hip.h): top, host pointers per output (NULL: not wanted) and the counters."""
    _fields_ = [("top", C.c_int), ("reserved0", C.c_int), ("field", C.POINTER(C.c_double) * len(PAIRS_FIELDS)),
                ("sum_n11", C.POINTER(C.c_uint64)), ("sumsq_n11", C.POINTER(C.c_uint64)), ("sum_n1", C.POINTER(C.c_uint64)),
                ("count", C.POINTER(C.c_uint32) * len(PAIRS_COUNTS)), ("extreme_pairs", C.POINTER(C.c_int64)),
                ("extreme_ppp_or_mid", C.POINTER(C.c_double)), ("extreme_log_or_obs", C.POINTER(C.c_double)),
                ("n", C.c_int64), ("m", C.c_int64), ("pair_draws", C.c_int64), ("pair_skipped", C.c_int64),
                ("reserved", C.c_int64 * 4)]


# theta-binned item fit (include/gpirt_hip.h GPIRT_BINS_*): the finished fields per (bin, item), per item and per bin, in
# order; the raw arrays of the state block with their dtypes and shapes ("c": B x m, "i": m, "b": B)
BINS_CELL_FIELDS = ("obs_rate", "rep_rate", "exp_rate", "z_mean", "ppp_cell", "ppp_cell_mid", "n_mean")
BINS_ITEM_FIELDS = ("ppp_chi2", "ppp_chi2_mid", "chi2_obs_mean", "chi2_rep_mean")
BINS_BIN_FIELDS = ("occupancy", "bin_lo", "bin_hi")
BINS_RAW = (("sum_n", "u8", "c"), ("sum_t", "u8", "c"), ("sum_r", "u8", "c"), ("sum_e", "f8", "c"), ("sum_z", "f8", "c"),
            ("cell_ge", "u4", "c"), ("cell_gt", "u4", "c"), ("cell_empty", "u4", "c"), ("chi_ge", "u4", "i"),
            ("chi_gt", "u4", "i"), ("chi_obs_sum", "f8", "i"), ("chi_rep_sum", "f8", "i"), ("occ_sum", "u8", "b"))
BINS_MAX_H, BINS_MAX_TOP, BINS_TAG = 15, 64, 0x534E4942


class PpcBins(C.Structure):
    """gpirt_ppc_bins (include/gpirt_hip.h): top, the cuts, host pointers per output (NULL: not wanted) and the counters."""
    _fields_ = [("top", C.c_int), ("h", C.c_int), ("cuts", C.c_int * (BINS_MAX_H + 1)),
                ("cell", C.POINTER(C.c_double) * len(BINS_CELL_FIELDS)), ("item", C.POINTER(C.c_double) * len(BINS_ITEM_FIELDS)),
                ("bin", C.POINTER(C.c_double) * len(BINS_BIN_FIELDS)),
                ("sum_n", C.POINTER(C.c_uint64)), ("sum_t", C.POINTER(C.c_uint64)), ("sum_r", C.POINTER(C.c_uint64)),
                ("sum_e", C.POINTER(C.c_double)), ("sum_z", C.POINTER(C.c_double)),
                ("cell_count", C.POINTER(C.c_uint32) * 3), ("chi_count", C.POINTER(C.c_uint32) * 2),
                ("chi_obs_sum", C.POINTER(C.c_double)), ("chi_rep_sum", C.POINTER(C.c_double)),
                ("occ_sum", C.POINTER(C.c_uint64)), ("worst_items", C.POINTER(C.c_int64)),
                ("worst_ppp_chi2_mid", C.POINTER(C.c_double)), ("worst_chi2_obs_mean", C.POINTER(C.c_double)),
                ("n", C.c_int64), ("m", C.c_int64), ("B", C.c_int64), ("bin_draws", C.c_int64), ("bin_skipped", C.c_int64),
                ("reserved", C.c_int64 * 4)]


# group-wise item fit (include/gpirt_hip.h GPIRT_DIF_*): the finished fields per (group, bin, item), per (group, item) and per
# (focal group, item; row 0 NaN), in order; the raw arrays of the state block with their dtypes and shapes ("c": G x B x m,
# "o": G x B, "g": G x m)
DIF_CELL_FIELDS = ("obs_rate", "rep_rate", "exp_rate")
DIF_GROUP_FIELDS = ("ppp_yes", "ppp_yes_mid", "ppp_chi2", "ppp_chi2_mid", "chi2_obs_mean", "chi2_rep_mean")
DIF_FOCAL_FIELDS = ("mh_log_or_obs_mean", "mh_log_or_rep_mean", "mh_delta_obs_mean", "ppp_mh", "ppp_mh_mid", "mh_undefined",
                    "std_obs_mean", "std_rep_mean", "std_undefined")
DIF_RAW = (("sum_n", "u8", "c"), ("sum_t", "u8", "c"), ("sum_r", "u8", "c"), ("sum_e", "f8", "c"), ("occ_sum", "u8", "o"),
           ("yes_ge", "u4", "g"), ("yes_gt", "u4", "g"), ("chi_ge", "u4", "g"), ("chi_gt", "u4", "g"), ("mh_ge", "u4", "g"),
           ("mh_gt", "u4", "g"), ("mh_undefined_count", "u4", "g"), ("std_undefined_count", "u4", "g"),
           ("chi_obs_sum", "f8", "g"), ("chi_rep_sum", "f8", "g"), ("mh_log_obs_sum", "f8", "g"), ("mh_log_rep_sum", "f8", "g"),
           ("std_obs_sum", "f8", "g"), ("std_rep_sum", "f8", "g"))
DIF_MAX_G, DIF_MAX_N, DIF_MAX_TOP, DIF_TAG, DIF_NSTATS = 4, 65534, 64, 0x31464944, 8


class PpcDif(C.Structure):
    """gpirt_ppc_dif (include/gpirt_hip.h): top, the groups, the cuts, host pointers per output (NULL: not wanted), counters."""
    _fields_ = [("top", C.c_int), ("G", C.c_int), ("h", C.c_int), ("cuts", C.c_int * (BINS_MAX_H + 1)), ("reserved0", C.c_int),
                ("groups", C.POINTER(C.c_int32)),
                ("cell", C.POINTER(C.c_double) * len(DIF_CELL_FIELDS)), ("occupancy", C.POINTER(C.c_double)),
                ("group", C.POINTER(C.c_double) * len(DIF_GROUP_FIELDS)), ("focal", C.POINTER(C.c_double) * len(DIF_FOCAL_FIELDS)),
                ("raw", C.c_void_p * len(DIF_RAW)), ("flagged_items", C.POINTER(C.c_int64)),
                ("flagged_groups", C.POINTER(C.c_int64)), ("flagged_ppp_mh_mid", C.POINTER(C.c_double)),
                ("n", C.c_int64), ("m", C.c_int64), ("B", C.c_int64), ("dif_draws", C.c_int64), ("dif_skipped", C.c_int64),
                ("group_size", C.c_int64 * DIF_MAX_G), ("reserved", C.c_int64 * 4)]


# score-based checks (include/gpirt_hip.h GPIRT_SCORES_*): the finished fields per score (m + 1), of the spread (3), per item and
# per (group, item), in order; the raw arrays of the state block with their dtypes and shapes ("h": m + 1, "s": 4 x m, "v": 2,
# "1": 1, "i": m, "c": K x m), the constants first
SCORES_HIST_FIELDS = ("score_hist_obs", "score_hist_rep_mean", "score_hist_rep_sd", "ppp_hist", "ppp_hist_mid", "ppp_cdf",
                      "ppp_cdf_mid")
SCORES_VAR_FIELDS = ("score_var_obs", "score_var_rep_mean", "ppp_var")
SCORES_ITEM_FIELDS = ("r_rep_mean", "r_rep_sd", "ppp_r", "ppp_r_mid", "r_undefined", "ppp_chi2", "ppp_chi2_mid", "chi2_obs_mean",
                      "chi2_rep_mean")
SCORES_CELL_FIELDS = ("obs_rate", "rep_rate", "exp_rate", "ppp_cell", "ppp_cell_mid")
SCORES_CONST = (("hist_obs", "i8", "h"), ("sums_obs", "i8", "s"), ("var_obs", "i8", "v"), ("r_obs", "f8", "i"), ("tNo", "u4", "c"),
                ("tT", "u4", "c"))
SCORES_RAW = SCORES_CONST + (
    ("hist_sum", "u8", "h"), ("hist_sumsq", "u8", "h"), ("hist_ge", "u4", "h"), ("hist_gt", "u4", "h"), ("cdf_ge", "u4", "h"),
    ("cdf_gt", "u4", "h"), ("var_ge", "u4", "1"), ("var_gt", "u4", "1"), ("var_rep_sum", "u8", "1"),
    ("r_ge", "u4", "i"), ("r_gt", "u4", "i"), ("r_undefined_count", "u4", "i"), ("r_rep_sum", "f8", "i"), ("r_rep_sumsq", "f8", "i"),
    ("cell_ge", "u4", "c"), ("cell_gt", "u4", "c"), ("cell_empty", "u4", "c"), ("sum_nr", "u8", "c"), ("sum_r", "u8", "c"),
    ("sum_eo", "f8", "c"), ("sum_er", "f8", "c"),
    ("chi_ge", "u4", "i"), ("chi_gt", "u4", "i"), ("chi_obs_sum", "f8", "i"), ("chi_rep_sum", "f8", "i"))
# the last counted draw's arrays of gpirt_sampler_ppc_scores_get
SCORES_LAST = (("xr", "i4", "n"), ("hist", "i8", "h"), ("sums", "i8", "s"), ("r", "f8", "i"), ("tNr", "u4", "c"), ("tR", "u4", "c"),
               ("tEo", "i8", "c"), ("tVo", "i8", "c"), ("tEr", "i8", "c"), ("tVr", "i8", "c"), ("chi", "f8", "x"))
SCORES_MAX_M, SCORES_MAX_N, SCORES_MAX_K, SCORES_MAX_TOP, SCORES_TAG = 4096, 65534, 16, 64, 0x31524353


class PpcScores(C.Structure):
    """gpirt_ppc_scores (include/gpirt_hip.h): top, the cuts, host pointers per output (NULL: not wanted), counters."""
    _fields_ = [("top", C.c_int), ("K", C.c_int), ("cuts", C.c_int * SCORES_MAX_K),
                ("hist", C.POINTER(C.c_double) * len(SCORES_HIST_FIELDS)), ("var", C.POINTER(C.c_double)),
                ("item", C.POINTER(C.c_double) * len(SCORES_ITEM_FIELDS)), ("cell", C.POINTER(C.c_double) * len(SCORES_CELL_FIELDS)),
                ("raw", C.c_void_p * len(SCORES_RAW)), ("group_lo", C.POINTER(C.c_int64)), ("group_hi", C.POINTER(C.c_int64)),
                ("worst_items", C.POINTER(C.c_int64)), ("worst_ppp_chi2_mid", C.POINTER(C.c_double)),
                ("n", C.c_int64), ("m", C.c_int64), ("score_draws", C.c_int64), ("score_skipped", C.c_int64),
                ("n_scored", C.c_int64), ("reserved", C.c_int64 * 4)]


# person fit (include/gpirt_hip.h GPIRT_PERSON_*): the finished fields per respondent (n) and per (group, respondent), in order;
# the raw arrays of the state block with their dtypes and shapes ("n": n, "c": K x n), the constants first
PERSON_RESP_FIELDS = ("guttman_obs", "guttman_norm_obs", "guttman_rep_mean", "guttman_norm_rep_mean", "ppp_guttman", "ppp_guttman_mid",
                      "guttman_undefined", "lz_obs_mean", "lz_rep_mean", "lz_rep_sd", "lz_undefined", "ppp_chi2", "ppp_chi2_mid",
                      "chi2_obs_mean", "chi2_rep_mean")
PERSON_CELL_FIELDS = ("obs_rate", "rep_rate", "exp_rate", "ppp_cell", "ppp_cell_mid")
PERSON_CONST = (("x_obs", "i8", "n"), ("g_obs", "i8", "n"), ("q_obs", "i8", "n"), ("tN", "u4", "c"), ("tT", "u4", "c"))
PERSON_RAW = PERSON_CONST + (
    ("g_ge", "u4", "n"), ("g_gt", "u4", "n"), ("g_undefined_count", "u4", "n"), ("g_rep_sum", "u8", "n"), ("gn_rep_sum", "f8", "n"),
    ("lz_undefined_count", "u4", "n"), ("lz_obs_sum", "f8", "n"), ("lz_rep_sum", "f8", "n"), ("lz_rep_sumsq", "f8", "n"),
    ("sum_r", "u8", "c"), ("sum_e", "f8", "c"), ("cell_ge", "u4", "c"), ("cell_gt", "u4", "c"),
    ("chi_ge", "u4", "n"), ("chi_gt", "u4", "n"), ("chi_obs_sum", "f8", "n"), ("chi_rep_sum", "f8", "n"))
# the last counted draw's arrays of gpirt_sampler_ppc_person_get ("3": 3 x n, "2": 2 x n)
PERSON_LAST = (("xr", "i8", "n"), ("gr", "i8", "n"), ("qr", "i8", "n"), ("tR", "u4", "c"), ("tE", "i8", "c"), ("tV", "i8", "c"),
               ("lz", "f8", "3"), ("chi", "f8", "2"))
PERSON_MAX_M, PERSON_MAX_N, PERSON_MAX_K, PERSON_MAX_TOP, PERSON_TAG = 4096, 65534, 16, 64, 0x31535250


class PpcPerson(C.Structure):
    """gpirt_ppc_person (include/gpirt_hip.h): top, the cuts, host pointers per output (NULL: not wanted), counters."""
    _fields_ = [("top", C.c_int), ("K", C.c_int), ("cuts", C.c_int * PERSON_MAX_K),
                ("resp", C.POINTER(C.c_double) * len(PERSON_RESP_FIELDS)), ("cell", C.POINTER(C.c_double) * len(PERSON_CELL_FIELDS)),
                ("raw", C.c_void_p * len(PERSON_RAW)), ("group_lo", C.POINTER(C.c_int64)), ("group_hi", C.POINTER(C.c_int64)),
                ("group_items", C.POINTER(C.c_int32)),
                ("worst_respondents", C.POINTER(C.c_int64)), ("worst_ppp_guttman_mid", C.POINTER(C.c_double)),
                ("n", C.c_int64), ("m", C.c_int64), ("person_draws", C.c_int64), ("person_skipped", C.c_int64),
                ("n_scored", C.c_int64), ("reserved", C.c_int64 * 4)]


# residual correlations (include/gpirt_hip.h GPIRT_RESID_*): the finished fields per pair (m x m), per item (m) and the scalars, in
# order; the raw arrays of the state block with their dtypes and shapes ("p": m x m, "i": m, "g": 16 words); the last counted
# draw's arrays of gpirt_sampler_ppc_resid_get ("c": n x m column-major, "d": 9 x n x m, "s": 8)
RESID_PAIR_FIELDS = ("n_co", "rc_obs_mean", "rc_rep_mean", "rc_rep_sd", "ppp_rc", "ppp_rc_mid", "undefined")
RESID_ITEM_FIELDS = ("infit_obs_mean", "infit_rep_mean", "infit_rep_sd", "ppp_infit", "ppp_infit_mid", "ss_obs_mean", "ss_rep_mean",
                     "ppp_ss", "ppp_ss_mid")
RESID_SCALARS = ("frob_obs_mean", "frob_rep_mean", "frob_rep_sd", "ppp_frob", "ppp_frob_mid", "max_obs_mean", "max_rep_mean", "ppp_max",
                 "ppp_max_mid", "absmax_obs_mean", "absmax_rep_mean", "ppp_absmax", "ppp_absmax_mid")
RESID_RAW = (("n_co_int", "i8", "p"), ("undefined_count", "u4", "p"), ("rc_ge", "u4", "p"), ("rc_gt", "u4", "p"),
             ("rc_obs_sum", "f8", "p"), ("rc_rep_sum", "f8", "p"), ("rc_rep_sumsq", "f8", "p"),
             ("ss_undefined", "u4", "i"), ("ss_ge", "u4", "i"), ("ss_gt", "u4", "i"), ("ss_obs_sum", "f8", "i"), ("ss_rep_sum", "f8", "i"),
             ("global", "u8", "g"))
RESID_LAST = (("d_obs", "i4", "c"), ("d_rep", "i4", "c"), ("w", "i4", "c"), ("digits", "i1", "d"), ("s_obs", "i8", "p"), ("s_rep", "i8", "p"),
              ("v", "i8", "p"), ("r_obs", "f8", "p"), ("r_rep", "f8", "p"), ("stats", "f8", "s"))
RESID_MAX_M, RESID_MAX_N, RESID_MAX_TOP, RESID_TAG = 4096, 65534, 64, 0x31445352


class PpcResid(C.Structure):
    """gpirt_ppc_resid (include/gpirt_hip.h): top, host pointers per output (NULL: not wanted), the scalars and the counters."""
    _fields_ = [("top", C.c_int), ("reserved0", C.c_int), ("pair", C.POINTER(C.c_double) * len(RESID_PAIR_FIELDS)),
                ("item", C.POINTER(C.c_double) * len(RESID_ITEM_FIELDS)), ("raw", C.c_void_p * len(RESID_RAW)),
                ("worst_pairs", C.POINTER(C.c_int64)), ("worst_ppp_rc_mid", C.POINTER(C.c_double)),
                ("worst_rc_obs_mean", C.POINTER(C.c_double)), ("worst_items", C.POINTER(C.c_int64)),
                ("worst_ppp_ss_mid", C.POINTER(C.c_double)), ("scalar", C.c_double * len(RESID_SCALARS)),
                ("n", C.c_int64), ("m", C.c_int64), ("resid_draws", C.c_int64), ("resid_skipped", C.c_int64),
                ("global_undefined", C.c_int64), ("reserved", C.c_int64 * 4)]


# rank posteriors (include/gpirt_hip.h gpirt_ranks)
RANK_MAX_PIVOTS, RANK_MAX_PIVOTS_CLOSED, RANK_MAX_N = 16, 32, 16384


class Ranks(C.Structure):
    """gpirt_ranks (include/gpirt_hip.h): the probabilities, the pivots (in: as given; out: closed and sorted), host
    pointers per output (NULL: not wanted) and the counts."""
    _fields_ = [("probs", C.POINTER(C.c_double)), ("nprobs", C.c_int), ("n_pivots", C.c_int),
                ("pivots", C.c_int64 * RANK_MAX_PIVOTS_CLOSED), ("pairwise", C.c_int), ("reserved0", C.c_int),
                ("rank_mean", C.POINTER(C.c_double)), ("rank_var", C.POINTER(C.c_double)), ("rank_q", C.POINTER(C.c_double)),
                ("p_pivot", C.POINTER(C.c_double)), ("pivot_share", C.POINTER(C.c_double)),
                ("rank2_sum", C.POINTER(C.c_uint64)), ("rank2_sumsq", C.POINTER(C.c_uint64)),
                ("rank_hist", C.POINTER(C.c_uint32)), ("pivot_cover", C.POINTER(C.c_uint32)), ("lt", C.POINTER(C.c_uint32)),
                ("draws", C.c_int64), ("skipped", C.c_int64), ("B", C.c_int64), ("w", C.c_int64),
                ("rank_bin_width", C.c_double), ("reserved", C.c_int64 * 4)]


# scoring new respondents (include/gpirt_hip.h gpirt_score)
SCORE_MAX_N = 16384


class Score(C.Structure):
    """gpirt_score (include/gpirt_hip.h): the probabilities, host pointers per output (NULL: not wanted) and the totals."""
    _fields_ = [("probs", C.POINTER(C.c_double)), ("nprobs", C.c_int), ("reserved0", C.c_int),
                ("grid_post", C.POINTER(C.c_double)), ("theta_mean", C.POINTER(C.c_double)),
                ("theta_sd", C.POINTER(C.c_double)), ("theta_quantiles", C.POINTER(C.c_double)),
                ("theta_map", C.POINTER(C.c_double)), ("lpd", C.POINTER(C.c_double)), ("loglik_mean", C.POINTER(C.c_double)),
                ("post_sum", C.POINTER(C.c_double)), ("lpd_acc", C.POINTER(C.c_double)), ("ll_sum", C.POINTER(C.c_double)),
                ("n_obs", C.POINTER(C.c_int64)), ("draws", C.POINTER(C.c_int64)), ("nonfinite", C.POINTER(C.c_int64)),
                ("n_new", C.c_int64), ("m", C.c_int64), ("lpd_total", C.c_double), ("se_lpd_total", C.c_double),
                ("reserved", C.c_int64 * 4)]


# predicting the new respondents' unseen answers (include/gpirt_hip.h gpirt_score_predict)
PREDICT_MAX_TOP = 16


class ScorePredict(C.Structure):
    """gpirt_score_predict (include/gpirt_hip.h): top, host pointers per output (NULL: not wanted) and the counters."""
    _fields_ = [("top", C.c_int), ("reserved0", C.c_int), ("p_yes", C.POINTER(C.c_double)), ("info", C.POINTER(C.c_double)),
                ("next_items", C.POINTER(C.c_int64)), ("next_info", C.POINTER(C.c_double)),
                ("pred_sum", C.POINTER(C.c_double)), ("info_sum", C.POINTER(C.c_double)),
                ("n_new", C.c_int64), ("m", C.c_int64), ("pred_draws", C.c_int64), ("pred_skipped", C.c_int64),
                ("reserved", C.c_int64 * 4)]


# IRF shape posteriors (include/gpirt_hip.h GPIRT_SHAPE_*): the raw arrays of a state block in order, with their dtypes
SHAPE_MAX_TOLS, SHAPE_MAX_TOP, SHAPE_TAG = 4, 64, 0x50414853
SHAPE_RAW = (("cls", "u4"), ("peak_hist", "u4"), ("valley_hist", "u4"), ("cross_first_hist", "u4"), ("cross_last_hist", "u4"),
             ("cross_count", "u4"), ("draws", "u4"), ("nonfinite", "u4"), ("slope", "f8"), ("info_sum", "f8"), ("ti_sum", "f8"),
             ("ti_sumsq", "f8"), ("rel", "f8"))


class Shape(C.Structure):
    """gpirt_shape (include/gpirt_hip.h): the window and tolerances, a host pointer per raw array (NULL: not wanted) and
    the counters."""
    _fields_ = [("k_half", C.c_int), ("n_tols", C.c_int), ("tols", C.c_double * SHAPE_MAX_TOLS),
                ("raw", C.c_void_p * len(SHAPE_RAW)), ("n", C.c_int64), ("m", C.c_int64), ("info_draws", C.c_int64),
                ("info_skipped", C.c_int64), ("reserved", C.c_int64 * 4)]


# sum-score posteriors (include/gpirt_hip.h GPIRT_SUMSCORE_*): the raw arrays of a state block in order, with their dtypes
SUMSCORE_MAX_ITEMS, SUMSCORE_TAG = 4096, 0x43534D53
SUMSCORE_RAW = (("joint_sum", "f8"), ("pi_sum", "f8"), ("pi_sumsq", "f8"), ("tcc_sum", "f8"), ("tcc_sumsq", "f8"), ("var_sum", "f8"),
                ("rel", "f8"), ("mask", "u1"), ("w", "f8"), ("last", "f8"), ("last_pi", "f8"))


class Sumscore(C.Structure):
    """gpirt_sumscore (include/gpirt_hip.h): the form's mask (in), a host pointer per raw array (NULL: not wanted) and the
    counters."""
    _fields_ = [("items", C.c_void_p), ("raw", C.c_void_p * len(SUMSCORE_RAW)), ("m", C.c_int64), ("M", C.c_int64),
                ("draws", C.c_int64), ("skipped", C.c_int64), ("rel_draws", C.c_int64), ("rel_skipped", C.c_int64),
                ("reserved", C.c_int64 * 4)]


# two-form score equating (include/gpirt_hip.h GPIRT_EQUATE_*): the raw arrays of a state block in order, with their dtypes
EQUATE_MAX_ITEMS, EQUATE_TAG, EQUATE_MAX_CUTS = 2048, 0x45545145, 8
EQUATE_RAW = (("joint_sum", "f8"), ("pix_sum", "f8"), ("pix_sumsq", "f8"), ("piy_sum", "f8"), ("piy_sumsq", "f8"), ("eyx_sum", "f8"),
              ("eyx_sumsq", "f8"), ("exy_sum", "f8"), ("exy_sumsq", "f8"), ("corr", "f8"), ("corr_terms", "f8"), ("mask_x", "u1"),
              ("mask_y", "u1"), ("w", "f8"), ("last_joint", "f8"), ("last_pix", "f8"), ("last_piy", "f8"), ("last_eyx", "f8"),
              ("last_exy", "f8"))


class Equate(C.Structure):
    """gpirt_equate (include/gpirt_hip.h): the two forms' masks (in), a host pointer per raw array (NULL: not wanted) and the
    counters."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("raw", C.c_void_p * len(EQUATE_RAW)), ("m", C.c_int64), ("Mx", C.c_int64),
                ("My", C.c_int64), ("draws", C.c_int64), ("skipped", C.c_int64), ("corr_draws", C.c_int64),
                ("corr_skipped", C.c_int64), ("eq_clamped", C.c_int64), ("reserved", C.c_int64 * 4)]


# PSIS-LOO (include/gpirt_hip.h GPIRT_LOO_*): the raw arrays of a state block in order, the pointwise outputs and the totals
LOO_MAX_TAIL, LOO_MAX_TOP, LOO_TAG, LOO_KEY_MAX = 1024, 64, 0x4F4F4C50, 700.0
LOO_RAW = (("keys", "f8"), ("evicted_sum", "f8"), ("evicted_sumsq", "f8"), ("p_sum", "f8"), ("count", "i4"), ("nonfinite", "i4"),
           ("y", "i1"))
LOO_POINTWISE = ("pareto_k", "elpd_loo", "n_eff", "lppd", "p_loo", "loo_p_yes")
LOO_TOTALS = ("elpd_loo", "se_elpd_loo", "p_loo", "looic", "se_looic", "n_obs", "lppd", "k_threshold", "k_good", "k_bad",
              "k_very_bad", "unsmoothed", "cells_incomplete", "elpd_mean")


class Loo(C.Structure):
    """gpirt_loo (include/gpirt_hip.h): tail and top (in), a host pointer per array (NULL: not wanted), the totals and the
    counters."""
    _fields_ = [("tail", C.c_int64), ("top", C.c_int64), ("raw", C.c_void_p * len(LOO_RAW)),
                ("pointwise", C.c_void_p * len(LOO_POINTWISE)), ("item_elpd_loo", C.c_void_p),
                ("respondent_elpd_loo", C.c_void_p), ("worst_index", C.c_void_p), ("worst_k", C.c_void_p),
                ("totals", C.c_double * len(LOO_TOTALS)), ("n", C.c_int64), ("m", C.c_int64), ("T", C.c_int64), ("M", C.c_int64),
                ("draws", C.c_int64), ("chains", C.c_int64), ("reserved", C.c_int64 * 4)]


# Item-pair IRF order posteriors (include/gpirt_hip.h GPIRT_ORDER_*): the raw arrays of a state block in order, with their dtypes
ORDER_MAX_M, ORDER_MAX_TOP, ORDER_TAG = 4096, 64, 0x5244524F
ORDER_RAW = (("above", "u4"), ("cross", "u4"), ("easier", "u4"), ("depth_sum", "f8"), ("easiness", "f8"), ("set_counts", "u8"))


class ShapeOrder(C.Structure):
    """gpirt_shape_order (include/gpirt_hip.h): top (in), the window and tolerances, a host pointer per raw array (NULL: not
    wanted), the worst pairs and the counters."""
    _fields_ = [("top", C.c_int), ("k_half", C.c_int), ("n_tols", C.c_int), ("tols", C.c_double * SHAPE_MAX_TOLS),
                ("raw", C.c_void_p * len(ORDER_RAW)), ("worst_a", C.c_void_p), ("worst_b", C.c_void_p), ("n_worst", C.c_int64),
                ("n", C.c_int64), ("m", C.c_int64), ("draws", C.c_int64), ("skipped", C.c_int64), ("reserved", C.c_int64 * 4)]


# autocorrelation ESS (include/gpirt_hip.h GPIRT_ACF_*): the series' bits, the raw arrays of a state block in order, the outputs
ACF_THETA, ACF_BETA, ACF_LL = 1, 2, 4
ACF_PARTS = {"theta": ACF_THETA, "beta": ACF_BETA, "ll": ACF_LL}
ACF_MAX_LAG, ACF_DEFAULT_LAG, ACF_MAX_TOP, ACF_TAG = 1024, 256, 64, 0x31464341
ACF_RAW = ("s", "sum", "head", "tail", "centre", "nonfinite", "ring")
ACF_VALUES = ("ess", "tau", "mcse", "rhat", "rho1", "mean", "sd")
ACF_FLAGS = ("lag_used", "truncated", "nonfinite", "constant")
ACF_BLOCKS = ("theta", "beta", "item_ll", "resp_ll", "total_ll")
ACF_BLOCK_STATS = ("min_ess", "max_tau", "max_rhat")
ACF_BLOCK_COUNTS = ("n_truncated", "n_nan")


class Acf(C.Structure):
    """gpirt_acf (include/gpirt_hip.h): top (in), a host pointer per output (NULL: not wanted), the block folds, the counters."""
    _fields_ = [("top", C.c_int64), ("value", C.POINTER(C.c_double) * len(ACF_VALUES)),
                ("flag", C.POINTER(C.c_int64) * len(ACF_FLAGS)), ("acf", C.POINTER(C.c_double)),
                ("worst_block", C.POINTER(C.c_int64)), ("worst_index", C.POINTER(C.c_int64)), ("worst_ess", C.POINTER(C.c_double)),
                ("block_stat", C.c_double * (len(ACF_BLOCKS) * len(ACF_BLOCK_STATS))),
                ("block_count", C.c_int64 * (len(ACF_BLOCKS) * len(ACF_BLOCK_COUNTS))),
                ("n", C.c_int64), ("m", C.c_int64), ("parts", C.c_int64), ("S", C.c_int64), ("H", C.c_int64), ("L", C.c_int64),
                ("P", C.c_int64), ("chains", C.c_int64), ("reserved", C.c_int64 * 4)]


# group posteriors (include/gpirt_hip.h GPIRT_GROUPS_*): the arrays of a state block in order, each (name, dtype, shape key) --
# the shape keys are those of gpirt_amd.groups.raw_shape
GROUPS_MAX_G, GROUPS_MAX_N, GROUPS_MAX_M, GROUPS_MAX_TOP, GROUPS_MED_BINS, GROUPS_TAG = 8, 65534, 4096, 64, 2001, 0x31505247
GROUPS_RAW = (("dens_sum", "u8", "g1k"), ("dens_sq", "u8", "g1k"), ("medhist", "u4", "g1m"), ("order", "u4", "6p"),
              ("ov_sum", "u8", "p"), ("d_undefined", "u4", "p"), ("mean_sum", "f8", "g1"), ("mean_sq", "f8", "g1"),
              ("sd_sum", "f8", "g1"), ("sd_sq", "f8", "g1"), ("a_sum", "f8", "p"), ("a_sq", "f8", "p"), ("ovl_sum", "f8", "p"),
              ("ovl_sq", "f8", "p"), ("d_sum", "f8", "p"), ("d_sq", "f8", "p"), ("median_cover", "u4", "n"),
              ("median_share", "f8", "n"), ("split_count", "u4", "pm"), ("nsplit_sum", "u8", "p"), ("nsplit_sq", "u8", "p"),
              ("support_sum", "f8", "gm"), ("support_sq", "f8", "gm"), ("rice_sum", "f8", "gm"), ("rice_sq", "f8", "gm"),
              ("gap_sum", "f8", "pm"), ("gap_sq", "f8", "pm"), ("loy_sum", "f8", "n"), ("loy_sq", "f8", "n"),
              ("loy_undefined", "u4", "g"), ("obs_with_sum", "u8", "n"), ("obs_n_sum", "u8", "n"))
# the last counted draw's tables of gpirt_sampler_groups_get, and the constants
GROUPS_LAST = (("hist", "u4", "g1k"), ("c1", "i8", "g1"), ("c2", "i8", "g1"), ("med2", "i8", "g1"), ("w", "i8", "p"), ("ov", "i8", "p"),
               ("latent_stats", "f8", "stats"), ("e", "u8", "gm"), ("side", "i1", "gm"), ("split", "u1", "pm"), ("contested", "u1", "m"),
               ("n_split", "i8", "p"), ("c_g", "i8", "g"), ("loy", "u8", "n"), ("obs_with", "u4", "n"), ("obs_n", "u4", "n"),
               ("counts", "i8", "4"), ("group_size", "i8", "9"), ("groups", "i1", "n"))


class Groups(C.Structure):
    """gpirt_groups (include/gpirt_hip.h): top (in), a host pointer per pooled array and list (NULL: not wanted), the counters."""
    _fields_ = [("top", C.c_int64), ("raw", C.c_void_p * len(GROUPS_RAW)), ("most_split_items", C.POINTER(C.c_int64)),
                ("most_split_p", C.POINTER(C.c_double)), ("least_loyal", C.POINTER(C.c_int64)),
                ("least_loyal_loyalty", C.POINTER(C.c_double)), ("n", C.c_int64), ("m", C.c_int64), ("G", C.c_int64),
                ("pairs", C.c_int64), ("included", C.c_int64), ("chains", C.c_int64), ("latent_draws", C.c_int64),
                ("latent_skipped", C.c_int64), ("votes_draws", C.c_int64), ("votes_skipped", C.c_int64),
                ("group_size", C.c_int64 * (GROUPS_MAX_G + 1)), ("reserved", C.c_int64 * 4)]


class Run(C.Structure):
    """gpirt_run (include/gpirt_hip.h): what gpirt_mcmc_run computes beside gpirt_mcmc_chains's outputs -- R's stream (NULL: the
    item RNG) and one pointer per analysis (NULL: not wanted)."""
    _fields_ = [("rs", C.c_void_p), ("quantiles", C.POINTER(Quantiles)), ("ppc", C.POINTER(Ppc)), ("ranks", C.POINTER(Ranks)),
                ("h_y_new", C.POINTER(C.c_double)), ("n_new", C.c_int64), ("score", C.POINTER(Score)),
                ("predict", C.POINTER(ScorePredict)), ("pairs", C.POINTER(PpcPairs)), ("bins", C.POINTER(PpcBins)),
                ("shape", C.POINTER(Shape)), ("sumscore", C.POINTER(Sumscore)), ("dif", C.POINTER(PpcDif)),
                ("equate", C.POINTER(Equate)), ("loo", C.POINTER(Loo)), ("order", C.POINTER(ShapeOrder)),
                ("reserved", C.c_void_p * 8)]


class Options(C.Structure):
    _fields_ = [
        ("rng_kind", C.c_int),
        ("seed", C.c_uint64),
        ("theta_stabilise", C.c_int),
        ("fstar_fused", C.c_int),
        ("device", C.c_int),
        ("reserved0", C.c_int),
        ("item0", C.c_int64),
        ("m_total", C.c_int64),
        ("reserved1", C.c_int),
        ("kernel_fp32", C.c_int),
        ("kstar_rank", C.c_int),
        ("reserved", C.c_int * 4),
        ("factor_structured", C.c_int),
    ]


class Kernel(C.Structure):
    """gpirt_kernel: the covariance kernel of a handle (include/gpirt_hip.h, "the covariance kernel")"""
    _fields_ = [("family", C.c_int), ("reserved0", C.c_int), ("length_scale", C.c_double), ("reserved", C.c_int64 * 4)]


KERNEL_SE, KERNEL_MATERN52, KERNEL_MATERN32 = 0, 1, 2
KERNEL_FAMILIES = {"se": KERNEL_SE, "matern52": KERNEL_MATERN52, "matern32": KERNEL_MATERN32}
LENGTH_SCALE_MIN, LENGTH_SCALE_MAX = 0.01, 1000.0

# the length scale as a parameter of the chain (include/gpirt_hip.h gpirt_ell; gpirt_amd.ell)
ELL_MAX_POINTS = 1025
ELL_COUNTS = ("updates", "accepted", "out_of_range", "failed")
ELL_PARTS = ("copies", "solve", "factor", "product", "delta", "decide", "commit", "restore")     # "times" of ell_get, ms
ELL_LAST = {-1: None, 0: "rejected", 1: "accepted", 2: "out_of_range", 3: "failed"}
ELL_KINDS = ("whitened", "centred")       # the two updates; a kind's index is the item index of its uniforms
ELL_PARTS_CENTRED = ("copies", "solve", "factor", "solve_prop", "quad", "logdet", "decide", "restore")   # "times_centred", ms


class Ell(C.Structure):
    """gpirt_ell (include/gpirt_hip.h): the grid's size, the width, the index, the counters and the last update."""
    _fields_ = [(k, C.c_int64) for k in ("points", "width", "index") + ELL_COUNTS + ("last", "last_proposed", "factorisations")] + [
        (k, C.c_double) for k in ("length_scale", "lo", "hi", "last_u0", "last_u1")] + [("reserved", C.c_int64 * 4)]


class EllCentred(C.Structure):
    """gpirt_ell_centred (include/gpirt_hip.h): the centred update's width, counters and last update."""
    _fields_ = [(k, C.c_int64) for k in ("width",) + ELL_COUNTS + ("last", "last_proposed", "factorisations")] + [
        (k, C.c_double) for k in ("last_u0", "last_u1")] + [("reserved", C.c_int64 * 6)]


# per-item GP amplitudes (include/gpirt_hip.h gpirt_amp; gpirt_amd.amp)
AMP_MAX_POINTS = 1025
AMP_MIN, AMP_MAX = 0.01, 1000.0
AMP_COUNTS = ("updates", "accepted", "out_of_range", "failed")             # the rows of amp_get("counts")
AMP_RECORD = ("dll", "log_ratio", "log_u", "status", "nonfinite")          # the rows of amp_get("record")
AMP_STATUS = ("rejected", "accepted", "out_of_range", "failed")            # a record's status by its code
AMP_MODES = (None, "fixed", "sampled")
# the centred amplitude update (include/gpirt_hip.h gpirt_amp_centred; gpirt_amd.amp.centred_*)
ST_AMP_CENTRED = 13               # item index item0 + j: index 0 .. 63 the augmentation's normals, 64 / 65 the two uniforms
AMP_CENTRED_RANK = 64
AMP_CENTRED_COUNTS = ("updates", "accepted", "same", "failed")             # the rows of amp_get("counts_centred")
AMP_CENTRED_RECORD = ("Q", "k_prop", "dll", "log_u", "status")             # the rows of amp_get("record_centred")
AMP_CENTRED_STATUS = ("rejected", "accepted", "same", "failed")            # a record's status by its code


class AmpCentred(C.Structure):
    """gpirt_amp_centred (include/gpirt_hip.h): the calls, the rank, the totals over the items and the acceptance of the decided."""
    _fields_ = [(k, C.c_int64) for k in ("calls", "rank") + AMP_CENTRED_COUNTS] + [
        (k, C.c_double) for k in ("accept_rate", "last_ms")] + [("reserved", C.c_int64 * 6)]


# the centred beta update (include/gpirt_hip.h gpirt_beta_centred; gpirt_amd.beta)
ST_BETA_CENTRED = 14              # item index item0 + j: index 0 / 1 the two normals
BETA_CENTRED_RANK = 64
BETA_CENTRED_COUNTS = ("updates", "failed")                                # the rows of beta_centred_get("counts")
BETA_CENTRED_STATUS = {0: "updated", 3: "failed"}                          # a record's status by its code


class BetaCentred(C.Structure):
    """gpirt_beta_centred (include/gpirt_hip.h): the calls, the rank and the totals over the items."""
    _fields_ = [(k, C.c_int64) for k in ("calls", "rank") + BETA_CENTRED_COUNTS] + [("last_ms", C.c_double), ("reserved", C.c_int64 * 6)]


# the collapsed scale and shift move (include/gpirt_hip.h gpirt_scale; gpirt_amd.scale)
ST_SCALE = 15                      # item index the kind (0 scale, 1 shift): index 0 the normal's uniform, 1 the decision's
SCALE_KINDS = ("scale", "shift")
SCALE_RECORD = ("kind", "z", "step", "c", "D", "Q", "J", "log_r", "u", "log_u", "status", "bad", "t", "width", "_14", "_15")
SCALE_STATUS = {0: "rejected", 1: "accepted", 2: "failed"}
SCALE_COUNTS = ("calls", "accepted", "failed")                              # the rows of scale_get("counts"), a column per kind
SCALE_TIMES = ("whole", "curve", "product", "logz", "decide", "commits")


class Scale(C.Structure):
    """gpirt_scale (include/gpirt_hip.h): per kind the calls, the accepted and failed ones, the width and the last call's time."""
    _fields_ = [("on", C.c_int64), ("calls", C.c_int64 * 2), ("accepted", C.c_int64 * 2), ("failed", C.c_int64 * 2),
                ("width", C.c_double * 2), ("last_ms", C.c_double * 2), ("reserved", C.c_int64 * 5)]


class Amp(C.Structure):
    """gpirt_amp (include/gpirt_hip.h): the mode, the grid's size, the totals over the items and the pooled acceptance."""
    _fields_ = [(k, C.c_int64) for k in ("on", "points", "m", "calls") + AMP_COUNTS + ("planned_draws", "recorded")] + [
        (k, C.c_double) for k in ("accept_rate", "lo", "hi", "min_amplitude", "max_amplitude")] + [("reserved", C.c_int64 * 4)]


# the consistent step's carry (include/gpirt_hip.h gpirt_carry; gpirt_amd.consistent)
CARRY_COUNTS = ("calls", "off_grid", "nonfinite", "total_off_grid", "total_nonfinite")


class Carry(C.Structure):
    """gpirt_carry (include/gpirt_hip.h): the carries so far, the last call's two counters, their sums, the last call's time."""
    _fields_ = [(k, C.c_int64) for k in CARRY_COUNTS] + [("last_ms", C.c_double), ("reserved", C.c_int64 * 4)]


# the population prior for theta (include/gpirt_hip.h gpirt_pop; gpirt_amd.pop)
ST_POP = 12                       # the two uniforms per group of a population-prior update: item index g, index 0 (mu) / 1 (sd)
POP_MAX_GROUPS, POP_MAX_POINTS = 8, 1024
POP_SD_MIN, POP_SD_MAX = 0.05, 10.0
POP_COUNTS = ("updates", "updated", "skipped", "failed")                   # the rows of pop_get("counts")
POP_MODES = (None, "fixed", "sampled")


# ordinal (graded) responses (include/gpirt_hip.h gpirt_ordinal; gpirt_amd.ordinal)
ST_ORD = 16                       # the two uniforms per threshold of a threshold update: item index item0 + j, index 2 (c - 1) / 2 (c - 1) + 1
ORD_MAX_C, ORD_MIN_POINTS, ORD_MAX_POINTS, ORD_MAX_WIDTH, ORD_MAX_N = 8, 9, 1001, 64, 16384


class Ordinal(C.Structure):
    """gpirt_ordinal (include/gpirt_hip.h): the sizes, the counters since enable and the records."""
    _fields_ = [(k, C.c_int64) for k in ("on", "n", "m", "categories", "points", "width", "calls", "pinned", "failed", "updates",
                                         "planned_draws", "recorded", "irf_draws")] + [
        ("hi", C.c_double), ("last_ms", C.c_double), ("lp_width", C.c_int64), ("reserved", C.c_int64 * 3)]


# ordinal model fit (include/gpirt_hip.h gpirt_ordinal_fit; gpirt_amd.ordinal.fit_*)
ST_ORD_PPC = 17                   # the replicate of the ordinal PPC: item index item0 + j, index i
OFIT_WAIC, OFIT_PRED, OFIT_PPC = 1, 2, 4
OFIT_PARTS = {"waic": OFIT_WAIC, "pred": OFIT_PRED, "ppc": OFIT_PPC}
OFIT_UNIT_FIELDS = ("n_obs", "obs_score", "score_ge", "score_gt", "rep_score_sum", "rep_score_sumsq", "agree_sum", "dev_ge",
                    "nonfinite", "dev_obs_sum", "dev_rep_sum")       # uint64 but for the last two (doubles)
OFIT_CAT_FIELDS = ("obs_count", "rep_count_sum", "rep_count_sumsq", "count_ge", "count_gt")
OFIT_TOTALS = ("lppd", "p_waic", "elpd_waic", "waic", "se_elpd_waic")


class OrdinalFit(C.Structure):
    """gpirt_ordinal_fit (include/gpirt_hip.h): the sizes, the draws and the WAIC totals of a fit state block."""
    _fields_ = [(k, C.c_int64) for k in ("n", "m", "categories", "parts", "draws", "n_obs")] + [
        (k, C.c_double) for k in OFIT_TOTALS] + [("reserved", C.c_int64 * 5)]


class Pop(C.Structure):
    """gpirt_pop (include/gpirt_hip.h): the mode, the sizes, the totals over the groups and the last call's off-grid members."""
    _fields_ = [(k, C.c_int64) for k in ("on", "groups", "n", "points_mu", "points_sd", "calls") + POP_COUNTS + (
        "off_grid", "planned_draws", "recorded")] + [(k, C.c_double) for k in ("mu_hi", "sd_lo", "sd_hi", "last_ms")] + [
        ("reserved", C.c_int64 * 4)]


TICK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int)

_vp, _i64, _i32, _u64, _u32, _dbl = C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_uint32, C.c_double
_dp = C.POINTER(C.c_double)

# name -> (restype, argtypes); every symbol include/gpirt_hip.h declares
SIGNATURES = {
    "gpirt_version": (_i32, []),
    "gpirt_last_error": (C.c_char_p, []),
    "gpirt_device_count": (_i32, [C.POINTER(_i32)]),
    "gpirt_create": (_i32, [C.POINTER(_vp), _i32, _vp]),
    "gpirt_create_own_stream": (_i32, [C.POINTER(_vp), _i32]),
    "gpirt_destroy": (_i32, [_vp]),
    "gpirt_synchronize": (_i32, [_vp]),
    "gpirt_set_stream": (_i32, [_vp, _vp]),
    "gpirt_calibrate_mfma_f64": (_i32, [_vp, _dp]),
    "gpirt_config_get": (_i32, [_vp, C.c_char_p, C.POINTER(_i32)]),
    "gpirt_config_set": (_i32, [_vp, C.c_char_p, _i32]),
    "gpirt_guard_fallbacks": (_i32, [_vp, C.POINTER(_i32)]),
    "gpirt_debug_trip_guard": (_i32, [_vp, _i32]),
    "gpirt_debug_rs_cand_limit": (_i32, [_vp, _i32]),
    "gpirt_debug_rs_mispredict": (_i32, [_vp, _i32]),
    "gpirt_debug_poison_allocs": (_i32, [_vp, _i32]),
    "gpirt_debug_rs_trace": (_i32, [_vp, _i32]),
    "gpirt_debug_last_mcmc_fallbacks": (_i32, []),
    "gpirt_kernel_default": (None, [C.POINTER(Kernel)]),
    "gpirt_kernel_check": (_i32, [C.POINTER(Kernel), _i32, _dp, C.POINTER(_i32)]),
    "gpirt_kernel_set": (_i32, [_vp, C.POINTER(Kernel)]),
    "gpirt_kernel_get": (_i32, [_vp, C.POINTER(Kernel)]),
    "gpirt_se_kernel": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _dbl]),
    "gpirt_potrf_lower": (_i32, [_vp, _vp, _i64, _i64]),
    "gpirt_factor": (_i32, [_vp, _vp, _i64, _vp, _i64]),
    "gpirt_potrf_panel_width": (_i64, []),
    "gpirt_potrf_begin": (_i32, [_vp]),
    "gpirt_potrf_panel_factor": (_i32, [_vp, _vp, _i64, _i64, _i64]),
    "gpirt_potrf_panel_update": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64]),
    "gpirt_potrf_panel_copy": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp, _i32]),
    "gpirt_potrf_finish": (_i32, [_vp]),
    "gpirt_potrf_subpanel_width": (_i64, [_i64]),
    "gpirt_potrf_panel_factor_part": (_i32, [_vp, _vp, _i64, _i64, _i64, _i32]),
    "gpirt_potrf_panel_update_part": (_i32, [_vp, _vp, _i64, _i64, _i64, _i64, _i32]),
    "gpirt_potrf_panel_copy_part": (_i32, [_vp, _vp, _i64, _i64, _i64, _i32, _vp, _i64, _i32]),
    "gpirt_debug_streams_busy": (_i32, [_vp, C.POINTER(_i32)]),
    "gpirt_debug_ll_term": (_i32, [_vp, _vp, _i64, _vp, _i32]),
    "gpirt_debug_theta_logpost": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "gpirt_debug_theta_clock": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _i64]),
    "gpirt_debug_panel_trace": (_i32, [_vp, _i64, _vp, _i64]),
    "gpirt_trmm_lz": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64]),
    "gpirt_trsm_lower": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32]),
    "gpirt_gemm": (_i32, [_vp, _i32, _i32, _i64, _i64, _i64, _dbl, _vp, _i64, _vp, _i64, _dbl, _vp, _i64]),
    "gpirt_ll_bar": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp]),
    "gpirt_draw_f": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _u64, _u32, _vp]),
    "gpirt_draw_f_linear": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _u64, _u32, _vp]),
    "gpirt_draw_fstar": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _u64, _u32, _i32, _vp, _vp, _vp]),
    "gpirt_draw_theta": (_i32, [_vp, _vp, _vp, _i64, _i64, _u64, _u32, _i32, _vp, _vp]),
    "gpirt_draw_beta": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _u64, _u32]),
    "gpirt_draw_beta_paths": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _u64, _u32, _vp]),
    "gpirt_item_uniforms": (_i32, [_vp, _u64, _u32, _u32, _u32, _i64, _i64, _vp]),
    "gpirt_item_normals": (_i32, [_vp, _u64, _u32, _u32, _u32, _i64, _i64, _vp]),
    "gpirt_rstream_create": (_i32, [C.POINTER(_vp), _u32]),
    "gpirt_rstream_from_state": (_i32, [C.POINTER(_vp), C.POINTER(_u32), _i32]),
    "gpirt_rstream_get_state": (_i32, [_vp, C.POINTER(_u32), C.POINTER(_i32)]),
    "gpirt_rstream_destroy": (_i32, [_vp]),
    "gpirt_rstream_unif": (_i32, [_vp, _dp, _i64]),
    "gpirt_rstream_norm": (_i32, [_vp, _dp, _i64]),
    "gpirt_default_options": (None, [C.POINTER(Options)]),
    "gpirt_fast_options": (None, [C.POINTER(Options)]),
    "gpirt_mcmc": (_i32, [_dp, _i64, _i64, _dp, _i32, _i32, _dp, _dp, _dp, C.POINTER(Options), _vp,
                           TICK_FN, _vp, _dp, _dp, _dp, _dp]),
    "gpirt_mcmc_summary": (_i32, [_dp, _i64, _i64, _dp, _i32, _i32, _dp, _dp, _dp, C.POINTER(Options), _vp,
                                   TICK_FN, _vp, _dp, _dp, _dp, _dp, C.POINTER(Summary)]),
    "gpirt_sampler_summary_enable": (_i32, [_vp, _i32]),
    "gpirt_sampler_summary_enable_planned": (_i32, [_vp, _i32, _i64]),
    "gpirt_summary_state_bytes": (_i32, [_i64, _i64, _i32, C.POINTER(_i64)]),
    "gpirt_sampler_summary_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_chain_seed": (_u64, [_u64, _i32]),
    "gpirt_chains_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(_i32), _i32, _dp, C.POINTER(Summary),
                                     C.POINTER(Diag)]),
    "gpirt_mcmc_chains": (_i32, [_dp, _i64, _i64, _dp, _i32, _i32, _i32, _dp, _dp, _dp, C.POINTER(Options), _i32,
                                  TICK_FN, _vp, _dp, _dp, _dp, _dp, C.POINTER(Summary), C.POINTER(Diag)]),
    "gpirt_mcmc_run": (_i32, [_dp, _i64, _i64, _dp, _i32, _i32, _i32, _dp, _dp, _dp, C.POINTER(Options), _i32,
                               TICK_FN, _vp, _dp, _dp, _dp, _dp, C.POINTER(Summary), C.POINTER(Diag), C.POINTER(Run)]),
    "gpirt_irf_band_edges": (_i32, [_dp]),
    "gpirt_summary_quantiles": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(_i32), _i32, C.POINTER(Quantiles)]),
    "gpirt_sampler_ppc_enable": (_i32, [_vp, _i32]),
    "gpirt_sampler_ppc_accumulate": (_i32, [_vp]),
    "gpirt_sampler_ppc_get": (_i32, [_vp, C.c_char_p, _dp, _i64]),
    "gpirt_sampler_ppc_totals": (_i32, [_vp, _dp]),
    "gpirt_sampler_ppc_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_ppc_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(Ppc)]),
    "gpirt_sampler_rank_enable": (_i32, [_vp, C.POINTER(C.c_int64), _i32, _i32]),
    "gpirt_sampler_rank_accumulate": (_i32, [_vp]),
    "gpirt_sampler_rank_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_rank_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_rank_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(Ranks)]),
    "gpirt_sampler_score_enable": (_i32, [_vp, _dp, _i64]),
    "gpirt_sampler_score_accumulate": (_i32, [_vp]),
    "gpirt_sampler_score_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_score_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_score_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(Score)]),
    "gpirt_sampler_score_predict_enable": (_i32, [_vp, _i32]),
    "gpirt_sampler_score_predict_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_score_predict_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_score_predict_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(ScorePredict)]),
    "gpirt_sampler_ppc_pairs_enable": (_i32, [_vp, _i32]),
    "gpirt_sampler_ppc_pairs_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ppc_pairs_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_ppc_pairs_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(PpcPairs)]),
    "gpirt_sampler_ppc_bins_enable": (_i32, [_vp, _i32, C.POINTER(C.c_int), _i32]),
    "gpirt_sampler_ppc_bins_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ppc_bins_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_ppc_bins_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(PpcBins)]),
    "gpirt_sampler_shape_enable": (_i32, [_vp, _i32, _dp, _i32, _i32]),
    "gpirt_sampler_shape_accumulate": (_i32, [_vp]),
    "gpirt_sampler_shape_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_shape_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_shape_state_bytes": (_i32, [_i64, C.POINTER(_i64)]),
    "gpirt_shape_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(Shape)]),
    "gpirt_sampler_sumscore_enable": (_i32, [_vp, _vp, _i32]),
    "gpirt_sampler_sumscore_accumulate": (_i32, [_vp]),
    "gpirt_sampler_sumscore_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_sumscore_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_sumscore_state_bytes": (_i32, [_i64, _i64, C.POINTER(_i64)]),
    "gpirt_sumscore_grid_weights": (_i32, [_dp]),
    "gpirt_sumscore_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(Sumscore)]),
    "gpirt_sampler_ppc_dif_enable": (_i32, [_vp, _i32, C.POINTER(C.c_int32), _i32, C.POINTER(C.c_int), _i32]),
    "gpirt_sampler_ppc_dif_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ppc_dif_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_ppc_dif_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(PpcDif)]),
    "gpirt_ppc_scores_check": (_i32, [_i64, _i64, _i32, C.POINTER(C.c_int)]),
    "gpirt_sampler_ppc_scores_enable": (_i32, [_vp, _i32, C.POINTER(C.c_int), _i32]),
    "gpirt_sampler_ppc_scores_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ppc_scores_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_ppc_scores_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(PpcScores)]),
    "gpirt_acf_check": (_i32, [_i64, _i64, _i32, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64)]),
    "gpirt_sampler_acf_enable": (_i32, [_vp, _i32, _i64, _i64, _i32]),
    "gpirt_sampler_acf_accumulate": (_i32, [_vp]),
    "gpirt_sampler_acf_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_acf_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_acf_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(Acf)]),
    "gpirt_groups_check": (_i32, [_i64, _i64, _i32, C.POINTER(C.c_int32), _i32, C.POINTER(_i64)]),
    "gpirt_sampler_groups_enable": (_i32, [_vp, _i32, C.POINTER(C.c_int32), _i32, _i32]),
    "gpirt_sampler_groups_accumulate": (_i32, [_vp]),
    "gpirt_sampler_groups_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_groups_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_groups_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(Groups)]),
    "gpirt_ppc_person_check": (_i32, [_i64, _i64, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int)]),
    "gpirt_sampler_ppc_person_enable": (_i32, [_vp, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int), _i32]),
    "gpirt_sampler_ppc_person_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ppc_person_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_ppc_person_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(PpcPerson)]),
    "gpirt_sampler_ppc_resid_enable": (_i32, [_vp, _i32]),
    "gpirt_sampler_ppc_resid_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ppc_resid_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_ppc_resid_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(PpcResid)]),
    "gpirt_sampler_equate_enable": (_i32, [_vp, _vp, _vp, _i32]),
    "gpirt_sampler_equate_accumulate": (_i32, [_vp]),
    "gpirt_sampler_equate_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_equate_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_equate_state_bytes": (_i32, [_i64, _i64, _i64, C.POINTER(_i64)]),
    "gpirt_equate_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(Equate)]),
    "gpirt_sampler_loo_enable": (_i32, [_vp, _i64, _i32, _i32]),
    "gpirt_sampler_loo_accumulate": (_i32, [_vp]),
    "gpirt_sampler_loo_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_loo_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_loo_tail_length": (_i32, [_i64, _i32, C.POINTER(_i64)]),
    "gpirt_loo_state_bytes": (_i32, [_i64, _i64, _i64, C.POINTER(_i64)]),
    "gpirt_loo_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(Loo)]),
    "gpirt_sampler_shape_order_enable": (_i32, [_vp, _i32]),
    "gpirt_sampler_shape_order_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_shape_order_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_shape_order_state_bytes": (_i32, [_i64, _i32, C.POINTER(_i64)]),
    "gpirt_shape_order_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(ShapeOrder)]),
    "gpirt_sampler_summary_accumulate": (_i32, [_vp]),
    "gpirt_sampler_summary_get": (_i32, [_vp, C.c_char_p, _dp, _i64]),
    "gpirt_sampler_summary_totals": (_i32, [_vp, _dp]),
    "gpirt_sampler_create": (_i32, [C.POINTER(_vp), _vp, _dp, _i64, _i64, _dp, _dp, _dp, _dp,
                                     C.POINTER(Options), _vp]),
    "gpirt_sampler_destroy": (_i32, [_vp]),
    "gpirt_sampler_init": (_i32, [_vp]),
    "gpirt_sampler_step": (_i32, [_vp]),
    "gpirt_sampler_draw_f": (_i32, [_vp]),
    "gpirt_sampler_draw_fstar": (_i32, [_vp]),
    "gpirt_sampler_theta_partial": (_i32, [_vp]),
    "gpirt_sampler_theta_finish": (_i32, [_vp]),
    "gpirt_sampler_set_theta_block": (_i32, [_vp, _vp, _i64, _i64, _i64]),
    "gpirt_sampler_theta_block": (_i32, [_vp]),
    "gpirt_sampler_theta_commit": (_i32, [_vp]),
    "gpirt_sampler_draw_beta": (_i32, [_vp]),
    "gpirt_sampler_factor": (_i32, [_vp]),
    "gpirt_sampler_skip_factor": (_i32, [_vp]),
    "gpirt_sampler_adopt_factor": (_i32, [_vp, _i32]),
    "gpirt_sampler_build_cov": (_i32, [_vp]),
    "gpirt_sampler_panel_factor": (_i32, [_vp, _i64]),
    "gpirt_sampler_panel_update": (_i32, [_vp, _i64, _i64]),
    "gpirt_sampler_panel_copy": (_i32, [_vp, _i64, _vp, _i32]),
    "gpirt_sampler_panel_rows": (_i32, [_vp, C.POINTER(_i64)]),
    "gpirt_sampler_panel_factor_part": (_i32, [_vp, _i64, _i32]),
    "gpirt_sampler_panel_update_part": (_i32, [_vp, _i64, _i64, _i32]),
    "gpirt_sampler_panel_copy_part": (_i32, [_vp, _i64, _i32, _vp, _i64, _i32]),
    "gpirt_sampler_ldl": (_i32, [_vp, C.POINTER(_i64)]),
    "gpirt_sampler_nu_lr_draws": (_i32, [_vp, C.POINTER(_i64)]),
    "gpirt_sampler_ess_pack_draws": (_i32, [_vp, C.POINTER(_i64)]),
    "gpirt_sampler_nu_lr_rows": (_i32, [_vp, _vp, _i64]),
    "gpirt_sampler_fstar_free_draws": (_i32, [_vp, C.POINTER(_i64)]),
    "gpirt_sampler_factor_lr_count": (_i32, [_vp, C.POINTER(_i64)]),
    "gpirt_sampler_dense_factor_count": (_i32, [_vp, C.POINTER(_i64)]),
    "gpirt_sampler_dense_factor": (_i32, [_vp]),
    "gpirt_sampler_factor_lr_parts": (_i32, [_vp, _vp, _i64]),
    "gpirt_sampler_factor_lr_width": (_i32, [_vp, C.POINTER(_i32)]),
    "gpirt_sampler_factor_lr_blocks": (_i32, [_vp, _vp, _i64]),
    "gpirt_sampler_copy_state": (_i32, [_vp, _vp]),
    "gpirt_sampler_accumulate_irf": (_i32, [_vp]),
    "gpirt_sampler_iteration": (_i32, [_vp, C.POINTER(_i32)]),
    "gpirt_sampler_check": (_i32, [_vp]),
    "gpirt_sampler_devptr": (_i32, [_vp, C.c_char_p, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_sampler_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_set": (_i32, [_vp, C.c_char_p, _dp, _i64]),
    "gpirt_sampler_finish_irfs": (_i32, [_vp, _i32, _dp]),
    "gpirt_sampler_enable_timing": (_i32, [_vp, _i32]),
    "gpirt_sampler_stage_times": (_i32, [_vp, _dp, _i32, C.POINTER(_i32), C.POINTER(C.c_char_p)]),
    "gpirt_prof_trailing": (_i32, [_vp, _i32, _dp, C.POINTER(_i64), _dp]),
    "gpirt_prof_enable": (_i32, [_vp, _i32]),
    "gpirt_prof_syrk": (_i32, [_vp, _i32, _i32, _dp, C.POINTER(_i64), _dp]),
    "gpirt_prof_syrk_bytes": (_i32, [_vp, _i32, _dp]),
    "gpirt_sampler_set_iteration": (_i32, [_vp, _i32]),
    "gpirt_ell_grid": (_i32, [_dbl, _dbl, _i32, _dp]),
    "gpirt_ell_check": (_i32, [_dbl, _dbl, _i32, _dp, _i32, _i32, C.POINTER(Kernel), C.POINTER(Options), _i64]),
    "gpirt_sampler_ell_enable": (_i32, [_vp, _dbl, _dbl, _i32, _dp, _i32, _i32, _i32]),
    "gpirt_sampler_draw_ell": (_i32, [_vp]),
    "gpirt_sampler_ell_width": (_i32, [_vp, _i32]),
    "gpirt_sampler_ell_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ell_stats": (_i32, [_vp, C.POINTER(Ell)]),
    "gpirt_sampler_draw_ell_centred": (_i32, [_vp]),
    "gpirt_sampler_ell_width_centred": (_i32, [_vp, _i32]),
    "gpirt_sampler_ell_centred_stats": (_i32, [_vp, C.POINTER(EllCentred)]),
    "gpirt_amp_check": (_i32, [_dbl, _dbl, _i32, _dp, _i32, C.POINTER(_i32), _i64, C.POINTER(Options)]),
    "gpirt_sampler_amp_set": (_i32, [_vp, _dp]),
    "gpirt_sampler_amp_enable": (_i32, [_vp, _dbl, _dbl, _i32, _dp, _i32, C.POINTER(_i32), _i64, _i32]),
    "gpirt_sampler_draw_amp": (_i32, [_vp]),
    "gpirt_sampler_amp_width": (_i32, [_vp, C.POINTER(_i32)]),
    "gpirt_sampler_amp_record": (_i32, [_vp]),
    "gpirt_sampler_amp_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_amp_stats": (_i32, [_vp, C.POINTER(Amp)]),
    "gpirt_sampler_draw_amp_centred": (_i32, [_vp]),
    "gpirt_sampler_amp_centred_stats": (_i32, [_vp, C.POINTER(AmpCentred)]),
    "gpirt_sampler_draw_beta_centred": (_i32, [_vp]),
    "gpirt_sampler_beta_centred_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_beta_centred_stats": (_i32, [_vp, C.POINTER(BetaCentred)]),
    "gpirt_sampler_scale_enable": (_i32, [_vp, _dbl, _dbl]),
    "gpirt_sampler_scale_width": (_i32, [_vp, _i32, _dbl]),
    "gpirt_sampler_draw_scale": (_i32, [_vp, _i32]),
    "gpirt_sampler_scale_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_scale_stats": (_i32, [_vp, C.POINTER(Scale)]),
    "gpirt_sampler_step_consistent_scale": (_i32, [_vp, _i32, _i32]),
    "gpirt_pop_check": (_i32, [C.POINTER(C.c_int32), _i64, _i32, _dp, _i64, _i32, _dbl, _i32, _dbl, _dbl, _i32, _dp, _dp,
                               C.POINTER(_i32), C.POINTER(_i32), C.POINTER(Options)]),
    "gpirt_pop_default_row": (_i32, [_dp]),
    "gpirt_pop_normal_row": (_i32, [_dbl, _dbl, _dp]),
    "gpirt_pop_grids": (_i32, [_dbl, _i32, _dbl, _dbl, _i32, _dp, _dp]),
    "gpirt_pop_lse": (_i32, [_dp, _i32, _dp, _i32, _dp]),
    "gpirt_sampler_pop_set": (_i32, [_vp, C.POINTER(C.c_int32), _i32, _dp]),
    "gpirt_sampler_pop_enable": (_i32, [_vp, C.POINTER(C.c_int32), _i32, _dp, _dbl, _i32, _dbl, _dbl, _i32, _dp, _dp,
                                        C.POINTER(_i32), C.POINTER(_i32), _i64, _i32]),
    "gpirt_sampler_draw_pop": (_i32, [_vp]),
    "gpirt_sampler_pop_record": (_i32, [_vp]),
    "gpirt_sampler_pop_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_pop_stats": (_i32, [_vp, C.POINTER(Pop)]),
    "gpirt_ordinal_check": (_i32, [C.POINTER(C.c_int8), _dp, _i64, _i64, _i32, _dbl, _i32, _dp, C.POINTER(C.c_int32), _i32,
                                   C.POINTER(Options)]),
    "gpirt_ordinal_grid": (_i32, [_dbl, _i32, _dp]),
    "gpirt_sampler_ordinal_enable": (_i32, [_vp, C.POINTER(C.c_int8), _i32, _dbl, _i32, _dp, C.POINTER(C.c_int32), _i32, _i64]),
    "gpirt_sampler_draw_thresholds": (_i32, [_vp]),
    "gpirt_sampler_ordinal_width": (_i32, [_vp, _i32]),
    "gpirt_sampler_ordinal_record": (_i32, [_vp]),
    "gpirt_sampler_ordinal_accumulate_irf": (_i32, [_vp]),
    "gpirt_sampler_ordinal_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ordinal_stats": (_i32, [_vp, C.POINTER(Ordinal)]),
    "gpirt_sampler_ordinal_fit_enable": (_i32, [_vp, _i32]),
    "gpirt_sampler_ordinal_fit_accumulate": (_i32, [_vp]),
    "gpirt_sampler_ordinal_fit_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ordinal_fit_totals": (_i32, [_vp, C.POINTER(OrdinalFit)]),
    "gpirt_sampler_ordinal_fit_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_ordinal_fit_combine": (_i32, [_vp, C.POINTER(_vp), _i32, _vp]),
    "gpirt_ordinal_fit_get": (_i32, [_vp, _vp, C.c_char_p, _vp, _i64]),
    "gpirt_ordinal_fit_totals": (_i32, [_vp, _vp, C.POINTER(OrdinalFit)]),
    "gpirt_sampler_ordinal_score_enable": (_i32, [_vp, C.POINTER(C.c_int8), _i64, _i32, _i32]),
    "gpirt_sampler_ordinal_score_accumulate": (_i32, [_vp]),
    "gpirt_sampler_ordinal_score_get": (_i32, [_vp, C.c_char_p, _vp, _i64]),
    "gpirt_sampler_ordinal_score_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_sampler_ordinal_score_predict_state": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "gpirt_ordinal_score_combine": (_i32, [_vp, _i32, C.POINTER(_vp), C.POINTER(_i32), _vp, _i64]),
    "gpirt_ordinal_score_predict_combine": (_i32, [_vp, _i32, C.POINTER(_vp), _vp, _i64]),
    "gpirt_sampler_carry_f": (_i32, [_vp, _i32]),
    "gpirt_sampler_step_consistent": (_i32, [_vp, _i32]),
    "gpirt_sampler_carry_stats": (_i32, [_vp, C.POINTER(Carry)]),
    "gpirt_sampler_prior_quad": (_i32, [_vp, _dp]),
}

_lib = None


def load():
    """dlopen the in-tree HIP library and attach the signatures (fails loudly if it is missing)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GpirtError(E_NODEVICE, f"{LIB_PATH} is missing: build it with "
                                         "`python -m gpirt_amd.build` (hipcc, gfx950). There is no CPU fallback.")
        # Load order matters in a Python process that also uses PyTorch-ROCm: torch bundles its own HIP runtime, and a
        # process that initialises the system runtime first (through this library) and torch's second ends with one of
        # them reporting "no ROCm-capable device".  Importing torch first makes the order the same everywhere
        # (the R host of INTEGRATION.md has no torch and no such issue).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return load().gpirt_last_error().decode("utf-8", "replace")


def check(rc: int) -> int:
    if rc < 0:
        raise GpirtError(rc, last_error())
    return rc


def state_ptrs(states, method: str):
    """What every combine starts from: the states as device tensors (a Sampler gives its `method`(), e.g. "rank_state"; a
    tensor is taken as it is), their count and their device pointers as a C array of void*."""
    tensors = [getattr(s, method)() if hasattr(s, method) else s for s in states]
    nc = len(tensors)
    return tensors, nc, (C.c_void_p * nc)(*[t.data_ptr() for t in tensors])


def header_words(state, words: int = 8) -> np.ndarray:
    """The first `words` 8-byte words of a state block (a torch tensor on the device, int64 or float64) as int64 on the host."""
    return state[:words].detach().cpu().numpy().view(np.int64)


def default_options() -> Options:
    o = Options()
    load().gpirt_default_options(C.byref(o))
    return o


def fast_options() -> Options:
    """The throughput preset of the C ABI (gpirt_fast_options): item-keyed RNG, theta_stabilise, fused + rank-64 draw_fstar."""
    o = Options()
    load().gpirt_fast_options(C.byref(o))
    return o
