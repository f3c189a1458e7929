"""Sampler-level host API: the gpirtMCMC() mirror and the stage-driven Sampler.

`gpirtMCMC()` keeps the reference's R signature and returned list (R/gpirtMCMC.R:85-105,
src/gpirtMCMC.cpp:112-116); it prepares the data exactly like the R wrapper and then crosses the
same boundary the R shim would (.Call -> extern "C" gpirt_mcmc, include/gpirt_hip.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import NGRID, RNG_ITEM, RNG_RSTREAM, Options, check
from .response_matrix import as_response_matrix

_dp = C.POINTER(C.c_double)


def _f64(a):
    return np.asfortranarray(np.array(a, dtype=np.float64))


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _options(rng, seed, theta_stabilise, fstar_fused, device, item0=0, m_total=0, kernel_fp32=False,
             kstar_rank=0, factor_structured=False) -> Options:
    o = _lib.default_options()
    o.rng_kind = RNG_RSTREAM if rng == "reference" else RNG_ITEM
    o.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    o.theta_stabilise = int(bool(theta_stabilise))
    o.fstar_fused = int(bool(fstar_fused))
    o.device = -1 if device is None else int(device)
    o.item0 = int(item0)
    o.m_total = int(m_total)
    o.kernel_fp32 = int(bool(kernel_fp32))
    o.kstar_rank = int(kstar_rank)
    o.factor_structured = int(bool(factor_structured))
    return o


def _call_options(rng, seed, preset, theta_stabilise, fstar_fused, kstar_rank, device) -> Options:
    """The options of a whole call: the library's fast preset with this call's seed and device, or the keywords'."""
    if preset == "fast":
        o = _lib.fast_options()
        o.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        o.device = -1 if device is None else int(device)
        return o
    return _options(rng, seed, theta_stabilise, fstar_fused, device, kstar_rank=kstar_rank)


def gpirtMCMC(data, sample_iterations, burn_iterations, vote_codes=None, beta_prior_means=None,
              beta_prior_sds=None, beta_proposal_sds=None, theta_init=None, *, rng="reference",
              seed=1, rstream=None, theta_stabilise=False, fstar_fused=False, kstar_rank=0, device=None,
              progress=False, preset=None, summaries=None, store_draws=True, chains=None, align=True, quantiles=None,
              ppc=None, ranks=None, score=None, shape=None, sumscore=None, equate=None, loo=None):
    """Drop-in for the reference's gpirtMCMC() (R/gpirtMCMC.R:85-105) on one MI355X.

    Positional arguments, defaults and the returned dict (theta (S+1) x n, beta 2 x m x (S+1),
    f n x m x (S+1), IRFs 1001 x m) follow the reference.  Keyword-only extras select the RNG
    contract instead of new required arguments:
      rng="reference": replay R's Mersenne-Twister stream (`rstream`, or RStream(seed), stands in
                       for R's .Random.seed); draw-for-draw comparable with the reference;
      rng="item":      counter-based per-item sub-streams keyed by `seed` (batched, shardable).
    fstar_fused / kstar_rank: algebraically identical, cheaper forms of draw_fstar:
      the mean as (L^-1 k*)^T (L^-1 f), and K(theta, theta*) through its exact rank-r Chebyshev factorisation.
    preset="fast": the library's throughput preset, gpirt_fast_options() (R: options(gpirt.hip.preset = "fast")) --
      item-keyed RNG with this call's `seed`, theta_stabilise, fstar_fused, kstar_rank = 64; what bench.py times.
    summaries: posterior summaries accumulated on the device over the S sampling iterations (include/gpirt_hip.h
      GPIRT_SUM_*): part names ("waic", "pred", "f", "theta_beta") or their bits.  The result then has a "summary" entry:
      the arrays of those parts (theta / beta moments always) and "totals" (a dict; WAIC's, with "waic").
    store_draws: True, False, or a subset of ("theta", "beta", "f"); a draw that is not stored comes back as None.  With
      summaries and no stored f a long chain at 8192 x 1024 needs O(n m) host memory instead of n m 8 bytes per iteration.
    chains: C chains one after another (gpirt_mcmc_chains; the item RNG only, chain c seeded gpirt_chain_seed(seed, c)).
      The draws come back stacked per chain (theta C x (S+1) x n, beta C x 2 x m x (S+1), f C x n x m x (S+1)), "summary"
      is pooled over the chains and "diagnostics" holds split-R-hat, the batch-means ESS and the MCSE of every theta, beta
      (and with "f" in summaries, f) value, their per-block scalars and the chains reflected by the theta -> -theta
      alignment (align=False: none).  theta_init may be (C, n); by default chain 0 starts at RStream(seed).rnorm(n) as
      today and chain c at RStream(chain_seed(seed, c) & 0xFFFFFFFF).rnorm(n).  chains=None: one chain, as before.
    quantiles: probabilities, e.g. (0.025, 0.5, 0.975) (gpirt_run.quantiles, gpirt_amd.quantiles): every chain also
      keeps theta histograms and IRF bands on the device (and the DIAG accumulators), for chains=None too; rng="reference"
      runs one chain, the chain gpirt_mcmc_summary runs.  The result gains "summary" and "diagnostics" as with chains and
      "quantiles": probs, theta (len(probs) x n, exact), theta_median, theta_mode, theta_hist, theta_rhat (the
      rank-normalised bulk / tail / max), irf (len(probs) x 1001 x m, in probability, within 1/256), irf_p_mean (E[P]),
      reflected and scalars.  Memory: the band is 1001 x m x 256 x 4 bytes per chain on the device (1.05 GB at
      m = 1024), theta's histograms 3 x 1001 x n x 4 bytes.  quantiles=None leaves every other path as it is.
    ppc: True adds posterior predictive checks (gpirt_run.ppc, gpirt_amd.ppc): after every sampling iteration the
      device replicates the response matrix from that draw and compares the yes count and the deviance of the replicate
      with the data's, per item, per respondent and overall, in O(n + m) memory.  The result gains "ppc": "item" and
      "respondent" (dicts of arrays: n_obs, obs_yes, rep_yes_mean, rep_yes_var, yes_ge, yes_gt, dev_obs_mean,
      dev_rep_mean, dev_ge, correct_mean, nonfinite, draws and the derived ppp_yes, ppp_yes_mid, ppp_dev) and "totals",
      and -- the call runs gpirt_mcmc_chains's chains -- "summary" and "diagnostics" as with
      chains (draws stacked per chain only with chains given).  The chain itself is untouched: the replicate draws from
      the counter-based generator under both RNG contracts and consumes nothing of R's stream.  ppc=None leaves every
      other path as it is.
      ppc=dict(pairs=True, top=20) also checks every PAIR of items (gpirt_run.pairs): "ppc" gains "pairs" with, per
      ordered pair (a, b) as m x m arrays, the observed 2 x 2 table over the co-observed respondents (n_co, obs_n11,
      obs_n10, obs_n01, obs_n00), the replicates' (rep_n11_mean, rep_n11_var, rep_n10_mean, rep_n01_mean, rep_n00_mean),
      agree_obs / agree_rep_mean, log_or_obs and the posterior predictive p-values ppp_n11, ppp_agree, ppp_or with their
      mid-p forms; "extreme" lists the `top` (1..64) pairs a < b whose ppp_or_mid lies farthest from 0.5 -- the pairs whose
      dependence the one-dimensional model does not reproduce; pair_draws, pair_skipped (a draw with a non-finite g in an
      observed cell is skipped whole for the pairs) and the raw sums and counts.  Memory: 68 bytes per ordered pair on the
      device (71 MB at m = 1024) plus the int8 operands; n <= 65534.  ppc=True is exactly as without it.
      ppc=dict(bins=True, bins_top=20) (or bins=(d_1, ..., d_h), the positive cut points as hundredths of theta or theta
      values; True = gpirt_amd.ppc.DEFAULT_CUTS, nine bins of equal N(0, 1) probability) also checks every item's
      response curve along theta (gpirt_run.bins): each draw groups the respondents by the bin of their theta, and "ppc"
      gains "bins" with, per (bin, item) as B x m arrays, obs_rate (the empirical IRF), rep_rate, exp_rate, z_mean,
      ppp_cell, ppp_cell_mid and n_mean; per item ppp_chi2, ppp_chi2_mid, chi2_obs_mean and chi2_rep_mean (the binned
      chi-square of the data against the replicates'); per bin occupancy, bin_lo, bin_hi; "worst" lists the `bins_top`
      (1..64) items with the smallest ppp_chi2_mid -- the items whose curve the data contradict; bin_draws, bin_skipped (a
      draw with a theta off the grid or a non-finite g in an observed cell is skipped whole) and the raw sums and counts.
      pairs and bins may be asked for together.
      ppc=dict(dif=groups) or dif=dict(groups=g, cuts=None, top=20) also checks measurement invariance (gpirt_run.dif):
      groups holds one code per row of the prepared data (-1 = left out, 0 = the reference group, 1..G-1 the focal groups,
      G <= 4).  Each draw stratifies the respondents by the bin of their theta (cuts as for bins; None = DEFAULT_CUTS), and
      "ppc" gains "dif" with the group-wise empirical IRFs obs_rate, rep_rate, exp_rate (G x B x m) and occupancy (G x B);
      per (group, item) ppp_yes, ppp_yes_mid, ppp_chi2, ppp_chi2_mid, chi2_obs_mean, chi2_rep_mean; per (focal group, item),
      indexed by the group code with row 0 NaN, the Mantel-Haenszel mh_log_or_obs_mean, mh_log_or_rep_mean,
      mh_delta_obs_mean (the ETS delta scale), ppp_mh, ppp_mh_mid, mh_undefined and the standardised P-difference
      std_obs_mean, std_rep_mean; "flagged" lists the `top` (1..64) (item, focal group) pairs whose ppp_mh_mid lies farthest
      from 0.5; dif_draws, dif_skipped, group_size and the raw sums and counts.  n <= 65534.  It composes with pairs and bins.
    ranks: True, or dict(pivots="median", pairwise=False, probs=(0.025, 0.5, 0.975)), adds the rank posteriors
      (gpirt_run.ranks, gpirt_amd.ranks): after every sampling iteration the device ranks that draw's theta (rank 1 =
      the smallest; ties take the mid-rank) and accumulates, in "ranks": rank_mean, rank_var, rank_quantiles
      (len(probs) x n, a rank-histogram bin's upper edge; exact for n <= 512), rank_bin_width, order (argsort of
      rank_mean), pivots (the positions asked for -- "median" and / or positions in 1..n, at most 16 --, closed under
      q <-> n + 1 - q and sorted), p_pivot and pivot_cover (len(pivots) x n), p_less (n x n, P(theta_i < theta_j)) or
      None, draws, skipped_draws (a draw with any theta off the grid is skipped whole), and the raw rank2_sum,
      rank2_sumsq, rank_hist, pivot_share, lt.  Memory with pairwise=True: 4 n^2 bytes per chain on the device (268 MB
      at n = 8192).  Chains are pooled with the reflection "diagnostics" reports.  Nothing is drawn: the chain is
      untouched under both RNG contracts.  "summary" and "diagnostics" come as with ppc.  ranks=None leaves every other
      path as it is.
    score: y_new (n_new x m), or dict(data=y_new, probs=(0.025, 0.5, 0.975)), scores respondents who are NOT in the fit
      (gpirt_run.score, gpirt_amd.score): y_new is coded +1 / -1 / NaN over the prepared data's m item columns (after
      unanimous items were dropped; another width is a ValueError), 1 <= n_new <= 16384.  After every sampling iteration
      the device forms, from that draw's f*, each new respondent's normalised posterior over the theta grid and the log
      marginal likelihood of their answers, and accumulates them; "score" holds grid_post (n_new x 1001), theta_mean,
      theta_sd, theta_quantiles (len(probs) x n_new), theta_map, lpd (the log pointwise predictive density of the
      respondent's answers), loglik_mean, n_obs, lpd_total, se_lpd_total, draws, nonfinite (a draw whose log-posterior is
      not finite for a respondent is skipped for that respondent alone) and the raw post_sum, lpd_acc, ll_sum.  Chains are
      pooled with the reflection "diagnostics" reports.  Nothing is drawn: the chain is untouched under both RNG contracts.
      "summary" and "diagnostics" come as with ranks.  score=None leaves every other path as it is.
      dict(data=y_new, predict=True, top=5) also predicts the answers those respondents have NOT given
      (gpirt_run.predict): "score" gains "predict" with p_yes (n_new x m: P(y_rj = +1 | y_new[r, :]), for every item),
      info (n_new x m: the expected information, in nats, that the answer to item j carries about theta_r -- the mutual
      information under each draw, averaged over the draws; valid for non-monotone items), next_items and next_info
      (n_new x top: each respondent's UNANSWERED items by decreasing info, padded with -1 / NaN; 1 <= top <= 16), pred_draws,
      pred_skipped (a draw whose f* holds a NaN cell is skipped whole for the prediction) and the raw pred_sum, info_sum.
      Without predict the score= argument behaves exactly as before, and the scores themselves do not depend on it.
    shape: True, or dict(window=3.0, tols=(0.0, 0.25, 1.0), probs=(0.025, 0.5, 0.975), top=20), adds the shape posteriors of
      the item response curves (gpirt_run.shape, gpirt_amd.shape): after every sampling iteration the device reads that
      draw's smooth curve g = k*^T S^-1 f + mu* (what draw_fstar draws f* around) and accumulates, per item, inside
      |theta| <= window (0.01..5.0): p_nonmonotone, p_increasing, p_decreasing, p_flat (len(tols) x m: the draw's largest fall
      and rise against each tolerance, in logits; at most 4), peak_quantiles and valley_quantiles (len(probs) x m, theta of
      the argmax / argmin), p_peak_interior, crossings (4 x m: P(0, 1, 2, >= 3 crossings of P = 1/2)), difficulty_quantiles
      (the first crossing), slope_max_mean, slope_min_mean (and _sd), and over the whole grid item_info (1001 x m, the mean
      Fisher information), test_info_mean, test_info_sd, sem (1001), reliability_mean, reliability_sd; "nonmonotone" lists the
      `top` (1..64) items most often non-monotone at the largest tolerance (items, p).  draws / nonfinite count per item (a
      curve with any non-finite value is skipped), info_draws / info_skipped per draw; the raw accumulators come with it.
      Memory at m = 1024: 24 MB of accumulators per chain plus 8 MB each for the curve and the draw's information.  Nothing is
      drawn: the chain is untouched under both RNG contracts.  Reflected chains are reflected exactly on their accumulators.
      shape=None leaves every other path as it is.  Two more keys, order=True and order_top=20 (1..64), add the item-pair order
      posteriors as out["shape"]["order"] (gpirt_run.order, gpirt_amd.shape.order_finish): per tolerance and ordered pair of
      items p_above, p_cross, p_tied (curve a above b on the whole window, crossing it, neither), p_easier, depth_mean,
      easiness_mean / _sd, rank_mean, order, cross_items_mean, p_iio, cross_pairs_mean / _sd, worst (the order_top pairs that
      cross most often at the largest tolerance), draws, skipped and the raw arrays; 2 <= m <= 4096, 46 MB per chain at m = 1024.
    sumscore: True, or dict(items=None, probs=(0.025, 0.5, 0.975)), adds the posteriors of the SUM SCORE S = number of yes
      answers on a form of items (gpirt_run.sumscore, gpirt_amd.sumscore): after every sampling iteration the device runs
      the Lord-Wingersky recursion over the form's items at every grid point of that draw's f*.  items: None (all items),
      column indices or a boolean mask over the PREPARED data's columns (after unanimous items were dropped); at most 4096
      items; a wrong index or an empty form is a ValueError.  "sumscore" holds score_dist, score_dist_sd, score_cdf (M + 1: the
      score distribution the model implies for a N(0, 1) population), post ((M + 1) x 1001: p(theta_k | S = s, data), the
      pooled joint normalised once -- not score='s mean of per-draw posteriors), theta_eap, theta_sd, theta_quantiles
      (len(probs) x (M + 1)), theta_map (the conversion table; NaN for a score without mass), score_given_theta (1001 x
      (M + 1)), tcc_mean, tcc_sd, csem (1001: the expected score along theta, its posterior sd, the predictive sd of the
      score at theta), reliability_mean, reliability_sd (the model-based counterpart of Cronbach's alpha), n_complete,
      obs_hist, exp_count (over the respondents who answered every item of the form), draws, skipped (a draw whose f* holds a
      NaN in a form column is skipped whole), rel_draws, rel_skipped, items and the raw accumulators.  Memory at M = 1024:
      33 MB per chain.  Nothing is drawn: the chain is untouched under both RNG contracts.  sumscore=None leaves every other
      path as it is.
    equate: dict(x=items_x, y=items_y, probs=(0.025, 0.5, 0.975), cuts=((cx, cy), ...)) relates the sum scores on TWO disjoint
      forms (gpirt_run.equate, gpirt_amd.equate): after every sampling iteration the device runs the sum-score recursion once
      per form and contracts the two score tables over the grid in one fp64 matrix-core product, the draw's joint distribution
      of (S_X, S_Y) for a N(0, 1) population.  x, y: column indices or boolean masks over the PREPARED data's columns, each
      non-empty, at most 2048 items, no column in both; cuts: up to 8 pairs of pass marks (a score >= the cut passes).  "equate"
      holds joint ((M_X + 1) x (M_Y + 1)), x_dist, x_dist_sd, y_dist, y_dist_sd, the equipercentile equivalents y_of_x_mean,
      y_of_x_sd (M_X + 1: an X score on Y's scale, posterior mean and sd over draws), x_of_y_mean, x_of_y_sd, the concordance
      y_given_x ((M_X + 1) x (M_Y + 1)), y_given_x_mean, y_given_x_quantiles (len(probs) x (M_X + 1)), x_given_y, x_given_y_mean,
      x_given_y_quantiles (rows of the pooled joint normalised once; NaN for a score without mass), corr_mean, corr_sd (the
      correlation of the two scores, per draw), agreement, kappa (per cut, from the pooled joint), draws, skipped (a draw whose
      f* holds a NaN in a column of either form is skipped whole), corr_draws, corr_skipped, eq_clamped, x_items, y_items and
      the raw accumulators.  Memory at M_X = M_Y = 1024: 75 MB per chain.  Nothing is drawn: the chain is untouched under both
      RNG contracts.  equate=None leaves every other path as it is.
    loo: True or dict(tail=None, top=20) adds PSIS-LOO (gpirt_run.loo, gpirt_amd.loo): after every sampling iteration the device
      enters each observed cell's key -y (f + mu) into the cell's heap of the M + 1 largest keys, T = chains x sample_iterations,
      M = min(T // 5, ceil(3 sqrt(T))) or `tail` (5 .. 1024); at the end one wave per cell fits the generalised Pareto tail.
      "loo" holds the totals elpd_loo, se_elpd_loo, p_loo, looic, se_looic, n_obs, lppd, k_threshold, k_good, k_bad, k_very_bad,
      unsmoothed, cells_incomplete; pointwise (pareto_k, elpd_loo, n_eff, lppd, p_loo, loo_p_yes, n x m each, NaN for a missing or
      an incomplete cell); item_elpd_loo (m), respondent_elpd_loo (n); worst (the `top` cells with the largest pareto_k: index,
      row, col, pareto_k); raw (the pooled state: tail = the kept keys descending, keys, evicted_sum, evicted_sumsq, p_sum, count,
      nonfinite, y) and T, M, draws, chains.  gpirt_amd.loo.compare(a["loo"], b["loo"]) is the elpd difference of two models
      with its standard error.  Memory: (8 (M + 1) + 32) bytes per cell and state, two states while chains are pooled.  Nothing
      is drawn: the chain is untouched under both RNG contracts.  loo=None leaves every other path as it is.
    """
    from .ops import RStream

    lib = _lib.load()
    data = as_response_matrix(data, vote_codes)                      # R/gpirtMCMC.R:93
    y = _f64(np.asarray(data))
    n, m = y.shape
    # defaults are evaluated AFTER the unanimous items were dropped (R lazy evaluation, quirk Q8)
    pm = _f64(np.zeros((2, m)) if beta_prior_means is None else beta_prior_means)
    ps = _f64(np.full((2, m), 3.0) if beta_prior_sds is None else beta_prior_sds)
    st = _f64(np.full((2, m), 0.1) if beta_proposal_sds is None else beta_proposal_sds)
    for a in (pm, ps, st):
        if a.shape != (2, m):
            raise ValueError("beta prior / proposal matrices must be 2 x ncol(data)")
    if preset == "fast":
        rng = "item"
    elif preset is not None:
        raise ValueError(f"unknown preset {preset!r}")
    if ranks is not None and ranks is not False:
        if ranks is not True and not isinstance(ranks, dict):
            raise ValueError("ranks must be None, False, True or a dict(pivots=..., pairwise=..., probs=...)")
        ranks = dict(ranks) if isinstance(ranks, dict) else {}
        unknown = set(ranks) - {"pivots", "pairwise", "probs"}
        if unknown:
            raise ValueError(f"ranks: unknown keys {sorted(unknown)}")
    else:
        ranks = None
    if score is not None:
        from . import score as SC
        if isinstance(score, dict):
            unknown = set(score) - {"data", "probs", "predict", "top"}
            if unknown or "data" not in score:
                raise ValueError(f"score: a dict needs data=y_new and may give probs, predict and top (unknown keys "
                                 f"{sorted(unknown)})")
            if "top" in score and not score.get("predict"):
                raise ValueError("score: top needs predict=True")
            score = dict(data=score["data"], probs=score.get("probs", SC.DEFAULT_PROBS), predict=bool(score.get("predict")),
                         top=SC.check_top(score.get("top", SC.DEFAULT_TOP)))
        else:
            score = dict(data=score, probs=SC.DEFAULT_PROBS, predict=False, top=SC.DEFAULT_TOP)
        score["data"] = np.asfortranarray(SC.check_y_new(score["data"], y.shape[1]))
    if shape is not None and shape is not False:
        from . import shape as SH
        shape = SH.parse(shape)
    else:
        shape = None
    if sumscore is not None and sumscore is not False:
        from . import sumscore as SS
        sumscore = SS.parse(sumscore, m)
    else:
        sumscore = None
    if equate is not None:
        from . import equate as EQ
        equate = EQ.parse(equate, m)
    if loo is not None and loo is not False:
        from . import loo as LO
        loo = LO.parse(loo)
        LO.tail_length((1 if chains is None else int(chains)) * int(sample_iterations), loo["tail"])
    else:
        loo = None
    pairs = bins = dif = None
    if isinstance(ppc, dict):
        from . import ppc as P
        unknown = set(ppc) - {"pairs", "top", "bins", "bins_top", "dif"}
        if unknown:
            raise ValueError(f"ppc: a dict may give pairs, top, bins, bins_top and dif (unknown keys {sorted(unknown)})")
        if "top" in ppc and not ppc.get("pairs"):
            raise ValueError("ppc: top needs pairs=True")
        if ppc.get("pairs"):
            pairs = dict(top=P.check_pairs_top(ppc.get("top", P.DEFAULT_PAIRS_TOP)))
        want_bins = ppc.get("bins")
        want_bins = want_bins is not None and want_bins is not False
        if "bins_top" in ppc and not want_bins:
            raise ValueError("ppc: bins_top needs bins=True or bins=cuts")
        if want_bins:
            bins = dict(cuts=P.check_cuts(P.DEFAULT_CUTS if ppc["bins"] is True else ppc["bins"]),
                        top=P.check_bins_top(ppc.get("bins_top", P.DEFAULT_BINS_TOP)))
        if ppc.get("dif") is not None and ppc.get("dif") is not False:
            dif = ppc["dif"] if isinstance(ppc["dif"], dict) else dict(groups=ppc["dif"])
            unknown = set(dif) - {"groups", "cuts", "top"}
            if unknown or "groups" not in dif:
                raise ValueError(f"ppc: dif takes groups, cuts and top (unknown keys {sorted(unknown)})")
            codes, G = P.check_groups(dif["groups"], y.shape[0])
            dif = dict(groups=codes, G=G, cuts=P.check_cuts(P.DEFAULT_CUTS if dif.get("cuts") is None else dif["cuts"]),
                       top=P.check_dif_top(dif.get("top", P.DEFAULT_DIF_TOP)))
        ppc = True
    if (quantiles is not None or ppc or ranks is not None or score is not None or shape is not None or sumscore is not None
            or equate is not None or loo is not None):
        return _mcmc_run(y, chains, sample_iterations, burn_iterations, pm, ps, st, theta_init, rng, seed, rstream, preset,
                         theta_stabilise, fstar_fused, kstar_rank, device, progress, summaries, store_draws, align,
                         dict(quantiles=quantiles, ppc=bool(ppc), ranks=ranks, score=score, pairs=pairs, bins=bins, shape=shape,
                              sumscore=sumscore, dif=dif, equate=equate, loo=loo))
    if chains is not None:
        if rng == "reference":
            raise ValueError("chains need the item RNG (rng='item' or preset='fast')")
        return _mcmc_chains(y, int(chains), sample_iterations, burn_iterations, pm, ps, st, theta_init, seed, preset,
                            theta_stabilise, fstar_fused, kstar_rank, device, progress, summaries, store_draws, align)
    rs = None
    if rng == "reference":
        rs = rstream if rstream is not None else RStream(seed)
    if theta_init is None:                                           # R/gpirtMCMC.R:95-97
        if rs is not None:
            theta_init = rs.rnorm(n)
        else:
            theta_init = RStream(seed).rnorm(n)
    theta0 = np.ascontiguousarray(theta_init, dtype=np.float64)
    if theta0.shape != (n,):
        raise ValueError("theta_init must have one value per respondent")
    S, B = int(sample_iterations), int(burn_iterations)
    keep = _keep(store_draws)
    th = np.empty((S + 1, n), order="F") if "theta" in keep else None
    be = np.empty((2, m, S + 1), order="F") if "beta" in keep else None
    ff = np.empty((n, m, S + 1), order="F") if "f" in keep else None
    irf = np.empty((NGRID, m), order="F")
    o = _call_options(rng, seed, preset, theta_stabilise, fstar_fused, kstar_rank, device)

    def _tick(ctx, it, total):                                       # src/gpirtMCMC.cpp:64-66
        if progress:
            print("\r%6.3f %% complete" % (100.0 * it / max(total, 1)), end="", flush=True)
        return 0

    cb = _lib.TICK_FN(_tick)
    if summaries is None and len(keep) == 3:
        rc = lib.gpirt_mcmc(_ptr(y), n, m, _ptr(theta0), S, B, _ptr(pm), _ptr(ps), _ptr(st), C.byref(o),
                            rs.ptr if rs is not None else None, cb, None, _ptr(th), _ptr(be), _ptr(ff), _ptr(irf))
    else:
        parts = _lib.summary_parts(summaries if summaries is not None else 0)
        sm = _lib.Summary()
        sm.parts = parts
        arrays = _summary_arrays(parts, n, m)
        for k, a in arrays.items():
            setattr(sm, "h_" + k, _ptr(a))
        opt = lambda a: _ptr(a) if a is not None else None           # noqa: E731
        rc = lib.gpirt_mcmc_summary(_ptr(y), n, m, _ptr(theta0), S, B, _ptr(pm), _ptr(ps), _ptr(st), C.byref(o),
                                    rs.ptr if rs is not None else None, cb, None, opt(th), opt(be), opt(ff), _ptr(irf),
                                    C.byref(sm))
    if progress:
        print("\r100.000 % complete")
    if rc > 0:
        raise RuntimeError("chol(): decomposition failed")           # what arma::chol throws
    check(rc)
    out = dict(theta=th, beta=be, f=ff, IRFs=irf)
    if summaries is not None:
        out["summary"] = dict(arrays, totals=_totals(sm.totals))
    return out


def _ell_entry(kind, entry) -> str:
    """the library entry of a length-scale call for one of the two updates (_lib.ELL_KINDS)"""
    if kind not in _lib.ELL_KINDS:
        raise ValueError(f"ell: kind must be one of {_lib.ELL_KINDS}, not {kind!r}")
    return entry + ("_centred" if kind == "centred" else "")


def _keep(store_draws) -> set:
    if store_draws is True:
        return {"theta", "beta", "f"}
    if store_draws is False or store_draws is None:
        return set()
    keep = {store_draws} if isinstance(store_draws, str) else set(store_draws)
    if not keep <= {"theta", "beta", "f"}:
        raise ValueError("store_draws must be True, False or a subset of ('theta', 'beta', 'f')")
    return keep


def _chains_setup(y, nc, S, theta_init, rs, one, seed, summaries, store_draws, progress):
    """What gpirt_mcmc_chains and gpirt_mcmc_run take alike, as one namespace: th0 (theta_init as nc columns), the draw
    arrays th, be, ff (one: gpirt_mcmc's layout; else chain-major blocks of it), irf, the pooled summary's struct sm with its
    `arrays` and `parts`, the diagnostics' struct d with its arrays darr, and the tick cb."""
    from types import SimpleNamespace
    from . import chains as CH
    n, m = y.shape
    if theta_init is None:
        th0 = rs.rnorm(n)[None, :] if rs is not None else CH.default_inits(n, nc, seed)
    else:
        t = np.asarray(theta_init, dtype=np.float64)
        th0 = np.broadcast_to(t, (nc, n)) if t.shape == (n,) else t
        if th0.shape != (nc, n):
            raise ValueError("theta_init must be (n,) or (chains, n)")
    p = SimpleNamespace(one=one, progress=progress)
    p.th0 = np.ascontiguousarray(th0)                                # n x C column-major: chain c's column at c n
    keep = _keep(store_draws)
    if one:
        p.th = np.empty((S + 1, n), order="F") if "theta" in keep else None
        p.be = np.empty((2, m, S + 1), order="F") if "beta" in keep else None
        p.ff = np.empty((n, m, S + 1), order="F") if "f" in keep else None
    else:     # chain-major blocks, each in gpirt_mcmc's layout; the returned arrays are views with the chain first
        p.th = np.empty((nc, n, S + 1)) if "theta" in keep else None
        p.be = np.empty((nc, S + 1, m, 2)) if "beta" in keep else None
        p.ff = np.empty((nc, S + 1, m, n)) if "f" in keep else None
    p.irf = np.empty((NGRID, m), order="F")
    p.parts = _lib.summary_parts(summaries if summaries is not None else 0) | _lib.SUM_THETA_BETA
    p.sm = _lib.Summary()
    p.sm.parts = p.parts
    p.arrays = _summary_arrays(p.parts, n, m)
    for k, a in p.arrays.items():
        setattr(p.sm, "h_" + k, _ptr(a))
    p.d, p.darr = CH.diag_struct(p.parts, n, m, nc)

    def _tick(ctx, it, total):
        if progress:
            print("\r%6.3f %% complete" % (100.0 * it / max(total, 1)), end="", flush=True)
        return 0

    p.cb = _lib.TICK_FN(_tick)
    return p


def _chains_args(y, p, nc, S, B, pm, ps, st, o, align):
    """gpirt_mcmc_chains's twenty arguments (gpirt_mcmc_run's first twenty) from _chains_setup's namespace."""
    opt = lambda a: _ptr(a) if a is not None else None               # noqa: E731
    return (_ptr(y), y.shape[0], y.shape[1], _ptr(p.th0), nc, S, B, _ptr(pm), _ptr(ps), _ptr(st), C.byref(o),
            int(bool(align)), p.cb, None, opt(p.th), opt(p.be), opt(p.ff), _ptr(p.irf), C.byref(p.sm), C.byref(p.d))


def _chains_result(rc, p) -> dict:
    """The call's return code checked; the draws (the chain first unless p.one), the IRFs, the pooled summary and the
    diagnostics as gpirtMCMC returns them."""
    from . import chains as CH
    if p.progress:
        print("\r100.000 % complete")
    if rc > 0:
        raise RuntimeError("chol(): decomposition failed")
    check(rc)
    summary = dict(p.arrays)
    if p.parts & _lib.SUM_WAIC:
        summary["totals"] = _totals(p.sm.totals)
    th, be, ff = p.th, p.be, p.ff
    if not p.one:
        th = th.transpose(0, 2, 1) if th is not None else None
        be = be.transpose(0, 3, 2, 1) if be is not None else None
        ff = ff.transpose(0, 3, 2, 1) if ff is not None else None
    return dict(theta=th, beta=be, f=ff, IRFs=p.irf, summary=summary, diagnostics=CH.diag_result(p.d, p.darr))


def _mcmc_chains(y, nc, S, B, pm, ps, st, theta_init, seed, preset, theta_stabilise, fstar_fused, kstar_rank, device,
                 progress, summaries, store_draws, align):
    """gpirtMCMC(chains=C): gpirt_mcmc_chains (include/gpirt_hip.h)."""
    lib = _lib.load()
    S, B = int(S), int(B)
    if nc < 1:
        raise ValueError("chains must be >= 1")
    p = _chains_setup(y, nc, S, theta_init, None, False, seed, summaries, store_draws, progress)
    o = _call_options("item", seed, preset, theta_stabilise, fstar_fused, kstar_rank, device)
    return _chains_result(lib.gpirt_mcmc_chains(*_chains_args(y, p, nc, S, B, pm, ps, st, o, align)), p)


def _mcmc_run(y, nc, S, B, pm, ps, st, theta_init, rng, seed, rstream, preset, theta_stabilise, fstar_fused,
              kstar_rank, device, progress, summaries, store_draws, align, want):
    """gpirtMCMC with any of the analyses: gpirt_mcmc_run (include/gpirt_hip.h).  chains=None: one chain, its draws in
    gpirt_mcmc's layout; else stacked per chain as _mcmc_chains returns them.  `want` holds what gpirtMCMC parsed, None (ppc:
    False) for what is not asked for: quantiles (the probabilities), ppc (a bool), ranks (a dict), score (dict(data, probs,
    predict, top)), pairs (dict(top)), bins (dict(cuts, top)), dif (dict(groups, G, cuts, top)) -- those three need ppc --,
    shape, sumscore, equate and loo (the dicts of their modules' parse).  Every combination runs the same chains."""
    from . import equate as EQ
    from . import loo as LO
    from . import ppc as P
    from . import quantiles as Q
    from . import ranks as RK
    from . import score as SC
    from . import shape as SH
    from . import sumscore as SS
    from .ops import RStream
    lib = _lib.load()
    n, m = y.shape
    S, B = int(S), int(B)
    one = nc is None
    C_ = 1 if one else int(nc)
    if C_ < 1:
        raise ValueError("chains must be >= 1")
    rs = None
    if rng == "reference":
        if C_ != 1:
            raise ValueError("rng='reference' runs one chain; several chains need the item RNG")
        rs = rstream if rstream is not None else RStream(seed)
    p = _chains_setup(y, C_, S, theta_init, rs, one, seed, summaries, store_draws, progress)
    o = _call_options(rng, seed, preset, theta_stabilise, fstar_fused, kstar_rank, device)
    probs, ranks, score, pairs, bins, dif = (want[k] for k in ("quantiles", "ranks", "score", "pairs", "bins", "dif"))
    shape, sumscore, equate, loo = (want[k] for k in ("shape", "sumscore", "equate", "loo"))
    order = shape is not None and shape["order"]
    predict = score is not None and score["predict"]
    # name -> (the struct, its arrays), for what is wanted; the arrays live until the results are read
    made = {}
    if probs is not None:
        made["quantiles"] = Q.quantiles_struct(probs, n, m, C_)
    if want["ppc"]:
        made["ppc"] = P.struct(n, m)
    if ranks is not None:
        made["ranks"] = RK.struct(n, ranks.get("pivots", "median"), ranks.get("probs", RK.DEFAULT_PROBS),
                                  bool(ranks.get("pairwise", False)))
    if score is not None:
        made["score"] = SC.struct(score["data"].shape[0], score["probs"])
    if predict:
        made["predict"] = SC.predict_struct(score["data"].shape[0], m, score["top"])
    if pairs is not None:
        made["pairs"] = P.pairs_struct(m, pairs["top"])
    if bins is not None:
        made["bins"] = P.bins_struct(m, bins["cuts"], bins["top"])
    if shape is not None:
        made["shape"] = SH.struct(m, shape["k_half"], shape["tols"])
    if sumscore is not None:
        made["sumscore"] = SS.struct(m, int(sumscore["mask"].sum()), sumscore["mask"])
    if dif is not None:
        made["dif"] = P.dif_struct(m, dif["G"], dif["cuts"], dif["top"], groups=dif["groups"])
    if equate is not None:
        made["equate"] = EQ.struct(m, int(equate["mask_x"].sum()), int(equate["mask_y"].sum()), equate["mask_x"],
                                   equate["mask_y"])
    if loo is not None:
        made["loo"] = LO.struct(n, m, LO.tail_length(C_ * S, loo["tail"]), loo["top"], loo["tail"])
    if order:
        made["order"] = SH.order_struct(m, len(shape["tols"]), shape["order_top"])
    run = _lib.Run()
    run.rs = rs.ptr if rs is not None else None
    for name, (struct, _) in made.items():
        setattr(run, name, C.pointer(struct))
    if score is not None:
        run.h_y_new, run.n_new = _ptr(score["data"]), score["data"].shape[0]
    rc = lib.gpirt_mcmc_run(*_chains_args(y, p, C_, S, B, pm, ps, st, o, align), C.byref(run))
    out = _chains_result(rc, p)
    if probs is not None:
        out["quantiles"] = Q.quantiles_result(*made["quantiles"])
    if want["ppc"]:
        out["ppc"] = P.result(*made["ppc"])
        if pairs is not None:
            out["ppc"]["pairs"] = P.pairs_result(*made["pairs"])
        if bins is not None:
            out["ppc"]["bins"] = P.bins_result(*made["bins"])
        if dif is not None:
            out["ppc"]["dif"] = P.dif_result(*made["dif"])
    if ranks is not None:
        out["ranks"] = RK.result(*made["ranks"])
    if score is not None:
        out["score"] = SC.result(*made["score"])
        if predict:
            out["score"]["predict"] = SC.predict_result(*made["predict"])
    if shape is not None:
        out["shape"] = SH.result(*made["shape"], shape["probs"], shape["top"])
        if order:
            out["shape"]["order"] = SH.order_result(*made["order"])
    if sumscore is not None:
        out["sumscore"] = SS.result(*made["sumscore"], sumscore["probs"], y)
    if equate is not None:
        out["equate"] = EQ.result(*made["equate"], equate["probs"], equate["cuts"])
    if loo is not None:
        out["loo"] = LO.result(*made["loo"])
    return out


def _summary_arrays(parts: int, n: int, m: int) -> dict:
    """host arrays of every output of the summary parts `parts` (theta / beta moments with any part)"""
    names = []
    if parts:
        names += ["theta_mean", "theta_var", "beta_mean", "beta_var"]
    if parts & _lib.SUM_PRED:
        names += ["p_yes"]
    if parts & _lib.SUM_WAIC:
        names += ["lppd", "p_waic"]
    if parts & _lib.SUM_F:
        names += ["f_mean", "f_var"]
    shape = {"theta_mean": (n,), "theta_var": (n,), "beta_mean": (2, m), "beta_var": (2, m)}
    return {k: np.empty(shape.get(k, (n, m)), order="F") for k in names}


def _totals(raw) -> dict:
    return {k: float(raw[i]) for i, k in enumerate(_lib.SUM_TOTALS)}


class Sampler:
    """Stage-driven sampler (gpirt_sampler_*): device-resident state, one iteration per step().
    preset="fast": the options are gpirt_fast_options() (what bench.py's headline is timed with) with this call's seed,
    item0 / m_total and kernel_fp32; rng, theta_stabilise, fstar_fused, kstar_rank and factor_structured are then the preset's.
    factor_structured: where the steady iteration reads nothing else of the factor, a factorisation builds only L's diagonal
    parts and node rows, from theta (csrc/factor_lr.hip, gpirt_amd/factor_lr.py); get("L") and every other reader of the
    whole factor get the dense one, formed on demand."""

    def __init__(self, handle, y, theta_init, beta_prior_means=None, beta_prior_sds=None,
                 beta_proposal_sds=None, *, rng="item", seed=1, rstream=None, theta_stabilise=True,
                 fstar_fused=False, item0=0, m_total=0, kernel_fp32=False, kstar_rank=0, factor_structured=False, preset=None):
        self.lib = _lib.load()
        self.handle = handle
        y = _f64(y)
        self.n, self.m = y.shape
        m = self.m
        pm = _f64(np.zeros((2, m)) if beta_prior_means is None else beta_prior_means)
        ps = _f64(np.full((2, m), 3.0) if beta_prior_sds is None else beta_prior_sds)
        st = _f64(np.full((2, m), 0.1) if beta_proposal_sds is None else beta_proposal_sds)
        theta0 = np.ascontiguousarray(theta_init, dtype=np.float64)
        self.rs = rstream
        if preset == "fast":
            o = _lib.fast_options()
            o.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            o.device = -1 if handle.device is None else int(handle.device)
            o.item0, o.m_total, o.kernel_fp32 = int(item0), int(m_total), int(bool(kernel_fp32))
        elif preset is None:
            o = _options(rng, seed, theta_stabilise, fstar_fused, handle.device, item0, m_total, kernel_fp32, kstar_rank,
                         factor_structured)
        else:
            raise ValueError(f"unknown preset {preset!r}")
        s = C.c_void_p()
        check(self.lib.gpirt_sampler_create(C.byref(s), handle.ptr, _ptr(y), self.n, m, _ptr(theta0), _ptr(pm),
                                            _ptr(ps), _ptr(st), C.byref(o),
                                            rstream.ptr if rstream is not None else None))
        self._s = s
        handle._register(self)

    def close(self):
        """Destroy the device state.  Idempotent; Handle.close() closes the samplers still alive on it first, so no order of
        teardown (fixtures, garbage collection at interpreter exit) can leave a sampler draining a freed handle."""
        if getattr(self, "_s", None):
            self.lib.gpirt_sampler_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name):
        rc = getattr(self.lib, name)(self._s)
        if rc > 0:
            raise RuntimeError("chol(): decomposition failed (leading minor %d)" % rc)
        check(rc)

    def _state(self, entry, typestr="<i8"):
        """Torch view (on the device) of the ONE block that the stage entry `entry` (gpirt_sampler_*_state) hands out."""
        import torch
        p = C.c_void_p()
        nb = C.c_int64()
        check(getattr(self.lib, entry)(self._s, C.byref(p), C.byref(nb)))

        class _Wrap:
            pass

        w = _Wrap()
        w.__cuda_array_interface__ = {"shape": (nb.value // 8,), "typestr": typestr, "data": (p.value, False), "version": 2}
        return torch.as_tensor(w, device=f"cuda:{self.handle.device}")

    def _get_into(self, entry, name, out):
        """The array `name` of the stage entry `entry` (gpirt_sampler_*_get with a byte count) into the host array `out`."""
        check(getattr(self.lib, entry)(self._s, name.encode(), C.c_void_p(out.ctypes.data), out.nbytes))

    def init(self): self._call("gpirt_sampler_init")

    def step(self, consistent=False, nugget=True, scale=None):
        """One iteration.  The default is the reference's (gpirt_sampler_step): theta moves and f stays at the old theta.
        consistent=True: gpirt_sampler_step_consistent -- the same stages with carry_f(nugget) between theta_finish and
        draw_beta, so that f belongs to the new theta (gpirt_amd.consistent).  scale: the kinds of the collapsed move ("scale",
        "shift" or a tuple of them) proposed between theta_partial and theta_finish of a consistent step
        (gpirt_sampler_step_consistent_scale, after scale_enable()); None makes the calls it made before."""
        if scale is not None:
            if not consistent:
                raise ValueError("step: scale = ... needs consistent=True (the move is part of the consistent step)")
            kinds = 0
            for k in ((scale,) if isinstance(scale, str) else tuple(scale)):
                kinds |= 1 << self._scale_kind(k)
            rc = self.lib.gpirt_sampler_step_consistent_scale(self._s, int(nugget), kinds)
            if rc > 0:
                raise RuntimeError("chol(): decomposition failed (leading minor %d)" % rc)
            check(rc)
            self._last_step_consistent = True
            return
        if not consistent:
            self._last_step_consistent = False
            self._call("gpirt_sampler_step")
            return
        rc = self.lib.gpirt_sampler_step_consistent(self._s, int(nugget))
        if rc > 0:
            raise RuntimeError("chol(): decomposition failed (leading minor %d)" % rc)
        check(rc)
        self._last_step_consistent = True

    def carry_f(self, nugget=True):
        """The carry stage, behind theta_finish (or theta_commit) and in front of draw_beta: f[i, :] becomes the curve
        fstar - mu_star at respondent i's new grid point, plus the model's nugget sd_j z_ij with nugget=True (gpirt_sampler_carry_f;
        gpirt_amd.consistent.carry_exact is its NumPy statement).  Refused with the reason under rng="reference" and before
        init()."""
        check(self.lib.gpirt_sampler_carry_f(self._s, int(nugget)))

    def carry_stats(self) -> dict:
        """calls, and off_grid / nonfinite of the last carry and summed over the sampler's life (total_*): rows whose theta is
        no grid point (their f stays) and non-finite fstar cells carried; time_ms: the last carry's device time with
        enable_timing() on."""
        c = _lib.Carry()
        check(self.lib.gpirt_sampler_carry_stats(self._s, C.byref(c)))
        out = {k: int(getattr(c, k)) for k in _lib.CARRY_COUNTS}
        out["time_ms"] = float(c.last_ms)
        return out

    def prior_quad(self) -> np.ndarray:
        """The prior check, m values: || L^-1 f_j ||^2 / (n a_j^2) for the sampler's current factor and f (a_j: the item's
        amplitude, 1 when amplitudes are off).  Near 1 says f_j looks like a draw from its prior at the current theta, which is
        what an update that reads the prior density assumes; after the reference's step() it is in the hundreds.  Nothing of
        the chain moves; a structured factor is replaced by the dense one first (dense_factor_count moves by one)."""
        q = np.empty(self.m)
        rc = self.lib.gpirt_sampler_prior_quad(self._s, _ptr(q))
        if rc > 0:
            raise RuntimeError("chol(): decomposition failed (leading minor %d)" % rc)
        check(rc)
        a = self.amp_get("amplitude") if self.amp()["mode"] else 1.0
        return q / (float(self.n) * a * a)

    def draw_f(self): self._call("gpirt_sampler_draw_f")
    def draw_fstar(self): self._call("gpirt_sampler_draw_fstar")
    def theta_partial(self): self._call("gpirt_sampler_theta_partial")
    def theta_finish(self): self._call("gpirt_sampler_theta_finish")
    def theta_block(self): self._call("gpirt_sampler_theta_block")
    def theta_commit(self): self._call("gpirt_sampler_theta_commit")

    def set_theta_block(self, y_block, i0: int, m_total: int):
        """This rank's block of respondents with ALL item columns (item-sharded runs, include/gpirt_hip.h)."""
        yb = _f64(np.asfortranarray(y_block))
        check(self.lib.gpirt_sampler_set_theta_block(self._s, _ptr(yb), int(i0), int(yb.shape[0]), int(m_total)))
    def draw_beta(self): self._call("gpirt_sampler_draw_beta")
    def factor(self): self._call("gpirt_sampler_factor")
    def skip_factor(self): self._call("gpirt_sampler_skip_factor")

    def adopt_factor(self, rows_with_L: bool):
        """L arrived from elsewhere; rows_with_L: the whole ldl x n buffer (the bordered rows too) was received."""
        rc = self.lib.gpirt_sampler_adopt_factor(self._s, int(bool(rows_with_L)))
        check(rc)
    def build_cov(self): self._call("gpirt_sampler_build_cov")

    # -- the factorisation in pieces (distributed hosts, include/gpirt_hip.h "gpirt_potrf_panel_*"), on "L" in place
    @property
    def panel_width(self) -> int:
        return int(self.lib.gpirt_potrf_panel_width())

    @property
    def torch_device(self):
        import torch
        return torch.device("cuda", self.handle.device)

    @property
    def panel_rows(self) -> int:
        """rows of L's column blocks that travel with a panel (n, plus the rows of the bordered factorisation)"""
        r = C.c_int64()
        check(self.lib.gpirt_sampler_panel_rows(self._s, C.byref(r)))
        return r.value

    def panel_factor(self, p: int):
        check(self.lib.gpirt_sampler_panel_factor(self._s, int(p)))

    def panel_update(self, p: int, c: int):
        check(self.lib.gpirt_sampler_panel_update(self._s, int(p), int(c)))

    def panel_copy(self, p: int, buf, to_buf: bool):
        """rows [pW, panel_rows) of outer panel p <-> the dense torch buffer `buf` (what the host broadcasts)"""
        check(self.lib.gpirt_sampler_panel_copy(self._s, int(p), C.c_void_p(buf.data_ptr()), int(bool(to_buf))))

    # ... by halves of an outer panel (half: 0 first sub-panel, 1 the rest, 2 whole; part: 0 needs only the first
    # sub-panel, 1 the rest, 2 all): what the pipelined distributed factorisation drives (gpirt_amd/distributed.py)
    @property
    def subpanel_width(self) -> int:
        return int(self.lib.gpirt_potrf_subpanel_width(int(self.n)))

    def panel_factor_part(self, p: int, half: int):
        check(self.lib.gpirt_sampler_panel_factor_part(self._s, int(p), int(half)))

    def panel_update_part(self, p: int, c: int, part: int):
        check(self.lib.gpirt_sampler_panel_update_part(self._s, int(p), int(c), int(part)))

    def panel_copy_part(self, p: int, half: int, buf, to_buf: bool):
        check(self.lib.gpirt_sampler_panel_copy_part(self._s, int(p), int(half), C.c_void_p(buf.data_ptr()), buf.numel(),
                                                     int(bool(to_buf))))

    def streams_busy(self) -> int:
        """bit mask of the handle's internal streams with work in flight (0: every piece has joined the handle stream)"""
        b = C.c_int()
        check(self.lib.gpirt_debug_streams_busy(self.handle.ptr, C.byref(b)))
        return b.value

    @property
    def nu_lr_draws(self) -> int:
        """draws of draw_f that formed nu = L z from L's diagonal parts and the 64 node rows (csrc/nu_lr.hip)"""
        r = C.c_int64()
        check(self.lib.gpirt_sampler_nu_lr_draws(self._s, C.byref(r)))
        return r.value

    @property
    def ess_pack_draws(self) -> int:
        """draws of draw_f whose slice kernel read the packed y and formed mu from theta and beta (csrc/ess_lin.hip)"""
        r = C.c_int64()
        check(self.lib.gpirt_sampler_ess_pack_draws(self._s, C.byref(r)))
        return r.value

    @property
    def fstar_free_draws(self) -> int:
        """draw_fstar calls that took C = S^-1 K(theta, c) from theta alone, without the solve through L (csrc/fstar_free.hip)"""
        r = C.c_int64()
        check(self.lib.gpirt_sampler_fstar_free_draws(self._s, C.byref(r)))
        return r.value

    @property
    def factor_lr_count(self) -> int:
        """factorisations that built only L's diagonal parts and node rows, from theta (csrc/factor_lr.hip)"""
        r = C.c_int64()
        check(self.lib.gpirt_sampler_factor_lr_count(self._s, C.byref(r)))
        return int(r.value)

    @property
    def dense_factor_count(self) -> int:
        """dense factorisations this sampler has enqueued, those formed on demand behind a structured factor included"""
        r = C.c_int64()
        check(self.lib.gpirt_sampler_dense_factor_count(self._s, C.byref(r)))
        return int(r.value)

    def dense_factor(self):
        """the dense factor now, if L holds a structured one: for a caller who reads L through a device pointer it kept"""
        self._call("gpirt_sampler_dense_factor")

    def factor_lr_parts(self) -> list:
        """L's 512-column diagonal parts as they stand, in part order (w x w arrays), without forming the dense factor"""
        out = np.empty((self.n, 512), dtype=np.float64)
        check(self.lib.gpirt_sampler_factor_lr_parts(self._s, C.c_void_p(out.ctypes.data), out.size))
        return [out[p:p + 512, :min(512, self.n - p)].T.copy() for p in range(0, self.n, 512)]

    @property
    def factor_lr_width(self) -> int:
        """the width of the diagonal parts a structured L holds (GPIRT_FLR_NARROW); 0: L is dense"""
        r = C.c_int()
        check(self.lib.gpirt_sampler_factor_lr_width(self._s, C.byref(r)))
        return int(r.value)

    def factor_lr_blocks(self) -> list:
        """L's diagonal parts at the width it holds them, in part order (w x w arrays), as they lie: nothing is factored for it"""
        W = self.factor_lr_width
        out = np.empty((self.n, max(W, 1)), dtype=np.float64)
        check(self.lib.gpirt_sampler_factor_lr_blocks(self._s, C.c_void_p(out.ctypes.data), self.n * W))
        return [out[p:p + W, :min(W, self.n - p)].T.copy() for p in range(0, self.n, W)]

    def nu_lr_rows(self) -> np.ndarray:
        """the 64 node rows below the factor as they stand, 64 x n"""
        out = np.empty((64, self.n), order="F")
        check(self.lib.gpirt_sampler_nu_lr_rows(self._s, C.c_void_p(out.ctypes.data), out.size))
        return out

    def copy_state_from(self, other: "Sampler"):
        check(self.lib.gpirt_sampler_copy_state(self._s, other._s))

    def accumulate_irf(self): self._call("gpirt_sampler_accumulate_irf")
    def check(self): self._call("gpirt_sampler_check")

    @property
    def iteration(self) -> int:
        it = C.c_int()
        check(self.lib.gpirt_sampler_iteration(self._s, C.byref(it)))
        return it.value

    def set_iteration(self, it: int):
        check(self.lib.gpirt_sampler_set_iteration(self._s, int(it)))

    _SHAPES = {"theta": "n", "f": "nm", "beta": "2m", "mu": "nm", "mu_star": "Nm", "fstar": "Nm", "L": "nn",
               "logpost": "Nn", "irf_sum": "Nm", "s": "N", "mean": "Nm", "nu": "nm", "z": "nm", "y": "nm", "gbar": "Nm"}

    def _shape(self, name):
        n, m, N = self.n, self.m, NGRID
        return {"n": (n,), "nm": (n, m), "2m": (2, m), "Nm": (N, m), "nn": (n, n), "Nn": (N, n), "N": (N,)}[
            self._SHAPES[name]]

    def get(self, name: str) -> np.ndarray:
        if name == "ess_k":
            out = np.empty(self.m, dtype=np.int32)
            check(self.lib.gpirt_sampler_get(self._s, b"ess_k", C.c_void_p(out.ctypes.data), self.m))
            return out
        if name == "rs_stats":      # the predicted replay's counters (64-bit words; R-stream samplers only)
            out = np.zeros(8, dtype=np.int64)
            check(self.lib.gpirt_sampler_get(self._s, b"rs_stats", C.c_void_p(out.ctypes.data), 8))
            return out
        shape = self._shape(name)
        out = np.empty(shape, order="F")
        check(self.lib.gpirt_sampler_get(self._s, name.encode(), C.c_void_p(out.ctypes.data), out.size))
        return out

    def set(self, name: str, value):
        v = _f64(value)
        check(self.lib.gpirt_sampler_set(self._s, name.encode(), _ptr(v), v.size))

    def devptr(self, name: str):
        p = C.c_void_p()
        cnt = C.c_int64()
        check(self.lib.gpirt_sampler_devptr(self._s, name.encode(), C.byref(p), C.byref(cnt)))
        return p.value, cnt.value

    def device_tensor(self, name: str):
        """Zero-copy torch view of a state array (used to hand buffers to torch.distributed)."""
        import torch

        ptr, cnt = self.devptr(name)

        class _Wrap:
            pass

        w = _Wrap()
        w.__cuda_array_interface__ = {"shape": (cnt,), "typestr": "<f8", "data": (ptr, False), "version": 2}
        return torch.as_tensor(w, device=f"cuda:{self.handle.device}")

    def finish_irfs(self, sample_iterations: int) -> np.ndarray:
        out = np.empty((NGRID, self.m), order="F")
        check(self.lib.gpirt_sampler_finish_irfs(self._s, int(sample_iterations), _ptr(out)))
        return out

    # -- posterior summaries accumulated on the device (include/gpirt_hip.h gpirt_sampler_summary_*)
    def summary_enable(self, parts, planned_draws=None):
        """Allocate and zero the accumulators of `parts` (names or GPIRT_SUM_* bits; 0 / () frees them).  planned_draws: the
        chain's draw count S, fixed now -- the only way to turn on GPIRT_SUM_DIAG (split-R-hat / ESS, gpirt_amd.chains).
        ("theta_hist", "diag") with planned_draws also keeps DIAG's half histograms of theta: the rank-normalised R-hat
        of gpirt_amd.quantiles."""
        self._sum_parts = _lib.summary_parts(parts)
        if planned_draws is None:
            check(self.lib.gpirt_sampler_summary_enable(self._s, self._sum_parts))
        else:
            check(self.lib.gpirt_sampler_summary_enable_planned(self._s, self._sum_parts, int(planned_draws)))

    def summary_state(self):
        """Torch view (float64, on the device) of the ONE block that holds every accumulator of the summaries, its header
        and the IRF sum refreshed: what gpirt_amd.chains.combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_summary_state", "<f8")

    def summary_accumulate(self):
        """Add the current state (after a sampling iteration's step) as one draw."""
        self._call("gpirt_sampler_summary_accumulate")

    def summary_get(self, name: str) -> np.ndarray:
        """One finished array; with "theta_hist" / "irf_band" on also theta_hist, theta_hist_h1, theta_hist_h2 (1001 x n
        counts), theta_off_grid (n), irf_p_mean, irf_nan (1001 x m) and irf_band (256 x 1001 x m)."""
        n, m = self.n, self.m
        shape = {"theta_mean": (n,), "theta_var": (n,), "beta_mean": (2, m), "beta_var": (2, m), "theta_hist": (NGRID, n),
                 "theta_hist_h1": (NGRID, n), "theta_hist_h2": (NGRID, n), "theta_off_grid": (n,),
                 "irf_p_mean": (NGRID, m), "irf_nan": (NGRID, m), "irf_band": (NGRID, m, _lib.IRF_BINS)}.get(name, (n, m))
        out = np.empty(shape, order="F")
        check(self.lib.gpirt_sampler_summary_get(self._s, name.encode(), _ptr(out), out.size))
        return out.transpose(2, 0, 1) if name == "irf_band" else out

    def summary_totals(self) -> dict:
        raw = (C.c_double * len(_lib.SUM_TOTALS))()
        check(self.lib.gpirt_sampler_summary_totals(self._s, raw))
        return _totals(raw)

    def summary(self) -> dict:
        """Every array of the enabled parts, plus "totals" (with GPIRT_SUM_WAIC)."""
        parts = getattr(self, "_sum_parts", 0) & _lib.SUM_POOLED
        out = {k: self.summary_get(k) for k in _summary_arrays(parts, self.n, self.m)}
        if parts & _lib.SUM_WAIC:
            out["totals"] = self.summary_totals()
        return out

    # -- posterior predictive checks accumulated on the device (include/gpirt_hip.h gpirt_sampler_ppc_*, gpirt_amd.ppc)
    def ppc_enable(self, on=True):
        """Allocate and zero the PPC accumulators and count n_obs / obs_yes on the device (on=False frees them)."""
        check(self.lib.gpirt_sampler_ppc_enable(self._s, int(bool(on))))

    def ppc_accumulate(self):
        """Add the replicate of the current state (after a sampling iteration's step) as one draw; the chain is untouched."""
        self._call("gpirt_sampler_ppc_accumulate")

    def ppc_get(self, name: str) -> np.ndarray:
        """One finished field: "item_<field>" (m values) or "respondent_<field>" (n), field one of _lib.PPC_FIELDS."""
        out = np.empty(self.m if name.startswith("item_") else self.n)
        check(self.lib.gpirt_sampler_ppc_get(self._s, name.encode(), _ptr(out), out.size))
        return out

    def ppc_totals(self) -> dict:
        raw = (C.c_double * len(_lib.PPC_FIELDS))()
        check(self.lib.gpirt_sampler_ppc_totals(self._s, raw))
        return {k: float(raw[i]) for i, k in enumerate(_lib.PPC_FIELDS)}

    def ppc_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the PPC accumulators, its header refreshed: what
        gpirt_amd.ppc.combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_ppc_state")

    def ppc(self) -> dict:
        """Every field of the items and the respondents, the derived ppp_* values and "totals" (gpirt_amd.ppc.result's shape)."""
        from . import ppc as P
        out = {}
        tot = self.ppc_totals()
        for unit in ("item", "respondent"):
            d = {k: self.ppc_get(f"{unit}_{k}") for k in _lib.PPC_FIELDS}
            out[unit] = P.derive(d)
        out["totals"] = {k: float(v) for k, v in P.derive(dict(tot)).items()}
        return out

    # -- pairwise item checks inside the PPC (include/gpirt_hip.h gpirt_sampler_ppc_pairs_*, gpirt_amd.ppc)
    def ppc_pairs_enable(self, top=20, on=True):
        """Allocate and zero the pairwise accumulators on a sampler whose ppc_enable is on and form the constants n_co, o11,
        o1: from then on every ppc_accumulate also adds that draw's replicate to every item pair's 2 x 2 table statistics.
        top (1..64): how many extreme pairs ppc_pairs() lists.  on=False frees the state."""
        if not on:
            check(self.lib.gpirt_sampler_ppc_pairs_enable(self._s, 0))
            return
        from . import ppc as P
        self._pairs_top = P.check_pairs_top(top)
        check(self.lib.gpirt_sampler_ppc_pairs_enable(self._s, 1))

    def ppc_pairs_get(self, name: str) -> np.ndarray:
        """One array by name: a finished field (_lib.PAIRS_FIELDS; float64 m x m), sum_n11, sumsq_n11, sum_n1 (uint64),
        n11_ge, n11_gt, agree_ge, agree_gt, or_ge, or_gt (uint32), counts (int64: pair_draws, pair_skipped) and, of the last
        counted draw, rep (int8, n x m) and r11, r1 (int32, m x m).  Pair (a, b) is at [a, b]."""
        m = self.m
        if name == "counts":
            out = np.empty(2, dtype=np.int64)
        elif name == "rep":
            out = np.empty((self.n, m), dtype=np.int8, order="F")
        elif name in ("r11", "r1"):
            out = np.empty((m, m), dtype=np.int32)
        elif name in _lib.PAIRS_SUMS:
            out = np.empty((m, m), dtype=np.uint64)
        elif name in _lib.PAIRS_COUNTS:
            out = np.empty((m, m), dtype=np.uint32)
        else:
            out = np.empty((m, m))
        self._get_into("gpirt_sampler_ppc_pairs_get", name, out)
        return out

    def ppc_pairs_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the pairwise accumulators: what
        gpirt_amd.ppc.pairs_combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_ppc_pairs_state")

    def ppc_pairs(self, top=None) -> dict:
        """Every finished output of this sampler's pairwise accumulators (gpirt_amd.ppc.pairs_result's shape):
        gpirt_ppc_pairs_combine over its own state; top defaults to ppc_pairs_enable's."""
        from . import ppc as P
        return P.pairs_combine(self.handle, [self], top=getattr(self, "_pairs_top", P.DEFAULT_PAIRS_TOP) if top is None else top)

    # -- theta-binned item fit inside the PPC (include/gpirt_hip.h gpirt_sampler_ppc_bins_*, gpirt_amd.ppc)
    def ppc_bins_enable(self, cuts=None, top=20, on=True):
        """Allocate and zero the theta-binned accumulators on a sampler whose ppc_enable is on: from then on every
        ppc_accumulate also groups the respondents by the bin of that draw's theta and adds the replicate's and the data's yes
        counts, E and V per (bin, item).  cuts: the positive cut points (hundredths of theta, or theta values; default
        gpirt_amd.ppc.DEFAULT_CUTS); top (1..64): how many items ppc_bins() lists as worst.  on=False frees the state."""
        if not on:
            check(self.lib.gpirt_sampler_ppc_bins_enable(self._s, 0, None, 0))
            self._bins_cuts = ()
            return
        from . import ppc as P
        cuts = P.check_cuts(P.DEFAULT_CUTS if cuts is None else cuts)
        self._bins_top = P.check_bins_top(top)
        check(self.lib.gpirt_sampler_ppc_bins_enable(self._s, len(cuts), (C.c_int * len(cuts))(*cuts), 1))
        self._bins_cuts = cuts

    def ppc_bins_get(self, name: str) -> np.ndarray:
        """One array by name: a finished field (_lib.BINS_CELL_FIELDS: float64 B x m; BINS_ITEM_FIELDS: m; BINS_BIN_FIELDS: B),
        a raw array of _lib.BINS_RAW, cuts (int64), counts (int64: bin_draws, bin_skipped) and, of the last counted draw, bin
        (uint8, n), tN, tT, tR (int32, B x m) and tE, tV (float64, B x m).  Cell (b, j) is at [b, j]."""
        from . import ppc as P
        m, B = self.m, 2 * len(getattr(self, "_bins_cuts", ())) + 1      # (not enabled: the library refuses the call)
        raw = {r[0]: r for r in _lib.BINS_RAW}
        if name == "counts":
            out = np.empty(2, dtype=np.int64)
        elif name == "cuts":
            out = np.empty(max((B - 1) // 2, 1), dtype=np.int64)
        elif name == "bin":
            out = np.empty(self.n, dtype=np.uint8)
        elif name in ("tN", "tT", "tR"):
            out = np.empty((B, m), dtype=np.int32)
        elif name.lower() in raw:
            _, dt, kind = raw[name.lower()]
            out = np.empty(P._bins_shape(kind, m, B), dtype=P._BIN_DTYPES[dt])
        elif name in _lib.BINS_ITEM_FIELDS:
            out = np.empty(m)
        elif name in _lib.BINS_BIN_FIELDS:
            out = np.empty(B)
        else:
            out = np.empty((B, m))
        self._get_into("gpirt_sampler_ppc_bins_get", name, out)
        return out

    def ppc_bins_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the theta-binned accumulators: what
        gpirt_amd.ppc.bins_combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_ppc_bins_state")

    def ppc_bins(self, top=None, sign=1) -> dict:
        """Every finished output of this sampler's theta-binned accumulators (gpirt_amd.ppc.bins_result's shape):
        gpirt_ppc_bins_combine over its own state; top defaults to ppc_bins_enable's, sign = -1 reverses the bin axis."""
        from . import ppc as P
        return P.bins_combine(self.handle, [self], signs=[sign],
                              top=getattr(self, "_bins_top", P.DEFAULT_BINS_TOP) if top is None else top)

    # -- group-wise item fit inside the PPC (include/gpirt_hip.h gpirt_sampler_ppc_dif_*, gpirt_amd.ppc)
    def ppc_dif_enable(self, groups=None, cuts=None, top=20, on=True):
        """Allocate and zero the group-wise accumulators on a sampler whose ppc_enable is on: from then on every ppc_accumulate
        also stratifies the respondents by (group, bin of that draw's theta) and adds the Mantel-Haenszel, standardised
        difference, yes-count and chi-square statistics of the data and of the replicate.  groups: one code per respondent
        (-1 = left out, 0 = reference, 1..G-1 focal); cuts as for ppc_bins_enable; top (1..64): how many (item, group) pairs
        ppc_dif() flags.  on=False frees the state."""
        if not on:
            check(self.lib.gpirt_sampler_ppc_dif_enable(self._s, 0, None, 0, None, 0))
            self._dif_shape = None
            return
        from . import ppc as P
        codes, G = P.check_groups(groups, self.n)
        cuts = P.check_cuts(P.DEFAULT_CUTS if cuts is None else cuts)
        self._dif_top = P.check_dif_top(top)
        check(self.lib.gpirt_sampler_ppc_dif_enable(self._s, G, codes.ctypes.data_as(C.POINTER(C.c_int32)), len(cuts),
                                                    (C.c_int * len(cuts))(*cuts), 1))
        self._dif_shape = (G, 2 * len(cuts) + 1)

    def ppc_dif_get(self, name: str) -> np.ndarray:
        """One array by name: a finished field (_lib.DIF_CELL_FIELDS: float64 G x B x m; occupancy: G x B; DIF_GROUP_FIELDS and
        DIF_FOCAL_FIELDS: G x m), a raw array of _lib.DIF_RAW, cuts (int64), counts (int64: dif_draws, dif_skipped), groups
        (int8, n), group_size (int64, 4) and, of the last counted draw, cell (uint8, n), tN, tT, tR (int32, G x B x m), tE, tV
        (uint64, the fixed-point sums) and stats (float64, 8 x G x m)."""
        from . import ppc as P
        m = self.m
        G, B = getattr(self, "_dif_shape", None) or (2, 3)           # (not enabled: the library refuses the call)
        raw = {r[0]: r for r in _lib.DIF_RAW}
        if name == "counts":
            out = np.empty(2, dtype=np.int64)
        elif name == "cuts":
            out = np.empty((B - 1) // 2, dtype=np.int64)
        elif name == "group_size":
            out = np.empty(_lib.DIF_MAX_G, dtype=np.int64)
        elif name == "groups":
            out = np.empty(self.n, dtype=np.int8)
        elif name == "cell":
            out = np.empty(self.n, dtype=np.uint8)
        elif name in ("tN", "tT", "tR"):
            out = np.empty((G, B, m), dtype=np.int32)
        elif name in ("tE", "tV"):
            out = np.empty((G, B, m), dtype=np.uint64)
        elif name == "stats":
            out = np.empty((_lib.DIF_NSTATS, G, m))
        elif name.lower() in raw:
            _, dt, kind = raw[name.lower()]
            out = np.empty(P._dif_shape(kind, m, G, B), dtype=P._BIN_DTYPES[dt])
        elif name in _lib.DIF_CELL_FIELDS:
            out = np.empty((G, B, m))
        elif name == "occupancy":
            out = np.empty((G, B))
        else:
            out = np.empty((G, m))
        self._get_into("gpirt_sampler_ppc_dif_get", name, out)
        return out

    def ppc_dif_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the group-wise accumulators: what
        gpirt_amd.ppc.dif_combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_ppc_dif_state")

    def ppc_dif(self, top=None, sign=1) -> dict:
        """Every finished output of this sampler's group-wise accumulators (gpirt_amd.ppc.dif_result's shape):
        gpirt_ppc_dif_combine over its own state; top defaults to ppc_dif_enable's, sign = -1 reverses the bin axis."""
        from . import ppc as P
        return P.dif_combine(self.handle, [self], signs=[sign],
                             top=getattr(self, "_dif_top", P.DEFAULT_DIF_TOP) if top is None else top)

    # -- score-based checks inside the PPC (include/gpirt_hip.h gpirt_sampler_ppc_scores_*, gpirt_amd.ppc)
    def ppc_scores_enable(self, cuts=None, groups=9, top=20, on=True):
        """Allocate and zero the score-based accumulators on a sampler whose ppc_enable is on, and count the data's constants on
        the device: from then on every ppc_accumulate also adds the replicate's score distribution, every item's correlation
        with the rest score and the item fit within groups of the rest score.  Scores are raw counts over each respondent's own
        observed items.  cuts: ascending integers in 1 .. m - 1 (K - 1 of them, 2 <= K <= 16 groups; the group of a rest score w
        is #{k : c_k <= w}); None: up to `groups` groups from the quantiles of the data's total scores
        (gpirt_amd.ppc.default_score_cuts).  top (1..64): how many items ppc_scores() lists as worst.  on=False frees the state."""
        if not on:
            check(self.lib.gpirt_sampler_ppc_scores_enable(self._s, 0, None, 0))
            self._scores_K = None
            return
        from . import ppc as P
        self._scores_top = P.check_scores_top(top)
        cuts = P.check_score_cuts(P.default_score_cuts(self.get("y"), groups) if cuts is None else cuts, self.m, self.n)
        check(self.lib.gpirt_sampler_ppc_scores_enable(self._s, len(cuts) + 1, (C.c_int * len(cuts))(*cuts), 1))
        self._scores_K = len(cuts) + 1

    def ppc_scores_get(self, name: str) -> np.ndarray:
        """One array by name: a finished field (_lib.SCORES_HIST_FIELDS: float64 m + 1; SCORES_VAR_FIELDS: a 0-d float64;
        SCORES_ITEM_FIELDS: m; SCORES_CELL_FIELDS: K x m), a raw array or constant of _lib.SCORES_RAW, group_lo, group_hi (int64,
        K), cuts (int64, K - 1), counts (int64: score_draws, score_skipped), x_obs (int32, n) and, of the last counted draw,
        the arrays of _lib.SCORES_LAST.  An unknown name is a ValueError."""
        from . import ppc as P
        n, m = self.n, self.m
        K = getattr(self, "_scores_K", None) or 2                    # (not enabled: the library refuses the call)
        shape, dtype = P.scores_field(name, n, m, K)
        out = np.empty(shape, dtype=dtype)
        self._get_into("gpirt_sampler_ppc_scores_get", name, out)
        return out

    def ppc_scores_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the score-based accumulators: what
        gpirt_amd.ppc.scores_combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_ppc_scores_state")

    def ppc_scores(self, top=None) -> dict:
        """Every finished output of this sampler's score-based accumulators (gpirt_amd.ppc.scores_result's shape):
        gpirt_ppc_scores_combine over its own state; top defaults to ppc_scores_enable's."""
        from . import ppc as P
        return P.scores_combine(self.handle, [self], top=getattr(self, "_scores_top", P.DEFAULT_SCORES_TOP) if top is None else top)

    # -- person fit inside the PPC (include/gpirt_hip.h gpirt_sampler_ppc_person_*, gpirt_amd.ppc)
    def ppc_person_enable(self, order=None, cuts=None, groups=5, top=20, on=True):
        """Allocate and zero the person-fit accumulators on a sampler whose ppc_enable is on, and count the data's constants on
        the device: from then on every ppc_accumulate also adds every respondent's Guttman errors, lz and person response
        function (the yes rate within groups of the items' easiness) of the replicate.  order: a permutation of 0 .. m - 1, the
        easiest item first; None: by the data's yes rate (gpirt_amd.ppc.default_item_order).  cuts: ascending integers in 1 .. m -
        1 that act on the POSITIONS in that order (K - 1 of them, 2 <= K <= 16 groups; position t lies in group #{k : c_k <=
        t}); None: `groups` groups of near-equal size (gpirt_amd.ppc.default_item_cuts).  top (1..64): how many respondents
        ppc_person() lists as worst.  on=False frees the state.  Stage API only: gpirtMCMC has no keyword for it."""
        if not on:
            check(self.lib.gpirt_sampler_ppc_person_enable(self._s, 0, None, None, 0))
            self._person_K = None
            return
        from . import ppc as P
        self._person_top = P.check_person_top(top)
        order, cuts = P.check_person_args(P.default_item_order(self.get("y")) if order is None else order,
                                          P.default_item_cuts(self.m, groups) if cuts is None else cuts, self.m, self.n)
        check(self.lib.gpirt_sampler_ppc_person_enable(self._s, len(cuts) + 1, order.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       (C.c_int * len(cuts))(*cuts), 1))
        self._person_K = len(cuts) + 1

    def ppc_person_get(self, name: str) -> np.ndarray:
        """One array by name: a finished field (_lib.PERSON_RESP_FIELDS: float64 n; PERSON_CELL_FIELDS: K x n), a raw array or
        constant of _lib.PERSON_RAW, group_lo, group_hi (int64, K), group_items, order (int32, m), cuts (int64, K - 1), counts
        (int64: person_draws, person_skipped) and, of the last counted draw, the arrays of _lib.PERSON_LAST.  An unknown name is
        a ValueError."""
        from . import ppc as P
        K = getattr(self, "_person_K", None) or 2                    # (not enabled: the library refuses the call)
        shape, dtype = P.person_field(name, self.n, self.m, K)
        out = np.empty(shape, dtype=dtype)
        self._get_into("gpirt_sampler_ppc_person_get", name, out)
        return out

    def ppc_person_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the person-fit accumulators: what
        gpirt_amd.ppc.person_combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_ppc_person_state")

    def ppc_person(self, top=None) -> dict:
        """Every finished output of this sampler's person-fit accumulators (gpirt_amd.ppc.person_result's shape):
        gpirt_ppc_person_combine over its own state; top defaults to ppc_person_enable's."""
        from . import ppc as P
        return P.person_combine(self.handle, [self], top=getattr(self, "_person_top", P.DEFAULT_PERSON_TOP) if top is None else top)

    # -- residual correlations inside the PPC (include/gpirt_hip.h gpirt_sampler_ppc_resid_*, gpirt_amd.ppc)
    def ppc_resid_enable(self, top=20, on=True):
        """Allocate and zero the residual-correlation accumulators on a sampler whose ppc_enable is on and form O and n_co: from
        then on every ppc_accumulate also adds that draw's residual correlations of every item pair, every item's infit and
        share in the dependence, and the global statistics Q, M+ and M, for the data and the replicate.  top (1..64): how many
        pairs and items ppc_resid() lists as worst.  on=False frees the state.  Stage API only: gpirtMCMC has no keyword for it."""
        if not on:
            check(self.lib.gpirt_sampler_ppc_resid_enable(self._s, 0))
            return
        top = int(top) if int(top) == top and top != 0 else -1          # (0 frees the state in C; the library names the fault)
        check(self.lib.gpirt_sampler_ppc_resid_enable(self._s, top))
        self._resid_top = top

    def ppc_resid_get(self, name: str) -> np.ndarray:
        """One array by name: a finished field (_lib.RESID_PAIR_FIELDS: float64 m x m; RESID_ITEM_FIELDS: m), "scalars" (float64,
        13, in _lib.RESID_SCALARS' order), a raw array of _lib.RESID_RAW, counts (int64: resid_draws, resid_skipped,
        global_undefined) and, of the last counted draw, the arrays of _lib.RESID_LAST.  Pair (a, b) is at [a, b]; d_obs, d_rep
        and w are n x m, digits is 9 x n x m.  An unknown name is refused by the library."""
        from . import ppc as P
        shape, dtype, order = P.resid_field(name, self.n, self.m)
        out = np.empty(shape, dtype=dtype, order=order)
        self._get_into("gpirt_sampler_ppc_resid_get", name, out)
        return out.transpose(0, 2, 1) if name == "digits" else out

    def ppc_resid_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the residual-correlation accumulators: what
        gpirt_amd.ppc.resid_combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_ppc_resid_state")

    def ppc_resid(self, top=None) -> dict:
        """Every finished output of this sampler's residual-correlation accumulators (gpirt_amd.ppc.resid_result's shape):
        gpirt_ppc_resid_combine over its own state; top defaults to ppc_resid_enable's."""
        from . import ppc as P
        return P.resid_combine(self.handle, [self], top=getattr(self, "_resid_top", P.DEFAULT_RESID_TOP) if top is None else top)

    # -- rank posteriors accumulated on the device (include/gpirt_hip.h gpirt_sampler_rank_*, gpirt_amd.ranks)
    def rank_enable(self, on=True, pivots="median", pairwise=False):
        """Allocate and zero the rank accumulators for `pivots` ("median" and / or positions in 1..n, at most 16; the
        library closes the set under q <-> n + 1 - q); pairwise=True keeps lt (4 n^2 bytes).  on=False frees them."""
        if not on:
            check(self.lib.gpirt_sampler_rank_enable(self._s, None, -1, 0))
            return
        from . import ranks as RK
        given, _ = RK.close_pivots(self.n, pivots)
        arr = (C.c_int64 * max(len(given), 1))(*given)
        check(self.lib.gpirt_sampler_rank_enable(self._s, arr, len(given), int(bool(pairwise))))

    def rank_accumulate(self):
        """Add the ranks of the current theta (after a sampling iteration's step) as one draw; the chain is untouched."""
        self._call("gpirt_sampler_rank_accumulate")

    def rank_get(self, name: str) -> np.ndarray:
        """One array by name: rank2_sum, rank2_sumsq (uint64, n), rank_hist (uint32, n x B), pivot_cover (uint32, P x n),
        pivot_share, p_pivot (P x n), rank_mean, rank_var (n), pivots (int64, P), lt (uint32, n x n),
        counts (int64: draws, skipped, B, w, P)."""
        c = np.zeros(5, dtype=np.int64)
        self._get_into("gpirt_sampler_rank_get", "counts", c)                                    # the header alone
        n, B, P = self.n, int(c[2]), int(c[4])
        shapes = dict(counts=((5,), np.int64), rank2_sum=((n,), np.uint64), rank2_sumsq=((n,), np.uint64),
                      rank_hist=((n, B), np.uint32), pivot_cover=((P, n), np.uint32), pivot_share=((P, n), np.float64),
                      p_pivot=((P, n), np.float64), rank_mean=((n,), np.float64), rank_var=((n,), np.float64),
                      pivots=((P,), np.int64), lt=((n, n), np.uint32))
        if name == "counts":
            return c
        shape, dt = shapes.get(name, ((0,), np.float64))
        out = np.empty(shape, dtype=dt)
        self._get_into("gpirt_sampler_rank_get", name, out)
        return out

    def rank_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the rank accumulators: what
        gpirt_amd.ranks.combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_rank_state")

    def ranks(self, probs=(0.025, 0.5, 0.975)) -> dict:
        """Every finished output of this sampler's accumulators (gpirt_amd.ranks.result's shape): gpirt_rank_combine
        over its own state, nothing reflected."""
        from . import ranks as RK
        return RK.combine(self.handle, [self], probs=probs)

    # -- shape posteriors of the item response curves (include/gpirt_hip.h gpirt_sampler_shape_*, gpirt_amd.shape)
    def shape_enable(self, window=3.0, tols=(0.0, 0.25, 1.0), on=True):
        """Allocate and zero the shape accumulators for the window |theta| <= window (0.01..5.0) and up to 4 tolerances
        (logits, >= 0); from the next draw_fstar on the sampler array "gbar" holds the draw's smooth curve.  on=False frees
        them."""
        if not on:
            check(self.lib.gpirt_sampler_shape_enable(self._s, 0, None, 0, 0))
            self._shape_ntols = 0
            return
        from . import shape as SH
        k_half, tols = SH.check_window(window), SH.check_tols(tols)
        check(self.lib.gpirt_sampler_shape_enable(self._s, k_half, (C.c_double * len(tols))(*tols), len(tols), 1))
        self._shape_ntols = len(tols)

    def shape_accumulate(self):
        """Add the current "gbar" (after a sampling iteration's step) as one draw; the chain is untouched."""
        self._call("gpirt_sampler_shape_accumulate")

    def shape_get(self, name: str) -> np.ndarray:
        """One array by name, in gpirt_amd.shape's layout ([k, j] arrays as 1001 x m): cls (n_tols x 4 x m), peak_hist,
        valley_hist, cross_first_hist, cross_last_hist (uint32), cross_count (4 x m), draws, nonfinite (m), slope (4 x m),
        info_sum, ti_sum, ti_sumsq, rel (2), counts (int64: info_draws, info_skipped), tols, and of the last draw info
        (1001 x m) and ti (1001)."""
        from . import shape as SH
        m, nt = self.m, getattr(self, "_shape_ntols", 0)                 # (not enabled: the library refuses the call)
        dts = dict(_lib.SHAPE_RAW)
        if name in dts:
            out = np.empty(SH._raw_shape(name, m), dtype=np.dtype(dts[name]))
        elif name == "counts":
            out = np.empty(2, dtype=np.int64)
        else:
            out = np.empty({"tols": (_lib.SHAPE_MAX_TOLS,), "info": (m, NGRID), "ti": (NGRID,)}.get(name, (0,)))
        self._get_into("gpirt_sampler_shape_get", name, out)
        if name == "tols":
            return out[:nt]
        return out.T if name == "info" else SH._public(name, out, nt)

    # -- item-pair order posteriors on top of the shape block (include/gpirt_hip.h gpirt_sampler_shape_order_*, gpirt_amd.shape)
    def shape_order_enable(self, on=True):
        """Allocate and zero the item-pair order block beside the shape accumulators (after shape_enable(); 2 <= m <= 4096):
        from then on shape_accumulate() also runs the order kernels on the same curves.  on=False frees it; shape_enable()
        drops it with the shape state."""
        check(self.lib.gpirt_sampler_shape_order_enable(self._s, 1 if on else 0))

    def shape_order_get(self, name: str) -> np.ndarray:
        """One array by name: above, cross (n_tols x m x m, uint32), easier (m x m), depth_sum (m x m), easiness (2 x m),
        set_counts (3 x n_tols, uint64: iio_draws, cross_pairs_sum, cross_pairs_sumsq), counts (int64: draws, skipped) and, of
        the last counted draw, u (m x m), e (m) and ncross (n_tols, int64)."""
        from . import shape as SH
        m, nt = self.m, getattr(self, "_shape_ntols", 0)                 # (not enabled: the library refuses the call)
        dts = dict(_lib.ORDER_RAW)
        if name in dts:
            out = np.empty(SH._order_raw_shape(name, m, nt), dtype=np.dtype(dts[name]))
        elif name in ("counts", "ncross"):
            out = np.empty(2 if name == "counts" else _lib.SHAPE_MAX_TOLS, dtype=np.int64)
        else:
            out = np.empty({"u": (m, m), "e": (m,)}.get(name, (0,)))
        self._get_into("gpirt_sampler_shape_order_get", name, out)
        if name == "ncross":
            return out[:nt]
        return out[:, :nt] if name == "set_counts" else out

    def shape_order_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the order accumulators: what
        gpirt_amd.shape.order_combine pools."""
        return self._state("gpirt_sampler_shape_order_state")

    def shape_order(self, top=20) -> dict:
        """Every finished output of this sampler's order block (gpirt_amd.shape.order_finish's dict)."""
        from . import shape as SH
        return SH.order_combine(self.handle, [self], top=top)

    def shape_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the shape accumulators: what
        gpirt_amd.shape.combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_shape_state")

    def shape(self, probs=(0.025, 0.5, 0.975), top=20, sign=1) -> dict:
        """Every finished output of this sampler's accumulators (gpirt_amd.shape.finish's dict): gpirt_shape_combine over
        its own state; sign = -1 reflects it."""
        from . import shape as SH
        return SH.combine(self.handle, [self], signs=[sign], probs=probs, top=top)

    # -- sum-score posteriors (include/gpirt_hip.h gpirt_sampler_sumscore_*, gpirt_amd.sumscore)
    def sumscore_enable(self, items=None, on=True):
        """Allocate and zero the sum-score accumulators for the form `items` (None: all m items; column indices or a boolean
        mask; 1..4096 items -- a wrong index, an empty form and a longer one are ValueErrors).  on=False frees them."""
        if not on:
            check(self.lib.gpirt_sampler_sumscore_enable(self._s, None, 0))
            self._sumscore_M = 0
            return
        from . import sumscore as SS
        mask = SS.form_mask(items, self.m)
        check(self.lib.gpirt_sampler_sumscore_enable(self._s, C.c_void_p(mask.ctypes.data), 1))
        self._sumscore_M = int(mask.sum())

    def sumscore_accumulate(self):
        """Add the current "fstar" (after a sampling iteration's step) as one draw; the chain is untouched."""
        self._call("gpirt_sampler_sumscore_accumulate")

    def sumscore_get(self, name: str) -> np.ndarray:
        """One array by name: joint_sum, last (1001 x (M + 1)), pi_sum, pi_sumsq, last_pi (M + 1), tcc_sum, tcc_sumsq, var_sum,
        w (1001), rel (2), mask (uint8, m), counts (int64: draws, skipped, rel_draws, rel_skipped), and of the last counted
        draw tcc and var (1001)."""
        from . import sumscore as SS
        m, M = self.m, getattr(self, "_sumscore_M", 0)                   # (not enabled: the library refuses the call)
        dts = dict(_lib.SUMSCORE_RAW)
        if name in dts:
            out = np.empty(SS._raw_shape(name, m, M), dtype=np.dtype(dts[name]))
        elif name == "counts":
            out = np.empty(4, dtype=np.int64)
        else:
            out = np.empty({"tcc": (NGRID,), "var": (NGRID,)}.get(name, (0,)))
        self._get_into("gpirt_sampler_sumscore_get", name, out)
        return out

    def sumscore_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the sum-score accumulators: what
        gpirt_amd.sumscore.combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_sumscore_state")

    def sumscore(self, probs=(0.025, 0.5, 0.975), sign=1, y=None) -> dict:
        """Every finished output of this sampler's accumulators (gpirt_amd.sumscore.finish's dict): gpirt_sumscore_combine
        over its own state; sign = -1 reverses its k axis; y (the data): also the observed score histogram."""
        from . import sumscore as SS
        return SS.combine(self.handle, [self], signs=[sign], probs=probs, y=y)

    # -- two-form score equating (include/gpirt_hip.h gpirt_sampler_equate_*, gpirt_amd.equate)
    def equate_enable(self, x=None, y=None, on=True):
        """Allocate and zero the equating accumulators for the disjoint forms `x` and `y` (column indices or boolean masks;
        1..2048 items each -- an empty form, a longer one and a column in both are ValueErrors).  on=False frees them."""
        if not on:
            check(self.lib.gpirt_sampler_equate_enable(self._s, None, None, 0))
            self._equate_M = (0, 0)
            return
        from . import equate as EQ
        mx, my = EQ.form_masks(x, y, self.m)
        check(self.lib.gpirt_sampler_equate_enable(self._s, C.c_void_p(mx.ctypes.data), C.c_void_p(my.ctypes.data), 1))
        self._equate_M = (int(mx.sum()), int(my.sum()))

    def equate_accumulate(self):
        """Add the current "fstar" (after a sampling iteration's step) as one draw; the chain is untouched."""
        self._call("gpirt_sampler_equate_accumulate")

    def equate_get(self, name: str) -> np.ndarray:
        """One array by name: joint_sum, last_joint ((M_X + 1) x (M_Y + 1)), pix_sum, pix_sumsq, last_pix, eyx_sum, eyx_sumsq,
        last_eyx (M_X + 1), piy_sum, piy_sumsq, last_piy, exy_sum, exy_sumsq, last_exy (M_Y + 1), corr (2), corr_terms (5), w
        (1001), mask_x, mask_y (uint8, m) and counts (int64: draws, skipped, corr_draws, corr_skipped, eq_clamped)."""
        from . import equate as EQ
        Mx, My = getattr(self, "_equate_M", (0, 0))                      # (not enabled: the library refuses the call)
        dts = dict(_lib.EQUATE_RAW)
        if name in dts:
            out = np.empty(EQ._raw_shape(name, self.m, Mx, My), dtype=np.dtype(dts[name]))
        elif name == "counts":
            out = np.empty(5, dtype=np.int64)
        else:
            out = np.empty(0)
        self._get_into("gpirt_sampler_equate_get", name, out)
        return out

    def equate_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the equating accumulators: what
        gpirt_amd.equate.combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_equate_state")

    def equate(self, probs=(0.025, 0.5, 0.975), cuts=None) -> dict:
        """Every finished output of this sampler's accumulators (gpirt_amd.equate.finish's dict): gpirt_equate_combine over
        its own state."""
        from . import equate as EQ
        return EQ.combine(self.handle, [self], probs=probs, cuts=cuts)

    # -- PSIS-LOO (include/gpirt_hip.h gpirt_sampler_loo_*, gpirt_amd.loo)
    def loo_enable(self, planned_draws=None, tail=None, on=True):
        """Allocate and zero the LOO state for `planned_draws` draws pooled over ALL chains (T) and the tail rule, or `tail`
        (5 .. 1024) keys; a bad tail, a tail of more than 1024 keys and one that T draws cannot fill are ValueErrors.  on=False
        frees it."""
        if not on:
            check(self.lib.gpirt_sampler_loo_enable(self._s, 0, 0, 0))
            self._loo_M = None
            return
        from . import loo as LO
        M = LO.tail_length(planned_draws, tail)
        check(self.lib.gpirt_sampler_loo_enable(self._s, int(planned_draws), 0 if tail is None else int(tail), 1))
        self._loo_M = M

    def loo_accumulate(self):
        """Enter the current f + mu (after a sampling iteration's step) as one draw; the chain is untouched."""
        self._call("gpirt_sampler_loo_accumulate")

    def loo_get(self, name: str) -> np.ndarray:
        """One array by name: keys (K x n x m, each cell's min-heap, slot 0 the smallest kept key), evicted_sum, evicted_sumsq,
        p_sum (n x m), count, nonfinite (int32), y (int8), counts (int64: n, m, T, M, draws, chains) and tail: the kept keys in
        descending order per cell (K x n x m, NaN where fewer than K keys are held)."""
        from . import loo as LO
        if name == "tail":
            return LO.sorted_tail(self.loo_get("keys"), self.loo_get("count"))
        M = getattr(self, "_loo_M", None) or 0                           # (not enabled: the library refuses the call)
        dts = dict(_lib.LOO_RAW)
        if name in dts:
            out = np.empty(LO._raw_shape(name, self.n, self.m, M), dtype=np.dtype(dts[name]))
        elif name == "counts":
            out = np.empty(6, dtype=np.int64)
        else:
            out = np.empty(0)
        self._get_into("gpirt_sampler_loo_get", name, out)
        if name == "keys":
            return out.transpose(0, 2, 1)
        return out.T if name in dts else out

    def loo_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the LOO state: what gpirt_amd.loo.combine pools."""
        return self._state("gpirt_sampler_loo_state")

    def loo(self, top=20) -> dict:
        """Every finished output of this sampler's state (gpirt_amd.loo.result's dict): gpirt_loo_combine over it alone."""
        from . import loo as LO
        return LO.combine(self.handle, [self], top=top)

    # -- autocorrelation ESS (include/gpirt_hip.h gpirt_sampler_acf_*, gpirt_amd.acf)
    def acf_enable(self, parts="all", planned_draws=None, max_lag=None, on=True):
        """Allocate and zero the autocorrelation state for this chain's `planned_draws` draws (S, fixed now, as DIAG's) and the
        series `parts` (GPIRT_ACF_* bits, names of ("theta", "beta", "ll") or "all").  max_lag: L, 1 .. min(S // 2 - 1, 1024);
        None: min(S // 2 - 1, 256).  No planned draws, halves of fewer than 4 draws and a lag window the halves cannot fill are
        ValueErrors.  on=False frees the state.  Stage API only: gpirtMCMC has no keyword for it (gpirt_amd.acf.run is the
        one-call way in)."""
        if not on:
            check(self.lib.gpirt_sampler_acf_enable(self._s, 0, 0, 0, 0))
            self._acf = None
            return
        from . import acf as AC
        mask = AC.parts_mask(parts)
        L = AC.lag_window(planned_draws, max_lag)
        check(self.lib.gpirt_sampler_acf_enable(self._s, mask, int(planned_draws), 0 if max_lag is None else int(max_lag), 1))
        self._acf = (mask, L, AC.n_values(self.n, self.m, mask))

    def acf_accumulate(self):
        """Enter the current theta, beta and f + mu (after a sampling iteration's step) as the chain's next draw; one beyond
        the planned draws is an error.  The chain is untouched."""
        self._call("gpirt_sampler_acf_accumulate")

    def acf_get(self, name: str) -> np.ndarray:
        """One array by name: s, head, tail (2 x (L + 1) x P), sum (2 x P), ring ((L + 1) x P), centre, last (P; float64),
        nonfinite (int64, P) -- theta's integer columns come back as float64, exactly -- and counts (int64: n, m, parts, S, H, L,
        P, draws)."""
        from . import acf as AC
        mask, L, P = getattr(self, "_acf", None) or (0, 0, 1)           # (not enabled: the library refuses the call)
        if name == "counts":
            out = np.empty(8, dtype=np.int64)
        else:
            out = np.empty(AC.raw_shape(name, P, L), dtype=np.int64)
        self._get_into("gpirt_sampler_acf_get", name, out)
        if name == "counts":
            return out
        return AC.decode_raw(name, out, 0 if name == "last" or not mask & _lib.ACF_THETA else self.n)

    def acf_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the autocorrelation state: what gpirt_amd.acf.combine
        finishes."""
        return self._state("gpirt_sampler_acf_state")

    def acf(self, top=20, sign=1) -> dict:
        """Every finished output of this sampler's state alone (gpirt_amd.acf.result's dict): gpirt_acf_combine over it with
        `sign` (+1, or -1 for the reflected chain)."""
        from . import acf as AC
        return AC.combine(self.handle, [self], signs=[sign], top=top)

    # -- group posteriors (include/gpirt_hip.h gpirt_sampler_groups_*, gpirt_amd.groups)
    def groups_enable(self, groups=None, top=20, on=True):
        """Allocate and zero the group posterior state: from then on every groups_accumulate() enters the current theta and
        f + mu as a draw of the groups' separation, overlap, medians, party-line votes and loyalty.  groups: one code per
        respondent (-1 = left out, 0 .. G - 1; 2 <= G <= 8, every group with a member); top (1..64): the length of the two lists
        groups() gives.  Refusals are ValueErrors that say which.  on=False frees the state.  Stage API only: gpirtMCMC has no
        keyword for it (gpirt_amd.groups.run is the one-call way in)."""
        if not on:
            check(self.lib.gpirt_sampler_groups_enable(self._s, 0, None, 0, 0))
            self._groups = None
            return
        from . import groups as GR
        codes, G = GR.check_groups(groups, self.n, self.m)
        top = GR.check_top(top)
        check(self.lib.gpirt_sampler_groups_enable(self._s, G, codes.ctypes.data_as(C.POINTER(C.c_int32)), top, 1))
        self._groups = (codes, G, top)

    def groups_accumulate(self):
        """Enter the current theta and f + mu (after a sampling iteration's step) as the next draw.  Nothing is drawn and the
        chain is untouched; a draw with an included theta off the grid is skipped for the latent part, one with a NaN f + mu
        for the vote part."""
        self._call("gpirt_sampler_groups_accumulate")

    def groups_get(self, name: str) -> np.ndarray:
        """One array by name: an accumulator of _lib.GROUPS_RAW, a constant (counts: int64 latent_draws, latent_skipped,
        votes_draws, votes_skipped; group_size: int64, 9; groups: int8, n) or a table of the last counted draw
        (_lib.GROUPS_LAST: hist, c1, c2, med2, w, ov, latent_stats, e, side, split, contested, n_split, c_g, loy, obs_with,
        obs_n)."""
        from . import groups as GR
        _, G, _ = getattr(self, "_groups", None) or (None, 2, 1)        # (not enabled: the library refuses the call)
        for nm, dt, key in _lib.GROUPS_RAW + _lib.GROUPS_LAST:
            if nm == name:
                out = np.empty(GR.raw_shape(key, self.n, self.m, G), dtype=GR._DT[dt])
                break
        else:
            raise ValueError(f"groups_get: unknown array '{name}'")
        self._get_into("gpirt_sampler_groups_get", name, out)
        return out

    def groups_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the group posterior state: what
        gpirt_amd.groups.combine pools."""
        return self._state("gpirt_sampler_groups_state")

    def groups(self, sign=1, top=None) -> dict:
        """Every finished output of this sampler's state alone (gpirt_amd.groups.finish's dict): gpirt_groups_combine over it
        with `sign` (+1, or -1 for the reflected chain)."""
        from . import groups as GR
        g = getattr(self, "_groups", None)
        return GR.combine(self.handle, [self], signs=[sign], top=(g[2] if g else 20) if top is None else top)

    # -- the kernel's length scale as a parameter of the chain (include/gpirt_hip.h gpirt_sampler_ell_*, gpirt_amd.ell)
    def ell_enable(self, lo=0.25, hi=4.0, points=129, log_prior=None, width=4, k0=None, on=True):
        """Put the length scale on the logarithmic grid ell_k = lo (hi / lo)^(k / (points - 1)) with the prior mass log_prior
        (`points` finite values; None: -(ln ell_k)^2 / 2) and the proposal width `width` (1 .. points - 1), start the chain
        at index k0 (None: the index of the length scale the sampler has) and factor under ell_k0.  After init().  Refused
        with the reason: rng="reference", kernel_fp32, an item shard, a length scale that is not on the grid, a kstar_rank
        whose certificate fails at lo.  on=False frees the state (the arguments are not looked at); a sampler it was never
        switched on for computes what it always did.  The handle's kernel (Handle.kernel()) is not touched."""
        if not on:
            check(self.lib.gpirt_sampler_ell_enable(self._s, 0.0, 0.0, 0, None, 0, 0, 0))
            self._ell_points = 0
            return
        lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float64)
        if lp is not None and lp.shape != (int(points),):
            raise ValueError(f"ell_enable: log_prior must hold points = {int(points)} values")
        check(self.lib.gpirt_sampler_ell_enable(self._s, float(lo), float(hi), int(points), None if lp is None else _ptr(lp),
                                                int(width), -1 if k0 is None else int(k0), 1))
        self._ell_points = int(points)

    def draw_ell(self, kind="whitened"):
        """One Metropolis update of the length scale.  kind="whitened": the prior-whitened one (nu = L^-1 f held fixed), see
        gpirt_amd.ell.step_exact; kind="centred": f held fixed and the GP prior decides, see gpirt_amd.ell.step_exact_centred.
        Each kind has its own width, call count, uniforms and counters."""
        self._call(_ell_entry(kind, "gpirt_sampler_draw_ell"))

    def ell_width(self, w: int, kind="whitened"):
        """The proposal width of that kind's updates from the next one on (1 .. points - 1)."""
        check(getattr(self.lib, _ell_entry(kind, "gpirt_sampler_ell_width"))(self._s, int(w)))

    def ell_get(self, name: str) -> np.ndarray:
        """One array by name: grid, log_prior (points), index (int64, 1), counts (int64: updates, accepted, out_of_range, failed)
        and, of the last update that reached the device, nu, f_prop (n x m), delta (m), record (dll, log_ratio, log_u, accept,
        nonfinite) and times (ms of device time with enable_timing() on: copies, solve, factor, product, delta, decide, commit,
        restore).  Of the last centred update that reached the device: nu_prop (n x m), dq (m), record_centred (dq, dld,
        log_ratio, log_u, accept, nonfinite), and counts_centred (int64, as counts), times_centred (_lib.ELL_PARTS_CENTRED).
        nu is that of whichever update ran last."""
        P = getattr(self, "_ell_points", 0)
        if name in ("index", "counts", "counts_centred"):
            out = np.empty(1 if name == "index" else 4, dtype=np.int64)
        elif name in ("nu", "f_prop", "nu_prop"):
            out = np.empty((self.n, self.m), order="F")
        else:
            out = np.empty({"delta": self.m, "record": 5, "times": len(_lib.ELL_PARTS), "dq": self.m, "record_centred": 6,
                            "times_centred": len(_lib.ELL_PARTS_CENTRED)}.get(name, P))
        self._get_into("gpirt_sampler_ell_get", name, out)
        return out

    def ell(self) -> dict:
        """The length scale's state (gpirt_sampler_ell_stats): index, length_scale, points, width, lo, hi, the counters
        (updates, accepted, out_of_range, failed), accept_rate, factorisations, and of the last update `last` ("accepted",
        "rejected", "out_of_range", "failed" or None), last_proposed and its two uniforms -- all of the whitened update; under
        "centred" (gpirt_sampler_ell_centred_stats) the centred update's width, counters, accept_rate, factorisations, last,
        last_proposed and uniforms."""
        e = _lib.Ell()
        check(self.lib.gpirt_sampler_ell_stats(self._s, C.byref(e)))
        out = {k: int(getattr(e, k)) for k in ("index", "points", "width", "last_proposed", "factorisations") + _lib.ELL_COUNTS}
        out.update({k: float(getattr(e, k)) for k in ("length_scale", "lo", "hi", "last_u0", "last_u1")})
        out["last"] = _lib.ELL_LAST[int(e.last)]
        out["accept_rate"] = out["accepted"] / out["updates"] if out["updates"] else float("nan")
        c = _lib.EllCentred()
        check(self.lib.gpirt_sampler_ell_centred_stats(self._s, C.byref(c)))
        cen = {k: int(getattr(c, k)) for k in ("width", "last_proposed", "factorisations") + _lib.ELL_COUNTS}
        cen.update(last_u0=float(c.last_u0), last_u1=float(c.last_u1), last=_lib.ELL_LAST[int(c.last)])
        cen["accept_rate"] = cen["accepted"] / cen["updates"] if cen["updates"] else float("nan")
        out["centred"] = cen
        return out

    # -- per-item GP amplitudes, fixed or sampled in the chain (include/gpirt_hip.h gpirt_sampler_amp_*, gpirt_amd.amp)
    def amp_set(self, a):
        """Fixed amplitudes: m values, each finite and in [0.01, 1000]; item j's prior is f_j ~ N(0, a_j^2 (K + 0.001 I)), so
        draw_f's prior draw is a_j L z_j and draw_fstar's standard deviation a_j s.  None turns amplitudes off.  After init(); f
        is not rescaled.  Refused with the reason: rng="reference", kernel_fp32, an item shard, and while amp_enable is on."""
        if a is None:
            check(self.lib.gpirt_sampler_amp_set(self._s, None))
            return
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.m,)))
        check(self.lib.gpirt_sampler_amp_set(self._s, _ptr(a)))

    def amp_enable(self, lo=0.1, hi=10.0, points=129, log_prior=None, width=4, k0=None, planned_draws=0, on=True):
        """Put every item's amplitude on the logarithmic grid a_k = lo (hi / lo)^(k / (points - 1)) with the prior mass log_prior
        (`points` finite values; None: -(ln a_k)^2 / 2, a choice), every item's proposal width `width` (1 .. points - 1) and the
        starting indices k0 (m values, or one for all; None: the grid point nearest 1).  planned_draws: how many amp_record()
        calls the draw buffer holds.  After init().  Refused with the reason: rng="reference", kernel_fp32, an item shard, and
        while amp_set is on.  on=False frees the state and turns amplitudes off."""
        if not on:
            check(self.lib.gpirt_sampler_amp_enable(self._s, 0.0, 0.0, 0, None, 0, None, 0, 0))
            self._amp_points = 0
            return
        lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float64)
        if lp is not None and lp.shape != (int(points),):
            raise ValueError(f"amp_enable: log_prior must hold points = {int(points)} values")
        kk = None if k0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(k0, dtype=np.int32), (self.m,)))
        check(self.lib.gpirt_sampler_amp_enable(self._s, float(lo), float(hi), int(points), None if lp is None else _ptr(lp),
                                                int(width), None if kk is None else kk.ctypes.data_as(C.POINTER(C.c_int)),
                                                int(planned_draws), 1))
        self._amp_points = int(points)

    def draw_amp(self):
        """One prior-whitened Metropolis update of every item's amplitude in one launch (gpirt_amd.amp.step_exact is its NumPy
        statement): nothing is read back."""
        self._call("gpirt_sampler_draw_amp")

    def draw_amp_centred(self):
        """One centred update of every item's amplitude on the GP's rank-64 smooth part (gpirt_sampler_draw_amp_centred;
        gpirt_amd.amp.centred_exact_coef and centred_exact_update are its NumPy statement): nothing is read back.  It reads the
        prior density of f, so it belongs behind step(consistent=True)."""
        self._call("gpirt_sampler_draw_amp_centred")

    def amp_centred(self) -> dict:
        """The centred update's totals (gpirt_sampler_amp_centred_stats): calls, rank, updates, accepted, same, failed, accept_rate
        (of the decided updates) and last_ms."""
        a = _lib.AmpCentred()
        check(self.lib.gpirt_sampler_amp_centred_stats(self._s, C.byref(a)))
        out = {k: int(getattr(a, k)) for k in ("calls", "rank") + _lib.AMP_CENTRED_COUNTS}
        out.update(accept_rate=float(a.accept_rate), last_ms=float(a.last_ms))
        return out

    def amp_width(self, w):
        """The proposal widths from the next update on: m values (or one for all), each in 1 .. points - 1."""
        w = np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.int32), (self.m,)))
        check(self.lib.gpirt_sampler_amp_width(self._s, w.ctypes.data_as(C.POINTER(C.c_int))))

    def amp_record(self):
        """Append the current indices to the draw buffer and add 1 to hist[k_j, j], on the device."""
        self._call("gpirt_sampler_amp_record")

    def amp_get(self, name: str) -> np.ndarray:
        """One array by name: grid, log_prior (points), amplitude (m), index, width (int32, m), counts (int64, 4 x m: updates,
        accepted, out_of_range, failed), record (5 x m of the last update: dll, log_ratio, log_u, status, nonfinite; status as
        _lib.AMP_STATUS), hist (uint32, points x m), draws (int32, recorded x m), time (1: ms of device time of the last update
        with enable_timing() on).  Of the centred update, from its first call on: counts_centred (int64, 4 x m: updates, accepted,
        same, failed), record_centred (5 x m: Q, k', dll, log u1, status as _lib.AMP_CENTRED_STATUS), rank (int), live (int32, 64),
        the last call's centred_T, centred_z, centred_w, centred_xi, centred_g (64 x m), centred_Q (m), centred_H (n x m, valid
        until the next draw_f), centred_Xh, centred_R, centred_F (64 x 64), time_centred."""
        P, m = getattr(self, "_amp_points", 0), self.m
        R = _lib.AMP_CENTRED_RANK
        if name == "rank":
            out = np.empty(1, dtype=np.int32)
            self._get_into("gpirt_sampler_amp_get", name, out)
            return int(out[0])
        if name == "live":
            out = np.empty(R, dtype=np.int32)
        elif name == "counts_centred":
            out = np.empty((4, m), dtype=np.int64)
        elif name == "record_centred":
            out = np.empty((5, m))
        elif name in ("centred_T", "centred_z", "centred_w", "centred_xi", "centred_g"):
            out = np.empty((R, m), order="F")
        elif name in ("centred_Xh", "centred_R", "centred_F"):
            out = np.empty((R, R), order="F")
        elif name == "centred_H":
            out = np.empty((self.n, m), order="F")
        elif name in ("centred_Q", "time_centred"):
            out = np.empty(m if name == "centred_Q" else 1)
        elif name in ("index", "width"):
            out = np.empty(m, dtype=np.int32)
        elif name == "counts":
            out = np.empty((4, m), dtype=np.int64)
        elif name == "record":
            out = np.empty((5, m))
        elif name == "hist":
            out = np.empty((P, m), dtype=np.uint32)
        elif name == "draws":
            out = np.empty((self.amp()["recorded"], m), dtype=np.int32)
        else:
            out = np.empty({"amplitude": m, "time": 1}.get(name, P))
        self._get_into("gpirt_sampler_amp_get", name, out)
        return out

    def amp(self) -> dict:
        """The amplitudes' state (gpirt_sampler_amp_stats): mode (None, "fixed" or "sampled"), points, m, calls, the counters
        summed over the items (updates, accepted, out_of_range, failed), the pooled accept_rate, planned_draws, recorded, lo, hi,
        min_amplitude and max_amplitude."""
        a = _lib.Amp()
        check(self.lib.gpirt_sampler_amp_stats(self._s, C.byref(a)))
        out = {k: int(getattr(a, k)) for k in ("points", "m", "calls", "planned_draws", "recorded") + _lib.AMP_COUNTS}
        out.update({k: float(getattr(a, k)) for k in ("accept_rate", "lo", "hi", "min_amplitude", "max_amplitude")})
        out["mode"] = _lib.AMP_MODES[int(a.on)]
        return out

    # -- the centred beta update: exact Gibbs for the mean's coefficients with f + mu held fixed (gpirt_sampler_draw_beta_centred)
    def draw_beta_centred(self):
        """One centred update of every item's beta (gpirt_sampler_draw_beta_centred; gpirt_amd.beta.centred_shared and
        centred_exact_update are its NumPy statement): beta_j and f_j move together with f_j + mu_j held fixed, so the likelihood
        does not change and nothing is accepted or rejected.  Nothing is read back.  It reads the prior density of f, so it
        belongs behind step(consistent=True)."""
        self._call("gpirt_sampler_draw_beta_centred")

    def beta_centred(self) -> dict:
        """The centred beta update's totals (gpirt_sampler_beta_centred_stats): calls, rank, updates, failed and last_ms."""
        a = _lib.BetaCentred()
        check(self.lib.gpirt_sampler_beta_centred_stats(self._s, C.byref(a)))
        out = {k: int(getattr(a, k)) for k in ("calls", "rank") + _lib.BETA_CENTRED_COUNTS}
        out.update(last_ms=float(a.last_ms))
        return out

    def beta_centred_get(self, name: str) -> np.ndarray:
        """One array of the last draw_beta_centred() by name: W (n x 2), B (2 x 2), P, Gx (64 x 2), T, z, mean, beta_old, beta_new
        (2 x m, as beta), chol (3 x m: c00, c10, c11), record (m: status, 0 updated, 3 failed), counts (int64, 2 x m: updates,
        failed), time (1: ms of device time of the last call with enable_timing() on), time_item (1: of that, the per-item
        kernel's)."""
        m, R = self.m, _lib.BETA_CENTRED_RANK
        if name == "W":
            out = np.empty((self.n, 2), order="F")
        elif name == "B":
            out = np.empty((2, 2), order="F")
        elif name in ("P", "Gx"):
            out = np.empty((R, 2), order="F")
        elif name in ("T", "z", "mean", "beta_old", "beta_new"):
            out = np.empty((2, m), order="F")
        elif name == "chol":
            out = np.empty((3, m), order="F")
        elif name == "counts":
            out = np.empty((2, m), dtype=np.int64)
        elif name == "record":
            out = np.empty(m)
        elif name in ("time", "time_item"):
            out = np.empty(1)
        else:
            raise ValueError(f"unknown centred beta array {name!r}")
        self._get_into("gpirt_sampler_beta_centred_get", name, out)
        return out

    # -- the collapsed scale and shift move: the linear mean with theta summed out (gpirt_sampler_draw_scale, gpirt_amd.scale)
    @staticmethod
    def _scale_kind(kind) -> int:
        if kind in _lib.SCALE_KINDS:
            return _lib.SCALE_KINDS.index(kind)
        if isinstance(kind, (int, np.integer)) and not isinstance(kind, bool):
            return int(kind)                      # (the library refuses anything but 0 and 1, with its reason)
        raise ValueError(f"scale: kind = {kind!r}, it is \"scale\" or \"shift\"")

    def scale_enable(self, w_scale=None, w_shift=None):
        """Allocate the move's buffers and set the proposal widths, the sds of eps (scale) and delta (shift)
        (gpirt_sampler_scale_enable).  None is the default 1 / sqrt(n), a choice and not a measurement; 0 proposes the state
        itself.  Calling it again only sets the widths."""
        nan = float("nan")
        check(self.lib.gpirt_sampler_scale_enable(self._s, nan if w_scale is None else float(w_scale),
                                                  nan if w_shift is None else float(w_shift)))

    def draw_scale(self, kind):
        """One proposal of kind "scale" (every slope times exp(-eps)) or "shift" (the linear mean at x + delta), decided on the
        likelihood with every theta summed out; legal between theta_partial() and theta_finish() (gpirt_sampler_draw_scale;
        gpirt_amd.scale.step_exact is its NumPy statement).  Nothing is read back."""
        check(self.lib.gpirt_sampler_draw_scale(self._s, self._scale_kind(kind)))

    def scale_width(self, kind, w):
        """Set one kind's proposal width (gpirt_sampler_scale_width)."""
        check(self.lib.gpirt_sampler_scale_width(self._s, self._scale_kind(kind), float(w)))

    def scale(self) -> dict:
        """The move's totals (gpirt_sampler_scale_stats): on, and per kind a dict(calls, accepted, failed, width, last_ms)."""
        a = _lib.Scale()
        check(self.lib.gpirt_sampler_scale_stats(self._s, C.byref(a)))
        out = dict(on=bool(a.on))
        for k, name in enumerate(_lib.SCALE_KINDS):
            out[name] = dict(calls=int(a.calls[k]), accepted=int(a.accepted[k]), failed=int(a.failed[k]), width=float(a.width[k]),
                             last_ms=float(a.last_ms[k]))
        return out

    def scale_get(self, name: str):
        """One array of the move by name: record (a dict by _lib.SCALE_RECORD's names, status as its word), lz, lz_prop, dlz (n),
        beta_prop (2 x m), mu_prop, fstar_prop (N x m), logpost, logpost_prop (N x n), counts (int64 3 x 2: calls, accepted, failed
        by kind), times (a dict by _lib.SCALE_TIMES' names, ms of the last call with enable_timing() on)."""
        N, n, m = _lib.NGRID, self.n, self.m
        if name == "record":
            raw = np.empty(len(_lib.SCALE_RECORD))
            self._get_into("gpirt_sampler_scale_get", name, raw)
            out = {k: float(v) for k, v in zip(_lib.SCALE_RECORD, raw) if not k.startswith("_")}
            out["kind"] = _lib.SCALE_KINDS[int(out["kind"])]
            out["status"] = _lib.SCALE_STATUS[int(out["status"])]
            return out
        if name == "times":
            raw = np.empty(len(_lib.SCALE_TIMES))
            self._get_into("gpirt_sampler_scale_get", name, raw)
            return dict(zip(_lib.SCALE_TIMES, map(float, raw)))
        if name in ("lz", "lz_prop", "dlz"):
            out = np.empty(n)
        elif name == "beta_prop":
            out = np.empty((2, m), order="F")
        elif name in ("mu_prop", "fstar_prop"):
            out = np.empty((N, m), order="F")
        elif name in ("logpost", "logpost_prop"):
            out = np.empty((N, n), order="F")
        elif name == "counts":
            out = np.empty((3, 2), dtype=np.int64)
        else:
            raise ValueError(f"unknown scale array {name!r}")
        self._get_into("gpirt_sampler_scale_get", name, out)
        return out

    # -- the population prior for theta, fixed or sampled in the chain (include/gpirt_hip.h gpirt_sampler_pop_*, gpirt_amd.pop)
    def pop_set(self, codes, log_prior=None):
        """A fixed population prior: one code per respondent in 0 .. G - 1 (every group with a member) and a G x 1001 table of
        finite log masses on the theta grid (log_prior[g] is group g's prior; it need not be normalised; None: the default
        N(0, 1) row for every group).  draw_theta adds row codes[i] in place of N(0, 1).  codes=None turns it off.  After init();
        works under both RNG contracts.  Refused with the reason: an item shard, theta_block in use, while pop_enable is on."""
        if codes is None:
            check(self.lib.gpirt_sampler_pop_set(self._s, None, 0, None))
            self._pop = (0, 0, 0)
            return
        from . import pop as PO
        cd = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
        if cd.shape != (self.n,):
            raise ValueError(f"pop_set: codes must hold n = {self.n} values")
        if log_prior is None:
            G = int(cd.max()) + 1 if cd.size else 1
            log_prior = np.tile(PO.default_row(), (max(G, 1), 1))
        lp = np.ascontiguousarray(log_prior, dtype=np.float64)
        if lp.ndim != 2 or lp.shape[1] != NGRID:
            raise ValueError(f"pop_set: log_prior must be G x {NGRID}")
        check(self.lib.gpirt_sampler_pop_set(self._s, cd.ctypes.data_as(C.POINTER(C.c_int32)), lp.shape[0], _ptr(lp)))
        self._pop = (lp.shape[0], 0, 0)

    def pop_enable(self, codes=None, groups=None, anchor_row=None, mu_hi=3.0, points_mu=121, sd_lo=0.2, sd_hi=5.0, points_sd=65,
                   log_hyper_mu=None, log_hyper_sd=None, a0=None, b0=None, planned_draws=0, on=True):
        """A sampled population prior: group 0 is the anchor and keeps anchor_row (1001 finite values; None: the N(0, 1) row),
        every group g >= 1 has (mu_g, sd_g) on gpirt_amd.pop.grids(mu_hi, points_mu, sd_lo, sd_hi, points_sd) with the
        hyperprior masses log_hyper_mu / log_hyper_sd (None: flat in mu, flat in log sd) and the start indices a0, b0 (G values
        each, or one for all; None: mu = 0's point and the sd point nearest 1).  groups: G (None: max(codes) + 1).
        planned_draws: how many pop_record() calls the draw buffer holds.  After init().  Refused with the reason:
        rng="reference", an item shard, theta_block in use, while pop_set is on.  on=False frees the state."""
        if not on:
            check(self.lib.gpirt_sampler_pop_enable(self._s, None, 0, None, 0.0, 0, 0.0, 0.0, 0, None, None, None, None, 0, 0))
            self._pop = (0, 0, 0)
            return
        cd = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
        if cd.shape != (self.n,):
            raise ValueError(f"pop_enable: codes must hold n = {self.n} values")
        G = int(groups) if groups is not None else (int(cd.max()) + 1 if cd.size else 1)
        Pm, Ps = int(points_mu), int(points_sd)

        def vec(v, size, what):
            if v is None:
                return None
            v = np.ascontiguousarray(v, dtype=np.float64)
            if v.shape != (size,):
                raise ValueError(f"pop_enable: {what} must hold {size} values")
            return v

        def ints(v):
            return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.int32), (max(G, 1),)))
        ar, hm, hs = vec(anchor_row, NGRID, "anchor_row"), vec(log_hyper_mu, Pm, "log_hyper_mu"), vec(log_hyper_sd, Ps, "log_hyper_sd")
        ia, ib = ints(a0), ints(b0)
        ip = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_int))          # noqa: E731
        dp = lambda v: None if v is None else _ptr(v)                                        # noqa: E731
        check(self.lib.gpirt_sampler_pop_enable(self._s, cd.ctypes.data_as(C.POINTER(C.c_int32)), G, dp(ar), float(mu_hi), Pm,
                                                float(sd_lo), float(sd_hi), Ps, dp(hm), dp(hs), ip(ia), ip(ib),
                                                int(planned_draws), 1))
        self._pop = (G, Pm, Ps)

    def draw_pop(self):
        """One exact Gibbs update of every group's (mu_g, sd_g), g >= 1, on the grids and the rebuild of the groups' rows: two
        launches, nothing is read back (gpirt_amd.pop.step_exact is its NumPy statement)."""
        self._call("gpirt_sampler_draw_pop")

    def pop_record(self):
        """Append the current (a_g, b_g) to the draw buffer and add 1 to hist_mu[a_g, g] and hist_sd[b_g, g], on the device."""
        self._call("gpirt_sampler_pop_record")

    def pop_get(self, name: str) -> np.ndarray:
        """One array by name: codes (int32, n), log_prior (G x 1001) -- the two a fixed prior knows --, mu_grid, log_hyper_mu
        (points_mu), sd_grid, log_hyper_sd (points_sd), lse (points_mu x points_sd), index (int32, G x 2: (a_g, b_g), group 0's
        -1), stats (int64, 3 x G: n_g, S1, S2 of the last draw_pop), off_grid (int64, G), lp_mu (G x points_mu), lp_sd
        (G x points_sd: the last draw_pop's rows), counts (int64, 4 x G: updates, updated, skipped, failed), hist_mu (uint32,
        points_mu x G), hist_sd (uint32, points_sd x G), draws (int32, recorded x G x 2), time (1: ms of device time of the last
        draw_pop with enable_timing() on)."""
        G, Pm, Ps = getattr(self, "_pop", (0, 0, 0))
        shapes = {"codes": ((self.n,), np.int32), "log_prior": ((G, NGRID), np.float64), "mu_grid": ((Pm,), np.float64),
                  "sd_grid": ((Ps,), np.float64), "log_hyper_mu": ((Pm,), np.float64), "log_hyper_sd": ((Ps,), np.float64),
                  "lse": ((Pm, Ps), np.float64), "index": ((G, 2), np.int32), "stats": ((3, G), np.int64),
                  "off_grid": ((G,), np.int64), "lp_mu": ((G, Pm), np.float64), "lp_sd": ((G, Ps), np.float64),
                  "counts": ((4, G), np.int64), "hist_mu": ((Pm, G), np.uint32), "hist_sd": ((Ps, G), np.uint32),
                  "time": ((1,), np.float64)}
        if name == "draws":
            out = np.empty((self.pop_stats()["recorded"], G, 2), dtype=np.int32)
        else:
            shape, dt = shapes.get(name, ((0,), np.float64))
            out = np.empty(shape, dtype=dt)
        self._get_into("gpirt_sampler_pop_get", name, out)
        return out

    def pop_stats(self) -> dict:
        """The population prior's state (gpirt_sampler_pop_stats): mode (None, "fixed" or "sampled"), groups, n, points_mu,
        points_sd, calls, the counters summed over the groups (updates, updated, skipped, failed), off_grid (members off the grid
        in the last draw_pop), planned_draws, recorded, mu_hi, sd_lo, sd_hi, time_ms."""
        p = _lib.Pop()
        check(self.lib.gpirt_sampler_pop_stats(self._s, C.byref(p)))
        out = {k: int(getattr(p, k)) for k in ("groups", "n", "points_mu", "points_sd", "calls", "off_grid", "planned_draws",
                                               "recorded") + _lib.POP_COUNTS}
        out.update({k: float(getattr(p, k)) for k in ("mu_hi", "sd_lo", "sd_hi")})
        out["time_ms"] = float(p.last_ms)
        out["mode"] = _lib.POP_MODES[int(p.on)]
        return out

    # -- ordinal (graded) responses, the thresholds sampled in the chain (include/gpirt_hip.h gpirt_sampler_ordinal_*, gpirt_amd.ordinal)
    def ordinal_enable(self, cat, C=None, hi=6.0, points=241, log_prior=None, K0=None, width=16, planned_draws=0):
        """Turn the chain into the cumulative-logit model on the categories cat (n x m, 0 = missing, 1 .. C; C: the number
        of categories, None: cat.max()).  The sampler must have been created on gpirt_amd.ordinal.dichotomise(cat).  The thresholds live on
        gpirt_amd.ordinal.grid(hi, points) with the log masses log_prior (None: -t^2 / 18) and start at the indices K0 (m x (C - 1),
        strictly increasing; None: the library's equally spaced start -- gpirt_amd.ordinal.init_thresholds gives the data's).
        beta[0, :] is set to 0 and stays there.  From then on step() runs the ordinal kernels and draw_thresholds() updates the
        thresholds; width: the window W of that update.  After init().  cat=None turns ordinal off.  Refused with the reason:
        rng="reference", an item shard, theta_block in use, n > 16384, an analysis block that reads y already on."""
        import ctypes as ct                   # (the keyword C is the issue's name for the number of categories)
        if cat is None:
            check(self.lib.gpirt_sampler_ordinal_enable(self._s, None, 0, 0.0, 0, None, None, 0, 0))
            self._ord = (0, 0, 0)
            return
        c8 = np.asfortranarray(np.asarray(cat, dtype=np.int8))
        if c8.shape != (self.n, self.m):
            raise ValueError(f"ordinal_enable: cat must be {self.n} x {self.m}")
        Cn = int(C) if C is not None else int(c8.max())
        P = int(points)
        lp = None if log_prior is None else np.ascontiguousarray(log_prior, dtype=np.float64).reshape(-1)
        if lp is not None and lp.shape != (P,):
            raise ValueError(f"ordinal_enable: log_prior must hold points = {P} values")
        k0 = None if K0 is None else np.ascontiguousarray(K0, dtype=np.int32)
        if k0 is not None and k0.shape != (self.m, max(Cn - 1, 0)):
            raise ValueError(f"ordinal_enable: K0 must be m x (C - 1) = {self.m} x {Cn - 1}")
        check(self.lib.gpirt_sampler_ordinal_enable(
            self._s, c8.ctypes.data_as(ct.POINTER(ct.c_int8)), Cn, float(hi), P, None if lp is None else _ptr(lp),
            None if k0 is None else k0.ctypes.data_as(ct.POINTER(ct.c_int32)), int(width), int(planned_draws)))
        self._ord = (Cn, P, int(width))

    def draw_thresholds(self):
        """One exact Gibbs update of every threshold on the grid inside a randomly placed window: one launch, nothing is read
        back (gpirt_amd.ordinal.thresholds_exact is its NumPy statement).  A call of its own after step(), as draw_pop is."""
        self._call("gpirt_sampler_draw_thresholds")

    def ordinal_width(self, width):
        """The window W of draw_thresholds from the next update on, 1 .. 64.  ordinal_get("lp") keeps the layout of the update
        that wrote it (ordinal_stats()["lp_width"]) until then."""
        check(self.lib.gpirt_sampler_ordinal_width(self._s, int(width)))
        Cn, P, _ = getattr(self, "_ord", (0, 0, 0))
        self._ord = (Cn, P, int(width))

    def ordinal_record(self):
        """Append the current threshold indices to the draw buffer and add 1 to their histogram cells, on the device."""
        self._call("gpirt_sampler_ordinal_record")

    def ordinal_accumulate_irf(self):
        """cum[j, c, k] += sigma(f*[k, j] - b_{j,c}) = P(y > c | theta_k) under the current draw (gpirt_amd.ordinal.curves)."""
        self._call("gpirt_sampler_ordinal_accumulate_irf")

    def ordinal_get(self, name: str) -> np.ndarray:
        """One array by name: cat (int8, n x m), grid, log_prior (points), index (int32, m x (C - 1)), thresholds (m x (C - 1)),
        counts (int64, m x C: observed cells per category), lp (m x (C - 1) x W: the last update's masses by window slot, -inf
        outside the candidates; W is that update's width), window (int32, m x (C - 1): the last windows' first index), hist (uint32, m x (C - 1) x points),
        draws (int32, recorded x m x (C - 1)), cum (m x (C - 1) x 1001), pinned, failed, updates (int64 scalars)."""
        Cn, P, W = getattr(self, "_ord", (0, 0, 0))
        if name == "lp":
            W = self.ordinal_stats()["lp_width"]      # the width of the update that wrote it, whatever ordinal_width set since
        m, R = self.m, max(Cn - 1, 0)
        shapes = {"grid": ((P,), np.float64), "log_prior": ((P,), np.float64), "index": ((m, R), np.int32),
                  "thresholds": ((m, R), np.float64), "counts": ((m, Cn), np.int64), "lp": ((m, R, W), np.float64),
                  "window": ((m, R), np.int32), "hist": ((m, R, P), np.uint32), "cum": ((m, R, NGRID), np.float64),
                  "pinned": ((1,), np.int64), "failed": ((1,), np.int64), "updates": ((1,), np.int64)}
        if name == "cat":
            out = np.empty((self.n, m), dtype=np.int8, order="F")
        elif name == "draws":
            out = np.empty((self.ordinal_stats()["recorded"], m, R), dtype=np.int32)
        else:
            shape, dt = shapes.get(name, ((0,), np.float64))
            out = np.empty(shape, dtype=dt)
        self._get_into("gpirt_sampler_ordinal_get", name, out)
        return int(out[0]) if name in ("pinned", "failed", "updates") else out

    def ordinal_stats(self) -> dict:
        """gpirt_sampler_ordinal_stats: on, n, m, categories, points, width, calls, pinned, failed, updates, planned_draws,
        recorded, irf_draws, lp_width (the W of the last update: the slots per row of "lp"), hi, time_ms."""
        p = _lib.Ordinal()
        check(self.lib.gpirt_sampler_ordinal_stats(self._s, C.byref(p)))
        out = {k: int(getattr(p, k)) for k in ("n", "m", "categories", "points", "width", "calls", "pinned", "failed", "updates",
                                               "planned_draws", "recorded", "irf_draws", "lp_width")}
        out.update(on=bool(p.on), hi=float(p.hi), time_ms=float(p.last_ms))
        return out

    def ordinal(self, probs=(0.025, 0.5, 0.975)) -> dict:
        """The recorded thresholds summarised and the accumulated curves finished (gpirt_amd.ordinal.summarise and curves)."""
        from . import ordinal as OR
        st = self.ordinal_stats()
        out = OR.summarise(self.ordinal_get("draws"), self.ordinal_get("grid"), probs=probs)
        out.update(hist=self.ordinal_get("hist"), counters={k: st[k] for k in ("pinned", "failed", "updates")})
        if st["irf_draws"]:
            out["curves"] = OR.curves(self.ordinal_get("cum"), st["irf_draws"])
        return out

    # -- ordinal model fit accumulated on the device (include/gpirt_hip.h gpirt_sampler_ordinal_fit_*, gpirt_amd.ordinal.fit_*)
    def ordinal_fit_enable(self, parts=("waic", "pred", "ppc")):
        """Allocate and zero the fit accumulators of the ordinal model for any subset of "waic" (pointwise WAIC, 24 bytes per cell),
        "pred" (the sums of P(y > c) per cell, missing ones included, 8 (C - 1) bytes per cell) and "ppc" (the first-order
        posterior predictive check per item, respondent, (item, category) and for the whole matrix).  After ordinal_enable.
        parts=None (or ()) frees the block."""
        from . import ordinal as OR
        bits = OR.fit_parts(parts)
        check(self.lib.gpirt_sampler_ordinal_fit_enable(self._s, bits))
        self._ofit = bits

    def ordinal_fit_accumulate(self):
        """Add the current state (after step() and draw_thresholds()) as one draw, with the sampler's current thresholds; the
        chain is untouched (the replicate draws from a stage of its own)."""
        self._call("gpirt_sampler_ordinal_fit_accumulate")

    def ordinal_fit_get(self, name: str) -> np.ndarray:
        """One raw array by name: draws; lse, ll_mean, ll_m2 (n x m; a missing cell: 0, 0, -1); pred_sum ((C - 1) x n x m);
        item_<f>, respondent_<f>, total_<f> for f in _lib.OFIT_UNIT_FIELDS; cat_<f> (m x C) for f in _lib.OFIT_CAT_FIELDS; and of
        the last counted draw rep (int8, n x m), delta, score (m + n + 1: items, respondents, the whole matrix), counts_rep (m x C)."""
        from . import ordinal as OR
        out = OR.fit_array(name, self.n, self.m, getattr(self, "_ord", (0, 0, 0))[0])
        return OR._fit_get_into(self.lib.gpirt_sampler_ordinal_fit_get, (self._s,), name, out)

    def ordinal_fit_totals(self) -> dict:
        """gpirt_sampler_ordinal_fit_totals: n, m, categories, parts, draws, n_obs, lppd, p_waic, elpd_waic, waic, se_elpd_waic."""
        from . import ordinal as OR
        t = _lib.OrdinalFit()
        check(self.lib.gpirt_sampler_ordinal_fit_totals(self._s, C.byref(t)))
        return OR._fit_totals_dict(t)

    def ordinal_fit_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the fit accumulators, its header refreshed: what
        gpirt_amd.ordinal.fit_combine pools."""
        return self._state("gpirt_sampler_ordinal_fit_state")

    def ordinal_fit(self) -> dict:
        """The finished fit output (gpirt_amd.ordinal.fit_result): waic, pred, item, respondent, totals and categories."""
        from . import ordinal as OR
        return OR.fit_result(self.ordinal_fit_get, self.ordinal_fit_totals(), self.ordinal_get("cat"))

    # -- scoring new respondents under ordinal responses (include/gpirt_hip.h gpirt_sampler_ordinal_score_*, gpirt_amd.ordinal.score_*)
    def ordinal_score_enable(self, cat_new, predict=False, top=5):
        """Upload cat_new (n_new x m over this sampler's items, 0 = missing, 1 .. C, 1 <= n_new <= 16384) and allocate the score
        accumulators; predict=True adds the category predictions and the next-item information for every new respondent and item
        (top, 1..16: how many unanswered items ordinal_score_predict() lists).  After ordinal_enable.  cat_new=None frees the block."""
        import ctypes as ct
        from . import ordinal as OR
        if cat_new is None:
            check(self.lib.gpirt_sampler_ordinal_score_enable(self._s, None, 0, 0, 0))
            self._oscore = (0, False, 0)
            return
        c8 = np.asfortranarray(OR.check_cat_new(cat_new, self.m))
        check(self.lib.gpirt_sampler_ordinal_score_enable(self._s, c8.ctypes.data_as(ct.POINTER(ct.c_int8)), c8.shape[0],
                                                          int(bool(predict)), int(top)))
        self._oscore = (c8.shape[0], bool(predict), int(top))
        self._oscore_cat = c8

    def ordinal_score_accumulate(self):
        """Score the new respondents under the current f* and thresholds (after step() and draw_thresholds()) as one draw; the
        chain is untouched."""
        self._call("gpirt_sampler_ordinal_score_accumulate")

    def ordinal_score_get(self, name: str) -> np.ndarray:
        """One array by name.  Raw: draws, nonfinite, n_obs (int64, n_new), lpd_acc, ll_sum (n_new), post_sum (n_new x 1001); of the
        last accumulate product (1001 x n_new, column-major), wc (n_new), w_table (m x C); with predict prob_sum (C x n_new x m),
        info_sum (n_new x m), counts (int64: pred_draws, pred_skipped), weights (1001 x n_new) and operands (1001 x (C + 1) m,
        both column-major) of the last counted draw.  Finished, from those sums (gpirt_amd.ordinal.score_result / predict_result):
        grid_post, theta_mean, theta_sd, theta_map, lpd, loglik_mean; probs (n_new x m x C), expected, info (n_new x m)."""
        from . import ordinal as OR
        n = getattr(self, "_oscore", (0, False, 0))[0]
        Cn, m = getattr(self, "_ord", (0, 0, 0))[0], self.m
        if name in ("grid_post", "theta_mean", "theta_sd", "theta_map", "lpd", "loglik_mean"):
            return self.ordinal_score()[name]
        if name in ("probs", "expected", "info"):
            return OR.predict_result({k: self.ordinal_score_get(k) for k in ("prob_sum", "info_sum", "counts")},
                                     getattr(self, "_oscore_cat", None), top=None)[name]
        if name in ("draws", "nonfinite", "n_obs", "counts"):
            out = np.empty(2 if name == "counts" else n, dtype=np.int64)
        elif name == "post_sum":
            out = np.empty((n, NGRID))
        elif name in ("product", "weights"):
            out = np.empty((NGRID, n), order="F")
        elif name == "operands":
            out = np.empty((NGRID, (Cn + 1) * m), order="F")
        elif name == "w_table":
            out = np.empty((m, Cn))
        elif name == "info_sum":
            out = np.empty((n, m), order="F")
        elif name == "prob_sum":
            out = np.empty((Cn, m, n))
            self._get_into("gpirt_sampler_ordinal_score_get", name, out)
            return out.transpose(0, 2, 1)                  # C planes of column-major n_new x m
        else:
            out = np.empty(n)
        self._get_into("gpirt_sampler_ordinal_score_get", name, out)
        return out

    def ordinal_score_state(self, predict=False):
        """Torch view (int64, on the device) of the ONE block that holds the score accumulators (predict=True: the prediction
        block): what gpirt_amd.ordinal.score_combine / score_predict_combine pool."""
        return self._state("gpirt_sampler_ordinal_score_predict_state" if predict else "gpirt_sampler_ordinal_score_state")

    def ordinal_score_predict_state(self):
        return self.ordinal_score_state(predict=True)

    def ordinal_score(self, probs=(0.025, 0.5, 0.975)) -> dict:
        """Every finished output of this sampler's score accumulators (gpirt_amd.score.result's keys): grid_post, theta_mean,
        theta_sd, theta_quantiles, theta_map, lpd, loglik_mean, lpd_total, se_lpd_total and the raw arrays."""
        from . import ordinal as OR
        return OR.score_combine(self.handle, [self], probs=probs)

    def ordinal_score_predict(self, top=None) -> dict:
        """Every finished output of the prediction part: probs (n_new x m x C), expected, info, next_items, next_info, prob_sum,
        info_sum, pred_draws, pred_skipped; top defaults to ordinal_score_enable's."""
        from . import ordinal as OR
        return OR.score_predict_combine(self.handle, [self], top=getattr(self, "_oscore", (0, False, 5))[2] if top is None else top)

    # -- scoring new respondents on the device (include/gpirt_hip.h gpirt_sampler_score_*, gpirt_amd.score)
    def score_enable(self, y_new):
        """Pack y_new (n_new x m over this sampler's items, +1 / -1 / NaN, 1 <= n_new <= 16384) and allocate the
        accumulators; y_new=None frees them."""
        if y_new is None:
            check(self.lib.gpirt_sampler_score_enable(self._s, None, 0))
            self._score_n = 0
            return
        from . import score as SC
        y = np.asfortranarray(SC.check_y_new(y_new, self.m))
        check(self.lib.gpirt_sampler_score_enable(self._s, _ptr(y), y.shape[0]))
        self._score_n = y.shape[0]

    def score_accumulate(self):
        """Score the new respondents under the current f* (after a sampling iteration's step) as one draw; the chain is
        untouched."""
        self._call("gpirt_sampler_score_accumulate")

    def score_get(self, name: str) -> np.ndarray:
        """One array by name: draws, nonfinite, n_obs (int64, n_new), lpd_acc, ll_sum, lpd, loglik_mean, theta_mean,
        theta_sd, theta_map (n_new), post_sum, grid_post (n_new x 1001), product (1001 x n_new, column-major: T of the
        last score_accumulate)."""
        n = getattr(self, "_score_n", 0)
        if name in ("draws", "nonfinite", "n_obs"):
            out = np.empty(n, dtype=np.int64)
        elif name in ("post_sum", "grid_post"):
            out = np.empty((n, NGRID))
        elif name == "product":
            out = np.empty((NGRID, n), order="F")
        else:
            out = np.empty(n)
        self._get_into("gpirt_sampler_score_get", name, out)
        return out

    def score_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the score accumulators: what
        gpirt_amd.score.combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_score_state")

    def score(self, probs=(0.025, 0.5, 0.975)) -> dict:
        """Every finished output of this sampler's accumulators (gpirt_amd.score.result's shape): gpirt_score_combine over
        its own state, nothing reflected."""
        from . import score as SC
        return SC.combine(self.handle, [self], probs=probs)

    # -- predicting the new respondents' unseen answers (include/gpirt_hip.h gpirt_sampler_score_predict_*, gpirt_amd.score)
    def score_predict_enable(self, top=5, on=True):
        """Allocate and zero the prediction accumulators on a sampler whose score_enable is on: from then on every
        score_accumulate also adds that draw's P(y_rj = +1) and next-item information for every new respondent and item.
        top (1..16): how many unanswered items score_predict() lists per respondent.  on=False frees the state."""
        if not on:
            check(self.lib.gpirt_sampler_score_predict_enable(self._s, 0))
            return
        from . import score as SC
        self._predict_top = SC.check_top(top)
        check(self.lib.gpirt_sampler_score_predict_enable(self._s, 1))

    def score_predict_get(self, name: str) -> np.ndarray:
        """One array by name: pred_sum, info_sum, p_yes, info (n_new x m), counts (int64: pred_draws, pred_skipped),
        weights (1001 x n_new, column-major: W of the last draw that counted)."""
        n = getattr(self, "_score_n", 0)
        if name == "counts":
            out = np.empty(2, dtype=np.int64)
        elif name == "weights":
            out = np.empty((NGRID, n), order="F")
        else:
            out = np.empty((n, self.m), order="F")
        self._get_into("gpirt_sampler_score_predict_get", name, out)
        return out

    def score_predict_state(self):
        """Torch view (int64, on the device) of the ONE block that holds the prediction accumulators: what
        gpirt_amd.score.predict_combine pools; copy it anywhere to combine it there."""
        return self._state("gpirt_sampler_score_predict_state")

    def score_predict(self, top=None) -> dict:
        """Every finished output of this sampler's prediction accumulators (gpirt_amd.score.predict_result's shape):
        gpirt_score_predict_combine over its own state; top defaults to score_predict_enable's."""
        from . import score as SC
        return SC.predict_combine(self.handle, [self], top=getattr(self, "_predict_top", SC.DEFAULT_TOP) if top is None else top)

    def enable_timing(self, on=True):
        check(self.lib.gpirt_sampler_enable_timing(self._s, int(on)))

    def stage_times(self) -> dict:
        ms = (C.c_double * 16)()
        k = C.c_int()
        check(self.lib.gpirt_sampler_stage_times(self._s, ms, 16, C.byref(k), None))
        names = ["draw_f", "draw_fstar", "theta_gemm", "theta_sample", "draw_beta", "factor"]
        out = {names[i]: ms[i] for i in range(k.value)}
        if getattr(self, "_last_step_consistent", False):       # the seventh stage of step(consistent=True)
            out["carry"] = self.carry_stats()["time_ms"]
        return out
