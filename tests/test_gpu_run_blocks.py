"""The analysis blocks side by side: gpirtMCMC with every analysis of the run enabled at once against the same call with one
block on, on the checkpoint-slot path (preset="fast", two chains) and on the live path (rng="reference", one chain); and the
refusal of every block's stage entries on a sampler that has nothing enabled, word for word."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CODES = dict(yea=[1], nay=[-1], missing=[None])
# Six draws after two of burn-in: one chain plans T = 6 draws for PSIS-LOO, two chains T = 12, so the rule's tail
# M = min(T // 5, ceil(3 sqrt(T))) holds a key (M = 1 and 2) and the plan is accepted with M < T; the burn-in makes a
# checkpoint's iteration number differ from its draw slot.
S, BURN = 6, 2


def senate_slice():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "senate116_y.npz"))
    y = d["y"].astype(np.float64)
    y[y == 0] = np.nan
    mixed = [j for j in range(y.shape[1]) if (y[:, j] == 1).sum() >= 10 and (y[:, j] == -1).sum() >= 10][:24]
    return np.asfortranarray(y[:100, mixed])


def same_tree(a, b, path=()):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            same_tree(a[k], b[k], path + (k,))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, z) in enumerate(zip(a, b)):
            same_tree(x, z, path + (i,))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), path
    else:
        assert a == b or (a != a and b != b), path


def without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


def analyses(y):
    """keyword -> value for every analysis of the run, and the single-block calls: name -> (keywords, what to read)"""
    n, m = y.shape
    y_new = y[10:15].copy()
    y_new[:, ::3] = np.nan                                     # unseen answers for the prediction
    groups = np.arange(n) % 2
    groups[::7] = -1
    full = dict(
        ppc=dict(pairs=True, top=5, bins=True, bins_top=5, dif=dict(groups=groups, top=5)),
        ranks=dict(pairwise=True),
        score=dict(data=y_new, predict=True, top=3),
        shape=dict(order=True, order_top=5),
        sumscore=True,
        equate=dict(x=list(range(0, m // 2)), y=list(range(m // 2, m))),
        loo=dict(top=5),
        quantiles=(0.025, 0.5, 0.975),
    )
    ppc_own = lambda r: without(r["ppc"], "pairs", "bins", "dif")                                  # noqa: E731
    single = {
        "ppc": (dict(ppc=True), lambda r: r["ppc"]),
        "pairs": (dict(ppc=dict(pairs=True, top=5)), lambda r: r["ppc"]["pairs"]),
        "bins": (dict(ppc=dict(bins=True, bins_top=5)), lambda r: r["ppc"]["bins"]),
        "dif": (dict(ppc=dict(dif=dict(groups=groups, top=5))), lambda r: r["ppc"]["dif"]),
        "ranks": (dict(ranks=full["ranks"]), lambda r: r["ranks"]),
        "score": (dict(score=dict(data=y_new)), lambda r: r["score"]),
        "predict": (dict(score=full["score"]), lambda r: r["score"]["predict"]),
        "shape": (dict(shape=True), lambda r: r["shape"]),
        "order": (dict(shape=full["shape"]), lambda r: r["shape"]["order"]),
        "sumscore": (dict(sumscore=True), lambda r: r["sumscore"]),
        "equate": (dict(equate=full["equate"]), lambda r: r["equate"]),
        "loo": (dict(loo=full["loo"]), lambda r: r["loo"]),
        "quantiles": (dict(quantiles=full["quantiles"]), lambda r: r["quantiles"]),
    }
    # what the all-on call holds of a block that has dependants on: the block's own outputs
    own = dict(single)
    own["ppc"] = (single["ppc"][0], ppc_own)
    own["score"] = (single["score"][0], lambda r: without(r["score"], "predict"))
    own["shape"] = (single["shape"][0], lambda r: without(r["shape"], "order"))
    return full, single, own


@pytest.mark.parametrize("path", ["slot", "live"])
def test_every_analysis_at_once_equals_each_alone(handle, path):
    """Every output of every block with all blocks on is, bit for bit, that of the call with the block alone (a dependant with
    its base); the chain, the IRFs, the pooled summary, the diagnostics and R's stream are those of the call with no analysis.
    path = "slot": preset="fast" with two chains, the blocks read checkpoint slots; "live": R's stream with one chain, the
    blocks read the sampler's state after every step.  What this catches is one block handed another block's pointer or
    iteration number when all are on.  Both calls go through the same accumulate path, so a value that is wrong for a block
    in the same way in both is not seen here: the blocks' own tests against their NumPy statements catch that."""
    from gpirt_amd import gpirtMCMC
    from gpirt_amd.ops import RStream
    y = senate_slice()
    full, single, own = analyses(y)
    streams = []
    if path == "slot":
        inits = np.random.default_rng(4).normal(size=(2, y.shape[0]))
        base = lambda: dict(vote_codes=CODES, theta_init=inits, preset="fast", seed=17, chains=2, summaries=("waic",))   # noqa: E731
    else:
        th0 = np.random.default_rng(8).normal(size=y.shape[0])

        def base():
            streams.append(RStream(77))
            return dict(vote_codes=CODES, theta_init=th0, rng="reference", rstream=streams[-1], summaries=("waic",))

    everything = gpirtMCMC(y, S, BURN, **base(), **full)
    plain = gpirtMCMC(y, S, BURN, **base())           # (under R's stream: gpirt_mcmc_summary, which has no diagnostics)
    for k in ("theta", "beta", "f", "IRFs"):
        assert np.array_equal(everything[k], plain[k], equal_nan=True), k
    for name, (kw, _) in single.items():
        alone = gpirtMCMC(y, S, BURN, **base(), **kw)
        same_tree(own[name][1](everything), own[name][1](alone), (name,))
        for k in ("theta", "beta", "f", "IRFs"):
            assert np.array_equal(alone[k], plain[k], equal_nan=True), (name, k)
        same_tree(everything["summary"], alone["summary"], (name, "summary"))
        same_tree(everything["diagnostics"], alone["diagnostics"], (name, "diagnostics"))
    if path == "slot":
        same_tree(everything["summary"], plain["summary"], ("summary",))
        same_tree(everything["diagnostics"], plain["diagnostics"], ("diagnostics",))
    else:
        (mt0, i0) = streams[0].state()
        for rs in streams[1:]:
            mt, i = rs.state()
            assert i == i0 and np.array_equal(mt, mt0)
    assert everything["loo"]["T"] == (2 * S if path == "slot" else S) and everything["loo"]["M"] == (2 if path == "slot" else 1)


# block -> (the prefix of its Sampler methods, its refusal as the library words it, whether it has X_accumulate)
BLOCKS = {
    "ppc": ("ppc", "the posterior predictive checks are not enabled (gpirt_sampler_ppc_enable)", True),
    "pairs": ("ppc_pairs", "the pairwise item checks are not enabled (gpirt_sampler_ppc_pairs_enable)", False),
    "bins": ("ppc_bins", "the theta-binned item fit is not enabled (gpirt_sampler_ppc_bins_enable)", False),
    "dif": ("ppc_dif", "the group-wise item fit is not enabled (gpirt_sampler_ppc_dif_enable)", False),
    "scores": ("ppc_scores", "the score-based checks are not enabled (gpirt_sampler_ppc_scores_enable)", False),
    "person": ("ppc_person", "the person fit is not enabled (gpirt_sampler_ppc_person_enable)", False),
    "resid": ("ppc_resid", "the residual correlations are not enabled (gpirt_sampler_ppc_resid_enable)", False),
    "rank": ("rank", "the rank posteriors are not enabled (gpirt_sampler_rank_enable)", True),
    "shape": ("shape", "the shape posteriors are not enabled (gpirt_sampler_shape_enable)", True),
    "sumscore": ("sumscore", "the sum-score posteriors are not enabled (gpirt_sampler_sumscore_enable)", True),
    "equate": ("equate", "the score equating is not enabled (gpirt_sampler_equate_enable)", True),
    "loo": ("loo", "PSIS-LOO is not enabled (gpirt_sampler_loo_enable)", True),
    "order": ("shape_order", "the order posteriors are not enabled (gpirt_sampler_shape_order_enable)", False),
    "acf": ("acf", "the autocorrelation ESS is not enabled (gpirt_sampler_acf_enable)", True),
    "score": ("score", "scoring is not enabled (gpirt_sampler_score_enable)", True),
    "predict": ("score_predict", "prediction is not enabled (gpirt_sampler_score_predict_enable)", False),
}
# an add-on enabled without its base: block -> (the refusal as it reads today, the enable's arguments)
NEEDS_BASE = {
    "pairs": (BLOCKS["ppc"][1], {}),
    "bins": (BLOCKS["ppc"][1], {}),
    "dif": (BLOCKS["ppc"][1], dict(groups=np.arange(8) % 2)),
    "scores": (BLOCKS["ppc"][1], {}),
    "person": (BLOCKS["ppc"][1], {}),
    "resid": (BLOCKS["ppc"][1], {}),
    "predict": (BLOCKS["score"][1], {}),
    "order": ("the order posteriors need the shape posteriors (gpirt_sampler_shape_enable first)", {}),
}


@pytest.fixture(scope="module")
def bare(handle):
    """an 8 x 3 sampler after init() with nothing enabled"""
    from gpirt_amd import Sampler
    rng = np.random.default_rng(3)
    y = np.asfortranarray(np.where(rng.random((8, 3)) < 0.5, 1.0, -1.0))
    s = Sampler(handle, y, rng.normal(size=8), preset="fast", seed=1)
    s.init()
    yield s
    s.close()


def refused(call, text):
    from gpirt_amd import _lib
    with pytest.raises(_lib.GpirtError) as e:
        call()
    assert str(e.value) == f"[gpirt {_lib.E_ARG}] {text}", str(e.value)


@pytest.mark.parametrize("block", list(BLOCKS))
def test_not_enabled_is_refused_in_the_same_words(bare, block):
    """get, state and (where the block has one) accumulate of a block that is off, and an add-on enabled without its base"""
    prefix, text, accumulates = BLOCKS[block]
    name = {"ppc": "item_n_obs", "score": "draws"}.get(block, "counts")
    refused(lambda: getattr(bare, prefix + "_get")(name), text)
    refused(lambda: getattr(bare, prefix + "_state")(), text)
    assert hasattr(bare, prefix + "_accumulate") == accumulates
    if accumulates:
        refused(lambda: getattr(bare, prefix + "_accumulate")(), text)
    if block in NEEDS_BASE:
        text, kw = NEEDS_BASE[block]
        refused(lambda: getattr(bare, prefix + "_enable")(**kw), text)
