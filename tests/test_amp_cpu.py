"""Per-item GP amplitudes, without a GPU: the ABI, every refusal of gpirt_amp_check, the NumPy statement gpirt_amd.amp.step_exact
as a correct sampler (its transition matrix leaves the exact conditional posterior invariant), the summaries, and the near-tie
margins of the trajectory the device is compared on (tests/test_gpu_amp.py).  Bounds and cases: tests/_amp_bounds.py."""
import ctypes as C

import numpy as np
import pytest

import _amp_bounds as AB


@pytest.fixture(scope="module")
def lib():
    import os
    from gpirt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------- the ABI ---
def test_abi(lib):
    from gpirt_amd import _lib
    from gpirt_amd.sampler import Sampler
    assert lib.gpirt_version() >= 129 and _lib.ST_AMP == 10
    for name in ("gpirt_amp_check", "gpirt_sampler_amp_set", "gpirt_sampler_amp_enable", "gpirt_sampler_draw_amp",
                 "gpirt_sampler_amp_width", "gpirt_sampler_amp_record", "gpirt_sampler_amp_get", "gpirt_sampler_amp_stats"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert C.sizeof(_lib.Amp) == 8 * 19 and _lib.Amp.accept_rate.offset == 80
    for name in ("amp_set", "amp_enable", "draw_amp", "amp_width", "amp_record", "amp_get", "amp"):
        assert callable(getattr(Sampler, name)), name


def test_grid_and_default_prior(lib):
    from gpirt_amd import amp as A, ell as E
    g = A.grid()
    assert g.shape == (129,) and g[0] == 0.1 and g[-1] == 10.0 and g[64] == 1.0 and A.nearest_one(g) == 64
    assert np.array_equal(g, E.grid(0.1, 10.0, 129))                          # gpirt_ell_grid's grid
    lp = A.default_log_prior(A.grid(0.5, 2.0, 3))
    assert np.allclose(lp, [-np.log(2.0) ** 2 / 2, 0.0, -np.log(2.0) ** 2 / 2], rtol=1e-15, atol=0)
    assert A.nearest_one(A.grid(0.5, 3.0, 2)) == 0 and A.nearest_one(A.grid(0.2, 2.0, 2)) == 1


# ------------------------------------------------------------------------------------------------------ refusals ---
def _refused(word, *a, **kw):
    from gpirt_amd import _lib, amp as A
    with pytest.raises(_lib.GpirtError) as e:
        A.check_args(*a, **kw)
    assert e.value.code == _lib.E_ARG and word in str(e.value), str(e.value)


def _opts(**kw):
    from gpirt_amd import _lib
    o = _lib.default_options()
    o.rng_kind = _lib.RNG_ITEM
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_every_refusal_of_amp_check_names_its_reason(lib):
    from gpirt_amd import _lib, amp as A
    A.check_args(0.1, 10.0, 129)                                                  # the defaults pass
    A.check_args(0.01, 1000.0, 1025, np.zeros(1025), 1024, np.array([0, 1024, 7]), 3, _opts())
    for lo, hi, points, word in [(0.1, 10.0, 1, "P = 1"), (0.1, 10.0, 1026, "P = 1026"), (0.009, 10.0, 9, "<= lo < hi <="),
                                 (0.1, 1001.0, 9, "<= lo < hi <="), (2.0, 2.0, 9, "<= lo < hi <="), (3.0, 2.0, 9, "<= lo < hi <="),
                                 (float("nan"), 2.0, 9, "<= lo < hi <="), (0.1, float("inf"), 9, "<= lo < hi <="),
                                 (1.0, 1.0 + 2.0 ** -50, 1025, "strictly increasing")]:
        _refused(word, lo, hi, points)
    lp = np.zeros(9)
    lp[4] = np.inf
    _refused("log_prior[4] is not finite", 0.1, 10.0, 9, lp)
    lp[4] = np.nan
    _refused("log_prior[4] is not finite", 0.1, 10.0, 9, lp)
    _refused("width = 0", 0.1, 10.0, 9, None, 0)
    _refused("width = 9", 0.1, 10.0, 9, None, 9)
    _refused("k0[1] = 9", 0.1, 10.0, 9, None, 4, np.array([0, 9, 3]), 3)
    _refused("k0[2] = -1", 0.1, 10.0, 9, None, 4, np.array([0, 8, -1]), 3)
    _refused("R's stream has no such draw", 0.1, 10.0, 9, options=_opts(rng_kind=_lib.RNG_RSTREAM))
    _refused("kernel_fp32", 0.1, 10.0, 9, options=_opts(kernel_fp32=1))
    _refused("item shard", 0.1, 10.0, 9, m=4, options=_opts(item0=4, m_total=8))
    _refused("item shard", 0.1, 10.0, 9, m=4, options=_opts(item0=0, m_total=8))
    with pytest.raises(ValueError, match="log_prior must hold"):
        A.check_args(0.1, 10.0, 9, np.zeros(8))
    with pytest.raises(ValueError, match="k0 must hold"):
        A.check_args(0.1, 10.0, 9, None, 4, np.zeros(2, dtype=np.int32), 3)


# ------------------------------------------------------------------------------------------- the statement itself ---
def test_proposal_and_uniforms_follow_the_length_scales_rule(lib):
    from gpirt_amd import _lib, amp as A, ell as E
    from gpirt_amd.ppc import item_uniform
    assert A.proposal is E.proposal
    u0, u1 = A.uniforms(7, 3, 5)
    assert (u0, u1) == tuple(float(x) for x in item_uniform(7, 3, _lib.ST_AMP, 5, np.arange(2, dtype=np.uint64)))
    a0, a1 = A.uniforms(7, 3, np.array([4, 5, 6]))
    assert (a0[1], a1[1]) == (u0, u1) and len({*a0, *a1}) == 6


def test_the_statement_leaves_the_exact_conditional_posterior_invariant(lib):
    """P = 5, n = 12, m = 2: the full P x P transition matrix implied by step_exact's rule per item, pi T = pi against
    conditional_posterior to 1e-12 -- and step_exact's own decisions are that rule's (its acceptance frequency from every state
    and proposal is 0 or 1 on the right side of log u1)."""
    from gpirt_amd import amp as A
    c = AB.case(12, 2, 5, 3, lo=0.25, hi=4.0, nan_share=0.1)
    pi = A.conditional_posterior(c["f"], c["k"], c["mu"], c["y"], c["grid"], c["log_prior"])
    assert pi.shape == (5, 2) and np.allclose(pi.sum(axis=0), 1.0, rtol=0, atol=1e-15) and (pi > 0).all()
    for w in (1, 2, 4):
        for j in range(2):
            T = AB.transition_matrix(c["f"][:, j], c["mu"][:, j], c["y"][:, j], int(c["k"][j]), c["grid"], c["log_prior"], w)
            assert np.abs(T.sum(axis=1) - 1).max() <= 1e-15
            err = np.abs(pi[:, j].astype(AB.LD) @ T - pi[:, j]).max()
            print(f"MEASURED w={w} item {j}: max |pi T - pi| = {float(err):.3e}")
            assert err <= 1e-12
    # step_exact takes the decision the matrix's rule takes: accepted iff log u1 < the same log ratio
    for t in range(1, 40):
        r = A.step_exact(c["f"], c["mu"], c["y"], c["k"], 2, 9, t, c["grid"], c["log_prior"])
        for j in range(2):
            d = A.proposal(r["u0"][j], 2)
            assert r["k_prop"][j] == c["k"][j] + d
            if r["status"][j] == "out_of_range":
                assert not 0 <= r["k_prop"][j] < 5 and r["k"][j] == c["k"][j]
                continue
            T = AB.transition_matrix(c["f"][:, j], c["mu"][:, j], c["y"][:, j], int(c["k"][j]), c["grid"], c["log_prior"], 2)
            p_acc = T[c["k"][j], r["k_prop"][j]] * 4
            assert (r["status"][j] == "accepted") == (r["u1"][j] < p_acc)
            want = (c["grid"][r["k_prop"][j]] / c["grid"][c["k"][j]]) * c["f"][:, j] if r["status"][j] == "accepted" else c["f"][:, j]
            assert r["f"][:, j].tobytes() == want.tobytes()


def test_failed_and_prior_only_items(lib):
    """an inf in f, and an overflowing c f: failed, the column as given; an item with every cell NaN: the prior alone decides"""
    from gpirt_amd import amp as A
    c = AB.case(12, 3, 5, 4, lo=0.25, hi=4.0)
    f = c["f"].copy(order="F")
    f[3, 0] = np.inf
    f[5, 1] = 1e308
    y = c["y"].copy(order="F")
    y[:, 2] = np.nan
    seen = set()
    for t in range(1, 30):
        r = A.step_exact(f, c["mu"], y, c["k"], 1, 5, t, c["grid"], c["log_prior"])
        assert r["status"][0] == "failed" and r["nonfinite"][0] >= 1
        assert r["status"][1] == ("failed" if r["k_prop"][1] > c["k"][1] else r["status"][1])
        assert r["dll"][2] == 0 and r["log_ratio"][2] == c["log_prior"][r["k_prop"][2]] - c["log_prior"][c["k"][2]]
        for j in (0, 1):
            if r["status"][j] == "failed":
                assert r["f"][:, j].tobytes() == f[:, j].tobytes() and r["k"][j] == c["k"][j]
        seen.update(r["status"])
    assert {"failed", "accepted", "rejected"} <= seen


def test_retune_and_summarise(lib):
    from gpirt_amd import amp as A
    w = A.retune([4, 4, 4, 1, 100, 3], [0.1, 0.3, 0.6, 0.0, 0.9, np.nan], 129)
    assert w.tolist() == [2, 4, 8, 1, 128, 3]
    g = A.grid(0.5, 2.0, 5)
    draws = np.array([[[0, 4], [1, 4], [1, 3], [2, 4]], [[2, 4], [2, 4], [1, 4], [0, 2]]])          # chains x S x m
    hist = np.stack([np.bincount(draws[:, :, j].ravel(), minlength=5) for j in range(2)], axis=1)
    s = A.summarise(draws, hist, g, probs=(0.25, 0.5, 1.0))
    assert s["hist"].tolist() == hist.tolist() and np.allclose(s["mean"], [g[draws[:, :, j]].mean() for j in range(2)], rtol=1e-15)
    assert np.allclose(s["sd"], [g[draws[:, :, j]].std() for j in range(2)], rtol=1e-14)
    assert s["quantiles"][0.25].tolist() == [g[0], g[3]] and s["quantiles"][0.5].tolist() == [g[1], g[4]]
    assert s["quantiles"][1.0].tolist() == [g[2], g[4]] and s["mode"].tolist() == [g[1], g[4]]
    assert s["p_below"].shape == (5, 2) and s["p_below"][1].tolist() == [5 / 8, 0.0] and (s["p_below"][-1] == 1).all()
    assert s["rhat"].shape == s["ess"].shape == (2,)


# ------------------------------------------------------------------------------------------------- the trajectory ---
def test_the_trajectory_seed_has_no_near_tie(lib):
    """The GPU trajectory (n = 40, m = 3, P = 17, w = 2, 200 updates, seed AB.SEED): no update of any item has a margin
    |log_ratio - log u1| under 100 times the ratio bound (the one ulp of the device's log u1 counted with it), so the device may leave out no case; the chain also meets accepted,
    rejected and out-of-range updates."""
    c = AB.case(AB.N, AB.M, AB.P, AB.SEED)
    ch = AB.chain(c, AB.W, AB.UPDATES)
    print(f"MEASURED trajectory: smallest margin / e_ratio = {ch['worst_margin']:.3e} at (update, item) {ch['where']}; "
          f"counts {ch['counts'].tolist()}")
    assert ch["worst_margin"] >= AB.MARGIN
    assert (ch["counts"][0] == AB.UPDATES).all() and ch["counts"][1].min() > 0 and ch["counts"][2].sum() > 0
    assert (ch["counts"][0] - ch["counts"][1:].sum(axis=0)).min() > 0                # rejected ones, in every item
