"""The length scale as a parameter of the chain, without a GPU: gpirt_ell_grid, every refusal of gpirt_ell_check, the proposal,
the NumPy statement gpirt_amd.ell.step_exact chained against the exact conditional posterior, and the near-tie margins of the
trajectory the device is compared on (tests/test_gpu_ell.py).  Bounds: tests/_ell_bounds.py."""
import ctypes as C

import numpy as np
import pytest

import _ell_bounds as EB

UPDATES, GPU_UPDATES = 4000, 2000


@pytest.fixture(scope="module")
def lib():
    import os
    from gpirt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def trajectory(lib):
    """the issue's case (n = 40, m = 3, P = 17, w = 2, 5 % NaN) and its NumPy chain of 4000 updates, computed once"""
    c = EB.case(EB.N, EB.M, EB.P, EB.SEED)
    return c, EB.chain(c, EB.W, UPDATES)


# ------------------------------------------------------------------------------------------------------- the grid ---
def test_abi(lib):
    from gpirt_amd import _lib
    assert lib.gpirt_version() >= 125 and _lib.ST_ELL == 9
    for name in ("gpirt_ell_grid", "gpirt_ell_check", "gpirt_sampler_ell_enable", "gpirt_sampler_draw_ell",
                 "gpirt_sampler_ell_width", "gpirt_sampler_ell_get", "gpirt_sampler_ell_stats"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert C.sizeof(_lib.Ell) == 8 * 19 and _lib.Ell.length_scale.offset == 80


@pytest.mark.parametrize("lo,hi,points", [(0.25, 4.0, 129), (0.01, 1000.0, 1025), (0.7, 3.0, 2), (0.3, 0.31, 1025), (1.0, 7.0, 33)])
def test_grid(lib, lo, hi, points):
    from gpirt_amd import ell as E
    g = E.grid(lo, hi, points)
    assert g.shape == (points,) and g[0] == lo and g[-1] == hi                  # the end points exactly
    assert (np.diff(g) > 0).all()
    k = np.arange(points, dtype=EB.LD)
    ref = EB.LD(lo) * (EB.LD(hi) / EB.LD(lo)) ** (k / EB.LD(points - 1))
    assert (np.abs(g.astype(EB.LD) - ref) <= 2.0 ** -52 * ref).all()


def test_grid_hits_the_default_kernel_at_the_default_arguments():
    from gpirt_amd import ell as E
    assert E.grid()[64] == 1.0 and E.default_log_prior(E.grid())[64] == 0.0
    lp = E.default_log_prior(E.grid(0.5, 2.0, 3))
    assert np.allclose(lp, [-np.log(2.0) ** 2 / 2, 0.0, -np.log(2.0) ** 2 / 2], rtol=1e-15, atol=0)


@pytest.mark.parametrize("lo,hi,points,word", [
    (0.25, 4.0, 1, "points"), (0.25, 4.0, 1026, "points"), (0.009, 4.0, 9, "lo"), (0.25, 1001.0, 9, "lo"), (2.0, 2.0, 9, "lo"),
    (3.0, 2.0, 9, "lo"), (float("nan"), 2.0, 9, "lo"), (0.25, float("inf"), 9, "lo"), (1.0, 1.0 + 2.0 ** -50, 1025, "strictly")])
def test_grid_refusals(lib, lo, hi, points, word):
    from gpirt_amd import _lib, ell as E
    with pytest.raises(_lib.GpirtError) as e:
        E.grid(lo, hi, points)
    assert e.value.code == _lib.E_ARG and word in str(e.value)
    assert lib.gpirt_ell_grid(0.25, 4.0, 9, None) == _lib.E_ARG


# ------------------------------------------------------------------------------------------------------ refusals ---
def _refused(word, *a, **kw):
    from gpirt_amd import _lib, ell as E
    with pytest.raises(_lib.GpirtError) as e:
        E.check_args(*a, **kw)
    assert e.value.code == _lib.E_ARG and word in str(e.value), str(e.value)


def _opts(**kw):
    from gpirt_amd import _lib
    o = _lib.default_options()
    o.rng_kind = _lib.RNG_ITEM
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_check_refusals_that_need_no_device(lib):
    from gpirt_amd import _lib, ell as E
    E.check_args(0.25, 4.0, 129)                                                 # the defaults pass
    E.check_args(0.25, 4.0, 129, np.zeros(129), 128, 128, kernel="se", options=_opts(), m=7)
    _refused("points", 0.25, 4.0, 1)
    lp = np.zeros(17)
    lp[3] = np.inf
    _refused("log_prior[3]", 0.25, 4.0, 17, lp)
    lp[3] = np.nan
    _refused("log_prior[3]", 0.25, 4.0, 17, lp)
    with pytest.raises(ValueError):
        E.check_args(0.25, 4.0, 17, np.zeros(16))
    for w in (0, -1, 17):
        _refused("width", 0.25, 4.0, 17, None, w)
    E.check_args(0.25, 4.0, 17, None, 16)
    for k0 in (-2, 17):
        _refused("k0", 0.25, 4.0, 17, None, 2, k0)
    _refused("R's stream has no such draw", 0.25, 4.0, 17, options=_opts(rng_kind=_lib.RNG_RSTREAM))
    _refused("kernel_fp32", 0.25, 4.0, 17, options=_opts(kernel_fp32=1))
    _refused("item shard", 0.25, 4.0, 17, options=_opts(item0=4, m_total=12), m=4)
    _refused("item shard", 0.25, 4.0, 17, options=_opts(item0=0, m_total=12), m=4)
    E.check_args(0.25, 4.0, 17, options=_opts(item0=0, m_total=4), m=4)
    # the handle's length scale must be a point of the grid
    _refused("not a point of the grid", 0.25, 4.0, 17, kernel=dict(family="se", length_scale=1.1))
    _refused("not a point of the grid", 0.3, 4.0, 17, kernel="matern52")
    g = E.grid(0.3, 4.0, 17)
    E.check_args(0.3, 4.0, 17, kernel=dict(family="matern52", length_scale=float(g[5])))
    # kstar_rank: the certificate at ell_0 = lo decides; a Matern family needs kstar_rank = 0
    fast = dict(fstar_fused=1, kstar_rank=64)
    _refused("kstar_rank", 0.25, 4.0, 17, kernel="se", options=_opts(**fast))
    E.check_args(0.7, 2.8, 3, width=1, kernel=dict(family="se", length_scale=float(E.grid(0.7, 2.8, 3)[1])), options=_opts(**fast))
    E.check_args(0.25, 4.0, 17, kernel="se", options=_opts(fstar_fused=1, kstar_rank=0))
    _refused("Matern", 0.5, 2.0, 3, width=1, kernel="matern32", options=_opts(**fast))
    E.check_args(0.5, 2.0, 3, width=1, kernel="matern32", options=_opts(fstar_fused=1))


def test_sharded_sampler_refuses():
    """(the refusal needs no device and no process group: the methods raise before they look at the sampler)"""
    from gpirt_amd.distributed import ShardedSampler
    for call in (ShardedSampler.ell_enable, ShardedSampler.draw_ell):
        with pytest.raises(ValueError, match="not offered for item shards"):
            call(object())


def test_the_certificate_grows_as_the_length_scale_shrinks():
    """why passing at lo covers the grid: at five grid points between lo and hi the rank-64 certificate never falls as ell does"""
    from gpirt_amd import ell as E, kernel as K
    g = E.grid(0.5, 4.0, 129)
    cert = [K.rank_certificate("se", float(g[k]), 64)["certificate"] for k in (0, 32, 64, 96, 128)]
    print("MEASURED certificates at lo .. hi:", " ".join(f"{v:.2e}" for v in cert))
    line = K.rank_certificate("se", 1.0, 48)["certificate"]
    assert cert[0] > line                                       # refused at lo = 0.5 ...
    assert all(a >= b or max(a, b) <= line for a, b in zip(cert, cert[1:]))      # ... and monotone down to rounding


# ------------------------------------------------------------------------------------------------------ proposal ---
@pytest.mark.parametrize("w", [1, 2, 7])
def test_proposal_is_symmetric(w):
    """2w equal bins of u0: every non-zero offset in -w .. w once, 0 never; the bins' edges belong to the upper bin"""
    from gpirt_amd import ell as E
    mids = [E.proposal((j + 0.5) / (2 * w), w) for j in range(2 * w)]
    assert sorted(mids) == [d for d in range(-w, w + 1) if d != 0]
    assert [E.proposal(j / (2 * w), w) for j in range(2 * w)] == mids
    assert E.proposal(np.nextafter(1.0, 0.0), w) == w and E.proposal(1.0, w) == w and E.proposal(2.0 ** -53, w) == -w
    assert sorted(-d for d in mids) == sorted(mids)


def test_uniforms_are_the_item_rng_at_stage_9():
    from gpirt_amd import ell as E, ppc as PP
    u0, u1 = E.uniforms(11, 3)
    assert u0 == float(PP.item_uniform(11, 3, 9, 0, 0)) and u1 == float(PP.item_uniform(11, 3, 9, 0, 1))
    assert 0 < u0 < 1 and 0 < u1 < 1 and E.uniforms(11, 4) != (u0, u1)


# ----------------------------------------------------------------------------------------------------- the chain ---
def test_step_exact_outcomes():
    from gpirt_amd import ell as E
    c = EB.case(24, 2, 5, 2)
    args = (c["theta"], c["f"], c["mu"], c["y"])
    out = E.step_exact(*args, 0, 0.01, 0.5, c["grid"], c["log_prior"], 2, "matern52")
    assert out["status"] == "out_of_range" and out["k"] == 0 and out["k_prop"] == -2 and out["f"] is not None
    acc = E.step_exact(*args, 2, 0.9, 2.0 ** -60, c["grid"], c["log_prior"], 1)            # a tiny u1 accepts anything finite
    assert acc["status"] == "accepted" and acc["k"] == 3
    assert np.array_equal(acc["f"], acc["f_prop"].astype(np.float64))
    Lp = E.factor(c["theta"], "se", c["grid"][3])
    assert float(np.abs(Lp @ acc["nu"] - acc["f_prop"]).max()) == 0.0
    rej = E.step_exact(*args, 2, 0.9, 1.0 - 2.0 ** -53, c["grid"], c["log_prior"] - 50.0 * np.arange(5), 1)
    assert rej["status"] == "rejected" and rej["k"] == 2 and rej["f"] is not acc["f"] and np.array_equal(rej["f"], c["f"])
    bad = c["f"].copy()
    bad[np.argwhere(~np.isnan(c["y"]))[0][0], 0] = np.nan
    fail = E.step_exact(c["theta"], bad, c["mu"], c["y"], 2, 0.9, 2.0 ** -60, c["grid"], c["log_prior"], 1)
    assert fail["status"] == "failed" and fail["k"] == 2


def test_chain_visits_the_conditional_posterior(trajectory):
    """4000 updates with nu held fixed (no step() in between): the visit frequencies against conditional_posterior, within the
    bound tests/_ell_bounds.py derives from the chain's ESS.  Measured on the CPU: total variation 0.0204, acceptance 0.506, ESS
    printed; drift max |f - L_k nu| 2.6e-14."""
    from gpirt_amd import ell as E
    c, ch = trajectory
    ks = np.array([r["k"] for r in ch["records"]])
    post = E.conditional_posterior(ch["nu0"], c["theta"], c["mu"], c["y"], c["grid"], c["log_prior"], c["family"])
    freq = np.bincount(ks, minlength=c["points"]) / len(ks)
    tv = 0.5 * float(np.abs(freq - post).sum())
    ess = EB.index_ess(ks)
    bound = EB.tv_bound(post, ess)
    acc = np.mean([r["status"] == "accepted" for r in ch["records"]])
    drift = float(np.abs(ch["f"].astype(EB.LD) - ch["cache"][ch["k"]] @ ch["nu0"]).max())
    print(f"MEASURED chain: TV {tv:.4f} (bound {bound:.4f}), ESS {ess:.0f} of {len(ks)}, acceptance {acc:.3f}, "
          f"states visited {int((freq > 0).sum())}, drift {drift:.2e}")
    assert abs(post.sum() - 1) < 1e-12 and 0 < ess <= len(ks)
    assert tv <= bound
    assert bound < 0.5                                           # (not vacuous: a chain stuck in one state is far outside)
    assert 0.5 * float(np.abs(np.eye(c["points"])[c["k"]] - post).sum()) > bound
    assert drift <= 2 * UPDATES * (2 * c["n"] + 1) * EB.U * EB.worst_constants(c)["kF"] * np.sqrt(c["n"]) * \
        float(np.abs(ch["nu0"]).max()) * EB.worst_constants(c)["L2"]


def test_no_update_of_the_gpu_trajectory_is_a_near_tie(trajectory):
    """On the reference alone: every |log_ratio - log u1| of the 2000 updates the device replays is at least 10x the derived
    device-versus-reference bound on log_ratio, so no update has to be left out of that comparison (cap 0)."""
    c, ch = trajectory
    rec = ch["records"][:GPU_UPDATES]
    margins = np.array([r["margin"] for r in rec if r["margin"] is not None])
    bound, _ = EB.trajectory_ratio_bound(c, ch["nu0"], GPU_UPDATES)
    print(f"MEASURED near-ties: smallest margin {margins.min():.3e} over {len(margins)} decided updates, "
          f"bound on log_ratio {bound:.3e} (x10 = {10 * bound:.3e})")
    assert len(margins) > 0.9 * GPU_UPDATES
    assert int((margins < 10 * bound).sum()) == 0
