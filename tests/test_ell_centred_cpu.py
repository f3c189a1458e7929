"""The centred length-scale update without a GPU: the ABI of library version 126, the uniforms, the NumPy statement
gpirt_amd.ell.step_exact_centred against the Gaussian density computed another way, its chain against the exact conditional
posterior, and the near-tie margins of the trajectories the device replays (tests/test_gpu_ell_centred.py).  Bounds:
tests/_ell_centred_bounds.py."""
import ctypes as C

import numpy as np
import pytest

import _ell_centred_bounds as CB


@pytest.fixture(scope="module")
def lib():
    import os
    from gpirt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def trajectory(lib):
    """the issue's case (n = 40, m = 3, 5 % NaN, 65 points, w = 4) and its NumPy chain of 4000 centred updates, computed once"""
    c = CB.chain_case()
    return c, CB.chain(c, CB.W, CB.UPDATES)


@pytest.fixture(scope="module")
def mixed(lib):
    c = CB.chain_case()
    return c, CB.mixed_chain(c, CB.W, CB.MIXED)


# -------------------------------------------------------------------------------------------------------- the ABI ---
def test_abi(lib):
    from gpirt_amd import _lib
    assert lib.gpirt_version() >= 126 and _lib.ST_ELL == 9
    vp, i32 = C.c_void_p, C.c_int
    want = {"gpirt_sampler_draw_ell_centred": (i32, [vp]), "gpirt_sampler_ell_width_centred": (i32, [vp, i32]),
            "gpirt_sampler_ell_centred_stats": (i32, [vp, C.POINTER(_lib.EllCentred)])}
    for name, sig in want.items():
        assert hasattr(lib, name) and _lib.SIGNATURES[name] == sig, name
    assert _lib.SIGNATURES["gpirt_sampler_draw_ell"] == (i32, [vp]) and _lib.SIGNATURES["gpirt_sampler_ell_width"] == (i32, [vp, i32])
    assert C.sizeof(_lib.Ell) == 8 * 19 and _lib.Ell.length_scale.offset == 80 and _lib.Ell.last_u0.offset == 104
    assert C.sizeof(_lib.EllCentred) == 8 * 16
    names = [f[0] for f in _lib.EllCentred._fields_]
    assert names == ["width", "updates", "accepted", "out_of_range", "failed", "last", "last_proposed", "factorisations", "last_u0",
                     "last_u1", "reserved"]
    assert _lib.EllCentred.last_u0.offset == 64 and _lib.EllCentred.reserved.offset == 80
    assert len(_lib.ELL_PARTS_CENTRED) == len(_lib.ELL_PARTS) == 8


def test_header_states_the_entries():
    import os
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "gpirt_hip.h")).read()
    for decl in ("int gpirt_sampler_draw_ell_centred(gpirt_sampler_t s);", "int gpirt_sampler_ell_width_centred(gpirt_sampler_t s, int w);",
                 "int gpirt_sampler_ell_centred_stats(gpirt_sampler_t s, gpirt_ell_centred* out);", "} gpirt_ell_centred;"):
        assert decl in text, decl
    assert re.search(r"GPIRT_ST_ELL = 9\s+/\*[^*]*item index 1", text)


def test_uniforms_of_the_two_kinds():
    from gpirt_amd import ell as E, ppc as PP
    for seed, t in ((11, 3), (7, 1), (2 ** 40 + 5, 1999)):
        u0, u1 = E.uniforms(seed, t, "centred")
        assert u0 == float(PP.item_uniform(seed, t, 9, 1, 0)) and u1 == float(PP.item_uniform(seed, t, 9, 1, 1))
        assert 0 < u0 < 1 and 0 < u1 < 1
        w = E.uniforms(seed, t, "whitened")
        assert w == E.uniforms(seed, t) and w == (float(PP.item_uniform(seed, t, 9, 0, 0)), float(PP.item_uniform(seed, t, 9, 0, 1)))
        assert len({u0, u1, *w}) == 4
    with pytest.raises(ValueError):
        E.uniforms(1, 1, "other")


def test_sharded_sampler_refuses_both_kinds():
    from gpirt_amd.distributed import ShardedSampler
    for kind in ("whitened", "centred"):
        with pytest.raises(ValueError, match="not offered for item shards"):
            ShardedSampler.draw_ell(object(), kind)


# ----------------------------------------------------------------------------------------------------- the update ---
def test_step_exact_centred_outcomes():
    from gpirt_amd import ell as E
    c = CB.case(24, 2, 5, 2)
    out = E.step_exact_centred(c["theta"], c["f"], 0, 0.01, 0.5, c["grid"], c["log_prior"], 2, "matern52")
    assert out["status"] == "out_of_range" and out["k"] == 0 and out["k_prop"] == -2 and "dq" not in out
    acc = E.step_exact_centred(c["theta"], c["f"], 2, 0.9, 2.0 ** -1000, c["grid"], c["log_prior"], 1)     # a tiny u1 accepts anything finite
    assert acc["status"] == "accepted" and acc["k"] == 3 and acc["k_prop"] == 3 and acc["dq"].shape == (2,)
    L, Lp = E.factor(c["theta"], "se", c["grid"][2]), E.factor(c["theta"], "se", c["grid"][3])
    assert float(np.abs(L @ acc["nu"] - c["f"]).max()) < 1e-15 and float(np.abs(Lp @ acc["nu_prop"] - c["f"]).max()) < 1e-15
    assert acc["log_ratio"] == CB.LD(-0.5) * acc["dq"].sum() - 2 * acc["dld"] + (CB.LD(c["log_prior"][3]) - CB.LD(c["log_prior"][2]))
    rej = E.step_exact_centred(c["theta"], c["f"], 2, 0.9, 1.0 - 2.0 ** -53, c["grid"], c["log_prior"] - 1e4 * np.arange(5), 1)
    assert rej["status"] == "rejected" and rej["k"] == 2 and rej["k_prop"] == 3
    bad = c["f"].copy()
    bad[3, 0] = np.nan
    fail = E.step_exact_centred(c["theta"], bad, 2, 0.9, 2.0 ** -1000, c["grid"], c["log_prior"], 1)
    assert fail["status"] == "failed" and fail["k"] == 2


@pytest.mark.parametrize("family,n,m,k,kp", [("se", 40, 3, 32, 35), ("se", 40, 3, 10, 7), ("matern52", 33, 2, 20, 24), ("matern32", 25, 4, 60, 59)])
def test_log_ratio_is_the_density_difference(family, n, m, k, kp):
    """log_ratio of step_exact_centred against sum_j log N(f_j; 0, S_k') - sum_j log N(f_j; 0, S_k) + the prior's difference, the
    densities from S itself by numpy.linalg.slogdet and solve, never through L: within the bound _ell_centred_bounds.py derives
    from the conditioning of S."""
    from gpirt_amd import ell as E, kernel as K
    c = CB.case(n, m, CB.P, 11, family)
    d = kp - k
    u0 = (d + CB.W + (0.5 if d < 0 else -0.5)) / (2 * CB.W)               # the middle of the proposal's bin of offset d
    assert E.proposal(u0, CB.W) == d
    r = E.step_exact_centred(c["theta"], c["f"], k, u0, 0.5, c["grid"], c["log_prior"], CB.W, family)
    assert r["k_prop"] == kp and r["status"] in ("accepted", "rejected")

    def log_density(ell):
        S = K.kernel_matrix(c["theta"], c["theta"], family, float(ell))
        S[np.diag_indices_from(S)] += E.JITTER
        sign, logdet = np.linalg.slogdet(S)
        assert sign == 1.0
        q = (c["f"] * np.linalg.solve(S, c["f"])).sum(axis=0)
        return -0.5 * q.sum() - 0.5 * m * logdet, np.abs(q), np.linalg.cond(S)

    (a, qa, ca), (b, qb, cb) = log_density(c["grid"][k]), log_density(c["grid"][kp])
    want = (b - a) + (c["log_prior"][kp] - c["log_prior"][k])
    tol = 4 * n * CB.U * (ca + cb) * (0.5 * float((qa + qb).sum()) + m)
    err = abs(float(r["log_ratio"]) - want)
    print(f"MEASURED {family} n={n} m={m} {k}->{kp}: log_ratio {float(r['log_ratio']):.6f}, density difference {want:.6f}, "
          f"error {err:.3e}, bound {tol:.3e} (cond {ca:.2e}, {cb:.2e})")
    assert err <= tol
    assert tol < 1e-3 * abs(want)                                         # (not vacuous: a sign or a factor 2 would be far outside)
    wrong = -0.5 * float(r["dq"].sum()) - 0.5 * m * float(r["dld"]) + (c["log_prior"][kp] - c["log_prior"][k])   # (0.5 m dld: log det L, not S)
    assert abs(wrong - want) > 100 * tol


def test_chain_visits_the_conditional_posterior(trajectory):
    """4000 centred updates with f held fixed against conditional_posterior_centred, in total variation under tv_bound of the
    chain's own ESS.  Measured on the CPU: total variation 0.0177 (bound 0.138), acceptance 0.452, ESS 1364, ten states above
    mass 1e-3."""
    from gpirt_amd import ell as E
    c, ch = trajectory
    rec = ch["records"]
    ks = np.array([r["k"] for r in rec])
    post = E.conditional_posterior_centred(c["f"], c["theta"], c["grid"], c["log_prior"], c["family"])
    freq = np.bincount(ks, minlength=c["points"]) / len(ks)
    tv = 0.5 * float(np.abs(freq - post).sum())
    ess = CB.index_ess(ks)
    bound = CB.tv_bound(post, ess)
    acc = np.mean([r["status"] == "accepted" for r in rec])
    print(f"MEASURED centred chain: TV {tv:.4f} (bound {bound:.4f}), ESS {ess:.0f} of {len(ks)}, acceptance {acc:.3f}, "
          f"states visited {int((freq > 0).sum())}, states above 1e-3: {int((post > 1e-3).sum())}")
    assert abs(post.sum() - 1) < 1e-12 and 0 < ess <= len(ks)
    assert tv <= bound
    assert bound < 0.5 and int((post > 1e-3).sum()) >= 5           # (the case exercises the update: the mass is spread)
    assert 0.5 * float(np.abs(np.eye(c["points"])[c["k"]] - post).sum()) > bound
    count = lambda st: sum(r["status"] == st for r in rec)                              # noqa: E731
    assert count("failed") == 0 and count("accepted") + count("rejected") + count("out_of_range") == len(rec)


def test_conditional_posterior_centred_is_the_stationary_law_of_the_ratio():
    """log_ratio of any move k -> k' is the difference of the log masses: detailed balance of the Metropolis rule"""
    from gpirt_amd import ell as E
    c = CB.case(24, 2, 9, 4)
    post = E.conditional_posterior_centred(c["f"], c["theta"], c["grid"], c["log_prior"], c["family"])
    for k, d, u0 in ((4, 1, 0.6), (4, -2, 0.1), (7, -1, 0.4)):
        assert E.proposal(u0, 2) == d
        r = E.step_exact_centred(c["theta"], c["f"], k, u0, 0.5, c["grid"], c["log_prior"], 2)
        assert abs(float(r["log_ratio"]) - (np.log(post[k + d]) - np.log(post[k]))) < 1e-9 * max(1.0, abs(float(r["log_ratio"])))


# ------------------------------------------------------------------------------------------------------ near-ties ---
def test_no_update_of_the_gpu_trajectories_is_a_near_tie(trajectory, mixed):
    """On the reference alone: every |log_ratio - log u1| of the 2000 centred updates and of the 500 + 500 mixed updates the device
    replays exceeds 10x the derived device-versus-reference bound on its log_ratio."""
    c, ch = trajectory
    rec = [r for r in ch["records"][:CB.GPU_UPDATES] if r["margin"] is not None]
    ratios = np.array([r["margin"] / CB.record_bound(c, r) for r in rec])
    print(f"MEASURED near-ties, centred: smallest margin {min(r['margin'] for r in rec):.3e} over {len(rec)} decided updates, "
          f"smallest margin / bound {ratios.min():.1f}")
    assert len(rec) > 0.9 * CB.GPU_UPDATES and ratios.min() > 10
    c, mx = mixed
    e_ratio, e_f, cb = CB.mixed_bounds(c, mx["records"])
    wh = np.array([r["margin"] / e_ratio for r in mx["records"] if r["kind"] == "whitened" and r["margin"] is not None])
    ce = np.array([r["margin"] / b for r, b in zip(mx["records"], cb) if b is not None])
    print(f"MEASURED near-ties, mixed: whitened bound {e_ratio:.3e}, smallest margin / bound {wh.min():.1f} over {len(wh)}; centred "
          f"smallest margin / bound {ce.min():.1f} over {len(ce)}; e_f {e_f.max():.3e}")
    assert len(wh) > 0.9 * CB.MIXED and len(ce) > 0.9 * CB.MIXED
    assert wh.min() > 10 and ce.min() > 10


def test_run_refuses_an_unknown_update():
    from gpirt_amd import ell as E
    with pytest.raises(ValueError, match="update must be"):
        E.run(np.ones((4, 2)), 2, 1, update="other")
