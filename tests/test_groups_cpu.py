"""The group posteriors on the host: gpirt_amd.groups (the NumPy statement of include/gpirt_hip.h's "group posteriors" section) on
a hand-worked example with every per-draw table entry as literals, the histogram form of U2 against the pair definition, the
reflection identity, pooling against one concatenated run, both skip rules, a constructed vote case, the order of the two lists,
every refusal and the C struct.  No device is needed."""
import ctypes as C
import re

import numpy as np
import pytest

from gpirt_amd import _lib
from gpirt_amd import groups as GR

U = 2 ** 44
INF = np.inf


def th(k):
    """grid values -5 + 0.01 k as the sampler holds them"""
    return -5.0 + np.asarray(k, dtype=np.float64) * 0.01


# ----------------------------------------------------------------------------------------------- the hand-worked example ---
CODES = np.array([0, 0, 0, 1, 1, -1, 1], dtype=np.int32)          # n = 7, respondent 5 is left out, n_0 = n_1 = 3
K1 = [500, 510, 490, 520, 510, 0, 530]
K2 = [500, 500, 500, 500, 480, 0, 500]
Y = np.array([[1, 1, 1], [-1, 1, 1], [np.nan, 1, 1], [-1, 1, 1], [-1, 1, 1], [1, 1, 1], [1, 1, 1]], dtype=np.float64)
G1_ = np.array([[INF, 0, INF], [INF, 0, INF], [INF, 0, -INF], [-INF, 0, INF], [-INF, 0, -INF], [np.nan] * 3, [-INF, 0, INF]])
G2_ = np.zeros((7, 3))
G2_[5] = np.nan


def hand_draws():
    t1, t2 = th(K1), th(K2)
    t1[5] = np.nan                                                  # a left-out respondent may hold anything
    t2[5] = 17.0
    return [GR.draw_tables(t1, G1_, Y, CODES, 2), GR.draw_tables(t2, G2_, Y, CODES, 2)]


def test_hand_worked_example_draw_one():
    la, vo = hand_draws()[0]["latent"], hand_draws()[0]["votes"]
    hist = np.zeros((3, 1001), dtype=np.uint32)
    hist[0, [490, 500, 510]] = 1
    hist[1, [510, 520, 530]] = 1
    hist[2, [490, 500, 520, 530]] = 1
    hist[2, 510] = 2
    assert np.array_equal(la["hist"], hist) and la["hist"].dtype == np.uint32
    assert la["c1"].tolist() == [0, 60, 60] and la["c2"].tolist() == [200, 1400, 1600]
    assert la["med2"].tolist() == [1000, 1040, 1020]
    assert la["w"].tolist() == [1 - 9] and la["ov"].tolist() == [3]           # one tie (510, 510): U2 = 1
    assert la["mean_order"].tolist() == [-1] and la["med_order"].tolist() == [-1]
    assert la["mean"].tolist() == [0.0, 20.0, 10.0]
    assert la["var"].tolist() == [600.0 / 9.0, 600.0 / 9.0, (6 * 1600 - 3600) / 36.0]
    assert la["a"].tolist() == [-8.0 / 9.0] and la["overlap"].tolist() == [3.0 / 9.0]
    assert la["d"].tolist() == [(0.0 - 20.0) / np.sqrt((3.0 * (600.0 / 9.0) + 3.0 * (600.0 / 9.0)) / 6.0)]
    assert la["cover"].tolist() == [True, False, False, True, False, False, False]
    assert la["share"].tolist() == [1.0, 0, 0, 1.0, 0, 0, 0]
    assert vo["e"].tolist() == [[3 * U, 3 * U // 2, 2 * U], [0, 3 * U // 2, 2 * U]] and vo["e"].dtype == np.uint64
    assert vo["side"].tolist() == [[1, 0, 1], [-1, 0, 1]]
    assert vo["support"].tolist() == [[1.0, 0.5, 2.0 / 3.0], [0.0, 0.5, 2.0 / 3.0]]
    assert vo["rice"].tolist() == [[1.0, 0.0, abs(2.0 * (2.0 / 3.0) - 1.0)], [1.0, 0.0, abs(2.0 * (2.0 / 3.0) - 1.0)]]
    assert vo["gap"].tolist() == [[1.0, 0.0, 0.0]] and vo["split"].tolist() == [[True, False, False]]
    assert vo["contested"].tolist() == [True, False, False] and vo["n_split"].tolist() == [1] and vo["c_g"].tolist() == [1, 1]
    assert vo["loy"].tolist() == [U, U, U, U, U, 0, U]
    assert vo["obs_n"].tolist() == [1, 1, 0, 1, 1, 0, 1] and vo["obs_with"].tolist() == [1, 0, 0, 1, 1, 0, 0]


def test_hand_worked_example_draw_two_and_accumulators():
    draws = hand_draws()
    la, vo = draws[1]["latent"], draws[1]["votes"]
    assert la["c1"].tolist() == [0, -20, -20] and la["c2"].tolist() == [0, 400, 400] and la["med2"].tolist() == [1000, 1000, 1000]
    assert la["w"].tolist() == [12 - 9] and la["ov"].tolist() == [6]
    assert la["mean_order"].tolist() == [1] and la["med_order"].tolist() == [0]
    assert la["var"][0] == 0.0 and la["sd"][0] == 0.0 and la["var"][1] == 800.0 / 9.0
    assert la["share"].tolist() == [2.0 / 6.0] * 3 + [0.5, 0, 0, 0.5]
    assert vo["side"].tolist() == [[0, 0, 0]] * 2 and vo["rice"].tolist() == [[0.0] * 3] * 2
    assert vo["n_split"].tolist() == [0] and vo["c_g"].tolist() == [0, 0] and vo["loy"].tolist() == [0] * 7
    raw = GR.from_tables(draws, CODES, 2, 3)
    assert (raw["latent_draws"], raw["latent_skipped"], raw["votes_draws"], raw["votes_skipped"]) == (2, 0, 2, 0)
    assert raw["order"].tolist() == [[1], [0], [1], [0], [1], [1]]
    assert raw["medhist"][0, 1000] == 2 and raw["medhist"][1, 1040] == 1 and raw["medhist"][1, 1000] == 1 and raw["medhist"].sum() == 6
    assert raw["dens_sum"][2, 510] == 2 and raw["dens_sq"][2, 510] == 4 and raw["dens_sum"][0, 500] == 4 and raw["dens_sq"][0, 500] == 10
    assert raw["ov_sum"].tolist() == [9] and raw["a_sum"].tolist() == [-8.0 / 9.0 + 3.0 / 9.0]
    assert raw["median_cover"].tolist() == [2, 1, 1, 2, 0, 0, 1]
    assert raw["split_count"].tolist() == [[1, 0, 0]] and raw["nsplit_sum"].tolist() == [1] and raw["nsplit_sq"].tolist() == [1]
    assert raw["loy_undefined"].tolist() == [1, 1] and raw["loy_sum"].tolist() == [1.0, 1, 1, 1, 1, 0, 1]
    assert raw["obs_n_sum"].tolist() == [1, 1, 0, 1, 1, 0, 1] and raw["obs_with_sum"].tolist() == [1, 0, 0, 1, 1, 0, 0]
    out = GR.finish(raw, CODES, 2, top=3)
    assert out["p_superior"][0, 1] == (1.0 + (-5.0 / 9.0) / 2.0) / 2.0 and out["p_superior"][1, 0] == 1.0 - out["p_superior"][0, 1]
    assert out["p_mean_gt"].tolist() == [[0.0, 0.5], [0.5, 0.0]] and out["p_median_gt"].tolist() == [[0.0, 0.0], [0.5, 0.0]]
    for g in range(2):
        assert abs(out["p_group_median"][CODES == g].sum() - 1.0) <= 2.0 ** -50
    assert out["loyalty"].tolist()[:5] == [1.0] * 5 and np.isnan(out["loyalty"][5])
    assert out["obs_loyalty"].tolist()[:2] == [1.0, 0.0] and np.isnan(out["obs_loyalty"][2])
    assert out["p_split"].tolist() == [[0.5, 0.0, 0.0]] and out["n_split_mean"].tolist() == [0.5]
    assert out["most_split"][0]["items"].tolist() == [0, 1, 2]
    assert out["least_loyal"]["respondents"].tolist() == [0, 1, 2]


# ------------------------------------------------------------------------------------------------------- random cases ---
def random_case(n, m, G, S, seed, chains=1):
    rng = np.random.default_rng(seed)
    codes = rng.integers(-1, G, n).astype(np.int32)
    codes[:G] = np.arange(G)
    theta = th(rng.integers(380, 620, (chains, S, n)) + 40 * np.maximum(codes, 0))
    g = rng.normal(0.0, 1.5, (chains, S, n, m)) + 0.8 * (np.maximum(codes, 0)[:, None] % 2) * np.sign(rng.normal(size=m))
    y = np.where(rng.random((n, m)) < 0.15, np.nan, np.where(rng.random((n, m)) < 0.5, 1.0, -1.0))
    return codes, theta, g, y


@pytest.mark.parametrize("n,G", [(40, 2), (61, 3), (97, 8)])
def test_u2_from_the_histogram_is_the_pair_definition(n, G):
    codes, theta, _, _ = random_case(n, 2, G, 3, 5)
    for t in range(3):
        tab = GR.latent_tables(theta[0, t], codes, G)
        ng = GR.group_sizes(codes, G)
        for p, (g, h) in enumerate(GR.pairs(G)):
            assert GR.u2_from_hist(tab["hist"][g], tab["hist"][h]) - ng[g] * ng[h] == tab["w"][p]
            assert GR.u2_from_hist(tab["hist"][h], tab["hist"][g]) - ng[g] * ng[h] == -tab["w"][p]          # antisymmetric
            ov_hg = int(np.sum(np.minimum(tab["hist"][h].astype(np.int64) * ng[g], tab["hist"][g].astype(np.int64) * ng[h])))
            assert ov_hg == tab["ov"][p] <= ng[g] * ng[h]                                                    # symmetric
        assert tab["hist"][G].sum() == ng[G] and np.array_equal(tab["hist"][:G].sum(axis=0), tab["hist"][G])


def test_an_even_sized_and_a_one_member_group():
    codes = np.array([0, 1, 1, 1, 1, 2, 2], dtype=np.int32)
    tab = GR.latent_tables(th([600, 400, 410, 430, 440, 500, 500]), codes, 3)
    assert tab["med2"].tolist() == [1200, 840, 1000, 440 + 440]     # n = 4: positions 2 and 3; all 7: position 4 twice
    st = GR.latent_draw_stats(tab, codes, 3)
    assert st["var"][0] == 0.0 and st["sd"][0] == 0.0 and st["mean"][0] == 100.0
    assert st["share"].tolist() == [1.0, 0, 0.5, 0.5, 0, 0.5, 0.5]
    assert np.isnan(st["d"][1]) and not np.isnan(st["d"][0])         # groups 0 and 2: the pooled variance is 0


def test_the_reflection_identity_holds_exactly_for_every_output_of_part_a():
    codes, theta, g, y = random_case(45, 4, 3, 6, 11, chains=2)
    a = GR.from_draws(theta, g, y, codes, signs=[1, 1], top=4)
    mirror = lambda t: th(1000 - GR.grid_k(t))        # the grid point k -> 1000 - k (negation need not land on the grid bit for bit)  # noqa: E731
    mirrored = theta.copy()
    mirrored[1] = mirror(theta[1])
    b = GR.from_draws(mirrored, g, y, codes, signs=[1, -1], top=4)
    c = GR.from_draws(mirror(theta), g, y, codes, signs=[-1, -1], top=4)
    assert a["latent_draws"] == 12
    for other in (b, c):
        for k in GR.LATENT_RAW:
            assert np.array_equal(a["raw"][k], other["raw"][k]), k
        for k in ("mean", "mean_sd", "sd_mean", "median_quantiles", "density", "density_sd", "p_superior", "p_superior_sd", "overlap",
                  "p_mean_gt", "p_median_gt", "d_mean", "d_sd", "p_group_median"):
            assert np.array_equal(a[k], other[k], equal_nan=True), k
    # and the reflection is not a no-op
    flipped = GR.from_draws(mirror(theta), g, y, codes, top=4)
    assert np.array_equal(flipped["mean"], -a["mean"]) and not np.array_equal(flipped["mean"], a["mean"])
    assert np.array_equal(flipped["p_superior"], a["p_superior"].T)


def test_pooling_two_chains_is_one_run_over_the_concatenated_draws():
    codes, theta, g, y = random_case(38, 5, 3, 5, 3, chains=2)
    two = GR.from_draws(theta, g, y, codes, top=5)
    one = GR.from_draws(theta.reshape(10, -1), g.reshape(10, 38, 5), y, codes, top=5)
    for name, dt, _ in _lib.GROUPS_RAW:
        if dt != "f8":
            assert np.array_equal(two["raw"][name], one["raw"][name]), name
        else:
            assert np.allclose(two["raw"][name], one["raw"][name], rtol=1e-13, atol=1e-13), name
    for c in GR.COUNTERS:
        assert two[c] == one[c]
    assert np.array_equal(two["p_split"], one["p_split"]) and np.array_equal(two["p_mean_gt"], one["p_mean_gt"])


def test_both_skip_rules_and_their_independence():
    codes, theta, g, y = random_case(30, 3, 2, 4, 9)
    theta, g = theta[0].copy(), g[0].copy()
    inc = np.nonzero(codes >= 0)[0]
    theta[1, inc[0]] = 0.123456                       # off the grid: draw 1 skips part A
    g[2, inc[1], 1] = np.nan                          # draw 2 skips part B
    theta[3, inc[2]] = np.nan                         # draw 3 skips part A
    g[3, inc[0], 0] = np.inf                          # +inf is taken
    out = GR.from_draws(theta, g, y, codes)
    assert (out["latent_draws"], out["latent_skipped"], out["votes_draws"], out["votes_skipped"]) == (2, 2, 3, 1)
    ref_a = GR.from_draws(theta[[0, 2]], g[[0, 2]], y, codes)
    ref_b = GR.from_draws(theta[[0, 1, 3]], g[[0, 1, 3]], y, codes)
    for k in GR.LATENT_RAW:
        assert np.array_equal(out["raw"][k], ref_a["raw"][k]), k
    for k in GR.VOTES_RAW:
        assert np.array_equal(out["raw"][k], ref_b["raw"][k]), k


def test_left_out_rows_holding_nan_change_nothing():
    codes, theta, g, y = random_case(33, 4, 3, 3, 21)
    out = GR.from_draws(theta, g, y, codes)
    left = codes < 0
    assert left.any()
    theta2, g2, y2 = theta.copy(), g.copy(), y.copy()
    theta2[..., left] = np.nan
    g2[..., left, :] = np.nan
    y2[left] = np.nan
    out2 = GR.from_draws(theta2, g2, y2, codes)
    for name, _, _ in _lib.GROUPS_RAW:
        assert out["raw"][name].tobytes() == out2["raw"][name].tobytes(), name


def test_a_constructed_vote_case():
    n, m = 24, 7
    codes = np.array([0, 1] * 12, dtype=np.int32)
    on = np.array([True, False, True, True, False, False, True])
    g = np.zeros((3, n, m))
    g[:, codes == 0] = np.where(on, 3.0, 0.0)
    g[:, codes == 1] = np.where(on, -3.0, 0.0)
    y = np.where(codes[:, None] == 0, 1.0, -1.0) * np.ones((n, m))
    y[0, 0] = -1.0                                    # one member votes against their group once
    out = GR.from_draws(np.zeros((3, n)), g, y, codes, top=4)
    assert np.array_equal(out["p_split"][0], on.astype(float))
    e = GR.votes_tables(g[0], codes, 2)
    st = GR.votes_draw_stats(e, GR.group_sizes(codes, 2))
    assert np.array_equal(e[:, ~on], np.full((2, 3), 12 * 2 ** 43, dtype=np.uint64))      # 2 e = n_g 2^44 exactly
    assert np.array_equal(st["side"][:, ~on], np.zeros((2, 3))) and np.array_equal(out["rice"][:, ~on], np.zeros((2, 3)))
    assert st["side"][0, on].tolist() == [1] * 4 and st["side"][1, on].tolist() == [-1] * 4
    plogis3 = 1.0 / (1.0 + np.exp(-3.0))
    assert np.all(np.abs(out["loyalty"] - plogis3) <= 2.0 ** -45)   # every term is p 2^44 rounded to an integer
    assert out["n_split_mean"][0] == 4.0 and out["n_split_sd"][0] == 0.0
    assert out["obs_loyalty"][0] == 0.75 and np.all(out["obs_loyalty"][1:] == 1.0)
    assert out["most_split"][0]["items"].tolist() == [0, 2, 3, 6]


def test_the_order_of_both_lists():
    raw = GR.empty_raw(6, 5, 2)
    codes = np.array([0, 0, 1, 1, -1, 1], dtype=np.int32)
    raw["votes_draws"] = 4
    raw["split_count"][0] = [2, 4, 2, 0, 4]
    raw["loy_sum"][:] = [3.0, 2.0, 2.0, 1.0, 0.0, 2.0]
    raw["loy_undefined"][:] = [0, 2]
    out = GR.finish(raw, codes, 2, top=6)
    assert out["most_split"][0]["items"].tolist() == [1, 4, 0, 2, 3, -1]
    assert out["most_split"][0]["p_split"].tolist()[:5] == [1.0, 1.0, 0.5, 0.5, 0.0] and np.isnan(out["most_split"][0]["p_split"][5])
    # loyalty: 0.75, 0.5 | 1.0, 0.5, 1.0 (group 1 has two defined draws); ties to the lowest i, the left-out respondent never
    assert out["least_loyal"]["respondents"].tolist() == [1, 3, 0, 2, 5, -1]
    assert out["least_loyal"]["loyalty"].tolist()[:5] == [0.5, 0.5, 0.75, 1.0, 1.0]


# ------------------------------------------------------------------------------------------------------ the contract ---
def test_every_refusal():
    ok = np.array([0, 1, -1, 1], dtype=np.int32)
    codes, G = GR.check_groups(ok, 4, 3)
    assert G == 2 and codes.dtype == np.int32
    for groups, n, m, word in ((None, 4, 3, "no group codes"), ([0, 1, 1], 4, 3, "one code per respondent"),
                               ([0.5, 1, 0, 1], 4, 3, "must be integers"), ([0, 1, -2, 1], 4, 3, "below -1"),
                               ([0, 0, 0, 0], 4, 3, "1 groups given"), ([0, 1, 3, 3], 4, 3, "group 2 has no member"),
                               (list(range(9)), 9, 3, "9 groups given"), ([0, 1, 0, 1], 4, 4097, "m = 4097"),
                               ([0, 1] * 32768, 65536, 3, "n = 65536")):
        with pytest.raises(ValueError, match=re.escape(word)):
            GR.check_groups(groups, n, m)
    for top in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match="top must be an integer in 1 .. 64"):
            GR.check_top(top)
    with pytest.raises(ValueError, match="signs"):
        GR.pool([GR.empty_raw(3, 2, 2)], signs=[0])
    lib = _lib.load()
    p = lambda a: np.asarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
    sizes = (C.c_int64 * 9)()
    assert lib.gpirt_groups_check(4, 3, 2, p(ok), 20, sizes) == 0 and list(sizes) == [1, 2, 3, 0, 0, 0, 0, 0, 0]
    assert lib.gpirt_groups_check(8, 3, 8, p(range(8)), 64, None) == 0
    big = np.zeros(65535, dtype=np.int32)
    big[0] = 1
    for n, m, G, groups, top, word in ((65535, 3, 2, big, 20, "n = 65535"), (0, 3, 2, ok, 20, "n = 0"), (4, 4097, 2, ok, 20, "m = 4097"),
                                       (4, 0, 2, ok, 20, "m = 0"), (4, 3, 1, ok, 20, "1 groups given"), (4, 3, 9, ok, 20, "9 groups given"),
                                       (4, 3, 2, ok, 0, "top = 0"), (4, 3, 2, ok, 65, "top = 65"), (4, 3, 3, ok, 20, "group 2 has no member"),
                                       (4, 3, 2, [0, 1, 2, 1], 20, "the code 2 of respondent 2"),
                                       (4, 3, 2, [0, 1, -2, 1], 20, "the code -2 of respondent 2")):
        assert lib.gpirt_groups_check(n, m, G, p(groups), top, None) == _lib.E_ARG and word in _lib.last_error(), word
        assert _lib.last_error().startswith("groups: ")            # its own wording, not the DIF block's
    assert lib.gpirt_groups_check(4, 3, 2, None, 20, None) == _lib.E_ARG
    r, _ = GR.struct(4, 3, 2, top=3)
    assert lib.gpirt_groups_combine(None, 1, None, None, C.byref(r)) == _lib.E_ARG
    assert lib.gpirt_sampler_groups_enable(None, 2, p(ok), 20, 1) == _lib.E_ARG
    assert lib.gpirt_sampler_groups_accumulate(None) == _lib.E_ARG
    assert lib.gpirt_sampler_groups_get(None, b"counts", None, 0) == _lib.E_ARG
    assert lib.gpirt_sampler_groups_state(None, None, None) == _lib.E_ARG


def test_the_sharded_sampler_refuses():
    from gpirt_amd.distributed import ShardedSampler
    with pytest.raises(ValueError, match="group posteriors are not offered for item shards"):
        ShardedSampler.groups_enable(None, [0, 1])


def test_c_abi_of_version_127():
    import os
    lib = _lib.load()
    assert lib.gpirt_version() >= 127
    for name in ("gpirt_groups_check", "gpirt_sampler_groups_enable", "gpirt_sampler_groups_accumulate", "gpirt_sampler_groups_get",
                 "gpirt_sampler_groups_state", "gpirt_groups_combine"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    S = _lib.Groups
    assert C.sizeof(S) == 8 * (1 + 32 + 4 + 6 + 4 + 9 + 4) == 480
    assert (S.top.offset, S.raw.offset, S.most_split_items.offset, S.least_loyal_loyalty.offset) == (0, 8, 264, 288)
    assert (S.n.offset, S.chains.offset, S.latent_draws.offset, S.group_size.offset, S.reserved.offset) == (296, 336, 344, 376, 448)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpirt_hip.h")).read()
    body = re.search(r"typedef struct gpirt_groups \{(.*?)\} gpirt_groups;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:\[[^\]]*\])?\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in S._fields_]
    defs = dict(re.findall(r"#define\s+(GPIRT_GROUPS_\w+)\s+(\d+)", src))
    assert int(defs["GPIRT_GROUPS_NARRAYS"]) == len(_lib.GROUPS_RAW) == 32
    for k, (name, _, _) in enumerate(_lib.GROUPS_RAW):
        assert int(defs["GPIRT_GROUPS_" + name.upper()]) == k, name
    assert (int(defs["GPIRT_GROUPS_MAX_G"]), int(defs["GPIRT_GROUPS_MAX_N"]), int(defs["GPIRT_GROUPS_MAX_M"]),
            int(defs["GPIRT_GROUPS_MAX_TOP"]), int(defs["GPIRT_GROUPS_MED_BINS"])) == (8, 65534, 4096, 64, 2001)
    # gpirt_run is untouched: the block is stage API only
    assert len(_lib.Run._fields_) == 17
