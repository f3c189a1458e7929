"""gpirt_amd.ranks.from_draws -- the NumPy statement of the rank posteriors' contract (include/gpirt_hip.h, "rank
posteriors") -- against a brute force built from np.sort and searchsorted per draw, its exact reflection rule, the
histogram's bin scheme and the pivots' shares; and the C ABI of library version 108 on a machine without a device."""
import math

import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
INT_FIELDS = ("rank2_sum", "rank2_sumsq", "rank_hist", "pivot_cover", "lt", "draws", "skipped_draws", "pivots")
DBL_FIELDS = ("rank_mean", "rank_var", "rank_quantiles", "p_less", "pivot_share", "p_pivot")


def grid(k):
    return -5.0 + np.asarray(k).astype(np.float64) * 0.01


def constructed_draws(n, seed=0):
    """(S, n) theta draws on the grid: heavy ties (5 distinct values), all equal, a strict order, a reversed strict order,
    one draw with an off-grid value, one with a NaN (both skipped), a random one with some ties."""
    rng = np.random.default_rng(seed)
    k = [rng.integers(498, 503, n), np.full(n, 700), rng.permutation(n) + 100, (rng.permutation(n) + 100)[::-1],
         rng.integers(0, 1001, n), rng.integers(400, 400 + max(2, n // 2), n), rng.integers(0, 1001, n)]
    th = grid(np.stack(k))
    th[4, n // 3] = 0.123456                 # off the grid
    th[6, 0] = np.nan
    return th


def brute_bins(n):
    """The header's bin rule restated: the smallest odd w with ceil((2n - 1) / w) <= 1025, B made odd, the padding split."""
    span = 2 * n - 1
    w = next(w for w in range(1, span + 2, 2) if math.ceil(span / w) <= 1025)
    B = math.ceil(span / w)
    B += 1 - B % 2
    assert (B * w - span) % 2 == 0
    return B, w, (B * w - span) // 2


def brute_pivots(n, pivots):
    """The header's pivot rule restated: "median" is (n + 1) / 2 for odd n, n / 2 and n / 2 + 1 for even n; the set is
    closed under q <-> n + 1 - q and sorted."""
    qs = set()
    for q in pivots:
        if q == "median":
            qs |= {(n + 1) // 2} if n % 2 else {n // 2, n // 2 + 1}
        else:
            qs.add(q)
    return sorted(qs | {n + 1 - q for q in qs})


def brute(theta, pivots, probs, pairwise=True):
    """One chain (S, n), straight from the definitions (nothing of the module under test)."""
    S_all, n = theta.shape
    closed = brute_pivots(n, pivots)
    B, w, pad = brute_bins(n)
    s1, s2 = [0] * n, [0] * n
    hist = np.zeros((n, B), dtype=np.uint32)
    cover = np.zeros((len(closed), n), dtype=np.uint32)
    share = np.zeros((len(closed), n))
    lt = np.zeros((n, n), dtype=np.uint32)
    r2_all = []
    S = skipped = 0
    for t in theta:
        k = np.rint((t + 5.0) * 100.0)
        with np.errstate(invalid="ignore"):
            if not ((k >= 0) & (k <= 1000) & (-5.0 + k * 0.01 == t)).all():
                skipped += 1
                continue
        S += 1
        srt = np.sort(k)
        less = np.searchsorted(srt, k, "left")
        eq = np.searchsorted(srt, k, "right") - less
        r2 = 2 * less + eq + 1
        r2_all.append(r2)
        for i in range(n):
            s1[i] += int(r2[i])
            s2[i] += int(r2[i]) ** 2
            hist[i, (int(r2[i]) - 2 + pad) // w] += 1
            for p, q in enumerate(closed):
                if less[i] < q <= less[i] + eq[i]:
                    cover[p, i] += 1
                    share[p, i] += 1.0 / eq[i]
            for j in range(n):
                lt[i, j] += k[i] < k[j]
    r2_all = np.sort(np.array(r2_all), axis=0)
    rq = np.array([[0.5 * (2 - pad + ((int(r2_all[max(1, math.ceil(q * S)) - 1, i]) - 2 + pad) // w + 1) * w - 1)
                    for i in range(n)] for q in probs])
    mean = np.array([a / (2.0 * S) for a in s1])
    var = np.array([float(S * b - a * a) / (4.0 * S * (S - 1)) for a, b in zip(s1, s2)])
    return dict(rank2_sum=np.array(s1, dtype=np.uint64), rank2_sumsq=np.array(s2, dtype=np.uint64), rank_hist=hist,
                pivot_cover=cover, pivot_share=share, p_pivot=share / S, lt=lt, p_less=lt / np.float64(S), draws=S,
                skipped_draws=skipped, pivots=np.array(closed), rank_mean=mean, rank_var=var, rank_quantiles=rq)


def assert_same(got, want, fields=INT_FIELDS + DBL_FIELDS):
    for f in fields:
        a, b = got[f], want[f]
        if b is None:
            assert a is None, f
            continue
        assert np.asarray(a).dtype.kind == np.asarray(b).dtype.kind or np.isscalar(b), (f, np.asarray(a).dtype)
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), f


@pytest.mark.parametrize("n", [2, 7, 12, 33])
def test_from_draws_against_brute_force(n):
    """Odd and even n; heavy ties, all equal, strict orders, an off-grid value and a NaN (each skips its draw)."""
    from gpirt_amd import ranks
    th = constructed_draws(n, seed=n)
    pivots = ["median", 1, min(3, n)]
    probs = (0.0, 0.025, 0.5, 0.8, 0.975, 1.0)
    got = ranks.from_draws(th, pivots, probs, pairwise=True)
    want = brute(th, pivots, probs)
    assert want["draws"] == 5 and want["skipped_draws"] == 2
    assert_same(got, want)
    assert got["rank_bin_width"] == 0.5
    # the all-equal draw alone: everyone has the mid-rank (n + 1) / 2 and covers every position with share 1 / n
    one = ranks.from_draws(th[1:2], pivots, probs, pairwise=True)
    assert np.array_equal(one["rank_mean"], np.full(n, (n + 1) / 2.0)) and not one["lt"].any()
    assert np.array_equal(one["pivot_cover"], np.ones_like(one["pivot_cover"]))
    assert np.array_equal(one["pivot_share"], np.full(one["pivot_share"].shape, 1.0 / n))
    assert np.isnan(one["rank_var"]).all()
    # a strict order alone: rank_mean is the rank, lt is the order's indicator, ties are none
    strict = ranks.from_draws(th[2:3], pivots, probs, pairwise=True)
    assert np.array_equal(np.sort(strict["rank_mean"]), np.arange(1, n + 1, dtype=np.float64))
    assert np.array_equal(strict["lt"] + strict["lt"].T + np.eye(n, dtype=np.uint32), np.ones((n, n), dtype=np.uint32))
    assert np.array_equal(strict["order"], np.argsort(th[2]))
    # without pairwise: no lt, everything else as before
    plain = ranks.from_draws(th, pivots, probs)
    assert plain["lt"] is None and plain["p_less"] is None
    assert_same(plain, want, tuple(f for f in INT_FIELDS + DBL_FIELDS if f not in ("lt", "p_less")))


def test_chains_pool_in_order():
    """(C, S, n): the integers add over the chains; one chain of all draws gives the same integers."""
    from gpirt_amd import ranks
    n = 12
    th = np.stack([constructed_draws(n, seed=c) for c in range(3)])
    pooled = ranks.from_draws(th, ("median", 2), pairwise=True)
    flat = ranks.from_draws(th.reshape(1, -1, n), ("median", 2), pairwise=True)
    assert_same(pooled, flat, INT_FIELDS + ("rank_mean", "rank_var", "rank_quantiles", "p_less"))
    assert pooled["draws"] == 15 and pooled["skipped_draws"] == 6


@pytest.mark.parametrize("n", [7, 12])
def test_reflection_identity(n):
    """from_draws of the reflected draws (grid index k -> 1000 - k: theta -> -theta on the grid) equals from_draws of the
    draws with sign -1, field for field and bit for bit: reversed histogram, swapped pivots, transposed lt."""
    from gpirt_amd import ranks
    from gpirt_amd.quantiles import grid_index
    th = np.stack([constructed_draws(n, seed=40 + c) for c in range(2)])
    k = grid_index(th)
    mirrored = np.where(k >= 0, grid(1000 - k), th)        # what is off the grid stays off it
    assert np.array_equal(grid_index(mirrored), np.where(k >= 0, 1000 - k, -1))
    pivots, probs = ("median", 2), (0.025, 0.5, 0.975)
    for signs in ([-1, -1], [1, -1]):
        direct = ranks.from_draws(np.stack([mirrored[c] if s < 0 else th[c] for c, s in enumerate(signs)]), pivots, probs,
                                  pairwise=True)
        by_sign = ranks.from_draws(th, pivots, probs, signs=signs, pairwise=True)
        assert_same(by_sign, direct)
    both = ranks.from_draws(th, pivots, probs, signs=[-1, -1], pairwise=True)
    plain = ranks.from_draws(th, pivots, probs, pairwise=True)
    assert np.array_equal(both["rank_hist"], plain["rank_hist"][:, ::-1])
    assert np.array_equal(both["pivot_cover"], plain["pivot_cover"][::-1]) and np.array_equal(both["lt"], plain["lt"].T)
    assert np.array_equal(both["rank_mean"], (n + 1) - plain["rank_mean"])
    # a chain pooled with its own mirror image is symmetric: everyone's mean rank is (n + 1) / 2, exactly
    sym = ranks.from_draws(np.stack([th[0], th[0]]), pivots, probs, signs=[1, -1], pairwise=True)
    assert np.array_equal(sym["rank_mean"], np.full(n, (n + 1) / 2.0))
    assert np.array_equal(sym["lt"], sym["lt"].T)


@pytest.mark.parametrize("n", [2, 3, 100, 512, 513, 8192, 16384])
def test_bin_scheme_is_symmetric(n):
    from gpirt_amd.ranks import bin_scheme
    B, w, pad = bin_scheme(n)
    span = 2 * n - 1
    assert w % 2 == 1 and B % 2 == 1 and (B * w) % 2 == 1 and B <= 1025
    assert 2 * pad == B * w - span and pad >= 0
    assert -(-span // w) <= 1025 and (w == 1 or -(-span // (w - 2)) > 1025)          # the smallest odd width
    assert (n > 512) or (w == 1 and pad <= 1)
    r2 = np.arange(2, 2 * n + 1)
    b = (r2 - 2 + pad) // w
    assert b.min() >= 0 and b.max() <= B - 1
    assert np.array_equal((2 * n + 2 - r2 - 2 + pad) // w, B - 1 - b)


@pytest.mark.parametrize("n", [7, 12, 33])
def test_pivot_shares_sum_to_one(n):
    """In every counted draw exactly eq_i respondents with share 1 / eq_i cover a position: sum_i p_pivot[q, i] = 1 within
    S n eps (S n terms, each within eps / 2 of its value, summed)."""
    from gpirt_amd import ranks
    th = constructed_draws(n, seed=3)
    out = ranks.from_draws(th, list(range(1, min(n, 16) + 1)))
    S = out["draws"]
    assert out["pivots"].tolist() == sorted(set(range(1, min(n, 16) + 1)) | {n + 1 - q for q in range(1, min(n, 16) + 1)})
    assert np.abs(out["p_pivot"].sum(axis=1) - 1.0).max() <= S * n * EPS
    assert (out["pivot_cover"].sum(axis=1) >= S).all()


@pytest.mark.parametrize("n", [2, 3, 7, 100, 512, 513, 1000, 8192, 16384])
def test_bin_scheme_and_pivots_against_their_restatement(n):
    from gpirt_amd import ranks
    assert ranks.bin_scheme(n) == brute_bins(n)
    for pivots in (["median"], [1], ["median", 1, min(3, n)], list(range(1, min(n, 16) + 1))):
        assert ranks.close_pivots(n, pivots)[1] == brute_pivots(n, pivots), pivots


def test_struct_takes_a_closed_set_of_up_to_32_positions():
    """Sixteen asymmetric positions close to 32: gpirt_rank_combine's struct is sized by the closed set of the state block
    and is not held to the 16 positions a caller may give."""
    from gpirt_amd import ranks
    n = 100
    given, closed = ranks.close_pivots(n, list(range(1, 17)))
    assert len(given) == 16 and len(closed) == 32
    r, arrays = ranks.struct(n, list(range(1, 17)))
    assert r.n_pivots == 16 and arrays["p_pivot"].shape == (32, n)
    r, arrays = ranks.struct(n, None, closed=closed)
    assert r.n_pivots == 0 and arrays["p_pivot"].shape == (32, n) and arrays["pivot_cover"].shape == (32, n)
    with pytest.raises(ValueError):
        ranks.struct(n, list(range(1, 18)))
    with pytest.raises(ValueError):
        ranks.struct(n, None, closed=list(range(1, 34)))


@pytest.mark.parametrize("bad", ["median", (41, 60), 1, [1, 2], dict(pivot=(1,))])
def test_gpirtmcmc_refuses_a_ranks_argument_it_would_not_read(bad):
    """Anything but None, False, True or a dict with known keys raises before a device is needed."""
    from gpirt_amd import gpirtMCMC
    y = np.where(np.random.default_rng(1).random((8, 4)) < 0.5, 1.0, -1.0)
    with pytest.raises(ValueError, match="ranks"):
        gpirtMCMC(y, 2, 1, vote_codes=dict(yea=[1], nay=[-1], missing=[None]), preset="fast", ranks=bad)


def test_pivot_arguments():
    from gpirt_amd import ranks
    assert ranks.close_pivots(100, ("median", 41, 60)) == ([50, 51, 41, 60], [41, 50, 51, 60])
    assert ranks.close_pivots(7, "median") == ([4], [4])
    assert ranks.close_pivots(8, 3) == ([3], [3, 6])
    with pytest.raises(ValueError):
        ranks.from_draws(np.zeros((1, 2, 40)), list(range(1, 18)))
    with pytest.raises(ValueError):
        ranks.from_draws(np.zeros((1, 2, 5)), [6])
    with pytest.raises(ValueError):
        ranks.close_pivots(5, "mean")


def test_abi_of_version_108():
    """The library exports the rank entry points, and gpirt_ranks has the header's size."""
    import ctypes as C

    from gpirt_amd import _lib
    lib = _lib.load()
    assert lib.gpirt_version() >= 108
    for name in ("gpirt_sampler_rank_enable", "gpirt_sampler_rank_accumulate", "gpirt_sampler_rank_get",
                 "gpirt_sampler_rank_state", "gpirt_rank_combine", "gpirt_mcmc_run"):
        assert hasattr(lib, name)
    # 8 + 4 + 4 + 32 * 8 + 4 + 4 + 10 pointers + 4 int64 + a double + 4 int64
    assert C.sizeof(_lib.Ranks) == 8 + 8 + 256 + 8 + 80 + 32 + 8 + 32
    # NULL arguments are refused with the library's error code and a message
    assert lib.gpirt_rank_combine(None, 1, None, None, None) == _lib.E_ARG
    assert _lib.last_error()
