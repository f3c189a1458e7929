"""The NumPy statement of the item-pair order posteriors (gpirt_amd.shape.order_from_draws) against a plain double loop over
pairs and grid points on small constructed curves, the parser's refusals, the library version and the state block's size."""
import ctypes as C

import numpy as np
import pytest

from gpirt_amd import shape as SH

NG = 1001
K = np.arange(NG)
BASE = (K - 500) / 64.0                     # exact in fp64, and so is BASE + c for the small dyadic c below
TOLS = (0.0, 0.25, 1.0)


def curves(k_half):
    """two draws of nine columns: every class at every tolerance, and gaps exactly equal to 0.25 and 1.0"""
    klo, khi = 500 - k_half, 500 + k_half
    zig = np.where(K % 2 == 0, 0.25, -0.25)
    spike = np.zeros(NG); spike[klo] = 2.0
    out_lo = np.zeros(NG)
    if klo > 0:
        out_lo[klo - 1] = 5.0               # outside W: not counted
    g0 = np.stack([BASE, BASE + 0.25, BASE + 1.0, BASE + zig, BASE - 1.0 + spike, BASE + 2.0 * zig, BASE.copy(),
                   BASE + out_lo, BASE + 8.0 * zig], axis=1)
    g1 = g0[:, ::-1].copy()
    return np.stack([g0, g1])


def loops(draws, k_half, tols):
    """the header, one scalar statement at a time"""
    S, _, m = draws.shape
    klo, khi = 500 - k_half, 500 + k_half
    nt = len(tols)
    above = np.zeros((nt, m, m), dtype=np.uint32)
    cross = np.zeros((nt, m, m), dtype=np.uint32)
    depth = np.zeros((m, m))
    setc = np.zeros((3, nt), dtype=np.uint64)
    for g in draws:
        nc = [0] * nt
        for a in range(m):
            for b in range(m):
                if a == b:
                    continue
                U, L = -np.inf, np.inf
                for k in range(klo, khi + 1):
                    d = g[k, a] - g[k, b]
                    U, L = max(U, d), min(L, d)
                for q, t in enumerate(tols):
                    if U > t and L < -t:
                        cross[q, a, b] += 1
                        nc[q] += a < b
                    elif U > t and L >= -t:
                        above[q, a, b] += 1
                    elif U <= t and L < -t:
                        above[q, b, a] += 1
                depth[a, b] += min(max(U, 0.0), max(-L, 0.0))
        for q in range(nt):
            setc[:, q] += np.array([nc[q] == 0, nc[q], nc[q] * nc[q]], dtype=np.uint64)
    # (a above b) was bumped from both orders of the pair
    return above // 2, cross, depth, setc


@pytest.mark.parametrize("k_half", [1, 20])
def test_order_from_draws_against_loops(k_half):
    g = curves(k_half)
    got = SH.order_from_draws(g, k_half / 100.0, TOLS, top=5)
    above, cross, depth, setc = loops(g, k_half, TOLS)
    assert np.array_equal(got["above"], above) and np.array_equal(got["cross"], cross)
    assert np.array_equal(got["depth_sum"], depth) and np.array_equal(got["set_counts"], setc)
    assert (got["draws"], got["skipped"]) == (2, 0)
    # every class at every tolerance
    tied = 2 - got["above"].astype(int) - got["above"].astype(int).transpose(0, 2, 1) - got["cross"]
    off = ~np.eye(g.shape[2], dtype=bool)
    for q in range(3):
        assert got["above"][q].any() and got["cross"][q].any() and tied[q][off].any(), q
        assert (tied[q][off] >= 0).all() and np.array_equal(got["cross"][q], got["cross"][q].T)
    # equality exactly at t: a gap of 0.25 is "above" at t = 0 and tied at t = 0.25; of 1.0 tied at t = 1.0; the zigzag of
    # +-0.25 crosses at t = 0 and is tied at t = 0.25
    dr = SH.order_from_draws(g[:1], k_half / 100.0, TOLS)
    assert dr["u"][1, 0] == 0.25 and dr["above"][:, 1, 0].tolist() == [1, 0, 0] and dr["cross"][:, 1, 0].tolist() == [0, 0, 0]
    assert dr["u"][2, 0] == 1.0 and dr["above"][:, 2, 0].tolist() == [1, 1, 0]
    assert dr["cross"][:, 3, 0].tolist() == [1, 0, 0] and dr["above"][:, 3, 0].tolist() == [0, 0, 0] and dr["above"][:, 0, 3].tolist() == [0, 0, 0]
    assert dr["cross"][:, 4, 0].tolist() == [1, 1, 0]                  # +1 at k_lo only, -1 elsewhere
    assert not dr["above"][:, 6, 0].any() and not dr["cross"][:, 6, 0].any() and dr["easier"][6, 0] == dr["easier"][0, 6] == 0
    if k_half == 20:
        assert not dr["cross"][:, 7, 0].any() and dr["u"][7, 0] == 0.0  # the spike outside W is not counted
    assert np.array_equal(dr["depth_sum"], dr["depth_sum"].T) and dr["depth_sum"][4, 0] == 1.0
    # finishing: probabilities sum to one off the diagonal, NaN on it; the mean rank is linear in p_easier
    p = got["p_above"] + got["p_above"].transpose(0, 2, 1) + got["p_cross"] + got["p_tied"]
    assert np.allclose(p[:, off], 1.0) and np.isnan(np.diagonal(got["p_cross"], axis1=1, axis2=2)).all()
    assert np.array_equal(got["rank_mean"], 1.0 + got["easier"].sum(axis=0) / 2.0)
    assert np.array_equal(got["easier"], SH.order_ranks_from_easiness(got["e_draws"]))
    assert np.array_equal(got["cross_items_mean"], got["cross"].sum(axis=2) / 2.0)
    w = got["worst"]
    assert w["pairs"].shape == (5, 2) and (w["pairs"][:, 0] < w["pairs"][:, 1]).all()
    assert (np.diff(w["p_cross"]) <= 0).all() and w["p_cross"][0] == got["p_cross"][2][off].max()
    same = w["p_cross"][:-1] == w["p_cross"][1:]
    flat = w["pairs"][:, 0] * 100 + w["pairs"][:, 1]
    assert (np.diff(flat)[same] > 0).all()                              # ties to the lowest (a, b)


def test_skipped_draws_and_pooling():
    g = curves(20)
    bad = g[0].copy(); bad[0, 2] = np.nan                               # outside W: the draw is skipped whole all the same
    inf = g[0].copy(); inf[500, 1] = -np.inf
    a = SH.order_from_draws(np.stack([g[0], bad, inf, g[1]]), 0.2, TOLS)
    b = SH.order_from_draws(g, 0.2, TOLS)
    assert (a["draws"], a["skipped"]) == (2, 2)
    for k in ("above", "cross", "depth_sum", "set_counts", "easier", "easiness", "u"):
        assert np.array_equal(a[k], b[k]), k
    two = SH.order_from_draws([g[:1], g[1:]], 0.2, TOLS)
    for k in ("above", "cross", "depth_sum", "set_counts", "easier"):
        assert np.array_equal(two[k], b[k]), k


def test_parser_refusals():
    assert SH.parse(True)["order"] is False and SH.parse(dict(order=True))["order_top"] == 20
    assert SH.parse(dict(order=True, order_top=64))["order_top"] == 64
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="order_top"):
            SH.parse(dict(order=True, order_top=bad))
    with pytest.raises(ValueError, match="unknown keys"):
        SH.parse(dict(order=True, orders=3))
    with pytest.raises(ValueError, match="order"):
        SH.parse(dict(order="yes"))
    with pytest.raises(ValueError, match="order_top"):
        SH.order_from_draws(curves(1), 0.01, TOLS, top=0)
    with pytest.raises(ValueError, match="2..4096"):
        SH.order_from_draws(curves(1)[:, :, :1], 0.01, TOLS)


def test_version_and_state_bytes():
    from gpirt_amd import _lib
    lib = _lib.load()
    assert lib.gpirt_version() >= 118
    for m, nt in ((2, 1), (3, 3), (33, 4), (1024, 3), (4096, 3)):
        b = C.c_int64()
        assert lib.gpirt_shape_order_state_bytes(m, nt, C.byref(b)) == 0
        want = 128
        for cells, width in ((nt * m * m, 4), (nt * m * m, 4), (m * m, 4), (m * m, 8), (2 * m, 8), (3 * 4, 8)):
            want += (cells * width + 15) // 16 * 16
        assert b.value == want == SH.order_state_bytes(m, nt), (m, nt)
    b = C.c_int64()
    for m, nt in ((1, 3), (4097, 3), (5, 0), (5, 5)):
        assert lib.gpirt_shape_order_state_bytes(m, nt, C.byref(b)) == _lib.E_ARG
    # the figures the README states: accumulators plus u
    assert abs((SH.order_state_bytes(1024, 3) + 8 * 1024 ** 2) / 1e6 - 46.1) < 0.1
    assert abs((SH.order_state_bytes(4096, 3) + 8 * 4096 ** 2) / 1e9 - 0.738) < 0.001
