"""Handle.draw_theta, Handle.theta_logpost and the Sampler's theta stages on constructed states (tests/_stage_exact.py,
draw_theta_cases) against theta_exact, src/draw-theta.cpp:3-37 in long double, under GPIRT_THETA_FIXED in {1, 2} and
stabilise in {False, True}.

one_item_finite / one_item_fallback (n = m = 130, respondent i answers item i alone; f* = -600 | -800 off the designed rows,
the second hands the launch to the fp64 product): per respondent a "point" mass at an interior row, at the "last_row"
(theta = +5.0), at "row_0" (0/0: degenerate, stabilised or not), a two-point "tie" at rows 300 and 700 with
w1 / (w1 + w2) = u_i +- {1e-6, 1e-9, 1e-11}, "flat" (the prior alone), "peaked" (below exp's range: degenerate only without
stabilisation) and "overflow" (f* = -800 on the whole grid under the answer: every row -inf, degenerate -- the device's
-1e300 stand-in must not turn it into a flat posterior).  dense_smooth, dense_nan_cell (one NaN f* that respondents with the
item missing must not see), dense_nan_row (what kstar_rank = 16 produces), dense_pm800, dense_overflow_item: n = 257, m = 48.

tests/test_stage_exact_cpu.py shows without a GPU that no respondent of any case is undecided under the derived bound of
the device's rounding.  Asserted: the grid row drawn and the degenerate count equal theta_exact's; the log-posterior is
within the product's bound where the reference is finite, NaN where it is NaN, and at or below -1e300 -- the product's
stand-in for -inf, INTEGRATION.md section 2 -- exactly where it is -inf; both products draw the same theta; the CPU oracle
agrees with the reference too.  On the Sampler's path a degenerate draw is the named error of check()."""
import numpy as np
import pytest

import _stage_exact as X

pytestmark = pytest.mark.gpu
CASES = ("one_item_finite", "one_item_fallback", "dense_smooth", "dense_nan_cell", "dense_nan_row", "dense_pm800",
         "dense_overflow_item")


def _rows(theta):
    return np.where(np.isnan(theta), -1, np.rint((theta + 5.0) / 0.01)).astype(np.int64)


def _logpost_ratio(lp, ref, what):
    """worst |device - reference| / bound over the finite entries; the non-finite ones must sit where the reference's do"""
    rl = ref["logpost"]
    nan, ninf = np.isnan(rl), np.isneginf(rl)
    assert np.array_equal(np.isnan(lp), nan), (what, "NaN elsewhere than the reference", int(np.isnan(lp).sum()), int(nan.sum()))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(lp <= X.SENTINEL, ninf), (what, "-inf elsewhere than the reference")
    fin = ~(nan | ninf)
    err = np.abs((lp[fin].astype(X.LD) - rl[fin]).astype(np.float64))
    return float((err / np.maximum(ref["lp_bound"][fin], 1e-300)).max()) if fin.any() else 0.0


@pytest.mark.parametrize("stabilise", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_draw_theta_constructed(handle, oracle, name, stabilise):
    from gpirt_amd.ops import to_device
    c = X.draw_theta_cases()[name]
    yd, fd = to_device(c["y"]), to_device(c["fstar"])
    rows, worst, undecided = {}, 0.0, 0
    for mode in (1, 2):
        ref = X.draw_theta_reference(name, stabilise, "fixed" if mode == 1 else "gemm")
        with handle.config("GPIRT_THETA_FIXED", mode):
            th, deg = handle.draw_theta(yd, fd, X.THETA_SEED, X.THETA_IT, stabilise=stabilise)
            lp, fb = handle.theta_logpost(yd, fd)
        assert fb == int(mode == 1 and X.theta_hands_over(c["fstar"]))
        rows[mode] = _rows(th.cpu().numpy())
        ratio = _logpost_ratio(lp.cpu().numpy(), ref, (name, mode))
        worst = max(worst, ratio)
        undecided += int(ref["undecided"].sum())
        ok = ~ref["undecided"]
        bad = np.flatnonzero((rows[mode] != ref["index"]) & ok)
        print(f"MEASURED {name} stabilise={stabilise} GPIRT_THETA_FIXED={mode}: worst |logpost - ref| / bound {ratio:.3f}; "
              f"undecided {int(ref['undecided'].sum())}; degenerate {deg} (reference {ref['degenerate']}); rows off {bad.size}")
        assert bad.size == 0, (name, mode, [(int(i), c["kinds"][i], int(rows[mode][i]), int(ref["index"][i])) for i in bad[:8]])
        assert deg == ref["degenerate"] and deg == int((rows[mode] < 0).sum())
        assert ratio <= 1.0
    assert np.array_equal(rows[1], rows[2])
    assert undecided == 0
    refo = X.draw_theta_reference(name, stabilise, "oracle")
    th_o, deg_o = oracle.draw_theta(oracle.ItemStream(X.THETA_SEED), c["y"], c["fstar"], it=X.THETA_IT, stabilise=stabilise)
    ok = ~refo["undecided"]
    assert np.array_equal(_rows(th_o)[ok], refo["index"][ok]) and deg_o == refo["degenerate"]
    assert np.array_equal(_rows(th_o)[ok], rows[1][ok])


def test_sampler_theta_stages_on_the_dense_layout(handle):
    """set("fstar") -> theta_partial -> theta_finish -> get("theta"), get("logpost"): the same rows, the same bound; whoever
    answered -1 to the item that overflows on the whole grid is the sampler's named error, with the reference's count"""
    from gpirt_amd.sampler import Sampler
    cases = X.draw_theta_cases()
    y = cases["dense_smooth"]["y"]
    n = y.shape[0]
    s = Sampler(handle, y, np.linspace(-2.0, 2.0, n), rng="item", seed=X.THETA_SEED, theta_stabilise=True)
    s.init()
    worst = 0.0
    for name in CASES[2:]:
        ref = X.draw_theta_reference(name, True, "fixed")
        s.set_iteration(X.THETA_IT - 1)
        s.set("fstar", cases[name]["fstar"])
        s.theta_partial(); s.theta_finish()
        rows = _rows(s.get("theta"))
        worst = max(worst, _logpost_ratio(s.get("logpost"), ref, name))
        assert ref["undecided"].sum() == 0 and np.array_equal(rows, ref["index"]), name
        if ref["degenerate"]:
            with pytest.raises(Exception, match=r"underflowed for %d respondent" % ref["degenerate"]):
                s.check()
        else:
            s.check()
    print(f"MEASURED sampler path, dense layout: worst |logpost - ref| / bound {worst:.3f}; undecided 0")
    assert worst <= 1.0
    assert X.draw_theta_reference("dense_overflow_item", True, "fixed")["degenerate"] > 0
    s.close()
