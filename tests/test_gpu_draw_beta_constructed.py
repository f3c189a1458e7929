"""Handle.draw_beta and Sampler.draw_beta() on constructed items (tests/_stage_exact.py, draw_beta_cases) against beta_exact,
src/draw-beta.cpp:3-41 in long double, at n in {1, 100, 256, 257, 1000} rows (256 | 257: the edges of the kernel's 256-thread
strided loop), one launch per n and one column per case:

ordinary; step0_zero, step1_zero, both_zero (r = 0 exactly: accepted); no_observed_row; single_observed_row; tight_prior
(ps = 1e-3); tie_s<k>_<p|m><6|9> (pm solved so that r = log u +- 1e-6 | 1e-9 at step k); accept_then_decide and
reject_then_decide (the two branches that hand the first coefficient's kept log-likelihood to the second);
both_overflow (r = NaN: rejected), proposal_overflow and proposal_overflow_s1 (r = -inf: rejected), current_overflow
(r = +inf: accepted).

tests/test_stage_exact_cpu.py shows without a GPU that no decision of any column is undecided under the derived bound.
Asserted: both decisions are the reference's; on a reject beta keeps its bits, on an accept it is within an ulp of
cv + step z; beta agrees with the CPU oracle to 1e-12.  On the Sampler's path the same beta, and mu, mu_star equal to
b0 + x b1 to an ulp of the larger operand."""
import numpy as np
import pytest

import _stage_exact as X

pytestmark = pytest.mark.gpu


def _device_normals(handle, c):
    """z at index 0 and 2 of every item's sub-stream as the device draws them: the restated generator's to the last places"""
    from gpirt_amd.ops import to_host
    m = len(c["names"])
    Z = to_host(handle.item_normals(c["seed"], c["it"], X.ST_BETA, 0, m, 4))[0::2]
    zr, _ = X.beta_randoms(c["seed"], c["it"], m)
    assert np.abs(Z - zr).max() <= 8 * 2.0 ** -52 * np.abs(zr).max()
    return Z


def _check(c, ref, out, what):
    """decisions and values of a 2 x m result against the references; returns the worst |beta - proposal| in ulps"""
    worst = 0.0
    for j, (nm, r) in enumerate(zip(c["names"], ref)):
        cv = c["beta"][:, j].copy()
        for k in range(2):
            if r["accept"][k]:
                ulp = np.spacing(max(abs(cv[k]), abs(r["proposal"][k])))
                d = abs(out[k, j] - r["proposal"][k]) / ulp
                worst = max(worst, d)
                assert d <= 1.0, (what, nm, k, "accepted by the reference", out[k, j], r["proposal"][k], cv[k])
                cv[k] = r["proposal"][k]
            else:
                assert out[k, j] == c["beta"][k, j], (what, nm, k, "rejected by the reference", out[k, j], c["beta"][k, j])
    return worst


@pytest.mark.parametrize("n", X.BETA_ORDERS)
def test_draw_beta_constructed(handle, oracle, n):
    from gpirt_amd.ops import to_device, to_host
    c = X.draw_beta_cases(n)
    ref = X.draw_beta_reference(n, _device_normals(handle, c))
    undecided = sum(r["undecided"] for r in ref)
    bd = to_device(c["beta"])
    handle.draw_beta(bd, to_device(c["theta"]), to_device(c["y"]), to_device(c["f"]), to_device(c["pm"]), to_device(c["ps"]),
                     to_device(c["step"]), c["seed"], c["it"])
    out = to_host(bd)
    worst = _check(c, ref, out, n)
    fin = [b for r in ref for b, mg in zip(r["bound"], r["margin"]) if np.isfinite(mg) and b > 0]
    tight = max(b / mg for r in ref for b, mg in zip(r["bound"], r["margin"]) if np.isfinite(mg))
    print(f"MEASURED n={n}: undecided decisions {undecided}; worst bound / margin {tight:.3f} (largest bound {max(fin):.2e}); "
          f"worst |beta - (cv + step z)| {worst:.2f} ulp")
    assert undecided == 0 and tight <= 1.0
    o = oracle.draw_beta(oracle.ItemStream(c["seed"]), c["beta"], c["theta"], c["y"], c["f"], c["pm"], c["ps"], c["step"], it=c["it"])
    assert np.abs(out - o).max() <= 1e-12


def test_sampler_draw_beta_and_its_means(handle):
    from gpirt_amd.sampler import Sampler
    n = 257
    c = X.draw_beta_cases(n)
    ref = X.draw_beta_reference(n, _device_normals(handle, c))
    s = Sampler(handle, c["y"], c["theta"], c["pm"], c["ps"], c["step"], rng="item", seed=c["seed"])
    s.init()
    s.set("theta", c["theta"]); s.set("f", c["f"]); s.set("beta", c["beta"])
    s.set_iteration(c["it"] - 1)
    s.draw_beta()
    out, mu, mu_star = s.get("beta"), s.get("mu"), s.get("mu_star")
    s.close()
    worst = _check(c, ref, out, "sampler")
    err = 0.0
    for x, got in ((c["theta"], mu), (X.grid(), mu_star)):
        a, b = out[0][None, :], x[:, None] * out[1][None, :]
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
        err = max(err, float((np.abs(got - (a + b)) / ulp).max()))
    print(f"MEASURED sampler path n={n}: undecided decisions {sum(r['undecided'] for r in ref)}; "
          f"worst |beta - (cv + step z)| {worst:.2f} ulp; worst |mu - (b0 + x b1)| {err:.2f} ulp of the larger operand")
    assert sum(r["undecided"] for r in ref) == 0 and err <= 1.0
