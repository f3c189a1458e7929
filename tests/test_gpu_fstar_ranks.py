"""draw_fstar's rank-r form at every rank the public option allows (gpirt_options.kstar_rank = 16..128 in steps of 16)
against the rank-r operator itself in long double (tests/_stage_exact.py, fstar_rank_exact), given the device's own theta,
L, f and mu* -- not against the full solve, which only agrees where the interpolation error is below rounding (r >= 48).

Layouts: n = 320 and 576 (n % 64 == 0: the r border rows are carried through the factorisation; 576 crosses one 512
block of the solve), n = 300 (explicit solves), n = 320 under GPIRT_BORDERED=2.  Sampler stage API, rng="item",
theta_stabilise, fstar_fused; m = 7."""
import numpy as np
import pytest

import _stage_exact as X

pytestmark = pytest.mark.gpu

RANKS = (16, 32, 48, 64, 80, 96, 112, 128)
LAYOUTS = {"bordered_320": (320, 1), "bordered_576": (576, 1), "explicit_300": (300, 1), "explicit_320": (320, 2)}
M, SEED = 7, 5
U = 2.0 ** -53


def _sampler(handle, n, r, bordered, **kw):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, M, seed=3)
    opts = dict(rng="item", seed=SEED, theta_stabilise=True, fstar_fused=True, kstar_rank=r)
    opts.update(kw)
    with handle.config("GPIRT_BORDERED", bordered):          # (the layout is chosen when the sampler is created)
        return Sampler(handle, y, th0, **opts)


def _draw(s):
    """(state, outputs, z) of one draw_fstar on the sampler's current state"""
    st = {k: np.array(s.get(k)) for k in ("theta", "L", "f", "mu_star")}
    it = s.iteration + 1
    s.draw_fstar()
    s.check()
    out = {k: np.array(s.get(k)) for k in ("s", "mean", "fstar")}
    z = np.asarray(s.handle.item_normals(SEED, it, X.ST_FSTAR, 0, M, X.NGRID).T.contiguous().cpu().numpy().T)
    return st, out, z


def _full_solve(handle, n, bordered, st):
    """the r = 0 sampler on the same state"""
    s0 = _sampler(handle, n, 0, bordered)
    s0.init()
    s0.draw_f()
    for name in ("theta", "f", "mu_star", "L"):
        s0.set(name, st[name])
    s0.draw_fstar()
    s0.check()
    out = {k: np.array(s0.get(k)) for k in ("s", "mean", "fstar")}
    s0.close()
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("r", RANKS)
def test_every_rank_against_the_rank_r_operator(handle, r, layout):
    n, bordered = LAYOUTS[layout]
    s = _sampler(handle, n, r, bordered)
    s.init()
    s.draw_f()
    st, out, z = _draw(s)
    s.close()
    ref = X.fstar_rank_exact(st["theta"], st["L"], st["f"], st["mu_star"], r, z)
    # R::rnorm(mean, s) is NaN for s < 0 (src/draw-fstar.cpp:27).  The exact operator has q <= 1, s >= 0; the r = 16
    # approximation (4.6e-3) can push q above 1 at some grid points, and the rank-r operator's f* is then NaN there, on the
    # device as in the reference: the NaN cells must coincide (wherever s is not within the tolerance of 0)
    s_ref = ref["s"].astype(np.float64)
    clear = np.abs(s_ref) > 1e-9
    nan_dev, nan_ref = np.isnan(out["fstar"]), np.isnan(ref["fstar"].astype(np.float64))
    assert np.array_equal(nan_dev[clear], nan_ref[clear])
    assert np.isfinite(out["s"]).all() and np.isfinite(out["mean"]).all()
    if r >= 32:
        assert not nan_dev.any() and (s_ref > 0).all()
    else:
        print(f"MEASURED r={r} {layout}: {int((s_ref < 0).sum())} of 1001 grid points have s < 0 (min {s_ref.min():.2e}): f* is NaN there")
    worst = {}
    for k in ("s", "mean", "fstar"):
        rk = ref[k].astype(np.float64)
        ok = ~(np.isnan(rk) | np.isnan(out[k]))
        worst[k] = float(np.abs(out[k].astype(X.LD) - ref[k])[ok].max()) / max(1.0, float(np.abs(rk[ok]).max()))
    print(f"MEASURED r={r} {layout}: |s - ref| {worst['s']:.2e}  |mean - ref| {worst['mean']:.2e}  |f* - ref| {worst['fstar']:.2e}"
          f"  (relative to max(1, max|ref|); cond(S) {ref['cond']:.2e})")
    for k in ("s", "mean", "fstar"):
        assert worst[k] <= 1e-9, (k, worst[k])
    # ... and the full solve on the same state
    full = _full_solve(handle, n, bordered, st)
    dist = {k: float(np.nanmax(np.abs(out[k] - full[k]))) for k in ("s", "mean", "fstar")}
    if r >= 48:
        print(f"MEASURED r={r} {layout}: distance to the full solve  s {dist['s']:.2e}  mean {dist['mean']:.2e}  f* {dist['fstar']:.2e}")
        for k in ("s", "mean", "fstar"):
            assert dist[k] <= 1e-9 * max(1.0, np.abs(full[k]).max()), (k, dist[k])
    else:
        # r = 16, 32 approximate K*: mean_r - mean_0 = (V U^T - K*^T) S^-1 f, so per grid point and item
        # |mean_r - mean_0| <= E ||S^-1 f_j||_1 with E the largest interpolation error over (theta_i, grid point), measured in
        # long double at this theta; 1e-9 max(1, max|mean|) on top for the two devices' rounding (the project's tolerance)
        E = X.interpolation_error(r, st["theta"])
        bound = E * float(ref["alpha1"].max()) + 1e-9 * max(1.0, float(np.abs(full["mean"]).max()))
        print(f"MEASURED r={r} {layout}: distance to the full solve  mean {dist['mean']:.2e} (bound {bound:.2e}, E {E:.2e}, "
              f"max ||S^-1 f||_1 {ref['alpha1'].max():.2e})  s {dist['s']:.2e}  f* {dist['fstar']:.2e}")
        assert dist["mean"] > 1e-9 and dist["fstar"] > 1e-9
        assert dist["mean"] <= bound


def _patterns(n):
    g = X.grid()
    one = np.full(n, g[617])
    two = np.where(np.arange(n) % 2 == 0, g[400], g[401])
    ends = np.where(np.arange(n) < n // 2, -5.0, 5.0)
    return {"one_point": one, "two_points_0.01_apart": two, "plus_minus_5": ends}


@pytest.mark.parametrize("pattern", ["one_point", "two_points_0.01_apart", "plus_minus_5"])
@pytest.mark.parametrize("r", [64, 128])
def test_constructed_theta(handle, r, pattern):
    """theta on one grid point, on two grid points 0.01 apart, at +-5: S = K + 0.001 I is as ill-conditioned as the jitter
    allows, v^T G v -> 1 at the occupied grid points (s ~ 1.5e-6 for n = 320 on one point) and -> 0 far from them, where
    the quadratic form cancels and the reference's sum of squares cannot.

    Tolerance on s, derived.  q_j = v_j^T G v_j, G = B^T B, B = L^-1 U.  (i) The computed solve satisfies
    (L + dL) B^ = U with |dL| <= n u |L| (u = 2^-53), so ||dB|| <= n u cond_2(L) ||B||, and the same again for the products of
    G: |dq| <= 4 n u sqrt(cond(S)) q, q <= 1.  (ii) The quadratic form is a sum of r^2 products of magnitudes
    |v_k| |G_kl| |v_l| with |G_kl| <= 1 (G_kk = k(c_k)^T S^-1 k(c_k) <= K(c_k, c_k) = 1, S >= K): at most (n + 2 r) u Lam^2, Lam =
    sum_k |v_jk| (the split-K sum over n, then two sums over r).  dq = (i) + (ii), and
    |d sqrt(q)| <= min(sqrt(dq), dq / sqrt(q)); one ulp of 1 for the final subtraction.
    mean and f*: the forward error of S x = f, 8 n u cond(S) relative to max(1, max|ref|)."""
    n = 320
    s = _sampler(handle, n, r, 1)
    s.init()
    s.draw_f()
    s.set("theta", _patterns(n)[pattern])
    s.factor()
    st, out, z = _draw(s)
    s.close()
    assert np.array_equal(st["theta"], _patterns(n)[pattern])
    ref = X.fstar_rank_exact(st["theta"], st["L"], st["f"], st["mu_star"], r, z)
    cond = ref["cond"]
    lam = float(np.abs(X.cheb_basis(r)[1]).sum(axis=1).max())
    q = np.maximum(ref["q"].astype(np.float64), 0.0)
    dq = 4 * n * U * np.sqrt(cond) * q + (n + 2 * r) * U * lam ** 2
    tol_s = np.minimum(np.sqrt(dq), dq / np.maximum(np.sqrt(q), 1e-300)) + 2 * U
    s_ref = ref["s"].astype(np.float64)
    err_s = np.abs(out["s"].astype(X.LD) - ref["s"]).astype(np.float64)
    print(f"MEASURED r={r} {pattern}: cond(S) {cond:.2e}  min s {s_ref.min():.3e}  max |s - ref| / tol {(err_s / tol_s).max():.3f}"
          f"  max |s - ref| {err_s.max():.2e}")
    assert (s_ref < 1.0).all() and (s_ref > 0).all()
    assert (out["s"] < 1.0).all(), "the clamp of the quadratic form produced s = 1 where the reference has s < 1"
    assert (err_s <= tol_s).all(), (float(err_s.max()), int(np.argmax(err_s / tol_s)))
    if pattern == "one_point":
        assert 1.0e-6 < s_ref.min() < 2.0e-6
    tol = 8 * n * U * cond
    for k in ("mean", "fstar"):
        rk = ref[k].astype(np.float64)
        e = float(np.abs(out[k].astype(X.LD) - ref[k]).max()) / max(1.0, float(np.abs(rk).max()))
        print(f"MEASURED r={r} {pattern}: |{k} - ref| {e:.2e} (tolerance {tol:.2e})")
        assert np.isfinite(out[k]).all() and e <= tol


def test_refused_ranks_leave_the_handle_usable(handle):
    from gpirt_amd import _lib
    for kw in (dict(r=8), dict(r=24), dict(r=144), dict(r=64, fstar_fused=False)):
        r = kw.pop("r")
        with pytest.raises(_lib.GpirtError) as ei:
            _sampler(handle, 320, r, 1, **kw)
        assert ei.value.code == _lib.E_ARG
        s = _sampler(handle, 64, 64, 1)                       # the handle is still usable
        s.init()
        s.draw_f()
        s.draw_fstar()
        s.check()
        assert np.isfinite(s.get("fstar")).all()
        s.close()
