"""Bounds for comparing the device's autocorrelation finish (csrc/acf.hip, acf_finish_kernel: fp64) and its log-likelihood pass
with the long-double statement gpirt_amd.acf.from_draws, derived from each case's raw sums and inputs; and the constructed draws
the CPU and the GPU tests share.  Nothing here is fitted to a device's output.

u = 2^-52 (twice fp64's unit roundoff) bounds every rounding below.  The raw sums are the same numbers on both sides (the tests
compare them bit for bit first), theta's integers convert to fp64 exactly and a sign is an exact product, so only the finish
rounds.  Per half-chain c and lag k, with dbar = sum / H:
  cross = dbar ((sum - tail_k) + (sum - head_k)): the quotient, two differences, a sum and a product        <= 5 u |cross|*
  sq    = ((H - k) dbar) dbar: dbar's own error twice and two products                                      <= 4 u |sq|
  gamma = ((s_k - cross) + sq) / H: three more roundings, each of at most the sum of the magnitudes         <= 3 u T / H
  with |cross|* = |dbar| (|sum - tail_k| + |sum - head_k|) and T = |s_k| + |cross|* + |sq|: |gamma error| <= 8 u T / H.
The mean over the M = 2C half-chains adds M roundings of partial sums and one quotient: (M + 1) u mean_c T / H.
  Eg_k = (9 + M) u mean_c T_c / H,   EW = Eg_0 H / (H - 1) + 2 u |W|.
Half means hm = centre + dbar: u |dbar| + u |hm|; their mean (M + 1) u hmax; a deviation e: Ee = (M + 4) u hmax with hmax the
largest of |centre|, |dbar|, |hm| over c; B = sum e^2 / (M - 1):
  EB = [sum_c 2 |e| Ee + M Ee^2 + (M + 2) u sum e^2] / (M - 1),   Ev = EW + EB + 3 u (|W| + B)   (var+'s bound).
rho_k = 1 - q, q = (W - gbar_k) / var+: EN = EW + Eg_k + u |W - gbar_k|; Eq = (EN + |q| Ev) / (var+ - Ev) + u |q|;
  Erho_k = Eq + u (1 + |q|)   (infinite unless Ev < var+ / 2).
A pair P_j = rho_2j + rho_2j+1: Ep_j = Erho_2j + Erho_2j+1 + u |P_j| (rho_0 = 1 is exact).
tau = -1 + 2 sum_j max(min_{i <= j} P_i, 0) -- Geyer's rule written without its stop: after the first P_j <= 0 the running minimum
is <= 0 and adds nothing --, and each term is 1-Lipschitz in the largest pair error, so with J pairs
  Etau = 2 J max_j Ep_j + 4 u J |tau| + 4 u / log10 N   (the sum's roundings; the floor 1 / log10 N, itself 1-Lipschitz).
This holds whether or not both sides stop at the same pair; lag_used and truncated, which do jump there, are compared only where
every pair that was looked at keeps more than 2 max_j Ep_j from 0 and from the running minimum before it (`decided`).
  ess = N / tau:  Eess = N Etau / (tau (tau - Etau)) + u ess   (infinite unless Etau < tau / 2);
  with rv = Ev / (var+ - Ev), re = Eess / (ess - Eess), rw = EW / (W - EW) (infinite unless EW < W / 2):
  mcse = sqrt(var+ / ess): mcse (rv + re + 2 u);  rhat = sqrt(var+ / W): rhat (rv + rw + 2 u);  sd: sd (rv + u)
  (sqrt halves a relative error; the bounds keep it whole);  mean: (M + 3) u hmax;  rho1: Erho_1;  acf: Erho_k.

The log-likelihood pass.  exp and log1p on the device are within 2 ulp, the cell -(log1p(e) + max(-a, 0)) rounds twice more:
4 u |cell|.  A series' value is a sum of its cells through at most A additions (the lane's, the tree's, the folds'), each
rounding at most u / 2 of a partial sum of magnitude <= sum |cell|: bound = (4 + A / 2) u sum |cell| with A = the number of
cells of the series' sum plus the partials it is folded from (cells + 8 + ceil(n / 256) + ceil(m / 32) + m is never less)."""
import numpy as np

from gpirt_amd import acf as AC

U = float(np.finfo(np.float64).eps)
ld = np.longdouble


def finish_bounds(out):
    """dict(ess, tau, mcse, rhat, rho1, mean, sd: P; acf: (L + 1) x P; pair: P, the largest Ep_j; decided: P bool) from
    from_draws's / finish's dict"""
    raws, H, L = out["raw"], out["H"], out["L"]
    M = 2 * len(raws)
    a = lambda k: np.concatenate([np.asarray(r[k], dtype=ld) for r in raws])     # noqa: E731
    sm, s, hd, tl = a("sum"), a("s"), a("head"), a("tail")
    cen = np.repeat(np.stack([np.asarray(r["centre"], dtype=ld) for r in raws]), 2, axis=0)
    Hd = ld(H)
    kk = np.arange(L + 1, dtype=ld)[None, :, None]
    dbar = sm / Hd
    with np.errstate(all="ignore"):
        cross_abs = np.abs(dbar)[:, None] * (np.abs(sm[:, None] - tl) + np.abs(sm[:, None] - hd))
        T = np.abs(s) + cross_abs + (Hd - kk) * (dbar ** 2)[:, None]
        Eg = (9 + M) * U * T.mean(axis=0) / Hd
        gamma = (s - dbar[:, None] * ((sm[:, None] - tl) + (sm[:, None] - hd)) + (Hd - kk) * dbar[:, None] ** 2) / Hd
        gm = gamma.mean(axis=0)
        W = gm[0] * Hd / (Hd - 1)
        EW = Eg[0] * Hd / (Hd - 1) + 2 * U * np.abs(W)
        hm = cen + dbar
        hmax = np.maximum(np.maximum(np.abs(cen), np.abs(dbar)), np.abs(hm)).max(axis=0)
        e = hm - hm.mean(axis=0)
        Ee = (M + 4) * U * hmax
        dev = (e ** 2).sum(axis=0)
        B = dev / (M - 1)
        EB = ((2 * np.abs(e) * Ee).sum(axis=0) + M * Ee ** 2 + (M + 2) * U * dev) / (M - 1)
        varp = W * (Hd - 1) / Hd + B
        Ev = EW + EB + 3 * U * (np.abs(W) + B)
        okv = Ev < varp / 2
        num = W - gm
        q = num / varp
        EN = EW + Eg + U * np.abs(num)
        Eq = (EN + np.abs(q) * Ev) / (varp - Ev) + U * np.abs(q)
        Erho = np.where(okv, Eq + U * (1 + np.abs(q)), np.inf)
        Erho[0] = 0
        rho = 1 - q
        rho[0] = 1
        J = (L + 1) // 2
        P_ = rho[0:2 * J:2] + rho[1:2 * J:2]
        Ep = (Erho[0:2 * J:2] + Erho[1:2 * J:2] + U * np.abs(P_)).max(axis=0)
        tau, ess = np.asarray(out["tau"], dtype=ld), np.asarray(out["ess"], dtype=ld)
        N = ld(M * H)
        Etau = 2 * J * Ep + 4 * U * J * np.abs(tau) + 4 * U / np.log10(N)
        Eess = np.where(Etau < tau / 2, N * Etau / (tau * (tau - Etau)) + U * ess, np.inf)
        rv = Ev / (varp - Ev)
        re = Eess / (ess - Eess)
        rw = np.where(EW < W / 2, EW / (W - EW), np.inf)
        f64 = lambda v: np.asarray(v, dtype=np.float64)                          # noqa: E731
        res = dict(tau=f64(Etau), ess=f64(Eess), mcse=f64(out["mcse"] * (rv + re + 2 * U)),
                   rhat=f64(out["rhat"] * (rv + rw + 2 * U)), sd=f64(np.where(okv, out["sd"] * (rv + U), np.inf)),
                   mean=f64((M + 3) * U * hmax), rho1=f64(Erho[min(1, L)]), acf=f64(Erho), pair=f64(Ep))
        res["decided"] = np.asarray(out["margin"] > 2 * Ep)
    return res


def ll_bounds(g, y):
    """(m + n + 1,) float64: the bound of |device - long double| for item_ll, resp_ll, total_ll of one draw, and the long-double
    values themselves"""
    g, y = np.asarray(g, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, m = y.shape
    obs = ~np.isnan(y)
    gl = np.where(obs, g, 0.0).astype(ld)
    cell = np.where(obs, -(np.log1p(np.exp(-np.abs(gl))) + np.maximum(-(np.where(obs, y, 0.0) * gl), 0)), ld(0))
    mag = np.abs(cell)
    extra = 8 + -(-n // 256) + -(-m // 32) + m
    item = (4 + (n + extra) / 2) * U * mag.sum(axis=0)
    resp = (4 + (m + extra) / 2) * U * mag.sum(axis=1)
    total = (4 + (n * m + extra) / 2) * U * mag.sum()
    want = np.concatenate([cell.sum(axis=0), cell.sum(axis=1), [cell.sum()]])
    return np.concatenate([item, resp, [total]]).astype(np.float64), want


# ---------------------------------------------------------------------------------------------------- constructed draws ---
SHAPES = ((33, 2), (65, 31), (257, 33), (1000, 17))
RUNS = ((40, 1), (40, 3), (40, 19), (41, 7))                          # (S, L): L = H - 1 at (40, 19); a middle draw at S = 41


def _ar1(rng, S, P, lo=0.0, hi=0.95):
    """S x P series x_t = phi_p x_{t-1} + sqrt(1 - phi_p^2) e_t with phi spread over lo .. hi across the values"""
    phi = np.linspace(lo, hi, P)
    e = rng.normal(size=(S, P))
    x = np.empty((S, P))
    x[0] = e[0]
    for t in range(1, S):
        x[t] = phi * x[t - 1] + np.sqrt(1 - phi ** 2) * e[t]
    return x


def make_y(n, m, seed):
    rng = np.random.default_rng(seed)
    y = np.where(rng.uniform(size=(n, m)) < 0.6, 1.0, -1.0)
    y[rng.uniform(size=(n, m)) < 0.08] = np.nan
    y[n - 1, m - 1] = 1.0
    y[0, 0] = -1.0
    return y


def constructed(n, m, S, seed, saturated=False):
    """dict(y, theta (S x n, grid points), beta (S x 2 x m), f, mu (S x n x m)) of AR(1)-like series with phi over 0 .. 0.95.
    Special values: theta 0 is constant, theta 1 is off the grid in draw 3; beta value 0 (item 0's intercept) is constant and
    beta value 3 holds one NaN (draw 5).  saturated: |f + mu| >= 800, where exp(-|g|) is exactly 0 and the cell's ll is exactly 0
    or -|g| on any correct libm."""
    rng = np.random.default_rng(seed)
    y = make_y(n, m, seed + 1)
    k = np.clip(np.rint(500 + 120 * _ar1(rng, S, n)), 0, 1000)
    theta = -5.0 + k * 0.01
    theta[:, 0] = theta[0, 0]
    if S > 5:
        theta[3, 1] = 0.123456
    beta = (0.5 + 1.5 * _ar1(rng, S, 2 * m)).reshape(S, m, 2).transpose(0, 2, 1).copy()     # value 2j + r at [r, j]
    beta[:, 0, 0] = 0.75
    if S > 5:
        beta[5, 1, 1] = np.nan
    z = _ar1(rng, S, n * m).reshape(S, m, n).transpose(0, 2, 1)
    if saturated:
        g = np.where(z >= 0, 1.0, -1.0) * (800.0 + 50.0 * np.abs(z))
        mu = np.zeros((S, n, m))
        f = g
    else:
        mu = np.broadcast_to((0.3 * _ar1(rng, S, m))[:, None, :], (S, n, m)).copy()
        f = 1.5 * z
    return dict(y=y, theta=theta, beta=beta, f=f, mu=mu)
