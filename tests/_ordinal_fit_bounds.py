"""Rounding bounds for the ordinal fit block (csrc/ordinal_fit.hip) against gpirt_amd.ordinal.fit_from_draws, and the cases the
CPU and GPU tests share.  Every bound is derived from the operations, never from the device's output.  EPS = 2^-52; a library
exp or log1p is taken to be within 2 ulp, a correctly rounded operation within EPS / 2.

ONE TERM.  ll = log1p(E) + max(+-d, 0), E = exp(-|d|).  An error of 2 ulp in E moves log1p(E) by at most 2 EPS of itself
(E / ((1 + E) log1p(E)) <= 1); log1p adds 2 ulp, the addition one rounding: 5 EPS, and as much on the other side of a comparison
of two float64 evaluations: taken as 6 EPS of the term in all (the two share every correctly rounded operation).  w = log1p(-x),
x = exp(-gap): 2 ulp in x move it by 2 A EPS of itself, A = x / ((1 - x) |log1p(-x)|), largest at the smallest gap, one grid
step h; with log1p's own 2 ulp: (2 A(h) + 2) EPS.  logP = -ll - ll + w is a sum of terms of ONE sign (each <= 0), so there is no
cancellation: its relative error is at most the largest term's, plus two additions: CELL(h) = 8 + 2 A(h) ulps.

SUMS.  A float64 sum of L terms of one sign is within (L - 1) EPS / 2 of the exact one in any order; two such sums in different
orders differ by at most (L - 1) EPS, relative.  S draws added one by one: (S - 1) EPS more."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def grid_np(hi=6.0, points=241):
    """gpirt_ordinal_grid in NumPy (long double, rounded once): no built library is needed."""
    k = np.arange(points)
    return (np.asarray(2 * k - (points - 1), dtype=np.longdouble) / np.longdouble(points - 1) * np.longdouble(hi)).astype(np.float64)


def w_amplification(h):
    x = np.exp(-float(h))
    return float(x / ((1.0 - x) * abs(np.log1p(-x))))


def cell_ulps(h=0.05):
    """CELL(h): the relative error of one logP in EPS, two float64 evaluations apart (or one from the exact value)."""
    return 8.0 + 2.0 * w_amplification(h)


def dev_rtol(L, S, h=0.05):
    """dev_obs_sum / dev_rep_sum of a unit with L cells over S draws: terms of one sign (-2 logP >= 0, the factor exact), each
    within CELL EPS, summed in another order ((L - 1) EPS), then S draws ((S - 1) EPS)."""
    return (cell_ulps(h) + L + S) * EPS


def pred_rtol(S):
    """A sum of e_c over S draws: E within 2 ulp on each side moves e = 1 / (1 + E) or E / (1 + E) by at most 2 EPS of itself,
    the addition and the division may round the other way once each (2 x EPS / 2 per side): 4 EPS; S positive terms added in the
    same order from different values: (S - 1) EPS more."""
    return (4.0 + S) * EPS


def lse_atol(M, S, h=0.05):
    """The running logaddexp of one cell over S draws against the exact one.  M >= |logP_s| and |lse| (an array per cell).  The
    inputs' errors (CELL EPS M) enter with weights that sum to 1; each of the S - 1 steps adds log1p(exp(-|a - b|)) in (0, log 2]
    within 4 ulp (< 3 EPS absolute), the rounded difference inside the exp (< 0.3 EPS after the derivative) and one rounded
    addition (EPS / 2 M): < (4 + M) EPS per step."""
    return (cell_ulps(h) * M + (S - 1) * (4.0 + M)) * EPS


def mean_atol(M, S, h=0.05):
    """Welford's mean after S draws: the inputs' errors averaged (CELL EPS M), and per step the rounded delta (|delta| <= 2 M), its
    division and the rounded sum (|mean| <= M): < 3 M EPS per step."""
    return (cell_ulps(h) + 3.0 * S) * M * EPS


def m2_atol(M, S, h=0.05):
    """Welford's M2 after S draws.  A perturbation dx of every input moves sum (x - mean)^2 by at most 2 sum |x - mean| dx <=
    4 S M^2 CELL EPS.  Per step the product delta (x - mean) <= 4 M^2 carries three roundings (< 12 M^2 EPS) and the mean's error
    (3 S M EPS) times |delta| <= 2 M: 6 S M^2 EPS; S steps."""
    return (4.0 * S * cell_ulps(h) + 6.0 * S * S + 12.0 * S) * M * M * EPS


def pooled_m2_atol(M, S, h=0.05):
    """M2 of two chains of S draws each pooled by Chan's formula, M2a + M2b + delta^2 na nb / n, against the 2 S draws' exact one:
    the two chains' own bounds (2 m2_atol(M, S)), the error of delta = mean_b - mean_a (2 mean_atol(M, S)) times d(delta^2 S / 2) =
    |delta| S <= 2 M S, and the formula's six roundings of terms <= 4 M^2 S / 2: 12 S M^2 EPS."""
    return 2.0 * m2_atol(M, S, h) + 2.0 * mean_atol(M, S, h) * 2.0 * M * S + 12.0 * S * M * M * EPS


def total_atol(cell_atol, values):
    """A total over N observed cells (lppd or p_waic): the cells' own bounds added, one more rounded operation per cell (the
    subtraction of log S or the division by S - 1) and a float64 sum of N terms of one sign in a fixed tree: (N + 2) EPS of sum |v|."""
    v = np.abs(np.asarray(values, dtype=np.float64))
    return float(np.sum(cell_atol) + (v.size + 2) * EPS * v.sum())


def magnitude(lp_draws_abs_max, S):
    """M of a cell: max_s |logP_s| + log S bounds |logP_s|, |lse|, |mean| and half of |delta|."""
    return np.asarray(lp_draws_abs_max, dtype=np.float64) + np.log(float(max(S, 1)))


# ---------------------------------------------------------------------------------------------------- the cases ------
SHAPES = [(100, 17, 3, 5), (257, 33, 5, 5), (1000, 64, 8, 4), (300, 20, 2, 4)]      # n, m, C, steps
SEED = 2**35 + 17


def make_case(n, m, C, seed):
    """Graded data (ordinal.make_graded) with about 3 % missing cells, one all-missing column (m // 3), one all-missing row
    (n // 2) and one item that uses a single category (the last item: category 1)."""
    from gpirt_amd import ordinal as OR
    d = OR.make_graded(n, m, C, seed=seed, na_frac=0.03)
    cat = np.array(d["cat"], order="F")
    cat[:, m - 1] = np.where(cat[:, m - 1] > 0, 1, 0)
    cat[:, m // 3] = 0
    cat[n // 2, :] = 0
    d["cat"] = np.asfortranarray(cat.astype(np.int8))
    return d


def theta_start(n, seed):
    rng = np.random.default_rng(seed + 1000)
    return -5.0 + 0.01 * np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01), 0, 1000)


def synthetic_draws(case, C, steps, seed):
    """Continuous g = theta slope + noise and thresholds on the 0.05 grid that wander by a few points per draw: what a chain's
    draws look like, without a device."""
    from gpirt_amd import ordinal as OR
    rng = np.random.default_rng(seed + 5)
    cat = case["cat"]
    n, m = cat.shape
    t = grid_np()
    K = OR.init_thresholds(cat, t, C).astype(np.int64)
    g, B = [], []
    for _ in range(steps):
        g.append(case["theta"][:, None] * case["slopes"][None, :] + 0.5 * rng.standard_normal((n, m)))
        Ks = np.sort(np.clip(K + rng.integers(-2, 3, K.shape), 0, t.size - 1), axis=1)
        for c in range(1, C - 1):
            Ks[:, c] = np.maximum(Ks[:, c], Ks[:, c - 1] + 1)
        B.append(t[np.clip(Ks, 0, t.size - 1)])
    return np.stack(g), np.stack(B)
