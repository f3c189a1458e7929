"""Derived bounds, the shared constructed cases and the trajectory seed of the amplitude tests (tests/test_amp_cpu.py,
tests/test_gpu_amp.py).

DEVICE AGAINST gpirt_amd.amp.step_exact, ONE UPDATE FROM THE SAME f.  u = 2^-53.  Both sides form c = grid[k'] / grid[k] as one
fp64 division and f' = c f as one fp64 multiplication, so f' is the same bits on both sides, and so are the two uniforms, the
proposal and the prior's difference up to its one rounding.  The only rounding between device and statement is in dll_j:
    per observed cell   the argument y (f + mu) carries u |a| per side (y is +-1: the sum's one rounding), ll_term_fast 2 ulp of
                        t (csrc/ll_fast.h), the difference of the two terms one more rounding:
                        2 u (|a0| + |a1|) + 5 u (t0 + t1)                                       (as tests/_ell_bounds.py)
    the additions       thread t adds its n / 256 rows, the tree adds 8 levels: (n / 256 + 9) u sum_i |t0 - t1|
    e_dll_j = sum over observed cells [2 u (|a0| + |a1|) + 5 u (t0 + t1)] + (n / 256 + 9) u sum_i |t0 - t1|
    log_ratio_j = dll_j + (lp[k'] - lp[k]): two roundings on the device, e_ratio_j = e_dll_j + 2 u (|dll_j| + |lp' - lp|)
log u1 is the device library's fp64 logarithm, documented to 1 ulp: |log_u_dev - log u1| <= 2 u |log u1| (one ulp is 2 u
relative), which the decision margins below cover with room.

A TRAJECTORY.  Every accepted update writes f <- c f with the statement's own bits, so f never parts from the statement's as long
as the decisions agree, and the decisions agree as long as no margin |log_ratio - log u1| comes near e_ratio: SEED below is
chosen (tests/test_amp_cpu.py asserts it) so that no update of any item in the 200 has a margin under 100 e_ratio.

THE CHAIN AGAINST conditional_posterior: tests/_ell_bounds.py's tv_bound with the index series' own ESS (index_ess), per item.

draw_fstar UNDER FIXED AMPLITUDES.  f* = m + sd z with sd = fl(a s) against the unit run's f*_1 = m + s z, the same m, s, z:
f* - m = fl(a s) z (1 + d1)(1 + d2), one rounding for the product and one for the sum relative to |f*| -- so
    |(f* - m) - a (f*_1 - m)| <= u |a s z| (3 + ...) + u (|f*| + a |f*_1|) + u (|f* - m| + a |f*_1 - m|)
held here as 4 u (|m| + a |f*_1 - m| + |f* - m|) + 4 u a (|m| + |f*_1 - m|): every subtraction against m and every product
counted once, with room of two.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
SEED = 1                      # the trajectory's seed (tests/test_amp_cpu.py asserts that none of its decisions is a near-tie);
                              # its 200 updates hold accepted, rejected and out-of-range ones in several items
P, W, N, M, UPDATES = 17, 2, 40, 3, 200          # the trajectory case of the issue
LO, HI = 0.1, 10.0
MARGIN = 100.0                # times e_ratio: what a trajectory decision must keep clear of


def case(n, m, points, seed, lo=LO, hi=HI, k=None, nan_share=0.05):
    """A constructed state: theta, beta, mu, f = a_k L z (fp64; L the factor of the unit squared exponential at theta), y
    (+1 / -1, `nan_share` NaN), the grid, the default prior and the starting indices k (m values; default: the grid point
    nearest 1 for every item)."""
    from gpirt_amd import amp as A, ell as E
    rng = np.random.default_rng(seed)
    theta = np.round(rng.standard_normal(n).clip(-4, 4), 2)
    g = A.grid(lo, hi, points)
    lp = A.default_log_prior(g)
    k = np.full(m, A.nearest_one(g), dtype=np.int64) if k is None else np.broadcast_to(np.asarray(k, dtype=np.int64), (m,)).copy()
    beta = np.stack([rng.normal(0, 1, m), rng.normal(1, 0.3, m)])
    mu = beta[0][None, :] + beta[1][None, :] * theta[:, None]
    L = E.factor(theta, "se", 1.0).astype(np.float64)
    f = (L @ rng.standard_normal((n, m))) * g[k][None, :]
    p = 1 / (1 + np.exp(-(f + mu)))
    y = np.where(rng.random((n, m)) < p, 1.0, -1.0)
    y[rng.random((n, m)) < nan_share] = np.nan
    return dict(theta=theta, beta=beta, mu=np.asfortranarray(mu), f=np.asfortranarray(f), y=np.asfortranarray(y), grid=g,
                log_prior=lp, k=k, n=n, m=m, points=points, seed=seed, lo=lo, hi=hi)


def dll_bounds(f, f_prop, mu, y, dll, lp_diff):
    """(e_dll, e_ratio) per item (the module docstring) for the move f -> f_prop (both n x m fp64), dll (m) and lp' - lp (m)"""
    from gpirt_amd import amp as A
    n = f.shape[0]
    obs = ~np.isnan(y)
    ys = np.where(obs, y, 0.0)
    with np.errstate(all="ignore"):
        a0, a1 = ys * (f + mu), ys * (f_prop + mu)
        t0, t1 = A.ll_term(a0).astype(np.float64), A.ll_term(a1).astype(np.float64)
    cells = np.where(obs, 2 * U * (np.abs(a0) + np.abs(a1)) + 5 * U * (t0 + t1), 0.0).sum(axis=0)
    adds = (n / 256 + 9) * U * np.where(obs, np.abs(t0 - t1), 0.0).sum(axis=0)
    e_dll = cells + adds
    return e_dll, e_dll + 2 * U * (np.abs(np.asarray(dll, dtype=np.float64)) + np.abs(np.asarray(lp_diff, dtype=np.float64)))


def step_bounds(c, f, k, ref):
    """(e_dll, e_ratio) per item of one step_exact record `ref` taken from (f, k) of case c; NaN for items out of range"""
    g, lp = c["grid"], c["log_prior"]
    m = c["m"]
    inside = (ref["k_prop"] >= 0) & (ref["k_prop"] < g.shape[0])
    kp = np.where(inside, ref["k_prop"], k)
    with np.errstate(all="ignore"):
        fp = (g[kp] / g[k])[None, :] * f
        e_dll, e_ratio = dll_bounds(f, fp, c["mu"], c["y"], ref["dll"].astype(np.float64), lp[kp] - lp[k])
    nan = np.full(m, np.nan)
    return np.where(inside, e_dll, nan), np.where(inside, e_ratio, nan)


def chain(c, widths, updates, seed=None, item0=0):
    """The NumPy chain from a case: `updates` step_exact calls with no step() in between.  Returns ks (updates x m: the indices
    after every update), status (updates x m), the smallest margin |log_ratio - log u1| / (e_ratio + 2 u |log u1|) over all updates and items that
    reached a decision (with where it was), the final f and k and the four counters per item (4 x m)."""
    from gpirt_amd import amp as A
    seed = c["seed"] if seed is None else seed
    k, f = c["k"].copy(), c["f"]
    m = c["m"]
    ks = np.empty((updates, m), dtype=np.int64)
    status = []
    counts = np.zeros((4, m), dtype=np.int64)
    worst, where = np.inf, None
    for t in range(1, updates + 1):
        r = A.step_exact(f, c["mu"], c["y"], k, widths, seed, t, c["grid"], c["log_prior"], item0)
        _, e_ratio = step_bounds(c, f, k, r)
        for j, st in enumerate(r["status"]):
            counts[0, j] += 1
            counts[1, j] += st == "accepted"
            counts[2, j] += st == "out_of_range"
            counts[3, j] += st == "failed"
            if st in ("accepted", "rejected"):
                # (the device's logarithm of u1 is within one ulp, 2 u |log u1|: counted with the ratio's bound)
                ratio = abs(float(r["log_ratio"][j] - r["log_u"][j])) / (e_ratio[j] + 2 * U * abs(float(r["log_u"][j])))
                if ratio < worst:
                    worst, where = ratio, (t, j)
        k, f = r["k"], r["f"]
        ks[t - 1] = k
        status.append(r["status"])
    return dict(ks=ks, status=status, worst_margin=worst, where=where, f=f, k=k, counts=counts)


def transition_matrix(fcol, mucol, ycol, k_at, amp_grid, log_prior, width):
    """The P x P transition matrix of one item's update as step_exact's rule implies it, with nu held fixed at (fcol, k_at):
    from k the proposal k' = k + d, d uniform on -w .. w without 0, each with probability 1 / (2 w); outside the grid the chain
    stays; inside it moves with probability min(1, exp(dll + lp[k'] - lp[k])), dll in long double from the curves
    (a_k / a_k_at) fcol.  Long double throughout."""
    from gpirt_amd import amp as A
    g = np.asarray(amp_grid, dtype=np.float64).astype(LD)
    P = g.shape[0]
    ll = np.array([A._loglik((g[kk] / g[k_at]) * fcol.astype(LD), mucol, ycol) for kk in range(P)], dtype=LD)
    T = np.zeros((P, P), dtype=LD)
    w = int(width)
    for kk in range(P):
        for d in list(range(-w, 0)) + list(range(1, w + 1)):
            kp = kk + d
            if kp < 0 or kp >= P:
                T[kk, kk] += LD(1) / LD(2 * w)
                continue
            acc = min(LD(1), np.exp((ll[kp] - ll[kk]) + (LD(log_prior[kp]) - LD(log_prior[kk]))))
            T[kk, kp] += acc / LD(2 * w)
            T[kk, kk] += (LD(1) - acc) / LD(2 * w)
    return T


def fstar_bound(a, mean, fstar_unit, fstar):
    """the bound of the module docstring on |(f* - mean) - a (f*_1 - mean)|, elementwise (a: per column)"""
    a = np.asarray(a, dtype=np.float64)[None, :]
    d1, d = np.abs(fstar_unit - mean), np.abs(fstar - mean)
    return 4 * U * (np.abs(mean) + a * d1 + d) + 4 * U * a * (np.abs(mean) + d1)
