"""The NumPy statement of scoring new respondents under ordinal responses (gpirt_amd.ordinal.score_from_draws,
predict_from_draws; csrc/ordinal_score.hip) against brute force, and the properties the device tests lean on.  No GPU.

Tolerances.  The brute force enumerates P_c = sigma(b_c - g) - sigma(b_{c-1} - g) in long double: at |g - b| <= 12 the difference
cancels at most 2^-64 e^12 ~ 1e-14 relative, the statement's own fp64 terms carry m * 4 eps ~ 5e-15 in T: 1e-12 relative covers
both with a margin of 50.  sum_c P_c = 1 + e with |e| <= sum_c P_c (4 eps |logP_c| + 2 eps) <= (4 log C + 2) eps < 8 eps, the long-double
contraction adds C eps / 2 and the division 1 eps: 16 eps.  Jensen gives info >= 0 exactly; h(q) and Hbar each carry a few eps of
their own magnitude <= log C, so info >= -32 eps (1 + log C), and a point mass gives |h(P_k) - Hc_k| within the same bound."""
import numpy as np
import pytest

from _score_bounds import compare as score_compare, delta_of

from gpirt_amd import ordinal as OR
from gpirt_amd import score as SC

EPS = np.finfo(np.float64).eps
LD = np.longdouble
N = 1001


def _draws(S, m, C, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    th = SC.grid()
    f = np.empty((S, N, m))
    B = np.empty((S, m, C - 1))
    t = OR.grid()
    for s in range(S):
        slopes = rng.uniform(0.6, 1.6, m) * rng.choice([-1.0, 1.0], m)
        f[s] = scale * (th[:, None] * slopes[None, :] + 0.3 * np.sin(th[:, None] * rng.uniform(0.5, 2.0, m)[None, :]))
        K = np.sort(np.stack([rng.choice(np.arange(80, 161), C - 1, replace=False) for _ in range(m)]), axis=1)
        B[s] = t[K]
    return f, B


def _cat_new(n, m, C, seed):
    rng = np.random.default_rng(seed + 5)
    cat = rng.integers(1, C + 1, size=(n, m)).astype(np.int8)
    cat[rng.random((n, m)) < 0.2] = 0
    cat[0, :] = 1                      # end categories alone: no w term
    cat[1, :] = C
    cat[n - 1, :] = 0                  # no answers: the prior
    return cat


def _brute(cat, f, B):
    """Everything by enumeration in long double: per draw the C category probabilities of every (k, j) as differences of sigmas."""
    S, _, m = f.shape
    n = cat.shape[0]
    C = B.shape[2] + 1
    pi = np.exp(SC.logprior().astype(LD))
    pi = pi / pi.sum()
    ls = np.empty((S, n), dtype=LD)
    post = np.zeros((n, N), dtype=LD)
    probs = np.zeros((n, m, C), dtype=LD)
    info = np.zeros((n, m), dtype=LD)
    for s in range(S):
        g = f[s].astype(LD)
        bb = np.concatenate([np.full((m, 1), -np.inf), B[s], np.full((m, 1), np.inf)], axis=1).astype(LD)
        sig = 1 / (1 + np.exp(-(bb.T[:, None, :] - g[None, :, :])))             # (C + 1, N, m): P(y <= c)
        P = sig[1:] - sig[:-1]                                                  # (C, N, m)
        H = -(P * np.log(P)).sum(axis=0)
        for r in range(n):
            L = np.ones(N, dtype=LD)
            for j in range(m):
                if cat[r, j]:
                    L = L * P[cat[r, j] - 1, :, j]
            marg = (pi * L).sum()
            wk = pi * L / marg
            ls[s, r] = np.log(marg)
            post[r] += wk
            q = np.einsum("k,ckj->cj", wk, P)
            probs[r] += q.T
            info[r] += -(q * np.log(q)).sum(axis=0) - wk @ H
    return dict(grid_post=post / S, lpd=np.log(np.exp(ls).mean(axis=0)), loglik_mean=ls.mean(axis=0), probs=probs / S, info=info / S)


@pytest.fixture(scope="module")
def case():
    n, m, C, S = 12, 5, 4, 3
    f, B = _draws(S, m, C, 11)
    cat = _cat_new(n, m, C, 11)
    return dict(cat=cat, f=f, B=B, n=n, m=m, C=C, S=S,
                score=OR.score_from_draws(cat, f, B, return_products=True),
                pred=OR.predict_from_draws(cat, f, B, top=3, return_draws=True), brute=_brute(cat, f, B))


def test_statement_against_brute_force(case):
    got, pred, want = case["score"], case["pred"], case["brute"]
    tol = 1e-12
    assert np.all(got["draws"] == case["S"]) and np.all(got["nonfinite"] == 0)
    assert np.array_equal(got["n_obs"], (case["cat"] != 0).sum(axis=1))
    for k in ("lpd", "loglik_mean"):
        gap = np.abs(got[k] - want[k].astype(np.float64))
        print(f"MEASURED {k}: gap {gap.max():.3e}")
        assert (gap <= tol * (1 + np.abs(got[k]))).all(), k
    gp = np.abs(got["grid_post"] - want["grid_post"].astype(np.float64))
    assert (gp <= tol * want["grid_post"].astype(np.float64) + 1e-300).all()
    assert np.allclose(got["grid_post"].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    # the respondent with no answers: the prior and l = 0
    pi = np.exp(SC.logprior()); pi /= pi.sum()
    assert np.abs(got["grid_post"][-1] - pi).max() <= 1e-15 and abs(got["lpd"][-1]) <= 2 * N * EPS
    pp = np.abs(pred["probs"] - want["probs"].astype(np.float64))
    assert (pp <= tol * want["probs"].astype(np.float64) + 1e-300).all()
    ip = np.abs(pred["info"] - want["info"].astype(np.float64))
    print(f"MEASURED probs gap {pp.max():.3e} info gap {ip.max():.3e}")
    assert (ip <= tol * (1 + np.log(case["C"]))).all()
    assert pred["pred_draws"] == case["S"] and pred["pred_skipped"] == 0
    # expected is the mean category of probs; the next items are the unanswered ones by decreasing info
    assert np.allclose(pred["expected"], (pred["probs"] * np.arange(1, case["C"] + 1)).sum(axis=2), rtol=0, atol=0)
    for r in range(case["n"]):
        cand = np.flatnonzero(case["cat"][r] == 0)
        order = cand[np.argsort(-pred["info"][r, cand], kind="stable")][:3]
        assert np.array_equal(pred["next_items"][r, :order.size], order) and (pred["next_items"][r, order.size:] == -1).all()


def test_probs_sum_to_one_and_info_nonnegative(case):
    pred, C = case["pred"], case["C"]
    gap = np.abs(pred["probs"].sum(axis=2) - 1.0)
    print(f"MEASURED sum_c probs - 1: {gap.max() / EPS:.2f} eps")
    assert (gap <= 16 * EPS).all()
    bound = 32 * EPS * (1 + np.log(C))
    assert (pred["info"] >= -bound).all()
    for f, B in zip(case["f"], case["B"]):
        P, H = OR.category_tables(f, B)                       # a point mass at k: q = P[:, k, :], info = h(P_k) - Hc_k = 0
        gap0 = np.abs(OR.category_entropy(P) - H)
        assert (gap0 <= bound).all(), gap0.max()
        assert (np.abs(P.sum(axis=0) - 1.0) <= 16 * EPS).all()


def test_tables_at_the_extremes():
    """+-inf and |f*| beyond exp()'s range: P is a unit vector, no NaN, Hc = 0"""
    f = np.zeros((N, 2))
    f[0, 0], f[1, 0], f[2, 0], f[3, 0] = np.inf, -np.inf, 800.0, -800.0
    B = np.array([[-1.0, 0.5, 2.0], [-0.05, 0.0, 0.05]])
    P, H = OR.category_tables(f, B)
    assert np.isfinite(P).all() and np.isfinite(H).all()
    assert np.array_equal(P[:, 0, 0], [0, 0, 0, 1]) and np.array_equal(P[:, 1, 0], [1, 0, 0, 0])
    assert np.array_equal(P[:, 2, 0], [0, 0, 0, 1]) and np.array_equal(P[:, 3, 0], [1, 0, 0, 0])
    assert (H[:4, 0] == 0).all()
    T = OR.score_product(np.array([[1, 0], [2, 0]], dtype=np.int8), f, B)
    assert T[0, 0] == -OR.SCORE_HELD and T[0, 1] == -OR.SCORE_HELD and T[1, 0] == 0.0 and np.isfinite(T).all()


def test_two_categories_are_the_binary_scorer():
    n, m, S = 9, 6, 3
    f, _ = _draws(S, m, 2, 23)
    B = np.zeros((S, m, 1))
    cat = _cat_new(n, m, 2, 23)
    y = np.where(cat == 0, np.nan, 2.0 * cat - 3.0)
    got = OR.score_from_draws(cat, f, B, return_products=True)
    want = SC.from_draws(y, f, return_products=True)
    big = max(float(np.abs(T).max()) for T in want["products"][0])
    for Tg, Tw in zip(got["products"][0], want["products"][0]):
        gap = np.abs(Tg - Tw).max()
        print(f"MEASURED product gap {gap:.3e} against {2 * m * EPS * big:.3e}")
        assert gap <= 2 * m * EPS * big
    assert all((wc == 0).all() for wc in got["wc"][0])
    score_compare(got, want, delta_of(want["products"][0], m), "C = 2 against the binary statement")


def test_wc_matters(case):
    cat, f, B = case["cat"], case["f"], case["B"]
    full = case["score"]
    bare = OR.score_from_draws(cat, f, B, with_w=False)
    interior = ((cat > 1) & (cat < case["C"])).any(axis=1)
    tol = 2 * N * EPS * (1 + np.abs(full["lpd"]))
    diff = np.abs(full["lpd"] - bare["lpd"])
    assert interior.any() and (~interior).any()
    assert (diff[interior] > tol[interior]).all(), "dropping Wc must move lpd wherever an interior category was answered"
    assert (diff[~interior] == 0).all()
    assert np.array_equal(full["grid_post"], bare["grid_post"])        # the weights do not see it
    # ... and it is a per-respondent constant that changes from draw to draw
    wc = np.array(case["score"]["wc"][0])
    assert (np.ptp(wc[:, interior], axis=0) > 0).all()
    assert np.allclose(wc[0], OR.score_w(cat, B[0]))


def test_pooling_with_a_sign(case):
    cat, f, B = case["cat"], case["f"], case["B"]
    two = OR.score_from_draws(cat, np.stack([f, f]), np.stack([B, B]), signs=[1, -1])
    one = case["score"]
    assert np.allclose(two["post_sum"], one["post_sum"] + one["post_sum"][:, ::-1], rtol=0, atol=0)
    assert np.abs(two["grid_post"] - two["grid_post"][:, ::-1]).max() == 0
    assert np.allclose(two["lpd"], one["lpd"], rtol=0, atol=8 * EPS * (1 + np.abs(one["lpd"]).max()))


def test_refusals():
    with pytest.raises(ValueError, match="item columns"):
        OR.check_cat_new(np.ones((3, 4), dtype=np.int8), m=5)
    with pytest.raises(ValueError, match="0 .. C = 3"):
        OR.check_cat_new(np.full((3, 4), 4), m=4, C=3)
    with pytest.raises(ValueError, match="outside 1..16384"):
        OR.check_cat_new(np.zeros((0, 4), dtype=np.int8))
