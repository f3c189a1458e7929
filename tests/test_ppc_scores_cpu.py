"""The score-based checks of the PPC without a device: the NumPy statement of the header (gpirt_amd.ppc.scores_*) on a
hand-worked example and on constructed edge cases, the default cuts, the argument checks and the C ABI of version 120."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpirt_amd import _lib
from gpirt_amd import ppc as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.nan


def _hand():
    """5 respondents x 3 items, K = 2 with the cut 1 (group 0: rest score 0, group 1: rest score >= 1), g = 0 everywhere
    (p = 1/2, p q = 1/4: E = N / 2, V = N / 4).  X = 2 1 0 3 1, Xr = 2 0 2 3 1; the replicate's value in the missing cell is 1
    and must not count."""
    y = np.array([[1, 1, -1], [1, -1, -1], [-1, -1, -1], [1, 1, 1], [-1, 1, NAN]], dtype=float)
    rep = np.array([[1, 0, 1], [0, 0, 0], [1, 1, 0], [1, 1, 1], [0, 1, 1]])
    return y, rep


def test_hand_worked_example():
    y, rep = _hand()
    d = P.scores_from_rep(y, np.zeros((1, 5, 3)), rep[None], cuts=(1,), top=3)
    last = d["last"]
    # 1. the score distribution
    assert d["hist_obs"].tolist() == [1, 2, 1, 1] and last["xr"].tolist() == [2, 0, 2, 3, 1] and last["hist"].tolist() == [1, 1, 2, 1]
    assert d["hist_sum"].tolist() == [1, 1, 2, 1] and d["hist_sumsq"].tolist() == [1, 1, 4, 1]
    assert d["hist_ge"].tolist() == [1, 0, 1, 1] and d["hist_gt"].tolist() == [0, 0, 1, 0]
    assert d["cdf_ge"].tolist() == [1, 0, 1, 1] and d["cdf_gt"].tolist() == [0, 0, 0, 0]          # C: 1 3 4 5 against 1 2 4 5
    # Vn = n_s S2 - S1^2: the data 5 x 15 - 7^2 = 26, the replicate 5 x 18 - 8^2 = 26
    assert d["var_obs"].tolist() == [26, 5] and d["var_rep_sum"].tolist() == [26]
    assert d["var_ge"].tolist() == [1] and d["var_gt"].tolist() == [0]
    assert d["score_var_obs"] == 26 / 25 == d["score_var_rep_mean"] and d["ppp_var"] == 1.0 and d["n_scored"] == 5
    assert d["score_hist_rep_mean"].tolist() == [1.0, 1.0, 2.0, 1.0] and np.isnan(d["score_hist_rep_sd"]).all()
    assert d["ppp_hist_mid"].tolist() == [0.5, 0.0, 1.0, 0.5]
    # 2. the item-rest correlations: (A, B, Cq, D) per item
    assert d["sums_obs"].T.tolist() == [[3, 4, 6, 3], [3, 4, 6, 3], [1, 5, 9, 2]]
    assert last["sums"].T.tolist() == [[3, 5, 7, 4], [3, 5, 9, 3], [2, 5, 9, 3]]
    # NUM, VA, VC: the data (3, 6, 14), (3, 6, 14), (3, 3, 11); the replicate (5, 6, 10), (0, 6, 20), (2, 4, 11)
    assert d["r_obs"].tolist() == [3 / np.sqrt(84.0), 3 / np.sqrt(84.0), 3 / np.sqrt(33.0)]
    assert last["r"].tolist() == [5 / np.sqrt(60.0), 0.0, 2 / np.sqrt(44.0)]
    assert d["r_ge"].tolist() == [1, 0, 0] and d["r_gt"].tolist() == [1, 0, 0] and d["r_undefined_count"].tolist() == [0, 0, 0]
    assert d["r_rep_sum"].tolist() == last["r"].tolist() and d["r_rep_sumsq"][0] == last["r"][0] * last["r"][0]
    assert d["r_rep_mean"].tolist() == last["r"].tolist() and np.isnan(d["r_rep_sd"]).all() and d["ppp_r"].tolist() == [1.0, 0.0, 0.0]
    # 3. the tables [group, item]
    assert d["tNo"].tolist() == [[2, 2, 1], [3, 3, 3]] and d["tT"].tolist() == [[1, 1, 0], [2, 2, 1]]
    assert last["tNr"].tolist() == [[1, 2, 1], [4, 3, 3]] and last["tR"].tolist() == [[0, 1, 0], [3, 2, 2]]
    assert np.array_equal(last["tEo"], d["tNo"].astype(np.int64) * 2**43) and np.array_equal(last["tVo"], d["tNo"].astype(np.int64) * 2**42)
    assert np.array_equal(last["tEr"], last["tNr"].astype(np.int64) * 2**43) and np.array_equal(last["tVr"], last["tNr"].astype(np.int64) * 2**42)
    # R No against T Nr: (0, 1), (2, 2), (0, 0); (9, 8), (6, 6), (6, 3)
    assert d["cell_ge"].tolist() == [[0, 1, 1], [1, 1, 1]] and d["cell_gt"].tolist() == [[0, 0, 0], [1, 0, 1]]
    assert d["cell_empty"].tolist() == [[0, 0, 0], [0, 0, 0]]
    third = 0.25 / 0.75
    # X2(T): 0 + 1/3, 0 + 1/3, 1 + 1/3; X2(R): 1 + 1, 0 + 1/3, 1 + 1/3
    assert last["chi"].tolist() == [[0.0 + third, 0.0 + third, 1.0 + third], [2.0, 0.0 + third, 1.0 + third]]
    assert d["chi_ge"].tolist() == [1, 1, 1] and d["chi_gt"].tolist() == [1, 0, 0]
    assert d["chi_obs_sum"].tolist() == last["chi"][0].tolist() and d["chi2_rep_mean"].tolist() == last["chi"][1].tolist()
    assert d["obs_rate"].tolist() == [[0.5, 0.5, 0.0], [2 / 3, 2 / 3, 1 / 3]]
    assert d["rep_rate"].tolist() == [[0.0, 0.5, 0.0], [0.75, 2 / 3, 2 / 3]] and (d["exp_rate"] == 0.5).all()
    assert d["ppp_cell_mid"].tolist() == [[0.0, 0.5, 0.5], [1.0, 0.5, 1.0]] and d["ppp_chi2_mid"].tolist() == [1.0, 0.5, 0.5]
    # the worst items: the smallest ppp_chi2_mid first, the tie to the lower j
    assert d["worst"]["items"].tolist() == [1, 2, 0] and d["worst"]["ppp_chi2_mid"].tolist() == [0.5, 0.5, 1.0]
    assert d["cuts"].tolist() == [1] and d["group_lo"].tolist() == [0, 1] and d["group_hi"].tolist() == [0, 2]
    assert (d["score_draws"], d["score_skipped"], d["K"], d["m"], d["n"]) == (1, 0, 2, 3, 5)
    # the steps: the tables, one draw's statistics, the accumulators
    obs = P.scores_observed(y, (1,))
    tab = P.scores_tables(y, np.zeros((5, 3)), rep, obs)
    st = P.scores_draw_stats(tab)
    assert st["chi"].tolist() == last["chi"].tolist() and st["Vn"] == 26 and bool(st["var_ge"]) and not bool(st["var_gt"])
    again = P.scores_from_tables([tab], top=3)
    for name, _dt, _kind in _lib.SCORES_RAW:
        assert np.array_equal(again[name], d[name], equal_nan=True), name
    # the same constants from a state block's arrays
    obs2 = P.scores_observed_from_arrays((1,), d["hist_obs"], d["sums_obs"], d["tNo"], d["tT"])
    assert np.array_equal(obs2["r"], obs["r"]) and obs2["var"] == obs["var"] and np.array_equal(obs2["n_item"], [5, 5, 4])


def test_all_yes_replicate_is_undefined_and_two_draws_pool():
    y, rep = _hand()
    ones = np.ones((5, 3), dtype=int)
    d = P.scores_from_rep(y, np.zeros((2, 5, 3)), np.stack([ones, rep]), cuts=(1,))
    assert d["r_undefined_count"].tolist() == [1, 1, 1] and d["r_undefined"].tolist() == [1.0, 1.0, 1.0]      # VA = 0 in draw 0
    one = P.scores_from_rep(y, np.zeros((1, 5, 3)), rep[None], cuts=(1,))
    for k in ("r_ge", "r_gt", "r_rep_sum", "r_rep_sumsq", "r_rep_mean", "ppp_r"):                # only draw 1 entered
        assert np.array_equal(d[k], one[k]), k
    # the all-yes draw: Xr = the observed count 3 3 3 3 2, every rest score >= 1: group 0 is empty in the replicate
    assert d["cell_empty"].tolist() == [[1, 1, 1], [0, 0, 0]] and d["sum_nr"][0].tolist() == one["sum_nr"][0].tolist()
    assert d["hist_sum"].tolist() == [1, 1, 3, 5] and d["hist_sumsq"].tolist() == [1, 1, 5, 17]
    assert d["score_hist_rep_sd"].tolist() == [np.sqrt(0.5), np.sqrt(0.5), np.sqrt(0.5), np.sqrt(4.5)]
    assert d["score_draws"] == 2 and np.isnan(d["r_rep_sd"]).all()


def test_empty_group_missing_row_and_skipped_draws():
    # nobody scores: group 1 (rest score >= 1) is empty in the data -- a NaN rate, and every draw counts in cell_empty
    y = -np.ones((4, 3))
    rep = np.array([[1, 1, 0], [0, 0, 0], [0, 1, 0], [0, 0, 0]])
    d = P.scores_from_rep(y, np.zeros((1, 4, 3)), rep[None], cuts=(1,))
    assert d["tNo"].tolist() == [[4, 4, 4], [0, 0, 0]] and np.isnan(d["obs_rate"][1]).all() and np.isnan(d["exp_rate"][1]).all()
    assert d["cell_empty"][1].tolist() == [1, 1, 1] and np.isnan(d["ppp_cell"][1]).all() and np.isnan(d["r_obs"]).all()
    assert d["r_undefined_count"].tolist() == [1, 1, 1] and np.isnan(d["ppp_r"]).all()
    # a respondent without an observed cell is left out of everything
    rng = np.random.default_rng(4)
    y = np.where(rng.random((30, 5)) < 0.5, 1.0, -1.0)
    y[rng.random((30, 5)) < 0.1] = NAN
    y[7] = NAN
    g = rng.normal(size=(3, 30, 5))
    rp = rng.random((3, 30, 5)) < 0.5
    a = P.scores_from_rep(y, g, rp, cuts=(1, 3))
    keep = np.arange(30) != 7
    b = P.scores_from_rep(y[keep], g[:, keep], rp[:, keep], cuts=(1, 3))
    for name, _dt, _kind in _lib.SCORES_RAW:
        assert np.array_equal(a[name], b[name], equal_nan=True), name
    assert a["n_scored"] == 29 == a["hist_obs"].sum() and a["last"]["xr"][7] == 0
    # a non-finite g in an observed cell skips the draw whole; a NaN in a missing cell is ignored
    g2 = g.copy()
    i, j = np.argwhere(~np.isnan(y))[0]
    g2[1, i, j] = np.inf
    g2[2, 7, 0] = NAN
    c = P.scores_from_rep(y, g2, rp, cuts=(1, 3))
    e = P.scores_from_rep(y, g[[0, 2]], rp[[0, 2]], cuts=(1, 3))
    assert (c["score_draws"], c["score_skipped"]) == (2, 1)
    for name, _dt, _kind in _lib.SCORES_RAW:
        assert np.array_equal(c[name], e[name], equal_nan=True), name
    # no draw at all: every mean is NaN
    z = P.scores_from_rep(y, g[:0], rp[:0], cuts=(1, 3))
    assert z["score_draws"] == 0 and np.isnan(z["score_hist_rep_mean"]).all() and np.isnan(z["ppp_chi2"]).all()
    assert np.isnan(z["score_var_rep_mean"]) and z["score_var_obs"] == a["score_var_obs"] and z["worst"]["items"].tolist() == [-1] * 20


def test_default_cuts_from_a_known_score_vector():
    scores = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 10]
    y = -np.ones((len(scores) + 1, 10))
    for i, s in enumerate(scores):
        y[i, :s] = 1.0
    y[-1] = NAN                                          # left out of the quantiles
    y = y[np.random.default_rng(0).permutation(len(y))]
    assert P.default_score_cuts(y) == (1, 2, 3, 4, 5, 6, 7, 8)           # the sorted scores at 2, 4, .., 16
    assert P.default_score_cuts(y, groups=3) == (3, 6)                   # ... at 6 and 12
    assert P.default_score_cuts(y, groups=16)[0] == 1 and len(P.default_score_cuts(y, groups=16)) == 8      # duplicates dropped
    top = np.ones((6, 4))                                # everybody at m: no quantile in 1 .. m - 1
    for bad in (-np.ones((6, 4)), top, np.full((3, 4), NAN)):
        with pytest.raises(ValueError, match="fewer than two score groups"):
            P.default_score_cuts(bad)
    with pytest.raises(ValueError, match="groups must be"):
        P.default_score_cuts(y, groups=17)
    d = P.scores_from_rep(y, np.zeros((0,) + y.shape), np.zeros((0,) + y.shape), top=2)
    assert d["cuts"].tolist() == [1, 2, 3, 4, 5, 6, 7, 8] and d["K"] == 9


def test_replicate_from_the_modules_philox():
    rng = np.random.default_rng(9)
    y = np.where(rng.random((40, 6)) < 0.5, 1.0, -1.0)
    y[rng.random((40, 6)) < 0.1] = NAN
    g = rng.normal(size=(2, 40, 6))
    d, gap = P.scores_from_draws(y, g, 11, [3, 4], cuts=(2, 4))
    assert 0 < gap < 1
    ob = ~np.isnan(y)
    reps = []
    for s, it in enumerate((3, 4)):
        p = 1.0 / (1.0 + np.exp(-g[s]))
        reps.append(ob & (P.replicate_uniforms(11, it, 40, 6) < p))
    want = P.scores_from_rep(y, g, np.stack(reps), cuts=(2, 4))
    for name, _dt, _kind in _lib.SCORES_RAW:
        assert np.array_equal(d[name], want[name], equal_nan=True), name
    assert np.array_equal(d["last"]["xr"], reps[1].sum(axis=1))


def test_refusals_say_what_is_wrong():
    assert P.check_score_cuts([1, 2.0, 5], 7) == (1, 2, 5)
    for bad, m, word in (((2, 1), 5, "increasing"), ((1, 1), 5, "increasing"), ((0, 2), 5, "increasing integers in 1..4"),
                         ((1, 5), 5, "increasing integers in 1..4"), ((1.5,), 5, "integers"), (("a",), 5, "integers"),
                         ((), 5, "1 score groups"), (tuple(range(1, 17)), 40, "17 score groups"), ((1,), 1, "outside 2..4096"),
                         ((1,), 4097, "outside 2..4096")):
        with pytest.raises(ValueError, match=word):
            P.check_score_cuts(bad, m)
    with pytest.raises(ValueError, match="beyond 65534"):
        P.check_score_cuts((1,), 5, n=65535)
    for top in (0, 65, 2.5):
        with pytest.raises(ValueError, match="top must be"):
            P.check_scores_top(top)
    with pytest.raises(ValueError, match="top must be"):
        P.scores_worst(np.zeros(4), top=65)
    with pytest.raises(ValueError, match="unknown field 'no_such_field'"):
        P.scores_field("no_such_field", 5, 3, 2)
    assert P.scores_field("tEo", 5, 3, 2) == ((2, 3), np.int64) and P.scores_field("ppp_var", 5, 3, 2) == ((), np.float64)
    assert P.scores_field("xr", 5, 3, 2) == ((5,), np.int32) and P.scores_field("chi", 5, 3, 2) == ((2, 3), np.float64)
    y, rep = _hand()
    with pytest.raises(ValueError, match="increasing"):
        P.scores_from_rep(y, np.zeros((1, 5, 3)), rep[None], cuts=(2, 1))


def _header_struct(name):
    """the (type, field, array length or None) triples of a struct of the header, in order"""
    src = open(os.path.join(ROOT, "include", "gpirt_hip.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    defs = dict(re.findall(r"#define\s+(GPIRT_\w+)\s+(\d+)", src))
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, rest = re.match(r"((?:const\s+)?\w+\s*\**)\s*(.*)", decl).groups()
        for item in rest.split(","):
            nm, dim = re.match(r"\s*(\w+)\s*(?:\[(.*?)\])?", item).groups()
            out.append((typ.replace(" ", ""), nm, None if dim is None else int(defs.get(dim, dim))))
    return out


def test_c_abi_of_version_120():
    lib = _lib.load()
    assert lib.gpirt_version() >= 120
    names = ("gpirt_ppc_scores_check", "gpirt_sampler_ppc_scores_enable", "gpirt_sampler_ppc_scores_get",
             "gpirt_sampler_ppc_scores_state", "gpirt_ppc_scores_combine")
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # _lib.PpcScores mirrors the header's struct field for field: name, type and length
    ctype = {"int": C.c_int, "double*": C.POINTER(C.c_double), "void*": C.c_void_p, "int64_t*": C.POINTER(C.c_int64), "int64_t": C.c_int64}
    fields = _header_struct("gpirt_ppc_scores")
    assert [f[1] for f in fields] == [f[0] for f in _lib.PpcScores._fields_]
    for (typ, nm, dim), (pn, pt) in zip(fields, _lib.PpcScores._fields_):
        assert pt is (ctype[typ] if dim is None else ctype[typ] * dim), nm
    p = _lib.PpcScores()
    assert C.sizeof(p) == 4 * 2 + 4 * 16 + 8 * (7 + 1 + 9 + 5) + 8 * 31 + 8 * 4 + 8 * 5 + 8 * 4
    assert len(_lib.SCORES_RAW) == 31 and _lib.SCORES_RAW[:6] == _lib.SCORES_CONST
    assert (len(_lib.SCORES_HIST_FIELDS), len(_lib.SCORES_ITEM_FIELDS), len(_lib.SCORES_CELL_FIELDS)) == (7, 9, 5)
    # the argument check alone: no device is touched
    c2 = (C.c_int * 2)
    assert lib.gpirt_ppc_scores_check(100, 10, 3, c2(2, 5)) == 0
    for n, m, K, cuts, word in ((65535, 10, 3, c2(2, 5), "beyond 65534"), (100, 1, 3, c2(2, 5), "outside 2..4096"),
                                (100, 4097, 3, c2(2, 5), "outside 2..4096"), (100, 10, 1, c2(2, 5), "1 score groups"),
                                (100, 10, 17, c2(2, 5), "17 score groups"), (100, 10, 3, c2(5, 2), "increasing"),
                                (100, 10, 3, c2(2, 10), "increasing integers in 1..9"), (100, 10, 3, None, "score groups")):
        assert lib.gpirt_ppc_scores_check(n, m, K, cuts) == _lib.E_ARG and word in _lib.last_error(), word
    # argument errors come back before any device is touched
    assert lib.gpirt_ppc_scores_combine(None, 1, None, C.byref(p)) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_scores_enable(None, 2, None, 1) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_scores_get(None, b"counts", None, 0) == _lib.E_ARG
    _, arr = P.scores_struct(5, 3, top=4)
    assert arr["obs_rate"].shape == (3, 5) and arr["cell_ge"].dtype == np.uint32 and arr["worst_items"].shape == (4,)
    assert arr["hist_obs"].shape == (6,) and arr["sums_obs"].shape == (4, 5) and arr["sum_nr"].dtype == np.uint64
