"""The person fit of the PPC without a device: the NumPy statement of the header (gpirt_amd.ppc.person_*) on hand-built cases
with known answers, the Guttman count against a prefix count, the lz identity in long double, the default order and cuts, the
argument checks and the C ABI of version 121."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpirt_amd import _lib
from gpirt_amd import ppc as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = np.nan
IDENT4 = np.arange(4)


def _pattern(*rows):
    """rows of 1 / 0 / None (missing) as a y matrix"""
    return np.array([[NAN if v is None else (1.0 if v else -1.0) for v in r] for r in rows])


def test_guttman_patterns_with_known_answers():
    # in position order: a perfect pattern, the reversed one, one with a missing cell, all yes, all no, nothing observed
    y = _pattern((1, 1, 0, 0), (0, 0, 1, 1), (0, None, 1, 1), (1, 1, 1, 1), (0, 0, 0, 0), (None,) * 4, (0, 1, 0, 1))
    o = P.person_observed(y, IDENT4, (2,))
    assert o["N"].tolist() == [4, 4, 3, 4, 4, 0, 4] and o["x"].tolist() == [2, 2, 2, 4, 0, 0, 2]
    # perfect: G = 0; reversed: G = Q = 4; the missing cell removes exactly its pairs (2 of the reversed pattern's 4);
    # (0, 1, 0, 1): the pairs (0, 1), (0, 3), (2, 3)
    assert o["g"].tolist() == [0, 4, 2, 0, 0, 0, 3] and o["q"].tolist() == [4, 4, 2, 0, 0, 0, 4]
    assert o["tN"].tolist() == [[2, 2, 1, 2, 2, 0, 2], [2, 2, 2, 2, 2, 0, 2]] and o["tT"].tolist() == [[2, 0, 0, 2, 0, 0, 1], [0, 2, 2, 2, 0, 0, 1]]
    # one draw whose replicate is the data itself, g = 0
    d = P.person_from_rep(y, np.zeros((1, 7, 4)), (y > 0)[None], IDENT4, (2,), top=3)
    assert d["guttman_obs"][:5].tolist() == [0.0, 4.0, 2.0, 0.0, 0.0] and np.isnan(d["guttman_obs"][5])
    assert d["guttman_norm_obs"][:3].tolist() == [0.0, 1.0, 1.0] and np.isnan(d["guttman_norm_obs"][3:6]).all()
    # X in {0, N}: Q = 0, the draw is undefined for the Guttman check; nothing observed: nothing moves, NaN on the way out
    assert d["g_undefined_count"].tolist() == [0, 0, 0, 1, 1, 0, 0] and d["g_ge"].tolist() == [1, 1, 1, 0, 0, 0, 1]
    assert d["g_gt"].tolist() == [0] * 7 and d["ppp_guttman_mid"][:3].tolist() == [0.5, 0.5, 0.5]
    assert np.isnan(d["ppp_guttman"][3:6]).all() and d["guttman_undefined"][3] == 1.0
    for f in _lib.PERSON_RESP_FIELDS:
        assert np.isnan(d[f][5]), f
    assert np.isnan(d["obs_rate"][:, 5]).all() and np.isnan(d["ppp_cell"][:, 5]).all() and d["n_scored"] == 6
    for name, _dt, kind in _lib.PERSON_RAW:
        assert not (d[name][..., 5]).any(), name
    assert d["gn_rep_sum"].tolist() == [0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.75] and d["g_rep_sum"].tolist() == [0, 4, 2, 0, 0, 0, 3]
    assert d["guttman_norm_rep_mean"][[0, 1, 2, 6]].tolist() == [0.0, 1.0, 1.0, 0.75]
    # g = 0: Vl = 0, lz is undefined for everybody with a cell
    assert d["lz_undefined_count"].tolist() == [1, 1, 1, 1, 1, 0, 1] and np.isnan(d["lz_obs_mean"]).all()
    # a random order: the same patterns laid out through it give the same counts
    order = np.array([2, 0, 3, 1])
    y2 = np.empty_like(y)
    y2[:, order] = y
    o2 = P.person_observed(y2, order, (2,))
    for k in ("N", "x", "g", "q", "tN", "tT"):
        assert np.array_equal(o2[k], o[k]), k


def _prefix_guttman(ob, bit):
    one = ob & bit
    zero = ob & ~bit
    before = np.cumsum(zero, axis=1) - zero
    return (one * before).sum(axis=1)


@pytest.mark.parametrize("n,m", [(40, 2), (25, 3), (60, 37), (12, 70)])
def test_pair_count_agrees_with_a_prefix_count(n, m):
    rng = np.random.default_rng(n + m)
    ob = rng.random((n, m)) > 0.15
    bit = rng.random((n, m)) < 0.5
    assert np.array_equal(P.person_guttman(ob, bit), _prefix_guttman(ob, bit))
    # ... and through person_observed under a random order
    y = np.where(bit, 1.0, -1.0)
    y[~ob] = NAN
    order = rng.permutation(m)
    o = P.person_observed(y, order, (1,))
    assert np.array_equal(o["g"], _prefix_guttman(ob[:, order], bit[:, order]))
    G, Q = o["g"], o["q"]
    assert (G <= Q).all() and (G >= 0).all()


def test_lz_identity_in_long_double():
    """sum (Y - p) g = l(y) - E[l] and sum p q g^2 = Var[l], with l(z) = sum z log p + (1 - z) log q"""
    ld = np.longdouble
    rng = np.random.default_rng(5)
    n, m = 20, 9
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.2] = NAN
    y[4] = NAN
    g = 2.0 * rng.normal(size=(n, m))
    rep = rng.random((n, m)) < 0.5
    order = rng.permutation(m)
    obs = P.person_observed(y, order, (3, 6))
    t = P.person_tables(y, g, rep, obs)
    assert t["lz"].dtype == ld
    ob = ~np.isnan(y)
    gl = g.astype(ld)
    p = 1 / (1 + np.exp(-gl))
    q = 1 / (1 + np.exp(gl))
    lp, lq = np.log(p), np.log(q)
    El = np.where(ob, p * lp + q * lq, 0).sum(axis=1)
    Vl = np.where(ob, p * q * (lp - lq) ** 2, 0).sum(axis=1)
    tiny = 64 * float(np.finfo(ld).eps)
    for z, row in (((y > 0), 0), (rep, 1)):
        l = np.where(ob, np.where(z, lp, lq), 0).sum(axis=1)
        assert (np.abs(t["lz"][row] - (l - El)) <= tiny * (1 + np.abs(l) + np.abs(El))).all()
    assert (np.abs(t["lz"][2] - Vl) <= tiny * (1 + Vl)).all() and (t["lz"][:, 4] == 0).all()
    st = P.person_draw_stats(t)
    Wo, Vd = t["lz"][0].astype(float), t["lz"][2].astype(float)
    live = obs["live"]
    assert np.array_equal(st["lz_obs"][live], Wo[live] / np.sqrt(Vd[live])) and st["lz_def"].tolist() == live.tolist()


def test_cells_and_chi_square_worked_by_hand():
    """2 respondents x 4 items, K = 2 with the cut 2, g = 0 everywhere: p = 1/2, p q = 1/4, so E = tN / 2 and V = tN / 4 per cell.
    Respondent 0: data (1 1 | 0 0), replicate (1 0 | 1 0); respondent 1: data (1 . | 0 1) with a missing cell, replicate (0 1 | 1 1)
    whose value in the missing cell must not count."""
    y = _pattern((1, 1, 0, 0), (1, None, 0, 1))
    rep = np.array([[1, 0, 1, 0], [0, 1, 1, 1]])
    d = P.person_from_rep(y, np.zeros((1, 2, 4)), rep[None], IDENT4, (2,), top=2)
    last = d["last"]
    assert d["tN"].tolist() == [[2, 1], [2, 2]] and d["tT"].tolist() == [[2, 1], [0, 1]] and last["tR"].tolist() == [[1, 0], [1, 2]]
    assert np.array_equal(last["tE"], d["tN"].astype(np.int64) * 2**43) and np.array_equal(last["tV"], d["tN"].astype(np.int64) * 2**42)
    assert last["xr"].tolist() == [2, 2] and last["gr"].tolist() == [1, 2] and last["qr"].tolist() == [4, 2]
    # R against T, cell by cell: (1, 2) (0, 1) | (1, 0) (2, 1)
    assert d["cell_ge"].tolist() == [[0, 0], [1, 1]] and d["cell_gt"].tolist() == [[0, 0], [1, 1]]
    assert d["sum_r"].tolist() == [[1, 0], [1, 2]] and d["sum_e"].tolist() == [[1.0, 0.5], [1.0, 1.0]]
    # X2 = sum (C - E)^2 / V.  Respondent 0: data (2 - 1)^2 / 0.5 + (0 - 1)^2 / 0.5 = 4, replicate 0 + 0 = 0.
    # Respondent 1: data (1 - 0.5)^2 / 0.25 + 0 = 1, replicate (0 - 0.5)^2 / 0.25 + (2 - 1)^2 / 0.5 = 3
    assert last["chi"].tolist() == [[4.0, 1.0], [0.0, 3.0]]
    assert d["chi_ge"].tolist() == [0, 1] and d["chi_gt"].tolist() == [0, 1] and d["ppp_chi2_mid"].tolist() == [0.0, 1.0]
    assert d["chi2_obs_mean"].tolist() == [4.0, 1.0] and d["chi2_rep_mean"].tolist() == [0.0, 3.0]
    assert d["obs_rate"].tolist() == [[1.0, 1.0], [0.0, 0.5]] and d["rep_rate"].tolist() == [[0.5, 0.0], [0.5, 1.0]]
    assert (d["exp_rate"] == 0.5).all() and d["ppp_cell_mid"].tolist() == [[0.0, 0.0], [1.0, 1.0]]
    # Guttman: respondent 0 G_obs = 0, Q = 4, G_rep = 1, Q_rep = 4: 1 x 4 > 0 x 4; respondent 1 over its three cells: the data
    # (1 0 1) G_obs = 1 of Q = 2, the replicate (0 1 1) G_rep = 2 of Q_rep = 2: 2 x 2 > 1 x 2
    assert d["g_obs"].tolist() == [0, 1] and d["q_obs"].tolist() == [4, 2] and d["g_ge"].tolist() == [1, 1] and d["g_gt"].tolist() == [1, 1]
    assert d["group_lo"].tolist() == [0, 2] and d["group_hi"].tolist() == [1, 3] and d["group_items"].tolist() == [0, 1, 2, 3]
    assert (d["person_draws"], d["person_skipped"], d["K"], d["m"], d["n"]) == (1, 0, 2, 4, 2)
    assert d["group_items"].dtype == np.int32 and d["tN"].dtype == np.uint32 and d["sum_r"].dtype == np.uint64 and d["x_obs"].dtype == np.int64


def test_worst_ordering_ties_and_nan():
    w = P.person_worst([0.5, NAN, 0.25, 0.5, 0.25, NAN, 0.0], top=5)
    assert w["respondents"].tolist() == [6, 2, 4, 0, 3] and w["ppp_guttman_mid"].tolist() == [0.0, 0.25, 0.25, 0.5, 0.5]
    w = P.person_worst([NAN, 0.5, NAN], top=3)
    assert w["respondents"].tolist() == [1, -1, -1] and w["ppp_guttman_mid"][0] == 0.5 and np.isnan(w["ppp_guttman_mid"][1:]).all()
    with pytest.raises(ValueError, match="top must be"):
        P.person_worst(np.zeros(4), top=65)


def test_two_chains_equal_the_concatenated_draws_and_skipped_draws():
    rng = np.random.default_rng(8)
    n, m = 30, 11
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < 0.1] = NAN
    y[7] = NAN
    g = rng.normal(size=(5, n, m))
    rp = rng.random((5, n, m)) < 0.5
    order, cuts = P.default_item_order(y), (3, 7)
    whole = P.person_from_rep(y, g, rp, order, cuts)
    obs = P.person_observed(y, order, cuts)
    tabs = [P.person_tables(y, g[s], rp[s], obs) for s in (0, 1, 2)] + [P.person_tables(y, g[s], rp[s], obs) for s in (3, 4)]
    both = P.person_from_tables(tabs)
    for name, _dt, _kind in _lib.PERSON_RAW:
        assert np.array_equal(whole[name], both[name], equal_nan=True), name
    for name in _lib.PERSON_RESP_FIELDS + _lib.PERSON_CELL_FIELDS:
        assert np.array_equal(whole[name], both[name], equal_nan=True), name
    assert np.array_equal(whole["worst"]["respondents"], both["worst"]["respondents"])
    # the integers of two chains add up to the whole
    a, b = P.person_from_rep(y, g[:3], rp[:3], order, cuts), P.person_from_rep(y, g[3:], rp[3:], order, cuts)
    for name, dt, kind in _lib.PERSON_RAW:
        if dt != "f8" and (name, dt, kind) not in _lib.PERSON_CONST:
            assert np.array_equal(a[name] + b[name], whole[name]), name
    # a non-finite g in an observed cell skips the draw whole; a NaN in a missing cell is ignored
    g2 = g.copy()
    i, j = np.argwhere(~np.isnan(y))[0]
    g2[1, i, j] = np.inf
    g2[2, 7, 0] = NAN
    c = P.person_from_rep(y, g2, rp, order, cuts)
    e = P.person_from_rep(y, g[[0, 2, 3, 4]], rp[[0, 2, 3, 4]], order, cuts)
    assert (c["person_draws"], c["person_skipped"]) == (4, 1)
    for name, _dt, _kind in _lib.PERSON_RAW:
        assert np.array_equal(c[name], e[name], equal_nan=True), name
    # no draw at all: every mean is NaN, the constants stand
    z = P.person_from_rep(y, g[:0], rp[:0], order, cuts)
    assert z["person_draws"] == 0 and np.isnan(z["ppp_guttman"]).all() and np.isnan(z["ppp_cell"]).all()
    assert np.array_equal(z["guttman_obs"], whole["guttman_obs"], equal_nan=True) and z["worst"]["respondents"].tolist() == [-1] * 20


def test_default_order_and_cuts():
    # yes rates 2/4, 3/3, 1/2, no cell, 2/4: item 1 first, the ties 0, 2, 4 by index, the unobserved item last
    y = _pattern((1, 1, 1, None, 0), (1, 1, 0, None, 1), (0, 1, None, None, 1), (0, None, None, None, 0))
    assert P.default_item_order(y).tolist() == [1, 0, 2, 4, 3] and P.default_item_order(y).dtype == np.int32
    assert P.default_item_cuts(10) == (2, 4, 6, 8) and P.default_item_cuts(33, 5) == (6, 13, 19, 26)
    assert P.default_item_cuts(2, 5) == (1,) and P.default_item_cuts(3, 16) == (1, 2) and len(P.default_item_cuts(4096, 16)) == 15
    with pytest.raises(ValueError, match="groups must be"):
        P.default_item_cuts(10, 17)
    d = P.person_from_rep(y, np.zeros((0,) + y.shape), np.zeros((0,) + y.shape), top=2)
    assert d["cuts"].tolist() == [1, 2, 3, 4] and d["group_items"].tolist() == [1, 0, 2, 4, 3]


def test_refusals_say_what_is_wrong():
    o, c = P.check_person_args([2, 0, 1.0], [1, 2.0], 3)
    assert o.tolist() == [2, 0, 1] and o.dtype == np.int32 and c == (1, 2)
    ident = list(range(5))
    for order, cuts, m, word in ((ident, (2, 1), 5, "increasing"), (ident, (0, 2), 5, "increasing integers in 1..4"),
                                 (ident, (1, 5), 5, "increasing integers in 1..4"), (ident, (1.5,), 5, "integers"),
                                 (ident, (), 5, "1 item groups"), (list(range(40)), tuple(range(1, 17)), 40, "17 item groups"),
                                 ([0], (1,), 1, "outside 2..4096"), (ident, (1,), 4097, "outside 2..4096"),
                                 ([0, 1, 1, 3, 4], (1,), 5, "entry 2 is 1"), ([0, 1, 5, 3, 4], (1,), 5, "entry 2 is 5"),
                                 ([0, 1, -1, 3, 4], (1,), 5, "entry 2 is -1"), (ident[:4], (1,), 5, "must hold 5 integers"),
                                 ([0, 1, 2.5, 3, 4], (1,), 5, "must hold 5 integers")):
        with pytest.raises(ValueError, match=word):
            P.check_person_args(order, cuts, m)
    with pytest.raises(ValueError, match="beyond 65534"):
        P.check_person_args(ident, (1,), 5, n=65535)
    for top in (0, 65, 2.5):
        with pytest.raises(ValueError, match="top must be"):
            P.check_person_top(top)
    with pytest.raises(ValueError, match="unknown field 'no_such_field'"):
        P.person_field("no_such_field", 5, 3, 2)
    assert P.person_field("tE", 5, 3, 2) == ((2, 5), np.int64) and P.person_field("ppp_guttman", 5, 3, 2) == ((5,), np.float64)
    assert P.person_field("xr", 5, 3, 2) == ((5,), np.int64) and P.person_field("lz", 5, 3, 2) == ((3, 5), np.float64)
    assert P.person_field("order", 5, 3, 2) == ((3,), np.int32) and P.person_field("tR", 5, 3, 2) == ((2, 5), np.uint32)
    assert P.person_field("chi", 5, 3, 2) == ((2, 5), np.float64) and P.person_field("ppp_cell", 5, 3, 4) == ((4, 5), np.float64)


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


def test_c_abi_of_version_121():
    lib = _lib.load()
    assert lib.gpirt_version() >= 121
    names = ("gpirt_ppc_person_check", "gpirt_sampler_ppc_person_enable", "gpirt_sampler_ppc_person_get",
             "gpirt_sampler_ppc_person_state", "gpirt_ppc_person_combine")
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # _lib.PpcPerson mirrors the header's struct field for field: name, type and length
    ctype = {"int": C.c_int, "double*": C.POINTER(C.c_double), "void*": C.c_void_p, "int64_t*": C.POINTER(C.c_int64),
             "int32_t*": C.POINTER(C.c_int32), "int64_t": C.c_int64}
    fields = _header_struct("gpirt_ppc_person")
    assert [f[1] for f in fields] == [f[0] for f in _lib.PpcPerson._fields_]
    for (typ, nm, dim), (pn, pt) in zip(fields, _lib.PpcPerson._fields_):
        assert pt is (ctype[typ] if dim is None else ctype[typ] * dim), nm
    p = _lib.PpcPerson()
    assert C.sizeof(p) == 4 * 2 + 4 * 16 + 8 * (15 + 5) + 8 * 22 + 8 * 5 + 8 * 5 + 8 * 4
    assert len(_lib.PERSON_RAW) == 22 and _lib.PERSON_RAW[:5] == _lib.PERSON_CONST
    assert (len(_lib.PERSON_RESP_FIELDS), len(_lib.PERSON_CELL_FIELDS), len(_lib.PERSON_LAST)) == (15, 5, 8)
    # gpirt_run is still what tests/test_run_cpu.py fixes: 17 fields, 8 reserved slots -- the person fit is stage API only
    run = _header_struct("gpirt_run")
    assert len(run) == 17 == len(_lib.Run._fields_) and run[-1][1:] == ("reserved", 8)
    # the argument check alone: no device is touched
    c2 = (C.c_int * 2)
    o10 = (C.c_int32 * 10)
    good = o10(*range(10))
    assert lib.gpirt_ppc_person_check(100, 10, 3, o10(3, 1, 4, 0, 5, 9, 2, 6, 8, 7), c2(2, 5)) == 0
    rep = o10(0, 1, 2, 3, 4, 5, 2, 7, 8, 9)
    far = o10(0, 1, 2, 10, 4, 5, 6, 7, 8, 9)
    neg = o10(-1, 1, 2, 3, 4, 5, 6, 7, 8, 9)
    for n, m, K, order, cuts, word in ((65535, 10, 3, good, c2(2, 5), "beyond 65534"), (100, 1, 3, good, c2(2, 5), "outside 2..4096"),
                                       (100, 4097, 3, good, c2(2, 5), "outside 2..4096"), (100, 10, 1, good, c2(2, 5), "1 item groups"),
                                       (100, 10, 17, good, c2(2, 5), "17 item groups"), (100, 10, 3, good, c2(5, 2), "increasing"),
                                       (100, 10, 3, good, c2(2, 10), "increasing integers in 1..9"), (100, 10, 3, good, None, "item groups"),
                                       (100, 10, 3, None, c2(2, 5), "no item order"), (100, 10, 3, rep, c2(2, 5), "entry 6 is 2: a repeat"),
                                       (100, 10, 3, far, c2(2, 5), "entry 3 is 10: out of range"),
                                       (100, 10, 3, neg, c2(2, 5), "entry 0 is -1: out of range")):
        assert lib.gpirt_ppc_person_check(n, m, K, order, cuts) == _lib.E_ARG and word in _lib.last_error(), word
    # argument errors come back before any device is touched
    assert lib.gpirt_ppc_person_combine(None, 1, None, C.byref(p)) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_person_enable(None, 2, None, None, 1) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_person_get(None, b"counts", None, 0) == _lib.E_ARG
    _, arr = P.person_struct(5, 3, 2, top=4)
    assert arr["obs_rate"].shape == (2, 5) and arr["cell_ge"].dtype == np.uint32 and arr["worst_respondents"].shape == (4,)
    assert arr["x_obs"].shape == (5,) and arr["group_items"].shape == (3,) and arr["sum_r"].dtype == np.uint64
