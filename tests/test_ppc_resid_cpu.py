"""The NumPy statement of the PPC's residual correlations (gpirt_amd.ppc.resid_*; include/gpirt_hip.h, "residual correlations in
the PPC") alone, without a GPU: the integer tables against a plain Python-integer triple loop, the digit split the device's int8
planes use, the invariances of the definition, and that the block sees what it is for -- a fitting model passes, a planted
near-duplicate pair heads the list while every margin of the plain PPC stays unremarkable, a second dimension fails the global
test."""
import numpy as np
import pytest

from gpirt_amd import ppc as P

U = 2 ** 22


def _case(n, m, seed, S=3, na=0.1):
    rng = np.random.default_rng(seed)
    y = np.where(rng.random((n, m)) < 0.5, 1.0, -1.0)
    y[rng.random((n, m)) < na] = np.nan
    g = 1.5 * rng.standard_normal((S, n, m))
    rep = rng.random((S, n, m)) < 0.5
    return y, g, rep


@pytest.mark.parametrize("n,m", [(7, 3), (40, 5)])
def test_tables_against_python_integers(n, m):
    y, g, rep = _case(n, m, seed=n)
    y[0, 0], y[1, 1] = 1.0, np.nan                              # (at least one of each)
    O = (~np.isnan(y)).astype(np.int64)
    for s in range(g.shape[0]):
        do, dr, w = P.resid_terms(y, g[s], rep[s])
        assert not do[O == 0].any() and not dr[O == 0].any() and not w[O == 0].any()
        assert np.abs(do).max() <= U and np.abs(dr).max() <= U and 0 <= w.min() and w.max() <= U // 4
        # the terms themselves, cell by cell in Python floats
        for i in range(n):
            for j in range(m):
                if O[i, j]:
                    p, q = 1.0 / (1.0 + np.exp(-g[s, i, j])), 1.0 / (1.0 + np.exp(g[s, i, j]))
                    assert abs(int(do[i, j]) - (q if y[i, j] > 0 else -p) * U) <= 0.5 + 1e-6
                    assert abs(int(dr[i, j]) - (q if rep[s, i, j] else -p) * U) <= 0.5 + 1e-6
                    assert abs(int(w[i, j]) - p * q * U) <= 0.5 + 1e-6
        t = P.resid_tables(do, dr, w, O)
        for a in range(m):
            for b in range(m):
                so = sr = v = 0
                for i in range(n):
                    so += int(do[i, a]) * int(do[i, b])
                    sr += int(dr[i, a]) * int(dr[i, b])
                    v += int(w[i, a]) * int(O[i, b])
                assert (int(t["s_obs"][a, b]), int(t["s_rep"][a, b]), int(t["v"][a, b])) == (so, sr, v), (a, b)
        assert t["s_obs"].dtype == np.int64 and np.array_equal(t["s_obs"], t["s_obs"].T) and np.array_equal(t["s_rep"], t["s_rep"].T)


def test_digit_split_and_rejoin():
    edges = [0, 127, 128, 129, 32767, 32768, U]
    x = np.array(sorted(set(edges + [-e for e in edges] + [1, -1, 255, 256, -255, -256, 32639, 32640, -32896, -32897, U - 1, 1 - U])))
    d0, d1, d2 = P.resid_digits(x)
    assert np.array_equal(P.resid_join(d0, d1, d2), x)
    assert d0.min() >= -128 and d0.max() <= 127 and d1.min() >= -128 and d1.max() <= 127 and np.abs(d2).max() <= 64
    assert d2[-1] == 64 and d2[0] == -64
    # ... and over the whole range
    x = np.arange(-U, U + 1)
    d0, d1, d2 = P.resid_digits(x)
    assert np.array_equal(P.resid_join(d0, d1, d2), x)
    assert (d0.min(), d0.max(), d1.min(), d1.max(), d2.min(), d2.max()) == (-128, 127, -128, 127, -64, 64)
    for d in (d0, d1, d2):
        assert np.array_equal(d.astype(np.int8), d)


def test_infinite_g_and_unobserved_nan():
    y = np.array([[1.0, -1.0, np.nan], [-1.0, 1.0, 1.0]])
    g = np.array([[np.inf, -np.inf, np.nan], [40.0, -40.0, 0.0]])
    do, dr, w = P.resid_terms(y, g, np.array([[1, 0, 1], [0, 1, 0]]))
    assert do.tolist() == [[0, 0, 0], [-U, U, U // 2]]
    assert dr.tolist() == [[0, 0, 0], [-U, U, -U // 2]]
    assert w.tolist() == [[0, 0, 0], [0, 0, U // 4]]


def test_invariances():
    n, m, S = 60, 6, 4
    y, g, rep = _case(n, m, seed=5, S=S, na=0.05)
    y[: n // 2, 0] = np.nan
    y[n // 2:, 1] = np.nan                                       # the pair (0, 1) has no co-observed respondent
    g[:, :, 4] = np.where(y[:, 4] > 0, 50.0, -50.0)[None]        # item 4: p = 0 or 1 everywhere
    base = P.resid_from_rep(y, g, rep, top=5)
    O = ~np.isnan(y)
    assert base["n_co"][0, 1] == 0
    for k in ("rc_obs_mean", "rc_rep_mean", "rc_rep_sd", "ppp_rc", "ppp_rc_mid", "undefined"):
        assert np.isnan(base[k][0, 1]) and np.isnan(base[k][1, 0]) and np.isnan(np.diag(base[k])).all(), k
    # item 4: V = 0 in every draw, so its pairs and its infit are undefined in every draw
    for s in range(S):
        t = P.resid_tables(*P.resid_terms(y, g[s], rep[s]), O.astype(np.int64))
        assert not t["v"][4].any() and t["v"][:, 4].any()
    live4 = base["n_co"][4] > 0
    assert np.array_equal(base["undefined_count"][4][live4], np.full(live4.sum(), S, dtype=np.uint32))
    assert np.isnan(base["rc_obs_mean"][4]).all() and np.isnan(base["infit_obs_mean"][4]) and np.isnan(base["ss_obs_mean"][4])
    assert base["ss_undefined"][4] == S and base["ss_undefined"][2] == 0 and base["global_undefined"] == 0
    assert (base["worst"]["pairs"] != 4).all()
    # respondents permuted: the integer tables, hence everything, unchanged
    perm = np.random.default_rng(1).permutation(n)
    for s in range(S):
        t0 = P.resid_tables(*P.resid_terms(y, g[s], rep[s]), O.astype(np.int64))
        t1 = P.resid_tables(*P.resid_terms(y[perm], g[s][perm], rep[s][perm]), O[perm].astype(np.int64))
        for k in t0:
            assert np.array_equal(t0[k], t1[k]), k
    again = P.resid_from_rep(y[perm], g[:, perm], rep[:, perm], top=5)
    for k in P._lib.RESID_PAIR_FIELDS + P._lib.RESID_ITEM_FIELDS + tuple(nm for nm, _, _ in P._lib.RESID_RAW):
        assert np.array_equal(again[k], base[k], equal_nan=True), k
    # items permuted: the pair arrays are permuted bit for bit; the sums over items change only in the order of their additions
    ip = np.array([3, 0, 5, 1, 4, 2])
    moved = P.resid_from_rep(y[:, ip], g[:, :, ip], rep[:, :, ip], top=5)
    for k in P._lib.RESID_PAIR_FIELDS:
        assert np.array_equal(moved[k], base[k][np.ix_(ip, ip)], equal_nan=True), k
    for k in ("infit_obs_mean", "infit_rep_mean", "infit_rep_sd", "ppp_infit", "ppp_infit_mid", "ppp_ss", "ppp_ss_mid"):
        assert np.array_equal(moved[k], base[k][ip], equal_nan=True), k
    for k in ("ss_obs_mean", "ss_rep_mean"):
        assert np.allclose(moved[k], base[k][ip], rtol=1e-12, atol=0, equal_nan=True), k
    for k in ("frob_obs_mean", "frob_rep_mean", "frob_rep_sd"):
        assert np.isclose(moved[k], base[k], rtol=1e-12, atol=0), k
    for k in ("max_obs_mean", "absmax_rep_mean", "ppp_frob", "ppp_max_mid", "ppp_absmax"):
        assert moved[k] == base[k], k


def test_lane_sum_is_a_sum_in_a_fixed_order():
    rng = np.random.default_rng(2)
    for L in (1, 63, 64, 65, 200):
        x = rng.random((3, L))
        want = []
        for row in x:
            lanes = [0.0] * 64
            for b, v in enumerate(row):
                lanes[b % 64] = lanes[b % 64] + v if b >= 64 else v
            tot = lanes[0]
            for v in lanes[1:]:
                tot = tot + v
            want.append(tot)
        assert np.array_equal(P.resid_lane_sum(x), np.array(want))


def test_skipped_draws_and_chains():
    n, m, S = 50, 5, 6
    y, g, rep = _case(n, m, seed=9, S=S, na=0.05)
    whole = P.resid_from_rep(y, g, rep)
    g2 = g.copy()
    obs = np.argwhere(~np.isnan(y))[3]
    g2[2, obs[0], obs[1]] = np.nan
    cut = P.resid_from_rep(y, g2, rep)
    keep = [0, 1, 3, 4, 5]
    assert (cut["resid_draws"], cut["resid_skipped"], whole["resid_skipped"]) == (S - 1, 1, 0)
    ref = P.resid_from_rep(y, g[keep], rep[keep])
    assert np.array_equal(cut["rc_obs_sum"], ref["rc_obs_sum"]) and np.array_equal(cut["global"], ref["global"])
    # a NaN in an unobserved cell changes nothing
    g3 = g.copy()
    hole = np.argwhere(np.isnan(y))[0]
    g3[:, hole[0], hole[1]] = np.nan
    same = P.resid_from_rep(y, g3, rep)
    for k, _, _ in P._lib.RESID_RAW:
        assert np.array_equal(same[k], whole[k]), k
    # two chains pooled: the integers are the whole's, the double sums the two chains' sums added
    O = (~np.isnan(y)).astype(np.int64)
    tabs = [P.resid_tables(*P.resid_terms(y, g[s], rep[s]), O) for s in range(S)]
    pooled = P.resid_from_tables(tabs, O.T @ O, chains=[2, 4], n=n)
    a, b = P.resid_from_tables(tabs[:2], O.T @ O), P.resid_from_tables(tabs[2:], O.T @ O)
    assert np.array_equal(pooled["rc_ge"], whole["rc_ge"]) and np.array_equal(pooled["rc_ge"], a["rc_ge"] + b["rc_ge"])
    assert np.array_equal(pooled["rc_rep_sum"], a["rc_rep_sum"] + b["rc_rep_sum"])
    assert np.allclose(pooled["rc_rep_sum"], whole["rc_rep_sum"], rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError):
        P.resid_from_rep(y, g, rep, top=65)


def _world(kind, seed=26, n=400, m=10, S=100):
    """theta ~ N(0, 1), ten Rasch items, draws g = the generating curve + N(0, 0.05^2) noise; "dup": item 1 copies item 0's
    answers with 10 % flips (both have difficulty 0, so its margin stays the model's); "dim": a second latent dimension on the
    upper half of the items that the curves know nothing of"""
    rng = np.random.default_rng(seed)
    th = rng.standard_normal(n)
    b = np.linspace(-1.2, 1.2, m)
    b[0] = b[1] = 0.0
    g0 = th[:, None] - b[None, :]
    gt = g0.copy()
    if kind == "dim":
        gt[:, m // 2:] += 1.5 * rng.standard_normal(n)[:, None]
    y = np.where(rng.random((n, m)) < 1.0 / (1.0 + np.exp(-gt)), 1.0, -1.0)
    if kind == "dup":
        y[:, 1] = np.where(rng.random(n) < 0.10, -y[:, 0], y[:, 0])
    y[rng.random((n, m)) < 0.03] = np.nan
    return y, g0[None] + 0.05 * rng.standard_normal((S, n, m)), range(1, S + 1)


def test_a_fitting_model_passes():
    y, g, iters = _world("model")
    r, gap = P.resid_from_draws(y, g, 11, iters)
    print(f"MEASURED ppp_frob_mid {r['ppp_frob_mid']:.3f} ppp_max_mid {r['ppp_max_mid']:.3f} min|u - p| {gap:.1e}")
    assert 0.05 <= r["ppp_frob_mid"] <= 0.95
    assert r["resid_draws"] == 100 and r["global_undefined"] == 0 and not r["undefined_count"].any()
    assert np.allclose(r["infit_rep_mean"], 1.0, atol=0.05)


def test_a_near_duplicate_pair_heads_the_list_with_quiet_margins():
    y, g, iters = _world("dup")
    S = len(iters)
    r, _ = P.resid_from_draws(y, g, 11, iters, top=3)
    plain = P.from_draws(y, g, 11, iters)
    assert plain["undecided"]["cells"] == 0
    mid = (plain["item"]["yes_ge"][0] + plain["item"]["yes_gt"][0]) / (2.0 * S)
    print(f"MEASURED worst {r['worst']['pairs'][0]} ppp_rc_mid {r['worst']['ppp_rc_mid'][0]:.3f} rc_obs_mean "
          f"{r['worst']['rc_obs_mean'][0]:.3f} margins in [{mid.min():.3f}, {mid.max():.3f}]")
    assert r["worst"]["pairs"][0].tolist() == [0, 1] and r["worst"]["ppp_rc_mid"][0] <= 0.02
    assert r["worst"]["rc_obs_mean"][0] > 0.5
    assert (mid >= 0.05).all() and (mid <= 0.95).all()
    assert set(r["worst_items"]["items"][:2].tolist()) == {0, 1}
    c = P.resid_contrasts(r, k=2)
    assert c["dropped"].size == 0 and c["values"][0] > 1.5 and set(np.argsort(-np.abs(c["vectors"][:, 0]))[:2].tolist()) == {0, 1}


def test_a_second_dimension_fails_the_global_test():
    y, g, iters = _world("dim")
    r, _ = P.resid_from_draws(y, g, 11, iters)
    print(f"MEASURED ppp_frob_mid {r['ppp_frob_mid']:.3f} frob_obs_mean {r['frob_obs_mean']:.3f} frob_rep_mean {r['frob_rep_mean']:.3f}")
    assert r["ppp_frob_mid"] <= 0.02


def test_contrasts_drop_items_with_nan_rows():
    y, g, iters = _world("model", S=5)
    y[:, 3] = np.nan
    r, _ = P.resid_from_draws(y, g, 11, iters)
    c = P.resid_contrasts(r, k=20)
    assert c["dropped"].tolist() == [3] and c["items"].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9]
    assert c["values"].shape == (9,) and c["vectors"].shape == (9, 9) and (np.diff(c["values"]) <= 0).all()
    assert "NO p-value" in P.resid_contrasts.__doc__


def _header_struct(name):
    """the (type, field, array length or None) triples of a struct of the header, in order"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpirt_hip.h")).read()
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
    return out, defs


def test_c_abi_of_version_123():
    import ctypes as C
    from gpirt_amd import _lib
    lib = _lib.load()
    assert lib.gpirt_version() >= 123
    for name in ("gpirt_sampler_ppc_resid_enable", "gpirt_sampler_ppc_resid_get", "gpirt_sampler_ppc_resid_state", "gpirt_ppc_resid_combine"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    # _lib.PpcResid mirrors the header's struct field for field: name, type and length; the field names follow the indices
    ctype = {"int": C.c_int, "double*": C.POINTER(C.c_double), "void*": C.c_void_p, "int64_t*": C.POINTER(C.c_int64),
             "int64_t": C.c_int64, "double": C.c_double}
    fields, defs = _header_struct("gpirt_ppc_resid")
    assert [f[1] for f in fields] == [f[0] for f in _lib.PpcResid._fields_]
    for (typ, nm, dim), (pn, pt) in zip(fields, _lib.PpcResid._fields_):
        assert pt is (ctype[typ] if dim is None else ctype[typ] * dim), nm
    for prefix, names in (("P", _lib.RESID_PAIR_FIELDS), ("I", _lib.RESID_ITEM_FIELDS), ("S", _lib.RESID_SCALARS)):
        for k, nm in enumerate(names):
            assert int(defs[f"GPIRT_RESID_{prefix}_{nm.upper()}"]) == k, nm
    assert (int(defs["GPIRT_RESID_NPAIR"]), int(defs["GPIRT_RESID_NITEM"]), int(defs["GPIRT_RESID_NSCALAR"]), int(defs["GPIRT_RESID_NRAW"])) == \
        (len(_lib.RESID_PAIR_FIELDS), len(_lib.RESID_ITEM_FIELDS), len(_lib.RESID_SCALARS), len(_lib.RESID_RAW)) == (7, 9, 13, 13)
    assert (int(defs["GPIRT_RESID_MAX_N"]), int(defs["GPIRT_RESID_MAX_M"]), int(defs["GPIRT_RESID_MAX_TOP"])) == \
        (_lib.RESID_MAX_N, _lib.RESID_MAX_M, _lib.RESID_MAX_TOP) == (65534, 4096, 64)
    # gpirt_run is still what tests/test_run_cpu.py fixes: the block is stage API only
    run, _ = _header_struct("gpirt_run")
    assert len(run) == len(_lib.Run._fields_) and "resid" not in [f[1] for f in run]
    # argument errors come back before any device is touched
    p, arr = P.resid_struct(5, top=4)
    assert lib.gpirt_ppc_resid_combine(None, 1, None, C.byref(p)) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_resid_enable(None, 20) == _lib.E_ARG
    assert lib.gpirt_sampler_ppc_resid_get(None, b"counts", None, 0) == _lib.E_ARG
    assert arr["ppp_rc"].shape == (5, 5) and arr["rc_ge"].dtype == np.uint32 and arr["n_co_int"].dtype == np.int64
    assert arr["global"].shape == (16,) and arr["worst_pairs"].shape == (4, 2) and arr["worst_items"].shape == (4,)
    assert P.resid_field("d_obs", 7, 5) == ((7, 5), np.int32, "F") and P.resid_field("digits", 7, 5) == ((9, 5, 7), np.int8, "C")
    assert P.resid_field("stats", 7, 5) == ((8,), np.float64, "C") and P.resid_field("ss_ge", 7, 5) == ((5,), np.uint32, "C")
