"""gpirt_amd.score.predict_from_draws -- the NumPy statement of "predicting new respondents' unseen answers"
(include/gpirt_hip.h) -- on inputs whose answer is known, the bounds of tests/_predict_bounds.py at the GPU tests' shapes,
and the C ABI of library version 110 on a machine without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from gpirt_amd import score as SC
from gpirt_amd.synthetic import make_responses

from _predict_bounds import compare, delta_from
from _score_bounds import EPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1001
NEW = ("gpirt_sampler_score_predict_enable", "gpirt_sampler_score_predict_get", "gpirt_sampler_score_predict_state",
       "gpirt_score_predict_combine", "gpirt_mcmc_run")


def _fstar(S, m, seed=3):
    """smooth item response functions on the grid plus a little noise per draw: (S, 1001, m)"""
    rng = np.random.default_rng(seed)
    th = SC.grid()
    a, b = rng.uniform(0.3, 2.0, m) * rng.choice([-1.0, 1.0], m), rng.normal(0.0, 1.0, m)
    return a * th[:, None] + b + 0.1 * rng.standard_normal((S, N, m))


def _y_new(n_new, m, seed=11):
    """about 30 % NaN, then (from three respondents on) one who answered nothing and one who answered everything"""
    y, _ = make_responses(n_new + 2, m, seed=seed, na_frac=0.3)
    full = np.array(y[n_new])
    full[np.isnan(full)] = 1.0
    y = np.array(y[:n_new])
    if n_new >= 3:
        y[-1, :] = np.nan
        y[-2, :] = full
    return y


def test_zero_fstar_gives_one_half_no_information_and_the_lowest_items():
    y = _y_new(9, 17)
    out = SC.predict_from_draws(y, np.zeros((3, N, 17)), top=4)
    gap_p, gap_i = np.abs(out["p_yes"] - 0.5).max(), np.abs(out["info"]).max()
    print(f"MEASURED zero f*: p_yes gap {gap_p:.3e}, info gap {gap_i:.3e}; draws {out['pred_draws']}")
    assert out["pred_draws"] == 3 and out["pred_skipped"] == 0
    assert gap_p <= 4 * EPS and gap_i <= 8 * EPS
    for r in range(9):                                   # every column is the same: the ties go to the lowest j
        un = np.flatnonzero(np.isnan(y[r]))[:4]
        assert np.array_equal(out["next_items"][r, :un.size], un) and (out["next_items"][r, un.size:] == -1).all()
    assert np.array_equal(np.isnan(out["next_info"]), out["next_items"] == -1)


def test_a_saturated_column_has_no_entropy_and_predicts_the_mass_above():
    m = 6
    y = _y_new(8, m, seed=5)
    f = _fstar(2, m)
    f[:, :, 2] = np.where(np.arange(N) >= 500, 800.0, -800.0)
    f[:, :, 4] = np.where(np.arange(N) >= 300, np.inf, -np.inf)
    P, H = SC.plogis_entropy(f[0])
    assert (H[:, 2] == 0).all() and (H[:, 4] == 0).all() and set(np.unique(P[:, [2, 4]])) == {0.0, 1.0}
    out = SC.predict_from_draws(y, f, return_draws=True)
    for d in range(2):
        w, q, hbar = out["weights"][0][d], out["q"][0][d], out["Hbar"][0][d]
        assert (hbar[:, [2, 4]] == 0).all()
        assert np.allclose(q[:, 2], w[500:].sum(axis=0), rtol=N * EPS, atol=1e-300)
        assert np.allclose(q[:, 4], w[300:].sum(axis=0), rtol=N * EPS, atol=1e-300)
    mass = np.mean([w[500:].sum(axis=0) for w in out["weights"][0]], axis=0)
    assert np.allclose(out["p_yes"][:, 2], mass, rtol=2 * N * EPS, atol=1e-300)
    # no residual entropy: the information of such an item is the whole entropy of the prediction
    want = np.mean([SC.binary_entropy(q[:, 2]) for q in out["q"][0]], axis=0)
    assert np.allclose(out["info"][:, 2], want, rtol=0, atol=8 * EPS)


def test_entropy_is_symmetric_log2_at_zero_and_zero_in_the_tails():
    f = np.array([0.0, 1.5, -1.5, 30.0, -30.0, 745.0, -746.0, np.inf, -np.inf])
    P, H = SC.plogis_entropy(f)
    assert H[0] == np.log1p(1.0) and P[0] == 0.5 and H[1] == H[2] and H[3] == H[4] and H[3] > 0
    assert H[6] == 0 and H[7] == 0 and H[8] == 0 and P[7] == 1 and P[8] == 0 and P[6] == 0
    assert np.allclose(P[1] + P[2], 1.0, rtol=2 * EPS)
    exact = -(P[1] * np.log(P[1]) + P[2] * np.log(P[2]))
    assert abs(H[1] - exact) <= 8 * EPS
    assert np.array_equal(SC.binary_entropy([0.0, 1.0, -1e-3, 1.0 + 1e-9, 0.5]), [0.0, 0.0, 0.0, 0.0, np.log(2.0)])


def test_no_answers_means_the_prior_weighted_mean():
    m = 5
    y = _y_new(6, m)
    f = _fstar(3, m, seed=9)
    out = SC.predict_from_draws(y, f, return_draws=True)
    prior = np.exp(SC.logprior() - SC.logprior_lse())
    assert np.isnan(y[-1]).all()
    for d in range(3):
        P, H = SC.plogis_entropy(f[d])
        assert np.allclose(out["q"][0][d][-1], prior @ P, rtol=4 * N * EPS, atol=0)
        assert np.allclose(out["Hbar"][0][d][-1], prior @ H, rtol=4 * N * EPS, atol=0)
    assert (out["info"] > -8 * EPS).all() and (out["info"] <= np.log(2.0)).all()
    assert (out["p_yes"] > 0).all() and (out["p_yes"] < 1).all()


def test_a_nan_cell_skips_the_whole_draw():
    m = 4
    y = _y_new(5, m)
    f = _fstar(3, m, seed=2)
    bad = f.copy()
    bad[1, 321, 3] = np.nan
    got, want = SC.predict_from_draws(y, bad), SC.predict_from_draws(y, f[[0, 2]])
    assert got["pred_skipped"] == 1 and got["pred_draws"] == 2 and want["pred_skipped"] == 0
    for k in ("pred_sum", "info_sum", "p_yes", "info", "next_items"):
        assert np.array_equal(got[k], want[k]), k
    none = SC.predict_from_draws(y, bad[1:2])
    assert none["pred_draws"] == 0 and np.isnan(none["p_yes"]).all() and np.isnan(none["info"]).all()
    assert (none["next_items"] == -1).all() and np.isnan(none["next_info"]).all()


def test_who_answered_everything_is_asked_nothing_and_chains_add():
    m = 7
    y = _y_new(6, m)
    f = _fstar(4, m, seed=4)
    out = SC.predict_from_draws(y, f, top=16)
    assert not np.isnan(y[-2]).any() and (out["next_items"][-2] == -1).all() and np.isnan(out["next_info"][-2]).all()
    assert np.array_equal(np.sort(out["next_items"][-1][:m]), np.arange(m)) and (out["next_items"][-1][m:] == -1).all()
    assert (np.diff(out["next_info"][-1][:m]) <= 0).all()
    for r in range(6):                                   # answered items are never listed, whatever their information
        listed = out["next_items"][r][out["next_items"][r] >= 0]
        assert np.isnan(y[r, listed]).all() and listed.size == min(16, int(np.isnan(y[r]).sum()))
    two = SC.predict_from_draws(y, f.reshape(2, 2, N, m))
    a, b = SC.predict_from_draws(y, f[:2]), SC.predict_from_draws(y, f[2:])
    assert np.array_equal(two["pred_sum"], a["pred_sum"] + b["pred_sum"]) and two["pred_draws"] == 4
    assert np.array_equal(two["info_sum"], a["info_sum"] + b["info_sum"])


def test_top_outside_1_to_16_raises():
    y, f = _y_new(3, 4), _fstar(1, 4)
    for top in (0, 17, -1, 2.5):
        with pytest.raises(ValueError, match="outside 1..16"):
            SC.predict_from_draws(y, f, top=top)
    assert SC.predict_from_draws(y, f, top=1)["next_items"].shape == (3, 1)
    assert SC.predict_from_draws(y, f, top=16)["next_items"].shape == (3, 16)


@pytest.mark.parametrize("m,n_new", [(17, 1), (3, 65), (33, 63), (65, 257)])
def test_bounds_leave_no_respondent_out_at_the_gpu_shapes(m, n_new):
    """The reference against itself at the GPU tests' (m, n_new) on smooth synthetic f*: the compared ranks of every
    respondent are further apart than twice the info bound, so the 1 % cap of the GPU comparison is not what passes it."""
    y = _y_new(n_new, m, seed=7 + n_new)
    want = SC.predict_from_draws(y, _fstar(4, m, seed=m), return_draws=True)
    share = compare(want, want, delta_from(want, m), y, f"self m={m} n_new={n_new}")
    assert share == 0.0


def test_abi_of_version_110():
    from gpirt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    assert lib.gpirt_version() >= 110
    hdr = open(os.path.join(ROOT, "include", "gpirt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define GPIRT_PREDICT_MAX_TOP\s+%d\b" % _lib.PREDICT_MAX_TOP, hdr)
    assert _lib.Run.predict.offset == _lib.Run.score.offset + 8          # gpirt_run: predict follows score


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_predict_struct_layout_matches_the_header():
    from gpirt_amd import _lib
    fields = [f[0] for f in _lib.ScorePredict._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gpirt_hip.h\"\nint main(void){printf(\"%zu\\n\", sizeof(gpirt_score_predict));"
    src += "".join('printf("%%zu\\n", offsetof(gpirt_score_predict, %s));' % f for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got[0] == C.sizeof(_lib.ScorePredict)
    assert got[1:] == [getattr(_lib.ScorePredict, f).offset for f in fields]
