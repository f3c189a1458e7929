"""Several chains and their diagnostics (include/gpirt_hip.h GPIRT_SUM_DIAG, gpirt_chains_combine, gpirt_mcmc_chains) on a
machine without a GPU: the entry points are exported and bound, gpirt_diag's layout is the header's, gpirt_chain_seed equals
its Python mirror, the argument checks, and the NumPy reference of split-R-hat / ESS / MCSE on cases with known answers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpirt_chain_seed", "gpirt_sampler_summary_enable_planned", "gpirt_summary_state_bytes", "gpirt_sampler_summary_state",
       "gpirt_chains_combine", "gpirt_mcmc_chains")


@pytest.fixture(scope="module")
def lib():
    from gpirt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_chain_symbols_are_exported_and_bound(lib):
    from gpirt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpirt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.gpirt_version() >= 105
    assert re.search(r"#define GPIRT_SUM_DIAG\s+%d\b" % _lib.SUM_DIAG, hdr)
    for i, b in enumerate(_lib.DIAG_BLOCKS):
        assert re.search(r"#define GPIRT_DIAG_%s\s+%d\b" % (b.upper(), i), hdr), b
    for i, k in enumerate(_lib.DIAG_SCALARS):
        assert re.search(r"#define GPIRT_DIAG_%s\s+%d\b" % (k.upper(), i), hdr), k
    for k, v in (("GAMMA", _lib.CHAIN_SEED_GAMMA), ("M1", _lib.CHAIN_SEED_M1), ("M2", _lib.CHAIN_SEED_M2)):
        assert re.search(r"#define GPIRT_CHAIN_SEED_%s\s+0x%XULL" % (k, v), hdr), k


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_diag_struct_layout_matches_the_header():
    from gpirt_amd import _lib
    fields = [f[0] for f in _lib.Diag._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gpirt_hip.h\"\nint main(void){printf(\"%zu\\n\", sizeof(gpirt_diag));"
    src += "".join('printf("%%zu\\n", offsetof(gpirt_diag, %s));' % f for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as fh:
            fh.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got[0] == C.sizeof(_lib.Diag)
    assert got[1:] == [getattr(_lib.Diag, f).offset for f in fields]


def test_chain_seed_c_equals_python(lib):
    from gpirt_amd import _lib
    for seed in (0, 1, 29, 12345, 2 ** 32 + 7, 2 ** 64 - 1):
        assert lib.gpirt_chain_seed(seed, 0) == seed == _lib.chain_seed(seed, 0)
        for c in (1, 2, 3, 17, 1000):
            assert lib.gpirt_chain_seed(seed, c) == _lib.chain_seed(seed, c), (seed, c)
    assert _lib.chain_seed(0, 1) == 0xE220A8397B1DCDAF          # the first output of splitmix64 from state 0
    assert len({_lib.chain_seed(7, c) for c in range(64)}) == 64


def test_chain_argument_errors(lib):
    from gpirt_amd import _lib
    dp = C.POINTER(C.c_double)
    n, m, nc = 4, 2, 2
    y = np.ones((n, m), order="F")
    th = np.zeros((nc, n))
    p = np.full((2, m), 0.1, order="F")
    irf = np.zeros((1001, m), order="F")
    sm = _lib.Summary()
    sm.parts = _lib.SUM_WAIC

    def call(o, parts=None, **kw):
        sm.parts = _lib.SUM_WAIC if parts is None else parts
        d = _lib.Diag()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.gpirt_mcmc_chains(y.ctypes.data_as(dp), n, m, th.ctypes.data_as(dp), nc, 4, 1, p.ctypes.data_as(dp),
                                     p.ctypes.data_as(dp), p.ctypes.data_as(dp), C.byref(o), 1, _lib.TICK_FN(0), None, None,
                                     None, None, irf.ctypes.data_as(dp), C.byref(sm), C.byref(d))

    o = _lib.default_options()                         # GPIRT_RNG_RSTREAM: refused
    assert call(o) == _lib.E_ARG and "GPIRT_RNG_ITEM" in _lib.last_error()
    o.rng_kind = _lib.RNG_ITEM
    assert call(o, parts=_lib.SUM_DIAG) == _lib.E_ARG   # the pooled summary takes the four parts only
    f = np.zeros((n, m))
    assert call(o, h_f_rhat=f.ctypes.data_as(dp)) == _lib.E_ARG    # f's diagnostics need GPIRT_SUM_F
    r = (C.c_int64 * 4)(1, 0, 0, 0)
    assert call(o, reserved=r) == _lib.E_ARG
    import torch
    if not torch.cuda.is_available():
        assert call(o) == _lib.E_NODEVICE
    # the stage entries
    b = C.c_int64()
    assert lib.gpirt_sampler_summary_enable_planned(None, _lib.SUM_DIAG, 4) == _lib.E_ARG
    assert lib.gpirt_sampler_summary_state(None, C.byref(C.c_void_p()), C.byref(b)) == _lib.E_ARG
    assert lib.gpirt_chains_combine(None, 2, None, None, 1, None, None, None) == _lib.E_ARG
    assert lib.gpirt_summary_state_bytes(10, 3, 64, C.byref(b)) == _lib.E_ARG
    assert lib.gpirt_summary_state_bytes(10, 3, _lib.SUM_WAIC | _lib.SUM_F | _lib.SUM_DIAG, C.byref(b)) == 0
    big = b.value
    assert lib.gpirt_summary_state_bytes(10, 3, _lib.SUM_WAIC | _lib.SUM_F, C.byref(b)) == 0
    assert b.value % 16 == 0 and big % 16 == 0
    # the DIAG accumulators: 7 more arrays of theta / beta (16 values) and of f (30 cells), each padded to an even count
    assert big - b.value == 8 * 7 * (16 + 30)


def test_numpy_reference_iid_normals():
    from gpirt_amd.chains import diagnostics_from_draws
    rng = np.random.default_rng(1)
    C_, S = 4, 2500
    x = rng.standard_normal((C_, S, 300))
    d = diagnostics_from_draws(x)
    assert np.abs(d["rhat"] - 1.0).max() < 0.01
    ess = d["ess"] / (C_ * S)
    assert 0.7 < ess.mean() < 1.3 and ess.min() > 0.4
    assert np.allclose(d["mcse"], np.sqrt(1.0 / (C_ * S)), rtol=0.35)


def test_numpy_reference_flags_chains_that_disagree():
    from gpirt_amd.chains import diagnostics_from_draws
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 400, 10))
    x[1] += 3.0
    assert (diagnostics_from_draws(x)["rhat"] > 1.5).all()
    # a mirror mode: reflecting chain 1 by its sign brings R-hat back
    y = rng.standard_normal((2, 400, 10)) + 3.0
    y[1] *= -1.0
    assert (diagnostics_from_draws(y)["rhat"] > 1.5).all()
    assert (diagnostics_from_draws(y, signs=[1, -1])["rhat"] < 1.05).all()


def test_numpy_reference_edges():
    from gpirt_amd.chains import diagnostics_from_draws
    rng = np.random.default_rng(3)
    for S in (1, 2, 3):                            # S < 4: R-hat NaN
        d = diagnostics_from_draws(rng.standard_normal((2, S, 3)))
        assert np.isnan(d["rhat"]).all()
        if S == 1:                                 # one batch: no ESS
            assert np.isnan(d["ess"]).all() and np.isnan(d["mcse"]).all()
        else:
            assert np.isfinite(d["ess"]).all()
    # S odd: the middle draw enters neither half -- changing it moves no half statistic, so R-hat's W and B stay put
    x = rng.standard_normal((2, 7, 3))
    z = x.copy()
    z[:, 3] += 100.0
    a, b = diagnostics_from_draws(x), diagnostics_from_draws(z)
    assert np.allclose(a["rhat"], b["rhat"], rtol=0, atol=1e-14)
    # W = 0: +inf when the half means differ, NaN when they do not
    c = np.zeros((2, 8, 2))
    c[1, :, 0] = 1.0
    r = diagnostics_from_draws(c)["rhat"]
    assert np.isposinf(r[0]) and np.isnan(r[1])


def test_numpy_reference_hand_worked_two_chains_s9():
    """Chain A = 1..9, chain B = 0 2 0 2 1 2 0 2 0.  Halves of N = 4 (the 5th draw in neither): A 2.5 / 7.5 (s^2 = 5/3),
    B 1 / 1 (s^2 = 4/3); xbar = 3, B = 4/3 x 28.5 = 38, W = 1.5, var+ = 0.75 x 1.5 + 38 / 4 = 10.625, R-hat = sqrt(10.625 /
    1.5).  Batches b = 3, a = 3: A's means 2 5 8 (sigma^2 = 3/2 x 18 = 27, lambda^2 = 7.5), B's 2/3 5/3 2/3 (sigma^2 = 3/2 x
    2/3 = 1, lambda^2 = 1); ESS = 18 x 4.25 / 14, MCSE = sqrt(14 / 18)."""
    from gpirt_amd.chains import block_scalars, diagnostics_from_draws
    x = np.array([[1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 2, 0, 2, 1, 2, 0, 2, 0]], dtype=np.float64)[:, :, None]
    d = diagnostics_from_draws(x)
    assert d["rhat"][0] == pytest.approx(np.sqrt(10.625 / 1.5), rel=1e-14)
    assert d["ess"][0] == pytest.approx(18 * 4.25 / 14, rel=1e-14)
    assert d["mcse"][0] == pytest.approx(np.sqrt(14 / 18), rel=1e-14)
    assert d["mean"][0] == pytest.approx(54 / 18, rel=1e-14)
    s = block_scalars(np.array([1.0, np.nan, 1.2, np.inf]), np.array([10.0, 3.0, np.nan, 5.0]))
    assert s == dict(max_rhat=np.inf, min_ess=3.0, n_rhat_high=2.0, n_rhat_nan=1.0, n_ess_nan=1.0)
