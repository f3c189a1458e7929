"""Posterior summaries (include/gpirt_hip.h gpirt_sampler_summary_*, gpirt_mcmc_summary) on a machine without a GPU: the
entry points are exported and bound, the whole call checks its arguments and then fails loudly (no CPU fallback), and the
kernels of csrc/summary.hip compile for gfx950 with no scratch memory."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gpirt_mcmc_summary", "gpirt_sampler_summary_enable", "gpirt_sampler_summary_accumulate",
       "gpirt_sampler_summary_get", "gpirt_sampler_summary_totals")


@pytest.fixture(scope="module")
def lib():
    from gpirt_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _call(lib, parts=None, irfs=True, summary=True, **ptrs):
    from gpirt_amd import _lib
    n, m, S = 4, 2, 1
    y = np.ones((n, m), order="F")
    y[0, 0] = -1.0
    th = np.zeros(n)
    p = np.full((2, m), 0.1, order="F")
    irf = np.zeros((1001, m), order="F")
    dp = C.POINTER(C.c_double)
    o = _lib.default_options()
    o.rng_kind = _lib.RNG_ITEM
    sm = _lib.Summary()
    sm.parts = _lib.SUM_WAIC | _lib.SUM_PRED if parts is None else parts
    keep = []
    for k, shape in ptrs.items():
        a = np.zeros(shape, order="F")
        keep.append(a)
        setattr(sm, "h_" + k, a.ctypes.data_as(dp))
    return lib.gpirt_mcmc_summary(y.ctypes.data_as(dp), n, m, th.ctypes.data_as(dp), S, 0, p.ctypes.data_as(dp),
                                  p.ctypes.data_as(dp), p.ctypes.data_as(dp), C.byref(o), None, _lib.TICK_FN(0), None,
                                  None, None, None, irf.ctypes.data_as(dp) if irfs else None,
                                  C.byref(sm) if summary else None)


def test_summary_symbols_are_exported_and_bound(lib):
    from gpirt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gpirt_hip.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.gpirt_version() >= 104
    # the totals' order is the header's
    for i, k in enumerate(_lib.SUM_TOTALS):
        assert re.search(r"#define GPIRT_SUM_T_%s\s+%d\b" % (k.upper(), i), hdr), k
    assert re.search(r"#define GPIRT_SUM_NTOTALS\s+%d\b" % len(_lib.SUM_TOTALS), hdr)
    for k, bit in _lib.SUM_PARTS.items():
        assert re.search(r"#define GPIRT_SUM_%s\s+%d\b" % (k.upper(), bit), hdr), k


def test_summary_parts_spec():
    from gpirt_amd import _lib
    assert _lib.summary_parts(("waic", "pred")) == _lib.SUM_WAIC | _lib.SUM_PRED
    assert _lib.summary_parts("f") == _lib.SUM_F
    assert _lib.summary_parts(5) == 5 and _lib.summary_parts(()) == 0
    with pytest.raises(ValueError):
        _lib.summary_parts(("waic", "loo"))


def test_mcmc_summary_without_a_device_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this test is for the GPU-less container")
    from gpirt_amd import _lib
    assert _call(lib) == _lib.E_NODEVICE
    assert _call(lib, p_yes=(4, 2), lppd=(4, 2), theta_mean=(4,)) == _lib.E_NODEVICE
    from gpirt_amd import gpirtMCMC
    with pytest.raises(_lib.GpirtError):
        gpirtMCMC(np.array([[1, 0], [0, 1], [1, 1], [0, 0]]), 1, 0, vote_codes=dict(yea=[1], nay=[0], missing=[None]),
                  rng="item", summaries=("waic",), store_draws=False)


def test_mcmc_summary_argument_errors(lib):
    from gpirt_amd import _lib
    assert _call(lib, parts=16) == _lib.E_ARG                       # unknown part bit
    assert _call(lib, parts=_lib.SUM_WAIC | 64) == _lib.E_ARG
    assert _call(lib, irfs=False) == _lib.E_ARG                     # h_irfs is required
    assert _call(lib, summary=False) == _lib.E_ARG
    assert _call(lib, parts=_lib.SUM_WAIC, p_yes=(4, 2)) == _lib.E_ARG      # an output of a part that is off
    assert _call(lib, parts=_lib.SUM_PRED, lppd=(4, 2)) == _lib.E_ARG
    assert _call(lib, parts=_lib.SUM_PRED, f_var=(4, 2)) == _lib.E_ARG
    assert _call(lib, parts=0, theta_mean=(4,)) == _lib.E_ARG
    assert "bad argument" in _lib.last_error()
    assert lib.gpirt_sampler_summary_enable(None, _lib.SUM_WAIC) == _lib.E_ARG
    assert lib.gpirt_sampler_summary_accumulate(None) == _lib.E_ARG
    out = np.zeros(4)
    assert lib.gpirt_sampler_summary_get(None, b"p_yes", out.ctypes.data_as(C.POINTER(C.c_double)), 4) == _lib.E_ARG
    assert lib.gpirt_sampler_summary_totals(None, out.ctypes.data_as(C.POINTER(C.c_double))) == _lib.E_ARG


def test_summary_kernels_use_no_scratch():
    """The accumulate kernel streams f, mu, y and the accumulators through registers, 16 bytes a lane; no instance of it,
    nor the finishing kernels, may touch scratch memory (the way tests/test_scratch_census.py checks its kernels)."""
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-function",
             "-Wno-unused-value"]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S",
                               os.path.join(ROOT, "gpirt_amd", "csrc", "summary.hip"), "-o", out])
        txt = open(out).read()
    ks = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        priv = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
        ks[m.group(1)] = int(priv.group(1)) if priv else 0
    acc = [k for k in ks if "summary_accumulate_kernel" in k]
    assert len(acc) == 8, sorted(ks)                                # every combination of (WAIC, PRED, F)
    for frag in ("summary_finish_kernel", "summary_totals_kernel", "summary_reduce_kernel"):
        assert any(frag in k for k in ks), (frag, sorted(ks))
    for k, scratch in ks.items():
        assert scratch == 0, f"{k}: {scratch} bytes of scratch per lane"
    assert "global_load_dwordx4" in txt and "global_store_dwordx4" in txt
