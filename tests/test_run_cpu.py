"""gpirt_run and gpirt_mcmc_run (include/gpirt_hip.h) on a machine without a GPU: _lib.Run mirrors the header's struct, and
the entry refuses a missing run, a reserved slot in use and a dependant without its base before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpirt_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from gpirt_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def test_run_mirrors_the_header():
    hdr = open(os.path.join(ROOT, "include", "gpirt_hip.h")).read()
    body = re.search(r"typedef struct gpirt_run \{(.*?)\} gpirt_run;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)(\[\d+\])?$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.Run._fields_]
    # 16 words -- the stream, the 13 analyses, y_new and n_new -- then the 8 reserved ones
    assert len(names) == 17 and C.sizeof(_lib.Run) == 8 * 24
    assert _lib.Run.reserved.offset == 8 * 16
    assert [getattr(_lib.Run, f).offset for f, _ in _lib.Run._fields_] == [8 * k for k in range(17)]
    for name, struct in (("quantiles", _lib.Quantiles), ("ppc", _lib.Ppc), ("ranks", _lib.Ranks), ("score", _lib.Score),
                         ("predict", _lib.ScorePredict), ("pairs", _lib.PpcPairs), ("bins", _lib.PpcBins),
                         ("shape", _lib.Shape), ("sumscore", _lib.Sumscore), ("dif", _lib.PpcDif), ("equate", _lib.Equate),
                         ("loo", _lib.Loo), ("order", _lib.ShapeOrder)):
        assert dict(_lib.Run._fields_)[name] is C.POINTER(struct), name
        assert re.search(r"gpirt_%s\*\s+%s;" % (re.sub(r"(?<!^)(?=[A-Z])", "_", struct.__name__).lower(), name), body), name


def _call(lib, run, chains=1, rng_item=True):
    dp = C.POINTER(C.c_double)
    y = np.ones((4, 2), order="F")
    y[0, :] = -1.0
    th = np.zeros((chains, 4))
    p = np.full((2, 2), 0.1, order="F")
    irf = np.zeros((1001, 2), order="F")
    o = _lib.fast_options() if rng_item else _lib.default_options()
    sm = _lib.Summary()
    a = lambda x: x.ctypes.data_as(dp)          # noqa: E731
    return lib.gpirt_mcmc_run(a(y), 4, 2, a(th), chains, 4, 1, a(p), a(p), a(p), C.byref(o), 1, _lib.TICK_FN(0), None, None,
                              None, None, a(irf), C.byref(sm), None, C.byref(run) if run is not None else None)


def test_run_is_required_and_its_reserved_slots_are_null(lib):
    assert _call(lib, None) == _lib.E_ARG
    assert "bad argument" in _lib.last_error()
    for slot in (0, 7):
        run = _lib.Run()
        run.reserved[slot] = 1
        assert _call(lib, run) == _lib.E_ARG
        assert "reserved" in _lib.last_error()


def test_the_rng_rule_names_the_entry(lib):
    rs = C.c_void_p()
    assert lib.gpirt_rstream_create(C.byref(rs), 7) == 0
    try:
        for item, stream, chains in ((False, False, 1), (False, True, 2), (True, True, 1)):
            run = _lib.Run()
            run.rs = rs if stream else None
            assert _call(lib, run, chains=chains, rng_item=item) == _lib.E_ARG
            assert _lib.last_error() == "gpirt_mcmc_run needs GPIRT_RNG_ITEM, or GPIRT_RNG_RSTREAM with rs and one chain"
    finally:
        lib.gpirt_rstream_destroy(rs)


def test_a_dependant_without_its_base_is_refused(lib):
    """predict needs score; pairs, bins and dif need ppc; order needs shape -- refused before any device is touched."""
    from gpirt_amd import ppc as P
    from gpirt_amd import score as SC
    from gpirt_amd import shape as SH
    groups = np.array([0, 1, 0, 1], dtype=np.int32)
    for name, (struct, arrays) in (("predict", SC.predict_struct(1, 2, 1)), ("pairs", P.pairs_struct(2, 1)),
                                   ("bins", P.bins_struct(2, P.DEFAULT_CUTS, 1)),
                                   ("dif", P.dif_struct(2, 2, P.DEFAULT_CUTS, 1, groups=groups)),
                                   ("order", SH.order_struct(2, 1, 1))):
        run = _lib.Run()
        setattr(run, name, C.pointer(struct))
        assert _call(lib, run) == _lib.E_ARG, name
        assert ("need the shape posteriors" if name == "order" else "bad argument") in _lib.last_error(), name


def test_an_empty_run_reaches_the_device(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this test is for a machine without a GPU")
    assert _call(lib, _lib.Run()) == _lib.E_NODEVICE
    assert "no CPU fallback" in _lib.last_error()
