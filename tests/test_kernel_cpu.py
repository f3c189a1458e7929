"""The covariance kernel's host side without a GPU: gpirt_kernel_check's refusals and decisions, its certificate against the
NumPy long-double figure (tests/_kernel_exact.py), and gpirt_amd.kernel's NumPy statement."""
import ctypes as C
import math

import numpy as np
import pytest

import _kernel_exact as KX


@pytest.fixture(scope="module")
def lib():
    from gpirt_amd import _lib, build
    import os
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


def _kernel(lib, family=0, ell=1.0):
    from gpirt_amd import _lib
    k = _lib.Kernel()
    lib.gpirt_kernel_default(C.byref(k))
    k.family, k.length_scale = family, ell
    return k


def _check(lib, k, r):
    cert, mr = C.c_double(-1.0), C.c_int(-1)
    rc = lib.gpirt_kernel_check(C.byref(k), r, C.byref(cert), C.byref(mr))
    return rc, cert.value, mr.value


def test_default_and_layout(lib):
    from gpirt_amd import _lib
    assert lib.gpirt_version() >= 124
    k = _lib.Kernel()
    k.family, k.reserved0, k.length_scale = 7, 7, 7.0
    lib.gpirt_kernel_default(C.byref(k))
    assert k.family == _lib.KERNEL_SE == 0 and k.length_scale == 1.0 and k.reserved0 == 0 and not any(k.reserved)
    assert C.sizeof(_lib.Kernel) == 48 and _lib.Kernel.length_scale.offset == 8 and _lib.Kernel.reserved.offset == 16
    assert (_lib.KERNEL_MATERN52, _lib.KERNEL_MATERN32) == (1, 2)
    assert lib.gpirt_kernel_check(C.byref(k), 0, None, None) == 0            # the outputs may be NULL
    assert lib.gpirt_kernel_check(None, 0, None, None) == _lib.E_ARG
    assert lib.gpirt_kernel_set(None, C.byref(k)) == _lib.E_ARG and lib.gpirt_kernel_get(None, C.byref(k)) == _lib.E_ARG


@pytest.mark.parametrize("family", [-1, 3, 17])
def test_check_refuses_a_family_out_of_range(lib, family):
    from gpirt_amd import _lib
    rc, _, _ = _check(lib, _kernel(lib, family), 0)
    assert rc == _lib.E_ARG and "family" in _lib.last_error()


@pytest.mark.parametrize("ell", [float("nan"), 0.0, -1.0, 0.009, 1001.0, float("inf")])
@pytest.mark.parametrize("family", [0, 1, 2])
def test_check_refuses_a_length_scale_out_of_range(lib, family, ell):
    from gpirt_amd import _lib
    rc, _, _ = _check(lib, _kernel(lib, family, ell), 0)
    assert rc == _lib.E_ARG and "length_scale" in _lib.last_error()


def test_check_accepts_the_limits_of_the_length_scale(lib):
    for ell in (0.01, 1000.0):
        for family in (0, 1, 2):
            assert _check(lib, _kernel(lib, family, ell), 0)[0] == 0


def test_check_refuses_a_reserved_word(lib):
    from gpirt_amd import _lib
    k = _kernel(lib)
    k.reserved0 = 1
    assert _check(lib, k, 0)[0] == _lib.E_ARG and "reserved" in _lib.last_error()
    for q in range(4):
        k = _kernel(lib)
        k.reserved[q] = 1
        assert _check(lib, k, 0)[0] == _lib.E_ARG and "reserved" in _lib.last_error()


@pytest.mark.parametrize("r", [-16, 8, 24, 144])
def test_check_refuses_a_rank_the_option_does_not_allow(lib, r):
    from gpirt_amd import _lib
    assert _check(lib, _kernel(lib), r)[0] == _lib.E_ARG and "kstar_rank" in _lib.last_error()


@pytest.mark.parametrize("family", [1, 2])
def test_check_refuses_every_rank_for_a_matern_kernel(lib, family):
    from gpirt_amd import _lib
    rc, cert, mr = _check(lib, _kernel(lib, family, 1.0), 64)
    assert rc == _lib.E_ARG and mr == 0
    assert "Matern" in _lib.last_error() and "not analytic" in _lib.last_error()
    assert cert > 1e-9                                   # (algebraic convergence: nowhere near rounding at r = 64)
    assert _check(lib, _kernel(lib, family, 1.0), 0) == (0, 0.0, 0)


def test_check_refuses_se_half_at_rank_64_and_names_the_rank_that_passes(lib):
    from gpirt_amd import _lib
    want = KX.min_rank("se", 0.5)
    assert want in (80, 96)                              # by the issue's table: 64 gives 2.3e-9, 96 1.4e-16
    rc, cert, mr = _check(lib, _kernel(lib, 0, 0.5), 64)
    msg = _lib.last_error()
    assert rc == _lib.E_ARG and mr == want
    assert f"{cert:.3g}" in msg and f"passes is {want}" in msg
    assert _check(lib, _kernel(lib, 0, 0.5), want)[0] == 0


@pytest.mark.parametrize("ell,r", [(1.0, 64), (0.7, 64), (2.0, 48), (0.35, 128), (0.5, 96), (1.0, 48)])
def test_check_accepts(lib, ell, r):
    rc, cert, mr = _check(lib, _kernel(lib, 0, ell), r)
    line = KX.certificate_line()
    print(f"MEASURED se ell={ell} r={r}: certificate {cert:.3e} (NumPy {KX.certificate('se', ell, r):.3e}, the line {line:.3e})")
    assert rc == 0 and mr == 0
    assert cert <= line and KX.certificate("se", ell, r) <= line


def test_check_refuses_the_approximate_ranks_of_the_unit_kernel(lib):
    """(se, 1) at r = 16 and 32 are the documented approximations: above the line, though a sampler under the DEFAULT kernel
    still takes them, as it always has"""
    from gpirt_amd import _lib
    for r in (16, 32):
        rc, cert, mr = _check(lib, _kernel(lib, 0, 1.0), r)
        assert rc == _lib.E_ARG and mr == 48 and cert > KX.certificate_line()


@pytest.mark.parametrize("ell,r", [(1.0, 32), (0.5, 64)])
def test_certificate_agrees_with_numpy(lib, ell, r):
    """where the figure is far above rounding the two long-double evaluations agree to 1e-6 relative"""
    _, cert, _ = _check(lib, _kernel(lib, 0, ell), r)
    ref = KX.certificate("se", ell, r)
    print(f"MEASURED se ell={ell} r={r}: certificate {cert:.9e}, NumPy {ref:.9e}")
    assert ref > 1e-10 and abs(cert - ref) <= 1e-6 * ref


def test_rank_certificate_wrapper():
    from gpirt_amd import _lib, kernel as K
    a = K.rank_certificate("se", 1.0, 64)
    assert a["accepted"] and a["min_rank"] == 0 and a["message"] == "" and 0 < a["certificate"] <= KX.certificate_line()
    b = K.rank_certificate("se", 0.5, 64)
    assert not b["accepted"] and b["min_rank"] == KX.min_rank("se", 0.5) and "refused" in b["message"]
    c = K.rank_certificate("matern52", 1.0, 64)
    assert not c["accepted"] and c["min_rank"] == 0
    assert K.rank_certificate("matern32", 2.0, 0)["accepted"]
    assert K.fast_rank(None) == 64 and K.fast_rank("se") == 64 and K.fast_rank(dict(family="se", length_scale=0.7)) == 64
    assert K.fast_rank(dict(family="se", length_scale=0.5)) == KX.min_rank("se", 0.5)
    assert K.fast_rank("matern52") == 0 and K.fast_rank(dict(family="matern32", length_scale=3.0)) == 0
    with pytest.raises(ValueError):
        K.rank_certificate("se", 1.0, 24)
    with pytest.raises(ValueError):
        K.rank_certificate("cubic", 1.0, 64)
    with pytest.raises(_lib.GpirtError):
        K.rank_certificate("se", 0.001, 64)
    with pytest.raises(_lib.GpirtError):
        K.fast_rank(dict(family="matern52", length_scale=float("nan")))


def test_kernel_arguments():
    from gpirt_amd import kernel as K
    assert K.spec(None) == (0, 1.0) and K.spec("matern32") == (2, 1.0)
    assert K.spec(dict(family="matern52", length_scale=0.7)) == (1, 0.7) and K.spec(dict(family=2)) == (2, 1.0)
    assert K.as_dict("se") == dict(family="se", length_scale=1.0)
    assert K.is_default(None) and K.is_default("se") and not K.is_default("matern52")
    assert not K.is_default(dict(family="se", length_scale=2.0))
    k = K.struct(dict(family="matern32", length_scale=2.5))
    assert (k.family, k.length_scale, k.reserved0) == (2, 2.5, 0) and not any(k.reserved)
    for bad in ("rbf", dict(family="se", scale=2.0), dict(length_scale=2.0), 3, dict(family=1.5)):
        with pytest.raises(ValueError):
            K.spec(bad)


@pytest.mark.parametrize("ell", KX.LENGTH_SCALES)
@pytest.mark.parametrize("family", KX.FAMILIES)
def test_kernel_matrix_against_long_double(family, ell):
    """the NumPy statement follows the device's operations, so it meets the device's derived bound (NumPy's exp is within an
    ulp, like the device library's); k(0) = 1 exactly and the matrix is symmetric"""
    from gpirt_amd import kernel as K
    rng = np.random.default_rng(11)
    x1, x2 = rng.standard_normal(257) * 2, rng.standard_normal(129) * 2
    x2[:5] = x1[:5]
    got = K.kernel_matrix(x1, x2, family, ell)
    err = float(np.abs(got.astype(KX.LD) - KX.kernel_ld(family, ell, x1, x2)).max())
    print(f"MEASURED kernel_matrix {family} ell={ell}: max |K - long double| {err:.2e} (bound {KX.k_tolerance(family, ell):.2e})")
    assert got.shape == (257, 129) and err <= KX.k_tolerance(family, ell)
    assert (got[np.arange(5), np.arange(5)] == 1.0).all()
    S = K.kernel_matrix(x1, x1, family, ell)
    assert np.array_equal(S, S.T) and (np.diag(S) == 1.0).all() and (S <= 1.0).all() and (S >= 0.0).all()


def test_kernel_matrix_default_is_the_reference_expression():
    from gpirt_amd import kernel as K
    x = np.linspace(-5, 5, 41)
    assert np.array_equal(K.kernel_matrix(x, x), np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2))
    with pytest.raises(ValueError):
        K.kernel_matrix(x, x, "se", 0.0)
    with pytest.raises(ValueError):
        K.kernel_matrix(x, x, "matern12", 1.0)


def test_families_at_their_defining_points():
    """the long-double references themselves: k(0) = 1, and the closed forms at r = 1"""
    one = KX.kernel_ld("se", 2.0, [0.0], [2.0])[0, 0]
    assert abs(float(one) - math.exp(-0.5)) < 1e-17
    a = math.sqrt(5.0)
    assert abs(float(KX.kernel_ld("matern52", 0.5, [1.0], [1.5])[0, 0]) - (1 + a + a * a / 3) * math.exp(-a)) < 1e-16
    a = math.sqrt(3.0)
    assert abs(float(KX.kernel_ld("matern32", 4.0, [-2.0], [2.0])[0, 0]) - (1 + a) * math.exp(-a)) < 1e-16
    for fam in KX.FAMILIES:
        assert KX.kernel_ld(fam, 0.35, [1.25], [1.25])[0, 0] == 1
