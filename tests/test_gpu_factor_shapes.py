"""The Cholesky factor and the triangular solves at the shapes the operator tests never reached, against LAPACK.

Reference throughout: LAPACK on the host in fp64 (tests/_factor_frame.py) on S = K(theta, theta) + 0.001 I built in NumPy
from grid-valued theta.  Tolerances are the project's own (tests/test_gpu_ops.py): max|L - L_ref| <= 1e-11,
||L L^T - S||_F / ||S||_F <= 1e-14 n, strict upper triangle exactly zero; solves <= 1e-10 max|X_ref|; L Z <= 1e-11.
LAPACK itself sits 1.2e-13 ... 1.6e-13 from a long-double Cholesky of the same S at n = 513 ... 2049, and the device factor
4.3e-13 from LAPACK at n = 8192, so the bounds have room.  Every case prints its measured maximum.

  A  odd leading dimensions, padded ones and a base that is only 8-byte aligned, for gpirt_potrf_lower, gpirt_factor,
     gpirt_trsm_lower and gpirt_trmm_lz -- every matrix inside a guard-band frame (a recognisable NaN around it and in
     the padding rows, compared bit for bit afterwards); the frame also around gpirt_gemm and gpirt_se_kernel.
     The persistent panel kernel fills LDS by LDS-DMA from 16-byte sources  A + even row + column * lda  (panel.hip,
     chunk_asm.h): with an odd lda or an 8-byte base every other column's source is 8-byte aligned only.  Nothing in the
     kernel branches on that; these tests are the measurement that the hardware serves such a source.
     All other 16-byte accesses of the factorisation and the solves are either LDS-side (solve64.h, potf2.h, trsm.hip's
     leaves) or guarded by (base & 15) == 0 && ld % 2 == 0 (gemm_f64.hip fastA / fastB, se_kernel.hip vec).
     A layout changes how bytes are fetched, never which products are formed or in which order (the tile sizes, the
     split-K counts and the schedule depend on n, nrhs and the switches alone), so every result must be BIT-IDENTICAL to
     the same call on an even leading dimension at a 16-byte aligned base: asserted for all four operators.
  B  gpirt_factor at both sides of every schedule edge of potrf.hip -- look-ahead (n > 2048), the 704-column first
     sub-panel (6144 <= n <= 10240), deferred updates (n <= 14336) -- and at ragged orders in between.  At 2111, 6200 and
     10241 GPIRT_DEFER=2 and GPIRT_LOOKAHEAD=2 must give the default's bits (same products per element, same order: what
     tests/test_gpu_fences.py asserts at its sizes).  GPIRT_PANEL=2 is a different algorithm inside an outer panel
     (right-looking 64-column steps with K = 64 updates instead of the left-looking kernel's chunk sums): other rounding,
     so it is held to the LAPACK tolerance instead of to the default's bits.
  C  gpirt_trsm_lower beyond n = 1792 against LAPACK's solves on LAPACK's factor (uploaded, so that a factor error cannot
     hide a solve error), orders and widths picked by the branches of trsm_rec; with GPIRT_TRSM_INV=2 at 2600 and 4352;
     and with the strict upper triangle of L filled with NaN, which must not change one bit of X.
  D  a matrix that is not positive definite at sizes with several row blocks, sub-panels, outer panels, look-ahead and
     deferred updates in flight: the returned order of the failing minor is LAPACK's, with the persistent and with the
     launch-per-step panel, and the same handle then factors the clean matrix to the tolerance.
"""
import gc
import re

import numpy as np
import pytest

import _factor_frame as F

pytestmark = pytest.mark.gpu

TOL_L, TOL_RESID, TOL_SOLVE, TOL_TRMM = 1e-11, 1e-14, 1e-10, 1e-11

_REF = {}        # n -> (theta, S, L_lapack); everything is dropped when an order above 3000 comes or goes


def _reference(n):
    if n not in _REF:
        if n > 3000 or any(k > 3000 for k in _REF):
            _REF.clear()
            gc.collect()
        theta = F.theta_grid(n, n)
        S = F.spd_matrix(theta)
        _REF[n] = (theta, S, F.lapack_factor(S))
    return _REF[n]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _check_factor(tag, L, n):
    _, S, Lref = _reference(n)
    err, resid, upper_zero = F.factor_errors(L, Lref, S)
    print(f"[factor] {tag}: max|L - L_lapack| = {err:.3e} (<= {TOL_L:g}), resid = {resid:.3e} (<= {TOL_RESID * n:.3e}), "
          f"upper zero: {upper_zero}")
    assert upper_zero, f"{tag}: the strict upper triangle is not zero"
    assert err <= TOL_L, f"{tag}: max|L - L_lapack| = {err:.3e}"          # (a NaN fails too)
    assert resid <= TOL_RESID * n, f"{tag}: residual {resid:.3e}"


def _factor_into(handle, theta_d, view):
    """gpirt_factor into a caller-owned matrix (Handle.factor allocates its own)."""
    from gpirt_amd._lib import check
    from gpirt_amd.ops import _ld, _p
    info = handle.lib.gpirt_factor(handle._h, _p(theta_d), theta_d.shape[0], _p(view), _ld(view))
    if info > 0:
        raise RuntimeError("chol(): decomposition failed (leading minor %d)" % info)
    check(info)


# ------------------------------------------------------------------------------------------------------------------ A

def _ld_of(n, kind):
    """odd: the nearest odd leading dimension above n (n itself when n is odd: packed); even: aligned twin of it;
    pad64: n + 64 rounded up to even."""
    if kind == "odd":
        return n if n % 2 else n + 1
    if kind == "even":
        return n + 2 if n % 2 == 0 else n + 1
    if kind == "pad64":
        return n + 64 + (n % 2)
    raise ValueError(kind)


# (n, lda, offset in doubles behind a 16-byte aligned address)
_FACTOR_LAYOUTS = ([(n, n, 0) for n in (65, 191, 193, 257, 1001, 1339, 2049, 2601)] +
                   [(n, n + pad, 0) for n in (300, 1000, 2600) for pad in (1, 2, 64)] +
                   [(n, n, 1) for n in (1000, 2600)])
_ALIGNED = {}    # (entry, n) -> the factor of the aligned, even-lda call (one order kept)


def _run_factor(handle, entry, n, lda, offset):
    from gpirt_amd.ops import to_device
    theta, S, _ = _reference(n)
    fr = F.Frame(n, n, lda, offset)
    if entry == "potrf_lower":
        fr.put(S)
        handle.potrf_lower(fr.view)
    else:
        _factor_into(handle, to_device(theta), fr.view)
    return fr


def _aligned_factor(handle, entry, n):
    if (entry, n) not in _ALIGNED:
        for key in [key for key in _ALIGNED if key[1] != n]:
            del _ALIGNED[key]
        fr = _run_factor(handle, entry, n, n + (n % 2), 0)
        fr.assert_intact(f"{entry} n={n} aligned twin")
        _ALIGNED[(entry, n)] = fr.get()
    return _ALIGNED[(entry, n)]


@pytest.mark.parametrize("entry", ["potrf_lower", "factor"])
@pytest.mark.parametrize("n,lda,offset", _FACTOR_LAYOUTS, ids=[f"n{n}-lda{l}-off{o}" for n, l, o in _FACTOR_LAYOUTS])
def test_factor_odd_padded_offset_layouts(handle, entry, n, lda, offset):
    """A: gpirt_potrf_lower / gpirt_factor on packed odd orders, odd and padded lda, an 8-byte aligned base -- LAPACK's
    factor to the tolerance, guard bands untouched, and the bits of the same call on an even lda at an aligned base."""
    tag = f"{entry} n={n} lda={lda} offset={offset}"
    fr = _run_factor(handle, entry, n, lda, offset)
    L = fr.get()
    fr.assert_intact(tag)
    _check_factor(tag, L, n)
    assert _bits_equal(L, _aligned_factor(handle, entry, n)), f"{tag}: differs from the aligned even-lda call"


_SOLVE_LAYOUTS = ["odd", "pad64", "offset"]


def _solve_frame(n, cols, kind):
    if kind == "offset":
        return F.Frame(n, cols, _ld_of(n, "even"), 1)
    return F.Frame(n, cols, _ld_of(n, kind), 0)


def _trmm_into(handle, Lv, Zv, outv):
    from gpirt_amd._lib import check
    from gpirt_amd.ops import _ld, _p
    n, m = Zv.shape
    check(handle.lib.gpirt_trmm_lz(handle._h, _p(Lv), n, _ld(Lv), _p(Zv), m, _ld(Zv), _p(outv), _ld(outv)))


_SOLVE_TWIN = {}     # (n, nrhs) -> results of the aligned even-ld calls (one entry kept)


def _solve_all(handle, n, nrhs, Lref, Z, kl, kb):
    """(X forward, X transposed, L Z) with L in a `kl` frame and the right-hand sides / the output in `kb` frames."""
    Lf = _solve_frame(n, n, kl).put(Lref)
    out = []
    frames = [Lf]
    for trans in (False, True):
        Bf = _solve_frame(n, nrhs, kb).put(Z)
        handle.trsm_lower(Lf.view, Bf.view, trans=trans)
        out.append(Bf.get())
        frames.append(Bf)
    Zf, Of = _solve_frame(n, nrhs, kb).put(Z), _solve_frame(n, nrhs, kb)
    _trmm_into(handle, Lf.view, Zf.view, Of.view)
    out.append(Of.get())
    frames += [Zf, Of]
    for f in frames:
        f.assert_intact(f"solves n={n} nrhs={nrhs} ldl:{kl} ldb:{kb}")
    return out


@pytest.mark.parametrize("kb", _SOLVE_LAYOUTS)
@pytest.mark.parametrize("kl", _SOLVE_LAYOUTS)
@pytest.mark.parametrize("n,nrhs", [(1339, 7), (1339, 300), (2600, 7), (2600, 300)])
def test_solves_odd_padded_offset_layouts(handle, n, nrhs, kl, kb):
    """A: gpirt_trsm_lower (both trans) and gpirt_trmm_lz with ldl and ldb varied independently over an odd leading
    dimension, a padded one and an 8-byte aligned base: LAPACK's solves / the host product to the tolerance, guard bands
    untouched, and the bits of the calls on even leading dimensions at aligned bases."""
    _, _, Lref = _reference(n)
    Z = np.random.default_rng(n + nrhs).standard_normal((n, nrhs))
    got = _solve_all(handle, n, nrhs, Lref, Z, kl, kb)
    if (n, nrhs) not in _SOLVE_TWIN:
        _SOLVE_TWIN.clear()
        Lt = F.Frame(n, n, _ld_of(n, "even"), 0).put(Lref)
        twin = []
        for trans in (False, True):
            Bt = F.Frame(n, nrhs, _ld_of(n, "even"), 0).put(Z)
            handle.trsm_lower(Lt.view, Bt.view, trans=trans)
            twin.append(Bt.get())
        Ot = F.Frame(n, nrhs, _ld_of(n, "even"), 0)
        _trmm_into(handle, Lt.view, F.Frame(n, nrhs, _ld_of(n, "even"), 0).put(Z).view, Ot.view)
        twin.append(Ot.get())
        _SOLVE_TWIN[(n, nrhs)] = twin
    twin = _SOLVE_TWIN[(n, nrhs)]
    for trans in (False, True):
        ref = F.lapack_solve(Lref, Z, trans)
        err, scale = float(np.abs(got[trans] - ref).max()), float(np.abs(ref).max())
        print(f"[trsm] n={n} nrhs={nrhs} trans={int(trans)} ldl:{kl} ldb:{kb}: max|X - X_lapack| = {err:.3e} "
              f"(<= {TOL_SOLVE * scale:.3e})")
        assert err <= TOL_SOLVE * scale
        assert _bits_equal(got[trans], twin[trans]), f"trsm trans={int(trans)} differs from the aligned even-ld call"
    err = float(np.abs(got[2] - Lref @ Z).max())
    print(f"[trmm] n={n} m={nrhs} ldl:{kl} ldz/ldo:{kb}: max|L Z - host| = {err:.3e} (<= {TOL_TRMM:g})")
    assert err <= TOL_TRMM
    assert _bits_equal(got[2], twin[2]), "trmm differs from the aligned even-ld call"


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
def test_gemm_inside_guard_bands(handle, ta, tb):
    """A: gpirt_gemm with ldc > M (odd), padded lda / ldb, alpha and beta both in play: the host product to the tolerance
    of test_gemm_matches_numpy, nothing written outside C, no padding value in the result."""
    M, N, K = 1001, 300, 513
    rng = np.random.default_rng(11 + 2 * ta + tb)
    A = rng.standard_normal((K, M) if ta else (M, K))
    B = rng.standard_normal((N, K) if tb else (K, N))
    C0 = rng.standard_normal((M, N))
    Af = F.Frame(A.shape[0], A.shape[1], A.shape[0] + 1, 0).put(A)
    Bf = F.Frame(B.shape[0], B.shape[1], B.shape[0] + 2, 1).put(B)
    Cf = F.Frame(M, N, M + 2, 0).put(C0)
    handle.gemm(Af.view, Bf.view, ta=ta, tb=tb, alpha=-1.5, beta=0.5, C_out=Cf.view)
    ref = -1.5 * (A.T if ta else A) @ (B.T if tb else B) + 0.5 * C0
    err = float(np.abs(Cf.get() - ref).max())
    print(f"[gemm] ta={int(ta)} tb={int(tb)} {M}x{N}x{K} ldc={M + 2}: max err = {err:.3e}")
    assert err <= 1e-11 * max(1.0, np.abs(ref).max())
    for f in (Af, Bf, Cf):
        f.assert_intact(f"gemm ta={int(ta)} tb={int(tb)}")
    # beta = 0 must not read C: the frame's NaN filling stays out of the result
    Cn = F.Frame(M, N, M + 1, 0)
    handle.gemm(Af.view, Bf.view, ta=ta, tb=tb, alpha=1.0, beta=0.0, C_out=Cn.view)
    ref = (A.T if ta else A) @ (B.T if tb else B)
    assert float(np.abs(Cn.get() - ref).max()) <= 1e-11 * max(1.0, np.abs(ref).max())
    Cn.assert_intact(f"gemm beta=0 ta={int(ta)} tb={int(tb)}")


@pytest.mark.parametrize("n1,n2,pad,offset", [(100, 100, 1, 0), (513, 77, 1, 0), (1024, 1001, 2, 0), (1024, 1001, 0, 1),
                                              (301, 40, 64, 1)])
def test_se_kernel_inside_guard_bands(handle, n1, n2, pad, offset):
    """A: gpirt_se_kernel with ld > n1 (odd and even) and an 8-byte aligned output: the NumPy kernel to 4e-16 (the bound
    of test_se_kernel), nothing written outside the n1 x n2 matrix."""
    from gpirt_amd._lib import check
    from gpirt_amd.ops import _ld, _p, to_device
    rng = np.random.default_rng(n1 + n2)
    x1, x2 = rng.standard_normal(n1) * 2, rng.standard_normal(n2) * 2
    jitter = 0.001 if n1 == n2 else 0.0
    Of = F.Frame(n1, n2, n1 + pad, offset)
    x1d, x2d = to_device(x1), to_device(x2)
    check(handle.lib.gpirt_se_kernel(handle._h, _p(x1d), n1, _p(x2d), n2, _p(Of.view), _ld(Of.view), jitter))
    ref = np.exp(-0.5 * (x1[:, None] - x2[None, :]) ** 2)
    if n1 == n2:
        ref[np.diag_indices(n1)] += jitter
    err = float(np.abs(Of.get() - ref).max())
    print(f"[se_kernel] {n1}x{n2} ld={n1 + pad} offset={offset}: max err = {err:.3e}")
    assert err <= 4e-16
    Of.assert_intact(f"se_kernel {n1}x{n2}")


# ------------------------------------------------------------------------------------------------------------------ B

_SCHEDULE_ORDERS = [2048, 2049, 2111, 3000, 5000, 6143, 6144, 6200, 10240, 10241, 14336, 14337]
_SWITCH_ORDERS = [2111, 6200, 10241]


@pytest.mark.parametrize("n", _SCHEDULE_ORDERS)
def test_factor_at_schedule_edges(handle, n):
    """B: gpirt_factor with the default switches at both sides of every schedule edge and at ragged orders between them,
    against LAPACK."""
    from gpirt_amd.ops import to_device, to_host
    theta, _, _ = _reference(n)
    L = to_host(handle.factor(to_device(theta)))
    _check_factor(f"schedule n={n}", L, n)


@pytest.mark.parametrize("switch", ["GPIRT_DEFER", "GPIRT_LOOKAHEAD"])
@pytest.mark.parametrize("n", _SWITCH_ORDERS)
def test_schedule_switches_keep_the_bits_at_ragged_orders(handle, n, switch):
    """B: the plain right-looking order (GPIRT_DEFER=2) and no look-ahead (GPIRT_LOOKAHEAD=2) apply the same products in
    the same order per element: the default factor bit for bit, at one ragged order per schedule class."""
    import torch
    from gpirt_amd.ops import to_device
    th = to_device(F.theta_grid(n, n))
    ref = handle.factor(th)
    with handle.config(switch, 2):
        got = handle.factor(th)
    same = torch.equal(ref.view(torch.int64), got.view(torch.int64))
    print(f"[switch] n={n} {switch}=2: bit-identical to the default: {same}")
    assert same


@pytest.mark.parametrize("n", _SWITCH_ORDERS)
def test_launch_per_step_panel_at_ragged_orders(handle, n):
    """B: GPIRT_PANEL=2 (the launch-per-step panel: the guard fallback's path) forms an outer panel by right-looking
    K = 64 updates, the persistent kernel by left-looking chunk sums -- different rounding, so not the default's bits: it is
    held to LAPACK with the same tolerance."""
    from gpirt_amd.ops import to_device, to_host
    theta, _, _ = _reference(n)
    with handle.config("GPIRT_PANEL", 2):
        L = to_host(handle.factor(to_device(theta)))
    _check_factor(f"GPIRT_PANEL=2 n={n}", L, n)


# ------------------------------------------------------------------------------------------------------------------ C

# n: 2304 = an odd count of 256-blocks, 2600 = ragged tail, 4096 / 4352 = 1024-aligned / not, 6200 = ragged, several levels
# nrhs: 1 and 64 (substitution only / inverses from 64 on), 300, 1281 (the nrhs <= 1280 switch of the thin form and of the
# triangular leaf product), 1001 + 40 (what draw_fstar passes)
_SOLVE_CASES = [(n, nrhs, inv) for n in (2304, 2600, 4096, 4352, 6200) for inv in ((1, 2) if n in (2600, 4352) else (1,))
                for nrhs in (1, 64, 300, 1281, 1041)]
_LDEV = {}       # n -> (L on the device, the same with NaN above the diagonal); one entry kept


def _device_factor(n):
    import torch
    from gpirt_amd.ops import to_device
    if n not in _LDEV:
        _LDEV.clear()
        _, _, Lref = _reference(n)
        Ld = to_device(Lref)
        Ln = Ld.clone()
        iu = torch.triu_indices(n, n, 1, device=Ld.device)
        Ln[iu[0], iu[1]] = float("nan")
        del iu
        _LDEV[n] = (Ld, Ln)
    return _LDEV[n]


@pytest.mark.parametrize("n,nrhs,inv", _SOLVE_CASES)
def test_trsm_beyond_1792_against_lapack(handle, n, nrhs, inv):
    """C: gpirt_trsm_lower, both trans, on LAPACK's factor against LAPACK's solve; GPIRT_TRSM_INV=2 (every leaf a
    substitution) at 2600 and 4352; and solve(trimatl(L), B) does not read above the diagonal: NaN there changes no bit."""
    from gpirt_amd.ops import to_device, to_host
    _, _, Lref = _reference(n)
    Ld, Lnan = _device_factor(n)
    B = np.random.default_rng(7 * n + nrhs).standard_normal((n, nrhs))
    for trans in (False, True):
        with handle.config("GPIRT_TRSM_INV", inv):
            X = to_host(handle.trsm_lower(Ld, to_device(B), trans=trans))
            Xn = to_host(handle.trsm_lower(Lnan, to_device(B), trans=trans))
        ref = F.lapack_solve(Lref, B, trans)
        err, scale = float(np.abs(X - ref).max()), float(np.abs(ref).max())
        print(f"[trsm] n={n} nrhs={nrhs} trans={int(trans)} GPIRT_TRSM_INV={inv}: max|X - X_lapack| = {err:.3e} "
              f"(<= {TOL_SOLVE * scale:.3e}), NaN above the diagonal changes X: {not _bits_equal(X, Xn)}")
        assert err <= TOL_SOLVE * scale
        assert _bits_equal(X, Xn), "the solve read the strict upper triangle of L"


# ------------------------------------------------------------------------------------------------------------------ D

# k: in the first 64-block, the first sub-panel, the second sub-panel, the second outer panel, the ragged last block; and at
# n = 6200 in the fifth outer panel, with look-ahead and deferred updates in flight
_NOT_PD = [(2600, 10), (2600, 300), (2600, 700), (2600, 1500), (2600, 2590), (6200, 5000)]


@pytest.mark.parametrize("panel", [1, 2])
@pytest.mark.parametrize("n,k", _NOT_PD)
def test_not_positive_definite_returns_lapacks_info_and_leaves_the_handle_usable(handle, n, k, panel):
    """D: S with S[k, k] = -1.  The call must raise with exactly LAPACK's info (k + 1), persistent and launch-per-step
    panel; the same handle must then factor the clean S to the tolerance (info word and progress counters reusable)."""
    from gpirt_amd.ops import to_device, to_host
    _, S, _ = _reference(n)
    bad = S.copy(order="F")
    bad[k, k] = -1.0
    info_ref = F.lapack_info(bad)
    assert info_ref == k + 1
    with handle.config("GPIRT_PANEL", panel):
        with pytest.raises(RuntimeError, match="decomposition failed") as e:
            handle.potrf_lower(to_device(bad))
        got = int(re.search(r"leading minor (\d+)", str(e.value)).group(1))
        print(f"[not PD] n={n} k={k} GPIRT_PANEL={panel}: info = {got}, LAPACK's = {info_ref}")
        assert got == info_ref
        del bad
        L = to_host(handle.potrf_lower(to_device(S)))
    _check_factor(f"clean refactor after info={info_ref}, n={n} GPIRT_PANEL={panel}", L, n)
