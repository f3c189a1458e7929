"""The structured factor in parts as narrow as draw_f's product reads them (gpirt_amd/csrc/factor_lr.hip).
GPIRT_FLR_NARROW: 1 = from n = 2048 on the parts are GPIRT_NU_SUB wide, 2 = always 512 (the library before version 140, bit for
bit), 3 = at every eligible n.  The small sizes here run with it and the three switches of tests/test_gpu_factor_lr.py at 3 and
GPIRT_NU_SUB at the width under test.

Bounds, those of tests/test_gpu_factor_lr.py (tests/test_factor_lr_narrow_cpu.py has the NumPy statement's figures at these
widths): 1e-10 on the blocks, 1e-9 on the node rows and on f* relative to max|f*|, 1e-10 max(1, max|f|) on f and on nu.  m = 8."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", fstar_fused=True, kstar_rank=64, theta_stabilise=True)
M = 8
NARROW = "GPIRT_FLR_NARROW"
OLDER = ("GPIRT_FACTOR_LR", "GPIRT_NU_LR", "GPIRT_FSTAR_FREE")
KINDS = ["grid_normal", "grid_uniform", "off_grid", "sorted", "all_equal", "half_minus5_half_plus5", "two_points_0.01_apart"]
SIZES = [64, 128, 192, 576, 1088, 1536]        # one block, exactly one part (at 64 / 128), ragged parts, several parts
WIDTHS = [64, 128, 256]


def theta_case(kind, n):
    rng = np.random.default_rng(2000 + n)
    g = -5.0 + np.arange(1001, dtype=np.float64) * 0.01
    normal = lambda: g[np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01).astype(int), 0, 1000)]
    return {"grid_normal": normal, "grid_uniform": lambda: g[rng.integers(0, 1001, n)], "off_grid": lambda: rng.uniform(-5.0, 5.0, n),
            "sorted": lambda: np.sort(normal()), "all_equal": lambda: np.full(n, g[617]),
            "half_minus5_half_plus5": lambda: np.where(np.arange(n) < n // 2, -5.0, 5.0),
            "two_points_0.01_apart": lambda: np.where(np.arange(n) % 2 == 0, g[400], g[401])}[kind]()


@contextlib.contextmanager
def switches(handle, older=3, narrow=3, width=None, **more):
    with contextlib.ExitStack() as st:
        for k in OLDER:
            st.enter_context(handle.config(k, older))
        st.enter_context(handle.config(NARROW, narrow))
        if width is not None:
            st.enter_context(handle.config("GPIRT_NU_SUB", width))
        for k, v in more.items():
            st.enter_context(handle.config(k, v))
        yield


def _sampler(handle, n, m=M, structured=True, seed=17, **kw):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=311 + n)
    return Sampler(handle, y, th0, seed=seed, **dict(FAST, factor_structured=structured, **kw))


def _blocks_of(L, w):
    return [L[p:p + w, p:p + w] for p in range(0, L.shape[0], w)]


def _factored(s):
    s.factor()
    s.check()
    return s.factor_lr_blocks(), np.array(s.nu_lr_rows())


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(np.array_equal(p, q) for p, q in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_blocks_and_node_rows_against_the_dense_factor(handle, n, w):
    s = _sampler(handle, n)
    s.init()
    with switches(handle, width=w):
        for kind in KINDS:
            s.set("theta", theta_case(kind, n))
            c0, d0 = s.factor_lr_count, s.dense_factor_count
            blocks, rows = _factored(s)
            assert s.factor_lr_width == w
            assert (s.factor_lr_count - c0, s.dense_factor_count - d0) == (1, 0)
            with handle.config("GPIRT_FACTOR_LR", 2):
                s.factor()
                s.check()
            assert s.factor_lr_width == 0
            L, rows_dense = np.array(s.get("L")), np.array(s.nu_lr_rows())
            assert (s.factor_lr_count - c0, s.dense_factor_count - d0) == (1, 1)
            dense = _blocks_of(L, w)
            assert [p.shape for p in blocks] == [p.shape for p in dense]
            gap_blocks = max(float(np.abs(a - b).max()) for a, b in zip(blocks, dense))
            gap_rows = float(np.abs(rows - rows_dense).max())
            pivot = min(float(np.diag(a).min()) for a in blocks)
            print(f"MEASURED {kind} n={n} w={w}: blocks {gap_blocks:.2e}, node rows {gap_rows:.2e}, smallest pivot {pivot:.4f}")
            for a in blocks:
                assert np.array_equal(a, np.tril(a)), "strict upper triangle inside a block"
            assert pivot >= 0.03
            assert gap_blocks <= 1e-10
            assert gap_rows <= 1e-9
    s.close()


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_the_two_schedules_give_the_same_bits(handle, n, w):
    s = _sampler(handle, n)
    s.init()
    with switches(handle, width=w):
        for kind in KINDS:
            s.set("theta", theta_case(kind, n))
            got = {}
            for fuse in (1, 2):
                with handle.config("GPIRT_FLR_FUSE", fuse):
                    got[fuse] = _factored(s)
                assert s.factor_lr_width == w
            assert _same(got[1], got[2]), (kind, n, w)
    s.close()


@pytest.mark.parametrize("n", [576, 1088])
def test_nothing_is_carried_from_one_factorisation_to_the_next(handle, n):
    th1, th2 = theta_case("off_grid", n), theta_case("grid_normal", n)
    with switches(handle, width=128):
        fresh = _sampler(handle, n)
        fresh.init()
        fresh.set("theta", th2)
        want = _factored(fresh)
        fresh.close()
        for first_width in (128, 256, 64, 512):
            s = _sampler(handle, n)
            s.init()
            s.set("theta", th1)
            with handle.config("GPIRT_NU_SUB", first_width):
                _factored(s)
                assert s.factor_lr_width == first_width
            s.set("theta", th2)
            assert _same(_factored(s), want), first_width
            s.close()


def test_item_shards_give_the_same_bits(handle):
    n, m = 1088, 8
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=5)
    kw = dict(FAST, factor_structured=True)
    a = Sampler(handle, y, th0, seed=5, **kw)
    shards = [Sampler(handle, y[:, j0:j0 + 4], th0, seed=5, item0=j0, m_total=m, **kw) for j0 in (0, 4)]
    with switches(handle, width=128):
        a.init()
        for j0, c in zip((0, 4), shards):
            c.init()
            for k in ("f", "mu", "beta"):
                c.set(k, a.get(k)[:, j0:j0 + 4])
        want = _factored(a)
        assert a.factor_lr_width == 128
        a.draw_f(); a.check()
        for j0, c in zip((0, 4), shards):
            assert _same(_factored(c), want), j0
            c.draw_f(); c.check()
            assert np.array_equal(c.get("f"), a.get("f")[:, j0:j0 + 4]), j0
    a.close()
    for c in shards:
        c.close()


def test_three_whole_steps_against_parts_512_wide(handle):
    n = 1088
    a, b = _sampler(handle, n), _sampler(handle, n)
    modes = ((a, 3), (b, 2))
    with switches(handle, width=128):
        for c in (a, b):
            c.init()
        for it in range(3):
            for c, narrow in modes:
                with handle.config(NARROW, narrow):
                    c.step()
                    c.check()
            assert (a.factor_lr_width, b.factor_lr_width) == (128, 512)
            fa, fb, sa, sb = a.get("f"), b.get("f"), a.get("fstar"), b.get("fstar")
            gap_f = float(np.abs(fa - fb).max()) / max(1.0, float(np.abs(fb).max()))
            gap_s = float(np.abs(sa - sb).max()) / float(np.abs(sb).max())
            print(f"MEASURED step {it + 1} at {n} x {M}: |f - f_512| / max(1, max|f|) {gap_f:.2e}, |f* - f*_512| / max|f*| {gap_s:.2e}")
            assert np.array_equal(a.get("theta"), b.get("theta"))
            assert np.array_equal(a.get("ess_k"), b.get("ess_k"))
            assert gap_f <= 1e-10
            assert gap_s <= 1e-9
    assert (a.factor_lr_count, b.factor_lr_count) == (3, 3)
    assert (a.dense_factor_count, b.dense_factor_count) == (1, 1)          # (init's factor is the dense one)
    a.close(); b.close()


def test_whoever_reads_wider_parts_gets_them(handle):
    n = 1088
    a, b = _sampler(handle, n), _sampler(handle, n, structured=False)
    with switches(handle, width=64):
        for c in (a, b):
            c.init()
        b.factor(); b.check()
        Lb = np.array(b.get("L"))
        # factor_lr_parts keeps its 512-wide shape: the structured factor at 512 is formed for it, counted in neither counter
        a.factor(); a.check()
        assert a.factor_lr_width == 64
        c0, d0 = a.factor_lr_count, a.dense_factor_count
        parts = a.factor_lr_parts()
        assert a.factor_lr_width == 512 and (a.factor_lr_count, a.dense_factor_count) == (c0, d0)
        dense = _blocks_of(Lb, 512)
        assert [p.shape for p in parts] == [p.shape for p in dense]
        gap = max(float(np.abs(p - q).max()) for p, q in zip(parts, dense))
        print(f"MEASURED n={n}: factor_lr_parts behind a factor at 64 against dense {gap:.2e}")
        assert gap <= 1e-10
        assert all(np.array_equal(p, np.tril(p)) for p in parts)
        # GPIRT_NU_SUB raised on a live sampler: draw_f's product reads 512-wide parts
        f0 = a.get("f")
        a.factor(); a.check()
        assert a.factor_lr_width == 64
        with handle.config("GPIRT_NU_SUB", 512):
            before = a.nu_lr_draws
            a.draw_f(); a.check()
            assert a.nu_lr_draws == before + 1 and a.factor_lr_width == 512
            nu_lr = a.get("nu")
            a.set("f", f0)
            with handle.config("GPIRT_NU_LR", 2):
                a.draw_f(); a.check()
            nu_dense = a.get("nu")
        assert (a.factor_lr_count, a.dense_factor_count) == (c0 + 1, d0 + 1)
        gap = float(np.abs(nu_lr - nu_dense).max())
        print(f"MEASURED n={n}: nu at GPIRT_NU_SUB=512 behind a factor at 64 against the dense product {gap:.2e}")
        assert np.isfinite(nu_lr).all()
        assert gap <= 1e-10 * max(1.0, float(np.abs(nu_dense).max()))
        # get("L") behind a narrow factor: the dense factor, one dense factorisation
        a.set("theta", b.get("theta"))
        a.factor(); a.check()
        assert a.factor_lr_width == 64
        d0 = a.dense_factor_count
        La = np.array(a.get("L"))
        assert a.dense_factor_count == d0 + 1 and a.factor_lr_width == 0
        assert np.array_equal(La, Lb)
        assert np.array_equal(np.array(a.get("L")), La) and a.dense_factor_count == d0 + 1
    a.close(); b.close()


def test_a_first_factor_on_poisoned_allocations(handle):
    import torch
    from gpirt_amd import _lib
    from gpirt_amd.ops import Handle
    lib = _lib.load()
    n = 1088
    out = {}
    for poison in (False, True):
        torch.cuda.synchronize()
        h = Handle()
        try:
            _lib.check(lib.gpirt_debug_poison_allocs(h._h, int(poison)))
            for w in WIDTHS:
                with switches(h, width=w):
                    s = _sampler(h, n)
                    s.init()
                    out[poison, w] = _factored(s)
                    assert s.factor_lr_width == w
                    s.close()
        finally:
            h.close()
    for w in WIDTHS:
        assert all(np.isfinite(p).all() for p in out[True, w][0]) and np.isfinite(out[True, w][1]).all(), w
        assert _same(out[False, w], out[True, w]), w


def test_the_rule(handle):
    assert handle.config_get(NARROW) == 1
    nu_sub = handle.config_get("GPIRT_NU_SUB")
    assert nu_sub == 128
    s = _sampler(handle, 1088)                                   # every switch at its default: dense below n = 2048
    s.init()
    s.factor(); s.check()
    assert s.factor_lr_width == 0 and s.factor_lr_count == 0
    with switches(handle, narrow=1):                             # the state the tests before version 140 run in
        s.factor(); s.check()
        assert s.factor_lr_width == 512
    s.close()
    s = _sampler(handle, 2048)
    s.init()
    assert s.factor_lr_width == 0                                # (init's factor is the dense one)
    s.factor(); s.check()
    assert s.factor_lr_width == nu_sub and s.factor_lr_count == 1
    with handle.config(NARROW, 2):
        s.factor(); s.check()
        assert s.factor_lr_width == 512 and s.factor_lr_count == 2
    s.close()


def test_a_width_outside_the_four_is_refused(handle):
    from gpirt_amd._lib import GpirtError
    s = _sampler(handle, 576)
    s.init()
    default = handle.config_get("GPIRT_NU_SUB")
    with switches(handle):
        for bad in (0, 32, 96, 192, 1024, -64):
            with pytest.raises(GpirtError):
                handle.config_set("GPIRT_NU_SUB", bad)
            assert handle.config_get("GPIRT_NU_SUB") == default
        s.factor(); s.check()
        assert s.factor_lr_width == default
    s.factor(); s.check()                                        # a dense L has no blocks to copy out
    assert s.factor_lr_width == 0
    with pytest.raises(GpirtError):
        s.factor_lr_blocks()
    s.close()
