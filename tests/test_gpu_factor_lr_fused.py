"""The structured factor's fused rounds (gpirt_amd/csrc/factor_lr.hip): GPIRT_FLR_FUSE = 1, the default,
runs one launch per 64-column round -- each round's update rides in the next round's launch, the pivot tile has no owner, the
diagonal is placed one launch late -- and = 2 runs the launches of library version 131.  Both add the same numbers in the same
order, so everything here is np.array_equal, on the same sampler state.  m = 8, the three structured switches at 3 as in
tests/test_gpu_factor_lr.py (the small sizes are not eligible otherwise)."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FAST = dict(rng="item", fstar_fused=True, kstar_rank=64, theta_stabilise=True)
M = 8
FUSE = "GPIRT_FLR_FUSE"
SWITCHES = ("GPIRT_FACTOR_LR", "GPIRT_NU_LR", "GPIRT_FSTAR_FREE")
KINDS = ["grid_normal", "grid_uniform", "off_grid", "sorted", "all_equal", "half_minus5_half_plus5", "two_points_0.01_apart"]


def theta_case(kind, n):
    rng = np.random.default_rng(2000 + n)
    g = -5.0 + np.arange(1001, dtype=np.float64) * 0.01
    normal = lambda: g[np.clip(np.rint((rng.standard_normal(n) + 5.0) / 0.01).astype(int), 0, 1000)]
    return {"grid_normal": normal, "grid_uniform": lambda: g[rng.integers(0, 1001, n)], "off_grid": lambda: rng.uniform(-5.0, 5.0, n),
            "sorted": lambda: np.sort(normal()), "all_equal": lambda: np.full(n, g[617]),
            "half_minus5_half_plus5": lambda: np.where(np.arange(n) < n // 2, -5.0, 5.0),
            "two_points_0.01_apart": lambda: np.where(np.arange(n) % 2 == 0, g[400], g[401])}[kind]()


@contextlib.contextmanager
def eligible_at_every_n(handle):
    with contextlib.ExitStack() as st:
        for k in SWITCHES:
            st.enter_context(handle.config(k, 3))
        yield


def _sampler(handle, n, m=M, seed=17, **kw):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=311 + n)
    return Sampler(handle, y, th0, seed=seed, **dict(FAST, factor_structured=True, **kw))


def _factored(handle, s, fuse, theta=None):
    """(parts, node rows) of one structured factorisation of s under GPIRT_FLR_FUSE = fuse"""
    if theta is not None:
        s.set("theta", theta)
    before = s.factor_lr_count
    with handle.config(FUSE, fuse):
        s.factor()
        s.check()
    assert s.factor_lr_count == before + 1
    return s.factor_lr_parts(), np.array(s.nu_lr_rows())


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(np.array_equal(p, q) for p, q in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


# 64: one block, one round; 128; 512: one full part; 576: a full part and one block; 960: seven blocks behind a full part; 1088; 1536
@pytest.mark.parametrize("n", [64, 128, 512, 576, 960, 1088, 1536])
def test_parts_and_node_rows_equal_the_unfused_launches(handle, n):
    assert handle.config_get(FUSE) == 1
    s = _sampler(handle, n)
    s.init()
    with eligible_at_every_n(handle):
        for kind in KINDS:
            s.set("theta", theta_case(kind, n))
            fused = _factored(handle, s, 1)
            plain = _factored(handle, s, 2)
            assert [p.shape for p in fused[0]] == [(min(512, n - p0),) * 2 for p0 in range(0, n, 512)]
            gap_parts = max(float(np.abs(a - b).max()) for a, b in zip(fused[0], plain[0]))
            gap_rows = float(np.abs(fused[1] - plain[1]).max())
            print(f"MEASURED {kind} n={n}: fused against unfused, parts {gap_parts:.2e}, node rows {gap_rows:.2e}")
            for a in fused[0]:
                assert np.array_equal(a, np.tril(a)), "strict upper triangle inside a part"
            assert all(np.array_equal(a, b) for a, b in zip(fused[0], plain[0])), kind
            assert np.array_equal(fused[1], plain[1]), kind
    s.close()


@pytest.mark.parametrize("n", [576, 1088])
def test_nothing_is_carried_from_one_factorisation_to_the_next(handle, n):
    """A pivot tile placed one launch late, or a slot of the pivot workspace, must not survive into the next factorisation:
    theta_1 then theta_2 on one sampler gives what a fresh sampler gives at theta_2.  At 576 a 512-row sampler of the same
    handle is factored first (one full part, then a full part and a block)."""
    th1, th2 = theta_case("grid_normal", n), theta_case("off_grid", n)
    with eligible_at_every_n(handle):
        if n == 576:
            small = _sampler(handle, 512)
            small.init()
            _factored(handle, small, 1, theta_case("sorted", 512))
            small.close()
        a = _sampler(handle, n)
        a.init()
        _factored(handle, a, 1, th1)
        twice = _factored(handle, a, 1, th2)
        b = _sampler(handle, n)
        b.init()
        fresh = _factored(handle, b, 1, th2)
        assert _same(twice, fresh)
        assert _same(twice, _factored(handle, b, 2, th2))
        # ... and in the other order of the two schedules on one sampler
        _factored(handle, a, 2, th1)
        assert _same(_factored(handle, a, 1, th2), fresh)
    a.close(); b.close()


def test_three_whole_steps_and_item_shards_equal_the_unfused_launches(handle):
    n = 1088
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    a, b = _sampler(handle, n), _sampler(handle, n)
    with eligible_at_every_n(handle):
        for c in (a, b):
            c.init()
        for it in range(3):
            for c, fuse in ((a, 1), (b, 2)):
                with handle.config(FUSE, fuse):
                    c.step()
                    c.check()
            for key in ("theta", "ess_k", "f", "fstar"):
                assert np.array_equal(a.get(key), b.get(key)), (it, key)
        assert (a.factor_lr_count, b.factor_lr_count) == (3, 3)
        a.close(); b.close()
        # two item shards of 4 columns under the fused rounds: the full sampler's bits, fused or not
        y, th0 = make_responses(n, M, seed=5)
        kw = dict(FAST, factor_structured=True)
        full = Sampler(handle, y, th0, seed=5, **kw)
        shards = [Sampler(handle, y[:, j0:j0 + 4], th0, seed=5, item0=j0, m_total=M, **kw) for j0 in (0, 4)]
        full.init()
        for j0, c in zip((0, 4), shards):
            c.init()
            for k in ("f", "mu", "beta"):
                c.set(k, full.get(k)[:, j0:j0 + 4])
        plain = _factored(handle, full, 2)
        it1 = full.iteration
        fused = _factored(handle, full, 1)
        full.set_iteration(it1)                                  # (draw_f's normals are keyed by the iteration: the shards' one)
        assert _same(fused, plain)
        full.draw_f(); full.check()
        for j0, c in zip((0, 4), shards):
            assert _same(_factored(handle, c, 1), fused), j0
            c.draw_f(); c.check()
            assert np.array_equal(c.get("f"), full.get("f")[:, j0:j0 + 4]), j0
        full.close()
        for c in shards:
            c.close()
