"""The normal fill that evaluates AS241's tail branch on a compacted list (csrc/rng_ess.hip item_fill_normal_kernel,
GPIRT_ZFILL_COMPACT=1) against item_fill_kernel (GPIRT_ZFILL_COMPACT=2): every value is qnorm_as241(item_uniform(...)) of its
own index either way, so the two fills are equal bit for bit -- at one element, inside one 1024-element tile, at its edges,
across tiles that straddle items, and at 8192 rows, where a tile lies inside one item and takes the path without a division."""
import numpy as np
import pytest

import _stage_exact as X

pytestmark = pytest.mark.gpu

SWITCH = "GPIRT_ZFILL_COMPACT"
SHAPES = ((1, 1), (63, 3), (1023, 2), (1024, 1), (1025, 5), (8192, 4))
STAGE = X.ST_F_Z


def _tail_key():
    """a (seed, iteration) whose element (item 0, index 0) lies in a tail of AS241, found with the restated generator"""
    for seed in range(1, 200):
        if abs(float(X.item_uniforms(seed, 1, STAGE, 0, 0)) - 0.5) > 0.425:
            return seed, 1
    raise AssertionError("no tail element among 199 seeds")


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("n_index,n_items", SHAPES)
def test_fill_bits(handle, n_index, n_items):
    from gpirt_amd.ops import to_host
    keys = (_tail_key(), (12345, 7)) if (n_index, n_items) == (1, 1) else ((11, 3), (12345, 7))
    for q, (seed, it) in enumerate(keys):
        item0 = 5 * q
        with handle.config(SWITCH, 1):
            new = to_host(handle.item_normals(seed, it, STAGE, item0, n_items, n_index))
        with handle.config(SWITCH, 2):
            old = to_host(handle.item_normals(seed, it, STAGE, item0, n_items, n_index))
        u = to_host(handle.item_uniforms(seed, it, STAGE, item0, n_items, n_index))
        tails = int((np.abs(u - 0.5) > 0.425).sum())
        print(f"MEASURED {n_index} x {n_items} key ({seed}, {it}): {tails} of {u.size} elements on the list")
        assert new.shape == (n_index, n_items) and _same_bits(new, old), np.argwhere(new != old)[:8]
        if q == 0:
            assert tails > 0                                    # the list path ran
        # ... and the values are the generator's: the restatement's, to the last places of the library's log and sqrt
        ref = X.item_normals(seed, it, STAGE, item0 + np.arange(n_items), n_index)
        assert np.abs(new - ref).max() <= 8 * 2.0 ** -52 * max(1.0, np.abs(ref).max())


def _three_steps(handle, switch):
    from gpirt_amd.sampler import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(2048, 8, seed=2048)
    with handle.config(SWITCH, switch):
        s = Sampler(handle, y, th0, rng="item", seed=23)
        s.init()
        for _ in range(3):
            s.step()
        out = tuple(s.get(k) for k in ("theta", "beta", "f", "fstar"))
        s.close()
    return out


def test_sampler_steps_bits(handle):
    new, old = _three_steps(handle, 1), _three_steps(handle, 2)
    for name, a, b in zip(("theta", "beta", "f", "fstar"), new, old):
        assert _same_bits(a, b), (name, int((a != b).sum()))
