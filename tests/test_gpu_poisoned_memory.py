"""Reads of memory nothing wrote (gpirt_debug_poison_allocs).

Fresh device memory usually holds zeros, or whatever the last owner left there: a kernel that reads a buffer nobody wrote can
give the right answer on one run and a different one on the next, and no test that compares numbers sees it.  Here every
configuration runs twice on a fresh Handle with the same seeds -- once as allocated, once with every floating buffer the
sampler allocates and every floating workspace the handle grows filled with 0xFF bytes (a quiet NaN in fp64 and fp32) at
allocation.  Whatever the kernels read must have been written first, so the two runs must agree bit for bit: f, theta, beta,
f*, L, the rejection counts and, under the R stream, the predicted replay's counters (a prediction spoiled by NaN shows there
only: rs_stats[2] counts rounds handed to the one-phase replay).  The clean runs themselves are checked against the oracle
elsewhere (tests/test_gpu_sampler.py, tests/test_gpu_configs.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (name, n, m, Sampler keywords, handle config, iterations)
CASES = [
    ("item_fast_ragged", 1339, 40, dict(rng="item", seed=5, preset="fast"), {}, 3),
    ("item_double_solve", 2600, 12, dict(rng="item", seed=6, fstar_fused=False, kstar_rank=0), {}, 3),
    ("item_fold_n9000", 9000, 6, dict(rng="item", seed=7, preset="fast"), {}, 2),
    ("item_kernel_fp32", 2048, 10, dict(rng="item", seed=8, kernel_fp32=True), {}, 3),
    ("rstream_dense_predictor", 1030, 14, dict(rng="reference"), {}, 3),
    ("rstream_structured_4500", 4500, 21, dict(rng="reference"), {}, 3),
    ("rstream_structured_8192", 8192, 16, dict(rng="reference"), {}, 3),
    ("rstream_one_phase", 1030, 14, dict(rng="reference"), {"GPIRT_RS_PREDICT": 2}, 3),
]


def _run(n, m, kw, cfg, its, poison):
    import torch
    from gpirt_amd import Sampler, _lib
    from gpirt_amd.ops import Handle, RStream
    from gpirt_amd.synthetic import make_responses
    lib = _lib.load()
    y, th0 = make_responses(n, m, seed=3 * n + m)
    torch.cuda.synchronize()
    h = Handle()
    try:
        _lib.check(lib.gpirt_debug_poison_allocs(h._h, int(poison)))
        for name, v in cfg.items():
            h.config_set(name, v)
        kw = dict(kw)
        rs = None
        if kw.get("rng") == "reference":
            rs = RStream(4321)
            kw.update(rstream=rs, theta_stabilise=True)
        s = Sampler(h, y, th0, **kw)
        s.init()
        for _ in range(its):
            s.step()
        s.check()
        out = {k: s.get(k) for k in ("f", "theta", "beta", "fstar", "L", "ess_k")}
        if rs is not None:
            out["rs_stats"] = s.get("rs_stats")
            out["rs_state"] = rs.state()
        s.close()
    finally:
        h.close()
    return out


@pytest.mark.parametrize("name,n,m,kw,cfg,its", CASES, ids=[c[0] for c in CASES])
def test_poisoned_allocations_change_nothing(name, n, m, kw, cfg, its):
    clean = _run(n, m, kw, cfg, its, poison=False)
    dirty = _run(n, m, kw, cfg, its, poison=True)
    if "rs_stats" in clean:
        # [first item not committed, mispredictions, rounds handed to the one-phase replay, predictor passes]
        assert np.array_equal(clean["rs_stats"], dirty["rs_stats"]), (name, "rs_stats clean / poisoned", clean["rs_stats"], dirty["rs_stats"])
        assert clean["rs_stats"][2] == 0, (name, clean["rs_stats"])
        (mt_a, mti_a), (mt_b, mti_b) = clean["rs_state"], dirty["rs_state"]
        assert mti_a == mti_b and np.array_equal(mt_a, mt_b), name
    for k in ("f", "theta", "beta", "fstar", "L", "ess_k"):
        a, b = clean[k], dirty[k]
        assert np.isfinite(a).all(), (name, k)
        assert np.array_equal(a, b, equal_nan=True), (name, k, float(np.nanmax(np.abs(a - b))) if a.dtype.kind == "f" else None)
    print(f"[poisoned allocations, {name}] identical; rs_stats {clean.get('rs_stats')}")
