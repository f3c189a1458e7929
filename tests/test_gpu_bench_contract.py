"""bench.py prints exactly one JSON line carrying the driver's contract fields, the roofline object and the
CPU baseline (small problem so it finishes in seconds)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    # 20 steps behind 5 warm-up steps: at this size the first iterations after a single warm-up step run at ~4 ms instead
    # of the steady ~1.2 ms, and a window of 3 of them timed the transient, not the iteration the default contract's rate
    # is compared with below
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n", "2048", "--m", "128", "--steps", "20",
                          "--warmup", "5"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["dtype"] == "f64" and d["vs_baseline"] is None
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1000.0) < 1.0
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 78.6
    if r["launches"]:
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0 < r["frac"] < 1
    c = d["cpu_baseline"]
    # the headline of cpu_baseline is the MEASURED leg (all host cores, one whole iteration at the full size, nothing
    # extrapolated); the reference-shaped single-thread figure, stretched from samples, is the sub-object
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c and c["extrapolated"] is False
    assert c["single_thread_reference_shaped"]["cores"] == 1 and c["single_thread_reference_shaped"]["extrapolated"] is True
    # what the DEFAULT contract (R-stream replay, everything as written) costs on the same problem, in the same line
    rr = d["config"]["reference_rng"]
    assert "error" not in rr, rr.get("error")             # (a failed default-contract run carries its reason, value None)
    assert rr["iterations"] == 2 and rr["value"] > 0 and d["config"]["reference_rng_iterations_per_s"] == rr["value"]
    assert rr["value"] < d["value"]


def test_bench_two_rank_rehearsal_carries_the_speedup_fields():
    """The first multi-GPU run must be self-contained (round-3 verdict, item 4): with --gpus N > 1 rank 0 also runs the
    FULL problem alone and the line carries item_shard_speedup (per stage and total), whole_iteration_speedup and the
    world size the backend reports.  Rehearsed here with two gloo ranks sharing the one GPU (the numbers mean nothing on
    one card; the fields, the barriers and the order of collectives are what is tested)."""
    port = 29650 + (os.getpid() % 300)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--single-device",
           "--respondents", "2048", "--items", "128", "--steps", "2", "--warmup", "1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["rccl_ranks"] == 2 and d["backend_reported"] == "gloo" and d["scaling"] == "strong"
    sp = d["item_shard_speedup"]
    assert set(sp["per_stage"]) >= {"draw_f", "draw_fstar"} and sp["total"] > 0
    assert sp["single_gpu_stage_ms"]["draw_f"] > 0 and sp["sharded_stage_ms_max_over_ranks"]["draw_f"] > 0
    assert d["whole_iteration_speedup"] > 0 and d["single_gpu_iterations_per_s"] > 0
    assert len(d["config"]["stage_ms_per_rank"]) == 2


def test_bench_dump_outputs_are_reproducible(tmp_path):
    """--dump-outputs DIR: the last timed step's theta, beta, f* and f as float64 .npy files, at most 64 MB in all (f sampled at
    fixed positions once it exceeds the per-array cap), and the same arguments give the same inputs, hence the same outputs."""
    import numpy as np
    lines = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n", "2048", "--m", "1024", "--steps", "2",
                              "--warmup", "1", "--no-cpu-baseline", "--no-reference-rng", "--no-alt-forms",
                              "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        got = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(got) == 1
        lines.append(json.loads(got[0]))
    d = lines[0]
    assert d["steps"] == 2 and abs(d["value"] * d["ms_per_step"] - 1000.0) < 1.0
    arrays = d["dump_outputs"]["arrays"]
    assert set(arrays) == {"theta", "beta", "fstar", "f"}
    assert arrays["theta"]["shape"] == [2048] and arrays["beta"]["shape"] == [2, 1024]
    assert arrays["fstar"]["shape"] == [1001, 1024] and arrays["f"]["shape"] == [2048, 1024]
    assert arrays["f"]["sampled_values"] == 1 << 20 and arrays["fstar"]["sampled_values"] is None
    total = 0
    for name, meta in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and np.all(np.isfinite(a)), name
        want = meta["sampled_values"] or int(np.prod(meta["shape"]))
        assert a.size == want, (name, a.size, want)
        assert np.array_equal(a, b), (name, float(np.abs(a - b).max()))
        total += a.nbytes
    assert total <= 64 << 20
