"""What the covariance kernel's families cost at the metric size, 8192 x 1024 (csrc/se_kernel.hip, gpirt_amd.kernel).

  python tools/kernel_cost.py --out profiles/kernel_cost.json
      in one process: (1) the lower build S = K(theta, theta) + 0.001 I per family -- Sampler.build_cov() under GPIRT_BORDERED=2,
      so that the launch is the lower builder alone --, event-timed over batches of --launches builds, --rounds rounds with the
      families taken in turn; "default" is the reference's kernel in its own instantiation, "se" the squared exponential at
      length scale 0.7.  The kernel is HBM-write bound: bytes = 8 x the lower block triangle.  (2) iterations/s
      of the steady step loop under Matern 5/2 (fstar_fused, no rank form: a Matern kernel has none) beside the default kernel
      with the fast preset (rank 64), --steps steps a round, alternating.
  python tools/kernel_cost.py --families default --no-chain
      the lower build of the default kernel alone: runs on a library without gpirt_kernel_set too (a parent commit's, for the
      comparison in one session).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"default": None, "se": dict(family="se", length_scale=0.7), "matern52": dict(family="matern52", length_scale=0.7),
           "matern32": dict(family="matern32", length_scale=0.7)}


def lower_bytes(n):
    nb = (n + 127) // 128
    return 8.0 * 128 * 128 * nb * (nb + 1) / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--families", default="default,se,matern52,matern32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    n, m = args.n, args.m
    names = [f for f in args.families.split(",") if f]
    y, th0 = make_responses(n, 8, seed=20240)
    handles, samplers = {}, {}
    for name in names:
        h = Handle(0)
        if KERNELS[name] is not None:
            h.set_kernel(KERNELS[name])
        h.config_set("GPIRT_BORDERED", 2)
        s = Sampler(h, y, th0, rng="item", seed=1, theta_stabilise=True, fstar_fused=True)
        s.init()
        s.check()
        handles[name], samplers[name] = h, s
    us = {name: [] for name in names}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(args.rounds + 1):                     # round 0 warms up
        for name in names:
            s = samplers[name]
            s.check()
            e0.record()
            for _ in range(args.launches):
                s.build_cov()
            e1.record()
            e1.synchronize()
            if rnd:
                us[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    for name in names:
        samplers[name].close()
        handles[name].close()
    b = lower_bytes(n)
    build = {name: dict(us_per_build=v, median_us=statistics.median(v), min_us=min(v), max_us=max(v),
                        tb_per_s=b / (statistics.median(v) * 1e-6) / 1e12) for name, v in us.items()}
    rec = dict(n=n, m=m, launches=args.launches, rounds=args.rounds, lower_bytes=b, kernels={k: KERNELS[k] for k in names},
               lower_build=build)
    if not args.no_chain:
        y, th0 = make_responses(n, m, seed=20240)
        forms = {"default_fast_rank64": (None, dict(preset="fast")),
                 "matern52_fused_rank0": (KERNELS["matern52"], dict(rng="item", theta_stabilise=True, fstar_fused=True)),
                 "default_fused_rank0": (None, dict(rng="item", theta_stabilise=True, fstar_fused=True))}
        rates = {k: [] for k in forms}
        live = {}
        for k, (kern, kw) in forms.items():
            h = Handle(0, kernel=kern)
            s = Sampler(h, y, th0, seed=1, **kw)
            s.init()
            for _ in range(args.warmup):
                s.step()
            s.check()
            live[k] = (h, s)
        for _ in range(5):
            for k, (h, s) in live.items():
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    s.step()
                s.check()
                rates[k].append(args.steps / (time.perf_counter() - t0))
        for h, s in live.values():
            s.close()
            h.close()
        rec["iterations_per_s"] = rates
        rec["median_iterations_per_s"] = {k: statistics.median(v) for k, v in rates.items()}
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
