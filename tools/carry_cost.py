"""What the consistent step costs at the metric size, 8192 x 1024, with the fast options, and what it does to the prior
quadratic form (csrc/carry.hip, gpirt_amd.consistent).

  python tools/carry_cost.py --out profiles/carry_cost.json
      one sampler, one process, gpirt_fast_options().
      (a) carry_f_kernel's device time by the sampler's event timing (Sampler.enable_timing, carry_stats()["time_ms"]), --calls
          calls with the nugget and --calls without, and the bytes it moves (n m doubles stored, theta read; the two gathers stay
          in cache).  The yardstick is item_fill_kernel producing the n x m normals of draw_f in the same run, the two taken in
          turn (device events around Handle.item_normals): the same Philox + AS241 work per value, the same bytes written.
      (b) iterations/s of step(consistent=True) against step(): --rounds rounds of --steps steps each, the two taken in turn,
          check() closing each.
      (c) Q, the mean over items of Sampler.prior_quad(), every --q-every steps of a chain of --q-steps steps under step() and
          under the consistent step, at --q-sizes (2048x256 and 8192x1024): each from a fresh sampler with the same seed.
  python tools/carry_cost.py --out profiles/carry_cost.json --headline-this 154.1,154.2,154.3 --headline-parent 154.0,154.2,154.4
      also records bench.py's headline (iterations/s of `bench.py --gpus 1`), three alternating runs each on this commit and on
      its parent in one session, as given: bench.py enables none of this
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def q_series(handle, n, m, steps, every, consistent, seed=1):
    """Q = prior_quad().mean() after every `every`-th step of a fresh fast-preset chain"""
    from gpirt_amd import Sampler
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=20240)
    s = Sampler(handle, y, th0, seed=seed, preset="fast")
    s.init()
    out = []
    for it in range(1, steps + 1):
        s.step(consistent=consistent)
        if it % every == 0:
            out.append(dict(step=it, Q=float(s.prior_quad().mean())))
    s.check()
    st = s.carry_stats()
    s.close()
    return dict(series=out, off_grid=st["total_off_grid"], nonfinite=st["total_nonfinite"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--q-steps", type=int, default=300)
    ap.add_argument("--q-every", type=int, default=50)
    ap.add_argument("--q-sizes", default="2048x256,8192x1024")
    ap.add_argument("--headline-this", default=None)
    ap.add_argument("--headline-parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from gpirt_amd import Sampler, _lib
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    n, m = args.n, args.m
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, seed=1, preset="fast")
    s.init()
    for _ in range(args.warmup):
        s.step(consistent=True)
    s.check()
    # (b) the step loop, the consistent step against the reference's
    rates = {"consistent": [], "reference": []}
    for _ in range(args.rounds):
        for name in ("consistent", "reference"):
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step(consistent=(name == "consistent"))
            s.check()
            rates[name].append(args.steps / (time.perf_counter() - t0))
    # the carry's share of a consistent step, by the sampler's events
    s.enable_timing(True)
    stage = {}
    for _ in range(10):
        s.step(consistent=True)
        for k, v in s.stage_times().items():
            stage.setdefault(k, []).append(v)
    # (a) the kernel against the yardstick, in turn
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {"carry_nugget": [], "carry_smooth": [], "item_fill": []}
    for c in range(args.calls + 3):
        s.carry_f(True)
        a = s.carry_stats()["time_ms"]
        s.carry_f(False)
        b = s.carry_stats()["time_ms"]
        e0.record(h.stream)
        z = h.item_normals(1, 1 + c, _lib.ST_F_Z, 0, m, n)
        e1.record(h.stream)
        e1.synchronize()
        del z
        if c >= 3:
            ms["carry_nugget"].append(a)
            ms["carry_smooth"].append(b)
            ms["item_fill"].append(e0.elapsed_time(e1))
    s.enable_timing(False)
    s.check()
    st = s.carry_stats()
    s.close()
    nm8 = 8.0 * n * m

    def row(v, moved):
        t = statistics.median(v)
        return dict(calls=len(v), ms=t, ms_min=min(v), ms_max=max(v), bytes=moved, tb_per_s=moved / (t * 1e-3) / 1e12)

    kernel = dict(carry_nugget=row(ms["carry_nugget"], nm8 + 8.0 * n), carry_smooth=row(ms["carry_smooth"], nm8 + 8.0 * n),
                  item_fill=row(ms["item_fill"], nm8))
    kernel["ratio_to_item_fill"] = kernel["carry_nugget"]["ms"] / kernel["item_fill"]["ms"]
    rec = dict(n=n, m=m, steps=args.steps, rounds=args.rounds, iterations_per_s=rates,
               median_iterations_per_s={k: statistics.median(v) for k, v in rates.items()},
               stage_ms={k: statistics.median(v) for k, v in stage.items()}, kernel=kernel,
               carry_counters=dict(calls=st["calls"], total_off_grid=st["total_off_grid"], total_nonfinite=st["total_nonfinite"]),
               prior_quad={})
    # (c) Q along a chain, per size and step
    for size in [v for v in args.q_sizes.split(",") if v]:
        qn, qm = (int(v) for v in size.split("x"))
        rec["prior_quad"][size] = dict(every=args.q_every, steps=args.q_steps,
                                       reference=q_series(h, qn, qm, args.q_steps, args.q_every, False),
                                       consistent=q_series(h, qn, qm, args.q_steps, args.q_every, True))
        print(size, json.dumps(rec["prior_quad"][size], default=float), flush=True)
    h.close()
    if args.headline_this and args.headline_parent:
        rec["headline"] = dict(this=[float(v) for v in args.headline_this.split(",")],
                               parent=[float(v) for v in args.headline_parent.split(",")])
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
