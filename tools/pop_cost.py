"""What the population prior for theta costs at the metric size, 8192 x 1024, with the fast options (csrc/pop.hip,
csrc/stages.hip theta_sample_kernel<true>, gpirt_amd.pop).

  python tools/pop_cost.py --out profiles/pop_cost.json
      one sampler, one process, gpirt_fast_options(), G = 2 and G = 8 (respondent i in group i mod G).
      (a) theta_finish with a table on against off, by the sampler's stage events (Sampler.enable_timing, stage_times()
          ["theta_sample"]): --rounds rounds of --steps steps each, the two taken in turn on the same sampler (pop_set with every
          row the default row, so that the chain is the same chain, then pop_set(None)).  The table adds one read per grid point
          from a row that the whole device shares (G x 8 KB: it stays in cache).
      (b) one draw_pop, by device events around its two launches (pop_get("time")), --calls calls on a chain that steps in
          between, on the default 121 x 65 grids, and the bytes it has to move: n theta values and n codes read once, plus per
          group g >= 1 one column and one row of lse and the two hyperprior rows ((P_mu + P_sd) x 16 bytes) and the 8 KB row
          written.
  python tools/pop_cost.py --out profiles/pop_cost.json --headline-this 808.1,808.2,808.3 --headline-parent 808.0,808.2,808.4
      also records bench.py's headline (iterations/s of `bench.py --gpus 1`), three alternating runs each on this commit and on
      its parent in one session, as given: bench.py enables none of this
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--groups", default="2,8")
    ap.add_argument("--headline-this", default=None)
    ap.add_argument("--headline-parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    from gpirt_amd import Sampler, pop as PO
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    n, m = args.n, args.m
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    rec = dict(n=n, m=m, steps=args.steps, rounds=args.rounds, groups={})
    for G in [int(v) for v in args.groups.split(",") if v]:
        codes = (np.arange(n) % G).astype(np.int32)
        table = np.tile(PO.default_row(), (G, 1))
        s = Sampler(h, y, th0, seed=1, preset="fast")
        s.init()
        for _ in range(args.warmup):
            s.step()
        s.check()
        s.enable_timing(True)
        ms = {"off": [], "on": []}
        for _ in range(args.rounds):
            for name in ("off", "on"):
                s.pop_set(codes, table) if name == "on" else s.pop_set(None)
                for _ in range(args.steps):
                    s.step()
                    ms[name].append(s.stage_times()["theta_sample"])
        s.pop_set(None)
        s.check()
        # (b) draw_pop on the default grids, the chain stepping in between
        s.pop_enable(codes, G, planned_draws=0)
        P_mu, P_sd = s.pop_stats()["points_mu"], s.pop_stats()["points_sd"]
        calls = []
        for c in range(args.calls + 3):
            s.step()
            s.draw_pop()
            if c >= 3:
                calls.append(float(s.pop_get("time")[0]))
        st = s.pop_stats()
        s.enable_timing(False)
        s.check()
        s.close()
        moved = 8.0 * n + 4.0 * n + (G - 1) * ((P_mu + P_sd) * 16.0 + 8.0 * 1001)
        t = statistics.median(calls)
        rec["groups"][str(G)] = dict(
            theta_sample_ms={k: dict(steps=len(v), median=statistics.median(v), min=min(v), max=max(v)) for k, v in ms.items()},
            theta_sample_ratio=statistics.median(ms["on"]) / statistics.median(ms["off"]),
            draw_pop=dict(calls=len(calls), points_mu=P_mu, points_sd=P_sd, ms=t, ms_min=min(calls), ms_max=max(calls), bytes=moved,
                          gb_per_s=moved / (t * 1e-3) / 1e9, updated=st["updated"], skipped=st["skipped"], failed=st["failed"]))
        print(G, json.dumps(rec["groups"][str(G)], default=float), flush=True)
    h.close()
    if args.headline_this and args.headline_parent:
        rec["headline"] = dict(this=[float(v) for v in args.headline_this.split(",")],
                               parent=[float(v) for v in args.headline_parent.split(",")],
                               bench_args="--gpus 1 --steps 300 --warmup 30")
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
