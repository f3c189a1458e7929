"""What the ordinal fit block costs at the metric size, 8192 x 1024, with the fast options, C = 5 and 10 % missing cells
(csrc/ordinal_fit.hip, gpirt_amd.ordinal.fit_*).

  python tools/ordinal_fit_cost.py --out profiles/ordinal_fit_cost.json
      one ordinal sampler, one process, gpirt_fast_options(), a host clock around work that ends in a synchronise:
      (a) --rounds alternating rounds of --steps iterations (step + draw_thresholds) with ordinal_fit_accumulate after every
          iteration against the same sampler with the block off: iterations per second of each round;
      (b) the accumulate alone, --calls back to back, for each part set, with the bytes each pass moves (counted from the
          shapes) and the rate that implies against the 2.6 TB/s the ACF block's pass reaches.
  python tools/ordinal_fit_cost.py --out ... --headline-this a,b,c --headline-parent a,b,c --headline-flags "..."
      also records bench.py's headline (three alternating runs each on this commit and its parent, as given with the flags
      they were run with: bench.py enables none of this).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PART_SETS = (("waic",), ("pred",), ("ppc",), ("waic", "pred"), ("waic", "ppc"), ("waic", "pred", "ppc"))
ACF_PASS_TB_S = 2.6


def pass_bytes(n, m, C, parts):
    """Bytes one accumulate moves, from the shapes: f and mu (8 each) and cat (1) read once; waic: lse, mean and M2 read and
    written for the observed cells (48, counted for every cell: an upper bound with missing cells); pred: C - 1 sums read and
    written (16 (C - 1)); ppc: the replicate written (1) and the partials (3 doubles and a word per row per strip, 3 doubles, a
    word and 8 counts per item per row block, written, then read by the units kernel)."""
    cells = n * m
    b = 17.0 * cells
    if "waic" in parts:
        b += 48.0 * cells
    if "pred" in parts:
        b += 16.0 * (C - 1) * cells
    if "ppc" in parts:
        strips, rblocks = (m + 31) // 32, (n + 255) // 256
        b += 1.0 * cells + 2.0 * (28.0 * strips * n + 60.0 * rblocks * m)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--categories", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--headline-this", default="")
    ap.add_argument("--headline-parent", default="")
    ap.add_argument("--headline-flags", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from gpirt_amd import Sampler
    from gpirt_amd import ordinal as OR
    from gpirt_amd.ops import Handle
    n, m, C = args.n, args.m, args.categories
    d = OR.make_graded(n, m, C, seed=20240, na_frac=0.1)
    cat = d["cat"]
    h = Handle(0)
    s = Sampler(h, OR.dichotomise(cat), d["theta"], seed=1, preset="fast")
    s.init()
    s.ordinal_enable(cat, C, K0=OR.init_thresholds(cat, OR.grid(), C))

    def iterations(k, fit):
        h.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            s.step()
            s.draw_thresholds()
            if fit:
                s.ordinal_fit_accumulate()
        h.synchronize()
        return k / (time.perf_counter() - t0)

    iterations(args.warmup, False)
    s.ordinal_fit_enable(("waic", "pred", "ppc"))
    iterations(2, True)
    s.ordinal_fit_enable(None)
    rate = {"on": [], "off": []}
    for _ in range(args.rounds):
        for mode in ("on", "off"):
            if mode == "on":
                s.ordinal_fit_enable(("waic", "pred", "ppc"))
            rate[mode].append(iterations(args.steps, mode == "on"))
            if mode == "on":
                s.ordinal_fit_enable(None)
    s.check()
    alone = {}
    for parts in PART_SETS:
        s.ordinal_fit_enable(parts)
        for _ in range(3):
            s.ordinal_fit_accumulate()
        h.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            s.ordinal_fit_accumulate()
        h.synchronize()
        ms = (time.perf_counter() - t0) / args.calls * 1e3
        b = pass_bytes(n, m, C, parts)
        alone["+".join(parts)] = dict(ms_per_call=ms, bytes=b, tb_per_s=b / (ms * 1e-3) / 1e12,
                                      share_of_acf_pass_rate=b / (ms * 1e-3) / 1e12 / ACF_PASS_TB_S)
        s.ordinal_fit_enable(None)
    s.check()
    s.close()
    h.close()
    on, off = statistics.median(rate["on"]), statistics.median(rate["off"])
    out = dict(n=n, m=m, categories=C, missing=float((cat == 0).mean()), steps=args.steps, rounds=args.rounds, calls=args.calls,
               iterations_per_s=dict(fit_on=rate["on"], fit_off=rate["off"], median_on=on, median_off=off,
                                     ms_added_per_iteration=(1.0 / on - 1.0 / off) * 1e3),
               accumulate_alone=alone, acf_pass_tb_per_s=ACF_PASS_TB_S,
               state_bytes_per_cell=dict(waic=24, pred=8 * (C - 1)))
    if args.headline_this or args.headline_parent:
        out["bench_headline_iterations_per_s"] = dict(flags=args.headline_flags,
                                                      this=[float(x) for x in args.headline_this.split(",")],
                                                      parent=[float(x) for x in args.headline_parent.split(",")])
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
