"""What the shape posteriors (csrc/shape.hip) cost at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/shape_cost.py --out profiles/shape_cost.json [--parent-ms X]
      in one process, interleaved, R rounds of K steps each: the steady step loop with the accumulators off (draw_fstar's
      epilogue stores no gbar), the same loop with them on and shape_accumulate after each step.  The record holds every
      round's time per iteration, the medians, and the added time per iteration against the plain loop of the same process.
      --parent-ms: the plain loop's median ms per iteration measured with this same tool (its "plain" entry) on the parent
      commit; the record then holds the ratio, which is expected to be 1 within the spread of the rounds.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("plain", "shape")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=3.0)
    ap.add_argument("--parent-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(args.n, args.m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    for _ in range(args.warmup):
        s.step()
    s.check()
    have_shape = hasattr(s, "shape_enable")          # (the parent commit has none: its plain loop is all there is to time)
    ms = {k: [] for k in FORMS}
    counts = None
    for _ in range(args.rounds):
        for form in FORMS:
            if form == "shape":
                if not have_shape:
                    continue
                s.shape_enable(window=args.window)
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if form == "shape":
                    s.shape_accumulate()
            s.check()
            ms[form].append((time.perf_counter() - t0) / args.steps * 1e3)
            if form == "shape":
                counts = s.shape_get("counts").tolist()
                s.shape_enable(on=False)
    s.close()
    h.close()
    med = {k: statistics.median(v) for k, v in ms.items() if v}
    rec = dict(n=args.n, m=args.m, options="gpirt_fast_options", window=args.window, rounds=args.rounds,
               steps_per_round=args.steps, ms_per_iteration=ms, median_ms_per_iteration=med,
               spread_ms_plain=max(ms["plain"]) - min(ms["plain"]))
    if "shape" in med:
        rec.update(added_ms_per_iteration=med["shape"] - med["plain"], ratio_to_plain=med["shape"] / med["plain"],
                   last_counts=counts)
    if args.parent_ms is not None:
        rec.update(parent_plain_ms_per_iteration=args.parent_ms, plain_ratio_to_parent=med["plain"] / args.parent_ms)
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
