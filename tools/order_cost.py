"""What the item-pair order posteriors (csrc/order.hip) cost at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/order_cost.py --out profiles/order_cost.json [--parent-ms X]
      in one process, interleaved, R rounds of K steps each: the steady step loop with the shape accumulators alone
      (shape_accumulate after each step), the same loop with the order block on, and the accumulation alone on a fixed gbar
      (K calls of shape_accumulate between two synchronisations) with and without the order block: their difference is the
      time of the order block's three kernels, of which the pair kernel is all but the easiness kernel's m small work-groups
      and the one-work-group finish.  The record holds every round's time, the medians, the added time per iteration and the
      kernels' time as a share of the parent commit's iteration (--parent-ms, 6.4 ms by default: the recorded figure).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("shape", "order")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=float, default=3.0)
    ap.add_argument("--parent-ms", type=float, default=6.4)
    ap.add_argument("--note", default=None)
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
    loop = {k: [] for k in FORMS}
    acc = {k: [] for k in FORMS}
    counts = None
    for _ in range(args.rounds):
        for form in FORMS:
            s.shape_enable(window=args.window)
            if form == "order":
                s.shape_order_enable()
            s.step()                                     # gbar holds a curve; the kernels' first launch is outside the window
            s.shape_accumulate()
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                s.shape_accumulate()
            s.check()
            loop[form].append((time.perf_counter() - t0) / args.steps * 1e3)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.shape_accumulate()
            s.check()
            acc[form].append((time.perf_counter() - t0) / args.steps * 1e3)
            if form == "order":
                counts = s.shape_order_get("counts").tolist()
            s.shape_enable(on=False)
    s.close()
    h.close()
    med_loop = {k: statistics.median(v) for k, v in loop.items()}
    med_acc = {k: statistics.median(v) for k, v in acc.items()}
    k_half = int(round(100 * args.window))
    pairs = args.m * (args.m + 1) // 2
    kernels_ms = med_acc["order"] - med_acc["shape"]
    rec = dict(n=args.n, m=args.m, options="gpirt_fast_options", window=args.window, rounds=args.rounds,
               steps_per_round=args.steps, loop_ms_per_iteration=loop, accumulate_ms_per_call=acc,
               median_loop_ms_per_iteration=med_loop, median_accumulate_ms_per_call=med_acc,
               spread_ms_shape_loop=max(loop["shape"]) - min(loop["shape"]),
               added_ms_per_iteration=med_loop["order"] - med_loop["shape"],
               loop_ratio_to_shape_alone=med_loop["order"] / med_loop["shape"],
               order_kernels_ms_per_draw=kernels_ms,
               fp64_vector_operations_per_draw=3 * pairs * (2 * k_half + 1),
               parent_ms_per_iteration=args.parent_ms, order_kernels_share_of_parent_iteration=kernels_ms / args.parent_ms,
               last_counts=counts)
    if args.note:
        rec["note"] = args.note
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
