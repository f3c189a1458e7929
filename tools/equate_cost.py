"""What the two-form score equating (csrc/equate.hip) costs at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/equate_cost.py --out profiles/equate_cost.json [--parent-ms X]
      in one process, interleaved, R rounds of K steps each: the steady step loop with the accumulators off ("plain"), the
      same loop with equate_accumulate after each step for M_X = M_Y = 512 (the two halves of the items, interleaved:
      "half") and for M_X = 1024 - rest, M_Y = rest ("long", --rest items in form Y).  The record holds every round's time per
      iteration, the medians and the added time per iteration against the plain loop of the same process; beside them the
      figures of profiles/sumscore_cost.json, if that file is there: the work is two recursions plus one product.
      --parent-ms: the plain loop's median ms per iteration measured with tools/sumscore_cost.py (its "plain" entry) on the
      parent commit; the record then holds the ratio, which is expected to be 1 within the spread of the rounds.
Nothing here gates: the record reports.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--rest", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = measure(args)
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


def measure(args):
    import numpy as np
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(args.n, args.m, seed=20240)
    m = y.shape[1]
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    for _ in range(args.warmup):
        s.step()
    s.check()
    cols = np.arange(m)
    forms = dict(plain=None, half=(cols[0::2], cols[1::2]), long=(cols[:m - args.rest], cols[m - args.rest:]))
    ms = {k: [] for k in forms}
    counts = {}
    for _ in range(args.rounds):
        for form, xy in forms.items():
            if xy is not None:
                s.equate_enable(*xy)
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if xy is not None:
                    s.equate_accumulate()
            s.check()
            ms[form].append((time.perf_counter() - t0) / args.steps * 1e3)
            if xy is not None:
                counts[form] = s.equate_get("counts").tolist()
                s.equate_enable(on=False)
    s.close()
    h.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    rec = dict(n=args.n, m=m, options="gpirt_fast_options", forms={k: [len(v[0]), len(v[1])] for k, v in forms.items() if v},
               rounds=args.rounds, steps_per_round=args.steps, ms_per_iteration=ms, median_ms_per_iteration=med,
               spread_ms_plain=max(ms["plain"]) - min(ms["plain"]),
               added_ms_per_iteration={k: med[k] - med["plain"] for k in forms if k != "plain"},
               ratio_to_plain={k: med[k] / med["plain"] for k in forms if k != "plain"}, last_counts=counts)
    if args.parent_ms is not None:
        rec.update(parent_plain_ms_per_iteration=args.parent_ms, plain_ratio_to_parent=med["plain"] / args.parent_ms)
    ss = os.path.join(ROOT, "profiles", "sumscore_cost.json")
    if os.path.exists(ss):
        with open(ss) as fh:
            old = json.load(fh)
        rec["sumscore_cost"] = {k: old[k] for k in ("form_items", "median_ms_per_iteration", "added_ms_per_iteration") if k in old}
    return rec


if __name__ == "__main__":
    main()
