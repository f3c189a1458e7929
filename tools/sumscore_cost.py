"""What the sum-score posteriors (csrc/sumscore.hip) cost at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/sumscore_cost.py --out profiles/sumscore_cost.json [--parent-ms X]
      in one process, interleaved, R rounds of K steps each: the steady step loop with the accumulators off, the same loop
      with them on (the form: all m items) and sumscore_accumulate after each step.  The record holds every
      round's time per iteration, the medians, and the added time per iteration against the plain loop of the same process.
      --parent-ms: the plain loop's median ms per iteration measured with this same tool (its "plain" entry) on the parent
      commit; the record then holds the ratio, which is expected to be 1 within the spread of the rounds.
  The kernels' own durations come from a run of their own (tracing slows the host, so never from the timed one), of any
  script that steps a sampler at this size with sumscore_accumulate after every step:
      rocprofv3 --kernel-trace --stats -d DIR -o ss -- python that_script.py
  and are added to an existing record, together with bench.py's "value" of several runs of the parent commit and of this
  change taken alternately in one session:
      python tools/sumscore_cost.py --record profiles/sumscore_cost.json --kernel-trace DIR/ss_results.db \
             --bench-parent V V V --bench-this V V V --out profiles/sumscore_cost.json
      --record: start from that record and time nothing; --kernel-trace: rocprofv3's database (or its kernel_stats CSV).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("plain", "sumscore")


def kernel_durations(path):
    """median / min / max duration in microseconds and the number of calls of every sumscore_* kernel in a rocprofv3
    --kernel-trace --stats output: its database (the `kernels` view) or its kernel_stats CSV (averages only)"""
    out = {}
    if path.endswith(".csv"):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                if "sumscore_" in row["Name"]:
                    out[_short(row["Name"])] = dict(calls=int(row["Calls"]), mean_us=float(row["AverageNs"]) / 1e3,
                                                    min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3)
        return out
    import sqlite3
    db = sqlite3.connect(path)
    per = {}
    for name, dur in db.execute("select name, duration from kernels where name like '%sumscore_%'"):
        per.setdefault(_short(name), []).append(dur / 1e3)
    for k, v in per.items():
        out[k] = dict(calls=len(v), median_us=statistics.median(v), min_us=min(v), max_us=max(v))
    return out


def _short(name):
    """sumscore_row_kernel<17> out of the demangled signature"""
    at = name.index("sumscore_")
    end = name.index("(", at) if "(" in name[at:] else len(name)
    return name[at:end]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-ms", type=float, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--record", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--bench-parent", type=float, nargs="+", default=None)
    ap.add_argument("--bench-this", type=float, nargs="+", default=None)
    args = ap.parse_args()
    if args.record:
        with open(args.record) as fh:
            rec = json.load(fh)
    else:
        rec = measure(args)
    if args.kernel_trace:
        rec["kernel_us"] = kernel_durations(args.kernel_trace)
        rec["kernel_us_total_median"] = sum(v.get("median_us", v.get("mean_us")) for v in rec["kernel_us"].values())
    if args.bench_parent and args.bench_this:
        rec["bench_iterations_per_s"] = dict(parent=args.bench_parent, this=args.bench_this,
                                             median_parent=statistics.median(args.bench_parent),
                                             median_this=statistics.median(args.bench_this),
                                             spread_parent=max(args.bench_parent) - min(args.bench_parent),
                                             spread_this=max(args.bench_this) - min(args.bench_this))
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


def measure(args):
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
    have_sumscore = hasattr(s, "sumscore_enable")          # (the parent commit has none: its plain loop is all there is to time)
    ms = {k: [] for k in FORMS}
    counts = None
    for _ in range(args.rounds):
        for form in FORMS:
            if form == "sumscore":
                if not have_sumscore:
                    continue
                s.sumscore_enable()
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if form == "sumscore":
                    s.sumscore_accumulate()
            s.check()
            ms[form].append((time.perf_counter() - t0) / args.steps * 1e3)
            if form == "sumscore":
                counts = s.sumscore_get("counts").tolist()
                s.sumscore_enable(on=False)
    s.close()
    h.close()
    med = {k: statistics.median(v) for k, v in ms.items() if v}
    rec = dict(n=args.n, m=args.m, options="gpirt_fast_options", form_items=args.m, rounds=args.rounds,
               steps_per_round=args.steps, ms_per_iteration=ms, median_ms_per_iteration=med,
               spread_ms_plain=max(ms["plain"]) - min(ms["plain"]))
    if "sumscore" in med:
        rec.update(added_ms_per_iteration=med["sumscore"] - med["plain"], ratio_to_plain=med["sumscore"] / med["plain"],
                   last_counts=counts)
    if args.parent_ms is not None:
        rec.update(parent_plain_ms_per_iteration=args.parent_ms, plain_ratio_to_parent=med["plain"] / args.parent_ms)
    return rec


if __name__ == "__main__":
    main()
