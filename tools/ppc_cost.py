"""What the posterior predictive checks (csrc/ppc.hip) cost at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/ppc_cost.py --out FILE.json
      in one process, alternating, R rounds of K steps each: the steady step loop, and the same loop + ppc_accumulate.
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/ppc_cost.py --kernel-only
      the replicate kernel (and its two small reductions) alone, 20 launches, for a trace that holds nothing else of note;
  python tools/ppc_cost.py --trace DIR --merge FILE.json
      the kernels' median durations from that trace and the replicate kernel's rate on the bytes it must read: f, mu and
      y once, 3 n m 8 bytes (201 MB at the metric size).  Held against summary_accumulate_kernel's 5.0 TB/s
      (profiles/summary_cost.json) that is about 40 us; "bound" records which side of 2 x 40 us the kernel is on: ten Philox
      rounds, an exp and a log1p per cell and a wave reduction per column can make the pass issue-bound instead.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("ppc_replicate_kernel", "ppc_units_kernel", "ppc_total_kernel")
SUMMARY_TB_PER_S = 5.0           # summary_accumulate_kernel, profiles/summary_cost.json


def sampler(n, m):
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    s.check()
    return h, s


def timing(args):
    n, m = args.n, args.m
    h, s = sampler(n, m)
    s.ppc_enable()
    for _ in range(args.warmup):
        s.step()
    s.check()
    rates = {"plain": [], "ppc": []}
    for _ in range(args.rounds):
        for form in rates:
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if form == "ppc":
                    s.ppc_accumulate()
            s.check()
            rates[form].append(args.steps / (time.perf_counter() - t0))
    tot = s.ppc_totals()
    s.close()
    h.close()
    med = {k: statistics.median(v) for k, v in rates.items()}
    return dict(n=n, m=m, options="gpirt_fast_options", rounds=args.rounds, steps_per_round=args.steps,
                iterations_per_s=rates, median_iterations_per_s=med, ratio_to_plain={"ppc": med["ppc"] / med["plain"]},
                totals=tot)


def kernel_only(args):
    h, s = sampler(args.n, args.m)
    s.step()
    s.ppc_enable()
    for _ in range(args.launches):
        s.ppc_accumulate()
    s.check()
    s.close()
    h.close()


def from_trace(args):
    f = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    out = {}
    for name in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if not us:
            raise SystemExit(f"no {name} in {f}")
        out[name] = dict(launches=len(us), median_us=statistics.median(us), min_us=min(us))
    b = 3.0 * args.n * args.m * 8.0
    med = out["ppc_replicate_kernel"]["median_us"]
    floor_us = b / (SUMMARY_TB_PER_S * 1e12) * 1e6
    out["ppc_replicate_kernel"].update(bytes_read=b, tb_per_s=b / (med * 1e-6) / 1e12,
                                       fraction_of_6_3_tb_per_s=b / (med * 1e-6) / 6.3e12,
                                       us_at_summary_kernel_rate=floor_us, ratio_to_that=med / floor_us,
                                       bound="memory" if med <= 2.0 * floor_us else "issue")
    out["per_draw_us"] = sum(out[k]["median_us"] for k in KERNELS)
    rec = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
    rec["kernels"] = out
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_only:
        kernel_only(args)
        return
    rec = from_trace(args) if args.trace else timing(args)
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    out = args.out or args.merge
    if out:
        with open(out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
