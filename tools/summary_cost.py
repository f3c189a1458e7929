"""What the posterior summaries (csrc/summary.hip) cost at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/summary_cost.py --out FILE.json
      in one process, alternating, R rounds of K steps each: the steady step loop; the same loop + summary_accumulate with
      WAIC + pred; the same with f's moments too.  Then gpirt_mcmc_summary over 200 samples with no draws stored: its wall
      time and the process's peak resident memory against what the f draws alone would take.
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/summary_cost.py --kernel-only
      the accumulate kernel alone, both forms, 20 launches each, for a trace that holds nothing else of note;
  python tools/summary_cost.py --trace DIR --merge FILE.json
      the kernel's median duration from that trace and its rate on the algorithmic bytes: f, mu, y read once, each
      accumulator read and written once (WAIC: 3, pred: 1, f: 2), theta and beta with their two moments.
"""
import argparse
import csv
import glob
import json
import os
import resource
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = {"waic_pred": ("waic", "pred"), "waic_pred_f": ("waic", "pred", "f")}
TEMPLATE = {"waic_pred": "summary_accumulate_kernel<true, true, false>", "waic_pred_f": "summary_accumulate_kernel<true, true, true>"}
ACCUMULATORS = {"waic_pred": 4, "waic_pred_f": 6}


def algorithmic_bytes(form, n, m):
    cells = n * m
    return 8.0 * (3 * cells + 2 * ACCUMULATORS[form] * cells + 3 * (n + 2 * m))


def sampler(n, m):
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    s.check()
    return h, s, y, th0


def timing(args):
    n, m = args.n, args.m
    h, s, y, th0 = sampler(n, m)
    for _ in range(args.warmup):
        s.step()
    s.check()
    rates = {"plain": [], "waic_pred": [], "waic_pred_f": []}
    for _ in range(args.rounds):
        for form in rates:
            s.summary_enable(FORMS.get(form, 0))
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if form != "plain":
                    s.summary_accumulate()
            s.check()
            rates[form].append(args.steps / (time.perf_counter() - t0))
    s.summary_enable(0)
    s.close()
    h.close()
    med = {k: statistics.median(v) for k, v in rates.items()}
    rec = dict(n=n, m=m, options="gpirt_fast_options", rounds=args.rounds, steps_per_round=args.steps,
               iterations_per_s={k: v for k, v in rates.items()}, median_iterations_per_s=med,
               ratio_to_plain={k: med[k] / med["plain"] for k in FORMS})
    # the whole call, 200 samples, nothing stored but the summaries
    from gpirt_amd import gpirtMCMC
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    t0 = time.perf_counter()
    res = gpirtMCMC(y, args.samples, 1, vote_codes=dict(yea=[1], nay=[-1], missing=[None]), theta_init=th0, preset="fast",
                    seed=1, summaries=("waic", "pred"), store_draws=False)
    wall = time.perf_counter() - t0
    rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    tot = res["summary"]["totals"]
    rec["mcmc_summary"] = dict(samples=args.samples, burn=1, wall_s=wall, iterations_per_s=(args.samples + 1) / wall,
                               peak_rss_bytes_before=rss0, peak_rss_bytes_after=rss1,
                               f_draws_bytes_if_stored=8.0 * n * m * (args.samples + 1), totals=tot)
    return rec


def kernel_only(args):
    h, s, _, _ = sampler(args.n, args.m)
    s.step()
    for form, parts in FORMS.items():
        s.summary_enable(parts)
        for _ in range(args.launches):
            s.summary_accumulate()
        s.check()
    s.summary_enable(0)
    s.close()
    h.close()


def from_trace(args):
    f = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    out = {}
    for form, name in TEMPLATE.items():
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if not us:
            raise SystemExit(f"no {name} in {f}")
        med = statistics.median(us)
        b = algorithmic_bytes(form, args.n, args.m)
        out[form] = dict(launches=len(us), median_us=med, min_us=min(us), algorithmic_bytes=b,
                         tb_per_s=b / (med * 1e-6) / 1e12, fraction_of_6_3_tb_per_s=b / (med * 1e-6) / 6.3e12)
    rec = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
    rec["accumulate_kernel"] = out
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=200)
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
