"""What the rank posteriors (csrc/ranks.hip) cost at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/rank_cost.py --out FILE.json
      in one process, alternating, R rounds of K steps each: the steady step loop, the same loop + rank_accumulate
      without the pairwise counters, and with them.  The number to record is the added time per iteration against the
      plain loop of the same process.
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/rank_cost.py --kernel-only
      a few steps with summary_accumulate and rank_accumulate (pairwise on) after each, then 20 more rank_accumulate
      launches: a trace that holds both rank kernels and summary_accumulate_kernel;
  python tools/rank_cost.py --trace DIR --merge FILE.json
      the two kernels' median durations from that trace, and the pairwise kernel's rate on the 8 n ld bytes it moves
      (one 4-byte counter read and written per pair; 537 MB at n = 8192) beside summary_accumulate_kernel's median in the
      same trace and the 5.0 TB/s profiles/summary_cost.json holds for it.
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

KERNELS = ("rank_accumulate_kernel", "rank_pairwise_kernel")
SUMMARY_TB_PER_S = 5.0           # summary_accumulate_kernel, profiles/summary_cost.json
FORMS = ("plain", "ranks", "ranks_pairwise")


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
    for _ in range(args.warmup):
        s.step()
    s.check()
    rates = {k: [] for k in FORMS}
    for _ in range(args.rounds):
        for form in FORMS:
            if form != "plain":
                s.rank_enable(pairwise=form == "ranks_pairwise")
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if form != "plain":
                    s.rank_accumulate()
            s.check()
            rates[form].append(args.steps / (time.perf_counter() - t0))
            if form != "plain":
                counts = s.rank_get("counts").tolist()
                s.rank_enable(on=False)
    s.close()
    h.close()
    med = {k: statistics.median(v) for k, v in rates.items()}
    added = {k: (1.0 / med[k] - 1.0 / med["plain"]) * 1e3 for k in FORMS[1:]}
    return dict(n=n, m=m, options="gpirt_fast_options", rounds=args.rounds, steps_per_round=args.steps,
                iterations_per_s=rates, median_iterations_per_s=med, added_ms_per_iteration=added,
                ratio_to_plain={k: med[k] / med["plain"] for k in FORMS[1:]}, last_counts=counts)


def kernel_only(args):
    h, s = sampler(args.n, args.m)
    s.summary_enable(("waic",))
    s.rank_enable(pairwise=True)
    for _ in range(3):
        s.step()
        s.summary_accumulate()
        s.rank_accumulate()
    for _ in range(args.launches):
        s.rank_accumulate()
    s.check()
    s.close()
    h.close()


def from_trace(args):
    f = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(f)))

    def durations(name):
        # "summary_accumulate_kernel" must not pick up summary_diag_accumulate_kernel or summary_hist_accumulate_kernel
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows
                if name + "<" in r["Kernel_Name"] or name + "(" in r["Kernel_Name"] or r["Kernel_Name"].endswith(name)]

    out = {}
    for name in KERNELS + ("summary_accumulate_kernel",):
        us = durations(name)
        if not us:
            raise SystemExit(f"no {name} in {f}")
        out[name] = dict(launches=len(us), median_us=statistics.median(us), min_us=min(us))
    ld = (args.n + 3) // 4 * 4
    b = 8.0 * args.n * ld
    med = out["rank_pairwise_kernel"]["median_us"]
    floor_us = b / (SUMMARY_TB_PER_S * 1e12) * 1e6
    out["rank_pairwise_kernel"].update(bytes_moved=b, tb_per_s=b / (med * 1e-6) / 1e12,
                                       fraction_of_6_3_tb_per_s=b / (med * 1e-6) / 6.3e12,
                                       us_at_summary_kernel_rate=floor_us, ratio_to_that=med / floor_us,
                                       ratio_to_summary_accumulate_kernel=med / out["summary_accumulate_kernel"]["median_us"])
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
