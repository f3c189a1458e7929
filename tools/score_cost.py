"""What scoring new respondents (csrc/score.hip) costs at the metric size, 8192 x 1024, n_new = 8192, with
gpirt_fast_options().

  python tools/score_cost.py --out FILE.json
      in one process, alternating, R rounds of K steps each: the steady step loop, and the same loop + score_accumulate.
      The number to record is the added time per iteration against the plain loop of the same process.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/score_cost.py --kernel-only
      a few steps with score_accumulate after each, then 20 more score_accumulate launches: a trace that holds the
      product's kernels (tf_mfma_kernel, or the fp64 GEMM under GPIRT_THETA_FIXED=2) and score_accumulate_kernel;
  python tools/score_cost.py --trace DIR --merge FILE.json
      those kernels' median durations from that trace, and score_accumulate_kernel's rate on the 3 x 8 N n_new bytes it
      moves (the product read, post_sum read and written; 197 MB at n_new = 8192).
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

KERNELS = ("score_accumulate_kernel", "score_clean_kernel", "score_flag_kernel", "tf_mfma_kernel", "tf_quant_kernel",
           "tf_rowmax_kernel")
FORMS = ("plain", "score")
NGRID = 1001


def sampler(n, m, n_new):
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=20240)
    y_new, _ = make_responses(n_new, m, seed=20241)
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    s.check()
    return h, s, y_new


def timing(args):
    h, s, y_new = sampler(args.n, args.m, args.n_new)
    for _ in range(args.warmup):
        s.step()
    s.check()
    rates = {k: [] for k in FORMS}
    draws = None
    for _ in range(args.rounds):
        for form in FORMS:
            if form == "score":
                s.score_enable(y_new)
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if form == "score":
                    s.score_accumulate()
            s.check()
            rates[form].append(args.steps / (time.perf_counter() - t0))
            if form == "score":
                draws = int(s.score_get("draws").min())
                s.score_enable(None)
    s.close()
    h.close()
    med = {k: statistics.median(v) for k, v in rates.items()}
    return dict(n=args.n, m=args.m, n_new=args.n_new, options="gpirt_fast_options", rounds=args.rounds,
                steps_per_round=args.steps, iterations_per_s=rates, median_iterations_per_s=med,
                added_ms_per_iteration=(1.0 / med["score"] - 1.0 / med["plain"]) * 1e3,
                ratio_to_plain=med["score"] / med["plain"], last_round_draws=draws)


def kernel_only(args):
    h, s, y_new = sampler(args.n, args.m, args.n_new)
    s.score_enable(y_new)
    for _ in range(3):
        s.step()
        s.score_accumulate()
    for _ in range(args.launches):
        s.score_accumulate()
    s.check()
    s.close()
    h.close()


def from_trace(args):
    f = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    out = {}
    for name in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if us:
            out[name] = dict(launches=len(us), median_us=statistics.median(us), min_us=min(us))
    if "score_accumulate_kernel" not in out:
        raise SystemExit(f"no score_accumulate_kernel in {f}")
    b = 3.0 * 8.0 * NGRID * args.n_new
    med = out["score_accumulate_kernel"]["median_us"]
    out["score_accumulate_kernel"].update(bytes_moved=b, tb_per_s=b / (med * 1e-6) / 1e12,
                                          fraction_of_6_3_tb_per_s=b / (med * 1e-6) / 6.3e12)
    # (tf_mfma_kernel also runs once per step for draw_theta: the medians are per launch, so that does not matter)
    out["per_draw_us"] = sum(v["median_us"] for v in out.values())
    rec = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
    rec["kernels"] = out
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--n-new", dest="n_new", type=int, default=8192)
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
