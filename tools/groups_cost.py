"""What the group posteriors (csrc/groups.hip) cost at the metric size, 8192 x 1024, with gpirt_fast_options(), G = 2 and G = 8.

  python tools/groups_cost.py --out profiles/groups_cost.json
      in one process, per G: R alternating rounds of K steps each, the steady step loop without and with groups_accumulate
      after every step; then the accumulate alone, `launches` calls between two synchronisations, set beside the floor the
      bytes give -- f and mu read twice, y once (the second pass only over the contested items, so the draw's own count of
      contested items is recorded with it) -- at the rate the acf pass is recorded to reach (2.6 TB/s);
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/groups_cost.py --kernel-only --groups 8
      groups_accumulate alone, `launches` calls, for a trace that holds nothing else of note;
  python tools/groups_cost.py --trace DIR --groups 8 --contested N --merge profiles/groups_cost.json
      the kernels' median durations from that trace, under "kernels" -> "G8" (N: the contested items the traced run printed);
  python tools/groups_cost.py --headlines "p1,p2,p3" "c1,c2,c3" --merge profiles/groups_cost.json
      bench.py's headline in alternating runs of the parent commit and this one.
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

KERNELS = ("grp_hist_kernel", "grp_latent_kernel", "grp_share_kernel", "grp_votes_kernel", "grp_items_kernel",
           "grp_loyalty_kernel", "grp_loy_update_kernel")
ACF_RATE = 2.6e12                    # bytes per second the acf block's pass over f, mu and y is recorded to reach (README)


def make_codes(truth, G):
    """G groups of equal size by the generating theta: the groups lie apart, so many items are contested and the second pass has
    work to do (groups that do not differ contest next to nothing, and the second pass then loads next to nothing)"""
    import numpy as np
    rank = np.argsort(np.argsort(truth))
    return (rank * G // truth.shape[0]).astype(np.int32)


def setup(args, G):
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    y, th0, truth = make_responses(args.n, args.m, seed=20240, return_truth=True)
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    for _ in range(args.warmup):
        s.step()
    s.check()
    s.groups_enable(make_codes(truth, G))
    s.groups_accumulate()
    s.check()
    return h, s


def timing(args):
    rec = dict(n=args.n, m=args.m, options="gpirt_fast_options", rounds=args.rounds, steps_per_round=args.steps, by_groups={})
    for G in args.groups:
        h, s = setup(args, G)
        rates = {"off": [], "on": []}
        for _ in range(args.rounds):
            for form in rates:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    s.step()
                    if form == "on":
                        s.groups_accumulate()
                s.check()
                rates[form].append(args.steps / (time.perf_counter() - t0))
        med = {k: statistics.median(v) for k, v in rates.items()}
        walls = []
        for _ in range(3):
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.launches):
                s.groups_accumulate()
            s.check()
            walls.append((time.perf_counter() - t0) / args.launches)
        contested = int(s.groups_get("contested").sum())
        cell = 8.0 * args.n * args.m
        b = dict(pass_1_f_mu=2 * cell, pass_2_f_mu_y_all_items=3 * cell, pass_2_f_mu_y_contested=3 * cell * contested / args.m)
        b["total_all_items"] = b["pass_1_f_mu"] + b["pass_2_f_mu_y_all_items"]
        b["total_this_draw"] = b["pass_1_f_mu"] + b["pass_2_f_mu_y_contested"]
        acc_s = statistics.median(walls)
        rec["by_groups"][f"G{G}"] = dict(
            iterations_per_s=rates, median_iterations_per_s=med, ratio_on_to_off=med["on"] / med["off"],
            ms_added_per_draw=1e3 * (1.0 / med["on"] - 1.0 / med["off"]),
            accumulate=dict(launches=args.launches, seconds_per_accumulate=walls, median_ms=acc_s * 1e3, contested_items=contested,
                            algorithmic_bytes=b, floor_ms_at_acf_rate_all_items=b["total_all_items"] / ACF_RATE * 1e3,
                            floor_ms_at_acf_rate_this_draw=b["total_this_draw"] / ACF_RATE * 1e3,
                            tb_per_s_this_draw=b["total_this_draw"] / acc_s / 1e12),
            state_bytes=int(s.groups_state().numel() * 8))
        s.groups_enable(on=False)
        s.close()
        h.close()
    return rec


def kernel_only(args):
    h, s = setup(args, args.groups[0])
    for _ in range(2 * args.rounds * args.steps):        # the chain as far along as the timing run's: as many items contested
        s.step()
    s.check()
    s.groups_accumulate()
    print("contested_items", int(s.groups_get("contested").sum()), flush=True)
    for _ in range(args.launches):
        s.groups_accumulate()
    s.check()
    s.close()
    h.close()


def from_trace(args):
    f = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for name in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if not us:
            raise SystemExit(f"no {name} in {f}")
        out[name] = dict(launches=len(us), median_us=statistics.median(us), min_us=min(us))
    out["per_draw_us"] = sum(out[k]["median_us"] for k in KERNELS)
    if args.contested is not None:
        out["contested_items"] = args.contested
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--groups", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--contested", type=int, default=None, help="what the traced run printed, kept beside its kernels")
    ap.add_argument("--headlines", nargs=2, default=None, metavar=("PARENT", "THIS"))
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_only:
        kernel_only(args)
        return
    rec = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
    if args.trace:
        rec.setdefault("kernels", {})[f"G{args.groups[0]}"] = from_trace(args)
    elif args.headlines:
        par, cur = ([float(v) for v in h.split(",")] for h in args.headlines)
        rec["bench_headline_iterations_per_s"] = dict(
            parent_commit=par, this_commit=cur, order="alternating, the parent first",
            ranges_overlap=bool(min(par) <= max(cur) and min(cur) <= max(par)))
    else:
        rec.update(timing(args))
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    out = args.out or args.merge
    if out:
        with open(out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
