"""What the residual correlations of the PPC (csrc/ppc_resid.hip) cost at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/resid_cost.py --out FILE.json [--bench BENCH.json] [--parent-headline X]
      in one process, alternating, R rounds of K steps each: the step loop + ppc_accumulate, and the same with the block
      enabled.  --bench: a result line of bench.py from the same session (block off); its headline and its theta_int8_product
      figure are recorded.  --parent-headline: the parent commit's recorded headline, kept beside it.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/resid_cost.py --kernel-only
      ppc_accumulate with the block alone, 20 launches, for a trace that holds nothing else of note;
  python tools/resid_cost.py --trace DIR --merge FILE.json
      the kernels' median durations from that trace, and resid_products_kernel's integer rate: the operations it issues -- nine
      digit-plane products on the lower 128-tiles of S_obs and of S_rep and three on all tiles of V, at depth n, padding included
      -- against the 5 POP/s int8 peak, beside pair_counts_kernel's and tf_mfma_kernel's recorded rates, and the operand bytes
      those passes stream from memory.  --parent-headline is accepted here too.
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

KERNELS = ("resid_terms_kernel", "resid_products_kernel", "resid_update_kernel", "resid_items_kernel", "resid_global_kernel")
INT8_PEAK_OPS = 5.0e15


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
    rates = {"ppc": [], "ppc_resid": []}
    for _ in range(args.rounds):
        for form in rates:
            s.ppc_enable()
            if form == "ppc_resid":
                s.ppc_resid_enable()
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                s.ppc_accumulate()
            s.check()
            rates[form].append(args.steps / (time.perf_counter() - t0))
    counts = s.ppc_resid_get("counts")
    s.close()
    h.close()
    med = {k: statistics.median(v) for k, v in rates.items()}
    rec = dict(n=n, m=m, options="gpirt_fast_options", rounds=args.rounds, steps_per_round=args.steps,
               iterations_per_s=rates, median_iterations_per_s=med,
               ratio_to_ppc_only={"ppc_resid": med["ppc_resid"] / med["ppc"]},
               ms_per_draw_added=1e3 / med["ppc_resid"] - 1e3 / med["ppc"],
               resid_draws_last_round=int(counts[0]), resid_skipped_last_round=int(counts[1]))
    if args.bench:
        rec["bench"] = bench_figures(args.bench)
    if args.parent_headline is not None:
        rec["bench_headline_parent_commit"] = args.parent_headline
    rec["note"] = "step rates (and bench.py, if given) from one session; 'kernels' from a rocprofv3 --kernel-trace run of its own"
    return rec


def bench_figures(path):
    """the headline, the rounds and every theta_int8 figure of a bench.py result line"""
    line = [ln for ln in open(path) if ln.lstrip().startswith("{")][-1]
    res = json.loads(line)
    out = {}

    def walk(d, pre=""):
        for k, v in d.items():
            if isinstance(v, dict):
                walk(v, pre + k + ".")
            elif "theta_int8" in k or "theta_int8" in pre or "round" in k or k in ("iterations_per_s", "value", "metric"):
                out[pre + k] = v

    walk(res)
    return out


def kernel_only(args):
    h, s = sampler(args.n, args.m)
    s.step()
    s.ppc_enable()
    s.ppc_resid_enable()
    for _ in range(args.launches):
        s.ppc_accumulate()
    s.check()
    s.close()
    h.close()


def from_trace(args):
    f = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for name in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if name == "resid_products_kernel":
            us = us[1:]                          # the first in time forms n_co at enable
        if not us:
            raise SystemExit(f"no {name} in {f}")
        out[name] = dict(launches=len(us), median_us=statistics.median(us), min_us=min(us))
    n, m = args.n, args.m
    nab = (m + 127) // 128
    kp = (n + 255) // 256 * 256
    passes = 2 * 9 * (nab * (nab + 1) // 2) + 3 * nab * nab      # 128 x 128 x depth passes of the pipeline
    ops = 2.0 * passes * 128 * 128 * kp
    med = out["resid_products_kernel"]["median_us"]
    rate = ops / (med * 1e-6)
    operand_bytes = 2.0 * passes * 128 * kp          # a pass streams 128 items of each operand at depth n, one byte each
    out["resid_products_kernel"].update(tile_passes=passes, work_groups=2 * nab * (nab + 1) + nab * nab, int_ops_issued=ops,
                                        useful_int_ops=2.0 * 12.0 * m * m * n, ops_per_s=rate,
                                        fraction_of_5_pops=rate / INT8_PEAK_OPS, operand_bytes_read=operand_bytes,
                                        operand_bytes_per_s=operand_bytes / (med * 1e-6))
    out["per_draw_us"] = sum(out[k]["median_us"] for k in KERNELS)
    rec = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
    rec["kernels"] = out
    if args.parent_headline is not None:
        rec["bench_headline_parent_commit"] = args.parent_headline
    for k, v in rec.get("bench", {}).items():          # (bench.py reports the product's rate in TOP/s)
        if k.endswith("theta_int8_product.achieved") and v:
            rec["kernels"]["resid_products_kernel"]["ratio_to_theta_int8_product"] = rate / 1e12 / v
    pc = os.path.join(ROOT, "profiles", "pair_cost.json")
    if os.path.exists(pc):                             # the yardsticks the pairs block recorded
        prev = json.load(open(pc))
        rec["pairs_block_recorded"] = dict(
            pair_counts_kernel_ops_per_s=prev.get("kernels", {}).get("pair_counts_kernel", {}).get("ops_per_s"),
            ratio_to_ppc_only=prev.get("ratio_to_ppc_only", {}).get("ppc_pairs"))
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
    ap.add_argument("--bench", default=None)
    ap.add_argument("--parent-headline", type=float, default=None)
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
