"""What predicting new respondents' unseen answers (csrc/predict.hip) costs at the metric size, 8192 x 1024, with
gpirt_fast_options(), at n_new = 256 and 16384.

  python tools/predict_cost.py --out FILE.json [--parent-lib PATH]
      per n_new, in one process, alternating, R rounds of K steps each: the step loop + score_accumulate with the
      prediction off, and the same loop with it on.  With --parent-lib (libgpirt_hip.so built from the parent commit) the
      scoring-only loop is also run in child processes, alternating between that library and this one, in the same
      session: their medians and the spread between the children of ONE library say whether switching the prediction off
      leaves the scorer as fast as it was.
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/predict_cost.py --kernel-only --n-new N
      a few steps with score_accumulate (prediction on) after each, then 10 more score_accumulate launches: a trace that
      holds the four launches of a predicted draw;
  python tools/predict_cost.py --trace DIR --n-new N --merge FILE.json
      their median durations from that trace, the epilogue's rate on the 6 x 8 n_new m bytes it moves and the
      contraction's on its 2 x n_new x 2m x 1024 flops.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the four launches of a predicted draw, by what their (demangled) names contain
LAUNCHES = dict(weights="score_accumulate_kernel<true>", operands="pred_operands_kernel",
                contraction="gemm_f64_kernel<true, false", epilogue="pred_epilogue_kernel")
NP = 1024


def sampler(n, m, n_new):
    from gpirt_amd import Sampler, _lib
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    if os.environ.get("GPIRT_HIP_LIBRARY"):              # an older build of the library: bind only what it exports
        import ctypes
        old = ctypes.CDLL(_lib.LIB_PATH)
        for name in [k for k in _lib.SIGNATURES if not hasattr(old, k)]:
            del _lib.SIGNATURES[name]
    y, th0 = make_responses(n, m, seed=20240)
    y_new, _ = make_responses(n_new, m, seed=20241, na_frac=0.3)
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    s.check()
    return h, s, y_new


def loop_rates(s, y_new, forms, rounds, steps):
    rates = {k: [] for k in forms}
    for _ in range(rounds):
        for form in forms:
            s.score_enable(y_new)
            if form == "predict":
                s.score_predict_enable()
            s.check()
            t0 = time.perf_counter()
            for _ in range(steps):
                s.step()
                s.score_accumulate()
            s.check()
            rates[form].append(steps / (time.perf_counter() - t0))
            s.score_enable(None)
    return rates


def timing(args):
    out = dict(n=args.n, m=args.m, options="gpirt_fast_options", rounds=args.rounds, steps_per_round=args.steps, sizes={})
    for n_new in args.n_new:
        h, s, y_new = sampler(args.n, args.m, n_new)
        for _ in range(args.warmup):
            s.step()
        s.check()
        rates = loop_rates(s, y_new, ("score", "predict"), args.rounds, args.steps)
        s.close()
        h.close()
        med = {k: statistics.median(v) for k, v in rates.items()}
        out["sizes"][str(n_new)] = dict(iterations_per_s=rates, median_iterations_per_s=med,
                                        added_ms_per_iteration=(1.0 / med["predict"] - 1.0 / med["score"]) * 1e3,
                                        ratio_to_scoring_only=med["predict"] / med["score"])
    if args.parent_lib:
        out["scoring_only_against_parent"] = against_parent(args)
    return out


def score_only(args):
    """child process: the scoring-only loop on whatever library GPIRT_HIP_LIBRARY names; prints one JSON line"""
    h, s, y_new = sampler(args.n, args.m, args.n_new[0])
    for _ in range(args.warmup):
        s.step()
    s.check()
    rates = loop_rates(s, y_new, ("score",), args.rounds, args.steps)["score"]
    s.close()
    h.close()
    print(json.dumps(dict(iterations_per_s=rates, median=statistics.median(rates))))


def against_parent(args):
    res = {}
    for n_new in args.n_new:
        runs = dict(parent=[], this=[])
        for _ in range(args.children):
            for who in ("parent", "this"):
                env = dict(os.environ)
                env.pop("GPIRT_HIP_LIBRARY", None)
                if who == "parent":
                    env["GPIRT_HIP_LIBRARY"] = os.path.abspath(args.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--score-only", "--n", str(args.n), "--m", str(args.m),
                       "--n-new", str(n_new), "--rounds", str(args.rounds), "--steps", str(args.steps)]
                line = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1]
                runs[who].append(json.loads(line)["median"])
        med = {k: statistics.median(v) for k, v in runs.items()}
        spread = max((max(v) - min(v)) / statistics.median(v) for v in runs.values())
        res[str(n_new)] = dict(child_medians_iterations_per_s=runs, median_iterations_per_s=med,
                               this_over_parent=med["this"] / med["parent"], run_to_run_spread=spread,
                               within_spread=abs(med["this"] / med["parent"] - 1.0) <= spread)
    return res


def kernel_only(args):
    h, s, y_new = sampler(args.n, args.m, args.n_new[0])
    s.score_enable(y_new)
    s.score_predict_enable()
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
    n_new, m = args.n_new[0], args.m
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us_of = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3      # noqa: E731
    out = {}
    for key, name in LAUNCHES.items():
        if key == "contraction":     # other stages launch this instantiation too: ours is the launch behind the operands' kernel
            us = [us_of(rows[i + 1]) for i, r in enumerate(rows[:-1])
                  if LAUNCHES["operands"] in r["Kernel_Name"] and "gemm_f64_kernel" in rows[i + 1]["Kernel_Name"]]
            name = next(r["Kernel_Name"] for i, r in enumerate(rows[1:]) if LAUNCHES["operands"] in rows[i]["Kernel_Name"])
        else:
            us = [us_of(r) for r in rows if name in r["Kernel_Name"]]
        if not us:
            raise SystemExit(f"no {name} in {f}")
        out[key] = dict(kernel=name, launches=len(us), median_us=statistics.median(us), min_us=min(us))
    b = 6.0 * 8.0 * n_new * m                            # C read (2), both sums read and written (4)
    out["epilogue"].update(bytes_moved=b, tb_per_s=b / (out["epilogue"]["median_us"] * 1e-6) / 1e12)
    fl = 2.0 * n_new * 2 * m * NP
    out["contraction"].update(flops=fl, tflops=fl / (out["contraction"]["median_us"] * 1e-6) / 1e12)
    out["per_draw_us"] = sum(v["median_us"] for v in out.values())
    rec = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
    rec.setdefault("launches", {})[str(n_new)] = out
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--n-new", dest="n_new", type=int, nargs="+", default=[256, 16384])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--children", type=int, default=3)
    ap.add_argument("--parent-lib", dest="parent_lib", default=None)
    ap.add_argument("--score-only", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_only:
        return kernel_only(args)
    if args.score_only:
        return score_only(args)
    rec = from_trace(args) if args.trace else timing(args)
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    out = args.out or args.merge
    if out:
        with open(out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
