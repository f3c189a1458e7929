"""What scoring new respondents under ordinal responses costs at the metric size, 8192 x 1024, with the fast options, C = 5 and
10 % missing cells, for n_new = 1024 and 16384 (csrc/ordinal_score.hip, gpirt_amd.ordinal.score_*).

  python tools/ordinal_score_cost.py --out profiles/ordinal_score_cost.json
      one ordinal sampler, one process, gpirt_fast_options(), a host clock around work that ends in a synchronise.  Per n_new and
      for the score part alone and with predict:
      (a) --rounds alternating rounds of --steps iterations (step + draw_thresholds) with ordinal_score_accumulate after every
          iteration against the same sampler with the block off: iterations per second of each round;
      (b) the accumulate alone, --calls back to back, and its cost per new respondent against what the chain's own theta_partial
          (the same product for the chain's n respondents; the device time of the theta_gemm stage) costs per respondent.
  python tools/ordinal_score_cost.py --out ... --headline-this a,b,c --headline-parent a,b,c --headline-flags "..."
      also records bench.py's headline (three alternating runs each on this commit and its parent, as given with the flags
      they were run with: bench.py enables none of this).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def state_bytes(n_new, m, C, predict):
    """Device memory of one state, from the shapes (include/gpirt_hip.h)"""
    b = 8.0 * (n_new * C * m + 1024 * C * m + 2 * 1001 * n_new + 1001 * m)
    if predict:
        b += 16.0 * (C + 1) * n_new * m + 8.0 * 1024 * (n_new + (C + 1) * m)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--categories", type=int, default=5)
    ap.add_argument("--n-new", default="1024,16384")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--headline-this", default="")
    ap.add_argument("--headline-parent", default="")
    ap.add_argument("--headline-flags", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from gpirt_amd import Sampler
    from gpirt_amd import ordinal as OR
    from gpirt_amd.ops import Handle
    n, m, C = args.n, args.m, args.categories
    d = OR.make_graded(n, m, C, seed=20240, na_frac=0.1)
    cat = d["cat"]
    h = Handle(0)
    s = Sampler(h, OR.dichotomise(cat), d["theta"], seed=1, preset="fast")
    s.init()
    s.ordinal_enable(cat, C, K0=OR.init_thresholds(cat, OR.grid(), C))

    def iterations(k, score):
        h.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            s.step()
            s.draw_thresholds()
            if score:
                s.ordinal_score_accumulate()
        h.synchronize()
        return k / (time.perf_counter() - t0)

    iterations(args.warmup, False)
    # the chain's own product per respondent: the device time of the theta_gemm stage
    s.enable_timing(True)
    gemm = []
    for _ in range(5):
        s.step()
        s.draw_thresholds()
        gemm.append(s.stage_times()["theta_gemm"])
    s.enable_timing(False)
    theta_ms = statistics.median(gemm)
    cases = {}
    for n_new in [int(x) for x in args.n_new.split(",")]:
        new = OR.make_graded(n_new, m, C, seed=777, na_frac=0.3, slopes=d["slopes"], thresholds=d["thresholds"])["cat"]
        for predict in (False, True):
            rate = {"on": [], "off": []}
            for _ in range(args.rounds):
                for mode in ("on", "off"):
                    if mode == "on":
                        s.ordinal_score_enable(new, predict=predict)
                        iterations(1, True)
                    rate[mode].append(iterations(args.steps, mode == "on"))
                    if mode == "on":
                        s.ordinal_score_enable(None)
            s.ordinal_score_enable(new, predict=predict)
            for _ in range(2):
                s.ordinal_score_accumulate()
            h.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                s.ordinal_score_accumulate()
            h.synchronize()
            ms = (time.perf_counter() - t0) / args.calls * 1e3
            s.ordinal_score_enable(None)
            s.check()
            on, off = statistics.median(rate["on"]), statistics.median(rate["off"])
            cases[f"n_new={n_new},predict={int(predict)}"] = dict(
                iterations_per_s=dict(on=rate["on"], off=rate["off"], median_on=on, median_off=off,
                                      ms_added_per_iteration=(1.0 / on - 1.0 / off) * 1e3),
                accumulate_alone_ms=ms, us_per_new_respondent=ms * 1e3 / n_new,
                ratio_to_theta_partial_per_respondent=(ms / n_new) / (theta_ms / n),
                state_bytes=state_bytes(n_new, m, C, predict))
    s.close()
    h.close()
    out = dict(n=n, m=m, categories=C, missing=float((cat == 0).mean()), steps=args.steps, rounds=args.rounds, calls=args.calls,
               theta_partial_ms=theta_ms, theta_partial_us_per_respondent=theta_ms * 1e3 / n, cases=cases,
               predict_state_bytes_16384x1024_C8=state_bytes(16384, 1024, 8, True) - state_bytes(16384, 1024, 8, False))
    if args.headline_this or args.headline_parent:
        out["bench_headline_iterations_per_s"] = dict(flags=args.headline_flags,
                                                      this=[float(x) for x in args.headline_this.split(",")],
                                                      parent=[float(x) for x in args.headline_parent.split(",")])
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
