"""What PSIS-LOO (csrc/loo.hip) costs at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/loo_cost.py --out profiles/loo_cost.json [--parent-ms X] [--planned 2000] [--tail M]
      in one process, interleaved, R rounds of K steps each: the steady step loop with the accumulators off ("plain") and the
      same loop with loo_accumulate after each step ("loo"; the state is made once for --planned draws, 9.4 GB at 2000).  The
      record holds every round's time per iteration, the medians, the added time per iteration, the slowdown and the accumulate
      kernel's bytes per second counted from its compulsory traffic (f, mu, the y byte, the root, p_sum and count: 49 bytes per
      cell and draw); then the finish (loo(top=20): sort, fit, totals, copies to the host) is timed on its own.
      --parent-ms: the plain loop's median ms per iteration measured on the parent commit (tools/equate_cost.py's "plain" entry
      there); the record then holds the ratio, which is expected to be 1 within the spread of the rounds.
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
    ap.add_argument("--planned", type=int, default=2000)
    ap.add_argument("--tail", type=int, default=None)
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
    from gpirt_amd import Sampler
    from gpirt_amd import loo as LO
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(args.n, args.m, seed=20240)
    n, m = y.shape
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    for _ in range(args.warmup):
        s.step()
    s.check()
    M = LO.tail_length(args.planned, args.tail)
    s.loo_enable(args.planned, args.tail)
    ms = dict(plain=[], loo=[])
    for _ in range(args.rounds):
        for kind in ("plain", "loo"):
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if kind == "loo":
                    s.loo_accumulate()
            s.check()
            ms[kind].append((time.perf_counter() - t0) / args.steps * 1e3)
    entered = int(s.loo_get("counts")[4])
    s.loo_enable(on=False)
    # the finish on a state that is complete: T = the draws of a short run
    T = max(args.rounds * args.steps, 30)
    s.loo_enable(T, None)
    for _ in range(T):
        s.step()
        s.loo_accumulate()
    s.check()
    t0 = time.perf_counter()
    fin = s.loo(top=20)
    finish_ms = (time.perf_counter() - t0) * 1e3
    s.close()
    h.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    added = med["loo"] - med["plain"]
    rec = dict(n=n, m=m, options="gpirt_fast_options", measured=True, planned_draws=args.planned, tail=M,
               state_bytes=n * m * (8 * (M + 1) + 33), rounds=args.rounds, steps_per_round=args.steps, draws_entered=entered,
               ms_per_iteration=ms, median_ms_per_iteration=med, spread_ms_plain=max(ms["plain"]) - min(ms["plain"]),
               added_ms_per_iteration=added, slowdown=med["loo"] / med["plain"],
               accumulate_bytes_per_s=(49.0 * n * m) / (added * 1e-3) if added > 0 else None,
               finish=dict(T=T, M=fin["M"], ms=finish_ms, cells_incomplete=fin["cells_incomplete"], n_obs=fin["n_obs"]))
    if args.parent_ms is not None:
        rec.update(parent_plain_ms_per_iteration=args.parent_ms, plain_ratio_to_parent=med["plain"] / args.parent_ms)
    return rec


if __name__ == "__main__":
    main()
