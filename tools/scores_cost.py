"""What the score-based checks (csrc/ppc_scores.hip) cost at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/scores_cost.py --out FILE.json
      in one session, alternating, R rounds of K steps each: the step loop + ppc_accumulate with ppc alone, with the block at
      the default cuts (up to 9 groups) and at 16 groups -- ms per sampling iteration, every round's figure kept so that the
      run-to-run spread can be read off -- and ppc_accumulate alone (L launches between two synchronisations) in the same three
      forms.  The block's two passes read f, mu and y twice (2 x 3 x 64 MB = 403 MB), write and read the bit plane and the row
      partials; what it adds to ppc_accumulate over those bytes is its achieved rate (a lower bound: the three small kernels around
      the passes are inside the figure).
  python tools/scores_cost.py --child scores_k16    (internal: one form's rounds as a JSON line)
  The kernels' own durations come from a separate run: rocprofv3 --kernel-trace --stats -- python tools/scores_cost.py --child scores_k16
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("ppc", "scores_default", "scores_k16")


def sampler(n, m):
    sys.path.insert(0, HERE)
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    s.check()
    return h, s


def cuts_of(form, s, m):
    if form == "scores_default":
        from gpirt_amd import ppc as P
        return P.default_score_cuts(s.get("y"))
    return tuple(1 + (k * (m - 1)) // 16 for k in range(1, 16))


def measure(args, forms):
    h, s = sampler(args.n, args.m)
    for _ in range(args.warmup):
        s.step()
    s.check()
    step_ms = {f: [] for f in forms}
    acc_ms = {f: [] for f in forms}
    groups = {}
    for _ in range(args.rounds):
        for form in forms:
            s.ppc_enable()
            if form != "ppc":
                cuts = cuts_of(form, s, args.m)
                groups[form] = len(cuts) + 1
                s.ppc_scores_enable(cuts)
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                s.ppc_accumulate()
            s.check()
            step_ms[form].append(1e3 * (time.perf_counter() - t0) / args.steps)
            s.ppc_accumulate()
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.launches):
                s.ppc_accumulate()
            s.check()
            acc_ms[form].append(1e3 * (time.perf_counter() - t0) / args.launches)
    s.close()
    h.close()
    return dict(ms_per_iteration=step_ms, ppc_accumulate_ms=acc_ms, groups=groups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args, [args.child])))
        return
    n, m = args.n, args.m
    rec = dict(n=n, m=m, options="gpirt_fast_options", measured=True, rounds=args.rounds, steps_per_round=args.steps,
               accumulate_launches_per_round=args.launches)
    alt = rec["alternating"] = measure(args, list(FORMS))
    med = statistics.median
    floor_bytes = 8.0 * n * m
    summary = {}
    for form in FORMS:
        v = alt["ms_per_iteration"][form]
        summary[f"{form}_ms_per_iteration"] = med(v)
        summary[f"{form}_ms_per_iteration_spread"] = [min(v), max(v)]
        summary[f"{form}_accumulate_ms"] = med(alt["ppc_accumulate_ms"][form])
        if form != "ppc":
            K = alt["groups"][form]
            strips, words = (m + 31) // 32, (n + 63) // 64
            plane = 8.0 * m * words                                # the bit plane: written by pass A, read by pass B
            parts = 4.0 * strips * n                               # the strips' row partials: written, then read
            tables = 8.0 * (5 * K + 4) * m                         # the draw's tables: added to, read, cleared
            moved = 6.0 * floor_bytes + 2.0 * plane + 2.0 * parts + 3.0 * tables
            added = med(alt["ppc_accumulate_ms"][form]) - med(alt["ppc_accumulate_ms"]["ppc"])
            summary[f"{form}_groups"] = K
            summary[f"{form}_added_ms_per_iteration"] = med(v) - med(alt["ms_per_iteration"]["ppc"])
            summary[f"{form}_added_accumulate_ms"] = added
            summary[f"{form}_bytes_per_accumulate"] = moved
            summary[f"{form}_achieved_bytes_per_s"] = moved / (added * 1e-3)
    summary["read_floor_bytes_two_passes_f_mu_y"] = 6.0 * floor_bytes
    summary["note"] = ("every figure from one session, the forms alternating; ppc_accumulate_ms is wall time over back-to-back launches "
                       "between two synchronisations (the PPC's own kernels included); achieved_bytes_per_s divides the block's bytes by "
                       "what it adds to that")
    rec["summary"] = summary
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
