"""What the person fit (csrc/ppc_person.hip) costs at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/person_cost.py --out FILE.json
      in one session, alternating, R rounds of K steps each: the step loop + ppc_accumulate with ppc alone, with the block at
      5 groups (the default) and at 16 groups -- ms per sampling iteration, every round's figure kept so that the run-to-run
      spread can be read off -- and ppc_accumulate alone (L launches between two synchronisations) in the same three forms.  The
      block's one pass reads f, mu and y once (3 x 67 MB = 201 MB), writes and reads the strips' partials (44 bytes per strip and
      respondent) and updates the respondents' accumulators; what it adds to ppc_accumulate over those bytes is its achieved rate
      (a lower bound: the finishing kernel is inside the figure).  The block off is this same build's path without it.
  python tools/person_cost.py --child person_k16    (internal: one form's rounds as a JSON line)
  The kernels' own durations come from a separate run: rocprofv3 --kernel-trace --stats -- python tools/person_cost.py --child person_k16
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("ppc", "person_k5", "person_k16")
sys.path.insert(0, HERE)


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


def strips_of(m, cuts):
    edges = (0,) + tuple(cuts) + (m,)
    return sum((hi - lo + 31) // 32 for lo, hi in zip(edges, edges[1:]))


def measure(args, forms):
    from gpirt_amd import ppc as P
    h, s = sampler(args.n, args.m)
    for _ in range(args.warmup):
        s.step()
    s.check()
    step_ms = {f: [] for f in forms}
    acc_ms = {f: [] for f in forms}
    strips = {}
    for _ in range(args.rounds):
        for form in forms:
            s.ppc_enable()
            if form != "ppc":
                K = int(form.rsplit("k", 1)[1])
                cuts = P.default_item_cuts(args.m, K)
                strips[form] = strips_of(args.m, cuts)
                s.ppc_person_enable(cuts=cuts)
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
    return dict(ms_per_iteration=step_ms, ppc_accumulate_ms=acc_ms, strips=strips)


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
            K = int(form.rsplit("k", 1)[1])
            parts = 44.0 * alt["strips"][form] * n                 # the strips' partials: written, then read
            cells = 76.0 * K * n                                   # per cell: tN, tT read, four accumulators read and written, tR, tE, tV kept
            resp = 224.0 * n                                       # per respondent: the accumulators read and written, the last draw's arrays
            moved = 3.0 * floor_bytes + 2.0 * parts + cells + resp
            added = med(alt["ppc_accumulate_ms"][form]) - med(alt["ppc_accumulate_ms"]["ppc"])
            summary[f"{form}_strips"] = alt["strips"][form]
            summary[f"{form}_added_ms_per_iteration"] = med(v) - med(alt["ms_per_iteration"]["ppc"])
            summary[f"{form}_added_accumulate_ms"] = added
            summary[f"{form}_bytes_per_accumulate"] = moved
            summary[f"{form}_achieved_bytes_per_s"] = moved / (added * 1e-3)
    summary["read_floor_bytes_one_pass_f_mu_y"] = 3.0 * floor_bytes
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
