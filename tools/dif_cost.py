"""What the group-wise item fit (csrc/ppc_dif.hip) costs at the metric size, 8192 x 1024, with gpirt_fast_options().

  python tools/dif_cost.py --out FILE.json [--parent-root DIR]
      in one session, alternating, R rounds of K steps each: the step loop + ppc_accumulate with ppc alone, with the block at
      (G = 2, h = 4) and at (G = 4, h = 15) -- ms per sampling iteration, every round's figure kept so that the run-to-run
      spread can be read off -- and ppc_accumulate alone (L launches between two synchronisations) in the same three forms.
      The block's own pass reads f, mu and y once more (3 x 64 MB = 192 MB); what it adds to ppc_accumulate over those bytes is
      its achieved rate (a lower bound: the two small kernels around it are inside the figure).
      --parent-root: a checkout of the parent commit with its library built; a child process measures ppc alone there before
      and after this commit's rounds.
  python tools/dif_cost.py --child ppc    (internal: one form's rounds as a JSON line)
  The kernels' own durations come from a separate run: rocprofv3 --kernel-trace --stats -- python tools/dif_cost.py --child dif_g4_h15
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"ppc": None, "dif_g2_h4": (2, (14, 43, 76, 122)), "dif_g4_h15": (4, tuple(range(10, 460, 30)))}


def sampler(root, n, m):
    sys.path.insert(0, root)
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    s.check()
    return h, s


def measure(args, forms):
    h, s = sampler(args.root, args.n, args.m)
    for _ in range(args.warmup):
        s.step()
    s.check()
    step_ms = {f: [] for f in forms}
    acc_ms = {f: [] for f in forms}
    for _ in range(args.rounds):
        for form in forms:
            s.ppc_enable()
            if FORMS[form] is not None:
                import numpy as np
                G, cuts = FORMS[form]
                s.ppc_dif_enable(np.arange(args.n) % G, cuts)
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
    return dict(ms_per_iteration=step_ms, ppc_accumulate_ms=acc_ms)


def child(args, root, form):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form, "--root", root, "--n", str(args.n), "--m",
                          str(args.m), "--rounds", str(args.rounds), "--steps", str(args.steps), "--warmup", str(args.warmup),
                          "--launches", str(args.launches)], check=True, capture_output=True, text=True, timeout=600)
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args, [args.child])))
        return
    n, m = args.n, args.m
    rec = dict(n=n, m=m, options="gpirt_fast_options", rounds=args.rounds, steps_per_round=args.steps,
               accumulate_launches_per_round=args.launches)
    parent = []
    if args.parent_root:
        parent.append(child(args, args.parent_root, "ppc"))
    rec["this_commit"] = child(args, HERE, "ppc")                  # a process of its own, as the parent's figure is
    rec["this_commit_alternating"] = measure(args, list(FORMS))
    if args.parent_root:
        parent.append(child(args, args.parent_root, "ppc"))
        rec["parent_commit"] = dict(ms_per_iteration=dict(ppc=sum((p["ms_per_iteration"]["ppc"] for p in parent), [])),
                                    ppc_accumulate_ms=dict(ppc=sum((p["ppc_accumulate_ms"]["ppc"] for p in parent), [])))
    med = lambda v: statistics.median(v)                           # noqa: E731
    alt = rec["this_commit_alternating"]
    summary = dict(ppc_ms_this_commit=med(rec["this_commit"]["ms_per_iteration"]["ppc"]),
                   ppc_ms_this_commit_spread=[min(rec["this_commit"]["ms_per_iteration"]["ppc"]),
                                              max(rec["this_commit"]["ms_per_iteration"]["ppc"])])
    if args.parent_root:
        pv = rec["parent_commit"]["ms_per_iteration"]["ppc"]
        summary.update(ppc_ms_parent_commit=med(pv), ppc_ms_parent_commit_spread=[min(pv), max(pv)])
    floor_bytes = 8.0 * n * m
    for form, spec in FORMS.items():
        summary[f"{form}_ms_per_iteration"] = med(alt["ms_per_iteration"][form])
        summary[f"{form}_accumulate_ms"] = med(alt["ppc_accumulate_ms"][form])
        if spec is not None:
            cells = spec[0] * (2 * len(spec[1]) + 1)
            tables = 24.0 * cells * m                              # the draw's tables: N | T | R, E, V as uint64
            moved = 3.0 * floor_bytes + 3.0 * tables               # f, mu, y read once; the tables added to, read, cleared
            added = med(alt["ppc_accumulate_ms"][form]) - med(alt["ppc_accumulate_ms"]["ppc"])
            summary[f"{form}_added_ms_per_iteration"] = med(alt["ms_per_iteration"][form]) - med(alt["ms_per_iteration"]["ppc"])
            summary[f"{form}_added_accumulate_ms"] = added
            summary[f"{form}_bytes_per_accumulate"] = moved
            summary[f"{form}_achieved_bytes_per_s"] = moved / (added * 1e-3)
    summary["read_floor_bytes_f_mu_y"] = 3.0 * floor_bytes
    summary["note"] = ("every figure from one session; ppc_accumulate_ms is wall time over back-to-back launches between two "
                       "synchronisations (the PPC's own kernels included); achieved_bytes_per_s divides the block's bytes by what it adds to that")
    rec["summary"] = summary
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
