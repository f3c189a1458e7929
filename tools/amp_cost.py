"""What per-item GP amplitudes cost at the metric size, 8192 x 1024, with the fast options (csrc/amp.hip, gpirt_amd.amp).

  python tools/amp_cost.py --out profiles/amp_cost.json
      one sampler, one process, gpirt_fast_options().
      (b) iterations/s of the step loop with Sampler.amp_set(ones) on against off: --rounds rounds of --steps steps each, the
          two taken in turn, check() closing each.  Amplitude 1 leaves the chain what it is, so the two run the same states and
          the difference is the scaling pass of draw_f and the epilogue's extra factor.
      (c) amp_update_kernel's device time by the sampler's event timing (Sampler.enable_timing, amp_get("time")), --updates
          updates after a step each on the default grid (0.1 .. 10, 129 points, width 4), with the share of items that accepted;
          then, with no step between them, under a prior table peaked at the starting index (every proposal rejected: the three
          reads alone) and under one that rises by 1e6 per index (every upward proposal accepted: the rewrite of those columns).
          The yardstick is ell_delta_kernel in the same run: the length-scale update's "delta" part (grid 0.7 .. 2.8, 65 points,
          as tools/ell_cost.py) after a step each.  Bytes: three n x m fp64 arrays read, plus a read and a write of the accepted
          columns; ell_delta_kernel reads four.
  python tools/amp_cost.py --out profiles/amp_cost.json --headline-this 154.1,154.2,154.3 --headline-parent 154.0,154.2,154.4
      (a) also records bench.py's headline (iterations/s of `bench.py --gpus 1`), three alternating runs each on this commit
          and on its parent in one session, as given
  python tools/amp_cost.py --out profiles/amp_cost.json --readme README.md
      also rewrites the paragraph between the two "amp_cost" marker comments of README.md from the record
  python tools/amp_cost.py --from profiles/amp_cost.json --readme README.md
      rewrites that paragraph from an earlier record; no device is touched
  python tools/amp_cost.py --centred --out profiles/amp_cost.json [--kernel-stats DIR/..._kernel_stats.csv]
      the centred update (csrc/amp_centred.hip) ADDED to the record at --out under "centred", everything
      else of it left as it is: one gpirt_sampler_draw_amp_centred after a consistent step each, median of --updates by the
      sampler's event timing, beside the whitened update in the same run; the step loop with both updates against the whitened
      one alone, --rounds alternating rounds of --steps consistent steps in one process.  --kernel-stats: a rocprofv3
      --kernel-trace --stats table of such a run (python tools/amp_cost.py --centred-profile under rocprofv3), from which the
      call's split by kernel is taken, with the update kernel's bytes (four arrays read, accepted columns read and written once
      more) and TB/s beside ell_delta_kernel's of the record.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BEGIN, END = "<!-- amp_cost: written by tools/amp_cost.py -->", "<!-- /amp_cost -->"


def paragraph(r) -> str:
    """the README's cost paragraph from a record"""
    import textwrap
    mi, u, rej, acc, d = r["median_iterations_per_s"], r["update"], r["all_rejected"], r["upward_accepted"], r["ell_delta_kernel"]
    txt = (f"Measured on one MI355X at {r['n']} x {r['m']} with `gpirt_fast_options()` (`tools/amp_cost.py`, "
           f"`profiles/amp_cost.json`; DESIGN.md section 37). The step loop with `amp_set(ones)` on against off, {r['rounds']} "
           f"alternating rounds of {r['steps']} steps in one process: {mi['on']:.1f} iterations/s on, {mi['off']:.1f} off (rounds "
           f"on: {', '.join(f'{v:.1f}' for v in r['iterations_per_s']['on'])}; off: "
           f"{', '.join(f'{v:.1f}' for v in r['iterations_per_s']['off'])}) -- what the scaling pass over nu and the epilogue's "
           f"extra factor cost. `amp_update_kernel`, one update of all {r['m']} items after a step each on the default grid "
           f"(median of {u['updates']}): {u['ms']:.3f} ms of device time with {100 * u['accepted_share']:.0f} % of the items "
           f"accepting, {u['bytes'] / 1e6:.0f} MB moved, {u['tb_per_s']:.2f} TB/s. With every proposal rejected (three arrays read, "
           f"{rej['bytes'] / 1e6:.0f} MB): {rej['ms']:.3f} ms, {rej['tb_per_s']:.2f} TB/s; with every upward proposal accepted "
           f"({100 * acc['accepted_share']:.0f} % of the items rewrite their column, {acc['bytes'] / 1e6:.0f} MB): {acc['ms']:.3f} "
           f"ms, {acc['tb_per_s']:.2f} TB/s. The yardstick, `ell_delta_kernel` in the same run (four arrays read, "
           f"{d['bytes'] / 1e6:.0f} MB): {d['ms']:.3f} ms, {d['tb_per_s']:.2f} TB/s. {r['verdict']}")
    if r.get("headline"):
        hl = r["headline"]
        txt += (f" With amplitudes off nothing is on the step path: `bench.py`'s headline, three alternating runs each in one "
                f"session, is {', '.join(f'{v:.2f}' for v in hl['this'])} iterations/s on this commit and "
                f"{', '.join(f'{v:.2f}' for v in hl['parent'])} on its parent.")
    return "\n".join(textwrap.wrap(txt, 124))


def write_readme(path, r):
    src = open(path).read()
    i, j = src.index(BEGIN), src.index(END)
    with open(path, "w") as fh:
        fh.write(src[:i + len(BEGIN)] + "\n" + paragraph(r) + "\n" + src[j:])


def verdict(rej, acc, d) -> str:
    """how the new kernel's rate stands against the yardstick's, in words"""
    ratio = rej["tb_per_s"] / d["tb_per_s"]
    if ratio >= 0.95:
        first = (f"The update's read-only rate is {ratio:.2f} of that kernel's: per row it evaluates the same two terms and "
                 f"loads one array less.")
    else:
        first = (f"The update's read-only rate falls short of that kernel's by {100 * (1 - ratio):.0f} %: it moves a quarter fewer "
                 f"bytes for the same two log-likelihood terms per row, so the terms' arithmetic weighs more against the loads, and "
                 f"every work-group first runs two Philox blocks and ends with a dependent decision by one thread.")
    second = (f" The accepting columns cost a second pass over f by the same work-group after the decision -- a dependent read and "
              f"write that cannot overlap the reduction -- which is the {acc['ms'] - rej['ms']:.3f} ms between the two figures.")
    return first + second


CENTRED_KERNELS = ("nu_basis_kernel", "gemm_f64_kernel", "sum_parts_kernel", "fstar_free_xhat_r_kernel", "amp_centred_coef_kernel",
                   "amp_centred_update_kernel")


def centred(args):
    """--centred / --centred-profile (the module docstring)"""
    import csv
    import numpy as np
    from gpirt_amd import Sampler
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    n, m = args.n, args.m
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, seed=1, preset="fast")
    s.init()
    s.amp_enable(0.1, 10.0, 129, None, 4)
    for _ in range(args.warmup):
        s.step(consistent=True)
        s.draw_amp()
        s.draw_amp_centred()
    s.check()
    if args.centred_profile:                       # under rocprofv3: the calls alone, so that the table's calls are theirs
        for _ in range(args.updates):
            s.draw_amp_centred()
        s.check()
        s.close()
        h.close()
        return
    s.enable_timing(True)
    ms, ms_w, acc, same = [], [], [], []
    for _ in range(args.updates):
        s.step(consistent=True)
        s.check()
        s.draw_amp()
        ms_w.append(float(s.amp_get("time")[0]))
        before = s.amp_centred()
        s.draw_amp_centred()
        ms.append(float(s.amp_get("time_centred")[0]))
        after = s.amp_centred()
        acc.append((after["accepted"] - before["accepted"]) / m)
        same.append((after["same"] - before["same"]) / m)
    s.enable_timing(False)
    rates = {"both": [], "whitened": []}
    for _ in range(args.rounds):
        for name in ("both", "whitened"):
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step(consistent=True)
                s.draw_amp()
                if name == "both":
                    s.draw_amp_centred()
            s.check()
            rates[name].append(args.steps / (time.perf_counter() - t0))
    st = s.amp_centred()
    s.close()
    h.close()
    rec = dict(n=n, m=m, rank=st["rank"], updates=args.updates, ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms),
               whitened_ms=statistics.median(ms_w), accepted_share=float(np.mean(acc)), same_share=float(np.mean(same)),
               failed=st["failed"], steps=args.steps, rounds=args.rounds, iterations_per_s=rates,
               median_iterations_per_s={k: statistics.median(v) for k, v in rates.items()})
    if args.kernel_stats:
        rows = {}
        for r in csv.DictReader(open(args.kernel_stats)):
            for k in CENTRED_KERNELS:
                if k in r["Name"]:
                    d = rows.setdefault(k, dict(calls=0, total_ns=0.0))
                    d["calls"] += int(r["Calls"])
                    d["total_ns"] += float(r["TotalDurationNs"])
        calls = rows.get("amp_centred_update_kernel", {}).get("calls", 0)
        if calls:
            for k, d in rows.items():
                d["us_per_call_of_draw"] = d["total_ns"] / calls / 1e3
            up = rows["amp_centred_update_kernel"]
            moved = (4.0 + 3.0 * rec["accepted_share"]) * 8.0 * n * m
            up.update(bytes=moved, tb_per_s=moved / (up["total_ns"] / calls * 1e-9) / 1e12)
        rec["kernels"] = rows
    full = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    if "ell_delta_kernel" in full:
        rec["ell_delta_kernel_tb_per_s"] = full["ell_delta_kernel"]["tb_per_s"]
    if args.headline_this and args.headline_parent:
        rec["headline"] = dict(this=[float(v) for v in args.headline_this.split(",")],
                               parent=[float(v) for v in args.headline_parent.split(",")])
    full["centred"] = rec
    txt = json.dumps(full, indent=1, default=float)
    print(json.dumps(rec, indent=1, default=float))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--readme", default=None)
    ap.add_argument("--from", dest="record", default=None)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--updates", type=int, default=40)
    ap.add_argument("--headline-this", default=None)
    ap.add_argument("--headline-parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--centred", action="store_true")
    ap.add_argument("--centred-profile", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    if args.centred or args.centred_profile:
        centred(args)
        return
    if args.record:
        write_readme(args.readme, json.load(open(args.record)))
        return

    import numpy as np
    from gpirt_amd import Sampler, amp as A, ell as E
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    n, m = args.n, args.m
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, seed=1, preset="fast")
    s.init()
    for _ in range(args.warmup):
        s.step()
    s.check()
    # (b) the step loop, fixed amplitudes on against off
    ones = np.ones(m)
    rates = {"on": [], "off": []}
    for _ in range(args.rounds):
        for name in ("on", "off"):
            s.amp_set(ones if name == "on" else None)
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
            s.check()
            rates[name].append(args.steps / (time.perf_counter() - t0))
    s.amp_set(None)
    # (c) the update kernel
    nm8 = 8.0 * n * m

    def timed(updates, step_between):
        ms, share = [], []
        for _ in range(updates):
            if step_between:
                s.step()
                s.check()
            before = s.amp()["accepted"]
            s.draw_amp()
            ms.append(float(s.amp_get("time")[0]))
            share.append((s.amp()["accepted"] - before) / m)
        t, sh = statistics.median(ms), float(np.mean(share))
        moved = (3.0 + 2.0 * sh) * nm8
        return dict(updates=updates, ms=t, ms_min=min(ms), ms_max=max(ms), accepted_share=sh, bytes=moved, tb_per_s=moved / (t * 1e-3) / 1e12)

    s.enable_timing(True)
    lo, hi, points, width = 0.1, 10.0, 129, 4
    s.amp_enable(lo, hi, points, None, width)
    for _ in range(5):
        s.draw_amp()
    update = timed(args.updates, True)
    k0 = A.nearest_one(A.grid(lo, hi, points))
    s.amp_enable(lo, hi, points, -1e6 * np.abs(np.arange(points) - k0), width, k0)
    all_rejected = timed(args.updates, False)
    s.amp_enable(lo, hi, points, 1e6 * np.arange(points), 1, 4)
    upward = timed(args.updates, False)
    s.amp_enable(on=False)
    # the yardstick: the length-scale update's delta kernel, a step before each
    s.close()
    h.close()
    g = E.grid(0.7, 2.8, 65)
    ke = int(np.argmin(np.abs(np.log(g))))
    h = Handle(0, kernel=dict(family="se", length_scale=float(g[ke])))
    s = Sampler(h, y, th0, seed=1, preset="fast")
    s.init()
    s.ell_enable(0.7, 2.8, 65, None, 4, ke)
    for _ in range(args.warmup):
        s.step()
    s.check()
    s.enable_timing(True)
    from gpirt_amd import _lib
    dms = []
    for _ in range(max(args.updates // 2, 5)):
        s.step()
        s.check()
        s.draw_ell()
        if s.ell()["last"] != "out_of_range":
            dms.append(float(s.ell_get("times")[_lib.ELL_PARTS.index("delta")]))
    s.enable_timing(False)
    s.check()
    s.close()
    h.close()
    dt = statistics.median(dms)
    delta = dict(updates=len(dms), ms=dt, ms_min=min(dms), ms_max=max(dms), bytes=4.0 * nm8, tb_per_s=4.0 * nm8 / (dt * 1e-3) / 1e12)
    rec = dict(n=n, m=m, steps=args.steps, rounds=args.rounds, grid=dict(lo=lo, hi=hi, points=points, width=width),
               iterations_per_s=rates, median_iterations_per_s={k: statistics.median(v) for k, v in rates.items()},
               update=update, all_rejected=all_rejected, upward_accepted=upward, ell_delta_kernel=delta,
               verdict=verdict(all_rejected, upward, delta))
    if args.headline_this and args.headline_parent:
        rec["headline"] = dict(this=[float(v) for v in args.headline_this.split(",")],
                               parent=[float(v) for v in args.headline_parent.split(",")])
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    if args.readme:
        write_readme(args.readme, json.loads(txt))


if __name__ == "__main__":
    main()
