"""What the collapsed scale and shift move costs (csrc/scale.hip), on one device at 8192 x 1024 under
gpirt_fast_options().

  python tools/scale_cost.py --out profiles/scale_cost.json [--headline-this a,b,.. --headline-parent a,b,..]
      - one gpirt_sampler_draw_scale of each kind between theta_partial and theta_finish of a consistent step's stages, median of
        --updates by the sampler's event timing: the whole call and its parts (curve, product, logz, decide, commits);
      - the yardstick, the same run's theta_partial stage time: the move contains one such product plus five small launches;
      - scale_logz_kernel's bytes (2 x 8 N n read) and TB/s, beside ell_delta_kernel (4 x 8 n m read) timed in the same run;
      - the consistent step loop with the move (both kinds) against without, --rounds alternating rounds of --steps steps;
      - bench.py's headline on this commit and on its parent as given on the command line (measured alternating in one session).
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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--updates", type=int, default=40)
    ap.add_argument("--headline-this", default=None)
    ap.add_argument("--headline-parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    from gpirt_amd import Sampler, _lib, ell as E
    from gpirt_amd.ops import Handle
    from gpirt_amd.sampler import NGRID
    from gpirt_amd.synthetic import make_responses
    n, m = args.n, args.m
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, seed=1, preset="fast")
    s.init()
    s.scale_enable()
    both = ("scale", "shift")
    for _ in range(args.warmup):
        s.step(consistent=True, scale=both)
    s.check()
    s.enable_timing(True)
    parts = {kd: {k: [] for k in _lib.SCALE_TIMES} for kd in both}
    partial = []
    for _ in range(args.updates):
        s.step(consistent=True)
        partial.append(float(s.stage_times()["theta_gemm"]))
        s.check()
        s.draw_f(); s.draw_fstar(); s.theta_partial()
        for kd in both:
            s.draw_scale(kd)
            for k, v in s.scale_get("times").items():
                parts[kd][k].append(v)
        s.theta_finish(); s.carry_f(); s.draw_beta(); s.factor()
    s.enable_timing(False)
    rates = {"both": [], "none": []}
    for _ in range(args.rounds):
        for name in ("both", "none"):
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step(consistent=True, scale=both if name == "both" else None)
            s.check()
            rates[name].append(args.steps / (time.perf_counter() - t0))
    st = s.scale()
    s.close()
    h.close()
    # the yardstick for the bandwidth: the length-scale update's delta kernel, a step before each, in the same process
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
    med = lambda v: dict(ms=statistics.median(v), ms_min=min(v), ms_max=max(v))          # noqa: E731
    lz_bytes, dt = 2.0 * 8.0 * NGRID * n, statistics.median(dms)
    tp = statistics.median(partial)
    rec = dict(n=n, m=m, updates=args.updates, theta_partial=med(partial), counts={kd: st[kd] for kd in both})
    for kd in both:
        t = {k: med(v) for k, v in parts[kd].items()}
        t["ratio_to_theta_partial"] = t["whole"]["ms"] / tp
        t["logz"].update(bytes=lz_bytes, tb_per_s=lz_bytes / (t["logz"]["ms"] * 1e-3) / 1e12)
        t["commits"].update(bytes_if_accepted=2.0 * 8.0 * NGRID * n + 8.0 * (5 * NGRID * m + n * m))
        t["curve"].update(bytes=8.0 * 4 * NGRID * m)
        rec[kd] = t
    rec["ell_delta_kernel"] = dict(updates=len(dms), ms=dt, ms_min=min(dms), ms_max=max(dms), bytes=4.0 * 8.0 * n * m,
                                   tb_per_s=4.0 * 8.0 * n * m / (dt * 1e-3) / 1e12)
    rec.update(steps=args.steps, rounds=args.rounds, iterations_per_s=rates,
               median_iterations_per_s={k: statistics.median(v) for k, v in rates.items()})
    if args.headline_this and args.headline_parent:
        rec["headline"] = dict(this=[float(v) for v in args.headline_this.split(",")],
                               parent=[float(v) for v in args.headline_parent.split(",")])
    print(json.dumps(rec, indent=1, default=float))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1, default=float) + "\n")


if __name__ == "__main__":
    main()
