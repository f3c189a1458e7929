"""What the centred beta update costs (csrc/beta_centred.hip), on one device at 8192 x 1024 under
gpirt_fast_options().

  python tools/beta_cost.py --out profiles/beta_centred.json [--headline-this a,b,.. --headline-parent a,b,..]
      ADDS the record "cost" to the file at --out, everything else of it left as it is:
      - one gpirt_sampler_draw_beta_centred after a consistent step each, median of --updates by the sampler's event timing: the
        whole call ("time") and its per-item kernel ("time_item");
      - the per-item kernel's bytes (f read and written once, mu written once: 3 x 8 n m; mu_star's 8 N m and the shared W on
        top are named apart) and TB/s, beside ell_delta_kernel (4 x 8 n m read) timed in the same run;
      - the consistent step loop with the move against without, --rounds alternating rounds of --steps steps in one process;
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
    for _ in range(args.warmup):
        s.step(consistent=True)
        s.draw_beta_centred()
    s.check()
    s.enable_timing(True)
    ms, ms_item = [], []
    for _ in range(args.updates):
        s.step(consistent=True)
        s.check()
        s.draw_beta_centred()
        ms.append(float(s.beta_centred_get("time")[0]))
        ms_item.append(float(s.beta_centred_get("time_item")[0]))
    s.enable_timing(False)
    rates = {"both": [], "mh": []}
    for _ in range(args.rounds):
        for name in ("both", "mh"):
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step(consistent=True)
                if name == "both":
                    s.draw_beta_centred()
            s.check()
            rates[name].append(args.steps / (time.perf_counter() - t0))
    st = s.beta_centred()
    s.close()
    h.close()
    # the yardstick: the length-scale update's delta kernel, a step before each, in the same process
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
    nm8 = 8.0 * n * m
    t_item, dt = statistics.median(ms_item), statistics.median(dms)
    rec = dict(n=n, m=m, rank=st["rank"], updates=args.updates, failed=st["failed"],
               call_ms=statistics.median(ms), call_ms_min=min(ms), call_ms_max=max(ms),
               item_kernel=dict(ms=t_item, ms_min=min(ms_item), ms_max=max(ms_item), bytes=3.0 * nm8, tb_per_s=3.0 * nm8 / (t_item * 1e-3) / 1e12,
                                mu_star_bytes=8.0 * NGRID * m, shared_bytes_per_item=8.0 * 3 * n),
               ell_delta_kernel=dict(updates=len(dms), ms=dt, ms_min=min(dms), ms_max=max(dms), bytes=4.0 * nm8,
                                     tb_per_s=4.0 * nm8 / (dt * 1e-3) / 1e12),
               steps=args.steps, rounds=args.rounds, iterations_per_s=rates,
               median_iterations_per_s={k: statistics.median(v) for k, v in rates.items()})
    if args.headline_this and args.headline_parent:
        rec["headline"] = dict(this=[float(v) for v in args.headline_this.split(",")],
                               parent=[float(v) for v in args.headline_parent.split(",")])
    full = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    full["cost"] = rec
    print(json.dumps(rec, indent=1, default=float))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(full, indent=1, default=float) + "\n")


if __name__ == "__main__":
    main()
