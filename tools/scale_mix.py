"""What a chain gains from the collapsed scale and shift move, in tools/beta_mix.py's configuration
exactly: 2048 x 256 synthetic answers of which the odd items carry a bump, four chains, 400 + 600 iterations, every iteration a
consistent step followed by draw_beta_centred, the same seeds both ways.

  python tools/scale_mix.py --out profiles/scale_mix.json [--large]
      for update="none" (beta_mix's "both" chain) and "both" (the scale and the shift inside every step): per chain the acceptance
      of the sampling phase and the adapted widths; the quartiles, the worst and the count above 1.05 of the slopes' and the
      intercepts' split-R-hat, the quartiles of Geyer's ESS; the same for S = mean_j log|b1_j|, sd(theta) and mean(theta); ESS per
      second.  --large adds one chain of 100 + 100 at 8192 x 1024 for the acceptance rate alone.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--bump", type=float, default=1.5)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--samples", type=int, default=600)
    ap.add_argument("--burn", type=int, default=400)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    from amp_mix import make
    from gpirt_amd import scale as SC
    y, _ = make(args.n, args.m, args.bump, 20240)
    q = lambda x: [float(v) for v in np.nanquantile(x, (0.25, 0.5, 0.75))]                 # noqa: E731
    rec = dict(n=args.n, m=args.m, chains=args.chains, samples=args.samples, burn=args.burn, draws=args.chains * args.samples,
               consistent=True)
    for mode in ("none", "both"):
        res = SC.run(y, args.samples, args.burn, chains=args.chains, seed=args.seed, update=mode, consistent=True)
        d = res["diag"]
        rows = {}
        for k, name in enumerate(("intercept", "slope")):
            r, e = d["beta"]["rhat"][k], d["beta"]["ess"][k]
            rows[name] = dict(rhat=dict(quartiles=q(r), worst=float(np.nanmax(r)), above_1_05=int((r > 1.05).sum())),
                              ess=dict(quartiles=q(e), smallest=float(np.nanmin(e))), ess_per_s=float(np.nanmedian(e) / res["seconds"]))
        for name in ("S", "sd_theta", "mean_theta"):
            rows[name] = dict(rhat=float(d[name]["rhat"]), ess=float(d[name]["ess"]), ess_per_s=float(d[name]["ess"]) / res["seconds"],
                              chain_means=[float(v) for v in res["series"][name].mean(axis=1)])
        rec[mode] = dict(rows, seconds=res["seconds"], counts=res["counts"])
    if args.large:
        from gpirt_amd.synthetic import make_responses
        yl, th0 = make_responses(8192, 1024, seed=20240)
        res = SC.run(yl, 100, 100, chains=1, seed=args.seed, update="both", consistent=True, theta_init=th0[None, :])
        rec["large"] = dict(n=8192, m=1024, samples=100, burn=100, counts=res["counts"], seconds=res["seconds"])
    print(json.dumps(rec, indent=1, default=float))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1, default=float) + "\n")


if __name__ == "__main__":
    main()
