"""What a chain gains from the centred beta update, in tools/amp_mix.py's configuration: 2048 x 256
synthetic answers of which the odd items carry a bump, four chains, 400 + 600 iterations, every iteration a consistent step.

  python tools/beta_mix.py --out profiles/beta_centred.json
      ADDS the record "mix" to the file at --out, everything else of it left as it is: for update="both" (the move after every
      step) and "mh" (the chain without it, same seeds), per row of beta (intercept, slope) the quartiles, the worst and the
      count above 1.05 of split-R-hat, the quartiles and the smallest of Geyer's ESS (of chains x samples draws), the wall time of
      the chains' loops and the median ESS per second.
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    from amp_mix import make
    from gpirt_amd import beta as Bt
    y, _ = make(args.n, args.m, args.bump, 20240)
    q = lambda x: [float(v) for v in np.nanquantile(x, (0.25, 0.5, 0.75))]                 # noqa: E731
    rec = dict(n=args.n, m=args.m, chains=args.chains, samples=args.samples, burn=args.burn, draws=args.chains * args.samples,
               consistent=True)
    for mode in ("both", "mh"):
        res = Bt.run(y, args.samples, args.burn, chains=args.chains, seed=args.seed, update=mode, consistent=True, store_draws=False)
        e = res["beta"]
        rows = {}
        for k, name in enumerate(("intercept", "slope")):
            rows[name] = dict(rhat=dict(quartiles=q(e["rhat"][k]), worst=float(np.nanmax(e["rhat"][k])),
                                        above_1_05=int((e["rhat"][k] > 1.05).sum())),
                              ess=dict(quartiles=q(e["ess"][k]), smallest=float(np.nanmin(e["ess"][k]))),
                              ess_per_s=float(np.nanmedian(e["ess"][k]) / e["seconds"]))
        rec[mode] = dict(rows, seconds=e["seconds"], calls=e["calls"], updates=e["updates"], failed=e["failed"], rank=e["rank"])
    full = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {}
    full["mix"] = rec
    print(json.dumps(rec, indent=1, default=float))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(full, indent=1, default=float) + "\n")


if __name__ == "__main__":
    main()
