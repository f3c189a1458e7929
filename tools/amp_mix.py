"""Do the sampled amplitudes tell items that need a nonparametric curve from items that are 2PL items?  (gpirt_amd.amp,
DESIGN.md section 37.)

  python tools/amp_mix.py --out profiles/amp_mix.json
      a synthetic set of --n respondents and --m items (2048 x 256): theta ~ N(0, 1); the even items are exactly linear in the
      logit, beta_0 + beta_1 theta; the odd items carry a bump of --bump logits (1.5) on top, bump exp(-(theta - c)^2 / (2 0.5^2))
      with c spread over -1.5 .. 1.5.  --chains chains (4) of amp.run on the default grid (0.1 .. 10, 129 points, width 4), one
      update after every step, the burn-in retuning each item's width.  Reported as measured: the sampling phase's acceptance per
      item (pooled over the chains: mean, min, max), the adapted widths, R-hat and ESS of log a_j (quartiles and the worst), the
      posterior mean amplitude of the two halves (mean, quartiles), how often a bumped item's posterior mean exceeds a linear
      item's (the AUC of the posterior mean as a classifier of the halves) and the same for P(a_j <= 1), the wall time.
  python tools/amp_mix.py --consistent --update both --out profiles/amp_mix_centred.json
      the same with every iteration a consistent step and the centred update beside the whitened one (--update whitened, centred
      or both): the record also names the mode and carries the centred update's counters and acceptance.
      The defaults (--update whitened, no --consistent) reproduce the first run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(n, m, bump, seed):
    """y (n x m of +1 / -1), and which items carry the bump"""
    import numpy as np
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal(n)
    b0, b1 = rng.normal(0, 0.7, m), rng.normal(1.0, 0.3, m)
    bumped = np.arange(m) % 2 == 1
    centre = np.linspace(-1.5, 1.5, m)
    g = b0[None, :] + b1[None, :] * theta[:, None]
    g = g + np.where(bumped[None, :], bump * np.exp(-(theta[:, None] - centre[None, :]) ** 2 / (2 * 0.5 ** 2)), 0.0)
    y = np.where(rng.random((n, m)) < 1 / (1 + np.exp(-g)), 1.0, -1.0)
    return y, bumped


def auc(a, b):
    """P(a value of `a` exceeds a value of `b`), ties counted half"""
    import numpy as np
    a, b = np.asarray(a)[:, None], np.asarray(b)[None, :]
    return float(((a > b) + 0.5 * (a == b)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--bump", type=float, default=1.5)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--samples", type=int, default=600)
    ap.add_argument("--burn", type=int, default=400)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--update", default="whitened", choices=("whitened", "centred", "both"))
    ap.add_argument("--consistent", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    from gpirt_amd import amp as A
    y, bumped = make(args.n, args.m, args.bump, 20240)
    t0 = time.perf_counter()
    res = A.run(y, args.samples, args.burn, chains=args.chains, seed=args.seed, store_draws=False, update=args.update,
                consistent=args.consistent)
    wall = time.perf_counter() - t0
    e = res["amp"]
    g = e["grid"]
    one = int(np.searchsorted(g, 1.0, side="right")) - 1
    p_le_1 = e["p_below"][one]
    q = lambda v: [float(x) for x in np.nanquantile(np.asarray(v, dtype=np.float64), [0.0, 0.25, 0.5, 0.75, 1.0])]       # noqa: E731
    acc = e["accept_rate"]
    rec = dict(n=args.n, m=args.m, bump=args.bump, chains=args.chains, samples=args.samples, burn=args.burn, seed=args.seed,
               grid=dict(lo=float(g[0]), hi=float(g[-1]), points=int(g.shape[0])), width_start=4, wall_s=wall,
               accept_rate=dict(mean=float(np.nanmean(acc)), quantiles=q(acc)),
               width=dict(quantiles=q(e["width"]), distinct=[int(v) for v in np.unique(e["width"])]),
               rhat=dict(quantiles=q(e["rhat"]), above_1_05=int((e["rhat"] > 1.05).sum()), above_1_1=int((e["rhat"] > 1.1).sum())),
               ess=dict(quantiles=q(e["ess"]), per_s_median=float(np.nanmedian(e["ess"]) / wall)),
               mean_amplitude=dict(linear=dict(mean=float(e["mean"][~bumped].mean()), quantiles=q(e["mean"][~bumped])),
                                   bumped=dict(mean=float(e["mean"][bumped].mean()), quantiles=q(e["mean"][bumped]))),
               p_amplitude_le_1=dict(linear=q(p_le_1[~bumped]), bumped=q(p_le_1[bumped])),
               separation=dict(auc_posterior_mean=auc(e["mean"][bumped], e["mean"][~bumped]),
                               auc_p_le_1=auc(p_le_1[~bumped], p_le_1[bumped]),
                               bumped_among_top_half=int(bumped[np.argsort(-e["mean"])[: args.m // 2]].sum())),
               counts_total={k: int(e["counts"][:, i].sum()) for i, k in enumerate(("updates", "accepted", "out_of_range", "failed"))},
               smallest=e["smallest"][:5], largest=e["largest"][:5])
    if args.update != "whitened" or args.consistent:
        rec.update(update=args.update, consistent=bool(args.consistent))
    if args.update != "whitened":
        cc = e["counts_centred"]
        rec.update(rank=int(e["rank"]), accept_rate_centred=dict(mean=float(np.nanmean(e["accept_rate_centred"])),
                                                               quantiles=q(e["accept_rate_centred"])),
                   counts_centred_total={k: int(cc[:, i].sum()) for i, k in enumerate(("updates", "accepted", "same", "failed"))})
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
