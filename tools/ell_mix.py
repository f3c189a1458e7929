"""Does the centred length-scale update, or the two interleaved, mix ell better than the whitened one alone?  (gpirt_amd.ell,
DESIGN.md section 34.)

  python tools/ell_mix.py --out profiles/ell_mix.json
      one data set, make_responses(--n, --m) (2048 x 256), a fine grid --lo .. --hi in --points points (0.5 .. 2 in 1025),
      kstar_rank as gpirt_amd.kernel.fast_rank gives it at lo, --chains chains with the same seeds for each of
      update = "whitened", "centred" and "both" of ell.run (one update, or the two in that order, after every step; the burn-in
      retunes each width from its own acceptance).  Per mode: the sampling phase's acceptance per kind and chain, the adapted
      widths, R-hat and ESS of log ell (ell.summarise), mean and sd of ell, the wall time of the whole run and ESS per second.
      Nothing is stored per draw but the index (store_draws=False).
  python tools/ell_mix.py --fixed-theta 600 --out profiles/ell_mix_fixed_theta.json
      the control: the same data and grid, theta held at its starting value -- draw_f(), draw_beta(), skip_factor() and one
      update, 600 times, for the whitened and the centred update each from the grid's middle.  step() reuses f after theta has
      moved (the reference's quirk Q3), so f is not the GP's value at the current theta; with theta fixed it is.
      Per kind: the index at the start, after a third of the run and at the end, its range over the last third, the acceptance.
  python tools/ell_mix.py --consistent --out profiles/ell_mix_consistent.json
      the three modes again with ell.run(consistent=True): every iteration is Sampler.step(consistent=True), which carries f to
      the new theta with the model's nugget (gpirt_amd.consistent) -- the state the centred update's prior density assumes.
      Per mode also Q: one more chain of the same configuration (the first chain's seed, the starting width, no retuning)
      driven by hand, with the mean over items of Sampler.prior_quad() every 50 steps and the index beside it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def q_probe(args, y, rank, mode, every=50):
    """Q = prior_quad().mean() and the index every `every` steps of one hand-driven chain of ell.run's configuration"""
    import numpy as np
    from gpirt_amd import Sampler, _lib, chains as CH, ell as E
    from gpirt_amd.ops import Handle
    g = E.grid(args.lo, args.hi, args.points)
    k0 = int(np.argmin(np.abs(np.log(g))))
    h = Handle(0, kernel=dict(family="se", length_scale=float(g[k0])))
    s = Sampler(h, y, CH.default_inits(args.n, 1, args.seed)[0], seed=args.seed, rng="item", theta_stabilise=True, fstar_fused=True,
                kstar_rank=rank)
    s.init()
    s.ell_enable(args.lo, args.hi, args.points, None, args.width, k0)
    kinds = {"whitened": ("whitened",), "centred": ("centred",), "both": _lib.ELL_KINDS}[mode]
    out = []
    for it in range(1, args.burn + args.samples + 1):
        s.step(consistent=args.consistent)
        for kd in kinds:
            s.draw_ell(kd)
        if it % every == 0:
            out.append(dict(step=it, Q=float(s.prior_quad().mean()), index=int(s.ell()["index"])))
    s.check()
    s.close()
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--lo", type=float, default=0.5)
    ap.add_argument("--hi", type=float, default=2.0)
    ap.add_argument("--points", type=int, default=1025)
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--burn", type=int, default=600)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--modes", default="whitened,centred,both")
    ap.add_argument("--fixed-theta", type=int, default=0)
    ap.add_argument("--consistent", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    from gpirt_amd import ell as E, kernel as K
    from gpirt_amd.synthetic import make_responses
    y, _ = make_responses(args.n, args.m, seed=20240)
    rank = K.fast_rank(dict(family="se", length_scale=args.lo))
    rec = dict(n=args.n, m=args.m, grid=dict(lo=args.lo, hi=args.hi, points=args.points), width_start=args.width, chains=args.chains,
               samples=args.samples, burn=args.burn, seed=args.seed, kstar_rank=rank, consistent=bool(args.consistent), modes={})
    if args.fixed_theta:
        from gpirt_amd import Sampler
        from gpirt_amd.ops import Handle
        _, th0 = make_responses(args.n, args.m, seed=20240)
        g = E.grid(args.lo, args.hi, args.points)
        k0, T = args.points // 2, args.fixed_theta
        rec["fixed_theta"] = dict(iterations=T, k0=k0, width=16, kinds={})
        for kind in ("whitened", "centred"):
            h = Handle(0, kernel=dict(family="se", length_scale=float(g[k0])))
            s = Sampler(h, y, th0, seed=args.seed, rng="item", theta_stabilise=True, fstar_fused=True, kstar_rank=rank)
            s.init()
            s.ell_enable(args.lo, args.hi, args.points, None, 16, k0)
            idx = []
            for _ in range(T):
                s.draw_f()
                s.draw_beta()
                s.skip_factor()
                s.draw_ell(kind)
                idx.append(s.ell()["index"])
            s.check()
            e = s.ell() if kind == "whitened" else s.ell()["centred"]
            last = idx[2 * T // 3:]
            rec["fixed_theta"]["kinds"][kind] = dict(index_first=idx[0], index_third=idx[T // 3], index_last=idx[-1], last_third_min=min(last),
                                                     last_third_max=max(last), last_third_mean_ell=float(np.mean(g[last])),
                                                     accept_rate=e["accept_rate"], out_of_range=e["out_of_range"], failed=e["failed"])
            print("fixed theta", kind, json.dumps(rec["fixed_theta"]["kinds"][kind], default=float), flush=True)
            s.close()
            h.close()
    for mode in [v for v in args.modes.split(",") if v]:
        t0 = time.perf_counter()
        res = E.run(y, args.samples, args.burn, chains=args.chains, seed=args.seed, lo=args.lo, hi=args.hi, points=args.points,
                    width=args.width, update=mode, store_draws=False, consistent=args.consistent)
        wall = time.perf_counter() - t0
        e = res["ell"]
        per_kind = (lambda v: {"whitened": v}) if mode == "whitened" else (lambda v: v)
        idx = np.atleast_2d(e["index"])
        rec["modes"][mode] = dict(accept_rate=per_kind(e["accept_rate"]), width=per_kind(e["width"]), counts=per_kind(e["counts"]),
                                  rhat=e["rhat"], ess=e["ess"], mean=e["mean"], sd=e["sd"], mode=e["mode"],
                                  quantiles={str(k): v for k, v in e["quantiles"].items()},
                                  index_first=[int(v) for v in idx[:, 0]], index_last=[int(v) for v in idx[:, -1]],
                                  index_min=int(idx.min()), index_max=int(idx.max()), distinct_indices=int(np.unique(idx).size),
                                  wall_s=wall, ess_per_s=e["ess"] / wall if np.isfinite(e["ess"]) else None)
        if args.consistent:
            rec["modes"][mode]["prior_quad"] = q_probe(args, y, rank, mode)
        print(mode, json.dumps(rec["modes"][mode], default=float), flush=True)
    txt = json.dumps(rec, indent=1, default=float)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
