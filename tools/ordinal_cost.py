"""What ordinal responses cost at the metric size, 8192 x 1024, with the fast options and C = 5 (csrc/ordinal.hip,
gpirt_amd.ordinal).

  python tools/ordinal_cost.py --out profiles/ordinal_cost.json
      one sampler, one process, gpirt_fast_options(), all by the sampler's stage events (Sampler.enable_timing):
      (a) draw_f, theta_partial ("theta_gemm") and draw_beta with ordinal on against the same sampler with it off, --rounds
          alternating rounds of --steps steps each (ordinal is enabled and turned off again between the rounds; with it on
          every step is followed by draw_thresholds, so that the chain is the ordinal one);
      (b) draw_thresholds alone at W = --width (ordinal_stats()["time_ms"]);
      with the bytes and ll evaluations each launch makes and the rate that implies.
  python tools/ordinal_cost.py --out ... --headline-this a,b,c --headline-parent a,b,c [--headline-this ... --headline-parent ...]
                                       --headline-flags "..." --z-ordinal z --z-binary z
      also records bench.py's headline (three alternating runs each on this commit and its parent, one --headline-this /
      --headline-parent pair per session, as given with the flags they were run with: bench.py enables none of this) and the
      two Fisher z of tests/test_gpu_ordinal.py's chain, as given.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--categories", type=int, default=5)
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--headline-this", action="append", default=[])
    ap.add_argument("--headline-parent", action="append", default=[])
    ap.add_argument("--headline-flags", default="")
    ap.add_argument("--z-ordinal", type=float, default=None)
    ap.add_argument("--z-binary", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    from gpirt_amd import Sampler
    from gpirt_amd import ordinal as OR
    from gpirt_amd.ops import Handle
    n, m, C, W = args.n, args.m, args.categories, args.width
    d = OR.make_graded(n, m, C, seed=20240)
    cat = d["cat"]
    y = OR.dichotomise(cat)
    t = OR.grid()
    K0 = OR.init_thresholds(cat, t, C)
    h = Handle(0)
    s = Sampler(h, y, d["theta"], seed=1, preset="fast")
    s.init()
    for _ in range(args.warmup):
        s.step()
    s.check()
    s.enable_timing(True)
    stages = {"on": {}, "off": {}}
    thr_ms, ks = [], []
    for _ in range(args.rounds):
        for mode in ("on", "off"):
            if mode == "on":
                s.ordinal_enable(cat, C, K0=K0, width=W)
            for it in range(args.steps):
                s.step()
                if mode == "on":
                    s.draw_thresholds()
                    thr_ms.append(s.ordinal_stats()["time_ms"])
                    ks.append(float(s.get("ess_k").mean()))
                if it >= 2:                                   # (the first steps after a switch still see the other model's state)
                    for k, v in s.stage_times().items():
                        stages[mode].setdefault(k, []).append(v)
            s.check()
            if mode == "on":
                K0 = s.ordinal_get("index")
                lp, counts = s.ordinal_get("lp"), s.ordinal_get("counts")
                st = s.ordinal_stats()
                s.ordinal_enable(None)
    s.enable_timing(False)
    s.close()
    h.close()

    def med(v):
        return dict(calls=len(v), ms=statistics.median(v), ms_min=min(v), ms_max=max(v))
    obs = int((cat > 0).sum())
    terms = int(OR.n_terms(cat, C))
    kbar = statistics.mean(ks)
    # one pass of the slice = `terms` ll evaluations; an item makes 1 + (1 + k) screened passes and, inside the band, exact ones
    passes = 2.0 + kbar
    f_on = med(stages["on"]["draw_f"])
    # first touch: f, nu, mu read, f written, cat read.  Beyond that the 512-lane class (2048 < n <= 8192) reads mu again in
    # every pass and the 1024-lane class (n > 8192) f, nu, mu and cat; counted for the screened passes, the exact ones inside
    # the screen's band come on top (they are not counted by the kernel)
    f_first = 8.0 * n * m * 4 + 1.0 * n * m
    per_pass = 0.0 if n <= 2048 else (8.0 * n * m if n <= 8192 else 25.0 * n * m)
    f_bytes = f_first + per_pass * passes
    cand = np.isfinite(lp).sum(axis=2)                         # candidates of the last update, m x (C - 1)
    thr_evals = float(sum((cand[:, c] * (counts[:, c] + counts[:, c + 1])).sum() for c in range(C - 1)))
    thr = med(thr_ms)
    g_ms = med(stages["on"]["theta_gemm"])
    out = dict(
        n=n, m=m, categories=C, width=W, steps=args.steps, rounds=args.rounds, observed_cells=obs, ll_terms_per_pass=terms,
        stages_ms={mode: {k: med(v) for k, v in stages[mode].items()} for mode in stages},
        draw_f=dict(mean_rejections=kbar, screened_passes_per_item=passes, ll_evaluations=terms * passes, bytes=f_bytes,
                    bytes_first_touch=f_first, bytes_reread_per_pass=per_pass,
                    note="draw_f's stage also holds nu = L Z; the slice launch is the part that differs",
                    g_ll_per_s=terms * passes / (f_on["ms"] * 1e-3) / 1e9),
        theta_partial=dict(table_ll_evaluations=1001 * m * (2 * C - 2), gemm_flops=2.0 * 1001 * n * C * m,
                           bytes=8.0 * (1001 * C * m + n * C * m + 1001 * n),
                           tflops=2.0 * 1001 * n * C * m / (g_ms["ms"] * 1e-3) / 1e12),
        draw_beta=dict(ll_evaluations=2 * terms, bytes=(8.0 * 2 + 1.0) * n * m + 8.0 * n * m + 8.0 * 1001 * m),
        draw_thresholds=dict(**thr, ll_evaluations=thr_evals, bytes=(8.0 * 2 + 1.0) * n * m,
                             g_ll_per_s=thr_evals / (thr["ms"] * 1e-3) / 1e9, pinned=st["pinned"], failed=st["failed"],
                             updates=st["updates"]))
    if args.headline_this or args.headline_parent:
        if len(args.headline_this) != len(args.headline_parent):
            raise SystemExit("--headline-this and --headline-parent come in pairs, one per session")
        out["bench_headline_iterations_per_s"] = dict(
            flags=args.headline_flags,
            sessions=[dict(this=[float(x) for x in a.split(",")], parent=[float(x) for x in b.split(",")])
                      for a, b in zip(args.headline_this, args.headline_parent)])
    if args.z_ordinal is not None and args.z_binary is not None:
        out["recovery_fisher_z"] = dict(ordinal=args.z_ordinal, binary=args.z_binary, n=512, margin=2 / (512 - 3) ** 0.5,
                                        source="tests/test_gpu_ordinal.py::test_a_chain_recovers_theta_no_worse_than_the_dichotomised_run")
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
