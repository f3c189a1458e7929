"""What the quantile accumulators (GPIRT_SUM_THETA_HIST, GPIRT_SUM_IRF_BAND, csrc/summary.hip) cost at the metric size,
8192 x 1024, with gpirt_fast_options().

  python tools/quantile_cost.py --out FILE.json
      in one process, alternating, R rounds of K steps each: the steady step loop; + summary_accumulate with
      WAIC + pred + DIAG; with WAIC + pred + DIAG + THETA_HIST + IRF_BAND (DIAG planned for a long chain).  Then
      gpirt_summary_quantiles of C = 4 state blocks, three probabilities, every output copied to the host.
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/quantile_cost.py --kernel-only
      the histogram kernel alone, 20 launches, then one quantile extraction of C = 4 blocks;
  python tools/quantile_cost.py --trace DIR --merge FILE.json
      the kernels' median durations from that trace; for the histogram kernel its rate on the algorithmic bytes (f* and
      theta read once, each cell's plogis sum read and written, one 4-byte counter read and written per cell and
      respondent; the edges are in LDS).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANNED = 1_000_000
PROBS = (0.025, 0.5, 0.975)
KERNELS = {"hist": "summary_hist_accumulate_kernel<true, true>", "theta": "quantile_theta_kernel",
           "irf": "quantile_irf_kernel"}


def parts_of(form):
    from gpirt_amd import _lib
    p = _lib.SUM_WAIC | _lib.SUM_PRED | _lib.SUM_DIAG
    if form == "waic_pred_diag_qnt":
        p |= _lib.SUM_THETA_HIST | _lib.SUM_IRF_BAND
    return p


def algorithmic_bytes(n, m):
    nm = 1001 * m
    return 8.0 * nm + 8.0 * n + 2 * 8.0 * nm + 2 * 4.0 * nm + 2 * 4.0 * 2 * n


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


def states(s, chains):
    """C copies of one complete chain's block with every part (the cost does not depend on the values)"""
    import torch
    s.summary_enable(parts_of("waic_pred_diag_qnt"), planned_draws=4)
    for _ in range(4):
        s.step()
        s.summary_accumulate()
    s.check()
    st = s.summary_state()
    blocks = [st.clone() for _ in range(chains)]
    torch.cuda.synchronize()
    return st, blocks


def timing(args):
    from gpirt_amd import quantiles as Q
    n, m = args.n, args.m
    h, s = sampler(n, m)
    for _ in range(args.warmup):
        s.step()
    s.check()
    forms = ("plain", "waic_pred_diag", "waic_pred_diag_qnt")
    rates = {k: [] for k in forms}
    for _ in range(args.rounds):
        for form in forms:
            if form == "plain":
                s.summary_enable(0)
            else:
                s.summary_enable(parts_of(form), planned_draws=PLANNED)
            s.check()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if form != "plain":
                    s.summary_accumulate()
            s.check()
            rates[form].append(args.steps / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in rates.items()}
    rec = dict(n=n, m=m, options="gpirt_fast_options", rounds=args.rounds, steps_per_round=args.steps,
               iterations_per_s=rates, median_iterations_per_s=med,
               ratio_qnt_to_waic_pred_diag=med["waic_pred_diag_qnt"] / med["waic_pred_diag"],
               ratio_qnt_to_plain=med["waic_pred_diag_qnt"] / med["plain"],
               targets=dict(ratio_qnt_to_waic_pred_diag=0.99, ratio_qnt_to_plain=0.965))
    st, blocks = states(s, args.chains)
    walls = []
    for _ in range(args.extractions):
        t0 = time.perf_counter()
        Q.from_states(h, blocks, PROBS)
        walls.append(time.perf_counter() - t0)
    rec["extraction"] = dict(chains=args.chains, probs=PROBS, state_block_bytes=int(st.numel() * 8), wall_s=walls,
                             median_wall_s=statistics.median(walls), target_s=0.1)
    s.summary_enable(0)
    s.close()
    h.close()
    return rec


def kernel_only(args):
    from gpirt_amd import quantiles as Q
    h, s = sampler(args.n, args.m)
    s.step()
    s.summary_enable(parts_of("waic_pred_diag_qnt"), planned_draws=PLANNED)
    for _ in range(args.launches):
        s.summary_accumulate()
    s.check()
    _, blocks = states(s, args.chains)
    Q.from_states(h, blocks, PROBS)
    s.summary_enable(0)
    s.close()
    h.close()


def from_trace(args):
    f = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    out = {}
    for key, name in KERNELS.items():
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if not us:
            raise SystemExit(f"no {name} in {f}")
        out[key] = dict(kernel=name, launches=len(us), median_us=statistics.median(us), min_us=min(us))
    b = algorithmic_bytes(args.n, args.m)
    med = out["hist"]["median_us"]
    out["hist"].update(algorithmic_bytes=b, tb_per_s=b / (med * 1e-6) / 1e12, fraction_of_6_3_tb_per_s=b / (med * 1e-6) / 6.3e12,
                       target_us=60.0)
    rec = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
    rec["kernels"] = out
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--extractions", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_only:
        kernel_only(args)
        return
    rec = from_trace(args) if args.trace else timing(args)
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    out = args.out or args.merge
    if out:
        with open(out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
