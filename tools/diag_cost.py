"""What the convergence diagnostics (GPIRT_SUM_DIAG, csrc/summary.hip) cost at the metric size, 8192 x 1024, with
gpirt_fast_options().

  python tools/diag_cost.py --out FILE.json
      in one process, alternating, R rounds of K steps each: the steady step loop; + summary_accumulate with WAIC + pred;
      with WAIC + pred + DIAG; with WAIC + pred + f + DIAG (DIAG planned for a long chain, so every timed draw is in the
      first half and adds to a batch).  Then gpirt_chains_combine of C = 4 state blocks with every part.
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/diag_cost.py --kernel-only
      the accumulate kernel alone, each DIAG form, 20 launches each, for a trace that holds nothing else of note;
  python tools/diag_cost.py --trace DIR --merge FILE.json
      the kernel's median duration from that trace and its rate on the algorithmic bytes: f, mu, y read once, each
      accumulator the draw touches read and written once (WAIC: 3, pred: 1, f: 2, and with DIAG the half's mean and M2 and
      the batch sum, of f too with f), theta and beta with theirs.
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

PLANNED = 1_000_000                  # a long chain: the timed draws sit in half 1, inside a batch of 1000
FORMS = {"waic_pred": ("waic", "pred"), "waic_pred_diag": ("waic", "pred", "diag"), "waic_pred_f_diag": ("waic", "pred", "f", "diag")}
TEMPLATE = {"waic_pred_diag": "summary_diag_accumulate_kernel<true, true, false>",
            "waic_pred_f_diag": "summary_diag_accumulate_kernel<true, true, true>"}
CELL_ACC = {"waic_pred_diag": 4, "waic_pred_f_diag": 6 + 3}
TB_ACC = 2 + 3


def parts_of(form):
    from gpirt_amd import _lib
    names = FORMS[form]
    return _lib.summary_parts([k for k in names if k != "diag"]) | (_lib.SUM_DIAG if "diag" in names else 0)


def enable(s, form):
    if form == "plain":
        s.summary_enable(0)
    elif "diag" in FORMS[form]:
        s.summary_enable(parts_of(form), planned_draws=PLANNED)
    else:
        s.summary_enable(parts_of(form))


def algorithmic_bytes(form, n, m):
    cells, tb = n * m, n + 2 * m
    return 8.0 * (3 * cells + 2 * CELL_ACC[form] * cells + tb + 2 * TB_ACC * tb)


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


def timing(args):
    import torch
    from gpirt_amd import _lib, chains
    n, m = args.n, args.m
    h, s = sampler(n, m)
    for _ in range(args.warmup):
        s.step()
    s.check()
    rates = {"plain": [], **{k: [] for k in FORMS}}
    for _ in range(args.rounds):
        for form in rates:
            enable(s, form)
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
               iterations_per_s=rates, median_iterations_per_s=med, ratio_to_plain={k: med[k] / med["plain"] for k in FORMS},
               targets=dict(waic_pred_diag=0.97, waic_pred_f_diag=0.95))
    # the combine of C = 4 complete state blocks with every part (copies of one chain's block: the cost does not depend on
    # the values); the wall time includes every pooled and diagnostic array's copy to the host
    s.summary_enable(_lib.SUM_WAIC | _lib.SUM_PRED | _lib.SUM_F | _lib.SUM_DIAG, planned_draws=4)
    for _ in range(4):
        s.step()
        s.summary_accumulate()
    s.check()
    st = s.summary_state()
    blocks = [st.clone() for _ in range(args.chains)]
    torch.cuda.synchronize()
    walls = []
    for _ in range(args.combines):
        t0 = time.perf_counter()
        chains.combine(h, blocks)
        walls.append(time.perf_counter() - t0)
    rec["combine"] = dict(chains=args.chains, state_block_bytes=int(st.numel() * 8), wall_s=walls,
                          median_wall_s=statistics.median(walls))
    s.summary_enable(0)
    s.close()
    h.close()
    return rec


def kernel_only(args):
    h, s = sampler(args.n, args.m)
    s.step()
    for form in TEMPLATE:
        enable(s, form)
        for _ in range(args.launches):
            s.summary_accumulate()
        s.check()
    s.summary_enable(0)
    s.close()
    h.close()


def from_trace(args):
    f = glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(f)))
    out = {}
    for form, name in TEMPLATE.items():
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        if not us:
            raise SystemExit(f"no {name} in {f}")
        med = statistics.median(us)
        b = algorithmic_bytes(form, args.n, args.m)
        out[form] = dict(launches=len(us), median_us=med, min_us=min(us), algorithmic_bytes=b,
                         tb_per_s=b / (med * 1e-6) / 1e12, fraction_of_6_3_tb_per_s=b / (med * 1e-6) / 6.3e12, target=0.7)
    rec = json.load(open(args.merge)) if args.merge and os.path.exists(args.merge) else {}
    rec["accumulate_kernel"] = out
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
    ap.add_argument("--combines", type=int, default=3)
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
