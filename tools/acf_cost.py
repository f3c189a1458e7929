"""What the autocorrelation block (csrc/acf.hip) costs at the metric size, 8192 x 1024, with gpirt_fast_options() and L = 256.

  python tools/acf_cost.py --out profiles/acf_cost.json
      in one process: the state is enabled once for a long chain and filled with L + 4 draws, so that every timed draw updates
      all L + 1 lags; then R alternating rounds of K steps each, the steady step loop without and with acf_accumulate after
      every step; then the accumulate alone, K launches between two synchronisations, and the bytes it moves by the algorithm:
      the ring's L + 1 slots read and one written, s read and written, sum / head, and one pass over f, mu and y.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANNED = 1_000_000                  # a long chain: the timed draws sit in half 1


def algorithmic_bytes(n, m, L, P):
    lag = 8.0 * P * ((L + 1) + 2 * (L + 1))          # the ring read, s read and written
    gather = 8.0 * P * (1 + 1 + 2 + 1)               # the value, the ring's slot, sum, head
    ll = 8.0 * 3 * n * m                             # f, mu, y
    return dict(lag=lag, gather=gather, ll_pass=ll, total=lag + gather + ll)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--max-lag", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from gpirt_amd import Sampler
    from gpirt_amd import acf as AC
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    n, m, L = args.n, args.m, args.max_lag
    y, th0 = make_responses(n, m, seed=20240)
    h = Handle(0)
    s = Sampler(h, y, th0, preset="fast", seed=1)
    s.init()
    for _ in range(args.warmup):
        s.step()
    s.check()
    s.acf_enable("all", PLANNED, L)
    for _ in range(L + 4):
        s.acf_accumulate()
    s.check()
    rates = {"off": [], "on": []}
    for _ in range(args.rounds):
        for form in rates:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                s.step()
                if form == "on":
                    s.acf_accumulate()
            s.check()
            rates[form].append(args.steps / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in rates.items()}
    walls = []
    for _ in range(3):
        s.check()
        t0 = time.perf_counter()
        for _ in range(args.launches):
            s.acf_accumulate()
        s.check()
        walls.append((time.perf_counter() - t0) / args.launches)
    P = AC.n_values(n, m, 7)
    b = algorithmic_bytes(n, m, L, P)
    acc_s = statistics.median(walls)
    rec = dict(n=n, m=m, L=L, P=P, options="gpirt_fast_options", rounds=args.rounds, steps_per_round=args.steps,
               iterations_per_s=rates, median_iterations_per_s=med, ratio_on_to_off=med["on"] / med["off"], target=0.97,
               accumulate=dict(launches=args.launches, seconds_per_accumulate=walls, median_ms=acc_s * 1e3, algorithmic_bytes=b,
                               tb_per_s=b["total"] / acc_s / 1e12),
               state_bytes=int(s.acf_state().numel() * 8))
    s.acf_enable(on=False)
    s.close()
    h.close()
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
