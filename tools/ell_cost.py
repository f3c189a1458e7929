"""What the length-scale update costs at the metric size, 8192 x 1024, with the fast options (csrc/ell.hip, gpirt_amd.ell).

  python tools/ell_cost.py --out profiles/ell_cost.json
      one sampler, one process.  The grid is 0.7 .. 2.8 in 65 points (the fast preset's rank 64 passes its certificate at 0.7),
      the chain starts at the grid point nearest 1.
      (1) iterations/s of the step loop with draw_ell() after every step, after every 10th step and not at all: --rounds
          rounds of --steps steps each, the three taken in turn, check() closing each.
      (2) one update split into its parts by the sampler's event timing (Sampler.enable_timing, ell_get("times")): the
          save / restore copies, the solve, the build and factorisation, the product, the three new kernels; the host's read is the
          call's wall time less the parts.  Medians over --updates updates after a step each, under the default prior; beside
          them the same run's stage_times() of a step (factor, draw_f) and the time of draw_f's product nu = L Z alone, which the
          update's product repeats (the handle's event pairs, class 3, over --steps steps of their own).  Then the same parts by
          outcome: the update is enabled again from index 0 under a prior table that rises by 1e6 per index, so that every upward
          proposal is accepted and every downward one rejected, and --updates updates run with no step between them -- the
          accepted path's commit copy is timed there.
      (3) the delta kernel's bytes (four n x m fp64 arrays) and TB/s.
      (4) the launch counts: factorisations enqueued by the updates against the updates that reached the device.
      (5) the acceptance rate at the default width 4 on the default grid (0.25 .. 4, 129 points; kstar_rank as
          gpirt_amd.kernel.fast_rank at 0.25 gives it) over --accept-updates updates after --burn steps, one update per step.
      (6) the centred update (Sampler.draw_ell("centred")), a section of its own ("centred") in the record: on the sampler of
          (1) to (4), after them, the parts of --updates centred updates after a step each and, in the same loop, of a whitened
          update after a step of its own, so that the two are timed side by side; the same parts by outcome under the rising prior
          table; the quad kernel against the delta kernel and logdet + decide against the whitened decide of that run; then, as
          (5), the centred update's acceptance on the default grid in a run of its own.
  python tools/ell_cost.py --out profiles/ell_cost.json --readme README.md
      also rewrites the paragraph between the two "ell_cost" marker comments of README.md from the record
  python tools/ell_cost.py --from profiles/ell_cost.json --readme README.md
      rewrites that paragraph from an earlier record; no device is touched
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


BEGIN, END = "<!-- ell_cost: written by tools/ell_cost.py -->", "<!-- /ell_cost -->"
BEGIN_C, END_C = "<!-- ell_cost_centred: written by tools/ell_cost.py -->", "<!-- /ell_cost_centred -->"


def paragraph(r) -> str:
    """the README's cost paragraph from a record"""
    import textwrap
    p, st, mi, g, d, a = (r["update_parts_ms"], r["step_stage_ms"], r["median_iterations_per_s"], r["grid"], r["default_grid"],
                          r["by_outcome"])
    acc, rej = a["accepted"], a["rejected"]
    txt = (f"Measured on one MI355X at {r['n']} x {r['m']} with the fast options, `kstar_rank` = {r['kstar_rank']} "
           f"(`tools/ell_cost.py`, `profiles/ell_cost.json`; DESIGN.md section 33; grid {g['lo']} .. {g['hi']} in {g['points']} points, "
           f"so that the rank passes its certificate at `lo`). In the chain, one update after every step, "
           f"{r['outcomes'].get('accepted', 0)} of {r['launches']['reached_the_device']} timed updates were accepted; an update is "
           f"{r['update_device_ms']:.2f} ms of device time and {r['update_wall_ms']:.2f} ms by the host's clock, the difference being "
           f"the host's read of the decision. Its parts: the save copies {p['copies']:.2f} ms, the solve {p['solve']:.2f} ms, the "
           f"build and factorisation {p['factor']:.2f} ms (the same run's `stage_times()[\"factor\"]`: {st['factor']:.2f} ms), the "
           f"product {p['product']:.2f} ms (`draw_f`'s product alone, which it repeats: {r['draw_f_product_ms']:.2f} ms; the whole "
           f"`draw_f` stage {st['draw_f']:.2f} ms), `ell_delta_kernel` {p['delta']:.3f} ms -- {r['delta_kernel']['bytes'] / 1e6:.0f} MB read, "
           f"{r['delta_kernel']['tb_per_s']:.1f} TB/s --, `ell_decide_kernel` {p['decide']:.3f} ms. By outcome, with a prior table that "
           f"makes every upward proposal accepted ({acc['count']} accepted, {rej['count']} rejected updates with no step between "
           f"them): `ell_commit_kernel` {acc['parts_ms']['commit']:.3f} ms when it copies f' to f and {rej['parts_ms']['commit']:.3f} ms "
           f"when it returns at once, the copy back of the factor buffer {rej['parts_ms']['restore']:.2f} ms on a reject; "
           f"{acc['device_ms']:.2f} ms of device time for an accepted update, {rej['device_ms']:.2f} ms for a rejected one. An update "
           f"costs about one iteration: {mi['off']:.1f} iterations/s without it, {mi['every_10th']:.1f} with an update after every "
           f"10th step, {mi['every_step']:.1f} after every step, in the same run. {r['launches']['factorisations']} factorisations for "
           f"{r['launches']['reached_the_device']} updates that reached the device. On `make_responses({r['n']}, {r['m']})` with the "
           f"documented defaults (grid {d['lo']} .. {d['hi']}, {d['points']} points, width {d['width']}) the acceptance rate is "
           f"{d['accept_rate']:.2f} over {d['updates']} updates after {r['burn']} steps. That run is NOT the fast options': at "
           f"`lo` = {d['lo']} no rank passes the certificate, so it runs `kstar_rank` = {d['kstar_rank']}; and it is a burn-in figure, "
           f"the index travelling from {d['index_first']} to {d['index_last']} (`ell` {d['length_scale_first']:.2f} to "
           f"{d['length_scale_last']:.2f}).")
    return "\n".join(textwrap.wrap(txt, 124))


def paragraph_centred(r) -> str:
    """the README's paragraph on the centred update's cost from a record's "centred" section"""
    import textwrap
    c = r["centred"]
    p, w, a, d = c["update_parts_ms"], c["whitened_parts_ms"], c["by_outcome"], c["default_grid"]
    acc, rej = a["accepted"], a["rejected"]
    txt = (f"The centred update in the same run (`tools/ell_cost.py`, section `centred` of `profiles/ell_cost.json`; the same "
           f"sampler, grid and options), one centred and one whitened update after a step each, medians of "
           f"{c['launches']['reached_the_device']} centred updates that reached the device "
           f"({c['outcomes'].get('accepted', 0)} accepted): {c['update_device_ms']:.2f} ms of device time and "
           f"{c['update_wall_ms']:.2f} ms by the host's clock, beside {c['whitened_device_ms']:.2f} ms for the whitened update "
           f"timed in that loop. Its parts: the save copies {p['copies']:.2f} ms, the first solve {p['solve']:.2f} ms, the build "
           f"and factorisation {p['factor']:.2f} ms, the second solve {p['solve_prop']:.2f} ms (the whitened update's product in "
           f"its place: {w['product']:.2f} ms), `ell_quad_kernel` {p['quad']:.3f} ms -- {c['quad_kernel']['bytes'] / 1e6:.0f} MB "
           f"read, {c['quad_kernel']['tb_per_s']:.1f} TB/s; `ell_delta_kernel` in the same loop {w['delta']:.3f} ms --, "
           f"`ell_logdet_kernel` {p['logdet']:.3f} ms and `ell_decide_centred_kernel` {p['decide']:.3f} ms (`ell_decide_kernel` "
           f"with the commit behind it: {w['decide'] + w['commit']:.3f} ms). By outcome under the rising prior table "
           f"({acc['count']} accepted, {rej['count']} rejected, no step between them): {acc['device_ms']:.2f} ms of device time "
           f"for an accepted update, {rej['device_ms']:.2f} ms for a rejected one, of which the copy back "
           f"{rej['parts_ms']['restore']:.2f} ms. {c['launches']['factorisations']} factorisations for "
           f"{c['launches']['reached_the_device']} updates that reached the device. On `make_responses({r['n']}, {r['m']})` with "
           f"the documented defaults (grid {d['lo']} .. {d['hi']}, {d['points']} points, width {d['width']}, `kstar_rank` = "
           f"{d['kstar_rank']}) the centred update's acceptance rate is {d['accept_rate']:.2f} over {d['updates']} updates after "
           f"{r['burn']} steps, one update per step, the index travelling from {d['index_first']} to {d['index_last']} (`ell` "
           f"{d['length_scale_first']:.2f} to {d['length_scale_last']:.2f}); the whitened update's figure above is from a run of "
           f"its own under the same conditions.")
    return "\n".join(textwrap.wrap(txt, 124))


def write_readme(path, r):
    src = open(path).read()
    i, j = src.index(BEGIN), src.index(END)
    src = src[:i + len(BEGIN)] + "\n" + paragraph(r) + "\n" + src[j:]
    if "centred" in r:
        i, j = src.index(BEGIN_C), src.index(END_C)
        src = src[:i + len(BEGIN_C)] + "\n" + paragraph_centred(r) + "\n" + src[j:]
    with open(path, "w") as fh:
        fh.write(src)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--readme", default=None)
    ap.add_argument("--from", dest="record", default=None)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--updates", type=int, default=40)
    ap.add_argument("--burn", type=int, default=20)
    ap.add_argument("--accept-updates", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.record:
        write_readme(args.readme, json.load(open(args.record)))
        return

    import numpy as np
    from gpirt_amd import Sampler, _lib, ell as E, kernel as K
    from gpirt_amd.ops import Handle
    from gpirt_amd.synthetic import make_responses
    n, m = args.n, args.m
    y, th0 = make_responses(n, m, seed=20240)
    lo, hi, points, width = 0.7, 2.8, 65, 4
    g = E.grid(lo, hi, points)
    k0 = int(np.argmin(np.abs(np.log(g))))
    h = Handle(0, kernel=dict(family="se", length_scale=float(g[k0])))
    s = Sampler(h, y, th0, seed=1, preset="fast")
    s.init()
    s.ell_enable(lo, hi, points, None, width, k0)
    for _ in range(args.warmup):
        s.step()
        s.draw_ell()
    s.check()
    # (1) the step loop
    rates = {"every_step": [], "every_10th": [], "off": []}
    every = {"every_step": 1, "every_10th": 10, "off": 0}
    for _ in range(args.rounds):
        for name, ev in every.items():
            t0 = time.perf_counter()
            for it in range(args.steps):
                s.step()
                if ev and (it + 1) % ev == 0:
                    s.draw_ell()
            s.check()
            rates[name].append(args.steps / (time.perf_counter() - t0))
    # (2) one update in parts, a step's stages beside them
    s.enable_timing(True)
    parts = {k: [] for k in _lib.ELL_PARTS}
    wall, stages, outcomes = [], {}, []
    before = s.ell()
    for _ in range(args.updates):
        s.step()
        for k, v in s.stage_times().items():
            stages.setdefault(k, []).append(v)
        s.check()
        t0 = time.perf_counter()
        s.draw_ell()
        wall.append((time.perf_counter() - t0) * 1e3)
        e = s.ell()
        outcomes.append(e["last"])
        if e["last"] != "out_of_range":
            for k, v in zip(_lib.ELL_PARTS, s.ell_get("times")):
                parts[k].append(float(v))
    s.enable_timing(False)
    after = s.ell()
    # draw_f's product alone: the handle's event pairs (class 3) over steps of their own
    h.prof_enable(True)
    h.prof_other(reset=True)
    for _ in range(args.steps):
        s.step()
    s.check()
    ms3, n3, _, _ = h.prof_other(reset=True)["draw_f_trmm"]
    h.prof_enable(False)
    # the parts by outcome: every upward proposal accepted, every downward one rejected
    s.ell_enable(lo, hi, points, 1e6 * np.arange(points), width, 0)
    s.check()
    s.enable_timing(True)
    by = {"accepted": dict(parts={k: [] for k in _lib.ELL_PARTS}, count=0), "rejected": dict(parts={k: [] for k in _lib.ELL_PARTS}, count=0)}
    for _ in range(args.updates):
        s.draw_ell()
        o = s.ell()["last"]
        if o in by:
            by[o]["count"] += 1
            for k, v in zip(_lib.ELL_PARTS, s.ell_get("times")):
                by[o]["parts"][k].append(float(v))
    s.enable_timing(False)
    s.check()
    by_outcome = {}
    for o, rec_o in by.items():
        pm = {k: statistics.median(v) if v else 0.0 for k, v in rec_o["parts"].items()}
        by_outcome[o] = dict(count=rec_o["count"], parts_ms=pm, device_ms=sum(pm.values()))
    reached = sum(o != "out_of_range" for o in outcomes)
    med = {k: statistics.median(v) if v else 0.0 for k, v in parts.items()}
    restore = [v for v, o in zip(parts["restore"], [o for o in outcomes if o != "out_of_range"]) if o != "accepted"]
    med["restore"] = statistics.median(restore) if restore else 0.0
    wall_reached = [w for w, o in zip(wall, outcomes) if o != "out_of_range"]
    delta_bytes = 4.0 * 8.0 * n * m
    rec = dict(n=n, m=m, grid=dict(lo=lo, hi=hi, points=points, width=width, k0=k0), kstar_rank=int(_lib.fast_options().kstar_rank), burn=args.burn,
               draw_f_product_ms=ms3 / n3 if n3 else None, by_outcome=by_outcome,
               iterations_per_s=rates, median_iterations_per_s={k: statistics.median(v) for k, v in rates.items()},
               update_parts_ms=med, update_device_ms=sum(v for k, v in med.items() if k != "restore"),
               update_wall_ms=statistics.median(wall_reached) if wall_reached else None,
               step_stage_ms={k: statistics.median(v) for k, v in stages.items()},
               delta_kernel=dict(bytes=delta_bytes, ms=med["delta"], tb_per_s=delta_bytes / (med["delta"] * 1e-3) / 1e12 if med["delta"] else None),
               launches=dict(updates=after["updates"] - before["updates"], reached_the_device=reached,
                             factorisations=after["factorisations"] - before["factorisations"]),
               outcomes={o: outcomes.count(o) for o in set(outcomes)}, accept_rate_this_grid=after["accept_rate"])
    # (6) the centred update on the same sampler: a centred and a whitened update side by side, a step before each
    s.ell_enable(lo, hi, points, None, width, k0)
    s.check()
    s.enable_timing(True)
    PC = _lib.ELL_PARTS_CENTRED
    cparts, wparts, cwall, coutcomes = {k: [] for k in PC}, {k: [] for k in _lib.ELL_PARTS}, [], []
    cbefore = s.ell()["centred"]
    for _ in range(args.updates):
        s.step()
        s.check()
        t0 = time.perf_counter()
        s.draw_ell("centred")
        cwall.append((time.perf_counter() - t0) * 1e3)
        o = s.ell()["centred"]["last"]
        coutcomes.append(o)
        if o != "out_of_range":
            for k, v in zip(PC, s.ell_get("times_centred")):
                cparts[k].append(float(v))
        s.step()
        s.check()
        s.draw_ell()
        if s.ell()["last"] != "out_of_range":
            for k, v in zip(_lib.ELL_PARTS, s.ell_get("times")):
                wparts[k].append(float(v))
    cafter = s.ell()["centred"]
    s.ell_enable(lo, hi, points, 1e6 * np.arange(points), width, 0)
    s.check()
    cby = {o: dict(parts={k: [] for k in PC}, count=0) for o in ("accepted", "rejected")}
    for _ in range(args.updates):
        s.draw_ell("centred")
        o = s.ell()["centred"]["last"]
        if o in cby:
            cby[o]["count"] += 1
            for k, v in zip(PC, s.ell_get("times_centred")):
                cby[o]["parts"][k].append(float(v))
    s.enable_timing(False)
    s.check()
    cby_outcome = {}
    for o, rec_o in cby.items():
        pm = {k: statistics.median(v) if v else 0.0 for k, v in rec_o["parts"].items()}
        cby_outcome[o] = dict(count=rec_o["count"], parts_ms=pm, device_ms=sum(pm.values()))
    creached = [o for o in coutcomes if o != "out_of_range"]
    cmed = {k: statistics.median(v) if v else 0.0 for k, v in cparts.items()}
    crestore = [v for v, o in zip(cparts["restore"], creached) if o != "accepted"]
    cmed["restore"] = statistics.median(crestore) if crestore else 0.0
    wmed = {k: statistics.median(v) if v else 0.0 for k, v in wparts.items()}
    cwall_reached = [w for w, o in zip(cwall, coutcomes) if o != "out_of_range"]
    quad_bytes = 2.0 * 8.0 * n * m
    rec["centred"] = dict(
        update_parts_ms=cmed, update_device_ms=sum(v for k, v in cmed.items() if k != "restore"),
        update_wall_ms=statistics.median(cwall_reached) if cwall_reached else None,
        whitened_parts_ms=wmed, whitened_device_ms=sum(v for k, v in wmed.items() if k != "restore"), by_outcome=cby_outcome,
        quad_kernel=dict(bytes=quad_bytes, ms=cmed["quad"], tb_per_s=quad_bytes / (cmed["quad"] * 1e-3) / 1e12 if cmed["quad"] else None),
        conditions=dict(quad_not_slower_than_delta=bool(cmed["quad"] <= wmed["delta"]), quad_ms=cmed["quad"], delta_ms=wmed["delta"],
                        logdet_plus_decide_ms=cmed["logdet"] + cmed["decide"], whitened_decide_ms=wmed["decide"]),
        launches=dict(updates=cafter["updates"] - cbefore["updates"], reached_the_device=len(creached),
                      factorisations=cafter["factorisations"] - cbefore["factorisations"]),
        outcomes={o: coutcomes.count(o) for o in set(coutcomes)})
    s.close()
    h.close()
    # (5) the documented defaults
    rank = K.fast_rank(dict(family="se", length_scale=0.25))
    gd = E.grid()
    kd = int(np.argmin(np.abs(np.log(gd))))
    h = Handle(0, kernel=dict(family="se", length_scale=float(gd[kd])))
    s = Sampler(h, y, th0, seed=1, rng="item", theta_stabilise=True, fstar_fused=True, kstar_rank=rank)
    s.init()
    s.ell_enable()
    idx = []
    for it in range(args.burn + args.accept_updates):
        s.step()
        if it == args.burn:
            start = s.ell()
        s.draw_ell()
        idx.append(s.ell()["index"])
    s.check()
    e = s.ell()
    done = e["updates"] - start["updates"]
    rec["default_grid"] = dict(lo=0.25, hi=4.0, points=129, width=4, kstar_rank=rank, updates=done,
                               accept_rate=(e["accepted"] - start["accepted"]) / done,
                               out_of_range=e["out_of_range"], failed=e["failed"], index_first=idx[0], index_last=idx[-1],
                               index_min=min(idx), index_max=max(idx), length_scale_first=float(gd[idx[0]]),
                               length_scale_last=e["length_scale"])
    s.close()
    h.close()
    # (6) the centred update's acceptance under the same conditions, in a run of its own
    h = Handle(0, kernel=dict(family="se", length_scale=float(gd[kd])))
    s = Sampler(h, y, th0, seed=1, rng="item", theta_stabilise=True, fstar_fused=True, kstar_rank=rank)
    s.init()
    s.ell_enable()
    idx = []
    for it in range(args.burn + args.accept_updates):
        s.step()
        if it == args.burn:
            start = s.ell()["centred"]
        s.draw_ell("centred")
        idx.append(s.ell()["index"])
    s.check()
    e = s.ell()
    done = e["centred"]["updates"] - start["updates"]
    rec["centred"]["default_grid"] = dict(lo=0.25, hi=4.0, points=129, width=4, kstar_rank=rank, updates=done,
                                          accept_rate=(e["centred"]["accepted"] - start["accepted"]) / done,
                                          out_of_range=e["centred"]["out_of_range"], failed=e["centred"]["failed"],
                                          index_first=idx[0], index_last=idx[-1], index_min=min(idx), index_max=max(idx),
                                          length_scale_first=float(gd[idx[0]]), length_scale_last=e["length_scale"])
    s.close()
    h.close()
    txt = json.dumps(rec, indent=1, default=float)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
    if args.readme:
        write_readme(args.readme, json.loads(txt))


if __name__ == "__main__":
    main()
