"""Item-column sharding of the sampler over torch.distributed (one process per GPU, RCCL over xGMI).

Given L and theta the m item columns of draw_f / draw_fstar / draw_beta are conditionally
independent (src/draw-f.cpp:69-71, src/draw-fstar.cpp:23-29, src/draw-beta.cpp:16-38), so rank r
owns columns [m*r/G, m*(r+1)/G).  What is not item-separable:
  * draw_theta sums the log-likelihood over ALL items per respondent (src/draw-theta.cpp:15-19).
    `theta="gather"` (default): the ranks all-gather their f* columns (N* x m, 8 MB at the metric size), every
    rank forms the log-posterior of ITS BLOCK OF RESPONDENTS over all items in one MFMA GEMM (the same sums in
    the same order as on one GPU) and draws theta for that block; the n draws are then combined (64 KB).
    `theta="allreduce"`: every rank computes the partial sum over its items for all respondents and the
    N* x n partial log-posteriors (66 MB) are all-reduced; every rank then draws the same theta.
    Either way the RNG is keyed by the global respondent index.
  * K + chol (src/gpirtMCMC.cpp:76-78): `chol="replicated"` factors on every rank (no traffic);
    `chol="bcast"` factors on rank 0 and broadcasts L (one RCCL broadcast per iteration);
    `chol="distributed"`: 1-D block-cyclic ownership of the 1024-column outer panels, pipelined by
    halves of a panel -- the owner factors the first sub-panel and broadcasts it while it factors the second; the next
    owner applies the first half's share of the update of its own first columns meanwhile, and every rank applies each
    finished panel to the block columns it owns.  Every rank ends with the full L: the panel broadcasts ARE the
    broadcast of L.  Same launches, same order as the single-GPU factorisation => bit-identical L.
The per-item RNG sub-streams are keyed by the GLOBAL item index, so the draws do not depend on G up to rounding: the
GEMM tiling / split-K partition of nu = L z and of the f* products depends on the local column count, so f and f* agree
to ~1e-12 between partitions, and theta -- a grid pick -- is identical unless one of those last bits flips a comparison
(probability ~1e-11 per draw).

`engine_factory(y_local, theta_init, pm, ps, step, item0, m_total)` must return an object with the
stage methods of gpirt_amd.Sampler; tests substitute a CPU engine to exercise this host logic
under gloo.
"""
from __future__ import annotations

import numpy as np

from . import _lib


def item_range(m: int, rank: int, world: int):
    """Contiguous block partition of the item columns."""
    lo = (m * rank) // world
    hi = (m * (rank + 1)) // world
    return lo, hi


class ShardedSampler:
    def __init__(self, engine_factory, y, theta_init, pm=None, ps=None, step=None, *, dist=None,
                 chol="replicated", theta="gather"):
        self.dist = dist
        self.rank = dist.get_rank() if dist is not None else 0
        self.world = dist.get_world_size() if dist is not None else 1
        y = np.asfortranarray(np.asarray(y, dtype=np.float64))
        self.n, self.m_total = y.shape
        self.lo, self.hi = item_range(self.m_total, self.rank, self.world)
        m = self.m_total
        pm = np.zeros((2, m)) if pm is None else np.asarray(pm, dtype=np.float64)
        ps = np.full((2, m), 3.0) if ps is None else np.asarray(ps, dtype=np.float64)
        step = np.full((2, m), 0.1) if step is None else np.asarray(step, dtype=np.float64)
        sl = slice(self.lo, self.hi)
        self.engine = engine_factory(y[:, sl], np.asarray(theta_init, dtype=np.float64), pm[:, sl], ps[:, sl],
                                     step[:, sl], self.lo, m)
        # The sharded path is checked against the CPU oracle (tests/test_distributed_cpu.py), which knows the reference's
        # kernel alone: an engine on a handle with another kernel (Handle.set_kernel) is refused, not run unchecked.
        eh = getattr(self.engine, "handle", None)
        if eh is not None and hasattr(eh, "kernel"):
            from . import kernel as K
            if not K.is_default(eh.kernel()):
                used = eh.kernel()
                self.engine.close()
                raise ValueError(f"ShardedSampler runs the default kernel only (squared exponential, length_scale 1); the "
                                 f"engine's handle is set to {used}")
        self.chol = chol
        if chol not in ("replicated", "bcast", "distributed"):
            raise ValueError("chol must be 'replicated', 'bcast' or 'distributed'")
        self._panel_bufs = None
        import os as _os
        self._debug = _os.environ.get("GPIRT_DIST_DEBUG") == "1"
        if theta not in ("gather", "allreduce"):
            raise ValueError("theta must be 'gather' or 'allreduce'")
        self.theta_mode = theta if self.world > 1 else "local"
        self._views = {}
        if self.theta_mode == "gather":
            self.i0, self.i1 = item_range(self.n, self.rank, self.world)     # this rank's block of respondents
            self.engine.set_theta_block(y[self.i0:self.i1, :], self.i0, m)
            # The gather path is chosen ONCE, from facts every rank agrees on (backend, m % world): a rank that
            # switched paths on its own (e.g. after a failed collective) would leave its peers in a different
            # collective.  Equal shards on a backend with the flat all-gather (RCCL, gloo) use it; anything else
            # all-reduces disjoint supports.
            self._flat_gather = (m % self.world == 0) and hasattr(dist, "all_gather_into_tensor")

    def _view(self, name):
        """torch view of an engine buffer, created once (the buffers live as long as the engine)"""
        v = self._views.get(name)
        if v is None:
            v = self._views[name] = self.engine.device_tensor(name)
        return v

    # -- collectives on the engine's buffers ------------------------------------------------
    def _allreduce_logpost(self):
        if self.world > 1:
            self.dist.all_reduce(self._view("logpost"))

    def _gather_fstar(self):
        """every rank's f* columns -> the full N* x m array on every rank (column-major: shards are contiguous)"""
        full, loc = self._view("fstar_full"), self._view("fstar")
        if self._flat_gather:
            self.dist.all_gather_into_tensor(full, loc)
            return
        N = full.numel() // self.m_total
        full.zero_()
        full[N * self.lo: N * self.hi].copy_(loc[: N * (self.hi - self.lo)])
        self.dist.all_reduce(full)                  # disjoint supports: the sum is the concatenation, exactly

    def _combine_theta(self):
        self.dist.all_reduce(self._view("theta_stage"))   # zero outside each rank's block

    def _factor_distributed(self):
        """Right-looking over outer panels, pipelined by HALVES of a panel.  Panel p is owned by rank
        p % world and factored as a first sub-panel A(p) (512 columns) and the rest B(p).  A(p) is broadcast while its
        owner factors B(p); the next owner applies A(p)'s half of the update of ITS first columns while B(p) is still
        being factored and travelling (the single-GPU factorisation splits that update the same way, potrf.hip
        crit_update), so behind B(p)'s arrival only K = 512 of update and the next first sub-panel are left on the chain.
        Every block column receives the panels' products in the same order as on one GPU: L is bit-identical.
        Collectives are issued in one fixed order on every rank: A(0), B(0), A(1), B(1), ..."""
        import torch
        e, W, n = self.engine, self.engine.panel_width, self.n
        H = e.subpanel_width
        NP = (n + W - 1) // W
        rows = e.panel_rows                         # n, plus the rows of a bordered factorisation
        owner = lambda p: p % self.world
        mine = lambda p: owner(p) == self.rank
        def cols(p, half):
            P0, P1 = p * W, min((p + 1) * W, n)
            mid = min(P0 + H, P1)
            return (P0, mid) if half == 0 else (mid, P1)

        if self._panel_bufs is None:
            # two broadcast buffers: one half travels while the previous one is still being unpacked / applied.  Sized for
            # the LARGEST part that will travel: half 1 ("the rest") is W - H columns wide -- wider than half 0 whenever
            # the sub-panel is narrower than half an outer panel (GPIRT_NBP < GPIRT_NBO / 2; round-3 advisor finding: the
            # buffers held rows * H doubles and a torch slice past the end truncates silently)
            need = max((rows - k0) * (k1 - k0) for p in range(NP) for k0, k1 in (cols(p, 0), cols(p, 1)))
            self._panel_bufs = [torch.empty(need, dtype=torch.float64, device=e.torch_device) for _ in range(2)]
        seq = [0]

        def send(p, half):      # collective: every rank calls it, in the same order
            k0, k1 = cols(p, half)
            if k1 <= k0:
                return None
            buf = self._panel_bufs[seq[0] % 2][: (rows - k0) * (k1 - k0)]
            if buf.numel() != (rows - k0) * (k1 - k0):
                raise RuntimeError("panel broadcast buffer too small for part (%d, %d)" % (p, half))
            seq[0] += 1
            if mine(p):
                e.panel_copy_part(p, half, buf, True)
            self._check_joined()
            return buf, self.dist.broadcast(buf, src=owner(p), async_op=True)

        def receive(p, half, h):
            if h is None:
                return
            buf, w = h
            w.wait()
            if not mine(p):
                e.panel_copy_part(p, half, buf, False)

        e.build_cov()
        if mine(0):
            e.panel_factor_part(0, 0)
        hA = send(0, 0)
        if mine(0):
            e.panel_factor_part(0, 1)               # beside A(0)'s broadcast
        receive(0, 0, hA)
        for p in range(NP):
            nxt = p + 1
            hB = send(p, 1)                          # B(p): behind its factorisation on the owner's stream
            if nxt < NP and mine(nxt):
                e.panel_update_part(p, nxt, 0)       # needs A(p) only: runs while B(p) is factored and travels
            receive(p, 1, hB)
            if nxt >= NP:
                break
            if mine(nxt):
                e.panel_update_part(p, nxt, 1)       # what is left on the chain: K = 512 on the first columns + the others
                e.panel_factor_part(nxt, 0)
            hA = send(nxt, 0)
            if mine(nxt):
                e.panel_factor_part(nxt, 1)          # beside A(p + 1)'s broadcast
            for c in range(nxt + 1, NP):             # panel p on the rest of this rank's block columns
                if mine(c):
                    e.panel_update_part(p, c, 2)
            receive(nxt, 0, hA)
        e.adopt_factor(True)                        # the panel copies carry the rows below the factor too (panel_rows)

    def _check_joined(self):
        """GPIRT_DIST_DEBUG=1: every piece must have joined the engine's stream before a collective is enqueued behind it
        (the library forks look-ahead work onto streams of its own; RCCL orders itself behind torch's current stream only)."""
        if self._debug and hasattr(self.engine, "streams_busy"):
            busy = self.engine.streams_busy()
            if busy:
                raise RuntimeError(f"a factorisation piece returned with internal streams still busy (mask {busy})")

    def _factor(self):
        if self.chol == "distributed" and self.world > 1:
            self._factor_distributed()
        elif self.chol in ("replicated", "distributed") or self.world == 1:
            self.engine.factor()
        else:
            if self.rank == 0:
                self.engine.factor()
                if hasattr(self.engine, "dense_factor"):
                    self.engine.dense_factor()      # (the "L" view is a kept pointer: a structured factor is made dense before it travels)
            else:
                self.engine.adopt_factor(True)      # the "L" view is the WHOLE ldl x n buffer: the bordered rows travel too
            self.dist.broadcast(self._view("L"), src=0)

    def init(self):
        self.engine.init()

    STAGES = ("draw_f", "draw_fstar", "theta_gemm", "theta_allreduce", "theta_sample", "draw_beta", "factor")

    def step(self, timer=None):
        """One MCMC iteration.  `timer(name)` (optional) is called after each stage is enqueued --
        bench.py passes a function that records a device event, to attribute time to stages."""
        e = self.engine
        t = timer if timer is not None else (lambda name: None)
        e.draw_f(); t("draw_f")
        e.draw_fstar(); t("draw_fstar")
        if self.theta_mode == "gather":
            self._gather_fstar(); t("theta_allreduce")
            e.theta_block(); t("theta_gemm")
            self._combine_theta(); e.theta_commit(); t("theta_sample")
        else:
            e.theta_partial(); t("theta_gemm")
            self._allreduce_logpost(); t("theta_allreduce")
            e.theta_finish(); t("theta_sample")
        e.draw_beta(); t("draw_beta")
        self._factor(); t("factor")

    def gather(self, name: str):
        """All ranks receive the full (column-concatenated) array `name` of item-sharded state.  Tensor collectives on
        the host copies (no pickling: `f` is 64 MiB per rank at the metric size): shards are padded to the largest
        item count so that one flat all-gather serves unequal partitions too."""
        return self._gather_columns(self.engine.get(name))

    # -- posterior summaries (include/gpirt_hip.h gpirt_sampler_summary_*): each rank accumulates its own item columns;
    # theta's moments are the same on every rank.  The quantile parts ("theta_hist", "irf_band", gpirt_amd.quantiles) are
    # not offered here: each rank's f* band would cover its own items only and would have to be gathered.
    def summary_enable(self, parts):
        bits = _lib.summary_parts(parts)
        if bits & (_lib.SUM_THETA_HIST | _lib.SUM_IRF_BAND):
            raise ValueError("ShardedSampler: the quantile parts (theta_hist, irf_band) are not offered for item shards")
        self.engine.summary_enable(parts)

    def summary_accumulate(self):
        self.engine.summary_accumulate()

    # -- posterior predictive checks (gpirt_amd.ppc): not offered for item shards -- a respondent's statistics run over ALL
    # items and would need one all-reduce per draw.  The replicate's uniforms are keyed by the global item index
    # (item0 + j), so a later sharded form replicates exactly what one GPU does.
    def ppc_enable(self, on=True):
        raise ValueError("ShardedSampler: posterior predictive checks are not offered for item shards "
                         "(the respondents' statistics would need an all-reduce per draw)")

    def ppc_pairs_enable(self, top=20, on=True):
        raise ValueError("ShardedSampler: the pairwise item checks are not offered for item shards "
                         "(a pair's table runs over two shards' replicates)")

    def ppc_bins_enable(self, cuts=None, top=20, on=True):
        raise ValueError("ShardedSampler: the theta-binned item fit is not offered for item shards "
                         "(it is an add-on to the posterior predictive checks, which are not offered either)")

    def ppc_dif_enable(self, groups=None, cuts=None, top=20, on=True):
        raise ValueError("ShardedSampler: the group-wise item fit is not offered for item shards "
                         "(it is an add-on to the posterior predictive checks, which are not offered either)")

    def ppc_scores_enable(self, cuts=None, groups=9, top=20, on=True):
        raise ValueError("ShardedSampler: the score-based checks are not offered for item shards "
                         "(a respondent's score runs over all items, and each rank holds its own columns)")

    def ppc_person_enable(self, order=None, cuts=None, groups=5, top=20, on=True):
        raise ValueError("ShardedSampler: the person fit is not offered for item shards "
                         "(a respondent's pattern runs over all items, and each rank holds its own columns)")

    def ppc_resid_enable(self, top=20, on=True):
        raise ValueError("ShardedSampler: the residual correlations are not offered for item shards "
                         "(a pair's items may lie on two ranks, and each rank holds its own columns)")

    # -- rank posteriors (gpirt_amd.ranks): theta is replicated on every rank, so each rank's engine holds the same ranks
    def rank_enable(self, on=True, pivots="median", pairwise=False):
        self.engine.rank_enable(on, pivots, pairwise)

    def rank_accumulate(self):
        self.engine.rank_accumulate()

    def ranks(self, probs=(0.025, 0.5, 0.975)):
        return self.engine.ranks(probs)

    # -- shape posteriors of the item response curves (gpirt_amd.shape): the test information runs over ALL items
    def shape_enable(self, window=3.0, tols=(0.0, 0.25, 1.0), on=True):
        raise ValueError("ShardedSampler: the shape posteriors are not offered for item shards (the test information and "
                         "the reliability of a draw run over all items, and each rank holds its own columns)")

    # -- sum-score posteriors (gpirt_amd.sumscore): the recursion of a draw runs over ALL items of the form
    def sumscore_enable(self, items=None, on=True):
        raise ValueError("ShardedSampler: the sum-score posteriors are not offered for item shards (the recursion runs over "
                         "all items of the form, and each rank holds its own f* columns)")

    # -- two-form score equating (gpirt_amd.equate): both forms' recursions run over items that live on different ranks
    def equate_enable(self, x=None, y=None, on=True):
        raise ValueError("ShardedSampler: the score equating is not offered for item shards (each form's recursion runs over "
                         "all of its items, and each rank holds its own f* columns)")

    # -- PSIS-LOO (gpirt_amd.loo): the cells are local to an item shard, but the totals, the respondent sums and the worst cells
    # run over all items and are not pooled across ranks here
    def loo_enable(self, planned_draws=None, tail=None, on=True):
        raise ValueError("ShardedSampler: PSIS-LOO is not offered for item shards (the totals, the respondent sums and the "
                         "worst cells run over all items; each rank holds its own columns)")

    def shape_order_enable(self, on=True):
        raise ValueError("ShardedSampler: the item-pair order posteriors are not offered for item shards (a pair's two curves "
                         "may live on two ranks, and the shape posteriors they sit on are not offered either)")

    # -- autocorrelation ESS (gpirt_amd.acf): beta's and the items' series are local to a shard, but the respondents' and the
    # total log-likelihood run over all items and are not pooled across ranks here
    def acf_enable(self, parts="all", planned_draws=None, max_lag=None, on=True):
        raise ValueError("ShardedSampler: the autocorrelation ESS is not offered for item shards (the respondents' and the "
                         "total log-likelihood series run over all items; each rank holds its own columns)")

    # -- group posteriors (gpirt_amd.groups): the vote part (sides, contested items, loyalty) runs over ALL items
    def groups_enable(self, groups=None, top=20, on=True):
        raise ValueError("ShardedSampler: the group posteriors are not offered for item shards (the vote part -- the contested "
                         "items and every respondent's loyalty -- runs over all items; each rank holds its own columns)")

    # -- the length scale in the chain (gpirt_amd.ell): the likelihood change of an update runs over ALL items and the factor is
    # the ranks' common one
    def ell_enable(self, lo=0.25, hi=4.0, points=129, log_prior=None, width=4, k0=None, on=True):
        raise ValueError("ShardedSampler: the length-scale update is not offered for item shards (its likelihood change runs "
                         "over all items, and each rank holds its own columns of f)")

    def draw_ell(self, kind="whitened"):
        raise ValueError("ShardedSampler: the length-scale update is not offered for item shards (its likelihood change runs "
                         "over all items, and each rank holds its own columns of f)")

    # -- per-item GP amplitudes (gpirt_amd.amp): the library keeps them for all items of one sampler
    def amp_set(self, a):
        raise ValueError("ShardedSampler: per-item amplitudes are not offered for item shards (the library keeps them for all "
                         "items of one sampler)")

    def amp_enable(self, lo=0.1, hi=10.0, points=129, log_prior=None, width=4, k0=None, planned_draws=0, on=True):
        raise ValueError("ShardedSampler: per-item amplitudes are not offered for item shards (the library keeps them for all "
                         "items of one sampler)")

    def draw_amp(self):
        raise ValueError("ShardedSampler: per-item amplitudes are not offered for item shards (the library keeps them for all "
                         "items of one sampler)")

    def draw_amp_centred(self):
        raise ValueError("ShardedSampler: per-item amplitudes are not offered for item shards (the library keeps them for all "
                         "items of one sampler)")

    def draw_beta_centred(self):
        raise ValueError("ShardedSampler: the centred beta update is not offered for item shards (the library refuses an item "
                         "shard: its shared 2 x 2 matrix is built for all items of one sampler)")

    def scale_enable(self, w_scale=None, w_shift=None):
        raise ValueError("ShardedSampler: the collapsed scale and shift move is not offered for item shards (the library refuses an "
                         "item shard: logpost then holds only part of the items)")

    def draw_scale(self, kind):
        self.scale_enable()

    # -- the population prior for theta (gpirt_amd.pop): the respondent-block theta path would need the codes of its block
    def pop_set(self, codes, log_prior=None):
        raise ValueError("ShardedSampler: a population prior is not offered for item shards (the respondent-block theta path "
                         "would need the codes of its respondents)")

    def pop_enable(self, codes=None, groups=None, **kw):
        raise ValueError("ShardedSampler: a population prior is not offered for item shards (the respondent-block theta path "
                         "would need the codes of its respondents)")

    def draw_pop(self):
        raise ValueError("ShardedSampler: a population prior is not offered for item shards (the respondent-block theta path "
                         "would need the codes of its respondents)")

    # -- scoring new respondents (gpirt_amd.score): the product of a new respondent runs over ALL items
    def score_enable(self, y_new):
        raise ValueError("ShardedSampler: scoring new respondents is not offered for item shards (a new respondent's "
                         "product runs over all items, and each rank holds its own f* columns)")

    def score_predict_enable(self, top=5, on=True):
        raise ValueError("ShardedSampler: predicting new respondents' answers is not offered for item shards (it is an "
                         "add-on to scoring, whose product runs over all items)")

    def summary_gather(self, name: str):
        """The full pointwise summary `name` (p_yes, lppd, p_waic, f_mean, f_var, beta_mean, beta_var) on every rank;
        theta_mean / theta_var are the local ones (identical on every rank)."""
        local = self.engine.summary_get(name)
        if name.startswith("theta_"):
            return local
        return self._gather_columns(local)

    def summary_totals(self) -> dict:
        """WAIC totals of the whole problem: sums of lppd, p_waic and n_obs over the ranks; the elpd spread combined by
        Chan's formula from each rank's (n_obs, mean, sum of squared deviations); one all-gather of three numbers a rank."""
        t = self.engine.summary_totals()
        if self.world == 1:
            return t
        import torch
        dev = getattr(self.engine, "torch_device", torch.device("cpu"))
        if self.dist.get_backend() == "gloo":
            dev = torch.device("cpu")
        keys = ("lppd", "p_waic", "n_obs", "elpd_mean", "elpd_ss")
        mine = torch.tensor([[t[k] for k in keys]], dtype=torch.float64, device=dev)
        full = torch.empty((self.world, len(keys)), dtype=torch.float64, device=dev)
        if hasattr(self.dist, "all_gather_into_tensor"):
            self.dist.all_gather_into_tensor(full, mine)
        else:
            parts = [torch.empty_like(mine) for _ in range(self.world)]
            self.dist.all_gather(parts, mine)
            full = torch.cat(parts, dim=0)
        rows = full.cpu().numpy()
        lppd = float(sum(r[0] for r in rows))                 # rank order: the same sums on every rank
        p_waic = float(sum(r[1] for r in rows))
        n, mean, ss = 0.0, 0.0, 0.0
        for r in rows:                                        # Chan et al.: pairwise combination of (count, mean, M2)
            nb, mb, sb = float(r[2]), float(r[3]), float(r[4])
            if nb == 0:
                continue
            tot = n + nb
            delta = mb - mean
            mean = mean + delta * (nb / tot)
            ss = ss + sb + delta * delta * (n * nb / tot)
            n = tot
        elpd = lppd - p_waic
        return dict(lppd=lppd, p_waic=p_waic, elpd_waic=elpd, waic=-2.0 * elpd,
                    se_elpd_waic=float(np.sqrt(n * (ss / (n - 1.0)))) if n > 1 else float("nan"),
                    n_obs=n, draws=t["draws"], elpd_mean=mean, elpd_ss=ss)

    def _gather_columns(self, arr):
        local = np.ascontiguousarray(arr.T)                       # (m_local, rows)
        if self.world == 1:
            return np.asfortranarray(local.T)
        import torch
        rows = local.shape[1]
        counts = [item_range(self.m_total, r, self.world) for r in range(self.world)]
        mmax = max(hi - lo for lo, hi in counts)
        dev = getattr(self.engine, "torch_device", torch.device("cpu"))
        if self.dist.get_backend() == "gloo":
            dev = torch.device("cpu")
        mine = torch.zeros((mmax, rows), dtype=torch.float64, device=dev)
        mine[: local.shape[0]] = torch.from_numpy(local).to(dev)
        full = torch.empty((self.world * mmax, rows), dtype=torch.float64, device=dev)
        if hasattr(self.dist, "all_gather_into_tensor"):
            self.dist.all_gather_into_tensor(full, mine)
        else:
            parts = [torch.empty_like(mine) for _ in range(self.world)]
            self.dist.all_gather(parts, mine)
            full = torch.cat(parts, dim=0)
        full = full.cpu().numpy()
        out = np.concatenate([full[r * mmax: r * mmax + (hi - lo)] for r, (lo, hi) in enumerate(counts)], axis=0)
        return np.asfortranarray(out.T)
