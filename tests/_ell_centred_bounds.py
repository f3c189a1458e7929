"""Derived bounds and the shared cases of the centred length-scale update's tests (tests/test_ell_centred_cpu.py,
tests/test_gpu_ell_centred.py).  A(S), kF, u = 2^-53 and e_nu_j are those of tests/_ell_bounds.py, whose `case`,
`factor_constants`, `tv_bound` and `index_ess` are used as they are.

DEVICE AGAINST gpirt_amd.ell.step_exact_centred, ONE UPDATE FROM THE SAME f.  Both sides factor S_k and S_k' in fp64 (the device's
blocked factorisation, NumPy's LAPACK call), ||L^-1 dL||_F <= A(S) per factor and 2 A(S) between the two (_ell_bounds.py);
everything after the factors is fp64 on the device and long double in the reference.
nu = L^-1 f, nu' = L'^-1 f:   ||d nu_j||_2 <= (2 A(S_k) + n u kF_k) ||nu_j||_2 =: e_nu_j,  ||d nu'_j||_2 <= (2 A(S_k') + n u kF_k')
                   ||nu'_j||_2 =: e_nu'_j (the factors' difference and a substitution's backward error, as in _ell_bounds.py).  When f
                   itself differs between the two sides by ||d f_j||_2 <= e_f_j (a mixed trajectory: the whitened updates before
                   have moved it), both gain ||L^-1||_2 e_f_j = e_f_j / sqrt(lmin(S)).
dq_j = sum_i (nu'_ij - nu_ij)(nu'_ij + nu_ij) = ||nu'_j||^2 - ||nu_j||^2:  its derivative in nu_j is -2 nu_j, in nu'_j 2 nu'_j, so
                   |d dq_j| <= 2 ||nu_j|| e_nu_j + 2 ||nu'_j|| e_nu'_j + e_nu_j^2 + e_nu'_j^2     (Cauchy-Schwarz; the squares: exact, not
                   first order)
                   plus the rounding: a cell is one subtraction, one addition and one product, 3 u |cell|; the additions of a
                   column in ell_delta_kernel's order, at most n / 256 + 1 per thread and 8 levels of the tree, (n / 256 + 9) u
                   sum_i |cell|:   r_dq_j = (n / 256 + 12) u sum_i |nu'_ij^2 - nu_ij^2|
                   e_dq_j = the sensitivity above + r_dq_j;   dq = sum_j dq_j in ascending j: e_dq = sum_j e_dq_j + m u sum_j |dq_j|
dld = sum_i (log L'_ii - log L_ii):  d log L_ii = dL_ii / L_ii to first order, which is the i-th diagonal entry of L^-1 dL up to the
                   strictly-lower part of L^-1 (L^-1 dL is lower triangular with diagonal dL_ii / L_ii).  So the factors' difference
                   moves sum_i log L_ii by |tr(L^-1 dL)| <= sqrt(n) ||L^-1 dL||_F <= sqrt(n) 2 A(S), and
                   |d dld| <= sqrt(n) (2 A(S_k) + 2 A(S_k')) + r_dld
                   r_dld: per logarithm the 1 ulp that the HIP math API documents for the fp64 log (ROCm documentation, HIP
                   math API reference, "Double precision mathematical functions", row log: maximum error 1 ULP), 1 ulp(v) <=
                   2 u |v|; the subtraction u |term|; the additions (n / 256 + 9) u sum_i |term_i|:
                   r_dld = sum_i 2 u (|log L'_ii| + |log L_ii|) + (n / 256 + 10) u sum_i |log L'_ii - log L_ii|
log_ratio = (-0.5 dq - m dld) + (lp' - lp):  -0.5 dq is exact; m dld, the subtraction, lp' - lp on the host and the addition round
                   once each, together at most 3 u (|0.5 dq| + |m dld| + |lp' - lp|):
                   e_ratio = 0.5 e_dq + m e_dld + 3 u (|0.5 dq| + |m dld| + |lp' - lp|)
max-abs figures are held under these 2-norm bounds (||x||_inf <= ||x||_2).

A TRAJECTORY of centred updates with no step() in between: f never moves, so every update is a first update from the same f and
carries the one-update bound of its own (k, k'), no drift.  A MIXED trajectory (whitened, centred, whitened, ...): the whitened
updates move f, and the two sides' f differ by at most the e_fp of _ell_bounds.trajectory_ratio_bound for the number of updates
made, either kind counted (each solves once with the current factor); a centred update then carries the bound above with that
e_f.  That the factors' difference does not accumulate through the solves is _ell_bounds.py's assumption for its trajectory, taken
over here for the mixed one; the measured figures are printed beside the bounds.

STAGE BY STAGE, GIVEN THE DEVICE'S OWN FACTORS L (under ell_k) and L' (under ell_k'; a fresh sampler's factor is bit for bit the
proposal's), each stage's reference in long double from the device's output of the stage before:
    nu against L^-1 f, nu' against L'^-1 f:   ||d nu_j||_2 <= n u kF ||nu_j||_2, kF of that factor    (the substitution's backward error)
    dq_j against the cells of (nu_dev, nu'_dev):   r_dq_j alone
    dld against sum_i (log L'_ii - log L_ii) of the device's diagonals:   r_dld alone
    dq against sum_j dq_dev_j:   m u sum_j |dq_j|;    log_ratio against (-0.5 dq_dev - m dld_dev) + (lp' - lp):   the 3 u term alone

THE CHAIN AGAINST conditional_posterior_centred: with f fixed the update is a Metropolis chain on P states; _ell_bounds.tv_bound
of the chain's own ESS (_ell_bounds.index_ess) applies word for word.

log_ratio AGAINST THE DENSITY (test_ell_centred_cpu.py).  log N(f_j; 0, S) = -0.5 f_j^T S^-1 f_j - 0.5 log det S + const, computed from
S itself in fp64 by numpy.linalg.solve and slogdet (LU with partial pivoting, backward stable: a relative error c n u cond(S) in
x = S^-1 f and an absolute error c n u cond(S) in log det S is what a backward error c n u ||S|| allows, d log det = tr(S^-1 dS) <= n
||S^-1|| ||dS||).  The reference side goes through the fp64 Cholesky factor, whose backward error A(S)-type bound is of the same
form.  With c = 4 for both sides together:
    |log_ratio - density difference| <= 4 n u [cond(S_k) + cond(S_k')] (0.5 sum_j (|q_j| + |q'_j|) + m), q_j = f_j^T S^-1 f_j.
"""
import numpy as np

from _ell_bounds import LD, U, case, factor_constants, index_ess, tv_bound          # noqa: F401  (shared with the test files)
import _ell_bounds as EB

SEED = 7                      # the trajectories' seed: chosen so that no update is a near-tie (test_ell_centred_cpu.py asserts it)
P, W, N, M = 65, 4, 40, 3     # the chain case of the issue: grid 0.25 .. 4 in 65 points, width 4
UPDATES, GPU_UPDATES, MIXED = 4000, 2000, 500


def chain_case():
    return case(N, M, P, SEED)


def chain(c, width, updates, seed=None):
    """The NumPy chain of centred updates from a case (f fixed).  Returns the per-update records (status, k, k_prop, margin =
    |log_ratio - log u1| or None, the norms of nu and nu' per item) and the factor cache."""
    from gpirt_amd import ell as E
    seed = c["seed"] if seed is None else seed
    k, cache, rec = c["k"], {}, []
    for t in range(1, updates + 1):
        u0, u1 = E.uniforms(seed, t, "centred")
        r = E.step_exact_centred(c["theta"], c["f"], k, u0, u1, c["grid"], c["log_prior"], width, c["family"], cache)
        rec.append(_record(r, k, "centred"))
        k = r["k"]
    return dict(records=rec, k=k, cache=cache)


def _record(r, k_before, kind):
    out = dict(kind=kind, status=r["status"], k_before=int(k_before), k=r["k"], k_prop=r["k_prop"], margin=None)
    if "log_ratio" in r:
        out["margin"] = abs(float(r["log_ratio"] - r["log_u"]))
        out["nn"] = np.sqrt((np.asarray(r["nu"], dtype=np.float64) ** 2).sum(axis=0))
        if kind == "centred":
            out["nnp"] = np.sqrt((np.asarray(r["nu_prop"], dtype=np.float64) ** 2).sum(axis=0))
            out["ref"] = {q: r[q] for q in ("dq", "dld")}
            out["abs_cells"] = np.abs(np.asarray((r["nu_prop"] - r["nu"]) * (r["nu_prop"] + r["nu"]), dtype=np.float64)).sum(axis=0)
    return out


def mixed_chain(c, width, pairs, seed=None):
    """The NumPy chain of `pairs` whitened updates each followed by a centred one, no step() in between: each kind with its own call
    count and uniforms.  Returns the records in order (2 x pairs), the final f and index and the cache."""
    from gpirt_amd import ell as E
    seed = c["seed"] if seed is None else seed
    k, f, cache, rec = c["k"], c["f"], {}, []
    for t in range(1, pairs + 1):
        r = E.step_exact(c["theta"], f, c["mu"], c["y"], k, *E.uniforms(seed, t), c["grid"], c["log_prior"], width, c["family"], cache)
        rec.append(_record(r, k, "whitened"))
        k, f = r["k"], r["f"]
        r = E.step_exact_centred(c["theta"], f, k, *E.uniforms(seed, t, "centred"), c["grid"], c["log_prior"], width, c["family"], cache)
        rec.append(_record(r, k, "centred"))
        k = r["k"]
    return dict(records=rec, f=f, k=k, cache=cache)


_CONSTANTS = {}


def constants(c, k):
    """factor_constants of case c at grid index k plus 1 / sqrt(lmin) (= kF / ||L||_F), kept per (case, k)"""
    key = (c["n"], c["m"], c["points"], c["seed"], c["family"], c["lo"], c["hi"], int(k))
    if key not in _CONSTANTS:
        a = dict(factor_constants(c["theta"], c["family"], c["grid"][k]))
        a["inv2"] = a["kF"] / a["LF"]
        _CONSTANTS[key] = a
    return _CONSTANTS[key]


def update_bounds(c, k, kp, nn, nnp, abs_cells, dq, dld, diag=None, e_f=None):
    """The end-to-end bounds of the module docstring for the centred update k -> kp of case c, from the reference's own figures:
    nn, nnp = ||nu_j||, ||nu'_j|| (m each), abs_cells = sum_i |cell| per item, dq (m), dld; diag = (diag L, diag L') of the reference
    (None: r_dld's logarithm terms are bounded with |log L_ii| <= log(1 / sqrt(0.001)) = 3.46, the jitter's floor, and |log L_ii| <=
    0.5 log(1.001) above); e_f: ||d f_j||_2 per item when f differs between the two sides."""
    n, m = c["n"], c["m"]
    a, b = constants(c, k), constants(c, kp)
    e_nu = (2 * a["A"] + n * U * a["kF"]) * nn
    e_nup = (2 * b["A"] + n * U * b["kF"]) * nnp
    if e_f is not None:
        e_nu = e_nu + a["inv2"] * e_f
        e_nup = e_nup + b["inv2"] * e_f
    r_dq = (n / 256 + 12) * U * abs_cells
    e_dqj = 2 * nn * e_nu + 2 * nnp * e_nup + e_nu ** 2 + e_nup ** 2 + r_dq
    dq = np.asarray(dq, dtype=np.float64)
    e_dq = float(e_dqj.sum() + m * U * np.abs(dq).sum())
    if diag is None:
        logs, terms = 2 * n * 3.46, 2 * n * 3.46
    else:
        lo, ln = np.log(np.asarray(diag[0], dtype=np.float64)), np.log(np.asarray(diag[1], dtype=np.float64))
        logs, terms = float((np.abs(lo) + np.abs(ln)).sum()), float(np.abs(ln - lo).sum())
    r_dld = 2 * U * logs + (n / 256 + 10) * U * terms
    e_dld = float(np.sqrt(n) * (2 * a["A"] + 2 * b["A"]) + r_dld)
    lpd = abs(float(c["log_prior"][kp] - c["log_prior"][k]))
    sizes = 0.5 * abs(float(dq.sum())) + m * abs(float(dld)) + lpd
    return dict(nu=e_nu, nu_prop=e_nup, dq=e_dqj, dq_sum=e_dq, dld=e_dld, log_ratio=0.5 * e_dq + m * e_dld + 3 * U * sizes)


def record_bound(c, r, e_f=None):
    """the log_ratio bound of one centred record of `chain` / `mixed_chain`"""
    return update_bounds(c, r["k_before"], r["k_prop"], r["nn"], r["nnp"], r["abs_cells"], r["ref"]["dq"], r["ref"]["dld"],
                         e_f=e_f)["log_ratio"]


def mixed_bounds(c, records):
    """(the whitened updates' log_ratio bound, e_f per item, the centred records' bounds) of a mixed trajectory: _ell_bounds's
    trajectory bound for len(records) updates with the largest ||nu_j|| any update of the trajectory met"""
    env = np.max([r["nn"] for r in records if r["margin"] is not None], axis=0)
    e_ratio, e_f = EB.trajectory_ratio_bound(c, env[None, :], len(records))
    return e_ratio, e_f, [record_bound(c, r, e_f) if r["kind"] == "centred" and r["margin"] is not None else None for r in records]


def stage_bounds(c, L, Lp, dev, k, kp):
    """The stage-by-stage layer: L, Lp the device's factors (n x n fp64) under ell_k and ell_kp, dev the device's nu, nu_prop, dq
    and record_centred.  Returns name -> (error, bound)."""
    from gpirt_amd import ell as E
    n, m = c["n"], c["m"]
    out = {}
    nu, nup, dq, rec = (np.asarray(dev[q]) for q in ("nu", "nu_prop", "dq", "record_centred"))
    for name, F, x in (("nu", L, nu), ("nu_prop", Lp, nup)):
        T = np.tril(F)
        sv = np.linalg.svd(T, compute_uv=False)
        kF = float(np.sqrt((T ** 2).sum()) / sv[-1])
        ref = E.solve_lower(T.astype(LD), c["f"])
        e = np.sqrt(((x.astype(LD) - ref).astype(np.float64) ** 2).sum(axis=0))
        out[name] = (e, n * U * kF * np.sqrt((x ** 2).sum(axis=0)))
    cells = (nup.astype(LD) - nu.astype(LD)) * (nup.astype(LD) + nu.astype(LD))
    out["dq"] = (np.abs(dq.astype(LD) - cells.sum(axis=0)).astype(np.float64),
                 (n / 256 + 12) * U * np.abs(cells.astype(np.float64)).sum(axis=0))
    lo, ln = np.log(np.diagonal(L).astype(LD)), np.log(np.diagonal(Lp).astype(LD))
    r_dld = 2 * U * float((np.abs(lo) + np.abs(ln)).sum()) + (n / 256 + 10) * U * float(np.abs(ln - lo).sum())
    out["dld"] = (abs(float(LD(rec[1]) - (ln - lo).sum())), r_dld)
    out["dq_sum"] = (abs(float(LD(rec[0]) - dq.astype(LD).sum())), m * U * float(np.abs(dq).sum()))
    lpd = LD(c["log_prior"][kp]) - LD(c["log_prior"][k])
    want = (LD(-0.5) * LD(rec[0]) - LD(m) * LD(rec[1])) + lpd
    out["log_ratio"] = (abs(float(LD(rec[2]) - want)), 3 * U * (0.5 * abs(float(rec[0])) + m * abs(float(rec[1])) + abs(float(lpd))))
    return out
