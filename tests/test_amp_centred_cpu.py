"""The centred amplitude update without a GPU (include/gpirt_hip.h "a centred amplitude update"; gpirt_amd.amp.centred_*): the
rank-64 basis at the default kernel, the NumPy statement against a direct dense computation of the augmentation's conditional,
prior invariance of the construction on the GPU test's configuration, the seed of the constructed cases, and the new C symbols."""
import ctypes as C

import numpy as np
import pytest

import _amp_centred_bounds as CB

LD = np.longdouble


def test_version_stage_and_symbols():
    from gpirt_amd import _lib
    lib = _lib.load()
    assert lib.gpirt_version() >= 135 and _lib.ST_AMP_CENTRED == 13
    for name in ("gpirt_sampler_draw_amp_centred", "gpirt_sampler_amp_centred_stats"):
        assert hasattr(lib, name), name
    a = _lib.AmpCentred()
    assert C.sizeof(a) == 8 * (6 + 2 + 6)                     # gpirt_amp_centred: six counters, two doubles, six reserved words
    # every existing stage keeps its number
    assert (_lib.ST_AMP, _lib.ST_CARRY, _lib.ST_POP, _lib.ST_ELL) == (10, 11, 12, 9)


def test_basis_at_the_default_kernel():
    """r = 32 and max |Phi Phi^T - K| <= 1e-12 over 500 grid thetas (measured: 4e-15)"""
    from gpirt_amd import amp as A
    theta = np.round(np.linspace(-5, 5, 500), 2)
    Phi, live, r = A.centred_basis(theta)
    assert r == 32 and live.sum() == 32 and Phi.shape == (500, 64) and Phi.dtype == LD
    assert not Phi[:, ~live].any()
    K = np.exp(LD(-0.5) * (theta.astype(LD)[:, None] - theta.astype(LD)[None, :]) ** 2)
    err = float(np.abs(Phi @ Phi.T - K).max())
    cond = np.linalg.cond((Phi.T @ Phi + LD(1e-3) * np.eye(64)).astype(np.float64))
    print(f"MEASURED basis: r = {r}, max |Phi Phi^T - K| = {err:.2e}, cond(A) = {cond:.2e}")
    assert err <= 1e-12


def _solve_ld(A, B):
    """A^-1 B by Gaussian elimination with partial pivoting in long double"""
    A = np.array(A, dtype=LD)
    B = np.array(B, dtype=LD)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]], B[[k, p]] = A[[p, k]], B[[p, k]]
        w = A[k + 1:, k] / A[k, k]
        A[k + 1:] -= w[:, None] * A[k][None, :]
        B[k + 1:] -= w[:, None] * B[k][None, :]
    for k in range(n - 1, -1, -1):
        B[k] = (B[k] - A[k, k + 1:] @ B[k + 1:]) / A[k, k]
    return B


def test_statement_against_the_dense_conditional():
    """40 x 3: xi | f, a is N(A^-1 Phi^T f, a^2 eps A^-1).  The statement's mean (z = 0) and its noise map (z = unit vectors)
    against the n x n forms Phi^T (Phi Phi^T + eps I)^-1 f and a^2 (I - Phi^T (Phi Phi^T + eps I)^-1 Phi), which share no code
    with it (elimination with pivoting in long double, no Cholesky factor of A).  cond(A) = 1e5 and long double carries 2^-64: 1e-12
    relative is three orders above what the two routes can differ by."""
    from gpirt_amd import amp as A
    c = CB.case(40, 3)
    eps = LD(1e-3)
    a = c["grid"][c["k"]]
    zero = np.zeros((64, 3))
    ref = A.centred_exact_coef(c["theta"], c["f"], a, 1, 1, z=zero)
    Phi, live, r = A.centred_basis(c["theta"])
    S = Phi @ Phi.T + eps * np.eye(40, dtype=LD)
    mean = Phi.T @ _solve_ld(S, c["f"].astype(LD))
    scale = float(np.abs(mean).max())
    assert float(np.abs(ref["xi"][live] - mean[live]).max()) <= 1e-12 * scale
    assert float(np.abs(ref["H"] - Phi @ mean).max()) <= 1e-12 * float(np.abs(c["f"]).max())
    assert float(np.abs(ref["Q"] - (mean[live] ** 2).sum(axis=0)).max()) <= 1e-12 * float(ref["Q"].max())
    cov = (LD(a[0]) ** 2) * (np.eye(64, dtype=LD) - Phi.T @ _solve_ld(S, Phi))
    lv = np.flatnonzero(live)
    cols = []
    for k in lv:                                                  # xi(z = e_k) - xi(z = 0) = a sqrt(eps) R^-T e_k
        z = zero.copy()
        z[k, 0] = 1.0
        cols.append(A.centred_exact_coef(c["theta"], c["f"], a, 1, 1, z=z)["xi"][:, 0] - ref["xi"][:, 0])
    M = np.array(cols).T[lv]                                      # r x r
    err = float(np.abs(M @ M.T - cov[np.ix_(lv, lv)]).max())
    print(f"MEASURED dense: mean within {float(np.abs(ref['xi'][live] - mean[live]).max()) / scale:.1e} relative, covariance {err:.1e}")
    assert err <= 1e-12 * float(np.abs(cov).max())
    # the move holds the nugget's whitened coordinates: f' - h = c (f - h), and a = a' reproduces f
    up = A.centred_exact_update(np.asarray(ref["H"], dtype=np.float64), np.asarray(ref["Q"], dtype=np.float64), c["f"], c["mu"],
                                c["y"], c["k"], 1, 1, c["grid"], c["log_prior"], r)
    H64 = np.asarray(ref["H"], dtype=np.float64)
    for j, st in enumerate(up["status"]):
        if st == "accepted":
            assert np.array_equal(up["f"][:, j], H64[:, j] + up["c"][j] * (c["f"][:, j] - H64[:, j]))
        else:
            assert up["f"][:, j].tobytes() == c["f"][:, j].tobytes()


def test_normals_and_uniforms_keying():
    """index 0 .. 63 the normals, 64 / 65 the uniforms, all of stage 13: no pair is shared, and the normals are AS 241 of their
    uniforms"""
    from gpirt_amd import amp as A
    from gpirt_amd.ppc import item_uniform
    z = A.centred_normals(7, 3, np.arange(4))
    u0, u1 = A.centred_uniforms(7, 3, np.arange(4))
    raw = item_uniform(7, 3, 13, np.arange(4, dtype=np.uint64)[None, :], np.arange(66, dtype=np.uint64)[:, None])
    assert z.shape == (64, 4) and np.array_equal(u0, raw[64]) and np.array_equal(u1, raw[65])
    assert len(np.unique(raw)) == raw.size
    assert np.array_equal(np.sign(z), np.sign(raw[:64] - 0.5)) and abs(z.mean()) < 0.3 and 0.7 < z.std() < 1.3
    assert np.array_equal(A.centred_uniforms(7, 3, 2), (raw[64, 2], raw[65, 2]))


def test_prior_invariance_of_the_construction():
    """The GPU chain's configuration in NumPy (tests/_amp_centred_bounds.py): every cell within 5 binomial sds; the two wrong
    variants the issue names fail by a wide margin, so the test has power."""
    kept, edges, mass = CB.pi_chain_numpy()
    z = CB.pi_zscores(kept, edges, mass)
    print(f"MEASURED prior invariance (NumPy): z = {np.round(z, 2).tolist()}")
    assert kept.shape == ((CB.PI_ROUNDS - CB.PI_BURN) // CB.PI_THIN, CB.PI_M) and abs(mass.sum() - 1) < 1e-12
    assert np.abs(z).max() <= CB.PI_SDS
    for kw in (dict(exponent_shift=-1), dict(noise=False)):
        zz = CB.pi_zscores(*CB.pi_chain_numpy(**kw))
        assert np.abs(zz).max() > 4 * CB.PI_SDS, kw


@pytest.mark.parametrize("m", CB.MS)
@pytest.mark.parametrize("n", CB.NS)
def test_the_constructed_cases_are_decided(n, m):
    """With tests/_amp_centred_bounds.py's seed the statement alone leaves at most 2 % of the items of every constructed case
    undecided (for m <= 5: none), and the cases together meet accepted updates and rewritten columns."""
    from gpirt_amd import amp as A
    c = CB.case(n, m)
    a = c["grid"][c["k"]]
    ref = A.centred_exact_coef(c["theta"], c["f"], a, CB.SEED, 1)
    up = A.centred_exact_update(np.asarray(ref["H"], dtype=np.float64), np.asarray(ref["Q"], dtype=np.float64), c["f"], c["mu"],
                                c["y"], c["k"], CB.SEED, 1, c["grid"], c["log_prior"], ref["r"])
    assert (~up["decided"]).sum() <= 0.02 * m
    b = CB.coef_bounds(ref, c["f"], a)
    # not vacuous: what a wrong kernel moves by order one is held to a few thousandths
    assert b["rho"] < 1e-4 and float((b["H"] / (np.abs(np.asarray(ref["H"], dtype=np.float64)) + 1)).max()) < 2e-2
    print(f"MEASURED n={n} m={m}: statuses {up['status']}, rho {b['rho']:.1e}, cond {ref['cond']:.1e}")
