"""The CPU oracle's stages under R's stream, on the device's state (test infrastructure only).

Under R's single Mersenne-Twister stream every draw depends on everything consumed before it, so the stages cannot be cut
into independent slices the way oracle/parallel.py cuts them under the item RNG.  What can be shared out: everything a stage
computes that does not touch the generator (draw_fstar's s and mean, src/draw-fstar.cpp:17-25), and draw_theta's loop,
which takes exactly one uniform per respondent in order (src/draw-theta.cpp:27): a block of respondents starts at a copy of
the generator advanced by the respondents in front of it.
"""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle as O
from oracle import parallel as P

_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def rstream_at(state):
    """An oracle RStream holding the generator state (mt, mti) of gpirt_amd.ops.RStream.state()."""
    mt, mti = state
    r = O.RStream(0)
    for q in range(624):
        r.s.mt[q] = int(mt[q])
    r.s.mti = int(mti)
    return r


def same_position(r, state):
    mt, mti = r.mt_state()
    return int(state[1]) == mti and np.array_equal(np.asarray(state[0], dtype=np.uint32), mt)


def draw_fstar(r, it, f, theta, L, mu_star, nthreads=None):
    """src/draw-fstar.cpp:10-31 under R's stream: s and the mean (with mu_star) on all cores, then the noise in the
    reference's order -- items outer, grid points inner (:23-29), one R::rnorm(mean, s_i) each (s_i == 0 consumes nothing).
    Returns (fstar, s, mean)."""
    _, s, mean = P.draw_fstar(0, it, f, theta, L, mu_star, nthreads)
    lib = O.lib()
    N, m = mean.shape
    out = np.empty((N, m), order="F")
    for j in range(m):
        for i in range(N):
            out[i, j] = lib.orc_rnorm(r.ref, mean[i, j], s[i])
    return out, s, mean


def draw_theta(r, it, y, fstar, stabilise=True, nthreads=None, block=256):
    """src/draw-theta.cpp:3-37 under R's stream, blocks of respondents side by side: each block starts at a copy of the
    generator walked forward by the blocks in front of it (one uniform per respondent, :27).  Leaves r after the last
    respondent.  Returns (theta, degenerate count)."""
    lib = O.lib()
    lib.orc_draw_theta_block.restype = C.c_int
    ts = O.theta_star()
    N = len(ts)
    prior = np.array([lib.orc_dnorm_log(t, 0.0, 1.0) for t in ts])
    fs = np.asfortranarray(np.array(fstar, dtype=np.float64))
    n, m = y.shape
    out = np.empty(n)
    jobs = []
    for a in range(0, n, block):
        b = min(a + block, n)
        jobs.append((a, b, O.Rng.from_buffer_copy(r.s)))
        for _ in range(b - a):
            lib.orc_unif_rand(r.ref)

    def job(a, b, g):
        yb = np.asfortranarray(np.array(y[a:b, :], dtype=np.float64))
        ob = np.empty(b - a)
        d = lib.orc_draw_theta_block(C.byref(g), C.c_uint32(it), _p(ts), _p(yb), _p(prior), _p(fs), C.c_int64(b - a),
                                     C.c_int64(m), C.c_int64(N), C.c_int(int(stabilise)), C.c_int64(a), _p(ob))
        out[a:b] = ob
        return d

    with ThreadPoolExecutor(nthreads or P.host_cores()) as pool:
        deg = list(pool.map(lambda t: job(*t), jobs))
    return out, int(sum(deg))
