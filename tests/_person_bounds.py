"""Bounds for comparing the device's three lz sums of the person fit (csrc/ppc_person.hip: Wo = sum (Y - p) g, Wr = sum (rep - p) g,
Vl = sum ((p q) g) g over a respondent's observed cells) with the long-double sums of gpirt_amd.ppc.person_tables, derived from
the inputs of each case.

Per term, with eps = 2^-52 and the long-double p, q of the cell as the truth:
  e = exp(-|g|) on the device is within 1 ulp (eps e); 1 + e and the division round once each (eps / 2), and e <= 1, so
  p = 1 / (1 + e) is within 1.5 eps p and e / (1 + e) within 2.5 eps: both p and q are within 2.5 eps of themselves.
  z = 0:  t = (0 - p) g: 2.5 eps |t| from p and eps / 2 |t| from the product                      <= 3 eps |t|
  z = 1:  1 - p is off by 2.5 eps p (p's error) + eps / 2 q (its own rounding); times |g|, and the product rounds once:
          2.5 eps p |g| + eps / 2 |t| + eps / 2 |t|                                                <= eps (2.5 p |g| + 3 |t|)
  Vl:     p and q 2.5 eps each, three products eps / 2 each                                       <= 7 eps |t|
The sum: the device adds a strip's cells in order and then the strips' sums in order; a strip without an observed cell adds an
exact 0.0, so a respondent with N observed cells sees at most 2 N roundings that matter, each at most eps / 2 of a partial sum,
which is at most sum |t|:                                                                          N eps sum |t|
(twice the first-order figure for a plain sum of N terms, which covers the second-order terms as well).
    bound = N eps sum |t| + sum (per-term bound)
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def lz_bounds(y, g, rep, order):
    """(3, n) long double: the bound of |device - long double| for Wo, Wr, Vl of one draw; y, g, rep are n x m in ITEM order"""
    ld = np.longdouble
    order = np.asarray(order)
    yp = np.asarray(y, dtype=np.float64)[:, order]
    ob = ~np.isnan(yp)
    Y = ob & (yp > 0)
    bit = ob & (np.asarray(rep)[:, order] != 0)
    gl = np.where(ob, np.asarray(g, dtype=np.float64)[:, order], 0.0).astype(ld)
    el = np.exp(-np.abs(gl))
    pl = np.where(gl >= 0, 1 / (1 + el), el / (1 + el))
    ql = np.where(gl >= 0, el / (1 + el), 1 / (1 + el))
    N = ob.sum(axis=1).astype(ld)
    ag = np.abs(gl)
    out = []
    for z in (Y, bit):
        t = np.where(ob, np.abs((z.astype(ld) - pl) * gl), ld(0))
        per = EPS * (np.where(z, 2.5 * pl * ag, ld(0)) + 3 * t)
        out.append(N * EPS * t.sum(axis=1) + np.where(ob, per, ld(0)).sum(axis=1))
    t = np.where(ob, pl * ql * gl * gl, ld(0))
    out.append(N * EPS * t.sum(axis=1) + 7 * EPS * t.sum(axis=1))
    return np.stack(out)
