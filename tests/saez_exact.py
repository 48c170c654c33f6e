"""The Saez-formula period start in real arithmetic, with the band every faithful float64 evaluation must land in.

Not a conftest: a plain helper of tests/test_saez_numerics.py, in the manner of tests/covid_exact.py.  It follows the
reference's own recipe and operation order (F/components/redistribution.py -- compute_and_set_new_period_rates_from_
saez_formula :437-513, estimate_uniform_income_elasticity :552-601, get_binned_saez_welfare_weight_and_pareto_params
:603-753, get_saez_marginal_rates :755-791, bracketize_schedule :793-823), not the kernel's.

Every quantity is carried as a pair (x, e):

- x is the recipe's value in real arithmetic (mpmath at PREC bits; the inputs, the constants and the bin edges are the
  float64 numbers the reference holds, taken exactly);
- e bounds |v - x| for ANY faithful float64 evaluation v of the recipe up to that point, u = 2**-53:
    * a +, -, * or / passes its operands' bounds through the operation (first order terms and the second order
      ones: nothing is dropped) and adds u * |result|;
    * a log does the same and adds K_LOG ulps of its result (ulp(r) <= 2u|r|);
    * a sum of k terms adds gamma(k) * sum|terms|, gamma(k) = ku / (1 - ku), whatever the order of the additions
      (the reference adds pairwise, the C restatement serially, the kernel per lane and then across lanes; a fused
      multiply-add rounds once where the bound counts twice);
    * max, min and clip are 1-Lipschitz: the larger operand bound, nothing added;
    * a divisor whose band reaches 0 gives e = inf (the generator of the test inputs keeps away from those).
- Discrete decisions are taken on exact data: the histogram (np.histogram's [e_i, e_i+1) bins, the last one closed),
  `z > 0 and tau < 1`, `pz[i] == 0` (a count), `len(zs) < 10`, `np.std(taus) < 1e-6` (rational arithmetic; the
  inputs stay a factor 2 away from the threshold so that a float evaluation takes the same side).

The 2x2 normal equations: the reference calls np.linalg.inv (LAPACK gesv: LU with partial pivoting, then two
triangular solves per column of the identity); the kernel and the C restatement use the closed-form inverse
(determinant).  Both are evaluations of the same real-arithmetic recipe, so `err` is the larger of the two bounds,
each derived operation by operation as above (a division in the LU path counted as reciprocal-then-multiply, which
optimised triangular solves use).  One thing is done by hand there: the computed determinant (the computed Schur
complement u22) divides every entry of the inverse, so it is taken out of XXi.T.dot(XY) as the one number it is
instead of being given a separate error in each term (_ols_closed, _ols_lu: an exact rewriting of the same floats).
Both lose about u * (mean / sd)**2 of log(1 - tau) to the cancellation in the determinant and as much again in the
numerator: the band widens by itself where the rates cluster and stays at a few u elsewhere.

Nothing here is fitted: no constant comes from the kernel, the restatement or a measurement.  Underflow is not
modelled (no intermediate of the recipe comes near it on the test inputs).
"""
import math
from fractions import Fraction

import mpmath
import numpy as np
from mpmath import mpf

PREC = 200
K_LOG = 1  # ulps allowed on a log result, as in covid_exact.py
U = 2.0 ** -53
_UP = 1.0 + 2.0 ** -40  # the bounds themselves are computed in float64: every step rounds them up by more than it can lose
INF = math.inf
BRANCHES = ("count", "std", "ols", "ols_clipped")


class V(object):
    """(x, e): real value (mpf) and the bound on what a faithful float64 evaluation can be away from it (float)."""
    __slots__ = ("x", "e")

    def __init__(self, x, e=0.0):
        self.x = x if isinstance(x, mpf) else mpf(float(x))
        self.e = e


def _ab(x):
    return abs(float(x)) * _UP + 5e-324


def _rnd(x, e):
    """the operation's own rounding on top of the propagated bound e: the computed result is within e of x before it"""
    if e == INF:
        return V(x, INF)
    return V(x, (e + U * (_ab(x) + e)) * _UP)


ZERO, ONE, HALF = V(0), V(1), V(0.5)


def add(a, b):
    return _rnd(a.x + b.x, a.e + b.e)


def sub(a, b):
    return _rnd(a.x - b.x, a.e + b.e)


def mul(a, b):
    if a.e == 0.0 and b.e == 0.0:
        return _rnd(a.x * b.x, 0.0)
    if a.e == INF or b.e == INF:
        return V(a.x * b.x, INF)
    return _rnd(a.x * b.x, (_ab(a.x) * b.e + _ab(b.x) * a.e + a.e * b.e) * _UP)


def div(a, b):
    x = a.x / b.x
    if a.e == 0.0 and b.e == 0.0:
        return _rnd(x, 0.0)
    if a.e == INF or b.e == INF:
        return V(x, INF)
    lo = abs(float(b.x)) / _UP - b.e  # the divisor's band must keep off 0
    if not lo > 0:
        return V(x, INF)
    return _rnd(x, (_ab(a.x) * b.e + _ab(b.x) * a.e) / (abs(float(b.x)) / _UP * lo) * _UP)


def vmax(a, b):
    return V(a.x if a.x >= b.x else b.x, max(a.e, b.e))


def vmin(a, b):
    return V(a.x if a.x <= b.x else b.x, max(a.e, b.e))


def clip(a, lo, hi):
    """np.clip with exact bounds"""
    x = a.x
    if x < lo:
        x = mpf(lo)
    if x > hi:
        x = mpf(hi)
    return V(x, a.e)


def log(a):
    x = mpmath.log(a.x)
    if a.e == 0.0:
        prop = 0.0
    else:
        lo = a.x - mpf(a.e)
        if not lo > 0:
            return V(x, INF)
        prop = _ab(x - mpmath.log(lo))  # the steeper side
    return V(x, (prop + K_LOG * 2 * U * (_ab(x) + prop)) * _UP)


def vsum(terms):
    """a sum of k terms in any order"""
    terms = [t for t in terms if not (t.e == 0.0 and t.x == 0)]  # adding an exact 0 changes nothing in any order
    k = len(terms)
    if k == 0:
        return V(0)
    x = mpmath.fsum(t.x for t in terms)
    if k == 1:
        return V(x, terms[0].e)
    e = sum(t.e for t in terms)
    mag = sum(_ab(t.x) + t.e for t in terms)
    g = k * U / (1 - k * U)
    return V(x, (e + g * mag) * _UP * _UP)


def _rdiv(a, b):
    """a / b evaluated as a * (1 / b): two roundings (a plain division fits inside)"""
    return mul(a, div(ONE, b))


def _rr(v):
    """one more rounding on v (a factor (1 + eps) moved onto it from elsewhere in a product)"""
    return _rnd(v.x, v.e)


def _recip_of_the_float(v):
    """1 / v-as-computed, in real arithmetic: no rounding of its own"""
    lo = abs(float(v.x)) / _UP - v.e
    if v.e == INF or not lo > 0:
        return V(1 / v.x, INF)
    return V(1 / v.x, v.e / (abs(float(v.x)) / _UP * lo) * _UP)


def _ols_closed(a, b, d, sxy, sy):
    """[[a, b], [b, d]]**-1 through the determinant, then XXi.T.dot(XY): the kernel's and the restatement's evaluation.
    i00 = d / det, i01 = -b / det, i11 = a / det share the one computed det, so
    elas = i00 * sxy + i01 * sy = ((d * sxy)(1 + e1)(1 + e2) - (b * sy)(1 + e3)(1 + e4))(1 + e5) / det-as-computed:
    the quotient's and the product's roundings sit on each term, the sum's on the numerator."""
    det = sub(mul(a, d), mul(b, b))
    elas = div(sub(_rr(mul(d, sxy)), _rr(mul(b, sy))), det)
    log_z0 = div(sub(_rr(mul(a, sy)), _rr(mul(b, sxy))), det)
    return elas, log_z0


def _ols_lu(a, b, d, sxy, sy, swap):
    """np.linalg.inv is gesv on the identity: LU with partial pivoting (l, u22), then per column P e_j a forward and a
    back substitution, x2 = w2 / u22, x1 = (y1 - r1[1] * x2) / r1[0]; then XXi.T.dot(XY).  Every entry of the inverse
    carries the factor rho = 1 / u22-as-computed: entry = rho * c, with c evaluated below (a division counted as
    reciprocal-then-multiply: two roundings), so each output is rho * (c * sxy + c' * sy)."""
    r1, r2 = ((b, d), (a, b)) if swap else ((a, b), (b, d))  # swap: the pivot is b, |b| > |a|
    l = _rdiv(r2[0], r1[0])
    u22 = sub(r2[1], mul(l, r1[1]))
    rho = _recip_of_the_float(u22)

    def solve(y1, y2):
        c2 = _rr(_rr(sub(y2, mul(l, y1))))
        c1 = _rdiv(sub(u22 if y1 is ONE else ZERO, mul(r1[1], c2)), r1[0])  # (y1 / rho - r1[1] * c2) / r1[0]
        return c1, c2

    c0 = solve(ZERO, ONE) if swap else solve(ONE, ZERO)  # column 0 of the inverse: (i00, i10) / rho
    c1 = solve(ONE, ZERO) if swap else solve(ZERO, ONE)  # column 1: (i01, i11) / rho
    elas = mul(rho, add(mul(c0[0], sxy), mul(c0[1], sy)))
    log_z0 = mul(rho, add(mul(c1[0], sxy), mul(c1[1], sy)))
    return elas, log_z0


def _fl(v):
    """(nom, err): x rounded once to float64, and the bound measured from that float"""
    nom = float(v.x)
    if v.e == INF:
        return nom, INF
    return nom, (v.e + _ab(v.x - mpf(nom))) * _UP


_LOG_CACHE = {}


def _log_cached(key, make):
    r = _LOG_CACHE.get(key)
    if r is None:
        r = _LOG_CACHE[key] = log(make())
    return r


def exact_std(taus):
    """np.std of float64 values in rational arithmetic, as a float (correct to a few ulps: only its side of 1e-6
    and its distance from it matter)"""
    fr = [Fraction(float(t)) for t in taus]
    mean = sum(fr) / len(fr)
    var = sum((t - mean) ** 2 for t in fr) / len(fr)
    with mpmath.workprec(PREC):
        return float(mpmath.sqrt(mpf(var.numerator) / mpf(var.denominator))), var < Fraction(1e-6) ** 2


def effective_buffer(local, additions, glob):
    """the `saez_buffer` property :514-525: [len, 2] float64"""
    local = np.asarray(local, np.float64).reshape(-1, 2)
    if glob is None or len(glob) == 0:
        return local
    glob = np.asarray(glob, np.float64).reshape(-1, 2)
    if additions == 0:
        return glob
    return np.concatenate([glob, local[-additions:]])  # a Python slice: more additions than samples takes them all


def period_start(samples, elas_state, running_avg, cfg):
    """One period start of the formula on a buffer that has reached its minimum size.

    samples: [len, 2] float64 (income, marginal rate); elas_state: (elas_t, elas_tm1, log_z0_t, log_z0_tm1) before the
    call; running_avg: [NB]; cfg: bracket_cutoffs [NB], rate_min, rate_max (the current, annealed limit), pareto_uniform
    (bool), fixed_elas (None or float), bin_edges (np.linspace(0, top, 101) itself).

    Returns {"nom": {...}, "err": {...}, "branch": one of BRANCHES, "n_empty": bins without incomes, "std": exact
    np.std of the usable rates (None when fewer than 10), "usable": their count}; outputs elas_t, elas_tm1, log_z0_t,
    log_z0_tm1 (scalars), next_rates [NB], running_avg [NB]."""
    with mpmath.workprec(PREC):
        return _period_start(np.asarray(samples, np.float64).reshape(-1, 2), [float(v) for v in elas_state],
                             np.asarray(running_avg, np.float64), cfg)


def _period_start(samples, elas_state, running_avg, cfg):
    z_all, tau_all = samples[:, 0], samples[:, 1]
    edges = np.asarray(cfg["bin_edges"], np.float64)
    T = len(edges) - 1
    cut = [float(c) for c in cfg["bracket_cutoffs"]]
    NB = len(cut)
    E9 = V(1e-9)

    # ---- :464-480 and estimate_uniform_income_elasticity ----
    elas_tm1, log_z0_tm1 = V(elas_state[0]), V(elas_state[2])
    use = (z_all > 0) & (tau_all < 1)
    zs, taus = z_all[use], tau_all[use]
    m = int(use.sum())
    std = None
    if m < 10:
        branch, elas_t, log_z0_t = "count", elas_tm1, log_z0_tm1
    else:
        std, below = exact_std(taus)
        if below:
            branch, elas_t, log_z0_t = "std", elas_tm1, log_z0_tm1
        else:
            xs = [_log_cached(("1-", float(t)), lambda t=t: vmax(sub(ONE, V(float(t))), E9)) for t in taus]
            ys = [_log_cached(("z", float(z)), lambda z=z: vmax(V(float(z)), E9)) for z in zs]
            a = vsum([mul(x, x) for x in xs])
            b = vsum(xs)
            d = V(m)
            sxy = vsum([mul(x, y) for x, y in zip(xs, ys)])
            sy = vsum(ys)
            det = a.x * d.x - b.x * b.x
            elas_x = (d.x * sxy.x - b.x * sy.x) / det
            logz_x = (a.x * sy.x - b.x * sxy.x) / det
            e_el = e_lz = 0.0
            gap = abs(float(abs(b.x) - abs(a.x)))  # the pivot is chosen on computed sums: both ways if they could tie
            pivots = [True, False] if gap <= (a.e + b.e) * _UP else [bool(abs(b.x) > abs(a.x))]
            for ols in [_ols_closed] + [lambda *w, s=s: _ols_lu(*w, swap=s) for s in pivots]:
                el, lz = ols(a, b, d, sxy, sy)
                assert abs(el.x - elas_x) <= abs(elas_x) * 1e-30 + 1e-40 and abs(lz.x - logz_x) <= abs(logz_x) * 1e-30 + 1e-40
                e_el, e_lz = max(e_el, el.e), max(e_lz, lz.e)
            elas, log_z0_t = V(elas_x, e_el), V(logz_x, e_lz)
            branch = "ols_clipped" if elas_x < 0 else "ols"
            elas_t = add(mul(sub(ONE, V(0.98)), vmax(elas, ZERO)), mul(V(0.98), elas_tm1))
    out = {"elas_t": elas_t, "elas_tm1": elas_tm1, "log_z0_t": log_z0_t, "log_z0_tm1": log_z0_tm1}
    elas_used = V(float(cfg["fixed_elas"])) if cfg.get("fixed_elas") is not None else elas_t

    # ---- np.histogram(incomes, bins=edges) ----
    below = z_all < edges[0]
    above = z_all > edges[T]
    mid = z_all[~below & ~above]
    idx = np.minimum(np.searchsorted(edges, mid, side="right") - 1, T - 1)  # the last bin is closed on the right
    counts = np.bincount(idx, minlength=T)[:T]
    n_below, n_above, n_total = int(below.sum()), int(above.sum()), len(z_all)
    assert int(counts.sum()) + n_below + n_above == n_total

    def pareto(v):  # :636-643
        return ONE if cfg["pareto_uniform"] else div(ONE, vmax(ONE, v))

    bin_z = [mul(HALF, add(V(edges[i]), V(edges[i + 1]))) for i in range(T)]
    width = [sub(V(edges[i + 1]), V(edges[i])) for i in range(T)]
    # compute_binned_g_distribution: pareto(max(z, 0)) is exactly 1 for every income below the first edge (0)
    w_below = V(n_below)
    z_above = [V(float(v)) for v in z_all[above]]
    w_above = vsum([pareto(v) for v in z_above]) if n_above else ZERO
    per_bin = [mul(V(int(counts[i])), pareto(bin_z[i])) if counts[i] else ZERO for i in range(T)]
    norm = add(add(add(vsum(per_bin), w_below), w_above), E9)
    dens = [div(p, norm) if p is not ZERO else ZERO for p in per_bin] + [div(w_above, norm)]
    ntot = V(n_total)
    pz = [div(V(int(c)), ntot) if c else ZERO for c in counts] + [div(V(n_above), ntot)]
    g = [None] * (T + 1)
    for i in range(T + 1):  # np.cumsum(...[::-1])[::-1]: the sum of the entries from i up
        g[i] = div(vsum(dens[i:]), add(vsum(pz[i:]), E9))
    gz = [mul(HALF, add(g[i], g[i + 1])) for i in range(T)] + [g[T]]
    # compute_binned_a_distribution
    p_below = div(V(n_below), ntot)
    az = [None] * (T + 1)
    cum = None
    for i in range(T):
        cum = add(pz[0], p_below) if i == 0 else clip(add(cum, pz[i]), 0, 1)
        if counts[i]:
            p_geq = add(sub(ONE, cum), mul(HALF, pz[i]))
            paz = div(mul(bin_z[i], pz[i]), add(clip(p_geq, 0, 1), E9))
            az[i] = div(paz, width[i])
    if n_above:
        mean_above = div(vsum(z_above), V(n_above))
        az[T] = div(mean_above, add(sub(mean_above, V(edges[T])), E9))
    else:
        az[T] = ZERO
    # ---- get_saez_marginal_rates ----
    taus_b = [None] * (T + 1)
    for i in range(T + 1):
        if az[i] is not None:
            omg = sub(ONE, gz[i])
            taus_b[i] = div(omg, add(add(omg, mul(az[i], elas_used)), E9))
    last_rate, last_idx = ZERO, -1
    for i in range(T + 1):
        if taus_b[i] is None:
            continue
        if i - last_idx > 1:  # np.linspace(last, tau, gap + 2)[1:-1]: arange * step + start
            gap = i - last_idx - 1
            step = div(sub(taus_b[i], last_rate), V(gap + 1))
            for j in range(1, gap + 1):
                taus_b[last_idx + j] = add(mul(V(j), step), last_rate)
        last_rate, last_idx = taus_b[i], i
    # ---- bracketize_schedule, np.clip, the running average ----
    rates = []
    last_total = ZERO
    for bi in range(NB - 1):
        income = V(cut[bi + 1])
        bin_taxes = []
        for i in range(T + 1):
            past = vmax(ZERO, sub(income, V(edges[i])))
            bin_income = vmin(width[i], past) if i < T else past  # the top bin's size is inf
            bin_taxes.append(mul(taus_b[i], bin_income) if bin_income.x != 0 or bin_income.e != 0 else ZERO)
        due = vmax(ZERO, vsum(bin_taxes))
        rates.append(div(sub(due, last_total), sub(V(cut[bi + 1]), V(cut[bi]))))
        last_total = due
    rates.append(taus_b[T])
    rates = [clip(r, float(cfg["rate_min"]), float(cfg["rate_max"])) for r in rates]
    avg = [add(mul(V(float(running_avg[bi])), V(0.99)), mul(rates[bi], V(0.01))) for bi in range(NB)]

    nom, err = {}, {}
    for k, v in out.items():
        nom[k], err[k] = _fl(v)
    for k, vs in (("next_rates", rates), ("running_avg", avg)):
        pairs = [_fl(v) for v in vs]
        nom[k] = np.array([p[0] for p in pairs])
        err[k] = np.array([p[1] for p in pairs])
    return {"nom": nom, "err": err, "branch": branch, "n_empty": int((counts == 0).sum()), "std": std, "usable": m}


def ratio(got, nom, err):
    """|got - nom| / err elementwise; 0 where both vanish (an exact result met exactly), inf for a miss of an exact one"""
    got, nom, err = np.asarray(got, np.float64), np.asarray(nom, np.float64), np.asarray(err, np.float64)
    dlt = np.abs(got - nom)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dlt == 0, 0.0, dlt / err)
    return np.where(np.isnan(r), np.inf, r)
