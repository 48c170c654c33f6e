"""A correctly rounded restatement of one COVID-19 day, with the band every faithful evaluation must land in.

Not a conftest: a plain helper of tests/test_covid_numerics.py.  It follows the reference's own op order
(F/scenarios/covid19/covid19_env.py -- sir_step :1477-1515, unemployment_step :1374-1441, economy_step :1444-1475,
compute_reward :995-1173), not the kernel's:

- basic operations run in NumPy at the dtype NumPy gives them there (exact IEEE operations; `m` must hold the model
  constants with the reference's dtypes -- float32 arrays and scalars, int32 population, Python ints -- as
  covid19_model.build_model returns them);
- the transcendental results (float32 `**` in the CRRA term, float64 `exp` / `log` in the softplus) come from mpmath
  at PREC bits, rounded once to the op's dtype;
- the float64 filter-bank sum is the exact sum of the reference's float64 products (math.fsum), widened by the
  order-independent bound gamma(n + 2) * sum|terms|, n = filter_len * num_filters: the reference adds them pairwise, the
  kernel per filter (FMA) and then weighted.

`day()` returns, per output, the correctly rounded value ("nom") and the band [lo, hi] the recipe spans over every
combination of +-K ulps on each transcendental result and of the sum bound.  Every op of the recipe is monotone in
each of its operands, so the band's ends are reached at the corners of that box (evaluated below, the planner's sums
included: every state's productivity moves the same way at a corner).  Results a correct library returns exactly
(exp(0) = 1, log(1) = 0, pow(x, 0) = pow(1, y) = 1) are not perturbed.
"""
import math

import mpmath
import numpy as np
from mpmath.libmp import from_float

F32 = np.float32
PREC = 160  # bits (48 decimal digits)

# ulps allowed on each transcendental result, from measurements against this module's correctly rounded values
# (tests/test_covid_numerics.py: test_device_math_ulp_error, test_host_numpy_math_ulp_error -- the numbers are there)
K_POWF = 2
K_EXP = 1
K_LOG = 1


def _rn(v, p, qmin):
    """mpf -> the nearest float with a p-bit significand and exponent >= qmin (ties to even), as a Python float."""
    if not v:
        return 0.0
    _, e = mpmath.frexp(v)
    q = max(int(e) - p, qmin)
    n = int(mpmath.nint(mpmath.ldexp(v, -q)))
    try:
        return math.ldexp(n, q)
    except OverflowError:
        return math.copysign(math.inf, n)


def _mpf(x):
    return mpmath.mpf(from_float(float(x)))


def _unique_map(fn, a):
    """fn on every distinct value of a (many arguments repeat: clipped CRRA inputs, unchanged windows)."""
    a = np.asarray(a)
    u, inv = np.unique(a, return_inverse=True)
    with mpmath.workprec(PREC):
        out = np.array([fn(x) for x in u.tolist()])
    return out[inv].reshape(a.shape)


def cr_powf(ax, ome):
    """float32 ax ** float32 ome, correctly rounded to float32."""
    y = _mpf(ome)

    def f(x):
        if x == 1.0 or float(ome) == 0.0:
            return 1.0
        return _rn(mpmath.power(_mpf(x), y), 24, -149)

    return _unique_map(f, np.asarray(ax, F32)).astype(F32)


def cr_exp(x):
    def f(v):
        if v == 0.0:
            return 1.0
        if v > 710.0:
            return math.inf
        return _rn(mpmath.exp(_mpf(v)), 53, -1074)

    return _unique_map(f, np.asarray(x, np.float64)).astype(np.float64)


def cr_log(x):
    def f(v):
        if v == 1.0:
            return 0.0
        if v == math.inf:
            return math.inf
        return _rn(mpmath.log(_mpf(v)), 53, -1074)

    return _unique_map(f, np.asarray(x, np.float64)).astype(np.float64)


def ulps(a, k, exact=None):
    """a moved k ulps (k < 0: down) in its own dtype; entries where `exact` holds stay put."""
    a = np.asarray(a)
    out = a.copy()
    target = np.array(np.inf if k > 0 else -np.inf, a.dtype)
    for _ in range(abs(k)):
        out = np.nextafter(out, target)
    if exact is not None:
        out = np.where(exact, a, out)
    return out.astype(a.dtype)


def ulp_distance(a, b):
    """|a - b| in units of the last place of the (float32 or float64) correctly rounded value b."""
    a, b = np.asarray(a), np.asarray(b)
    itype = np.int32 if a.dtype == np.float32 else np.int64
    ia = a.view(itype).astype(np.int64)
    ib = b.view(itype).astype(np.int64)
    # map the sign-magnitude encoding onto a monotone integer line
    ia = np.where(ia < 0, np.iinfo(itype).min - ia, ia)
    ib = np.where(ib < 0, np.iinfo(itype).min - ib, ib)
    return np.abs(ia - ib)


# ---- pieces of the reference's day ----
def sir(m, S1, I1, R1, V1, lvl, vac):
    """sir_step + the state update of scenario_step (:744-792), in the reference's dtypes: all basic operations."""
    beta = (m["beta_intercepts"][None] * 1 + (m["beta_slopes"][None] * 1) * lvl.astype(np.int32)).astype(F32)
    vac = vac.astype(np.int32)
    sfv = np.minimum(np.ones(S1.shape, np.int32), vac / (S1 + 1e-10)).astype(F32)
    vacc_t = np.minimum(vac, S1)
    si_over_n = (S1 / m["us_state_population"][None]) * I1
    dS = (-beta * si_over_n * (1 - sfv) - vacc_t).astype(F32)
    dR = (m["gamma"] * I1 + vacc_t).astype(F32)
    dI = -dS - dR
    dV = vacc_t.astype(F32)
    S = np.maximum(S1 + dS, 0)
    I = np.maximum(I1 + dI, 0)  # noqa: E741
    R = np.maximum(R1 + dR, 0)
    V = np.maximum(V1 + dV, 0)
    D = m["death_rate"] * (R - V)
    return dict(susceptible=S, infected=I, recovered=R, vaccinated=V, deaths=D)


def filter_sum_band(m, window):
    """window: [B, L + 1, n] the daily stringency levels of the window (the day before it first, today last).
    Returns (x_nom, x_lo, x_hi) [B, n] float64: the correctly rounded exact sum of the reference's products
    (delta * w) * filter, and the band every summation order of those products (or of the kernel's FMA per filter,
    then weighted) stays inside."""
    window = np.asarray(window, np.float64)
    B, L1, n = window.shape
    L = L1 - 1
    w = np.asarray(m["conv_weights"], np.float64)  # [n, F] (float32 values)
    filt = np.asarray(m["unemp_conv_filters"], np.float64)  # [F, L]
    F = filt.shape[0]
    delta = window[:, 1:] - window[:, :-1]  # [B, L, n] small integers, exact
    nterms = L * F
    u = 2.0 ** -53
    gamma = (nterms + 2) * u / (1 - (nterms + 2) * u)
    x_nom = np.zeros((B, n))
    x_lo = np.zeros((B, n))
    x_hi = np.zeros((B, n))
    bb, ll, ss = np.nonzero(delta)
    order = np.lexsort((ll, ss, bb))
    bb, ll, ss = bb[order], ll[order], ss[order]
    keys = bb * n + ss
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    ends = np.r_[starts[1:], len(keys)]
    for a, z in zip(starts.tolist(), ends.tolist()):
        b, s = int(bb[a]), int(ss[a])
        d = delta[b, ll[a:z], s]  # [k]
        terms = ((d[:, None] * w[s][None, :]) * filt[:, ll[a:z]].T).ravel()  # the reference's float64 products
        x = math.fsum(terms.tolist())
        r = gamma * math.fsum(np.abs(terms).tolist())
        x_nom[b, s] = x
        x_lo[b, s] = np.nextafter(x - r, -np.inf)
        x_hi[b, s] = np.nextafter(x + r, np.inf)
    return x_nom, x_lo, x_hi


def softplus_recipe(x, ex, lg_of):
    """The reference's softplus (:1358-1372, beta = 1) given exp(x) = ex and a log: log(1 + ex) * (x <= 20) + x * (x > 20)."""
    y = lg_of(1 + ex)
    return y * (x <= 20) + x * (x > 20)


def excess_band(m, window, k_exp=None, k_log=None):
    """excess unemployment (the softplus of the filter sum): nominal and band, [B, n] float64."""
    k_exp = K_EXP if k_exp is None else k_exp
    k_log = K_LOG if k_log is None else k_log
    x_nom, x_lo, x_hi = filter_sum_band(m, window)
    out = []
    for x, k in ((x_nom, 0), (x_lo, -1), (x_hi, 1)):
        ex = ulps(cr_exp(x), k * k_exp, exact=x == 0)
        out.append(softplus_recipe(x, ex, lambda v: ulps(cr_log(v), k * k_log, exact=v == 1)))
    return out  # nom, lo, hi


def unemployed_from_excess(m, excess):
    return (excess + m["unemployment_bias"][None]) * m["us_state_population"][None] / 100


def productivity(m, I, D, unemployed, subsidy):
    """economy_step + the subsidy (:787-792): postsubsidy productivity, float32."""
    incap = (m["infection_too_sick_to_work_rate"] * I) + D
    cant = (incap * m["population_between_age_18_65"]) + unemployed
    workers = m["us_state_population"][None] * m["population_between_age_18_65"]
    prod = (np.maximum(0, workers - cant) * m["daily_production_per_worker"]).astype(F32)
    return prod + subsidy


def crra_recipe(m, x, pw):
    """crra_nonlinearity (:1056-1078) with ax ** (1 - eta) given as pw(ax, 1 - eta)."""
    eta = m["economic_reward_crra_eta"]
    ax = np.clip(m["num_days_in_an_year"] * x, 0.1, 3)
    return (1 + (pw(ax, 1 - eta) - 1) / (1 - eta)) / m["num_days_in_an_year"]


def crra_band(m, xs, k_pow=None):
    """xs: (nominal, one corner, the other corner) of the CRRA input.  Returns (nom, lo, hi) over +-k ulps of powf."""
    k_pow = K_POWF if k_pow is None else k_pow
    nom = crra_recipe(m, xs[0], cr_powf)
    vals = [nom]
    for x in xs[1:]:
        for k in (-k_pow, k_pow):
            def pw(ax, ome, k=k):
                return ulps(cr_powf(ax, ome), k, exact=(ax == 1) | (ome == 0))
            vals.append(crra_recipe(m, x, pw))
    with np.errstate(invalid="ignore"):
        lo = np.minimum.reduce(vals[1:])
        hi = np.maximum.reduce(vals[1:])
    return nom, lo, hi


def minmax(x, lo, hi):
    return (x - lo) / (hi - lo + 1e-10)


def _band3(vals):
    with np.errstate(invalid="ignore"):
        return vals[0], np.minimum.reduce(vals[1:]), np.maximum.reduce(vals[1:])


def day(m, pre, lvl, vac, window, subsidy, k_pow=None, k_exp=None, k_log=None, sir_state=None):
    """One day of B replicas.

    pre: dict of the previous day's float32 state [B, n] (susceptible, infected, recovered, vaccinated, deaths);
    lvl: [B, n] the stringency level beta_delay days ago (the SIR's); vac: [B, n] vaccines delivered for this day;
    window: [B, L + 1, n] the stringency levels of the filter window ending with today's; subsidy: [B, n] float32;
    sir_state: optional dict of today's S/I/R/V/D to use instead of the restated SIR (an injected day).

    Returns a dict: exact results as arrays (the SIR state, the agents' health term `h`, the planner's health term
    `ph`), banded results as (nom, lo, hi) triples."""
    r = {}
    st = sir(m, pre["susceptible"], pre["infected"], pre["recovered"], pre["vaccinated"], lvl, vac) \
        if sir_state is None else sir_state
    r.update(st)
    ex = excess_band(m, window, k_exp, k_log)
    U = [unemployed_from_excess(m, e) for e in ex]
    r["unemployed"] = tuple(U)
    P = [productivity(m, st["infected"], st["deaths"], u, subsidy) for u in U]  # more unemployed: less productivity
    r["postsubsidy_productivity"] = (P[0], P[2], P[1])
    # ---- compute_reward :995-1173 ----
    md = st["deaths"] - pre["deaths"]
    h = (-md.astype(F32) * m["value_of_life"] / m["agents_health_norm"][None]).astype(F32)
    h = minmax(h, m["min_marginal_agent_health_index"][None], m["max_marginal_agent_health_index"][None]).astype(F32)
    r["h"] = h
    e = crra_band(m, [p / m["agents_economic_norm"][None] for p in P], k_pow)
    e = [minmax(v, m["min_marginal_agent_economic_index"][None],
                m["max_marginal_agent_economic_index"][None]).astype(F32) for v in e]
    r["e"] = _band3([e[0], e[1], e[2]])
    wh = m["weightage_on_marginal_agent_health_index"][None]
    we = m["weightage_on_marginal_agent_economic_index"][None]
    ra = [(wh * h + we * v) / (wh + we) / m["reward_normalization_factor"] for v in e]
    r["rew_a"] = _band3(ra)
    ph = -np.sum(md, axis=1).astype(F32) * m["value_of_life"] / m["planner_health_norm"]
    ph = minmax(ph, m["min_marginal_planner_health_index"], m["max_marginal_planner_health_index"])
    r["ph"] = ph
    cost = (1 + m["risk_free_interest_rate"]) * np.sum(subsidy, axis=1)
    pe = crra_band(m, [(np.sum(p, axis=1) - cost) / m["planner_economic_norm"] for p in P], k_pow)
    pe = [minmax(v, m["min_marginal_planner_economic_index"], m["max_marginal_planner_economic_index"]) for v in pe]
    r["pe"] = _band3(pe)
    wph = m["weightage_on_marginal_planner_health_index"]
    wpe = m["weightage_on_marginal_planner_economic_index"]
    rp = [(wph * ph + wpe * v) / (wph + wpe) / m["reward_normalization_factor"] for v in pe]
    r["rew_p"] = _band3(rp)
    return r


def inside(x, band, where, tol=0.0):
    """Asserts lo <= x <= hi elementwise (NaN where the recipe gives NaN); returns the largest excursion past the
    band's ends (0 inside)."""
    _, lo, hi = band
    x = np.asarray(x, np.float64)
    lo = np.asarray(lo, np.float64)
    hi = np.asarray(hi, np.float64)
    nan = np.isnan(lo) | np.isnan(hi)
    assert np.array_equal(np.isnan(x), nan), "%s: NaN pattern differs from the recipe's" % where
    with np.errstate(invalid="ignore"):
        out = np.where(nan, 0.0, np.maximum(lo - x, x - hi))
    worst = float(out.max()) if out.size else 0.0
    if worst > tol:
        i = np.unravel_index(int(np.argmax(out)), out.shape)
        raise AssertionError("%s: %r outside [%r, %r] at %s (by %.3g)" % (where, x[i], lo[i], hi[i], i, worst))
    return worst


def width(band):
    _, lo, hi = band
    with np.errstate(invalid="ignore"):
        d = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    d = d[~np.isnan(d)]
    return float(d.max()) if d.size else 0.0
