"""The Saez formula (csrc/aie_kernels_saez.hip, its C restatement, the live reference) against the reference's recipe in
real arithmetic with a derived band (tests/saez_exact.py), at the buffers where the formula's code can go wrong.

One input table per SAEZ_CASES configuration (`inputs(case)`), shared by the CPU and the GPU tests: buffer lengths
around the wavefront (1 .. 500), incomes on and one ulp off the bin edges and the top cutoff, signed zeros, everybody
above the top cutoff / negative / zero, a lone occupied bin, 9 against 10 usable OLS samples, spread / four-valued /
constant / clustered rates (sd 1e-2 .. 2e-6), a negative fitted elasticity, the annealed limit and the clips, and the
global-plus-local buffer with `additions` on either side of the local length.  Every output of every evaluation must
lie within nom +- err; err is derived (saez_exact's docstring), so the band is a few u on ordinary buffers and widens by
itself where the 2x2 normal equations cancel.

- CPU, `reference`: the live reference's compute_and_set_new_period_rates_from_saez_formula().
- CPU: the C restatement (OracleEnv.saez_period_start).
- CPU: a NumPy transcription of the recipe passes with serial, pairwise and 64-way strided sums; ten one-line mutants
  of it each leave the band on some input (the band can fail).
- GPU: aie_saez_kernel, one replica per input, one step; and the sample buffer's move in the step kernel's tax_enact
  against the restatement bit for bit.

Worst |got - nom| / err per output group (elasticity estimates; bracket rates and running average) over the four
configurations; run with -s for the per-configuration figures:
    live reference    elasticity 0.132  rates 0.646
    C restatement     elasticity 0.132  rates 0.646
    aie_saez_kernel   elasticity 0.132  rates 0.646  (MI355X)
(the worst cases are the recipe's last few operations -- a bracket rate into the running average, the fitted
elasticity into its moving average -- where the band is a few u wide and all three round alike.)
"""
import functools

import numpy as np
import pytest

import saez_exact as sx
from helpers import make_env

GROUPS = {"elasticity": ("elas_t", "elas_tm1", "log_z0_t", "log_z0_tm1"), "rates": ("next_rates", "running_avg")}
LENGTHS = (1, 9, 10, 24, 63, 64, 65, 128, 500)
GLOBAL_CAP = 512


def _cases():
    from test_oracle_vs_reference import SAEZ_CASES

    return sorted(SAEZ_CASES)


@functools.lru_cache(maxsize=None)
def _case(case):
    """The configuration's environment config and the numbers of its tax component the formula reads."""
    from test_oracle_vs_reference import _saez_cfg

    cfg, _ = _saez_cfg(case)
    tax = make_env(cfg).get_component("PeriodicBracketTax")
    top = float(tax.bracket_cutoffs[-1])
    return dict(cfg=cfg, cutoffs=np.asarray(tax.bracket_cutoffs, np.float64), NB=int(tax.n_brackets), top=top,
                rate_min=float(tax.rate_min), rate_max=float(tax.rate_max),
                annealing=None if tax.tax_annealing_schedule is None else
                (float(tax._annealing_warmup), float(tax._annealing_slope)),
                pareto_uniform=tax.pareto_weight_type == "uniform", fixed_elas=tax._saez_fixed_elas,
                edges=np.linspace(0, top, 101))


def _rate_limit(c, completions):
    """curr_rate_max: rate_max, or the annealed limit min(max(slope * (completions - warmup), 0), 1) * rate_max"""
    if c["annealing"] is None:
        return c["rate_max"]
    warmup, slope = c["annealing"]
    return min(max(slope * (float(completions) - warmup), 0.0), 1.0) * c["rate_max"]


def _exact_cfg(c, completions):
    return dict(bracket_cutoffs=c["cutoffs"], rate_min=c["rate_min"], rate_max=_rate_limit(c, completions),
                pareto_uniform=c["pareto_uniform"], fixed_elas=c["fixed_elas"], bin_edges=c["edges"])


# ----------------------------------------------------------------------------------------------------------------------
# the input table
# ----------------------------------------------------------------------------------------------------------------------
def _mixed_incomes(rs, m, top):
    """negative, zero, rounding-residue, in-range and above-top incomes"""
    kind = rs.randint(0, 6, size=m)
    return np.where(kind == 0, -rs.rand(m) * 3, np.where(kind == 1, 0.0, np.where(
        kind == 2, rs.rand(m) * 1e-14, np.where(kind == 5, top * (1 + rs.rand(m)), rs.rand(m) * top))))


def _clustered(rs, m, sd):
    """m rates around 0.3 whose exact standard deviation is sd (to a few u), a hair above it"""
    d = rs.randn(m)
    d = (d - d.mean()) / d.std()
    return 0.3 + d * (sd * (1 + 1e-3))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """The table: a list of dicts -- name, group (inputs of a group share one device batch: its `size` = _buffer_size
    and, for the global inputs, its global buffer), local [llen, 2], additions, glob (None or [glen, 2]), reached (the
    flag before the period start), elas [4], avg [NB], completions."""
    c = _case(case)
    top, edges, NB = c["top"], c["edges"], c["NB"]
    rs = np.random.RandomState(_cases().index(case) + 100)
    table = []

    def put(name, z, tau, size=60, group=None, additions=0, glob=None, reached=0, completions=3, elas=None):
        local = np.stack([np.asarray(z, np.float64), np.asarray(tau, np.float64)], 1)
        table.append(dict(name=name, group=group or "size%d" % size, size=size, local=local, additions=additions, glob=glob,
                          reached=reached, completions=completions,
                          elas=np.array([rs.rand() * 2, rs.rand(), rs.randn(), rs.randn()]) if elas is None else elas,
                          avg=rs.rand(NB) * 0.5))

    def spread(m):
        return rs.rand(m) * 0.9

    def inside(m):  # positive incomes inside the bins
        return (0.02 + 0.96 * rs.rand(m)) * top

    # ---- lengths: _buffer_size is the length, so `len >= _buffer_size` is decided at equality ----
    for L in LENGTHS:
        put("len%d" % L, _mixed_incomes(rs, L, top), spread(L), size=L)
    put("short_not_reached", inside(40), spread(40))  # random rates: no formula
    put("short_but_reached_before", inside(40), spread(40), reached=1)
    # ---- incomes on the edges ----
    for i in (0, 1, 50, 99, 100):
        e = edges[i]
        z = inside(60)
        z[:18] = np.repeat([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)], 6)
        put("edge%d" % i, z, spread(60))
    z = inside(60)
    z[:20] = np.tile([0.0, -0.0], 10)
    put("signed_zeros", z, spread(60))
    z = inside(60) * 0.9
    z[:6] = top
    put("some_exactly_top_nobody_above", z, spread(60))
    put("all_exactly_top", np.full(60, top), spread(60))
    put("all_above_top", top * (1 + rs.rand(60)), spread(60))
    put("all_just_above_top", np.full(60, np.nextafter(top, np.inf)), spread(60))
    put("all_negative", -rs.rand(60) * 3 - 1e-3, spread(60))
    put("all_zero", np.zeros(60), spread(60))
    put("one_bin_in_the_middle", edges[40] + rs.rand(60) * (edges[41] - edges[40]) * 0.99, spread(60))
    z = np.where(rs.rand(60) < 0.5, edges[1] + rs.rand(60) * (edges[2] - edges[1]) * 0.99,
                 edges[30] + rs.rand(60) * (edges[36] - edges[30]))
    put("bin0_empty_bin1_occupied", z, spread(60))
    # ---- 9 against 10 usable samples among 60: z > 0 and tau < 1 ----
    for k in (9, 10):
        z, tau = inside(60), spread(60)
        z[0], tau[1] = 5e-324, np.nextafter(1.0, 0.0)  # usable, both of them
        tau[k:20] = 1.0  # tau == 1: not usable
        tau[20:30] = 1.0 + rs.rand(10)
        z[30:40], z[40:50], z[50:] = 0.0, -0.0, -rs.rand(10) - 0.1  # z <= 0: not usable
        put("usable%d" % k, z, tau)
    # ---- rates ----
    put("spread", _mixed_incomes(rs, 60, top), spread(60))
    put("four_values", inside(60), rs.choice([0.0, 0.1, 0.25, 0.6], size=60))
    put("all_equal", inside(60), np.full(60, 0.35))
    for sd in (1e-2, 1e-3, 1e-4, 2e-6):
        put("clustered_sd%g" % sd, inside(60), _clustered(rs, 60, sd))
    tau = spread(60)
    put("elasticity_negative", np.exp(1.0 - 1.5 * np.log(1 - tau) + 0.1 * rs.randn(60)), tau)
    put("elasticity_positive", np.exp(1.0 + 0.8 * np.log(1 - tau) + 0.1 * rs.randn(60)), tau)
    put("elasticity_state_zero", _mixed_incomes(rs, 60, top), np.full(60, 0.2), elas=np.array([0.0, 0.3, 0.0, -1.0]))
    # ---- annealing and the clips ----
    for comp in (0, 3, 50):
        put("completions%d" % comp, _mixed_incomes(rs, 60, top), spread(60), completions=comp)
    put("top_rate_near_one", -rs.rand(60) - 0.5, spread(60), completions=50)  # nobody taxable: the top rate is 1 / (1 + 1e-9)
    put("low_rates", inside(60) * 0.05, spread(60), completions=50)  # everybody in the lowest bins
    # ---- the trainer's global buffer followed by min(additions, llen) local samples ----
    for glen, size, llen in ((37, 40, 20), (64, 64, 20), (450, 455, 30)):
        glob = np.stack([_mixed_incomes(rs, glen, top), spread(glen)], 1)
        for adds in (0, 5, llen, llen + 13):
            put("global%d_additions%d" % (glen, adds), _mixed_incomes(rs, llen, top), spread(llen), size=size,
                group="global%d" % glen, additions=adds, glob=glob)
    return table


@functools.lru_cache(maxsize=None)
def exact(case):
    """Per input of the table: the exact model's decision `reached`, and saez_exact.period_start's result where the
    formula runs (None where the buffer stays short: random rates).  The generator's conditions are asserted here."""
    c = _case(case)
    out = []
    for inp in inputs(case):
        samples = sx.effective_buffer(inp["local"], inp["additions"], inp["glob"])
        reached = bool(inp["reached"]) or len(samples) >= inp["size"]
        r = None
        if reached:
            r = sx.period_start(samples, inp["elas"], inp["avg"], _exact_cfg(c, inp["completions"]))
            if r["std"] is not None:
                assert r["std"] <= 0.5e-6 or r["std"] >= 2e-6, "%s %s: std %g too near 1e-6" % (case, inp["name"], r["std"])
            for k, e in r["err"].items():
                assert np.all(np.isfinite(e)), "%s %s: no finite band for %s" % (case, inp["name"], k)
        out.append(dict(reached=reached, n=len(samples), r=r))
    return out


def _outputs_of(elas4, next_rates, running_avg):
    return {"elas_t": elas4[0], "elas_tm1": elas4[1], "log_z0_t": elas4[2], "log_z0_tm1": elas4[3],
            "next_rates": np.asarray(next_rates, np.float64), "running_avg": np.asarray(running_avg, np.float64)}


def _worst_ratios(got, r):
    """{group: worst |got - nom| / err}"""
    return {g: max(float(np.max(sx.ratio(got[k], r["nom"][k], r["err"][k]))) for k in keys) for g, keys in GROUPS.items()}


def _check_band(who, case, results):
    """results: [(input, exact entry, outputs dict)]; asserts the band, prints and returns the worst ratios."""
    worst = dict.fromkeys(GROUPS, 0.0)
    for inp, ex, got in results:
        w = _worst_ratios(got, ex["r"])
        for g in GROUPS:
            assert w[g] <= 1.0, "%s, %s, input %s (branch %s): %s at %.3g of its band\n got %r\n nom %r\n err %r" % (
                who, case, inp["name"], ex["r"]["branch"], g, w[g], {k: got[k] for k in GROUPS[g]},
                {k: ex["r"]["nom"][k] for k in GROUPS[g]}, {k: ex["r"]["err"][k] for k in GROUPS[g]})
            worst[g] = max(worst[g], w[g])
    print("%s, %s: worst |got - nom| / err: %s over %d inputs" % (
        who, case, ", ".join("%s %.3g" % (g, worst[g]) for g in GROUPS), len(results)))
    return worst


def _assert_coverage(case):
    """Every branch, length and edge the table promises, from the exact model's record."""
    c = _case(case)
    ins, exs = inputs(case), exact(case)
    ran = [(i, e) for i, e in zip(ins, exs) if e["reached"]]
    branches = {e["r"]["branch"] for _, e in ran}
    assert branches == set(sx.BRANCHES), branches
    assert set(LENGTHS) <= {e["n"] for _, e in ran}
    assert any(not e["reached"] for e in exs)
    by = {i["name"]: e for i, e in zip(ins, exs)}
    assert by["usable9"]["r"]["usable"] == 9 and by["usable9"]["r"]["branch"] == "count"
    assert by["usable10"]["r"]["usable"] == 10 and by["usable10"]["r"]["branch"] in ("ols", "ols_clipped")
    assert by["all_equal"]["r"]["branch"] == "std" and by["elasticity_negative"]["r"]["branch"] == "ols_clipped"
    assert by["all_above_top"]["r"]["n_empty"] == 100 and by["all_negative"]["r"]["n_empty"] == 100
    assert by["all_exactly_top"]["r"]["n_empty"] == 99 and by["all_zero"]["r"]["n_empty"] == 99 and by["one_bin_in_the_middle"]["r"]["n_empty"] == 99
    for sd in (1e-2, 1e-3, 1e-4, 2e-6):
        assert by["clustered_sd%g" % sd]["r"]["branch"].startswith("ols")
        assert sd <= by["clustered_sd%g" % sd]["r"]["std"] <= sd * 1.01
    for glen, llen in ((37, 20), (64, 20), (450, 30)):
        assert [by["global%d_additions%d" % (glen, a)]["n"] for a in (0, 5, llen, llen + 13)] == \
            [glen, glen + 5, glen + llen, glen + llen]
    assert not by["global37_additions0"]["reached"] and by["global64_additions0"]["reached"]
    rates = np.concatenate([e["r"]["nom"]["next_rates"] for _, e in ran])
    if c["rate_min"] > 0:  # the formula's rates are positive: only a floor above 0 can be hit
        assert (rates == c["rate_min"]).any()
    if _rate_limit(c, 0) < 1.0:  # the formula's rates stay below 1: only a limit below 1 can be hit
        assert any((e["r"]["nom"]["next_rates"] == _rate_limit(c, i["completions"])).any() for i, e in ran)


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the live reference, the C restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _cases())
def test_table_covers_what_it_promises(case):
    assert 40 <= len(inputs(case)) <= 70
    _assert_coverage(case)


@pytest.mark.reference
@pytest.mark.parametrize("case", _cases())
def test_live_reference_lies_in_the_band(case):
    """The reference's own period start on every input of the table, through its own state fields."""
    from test_oracle_vs_reference import _ref_env

    c = _case(case)
    np.random.seed(9)
    ref = _ref_env(c["cfg"])
    from ai_economist.foundation.components.utils import annealed_tax_limit

    ref.reset()
    tc = ref.get_component("PeriodicBracketTax")
    assert np.array_equal(tc._saez_income_bin_edges, c["edges"]) and np.array_equal(tc.bracket_cutoffs, c["cutoffs"])
    results = []
    for inp, ex in zip(inputs(case), exact(case)):
        tc._buffer_size = inp["size"]
        tc._local_saez_buffer = inp["local"].tolist()
        tc._global_saez_buffer = [] if inp["glob"] is None else inp["glob"].tolist()
        tc._additions_this_episode = inp["additions"]
        tc._reached_min_samples = bool(inp["reached"])
        tc.elas_t, tc.elas_tm1, tc.log_z0_t, tc.log_z0_tm1 = [float(v) for v in inp["elas"]]
        tc.running_avg_tax_rates = inp["avg"].copy()
        if tc.tax_annealing_schedule is not None:
            tc._last_completions = inp["completions"]
            tc._annealed_rate_max = annealed_tax_limit(inp["completions"], tc._annealing_warmup, tc._annealing_slope,
                                                       tc.rate_max)
            assert tc._annealed_rate_max == _rate_limit(c, inp["completions"])
        assert len(tc.saez_buffer) == ex["n"]
        tc.compute_and_set_new_period_rates_from_saez_formula()
        assert bool(tc._reached_min_samples) == ex["reached"], inp["name"]
        if ex["reached"]:
            results.append((inp, ex, _outputs_of([tc.elas_t, tc.elas_tm1, tc.log_z0_t, tc.log_z0_tm1],
                                                 tc.curr_bracket_tax_rates, tc.running_avg_tax_rates)))
    _check_band("live reference", case, results)


def _set_oracle_state(o, e, inp):
    n = len(inp["local"])
    o.t["saez_buffer"][e][:n] = inp["local"]
    o.t["saez_buffer_len"][e] = n
    o.t["saez_additions"][e] = inp["additions"]
    o.t["saez_reached_min_samples"][e] = inp["reached"]
    o.t["saez_elas"][e] = inp["elas"]
    o.t["saez_running_avg_tax_rates"][e] = inp["avg"]
    o.t["tax_last_completions"][e] = inp["completions"]
    o.t["tax_cycle_pos"][e] = 1


def _groups(case):
    """[(group name, size, glob, [(input, exact entry)])] in table order"""
    out = {}
    for inp, ex in zip(inputs(case), exact(case)):
        out.setdefault(inp["group"], (inp["group"], inp["size"], inp["glob"], []))[3].append((inp, ex))
    return list(out.values())


def _host_for(case, size, n_envs, **kw):
    host = make_env(_case(case)["cfg"], n_envs=n_envs, **kw)
    tax = host.get_component("PeriodicBracketTax")
    tax._buffer_size = size
    tax._global_buffer_capacity = GLOBAL_CAP
    return host


@pytest.mark.parametrize("case", _cases())
def test_c_restatement_lies_in_the_band(case):
    from oracle_lib import OracleEnv

    results = []
    for _, size, glob, members in _groups(case):
        host = _host_for(case, size, len(members))
        o = OracleEnv(host.build_config(), host.layout_planes())
        o.seed(1)
        o.reset()
        if glob is not None:
            o.set_global_saez_buffer(glob)
        for e, (inp, _) in enumerate(members):
            _set_oracle_state(o, e, inp)
        o.saez_period_start()
        for e, (inp, ex) in enumerate(members):
            assert bool(o.t["saez_reached_min_samples"][e]) == ex["reached"], inp["name"]
            if ex["reached"]:
                assert np.array_equal(o.t["tax_saez_bracket_rates"][e], o.t["saez_next_rates"][e])
                results.append((inp, ex, _outputs_of(o.t["saez_elas"][e], o.t["saez_next_rates"][e],
                                                     o.t["saez_running_avg_tax_rates"][e])))
    _check_band("C restatement", case, results)


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the band must be able to fail -- a NumPy transcription of the recipe and its one-line mutants
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = ("pareto_norm_without_1e-9", "geq_z_norm_without_1e-9", "rate_denominator_without_1e-9",
           "above_is_geq_top", "half_open_last_bin", "fewer_than_9", "half_pz_dropped", "elasticity_not_clipped",
           "additions_not_capped", "running_average_098_002")


def _sum_serial(a):
    s = 0.0
    for v in np.asarray(a, np.float64).ravel():
        s = s + v
    return s


def _sum_strided(a):
    a = np.asarray(a, np.float64).ravel()
    return _sum_serial([_sum_serial(a[lane::64]) for lane in range(64)])


def _numpy_recipe(inp, c, mut=None, vsum=np.sum):
    """redistribution.py:437-823 in NumPy float64, `vsum` for every sum of more than two terms; `mut` one of MUTANTS."""
    local, glob, adds = inp["local"], inp["glob"], inp["additions"]
    if glob is None:
        buf = local
    else:
        tail = adds if mut == "additions_not_capped" else min(adds, len(local))
        buf = np.concatenate([glob, local[len(local) - tail:]]) if tail else glob
    z, tau = buf[:, 0], buf[:, 1]
    edges, T, NB = c["edges"], 100, c["NB"]
    elas_tm1, log_z0_tm1 = float(inp["elas"][0]), float(inp["elas"][2])
    use = (z > 0) & (tau < 1)
    zs, ts = z[use], tau[use]
    elas_t, log_z0_t = elas_tm1, log_z0_tm1
    if not len(zs) < (9 if mut == "fewer_than_9" else 10):
        mean = vsum(ts) / len(ts)
        if not np.sqrt(vsum((ts - mean) ** 2) / len(ts)) < 1e-6:
            x = np.log(np.maximum(1 - ts, 1e-9))
            y = np.log(np.maximum(zs, 1e-9))
            xtx = np.array([[vsum(x * x), vsum(x)], [vsum(x), float(len(x))]])
            xxi = np.linalg.inv(xtx)
            xy = np.array([vsum(x * y), vsum(y)])
            elas = xxi[0, 0] * xy[0] + xxi[1, 0] * xy[1]
            log_z0_t = xxi[0, 1] * xy[0] + xxi[1, 1] * xy[1]
            inst = elas if mut == "elasticity_not_clipped" else max(elas, 0.0)
            elas_t = ((1 - 0.98) * inst) + (0.98 * elas_tm1)
    elas4 = [elas_t, elas_tm1, log_z0_t, log_z0_tm1]
    if c["fixed_elas"] is not None:
        elas_t = float(c["fixed_elas"])
    # np.histogram: [e_i, e_i+1), the last bin closed
    keep = (z >= edges[0]) & ((z < edges[T]) if mut == "half_open_last_bin" else (z <= edges[T]))
    idx = np.minimum(np.searchsorted(edges, z[keep], side="right") - 1, T - 1)
    counts = np.bincount(idx, minlength=T).astype(np.float64)
    below = z[z < edges[0]]
    above = z[(z >= edges[T]) if mut == "above_is_geq_top" else (z > edges[T])]

    def pareto(v):
        return np.ones_like(v) if c["pareto_uniform"] else 1.0 / np.maximum(1, v)

    w_below = vsum(pareto(np.maximum(below, 0))) if len(below) else 0
    w_above = vsum(pareto(above)) if len(above) else 0
    per_bin = counts * pareto(0.5 * (edges[:-1] + edges[1:]))
    cum = vsum(per_bin)
    cum += w_below
    cum += w_above
    norm = cum if mut == "pareto_norm_without_1e-9" else cum + 1e-9
    dens = np.concatenate([per_bin, [w_above]]) / norm
    n_total = vsum(counts) + len(below) + len(above)
    pz = np.concatenate([counts, [len(above)]]) / n_total
    cd = np.array([vsum(dens[i:]) for i in range(T + 1)])
    cp = np.array([vsum(pz[i:]) for i in range(T + 1)])
    g = cd / (cp if mut == "geq_z_norm_without_1e-9" else cp + 1e-9)
    gz = np.concatenate([0.5 * (g[:-1] + g[1:]), [g[-1]]])
    cum_pz = [pz[0] + len(below) / n_total]
    for p in pz[1:]:
        cum_pz.append(min(max(cum_pz[-1] + p, 0), 1.0))
    p_geq = 1 - np.array(cum_pz) + (0 if mut == "half_pz_dropped" else 0.5 * pz)
    az = np.full(T + 1, np.nan)
    for i in range(T):
        if pz[i] != 0:
            paz = 0.5 * (edges[i] + edges[i + 1]) * pz[i] / (min(max(p_geq[i], 0), 1) + 1e-9)
            az[i] = paz / (edges[i + 1] - edges[i])
    az[T] = 0.0
    if len(above):
        mean_above = vsum(above) / len(above)
        az[T] = mean_above / (mean_above - edges[T] + 1e-9)
    taus = (1.0 - gz) / (1.0 - gz + az * elas_t + (0 if mut == "rate_denominator_without_1e-9" else 1e-9))
    last, last_i = 0.0, -1
    for i in range(T + 1):
        if np.isnan(taus[i]):
            continue
        if i - last_i > 1:
            taus[last_i + 1:i] = np.linspace(last, taus[i], i - last_i + 1)[1:-1]
        last, last_i = float(taus[i]), i
    sizes = np.concatenate([edges[1:] - edges[:-1], [np.inf]])
    rates, last_total = [], 0
    for b in range(NB - 1):
        due = max(0, vsum(taus * np.minimum(sizes, np.maximum(0, c["cutoffs"][b + 1] - edges))))
        rates.append((due - last_total) / (c["cutoffs"][b + 1] - c["cutoffs"][b]))
        last_total = due
    rates.append(taus[T])
    rates = np.clip(np.array(rates), c["rate_min"], _rate_limit(c, inp["completions"]))
    w = (0.98, 0.02) if mut == "running_average_098_002" else (0.99, 0.01)
    return _outputs_of(elas4, rates, (inp["avg"] * w[0]) + (rates * w[1]))


@pytest.mark.parametrize("summation", ["pairwise", "serial", "strided64"])
@pytest.mark.parametrize("case", _cases())
def test_numpy_transcription_lies_in_the_band(case, summation):
    """Summation order is not a mutant: np.sum (pairwise), one serial loop, 64 strided partial sums then their sum."""
    vsum = {"pairwise": np.sum, "serial": _sum_serial, "strided64": _sum_strided}[summation]
    c = _case(case)
    with np.errstate(all="ignore"):
        results = [(inp, ex, _numpy_recipe(inp, c, vsum=vsum)) for inp, ex in zip(inputs(case), exact(case))
                   if ex["reached"]]
    _check_band("NumPy transcription (%s sums)" % summation, case, results)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_band_catches_mutant(mutant):
    """Each one-line mutant of the transcription leaves the band on at least one input of every configuration's
    table in which the mutated line can matter at all."""
    for case in _cases():
        c = _case(case)
        caught = []
        with np.errstate(all="ignore"):
            for inp, ex in zip(inputs(case), exact(case)):
                if not ex["reached"]:
                    continue
                w = _worst_ratios(_numpy_recipe(inp, c, mut=mutant), ex["r"])
                if not max(w.values()) <= 1.0:  # a NaN is out of the band too
                    caught.append(inp["name"])
        print("%s, %s: caught on %d inputs: %s" % (mutant, case, len(caught), " ".join(caught[:8])))
        assert caught, "%s survives the table of %s" % (mutant, case)


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases())
def test_hip_saez_kernel_lies_in_the_band(case):
    """aie_saez_kernel: one replica per input (the inputs of a group share a batch: one _buffer_size, one global buffer),
    the state injected through the tensor views, one step at a period start.  Estimates, next rates, running average
    and the latched bracket rates within nom +- err; `reached` as the exact model decides; the MT19937 key as the
    restatement leaves it (the formula draws nothing, the short buffers draw their random rates)."""
    import torch
    from oracle_lib import OracleEnv

    _assert_coverage(case)
    results = []
    for name, size, glob, members in _groups(case):
        E = len(members)
        host = _host_for(case, size, E, device="cuda:0")
        host.seed(5)
        host.reset()
        be = host.backend
        o = OracleEnv(host.build_config(), host.layout_planes())
        o.seed(5)
        o.reset()
        assert be.tensors["saez_buffer"].shape[1] >= max(len(i["local"]) for i, _ in members)
        if glob is not None:
            assert len(glob) <= int(be.tensors["saez_global_buffer"].shape[1])
            g = torch.from_numpy(np.ascontiguousarray(glob)).to(be.device)
            be._check(be.lib.aie_set_global_saez_buffer(be.handle, g.data_ptr(), len(glob)))
            o.set_global_saez_buffer(glob)
        for e, (inp, _) in enumerate(members):
            _set_oracle_state(o, e, inp)
        for k in ("saez_buffer", "saez_buffer_len", "saez_additions", "saez_reached_min_samples", "saez_elas",
                  "saez_running_avg_tax_rates", "tax_last_completions", "tax_cycle_pos"):
            be.tensors[k].copy_(torch.from_numpy(np.ascontiguousarray(o.t[k])).to(be.tensors[k].device))
        a, p = be.sample_random_actions(seed=1)
        a, p = torch.zeros_like(a), torch.zeros_like(p)
        host.step({"a": a, "p": p})
        torch.cuda.synchronize()
        o.step(a.cpu().numpy(), p.cpu().numpy())
        got = {k: be.tensors[k].cpu().numpy() for k in ("saez_elas", "saez_next_rates", "saez_running_avg_tax_rates",
                                                        "tax_saez_bracket_rates", "saez_reached_min_samples")}
        assert np.array_equal(be.tensors["mt"].cpu().numpy().view(np.uint32), o.t["mt"]), name
        assert np.array_equal(be.tensors["mt_pos"].cpu().numpy(), o.t["mt_pos"]), name
        for e, (inp, ex) in enumerate(members):
            assert bool(got["saez_reached_min_samples"][e]) == ex["reached"], inp["name"]
            if ex["reached"]:
                assert np.array_equal(got["tax_saez_bracket_rates"][e], got["saez_next_rates"][e]), inp["name"]
                results.append((inp, ex, _outputs_of(got["saez_elas"][e], got["saez_next_rates"][e],
                                                     got["saez_running_avg_tax_rates"][e])))
    _check_band("aie_saez_kernel", case, results)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [31, 32, 33, 500])
def test_hip_saez_buffer_move_is_bit_exact(size):
    """tax_enact's _update_saez_buffer in the gather-trade-build step kernel: 5 agents append 10 doubles to a buffer two
    samples short of _buffer_size, and the oldest are dropped by moving the rest down in chunks of 64 doubles (one
    chunk, exactly one, one and a bit, sixteen).  The move computes nothing: buffer, length and additions equal the
    restatement's bit for bit after every step, over three tax days.  A one-sample global buffer keeps the replicas in
    the random-rate phase (1 + additions stays short of _buffer_size), where the appended incomes and marginal rates
    are copies of state the suite compares with == elsewhere."""
    import torch
    from oracle_lib import OracleEnv
    from test_oracle_vs_reference import SAEZ_NO_AUCTION

    cfg = dict(SAEZ_NO_AUCTION, components=[list(c) for c in SAEZ_NO_AUCTION["components"]])
    cfg["components"][-1] = ["PeriodicBracketTax", {"tax_model": "saez", "period": 3}]
    E = 6
    env = make_env(cfg, n_envs=E, device="cuda:0")
    tax = env.get_component("PeriodicBracketTax")
    tax._buffer_size = size
    tax._global_buffer_capacity = 8
    env.seed(4)
    env.reset()
    be = env.backend
    o = OracleEnv(env.build_config(), env.layout_planes())
    o.seed(4)
    o.reset()
    cap = o.t["saez_buffer"].shape[1]
    assert cap == size + 5
    one = np.array([[1.5, 0.25]])
    g = torch.from_numpy(one).to(be.device)
    be._check(be.lib.aie_set_global_saez_buffer(be.handle, g.data_ptr(), 1))
    o.set_global_saez_buffer(one)
    ramp = (np.arange(E)[:, None, None] * 10000.0 + np.arange(cap)[None, :, None] * 2.0 + np.arange(2)[None, None, :]) + 0.125
    ramp[:, size - 2:] = -7.0  # past the filled length: must never show up below it
    o.t["saez_buffer"][...] = ramp
    o.t["saez_buffer_len"][...] = size - 2
    for k in ("saez_buffer", "saez_buffer_len"):
        be.tensors[k].copy_(torch.from_numpy(np.ascontiguousarray(o.t[k])).to(be.tensors[k].device))
    rs = np.random.RandomState(2)
    moved = 0
    for t in range(9):
        a, p = be.sample_random_actions(seed=3)
        an = a.cpu().numpy().copy()
        an[rs.rand(*an.shape) < 0.35] = 1  # builds: incomes
        a = torch.as_tensor(an, device=a.device)
        env.step({"a": a, "p": p})
        torch.cuda.synchronize()
        o.step(an, p.cpu().numpy())
        n = o.t["saez_buffer_len"]
        assert np.array_equal(be.tensors["saez_buffer_len"].cpu().numpy(), n), "step %d" % (t + 1)
        assert np.array_equal(be.tensors["saez_additions"].cpu().numpy(), o.t["saez_additions"]), "step %d" % (t + 1)
        got = be.tensors["saez_buffer"].cpu().numpy()
        for e in range(E):
            assert np.array_equal(got[e, :n[e]].view(np.uint64), o.t["saez_buffer"][e, :n[e]].view(np.uint64)), \
                "step %d replica %d" % (t + 1, e)
        if (t + 1) % 3 == 0:
            moved += 1
            assert (n == size).all() and (o.t["saez_additions"] == 5 * moved).all()
            keep = size - 5 * moved  # what is left of the ramp, moved down
            if keep > 0:
                assert np.array_equal(o.t["saez_buffer"][:, :keep], ramp[:, 5 * moved - 2:size - 2])
        assert not o.t["saez_reached_min_samples"].any()
    assert moved == 3
