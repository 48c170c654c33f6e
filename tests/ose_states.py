"""States and shapes of the one-step-economy kernels (csrc/aie_kernels_ose.hip) that a uniform random policy on the
usual configurations never reaches, and how the tests get there.

  ose_cfg(n, ...)                       one-step-economy + SimpleLabor (+ WealthRedistribution) + PeriodicBracketTax with
                                        explicit skills (nothing is drawn from the global NumPy stream)
  policy_actions(case, info, ...)       scripted policies, evaluated on the host from the oracle's masks (so they respect
                                        mask_first_step and the planner's closed masks): a deterministic function of the
                                        masks, the case's seed and the step number of the run
  census(before, after, actions, info)  named reach conditions of ONE step, from state tensors only (NumPy; oracle and
                                        device tensors alike) -- what keeps the GPU tests from being vacuous
  shape_class(tensors)                  how ose_store_rows sees a case: row widths, quads per row, rows per pass
  injected_state(kind, ...)             states in the load_state format a policy cannot reach within a test's time

No test functions here: tests/test_ose_states_cpu.py checks on the oracle alone that every case below reaches the
conditions it declares and that the cases together cover every condition and every shape class (and, reference-marked,
pins the policy rollouts to the live reference); tests/test_gpu_ose_states.py runs the same cases on the device against
the oracle.

The kernel's lane edges the agent counts stand for: one lane owns agents l and l + 64, so 63 / 64 / 65 and 127 / 128 are
the last lane of the first slot, a full first slot, one agent in the second slot (rank_sort's +inf padding fills 63 of
its 64 places; the permutation skip starts at a mask group with one index) and both slots full but one; 29 / 30 / 31
straddle get_gini's switch from the pairwise difference matrix to the sorted cumulative sum; 2 and 3 are the smallest.
"""
import numpy as np

COMP = {4: "PeriodicBracketTax", 5: "SimpleLabor", 9: "WealthRedistribution"}
TAX_MODEL_WRAPPER = 0
STATE_KEYS = ("inv_coin", "esc_coin", "labor", "production", "tax_cycle_pos", "tax_rate_idx", "tax_last_coin",
              "tax_last_income", "tax_last_marginal_rate", "metrics_tax_days", "metrics_tax_paid_sum", "timestep", "done")
LOAD_KEYS = ("inv_coin", "esc_coin", "tax_last_coin", "labor", "production", "tax_cycle_pos", "tax_rate_idx")

CONDITIONS = ("top_bracket_occupied", "every_bracket_occupied", "income_on_cutoff", "income_negative", "income_tiny",
              "all_incomes_tied", "all_coin_zero", "one_agent_holds_all_coin", "cycle_pos_ge_3", "no_tax_day_in_episode",
              "tax_takes_all_coin", "rate_index_top", "planner_mask_closed_mid_period", "gini_pairwise_branch",
              "gini_sorted_branch", "second_lane_slot_used", "eta_is_one")


def snapshot(tensors, sl=None):
    """Copies of the state tensors the census reads, as NumPy arrays (oracle arrays or device tensors)."""
    out = {}
    for k in STATE_KEYS:
        if k in tensors:
            v = tensors[k]
            v = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
            out[k] = np.array(v if sl is None else v[sl])
    return out


class Info:
    """What the census and the policies need to know about a configuration: from a host environment, or -- the census'
    self-test -- from keywords."""

    def __init__(self, env=None, **kw):
        if env is not None:
            c = env.build_config()
            names_p = env.action_subspace_names()[1]
            nb = int(c.tax_n_brackets)
            comps = [COMP.get(int(x), "?") for x in list(c.components)[: c.n_components]]
            has_tax = "PeriodicBracketTax" in comps
            kw = dict(n=int(c.n_agents), comps=comps, NB=nb if has_tax else 0,
                      cut=np.array(list(c.tax_bracket_cutoffs)[:nb], np.float64), period=int(c.tax_period),
                      tax_model=int(c.tax_model), disc=np.array(list(c.tax_disc_rates)[: c.tax_n_disc_rates], np.float64),
                      fixed=np.array(list(c.tax_fixed_rates)[:nb], np.float64), n_sub_p=len(names_p),
                      sub_p_dim=int(names_p[0][1]) if names_p else 0, multi_p=bool(c.multi_action_mode_planner),
                      episode_length=int(c.episode_length), isoelastic=int(c.ose_agent_reward_type) == 1,
                      eta=float(c.isoelastic_eta), num_hours=int(c.labor_num_hours))
            assert not c.tax_annealing and not c.tax_disable  # (rates() below knows neither)
        self.__dict__.update(kw)
        self.has_tax = "PeriodicBracketTax" in self.comps

    def rates(self, t):
        """[E, NB] marginal rates in force: the planner's choice (model_wrapper) or the fixed schedule."""
        if self.tax_model == TAX_MODEL_WRAPPER:
            return self.disc[t["tax_rate_idx"]]
        return np.broadcast_to(self.fixed, (len(t["tax_cycle_pos"]), self.NB))


def taxes_due(info, rates, inc):
    """taxes_due (redistribution.py:846-851) for incomes [D, n] under rates [D, NB]."""
    size = np.append(np.diff(info.cut), np.inf)
    binned = np.minimum(size[None, None, :], np.maximum(inc[:, :, None] - info.cut[None, None, :], 0.0))
    return (rates[:, None, :] * binned).sum(2)


def census(before, after, actions, info):
    """{condition: bool} for one step of E replicas.  before / after: snapshot()s around the step (after: ahead of any
    reset), actions: the agents' action buffer (unused by today's conditions, kept for the signature the callers share).
    A tax day is a step that starts with tax_cycle_pos >= period (only the tax component moves that counter).
    `bracket_counts` (int [NB]) is extra: Reach adds it up for every_bracket_occupied."""
    n = info.n
    out = {k: False for k in CONDITIONS}
    out["bracket_counts"] = np.zeros(max(info.NB, 1), np.int64)
    coin = after["inv_coin"] + after["esc_coin"]
    out["all_coin_zero"] = bool(((coin == 0).all(1) & (after["labor"] > 0).any(1)).any())
    out["one_agent_holds_all_coin"] = bool((((coin > 0).sum(1) == 1) & ((coin == 0).sum(1) == n - 1)).any())
    out["gini_pairwise_branch"] = n < 30
    out["gini_sorted_branch"] = n >= 30
    out["second_lane_slot_used"] = n > 64
    out["eta_is_one"] = bool(info.isoelastic and info.eta == 1.0)
    if not info.has_tax:
        return out
    pos = after["tax_cycle_pos"]
    out["cycle_pos_ge_3"] = bool((pos >= 3).any())
    out["planner_mask_closed_mid_period"] = bool(info.n_sub_p > 0 and ((pos > 1) & (pos < info.period)).any())
    out["no_tax_day_in_episode"] = bool(info.period > info.episode_length
                                        and ((after["done"] != 0) & (after["metrics_tax_days"] == 0)).any())
    if info.tax_model == TAX_MODEL_WRAPPER:
        out["rate_index_top"] = bool((after["tax_rate_idx"] == len(info.disc) - 1).any())
    day = before["tax_cycle_pos"] >= info.period
    if day.any():
        inc = after["tax_last_income"][day]  # [D, n]
        nonneg = inc >= 0
        b = np.clip(np.searchsorted(info.cut, inc, side="right") - 1, 0, info.NB - 1)
        out["bracket_counts"] = np.bincount(b[nonneg].reshape(-1), minlength=info.NB).astype(np.int64)
        out["top_bracket_occupied"] = bool(out["bracket_counts"][info.NB - 1] > 0)
        out["income_on_cutoff"] = bool(np.isin(inc, info.cut[1:]).any())
        out["income_negative"] = bool((inc < 0).any())
        out["income_tiny"] = bool(((inc > 0) & (inc < 1e-6)).any())
        out["all_incomes_tied"] = bool(((inc == inc[:, :1]).all(1) & (inc[:, 0] > 0)).any())
        due = taxes_due(info, info.rates(after)[day], inc)  # (rate indices change at period starts, ahead of the levy)
        paid = (after["metrics_tax_paid_sum"] - before["metrics_tax_paid_sum"])[day]
        out["tax_takes_all_coin"] = bool(((paid < due * (1 - 1e-9)) & (before["esc_coin"][day] > 0)).any())
    return out


class Reach:
    """Union of census() results over the steps of a case."""

    def __init__(self):
        self.flags, self.brackets = {k: False for k in CONDITIONS}, None

    def add(self, c):
        for k in CONDITIONS:
            self.flags[k] = self.flags[k] or bool(c[k])
        b = c["bracket_counts"]
        if b.sum():
            self.brackets = b if self.brackets is None else self.brackets + b

    def result(self):
        out = dict(self.flags)
        out["every_bracket_occupied"] = self.brackets is not None and bool((self.brackets > 0).all())
        return out

    def reached(self):
        return sorted(k for k, v in self.result().items() if v)


def shape_class(tensors):
    """How ose_store_rows sees a configuration, from the tensor shapes alone: FA / MA floats per agent row, L4 = quads
    per row, rows per pass of one wavefront; MP = the planner's mask entries."""
    fa, ma = int(tensors["obs_a_flat"].shape[-1]), int(tensors["obs_a_action_mask"].shape[-1])
    out = dict(n=int(tensors["obs_a_flat"].shape[1]), FA=fa, MA=ma, MP=int(tensors["obs_p_action_mask"].shape[-1]))
    for k, f in (("FA", fa), ("MA", ma)):
        out[k + "_L4"] = (f + 3) // 4
        out[k + "_rows_per_pass"] = 64 // ((f + 3) // 4)
    return out


# ----------------------------------------------------------------------------------------------------------------
# configurations
# ----------------------------------------------------------------------------------------------------------------
C5_TAX = dict(bracket_spacing="us-federal", period=1, tax_model="model_wrapper")
NB2_TAX = dict(bracket_spacing="linear", n_brackets=2, top_bracket_cutoff=50.0, tax_model="model_wrapper", period=1)
NB16_TAX = dict(bracket_spacing="linear", n_brackets=16, top_bracket_cutoff=320.0, tax_model="model_wrapper", period=2)
ON_CUTOFF_TAX = dict(bracket_spacing="linear", n_brackets=5, top_bracket_cutoff=100.0, tax_model="fixed-bracket-rates",
                     fixed_bracket_rates=[0.0, 0.1, 0.25, 0.5, 1.0], period=1)
LTW = ("SimpleLabor", "PeriodicBracketTax", "WealthRedistribution")
TLW = ("PeriodicBracketTax", "SimpleLabor", "WealthRedistribution")
WLT = ("WealthRedistribution", "SimpleLabor", "PeriodicBracketTax")


def default_skills(n):
    return [float(x) for x in np.sort(1 + np.random.RandomState(4).rand(n) * 2)]


def ose_cfg(n, tax=None, skills=None, order=("SimpleLabor", "PeriodicBracketTax"), episode_length=2, labor=None, **kw):
    kws = {"SimpleLabor": dict(labor or {}, skills=list(skills) if skills is not None else default_skills(n)),
           "PeriodicBracketTax": dict(C5_TAX if tax is None else tax), "WealthRedistribution": {}}
    return dict(dict(scenario_name="one-step-economy", world_size=[1, 1], n_agents=n, episode_length=episode_length,
                     components=[[name, kws[name]] for name in order]), **kw)


# ----------------------------------------------------------------------------------------------------------------
# scripted policies
# ----------------------------------------------------------------------------------------------------------------
POLICIES = ("random", "max_hours", "one_worker", "same_hours", "alternate", "on_cutoff")


def policy_actions(case, info, masks_a, masks_p, k):
    """Actions of the case's policy for step k of the run (0-based, counted over episode ends).  Returns
    (a int32 [E, n, 1], p int32 [E, width]).  An hour count the agent's mask forbids becomes NO-OP, and so does a rate
    the planner's mask forbids (mask_first_step; the tax masks are open on the first day of a period only).

    max_hours   everybody works 100 h             one_worker  the last agent works 100 h, everyone else 0
    same_hours  everybody works 37 h              alternate   agent i works 100 h when (i + k) is even, else 0
    on_cutoff   case["hours"][i] hours, doubled on odd steps
    planner     case["planner"]: "random", or one action index for every bracket (0 = NO-OP: the rates stay at index 0;
                21 = the top rate of the default discretisation)"""
    kind = case["policy"]
    masks_a = np.asarray(masks_a)
    E, n, H = masks_a.shape[0], info.n, info.num_hours
    rs = np.random.RandomState((int(case["seed"]) * 1000003 + int(k) * 7919 + POLICIES.index(kind)) % (2 ** 31))
    idx = np.arange(n)
    drawn = rs.randint(0, H + 1, size=(E, n))
    if kind == "random":
        h = drawn
    elif kind == "max_hours":
        h = np.full(n, H)
    elif kind == "one_worker":
        h = np.where(idx == n - 1, H, 0)
    elif kind == "same_hours":
        h = np.full(n, 37)
    elif kind == "alternate":
        h = np.where((idx + k) % 2 == 0, H, 0)
    elif kind == "on_cutoff":
        h = np.asarray(case["hours"]) * (1 + k % 2)
    else:
        raise ValueError(kind)
    h = np.broadcast_to(h, (E, n)).astype(np.int64)
    allowed = np.take_along_axis(masks_a.reshape(E, n, -1), h[:, :, None], 2)[:, :, 0] > 0.5
    a = np.where(allowed, h, 0).astype(np.int32)[:, :, None]
    planner = case.get("planner", "random")
    if info.n_sub_p == 0:
        return a, np.zeros((E, 1), np.int32)
    mp = np.asarray(masks_p).reshape(E, -1)
    D = info.sub_p_dim
    if info.multi_p:  # one column per bracket; the mask holds [NO-OP, D rates] per bracket
        want = rs.randint(0, D + 1, size=(E, info.n_sub_p)) if planner == "random" else np.full((E, info.n_sub_p), int(planner))
        ok = np.take_along_axis(mp.reshape(E, info.n_sub_p, D + 1), want[:, :, None], 2)[:, :, 0] > 0.5
    else:  # one index over [NO-OP, bracket 0's rates, bracket 1's rates, ...]
        assert planner == "random"
        want = rs.randint(0, 1 + info.n_sub_p * D, size=(E, 1))
        ok = np.take_along_axis(mp, want, 1) > 0.5
    return a, np.where(ok, want, 0).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------
# injected states
# ----------------------------------------------------------------------------------------------------------------
STATE_KINDS = ("escrow_on_tax_day", "last_coin_above_coin", "tiny_income", "coin_span", "coin_zero_labor_100",
               "one_agent_holds_all")


def injected_state(kind, info, base, rng):
    """A state of kind `kind` for one replica in the load_state format (LOAD_KEYS).  base: the replica's state right
    after a reset.  Every kind makes the first step a tax day and leaves the rates where the kind wants them (the
    first step is a NO-OP for the planner too)."""
    n = info.n
    s = {k: np.array(base[k]) for k in LOAD_KEYS}
    s["inv_coin"] = np.round(rng.uniform(5, 50, size=n), 3)
    s["esc_coin"] = np.zeros(n)
    s["tax_last_coin"] = np.round(s["inv_coin"] * rng.uniform(0.2, 0.9, size=n), 3)
    s["labor"] = np.round(rng.uniform(0, 100, size=n))
    s["production"] = np.round(rng.uniform(0, 300, size=n), 2)
    s["tax_cycle_pos"] = np.array(info.period, np.int32)
    top = max(len(info.disc) - 1, 0)  # (a fixed schedule has no rate indices: they stay 0)
    s["tax_rate_idx"] = rng.randint(0, top + 1, size=max(info.NB, 1))[: info.NB].astype(np.int32)
    if kind == "escrow_on_tax_day":  # coin 1 with 500 in escrow under a 100 % schedule: the levy takes the coin in hand
        s["inv_coin"], s["esc_coin"], s["tax_last_coin"] = np.ones(n), np.full(n, 500.0), np.zeros(n)
        s["tax_rate_idx"] = np.full(info.NB, top, np.int32)
    elif kind == "last_coin_above_coin":  # negative incomes without WealthRedistribution
        s["tax_last_coin"] = s["inv_coin"] + np.round(rng.uniform(1, 20, size=n), 3)
    elif kind == "tiny_income":  # 2^-21 = 4.8e-7 above last_coin (multiples of 0.5 keep the subtraction exact)
        s["tax_last_coin"] = np.arange(n) % 7 * 0.5
        s["inv_coin"] = s["tax_last_coin"] + 2.0 ** -21
    elif kind == "coin_span":  # ten decades in one replica
        s["inv_coin"] = 10.0 ** rng.uniform(-3, 7, size=n)
        s["inv_coin"][0], s["inv_coin"][n - 1] = 0.0009765625, 1.0e7
        s["tax_last_coin"] = s["inv_coin"] * 0.5
    elif kind == "coin_zero_labor_100":
        s["inv_coin"], s["tax_last_coin"], s["labor"] = np.zeros(n), np.zeros(n), np.full(n, 100.0)
    elif kind == "one_agent_holds_all":  # (income 0: the levy leaves the coin where it is)
        s["inv_coin"] = np.eye(n)[int(rng.randint(n))] * 7777.0
        s["tax_last_coin"] = s["inv_coin"].copy()
    else:
        raise ValueError(kind)
    return s


def injected_states(case, info, oracle):
    """One injected_state per replica (the kinds of the case in turn), built on the oracle's reset states."""
    rng = np.random.RandomState(case["seed"])
    return [injected_state(case["kinds"][e % len(case["kinds"])], info,
                           {k: np.array(oracle.t[k][e]) for k in LOAD_KEYS}, rng) for e in range(case["E"])]


def injected_actions(case, info, masks_a, masks_p, k):
    """Step k of an injected run: a NO-OP step first (a tax day on the untouched state), then the case's policy."""
    if k == 0:
        E = np.asarray(masks_a).shape[0]
        return np.zeros((E, info.n, 1), np.int32), np.zeros((E, info.n_sub_p if info.multi_p and info.n_sub_p else 1), np.int32)
    return policy_actions(case, info, masks_a, masks_p, k)


# ----------------------------------------------------------------------------------------------------------------
# cases (shared by tests/test_ose_states_cpu.py and tests/test_gpu_ose_states.py)
# ----------------------------------------------------------------------------------------------------------------
def _case(cfg, policy, steps, reach=(), E=8, seed=7, **kw):
    return dict(dict(cfg=cfg, policy=policy, steps=steps, reach=tuple(reach), E=E, seed=seed), **kw)


_WIDE = ("gini_sorted_branch", "second_lane_slot_used")
# name -> policy rollout: E replicas, `steps` steps through one episode end and its reset.  kernel: what the device
# test selects and asserts ("instance": the compile-time instance of BASELINE configs[4]'s family -- one-step-economy keeps
# its tax period in the family, so only period 1 stays on it; "generic", the default: aie_ose_step_kernel).
# reach: the conditions the run must come to (checked on the oracle alone, tests/test_ose_states_cpu.py)
ROLLOUTS = {
    # 100 h x skill <= 3 for three steps: incomes of up to 900 against a top cutoff of 510.3; tax_phase 1/3, 2/3, 1
    "c5_period3_max_hours": _case(ose_cfg(100, dict(C5_TAX, period=3), episode_length=9), "max_hours", 13,
                                  ("top_bracket_occupied", "cycle_pos_ge_3", "planner_mask_closed_mid_period") + _WIDE),
    "c5_period7_episode5": _case(ose_cfg(100, dict(C5_TAX, period=7), episode_length=5), "max_hours", 8,
                                 ("no_tax_day_in_episode", "cycle_pos_ge_3", "planner_mask_closed_mid_period") + _WIDE),
    # incomes 25 / 50 / 75 / 100 (and twice that): every one of them on a cutoff of [0, 25, 50, 75, 100]
    "on_cutoff_6": _case(ose_cfg(6, ON_CUTOFF_TAX, skills=[1.0, 1.25, 2.5, 2.0, 1.5, 3.0], episode_length=4), "on_cutoff", 9,
                         ("every_bracket_occupied", "top_bracket_occupied", "income_on_cutoff", "gini_pairwise_branch"),
                         hours=[25, 20, 10, 50, 50, 25]),
    # the equal split between the levy's two looks at coin: whoever worked less than the average "earned" a negative income
    "alternate_31_labor_tax_wealth": _case(ose_cfg(31, order=LTW, episode_length=6), "alternate", 13,
                                           ("income_negative", "gini_sorted_branch")),
    "alternate_31_wealth_labor_tax": _case(ose_cfg(31, order=WLT, episode_length=6), "alternate", 13,
                                           ("income_negative", "gini_sorted_branch")),
    "alternate_31_tax_labor_wealth": _case(ose_cfg(31, order=TLW, episode_length=6), "alternate", 13, ("gini_sorted_branch",)),
    "one_worker_30": _case(ose_cfg(30, episode_length=4, planner_reward_type="coin_eq_times_productivity"), "one_worker", 9,
                           ("rate_index_top", "gini_sorted_branch"), planner=21),
    "same_hours_64_top_rate": _case(ose_cfg(64, episode_length=4), "same_hours", 9, ("rate_index_top", "gini_sorted_branch"),
                                    planner=21),
    "same_hours_64_equal_skills": _case(ose_cfg(64, skills=[2.0] * 64, episode_length=4), "same_hours", 9,
                                        ("all_incomes_tied", "gini_sorted_branch"), planner=0),
    "fast_rng_65": _case(ose_cfg(65, episode_length=3), "random", 7, _WIDE, env_kw=dict(rng_mode="fast")),
    "auto_reset_65_period3": _case(ose_cfg(65, dict(C5_TAX, period=3), episode_length=5), "random", 12,
                                   ("cycle_pos_ge_3", "planner_mask_closed_mid_period") + _WIDE, auto_reset=True),
    "eta_one_29": _case(ose_cfg(29, episode_length=3, agent_reward_type="isoelastic_coin_minus_labor", isoelastic_eta=1.0,
                                planner_reward_type="coin_eq_times_productivity", mixing_weight_gini_vs_coin=0.3),
                        "random", 7, ("eta_is_one", "gini_pairwise_branch")),
    "eta_one_31": _case(ose_cfg(31, episode_length=3, agent_reward_type="isoelastic_coin_minus_labor", isoelastic_eta=1.0,
                                planner_reward_type="inv_income_weighted_utility"),
                        "random", 7, ("eta_is_one", "gini_sorted_branch")),
    "c5_instance": _case(ose_cfg(100, episode_length=4), "alternate", 9, ("rate_index_top",) + _WIDE, planner=21,
                         kernel="instance"),
    "c5_generic": _case(ose_cfg(100, episode_length=4), "alternate", 9, ("rate_index_top",) + _WIDE, planner=21,
                        kernel="generic_selected"),
}

# the agent-count sweep on the random policy, crossed with the bracket count (the flat vector is FA = NB + n + 6 floats,
# the planner's mask 22 * NB): every residue of FA mod 4, many rows per pass with a ragged tail (FA = 10, 11) and one
# row per pass with whole quads (FA = 140), MP = 352, both Gini branches, both lane slots -- asserted from the tensor
# shapes by test_ose_states_cpu.test_sweep_covers_the_row_store_shapes
SWEEP_TAX = {2: NB2_TAX, 7: C5_TAX, 16: NB16_TAX}
for _n, _nb in ((2, 2), (3, 2), (3, 7), (29, 16), (30, 2), (31, 16), (63, 7), (64, 16), (65, 2), (127, 7), (127, 16), (128, 2)):
    ROLLOUTS["sweep_n%d_nb%d" % (_n, _nb)] = _case(
        ose_cfg(_n, SWEEP_TAX[_nb], episode_length=3, planner_reward_type="coin_eq_times_productivity" if _n % 2 else
                "inv_income_weighted_utility"), "random", 7,
        (("gini_pairwise_branch",) if _n < 30 else ("gini_sorted_branch",)) + (("second_lane_slot_used",) if _n > 64 else ()),
        sweep=True)

# name -> injected run: replica e starts from injected_state(kinds[e % len(kinds)]) (load_state on both sides); a NO-OP
# step and two steps of the policy.  Only the oracle vouches for these states.
INJECTED = {
    # period 1 at an odd agent count: the record load skips last_income / last_marginal_rate, a range that ends mid-quad
    "wrapper_65_period1": _case(ose_cfg(65, episode_length=6), "alternate", 3,
                                ("tax_takes_all_coin", "income_negative", "income_tiny", "all_coin_zero", "rate_index_top")
                                + _WIDE, E=10, seed=3, planner=0, kinds=STATE_KINDS[:5]),
    "wrapper_128_period3": _case(ose_cfg(128, dict(C5_TAX, period=3), episode_length=6), "random", 3,
                                 ("one_agent_holds_all_coin", "tax_takes_all_coin", "income_negative", "cycle_pos_ge_3")
                                 + _WIDE, E=12, seed=5, kinds=STATE_KINDS),
    "fixed_rates_29": _case(ose_cfg(29, ON_CUTOFF_TAX, episode_length=6), "same_hours", 3,
                            ("tax_takes_all_coin", "income_negative", "income_tiny", "all_coin_zero",
                             "one_agent_holds_all_coin", "gini_pairwise_branch"), E=12, seed=9, kinds=STATE_KINDS),
}


def oracle_env(case):
    """(host env, OracleEnv, Info) of the case's E replicas, seeded and reset."""
    from helpers import make_env
    from oracle_lib import OracleEnv

    env = make_env(case["cfg"], n_envs=case["E"], **case.get("env_kw", {}))
    o = OracleEnv(env.build_config(), env.layout_planes())
    o.seed(case["seed"])
    o.reset()
    return env, o, Info(env)


def run_on_oracle(case, on_step=None):
    """Runs a ROLLOUTS or INJECTED case on the oracle alone; returns (Reach, shape_class).  on_step(k, a, p, oracle)
    sees every step ahead of the reset that may follow it."""
    env, o, info = oracle_env(case)
    reach, resets = Reach(), 0
    injected = "kinds" in case
    if injected:
        for e, s in enumerate(injected_states(case, info, o)):
            o.load_state(s, e=e)
    for k in range(case["steps"]):
        act = injected_actions if injected else policy_actions
        a, p = act(case, info, o.t["obs_a_action_mask"], o.t["obs_p_action_mask"], k)
        before = snapshot(o.t)
        o.step(a, p)
        reach.add(census(before, snapshot(o.t), a, info))
        if on_step is not None:
            on_step(k, a, p, o)
        if o.t["done"].all():
            o.reset(o.t["done"].copy())
            resets += 1
    assert not o.t["error_flags"].any()
    assert injected or resets >= 1, "the run does not cross an episode end"
    return reach, shape_class(o.t)
