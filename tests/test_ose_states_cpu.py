"""CPU guard of tests/test_gpu_ose_states.py, and the scripted one-step-economy policies side by side with the live
reference.

Without a GPU and without the reference: every case of the GPU file (ose_states.ROLLOUTS / INJECTED) runs on the oracle
alone; its declared reach conditions (ose_states.census) all come out true, no replica raises an error flag, the union
over the cases is the whole condition list, and the agent-count sweep covers every shape class of the kernel's row store
(read from the tensor shapes).  That is what keeps the device tests from being vacuous: a condition, not a measurement --
sizes, seeds and policies were chosen so that the oracle alone meets it.

Reference-marked: the scripted policies drive the UNMODIFIED reference and the oracle side by side (the comparisons and
tolerances of test_oracle_vs_reference.test_oracle_tracks_live_reference_one_step_economy) through an episode end, and the
census of the reference's own state must show what the case declares: incomes on every cutoff, negative incomes under
WealthRedistribution, a tax period of three steps, the top bracket, ties.

Conditions for which the oracle is the ONLY witness:
  * everything ose_states.INJECTED reaches by injection alone -- tax_takes_all_coin (coin in escrow does not exist in
    this scenario without it), income_tiny, all_coin_zero with labour, one_agent_holds_all_coin, and income_negative
    WITHOUT WealthRedistribution;
  * eta_is_one: the reference itself raises there (rewards.py:38, np.max(1, coin)), so log utility is the oracle's
    reading of the docstring above that line, log(max(1, coin));
  * the cases with more than 31 agents other than c5_period3_max_hours (the reference takes too long for a test).
"""
import functools

import numpy as np
import pytest

import ose_states as S
from helpers import compare_state, make_env


@functools.lru_cache(maxsize=None)
def _run(name):
    reach, shape = S.run_on_oracle(S.ROLLOUTS.get(name) or S.INJECTED[name])
    return reach.result(), shape


ALL_CASES = sorted(S.ROLLOUTS) + sorted(S.INJECTED)


@pytest.mark.parametrize("name", ALL_CASES)
def test_case_reaches_its_conditions_on_the_oracle(name):
    case = S.ROLLOUTS.get(name) or S.INJECTED[name]
    assert set(case["reach"]) <= set(S.CONDITIONS)
    assert 8 <= case["E"] <= 16 and case["steps"] <= 20
    got, _ = _run(name)
    missing = [k for k in case["reach"] if not got[k]]
    assert not missing, "%s does not reach %s" % (name, missing)


def test_cases_cover_every_condition():
    reached = set()
    for name in ALL_CASES:
        case = S.ROLLOUTS.get(name) or S.INJECTED[name]
        got, _ = _run(name)
        reached |= {k for k in case["reach"] if got[k]}
    assert not [k for k in S.CONDITIONS if k not in reached]


def test_order_tax_labor_wealth_reaches_no_negative_income():
    """The third component order is there for the order, not for the condition: the levy sees coin ahead of the equal
    split's effect on last_coin, and no income comes out negative."""
    got, _ = _run("alternate_31_tax_labor_wealth")
    assert not got["income_negative"]


def test_sweep_covers_the_row_store_shapes():
    """ose_store_rows writes a row of F floats with L4 = ceil(F / 4) lanes, 64 // L4 rows per pass, the last quad short
    when F % 4 != 0.  From the tensor shapes of the sweep's cells: all four residues of FA mod 4; many rows per pass with
    a ragged tail and one row per pass with whole quads; the widest planner mask (16 brackets x 22 = 352); both Gini
    branches at their edge; the lane edges 63 / 64 / 65 and 127 / 128."""
    shapes = [_run(name)[1] for name in sorted(S.ROLLOUTS) if S.ROLLOUTS[name].get("sweep")]
    assert 6 <= len(shapes)
    assert {s["FA"] % 4 for s in shapes} == {0, 1, 2, 3}
    assert any(s["FA_rows_per_pass"] >= 16 and s["FA"] % 4 != 0 for s in shapes)
    assert any(s["FA_rows_per_pass"] == 1 and s["FA"] % 4 == 0 for s in shapes)
    assert any(s["FA_rows_per_pass"] == 1 and s["FA"] % 4 != 0 for s in shapes)
    assert any(1 < s["FA_rows_per_pass"] < 16 for s in shapes)
    assert {s["MP"] for s in shapes} >= {44, 154, 352}
    assert {2, 3, 29, 30, 31, 63, 64, 65, 127, 128} <= {s["n"] for s in shapes}
    assert all(s["MA"] == 101 and s["MA_L4"] <= 64 and s["FA_L4"] <= 64 for s in shapes)
    # period 1 skips last_income / last_marginal_rate on the record load: odd agent counts end that range mid-quad, and
    # the same agent count occurs beside period 2
    period = {name: S.ROLLOUTS[name]["cfg"]["components"][1][1]["period"] for name in S.ROLLOUTS if S.ROLLOUTS[name].get("sweep")}
    by_n = {}
    for name, per in period.items():
        by_n.setdefault(S.ROLLOUTS[name]["cfg"]["n_agents"], set()).add(per)
    assert any(n % 2 == 1 and pers == {1, 2} for n, pers in by_n.items())


# ---- the census itself ------------------------------------------------------------------------------------------
def _hand_made(n=4, **info_kw):
    """A before / after pair of two replicas in which nothing happens: no tax day, coin 1 .. 2n, nobody works."""
    kw = dict(n=n, comps=["SimpleLabor", "PeriodicBracketTax"], NB=3, cut=np.array([0.0, 10.0, 20.0]), period=2, tax_model=0,
              disc=np.linspace(0, 1, 21), fixed=np.zeros(3), n_sub_p=3, sub_p_dim=21, multi_p=True, episode_length=10,
              isoelastic=False, eta=0.23, num_hours=100)
    kw.update(info_kw)
    info = S.Info(**kw)
    z = lambda dt=np.float64: np.zeros((2, n), dt)  # noqa: E731
    before = dict(inv_coin=np.arange(1.0, 2 * n + 1).reshape(2, n), esc_coin=z(), labor=z(), production=z(),
                  tax_cycle_pos=np.ones(2, np.int32), tax_rate_idx=np.zeros((2, 3), np.int32), tax_last_coin=z(),
                  tax_last_income=z(), tax_last_marginal_rate=z(), metrics_tax_days=np.zeros(2, np.int32),
                  metrics_tax_paid_sum=z(), timestep=np.zeros(2, np.int32), done=np.zeros(2, np.uint8))
    after = {k: v.copy() for k, v in before.items()}
    after["tax_cycle_pos"][:] = 2
    after["timestep"][:] = 1
    return before, after, info


def _flags(before, after, info):
    r = S.Reach()
    r.add(S.census(before, after, np.zeros((2, info.n, 1), np.int32), info))
    return {k for k, v in r.result().items() if v}


def _tax_day(b, a, inc, idx=0):
    """Replica 0 levies on incomes `inc` at rate index `idx`; everybody pays what is due."""
    b["tax_cycle_pos"][0], a["tax_cycle_pos"][0] = 2, 1
    a["tax_last_income"][0] = inc
    a["tax_rate_idx"][0] = idx
    a["metrics_tax_days"][0] = 1


def _edit_takes_all(b, a, info):
    _tax_day(b, a, [8.0, 1.0, 2.0, 3.0], idx=10)  # 50 %: 4 due, 1 in hand, 7 in escrow
    a["metrics_tax_paid_sum"][0] = S.taxes_due(info, info.rates(a)[:1], a["tax_last_income"][:1])[0]
    a["metrics_tax_paid_sum"][0, 0] = 1.0
    b["esc_coin"][0, 0] = a["esc_coin"][0, 0] = 7.0


# condition -> (keywords of the hand-made pair's Info, edit of the pair or of the Info, what the edit implies besides)
_SELF_TEST = {
    "top_bracket_occupied": ({}, lambda b, a, i: _tax_day(b, a, [25.0, 1.0, 2.0, 3.0]), ()),
    "every_bracket_occupied": ({}, lambda b, a, i: _tax_day(b, a, [25.0, 12.0, 2.0, 3.0]), ("top_bracket_occupied",)),
    "income_on_cutoff": ({}, lambda b, a, i: _tax_day(b, a, [10.0, 1.0, 2.0, 3.0]), ()),
    "income_negative": ({}, lambda b, a, i: _tax_day(b, a, [-1.0, 1.0, 2.0, 3.0]), ()),
    "income_tiny": ({}, lambda b, a, i: _tax_day(b, a, [5e-7, 1.0, 2.0, 3.0]), ()),
    "all_incomes_tied": ({}, lambda b, a, i: _tax_day(b, a, [3.0, 3.0, 3.0, 3.0]), ()),
    "all_coin_zero": ({}, lambda b, a, i: (a["inv_coin"].__setitem__(0, 0.0), a["labor"].__setitem__((0, 1), 100.0)), ()),
    "one_agent_holds_all_coin": ({}, lambda b, a, i: a["inv_coin"].__setitem__(1, [0.0, 0.0, 9.0, 0.0]), ()),
    "cycle_pos_ge_3": (dict(period=3), lambda b, a, i: a["tax_cycle_pos"].__setitem__(1, 3), ()),
    "no_tax_day_in_episode": (dict(period=12), lambda b, a, i: a["done"].__setitem__(1, 1), ()),
    "tax_takes_all_coin": ({}, _edit_takes_all, ()),
    "rate_index_top": ({}, lambda b, a, i: a["tax_rate_idx"].__setitem__((1, 2), 20), ()),
    "planner_mask_closed_mid_period": ({}, lambda b, a, i: setattr(i, "period", 3), ()),
    "eta_is_one": (dict(isoelastic=True), lambda b, a, i: setattr(i, "eta", 1.0), ()),
}


@pytest.mark.parametrize("cond", [c for c in S.CONDITIONS if c in _SELF_TEST])
def test_census_flips_exactly_the_condition_of_a_hand_made_pair(cond):
    """A hand-made before / after pair per condition: the unedited pair shows nothing but its Gini branch (and, where the
    condition needs a period longer than two steps, the planner's closed mask at position 2), the edited one exactly that
    condition more (and, for every_bracket_occupied, the top bracket it implies)."""
    assert _flags(*_hand_made()) == {"gini_pairwise_branch"}
    setup, edit, implied = _SELF_TEST[cond]
    b, a, info = _hand_made(**setup)
    quiet = _flags(b, a, info)
    assert cond not in quiet and quiet <= {"gini_pairwise_branch", "planner_mask_closed_mid_period"}
    edit(b, a, info)
    got = _flags(b, a, info)
    assert got == quiet | {cond} | set(implied), sorted(got)


def test_census_reads_the_lane_and_gini_classes_from_the_agent_count():
    shape_flags = {"gini_pairwise_branch", "gini_sorted_branch", "second_lane_slot_used"}
    assert set(S.CONDITIONS) == set(_SELF_TEST) | shape_flags
    want = {29: {"gini_pairwise_branch"}, 30: {"gini_sorted_branch"}, 64: {"gini_sorted_branch"},
            65: {"gini_sorted_branch", "second_lane_slot_used"}, 128: {"gini_sorted_branch", "second_lane_slot_used"}}
    for n, flags in want.items():
        assert _flags(*_hand_made(n=n)) == flags, n


# ---- what the host refuses --------------------------------------------------------------------------------------
def test_agent_counts_outside_2_to_128_are_refused_at_construction():
    with pytest.raises(AssertionError):
        make_env(S.ose_cfg(1, skills=[1.0])).build_config()
    with pytest.raises(ValueError, match="SimpleLabor supports at most 128 agents"):
        make_env(S.ose_cfg(129)).build_config()
    make_env(S.ose_cfg(128)).build_config()
    make_env(S.ose_cfg(2)).build_config()


def test_mask_rows_wider_than_a_wavefront_stores_are_refused():
    """ose_store_rows writes an agent's row with one 16-byte quad per lane: 64 lanes, 256 floats.  A mask row is
    [NO-OP, hours...], so SimpleLabor.num_labor_hours above 255 would leave the agents' masks unwritten without an error:
    aie_build_params (shared by the library and the oracle) refuses it.  The Python component pins 100 hours; the C
    interface is where another value can come from."""
    from oracle_lib import OracleEnv

    env = make_env(S.ose_cfg(5))
    for hours, ok in ((100, True), (255, True), (256, False), (543, False), (1000, False), (0, False)):
        cfg = env.build_config()
        cfg.labor_num_hours = hours
        if ok:
            o = OracleEnv(cfg, env.layout_planes())
            assert o.t["obs_a_action_mask"].shape == (1, 5, hours + 1)
            o.reset()
            o.step(np.full((1, 5, 1), hours, np.int32), np.zeros((1, 7), np.int32))  # (first step: masked, a NO-OP)
            o.step(np.full((1, 5, 1), hours, np.int32), np.zeros((1, 7), np.int32))
            assert (o.t["labor"] == hours).all() and (o.t["obs_a_action_mask"] == 1).all() and not o.t["error_flags"].any()
        else:
            with pytest.raises(ValueError, match="num_labor_hours out of range"):
                OracleEnv(cfg, env.layout_planes())


# ---- the policies in the live reference -------------------------------------------------------------------------
REFERENCE_CASES = sorted(name for name, c in S.ROLLOUTS.items()
                         if c["cfg"]["n_agents"] <= 31 and c["cfg"].get("isoelastic_eta") != 1.0) + ["c5_period3_max_hours"]


def _reference_pair(case):
    """(reference env, host env, oracle, Info) of one replica; the reference takes its skills as a plain attribute its
    reset reads (its constructor estimates them from the global stream)."""
    from oracle_lib import OracleEnv
    from test_oracle_vs_reference import _ref_env

    cfg = case["cfg"]
    ref_cfg = dict(cfg, components=[[name, {k: v for k, v in kw.items() if k != "skills"}] for name, kw in cfg["components"]])
    np.random.seed(77)
    ref = _ref_env(ref_cfg)
    skills = [kw["skills"] for name, kw in cfg["components"] if name == "SimpleLabor"][0]
    ref.get_component("SimpleLabor").skills = np.asarray(skills, np.float64)
    host = make_env(cfg)
    o = OracleEnv(host.build_config(), host.layout_planes())
    return ref, host, o, S.Info(host)


@pytest.mark.reference
@pytest.mark.parametrize("name", REFERENCE_CASES)
def test_oracle_tracks_live_reference_under_scripted_one_step_economy_policies(name):
    from ref_extract import extract_obs, extract_state, rewards_array
    from test_oracle_vs_reference import check_metrics

    case = dict(S.ROLLOUTS[name])
    steps = 10 if name == "c5_period3_max_hours" else case["steps"]
    ref, host, o, info = _reference_pair(case)
    np.random.seed(5)
    st = np.random.get_state()
    o.t["mt"][0] = st[1]
    o.t["mt_pos"][0] = st[2]
    obs = ref.reset()
    o.reset()
    reach = S.Reach()

    def check(where, obs, rew=None):
        compare_state({k: v[0] for k, v in o.t.items()}, extract_state(ref), where=where, f64_tol=1e-9)
        assert np.array_equal(o.t["mt"][0], np.random.get_state()[1]), where + ": MT19937 state"
        for k, want in extract_obs(ref, obs).items():
            np.testing.assert_allclose(o.t[k][0], want, rtol=2e-6, atol=2e-6, err_msg="%s: obs %s" % (where, k))
        if rew is not None:
            got = np.concatenate([o.t["rewards_a"][0], o.t["rewards_p"][[0]]])
            np.testing.assert_allclose(got, rewards_array(ref, rew), rtol=2e-7, atol=1e-5, err_msg=where)
        check_metrics(ref, host, o, where)

    def ref_snapshot(done):
        """The census' fields from the reference's own state (the two episode accumulators and `done` have no field
        there: the oracle's, which check_metrics holds to the reference's metrics)."""
        s = S.snapshot(o.t)
        for k, v in extract_state(ref).items():
            if k in s:
                s[k] = np.asarray(v)[None].astype(s[k].dtype)
        s["done"] = np.array([int(done)], np.uint8)
        return s

    check(name + " reset", obs)
    ended = 0
    for k in range(steps):
        a, p = S.policy_actions(case, info, o.t["obs_a_action_mask"], o.t["obs_p_action_mask"], k)
        acts = {str(i): int(a[0, i, 0]) for i in range(info.n)}
        if info.n_sub_p:
            acts["p"] = [int(x) for x in p[0]] if info.multi_p else int(p[0, 0])
        before = ref_snapshot(False)
        obs, rew, done, _ = ref.step(acts)
        o.step(a, p)
        check("%s step %d" % (name, k + 1), obs, rew)
        reach.add(S.census(before, ref_snapshot(done["__all__"]), a, info))
        assert bool(o.t["done"][0]) == bool(done["__all__"])
        if done["__all__"]:
            ended += 1
            obs = ref.reset()
            o.reset()
            check("%s reset after step %d" % (name, k + 1), obs)
    assert ended >= 1
    got = reach.result()
    missing = [c for c in case["reach"] if not got[c]]
    assert not missing, "%s does not reach %s in the reference (reached: %s)" % (name, missing, reach.reached())
