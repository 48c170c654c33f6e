"""CPU guard of tests/test_gpu_rich_states.py, and the scripted policies side by side with the live reference.

Without a GPU and without the reference: every scenario of the GPU file (rich_states.ROLLOUTS / INJECTED) runs on the
oracle alone; its injected states satisfy the reference's invariants (before the first step and after every step), its
declared reach conditions (rich_states.census) all come out true, no replica raises an error flag, and the union over
the scenarios is the whole condition list.  That is what keeps the device tests from being vacuous: a condition, not a
measurement -- sizes and seeds were chosen so that the oracle alone meets it.

Reference-marked: the three policies drive the UNMODIFIED reference and the oracle side by side (the comparisons and
tolerances of test_oracle_vs_reference.test_oracle_tracks_live_reference) on the scalar-scaled configurations, through
an episode end, and the census of that very run must show what a policy reaches in the reference: every bracket
occupied on tax days, n trades in one step, a full bid book that later expires whole, ten houses, ties, trades at either
side's price and at prices 0 and max, a bid and an ask of one agent in one step (multi-action) ...

Conditions only INJECTION reaches -- for these the oracle is the only witness (no reference run gets there in a test's
time, or a mask-respecting policy never does):
  tax_income_on_cutoff, tax_tiny_income (an income of exactly 1.94 or of 4.8e-7 needs hand-placed coin);
  tax_nb_ge8_ragged / tax_nb_multiple_of_8, tax_annealed_cap_in_high_bracket (11 / 16 brackets and the annealed states
  are injected-only here; the reference-marked variants of test_oracle_vs_reference cover annealing in low brackets);
  cda_ask_book_full (every agent needs max_num_orders units of one resource and nobody may bid);
  cda_bid_refused_for_coin, cda_ask_refused_without_inventory in single-action mode (masks forbid them: `pushy` agents);
  all_moves_blocked, inventory_ge_256, coin_span_1e-3_1e5, one_agent_holds_all_coin, total_coin_zero.
"""
import functools

import numpy as np
import pytest

import rich_states as R
from helpers import compare_state, make_env


@functools.lru_cache(maxsize=None)
def _reach(name):
    if name in R.ROLLOUTS:
        return R.rollout_on_oracle(R.ROLLOUTS[name]).result()
    return R.injected_on_oracle(R.INJECTED[name]).result()  # (asserts the invariants of every state, every step)


@pytest.mark.parametrize("name", sorted(R.ROLLOUTS) + sorted(R.INJECTED))
def test_scenario_reaches_its_conditions_on_the_oracle(name):
    case = R.ROLLOUTS.get(name) or R.INJECTED[name]
    assert set(case["reach"]) <= set(R.CONDITIONS)
    got = _reach(name)
    missing = [k for k in case["reach"] if not got[k]]
    assert not missing, "%s does not reach %s" % (name, missing)


def test_scenarios_cover_every_condition():
    reached = set()
    for name in list(R.ROLLOUTS) + list(R.INJECTED):
        case = R.ROLLOUTS.get(name) or R.INJECTED[name]
        got = _reach(name)
        reached |= {k for k in case["reach"] if got[k]}
    assert not [k for k in R.CONDITIONS if k not in reached]


def test_invariants_reject_broken_states():
    """assert_invariants is not vacuous: a crossed book, a wrong escrow, an unsorted book, a house on a source block and
    two agents on one cell are each refused."""
    case = R.INJECTED["wrapper_4ag"]
    env, o = R.oracle_env(case["cfg"], 2, 1)
    info = R.Info(env)
    base = {k: np.array(o.t[k][0]) for k in R.INVARIANT_KEYS if k in o.t}
    good = R.rich_state(env, base, "book_ties", np.random.RandomState(2), info)
    R.assert_invariants(good, env, info)

    def broken(edit):
        s = {k: np.array(v) for k, v in good.items()}
        edit(s)
        with pytest.raises(AssertionError):
            R.assert_invariants(s, env, info)

    def cross(s):  # the best Stone bid of agent a jumps over an ask of another agent
        o0 = int(s["cda_bids"][0, 0])
        s["cda_bids"][0, 0] = (o0 & ~0xff00) | (10 << 8)
    broken(cross)
    broken(lambda s: s["esc_coin"].__setitem__(0, s["esc_coin"][0] + 1.0))
    nb = int(good["cda_n_bids"][0])
    assert R.ORD_PRICE(good["cda_bids"][0, 0]) != R.ORD_PRICE(good["cda_bids"][0, nb - 1])
    broken(lambda s: s["cda_bids"][0].__setitem__(slice(0, nb), s["cda_bids"][0, :nb][::-1].copy()))  # ascending bids
    broken(lambda s: s["cda_n_orders"].__setitem__((0, 0), s["cda_n_orders"][0, 0] + 1))
    broken(lambda s: s["house_owner"].__setitem__(tuple(np.argwhere((s["cell_flags"] & 6) > 0)[0]), 1))
    broken(lambda s: (s["loc_r"].__setitem__(1, s["loc_r"][0]), s["loc_c"].__setitem__(1, s["loc_c"][0])))


# ---- the policies in the live reference ------------------------------------------------------------------------
_POLICY_REACH = R._both("cda_n_trades_in_a_step", "cda_bid_book_full", "cda_expiry_in_full_book", "cda_trade_at_ask_price",
                        "cda_trade_at_bid_price", "cda_equal_price_other_lifetime", "cda_equal_price_equal_lifetime",
                        "cda_trade_at_max_price")
REFERENCE_CASES = {
    "builder_4ag": dict(cfg=R.scaled_cfg(4, episode_length=150), policy="builder", seed=5, steps=160,
                        reach=("houses_ge_10", "build_with_exact_resources")),
    "market_4ag": dict(cfg=R.scaled_cfg(4, episode_length=100), policy="market", seed=12, steps=110,
                       reach=_POLICY_REACH + R._both("cda_trade_at_price_0")),
    # a payment of 22 against cutoffs of [0, 1.21, 4.93, 10.53, 20.09, 25.51, 63.79]: one, two and three houses in a tax
    # period are incomes in brackets 4, 5 and 6, sales fill the lower ones -- every bracket within ONE replica
    "mix_10ag": dict(cfg=R.scaled_cfg(10, episode_length=200, payment=22, tax=dict(usd_scaling=8000.0)), policy="mix", seed=1,
                     steps=205, reach=("tax_every_bracket", "houses_ge_10")),
    "mix_4ag_multi_action_annealed": dict(
        cfg=R.scaled_cfg(4, episode_length=120, multi_action_mode_agents=True, tax=dict(tax_annealing_schedule=[-1, 0.35])),
        policy="mix", seed=3, steps=125,
        reach=R._both("cda_bid_and_ask_same_step", "cda_refused_at_quota") + ("houses_ge_10",)),
}


@pytest.mark.reference
@pytest.mark.parametrize("name", sorted(REFERENCE_CASES))
def test_oracle_tracks_live_reference_under_scripted_policies(name):
    from oracle_lib import OracleEnv
    from ref_extract import extract_obs, extract_state, rewards_array
    from test_oracle_vs_reference import _ref_env, check_metrics

    case = REFERENCE_CASES[name]
    cfg = case["cfg"]
    ref = _ref_env(cfg)
    host = make_env(cfg)
    o = OracleEnv(host.build_config(), host.layout_planes())
    np.random.seed(31 + case["seed"])
    st = np.random.get_state()
    o.t["mt"][0] = st[1]
    o.t["mt_pos"][0] = st[2]
    obs = ref.reset()
    o.reset()
    info, reach = R.Info(host), R.Reach()

    def check(where, obs, rew=None):
        compare_state({k: v[0] for k, v in o.t.items()}, extract_state(ref), where=where, f64_tol=1e-9)
        assert np.array_equal(o.t["mt"][0], np.random.get_state()[1]), where + ": MT19937 state"
        for k, want in extract_obs(ref, obs).items():
            got = o.t[k][0]
            if want.dtype.kind in "iu":
                assert np.array_equal(got, want), "%s: obs %s" % (where, k)
            else:
                np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6, err_msg="%s: obs %s" % (where, k))
        if rew is not None:
            got = np.concatenate([o.t["rewards_a"][0], o.t["rewards_p"][[0]]])
            np.testing.assert_allclose(got, rewards_array(ref, rew), rtol=0, atol=1e-5, err_msg=where)
        check_metrics(ref, host, o, where)

    check(name + " reset", obs)
    ended = 0
    for t in range(case["steps"]):
        a, p = R.policy_actions(case["policy"], host, o.t["obs_a_action_mask"], o.t["obs_p_action_mask"], case["seed"],
                                int(o.t["timestep"][0]), info)
        acts = {str(i): ([int(x) for x in a[0, i]] if info.multi else int(a[0, i, 0])) for i in range(info.n)}
        acts["p"] = [int(x) for x in p[0]] if info.multi_p else int(p[0, 0])
        before = R.snapshot(o.t)
        obs, rew, done, _ = ref.step(acts)
        o.step(a, p)
        check("%s step %d" % (name, t + 1), obs, rew)
        reach.add(R.census(before, R.snapshot(o.t), a, host, info))
        R.assert_invariants({k: v[0] for k, v in R.snapshot(o.t).items()}, host, info, "%s step %d" % (name, t + 1))
        assert bool(o.t["done"][0]) == bool(done["__all__"])
        if done["__all__"]:
            ended += 1
            obs = ref.reset()
            o.reset()
            check("%s reset after step %d" % (name, t + 1), obs)
    assert ended == 1
    got = reach.result()
    missing = [k for k in case["reach"] if not got[k]]
    assert not missing, "%s does not reach %s in the reference (reached: %s)" % (name, missing, reach.reached())
