"""The flat observation vectors updated in place (csrc/aie_gtb_observe.h: update_flat_observations): a whole step whose
tensors still show the previous step writes only what the step changed -- time, world scalars, marginal rate and tax
calendar always, a histogram column when the auction touched it, the tax block's slow entries through the full writer on
the two steps of a period that change them.  Everything here compares the observation tensors, rewards and done with the
CPU oracle (or with a twin that takes the full path) after EVERY step, bit for bit: an entry the in-place path forgets
keeps the previous step's value, which no tolerance would notice for long."""

import numpy as np
import pytest

import rich_states as R
from helpers import C2, dev_library, dev_switches, make_env, oracle_host_pre_reset

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLAT = ("obs_a_flat", "obs_p_flat", "obs_p_agents")


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def _same(got, want, where):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (where, got.dtype, want.dtype, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    if bad.any():
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print("%s: %d of %d entries differ, max |diff| %g, first at %s" % (
            where, int(bad.sum()), bad.size, float(np.nanmax(diff)), tuple(int(i[0]) for i in np.nonzero(bad))))
    assert not bad.any(), where


def _outputs(be, oracle, where, sl=None, rewards=None):
    """obs_*, rewards_* and done of the replicas `sl` against the oracle's, bit for bit (`rewards`: the oracle's
    rewards / done of the terminal step, where an auto-reset has since restarted it)."""
    sl = slice(None) if sl is None else sl
    for k, v in be.tensors.items():
        if k.startswith("obs_"):
            _same(v[sl].cpu().numpy(), oracle.t[k][sl], "%s: %s" % (where, k))
        elif k.startswith("rewards") or k == "done":
            want = oracle.t[k] if rewards is None else rewards[k]
            _same(v[sl].cpu().numpy(), want[sl], "%s: %s" % (where, k))


def _pair(cfg, E, seed, kernel=None, **env_kw):
    from oracle_lib import OracleEnv

    env = make_env(cfg, n_envs=E, device=DEV, **env_kw)
    be = env.backend
    if kernel == "generic":
        assert be.lib.aie_select_step_kernel(be.handle, 1) == 0  # AIE_KERNEL_GENERIC
    env.seed(seed)
    env.reset()
    oracle = OracleEnv(env.build_config(), env.layout_planes())
    oracle.seed(seed)
    oracle_host_pre_reset(env, oracle)
    oracle.reset()
    inst = be.lib.aie_step_kernel_instance(be.handle)
    if kernel == "instance":
        assert inst >= 0, "no compile-time instance selected"
    elif kernel == "generic":
        assert inst == -1
    return env, oracle, R.Info(env)


def _step_both(env, oracle, a, p):
    import torch

    env.backend.step(torch.as_tensor(a, device=DEV), torch.as_tensor(p, device=DEV))
    oracle.step(a, p)


def _churn_cfg(n, orders=2):
    """Short-lived orders on few prices (the market policy): creations, fills and expiries of several orders at one
    price in one step.  orders == 5 keeps C2 / C3 in their instances' families."""
    if n <= 10:
        return R.scaled_cfg(n, episode_length=60, period=20, cda=dict(order_duration=3, max_num_orders=orders))
    cfg = R._big_cfg(n, orders)
    cfg["components"] = [[k, dict(v, order_duration=3) if k == "ContinuousDoubleAuction" else v] for k, v in cfg["components"]]
    return cfg


def test_tax_period_boundaries_with_auto_reset():
    """C2's instance, tax period 5, episodes of 23 steps (they end inside a period), two of them under auto-reset: first
    days, tax days, the days after, and the reset's full rewrite in between."""
    comps = [["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 5}], ["Gather", {}], ["PeriodicBracketTax", {"period": 5}]]
    env, oracle, info = _pair(dict(C2, components=comps, episode_length=23), 16, 3, kernel="instance")
    be = env.backend
    be.set_auto_reset(True)
    _outputs(be, oracle, "after reset")
    ends = tax_days = 0
    for t in range(50):
        a, p = R.policy_actions("mix", env, oracle.t["obs_a_action_mask"], oracle.t["obs_p_action_mask"], 3,
                                int(oracle.t["timestep"][0]), info)
        days = oracle.t["metrics_tax_days"].copy()
        _step_both(env, oracle, a, p)
        tax_days += int((oracle.t["metrics_tax_days"] > days).any())
        term = {k: oracle.t[k].copy() for k in oracle.t if k.startswith("rewards") or k == "done"}
        if term["done"].any():
            assert term["done"].all()
            ends += 1
            oracle.reset(term["done"].copy())
        _outputs(be, oracle, "step %d" % (t + 1), rewards=term)
    assert ends == 2 and tax_days >= 8
    assert int(be.tensors["error_flags"].abs().sum()) == 0


@pytest.mark.parametrize("n,orders,kernel", [(4, 2, None), (10, 2, None), (4, 5, "instance"), (10, 5, "instance"), (33, 2, "generic")])
def test_book_churn(n, orders, kernel):
    """The market policy on orders that live three steps.  33 agents with two orders each: books of 66 slots per side
    (the full-featured kernel's LDS books), more (column, agent) items than lanes."""
    E = 16 if n <= 10 else 8
    env, oracle, info = _pair(_churn_cfg(n, orders), E, 7, kernel=kernel)
    be = env.backend
    changed = {k: 0 for k in ("cda_ask_hist", "cda_bid_hist")}
    for t in range(45):
        a, p = R.policy_actions("market", env, oracle.t["obs_a_action_mask"], oracle.t["obs_p_action_mask"], 7, t, info)
        before = {k: oracle.t[k].copy() for k in changed}
        _step_both(env, oracle, a, p)
        for k in changed:
            changed[k] += int((before[k] != oracle.t[k]).any())
        _outputs(be, oracle, "n=%d step %d" % (n, t + 1))
    assert min(changed.values()) >= 10, changed  # (the books did churn)
    assert float(oracle.t["cda_price_history"].sum()) > 0  # (and orders were filled)
    assert int(be.tensors["error_flags"].abs().sum()) == 0


@pytest.mark.parametrize("dense_log", [False, True])
def test_two_agents_on_7x9(dense_log):
    """The smallest n, fragment lengths that are no multiples of 4; the generic kernel, and aie_step_kernel_log with its
    one dense-logged replica."""
    cfg = dict(scenario_name="uniform/simple_wood_and_stone", n_agents=2, world_size=[7, 9], episode_length=20,
               components=[["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 2, "order_duration": 3}],
                           ["Gather", {}], ["PeriodicBracketTax", {"period": 7}]],
               starting_agent_coin=20, starting_wood_coverage=0.15, starting_stone_coverage=0.15, wood_regen_weight=0.3,
               stone_regen_weight=0.3, mobile_agent_observation_range=2)
    if dense_log:
        cfg["dense_log_frequency"] = 1
    env, oracle, info = _pair(cfg, 8, 5, kernel=None if dense_log else "generic")
    be = env.backend
    assert ("log_events" in be.tensors) == dense_log
    for t in range(30):
        a, p = be.sample_random_actions(seed=11)
        a, p = a.cpu().numpy(), p.cpu().numpy()
        _step_both(env, oracle, a, p)
        _outputs(be, oracle, "step %d" % (t + 1))
        if oracle.t["done"].all():
            env.reset(be.tensors["done"])
            oracle_host_pre_reset(env, oracle)
            oracle.reset(oracle.t["done"].copy())
            _outputs(be, oracle, "step %d and reset" % (t + 1))
    assert int(be.tensors["error_flags"].abs().sum()) == 0


def test_dephased_masked_resets():
    """16 replicas, restarted in blocks of 4 every 5 steps: reset and stepping replicas share 128-byte lines of the
    env-major tensors (obs_a_time, obs_p_time, the ends of neighbouring rows)."""
    import torch

    env, oracle, info = _pair(dict(C2, episode_length=200), 16, 9, kernel="instance")
    be = env.backend
    for t in range(40):
        a, p = be.sample_random_actions(seed=21)
        _step_both(env, oracle, a.cpu().numpy(), p.cpu().numpy())
        _outputs(be, oracle, "step %d" % (t + 1))
        if t % 5 == 4:
            blk = (t // 5) % 4
            mask = np.zeros(16, np.uint8)
            mask[4 * blk: 4 * blk + 4] = 1
            env.reset(torch.as_tensor(mask, device=DEV))
            oracle.reset(mask)
            _outputs(be, oracle, "step %d and reset of block %d" % (t + 1, blk))
    assert len(set(oracle.t["timestep"].tolist())) == 4  # (four phases)


def _nan_fill(be):
    for k in FLAT:
        be.tensors[k].fill_(float("nan"))


def test_invalidation_rewrites_in_full_and_nothing_else_does():
    env, oracle, info = _pair(dict(C2), 8, 13, kernel="instance")
    be = env.backend

    def step(seed):
        a, p = be.sample_random_actions(seed=seed)
        _step_both(env, oracle, a.cpu().numpy(), p.cpu().numpy())

    for t in range(3):
        step(31)
    _outputs(be, oracle, "before")
    subset = [1, 4, 6]
    others = [e for e in range(8) if e not in subset]
    _nan_fill(be)
    be.invalidate_observations(subset)
    step(32)
    _outputs(be, oracle, "invalidated replicas", sl=subset)
    flat = be.tensors["obs_a_flat"].cpu().numpy()
    assert not np.isnan(flat[subset]).any()
    # the others went down the in-place path: the static block (Build: payment, skill -- the vector's first two entries)
    # still shows the fill; what a step always writes (time) does not
    assert np.isnan(flat[others][:, :, :2]).all()
    assert not np.isnan(be.tensors["obs_a_time"].cpu().numpy()).any()
    assert np.isnan(be.tensors["obs_p_flat"].cpu().numpy()[others]).any()
    assert np.isnan(be.tensors["obs_p_agents"].cpu().numpy()[others]).any()
    for k in FLAT:
        got = be.tensors[k].cpu().numpy()[others]
        keep = ~np.isnan(got)
        assert keep.any(), k  # (what the in-place path did write is right)
        assert np.array_equal(_bits(got)[keep], _bits(oracle.t[k][others])[keep]), k
    be.invalidate_observations()
    step(33)
    _outputs(be, oracle, "all invalidated")
    # aie_upload of a record field invalidates by itself (the same values: the state does not change)
    _nan_fill(be)
    be.upload("cda_ask_hist", be.download("cda_ask_hist"))
    step(34)
    _outputs(be, oracle, "after aie_upload")
    for k in FLAT:
        assert not np.isnan(be.tensors[k].cpu().numpy()).any(), k


def _market_actions(env, be, seed, t, info):
    return R.policy_actions("market", env, be.tensors["obs_a_action_mask"].cpu().numpy(),
                            be.tensors["obs_p_action_mask"].cpu().numpy(), seed, t, info)


def test_development_switch_equals_the_in_place_path():
    """-DAIE_DEV build: the switch AIE_DEV_FLAT_FULL rewrites the flat vectors in full on every step; its twin does not."""
    import torch

    with dev_library():
        envs = [make_env(_churn_cfg(4, 5), n_envs=16, device=DEV) for _ in range(2)]
        for env in envs:
            env.seed(15)
            env.reset()
    full, inc = envs[0].backend, envs[1].backend
    assert full.lib.aie_dev_set_skip_mask(full.handle, dev_switches()["AIE_DEV_FLAT_FULL"]) == 0
    info = R.Info(envs[0])
    for t in range(60):
        a, p = _market_actions(envs[1], inc, 15, t, info)
        for be in (full, inc):
            be.step(torch.as_tensor(a, device=DEV), torch.as_tensor(p, device=DEV))
        bad = [k for k in inc.tensors if not torch.equal(full.tensors[k], inc.tensors[k])]
        assert not bad, "step %d: %s differ" % (t + 1, bad)
    assert float(inc.tensors["cda_price_history"].sum()) > 0


def test_partial_launches_stay_on_the_full_path():
    """A scenario with a compute_reward hook steps through aie_step_range launches (full rewrites); its hook is the
    identity, so it has to show what the plain environment's in-place steps show."""
    import torch

    from test_user_scenario import _kwargs, _subclass

    cfg = _churn_cfg(4, 5)
    plain = make_env(cfg, n_envs=16, device=DEV)
    hooked = _subclass(cfg["scenario_name"], "FlatInPlaceIdentity", compute_reward=lambda self, t, rew: None)(
        **_kwargs(cfg, n_envs=16, device=DEV))
    assert hooked.scenario_hooks == ("compute_reward",)
    for env in (plain, hooked):
        env.seed(17)
        env.reset()
    info = R.Info(plain)
    for t in range(45):
        a, p = _market_actions(plain, plain.backend, 17, t, info)
        for env in (plain, hooked):
            env.step({"a": torch.as_tensor(a, device=DEV), "p": torch.as_tensor(p, device=DEV)})
        for k, v in plain.backend.tensors.items():
            if k.startswith("obs_") or k.startswith("rewards") or k == "done":
                assert torch.equal(v, hooked.backend.tensors[k]), "step %d: %s" % (t + 1, k)
    assert float(plain.backend.tensors["cda_price_history"].sum()) > 0


def test_annealed_rates_on_the_first_step_of_an_episode():
    """tax_annealing_schedule: the reset latches the completions count that caps the rates BEHIND its own observations,
    so the episode's first step shows other curr_rates than the reset did -- without a tax day in between."""
    rates = [0.257, 0.584, 0.79, 0.825, 0.94]
    comps = [["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 5}], ["Gather", {}],
             ["PeriodicBracketTax", dict(period=7, tax_model="fixed-bracket-rates", n_brackets=5, bracket_spacing="linear",
                                         top_bracket_cutoff=20.0, fixed_bracket_rates=rates, tax_annealing_schedule=[1, 0.6])]]
    env, oracle, info = _pair(dict(C2, components=comps, episode_length=12), 8, 3)
    be = env.backend
    lo = 2 + 10 * info.P + 2 + 1  # curr_rates in an agent's vector: behind Build (2), the auction (10 P + 2) and Gather (1)
    moved, at_reset = 0, None
    for t in range(40):
        a, p = be.sample_random_actions(seed=17)
        _step_both(env, oracle, a.cpu().numpy(), p.cpu().numpy())
        _outputs(be, oracle, "step %d" % (t + 1))
        if at_reset is not None:  # the first step of an episode
            moved += int((at_reset != oracle.t["obs_a_flat"][:, :, lo: lo + 5]).any())
            at_reset = None
        if oracle.t["done"].all():
            env.reset(be.tensors["done"])
            oracle.reset(oracle.t["done"].copy())
            _outputs(be, oracle, "step %d and reset" % (t + 1))
            at_reset = oracle.t["obs_a_flat"][:, :, lo: lo + 5].copy()
    assert moved >= 2, moved
