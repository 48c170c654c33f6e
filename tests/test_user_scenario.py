"""User-registered SCENARIOS with hooks of their own: scenario_step, generate_observations, compute_reward,
additional_reset_steps and scenario_metrics, the reference's scenario contract (F/base/base_env.py:1037-1141; call sites
:903-911, :1005-1011, :644-663) over the batch.  Five toy scenarios, written once against the reference's scenario classes
(tools/gen_golden_scenario.py, which produced tests/golden/scenario/*.npz by running the UNMODIFIED reference with them
registered) and once against this package's (below): state after every step, the generator's state, rewards, done,
resets and the observations -- the additional keys and, after a hook's map edit, the maps and masks -- must equal the
reference's.  Underneath: aie_step_range's split end of a step (AIE_STEP_REGEN / EMIT / CLOSE) must be bit-identical to
AIE_STEP_TAIL when nothing runs in between.

On a tree without the hooks the fixture tests fail at the first hooked step (the hooks are never called: the map, the
rewards or the first baseline differ, and toy (d)'s generator advances where the reference's does not)."""
import glob
import json
import os
import zlib

import numpy as np
import pytest

from helpers import C2, GOLDEN, compare_state, make_env, state_from_golden

OBS_TOL = 2e-6  # the project's bars for host-hook fixtures (tests/test_acting_component.py, tests/test_batched_component.py)
REW_TOL = 1e-5
SCENARIO = os.path.join(GOLDEN, "scenario")
TOY = {"a": "scenario_a_drought_4ag", "b": "scenario_b_toil_4ag", "c": "scenario_c_grant_4ag", "d": "scenario_d_refill_4ag",
       "e": "scenario_e_drought_uniform_tithe_10ag"}


def scenario_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(SCENARIO, "*.npz")))


def load_scenario(name):
    with np.load(os.path.join(SCENARIO, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg_json"]))
    g["cfg"]["_construction_seed"] = int(g["construction_seed"])
    g["flat"] = json.loads(str(g["flat_json"]))
    return g


@pytest.fixture(autouse=True)
def _registries_as_found():
    """tests/test_cabi_symbols.py pins the entries of both registries: the classes this file registers leave them again
    with the test that registered them."""
    from ai_economist_amd import foundation

    saved = [(reg, list(reg._names), dict(reg._by_lower)) for reg in (foundation.scenarios, foundation.components)]
    yield
    for reg, names, by_lower in saved:
        reg._names[:] = names
        reg._by_lower.clear()
        reg._by_lower.update(by_lower)


def register_scenarios():
    """The toys of tools/gen_golden_scenario.py as batched torch code."""
    import torch

    from ai_economist_amd import foundation
    from ai_economist_amd.foundation.scenarios.dynamic_layout import Uniform
    from ai_economist_amd.foundation.scenarios.layout_from_file import LayoutFromFile
    from test_acting_component import register_toys

    register_toys()  # (Tithe, toy (e))
    if foundation.scenarios.has("toy_drought/simple_wood_and_stone"):
        return

    class DroughtHooks:
        dries = "wood"

        def scenario_step(self, t):
            stays = (t["timestep"] % 4 != 0)
            m = t[self.dries]
            upper = m[:, : m.shape[1] // 2]
            upper.mul_(stays.to(upper.dtype)[:, None, None])

        def generate_observations(self, t):
            wood, stone = t["wood"].double(), t["stone"].double()
            E, n = t["inv_coin"].shape
            half = wood.shape[1] // 2
            w_up, w_lo = wood[:, :half].sum((1, 2)), wood[:, half:].sum((1, 2))
            s_up, s_lo = stone[:, :half].sum((1, 2)), stone[:, half:].sum((1, 2))
            wood_left = (w_up + w_lo) * 0.01
            phase = (t["timestep"] % 4).double() / 4.0
            stones = (s_up + s_lo) * 0.01
            patch = torch.stack([torch.stack([w_up, w_lo], -1), torch.stack([s_up, s_lo], -1)], -2)  # [E, 2, 2]

            def per_agent(x):
                return x[:, None].expand(E, n)

            return {"a": {"wood_left": per_agent(wood_left),
                          "season": torch.stack([per_agent(phase), per_agent(stones), t["inv_coin"] * 0.5], -1),
                          "patch": patch[:, None].expand(E, n, 2, 2)},
                    "p": {"wood_left": wood_left, "season": torch.stack([phase, stones, w_lo * 0.01], -1), "patch": patch}}

    @foundation.scenarios.add
    class ToyDrought(DroughtHooks, LayoutFromFile):
        name = "toy_drought/simple_wood_and_stone"

    @foundation.scenarios.add
    class ToyDroughtUniform(DroughtHooks, Uniform):
        name = "toy_drought_uniform/simple_wood_and_stone"
        dries = "stone"

    @foundation.scenarios.add
    class ToyToil(LayoutFromFile):
        name = "toy_toil/simple_wood_and_stone"

        def compute_reward(self, t, rew):  # (replacements; ToyToilInPlace below edits in place)
            a = rew["a"].double() - 0.05 * t["labor"]
            return {"a": a.float(), "p": a.mean(1).float()}

    @foundation.scenarios.add
    class ToyGrant(LayoutFromFile):
        name = "toy_grant/simple_wood_and_stone"

        def additional_reset_steps(self, t, env_mask=None):
            coin = t["inv_coin"]
            coin[:, 0] += 5.0 if env_mask is None else 5.0 * (env_mask != 0).to(coin.dtype)
            return True

    @foundation.scenarios.add
    class ToyRefill(LayoutFromFile):
        name = "toy_refill/simple_wood_and_stone"
        builtin_regeneration = False

        def scenario_step(self, t):
            due = (t["timestep"] % 5 == 0)[:, None, None]
            flags = t["cell_flags"]  # (include/aie.h: 1 water, 2 Stone source block, 4 Wood source block)
            for res, bit in (("wood", 4), ("stone", 2)):
                m = t[res]
                m.copy_(torch.where(due & ((flags & bit) != 0) & (m < 1), torch.ones_like(m), m))

    @foundation.scenarios.add
    class ToyPlain(LayoutFromFile):  # registered, overrides nothing
        name = "toy_plain/simple_wood_and_stone"


def _subclass(base_name, cls_name, **members):
    """A scenario class derived from a registered one (not registered itself: constructed directly)."""
    from ai_economist_amd import foundation

    return type(cls_name, (foundation.scenarios.get(base_name),), members)


def _kwargs(cfg, **extra):
    kw = dict(cfg)
    kw.pop("_construction_seed", None)
    kw.pop("scenario_name")
    kw["components"] = [tuple(c) for c in kw["components"]]
    kw.update(extra)
    return kw


# ---------------------------------------------------------------- CPU

def test_all_five_scenario_fixtures_are_present():
    assert scenario_names() == sorted(TOY.values())
    for name in scenario_names():
        assert 20 * 1024 < os.path.getsize(os.path.join(SCENARIO, name + ".npz")) < 64 * 1024


def _fake_tensors(env, E=2):
    import torch

    H, W = env.world_size
    return {"wood": torch.zeros((E, H, W), dtype=torch.uint8), "stone": torch.ones((E, H, W), dtype=torch.uint8),
            "timestep": torch.zeros(E, dtype=torch.int32), "inv_coin": torch.zeros((E, env.n_agents), dtype=torch.float64)}


@pytest.mark.parametrize("name", sorted(TOY.values()))
def test_flat_key_tables_with_world_keys_equal_the_reference(name):
    """The sorted-key position and size of every flattened key, the scenario's own among them, and what stays a key of its
    own (more than one dimension per actor), against the reference's packager (F/base/base_env.py:561-589)."""
    register_scenarios()
    g = load_scenario(name)
    env = make_env(g["cfg"])
    extra = env.host_observation_values(_fake_tensors(env))
    tab = env.host_flat_keys(extra)
    for who in "ap":
        assert [(key, size) for key, _off, size, _sc in tab[who]] == [tuple(x) for x in g["flat"][who]["flat"]], who
        assert tab["sizes"][who] == g["ob_obs_%s_flat" % who].shape[-1]
        off = 0
        for _key, o, size, scalar in tab[who]:
            assert o == off and (size == 1 or not scalar)
            off += size
        assert sorted(tab["perm"][who]) == list(range(tab["sizes"][who]))
        multi = sorted(k for k, v in extra[who].items() if v.dim() > (3 if who == "a" else 2))
        assert multi == [k for k in g["flat"][who]["kept"] if k not in ("action_mask", "world-map", "world-idx_map")]
    if name in (TOY["a"], TOY["e"]):
        assert [k for k, _, _, _ in tab["a"]][-2:] == ["world-season", "world-wood_left"] and "world-patch" in extra["p"]
    else:
        assert not extra["a"] and not extra["p"]


def test_observation_key_collisions_and_planner_blocks_are_refused():
    import torch

    register_scenarios()
    cfg = load_scenario(TOY["a"])["cfg"]
    one = torch.zeros((2, 4))

    def build(result):
        return _subclass("layout_from_file/simple_wood_and_stone", "ToyKeys", generate_observations=lambda self, t: result)(**_kwargs(cfg))

    with pytest.raises(ValueError, match="world-inventory-Coin.*already taken"):
        build({"a": {"inventory-Coin": one}}).host_observation_values({})
    with pytest.raises(ValueError, match="world-map.*already taken"):
        build({"p": {"map": one[:, 0]}}).host_observation_values({})
    with pytest.raises(NotImplementedError, match="per-agent planner observation blocks"):
        build({"a": {}, "p0": {"x": one[:, 0]}}).host_observation_values({})
    with pytest.raises(ValueError, match="keyed 'a'"):
        build({"agents": {"x": one}}).host_observation_values({})
    ok = build({"a": {"x": one}, "p": {"y": one[:, 0]}}).host_observation_values({})
    assert sorted(ok["a"]) == ["world-x"] and sorted(ok["p"]) == ["world-y"]


def test_hooks_outside_gather_trade_build_and_with_dense_logs_are_refused():
    from helpers import covid_golden_names, load_covid_golden

    register_scenarios()
    hook = dict(scenario_step=lambda self, t: None)
    with pytest.raises(NotImplementedError, match="gather-trade-build scenarios only"):
        _subclass("one-step-economy", "ToyOse", **hook)(n_agents=4, world_size=[1, 1], episode_length=2, components=[("SimpleLabor", {})])
    covid = dict(load_covid_golden(covid_golden_names()[0])["cfg"])
    with pytest.raises(NotImplementedError, match="gather-trade-build scenarios only"):
        _subclass("CovidAndEconomySimulation", "ToyCovid", compute_reward=lambda self, t, rew: None)(**_kwargs(dict(covid, scenario_name="x")))
    with pytest.raises(NotImplementedError, match="gather-trade-build scenarios only"):
        _subclass("one-step-economy", "ToyOseNoRegen", builtin_regeneration=False)(
            n_agents=4, world_size=[1, 1], episode_length=2, components=[("SimpleLabor", {})])
    # the same classes without an override still build
    _subclass("one-step-economy", "ToyOsePlain")(n_agents=4, world_size=[1, 1], episode_length=2, components=[("SimpleLabor", {})])
    for name in TOY.values():
        with pytest.raises(NotImplementedError, match="dense logs"):
            make_env(load_scenario(name)["cfg"], dense_log_frequency=1)
    make_env(dict(load_scenario(TOY["c"])["cfg"], scenario_name="toy_plain/simple_wood_and_stone"), dense_log_frequency=1)


def test_subclass_without_overrides_is_its_parent():
    register_scenarios()
    cfg = load_scenario(TOY["b"])["cfg"]
    plain = make_env(dict(cfg, scenario_name="toy_plain/simple_wood_and_stone"), n_envs=5)
    parent = make_env(dict(cfg, scenario_name="layout_from_file/simple_wood_and_stone"), n_envs=5)
    assert bytes(plain.build_config()) == bytes(parent.build_config())
    assert plain.scenario_hooks == () and plain.step_plan() == [] and plain.planned_launches() == []
    assert parent.scenario_hooks == ()
    hooked = make_env(cfg, n_envs=5)
    assert bytes(hooked.build_config()) == bytes(parent.build_config())  # (hooks are host code: the device sees the parent)
    assert hooked.scenario_hooks == ("compute_reward",)


def test_launch_plan_per_override_set():
    """As few launches as the hooks allow (the tuples are aie_step_range's comp_lo, comp_hi, phases)."""
    from ai_economist_amd import _cabi

    register_scenarios()
    H, T, R, E, C = _cabi.STEP_HEAD, _cabi.STEP_TAIL, _cabi.STEP_REGEN, _cabi.STEP_EMIT, _cabi.STEP_CLOSE
    assert (H, T, R, E, C) == (1, 2, 64, 128, 256)
    plans = {k: make_env(load_scenario(TOY[k])["cfg"]) for k in TOY}
    assert plans["a"].planned_launches() == [(0, 3, H | R), (3, 3, E | C)]
    assert plans["a"].step_plan() == [("launch", 0, 3, H | R), ("scenario_step",), ("launch", 3, 3, E | C)]
    assert plans["b"].planned_launches() == [(0, 4, H | R | E), (4, 4, C)]
    assert plans["b"].step_plan()[1] == ("compute_reward",)
    assert plans["c"].planned_launches() == [(0, 4, H | T)]  # (a reset hook only: the step is one ranged launch)
    assert plans["d"].planned_launches() == [(0, 3, H), (3, 3, E | C)]  # (no REGEN anywhere)
    assert plans["e"].step_plan() == [("launch", 0, 1, H), ("component", "Tithe"), ("launch", 1, 2, R), ("scenario_step",),
                                      ("launch", 2, 2, E | C)]
    cfg = load_scenario(TOY["a"])["cfg"]
    noop, noop_r = (lambda self, t: None), (lambda self, t, rew: None)

    def plan(members, components=None):
        c = dict(cfg) if components is None else dict(cfg, components=components)
        return _subclass("layout_from_file/simple_wood_and_stone", "ToyPlan", **members)(**_kwargs(c)).planned_launches()

    assert plan(dict(scenario_step=noop, compute_reward=noop_r)) == [(0, 3, H | R), (3, 3, E), (3, 3, C)]
    assert plan(dict(builtin_regeneration=False, compute_reward=noop_r)) == [(0, 3, H), (3, 3, E), (3, 3, C)]
    assert plan(dict(builtin_regeneration=False)) == [(0, 3, H), (3, 3, E | C)]
    assert plan(dict(generate_observations=lambda self, t: {})) == [(0, 3, H | T)]
    # a host component listed last runs ahead of the regeneration, the scenario's own step behind it
    last = [["Build", {}], ["Gather", {}], ["Tithe", {}]]
    assert plan(dict(scenario_step=noop), last) == [(0, 2, H), (2, 2, R), (2, 2, E | C)]
    assert plan(dict(compute_reward=noop_r), last) == [(0, 2, H), (2, 2, R | E), (2, 2, C)]
    assert plan(dict(builtin_regeneration=False, scenario_step=noop), last) == [(0, 2, H), (2, 2, E | C)]
    first = [["Tithe", {}], ["Build", {}], ["Gather", {}]]
    assert plan(dict(compute_reward=noop_r), first) == [(0, 0, H), (0, 2, R | E), (2, 2, C)]
    assert plan({}, first) == [(0, 0, H), (0, 2, T)]  # (host components alone: as before)


# ---------------------------------------------------------------- GPU: the split end of a step

def _all_tensors(be, log):
    out = {k: v.detach().cpu().clone() for k, v in be.tensors.items()}
    out["reward_log"] = log.detach().cpu().clone()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rng_mode", ["numpy", "fast"])
def test_split_tail_is_bit_identical_to_the_whole_step(rng_mode):
    """aie_step; HEAD | TAIL; the components, then REGEN | EMIT | CLOSE in one launch; the components, then REGEN, EMIT
    and CLOSE in three: every tensor and the reward log equal, over an episode end, tax days and expiring orders."""
    import torch

    from ai_economist_amd import _cabi

    H, T, R, Em, C = _cabi.STEP_HEAD, _cabi.STEP_TAIL, _cabi.STEP_REGEN, _cabi.STEP_EMIT, _cabi.STEP_CLOSE
    comps = [["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 5, "order_duration": 6}], ["Gather", {}],
             ["PeriodicBracketTax", {"period": 9}]]
    cfg = dict(C2, components=comps, episode_length=28, resource_regen_prob=0.05)
    E, nb = 64, 4
    ways = {"aie_step": None, "tail": [(0, nb, H | T)], "one": [(0, nb, H), (nb, nb, R | Em | C)],
            "three": [(0, nb, H), (nb, nb, R), (nb, nb, Em), (nb, nb, C)],
            "joined": [(0, nb, H | R | Em), (nb, nb, C)]}
    envs, logs = {}, {}
    for w in ways:
        env = make_env(cfg, n_envs=E, device="cuda:0", rng_mode=rng_mode)
        env.seed(5)
        env.reset()
        envs[w], logs[w] = env, env.backend.set_reward_log(4)
    rng = np.random.RandomState(3)
    names_a, names_p = envs["tail"].action_subspace_names()
    A = 1 + sum(k for _, k in names_a)
    seen_done = seen_tax = 0
    for t in range(1, 37):
        a = torch.as_tensor(rng.randint(0, A, size=(E, 4)).astype(np.int32), device="cuda:0")
        p = torch.as_tensor(np.stack([rng.randint(0, k + 1, size=E) for _, k in names_p], 1).astype(np.int32), device="cuda:0")
        for w, launches in ways.items():
            be = envs[w].backend
            if launches is None:
                be.step(a, p)
            else:
                for lo, hi, ph in launches:
                    be.step_range(a, p, lo, hi, ph)
        want = _all_tensors(envs["aie_step"].backend, logs["aie_step"])
        for w in ways:
            got = _all_tensors(envs[w].backend, logs[w])
            assert sorted(got) == sorted(want)
            bad = [k for k in want if not torch.equal(got[k], want[k])]
            assert not bad, "%s, step %d, %s: %s differ" % (rng_mode, t, w, bad)
        seen_tax += int(want["tax_cycle_pos"][0] == 1 and t > 1)
        if bool(want["done"].all()):
            seen_done += 1
            for env in envs.values():
                env.reset()
    assert seen_done == 1 and seen_tax >= 3
    assert int(want["error_flags"].abs().sum()) == 0
    assert float(logs["aie_step"].abs().sum()) > 0


@pytest.mark.gpu
def test_step_range_validates_the_new_phases():
    from ai_economist_amd import _cabi

    H, T, O, R, Em, C = (_cabi.STEP_HEAD, _cabi.STEP_TAIL, _cabi.STEP_OBSERVE, _cabi.STEP_REGEN, _cabi.STEP_EMIT, _cabi.STEP_CLOSE)
    env = make_env(C2, n_envs=2, device="cuda:0")
    env.seed(1)
    env.reset()
    be = env.backend
    before = {k: v.clone() for k, v in be.tensors.items()}
    for lo, hi, ph, text in ((0, 0, R | T, "exclude TAIL and OBSERVE"), (0, 0, Em | O, "exclude TAIL and OBSERVE"),
                             (0, 0, C | O, "exclude TAIL and OBSERVE"), (0, 4, R | Em | C, "CLOSE takes no component range"),
                             (3, 4, C, "CLOSE takes no component range"), (4, 4, R | C, "REGEN | CLOSE without EMIT"),
                             (4, 4, H | C, "HEAD | CLOSE without EMIT"), (0, 4, Em, "EMIT with components or HEAD but without REGEN"),
                             (4, 4, H | Em, "EMIT with components or HEAD but without REGEN"), (0, 0, 512, "phases 512"),
                             (0, 0, 32, "phases 32")):
        with pytest.raises(ValueError, match="aie_step_range: .*%s" % text.replace("|", r"\|")) as err:
            be.step_range(None, None, lo, hi, ph)
        assert "phases %d" % ph in str(err.value)
    import torch

    torch.cuda.synchronize()
    assert all(torch.equal(before[k], v) for k, v in be.tensors.items())  # (a refused call launches nothing)


# ---------------------------------------------------------------- GPU: the fixtures, step by step

def _follow(name, on_step=None, on_env=None, **extra):
    """Steps a 3-replica environment through the fixture (the procedure of tests/test_acting_component.py: replicas 0
    and 2 take the fixture's actions, replica 1 others)."""
    from test_acting_component import _batch_actions, _obs_check, _replica

    register_scenarios()
    g = load_scenario(name)
    E = 3
    env = make_env(g["cfg"], n_envs=E, device="cuda:0", **extra)
    assert env.scenario_hooks
    be = env.backend
    be.set_rng_state(np.stack([g["pre_reset_mt"]] * E), np.full(E, int(g["pre_reset_pos"]), np.int32))
    obs = env.reset()
    if on_env is not None:
        on_env(env)
    for e in (0, 2):
        compare_state(_replica(be, e), state_from_golden(g, "s0_"), where="%s reset replica %d" % (name, e))
    obs_steps = list(g["obs_steps"])
    assert 0 in obs_steps
    _obs_check(obs, g, obs_steps.index(0), name + " reset obs", 2)
    resets = {int(t): i for i, t in enumerate(g["reset_at"])}
    assert resets
    for t in range(g["actions_a"].shape[0]):
        obs, rew, done, _ = env.step(_batch_actions(g, t, E, env))
        want = state_from_golden(g, "st_", t)
        for e in (0, 2):
            got = _replica(be, e)
            where = "%s step %d replica %d" % (name, t + 1, e)
            compare_state(got, want, where=where)
            assert zlib.crc32(got["mt"].tobytes()) == int(g["st_mt_crc"][t]), where + ": the generator's state"
            if g["host_a"].shape[-1]:
                assert np.array_equal(got["host_actions_a"], g["host_a"][t]), where
            r = np.concatenate([got["rewards_a"], got["rewards_p"][None]])
            print("%s: largest reward error %.3g" % (where, float(np.max(np.abs(r - g["rew"][t])))))
            np.testing.assert_allclose(r, g["rew"][t], rtol=2e-7, atol=REW_TOL, err_msg=where)
            assert np.array_equal(rew["a"][e].cpu().numpy(), got["rewards_a"]), where  # (env.step returns the same values)
            assert int(got["done"]) == int(g["done"][t]) == int(done["__all__"][e]), where
            assert int(got["error_flags"]) == 0, where
        if on_step is not None:
            on_step(env, t, g)
        if (t + 1) in obs_steps:
            _obs_check(obs, g, obs_steps.index(t + 1), "%s step %d" % (name, t + 1), 2)
        if (t + 1) in resets:
            obs = env.reset(be.tensors["done"])  # (replica 1 shares the clock: its episode ends with the others')
            compare_state(_replica(be, 0), state_from_golden(g, "rs_", resets[t + 1]), where="%s reset after step %d" % (name, t + 1))
    return env, g


@pytest.mark.gpu
@pytest.mark.parametrize("toy", sorted(TOY))
def test_toy_scenarios_match_the_reference_with_the_same_scenarios(toy):
    env, g = _follow(TOY[toy])
    assert env.planned_launches()  # (ranged launches: the full-featured kernel, whatever instance the configuration has)
    kept = [k for k in g if k.startswith("ob_")]
    if toy in "ae":  # the maps after the hook's edit (the full-rewrite path behind a REGEN-only launch), the additional keys
        assert "ob_obs_a_world-map" in kept and "ob_obs_p_world-idx_map" in kept and "ob_obs_p_world-patch" in kept
        assert any(int(s) % 4 == 0 and int(s) > 0 for s in g["obs_steps"])
    assert "ob_obs_a_action_mask" in kept and "ob_obs_a_flat" in kept


@pytest.mark.gpu
def test_unflattened_observations_carry_the_world_keys():
    from test_acting_component import _batch_actions

    register_scenarios()
    g = load_scenario(TOY["a"])
    env = make_env(g["cfg"], n_envs=3, device="cuda:0", flatten_observations=False)
    be = env.backend
    be.set_rng_state(np.stack([g["pre_reset_mt"]] * 3), np.full(3, int(g["pre_reset_pos"]), np.int32))
    env.reset()
    for t in range(4):
        obs, _, _, _ = env.step(_batch_actions(g, t, 3, env))
    k = list(g["obs_steps"]).index(4)
    for who in "ap":
        flat = g["ob_obs_%s_flat" % who][k]
        off = 0
        for key, size in g["flat"][who]["flat"]:
            if key.startswith("world-") and key != "time":
                got = obs[who][key][2].cpu().numpy().astype(np.float32)
                want = flat[..., off:off + size]
                np.testing.assert_allclose(got.reshape(want.shape), want, rtol=OBS_TOL, atol=OBS_TOL, err_msg=key)
            off += size
        assert "flat" not in obs[who] and tuple(obs[who]["world-patch"].shape[-2:]) == (2, 2)
        np.testing.assert_allclose(obs[who]["world-patch"][2].cpu().numpy(), g["ob_obs_%s_world-patch" % who][k], rtol=0, atol=0)


@pytest.mark.gpu
def test_reward_edit_reaches_the_reward_log():
    """Toy (b) with a reward log of 4 slots: the slot of every step holds the EDITED rewards and the done flag."""
    import torch

    log = {}

    def switch_on(env):
        log["log"] = env.backend.set_reward_log(4)

    def check(env, t, g):
        tt = env.backend.tensors
        filled = (int(tt["rew_log_slot"][0]) - 1) % 4  # (the field names the slot the NEXT step fills)
        assert filled == t % 4 and bool((tt["rew_log_slot"] == tt["rew_log_slot"][0]).all()), t
        slot = log["log"][filled]
        assert torch.equal(slot[:, :4], tt["rewards_a"]) and torch.equal(slot[:, 4], tt["rewards_p"]), t
        assert torch.equal(slot[:, 5], tt["done"].to(slot.dtype)), t
        np.testing.assert_allclose(slot[0].cpu().numpy()[:5], g["rew"][t], rtol=2e-7, atol=REW_TOL)
        log["big"] = log.get("big", 0) + int((0.05 * g["st_labor"][t]).max() >= 1e-2)

    env, g = _follow(TOY["b"], on_step=check, on_env=switch_on)
    assert log["big"] > g["rew"].shape[0] // 2  # the edit is three orders above the bar on most steps
    assert int(g["done"].sum()) >= 1


@pytest.mark.gpu
def test_in_place_reward_edit_equals_returned_replacements():
    import torch

    from test_acting_component import _batch_actions

    register_scenarios()
    g = load_scenario(TOY["b"])

    def in_place(self, t, rew):
        a = rew["a"].double() - 0.05 * t["labor"]
        rew["a"].copy_(a.float())
        rew["p"].copy_(a.mean(1).float())

    envs = [make_env(g["cfg"], n_envs=3, device="cuda:0"),
            _subclass("layout_from_file/simple_wood_and_stone", "ToyToilInPlace", compute_reward=in_place)(
                **_kwargs(g["cfg"], n_envs=3, device="cuda:0"))]
    for env in envs:
        env.seed(9)
        env.reset()
    for t in range(6):
        out = [env.step(_batch_actions(g, t, 3, env)) for env in envs]
        assert torch.equal(out[0][1]["a"], out[1][1]["a"]) and torch.equal(out[0][1]["p"], out[1][1]["p"])
    assert float(out[0][1]["a"].abs().sum()) > 0


@pytest.mark.gpu
def test_masked_reset_with_a_reset_hook_touches_only_its_rows():
    """Toy (c), the twin method of tests/test_batched_component.py: S resets a mask's replicas at step k, F all of them, N
    none; outside the mask S equals N -- state, observations, reward baseline (util) and tax snapshot (tax_last_coin) --
    inside it F, every tensor and every observation bit for bit."""
    import torch

    from test_batched_component import TWIN_E, _twin_actions, _twin_assert, _twin_masks, _twin_snapshot

    register_scenarios()
    cfg = load_scenario(TOY["c"])["cfg"]
    E, k = TWIN_E, 7  # (tax period 5, episode length 12: the middle of the second period)
    masks = _twin_masks(E)
    masks = {m: masks[m] for m in ("first", "alternate", "all_but_one", "none")}  # strict subsets (and the empty one)

    def build():
        env = make_env(cfg, n_envs=E, device="cuda:0")
        env.seed(17)
        return env

    S = {m: build() for m in masks}
    N, F = build(), build()
    envs = list(S.values()) + [N, F]
    snap = {id(env): _twin_snapshot(env, env.reset()) for env in envs}
    assert bool((snap[id(N)]["inv_coin"][:, 0] == cfg["starting_agent_coin"] + 5.0).all())
    assert bool((snap[id(N)]["tax_last_coin"][:, 0] == cfg["starting_agent_coin"]).all())  # (the snapshot was taken before the grant)
    rng = np.random.RandomState(1000 + k)

    def check(where):
        for m, rows in masks.items():
            s = snap[id(S[m])]
            assert "util" in s and "tax_last_coin" in s and any(x.startswith("obs") for x in s)
            _twin_assert(s, snap[id(N)], [e for e in range(E) if e not in rows], "%s: mask %s, outside vs no reset" % (where, m))
            _twin_assert(s, snap[id(F)], rows, "%s: mask %s, inside vs full reset" % (where, m))

    for t in range(1, 12 + 5 + 1):
        act = _twin_actions(N, rng, E)
        for env in envs:
            obs, _, _, _ = env.step(act)
            snap[id(env)] = _twin_snapshot(env, obs)
        check("step %d" % t)
        if t == k:
            for m, rows in masks.items():
                mask = torch.zeros(E, dtype=torch.uint8, device="cuda:0")
                mask[rows] = 1
                snap[id(S[m])] = _twin_snapshot(S[m], S[m].reset(mask))
            snap[id(F)] = _twin_snapshot(F, F.reset())
            check("reset at step %d" % t)
            continue
        reset_any = False
        for env in envs:
            done = env.backend.tensors["done"]
            if bool(done.any().item()):
                snap[id(env)] = _twin_snapshot(env, env.reset(done))
                reset_any = True
        if reset_any:
            check("reset(done) after step %d" % t)
    assert int(N.backend.tensors["completions"].min()) >= 1


@pytest.mark.gpu
def test_hooked_environments_are_refused_what_host_components_are():
    from ai_economist_amd import rollout

    register_scenarios()
    cfg = load_scenario(TOY["a"])["cfg"]
    env = make_env(cfg, n_envs=4, device="cuda:0")
    env.seed(3)
    env.reset()
    be = env.backend
    assert any("scenario hooks" in x for x in be.host_components)
    with pytest.raises(NotImplementedError, match="host components.*scenario hooks of ToyDrought"):
        rollout.GraphedStep(env, lambda t, a, p: None)
    with pytest.raises(NotImplementedError, match=r"Backend\.step: .*scenario hooks"):
        be.step(None, None)
    with pytest.raises(NotImplementedError, match=r"set_auto_reset\(True\).*scenario hooks"):
        be.set_auto_reset(True)
    a, p = be._action_buffers(0)
    with pytest.raises(NotImplementedError, match="step_sample_next.*scenario hooks"):
        be.step_sample_next(a, p, seed=1)
    saez = [c if c[0] != "PeriodicBracketTax" else ["PeriodicBracketTax", dict(c[1], tax_model="saez")]
            for c in load_scenario(TOY["b"])["cfg"]["components"]]
    senv = make_env(dict(load_scenario(TOY["b"])["cfg"], components=saez), n_envs=2, device="cuda:0")
    senv.seed(3)
    senv.reset()
    with pytest.raises(NotImplementedError, match="saez"):
        senv.step()
    # the registered subclass that overrides nothing is its parent: whole steps, capture and auto-reset
    plain = make_env(dict(cfg, scenario_name="toy_plain/simple_wood_and_stone"), n_envs=4, device="cuda:0")
    plain.seed(3)
    plain.reset()
    pb = plain.backend
    assert pb.host_components == ()
    pb.step(None, None)
    pb.set_auto_reset(True)
    pb.set_auto_reset(False)
    graphed = rollout.GraphedStep(plain, lambda t, a, p: None, auto_reset=True)
    graphed.eager(2)
    plain.check_errors()


@pytest.mark.gpu
def test_scenario_metrics_is_part_of_the_same_surface():
    register_scenarios()
    cfg = load_scenario(TOY["a"])["cfg"]

    def metrics(self, tensors):
        m = type(self).__mro__[1].scenario_metrics(self, tensors)
        m["toy/wood_cells"] = tensors["wood"].reshape(tensors["wood"].shape[0], -1).sum(1).astype(np.float64)
        return m

    env = _subclass("toy_drought/simple_wood_and_stone", "ToyMetrics", scenario_metrics=metrics)(**_kwargs(cfg, n_envs=3, device="cuda:0"))
    env.seed(2)
    env.reset()
    for _ in range(4):
        env.step()
    m = env.metrics
    wood = env.backend.tensors["wood"]
    assert np.array_equal(m["toy/wood_cells"], wood.reshape(3, -1).sum(1).cpu().numpy().astype(np.float64))
    assert int(wood[:, : wood.shape[1] // 2].sum()) == 0  # (step 4: the hook has just cleared the upper half)
    assert "social/productivity" in m and env.scenario_hooks == ("scenario_step", "generate_observations")


@pytest.mark.gpu
def test_a_batch_of_4096_hooked_replicas_steps_clean():
    import torch

    register_scenarios()
    cfg = load_scenario(TOY["a"])["cfg"]
    E = 4096
    env = make_env(cfg, n_envs=E, device="cuda:0")
    env.seed(100)
    obs = env.reset()
    be = env.backend
    A = 1 + sum(k for _, k in env.action_subspace_names()[0])
    gen = torch.Generator(device="cpu").manual_seed(1)
    for t in range(5):
        a = torch.randint(0, A, (E, 4), generator=gen, dtype=torch.int32).to("cuda:0")
        obs, rew, done, _ = env.step({"a": a})
    env.check_errors()
    wood = be.tensors["wood"]
    assert int(wood[:, : wood.shape[1] // 2].sum()) == 0 or int(be.tensors["timestep"][0]) % 4 != 0
    assert int(be.tensors["timestep"].min()) == 5 and tuple(obs["a"]["flat"].shape[:2]) == (E, 4)
    assert obs["a"]["flat"].shape[-1] == load_scenario(TOY["a"])["ob_obs_a_flat"].shape[-1]
    assert bool(torch.isfinite(rew["a"]).all())
