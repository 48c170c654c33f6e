#!/usr/bin/env python
"""Golden fixtures for user-registered SCENARIOS with hooks of their own (tests/golden/scenario/*.npz): the unmodified
reference Foundation with toy scenarios -- defined HERE against the reference's own scenario classes and registered through
its open scenario registry (F/base/base_env.py:1144, F/base/registrar.py:48-66) -- that override scenario_step,
generate_observations, compute_reward and additional_reset_steps (F/base/base_env.py:1037-1141).  The same scenarios
written against ai_economist_amd.foundation's scenario classes (tests/test_user_scenario.py) have to reproduce the fixtures:
state after every step, the generator's state, rewards, done, resets, observations with the additional keys.

Each fixture holds the fields of tools/gen_golden_acting.py (whose action policy and toy components this script imports),
with the map observations kept at the observed steps of the toys that edit the map, and
  flat_json     per actor class ("a", "p") the reference packager's sorted flattened keys with their sizes, and the keys it
                keeps as they are (F/base/base_env.py:561-589).

Toys:
  toy_drought/...      (a) scenario_step: super(), then every 4th step Wood is cleared on the upper half of the map;
                           generate_observations: a scalar, a vector and a 2 x 2 array for agents and planner
  toy_toil/...         (b) compute_reward: super(), then 0.05 * labor off every agent's reward, planner := the agents' mean
  toy_grant/...        (c) additional_reset_steps: super(), then five extra coin for agent 0
  toy_refill/...       (d) scenario_step WITHOUT super(): every 5th step all source cells are refilled; no draws
  toy_drought_uniform/ (e) (a)'s hooks on a uniform/ subclass (Stone dries up there: the upper rows are where uniform/ grows
                           it), 10 multi-action agents, Tithe among the components

Runs where the reference is installed only:   python tools/gen_golden_scenario.py
"""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402  (extract_state / extract_obs / rewards_array / GTB)
import gen_golden_acting as acting  # noqa: E402  (draw_actions, the reference-side Tithe)

OUT = os.path.join(ROOT, "tests", "golden", "scenario")
GTB = gen_golden.GTB


def register_reference_scenarios():
    foundation = acting.register_reference_toys()
    from ai_economist.foundation.base.base_env import scenario_registry
    from ai_economist.foundation.scenarios.simple_wood_and_stone.dynamic_layout import Uniform
    from ai_economist.foundation.scenarios.simple_wood_and_stone.layout_from_file import LayoutFromFile

    if scenario_registry.has("toy_drought/simple_wood_and_stone"):
        return foundation

    class DroughtHooks:
        dries = "Wood"  # (uniform/ grows its Stone in the upper rows and its Wood in the lower ones)

        def scenario_step(self):
            super().scenario_step()
            if self.world.timestep % 4 == 0:
                m = np.array(self.world.maps.get(self.dries))
                self.changed = getattr(self, "changed", 0) + int(np.sum(m[: self.world_size[0] // 2] > 0))
                m[: self.world_size[0] // 2] = 0
                self.world.maps.set(self.dries, m)

        def generate_observations(self):
            obs = super().generate_observations()
            wood, stone = self.world.maps.get("Wood"), self.world.maps.get("Stone")
            half = self.world_size[0] // 2
            wood_left = float(np.sum(wood)) * 0.01
            phase = (self.world.timestep % 4) / 4.0
            patch = np.array([[float(np.sum(wood[:half])), float(np.sum(wood[half:]))],
                              [float(np.sum(stone[:half])), float(np.sum(stone[half:]))]])
            for agent in self.world.agents:
                o = obs[str(agent.idx)]
                o["wood_left"] = wood_left
                o["season"] = np.array([phase, float(np.sum(stone)) * 0.01, agent.state["inventory"]["Coin"] * 0.5])
                o["patch"] = patch
            p = obs[self.world.planner.idx]
            p["wood_left"] = wood_left
            p["season"] = np.array([phase, float(np.sum(stone)) * 0.01, float(np.sum(wood[half:])) * 0.01])
            p["patch"] = patch
            return obs

    @scenario_registry.add
    class ToyDrought(DroughtHooks, LayoutFromFile):
        name = "toy_drought/simple_wood_and_stone"

    @scenario_registry.add
    class ToyDroughtUniform(DroughtHooks, Uniform):
        name = "toy_drought_uniform/simple_wood_and_stone"
        dries = "Stone"

    @scenario_registry.add
    class ToyToil(LayoutFromFile):
        name = "toy_toil/simple_wood_and_stone"

        def compute_reward(self):
            rew = super().compute_reward()
            self.edits = []
            for agent in self.world.agents:
                self.edits.append(0.05 * agent.state["endogenous"]["Labor"])
                rew[agent.idx] -= self.edits[-1]
            rew[self.world.planner.idx] = float(np.mean([rew[agent.idx] for agent in self.world.agents]))
            return rew

    @scenario_registry.add
    class ToyGrant(LayoutFromFile):
        name = "toy_grant/simple_wood_and_stone"

        def additional_reset_steps(self):
            super().additional_reset_steps()
            self.world.agents[0].state["inventory"]["Coin"] += 5.0

    @scenario_registry.add
    class ToyRefill(LayoutFromFile):
        name = "toy_refill/simple_wood_and_stone"

        def scenario_step(self):  # (no super(): no stochastic regeneration, no draws)
            if self.world.timestep % 5 == 0:
                for res in ("Wood", "Stone"):
                    self.changed = getattr(self, "changed", 0) + int(np.sum(
                        self.world.maps.get(res) < self.world.maps.get(res + "SourceBlock")))
                    self.world.maps.set(res, np.maximum(self.world.maps.get(res), self.world.maps.get(res + "SourceBlock")))

    return foundation


LAYOUT = "quadrant_25x25_20each_30clump.txt"
DENSE = "uniform_25x25_25each_65clump.txt"
CASES = {
    "scenario_a_drought_4ag": dict(
        cfg=dict(scenario_name="toy_drought/simple_wood_and_stone", n_agents=4, world_size=[25, 25], episode_length=18,
                 components=[GTB[0], GTB[1], GTB[2]], starting_agent_coin=10, resource_regen_prob=0.05, env_layout_file=LAYOUT),
        seed=31, t_steps=24, obs_steps=[0, 4, 5, 18, 24], keep_maps=True),
    "scenario_b_toil_4ag": dict(
        cfg=dict(scenario_name="toy_toil/simple_wood_and_stone", n_agents=4, world_size=[25, 25], episode_length=20,
                 components=[GTB[0], GTB[1], GTB[2], ["PeriodicBracketTax", {"period": 7}]],
                 starting_agent_coin=10, env_layout_file=LAYOUT),
        seed=37, t_steps=28, obs_steps=[0, 1, 7, 8, 20, 28]),
    "scenario_c_grant_4ag": dict(
        cfg=dict(scenario_name="toy_grant/simple_wood_and_stone", n_agents=4, world_size=[25, 25], episode_length=12,
                 components=[GTB[0], GTB[1], GTB[2], ["PeriodicBracketTax", {"period": 5}]],
                 starting_agent_coin=3, env_layout_file=LAYOUT),
        seed=43, t_steps=20, obs_steps=[0, 1, 2, 5, 6, 12, 13, 20]),
    "scenario_d_refill_4ag": dict(
        cfg=dict(scenario_name="toy_refill/simple_wood_and_stone", n_agents=4, world_size=[25, 25], episode_length=22,
                 components=[GTB[0], GTB[1], GTB[2]], starting_agent_coin=10, env_layout_file=DENSE),
        seed=50, t_steps=30, obs_steps=[0, 1, 5, 6, 22, 30]),
    "scenario_e_drought_uniform_tithe_10ag": dict(
        cfg=dict(scenario_name="toy_drought_uniform/simple_wood_and_stone", n_agents=10, world_size=[15, 15], episode_length=12,
                 components=[["Build", {}], ["Tithe", {}], ["Gather", {}]], multi_action_mode_agents=True,
                 starting_agent_coin=3, starting_stone_coverage=0.12, starting_wood_coverage=0.12),
        seed=53, t_steps=17, obs_steps=[0, 4, 12, 17], keep_maps=True),
}


def _flat_tables(env):
    """The packager's decision per actor class, with sizes (from the unflattened observations)."""
    raw = env._generate_observations(flatten_observations=False, flatten_masks=True)
    out = {}
    for who, idx in (("a", "0"), ("p", "p")):
        keep_as_is, flatten, _ = env._packagers[idx]
        out[who] = {"flat": [(k, int(np.asarray(raw[idx][k]).size)) for k in flatten],
                    "kept": sorted(k for k in keep_as_is if k != "time")}
    return out


def run_case(name, cfg, seed, t_steps, obs_steps, keep_maps=False, action_seed=321):
    foundation = register_reference_scenarios()
    kwargs = dict(cfg)
    scenario = kwargs.pop("scenario_name")
    kwargs["components"] = [tuple(c) for c in kwargs["components"]]
    np.random.seed(seed + 1000)
    env = foundation.make_env_instance(scenario, **kwargs)
    np.random.seed(seed)
    st = np.random.get_state()
    out = {"cfg_json": np.array(json.dumps(cfg)), "construction_seed": np.array(seed + 1000, np.int64),
           "pre_reset_mt": np.array(st[1], np.uint32), "pre_reset_pos": np.array(st[2], np.int32)}
    toys = [c for c in env._components if c.name in acting.TOYS]
    obs = env.reset()
    out["flat_json"] = np.array(json.dumps(_flat_tables(env)))
    for k, v in gen_golden.extract_state(env).items():
        out["s0_" + k] = v
    rng = np.random.RandomState(action_seed)
    acts, acts_p = acting.draw_actions(env, rng, t_steps)
    out["actions_a"], out["actions_p"] = acts, acts_p
    states, rews, dones, kept, obs_rec, reset_states, host_a, edits = [], [], [], [], {}, [], [], []
    multi_a, multi_p = env.world.agents[0].multi_action_mode, env.world.planner.multi_action_mode

    def keep(t, o):
        kept.append(t)
        for k, v in gen_golden.extract_obs(env, o).items():
            if keep_maps or not (k.endswith("world-map") or k.endswith("world-idx_map")):
                obs_rec.setdefault(k, []).append(v)

    if 0 in obs_steps:
        keep(0, obs)
    for t in range(t_steps):
        ad = {str(i): ([int(x) for x in acts[t, i]] if multi_a else int(acts[t, i])) for i in range(env.n_agents)}
        if acts_p.shape[1]:
            ad["p"] = [int(x) for x in acts_p[t]] if multi_p else int(acts_p[t, 0])
        obs, rew, done, _ = env.step(ad)
        sa = [c.seen for c in toys]
        host_a.append(np.concatenate([np.asarray(s, np.int32).reshape(env.n_agents, -1) for s in sa], axis=1)
                      if sa else np.zeros((env.n_agents, 0), np.int32))
        if hasattr(env, "edits"):
            edits.append(list(env.edits))
        states.append(gen_golden.extract_state(env))
        rews.append(gen_golden.rewards_array(env, rew))
        dones.append(done["__all__"])
        if (t + 1) in obs_steps:
            keep(t + 1, obs)
        if done["__all__"] and t + 1 < t_steps:
            obs = env.reset()
            reset_states.append((t + 1, gen_golden.extract_state(env)))
    if hasattr(env, "scenario_step") and type(env).__name__ != "ToyToil" and type(env).__name__ != "ToyGrant":
        assert getattr(env, "changed", 0) > 0, name  # toys (a), (d), (e): the hook's map edit did change cells
    if edits:  # toy (b): a skipped hook must miss the reward bar by orders of magnitude on most steps
        big = np.mean(np.max(np.array(edits), axis=1) >= 1e-2)
        assert big > 0.5, (name, big)
    for k in states[0]:
        if k == "mt":
            out["st_mt_crc"] = np.array([zlib.crc32(s["mt"].tobytes()) for s in states], np.uint32)
            continue
        out["st_" + k] = np.stack([s[k] for s in states])
    out["rew"], out["done"] = np.stack(rews), np.array(dones, np.uint8)
    out["host_a"] = np.stack(host_a)
    out["obs_steps"] = np.array(kept, np.int32)
    for k, v in obs_rec.items():
        out["ob_" + k] = np.stack(v)
    assert reset_states, name
    out["reset_at"] = np.array([t for t, _ in reset_states], np.int32)
    for k in reset_states[0][1]:
        if k != "mt":
            out["rs_" + k] = np.stack([s[k] for _, s in reset_states])
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-40s %6.1f KB  wood at the end %d, cells the hook changed %d, reward range [%.3f, %.3f]" % (
        name, os.path.getsize(path) / 1024.0, int(states[-1]["wood"].sum()), getattr(env, "changed", 0), out["rew"].min(),
        out["rew"].max()))


if __name__ == "__main__":
    for case, kw in CASES.items():
        run_case(case, **kw)
