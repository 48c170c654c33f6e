#!/usr/bin/env python
"""Golden fixtures for host components that ACT (tests/golden/acting/*.npz): the unmodified reference Foundation with toy
components -- defined HERE against the reference's own BaseComponent and registered through its open component registry
(F/base/base_component.py:378, F/base/registrar.py:48-66) -- that own action subspaces and masks (get_n_actions +
generate_masks + component_step, F/base/base_component.py:159-176, 262-290), listed among the built-in ones.  The same
components written as ai_economist_amd.foundation.ActingComponent (tests/test_acting_component.py) have to reproduce the
fixtures: the action layout, state after every step, rewards, the decoded sub-actions, the flattened masks.

Each fixture holds (format of oracle/gen_golden.py, whose extraction helpers this script imports as they are):
  cfg_json, pre_reset_mt / pre_reset_pos, s0_<field>, st_<field> [T, ...], st_mt_crc, rew, done, reset_at / rs_<field>,
  actions_a [T, n] (single-action agents) or [T, n, subspaces], actions_p [T, planner columns],
  host_a [T, n, Ha] / host_p [T, Hp]      the foreign sub-actions as the toy components read them (get_component_action),
  obs_steps [K], ob_obs_{a,p}_{flat,action_mask,time}, ob_obs_p_agents     observations at the observed steps (0: reset),
  layout_json                              per actor class the reference's action-name list and action_dim,
  masks_json                               at every observed step the reference's flatten_masks=False mask dictionaries.

Runs where the reference is installed only:   python tools/gen_golden_acting.py
"""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden  # noqa: E402  (extract_state / extract_obs / rewards_array / sample_actions / GTB)
from ref_harness import load_reference_foundation  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "acting")
GTB = gen_golden.GTB


def register_reference_toys():
    foundation = load_reference_foundation()
    from ai_economist.foundation.base.base_component import BaseComponent, component_registry

    if component_registry.has("Tithe"):
        return foundation

    @component_registry.add
    class Tithe(BaseComponent):
        """Agents, one int subspace with a state-dependent mask: choice k moves k coin into a pot that is split equally
        among all agents; allowed iff the agent holds at least k coin, a forbidden choice does nothing."""
        name = "Tithe"
        required_entities = ["Coin", "House"]  # (House: the scenario's maps need the landmark even where Build is not listed)
        agent_subclasses = ["BasicMobileAgent"]

        def get_n_actions(self, agent_cls_name):
            return 3 if agent_cls_name == "BasicMobileAgent" else None

        def get_additional_state_fields(self, agent_cls_name):
            return {}

        def component_step(self):
            pot = 0.0
            self.seen = []
            for agent in self.world.agents:
                k = int(agent.get_component_action(self.name))
                self.seen.append([k])
                if k > 0 and agent.state["inventory"]["Coin"] >= k:
                    agent.state["inventory"]["Coin"] -= float(k)
                    pot += float(k)
            share = pot / self.n_agents
            for agent in self.world.agents:
                agent.state["inventory"]["Coin"] += share

        def generate_observations(self):
            return {}

        def generate_masks(self, completions=0):
            return {agent.idx: np.array([agent.state["inventory"]["Coin"] >= k for k in (1, 2, 3)], np.float32)
                    for agent in self.world.agents}

    @component_registry.add
    class Regimen(BaseComponent):
        """Agents, two named sub-actions: "rest" (1 choice: one unit of labor less, not below zero; allowed while there
        is labor) and "train" (choice k: pay k coin for k / 2 units of labor; allowed iff the agent holds k coin)."""
        name = "Regimen"
        required_entities = ["Coin", "Labor"]
        agent_subclasses = ["BasicMobileAgent"]

        def get_n_actions(self, agent_cls_name):
            return [("rest", 1), ("train", 2)] if agent_cls_name == "BasicMobileAgent" else None

        def get_additional_state_fields(self, agent_cls_name):
            return {}

        def component_step(self):
            self.seen = []
            for agent in self.world.agents:
                rest = int(agent.get_component_action(self.name, "rest"))
                train = int(agent.get_component_action(self.name, "train"))
                self.seen.append([rest, train])
                if rest == 1 and agent.state["endogenous"]["Labor"] > 0:
                    agent.state["endogenous"]["Labor"] = max(agent.state["endogenous"]["Labor"] - 1.0, 0.0)
                if train > 0 and agent.state["inventory"]["Coin"] >= train:
                    agent.state["inventory"]["Coin"] -= float(train)
                    agent.state["endogenous"]["Labor"] += 0.5 * train

        def generate_observations(self):
            return {}

        def generate_masks(self, completions=0):
            return {agent.idx: {"rest": np.array([agent.state["endogenous"]["Labor"] > 0], np.float32),
                                "train": np.array([agent.state["inventory"]["Coin"] >= k for k in (1, 2)], np.float32)}
                    for agent in self.world.agents}

    @component_registry.add
    class Stimulus(BaseComponent):
        """Planner, one int subspace with a time-dependent mask: on every `every`-th timestep choice k pays each agent
        k * amount coin; the mask is open only when the coming step is such a step, a forbidden choice does nothing."""
        name = "Stimulus"
        required_entities = ["Coin"]
        agent_subclasses = ["BasicPlanner"]

        def __init__(self, *args, amount=0.5, every=3, **kwargs):
            super().__init__(*args, **kwargs)
            self.amount = float(amount)
            self.every = int(every)

        def get_n_actions(self, agent_cls_name):
            return 4 if agent_cls_name == "BasicPlanner" else None

        def get_additional_state_fields(self, agent_cls_name):
            return {}

        def component_step(self):
            k = int(self.world.planner.get_component_action(self.name))
            self.seen = [k]
            if k > 0 and self.world.timestep % self.every == 0:
                for agent in self.world.agents:
                    agent.state["inventory"]["Coin"] += k * self.amount

        def generate_observations(self):
            return {}

        def generate_masks(self, completions=0):
            is_open = (self.world.timestep + 1) % self.every == 0
            return {self.world.planner.idx: np.full(4, 1.0 if is_open else 0.0, np.float32)}

    return foundation


LAYOUT = "quadrant_25x25_20each_30clump.txt"
CASES = {
    # 1. the full tuple with taxes the planner sets, Tithe between the auction and Gather, across an episode end
    "acting_tithe_mid_4ag": dict(
        cfg=dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=4, world_size=[25, 25], episode_length=24,
                 components=[GTB[0], GTB[1], ["Tithe", {}], GTB[2], ["PeriodicBracketTax", {"period": 8}]],
                 starting_agent_coin=10, env_layout_file=LAYOUT),
        seed=41, t_steps=32, obs_steps=[0, 1, 2, 8, 9, 24, 25, 32]),
    # 2. multi-action agents on a generated layout, the two-sub-action component listed first
    "acting_regimen_first_multi_5ag": dict(
        cfg=dict(scenario_name="uniform/simple_wood_and_stone", n_agents=5, world_size=[15, 15], episode_length=16,
                 components=[["Regimen", {}], ["Build", {}], ["Gather", {}]], multi_action_mode_agents=True,
                 starting_agent_coin=3, starting_stone_coverage=0.12, starting_wood_coverage=0.12),
        seed=7, t_steps=22, obs_steps=[0, 1, 2, 16, 17, 22]),
    # 3. a planner subspace AHEAD of the tax brackets, single-action planner, 10 agents
    "acting_stimulus_ahead_single_10ag": dict(
        cfg=dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=10, world_size=[25, 25], episode_length=20,
                 components=[GTB[0], GTB[1], GTB[2], ["Stimulus", {"amount": 0.5, "every": 3}],
                             ["PeriodicBracketTax", {"period": 6}]],
                 multi_action_mode_planner=False, starting_agent_coin=10, env_layout_file=LAYOUT),
        seed=13, t_steps=20, obs_steps=[0, 1, 2, 3, 6, 7, 20]),
    # 4. the planner subspace BEHIND the tax brackets, multi-action planner
    "acting_stimulus_behind_multi_4ag": dict(
        cfg=dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=4, world_size=[25, 25], episode_length=20,
                 components=[GTB[0], GTB[1], GTB[2], ["PeriodicBracketTax", {"period": 5}],
                             ["Stimulus", {"amount": 1.5, "every": 4}]],
                 multi_action_mode_planner=True, starting_agent_coin=10, env_layout_file=LAYOUT),
        seed=17, t_steps=20, obs_steps=[0, 1, 3, 4, 5, 6, 20]),
    # 5. Tithe as the agents' ONLY acting component: the reference's one-component single-action path (base_agent.py:163-165)
    "acting_tithe_only_4ag": dict(
        cfg=dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=4, world_size=[25, 25], episode_length=12,
                 components=[["Tithe", {}], ["PeriodicBracketTax", {"period": 4}]],
                 starting_agent_coin=2, env_layout_file=LAYOUT),
        seed=23, t_steps=18, obs_steps=[0, 1, 2, 4, 5, 12, 13, 18]),
}
TOYS = ("Tithe", "Regimen", "Stimulus")


def draw_actions(env, rng, t_steps, p_foreign=0.45):
    """Actions per step: gen_golden's biased policy for the built-in subspaces; the foreign subspaces get a uniformly
    random choice (NO-OP included) with probability p_foreign -- whatever the masks say, so that allowed and forbidden
    choices both occur."""
    n = env.n_agents
    ag = env.world.agents[0]
    names = list(ag._action_names)
    foreign = [k for k, nm in enumerate(names) if nm.split(".")[0] in TOYS]
    if ag.multi_action_mode:
        acts = np.zeros((t_steps, n, len(names)), np.int32)
        for t in range(t_steps):
            for i in range(n):
                u = rng.rand()
                for k, nm in enumerate(names):
                    d = ag.action_dim[nm]  # (NO-OP included in multi-action mode)
                    if k in foreign:
                        acts[t, i, k] = rng.randint(0, d) if rng.rand() < p_foreign else 0
                    elif nm == "Gather" and u < 0.6:
                        acts[t, i, k] = rng.randint(1, d)
                    elif nm == "Build" and 0.6 <= u < 0.85:
                        acts[t, i, k] = 1
    else:
        acts, _, _ = gen_golden.sample_actions(env, rng, t_steps)
        base, ranges = 1, {}
        for nm in names:
            ranges[nm] = (base, base + ag.action_dim[nm])
            base += ag.action_dim[nm]
        for t in range(t_steps):
            for i in range(n):
                if foreign and rng.rand() < p_foreign:
                    lo, hi = ranges[names[foreign[rng.randint(0, len(foreign))]]]
                    acts[t, i] = rng.randint(lo, hi)
    pl = env.world.planner
    pnames = list(pl._action_names)
    if not pnames or pnames[0] == "PassiveAgentPlaceholder":
        return acts, np.zeros((t_steps, 0), np.int32)
    if pl.multi_action_mode:
        acts_p = np.stack([rng.randint(0, pl.action_dim[nm], size=t_steps) for nm in pnames], axis=1).astype(np.int32)
    else:
        total = 1 + sum(pl.action_dim[nm] for nm in pnames)
        acts_p = rng.randint(0, total, size=(t_steps, 1)).astype(np.int32)
        base = 1
        for nm in pnames:  # the foreign rows often enough
            if nm.split(".")[0] in TOYS:
                pick = rng.rand(t_steps) < p_foreign
                acts_p[pick, 0] = rng.randint(base, base + pl.action_dim[nm], size=int(pick.sum()))
            base += pl.action_dim[nm]
    return acts, acts_p


def _layout(actor):
    return {"names": list(actor._action_names), "action_dim": {k: int(v) for k, v in actor.action_dim.items()},
            "multi_action_mode": bool(actor.multi_action_mode)}


def run_case(name, cfg, seed, t_steps, obs_steps, action_seed=321):
    foundation = register_reference_toys()
    kwargs = dict(cfg)
    scenario = kwargs.pop("scenario_name")
    kwargs["components"] = [tuple(c) for c in kwargs["components"]]
    np.random.seed(seed + 1000)
    env = foundation.make_env_instance(scenario, **kwargs)
    np.random.seed(seed)
    st = np.random.get_state()
    out = {"cfg_json": np.array(json.dumps(cfg)), "construction_seed": np.array(seed + 1000, np.int64),
           "pre_reset_mt": np.array(st[1], np.uint32), "pre_reset_pos": np.array(st[2], np.int32)}
    out["layout_json"] = np.array(json.dumps({"a": _layout(env.world.agents[0]), "p": _layout(env.world.planner)}))
    toys = [c for c in env._components if c.name in TOYS]
    obs = env.reset()
    for k, v in gen_golden.extract_state(env).items():
        out["s0_" + k] = v
    rng = np.random.RandomState(action_seed)
    acts, acts_p = draw_actions(env, rng, t_steps)
    out["actions_a"], out["actions_p"] = acts, acts_p
    states, rews, dones, kept, obs_rec, masks_rec, reset_states, host_a, host_p = [], [], [], [], {}, [], [], [], []
    multi_a, multi_p = env.world.agents[0].multi_action_mode, env.world.planner.multi_action_mode

    def keep(t, o):
        kept.append(t)
        for k, v in gen_golden.extract_obs(env, o).items():
            if "world-" not in k:  # the flat vectors, masks and time: the maps are the built-in fixtures' business
                obs_rec.setdefault(k, []).append(v)
        masks_rec.append(env._generate_masks(flatten_masks=False))

    if 0 in obs_steps:
        keep(0, obs)
    n_forbidden = n_allowed = 0
    for t in range(t_steps):
        ad = {str(i): ([int(x) for x in acts[t, i]] if multi_a else int(acts[t, i])) for i in range(env.n_agents)}
        if acts_p.shape[1]:
            ad["p"] = [int(x) for x in acts_p[t]] if multi_p else int(acts_p[t, 0])
        before = {c.name: c.generate_masks() for c in toys}
        obs, rew, done, _ = env.step(ad)
        sa = [c.seen for c in toys if "BasicMobileAgent" in c.agent_subclasses]
        sp = [c.seen for c in toys if "BasicPlanner" in c.agent_subclasses]
        host_a.append(np.concatenate([np.asarray(s, np.int32).reshape(env.n_agents, -1) for s in sa], axis=1)
                      if sa else np.zeros((env.n_agents, 0), np.int32))
        host_p.append(np.concatenate([np.asarray(s, np.int32).reshape(-1) for s in sp]) if sp else np.zeros(0, np.int32))
        for c in toys:  # how many foreign choices the mask in force allowed / forbade
            for idx, m in before[c.name].items():
                row = np.asarray(c.seen if idx == "p" else c.seen[int(idx)]).reshape(-1)
                ms = list(m.values()) if isinstance(m, dict) else [m]
                for choice, mm in zip(row, ms):
                    if choice > 0:
                        if mm[choice - 1] > 0:
                            n_allowed += 1
                        else:
                            n_forbidden += 1
        states.append(gen_golden.extract_state(env))
        rews.append(gen_golden.rewards_array(env, rew))
        dones.append(done["__all__"])
        if (t + 1) in obs_steps:
            keep(t + 1, obs)
        if done["__all__"] and t + 1 < t_steps:
            obs = env.reset()
            reset_states.append((t + 1, gen_golden.extract_state(env)))
    assert n_allowed > 0 and n_forbidden > 0, (name, n_allowed, n_forbidden)
    for k in states[0]:
        if k == "mt":
            out["st_mt_crc"] = np.array([zlib.crc32(s["mt"].tobytes()) for s in states], np.uint32)
            continue
        out["st_" + k] = np.stack([s[k] for s in states])
    out["rew"], out["done"] = np.stack(rews), np.array(dones, np.uint8)
    out["host_a"], out["host_p"] = np.stack(host_a), np.stack(host_p)
    out["obs_steps"] = np.array(kept, np.int32)
    for k, v in obs_rec.items():
        out["ob_" + k] = np.stack(v)
    out["masks_json"] = np.array(json.dumps(masks_rec))
    if reset_states:
        out["reset_at"] = np.array([t for t, _ in reset_states], np.int32)
        for k in reset_states[0][1]:
            if k != "mt":
                out["rs_" + k] = np.stack([s[k] for _, s in reset_states])
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-36s %6.1f KB  foreign choices: %d allowed, %d forbidden; agents %s; planner %s" % (
        name, os.path.getsize(path) / 1024.0, n_allowed, n_forbidden, env.world.agents[0]._action_names,
        env.world.planner._action_names))


if __name__ == "__main__":
    for case, kw in CASES.items():
        run_case(case, **kw)
