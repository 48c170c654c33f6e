"""User-registered components: the reference's component registry is open (F/base/base_component.py:378,
F/base/registrar.py:48-66); here a component of the user's subclasses foundation.BatchedComponent -- its dynamics run as
torch code on the batch's state tensors between launches of aie_step_range.  Three toy components, written once against the
reference's BaseComponent (oracle/gen_golden_custom.py, which produced tests/golden/custom_*.npz by running the UNMODIFIED
reference with them registered) and once as BatchedComponents (below), listed first, last, between and next to the
built-in components: state after every step, rewards, done, resets, and the flat observation vectors with the components'
keys at their sorted positions must equal the reference's."""
import zlib

import numpy as np
import pytest

from helpers import compare_state, custom_golden_names, load_golden, make_env, state_from_golden

OBS_TOL = 2e-6
REW_TOL = 1e-5


def register_toys():
    from ai_economist_amd import foundation

    if foundation.components.has("CoinSubsidy"):
        return

    @foundation.components.add
    class CoinSubsidy(foundation.BatchedComponent):
        name = "CoinSubsidy"
        required_entities = ["Coin"]
        agent_subclasses = ["BasicMobileAgent", "BasicPlanner"]

        def __init__(self, *args, amount=0.5, every=3, **kwargs):
            super().__init__(*args, **kwargs)
            self.amount, self.every = float(amount), int(every)

        def component_step(self, t):
            import torch

            coin = t["inv_coin"]
            due = (t["timestep"] % self.every == 0).to(coin.dtype)
            share = self.amount * torch.arange(1, coin.shape[1] + 1, device=coin.device, dtype=coin.dtype)
            coin += due[:, None] * share[None, :]

        def generate_observations(self, t):
            import torch

            coin = t["inv_coin"]
            E, n = coin.shape
            nxt = (self.every - t["timestep"] % self.every).to(torch.float32)
            share = torch.stack([self.amount * torch.arange(1, n + 1, device=coin.device, dtype=torch.float32),
                                 torch.full((n,), self.amount, device=coin.device)], dim=-1)
            return {"a": {"next_in": nxt[:, None].expand(E, n), "share": share[None].expand(E, n, 2)}, "p": {"next_in": nxt}}

    @foundation.components.add
    class LaborRelief(foundation.BatchedComponent):
        name = "LaborRelief"
        required_entities = ["Labor"]
        agent_subclasses = ["BasicMobileAgent"]

        def __init__(self, *args, cap=3.0, **kwargs):
            super().__init__(*args, **kwargs)
            self.cap = float(cap)

        def additional_reset_steps(self, t, env_mask=None):
            coin = t["inv_coin"]
            if env_mask is None:
                coin += 2.0
            else:
                coin += 2.0 * env_mask.to(coin.dtype)[:, None]
            return True

        def component_step(self, t):
            t["labor"].clamp_(max=self.cap)

    @foundation.components.add
    class ResetGrant(foundation.BatchedComponent):
        name = "ResetGrant"
        required_entities = ["Coin"]
        agent_subclasses = ["BasicMobileAgent"]

        def __init__(self, *args, amount=50.0, **kwargs):
            super().__init__(*args, **kwargs)
            self.amount = float(amount)

        def additional_reset_steps(self, t, env_mask=None):
            coin = t["inv_coin"]
            if env_mask is None:
                coin += self.amount
            else:
                coin += self.amount * env_mask.to(coin.dtype)[:, None]
            return True

        def component_step(self, t):
            pass


def _replica(be, e):
    out = {}
    for k, t in be.tensors.items():
        if t.shape[0] != be.E:
            continue
        v = t[e].cpu().numpy()
        out[k] = v.view(np.uint32) if k == "mt" else v
    return out


def _obs_check(obs, g, k, where, e):
    """The observation dict env.reset() / env.step() returned against the fixture's (flat vectors: the merged ones)."""
    for name in [x for x in g.keys() if x.startswith("ob_")]:
        who, key = name[3:].split("_", 2)[1], name[3:].split("_", 2)[2]  # ob_obs_a_flat -> a, flat
        want = g[name][k]
        got = obs[who][key][e].cpu().numpy()
        assert got.shape == want.shape, "%s: obs %s shape %s vs %s" % (where, name, got.shape, want.shape)
        if want.dtype.kind in "iu":
            assert np.array_equal(got, want), "%s: obs %s differs" % (where, name)
        else:
            np.testing.assert_allclose(got, want, rtol=OBS_TOL, atol=OBS_TOL, err_msg="%s: obs %s" % (where, name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", custom_golden_names())
def test_host_components_match_the_reference_with_the_same_components(name):
    import torch

    register_toys()
    g = load_golden(name)
    E = 3  # replicas 0 and 2 follow the fixture; replica 1 runs something else
    env = make_env(g["cfg"], n_envs=E, device="cuda:0")
    assert [c.name for c in env.components] == [c[0] for c in g["cfg"]["components"]]
    be = env.backend
    # the reset path: the fixture's generator state, then reset (the components' reset hooks included)
    keys = np.stack([g["pre_reset_mt"]] * E)
    be.set_rng_state(keys, np.full(E, int(g["pre_reset_pos"]), np.int32))
    obs = env.reset()
    want0 = state_from_golden(g, "s0_")
    for e in (0, 2):
        compare_state(_replica(be, e), want0, where="%s reset replica %d" % (name, e))
    obs_steps = list(g["obs_steps"])
    if 0 in obs_steps:
        _obs_check(obs, g, obs_steps.index(0), name + " reset obs", e=2)
    T = g["actions_a"].shape[0]
    resets = {int(t): i for i, t in enumerate(g.get("reset_at", []))}
    n = env.n_agents
    for t in range(T):
        a = np.zeros((E, n), np.int32)
        a[0] = a[2] = g["actions_a"][t]
        a[1] = (g["actions_a"][t] * 7 + t) % 6
        act = {"a": torch.as_tensor(a, device="cuda:0")}
        if g["actions_p"].shape[1]:
            p = np.zeros((E, g["actions_p"].shape[1]), np.int32)
            p[0] = p[2] = g["actions_p"][t]
            act["p"] = torch.as_tensor(p, device="cuda:0")
        obs, rew, done, _ = env.step(act)
        want = state_from_golden(g, "st_", t)
        for e in (0, 2):
            got = _replica(be, e)
            compare_state(got, want, where="%s step %d replica %d" % (name, t + 1, e))
            assert zlib.crc32(got["mt"].tobytes()) == int(g["st_mt_crc"][t])
            r = np.concatenate([got["rewards_a"], got["rewards_p"][None]])
            np.testing.assert_allclose(r, g["rew"][t], rtol=2e-7, atol=REW_TOL)
            assert int(got["done"]) == int(g["done"][t])
        if (t + 1) in obs_steps:
            _obs_check(obs, g, obs_steps.index(t + 1), "%s step %d" % (name, t + 1), e=2)
        if (t + 1) in resets:
            # replica 1 follows other actions but the same clock: its episode ends with the others'
            obs = env.reset(be.tensors["done"])
            compare_state(_replica(be, 0), state_from_golden(g, "rs_", resets[t + 1]), where="%s reset after step %d" % (name, t + 1))


@pytest.mark.gpu
def test_host_components_batch_and_unflattened_keys():
    """4096 replicas step through the split launches; with flatten_observations=False the component's keys appear under
    "<Component>-<key>" beside the built-in ones; a whole step through aie_step_range equals aie_step when no hook edits."""
    import torch

    from helpers import C2

    register_toys()
    comps = [list(c) for c in C2["components"]]
    cfg = dict(C2, components=comps[:2] + [["CoinSubsidy", {"amount": 1.0, "every": 2}]] + comps[2:], episode_length=6)
    env = make_env(cfg, n_envs=4096, device="cuda:0", flatten_observations=False)
    env.seed(3)
    obs = env.reset()
    be = env.backend
    assert "CoinSubsidy-next_in" in obs["a"] and "CoinSubsidy-share" in obs["a"] and "CoinSubsidy-next_in" in obs["p"]
    assert tuple(obs["a"]["CoinSubsidy-share"].shape) == (4096, 4, 2)
    for t in range(4):
        a, p = be.sample_random_actions(5, 0, slot=0)
        obs, rew, done, _ = env.step({"a": a, "p": p})
    torch.cuda.synchronize()
    assert float(obs["a"]["CoinSubsidy-next_in"][0, 0]) == float(2 - 4 % 2)
    assert int(be.tensors["timestep"].min()) == 4 and int(be.tensors["timestep"].max()) == 4
    # aie_step_range(0, n, HEAD | TAIL) == aie_step on a twin without host components
    twins = []
    for _ in range(2):
        e2 = make_env(dict(C2, episode_length=6), n_envs=64, device="cuda:0")
        e2.seed(9)
        e2.reset()
        twins.append(e2)
    a, p = twins[0].backend.sample_random_actions(8, 0, slot=0)
    for _ in range(5):
        twins[0].backend.step(a, p)
        twins[1].backend.step_range(a, p, 0, len(C2["components"]), 3)
    torch.cuda.synchronize()
    for k in twins[0].backend.tensors:
        if k != "sample_t":  # (the draw index of the synthetic policy: only the first twin drew the actions)
            assert torch.equal(twins[0].backend.tensors[k], twins[1].backend.tensors[k]), k


def test_host_component_with_actions_or_in_other_scenarios_is_refused():
    from ai_economist_amd import foundation

    register_toys()

    class Acting(foundation.BatchedComponent):
        name = "ActingToy"
        required_entities = ["Coin"]
        agent_subclasses = ["BasicMobileAgent"]

        def get_n_actions(self, agent_cls_name):
            return 3

    foundation.components.add(Acting)
    base = dict(n_agents=4, world_size=[25, 25], episode_length=10)
    with pytest.raises(NotImplementedError, match="action subspaces"):
        foundation.make_env_instance("layout_from_file/simple_wood_and_stone", components=[("Build", {}), ("ActingToy", {})], **base)
    with pytest.raises(NotImplementedError, match="gather-trade-build"):
        foundation.make_env_instance("one-step-economy", n_agents=4, world_size=[1, 1], episode_length=2,
                                     components=[("SimpleLabor", {}), ("CoinSubsidy", {})])
    # an unknown class that is no BatchedComponent keeps the clear refusal
    class Plain(foundation.BaseComponent):
        name = "PlainToy"
        required_entities = ["Coin"]
        agent_subclasses = ["BasicMobileAgent"]

    foundation.components.add(Plain)
    with pytest.raises(NotImplementedError, match="BatchedComponent"):
        foundation.make_env_instance("layout_from_file/simple_wood_and_stone", components=[("PlainToy", {})], **base)


# ---- masked resets with host components: twins instead of the oracle ----
#
# Three kinds of environment built from one configuration and seed step with the same actions: S resets the replicas of a
# mask at step k, F resets all of them at step k, N does not reset.  The kernels are the same and every replica draws
# from its own stream, so from then on the rows of S outside the mask must equal N's and the rows inside it F's, bit
# for bit: state tensors, rewards, done and the observations env.reset / env.step return (the host components' keys
# included).  A reset that reached past its mask -- the follow-up launches that rewrite the observations after the
# components' reset hooks, or retake the tax's coin snapshot -- shows up as a difference in the rows it should not touch.

TWIN_E = 7  # odd: "alternate rows" is not half of the batch


def _twin_masks(E):
    return {"first": [0], "last": [E - 1], "alternate": list(range(0, E, 2)),
            "all_but_one": [e for e in range(E) if e != E // 2], "none": [], "all": list(range(E))}


def _tax_period(cfg):
    for name, kw in cfg["components"]:
        if name == "PeriodicBracketTax":
            return int(kw.get("period", 100))
    return None


def _twin_cases():
    out = []
    for name in custom_golden_names():
        cfg = load_golden(name)["cfg"]
        T, P = int(cfg["episode_length"]), _tax_period(cfg)
        if P is not None and P < T:
            ks = [("mid_period", P + P // 2 if P + P // 2 < T else P // 2), ("tax_day", P)]
        else:  # no tax day inside an episode: the middle of the episode and its first step
            ks = [("mid_period", T // 2), ("first_step", 1)]
        for what, k in ks:
            out.append(pytest.param(name, "numpy", k, id="%s-k%d-%s" % (name, k, what)))
    # generated layouts drawn ahead of their resets (rng_mode "fast")
    out.append(pytest.param("custom_first_and_last_5ag", "fast", 7, id="custom_first_and_last_5ag-fast-k7"))
    return out


def _leaves(prefix, d, E, out):
    import torch

    for k, v in d.items():
        if isinstance(v, dict):
            _leaves("%s/%s" % (prefix, k), v, E, out)
        elif isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == E:
            out["%s/%s" % (prefix, k)] = v.detach().cpu().clone()


def _twin_snapshot(env, obs):
    """Every tensor of the backend whose leading dimension is the replica, and every observation (CPU copies)."""
    be = env.backend
    out = {}
    for k, t in be.tensors.items():
        if t.dim() >= 1 and t.shape[0] == be.E:
            out[k] = t.detach().cpu().clone()
    _leaves("obs", obs, be.E, out)
    return out


def _twin_assert(got, want, rows, where):
    import torch

    if not rows:
        return
    assert sorted(got) == sorted(want), where
    idx = torch.as_tensor(rows, dtype=torch.long)
    bad = [k for k in want if not torch.equal(got[k][idx], want[k][idx])]
    assert not bad, "%s: rows %s differ in %s" % (where, rows, bad)


def _twin_actions(env, rng, E):
    import torch

    n = env.n_agents
    sub_a, sub_p = env.action_subspace_names()
    be = env.backend
    wa = be.act_a_numel // (E * n)
    if wa == 1:
        a = rng.randint(0, 1 + sum(k for _, k in sub_a), size=(E, n, 1))
    else:
        a = np.stack([rng.randint(0, k, size=(E, n)) for _, k in sub_a], axis=-1)
    act = {"a": torch.as_tensor(a.astype(np.int32), device=be.device)}
    if sub_p:  # (a planner without actions -- a fixed-rate tax -- takes the NO-OPs env.step fills in)
        p = np.stack([rng.randint(0, k, size=E) for _, k in sub_p], axis=-1)
        act["p"] = torch.as_tensor(p.astype(np.int32), device=be.device)
    return act


@pytest.mark.gpu
@pytest.mark.parametrize("name,rng_mode,k", _twin_cases())
def test_masked_reset_with_host_components_touches_only_its_rows(name, rng_mode, k):
    import torch

    register_toys()
    cfg = load_golden(name)["cfg"]
    E = TWIN_E
    masks = _twin_masks(E)
    extra = dict(rng_mode=rng_mode) if rng_mode != "numpy" else {}

    def build():
        env = make_env(cfg, n_envs=E, device="cuda:0", **extra)
        env.seed(17)
        return env

    S = {m: build() for m in masks}
    N, F = build(), build()
    envs = list(S.values()) + [N, F]
    snap = {id(env): _twin_snapshot(env, env.reset()) for env in envs}
    T, P = int(cfg["episode_length"]), _tax_period(cfg)
    steps = k + max(2 * P if P is not None and P < T else 0, T - k) + 2  # two tax periods and past N's episode end
    rng = np.random.RandomState(1000 + k)

    def check(where):
        for m, rows in masks.items():
            s = snap[id(S[m])]
            _twin_assert(s, snap[id(N)], [e for e in range(E) if e not in rows], "%s: mask %s, outside vs no reset" % (where, m))
            _twin_assert(s, snap[id(F)], rows, "%s: mask %s, inside vs full reset" % (where, m))

    for t in range(1, steps + 1):
        act = _twin_actions(N, rng, E)
        for env in envs:
            obs, _, _, _ = env.step(act)
            snap[id(env)] = _twin_snapshot(env, obs)
        check("%s step %d" % (name, t))
        if t == k:
            for m, rows in masks.items():
                mask = torch.zeros(E, dtype=torch.uint8, device="cuda:0")
                mask[rows] = 1
                snap[id(S[m])] = _twin_snapshot(S[m], S[m].reset(mask))
            snap[id(F)] = _twin_snapshot(F, F.reset())
            check("%s reset at step %d" % (name, t))
            continue
        # replicas whose episode ended restart (a rollout's env.reset(done)); the rows of S follow their twins' clocks
        reset_any = False
        for env in envs:
            done = env.backend.tensors["done"]
            if bool(done.any().item()):
                snap[id(env)] = _twin_snapshot(env, env.reset(done))
                reset_any = True
        if reset_any:
            check("%s reset(done) after step %d" % (name, t))
    assert int(N.backend.tensors["completions"].min()) >= 1  # the untouched rows crossed an episode end


@pytest.mark.gpu
def test_paths_that_skip_the_host_hooks_are_refused():
    """The backend's whole-step calls (aie_step, aie_step_sample_next), auto-reset inside the step and GraphedStep (which
    captures aie_step and turns auto-reset on) would run steps and resets without the host components' hooks: on an
    environment with host components they raise before they launch anything; env.step and env.reset keep working."""
    import torch

    from ai_economist_amd.rollout import GraphedStep

    register_toys()
    env = make_env(load_golden("custom_grant_ahead_of_tax_4ag")["cfg"], n_envs=4, device="cuda:0")
    env.seed(3)
    env.reset()
    be = env.backend
    a, p = be.sample_random_actions(5, 0, slot=0)
    torch.cuda.synchronize()
    before = {k: t.clone() for k, t in be.tensors.items()}
    with pytest.raises(NotImplementedError, match="ResetGrant"):
        GraphedStep(env, lambda tensors, act_a, act_p: None, auto_reset=False)
    with pytest.raises(NotImplementedError, match="ResetGrant"):
        GraphedStep(env, lambda tensors, act_a, act_p: None)
    with pytest.raises(NotImplementedError, match="host components"):
        be.step(a, p)
    with pytest.raises(NotImplementedError, match="host components"):
        be.step_sample_next(a, p, 5, 0, next_slot=1)
    with pytest.raises(NotImplementedError, match="host components"):
        be.set_auto_reset(True)
    be.set_auto_reset(False)  # (off is what such an environment runs with)
    torch.cuda.synchronize()
    for k, t in be.tensors.items():
        assert torch.equal(t, before[k]), "a refused call changed %s" % k
    obs, rew, done, _ = env.step({"a": a, "p": p})
    assert int(be.tensors["timestep"].min()) == 1 and int(be.tensors["timestep"].max()) == 1
    env.reset()
    assert int(be.tensors["timestep"].max()) == 0
    # an environment without host components keeps every path
    plain = make_env(dict(load_golden("custom_grant_ahead_of_tax_4ag")["cfg"], components=[["Build", {}], ["Gather", {}]]),
                     n_envs=4, device="cuda:0")
    plain.seed(3)
    plain.reset()
    plain.backend.step(None, None)
    plain.backend.set_auto_reset(True)
    plain.backend.set_auto_reset(False)
