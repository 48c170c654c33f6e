"""Host components that ACT (foundation.ActingComponent): a user's component owns action subspaces and their masks, the
reference's component contract get_n_actions + generate_masks + component_step (F/base/base_component.py:159-176, 262-290;
the action layout of F/base/base_agent.py:97-180).  Three toy components, written once against the reference's
BaseComponent (tools/gen_golden_acting.py, which produced tests/golden/acting/*.npz by running the UNMODIFIED reference with
them registered) and once as ActingComponents (below): the action names, dimensions and mask keys, the decoded sub-actions,
state after every step, rewards, done, resets and the flattened masks -- the components' entries included -- must equal
the reference's; the device samplers must respect the components' masks."""
import glob
import json
import os
import zlib

import numpy as np
import pytest

from helpers import GOLDEN, compare_state, make_env, state_from_golden

OBS_TOL = 2e-6  # the project's bars for host-component fixtures (tests/test_batched_component.py)
REW_TOL = 1e-5
ACTING = os.path.join(GOLDEN, "acting")


def acting_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ACTING, "*.npz")))


def load_acting(name):
    with np.load(os.path.join(ACTING, name + ".npz")) as z:
        g = {k: z[k] for k in z.files}
    g["cfg"] = json.loads(str(g["cfg_json"]))
    g["cfg"]["_construction_seed"] = int(g["construction_seed"])
    g["layout"] = json.loads(str(g["layout_json"]))
    g["masks"] = json.loads(str(g["masks_json"]))
    return g


@pytest.fixture(autouse=True)
def _registry_as_found():
    """tests/test_cabi_symbols.py pins the component registry's entries: the classes this file registers leave it again
    with the test that registered them."""
    from ai_economist_amd import foundation

    reg = foundation.components
    names, by_lower = list(reg._names), dict(reg._by_lower)
    yield
    reg._names[:] = names
    reg._by_lower.clear()
    reg._by_lower.update(by_lower)


def register_toys():
    import torch

    from ai_economist_amd import foundation

    if foundation.components.has("Tithe"):
        return

    @foundation.components.add
    class Tithe(foundation.ActingComponent):
        name = "Tithe"
        required_entities = ["Coin", "House"]
        agent_subclasses = ["BasicMobileAgent"]

        def get_n_actions(self, agent_cls_name):
            return 3 if agent_cls_name == "BasicMobileAgent" else None

        def component_step(self, t):
            coin = t["inv_coin"]
            k = self.agent_actions(t).to(coin.dtype)
            k = k * (coin >= k).to(coin.dtype)  # a forbidden choice does nothing
            coin -= k
            coin += k.sum(dim=1, keepdim=True) / coin.shape[1]

        def generate_masks(self, t, completions=0):
            coin = t["inv_coin"]
            return {"a": coin[:, :, None] >= torch.arange(1, 4, device=coin.device, dtype=coin.dtype)}

    @foundation.components.add
    class Regimen(foundation.ActingComponent):
        name = "Regimen"
        required_entities = ["Coin", "Labor"]
        agent_subclasses = ["BasicMobileAgent"]

        def get_n_actions(self, agent_cls_name):
            return [("rest", 1), ("train", 2)] if agent_cls_name == "BasicMobileAgent" else None

        def component_step(self, t):
            coin, labor = t["inv_coin"], t["labor"]
            resting = (self.agent_actions(t, "rest") == 1) & (labor > 0)
            labor.copy_(torch.where(resting, (labor - 1.0).clamp(min=0.0), labor))
            train = self.agent_actions(t, "train").to(coin.dtype)
            train = train * (coin >= train).to(coin.dtype)
            coin -= train
            labor += 0.5 * train

        def generate_masks(self, t, completions=0):
            coin = t["inv_coin"]
            return {"a": {"rest": (t["labor"] > 0)[:, :, None],
                          "train": coin[:, :, None] >= torch.arange(1, 3, device=coin.device, dtype=coin.dtype)}}

    @foundation.components.add
    class Stimulus(foundation.ActingComponent):
        name = "Stimulus"
        required_entities = ["Coin"]
        agent_subclasses = ["BasicPlanner"]

        def __init__(self, *args, amount=0.5, every=3, **kwargs):
            super().__init__(*args, **kwargs)
            self.amount, self.every = float(amount), int(every)

        def get_n_actions(self, agent_cls_name):
            return 4 if agent_cls_name == "BasicPlanner" else None

        def component_step(self, t):
            coin = t["inv_coin"]
            k = self.planner_actions(t).to(coin.dtype)
            due = (t["timestep"] % self.every == 0).to(coin.dtype)
            coin += (k * self.amount * due)[:, None]

        def generate_masks(self, t, completions=0):
            is_open = (t["timestep"] + 1) % self.every == 0
            return {"p": is_open[:, None].expand(is_open.shape[0], 4)}


# ---------------------------------------------------------------- CPU: the action layout and the construction errors

def _reference_layout(g, who):
    lay = g["layout"][who]
    names = [nm for nm in lay["names"] if nm != "PassiveAgentPlaceholder"]
    extra = 1 if lay["multi_action_mode"] else 0  # (action_dim counts the sub-action's own NO-OP in multi-action mode)
    return names, [lay["action_dim"][nm] - extra for nm in names], lay["multi_action_mode"]


@pytest.mark.parametrize("name", acting_names())
def test_action_names_dims_and_mask_keys_equal_the_reference(name):
    import ctypes

    from ai_economist_amd import _build, _cabi
    from ai_economist_amd.foundation.obs_keys import mask_keys

    register_toys()
    g = load_acting(name)
    env = make_env(g["cfg"])
    got = dict(zip("ap", env.action_subspace_names()))
    tab = mask_keys(env)
    for who in "ap":
        names, dims, multi = _reference_layout(g, who)
        assert [nm for nm, _ in got[who]] == names
        assert [k for _, k in got[who]] == dims
        # the flattened mask: one leading NO-OP entry (single-action) or one per subspace (multi-action), base_agent.py:440-460
        off, want = 0 if multi else 1, []
        for nm, k in zip(names, dims):
            off += 1 if multi else 0
            want.append((nm, off, k))
            off += k
        assert tab[who] == want
        assert tab["sizes"][who] == g["ob_obs_%s_action_mask" % who].shape[-1] == max(off, 1)
        # (flatten_masks=False: a dictionary; the reference fills it component by component in each component's own key
        # order, e.g. the auction's Sell_ before Buy_, so the key SET is what is compared)
        ref_keys = g["masks"][0]["0" if who == "a" else "p"].keys()
        assert sorted(nm for nm, _, _ in tab[who]) == sorted(ref_keys)
    # the C layout takes the same configuration (no GPU needed) and gives the host-action tensors room
    lib = _cabi.bind(ctypes.CDLL(_build.build()))
    cfg = env.build_config()
    nbytes = lib.aie_arena_bytes(ctypes.byref(cfg))
    assert nbytes > 0, lib.aie_last_error(None)
    assert cfg.host_a_n == g["host_a"].shape[-1] and cfg.host_p_n == g["host_p"].shape[-1]
    assert cfg.host_a_n + cfg.host_p_n > 0
    plain = env.build_config()
    plain.host_a_n = plain.host_p_n = 0
    assert 0 < lib.aie_arena_bytes(ctypes.byref(plain)) < nbytes


def test_all_five_acting_fixtures_are_present():
    assert acting_names() == ["acting_regimen_first_multi_5ag", "acting_stimulus_ahead_single_10ag",
                              "acting_stimulus_behind_multi_4ag", "acting_tithe_mid_4ag", "acting_tithe_only_4ag"]
    for name in acting_names():
        assert os.path.getsize(os.path.join(ACTING, name + ".npz")) < 128 * 1024


def _toy(n_actions, cls_name, base=None):
    from ai_economist_amd import foundation

    base = base or foundation.ActingComponent

    class Toy(base):
        name = cls_name
        required_entities = ["Coin"]
        agent_subclasses = ["BasicMobileAgent", "BasicPlanner"]

        def get_n_actions(self, agent_cls_name):
            return n_actions(agent_cls_name) if callable(n_actions) else n_actions

        def component_step(self, t):
            pass

    if not foundation.components.has(cls_name):
        foundation.components.add(Toy)
    return cls_name


def test_construction_errors_and_refusals():
    import ctypes

    from ai_economist_amd import _build, _cabi, foundation

    register_toys()
    base = dict(n_agents=4, world_size=[25, 25], episode_length=10)

    def gtb(toy, **kw):
        return foundation.make_env_instance("layout_from_file/simple_wood_and_stone",
                                            components=[("Build", {}), (toy, {}), ("Gather", {})], **dict(base, **kw))

    with pytest.raises(NameError, match="illegally named"):  # base_agent.py:136-142
        gtb(_toy([("a.b", 2)], "ActDotted"))
    with pytest.raises(TypeError, match="unexpected type"):  # base_agent.py:148-153
        gtb(_toy("three", "ActString"))
    with pytest.raises(ValueError, match="too many action subspaces"):
        gtb(_toy([("s%d" % k, 2) for k in range(9)], "ActNine"))
    # n == 0 entries and None / 0 register nothing (base_agent.py:121-135)
    env = gtb(_toy(lambda cls: [("none", 0), ("two", 2)] if cls == "BasicMobileAgent" else 0, "ActSparse"))
    names_a, names_p = env.action_subspace_names()
    assert names_a == [("Build", 1), ("ActSparse.two", 2), ("Gather", 4)] and names_p == []
    cfg = env.build_config()
    assert (cfg.host_a_n, cfg.host_a_dim[0], cfg.host_a_before[0], cfg.host_p_n) == (1, 2, 1, 0)
    # the library refuses what the mirror would never send: a count past the table, a non-positive dimension, an order
    lib = _cabi.bind(ctypes.CDLL(_build.build()))
    assert lib.aie_arena_bytes(ctypes.byref(cfg)) > 0
    for field, value in (("host_a_n", _cabi.MAX_HOST_SUBSPACES + 1), ("host_p_n", -1)):
        bad = env.build_config()
        setattr(bad, field, value)
        assert lib.aie_arena_bytes(ctypes.byref(bad)) == _cabi.E_INVALID
        assert b"host components" in lib.aie_last_error(None)
    bad = env.build_config()
    bad.host_a_dim[0] = 0
    assert lib.aie_arena_bytes(ctypes.byref(bad)) == _cabi.E_INVALID
    bad = env.build_config()
    bad.host_a_before[0] = cfg.n_components + 1
    assert lib.aie_arena_bytes(ctypes.byref(bad)) == _cabi.E_INVALID
    # a flattened mask past AIE_MAX_MASK is refused with the sizes in the message
    wide = gtb(_toy(lambda cls: _cabi.MAX_MASK if cls == "BasicMobileAgent" else None, "ActWide")).build_config()
    assert lib.aie_arena_bytes(ctypes.byref(wide)) == _cabi.E_INVALID
    assert b"mask too long" in lib.aie_last_error(None)
    # a plain BatchedComponent with actions stays refused, and the message names the way in
    with pytest.raises(NotImplementedError, match="action subspaces.*ActingComponent"):
        gtb(_toy(3, "ActPlainBatched", base=foundation.BatchedComponent))
    # COVID / one-step-economy, dense logs: refused as for every host component
    with pytest.raises(NotImplementedError, match="gather-trade-build"):
        foundation.make_env_instance("one-step-economy", n_agents=4, world_size=[1, 1], episode_length=2,
                                     components=[("SimpleLabor", {}), ("Tithe", {})])
    from helpers import covid_golden_names, load_covid_golden

    covid = dict(load_covid_golden(covid_golden_names()[0])["cfg"], scenario_name="CovidAndEconomySimulation")
    covid["components"] = list(covid["components"]) + [("Stimulus", {})]
    with pytest.raises(NotImplementedError, match="gather-trade-build"):
        make_env(covid)
    with pytest.raises(NotImplementedError, match="dense logs"):
        gtb("Tithe", dense_log_frequency=1)


def test_layout_without_foreign_subspaces_is_unchanged():
    """With the new aie_config fields zero the planner's generalised layout is the old one: the single-action and
    multi-action mask sizes of the BASELINE tuple (1 + 7 x 21 and 7 x 22 planner entries; 1 + 1 + 4 x 11 + 4 agent ones)."""
    from helpers import C2
    from ai_economist_amd.foundation.obs_keys import mask_keys

    for multi_p, want_p in ((True, 7 * 22), (False, 1 + 7 * 21)):
        env = make_env(dict(C2, multi_action_mode_planner=multi_p))
        cfg = env.build_config()
        assert cfg.host_a_n == 0 and cfg.host_p_n == 0
        tab = mask_keys(env)
        assert tab["sizes"] == {"a": 50, "p": want_p}


def test_large_tax_planners_still_build_with_and_without_foreign_subspaces():
    """The planner's mask is not bounded by AIE_MAX_MASK (nothing on its side is sized by it): 16 brackets x 51 rates
    (multi-action: 16 x 52 = 832 entries) and 12 x 51 single-action (613) build as they always did, also with a foreign
    planner subspace beside them; only the foreign part is bounded."""
    import ctypes

    from helpers import C2
    from ai_economist_amd import _build, _cabi

    register_toys()
    lib = _cabi.bind(ctypes.CDLL(_build.build()))
    comps = [list(c) for c in C2["components"]]
    for nb, multi, want_mp in ((16, True, 16 * 52), (12, False, 1 + 12 * 51), (16, False, 1 + 16 * 51)):
        tax = ["PeriodicBracketTax", dict(bracket_spacing="linear", n_brackets=nb, top_bracket_cutoff=150, rate_disc=0.02)]
        for extra, foreign in (([], 0), ([["Stimulus", {}]], 4 + (1 if multi else 0))):
            env = make_env(dict(C2, components=comps[:3] + [tax] + extra, multi_action_mode_planner=multi))
            cfg = env.build_config()
            assert (cfg.tax_n_brackets, cfg.tax_n_disc_rates, cfg.host_p_n) == (nb, 51, len(extra))
            assert lib.aie_arena_bytes(ctypes.byref(cfg)) > 0, lib.aie_last_error(None)
            from ai_economist_amd.foundation.obs_keys import mask_keys

            assert mask_keys(env)["sizes"]["p"] == want_mp + foreign
    # a foreign planner subspace past the bound is refused on its own account
    cfg = env.build_config()
    cfg.host_p_n = 2  # (each within the per-subspace bound, together past it)
    cfg.host_p_dim[0], cfg.host_p_dim[1] = _cabi.MAX_MASK, 4
    cfg.host_p_before[1] = cfg.host_p_before[0]
    assert lib.aie_arena_bytes(ctypes.byref(cfg)) == _cabi.E_INVALID
    assert b"planner action mask too long" in lib.aie_last_error(None)


def test_mirrored_limits_equal_the_headers():
    """_cabi.MAX_MASK / MAX_SUBSPACES / MAX_HOST_SUBSPACES are hand-kept copies of header constants that
    aie_sizeof_config does not cover."""
    import re

    from helpers import ROOT
    from ai_economist_amd import _cabi

    text = open(os.path.join(ROOT, "ai-economist_amd", "csrc", "aie_layout.h")).read() + open(os.path.join(ROOT, "include", "aie.h")).read()

    def define(name):
        return int(re.search(r"#define %s (\d+)" % name, text).group(1))

    assert _cabi.MAX_MASK == define("AIE_MAX_MASK")
    assert _cabi.MAX_SUBSPACES == define("AIE_MAX_SUBSPACES")
    assert _cabi.MAX_HOST_SUBSPACES == define("AIE_MAX_HOST_SUBSPACES")
    assert _cabi.ABI_VERSION == define("AIE_ABI_VERSION")


# ---------------------------------------------------------------- GPU: the fixtures, step by step

def _replica(be, e):
    out = {}
    for k, t in be.tensors.items():
        if t.shape[0] != be.E:
            continue
        v = t[e].cpu().numpy()
        out[k] = v.view(np.uint32) if k == "mt" else v
    return out


def _obs_check(obs, g, k, where, e):
    """The observation dict env.reset() / env.step() returned against the fixture's: integer tensors and the action
    masks exact, the flat vectors within OBS_TOL."""
    for name in [x for x in g.keys() if x.startswith("ob_")]:
        who, key = name[3:].split("_", 2)[1], name[3:].split("_", 2)[2]  # ob_obs_a_flat -> a, flat
        want = g[name][k]
        got = obs[who][key][e].cpu().numpy()
        assert got.shape == want.shape, "%s: obs %s shape %s vs %s" % (where, name, got.shape, want.shape)
        if want.dtype.kind in "iu" or key == "action_mask":
            assert np.array_equal(got, want), "%s: obs %s differs\n got=%s\nwant=%s" % (where, name, got, want)
        else:
            np.testing.assert_allclose(got, want, rtol=OBS_TOL, atol=OBS_TOL, err_msg="%s: obs %s" % (where, name))


def _batch_actions(g, t, E, env):
    """Replicas 0 and 2 take the fixture's actions of step t, replica 1 something else (in range)."""
    import torch

    names_a, names_p = env.action_subspace_names()
    a_fix = g["actions_a"][t]
    a = np.zeros((E,) + a_fix.shape, np.int32)
    a[0] = a[2] = a_fix
    if a_fix.ndim == 1:
        a[1] = (a_fix * 7 + t) % (1 + sum(k for _, k in names_a))
    else:
        a[1] = (a_fix * 3 + t) % (np.array([k for _, k in names_a]) + 1)
    act = {"a": torch.as_tensor(a, device="cuda:0")}
    if g["actions_p"].shape[1]:
        p_fix = g["actions_p"][t]
        p = np.zeros((E, p_fix.shape[0]), np.int32)
        p[0] = p[2] = p_fix
        if env.multi_action_mode_planner:
            p[1] = (p_fix * 5 + t) % (np.array([k for _, k in names_p]) + 1)
        else:
            p[1] = (p_fix * 5 + t) % (1 + sum(k for _, k in names_p))
        act["p"] = torch.as_tensor(p, device="cuda:0")
    return act


def _follow(name, on_obs=None, **extra):
    """Steps a 3-replica environment through the fixture (the procedure of tests/test_batched_component.py)."""
    register_toys()
    g = load_acting(name)
    E = 3
    env = make_env(g["cfg"], n_envs=E, device="cuda:0", **extra)
    assert [c.name for c in env.components] == [c[0] for c in g["cfg"]["components"]]
    be = env.backend
    be.set_rng_state(np.stack([g["pre_reset_mt"]] * E), np.full(E, int(g["pre_reset_pos"]), np.int32))
    obs = env.reset()
    for e in (0, 2):
        compare_state(_replica(be, e), state_from_golden(g, "s0_"), where="%s reset replica %d" % (name, e))
    obs_steps = list(g["obs_steps"])
    assert 0 in obs_steps
    (on_obs or _obs_check)(obs, g, obs_steps.index(0), name + " reset obs", 2)
    resets = {int(t): i for i, t in enumerate(g.get("reset_at", []))}
    for t in range(g["actions_a"].shape[0]):
        obs, rew, done, _ = env.step(_batch_actions(g, t, E, env))
        want = state_from_golden(g, "st_", t)
        for e in (0, 2):
            got = _replica(be, e)
            where = "%s step %d replica %d" % (name, t + 1, e)
            compare_state(got, want, where=where)
            assert zlib.crc32(got["mt"].tobytes()) == int(g["st_mt_crc"][t]), where
            if g["host_a"].shape[-1]:
                assert np.array_equal(got["host_actions_a"], g["host_a"][t]), where
            if g["host_p"].shape[-1]:
                assert np.array_equal(got["host_actions_p"], g["host_p"][t]), where
            r = np.concatenate([got["rewards_a"], got["rewards_p"][None]])
            np.testing.assert_allclose(r, g["rew"][t], rtol=2e-7, atol=REW_TOL, err_msg=where)
            assert int(got["done"]) == int(g["done"][t]), where
            assert int(got["error_flags"]) == 0, where
        if (t + 1) in obs_steps:
            (on_obs or _obs_check)(obs, g, obs_steps.index(t + 1), "%s step %d" % (name, t + 1), 2)
        if (t + 1) in resets:
            obs = env.reset(be.tensors["done"])  # (replica 1 shares the clock: its episode ends with the others')
            compare_state(_replica(be, 0), state_from_golden(g, "rs_", resets[t + 1]), where="%s reset after step %d" % (name, t + 1))
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("name", acting_names())
def test_acting_components_match_the_reference_with_the_same_components(name):
    env = _follow(name)
    t = env.backend.tensors
    g = load_acting(name)
    assert ("host_actions_a" in t) == bool(g["host_a"].shape[-1]) and ("host_actions_p" in t) == bool(g["host_p"].shape[-1])
    assert env.backend.lib.aie_step_kernel_instance(env.backend.handle) == -1  # (the full-featured kernel, no instance)


@pytest.mark.gpu
@pytest.mark.parametrize("name", acting_names())
def test_unflattened_masks_have_the_reference_keys_and_values(name):
    """flatten_masks=False: obs[...]["action_mask"] is the reference's dictionary {"<Component>[.<sub>]": mask}."""
    seen = []

    def check(obs, g, k, where, e):
        ref = g["masks"][k]
        ma, mp = obs["a"]["action_mask"], obs["p"]["action_mask"]
        assert sorted(ma.keys()) == sorted(ref["0"].keys()), where  # (a dictionary: the key set)
        assert sorted(mp.keys()) == sorted(ref["p"].keys()), where
        for key, m in ma.items():
            want = np.array([ref[str(i)][key] for i in range(m.shape[1])], np.float32)
            assert np.array_equal(m[e].cpu().numpy(), want), "%s: agents' mask %s" % (where, key)
        for key, m in mp.items():
            assert np.array_equal(m[e].cpu().numpy(), np.array(ref["p"][key], np.float32)), "%s: planner's mask %s" % (where, key)
        seen.append(k)

    _follow(name, on_obs=check, flatten_masks=False)
    assert len(seen) == len(load_acting(name)["obs_steps"])


@pytest.mark.gpu
def test_out_of_range_foreign_index_raises_the_flag_and_is_a_noop():
    import torch

    register_toys()
    # single-action agents: the index one past the action space; replica 1 sends NO-OPs
    g = load_acting("acting_tithe_mid_4ag")
    env = make_env(g["cfg"], n_envs=2, device="cuda:0")
    env.seed(3)
    env.reset()
    be = env.backend
    A = 1 + sum(k for _, k in env.action_subspace_names()[0])
    a = torch.zeros((2, 4), dtype=torch.int32, device="cuda:0")
    a[0, 1] = A
    a[0, 2] = -1
    env.step({"a": a})
    assert be.tensors["error_flags"].tolist() == [1, 0]
    assert int(be.tensors["host_actions_a"].abs().sum()) == 0
    with pytest.raises(ValueError, match="agent action index"):
        env.check_errors()
    # multi-action agents: a foreign column past its dimension decodes to NO-OP, the other columns still count
    g = load_acting("acting_regimen_first_multi_5ag")
    env = make_env(g["cfg"], n_envs=2, device="cuda:0")
    env.seed(3)
    env.reset()
    be = env.backend
    names = [nm for nm, _ in env.action_subspace_names()[0]]
    a = torch.zeros((2, 5, len(names)), dtype=torch.int32, device="cuda:0")
    a[0, 0, names.index("Regimen.train")] = 3   # (2 choices)
    a[0, 0, names.index("Regimen.rest")] = 1
    a[1, 0, names.index("Regimen.train")] = 2
    coin0 = be.tensors["inv_coin"].clone()
    env.step({"a": a})
    assert be.tensors["error_flags"].tolist() == [1, 0]
    ha = be.tensors["host_actions_a"]
    assert ha[0, 0].tolist() == [1, 0] and ha[1, 0].tolist() == [0, 2]
    assert float(be.tensors["inv_coin"][0, 0]) == float(coin0[0, 0])      # the out-of-range "train" did nothing
    assert float(be.tensors["inv_coin"][1, 0]) == float(coin0[1, 0]) - 2  # the valid one paid 2 coin
    # the planner, both modes
    for name in ("acting_stimulus_behind_multi_4ag", "acting_stimulus_ahead_single_10ag"):
        g = load_acting(name)
        env = make_env(g["cfg"], n_envs=2, device="cuda:0")
        env.seed(3)
        env.reset()
        be = env.backend
        names_p = env.action_subspace_names()[1]
        if env.multi_action_mode_planner:
            p = torch.zeros((2, len(names_p)), dtype=torch.int32, device="cuda:0")
            p[0, [nm for nm, _ in names_p].index("Stimulus")] = 5  # (4 choices)
        else:
            p = torch.zeros((2, 1), dtype=torch.int32, device="cuda:0")
            p[0, 0] = 1 + sum(k for _, k in names_p)
        env.step({"p": p})
        assert be.tensors["error_flags"].tolist() == [2, 0], name
        assert be.tensors["host_actions_p"].tolist() == [[0], [0]], name
        with pytest.raises(ValueError, match="planner action index"):
            env.check_errors()


def _mask_rows(env):
    """[(who, slot within the replica's agent / planner columns, offset, length)] of the sampler's rows per actor."""
    from ai_economist_amd.foundation.obs_keys import mask_keys

    tab = mask_keys(env)
    rows = {}
    for who, multi in (("a", env.multi_action_mode_agents), ("p", env.multi_action_mode_planner)):
        if multi and tab[who]:
            rows[who] = [(off - 1, size + 1) for _, off, size in tab[who]]  # each with its own NO-OP entry in front
        else:
            rows[who] = [(0, tab["sizes"][who])]
    return rows, tab


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["acting_tithe_mid_4ag", "acting_regimen_first_multi_5ag", "acting_stimulus_ahead_single_10ag",
                                  "acting_tithe_only_4ag"])
def test_masked_sampler_respects_the_components_masks(name):
    """aie_sample_masked_actions reads the arena's mask tensors, which carry the host components' entries: over an
    episode of its own actions it never returns a forbidden entry, stays in range, and does pick foreign entries."""
    import torch

    register_toys()
    g = load_acting(name)
    E = 64
    # (2 coin to start with: Tithe's third choice and, with no labor yet, Regimen's rest are forbidden from the reset on)
    env = make_env(dict(g["cfg"], starting_agent_coin=2), n_envs=E, device="cuda:0")
    env.seed(11)
    obs = env.reset()
    be = env.backend
    rows, tab = _mask_rows(env)
    foreign = {who: [(off, size) for key, off, size in tab[who] if key.split(".")[0] in ("Tithe", "Regimen", "Stimulus")] for who in "ap"}
    picked, forbidden_seen = 0, 0
    for t in range(int(g["cfg"]["episode_length"]) - 1):
        ma, mp = be.tensors["obs_a_action_mask"].clone(), be.tensors["obs_p_action_mask"].clone()
        a, p = be.sample_masked_actions(seed=77, slot=t & 1)
        torch.cuda.synchronize()
        for who, act, mask in (("a", a, ma), ("p", p, mp)):
            for s, (lo, ln) in enumerate(rows[who]):
                v = act[..., s].long()
                assert int(v.min()) >= 0 and int(v.max()) < ln, (name, t, who, s)
                assert bool((mask.gather(-1, (lo + v).unsqueeze(-1)) > 0.5).all()), (name, t, who, s)
                multi = env.multi_action_mode_agents if who == "a" else env.multi_action_mode_planner
                for off, size in foreign[who]:
                    if multi and off - 1 == lo:
                        picked += int((v > 0).sum())
                    elif not multi:
                        picked += int(((v >= off) & (v < off + size)).sum())
            for off, size in foreign[who]:
                forbidden_seen += int((mask.narrow(-1, off, size) < 0.5).sum())
        obs, _, _, _ = env.step({"a": a, "p": p})
    assert picked > 0 and forbidden_seen > 0  # the check above met both allowed and forbidden foreign entries
    assert not bool(be.tensors["error_flags"].any())


@pytest.mark.gpu
def test_samplers_refuse_a_multi_action_planner_with_rows_of_different_lengths():
    register_toys()
    g = load_acting("acting_stimulus_behind_multi_4ag")  # tax rows of 1 + 21 entries, the Stimulus row of 1 + 4
    env = make_env(g["cfg"], n_envs=4, device="cuda:0")
    env.seed(2)
    env.reset()
    be = env.backend
    import torch

    for call in (lambda: be.sample_masked_actions(seed=1), lambda: be.sample_random_actions(seed=1),
                 lambda: be.sample_policy_actions(torch.zeros_like(be.tensors["obs_a_action_mask"]),
                                                  torch.zeros_like(be.tensors["obs_p_action_mask"]), seed=1)):
        with pytest.raises(NotImplementedError, match="multi-action planner"):
            call()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["acting_tithe_mid_4ag", "acting_regimen_first_multi_5ag", "acting_stimulus_ahead_single_10ag"])
def test_policy_sampler_equals_its_python_transcription_on_rows_with_foreign_entries(name):
    import torch

    from helpers import counter_rng, sampler_entry_rng, sampler_pick_row

    register_toys()
    g = load_acting(name)
    E = 3
    env = make_env(g["cfg"], n_envs=E, device="cuda:0", env_offset=20)
    env.seed(4)
    env.reset()
    be = env.backend
    n = env.n_agents
    rows, _ = _mask_rows(env)
    wa, wp = len(rows["a"]), len(rows["p"])
    per_env = n * wa + wp
    gen = torch.Generator(device="cpu").manual_seed(9)
    nonzero = 0
    for t in range(3):
        ma, mp = be.tensors["obs_a_action_mask"].cpu().numpy(), be.tensors["obs_p_action_mask"].cpu().numpy()
        la = (torch.randn(ma.shape, generator=gen) * 2).float()
        lp = (torch.randn(mp.shape, generator=gen) * 2).float()
        a, p = be.sample_policy_actions(la.to("cuda:0"), lp.to("cuda:0"), seed=31, env_offset=20)
        torch.cuda.synchronize()
        assert int(be.tensors["sample_t"][0]) == t + 1
        for e in range(E):
            base = counter_rng(31, 20 + e, t, per_env)
            for i in range(n):
                for s, (lo, ln) in enumerate(rows["a"]):
                    want = sampler_pick_row(la[e, i, lo:lo + ln].numpy(), ma[e, i, lo:lo + ln], sampler_entry_rng(base, i * wa + s))
                    assert int(a[e, i, s]) == want, (name, t, e, i, s)
            for s, (lo, ln) in enumerate(rows["p"]):
                want = sampler_pick_row(lp[e, lo:lo + ln].numpy(), mp[e, lo:lo + ln], sampler_entry_rng(base, n * wa + s))
                assert int(p[e, s]) == want, (name, t, e, s)
        nonzero += int((a != 0).sum())
        env.step({"a": a, "p": p})
    assert nonzero > 0


@pytest.mark.gpu
def test_masked_reset_of_an_acting_environment_touches_only_its_rows():
    """The twin method of tests/test_batched_component.py on an acting case: S resets a mask's replicas at step k, F all of
    them, N none; outside the mask S equals N, inside it F -- every tensor (host_actions_* and the mask tensors with the
    components' entries included) and every observation, bit for bit."""
    import torch

    from test_batched_component import TWIN_E, _twin_actions, _twin_assert, _twin_masks, _twin_snapshot

    register_toys()
    name = "acting_tithe_mid_4ag"
    cfg = load_acting(name)["cfg"]
    E, k = TWIN_E, 12  # (tax period 8, episode length 24: the middle of the second period)
    masks = _twin_masks(E)

    def build():
        env = make_env(cfg, n_envs=E, device="cuda:0")
        env.seed(17)
        return env

    S = {m: build() for m in masks}
    N, F = build(), build()
    envs = list(S.values()) + [N, F]
    snap = {id(env): _twin_snapshot(env, env.reset()) for env in envs}
    rng = np.random.RandomState(1000 + k)

    def check(where):
        for m, rows in masks.items():
            s = snap[id(S[m])]
            _twin_assert(s, snap[id(N)], [e for e in range(E) if e not in rows], "%s: mask %s, outside vs no reset" % (where, m))
            _twin_assert(s, snap[id(F)], rows, "%s: mask %s, inside vs full reset" % (where, m))

    for t in range(1, 24 + 8 + 1):
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
        reset_any = False
        for env in envs:
            done = env.backend.tensors["done"]
            if bool(done.any().item()):
                snap[id(env)] = _twin_snapshot(env, env.reset(done))
                reset_any = True
        if reset_any:
            check("%s reset(done) after step %d" % (name, t))
    assert int(N.backend.tensors["completions"].min()) >= 1
    assert "host_actions_a" in snap[id(N)]
