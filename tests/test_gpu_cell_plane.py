"""GPU tests (pytest -m gpu): the cells' byte plane (`cells_packed`, csrc/aie_layout.h: o_cells8) that a step reads on its
way in instead of the cell words.  The invariant -- wherever `obs_valid` != 0 the plane is the packing of `cells` -- after
a reset and after every step, on a compile-time instance and on the generic kernel, step by step against the CPU oracle
(tests/test_gpu_parity.py: _compare_all); a plane that something outside the kernels spoiled; a step that changes more
cells than its change log holds; split steps; and a configuration the byte cannot hold (8 agents), which has no plane.

Shapes: H W no multiple of 4 (5 x 5: one word arrives with the next field's unit), no multiple of 16 (6 x 6), more plane
dwords than the two waves' 128 lanes with a partial last group (23 x 23, 25 x 25); 5 replicas (workgroup b is replica b)
and 16 (the XCD remap); 2, 4 and 7 agents (owner field 1 ... 7)."""
import numpy as np
import pytest

from helpers import C2, make_env, oracle_host_pre_reset
from test_gpu_parity import _compare_all

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AIE_DIRTY_CAP = 64  # csrc/aie_device.h


def _uniform(h, w, n, **kw):
    cfg = dict(scenario_name="uniform/simple_wood_and_stone", n_agents=n, world_size=[h, w], episode_length=100,
               components=[["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 3, "order_duration": 15}],
                           ["Gather", {}], ["PeriodicBracketTax", {"period": 7}]],
               starting_agent_coin=5, starting_wood_coverage=0.15, starting_stone_coverage=0.15,
               wood_regen_weight=0.3, stone_regen_weight=0.3)
    cfg.update(kw)
    return cfg


# name: (configuration, replicas, kernel)
CASES = {
    "5x5_n2_e5_generic": (_uniform(5, 5, 2), 5, "generic"),
    "6x6_n7_e16_generic": (_uniform(6, 6, 7), 16, "generic"),
    "23x23_n4_e5_generic": (_uniform(23, 23, 4, starting_wood_coverage=0.05, starting_stone_coverage=0.05), 5, "generic"),
    "25x25_n4_e16_instance": (dict(C2, episode_length=100, resource_regen_prob=0.1), 16, "instance"),
    "25x25_n4_e5_generic": (dict(C2, episode_length=100, resource_regen_prob=0.1), 5, "generic"),
}


def pack(cells):
    """csrc/aie_layout.h: aie_cell_pack8, on the uint32 cell words."""
    c = np.asarray(cells).astype(np.uint32)
    owner = (((c >> 16) & 0xff) + 1) & 7
    return (((c >> 24) & 7) | ((c & 1) << 3) | (((c >> 8) & 1) << 4) | (owner << 5)).astype(np.uint8)


def _plane_holds(be, where, everywhere=True):
    """The invariant; `everywhere`: obs_valid is also expected to be set for every replica."""
    valid = be.tensors["obs_valid"].cpu().numpy() != 0
    if everywhere:
        assert valid.all(), "%s: obs_valid %s" % (where, valid)
    got = be.tensors["cells_packed"].cpu().numpy()
    want = pack(be.tensors["cells"].cpu().numpy().view(np.uint32))
    bad = (got != want).reshape(len(valid), -1).any(1) & valid
    assert not bad.any(), "%s: cells_packed is not the packing of cells in replicas %s" % (where, np.nonzero(bad)[0])


def _pair(cfg, E, kernel, seed):
    from oracle_lib import OracleEnv

    env = make_env(cfg, n_envs=E, device=DEV)
    be = env.backend
    if kernel == "generic":
        assert be.lib.aie_select_step_kernel(be.handle, 1) == 0
    env.seed(seed)
    env.reset()
    oracle = OracleEnv(env.build_config(), env.layout_planes())
    oracle.seed(seed)
    oracle_host_pre_reset(env, oracle)
    oracle.reset()
    inst = be.lib.aie_step_kernel_instance(be.handle)
    assert (inst >= 0) == (kernel == "instance"), inst
    return env, be, oracle


def _step_both(env, be, oracle, seed, where):
    import torch

    a, p = be.sample_random_actions(seed=seed)
    env.step({"a": a, "p": p})
    torch.cuda.synchronize()
    oracle.step(a.cpu().numpy(), p.cpu().numpy())
    _compare_all(be, oracle, where)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plane_follows_the_cells_step_by_step(name):
    """Reset, 60 random-policy steps, then houses of every owner index loaded on both sides and 12 more steps: the state
    equals the oracle's and the plane the packing of the cells after each of them."""
    cfg, E, kernel = CASES[name]
    n, (H, W) = cfg["n_agents"], cfg["world_size"]
    env, be, oracle = _pair(cfg, E, kernel, seed=23)
    assert tuple(be.tensors["cells_packed"].shape) == (E, H, W)
    _compare_all(be, oracle, name + " reset")
    _plane_holds(be, name + " reset")
    for t in range(60):
        _step_both(env, be, oracle, 7, "%s step %d" % (name, t + 1))
        _plane_holds(be, "%s step %d" % (name, t + 1))
    # a house of every owner on cells that are free in every replica's state (no resource, no source, no water, no house,
    # nobody standing there)
    rs = np.random.RandomState(5)
    for e in range(E):
        t = oracle.t
        free = (t["stone"][e] == 0) & (t["wood"][e] == 0) & (t["cell_flags"][e] == 0) & (t["house_owner"][e] < 0)
        free[t["loc_r"][e], t["loc_c"][e]] = False
        spots = np.argwhere(free)
        assert len(spots) >= n, (name, e, len(spots))
        owner = np.array(t["house_owner"][e])
        for k, q in enumerate(rs.permutation(len(spots))[: min(len(spots), 2 * n)]):
            owner[tuple(spots[q])] = k % n
        be.load_state({"house_owner": owner}, e=e)
        oracle.load_state({"house_owner": owner}, e=e)
    assert not (be.tensors["obs_valid"].cpu().numpy() != 0).any()  # (load_state invalidates: the next step reads the words)
    for t in range(12):
        _step_both(env, be, oracle, 9, "%s loaded, step %d" % (name, t + 1))
        _plane_holds(be, "%s loaded, step %d" % (name, t + 1))
    owners = be.tensors["house_owner"].cpu().numpy()
    assert set(range(n)) <= set(np.unique(owners).tolist()), np.unique(owners)
    assert int(be.tensors["error_flags"].abs().sum()) == 0


def test_eight_agents_have_no_plane():
    """The owner field holds seven agents: with eight the record has no plane and the kernels step as before."""
    env, be, oracle = _pair(_uniform(6, 6, 8), 5, "generic", seed=3)
    assert "cells_packed" not in be.tensors and "cells_packed" not in oracle.t
    _compare_all(be, oracle, "reset")
    for t in range(20):
        _step_both(env, be, oracle, 7, "8 agents step %d" % (t + 1))


@pytest.mark.parametrize("name", ["25x25_n4_e16_instance", "23x23_n4_e5_generic"])
def test_poisoned_plane_is_not_read_and_is_healed(name):
    """cells_packed := 0xff with the observations invalidated: the step takes the words, equals the oracle and leaves a
    correct plane; the steps behind it read that plane."""
    cfg, E, kernel = CASES[name]
    env, be, oracle = _pair(cfg, E, kernel, seed=31)
    for t in range(5):
        _step_both(env, be, oracle, 7, "%s step %d" % (name, t + 1))
    be.tensors["cells_packed"].fill_(0xff)
    be.invalidate_observations()
    for t in range(5, 10):
        _step_both(env, be, oracle, 7, "%s poisoned, step %d" % (name, t + 1))
        _plane_holds(be, "%s poisoned, step %d" % (name, t + 1))


def test_change_log_overflow_writes_the_whole_plane():
    """25 x 25 quadrant layout, regen_weight 1, every source emptied by upload: one step respawns more cells than
    AIE_DIRTY_CAP.  Once as the upload leaves it (observations invalidated: the words are read), once with the plane and
    obs_valid uploaded to match the emptied cells, so that the step reads the plane and its change log overflows."""
    cfg = dict(_uniform(25, 25, 4, starting_wood_coverage=0.08, starting_stone_coverage=0.08, wood_regen_weight=1.0,
                        stone_regen_weight=1.0), scenario_name="quadrant/simple_wood_and_stone")
    E = 16
    env, be, oracle = _pair(cfg, E, "generic", seed=11)
    for t in range(3):
        _step_both(env, be, oracle, 7, "overflow step %d" % (t + 1))
    for matched in (False, True):
        for k in ("stone", "wood"):
            be.upload(k, np.zeros_like(oracle.t[k]))
            oracle.t[k][...] = 0
        if matched:
            be.upload("cells_packed", pack(be.download("cells").view(np.uint32)))
            be.upload("obs_valid", np.ones(E, np.int32))
            assert (be.tensors["obs_valid"].cpu().numpy() == 1).all()
        where = "overflow, plane %s" % ("matched" if matched else "stale")
        _step_both(env, be, oracle, 7, where)
        _plane_holds(be, where)
        respawned = int((oracle.t["stone"][0] != 0).sum() + (oracle.t["wood"][0] != 0).sum())
        assert respawned > AIE_DIRTY_CAP, respawned
        _step_both(env, be, oracle, 7, where + ", next step")
        _plane_holds(be, where + ", next step")


@pytest.mark.parametrize("name", ["25x25_n4_e16_instance", "6x6_n7_e16_generic"])
def test_split_steps_keep_the_invariant(name):
    """aie_step_range: the head (components), then the tail.  The head leaves obs_valid == 0 (nothing to hold); the tail
    reads the words and sets it, and the plane is right again; now and then a whole step reads that plane."""
    import torch

    from ai_economist_amd import _cabi

    cfg, E, _ = CASES[name]
    env, be, oracle = _pair(cfg, E, "instance" if "instance" in name else "generic", seed=17)
    nc = len(cfg["components"])
    for t in range(20):
        a, p = be.sample_random_actions(seed=7)
        where = "%s split step %d" % (name, t + 1)
        if t % 4 == 3:
            be.step(a, p)
        else:
            be.step_range(a, p, 0, nc, _cabi.STEP_HEAD)
            _plane_holds(be, where + " head", everywhere=False)
            be.step_range(a, p, nc, nc, _cabi.STEP_TAIL)
        torch.cuda.synchronize()
        oracle.step(a.cpu().numpy(), p.cpu().numpy())
        _compare_all(be, oracle, where)
        _plane_holds(be, where)
