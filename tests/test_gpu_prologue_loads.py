"""GPU tests (pytest -m gpu): the gather-trade-build step kernel's way in, up to the barrier behind which the record is in
LDS (csrc/aie_kernels.hip: step_body, barrier (2)).  Each wave requests what it fetches there before it waits for any of
it: the first its action words, its unit of the record and its dwords of the cells' byte plane (without the plane: its
first three units), the second its unit, the constant tables and the rows of the generator's state that the draw window
covers.  Which rows those are -- one, two or three, cut at word 623, or none (the components twist at their first draw)
-- depends on the generator's position alone.  So every replica is put at each of the positions below in turn
(aie_set_rng_state) and stepped three times under a
scripted policy that walks, gathers and builds, on a compile-time instance with and without the cells' byte plane, on an
instance without tax table and auction, and on the generic kernel; after each step the whole arena equals the CPU
oracle's (tests/test_gpu_parity.py: _compare_all -- record fields, generator key and position, observations, masks,
rewards, done).

aie_set_rng_state writes record fields and so invalidates the observations: the step behind it would read the cell words
and rewrite every observation.  The cases here put obs_valid back (the generator shows in no observation), so that the
steps take the everyday path: the plane on the way in, observations in place.  The stale path has cases of its own."""
import numpy as np
import pytest

import rich_states as R
from helpers import C1_INSTANCE, C2, make_env, oracle_host_pre_reset
from test_gpu_parity import _compare_all

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# draw window of 128 words (csrc/aie_device.h: stage_window_words, up to 16 agents), 64 words per row of the state:
#   0, 64, 448, 512        the window starts a row: two rows
#   1, 63, 447, 511        three rows (447 + 128 = 575 ends row 8; 511 would reach 638: cut at word 623)
#   496, 497               the cut itself: 496 + 128 = 624 fits, 497 loses a word
#   560, 575               rows 8 and 9, cut (575: one word of row 8)
#   576, 600, 623          the last row alone, 48 words long; 623: a single word
#   624                    nothing to fetch: the first draw twists
POSITIONS = (0, 1, 63, 64, 447, 448, 496, 497, 511, 512, 560, 575, 576, 600, 623, 624)
WARMUP = 40  # policy steps ahead of the first position: inventories to build from, agents apart

# name: (configuration, replicas, kernel)
CASES = {
    "c2_e16_instance": (dict(C2), 16, "instance"),
    "c2_e9_instance": (dict(C2), 9, "instance"),  # (9 is no multiple of 8: workgroup b is replica b)
    "c2_n10_e16_instance": (dict(C2, n_agents=10), 16, "instance"),  # (no plane: the owner field holds 7 agents)
    "build_gather_e16_instance": (dict(C1_INSTANCE), 16, "instance"),  # (no tax table, no auction)
    "c2_e16_generic": (dict(C2), 16, "generic"),
}


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
    if kernel is not None:
        assert (inst >= 0) == (kernel == "instance"), inst
    return env, be, oracle, R.Info(env)


def _run(env, o, info, seed, positions, on_position, on_step, policy):
    """The run on the oracle (the device follows through the hooks): WARMUP policy steps, then every position in turn,
    three policy steps each.  Returns (agents that gathered, agents that built) behind the warm-up, as sets of (e, i)."""
    gathered, built = set(), set()
    t = 0

    def step(where, count):
        nonlocal t
        a, p = R.policy_actions(policy, env, o.t["obs_a_action_mask"], o.t["obs_p_action_mask"], seed, t, info)
        inv, houses = o.t["inv_res"].copy(), o.t["house_owner"].copy()
        o.step(a, p)
        t += 1
        if count:
            for e, i in zip(*np.nonzero((o.t["inv_res"] > inv).any(1))):
                gathered.add((int(e), int(i)))
            for e, r, c in zip(*np.nonzero(o.t["house_owner"] != houses)):
                built.add((int(e), int(o.t["house_owner"][e, r, c])))
        if on_step is not None:
            on_step(a, p, where)

    for k in range(WARMUP):
        step("warm-up step %d" % (k + 1), False)
    for pos in positions:
        o.t["mt_pos"][...] = pos
        o.t["mt_has_gauss"][...] = 0
        o.t["mt_gauss"][...] = 0
        if on_position is not None:
            on_position(pos)
        for k in range(3):
            step("position %d, step %d" % (pos, k + 1), True)
    assert not o.t["error_flags"].any()
    return gathered, built


def _device_run(name, cfg, E, kernel, positions, stale=False, policy="builder", seed=29):
    import torch

    env, be, oracle, info = _pair(cfg, E, kernel, seed)
    _compare_all(be, oracle, name + " reset")

    def on_position(pos):
        be.set_rng_state(oracle.t["mt"], np.full(E, pos, np.int32))
        if stale:  # something outside the kernels wrote the cells: the step reads the words, not the plane
            be.upload("cells", be.download("cells"))
            assert not (be.tensors["obs_valid"].cpu().numpy() != 0).any()
        else:
            be.upload("obs_valid", np.ones(E, np.int32))
            assert (be.tensors["obs_valid"].cpu().numpy() == 1).all()
        assert (be.tensors["mt_pos"].cpu().numpy() == pos).all()

    def on_step(a, p, where):
        env.step({"a": torch.as_tensor(a, device=DEV), "p": torch.as_tensor(p, device=DEV)})
        torch.cuda.synchronize()
        _compare_all(be, oracle, "%s %s" % (name, where))

    gathered, built = _run(env, oracle, info, seed, positions, on_position, on_step, policy)
    assert int(be.tensors["error_flags"].abs().sum()) == 0
    return gathered, built


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_window_shape_matches_the_oracle(name):
    """Each position of POSITIONS, three steps each, the arena against the oracle after every step; over the run several
    agents gather and several build."""
    cfg, E, kernel = CASES[name]
    gathered, built = _device_run(name, cfg, E, kernel, POSITIONS)
    assert len(gathered) >= 4 and len(built) >= 4, (len(gathered), len(built))


@pytest.mark.parametrize("name", ["c2_e16_instance", "c2_e9_instance", "c2_e16_generic"])
def test_stale_state_steps_match_the_oracle(name):
    """obs_valid == 0 behind an upload of `cells`: both waves fetch the cell words behind barrier (2), over what the
    plane gave.  A full window, a single row and the empty window."""
    cfg, E, kernel = CASES[name]
    _device_run(name + " stale", cfg, E, kernel, (0, 575, 624), stale=True)


@pytest.mark.parametrize("kernel", [None, "generic"])
def test_multi_action_words_match_the_oracle(kernel):
    """Multi-action agents (a word per subspace and agent) and a multi-action planner (a word per bracket) at position
    600: the first wave's action words beside a window that is cut at word 623."""
    cfg = dict(C2, multi_action_mode_agents=True, multi_action_mode_planner=True)
    _device_run("multi-action, %s kernel" % (kernel or "default"), cfg, 16, kernel, (600,), policy="mix")
