"""GPU tests (pytest -m gpu): the gather-trade-build step kernel's way out (csrc/aie_gtb_state.h: store_record_step,
csrc/aie_device.h: store_generator_rows).  The 16-byte units of the record image and the listed cells leave behind the
last barrier; where the regeneration left the generator's rows in its LDS window they leave as 156 16-byte
write-through units through a descriptor that ends with word 623, everywhere else as ten dwords per lane.  What can go
wrong is a unit too many or too few, rows taken from a window that does not hold the final state, or bytes behind word
623 (the source count and list, the cells' byte plane) overwritten.

So every case steps the device beside the CPU oracle and compares after EVERY step
  * the whole record: every field of the image, the generator's key and position (tests/test_gpu_parity.py:
    _compare_all) and the cell words with their flag bytes, bit for bit; the source count and list against the flag
    bytes and the byte plane against the cell words; the raw bytes between the key's last word and the plane against
    what they were before the step;
  * the observation tensors, rewards and done (_compare_all).
Each case runs at 5 replicas (workgroup b steps replica b), at 8 and at 16: replica_of_block (csrc/aie_device.h) spreads
a batch that is a multiple of 8 over the XCDs, which at 8 replicas is still the identity and at 16 the first
permutation."""
import contextlib

import numpy as np
import pytest

from helpers import C2, dev_library, make_env, oracle_host_pre_reset
from test_gpu_cell_plane import AIE_DIRTY_CAP, _uniform, pack
from test_gpu_parity import _compare_all, _expected_src_list

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPLICAS = (5, 8, 16)
AIE_SRC_CAP = 128  # csrc/aie_device.h
EXTRA = ("cells", "cell_flags", "error_flags")  # (source list and plane: against the flag bytes and the cells, Pair.check)

# 7 x 9, sources of both kinds, water, 4 H W = 252 words per step
TINY_LAYOUT = "W.S...W.S;.........;..@@@....;S.......W;.........;...W.S...;W.S...S.W"
TINY = dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=4, world_size=[7, 9], episode_length=100,
            components=[["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 3, "order_duration": 15}],
                        ["Gather", {}], ["PeriodicBracketTax", {"period": 7}]],
            starting_agent_coin=10, env_layout_file=TINY_LAYOUT, resource_regen_prob=0.2, mobile_agent_observation_range=2)
DENSE = dict(scenario_name="uniform/simple_wood_and_stone", n_agents=4, world_size=[20, 20], episode_length=100,
             components=[["Build", {}], ["Gather", {}]], starting_agent_coin=3, starting_stone_coverage=0.22,
             starting_wood_coverage=0.22, wood_regen_weight=0.3, stone_regen_weight=0.2)


class Pair:
    """A device environment and the oracle beside it, seeded alike and reset."""

    def __init__(self, cfg, E, seed, kernel=None, dev=False, **env_kw):
        from oracle_lib import OracleEnv

        with dev_library() if dev else contextlib.nullcontext():  # (the backend loads its library when it is created)
            self.env = make_env(cfg, n_envs=E, device=DEV, **env_kw)
            self.E, self.be = E, self.env.backend
            if kernel == "generic":
                assert self.be.lib.aie_select_step_kernel(self.be.handle, 1) == 0
            self.env.seed(seed)
            self.env.reset()
        self.oracle = OracleEnv(self.env.build_config(), self.env.layout_planes())
        self.oracle.seed(seed)
        oracle_host_pre_reset(self.env, self.oracle)
        self.oracle.reset()
        if kernel is not None:
            inst = self.be.lib.aie_step_kernel_instance(self.be.handle)
            assert (inst >= 0) == (kernel == "instance"), inst
        d = self.be.descs
        self.rec_bytes = int(d["mt"][2][0])  # (the records open the arena, one after the other)
        self.key_end = int(d["mt"][3]) + 4 * int(d["mt"][1][1])
        self.tail_end = int(d["cells_packed"][3]) if "cells_packed" in d else self.rec_bytes
        if "regen_src_n" in d:  # nothing between word 623 and the source count
            assert int(d["regen_src_n"][3]) == self.key_end and int(d["mt"][3]) % 16 == 0
        self.check("reset")

    def behind_the_key(self):
        rec = self.be.arena[: self.E * self.rec_bytes].view(self.E, self.rec_bytes)
        return rec[:, self.key_end: self.tail_end].cpu().numpy().copy()

    def check(self, where):
        be, o = self.be, self.oracle
        _compare_all(be, o, where)
        for k in EXTRA:
            if k in be.tensors and k in o.t:
                got, want = np.ascontiguousarray(be.tensors[k].cpu().numpy()), np.ascontiguousarray(o.t[k])
                assert got.dtype.itemsize == want.dtype.itemsize and got.shape == want.shape, (where, k)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), "%s: %s differs" % (where, k)
        if "cells_packed" in be.tensors:
            assert np.array_equal(be.tensors["cells_packed"].cpu().numpy(),
                                  pack(be.tensors["cells"].cpu().numpy().view(np.uint32))), "%s: the plane" % where
        if "regen_src_list" in be.tensors:
            flags = be.tensors["cell_flags"].reshape(self.E, -1).cpu().numpy()
            cap = int(be.tensors["regen_src_list"].shape[-1])
            got = be.tensors["regen_src_list"].cpu().numpy().view(np.uint16).astype(np.int64)
            for e in range(self.E):
                n, lst = _expected_src_list(flags[e], cap)
                assert int(be.tensors["regen_src_n"][e]) == n and np.array_equal(got[e], lst), (where, e)

    def step(self, seed, where):
        """One random-policy step on both sides; returns the words the components drew, modulo 624, per replica."""
        import torch

        before = self.behind_the_key()
        pos = self.oracle.t["mt_pos"].astype(np.int64).copy()
        a, p = self.be.sample_random_actions(seed=seed)
        self.be.step(a, p)
        torch.cuda.synchronize()
        self.oracle.step(a.cpu().numpy(), p.cpu().numpy())
        self.check(where)
        assert (self.be.tensors["obs_valid"].cpu().numpy() == 1).all(), where
        assert np.array_equal(self.behind_the_key(), before), "%s: bytes behind word 623 changed" % where
        H, W = self.env.world_size
        return (self.oracle.t["mt_pos"].astype(np.int64) - pos - 4 * H * W) % 624

    def set_position(self, pos):
        """Every replica's generator at word `pos` of its current state, the observations still valid."""
        o, be = self.oracle, self.be
        o.t["mt_pos"][...] = pos
        o.t["mt_has_gauss"][...] = 0
        o.t["mt_gauss"][...] = 0
        be.set_rng_state(o.t["mt"], np.full(self.E, pos, np.int32))
        be.upload("obs_valid", np.ones(self.E, np.int32))


def _twists(pos_before, pos_after, words):
    """How often a step that consumed `words` words from pos_before twisted (position 624: the next draw twists)."""
    return (pos_before + words - pos_after) // 624


@pytest.mark.parametrize("E", REPLICAS)
def test_headline_shape(E):
    """BASELINE configs[1] on its compile-time instance, 14 steps: 2500 regeneration words a step, four or five twists,
    the position wraps; the rows leave from the window."""
    pr = Pair(dict(C2), E, 3, kernel="instance")
    twists = set()
    for t in range(14):
        if t == 7:  # two words short of the state's end: five twists whatever the components draw
            pr.set_position(622)
        pos = pr.oracle.t["mt_pos"].astype(np.int64).copy()
        drawn = pr.step(11, "C2, %d replicas, step %d" % (E, t + 1))
        twists |= set(_twists(pos, pr.oracle.t["mt_pos"], 2500 + drawn).tolist())
    assert twists == {4, 5}, twists
    assert int(pr.be.tensors["error_flags"].abs().sum()) == 0


@pytest.mark.parametrize("E", REPLICAS)
def test_tiny_world(E):
    """7 x 9, fixed layout: 252 words a step, so a step twists once or not at all -- the window then holds rows no twist
    of this launch produced -- and a double's two words fall on either side of word 623."""
    pr = Pair(dict(TINY), E, 5)
    twists = set()
    for t in range(12):
        if t == 6:  # the regeneration starts on an odd word close to the end: the carried half-double
            pr.set_position(623 - 2 * 20)
        pos = pr.oracle.t["mt_pos"].astype(np.int64).copy()
        drawn = pr.step(13, "7x9, %d replicas, step %d" % (E, t + 1))
        twists |= set(_twists(pos, pr.oracle.t["mt_pos"], 252 + drawn).tolist())
    assert twists == {0, 1}, twists


@pytest.mark.parametrize("E", REPLICAS)
def test_ten_agents_have_no_window(E):
    """BASELINE configs[2]: the record leaves no room for the LDS window, the rows leave as ten dwords per lane."""
    pr = Pair(dict(C2, n_agents=10), E, 7, kernel="instance")
    for t in range(8):
        pr.step(17, "ten agents, %d replicas, step %d" % (E, t + 1))


@pytest.mark.parametrize("E", REPLICAS)
def test_counter_stream(E):
    """rng_mode "fast": the state is four words of the image, there are no rows to store."""
    pr = Pair(dict(C2), E, 9, rng_mode="fast")
    for t in range(8):
        pr.step(19, "counter stream, %d replicas, step %d" % (E, t + 1))


@pytest.mark.parametrize("E", REPLICAS)
def test_long_source_list(E):
    """More source doubles than AIE_SRC_CAP: the regeneration goes row by row and leaves nothing in the window."""
    pr = Pair(dict(DENSE), E, 4)
    assert (pr.be.tensors["regen_src_n"].cpu().numpy() > AIE_SRC_CAP).all()
    for t in range(8):
        pr.step(21, "long list, %d replicas, step %d" % (E, t + 1))


@pytest.mark.parametrize("E", REPLICAS)
def test_upload_between_two_steps(E):
    """aie_upload of a state tensor clears obs_valid: the next launch reads the cell words and writes every cell unit
    and the whole plane on its way out."""
    pr = Pair(dict(C2), E, 13, kernel="instance")
    for t in range(6):
        if t in (2, 3):
            pr.be.upload("cells", pr.be.download("cells"))
            assert not (pr.be.tensors["obs_valid"].cpu().numpy() != 0).any()
        pr.step(23, "upload, %d replicas, step %d" % (E, t + 1))


@pytest.mark.parametrize("E", REPLICAS)
def test_change_log_overflow(E):
    """Every source emptied under a regeneration weight of 1, plane and obs_valid uploaded to match: the step reads the
    plane, respawns more cells than its change log holds and writes everything.  (The crowded five-agent state of
    tests/rich_states.py changes a handful of cells a step; this is the cheap way to an overflow,
    tests/test_gpu_cell_plane.py.)"""
    cfg = dict(_uniform(25, 25, 4, starting_wood_coverage=0.08, starting_stone_coverage=0.08, wood_regen_weight=1.0,
                        stone_regen_weight=1.0), scenario_name="quadrant/simple_wood_and_stone")
    pr = Pair(cfg, E, 11)
    be, o = pr.be, pr.oracle
    pr.step(7, "overflow, %d replicas, step 1" % E)
    for k in ("stone", "wood"):
        be.upload(k, np.zeros_like(o.t[k]))
        o.t[k][...] = 0
    be.upload("cells_packed", pack(be.download("cells").view(np.uint32)))
    be.upload("obs_valid", np.ones(E, np.int32))
    pr.step(7, "overflow, %d replicas, the overflowing step" % E)
    respawned = (o.t["stone"] != 0).reshape(E, -1).sum(1) + (o.t["wood"] != 0).reshape(E, -1).sum(1)
    assert (respawned > AIE_DIRTY_CAP).all(), respawned
    pr.step(7, "overflow, %d replicas, the step behind it" % E)


@pytest.mark.parametrize("E", REPLICAS)
def test_twisting_refill(E):
    """The full-featured kernel of the development library with a draw window of 8 words, the generator four words short
    of its state's end: the first wave's refill twists the state in HBM, the second wave reads it back, regenerates
    and stores the rows wide."""
    pr = Pair(dict(C2), E, 15, dev=True)
    assert pr.be.lib.aie_dev_set_draw_window(pr.be.handle, 8) == 0
    past = 0
    for t in range(8):
        if t % 2 == 0:
            pr.set_position(620)
        drawn = pr.step(27, "refill, %d replicas, step %d" % (E, t + 1))
        if t % 2 == 0:
            past += int((drawn > 4).sum())  # (the components went past word 623)
    assert past >= E, past
