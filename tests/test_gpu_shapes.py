"""GPU tests (pytest -m gpu): the HIP step and reset kernels against the CPU oracle at the shapes the rest of the suite
leaves out -- non-square worlds (every other map is square, so a swapped H and W would pass), the 4096-cell limit of
device-drawn layouts from both sides, and 13-62 agents with order books on either side of 64 slots and both of gini's
branches.  The oracle is pinned against the live reference at the same configurations
(tests/test_oracle_vs_reference_shapes.py).  Every field of every replica after every step; each run crosses an episode
end and a masked reset of a strict subset of the replicas."""
import numpy as np
import pytest

from helpers import AGENT_CASES, SHAPE_CASES, book_slots, make_env, oracle_host_pre_reset
from test_gpu_parity import _compare_all

pytestmark = pytest.mark.gpu

AIE_NT = 64  # a non-log step kernel holds order books of up to AIE_NT slots (csrc/aie_capi.hip: P.M > AIE_NT -> log)
LOG_KERNEL_CASES = {"n13_book65", "n33_book66"}  # the rest of AGENT_CASES must stay on the non-log kernels


def _run_against_oracle(env, cfg_T, seed, where0, E):
    """Reset, then episode_length + episode_length // 3 + 2 steps: replicas 1, 4, 7, ... are reset at a third of the
    episode, every replica is reset when it is done (the others at the episode end, the subset a third later).  Returns
    the most bids one replica's book held for one resource."""
    import torch
    from oracle_lib import OracleEnv

    be = env.backend
    oracle = OracleEnv(env.build_config(), env.layout_planes())
    env.seed(seed)
    oracle.seed(seed)
    env.reset()
    oracle_host_pre_reset(env, oracle)
    oracle.reset()
    _compare_all(be, oracle, where0 + " reset")
    mid = cfg_T // 3
    subset = (np.arange(E) % 3 == 1).astype(np.uint8)
    ends = fill = 0
    for t in range(cfg_T + mid + 2):
        a, p = be.sample_random_actions(seed=seed + 11)
        env.step({"a": a, "p": p})
        torch.cuda.synchronize()
        oracle.step(a.cpu().numpy(), p.cpu().numpy(), nthreads=4)
        _compare_all(be, oracle, "%s step %d" % (where0, t + 1))
        if "cda_n_bids" in oracle.t:
            fill = max(fill, int(oracle.t["cda_n_bids"].max()))
        done = be.tensors["done"].cpu().numpy().astype(np.uint8)
        if t + 1 == mid:
            assert not done.any()
            mask = subset
        elif done.any():
            assert np.array_equal(done, subset) or np.array_equal(done, 1 - subset), (where0, t + 1, done)
            mask = done
            ends += 1
        else:
            continue
        env.reset(torch.as_tensor(mask, device="cuda:0"))
        oracle_host_pre_reset(env, oracle, which=np.nonzero(mask)[0])
        oracle.reset(mask)
        torch.cuda.synchronize()
        _compare_all(be, oracle, "%s masked reset after step %d" % (where0, t + 1))
    assert ends == 2, ends
    return fill


@pytest.mark.parametrize("case", sorted(SHAPE_CASES))
def test_hip_matches_oracle_on_non_square_worlds(case):
    cfg = SHAPE_CASES[case]
    H, W = cfg["world_size"]
    E = 12
    np.random.seed(61)
    env = make_env(cfg, n_envs=E, device="cuda:0")
    assert bool(env.layouts_on_device) == (H * W <= 4096), "device-drawn layouts end at 4096 cells"
    be = env.backend
    assert tuple(be.tensors["stone"].shape[1:]) == (H, W)
    _run_against_oracle(env, cfg["episode_length"], 8, case, E)
    if case in ("uniform_24x160", "uniform_160x24"):  # past the sparse regeneration's source list: the row-by-row sweep
        cap = int(be.tensors["regen_src_list"].shape[-1])
        assert (be.tensors["regen_src_n"].cpu().numpy() > cap).all()


@pytest.mark.parametrize("case", sorted(AGENT_CASES))
def test_hip_matches_oracle_with_many_agents(case):
    cfg = AGENT_CASES[case]
    M = book_slots(cfg)
    log_kernel = case in LOG_KERNEL_CASES
    assert (M > AIE_NT) == log_kernel, "%s: a %d-slot book has drifted to the other kernel" % (case, M)
    E = 8
    env = make_env(cfg, n_envs=E, device="cuda:0")
    be = env.backend
    assert int(be.tensors["cda_bids"].shape[-1]) == M
    k = be.lib.aie_step_kernel_instance(be.handle)
    print("%s: n=%d M=%d kernel %s" % (case, cfg["n_agents"], M, "log" if log_kernel else
                                        "instance %d" % k if k >= 0 else "generic"))
    fill = _run_against_oracle(env, cfg["episode_length"], 5, case, E)
    print("%s: up to %d of %d bid slots in use" % (case, fill, M))
    assert fill > min(M, AIE_NT) // 2, (case, fill, M)


def test_hip_fast_mode_layouts_drawn_ahead_on_a_non_square_world():
    """rng_mode="fast" on 12 x 37: layouts come from a stream of their own and are drawn AHEAD of their resets once a
    quarter of the replicas have used theirs up (tests/test_rng_fast.py has the square case); a de-phased pattern of masked
    resets takes both roads (installed from the staging area; drawn inside the reset) and equals the oracle."""
    import torch
    from oracle_lib import OracleEnv

    E = 48
    cfg = dict(SHAPE_CASES["uniform_12x37_source_counts"], episode_length=1000)
    env = make_env(cfg, n_envs=E, device="cuda:0", rng_mode="fast")
    be = env.backend
    env.seed(19)
    env.reset()
    oracle = OracleEnv(env.build_config(), env.layout_planes())
    oracle.seed(19)
    oracle.reset()
    ctl = be.tensors["layout_stage_ctl"]
    torch.cuda.synchronize()
    base = ctl.cpu().reshape(-1).tolist()
    _compare_all(be, oracle, "after reset")
    rs = np.random.RandomState(3)
    groups = [list(range(0, 4)), list(range(0, 4)), list(range(4, 20)), list(range(2, 6)), list(range(20, 48)),
              list(range(0, 48)), list(rs.choice(E, 10, replace=False)), list(rs.choice(E, 15, replace=False))]
    for k, grp in enumerate(groups):
        for _ in range(3):
            a, p = be.sample_random_actions(seed=41)
            env.step({"a": a, "p": p})
            oracle.step(a.cpu().numpy(), p.cpu().numpy(), nthreads=4)
        torch.cuda.synchronize()
        _compare_all(be, oracle, "steps before masked reset %d" % k)
        mask = np.zeros(E, np.uint8)
        mask[grp] = 1
        env.reset(torch.from_numpy(mask).to("cuda:0"))
        oracle.reset(mask)
        torch.cuda.synchronize()
        _compare_all(be, oracle, "masked reset %d" % k)
    staged, inside = [x - y for x, y in zip(ctl.cpu().reshape(-1).tolist()[2:], base[2:])]
    assert staged + inside == sum(len(g) for g in groups)
    assert staged > 0 and inside > 0, (staged, inside)
