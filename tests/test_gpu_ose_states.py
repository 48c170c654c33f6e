"""The one-step-economy kernels (csrc/aie_kernels_ose.hip) at their lane edges and in the states a uniform random
policy never reaches (tests/ose_states.py): agent counts around 30, 64 and 128, tax periods of three and seven steps,
2 / 5 / 7 / 16 brackets, incomes on the cutoffs, negative and tiny incomes, coin in escrow on a tax day, log utility --
on the device against the CPU oracle, every field after every step and every reset at the exactness of
tests/test_gpu_parity.py (_compare_all: integers, generator key and f64 state bit for bit, observations and rewards at
OBS_TOL), env.metrics at every tax day and at episode end.

tests/test_ose_states_cpu.py checks, without a GPU, that each case here reaches the conditions it declares; here the
census of the DEVICE's state must show them too.  One launch per step, E <= 16, <= 20 steps."""
import numpy as np
import pytest

import ose_states as S
from helpers import make_env
from test_gpu_parity import _compare_all, _compare_metrics

pytestmark = pytest.mark.gpu


def _pair(case):
    """(device env, oracle, Info): same configuration, same seed, both reset, on the kernel the case names."""
    from oracle_lib import OracleEnv

    env = make_env(case["cfg"], n_envs=case["E"], device="cuda:0", **case.get("env_kw", {}))
    be = env.backend
    if case.get("kernel") == "generic_selected":
        assert be.lib.aie_select_step_kernel(be.handle, 1) == 0  # AIE_KERNEL_GENERIC (step and reset)
    env.seed(case["seed"])
    env.reset()
    oracle = OracleEnv(env.build_config(), env.layout_planes())
    oracle.seed(case["seed"])
    oracle.reset()
    # which kernel runs: the build's one-step-economy instance is BASELINE configs[4]'s family (100 agents, us-federal
    # brackets, model_wrapper, tax period 1 -- the period stays in the family here); everything else is generic
    inst = be.lib.aie_step_kernel_instance(be.handle)
    if case.get("kernel") == "instance":
        assert inst >= 0, "no compile-time instance selected"
    else:
        assert inst == -1
    return env, oracle, S.Info(env)


def _step_both(env, oracle, a, p):
    import torch

    env.step({"a": torch.as_tensor(a, device="cuda:0"), "p": torch.as_tensor(p, device="cuda:0")})
    oracle.step(a, p)


def _assert_reached(name, case, reach):
    got = reach.result()
    missing = [k for k in case["reach"] if not got[k]]
    assert not missing, "%s: the device's own state does not show %s" % (name, missing)


@pytest.mark.parametrize("name", sorted(n for n, c in S.ROLLOUTS.items() if not c.get("auto_reset")))
def test_hip_matches_oracle_on_one_step_economy_policy_rollouts(name):
    """A scripted policy, evaluated on the host from the oracle's masks, drives E replicas through an episode, its reset
    and the first steps of the next; the device is compared after every step and every reset."""
    case = S.ROLLOUTS[name]
    env, oracle, info = _pair(case)
    be = env.backend
    _compare_all(be, oracle, name + " after reset")
    reach, resets = S.Reach(), 0
    for k in range(case["steps"]):
        a, p = S.policy_actions(case, info, oracle.t["obs_a_action_mask"], oracle.t["obs_p_action_mask"], k)
        tax_day = bool((oracle.t["tax_cycle_pos"] >= info.period).any())
        before = S.snapshot(be.tensors)
        _step_both(env, oracle, a, p)
        where = "%s step %d" % (name, k + 1)
        _compare_all(be, oracle, where)
        reach.add(S.census(before, S.snapshot(be.tensors), a, info))
        if tax_day or oracle.t["done"].all():
            _compare_metrics(env, oracle, where, require_trade_tax=False)
        if oracle.t["done"].all():
            assert bool(be.tensors["done"].all())
            env.reset(be.tensors["done"])
            oracle.reset(oracle.t["done"].copy())
            resets += 1
            _compare_all(be, oracle, where + " and reset")
    assert resets >= 1
    assert int(be.tensors["error_flags"].abs().sum()) == 0
    _assert_reached(name, case, reach)


@pytest.mark.parametrize("name", sorted(n for n, c in S.ROLLOUTS.items() if c.get("auto_reset")))
def test_hip_auto_reset_matches_oracle_step_then_masked_reset(name):
    """aie_set_auto_reset at 65 agents and a tax period of three steps: the device with auto-reset against a second device
    environment that steps and then resets the finished replicas from the host (the comparison of
    test_gpu_parity.test_auto_reset_equals_step_then_masked_reset), and that second one against the oracle at both
    stages.  Half of the replicas are one step ahead, so every launch mixes restarting and running replicas."""
    import torch

    case = S.ROLLOUTS[name]
    E = case["E"]
    env_auto, oracle, info = _pair(case)
    env_ref, _, _ = _pair(case)
    b_auto, b_ref = env_auto.backend, env_ref.backend
    a, p = S.policy_actions(case, info, oracle.t["obs_a_action_mask"], oracle.t["obs_p_action_mask"], 0)
    odd = (np.arange(E) % 2).astype(np.uint8)
    for b in (b_auto, b_ref):  # de-phase: half of the replicas restart one step in
        b.step(torch.as_tensor(a, device="cuda:0"), torch.as_tensor(p, device="cuda:0"))
        b.reset(torch.as_tensor(odd, device="cuda:0"))
    oracle.step(a, p)
    oracle.reset(odd)
    _compare_all(b_ref, oracle, name + " de-phased")
    b_auto.set_auto_reset(True)
    reach, restarts = S.Reach(), 0
    for k in range(1, case["steps"]):
        a, p = S.policy_actions(case, info, oracle.t["obs_a_action_mask"], oracle.t["obs_p_action_mask"], k)
        ta, tp = torch.as_tensor(a, device="cuda:0"), torch.as_tensor(p, device="cuda:0")
        where = "%s step %d" % (name, k + 1)
        before = S.snapshot(b_ref.tensors)
        b_auto.step(ta, tp)
        b_ref.step(ta, tp)
        oracle.step(a, p)
        _compare_all(b_ref, oracle, where)
        reach.add(S.census(before, S.snapshot(b_ref.tensors), a, info))
        done = b_ref.tensors["done"].clone()
        rew_a, rew_p = b_ref.tensors["rewards_a"].clone(), b_ref.tensors["rewards_p"].clone()
        if bool(done.any()):
            restarts += int(done.sum())
            b_ref.reset(done)
            oracle.reset(oracle.t["done"].copy())
            _compare_all(b_ref, oracle, where + " and masked reset")
        torch.cuda.synchronize()
        assert torch.equal(b_auto.tensors["done"], done), where + ": done"
        assert torch.equal(b_auto.tensors["rewards_a"], rew_a) and torch.equal(b_auto.tensors["rewards_p"], rew_p), where
        for key, v in b_ref.tensors.items():
            if key in ("done", "rewards_a", "rewards_p", "sample_t") or key.startswith("metrics_"):
                continue
            assert torch.equal(v, b_auto.tensors[key]), "%s: %s differs" % (where, key)
    assert restarts >= E
    assert int(b_auto.tensors["error_flags"].abs().sum()) == 0 and int(b_ref.tensors["error_flags"].abs().sum()) == 0
    _assert_reached(name, case, reach)


@pytest.mark.parametrize("name", sorted(S.INJECTED))
def test_hip_matches_oracle_from_injected_one_step_economy_states(name):
    """Every replica starts from another ose_states.injected_state (coin 1 with 500 in escrow on a tax day, last_coin above
    coin, an income of 4.8e-7, coin over ten decades, no coin at all after 100 hours, one agent holding everything),
    loaded on both sides; then a NO-OP step and two steps of the case's policy.  Only the oracle vouches for these
    states (tests/test_ose_states_cpu.py says which conditions no reference run stands behind)."""
    case = S.INJECTED[name]
    env, oracle, info = _pair(case)
    be = env.backend
    for e, s in enumerate(S.injected_states(case, info, oracle)):
        be.load_state(s, e=e)
        oracle.load_state(s, e=e)
    be.invalidate_observations()
    reach = S.Reach()
    for k in range(case["steps"]):
        a, p = S.injected_actions(case, info, oracle.t["obs_a_action_mask"], oracle.t["obs_p_action_mask"], k)
        tax_day = bool((oracle.t["tax_cycle_pos"] >= info.period).any())
        before = S.snapshot(be.tensors)
        _step_both(env, oracle, a, p)
        where = "%s step %d" % (name, k + 1)
        _compare_all(be, oracle, where)
        reach.add(S.census(before, S.snapshot(be.tensors), a, info))
        if tax_day:
            _compare_metrics(env, oracle, where, require_trade_tax=False)
    assert int(be.tensors["error_flags"].abs().sum()) == 0
    _assert_reached(name, case, reach)
