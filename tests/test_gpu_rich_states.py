"""The step and reset kernels in the rich states a random policy never reaches (tests/rich_states.py): scripted
closed-loop policies over a whole episode and its reset, and injected states with hand-built order books, on the device
against the CPU oracle -- every field after every step, at the exactness of tests/test_gpu_parity.py (_compare_all:
integers, books, generator key and f64 state bit for bit, observations and rewards at OBS_TOL).

tests/test_rich_states_cpu.py checks, without a GPU, that each scenario here reaches the conditions it declares."""
import numpy as np
import pytest

import rich_states as R
from helpers import make_env, oracle_host_pre_reset
from test_gpu_parity import _compare_all, _compare_metrics

pytestmark = pytest.mark.gpu


def _pair(case):
    """(device env, oracle, Info): same configuration, same seed, both reset."""
    from oracle_lib import OracleEnv

    env = make_env(case["cfg"], n_envs=case["E"], device="cuda:0", **case.get("env_kw", {}))
    be = env.backend
    if case.get("kernel") == "generic":
        assert be.lib.aie_select_step_kernel(be.handle, 1) == 0  # AIE_KERNEL_GENERIC (step and reset)
    env.seed(case["seed"])
    env.reset()
    oracle = OracleEnv(env.build_config(), env.layout_planes())
    oracle.seed(case["seed"])
    oracle_host_pre_reset(env, oracle)
    oracle.reset()
    # which kernel runs: scalars alone (payment, tax period, cutoffs, regeneration, starting coin) leave C2 / C3 on
    # their compile-time instances
    inst = be.lib.aie_step_kernel_instance(be.handle)
    if case.get("kernel") == "instance":
        assert inst >= 0, "no compile-time instance selected"
    elif case.get("kernel") == "generic":
        assert inst == -1
    return env, oracle, R.Info(env)


@pytest.mark.parametrize("name", sorted(n for n, c in R.ROLLOUTS.items() if "dense_log_frequency" not in c["cfg"]))
def test_hip_matches_oracle_on_policy_rollouts(name):
    """A scripted policy, evaluated on the host from the oracle's masks, drives E replicas through one whole episode,
    its reset and the first steps of the next; the device is compared after every step and every reset, env.metrics at
    every tax day."""
    import torch

    case = R.ROLLOUTS[name]
    env, oracle, info = _pair(case)
    be = env.backend
    n, E = info.n, case["E"]
    log = be.set_reward_log(3) if case.get("reward_log") else None
    _compare_all(be, oracle, name + " after reset")
    tax_days = resets = 0
    for t in range(R.rollout_steps(case)):
        a, p = R.policy_actions(case["policy"], env, oracle.t["obs_a_action_mask"], oracle.t["obs_p_action_mask"],
                                case["seed"], int(oracle.t["timestep"][0]), info)
        days = oracle.t["metrics_tax_days"].copy()
        env.step({"a": torch.as_tensor(a, device="cuda:0"), "p": torch.as_tensor(p, device="cuda:0")})
        oracle.step(a, p)
        where = "%s step %d" % (name, t + 1)
        _compare_all(be, oracle, where)
        if log is not None:  # the reward log's slot of this step: the same floats as the reward tensors
            row = log[t % 3].cpu().numpy()
            assert np.array_equal(row[:, :n], be.tensors["rewards_a"].cpu().numpy()), where
            assert np.array_equal(row[:, n], be.tensors["rewards_p"].cpu().numpy()), where
            assert np.array_equal(row[:, n + 1] > 0.5, oracle.t["done"].astype(bool)), where
        if (oracle.t["metrics_tax_days"] > days).any():
            tax_days += 1
            _compare_metrics(env, oracle, where)
        if oracle.t["done"].all():
            assert bool(be.tensors["done"].all())
            env.reset(be.tensors["done"])
            oracle_host_pre_reset(env, oracle)
            oracle.reset(oracle.t["done"].copy())
            resets += 1
            _compare_all(be, oracle, where + " and reset")
    assert resets == 1 and tax_days >= 2
    assert int(be.tensors["error_flags"].abs().sum()) == 0


def test_hip_matches_oracle_on_a_policy_rollout_with_a_dense_logged_replica():
    """Multi-action agents on the mix policy with every episode of replica 0 dense-logged: busy steps fill the event
    rows (builds, gathers, several trades per agent, tax rows).  Rows and assembled logs as in
    test_dense_log.test_hip_dense_log_matches_oracle; everything else as in the rollouts above."""
    import torch
    from oracle_lib import OracleEnv
    from test_dense_log import OracleBackend, assert_logs_equal

    name = "mix_multi_action_dense_log"
    case = R.ROLLOUTS[name]
    E = case["E"]
    env = make_env(case["cfg"], n_envs=E, device="cuda:0")
    env.seed(case["seed"])
    twin = make_env(case["cfg"], n_envs=E)
    o = OracleEnv(twin.build_config(), twin.layout_planes())
    o.seed(case["seed"])
    twin._backend = OracleBackend(o)
    twin.host_pre_reset = lambda mask: oracle_host_pre_reset(twin, o)
    info = R.Info(twin)
    busiest = 0
    for ep in range(2):
        env.reset()
        twin.reset()
        be = env.backend
        assert "log_events" in be.tensors
        _compare_all(be, o, "%s reset %d" % (name, ep))
        for t in range(case["cfg"]["episode_length"] if ep == 0 else 3):
            a, p = R.policy_actions(case["policy"], twin, o.t["obs_a_action_mask"], o.t["obs_p_action_mask"], case["seed"],
                                    int(o.t["timestep"][0]), info)
            assert env._dense_log_this_episode
            days = o.t["metrics_tax_days"].copy()
            env.step({"a": torch.as_tensor(a, device="cuda:0"), "p": torch.as_tensor(p, device="cuda:0")})
            twin.step({"a": torch.from_numpy(a), "p": torch.from_numpy(p)})
            where = "%s episode %d step %d" % (name, ep, t + 1)
            _compare_all(be, o, where)
            cnt = be.tensors["log_event_count"].cpu().numpy()
            assert np.array_equal(cnt, o.t["log_event_count"]), where
            busiest = max(busiest, int(cnt[0]))
            got = be.tensors["log_events"].cpu().numpy()[0, : cnt[0]]
            want = o.t["log_events"][0, : cnt[0]]
            assert np.array_equal(got[:, :10], want[:, :10]), where  # event type + integer fields
            if cnt[0]:
                np.testing.assert_allclose(np.ascontiguousarray(got[:, 10:]).view(np.float64),
                                           np.ascontiguousarray(want[:, 10:]).view(np.float64), rtol=1e-9, atol=1e-9)
            if (o.t["metrics_tax_days"] > days).any():
                _compare_metrics(env, o, where)
        if ep == 0:
            assert bool(be.tensors["done"][0]) and bool(o.t["done"][0])
            assert_logs_equal(env.previous_episode_dense_log, twin.previous_episode_dense_log, tol=1e-6)
    assert busiest >= info.NB + info.n, busiest  # a tax day alone: one row per bracket and one per agent
    assert int(be.tensors["error_flags"].abs().sum()) == 0


@pytest.mark.parametrize("name", sorted(R.INJECTED))
def test_hip_matches_oracle_from_injected_states(name):
    """Every replica starts from another rich_state (full books, ties, incomes on the cutoffs, coin in escrow on a tax
    day, walled-in agents, inventories past 255, extreme coin ...), loaded on both sides; then a NO-OP step and the
    market / builder script (rich_states.injected_actions)."""
    import torch

    case = R.INJECTED[name]
    env, oracle, info = _pair(case)
    be = env.backend
    states = R.injected_states(case, env, oracle, info)
    for e, s in enumerate(states):
        sub = {k: s[k] for k in R.LOAD_KEYS if k in s}
        be.load_state(sub, e=e)
        oracle.load_state(sub, e=e)
    be.invalidate_observations()
    for k in range(case["steps"]):
        a, p = R.injected_actions(case, env, oracle, k, info)
        days = oracle.t["metrics_tax_days"].copy()
        env.step({"a": torch.as_tensor(a, device="cuda:0"), "p": torch.as_tensor(p, device="cuda:0")})
        oracle.step(a, p)
        where = "%s step %d" % (name, k + 1)
        _compare_all(be, oracle, where)
        if (oracle.t["metrics_tax_days"] > days).any():
            _compare_metrics(env, oracle, where)
    assert int(be.tensors["error_flags"].abs().sum()) == 0
    after = R.snapshot(be.tensors)
    for e in range(case["E"]):
        R.assert_invariants({kk: after[kk][e] for kk in R.INVARIANT_KEYS if kk in after}, env, info,
                            "%s: device replica %d" % (name, e), source_list=bool(after.get("regen_src_n", np.zeros(1))[e]))
