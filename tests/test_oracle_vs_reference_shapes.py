"""CPU tests that need the live reference (/root/reference, skipped elsewhere): the C restatement side by side with the
UNMODIFIED reference env at shapes the other parity tests leave out -- non-square worlds (a swapped H and W is invisible on
a square map), the 4096-cell limit of device-drawn layouts from both sides, and 13-62 agents with order books on either
side of 64 slots and both of gini's branches (helpers.SHAPE_CASES / AGENT_CASES, the cases tests/test_gpu_shapes.py holds
the device to).  Two episodes each: state, MT19937 stream, observations, rewards, metrics."""
import numpy as np
import pytest

from helpers import AGENT_CASES, REFUSED_SHAPES, SHAPE_CASES, compare_state, make_env, oracle_host_pre_reset
from test_oracle_vs_reference import _random_actions, _ref_env, check_metrics

pytestmark = pytest.mark.reference


def _track_live_reference(cfg, seed, where0):
    from oracle_lib import OracleEnv
    from ref_extract import extract_obs, extract_state, rewards_array

    np.random.seed(500 + seed)
    ref = _ref_env(cfg)
    host = make_env(cfg)
    o = OracleEnv(host.build_config(), host.layout_planes())
    np.random.seed(31 + seed)
    st = np.random.get_state()
    o.t["mt"][0] = st[1]
    o.t["mt_pos"][0] = st[2]
    obs = ref.reset()
    oracle_host_pre_reset(host, o)
    o.reset()
    rng = np.random.RandomState(5 + seed)
    multi_a = bool(cfg.get("multi_action_mode_agents", False))
    multi_p = bool(cfg.get("multi_action_mode_planner", True))

    def check(where, obs, rew=None):
        compare_state({k: v[0] for k, v in o.t.items()}, extract_state(ref), where=where, f64_tol=1e-9)
        assert np.array_equal(o.t["mt"][0], np.random.get_state()[1]), where + ": MT19937 state"
        for k, want in extract_obs(ref, obs).items():
            got = o.t[k][0]
            assert got.shape == want.shape, "%s: obs %s shape %s, reference %s" % (where, k, got.shape, want.shape)
            if want.dtype.kind in "iu":
                assert np.array_equal(got, want), "%s: obs %s" % (where, k)
            else:
                np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6, err_msg="%s: obs %s" % (where, k))
        if rew is not None:
            got = np.concatenate([o.t["rewards_a"][0], o.t["rewards_p"][[0]]])
            np.testing.assert_allclose(got, rewards_array(ref, rew), rtol=0, atol=1e-5, err_msg=where)
        check_metrics(ref, host, o, where)

    check(where0 + " reset", obs)
    resets = 0
    for t in range(2 * cfg["episode_length"] + 5):
        acts, aa, pa = _random_actions(ref, rng, multi_a, multi_p)
        obs, rew, done, _ = ref.step(acts)
        o.step(aa[None], pa[None])
        check("%s step %d" % (where0, t + 1), obs, rew)
        assert bool(o.t["done"][0]) == bool(done["__all__"])
        if done["__all__"]:
            obs = ref.reset()
            oracle_host_pre_reset(host, o)
            o.reset()
            resets += 1
            check("%s reset after step %d" % (where0, t + 1), obs)
    assert resets == 2
    return ref, o


@pytest.mark.parametrize("case", sorted(SHAPE_CASES))
@pytest.mark.parametrize("seed", [0, 1])
def test_oracle_tracks_live_reference_on_non_square_worlds(case, seed):
    cfg = SHAPE_CASES[case]
    ref, _ = _track_live_reference(cfg, seed, "%s seed %d" % (case, seed))
    H, W = cfg["world_size"]
    assert ref.world.maps.get("Wood").shape == (H, W)


@pytest.mark.parametrize("case", sorted(AGENT_CASES))
def test_oracle_tracks_live_reference_with_many_agents(case):
    cfg = AGENT_CASES[case]
    ref, o = _track_live_reference(cfg, 3, case)
    assert ref.n_agents == cfg["n_agents"]


@pytest.mark.parametrize("case", sorted(REFUSED_SHAPES))
def test_quadrant_shapes_the_reference_refuses_are_refused(case):
    """quadrant/ with width // 2 >= height (or height // 2 >= width): the reference's water lines index past the map
    (dynamic_layout.py:951-952) and its constructor raises IndexError; so does the product's, before any device work."""
    cfg = REFUSED_SHAPES[case]
    with pytest.raises(IndexError):
        _ref_env(cfg)
    with pytest.raises(IndexError):
        make_env(cfg, n_envs=2)
