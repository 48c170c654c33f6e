"""The PPO rollout seam on the device: aie_gae, aie_trajectory_store, rollout.Trajectory and GraphedStep(trajectory=...).

  * aie_gae against the plain NumPy float32 loop (tests/gae_ref.py) bit for bit on synthetic logs the test uploads: the
    three scenario families' (E, n), T = 1, 7, 200 and the kernel's chunk edges (8, 9, 15, 16, 17, 24, 33 steps), a ring that
    wraps from first_slot != 0 -- inside a chunk of 8 steps and exactly between two --, an all-done row, NaN behind done
    steps, every NULL combination, and the invalid arguments (refused, nothing launched);
  * aie_trajectory_store, eager, 7 steps into 4 slots with auto-reset: every slot equals the host snapshot taken just before
    its store, the counters are k % 4 -- segments of 4 B, 344 B, a 16-byte-aligned size, a destination 4 bytes off, a
    record field (source stride = the record's) and COVID's transposed masks (== Backend.action_masks());
  * GraphedStep(trajectory=...): the replayed loop and an eager twin take the same 2 T + 1 steps -- buffers, reward logs and
    arenas equal bit for bit;
  * consistency: policy_evaluate(stored logits, stored masks, stored actions) == the stored logp (importance ratio exactly
    1), and Trajectory.advantages() == gae_ref on the downloaded log and values, across an auto-reset inside the fragment.
"""
import ctypes

import numpy as np
import pytest

import gae_ref
from gae_ref import bits, f32
from helpers import load_covid_golden, make_env

pytestmark = pytest.mark.gpu

GTB = [["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 5}], ["Gather", {}], ["PeriodicBracketTax", {}]]
C2 = dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=4, world_size=[25, 25], episode_length=1000,
          components=GTB, starting_agent_coin=10, env_layout_file="quadrant_25x25_20each_30clump.txt")
GAMMA, LAM = 0.998, 0.98
DEV = "cuda:0"


def _cfg(case, **kw):
    if case == "covid":
        return dict(load_covid_golden("c4_covid_variant")["cfg"], scenario_name="CovidAndEconomySimulation")
    if case == "one_step_economy":
        rs = np.random.RandomState(4)
        return dict(scenario_name="one-step-economy", n_agents=12, world_size=[1, 1], episode_length=3,
                    components=[["SimpleLabor", {"skills": [float(x) for x in np.sort(1 + rs.rand(12) * 2)]}],
                                ["PeriodicBracketTax", {"bracket_spacing": "us-federal", "period": 1, "tax_model": "model_wrapper"}]])
    return dict(C2, **kw)


def _env(case, E, seed=3, **kw):
    env = make_env(_cfg(case, **kw), n_envs=E, device=DEV)
    if case != "covid":
        env.seed(seed)
    env.reset()
    return env


_ENVS = {}
GAE_ENVS = {"gtb_c2": (5, 4), "one_step_economy": (64, 12), "covid": (3, 51)}


def _gae_env(case):
    if case not in _ENVS:
        E, n = GAE_ENVS[case]
        _ENVS[case] = _env(case, E)
        assert (_ENVS[case].backend.E, _ENVS[case].backend.n) == (E, n)
    return _ENVS[case].backend


def _synthetic(E, n, T, n_slots, first, seed, poison=True):
    """(log [n_slots, E, n + 2], values_a [T + 1, E, n], values_p [T + 1, E]): N(0, 1) rewards, N(0, 10^2) values, done with
    probability 0.2, one all-done row, the last step done for every second replica; NaN / inf in V_{t+1} behind done steps
    (row T included); the slots outside the fragment hold NaN (they must not be read)."""
    rng = np.random.RandomState(seed)
    log = np.full((n_slots, E, n + 2), np.nan, f32)
    rows = (first + np.arange(T)) % n_slots
    done = (rng.rand(T, E) < 0.2).astype(f32)
    done[T // 2] = 1.0
    done[T - 1, ::2] = 1.0
    log[rows, :, : n + 1] = rng.randn(T, E, n + 1).astype(f32)
    log[rows, :, n + 1] = done
    va = (rng.randn(T + 1, E, n) * 10).astype(f32)
    vp = (rng.randn(T + 1, E) * 10).astype(f32)
    if poison:
        t_idx, e_idx = np.nonzero(done > 0.5)
        kinds = np.array([np.nan, np.inf, -np.inf], f32)
        for k, (t, e) in enumerate(zip(t_idx, e_idx)):
            if t == T - 1 or k % 3 == 0:  # every bootstrap value behind a done last step, a third of the others
                va[t + 1, e, :] = kinds[k % 3]
                vp[t + 1, e] = kinds[(k + 1) % 3]
    return log, va, vp


def _same_bits(got, want, what):
    """Bit for bit; where the reference is NaN (a step whose OWN value was poisoned, and its episode before it) NaN."""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    want = np.asarray(want, f32)
    got = got.reshape(want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN where the reference has none (or the reverse)"
    bad = np.flatnonzero((bits(got) != bits(want)) & ~nan)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r, want %r" % (
        what, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _ring_placements(T):
    """(n_slots, first_slot): a ring that wraps (T >= 3); the trajectory's own; full wrap; then the kernel's chunk edges.  Time
    runs backwards from step T - 1 in chunks of U = 8 steps (csrc/aie_kernels_rollout.hip: AIE_GAE_U), so a chunk starts at a
    step t = T (mod 8); the ring wraps in front of step n_slots - first."""
    out = [(T + 3, T + 1), (T, 0), (T, T - 1)]
    if T >= 4:
        out.append((T + 1, T - 3))   # the wrap in front of step 4: inside a chunk unless T = 4 (mod 8)
    if T >= 9:
        out.append((T + 3, T - 5))   # first = n_slots - 8: steps 0 .. 7 end the ring, step 8 is slot 0
        out.append((T, 8))           # the wrap in front of step T - 8: exactly between the first two chunks the kernel takes
    return out


# 8, 9: one full chunk, and one more step; 15, 16, 17: both register buffers, and one more step; 24, 33: an odd number of chunks
@pytest.mark.parametrize("T", [1, 7, 200, 8, 9, 15, 16, 17, 24, 33])
@pytest.mark.parametrize("case", list(GAE_ENVS))
def test_gae_equals_the_numpy_float32_loop(case, T):
    import torch

    be = _gae_env(case)
    E, n = be.E, be.n
    for n_slots, first in _ring_placements(T):
        log, va, vp = _synthetic(E, n, T, n_slots, first, 100 * T + n_slots + first)
        want = gae_ref.from_log(log, first, T, va, vp, GAMMA, LAM)
        got = be.gae(T, torch.tensor(log, device=DEV), torch.tensor(va, device=DEV), torch.tensor(vp, device=DEV), GAMMA, LAM,
                     first_slot=first)
        torch.cuda.synchronize()
        for g, w, name in zip(got, want, ("adv_a", "adv_p", "ret_a", "ret_p")):
            _same_bits(g, w, "%s T=%d slots=%d first=%d %s" % (case, T, n_slots, first, name))
        # a done step selects: whatever sits behind it, its own advantage is r - V (finite here wherever its own V is)
        rows = (first + np.arange(T)) % n_slots
        done = log[rows, :, n + 1] > 0.5
        own_ok = np.isfinite(vp[:T])
        adv_p = got[1].cpu().numpy()
        sel = done & own_ok
        assert sel.any() and np.array_equal(bits(adv_p[sel]), bits((log[rows, :, n] - vp[:T])[sel]))
    # no poison: everything finite, and other discount factors
    log, va, vp = _synthetic(E, n, T, T + 3, 2, 7 * T, poison=False)
    for gamma, lam in ((0.9, 0.5), (1.0, 1.0)):
        want = gae_ref.from_log(log, 2, T, va, vp, gamma, lam)
        got = be.gae(T, torch.tensor(log, device=DEV), torch.tensor(va, device=DEV), torch.tensor(vp, device=DEV), gamma, lam,
                     first_slot=2)
        for g, w in zip(got, want):
            assert np.isfinite(w).all()
            _same_bits(g, w, "%s T=%d gamma=%g" % (case, T, gamma))


def test_gae_null_combinations_and_invalid_arguments():
    import torch

    from ai_economist_amd import _cabi

    be = _gae_env("gtb_c2")
    E, n, T, n_slots, first = be.E, be.n, 7, 10, 8
    log, va, vp = _synthetic(E, n, T, n_slots, first, 5)
    want = gae_ref.from_log(log, first, T, va, vp, GAMMA, LAM)
    d_log, d_va, d_vp = (torch.tensor(x, device=DEV) for x in (log, va, vp))
    SENT = 12345.0
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def fresh():
        return [torch.full((T, E, n), SENT, device=DEV), torch.full((T, E), SENT, device=DEV),
                torch.full((T, E, n), SENT, device=DEV), torch.full((T, E), SENT, device=DEV)]

    def call(T_, log_, slots_, first_, va_, vp_, outs):
        return be.lib.aie_gae(be.handle, T_, P(log_), slots_, first_, P(va_), P(vp_), GAMMA, LAM, P(outs[0]), P(outs[1]), P(outs[2]),
                              P(outs[3]), None)

    # every subset of the four outputs: agents only, planner only, no returns, returns only, ...; the values of a class
    # without outputs may be NULL
    for keep in range(16):
        out = fresh()
        use = [out[i] if keep >> i & 1 else None for i in range(4)]
        need_a, need_p = bool(keep & 5), bool(keep & 10)
        assert call(T, d_log, n_slots, first, d_va if need_a else None, d_vp if need_p else None, use) == 0, keep
        torch.cuda.synchronize()
        for i in range(4):
            if use[i] is None:
                assert bool((out[i] == SENT).all()), keep
            else:
                _same_bits(out[i], want[i], "outputs %d, %d" % (keep, i))
    # refusals: nothing is launched, nothing is written
    out = fresh()
    bad = [(0, d_log, n_slots, first, d_va, d_vp, out), (n_slots + 1, d_log, n_slots, first, d_va, d_vp, out),
           (T, d_log, T - 1, 0, d_va, d_vp, out), (T, d_log, n_slots, -1, d_va, d_vp, out),
           (T, d_log, n_slots, n_slots, d_va, d_vp, out), (T, None, n_slots, first, d_va, d_vp, out),
           (T, d_log, n_slots, first, None, d_vp, out), (T, d_log, n_slots, first, d_va, None, out),
           (T, d_log, n_slots, first, None, d_vp, [None, None, out[2], None])]
    for args in bad:
        assert call(*args) == _cabi.E_INVALID, args[:4]
        assert be.lib.aie_last_error(be.handle)
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in out)
    with pytest.raises(ValueError):
        be.gae(T, d_log, d_va, d_vp, GAMMA, LAM, first_slot=n_slots)


STORE_CASES = {"gtb_c2": ("obs_a_flat", "obs_p_flat"), "one_step_economy": ("obs_a_flat", "obs_p_flat"),
               "covid": ("obs_a_world-agent_state", "obs_p_FederalGovernmentSubsidy-t_until_next_subsidy")}


@pytest.mark.parametrize("case", list(STORE_CASES))
def test_trajectory_store_fills_the_ring_slot_by_slot(case):
    import torch

    from ai_economist_amd import _cabi
    from ai_economist_amd.rollout import Trajectory

    E, T, STEPS = 5, 4, 7
    env = _env(case, E, episode_length=6)
    be = env.backend
    be.set_auto_reset(True)
    traj = Trajectory(env, T, observations=STORE_CASES[case], logp=False, values=False)
    assert traj.log.shape == (T, E, be.n + 2) and be.reward_log is traj.log
    t = be.tensors
    if case == "gtb_c2":
        assert t["obs_p_flat"][0].numel() * 4 == 344  # 8-byte aligned only: the 4-byte path
    # beside the trajectory's own segments (observations, masks -- COVID's transposed --, actions):
    val = torch.zeros(E, device=DEV)                       # 4 bytes per replica (a planner value)
    blk = torch.zeros(E, 8, device=DEV)                    # 32 bytes per replica, everything 16-byte aligned: the wide path
    d_val = torch.zeros(T, E, device=DEV)
    d_blk = torch.zeros(T, E, 8, device=DEV)
    off_store = torch.zeros(T * E * 8 + 1, device=DEV)
    d_off = off_store[1:].view(T, E, 8)                    # the same block to a destination 4 bytes off: 4-byte accesses
    d_rec = torch.zeros(T, E, dtype=torch.int32, device=DEV)
    rec = t["sample_t"]                                    # a record field: source stride = the record's
    assert blk.data_ptr() % 16 == 0 and d_blk.data_ptr() % 16 == 0 and d_off.data_ptr() % 16 == 4
    a, p = be._action_buffers(0)
    seg = be.trajectory_segment
    extra = [seg(val, d_val), seg(blk, d_blk), seg(rec, d_rec)]
    s_off, _ = seg(blk, d_blk)
    s_off.dst = d_off.data_ptr()
    assert extra[2][0].src_stride == (rec.stride(0) * 4) and extra[2][0].src_stride > 4 and extra[2][0].bytes == 4
    segs = list(traj._fixed) + [seg(a, traj.actions_a), seg(p, traj.actions_p)] + extra + [s_off]
    names = list(STORE_CASES[case]) + ["masks_a", "masks_p", "actions_a", "actions_p", "val", "blk", "rec", "off"]
    dsts = [traj.obs[k] for k in STORE_CASES[case]] + [traj.masks_a, traj.masks_p, traj.actions_a, traj.actions_p, d_val, d_blk,
                                                       d_rec, d_off]
    assert len(segs) == len(dsts) <= _cabi.TRAJ_MAX_SEGMENTS
    g = torch.Generator(device="cpu").manual_seed(1)
    snaps, dones = [], []

    def check(k):
        torch.cuda.synchronize()
        assert traj.slots.cpu().tolist() == [k % T] * E
        for s in range(T):
            last = max(j for j in range(k) if j % T == s)
            for name, dst, want in zip(names, dsts, snaps[last]):
                assert dst[s].dtype == want.dtype and torch.equal(dst[s].cpu().view(torch.uint8), want.view(torch.uint8)), \
                    "%s: slot %d != the snapshot of step %d (%s)" % (case, s, last, name)
            assert torch.equal(traj.log[s, :, -1].cpu(), dones[last])

    for k in range(STEPS):
        la = torch.randn(tuple(traj.masks_a.shape[1:]), generator=g).to(DEV)
        lp = torch.randn(tuple(traj.masks_p.shape[1:]), generator=g).to(DEV)
        be.sample_policy_actions(la, lp, seed=9)
        val.copy_(torch.randn(E, generator=g))
        blk.copy_(torch.randn(E, 8, generator=g))
        ma, mp = be.action_masks()
        torch.cuda.synchronize()
        snaps.append([t[name].cpu().clone() for name in STORE_CASES[case]] +
                     [x.cpu().clone() for x in (ma, mp, a, p, val, blk, rec, blk)])
        be.trajectory_store(segs, T, traj.slots)
        be.step(a, p)
        torch.cuda.synchronize()
        dones.append(t["done"].cpu().float())
        if k + 1 in (T, STEPS):
            check(k + 1)
    if case != "covid":
        assert any(bool(d.any()) for d in dones[:-1]), "no episode ended inside the run"
    if case == "gtb_c2":
        assert len({s[2].numpy().tobytes() for s in snaps}) > 1, "the masks never changed"
    traj.rewind()
    torch.cuda.synchronize()
    assert traj.slots.cpu().tolist() == [0] * E
    # refusals
    bad = seg(val, d_val)[0]
    bad.bytes = 6
    for segments, slots, what in (([], T, "no segments"), ([segs[0]] * 17, T, "17 segments"), ([bad], T, "6 bytes"), ([segs[0]], 0, "0 slots")):
        with pytest.raises(ValueError):
            be.trajectory_store(segments, slots, traj.slots)
    odd = seg(val, d_val)[0]
    odd.src_stride = 6
    rows = seg(blk, d_blk)[0]
    rows.rows = 3  # 8 elements
    null = seg(val, d_val)[0]
    null.dst = None
    for s in (odd, rows, null):
        with pytest.raises(ValueError):
            be.trajectory_store([s], T, traj.slots)
    torch.cuda.synchronize()
    assert traj.slots.cpu().tolist() == [0] * E
    with pytest.raises(RuntimeError):
        Trajectory(env, T, observations=STORE_CASES[case])  # the backend has a reward log already


def _mlp_pair(E, T, episode_length, seed):
    from ai_economist_amd.rollout import MaskedMLPPolicy, Trajectory

    env = _env("gtb_c2", E, seed=seed, episode_length=episode_length, starting_agent_coin=12)
    pol = MaskedMLPPolicy(env.backend, seed=3, record_logp=True, value_head=True)
    return env, pol, Trajectory(env, T)


def test_graphed_step_with_a_trajectory_equals_its_eager_twin():
    import torch

    from ai_economist_amd.rollout import GraphedStep, MaskedMLPPolicy, Trajectory

    E, T, WARM = 6, 4, 3
    N = 2 * T + 1
    env_g, pol_g, traj_g = _mlp_pair(E, T, 5, 5)
    env_e, pol_e, traj_e = _mlp_pair(E, T, 5, 5)
    plain = MaskedMLPPolicy(env_e.backend, seed=3)
    for k in ("wa1", "wa2", "wa3", "wp1", "wp2", "wp3"):  # the value head's weights are drawn behind the six layers'
        assert torch.equal(getattr(plain, k), getattr(pol_e, k))
    with pytest.raises(ValueError):
        GraphedStep(env_e, plain, trajectory=traj_e)  # the trajectory keeps logp and values, the policy has neither
    gs = GraphedStep(env_g, pol_g, auto_reset=True, warmup=WARM, trajectory=traj_g)
    be_e = env_e.backend
    be_e.set_auto_reset(True)
    a_e, p_e = be_e._action_buffers(0)

    def eager(steps):
        for _ in range(steps):
            pol_e(be_e.tensors, a_e, p_e)
            traj_e.store(a_e, p_e, pol_e.logp_a, pol_e.logp_p, pol_e.value_a, pol_e.value_p)
            be_e.step(a_e, p_e)

    eager(WARM)  # the warm-up iterations are real steps and real stores
    torch.cuda.synchronize()
    assert traj_g.slots.cpu().tolist() == [WARM % T] * E
    traj_g.rewind()
    traj_e.rewind()
    gs.replay(N)
    eager(N)
    torch.cuda.synchronize()
    assert traj_g.slots.cpu().tolist() == [N % T] * E == traj_e.slots.cpu().tolist()
    fg, fe = traj_g.flat(), traj_e.flat()
    assert fg["obs"]["obs_a_flat"].shape[0] == T * E and fg["logp_a"].shape[0] == T * E
    for k in ("masks_a", "masks_p", "actions_a", "actions_p", "logp_a", "logp_p", "values_a", "values_p", "done"):
        assert torch.equal(fg[k].contiguous().view(torch.int32), fe[k].contiguous().view(torch.int32)), k
    for k in fg["obs"]:
        assert torch.equal(fg["obs"][k].view(torch.int32), fe["obs"][k].view(torch.int32)), k
    assert torch.equal(traj_g.log.view(torch.int32), traj_e.log.view(torch.int32))
    assert torch.equal(env_g.backend.arena, be_e.arena), "replayed loop != eager loop"
    assert bool(traj_g.logp_a.ne(0).any()) and bool(traj_g.values_a[:T].ne(0).all()) and bool(traj_g.log[..., -1].any())
    assert not bool(traj_g.values_a[T].any())  # row T is finish()'s, no store reaches it


def test_stored_logp_is_the_evaluated_logp_and_advantages_equal_the_reference():
    import torch

    E, T = 7, 8
    env, pol, traj = _mlp_pair(E, T, 3, 8)  # episodes of 3 steps: auto-resets inside the fragment
    be = env.backend
    be.set_auto_reset(True)
    a, p = be._action_buffers(0)
    kept_a, kept_p = [], []

    def policy(tensors, aa, ap):  # a test policy that keeps its own logits of every step
        la, lp = pol.logits(tensors)
        kept_a.append(la.clone())
        kept_p.append(lp.clone())
        be.sample_policy_actions(la, lp, 77, out=(aa, ap, pol.logp_a, pol.logp_p), logp=True)

    for _ in range(2):  # (not at the start of an episode)
        policy(be.tensors, a, p)
        be.step(a, p)
    del kept_a[:], kept_p[:]
    traj.rewind()
    for _ in range(T):
        policy(be.tensors, a, p)
        traj.store(a, p, pol.logp_a, pol.logp_p, pol.value_a, pol.value_p)
        be.step(a, p)
    pol.logits(be.tensors)
    traj.finish(pol.value_a, pol.value_p)
    f = traj.flat()
    logp_a, logp_p, _, _ = be.policy_evaluate(torch.cat(kept_a), torch.cat(kept_p), f["masks_a"], f["masks_p"], f["actions_a"],
                                              f["actions_p"], entropy=False)
    torch.cuda.synchronize()
    assert torch.equal(logp_a.view(torch.int32), f["logp_a"].view(torch.int32))  # importance ratio exactly 1
    assert torch.equal(logp_p.view(torch.int32), f["logp_p"].view(torch.int32))
    assert bool(f["logp_a"].ne(0).any()) and bool(torch.isfinite(f["logp_a"]).all())
    got = traj.advantages(GAMMA, LAM)
    torch.cuda.synchronize()
    log = traj.log.cpu().numpy()
    done = log[:, :, -1] > 0.5
    assert done[: T - 1].any() and not done.all(), "no auto-reset inside the fragment"
    want = gae_ref.from_log(log, 0, T, traj.values_a.cpu().numpy(), traj.values_p.cpu().numpy(), GAMMA, LAM)
    for g, w, name in zip(got, want, ("adv_a", "adv_p", "ret_a", "ret_p")):
        assert np.isfinite(w).all()
        _same_bits(g, w, name)
