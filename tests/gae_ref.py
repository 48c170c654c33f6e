"""Generalised advantage estimation as every trainer writes it: the plain serial float32 loop, in NumPy.  The reference of
tests/test_trajectory_cpu.py (against the header's aie_gae_step) and tests/test_gpu_trajectory.py (against aie_gae) --
written on its own, not a restatement of the kernel.  NumPy's float32 scalars and arrays round every product and sum to
float32 on its own (no fma)."""
import numpy as np

f32 = np.float32


def gae(rewards, dones, values, gamma, lam):
    """rewards [T, ...], dones [T, ...] (> 0.5 = the episode ended at this step), values [T + 1, ...] (row T: bootstrap)
    -> (advantages [T, ...], returns [T, ...]), float32.  A done step selects: nothing behind it is touched."""
    rewards, values = np.asarray(rewards, f32), np.asarray(values, f32)
    done = np.asarray(dones) > 0.5
    T = rewards.shape[0]
    gamma, gl = f32(gamma), f32(gamma) * f32(lam)
    adv = np.zeros(rewards.shape, f32)
    last = np.zeros(rewards.shape[1:], f32)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            cont = ((rewards[t] + gamma * values[t + 1]) - values[t]) + gl * last
            last = np.where(done[t], rewards[t] - values[t], cont).astype(f32)
            adv[t] = last
        return adv, (adv + values[:T]).astype(f32)


def from_log(log, first_slot, T, values_a, values_p, gamma, lam):
    """The same from a reward log f32 [n_slots, E, n + 2] (agents' rewards, planner's reward, done; time t in slot
    (first_slot + t) % n_slots) -> (adv_a [T, E, n], adv_p [T, E], ret_a, ret_p); a class whose values are None gives None."""
    log = np.asarray(log, f32)
    n = log.shape[2] - 2
    rows = log[(first_slot + np.arange(T)) % log.shape[0]]
    done = rows[:, :, n + 1]
    adv_a = ret_a = adv_p = ret_p = None
    if values_a is not None:
        adv_a, ret_a = gae(rows[:, :, :n], np.repeat(done[:, :, None], n, axis=2), values_a, gamma, lam)
    if values_p is not None:
        adv_p, ret_p = gae(rows[:, :, n], done, values_p, gamma, lam)
    return adv_a, adv_p, ret_a, ret_p


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)
