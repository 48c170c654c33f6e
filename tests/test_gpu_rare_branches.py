"""The step kernel's rarely taken branches on the device against the CPU oracle: the episode accumulators behind
env.metrics are touched on a trade and on a tax day only, and the price histories are decayed ahead of the components
-- the places where the kernel forms an address (accumulators in the arena, per-lane LDS slots) away from where it
was first needed, so a register allocation that moves them shows here and nowhere in a random rollout's first steps.

Shape: BASELINE configs[1]'s family at its smallest -- 4 agents, the 25 x 25 quadrant layout, 8 replicas -- with a tax
day every second step and one injected state with a hand-built order book per replica (tests/rich_states.py), driven
12 steps by the market script.  The same at 5 agents (the generic kernel) and with rng_mode="fast".  After every step:
record, books, generator key, f64 state and accumulators bit for bit, observations and rewards at OBS_TOL
(tests/test_gpu_parity.py: _compare_all)."""
import numpy as np
import pytest

import rich_states as R
from helpers import C2, GTB, _components_with

E, STEPS = 8, 12
KINDS = ("book_resting_asks", "book_resting_bids", "book_ties", "book_full_bids", "book_full_asks", "tax_escrow",
         "tax_ladder", "coin_extremes")


def _case(n_agents, kernel, **env_kw):
    cfg = dict(C2, n_agents=n_agents, components=_components_with(GTB, PeriodicBracketTax=dict(period=2)))
    return dict(cfg=cfg, kinds=KINDS, E=E, steps=STEPS, seed=31, kernel=kernel, env_kw=env_kw)


CASES = {
    "c2_instance": _case(4, "instance"),
    "5_agents_generic": _case(5, "generic"),
    "c2_fast_rng_instance": _case(4, "instance", rng_mode="fast"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_accumulators_and_price_history_match_oracle(name):
    import torch

    from test_gpu_parity import _compare_all, _compare_metrics
    from test_gpu_rich_states import _pair

    case = CASES[name]
    env, oracle, info = _pair(case)
    be = env.backend
    for e, s in enumerate(R.injected_states(case, env, oracle, info)):
        sub = {k: s[k] for k in R.LOAD_KEYS if k in s}
        be.load_state(sub, e=e)
        oracle.load_state(sub, e=e)
    be.invalidate_observations()
    traded = np.zeros(E, bool)
    tax_days = decays = 0
    for k in range(STEPS):
        a, p = R.injected_actions(case, env, oracle, k, info)
        trades, days = oracle.t["metrics_cda_trades"].copy(), oracle.t["metrics_tax_days"].copy()
        history = oracle.t["cda_price_history"].copy()
        env.step({"a": torch.as_tensor(a, device="cuda:0"), "p": torch.as_tensor(p, device="cuda:0")})
        oracle.step(a, p)
        where = "%s step %d" % (name, k + 1)
        _compare_all(be, oracle, where)
        for key in be.tensors:  # (what _compare_all compares too; here with the promise spelled out: bit for bit)
            if key.startswith("metrics_"):
                got, want = be.tensors[key].cpu().numpy(), oracle.t[key]
                assert got.tobytes() == np.ascontiguousarray(want).astype(got.dtype, copy=False).tobytes(), "%s: %s" % (where, key)
        traded |= (oracle.t["metrics_cda_trades"] != trades).reshape(E, -1).any(1)
        decays += int((history != 0).reshape(E, -1).any(1).sum())  # replicas whose decay had something to multiply
        if (oracle.t["metrics_tax_days"] > days).any():
            tax_days += 1
            _compare_metrics(env, oracle, where)
    assert int(traded.sum()) >= 3, "trades in %d of %d replicas only" % (int(traded.sum()), E)
    assert tax_days >= STEPS // 2 and decays >= 3 * (STEPS // 2), (tax_days, decays)
    assert int(be.tensors["error_flags"].abs().sum()) == 0
