"""aie_sample_policy_actions_logp, aie_policy_evaluate and aie_policy_evaluate_backward on the device, against the Python
transcription (tests/policy_eval_ref.py, which tests/test_policy_evaluate_cpu.py holds to the header bit for bit):

  * the LOGP sampler picks what aie_sample_policy_actions picks and advances `sample_t` the same way (a twin environment),
    and its logp is the transcription's, bit for bit -- the six row-shape cases of the sampler's own parity test and
    COVID's collated masks, over steps whose masks change, at 1, 5 and 64 replicas;
  * evaluate forward / backward equal the transcription bit for bit: the arena's masks (B = E) and the caller's masks at
    B = 1, 5 and 3 E + 1, with NaN logits, ties, hopeless logits, fully masked rows, disallowed and out-of-range stored
    actions, NULL actor classes and NULL outputs;
  * rollout.masked_logp_entropy: gradients at an MLP's logits against float64 torch autograd (the CPU test's bound: three
    times torch-float32's own error), and the importance ratio of freshly sampled actions is exactly 1;
  * GraphedStep with MaskedMLPPolicy(record_logp=True): the replayed loop equals the eager one (actions, logp, arena).
"""
import math

import numpy as np
import pytest

import policy_eval_ref as ref
from helpers import load_covid_golden, make_env

pytestmark = pytest.mark.gpu
f32 = np.float32

GTB = [["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 5}], ["Gather", {}], ["PeriodicBracketTax", {}]]
C2 = dict(scenario_name="layout_from_file/simple_wood_and_stone", n_agents=4, world_size=[25, 25], episode_length=1000,
          components=GTB, starting_agent_coin=10, env_layout_file="quadrant_25x25_20each_30clump.txt")
CASES = ["gtb_c2", "gtb_multi_action", "one_step_economy", "rows_22_12", "rows_6_52", "rows_6_12_five_agents", "covid"]


def _cfg(case):
    if case == "covid":
        return dict(load_covid_golden("c4_covid_variant")["cfg"], scenario_name="CovidAndEconomySimulation")
    if case == "one_step_economy":
        rs = np.random.RandomState(4)
        return dict(scenario_name="one-step-economy", n_agents=12, world_size=[1, 1], episode_length=3,
                    components=[["SimpleLabor", {"skills": [float(x) for x in np.sort(1 + rs.rand(12) * 2)]}],
                                ["PeriodicBracketTax", {"bracket_spacing": "us-federal", "period": 1, "tax_model": "model_wrapper"}]])
    if case.startswith("rows_"):
        def tax(disc):
            return ["PeriodicBracketTax", {"rate_disc": disc, "period": 10}]
        comps = {"rows_22_12": [["Build", {}], ["ContinuousDoubleAuction", {"max_num_orders": 5, "max_bid_ask": 3}], ["Gather", {}], tax(0.1)],
                 "rows_6_52": [["Build", {}], ["Gather", {}], tax(0.02)],
                 "rows_6_12_five_agents": [["Build", {}], ["Gather", {}], tax(0.1)]}[case]
        return dict(C2, episode_length=30, components=comps, n_agents=5 if case.endswith("five_agents") else 4)
    return dict(C2, episode_length=30, multi_action_mode_agents=(case == "gtb_multi_action"),
                multi_action_mode_planner=(case != "gtb_multi_action"))


def _rows(env, case, be):
    """{"a": [(offset, length)] per action column, "p": ...}: the sampler's rows inside one actor's logits."""
    if case == "covid":
        return {"a": [(0, be.tensors["obs_a_action_mask"].shape[1])], "p": [(0, be.tensors["obs_p_action_mask"].shape[-1])]}
    from ai_economist_amd.foundation.obs_keys import mask_keys

    tab = mask_keys(env)
    rows = {}
    for who, multi in (("a", env.multi_action_mode_agents), ("p", env.multi_action_mode_planner)):
        if multi and tab[who]:
            rows[who] = [(off - 1, size + 1) for _, off, size in tab[who]]
        else:
            rows[who] = [(0, tab["sizes"][who])]
    return rows


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _want_forward(rows, logits, masks, actions):
    """logits / masks [B, actors, W], actions [B, actors, width] -> (logp, entropy) [B, actors, width]."""
    B, A, _ = logits.shape
    lp, H = np.zeros(actions.shape, f32), np.zeros(actions.shape, f32)
    for s, (lo, ln) in enumerate(rows):
        a, b = ref.rows_forward(logits[:, :, lo:lo + ln].reshape(B * A, ln), masks[:, :, lo:lo + ln].reshape(B * A, ln),
                                actions[:, :, s].reshape(-1))
        lp[:, :, s], H[:, :, s] = a.reshape(B, A), b.reshape(B, A)
    return lp, H


def _want_backward(rows, logits, masks, actions, gl, gh):
    B, A, _ = logits.shape
    g = np.zeros(logits.shape, f32)
    for s, (lo, ln) in enumerate(rows):
        g[:, :, lo:lo + ln] = ref.rows_backward(logits[:, :, lo:lo + ln].reshape(B * A, ln), masks[:, :, lo:lo + ln].reshape(B * A, ln),
                                                actions[:, :, s].reshape(-1), gl[:, :, s].reshape(-1),
                                                gh[:, :, s].reshape(-1)).reshape(B, A, ln)
    return g


def _same(got, want, what):
    got, want = got.detach().cpu().numpy().reshape(want.shape), np.asarray(want, f32)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r, want %r" % (
        what, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])


def _check_evaluate(be, rows, la, lp, ma, mp, aa, ap, rng, what, arena_masks=False):
    """forward and backward of one batch (numpy operands, [B, ...]) against the transcription."""
    import torch

    dev = be.device
    t = lambda x: torch.as_tensor(x).to(dev)  # noqa: E731
    B = la.shape[0]
    n = la.shape[1]
    got = be.policy_evaluate(t(la), t(lp), None if arena_masks else t(ma), None if arena_masks else t(mp), t(aa), t(ap))
    wla, wHa = _want_forward(rows["a"], la, ma, aa)
    wlp, wHp = _want_forward(rows["p"], lp[:, None, :], mp[:, None, :], ap[:, None, :])
    _same(got[0], wla, what + ": agents' logp")
    _same(got[1], wlp[:, 0], what + ": planner's logp")
    _same(got[2], wHa, what + ": agents' entropy")
    _same(got[3], wHp[:, 0], what + ": planner's entropy")
    gla, gha = rng.randn(*aa.shape).astype(f32), rng.randn(*aa.shape).astype(f32)
    glp, ghp = rng.randn(*ap.shape).astype(f32), rng.randn(*ap.shape).astype(f32)
    ga, gp = be.policy_evaluate_backward(t(la), t(lp), None if arena_masks else t(ma), None if arena_masks else t(mp), t(aa), t(ap),
                                         t(gla), t(glp), t(gha), t(ghp))
    wga = _want_backward(rows["a"], la, ma, aa, gla, gha)
    wgp = _want_backward(rows["p"], lp[:, None, :], mp[:, None, :], ap[:, None, :], glp[:, None, :], ghp[:, None, :])
    _same(ga, wga, what + ": agents' gradient")
    _same(gp, wgp[:, 0], what + ": planner's gradient")
    assert not ga.cpu().numpy().reshape(ma.shape)[ma < 0.5].any() and not gp.cpu().numpy()[mp < 0.5].any()
    return got


@pytest.mark.parametrize("E", [1, 5, 64])
@pytest.mark.parametrize("case", CASES)
def test_logp_sampler_and_evaluate_equal_the_transcription(case, E):
    import torch

    cfg = _cfg(case)
    envs = []
    for _ in range(2):
        env = make_env(cfg, n_envs=E, device="cuda:0", env_offset=1000)
        if case != "covid":
            env.seed(3)
        env.reset()
        envs.append(env)
    env, twin = envs
    be, bt = env.backend, twin.backend
    rows = _rows(env, case, be)
    n = be.n
    WA = sum(ln for _, ln in rows["a"]) if case != "covid" else rows["a"][0][1]
    MP = be.tensors["obs_p_action_mask"].shape[-1]
    g = torch.Generator(device="cpu").manual_seed(11)
    rng = np.random.RandomState(7)
    T = int(cfg["episode_length"]) if case != "covid" else 1 << 30
    traj = []
    steps = 12 if E == 64 else 8
    masks_seen = set()
    for t in range(steps):
        la = (torch.randn(E, n, WA, generator=g) * 3).float()
        lp = (torch.randn(E, MP, generator=g) * 3).float()
        la[t % E, 0, 1:4] = float("nan")           # NaN logits are masked entries
        la[(t + 1) % E, 1 % n, :] = 0.25            # all-equal logits
        lp[(t + 2) % E, :] = -1e30                  # hopeless logits
        la[(t + 3) % E, 2 % n, :] = float("nan")    # a fully NaN row: NO-OP, logp 0
        if t % 3 == 2:
            la[(t + 4) % E, 3 % n, 1:] = -200.0     # entries 80 and more below the maximum: weight 0, finite logp
        wa, wp = bt.sample_policy_actions(la.to("cuda:0"), lp.to("cuda:0"), seed=77, env_offset=1000)
        a, p, ga, gp = be.sample_policy_actions(la.to("cuda:0"), lp.to("cuda:0"), seed=77, env_offset=1000, logp=True)
        torch.cuda.synchronize()
        assert torch.equal(a, wa) and torch.equal(p, wp), "step %d: the LOGP sampler picks differently" % t
        assert torch.equal(be.tensors["sample_t"], bt.tensors["sample_t"]) and int(be.tensors["sample_t"][0]) == t + 1
        ma, mp = be.action_masks()
        if case == "covid":
            assert torch.equal(ma, be.tensors["obs_a_action_mask"].transpose(1, 2))
        else:
            assert torch.equal(ma, be.tensors["obs_a_action_mask"])
        assert torch.equal(mp, be.tensors["obs_p_action_mask"])
        lah, lph, mah, mph = la.numpy(), lp.numpy(), ma.cpu().numpy(), mp.cpu().numpy()
        aah, aph = a.cpu().numpy(), p.cpu().numpy()
        masks_seen.add(mah.tobytes() + mph.tobytes())
        wla, _ = _want_forward(rows["a"], lah, mah, aah)
        wlp, _ = _want_forward(rows["p"], lph[:, None, :], mph[:, None, :], aph[:, None, :])
        _same(ga, wla, "step %d: agents' logp of the picks" % t)
        _same(gp, wlp[:, 0], "step %d: planner's logp of the picks" % t)
        assert (aah[(t + 3) % E, 2 % n] == 0).all() and not ga.cpu().numpy()[(t + 3) % E, 2 % n].any()
        if t % 4 == 0:  # evaluate under the arena's masks (B = E): the sampled actions' logp, bit for bit
            got = _check_evaluate(be, rows, lah, lph, mah, mph, aah, aph, rng, "step %d, arena masks" % t, arena_masks=True)
            assert torch.equal(got[0].view(torch.int32), ga.view(torch.int32)) and torch.equal(got[1].view(torch.int32), gp.view(torch.int32))
        traj.append((lah, lph, mah, mph, aah, aph))
        env.step({"a": a, "p": p})
        twin.step({"a": wa, "p": wp})
        if (t + 1) % T == 0:
            env.reset(be.tensors["done"])
            twin.reset(bt.tensors["done"])
    assert len(masks_seen) > 1, "the masks never changed"
    assert torch.equal(be.arena, bt.arena)
    # ---- the caller's masks, B = 1, 5, 3 E + 1: stored steps, new logits, a few spoiled rows ----
    cat = [np.concatenate([s[k] for s in traj]) for k in range(6)]
    for B in (1, 5, 3 * E + 1):
        idx = rng.permutation(len(cat[0]))[:B]
        assert len(idx) == B
        la, lp, ma, mp, aa, ap = (c[idx].copy() for c in cat)
        la = (la + rng.randn(*la.shape).astype(f32)).astype(f32)
        lp = (lp + rng.randn(*lp.shape).astype(f32)).astype(f32)
        if B > 1:
            ma[0, 0, :] = 0.0                                  # a fully masked row
            mp[B - 1, :] = 0.0
            lo, ln = rows["a"][-1]
            aa[1, n - 1, -1] = ln                               # a stored action outside its row
            dis = np.flatnonzero(mp[0, :rows["p"][0][1]] < 0.5)
            if dis.size:
                ap[0, 0] = dis[0]                               # a stored action its mask does not allow
            aa[2 % B, 0, 0] = -1
        _check_evaluate(be, rows, la, lp, ma, mp, aa, ap, rng, "caller masks, B = %d" % B)


def test_null_actor_classes_and_null_outputs():
    import torch

    E = 8
    env = make_env(dict(C2, episode_length=30), n_envs=E, device="cuda:0")
    env.seed(2)
    env.reset()
    be = env.backend
    rows = _rows(env, "gtb_c2", be)
    rng = np.random.RandomState(3)
    for _ in range(3):
        a, p = be.sample_masked_actions(seed=5)
        env.step({"a": a, "p": p})
    ma, mp = be.action_masks()
    la = torch.randn(ma.shape, device="cuda:0") * 2
    lp = torch.randn(mp.shape, device="cuda:0") * 2
    a, p, ga, gp = be.sample_policy_actions(la, lp, seed=1, logp=True)
    a, p, ga, gp = a.clone(), p.clone(), ga.clone(), gp.clone()
    wHa = _want_forward(rows["a"], la.cpu().numpy(), ma.cpu().numpy(), a.cpu().numpy())[1]
    wHp = _want_forward(rows["p"], lp.cpu().numpy()[:, None], mp.cpu().numpy()[:, None], p.cpu().numpy()[:, None])[1][:, 0]
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    SENT = 12345.0

    def fresh():
        return [torch.full(a.shape, SENT, device="cuda:0"), torch.full(p.shape, SENT, device="cuda:0"),
                torch.full(a.shape, SENT, device="cuda:0"), torch.full(p.shape, SENT, device="cuda:0")]

    # forward: every subset of the four outputs; an actor class without outputs may have NULL inputs
    for keep in range(1, 16):
        out = fresh()
        use = [out[i] if keep >> i & 1 else None for i in range(4)]
        need_a, need_p = use[0] is not None or use[2] is not None, use[1] is not None or use[3] is not None
        be._check(be.lib.aie_policy_evaluate(
            be.handle, E, P(la) if need_a else None, P(lp) if need_p else None, P(ma) if need_a else None, P(mp) if need_p else None,
            P(a) if use[0] is not None else None, P(p) if use[1] is not None else None, P(use[0]), P(use[1]), P(use[2]), P(use[3]), None))
        torch.cuda.synchronize()
        for i, want in enumerate((ga, gp, wHa, wHp)):
            if use[i] is None:
                assert bool((out[i] == SENT).all())
            elif i < 2:
                assert torch.equal(out[i].view(torch.int32), want.view(torch.int32)), keep
            else:
                _same(out[i], want, "entropy, outputs %d" % keep)
    # the LOGP sampler: NULL pairs as aie_sample_policy_actions; an action buffer without its logp buffer is refused
    before_a, before_ga = a.clone(), ga.clone()
    be._check(be.lib.aie_sample_policy_actions_logp(be.handle, None, P(lp), 77, 0, None, P(p), None, P(gp), None))
    torch.cuda.synchronize()
    assert torch.equal(a, before_a) and torch.equal(ga, before_ga)
    assert be.lib.aie_sample_policy_actions_logp(be.handle, P(la), P(lp), 77, 0, P(a), P(p), None, P(gp), None) != 0
    assert be.lib.aie_sample_policy_actions_logp(be.handle, None, None, 77, 0, P(a), None, P(ga), None, None) != 0
    # backward: one actor class only, NULL incoming gradients (= zeros)
    gl = torch.randn(a.shape, device="cuda:0")
    grad_a, grad_p = torch.full(la.shape, SENT, device="cuda:0"), torch.full(lp.shape, SENT, device="cuda:0")
    be._check(be.lib.aie_policy_evaluate_backward(be.handle, E, P(la), None, P(ma), None, P(a), None, P(gl), None, None, None,
                                                  P(grad_a), None, None))
    torch.cuda.synchronize()
    want = _want_backward(rows["a"], la.cpu().numpy(), ma.cpu().numpy(), a.cpu().numpy(), gl.cpu().numpy(), np.zeros(a.shape, f32))
    _same(grad_a, want, "agents only, no entropy gradient")
    assert bool((grad_p == SENT).all())
    be._check(be.lib.aie_policy_evaluate_backward(be.handle, E, None, P(lp), None, P(mp), None, None, None, None, None, None,
                                                  None, P(grad_p), None))
    torch.cuda.synchronize()
    assert not grad_p.any()  # no incoming gradient at all: zeros
    # refusals: B != E without the caller's masks; an output without its logits
    assert be.lib.aie_policy_evaluate(be.handle, E + 1, P(la), None, None, None, P(a), None, P(ga), None, None, None, None) != 0
    assert be.lib.aie_policy_evaluate(be.handle, E, None, None, None, None, P(a), None, P(ga), None, None, None, None) != 0


def test_masked_logp_entropy_gradients_and_importance_ratio():
    import torch

    from ai_economist_amd.rollout import MaskedMLPPolicy, masked_logp_entropy

    E = 256
    env = make_env(dict(C2, episode_length=30), n_envs=E, device="cuda:0")
    env.seed(4)
    env.reset()
    be = env.backend
    pol = MaskedMLPPolicy(be, seed=2, record_logp=True)
    a, p = be._action_buffers(0)
    for _ in range(5):
        pol(be.tensors, a, p)
        env.step({"a": a, "p": p})
    pol(be.tensors, a, p)  # the stored step: observations -> logits -> actions, logp
    ma, mp = be.action_masks()
    la, lp = pol.logits(be.tensors)
    la = la.view(E, be.n, -1).detach().requires_grad_(True)
    lp = lp.detach().requires_grad_(True)
    logp_a, logp_p, ent_a, ent_p = masked_logp_entropy(be, la, lp, ma, mp, a, p)
    # the importance ratio of the step that was just sampled is exactly 1
    assert torch.equal(logp_a.detach().view(torch.int32), pol.logp_a.view(torch.int32))
    assert torch.equal(logp_p.detach().view(torch.int32), pol.logp_p.view(torch.int32))
    assert bool((torch.exp(logp_a.detach() - pol.logp_a) == 1.0).all())
    adv_a = torch.randn(logp_a.shape, device="cuda:0")
    adv_p = torch.randn(logp_p.shape, device="cuda:0")
    loss = -(logp_a * adv_a).sum() - (logp_p * adv_p).sum() - 0.05 * (ent_a.sum() + ent_p.sum())
    loss.backward()
    assert la.grad.shape == la.shape and lp.grad.shape == lp.shape

    def torch_grad(x, m, act, adv, dtype, rows):  # the torch formulation, per row, on the host
        x = x.detach().cpu().to(dtype).requires_grad_(True)
        m, act, adv = m.cpu() > 0.5, act.cpu().long(), adv.cpu().to(dtype)
        total = 0
        for s, (lo, ln) in enumerate(rows):
            lsm = torch.log_softmax(x[..., lo:lo + ln].masked_fill(~m[..., lo:lo + ln], -math.inf), -1)
            lg = lsm.gather(-1, act[..., s:s + 1])[..., 0]
            H = -(lsm.exp() * lsm.masked_fill(~m[..., lo:lo + ln], 0.0)).sum(-1)
            total = total - (lg * adv[..., s]).sum() - 0.05 * H.sum()
        total.backward()
        return x.grad.double().numpy()

    rows = _rows(env, "gtb_c2", be)
    for who, x, m, act, adv, r in (("agents", la, ma, a, adv_a, rows["a"]),
                                   ("planner", lp[:, None], mp[:, None], p[:, None], adv_p[:, None], rows["p"])):
        want = torch_grad(x, m, act, adv, torch.float64, r)
        t32 = torch_grad(x, m, act, adv, torch.float32, r)
        got = (la.grad if who == "agents" else lp.grad[:, None]).double().cpu().numpy()
        eo, et = np.abs(got - want).max(), np.abs(t32 - want).max()
        print("%s: gradient max error %.3e, torch-float32's %.3e, ratio %.2f" % (who, eo, et, eo / et))
        assert eo <= 3.0 * et, who
        assert not got[(m.cpu().numpy() < 0.5)].any(), who


def test_record_logp_is_hipgraph_replayable():
    """policy (with record_logp) -> aie_step captured once and replayed equals the same loop issued call by call: the
    actions, the log-probabilities and the whole arena, bit for bit (the pattern of test_step_is_hipgraph_replayable)."""
    import torch

    from ai_economist_amd.rollout import GraphedStep, MaskedMLPPolicy

    cfg = dict(C2, episode_length=40, starting_agent_coin=12)
    E, WARM, N = 48, 3, 48

    def start():
        env = make_env(cfg, n_envs=E, device="cuda:0")
        env.seed(5)
        env.reset()
        return env

    env_g, env_e = start(), start()
    pol_g = MaskedMLPPolicy(env_g.backend, seed=3, record_logp=True)
    pol_e = MaskedMLPPolicy(env_e.backend, seed=3, record_logp=True)
    gs = GraphedStep(env_g, pol_g, auto_reset=True, warmup=WARM)
    be_e = env_e.backend
    be_e.set_auto_reset(True)
    a_e, p_e = be_e._action_buffers(0)
    for t in range(WARM + N):
        pol_e(be_e.tensors, a_e, p_e)
        be_e.step(a_e, p_e)
    gs.replay(N)
    torch.cuda.synchronize()
    assert int(be_e.tensors["sample_t"][0]) == WARM + N
    assert torch.equal(gs.actions_a, a_e) and torch.equal(gs.actions_p, p_e)
    assert torch.equal(pol_g.logp_a.view(torch.int32), pol_e.logp_a.view(torch.int32))
    assert torch.equal(pol_g.logp_p.view(torch.int32), pol_e.logp_p.view(torch.int32))
    assert bool((pol_e.logp_a <= 0).all()) and bool(pol_e.logp_a.ne(0).any())
    assert torch.equal(env_g.backend.arena, be_e.arena), "replayed loop != eager loop"
    assert bool(torch.isfinite(pol_e.logp_p).all())
