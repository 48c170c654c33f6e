"""aie_ppo_loss on the device (Backend.ppo_loss, rollout.ppo_loss, Trajectory.ppo_batch) against the Python transcription
(tests/ppo_ref.py, which tests/test_ppo_loss_cpu.py holds to the header bit for bit):

  * the four row-shape families (C2: agents in 64-lane segments and the generic 7-slot planner; COVID: 16-lane segments,
    four actors to a wave, a partial last wave; ragged multi-action agents; rows of 6 and 52) at B = 1, 5 and 67 with the
    CPU test's edges planted: gradients and value gradients bit for bit with every entry written (the buffers start as
    NaN), the skipped count and max |d| exact, the means within the bound another order of float64 summation may differ
    by (ppo_ref.statistics); a NULL class, NULL values, moments;
  * a minibatch by index (repeats, out of order) equals the same call on index_select copies, statistics included;
  * more work items than twice the launched wavefronts: the strided loop, and a second run gives the same bits;
  * rollout.ppo_loss through a torch.nn MLP per class against the float64 torch formulation (3 x torch-float32's error),
    and the incoming gradient scales the result;
  * Trajectory.ppo_batch after a graphed rollout: the first loss of a fragment has kl 0, clip fraction 0, nothing skipped;
  * one call captured in a graph: two replays and the eager call give the same bits.
"""
import math

import numpy as np
import pytest

import ppo_ref as ref
from helpers import make_env
from test_gpu_policy_evaluate import C2, _cfg, _rows

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
COEFS = dict(clip=0.3, vf_clip=50.0, vf_coef=0.05, ent_coef=0.025)
COEFS_P = dict(clip=0.2, vf_coef=0.5, ent_coef=0.1)  # the planner's own, where a test gives it some
CASES = {"gtb_c2": 5, "covid": 1, "gtb_multi_action": 5, "rows_6_52": 1}  # n_envs: B is not tied to it
_ENVS = {}


def _env(case):
    if case not in _ENVS:
        env = make_env(_cfg(case), n_envs=CASES[case], device=DEV)
        if case != "covid":
            env.seed(3)
        env.reset()
        be = env.backend
        ma, mp = be.action_masks()
        rows = _rows(env, case, be)
        WA, MP = int(ma.shape[-1]), int(mp.shape[-1])
        assert sum(ln for _, ln in rows["a"]) == WA and sum(ln for _, ln in rows["p"]) == MP  # the rows cover the logits
        _ENVS[case] = (env, be, rows, WA, MP)
    return _ENVS[case]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _batches(case, B, seed, edges=True, moments=(None, None)):
    """numpy operands of both classes, [B, actors, ...], with the edges planted where the batch has room."""
    _, be, rows, WA, MP = _env(case)
    ba = ref.random_batch(rows["a"], WA, B, be.n, seed)
    bp = ref.random_batch(rows["p"], MP, B, 1, seed + 1)
    where = (None, None)
    if edges:
        where = (ref.plant_edges(rows["a"], ba, seed + 2, COEFS["vf_clip"], moments[0]),
                 ref.plant_edges(rows["p"], bp, seed + 3, COEFS["vf_clip"], moments[1]))
    return ba, bp, where


def _stored(ba, bp):
    """The dict Backend.ppo_loss takes, on the device (the planner's tensors without the actor dimension)."""
    import torch

    out = {}
    for who, b in (("a", ba), ("p", bp)):
        if b is None:
            continue
        for k in ("masks", "actions", "logp_old", "adv", "values_old", "returns"):
            v = b[k] if who == "a" else b[k][:, 0]
            out["%s_%s" % (k, who)] = torch.as_tensor(np.ascontiguousarray(v)).to(DEV)
    return out


def _net(b, who, key):
    import torch

    return None if b is None else torch.as_tensor(np.ascontiguousarray(b[key] if who == "a" else b[key][:, 0])).to(DEV)


def _run(be, ba, bp, values=True, moments=(None, None), coeffs_p=None, index=None, stored=None, coefs=COEFS):
    """One call into NaN-filled buffers -> per class (stats, grad, grad_v) as numpy, or None."""
    import torch

    la, lp = _net(ba, "a", "logits"), _net(bp, "p", "logits")
    va, vp = (_net(ba, "a", "values"), _net(bp, "p", "values")) if values else (None, None)
    nan = lambda t: None if t is None else torch.full_like(t, float("nan"))  # noqa: E731
    out = tuple((torch.full((8,), float("nan"), device=DEV), nan(lg), nan(v)) if lg is not None else None
                for lg, v in ((la, va), (lp, vp)))
    mom = tuple(None if m is None else torch.tensor(m, dtype=torch.float32, device=DEV) for m in moments)
    got = be.ppo_loss(la, lp, va, vp, stored if stored is not None else _stored(ba, bp), index=index, coeffs_p=coeffs_p,
                      adv_moments=mom, out=out, **coefs)
    torch.cuda.synchronize()
    for g, o in zip(got, out):
        assert (g is None) == (o is None) and (g is None or all(x is y for x, y in zip(g, o)))
    return tuple(None if o is None else tuple(None if t is None else t.cpu().numpy() for t in o) for o in out)


def _want(rows, b, values=True, moments=None, coefs=COEFS):
    return ref.ppo_class(rows, b["logits"], b["masks"], b["actions"], b["logp_old"], b["adv"], b["values"] if values else None,
                         b["values_old"], b["returns"], moments=moments, **coefs)


def _hold(got, want, what):
    stats, grad, grad_v = got
    bad = np.flatnonzero(bits(grad).reshape(-1) != bits(want["grad"]).reshape(-1))
    assert bad.size == 0, "%s: %d of %d gradient entries differ, first at %d: got %r, want %r" % (
        what, bad.size, grad.size, bad[0], grad.reshape(-1)[bad[0]], want["grad"].reshape(-1)[bad[0]])
    assert (grad_v is None) == (want["grad_v"] is None), what
    if grad_v is not None:
        assert np.array_equal(bits(grad_v).reshape(-1), bits(want["grad_v"]).reshape(-1)), what + ": value gradients"
    assert stats[6] == want["stats"][6] and bits(stats[7]) == bits(want["stats"][7]), (what, stats, want["stats"])
    err = np.abs(stats[:6].astype(np.float64) - want["stats"][:6].astype(np.float64))
    print("%s: stats %s, |error| %s, bound %s" % (what, stats, err, want["tol"][:6]))
    assert (err <= want["tol"][:6]).all(), "%s: stats %s, want %s, bound %s" % (what, stats[:6], want["stats"][:6], want["tol"][:6])


@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("case", list(CASES))
def test_device_equals_the_transcription(case, B):
    _, be, rows, _, _ = _env(case)
    coefs_p = dict(COEFS, **COEFS_P)
    ba, bp, where = _batches(case, B, seed=10 * B + len(case))
    if B == 67:
        assert set(where[0]) == set(ref.EDGES) == set(where[1])
    got = _run(be, ba, bp, coeffs_p=COEFS_P)
    want_a, want_p = _want(rows["a"], ba), _want(rows["p"], bp, coefs=coefs_p)
    _hold(got[0], want_a, "%s B=%d agents" % (case, B))
    _hold(got[1], want_p, "%s B=%d planner" % (case, B))
    if B == 67:
        assert want_a["stats"][6] == 6 and want_p["stats"][6] == 6 and want_p["stats"][7] > 79 and want_a["stats"][5] > 0
        # the CPU test's coefficient variants: r exactly on either clip bound (1 - r and r - 1 are exact), and vf_clip = 0
        r = {(who, e): ref.ratio_of(rows[who], b, w[e]) for who, b, w in (("a", ba, where[0]), ("p", bp, where[1]))
             for e in ("r_at_lo", "r_at_hi")}
        for what, ca, cp in (("r at lo_c", dict(clip=float(f32(1) - r["a", "r_at_lo"])), dict(clip=float(f32(1) - r["p", "r_at_lo"]))),
                             ("r at hi_c", dict(clip=float(r["a", "r_at_hi"] - f32(1))), dict(clip=float(r["p", "r_at_hi"] - f32(1)))),
                             ("vf_clip 0", dict(vf_clip=0.0), dict(vf_clip=0.0))):
            var = _run(be, ba, bp, coeffs_p=dict(COEFS_P, **cp), coefs=dict(COEFS, **ca))
            for g, w, who, b, wh in ((var[0], _want(rows["a"], ba, coefs=dict(COEFS, **ca)), "a", ba, where[0]),
                                     (var[1], _want(rows["p"], bp, coefs=dict(coefs_p, **cp)), "p", bp, where[1])):
                _hold(g, w, "%s B=%d %s, %s" % (case, B, who, what))
                for e, bound in (("r_at_lo", "lo_c"), ("r_at_hi", "hi_c")):
                    if what == "r at " + bound:
                        assert 0.5 < r[who, e] < 2 and w["r"][wh[e]] == w[bound] and w["valid"][wh[e]]
                        assert w["clipf"][wh[e]] == 0 and w["unclipped"][wh[e]]
                if what == "vf_clip 0":
                    e1 = (b["values"] - b["returns"]).astype(f32).reshape(-1)
                    assert np.array_equal(bits(w["vf"]), bits((e1 * e1).astype(f32)))
                    assert np.array_equal(bits(g[2]).reshape(-1), bits((w["kv"] * (e1 + e1).astype(f32)).astype(f32)))
    # a NULL class: the other class's results hold as before (its sums run in another order: fewer work items)
    only_a, only_p = _run(be, ba, None), _run(be, None, bp, coeffs_p=COEFS_P)
    assert only_a[1] is None and only_p[0] is None
    _hold(only_a[0], want_a, "%s B=%d agents alone" % (case, B))
    _hold(only_p[1], want_p, "%s B=%d planner alone" % (case, B))
    # no values: no value term, no value gradient
    nv = _run(be, ba, bp, values=False, coeffs_p=COEFS_P)
    _hold(nv[0], _want(rows["a"], ba, values=False), "%s B=%d agents, no values" % (case, B))
    _hold(nv[1], _want(rows["p"], bp, values=False, coefs=coefs_p), "%s B=%d planner, no values" % (case, B))
    assert nv[0][0][2] == 0 and nv[0][2] is None
    # moments on the device, one class with and one without
    mom = ((0.3, 1.7), None)
    ba, bp, _ = _batches(case, B, seed=10 * B + len(case), moments=mom)
    got = _run(be, ba, bp, moments=mom)
    _hold(got[0], _want(rows["a"], ba, moments=mom[0]), "%s B=%d agents, moments" % (case, B))
    _hold(got[1], _want(rows["p"], bp), "%s B=%d planner beside moments" % (case, B))


def test_refusals():
    import torch

    from ai_economist_amd import _cabi

    _, be, rows, _, _ = _env("gtb_c2")
    ba, bp, _ = _batches("gtb_c2", 3, seed=1, edges=False)
    st = _stored(ba, bp)
    la, lp, va, vp = _net(ba, "a", "logits"), _net(bp, "p", "logits"), _net(ba, "a", "values"), _net(bp, "p", "values")
    with pytest.raises(Exception):
        be.ppo_loss(la, lp, va, vp, st, clip=0.0)
    with pytest.raises(ValueError):
        be.ppo_loss(la, lp, va, vp, dict(st, actions_a=st["actions_a"].long()))
    with pytest.raises(ValueError):
        be.ppo_loss(la, lp, va, vp, dict(st, adv_p=st["adv_p"][:2]))
    with pytest.raises(ValueError):
        be.ppo_loss(la, lp, va, vp, st, index=torch.zeros(3, dtype=torch.int64, device=DEV))
    assert be.lib.aie_ppo_workspace_bytes(be.handle, 3) == 3 * (be.n + 1) * 128
    assert be._ppo_ws.numel() * 8 == 128 * _cabi.PPO_MAX_WAVES  # one workspace per backend, large enough for every B
    assert be.lib.aie_ppo_workspace_bytes(be.handle, 0) < 0
    assert be.lib.aie_ppo_workspace_bytes(be.handle, 10 ** 9) == 128 * _cabi.PPO_MAX_WAVES
    torch.cuda.synchronize()


def test_minibatch_by_index_equals_the_gathered_copies():
    import torch

    _, be, rows, _, _ = _env("gtb_c2")
    R, B = 200, 67
    sa, sp, _ = _batches("gtb_c2", R, seed=77)  # the stored fragment, edges included
    rng = np.random.RandomState(5)
    idx = rng.randint(0, R, B)
    idx[:6] = [199, 0, 199, 3, 3, 198]  # repeats, out of order, both ends
    assert len(set(idx.tolist())) < B and (np.diff(idx) < 0).any() and idx.min() >= 0 and idx.max() < R
    na, np_, _ = _batches("gtb_c2", B, seed=78, edges=False)  # the networks' outputs of the minibatch
    ga = {k: (na[k] if k in ("logits", "values") else sa[k][idx]) for k in sa}
    gp = {k: (np_[k] if k in ("logits", "values") else sp[k][idx]) for k in sp}
    index = torch.as_tensor(idx.astype(np.int32)).to(DEV)
    by_index = _run(be, ga, gp, index=index, stored=_stored(sa, sp), coeffs_p=COEFS_P)
    stored = _stored(sa, sp)
    copies = {k: v.index_select(0, index.long()).contiguous() for k, v in stored.items()}
    by_copy = _run(be, ga, gp, stored=copies, coeffs_p=COEFS_P)
    for x, y in zip(by_index, by_copy):
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(x, y))
    _hold(by_index[0], _want(rows["a"], ga), "index, agents")
    _hold(by_index[1], _want(rows["p"], gp, coefs=dict(COEFS, **COEFS_P)), "index, planner")
    assert by_index[0][0][6] > 0  # (the fragment's planted edges reached the minibatch)


def test_more_work_items_than_wavefronts():
    from ai_economist_amd import _cabi

    _, be, rows, WA, MP = _env("covid")
    items = -(-be.n // (64 // pref_segment(WA))) + 1  # the agents' waves per batch element, and the planner's
    B = 2 * _cabi.PPO_MAX_WAVES // items + 3
    work = B * items
    assert work > 2 * _cabi.PPO_MAX_WAVES and work % _cabi.PPO_MAX_WAVES and be.n % 4  # strided, ragged end, partial wave
    ba, bp, _ = _batches("covid", B, seed=4)
    assert sum(v.nbytes for v in ba.values()) < 16 << 20
    first = _run(be, ba, bp)
    _hold(first[0], _want(rows["a"], ba), "grid-stride, agents")
    _hold(first[1], _want(rows["p"], bp), "grid-stride, planner")
    again = _run(be, ba, bp)
    for x, y in zip(first, again):
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(x, y))


def pref_segment(n):
    import policy_eval_ref

    return policy_eval_ref.segment(n)


def _torch_class_loss(rows, logits, values, st, who, coefs, dtype):
    """One class's loss as plain torch in `dtype` from logits [B, actors, W] and values [B, actors] (device tensors with
    a graph), the stored operands from the dict."""
    import torch

    t = lambda k: st["%s_%s" % (k, who)].reshape(logits.shape[:2] + (-1,))  # noqa: E731
    allowed, act = t("masks") > 0.5, t("actions").long()
    logp = ent = 0
    for s, (lo, ln) in enumerate(rows):
        ok = allowed[..., lo:lo + ln]
        lsm = torch.log_softmax(logits[..., lo:lo + ln].masked_fill(~ok, -math.inf), -1)
        logp = logp + lsm.gather(-1, act[..., s:s + 1])[..., 0]
        ent = ent - (lsm.exp() * lsm.masked_fill(~ok, 0.0)).sum(-1)
    adv, vo, rt = (t(k)[..., 0].to(dtype) for k in ("adv", "values_old", "returns"))
    ratio = (logp - t("logp_old").to(dtype).sum(-1)).exp()
    pol = -torch.min(ratio * adv, ratio.clamp(1 - coefs["clip"], 1 + coefs["clip"]) * adv).mean()
    vc = vo + (values - vo).clamp(-coefs["vf_clip"], coefs["vf_clip"])
    vf = torch.max((values - rt) ** 2, (vc - rt) ** 2).mean()
    return pol + coefs["vf_coef"] * vf - coefs["ent_coef"] * ent.mean()


def test_rollout_ppo_loss_through_an_mlp():
    import torch

    from ai_economist_amd import rollout

    _, be, rows, WA, MP = _env("gtb_c2")
    B, F, HID = 64, 24, 32
    ba, bp, _ = _batches("gtb_c2", B, seed=31, edges=False)
    st = _stored(ba, bp)
    torch.manual_seed(3)
    nets = {"a": torch.nn.Sequential(torch.nn.Linear(F, HID), torch.nn.Tanh(), torch.nn.Linear(HID, WA + 1)).to(DEV),
            "p": torch.nn.Sequential(torch.nn.Linear(F, HID), torch.nn.Tanh(), torch.nn.Linear(HID, MP + 1)).to(DEV)}
    feats = {"a": torch.randn(B, be.n, F, device=DEV), "p": torch.randn(B, 1, F, device=DEV)}
    coefs_p = dict(COEFS, **COEFS_P)
    with torch.no_grad():  # the stored logp: the nets' own distribution a small step ago, so the ratios are near 1
        near = {who: net(feats[who])[..., :-1] + 0.05 * torch.randn(B, feats[who].shape[1], w, device=DEV)
                for (who, net), w in zip(nets.items(), (WA, MP))}
        st["logp_old_a"], st["logp_old_p"], _, _ = be.policy_evaluate(near["a"], near["p"][:, 0], st["masks_a"], st["masks_p"],
                                                                      st["actions_a"], st["actions_p"], entropy=False)
    assert bool(torch.isfinite(st["logp_old_a"]).all()) and bool(torch.isfinite(st["logp_old_p"]).all())

    def outputs(dtype):
        out = {}
        for who, net in nets.items():
            net.to(dtype)
            net.zero_grad()
            y = net(feats[who].to(dtype))
            out[who] = (y[..., :-1], y[..., -1])
        return out

    def grads():
        got = {who: torch.cat([p.grad.double().reshape(-1) for p in net.parameters()]).cpu().numpy() for who, net in nets.items()}
        return got

    def torch_form(dtype):
        o = outputs(dtype)
        (_torch_class_loss(rows["a"], o["a"][0], o["a"][1], st, "a", COEFS, dtype)
         + _torch_class_loss(rows["p"], o["p"][0], o["p"][1], st, "p", coefs_p, dtype)).backward()
        return grads()

    def ours(scale_a=1.0):
        o = outputs(torch.float32)
        o["a"][0].retain_grad()
        loss_a, loss_p, stats_a, stats_p = rollout.ppo_loss(be, o["a"][0], o["p"][0][:, 0], o["a"][1], o["p"][1][:, 0], st,
                                                            coeffs_p=COEFS_P, **COEFS)
        assert loss_a.dim() == 0 and loss_p.dim() == 0 and stats_a.shape == (8,) and not stats_a.requires_grad
        assert float(loss_a.detach()) == float(stats_a[0]) and float(loss_p.detach()) == float(stats_p[0])
        (scale_a * loss_a + loss_p).backward()
        return grads(), float(loss_a.detach()), float(loss_p.detach()), o["a"][0].grad.clone()

    want, t32 = torch_form(torch.float64), torch_form(torch.float32)
    got, loss_a, loss_p, at_logits = ours()
    for who in ("a", "p"):
        eo, et = np.abs(got[who] - want[who]).max(), np.abs(t32[who] - want[who]).max()
        print("%s: parameter gradients' max error %.3e, torch-float32's %.3e, ratio %.2f" % (who, eo, et, eo / et))
        assert eo <= 3.0 * et and np.abs(want[who]).max() > 0, who
    with pytest.raises(RuntimeError):  # no double backward through the stored gradients
        o = outputs(torch.float32)
        la_, _, _, _ = rollout.ppo_loss(be, o["a"][0], None, o["a"][1], None, st, **COEFS)
        (g_,) = torch.autograd.grad(la_, o["a"][0], create_graph=True)
        g_.sum().backward()
    doubled, _, _, doubled_at_logits = ours(2.0)
    assert torch.equal(doubled_at_logits, 2.0 * at_logits) and bool(at_logits.ne(0).any())  # (a power of two: exact)
    assert np.allclose(doubled["a"], 2.0 * got["a"], rtol=1e-5, atol=0) and np.allclose(doubled["p"], got["p"], rtol=1e-5, atol=0)
    # a class that is left out
    o = outputs(torch.float32)
    la, lp, sa, sp = rollout.ppo_loss(be, o["a"][0], None, o["a"][1], None, st, **COEFS)
    assert lp is None and sp is None and float(la.detach()) == loss_a


def test_trajectory_ppo_batch_first_loss_of_a_fragment():
    import torch

    from ai_economist_amd import rollout
    from ai_economist_amd.rollout import GraphedStep, MaskedMLPPolicy, Trajectory

    E, T = 6, 4
    env = make_env(dict(C2, episode_length=30, starting_agent_coin=12), n_envs=E, device=DEV)
    env.seed(5)
    env.reset()
    be = env.backend
    pol = MaskedMLPPolicy(be, seed=3, record_logp=True, value_head=True)
    traj = Trajectory(env, T)
    gs = GraphedStep(env, pol, auto_reset=True, warmup=3, trajectory=traj)
    traj.rewind()
    gs.replay(T)
    pol.logits(be.tensors)
    traj.finish(pol.value_a, pol.value_p)
    adv_a, adv_p, ret_a, ret_p = traj.advantages()
    batch = traj.ppo_batch(adv_a, adv_p, ret_a, ret_p)
    assert batch["masks_a"].shape[0] == T * E and batch["values_old_p"].shape == (T * E,)
    assert batch["masks_a"].data_ptr() == traj.masks_a.data_ptr() and batch["adv_a"].data_ptr() == adv_a.data_ptr()  # views
    # the logits of the stored observations by the same network, a step at a time: the rollout's own shapes
    la, lp, va, vp = [], [], [], []
    for t in range(T):
        a, p = pol.logits({k: v[t] for k, v in traj.obs.items()})
        la.append(a.view(E, be.n, -1).clone())
        lp.append(p.clone())
        va.append(pol.value_a.clone())
        vp.append(pol.value_p.clone())
    la, lp, va, vp = (torch.cat(x) for x in (la, lp, va, vp))
    assert torch.equal(va.view(T, E, be.n), traj.values_a[:T]) and torch.equal(vp.view(T, E), traj.values_p[:T])
    la.requires_grad_(True)
    loss_a, loss_p, stats_a, stats_p = rollout.ppo_loss(be, la, lp, va, vp, batch)
    torch.cuda.synchronize()
    for who, s in (("agents", stats_a.cpu().numpy()), ("planner", stats_p.cpu().numpy())):
        print(who, s)
        # (recomputed at the rollout's shapes the logits are bitwise the rollout's: the ratio is exactly 1)
        assert s[4] == 0 and s[5] == 0 and s[6] == 0 and s[7] == 0, (who, s)
        assert np.isfinite(s).all() and s[3] >= 0 and (who == "planner" or s[3] > 0)  # (a planner between tax periods: NO-OP only)
    loss_a.backward()
    assert la.grad.shape == la.shape and bool(la.grad.ne(0).any())
    # a minibatch of the fragment by index
    index = torch.tensor([5, 0, 23, 7, 7], dtype=torch.int32, device=DEV)
    sel = index.long()
    _, _, sa, sp = rollout.ppo_loss(be, la.detach()[sel], lp[sel], va[sel], vp[sel], batch, index=index)
    assert float(sa[4]) == 0 and float(sa[6]) == 0 and float(sp[7]) == 0


def test_one_call_in_a_graph_replays_to_the_same_bits():
    import torch

    _, be, rows, _, _ = _env("gtb_c2")
    ba, bp, _ = _batches("gtb_c2", 67, seed=9)
    st = _stored(ba, bp)
    la, lp, va, vp = _net(ba, "a", "logits"), _net(bp, "p", "logits"), _net(ba, "a", "values"), _net(bp, "p", "values")
    flat = lambda res: [t.clone() for cls in res for t in cls]  # noqa: E731
    eager = flat(be.ppo_loss(la, lp, va, vp, st, coeffs_p=COEFS_P, **COEFS))  # (also the warm-up: the workspace exists)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        be.ppo_loss(la, lp, va, vp, st, coeffs_p=COEFS_P, **COEFS)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = be.ppo_loss(la, lp, va, vp, st, coeffs_p=COEFS_P, **COEFS)
    for _ in range(2):
        for t in (t for cls in res for t in cls):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(flat(res), eager):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
