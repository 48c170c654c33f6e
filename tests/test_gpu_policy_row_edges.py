"""The policy-side kernels where a lane segment or a 64-entry chunk is exactly full, or one entry over: the sampler (the five
fast instances no other test launches, the generic kernel with a last chunk of one entry), aie_policy_evaluate forward and
backward, and aie_ppo_loss, on the configurations of tests/row_edges.py (tests/test_policy_row_edges_cpu.py holds the table
to the instance each case names).

  1. the sampler along the dynamics: every sub-action of every replica equals oracle/'s restatement over 24 steps across the
     tax days, `sample_t` and `error_flags` with it; the LOGP sampler on a twin environment picks the same and its logp is
     policy_eval_ref's, bit for bit (5 and 64 replicas);
  2. the sampler under planted masks and logits (the dynamics rarely open a row's last entry): only the last entry allowed,
     only entry 0, nothing, a dominant last logit, equal logits, NaN on the last entry, -1e30 everywhere, the last entry the
     only finite one -- against the oracle on every row and against the Python transcription on some; the census (the last
     entry picked, entry 0 picked, a fully masked row gave 0) is asserted per class;
  3. the evaluator forward and backward at B = 1, 5, 67 under the caller's masks, stored actions at len - 1, len, SEG - 1,
     SEG, -1 and on a masked entry, rows with nothing allowed: bit for bit, every gradient entry written (NaN-filled buffers);
  4. the PPO loss with ppo_ref's planted edges at B = 1, 5, 67: gradients bit for bit, statistics within ppo_ref's bound;
  5. independently of the transcriptions: evaluator and PPO loss against float64 torch, at most 3 x torch-float32's own
     maximum error on the same rows, per quantity (the CPU tests' rule); the measured ratios are printed.
"""
import math

import numpy as np
import pytest

import policy_eval_ref as ref
import ppo_ref
import row_edges
from helpers import counter_rng, make_env, sampler_entry_rng, sampler_pick_row
from test_gpu_policy_evaluate import _check_evaluate, _rows, _same, _want_backward, _want_forward
from test_gpu_ppo_loss import COEFS, COEFS_P, _hold, _run, _want

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
FACTOR = 3.0  # the project's yardstick (tests/test_policy_evaluate_cpu.py): <= 3 x torch-float32's own max error
_ENVS = {}


def _env(name):
    """One small environment per case for the calls that take their own masks: (backend, rows, WA, MP)."""
    if name not in _ENVS:
        case = row_edges.case(name)
        env = make_env(case.cfg, n_envs=5, device=DEV)
        env.seed(3)
        env.reset()
        be = env.backend
        WA, MP = int(be.tensors["obs_a_action_mask"].shape[-1]), int(be.tensors["obs_p_action_mask"].shape[-1])
        assert (be.n, WA, MP) == (case.n, case.len_a, case.rows_p * case.len_p)
        assert _rows(env, name, be) == case.rows()  # (the table's rows are the evaluator tests' own reading of the masks)
        _ENVS[name] = (env, be, case.rows(), WA, MP)
    return _ENVS[name][1:]


def _start(case, E, offset, seed=3):
    env = make_env(case.cfg, n_envs=E, device=DEV, env_offset=offset)
    env.seed(seed)
    env.reset()
    return env


def _logp_of(rows, la, lp, ma, mp, a, p):
    wla, _ = _want_forward(rows["a"], la, ma, a)
    wlp, _ = _want_forward(rows["p"], lp[:, None, :], mp[:, None, :], p[:, None, :])
    return wla, wlp[:, 0]


# ---- 1. the sampler along the dynamics ----
@pytest.mark.parametrize("E", [5, 64])
@pytest.mark.parametrize("name", row_edges.CASES)
def test_sampler_along_the_dynamics(name, E):
    import torch
    from oracle_lib import OracleEnv

    case = row_edges.case(name)
    OFF, SEED = 1000, 77
    env, twin = _start(case, E, OFF), _start(case, E, OFF)
    be, bt = env.backend, twin.backend
    oracle = OracleEnv(env.build_config(), env.layout_planes())
    oracle.seed(3 + OFF)
    oracle.reset()
    rows = case.rows()
    n, MA, MP = be.n, case.len_a, case.rows_p * case.len_p
    assert tuple(be.tensors["obs_a_action_mask"].shape) == (E, n, MA) and tuple(be.tensors["obs_p_action_mask"].shape) == (E, MP)
    g = torch.Generator(device="cpu").manual_seed(11)
    seen_a, seen_p, masks_seen = set(), set(), set()
    for t in range(24):  # tax days at steps 0, 10 and 20 (period 10)
        la = (torch.randn(E, n, MA, generator=g) * 3).float()
        lp = (torch.randn(E, MP, generator=g) * 3).float()
        la[t % E, 0, 1:4] = float("nan")           # NaN logits are masked entries
        la[(t + 1) % E, 1, :] = 0.25                # all-equal logits
        lp[(t + 2) % E, :] = -1e30                  # hopeless logits still yield an allowed entry
        la[(t + 3) % E, 2, :] = float("nan")        # a fully NaN row: NO-OP
        dla, dlp = la.to(DEV), lp.to(DEV)
        a, p = be.sample_policy_actions(dla, dlp, seed=SEED, env_offset=OFF)
        ta, tp, ga, gp = bt.sample_policy_actions(dla, dlp, seed=SEED, env_offset=OFF, logp=True)
        torch.cuda.synchronize()
        ma, mp = be.tensors["obs_a_action_mask"].cpu().numpy(), be.tensors["obs_p_action_mask"].cpu().numpy()
        assert np.array_equal(ma, oracle.t["obs_a_action_mask"]) and np.array_equal(mp, oracle.t["obs_p_action_mask"])
        wa, wp = oracle.sample_policy_actions(la.numpy(), lp.numpy(), SEED, OFF, width_a=a.shape[-1], width_p=p.shape[-1])
        ah, ph = a.cpu().numpy(), p.cpu().numpy()
        assert np.array_equal(ah, wa), "step %d: agents' sub-actions differ at %s" % (t, np.argwhere(ah != wa)[:4].tolist())
        assert np.array_equal(ph, wp), "step %d: planner's sub-actions differ at %s" % (t, np.argwhere(ph != wp)[:4].tolist())
        assert torch.equal(ta, a) and torch.equal(tp, p), "step %d: the LOGP sampler picks differently" % t
        assert np.array_equal(be.tensors["sample_t"].cpu().numpy(), oracle.t["sample_t"]) and int(oracle.t["sample_t"][0]) == t + 1
        assert torch.equal(bt.tensors["sample_t"], be.tensors["sample_t"])
        wla, wlp = _logp_of(rows, la.numpy(), lp.numpy(), ma, mp, ah, ph)
        _same(ga, wla, "step %d: agents' logp of the picks" % t)
        _same(gp, wlp, "step %d: planner's logp of the picks" % t)
        assert (wa[(t + 3) % E, 2] == 0).all() and not ga.cpu().numpy()[(t + 3) % E, 2].any()
        seen_a.update(np.unique(wa).tolist())
        seen_p.update(np.unique(wp).tolist())
        masks_seen.add(ma.tobytes() + mp.tobytes())
        env.step({"a": a, "p": p})
        twin.step({"a": ta, "p": tp})
        oracle.step(wa.reshape(E, -1), wp, nthreads=4)
    assert int(be.tensors["error_flags"].abs().sum()) == 0 and int(bt.tensors["error_flags"].abs().sum()) == 0
    assert torch.equal(be.arena, bt.arena)
    assert len(masks_seen) > 1 and len(seen_a) > 2 and len(seen_p) > 1
    print("%s E=%d: agents picked %d of %d entries (largest %d), the planner %d of %d (largest %d)" % (
        name, E, len(seen_a), case.len_a, max(seen_a), len(seen_p), case.len_p, max(seen_p)))


# ---- 2. the sampler under planted masks and logits ----
PLANTS = ("last_only", "first_only", "nothing", "last_dominant", "all_equal", "nan_on_last", "hopeless", "last_only_finite", "random")


def _plant(kind, lg, mk, rng):
    """One row's logits and mask, in place."""
    n = len(lg)
    lg[:] = (rng.randn(n) * 3).astype(f32)
    mk[:] = 1.0
    if kind == "last_only":
        mk[:] = 0.0
        mk[n - 1] = 1.0
    elif kind == "first_only":
        mk[:] = 0.0
        mk[0] = 1.0
    elif kind == "nothing":
        mk[:] = 0.0
    elif kind == "last_dominant":
        lg[n - 1] = lg.max() + f32(30.0)
    elif kind == "all_equal":
        lg[:] = 0.25
    elif kind == "nan_on_last":
        lg[n - 1] = np.nan
    elif kind == "hopeless":
        lg[:] = -1e30
    elif kind == "last_only_finite":
        lg[: n - 1] = np.nan
    else:
        mk[:] = (rng.rand(n) < 0.6).astype(f32)


@pytest.mark.parametrize("name", row_edges.CASES)
def test_sampler_under_planted_masks_and_logits(name):
    import torch
    from oracle_lib import OracleEnv

    case = row_edges.case(name)
    E, OFF, SEED, CALLS = 64, 300, 5, 4
    env = _start(case, E, OFF)
    be = env.backend
    oracle = OracleEnv(env.build_config(), env.layout_planes())
    oracle.seed(3 + OFF)
    oracle.reset()
    rows = case.rows()
    n, MA, MP = be.n, case.len_a, case.rows_p * case.len_p
    per_env = n + case.rows_p
    rng = np.random.RandomState(len(name) + 17)
    census = {who: dict(last=0, first=0, nothing=0) for who in "ap"}
    for call in range(CALLS):
        la, ma = np.zeros((E, n, MA), f32), np.zeros((E, n, MA), f32)
        lp, mp = np.zeros((E, MP), f32), np.zeros((E, MP), f32)
        kinds = {}
        for e in range(E):
            for i in range(n):
                kinds["a", e, i] = PLANTS[(e + 2 * i + 3 * call) % len(PLANTS)]
                _plant(kinds["a", e, i], la[e, i], ma[e, i], rng)
            for s, (lo, ln) in enumerate(rows["p"]):
                kinds["p", e, s] = PLANTS[(e + 4 * s + 5 * call + 1) % len(PLANTS)]
                _plant(kinds["p", e, s], lp[e, lo:lo + ln], mp[e, lo:lo + ln], rng)
        # the same arrays on either side: the arena's masks and the oracle's
        be.tensors["obs_a_action_mask"].copy_(torch.as_tensor(ma))
        be.tensors["obs_p_action_mask"].copy_(torch.as_tensor(mp))
        oracle.t["obs_a_action_mask"][...] = ma
        oracle.t["obs_p_action_mask"][...] = mp
        dla, dlp = torch.as_tensor(la).to(DEV), torch.as_tensor(lp).to(DEV)
        kept_t = be.tensors["sample_t"].clone()
        a, p = be.sample_policy_actions(dla, dlp, seed=SEED, env_offset=OFF)
        torch.cuda.synchronize()
        ah, ph = a.cpu().numpy().copy(), p.cpu().numpy().copy()
        assert int(be.tensors["sample_t"][0]) == call + 1
        wa, wp = oracle.sample_policy_actions(la, lp, SEED, OFF, width_a=1, width_p=case.rows_p)
        assert np.array_equal(ah, wa), "call %d: agents differ at %s" % (call, [(tuple(q), kinds["a", q[0], q[1]]) for q in np.argwhere(ah != wa)[:4]])
        assert np.array_equal(ph, wp), "call %d: planner differs at %s" % (call, [(tuple(q), kinds["p", q[0], q[1]]) for q in np.argwhere(ph != wp)[:4]])
        # the LOGP instance from the same draw index: the same picks, the transcription's logp
        be.tensors["sample_t"].copy_(kept_t)
        a2, p2, ga, gp = be.sample_policy_actions(dla, dlp, seed=SEED, env_offset=OFF, logp=True)
        torch.cuda.synchronize()
        assert np.array_equal(a2.cpu().numpy(), ah) and np.array_equal(p2.cpu().numpy(), ph), "call %d: the LOGP sampler picks differently" % call
        assert int(be.tensors["sample_t"][0]) == call + 1
        wla, wlp = _logp_of(rows, la, lp, ma, mp, ah, ph)
        _same(ga, wla, "call %d: agents' logp of the picks" % call)
        _same(gp, wlp, "call %d: planner's logp of the picks" % call)
        # the Python transcription on the first replicas (exact rational fused multiply-adds: slow)
        for e in range(3 if call < 2 else 0):
            base = counter_rng(SEED, OFF + e, call, per_env)
            for i in range(n):
                assert ah[e, i, 0] == sampler_pick_row(la[e, i], ma[e, i], sampler_entry_rng(base, i)), (call, e, i, kinds["a", e, i])
            for s, (lo, ln) in enumerate(rows["p"]):
                assert ph[e, s] == sampler_pick_row(lp[e, lo:lo + ln], mp[e, lo:lo + ln], sampler_entry_rng(base, n + s)), (call, e, s)
        # what each plant must give, whatever the references say; the census
        for (who, e, r), kind in kinds.items():
            pick, ln = (int(ah[e, r, 0]), MA) if who == "a" else (int(ph[e, r]), case.len_p)
            lg_row, mk_row = (la[e, r], ma[e, r]) if who == "a" else (lp[e, rows["p"][r][0]:][:ln], mp[e, rows["p"][r][0]:][:ln])
            c = census[who]
            if kind in ("last_only", "last_only_finite"):
                assert pick == ln - 1, (who, e, r, kind, pick)
            elif kind in ("first_only", "nothing"):
                assert pick == 0, (who, e, r, kind, pick)
                c["nothing"] += kind == "nothing"
            elif kind == "nan_on_last":
                assert pick < ln - 1 or ln == 1, (who, e, r, kind, pick)
            assert pick == 0 or (mk_row[pick] > 0.5 and lg_row[pick] == lg_row[pick]), (who, e, r, kind, pick)
            c["last"] += pick == ln - 1
            c["first"] += pick == 0 and kind != "nothing"
    for who in "ap":
        c = census[who]
        print("%s class %s: last entry picked %d times, entry 0 %d times, fully masked rows %d" % (name, who, c["last"], c["first"], c["nothing"]))
        assert c["last"] > 0, "%s class %s: no row's last entry was ever picked" % (name, who)
        assert c["first"] > 0, "%s class %s: entry 0 was never picked" % (name, who)
        assert c["nothing"] > 0, "%s class %s: no fully masked row" % (name, who)
    assert int(be.tensors["error_flags"].abs().sum()) == 0


# ---- 3. the evaluator ----
ACTION_PLANTS = ("none", "last", "len", "seg_minus_1", "seg", "minus_1", "masked", "row_masked")


def _eval_batch(case, rows, B, n, WA, MP, seed):
    """Operands [B, ...] under the caller's own random masks, with the stored actions planted row after row.
    -> (la, lp, ma, mp, aa, ap, {class: set of plants})."""
    rng = np.random.RandomState(seed)
    la, lp = (rng.randn(B, n, WA) * 3).astype(f32), (rng.randn(B, MP) * 3).astype(f32)
    ma, mp = (rng.rand(B, n, WA) < 0.7).astype(f32), (rng.rand(B, MP) < 0.7).astype(f32)
    aa, ap = np.zeros((B, n, 1), np.int32), np.zeros((B, case.rows_p), np.int32)
    planted = {"a": set(), "p": set()}
    flat = [("a", b, i, 0, WA) for b in range(B) for i in range(n)] + \
           [("p", b, s, lo, ln) for b in range(B) for s, (lo, ln) in enumerate(rows["p"])]
    for j, (who, b, r, lo, ln) in enumerate(flat):
        mk = ma[b, r] if who == "a" else mp[b, lo:lo + ln]
        mk[rng.randint(ln)] = 1.0
        seg = ref.segment(ln)
        kind = ACTION_PLANTS[(j + B) % len(ACTION_PLANTS)]
        act = int(rng.choice(np.flatnonzero(mk > 0.5)))
        if kind == "last":
            mk[ln - 1] = 1.0
            act = ln - 1
        elif kind == "len":          # (a lane that exists but holds no entry wherever len < SEG)
            act = ln
        elif kind == "seg_minus_1":  # (the row's last entry where the segment is full, else past the row)
            act = seg - 1
        elif kind == "seg":
            act = seg
        elif kind == "minus_1":
            act = -1
        elif kind == "masked":       # (the entry behind an allowed one, which stays allowed)
            act = (act + 1) % ln
            mk[act] = 0.0
        elif kind == "row_masked":
            mk[:] = 0.0
        planted[who].add(kind)
        if who == "a":
            aa[b, r, 0] = act
        else:
            ap[b, r] = act
    return la, lp, ma, mp, aa, ap, planted


@pytest.mark.parametrize("name", row_edges.CASES)
def test_evaluator_forward_and_backward(name):
    import torch

    case = row_edges.case(name)
    be, rows, WA, MP = _env(name)
    n = be.n
    rng = np.random.RandomState(7)
    SENT = 64
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    t = lambda x: torch.as_tensor(x).to(DEV)  # noqa: E731
    for B in (1, 5, 67):
        la, lp, ma, mp, aa, ap, planted = _eval_batch(case, rows, B, n, WA, MP, seed=100 * B + len(name))
        if B == 67:
            assert planted["a"] == set(ACTION_PLANTS) == planted["p"]
        _check_evaluate(be, rows, la, lp, ma, mp, aa, ap, rng, "%s, caller masks, B = %d" % (name, B))
        # the planted rows do what they are planted for
        wla, _ = _want_forward(rows["a"], la, ma, aa)
        inr = (aa[..., 0] >= 0) & (aa[..., 0] < WA)
        assert np.isneginf(wla[..., 0][~inr & (ma.sum(-1) > 0)]).all() and (wla[..., 0][ma.sum(-1) == 0] == 0).all()
        # every entry is written: NaN-filled outputs with sentinels behind them, through the C call
        gla, gha = rng.randn(*aa.shape).astype(f32), rng.randn(*aa.shape).astype(f32)
        glp, ghp = rng.randn(*ap.shape).astype(f32), rng.randn(*ap.shape).astype(f32)
        d = [t(x) for x in (la, lp, ma, mp, aa, ap, gla, glp, gha, ghp)]
        nan = lambda k: torch.full((k + SENT,), float("nan"), device=DEV)  # noqa: E731
        out = [nan(aa.size), nan(ap.size), nan(aa.size), nan(ap.size)]
        be._check(be.lib.aie_policy_evaluate(be.handle, B, *[P(x) for x in d[:6]], *[P(o) for o in out], None))
        grads = [nan(la.size), nan(lp.size)]
        be._check(be.lib.aie_policy_evaluate_backward(be.handle, B, *[P(x) for x in d], P(grads[0]), P(grads[1]), None))
        torch.cuda.synchronize()
        wla, wHa = _want_forward(rows["a"], la, ma, aa)
        wlp, wHp = _want_forward(rows["p"], lp[:, None, :], mp[:, None, :], ap[:, None, :])
        wga = _want_backward(rows["a"], la, ma, aa, gla, gha)
        wgp = _want_backward(rows["p"], lp[:, None, :], mp[:, None, :], ap[:, None, :], glp[:, None, :], ghp[:, None, :])
        for got, want, what in ((out[0], wla, "agents' logp"), (out[1], wlp[:, 0], "planner's logp"), (out[2], wHa, "agents' entropy"),
                                (out[3], wHp[:, 0], "planner's entropy"), (grads[0], wga, "agents' gradient"),
                                (grads[1], wgp[:, 0], "planner's gradient")):
            k = want.size
            assert not bool(torch.isnan(got[:k]).any()), "%s B = %d: %s has entries that were not written" % (name, B, what)
            _same(got[:k], want, "%s B = %d, NaN-filled buffers: %s" % (name, B, what))
            assert bool(torch.isnan(got[k:]).all()), "%s B = %d: wrote behind %s" % (name, B, what)
        assert not grads[0][: la.size].cpu().numpy().reshape(ma.shape)[ma < 0.5].any()
        assert not grads[1][: lp.size].cpu().numpy().reshape(mp.shape)[mp < 0.5].any()


# ---- 4. the PPO loss ----
def _ppo_batches(case, rows, B, n, WA, MP, seed, edges=True):
    out, where = [], []
    for who, W, actors, s in (("a", WA, n, seed), ("p", MP, 1, seed + 1)):
        b = ppo_ref.random_batch(rows[who], W, B, actors, s)
        if edges:
            # some stored actions on their row's LAST entry (allowed), with an old logp to match
            N, w = B * actors, len(rows[who])
            x, m, act = b["logits"].reshape(N, W), b["masks"].reshape(N, W), b["actions"].reshape(N, w)
            sel = np.arange(N)[::3]
            for k, (lo, ln) in enumerate(rows[who]):
                m[sel, lo + ln - 1] = 1.0
                act[sel, k] = ln - 1
            r = np.random.RandomState(s + 50)
            lp_old, _ = ppo_ref.slot_terms(rows[who], (x + 0.1 * r.randn(N, W)).astype(f32), m, act)
            b["logp_old"].reshape(N, w)[...] = lp_old
            where.append(ppo_ref.plant_edges(rows[who], b, s + 2, COEFS["vf_clip"]))
        out.append(b)
    return out[0], out[1], where


@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("name", row_edges.CASES)
def test_ppo_loss_equals_the_transcription(name, B):
    case = row_edges.case(name)
    be, rows, WA, MP = _env(name)
    coefs_p = dict(COEFS, **COEFS_P)
    ba, bp, where = _ppo_batches(case, rows, B, be.n, WA, MP, seed=10 * B + len(name))
    if B == 67:
        assert set(where[0]) == set(ppo_ref.EDGES) == set(where[1])
    got = _run(be, ba, bp, coeffs_p=COEFS_P)
    want_a, want_p = _want(rows["a"], ba), _want(rows["p"], bp, coefs=coefs_p)
    _hold(got[0], want_a, "%s B=%d agents" % (name, B))
    _hold(got[1], want_p, "%s B=%d planner" % (name, B))
    if B == 67:
        assert want_a["stats"][6] == 6 and want_p["stats"][6] == 6 and want_a["stats"][5] > 0
        last = ba["actions"][..., 0] == case.len_a - 1
        assert last.sum() >= 67 and np.isfinite(want_a["logp"][last.reshape(-1), 0]).sum() >= 60
    # each class alone, and without values
    only_a, only_p = _run(be, ba, None), _run(be, None, bp, coeffs_p=COEFS_P)
    _hold(only_a[0], want_a, "%s B=%d agents alone" % (name, B))
    _hold(only_p[1], want_p, "%s B=%d planner alone" % (name, B))
    nv = _run(be, ba, bp, values=False, coeffs_p=COEFS_P)
    _hold(nv[0], _want(rows["a"], ba, values=False), "%s B=%d agents, no values" % (name, B))
    _hold(nv[1], _want(rows["p"], bp, values=False, coefs=coefs_p), "%s B=%d planner, no values" % (name, B))


# ---- 5. against float64 torch ----
BATCHES, B64 = 12, 67  # a maximum error wants more than one batch of rows: 12 calls of B = 67


def _torch_eval(rows, x, m, act, gl, gh, dtype):
    """x / m [N, W], act / gl / gh [N, w] -> (logp [N, w], entropy [N, w], d(sum gl logp + gh H) / dx) as float64 numpy."""
    import torch

    x = torch.tensor(x, dtype=dtype, requires_grad=True)
    allowed = torch.tensor(m > 0.5)
    lps, Hs = [], []
    for s, (lo, ln) in enumerate(rows):
        ok = allowed[:, lo:lo + ln]
        lsm = torch.log_softmax(x[:, lo:lo + ln].masked_fill(~ok, -math.inf), -1)
        lps.append(lsm.gather(-1, torch.tensor(act[:, s:s + 1], dtype=torch.int64))[:, 0])
        Hs.append(-(lsm.exp() * lsm.masked_fill(~ok, 0.0)).sum(-1))
    lp, H = torch.stack(lps, 1), torch.stack(Hs, 1)
    ((lp * torch.tensor(gl, dtype=dtype)).sum() + (H * torch.tensor(gh, dtype=dtype)).sum()).backward()
    return lp.detach().double().numpy(), H.detach().double().numpy(), x.grad.double().numpy()


@pytest.mark.parametrize("name", row_edges.CASES)
def test_evaluator_against_float64(name):
    import torch

    case = row_edges.case(name)
    be, rows, WA, MP = _env(name)
    n, B = be.n, B64
    names = ("logp", "entropy", "gradient")
    eo, et = {"a": np.zeros(3), "p": np.zeros(3)}, {"a": np.zeros(3), "p": np.zeros(3)}
    t = lambda x: torch.as_tensor(x).to(DEV)  # noqa: E731
    for k in range(BATCHES):
        rng = np.random.RandomState(1000 * k + len(name))
        ops = {}
        for who, actors, W in (("a", n, WA), ("p", 1, MP)):
            N, w = B * actors, len(rows[who])
            x, m = (rng.randn(N, W) * 3).astype(f32), (rng.rand(N, W) < 0.7).astype(f32)
            act = np.zeros((N, w), np.int32)
            for s, (lo, ln) in enumerate(rows[who]):
                m[np.arange(N), lo + rng.randint(0, ln, N)] = 1.0
                act[:, s] = (rng.rand(N, ln) * m[:, lo:lo + ln]).argmax(1)  # an allowed entry
            ops[who] = (x, m, act, rng.randn(N, w).astype(f32), rng.randn(N, w).astype(f32))
        (xa, ma, aa, gla, gha), (xp, mp, ap, glp, ghp) = ops["a"], ops["p"]
        sa, sp = (B, n, 1), (B, case.rows_p)
        fw = be.policy_evaluate(t(xa.reshape(B, n, WA)), t(xp), t(ma.reshape(B, n, WA)), t(mp), t(aa.reshape(sa)), t(ap.reshape(sp)))
        bw = be.policy_evaluate_backward(t(xa.reshape(B, n, WA)), t(xp), t(ma.reshape(B, n, WA)), t(mp), t(aa.reshape(sa)), t(ap.reshape(sp)),
                                         t(gla.reshape(sa)), t(glp.reshape(sp)), t(gha.reshape(sa)), t(ghp.reshape(sp)))
        torch.cuda.synchronize()
        for who, c, (x, m, act, gl, gh) in (("a", 0, ops["a"]), ("p", 1, ops["p"])):
            ours = (fw[c].double().cpu().numpy().reshape(act.shape), fw[2 + c].double().cpu().numpy().reshape(act.shape),
                    bw[c].double().cpu().numpy().reshape(x.shape))
            want, t32 = _torch_eval(rows[who], x, m, act, gl, gh, torch.float64), _torch_eval(rows[who], x, m, act, gl, gh, torch.float32)
            assert not ours[2][m < 0.5].any()
            for j in range(3):
                eo[who][j] = max(eo[who][j], np.abs(ours[j] - want[j]).max())
                et[who][j] = max(et[who][j], np.abs(t32[j] - want[j]).max())
    for who in "ap":
        for j, q in enumerate(names):
            print("%s class %s %-9s device %.3e  torch-float32 %.3e  ratio %.2f" % (name, who, q, eo[who][j], et[who][j], eo[who][j] / et[who][j]))
    for who in "ap":
        for j, q in enumerate(names):
            assert eo[who][j] <= FACTOR * et[who][j], "%s class %s %s: %.2f x torch-float32's max error" % (name, who, q, eo[who][j] / et[who][j])


@pytest.mark.parametrize("name", row_edges.CASES)
def test_ppo_loss_against_float64(name):
    import torch
    from test_ppo_loss_cpu import _torch_loss

    case = row_edges.case(name)
    be, rows, WA, MP = _env(name)
    names = ("loss", "logits' gradient", "values' gradient")
    eo, et = {"a": np.zeros(3), "p": np.zeros(3)}, {"a": np.zeros(3), "p": np.zeros(3)}
    for k in range(BATCHES):
        ba, bp, _ = _ppo_batches(case, rows, B64, be.n, WA, MP, seed=100 * k + len(name), edges=False)  # nothing invalid, no ties
        got = _run(be, ba, bp)
        for who, c, b in (("a", 0, ba), ("p", 1, bp)):
            stats, grad, grad_v = got[c]
            assert stats[6] == 0 and not grad.reshape(b["masks"].shape)[b["masks"] < 0.5].any()
            ours = (float(stats[0]), grad.astype(np.float64).reshape(b["logits"].shape), grad_v.astype(np.float64).reshape(b["values"].shape))
            want = _torch_loss(rows[who], b, dtype=torch.float64, **COEFS)
            t32 = _torch_loss(rows[who], b, dtype=torch.float32, **COEFS)
            for j in range(3):
                eo[who][j] = max(eo[who][j], np.abs(np.asarray(ours[j]) - want[j]).max())
                et[who][j] = max(et[who][j], np.abs(np.asarray(t32[j]) - want[j]).max())
    for who in "ap":
        for j, q in enumerate(names):
            print("%s class %s %-17s device %.3e  torch-float32 %.3e  ratio %.2f" % (name, who, q, eo[who][j], et[who][j], eo[who][j] / et[who][j]))
    for who in "ap":
        for j, q in enumerate(names):
            assert eo[who][j] <= FACTOR * et[who][j], "%s class %s %s: %.2f x torch-float32's max error" % (name, who, q, eo[who][j] / et[who][j])
