"""Python transcription of the PPO loss (csrc/aie_trainer_math.h: the comment above aie_ppo_actor_terms), written from that
comment: float32 operation for operation, vectorised over actors (numpy rounds every float32 operation on its own).

  * slot terms (logp_s, H_s, the slots' gradient rows) come from policy_eval_ref.rows_forward / rows_backward, which
    tests/test_policy_evaluate_cpu.py holds to the header bit for bit;
  * per-actor terms, slot gradients' two incoming scalars and the value terms are numpy float32;
  * the statistics are the float64 `math.fsum` of the float32 terms (the exact sum, rounded once), with the bound the
    device's own order of summation has to hold against it.

An actor class is described by `rows`: [(offset, length)] of its action slots inside one actor's logits.
"""
import math

import numpy as np

import policy_eval_ref as ref

f32 = np.float32
N_STATS = 8


def joint(x):
    """x [N, w] -> x[:, 0] + x[:, 1] + ... added in slot order, each sum rounded."""
    x = np.asarray(x, f32)
    s = x[:, 0].copy()
    with np.errstate(all="ignore"):
        for k in range(1, x.shape[1]):
            s = (s + x[:, k]).astype(f32)
    return s


def slot_terms(rows, logits, masks, actions):
    """logits / masks [N, W], actions [N, w] -> (logp [N, w], H [N, w])."""
    N = logits.shape[0]
    lp, H = np.zeros((N, len(rows)), f32), np.zeros((N, len(rows)), f32)
    for s, (lo, ln) in enumerate(rows):
        lp[:, s], H[:, s] = ref.rows_forward(logits[:, lo:lo + ln], masks[:, lo:lo + ln], actions[:, s])
    return lp, H


def advantage(adv, moments):
    adv = np.asarray(adv, f32)
    if moments is None:
        return adv
    with np.errstate(all="ignore"):
        c = (adv - f32(moments[0])).astype(f32)
        return (c * f32(moments[1])).astype(f32)


def actor_terms(logp, logp_old, adv, clip, scale, moments=None):
    """logp / logp_old [N, w], adv [N] -> dict of [N] arrays: ln, lo, d, valid, r, unclipped, pol, kl, clipf, absd, g_logp."""
    logp, logp_old = np.asarray(logp, f32), np.asarray(logp_old, f32)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        ln, lo = joint(logp), joint(logp_old)
        d = (ln - lo).astype(f32)
        finite = np.isfinite(logp).all(1) & np.isfinite(logp_old).all(1)
        valid = finite & (np.abs(d) <= f32(80.0))
        Ap = advantage(adv, moments)
        r = ref.expf_v(np.where(valid, d, f32(0.0)).astype(f32))
        lo_c, hi_c = f32(one - f32(clip)), f32(one + f32(clip))
        rc = np.where(r < lo_c, lo_c, r).astype(f32)
        rc = np.where(rc > hi_c, hi_c, rc).astype(f32)
        u = (r * Ap).astype(f32)
        c = (rc * Ap).astype(f32)
        unclipped = u <= c
        surr = np.where(unclipped, u, c).astype(f32)
        su = (f32(scale) * u).astype(f32)
        zero = f32(0.0)
        return dict(ln=ln, lo=lo, d=d, valid=valid, r=r, Ap=Ap, unclipped=unclipped,
                    pol=np.where(valid, -surr, zero).astype(f32), kl=np.where(valid, -d, zero).astype(f32),
                    clipf=(valid & ((r < lo_c) | (r > hi_c))).astype(f32), absd=np.where(valid, np.abs(d), zero).astype(f32),
                    g_logp=np.where(valid & unclipped, -su, zero).astype(f32), lo_c=lo_c, hi_c=hi_c)


def value_terms(v, v_old, ret, vf_clip, kv):
    """[N] arrays -> (vf [N], grad_v [N])."""
    v, v_old, ret = (np.asarray(t, f32) for t in (v, v_old, ret))
    with np.errstate(all="ignore"):
        e1 = (v - ret).astype(f32)
        q1 = (e1 * e1).astype(f32)
        vf, dq = q1, e1
        if f32(vf_clip) > 0:
            cl = f32(vf_clip)
            dv = (v - v_old).astype(f32)
            dc = np.where(dv < -cl, -cl, dv).astype(f32)
            dc = np.where(dc > cl, cl, dc).astype(f32)
            vc = (v_old + dc).astype(f32)
            e2 = (vc - ret).astype(f32)
            q2 = (e2 * e2).astype(f32)
            first = q1 >= q2
            vf = np.where(first, q1, q2).astype(f32)
            dq = np.where(first, e1, np.where(dc == dv, e2, f32(0.0))).astype(f32)
        dq2 = (dq + dq).astype(f32)
        return vf, (f32(kv) * dq2).astype(f32)


def ulp32(x):
    return float(np.spacing(np.abs(f32(x)))) if np.isfinite(x) else 0.0


def statistics(pol, vf, He, kl, clipf, valid, absd, vf_coef, ent_coef):
    """The eight statistics from the exact (`fsum`) float64 sums, and `tol`: what another order of float64 summation may
    differ by -- per mean (N - 1) 2^-53 sum|term| / N, plus one float32 ulp for the final rounding; for the loss the three
    means' bounds weighted by the coefficients, plus one ulp."""
    N = len(pol)
    terms = [None, pol, vf, He, kl, clipf]
    mean, bound = [0.0] * 6, [0.0] * 6
    for k in range(1, 6):
        t = np.asarray(terms[k], f32).astype(np.float64)
        mean[k] = math.fsum(t) / N
        bound[k] = (N - 1) * 2.0 ** -53 * math.fsum(np.abs(t)) / N
    cv, ce = float(f32(vf_coef)), float(f32(ent_coef))
    loss = mean[1] + cv * mean[2] - ce * mean[3]
    stats = np.array([loss] + mean[1:] + [float((~np.asarray(valid)).sum()), float(np.max(absd, initial=0.0))]).astype(f32)
    tol = np.zeros(N_STATS)
    tol[0] = bound[1] + abs(cv) * bound[2] + abs(ce) * bound[3] + ulp32(stats[0])
    for k in range(1, 6):
        tol[k] = bound[k] + ulp32(stats[k])
    return stats, tol


def ppo_class(rows, logits, masks, actions, logp_old, adv, values, values_old, returns, clip, vf_clip, vf_coef, ent_coef,
              moments=None):
    """One actor class.  logits / masks [B, actors, W] (logits at batch element b, everything else already gathered to
    b), actions / logp_old [B, actors, w], adv / values / values_old / returns [B, actors] (values None: no value term).
    -> dict(grad [B, actors, W], grad_v [B, actors] or None, stats [8], tol [8], and the per-actor terms)."""
    B, A, W = logits.shape
    N = B * A
    x, m = np.asarray(logits, f32).reshape(N, W), np.asarray(masks, f32).reshape(N, W)
    act = np.asarray(actions).reshape(N, len(rows))
    lp, H = slot_terms(rows, x, m, act)
    with np.errstate(all="ignore"):
        scale = f32(f32(1.0) / f32(N))
        g_H = f32(-f32(scale * f32(ent_coef)))
        kv = f32(scale * f32(vf_coef))
    t = actor_terms(lp, np.asarray(logp_old, f32).reshape(N, len(rows)), np.asarray(adv, f32).reshape(N), clip, scale, moments)
    He = joint(H)
    grad = np.zeros((N, W), f32)
    for s, (lo, ln) in enumerate(rows):
        grad[:, lo:lo + ln] = ref.rows_backward(x[:, lo:lo + ln], m[:, lo:lo + ln], act[:, s], t["g_logp"], np.full(N, g_H, f32))
    vf, grad_v = np.zeros(N, f32), None
    if values is not None:
        vf, grad_v = value_terms(np.asarray(values, f32).reshape(N), np.asarray(values_old, f32).reshape(N),
                                 np.asarray(returns, f32).reshape(N), vf_clip, kv)
        grad_v = grad_v.reshape(B, A)
    stats, tol = statistics(t["pol"], vf, He, t["kl"], t["clipf"], t["valid"], t["absd"], vf_coef, ent_coef)
    return dict(t, grad=grad.reshape(B, A, W), grad_v=grad_v, stats=stats, tol=tol, logp=lp, H=H, He=He, vf=vf, scale=scale, g_H=g_H,
                kv=kv)


# ---- inputs: a random batch and the edge cases planted at known actors (shared by the CPU and the GPU tests) -----------
def random_batch(rows, W, B, A, seed, sigma=2.0, drift=0.1):
    """dict of numpy operands [B, A, ...] of one actor class: every slot has an allowed entry, stored actions are allowed,
    logp_old is the evaluation of slightly different logits (small log-ratios), nothing invalid, no ties planted."""
    rng = np.random.RandomState(seed)
    N, w = B * A, len(rows)
    x = (rng.randn(N, W) * sigma).astype(f32)
    m = (rng.rand(N, W) < 0.7).astype(f32)
    act = np.zeros((N, w), np.int32)
    for s, (lo, ln) in enumerate(rows):
        m[np.arange(N), lo + rng.randint(0, ln, N)] = 1.0
        act[:, s] = (rng.rand(N, ln) * m[:, lo:lo + ln]).argmax(1)
    lp_old, _ = slot_terms(rows, (x + drift * rng.randn(N, W)).astype(f32), m, act)
    v = (rng.randn(N) * 3).astype(f32)
    return dict(logits=x.reshape(B, A, W), masks=m.reshape(B, A, W), actions=act.reshape(B, A, w), logp_old=lp_old.reshape(B, A, w),
                adv=rng.randn(B, A).astype(f32), values=v.reshape(B, A),
                values_old=(v + rng.randn(N).astype(f32) * f32(2.0)).astype(f32).reshape(B, A),
                returns=(rng.randn(B, A) * 3).astype(f32))


EDGES = ("nan_logits", "masked_slot", "masked_all", "disallowed_action", "action_past_row", "action_negative", "old_logp_minus_inf",
         "d_inside_plus", "d_inside_minus", "d_outside_plus", "d_outside_minus", "adv_zero", "fresh", "r_at_lo", "r_at_hi",
         "clipped_low_adv_pos", "clipped_low_adv_neg", "clipped_high_adv_pos", "clipped_high_adv_neg",
         "q_tie", "dv_at_plus_clip", "dv_at_minus_clip", "dv_past_clip_first", "dv_past_clip_second")


def plant_edges(rows, batch, seed, vf_clip=50.0, moments=None):
    """Plants as many of EDGES as the batch has actors, at distinct actors chosen by `seed`, in place.
    -> {edge: flat actor index}."""
    x, m, act, lp_old = batch["logits"], batch["masks"], batch["actions"], batch["logp_old"]
    B, A, W = x.shape
    N, w = B * A, len(rows)
    x, m, act, lp_old = x.reshape(N, W), m.reshape(N, W), act.reshape(N, w), lp_old.reshape(N, w)
    adv, v, v_old, ret = (batch[k].reshape(N) for k in ("adv", "values", "values_old", "returns"))
    rng = np.random.RandomState(seed)
    where = dict(zip(EDGES, rng.permutation(N)[:len(EDGES)].tolist()))
    lo0, ln0 = rows[0]
    lol, lnl = rows[-1]
    for e, i in where.items():
        if e == "nan_logits":
            for lo, ln in rows:
                k = lo + rng.randint(0, ln)
                if k != lo + act[i, rows.index((lo, ln))]:
                    x[i, k] = np.nan
        elif e == "masked_slot":
            m[i, lo0:lo0 + ln0] = 0.0
        elif e == "masked_all":
            m[i, :] = 0.0
        elif e == "disallowed_action":
            m[i, lol + act[i, -1]] = 0.0
            m[i, lol + (act[i, -1] + 1) % lnl] = 1.0 if lnl > 1 else 0.0
        elif e == "action_past_row":
            act[i, -1] = lnl
        elif e == "action_negative":
            act[i, 0] = -1
        elif e == "old_logp_minus_inf":
            lp_old[i, -1] = -np.inf
        elif e == "adv_zero":
            adv[i] = 0.0 if moments is None else f32(moments[0])
        elif e == "q_tie":
            v_old[i] = 0.0        # dv = v, vc = 0 + v = v: e2 = e1 (vf_clip > |v|)
            v[i] = f32(1.25)
        elif e == "dv_at_plus_clip":
            v_old[i], v[i] = f32(1.5), f32(f32(1.5) + f32(vf_clip))
        elif e == "dv_at_minus_clip":
            v_old[i], v[i] = f32(1.5), f32(f32(1.5) - f32(vf_clip))
        elif e == "dv_past_clip_first":   # the unclipped error is the larger one: the gradient flows
            v_old[i], v[i], ret[i] = f32(0.0), f32(2.0 * vf_clip + 4.0), f32(1.0)
        elif e == "dv_past_clip_second":  # the clipped error is the larger one: no gradient
            v_old[i], v[i], ret[i] = f32(0.0), f32(2.0 * vf_clip + 4.0), f32(4.0 * vf_clip + 9.0)
    # the edges stated in terms of the log-ratio: old logp from the new one
    lp, _ = slot_terms(rows, x, m, act)
    deltas = dict(d_inside_plus=79.9, d_inside_minus=-79.9, d_outside_plus=80.1, d_outside_minus=-80.1, fresh=0.0, r_at_lo=-0.25,
                  r_at_hi=0.25, clipped_low_adv_pos=-0.5, clipped_low_adv_neg=-0.5, clipped_high_adv_pos=0.5,
                  clipped_high_adv_neg=0.5)
    for e, delta in deltas.items():
        if e in where:
            i = where[e]
            lp_old[i] = lp[i]
            with np.errstate(all="ignore"):
                lp_old[i, 0] = f32(lp[i, 0] - f32(delta))
            if e.endswith("adv_pos") or e.endswith("adv_neg"):
                mag = f32(1.5) if moments is None else f32(moments[0] + 1.5 / moments[1])
                neg = f32(-1.5) if moments is None else f32(moments[0] - 1.5 / moments[1])
                adv[i] = mag if e.endswith("adv_pos") else neg
    return where


def ratio_of(rows, batch, i):
    """The ratio r of flat actor i (float32): 1 - r and r - 1 are clip values at which r sits exactly on a clip bound."""
    B, A, W = batch["logits"].shape
    w = len(rows)
    sel = lambda k, last: batch[k].reshape(B * A, last)[i:i + 1]  # noqa: E731
    lp, _ = slot_terms(rows, sel("logits", W), sel("masks", W), sel("actions", w))
    t = actor_terms(lp, sel("logp_old", w), np.zeros(1, f32), 0.3, 1.0)
    assert t["valid"][0]
    return t["r"][0]
