"""Adam under a gradient-norm clip (include/aie.h: aie_adam_step), transcribed in numpy from the contract's text --
independent of csrc/aie_trainer_math.h's code:

    sum of squares, float64: chunks of CHUNK = 1024 consecutive elements; slot s of 256 adds its elements 4s .. 4s + 3
      ascending from +0 (a missing element is +0); slot[i] += slot[i ^ 2^L] for L = 0 .. 7, all i at once; the group's n2
      = its chunk sums ascending from +0, tensor after tensor, chunk after chunk;
    scalars, float64: norm = sqrt(n2); coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1; with t == 0: p1 = p2 = 1;
      t += 1, p1 *= beta1, p2 *= beta2; step = lr / (1 - p1); b2s = sqrt(1 - p2); coef, step, b2s rounded to float32 once;
    per element, float32, each operation rounded on its own: gc = g * coef; m = fmaf(1 - beta1, gc, beta1 * m);
      v = fmaf((1 - beta2) * gc, gc, beta2 * v); d = sqrtf(v) / b2s + eps; w = fmaf(-step, m / d, w);
    a group whose n2 is not finite is skipped: w, m, v and the state keep their bits, stats[3] = 1;
    stats = [norm, coef (0 if skipped), t after the call, skipped].

fmaf is policy_mlp_ref.fma32 (exact); numpy's float32 multiply, divide and sqrt are correctly rounded.  A GROUP here is a
dict: w, m, v (lists of float32 arrays, updated in place), t (int), p1, p2 (float), and hyper-parameters beta1, beta2, eps,
max_norm as float32 values.

Also here: the float64 pass with the running error bound of the float32 evaluation beside it (step_f64), and the random
cases the CPU and the GPU tests share."""
import math

import numpy as np

from policy_mlp_ref import fma32

f32, f64 = np.float32, np.float64
CHUNK, SLOTS, N_STATS = 1024, 256, 4
SIZES = [1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17]
_PARTNER = [np.arange(SLOTS) ^ (1 << L) for L in range(8)]


def chunk_sumsq(g):
    """One chunk (at most CHUNK float32) -> its float64 sum of squares in the contract's order."""
    q = np.zeros(CHUNK, f64)
    q[: g.size] = g.astype(f64)
    q = (q * q).reshape(SLOTS, 4)  # exact: 48 bits
    slot = np.zeros(SLOTS, f64)
    for k in range(4):
        slot = slot + q[:, k]
    for L in range(8):
        slot = slot + slot[_PARTNER[L]]
    return float(slot[0])


def group_sumsq(grads):
    n2 = 0.0
    with np.errstate(all="ignore"):
        for g in grads:
            g = np.asarray(g, f32).reshape(-1)
            for e in range(0, g.size, CHUNK):
                n2 = n2 + chunk_sumsq(g[e: e + CHUNK])
    return n2


def scalars(n2, G, lr):
    """-> (norm, coef, t, p1, p2, step, b2s) in float64 from the group's OLD state; nothing is rounded here."""
    norm = math.sqrt(n2) if n2 == n2 and n2 >= 0 else float("nan")
    mx = float(G["max_norm"])
    coef = min(1.0, mx / (norm + 1e-6)) if mx > 0 else 1.0
    p1, p2 = (1.0, 1.0) if G["t"] == 0 else (G["p1"], G["p2"])
    p1, p2 = p1 * float(G["beta1"]), p2 * float(G["beta2"])
    return norm, coef, G["t"] + 1, p1, p2, float(lr) / (1.0 - p1), math.sqrt(1.0 - p2)


def step(G, grads, lr):
    """One call on one group, in place -> stats (float32 [4])."""
    n2 = group_sumsq(grads)
    if not math.isfinite(n2):
        return np.array([math.sqrt(n2) if n2 > 0 else float("nan"), 0.0, G["t"], 1.0], f32)
    norm, coef, t, p1, p2, stp, b2s = scalars(n2, G, lr)
    coef32, step32, b2s32 = f32(coef), f32(stp), f32(b2s)
    b1, b2, eps = f32(G["beta1"]), f32(G["beta2"]), f32(G["eps"])
    omb1, omb2 = f32(1) - b1, f32(1) - b2
    with np.errstate(all="ignore"):
        for i, g in enumerate(grads):
            g = np.asarray(g, f32).reshape(-1)
            w, m, v = (G[k][i].reshape(-1) for k in "wmv")
            gc = g * coef32
            mn = fma32(omb1, gc, b1 * m)
            vn = fma32(omb2 * gc, gc, b2 * v)
            d = np.sqrt(vn) / b2s32 + eps
            w[:] = fma32(-step32, mn / d, w)
            m[:] = mn
            v[:] = vn
    G["t"], G["p1"], G["p2"] = t, p1, p2
    return np.array([norm, coef32, t, 0.0], f32)


def new_group(sizes, seed, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=0.5, scale=1.0):
    g = np.random.default_rng(seed)
    return dict(w=[(scale * g.standard_normal(n)).astype(f32) for n in sizes], m=[np.zeros(n, f32) for n in sizes],
                v=[np.zeros(n, f32) for n in sizes], t=0, p1=0.0, p2=0.0, beta1=f32(beta1), beta2=f32(beta2), eps=f32(eps),
                max_norm=f32(max_norm))


def copy_group(G):
    return {k: [a.copy() for a in v] if isinstance(v, list) else v for k, v in G.items()}


def random_grads(sizes, seed, scale=1.0):
    """Gradients of standard deviation scale / sqrt(total elements): the group's norm is about `scale`."""
    g = np.random.default_rng(seed)
    total = float(sum(sizes))
    return [(scale / math.sqrt(total) * g.standard_normal(n)).astype(f32) for n in sizes]


def gamma(n, u):
    return n * u / (1.0 - n * u)


def new_f64(G):
    """The float64 pass's state for a float32 group: values and, beside them, the running error bounds (zeros)."""
    z = lambda k: [a.astype(f64) for a in G[k]]  # noqa: E731
    return dict(w=z("w"), m=z("m"), v=z("v"), Ew=[np.zeros(a.size) for a in G["w"]], Em=[np.zeros(a.size) for a in G["w"]],
                Ev=[np.zeros(a.size) for a in G["w"]], t=0, p1=0.0, p2=0.0)


def step_f64(G, S, grads, lr, u=2.0 ** -24):
    """One step of the float64 pass S (new_f64) on the float32 group's hyper-parameters G, with the running bound of an
    evaluation in arithmetic of unit roundoff u around it (no underflow: the tests' magnitudes are far from it).  n2 and
    the float64 scalars are shared -- the float32 evaluation takes them from float64 and rounds coef, step and b2s once
    (relative error u each) -- so both take the same side of the clip.  With tildes for the evaluation's values and
    E_x >= |x~ - x| carried from step to step, gamma_n = n u / (1 - n u):
      gc~ = fl(g fl(coef)):                         E_gc = gamma_2 |gc|
      m'~ = fl(fl(1 - b1) gc~ + fl(b1 m~)):         E_m' = omb1 E_gc + b1 E_m + gamma_3 (omb1 (|gc| + E_gc) + b1 (|m| + E_m))
      v'~ = fl(fl(fl(1 - b2) gc~) gc~ + fl(b2 v~)):  E_g2 = (2 |gc| + E_gc) E_gc,
                                                    E_v' = omb2 E_g2 + b2 E_v + gamma_3 (omb2 (gc^2 + E_g2) + b2 (|v| + E_v))
      r~ = fl(sqrt(v'~)):  |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt(|a - b|)):
                                                    E_r = min(E_v' / sqrt(v'), sqrt(E_v')) (1 + u) + u sqrt(v')
      q~ = fl(r~ / fl(b2s)):                        E_q = (E_r (1 + gamma_2) + gamma_2 sqrt(v')) / b2s
      d~ = fl(q~ + eps):                            E_d = E_q + u (d + E_q)          (d >= eps > 0; asserted: E_d < d)
      x~ = fl(m'~ / d~), x = m' / d:                E_x = (E_m' + |x| E_d) / (d - E_d) (1 + u) + u |x|
      w'~ = fl(-fl(step) x~ + w~):                  E_w' = (E_w + step (E_x (1 + u) + u |x|)) (1 + u) + u |w'|
    -> the largest ratio seen is the caller's to compute: the bounds live in S."""
    n2 = group_sumsq(grads)
    assert math.isfinite(n2)
    norm, coef, t, p1, p2, stp, b2s = scalars(n2, dict(G, t=S["t"], p1=S["p1"], p2=S["p2"]), lr)
    b1, b2, eps = float(G["beta1"]), float(G["beta2"]), float(G["eps"])
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    g2, g3 = gamma(2, u), gamma(3, u)
    for i, g in enumerate(grads):
        g = np.asarray(g, f32).reshape(-1).astype(f64)
        w, m, v, Ew, Em, Ev = (S[k][i] for k in ("w", "m", "v", "Ew", "Em", "Ev"))
        gc = g * coef
        Egc = g2 * np.abs(gc)
        mn = omb1 * gc + b1 * m
        Emn = omb1 * Egc + b1 * Em + g3 * (omb1 * (np.abs(gc) + Egc) + b1 * (np.abs(m) + Em))
        Eg2 = (2.0 * np.abs(gc) + Egc) * Egc
        vn = omb2 * gc * gc + b2 * v
        Evn = omb2 * Eg2 + b2 * Ev + g3 * (omb2 * (gc * gc + Eg2) + b2 * (np.abs(v) + Ev))
        rt = np.sqrt(vn)
        with np.errstate(all="ignore"):
            lip = np.where(rt > 0, Evn / np.where(rt > 0, rt, 1.0), np.inf)
        Er = np.minimum(lip, np.sqrt(Evn)) * (1.0 + u) + u * rt
        Eq = (Er * (1.0 + g2) + g2 * rt) / b2s
        d = rt / b2s + eps
        Ed = Eq + u * (d + Eq)
        assert (Ed < d).all()
        x = mn / d
        Ex = (Emn + np.abs(x) * Ed) / (d - Ed) * (1.0 + u) + u * np.abs(x)
        wn = w - stp * x
        S["Ew"][i] = (Ew + stp * (Ex * (1.0 + u) + u * np.abs(x))) * (1.0 + u) + u * np.abs(wn)
        S["w"][i], S["m"][i], S["v"][i], S["Em"][i], S["Ev"][i] = wn, mn, vn, Emn, Evn
    S["t"], S["p1"], S["p2"] = t, p1, p2
    return norm, coef
