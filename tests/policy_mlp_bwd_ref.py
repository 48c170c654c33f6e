"""The policy network's backward pass (include/aie.h: aie_policy_mlp_backward), transcribed in numpy from the contract in
the header's comment -- independent of the helpers' code.  With chain0(a, w) = chain(+0; a, w) of policy_mlp_ref:

    h1, h2 as the forward's;   dz3 = g_logits, dv = g_values
    dh2[j] = chain0 over m ascending of (dz3[m], W3[j][m]), then with a value column fmaf(dv, wv[j], acc)
    dz2 = h2 > 0 ? dh2 : 0;    dh1[j] = chain0 over k ascending of (dz2[k], W2[j][k]);    dz1 = h1 > 0 ? dh1 : 0
    per segment of `seg` consecutive rows: partial(gW_L[k][j]) = chain0 over its rows ascending of (a_L[r][k], dz_L[r][j]),
    a_1 = x, a_2 = h1, a_3 = h2; gwv pairs (h2, dv); a bias is the chain with the activation 1
    entry = the float64 sum of the partials, ascending, rounded to float32 once

Also here: the float64 pass with the running error bound of a float32 evaluation beside it (backward_f64), and the
incoming gradients the CPU and the GPU tests share."""
import numpy as np

import policy_mlp_ref as ref

f32, f64 = np.float32, np.float64
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3", "wv", "bv")


def hidden(x, W):
    """The forward's h1 and h2, float32."""
    with np.errstate(all="ignore"):
        h1 = ref.relu(ref.chain(W["b1"], x, W["w1"]))
        h2 = ref.relu(ref.chain(W["b2"], h1, W["w2"]))
    return h1, h2


def _outer_sum(a, d, seg):
    """a [R, K] (None: the constant 1), d [R, N] -> [K, N] (or [N]): per segment one fma chain over its rows, the partials
    added in float64."""
    rows = d.shape[0]
    a = np.ones((rows, 1), f32) if a is None else np.asarray(a, f32)
    total = np.zeros((a.shape[1], d.shape[1]), f64)
    for r0 in range(0, rows, seg):
        acc = np.zeros(total.shape, f32)
        for r in range(r0, min(r0 + seg, rows)):
            acc = ref.fma32(a[r][:, None], d[r][None, :], acc)
        total = total + acc.astype(f64)
    return total.astype(f32)


def backward(x, W, g_logits, g_values, seg):
    """-> dict of the eight gradients (six without a value column), float32, in the weights' shapes."""
    x, g_logits = np.asarray(x, f32), np.asarray(g_logits, f32)
    value = W.get("wv") is not None
    h1, h2 = hidden(x, W)
    zero_h = np.zeros(W["w1"].shape[1], f32)
    with np.errstate(all="ignore"):
        dh2 = ref.chain(zero_h, g_logits, np.asarray(W["w3"], f32).T)
        if value:
            g_values = np.asarray(g_values, f32)
            dh2 = ref.fma32(g_values[:, None], np.asarray(W["wv"], f32).reshape(1, -1), dh2)
        dz2 = np.where(h2 > 0, dh2, f32(0)).astype(f32)
        dh1 = ref.chain(zero_h, dz2, np.asarray(W["w2"], f32).T)
        dz1 = np.where(h1 > 0, dh1, f32(0)).astype(f32)
        G = {"w1": _outer_sum(x, dz1, seg), "b1": _outer_sum(None, dz1, seg)[0],
             "w2": _outer_sum(h1, dz2, seg), "b2": _outer_sum(None, dz2, seg)[0],
             "w3": _outer_sum(h2, g_logits, seg), "b3": _outer_sum(None, g_logits, seg)[0]}
        if value:
            G["wv"] = _outer_sum(h2, g_values[:, None], seg)[:, 0]
            G["bv"] = _outer_sum(None, g_values[:, None], seg)[0]
    return G


def backward_f64(x, W, g_logits, g_values, seg):
    """The float64 pass on the same float32 numbers with the float32 forward's ReLU masks imposed (m1 = h1 > 0 and
    m2 = h2 > 0 of policy_mlp_ref's float32 pass; both passes then differentiate the same piecewise-linear function), and
    beside it the bound of a float32 evaluation -> (gradients, bounds), two dicts of float64 arrays.

    gamma_n = n u / (1 - n u), u = 2^-24, bounds a sum of n terms (or n - 1 and a start value) in any order of fused or
    unfused multiply-adds.  Hats are the float32 evaluation's values, e_* its distance from this pass:
      z1 = x W1 + b1, h1 = m1 z1:   ^h1 = relu(^z1) = m1 ^z1 (the mask is ^z1's own), so
                                    e_h1 = m1 gamma_{F+1} (|x| |W1| + |b1|);
      h2 = m2 (h1 W2 + b2):         e_h2 = m2 (e_h1 |W2| + gamma_{H+1} ((|h1| + e_h1) |W2| + |b2|))     (as forward_f64);
      dz3, dv are inputs: exact;
      dh2 = dz3 W3^T + dv wv^T:     M + v terms from zero: e_dz2 = m2 gamma_{M+v} (|dz3| |W3|^T + |dv| |wv|^T);
      dh1 = dz2 W2^T:               e_dz1 = m1 (e_dz2 |W2|^T + gamma_H (|dz2| + e_dz2) |W2|^T);
      g[k][j] = sum_r a[r][k] d[r][j], bilinear in two perturbed operands, every term passing through at most
      n = min(rows, seg) roundings of its segment's chain plus one per segment of the sum (the float64 adds and the one
      rounding to float32 are no more than that):
        e_g = e_a^T |d| + |a|^T e_d + e_a^T e_d + gamma_n (|a| + e_a)^T (|d| + e_d);   a bias has a = 1, e_a = 0."""
    x64, gl = np.asarray(x, f64), np.asarray(g_logits, f64)
    value = W.get("wv") is not None
    h1_32, h2_32 = hidden(x, W)
    m1, m2 = (h1_32 > 0).astype(f64), (h2_32 > 0).astype(f64)
    w1, b1, w2, b2, w3 = (np.asarray(W[k], f64) for k in ("w1", "b1", "w2", "b2", "w3"))
    F, H = w1.shape
    M = w3.shape[1]
    g = ref.gamma
    h1 = m1 * (x64 @ w1 + b1)
    e_h1 = m1 * g(F + 1) * (np.abs(x64) @ np.abs(w1) + np.abs(b1))
    h2 = m2 * (h1 @ w2 + b2)
    e_h2 = m2 * (e_h1 @ np.abs(w2) + g(H + 1) * ((np.abs(h1) + e_h1) @ np.abs(w2) + np.abs(b2)))
    dh2, mag = gl @ w3.T, np.abs(gl) @ np.abs(w3).T
    if value:
        gv, wv = np.asarray(g_values, f64), np.asarray(W["wv"], f64).reshape(-1)
        dh2 = dh2 + gv[:, None] * wv[None, :]
        mag = mag + np.abs(gv)[:, None] * np.abs(wv)[None, :]
    dz2, e_dz2 = m2 * dh2, m2 * g(M + (1 if value else 0)) * mag
    dz1 = m1 * (dz2 @ w2.T)
    e_dz1 = m1 * (e_dz2 @ np.abs(w2).T + g(H) * ((np.abs(dz2) + e_dz2) @ np.abs(w2).T))
    rows = x64.shape[0]
    n = min(rows, seg) + -(-rows // seg)

    def grad(a, e_a, d, e_d):
        val = a.T @ d
        err = e_a.T @ np.abs(d) + np.abs(a).T @ e_d + e_a.T @ e_d + g(n) * ((np.abs(a) + e_a).T @ (np.abs(d) + e_d))
        return val, err

    one, zero = np.ones((rows, 1)), np.zeros((rows, 1))
    G, E = {}, {}
    for name, a, e_a, d, e_d in (("1", x64, np.zeros_like(x64), dz1, e_dz1), ("2", h1, e_h1, dz2, e_dz2),
                                 ("3", h2, e_h2, gl, np.zeros_like(gl))):
        G["w" + name], E["w" + name] = grad(a, e_a, d, e_d)
        gb, eb = grad(one, zero, d, e_d)
        G["b" + name], E["b" + name] = gb[0], eb[0]
    if value:
        gw, ew = grad(h2, e_h2, gv[:, None], zero)
        G["wv"], E["wv"] = gw[:, 0], ew[:, 0]
        gb, eb = grad(one, zero, gv[:, None], zero)
        G["bv"], E["bv"] = gb[0], eb[0]
    return G, E


def random_grads(rows, M, seed, value=True):
    """Incoming gradients drawn like aie_ppo_loss's grad_logits and grad_values: every row of g_logits with several allowed entries sums to
    (nearly) zero, the entries a mask would forbid are exact zeros, a few rows are zero altogether; of the size 1 / rows."""
    g = np.random.default_rng(seed)
    allowed = g.random((rows, M)) < 0.7
    allowed[:, 0] = True
    gl = np.where(allowed, g.standard_normal((rows, M)), 0.0)
    several = allowed.sum(1, keepdims=True) > 1  # (a row with one allowed entry keeps it: all zeros would test nothing)
    gl -= (allowed & several) * (gl.sum(1, keepdims=True) / allowed.sum(1, keepdims=True))
    gv = g.standard_normal(rows)
    dead = g.random(rows) < 0.1
    gl[dead] = 0
    gv[dead & (g.random(rows) < 0.5)] = 0
    gl = (gl / rows).astype(f32)
    gl[~allowed] = 0
    return gl, ((gv / rows).astype(f32) if value else None)


def rows_with_zeros(rows, F, seed):
    """policy_mlp_ref.random_rows without the extreme magnitudes, with exact zeros."""
    x = ref.random_rows(rows, F, seed, planted=False)
    x[np.random.default_rng(seed + 1).random((rows, F)) < 0.15] = 0
    return x
