"""The convolutional encoder of the egocentric crop (include/aie.h: aie_policy_conv_forward / _backward) and the MLP's
input gradient (aie_policy_mlp_input_grad), transcribed in numpy from the contract in include/aie.h's comments --
independent of the header's code.  A shape is (C_map, D, h, w, V):

    input     C = C_map + 2 D channels: the map's planes, then emb[clamp(idx[i])][d] as channel C_map + i D + d
    conv1     3x3, stride 2, no padding, F1 = 16 filters, ReLU; w1 [9 C, F1] with k = (ky 3 + kx) C + c (Keras' HWIO, flattened)
    conv2     the same with F2 = 32 filters on conv1's output
    features  Keras' Flatten of [oh2, ow2, F2]

Every output is ONE ascending float32 fmaf chain from its bias (policy_mlp_ref.chain: fmaf emulated exactly in float64).
Backward: dz2 = g_feat under a2's mask; da1 over the windows (oy, ox) ascending and f ascending inside; dz1 under a1's mask;
dx likewise for the embedding's channels; a row's embedding table over (i, y, x) ascending; across rows segments of SEG rows,
one chain per weight entry over (row, output position) ascending, the tables added row by row; the segments' partials in
float64, ascending, rounded once.

Also here: the float64 pass with the running bound of a float32 evaluation beside it (the ReLU masks imposed, as in
policy_mlp_bwd_ref), the random weights and the planted inputs the CPU and the GPU tests share."""
import numpy as np

from policy_mlp_ref import U, chain, fma32, gamma, relu

f32, f64 = np.float32, np.float64
F1, F2 = 16, 32
NAMES = ("emb", "w1", "b1", "w2", "b2")

SHAPES = [(7, 4, 11, 11, 100)]  # the shipped one: 7 map planes, idx_emb_dim 4, the 11 x 11 crop, input_emb_vocab 100
EDGE_SHAPES = [
    (7, 4, 7, 7, 100),     # oh2 = ow2 = 1, NF = 32: the smallest crop two such convolutions accept
    (7, 4, 8, 8, 100),     # the last row and column are read by no window
    (7, 4, 9, 11, 100),    # non-square
    (7, 4, 15, 15, 100),   # the maximum
    (1, 1, 11, 11, 100),   # K = 27, no multiple of 4
    (32, 8, 11, 11, 100),  # the widest K
    (7, 4, 11, 11, 1),     # V = 1: every index clamps to the one row
    (7, 4, 11, 11, 128),   # V = 128
]


def dims(shape):
    C_map, D, h, w, V = shape
    oh1, ow1 = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    oh2, ow2 = (oh1 - 3) // 2 + 1, (ow1 - 3) // 2 + 1
    return dict(C_map=C_map, D=D, h=h, w=w, V=V, C=C_map + 2 * D, oh1=oh1, ow1=ow1, oh2=oh2, ow2=ow2, P1=oh1 * ow1, P2=oh2 * ow2,
                NF=oh2 * ow2 * F2)


def random_weights(shape, seed, dead=True):
    """float32 weights ~ N(0, 1 / in) with small biases; dead: a few biases negative enough to kill whole filters."""
    d, g = dims(shape), np.random.default_rng(seed)
    W = {"emb": g.standard_normal((d["V"], d["D"])).astype(f32),
         "w1": (g.standard_normal((9 * d["C"], F1)) / np.sqrt(9 * d["C"])).astype(f32), "b1": (0.1 * g.standard_normal(F1)).astype(f32),
         "w2": (g.standard_normal((9 * F1, F2)) / np.sqrt(9 * F1)).astype(f32), "b2": (0.1 * g.standard_normal(F2)).astype(f32)}
    if dead:
        W["b1"][g.integers(0, F1, 2)] = f32(-1e6)
        W["b2"][g.integers(0, F2, 3)] = f32(-1e6)
        W["w2"][g.integers(0, 9 * F1, 4), g.integers(0, F2, 4)] = 0
    return W


def random_crop(rows, shape, seed, out_of_range=False):
    """(map [rows, C_map, h, w] float32 in [0, 2) with planted zeros and a row of zeros, idx [rows, 2, h, w] int16 with 0 and
    V - 1 among them; out_of_range: some indices below 0 and some at or above V)."""
    d, g = dims(shape), np.random.default_rng(seed)
    m = g.uniform(0, 2, (rows, d["C_map"], d["h"], d["w"])).astype(f32)
    m[g.random(m.shape) < 0.3] = 0
    idx = g.integers(0, d["V"], (rows, 2, d["h"], d["w"])).astype(np.int16)
    idx[0, 0, 0, 0], idx[0, 1, -1, -1] = 0, d["V"] - 1
    if rows > 1:
        m[1] = 0  # an all-zero crop
    if out_of_range:
        idx[g.random(idx.shape) < 0.1] = -3
        idx[g.random(idx.shape) < 0.1] = d["V"]
        idx[g.random(idx.shape) < 0.05] = 32767
        idx[0, 0, 0, 1], idx[0, 0, 0, 2] = -32768, d["V"] + 5
    return m, idx


def clamp(idx, V):
    return np.clip(idx.astype(np.int64), 0, V - 1)


def embed_input(m, idx, emb, dtype=f32):
    """-> X [rows, h, w, C]: the map's planes, then plane 0's embedding, then plane 1's."""
    e = np.asarray(emb, dtype)[clamp(idx, emb.shape[0])]  # [rows, 2, h, w, D]
    return np.concatenate([np.moveaxis(np.asarray(m, dtype), 1, -1), e[:, 0], e[:, 1]], axis=-1)


def im2col(X, oh, ow):
    """X [rows, H, W, C] -> [rows, oh * ow, 9 C] with k = (ky 3 + kx) C + c, windows at stride 2."""
    cols = [X[:, ky:ky + 2 * oh - 1:2, kx:kx + 2 * ow - 1:2, :] for ky in range(3) for kx in range(3)]
    return np.concatenate(cols, axis=-1).reshape(X.shape[0], oh * ow, -1)


def forward(m, idx, W, shape, full=False):
    """-> features [rows, NF] (full: also X, a1 [rows, oh1, ow1, F1])."""
    d = dims(shape)
    rows = m.shape[0]
    X = embed_input(m, idx, W["emb"])
    with np.errstate(all="ignore"):
        a1 = relu(chain(W["b1"], im2col(X, d["oh1"], d["ow1"]).reshape(rows * d["P1"], -1), W["w1"])).reshape(rows, d["oh1"], d["ow1"], F1)
        a2 = relu(chain(W["b2"], im2col(a1, d["oh2"], d["ow2"]).reshape(rows * d["P2"], -1), W["w2"])).reshape(rows, d["NF"])
    return (a2, X, a1) if full else a2


def _transposed(dz, wt, sc, H, Wd):
    """The input gradient of a 3x3 stride-2 convolution: dz [rows, oh, ow, nf], wt [9 sc, nf] -> [rows, H, Wd, sc]; per input
    one chain over the windows (oy, ox) ascending that hold it and over f ascending inside."""
    rows, oh, ow, nf = dz.shape
    acc = np.zeros((rows, H, Wd, sc), f32)
    for oy in range(oh):
        for ox in range(ow):
            for ky in range(3):
                for kx in range(3):  # (each (ky, kx) is another input cell: their order among one another is immaterial)
                    wk = wt[(ky * 3 + kx) * sc:(ky * 3 + kx + 1) * sc]  # [sc, nf]
                    for f in range(nf):
                        acc[:, 2 * oy + ky, 2 * ox + kx, :] = fma32(dz[:, oy, ox, f][:, None], wk[None, :, f], acc[:, 2 * oy + ky, 2 * ox + kx, :])
    return acc


def _entry_sums(act, dz, seg):
    """act [rows, P, K] (None: the constant 1), dz [rows, P, N] -> [K, N] (or [N]): per segment one chain over (row, p)
    ascending, the segments in float64."""
    rows, P, N = dz.shape
    K = act.shape[2] if act is not None else 1
    total = np.zeros((K, N), f64)
    for r0 in range(0, rows, seg):
        acc = np.zeros((K, N), f32)
        for r in range(r0, min(r0 + seg, rows)):
            for p in range(P):
                a = act[r, p][:, None] if act is not None else f32(1)
                acc = fma32(a, dz[r, p][None, :], acc)
        total += acc.astype(f64)
    out = total.astype(f32)
    return out if act is not None else out[0]


def backward(m, idx, W, g_feat, shape, seg):
    """-> dict emb, w1, b1, w2, b2 of float32 gradients in the weights' shapes."""
    d = dims(shape)
    rows, V, D, C_map = m.shape[0], d["V"], d["D"], d["C_map"]
    a2, X, a1 = forward(m, idx, W, shape, full=True)
    with np.errstate(all="ignore"):
        dz2 = np.where(a2 > 0, np.asarray(g_feat, f32), f32(0)).astype(f32).reshape(rows, d["oh2"], d["ow2"], F2)
        da1 = _transposed(dz2, W["w2"], F1, d["oh1"], d["ow1"])
        dz1 = np.where(a1 > 0, da1, f32(0)).astype(f32)
        # the embedding's channels only: the columns of w1 that belong to them
        rows_k = np.array([(t * d["C"]) + C_map + e for t in range(9) for e in range(2 * D)])
        dx = _transposed(dz1, W["w1"][rows_k], 2 * D, d["h"], d["w"])  # [rows, h, w, 2 D]
        G = {"w2": _entry_sums(im2col(a1, d["oh2"], d["ow2"]), dz2.reshape(rows, d["P2"], F2), seg),
             "b2": _entry_sums(None, dz2.reshape(rows, d["P2"], F2), seg),
             "w1": _entry_sums(im2col(X, d["oh1"], d["ow1"]), dz1.reshape(rows, d["P1"], F1), seg),
             "b1": _entry_sums(None, dz1.reshape(rows, d["P1"], F1), seg)}
        # a row's table: (i, y, x) ascending, plain float32 additions from +0
        table = np.zeros((rows, V, D), f32)
        v = clamp(idx, V).reshape(rows, 2, d["h"] * d["w"])
        dxe = dx.reshape(rows, d["h"] * d["w"], 2, D)
        ar = np.arange(rows)
        for i in range(2):
            for cell in range(d["h"] * d["w"]):
                table[ar, v[:, i, cell]] = table[ar, v[:, i, cell]] + dxe[:, cell, i]
        total = np.zeros((V, D), f64)
        for r0 in range(0, rows, seg):
            acc = np.zeros((V, D), f32)
            for r in range(r0, min(r0 + seg, rows)):
                acc = acc + table[r]
            total += acc.astype(f64)
        G["emb"] = total.astype(f32)
    return G


def input_grad(dz1, w1, ncols):
    """aie_policy_mlp_input_grad: dz1 [rows, H], w1 [F, H] -> g_x [rows, ncols], chain0 over k ascending of (dz1[r][k], w1[j][k])."""
    return chain(np.zeros(ncols, f32), dz1, np.asarray(w1, f32)[:ncols].T)


# ---- the float64 pass and the bound of a float32 evaluation around it ----
def _layer64(cols, err, w, b):
    w, b = np.asarray(w, f64), np.asarray(b, f64)
    y = cols @ w + b
    mag = (np.abs(cols) + err) @ np.abs(w) + np.abs(b)
    return y, err @ np.abs(w) + gamma(w.shape[0] + 1) * mag


def forward_f64(m, idx, W, shape, masks=None):
    """-> (features, bound, aux): the float64 pass on the same float32 numbers and the bound of a float32 evaluation, layer by
    layer as policy_mlp_ref.forward_f64 (the input is exact: a copy or a table look-up).  masks (m1, m2): imposed instead
    of the pass's own ReLU decisions (the backward's comparison)."""
    d = dims(shape)
    rows = m.shape[0]
    X = embed_input(m, idx, W["emb"], f64)
    c1 = im2col(X, d["oh1"], d["ow1"]).reshape(rows * d["P1"], -1)
    z1, e1 = _layer64(c1, np.zeros_like(c1), W["w1"], W["b1"])
    m1 = (z1 > 0) if masks is None else masks[0].reshape(z1.shape)
    a1, e1 = (z1 * m1).reshape(rows, d["oh1"], d["ow1"], F1), (e1 if masks is None else e1 * m1).reshape(rows, d["oh1"], d["ow1"], F1)
    c2 = im2col(a1, d["oh2"], d["ow2"]).reshape(rows * d["P2"], -1)
    z2, e2 = _layer64(c2, im2col(e1, d["oh2"], d["ow2"]).reshape(c2.shape), W["w2"], W["b2"])
    m2 = (z2 > 0) if masks is None else masks[1].reshape(z2.shape)
    a2 = (z2 * m2).reshape(rows, d["NF"])
    return a2, (e2 if masks is None else e2 * m2).reshape(rows, d["NF"]), dict(X=X, a1=a1, e1=e1, m1=m1, m2=m2)


def _transposed64(dz, wt, sc, H, Wd):
    rows, oh, ow, nf = dz.shape
    out = np.zeros((rows, H, Wd, sc), f64)
    for oy in range(oh):
        for ox in range(ow):
            for ky in range(3):
                for kx in range(3):
                    out[:, 2 * oy + ky, 2 * ox + kx, :] += dz[:, oy, ox, :] @ wt[(ky * 3 + kx) * sc:(ky * 3 + kx + 1) * sc].T
    return out


def backward_f64(m, idx, W, g_feat, shape, seg, masks, e_g=None):
    """-> (G, E): the float64 gradients under the given ReLU masks (m1 [rows, oh1, ow1, F1], m2 [rows, NF], booleans) and the
    bound of the float32 evaluation of the contract around them.  Derivation, with gamma_n = n u / (1 - n u), u = 2^-24:
      * a sum of n float32 terms in any order, each term a product of inputs off by err, is off by at most
        (the terms' propagated errors) + gamma_n (the sum of the terms' magnitudes, errors included);
      * dz2 is exact (a masked copy); da1 sums at most 4 windows x F2 terms; dz1 is da1 masked; dx sums at most 4 x F1 terms;
      * a weight entry sums min(rows, SEG) P products in float32, the segments in float64, and rounds once: n = that + 2;
        a1 carries the forward's bound e1, the input none;
      * an embedding entry sums at most 2 h w additions per row, SEG rows, the segments, and rounds once.
    e_g: what g_feat itself may be off by (None: exact), propagated through every stage."""
    d = dims(shape)
    rows, V, D, C_map = m.shape[0], d["V"], d["D"], d["C_map"]
    _, _, aux = forward_f64(m, idx, W, shape, masks=masks)
    X, a1, e1 = aux["X"], aux["a1"], aux["e1"]
    w1, w2 = np.asarray(W["w1"], f64), np.asarray(W["w2"], f64)
    dz2 = (np.asarray(g_feat, f64) * masks[1].reshape(rows, -1)).reshape(rows, d["oh2"], d["ow2"], F2)
    e_dz2 = np.zeros_like(dz2) if e_g is None else (np.asarray(e_g, f64) * masks[1].reshape(rows, -1)).reshape(dz2.shape)
    da1 = _transposed64(dz2, w2, F1, d["oh1"], d["ow1"])
    e_da1 = _transposed64(e_dz2, np.abs(w2), F1, d["oh1"], d["ow1"]) + \
        gamma(4 * F2) * _transposed64(np.abs(dz2) + e_dz2, np.abs(w2), F1, d["oh1"], d["ow1"])
    m1 = masks[0].reshape(da1.shape)
    dz1, e_dz1 = da1 * m1, e_da1 * m1
    rows_k = np.array([(t * d["C"]) + C_map + e for t in range(9) for e in range(2 * D)])
    dx = _transposed64(dz1, w1[rows_k], 2 * D, d["h"], d["w"])
    e_dx = _transposed64(e_dz1, np.abs(w1[rows_k]), 2 * D, d["h"], d["w"]) + \
        gamma(4 * F1) * _transposed64(np.abs(dz1) + e_dz1, np.abs(w1[rows_k]), 2 * D, d["h"], d["w"])
    G, E = {}, {}
    for name, bias, act, e_act, dz, e_dz, P in (("w2", "b2", im2col(a1, d["oh2"], d["ow2"]), im2col(e1, d["oh2"], d["ow2"]),
                                                 dz2.reshape(rows, d["P2"], F2), e_dz2.reshape(rows, d["P2"], F2), d["P2"]),
                                                ("w1", "b1", im2col(X, d["oh1"], d["ow1"]), None, dz1.reshape(rows, d["P1"], F1),
                                                 e_dz1.reshape(rows, d["P1"], F1), d["P1"])):
        g = gamma(min(rows, seg) * P + 2)
        e_act = np.zeros_like(act) if e_act is None else e_act
        e_dz = np.zeros_like(dz) if e_dz is None else e_dz
        A, EA = act.reshape(rows * P, -1), e_act.reshape(rows * P, -1)
        Z, EZ = dz.reshape(rows * P, -1), e_dz.reshape(rows * P, -1)
        G[name] = A.T @ Z
        mag = (np.abs(A) + EA).T @ (np.abs(Z) + EZ)
        E[name] = mag - np.abs(A).T @ np.abs(Z) + g * mag
        G[bias] = Z.sum(0)
        E[bias] = EZ.sum(0) + g * (np.abs(Z) + EZ).sum(0)
    v = clamp(idx, V).reshape(rows, 2, d["h"] * d["w"])
    dxe, e_dxe = dx.reshape(rows, d["h"] * d["w"], 2, D), e_dx.reshape(rows, d["h"] * d["w"], 2, D)
    G["emb"], prop, mag = np.zeros((V, D)), np.zeros((V, D)), np.zeros((V, D))
    for i in range(2):
        np.add.at(G["emb"], v[:, i], dxe[:, :, i])
        np.add.at(prop, v[:, i], e_dxe[:, :, i])
        np.add.at(mag, v[:, i], np.abs(dxe[:, :, i]) + e_dxe[:, :, i])
    E["emb"] = prop + gamma(2 * d["h"] * d["w"] + min(rows, seg) + 2) * mag
    return G, E


def input_grad_f64(dz1, w1, ncols):
    """-> (g_x, bound): H products per entry from exact inputs."""
    dz, w = np.asarray(dz1, f64), np.asarray(w1, f64)[:ncols]
    return dz @ w.T, gamma(w.shape[1]) * (np.abs(dz) @ np.abs(w).T)


def network_f64(m, idx, flat, x_p, Wc, Wa, Wp, gl_a, gv_a, gl_p, gv_p, shape, seg, masks_c, masks_a, masks_p):
    """The whole network in float64 with the bound of its float32 evaluation, from the crop to the gradients of all 21
    tensors: the encoder's forward (forward_f64), x_a = [features, flat] with the features' bound, both classes' MLP backward
    with that input error (mlp_backward_f64), the agents' input gradient with its bound as the encoder's g_feat
    (backward_f64, e_g).  masks_*: the float32 contract's ReLU decisions -- (a1 > 0, a2 > 0) and (h1 > 0, h2 > 0) per class --
    imposed on the float64 pass, as in policy_mlp_bwd_ref.  -> (G, E): dicts keyed ("c" | "a" | "p", name)."""
    feat, e_feat, _ = forward_f64(m, idx, Wc, shape, masks=masks_c)
    NF = feat.shape[1]
    xa = np.concatenate([feat, np.asarray(flat, f64)], 1)
    exa = np.concatenate([e_feat, np.zeros(np.asarray(flat).shape)], 1)
    Ga, Ea, gx, egx = mlp_backward_f64(xa, exa, Wa, gl_a, gv_a, seg, masks_a)
    xp = np.asarray(x_p, f64)
    Gp, Ep, _, _ = mlp_backward_f64(xp, np.zeros_like(xp), Wp, gl_p, gv_p, seg, masks_p)
    Gc, Ec = backward_f64(m, idx, Wc, gx[:, :NF], shape, seg, masks_c, e_g=egx[:, :NF])
    G = {("c", k): v for k, v in Gc.items()}
    E = {("c", k): v for k, v in Ec.items()}
    for who, g, e in (("a", Ga, Ea), ("p", Gp, Ep)):
        G.update({(who, k): v for k, v in g.items()})
        E.update({(who, k): v for k, v in e.items()})
    return G, E


def mlp_backward_f64(x, ex, W, g_logits, g_values, seg, masks):
    """One class's MLP backward in float64 from an input x that the float32 evaluation knows only to within ex, under the given
    ReLU masks (m1, m2: [rows, H] booleans) -> (G, E, g_x, e_gx): the eight gradients and the input gradient with the
    bounds of their float32 evaluation.  The rules are backward_f64's: a layer y = b + a @ w from inputs off by e is off by
    e @ |w| + gamma_{K+1} ((|a| + e) @ |w| + |b|); a transposed product of K terms likewise with gamma_K (K + 1 with the value
    column's term); a weight entry sums min(rows, SEG) products in float32, the segments in float64, and rounds once."""
    x, ex = np.asarray(x, f64), np.asarray(ex, f64)
    w = {k: np.asarray(v, f64) for k, v in W.items()}
    wv = w["wv"].reshape(-1)
    m1, m2 = (np.asarray(k, f64) for k in masks)
    rows, F = x.shape
    H, M = w["w2"].shape[0], w["w3"].shape[1]

    def layer(a, e, wt, b, mask):
        y = (a @ wt + b) * mask
        return y, (e @ np.abs(wt) + gamma(wt.shape[0] + 1) * ((np.abs(a) + e) @ np.abs(wt) + np.abs(b))) * mask

    h1, e1 = layer(x, ex, w["w1"], w["b1"], m1)
    h2, e2 = layer(h1, e1, w["w2"], w["b2"], m2)
    dz3, dv = np.asarray(g_logits, f64).reshape(rows, M), np.asarray(g_values, f64).reshape(rows)
    dz2 = (dz3 @ w["w3"].T + dv[:, None] * wv[None, :]) * m2
    e_dz2 = gamma(M + 1) * (np.abs(dz3) @ np.abs(w["w3"]).T + np.abs(dv)[:, None] * np.abs(wv)[None, :]) * m2
    dz1 = (dz2 @ w["w2"].T) * m1
    e_dz1 = (e_dz2 @ np.abs(w["w2"]).T + gamma(H) * ((np.abs(dz2) + e_dz2) @ np.abs(w["w2"]).T)) * m1
    gx = dz1 @ w["w1"].T
    e_gx = e_dz1 @ np.abs(w["w1"]).T + gamma(H) * ((np.abs(dz1) + e_dz1) @ np.abs(w["w1"]).T)
    g = gamma(min(rows, seg) + 2)
    G, E = {}, {}
    zero = np.zeros((rows, 1))
    for name, bias, a, ea, dz, edz in (("w1", "b1", x, ex, dz1, e_dz1), ("w2", "b2", h1, e1, dz2, e_dz2),
                                       ("w3", "b3", h2, e2, dz3, np.zeros_like(dz3)), ("wv", "bv", h2, e2, dv[:, None], zero)):
        mag = (np.abs(a) + ea).T @ (np.abs(dz) + edz)
        G[name], E[name] = a.T @ dz, mag - np.abs(a).T @ np.abs(dz) + g * mag
        G[bias], E[bias] = dz.sum(0), edz.sum(0) + g * (np.abs(dz) + edz).sum(0)
    G["wv"], E["wv"] = G["wv"].reshape(-1), E["wv"].reshape(-1)
    return G, E, gx, e_gx
