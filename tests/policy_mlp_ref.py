"""The policy network's forward pass (include/aie.h: aie_policy_mlp_forward), transcribed in numpy from the contract in
csrc/aie_trainer_math.h's comment -- independent of the header's code:

    chain(c; a, w) = acc, with acc = c and then acc = fmaf(a[k], w[k], acc) for k = 0, 1, ... ascending, all float32
    relu(v) = v > 0 ? v : 0
    h1 = relu(chain(b1; x, W1)),  h2 = relu(chain(b2; h1, W2)),  logits = chain(b3; h2, W3),  value = chain(bv; h2, wv)

fmaf is emulated exactly in float64: the product of two float32 is exact in float64 (48 bits); TwoSum gives the sum's
rounding error; if the sum is inexact and its last mantissa bit is even it moves one ulp towards the error (round to odd);
rounding that to float32 is then the correctly rounded fma (53 >= 24 + 2 bits).  Vectorised over rows and outputs, a Python
loop over k.

Also here: the float64 pass with the running error bound of a float32 chain evaluation beside it, the random weights
and the planted inputs the CPU and the GPU tests share."""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24

# (F, H, M): C2's agents and planner, the smallest, two ragged ones
SHAPES = [(136, 128, 50), (86, 128, 154), (1, 16, 1), (7, 32, 3), (33, 256, 67)]

# ---- the widths the kernel's loops branch on (csrc/aie_kernels_mlp.hip: mlp_tiles, mlp_layer) ----
# A layer with K inputs walks them in k-steps of 4, a staged chunk of CHUNK columns at a time (the first layer; a hidden
# layer's K = H <= CHUNK is one chunk).  Of a chunk's steps the first `nfull` lie wholly inside K; mlp_tiles takes
# G = nfull // KC whole groups of KC steps without a branch -- its loop has four shapes: G = 0, G = 1, G even, G odd and >= 3
# (the `g + 2 < G` refill, then the left-over group) -- and the `tail` steps behind them under their count (the last of them
# ragged where K is no multiple of 4).  The workgroup's four waves share a layer's NT = ceil(N / 16) output tiles in groups
# of eight: NT = 3, 5, 9, 13 leave waves without a tile inside loops that hold barriers.  The value head is column M of the
# head's matrix: where M is a multiple of 16 it opens a tile of its own.
KC, STEP, CHUNK, TILE = 8, 4, 256, 16  # MLP_KC, the MFMA's k, AIE_MLP_CHUNK, the MFMA's columns: test_policy_mlp_cpu.py reads them back
EDGE_SHAPES = [(63, 48, 15), (64, 80, 16), (65, 96, 17), (96, 112, 63), (255, 144, 64), (256, 160, 65), (257, 208, 31),
               (100, 224, 32), (12, 240, 48), (128, 64, 128), (40, 176, 5), (40, 192, 5)]


def loop_shape(K):
    """[(G, tail steps, ragged last step?)] per staged chunk of a layer with K inputs."""
    out, kpad = [], -(-K // STEP) * STEP
    for k0 in range(0, kpad, CHUNK):
        nsteps = min(kpad - k0, CHUNK) // STEP
        nfull = min((K - k0) // STEP, nsteps)
        out.append((nfull // KC, nsteps - nfull // KC * KC, nfull < nsteps))
    return out


def tiles(N):
    return -(-N // TILE)


def loop_class(G):
    return "G=0" if G == 0 else "G=1" if G == 1 else "G even" if G % 2 == 0 else "G odd >= 3"


def coverage_table(shapes=None):
    """One line per shape: per layer the (G, tail) of every chunk and NT (the head's with the value column and without)."""
    lines = []
    for F, H, M in (EDGE_SHAPES if shapes is None else shapes):
        first = " + ".join("G %d tail %d%s" % (g, t, "r" if r else "") for g, t, r in loop_shape(F))
        (g, t, _), = loop_shape(H)
        lines.append("(%3d, %3d, %3d)  first: %s, NT %d;  hidden and head: G %d tail %d;  hidden NT %d, head NT %d / %d" % (
            F, H, M, first, tiles(H), g, t, tiles(H), tiles(M + 1), tiles(M)))
    return "\n".join(lines)


# coverage_table() of EDGE_SHAPES ("r": the tail's last step is ragged; head NT with / without the value column);
# test_policy_mlp_cpu.py holds this text to the function and asserts the classes below it
EDGE_COVERAGE = """\
( 63,  48,  15)  first: G 1 tail 8r, NT 3;  hidden and head: G 1 tail 4;  hidden NT 3, head NT 1 / 1
( 64,  80,  16)  first: G 2 tail 0, NT 5;  hidden and head: G 2 tail 4;  hidden NT 5, head NT 2 / 1
( 65,  96,  17)  first: G 2 tail 1r, NT 6;  hidden and head: G 3 tail 0;  hidden NT 6, head NT 2 / 2
( 96, 112,  63)  first: G 3 tail 0, NT 7;  hidden and head: G 3 tail 4;  hidden NT 7, head NT 4 / 4
(255, 144,  64)  first: G 7 tail 8r, NT 9;  hidden and head: G 4 tail 4;  hidden NT 9, head NT 5 / 4
(256, 160,  65)  first: G 8 tail 0, NT 10;  hidden and head: G 5 tail 0;  hidden NT 10, head NT 5 / 5
(257, 208,  31)  first: G 8 tail 0 + G 0 tail 1r, NT 13;  hidden and head: G 6 tail 4;  hidden NT 13, head NT 2 / 2
(100, 224,  32)  first: G 3 tail 1, NT 14;  hidden and head: G 7 tail 0;  hidden NT 14, head NT 3 / 2
( 12, 240,  48)  first: G 0 tail 3, NT 15;  hidden and head: G 7 tail 4;  hidden NT 15, head NT 4 / 3
(128,  64, 128)  first: G 4 tail 0, NT 4;  hidden and head: G 2 tail 0;  hidden NT 4, head NT 9 / 8
( 40, 176,   5)  first: G 1 tail 2, NT 11;  hidden and head: G 5 tail 4;  hidden NT 11, head NT 1 / 1
( 40, 192,   5)  first: G 1 tail 2, NT 12;  hidden and head: G 6 tail 0;  hidden NT 12, head NT 1 / 1"""


def edge_coverage(shapes=None):
    """The classes the shapes reach, as a set of names (test_policy_mlp_cpu.py asserts the ones the kernel's loops have)."""
    got = set()
    for F, H, M in (EDGE_SHAPES if shapes is None else shapes):
        for g, t, r in loop_shape(F):
            got.add("first layer: %s" % loop_class(g))
        (g, t, _), = loop_shape(H)
        got.add("hidden layer: %s" % loop_class(g))
        if g and g % 2 == 0 and t == KC // 2:
            got.add("hidden layer: G even, a tail of %d steps" % t)
        if g % 2 == 1 and g >= 3 and t == KC // 2:
            got.add("hidden layer: G odd >= 3, a tail of %d steps" % t)
        got.add("NT=%d" % tiles(H))
        got.add("head NT=%d" % tiles(M + 1))
        if M % TILE == 0:
            got.add("the value column alone in a tile")
        got.add("M=%d" % M)
        got.add("F=%d" % F)
        if F > CHUNK:
            got.add("a second staged chunk")
        if F % 64 == 0:
            got.add("the bias row of the backward's [(F + 1), H] block alone in a 64-row group")
    return got


def fma32(a, b, c):
    """float32 fmaf(a, b, c), elementwise with broadcasting."""
    p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)  # exact
    c = np.asarray(c, f32).astype(f64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)  # TwoSum: s + e == p + c exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    towards = np.where((e > 0), np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, towards), s)
    return s.astype(f32)


def chain(c, a, w):
    """a [R, K], w [K, N], c [N] -> [R, N]: one ascending-k fma chain per output."""
    a, w = np.asarray(a, f32), np.asarray(w, f32)
    acc = np.broadcast_to(np.asarray(c, f32), (a.shape[0], w.shape[1])).copy()
    for k in range(a.shape[1]):
        acc = fma32(a[:, k:k + 1], w[k:k + 1, :], acc)
    return acc


def relu(v):
    return np.where(v > 0, v, f32(0)).astype(f32)


def forward(x, W):
    """W: dict w1 [F, H], b1, w2, b2, w3 [H, M], b3, optionally wv [H], bv [1] -> (logits [R, M], value [R] or None)."""
    with np.errstate(all="ignore"):
        h1 = relu(chain(W["b1"], x, W["w1"]))
        h2 = relu(chain(W["b2"], h1, W["w2"]))
        logits = chain(W["b3"], h2, W["w3"])
        value = None
        if W.get("wv") is not None:
            value = chain(W["bv"], h2, np.asarray(W["wv"], f32).reshape(-1, 1))[:, 0]
    return logits, value


def gamma(n):
    return n * U / (1.0 - n * U)


def forward_f64(x, W):
    """The float64 pass on the same float32 numbers, with the error bound of a float32 evaluation beside it: a layer
    y = b + x @ w computed in float32 from inputs that are off by err_in is off by at most
        err_out = sum |w| err_in + gamma_{K+1} (sum |x| |w| + |b|),      gamma_n = n u / (1 - n u), u = 2^-24
    (any order of K fused or unfused multiply-adds; |x| are the float64 pass's magnitudes plus err_in), and ReLU is
    1-Lipschitz.  -> (logits, value or None, bound_logits, bound_value or None), float64."""
    def layer(xv, err, w, b):
        w, b = np.asarray(w, f64), np.asarray(b, f64)
        y = xv @ w + b
        mag = (np.abs(xv) + err) @ np.abs(w) + np.abs(b)
        return y, err @ np.abs(w) + gamma(w.shape[0] + 1) * mag

    xv = np.asarray(x, f64)
    h, e = layer(xv, np.zeros_like(xv), W["w1"], W["b1"])
    h = np.maximum(h, 0.0)
    h2, e2 = layer(h, e, W["w2"], W["b2"])
    h2 = np.maximum(h2, 0.0)
    lg, elg = layer(h2, e2, W["w3"], W["b3"])
    v = ev = None
    if W.get("wv") is not None:
        v, ev = layer(h2, e2, np.asarray(W["wv"], f64).reshape(-1, 1), W["bv"])
        v, ev = v[:, 0], ev[:, 0]
    return lg, v, elg, ev


def random_weights(F, H, M, seed, value=True, dead=True):
    """float32 weights ~ N(0, 1 / in) with small biases; dead: a few negative biases large enough to kill whole ReLU
    columns, and a few zero weights."""
    g = np.random.default_rng(seed)
    W = {}
    for name, (i, o) in (("1", (F, H)), ("2", (H, H)), ("3", (H, M))):
        W["w" + name] = (g.standard_normal((i, o)) / np.sqrt(i)).astype(f32)
        W["b" + name] = (0.1 * g.standard_normal(o)).astype(f32)
    if value:
        W["wv"] = (g.standard_normal(H) / np.sqrt(H)).astype(f32)
        W["bv"] = (0.1 * g.standard_normal(1)).astype(f32)
    if dead:
        W["b1"][g.integers(0, H, max(1, H // 8))] = f32(-1e6)
        W["b2"][g.integers(0, H, max(1, H // 8))] = f32(-1e6)
        W["w2"][g.integers(0, H, 4), g.integers(0, H, 4)] = 0
    return W


def random_rows(rows, F, seed, planted=True):
    """float32 observations in [-2, 2); planted: exact zeros, a row of zeros, entries near 1e-38 and (in rows of their own,
    so that the float32 range holds through three layers) near 1e30."""
    g = np.random.default_rng(seed)
    x = g.uniform(-2, 2, (rows, F)).astype(f32)
    if planted:
        x[g.random((rows, F)) < 0.15] = 0
        x[g.random((rows, F)) < 0.05] = f32(1.2e-38)
        x[g.random((rows, F)) < 0.02] = f32(-3.1e-39)  # a subnormal
        if rows > 2:
            x[1] = 0
            x[2, g.integers(0, F)] = f32(1e30)
        if rows > 5:
            x[5] = (g.choice([-1.0, 1.0], F) * 1e30).astype(f32)
    return x
