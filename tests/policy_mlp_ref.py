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
