"""Python transcription of the policy evaluation (csrc/aie_trainer_math.h: aie_sampler_logf, aie_policy_row_stats / _logp /
_backward): log-probability, entropy and logit gradient of one action slot under its mask, float32 operation for
operation.  Two forms of the same arithmetic:

  * scalar, on helpers.fmaf (exact rational fused multiply-add), helpers.sampler_expf and the scan order of
    helpers.sampler_pick_row -- the form the bit-for-bit tests hold the header and the kernels to;
  * vectorised over rows of one length (numpy), for the accuracy tests' 100 000 rows: its fused multiply-add goes through
    float64 with round-to-odd (one rounding to float32, like the hardware's), and the tests hold it to the scalar form.
"""
import numpy as np

from helpers import fmaf, sampler_expf

f32 = np.float32
LOG_COEFFS = ("0x1.07826ep-4", "-0x1.dbcd16p-4", "0x1.ec6694p-4", "-0x1.fd3baep-4", "0x1.22db42p-3", "-0x1.554b4ap-3",
              "0x1.99a98p-3", "-0x1.000064p-2", "0x1.55553cp-2", "-0x1.fffffep-2")  # highest first
LN2_HI, LN2_LO = "0x1.62e4p-1", "0x1.7f7d1cp-20"
_h = float.fromhex


def segment(n):
    return 64 if n > 64 else (16 if n <= 16 else 32 if n <= 32 else 64)


# ---- scalar ---------------------------------------------------------------------------------------------------------
def _split(T):
    b = int(f32(T).view(np.uint32))
    mant = b & 0x7fffff
    big = mant > 0x3504f3
    e = (b >> 23) - 127 + int(big)
    m = np.uint32((0x3f000000 if big else 0x3f800000) | mant).view(f32)
    return m, e


def sampler_logf(T):
    m, e = _split(T)
    f = f32(m - f32(1.0))
    h = f32(_h(LOG_COEFFS[0]))
    for c in LOG_COEFFS[1:]:
        h = fmaf(h, f, f32(_h(c)))
    t = f32(f * f)
    lp = fmaf(t, h, f)
    fe = f32(e)
    return fmaf(fe, f32(_h(LN2_HI)), fmaf(fe, f32(_h(LN2_LO)), lp))


def scan64(v, seg):
    """helpers.sampler_pick_row's prefix sums of one 64-entry chunk."""
    zero = f32(0.0)
    for d in (1, 2, 4, 8):
        v = [v[r] + (v[r - d] if (r & 15) >= d else zero) for r in range(64)]
    if seg >= 32:
        v = [v[r] + v[(r & ~15) - 1] if (r >> 4) & 1 else v[r] for r in range(64)]
    if seg >= 64:
        v = [v[r] + v[31] if r >= 32 else v[r] for r in range(64)]
    return v


def _allowed(lg, mask, k):
    return 0 <= k < len(lg) and bool(mask[k] > 0.5) and bool(lg[k] == lg[k])


def row_stats(logits, mask):
    """dict(M, T, S, L, H, any) of one row."""
    lg = [f32(v) for v in logits]
    n = len(lg)
    zero = f32(0.0)
    R = dict(M=f32(-np.inf), T=zero, S=zero, L=zero, H=zero, any=False)
    ok = [_allowed(lg, mask, k) for k in range(n)]
    if not any(ok):
        return R
    with np.errstate(all="ignore"):
        M = R["M"] = max(lg[k] for k in range(n) if ok[k])
        nch, seg = (n + 63) // 64, segment(n)
        cT = cS = zero
        for ch in range(nch):
            w, v = [zero] * 64, [zero] * 64
            for r in range(64):
                k = 64 * ch + r
                if k < n and ok[k]:
                    y = f32(lg[k] - M)
                    w[r] = sampler_expf(y)
                    if y > f32(-80.0):
                        v[r] = f32(w[r] * y)
            w, v = scan64(w, seg), scan64(v, seg)
            cT, cS = f32(cT + w[seg - 1]), f32(cS + v[seg - 1])
        R["T"], R["S"] = cT, cS
        if not cT > 0:
            return R
        R["any"] = True
        R["L"] = sampler_logf(cT)
        R["H"] = f32(R["L"] - f32(cS / cT))
    return R


def row_forward(logits, mask, action):
    """(logp of `action`, entropy) of one row."""
    R = row_stats(logits, mask)
    lg = [f32(v) for v in logits]
    if not R["any"]:
        return f32(0.0), f32(0.0)
    if not _allowed(lg, mask, int(action)):
        return f32(-np.inf), R["H"]
    with np.errstate(all="ignore"):
        return f32(f32(lg[int(action)] - R["M"]) - R["L"]), R["H"]


def row_backward(logits, mask, action, g_logp, g_H):
    """d(g_logp logp + g_H H) / d logits of one row."""
    R = row_stats(logits, mask)
    lg = [f32(v) for v in logits]
    n = len(lg)
    g = np.zeros(n, f32)
    if not R["any"]:
        return g
    gl = f32(g_logp) if _allowed(lg, mask, int(action)) else f32(0.0)
    gh = f32(g_H)
    with np.errstate(all="ignore"):
        for k in range(n):
            if not _allowed(lg, mask, k):
                continue
            y = f32(lg[k] - R["M"])
            p = f32(sampler_expf(y) / R["T"])
            t1 = f32((f32(1.0) if k == int(action) else f32(0.0)) - p)
            a1 = f32(gl * t1)
            lh = f32(f32(y - R["L"]) + R["H"])
            t2 = f32(p * lh) if y > f32(-80.0) else f32(0.0)
            g[k] = f32(a1 - f32(gh * t2))
    return g


# ---- vectorised over rows of one length -----------------------------------------------------------------------------
def fma_v(a, b, c):
    """float32 fused multiply-add on arrays: the product is exact in float64; the sum is rounded to odd there (its
    rounding error from the two-sum), so the final rounding to float32 is the only one that counts."""
    a, b, c = (np.asarray(v, f32).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = np.ascontiguousarray(s).view(np.int64)
        need = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        up = (err > 0) == (s > 0)
        bits = np.where(need, np.where(up, bits + 1, bits - 1), bits)
        return bits.view(np.float64).astype(f32)


def expf_v(y):
    y = np.asarray(y, f32)
    with np.errstate(all="ignore"):
        live = y > f32(-80.0)
        ys = np.where(live, y, f32(0.0))
        n = np.rint(ys * f32(_h("0x1.715476p+0")))
        r = fma_v(n, f32(-_h("0x1.62e4p-1")), ys)
        r = fma_v(n, f32(-_h("0x1.7f7d1cp-20")), r)
        p = np.full(y.shape, f32(_h("0x1.6c16c2p-10")), f32)
        for c in ("0x1.111112p-7", "0x1.555556p-5", "0x1.555556p-3", "0x1p-1", "0x1p+0", "0x1p+0"):
            p = fma_v(p, r, f32(_h(c)))
        return np.where(live, np.ldexp(p, n.astype(np.int32)), f32(0.0)).astype(f32)


def logf_v(T):
    T = np.ascontiguousarray(T, f32)
    b = T.view(np.uint32)
    mant = b & np.uint32(0x7fffff)
    big = mant > 0x3504f3
    e = (b >> np.uint32(23)).astype(np.int32) - 127 + big
    m = (np.where(big, np.uint32(0x3f000000), np.uint32(0x3f800000)) | mant).astype(np.uint32).view(f32)
    f = m - f32(1.0)
    h = np.full(T.shape, f32(_h(LOG_COEFFS[0])), f32)
    for c in LOG_COEFFS[1:]:
        h = fma_v(h, f, f32(_h(c)))
    lp = fma_v(f * f, h, f)
    fe = e.astype(f32)
    return fma_v(fe, f32(_h(LN2_HI)), fma_v(fe, f32(_h(LN2_LO)), lp))


def _scan_v(v, seg):  # v: [R, 64] float32
    r = np.arange(64)
    for d in (1, 2, 4, 8):
        sh = np.zeros_like(v)
        sh[:, d:] = v[:, :-d]
        v = v + np.where((r & 15) >= d, sh, f32(0.0))
    if seg >= 32:
        v = np.where((r >> 4) & 1 == 1, v + v[:, np.maximum((r & ~15) - 1, 0)], v)
    if seg >= 64:
        v = np.where(r >= 32, v + v[:, 31:32], v)
    return v


def rows_stats(logits, mask):
    """Arrays M, T, S, L, H, any (each [R]) and y, w, ok ([R, n]) of R rows of n entries."""
    x = np.asarray(logits, f32)
    R, n = x.shape
    ok = (np.asarray(mask) > 0.5) & (x == x)
    with np.errstate(all="ignore"):
        M = np.where(ok, x, f32(-np.inf)).max(1).astype(f32)
        y = (x - M[:, None]).astype(f32)
        w = np.where(ok, expf_v(y), f32(0.0)).astype(f32)
        v = np.where(ok & (y > f32(-80.0)), w * y, f32(0.0)).astype(f32)
        nch, seg = (n + 63) // 64, segment(n)
        cT, cS = np.zeros(R, f32), np.zeros(R, f32)
        for ch in range(nch):
            cw, cv = np.zeros((R, 64), f32), np.zeros((R, 64), f32)
            m = min(64, n - 64 * ch)
            cw[:, :m], cv[:, :m] = w[:, 64 * ch:64 * ch + m], v[:, 64 * ch:64 * ch + m]
            cT = cT + _scan_v(cw, seg)[:, seg - 1]
            cS = cS + _scan_v(cv, seg)[:, seg - 1]
        alive = cT > 0
        Ts = np.where(alive, cT, f32(1.0)).astype(f32)
        L = np.where(alive, logf_v(Ts), f32(0.0)).astype(f32)
        H = np.where(alive, L - cS / Ts, f32(0.0)).astype(f32)
    return dict(M=M, T=cT, S=cS, L=L, H=H, any=alive, y=y, w=w, ok=ok, Ts=Ts)


def rows_forward(logits, mask, actions):
    S = rows_stats(logits, mask)
    R, n = S["y"].shape
    a = np.asarray(actions).astype(np.int64)
    inr = (a >= 0) & (a < n)
    ac = np.where(inr, a, 0)
    idx = np.arange(R)
    with np.errstate(all="ignore"):
        lp = (S["y"][idx, ac] - S["L"]).astype(f32)
    lp = np.where(inr & S["ok"][idx, ac], lp, f32(-np.inf))
    return np.where(S["any"], lp, f32(0.0)).astype(f32), S["H"]


def rows_backward(logits, mask, actions, g_logp, g_H):
    S = rows_stats(logits, mask)
    R, n = S["y"].shape
    a = np.asarray(actions).astype(np.int64)
    inr = (a >= 0) & (a < n)
    idx = np.arange(R)
    a_ok = inr & S["ok"][idx, np.where(inr, a, 0)]
    gl = np.where(a_ok, np.asarray(g_logp, f32), f32(0.0)).astype(f32)[:, None]
    gh = np.asarray(g_H, f32)[:, None]
    with np.errstate(all="ignore"):
        p = (S["w"] / S["Ts"][:, None]).astype(f32)
        ind = (np.arange(n)[None, :] == a[:, None]).astype(f32)
        a1 = gl * (ind - p)
        lh = (S["y"] - S["L"][:, None]) + S["H"][:, None]
        t2 = np.where(S["y"] > f32(-80.0), p * lh, f32(0.0)).astype(f32)
        g = (a1 - gh * t2).astype(f32)
    return np.where(S["ok"] & S["any"][:, None], g, f32(0.0)).astype(f32)
