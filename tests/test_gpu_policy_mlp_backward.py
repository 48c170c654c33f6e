"""aie_policy_mlp_backward on the device (Backend.policy_mlp_backward, rollout.policy_mlp, MaskedMLPPolicy.evaluate)
against the header's helpers compiled on the CPU (tests/test_policy_mlp_backward_cpu.py holds them to an independent
transcription):

  * values: each shape of policy_mlp_ref.SHAPES as the planner class with the next one as the agents' class in the same
    call, each class alone, the value column on and off, at B = 1 .. 2 SEG + 17 (the agents' 4 B rows cross the row tile's
    and the segment's edges) -- float == with no NaN anywhere, every gradient entry written (the buffers start as NaN),
    64 sentinel floats behind each gradient and 4 KiB behind the workspace untouched; COVID's 51 agents once; the shapes of
    policy_mlp_ref.EDGE_SHAPES (the widths the kernels' loops branch on) the same way at fewer row counts, two of them at
    the segment's edge;
  * a leading dimension larger than F with an address that is only 8-byte aligned equals the contiguous copy; F beyond one
    and two staged chunks with H = 256;
  * two calls, and a call with a second, larger workspace, give the same bits;
  * the refusals return the header's codes and write nothing, neither gradients nor workspace;
  * rollout.policy_mlp under rollout.ppo_loss: .grad of all sixteen tensors equals a direct call on ppo_loss's own
    gradients bit for bit, and lies inside the derived bound around the float64 pass;
  * three updates (forward, ppo_loss, backward, an in-place SGD step) captured in one graph and replayed equal the eager
    ones bit for bit, and the policy's next logits() sees them.
"""
import ctypes as C
import tempfile

import numpy as np
import pytest

import policy_mlp_bwd_ref as bref
import policy_mlp_ref as ref
from helpers import make_env
from test_gpu_policy_evaluate import _cfg
from test_policy_mlp_backward_cpu import build_bwd_shim, c_backward

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
SENTINEL = 64
WS_GUARD = 1024  # floats: 4 KiB
NAMES = bref.NAMES
_ENVS = {}


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as d:
        yield build_bwd_shim(d)


def _be(case="gtb_c2"):
    if case not in _ENVS:
        env = make_env(_cfg(case), n_envs={"gtb_c2": 5, "covid": 1}[case], device=DEV)
        if case != "covid":
            env.seed(3)
        env.reset()
        _ENVS[case] = env
    return _ENVS[case].backend


def _seg():
    from ai_economist_amd import _cabi

    return _cabi.MLP_BWD_SEG


def _dev(a):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


class _Class:
    """One class's operands on the device, its NaN-filled gradient buffers (SENTINEL floats behind each) and the struct."""

    def __init__(self, x, W, gl, gv, x_dev=None):
        import torch

        from ai_economist_amd import _cabi

        self.np = (x, W, gl, gv)
        self.x = x_dev if x_dev is not None else _dev(x)
        self.W = {k: _dev(v) for k, v in W.items()}
        self.gl, self.gv = _dev(gl), _dev(gv)
        self.buf = {k: torch.full((v.numel() + SENTINEL,), float("nan"), device=DEV) for k, v in self.W.items()}
        self.grads = {k: self.buf[k][: v.numel()].view(v.shape) for k, v in self.W.items()}
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        F, H, M = x.shape[1], W["w1"].shape[1], W["w3"].shape[1]
        net = _cabi.AieMlpClass(x=self.x.data_ptr(), x_ld=self.x.stride(0) if x.shape[0] > 1 else F, F=F, H=H, M=M,
                                **{k: p(self.W.get(k)) for k in NAMES})
        self.c = _cabi.AieMlpGradClass(net=net, g_logits=p(self.gl), g_values=p(self.gv),
                                       **{"g" + k: p(self.buf.get(k)) for k in NAMES})

    def clear(self):
        for b in self.buf.values():
            b.fill_(float("nan"))

    def untouched(self):
        import torch

        return all(bool(torch.isnan(b).all()) for b in self.buf.values())


def _call(be, B, ca, cp, extra=0, ws=None):
    """The C call with a NaN-filled workspace of the size the library asks for (+ `extra` floats) and WS_GUARD floats
    behind it -> (return code, the workspace tensor, the floats the call may use)."""
    import torch

    r = lambda c: None if c is None else C.byref(c.c)  # noqa: E731
    need = int(be.lib.aie_policy_mlp_backward_workspace_bytes(be.handle, C.c_int64(B), r(ca), r(cp)))
    use = (max(need, 0) // 4) + extra
    if ws is None:
        ws = torch.full((use + WS_GUARD,), float("nan"), device=DEV)
    rc = be.lib.aie_policy_mlp_backward(be.handle, C.c_int64(B), r(ca), r(cp), C.c_void_p(ws.data_ptr()), C.c_int64(use * 4), be._stream())
    torch.cuda.synchronize()
    return rc, ws, use


def _hold(shim, what, cls, want=None):
    """The device's gradients == the header's; nothing behind them was touched."""
    x, W, gl, gv = cls.np
    want = want if want is not None else c_backward(shim, x, W, gl, gv)
    for k, w in want.items():
        assert not np.isnan(w).any()
        buf = cls.buf[k].cpu().numpy()
        got, tail = buf[: w.size].reshape(w.shape), buf[w.size:]
        assert not np.isnan(got).any(), "%s: %d entries of g%s not written (or NaN)" % (what, np.isnan(got).sum(), k)
        bad = np.argwhere(got != w)
        assert bad.size == 0, "%s: %d of %d entries of g%s differ, first at %s: got %r, want %r" % (
            what, len(bad), w.size, k, bad[0], got[tuple(bad[0])], w[tuple(bad[0])])
        assert np.isnan(tail).all(), "%s: wrote behind g%s" % (what, k)
    return want


def _operands(F, H, M, rows, seed, value):
    W = ref.random_weights(F, H, M, seed=seed, value=value, dead=True)
    x = bref.rows_with_zeros(rows, F, seed=seed + 1)
    gl, gv = bref.random_grads(rows, M, seed=seed + 2, value=value)
    return x, W, gl, gv


ALL_SHAPES = ref.SHAPES + ref.EDGE_SHAPES  # (the edge shapes: the widths the kernels' loops branch on)
# the edge shapes that also run at the segment's edge: F = 64 (the bias row of the [(F + 1), H] block alone in a 64-row group)
# with H = 80, and F past one staged chunk with H = 208 -- the planner's rows SEG - 1, SEG, SEG + 1, the agents' four times that
SEG_EDGE_SHAPES = [(64, 80, 16), (257, 208, 31)]


def _pair(si):
    """The planner's shape and the agents': the next one of the same list."""
    group = ref.SHAPES if si < len(ref.SHAPES) else ref.EDGE_SHAPES
    return ALL_SHAPES[si], group[(group.index(ALL_SHAPES[si]) + 1) % len(group)]


@pytest.mark.parametrize("value", [True, False], ids=["value", "novalue"])
@pytest.mark.parametrize("si", range(len(ALL_SHAPES)), ids=["%dx%dx%d" % s for s in ALL_SHAPES])
def test_device_equals_the_header(shim, si, value):
    import torch

    be = _be()
    n, SEG = be.n, _seg()
    assert n == 4
    (Fp, Hp, Mp), (Fa, Ha, Ma) = _pair(si)  # the agents' class: the next shape in the same call
    counts = (1, 3, 31, 33, 65, SEG - 1, SEG, SEG + 1, 2 * SEG + 17)
    if si >= len(ref.SHAPES):  # the widths are what is new: both row tiles' edges, the agents' 4 B rows past a segment at 65
        counts = (1, 3, 33, 65) + ((SEG - 1, SEG, SEG + 1) if ALL_SHAPES[si] in SEG_EDGE_SHAPES else ())
    for B in counts:
        cp = _Class(*_operands(Fp, Hp, Mp, B, 100 + si + B, value))
        ca = _Class(*_operands(Fa, Ha, Ma, B * n, 200 + si + B, not value))  # (and the other choice of the value column)
        want = {}
        for which in ("both", "planner", "agents"):
            ca.clear(), cp.clear()
            use_a, use_p = which != "planner", which != "agents"
            rc, ws, use = _call(be, B, ca if use_a else None, cp if use_p else None)
            what = "%s B %d (%s)" % (ALL_SHAPES[si], B, which)
            assert rc == 0, (what, be.lib.aie_last_error(be.handle))
            assert bool(torch.isnan(ws[use:]).all()), what + ": wrote behind the workspace"
            for name, cls, used in (("planner", cp, use_p), ("agents", ca, use_a)):
                if used:
                    want[name] = _hold(shim, name + " " + what, cls, want.get(name))
                else:
                    assert cls.untouched(), what


def test_agent_rows_that_are_no_multiple_of_four(shim):
    """COVID's 51 agents: 153 rows in the agents' class."""
    be = _be("covid")
    assert be.n == 51
    F, H, M = ref.SHAPES[0]
    ca = _Class(*_operands(F, H, M, 3 * be.n, 9, True))
    rc, _, _ = _call(be, 3, ca, None)
    assert rc == 0
    _hold(shim, "covid agents", ca)


def test_backend_call_is_the_c_call(shim):
    import torch

    be = _be()
    B = 37
    Fa, Ha, Ma = ref.SHAPES[3]
    Fp, Hp, Mp = ref.SHAPES[0]
    ca, cp = _Class(*_operands(Fa, Ha, Ma, B * be.n, 31, True)), _Class(*_operands(Fp, Hp, Mp, B, 32, False))
    ga, gp = be.policy_mlp_backward(ca.x.view(B, be.n, Fa), cp.x, ca.W, cp.W, ca.gl, cp.gl, ca.gv, None)
    got = be.policy_mlp_backward(ca.x, cp.x, ca.W, cp.W, ca.gl, cp.gl, ca.gv, None, out=(ca.grads, cp.grads))
    torch.cuda.synchronize()
    assert got[0] is not None and all(got[0][k] is ca.grads[k] for k in ca.grads) and set(gp) == set(NAMES[:6])
    _hold(shim, "agents, out=", ca)
    _hold(shim, "planner, out=", cp)
    for g, cls in ((ga, ca), (gp, cp)):
        assert all(g[k].shape == cls.W[k].shape and torch.equal(g[k].view(torch.int32), cls.grads[k].view(torch.int32)) for k in g)
    with pytest.raises(ValueError):
        be.policy_mlp_backward(ca.x, None, ca.W, None, ca.gl, None, None, None)  # wv without g_values
    with pytest.raises(ValueError):
        be.policy_mlp_backward(None, cp.x, None, cp.W, None, cp.gl[:, :3], None, None)


def test_leading_dimension_alignment_and_chunks(shim):
    import torch

    be = _be()
    F, H, M = 86, 128, 154
    rows = 37
    x, W, gl, gv = _operands(F, H, M, rows, 17, True)
    big = torch.full((rows, F + 9), float("nan"), device=DEV)  # rows of 380 bytes; the view starts 8 bytes into them
    big[:, 2: 2 + F] = _dev(x)
    view = big[:, 2: 2 + F]
    assert view.stride(0) == F + 9 and view.data_ptr() % 16 == 8
    strided, contiguous = _Class(x, W, gl, gv, x_dev=view), _Class(x, W, gl, gv)
    for cls in (strided, contiguous):
        assert _call(be, rows, None, cls)[0] == 0
    want = _hold(shim, "x_ld > F", strided)
    _hold(shim, "contiguous", contiguous, want)
    for F, H, M in ((300, 256, 5), (515, 256, 9)):  # F beyond one staged chunk (256 columns), and beyond two
        cls = _Class(*_operands(F, H, M, 35, F, True))
        assert _call(be, 35, None, cls)[0] == 0
        _hold(shim, "F = %d" % F, cls)


def test_two_calls_and_a_larger_workspace_give_the_same_bits():
    import torch

    be = _be()
    B, SEG = 150, _seg()
    assert B * be.n > 2 * SEG
    Fa, Ha, Ma = ref.SHAPES[0]
    Fp, Hp, Mp = ref.SHAPES[1]
    ca, cp = _Class(*_operands(Fa, Ha, Ma, B * be.n, 51, True)), _Class(*_operands(Fp, Hp, Mp, B, 52, True))
    runs = []
    for extra in (0, 0, 12345):
        ca.clear(), cp.clear()
        rc, ws, use = _call(be, B, ca, cp, extra=extra)
        assert rc == 0 and bool(torch.isnan(ws[use:]).all())
        runs.append({w + k: g.clone().view(torch.int32) for w, cls in (("a", ca), ("p", cp)) for k, g in cls.grads.items()})
        assert not any(bool(torch.isnan(g).any()) for cls in (ca, cp) for g in cls.grads.values())
    for again in runs[1:]:
        assert all(torch.equal(runs[0][k], again[k]) for k in runs[0])


def test_refusals_write_nothing():
    import torch

    from ai_economist_amd import _cabi

    be = _be()
    B = 3

    def attempt(F=8, H=32, M=5, value=True, ws_fault=None, **override):
        Fs = max(F, 1)
        x, W, gl, gv = _operands(Fs, H if 16 <= H <= 256 else 32, min(M, 1024), B, 7, True)
        cls = _Class(x, W, gl, gv)
        cls.c.net.F, cls.c.net.H, cls.c.net.M = F, H, M
        if not value:
            cls.c.net.wv = cls.c.net.bv = None
        for k, val in override.items():
            setattr(cls.c.net if k in ("x_ld", "w2") else cls.c, k, val)
        need = int(be.lib.aie_policy_mlp_backward_workspace_bytes(be.handle, C.c_int64(B), None, C.byref(cls.c)))
        ws = torch.full((4096 + WS_GUARD,), float("nan"), device=DEV) if need <= 0 else None
        if ws_fault is None:
            rc, ws, _ = _call(be, B, None, cls, ws=ws)
        else:
            ws = torch.full((need // 4 + WS_GUARD,), float("nan"), device=DEV)
            ptr, size = {"null": (None, need), "misaligned": (ws.data_ptr() + 4, need), "small": (ws.data_ptr(), need - 4)}[ws_fault]
            rc = be.lib.aie_policy_mlp_backward(be.handle, C.c_int64(B), None, C.byref(cls.c), C.c_void_p(ptr), C.c_int64(size),
                                                be._stream())
            torch.cuda.synchronize()
        return rc, need, cls.untouched() and bool(torch.isnan(ws).all())

    rc, need, clean = attempt()
    assert rc == 0 and need > 0 and not clean  # (the call itself is a good one)
    I, U = _cabi.E_INVALID, _cabi.E_UNSUPPORTED
    for kw, code in ((dict(H=24), U), (dict(H=272), U), (dict(H=8), U), (dict(F=0), I), (dict(M=1025), I), (dict(x_ld=7), I),
                     (dict(w2=None), I), (dict(g_logits=None), I), (dict(gw2=None), I), (dict(gb3=None), I),
                     (dict(g_values=None), I), (dict(gwv=None), I), (dict(gbv=None), I), (dict(value=False), I)):
        rc, need, clean = attempt(**kw)
        assert (rc, clean) == (code, True) and need == code, kw
        assert b"aie_policy_mlp_backward" in be.lib.aie_last_error(be.handle)
    for fault in ("null", "misaligned", "small"):
        rc, need, clean = attempt(ws_fault=fault)
        assert (rc, clean) == (I, True) and need > 0, fault
        assert b"workspace" in be.lib.aie_last_error(be.handle)
    c = _cabi.AieMlpGradClass()
    assert be.lib.aie_policy_mlp_backward(be.handle, C.c_int64(0), None, C.byref(c), None, C.c_int64(0), be._stream()) == I  # B < 1
    assert be.lib.aie_policy_mlp_backward(be.handle, C.c_int64(4), None, None, None, C.c_int64(0), be._stream()) == 0  # no class
    assert be.lib.aie_policy_mlp_backward_workspace_bytes(be.handle, C.c_int64(4), None, None) == 0


POLICY_TENSORS = ["%s%s%s" % (k[0], who, k[1]) for who in "ap" for k in NAMES]  # wa1, ba1, ... bpv: sixteen


def _ppo_operands(B, seed):
    """Observations of the policy's widths for B batch elements and ppo_loss's stored operands for them."""
    from test_gpu_ppo_loss import _batches, _env, _stored

    _, be, _, WA, MP = _env("gtb_c2")
    ba, bp, _ = _batches("gtb_c2", B, seed=seed, edges=False)
    return be, WA, MP, _stored(ba, bp)


def _fresh_logp_old(be, pol, dxa, dxp, stored):
    """logp_old := the stored actions' log-probabilities under the policy's own logits, as after a rollout: the first
    update's ratios are exactly 1 (the random batch's own are those of unrelated logits: joint ratios of e^20 and more)."""
    la, lp, _, _ = be.policy_mlp_forward(dxa, dxp, pol.weights_a, pol.weights_p)
    ga, gp, _, _ = be.policy_evaluate(la.view(stored["masks_a"].shape), lp, stored["masks_a"], stored["masks_p"], stored["actions_a"],
                                      stored["actions_p"], entropy=False)
    return dict(stored, logp_old_a=ga.view(stored["logp_old_a"].shape).contiguous(), logp_old_p=gp.view(stored["logp_old_p"].shape).contiguous())


def test_policy_mlp_under_ppo_loss_fills_the_weights_grad(shim):
    import torch

    from ai_economist_amd import rollout

    B = 67  # 268 agent rows: two segments
    be, WA, MP, stored = _ppo_operands(B, seed=21)
    from ai_economist_amd.rollout import MaskedMLPPolicy

    pol = MaskedMLPPolicy(be, network="library", seed=3, value_head=True)
    assert (pol.MA, pol.MP) == (WA, MP) and len(POLICY_TENSORS) == 16
    for k in POLICY_TENSORS:
        getattr(pol, k).requires_grad_(True)
    g = np.random.default_rng(5)
    FA, FP = pol.wa1.shape[0], pol.wp1.shape[0]
    xa, xp = bref.rows_with_zeros(B * be.n, FA, 61), bref.rows_with_zeros(B, FP, 62)
    pol.bav.data.fill_(0.25), pol.ba2.data.copy_(_dev((0.1 * g.standard_normal(pol.ba2.shape[0])).astype(f32)))
    dxa, dxp = _dev(xa), _dev(xp)
    stored = _fresh_logp_old(be, pol, dxa, dxp, stored)
    la, lp, va, vp = pol.evaluate(dxa, dxp)
    assert la.requires_grad and vp.requires_grad
    fwd = be.policy_mlp_forward(dxa, dxp, pol.weights_a, pol.weights_p)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((la, lp, va, vp), fwd))
    la.retain_grad(), lp.retain_grad(), va.retain_grad(), vp.retain_grad()
    loss_a, loss_p, _, _ = rollout.ppo_loss(be, la, lp, va, vp, stored)
    (loss_a + loss_p).backward()
    torch.cuda.synchronize()
    # a direct call on ppo_loss's own gradients
    wa = {k: v.detach() for k, v in pol.weights_a.items()}
    wp = {k: v.detach() for k, v in pol.weights_p.items()}
    ga, gp = be.policy_mlp_backward(dxa, dxp, wa, wp, la.grad.contiguous(), lp.grad.contiguous(), va.grad.contiguous(), vp.grad.contiguous())
    torch.cuda.synchronize()
    assert bool(la.grad.ne(0).any()) and bool(vp.grad.ne(0).any())
    for who, x, grads, gl, gv in (("a", xa, ga, la.grad, va.grad), ("p", xp, gp, lp.grad, vp.grad)):
        W = {k: getattr(pol, "%s%s%s" % (k[0], who, k[1])).detach().cpu().numpy().reshape(grads[k].shape) for k in NAMES}
        G64, E = bref.backward_f64(x, W, gl.cpu().numpy().reshape(x.shape[0], -1), gv.cpu().numpy().reshape(-1), _seg())
        want = c_backward(shim, x, W, gl.cpu().numpy().reshape(x.shape[0], -1), gv.cpu().numpy().reshape(-1))
        worst = 0.0
        for k in NAMES:
            t = getattr(pol, "%s%s%s" % (k[0], who, k[1]))
            assert t.grad is not None and t.grad.shape == t.shape, (who, k)
            assert torch.equal(t.grad.reshape(-1).view(torch.int32), grads[k].reshape(-1).view(torch.int32)), (who, k)
            got = t.grad.cpu().numpy().reshape(G64[k].shape)
            assert (got == want[k].reshape(got.shape)).all(), (who, k)
            err = np.abs(got.astype(np.float64) - G64[k])
            assert (err <= E[k]).all(), "class %s: g%s leaves the derived bound" % (who, k)
            worst = max(worst, float((err / np.maximum(E[k], 1e-300)).max()))
            assert np.abs(got).max() > 0, (who, k)
        print("class %s: max error / bound %.4f" % (who, worst))


def _three_updates(graphed):
    """Three updates -- forward, ppo_loss, backward, w += -lr g on all sixteen tensors -- from one start -> (the weights'
    bits, the policy's logits before and after)."""
    import torch

    from ai_economist_amd.rollout import MaskedMLPPolicy

    B, LR = 40, 0.05
    be, WA, MP, stored = _ppo_operands(B, seed=33)
    pol = MaskedMLPPolicy(be, network="library", seed=3, value_head=True)
    before = [t.clone() for t in pol.logits(be.tensors)]
    FA, FP = pol.wa1.shape[0], pol.wp1.shape[0]
    dxa, dxp = _dev(bref.rows_with_zeros(B * be.n, FA, 71)), _dev(bref.rows_with_zeros(B, FP, 72))
    stored = _fresh_logp_old(be, pol, dxa, dxp, stored)
    f = dict(dtype=torch.float32, device=DEV)
    net = (torch.empty((B * be.n, WA), **f), torch.empty((B, MP), **f), torch.empty(B * be.n, **f), torch.empty(B, **f))
    loss = tuple((torch.empty(8, **f), torch.empty_like(lg), torch.empty_like(v)) for lg, v in ((net[0], net[2]), (net[1], net[3])))
    grads = tuple({k: torch.empty_like(v) for k, v in w.items()} for w in (pol.weights_a, pol.weights_p))
    start = [{k: v.clone() for k, v in w.items()} for w in (pol.weights_a, pol.weights_p)]

    def update():
        be.policy_mlp_forward(dxa, dxp, pol.weights_a, pol.weights_p, out=net)
        be.ppo_loss(net[0], net[1], net[2], net[3], stored, out=loss)
        be.policy_mlp_backward(dxa, dxp, pol.weights_a, pol.weights_p, loss[0][1], loss[1][1], loss[0][2], loss[1][2], out=grads)
        for w, g in zip((pol.weights_a, pol.weights_p), grads):
            for k in w:
                w[k].add_(g[k], alpha=-LR)

    if graphed:
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            update()  # the warm-up: the workspaces exist
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for w, s in zip((pol.weights_a, pol.weights_p), start):  # back to the start
            for k in w:
                w[k].copy_(s[k])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            update()
        for w, s in zip((pol.weights_a, pol.weights_p), start):  # (capture runs nothing; all the same)
            for k in w:
                w[k].copy_(s[k])
        for _ in range(3):
            graph.replay()
    else:
        for _ in range(3):
            update()
    torch.cuda.synchronize()
    after = [t.clone() for t in pol.logits(be.tensors)]
    torch.cuda.synchronize()
    bits = {who + k: v.clone().view(-1).view(torch.int32) for who, w in (("a", pol.weights_a), ("p", pol.weights_p)) for k, v in w.items()}
    moved = all(not torch.equal(w[k], s[k]) for w, s in zip((pol.weights_a, pol.weights_p), start) for k in w)
    return bits, before, after, moved


def test_three_captured_updates_equal_three_eager_ones():
    import torch

    eager, before, after, moved = _three_updates(False)
    assert moved, "an update left a weight tensor where it was"
    assert not torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])
    print("logits after the updates: largest", [float(t.abs().max()) for t in after], "moved by",
          [float((a - b).abs().max()) for a, b in zip(after, before)])
    assert all(bool(torch.isfinite(t).all()) for t in after)
    replayed, before_g, after_g, _ = _three_updates(True)
    assert len(eager) == 16
    for k in eager:
        assert torch.equal(eager[k], replayed[k]), "replayed != eager: " + k
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))  # noqa: E731
    assert all(same(a, b) for a, b in zip(before, before_g)) and all(same(a, b) for a, b in zip(after, after_g))
