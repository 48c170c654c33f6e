"""aie_policy_conv_forward, aie_policy_mlp_input_grad and aie_policy_conv_backward on the device (Backend.policy_conv_forward,
.policy_mlp_input_grad, .policy_conv_backward, rollout.policy_conv_mlp, MaskedMLPPolicy(spatial=True)) against the header's
helpers compiled on the CPU (tests/test_policy_conv_cpu.py holds them to an independent transcription), on 5 replicas of the
headline configuration:

  * forward: bit for bit the header's for every shape of policy_conv_ref.SHAPES (at 1, 3, tile - 1, tile, tile + 1, SEG + 1,
    2 SEG + 17 rows) and EDGE_SHAPES (1, 3, tile + 1); the output starts as NaN and every entry is written; an x_ld larger
    than NF + F_flat leaves the gap's NaNs and 64 sentinel floats behind alone; flat = None writes the features only; row
    strides larger than a row with 8-byte-aligned bases equal the contiguous copy;
  * on the real arena after a reset and after a few steps, against the header fed with the downloaded tensors;
  * the input gradient: the header's chain on the workspace's dz1 for ncols in {1, NF, F}, nothing written behind it, and
    the backward's sixteen gradients the same bits whether or not it runs;
  * the backward: all five gradients the header's, two calls and a larger workspace the same bits, 4 KiB behind the
    workspace untouched, refusals write nothing;
  * rollout.policy_conv_mlp under rollout.ppo_loss: .grad of all 21 tensors equals the direct calls bit for bit and lies
    inside the bound, propagated from the chain lengths through every stage (policy_conv_ref.network_f64), around torch's
    float64 pass of the whole network from the crop on (embedding, cat, two conv2d, flatten, cat, the MLPs, on the loss's
    gradients; the float32 contract's ReLU decisions, computed on the CPU, imposed); each stage also equals the header's
    on the device's own intermediates bit for bit;
  * two updates (encoder, MLP, loss, the three backward calls, Adam.step) captured in one graph equal the eager ones;
  * MaskedMLPPolicy(spatial=True) in a GraphedStep replay gives the eager run's actions, the next logits() sees updated
    weights, and spatial=False gives the same logits as a direct policy_mlp_forward call on its weights.
"""
import ctypes as C
import tempfile

import numpy as np
import pytest

import policy_conv_ref as cref
import policy_mlp_bwd_ref as bref
from helpers import make_env
from test_gpu_policy_evaluate import _cfg
from test_policy_conv_cpu import build_conv_shim, c_backward, c_forward, hold_network, random_g_feat

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DEV = "cuda:0"
SENTINEL = 64
WS_GUARD = 1024  # floats: 4 KiB
NAMES = cref.NAMES
_ENVS = {}


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as d:
        yield build_conv_shim(d)


@pytest.fixture(scope="module")
def mlp_shim():
    from test_policy_mlp_backward_cpu import build_bwd_shim

    with tempfile.TemporaryDirectory() as d:
        yield build_bwd_shim(d)


def _env(key="shared", **kw):
    if key not in _ENVS:
        env = make_env(dict(_cfg("gtb_c2"), **kw), n_envs=5, device=DEV)
        env.seed(3)
        env.reset()
        _ENVS[key] = env
    return _ENVS[key]


def _be():
    return _env().backend


def _seg():
    from ai_economist_amd import _cabi

    return _cabi.MLP_BWD_SEG


def _dev(a):
    import torch

    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _tile(shape):
    """Rows per workgroup: as many as 64 KB of LDS hold, at most 16 (csrc/aie_trainer_plan.h; test_policy_conv_cpu.py holds the
    plan to this formula)."""
    d = cref.dims(shape)
    lds_row, tr = d["h"] * d["w"] * d["C"] + d["P1"] * cref.F1, 16
    while tr > 1 and 4 * tr * lds_row > 65536:
        tr //= 2
    return tr


def _row_counts(shape):
    tr, SEG = _tile(shape), _seg()
    if shape in cref.SHAPES:
        return sorted({1, 3, max(tr - 1, 1), tr, tr + 1, SEG + 1, 2 * SEG + 17})
    return sorted({1, 3, tr + 1})


def _bits(t):
    import torch

    return t.contiguous().view(-1).view(torch.int32)


@pytest.mark.parametrize("shape", cref.SHAPES + cref.EDGE_SHAPES, ids=lambda s: "%dx%d_%dx%d_V%d" % s)
def test_forward_equals_the_header(shim, shape):
    import torch

    be, d = _be(), cref.dims(shape)
    NF, F_flat, GAP = d["NF"], 37, 5
    for i, rows in enumerate(_row_counts(shape)):
        W = cref.random_weights(shape, seed=41 * d["C"] + i, dead=True)
        m, idx = cref.random_crop(rows, shape, seed=19 * d["h"] + i, out_of_range=(i == 1))
        flat = np.random.default_rng(i).standard_normal((rows, F_flat)).astype(f32)
        want = c_forward(shim, m, idx, W, shape)
        Wd = {k: _dev(v) for k, v in W.items()}
        x_ld = NF + F_flat + GAP
        buf = torch.full((rows * x_ld + SENTINEL,), float("nan"), device=DEV)
        out = buf[: rows * x_ld].view(rows, x_ld)
        got = be.policy_conv_forward(_dev(m), _dev(idx), _dev(flat), Wd, out=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        x = host[: rows * x_ld].reshape(rows, x_ld)
        assert not np.isnan(x[:, : NF + F_flat]).any(), "%s, %d rows: entries not written" % (shape, rows)
        assert x[:, :NF].tobytes() == want.tobytes(), "%s, %d rows: %d features differ" % (shape, rows, (x[:, :NF] != want).sum())
        assert x[:, NF:NF + F_flat].tobytes() == flat.tobytes()
        assert np.isnan(x[:, NF + F_flat:]).all() and np.isnan(host[rows * x_ld:]).all(), "wrote into the gap or behind x_out"
        # flat = None: the features only, into a contiguous tensor of the call's own
        only = be.policy_conv_forward(_dev(m), _dev(idx), None, Wd)
        assert tuple(only.shape) == (rows, NF) and only.cpu().numpy().tobytes() == want.tobytes()
        if i < 3:  # row strides larger than a row, bases only 8-byte aligned
            mb = torch.full((rows * (m[0].size + 2) + 2,), float("nan"), device=DEV)
            ms = mb[2:].view(rows, m[0].size + 2)[:, : m[0].size].view(rows, *m.shape[1:]) if rows == 1 else \
                torch.as_strided(mb, (rows,) + m.shape[1:], (m[0].size + 2, d["h"] * d["w"], d["w"], 1), 2)
            ms.copy_(_dev(m))
            ib = torch.zeros((rows * (idx[0].size + 4) + 4,), dtype=torch.int16, device=DEV)
            is_ = torch.as_strided(ib, (rows,) + idx.shape[1:], (idx[0].size + 4, d["h"] * d["w"], d["w"], 1), 4)
            is_.copy_(_dev(idx))
            fb = torch.zeros((rows, F_flat + 3), device=DEV)
            fb[:, :F_flat].copy_(_dev(flat))
            assert ms.data_ptr() % 16 == 8 and is_.data_ptr() % 16 == 8
            strided = be.policy_conv_forward(ms, is_, fb[:, :F_flat], Wd)
            assert strided.cpu().numpy().tobytes() == x[:, : NF + F_flat].tobytes(), "strided operands differ"


def _arena_weights(be, seed):
    t = be.tensors
    C_map, h, w = (int(v) for v in t["obs_a_world-map"].shape[-3:])
    shape = (C_map, 4, h, w, 100)
    return shape, cref.random_weights(shape, seed=seed, dead=False)


def test_forward_on_the_real_arena(shim):
    import torch

    env = _env("arena")
    be = env.backend
    t = be.tensors
    shape, W = _arena_weights(be, 7)
    assert shape[:1] + shape[2:4] == (7, 11, 11) and t["obs_a_world-idx_map"].dtype == torch.int16
    Wd = {k: _dev(v) for k, v in W.items()}
    for steps in (0, 4):
        for _ in range(steps):
            a, p = be.sample_masked_actions(1234)
            be.step(a, p)
        got = be.policy_conv_forward(t["obs_a_world-map"], t["obs_a_world-idx_map"], t["obs_a_flat"], Wd)
        torch.cuda.synchronize()
        m = t["obs_a_world-map"].cpu().numpy().reshape(-1, *shape[:1], *shape[2:4])
        idx = t["obs_a_world-idx_map"].cpu().numpy().reshape(-1, 2, *shape[2:4])
        flat = t["obs_a_flat"].cpu().numpy().reshape(m.shape[0], -1)
        want = c_forward(shim, m, idx, W, shape)
        g = got.cpu().numpy()
        assert g.shape == (be.E * be.n, 128 + flat.shape[1])
        assert g[:, :128].tobytes() == want.tobytes() and g[:, 128:].tobytes() == flat.tobytes(), "after %d steps" % steps
        assert (want > 0).any() and idx.max() > 0
    assert int(t["error_flags"].abs().sum()) == 0


def _mlp_case(rows_a, F, H, M, seed):
    """An MLP backward's operands for the agents' class of B = rows_a / n batch elements."""
    import policy_mlp_ref as ref

    W = ref.random_weights(F, H, M, seed=seed, value=True, dead=True)
    x = bref.rows_with_zeros(rows_a, F, seed=seed + 1)
    gl, gv = bref.random_grads(rows_a, M, seed=seed + 2, value=True)
    return x, W, gl, gv


def test_input_grad_equals_the_header_and_leaves_the_backward_alone(shim):
    import torch

    be = _be()
    NF, F, H, M = 128, 264, 128, 50
    for B in (1, 5, 65):
        rows = B * be.n
        x, W, gl, gv = _mlp_case(rows, F, H, M, seed=B)
        xp, Wp, glp, gvp = _mlp_case(B * be.n, 86, 128, 154, seed=B + 50)
        xp, glp, gvp = xp[:B], glp[:B], gvp[:B]
        ops = (_dev(x), _dev(xp), {k: _dev(v) for k, v in W.items()}, {k: _dev(v) for k, v in Wp.items()}, _dev(gl), _dev(glp),
               _dev(gv), _dev(gvp))
        ga0, gp0 = be.policy_mlp_backward(*ops)
        torch.cuda.synchronize()
        base = {("a", k): _bits(v).clone() for k, v in ga0.items()}
        base.update({("p", k): _bits(v).clone() for k, v in gp0.items()})
        for ncols in (1, NF, F):
            ga, gp = be.policy_mlp_backward(*ops)
            ld = ncols + 3
            buf = torch.full((rows * ld + SENTINEL,), float("nan"), device=DEV)
            out = buf[: rows * ld].view(rows, ld)
            pb = torch.full((B * 86 + SENTINEL,), float("nan"), device=DEV)
            g_x, g_xp = be.policy_mlp_input_grad(ncols_a=ncols, ncols_p=86, out=(out, pb[: B * 86].view(B, 86)))
            torch.cuda.synchronize()
            for (who, k), bits in base.items():
                assert torch.equal(_bits((ga if who == "a" else gp)[k]), bits), "the backward's g%s_%s changed" % (k, who)
            ws = be._mlp_bwd_ws.cpu().numpy()
            dz1 = ws[3 * rows * H: 4 * rows * H].reshape(rows, H)
            fl_a = 4 * rows * H + -(-rows // _seg()) * ((F + 1) * H + (H + 1) * H + (H + 1) * (M + 1))
            off_p = -(-fl_a // 64) * 64
            dz1p = ws[off_p + 3 * B * 128: off_p + 4 * B * 128].reshape(B, 128)
            assert not np.isnan(dz1).any() and (dz1 == 0).any() and np.abs(dz1).max() > 0
            host = buf.cpu().numpy()
            got = host[: rows * ld].reshape(rows, ld)
            want = np.full((rows, ncols), np.nan, f32)
            shim.shim_input_grad(dz1.ctypes.data, W["w1"].ctypes.data, rows, H, ncols, want.ctypes.data, ncols)
            assert got[:, :ncols].tobytes() == want.tobytes(), "B %d, ncols %d" % (B, ncols)
            assert np.isnan(got[:, ncols:]).all() and np.isnan(host[rows * ld:]).all(), "wrote behind g_x"
            wantp = np.full((B, 86), np.nan, f32)
            shim.shim_input_grad(dz1p.ctypes.data, Wp["w1"].ctypes.data, B, 128, 86, wantp.ctypes.data, 86)
            hp = pb.cpu().numpy()
            assert hp[: B * 86].tobytes() == wantp.tobytes() and np.isnan(hp[B * 86:]).all()
            g64, bound = cref.input_grad_f64(dz1, W["w1"], ncols)
            assert (np.abs(want.astype(f64) - g64) <= bound).all()
        # a class left out
        be.policy_mlp_backward(*ops)
        only_p = be.policy_mlp_input_grad(ncols_p=5)
        assert only_p[0] is None and tuple(only_p[1].shape) == (B, 5)
    with pytest.raises(ValueError):
        be.policy_mlp_input_grad(ncols_a=F + 1)


class _Grad:
    """The backward's operands on the device, NaN-filled gradient buffers with SENTINEL floats behind each, the struct."""

    def __init__(self, be, shape, rows, seed, g_ld_extra=0):
        import torch

        from ai_economist_amd import _cabi

        d = cref.dims(shape)
        self.shape, self.rows = shape, rows
        self.W = cref.random_weights(shape, seed=seed, dead=True)
        self.m, self.idx = cref.random_crop(rows, shape, seed=seed + 1, out_of_range=(rows == 3))
        self.gf = random_g_feat(rows, d["NF"] + g_ld_extra, seed=seed + 2)
        self.dm, self.di, self.dg = _dev(self.m), _dev(self.idx), _dev(self.gf)
        self.Wd = {k: _dev(v) for k, v in self.W.items()}
        self.buf = {k: torch.full((v.numel() + SENTINEL,), float("nan"), device=DEV) for k, v in self.Wd.items()}
        self.out = {k: self.buf[k][: v.numel()].view(v.shape) for k, v in self.Wd.items()}
        net = _cabi.AieConvClass(map=self.dm.data_ptr(), map_ld=self.m[0].size, idx=self.di.data_ptr(), idx_ld=self.idx[0].size,
                                 **{k: self.Wd[k].data_ptr() for k in NAMES}, C_map=shape[0], D=shape[1], h=shape[2], w=shape[3], V=shape[4])
        self.c = _cabi.AieConvGradClass(net=net, g_feat=self.dg.data_ptr(), g_ld=self.gf.shape[1],
                                        **{"g" + k: self.buf[k].data_ptr() for k in NAMES})

    def want(self, shim):
        return c_backward(shim, self.m, self.idx, self.W, self.gf[:, : cref.dims(self.shape)["NF"]], self.shape) \
            if self.gf.shape[1] == cref.dims(self.shape)["NF"] else self._want_ld(shim)

    def _want_ld(self, shim):
        NF = cref.dims(self.shape)["NF"]
        return c_backward(shim, self.m, self.idx, self.W, np.ascontiguousarray(self.gf[:, :NF]), self.shape)

    def clear(self):
        for b in self.buf.values():
            b.fill_(float("nan"))

    def untouched(self):
        import torch

        return all(bool(torch.isnan(b).all()) for b in self.buf.values())


def _call(be, g, extra=0, ws=None, short=0):
    import torch

    need = int(be.lib.aie_policy_conv_backward_workspace_bytes(be.handle, C.c_int64(g.rows), C.byref(g.c)))
    use = max(need, 0) // 4 + extra
    if ws is None:
        ws = torch.full((use + WS_GUARD,), float("nan"), device=DEV)
    rc = be.lib.aie_policy_conv_backward(be.handle, C.c_int64(g.rows), C.byref(g.c), C.c_void_p(ws.data_ptr()), C.c_int64(use * 4 - short),
                                         be._stream())
    torch.cuda.synchronize()
    return rc, ws, use, need


def _hold(what, g, want):
    for k, w in want.items():
        buf = g.buf[k].cpu().numpy()
        got, tail = buf[: w.size].reshape(w.shape), buf[w.size:]
        assert not np.isnan(got).any(), "%s: %d entries of g%s not written" % (what, np.isnan(got).sum(), k)
        bad = np.argwhere(got != w)
        assert bad.size == 0, "%s: %d of %d entries of g%s differ, first at %s: got %r, want %r" % (
            what, len(bad), w.size, k, bad[0], got[tuple(bad[0])], w[tuple(bad[0])])
        assert got.tobytes() == w.tobytes(), (what, k)
        assert np.isnan(tail).all(), "%s: wrote behind g%s" % (what, k)


@pytest.mark.parametrize("shape", cref.SHAPES + cref.EDGE_SHAPES, ids=lambda s: "%dx%d_%dx%d_V%d" % s)
def test_backward_equals_the_header(shim, shape):
    be = _be()
    for i, rows in enumerate(_row_counts(shape)):
        g = _Grad(be, shape, rows, seed=100 * i + shape[2], g_ld_extra=(3 if i % 2 else 0))
        rc, ws, use, need = _call(be, g)
        assert rc == 0, be.lib.aie_last_error(be.handle)
        what = "%s, %d rows" % (shape, rows)
        _hold(what, g, g.want(shim))
        assert np.isnan(ws[use:].cpu().numpy()).all(), what + ": wrote behind the workspace"
        first = {k: _bits(v).clone() for k, v in g.out.items()}
        if i in (0, len(_row_counts(shape)) - 1):  # two calls, and a larger workspace elsewhere: the same bits
            import torch

            g.clear()
            assert _call(be, g, ws=ws)[0] == 0
            assert all(torch.equal(_bits(g.out[k]), first[k]) for k in NAMES), what + ": a second call differs"
            g.clear()
            rc2, ws2, use2, _ = _call(be, g, extra=4096)
            assert rc2 == 0 and all(torch.equal(_bits(g.out[k]), first[k]) for k in NAMES), what + ": a larger workspace differs"
            assert np.isnan(ws2[use2:].cpu().numpy()).all()
        # the Backend's call is the C call
        got = be.policy_conv_backward(g.dm, g.di, g.Wd, g.dg)
        import torch

        torch.cuda.synchronize()
        assert all(torch.equal(_bits(got[k]), first[k]) for k in NAMES)


def test_refusals_write_nothing():
    import torch

    from ai_economist_amd import _cabi

    be = _be()
    shape = cref.SHAPES[0]
    g = _Grad(be, shape, 9, seed=5)
    assert _call(be, g)[0] == 0 and not g.untouched()
    for kw, code in ((dict(h=25, w=25), _cabi.E_UNSUPPORTED), (dict(D=9), _cabi.E_UNSUPPORTED), (dict(V=129), _cabi.E_UNSUPPORTED),
                     (dict(C_map=33), _cabi.E_UNSUPPORTED), (dict(emb=None), _cabi.E_INVALID), (dict(map_ld=7 * 121 - 1), _cabi.E_INVALID)):
        g = _Grad(be, shape, 9, seed=5)
        for k, v in kw.items():
            setattr(g.c.net, k, v)
        ws = torch.full((1 << 20,), float("nan"), device=DEV)
        rc = be.lib.aie_policy_conv_backward(be.handle, C.c_int64(9), C.byref(g.c), C.c_void_p(ws.data_ptr()), C.c_int64(ws.numel() * 4),
                                             be._stream())
        torch.cuda.synchronize()
        assert rc == code and g.untouched() and bool(torch.isnan(ws).all()), kw
        assert b"aie_policy_conv_backward" in be.lib.aie_last_error(be.handle)
        assert be.lib.aie_policy_conv_backward_workspace_bytes(be.handle, C.c_int64(9), C.byref(g.c)) == code
        # the forward refuses the same class the same way and writes nothing
        x = torch.full((9, 128), float("nan"), device=DEV)
        g.c.net.x_out, g.c.net.x_ld = x.data_ptr(), 128
        assert be.lib.aie_policy_conv_forward(be.handle, C.c_int64(9), C.byref(g.c.net), be._stream()) == code
        torch.cuda.synchronize()
        assert bool(torch.isnan(x).all())
    g = _Grad(be, shape, 9, seed=5)
    rc, ws, use, need = _call(be, g, short=4)  # a short workspace
    assert rc == _cabi.E_INVALID and g.untouched() and bool(torch.isnan(ws).all())
    g.c.gw2 = None
    assert _call(be, g)[0] == _cabi.E_INVALID and g.untouched()
    with pytest.raises(ValueError):
        be.policy_conv_forward(g.dm, g.di.to(torch.int32), None, g.Wd)  # nothing is converted
    with pytest.raises(ValueError):
        be.policy_conv_forward(g.dm, g.di, None, dict(g.Wd, w1=g.Wd["w1"].t()))
    with pytest.raises(ValueError):
        be.policy_conv_backward(g.dm, g.di, g.Wd, g.dg[:, :100])


CONV_TENSORS = ["conv_" + k for k in NAMES]
MLP_NAMES = bref.NAMES


def _spatial_policy(be, seed=3):
    from ai_economist_amd.rollout import MaskedMLPPolicy

    pol = MaskedMLPPolicy(be, network="library", seed=seed, value_head=True, record_logp=True, spatial=True)
    pol.conv_weights["b1"].copy_(_dev((0.05 * np.random.default_rng(1).standard_normal(16)).astype(f32)))
    pol.bav.fill_(0.25)
    return pol


def _stored_operands(B, seed):
    from test_gpu_ppo_loss import _batches, _env as ppo_env, _stored

    _, be, _, WA, MP = ppo_env("gtb_c2")
    ba, bp, _ = _batches("gtb_c2", B, seed=seed, edges=False)
    return be, _stored(ba, bp)


def _fresh_logp_old(be, pol, crop, dxp, stored):
    x = be.policy_conv_forward(crop[0], crop[1], crop[2], pol.conv_weights)
    la, lp, _, _ = be.policy_mlp_forward(x, dxp, pol.weights_a, pol.weights_p)
    ga, gp, _, _ = be.policy_evaluate(la.view(stored["masks_a"].shape), lp, stored["masks_a"], stored["masks_p"], stored["actions_a"],
                                      stored["actions_p"], entropy=False)
    return dict(stored, logp_old_a=ga.view(stored["logp_old_a"].shape).contiguous(), logp_old_p=gp.view(stored["logp_old_p"].shape).contiguous())


def _crop_batch(be, pol, B, seed):
    shape = (7, 4, 11, 11, 100)
    m, idx = cref.random_crop(B * be.n, shape, seed=seed)
    FA, FP = pol.wa1.shape[0] - pol.NF, pol.wp1.shape[0]
    flat, xp = bref.rows_with_zeros(B * be.n, FA, seed + 1), bref.rows_with_zeros(B, FP, seed + 2)
    return shape, (m, idx, flat, xp), (_dev(m), _dev(idx), _dev(flat)), _dev(xp)


def test_policy_conv_mlp_under_ppo_loss_fills_all_grads(shim, mlp_shim):
    import torch

    from ai_economist_amd import rollout
    from test_policy_mlp_backward_cpu import c_backward as mlp_c_backward

    B = 67  # 268 agent rows: two segments
    be, stored = _stored_operands(B, seed=21)
    pol = _spatial_policy(be)
    assert len(pol.params_a) == 13 and len(pol.params_p) == 8 and pol.NF == 128
    params = list(pol.params_a.items()) + list(pol.params_p.items())
    leaves = {"a": dict(pol.weights_a), "p": dict(pol.weights_p)}
    for who in "ap":  # the value columns: leaves are the [hidden, 1] tensors, as MaskedMLPPolicy.evaluate takes them
        leaves[who]["wv"] = getattr(pol, "w%sv" % who)
    all_leaves = list(pol.conv_weights.values()) + list(leaves["a"].values()) + list(leaves["p"].values())
    assert len(all_leaves) == 21 == len(params)
    for t in all_leaves:
        t.requires_grad_(True)
    shape, (m, idx, flat, xp), crop, dxp = _crop_batch(be, pol, B, seed=61)
    with torch.no_grad():
        stored = _fresh_logp_old(be, pol, crop, dxp, stored)
    la, lp, va, vp = pol.evaluate(crop, dxp)
    assert la.requires_grad and vp.requires_grad
    with torch.no_grad():
        x_cat = be.policy_conv_forward(crop[0], crop[1], crop[2], pol.conv_weights)
        fwd = be.policy_mlp_forward(x_cat, dxp, pol.weights_a, pol.weights_p)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((la, lp, va, vp), fwd))
    la.retain_grad(), lp.retain_grad(), va.retain_grad(), vp.retain_grad()
    loss_a, loss_p, _, _ = rollout.ppo_loss(be, la, lp, va, vp, stored)
    (loss_a + loss_p).backward()
    torch.cuda.synchronize()
    # the direct calls on ppo_loss's own gradients, in the autograd function's order
    det = lambda w: {k: v.detach() for k, v in w.items()}  # noqa: E731
    wa, wp, wc = det(pol.weights_a), det(pol.weights_p), det(pol.conv_weights)
    ga, gp = be.policy_mlp_backward(x_cat, dxp, wa, wp, la.grad.contiguous(), lp.grad.contiguous(), va.grad.contiguous(), vp.grad.contiguous())
    g_x, _ = be.policy_mlp_input_grad(ncols_a=pol.NF)
    gc = be.policy_conv_backward(crop[0], crop[1], wc, g_x)
    torch.cuda.synchronize()
    assert bool(la.grad.ne(0).any()) and bool(g_x.ne(0).any())
    for k in NAMES:
        t = pol.conv_weights[k]
        assert t.grad is not None and torch.equal(_bits(t.grad), _bits(gc[k])), "conv " + k
        assert bool(t.grad.ne(0).any()), "conv " + k
    for who, grads in (("a", ga), ("p", gp)):
        for k in MLP_NAMES:
            t = leaves[who][k]
            assert t.grad is not None and torch.equal(_bits(t.grad), _bits(grads[k])), (who, k)
    # the header's, stage by stage on the device's own intermediates: bit for bit
    Wc = {k: v.detach().cpu().numpy() for k, v in pol.conv_weights.items()}
    gf = g_x.cpu().numpy()
    want = c_backward(shim, m, idx, Wc, gf, shape)
    feat = x_cat.cpu().numpy()[:, : pol.NF]
    assert feat.tobytes() == c_forward(shim, m, idx, Wc, shape).tobytes()
    got21 = {}
    for k in NAMES:
        got = pol.conv_weights[k].grad.cpu().numpy()
        assert got.tobytes() == want[k].tobytes(), "conv g%s is not the header's" % k
        got21[("c", k)] = got
    xs = {"a": x_cat.cpu().numpy(), "p": xp}
    Wm, loss_g = {}, {}
    for who, gl, gv in (("a", la.grad, va.grad), ("p", lp.grad, vp.grad)):
        x = xs[who]
        W = {k: leaves[who][k].detach().cpu().numpy().reshape(-1) if k == "wv" else leaves[who][k].detach().cpu().numpy() for k in MLP_NAMES}
        gln, gvn = gl.cpu().numpy().reshape(x.shape[0], -1), gv.cpu().numpy().reshape(-1)
        wantm = mlp_c_backward(mlp_shim, x, W, gln, gvn)
        for k in MLP_NAMES:
            got = leaves[who][k].grad.cpu().numpy().reshape(wantm[k].shape)
            assert (got == wantm[k]).all(), (who, k)
            got21[(who, k)] = got
        Wm[who], loss_g[who] = W, (gln, gvn)
    # ... and end to end, against nothing of the library's but the loss's gradients: all 21 inside the bound, propagated from the
    # chain lengths through every stage, around torch's float64 pass of the whole network from the crop on
    hold_network(shim, got21, m, idx, flat, xp, Wc, Wm["a"], Wm["p"], loss_g["a"][0], loss_g["a"][1], loss_g["p"][0], loss_g["p"][1],
                 shape, _seg(), who="the device")


def _two_updates(graphed):
    """Two updates -- encoder, MLP, ppo_loss, the three backward calls, Adam.step on all 21 tensors -- from one start."""
    import torch

    from ai_economist_amd import rollout

    B = 40
    be, stored = _stored_operands(B, seed=33)
    pol = _spatial_policy(be)
    before = [t.clone() for t in pol.logits(be.tensors)]
    shape, _, crop, dxp = _crop_batch(be, pol, B, seed=71)
    stored = _fresh_logp_old(be, pol, crop, dxp, stored)
    f = dict(dtype=torch.float32, device=DEV)
    rows, WA, MP = B * be.n, pol.MA, pol.MP
    x_cat = torch.empty((rows, pol.wa1.shape[0]), **f)
    net = (torch.empty((rows, WA), **f), torch.empty((B, MP), **f), torch.empty(rows, **f), torch.empty(B, **f))
    loss = tuple((torch.empty(8, **f), torch.empty_like(lg), torch.empty_like(v)) for lg, v in ((net[0], net[2]), (net[1], net[3])))
    grads = tuple({k: torch.empty_like(v) for k, v in w.items()} for w in (pol.weights_a, pol.weights_p))
    g_x = torch.empty((rows, pol.NF), **f)
    gconv = {k: torch.empty_like(v) for k, v in pol.conv_weights.items()}
    opt = rollout.Adam(be, pol.params_a, pol.params_p, lr=1e-2)
    grads_a = dict(grads[0], **{"conv_" + k: v for k, v in gconv.items()})
    everything = list(pol.params_a.values()) + list(pol.params_p.values())
    start = [t.clone() for t in everything]

    def update():
        be.policy_conv_forward(crop[0], crop[1], crop[2], pol.conv_weights, out=x_cat)
        be.policy_mlp_forward(x_cat, dxp, pol.weights_a, pol.weights_p, out=net)
        be.ppo_loss(net[0], net[1], net[2], net[3], stored, out=loss)
        be.policy_mlp_backward(x_cat, dxp, pol.weights_a, pol.weights_p, loss[0][1], loss[1][1], loss[0][2], loss[1][2], out=grads)
        be.policy_mlp_input_grad(ncols_a=pol.NF, out=(g_x, None))
        be.policy_conv_backward(crop[0], crop[1], pol.conv_weights, g_x, out=gconv)
        opt.step((grads_a, grads[1]))

    def restart():
        for t, s in zip(everything, start):
            t.copy_(s)
        for G in opt.groups:
            G["state"].zero_()
            for t in G["m"] + G["v"]:
                t.zero_()

    if graphed:
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            update()  # the warm-up: the workspaces exist
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        restart()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            update()
        restart()
        for _ in range(2):
            graph.replay()
    else:
        for _ in range(2):
            update()
    torch.cuda.synchronize()
    after = [t.clone() for t in pol.logits(be.tensors)]
    torch.cuda.synchronize()
    bits = {k: _bits(v).clone() for k, v in list(pol.params_a.items()) + [("p_" + k, v) for k, v in pol.params_p.items()]}
    moved = all(not torch.equal(t, s) for t, s in zip(everything, start))
    return bits, before, after, moved


def test_two_captured_updates_equal_two_eager_ones():
    import torch

    eager, before, after, moved = _two_updates(False)
    assert moved, "an update left a weight tensor where it was"
    assert len(eager) == 21
    assert not torch.equal(before[0], after[0]) and all(bool(torch.isfinite(t).all()) for t in after)  # logits() sees the new weights
    replayed, before_g, after_g, _ = _two_updates(True)
    for k in eager:
        assert torch.equal(eager[k], replayed[k]), "replayed != eager: " + k
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before + after, before_g + after_g))


def _spatial_rollout(graphed, N):
    import torch

    from ai_economist_amd.rollout import GraphedStep, Trajectory

    WARM = 3
    env = make_env(dict(_cfg("gtb_c2"), episode_length=7), n_envs=5, device=DEV)
    env.seed(5)
    env.reset()
    be = env.backend
    pol = _spatial_policy(be)
    traj = Trajectory(env, N, observations=("obs_a_world-map", "obs_a_world-idx_map", "obs_a_flat", "obs_p_flat"))
    a, p = be._action_buffers(0)
    if graphed:
        gs = GraphedStep(env, pol, auto_reset=True, warmup=WARM, trajectory=traj)
        traj.rewind()
        gs.replay(N)
    else:
        be.set_auto_reset(True)
        for i in range(WARM + N):
            if i == WARM:
                traj.rewind()
            pol(be.tensors, a, p)
            traj.store(a, p, pol.logp_a, pol.logp_p, pol.value_a, pol.value_p)
            be.step(a, p)
    torch.cuda.synchronize()
    assert int(be.tensors["error_flags"].abs().sum()) == 0
    fl = traj.flat()
    out = {k: fl[k].contiguous().view(torch.int32).cpu() for k in ("actions_a", "actions_p", "logp_a", "logp_p", "values_a", "values_p")}
    return out, pol, traj, be


def test_spatial_policy_replays_and_reads_stored_crops(shim):
    import torch

    from ai_economist_amd.rollout import MaskedMLPPolicy

    N = 12
    (g, pol, traj, be), (e, _, _, _) = _spatial_rollout(True, N), _spatial_rollout(False, N)
    for k in g:
        assert torch.equal(g[k], e[k]), "replayed != eager: " + k
    assert bool(g["actions_a"].ne(0).any()) and bool(g["values_a"].ne(0).all())
    # the stored crops are legal operands where they lie: the policy's stored values are the encoder's and the MLP's on them
    obs = traj.flat()["obs"]
    la, lp, va, vp = pol.evaluate((obs["obs_a_world-map"], obs["obs_a_world-idx_map"], obs["obs_a_flat"]), obs["obs_p_flat"])
    torch.cuda.synchronize()
    assert torch.equal(va.detach().reshape(-1).view(torch.int32), g["values_a"].reshape(-1).to(DEV))
    assert torch.equal(vp.detach().reshape(-1).view(torch.int32), g["values_p"].reshape(-1).to(DEV))
    # ... and the header's on the downloaded tensors
    Wc = {k: v.cpu().numpy() for k, v in pol.conv_weights.items()}
    m = obs["obs_a_world-map"].cpu().numpy().reshape(-1, 7, 11, 11)
    idx = obs["obs_a_world-idx_map"].cpu().numpy().reshape(-1, 2, 11, 11)
    x = be.policy_conv_forward(obs["obs_a_world-map"], obs["obs_a_world-idx_map"], obs["obs_a_flat"], pol.conv_weights)
    assert x.cpu().numpy()[:, :128].tobytes() == c_forward(shim, m, idx, Wc, (7, 4, 11, 11, 100)).tobytes()
    # the next logits() sees an in-place update
    first = pol.logits(be.tensors)[0].clone()
    pol.conv_weights["w2"].mul_(0.5)
    assert not torch.equal(pol.logits(be.tensors)[0], first)
    # spatial=False: the weights a seed gave before, and logits() is policy_mlp_forward on them
    flat_pol = MaskedMLPPolicy(be, network="library", seed=3, value_head=True)
    again = MaskedMLPPolicy(be, network="library", seed=3, value_head=True, spatial=True)
    FA = flat_pol.wa1.shape[0]
    assert torch.equal(again.wa1[-FA:], flat_pol.wa1) and again.wa1.shape[0] == 128 + FA
    for k in ("wa2", "wa3", "wp1", "wp2", "wp3", "wav", "wpv"):
        assert torch.equal(getattr(again, k), getattr(flat_pol, k)), k
    lg = [t.clone() for t in flat_pol.logits(be.tensors)]
    direct = be.policy_mlp_forward(be.tensors["obs_a_flat"], be.tensors["obs_p_flat"], flat_pol.weights_a, flat_pol.weights_p)
    torch.cuda.synchronize()
    assert torch.equal(_bits(lg[0]), _bits(direct[0])) and torch.equal(_bits(lg[1]), _bits(direct[1]))
    assert not hasattr(flat_pol, "x_cat") and not flat_pol.spatial
