"""The convolutional encoder and the MLP's input gradient, CPU side (csrc/aie_trainer_math.h: aie_conv_row_forward,
aie_conv_backward_host, aie_mlp_input_grad_entry -- the helpers the kernels call output by output; csrc/aie_trainer_plan.h:
the plans):

  * values: the header's helpers, compiled here with the host C compiler, == the numpy transcription (tests/policy_conv_ref.py)
    bit for bit -- forward, input gradient and all five gradients -- on the shipped shape at 1, 3, SEG - 1, SEG, SEG + 1 rows
    and on the edge shapes at 1, 3 and SEG + 1, with indices 0 and V - 1, an all-zero crop, dead filters, and one case with
    out-of-range indices on both sides;
  * accuracy: every float32 result within the derived bound around the float64 pass (policy_conv_ref.forward_f64 /
    backward_f64: derived from the chain lengths, not measured);
  * conventions: the float64 pass equals torch's embedding / conv2d(stride 2) / flatten in float64 on the CPU, and autograd
    for the gradients -- the layouts are Keras' (HWIO kernels, channels-last flatten, map planes ahead of the embeddings),
    not merely self-consistent;
  * the plans' refusals: every limit, NULL operands, strides, a short workspace, misaligned pointers -- without a GPU.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import policy_conv_ref as cref
import policy_mlp_ref as ref
from helpers import ROOT

CSRC = os.path.join(ROOT, "ai-economist_amd", "csrc")
f32, f64 = np.float32, np.float64

SHIM = r"""
#include <stdlib.h>
#include "aie_trainer_plan.h"
int shim_seg(void) { return AIE_MLP_BWD_SEG; }
int shim_f1(void) { return AIE_CONV_F1; }
int shim_f2(void) { return AIE_CONV_F2; }
int shim_igrad_tile(void) { return AIE_IGRAD_TILE; }
void shim_conv_forward(int C_map, int D, int h, int w, int V, long rows, const float* map, long map_ld, const int16_t* idx, long idx_ld,
                       const float* emb, const float* w1, const float* b1, const float* w2, const float* b2, float* feat) {
  const aie_conv_shape S = aie_conv_shape_of(C_map, D, h, w, V);
  float* X = (float*)malloc(sizeof(float) * (size_t)(S.hw * S.C + S.P1 * AIE_CONV_F1));
  for (long r = 0; r < rows; ++r)
    aie_conv_row_forward(&S, map + r * map_ld, idx + r * idx_ld, emb, w1, b1, w2, b2, X, X + S.hw * S.C, feat + r * S.NF);
  free(X);
}
void shim_conv_backward(int C_map, int D, int h, int w, int V, long rows, const float* map, long map_ld, const int16_t* idx,
                        long idx_ld, const float* emb, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* g_feat, long g_ld, float* gemb, float* gw1, float* gb1, float* gw2, float* gb2) {
  const aie_conv_shape S = aie_conv_shape_of(C_map, D, h, w, V);
  const size_t per = (size_t)(S.hw * S.C + 2 * S.P1 * AIE_CONV_F1 + 2 * S.NF + 2 * S.hw * S.D);
  float* scratch = (float*)malloc(sizeof(float) * ((size_t)rows * per + (size_t)(S.V * S.D)));
  aie_conv_backward_host(&S, rows, map, map_ld, idx, idx_ld, emb, w1, b1, w2, b2, g_feat, g_ld, scratch, gemb, gw1, gb1, gw2, gb2);
  free(scratch);
}
void shim_input_grad(const float* dz1, const float* w1, long rows, int H, int ncols, float* g_x, long ld) {
  for (long r = 0; r < rows; ++r)
    for (int j = 0; j < ncols; ++j) g_x[r * ld + j] = aie_mlp_input_grad_entry(dz1 + r * H, w1, H, j);
}
int shim_plan_forward(long long rows, const aie_conv_class* k, char* err, size_t n, aie_conv_fwd_plan* p) {
  return aie_plan_conv_forward(rows, k, err, n, p);
}
int shim_plan_backward(long long rows, const aie_conv_grad_class* q, int query, void* ws, long long bytes, char* err, size_t n,
                       aie_conv_bwd_plan* p) {
  return aie_plan_conv_backward(rows, q, query, ws, bytes, err, n, p);
}
int shim_plan_input_grad(int n_agents, long long B, const aie_mlp_grad_class* a, const aie_mlp_grad_class* q, void* ws, long long bytes,
                         float* gxa, long long lda, int nca, float* gxp, long long ldp, int ncp, char* err, size_t n,
                         aie_mlp_igrad_plan* p) {
  aie_params* P = (aie_params*)calloc(1, sizeof(aie_params));
  P->n = n_agents;
  const int rc = aie_plan_mlp_input_grad(P, B, a, q, ws, bytes, gxa, lda, nca, gxp, ldp, ncp, err, n, p);
  free(P);
  return rc;
}
size_t shim_sizeof_fwd_plan(void) { return sizeof(aie_conv_fwd_plan); }
size_t shim_sizeof_bwd_plan(void) { return sizeof(aie_conv_bwd_plan); }
size_t shim_sizeof_igrad_plan(void) { return sizeof(aie_mlp_igrad_plan); }
/* what the tests read back of a plan */
void shim_fwd_geometry(const aie_conv_fwd_plan* p, long long* o) {
  o[0] = p->grid, o[1] = p->block, o[2] = (long long)p->lds, o[3] = p->A.tr, o[4] = p->A.lds_row, o[5] = p->A.S.NF;
}
void shim_bwd_geometry(const aie_conv_bwd_plan* p, long long* o) {
  o[0] = p->need, o[1] = p->grid_rows, o[2] = p->grid_seg, o[3] = p->grid_reduce, o[4] = (long long)p->lds_rows, o[5] = (long long)p->lds_seg;
  o[6] = p->A.nseg, o[7] = p->A.Pn, o[8] = p->A.partial - p->A.a1;
}
void shim_igrad_geometry(const aie_mlp_igrad_plan* p, long long* o) {
  o[0] = p->grid, o[1] = (long long)p->lds, o[2] = p->A.agents.blocks, o[3] = p->A.planner.blocks, o[4] = p->need;
  o[5] = (long long)(uintptr_t)p->A.agents.dz1, o[6] = (long long)(uintptr_t)p->A.planner.dz1;
}
"""


def build_conv_shim(d):
    src, so = os.path.join(d, "shim_conv.c"), os.path.join(d, "shim_conv.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), src, "-o", so, "-lm"], check=True)
    lib = ctypes.CDLL(so)
    for k in ("shim_seg", "shim_f1", "shim_f2", "shim_igrad_tile"):
        getattr(lib, k).restype = ctypes.c_int
    for k in ("shim_sizeof_fwd_plan", "shim_sizeof_bwd_plan", "shim_sizeof_igrad_plan"):
        getattr(lib, k).restype = ctypes.c_size_t
    vp, ll, ci = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    lib.shim_conv_forward.argtypes = [ci] * 5 + [ctypes.c_long, vp, ctypes.c_long, vp, ctypes.c_long] + [vp] * 6
    lib.shim_conv_backward.argtypes = [ci] * 5 + [ctypes.c_long, vp, ctypes.c_long, vp, ctypes.c_long] + [vp] * 6 + [ctypes.c_long] + [vp] * 5
    lib.shim_input_grad.argtypes = [vp, vp, ctypes.c_long, ci, ci, vp, ctypes.c_long]
    lib.shim_plan_forward.argtypes = [ll, vp, vp, ctypes.c_size_t, vp]
    lib.shim_plan_backward.argtypes = [ll, vp, ci, vp, ll, vp, ctypes.c_size_t, vp]
    lib.shim_plan_input_grad.argtypes = [ci, ll, vp, vp, vp, ll, vp, ll, ci, vp, ll, ci, vp, ctypes.c_size_t, vp]
    for k in ("shim_fwd_geometry", "shim_bwd_geometry", "shim_igrad_geometry"):
        getattr(lib, k).argtypes = [vp, vp]
    return lib


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as d:
        yield build_conv_shim(d)


def _p(a):
    return a.ctypes.data if a is not None else None


def c_forward(lib, m, idx, W, shape):
    m, idx = np.ascontiguousarray(m, f32), np.ascontiguousarray(idx, np.int16)
    d = cref.dims(shape)
    rows = m.shape[0]
    feat = np.full((rows, d["NF"]), np.nan, f32)
    lib.shim_conv_forward(*shape, rows, _p(m), m[0].size, _p(idx), idx[0].size, *[_p(np.ascontiguousarray(W[k], f32)) for k in cref.NAMES],
                          _p(feat))
    return feat


def c_backward(lib, m, idx, W, g_feat, shape):
    m, idx, g_feat = np.ascontiguousarray(m, f32), np.ascontiguousarray(idx, np.int16), np.ascontiguousarray(g_feat, f32)
    Wc = {k: np.ascontiguousarray(W[k], f32) for k in cref.NAMES}
    G = {k: np.full(Wc[k].shape, np.nan, f32) for k in cref.NAMES}
    lib.shim_conv_backward(*shape, m.shape[0], _p(m), m[0].size, _p(idx), idx[0].size, *[_p(Wc[k]) for k in cref.NAMES],
                           _p(g_feat), g_feat.shape[1], *[_p(G[k]) for k in cref.NAMES])
    return G


def random_g_feat(rows, NF, seed):
    g = np.random.default_rng(seed)
    gf = (g.standard_normal((rows, NF)) / 64).astype(f32)
    gf[g.random(gf.shape) < 0.1] = 0
    return gf


def cases(SEG):
    out = [(s, r, False) for s in cref.SHAPES for r in (1, 3, SEG - 1, SEG, SEG + 1)]
    out += [(s, r, False) for s in cref.EDGE_SHAPES for r in (1, 3, SEG + 1)]
    return out + [(cref.SHAPES[0], 5, True)]  # out-of-range indices on both sides


def test_the_constants_are_the_bindings(shim):
    from ai_economist_amd import _cabi

    assert shim.shim_seg() == _cabi.MLP_BWD_SEG
    assert (shim.shim_f1(), shim.shim_f2()) == (_cabi.CONV_F1, _cabi.CONV_F2) == (cref.F1, cref.F2)
    for s in cref.SHAPES + cref.EDGE_SHAPES:
        d = cref.dims(s)
        assert d["oh2"] >= 1 and d["ow2"] >= 1
    assert cref.dims(cref.SHAPES[0])["NF"] == 128 and cref.dims(cref.EDGE_SHAPES[0])["NF"] == 32
    assert all((9 * cref.dims(s)["C"]) % 4 for s in [cref.EDGE_SHAPES[4]])  # K = 27


@pytest.mark.parametrize("shape", cref.SHAPES + cref.EDGE_SHAPES, ids=lambda s: "%dx%d_%dx%d_V%d" % s)
def test_header_equals_the_transcription(shim, shape):
    SEG = shim.shim_seg()
    d = cref.dims(shape)
    for i, (s, rows, oor) in enumerate(c for c in cases(SEG) if c[0] == shape):
        W = cref.random_weights(shape, seed=31 * d["C"] + i, dead=True)
        m, idx = cref.random_crop(rows, shape, seed=17 * d["h"] + i, out_of_range=oor)
        clamped = cref.clamp(idx, d["V"])
        assert clamped.min() == 0 and clamped.max() == d["V"] - 1
        if oor:
            assert idx.min() < 0 and idx.max() >= d["V"]
        gf = random_g_feat(rows, d["NF"], seed=5 + i)
        want_f, _, a1 = cref.forward(m, idx, W, shape, full=True)
        got_f = c_forward(shim, m, idx, W, shape)
        assert np.isfinite(want_f).all() and not np.isnan(got_f).any()
        assert got_f.tobytes() == want_f.tobytes(), "%s, %d rows: %d features differ" % (shape, rows, (got_f != want_f).sum())
        assert (want_f == 0).any() and (a1 == 0).any() and (want_f > 0).any()  # ReLU's zero side, and dead filters
        if rows > 1:
            assert (m[1] == 0).all()
        want = cref.backward(m, idx, W, gf, shape, SEG)
        got = c_backward(shim, m, idx, W, gf, shape)
        for k in cref.NAMES:
            assert got[k].shape == want[k].shape and not np.isnan(got[k]).any()
            assert (got[k] == want[k]).all(), "%s, %d rows: %d entries of g%s differ" % (shape, rows, (got[k] != want[k]).sum(), k)
            assert got[k].tobytes() == want[k].tobytes(), (shape, rows, k)
        assert np.abs(want["w1"]).max() > 0 and np.abs(want["emb"]).max() > 0


@pytest.mark.parametrize("H, F", [(128, 264), (16, 1), (256, 33), (48, 300)])
def test_input_grad_equals_the_transcription(shim, H, F):
    g = np.random.default_rng(H + F)
    SEG = shim.shim_seg()
    for rows in (1, 3, SEG - 1, SEG, SEG + 1):
        dz1 = (g.standard_normal((rows, H)) / 32).astype(f32)
        dz1[g.random(dz1.shape) < 0.4] = 0  # ReLU's zero side
        w1 = (g.standard_normal((F, H)) / np.sqrt(F)).astype(f32)
        for ncols in sorted({1, min(128, F), F}):
            got = np.full((rows, ncols + 3), np.nan, f32)
            shim.shim_input_grad(_p(dz1), _p(w1), rows, H, ncols, _p(got), ncols + 3)
            want = cref.input_grad(dz1, w1, ncols)
            assert got[:, :ncols].tobytes() == want.tobytes() and np.isnan(got[:, ncols:]).all()
            g64, bound = cref.input_grad_f64(dz1, w1, ncols)
            assert (np.abs(want.astype(f64) - g64) <= bound).all()


def _torch_pass(m, idx, W, gf, shape, dtype):
    """torch's formulation: embedding, cat (map first), conv2d(stride 2) with the HWIO kernels permuted to OIHW, channels-last
    flatten; the gradients of (features * gf).sum() by autograd."""
    import torch
    import torch.nn.functional as Fn

    d = cref.dims(shape)
    t = {k: torch.tensor(np.asarray(W[k]), dtype=dtype, requires_grad=True) for k in cref.NAMES}
    e = Fn.embedding(torch.tensor(cref.clamp(idx, d["V"])), t["emb"])  # [rows, 2, h, w, D]
    e = e.permute(0, 1, 4, 2, 3).reshape(idx.shape[0], 2 * d["D"], d["h"], d["w"])
    x = torch.cat([torch.tensor(np.asarray(m), dtype=dtype), e], dim=1)
    k1 = t["w1"].reshape(3, 3, d["C"], cref.F1).permute(3, 2, 0, 1)
    k2 = t["w2"].reshape(3, 3, cref.F1, cref.F2).permute(3, 2, 0, 1)
    a1 = torch.relu(Fn.conv2d(x, k1, t["b1"], stride=2))
    a2 = torch.relu(Fn.conv2d(a1, k2, t["b2"], stride=2))
    feat = a2.permute(0, 2, 3, 1).reshape(idx.shape[0], -1)
    (feat * torch.tensor(np.asarray(gf), dtype=dtype)).sum().backward()
    return feat.detach().numpy(), {k: t[k].grad.numpy() for k in cref.NAMES}, a1.detach().permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("shape", cref.SHAPES + cref.EDGE_SHAPES, ids=lambda s: "%dx%d_%dx%d_V%d" % s)
def test_accuracy_and_conventions(shim, shape):
    import torch

    SEG = shim.shim_seg()
    d = cref.dims(shape)
    for rows, oor in ((9, True), (SEG + 1, False)):
        W = cref.random_weights(shape, seed=3 + d["C"], dead=False)
        m, idx = cref.random_crop(rows, shape, seed=5 + d["w"], out_of_range=oor)
        gf = random_g_feat(rows, d["NF"], seed=9)
        # the conventions: the float64 pass with its own masks against torch in float64
        f64_own, _, aux = cref.forward_f64(m, idx, W, shape)
        t_feat, t_grads, t_a1 = _torch_pass(m, idx, W, gf, shape, torch.float64)
        assert np.abs(t_feat - f64_own).max() <= 1e-12 * max(1.0, np.abs(f64_own).max())
        own = (aux["m1"].reshape(rows, d["oh1"], d["ow1"], cref.F1), aux["m2"].reshape(rows, d["NF"]))
        assert ((t_a1 > 0) == own[0]).all()
        G_own, E_own = cref.backward_f64(m, idx, W, gf, shape, SEG, own)
        for k in cref.NAMES:
            assert (np.abs(t_grads[k].reshape(G_own[k].shape) - G_own[k]) <= E_own[k] * 2.0 ** -28 + 1e-300).all(), "autograd differs in g" + k
        # the accuracy: the header's float32 within the derived bound around the float64 pass under the float32 masks
        got_f = c_forward(shim, m, idx, W, shape)
        f64_feat, bound, _ = cref.forward_f64(m, idx, W, shape)
        assert (np.abs(got_f.astype(f64) - f64_feat) <= bound).all(), "the features leave the bound"
        _, _, a1 = cref.forward(m, idx, W, shape, full=True)
        masks = (a1 > 0, got_f > 0)
        G64, E = cref.backward_f64(m, idx, W, gf, shape, SEG, masks)
        got = c_backward(shim, m, idx, W, gf, shape)
        worst = 0.0
        for k in cref.NAMES:
            err = np.abs(got[k].astype(f64) - G64[k])
            assert (err <= E[k]).all(), "g%s leaves the bound at %d rows" % (k, rows)
            worst = max(worst, float((err / np.maximum(E[k], 1e-300)).max()))
        print("%s, %d rows: max error / bound %.3f" % (shape, rows, worst))


# ---- the whole network: crop -> encoder -> [features, flat] -> MLP, and back; the GPU test holds the device to the same ----
def torch_network_f64(m, idx, flat, xp, Wc, Wa, Wp, gl_a, gv_a, gl_p, gv_p, shape, masks_c, masks_a, masks_p):
    """torch's float64 formulation of the whole network (embedding, cat, two conv2d(stride 2), flatten, cat, the MLPs) with the
    given ReLU decisions imposed (pre-activation times a 0 / 1 constant, as test_policy_mlp_backward_cpu does), and autograd's
    gradients of sum(logits * g_logits) + sum(values * g_values) over both classes -> {(class, name): gradient}."""
    import torch
    import torch.nn.functional as Fn

    d, dt = cref.dims(shape), torch.float64
    rows = m.shape[0]
    leaf = lambda W: {k: torch.tensor(np.asarray(v), dtype=dt, requires_grad=True) for k, v in W.items()}  # noqa: E731
    con = lambda a: torch.tensor(np.asarray(a, f64))  # noqa: E731
    tc, ta, tp = leaf(Wc), leaf(Wa), leaf(Wp)
    e = Fn.embedding(torch.tensor(cref.clamp(idx, d["V"])), tc["emb"]).permute(0, 1, 4, 2, 3).reshape(rows, 2 * d["D"], d["h"], d["w"])
    x = torch.cat([con(m), e], dim=1)
    k1 = tc["w1"].reshape(3, 3, d["C"], cref.F1).permute(3, 2, 0, 1)
    k2 = tc["w2"].reshape(3, 3, cref.F1, cref.F2).permute(3, 2, 0, 1)
    m1 = con(masks_c[0].reshape(rows, d["oh1"], d["ow1"], cref.F1)).permute(0, 3, 1, 2)
    m2 = con(masks_c[1].reshape(rows, d["oh2"], d["ow2"], cref.F2)).permute(0, 3, 1, 2)
    a1 = Fn.conv2d(x, k1, tc["b1"], stride=2) * m1
    a2 = Fn.conv2d(a1, k2, tc["b2"], stride=2) * m2
    xa = torch.cat([a2.permute(0, 2, 3, 1).reshape(rows, -1), con(flat)], dim=1)
    total = 0
    for xin, t, masks, gl, gv in ((xa, ta, masks_a, gl_a, gv_a), (con(xp), tp, masks_p, gl_p, gv_p)):
        h1 = (xin @ t["w1"] + t["b1"]) * con(masks[0])
        h2 = (h1 @ t["w2"] + t["b2"]) * con(masks[1])
        lg, v = h2 @ t["w3"] + t["b3"], h2 @ t["wv"].reshape(-1) + t["bv"]
        total = total + (lg * con(gl).reshape(lg.shape)).sum() + (v * con(gv).reshape(-1)).sum()
    total.backward()
    out = {("c", k): t_.grad.numpy() for k, t_ in tc.items()}
    out.update({("a", k): t_.grad.numpy() for k, t_ in ta.items()})
    out.update({("p", k): t_.grad.numpy() for k, t_ in tp.items()})
    return out


def contract_masks(shim, m, idx, flat, xp, Wc, Wa, Wp, shape):
    """The float32 contract's forward on the CPU -> (x_a = [features, flat], the encoder's and the two MLPs' ReLU decisions)."""
    import policy_mlp_bwd_ref as bref

    feat = c_forward(shim, m, idx, Wc, shape)
    _, _, a1 = cref.forward(m, idx, Wc, shape, full=True)
    xa = np.concatenate([feat, np.asarray(flat, f32)], 1)
    ha, hp = bref.hidden(xa, Wa), bref.hidden(np.asarray(xp, f32), Wp)
    return xa, (a1 > 0, feat > 0), (ha[0] > 0, ha[1] > 0), (hp[0] > 0, hp[1] > 0)


def hold_network(shim, grads, m, idx, flat, xp, Wc, Wa, Wp, gl_a, gv_a, gl_p, gv_p, shape, seg, who="the header"):
    """grads {(class, name): float32 gradient} of all 21 tensors lie inside the bound, propagated from the chain lengths through
    every stage (policy_conv_ref.network_f64), around torch's float64 pass of the whole network."""
    _, mc, ma, mp = contract_masks(shim, m, idx, flat, xp, Wc, Wa, Wp, shape)
    G, E = cref.network_f64(m, idx, flat, xp, Wc, Wa, Wp, gl_a, gv_a, gl_p, gv_p, shape, seg, mc, ma, mp)
    T = torch_network_f64(m, idx, flat, xp, Wc, Wa, Wp, gl_a, gv_a, gl_p, gv_p, shape, mc, ma, mp)
    assert len(G) == len(T) == 21 and set(grads) == set(G)
    worst = 0.0
    for key in sorted(G):
        t = T[key].reshape(G[key].shape)
        # two float64 evaluations of one formula: 2^-20 of the float32 bound is generous
        assert (np.abs(t - G[key]) <= E[key] * 2.0 ** -20 + 1e-300).all(), "torch's float64 pass differs in %s" % (key,)
        err = np.abs(np.asarray(grads[key], f64).reshape(t.shape) - t)
        assert (err <= E[key]).all(), "%s: the gradient of %s leaves the derived bound around torch's float64 pass" % (who, key)
        assert np.abs(t).max() > 0, key
        worst = max(worst, float((err / np.maximum(E[key], 1e-300)).max()))
    print("%s: all 21 gradients inside the bound around torch's float64 pass, max error / bound %.4f" % (who, worst))
    return worst


def test_whole_network_gradients_within_the_bound_of_the_torch_pass(shim):
    """The contract's own float32 chain on the CPU -- the header's encoder, the transcribed MLP backward and input gradient, the
    header's encoder backward on that input gradient -- against torch's float64 pass of the whole network."""
    import policy_mlp_bwd_ref as bref

    shape, SEG = cref.SHAPES[0], shim.shim_seg()
    d = cref.dims(shape)
    rows, n, FA, H = SEG + 12, 4, 136, 128
    B = rows // n
    Wc = cref.random_weights(shape, seed=2, dead=False)
    Wa = ref.random_weights(d["NF"] + FA, H, 50, seed=3, value=True, dead=False)
    Wp = ref.random_weights(86, H, 154, seed=4, value=True, dead=False)
    m, idx = cref.random_crop(rows, shape, seed=5)
    flat, xp = bref.rows_with_zeros(rows, FA, 6), bref.rows_with_zeros(B, 86, 7)
    gl_a, gv_a = bref.random_grads(rows, 50, seed=8)
    gl_p, gv_p = bref.random_grads(B, 154, seed=9)
    xa, mc, ma, mp = contract_masks(shim, m, idx, flat, xp, Wc, Wa, Wp, shape)
    grads = {("a", k): v for k, v in bref.backward(xa, Wa, gl_a, gv_a, SEG).items()}
    grads.update({("p", k): v for k, v in bref.backward(xp, Wp, gl_p, gv_p, SEG).items()})
    # dz1 of the agents' class in the contract's chains, then the input gradient and the encoder's backward on it
    with np.errstate(all="ignore"):
        dh2 = ref.fma32(gv_a[:, None], np.asarray(Wa["wv"], f32)[None, :], ref.chain(np.zeros(H, f32), gl_a, Wa["w3"].T))
        dz2 = np.where(ma[1], dh2, f32(0)).astype(f32)
        dz1 = np.where(ma[0], ref.chain(np.zeros(H, f32), dz2, Wa["w2"].T), f32(0)).astype(f32)
    g_x = cref.input_grad(dz1, Wa["w1"], d["NF"])
    grads.update({("c", k): v for k, v in c_backward(shim, m, idx, Wc, g_x, shape).items()})
    hold_network(shim, grads, m, idx, flat, xp, Wc, Wa, Wp, gl_a, gv_a, gl_p, gv_p, shape, SEG)


# ---- the plans ----
def _plans(shim):
    from ai_economist_amd import _cabi

    return _cabi, ctypes.create_string_buffer(512)


def conv_class(_cabi, shape=(7, 4, 11, 11, 100), F_flat=136, **kw):
    d = cref.dims(shape)
    k = _cabi.AieConvClass(map=0x10000, map_ld=shape[0] * d["h"] * d["w"], idx=0x20000, idx_ld=2 * d["h"] * d["w"], emb=0x30000,
                           w1=0x40000, b1=0x50000, w2=0x60000, b2=0x70000, flat=0x80000 if F_flat else None, flat_ld=F_flat,
                           x_out=0x90000, x_ld=d["NF"] + F_flat, C_map=shape[0], D=shape[1], h=shape[2], w=shape[3], V=shape[4],
                           F_flat=F_flat)
    for key, v in kw.items():
        setattr(k, key, v)
    return k


def grad_class(_cabi, shape=(7, 4, 11, 11, 100), **kw):
    q = _cabi.AieConvGradClass(net=conv_class(_cabi, shape), g_feat=0xa0000, g_ld=cref.dims(shape)["NF"], gemb=0xb0000, gw1=0xc0000,
                               gb1=0xd0000, gw2=0xe0000, gb2=0xf0000)
    for key, v in kw.items():
        if key.startswith("net_"):
            setattr(q.net, key[4:], v)
        else:
            setattr(q, key, v)
    return q


def fwd(shim, rows, k):
    _cabi, err = _plans(shim)
    plan = ctypes.create_string_buffer(shim.shim_sizeof_fwd_plan())
    rc = shim.shim_plan_forward(rows, ctypes.addressof(k) if k is not None else None, ctypes.addressof(err), 512, ctypes.addressof(plan))
    o = (ctypes.c_longlong * 8)()
    shim.shim_fwd_geometry(ctypes.addressof(plan), ctypes.addressof(o))
    return rc, err.value.decode(), list(o)


def bwd(shim, rows, q, query=0, ws=0x100000, nbytes=1 << 40):
    _cabi, err = _plans(shim)
    plan = ctypes.create_string_buffer(shim.shim_sizeof_bwd_plan())
    rc = shim.shim_plan_backward(rows, ctypes.addressof(q) if q is not None else None, query, ws, nbytes, ctypes.addressof(err), 512,
                                 ctypes.addressof(plan))
    o = (ctypes.c_longlong * 12)()
    shim.shim_bwd_geometry(ctypes.addressof(plan), ctypes.addressof(o))
    return rc, err.value.decode(), list(o)


@pytest.mark.parametrize("shape", cref.SHAPES + cref.EDGE_SHAPES, ids=lambda s: "%dx%d_%dx%d_V%d" % s)
def test_plans_accept_the_supported_shapes(shim, shape):
    _cabi, _ = _plans(shim)
    d = cref.dims(shape)
    SEG = shim.shim_seg()
    for rows in (1, 17, 2 * SEG + 17):
        rc, err, o = fwd(shim, rows, conv_class(_cabi, shape))
        assert rc == 0, err
        grid, block, lds, tr, lds_row, NF = o[:6]
        assert NF == d["NF"] and block == 256 and tr in (1, 2, 4, 8, 16) and grid == -(-rows // tr)
        assert lds_row == d["h"] * d["w"] * d["C"] + d["P1"] * cref.F1 and lds == 4 * tr * lds_row <= 65536
        assert tr == 16 or 4 * 2 * tr * lds_row > 65536  # as many rows as the budget holds
        rc, err, o = bwd(shim, rows, grad_class(_cabi, shape))
        assert rc == 0, err
        need, grid_rows, grid_seg, grid_reduce, lds_rows, lds_seg, nseg, Pn, carve = o[:9]
        n_w = (9 * d["C"] + 1) * cref.F1 + (9 * cref.F1 + 1) * cref.F2
        assert nseg == -(-rows // SEG) and Pn == -(-(n_w + d["V"] * d["D"]) // 4) * 4
        per_row = 2 * d["P1"] * cref.F1 + d["NF"] + 2 * d["h"] * d["w"] * d["D"]
        assert carve == rows * per_row and need == -(-(rows * per_row + nseg * Pn) // 64) * 64 * 4
        assert grid_seg == nseg * (-(-n_w // 256) + 1) and grid_reduce == -(-Pn // 256)
        assert lds_rows <= 65536 and lds_seg == 16 * d["V"] * d["D"] * 4 <= 65536
        assert bwd(shim, rows, grad_class(_cabi, shape), query=1, ws=None, nbytes=0)[0] == 0
        assert bwd(shim, rows, grad_class(_cabi, shape), nbytes=need)[0] == 0


def test_plan_refusals(shim):
    _cabi, _ = _plans(shim)
    INV, UNS = _cabi.E_INVALID, _cabi.E_UNSUPPORTED
    for kw, code, word in ((dict(C_map=0), UNS, "1 .. 32"), (dict(C_map=33, map_ld=33 * 121), UNS, "1 .. 32"),
                           (dict(D=0), UNS, "1 .. 8"), (dict(D=9), UNS, "1 .. 8"),
                           (dict(h=6), UNS, "7 .. 15"), (dict(w=6), UNS, "7 .. 15"), (dict(h=16), UNS, "7 .. 15"),
                           (dict(h=25, w=25, map_ld=7 * 625, idx_ld=1250), UNS, "7 .. 15"),  # full observability's crop
                           (dict(V=0), UNS, "1 .. 128"), (dict(V=129), UNS, "1 .. 128"),
                           (dict(map=None), INV, "NULL"), (dict(idx=None), INV, "NULL"), (dict(emb=None), INV, "NULL"),
                           (dict(w1=None), INV, "NULL"), (dict(b1=None), INV, "NULL"), (dict(w2=None), INV, "NULL"),
                           (dict(b2=None), INV, "NULL"),
                           (dict(map_ld=7 * 121 - 1), INV, "map_ld"), (dict(idx_ld=241), INV, "idx_ld"),
                           (dict(map=0x10002), INV, "aligned"), (dict(idx=0x20001), INV, "aligned"), (dict(w2=0x60001), INV, "aligned")):
        rc, err, _ = fwd(shim, 8, conv_class(_cabi, **kw))
        assert rc == code and word in err and "aie_policy_conv_forward" in err, (kw, rc, err)
        rc, err, _ = bwd(shim, 8, grad_class(_cabi, **{"net_" + k: v for k, v in kw.items()}))
        assert rc == code and word in err and "aie_policy_conv_backward" in err, (kw, rc, err)
    for kw in (dict(x_out=None), dict(x_out=0x90002), dict(x_ld=128 + 135), dict(F_flat=-1), dict(F_flat=1025, x_ld=4096),
               dict(flat=None), dict(flat=0x80001), dict(flat_ld=135)):
        rc, err, _ = fwd(shim, 8, conv_class(_cabi, **kw))
        assert rc == INV and "x_out" in err, (kw, rc, err)
    k = conv_class(_cabi)
    k.F_flat = 0  # a flat pointer with no columns
    assert fwd(shim, 8, k)[0] == INV
    assert fwd(shim, 8, conv_class(_cabi, F_flat=0))[0] == 0  # flat NULL with F_flat 0: the features only
    assert fwd(shim, 0, conv_class(_cabi))[0] == INV and fwd(shim, 8, None)[0] == INV and bwd(shim, 8, None)[0] == INV
    for kw in (dict(g_feat=None), dict(gemb=None), dict(gw1=None), dict(gb1=None), dict(gw2=None), dict(gb2=None), dict(g_ld=127),
               dict(gw1=0xc0002)):
        rc, err, _ = bwd(shim, 8, grad_class(_cabi, **kw))
        assert rc == INV and "g_feat" in err, (kw, rc, err)
    need = bwd(shim, 8, grad_class(_cabi), query=1, ws=None, nbytes=0)[2][0]
    assert need > 0
    for ws, nbytes in ((None, need), (0x100008, need), (0x100000, need - 1)):
        rc, err, _ = bwd(shim, 8, grad_class(_cabi), ws=ws, nbytes=nbytes)
        assert rc == INV and "workspace" in err and str(need) in err


def test_input_grad_plan(shim):
    from ai_economist_amd import _cabi

    def mlp_grad(F, H, M, value=True):
        net = _cabi.AieMlpClass(x=0x1000, x_ld=F, w1=0x2000, b1=0x3000, w2=0x4000, b2=0x5000, w3=0x6000, b3=0x7000,
                                wv=0x8000 if value else None, bv=0x9000 if value else None, logits=None, values=None, F=F, H=H, M=M)
        v = 0x100 if value else None
        return _cabi.AieMlpGradClass(net=net, g_logits=0xa000, g_values=v and 0xb000, gw1=0xc000, gb1=0xd000, gw2=0xe000, gb2=0xf000,
                                     gw3=0x10000, gb3=0x11000, gwv=v and 0x12000, gbv=v and 0x13000)

    def call(B, a, q, ws, nbytes, gxa, lda, nca, gxp, ldp, ncp, n=4):
        err = ctypes.create_string_buffer(512)
        plan = ctypes.create_string_buffer(shim.shim_sizeof_igrad_plan())
        rc = shim.shim_plan_input_grad(n, B, ctypes.addressof(a) if a else None, ctypes.addressof(q) if q else None, ws, nbytes,
                                       gxa, lda, nca, gxp, ldp, ncp, ctypes.addressof(err), 512, ctypes.addressof(plan))
        o = (ctypes.c_longlong * 8)()
        shim.shim_igrad_geometry(ctypes.addressof(plan), ctypes.addressof(o))
        return rc, err.value.decode(), list(o)

    a, q = mlp_grad(264, 128, 50), mlp_grad(86, 128, 154)
    B, n, T = 70, 4, shim.shim_igrad_tile()
    rc, err, o = call(B, a, q, 0x100000, 1 << 40, 0x200000, 264, 128, 0x300000, 86, 86)
    assert rc == 0, err
    rows_a = B * n
    assert o[2] == -(-rows_a // T) * 1 and o[3] == -(-B // T) and o[0] == o[2] + o[3] and o[1] == T * 128 * 4
    # dz1 is the fourth [rows, H] block of the class's share: where aie_plan_mlp_backward_launch puts it
    assert o[5] == 0x100000 + 4 * 3 * rows_a * 128
    fl_a = 4 * rows_a * 128 + -(-rows_a // shim.shim_seg()) * ((264 + 1) * 128 + 129 * 128 + 129 * 51)
    assert o[6] == 0x100000 + 4 * (-(-fl_a // 64) * 64) + 4 * 3 * B * 128
    need = o[4]
    rc, err, o = call(B, a, q, 0x100000, need, 0x200000, 300, 264, None, 0, 0)  # the planner left out; 264 columns: two groups
    assert rc == 0 and o[3] == 0 and o[2] == -(-rows_a // T) * 2
    assert call(B, a, q, 0x100000, need, None, 0, 0, None, 0, 0)[2][0] == 0  # nothing asked for: nothing to launch
    INV = _cabi.E_INVALID
    for args, word in (((0x100000, need - 1, 0x200000, 264, 128, None, 0, 0), "workspace"),
                       ((None, need, 0x200000, 264, 128, None, 0, 0), "workspace"),
                       ((0x100004, need, 0x200000, 264, 128, None, 0, 0), "workspace"),
                       ((0x100000, need, 0x200000, 264, 0, None, 0, 0), "ncols"),
                       ((0x100000, need, 0x200000, 264, 265, None, 0, 0), "ncols"),
                       ((0x100000, need, 0x200000, 127, 128, None, 0, 0), "ncols"),
                       ((0x100000, need, 0x200002, 264, 128, None, 0, 0), "aligned")):
        rc, err, _ = call(B, a, q, *args)
        assert rc == INV and word in err and "aie_policy_mlp_input_grad" in err, (args, rc, err)
    rc, err, _ = call(B, a, None, 0x100000, need, None, 0, 0, 0x300000, 86, 86)  # a g_x without its class
    assert rc == INV and "class" in err
    assert call(0, a, q, 0x100000, need, 0x200000, 264, 128, None, 0, 0)[0] == INV  # the backward's own refusals
