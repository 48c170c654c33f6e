"""The policy network's backward pass, CPU side (csrc/aie_trainer_math.h: aie_mlp_row_backward, aie_mlp_grad_entry -- the twins
of aie_policy_mlp_backward's kernels):

  * values: the header's helpers, compiled here with the host C compiler, == the numpy transcription
    (tests/policy_mlp_bwd_ref.py) on the five shapes of policy_mlp_ref.SHAPES, the value column on and off, at 1 ..
    2 SEG + 17 rows (a short, a whole and several segments), with dead ReLU columns, exact zeros in the observations and
    incoming gradients drawn like aie_ppo_loss's (float ==: there is no NaN anywhere);
  * accuracy: every entry within the running bound of a float32 evaluation around the float64 pass with the same ReLU
    masks (policy_mlp_bwd_ref.backward_f64: derived, not measured); torch's float64 autograd of the same masked network
    equals that pass to float64 rounding (the formulas, independently), and torch's float32 CPU autograd lies inside the
    same bound, so the bound is a fair one.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import policy_mlp_bwd_ref as bref
import policy_mlp_ref as ref
from helpers import ROOT
from test_policy_mlp_cpu import _fp

CSRC = os.path.join(ROOT, "ai-economist_amd", "csrc")
f32, f64 = np.float32, np.float64

SHIM = r"""
#include <stdlib.h>
#include "aie_trainer_math.h"
int shim_seg(void) { return AIE_MLP_BWD_SEG; }
void shim_mlp_backward(const float* x, long x_ld, long rows, int F, int H, int M, const float* w1, const float* b1, const float* w2,
                       const float* b2, const float* w3, const float* wv, const float* g_logits, const float* g_values, float* gw1,
                       float* gb1, float* gw2, float* gb2, float* gw3, float* gb3, float* gwv, float* gbv) {
  float* scratch = (float*)malloc(sizeof(float) * 4 * (size_t)rows * (size_t)H);
  aie_mlp_backward_host(x, x_ld, rows, F, H, M, w1, b1, w2, b2, w3, wv, g_logits, g_values, scratch, gw1, gb1, gw2, gb2, gw3, gb3,
                        gwv, gbv);
  free(scratch);
}
"""


def build_bwd_shim(d):
    src, so = os.path.join(d, "shim_bwd.c"), os.path.join(d, "shim_bwd.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), src, "-o", so, "-lm"], check=True)
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.shim_seg.restype = ctypes.c_int
    lib.shim_mlp_backward.argtypes = [fp, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [fp] * 16
    return lib


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as d:
        yield build_bwd_shim(d)


def c_backward(lib, x, W, g_logits, g_values):
    """The header's helpers -> the dict of gradients; outputs start as NaN."""
    x = np.ascontiguousarray(x, f32)
    W = {k: np.ascontiguousarray(v, f32) for k, v in W.items() if v is not None}
    g_logits = np.ascontiguousarray(g_logits, f32)
    g_values = np.ascontiguousarray(g_values, f32) if "wv" in W else None
    rows, F = x.shape
    G = {k: np.full(W[k].shape, np.nan, f32) for k in bref.NAMES if k in W}
    lib.shim_mlp_backward(_fp(x), F, rows, F, W["w1"].shape[1], W["w3"].shape[1], _fp(W["w1"]), _fp(W["b1"]), _fp(W["w2"]),
                          _fp(W["b2"]), _fp(W["w3"]), _fp(W.get("wv")), _fp(g_logits), _fp(g_values),
                          *[_fp(G.get(k)) for k in bref.NAMES])
    return G


def test_the_constant_is_the_bindings(shim):
    from ai_economist_amd import _cabi

    assert shim.shim_seg() == _cabi.MLP_BWD_SEG and _cabi.MLP_BWD_SEG % 64 == 0


@pytest.mark.parametrize("value", [True, False], ids=["value", "novalue"])
@pytest.mark.parametrize("shape", ref.SHAPES + ref.EDGE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_header_equals_the_transcription(shim, shape, value):
    F, H, M = shape
    SEG = shim.shim_seg()
    largest = sorted(ref.SHAPES, key=lambda s: s[0] * s[1] + s[1] * s[1] + s[1] * s[2])[-2:]
    counts = [1, 33, SEG - 1, SEG, SEG + 1] + ([] if shape in largest else [2 * SEG + 17])
    if shape in ref.EDGE_SHAPES:  # the widths are what is new: a short segment, and a whole one and a row
        counts = [1, 33, SEG + 1]
    for i, rows in enumerate(counts):
        W = ref.random_weights(F, H, M, seed=7 * F + i, value=value, dead=True)
        x = bref.rows_with_zeros(rows, F, seed=11 * M + i)
        gl, gv = bref.random_grads(rows, M, seed=13 * H + i, value=value)
        assert ((gl == 0).any() or gl.size < 100) and ((x == 0).any() or x.size < 100)  # (the planted zeros are there)
        got = c_backward(shim, x, W, gl, gv)
        want = bref.backward(x, W, gl, gv, SEG)
        assert set(got) == set(want) and (("wv" in got) == value)
        for k in want:
            assert np.isfinite(want[k]).all() and not np.isnan(got[k]).any(), (shape, rows, k)
            assert got[k].shape == want[k].shape
            assert (got[k] == want[k]).all(), "%s, %d rows: %d entries of g%s differ" % (shape, rows, (got[k] != want[k]).sum(), k)
        if rows >= 33:
            assert np.abs(want["w1"]).max() > 0 and np.abs(want["w2"]).max() > 0


def _torch_grads(x, W, gl, gv, m1, m2, dtype):
    """torch's autograd of the network with the masks imposed (pre-activation times a 0 / 1 constant)."""
    import torch

    t = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in W.items()}
    tx, tm1, tm2 = (torch.tensor(np.asarray(a), dtype=dtype) for a in (x, m1, m2))
    h1 = (tx @ t["w1"] + t["b1"]) * tm1
    h2 = (h1 @ t["w2"] + t["b2"]) * tm2
    lg = h2 @ t["w3"] + t["b3"]
    v = h2 @ t["wv"].reshape(-1) + t["bv"]
    ((lg * torch.tensor(gl, dtype=dtype)).sum() + (v * torch.tensor(gv, dtype=dtype)).sum()).backward()
    return {k: t[k].grad.numpy() for k in t}


@pytest.mark.parametrize("shape", ref.SHAPES + ref.EDGE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_accuracy_within_the_derived_bound(shim, shape):
    import torch

    F, H, M = shape
    SEG = shim.shim_seg()
    # SEG + 1 rows: two segments, and n = SEG + 2 roundings are no fewer than the rows torch's sum takes in any order
    for rows in (70, SEG + 1):
        W = ref.random_weights(F, H, M, seed=3 + F, value=True, dead=False)
        x = bref.rows_with_zeros(rows, F, seed=5 + M)
        gl, gv = bref.random_grads(rows, M, seed=9 + H)
        G64, E = bref.backward_f64(x, W, gl, gv, SEG)
        got = c_backward(shim, x, W, gl, gv)
        h1, h2 = bref.hidden(x, W)
        m1, m2 = (h1 > 0), (h2 > 0)
        t64 = _torch_grads(x, W, gl, gv, m1, m2, torch.float64)
        t32 = _torch_grads(x, W, gl, gv, m1, m2, torch.float32)
        worst = {"header": 0.0, "torch": 0.0}
        for k in bref.NAMES:
            # two float64 evaluations: the same derivation with u = 2^-53 for each of them, 2 x 2^-29 of the float32 bound
            assert (np.abs(t64[k].reshape(G64[k].shape) - G64[k]) <= E[k] * 2.0 ** -28).all(), "float64 autograd differs in g" + k
            for name, g in (("header", got[k]), ("torch", t32[k])):
                err = np.abs(g.astype(f64).reshape(G64[k].shape) - G64[k])
                assert (err <= E[k]).all(), "%s: g%s leaves the bound at %d rows" % (name, k, rows)
                worst[name] = max(worst[name], float((err / np.maximum(E[k], 1e-300)).max()))
        print("%s, %d rows: max error / bound %.3f (header), %.3f (torch float32)" % (shape, rows, worst["header"], worst["torch"]))
