"""The policy network's forward pass, CPU side (csrc/aie_trainer_math.h: aie_mlp_row -- the twin of aie_policy_mlp_forward):

  * the fma emulation of tests/policy_mlp_ref.py against the C library's fmaf on 10^5 random triples, halfway cases
    (c = -a b rounded, plus or minus one ulp) among them;
  * policy_mlp_ref.EDGE_SHAPES reaches every shape of the device kernel's loops (worked out from the kernel's constants);
  * values: the header's helper, compiled here with the host C compiler, == the numpy transcription on the shapes of
    policy_mlp_ref.SHAPES and EDGE_SHAPES with 1 - 70 rows, the value column on and off, inputs planted with zeros, dead ReLU columns and
    entries near 1e-38 and 1e30 (float ==: there is no NaN anywhere);
  * accuracy: every logit and value within the running bound of a float32 evaluation around the float64 pass on the same
    float32 numbers (policy_mlp_ref.forward_f64: derived, not measured) -- and torch's CPU float32 MLP inside the same
    bound, so the bound is a fair one.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import policy_mlp_ref as ref
from helpers import ROOT

CSRC = os.path.join(ROOT, "ai-economist_amd", "csrc")
f32 = np.float32

SHIM = r"""
#include <stdlib.h>
#include "aie_trainer_math.h"
void shim_fmaf(const float* a, const float* b, const float* c, long n, float* out) {
  for (long i = 0; i < n; ++i) out[i] = fmaf(a[i], b[i], c[i]);
}
void shim_mlp(const float* x, long x_ld, long rows, int F, int H, int M, const float* w1, const float* b1, const float* w2,
              const float* b2, const float* w3, const float* b3, const float* wv, const float* bv, float* logits, float* values) {
  float* h = (float*)malloc(sizeof(float) * 2 * (size_t)H);
  for (long r = 0; r < rows; ++r)
    aie_mlp_row(x + r * x_ld, F, H, M, w1, b1, w2, b2, w3, b3, wv, bv, h, h + H, logits + r * M, values ? values + r : 0);
  free(h);
}
"""


def build_shim(d):
    src, so = os.path.join(d, "shim.c"), os.path.join(d, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC,
                    "-I" + os.path.join(ROOT, "include"), src, "-o", so, "-lm"], check=True)
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.shim_fmaf.argtypes = [fp, fp, fp, ctypes.c_long, fp]
    lib.shim_mlp.argtypes = [fp, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [fp] * 10
    return lib


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as d:
        yield build_shim(d)


def _fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def c_forward(lib, x, W):
    """The header's helper row by row -> (logits [R, M], values [R] or None); outputs start as NaN."""
    x = np.ascontiguousarray(x, f32)
    W = {k: np.ascontiguousarray(v, f32) for k, v in W.items() if v is not None}
    rows, F = x.shape
    H, M = W["w1"].shape[1], W["w3"].shape[1]
    logits = np.full((rows, M), np.nan, f32)
    values = np.full(rows, np.nan, f32) if "wv" in W else None
    lib.shim_mlp(_fp(x), F, rows, F, H, M, _fp(W["w1"]), _fp(W["b1"]), _fp(W["w2"]), _fp(W["b2"]), _fp(W["w3"]), _fp(W["b3"]),
                 _fp(W.get("wv")), _fp(W.get("bv")), _fp(logits), _fp(values))
    return logits, values


def test_fma_emulation_is_the_c_librarys(shim):
    g = np.random.default_rng(0)
    n = 100000
    a = (g.standard_normal(n) * 10.0 ** g.integers(-12, 12, n)).astype(f32)
    b = (g.standard_normal(n) * 10.0 ** g.integers(-12, 12, n)).astype(f32)
    c = (g.standard_normal(n) * 10.0 ** g.integers(-24, 24, n)).astype(f32)
    # a third: c cancels the product up to its own rounding, plus or minus one ulp -- the halfway and near-halfway cases
    q = n // 3
    p = (a[:q].astype(np.float64) * b[:q].astype(np.float64)).astype(f32)
    c[:q] = -p
    c[: q // 3] = np.nextafter(c[: q // 3], f32(np.inf))
    c[q // 3: 2 * q // 3] = np.nextafter(c[q // 3: 2 * q // 3], f32(-np.inf))
    # and exact halfway sums: a b has 2 set bits 24 places apart, c a power of two beside them
    a[q: q + 1000] = f32(1 + 2.0 ** -12)
    b[q: q + 1000] = f32(1 + 2.0 ** -12)  # a b = 1 + 2^-11 + 2^-24: 2^-24 is half an ulp of 1
    c[q: q + 1000] = (g.integers(-4, 5, 1000) * 2.0 ** -11).astype(f32)
    # small ones: subnormal results
    a[-2000:] *= f32(1e-20)
    c[-2000:] *= f32(1e-20)
    assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()
    want = np.empty(n, f32)
    shim.shim_fmaf(_fp(a), _fp(b), _fp(c), n, _fp(want))
    with np.errstate(all="ignore"):
        got = ref.fma32(a, b, c)
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "fma32 differs at %d triples, first (%r, %r, %r): %r, fmaf %r" % (
        bad.size, a[bad[0]], b[bad[0]], c[bad[0]], got[bad[0]], want[bad[0]])


def test_edge_shapes_cover_the_kernels_loop_shapes():
    """policy_mlp_ref.EDGE_SHAPES reaches every shape of the kernel's loops -- worked out from the kernel's own constants, read
    back from the sources here -- and the table beside the list is what the function gives."""
    import re

    src = open(os.path.join(CSRC, "aie_kernels_mlp.hip")).read()
    hdr = open(os.path.join(CSRC, "aie_trainer_math.h")).read()
    assert int(re.search(r"constexpr int MLP_KC = (\d+);", src).group(1)) == ref.KC
    assert int(re.search(r"#define AIE_MLP_CHUNK (\d+)", hdr).group(1)) == ref.CHUNK
    assert "mfma_f32_16x16x4f32" in src and (ref.TILE, ref.STEP) == (16, 4)
    assert ref.coverage_table() == ref.EDGE_COVERAGE
    assert all(16 <= H <= 256 and H % 16 == 0 and 1 <= F <= 1024 and 1 <= M <= 1024 for F, H, M in ref.EDGE_SHAPES)
    got = ref.edge_coverage()
    want = ["hidden layer: G odd >= 3", "first layer: G odd >= 3", "hidden layer: G even, a tail of 4 steps",
            "hidden layer: G odd >= 3, a tail of 4 steps", "hidden layer: G even", "hidden layer: G=1", "first layer: G=0",
            "first layer: G=1", "first layer: G even", "a second staged chunk", "the value column alone in a tile",
            "the bias row of the backward's [(F + 1), H] block alone in a 64-row group"]
    want += ["NT=%d" % t for t in (3, 5, 9, 13)] + ["M=%d" % m for m in (15, 16, 17, 32, 48, 63, 64, 65, 128)]
    want += ["F=%d" % f for f in (63, 64, 65, 255, 256, 257)]
    assert not [w for w in want if w not in got], [w for w in want if w not in got]
    # G odd and >= 3: in a hidden layer at H = 96, 160 and 224, in the first layer at F = 96 .. 127
    odd = lambda K: [g for g, _, _ in ref.loop_shape(K)][0] % 2 == 1 and ref.loop_shape(K)[0][0] >= 3  # noqa: E731
    assert all(odd(H) for H in (96, 160, 224)) and {H for _, H, _ in ref.EDGE_SHAPES} >= {96, 160, 224}
    assert all(odd(F) for F in range(96, 128)) and any(96 <= F < 128 for F, _, _ in ref.EDGE_SHAPES)
    # what SHAPES alone reaches: G = 0, 1, 4, 8 in the hidden layers and NT = 1, 2, 8, 16 -- none of the above
    old = ref.edge_coverage(ref.SHAPES)
    assert not old & {"hidden layer: G odd >= 3", "NT=3", "NT=5", "NT=9", "NT=13", "the value column alone in a tile"}


@pytest.mark.parametrize("value", [True, False])
@pytest.mark.parametrize("shape", ref.SHAPES + ref.EDGE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_header_equals_the_transcription(shim, shape, value):
    F, H, M = shape
    for i, rows in enumerate((1, 33, 70)):
        W = ref.random_weights(F, H, M, seed=7 * F + i, value=value)
        x = ref.random_rows(rows, F, seed=11 * M + i)
        got_l, got_v = c_forward(shim, x, W)
        want_l, want_v = ref.forward(x, W)
        assert not np.isnan(want_l).any() and not np.isnan(got_l).any()
        assert (got_l == want_l).all(), "%s, %d rows: %d logits differ" % (shape, rows, (got_l != want_l).sum())
        assert (got_v is None) == (want_v is None) == (not value)
        if value:
            assert not np.isnan(got_v).any() and (got_v == want_v).all(), "%s, %d rows: values differ" % (shape, rows)
        # the planted inputs do what they are planted for: dead columns, and the large rows stay finite
        assert np.isfinite(want_l).all()
        if rows > 5 and F > 1:
            assert np.abs(want_l[5]).max() > 1e20


@pytest.mark.parametrize("shape", ref.SHAPES + ref.EDGE_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_accuracy_within_the_derived_bound(shim, shape):
    import torch

    F, H, M = shape
    W = ref.random_weights(F, H, M, seed=3 + F, value=True, dead=False)  # (a bias of -1e6 would widen the bound)
    x = ref.random_rows(70, F, seed=5 + M)
    lg64, v64, blg, bv = ref.forward_f64(x, W)
    got_l, got_v = c_forward(shim, x, W)
    el, ev = np.abs(got_l.astype(np.float64) - lg64), np.abs(got_v.astype(np.float64) - v64)
    print("%s: header: max error / bound %.3f (logits), %.3f (value)" % (shape, (el / blg).max(), (ev / bv).max()))
    assert (el <= blg).all() and (ev <= bv).all()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in W.items()}
    h = torch.relu(torch.addmm(t["b1"], torch.from_numpy(x), t["w1"]))
    h = torch.relu(torch.addmm(t["b2"], h, t["w2"]))
    tl = torch.addmm(t["b3"], h, t["w3"]).numpy()
    tv = torch.addmv(t["bv"], h, t["wv"]).numpy()
    etl, etv = np.abs(tl.astype(np.float64) - lg64), np.abs(tv.astype(np.float64) - v64)
    print("%s: torch:  max error / bound %.3f (logits), %.3f (value)" % (shape, (etl / blg).max(), (etv / bv).max()))
    assert (etl <= blg).all() and (etv <= bv).all()
