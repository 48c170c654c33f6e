"""aie_adam_step's host plan (csrc/aie_trainer_plan.h: aie_plan_adam_groups, aie_plan_adam), compiled here with the host C
compiler: what aie_capi.hip's entry point checks, hands to its two kernels and launches, without a device.  Operands are
fake addresses: a plan dereferences nothing but the descriptor array, which is host memory.

Every expectation is written out here from include/aie.h's text, never taken from the plan: the grid (a workgroup per
chunk of 1024 elements, both groups in one launch), the chunk table (a tensor's first chunk in its group), the `wide`
flags (all four pointers 16-byte aligned), the workspace's size (8 * (4 + chunks) bytes per group) and carve-up, and --
for every refusal the header documents -- the code, a message that names the function, silence with err == NULL, and
which refusal wins when two apply (the header's order).
"""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "ai-economist_amd", "csrc")
OK, INVALID = 0, -1
CHUNK, MAX_TENSORS, HEAD = 1024, 16, 4
GRID_MAX = 0x7FFFFF00
vp, i32, u32, i64, f32 = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.c_float


def _struct(name, *groups):
    fields = []
    for typ, names in groups:
        fields += [(n, typ) for n in names.split()]
    return type(name, (C.Structure,), {"_fields_": fields})


# mirrors of the kernels' argument (aie_trainer_math.h) and of the plan; the shim's sizeof guards them
TensorK = _struct("TensorK", (vp, "w g m v"), (i64, "n"), (i32, "first wide"))
GroupK = _struct("GroupK", (TensorK * MAX_TENSORS, "t"), (vp, "lr state stats ws"), (f32, "beta1 beta2 eps max_norm"),
                 (i32, "n_tensors chunks"))
AdamArgs = _struct("AdamArgs", (GroupK * 2, "grp"))
AdamPlan = _struct("AdamPlan", (AdamArgs, "A"), (i64 * 2, "ws_bytes"), (i64, "need"), (u32, "grid block"))

SHIM = r"""
#include "aie_trainer_plan.h"
int shim_sizeof(void) { return (int)sizeof(aie_adam_plan); }
int shim_const(int i) {
  const int v[4] = {AIE_OPT_CHUNK, AIE_OPT_MAX_TENSORS, AIE_OPT_WS_HEAD, AIE_OPT_SLOTS};
  return v[i];
}
/* query != 0: the workspace-bytes query's path (the first step alone) */
int shim_adam(const aie_opt_group* a, const aie_opt_group* q, int query, void* ws, long long bytes, char* err, size_t n,
              aie_adam_plan* p) {
  return query ? aie_plan_adam_groups(a, q, err, n, p) : aie_plan_adam(a, q, ws, bytes, err, n, p);
}
"""


@pytest.fixture(scope="module")
def lib():
    with tempfile.TemporaryDirectory() as d:
        src, so = os.path.join(d, "shim_opt_plan.c"), os.path.join(d, "shim_opt_plan.so")
        with open(src, "w") as f:
            f.write(SHIM)
        subprocess.run(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src,
                        "-o", so, "-lm"], check=True)
        L = C.CDLL(so)
        L.shim_adam.argtypes = [vp, vp, C.c_int, vp, C.c_longlong, C.c_char_p, C.c_size_t, vp]
        yield L


_next = [0x7F0000000000]
WS = 0x7C0000000100


def addr(offset=0):
    """A fresh fake device address, 256-byte aligned plus `offset`."""
    _next[0] += 0x10000000
    return _next[0] + offset


def group(sizes, offsets=None, **kw):
    """An aie_opt_group of tensors with the given element counts; offsets[i]: (w, g, m, v) byte offsets from 256-byte
    alignment.  -> (the structure, its descriptor array: keep both alive)."""
    from ai_economist_amd import _cabi

    offsets = offsets or [(0, 0, 0, 0)] * len(sizes)
    arr = (_cabi.AieOptTensor * max(1, len(sizes)))(*[_cabi.AieOptTensor(addr(o[0]), addr(o[1]), addr(o[2]), addr(o[3]), n)
                                                     for n, o in zip(sizes, offsets)])
    f = dict(tensors=arr, n_tensors=len(sizes), beta1=0.9, beta2=0.999, eps=1e-8, max_norm=10.0, d_lr=addr(4), d_state=addr(8),
             d_stats=addr(4))
    f.update(kw)
    return _cabi.AieOptGroup(**f), arr


def call(lib, ga, gp, ws=WS, nbytes=1 << 40, query=0):
    """-> (rc, message, plan).  Runs the plan a second time with err == NULL: the same code, and nothing to write to."""
    err = C.create_string_buffer(b"\xaa" * 511, 512)
    plan, quiet = AdamPlan(), AdamPlan()
    a = C.addressof(ga[0]) if ga else None
    p = C.addressof(gp[0]) if gp else None
    rc = lib.shim_adam(a, p, query, ws, nbytes, err, 512, C.addressof(plan))
    assert lib.shim_adam(a, p, query, ws, nbytes, None, 0, C.addressof(quiet)) == rc
    if rc == OK:
        assert err.raw[:4] == b"\xaa" * 4, "an accepted call wrote a message"
        assert bytes(plan) == bytes(quiet)
        return rc, "", plan
    msg = err.value.decode()
    assert msg and len(msg) < 511 and "\xaa" not in msg
    assert msg.startswith("aie_adam_step: "), msg
    return rc, msg, plan


def ceil(a, b):
    return -(-a // b)


def test_the_mirror_and_constants_are_the_headers(lib):
    from ai_economist_amd import _cabi

    assert lib.shim_sizeof() == C.sizeof(AdamPlan)
    assert [lib.shim_const(i) for i in range(4)] == [CHUNK, MAX_TENSORS, HEAD, 256]
    assert (CHUNK, MAX_TENSORS) == (_cabi.OPT_CHUNK, _cabi.OPT_MAX_TENSORS)
    assert C.sizeof(AdamArgs) <= 4096  # a kernel argument


SIZES_A = [1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17]
SIZES_P = [136 * 128, 128, 128 * 128, 128, 128 * 50, 50, 128, 1]  # C2's agents' network: 40 627 parameters


def check_group(K, g, arr, sizes, offsets, ws):
    first = 0
    for i, n in enumerate(sizes):
        t, o = K.t[i], offsets[i]
        assert (t.w, t.g, t.m, t.v, t.n) == (arr[i].w, arr[i].g, arr[i].m, arr[i].v, n)
        assert t.first == first and t.wide == int(all(x % 16 == 0 for x in o)), (i, t.first, t.wide)
        first += ceil(n, CHUNK)
    for i in range(len(sizes), MAX_TENSORS):
        assert (K.t[i].w, K.t[i].n) == (None, 0)
    assert (K.n_tensors, K.chunks) == (len(sizes), first)
    assert (K.lr, K.state, K.stats, K.ws) == (g.d_lr, g.d_state, g.d_stats, ws)
    assert (K.beta1, K.beta2, K.eps, K.max_norm) == (g.beta1, g.beta2, g.eps, g.max_norm)
    return first


@pytest.mark.parametrize("which", ["both", "agents", "planner"])
def test_grid_chunk_table_wide_flags_and_workspace(lib, which):
    # every way a tensor can miss 16-byte alignment: one pointer at a time, by 4, 8 or 12 bytes, and all four by 4
    off_a = [(0, 0, 0, 0), (4, 0, 0, 0), (0, 8, 0, 0), (0, 0, 12, 0), (0, 0, 0, 4), (4, 4, 4, 4), (16, 32, 48, 64)] + [(0, 0, 0, 0)] * 4
    off_p = [(0, 0, 0, 0)] * len(SIZES_P)
    ga = group(SIZES_A, off_a, max_norm=0.0) if which != "planner" else None
    gp = group(SIZES_P, off_p, beta1=0.0, beta2=0.5, eps=1e-3) if which != "agents" else None
    chunks_a = sum(ceil(n, CHUNK) for n in SIZES_A) if ga else 0
    chunks_p = sum(ceil(n, CHUNK) for n in SIZES_P) if gp else 0
    bytes_a = 8 * (HEAD + chunks_a) if ga else 0
    bytes_p = 8 * (HEAD + chunks_p) if gp else 0
    need = bytes_a + bytes_p
    for query in (1, 0):
        rc, _, p = call(lib, ga, gp, nbytes=need, query=query)
        assert rc == OK
        assert (p.grid, p.block, p.need, tuple(p.ws_bytes)) == (chunks_a + chunks_p, 256, need, (bytes_a, bytes_p))
        if ga:
            assert check_group(p.A.grp[0], ga[0], ga[1], SIZES_A, off_a, None if query else WS) == chunks_a
        else:
            assert p.A.grp[0].chunks == 0 and p.A.grp[0].n_tensors == 0
        if gp:
            assert check_group(p.A.grp[1], gp[0], gp[1], SIZES_P, off_p, None if query else WS + bytes_a) == chunks_p
        else:
            assert p.A.grp[1].chunks == 0
    assert chunks_p == 17 + 1 + 16 + 1 + 7 + 1 + 1 + 1 or not gp
    # a byte short is refused; the query does not look at the workspace
    rc, msg, _ = call(lib, ga, gp, nbytes=need - 1)
    assert rc == INVALID and "workspace" in msg and str(need) in msg
    assert call(lib, ga, gp, ws=None, nbytes=0, query=1)[0] == OK


def test_no_group_launches_nothing(lib):
    for query in (0, 1):
        rc, _, p = call(lib, None, None, ws=None, nbytes=0, query=query)
        assert (rc, p.grid, p.need) == (OK, 0, 0)


def test_sixteen_tensors_and_a_large_one(lib):
    g16 = group([1] * 16)
    rc, _, p = call(lib, g16, None)
    assert rc == OK and p.grid == 16 and [p.A.grp[0].t[i].first for i in range(16)] == list(range(16))
    big = group([(1 << 33) + 1])  # element indices beyond 2^32: 8 388 609 chunks
    rc, _, p = call(lib, None, big)
    assert rc == OK and p.grid == (1 << 23) + 1 and p.need == 8 * (HEAD + (1 << 23) + 1)
    # more chunks than one launch takes: in one tensor, and across the two groups
    assert call(lib, group([CHUNK * (GRID_MAX + 1)]), None)[0] == INVALID
    assert call(lib, group([CHUNK * GRID_MAX]), None)[0] == OK
    rc, msg, _ = call(lib, group([CHUNK * GRID_MAX]), group([1]))
    assert rc == INVALID and "planner's" in msg and "chunks" in msg


def bad_tensor(field, value):
    def make():
        g, arr = group([5, 7, 9])
        setattr(arr[1], field, value)
        return g, arr
    return make


NAN = float("nan")
REFUSALS = {  # name -> (a maker of the group, a word of the message)
    "no_tensors": (lambda: group([], n_tensors=0), "tensors"),
    "seventeen_tensors": (lambda: group([1], n_tensors=17), "tensors"),
    "null_tensors": (lambda: group([1], tensors=None), "tensors"),
    "beta1_one": (lambda: group([1], beta1=1.0), "beta1"),
    "beta1_negative": (lambda: group([1], beta1=-0.1), "beta1"),
    "beta1_nan": (lambda: group([1], beta1=NAN), "beta1"),
    "beta2_one": (lambda: group([1], beta2=1.0), "beta2"),
    "beta2_negative": (lambda: group([1], beta2=-1e-3), "beta2"),
    "eps_zero": (lambda: group([1], eps=0.0), "eps"),
    "eps_negative": (lambda: group([1], eps=-1e-8), "eps"),
    "eps_nan": (lambda: group([1], eps=NAN), "eps"),
    "lr_null": (lambda: group([1], d_lr=None), "d_lr"),
    "lr_misaligned": (lambda: group([1], d_lr=addr(2)), "d_lr"),
    "state_null": (lambda: group([1], d_state=None), "d_state"),
    "state_misaligned": (lambda: group([1], d_state=addr(4)), "d_state"),
    "stats_null": (lambda: group([1], d_stats=None), "d_stats"),
    "stats_misaligned": (lambda: group([1], d_stats=addr(1)), "d_stats"),
    "w_null": (bad_tensor("w", None), "tensor 1"),
    "g_null": (bad_tensor("g", None), "tensor 1"),
    "m_null": (bad_tensor("m", None), "tensor 1"),
    "v_null": (bad_tensor("v", None), "tensor 1"),
    "w_misaligned": (bad_tensor("w", 0x7B0000000002), "tensor 1"),
    "g_misaligned": (bad_tensor("g", 0x7B0000000001), "tensor 1"),
    "m_misaligned": (bad_tensor("m", 0x7B0000000003), "tensor 1"),
    "v_misaligned": (bad_tensor("v", 0x7B0000000006), "tensor 1"),
    "n_zero": (bad_tensor("n", 0), "tensor 1"),
    "n_negative": (bad_tensor("n", -4), "tensor 1"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(lib, name):
    make, word = REFUSALS[name]
    good = group([3, 2000])
    for query in (0, 1):  # the query refuses what the call refuses, the workspace apart
        for ga, gp, who in ((make(), None, "agents'"), (None, make(), "planner's"), (good, make(), "planner's"), (make(), good, "agents'")):
            rc, msg, _ = call(lib, ga, gp, query=query)
            assert rc == INVALID and word in msg and who in msg, (name, msg)


def test_workspace_refusals(lib):
    g = group([3, 2000])
    need = 8 * (HEAD + 1 + 2)
    assert call(lib, g, None, nbytes=need)[0] == OK
    for ws, nbytes in ((None, need), (WS + 4, need), (WS + 1, need), (WS, need - 8), (WS, 0), (WS, -1)):
        rc, msg, _ = call(lib, g, None, ws=ws, nbytes=nbytes)
        assert rc == INVALID and "workspace" in msg and "aie_adam_workspace_bytes" in msg, msg


def test_which_refusal_wins(lib):
    """The header's order: the agents' group before the planner's; in a group the tensor count, the hyper-parameters, the
    three scalar pointers, the tensors in order; the workspace last."""
    def first_word(ga, gp, **kw):
        rc, msg, _ = call(lib, ga, gp, **kw)
        assert rc == INVALID
        return msg

    assert "agents'" in first_word(group([1], eps=0.0), group([1], n_tensors=0))
    assert "tensors at" in first_word(group([1], n_tensors=0, beta1=2.0, d_lr=None), None)
    assert "beta1" in first_word(group([1], beta1=2.0, d_lr=None), None)
    g, arr = group([1, 1], d_stats=None)
    arr[0].n = 0
    assert "d_stats" in first_word((g, arr), None)
    g, arr = group([1, 1, 1])
    arr[2].w, arr[1].n = None, 0
    assert "tensor 1" in first_word((g, arr), None)
    g, arr = group([1, 1])
    arr[1].v = None
    assert "tensor 1" in first_word((g, arr), None, ws=None, nbytes=0)  # a bad tensor before a bad workspace
    assert "planner's" in first_word(group([1]), group([1], eps=0.0), ws=None, nbytes=0)
