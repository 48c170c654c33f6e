"""The trainer calls' host plans (csrc/aie_trainer_plan.h), compiled here with the host C compiler: what aie_capi.hip's
entry points check, hand to their kernels and launch, without a device.  Parameter blocks come from aie_build_params on the
C2 configuration (4 agents of 50 logits, a planner of seven 22-entry rows) and COVID (51 agents of 11 logits with collated
masks, a planner of 21).  Operands are fake, aligned addresses: a plan dereferences nothing.

Every expectation is written out here from the formulas include/aie.h and csrc/aie_trainer_math.h document, never taken from the
plan: the MLP groups' geometry and the backward's workspace layout, the PPO loss's wavefronts and workspace, the
evaluator's work items, the GAE grid, the trajectory copy's width, and -- for every refusal include/aie.h documents -- the
code, a message that names the function, silence with err == NULL, and which refusal wins when two apply.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import C2, ROOT, load_covid_golden, make_env

CSRC = os.path.join(ROOT, "ai-economist_amd", "csrc")
OK, INVALID, UNSUPPORTED = 0, -1, -5
TILE, CHUNK, SEG, MAX_WAVES, RECORD = 32, 256, 256, 8192, 16  # aie_trainer_math.h / aie.h; checked against the header below
vp, i32, u32, i64, f32 = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.c_float


def _struct(name, *groups):
    fields = []
    for typ, names in groups:
        fields += [(n, typ) for n in names.split()]
    return type(name, (C.Structure,), {"_fields_": fields})


# ---- mirrors of the kernel arguments (aie_trainer_math.h) and of the plans; the shim's sizeof guards them ----
EvalGroup = _struct("EvalGroup", (vp, "lg mk act g_logp g_ent logp ent grad"), (u32, "lg_bstride mk_bstride"),
                    (i32, "len lrs mrs mks lsh rows items generic"))
EvalArgs = _struct("EvalArgs", (EvalGroup, "agents planner"), (vp, "params"), (u32, "B items"), (i32, "act_a_width ragged"))
EvalPlan = _struct("EvalPlan", (EvalArgs, "A"), (u32, "grid block"))
GaeArgs = _struct("GaeArgs", (vp, "log va vp adv_a adv_p ret_a ret_p"), (i32, "T slots first E n"), (f32, "gamma gl"))
GaePlan = _struct("GaePlan", (GaeArgs, "A"), (u32, "grid block"))
PpoGroup = _struct("PpoGroup", (vp, "lg val mk act lp_old adv val_old ret mom grad grad_v stats"),
                   (f32, "clip vf_clip vf_coef ent_coef scale g_H kv"), (u32, "lg_bstride"),
                   (i32, "len lrs lsh rows w actors items generic"))
PpoArgs = _struct("PpoArgs", (PpoGroup, "agents planner"), (vp, "params index ws"), (u32, "B items waves"), (i32, "act_a_width ragged"))
PpoPlan = _struct("PpoPlan", (PpoArgs, "A"), (u32, "grid block reduce_grid reduce_block"), (i64, "need"))
MlpGroup = _struct("MlpGroup", (vp, "x w1 b1 w2 b2 w3 b3 wv bv logits values"), (i64, "x_ld rows"), (i32, "F H M blocks lds_a lds_h"))
MlpArgs = _struct("MlpArgs", (MlpGroup, "agents planner"))
MlpFwdPlan = _struct("MlpFwdPlan", (MlpArgs, "A"), (u32, "grid block"), (C.c_size_t, "lds"))
MlpBwdGroup = _struct("MlpBwdGroup", (MlpGroup, "net"), (vp, "g_logits g_values h1 h2 dz2 dz1 partial gw1 gb1 gw2 gb2 gw3 gb3 gwv gbv"),
                      (i32, "lds_c nseg P off2 off3 N3"), (i32 * 3, "cg items"), (i32, "per_seg"), (i64, "n_items"))
MlpBwdArgs = _struct("MlpBwdArgs", (MlpBwdGroup, "agents planner"), (i32, "reduce_blocks_a"))
MlpBwdPlan = _struct("MlpBwdPlan", (MlpBwdArgs, "A"), (i64 * 2, "ws_floats"), (i64, "need"),
                     (u32, "grid_rows grid_atd grid_reduce block"), (C.c_size_t, "lds"))
TrajSegK = _struct("TrajSegK", (vp, "src dst"), (i64, "src_stride"), (i32, "bytes"), (C.c_int16, "rows wide"))
TrajArgs = _struct("TrajArgs", (TrajSegK * 16, "seg"), (vp, "slot"), (i32, "n_segs n_slots E pad_"))
TrajPlan = _struct("TrajPlan", (TrajArgs, "A"), (u32, "grid block"))
PLANS = [EvalPlan, GaePlan, PpoPlan, MlpFwdPlan, MlpBwdPlan, TrajPlan]

SHIM = r"""
#include <stdlib.h>
#include "aie_layout_build.h"
#include "aie_trainer_plan.h"
typedef const void* cv;
void* shim_params(const aie_config* c, char* err, int n) {
  aie_params* p = (aie_params*)malloc(sizeof(aie_params));
  if (aie_build_params(c, p, NULL, err, (size_t)n) != AIE_OK) { free(p); return NULL; }
  return p;
}
void shim_free(void* p) { free(p); }
int shim_sizeof(int i) {
  const size_t s[6] = {sizeof(aie_eval_plan), sizeof(aie_gae_plan), sizeof(aie_ppo_plan), sizeof(aie_mlp_fwd_plan),
                       sizeof(aie_mlp_bwd_plan), sizeof(aie_traj_plan)};
  return (int)s[i];
}
int shim_const(int i) {
  const int v[5] = {AIE_MLP_TILE_ROWS, AIE_MLP_CHUNK, AIE_MLP_BWD_SEG, AIE_PPO_MAX_WAVES, AIE_PPO_RECORD};
  return v[i];
}
int shim_evaluate(const aie_params* P, cv dp, cv arena, long long B, cv* o, char* err, size_t n, aie_eval_plan* p) {
  return aie_plan_policy_evaluate(P, dp, arena, B, o[0], o[1], o[2], o[3], o[4], o[5], (float*)o[6], (float*)o[7], (float*)o[8],
                                  (float*)o[9], err, n, p);
}
int shim_evaluate_backward(const aie_params* P, cv dp, cv arena, long long B, cv* o, char* err, size_t n, aie_eval_plan* p) {
  return aie_plan_policy_evaluate_backward(P, dp, arena, B, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], (float*)o[10],
                                           (float*)o[11], err, n, p);
}
int shim_gae(const aie_params* P, int T, cv log, int slots, int first, float gamma, float lambda, cv* o, char* err, size_t n,
             aie_gae_plan* p) {
  return aie_plan_gae(P, T, log, slots, first, o[0], o[1], gamma, lambda, (float*)o[2], (float*)o[3], (float*)o[4], (float*)o[5], err,
                      n, p);
}
long long shim_ppo_workspace_bytes(const aie_params* P, long long B) { return aie_plan_ppo_workspace_bytes(P, B); }
int shim_ppo(const aie_params* P, cv dp, cv arena, long long B, const aie_ppo_class* a, const aie_ppo_class* q, cv index, void* ws,
             char* err, size_t n, aie_ppo_plan* p) {
  return aie_plan_ppo_loss(P, dp, arena, B, a, q, index, ws, err, n, p);
}
int shim_mlp_forward(const aie_params* P, long long B, const aie_mlp_class* a, const aie_mlp_class* q, char* err, size_t n,
                     aie_mlp_fwd_plan* p) {
  return aie_plan_mlp_forward(P, B, a, q, err, n, p);
}
/* ws NULL: the workspace-bytes query's path (the first step alone) */
int shim_mlp_backward(const aie_params* P, long long B, const aie_mlp_grad_class* a, const aie_mlp_grad_class* q, void* ws, char* err,
                      size_t n, aie_mlp_bwd_plan* p) {
  const int rc = aie_plan_mlp_backward(P, B, a, q, err, n, p);
  return rc != AIE_OK || !ws ? rc : aie_plan_mlp_backward_launch(p, B, a, q, ws, err, n);
}
int shim_trajectory(const aie_params* P, const aie_traj_segment* s, int n_segs, int n_slots, int32_t* slot, char* err, size_t n,
                    aie_traj_plan* p) {
  return aie_plan_trajectory_store(P, s, n_segs, n_slots, slot, err, n, p);
}
"""


class Plans:
    """The compiled shim and the parameter blocks of the configurations."""

    def __init__(self, d):
        from ai_economist_amd import _cabi

        self.cabi = _cabi
        src, so = os.path.join(d, "shim_plan.c"), os.path.join(d, "shim_plan.so")
        with open(src, "w") as f:
            f.write(SHIM)
        subprocess.run(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src,
                        "-o", so, "-lm"], check=True)
        L = self.lib = C.CDLL(so)
        L.shim_params.restype = vp
        L.shim_params.argtypes = [vp, C.c_char_p, C.c_int]
        L.shim_free.argtypes = [vp]
        L.shim_ppo_workspace_bytes.restype = C.c_longlong
        L.shim_ppo_workspace_bytes.argtypes = [vp, C.c_longlong]
        tail = [C.c_char_p, C.c_size_t, vp]
        L.shim_evaluate.argtypes = L.shim_evaluate_backward.argtypes = [vp, vp, vp, C.c_longlong, vp] + tail
        L.shim_gae.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, f32, f32, vp] + tail
        L.shim_ppo.argtypes = [vp, vp, vp, C.c_longlong, vp, vp, vp, vp] + tail
        L.shim_mlp_forward.argtypes = [vp, C.c_longlong, vp, vp] + tail
        L.shim_mlp_backward.argtypes = [vp, C.c_longlong, vp, vp, vp] + tail
        L.shim_trajectory.argtypes = [vp, vp, C.c_int, C.c_int, vp] + tail
        self.params, self.cfg = {}, {}
        covid = dict(load_covid_golden("c4_covid_51ag")["cfg"], scenario_name="CovidAndEconomySimulation")
        multi = dict(C2, multi_action_mode_agents=True)  # six action slots per agent (Build, four of the auction, Gather)
        for name, cfg, E in (("c2", C2, 5), ("covid", covid, 3), ("ragged_planner", C2, 5), ("c2_multi", multi, 5)):
            c = make_env(cfg, n_envs=E).build_config()
            if name == "ragged_planner":  # a foreign planner row of another length than the tax rows': what the samplers refuse
                c.host_p_n, c.host_p_dim[0], c.host_p_before[0] = 1, 5, c.n_components
            err = C.create_string_buffer(512)
            self.params[name] = L.shim_params(C.addressof(c), err, 512)
            assert self.params[name], err.value
            self.cfg[name] = c

    def close(self):
        for p in self.params.values():
            self.lib.shim_free(p)

    def call(self, fn, plan_type, *args):
        """-> (rc, message, plan).  Runs the plan a second time with err == NULL: the same code, and nothing to write to."""
        err = C.create_string_buffer(b"\xaa" * 511, 512)
        plan, quiet = plan_type(), plan_type()
        rc = getattr(self.lib, fn)(*args, err, 512, C.addressof(plan))
        assert getattr(self.lib, fn)(*args, None, 0, C.addressof(quiet)) == rc
        if rc == OK:
            assert err.raw[:4] == b"\xaa" * 4, "an accepted call wrote a message"
            assert bytes(plan) == bytes(quiet)
            return rc, "", plan
        msg = err.value.decode()
        assert msg and len(msg) < 511 and "\xaa" not in msg
        return rc, msg, plan


@pytest.fixture(scope="module")
def S():
    with tempfile.TemporaryDirectory() as d:
        s = Plans(d)
        yield s
        s.close()


def ceil(a, b):
    return -(-a // b)


def pad4(v):
    return (v + 3) // 4 * 4


DP, ARENA, WS = 0x7E0000000000, 0x7D0000000000, 0x7C0000000100  # device parameter block, arena, workspace
_next = [0x7F0000000000]


def addr(align=256):
    """A fresh fake device address."""
    _next[0] += 0x100000
    return _next[0] + (align if align < 256 else 0)


def ptrs(*v):
    return (vp * len(v))(*v)


def refused(S, code, starts, fn, plan_type, *args):
    rc, msg, _ = S.call(fn, plan_type, *args)
    assert rc == code, (rc, msg)
    assert msg.startswith(starts), msg
    return msg


def test_the_mirrors_and_constants_are_the_headers(S):
    for i, t in enumerate(PLANS):
        assert S.lib.shim_sizeof(i) == C.sizeof(t), t.__name__
    assert [S.lib.shim_const(i) for i in range(5)] == [TILE, CHUNK, SEG, MAX_WAVES, RECORD]
    assert (SEG, MAX_WAVES) == (S.cabi.MLP_BWD_SEG, S.cabi.PPO_MAX_WAVES) and S.cabi.TRAJ_MAX_SEGMENTS == 16


# ---- the policy MLP ----
SHAPES = [(1, 16, 1), (255, 16, 3), (256, 128, 50), (257, 256, 1024), (1024, 256, 1)]


def mlp_class(S, F, H, M, value=True, x_ld=None, forward=True):
    k = S.cabi.AieMlpClass(x=addr(), x_ld=F if x_ld is None else x_ld, w1=addr(), b1=addr(), w2=addr(), b2=addr(), w3=addr(), b3=addr(),
                           wv=addr() if value else None, bv=addr() if value else None, logits=addr() if forward else None,
                           values=addr() if forward and value else None, F=F, H=H, M=M)
    return k


def grad_class(S, F, H, M, value=True, **kw):
    g = {k: addr() for k in ("g_logits", "gw1", "gb1", "gw2", "gb2", "gw3", "gb3")}
    if value:
        g.update(g_values=addr(), gwv=addr(), gbv=addr())
    return S.cabi.AieMlpGradClass(net=mlp_class(S, F, H, M, value, forward=False, **kw), **g)


def want_group(F, H, M, rows):
    """aie_trainer_math.h: the two LDS images' row strides and the row tiles of a class."""
    return dict(F=F, H=H, M=M, rows=rows, lds_a=max(min(pad4(F), CHUNK), H) + 2, lds_h=H + 2, blocks=ceil(rows, TILE))


def check_group(G, want, k):
    for name, v in want.items():
        assert getattr(G, name) == v, (name, getattr(G, name), v)
    for name in ("x", "x_ld", "w1", "b1", "w2", "b2", "w3", "b3", "wv", "bv"):
        assert getattr(G, name) == getattr(k, name), name
    assert G.lds_a % 4 == 2 and G.lds_h % 4 == 2  # (what spreads a fragment read over the banks)


@pytest.mark.parametrize("cfg,n", [("c2", 4), ("covid", 51)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_mlp_class_fill_forward_and_backward_agree(S, cfg, n, shape):
    F, H, M = shape
    P = S.params[cfg]
    other = SHAPES[(SHAPES.index(shape) + 2) % len(SHAPES)]  # the planner's network: another shape, no value column
    for B in (1, 7, 33):
        a, q = mlp_class(S, F, H, M, x_ld=F + 5), mlp_class(S, *other, value=False)
        rc, _, fw = S.call("shim_mlp_forward", MlpFwdPlan, P, B, C.addressof(a), C.addressof(q))
        assert rc == OK
        wa, wq = want_group(F, H, M, B * n), want_group(*other, B)
        check_group(fw.A.agents, wa, a)
        check_group(fw.A.planner, wq, q)
        assert (fw.A.agents.logits, fw.A.agents.values, fw.A.planner.logits, fw.A.planner.values) == (a.logits, a.values, q.logits, None)
        assert (fw.grid, fw.block) == (wa["blocks"] + wq["blocks"], 256)
        assert fw.lds == max(TILE * (w["lds_a"] + w["lds_h"]) * 4 for w in (wa, wq))  # the larger class wins
        # one class alone: the other's group stays zero and takes no part
        rc, _, solo = S.call("shim_mlp_forward", MlpFwdPlan, P, B, None, C.addressof(q))
        assert rc == OK and bytes(solo.A.agents) == bytes(MlpGroup()) and bytes(solo.A.planner) == bytes(fw.A.planner)
        assert (solo.grid, solo.lds) == (wq["blocks"], TILE * (wq["lds_a"] + wq["lds_h"]) * 4)
        # the backward's net group: the forward's, bit for bit, apart from logits and values
        ga, gq = grad_class(S, F, H, M), grad_class(S, *other, value=False)
        for name in ("x", "x_ld", "w1", "b1", "w2", "b2", "w3", "b3", "wv", "bv"):
            setattr(ga.net, name, getattr(a, name))
            setattr(gq.net, name, getattr(q, name))
        rc, _, bw = S.call("shim_mlp_backward", MlpBwdPlan, P, B, C.addressof(ga), C.addressof(gq), WS)
        assert rc == OK
        for fg, bg in ((fw.A.agents, bw.A.agents.net), (fw.A.planner, bw.A.planner.net)):
            f = MlpGroup.from_buffer_copy(bytes(fg))
            f.logits = f.values = None
            assert bytes(f) == bytes(bg) and bg.logits is None and bg.values is None
        lds_c = [min(pad4(m), CHUNK) + 2 for m in (M, other[2])]
        assert [bw.A.agents.lds_c, bw.A.planner.lds_c] == lds_c
        assert bw.lds == max(TILE * (w["lds_a"] + w["lds_h"] + c) * 4 for w, c in ((wa, lds_c[0]), (wq, lds_c[1])))


def want_backward(F, H, M, v, rows):
    """include/aie.h: the workspace; aie_trainer_math.h: the partials' three blocks [(K + 1), N] and the second launch's items (four
    16-row bands by up to four 16-column tiles, per layer and segment)."""
    nseg = ceil(rows, SEG)
    N3 = M + v
    blocks = [(F + 1, H), (H + 1, H), (H + 1, N3)]
    P = sum(k * n for k, n in blocks)
    items = [ceil(ceil(k, 16), 4) * ceil(ceil(n, 16), 4) for k, n in blocks]
    return dict(nseg=nseg, N3=N3, P=P, off2=blocks[0][0] * blocks[0][1], off3=blocks[0][0] * blocks[0][1] + blocks[1][0] * blocks[1][1],
                per_seg=sum(items), n_items=nseg * sum(items), floats=ceil(4 * rows * H + nseg * P, 64) * 64)


@pytest.mark.parametrize("B", [1, 32, 33, 256, 257, 2 * 256 + 17])
def test_mlp_backward_workspace_and_launches(S, B):
    n = 4
    P = S.params["c2"]
    for (Fa, Ha, Ma), (Fp, Hp, Mp), va, vq in (((200, 128, 50), (86, 16, 22), 1, 0), ((1, 16, 1), (1024, 256, 3), 0, 1)):
        ga, gq = grad_class(S, Fa, Ha, Ma, value=bool(va)), grad_class(S, Fp, Hp, Mp, value=bool(vq))
        wa, wq = want_backward(Fa, Ha, Ma, va, B * n), want_backward(Fp, Hp, Mp, vq, B)
        # the query: the first step alone
        rc, _, query = S.call("shim_mlp_backward", MlpBwdPlan, P, B, C.addressof(ga), C.addressof(gq), None)
        assert rc == OK and query.need == 4 * (wa["floats"] + wq["floats"]) and query.grid_rows == 0
        rc, _, bw = S.call("shim_mlp_backward", MlpBwdPlan, P, B, C.addressof(ga), C.addressof(gq), WS)
        assert rc == OK and bw.need == query.need and list(bw.ws_floats) == [wa["floats"], wq["floats"]]
        base = WS
        for Q, w, g, rows, H in ((bw.A.agents, wa, ga, B * n, Ha), (bw.A.planner, wq, gq, B, Hp)):
            for name in ("nseg", "N3", "P", "off2", "off3", "per_seg", "n_items"):
                assert getattr(Q, name) == w[name], name
            assert sum(Q.items) == w["per_seg"]
            # h1, h2, dz2, dz1 as [rows, H] each, then the partials [nseg][P]; the next class starts where this one ends
            assert [Q.h1, Q.h2, Q.dz2, Q.dz1, Q.partial] == [base + 4 * i * rows * H for i in range(5)]
            assert Q.partial + 4 * w["nseg"] * w["P"] <= base + 4 * w["floats"] < Q.partial + 4 * w["nseg"] * w["P"] + 4 * 64
            base += 4 * w["floats"]
            for name in ("g_logits", "g_values", "gw1", "gb1", "gw2", "gb2", "gw3", "gb3", "gwv", "gbv"):
                assert getattr(Q, name) == getattr(g, name), name
        assert base == WS + bw.need
        assert bw.A.reduce_blocks_a == ceil(wa["P"], 256)
        assert (bw.grid_rows, bw.grid_atd, bw.grid_reduce, bw.block) == (
            ceil(B * n, TILE) + ceil(B, TILE), wa["n_items"] + wq["n_items"], ceil(wa["P"], 256) + ceil(wq["P"], 256), 256)
        # the planner alone: its region starts at the workspace, and no workgroup of the third launch is the agents'
        rc, _, solo = S.call("shim_mlp_backward", MlpBwdPlan, P, B, None, C.addressof(gq), WS)
        assert rc == OK and solo.need == 4 * wq["floats"] and solo.A.planner.h1 == WS and solo.A.reduce_blocks_a == 0
        assert bytes(solo.A.agents) == bytes(MlpBwdGroup())


def test_mlp_refusals(S):
    P = S.params["c2"]
    # (byref, not addressof: the tuple then keeps a class built in the call's argument list alive until the plan has read it)
    fwd = lambda B, a, q: ("shim_mlp_forward", MlpFwdPlan, P, B, a and C.byref(a), q and C.byref(q))  # noqa: E731
    bwd = lambda B, a, q, ws=WS: ("shim_mlp_backward", MlpBwdPlan, P, B, a and C.byref(a), q and C.byref(q), ws)  # noqa: E731
    F, B = "aie_policy_mlp_forward: ", "aie_policy_mlp_backward: "
    good, gg = mlp_class(S, 20, 32, 5), grad_class(S, 20, 32, 5)
    # both classes NULL: nothing to launch, after the check of B
    for call, name in ((fwd, F), (bwd, B)):
        rc, _, p = S.call(*call(3, None, None))
        assert rc == OK and (p.grid if call is fwd else p.grid_rows + p.need) == 0
        assert "B = 0" in refused(S, INVALID, name, *call(0, None, None))
        assert "B = -2" in refused(S, INVALID, name, *call(-2, good if call is fwd else gg, None))
    # the forward's own operands
    for change, code in ((dict(F=0), INVALID), (dict(F=1025), INVALID), (dict(M=0), INVALID), (dict(M=1025), INVALID),
                         (dict(x_ld=19), INVALID), (dict(x=None), INVALID), (dict(w1=None), INVALID), (dict(b1=None), INVALID),
                         (dict(w2=None), INVALID), (dict(b2=None), INVALID), (dict(w3=None), INVALID), (dict(b3=None), INVALID),
                         (dict(logits=None), INVALID), (dict(values=None), INVALID), (dict(wv=None), INVALID), (dict(bv=None), INVALID),
                         (dict(H=0), UNSUPPORTED), (dict(H=8), UNSUPPORTED), (dict(H=24), UNSUPPORTED), (dict(H=272), UNSUPPORTED)):
        for c in (0, 1):
            k = mlp_class(S, 20, 32, 5)
            for name, v in change.items():
                setattr(k, name, v)
            msg = refused(S, code, F + "the %s " % ("planner's" if c else "agents'"), *fwd(2, *((good, k) if c else (k, good))))
            assert ("hidden width %d" % k.H in msg) if code == UNSUPPORTED else ("F (%d) and M (%d)" % (k.F, k.M) in msg)
    # the backward: the forward's refusals for its net (logits and values are ignored there), and its gradient pointers
    for change, code in ((dict(F=0), INVALID), (dict(M=1025), INVALID), (dict(x_ld=19), INVALID), (dict(x=None), INVALID),
                         (dict(w3=None), INVALID), (dict(bv=None), INVALID), (dict(wv=None), INVALID), (dict(H=8), UNSUPPORTED),
                         (dict(H=272), UNSUPPORTED)):
        for c in (0, 1):
            g = grad_class(S, 20, 32, 5)
            for name, v in change.items():
                setattr(g.net, name, v)
            refused(S, code, B + "the %s " % ("planner's" if c else "agents'"), *bwd(2, *((gg, g) if c else (g, gg))))
            # (the query refuses with the same code)
            assert S.call(*bwd(2, *((gg, g) if c else (g, gg)), None))[0] == code
    g = grad_class(S, 20, 32, 5)
    g.net.logits, g.net.values = addr(), None  # ignored
    assert S.call(*bwd(2, g, None))[0] == OK
    for name in ("g_logits", "gw1", "gb1", "gw2", "gb2", "gw3", "gb3", "g_values", "gwv", "gbv"):
        g = grad_class(S, 20, 32, 5)
        setattr(g, name, None)
        assert "g_logits" in refused(S, INVALID, B + "the agents' ", *bwd(2, g, gg))
    for name in ("g_values", "gwv", "gbv"):  # there without net.wv
        g = grad_class(S, 20, 32, 5, value=False)
        setattr(g, name, addr())
        refused(S, INVALID, B + "the planner's ", *bwd(2, None, g))
    # more than one call takes: 0x3fffffff row tiles per class
    assert S.call(*fwd(TILE * 0x3fffffff, None, good))[0] == OK
    assert "more than one" in refused(S, INVALID, F, *fwd(TILE * 0x3fffffff + 1, None, good))
    assert "more than one" in refused(S, INVALID, B, *bwd(TILE * 0x3fffffff + 1, None, gg))
    # the backward's second launch: a workgroup per item, nseg x per_seg of them -- past one launch long before the row tiles are
    big = grad_class(S, 1024, 256, 1024)
    items = sum(ceil(ceil(k, 16), 4) * ceil(ceil(m, 16), 4) for k, m in ((1025, 256), (257, 256), (257, 1025)))
    Bmax = 0x7fffff00 // items * SEG // 4  # the agents' rows are 4 B
    assert S.call(*bwd(Bmax, big, None))[0] == OK and S.call(*bwd(Bmax + SEG, big, None, None))[0] == OK  # (the query does not launch)
    assert "more than one call" in refused(S, INVALID, B, *bwd(Bmax + SEG, big, None))
    # (the forward's bound on the workgroups of BOTH classes cannot be reached: the planner has at most half the agents' tiles, n >= 2,
    # and each class is held to 0x3fffffff -- 1.5 x 0x3fffffff < 0x7fffff00; the same for the backward's row tiles)
    # ---- two refusals at once: today's winner ----
    bad_h, no_ptr = mlp_class(S, 20, 40, 5), mlp_class(S, 20, 32, 5)
    no_ptr.w2 = None
    assert "B = 0" in refused(S, INVALID, F, *fwd(0, bad_h, None))                 # B ahead of the classes
    both = mlp_class(S, 20, 40, 5)
    both.logits = None
    refused(S, INVALID, F + "the agents' class needs", *fwd(2, both, None))        # a class's operands ahead of its hidden width
    refused(S, UNSUPPORTED, F + "the agents' hidden", *fwd(2, bad_h, no_ptr))      # the agents ahead of the planner
    g = grad_class(S, 20, 40, 5)
    g.gw2 = None
    refused(S, INVALID, B + "the agents' class needs g_logits", *bwd(2, g, None))  # a gradient pointer ahead of the hidden width
    g.net.x = None
    assert "x_ld" in refused(S, INVALID, B + "the agents' class needs F", *bwd(2, g, None))  # the net ahead of the gradients
    assert "B = 0" in refused(S, INVALID, B, *bwd(0, g, None))


# ---- the PPO loss ----
def ppo_class(S, values=True, **kw):
    k = dict(logits=addr(), values=addr() if values else None, masks=addr(), actions=addr(), logp_old=addr(), adv=addr(),
             values_old=addr() if values else None, returns=addr() if values else None, adv_moments=None, grad_logits=addr(),
             grad_values=addr() if values else None, stats=addr(), clip=0.3, vf_clip=50.0, vf_coef=0.05, ent_coef=0.025)
    k.update(kw)
    return S.cabi.AiePpoClass(**k)


# work items per batch element: agents' rows in aligned lane segments, or one per actor on the generic path
#   c2: 4 single-slot agents of 50 logits (a wavefront each); the planner has 7 slots: generic, one item
#   covid: 51 single-slot agents of 11 logits (16 lanes: four rows a wavefront); the planner one row of 21
PPO_ITEMS = {"c2": (4, 1, 4, 1), "covid": (ceil(51, 4), 1, 51, 1)}  # items_a, items_p, actors_a, actors_p


@pytest.mark.parametrize("cfg", ["c2", "covid"])
def test_ppo_waves_workspace_and_paths(S, cfg):
    P = S.params[cfg]
    ia, ip, na, np_ = PPO_ITEMS[cfg]
    for B in (1, 7, 4096, MAX_WAVES + 3):
        a, q = ppo_class(S), ppo_class(S, values=False, clip=0.2, ent_coef=0.5)
        rc, _, p = S.call("shim_ppo", PpoPlan, P, DP, ARENA, B, C.addressof(a), C.addressof(q), addr(), WS)
        assert rc == OK
        A = p.A
        assert (A.agents.items, A.planner.items, A.items, A.B) == (ia, ip, ia + ip, B)
        assert (A.agents.actors, A.planner.actors) == (na, np_)
        assert (A.agents.generic, A.planner.generic) == (0, 1 if cfg == "c2" else 0)  # more than one slot per actor: generic
        assert (A.agents.w, A.planner.w) == (1, 7 if cfg == "c2" else 1)
        waves = min(B * (ia + ip), MAX_WAVES)
        assert A.waves == waves and p.need == waves * RECORD * 8
        assert (p.grid, p.block, p.reduce_grid, p.reduce_block) == (ceil(waves, 4), 256, 1, 1024)
        bound = S.lib.shim_ppo_workspace_bytes(P, B)
        assert p.need <= bound == min(B * (na + 1), MAX_WAVES) * 128 <= MAX_WAVES * 128
        assert (A.params, A.ws) == (DP, WS) and A.agents.lg == a.logits and A.planner.stats == q.stats and A.planner.val is None
        for G, k, actors in ((A.agents, a, na), (A.planner, q, np_)):
            scale = np.float32(1.0) / np.float32(B * actors)
            assert G.scale == scale and G.g_H == -(scale * np.float32(k.ent_coef)) and G.kv == scale * np.float32(k.vf_coef)
            assert (G.clip, G.vf_clip) == (k.clip, k.vf_clip)
        # one class: the other takes no wavefronts
        rc, _, solo = S.call("shim_ppo", PpoPlan, P, DP, ARENA, B, None, C.addressof(q), None, WS)
        assert rc == OK and solo.A.items == ip and solo.A.waves == min(B * ip, MAX_WAVES) and solo.A.index is None
    assert S.lib.shim_ppo_workspace_bytes(P, 0) == INVALID
    rc, _, none = S.call("shim_ppo", PpoPlan, P, DP, ARENA, 3, None, None, None, None)
    assert rc == OK and none.grid == 0  # no class: B and the samplers' refusals are checked, nothing is launched


def test_ppo_refusals(S):
    P = S.params["c2"]
    call = lambda B, a, q, P=P: ("shim_ppo", PpoPlan, P, DP, ARENA, B, a and C.byref(a), q and C.byref(q), None, WS)  # noqa: E731
    N = "aie_ppo_loss: "
    for c in (0, 1):
        for kw in (dict(logits=None), dict(masks=None), dict(actions=None), dict(logp_old=None), dict(adv=None), dict(grad_logits=None),
                   dict(stats=None), dict(values_old=None), dict(returns=None), dict(grad_values=None), dict(clip=0.0), dict(clip=-1.0),
                   dict(clip=float("nan"))):
            k = ppo_class(S, **kw)
            refused(S, INVALID, N + "the %s class" % ("planner's" if c else "agents'"), *call(4, *((None, k) if c else (k, None))))
        k = ppo_class(S, values=False, grad_values=addr())  # grad_values without values
        refused(S, INVALID, N + "the ", *call(4, *((None, k) if c else (k, None))))
    for B in (0, -1):
        assert "B = %d" % B in refused(S, INVALID, N, *call(B, ppo_class(S), None))
        assert "B = %d" % B in refused(S, INVALID, N, *call(B, None, None))
    # (the rows' shape is the evaluator's, and so is its bound: 4 + 4 wavefronts per batch element there, 4 + 1 items here)
    assert "more than one" in refused(S, INVALID, N, *call(0x7fffff00 // 8 + 1, ppo_class(S), ppo_class(S)))
    assert S.call(*call(0x7fffff00 // 8, ppo_class(S), ppo_class(S)))[0] == OK
    # the samplers' refusal: its own words
    R = S.params["ragged_planner"]
    refused(S, UNSUPPORTED, "samplers: ", *call(4, ppo_class(S), None, P=R))
    # ---- two at once ----
    refused(S, INVALID, N + "the agents' class", *call(0, ppo_class(S, adv=None), None))             # a class ahead of B
    refused(S, INVALID, N + "the agents' class", *call(4, ppo_class(S, adv=None), ppo_class(S, stats=None)))
    refused(S, INVALID, N + "the planner's class", *call(4, None, ppo_class(S, clip=0.0), P=R))      # ... and of the samplers'
    refused(S, UNSUPPORTED, "samplers: ", *call(0, ppo_class(S), None, P=R))                           # the samplers' ahead of B


# ---- policy evaluation ----
def eval_ops(classes="ap", masks=True, logp=True, entropy=True):
    """[logits_a, logits_p, masks_a, masks_p, actions_a, actions_p, logp_a, logp_p, entropy_a, entropy_p]"""
    a, q = "a" in classes, "p" in classes
    return [addr() if a else None, addr() if q else None, addr() if a and masks else None, addr() if q and masks else None,
            addr() if a else None, addr() if q else None, addr() if a and logp else None, addr() if q and logp else None,
            addr() if a and entropy else None, addr() if q and entropy else None]


# (rows, entries, lanes a row takes) per class: the fast path packs 64 // lanes rows into a wavefront
EVAL_ROWS = {"c2": ((4, 50, 64), (7, 22, 32)), "covid": ((51, 11, 16), (1, 21, 32))}


@pytest.mark.parametrize("cfg,E", [("c2", 5), ("covid", 3)])
def test_evaluate_items_masks_and_grid(S, cfg, E):
    P = S.params[cfg]
    (ra, la, sa), (rp, lp, sp) = EVAL_ROWS[cfg]
    ia, ip = ceil(ra, 64 // sa), ceil(rp, 64 // sp)
    for B in (1, E, 1000):
        for classes, items in (("ap", (ia, ip)), ("a", (ia, 0)), ("p", (0, ip))):
            o = eval_ops(classes)
            rc, _, p = S.call("shim_evaluate", EvalPlan, P, DP, ARENA, B, ptrs(*o))
            assert rc == OK
            A = p.A
            assert (A.agents.items, A.planner.items, A.items, A.B, A.params) == items + (sum(items), B, DP)
            assert (p.grid, p.block) == (ceil(B * sum(items), 4), 256)
            assert (A.agents.generic, A.planner.generic, A.ragged) == (0, 0, 0)
            for G, on, k, rows, ln, seg in ((A.agents, "a" in classes, 0, ra, la, sa), (A.planner, "p" in classes, 1, rp, lp, sp)):
                assert (G.rows, G.len, 1 << G.lsh, G.lrs, G.lg_bstride) == (rows, ln, seg, ln, rows * ln)
                if on:  # the caller's masks: the logits' layout
                    assert (G.lg, G.mk, G.act, G.logp, G.ent) == (o[k], o[2 + k], o[4 + k], o[6 + k], o[8 + k])
                    assert (G.mk_bstride, G.mrs, G.mks) == (rows * ln, ln, 1)
            # the backward shares the rows' shape; a class is there when its gradient buffer is
            ob = o[:6] + [addr() if "a" in classes else None, None, None, addr(), addr() if "a" in classes else None, addr() if "p" in classes else None]
            rc, _, b = S.call("shim_evaluate_backward", EvalPlan, P, DP, ARENA, B, ptrs(*ob))
            assert rc == OK and (b.grid, b.A.agents.items, b.A.planner.items) == (p.grid,) + items
            assert (b.A.agents.grad, b.A.planner.grad, b.A.agents.g_logp, b.A.planner.g_ent) == (ob[10], ob[11], ob[6], ob[9])
    # a class none of whose outputs is asked for is left out; with no output at all there is nothing to launch
    o = eval_ops("ap")
    o[7] = o[9] = None
    rc, _, p = S.call("shim_evaluate", EvalPlan, P, DP, ARENA, 4, ptrs(*o))
    assert rc == OK and (p.A.agents.items, p.A.planner.items) == (ia, 0)
    rc, _, p = S.call("shim_evaluate", EvalPlan, P, DP, ARENA, 4, ptrs(*eval_ops("ap", logp=False, entropy=False)))
    assert rc == OK and p.grid == 0 and p.A.items == 0
    # the arena's current masks: B == E only; COVID's agent masks are collated there (entry stride n, row stride 1)
    o = eval_ops("ap", masks=False)
    rc, _, p = S.call("shim_evaluate", EvalPlan, P, DP, ARENA, E, ptrs(*o))
    assert rc == OK and ARENA < p.A.agents.mk and ARENA < p.A.planner.mk and p.A.agents.mk % 4 == 0
    assert (p.A.agents.mrs, p.A.agents.mks) == ((1, ra) if cfg == "covid" else (la, 1)) and (p.A.planner.mrs, p.A.planner.mks) == (lp, 1)
    for B in (E - 1, E + 1):
        assert "B = %d" % B in refused(S, INVALID, "aie_policy_evaluate: ", "shim_evaluate", EvalPlan, P, DP, ARENA, B, ptrs(*o))
        o2 = eval_ops("ap")
        o2[3] = None  # one class's masks are enough to tie B to E
        refused(S, INVALID, "aie_policy_evaluate: ", "shim_evaluate", EvalPlan, P, DP, ARENA, B, ptrs(*o2))


def test_evaluate_generic_path_is_a_row_per_wavefront(S):
    """Multi-action agents: rows of different lengths (ragged), n x 6 of them per batch element, one row a wavefront -- where
    the fast path would pack them.  The planner's seven 22-entry rows stay on the fast path."""
    P = S.params["c2_multi"]
    rows_a, items_p = 4 * 6, ceil(7, 64 // 32)
    for B in (1, 5, 333):
        o = eval_ops("ap")
        ob = o[:6] + [addr(), addr(), None, None, addr(), addr()]
        for fn, ops in (("shim_evaluate", o), ("shim_evaluate_backward", ob)):
            rc, _, p = S.call(fn, EvalPlan, P, DP, ARENA, B, ptrs(*ops))
            assert rc == OK
            A = p.A
            assert (A.ragged, A.act_a_width, A.agents.generic, A.planner.generic) == (1, 6, 1, 0)
            assert (A.agents.rows, A.agents.items, A.planner.items, A.items) == (rows_a, rows_a, items_p, rows_a + items_p)
            assert (p.grid, p.block) == (ceil(B * (rows_a + items_p), 4), 256)
        rc, _, p = S.call("shim_evaluate", EvalPlan, P, DP, ARENA, B, ptrs(*eval_ops("a")))
        assert rc == OK and (p.A.agents.items, p.A.planner.items, p.grid) == (rows_a, 0, ceil(B * rows_a, 4))
        # the PPO loss on the same rows: an item is an ACTOR there, six slots each
        rc, _, q = S.call("shim_ppo", PpoPlan, P, DP, ARENA, B, C.addressof(ppo_class(S)), None, None, WS)
        assert rc == OK and (q.A.agents.generic, q.A.agents.w, q.A.agents.actors, q.A.agents.items, q.A.ragged) == (1, 6, 4, 4, 1)


def test_evaluate_refusals(S):
    P, R = S.params["c2"], S.params["ragged_planner"]
    fw = lambda B, o, P=P: ("shim_evaluate", EvalPlan, P, DP, ARENA, B, ptrs(*o))  # noqa: E731
    bw = lambda B, o, P=P: ("shim_evaluate_backward", EvalPlan, P, DP, ARENA, B, ptrs(*o))  # noqa: E731
    F, Bk = "aie_policy_evaluate: ", "aie_policy_evaluate_backward: "
    for drop in ((0,), (1,), (4,), (5,)):  # logits or stored actions missing under a logp; logits under an entropy
        o = eval_ops("ap")
        for i in drop:
            o[i] = None
        refused(S, INVALID, F + "an output without", *fw(4, o))
    o = eval_ops("ap", logp=False)
    o[4] = o[5] = None  # entropy alone needs no actions
    assert S.call(*fw(4, o))[0] == OK
    good_b = lambda: eval_ops("ap")[:6] + [addr(), addr(), None, None, addr(), addr()]  # noqa: E731
    for i in (0, 1, 4, 5):  # a gradient buffer without its logits; a logp gradient without the stored actions
        o = good_b()
        o[i] = None
        refused(S, INVALID, Bk + "a gradient buffer without", *bw(4, o))
    for call, name, ops in ((fw, F, eval_ops("ap")), (bw, Bk, good_b())):
        for B in (0, -3):
            assert "B = %d" % B in refused(S, INVALID, name, *call(B, ops))
        assert "more than one launch" in refused(S, INVALID, name, *call(0x7fffff00 // 8 + 1, ops))
        assert S.call(*call(0x7fffff00 // 8, ops))[0] == OK
        refused(S, UNSUPPORTED, "samplers: ", *call(4, ops, P=R))
        # ---- two at once: the operands ahead of the samplers' refusal, that ahead of B ----
        bad = list(ops)
        bad[0] = None
        refused(S, INVALID, name, *call(0, bad, P=R))
        refused(S, UNSUPPORTED, "samplers: ", *call(0, ops, P=R))


# ---- GAE ----
@pytest.mark.parametrize("cfg,E,n", [("c2", 5, 4), ("covid", 3, 51)])
def test_gae_plan(S, cfg, E, n):
    P = S.params[cfg]
    log, o = addr(), [addr() for _ in range(6)]  # values_a, values_p, adv_a, adv_p, ret_a, ret_p
    gamma, lam = 0.998, 0.98
    rc, _, p = S.call("shim_gae", GaePlan, P, 200, log, 256, 255, gamma, lam, ptrs(*o))
    assert rc == OK and (p.grid, p.block) == (ceil(E * (n + 2), 64), 64)
    A = p.A
    assert (A.log, A.va, A.vp, A.adv_a, A.adv_p, A.ret_a, A.ret_p) == (log,) + tuple(o)
    assert (A.T, A.slots, A.first, A.E, A.n) == (200, 256, 255, E, n)
    assert A.gamma == np.float32(gamma) and A.gl == np.float32(gamma) * np.float32(lam)  # one rounded float32 product
    # a class none of whose outputs is asked for is left out; neither: nothing to launch
    rc, _, p = S.call("shim_gae", GaePlan, P, 1, log, 1, 0, gamma, lam, ptrs(o[0], o[1], None, o[3], None, None))
    assert rc == OK and (p.A.va, p.A.vp, p.grid) == (None, o[1], ceil(E * (n + 2), 64))
    rc, _, p = S.call("shim_gae", GaePlan, P, 1, log, 1, 0, gamma, lam, ptrs(o[0], o[1], None, None, None, None))
    assert rc == OK and p.grid == 0
    N = "aie_gae: "
    for T, lg, slots, first in ((0, log, 8, 0), (9, log, 8, 0), (4, log, 8, -1), (4, log, 8, 8), (4, None, 8, 0)):
        refused(S, INVALID, N + "T = %d" % T, "shim_gae", GaePlan, P, T, lg, slots, first, gamma, lam, ptrs(*o))
    for ops in ((None, o[1], o[2], o[3], None, None), (None, o[1], None, None, o[4], None), (o[0], None, None, o[3], None, None),
                (o[0], None, None, None, None, o[5])):
        refused(S, INVALID, N + "an output without its values", "shim_gae", GaePlan, P, 4, log, 8, 0, gamma, lam, ptrs(*ops))
    # (the bound on the floats of a log row, E (n + 2) <= 0x7fffff00, takes more replicas than a parameter block built here has)
    # two at once: the ring ahead of the values
    refused(S, INVALID, N + "T = 0", "shim_gae", GaePlan, P, 0, log, 8, 0, gamma, lam, ptrs(None, None, o[2], None, None, None))
    refused(S, INVALID, N + "T = 4", "shim_gae", GaePlan, P, 4, None, 8, 0, gamma, lam, ptrs(None, None, o[2], None, None, None))


# ---- trajectory storage ----
def test_trajectory_plan(S):
    P = S.params["covid"]
    Seg = S.cabi.AieTrajSegment
    slot = addr()
    call = lambda segs, n=None, slots=8, slot=slot: ("shim_trajectory", TrajPlan, P, (Seg * max(1, len(segs)))(*segs) if segs is not None  # noqa: E731
                                                     else None, len(segs) if n is None else n, slots, slot)
    a16 = 0x7B0000000000
    # wide exactly when source, destination, stride and size are all multiples of 16 and the copy is plain
    cases = [(a16, a16 + 0x1000, 64, 32, 0, 1), (a16, a16 + 0x1000, 64, 32, 1, 1), (a16 + 4, a16 + 0x1000, 64, 32, 0, 0),
             (a16, a16 + 0x1008, 64, 32, 0, 0), (a16, a16 + 0x1000, 72, 32, 0, 0), (a16, a16 + 0x1000, 64, 24, 0, 0),
             (a16, a16 + 0x1000, 64, 32, 2, 0), (a16, a16 + 0x1000, 51 * 11 * 4, 51 * 11 * 4, 11, 0), (a16, a16 + 0x1000, 4, 4, 0, 0),
             (a16, a16 + 0x1000, 0, 16, 0, 1), (a16, a16 + 0x1000, 32767 * 4, 32767 * 4, 32767, 0)]
    segs = [Seg(s, d, st, b, r) for s, d, st, b, r, _ in cases]
    rc, _, p = S.call(*call(segs))
    assert rc == OK and (p.grid, p.block) == (3, 256)  # a workgroup per replica
    assert (p.A.slot, p.A.n_segs, p.A.n_slots, p.A.E) == (slot, len(cases), 8, 3)
    for k, (s, d, st, b, r, wide) in zip(p.A.seg, cases):
        assert (k.src, k.dst, k.src_stride, k.bytes, k.rows, k.wide) == (s, d, st, b, r, wide)
    assert S.call(*call(segs[:1] * 16))[0] == OK
    N = "aie_trajectory_store: "
    for bad in (call([], n=0), call(segs[:1] * 17), call(None, n=1), call(segs[:1], slots=0), call(segs[:1], slot=None)):
        refused(S, INVALID, N, *bad)
    assert "17 segments" in refused(S, INVALID, N, *call(segs[:1] * 17))
    for s, d, st, b, r in ((None, a16, 64, 32, 0), (a16, None, 64, 32, 0), (a16, a16, 64, 0, 0), (a16, a16, 64, 30, 0), (a16, a16, 62, 32, 0),
                           (a16 + 2, a16, 64, 32, 0), (a16, a16 + 1, 64, 32, 0), (a16, a16, 64, 32, -1), (a16, a16, 32768 * 4, 32768 * 4, 32768),
                           (a16, a16, 64, 32, 3)):  # (32 bytes: 8 elements, which 3 rows do not divide)
        assert "rows %d" % r in refused(S, INVALID, N + "segment 1 ", *call([segs[0], Seg(s, d, st, b, r), segs[1]]))
    # two at once: the counts ahead of a segment; the first bad segment ahead of a later one
    assert "0 slots" in refused(S, INVALID, N + "1 segments", *call([Seg(None, a16, 64, 32, 0)], slots=0))
    refused(S, INVALID, N + "segment 1 ", *call([segs[0], Seg(a16, a16, 64, 30, 0), segs[1], Seg(None, a16, 64, 32, 0)]))
