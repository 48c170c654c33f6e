"""aie_adam_step on the device (Backend.adam_step, rollout.Adam) against the header's helpers compiled on the CPU
(tests/test_adam_cpu.py holds them to an independent transcription):

  * values: three eager steps at the CPU test's tensor sizes -- both groups, each alone, sixteen tensors, the clip switching
    on and off, the learning rate changing -- equal the helpers under float ==: weights, moments, state and statistics;
    64 sentinel floats behind (and 4 bytes before) each of w, m, v and 4 KiB behind the workspace untouched, g unchanged;
  * every tensor at base + 4 bytes (the 4-byte path) gives the bits of its 16-byte-aligned twin;
  * two calls from equal starts give the same bits; a group with a NaN in its gradient keeps every bit while the other one
    steps; the refusals return AIE_E_INVALID, name the function and write nothing;
  * one captured step replayed three times, with set_lr and new gradients between the replays, equals the eager sequence
    bit for bit, the step count and the statistics included;
  * end to end on a small gather-trade-build environment: three updates -- forward, the PPO loss, backward, Adam.step() --
    through autograd (.grad), through the direct calls, and captured in a graph agree bit for bit; the weights equal the
    CPU helpers fed the device's own gradients; the policy's next logits() sees them.
"""
import ctypes as C
import tempfile

import numpy as np
import pytest

import optim_ref as oref
import policy_mlp_bwd_ref as bref
from test_adam_cpu import LRS, HostGroup, build_adam_shim, c_step, same_stats
from test_gpu_policy_mlp_backward import _be, _dev, _fresh_logp_old, _ppo_operands

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
SENTINEL = 64
WS_GUARD = 512  # float64: 4 KiB
CHUNK = oref.CHUNK
SCALES = [1.0, 0.01, 1.0]  # gradient norms around max_norm = 0.5: clipped, not clipped, clipped


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as d:
        yield build_adam_shim(d)


class DevGroup:
    """A group of optim_ref's on the device: every operand in a NaN-filled buffer of its own with `lead` floats before it
    (lead = 1: every tensor starts 4 bytes behind a 16-byte boundary) and SENTINEL floats behind it; the C descriptor."""

    def __init__(self, G, lead=0):
        import torch

        from ai_economist_amd import _cabi

        self.n = [a.size for a in G["w"]]
        self.lead = lead
        self.buf = {k: [torch.full((n + lead + SENTINEL,), float("nan"), device=DEV) for n in self.n] for k in "wgmv"}
        self.t = {k: [b[lead: lead + n] for b, n in zip(self.buf[k], self.n)] for k in "wgmv"}
        for k in "wmv":
            for t, a in zip(self.t[k], G[k]):
                t.copy_(_dev(a))
        for t in self.t["g"]:
            t.zero_()
        assert all(t.data_ptr() % 16 == 4 * lead for k in "wgmv" for t in self.t[k])
        self.state = torch.zeros(4, dtype=torch.int64, device=DEV)
        self.stats = torch.full((4,), float("nan"), device=DEV)
        self.lr = torch.zeros(1, device=DEV)
        self.arr = (_cabi.AieOptTensor * len(self.n))(*[
            _cabi.AieOptTensor(*[self.t[k][i].data_ptr() for k in "wgmv"], self.n[i]) for i in range(len(self.n))])
        self.c = _cabi.AieOptGroup(tensors=self.arr, n_tensors=len(self.n), beta1=G["beta1"], beta2=G["beta2"], eps=G["eps"],
                                   max_norm=G["max_norm"], d_lr=self.lr.data_ptr(), d_state=self.state.data_ptr(),
                                   d_stats=self.stats.data_ptr())

    def set(self, grads, lr):
        for t, g in zip(self.t["g"], grads):
            t.copy_(_dev(np.asarray(g, f32)))
        self.lr.fill_(float(lr))

    def bits(self):
        """Everything a call may change, as int32 / int64 copies."""
        import torch

        return [t.clone().view(torch.int32) for k in "wmv" for t in self.t[k]] + [self.state.clone()]

    def guards_untouched(self):
        import torch

        return all(bool(torch.isnan(b[: self.lead]).all()) and bool(torch.isnan(b[self.lead + n:]).all())
                   for k in "wgmv" for b, n in zip(self.buf[k], self.n))


def _same(a, b):
    import torch

    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _call(be, da, dp, ws=None, short=0):
    """The C call with a NaN-filled workspace of the size the library asks for and WS_GUARD float64 behind it ->
    (return code, the workspace, the float64 words the call may use)."""
    import torch

    r = lambda d: None if d is None else C.byref(d.c)  # noqa: E731
    need = int(be.lib.aie_adam_workspace_bytes(be.handle, r(da), r(dp)))
    use = max(need, 0) // 8
    if ws is None:
        ws = torch.full((use + WS_GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    rc = be.lib.aie_adam_step(be.handle, r(da), r(dp), C.c_void_p(ws.data_ptr()), C.c_int64(need - short), be._stream())
    torch.cuda.synchronize()
    return rc, ws, use


def _hold(what, D, H, grads):
    """The device's group == the header's after the same step; nothing around the tensors was touched, g is the input."""
    for k in "wmv":
        for i, (t, a) in enumerate(zip(D.t[k], getattr(H, k))):
            got = t.cpu().numpy()
            bad = np.flatnonzero(~(got == a))
            assert bad.size == 0, "%s: %d of %d entries of %s[%d] differ, first at %d: got %r, want %r" % (
                what, bad.size, a.size, k, i, bad[0], got[bad[0]], a[bad[0]])
    assert (D.state.cpu().numpy() == H.state).all(), (what, D.state.cpu().numpy(), H.state)
    assert same_stats(D.stats.cpu().numpy(), H.stats), (what, D.stats.cpu().numpy(), H.stats)
    assert all((t.cpu().numpy().view(np.uint32) == np.asarray(g, f32).view(np.uint32)).all()  # (bits: a planted NaN too)
               for t, g in zip(D.t["g"], grads)), what + ": g modified"
    assert D.guards_untouched(), what + ": wrote outside a tensor"


SIXTEEN = oref.SIZES + [7, 64, 1000, 1025, 2048]


@pytest.mark.parametrize("which, sizes_a, sizes_p", [("both", oref.SIZES, oref.SIZES[:8]), ("agents", SIXTEEN, None),
                                                     ("planner", None, [2 * CHUNK + 17])], ids=["both", "agents16", "planner1"])
def test_device_equals_the_header(shim, which, sizes_a, sizes_p):
    import torch

    be = _be()
    G = [oref.new_group(s, seed=50 + c) if s else None for c, s in enumerate((sizes_a, sizes_p))]
    D = [DevGroup(g) if g else None for g in G]
    H = [HostGroup(g, LRS[0]) if g else None for g in G]
    clipped = set()
    for t, scale in enumerate(SCALES):
        grads = [oref.random_grads(s, 300 + 10 * t + c, scale) if s else None for c, s in enumerate((sizes_a, sizes_p))]
        for c in range(2):
            if G[c]:
                D[c].set(grads[c], LRS[t + 1])
                H[c].set(grads[c], LRS[t + 1])
        rc, ws, use = _call(be, D[0], D[1])
        assert rc == 0, be.lib.aie_last_error(be.handle)
        assert bool(torch.isnan(ws[use:]).all()), "wrote behind the workspace"
        assert not bool(torch.isnan(ws[:use]).any())  # (it is exactly as large as it needs to be)
        c_step(shim, H[0], H[1])
        for c in range(2):
            if G[c]:
                _hold("%s, group %d, step %d" % (which, c, t + 1), D[c], H[c], grads[c])
                assert H[c].stats[3] == 0 and H[c].stats[2] == t + 1
                clipped.add(bool(H[c].stats[1] < 1))
    assert clipped == {False, True}


def test_four_byte_alignment_gives_the_aligned_twins_bits(shim):
    be = _be()
    sizes = (oref.SIZES, [CHUNK + 1, 4, 2 * CHUNK + 17])
    G = [oref.new_group(s, seed=60 + c) for c, s in enumerate(sizes)]
    aligned, shifted = [DevGroup(g) for g in G], [DevGroup(g, lead=1) for g in G]
    H = [HostGroup(g, LRS[0]) for g in G]
    for t, scale in enumerate(SCALES):
        grads = [oref.random_grads(s, 400 + 10 * t + c, scale) for c, s in enumerate(sizes)]
        for pair in (aligned, shifted, H):
            for c in range(2):
                pair[c].set(grads[c], LRS[t])
        assert _call(be, aligned[0], aligned[1])[0] == 0 and _call(be, shifted[0], shifted[1])[0] == 0
        c_step(shim, H[0], H[1])
        for c in range(2):
            assert _same(aligned[c].bits(), shifted[c].bits()), "group %d, step %d: the 4-byte path differs" % (c, t + 1)
            _hold("shifted, group %d, step %d" % (c, t + 1), shifted[c], H[c], grads[c])
            assert aligned[c].guards_untouched()


def test_two_calls_the_same_bits_and_a_skipped_group_keeps_every_bit(shim):
    import torch

    be = _be()
    sizes = ([CHUNK + 1, 5, 256], [3, 2 * CHUNK + 17])
    G = [oref.new_group(s, seed=70 + c) for c, s in enumerate(sizes)]
    runs = [[DevGroup(g) for g in G] for _ in range(2)]
    H = [HostGroup(g, LRS[0]) for g in G]
    for t in range(3):
        grads = [oref.random_grads(s, 500 + 10 * t + c, 1.0) for c, s in enumerate(sizes)]
        if t == 1:
            grads[0][-1][-1] = np.nan  # the agents' group is skipped at the second step
        for pair in runs + [H]:
            for c in range(2):
                pair[c].set(grads[c], LRS[t])
        before = runs[0][0].bits()
        for pair in runs:
            assert _call(be, pair[0], pair[1])[0] == 0
        c_step(shim, H[0], H[1])
        for c in range(2):
            assert _same(runs[0][c].bits(), runs[1][c].bits()) and torch.equal(runs[0][c].stats.view(torch.int32),
                                                                              runs[1][c].stats.view(torch.int32))
            _hold("group %d, step %d" % (c, t + 1), runs[0][c], H[c], grads[c])
        skipped = float(runs[0][0].stats[3]) == 1.0
        assert skipped == (t == 1) and _same(before, runs[0][0].bits()) == skipped
        assert float(runs[0][1].stats[3]) == 0.0
    assert [int(d.state[0]) for d in runs[0]] == [2, 3]


def test_refusals_write_nothing():
    import torch

    from ai_economist_amd import _cabi

    be = _be()
    G = oref.new_group([5, CHUNK + 1], seed=80)
    grads = oref.random_grads([5, CHUNK + 1], 81, 1.0)

    def attempt(ws_fault=None, tensor=None, **override):
        d, other = DevGroup(G), DevGroup(G)
        d.set(grads, LRS[0]), other.set(grads, LRS[0])
        for k, val in override.items():
            setattr(d.c, k, val)
        if tensor:
            setattr(d.arr[1], *tensor)
        before = d.bits() + other.bits()
        if ws_fault is None:
            rc, ws, _ = _call(be, other, d)  # the good group first: nothing of it may run either
        else:
            need = int(be.lib.aie_adam_workspace_bytes(be.handle, C.byref(other.c), C.byref(d.c)))
            assert need == 8 * (2 * 4 + 2 * 3)
            ws = torch.full((need // 8 + WS_GUARD,), float("nan"), dtype=torch.float64, device=DEV)
            p, size = {"null": (None, need), "misaligned": (ws.data_ptr() + 4, need), "small": (ws.data_ptr(), need - 8)}[ws_fault]
            rc = be.lib.aie_adam_step(be.handle, C.byref(other.c), C.byref(d.c), C.c_void_p(p), C.c_int64(size), be._stream())
            torch.cuda.synchronize()
        clean = _same(before, d.bits() + other.bits()) and bool(torch.isnan(ws).all()) and bool(torch.isnan(d.stats).all()) \
            and bool(torch.isnan(other.stats).all()) and d.guards_untouched() and other.guards_untouched()
        return rc, clean

    rc, clean = attempt()
    assert rc == 0 and not clean  # (the call itself is a good one)
    for kw in (dict(n_tensors=0), dict(n_tensors=17), dict(beta1=1.0), dict(beta2=-0.5), dict(eps=0.0), dict(d_lr=None),
               dict(d_state=None), dict(d_stats=None), dict(tensor=("w", None)), dict(tensor=("g", None)), dict(tensor=("m", None)),
               dict(tensor=("v", None)), dict(tensor=("n", 0)), dict(ws_fault="null"), dict(ws_fault="misaligned"),
               dict(ws_fault="small")):
        rc, clean = attempt(**kw)
        assert (rc, clean) == (_cabi.E_INVALID, True), kw
        assert b"aie_adam_step" in be.lib.aie_last_error(be.handle), kw
    assert be.lib.aie_adam_step(be.handle, None, None, None, C.c_int64(0), be._stream()) == 0  # no group
    assert be.lib.aie_adam_workspace_bytes(be.handle, None, None) == 0
    with pytest.raises(ValueError):  # the operand check: never converted
        be.adam_group([(torch.zeros(4, device=DEV), torch.zeros(4, device=DEV, dtype=torch.float64), torch.zeros(4, device=DEV),
                        torch.zeros(4, device=DEV))], torch.zeros(1, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV),
                      torch.zeros(4, device=DEV))
    with pytest.raises(ValueError):
        be.adam_group([(torch.zeros(8, device=DEV)[::2],) * 4], torch.zeros(1, device=DEV),
                      torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, device=DEV))


def _adam_sequence(graphed, shim=None):
    """Three steps of rollout.Adam on lists of tensors, new gradients and a new learning rate before each -> the bits of
    everything after each step."""
    import torch

    from ai_economist_amd import rollout

    be = _be()
    sizes = ([CHUNK + 1, 5, 256, 1], [3, 2 * CHUNK + 17])
    G = [oref.new_group(s, seed=90 + c) for c, s in enumerate(sizes)]
    params = [[_dev(a) for a in g["w"]] for g in G]
    start = [[p.clone() for p in ps] for ps in params]
    gbuf = [[torch.zeros_like(p) for p in ps] for ps in params]
    opt = rollout.Adam(be, params[0], params[1], lr=float(LRS[0]), max_norm=0.5)
    H = [HostGroup(g, LRS[0]) for g in G] if shim else None

    def restart():
        for c in range(2):
            for p, s in zip(params[c], start[c]):
                p.copy_(s)
            for k in ("m", "v"):
                for t in opt.groups[c][k]:
                    t.zero_()
            opt.groups[c]["state"].zero_()

    graph = None
    if graphed:
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            opt.step(grads=gbuf)  # the warm-up
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        restart()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            opt.step(grads=gbuf)
        restart()  # (capture runs nothing; all the same)
    out = []
    for t, scale in enumerate(SCALES):
        grads = [oref.random_grads(s, 600 + 10 * t + c, scale) for c, s in enumerate(sizes)]
        for c in range(2):
            for b, g in zip(gbuf[c], grads[c]):
                b.copy_(_dev(g))
        opt.set_lr(float(LRS[t + 2]))
        graph.replay() if graphed else opt.step(grads=gbuf)
        torch.cuda.synchronize()
        out.append([x.clone().view(torch.int32) for c in range(2) for k in ("params", "m", "v") for x in opt.groups[c][k]]
                   + [opt.groups[c]["state"].clone() for c in range(2)] + [s.clone().view(torch.int32) for s in opt.stats()])
        assert [int(s) for s in opt.steps()] == [t + 1, t + 1]
        if shim:
            for c in range(2):
                H[c].set(grads[c], LRS[t + 2])
            c_step(shim, H[0], H[1])
            for c in range(2):
                for k, hk in (("params", "w"), ("m", "m"), ("v", "v")):
                    assert all((x.cpu().numpy() == a).all() for x, a in zip(opt.groups[c][k], getattr(H[c], hk))), (c, k, t)
                assert same_stats(opt.stats()[c].cpu().numpy(), H[c].stats)
    assert all(params[c][i].data_ptr() == opt.groups[c]["params"][i].data_ptr() for c in range(2) for i in range(len(params[c])))
    return out


def test_a_captured_step_replayed_equals_the_eager_sequence(shim):
    eager = _adam_sequence(False, shim)
    replayed = _adam_sequence(True)
    for t, (a, b) in enumerate(zip(eager, replayed)):
        assert _same(a, b), "step %d: replayed != eager" % (t + 1)


def _three_updates(mode, shim=None):
    """Three PPO updates of a small policy from one start.  mode "autograd": policy.evaluate, rollout.ppo_loss, backward(),
    Adam.step() on .grad; "direct": the backend's calls on fixed buffers, Adam.step(grads=); "graph": those captured once
    and replayed.  -> (the sixteen tensors' bits, both moments' and the states' bits, logits before, logits after)."""
    import torch

    from ai_economist_amd import rollout
    from ai_economist_amd.rollout import MaskedMLPPolicy

    B = 40
    be, WA, MP, stored = _ppo_operands(B, seed=33)
    pol = MaskedMLPPolicy(be, network="library", hidden=16, seed=3, value_head=True)
    before = [t.clone() for t in pol.logits(be.tensors)]
    FA, FP = pol.wa1.shape[0], pol.wp1.shape[0]
    dxa, dxp = _dev(bref.rows_with_zeros(B * be.n, FA, 71)), _dev(bref.rows_with_zeros(B, FP, 72))
    stored = _fresh_logp_old(be, pol, dxa, dxp, stored)
    weights = (pol.weights_a, pol.weights_p)
    opt = rollout.Adam(be, pol.weights_a, pol.weights_p, lr=1e-2, max_norm=0.05)
    start = [{k: v.clone() for k, v in w.items()} for w in weights]
    H = None
    if shim:
        G = [dict(oref.new_group([1], 0, max_norm=0.05), w=[v.cpu().numpy().reshape(-1) for v in w.values()],
                  m=[np.zeros(v.numel(), f32) for v in w.values()], v=[np.zeros(v.numel(), f32) for v in w.values()]) for w in weights]
        H = [HostGroup(g, f32(1e-2)) for g in G]

    def restart():
        for c, w in enumerate(weights):
            for k in w:
                w[k].copy_(start[c][k])
            for k in ("m", "v"):
                for t in opt.groups[c][k]:
                    t.zero_()
            opt.groups[c]["state"].zero_()

    if mode == "autograd":
        leaves = [getattr(pol, "%s%s%s" % (k[0], who, k[1])) for who in "ap" for k in bref.NAMES]
        for t in leaves:
            t.requires_grad_(True)
        for _ in range(3):
            for t in leaves:
                t.grad = None
            la, lp, va, vp = pol.evaluate(dxa, dxp)
            loss_a, loss_p, _, _ = rollout.ppo_loss(be, la, lp, va, vp, stored)
            (loss_a + loss_p).backward()
            opt.step()
        for t in leaves:
            t.requires_grad_(False)
    else:
        f = dict(dtype=torch.float32, device=DEV)
        net = (torch.empty((B * be.n, WA), **f), torch.empty((B, MP), **f), torch.empty(B * be.n, **f), torch.empty(B, **f))
        loss = tuple((torch.empty(8, **f), torch.empty_like(lg), torch.empty_like(v)) for lg, v in ((net[0], net[2]), (net[1], net[3])))
        grads = tuple({k: torch.empty_like(v) for k, v in w.items()} for w in weights)

        def update():
            be.policy_mlp_forward(dxa, dxp, pol.weights_a, pol.weights_p, out=net)
            be.ppo_loss(net[0], net[1], net[2], net[3], stored, out=loss)
            be.policy_mlp_backward(dxa, dxp, pol.weights_a, pol.weights_p, loss[0][1], loss[1][1], loss[0][2], loss[1][2], out=grads)
            opt.step(grads=grads)

        if mode == "graph":
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
            for _ in range(3):
                graph.replay()
        else:
            for _ in range(3):
                update()
                if H:  # the CPU helpers, fed the device's own gradients
                    torch.cuda.synchronize()
                    for c in range(2):
                        H[c].set([grads[c][k].cpu().numpy().reshape(-1) for k in weights[c]], f32(1e-2))
                    c_step(shim, H[0], H[1])
                    for c in range(2):
                        for k, a in zip(weights[c], H[c].w):
                            assert (weights[c][k].cpu().numpy().reshape(-1) == a).all(), "class %d, %s: != the helpers" % (c, k)
                        assert same_stats(opt.stats()[c].cpu().numpy(), H[c].stats)
    torch.cuda.synchronize()
    after = [t.clone() for t in pol.logits(be.tensors)]
    torch.cuda.synchronize()
    bits = [v.clone().view(-1).view(torch.int32) for w in weights for v in w.values()]
    more = [x.clone().view(torch.int32) for c in range(2) for k in ("m", "v") for x in opt.groups[c][k]] \
        + [opt.groups[c]["state"].clone() for c in range(2)]
    moved = all(not torch.equal(w[k], s[k]) for w, s in zip(weights, start) for k in w)
    print(mode, "stats:", [s.cpu().numpy().tolist() for s in opt.stats()])
    return bits, more, before, after, moved


def test_three_updates_end_to_end(shim):
    import torch

    direct, more_d, before, after, moved = _three_updates("direct", shim)
    assert len(direct) == 16 and moved, "an update left a weight tensor where it was"
    assert not torch.equal(before[0], after[0]) and not torch.equal(before[1], after[1])
    assert all(bool(torch.isfinite(t).all()) for t in after)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))  # noqa: E731
    for mode in ("graph", "autograd"):
        bits, more, before_m, after_m, _ = _three_updates(mode)
        assert _same(direct, bits) and _same(more_d, more), mode + " != direct"
        assert all(same(a, b) for a, b in zip(before, before_m)) and all(same(a, b) for a, b in zip(after, after_m)), mode
