"""aie_policy_mlp_forward on the device (Backend.policy_mlp_forward, rollout.MaskedMLPPolicy(network="library"),
rollout.mlp_weights) against the header's helper compiled on the CPU (tests/test_policy_mlp_cpu.py holds it to an
independent transcription):

  * values: the shapes of policy_mlp_ref.SHAPES and EDGE_SHAPES (the widths at which the kernel's loops take another shape:
    an odd number of k-step groups, a tail of four steps, waves without an output tile, the value column alone in a tile,
    F at the staged chunk's edge) as the planner class at 1 .. 130 rows (either row tile meets its
    edge) with another shape as the agents' class in the same launch, each class alone, the value column on and off --
    float == with no NaN anywhere, every entry in range written (the buffers start as NaN), 64 sentinel rows behind them
    untouched; COVID's 51 agents give the agents' class row counts that are no multiple of 4;
  * a leading dimension larger than F and an address that is only 8-byte aligned equal the contiguous copy; F beyond one
    staged chunk;
  * the refusals return the header's codes and write nothing;
  * the policy path at C2: library and torch networks of one seed inside the derived bound around the float64 pass,
    the picks and logp are the sampler's on the policy's own logits buffers, 20 graph replays with a trajectory equal 20
    eager iterations, and a second pair of runs repeats the first's bits;
  * an in-place weight update between two replays of a captured policy is seen by the second.
"""
import ctypes as C
import tempfile

import numpy as np
import pytest

import policy_mlp_ref as ref
from helpers import make_env
from test_gpu_policy_evaluate import C2, _cfg
from test_policy_mlp_cpu import build_shim, c_forward

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
ROWS = [1, 3, 31, 32, 33, 63, 64, 65, 130]
SENTINEL = 64
_ENVS = {}


@pytest.fixture(scope="module")
def shim():
    with tempfile.TemporaryDirectory() as d:
        yield build_shim(d)


def _be(case="gtb_c2"):
    if case not in _ENVS:
        env = make_env(_cfg(case), n_envs={"gtb_c2": 5, "covid": 1}[case], device=DEV)
        if case != "covid":
            env.seed(3)
        env.reset()
        _ENVS[case] = env
    return _ENVS[case].backend


def _dev(a):
    import torch

    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _weights(W):
    return {k: _dev(v) for k, v in W.items()}


def _outputs(rows, M, value):
    """NaN-filled (logits, values) with SENTINEL rows behind the `rows` the call may write."""
    import torch

    lg = torch.full((rows + SENTINEL, M), float("nan"), device=DEV)
    v = torch.full((rows + SENTINEL,), float("nan"), device=DEV) if value else None
    return lg, v


def _hold(shim, what, x, W, lg, v, rows):
    """The device's outputs == the header's; nothing behind them was touched."""
    want_l, want_v = c_forward(shim, x, W)
    assert not np.isnan(want_l).any()
    got = lg.cpu().numpy()
    assert not np.isnan(got[:rows]).any(), "%s: %d logits not written (or NaN)" % (what, np.isnan(got[:rows]).sum())
    bad = np.argwhere(got[:rows] != want_l)
    assert bad.size == 0, "%s: %d of %d logits differ, first at %s: got %r, want %r" % (
        what, len(bad), want_l.size, bad[0], got[tuple(bad[0])], want_l[tuple(bad[0])])
    assert np.isnan(got[rows:]).all(), "%s: wrote behind the logits" % what
    assert (v is None) == (want_v is None)
    if v is not None:
        gv = v.cpu().numpy()
        assert not np.isnan(gv[:rows]).any() and (gv[:rows] == want_v).all(), "%s: values differ" % what
        assert np.isnan(gv[rows:]).all(), "%s: wrote behind the values" % what


ALL_SHAPES = ref.SHAPES + ref.EDGE_SHAPES  # (the edge shapes: the widths the kernel's loops branch on)


def _pair(si):
    """The planner's shape and the agents': the next one of the same list."""
    group = ref.SHAPES if si < len(ref.SHAPES) else ref.EDGE_SHAPES
    return ALL_SHAPES[si], group[(group.index(ALL_SHAPES[si]) + 1) % len(group)]


@pytest.mark.parametrize("value", [True, False], ids=["value", "novalue"])
@pytest.mark.parametrize("si", range(len(ALL_SHAPES)), ids=["%dx%dx%d" % s for s in ALL_SHAPES])
def test_device_equals_the_header(shim, si, value):
    import torch

    be = _be()
    n = be.n
    (Fp, Hp, Mp), (Fa, Ha, Ma) = _pair(si)  # the agents' class: another shape in the same launch
    Wp = ref.random_weights(Fp, Hp, Mp, seed=100 + si, value=value)
    Wa = ref.random_weights(Fa, Ha, Ma, seed=200 + si, value=not value)  # (and the other choice of the value column)
    dWp, dWa = _weights(Wp), _weights(Wa)
    for B in ROWS:
        xp, xa = ref.random_rows(B, Fp, seed=B + si), ref.random_rows(B * n, Fa, seed=3 * B + si)
        dxp, dxa = _dev(xp), _dev(xa)
        for which in ("both", "planner", "agents"):
            la, va = _outputs(B * n, Ma, not value)
            lp, vp = _outputs(B, Mp, value)
            use_a, use_p = which != "planner", which != "agents"
            out = (la[: B * n] if use_a else None, lp[:B] if use_p else None,
                   va[: B * n] if use_a and va is not None else None, vp[:B] if use_p and vp is not None else None)
            got = be.policy_mlp_forward(dxa if use_a else None, dxp if use_p else None, dWa, dWp, out=out)
            torch.cuda.synchronize()
            assert all((g is None and o is None) or g is o for g, o in zip(got, out))
            what = "%s rows %d (%s)" % (ALL_SHAPES[si], B, which)
            if use_p:
                _hold(shim, "planner " + what, xp, Wp, lp, vp, B)
            else:
                assert bool(torch.isnan(lp).all())
            if use_a:
                _hold(shim, "agents " + what, xa, Wa, la, va, B * n)
            else:
                assert bool(torch.isnan(la).all())


def test_agent_rows_that_are_no_multiple_of_four(shim):
    """COVID's 51 agents: 51 and 153 rows in the agents' class."""
    import torch

    be = _be("covid")
    assert be.n == 51
    F, H, M = ref.SHAPES[0]
    W = ref.random_weights(F, H, M, seed=9, value=True)
    dW = _weights(W)
    for B in (1, 3):
        x = ref.random_rows(B * be.n, F, seed=40 + B)
        lg, v = _outputs(B * be.n, M, True)
        be.policy_mlp_forward(_dev(x).view(B, be.n, F), None, dW, None, out=(lg[: B * be.n], None, v[: B * be.n], None))
        torch.cuda.synchronize()
        _hold(shim, "covid agents, B = %d" % B, x, W, lg, v, B * be.n)


def test_leading_dimension_alignment_and_chunks(shim):
    import torch

    be = _be()
    F, H, M = 86, 128, 154
    W = ref.random_weights(F, H, M, seed=17, value=True)
    dW = _weights(W)
    rows = 37
    x = ref.random_rows(rows, F, seed=18)
    big = torch.full((rows, F + 9), float("nan"), device=DEV)  # rows of 380 bytes; the view starts 8 bytes into them
    big[:, 2: 2 + F] = _dev(x)
    view = big[:, 2: 2 + F]
    assert view.stride(0) == F + 9 and view.data_ptr() % 16 == 8
    lg, v = _outputs(rows, M, True)
    be.policy_mlp_forward(None, view, None, dW, out=(None, lg[:rows], None, v[:rows]))
    _, lc, _, vc = be.policy_mlp_forward(None, view.contiguous(), None, dW)
    torch.cuda.synchronize()
    assert torch.equal(lg[:rows].view(torch.int32), lc.view(torch.int32)) and torch.equal(v[:rows].view(torch.int32), vc.view(torch.int32))
    _hold(shim, "x_ld > F", x, W, lg, v, rows)
    # the arena's own planner observations: rows of 344 bytes
    xp = be.tensors["obs_p_flat"]
    Wp = ref.random_weights(int(xp.shape[-1]), 32, 5, seed=19, value=False)
    lg, _ = _outputs(be.E, 5, False)
    be.policy_mlp_forward(None, xp, None, _weights(Wp), out=(None, lg[: be.E], None, None))
    torch.cuda.synchronize()
    _hold(shim, "obs_p_flat", xp.cpu().numpy(), Wp, lg, None, be.E)
    # F beyond one staged chunk (256 columns), and beyond two; two column groups per wave (H = 256)
    for F, H, M in ((300, 32, 5), (515, 256, 9)):
        W = ref.random_weights(F, H, M, seed=F, value=True)
        x = ref.random_rows(35, F, seed=F + 1)
        lg, v = _outputs(35, M, True)
        be.policy_mlp_forward(None, _dev(x), None, _weights(W), out=(None, lg[:35], None, v[:35]))
        torch.cuda.synchronize()
        _hold(shim, "F = %d" % F, x, W, lg, v, 35)


def test_refusals_write_nothing():
    import torch

    from ai_economist_amd import _cabi

    be = _be()
    B = 3

    def call(F, H, M, value=True, values_out=True, **override):
        t = {k: torch.zeros(s, device=DEV) for k, s in (("w1", (max(F, 1), H)), ("b1", (H,)), ("w2", (H, H)), ("b2", (H,)),
                                                          ("w3", (H, M)), ("b3", (M,)), ("wv", (H,)), ("bv", (1,)))}
        x = torch.ones((B, max(F, 1)), device=DEV)
        lg, v = _outputs(B, M, True)
        p = lambda k: t[k].data_ptr()  # noqa: E731
        c = _cabi.AieMlpClass(x=x.data_ptr(), x_ld=max(F, 1), w1=p("w1"), b1=p("b1"), w2=p("w2"), b2=p("b2"), w3=p("w3"), b3=p("b3"),
                              wv=p("wv") if value else None, bv=p("bv") if value else None, logits=lg.data_ptr(),
                              values=v.data_ptr() if values_out else None, F=F, H=H, M=M)
        for k, val in override.items():
            setattr(c, k, val)
        rc = be.lib.aie_policy_mlp_forward(be.handle, C.c_int64(B), None, C.byref(c), be._stream())
        torch.cuda.synchronize()
        return rc, bool(torch.isnan(lg).all()) and bool(torch.isnan(v).all())

    assert call(8, 32, 5) == (0, False)  # (the call itself is a good one)
    for kw, code in ((dict(F=8, H=24, M=5), _cabi.E_UNSUPPORTED), (dict(F=8, H=272, M=5), _cabi.E_UNSUPPORTED),
                     (dict(F=8, H=8, M=5), _cabi.E_UNSUPPORTED), (dict(F=0, H=32, M=5), _cabi.E_INVALID),
                     (dict(F=8, H=32, M=1025), _cabi.E_INVALID), (dict(F=8, H=32, M=5, value=False), _cabi.E_INVALID),
                     (dict(F=8, H=32, M=5, values_out=False), _cabi.E_INVALID), (dict(F=8, H=32, M=5, x_ld=7), _cabi.E_INVALID),
                     (dict(F=8, H=32, M=5, w2=None), _cabi.E_INVALID)):
        assert call(**kw) == (code, True), kw
    assert b"aie_policy_mlp_forward" in be.lib.aie_last_error(be.handle)
    c = _cabi.AieMlpClass()
    assert be.lib.aie_policy_mlp_forward(be.handle, C.c_int64(0), None, C.byref(c), be._stream()) == _cabi.E_INVALID  # B < 1
    assert be.lib.aie_policy_mlp_forward(be.handle, C.c_int64(4), None, None, be._stream()) == 0  # no class: nothing to do


def _policies(E, seed, episode_length=1000):
    from ai_economist_amd.rollout import MaskedMLPPolicy

    env = make_env(dict(C2, episode_length=episode_length), n_envs=E, device=DEV)
    env.seed(seed)
    env.reset()
    kw = dict(seed=3, record_logp=True, value_head=True)
    return env, MaskedMLPPolicy(env.backend, network="library", **kw), MaskedMLPPolicy(env.backend, **kw)


def _policy_weights(pol, who):
    W = {k: getattr(pol, "w%s%s" % (who, k[1])).cpu().numpy() for k in ("w1", "w2", "w3")}
    W.update({k: getattr(pol, "b%s%s" % (who, k[1])).cpu().numpy() for k in ("b1", "b2", "b3")})
    W["wv"] = getattr(pol, "w%sv" % who).cpu().numpy().reshape(-1)
    W["bv"] = getattr(pol, "b%sv" % who).cpu().numpy()
    return W


def test_policy_path_networks_agree_and_the_picks_are_the_samplers(shim):
    import torch

    from ai_economist_amd.rollout import MaskedMLPPolicy

    env, lib, tor = _policies(5, seed=4)
    be = env.backend
    with pytest.raises(ValueError):
        MaskedMLPPolicy(be, network="library", dtype=torch.bfloat16)
    a, p = be._action_buffers(0)
    for _ in range(3):  # a few steps in: the observations are no longer the reset's
        lib(be.tensors, a, p)
        be.step(a, p)
    t = be.tensors
    kept_t = t["sample_t"].clone()
    lib(t, a, p)
    picks = (a.clone(), p.clone(), lib.logp_a.clone(), lib.logp_p.clone())
    la_t, lp_t = tor.logits(t)
    torch.cuda.synchronize()
    for who, x, lg_l, lg_t, v_l, v_t in (("a", t["obs_a_flat"].reshape(-1, t["obs_a_flat"].shape[-1]), lib.logits_a, la_t, lib.value_a, tor.value_a),
                                         ("p", t["obs_p_flat"], lib.logits_p, lp_t, lib.value_p, tor.value_p)):
        W = _policy_weights(lib, who)
        assert all(torch.equal(getattr(lib, k), getattr(tor, k)) for k in ("w%s1" % who, "w%s3" % who, "w%sv" % who))
        xn = x.cpu().numpy()
        lg64, v64, blg, bv = ref.forward_f64(xn, W)
        for name, net_l, net_v in (("library", lg_l, v_l), ("torch", lg_t, v_t)):
            el = np.abs(net_l.cpu().numpy().astype(np.float64).reshape(lg64.shape) - lg64)
            ev = np.abs(net_v.cpu().numpy().astype(np.float64).reshape(-1) - v64)
            print("%s, class %s: max error / bound %.4f (logits) %.4f (values)" % (name, who, (el / blg).max(), (ev / bv).max()))
            assert (el <= blg).all() and (ev <= bv).all(), (name, who)
        # ... and the library's network is the header's, value for value
        want_l, want_v = c_forward(shim, xn, W)
        assert (lg_l.cpu().numpy() == want_l).all() and (v_l.cpu().numpy().reshape(-1) == want_v).all()
    # the picks: the sampler's, on the policy's own logits buffers and the same draw index
    t["sample_t"].copy_(kept_t)
    a2, p2, ga, gp = be.sample_policy_actions(lib.logits_a, lib.logits_p, lib.sample_seed, logp=True)
    torch.cuda.synchronize()
    assert torch.equal(a2.view(picks[0].shape), picks[0]) and torch.equal(p2.view(picks[1].shape), picks[1])
    assert torch.equal(ga.view(torch.int32).view(picks[2].shape), picks[2].view(torch.int32))
    assert torch.equal(gp.view(torch.int32).view(picks[3].shape), picks[3].view(torch.int32))
    assert bool(picks[2].ne(0).any())


def _rollout(graphed, N, T):
    """N iterations of policy -> store -> step from a fresh C2 environment, replayed or eager -> what the trajectory holds."""
    import torch

    from ai_economist_amd.rollout import GraphedStep, Trajectory

    WARM = 3
    env, pol, _ = _policies(6, seed=5, episode_length=7)  # (auto-resets inside the run)
    be = env.backend
    traj = Trajectory(env, T)
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
    f = traj.flat()
    out = {k: f[k].contiguous().view(torch.int32).cpu() for k in ("actions_a", "actions_p", "logp_a", "logp_p", "values_a", "values_p")}
    out["log"] = traj.log.view(torch.int32).cpu()  # rewards and done
    assert bool(f["values_a"].ne(0).all()) and bool(traj.log[..., -1].any())
    return out


def test_graphed_rollout_equals_eager_and_repeats():
    import torch

    N = T = 20
    first = (_rollout(True, N, T), _rollout(False, N, T))
    for k in first[0]:
        assert torch.equal(first[0][k], first[1][k]), "replayed != eager: " + k
    second = (_rollout(True, N, T), _rollout(False, N, T))
    for run, again in zip(first, second):
        for k in run:
            assert torch.equal(run[k], again[k]), "a second run differs: " + k


def test_in_place_weight_update_is_seen_by_the_next_replay(shim):
    import torch

    env, pol, _ = _policies(5, seed=6)
    be = env.backend
    t = be.tensors
    side = torch.cuda.Stream(device=be.device)
    side.wait_stream(torch.cuda.current_stream(be.device))
    with torch.cuda.stream(side):
        pol.logits(t)
    torch.cuda.current_stream(be.device).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pol.logits(t)
    xa = t["obs_a_flat"].reshape(-1, t["obs_a_flat"].shape[-1]).cpu().numpy()
    for scale in (None, 0.5):
        if scale is not None:
            pol.wa3.mul_(scale)  # what an optimizer step does: in place
        pol.logits_a.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        W = _policy_weights(pol, "a")
        want_l, want_v = c_forward(shim, xa, W)
        assert (pol.logits_a.cpu().numpy() == want_l).all(), "scale %s" % scale
        assert (pol.value_a.cpu().numpy().reshape(-1) == want_v).all()
    assert np.abs(want_l).max() > 0


def test_mlp_weights_from_linear_layers(shim):
    import torch

    from ai_economist_amd.rollout import mlp_weights

    be = _be()
    torch.manual_seed(0)
    F, H, M = 13, 32, 6
    layers = [torch.nn.Linear(F, H), torch.nn.Linear(H, H), torch.nn.Linear(H, M), torch.nn.Linear(H, 1)]
    layers = [m.to(DEV) for m in layers]
    w = mlp_weights(*layers)
    x = ref.random_rows(9, F, seed=2, planted=False)
    for step in range(2):
        if step:
            with torch.no_grad():
                for m in layers:
                    m.weight.mul_(0.75)
                    m.bias.add_(0.125)
            kept = w.w1.data_ptr()
            assert w.refresh() is w and w.w1.data_ptr() == kept
        _, lg, _, v = be.policy_mlp_forward(None, _dev(x), None, w)
        torch.cuda.synchronize()
        W = {"w%d" % (i + 1): m.weight.detach().t().cpu().numpy() for i, m in enumerate(layers[:3])}
        W.update({"b%d" % (i + 1): m.bias.detach().cpu().numpy() for i, m in enumerate(layers[:3])})
        W["wv"], W["bv"] = layers[3].weight.detach().cpu().numpy().reshape(-1), layers[3].bias.detach().cpu().numpy()
        want_l, want_v = c_forward(shim, x, W)
        assert (lg.cpu().numpy() == want_l).all() and (v.cpu().numpy() == want_v).all()
