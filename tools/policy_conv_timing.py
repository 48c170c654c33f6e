#!/usr/bin/env python
"""The agents' convolutional encoder in front of the policy network -- forward, and a whole PPO update -- the library's
launches against the torch formulation, at C2's shapes with 4096 batch elements (16 384 agent rows: the 7 x 11 x 11 map crop
and the 2 x 11 x 11 index crop through an embedding of 4 over 100 entries and two 3x3 stride-2 convolutions to 128 features,
then 128 + 136 -> 128 -> 128 -> 50 + 1; 4096 planner rows through 86 -> 128 -> 128 -> 154 + 1).

   python tools/policy_conv_timing.py [output directory, default profiles/]        (GPU only)

One child process takes a rollout's operands from a C2 environment (the crops, the flat observations, masks, sampled actions
and their logp, the policy's values; random advantages and returns) and builds, as captured graphs on the same weights:
  library   forward:  policy_conv_forward, policy_mlp_forward (two launches)
            update:   the forward, ppo_loss, policy_mlp_backward, policy_mlp_input_grad, policy_conv_backward, one in-place
                      SGD step (_foreach_add_)
  torch     forward:  embedding, cat, two conv2d(stride=2) with relu, flatten, cat, the addmm / relu network
            update:   that forward, rollout.ppo_loss (the library's loss in both), autograd.grad, the same SGD step
and times each -- device events around REPLAYS replays behind WARMUP warm-up replays -- in ROUNDS alternating rounds, so that
both see the same machine; it prints the median and the extremes over the rounds.  The parent runs that child once plainly
(the timings of record) and once more under rocprofv3 --kernel-trace --stats for the per-kernel times.
Writes policy_conv_timing.txt and policy_conv_kernel_stats.csv."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAYS, WARMUP, ROUNDS = 50, 5, 7
LR = 1e-7  # (the weights barely move over the run: every replay does the same work)

if len(sys.argv) > 1 and sys.argv[1] == "child":
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import torch
    import torch.nn.functional as Fn

    import bench
    from ai_economist_amd import rollout
    from ai_economist_amd.rollout import MaskedMLPPolicy
    from helpers import make_env

    E = 4096
    env = make_env(dict(bench.C2_CFG), n_envs=E, device="cuda:0")
    env.seed(1)
    env.reset()
    be = env.backend
    dev = be.device
    pol = MaskedMLPPolicy(be, hidden=128, record_logp=True, value_head=True, network="library", spatial=True)
    a, p = be._action_buffers(0)
    for _ in range(5):  # a few steps in
        pol(be.tensors, a, p)
        be.step(a, p)
    pol(be.tensors, a, p)
    torch.cuda.synchronize()
    t = be.tensors
    cm, ci = t["obs_a_world-map"].clone(), t["obs_a_world-idx_map"].clone()
    xf, xp = t["obs_a_flat"].clone(), t["obs_p_flat"].clone()
    rows, NF = E * be.n, pol.NF
    ma, mp = be.action_masks()
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    batch = dict(masks_a=ma.clone().contiguous(), masks_p=mp.clone().contiguous(), actions_a=a.clone(), actions_p=p.clone(),
                 logp_old_a=pol.logp_a.clone(), logp_old_p=pol.logp_p.clone(), adv_a=rnd(E, be.n), adv_p=rnd(E),
                 values_old_a=pol.value_a.clone(), values_old_p=pol.value_p.clone(), returns_a=rnd(E, be.n), returns_p=rnd(E))
    f = dict(dtype=torch.float32, device=dev)
    wa, wp, wc = pol.weights_a, pol.weights_p, pol.conv_weights
    flat_w = list(wa.values()) + list(wp.values()) + list(wc.values())
    x_cat = torch.empty((rows, pol.wa1.shape[0]), **f)
    net = (torch.empty((rows, pol.MA), **f), torch.empty((E, pol.MP), **f), torch.empty(rows, **f), torch.empty(E, **f))
    loss = tuple((torch.empty(8, **f), torch.empty_like(lg), torch.empty_like(v)) for lg, v in ((net[0], net[2]), (net[1], net[3])))
    grads = tuple({k: torch.empty_like(v) for k, v in w.items()} for w in (wa, wp, wc))
    flat_g = [v for d in grads for v in d.values()]
    g_x = torch.empty((rows, NF), **f)

    def lib_forward():
        be.policy_conv_forward(cm, ci, xf, wc, out=x_cat)
        be.policy_mlp_forward(x_cat, xp, wa, wp, out=net)

    def lib_backward():
        be.policy_mlp_backward(x_cat, xp, wa, wp, loss[0][1], loss[1][1], loss[0][2], loss[1][2], out=grads[:2])
        be.policy_mlp_input_grad(ncols_a=NF, out=(g_x, None))
        be.policy_conv_backward(cm, ci, wc, g_x, out=grads[2])

    def lib_update():
        lib_forward()
        be.ppo_loss(net[0], net[1], net[2], net[3], batch, out=loss)
        lib_backward()
        torch._foreach_add_(flat_w, flat_g, alpha=-LR)

    lib_update()
    torch.cuda.synchronize()
    tw = [w.clone().requires_grad_(True) for w in flat_w]  # the torch network's own copies
    ta = dict(zip(wa, tw[:len(wa)]))
    tp = dict(zip(wp, tw[len(wa):len(wa) + len(wp)]))
    tc = dict(zip(wc, tw[len(wa) + len(wp):]))
    C_map, h, w_ = (int(v) for v in cm.shape[-3:])
    D, V = int(wc["emb"].shape[1]), int(wc["emb"].shape[0])
    C = C_map + 2 * D
    cmr, cir, xfr = cm.reshape(rows, C_map, h, w_), ci.reshape(rows, 2, h, w_).long().clamp_(0, V - 1), xf.reshape(rows, -1)

    def torch_forward():
        e = Fn.embedding(cir, tc["emb"]).permute(0, 1, 4, 2, 3).reshape(rows, 2 * D, h, w_)
        x = torch.cat([cmr, e], 1)
        k1 = tc["w1"].view(3, 3, C, 16).permute(3, 2, 0, 1)
        k2 = tc["w2"].view(3, 3, 16, 32).permute(3, 2, 0, 1)
        a1 = Fn.conv2d(x, k1, tc["b1"], stride=2).relu()
        a2 = Fn.conv2d(a1, k2, tc["b2"], stride=2).relu()
        xa = torch.cat([a2.permute(0, 2, 3, 1).reshape(rows, -1), xfr], 1)
        out = []
        for x, w in ((xa, ta), (xp, tp)):
            hh = torch.addmm(w["b1"], x, w["w1"]).relu()
            hh = torch.addmm(w["b2"], hh, w["w2"]).relu()
            out.append((torch.addmm(w["b3"], hh, w["w3"]), torch.addmv(w["bv"], hh, w["wv"])))
        return out[0][0], out[1][0], out[0][1], out[1][1]

    def torch_update():
        la, lp, va, vp = torch_forward()
        loss_a, loss_p, _, _ = rollout.ppo_loss(be, la, lp, va, vp, batch)
        gs = torch.autograd.grad(loss_a + loss_p, tw)
        with torch.no_grad():
            torch._foreach_add_(tw, list(gs), alpha=-LR)
        return gs

    def torch_forward_only():
        with torch.no_grad():
            return torch_forward()

    def capture(fn):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            keep = fn()
        return graph, keep

    # the two formulations agree (float32 sums in different orders)
    lib_forward()
    got = torch_forward_only()
    torch.cuda.synchronize()
    worst = max(float((a_ - b_.view(a_.shape)).abs().max() / (a_.abs().max() + 1e-30)) for a_, b_ in zip(got, net))
    print("largest difference between torch's and the library's outputs, relative to the tensor's largest entry: %.2e" % worst, flush=True)
    cases = [("library", "forward", capture(lib_forward)), ("library", "update", capture(lib_update)),
             ("torch", "forward", capture(torch_forward_only)), ("torch", "update", capture(torch_update))]

    def timed(graph):
        for _ in range(WARMUP):
            graph.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / REPLAYS  # us per replay

    res = {}
    for _ in range(ROUNDS):
        for who, what, (graph, _) in cases:
            res.setdefault((what, who), []).append(timed(graph))
    med = {}
    for (what, who), ts in sorted(res.items()):
        ts = sorted(ts)
        med[(what, who)] = ts[len(ts) // 2]
        print("%-8s %-8s median %8.1f us per replay (min %.1f, max %.1f over %d rounds of %d replays; device events)"
              % (what, who, ts[len(ts) // 2], ts[0], ts[-1], ROUNDS, REPLAYS), flush=True)
    for what in ("forward", "update"):
        print("%s: library / torch = %.2f (device events)" % (what, med[(what, "library")] / med[(what, "torch")]), flush=True)
else:
    import csv
    import glob
    import shutil
    import tempfile

    dest = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(dest, exist_ok=True)
    child = [sys.executable, os.path.abspath(__file__), "child"]
    plain = subprocess.run(child, timeout=400, cwd=tempfile.gettempdir(), capture_output=True, text=True)
    lines = [ln for ln in plain.stdout.splitlines() if "device events" in ln or "largest difference" in ln]
    if plain.returncode != 0 or not lines:
        sys.stderr.write(plain.stdout[-3000:] + plain.stderr[-3000:])
        sys.exit(plain.returncode or 1)
    out = os.path.join(tempfile.gettempdir(), "policy_conv_timing_prof")
    shutil.rmtree(out, ignore_errors=True)
    run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "p", "--"] + child,
                         timeout=400, cwd=tempfile.gettempdir(), capture_output=True, text=True)
    stats = glob.glob(out + "/**/*kernel_stats.csv", recursive=True)
    if run.returncode != 0 or not stats:
        sys.stderr.write(run.stdout[-3000:] + run.stderr[-3000:])
        sys.exit(run.returncode or 1)
    shutil.copy(stats[0], os.path.join(dest, "policy_conv_kernel_stats.csv"))
    ours, other = [], []
    for r in csv.DictReader(open(stats[0])):
        row = "%-64s average %8.2f us (min %.2f, max %.2f) over %s launches" % (
            r["Name"].split("(")[0][:64], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, r["Calls"])
        if "aie_policy" in r["Name"] or "aie_ppo" in r["Name"]:
            ours.append(row)
        elif int(r["Calls"]) >= ROUNDS * REPLAYS:  # the torch network's kernels: every replay of a graph
            other.append(row)
    report = ["C2's shapes, 4096 batch elements: 16 384 agent rows, crop 7 + 2 x 4 channels on 11 x 11 -> 5 x 5 x 16 -> 2 x 2 x 32 = 128",
              "features, then 264 -> 128 -> 128 -> 50 + 1; 4096 planner rows 86 -> 128 -> 128 -> 154 + 1; float32; captured graphs,",
              "%d rounds alternating the cases" % ROUNDS, "", "event to event (profiler off):"] + lines + [
        "", "kernel time by name (a second run of the same script under rocprofv3 --kernel-trace --stats):",
        "the library's kernels:"] + sorted(ours) + ["", "every other kernel launched by each replay (torch):"] + sorted(other)
    with open(os.path.join(dest, "policy_conv_timing.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
