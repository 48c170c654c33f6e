#!/usr/bin/env python
"""The policy network's backward pass and a whole PPO update, torch autograd against the library's three launches, at C2's
shapes with 4096 batch elements (16 384 agent rows through 136 -> 128 -> 128 -> 50 + 1, 4096 planner rows through
86 -> 128 -> 128 -> 154 + 1).

   python tools/policy_mlp_backward_timing.py [output directory, default profiles/]        (GPU only)

One child process takes a rollout's operands from a C2 environment (observations, masks, sampled actions and their logp,
the policy's values; random advantages and returns) and builds, as captured graphs on the same weights:
  library   forward + backward:  policy_mlp_forward, policy_mlp_backward on ppo_loss's stored gradients
            backward alone:      policy_mlp_backward (three launches)
            update:              policy_mlp_forward, ppo_loss, policy_mlp_backward, one in-place SGD step (_foreach_add_)
  torch     forward alone, forward + backward (autograd.grad of the addmm / relu network on the same gradients; a backward
            cannot be captured without its forward, so "backward" is the difference of the two), and the update: the torch
            network, rollout.ppo_loss (the library's loss in both), autograd.grad, the same SGD step
and times each -- device events around REPLAYS replays behind WARMUP warm-up replays -- in ROUNDS alternating rounds, so
that both see the same machine; it prints the median and the extremes over the rounds.  The parent runs that child once
plainly (the timings of record) and once more under rocprofv3 --kernel-trace --stats for the per-kernel times.
Writes policy_mlp_backward_timing.txt and policy_mlp_backward_kernel_stats.csv."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAYS, WARMUP, ROUNDS = 100, 10, 7
LR = 1e-7  # (the weights barely move over the run: every replay does the same work)

if len(sys.argv) > 1 and sys.argv[1] == "child":
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import torch

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
    pol = MaskedMLPPolicy(be, hidden=128, record_logp=True, value_head=True, network="library")
    a, p = be._action_buffers(0)
    for _ in range(5):  # a few steps in
        pol(be.tensors, a, p)
        be.step(a, p)
    pol(be.tensors, a, p)
    torch.cuda.synchronize()
    xa = be.tensors["obs_a_flat"].reshape(E * be.n, -1).clone()
    xp = be.tensors["obs_p_flat"].clone()
    ma, mp = be.action_masks()
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    batch = dict(masks_a=ma.clone().contiguous(), masks_p=mp.clone().contiguous(), actions_a=a.clone(), actions_p=p.clone(),
                 logp_old_a=pol.logp_a.clone(), logp_old_p=pol.logp_p.clone(), adv_a=rnd(E, be.n), adv_p=rnd(E),
                 values_old_a=pol.value_a.clone(), values_old_p=pol.value_p.clone(), returns_a=rnd(E, be.n), returns_p=rnd(E))
    f = dict(dtype=torch.float32, device=dev)
    wa, wp = pol.weights_a, pol.weights_p
    flat_w = list(wa.values()) + list(wp.values())
    net = (torch.empty((E * be.n, pol.MA), **f), torch.empty((E, pol.MP), **f), torch.empty(E * be.n, **f), torch.empty(E, **f))
    loss = tuple((torch.empty(8, **f), torch.empty_like(lg), torch.empty_like(v)) for lg, v in ((net[0], net[2]), (net[1], net[3])))
    grads = tuple({k: torch.empty_like(v) for k, v in w.items()} for w in (wa, wp))
    flat_g = list(grads[0].values()) + list(grads[1].values())

    def lib_forward():
        be.policy_mlp_forward(xa, xp, wa, wp, out=net)

    def lib_backward():
        be.policy_mlp_backward(xa, xp, wa, wp, loss[0][1], loss[1][1], loss[0][2], loss[1][2], out=grads)

    def lib_update():
        lib_forward()
        be.ppo_loss(net[0], net[1], net[2], net[3], batch, out=loss)
        lib_backward()
        torch._foreach_add_(flat_w, flat_g, alpha=-LR)

    lib_update()  # the stored gradients every backward below starts from
    torch.cuda.synchronize()
    tw = [w.clone().requires_grad_(True) for w in flat_w]  # the torch network's own copies, [in, out] as well
    ta, tp = dict(zip(wa, tw[:len(wa)])), dict(zip(wp, tw[len(wa):]))

    def torch_forward():
        out = []
        for x, w in ((xa, ta), (xp, tp)):
            h = torch.addmm(w["b1"], x, w["w1"]).relu()
            h = torch.addmm(w["b2"], h, w["w2"]).relu()
            out.append((torch.addmm(w["b3"], h, w["w3"]), torch.addmv(w["bv"], h, w["wv"])))
        return out[0][0], out[1][0], out[0][1], out[1][1]

    def torch_forward_backward():
        la, lp, va, vp = torch_forward()
        return torch.autograd.grad((la, lp, va, vp), tw, (loss[0][1], loss[1][1], loss[0][2], loss[1][2]))

    def torch_update():
        la, lp, va, vp = torch_forward()
        loss_a, loss_p, _, _ = rollout.ppo_loss(be, la, lp, va, vp, batch)
        gs = torch.autograd.grad(loss_a + loss_p, tw)
        with torch.no_grad():
            torch._foreach_add_(tw, list(gs), alpha=-LR)

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

    cases = [("library", "forward + backward", capture(lambda: (lib_forward(), lib_backward()))),
             ("library", "backward alone", capture(lib_backward)),
             ("library", "update", capture(lib_update)),
             ("torch", "forward alone", capture(torch_forward_only)),
             ("torch", "forward + backward", capture(torch_forward_backward)),
             ("torch", "update", capture(torch_update))]
    # the two backward passes agree (float32 sums in different orders)
    got = torch_forward_backward()
    lib_forward(), lib_backward()
    torch.cuda.synchronize()
    worst = max(float((a - b.view(a.shape)).abs().max() / (a.abs().max() + 1e-30)) for a, b in zip(got, flat_g))
    print("largest difference between torch's and the library's gradients, relative to the tensor's largest entry: %.2e" % worst,
          flush=True)

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
        print("%-20s %-8s median %7.1f us per replay (min %.1f, max %.1f over %d rounds of %d replays; device events)"
              % (what, who, ts[len(ts) // 2], ts[0], ts[-1], ROUNDS, REPLAYS), flush=True)
    tb = med[("forward + backward", "torch")] - med[("forward alone", "torch")]
    lb = med[("backward alone", "library")]
    print("backward: torch %.1f us (forward + backward minus forward alone), library %.1f us: library / torch = %.2f (device events)"
          % (tb, lb, lb / tb), flush=True)
    print("update: library / torch = %.2f (device events)" % (med[("update", "library")] / med[("update", "torch")]), flush=True)
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
    out = os.path.join(tempfile.gettempdir(), "policy_mlp_backward_timing_prof")
    shutil.rmtree(out, ignore_errors=True)
    run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "p", "--"] + child,
                         timeout=400, cwd=tempfile.gettempdir(), capture_output=True, text=True)
    stats = glob.glob(out + "/**/*kernel_stats.csv", recursive=True)
    if run.returncode != 0 or not stats:
        sys.stderr.write(run.stdout[-3000:] + run.stderr[-3000:])
        sys.exit(run.returncode or 1)
    shutil.copy(stats[0], os.path.join(dest, "policy_mlp_backward_kernel_stats.csv"))
    ours, other = [], []
    for r in csv.DictReader(open(stats[0])):
        row = "%-64s average %8.2f us (min %.2f, max %.2f) over %s launches" % (
            r["Name"].split("(")[0][:64], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, r["Calls"])
        if "aie_policy_mlp" in r["Name"] or "aie_ppo" in r["Name"]:
            ours.append(row)
        elif int(r["Calls"]) >= ROUNDS * REPLAYS:  # the torch network's kernels: every replay of a graph
            other.append(row)
    report = ["C2's shapes, 4096 batch elements: 16 384 agent rows 136 -> 128 -> 128 -> 50 + 1, 4096 planner rows 86 -> 128 -> 128 -> 154 + 1,",
              "float32; captured graphs, %d rounds alternating the cases" % ROUNDS, "", "event to event (profiler off):"] + lines + [
        "", "kernel time by name (a second run of the same script under rocprofv3 --kernel-trace --stats):",
        "the library's kernels:"] + sorted(ours) + ["", "every other kernel launched by each replay (torch):"] + sorted(other)
    with open(os.path.join(dest, "policy_mlp_backward_timing.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
