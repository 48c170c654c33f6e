#!/usr/bin/env python
"""The optimizer step and a whole PPO update, the library's aie_adam_step (two launches) against torch's clip_grad_norm_ and
torch.optim.Adam(capturable=True), at C2's shapes with 4096 batch elements: the sixteen weight tensors of the agents'
136 -> 128 -> 128 -> 50 + 1 and the planner's 86 -> 128 -> 128 -> 154 + 1 (the child prints the parameter count).

   python tools/adam_timing.py [output directory, default profiles/]        (GPU only)

One child process takes a rollout's operands from a C2 environment, as tools/policy_mlp_backward_timing.py does, and
builds, as captured graphs:
  step alone   library:        rollout.Adam.step on the backward's gradient buffers (max_norm 10, one norm per class)
               torch foreach:  clip_grad_norm_(foreach=True) per class, then ONE Adam(capturable=True, foreach=True) over all
                               sixteen tensors (the fewest launches that compute the same thing)
               torch fused:    the same with Adam(capturable=True, fused=True), where this torch has it
  update       policy_mlp_forward, ppo_loss, policy_mlp_backward (the library's, in every case), then each of the steps
and times each -- device events around REPLAYS replays behind WARMUP warm-up replays -- in ROUNDS alternating rounds, so
that all see the same machine; it prints the median and the extremes over the rounds.  torch's optimizers update clones
of the weights whose .grad are the library's gradient buffers: the same work on the same numbers.  The parent runs that
child once plainly (the timings of record) and once more under rocprofv3 --kernel-trace --stats for the library's
per-kernel times.  Writes adam_timing.txt with the library's source hash."""
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
    net = (torch.empty((E * be.n, pol.MA), **f), torch.empty((E, pol.MP), **f), torch.empty(E * be.n, **f), torch.empty(E, **f))
    loss = tuple((torch.empty(8, **f), torch.empty_like(lg), torch.empty_like(v)) for lg, v in ((net[0], net[2]), (net[1], net[3])))
    grads = tuple({k: torch.empty_like(v) for k, v in w.items()} for w in (wa, wp))
    n_params = sum(v.numel() for w in (wa, wp) for v in w.values())
    opt = rollout.Adam(be, wa, wp, lr=LR, max_norm=10.0)

    def lib_gradients():
        be.policy_mlp_forward(xa, xp, wa, wp, out=net)
        be.ppo_loss(net[0], net[1], net[2], net[3], batch, out=loss)
        be.policy_mlp_backward(xa, xp, wa, wp, loss[0][1], loss[1][1], loss[0][2], loss[1][2], out=grads)

    def lib_step():
        opt.step(grads=grads)

    lib_gradients()  # the gradients every step below starts from
    torch.cuda.synchronize()

    def torch_optimizer(**kw):
        """Clones of the weights whose .grad are the library's gradient buffers -> the step as a function."""
        tw = [[v.clone().requires_grad_(True) for v in w.values()] for w in (wa, wp)]
        for ws, gs in zip(tw, grads):
            for t, gr in zip(ws, gs.values()):
                t.grad = gr.view(t.shape)
        adam = torch.optim.Adam(tw[0] + tw[1], lr=LR, betas=(0.9, 0.999), eps=1e-8, capturable=True, **kw)

        def step():
            torch.nn.utils.clip_grad_norm_(tw[0], 10.0, foreach=True)
            torch.nn.utils.clip_grad_norm_(tw[1], 10.0, foreach=True)
            adam.step()
        return step

    steps = [("library", lib_step), ("torch foreach", torch_optimizer(foreach=True))]
    try:
        fused = torch_optimizer(fused=True)
        fused()
        torch.cuda.synchronize()
        steps.append(("torch fused", fused))
    except Exception as e:  # this torch has no fused Adam for the device
        print("torch fused: not available here (%s)" % str(e).splitlines()[0][:120], flush=True)

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
            fn()
        return graph

    cases = [("step alone", who, capture(fn)) for who, fn in steps]
    cases += [("update", who, capture(lambda fn=fn: (lib_gradients(), fn()))) for who, fn in steps]
    print("%d parameters in sixteen tensors; after the warm-ups the library's step count is %s, its statistics %s"
          % (n_params, [int(t) for t in opt.steps()], [[round(float(x), 6) for x in s] for s in opt.stats()]), flush=True)

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
        for what, who, graph in cases:
            res.setdefault((what, who), []).append(timed(graph))
    med = {}
    for what in ("step alone", "update"):
        for who, _ in steps:
            ts = sorted(res[(what, who)])
            med[(what, who)] = ts[len(ts) // 2]
            print("%-11s %-14s median %7.1f us per replay (min %.1f, max %.1f over %d rounds of %d replays; device events)"
                  % (what, who, ts[len(ts) // 2], ts[0], ts[-1], ROUNDS, REPLAYS), flush=True)
    for what in ("step alone", "update"):
        best = min((med[(what, who)], who) for who, _ in steps[1:])
        print("%s: library / %s (torch's fastest) = %.2f (device events)" % (what, best[1], med[(what, "library")] / best[0]), flush=True)
else:
    import csv
    import glob
    import shutil
    import tempfile

    dest = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(dest, exist_ok=True)
    child = [sys.executable, os.path.abspath(__file__), "child"]
    plain = subprocess.run(child, timeout=400, cwd=tempfile.gettempdir(), capture_output=True, text=True)
    lines = [ln for ln in plain.stdout.splitlines() if "device events" in ln or "parameters" in ln or "torch fused:" in ln]
    if plain.returncode != 0 or not lines:
        sys.stderr.write(plain.stdout[-3000:] + plain.stderr[-3000:])
        sys.exit(plain.returncode or 1)
    try:
        srchash = open(os.path.join(ROOT, "ai-economist_amd", "csrc", "libaie_hip.so.srchash")).read().strip()
    except OSError:
        srchash = "unknown"
    report = ["C2's shapes, 4096 batch elements, float32; captured graphs, %d rounds alternating the cases" % ROUNDS,
              "library source hash " + srchash, "", "event to event (profiler off):"] + lines
    out = os.path.join(tempfile.gettempdir(), "adam_timing_prof")
    shutil.rmtree(out, ignore_errors=True)
    run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "p", "--"] + child,
                         timeout=400, cwd=tempfile.gettempdir(), capture_output=True, text=True)
    stats = glob.glob(out + "/**/*kernel_stats.csv", recursive=True)
    if run.returncode != 0 or not stats:
        report += ["", "(the second run under rocprofv3 --kernel-trace --stats gave no kernel statistics)"]
    else:
        ours = []
        for r in csv.DictReader(open(stats[0])):
            if "aie_adam" in r["Name"]:
                ours.append("%-40s average %8.2f us (min %.2f, max %.2f) over %s launches" % (
                    r["Name"].split("(")[0][:40], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, r["Calls"]))
        report += ["", "kernel time by name (a second run of the same script under rocprofv3 --kernel-trace --stats):"] + sorted(ours)
    with open(os.path.join(dest, "adam_timing.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
