#!/usr/bin/env python
"""The policy sampler with and without log-probabilities, and policy evaluation (forward + backward) against the torch
formulation, on C2's shapes (4096 replicas: 45 056 rows, 1.45 M entries), under rocprofv3 --kernel-trace --stats.

   python tools/policy_eval_timing.py [output directory, default profiles/]        (GPU only)

The child process runs, N launches each and back to back: aie_sample_policy_actions, aie_sample_policy_actions_logp,
aie_policy_evaluate + aie_policy_evaluate_backward (through rollout.masked_logp_entropy and loss.backward()), and the
torch formulation of the same loss (masked_fill, log_softmax, gather, the entropy sum, autograd backward).  It prints
event-to-event medians; the parent reads the kernel statistics: the library's kernels by name, the torch formulation as the
sum over every other kernel that ran at least N times.  Writes policy_eval_kernel_stats.csv and policy_eval_timing.txt."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 100

if len(sys.argv) > 1 and sys.argv[1] == "child":
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import torch

    import bench
    from ai_economist_amd.rollout import masked_logp_entropy
    from helpers import make_env

    E = 4096
    env = make_env(dict(bench.C2_CFG), n_envs=E, device="cuda:0")
    env.seed(1)
    env.reset()
    be = env.backend
    for t in range(20):  # masks of a running episode
        a, p = be.sample_masked_actions(seed=3)
        be.step(a, p)
    ma, mp = be.action_masks()
    la = torch.randn(ma.shape, device="cuda").requires_grad_(True)
    lp = torch.randn(mp.shape, device="cuda").requires_grad_(True)
    a, p, ga, gp = be.sample_policy_actions(la.detach(), lp.detach(), seed=5, logp=True)
    a, p = a.clone(), p.clone()
    adv_a, adv_p = torch.randn(a.shape, device="cuda"), torch.randn(p.shape, device="cuda")
    W = p.shape[-1]
    al, pl = a.long(), p.long()
    na, npl = ma < 0.5, (mp < 0.5).view(E, W, -1)

    def plain():
        be.sample_policy_actions(la.detach(), lp.detach(), seed=5)

    def with_logp():
        be.sample_policy_actions(la.detach(), lp.detach(), seed=5, logp=True)

    def fused():
        la.grad = lp.grad = None
        la_, lp_, ea, ep = masked_logp_entropy(be, la, lp, ma, mp, a, p)
        (-(la_ * adv_a).sum() - (lp_ * adv_p).sum() - 0.05 * (ea.sum() + ep.sum())).backward()

    def fused_kernels_only():
        be.policy_evaluate(la.detach(), lp.detach(), ma, mp, a, p)
        be.policy_evaluate_backward(la.detach(), lp.detach(), ma, mp, a, p, adv_a, adv_p, adv_a, adv_p)

    def torch_form():
        la.grad = lp.grad = None
        total = 0
        for x, dead, act, adv in ((la, na, al, adv_a), (lp.view(E, W, -1), npl, pl.view(E, W, 1), adv_p.view(E, W, 1))):
            lsm = torch.log_softmax(x.masked_fill(dead, float("-inf")), -1)
            lg = lsm.gather(-1, act)
            H = -(lsm.exp() * lsm.masked_fill(dead, 0.0)).sum(-1)
            total = total - (lg * adv).sum() - 0.05 * H.sum()
        total.backward()

    for name, fn in (("sampler", plain), ("sampler_logp", with_logp), ("evaluate_fused_autograd", fused),
                     ("evaluate_fused_two_launches", fused_kernels_only), ("evaluate_torch", torch_form)):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
        for s, e in evs:
            s.record()
            fn()
            e.record()
        torch.cuda.synchronize()
        ts = sorted(s.elapsed_time(e) * 1e3 for s, e in evs)
        print("%-30s median %.1f us, p10 %.1f, p90 %.1f (event to event)" % (name, ts[N // 2], ts[N // 10], ts[9 * N // 10]), flush=True)
else:
    import csv
    import glob
    import shutil
    import tempfile

    dest = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(dest, exist_ok=True)
    out = os.path.join(tempfile.gettempdir(), "policy_eval_timing_prof")
    shutil.rmtree(out, ignore_errors=True)
    run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "p", "--",
                          sys.executable, os.path.abspath(__file__), "child"], timeout=500, cwd=tempfile.gettempdir(),
                         capture_output=True, text=True)
    lines = [ln for ln in run.stdout.splitlines() if "event to event" in ln]
    if run.returncode != 0 or not lines:
        sys.stderr.write(run.stdout[-3000:] + run.stderr[-3000:])
        sys.exit(run.returncode or 1)
    stats = glob.glob(out + "/**/*kernel_stats.csv", recursive=True)
    shutil.copy(stats[0], os.path.join(dest, "policy_eval_kernel_stats.csv"))
    ours, other_ns = [], 0.0
    for r in csv.DictReader(open(stats[0])):
        if "aie_" in r["Name"]:
            if "policy" in r["Name"]:
                ours.append("%-72s average %.2f us (min %.2f, max %.2f) over %s launches" % (
                    r["Name"].split("(")[0][:72], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, r["Calls"]))
        elif int(r["Calls"]) >= N:
            other_ns += float(r["TotalDurationNs"])
    # the torch formulation ran 10 + N times; kernels torch launches for the fused path's loss (sums, multiplies) count too
    report = ["C2 shapes, 4096 replicas (45 056 rows, 1.45 M entries); rocprofv3 --kernel-trace --stats, %d timed launches each" % N,
              "", "kernel time by name:"] + sorted(ours) + [
        "", "every other kernel that ran >= %d times (the torch formulation and the loss arithmetic around the fused path), "
        "summed per iteration of the torch formulation: %.1f us" % (N, other_ns / 1e3 / (N + 10)), "", "event to event, host included:"] + lines
    with open(os.path.join(dest, "policy_eval_timing.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
