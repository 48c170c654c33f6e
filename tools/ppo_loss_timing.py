#!/usr/bin/env python
"""The PPO loss with its gradients on C2's shapes, three ways, under rocprofv3 --kernel-trace --stats (timing only):

   python tools/ppo_loss_timing.py [output directory, default profiles/]        (GPU only)

  fused     rollout.ppo_loss + (loss_a + loss_p).backward(): aie_ppo_loss (two launches) and autograd's multiply by 1
  library   today's best formulation without it: rollout.masked_logp_entropy (aie_policy_evaluate and its backward), the
            loss in torch (sum over slots, ratio, clipped minimum, clipped value loss, entropy, means), .backward()
  torch     everything in torch (masked_fill, log_softmax, gather, ... and autograd)

on a whole batch of B = 4096, a whole fragment of B = 200 x 4096, and a minibatch of 4096 rows drawn by index from that
fragment (`library` and `torch` gather every stored operand with index_select first; `fused` reads through the index).
The child process runs each (case, formulation) block back to back between two aie_sample_masked_actions launches, which
only mark the block in the kernel trace; the parent counts, per block, kernel launches and kernel time per iteration.
Writes ppo_loss_timing.txt and ppo_loss_kernel_stats.csv."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "aie_sample_masked_actions_kernel"
COEFS = dict(clip=0.3, vf_clip=50.0, vf_coef=0.05, ent_coef=0.025)

if len(sys.argv) > 1 and sys.argv[1] == "child":
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import torch

    import bench
    from ai_economist_amd.rollout import masked_logp_entropy, ppo_loss
    from helpers import make_env

    E, T = 4096, 200
    env = make_env(dict(bench.C2_CFG), n_envs=E, device="cuda:0")
    env.seed(1)
    env.reset()
    be = env.backend
    n = be.n
    ma0, mp0 = be.action_masks()
    MA, MP = ma0.shape[-1], mp0.shape[-1]
    W = be._action_buffers(0)[1].shape[-1]  # the planner's action slots
    R = T * E
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)  # noqa: E731
    rndn = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    # the stored fragment: random masks with every stored action allowed, old logp from slightly different logits
    st = {"actions_a": (rnd(R, n, 1) * MA).int().clamp_(max=MA - 1), "actions_p": (rnd(R, W) * (MP // W)).int().clamp_(max=MP // W - 1)}
    st["masks_a"] = (rnd(R, n, MA) < 0.7).float().scatter_(2, st["actions_a"].long(), 1.0)
    st["masks_p"] = (rnd(R, W, MP // W) < 0.7).float().scatter_(2, st["actions_p"].long().unsqueeze(-1), 1.0).view(R, MP)
    la_all, lp_all = rndn(R, n, MA), rndn(R, MP)
    st["logp_old_a"], st["logp_old_p"], _, _ = be.policy_evaluate(la_all + 0.1 * rndn(R, n, MA), lp_all + 0.1 * rndn(R, MP), st["masks_a"],
                                                                  st["masks_p"], st["actions_a"], st["actions_p"], entropy=False)
    for who, shape in (("a", (R, n)), ("p", (R,))):
        st["adv_" + who], st["values_old_" + who], st["returns_" + who] = rndn(*shape), rndn(*shape), rndn(*shape)
    index = torch.randint(0, R, (E,), device="cuda", generator=g).int()
    N_OF = {"batch 4096": 100, "fragment 200 x 4096": 10, "minibatch 4096 by index": 100}

    def case(name):
        """(logits_a, logits_p, values_a, values_p) leaves, the stored dict, the index, and the gather for the others."""
        if name == "batch 4096":
            rows, stored, idx = slice(0, E), {k: v[:E] for k, v in st.items()}, None
        elif name == "fragment 200 x 4096":
            rows, stored, idx = slice(0, R), st, None
        else:
            rows, stored, idx = index.long(), st, index
        B = E if name != "fragment 200 x 4096" else R
        nets = [la_all[rows].clone().requires_grad_(True), lp_all[rows].clone().requires_grad_(True),
                rndn(B, n).requires_grad_(True), rndn(B).requires_grad_(True)]
        return nets, stored, idx

    def gathered(stored, idx):
        return stored if idx is None else {k: v.index_select(0, idx.long()) for k, v in stored.items()}

    def torch_loss(logp, ent, value, s, who):  # logp, ent: [B, actors, slots]
        ratio = (logp.sum(-1) - s["logp_old_" + who].view(logp.shape).sum(-1)).exp()
        adv = s["adv_" + who].view(ratio.shape)
        pol = -torch.min(ratio * adv, ratio.clamp(1 - COEFS["clip"], 1 + COEFS["clip"]) * adv).mean()
        vo, rt, v = s["values_old_" + who].view(ratio.shape), s["returns_" + who].view(ratio.shape), value.view(ratio.shape)
        vf = torch.max((v - rt) ** 2, (vo + (v - vo).clamp(-COEFS["vf_clip"], COEFS["vf_clip"]) - rt) ** 2).mean()
        return pol + COEFS["vf_coef"] * vf - COEFS["ent_coef"] * ent.sum(-1).mean()

    def fused(nets, stored, idx):
        loss_a, loss_p, _, _ = ppo_loss(be, nets[0], nets[1], nets[2], nets[3], stored, index=idx, **COEFS)
        (loss_a + loss_p).backward()

    def library(nets, stored, idx):
        s = gathered(stored, idx)
        B = nets[0].shape[0]
        la_, lp_, ea, ep = masked_logp_entropy(be, nets[0], nets[1], s["masks_a"], s["masks_p"], s["actions_a"], s["actions_p"])
        (torch_loss(la_, ea, nets[2], s, "a") + torch_loss(lp_.view(B, 1, W), ep.view(B, 1, W), nets[3], s, "p")).backward()

    def all_torch(nets, stored, idx):
        s = gathered(stored, idx)
        B = nets[0].shape[0]
        total = 0
        for x, m, act, val, who in ((nets[0].view(B, n, 1, MA), s["masks_a"].view(B, n, 1, MA), s["actions_a"].view(B, n, 1, 1), nets[2], "a"),
                                    (nets[1].view(B, 1, W, -1), s["masks_p"].view(B, 1, W, -1), s["actions_p"].view(B, 1, W, 1), nets[3], "p")):
            dead = m < 0.5
            lsm = torch.log_softmax(x.masked_fill(dead, float("-inf")), -1)
            logp = lsm.gather(-1, act.long())[..., 0]
            ent = -(lsm.exp() * lsm.masked_fill(dead, 0.0)).sum(-1)
            total = total + torch_loss(logp, ent, val, s, who)
        total.backward()

    for name, N in N_OF.items():
        nets, stored, idx = case(name)
        # what one fused call allocates beyond its two gradients (and, once, the workspace)
        be.ppo_loss(nets[0], nets[1], nets[2], nets[3], stored, index=idx, **COEFS)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = be.ppo_loss(nets[0], nets[1], nets[2], nets[3], stored, index=idx, **COEFS)
        torch.cuda.synchronize()
        grads = sum(t.numel() * 4 for cls in out for t in cls[1:])
        print("alloc   | %s | one be.ppo_loss call: peak %d bytes above the operands; its four gradient tensors are %d bytes"
              % (name, torch.cuda.max_memory_allocated() - before, grads), flush=True)
        del out
        for form, fn in (("fused", fused), ("library", library), ("torch", all_torch)):
            for _ in range(3):
                for t in nets:
                    t.grad = None
                fn(nets, stored, idx)
            torch.cuda.synchronize()
            be.sample_masked_actions(seed=3)  # the block's start in the kernel trace
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
            for s_, e_ in evs:
                for t in nets:
                    t.grad = None
                s_.record()
                fn(nets, stored, idx)
                e_.record()
            be.sample_masked_actions(seed=3)  # ... and its end
            torch.cuda.synchronize()
            ts = sorted(s_.elapsed_time(e_) * 1e3 for s_, e_ in evs)
            print("block   | %s | %s | %d | median %.1f us, p10 %.1f, p90 %.1f (event to event)"
                  % (name, form, N, ts[N // 2], ts[N // 10], ts[9 * N // 10]), flush=True)
        del nets
else:
    import csv
    import glob
    import shutil
    import tempfile

    dest = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(dest, exist_ok=True)
    out = os.path.join(tempfile.gettempdir(), "ppo_loss_timing_prof")
    shutil.rmtree(out, ignore_errors=True)
    run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "p", "--",
                          sys.executable, os.path.abspath(__file__), "child"], timeout=900, cwd=tempfile.gettempdir(),
                         capture_output=True, text=True)
    blocks = [ln.split(" | ") for ln in run.stdout.splitlines() if ln.startswith("block   | ")]
    allocs = [ln for ln in run.stdout.splitlines() if ln.startswith("alloc   | ")]
    if run.returncode != 0 or not blocks:
        sys.stderr.write(run.stdout[-3000:] + run.stderr[-3000:])
        sys.exit(run.returncode or 1)
    stats = glob.glob(out + "/**/*kernel_stats.csv", recursive=True)
    shutil.copy(stats[0], os.path.join(dest, "ppo_loss_kernel_stats.csv"))
    trace = [f for f in glob.glob(out + "/**/*kernel_trace.csv", recursive=True)][0]
    rows = list(csv.DictReader(open(trace)))
    col = lambda want: [k for k in rows[0] if k.lower() == want][0]  # noqa: E731
    kn, ks, ke = col("kernel_name"), col("start_timestamp"), col("end_timestamp")
    rows.sort(key=lambda r: int(r[ks]))
    marks = [i for i, r in enumerate(rows) if r[kn].startswith(MARK)]
    assert len(marks) == 2 * len(blocks), (len(marks), len(blocks))
    report = ["C2 shapes (4 agents x 50 logits, planner 7 x 22); rocprofv3 --kernel-trace --stats; per timed iteration of each block",
              "", "%-26s %-8s %10s %14s %18s   %s" % ("case", "form", "launches", "kernel us", "aie_ppo launches", "event to event, host included")]
    for i, (_, name, form, N, host) in enumerate(blocks):
        N = int(N)
        mine = [r for r in rows[marks[2 * i] + 1:marks[2 * i + 1]] if not r[kn].startswith("aie_sample_")]
        ppo = sum(1 for r in mine if r[kn].startswith("aie_ppo_"))
        report.append("%-26s %-8s %10.1f %14.1f %18s   %s" % (
            name, form, len(mine) / N, sum(int(r[ke]) - int(r[ks]) for r in mine) / 1e3 / N,
            "%.2f" % (ppo / N) if form == "fused" else "-", host.strip()))
    report += ["", "(fused: aie_ppo_loss_kernel + aie_ppo_reduce_kernel, and torch's own small kernels around them: two clones of "
               "a statistic, the sum of the two losses, autograd's multiplies of the gradients by 1)", ""] + allocs
    ours = ["%-40s average %.2f us (min %.2f, max %.2f) over %s launches" % (
        r["Name"].split("(")[0][:40], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, r["Calls"])
        for r in csv.DictReader(open(stats[0])) if "aie_ppo" in r["Name"] or "aie_policy_eval" in r["Name"]]
    report += ["", "the library's kernels over the whole run (all three cases together):"] + sorted(ours)
    with open(os.path.join(dest, "ppo_loss_timing.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
