#!/usr/bin/env python
"""The policy network in the rollout loop, torch against the library's one launch, on C2 at 4096 replicas (16 384 agent
rows through 136 -> 128 -> 128 -> 50 + 1, 4096 planner rows through 86 -> 128 -> 128 -> 154 + 1).

   python tools/policy_mlp_timing.py [output directory, default profiles/]        (GPU only)
   python tools/policy_mlp_timing.py pmc [output directory]     hardware counters of the network's kernel -> policy_mlp_pmc.txt

One child process builds, for network = "torch" and network = "library", a MaskedMLPPolicy (value head and logp on: what
a PPO rollout runs), a captured graph of the policy alone and a GraphedStep iteration (policy + aie_step + auto-reset),
and times each as bench.py's C2pi leg does -- device events around 200 replays behind 20 warm-up replays -- in ROUNDS
alternating rounds, so that the two networks see the same machine; it prints the median and the extremes over the rounds.
The parent runs that child once plainly (the timings of record) and once more under rocprofv3 --kernel-trace --stats for
the per-kernel times.  Writes policy_mlp_timing.txt and policy_mlp_kernel_stats.csv."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAYS, WARMUP, ROUNDS = 200, 20, 7

G1 = "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE"
G2 = "SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VMEM SQ_INSTS_VMEM_RD"

if len(sys.argv) > 1 and sys.argv[1] == "child-mlp":  # the network's launch alone, for a counter pass
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import torch

    import bench
    from ai_economist_amd.rollout import MaskedMLPPolicy
    from helpers import make_env

    env = make_env(dict(bench.C2_CFG), n_envs=4096, device="cuda:0")
    env.seed(1)
    env.reset()
    pol = MaskedMLPPolicy(env.backend, hidden=128, record_logp=True, value_head=True, network="library")
    for _ in range(30):
        pol.logits(env.backend.tensors)
    torch.cuda.synchronize()
elif len(sys.argv) > 1 and sys.argv[1] == "pmc":
    # counters of aie_policy_mlp_kernel: two --pmc passes of their own, no tracing beside them
    import collections
    import csv
    import glob
    import shutil
    import tempfile

    dest = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
    os.makedirs(dest, exist_ok=True)
    acc = collections.defaultdict(list)
    for i, group in enumerate((G1, G2)):
        out = os.path.join(tempfile.gettempdir(), "policy_mlp_pmc_%d" % i)
        shutil.rmtree(out, ignore_errors=True)
        run = subprocess.run(["rocprofv3", "--pmc"] + group.split() + ["--output-format", "csv", "-d", out, "-o", "p", "--",
                              sys.executable, os.path.abspath(__file__), "child-mlp"], timeout=400, cwd=tempfile.gettempdir(),
                             capture_output=True, text=True)
        files = glob.glob(out + "/**/*counter_collection.csv", recursive=True)
        if run.returncode != 0 or not files:
            sys.stderr.write(run.stdout[-2000:] + run.stderr[-2000:])
            sys.exit(run.returncode or 1)
        for r in csv.DictReader(open(files[0])):
            if "aie_policy_mlp" in r["Kernel_Name"]:
                acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
    lines = ["aie_policy_mlp_kernel at C2, 4096 replicas: mean per launch over %d launches, rocprofv3 --pmc (two passes, no tracing);"
             % len(next(iter(acc.values()))), "cycle counters are summed over the chip's SIMDs / CUs as the counter is defined", ""]
    lines += ["%-28s %.5g" % (k, sum(v) / len(v)) for k, v in sorted(acc.items())]
    with open(os.path.join(dest, "policy_mlp_pmc.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
elif len(sys.argv) > 1 and sys.argv[1] == "child":
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import torch

    import bench
    from ai_economist_amd.rollout import GraphedStep, MaskedMLPPolicy
    from helpers import make_env

    E = 4096
    cases = {}
    for network in ("torch", "library"):
        env = make_env(dict(bench.C2_CFG), n_envs=E, device="cuda:0")
        env.seed(1)
        env.reset()
        pol = MaskedMLPPolicy(env.backend, hidden=128, record_logp=True, value_head=True, network=network)
        gs = GraphedStep(env, pol, auto_reset=True, warmup=3)
        g_pol = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_pol):
            pol(env.backend.tensors, gs.actions_a, gs.actions_p)
        cases[network] = (env, pol, gs, g_pol)

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / REPLAYS  # us per replay

    got = {}
    for _ in range(ROUNDS):
        for network, (env, pol, gs, g_pol) in cases.items():
            got.setdefault((network, "policy only"), []).append(timed(g_pol.replay))
            got.setdefault((network, "policy + step"), []).append(timed(lambda: gs.replay(1)))
    for env, _, _, _ in cases.values():
        assert int(env.backend.tensors["error_flags"].abs().sum()) == 0
    for (network, what), ts in sorted(got.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        ts = sorted(ts)
        print("%-14s network=%-8s median %6.1f us per replay (min %.1f, max %.1f over %d rounds of %d replays; device events)"
              % (what, network, ts[len(ts) // 2], ts[0], ts[-1], ROUNDS, REPLAYS), flush=True)
else:
    import csv
    import glob
    import shutil
    import tempfile

    dest = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(dest, exist_ok=True)
    child = [sys.executable, os.path.abspath(__file__), "child"]
    plain = subprocess.run(child, timeout=500, cwd=tempfile.gettempdir(), capture_output=True, text=True)
    lines = [ln for ln in plain.stdout.splitlines() if "device events" in ln]
    if plain.returncode != 0 or not lines:
        sys.stderr.write(plain.stdout[-3000:] + plain.stderr[-3000:])
        sys.exit(plain.returncode or 1)
    out = os.path.join(tempfile.gettempdir(), "policy_mlp_timing_prof")
    shutil.rmtree(out, ignore_errors=True)
    run = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "p", "--"] + child,
                         timeout=500, cwd=tempfile.gettempdir(), capture_output=True, text=True)
    stats = glob.glob(out + "/**/*kernel_stats.csv", recursive=True)
    if run.returncode != 0 or not stats:
        sys.stderr.write(run.stdout[-3000:] + run.stderr[-3000:])
        sys.exit(run.returncode or 1)
    shutil.copy(stats[0], os.path.join(dest, "policy_mlp_kernel_stats.csv"))
    ours, other = [], []
    for r in csv.DictReader(open(stats[0])):
        row = "%-64s average %8.2f us (min %.2f, max %.2f) over %s launches" % (
            r["Name"].split("(")[0][:64], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, r["Calls"])
        if "aie_policy_mlp" in r["Name"] or "aie_sample_policy" in r["Name"] or "aie_step" in r["Name"]:
            ours.append(row)
        elif int(r["Calls"]) >= 2 * ROUNDS * REPLAYS:  # the torch network's kernels: every replay of both graphs
            other.append(row)
    report = ["C2, 4096 replicas: 16 384 agent rows 136 -> 128 -> 128 -> 50 + 1, 4096 planner rows 86 -> 128 -> 128 -> 154 + 1, float32;",
              "MaskedMLPPolicy(record_logp=True, value_head=True), captured graphs, %d rounds alternating the two networks" % ROUNDS,
              "", "event to event (profiler off):"] + lines + [
        "", "kernel time by name (a second run of the same script under rocprofv3 --kernel-trace --stats):",
        "the library's kernels:"] + sorted(ours) + ["", "every other kernel launched by each replay (the torch network):"] + sorted(other)
    with open(os.path.join(dest, "policy_mlp_timing.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))
