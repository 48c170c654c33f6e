#!/usr/bin/env python
"""The trajectory store and aie_gae against their torch formulations on the same tensors, in the same run: C2, 4096 replicas,
T = 200, flat observations.

   python tools/trajectory_timing.py [output directory, default profiles/]        (GPU only)

Four GPU steps, each a child process of its own under `timeout -k 10`, chained: the first that fails ends the run.
  store          (a) per-step storage of the ten trajectory tensors (observations, masks, actions, logp, values) replayed from
                 a hipGraph: ONE aie_trajectory_store launch, against index_copy_ with a device index (one per tensor, plus
                 the two launches that advance the index); the storage alone, and inside the whole captured iteration
                 (policy -> store -> step) beside the iteration with no storage at all;
  gae            (b) aie_gae against the torch T-step loop (agents and planner in one tensor, ~7 launches per step), eager and
                 captured, and against the bytes it moves;
  profile-store, profile-gae    the same work under rocprofv3 --kernel-trace --stats (runs of their own): kernel time by name
                 for the library's two kernels, the sum over every other kernel for the torch formulation.
Event-to-event medians come from the first two steps, kernel times from the last two.  Writes trajectory_timing.txt and the two
kernel statistics files."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, T, N = 4096, 200, 100
GAMMA, LAM = 0.998, 0.98


def _median(fn, n=N, warm=5):
    import torch

    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for s, e in evs:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    ts = sorted(s.elapsed_time(e) * 1e3 for s, e in evs)
    return ts[n // 2], ts[n // 10], ts[9 * n // 10]


def _line(name, m):
    print("%-44s median %.1f us, p10 %.1f, p90 %.1f (event to event)" % ((name,) + m), flush=True)


def _setup():
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import bench
    from ai_economist_amd.rollout import MaskedMLPPolicy, Trajectory
    from helpers import make_env

    env = make_env(dict(bench.C2_CFG), n_envs=E, device="cuda:0")
    env.seed(1)
    env.reset()
    pol = MaskedMLPPolicy(env.backend, seed=1, record_logp=True, value_head=True)
    return env, pol, Trajectory(env, T)


class TorchStore:
    """The torch formulation of the store: buf.index_copy_(0, idx, x[None]) per tensor with the slot index in device memory,
    then idx = (idx + 1) % T -- capturable, two more launches."""

    def __init__(self, traj, pol, actions):
        import torch

        be = traj.be
        self.idx = torch.zeros(1, dtype=torch.int64, device=be.device)
        self.T = traj.T
        t = be.tensors
        a, p = actions
        self.pairs = [(t[k], traj.obs[k]) for k in traj.obs] + [
            (t["obs_a_action_mask"], traj.masks_a), (t["obs_p_action_mask"], traj.masks_p), (a, traj.actions_a),
            (p, traj.actions_p), (pol.logp_a, traj.logp_a), (pol.logp_p, traj.logp_p),
            (pol.value_a, traj.values_a[: traj.T]), (pol.value_p, traj.values_p[: traj.T])]

    def __call__(self):
        for src, dst in self.pairs:
            dst.index_copy_(0, self.idx, src.unsqueeze(0))
        self.idx.add_(1).remainder_(self.T)


def _graph(fn):
    import torch

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def child_store(profile):
    import torch

    from ai_economist_amd.rollout import GraphedStep

    env, pol, traj = _setup()
    be = env.backend
    a, p = be._action_buffers(0)
    pol(be.tensors, a, p)
    ts = TorchStore(traj, pol, (a, p))

    def ours():
        traj.store(a, p, pol.logp_a, pol.logp_p, pol.value_a, pol.value_p)

    nbytes = sum(src.numel() * src.element_size() for src, _ in ts.pairs)
    print("stored per step: %d tensors, %.2f MB" % (len(ts.pairs), nbytes / 1e6), flush=True)
    g_ours, g_torch = _graph(ours), _graph(ts)
    if profile:  # kernel times by name: N replays of each, nothing else
        for _ in range(N):
            g_ours.replay()
        for _ in range(N):
            g_torch.replay()
        torch.cuda.synchronize()
        return
    _line("store alone, aie_trajectory_store (graph)", _median(g_ours.replay))
    _line("store alone, torch index_copy_ (graph)", _median(g_torch.replay))
    _line("store alone, aie_trajectory_store (eager)", _median(ours))
    _line("store alone, torch index_copy_ (eager)", _median(ts))

    # the whole captured iteration: policy -> [store] -> step
    def with_torch_store(tensors, aa, ap):
        pol(tensors, aa, ap)
        ts()

    for name, kw, policy in (("iteration, no storage", {}, pol), ("iteration, aie_trajectory_store", dict(trajectory=traj), pol),
                             ("iteration, torch index_copy_", {}, with_torch_store)):
        gs = GraphedStep(env, policy, auto_reset=True, **kw)
        traj.rewind()
        _line(name + " (graph)", _median(gs.replay))


def child_gae(profile):
    import torch

    env, pol, traj = _setup()
    be = env.backend
    n = be.n
    g = torch.Generator(device="cpu").manual_seed(1)
    log = torch.randn(T, E, n + 2, generator=g)
    log[..., n + 1] = (torch.rand(T, E, generator=g) < 0.005).float()
    log = log.to("cuda:0")
    va = (torch.randn(T + 1, E, n, generator=g) * 10).to("cuda:0")
    vp = (torch.randn(T + 1, E, generator=g) * 10).to("cuda:0")
    out = [torch.empty(T, E, n, device="cuda:0"), torch.empty(T, E, device="cuda:0"),
           torch.empty(T, E, n, device="cuda:0"), torch.empty(T, E, device="cuda:0")]

    def ours():
        be.gae(T, log, va, vp, GAMMA, LAM, out=out)

    # the torch formulation on the same log: both actor classes as one [.., n + 1] tensor (half the launches of two loops)
    v = torch.cat([va, vp[..., None]], -1)
    r, nd = log[..., : n + 1], 1.0 - log[..., n + 1:]
    adv = torch.empty(T, E, n + 1, device="cuda:0")
    ret = torch.empty(T, E, n + 1, device="cuda:0")
    gl = GAMMA * LAM

    def torch_loop():
        last = torch.zeros(E, n + 1, device="cuda:0")
        for t in range(T - 1, -1, -1):
            delta = r[t] + GAMMA * v[t + 1] * nd[t] - v[t]
            last = delta + gl * nd[t] * last
            adv[t].copy_(last)
        torch.add(adv, v[:T], out=ret)

    ours()
    torch_loop()
    torch.cuda.synchronize()
    err = max(float((adv[..., :n] - out[0]).abs().max()), float((adv[..., n] - out[1]).abs().max()))
    print("aie_gae against the torch loop: max difference %.2e (max |A| %.1f)" % (err, float(adv.abs().max())), flush=True)
    g_ours, g_torch = _graph(ours), _graph(torch_loop)
    if profile:
        for _ in range(N):
            g_ours.replay()
        for _ in range(10):
            g_torch.replay()
        torch.cuda.synchronize()
        return
    moved = 4 * (T * E * (n + 2) + (T + 1) * E * (n + 1) + 2 * T * E * (n + 1))
    m = _median(ours)
    _line("aie_gae (eager, one launch)", m)
    _line("aie_gae (graph)", _median(g_ours.replay))
    print("aie_gae moves %.1f MB: %.2f TB/s at the eager median" % (moved / 1e6, moved / m[0] / 1e6), flush=True)
    _line("torch T-step loop (eager)", _median(torch_loop, n=10, warm=2))
    _line("torch T-step loop (graph)", _median(g_torch.replay, n=20, warm=2))


def parent():
    import csv
    import glob
    import shutil
    import tempfile

    dest = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    os.makedirs(dest, exist_ok=True)
    me = os.path.abspath(__file__)
    report = ["C2, %d replicas, T = %d, flat observations; %d timed launches each" % (E, T, N), ""]
    for step, secs in (("store", 240), ("gae", 240), ("profile-store", 300), ("profile-gae", 300)):
        cmd = ["timeout", "-k", "10", str(secs)]
        out = None
        if step.startswith("profile"):
            out = os.path.join(tempfile.gettempdir(), "trajectory_timing_" + step)
            shutil.rmtree(out, ignore_errors=True)
            cmd += ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "p", "--"]
        run = subprocess.run(cmd + [sys.executable, me, "child", step], cwd=tempfile.gettempdir(), capture_output=True, text=True)
        if run.returncode != 0:  # chained: nothing more is started on the GPU
            sys.stderr.write("step %s ended with status %d\n" % (step, run.returncode) + run.stdout[-3000:] + run.stderr[-3000:])
            with open(os.path.join(dest, "trajectory_timing.txt"), "w") as f:
                f.write("\n".join(report + ["step %s ended with status %d" % (step, run.returncode)]) + "\n")
            sys.exit(run.returncode)
        if out is None:
            report += ["[%s]" % step] + [ln for ln in run.stdout.splitlines() if "event to event" in ln or ln.startswith(("aie_gae ", "stored"))] + [""]
            continue
        stats = glob.glob(out + "/**/*kernel_stats.csv", recursive=True)
        shutil.copy(stats[0], os.path.join(dest, "trajectory_%s_kernel_stats.csv" % step.replace("-", "_")))
        which = "aie_trajectory_store_kernel" if step == "profile-store" else "aie_gae_kernel"
        # how often the torch formulation ran in the profiled child (replays + warm-up iterations + the eager check) and how
        # often each of its kernels must have run to count as its own (the loop's: T times per run; set-up fills do not)
        runs, floor = (N + 3, N) if step == "profile-store" else (10 + 3 + 1, T * 10)
        ours, other_ns, other_calls = "", 0.0, 0
        for r in csv.DictReader(open(stats[0])):
            if which in r["Name"] and int(r["Calls"]) >= N:
                ours = "%-30s average %.2f us (min %.2f, max %.2f) over %s launches" % (
                    which, float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3, r["Calls"])
            elif "aie_" not in r["Name"] and int(r["Calls"]) >= floor:
                other_ns += float(r["TotalDurationNs"])
                other_calls += int(r["Calls"])
        report += ["[%s] kernel time, rocprofv3 --kernel-trace --stats" % step, ours,
                   "torch formulation: %.1f us of kernel time in %.0f launches per %s (every other kernel with >= %d launches, "
                   "over the %d times the formulation ran)" % (other_ns / 1e3 / runs, other_calls / runs,
                                                              "step" if step == "profile-store" else "fragment", floor, runs), ""]
    with open(os.path.join(dest, "trajectory_timing.txt"), "w") as f:
        f.write("\n".join(report) + "\n")
    print("\n".join(report))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "child":
        step = sys.argv[2]
        (child_store if step.endswith("store") else child_gae)(step.startswith("profile"))
    else:
        parent()
