#!/usr/bin/env python
"""Development tool: times aie_step_kernel with individual phases skipped
(aie_dev_set_skip_mask) to see where a launch spends its time.  GPU only."""
import sys

import torch

import devlib

bench, make_env = devlib.setup()

E = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
cfg = dict(bench.C2_CFG)
if len(sys.argv) > 2:
    cfg["n_agents"] = int(sys.argv[2])
env = make_env(cfg, n_envs=E, device="cuda:0")
env.seed(1)
env.reset()
be = env.backend
for _ in range(300):
    a, p = be.sample_random_actions(1234)
    be.step(a, p)
torch.cuda.synchronize()
snap = be.arena.clone()


def timeit(mask, n=200):
    be.arena.copy_(snap)
    be.lib.aie_dev_set_skip_mask(be.handle, mask)
    a, p = be.sample_random_actions(1234)
    for _ in range(20):
        be.step(a, p)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(n):
        be.step(a, p)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


S = {k[len("AIE_DEV_SKIP_"):]: v for k, v in devlib.switches("AIE_DEV_SKIP_").items()}  # csrc/aie_layout.h
PHASES = ["COMPONENTS", "REGEN", "MAP_OBS", "FLAT_AND_MASKS", "REWARDS"]
ALL = sum(S[k] for k in PHASES) | S["RECORD_STORE"]
names = {0: "full", ALL: "only load+decode+locmap"}
names.update({S[k]: "-" + k.lower() for k in PHASES + ["RECORD_STORE"]})
names.update({ALL & ~S[k]: "only " + k.lower() for k in PHASES})
names.update({S[k]: "-" + k.lower() for k in ("FLAT_STAGE_A", "FLAT_CDA", "FLAT_TAX", "MASKS", "PLANNER_COPY_OUT", "BUILD", "CDA", "GATHER", "TAX")})
full = timeit(0)
for m, nm in names.items():
    t = timeit(m)
    print("%-34s %8.1f us   (delta vs full %+7.1f)" % (nm, t, t - full))
