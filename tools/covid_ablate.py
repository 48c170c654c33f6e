#!/usr/bin/env python
"""Development tool: launch time of the COVID step kernel (BASELINE configs[3], recurrence instantiation) with parts of
its memory traffic switched off (CV_SKIP in csrc/aie_kernels_covid.hip, -DAIE_DEV build).  GPU only."""
import torch

import devlib

bench, _ = devlib.setup()

E = 8192
env = bench.make_env(bench._c4_cfg(), n_envs=E, device="cuda:0")
env.reset()
be = env.backend
cur = [be.sample_random_actions(1234, 0, slot=0), 0]


def step():
    cur[0] = be.step_sample_next(cur[0][0], cur[0][1], 1234, 0, next_slot=cur[1] ^ 1)
    cur[1] ^= 1


def timed(n):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    ev0.record()
    for _ in range(n):
        step()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / n * 1e3


NAMES = {v: k[len("AIE_CV_SKIP_"):].lower().replace("_", " ") for k, v in devlib.switches("AIE_CV_SKIP_").items()}  # csrc/aie_layout.h
for _ in range(20):
    step()
base = None
for mask in (0, 1, 2, 3, 4, 8, 16, sum(NAMES), 0):
    be.lib.aie_dev_set_skip_mask(be.handle, mask)
    for _ in range(5):
        step()
    env.reset()
    us = min(timed(100) for _ in range(3))
    base = base or us
    print("skip %-3d %-80s %.2f us (%+.2f)" % (mask, " + ".join(v for k, v in NAMES.items() if mask & k) or "nothing", us, us - base))
