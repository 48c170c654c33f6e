#!/usr/bin/env python
"""Development tool: runs 20 launches of aie_step_kernel per dev skip mask so that a
`rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU ...` run can attribute dynamic instruction
counts to phases (parse with tools/phase_insts_report.py)."""
import torch

import devlib

bench, make_env = devlib.setup()

S = devlib.switches("AIE_DEV_SKIP_")  # csrc/aie_layout.h: bits 0 .. 14 one at a time, then the six coarse phases together
MASKS = [0] + sorted(v for v in S.values() if v <= S["AIE_DEV_SKIP_TAX"]) + [sum(v for v in S.values() if v <= S["AIE_DEV_SKIP_RECORD_STORE"])]
env = make_env(bench.C2_CFG, n_envs=4096, device="cuda:0")
env.seed(1)
env.reset()
be = env.backend
for _ in range(300):
    a, p = be.sample_random_actions(1234)
    be.step(a, p)
torch.cuda.synchronize()
snap = be.arena.clone()
a, p = be.sample_random_actions(1234)
for m in MASKS:
    be.arena.copy_(snap)
    be.lib.aie_dev_set_skip_mask(be.handle, m)
    for _ in range(20):
        be.step(a, p)
    torch.cuda.synchronize()
print("masks", MASKS)
