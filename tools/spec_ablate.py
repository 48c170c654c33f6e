#!/usr/bin/env python
"""Development tool: launch time of the gather-trade-build step kernel's COMPILE-TIME instance with one phase switched
off at a time (aie_dev_set_skip_mask through the -DAIE_DEV build: the traced instances honour the mask), from one
arena snapshot.  Run under `rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU ...` to get the dynamic
instruction counts of the same launches (parse with tools/spec_ablate_report.py).  GPU only.

   python tools/spec_ablate.py [n_agents ...]        (default: 4 10)
"""
import os
import sys

import torch

import devlib

bench, make_env = devlib.setup()

S = {k[len("AIE_DEV_"):]: v for k, v in devlib.switches("AIE_DEV_").items()}  # csrc/aie_layout.h
SHOW = {"SKIP_COMPONENTS": "-components", "SKIP_REGEN": "-regen", "SKIP_MAP_OBS": "-map observations",
        "SKIP_FLAT_AND_MASKS": "-flat vectors -masks", "SKIP_REWARDS": "-rewards", "SKIP_RECORD_STORE": "-record store",
        "SKIP_FLAT_STAGE_A": "-flat stage A", "SKIP_FLAT_CDA": "-flat cda", "SKIP_FLAT_TAX": "-flat tax", "SKIP_MASKS": "-masks",
        "SKIP_PLANNER_COPY_OUT": "-planner copy-out", "SKIP_BUILD": "-build", "SKIP_CDA": "-cda", "SKIP_GATHER": "-gather",
        "SKIP_TAX": "-tax", "MAP_OBS_FULL": "full map rewrite instead of in-place", "FLAT_FULL": "flat vectors rewritten in full",
        "SKIP_DRAW_WINDOW": "skeleton - draw window", "SKIP_LOCMAP": "skeleton - occupancy map",
        "SKIP_ACTION_DECODE": "skeleton - action decode", "SKIP_GENERATOR_ROWS": "skeleton - generator rows to registers"}
LOAD = ["SKIP_DRAW_WINDOW", "SKIP_LOCMAP", "SKIP_ACTION_DECODE", "SKIP_GENERATOR_ROWS"]  # what the skeleton still does
SINGLE = [k for k in SHOW if k not in LOAD]
TAILS = S["SKIP_COMPONENTS"] | S["SKIP_REGEN"] | S["SKIP_MAP_OBS"] | S["SKIP_FLAT_AND_MASKS"] | S["SKIP_REWARDS"] | S["SKIP_MASKS"]
SK = TAILS | S["SKIP_RECORD_STORE"]  # the skeleton: record in, decode, occupancy map (nothing else, no record store)
ALL_LOAD = sum(S[k] for k in LOAD)
NAMES = {0: "full", TAILS: "record in, decode, occupancy map, record out only", SK: "record in, decode, occupancy map only",
         S["SKIP_FLAT_AND_MASKS"] | S["SKIP_REWARDS"]: "-flat -rewards (wave 0 tail)",
         S["SKIP_REGEN"] | S["SKIP_MAP_OBS"] | S["SKIP_MASKS"]: "-regen -map obs -masks (wave 1 tail)", SK | ALL_LOAD: "skeleton - all four"}
NAMES.update({S[k]: SHOW[k] for k in SINGLE})
NAMES.update({SK | S[k]: SHOW[k] for k in LOAD})
SKELETON = [TAILS, SK] + [SK | S[k] for k in LOAD] + [SK | ALL_LOAD, 0]
MASKS = [0] + [S[k] for k in SINGLE] + [S["SKIP_FLAT_AND_MASKS"] | S["SKIP_REWARDS"], S["SKIP_REGEN"] | S["SKIP_MAP_OBS"] | S["SKIP_MASKS"]] + SKELETON
if os.environ.get("ABLATE_SKELETON"):
    MASKS = [0] + SKELETON
LAUNCHES = 30
E = 4096


def main():
    import json

    agents = [int(x) for x in sys.argv[1:]] or [4, 10]
    times = {}
    for n in agents:
        env = make_env(dict(bench.C2_CFG, n_agents=n), n_envs=E, device="cuda:0")
        env.seed(1)
        env.reset()
        be = env.backend
        print("n_agents", n, "step kernel instance", be.lib.aie_step_kernel_instance(be.handle), flush=True)
        for _ in range(300):
            a, p = be.sample_random_actions(1234)
            be.step(a, p)
        torch.cuda.synchronize()
        snap = be.arena.clone()
        a, p = be.sample_random_actions(1234)
        base = None
        for m in MASKS:
            be.arena.copy_(snap)
            be.lib.aie_dev_set_skip_mask(be.handle, m)
            for _ in range(5):
                be.step(a, p)
            be.arena.copy_(snap)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                be.step(a, p)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1000.0 / LAUNCHES
            if base is None:
                base = us
            print("  mask %6d %-40s %7.2f us per launch (%+6.2f)" % (m, NAMES.get(m, "?"), us, us - base), flush=True)
            times.setdefault(str(n), []).append({"mask": m, "phase_off": NAMES.get(m, "?"), "us_per_launch": us})
        be.lib.aie_dev_set_skip_mask(be.handle, 0)
        del env, be
    if os.environ.get("ABLATE_JSON"):  # launch times per switched-off phase (tools/spec_ablate_report.py adds the counters)
        json.dump(times, open(os.environ["ABLATE_JSON"], "w"), indent=1)


if __name__ == "__main__":
    main()
