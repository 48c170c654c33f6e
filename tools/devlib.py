"""What the development tools share: the -DAIE_DEV library (libaie_hip_dev.so: aie_dev_* hooks, traced kernels --
ai_economist_amd._cabi.bind_dev declares their prototypes) and the names of the development switches.

   import devlib
   bench, make_env = devlib.setup()          # before anything creates an environment
   SKIP = devlib.switches()                  # {"AIE_DEV_SKIP_REGEN": 2, ...}
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def setup():
    """Environments created from here on load the dev library; returns (bench, helpers.make_env)."""
    os.environ["AIE_DEV_LIB"] = "1"  # the aie_dev_* hooks live in libaie_hip_dev.so (-DAIE_DEV) only
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import bench
    from helpers import make_env

    return bench, make_env


def switches(prefix=""):
    """The development switches csrc/aie_layout.h names (AIE_DEV_* for the gather-trade-build step kernel, AIE_OSE_SKIP_*,
    AIE_CV_SKIP_*, AIE_SAMPLER_SKIP_*): {name: value}, those whose name starts with `prefix`."""
    with open(os.path.join(ROOT, "ai-economist_amd", "csrc", "aie_layout.h")) as f:
        found = re.findall(r"^#define (AIE_(?:DEV|OSE_SKIP|CV_SKIP|SAMPLER_SKIP)_\w+) \(1 << (\d+)\)", f.read(), re.M)
    return {name: 1 << int(bit) for name, bit in found if name.startswith(prefix)}
