"""CPU test: what the headline step kernel (aie_step_kernel_spec<0>, BASELINE configs[1]) costs a compute unit, read
from the kernel metadata of the BUILT library -- no private segment (a kernel that enables scratch starts later), no
scalar value parked in a vector register's lanes, no vector register in scratch, at most the 64 vector registers of
8 waves per SIMD -- and from the host's own LDS formula: at most 10 240 B per workgroup, so that 16 workgroups stay
resident per CU.  Metadata fields only; the instruction text is tools/kernel_isa_diff.py's business."""
import os
import re
import shutil
import subprocess

import pytest

from helpers import ROOT

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _llvm_tool(name):
    """A ROCm LLVM tool: on the PATH, or beside the compiler hipcc drives."""
    from ai_economist_amd import _build

    dirs = []
    if _build.have_hipcc():
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(_build.hipcc_path())))
        dirs += [os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin")]
    dirs += ["/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin"]
    for cand in [shutil.which(name)] + [os.path.join(d, name) for d in dirs]:
        if cand and os.path.exists(cand):
            return cand
    return None


def _need_tools(*names):
    tools = {n: _llvm_tool(n) for n in names}
    missing = sorted(n for n, p in tools.items() if p is None)
    if missing:
        pytest.skip("ROCm LLVM tools not found (%s): the library's kernel metadata cannot be read" % ", ".join(missing))
    return tools


def kernel_metadata(lib, tmp_path):
    """{kernel symbol: {metadata field: text}} of the gfx950 code object inside `lib` (the fields of amdhsa.kernels)."""
    t = _need_tools("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([t["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + fat, lib, str(tmp_path / "rest.so")], check=True)
    subprocess.run([t["clang-offload-bundler"], "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET,
                    "--output=" + co], check=True)
    notes = subprocess.run([t["llvm-readelf"], "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"(?m)^  - (?=\.)", notes.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0])[1:]:
        fields = dict(re.findall(r"(?m)^(?:    )?\.(\w+): +(\S.*)$", block))
        kernels[fields["name"]] = fields
    return kernels


def test_headline_step_kernel_has_no_scratch_and_no_spills(tmp_path):
    from ai_economist_amd import _build

    if not _build.have_hipcc():
        pytest.skip("hipcc not found: no library to read")
    kernels = kernel_metadata(_build.build(), tmp_path)
    names = [k for k in kernels if re.match(r"_Z\d+aie_step_kernel_specILi0EE", k)]
    assert len(names) == 1, names
    k = kernels[names[0]]
    assert int(k["private_segment_fixed_size"]) == 0, k
    assert int(k["sgpr_spill_count"]) == 0, k
    assert int(k["vgpr_spill_count"]) == 0, k
    assert int(k["vgpr_count"]) <= 64, k
    assert int(k["agpr_count"]) == 0, k


def test_headline_configuration_keeps_16_workgroups_per_cu(tmp_path):
    """aie::lds_bytes of configs[1]'s constant image, evaluated by the host code of csrc/aie_device.h itself: a
    host-only compile of three lines.  Nothing is launched, so the (absent) device image stays an unresolved symbol."""
    from ai_economist_amd import _build

    if not _build.have_hipcc():
        pytest.skip("hipcc not found: the host side of aie_device.h cannot be compiled")
    src, exe = tmp_path / "lds_bytes.hip", str(tmp_path / "lds_bytes")
    src.write_text('#include "aie_device.h"\n#include <cstdio>\n'
                   'int main() { printf("%zu\\n", aie::lds_bytes(*reinterpret_cast<const aie_params*>(aie_spec_image<0>::bytes))); }\n')
    subprocess.run([_build.hipcc_path(), "--cuda-host-only", "-O0", "-std=c++17", "-Wno-comment", "-I" + os.path.join(ROOT, "include"),
                    "-I" + _build.CSRC, "-Wl,--unresolved-symbols=ignore-all", str(src), "-o", exe], check=True)
    lds = int(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert 0 < lds <= 10240, lds
