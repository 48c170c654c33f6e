"""CPU tests: what the kernel sources are made of.  Every csrc/aie_kernels*.hip and the device library header is a
unit that compiles on its own (it includes what it uses: no file relies on its place in aie_capi.hip's include block),
no kernel file outside the gather-trade-build family is compiled from gather-trade-build code, the family's four headers
of device functions include one another in one direction only (state <- components, state <- observe, the layout
generator beside them, and none of them the kernel file), the layout header is cut in three -- what a kernel reads
(aie_layout.h), the host's builders of the parameter block (aie_layout_build.h: no kernel file is compiled from it) and the
trainer side's arithmetic (aie_trainer_math.h: no step-side file and neither run-time unit is compiled from it) -- each
of which compiles on its own as C99 and as HIP, the cache key of each
run-time unit (aie_jit.h: kSources + kSourcesOse / kSourcesGtb) names exactly the project files that unit is compiled
from, and the library's staleness hash (_build.source_files) reads every project file aie_capi.hip is compiled from.
The compiler's own preprocessor says what a unit includes (the `# n "file"` line markers); nothing is launched."""
import ast
import glob
import os
import re
import subprocess

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "ai-economist_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
KERNEL_FILES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "aie_kernels*.hip")))
# the gather-trade-build family ("How the kernel sources are organised"): its kernel file and the four headers
# of device functions it is cut into; every other kernel file sees the device library only
GTB_HEADERS = ["aie_gtb_state.h", "aie_gtb_components.h", "aie_gtb_observe.h", "aie_gtb_layoutgen.h"]
GTB_FILES = ["aie_kernels.hip"] + GTB_HEADERS
DEVICE_HEADERS = ["aie_device.h"] + GTB_HEADERS
# the layout header and the two cut out of it: only aie_layout.h is in a specialisation's key (aie_jit.h: kSources)
LAYOUT_HEADERS = ["aie_layout.h", "aie_layout_build.h", "aie_trainer_math.h"]
NOT_KEYED = ["aie_layout_build.h", "aie_trainer_math.h"]
STEP_SIDE = ["aie_kernels.hip", "aie_kernels_ose.hip", "aie_kernels_covid.hip", "aie_kernels_saez.hip"] + DEVICE_HEADERS
# aie_jit_image.h as aie_jit.h writes it per configuration; the preprocessor does not care for the image's size
STUB_IMAGE = ("#pragma once\n#define AIE_N_SPECS 1\ntemplate <int K> struct aie_spec_image;\n"
              "alignas(16) static constexpr unsigned char aie_jit_bytes[1] = {0};\n"
              "template <> struct aie_spec_image<0> { static constexpr const unsigned char* bytes = aie_jit_bytes; "
              "static constexpr int waves = 8; };\n")


def _hipcc():
    from ai_economist_amd import _build

    if not _build.have_hipcc():
        pytest.skip("hipcc not found: the kernel sources cannot be compiled")
    return [_build.hipcc_path(), "--offload-arch=gfx950", "--cuda-device-only", "-std=c++17", "-Wno-comment",
            "-Wno-pragma-once-outside-header", "-I" + CSRC, "-I" + INCLUDE]


def _project_files(unit, extra=()):
    """The files under the repository that the device side of `unit` is compiled from, the unit itself included."""
    text = subprocess.run(_hipcc() + ["-E"] + list(extra) + ["-x", "hip", unit, "-o", "-"], check=True, capture_output=True, text=True).stdout
    files = {os.path.realpath(f) for f in re.findall(r'(?m)^# \d+ "([^"<][^"]*)"', text)}
    return {f for f in files if f.startswith(os.path.realpath(ROOT) + os.sep)}


@pytest.mark.parametrize("name", KERNEL_FILES + DEVICE_HEADERS)
def test_each_kernel_file_compiles_on_its_own(name):
    r = subprocess.run(_hipcc() + ["-fsyntax-only", "-x", "hip", os.path.join(CSRC, name)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("name", [n for n in KERNEL_FILES if n not in GTB_FILES])
def test_only_the_gather_trade_build_family_sees_gather_trade_build_code(name):
    assert all(os.path.exists(os.path.join(CSRC, n)) for n in GTB_FILES), GTB_FILES
    seen = {os.path.basename(f) for f in _project_files(os.path.join(CSRC, name))}
    assert "aie_device.h" in seen and not seen & set(GTB_FILES), sorted(seen)


@pytest.mark.parametrize("name, unseen", [
    ("aie_gtb_state.h", ["aie_gtb_components.h", "aie_gtb_observe.h", "aie_gtb_layoutgen.h"]),
    ("aie_gtb_components.h", ["aie_gtb_observe.h", "aie_gtb_layoutgen.h"]),
    ("aie_gtb_observe.h", ["aie_gtb_components.h", "aie_gtb_layoutgen.h"]),
    ("aie_gtb_layoutgen.h", ["aie_gtb_components.h", "aie_gtb_observe.h"]),
])
def test_gather_trade_build_headers_depend_one_way(name, unseen):
    """state <- components, state <- observe, layoutgen beside them; all four <- aie_kernels.hip and never back."""
    seen = {os.path.basename(f) for f in _project_files(os.path.join(CSRC, name))}
    assert name in seen and "aie_device.h" in seen, sorted(seen)
    assert not seen & set(unseen + ["aie_kernels.hip"]), sorted(seen)


@pytest.mark.parametrize("name", STEP_SIDE)
def test_step_side_sees_neither_the_builders_nor_the_trainer_arithmetic(name):
    assert os.path.exists(os.path.join(CSRC, name)) and all(os.path.exists(os.path.join(CSRC, n)) for n in NOT_KEYED)
    seen = {os.path.basename(f) for f in _project_files(os.path.join(CSRC, name))}
    assert "aie_layout.h" in seen and not seen & set(NOT_KEYED), sorted(seen)


@pytest.mark.parametrize("name", KERNEL_FILES)
def test_no_kernel_file_sees_the_host_builders(name):
    """... and the trainer side's kernel files are the ones compiled from its arithmetic."""
    seen = {os.path.basename(f) for f in _project_files(os.path.join(CSRC, name))}
    assert "aie_layout.h" in seen and "aie_layout_build.h" not in seen, sorted(seen)
    assert ("aie_trainer_math.h" in seen) == (name not in STEP_SIDE), sorted(seen)


@pytest.mark.parametrize("lang", ["c99", "hip"])
@pytest.mark.parametrize("name", LAYOUT_HEADERS)
def test_each_layout_header_compiles_on_its_own(name, lang):
    """As C99 with the host C compiler, and as HIP (host and device passes: aie_layout_build.h is host code)."""
    if lang == "c99":
        # (aie_layout.h really alone: without what follows it for host C of before the cut, see the next test)
        cmd = ["gcc", "-std=c99", "-fsyntax-only", "-DAIE_LAYOUT_H_ONLY", "-I" + CSRC, "-I" + INCLUDE, "-x", "c"]
    else:
        cmd = [a for a in _hipcc() if a != "--cuda-device-only"] + ["-fsyntax-only", "-x", "hip"]
    r = subprocess.run(cmd + [os.path.join(CSRC, name)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_host_c_code_of_before_the_cut_still_compiles(tmp_path):
    """The suite and the restatement of the commit before the cut are run against this library unchanged; their C
    includes aie_layout.h alone (the plan shim: aie_trainer_plan.h alone) and calls the builders and the trainer
    helpers, so for host C that reaches aie_layout.h without having named the builders the other two follow (its last
    lines).  Behind aie_layout_build.h nothing follows: the spec generator compiles no trainer arithmetic."""
    uses = "void* uses[] = {(void*)aie_build_params, (void*)aie_mlp_row, (void*)aie_gae_step};\n"
    gcc = ["gcc", "-std=c99", "-fsyntax-only", "-I" + CSRC, "-I" + INCLUDE]
    for head, ok in (('#include "aie_layout.h"\n', True),
                     ('#include "aie_trainer_plan.h"\n', True),
                     ('#include "aie_layout_build.h"\n#include "aie_layout.h"\n', False)):
        src = tmp_path / "uses.c"
        src.write_text(head + uses)
        r = subprocess.run(gcc + [str(src)], capture_output=True, text=True)
        assert (r.returncode == 0) == ok, (head, r.stderr[-2000:])


def _jit_listed(name):
    """One of csrc/aie_jit.h's lists of file names (kSources, kSourcesOse, kSourcesGtb)."""
    with open(os.path.join(CSRC, "aie_jit.h")) as f:
        return re.findall(r'"([^"]+)"', re.search(name + r"\[\]\s*=\s*\{(.*?)\};", f.read(), re.S).group(1))


def _jit_units():
    """{"ose" / "gtb": (the unit's key list, its source string)} as csrc/aie_jit.h states them: the shared list plus the
    unit's own."""
    with open(os.path.join(CSRC, "aie_jit.h")) as f:
        text = f.read()
    listed = _jit_listed
    units = re.search(r'std::string src = ose \? ("(?:[^"\\]|\\.)*")\s*:\s*("(?:[^"\\]|\\.)*");', text)
    return {"ose": (listed("kSources") + listed("kSourcesOse"), ast.literal_eval(units.group(1))),
            "gtb": (listed("kSources") + listed("kSourcesGtb"), ast.literal_eval(units.group(2)))}


def test_specialisation_cache_key_covers_what_it_compiles(tmp_path):
    units = _jit_units()
    (tmp_path / "aie_jit_image.h").write_text(STUB_IMAGE)
    for which, (listed, unit) in units.items():  # each unit's key is its own
        assert "#define AIE_JIT 1" in unit and ("#define AIE_JIT_OSE 1" in unit) == (which == "ose"), unit
        src = tmp_path / ("aie_jit_%s.hip" % which)
        src.write_text(unit)
        compiled = _project_files(str(src), ["-I" + str(tmp_path)])
        compiled = {f for f in compiled if not f.startswith(os.path.realpath(str(tmp_path)) + os.sep)}
        keyed = {os.path.realpath(os.path.join(CSRC, s)) for s in listed} | {os.path.realpath(os.path.join(INCLUDE, "aie.h"))}
        assert len(listed) == len(set(listed)), listed
        assert compiled == keyed, (which, sorted(compiled - keyed), sorted(keyed - compiled))
        # the builders and the trainer arithmetic are not keyed because no unit is compiled from them
        assert "aie_layout.h" in listed and not {os.path.basename(f) for f in compiled} & set(NOT_KEYED), sorted(compiled)
    # the unit's own step / reset kernel files only: an edit to a trainer-side kernel file, or to the other scenario
    # family's, leaves a unit's cached code objects valid
    assert sorted(s for s in units["ose"][0] if s.endswith(".hip")) == ["aie_kernels_ose.hip"], units["ose"][0]
    assert sorted(s for s in units["gtb"][0] if s.endswith(".hip")) == ["aie_kernels.hip"], units["gtb"][0]
    # cutting the gather-trade-build unit into files leaves the other unit's key, and so its cached code objects, alone
    assert units["ose"][0] == _jit_listed("kSources") + ["aie_kernels_ose.hip"], units["ose"][0]
    assert sorted(units["gtb"][0]) == sorted(_jit_listed("kSources") + GTB_FILES), units["gtb"][0]


def test_library_staleness_hash_reads_what_the_library_is_compiled_from():
    from ai_economist_amd import _build

    compiled = _project_files(os.path.join(CSRC, "aie_capi.hip"))
    hashed = {os.path.realpath(f) for f in _build.source_files()}
    assert KERNEL_FILES and {os.path.realpath(os.path.join(CSRC, n)) for n in KERNEL_FILES} <= compiled  # (no dead kernel file)
    assert compiled <= hashed, sorted(compiled - hashed)
