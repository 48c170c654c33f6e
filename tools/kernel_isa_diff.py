"""Are kernels of two builds the same instructions?  Compares, kernel by kernel, two device assembly files of
csrc/aie_capi.hip (hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude --cuda-device-only -S ... -o X.s; the file
tools/kernel_asm_stats.py leaves in the temporary directory is one) after dropping comments, directives and label numbers.
Kernels are paired by their demangled names up to the template arguments the newer build added at the end
(`foo<6, 5>` ~ `foo<6, 5, false>`, `foo` ~ `foo<false>`).  The translation unit's id (`__hip_cuid_*`, a hash of the
compile's input) is no function and is left out.

   python tools/kernel_isa_diff.py before.s after.s [substring of the kernels' names, default sample_policy;
                                                     "" compares every kernel and device function]"""
import difflib
import re
import subprocess
import sys


def bodies(path, want):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^([A-Za-z_]\w*):", line)
        if m and not line.startswith(".L"):
            cur = m.group(1) if want in m.group(1) and not m.group(1).startswith("__hip_cuid_") else None
            if cur:
                out[cur] = []
            continue
        t = line.strip()
        if cur is None or not t or t.startswith((";", "//", ".")):
            if t.startswith(".Lfunc_end"):
                cur = None
            continue
        t = re.sub(r"\s*;.*$", "", t)
        out[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", t)))
    names = subprocess.run(["c++filt"] + list(out), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"^void ", "", re.sub(r"\(.*", "", n)): b for n, b in zip(names, out.values())}


def main():
    want = sys.argv[3] if len(sys.argv) > 3 else "sample_policy"
    old, new = bodies(sys.argv[1], want), bodies(sys.argv[2], want)
    differ = 0
    for name, body in sorted(old.items()):
        cands = [n for n in new if n == name or n == name + "<false>" or (name.endswith(">") and n == name[:-1] + ", false>")]
        if len(cands) != 1:
            print("%-64s no counterpart" % name[:64])
            differ += 1
            continue
        same = body == new[cands[0]]
        differ += not same
        print("%-64s %5d instructions  %s" % (name[:64], len(body), "identical" if same else "DIFFERENT (%d)" % len(new[cands[0]])))
        if not same:
            for ln in list(difflib.unified_diff(body, new[cands[0]], lineterm="", n=1))[:20]:
                print("      " + ln)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
