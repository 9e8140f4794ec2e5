"""Device code of two source trees, kernel by kernel (no GPU needed):

    python tools/isa_compare.py <parent csrc dir> <result csrc dir> file.hip [file.hip ...]

Compiles each file of both trees with the library's own flags plus --cuda-device-only -S -Rpass-analysis=kernel-resource-usage, normalises
the assembly as profiles/gemm_one_plan.txt describes (__hip_cuid_*, the function index in block labels, column padding; instructions =
lines that are neither labels, directives nor comments) and reports per kernel and instantiation: identical text or not, the
instruction counts, and VGPRs / AGPRs / SGPRs / scratch / occupancy / static LDS of both."""
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from divergen_amd.csrc.build import FLAGS, HIPCC  # noqa: E402

KEYS = ("VGPRs", "AGPRs", "SGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def compile_s(path):
    p = subprocess.run([HIPCC] + FLAGS + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", "-", path],
                       capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(p.stderr[-2000:])
    return p.stdout, p.stderr


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool] + names, capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(asm):
    """name -> normalised instruction lines"""
    res, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L") and ("; @" + m.group(1)) in line:
            cur = m.group(1)
            res[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].strip()
        if not s or s.endswith(":") or s.startswith("."):
            continue
        s = re.sub(r"__hip_cuid_\w+", "__hip_cuid", s)
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        res[cur].append(re.sub(r"\s+", " ", s))
    return res


def resources(remarks):
    res, cur = {}, None
    for line in remarks.split("\n"):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        for k in KEYS:
            m = re.search(re.escape(k) + r": (\d+)", line)
            if m and cur and k not in res[cur]:
                res[cur][k] = int(m.group(1))
    return res


def main():
    a_dir, b_dir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    for f in files:
        (a_s, a_r), (b_s, b_r) = compile_s(os.path.join(a_dir, f)), compile_s(os.path.join(b_dir, f))
        ka, kb, ra, rb = kernels(a_s), kernels(b_s), resources(a_r), resources(b_r)
        ka = {k: v for k, v in ka.items() if k in ra}
        kb = {k: v for k, v in kb.items() if k in rb}
        names = demangle(sorted(set(ka) | set(kb)))
        same = [k for k in ka if k in kb and ka[k] == kb[k]]
        print("%s: %d -> %d kernels, %d with identical text" % (f, len(ka), len(kb), len(same)))
        for k in sorted(set(ka) | set(kb)):
            nm = re.sub(r"^void ", "", names[k].replace("(anonymous namespace)::", "")).split("(")[0]
            if k not in kb or k not in ka:
                print("  %-9s %s" % ("gone" if k not in kb else "new", nm))
                bad += 1
                continue
            req = ra[k] == rb[k]
            r = " ".join("%s %d" % (key.split(" ")[0], ra[k].get(key, -1)) for key in KEYS)
            if ka[k] == kb[k] and req:
                print("  identical %-44s instructions %5d   %s" % (nm, len(ka[k]), r))
            else:
                bad += 1
                print("  DIFFERS   %-44s instructions %5d -> %5d   resources %s: %s | %s" % (
                    nm, len(ka[k]), len(kb[k]), "equal" if req else "DIFFER", r,
                    " ".join("%s %d" % (key.split(" ")[0], rb[k].get(key, -1)) for key in KEYS)))
    print("kernels that differ, appear or disappear: %d" % bad)


if __name__ == "__main__":
    main()
