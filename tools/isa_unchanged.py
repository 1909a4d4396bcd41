#!/usr/bin/env python3
"""Are the kernels a parent commit compiled byte-identical in this tree?  The three translation units that hold device code are
compiled device-only for gfx950 (-S, the library's flags, -Rpass-analysis=kernel-resource-usage) at the parent and here; the
assembly is cut into its functions and compared name by name, the resource remarks kernel by kernel.  Needs no GPU.

usage: tools/isa_unchanged.py PARENT_REV out.txt [table.md]   (the method of profiles/r09/isa_sweeps_unchanged.txt and profiles/r10/isa_unchanged.txt)
table.md, when given, receives one markdown row per kernel whose body or remarks differ: SGPRs, VGPRs, spills, scratch, occupancy and
LDS, parent / here (what profiles/rNN/README.md tabulates).
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from raftsql_amd import build as b  # noqa: E402

UNITS = ["raftq_capi.hip", "raftq_step.hip", "raftq_wire.hip"]


def compile_unit(root, unit, out):
    cmd = [b._hipcc(), f"--offload-arch={b.ARCH}", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(root, "include"),
           "-I" + os.path.join(root, "raftsql_amd", "csrc"), "--cuda-device-only", "-S", os.path.join(root, "raftsql_amd", "csrc", unit), "-o", out,
           "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit(p.stderr[-3000:])
    return p.stderr


def functions(asm):
    """{name: body} with the numbers the compiler gives a function by its position in the file blanked"""
    out = {}
    for m in re.finditer(r"; -- Begin function (\S+)\n(.*?); -- End function", asm, flags=re.S):
        body = re.sub(r"\.LBB\d+_|BB\d+_|\.Lfunc_begin\d+|\.Lfunc_end\d+|\.Ltmp\d+", "#", m.group(2))
        out[m.group(1)] = re.sub(r"[ \t]+", " ", body)
    return out


def remarks(err):
    """{kernel: its resource remarks as text}"""
    out, cur = {}, None
    for ln in err.splitlines():
        m = re.search(r"remark: (?:\s*)([A-Za-z ]+?)(?: \[[^\]]+\])?: (.*?) \[-Rpass", ln)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k == "Function Name":
            cur = v
            out[cur] = []
        elif cur is not None:
            out[cur].append("%s=%s" % (k, v))
    return {k: " ".join(v) for k, v in out.items()}


def table(changed):
    """markdown rows of [(demangled name, parent's remarks, this tree's)]"""
    keys = ("TotalSGPRs", "VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")
    rows = ["| kernel | " + " | ".join(k + (" parent / here" if i == 0 else "") for i, k in enumerate(keys)) + " |", "|" + "---|" * (len(keys) + 1)]
    seen = set()
    for name, r0, r1 in changed:
        if name in seen:  # (a kernel of a shared header is compiled into more than one unit)
            continue
        seen.add(name)
        d0, d1 = ({k.strip(): v for k, v in re.findall(r"([A-Za-z][A-Za-z ]*)=(\S+)", r)} for r in (r0, r1))
        get = lambda d, k: d.get(k, "-")  # noqa: E731
        rows.append("| `%s` | " % name + " | ".join("%s / %s" % (get(d0, k), get(d1, k)) for k in keys) + " |")
    return "\n".join(rows) + "\n"


def digest(fns, names):
    h = hashlib.sha256()
    for n in sorted(names):
        h.update(n.encode() + b"\0" + fns[n].encode() + b"\0")
    return h.hexdigest()[:32]


def main():
    parent, out_path = sys.argv[1], sys.argv[2]
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", parent], capture_output=True, text=True, check=True).stdout.strip()
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "parent")
        os.makedirs(old)
        ar = subprocess.run(["git", "-C", ROOT, "archive", parent, "include", "raftsql_amd/csrc"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=ar, check=True)
        jobs = [(side, root, u) for side, root in (("parent", old), ("here", ROOT)) for u in UNITS]
        with ThreadPoolExecutor(len(jobs)) as ex:
            errs = list(ex.map(lambda j: compile_unit(j[1], j[2], os.path.join(tmp, j[0] + "_" + j[2] + ".s")), jobs))
        res = {(j[0], j[2]): (functions(open(os.path.join(tmp, j[0] + "_" + j[2] + ".s")).read()), remarks(e)) for j, e in zip(jobs, errs)}
    lines = ["raftq_capi.hip, raftq_step.hip and raftq_wire.hip -- the three translation units that hold device code -- compiled device-only",
             "for gfx950 with the library's flags (raftsql_amd/build.py: -O3 -std=c++17 -fPIC, --cuda-device-only -S) and",
             "-Rpass-analysis=kernel-resource-usage, at the parent commit (%s) and at this tree (tools/isa_unchanged.py).  Needs no GPU." % rev,
             b.toolchain()["version"][0], "",
             "The assembly is cut into its functions (\"; -- Begin function NAME\" .. \"; -- End function\": the instructions, the kernel",
             "descriptor, the compiler's per-function comments), the two sides compared name by name after blanking the numbers the compiler",
             "gives a function by its position in the file (.LBB<k>_, BB<k>_, .Lfunc_begin<k>, .Lfunc_end<k>, .Ltmp<k>) and making runs of",
             "blanks one blank; the resource remarks (SGPRs, VGPRs, AGPRs, scratch, occupancy, spills, LDS) compared kernel by kernel as text.", ""]
    bad = 0
    changed = []
    for u in UNITS:
        (f0, r0), (f1, r1) = res[("parent", u)], res[("here", u)]
        missing = sorted(set(f0) - set(f1))
        differ = sorted(n for n in f0 if n in f1 and f0[n] != f1[n])
        rdiff = sorted(k for k in r0 if r1.get(k) != r0[k])
        new = sorted(set(f1) - set(f0))
        bad += len(missing) + len(differ) + len(rdiff)
        base = lambda k: subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip().split("(")[0]  # noqa: E731
        for k in sorted(set(differ + rdiff) & set(r0) & set(r1)):
            changed.append((base(k), r0[k], r1[k]))
        renamed = {base(k): k for k in new if k in r1}  # a kernel whose signature changed has another mangled name
        for k in missing:
            if k in r0 and base(k) in renamed:
                changed.append((base(k) + " (new signature)", r0[k], r1[renamed[base(k)]]))
        dem = subprocess.run(["c++filt"] + new, capture_output=True, text=True).stdout.split("\n") if new else []
        common = [n for n in f0 if n in f1]
        lines += ["%s: %d kernels with resource remarks at the parent, %d here; %d functions at the parent, %d here" % (u, len(r0), len(r1), len(f0), len(f1)),
                  "    missing here: %d; bodies that differ: %d; kernels whose remarks differ: %d" % (len(missing), len(differ), len(rdiff)),
                  "    sha256 over the parent's names, parent / here: %s / %s" % (digest(f0, common), digest(f1, common)),
                  "    new here: %s" % (", ".join(d for d in dem if d) or "none")]
        lines += ["    DIFFERS: " + n for n in missing + differ + rdiff]
    lines.append("")
    lines.append("every function the parent compiled is unchanged" if bad == 0 else "%d functions CHANGED" % bad)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(table(changed))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
