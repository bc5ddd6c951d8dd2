"""Every gfx950 kernel of one build of libmadrl_hip.so (or of one object file) against another's: the procedure of
profiles/r13_hostage_crowd/README.md as a script.

    python scripts/kernels_vs_parent.py PARENT NEW [--filter SUBSTRING]

Both files are unbundled (`llvm-objdump --offloading`), every gfx950 code object is disassembled (`llvm-objdump -d`; per function the
mnemonics, operands and instruction encodings, addresses and symbol comments removed) and its per-kernel metadata read
(`llvm-readelf --notes`).  Prints the census (kernels in each, identical, missing, new) and, for the kernels that differ, a table of
instructions, VGPRs, SGPRs, scalars parked in VGPR lanes, private segment, VGPR spills and waves per SIMD (512 VGPRs over the count
rounded up to 8), parent -> new.  Exit status 0 always: it reports, the reader judges.
"""
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import isa   # noqa: E402  (the tests' reader of a library's notes)
from isa import LLVM   # noqa: E402


def kernels(path):
    """-> {mangled name: (tuple of instruction lines, {metadata})}"""
    out = {}
    meta = isa.built_kernels(path)
    with isa.code_objects(path) as cos:
        for co in cos:
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    cur = m.group(1)
                    if cur in meta:
                        out[cur] = ([], meta[cur])
                    continue
                if cur in out and "//" in line:
                    text, enc = line.split("//", 1)
                    enc = re.sub(r"<[^>]*>", "", enc.split(":", 1)[1] if ":" in enc else enc)   # drop the address and the symbol comment
                    out[cur][0].append(" ".join(text.split()) + " | " + " ".join(enc.split()))
    return {k: (tuple(v[0]), v[1]) for k, v in out.items()}


def demangle(names):
    tool = next((t for t in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if tool is None or not names:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, (re.sub(r"^void madrl::(\w+::)?", "", l).split("(madrl::")[0] for l in r.stdout.splitlines())))


def waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def main(argv):
    flt = argv[argv.index("--filter") + 1] if "--filter" in argv else ""
    a, b = kernels(argv[0]), kernels(argv[1])
    if flt:
        a = {k: v for k, v in a.items() if flt in k}
        b = {k: v for k, v in b.items() if flt in k}
    both = sorted(set(a) & set(b))
    same_dis = [k for k in both if a[k][0] == b[k][0]]
    same_meta = [k for k in both if a[k][1] == b[k][1]]
    differ = [k for k in both if a[k] != b[k]]
    print("%d kernels in the parent, %d here; %d identical in disassembly, %d identical in metadata, %d identical in both, %d missing, %d new"
          % (len(a), len(b), len(same_dis), len(same_meta), len(both) - len(differ), len(set(a) - set(b)), len(set(b) - set(a))))
    names = demangle(differ + sorted(set(a) ^ set(b)))
    for k in sorted(set(a) - set(b)):
        print("missing: " + names[k])
    for k in sorted(set(b) - set(a)):
        print("new: " + names[k])
    if differ:
        arrow = lambda x, y: str(x) if x == y else "%s -> %s" % (x, y)
        print("| kernel | instructions parent -> here | VGPRs | SGPRs | scalars parked in VGPR lanes | private segment | VGPR spills | waves per SIMD | LDS, kernel arguments |")
        print("|---|---|---|---|---|---|---|---|---|")
        for k in sorted(differ, key=lambda k: names[k]):
            ma, mb = a[k][1], b[k][1]
            print("| `%s` | %s | %s | %s | %s | %s | %s | %s | %s |" % (
                names[k], arrow(len(a[k][0]), len(b[k][0])), arrow(ma["vgprs"], mb["vgprs"]), arrow(ma["sgprs"], mb["sgprs"]),
                arrow(ma["sgpr_spills"], mb["sgpr_spills"]), arrow(ma["scratch"], mb["scratch"]), arrow(ma["vgpr_spills"], mb["vgpr_spills"]),
                arrow(waves(ma["vgprs"]), waves(mb["vgprs"])),
                "the parent's" if (ma["lds"], ma["kernarg"], ma["all_args"]) == (mb["lds"], mb["kernarg"], mb["all_args"]) else "CHANGED"))


if __name__ == "__main__":
    main(sys.argv[1:])
