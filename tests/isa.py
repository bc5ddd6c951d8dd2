"""What the CPU tests of emitted gfx950 code and of the built code objects share (a plain module, no test file and no conftest):
  * compile_asm: a translation unit through the build's own compiler and flags to assembly text, once per process;
  * kernel_body / kernel_insts / kernel_meta: one kernel's lines, instructions and amdhsa.kernels entry of such a text;
  * blocks / env_loop / before_env_loop: the basic blocks with LLVM's loop annotations, and the env loop found from them;
  * salu: which instructions are issued on the scalar ALU;
  * mangled: the Itanium name of a Pursuit kernel instantiation;
  * built_kernels: the notes of every gfx950 kernel of libmadrl_hip.so, read once per process;
  * def_lines: a csrc/*.def list;  masked_spills: scripts/find_masked_spills.py over a text.
scripts/kernels_vs_parent.py reads its metadata through built_kernels as well."""
import contextlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import find_masked_spills   # noqa: E402

CSRC = os.path.join(ROOT, "madrl_amd", "csrc")
SO = os.path.join(ROOT, "madrl_amd", "libmadrl_hip.so")
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


# ------------------------------------------------------------------ names
WAVE_ARGS = "NS0_7WaveDevENS0_6WaveIOE"                 # (const WaveDev, const WaveIO): pursuit_wave_kernel and pursuit_group_kernel
CROWD_ARGS = "NS0_8CrowdDevENS0_7CrowdIOE"              # (const CrowdDev, const CrowdIO): pursuit_crowd_kernel
LIVE_CROWD_ARGS = CROWD_ARGS + "PKi"                    # ... and the pending counts, const int32_t *: pursuit_live_crowd_kernel


def mangled(ns, kernel, shape, ints, tail, params):
    """the Itanium name of madrl::NS::KERNEL<NS::SHAPE<ints...>, tail...>(params): tail holds the template arguments after the shape,
    ints and bools; params is the mangled parameter list (WAVE_ARGS, CROWD_ARGS, LIVE_CROWD_ARGS)"""
    lit = lambda v: ("Lb%dE" if isinstance(v, bool) else "Li%dE") % v
    return "_ZN5madrl2%s%d%sINS0_%d%sI%sEE%sEEv%s" % (ns, len(kernel), kernel, len(shape), shape, "".join(lit(v) for v in ints),
                                                     "".join(lit(v) for v in tail), params)


def wave_kernel(shape, ints, inject=False):
    """pw::pursuit_wave_kernel<SHAPE<ints>, 1, INJECT, false>: the step launch (MODE 1) without the controller"""
    return mangled("pw", "pursuit_wave_kernel", shape, ints, (1, inject, False), WAVE_ARGS)


def group_kernel(shape, ints, inject=False):
    """pw::pursuit_group_kernel<SHAPE<ints>, 1, INJECT>"""
    return mangled("pw", "pursuit_group_kernel", shape, ints, (1, inject), WAVE_ARGS)


def crowd_kernel(ints, mode, live=False):
    """pc::pursuit_crowd_kernel<CShape<ints>, MODE> or, with per-env agent counts, pc::pursuit_live_crowd_kernel<LCShape<ints>, MODE>"""
    if live:
        return mangled("pc", "pursuit_live_crowd_kernel", "LCShape", ints, (mode,), LIVE_CROWD_ARGS)
    return mangled("pc", "pursuit_crowd_kernel", "CShape", ints, (mode,), CROWD_ARGS)


# ------------------------------------------------------------------ the headline instantiation (BASELINE configs[1])
SHAPE = (16, 16, 8, 30, 7, 1)    # XS, YS, P, E, obs_range, flatten
NS = 5                           # float4 slots per lane: 8 pursuers x 37 float4 = 296 slots over 64 lanes
VM_PER_ENV = 5 * NS + 6          # global stores per env; the record prefetch is waited for with exactly s_waitcnt vmcnt(VM_PER_ENV)
HEADLINE_VGPRS = 96              # five wavefronts per SIMD
HEADLINE = wave_kernel("Shape", SHAPE)
HEADLINE_TU = """#include "common.hpp"
#include "pursuit_wave.hpp"
namespace madrl { namespace pw {
template __global__ void pursuit_wave_kernel<Shape<%d, %d, %d, %d, %d, %d>, 1, false, false>(const WaveDev, const WaveIO);
} }
""" % SHAPE


def group_tu(kernels, inject):
    """the translation unit that instantiates pw::pursuit_group_kernel<KIND<cap...>, 1, INJECT> for every (kind, cap) of kernels"""
    lines = ["template __global__ void pursuit_group_kernel<%s<%d, %d, %d, %d, %d, %d, %d>, 1, %s>(const WaveDev, const WaveIO);\n"
             % ((kind,) + cap + ("true" if inject else "false",)) for kind, cap in kernels]
    return '#include "common.hpp"\n#include "pursuit_group.hpp"\nnamespace madrl { namespace pw {\n' + "".join(lines) + "} }\n"


# ------------------------------------------------------------------ compiling
_ASM = {}


def compile_asm(tu_text, extra_flags=(), path=None):
    """the gfx950 assembly of a translation unit given as text -- or, with tu_text None, of the source file at path -- compiled with the
    build's own compiler and flags (without -Wall) and extra_flags; each distinct request is compiled once per process"""
    key = (tu_text, tuple(extra_flags), path)
    if key not in _ASM:
        import pytest
        from madrl_amd import build as B
        if not os.path.exists(B.HIPCC):
            pytest.skip("no hipcc")
        with tempfile.TemporaryDirectory() as tmp:
            src, out = path or os.path.join(tmp, "tu.hip"), os.path.join(tmp, "tu.s")
            if path is None:
                with open(src, "w") as f:
                    f.write(tu_text)
            subprocess.run([B.HIPCC] + [f for f in B.FLAGS if f != "-Wall"] + list(extra_flags) +
                           ["-I", B.CSRC, "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
            with open(out) as f:
                _ASM[key] = f.read()
    return _ASM[key]


def masked_spills(text, want=""):
    """scripts/find_masked_spills.py over the kernels of an assembly text whose names contain want"""
    return find_masked_spills.scan_text(text, want)


# ------------------------------------------------------------------ one kernel of an assembly text
def kernel_body(text, name):
    """the lines of the kernel with that mangled name, from its label up to .Lfunc_end"""
    lines = text.split("\n")
    at = [i for i, l in enumerate(lines) if l.startswith(name + ":")]
    if len(at) != 1:
        raise LookupError("%d kernels named %s in the assembly" % (len(at), name))
    end = next(i for i in range(at[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[at[0]:end]


def _inst(line):
    """the instruction of an assembly line, without its comment; None for labels, directives, comments and empty lines"""
    t = line.strip()
    return t.split(";")[0].strip() if t and not t.startswith((";", ".", "//")) else None


def kernel_insts(text, name):
    return [i for i in map(_inst, kernel_body(text, name)[1:]) if i is not None]


def kernel_meta(text, name):
    """that kernel's entry of amdhsa.kernels as a dict of its integer fields (vgpr_count, sgpr_count, vgpr_spill_count, sgpr_spill_count,
    private_segment_fixed_size, group_segment_fixed_size, kernarg_segment_size, ...); the fields of its arguments are left out"""
    entries = re.split(r"\n  - (?=\.)", text[text.index("amdhsa.kernels:"):])[1:]   # one list item per kernel
    mine = [e for e in entries if re.search(r"^ *\.name:\s+%s$" % re.escape(name), e, re.M)]
    if len(mine) != 1:
        raise LookupError("%d entries named %s in amdhsa.kernels" % (len(mine), name))
    return {k: int(v) for k, v in re.findall(r"^(?: {4})?\.(\w+):\s+(\d+)\s*$", mine[0], re.M)}


# ------------------------------------------------------------------ basic blocks and loops
def blocks(body):
    """the basic blocks of a kernel body in layout order: dicts of name (the BBn_m of a label, None for the entry and for fall-through
    blocks), notes (the label line and LLVM's loop annotations after it) and insts"""
    out, cur, annotating = [], None, False
    for l in body:
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", l)
        if m:
            cur, annotating = dict(name=m.group(1), notes=l, insts=[]), True
            out.append(cur)
        elif cur is not None:
            t = l.strip()
            if t.startswith(";") and annotating:
                cur["notes"] += " " + t   # the annotation lines right after the label
            elif _inst(l) is not None:
                annotating = False
                cur["insts"].append(_inst(l))
    return out


def _header(b):
    """the header of the innermost loop a block is in (LLVM annotates each block with it), the block itself if it is one"""
    m = re.search(r"Header=(BB\d+_\d+)", b["notes"])
    return m.group(1) if m else b["name"]


def _parents(b):
    """of a loop header: the headers of the loops around it, outermost first"""
    return re.findall(r"Parent Loop (BB\d+_\d+)", b["notes"])


def loop_blocks(blks, header):
    """the blocks of the loop with that header, inner loops included (each inner loop header is annotated with its parent loops)"""
    headers = {header} | {b["name"] for b in blks if b["name"] and header in _parents(b)}
    return [b for b in blks if _header(b) in headers]


def exact_wait(n):
    """home block of the env loop, the wave rule: it holds the record prefetch's exact wait"""
    return lambda b: "s_waitcnt vmcnt(%d)" % n in b["insts"]


def nt_float4_store(b):
    """home block of the env loop, the store rule: it holds a non-temporal float4 store (an observation store)"""
    return any(i.startswith("global_store_dwordx4") and i.endswith(" nt") for i in b["insts"])


def env_loop(blks, home, once=None):
    """the instructions of the outermost loop around the first block that home selects, inner loops included.  With once, a message:
    home must select exactly one block"""
    homes = [b for b in blks if home(b)]
    assert once is None or len(homes) == 1, once
    assert homes, "no block of the kernel is the env loop's home"
    head = next((b for b in blks if b["name"] == _header(homes[0])), homes[0])
    return [i for b in loop_blocks(blks, (_parents(head) or [head["name"]])[0]) for i in b["insts"]]


def wave_env_loop(text, name, n):
    """the env loop of a one-wavefront kernel: the loop that holds the one exact wait s_waitcnt vmcnt(n)"""
    return env_loop(blocks(kernel_body(text, name)), exact_wait(n), once="the record prefetch's exact wait vmcnt(%d) must appear once" % n)


def store_env_loop(text, name):
    """the env loop of a multi-wavefront kernel: the outermost loop around the observation stores (global_store_dwordx4 ... nt)"""
    return env_loop(blocks(kernel_body(text, name)), nt_float4_store)


def before_env_loop(blks):
    """-> (blocks before the env loop, names of the loop headers among them).  The env loop is the one outermost loop (Depth=1 header)
    that holds global stores; 'before' = not in that loop and laid out before its header."""
    heads = [b["name"] for b in blks if "Loop Header: Depth=1" in b["notes"]]
    env = [h for h in heads if any(i.startswith("global_store") for b in loop_blocks(blks, h) for i in b["insts"])]
    assert len(env) == 1, "expected one top-level loop with global stores (the env loop), found %r" % env
    at = next(i for i, b in enumerate(blks) if b["name"] == env[0])
    inside = loop_blocks(blks, env[0])
    pre = [b for b in blks[:at] if not any(b is x for x in inside)]
    assert pre, "no code before the env loop?"
    return pre, [b["name"] for b in pre if "Loop Header" in b["notes"]]


# not issued on the scalar ALU: waits, nops, branches, scalar memory, barriers
NOT_SALU = ("s_waitcnt", "s_nop", "s_branch", "s_cbranch", "s_load", "s_buffer", "s_barrier", "s_setprio", "s_sleep", "s_endpgm")


def salu(insts):
    return [i for i in insts if i.startswith("s_") and not i.startswith(NOT_SALU)]


# ------------------------------------------------------------------ the built library
@contextlib.contextmanager
def code_objects(path):
    """the gfx950 code objects of a library or object file, unbundled into a directory that lives as long as the with block"""
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(path, tmp)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", os.path.basename(path)], cwd=tmp, check=True, capture_output=True)
        yield [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if f.endswith("gfx950")]


NOTES = (("scratch", "private_segment_fixed_size"), ("vgpr_spills", "vgpr_spill_count"), ("vgprs", "vgpr_count"), ("sgprs", "sgpr_count"),
         ("sgpr_spills", "sgpr_spill_count"), ("lds", "group_segment_fixed_size"), ("kernarg", "kernarg_segment_size"))
_BUILT = {}


def built_kernels(path=SO):
    """kernel name -> the NOTES fields of its entry in the notes of the built library's gfx950 code objects, args (the (offset, size)
    of its by-value arguments) and all_args ((offset, size, value_kind) of every argument); read once per process and library"""
    tools = [os.path.join(LLVM, t) for t in ("llvm-objdump", "llvm-readelf")]
    if not all(os.path.exists(f) for f in [path] + tools):
        import pytest
        pytest.skip("built library or llvm tools not available")
    key = (os.path.abspath(path), os.path.getmtime(path))
    if key not in _BUILT:
        out = {}
        with code_objects(path) as cos:
            for co in cos:
                notes = subprocess.run([tools[1], "--notes", co], capture_output=True, text=True, check=True).stdout
                for blk in re.split(r"\n  - \.agpr_count:", notes)[1:]:
                    name = re.search(r"\.name:\s+(\S+)", blk)
                    if not name:
                        continue
                    k = {short: int(re.search(r"\.%s:\s+(\d+)" % field, blk).group(1)) for short, field in NOTES}
                    k["all_args"] = tuple((int(o), int(s), kind) for o, s, kind in
                                          re.findall(r"- \.offset:\s+(\d+)\s+\.size:\s+(\d+)\s+\.value_kind:\s+(\w+)", blk))
                    k["args"] = [(o, s) for o, s, kind in k["all_args"] if kind == "by_value"]
                    out[name.group(1)] = k
        assert out, "no gfx950 kernels found in the library"
        _BUILT[key] = out
    return _BUILT[key]


# ------------------------------------------------------------------ the lists
def def_lines(name, kinds=None):
    """the lines KIND(int, ...) of csrc/NAME as {kind: [tuples in file order]}: an entry for each of kinds, or for every kind the file has"""
    out = {k: [] for k in kinds or ()}
    for m in re.finditer(r"^\s*([A-Z]+)\(([^)]*)\)", open(os.path.join(CSRC, name)).read(), re.M):
        if kinds is None or m.group(1) in kinds:
            out.setdefault(m.group(1), []).append(tuple(int(v) for v in m.group(2).split(",")))
    return out
