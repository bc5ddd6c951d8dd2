"""Build libmadrl_hip.so in-tree with hipcc for gfx950 (no GPU needed: hipcc cross-compiles).

    python -m madrl_amd.build [--force]
    python -m madrl_amd.build --pursuit-shape XS YS N_PURSUERS N_EVADERS OBS_RANGE FLATTEN      # give this shape the fast path, rebuild
    python -m madrl_amd.build --pursuit-live-shape XS YS N_PURSUERS N_EVADERS OBS_RANGE FLATTEN # ... and per-env agent counts at this capacity
    python -m madrl_amd.build --pursuit-crowd-shape XS YS N_PURSUERS N_EVADERS OBS_RANGE FLATTEN # more than 64 pursuers or evaders: the crowd kernel
    python -m madrl_amd.build --pursuit-live-crowd-shape XS YS N_PURSUERS N_EVADERS OBS_RANGE FLATTEN # ... and per-env agent counts on it
    python -m madrl_amd.build --pursuit-to-shape XS YS N_PURSUERS N_EVADERS OBS_RANGE FLATTEN   # the two-buffer step (step_to) on this shape's fast kernel
    python -m madrl_amd.build --pursuit-to-group-shape XS YS N_PURSUERS N_EVADERS OBS_RANGE FLATTEN [LIVE] # ... of a multi-wavefront shape (LIVE 1: with per-env agent counts)
    python -m madrl_amd.build --pursuit-to-group-f16-shape XS YS N_PURSUERS N_EVADERS OBS_RANGE FLATTEN [LIVE] # the half-precision step_to (obs_dtype=torch.float16) of a multi-wavefront shape
    python -m madrl_amd.build --waterworld-shape N_PURSUERS N_EVADERS N_POISON N_SENSORS [OBS_DIM]   # refused when it cannot be built (waterworld_shape_refusal)

The fast paths (one wavefront -- or a group of wavefronts -- per env, everything about the shape a compile-time constant) exist for the
shapes listed in csrc/*_specializations.def: the BASELINE configurations, the reference's own runner / script defaults, the test shapes.
Any other shape runs on the generic kernels, at about half the speed.  The options above append a line to
csrc/*_specializations.local.def (git-ignored, included after the committed list) and rebuild the one object that changed (~30 s).

-ffp-contract=off: reward arithmetic and the reset window are float64 expressions that must
round step by step like NumPy does in the reference; an FMA contraction would change bits.
"""
import collections
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libmadrl_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fno-fast-math", "-Wall", "-Wno-unused-function",
         "-Wno-pass-failed"]   # (`#pragma unroll` on loops whose bounds are only known in the specialised instantiations: the generic ones stay rolled)
# per-source additions.  multiwalker: the SLP vectorizer pairs the solver's scalar float math into packed-fp32 instructions, which
# need every loop constant replicated into register pairs -- the 180-sweep loop then runs out of VGPRs (AGPR copies, scratch)
# pursuit_to_f16_live: the default scalar register allocator leaves the kernel a private segment that nothing touches (see the file's head)
EXTRA_FLAGS = {"multiwalker_c": ["-fno-slp-vectorize"],   # file-name prefix -> flags (the capacity classes multiwalker_c4 / _c8 / _c10.hip)
               "pursuit_to_f16_live": ["-mllvm", "-sgpr-regalloc=basic"]}


def pursuit_fast_path(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id=True):
    """-> ("X", None) one wavefront per env, ("XG", NW) NW wavefronts per env, or (None, why not): the static_asserts of
    pursuit_wave.hpp / pursuit_group.hpp, evaluated here so that a shape that cannot have a fast path is refused before it breaks the build"""
    P, E, R = int(n_pursuers), int(n_evaders), int(obs_range)
    A = P + E
    if R % 2 == 0:
        return None, "even obs_range"
    if flatten and not include_id:
        return None, "flatten without the id: rows are not whole float4s"
    if P > 64 or E > 64 or A > 128:
        return None, "more than 64 pursuers or evaders (or 128 agents)"
    D = 3 * R * R + 1 if flatten else 4 * R * R
    if D % 4:
        return None, "observation row is not a whole number of float4"
    # one wavefront per env when the agents fit its lanes AND the row fits 8 float4 slots per lane (slot constants in registers,
    # pursuit_wave.hpp); otherwise two wavefronts (pursuit_group.hpp) -- four for long rows, whose slot constants come from an LDS table ("LONG ROWS": more than 8 slots per thread of two wavefronts), up to 32 slots per thread
    slots = lambda n: (P * (D // 4) + 64 * n - 1) // (64 * n)
    nw = 1 if (A <= 64 and slots(1) <= 8) else (2 if slots(2) <= 8 else 4)   # long rows: four wavefronts share the env's LDS (occupancy is LDS-bound there)
    if slots(nw) > 32:
        return None, "more than 32 float4 slots per thread (n_pursuers x row length too large)"
    pad = max((R - 1) // 2, 1)
    gsz = ((xs + 2 * pad) * (ys + 2 * pad) + 3) // 4 * 4
    tabled = slots(nw) > 8
    if (3 * gsz + 2 + P + 72 + (xs * ys + 3) // 4 + 2 * P + 16 + (2 * (D // 4) if tabled else 0)) * 4 > 64 * 1024:
        return None, "map too large for the LDS layers"
    if tabled and 3 * gsz + 2 + P >= 32768:
        return None, "map too large for the 15-bit offsets of the long-row table"
    ngw, ntw = max((E + 31) // 32, 1), (A + 31) // 32
    rec = ((16 + 2 * A + 3) // 4 * 4 + 4 * ngw + 4 * ntw + 15) // 16 * 16
    if rec > 256:
        return None, "state record above 256 bytes"
    return ("X", None) if nw == 1 else ("XG", nw)


def pursuit_crowd_lds_bytes(xs, ys, n_pursuers, n_evaders, obs_range, flatten):
    """the static LDS of the crowd kernel's workgroup (CShape::LDS_DWORDS, pursuit_crowd.hpp): one dword per cell of the padded map, the value
    table, the agents' bytes and words"""
    P, E, R = int(n_pursuers), int(n_evaders), int(obs_range)
    A = P + E
    up = lambda v, a: (v + a - 1) // a * a
    pad = max((R - 1) // 2, 1)
    D = 3 * R * R + 1 if flatten else 4 * R * R
    ngw, ntw = max((E + 31) // 32, 1), (A + 31) // 32
    dwords = (up((xs + 2 * pad) * (ys + 2 * pad), 16) + 256 + (up(D, 4) if flatten else 0) + 2 * up(P, 2) + 2 * up(P, 4) + 2 * up(ngw, 4) +
              up(ntw, 4) + 8 + 2 * up(A, 16) // 4)
    return 4 * dwords


def pursuit_crowd_path(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id=True):
    """-> ("XC", NW): the crowd kernel (pursuit_crowd.hpp: agents looped over the threads of NW wavefronts, any count up to 1 023 of a kind)
    can be compiled for this shape, or (None, why not): the static_asserts of CShape, evaluated here.  It says nothing about the X / XG fast
    paths (pursuit_fast_path): a shape that has one of those keeps it."""
    xs, ys, P, E, R = int(xs), int(ys), int(n_pursuers), int(n_evaders), int(obs_range)
    if R % 2 == 0:
        return None, "even obs_range"
    if flatten and not include_id:
        return None, "flatten without the id: rows are not whole float4s"
    if not (1 <= P <= 1023 and 0 <= E <= 1023):
        return None, "more than 1 023 pursuers or evaders"
    if not (1 <= xs <= 255 and 1 <= ys <= 255):
        return None, "coordinates above 255 do not fit the bytes of the state record"
    D = 3 * R * R + 1 if flatten else 4 * R * R
    if D % 4:
        return None, "observation row is not a whole number of float4"
    lds = pursuit_crowd_lds_bytes(xs, ys, P, E, R, flatten)
    if lds > 160 * 1024:
        return None, "map too large for the LDS cells (%d bytes, a workgroup may declare 163 840)" % lds
    # wavefronts per env.  Short rows: one or two -- the dynamics are a chain of a dozen barriers, and many small workgroups per CU hide it
    # better than few large ones (measured, scripts/crowd_time.py at 16 384 envs: 20 v 300 on 24 x 24 takes 207 us per step with four
    # wavefronts, 184 with one).  Long rows: eight while three such workgroups fit a CU, sixteen when the cells of one env fill most of
    # it (occupancy then comes from the workgroup itself)
    slots = P * (D // 4)
    return "XC", (1 if slots <= 2048 else 2 if slots <= 8192 else (8 if lds <= 40 * 1024 else 16))


def _append_local(def_name, line):
    path = os.path.join(CSRC, def_name.replace(".def", ".local.def"))
    committed = open(os.path.join(CSRC, def_name)).read() + (open(path).read() if os.path.exists(path) else "")
    norm = lambda t: "".join(t.split())
    if norm(line.split("//")[0]) in norm(committed):
        return False
    with open(path, "a") as f:
        f.write(line + "\n")
    return True


def _add(*pairs):
    """append each (list file, line) to the local companion of that list unless the lists hold the line already -> whether anything was added"""
    return any([_append_local(name, line + "   // added by madrl_amd.build") for name, line in pairs])


class _Shape(collections.namedtuple("_Shape", "kind nw args why_wave why_crowd")):
    """a shape, classified once (_classify).  kind, nw: the family that takes it -- "X" (nw None), "XG" or, for a shape without an X / XG fast
    path, "XC", with its NW -- or None; args: the numbers of its line, that NW included; why_wave / why_crowd: what pursuit_fast_path /
    pursuit_crowd_path refuse it for, or None"""
    def line(self, macro):
        return "%s(%s)" % (macro, self.args)


def _classify(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id=True):
    (kind, nw), (ckind, cnw) = (f(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id) for f in (pursuit_fast_path, pursuit_crowd_path))
    why_wave, why_crowd = nw if kind is None else None, cnw if ckind is None else None
    if kind is None:
        kind, nw = ckind, None if ckind is None else cnw
    args = "%d, %d, %d, %d, %d, %d" % (xs, ys, n_pursuers, n_evaders, obs_range, int(bool(flatten))) + ("" if nw is None else ", %d" % nw)
    return _Shape(kind, nw, args, why_wave, why_crowd)


def add_pursuit_shape(xs, ys, n_pursuers, n_evaders, obs_range, flatten):
    c = _classify(xs, ys, n_pursuers, n_evaders, obs_range, flatten)
    if c.why_wave is not None:
        raise ValueError("no fast path for this PursuitEvade shape: %s (it runs on the generic kernel)" % c.why_wave)
    return _add(("pursuit_specializations.def", c.line(c.kind)))


def add_pursuit_crowd_shape(xs, ys, n_pursuers, n_evaders, obs_range, flatten):
    kind, nw = pursuit_crowd_path(xs, ys, n_pursuers, n_evaders, obs_range, flatten)   # (also for a shape that has an X / XG fast path)
    if kind is None:
        raise ValueError("no crowd kernel for this PursuitEvade shape: %s (it runs on the generic kernel)" % nw)
    return _add(("pursuit_crowd_specializations.def", "XC(%d, %d, %d, %d, %d, %d, %d)" % (xs, ys, n_pursuers, n_evaders, obs_range, int(bool(flatten)), nw)))


def pursuit_live_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id=True):
    """-> (live line, fixed line) that give a per-env-counts capacity its fast path: XL(...) over an X(...) shape, XLG(..., NW) over an
    XG(..., NW) shape -- or None when the capacity has no fast path at all (pursuit_fast_path says why).  Pure: nothing is written."""
    c = _classify(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id)
    return (c.line("XL" + c.kind[1:]), c.line(c.kind)) if c.kind in ("X", "XG") else None


def add_pursuit_live_shape(xs, ys, n_pursuers, n_evaders, obs_range, flatten):
    """per-env agent counts at this capacity on the fast path: the live line in the local live list, and the fixed-shape line it stands on
    in the local fixed list if it is missing"""
    lines = pursuit_live_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten)
    if lines is None:
        raise ValueError("no fast path for this PursuitEvade capacity: %s (per-env agent counts run on the generic kernel)"
                         % _classify(xs, ys, n_pursuers, n_evaders, obs_range, flatten).why_wave)
    return _add(("pursuit_specializations.def", lines[1]), ("pursuit_live_specializations.def", lines[0]))


def pursuit_live_crowd_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id=True):
    """-> (live line, fixed line) that give a per-env-counts capacity above 64 pursuers or evaders the crowd kernel: XLC(..., NW) over an
    XC(..., NW) shape -- or None when the crowd kernel cannot take the capacity (pursuit_crowd_path says why) or when it has an X / XG
    fast path (pursuit_live_lines forms its lines).  Pure: nothing is written."""
    c = _classify(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id)
    return (c.line("XLC"), c.line("XC")) if c.kind == "XC" else None


def add_pursuit_live_crowd_shape(xs, ys, n_pursuers, n_evaders, obs_range, flatten):
    """per-env agent counts at this capacity on the crowd kernel: the XLC line in the local live list, and the XC line it stands on in the
    local crowd list if it is missing"""
    lines = pursuit_live_crowd_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten)
    if lines is None:
        c = _classify(xs, ys, n_pursuers, n_evaders, obs_range, flatten)
        if c.kind is not None:
            raise ValueError("this PursuitEvade capacity has a one-wavefront / multi-wavefront fast path: use --pursuit-live-shape")
        raise ValueError("no crowd kernel for this PursuitEvade capacity: %s (per-env agent counts run on the generic kernel)" % c.why_crowd)
    return _add(("pursuit_crowd_specializations.def", lines[1]), ("pursuit_live_specializations.def", lines[0]))


def pursuit_to_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id=True):
    """-> (two-buffer line, fixed line) that give step_to() of a shape its fast kernel: X(...) over an X(...) shape, XC(..., NW) over an
    XC(..., NW) shape -- or (None, why not): the lines of a multi-wavefront (XG) shape are formed by pursuit_to_group_lines, and a shape
    without an X / XC fast path has nothing to stand on.  Pure: nothing is written."""
    c = _classify(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id)
    if c.kind == "XG":
        return None, ("its fast path is the multi-wavefront kernel (XG, %d wavefronts), whose two-buffer line --pursuit-to-group-shape adds: "
                      "use that option" % c.nw)
    if c.kind is None:
        return None, "the shape has no X / XC fast path (one wavefront: %s; crowd kernel: %s)" % (c.why_wave, c.why_crowd)
    return c.line(c.kind), c.line(c.kind)


def add_pursuit_to_shape(xs, ys, n_pursuers, n_evaders, obs_range, flatten):
    """step_to() of this shape on the two-buffer instantiation of its fast kernel: the line in the local two-buffer list, and the X / XC
    line it stands on in the local fixed list if it is missing"""
    line, fixed = pursuit_to_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten)
    if line is None:
        raise ValueError("no two-buffer fast kernel for this PursuitEvade shape: %s (step_to runs on the generic kernel)" % fixed)
    return _add(("pursuit_specializations.def" if fixed.startswith("X(") else "pursuit_crowd_specializations.def", fixed),
                ("pursuit_to_specializations.def", line))


def _group_lines(shape, include_id, macro, x_why, xc_why):
    """-> (line under `macro`, XG line) of a multi-wavefront shape, or (None, why not): an X shape x_why, an XC shape xc_why after the
    refusal of pursuit_fast_path, any other shape that refusal alone"""
    c = _classify(*shape, include_id=include_id)
    if c.kind == "XG":
        return c.line(macro), c.line("XG")
    return None, x_why if c.kind == "X" else "no multi-wavefront fast path (%s); %s" % (c.why_wave, xc_why) if c.kind == "XC" else c.why_wave


def pursuit_to_group_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id=True, live=False):
    """-> (two-buffer line, fixed line) that give step_to() of a multi-wavefront shape its fast kernel: XG(..., NW) -- live: XLG(..., NW),
    the handles with per-env agent counts -- over an XG(..., NW) shape, or (None, why not): a one-wavefront or crowd shape has its lines
    from pursuit_to_lines, and a shape without a fast path has nothing to stand on.  Pure: nothing is written."""
    return _group_lines((xs, ys, n_pursuers, n_evaders, obs_range, flatten), include_id, "XLG" if live else "XG",
                        "its fast path is the one-wavefront kernel (X): use --pursuit-to-shape",
                        "the crowd kernel takes this shape: use --pursuit-to-shape")


def add_pursuit_to_group_shape(xs, ys, n_pursuers, n_evaders, obs_range, flatten, live=0):
    """step_to() of this multi-wavefront shape on the two-buffer instantiation of the group kernel: the XG (live: XLG) line in the local
    two-buffer list, the XG line it stands on in the local fixed list if it is missing, and with `live` the XLG line of the live list"""
    line, fixed = pursuit_to_group_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten, live=bool(live))
    if line is None:
        raise ValueError("no two-buffer multi-wavefront kernel for this PursuitEvade shape: %s (step_to runs on the generic kernel)" % fixed)
    return _add(("pursuit_specializations.def", fixed), *([("pursuit_live_specializations.def", line)] if live else []),
                ("pursuit_to_specializations.def", line))


def pursuit_to_group_f16_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten, include_id=True, live=False):
    """-> (half line, fixed line) that give the half-precision step_to() (obs_dtype=torch.float16) of a multi-wavefront shape its fast
    kernel: HG(..., NW) -- live: HLG(..., NW), the handles with per-env agent counts -- over an XG(..., NW) shape, or (None, why not): the
    half kernels of a one-wavefront shape come with its --pursuit-to-shape line, the crowd kernel has no half form, and a shape without a
    fast path has nothing to stand on.  Pure: nothing is written."""
    return _group_lines((xs, ys, n_pursuers, n_evaders, obs_range, flatten), include_id, "HLG" if live else "HG",
                        "its fast path is the one-wavefront kernel (X), whose half kernel comes with its two-buffer line: use --pursuit-to-shape",
                        "the crowd kernel takes this shape, and it has no half form")


def add_pursuit_to_group_f16_shape(xs, ys, n_pursuers, n_evaders, obs_range, flatten, live=0):
    """the half-precision step_to() of this multi-wavefront shape on the binary16 instantiation of the group kernel: the HG (live: HLG)
    line in the local half list, the XG line it stands on in the local fixed list if it is missing, and with `live` the XLG line of the
    live list"""
    line, fixed = pursuit_to_group_f16_lines(xs, ys, n_pursuers, n_evaders, obs_range, flatten, live=bool(live))
    if line is None:
        raise ValueError("no half-precision multi-wavefront kernel for this PursuitEvade shape: %s (the half step_to runs on the generic kernel)" % fixed)
    return _add(("pursuit_specializations.def", fixed), *([("pursuit_live_specializations.def", "XLG" + fixed[2:])] if live else []),
                ("pursuit_to_f16_group_specializations.def", line))


def waterworld_wave_lds_bytes(n_pursuers, n_evaders, n_poison, n_sensors, obs_dim):
    """the static LDS of a specialised one-wavefront Waterworld kernel (SPEC_BYTES, waterworld_wave_body.inc: wave_lds_bytes(4 * NP + 4, ...) of
    particle_wave.hpp): the record | the staged rows [n_pursuers + 1][obs_dim] | the sensor vectors, each a whole number of 16 bytes, then the
    reach masks, the collision bytes and the flags; the generic kernel's dynamic LDS (ww_lds_bytes) is the same number"""
    P, E, PO, K, D = int(n_pursuers), int(n_evaders), int(n_poison), int(n_sensors), int(obs_dim)
    up4 = lambda v: (v + 3) // 4 * 4
    return ((up4(4 * (P + E + PO) + 4) + up4((P + 1) * D) + up4(2 * K)) * 4 + 8 * P + P * (E + PO) + 2 * E + PO + 15) // 16 * 16


def waterworld_shape_refusal(n_pursuers, n_evaders, n_poison, n_sensors, obs_dim):
    """why a line X(n_pursuers, n_evaders, n_poison, n_sensors, obs_dim) cannot be built or would never run, or None: what ww_validate
    (waterworld.hip), ww_obs_dim_of, particle_create (common.hpp) and the static_asserts of waterworld_wave_body.inc say, evaluated here so
    that such a shape is refused before it breaks the build"""
    P, E, PO, K, D = int(n_pursuers), int(n_evaders), int(n_poison), int(n_sensors), int(obs_dim)
    if min(P, E, PO) < 1 or P + E + PO > 62 or 2 * P > 64 or not 1 <= K <= 256:
        return "no Waterworld kernel for this shape at all (madrl_waterworld_create refuses it)"
    widths = [K * nfeat + 2 + addid for nfeat in (4, 7) for addid in (0, 1)]
    if D not in widths:
        return ("OBS_DIM %d is no row width of %d sensors: %d / %d without speed features (without / with the agent id), %d / %d with them; "
                "no configuration would ever take the line" % ((D, K) + tuple(widths)))
    lds = waterworld_wave_lds_bytes(P, E, PO, K, D)
    if lds > 64 * 1024:
        return ("the shape needs %d bytes of LDS per workgroup, a Waterworld handle may use 65 536 (madrl_waterworld_create refuses it): "
                "fewer sensors or fewer pursuers" % lds)
    return None


def add_waterworld_shape(n_pursuers, n_evaders, n_poison, n_sensors, obs_dim=None):
    if obs_dim is None:
        obs_dim = n_sensors * 7 + 2 + 1          # speed features and the agent id (the reference's defaults)
    why = waterworld_shape_refusal(n_pursuers, n_evaders, n_poison, n_sensors, obs_dim)
    if why is not None:   # before anything is written: a line that cannot compile would break every later build
        raise ValueError("no specialised Waterworld kernel for this shape: " + why)
    return _append_local("waterworld_specializations.def", "X(%d, %d, %d, %d, %d)   // added by madrl_amd.build" % (n_pursuers, n_evaders, n_poison, n_sensors, obs_dim))


def waterworld_line_of(n_pursuers, n_evaders, n_poison=10, n_sensors=30, speed_features=True, addid=True):
    """the dispatch key of ww_launch (waterworld.hip) restated: (Np, Ne, Npo, K, ww_obs_dim_of) of a configuration, compared with every
    line of the lists -> the lines that match it (the host takes the last one; a list without duplicates has at most one)"""
    key = (int(n_pursuers), int(n_evaders), int(n_poison), int(n_sensors),
           int(n_sensors) * (7 if speed_features else 4) + 2 + (1 if addid else 0))
    return [line for line in waterworld_lines() if line == key]


def waterworld_lines():
    """the X(...) argument tuples of csrc/waterworld_specializations.def and of its .local.def companion, in file order, duplicates kept"""
    out = []
    for path in (os.path.join(CSRC, "waterworld_specializations.def"), os.path.join(CSRC, "waterworld_specializations.local.def")):
        if os.path.exists(path):
            out += [tuple(int(v) for v in m.group(1).split(",")) for m in re.finditer(r"^\s*X\(([^)]*)\)", open(path).read(), re.M)]
    return out


def specialised_shapes(def_name):
    """the X(...) / XG(...) argument tuples of a csrc/*_specializations.def list and of its git-ignored .local.def companion"""
    out = set()
    for path in (os.path.join(CSRC, def_name), os.path.join(CSRC, def_name.replace(".def", ".local.def"))):
        if os.path.exists(path):
            for m in re.finditer(r"^\s*XG?\(([^)]*)\)", open(path).read(), re.M):
                out.add(tuple(int(v) for v in m.group(1).split(",")))
    return out


def waterworld_is_specialised(n_pursuers, n_evaders, n_poison, n_sensors, obs_dim):
    return (int(n_pursuers), int(n_evaders), int(n_poison), int(n_sensors), int(obs_dim)) in specialised_shapes("waterworld_specializations.def")


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


_INC = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _deps(src, seen=None):
    """the files one source depends on: itself and, recursively, every `#include "..."` in it that exists (the git-ignored *.local.def
    lists are behind __has_include: they count once they exist) -- so appending a Pursuit shape re-compiles pursuit.hip and nothing else"""
    seen = set() if seen is None else seen
    if src in seen or not os.path.exists(src):
        return seen
    seen.add(src)
    for inc in _INC.findall(open(src).read()):
        _deps(os.path.normpath(os.path.join(os.path.dirname(src), inc)), seen)
    return seen


def _compile(src, obj, verbose):
    cmd = [HIPCC] + FLAGS + [f for pat, fl in EXTRA_FLAGS.items() if os.path.basename(src).startswith(pat) for f in fl] + ["-c", src, "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def build(force=False, verbose=False):
    objs, stale = [], []
    for src in sources():
        obj = src[:-4] + ".o"
        objs.append(obj)
        if force or not os.path.exists(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in _deps(src)):
            stale.append((src, obj))
    if stale:   # the objects are independent: compile them side by side (the three MultiWalker classes take a minute each)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(len(stale), os.cpu_count() or 1)) as ex:
            for f in [ex.submit(_compile, src, obj, verbose) for src, obj in stale]:
                f.result()
    for f in os.listdir(CSRC):   # objects whose source is gone (a renamed file) must not be linked
        if f.endswith(".o") and os.path.join(CSRC, f) not in objs:
            os.remove(os.path.join(CSRC, f))
    if force or not os.path.exists(SO) or any(os.path.getmtime(o) > os.path.getmtime(SO) for o in objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    argv = sys.argv[1:]
    for flag, fn, lo, hi in (("--pursuit-shape", add_pursuit_shape, 6, 6), ("--pursuit-live-shape", add_pursuit_live_shape, 6, 6),
                             ("--pursuit-crowd-shape", add_pursuit_crowd_shape, 6, 6),
                             ("--pursuit-live-crowd-shape", add_pursuit_live_crowd_shape, 6, 6),
                             ("--pursuit-to-shape", add_pursuit_to_shape, 6, 6),
                             ("--pursuit-to-group-shape", add_pursuit_to_group_shape, 6, 7),
                             ("--pursuit-to-group-f16-shape", add_pursuit_to_group_f16_shape, 6, 7),
                             ("--waterworld-shape", add_waterworld_shape, 4, 5)):
        while flag in argv:
            i = argv.index(flag)
            vals = []
            while i + 1 + len(vals) < len(argv) and len(vals) < hi and argv[i + 1 + len(vals)].lstrip("-").isdigit():
                vals.append(int(argv[i + 1 + len(vals)]))
            if len(vals) < lo:
                raise SystemExit("%s takes %d%s integers" % (flag, lo, "" if lo == hi else " or %d" % hi))
            print("%s %s: %s" % (flag, vals, "added" if fn(*vals) else "already specialised"))
            del argv[i:i + 1 + len(vals)]
    print(build(force="--force" in argv, verbose=True))
