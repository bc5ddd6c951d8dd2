"""Which kernel a PursuitEvade configuration runs on, and what the caller's state buffer holds for it (madrl_amd/csrc/pursuit.hip, host side;
DESIGN.md §4.3 "Host dispatch").

CPU (-m "not gpu"): for every committed X / XG / XC line, madrl_pursuit_state_bytes / _flags_offset give records, padded to 256 bytes, then
the mask plane of the line's kernel family, then one flag dword per env -- the mask plane's size written out here from DESIGN.md's rules,
not read from the library -- and the rules that take a configuration off its line (no id in a flatten row, evader control, no line).
GPU (-m gpu): test_dispatch_matrix, one capacity per family, with and without per-env agent counts."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madrl_amd", "csrc")
N = 1000   # records of 112 bytes and the like: the padding to 256 bytes shows


def _lines(name, kind):
    text = open(os.path.join(CSRC, name)).read()
    return [tuple(int(v) for v in m.group(1).split(",")) for m in re.finditer(r"^\s*%s\(([^)]*)\)" % kind, text, re.M)]


X_LINES = _lines("pursuit_specializations.def", "X")
XG_LINES = _lines("pursuit_specializations.def", "XG")
XC_LINES = _lines("pursuit_crowd_specializations.def", "XC")


def _mask_bytes(kind, line):
    """bytes per env of what the line's kernel remembers about the observation buffer"""
    if kind == "X":    # one dword per lane of the env's wavefront
        return 256
    if kind == "XC":   # one word per env: "channel 3 is not known to hold +0.0"
        return 4
    xs, ys, P, E, R, fl, nw = line
    D = 3 * R * R + 1 if fl else 4 * R * R
    ns = -(-(P * (D // 4)) // (64 * nw))          # float4 slots per thread
    mwords = -(-ns // 8) if ns > 8 else 1        # one bit per slot in each byte of a mask dword
    return 256 * nw * mwords


def _cfg(line, **over):
    from madrl_amd import _lib
    c = _lib.PursuitConfig()
    c.struct_size = C.sizeof(_lib.PursuitConfig)
    c.xs, c.ys, c.n_pursuers, c.n_evaders, c.obs_range, c.flatten = line[:6]
    c.n_catch, c.surround, c.include_id, c.n_maps = 2, 1, 1, 1
    c.layer_norm, c.constraint_window = 10.0, 1.0
    for k, v in over.items():
        setattr(c, k, v)
    return c


def _check(cfg, mask, what):
    from madrl_amd import _lib
    L = _lib.lib()
    rec, total, flags = C.c_int32(), C.c_uint64(), C.c_uint64()
    assert L.madrl_pursuit_record_bytes(C.byref(cfg), C.byref(rec)) == 0, what
    assert L.madrl_pursuit_state_bytes(C.byref(cfg), N, C.byref(total)) == 0, what
    assert L.madrl_pursuit_flags_offset(C.byref(cfg), N, C.byref(flags)) == 0, what
    want = (rec.value * N + 255) // 256 * 256 + mask * N
    assert flags.value == want, (what, flags.value, want)
    assert total.value == want + 4 * N, (what, total.value, want + 4 * N)


def test_the_committed_lists_are_the_ones_this_file_knows():
    assert len(X_LINES) >= 13 and len(XG_LINES) >= 4 and len(XC_LINES) >= 5
    assert {(l[:6], _mask_bytes("XG", l)) for l in XG_LINES} >= {
        ((32, 32, 16, 60, 7, 1), 512), ((16, 16, 20, 50, 5, 1), 512), ((32, 32, 30, 50, 11, 1), 2048), ((32, 32, 30, 30, 11, 1), 2048)}
    keys = [l[:6] for l in X_LINES + XG_LINES + XC_LINES]
    assert len(set(keys)) == len(keys)   # one line per shape: the order of the lists decides nothing in the committed tree


@pytest.mark.parametrize("kind,line", [(k, l) for k, ls in (("X", X_LINES), ("XG", XG_LINES), ("XC", XC_LINES)) for l in ls],
                         ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_state_buffer_of_every_committed_line(kind, line):
    _check(_cfg(line), _mask_bytes(kind, line), (kind, line))
    if line[5]:   # a flatten row without the id is not a whole number of float4: generic kernel, no mask plane
        _check(_cfg(line, include_id=0), 0, (kind, line, "include_id=0"))
    if line[3] >= line[2]:   # evader control (n_evaders >= n_pursuers): the one-wavefront kernel has it, the group and crowd kernels do not
        _check(_cfg(line, control_evaders=1), 256 if kind == "X" else 0, (kind, line, "control_evaders=1"))


def test_rule_cases():
    x, xg, xc = (16, 16, 8, 30, 7, 1), (16, 16, 20, 50, 5, 1, 2), (24, 24, 20, 300, 9, 1, 1)
    assert x in X_LINES and xg in XG_LINES and xc in XC_LINES
    for line in (x, xg, xc):
        _check(_cfg(line, include_id=0), 0, (line, "include_id=0"))
    _check(_cfg(xg, control_evaders=1), 0, "XG, control_evaders=1")
    _check(_cfg(xc, control_evaders=1), 0, "XC, control_evaders=1")
    _check(_cfg(x, control_evaders=1), 256, "X, control_evaders=1")
    unlisted = (16, 16, 7, 30, 7, 1)
    assert unlisted not in [l[:6] for l in X_LINES + XG_LINES + XC_LINES]
    _check(_cfg(unlisted), 0, "unlisted shape")


# ------------------------------------------------------------------ GPU
DEV = "cuda:0"
# capacity, has a live-count line (XL / XLG / XLC)
MATRIX = [((10, 10, 2, 2, 3, 1), True),       # X + XL
          ((16, 16, 20, 50, 5, 1), True),     # XG + XLG
          ((24, 24, 20, 300, 9, 1), True),    # XC + XLC
          ((24, 24, 70, 90, 9, 1), False)]    # XC only


@pytest.mark.gpu
@pytest.mark.parametrize("per_env_counts", [False, True], ids=["fixed", "per_env_counts"])
@pytest.mark.parametrize("cap,has_live", MATRIX, ids=["X", "XG", "XC", "XC_only"])
def test_dispatch_matrix(cap, has_live, per_env_counts):
    import numpy as np
    import torch
    from madrl_amd import _lib
    from madrl_amd.pursuit import BatchedPursuitEvade
    xs, ys, P, E, R, fl = cap
    assert (cap in X_LINES) + (cap in [l[:6] for l in XG_LINES]) + (cap in [l[:6] for l in XC_LINES]) == 1
    live = _lines("pursuit_live_specializations.def", "XL") + [l[:6] for k in ("XLG", "XLC") for l in _lines("pursuit_live_specializations.def", k)]
    assert (cap in live) == has_live
    fast = has_live or not per_env_counts   # what `auto` runs
    n_envs = 3
    kw = dict(n_pursuers=P, n_evaders=E, obs_range=R, n_catch=2, surround=True, flatten=bool(fl), reward_mech="local")
    mk = lambda kernel: BatchedPursuitEvade([np.zeros((xs, ys), np.int32)], n_envs=n_envs, device=DEV, seed=9, max_steps=3, auto_reset=True,
                                            kernel=kernel, per_env_counts=per_env_counts, **kw)
    a, g = mk("auto"), mk("generic")
    L = _lib.lib()

    # ---- kernel kind under each setting
    assert a.kernel_kind == ("wave" if fast else "generic") and g.kernel_kind == "generic"
    a.set_kernel("generic")
    assert a.kernel_kind == "generic"
    if fast:
        a.set_kernel("wave")
        assert a.kernel_kind == "wave"
    else:
        with pytest.raises(_lib.MadrlError, match="no live-count specialisation was compiled for this capacity"):
            a.set_kernel("wave")
        assert a.kernel_kind == "generic"
        a.set_kernel("auto")
        assert a.kernel_kind == "generic"

    # ---- order of the two calls: counts asked for after kernel WAVE was
    pend = torch.tensor([P, E], dtype=torch.int32, device=DEV).repeat(n_envs, 1).contiguous()
    rc = L.madrl_pursuit_set_agent_counts(a._handle, _lib.ptr(a._pending if per_env_counts else pend))
    if not has_live and not per_env_counts:   # WAVE stands (the fixed XC kernel), and no live kernel could honour it
        assert rc != 0 and "kernel WAVE was requested and no live-count specialisation was compiled" in L.madrl_last_error().decode()
    else:
        assert rc == 0, L.madrl_last_error()
        if not per_env_counts:
            assert a.kernel_kind == "wave"   # the live instantiation of the line
            assert L.madrl_pursuit_set_agent_counts(a._handle, None) == 0
    assert a.kernel_kind == ("wave" if fast else "generic")

    # ---- one reset and two steps on the fast kernel and on the generic one, then two steps with both on the generic kernel, then the fast
    # kernel again: what it knew about the observation buffer is void after the generic launches
    if per_env_counts:
        for env in (a, g):
            env.set_agent_counts(n_pursuers=torch.tensor([P, max(P - 1, 1), 1]), n_evaders=torch.tensor([E, E - 1, 1]))
    assert torch.equal(a.reset(), g.reset())
    gen = torch.Generator(device="cpu").manual_seed(4)
    t = 0
    for kernel, steps in ((None, 2), ("generic", 2), ("wave" if fast else "auto", 2)):
        if kernel:
            a.set_kernel(kernel)
        assert a.kernel_kind == ("generic" if kernel == "generic" or not fast else "wave")
        for _ in range(steps):
            act = torch.randint(0, 5, (n_envs, P), generator=gen, dtype=torch.int32).to(DEV)
            oa, ra, da, ia = a.step(act)
            og, rg, dg, ig = g.step(act)
            what = "step %d (%s)" % (t, a.kernel_kind)
            assert torch.equal(oa, og), what + ": observations"
            assert torch.equal(ra.view(torch.int32), rg.view(torch.int32)), what + ": rewards"
            assert torch.equal(ia["done_bits"], ig["done_bits"]) and torch.equal(da, dg), what + ": done"
            assert torch.equal(ia["removed"], ig["removed"]), what + ": removed"
            t += 1
    sa, sg = a.get_state(), g.get_state()
    for k in ("pos_p", "pos_e", "gone", "term_p", "term_e", "map_id", "tick", "t"):
        assert torch.equal(sa[k], sg[k]), "state[%s]" % k
