"""Every committed line of every Pursuit specialisation list is reachable, and nothing else is (madrl_amd/csrc/pursuit.hip, DESIGN.md §4.3
"Host dispatch").

For each X / XG / XC line: handles of two envs with the configuration's counts and with per-env agent counts, each with float32 and with
float16 observations, and -- where n_evaders >= n_pursuers -- one evader-control handle.  What each handle must run on is formed here from
list membership alone (isa.def_lines over the six lists and their .local.def companions), never asked of the library first:
  * kernel_kind is "wave" exactly when the line (per-env counts: and its XL / XLG / XLC line) is listed; in evader control, for an X line;
  * step_to_kernel_kind is "wave" exactly when the handle's two-buffer line is listed too: X / XG / XC, with per-env counts XL / XLG /
    XLC, of pursuit_to_specializations.def -- for float16 observations the X / XL lines of that list and the HG / HLG lines of
    pursuit_to_f16_group_specializations.def, never a crowd line -- and never in evader control;
  * last_step_entry after every step: "fixed" exactly for an in-place float32 step with the configuration's counts on a line with an XF
    line (the handles here meet the fixed-constants contract), "wave" for every other fast step, "generic" otherwise.
Every handle does one reset and two steps (max_steps 2 with auto-reset: the second step ends the episodes), the float32 handles one more
step_to into a second buffer, each compared bit for bit with a kernel="generic" twin of the same seed and actions.  Two envs is the
smallest batch at which a wrong launcher, a wrong geometry or a wrong mask-plane length shows; the largest handle, 128 x 128 with 100 v 300
and obs_range 21, has 1.4 MB of float32 rows."""
import os

import pytest

import isa

DEV = "cuda:0"
N_ENVS = 2


def _list(name, kinds):
    """{kind: [lines]} of a list and of its .local.def companion, as pursuit.hip includes them"""
    out = isa.def_lines(name, kinds)
    local = name.replace(".def", ".local.def")
    if os.path.exists(os.path.join(isa.CSRC, local)):
        for k, v in isa.def_lines(local, kinds).items():
            out[k] += v
    return out


BASE = dict(_list("pursuit_specializations.def", ("X", "XG")), **_list("pursuit_crowd_specializations.def", ("XC",)))
LIVE = _list("pursuit_live_specializations.def", ("XL", "XLG", "XLC"))
FIXED = _list("pursuit_fixed_specializations.def", ("XF",))["XF"]
TO = _list("pursuit_to_specializations.def", ("X", "XL", "XG", "XLG", "XC", "XLC"))
HALF = _list("pursuit_to_f16_group_specializations.def", ("HG", "HLG"))
LINES = [(kind, line) for kind in ("X", "XG", "XC") for line in BASE[kind]]


def test_the_lists_leave_out_what_the_cases_below_count_on():
    keys = [line[:6] for _, line in LINES]
    assert len(set(keys)) == len(keys)   # one line per shape: which line a configuration finds does not depend on the order
    assert (32, 32, 16, 60, 7, 1, 2) in BASE["XG"] and (32, 32, 16, 60, 7, 1, 2) in TO["XG"]   # in place and float32 two-buffer only:
    assert (32, 32, 16, 60, 7, 1, 2) not in LIVE["XLG"] + HALF["HG"] + HALF["HLG"]              # no live line, no half line
    assert (16, 16, 20, 50, 5, 1, 2) in TO["XLG"] and (16, 16, 20, 50, 5, 1, 2) not in TO["XG"]   # two buffers with per-env counts only
    assert (24, 24, 70, 90, 9, 1, 2) in BASE["XC"] and (24, 24, 70, 90, 9, 1, 2) not in LIVE["XLC"]
    assert not {line[:6] for line in HALF["HG"] + HALF["HLG"]} & {line[:6] for line in BASE["XC"]}   # no half form of a crowd line
    assert len(FIXED) >= 5 and all(line in BASE["X"] for line in FIXED)


def _expected(kind, line, live, half, evader_control):
    """(kernel_kind, step_to_kernel_kind, last_step_entry of a step(), ... of a float32 step_to) from the lists"""
    live_kind = "XL" + kind[1:]
    in_place = kind == "X" if evader_control else (not live or line in LIVE[live_kind])
    if not half:
        listed = line in TO[live_kind if live else kind]
    else:
        listed = line in {"X": TO["XL" if live else "X"], "XG": HALF["HLG" if live else "HG"], "XC": []}[kind]
    two_buffer = in_place and listed and not evader_control
    wave = lambda fast: "wave" if fast else "generic"
    if half:    # a step() of a float16 handle goes from one internal buffer to the other: a two-buffer launch
        step = wave(two_buffer)
    else:
        step = "fixed" if in_place and not live and not evader_control and line in FIXED else wave(in_place)
    return wave(in_place), wave(two_buffer), step, wave(two_buffer)


def _walk(kind, line, live, half, evader_control):
    import numpy as np
    import torch
    from madrl_amd.pursuit import BatchedPursuitEvade
    xs, ys, P, E, R, fl = line[:6]
    what = "%s%s %s%s%s" % (kind, line, "per-env counts" if live else "fixed counts", ", float16" if half else "", ", evader control" if evader_control else "")
    kw = dict(n_pursuers=P, n_evaders=E, obs_range=R, n_catch=2, surround=True, flatten=bool(fl), reward_mech="local")
    if evader_control:
        kw["train_pursuit"] = False
    mk = lambda kernel: BatchedPursuitEvade([np.zeros((xs, ys), np.int32)], n_envs=N_ENVS, device=DEV, seed=11, max_steps=2, auto_reset=True,
                                            kernel=kernel, per_env_counts=live, obs_dtype=torch.float16 if half else torch.float32, **kw)
    a, g = mk("auto"), mk("generic")
    want_kind, want_to, want_step, want_step_to = _expected(kind, line, live, half, evader_control)
    print(what, "->", a.kernel_kind, a.step_to_kernel_kind)
    assert (a.kernel_kind, a.step_to_kernel_kind) == (want_kind, want_to), what
    assert (g.kernel_kind, g.step_to_kernel_kind) == ("generic", "generic"), what
    if live:   # the second env below its capacity
        for env in (a, g):
            env.set_agent_counts(n_pursuers=torch.tensor([P, max(P - 1, 1)]), n_evaders=torch.tensor([E, max(E - 1, 1)]))
    bits = lambda t: t.view(torch.int16 if t.dtype is torch.float16 else torch.int32)
    assert torch.equal(bits(a.reset()), bits(g.reset())), what + ": reset"
    gen = torch.Generator(device="cpu").manual_seed(5)
    second = [torch.empty((N_ENVS, P, a.obs_dim), dtype=torch.float32, device=DEV) for _ in (a, g)]
    for t in range(2 if half else 3):
        act = torch.randint(0, 5, (N_ENVS, P), generator=gen, dtype=torch.int32).to(DEV)
        if t < 2:
            (oa, ra, da, ia), (og, rg, dg, ig) = a.step(act), g.step(act)
        else:
            (oa, ra, da, ia), (og, rg, dg, ig) = a.step_to(act, second[0]), g.step_to(act, second[1])
        at = "%s: step %d" % (what, t)
        assert (a.last_step_entry, g.last_step_entry) == (want_step if t < 2 else want_step_to, "generic"), at
        assert torch.equal(bits(oa), bits(og)), at + ": observations"
        assert torch.equal(bits(ra), bits(rg)), at + ": rewards"
        assert torch.equal(ia["done_bits"], ig["done_bits"]) and torch.equal(da, dg), at + ": done"
        assert torch.equal(ia["removed"], ig["removed"]), at + ": removed"


@pytest.mark.gpu
@pytest.mark.parametrize("kind,line", LINES, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_every_listed_kernel_of_the_line_is_reachable_and_nothing_else(kind, line, monkeypatch):
    monkeypatch.delenv("MADRL_PURSUIT_FIXED", raising=False)   # (read when a handle is created)
    for live in (False, True):
        for half in (False, True):
            _walk(kind, line, live, half, False)
    if line[3] >= line[2]:
        _walk(kind, line, False, False, True)
