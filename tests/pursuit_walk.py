"""Walks of a Pursuit handle through every ordered pair of API calls, against the C oracle (tests/test_pursuit_walk_cpu.py,
tests/test_pursuit_walk_gpu.py).

What a Pursuit fast path computes depends on state nobody sees: the stale-zero masks and the buffer / element format they describe, the
kernel entry chosen launch by launch, the parity of the alternating walk, pending per-env counts, and -- in BatchedPursuitEvade -- the
tensor version counter, the private float32 copy of a half reset and obs_buffer following step_to.  Each feature's own test file drives it
through a scripted sequence; here every op kind is followed once by every op kind (an Eulerian circuit of the complete directed graph over
the kinds), and after every op every observation buffer the test owns is compared bit for bit with `Model`, which knows nothing of masks:
it loads the source buffer into the oracle's persistent local_obs, steps, applies the fused auto-reset and writes the destination.

Buffers start full of SENTINELS -- negative integers, exact in binary16, a set of their own per slot, neighbours different -- so a cell a
launch must keep shows what it held and a store that should not have happened shows as a 0.0 (or a count) over a sentinel.

An op is a dict(kind=, prims=[...]); a prim is a tuple both `Model.apply` and the device replayers (`AbiDevice`, `PyDevice`) understand:
  ("conv", src, sfmt, dst)                 caller-side conversion of a whole buffer into a slot of the other format
  ("write", slot, fmt, rows, salt)         the caller fills rows with fresh sentinels
  ("inval",)                               madrl_pursuit_invalidate_obs
  ("step", how, src, dst, fmt, act, inj, inj_ok)   how: "inplace" | "to" | "f16"; fmt: the format BOTH buffers are read in
  ("reset", slot, fmt, mask)               fmt "h": on a widened copy, rounded back (BatchedPursuitEvade's half reset)
  ("zero", slot)                           zero a float32 slot and declare it
  ("set_t", t) ("set_pos", n, m) ("get_state",) ("kernel", generic) ("walk", mode) ("launch", max_blocks) ("params", catchr)
  ("cur", cw, catchr) ("inject", on) ("pending", envs, counts)
  ("edit", slot, fmt, rows, salt, seen)    PyDevice: an edit of the current tensor the version counter sees / does not see
"""
import ctypes as C

import numpy as np

N, H, BASE = 7, 5, 4100
AGES = (np.arange(N) * 3) % H            # episode clocks after the first reset: staggered
GUARD, GUARD_BYTE = 4096, 0xA5
BAD_ACTIONS = (-1, 5, 7, 2 ** 31 - 1, -2 ** 31)   # "anything else is treated as 4" (include/madrl_hip.h, actions_dev)
ENTRY_NONE, ENTRY_GENERIC, ENTRY_WAVE, ENTRY_FIXED = 0, 1, 2, 3   # MADRL_STEP_ENTRY_*
KERNEL_GENERIC, KERNEL_WAVE = 1, 2

_X = dict(n_catch=2, surround=True, reward_mech="local")
# name -> the two seeds of its walks (chosen so that the conditions of tests/test_pursuit_walk_cpu.py hold), shape (xs, ys, P, E, R, flatten), env kwargs, and what the .def lists give the handle (written out here, not asked of the
# library): fixed = a line in pursuit_fixed_specializations.def and a configuration inside its contract; to / f16 = a two-buffer / half
# two-buffer fast kernel (pursuit_to_specializations.def without control_evaders; X / XL lines and the HG / HLG lines)
HANDLES = {
    "XF_c1": dict(seeds=(3, 4), shape=(16, 16, 8, 30, 7, 1), kw=dict(_X), fixed=True, to=True, f16=True),
    "X_window_wider_than_map": dict(seeds=(1, 2), shape=(6, 6, 3, 5, 11, 0), kw={}, fixed=False, to=True, f16=True),
    "X_evader_control": dict(seeds=(1, 4), shape=(16, 16, 8, 12, 7, 1), kw=dict(train_pursuit=False, surround=False, n_catch=1, reward_mech="local"),
                             fixed=False, to=False, f16=False),
    "XG_13_slots": dict(seeds=(1, 3), shape=(10, 10, 36, 12, 11, 1), kw={}, fixed=False, to=True, f16=True),
    "XC_20v300": dict(seeds=(1, 3), shape=(24, 24, 20, 300, 9, 1), kw=dict(_X), fixed=False, to=True, f16=False),
    "XL_c1_live": dict(seeds=(2, 3), shape=(16, 16, 8, 30, 7, 1), kw=dict(_X), live=True, fixed=False, to=True, f16=True),
    "XLG_live": dict(seeds=(2, 3), shape=(16, 16, 20, 50, 5, 1), kw=dict(_X), live=True, fixed=False, to=True, f16=True),
}

ABI_KINDS = ("step", "step_foreign", "step_to", "step_to_f16", "reinterpret", "reset_all", "reset_mask", "invalidate", "write_current",
             "write_other", "declare_zero", "set_t", "set_pos", "get_state", "kernel_generic", "kernel_auto", "set_walk", "set_launch",
             "set_params", "curriculum", "inject")
PY_KINDS = ("step", "step_to", "step_into", "reset_all", "reset_mask", "edit_seen", "edit_data", "set_t", "set_pos", "get_state",
            "kernel_generic", "kernel_auto", "set_walk", "set_launch", "curriculum", "inject")
PY_SEEDS = (1, 3)   # of the walks through BatchedPursuitEvade itself (XF_c1, either observation dtype)
ABI_SLOTS = (("f0", "f"), ("f1", "f"), ("f2", "f"), ("h0", "h"), ("h1", "h"), ("h2", "h"))


def kinds_of(name):
    return ABI_KINDS + (("pending",) if HANDLES[name].get("live") else ())


def py_slots(half):
    return (("own_a", "h"), ("own_b", "h"), ("r0", "h"), ("r1", "h"), ("r2", "h")) if half else (("own", "f"), ("r0", "f"), ("r1", "f"), ("r2", "f"))


def maps_of(spec):
    from madrl_amd.maps import rectangle_map
    xs, ys = spec["shape"][:2]
    return [rectangle_map(xs, ys)] if min(xs, ys) >= 16 else [np.zeros((xs, ys), np.int32)]


def env_kwargs(spec):
    xs, ys, P, E, R, fl = spec["shape"]
    return dict(spec["kw"], n_pursuers=P, n_evaders=E, obs_range=R, flatten=bool(fl))


def half_bits(x):
    """the header's rule for a stored half: round-to-nearest-even binary16 of the float32 value, as uint16"""
    with np.errstate(over="ignore"):   # (overflow to infinity is the rule, not an accident)
        return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def widen(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def sentinels(slot_index, idx, salt):
    """float32 values for the elements idx of slot number slot_index: -(16 + 100 slot + 0..96), integers below 2048 (exact in binary16)"""
    idx = np.asarray(idx, np.int64)
    return -(16.0 + 100.0 * slot_index + ((idx * 7 + salt * 13) % 97)).astype(np.float32)


def is_sentinel(x32):
    return x32 <= -16.0


# ------------------------------------------------------------------------------------------------------------------ the truth
class Model(object):
    """The truth, on the CPU: one one-env PursuitOracle per env (shape (p, e), env_id_base + n -- what the header promises env n equals;
    for a fixed-shape handle that is the batched oracle env by env), named buffers as raw bytes, episode clocks, and the control state
    the entry prediction needs."""

    def __init__(self, name, seed, slots=ABI_SLOTS, slot_bytes=None, spec=None, maps=None, max_steps=H, auto_reset=True):
        from oracle import pursuit as po
        self.po, self.name, self.spec, self.seed = po, name, spec or HANDLES[name], seed
        self.H, self.auto_reset = max_steps, auto_reset
        xs, ys, self.P, self.E, self.R, fl = self.spec["shape"]
        self.flat, self.is_live = bool(fl), bool(self.spec.get("live"))
        self.kw, self.maps = env_kwargs(self.spec), maps if maps is not None else maps_of(self.spec)
        self.train_pursuit = self.kw.get("train_pursuit", True)
        self.catchr, self.cw_env, self.cr_env = 0.01, None, None
        self.live = [(self.P, self.E)] * N
        self.pending = [(self.P, self.E)] * N
        self.orcs = [self._make(n, self.P, self.E) for n in range(N)]
        self.D = self.orcs[0].D
        self.n = N * self.P * self.D
        self.t = np.zeros(N, np.int64)
        self.slots = tuple(slots)
        self.fmt_of = dict(self.slots)
        self.index_of = {s: i for i, (s, _) in enumerate(self.slots)}
        full = (4 * self.n + 15) // 16 * 16
        self.nbytes = {s: (slot_bytes(s, f, self.n) if slot_bytes else full) for s, f in self.slots}
        self.buf = {}
        for s, f in self.slots:   # every slot starts full of its sentinels, a half slot over all of its bytes
            b = np.zeros(self.nbytes[s], np.uint8)
            if f == "f":
                k = self.nbytes[s] // 4
                b[:4 * k].view(np.float32)[:] = sentinels(self.index_of[s], np.arange(k), 0)
            else:
                k = self.nbytes[s] // 2
                b[:2 * k].view(np.uint16)[:] = half_bits(sentinels(self.index_of[s], np.arange(k), 0))
            self.buf[s] = b
        self.cur = None
        self.generic, self.inj, self.walk_mode, self.last_entry = False, False, 0, ENTRY_NONE
        self.rew = np.zeros((N, self.P), np.float32)
        self.done = np.zeros(N, np.uint8)
        self.removed = np.zeros(N, np.int32)
        # what the CPU test asks of a walk
        self.fused = np.zeros(N, np.int64)
        self.catches, self.overwritten, self.mid_episode_resets, self.entries = 0, 0, 0, []

    def _make(self, n, p, e):
        orc = self.po.PursuitOracle(self.maps, n_envs=1, seed=self.seed, env_id_base=BASE + n, **dict(self.kw, n_pursuers=p, n_evaders=e))
        self._curriculum_to(orc, n)
        return orc

    def _curriculum_to(self, orc, n):
        orc.set_params(self.catchr, 1.0)
        orc.set_curriculum(None if self.cw_env is None else self.cw_env[n:n + 1], None if self.cr_env is None else self.cr_env[n:n + 1])

    # -- buffers
    def view(self, slot, fmt):
        return self.buf[slot][:4 * self.n].view(np.float32) if fmt == "f" else self.buf[slot][:2 * self.n].view(np.uint16)

    def read32(self, slot, fmt):
        v = self.view(slot, fmt)
        x = v.copy() if fmt == "f" else widen(v)
        assert not np.isnan(x).any(), "a NaN in %s read as %s: raw carry-over and re-rounding would differ" % (slot, fmt)
        return x.reshape(N, self.P, self.D)

    def store32(self, slot, fmt, x):
        v = self.view(slot, fmt)
        before = v.copy()
        v[:] = x.reshape(-1) if fmt == "f" else half_bits(x.reshape(-1))
        was = is_sentinel(before if fmt == "f" else widen(before))
        self.overwritten += int((was & (v != before)).sum())

    def no_nan(self):
        for s, f in self.slots:
            self.read32(s, f)

    def sentinels_left(self, fmt):
        return sum(int(is_sentinel(self.read32(s, f)).sum()) for s, f in self.slots if f == fmt)

    # -- the oracle side of a launch
    def _load(self, n, rows):
        orc, p, R = self.orcs[n], self.live[n][0], self.R
        lo = orc.local_obs()
        a = rows[:p].astype(np.float64)
        if self.flat:   # channels 0 - 2 of every row; the id is not part of local_obs
            lo[0, :, :3] = a[:, :3 * R * R].reshape(p, 3, R, R)
        else:           # (R, R, 4) rows
            lo[0] = a.reshape(p, R, R, 4).transpose(0, 3, 1, 2)
        orc.set_local_obs(lo)
        orc.obs[0] = rows[:p]   # (what the oracle leaves alone in its output rows: absent observers)

    def _reset_env(self, n, rows, inj_pos=None, inj_map=None):
        if self.pending[n] != self.live[n]:   # per-env counts: a fresh oracle of the new shape takes the old one's tick
            old, (p, e) = self.orcs[n], self.pending[n]
            new = self._make(n, p, e)
            st = new.get_state()
            st["tick"][:] = old.get_state()["tick"]
            new.set_state(st)
            self.orcs[n], self.live[n] = new, (p, e)
        self._load(n, rows)
        self.orcs[n].reset(inj_pos=inj_pos, inj_map=inj_map)
        rows[:self.live[n][0]] = self.orcs[n].obs[0]
        self.t[n] = 0

    def predict(self, how, inj):
        """the header's rules (madrl_pursuit_last_step_entry, step_to, step_to_f16) for this launch"""
        if self.generic:
            return ENTRY_GENERIC
        if how == "inplace":
            fixed = self.spec["fixed"] and not inj and self.cw_env is None and self.walk_mode != 1 and not self.is_live
            return ENTRY_FIXED if fixed else ENTRY_WAVE
        return ENTRY_WAVE if self.spec["to" if how == "to" else "f16"] else ENTRY_GENERIC

    def kernel_kinds(self):
        """(kernel_kind, step_to_kernel_kind, step_to_f16_kernel_kind)"""
        w = lambda ok: KERNEL_WAVE if ok and not self.generic else KERNEL_GENERIC
        return w(True), w(self.spec["to"]), w(self.spec["f16"])

    def step(self, how, src, dst, fmt, act, inj, inj_ok=True):
        A = self.read32(src, fmt)
        out = A.copy()
        act = np.where((act < 0) | (act > 4), 4, act).astype(np.int32)
        use_inj = self.inj and inj_ok
        self.rew[:] = 0
        for n in range(N):
            orc, (p, e) = self.orcs[n], self.live[n]
            self._load(n, A[n])
            ia = inj[n, :(e if self.train_pursuit else p)][None] if use_inj else None
            _, r, d, rem = orc.step(act[n, :p][None], ia)
            out[n, :p] = orc.obs[0]
            self.rew[n, :p] = r[0].astype(np.float32)
            self.done[n], self.removed[n] = d[0], rem[0]
        self.store32(dst, fmt, out)
        self.t += 1
        if self.H:
            self.done |= (self.t >= self.H).astype(np.uint8) << 1
        self.catches += int(self.removed.sum())
        if self.auto_reset and self.done.any():   # the fused auto-reset: a second pass over what the first left in the destination
            B = self.read32(dst, fmt)
            for n in np.nonzero(self.done)[0]:
                self._reset_env(n, B[n])
                self.fused[n] += 1
            self.store32(dst, fmt, B)
        self.cur = (dst, fmt)
        self.last_entry = self.predict(how, use_inj)
        self.entries.append(self.last_entry)

    def reset(self, slot, fmt, mask, inj_pos=None, inj_map=None):
        B = self.read32(slot, fmt)
        for n in range(N):
            if mask is None or mask[n]:
                self.mid_episode_resets += int(mask is not None and self.t[n] > 0)
                self._reset_env(n, B[n], inj_pos, inj_map)
        self.store32(slot, fmt, B)
        self.cur = (slot, fmt)

    def state(self):
        """get_state at the capacity: pursuers that do not exist at (-1, -1), evader slots past the live count gone"""
        P, E = self.P, self.E
        st = dict(pos_p=np.full((N, P, 2), -1, np.int32), pos_e=np.full((N, E, 2), -1, np.int32), gone=np.ones((N, E), np.uint8),
                  term_p=np.zeros((N, P), np.uint8), term_e=np.zeros((N, E), np.uint8), map_id=np.zeros(N, np.int32),
                  tick=np.zeros(N, np.uint32), t=self.t.astype(np.int32))
        for n in range(N):
            s, (p, e) = self.orcs[n].get_state(), self.live[n]
            st["pos_p"][n, :p], st["term_p"][n, :p] = s["pos_p"][0], s["term_p"][0]
            st["pos_e"][n, :e], st["gone"][n, :e], st["term_e"][n, :e] = s["pos_e"][0], s["gone"][0], s["term_e"][0]
            st["map_id"][n], st["tick"][n] = s["map_id"][0], s["tick"][0]
        return st

    def set_pos(self, n, m):
        """env n takes the agents of env m (same counts), or -- per-env counts that differ -- its own pursuers moved round by one"""
        own = self.orcs[n].get_state()
        if self.live[m] == self.live[n]:
            src = self.orcs[m].get_state()
            for k in ("pos_p", "pos_e", "gone", "term_p", "term_e"):
                own[k] = src[k].copy()
        else:
            own["pos_p"], own["term_p"] = np.roll(own["pos_p"], 1, axis=1), np.roll(own["term_p"], 1, axis=1)
        self.orcs[n].set_state(own)
        return self.state()

    def apply(self, prim):
        k = prim[0]
        if k == "conv":
            _, src, sfmt, dst = prim
            if sfmt == "f":
                self.view(dst, "h")[:] = half_bits(self.view(src, "f"))
            else:
                self.view(dst, "f")[:] = widen(self.view(src, "h"))
        elif k in ("write", "edit"):
            _, slot, fmt, rows, salt = prim[:5]
            idx = (np.asarray(rows)[:, None] * self.D + np.arange(self.D)[None, :]).reshape(-1)
            v = sentinels(self.index_of[slot], idx, salt)
            self.view(slot, fmt)[idx] = v if fmt == "f" else half_bits(v)
        elif k == "step":
            self.step(*prim[1:])
        elif k == "reset":
            self.reset(*prim[1:])
        elif k == "zero":
            self.view(prim[1], "f")[:] = 0.0
            self.cur = (prim[1], "f")
        elif k == "set_t":
            self.t[:] = prim[1]
        elif k == "set_pos":
            return self.set_pos(prim[1], prim[2])
        elif k == "get_state":
            return self.state()
        elif k == "kernel":
            self.generic = bool(prim[1])
        elif k == "walk":
            self.walk_mode = prim[1]
        elif k == "params":
            self.catchr = prim[1]
            for n in range(N):
                self._curriculum_to(self.orcs[n], n)
        elif k == "cur":
            self.cw_env, self.cr_env = prim[1], prim[2]
            for n in range(N):
                self._curriculum_to(self.orcs[n], n)
        elif k == "inject":
            self.inj = bool(prim[1])
        elif k == "pending":
            for n, c in zip(prim[1], prim[2]):
                self.pending[n] = (int(c[0]), int(c[1]))
        else:
            assert k in ("inval", "launch"), k
        return None

    def start(self, first):
        """the initial reset into `first` and the staggered clocks: where every walk starts"""
        self.apply(("reset", first, self.fmt_of[first], None))
        self.apply(("set_t", AGES))


# ------------------------------------------------------------------------------------------------------------------ the walk
def circuit(kinds, rng):
    """Hierholzer's algorithm on the complete directed graph over `kinds`, self-loops included, with seeded choices: a closed walk of
    len(kinds) ** 2 + 1 vertices in which every ordered pair of kinds is adjacent exactly once"""
    out = {k: [kinds[i] for i in rng.permutation(len(kinds))] for k in kinds}
    stack, walk = [kinds[rng.randint(len(kinds))]], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == len(kinds) ** 2 + 1
    return walk


class _Planner(object):
    """turns a kind into prims, drawing the free parameters and keeping track of which buffer is current"""

    def __init__(self, name, rng, slots, first):
        self.rng, self.slots = rng, tuple(slots)
        xs, ys, self.P, self.E, R, fl = HANDLES[name]["shape"]
        self.n_inj = self.E if HANDLES[name]["kw"].get("train_pursuit", True) else self.P
        self.cur = (first, dict(slots)[first])
        self.salt = 0

    def other(self, fmt, exclude=()):
        names = [s for s, f in self.slots if f == fmt and s not in exclude]
        return names[self.rng.randint(len(names))]

    def ensure(self, fmt):
        """the current buffer in format fmt: itself, or converted by the caller into a non-current slot of that format"""
        slot, f = self.cur
        if f == fmt:
            return [], slot
        dst = self.other(fmt)
        return [("conv", slot, f, dst)], dst

    def actions(self):
        act = self.rng.randint(5, size=(N, self.P)).astype(np.int64)
        bad = self.rng.randint(8, size=act.shape) == 0   # one entry in eight is outside 0..4
        act[bad] = np.asarray(BAD_ACTIONS, np.int64)[self.rng.randint(len(BAD_ACTIONS), size=int(bad.sum()))]
        return act.astype(np.int32)

    def launch_args(self):
        return self.actions(), self.rng.randint(5, size=(N, self.n_inj)).astype(np.int32)

    def rows(self):
        pick = self.rng.rand(N * self.P) < 0.3
        pick[self.rng.randint(N * self.P)] = True
        return np.nonzero(pick)[0]

    def mask(self):
        m = (self.rng.rand(N) < 0.5).astype(np.uint8)
        m[self.rng.randint(N)] = 1
        return m

    def step(self, how, src, dst, fmt, inj_ok=True):
        act, inj = self.launch_args()
        self.cur = (dst, fmt)
        return ("step", how, src, dst, fmt, act, inj, inj_ok)

    def common(self, kind):
        rng = self.rng
        if kind == "set_t":
            return [("set_t", rng.randint(H, size=N))]
        if kind == "set_pos":
            n = rng.randint(N)
            return [("set_pos", n, (n + 1 + rng.randint(N - 1)) % N)]
        if kind == "get_state":
            return [("get_state",)]
        if kind in ("kernel_generic", "kernel_auto"):
            return [("kernel", kind == "kernel_generic")]
        if kind == "set_walk":
            return [("walk", int(rng.randint(3)))]
        if kind == "set_launch":
            return [("launch", int(rng.randint(4)))]
        if kind == "set_params":
            return [("params", float(rng.choice([0.01, 0.0, 0.5, -0.25])))]
        if kind == "curriculum":
            if rng.rand() < 0.5:
                return [("cur", None, None)]
            return [("cur", rng.choice([1.0, 0.5, 0.3], size=N), rng.choice([0.01, 0.0, 0.5], size=N))]
        if kind == "inject":
            return [("inject", bool(rng.rand() < 0.5))]
        if kind == "pending":
            envs = np.nonzero(self.mask())[0]
            return [("pending", envs, [(int(rng.choice([1, 2, self.P - 1, self.P, 1 + rng.randint(self.P)])),
                                        int(rng.choice([1, 3, self.E, 1 + rng.randint(self.E)]))) for _ in envs])]
        raise KeyError(kind)

    def reset_prims(self, kind, fmt_run="f"):
        pre, s = self.ensure("f") if fmt_run == "f" else ([], self.cur[0])
        self.cur = (s, fmt_run)
        return pre + [("reset", s, fmt_run, self.mask() if kind == "reset_mask" else None)]

    def abi(self, kind):
        rng = self.rng
        slot, fmt = self.cur
        if kind == "step":
            pre, s = self.ensure("f")
            return pre + [self.step("inplace", s, s, "f")]
        if kind == "step_foreign":   # another float32 slot, stepped from its own contents
            s = self.other("f", (slot,))
            return [self.step("inplace", s, s, "f")]
        if kind == "step_to":
            pre, s = self.ensure("f")
            return pre + [self.step("to", s, self.other("f", (s,)), "f")]
        if kind == "step_to_f16":
            pre, s = self.ensure("h")
            return pre + [self.step("f16", s, self.other("h", (s,)), "h")]
        if kind == "reinterpret":    # the current float32 slot's memory read as binary16, nothing written
            pre, s = self.ensure("f")
            return pre + [self.step("f16", s, self.other("h"), "h")]
        if kind in ("reset_all", "reset_mask"):
            return self.reset_prims(kind)
        if kind == "invalidate":
            return [("inval",)]
        if kind in ("write_current", "write_other"):
            self.salt += 1
            if kind == "write_current":
                return [("write", slot, fmt, self.rows(), self.salt), ("inval",)]
            s = [x for x, _ in self.slots if x != slot][rng.randint(len(self.slots) - 1)]
            return [("write", s, dict(self.slots)[s], self.rows(), self.salt)]   # no invalidate: another pointer is forgotten by itself
        if kind == "declare_zero":
            s = self.other("f")
            self.cur = (s, "f")
            return [("zero", s)]
        return self.common(kind)

    def py(self, kind, half):
        slot, fmt = self.cur
        if kind == "step":
            dst = slot if not half else ("own_b" if slot == "own_a" else "own_a")
            return [self.step("f16" if half else "inplace", slot, dst, fmt)]
        if kind == "step_to":
            ring = [s for s, _ in self.slots if s.startswith("r") and s != slot]
            return [self.step("f16" if half else "to", slot, ring[self.rng.randint(len(ring))], fmt)]
        if kind == "step_into":   # no evader actions on this entry point
            ring = [s for s, _ in self.slots if s.startswith("r") and s != slot]
            dst = ring[self.rng.randint(len(ring))] if self.rng.rand() < 0.5 else None
            if dst is None:
                return [self.step("f16", slot, "own_b" if slot == "own_a" else "own_a", fmt, False) if half else
                        self.step("inplace", slot, slot, fmt, False), ("into", None)]
            return [self.step("f16" if half else "to", slot, dst, fmt, False), ("into", dst)]
        if kind in ("reset_all", "reset_mask"):
            return self.reset_prims(kind, fmt)
        if kind in ("edit_seen", "edit_data"):
            self.salt += 1
            return [("edit", slot, fmt, self.rows(), self.salt, kind == "edit_seen")]
        return self.common(kind)


def walk(kinds, seed, name, python_half=None):
    """The ops of one walk over `kinds` on handle `name`, deterministic in its arguments: an Eulerian circuit over the kinds, so that every
    ordered pair of kinds occurs exactly once, with the free parameters (slots, masks, values, actions) drawn from the seed.  It starts
    after Model.start / the devices' start().  python_half None = through the C ABI, False / True = BatchedPursuitEvade itself with
    float32 / half observations."""
    rng = np.random.RandomState(seed)
    if python_half is None:
        slots, first = ABI_SLOTS, "f0"
    else:
        slots, first = py_slots(python_half), "own_a" if python_half else "own"
    pl = _Planner(name, rng, slots, first)
    return [dict(kind=k, prims=pl.abi(k) if python_half is None else pl.py(k, python_half)) for k in circuit(tuple(kinds), rng)]


def model_for(name, seed, python_half=None):
    if python_half is None:
        m = Model(name, seed)
        m.start("f0")
        return m
    m = Model(name, seed, py_slots(python_half), lambda s, f, n: n * (4 if f == "f" else 2))
    m.start("own_a" if python_half else "own")
    return m


def run_model(model, ops):
    for op in ops:
        for prim in op["prims"]:
            if prim[0] != "into":
                model.apply(prim)
        model.no_nan()
    return model


# ------------------------------------------------------------------------------------------------------------------ the GPU side
DEV = "cuda:0"


class Arena(object):
    """all test-owned observation memory: [guard][slot][guard][slot] ... [guard] in one byte tensor, every slot 16-byte aligned"""

    def __init__(self, model, names):
        import torch
        self.names, self.off = list(names), {}
        at = GUARD
        for s in self.names:
            self.off[s] = at
            at += (model.nbytes[s] + 15) // 16 * 16 + GUARD
        host = np.full(at, GUARD_BYTE, np.uint8)
        self.is_guard = np.ones(at, bool)
        for s in self.names:
            host[self.off[s]:self.off[s] + model.nbytes[s]] = model.buf[s]
            self.is_guard[self.off[s]:self.off[s] + model.nbytes[s]] = False
        self.raw = torch.as_tensor(host).to(DEV)
        assert all((self.raw.data_ptr() + o) % 16 == 0 for o in self.off.values())

    def view(self, slot, fmt, n):
        import torch
        o = self.off[slot]
        return self.raw[o:o + 4 * n].view(torch.float32) if fmt == "f" else self.raw[o:o + 2 * n].view(torch.float16)

    def host(self):
        return self.raw.cpu().numpy()


def make_env(name, seed, half=False):
    import torch
    from madrl_amd.pursuit import BatchedPursuitEvade
    kw = dict(obs_dtype=torch.float16) if half else {}
    return BatchedPursuitEvade(maps_of(HANDLES[name]), n_envs=N, device=DEV, seed=seed, env_id_base=BASE, max_steps=H, auto_reset=True,
                               per_env_counts=bool(HANDLES[name].get("live")), **dict(env_kwargs(HANDLES[name]), **kw))


def _differs(model, slot, fmt, got):
    """count of differing elements of a slot (its bytes beyond the elements compared as bytes)"""
    want = model.buf[slot]
    width = 4 if fmt == "f" else 2
    k = len(want) // width * width
    return int((got[:k].view(np.uint8).reshape(-1, width) != want[:k].reshape(-1, width)).any(axis=1).sum()) + int((got[k:] != want[k:]).sum())


class _Device(object):
    """what AbiDevice and PyDevice share: the env, its I/O tensors and the per-op comparison"""

    def __init__(self, env, model, arena_slots):
        import torch
        from madrl_amd import _lib
        self.torch, self._lib, self.L = torch, _lib, _lib.lib()
        self.model, self.env = model, env
        self.h, self.stream = self.env._handle, _lib.current_stream(self.env.device)
        self.arena = Arena(model, arena_slots)
        P, n_inj = model.P, (model.E if model.train_pursuit else model.P)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
        self.act, self.inj = z((N, P), torch.int32), z((N, n_inj), torch.int32)
        self.rew, self.done, self.removed = z((N, P), torch.float32), z(N, torch.uint8), z(N, torch.int32)
        self.cw, self.cr, self.mask = z(N, torch.float64), z(N, torch.float64), z(N, torch.uint8)
        self.inj_on, self.stepped = False, False

    def up(self, dst, a):
        dst.copy_(self.torch.as_tensor(np.ascontiguousarray(a)).to(dst.dtype).reshape(dst.shape))
        return dst

    def i32(self, fn):
        out = C.c_int32()
        self._lib.check(fn(self.h, C.byref(out)))
        return out.value

    def owned(self):
        return {}

    def compare(self, i, kind, prev):
        """after every op: guards, every slot, the outputs of a launch, the entry and the kinds"""
        where = "op %d (%s after %s)" % (i, kind, prev)
        self.torch.cuda.synchronize()
        m, host = self.model, self.arena.host()
        assert (host[self.arena.is_guard] == GUARD_BYTE).all(), "%s: %d guard bytes were written" % (where, int((host[self.arena.is_guard] != GUARD_BYTE).sum()))
        got = {s: host[self.arena.off[s]:self.arena.off[s] + m.nbytes[s]] for s in self.arena.names}
        got.update({s: t.contiguous().view(self.torch.uint8).reshape(-1).cpu().numpy() for s, t in self.owned().items()})
        for s, f in m.slots:
            bad = _differs(m, s, f, got[s])
            assert bad == 0, "%s: slot %s: %d elements differ from the model (current buffer: %s)" % (where, s, bad, m.cur)
        if self.stepped:
            rew, done, rem = self.rew.cpu().numpy(), self.done.cpu().numpy(), self.removed.cpu().numpy()
            bad = int((rew.view(np.int32) != m.rew.view(np.int32)).sum())
            assert bad == 0, "%s: %d rewards differ in their bits" % (where, bad)
            assert np.array_equal(done, m.done), "%s: done bytes %d differ: %r, model %r" % (where, int((done != m.done).sum()), done, m.done)
            assert np.array_equal(rem, m.removed), "%s: removed: %d differ" % (where, int((rem != m.removed).sum()))
            self.stepped = False
        entry = self.i32(self.L.madrl_pursuit_last_step_entry)
        assert entry == m.last_entry, "%s: last_step_entry %d, the header's rules give %d" % (where, entry, m.last_entry)
        kinds = (self.i32(self.L.madrl_pursuit_kernel_kind), self.i32(self.L.madrl_pursuit_step_to_kernel_kind),
                 self.i32(self.L.madrl_pursuit_step_to_f16_kernel_kind))
        assert kinds == m.kernel_kinds(), "%s: kernel kinds %r, the header's rules give %r" % (where, kinds, m.kernel_kinds())

    def check_state(self, want, where):
        st = self.env.get_state()
        for k in ("pos_p", "pos_e", "gone", "term_p", "term_e", "map_id", "tick", "t"):
            got = st[k].cpu().numpy()
            assert np.array_equal(got.astype(np.int64) & 0xFFFFFFFF, want[k].astype(np.int64) & 0xFFFFFFFF), \
                "%s: get_state %s: %d differ" % (where, k, int((got.astype(np.int64) != want[k].astype(np.int64)).sum()))

    def common(self, prim, res):
        """the prims that are one call on either level; True if handled"""
        k, L, ck, env = prim[0], self.L, self._lib.check, self.env
        if k == "set_t":
            env.set_state(dict(t=prim[1]))
        elif k == "set_pos":
            env.set_state({key: res[key] for key in ("pos_p", "pos_e", "gone", "term_p", "term_e", "map_id")})
        elif k == "get_state":
            self.check_state(res, "get_state")
        elif k == "kernel":
            env.set_kernel("generic" if prim[1] else "auto")
        elif k == "walk":
            env.set_walk(("auto", "alternate", "forward")[prim[1]])
        elif k == "launch":
            env.set_launch(max_blocks=prim[1])
        elif k == "inject":
            self.inj_on = prim[1]
        elif k == "pending":
            for n, c in zip(prim[1], prim[2]):
                env._pending[int(n)] = self.torch.tensor(c, dtype=self.torch.int32, device=DEV)
        else:
            return False
        return True


class AbiDevice(_Device):
    """the walk through the C ABI on env._handle: every pointer the library sees is a slot of the arena"""

    def __init__(self, env, model):
        _Device.__init__(self, env, model, [s for s, _ in ABI_SLOTS])

    def v(self, slot, fmt):
        return self.arena.view(slot, fmt, self.model.n)

    def apply(self, prim, res):
        k, L, ck, ptr, h, s = prim[0], self.L, self._lib.check, self._lib.ptr, self.h, self.stream
        if self.common(prim, res):
            return
        if k == "conv":
            self.v(prim[3], "h" if prim[2] == "f" else "f").copy_(self.v(prim[1], prim[2]))
        elif k == "write":
            _, slot, fmt, rows, salt = prim
            D = self.model.D
            idx = (np.asarray(rows)[:, None] * D + np.arange(D)[None, :]).reshape(-1)
            vals = self.torch.as_tensor(sentinels(self.model.index_of[slot], idx, salt)).to(DEV)
            self.v(slot, fmt)[self.torch.as_tensor(idx).to(DEV)] = vals.to(self.v(slot, fmt).dtype)
        elif k == "inval":
            ck(L.madrl_pursuit_invalidate_obs(h))
        elif k == "step":
            _, how, src, dst, fmt, act, inj, _ok = prim
            self.up(self.act, act), self.up(self.inj, inj)
            ia = ptr(self.inj) if self.inj_on else None
            out = (ptr(self.rew), ptr(self.done), ptr(self.removed), s)
            if how == "inplace":
                ck(L.madrl_pursuit_step(h, ptr(self.act), ia, ptr(self.v(dst, "f")), *out))
            elif how == "to":
                ck(L.madrl_pursuit_step_to(h, ptr(self.act), ia, ptr(self.v(src, "f")), ptr(self.v(dst, "f")), *out))
            else:
                ck(L.madrl_pursuit_step_to_f16(h, ptr(self.act), ia, ptr(self.v(src, "h")), ptr(self.v(dst, "h")), *out))
            self.stepped = True
        elif k == "reset":
            _, slot, fmt, mask = prim
            assert fmt == "f"
            ck(L.madrl_pursuit_reset(h, None if mask is None else ptr(self.up(self.mask, mask)), None, None, ptr(self.v(slot, "f")), s))
        elif k == "zero":
            self.v(prim[1], "f").zero_()
            ck(L.madrl_pursuit_declare_obs_zero(h, ptr(self.v(prim[1], "f")), s))
        elif k == "params":
            ck(L.madrl_pursuit_set_params(h, prim[1], 1.0))
        elif k == "cur":
            if prim[1] is None:
                ck(L.madrl_pursuit_set_curriculum(h, None, None))
            else:
                ck(L.madrl_pursuit_set_curriculum(h, ptr(self.up(self.cw, prim[1])), ptr(self.up(self.cr, prim[2]))))
        else:
            raise KeyError(k)

    def start(self):
        self.apply(("reset", "f0", "f", None), None)
        self.common(("set_t", AGES), None)


class PyDevice(_Device):
    """the walk through BatchedPursuitEvade itself: its own buffer(s) and a ring of three trajectory slots in the arena"""

    def __init__(self, env, model):
        torch = __import__("torch")
        _Device.__init__(self, env, model, ["r0", "r1", "r2"])
        half = env.obs_dtype is torch.float16
        self.half, self.fmt = half, "h" if half else "f"
        m = model
        self.own = dict(zip(("own_a", "own_b"), env._half_pair)) if half else {"own": env._obs}
        for s, t in self.own.items():   # the env's zeroed buffers take their sentinels like any slot: an edit the env must notice
            src = m.view(s, self.fmt)
            t.view(-1).copy_(torch.as_tensor((src.view(np.float16) if half else src).copy()))
        self.into = None

    def owned(self):
        return self.own

    def tensor(self, slot):
        if slot in self.own:
            return self.own[slot]
        return self.arena.view(slot, self.fmt, self.model.n).view(N, self.model.P, self.model.D)

    def result(self, out, dst):
        obs, rew, done, info = out
        want = self.tensor(dst)
        assert obs.data_ptr() == want.data_ptr() == self.env.obs_buffer.data_ptr() and obs.dtype == want.dtype
        self.rew.copy_(rew), self.done.copy_(info["done_bits"]), self.removed.copy_(info["removed"])
        assert np.array_equal(done.cpu().numpy(), (info["done_bits"].cpu().numpy() & 1) != 0)
        self.stepped = True

    def apply(self, prim, res):
        k, env, torch = prim[0], self.env, self.torch
        if self.common(prim, res):
            return
        if k == "step":
            _, how, src, dst, fmt, act, inj, inj_ok = prim
            assert env.obs_buffer.data_ptr() == self.tensor(src).data_ptr()
            self.up(self.act, act), self.up(self.inj, inj)
            ea = self.inj if self.inj_on else None
            if not inj_ok:
                self.pending_step = (src, dst)   # issued by the "into" prim that follows
            elif dst == src or (self.half and dst in self.own):
                self.result(env.step(self.act, evader_actions=ea), dst)
            else:
                self.result(env.step_to(self.act, self.tensor(dst), evader_actions=ea), dst)
        elif k == "into":
            src, dst = self.pending_step
            obs = env.step_into(self.act, self.rew, self.done, obs_out=None if prim[1] is None else self.tensor(dst))
            assert obs.data_ptr() == self.tensor(dst).data_ptr() == env.obs_buffer.data_ptr()
            self.removed.copy_(env._removed)
            self.stepped = True
        elif k == "reset":
            _, slot, fmt, mask = prim
            obs = env.reset() if mask is None else env.reset(mask=self.up(self.mask, mask))
            assert obs.data_ptr() == self.tensor(slot).data_ptr()
        elif k == "edit":
            _, slot, fmt, rows, salt, seen = prim
            D = self.model.D
            idx = (np.asarray(rows)[:, None] * D + np.arange(D)[None, :]).reshape(-1)
            vals = torch.as_tensor(sentinels(self.model.index_of[slot], idx, salt)).to(DEV).to(env.obs_buffer.dtype)
            buf = env.obs_buffer
            assert buf.data_ptr() == self.tensor(slot).data_ptr()
            version = buf._version
            if seen:    # through the tensor: the version counter moves, no invalidate call
                buf.view(-1)[torch.as_tensor(idx).to(DEV)] = vals
                assert buf._version != version
            else:       # behind PyTorch's back
                buf.data.view(-1)[torch.as_tensor(idx).to(DEV)] = vals
                assert buf._version == version
                env.invalidate_obs()
        elif k == "params":
            env.set_param_values(dict(catchr=prim[1]))
        elif k == "cur":
            if prim[1] is None:
                env.clear_curriculum()
            else:
                env.set_curriculum(constraint_window=prim[1], catchr=prim[2])
        else:
            raise KeyError(k)

    def start(self):
        self.apply(("reset", "own_a" if self.half else "own", self.fmt, None), None)
        self.common(("set_t", AGES), None)


def replay(env, model, ops, python=False):
    """Every op on the model, then on env -- through the C ABI on env._handle, or (python=True) through BatchedPursuitEvade's own methods --
    then the comparison; the message of a failure names the op's index and kind, the kind before it and how many elements differ."""
    dev = PyDevice(env, model) if python else AbiDevice(env, model)
    dev.start()
    dev.compare(-1, "start", None)
    prev = "start"
    for i, op in enumerate(ops):
        for prim in op["prims"]:
            res = model.apply(prim) if prim[0] != "into" else None
            dev.apply(prim, res)
        dev.compare(i, op["kind"], prev)
        prev = op["kind"]
    dev.check_state(model.state(), "after the last op")
