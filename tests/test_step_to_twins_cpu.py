"""CPU test (-m "not gpu") of the comparisons of step_to_twins.py, which otherwise only ever run on a GPU: InPlaceTwins and HalfTwins
pass over two stand-in envs that are right by construction, and one wrong bit or element in one env, or a run that could only pass
emptily, raises.

Toy is the stand-in: CPU tensors and the surface the harness touches, nothing of PursuitEvade.  Its rule: an env has a position that the
actions move; a pass stores the elements (j + position + row) % 3 != 0 of the rows of its live pursuers, never the last element of a
row, and keeps the others; a two-buffer step carries the kept elements over bit for bit; every third step ends the episode, takes the
pending counts and makes a second pass.  A half instance stores value.to(float16)."""
import pytest
import torch

from step_to_twins import F16, F32, Case, HalfTwins, InPlaceTwins

N, P, E, D, ENV, HOPS = 4, 3, 2, 6, 1, 8
VALUES = torch.tensor([0.1, 0.3, 0.5, 1.0 / 30000, 1.0, 0.2, 0.3], dtype=F32)   # 0.3: 0x34CD to nearest even, 0x34CC truncated
COUNTS = [(3, 2), (2, 1), (1, 2), (3, 0)]
CASES = {
    "plain": Case(None, None, {}, None, {}),
    "counts": Case(None, None, {}, COUNTS, {}),
    "evader_actions": Case(None, None, {}, None, dict(evader_actions=True)),
    "counts_evader_actions_sightings": Case(None, None, {}, COUNTS, dict(evader_actions=True, rne=True, subnormal=True)),
}


def _flip(t, *index):
    """the lowest bit of one element"""
    t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])[index] ^= 1


class Toy(object):
    """defect: planted once, in env ENV, at step `when` (the first step is 0); mode: a way the whole run goes, the same in both twins"""

    def __init__(self, dtype, device, defect=None, when=1, mode=None):
        self.n_pursuers, self.n_evaders, self.defect, self.when, self.mode = P, E, defect, when, mode
        self._obs = torch.zeros((N, P, D), dtype=dtype, device=device)
        self.pending = torch.tensor([[P, E]] * N, dtype=torch.int32, device=device)
        self.kernel_kind = self.step_to_kernel_kind = "toy"
        self.steps = 0

    obs_buffer = property(lambda self: self._obs)

    def set_kernel(self, kind):
        self.kernel_kind = self.step_to_kernel_kind = kind

    def invalidate_obs(self):
        pass

    def set_agent_counts(self, n_pursuers, n_evaders):
        self.pending = torch.stack([n_pursuers, n_evaders], dim=1).to(torch.int32)

    def agent_counts(self):
        return self.pending.clone(), self.live.clone()

    def get_state(self):
        st = dict(pos=self.pos.clone(), t=self.t.clone(), tick=self.tick.clone(), pending=self.pending.clone(), live=self.live.clone())
        if self.defect in ("state_pos", "state_t", "state_tick"):
            st[self.defect[6:]][ENV] ^= 1
        return st

    def _pass(self, dest, envs, stepping):
        k, j, pos = torch.arange(P)[None, :, None], torch.arange(D)[None, None, :], self.pos[:, None, None]
        store = ((j + pos + k) % 3 != 0) & (j < D - 1) & (k < self.live[:, 0].long()[:, None, None])
        if self.mode == "no_kept_cell_survives":
            store = torch.ones_like(store)
        if self.mode == "nothing_stored_after_the_reset" and stepping:
            store = torch.zeros_like(store)
        store = store & envs[:, None, None]
        dest[store] = VALUES[(pos + k + 2 * j) % len(VALUES)].to(dest.dtype)[store]
        return store

    def reset(self):
        self.live = self.pending.clone()
        self.pos, self.t, self.tick = torch.arange(N) * 2 % 7, torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
        self._pass(self._obs, torch.ones(N, dtype=torch.bool), False)
        return self._obs

    def step(self, actions, evader_actions=None):
        return self.step_to(actions, self._obs, evader_actions=evader_actions)

    def step_to(self, actions, dest, evader_actions=None):
        src = self._obs
        if dest.data_ptr() != src.data_ptr():
            dest.copy_(src)   # the kept elements
        self.pos = (self.pos + actions.sum(1) + (0 if evader_actions is None else evader_actions.sum(1))) % 7
        if self.mode == "an_env_never_ends":
            self.t[torch.arange(N) != ENV] += 1
        else:
            self.t += 1
        live = torch.arange(P)[None, :] < self.live[:, :1]
        rew = torch.where(live, self.pos[:, None] * 0.25 + torch.arange(P)[None, :], torch.zeros(())).to(F32)
        ended = self.t >= 3
        info = dict(done_bits=ended.to(torch.uint8) << 1, removed=(self.pos % 3).to(torch.int32), truncated=ended.clone(),
                    count_overflow=torch.zeros(N, dtype=torch.bool))
        stored = self._pass(dest, torch.ones(N, dtype=torch.bool), True)
        if bool(ended.any()):   # the fused reset and its second pass
            if self.mode != "pending_counts_never_taken":
                self.live = torch.where(ended[:, None], self.pending, self.live)
            self.tick += ended.to(torch.int32)
            self.pos = torch.where(ended, (self.pos * 3 + self.tick) % 7, self.pos)
            self.t = torch.where(ended, torch.zeros_like(self.t), self.t)
            stored |= self._pass(dest, ended, True)
        self._obs = out = dest
        done = ended.clone()
        if self.defect is not None and self.steps >= self.when:
            out = self._plant(src, dest, stored, rew, done, info)
        self.steps += 1
        return out, rew, done, info

    def _plant(self, src, dest, stored, rew, done, info):
        d, kept = self.defect, (ENV, 0, D - 1)   # (the last element of a row is never stored)
        where = stored[ENV].nonzero()[0]
        if d == "truncated_half":   # at the first stored 0.3 of the env there is
            hit = (stored[ENV] & (dest[ENV].view(torch.int16) == 0x34CD)).nonzero()
            if len(hit) == 0:
                return dest
            dest.view(torch.int16)[(ENV,) + tuple(hit[0])] = 0x34CC
        elif d == "stored_element_one_ulp":
            _flip(dest, ENV, *where)
        elif d == "kept_element_zeroed":
            dest[kept] = 0.0
        elif d == "kept_half_neighbour":   # widened, and the half of the next binary16 value stored
            dest.view(torch.int16)[kept] += 1
        elif d == "source_written":
            _flip(src, ENV, *where)
        elif d == "returned_from_another_tensor":
            self.defect = None
            return dest.clone()
        elif d == "obs_buffer_left_elsewhere":
            self._obs = dest.clone()
        elif d in ("guard_before_the_first_slot", "guard_after_the_last_slot"):
            raw = torch.empty(0, dtype=torch.uint8).set_(dest.untyped_storage())
            first = dest.storage_offset() * dest.element_size()
            raw[first - 1 if d == "guard_before_the_first_slot" else first + dest.numel() * dest.element_size()] = 0
        elif d == "reward":
            _flip(rew, ENV, 0)
        elif d == "done":
            done[ENV] = ~done[ENV]
        elif d in ("truncated", "count_overflow"):
            info[d][ENV] = ~info[d][ENV]
        elif d in ("done_bits", "removed"):
            info[d][ENV] ^= 1
        else:
            assert d.startswith("state_"), d
            return dest
        self.defect = None
        return dest


def _make(defect=None, when=1, mode=None):
    """the harness's make=: the second env it asks for (InPlaceTwins.env, HalfTwins.h) carries the defect"""
    made = []

    def make(case, obs_dtype=F32, n=None, device="cpu"):
        assert n == N
        made.append(Toy(obs_dtype, device, defect if made else None, when, mode))
        return made[-1]
    return make


def _in_place(case, **kw):
    tw = InPlaceTwins(CASES[case], n=N, device="cpu", make=_make(**kw))
    for k in range(4):
        tw.hop(("hop", k))
    for k in range(2):
        tw.in_place(("in place", k))
    tw.recount()
    for k in range(4):
        tw.hop(("hop again", k))
    tw.check_state()
    return tw


def _half(case, **kw):
    tw = HalfTwins(CASES[case], n=N, device="cpu", make=_make(**kw))
    tw.run(HOPS)
    tw.finish()
    return tw


@pytest.mark.parametrize("case", sorted(CASES))
def test_right_stand_ins_pass_in_place_twins(case):
    tw = _in_place(case)
    assert tw.ring[tw.at].data_ptr() == tw.env.obs_buffer.data_ptr() != tw.ref.obs_buffer.data_ptr()
    assert bool((tw.ring[tw.at] == 7.0).any()) and not bool((tw.ring[tw.at] > 100.0).any())   # kept cells travelled from slot to slot
    if CASES[case].counts is not None:
        assert torch.equal(tw.env.agent_counts()[1], torch.tensor(COUNTS[::-1], dtype=torch.int32))


@pytest.mark.parametrize("case", sorted(CASES))
def test_right_stand_ins_pass_half_twins(case):
    tw = _half(case)
    assert tw.rne_differs and tw.subnormal and int(tw.dones.sum()) == 2 * N and tw.h.obs_buffer.dtype is F16
    assert tw.hr.slots[(HOPS - 1) % 3].data_ptr() == tw.h.obs_buffer.data_ptr()


def test_half_kernel_is_set_on_the_half_twin_alone():
    tw = HalfTwins(CASES["plain"], n=N, half_kernel="generic", device="cpu", make=_make())
    assert tw.h.kernel_kind == "generic" and tw.f.kernel_kind == "toy"


# defect: the message of the assertion that must catch it, in InPlaceTwins and in HalfTwins (None: the assertion has no message)
DEFECTS = {
    "stored_element_one_ulp": ("observations", "slot"),
    "kept_element_zeroed": ("observations", "slot"),
    "source_written": ("previous slot was written", "obs_prev was written"),
    "returned_from_another_tensor": (None, None),
    "obs_buffer_left_elsewhere": (None, None),
    "reward": ("rewards", "rewards"),
    "done": ("'done'", "'done'"),
    "done_bits": ("done_bits", "done_bits"),
    "removed": ("removed", "removed"),
    "truncated": ("truncated", "truncated"),
    "count_overflow": ("count_overflow", "count_overflow"),
    "state_pos": ("^pos$", "^pos$"),
    "state_t": ("^t$", "^t$"),
    "state_tick": ("^tick$", "^tick$"),
}
HALF_DEFECTS = {
    "truncated_half": "slot",
    "kept_half_neighbour": "slot",
    "guard_before_the_first_slot": "guard band",
    "guard_after_the_last_slot": "guard band",
}
EMPTY_RUNS = {
    "no_kept_cell_survives": "no kept cell still reads 7.0",
    "nothing_stored_after_the_reset": "no kept cell was ever stored",
    "an_env_never_ends": "every env ended an episode",
    "pending_counts_never_taken": "the changed counts were never taken",
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_one_wrong_bit_raises_in_place_twins(defect):
    with pytest.raises(AssertionError, match=DEFECTS[defect][0]):
        _in_place("counts_evader_actions_sightings", defect=defect)


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_one_wrong_bit_raises_half_twins(defect):
    with pytest.raises(AssertionError, match=DEFECTS[defect][1]):
        _half("counts_evader_actions_sightings", defect=defect)


@pytest.mark.parametrize("defect", sorted(HALF_DEFECTS))
def test_one_wrong_half_or_guard_byte_raises(defect):
    with pytest.raises(AssertionError, match=HALF_DEFECTS[defect]):
        _half("plain", defect=defect, when=2 if defect == "guard_after_the_last_slot" else 0)   # (step 0 is on slot 0, step 2 on the last)


@pytest.mark.parametrize("mode", sorted(EMPTY_RUNS))
def test_a_run_that_could_only_pass_emptily_raises(mode):
    with pytest.raises(AssertionError, match=EMPTY_RUNS[mode]):
        _half("counts" if mode == "pending_counts_never_taken" else "plain", mode=mode)
