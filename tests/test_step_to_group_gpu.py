"""The two-buffer step on the multi-wavefront family: step_to of a handle on an XG / XLG line of csrc/pursuit_to_specializations.def
(pursuit_group_kernel over a TGShape / TLGShape, pursuit_group.hpp).

The method is that of tests/test_step_to_gpu.py: twins with the same seed, one stepping in place -- the yardstick, which the rest of the
suite pins to the reference's goldens and the C oracle -- the other through a ring of three buffers with step_to, compared bit for bit
after every hop.  The in-place buffer and the ring's first slot start as 7.0, the ring's other slots as 101.0 and 102.0, and the envs are
told so (invalidate_obs): a cell a step never stores, a read from the wrong slot and a mask that claims "zero" for a cell that holds 7.0
are all visible.  The conditions that keep a case from passing emptily (resets occurred, kept cells exist) are asserted on the in-place
twin."""
import pytest
import torch

from helpers import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ENVS, STEPS = 7, 12


def _maps(pool, xs, ys):
    from madrl_amd.maps import rectangle_map, synthetic_map_pool
    return synthetic_map_pool(3, xs, ys) if pool else [rectangle_map(xs, ys)]


def _counts(p, e):
    return [(p, e), (p - 1, e - 1), (15, 15), (4, 4), (1, 1), (p, 1), (12, 0)]


AUTHORS = dict(obs_range=11, flatten=True, surround=True, sample_maps=True)
# name: (map size, pool of maps, env kwargs, per-env counts or None, twin kwargs)
CASES = {
    "XG_c5_16v60": ((32, 32), False, dict(n_pursuers=16, n_evaders=60, obs_range=7, flatten=True, surround=True, n_catch=2), None, {}),
    "XG_authors_30v50": ((32, 32), True, dict(n_pursuers=30, n_evaders=50, **AUTHORS), None, {}),
    "XG_authors_30v30": ((32, 32), True, dict(n_pursuers=30, n_evaders=30, **AUTHORS), None, {}),
    "XLG_authors_30v50": ((32, 32), True, dict(n_pursuers=30, n_evaders=50, per_env_counts=True, **AUTHORS), _counts(30, 50), {}),
    "XLG_authors_30v30": ((32, 32), True, dict(n_pursuers=30, n_evaders=30, per_env_counts=True, **AUTHORS), _counts(30, 30), {}),
    "XLG_20v50": ((16, 16), False, dict(n_pursuers=20, n_evaders=50, obs_range=5, flatten=True, per_env_counts=True), _counts(20, 50), {}),
}
# long rows past the authors' two mask words, on rectangle_map (the last XG lines of csrc/pursuit_to_specializations.def): a mask word of
# 5 slots (a remainder batch of 1 after one batch of MADRL_PG_TO_BATCH = 4), one of 7 (a remainder batch of 3), and the limit: 32 slots,
# four mask words, 64 pursuers
CASES["XG_13_slots_36v12"] = ((10, 10), False, dict(n_pursuers=36, n_evaders=12, obs_range=11, flatten=True, surround=False, n_catch=2), None, {})
CASES["XG_23_slots_46v10"] = ((12, 12), False, dict(n_pursuers=46, n_evaders=10, obs_range=13, flatten=True, surround=False, n_catch=2), None, {})
CASES["XG_32_slots_64v20"] = ((12, 12), False, dict(n_pursuers=64, n_evaders=20, obs_range=13, flatten=True, surround=False, n_catch=2,
                                                    reward_mech="global"), None, {})
CASES["XG_authors_30v50_global"] = CASES["XG_authors_30v50"][:2] + (dict(CASES["XG_authors_30v50"][2], reward_mech="global"), None, {})
CASES["XLG_20v50_global"] = CASES["XLG_20v50"][:2] + (dict(CASES["XLG_20v50"][2], reward_mech="global"), _counts(20, 50), {})
CASES["XG_c5_16v60_evader_actions"] = CASES["XG_c5_16v60"][:4] + (dict(evader_actions=True),)
CASES["XLG_authors_30v50_alternate"] = CASES["XLG_authors_30v50"][:4] + (dict(walk="alternate"),)
CASES["XG_authors_30v30_one_env_per_workgroup"] = CASES["XG_authors_30v30"][:4] + (dict(max_blocks=None),)


# The seed of every case's twins: one for which the in-place twin still holds a 7.0 after the twelve hops.  The live cases keep whole rows
# of absent pursuers with any seed; a fixed-shape case keeps a 7.0 only where a window cell lies outside the map after every reset (with
# this seed 4 elements of the 16 v 60 case and 52 of the 30-pursuer cases; seed 21 of tests/test_step_to_gpu.py leaves none)
SEED = 1


def _mk(name, max_blocks=2, walk=None):
    from madrl_amd.pursuit import BatchedPursuitEvade
    (xs, ys), pool, kw = CASES[name][:3]
    env = BatchedPursuitEvade(_maps(pool, xs, ys), n_envs=N_ENVS, device=DEV, seed=SEED, max_steps=3, auto_reset=True, **kw)
    if max_blocks is not None:
        env.set_launch(max_blocks=max_blocks)   # a workgroup walks several envs: the loop-carried state is exercised
    if walk is not None:
        env.set_walk(walk)
    return env


class Twins(object):
    """`ref` steps in place; `env` steps through `ring`, whose first slot is its own buffer"""

    def __init__(self, name):
        self.counts = CASES[name][3]
        tkw = dict(CASES[name][4])
        self.with_eact = tkw.pop("evader_actions", False)
        self.ref, self.env = _mk(name, **tkw), _mk(name, **tkw)
        self.P, self.E = int(self.ref.n_pursuers), int(self.ref.n_evaders)
        for e in (self.ref, self.env):
            e.obs_buffer.fill_(7.0)
        first = self.env.obs_buffer
        self.ring = [first, torch.full_like(first, 101.0), torch.full_like(first, 102.0)]
        self.at = 0
        self.gen = torch.Generator(device="cpu").manual_seed(5)
        for e in (self.ref, self.env):
            e.invalidate_obs()
            if self.counts is not None:
                c = torch.tensor(self.counts, dtype=torch.int32, device=DEV)
                e.set_agent_counts(c[:, 0], c[:, 1])
        a, b = self.ref.reset(), self.env.reset()
        assert same_bits(a, b)

    def actions(self):
        act = torch.randint(0, 5, (N_ENVS, self.P), generator=self.gen).to(torch.int32).to(DEV)
        eact = torch.randint(0, 5, (N_ENVS, self.E), generator=self.gen).to(torch.int32).to(DEV) if self.with_eact else None
        return act, eact

    def check_results(self, ra, rb, what):
        (oa, rwa, da, ia), (ob, rwb, db, ib) = ra, rb
        assert same_bits(oa, ob), (what, "observations")
        assert same_bits(rwa, rwb), (what, "rewards")
        assert torch.equal(da, db), (what, "done")
        for k in ("done_bits", "removed", "truncated", "count_overflow"):
            assert torch.equal(ia[k], ib[k]), (what, k)

    def hop(self, what):
        act, eact = self.actions()
        nxt = (self.at + 1) % 3
        prev_before = self.ring[self.at].clone()
        ra = self.ref.step(act, evader_actions=eact)
        rb = self.env.step_to(act, self.ring[nxt], evader_actions=eact)
        self.check_results(ra, rb, what)
        assert rb[0].data_ptr() == self.ring[nxt].data_ptr() and self.env.obs_buffer.data_ptr() == self.ring[nxt].data_ptr()
        assert same_bits(self.ring[nxt], self.ref.obs_buffer), (what, "slot")
        assert same_bits(self.ring[self.at], prev_before), (what, "the previous slot was written")
        self.at = nxt

    def in_place(self, what):
        act, eact = self.actions()
        self.check_results(self.ref.step(act, evader_actions=eact), self.env.step(act, evader_actions=eact), what)
        assert same_bits(self.ring[self.at], self.ref.obs_buffer), (what, "slot")

    def check_state(self):
        a, b = self.ref.get_state(), self.env.get_state()
        for k in a:
            assert torch.equal(a[k], b[k]), k

    def recount(self):
        """per-env counts: other pending counts, taken at each env's next fused reset (the row count of an env changes between the passes)"""
        if self.counts is None:
            return
        c = torch.tensor(self.counts[::-1], dtype=torch.int32, device=DEV)
        for e in (self.ref, self.env):
            e.set_agent_counts(c[:, 0], c[:, 1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_group_step_to_equals_the_in_place_step(name):
    tw = Twins(name)
    assert tw.env.kernel_kind == "wave" and tw.env.step_to_kernel_kind == "wave"
    dones = 0
    for k in range(STEPS):
        if k == 4:
            tw.recount()
        tw.hop(k)
        dones += int((tw.ref._done != 0).sum())
    # the yardstick's own run: fused resets (and their second observation pass) occurred, cells that no step ever stores still hold
    # the fill value at the end, and the slot holds them too and nothing of the ring's other fill values
    assert dones >= 3 * N_ENVS
    assert bool((tw.ref.obs_buffer == 7.0).any())
    assert bool((tw.ring[tw.at] == 7.0).any()) and not bool((tw.ring[tw.at] > 100.0).any())
    tw.check_state()
    assert tw.env.step_to_kernel_kind == "wave"


@pytest.mark.parametrize("name", ["XG_c5_16v60", "XG_authors_30v50", "XLG_authors_30v50", "XLG_authors_30v30", "XLG_20v50"])
def test_group_knowledge_travels_with_the_buffer(name):
    """six hops, four in-place steps on the last slot without any invalidate, four more hops: what the fast path knows about the buffer
    (the stale-zero masks) must describe the slot the env is on"""
    tw = Twins(name)
    assert tw.env.step_to_kernel_kind == "wave"
    for k in range(6):
        tw.hop(("hop", k))
    for k in range(4):
        tw.in_place(("in place", k))
    tw.recount()
    for k in range(4):
        tw.hop(("hop again", k))
    tw.check_state()
