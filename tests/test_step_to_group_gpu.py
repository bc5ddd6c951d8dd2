"""The two-buffer step on the multi-wavefront family: step_to of a handle on an XG / XLG line of csrc/pursuit_to_specializations.def
(pursuit_group_kernel over a TGShape / TLGShape, pursuit_group.hpp).

The method is that of tests/test_step_to_gpu.py, over the same harness (tests/step_to_twins.py: InPlaceTwins): twins with the same seed,
one stepping in place -- the yardstick, which the rest of the suite pins to the reference's goldens and the C oracle -- the other
through a ring of three buffers with step_to, compared bit for bit after every hop.  The in-place buffer and the ring's first slot start as 7.0, the ring's other slots as 101.0 and 102.0, and the envs are
told so (invalidate_obs): a cell a step never stores, a read from the wrong slot and a mask that claims "zero" for a cell that holds 7.0
are all visible.  The conditions that keep a case from passing emptily (resets occurred, kept cells exist) are asserted on the in-place
twin."""
import pytest

from step_to_twins import Case, InPlaceTwins

pytestmark = pytest.mark.gpu

N_ENVS, STEPS = 7, 12


def _counts(p, e):
    return [(p, e), (p - 1, e - 1), (15, 15), (4, 4), (1, 1), (p, 1), (12, 0)]


AUTHORS = dict(obs_range=11, flatten=True, surround=True, sample_maps=True)
CASES = {
    "XG_c5_16v60": Case("rect", (32, 32), dict(n_pursuers=16, n_evaders=60, obs_range=7, flatten=True, surround=True, n_catch=2), None, {}),
    "XG_authors_30v50": Case("pool", (32, 32), dict(n_pursuers=30, n_evaders=50, **AUTHORS), None, {}),
    "XG_authors_30v30": Case("pool", (32, 32), dict(n_pursuers=30, n_evaders=30, **AUTHORS), None, {}),
    "XLG_authors_30v50": Case("pool", (32, 32), dict(n_pursuers=30, n_evaders=50, per_env_counts=True, **AUTHORS), _counts(30, 50), {}),
    "XLG_authors_30v30": Case("pool", (32, 32), dict(n_pursuers=30, n_evaders=30, per_env_counts=True, **AUTHORS), _counts(30, 30), {}),
    "XLG_20v50": Case("rect", (16, 16), dict(n_pursuers=20, n_evaders=50, obs_range=5, flatten=True, per_env_counts=True), _counts(20, 50), {}),
}
# long rows past the authors' two mask words, on rectangle_map (the last XG lines of csrc/pursuit_to_specializations.def): a mask word of
# 5 slots (a remainder batch of 1 after one batch of MADRL_PG_TO_BATCH = 4), one of 7 (a remainder batch of 3), and the limit: 32 slots,
# four mask words, 64 pursuers
CASES["XG_13_slots_36v12"] = Case("rect", (10, 10), dict(n_pursuers=36, n_evaders=12, obs_range=11, flatten=True, surround=False, n_catch=2), None, {})
CASES["XG_23_slots_46v10"] = Case("rect", (12, 12), dict(n_pursuers=46, n_evaders=10, obs_range=13, flatten=True, surround=False, n_catch=2), None, {})
CASES["XG_32_slots_64v20"] = Case("rect", (12, 12), dict(n_pursuers=64, n_evaders=20, obs_range=13, flatten=True, surround=False, n_catch=2,
                                                         reward_mech="global"), None, {})
CASES["XG_authors_30v50_global"] = CASES["XG_authors_30v50"]._replace(env=dict(CASES["XG_authors_30v50"].env, reward_mech="global"))
CASES["XLG_20v50_global"] = CASES["XLG_20v50"]._replace(env=dict(CASES["XLG_20v50"].env, reward_mech="global"))
CASES["XG_c5_16v60_evader_actions"] = CASES["XG_c5_16v60"]._replace(twin=dict(evader_actions=True))
CASES["XLG_authors_30v50_alternate"] = CASES["XLG_authors_30v50"]._replace(twin=dict(walk="alternate"))
CASES["XG_authors_30v30_one_env_per_workgroup"] = CASES["XG_authors_30v30"]._replace(twin=dict(max_blocks=None))


# The seed of every case's twins: one for which the in-place twin still holds a 7.0 after the twelve hops.  The live cases keep whole rows
# of absent pursuers with any seed; a fixed-shape case keeps a 7.0 only where a window cell lies outside the map after every reset (with
# this seed 4 elements of the 16 v 60 case and 52 of the 30-pursuer cases; seed 21 of tests/test_step_to_gpu.py leaves none)
SEED = 1


def _twins(name):
    return InPlaceTwins(CASES[name], n=N_ENVS, seed=SEED)


@pytest.mark.parametrize("name", sorted(CASES))
def test_group_step_to_equals_the_in_place_step(name):
    tw = _twins(name)
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
    tw = _twins(name)
    assert tw.env.step_to_kernel_kind == "wave"
    for k in range(6):
        tw.hop(("hop", k))
    for k in range(4):
        tw.in_place(("in place", k))
    tw.recount()
    for k in range(4):
        tw.hop(("hop again", k))
    tw.check_state()
