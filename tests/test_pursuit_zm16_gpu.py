"""GPU tests (-m gpu): the 16-bit-per-lane stale-zero masks of the one-wavefront Pursuit kernel (madrl_amd/csrc/pursuit_zm16.hpp).

Shapes that have the format (flatten, at most 5 float4 slots per lane, at most 4 of them with a channel-1 / 2 cell) keep 128 B of masks per
env in the first half of the state buffer's mask region; the others keep the 256 B dword form.  70 envs on 3 workgroups (every workgroup
walks more than 20 envs: the loop-carried prefetch of record, action and mask words runs), max_steps 40 with auto-reset (the two-pass reset
path runs).  Everything is compared bit for bit with the C oracle, step by step.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, BLOCKS, H = 70, 3, 40

# name -> (map side, pursuers, evaders, obs_range, flatten, slots per lane)
SHAPES = {
    "c2_8v30_r7": (16, 8, 30, 7, True),       # 5 slots per lane: every lane drops one bit position
    "5v9_r5": (16, 5, 9, 5, True),            # 2 slots per lane
    "tiny5_4v3_r3": (5, 4, 3, 3, True),       # 1 slot per lane
    "13v51_r7": (16, 13, 51, 7, True),        # 8 slots per lane: the dword form
    "c2_hwc": (16, 8, 30, 7, False),          # (R, R, 4) rows: the dword form
}


def _kw(name):
    side, P, E, R, flatten = SHAPES[name]
    return side, dict(n_pursuers=P, n_evaders=E, obs_range=R, n_catch=2, surround=True, flatten=flatten, reward_mech="local")


def _pair(name, seed=11):
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    from oracle import pursuit as po
    side, kw = _kw(name)
    maps = [rectangle_map(side, side)]
    env = BatchedPursuitEvade(maps, n_envs=N, device=DEV, seed=seed, env_id_base=500, max_steps=H, auto_reset=True, kernel="auto", **kw)
    env.set_launch(max_blocks=BLOCKS)
    assert env.kernel_kind == "wave"
    orc = po.PursuitOracle(maps, n_envs=N, seed=seed, env_id_base=500, **kw)
    return env, orc


def _cmp_state(env, orc, msg):
    sg, sr = env.get_state(), orc.get_state()
    for k in ("pos_p", "pos_e", "gone", "term_p", "term_e", "map_id"):
        assert np.array_equal(sg[k].cpu().numpy(), sr[k]), "%s: state[%s]" % (msg, k)
    assert np.array_equal(sg["tick"].cpu().numpy().view(np.uint32), sr["tick"]), msg + ": tick"


def _run_against_oracle(name, T, sevens):
    """T free-running steps of `name` against the oracle.  sevens: channels 1 and 2 of every row hold 7.0 after the reset, on both sides,
    and the env is told that nothing is known about its buffer."""
    env, orc = _pair(name)
    side, kw = _kw(name)
    P, R = kw["n_pursuers"], kw["obs_range"]
    obs, oobs = env.reset(), orc.reset()
    assert np.array_equal(obs.reshape(oobs.shape).cpu().numpy(), oobs), "reset obs"
    if sevens:
        assert kw["flatten"]
        lo = orc.local_obs()
        lo[:, :, 1:3] = 7.0
        orc.set_local_obs(lo)
        obs.data.view(N, P, -1)[:, :, R * R:3 * R * R] = 7.0   # .data: only invalidate_obs() tells the env
        env.invalidate_obs()
        never_inside = np.ones(orc.obs.shape, bool)
    rng = np.random.RandomState(5)
    tstep = np.zeros(N, np.int64)
    n_resets = np.zeros(N, np.int64)
    n_removed = 0
    for t in range(T):
        act = rng.randint(5, size=(N, P))
        obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
        oobs, orew, odone, orem = orc.step(act)
        tstep += 1
        bits = odone.astype(np.uint8) | ((tstep >= H).astype(np.uint8) << 1)
        assert np.array_equal(info["done_bits"].cpu().numpy(), bits), "step %d done bits" % t
        assert np.array_equal(info["removed"].cpu().numpy(), orem), "step %d removed" % t
        assert np.array_equal(rew.cpu().numpy(), orew.astype(np.float32)), "step %d rewards" % t
        if sevens:
            never_inside &= orc.obs == 7.0   # (the step's own pass, before a reset's second one)
        mask = (bits != 0).astype(np.uint8)
        if mask.any():
            orc.reset(mask=mask)
            tstep[mask != 0] = 0
            n_resets += mask
        if sevens:
            never_inside &= orc.obs == 7.0
        n_removed += int(orem.sum())
        got = obs.reshape(orc.obs.shape).cpu().numpy()
        assert np.array_equal(got, orc.obs), "step %d obs: %d cells differ" % (t, int((got != orc.obs).sum()))
        if sevens and t == 9:
            sevens_at_10 = int(never_inside.sum())
        if t % 50 == 0 or t == T - 1:
            _cmp_state(env, orc, "step %d" % t)
    assert n_removed > 0 and bool((n_resets >= T // H - 1).all())
    if sevens:
        # no observation value is 7.0 (a count of 70 at layer_norm 10): a cell that still reads 7.0 in the oracle was never inside the map
        # (compared above at every step; the run is not empty: such cells exist after step 10, some of them sharing a float4 with stored cells)
        assert bool((got[never_inside] == 7.0).all())
        assert sevens_at_10 > 0
    return env


@pytest.mark.parametrize("start", ["declared_zero", "sevens_nothing_known"])
@pytest.mark.parametrize("name", ["c2_8v30_r7", "5v9_r5", "tiny5_4v3_r3"])
def test_zm16_shapes_600_steps_vs_oracle(name, start):
    _run_against_oracle(name, 600, sevens=(start == "sevens_nothing_known"))


@pytest.mark.parametrize("name", ["13v51_r7", "c2_hwc"])
def test_dword_form_shapes_200_steps_vs_oracle(name):
    _run_against_oracle(name, 200, sevens=False)


def test_c2_forward_and_alternate_walk_agree():
    outs = []
    for walk in ("forward", "alternate"):
        env, _ = _pair("c2_8v30_r7")
        env.set_walk(walk)
        env.reset()
        g = torch.Generator(device="cpu").manual_seed(0)
        acc = []
        for t in range(90):
            a = torch.randint(0, 5, (N, 8), generator=g, dtype=torch.int32).to(DEV)
            o, r, d, info = env.step(a)
            acc.append((o.clone(), r.clone(), d.clone(), info["removed"].clone()))
        outs.append(acc)
    for t, ((o1, r1, d1, m1), (o2, r2, d2, m2)) in enumerate(zip(*outs)):
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(m1, m2), "step %d" % t


def test_c2_masks_use_the_first_half_of_their_region():
    """The mask region keeps 256 B per env; a shape with the 16-bit form uses its first N x 128 bytes.  After the library's own
    invalidate (0xFF over the whole region at the next launch) and 300 steps, bytes [N 128, N 256) still hold 0xFF -- a wrong stride, or a
    lane >= 32 storing, would have written there -- and the first half does not (masks at their equilibrium are mostly zero)."""
    import ctypes as C
    from madrl_amd import _lib
    env, _ = _pair("c2_8v30_r7")
    env.reset()
    env.invalidate_obs()
    foff = C.c_uint64()
    _lib.check(_lib.lib().madrl_pursuit_flags_offset(C.byref(env._config()), N, C.byref(foff)))
    region = env._state[foff.value - 256 * N:foff.value]
    assert foff.value - 256 * N == (env.record_bytes * N + 255) // 256 * 256
    g = torch.Generator(device="cpu").manual_seed(1)
    for t in range(300):
        env.step(torch.randint(0, 5, (N, 8), generator=g, dtype=torch.int32).to(DEV))
    torch.cuda.synchronize()
    region = region.cpu().numpy()
    assert bool((region[128 * N:] == 0xFF).all()), "%d bytes of the unused half were written" % int((region[128 * N:] != 0xFF).sum())
    first = region[:128 * N].reshape(N, 128)
    assert bool((first != 0xFF).any(axis=1).all()), "an env whose 128 mask bytes were never written"
