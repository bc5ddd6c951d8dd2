"""The Pursuit fast kernels' start-up (pursuit_wave.hpp "table staging", pursuit_group.hpp): every workgroup stages its tables, the
slot constants and its first env's record in batches of unconditional loads from CLAMPED indices, and a change of map inside the env
loop (load_map) does the same.  Bit-exact against the CPU oracle, free-running with fused auto-resets, on the smallest compiled shapes
that reach each path:

  * X(5,5,4,3,3,1)       the padded layer has 52 dwords < 64 lanes: the only trip of every table is the clamped tail
  * X(16,16,8,30,7,1)    the headline shape: 7 full trips and a 36-lane tail per layer
  * X(13,14,3,27,7,0)    three maps, sample_maps: load_map to a map other than the staged map 0, maps changing at resets
  * XG(16,16,20,50,5,1,2) on the 16 x 16 map pool with sample_maps, and XG(32,32,16,60,7,1,2) (two batches of loads)

each at n_envs = 1 with the default grid (every other workgroup stages its tables, fetches an env that is not its own and must store
nothing), n_envs = 3 on 2 workgroups and n_envs = 130 on 64.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, T = 5, 13

SHAPES = {
    "X_5x5_4v3": ("golden:pursuit_tiny5_dense", None),
    "X_16x16_8v30": ("rect16", dict(n_pursuers=8, n_evaders=30, obs_range=7, n_catch=2, surround=True, flatten=True, reward_mech="local")),
    "X_13x14_3v27_three_maps": ("golden:pursuit_fuzz_20", dict(sample_maps=True)),
    "XG_16x16_20v50_pool": ("pool16", dict(n_pursuers=20, n_evaders=50, obs_range=5, n_catch=2, surround=True, flatten=True,
                                           reward_mech="local", sample_maps=True)),
    "XG_32x32_16v60": ("rect32", dict(n_pursuers=16, n_evaders=60, obs_range=7, n_catch=2, surround=True, flatten=True, reward_mech="local")),
}
LAUNCHES = {"one_env_default_grid": (1, 0), "three_envs_two_blocks": (3, 2), "130_envs_64_blocks": (130, 64)}


def _config(shape):
    from conftest import GOLDEN
    from madrl_amd.maps import rectangle_map
    from oracle import pursuit as po
    src, kw = SHAPES[shape]
    if src.startswith("golden:"):
        g = np.load(os.path.join(GOLDEN, src[7:] + ".npz"))
        cfg = po.config_from_golden(g)
        cfg.update(kw or {})
        return list(g["maps"]), cfg
    if src == "pool16":
        return list(np.load(os.path.join(GOLDEN, "pursuit_pool16_sample_maps.npz"))["maps"]), dict(kw)
    side = int(src[4:])
    return [rectangle_map(side, side)], dict(kw)


@pytest.mark.parametrize("launch", sorted(LAUNCHES), ids=sorted(LAUNCHES))
@pytest.mark.parametrize("shape", sorted(SHAPES), ids=sorted(SHAPES))
def test_startup_paths_bit_exact(shape, launch):
    from madrl_amd.pursuit import BatchedPursuitEvade
    from oracle import pursuit as po
    maps, kw = _config(shape)
    N, max_blocks = LAUNCHES[launch]
    P = kw["n_pursuers"]
    env = BatchedPursuitEvade(maps, n_envs=N, device=DEV, seed=41, env_id_base=5, max_steps=H, auto_reset=True, max_blocks=max_blocks, **kw)
    assert env.kernel_kind == "wave"
    orc = po.PursuitOracle(maps, n_envs=N, seed=41, env_id_base=5, **kw)
    obs = env.reset()
    assert np.array_equal(obs.cpu().numpy().reshape(orc.obs.shape), orc.reset()), "reset observations"
    tstep = np.zeros(N, np.int64)
    rng = np.random.RandomState(23)
    maps_seen = set()
    for t in range(T):
        act = rng.randint(5, size=(N, P)).astype(np.int32)
        obs, rew, done, info = env.step(torch.as_tensor(act, device=DEV))
        oobs, orew, odone, orem = orc.step(act)
        tstep += 1
        bits = odone.astype(np.uint8) | ((tstep >= H).astype(np.uint8) << 1)
        assert np.array_equal(info["done_bits"].cpu().numpy(), bits), "step %d done bits" % t
        assert np.array_equal(info["removed"].cpu().numpy(), orem), "step %d removed" % t
        assert np.array_equal(rew.cpu().numpy(), orew.astype(np.float32)), "step %d rewards" % t
        mask = (bits != 0).astype(np.uint8)
        if mask.any():
            orc.reset(mask=mask)
            tstep[mask != 0] = 0
        got = obs.cpu().numpy().reshape(orc.obs.shape)
        assert np.array_equal(got, orc.obs), "step %d: %d observation cells differ" % (t, int((got != orc.obs).sum()))
        maps_seen.update(int(m) for m in orc.get_state()["map_id"])
    gst, ost = env.get_state(), orc.get_state()
    for k in ("pos_p", "pos_e", "gone", "term_p", "term_e", "map_id"):
        assert np.array_equal(gst[k].cpu().numpy(), ost[k]), "final state[%s]" % k
    assert np.array_equal(gst["tick"].cpu().numpy().view(np.uint32), ost["tick"])
    assert np.array_equal(gst["t"].cpu().numpy(), tstep)
    if kw.get("sample_maps") and N > 1:
        assert maps_seen - {0}, "no env ever ran on a map other than the staged map 0"
