"""GPU test (-m gpu): a partial reset under StandardizedEnv's epilogue path.  reset(mask=...) hands the mask to madrl_wrap_obsnorm: the envs
outside it keep their running statistics and their standardised rows -- what the fused Waterworld kernels have always done under a mask.
(Before, the epilogue path pushed the unchanged rows of the other envs through the statistics a second time.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_waterworld_partial_reset_epilogue_equals_fused_and_leaves_the_other_envs_alone():
    from madrl_amd.waterworld import BatchedMAWaterWorld
    from madrl_amd.wrappers import StandardizedEnv
    N = 96
    mk = lambda: BatchedMAWaterWorld(5, 10, n_envs=N, device=DEV, seed=9, max_steps=12, auto_reset=True)
    cfg = dict(scale_reward=0.7, enable_obsnorm=True, enable_rewnorm=True, obs_alpha=0.05, rew_alpha=0.05)
    fused, plain = StandardizedEnv(mk(), **cfg), StandardizedEnv(mk(), fused=False, **cfg)
    assert fused._fused and not plain._fused
    fused.reset(); plain.reset()
    g = torch.Generator(device="cpu").manual_seed(2)
    acts = (torch.rand((6, N, 5, 2), generator=g) * 2 - 1).to(DEV)
    for t in range(4):
        fused.step(acts[t])
        op, _, _, _ = plain.step(acts[t])
    mask = torch.arange(N, device=DEV) % 3 == 1
    keep = ~mask
    names = ("obs_mean", "obs_var", "rew_mean", "rew_var")
    before = {k: getattr(plain, "_" + k).clone() for k in names}
    rows = op.clone()
    of, op = fused.reset(mask=mask), plain.reset(mask=mask)
    assert torch.equal(of, op), "reset(mask): epilogue kernels != fused"
    for k in names:
        assert torch.equal(getattr(plain, "_" + k), fused._fused_state[k]), k
        assert torch.equal(getattr(plain, "_" + k)[keep], before[k][keep]), k
    assert torch.equal(op[keep], rows[keep])
    assert not torch.equal(op[mask], rows[mask]) and not torch.equal(plain._obs_mean[mask], before["obs_mean"][mask])
    for t in range(4, 6):
        of, rf, df, _ = fused.step(acts[t])
        op, rp, dp, _ = plain.step(acts[t])
        assert torch.equal(of, op) and torch.equal(rf, rp) and torch.equal(df, dp), t


def test_first_call_with_a_mask_returns_zero_rows_for_the_other_envs():
    """the wrapper's output buffer starts zero-filled, so a first reset that is partial returns defined rows for the envs outside the mask"""
    from madrl_amd.maps import rectangle_map
    from madrl_amd.pursuit import BatchedPursuitEvade
    from madrl_amd.wrappers import StandardizedEnv
    N = 32
    env = BatchedPursuitEvade([rectangle_map(16, 16)], n_envs=N, device=DEV, seed=3, n_pursuers=8, n_evaders=30, obs_range=7)
    env.reset()
    w = StandardizedEnv(env, enable_obsnorm=True)
    assert not w._fused
    mask = torch.arange(N, device=DEV) % 2 == 0
    obs = w.reset(mask=mask)
    assert float(obs[~mask].abs().sum()) == 0.0 and float(obs[mask].abs().sum()) > 0.0
    assert float(w._obs_mean[~mask].abs().sum()) == 0.0 and torch.equal(w._obs_var[~mask], torch.ones_like(w._obs_var[~mask]))
