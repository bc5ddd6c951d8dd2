"""GPU tests (-m gpu): StandardizedEnv fused into the hostage-world step / reset kernels (madrl_hostage_set_standardize,
hostage_kernel<..., FUSED>).  The fused form must equal the stand-alone epilogue kernels (madrl_wrap_obsnorm / madrl_wrap_rewnorm) over
an identical env bit for bit, and both stay within 1e-5 of the NumPy restatement of the reference wrapper (oracle/wrappers_oracle.py).
The fused twin is asked for with fused=True, so that every configuration runs the fused kernels: StandardizedEnv's own choice over a hostage
world fuses with enable_obsnorm only -- measured at 32 768 envs, 121.5 us fused against 129.4-130.1 with obsnorm + rewnorm, but 40.1-40.4
against 32.8-33.2 without normalisation (test_automatic_choice_follows_the_measurement)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ALPHA = dict(obs_alpha=0.05, rew_alpha=0.05)
# (enable_obsnorm, enable_rewnorm, scale_reward); the last one is the authors' own StandardizedEnv(env)
MODES = [(True, True, 0.7), (True, False, 1.0), (False, False, 1.0)]
MODE_IDS = ["obsnorm_rewnorm", "obsnorm", "authors_default"]

SPECIALISED = dict(args=(3, 10, 5, 2, 2), kw={}, n_envs=256)                       # hostage_kernel<.., 3, 10, 5, 30, 156>: 468 row elements
# generic instantiation; 2 x 65 = 130 row elements: no multiple of 4, one partial batch of four per lane
ODD_ROW = dict(args=(2, 3, 2, 1, 1), kw=dict(n_sensors=12, addid=False, reward_mech="local"), n_envs=67)
# generic instantiation; 5 x 61 = 305 row elements: one full batch of 256 and a partial one of 49
LONG_ROW = dict(args=(5, 3, 2, 1, 1), kw=dict(n_sensors=11, reward_mech="local"), n_envs=67)


def _mk(shape, **over):
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    kw = dict(n_envs=shape["n_envs"], device=DEV, seed=9, max_steps=12, auto_reset=True)
    kw.update(shape["kw"])
    kw.update(over)
    return BatchedContinuousHostageWorld(*shape["args"], **kw)


def _cfg(mode):
    on, rn, scale = mode
    return dict(scale_reward=scale, enable_obsnorm=on, enable_rewnorm=rn, **ALPHA)


def _actions(shape, steps, seed=2):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand((steps, shape["n_envs"], shape["args"][0], 2), generator=g) * 2 - 1).to(DEV)


def _compare_with_epilogue_and_oracle(shape, mode, steps=30):
    from madrl_amd.wrappers import StandardizedEnv
    from oracle import wrappers_oracle as wo
    cfg = _cfg(mode)
    fused, plain, raw = StandardizedEnv(_mk(shape), fused=True, **cfg), StandardizedEnv(_mk(shape), fused=False, **cfg), _mk(shape)
    assert fused._fused and not plain._fused
    N, Nr, D = shape["n_envs"], shape["args"][0], raw.obs_dim
    so = wo.StdOracle((N, Nr, D), (N, Nr), **cfg)
    of, op = fused.reset(), plain.reset()
    ref = so.obs(raw.reset().cpu().numpy())
    assert torch.equal(of, op), "reset: fused != epilogue kernels"
    assert np.abs(of.cpu().numpy() - ref).max() < 1e-5
    acts = _actions(shape, steps)
    n_done = 0
    for t in range(steps):
        of, rf, df, _ = fused.step(acts[t])
        op, rp, dp, _ = plain.step(acts[t])
        ro, rr, rd, _ = raw.step(acts[t])
        assert torch.equal(of, op) and torch.equal(rf, rp) and torch.equal(df, dp), "step %d: fused != epilogue kernels" % t
        assert torch.equal(df, rd), t
        assert np.abs(of.cpu().numpy() - so.obs(ro.cpu().numpy())).max() < 1e-5, t
        want = so.rew(rr.cpu().numpy())
        assert np.abs(rf.cpu().numpy() - want).max() < 1e-5 * max(1.0, np.abs(want).max()), t
        assert np.abs(rp.cpu().numpy() - want).max() < 1e-5 * max(1.0, np.abs(want).max()), t
        n_done += int(df.sum())
    assert n_done >= 2 * N   # max_steps = 12: every env went through two fused resets
    if mode[0]:
        assert torch.equal(fused._obs_mean, plain._obs_mean) and torch.equal(fused._obs_var, plain._obs_var)
        assert np.abs(fused._obs_mean.cpu().numpy() - so.om).max() < 1e-5
    if mode[1]:
        assert torch.equal(fused._rew_mean, plain._rew_mean) and torch.equal(fused._rew_var, plain._rew_var)
    if not mode[0]:   # no observation normalisation: the wrapper's rows are the raw rows
        assert torch.equal(of, ro)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_fused_equals_epilogue_equals_oracle_specialised_shape(mode):
    _compare_with_epilogue_and_oracle(SPECIALISED, mode)


@pytest.mark.parametrize("shape", [ODD_ROW, LONG_ROW], ids=["row_130", "row_305"])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_generic_instantiation_and_its_tails(shape, mode):
    _compare_with_epilogue_and_oracle(shape, mode)


@pytest.mark.parametrize("shape", [SPECIALISED, ODD_ROW], ids=["specialised", "generic"])
def test_partial_reset_leaves_the_other_envs_alone(shape):
    from madrl_amd.wrappers import StandardizedEnv
    cfg = _cfg(MODES[0])
    fused, plain = StandardizedEnv(_mk(shape), fused=True, **cfg), StandardizedEnv(_mk(shape), fused=False, **cfg)
    fused.reset(); plain.reset()
    acts = _actions(shape, 6)
    for t in range(4):
        of, _, _, _ = fused.step(acts[t])
        plain.step(acts[t])
    N = shape["n_envs"]
    mask = (torch.arange(N, device=DEV) % 3 == 1)
    keep = ~mask
    names = ("obs_mean", "obs_var", "rew_mean", "rew_var")
    before = {k: fused._fused_state[k].clone() for k in names}
    rows = of.clone()
    of, op = fused.reset(mask=mask), plain.reset(mask=mask)
    assert torch.equal(of, op), "reset(mask): fused != epilogue kernels"
    for k in names:
        assert torch.equal(fused._fused_state[k], getattr(plain, "_" + k)), k
        assert torch.equal(fused._fused_state[k][keep], before[k][keep]), k
    assert torch.equal(of[keep], rows[keep])
    assert not torch.equal(of[mask], rows[mask]) and not torch.equal(fused._obs_mean[mask], before["obs_mean"][mask])
    assert torch.equal(fused._rew_mean, before["rew_mean"])   # a reset produces no reward
    for t in range(4, 6):   # and the two keep agreeing afterwards
        of, rf, df, _ = fused.step(acts[t])
        op, rp, dp, _ = plain.step(acts[t])
        assert torch.equal(of, op) and torch.equal(rf, rp) and torch.equal(df, dp), t


def test_binding_survives_seed():
    from madrl_amd.wrappers import StandardizedEnv
    shape = dict(SPECIALISED, n_envs=96)
    cfg = dict(scale_reward=0.1, enable_obsnorm=True, enable_rewnorm=True, **ALPHA)
    fused, plain = StandardizedEnv(_mk(shape, seed=3), fused=True, **cfg), StandardizedEnv(_mk(shape, seed=3), fused=False, **cfg)
    assert fused._fused and not plain._fused
    acts = _actions(shape, 6)
    fused.reset(); plain.reset()
    for t in range(3):
        fused.step(acts[t]); plain.step(acts[t])
    st = fused._fused_state
    ptrs = {k: v.data_ptr() for k, v in st.items()}
    mean = st["obs_mean"].clone()
    assert float(mean.abs().sum()) > 0
    for env in (fused, plain):
        assert env.seed(11) == [11]
    assert fused._fused_state is st and fused.unwrapped._std is st and {k: v.data_ptr() for k, v in st.items()} == ptrs
    assert torch.equal(st["obs_mean"], mean), "seed() keeps the running statistics"
    a, b = fused.reset(), plain.reset()
    assert torch.equal(a, b), "after seed() the fused wrapper must still return standardised observations"
    for t in range(3, 6):
        o1, r1, d1, _ = fused.step(acts[t])
        o2, r2, d2, _ = plain.step(acts[t])
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), t
    assert torch.equal(fused._obs_mean, plain._obs_mean) and torch.equal(fused._rew_var, plain._rew_var)
    assert not torch.equal(r1, fused.unwrapped._rew), "rewards are scaled and normalised in the wrapper output"


def test_unbind_obs_out_and_step_on_stream():
    shape = dict(SPECIALISED, n_envs=64)
    env, twin, never = _mk(shape), _mk(shape), _mk(shape)
    cfg = _cfg(MODES[0])
    st, st2 = env.bind_standardize(**cfg), twin.bind_standardize(**cfg)
    assert env.fused_standardize and env._std is st
    acts = _actions(shape, 4)
    assert env.reset() is st["obs_out"]
    twin.reset(); never.reset()
    with pytest.raises(ValueError, match="obs_out"):
        env.step(acts[0], obs_out=torch.empty_like(st["obs_out"]))
    # step_on_stream on a bound env: the wrapper's tensors, the values of step()
    o1, r1, d1, _ = env.step(acts[0])
    out = twin.step_on_stream(acts[0], torch.cuda.current_stream(torch.device(DEV)))
    assert out is not None
    o2, r2, d2, _ = out
    assert o1 is st["obs_out"] and r1 is st["rew_out"] and o2 is st2["obs_out"] and r2 is st2["rew_out"]
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    never.step(acts[0])
    assert not torch.equal(o1, never._obs)
    # unbound: raw observations and rewards again, those of an env that never had a binding
    env.unbind_standardize()
    assert env._std is None
    frozen = st["obs_mean"].clone()
    for t in range(1, 4):
        o, r, d, _ = env.step(acts[t])
        on, rn, dn, _ = never.step(acts[t])
        assert o is env._obs and torch.equal(o, on) and torch.equal(r, rn) and torch.equal(d, dn), t
    assert torch.equal(env.reset(), never.reset())
    assert torch.equal(st["obs_mean"], frozen), "an unbound env leaves the statistics alone"


def test_crowd_env_takes_the_epilogue_kernels():
    from madrl_amd import _lib
    from madrl_amd.hostage import BatchedContinuousHostageWorld
    from madrl_amd.wrappers import StandardizedEnv
    mk = lambda: BatchedContinuousHostageWorld(20, 30, 40, 2, 1, crowd=True, n_envs=8, device=DEV, seed=5, max_steps=6, auto_reset=True)
    env = mk()
    assert not env.fused_standardize
    with pytest.raises(_lib.MadrlError, match="crowd"):
        env.bind_standardize(enable_obsnorm=True)
    cfg = dict(enable_obsnorm=True, enable_rewnorm=True)
    auto, plain = StandardizedEnv(env, **cfg), StandardizedEnv(mk(), fused=False, **cfg)
    assert not auto._fused and auto.unwrapped._std is None
    with pytest.raises(ValueError, match="fused=True"):
        StandardizedEnv(mk(), fused=True, **cfg)
    assert torch.equal(auto.reset(), plain.reset())
    g = torch.Generator(device="cpu").manual_seed(2)
    for t in range(8):
        a = (torch.rand((8, 20, 2), generator=g) * 2 - 1).to(DEV)
        oa, ra, da, _ = auto.step(a)
        op, rp, dp, _ = plain.step(a)
        assert torch.equal(oa, op) and torch.equal(ra, rp) and torch.equal(da, dp), t
    assert torch.isfinite(oa).all() and not torch.equal(oa, auto.unwrapped._obs)   # standardised, not the raw rows


def test_rollout_collector_over_fused_and_epilogue_wrappers():
    from madrl_amd.rollout import RolloutCollector
    from madrl_amd.wrappers import StandardizedEnv
    shape, T = dict(SPECIALISED, n_envs=64), 8
    cfg = _cfg(MODES[0])
    acts = _actions(shape, 2 * T, seed=4)

    def policy():
        calls = [0]

        def act(obs):
            calls[0] += 1
            return acts[calls[0] - 1]
        return act
    fused, plain = StandardizedEnv(_mk(shape, max_steps=5), fused=True, **cfg), StandardizedEnv(_mk(shape, max_steps=5), fused=False, **cfg)
    assert fused._fused and not plain._fused
    cf, cp = RolloutCollector(fused, policy(), T, store_observations=True), RolloutCollector(plain, policy(), T, store_observations=True)
    assert not cf._slots and not cp._slots
    for it in range(2):
        tf, tp = cf.collect(), cp.collect()
        assert torch.equal(tf.rewards, tp.rewards) and torch.equal(tf.dones, tp.dones) and torch.equal(tf.returns, tp.returns), it
        assert torch.equal(tf.observations, tp.observations), it
    assert int((tf.dones != 0).sum()) >= 64   # max_steps = 5: episodes ended and restarted inside the horizon


def test_automatic_choice_follows_the_measurement():
    from madrl_amd.wrappers import StandardizedEnv
    shape = dict(SPECIALISED, n_envs=16)
    env = _mk(shape)
    assert env.fused_standardize and env.fused_standardize_pays(enable_obsnorm=True) and not env.fused_standardize_pays()
    # with observation normalisation the fused kernels are the faster form: taken by itself
    auto, plain = StandardizedEnv(env, enable_obsnorm=True, enable_rewnorm=True), StandardizedEnv(_mk(shape), fused=False, enable_obsnorm=True, enable_rewnorm=True)
    assert auto._fused and env._std is auto._fused_state
    assert torch.equal(auto.reset(), plain.reset())
    # the authors' own StandardizedEnv(env): the epilogue path by itself, the fused kernels on request, the same rows
    env2 = _mk(shape)
    default, asked = StandardizedEnv(env2), StandardizedEnv(_mk(shape), fused=True)
    assert not default._fused and env2._std is None
    assert asked._fused and asked.unwrapped._std is asked._fused_state
    assert torch.equal(default.reset(), asked.reset())
