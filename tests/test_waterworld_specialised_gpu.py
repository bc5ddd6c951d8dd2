"""GPU tests (-m gpu) of the specialised one-wavefront Waterworld kernels beyond the shapes anybody runs for speed: the nine test lines of
csrc/waterworld_specializations.def (waterworld_parity.SPEC_SHAPES says what each one reaches), waterworld_kernel<...> and its half twin
waterworld_kernel_f16<...>.

The definition of right is the float32 build of the C oracle, bit for bit: (a) the float32 env free-running against it, one workgroup per
env and three workgroups for 64 envs (each then walks 21 or 22 envs through the record prefetch), with (b) a reset(mask=) of every third
env half way; (c) the FUSED instantiations against a second env and the stand-alone epilogue kernels; (d) the half rows against a float32
twin.  Every env says after every launch that the launch ran a specialised instantiation (last_launch_kernel), so that none of this can
pass on the generic kernel; and every run has to have caught evaders and poison and ended an episode per env, counted on the oracle."""
import numpy as np
import pytest
import torch

from waterworld_parity import DEV, MASK_RESET_AT, RUN, SPEC_SHAPES, exercised, mk, oracle_run, vs_f32_oracle

pytestmark = pytest.mark.gpu
NAMES = sorted(SPEC_SHAPES)
F16, F32 = torch.float16, torch.float32
NAN16 = 0x7E5A   # a quiet NaN no row holds: what a half buffer, a slot and its guards are filled with
SCALE, ALPHA, EPS = 0.7, 0.05, 1e-8
SEEDS = dict(seed=77, env_id_base=500, max_steps=RUN["H"], auto_reset=True)   # what vs_f32_oracle and oracle_run give both sides


def _specialised(env, where):
    assert env.last_launch_kernel == "specialised", "%s ran on the %s kernel" % (where, env.last_launch_kernel)


def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("max_blocks", [0, 3])
@pytest.mark.parametrize("name", NAMES)
def test_specialised_float32_matches_the_oracle_bit_for_bit(name, max_blocks):
    """(a), (b): free-running, nothing copied across; observations, rewards, done, both counters and the whole state in every bit"""
    line, kw = SPEC_SHAPES[name]
    launches = []

    def each(env, where):
        assert env.obs_dim == line[4] and env.kernel_kind == "wave"
        _specialised(env, where)
        launches.append(where)

    totals = vs_f32_oracle(kw, False, env_kw=dict(max_blocks=max_blocks), mask_reset_at=MASK_RESET_AT, bits=True, each_launch=each, **RUN)
    assert len(launches) == RUN["T"] + 2                      # the reset, the masked reset and every step
    assert totals == oracle_run(name, MASK_RESET_AT)[1:]      # the shared run is this run
    exercised(*totals, what=name)


@pytest.mark.parametrize("name", NAMES)
def test_specialised_fused_standardize_equals_step_and_epilogue_kernels(name):
    """(c): the FUSED = true instantiations against a second env of the shape and madrl_wrap_obsnorm / madrl_wrap_rewnorm: outputs and all
    four statistics tensors equal in every bit"""
    from madrl_amd import _lib
    L = _lib.lib()
    line, kw = SPEC_SHAPES[name]
    acts, ev, po, ends = oracle_run(name)
    n, A, D = RUN["N"], line[0], line[4]
    fused, plain = mk(n, **SEEDS, **kw), mk(n, **SEEDS, **kw)
    st = fused.bind_standardize(scale_reward=SCALE, enable_obsnorm=True, enable_rewnorm=True, obs_alpha=ALPHA, rew_alpha=ALPHA, eps=EPS)
    assert plain.obs_dim == D
    f64 = dict(dtype=torch.float64, device=DEV)
    om, ov, oo = torch.zeros((n, A, D), **f64), torch.ones((n, A, D), **f64), torch.zeros((n, A, D), device=DEV)
    rm, rv, ro = torch.zeros((n, A), **f64), torch.ones((n, A), **f64), torch.zeros((n, A), device=DEV)
    stream = _lib.current_stream(torch.device(DEV))

    def obsnorm(obs):
        _lib.check(L.madrl_wrap_obsnorm(_lib.ptr(obs), _lib.ptr(om), _lib.ptr(ov), _lib.ptr(oo), obs.numel(), obs.numel() // n, None, ALPHA, EPS,
                                        stream))
        return oo

    def rewnorm(rew):
        _lib.check(L.madrl_wrap_rewnorm(_lib.ptr(rew), _lib.ptr(rm), _lib.ptr(rv), _lib.ptr(ro), rew.numel(), rew.numel() // n, None, ALPHA, EPS,
                                        SCALE, 1, stream))
        return ro

    same = lambda a, b: torch.equal(_bits(a), _bits(b))
    assert same(fused.reset(), obsnorm(plain.reset())), "reset"
    _specialised(fused, "the fused reset"); _specialised(plain, "the plain reset")
    got = np.zeros(3, np.int64)
    for t in range(RUN["T"]):
        act = torch.from_numpy(np.array(acts[t])).to(DEV)      # (a writable copy: the shared run stays read-only)
        of, rf, df, inf = fused.step(act)
        op, rp, dp, inp = plain.step(act)
        _specialised(fused, "fused step %d" % t); _specialised(plain, "plain step %d" % t)
        assert same(of, obsnorm(op)) and same(rf, rewnorm(rp)) and torch.equal(df, dp), "step %d" % t
        assert sorted(inf) == sorted(inp) and all(torch.equal(inf[k], inp[k]) for k in inf), "step %d" % t
        got += (int(inp["evcatches"].sum()), int(inp["pocatches"].sum()), int(dp.sum()))
    for k, v in dict(obs_mean=om, obs_var=ov, rew_mean=rm, rew_var=rv).items():
        assert same(st[k], v), k
    assert tuple(got) == (ev, po, ends)          # the oracle's run is this run
    exercised(ev, po, ends, what=name)


def _half_bits(t):
    """the 16-bit patterns a half row holds where the float32 twin holds t: round to nearest even, subnormals kept"""
    return (t.to(F16) if t.dtype is F32 else t).contiguous().view(torch.int16).reshape(-1)


@pytest.mark.parametrize("name", NAMES)
def test_specialised_half_rows_are_the_float32_rows_rounded(name):
    """(d): obs_dtype=torch.float16 against a float32 twin -- reset(), 20 steps into the env's own buffer, reset(mask=) of every third env,
    20 steps through step(obs_out=) into a slot that starts one element past a 4-byte boundary, between guard bands"""
    line, kw = SPEC_SHAPES[name]
    acts, ev, po, ends = oracle_run(name, MASK_RESET_AT)
    n = RUN["N"]
    F, H = mk(n, max_blocks=3, **SEEDS, **kw), mk(n, max_blocks=3, obs_dtype=F16, **SEEDS, **kw)
    assert H.obs_dim == F.obs_dim == line[4] and H._obs.dtype is F16 and F._obs.dtype is F32
    H._obs.view(torch.int16).fill_(NAN16)    # whatever a launch leaves unwritten stays a NaN

    def rows(h, f, what):
        assert h.dtype is F16 and f.dtype is F32 and h.shape == f.shape, what
        diff = int((_half_bits(h) != _half_bits(f)).sum())
        assert diff == 0, "%s: %d of %d elements differ from the float32 twin's halves" % (what, diff, f.numel())

    def state(what):
        sf, sh = F.get_state(), H.get_state()
        assert sf.keys() == sh.keys()
        for k in sf:
            assert torch.equal(_bits(sf[k]), _bits(sh[k])), (what, k)
        _specialised(H, what); _specialised(F, what)

    rows(H.reset(), F.reset(), "reset"); state("reset")
    numel, guard = F._obs.numel(), 64
    ring = torch.full((guard + 1 + numel + guard,), NAN16, dtype=torch.int16, device=DEV)
    at = guard + 1 if ring.data_ptr() % 4 == 0 else guard      # (torch allocates on far more than 4 bytes: the first)
    slot, want = ring[at:at + numel].view(F16), ring.clone()
    assert slot.data_ptr() % 4 == 2 and slot.is_contiguous()
    got = np.zeros(3, np.int64)
    for t in range(RUN["T"]):
        if t == MASK_RESET_AT:
            mask = np.arange(n) % 3 == 0
            rows(H.reset(mask=mask), F.reset(mask=mask), "reset(mask=)"); state("reset(mask=)")   # the other envs' rows keep their 16 bits
        act = torch.from_numpy(np.array(acts[t])).to(DEV)      # (a writable copy: the shared run stays read-only)
        of, rf, df, inf = F.step(act)
        if t < MASK_RESET_AT:
            oh, rh, dh, inh = H.step(act)
            assert oh.data_ptr() == H._obs.data_ptr()
        else:
            oh, rh, dh, inh = H.step(act, obs_out=slot)
            assert oh.data_ptr() == slot.data_ptr() and oh.shape == F._obs.shape
            want[at:at + numel] = _half_bits(of)
            bad = (ring != want).nonzero().reshape(-1)
            assert bad.numel() == 0, "step %d: %d elements of the ring are wrong, the first at %d (the slot is %d .. %d)" % (
                t, bad.numel(), int(bad[0]), at, at + numel - 1)
        rows(oh, of, "step %d" % t)
        assert rh.dtype is F32 and torch.equal(rh.view(torch.int32), rf.view(torch.int32)), t
        assert torch.equal(_bits(dh), _bits(df)), t
        assert inf.keys() == inh.keys() and all(torch.equal(inf[k], inh[k]) for k in inf), t
        state("step %d" % t)
        got += (int(inf["evcatches"].sum()), int(inf["pocatches"].sum()), int(df.sum()))
    assert tuple(got) == (ev, po, ends)          # the oracle's run is this run
    exercised(ev, po, ends, what=name)


def test_last_launch_kernel_names_every_family():
    """the observability the tests above stand on: "none" before a handle's first launch, then the family of the last reset / step"""
    fast = dict(n_coop=1, n_sensors=4, radius=0.03)
    act = lambda env: torch.zeros((env.n_envs, env.n_pursuers, 2), device=DEV)
    for kw, want in ((dict(n_pursuers=3, n_evaders=4, n_poison=4, **fast), "generic"),
                     (dict(n_pursuers=3, n_evaders=4, n_poison=4, obs_dtype=F16, **fast), "generic"),
                     (dict(n_pursuers=5, n_evaders=10), "specialised"),
                     (dict(n_pursuers=5, n_evaders=10, obs_dtype=F16), "specialised"),
                     (dict(n_pursuers=5, n_evaders=10, per_env_counts="wave"), "live"),
                     (dict(n_pursuers=5, n_evaders=10, sensor_range=np.array([0.2, 0.1, 0.3, 0.2, 0.25])), "ranged"),
                     (dict(n_pursuers=5, n_evaders=10, crowd=True), "crowd")):
        env = mk(4, seed=1, **kw)
        assert env.last_launch_kernel == "none", kw
        env.reset()
        assert env.last_launch_kernel == want, kw
        env.step(act(env))
        assert env.last_launch_kernel == want, kw
        env.seed(2)                                # a new handle
        assert env.last_launch_kernel == "none", kw
