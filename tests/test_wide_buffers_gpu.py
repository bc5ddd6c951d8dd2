"""GPU tests (-m gpu): the env kernels and the epilogue kernels on buffers past 2^32 bytes, and past 2^31 elements.

One shared check (tests/wide.py, assert_big_equals_parts): a `big` handle whose buffer has at least 64 whole envs beyond the line, K `part`
handles of N / K envs (same seed, env_id_base advanced; every part buffer below 2^31 bytes) and a 48-env `probe` on big's last envs.
Compared bit for bit, on the device, after reset(), after every step (max_steps 3 with auto-reset, 8 steps) and after one reset(mask=)
on every third env: the whole observation buffer (stale cells included), rewards, done bytes, removed, the info tensors, every
get_state() key, the flag plane and the raw state buffer (records, stale-zero masks) -- big against its parts, big's tail against the
probe, and the probe against the C oracle.  Each case uses the compiled shape of its kernel with the longest rows, so the env count stays
small, and asserts the kernel it ran on.

A row base, an action or reward pointer or a mask offset narrowed to 32 bits computes the same as today on every other test of the suite;
here big's envs beyond the line would be written over its first envs (or fault): big differs from its parts in both places.

Behind the PursuitEvade cases: the Waterworld and hostage-world kernels (one wavefront, crowd) against their float32 oracles in the same
three comparisons; the fused StandardizedEnv step of both worlds with float64 statistics past 2^32 bytes; MultiWalker's ten-walker class
with a state buffer past 2^32 bytes against the CPU build; obsnorm / rewnorm / the frame stack against their parts; the device policies over
the big crowd and Waterworld observation buffers; madrl_rollout_gae on more than 2^31 bytes against its oracle.

A case skips only when the device has less free memory than it needs (below 20 GiB each)."""
import numpy as np
import pytest

import wide
from wide import PursuitCase

pytestmark = pytest.mark.gpu

HEAD, HEAD_HWC_SMALL = (16, 16, 8, 30, 7, 1), (6, 6, 3, 5, 11, 0)
LIMIT = (16, 16, 13, 51, 7, 1)        # 8 slots per lane, the one-wavefront limit: its longest rows
AUTHORS = (32, 32, 30, 50, 11, 1)     # XG / HG, four wavefronts per env
CNN48 = (48, 48, 100, 300, 21, 0)     # XC: the CNN shape's (R, R, 4) rows on a small map
GENERIC = ("generic", "generic", "generic")
LIVE_COUNTS = [(8, 30), (7, 29), (4, 26), (1, 1), (8, 1), (1, 30), (5, 12)]

IN_PLACE = {
    "wave_forward": PursuitCase("rect", LIMIT, walk="forward"),
    "wave_alternate": PursuitCase("rect", LIMIT, walk="alternate"),   # envs indexed n_envs - 1 - e on every other launch
    "fixed": PursuitCase("rect", HEAD, walk="forward", kinds=("wave", "wave", "fixed")),
    "group": PursuitCase("rect", AUTHORS),
    "crowd": PursuitCase("rect", CNN48),
    "generic": PursuitCase("rect", CNN48, kernel="generic", kinds=GENERIC),
    "live_counts": PursuitCase("rect", HEAD, counts=LIVE_COUNTS),
}
STEP_TO = {
    "wave": PursuitCase("rect", HEAD, mode="step_to"),
    "group": PursuitCase("rect", AUTHORS, mode="step_to"),
    "crowd": PursuitCase("rect", CNN48, mode="step_to"),
    "generic": PursuitCase("rect", CNN48, mode="step_to", kernel="generic", kinds=GENERIC),
}
HALF = {
    "wave": PursuitCase("open", HEAD_HWC_SMALL, mode="half"),   # window wider than the map: every row has kept cells
    "group": PursuitCase("rect", AUTHORS, mode="half"),
    "generic": PursuitCase("rect", CNN48, mode="half", kernel="generic", kinds=GENERIC),
}


@pytest.mark.parametrize("name", sorted(IN_PLACE))
def test_in_place_step_past_4_gib(name, monkeypatch):
    """the crowd case also runs PursuitHeuristicPolicy over the big (R, R, 4) observation buffer (wide.pursuit_policy_check)"""
    N, K, nbytes = wide.assert_big_equals_parts(IN_PLACE[name], monkeypatch, policy=(name == "crowd"))
    assert K == 3 and nbytes > 2**32


@pytest.mark.parametrize("name", sorted(STEP_TO))
def test_two_buffer_step_between_two_buffers_past_4_gib(name, monkeypatch):
    N, K, nbytes = wide.assert_big_equals_parts(STEP_TO[name], monkeypatch)
    assert K == 3 and nbytes > 2**32


@pytest.mark.parametrize("name", sorted(HALF))
def test_half_precision_step_past_4_gib_and_2_31_elements(name, monkeypatch):
    N, K, nbytes = wide.assert_big_equals_parts(HALF[name], monkeypatch, mask_reset_first=True)
    assert K == 3 and nbytes > 2**32 and nbytes // 2 > 2**31


@pytest.mark.parametrize("name", ["crowd", "generic"])
def test_float32_element_offsets_past_2_31(name, monkeypatch):
    """N * n_agents * obs_dim >= 2^31 + 64 rows: an element index (not only a byte offset) that does not fit a signed 32-bit register"""
    N, K, nbytes = wide.assert_big_equals_parts(IN_PLACE[name], monkeypatch, line_bytes=4 * 2**31, parts=5)
    assert K == 5 and nbytes // 4 > 2**31


# Waterworld and the hostage world: the one-wavefront kernels at their widest compiled rows, the crowd kernels with many agents and sensors
# and few other particles (long rows, so the env count stays small and a step cheap)
PARTICLE = {
    "waterworld_wave": wide.ParticleCase("waterworld", (5, 10), "wave", n_poison=10, n_sensors=30, radius=0.03, ev_speed=0.03, action_scale=0.03),
    "waterworld_crowd": wide.ParticleCase("waterworld", (40, 3), "crowd", n_poison=3, n_coop=2, n_sensors=200, sensor_range=0.5, radius=0.03, ev_speed=0.03, action_scale=0.03),
    "hostage_wave": wide.ParticleCase("hostage", (10, 10, 5, 2, 2), "wave", n_sensors=30, action_scale=0.03, bad_speed=0.03, radius=0.03),
    "hostage_crowd": wide.ParticleCase("hostage", (40, 3, 3, 2, 1), "crowd", n_sensors=200, sensor_range=0.5, action_scale=0.03, bad_speed=0.03, radius=0.03),
}


@pytest.mark.parametrize("name", sorted(PARTICLE))
def test_particle_world_step_past_4_gib(name):
    """the Waterworld one-wavefront case also runs WaterworldHeuristicPolicy over the big observation buffer (wide.waterworld_policy_check)"""
    N, K, nbytes = wide.assert_big_equals_parts_particle(PARTICLE[name], policy=(name == "waterworld_wave"))
    assert K == 3 and nbytes > 2**32


@pytest.mark.parametrize("name", ["waterworld_wave", "hostage_wave"])
def test_fused_standardized_step_with_statistics_past_4_gib(name):
    N, K = wide.assert_fused_std_big_equals_parts(PARTICLE[name])
    assert K == 3


@pytest.mark.parametrize("fused", [False, True], ids=["three_launches", "one_launch"])
def test_multiwalker_state_buffer_past_4_gib(fused):
    """The ten-walker capacity class with the env count chosen so that the STATE buffer passes 2^32 bytes: the per-env blocks (world record
    and step scratch) end just below 2^31, the spare records behind them cross it, and the spares' observations and lists cross 2^32.
    max_steps 5 with auto-reset through spares: every env takes its spare once.  big against K parts: observations, rewards, done bytes
    and every env's world record; big's last 48 envs against the probe; the probe against the CPU build of the same source, world
    records byte for byte."""
    import torch
    W, H, STEPS = 10, 5, 7
    one = wide.mw_make(64, W, fused, H, wide.ID_BASE)
    per_env, stride, world = -(-one._state.numel() // 64), one.record_stride, one.world_bytes
    del one
    N, K = wide.plan(per_env)
    per = N // K
    mk = lambda n, off: wide.mw_make(n, W, fused, H, wide.ID_BASE + off)
    wide.need_device_bytes(2 * N * per_env + 2**30)
    torch.cuda.reset_peak_memory_stats()
    big = mk(N, 0)
    assert big._state.numel() > 2**32 + (wide.BEYOND - 1) * per_env and N * stride < 2**31 < 2 * N * stride < 2**32, "where the lines fall"
    part = [mk(per, j * per) for j in range(K)]
    assert all(p._state.numel() < 2**31 for p in part)
    probe, orc = mk(wide.PROBE, N - wide.PROBE), wide.MwProbeOracle(wide.PROBE, W, H, wide.ID_BASE + N - wide.PROBE)

    def compare(what):
        for name, p, at in [("part %d" % j, p, j * per) for j, p in enumerate(part)] + [("the probe", probe, N - wide.PROBE)]:
            sl = slice(at, at + p.n_envs)
            assert wide.bits_equal(big._obs[sl], p._obs), "%s, %s: observations" % (what, name)
            assert wide.bits_equal(big._rew[sl], p._rew) and torch.equal(big._done[sl], p._done), "%s, %s: rewards / done bytes" % (what, name)
            same = (big.state_buffer[sl, :world] == p.state_buffer[:, :world]).all(dim=1)
            assert bool(same.all()), "%s, %s: %d world records differ" % (what, name, int((~same).sum()))

    for e in [big] + part + [probe]:
        e.reset()
    orc.reset(probe)
    compare("after reset")
    gen = torch.Generator(device=wide.DEV).manual_seed(7)
    for t in range(STEPS):
        act = torch.rand((N, W, 4), generator=gen, device=wide.DEV) * 2 - 1
        for e, at in [(big, 0)] + [(p, j * per) for j, p in enumerate(part)] + [(probe, N - wide.PROBE)]:
            e.step(act[at:at + e.n_envs])
        compare("step %d" % t)
        orc.step(probe, act[N - wide.PROBE:].cpu().numpy(), "step %d, the probe" % t)
    assert orc.resets >= wide.PROBE
    third = torch.arange(N, device=wide.DEV) % 3 == 0
    for e, at in [(big, 0)] + [(p, j * per) for j, p in enumerate(part)] + [(probe, N - wide.PROBE)]:
        e.reset(mask=third[at:at + e.n_envs])
    compare("after reset(mask=)")
    orc.reset(probe, "reset(mask=)", mask=third[N - wide.PROBE:].cpu().numpy().astype(np.uint8))
    used = torch.cuda.max_memory_allocated()
    assert used < 20 * 2**30
    print("N=%d K=%d state=%.3f GiB peak=%.2f GiB" % (N, K, big._state.numel() / 2.0**30, used / 2.0**30))
    del big, part, probe
    wide.free_device()


# ---------------------------------------------------------------------------------------------------------------- epilogue kernels
def _epilogue(kind, n_envs, E, x, state, calls, env0, big_n_envs):
    """`calls` calls of one epilogue kernel through the C ABI on envs [env0, env0 + n_envs) of the inputs; x: the input buffer of the WHOLE
    batch, refilled per call from a seeded generator (so every run sees the same values); state: the run's own tensors"""
    import torch
    from madrl_amd import _lib
    L, P, st = _lib.lib(), _lib.ptr, _lib.current_stream(torch.device(wide.DEV))
    n, lo = n_envs * E, env0 * E
    for t in range(calls):
        g = torch.Generator(device=wide.DEV).manual_seed(100 + t)
        x.normal_(generator=g)
        masks = torch.randint(0, 2, (2, big_n_envs), generator=g, device=wide.DEV, dtype=torch.uint8)
        xin = x[lo:lo + n]
        m = masks[0, env0:env0 + n_envs].contiguous() if (kind.endswith("masked") and t > 0) else None
        assert xin.data_ptr() % 16 == 0 and all(v.data_ptr() % 16 == 0 for v in state.values()), "the aligned kernels are the ones under test"
        if kind.startswith("obsnorm"):   # no mask, aligned: obsnorm_pairs_kernel; masked: obsnorm_kernel
            _lib.check(L.madrl_wrap_obsnorm(P(xin), P(state["mean"]), P(state["var"]), P(state["out"]), n, E, P(m), 0.05, 1e-8, st))
        elif kind.startswith("rewnorm"):
            _lib.check(L.madrl_wrap_rewnorm(P(xin), P(state["mean"]), P(state["var"]), P(state["out"]), n, E, P(m), 0.05, 1e-8, 0.7, 1, st))
        else:   # the frame stack: everything reset, a plain push, reset bytes under an active mask
            k = int(kind[-1])
            rm = None if t == 1 else (torch.ones(n_envs, dtype=torch.uint8, device=wide.DEV) if t == 0 else masks[0, env0:env0 + n_envs].contiguous())
            am = masks[1, env0:env0 + n_envs].contiguous() if t == 2 else None
            _lib.check(L.madrl_wrap_obsbuffer(P(xin), P(state["buf"]), n, E, k, P(rm), P(am), st))
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["obsnorm", "obsnorm_masked", "rewnorm", "rewnorm_masked", "obsbuffer_k4", "obsbuffer_k3"])
def test_epilogue_kernels_past_4_gib_equal_their_parts(kind):
    """obsnorm / rewnorm with float64 statistics past 2^32 bytes (their float32 rows past 2^31), the frame stack with a buffer past 2^32
    bytes: the whole batch in one call against the same calls on K parts of whole envs, every tensor bit for bit (the kernels are
    element-wise, so a part computes what the batch computes: the existing contract).  The parts run one after the other, which keeps the
    peak below 20 GiB."""
    import torch
    stack = kind.startswith("obsbuffer")
    E, k = (5 if kind.startswith("rewnorm") else 1028), (int(kind[-1]) if stack else 0)
    N, K = wide.plan(E * (4 * k if stack else 8))
    per, calls = N // K, 3
    sizes = dict(buf=(k, torch.float32)) if stack else dict(mean=(1, torch.float64), var=(1, torch.float64), out=(1, torch.float32))
    nbytes = lambda n_envs: sum(n_envs * E * m * torch.empty(0, dtype=dt).element_size() for m, dt in sizes.values())
    wide.need_device_bytes(nbytes(N) + nbytes(per) + 4 * N * E + 2**28)
    torch.cuda.reset_peak_memory_stats()

    def fresh(n_envs):
        st = {name: torch.zeros(n_envs * E * m, dtype=dt, device=wide.DEV) for name, (m, dt) in sizes.items()}
        if "var" in st:
            st["var"].fill_(1.0)
        if "out" in st:
            st["out"].fill_(float("nan"))
        return st

    x = torch.empty(N * E, dtype=torch.float32, device=wide.DEV)
    big = fresh(N)
    assert max(v.numel() * v.element_size() for v in big.values()) >= 2**32 + wide.BEYOND * E
    _epilogue(kind, N, E, x, big, calls, 0, N)
    for j in range(K):
        part = fresh(per)
        assert all(v.numel() * v.element_size() < 2**31 for v in part.values())
        _epilogue(kind, per, E, x, part, calls, j * per, N)
        for name, (m, _dt) in sizes.items():
            a = big[name][j * per * E * m:(j + 1) * per * E * m]
            assert wide.bits_equal(a, part[name]), "%s, part %d of %d: %s" % (kind, j, K, name)
        del part
        wide.free_device()
    assert not bool(torch.isnan(big["buf" if stack else "out"]).any()), "an element never written"
    used = torch.cuda.max_memory_allocated()
    assert used < 20 * 2**30
    print("%s N=%d K=%d largest=%.3f GiB peak=%.2f GiB" % (kind, N, K, max(v.numel() * v.element_size() for v in big.values()) / 2.0**30, used / 2.0**30))
    del big, x
    wide.free_device()


# ---------------------------------------------------------------------------------------------------------------- returns / GAE
def test_gae_on_more_than_2_31_bytes_against_the_oracle():
    """madrl_rollout_gae on T x N x A float32 of more than 2^31 bytes (the value tensor, T + 1 rows, passes it inside its last row): the
    last 4 096 columns and 4 096 columns around every power-of-two byte line from 2^28 up, of the reward / return layout and of the value
    layout, against oracle/rollout_oracle.py with the bound of tests/test_rollout.py, 1e-5 * max(1, |x|).  Columns are independent, so the
    oracle sees only the checked ones."""
    import torch
    from madrl_amd import _lib
    from oracle import rollout_oracle as ro
    T, A, W = 3, 8, 512                                   # W envs of A agents: 4 096 columns
    N = -(-(2**31 // (T * A * 4) + 2 * W) // 8) * 8
    cols = N * A
    assert T * cols * 4 > 2**31 + W * A * 4
    wide.need_device_bytes((4 * T + 1) * cols * 4 + 2**30)
    g = torch.Generator(device=wide.DEV).manual_seed(11)
    rew = torch.randn((T, N, A), generator=g, device=wide.DEV)
    val = torch.randn((T + 1, N, A), generator=g, device=wide.DEV)
    done = torch.tensor([0, 0, 0, 1, 2, 3, 0x80, 0x81], dtype=torch.uint8, device=wide.DEV)[torch.randint(0, 8, (T, N), generator=g, device=wide.DEV)]
    ret, adv = torch.full_like(rew, float("nan")), torch.full_like(rew, float("nan"))
    _lib.check(_lib.lib().madrl_rollout_gae(_lib.ptr(rew), _lib.ptr(done), _lib.ptr(val), T, N, A, 0.99, 0.95, _lib.ptr(ret), _lib.ptr(adv),
                                            _lib.current_stream(torch.device(wide.DEV))))
    assert not bool(torch.isnan(ret).any()) and not bool(torch.isnan(adv).any()), "a column never written"
    starts = {N - W}
    for rows in (T, T + 1):
        for e in range(28, 33):
            if 2**e < rows * cols * 4:
                env = ((2**e // 4) % cols) // A           # the env whose column holds the byte at the line
                starts.add(min(max(env - W // 2, 0), N - W))
    assert len(starts) >= 5
    for s in sorted(starts):
        sl = slice(s, s + W)
        r, d, v = rew[:, sl].cpu().numpy(), done[:, sl].cpu().numpy(), val[:, sl].cpu().numpy()
        ref_ret, ref_adv = ro.gae(r, d & 3, v, 0.99, 0.95)
        for name, got, want in (("returns", ret[:, sl].cpu().numpy(), ref_ret), ("advantages", adv[:, sl].cpu().numpy(), ref_adv)):
            err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            assert err.max() <= 1e-5, "%s, envs from %d: %r" % (name, s, err.max())
    del rew, val, ret, adv
    wide.free_device()
