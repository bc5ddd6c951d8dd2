"""What the three Pursuit per-env-counts files (test_live_counts_gpu.py, test_live_counts_group_gpu.py, test_live_counts_crowd_gpu.py)
run in common: an env at live counts (p, e) of a capacity against a fixed-shape (p, e) batch, and the history of pending counts that the
live kernel and the generic kernel must agree on.  Each file calls these with its own capacities, batch sizes, seeds and run lengths."""
import numpy as np
import torch

DEV = "cuda:0"


def pursuit_state_equal(cap, fix, p, e):
    a, b = cap.get_state(), fix.get_state()
    assert torch.equal(a["pos_p"][:, :p], b["pos_p"]) and bool((a["pos_p"][:, p:] == -1).all())
    assert torch.equal(a["term_p"][:, :p], b["term_p"]) and not bool(a["term_p"][:, p:].any())
    assert torch.equal(a["pos_e"][:, :e], b["pos_e"]) and bool((a["pos_e"][:, e:] == -1).all())
    assert torch.equal(a["gone"][:, :e], b["gone"]) and bool(a["gone"][:, e:].all())
    assert torch.equal(a["term_e"][:, :e], b["term_e"])
    for k in ("map_id", "tick", "t"):
        assert torch.equal(a[k], b[k]), k


def counts_tensor(blocks, per):
    """[len(blocks) * per, 2]: `per` envs at each (p, e) of blocks, block after block"""
    return torch.tensor([c for c in blocks for _ in range(per)], dtype=torch.int32, device=DEV)


def assert_live_equals_fixed(env, fix, p, e, P, steps, rng, state_every, last_too=False):
    """env (capacity P pursuers, per_env_counts=True) with every env at live (p, e) against fix, a fixed-shape (p, e) batch of the same
    seed and env_id_base: the reset and `steps` free-running steps, the state compared every `state_every` steps (and after the last)"""
    N = env.n_envs
    env.set_agent_counts(p, e)
    obs_c, obs_f = env.reset(), fix.reset()
    assert torch.equal(obs_c[:, :p], obs_f) and not bool(obs_c[:, p:].any())
    pursuit_state_equal(env, fix, p, e)
    for it in range(steps):
        act = torch.as_tensor(rng.randint(5, size=(N, P)), device=DEV, dtype=torch.int32)
        obs_c, rew_c, done_c, info_c = env.step(act)
        obs_f, rew_f, done_f, info_f = fix.step(act[:, :p].contiguous())
        assert torch.equal(obs_c[:, :p], obs_f), it
        assert not bool(obs_c[:, p:].any()), it   # rows >= p never written (the buffer started as zeros)
        assert torch.equal(rew_c[:, :p], rew_f) and not bool(rew_c[:, p:].any()), it
        assert torch.equal(info_c["done_bits"], info_f["done_bits"]) and torch.equal(info_c["removed"], info_f["removed"]), it
        assert torch.equal(env._flags, fix._flags), it   # done / truncated / count_overflow flag plane
        if it % state_every == state_every - 1 or (last_too and it == steps - 1):
            pursuit_state_equal(env, fix, p, e)
    pend, live = env.agent_counts()
    assert bool((live == torch.tensor([p, e], device=DEV, dtype=torch.int32)).all()) and torch.equal(pend, live)


def assert_pending_counts_history(envs, counts, P):
    """envs: the same batch on the live kernel ("wave") and on the generic kernel, freshly built (zeroed buffers); counts: the counts the
    envs start with.  Counts change mid-episode (down, then back up: rows that were not written for a while come back) and take effect at
    each env's own reset, explicit or fused; the two kernels must agree on every output, also after an in-place edit of the returned
    observations (what a fast path knew about the buffer no longer holds, and the edited values must be left alone)."""
    N = len(counts)
    for env in envs:
        env.set_agent_counts(counts[:, 0], counts[:, 1])
        env.reset()
    rng = np.random.RandomState(1)
    k = torch.arange(P, device=DEV)[None, :]

    def step_both(it):
        act = torch.as_tensor(rng.randint(5, size=(N, P)), device=DEV)
        out = [env.step(act) for env in envs]
        (ow, rw, dw, iw), (og, rg, dg, ig) = out
        assert torch.equal(ow, og) and torch.equal(rw, rg) and torch.equal(iw["done_bits"], ig["done_bits"]), it
        assert torch.equal(iw["removed"], ig["removed"]) and torch.equal(envs[0]._flags, envs[1]._flags), it
        return iw, (ow, og)

    for it in range(7):
        step_both(it)
    schedule = [counts.flip(0).contiguous(), counts.contiguous()]   # the floor block goes to full capacity and back, the full block down
    live = counts
    for phase, new in enumerate(schedule):
        for env in envs:
            env.set_agent_counts(new[:, 0], new[:, 1])
        switched = torch.zeros(N, dtype=torch.bool, device=DEV)
        for it in range(30):
            info, obs = step_both((phase, it))
            switched |= info["done_bits"] != 0
            for env in envs:
                pend, lv = env.agent_counts()
                assert torch.equal(pend, new)
                assert torch.equal(lv, torch.where(switched[:, None], new, live)), (phase, it)
                st = env.get_state()
                ghost = k >= lv[:, :1]
                assert bool((st["pos_p"][ghost] == -1).all()) and bool((st["pos_p"][~ghost] >= 0).all())
                assert torch.equal(env.live_agents(), ~ghost)
        assert bool(switched.all())   # max_steps 25: every env has reset
        live = new
        if phase == 0:   # an in-place edit of the returned tensor: the fast path must notice it (no stale-zero promise holds any more)
            for o in obs:
                o.view(N, P, -1)[:, :, ::7] += 0.5
    # an explicit reset(mask=) takes the pending counts of the masked envs only
    new = torch.tensor([[5, 9]], dtype=torch.int32, device=DEV).repeat(N, 1)
    mask = torch.arange(N, device=DEV) % 2 == 1
    outs = []
    for env in envs:
        env.set_agent_counts(new[:, 0], new[:, 1])
        outs.append(env.reset(mask=mask))
        assert torch.equal(env.agent_counts()[1], torch.where(mask[:, None], new, live))
    assert torch.equal(outs[0], outs[1])
    for it in range(5):
        step_both(("after reset", it))
    for env, kind in zip(envs, ("wave", "generic")):
        assert env.kernel_kind == kind
