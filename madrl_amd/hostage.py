"""Batched ContinuousHostageWorld on MI355X -- host-side mirror of the reference class
`madrl_environments.hostage.ContinuousHostageWorld` (hostage.py:74-430).

* `BatchedContinuousHostageWorld(n_good, n_hostages, n_bad, n_coop_save, n_coop_avoid, ..., n_envs=..., device=...)`: same
  positional / keyword arguments and defaults as the reference constructor (:76-81), same `agents`, `reward_mech`,
  `timestep_limit`, `reset()`, `step()`, `seed()`, `is_terminal`, `is_gate_open`; tensors:
      reset()       -> obs float32 [N, n_good, D]          D = 5K + 6  (K sensors)
      step(action)  -> obs, rew float32 [N, n_good], done bool [N], {'ho_saved','cr_encs': int32 [N]}
  `crowd=True` runs envs beyond one wavefront's worth of particles (more than 61 particles or 32 rescuers) on the multi-wavefront kernel;
  with `per_env_counts=True` as well, n_good / n_hostages / n_bad are a capacity and every env runs its own counts.
* `ContinuousHostageWorld(...)`: N == 1 drop-in with the reference's return types.

Arithmetic is float32 in the HIP kernel (reference: float64; tolerance 1e-5, tests/)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .base import Agent
from .particle import BatchedParticleWorld, ParticleWorld
from .spaces import Box


class CircAgent(Agent):
    """hostage.py:10-60 (spaces only)."""

    def __init__(self, idx, obs_dim):
        self._idx, self._obs_dim = idx, obs_dim

    @property
    def observation_space(self):
        return Box(low=-np.inf, high=np.inf, shape=(self._obs_dim,))

    @property
    def action_space(self):
        return Box(low=-10, high=10, shape=(2,))


class BatchedContinuousHostageWorld(BatchedParticleWorld):
    _SYM, _AGENT = "madrl_hostage", CircAgent
    _COUNTS, _INJECT = ("n_good", "n_hostages", "n_bad"), "n_bad"
    _INFO_KEYS = ("ho_saved", "cr_encs")
    _STATE = (("pos", torch.float32, ("NP", 2)), ("vel", torch.float32, ("NP", 2)), ("key", torch.float32, (2,)), ("bomb", torch.float32, (2,)),
              ("saved", torch.int64, ()), ("flags", torch.uint8, ()), ("t", torch.int32, ()), ("tick", torch.int32, ()))

    def __init__(self, n_good, n_hostages, n_bad, n_coop_save, n_coop_avoid, radius=0.015, key_loc=None, bad_speed=0.01, n_sensors=30,
                 sensor_range=0.2, action_scale=0.01, save_reward=5., hit_reward=-1., encounter_reward=0.01, not_saved_reward=-3,
                 bomb_reward=-5., bomb_radius=0.05, key_radius=0.0075, control_penalty=-.1, reward_mech='global', addid=True,
                 n_envs=1, device="cuda:0", seed=0, env_id_base=0, max_steps=0, auto_reset=False, max_blocks=0, crowd=False,
                 per_env_counts=False, obs_dtype=torch.float32, **kwargs):
        """crowd=True: the multi-wavefront kernel (csrc/hostage_crowd.hip) -- up to 128 rescuers, 64 hostages and 1 023 particles per env,
        any sensor count up to 256; the same results bit for bit on a shape both kernels take.  Without it an env holds at most 61 particles
        and 32 rescuers.
        per_env_counts=True (with crowd=True): n_good / n_hostages / n_bad are a capacity and every env runs its own counts
        (set_particle_counts), taken at its next reset; all tensors keep the capacity's shapes, slotted by class (rescuer i at i, hostage m
        at n_good + m, criminal m at n_good + n_hostages + m; bit m of the saved mask is hostage m).  A pickle keeps the constructor
        arguments only: the counts of the copy are back at the capacity.  per_env_counts="wave" (Waterworld's one-wavefront form) is a
        ValueError here: hostage_kernel has no live counts.
        obs_dtype=torch.float16: every observation tensor the env hands out or accepts (reset(), reset(mask=), step(), step(respawn=),
        step_on_stream(), step(obs_out=)) is float16 and holds, element for element, the round-to-nearest-even half of what the float32 env
        holds (torch's .to(torch.float16): subnormals kept); rewards, done, info and the state are the float32 env's, bit for bit.  It runs
        on the one-wavefront kernel alone (specialised for 3 / 10 / 5 with 30 sensors): with crowd=True or per_env_counts it is a
        ValueError, it has no fused StandardizedEnv (fused_standardize is False; a StandardizedEnv without enable_obsnorm passes the rows
        through, one with it and ObservationBuffer raise TypeError), and any other dtype is a ValueError."""
        self._ctor = dict(locals())
        self._ctor.pop("self"); self._ctor.pop("kwargs"); self._ctor.pop("__class__", None)
        self._flags(crowd, per_env_counts)
        self._half(obs_dtype)
        self.n_good, self.n_hostages, self.n_bad = n_good, n_hostages, n_bad
        self.n_coop_save, self.n_coop_avoid, self.radius, self.key_loc = n_coop_save, n_coop_avoid, radius, key_loc
        self.key_radius, self.bad_speed, self.n_sensors = key_radius, bad_speed, n_sensors
        self.sensor_range = np.ones(n_good) * sensor_range
        self.action_scale, self.save_reward, self.hit_reward = action_scale, save_reward, hit_reward
        self.encounter_reward, self.not_saved_reward, self.bomb_reward = encounter_reward, not_saved_reward, bomb_reward
        self.bomb_radius, self.control_penalty = bomb_radius, control_penalty
        self._reward_mech, self._addid = reward_mech, addid
        self.n_envs, self.device = int(n_envs), torch.device(device)
        self._seed_value, self.env_id_base = int(seed), int(env_id_base)
        self.max_steps, self.auto_reset, self._max_blocks = int(max_steps), bool(auto_reset), int(max_blocks)
        self._handle = None
        self.setup()

    def _config(self):
        c = _lib.HostageConfig()
        c.struct_size = C.sizeof(_lib.HostageConfig)
        c.n_good, c.n_hostages, c.n_bad = self.n_good, self.n_hostages, self.n_bad
        c.n_coop_save, c.n_coop_avoid, c.n_sensors = self.n_coop_save, self.n_coop_avoid, self.n_sensors
        c.addid, c.reward_global = int(bool(self._addid)), int(self._reward_mech == "global")
        c.key_fixed = int(self.key_loc is not None)
        c.max_steps, c.auto_reset = self.max_steps, int(self.auto_reset)
        c.radius, c.bad_speed = float(self.radius), float(self.bad_speed)
        c.sensor_range, c.action_scale = float(self.sensor_range[0]), float(self.action_scale)
        c.save_reward, c.hit_reward, c.encounter_reward = float(self.save_reward), float(self.hit_reward), float(self.encounter_reward)
        c.not_saved_reward, c.bomb_reward = float(self.not_saved_reward), float(self.bomb_reward)
        c.bomb_radius, c.key_radius, c.control_penalty = float(self.bomb_radius), float(self.key_radius), float(self.control_penalty)
        if self.key_loc is not None:
            k = np.asarray(self.key_loc, np.float64).reshape(2)
            c.key_loc[0], c.key_loc[1] = float(k[0]), float(k[1])
        c.seed, c.env_id_base = self._seed_value, self.env_id_base
        c.crowd = int(self._crowd)
        return c

    def fused_standardize_pays(self, enable_obsnorm=False, enable_rewnorm=False):
        """whether StandardizedEnv(env) should fuse by itself (fused=None): where the fused step measured faster than step + epilogue launches.
        32 768 envs of (3, 10, 5, 2, 2): with obsnorm + rewnorm 121.5 us fused against 129.4-130.1; without normalisation 40.1-40.4 against
        32.8-33.2.  The gain is the observation pass, so the rule is: with enable_obsnorm.  fused=True fuses either way."""
        return bool(enable_obsnorm)

    @property
    def is_gate_open(self):
        return (self.get_state()["flags"] & 1).bool()

    def _all_saved(self, n_hostages):
        """the saved mask of "all saved" for hostage counts int [N], as the int64 the state holds it in"""
        h = n_hostages.to(torch.int64)
        return torch.where(h >= 64, torch.full_like(h, -1), (torch.ones_like(h) << h.clamp(max=63)) - 1)

    @property
    def is_terminal(self):
        s = self.get_state()
        if self.per_env_counts:   # each env's live hostage count
            allm = self._all_saved(s["counts"][:, 1])
        else:
            allm = (1 << self.n_hostages) - 1
            if self.n_hostages >= 64:
                allm = -1   # the 64 bits of the mask as the int64 the state holds them in: the top one is the sign
        return ((s["flags"] & 2) != 0) | ((s["saved"] & allm) == allm) | (s["t"] >= self.timestep_limit)  # :179-182

    def set_particle_counts(self, n_good=None, n_hostages=None, n_bad=None, mask=None):
        """PENDING counts of the envs in `mask` (all: None): an int or an int [N] per count, each in 1 .. the capacity.  An env takes them
        at its next reset -- reset(), reset(mask=) or the auto-reset of a step; its running episode keeps its particles."""
        self._set_pending((n_good, n_hostages, n_bad), mask)

    def set_state(self, counts=None, **kw):
        """counts (per_env_counts=True): live counts int [N, 3] of the state being restored; pos and vel (slotted at the capacity) must
        come with them, and the bits of `saved` at or above an env's hostage count are cleared.  The pending counts are not touched."""
        def signed(v):   # numpy's unsigned masks and ticks as the int64 torch takes
            v = np.asarray(v)
            return v.astype(np.int64) if v.dtype in (np.uint64, np.uint32) else v
        if counts is not None:
            live, kw["pos"], kw["vel"] = self._restored_counts(counts, kw.get("pos"), kw.get("vel"))
            if kw.get("saved") is not None:
                sv = kw["saved"]
                sv = torch.as_tensor(sv if torch.is_tensor(sv) else signed(sv), device=self.device).reshape(self.n_envs).to(torch.int64)
                kw["saved"] = sv & self._all_saved(live[:, 1])
            self._live.copy_(live)
        self._set_state(kw, signed)


class ContinuousHostageWorld(ParticleWorld):
    """N == 1 drop-in with the reference's return types (hostage.py:74)."""
    _BATCHED = BatchedContinuousHostageWorld

    def step(self, action_Nr2):
        return self._step(action_Nr2)

    @property
    def is_gate_open(self):
        return bool(self._env.is_gate_open[0].item())
