"""Batched MAWaterWorld on MI355X -- host-side mirror of the reference class
`madrl_environments.pursuit.MAWaterWorld` (waterworld.py:75-436).

* `BatchedMAWaterWorld(n_pursuers, n_evaders, ..., n_envs=..., device=...)`: same positional /
  keyword arguments and defaults as the reference constructor (:77-81), same `agents`,
  `reward_mech`, `timestep_limit`, `reset()`, `step()`, `seed()`, `is_terminal`; tensors:
      reset()       -> obs float32 [N, Np, D]          D = 7K + 3  (K sensors)
      step(action)  -> obs, rew float32 [N, Np], done bool [N], {'evcatches','pocatches': int32 [N]}
* `MAWaterWorld(...)`: N == 1 drop-in with the reference's return types.

Arithmetic is float32 in the HIP kernel (reference: float64; tolerance 1e-5, tests/).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .base import Agent
from .particle import BatchedParticleWorld, ParticleWorld, sensor_vectors  # noqa: F401  (sensor_vectors: imported from here by callers)
from .spaces import Box


class Archea(Agent):
    """waterworld.py:10-72 (spaces only)."""

    def __init__(self, idx, obs_dim):
        self._idx = idx
        self._obs_dim = obs_dim

    @property
    def observation_space(self):
        return Box(low=-10, high=10, shape=(self._obs_dim,))

    @property
    def action_space(self):
        return Box(low=-1, high=1, shape=(2,))


class BatchedMAWaterWorld(BatchedParticleWorld):
    _SYM, _AGENT = "madrl_waterworld", Archea
    _COUNTS, _INJECT = ("n_pursuers", "n_evaders", "n_poison"), "n_particles"
    _INFO_KEYS = ("evcatches", "pocatches")
    _WAVE_LIVE = True
    _STATE = (("pos", torch.float32, ("NP", 2)), ("vel", torch.float32, ("NP", 2)), ("obst", torch.float32, (2,)), ("t", torch.int32, ()),
              ("tick", torch.int32, ()))

    def __init__(self, n_pursuers, n_evaders, n_coop=2, n_poison=10, radius=0.015, obstacle_radius=0.2,
                 obstacle_loc=np.array([0.5, 0.5]), ev_speed=0.01, poison_speed=0.01, n_sensors=30,
                 sensor_range=0.2, action_scale=0.01, poison_reward=-1., food_reward=1., encounter_reward=.05,
                 control_penalty=-.5, reward_mech='local', addid=True, speed_features=True,
                 n_envs=1, device="cuda:0", seed=0, env_id_base=0, max_steps=0, auto_reset=False, max_blocks=0,
                 crowd=False, per_env_counts=False, obs_dtype=torch.float32, **kwargs):
        """crowd=True: the multi-wavefront kernel (csrc/waterworld_crowd.hip) -- up to 128 pursuers and 1 023 particles per env, any
        sensor count; same results bit for bit on a shape both kernels take.  The default keeps the one-wavefront kernel and its limits
        (62 particles, 32 pursuers).
        per_env_counts=True (with crowd=True): n_pursuers / n_evaders / n_poison are a capacity and every env runs its own counts
        (set_particle_counts), taken at its next reset; all tensors keep the capacity's shapes, slotted by class (pursuer i at i, evader
        m at n_pursuers + m, poison m at n_pursuers + n_evaders + m).  A pickle keeps the constructor arguments only: the counts of the
        copy are back at the capacity.
        per_env_counts="wave" (without crowd=True): the same contract on the one-wavefront kernel (waterworld_kernel_live), for a capacity
        within its limits -- the twin of an env at (p, e, po) is then env n of a fixed-shape one-wavefront batch, which computes what the
        crowd kernel does.  Which to choose: "wave" whenever the capacity fits 62 particles and 32 pursuers (one wavefront per env instead
        of a workgroup of four; DESIGN.md 4.4c has the timing); crowd=True, per_env_counts=True beyond that.  The live one-wavefront kernel
        is the generic instantiation -- there is no compile-time capacity -- and has no fused StandardizedEnv (the wrapper runs its epilogue
        kernels).
        sensor_range: a float or, as in the reference (waterworld.py:96, :109), one value per pursuer.  An array whose elements differ
        runs on the ranged kernels (madrl_waterworld_set_sensor_ranges; crowd=True or not): observation row i is bit for bit row i of a
        batch with sensor_range=sensor_range[i], everything else is unchanged.  Such a batch runs the generic one-wavefront kernel whatever
        its shape, has no fused StandardizedEnv (the wrapper runs its epilogue kernels) and does not combine with per_env_counts
        (ValueError).  An all-equal array is the float.
        obs_dtype=torch.float16: every observation tensor the env hands out or accepts (reset(), reset(mask=), step(), step(respawn=),
        step_on_stream(), step(obs_out=)) is float16 and holds, element for element, the round-to-nearest-even half of what the float32 env
        holds (torch's .to(torch.float16): subnormals kept); rewards, done, info and the state are the float32 env's, bit for bit.  Half the
        bytes per stored row -- a rollout's observation slots (RolloutCollector(store_observations=True)) are allocated in this dtype, and
        WaterworldHeuristicPolicy(obs_dtype=torch.float16) reads them.  It runs on the fixed-shape one-wavefront kernel alone (specialised
        for the shapes of csrc/waterworld_specializations.def): with crowd=True, per_env_counts or differing ranges it is a ValueError, it
        has no fused StandardizedEnv (fused_standardize is False; a StandardizedEnv without enable_obsnorm passes the rows through, one with
        it and ObservationBuffer raise TypeError), and any other dtype is a ValueError."""
        # like the reference, unknown kwargs are swallowed (waterworld.py:81,:483 passes obs_loc=None)
        self._ctor = dict(locals())
        self._ctor.pop("self"); self._ctor.pop("kwargs"); self._ctor.pop("__class__", None)
        self._flags(crowd, per_env_counts)
        self.n_pursuers, self.n_evaders, self.n_coop, self.n_poison = n_pursuers, n_evaders, n_coop, n_poison
        self.radius, self.obstacle_radius, self.obstacle_loc = radius, obstacle_radius, obstacle_loc
        self.ev_speed, self.poison_speed, self.n_sensors = ev_speed, poison_speed, n_sensors
        self.sensor_range = np.ones(n_pursuers) * sensor_range
        if self._ranged:   # checked here, before a device is touched
            if not (np.isfinite(self.sensor_range).all() and (self.sensor_range > 0).all()):
                raise ValueError("sensor_range: every element of a per-pursuer array must be finite and > 0 (got %r)" % (self.sensor_range,))
            if self.per_env_counts:
                raise ValueError("per-pursuer sensor ranges do not combine with per_env_counts: the live-count kernels take one range "
                                 "(pass a float, or an array of equal elements)")
        self._half(obs_dtype, self._ranged)
        self.action_scale, self.poison_reward, self.food_reward = action_scale, poison_reward, food_reward
        self.control_penalty, self.encounter_reward = control_penalty, encounter_reward
        self.n_obstacles = 1
        self._reward_mech, self._addid, self._speed_features = reward_mech, addid, speed_features
        self.n_envs, self.device = int(n_envs), torch.device(device)
        self._seed_value, self.env_id_base = int(seed), int(env_id_base)
        self.max_steps, self.auto_reset, self._max_blocks = int(max_steps), bool(auto_reset), int(max_blocks)
        self._handle = None
        self.setup()

    def _config(self):
        c = _lib.WaterworldConfig()
        c.struct_size = C.sizeof(_lib.WaterworldConfig)
        c.n_pursuers, c.n_evaders, c.n_coop, c.n_poison = self.n_pursuers, self.n_evaders, self.n_coop, self.n_poison
        c.n_sensors, c.addid, c.speed_features = self.n_sensors, int(bool(self._addid)), int(bool(self._speed_features))
        c.reward_global = int(self._reward_mech == "global")
        c.obstacle_fixed = int(self.obstacle_loc is not None)
        c.max_steps, c.auto_reset, c.crowd = self.max_steps, int(self.auto_reset), int(self._crowd)
        c.radius, c.obstacle_radius = float(self.radius), float(self.obstacle_radius)
        c.ev_speed, c.poison_speed = float(self.ev_speed), float(self.poison_speed)
        c.sensor_range, c.action_scale = float(self.sensor_range[0]), float(self.action_scale)
        c.poison_reward, c.food_reward = float(self.poison_reward), float(self.food_reward)
        c.encounter_reward, c.control_penalty = float(self.encounter_reward), float(self.control_penalty)
        if self.obstacle_loc is not None:
            c.obstacle_loc[0], c.obstacle_loc[1] = float(self.obstacle_loc[0]), float(self.obstacle_loc[1])
        c.seed, c.env_id_base = self._seed_value, self.env_id_base
        return c

    @property
    def _ranged(self):
        """the elements of sensor_range differ: the batch runs on the ranged kernels (read from the live attribute, like every parameter)"""
        r = np.asarray(self.sensor_range, dtype=np.float64).reshape(-1)
        return bool((r != r[0]).any())

    def _bind_handle(self, h):
        if self._ranged:   # every handle the batch creates: the constructor's, seed()'s, set_param_values()'s, an unpickled copy's
            r = np.ascontiguousarray(self.sensor_range, dtype=np.float64).reshape(-1)
            if r.shape != (int(self.n_pursuers),):
                raise ValueError("sensor_range has %d elements for %d pursuers" % (r.size, int(self.n_pursuers)))
            _lib.check(_lib.lib().madrl_waterworld_set_sensor_ranges(h, r.ctypes.data_as(C.c_void_p)))

    @property
    def fused_standardize(self):
        return not self._ranged and super().fused_standardize

    def bind_standardize(self, *args, **kwargs):
        if self._ranged:
            raise _lib.MadrlError("bind_standardize: the ranged kernel (per-pursuer sensor_range) has no fused StandardizedEnv; "
                                  "StandardizedEnv(env) or StandardizedEnv(env, fused=False) runs the epilogue kernels over it")
        return super().bind_standardize(*args, **kwargs)

    _hinted = set()

    def _hint_fast_path(self, D):
        """A large batch of a shape that is not in csrc/waterworld_specializations.def runs on the generic instantiation (dynamic LDS layout,
        run-time loop bounds: about half the speed): say once per shape how to give it its own kernel.  Results are identical either way."""
        if self._ranged:   # the ranged kernel takes its shape at run time: there is nothing to specialise
            return
        from . import build as _build
        shape = (int(self.n_pursuers), int(self.n_evaders), int(self.n_poison), int(self.n_sensors), int(D))
        if shape in BatchedMAWaterWorld._hinted or _build.waterworld_is_specialised(*shape):
            return
        import warnings
        BatchedMAWaterWorld._hinted.add(shape)
        warnings.warn("MAWaterWorld with %d pursuers / %d evaders / %d poison / %d sensors (obs_dim %d) runs on the generic kernel; `python -m madrl_amd.build "
                      "--waterworld-shape %d %d %d %d %d` compiles the specialised kernel for this shape (results are identical, a step takes about half the "
                      "time)" % (shape + shape), stacklevel=3)

    _LAUNCH_KERNELS = ("none", "generic", "specialised", "live", "ranged", "crowd")

    @property
    def last_launch_kernel(self):
        """the kernel family the handle's last reset / step launch ran on (include/madrl_hip.h, madrl_waterworld_last_launch_kernel): "none"
        before the first launch of a handle, "specialised" for a fixed-shape launch of a shape in csrc/waterworld_specializations.def,
        "generic" for any other fixed-shape one-wavefront launch, "live" / "ranged" for the per-env-count and per-pursuer-range entries,
        "crowd" with crowd=True.  float32 and float16 rows report alike."""
        out = C.c_int32()
        _lib.check(_lib.lib().madrl_waterworld_last_launch_kernel(self._handle, C.byref(out)))
        return self._LAUNCH_KERNELS[out.value]

    def get_param_values(self):
        return self.__dict__

    @property
    def is_terminal(self):
        return self.get_state()["t"] >= self.timestep_limit

    def set_particle_counts(self, n_pursuers=None, n_evaders=None, n_poison=None, mask=None):
        """PENDING counts of the envs in `mask` (all: None): an int or an int [N] per count, each in 1 .. the capacity.  An env takes them
        at its next reset -- reset(), reset(mask=) or the auto-reset of a step; its running episode keeps its particles."""
        self._set_pending((n_pursuers, n_evaders, n_poison), mask)

    def set_state(self, pos=None, vel=None, obst=None, t=None, tick=None, counts=None):
        """counts (per_env_counts=True): live counts int [N, 3] of the state being restored; pos and vel (slotted at the capacity) must
        come with them.  The pending counts are not touched."""
        if counts is not None:
            live, pos, vel = self._restored_counts(counts, pos, vel)
            self._live.copy_(live)
        self._set_state(dict(pos=pos, vel=vel, obst=obst, t=t, tick=tick))


class MAWaterWorld(ParticleWorld):
    """N == 1 drop-in with the reference's return types (waterworld.py:75)."""
    _BATCHED = BatchedMAWaterWorld

    def step(self, action_Np2):
        return self._step(action_Np2)
