"""The host layer the two particle worlds share (madrl_amd/waterworld.py, madrl_amd/hostage.py): buffers and handle, seed / reset / step,
the fused StandardizedEnv binding, state access, pickling -- and the N == 1 drop-in shell.  A world declares its C symbols, attribute names,
info keys and state layout (the class attributes below) and keeps its constructor, `_config()` and what only it has."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib
from .base import AbstractMAEnv, SingleEnvDelegate

_CALLS = ("obs_dim", "state_bytes", "create", "destroy", "set_launch", "kernel_kind", "set_particle_counts", "set_standardize", "reset", "step",
          "get_state", "set_state", "reset_f16", "step_f16")
_API = {}   # C symbol prefix -> the world's functions under their short names (filled by setup(): nothing is kept on the instance)


def _api(prefix):
    L = _lib.lib()
    if prefix not in _API:
        _API[prefix] = SimpleNamespace(**{name: getattr(L, "%s_%s" % (prefix, name)) for name in _CALLS})
    return _API[prefix]


def sensor_vectors(n_sensors):
    """Archea.__init__, waterworld.py:29-31: unit vectors of the K ray sensors (float64)."""
    angles = np.linspace(0., 2. * np.pi, n_sensors + 1)[:-1]
    return np.ascontiguousarray(np.c_[np.cos(angles), np.sin(angles)])


class BatchedParticleWorld(AbstractMAEnv):
    """A subclass's constructor assigns the reference's parameters, `_ctor`, `_crowd`, n_envs, device, `_seed_value`, env_id_base, max_steps,
    auto_reset, `_max_blocks` and `_handle = None`, then calls setup().  Every parameter, the agent count included, is read from the live
    attributes where it is used: nothing of them is copied here.
    per_env_counts=True (which `_flags()` takes from the constructor, with crowd=True): the `_COUNTS` attributes are a capacity and every env
    runs its own counts, taken at its next reset (set_particle_counts of the world, with its own keyword names); all tensors keep the
    capacity's shapes, slotted by class.  per_env_counts="wave" (without crowd=True) is the same on the one-wavefront kernel, for a world
    whose one-wavefront kernel has a live-count entry (`_WAVE_LIVE`).
    obs_dtype=torch.float16 (which `_half()` takes from the constructor): every observation tensor the env hands out or accepts is float16
    -- the round-to-nearest-even half of what the float32 env holds there; rewards, done, info and the state are the float32 env's.  It
    runs on the fixed-shape one-wavefront kernels alone (madrl_*_reset_f16 / madrl_*_step_f16)."""
    per_env_counts = False
    obs_dtype = torch.float32
    _WAVE_LIVE = False  # the world's one-wavefront kernel takes per-env counts (per_env_counts="wave")
    _SYM = None         # prefix of the C symbols: "madrl_waterworld"
    _COUNTS = None      # names of the attributes that hold the particle counts, the agents' first: ("n_pursuers", "n_evaders", "n_poison")
    _INJECT = None      # name of the attribute that holds the row count of step(respawn=...)
    _INFO_KEYS = None   # the two info keys of step()
    _AGENT = None       # the agent class: _AGENT(idx, obs_dim)
    _STATE = None       # get_state / set_state: ((name, dtype, per-env shape), ...) in the C functions' order, "NP" = n_particles

    def _flags(self, crowd, per_env_counts):
        """the two kernel flags of a constructor, after `self._ctor = dict(locals())`: only a set flag travels, so pickles of the envs that
        existed before a flag stay what they were"""
        for flag in ("crowd", "per_env_counts"):
            if not self._ctor[flag]:
                self._ctor.pop(flag)
        if isinstance(per_env_counts, str):   # the one-wavefront form is asked for by value
            if per_env_counts != "wave":
                raise ValueError("per_env_counts must be False, True (the crowd kernel's form, with crowd=True) or \"wave\" (got %r)" % (per_env_counts,))
            if not self._WAVE_LIVE:
                raise ValueError("per_env_counts=\"wave\": the one-wavefront kernel of %s has no live counts; use crowd=True, per_env_counts=True"
                                 % type(self).__name__)
            if crowd:
                raise ValueError("per_env_counts=\"wave\" is the one-wavefront kernel's form: construct the batch without crowd=True "
                                 "(crowd=True takes per_env_counts=True)")
        elif per_env_counts not in (False, True, 0, 1, None):
            raise ValueError("per_env_counts must be False, True (the crowd kernel's form, with crowd=True) or \"wave\" (got %r)" % (per_env_counts,))
        elif per_env_counts and not crowd:
            raise ValueError("per_env_counts=True runs on the crowd kernel: construct the batch with crowd=True"
                             + (" (or ask for the one-wavefront kernel's form with per_env_counts=\"wave\")" if self._WAVE_LIVE else ""))
        self._crowd, self.per_env_counts = bool(crowd), bool(per_env_counts)

    def _half(self, obs_dtype, ranged=False):
        """the observation dtype of a constructor, after `_flags()` and before a device is touched: only a set one travels in `_ctor`"""
        if obs_dtype is torch.float32:   # (the class attribute says so: nothing is added to the instance either)
            self._ctor.pop("obs_dtype")
            return
        if obs_dtype is not torch.float16:
            raise ValueError("obs_dtype must be torch.float32 or torch.float16, got %r" % (obs_dtype,))
        elif self._crowd:
            raise ValueError("obs_dtype=torch.float16 runs on the one-wavefront kernel: the crowd kernel (crowd=True) has no half-precision rows")
        elif self.per_env_counts:
            raise ValueError("obs_dtype=torch.float16 runs on the fixed-shape kernel: the live-count kernels (per_env_counts) have no half-precision rows")
        elif ranged:
            raise ValueError("obs_dtype=torch.float16 runs on the fixed-shape kernel: the ranged kernel (a sensor_range whose elements differ) has "
                             "no half-precision rows (pass a float, or an array of equal elements)")
        self.obs_dtype = obs_dtype

    @property
    def _f16(self):
        return self.obs_dtype is torch.float16

    def setup(self):
        c = _api(self._SYM)
        if self.device.type != "cuda":
            raise _lib.MadrlError("%s needs a ROCm device (got %s); there is no CPU path" % (type(self).__name__, self.device))
        cfg = self._config()
        dim, nbytes = C.c_int32(), C.c_uint64()
        _lib.check(c.obs_dim(C.byref(cfg), C.byref(dim)))
        _lib.check(c.state_bytes(C.byref(cfg), self.n_envs, C.byref(nbytes)))
        counts = [getattr(self, k) for k in self._COUNTS]
        N, Na, D, dev = self.n_envs, counts[0], dim.value, self.device
        self.n_particles = sum(counts)
        if getattr(self, "_shape_key", None) != (N, Na, D, nbytes.value) or self._obs.dtype is not self.obs_dtype:
            self._state = torch.zeros(nbytes.value, dtype=torch.uint8, device=dev)
            self._obs = torch.zeros((N, Na, D), dtype=self.obs_dtype, device=dev)
            self._rew = torch.zeros((N, Na), dtype=torch.float32, device=dev)
            self._done = torch.zeros(N, dtype=torch.uint8, device=dev)
            self._info = torch.zeros((N, 2), dtype=torch.int32, device=dev)
            self._shape_key = (N, Na, D, nbytes.value)
        self.obs_dim = D
        self._destroy()
        h = C.c_void_p()
        self._sensors = sensor_vectors(self.n_sensors)
        dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
        _lib.check(c.create(C.byref(cfg), self._sensors.ctypes.data_as(C.c_void_p), N, dev_index, _lib.ptr(self._state), C.byref(h)))
        self._handle = h
        self._bind_handle(h)
        if self._max_blocks:
            _lib.check(c.set_launch(h, self._max_blocks))
        if N >= 4096 and not self._crowd and not self.per_env_counts:   # (the crowd and live-count kernels take their shape at run time: there is nothing to specialise)
            self._hint_fast_path(D)
        self._agents = [self._AGENT(i + 1, D) for i in range(Na)]
        # A fused StandardizedEnv binding belongs to the handle that was just replaced (seed() and set_param_values() come
        # through here): bind the new handle to the SAME statistics / output tensors, or -- when the shapes changed -- to
        # fresh ones, so that the wrapper keeps receiving standardised rows.
        old, self._std = getattr(self, "_std", None), None
        if old is not None:
            if tuple(old["obs_out"].shape) == (N, Na, D):
                self.bind_standardize(tensors=old, **self._std_kwargs)
            else:   # new shapes: fresh statistics, handed to the wrapper through the SAME dict object it holds
                fresh = self.bind_standardize(tensors=None, **self._std_kwargs)
                old.clear(); old.update(fresh)
                self._std = old
        if self.per_env_counts:   # the count tensors outlive a re-created handle of the same capacity (seed()); otherwise: the capacity
            cap = tuple(int(k) for k in counts)
            if getattr(self, "_counts_key", None) != (N, cap):
                self._pending = torch.tensor(cap, dtype=torch.int32, device=dev).repeat(N, 1).contiguous()
                self._live = self._pending.clone()
                self._counts_key = (N, cap)
            _lib.check(c.set_particle_counts(h, _lib.ptr(self._pending), _lib.ptr(self._live)))

    def _bind_handle(self, h):
        """what a world binds to every handle it creates, before anything else is (called by setup() itself)"""

    def _hint_fast_path(self, D):
        """a world with a list of specialised shapes says here that a large batch runs on the generic kernel (called by setup() itself)"""

    @property
    def kernel_kind(self):
        """"wave": one wavefront per env; "crowd": one workgroup of several wavefronts per env (crowd=True)"""
        kind = C.c_int32()
        _lib.check(_API[self._SYM].kernel_kind(self._handle, C.byref(kind)))
        return ("wave", "crowd")[kind.value]

    @property
    def fused_standardize(self):
        """whether bind_standardize() works on this env (StandardizedEnv asks): the crowd, live-count and half-precision kernels have no fused form"""
        return not self._crowd and not self.per_env_counts and not self._f16

    def set_launch(self, max_blocks=0):
        self._max_blocks = int(max_blocks)
        _lib.check(_API[self._SYM].set_launch(self._handle, self._max_blocks))

    def _destroy(self):
        if getattr(self, "_handle", None):
            _API[self._SYM].destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    # ------------------------------------------------------------------ reference API
    @property
    def reward_mech(self):
        return self._reward_mech

    @property
    def timestep_limit(self):
        return self.max_steps if self.max_steps > 0 else 1000  # waterworld.py:124-126, hostage.py:118-120

    @property
    def agents(self):
        return self._agents

    def seed(self, seed=None):
        if seed is None:
            seed = int(np.random.randint(2**31 - 1))
        self._seed_value = int(seed)
        self.setup()
        return [self._seed_value]

    def reset(self, mask=None):
        if mask is not None:
            mask = torch.as_tensor(mask, device=self.device).reshape(self.n_envs).to(torch.uint8).contiguous()
        std = getattr(self, "_std", None)
        if self._f16:   # (a half env binds no StandardizedEnv)
            _lib.check(_API[self._SYM].reset_f16(self._handle, _lib.ptr(mask), _lib.ptr(self._obs), _lib.current_stream(self.device)))
            return self._obs
        _lib.check(_API[self._SYM].reset(self._handle, _lib.ptr(mask), None if std else _lib.ptr(self._obs), _lib.current_stream(self.device)))
        return std["obs_out"] if std else self._obs

    # ------------------------------------------------------------------ fused StandardizedEnv (include/madrl_hip.h)
    def bind_standardize(self, scale_reward=1.0, enable_obsnorm=False, enable_rewnorm=False, obs_alpha=0.001, rew_alpha=0.001, eps=1e-8,
                         tensors=None):
        """The kernels normalise observations / rewards on their way out (madrl_*_set_standardize): reset() and
        step() then return the standardised tensors and the raw observation row is not stored.  Returns the dict of
        state tensors (running statistics, outputs) the wrapper owns; `tensors` re-binds an existing dict (setup()).
        The crowd kernel has no fused form: StandardizedEnv runs its epilogue kernels over such an env."""
        if self._crowd:
            raise _lib.MadrlError("bind_standardize: the crowd kernel (crowd=True) has no fused StandardizedEnv; "
                                  "StandardizedEnv(env) or StandardizedEnv(env, fused=False) runs the epilogue kernels over it")
        if self.per_env_counts:
            raise _lib.MadrlError("bind_standardize: the live-count kernel (per_env_counts=\"wave\") has no fused StandardizedEnv; "
                                  "StandardizedEnv(env) or StandardizedEnv(env, fused=False) runs the epilogue kernels over it")
        if self._f16:
            raise _lib.MadrlError("bind_standardize: the half-precision kernel (obs_dtype=torch.float16) has no fused StandardizedEnv; "
                                  "StandardizedEnv(env) without enable_obsnorm passes its rows through")
        N, Na, D, dev = self.n_envs, getattr(self, self._COUNTS[0]), self.obs_dim, self.device
        self._std_kwargs = dict(scale_reward=scale_reward, enable_obsnorm=enable_obsnorm, enable_rewnorm=enable_rewnorm,
                                obs_alpha=obs_alpha, rew_alpha=rew_alpha, eps=eps)
        st = tensors if tensors is not None else dict(
            obs_mean=torch.zeros((N, Na, D), dtype=torch.float64, device=dev), obs_var=torch.ones((N, Na, D), dtype=torch.float64, device=dev),
            obs_out=torch.zeros((N, Na, D), dtype=torch.float32, device=dev),
            rew_mean=torch.zeros((N, Na), dtype=torch.float64, device=dev), rew_var=torch.ones((N, Na), dtype=torch.float64, device=dev),
            rew_out=torch.zeros((N, Na), dtype=torch.float32, device=dev))
        a = _lib.StandardizeArgs()
        a.struct_size = C.sizeof(_lib.StandardizeArgs)
        a.enable_obsnorm, a.enable_rewnorm = int(bool(enable_obsnorm)), int(bool(enable_rewnorm))
        a.obs_alpha, a.rew_alpha, a.eps, a.scale_reward = float(obs_alpha), float(rew_alpha), float(eps), float(scale_reward)
        for k, v in st.items():
            setattr(a, k, v.data_ptr())
        _lib.check(_API[self._SYM].set_standardize(self._handle, C.byref(a)))
        self._std = st
        return st

    def unbind_standardize(self):
        _lib.check(_API[self._SYM].set_standardize(self._handle, None))
        self._std = None

    def step(self, action, respawn=None, obs_out=None):
        """waterworld.py:220-436, hostage.py:228-430.  action: float [N, n_agents, 2] (or anything that reshapes to it).
        respawn: optional float [N, rows, 4] injected respawn outcomes (parity hook; rows: every particle in Waterworld, the criminals in
        the hostage world).
        obs_out: optional contiguous destination of N * n_agents * obs_dim elements of the env's obs_dtype on the env's device (e.g. a slot
        of a trajectory tensor) the kernel writes the observations to instead of the env's own buffer; its [N, n_agents, D] view is returned.
        A float16 destination needs 2-byte alignment only.  Refused while a fused StandardizedEnv is bound: the observation tensor the
        kernel writes then belongs to the wrapper."""
        r = None
        if respawn is not None:
            r = torch.as_tensor(respawn, device=self.device).reshape(self.n_envs, getattr(self, self._INJECT), 4).to(torch.float32).contiguous()
        return self._launch_step(self._actions(action), r, _lib.current_stream(self.device), obs_out)

    @property
    def takes_obs_out(self):
        return self._std is None

    def step_into(self, actions, rew_out, done_out, obs_out=None):
        """AbstractMAEnv.step_into: the kernel writes rewards and done bytes into the caller's tensors (the C ABI takes any device pointer).
        While a fused StandardizedEnv is bound the rewards it hands out are the wrapper's: step() and the two copies then."""
        if self._std is not None:
            return super().step_into(actions, rew_out, done_out, obs_out)
        N, Na = self.n_envs, getattr(self, self._COUNTS[0])
        assert rew_out.dtype == torch.float32 and rew_out.numel() == N * Na and done_out.dtype == torch.uint8 and done_out.numel() == N
        return self._launch_step(self._actions(actions), None, _lib.current_stream(self.device), obs_out, rew_out, done_out)[0]

    def _actions(self, action):
        """step()'s action argument as the float32 [N, n_agents, 2] tensor the kernel reads"""
        if self._conforming(action):
            return action
        N, Na = self.n_envs, getattr(self, self._COUNTS[0])
        a = torch.as_tensor(action, device=self.device)
        if a.numel() != N * Na * 2:
            raise AssertionError("action has %d elements, expected %d" % (a.numel(), N * Na * 2))  # waterworld.py:227, hostage.py:234
        return a.reshape(N, Na, 2).to(torch.float32).contiguous()

    def _conforming(self, a):
        """an action tensor the kernel can read as it is (float32, contiguous, on the device, N * n_agents * 2 elements): no torch kernel needed"""
        return (type(a) is torch.Tensor and a.dtype is torch.float32 and a.device == self.device and a.is_contiguous()
                and a.numel() == self.n_envs * getattr(self, self._COUNTS[0]) * 2)

    def step_on_stream(self, action, stream):
        """step() launched on `stream` (a torch.cuda.Stream) without making it the current stream -- for callers that drive sub-batches on
        their own streams (madrl_amd/sharded.py): entering a `with torch.cuda.stream(...)` block costs the host more than this launch.
        Returns None when the action needs a conversion kernel (the caller then takes step() under the stream context)."""
        if not self._conforming(action):
            return None
        return self._launch_step(action, None, C.c_void_p(stream.cuda_stream))

    def _launch_step(self, a, r, stream_ptr, obs_out=None, rew=None, done=None):
        """rew / done: where the kernel writes rewards and done bytes (None: the env's own buffers)"""
        std = getattr(self, "_std", None)
        obs, rew, done = self._obs, self._rew if rew is None else rew, self._done if done is None else done
        if obs_out is not None:
            if std:
                raise ValueError("obs_out: a fused StandardizedEnv is bound to this env, the kernel's observation output belongs to the wrapper")
            obs = _lib.obs_destination(obs_out, self._obs)
        step = _API[self._SYM].step_f16 if self._f16 else _API[self._SYM].step
        _lib.check(step(self._handle, _lib.ptr(a), _lib.ptr(r), None if std else _lib.ptr(obs), _lib.ptr(rew),
                        _lib.ptr(done), _lib.ptr(self._info), stream_ptr))
        # `done` is a bool VIEW of the byte the kernel wrote (0 / 1): no torch kernel runs after the launch
        info = {self._INFO_KEYS[0]: self._info[:, 0], self._INFO_KEYS[1]: self._info[:, 1], "done_bits": done}
        if std:  # fused StandardizedEnv: standardised observations and scaled / normalised rewards straight from the kernel
            return std["obs_out"], std["rew_out"], done.view(torch.bool), info
        return obs, rew, done.view(torch.bool), info

    # ------------------------------------------------------------------ per-env particle counts (per_env_counts=True)
    def _require_counts(self, what):
        if not self.per_env_counts:
            raise RuntimeError("%s: this batch has one particle count for all envs; construct it with crowd=True, per_env_counts=True%s"
                               % (what, " or with per_env_counts=\"wave\"" if self._WAVE_LIVE else ""))

    def _checked_counts(self, v, col, name, m=None):
        """an int or an int [N] as int32 [N] within 1 .. the capacity (where m is set)"""
        t = torch.as_tensor(v, device=self.device).to(torch.int32)
        t = t.expand(self.n_envs) if t.dim() == 0 else t.reshape(self.n_envs)
        bad = (t < 1) | (t > int(getattr(self, self._COUNTS[col])))
        if bool((bad if m is None else bad & m).any()):
            raise ValueError("%s must be in 1..%d (the batch's capacity)" % (name, int(getattr(self, self._COUNTS[col]))))
        return t

    def _set_pending(self, values, mask):
        """set_particle_counts of a world: `values` in the order of _COUNTS, each None (stays), an int or an int [N]"""
        self._require_counts("set_particle_counts")
        m = torch.ones(self.n_envs, dtype=torch.bool, device=self.device) if mask is None else \
            torch.as_tensor(mask, device=self.device).reshape(self.n_envs) != 0
        new = [None if v is None else self._checked_counts(v, col, name, m) for col, (v, name) in enumerate(zip(values, self._COUNTS))]
        for col, t in enumerate(new):
            if t is not None:
                self._pending[:, col] = torch.where(m, t, self._pending[:, col])

    def particle_counts(self):
        """(pending, live): int32 [N, 3] copies of the counts per env, in the order of the constructor's -- what its next reset takes, and
        what its running episode has"""
        self._require_counts("particle_counts")
        return self._pending.clone(), self._live.clone()

    def live_agents(self):
        """bool [N, agents of the capacity]: the agents of each env's running episode (action rows past them are ignored, their reward and
        observation rows are zero)"""
        self._require_counts("live_agents")
        return torch.arange(int(getattr(self, self._COUNTS[0])), device=self.device)[None, :] < self._live[:, :1]

    def _slot_exists(self, live):
        """bool [N, NP]: the slots (the three classes at the capacity) that hold a particle under the live counts int [N, 3]"""
        parts = [torch.arange(int(getattr(self, k)), device=self.device)[None, :] < live[:, c:c + 1] for c, k in enumerate(self._COUNTS)]
        return torch.cat(parts, dim=1)

    def _restored_counts(self, counts, pos, vel):
        """set_state(counts=): the live counts int [N, 3] of the state being restored, checked -> (live int32 [N, 3], pos, vel) with
        (-1, -1) / 0 in the slots that hold no particle.  pos and vel, slotted at the capacity, must come with the counts.  The caller
        copies `live` into self._live once the rest of its arguments is checked; the pending counts are not touched."""
        self._require_counts("set_state(counts=)")
        if pos is None or vel is None:
            raise ValueError("set_state(counts=) needs pos and vel in the same call: the counts say which of their slots hold a particle")
        c = torch.as_tensor(counts if torch.is_tensor(counts) else np.asarray(counts), device=self.device).reshape(self.n_envs, 3)
        live = torch.stack([self._checked_counts(c[:, col], col, name) for col, name in enumerate(self._COUNTS)], dim=1)
        shape = (self.n_envs, self.n_particles, 2)
        conv = lambda v: torch.as_tensor(v if torch.is_tensor(v) else np.asarray(v), device=self.device).reshape(shape).to(torch.float32)
        is_ = self._slot_exists(live)[:, :, None]
        return live, torch.where(is_, conv(pos), -1.0), torch.where(is_, conv(vel), 0.0)

    # ------------------------------------------------------------------ state access
    def _state_layout(self):
        """_STATE with the batch's shapes: [(name, dtype, shape), ...]"""
        return [(k, dt, (self.n_envs,) + tuple(self.n_particles if s == "NP" else s for s in shape)) for k, dt, shape in self._STATE]

    def get_state(self):
        """with per_env_counts: also "counts", the live counts int32 [N, 3]; a slot without a particle reads (-1, -1) / (0, 0)"""
        st = {k: torch.zeros(shape, dtype=dt, device=self.device) for k, dt, shape in self._state_layout()}
        _lib.check(_API[self._SYM].get_state(self._handle, *[_lib.ptr(v) for v in st.values()], _lib.current_stream(self.device)))
        if self.per_env_counts:
            st["counts"] = self._live.clone()
        return st

    def _set_state(self, values, to_array=np.asarray):
        """values: {name: tensor, array-like or None (that part stays)}; to_array: what makes an array of a value that is no tensor"""
        args = []
        for k, dt, shape in self._state_layout():
            v = values.get(k)
            if v is not None:
                v = torch.as_tensor(v if torch.is_tensor(v) else to_array(v), device=self.device).reshape(shape).to(dt).contiguous()
            args.append(v)
        self._keepalive = args
        _lib.check(_API[self._SYM].set_state(self._handle, *[_lib.ptr(a) for a in args], _lib.current_stream(self.device)))

    def __getstate__(self):
        return dict(self._ctor)

    def __setstate__(self, d):
        self.__init__(**d)


class ParticleWorld(SingleEnvDelegate, AbstractMAEnv):
    """N == 1 drop-in with the reference's return types over a one-env `_BATCHED` engine."""
    _BATCHED = None

    def __init__(self, *args, **kwargs):
        kwargs.pop("n_envs", None)
        if kwargs.get("obs_dtype", torch.float32) is not torch.float32:   # the drop-in returns the reference's types: float64 arrays
            raise ValueError("%s returns the reference's float64 observations; obs_dtype=%r is for the batched engine (%s)"
                             % (type(self).__name__, kwargs["obs_dtype"], self._BATCHED.__name__))
        self._env = self._BATCHED(*args, n_envs=1, **kwargs)

    @property
    def agents(self):
        return self._env.agents

    @property
    def reward_mech(self):
        return self._env.reward_mech

    @property
    def timestep_limit(self):
        return self._env.timestep_limit

    def seed(self, seed=None):
        return self._env.seed(seed)

    def _obslist(self, obs):
        o = obs[0].detach().cpu().numpy().astype(np.float64)
        return [o[i] for i in range(o.shape[0])]

    def reset(self):
        return self._obslist(self._env.reset())

    def _step(self, action):
        """step() of a world, which keeps the reference's parameter name"""
        a = np.asarray(action, dtype=np.float64).reshape((len(self._env.agents), 2))  # waterworld.py:221-222, hostage.py:229-230
        obs, rew, done, info = self._env.step(a[None])
        return (self._obslist(obs), rew[0].detach().cpu().numpy().astype(np.float64), bool(done[0].item()),
                {k: int(info[k][0].item()) for k in self._env._INFO_KEYS})

    @property
    def is_terminal(self):
        return bool(self._env.is_terminal[0].item())
