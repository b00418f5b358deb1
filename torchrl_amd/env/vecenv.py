"""Host-side vector env over ordinary Python envs (torchrl/env/vecenv.py:6-78) and its bridge to the device
collectors.

`VecEnv` keeps the reference's protocol -- `reset()` -> (N, D); `step(actions (N, A))` -> (obs (N, D),
rewards (N, 1), dones (N, 1) bool, infos: key -> array over the envs that reported it); `partial_reset(mask)`
returns the WHOLE observation array; `seed(s)` gives env i the seed `s * N + i`; unknown attributes fall through
to the first env -- for envs with the gym interface (`reset()`, `step(a) -> (obs, reward, done, info)`,
`observation_space`, `action_space`, optional `seed / train / eval / close / render`).

The physics of such envs runs on the host, one Python call per env and step: that part is the reference's cost
and stays it.  Everything else of a collector step -- policy and value networks, exploration noise, log-probs,
time-limit bootstrap, episode bookkeeping, the replay write -- runs in the same HIP kernels as for the on-GPU
envs; `HostEnvBridge` is the adaptor the collectors wrap a `VecEnv` in (two small host syncs per step: actions
out, observations / rewards / dones in).  `HostFrameBridge` is the same adaptor for envs that return uint8 images:
the k-stacks the conv Q network reads are kept on the device (trl_frame_stack_push_u8)."""
import numpy as np
import torch

from .. import _C


class VecEnv:
    is_device_env = False
    # The reference's partial_reset writes the fresh observations INTO the array `step` just returned (vecenv.py:50), and
    # its collectors add the sample after the reset (collector/base.py:203-227, on_policy.py:132-151): the `next_obs` row
    # they store for an env that was reset in a step -- by `done` or by max_episode_frames, where `terminals` stays
    # False and the TD target bootstraps from it -- is the RESET observation.  True (default): reproduce exactly that
    # (tests/golden/collect_hostenv.npz).  False: the stored transition keeps the observation the env produced.
    alias_reset_obs = True

    def __init__(self, env_nums, env_funcs, env_args):
        self.env_nums = int(env_nums)
        if isinstance(env_funcs, (list, tuple)):
            if len(env_funcs) != self.env_nums or len(env_args) != self.env_nums:
                raise ValueError("need one env constructor and one argument tuple per env")
            self.env_funcs, self.env_args = list(env_funcs), list(env_args)
        else:
            self.env_funcs = [env_funcs] * self.env_nums
            self.env_args = [env_args] * self.env_nums
        self.set_up_envs()

    def set_up_envs(self):
        self.envs = [fn(*arg) for fn, arg in zip(self.env_funcs, self.env_args)]

    def _each(self, name, *args):
        for env in self.envs:
            fn = getattr(env, name, None)
            if callable(fn):
                fn(*args)

    def train(self):
        self._each("train")

    def eval(self):
        self._each("eval")

    def close(self):
        self._each("close")

    def render(self):
        self._each("render")

    def reset(self, **kwargs):
        self._obs = np.stack([np.asarray(env.reset()) for env in self.envs])
        return self._obs

    def partial_reset(self, index_mask, **kwargs):
        index_mask = np.asarray(index_mask).reshape(-1).astype(bool)
        if not self.alias_reset_obs:
            self._obs = self._obs.copy()                                   # leave the array `step` returned alone
        for index in np.flatnonzero(index_mask):
            self._obs[index] = np.asarray(self.envs[index].reset())
        return self._obs

    def step(self, actions):
        actions = np.asarray(actions)
        results = [env.step(np.squeeze(a)) for env, a in zip(self.envs, np.split(actions, self.env_nums))]
        obs, rews, dones, infos = zip(*results)
        self._obs = np.stack([np.asarray(o) for o in obs])
        merged = {}
        for info in infos:                                   # merge_with(np.array, *infos)
            for key, value in (info or {}).items():
                merged.setdefault(key, []).append(value)
        merged = {key: np.array(values) for key, values in merged.items()}
        return (self._obs, np.stack(rews).astype(np.float64)[:, np.newaxis],
                np.stack(dones).astype(bool)[:, np.newaxis], merged)

    def seed(self, seed):
        for idx, env in enumerate(self.envs):
            if callable(getattr(env, "seed", None)):
                env.seed(seed * self.env_nums + idx)

    @property
    def observation_space(self):
        return self.envs[0].observation_space

    @property
    def action_space(self):
        return self.envs[0].action_space

    def __getattr__(self, attr):
        if attr in ("envs", "_wrapped_env"):
            raise AttributeError(attr)
        return getattr(self.envs[0], attr)


class HostEnvBridge:
    """What the device collectors need from an env, for a host `VecEnv`: device mirrors of the current observations
    and of the per-env step / return counters, and the two host round trips of a step."""
    is_device_env = False
    is_host_env = True
    kind = "vector"

    def __init__(self, venv, device):
        self.venv = venv
        self.env_nums = int(venv.env_nums)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("collectors run their networks on the GPU: pass device='cuda:<n>'")
        obs_shape, act_space = venv.observation_space.shape, venv.action_space
        self.discrete = hasattr(act_space, "n")                           # Discrete(n): actions are (N,) integers
        if len(obs_shape) != 1 or not (self.discrete or (hasattr(act_space, "shape") and len(act_space.shape) == 1)):
            raise ValueError("HostEnvBridge drives flat-observation envs with Box or Discrete actions "
                             "(got observation %r, action %r)" % (obs_shape, act_space))
        self.obs_dim = int(obs_shape[0])
        self.act_dim = 1 if self.discrete else int(act_space.shape[0])    # stored action width
        self.action_num = int(act_space.n) if self.discrete else 0
        n = self.env_nums
        self.cur_obs = torch.zeros(n, self.obs_dim, device=self.device)
        self.cur_step = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.ep_return = torch.zeros(n, device=self.device)
        self.training = True
        # episode length if the envs advertise one (gym's TimeLimit, or a `horizon` attribute); 0: unknown
        self.horizon = int(getattr(venv, "_max_episode_steps", None) or getattr(venv, "horizon", None) or 0)

    # ---- the reference protocol, with device observations ----
    @property
    def observation_space(self):
        return self.venv.observation_space

    @property
    def action_space(self):
        return self.venv.action_space

    def train(self):
        self.training = True
        self.venv.train()

    def eval(self):
        self.training = False
        self.venv.eval()

    def close(self):
        self.venv.close()

    def render(self):
        self.venv.render()

    def seed(self, seed):
        self.venv.seed(seed)

    def _upload(self, array, out):
        out.copy_(torch.as_tensor(np.ascontiguousarray(array, dtype=np.float32)).view(out.shape), non_blocking=True)
        return out

    def reset(self, **kwargs):
        self._upload(self.venv.reset(**kwargs), self.cur_obs)
        self.cur_step.zero_()
        self.ep_return.zero_()
        return self.cur_obs

    # ---- the two host round trips of a collector step ----
    def host_step(self, act, next_obs, rewards, dones, time_limits=None):
        """act (N, A) device -> envs; fills the device rows next_obs (N, D), rewards, dones, time_limits (N, 1)."""
        a = act.detach().cpu().numpy()
        obs, rew, done, infos = self.venv.step(a.reshape(-1).astype(np.int64) if self.discrete else a.astype(np.float64))
        self._upload(obs, next_obs)
        self.cur_obs.copy_(next_obs)
        self._upload(rew, rewards)
        self._upload(done, dones)
        if time_limits is not None:
            if "time_limit" in infos and len(infos["time_limit"]) == self.env_nums:   # collector/base.py:213-215
                self._upload(infos["time_limit"], time_limits)
            else:
                time_limits.zero_()
        return done

    def host_partial_reset(self, mask, stored_next_obs=None):
        """mask (N,) uint8 device: reset those envs; `cur_obs` becomes the env's whole observation array.
        stored_next_obs: the ring row this step's `next_obs` went to when it holds env.step's own array (no observation
        wrapper in between) -- with `alias_reset_obs` it then reads what the reference stores, the array AFTER the reset."""
        m = mask.cpu().numpy().astype(bool)
        if m.any():
            self._upload(self.venv.partial_reset(m), self.cur_obs)
            if stored_next_obs is not None and getattr(self.venv, "alias_reset_obs", False):
                stored_next_obs.copy_(self.cur_obs)
        return m


def is_pixel_space(space):
    """An observation space of uint8 images: (H, W), (1, H, W) or (C, H, W)."""
    shape = tuple(getattr(space, "shape", None) or ())
    try:
        dtype = np.dtype(getattr(space, "dtype", np.float32))
    except TypeError:
        return False
    return len(shape) in (2, 3) and dtype == np.uint8


def bridge_host_env(venv, device, like=None):
    """The bridge the collectors wrap a host `VecEnv` in: `HostFrameBridge` for uint8 image observations (with the
    settings of `like`, another such bridge, when given: a deep copy of a `SubProcVecEnv` is a fresh object),
    `HostEnvBridge` for everything else."""
    if is_pixel_space(venv.observation_space):
        if isinstance(like, HostFrameBridge):                            # (settings the VecEnv carries itself come first)
            return HostFrameBridge(venv, device, frame_stack=getattr(venv, "frame_stack", like.frame_stack),
                                   clip_rewards=getattr(venv, "clip_rewards", like.clip_rewards))
        return HostFrameBridge(venv, device)
    return HostEnvBridge(venv, device)


class HostFrameBridge:
    """`HostEnvBridge` for host envs that return uint8 IMAGES -- the reference's pixel tasks stepped in Python behind
    WarpFrame -> FrameStack -> VecEnv (examples/dqn_atari_vec.py) -- with the attributes the collectors' frame path reads
    off `SynthFrameVecEnv`: `cur_obs` is the (N, C, H, W) uint8 stack the conv Q network reads, resident on the device.

    Two observation layouts of the wrapped `VecEnv` / `SubProcVecEnv`:
      single frames   the envs return (H, W) or (1, H, W) and the bridge is built with `frame_stack=k` (True: 4; default:
                      the `frame_stack` attribute the factory left on the VecEnv).  The host uploads the N new frames of
                      a step, H*W bytes per env, and trl_frame_stack_push_u8 keeps the k-stacks on the device: FrameStack
                      (env/atari_wrapper.py:198-227) without the host-side concatenation and with 1/k of the upload.
                      `reset()` and the reset of single envs fill a stack with k copies of the first frame (:214-218).
      whole stacks    the envs return (C, H, W), stacked by themselves, and there is no `frame_stack`: the stacks are
                      uploaded as they come; the kernel is not used.

    Host round trips of a step, as in `HostEnvBridge.host_step / host_partial_reset`: actions D2H; frames, rewards, dones
    and `time_limit` H2D; the reset mask D2H; the reset frames of the masked envs H2D.

    Stored `next_obs` is the env's own post-step stack: the `alias_reset_obs` of the flat host path (the reference's
    VecEnv writes the reset observation into the array `step` returned, so its ring rows of reset envs hold the RESET
    observation) is NOT reproduced for frames -- the same as `SynthFrameVecEnv`, and the only thing the
    frame-deduplicating buffer can store (a row's next_obs is its obs shifted by the one appended frame).

    `clip_rewards=True` (default: the attribute the factory left on the VecEnv): in training mode the collector sees and
    stores sign(reward), the reference's ClipRewardEnv (atari_wrapper.py:125-131); in evaluation mode rewards pass as
    they are (evaluation returns are the task's own, as with `reward_scale` on the device envs)."""
    is_device_env = False
    is_host_env = True
    kind = "frames"

    def __init__(self, venv, device, frame_stack=None, clip_rewards=None):
        self.venv = venv
        self.env_nums = int(venv.env_nums)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("collectors run their networks on the GPU: pass device='cuda:<n>'")
        if frame_stack is None:
            frame_stack = getattr(venv, "frame_stack", 0)
        if clip_rewards is None:
            clip_rewards = getattr(venv, "clip_rewards", False)
        k = 4 if frame_stack is True else int(frame_stack or 0)
        if k < 0:
            raise ValueError("HostFrameBridge: frame_stack must be a positive stack depth (or True for 4), got %r" % (frame_stack,))
        self.frame_stack, self.clip_rewards = k, bool(clip_rewards)
        space, act_space = venv.observation_space, venv.action_space
        shape = tuple(int(v) for v in (getattr(space, "shape", None) or ()))
        try:
            dtype = np.dtype(getattr(space, "dtype", None))
        except TypeError:
            dtype = None
        if dtype != np.uint8:
            raise ValueError("HostFrameBridge drives envs with uint8 image observations, got dtype %r (shape %r)"
                             % (getattr(space, "dtype", None), shape))
        single = len(shape) == 2 or (len(shape) == 3 and shape[0] == 1)
        if k and not single:
            raise ValueError("HostFrameBridge(frame_stack=%d) stacks single frames, (H, W) or (1, H, W); the envs return %r "
                             "-- envs that stack their frames themselves are bridged without frame_stack" % (k, shape))
        if not k and len(shape) != 3:
            raise ValueError("HostFrameBridge without frame_stack takes whole (C, H, W) stacks; the envs return %r "
                             "-- pass frame_stack=k for envs that return single frames" % (shape,))
        H, W = shape[-2], shape[-1]
        if H * W <= 0 or (H * W) % 16 != 0:
            raise ValueError("HostFrameBridge: the frame kernels copy 16-byte vectors, H * W must be a positive multiple of "
                             "16; got %d x %d = %d" % (H, W, H * W))
        if not hasattr(act_space, "n"):
            raise ValueError("HostFrameBridge drives envs with Discrete actions (a Q network picks one), got %r" % (act_space,))
        self.frame_shape = (k if k else shape[0], H, W)
        self.action_num = int(act_space.n)
        from gym import spaces
        self._observation_space = spaces.Box(0, 255, self.frame_shape, dtype=np.uint8)
        n, dev = self.env_nums, self.device
        self.cur_obs = torch.zeros((n,) + self.frame_shape, dtype=torch.uint8, device=dev)
        self.cur_step = torch.zeros(n, dtype=torch.int32, device=dev)
        self.ep_return = torch.zeros(n, device=dev)
        self._reward_scale = 1                                            # (the collectors set it; host rewards are not scaled)
        self.training = True
        self.horizon = int(getattr(venv, "_max_episode_steps", None) or getattr(venv, "horizon", None) or 0)
        # what one env uploads per step: the new frame, or the whole stack
        self._per_env = H * W if k else self.frame_shape[0] * H * W
        self._frame_stager = _C.PinnedStager(n * self._per_env, torch.uint8)
        self._scalar_stager = _C.PinnedStager(3 * n, torch.float32)     # rewards | dones | time_limits of a step
        self._frames_dev = torch.zeros(n, H * W, dtype=torch.uint8, device=dev) if k else None
        self._ones = torch.ones(n, dtype=torch.uint8, device=dev) if k else None
        self.h2d_bytes = 0                                                # uploaded so far (frames and scalars)

    # ---- the reference protocol, with device observations ----
    @property
    def observation_space(self):
        return self._observation_space

    @property
    def action_space(self):
        return self.venv.action_space

    def train(self):
        self.training = True
        self.venv.train()

    def eval(self):
        self.training = False
        self.venv.eval()

    def close(self):
        self.venv.close()

    def render(self):
        self.venv.render()

    def seed(self, seed):
        self.venv.seed(seed)

    def _upload_frames(self, obs, rows=None):
        """Host frames (single-frame mode) or stacks of the envs in `rows` (index array; None: all) -> `cur_obs`; one
        upload and, in single-frame mode, one push launch per run of consecutive envs.  rows given = a reset: the stacks
        of those envs are FILLED with their frame, the others stay as they are."""
        n, per = self.env_nums, self._per_env
        obs = np.asarray(obs)
        if obs.dtype != np.uint8 or obs.size != n * per:
            raise ValueError("HostFrameBridge: the envs returned %s %r, expected uint8 frames of %d bytes for each of %d envs"
                             % (obs.dtype, obs.shape, per, n))
        obs = obs.reshape(n, per)
        if rows is None:
            runs = [(0, n)]
        else:
            rows = np.asarray(rows)
            cuts = np.flatnonzero(np.diff(rows) != 1) + 1
            runs = [(int(r[0]), int(r[-1]) + 1) for r in np.split(rows, cuts)]
        host = self._frame_stager.stage().numpy().reshape(n, per)
        for a, b in runs:
            host[a:b] = obs[a:b]
        dst = self._frames_dev if self.frame_stack else self.cur_obs
        self._frame_stager.upload_parts([(dst[a:b], a * per, b * per) for a, b in runs])
        self.h2d_bytes += sum(b - a for a, b in runs) * per
        if self.frame_stack:
            for a, b in runs:
                _C.frame_stack_push(self.cur_obs[a:b], self._frames_dev[a:b], None if rows is None else self._ones[a:b])

    def reset(self, **kwargs):
        obs = self.venv.reset(**kwargs)
        if self.frame_stack:
            self._upload_frames(obs, rows=np.arange(self.env_nums))      # k copies of every env's first frame
        else:
            self._upload_frames(obs)
        self.cur_step.zero_()
        self.ep_return.zero_()
        return self.cur_obs

    # ---- the two host round trips of a collector step ----
    def host_step(self, act, next_obs, rewards, dones, time_limits=None):
        """act (N,) int64 device -> envs; `cur_obs` becomes the post-step stacks (copied to the ring row `next_obs` when
        given); fills the device rows rewards, dones (, time_limits) (N, 1)."""
        n = self.env_nums
        a = act.detach().cpu().numpy().reshape(-1).astype(np.int64)
        obs, rew, done, infos = self.venv.step(a)
        self._upload_frames(obs)
        if next_obs is not None:
            next_obs.copy_(self.cur_obs)
        rew = np.asarray(rew, dtype=np.float64).reshape(n)
        if self.training and self.clip_rewards:
            rew = np.sign(rew)
        host = self._scalar_stager.stage().numpy()
        host[:n] = rew
        host[n:2 * n] = np.asarray(done).reshape(n)
        tl = infos.get("time_limit") if isinstance(infos, dict) else None
        host[2 * n:] = np.asarray(tl).reshape(n) if tl is not None and len(tl) == n else 0.0   # collector/base.py:213-215
        parts = [(rewards, 0, n), (dones, n, 2 * n)]
        if time_limits is not None:
            parts.append((time_limits, 2 * n, 3 * n))
        self._scalar_stager.upload_parts(parts)
        self.h2d_bytes += 4 * n * len(parts)
        return done

    def host_partial_reset(self, mask):
        """mask (N,) uint8 device: reset those envs; their stacks in `cur_obs` become the reset stacks (single-frame mode:
        k copies of the first frame), the other envs' stay."""
        m = mask.cpu().numpy().astype(bool)
        if m.any():
            self._upload_frames(self.venv.partial_reset(m), rows=np.flatnonzero(m))
        return m
