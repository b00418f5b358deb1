"""Env factories with the reference's signatures (torchrl/env/get_env.py:39-87).

The synthetic on-GPU ids (no gym / MuJoCo / ALE in the image, and real physics is not the benchmark) plus three
pure-Python host tasks (`PyPendulum-v0`, `PyCartPole-v0` and the pixel task `PyCatch-v0`) behind `VecEnv` /
`SubProcVecEnv`."""
from .base_wrapper import NormObs
from .py_envs import CartPoleEnv, CatchEnv, PendulumEnv
from .subproc_vecenv import SubProcVecEnv
from .synth import SynthVecEnv, SynthFrameVecEnv, SYNTH_IDS, SYNTH_FRAME_IDS
from .vecenv import VecEnv, is_pixel_space

# pure-Python tasks stepped on the host (the reference's gym ids are not installable here)
HOST_IDS = {"PyPendulum-v0": PendulumEnv, "PyCartPole-v0": CartPoleEnv, "PyCatch-v0": CatchEnv}


def _host_vec_env(venv, env_param):
    """A pixel host id takes the reference's wrap_deepmind keys (env/atari_wrapper.py:230-247): the VecEnv carries them to
    the bridge the collector wraps it in (torchrl_amd.env.HostFrameBridge).  `frame_stack`: stacks of 4, held on the
    device; `clip_rewards`: sign(reward) while training; `scale`: accepted -- the /255 - 0.5 of ScaledFloatFrame lives in
    the first conv layer (see SynthFrameVecEnv)."""
    if is_pixel_space(venv.observation_space):
        venv.frame_stack = 4 if env_param.get("frame_stack", False) else 0
        venv.clip_rewards = bool(env_param.get("clip_rewards", False))
    return venv


def _check(env_id, env_param):
    if env_id not in SYNTH_IDS and env_id not in SYNTH_FRAME_IDS and env_id not in HOST_IDS:
        raise ValueError("unknown env id %r: torchrl_amd ships the synthetic ids %s and the host ids %s"
                         % (env_id, sorted(SYNTH_IDS) + sorted(SYNTH_FRAME_IDS), sorted(HOST_IDS)))
    if "rew_norm" in env_param:
        raise NotImplementedError("rew_norm (NormRet wrapper) is not built")


def get_vec_env(env_id, env_param, vec_env_nums, device=None, index_offset=0, total_env_nums=None):
    _check(env_id, env_param)
    if env_id in HOST_IDS:                                   # host Python envs: the collectors bridge them to the device
        if env_param.get("obs_norm", False):
            raise NotImplementedError("obs_norm on host ids: wrap NormObs(HostEnvBridge(env, device)) explicitly")
        return _host_vec_env(VecEnv(vec_env_nums, HOST_IDS[env_id], ()), env_param)
    if env_id in SYNTH_FRAME_IDS:
        return SynthFrameVecEnv(vec_env_nums, reward_scale=env_param.get("reward_scale", 1), device=device,
                                index_offset=index_offset, total_env_nums=total_env_nums, **SYNTH_FRAME_IDS[env_id])
    env = SynthVecEnv(vec_env_nums, reward_scale=env_param.get("reward_scale", 1), device=device,
                      index_offset=index_offset, total_env_nums=total_env_nums, **SYNTH_IDS[env_id])
    if env_param.get("obs_norm", False):                     # env/get_env.py:75-76
        env = NormObs(env)
    return env


def get_subprocvec_env(env_id, env_param, vec_env_nums, proc_nums, **kwargs):
    """Host ids: the envs are stepped in `proc_nums` spawned worker processes (env/subproc_vecenv.py); the synthetic
    ids live on the GPU, where process-parallel stepping is what the kernels replace."""
    _check(env_id, env_param)
    if env_id in HOST_IDS:
        return _host_vec_env(SubProcVecEnv(proc_nums, vec_env_nums, HOST_IDS[env_id], ()), env_param)
    return get_vec_env(env_id, env_param, vec_env_nums, **kwargs)


def get_env(env_id, env_param, **kwargs):
    return get_vec_env(env_id, env_param, 1, **kwargs)
