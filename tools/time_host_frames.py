"""Collection from host pixel envs, timed (profiles/NOTES_host_frames.md): wall time per vector step of `VecCollector` on
`PyCatch-v0` at N = 16 in single-frame mode (HostFrameBridge keeps the stacks on the device) and in whole-stack mode (the
same env behind a host-side FrameStack), split into host env time, the host round trips, the wait for the device and the
rest (launch issue); the flat host path (`PyCartPole-v0`, MLP Q-network) beside it; H2D bytes per step.  Every wall time is
a host clock around work that ends in a device synchronise; the split comes from one more rollout with a synchronise in
front of each round trip (so it sums to a little more than the wall time).

    python tools/time_host_frames.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torchrl.networks as networks                       # noqa: E402
import torchrl.policies as policies                       # noqa: E402
from torchrl.collector import VecCollector                # noqa: E402
from torchrl.env import HostFrameBridge, VecEnv, get_vec_env   # noqa: E402
from torchrl.env.py_envs import CatchEnv                  # noqa: E402
from torchrl.replay_buffers import BaseReplayBuffer       # noqa: E402

DEV = torch.device("cuda:0")
N, STEPS, REPS = 16, 200, 5
CONVS = [[16, [8, 8], [4, 4], [0, 0]], [32, [4, 4], [2, 2], [0, 0]], [64, [3, 3], [1, 1], [0, 0]]]


class StackedCatch(CatchEnv):
    """CatchEnv behind a host-side FrameStack(4): whole (4, 84, 84) stacks leave the env."""

    def __init__(self, seed=0):
        super().__init__(seed)
        from gym import spaces
        self.observation_space = spaces.Box(0, 255, (4, 84, 84), dtype=np.uint8)
        self._frames = []

    def reset(self):
        f = super().reset()
        self._frames = [f] * 4
        return np.stack(self._frames)

    def step(self, action):
        f, r, d, info = super().step(action)
        self._frames = self._frames[1:] + [f]
        return np.stack(self._frames), r, d, info


class Timers(dict):
    def wrap(self, obj, name, key, sync_first=False):
        fn = getattr(obj, name)

        def timed(*a, **k):
            if sync_first:
                t0 = time.perf_counter()
                torch.cuda.synchronize()
                self["gpu_wait"] = self.get("gpu_wait", 0.0) + time.perf_counter() - t0
            t0 = time.perf_counter()
            out = fn(*a, **k)
            self[key] = self.get(key, 0.0) + time.perf_counter() - t0
            return out
        setattr(obj, name, timed)


def frame_collector(mode):
    if mode == "single":
        env, ev = get_vec_env("PyCatch-v0", {"frame_stack": True, "clip_rewards": True}, N), get_vec_env("PyCatch-v0", {"frame_stack": True}, N)
    else:
        env, ev = VecEnv(N, StackedCatch, ()), VecEnv(N, StackedCatch, ())
    env.seed(0)
    torch.manual_seed(0)
    qf = networks.Net(output_shape=3, base_type=networks.CNNBase, append_hidden_shapes=[512], activation_func=torch.nn.Tanh,
                      input_shape=(4, 84, 84), hidden_shapes=CONVS)
    pf = policies.EpsilonGreedyDQNDiscretePolicy(qf=qf, start_epsilon=1, end_epsilon=0.1, decay_frames=3000, action_shape=3)
    buf = BaseReplayBuffer(N * 256, env_nums=N)
    return VecCollector(env=env, eval_env=ev, pf=pf, replay_buffer=buf, device=DEV, epoch_frames=N * STEPS,
                        max_episode_frames=999, eval_episodes=1)


def flat_collector():
    env, ev = get_vec_env("PyCartPole-v0", {}, N), get_vec_env("PyCartPole-v0", {}, N)
    env.seed(0)
    torch.manual_seed(0)
    qf = networks.Net(input_shape=4, output_shape=2, hidden_shapes=[128, 128, 128], append_hidden_shapes=[],
                      base_type=networks.MLPBase, activation_func=torch.nn.ReLU)
    pf = policies.EpsilonGreedyDQNDiscretePolicy(qf, start_epsilon=1, end_epsilon=0.1, decay_frames=3000, action_shape=2)
    buf = BaseReplayBuffer(N * 256, env_nums=N)
    return VecCollector(env=env, eval_env=ev, pf=pf, replay_buffer=buf, device=DEV, epoch_frames=N * STEPS,
                        max_episode_frames=999, eval_episodes=1)


def wall_per_step(col):
    col.rollout(STEPS)                                                   # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        col.rollout(STEPS)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / STEPS * 1e6)
    return {"median_us": float(np.median(out)), "min_us": float(min(out)), "max_us": float(max(out))}


def split_per_step(col, frames):
    """One more rollout with timers around the pieces (a device synchronisation in front of each host round trip, so that
    waiting for the launches is not booked under the copy)."""
    env, t = col.env, Timers()
    t.wrap(env.venv, "step", "host_env")
    t.wrap(env.venv, "partial_reset", "host_env")
    if frames:
        t.wrap(env, "_upload_frames", "h2d_frames_and_push_issue")
        t.wrap(env._scalar_stager, "upload_parts", "h2d_scalars_issue")
    else:
        t.wrap(env, "_upload", "h2d_issue")
    t.wrap(env, "host_step", "host_step_total", sync_first=True)
    t.wrap(env, "host_partial_reset", "partial_reset_total", sync_first=True)
    np.random.seed(0)
    t0 = time.perf_counter()
    col.rollout(STEPS)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    us = {k: v / STEPS * 1e6 for k, v in t.items()}
    inner = sum(v for k, v in us.items() if k.startswith("h2d") or k == "host_env")
    us["d2h_actions_and_mask"] = us["host_step_total"] + us["partial_reset_total"] - inner
    us["host_side_launch_issue_rest"] = total / STEPS * 1e6 - us["host_step_total"] - us["partial_reset_total"] - us["gpu_wait"]
    us["total_instrumented"] = total / STEPS * 1e6
    return us


def main():
    res = {"N": N, "steps": STEPS, "device": torch.cuda.get_device_name(0)}
    for mode in ("single", "stacks"):
        col = frame_collector(mode)
        assert isinstance(col.env, HostFrameBridge) and col.env.frame_stack == (4 if mode == "single" else 0)
        np.random.seed(0)
        wall = wall_per_step(col)
        b0 = col.env.h2d_bytes
        split = split_per_step(col, True)
        res["catch_" + mode] = {"wall": wall, "split_us": split, "h2d_bytes_per_step": (col.env.h2d_bytes - b0) / STEPS,
                                "h2d_frame_bytes_per_env_step": col.env._per_env}
        col.terminate()
    col = flat_collector()
    np.random.seed(0)
    res["cartpole_flat"] = {"wall": wall_per_step(col), "split_us": split_per_step(col, False)}
    col.terminate()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
