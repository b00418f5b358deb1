"""Numpy restatement of collection from host pixel envs -- TEST INFRASTRUCTURE ONLY (tests/test_host_frames_*.py).

`ScriptedFrameEnv` is a host env with the gym interface whose frames encode (env, episode, t), so that any mix-up of
envs, episodes or stack order shows as a wrong byte.  `replay` walks the reference's vector collection loop
(torchrl/collector/base.py:184-230: step, count, reset where done or over length) over such envs with given actions
and keeps the k-stacks with `oracle.frames.FrameStackOracle` (pinned to the reference's FrameStack by
tests/golden/frame_dedup.npz).  The stored `next_obs` is the env's own post-step stack (HostFrameBridge's contract).
"""
import numpy as np

from oracle.frames import FrameStackOracle


def scripted_frame(env, episode, t, shape):
    """Every byte depends on (env, episode, t) and on its position; the first three bytes spell the triple."""
    h, w = shape
    f = ((np.arange(h * w, dtype=np.int64) * 7 + env * 37 + episode * 11 + t * 5) % 251).astype(np.uint8)
    f[:3] = (env, episode, t)
    return f.reshape(h, w)


class ScriptedFrameEnv:
    """Episode of `length` steps; reward = action + t / 4 - env (exact in float32); `done` at t == length, reported as a
    time limit in odd episodes.  stacked=k: the env keeps its own FrameStack and returns (k, H, W) stacks; with
    `channel=True` single frames come as (1, H, W) instead of (H, W)."""

    def __init__(self, index, length, shape=(84, 84), actions=3, stacked=0, channel=False):
        from gym import spaces
        self.index, self.length, self.shape, self.stacked, self.channel = int(index), int(length), tuple(shape), int(stacked), channel
        obs_shape = (self.stacked,) + self.shape if self.stacked else ((1,) + self.shape if channel else self.shape)
        self.observation_space = spaces.Box(0, 255, obs_shape, dtype=np.uint8)
        self.action_space = spaces.Discrete(actions)
        self.episode, self.t, self.taken = -1, 0, []                     # taken: every action this env was stepped with
        self._stack = FrameStackOracle(self.stacked) if self.stacked else None

    def _frame(self):
        f = scripted_frame(self.index, self.episode, self.t, self.shape)
        return f[None] if (self.stacked or self.channel) else f

    def reset(self):
        self.episode += 1
        self.t = 0
        f = self._frame()
        return np.asarray(self._stack.reset(f)) if self.stacked else f

    def step(self, action):
        self.t += 1
        self.taken.append(int(action))
        f = self._frame()
        done = self.t >= self.length
        reward = float(int(action)) + self.t / 4.0 - self.index
        ob = np.asarray(self._stack.step(f)) if self.stacked else f
        return ob, reward, done, {"time_limit": bool(done and self.episode % 2 == 1)}


def replay(envs, acts, k, max_episode_frames, clip_rewards=False):
    """envs: fresh single-frame ScriptedFrameEnv objects (not yet reset); acts (steps, N) ints.  Returns the ring
    contents in step order -- obs / next_obs (steps, N, k, H, W) uint8, rewards / terminals / time_limits (steps, N, 1)
    float32 --, the final stacks `cur_obs`, the episode log [(step, env, return)] in the collector's order and the summed
    reward.  The running return of an env is cleared when it reports done, not at an over-length reset (base.py:199-228)."""
    acts = np.asarray(acts)
    steps, n = acts.shape
    stacks = [FrameStackOracle(k) for _ in envs]
    cur = [np.asarray(s.reset(_chw(e.reset()))) for s, e in zip(stacks, envs)]
    out = {key: [] for key in ("obs", "next_obs", "rewards", "terminals", "time_limits")}
    count, ret, log, total = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float32), [], 0.0
    for t in range(steps):
        rows = {key: [] for key in out}
        for i, (env, stack) in enumerate(zip(envs, stacks)):
            frame, rew, done, info = env.step(acts[t, i])
            if clip_rewards:
                rew = float(np.sign(rew))
            nxt = np.asarray(stack.step(_chw(frame)))
            rows["obs"].append(cur[i])
            rows["next_obs"].append(nxt)
            rows["rewards"].append([rew])
            rows["terminals"].append([float(done)])
            rows["time_limits"].append([float(info["time_limit"])])
            total += rew
            count[i] += 1
            ret[i] += np.float32(rew)
            if done:
                log.append((t, i, float(ret[i])))
                ret[i] = 0.0
            if done or count[i] >= max_episode_frames:
                nxt = np.asarray(stack.reset(_chw(env.reset())))
                count[i] = 0
            cur[i] = nxt
        for key in out:
            out[key].append(np.stack(rows[key]) if key in ("obs", "next_obs") else np.array(rows[key], dtype=np.float32))
    res = {key: np.stack(v) for key, v in out.items()}
    res.update(cur_obs=np.stack(cur), episodes=log, total=total)
    return res


def _chw(frame):
    frame = np.asarray(frame)
    return frame[None] if frame.ndim == 2 else frame
