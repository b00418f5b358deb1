"""Host pixel envs, the parts that need no GPU: the `PyCatch-v0` task, its factories, `VecEnv` against `SubProcVecEnv`
over it, and the numpy restatement the GPU tests compare the collectors with (tests/_host_frames_ref.py)."""
from fractions import Fraction

import numpy as np
import pytest

from tests._host_frames_ref import ScriptedFrameEnv, replay, scripted_frame


def _episode(seed, action):
    from torchrl.env.py_envs import CatchEnv
    env = CatchEnv(seed)
    frames, rewards, dones, infos = [env.reset()], [], [], []
    for _ in range(40):
        f, r, d, info = env.step(action)
        frames.append(f)
        rewards.append(r)
        dones.append(d)
        infos.append(info)
        if d:
            break
    return frames, rewards, dones, infos


def test_catch_frames_episode_length_and_determinism():
    from torchrl.env.py_envs import CatchEnv
    a, b = _episode(7, 2), _episode(7, 2)
    assert len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    assert a[1] == b[1] and a[2] == b[2]
    frames, rewards, dones, infos = a
    assert len(rewards) == 20 and dones == [False] * 19 + [True] and CatchEnv._max_episode_steps == 20
    assert rewards[:19] == [0.0] * 19 and rewards[19] in (1.0, -1.0)
    assert all(info == {"time_limit": False} for info in infos)
    env = CatchEnv(7)
    assert env.observation_space.shape == (84, 84) and np.dtype(env.observation_space.dtype) == np.uint8
    assert env.action_space.n == 3
    col = int(np.random.RandomState(7).randint(0, 21))                    # the ball's column: the env's own stream
    for t, f in enumerate(frames):
        assert f.shape == (84, 84) and f.dtype == np.uint8 and set(np.unique(f)) <= {0, 128, 255}
        ball = np.argwhere(f == 255)
        assert len(ball) == 16 and ball.min(0).tolist() == [4 * t, 4 * col] and ball.max(0).tolist() == [4 * t + 3, 4 * col + 3]
    first = frames[0]
    assert (first[80:, 36:48] == 128).all() and (first == 128).sum() == 4 * 12     # three cells, centred (cells 9..11)
    assert not np.array_equal(_episode(8, 2)[0][0], first) or np.random.RandomState(8).randint(0, 21) == col


def test_catch_reward_sign_for_constant_actions():
    """By hand: the paddle's centre starts in cell 10 and is kept in 1..19.  Always left: cell 1 after 9 steps, covering
    columns 0..2; always stay: 9..11; always right: 18..20.  +1 exactly when the ball's column is covered."""
    covered = {0: {0, 1, 2}, 1: {9, 10, 11}, 2: {18, 19, 20}}
    caught = {0: 0, 1: 0, 2: 0}
    for seed in range(60):
        col = int(np.random.RandomState(seed).randint(0, 21))
        for action in (0, 1, 2):
            want = 1.0 if col in covered[action] else -1.0
            assert _episode(seed, action)[1][-1] == want, (seed, col, action)
            caught[action] += want > 0
    assert all(v > 0 for v in caught.values()), caught                     # every action's +1 case occurred


def test_random_policy_expected_return_by_enumeration():
    """The exact expected return of the uniformly random policy, the yardstick of profiles/NOTES_host_frames.md: the
    paddle's distribution after 20 uniform moves (kept in 1..19) against a uniform ball column.  The paddle always covers
    3 of the 21 columns, whatever it does, so a policy that ignores the ball catches with probability 1/7: return -5/7."""
    dist = {10: Fraction(1)}
    for _ in range(20):
        nxt = {}
        for x, p in dist.items():
            for d in (-1, 0, 1):
                y = min(19, max(1, x + d))
                nxt[y] = nxt.get(y, 0) + p / 3
        dist = nxt
    p_catch = sum(p * sum(1 for c in range(21) if abs(c - x) <= 1) for x, p in dist.items()) / 21
    assert p_catch == Fraction(1, 7) and 2 * p_catch - 1 == Fraction(-5, 7)


def test_vecenv_and_subprocvecenv_agree_on_catch():
    from torchrl.env import get_subprocvec_env, get_vec_env
    n, steps = 4, 45                                                      # two episode ends inside
    rs = np.random.RandomState(3)
    script = rs.randint(0, 3, size=(steps, n))
    runs = []
    for make in (lambda: get_vec_env("PyCatch-v0", {}, n), lambda: get_subprocvec_env("PyCatch-v0", {}, n, 2)):
        env = make()
        try:
            env.seed(5)
            seq = [env.reset().copy()]
            for t in range(steps):
                obs, rew, done, info = env.step(script[t])
                seq += [obs.copy(), rew.copy(), done.copy(), np.asarray(info["time_limit"]).copy()]
                if done.any():
                    seq.append(env.partial_reset(done.reshape(-1)).copy())
            runs.append(seq)
        finally:
            env.close()
    assert len(runs[0]) == len(runs[1]) > 4 * steps + 1
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert runs[0][0].shape == (n, 84, 84) and runs[0][0].dtype == np.uint8


def test_factory_returns_a_host_vecenv_carrying_the_wrapper_settings():
    from torchrl.env import VecEnv, get_vec_env
    from torchrl.env.get_env import HOST_IDS
    from torchrl.env.py_envs import CatchEnv
    assert HOST_IDS["PyCatch-v0"] is CatchEnv
    env = get_vec_env("PyCatch-v0", {"frame_stack": True, "clip_rewards": True, "scale": True}, 3)
    assert isinstance(env, VecEnv) and env.env_nums == 3 and not env.is_device_env
    assert env.frame_stack == 4 and env.clip_rewards is True
    assert env.observation_space.shape == (84, 84) and env.action_space.n == 3 and env._max_episode_steps == 20
    plain = get_vec_env("PyCatch-v0", {}, 2)
    assert plain.frame_stack == 0 and plain.clip_rewards is False
    flat = get_vec_env("PyCartPole-v0", {}, 2)                             # flat host ids carry no pixel settings
    assert "frame_stack" not in vars(flat)
    with pytest.raises(NotImplementedError):
        get_vec_env("PyCatch-v0", {"rew_norm": True}, 2)


def test_restatement_against_a_hand_written_example():
    """One env (index 0), two-step episodes, stacks of two, actions 1, 2, 0: the second step ends the episode."""
    F = lambda ep, t: scripted_frame(0, ep, t, (4, 8))
    res = replay([ScriptedFrameEnv(0, 2, shape=(4, 8))], [[1], [2], [0]], 2, 999)
    want_obs = [[F(0, 0), F(0, 0)], [F(0, 0), F(0, 1)], [F(1, 0), F(1, 0)]]        # the reset fills with the first frame
    want_next = [[F(0, 0), F(0, 1)], [F(0, 1), F(0, 2)], [F(1, 0), F(1, 1)]]       # ... and next_obs of step 1 is pre-reset
    assert res["obs"].shape == (3, 1, 2, 4, 8) and res["obs"].dtype == np.uint8
    assert np.array_equal(res["obs"][:, 0], np.array(want_obs)) and np.array_equal(res["next_obs"][:, 0], np.array(want_next))
    assert res["rewards"].reshape(-1).tolist() == [1.25, 2.5, 0.25]
    assert res["terminals"].reshape(-1).tolist() == [0.0, 1.0, 0.0] and res["time_limits"].reshape(-1).tolist() == [0.0] * 3
    assert np.array_equal(res["cur_obs"][0], np.array([F(1, 0), F(1, 1)]))
    assert res["episodes"] == [(1, 0, 3.75)] and res["total"] == 4.0
    assert F(1, 1).reshape(-1)[:3].tolist() == [0, 1, 1] and not np.array_equal(F(0, 1), F(1, 1))
    # over-length reset: max_episode_frames = 2 in a five-step episode -- a reset with terminals False, the return runs on
    res = replay([ScriptedFrameEnv(1, 5, shape=(4, 8))], [[0], [0], [0]], 2, 2)
    G = lambda ep, t: scripted_frame(1, ep, t, (4, 8))
    assert res["terminals"].reshape(-1).tolist() == [0.0] * 3 and res["episodes"] == []
    assert np.array_equal(res["next_obs"][1, 0], np.array([G(0, 1), G(0, 2)]))
    assert np.array_equal(res["obs"][2, 0], np.array([G(1, 0), G(1, 0)]))
    # an env that stacks for itself returns the same stacks the restatement keeps
    env = ScriptedFrameEnv(0, 2, shape=(4, 8), stacked=2)
    assert np.array_equal(env.reset(), np.array(want_obs[0])) and np.array_equal(env.step(1)[0], np.array(want_next[0]))
    ob, rew, done, info = env.step(2)
    assert np.array_equal(ob, np.array(want_next[1])) and done and rew == 2.5 and info == {"time_limit": False}
