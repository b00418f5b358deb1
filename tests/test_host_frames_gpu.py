"""Host pixel envs under the device collectors: the device-side FrameStack kernel (trl_frame_stack_push_u8) against
numpy, byte for byte; `VecCollector` over `HostFrameBridge` against the numpy restatement of the reference's loop
(tests/_host_frames_ref.py) in single-frame mode (the kernel keeps the stacks) and whole-stack mode; the
frame-deduplicating buffer over such a rollout; greedy evaluation; DQN / QR-DQN on `PyCatch-v0`."""
import numpy as np
import pytest
import torch

from tests._host_frames_ref import ScriptedFrameEnv, replay

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (3, 5, 7)                                                       # episode lengths: the envs are out of step
STEPS = 12


# ---------------------------------------------------------------- the kernel
def _push_ref(stacks, frames, mask):
    for n in range(stacks.shape[0]):
        if mask is not None and mask[n]:
            stacks[n, :] = frames[n]                                      # FrameStack.reset: k copies
        else:
            stacks[n, :-1] = stacks[n, 1:].copy()                         # FrameStack.step: drop the oldest, append
            stacks[n, -1] = frames[n]


@pytest.mark.parametrize("HW", [16, 4112, 7056])      # one vector | 257 vectors: one thread's second trip | 84 x 84
@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("N", [1, 2, 65])
def test_frame_stack_push_equals_numpy(N, C, HW):
    from torchrl_amd import _C
    rs = np.random.RandomState(N * 1000 + C * 100 + HW % 97)
    pad, size = 64, N * C * HW
    for kind in ("none", "zero", "one", "alternating"):
        host = rs.randint(0, 256, size=pad + size + pad).astype(np.uint8)
        raw = torch.tensor(host, device=DEV)
        stacks = raw[pad:pad + size].view(N, C, HW)                       # canary bytes on both sides
        want = host[pad:pad + size].reshape(N, C, HW).copy()
        for push in range(6):                                             # six pushes in place: C = 4 turns over fully
            frames = rs.randint(0, 256, size=(N, HW)).astype(np.uint8)
            mask = {"none": None, "zero": np.zeros(N, np.uint8), "one": np.ones(N, np.uint8),
                    "alternating": ((np.arange(N) + push) % 2).astype(np.uint8)}[kind]
            _C.frame_stack_push(stacks, torch.tensor(frames, device=DEV), None if mask is None else torch.tensor(mask, device=DEV))
            _push_ref(want, frames, mask)
            assert np.array_equal(stacks.cpu().numpy(), want), (kind, push)
        got = raw.cpu().numpy()
        assert np.array_equal(got[:pad], host[:pad]) and np.array_equal(got[pad + size:], host[pad + size:]), kind


def test_frame_stack_push_refuses_bad_arguments():
    import ctypes
    from torchrl_amd import _C
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=DEV)
    with pytest.raises(_C.TrlError, match="multiple of 16"):
        _C.frame_stack_push(u8(2, 4, 24), u8(2, 24))
    with pytest.raises(_C.TrlError, match="bad sizes"):
        _C.frame_stack_push(u8(2, 0, 16), u8(2, 16))                       # C = 0
    with pytest.raises(_C.TrlError, match="frames"):
        _C.frame_stack_push(u8(2, 4, 16), u8(3, 16))
    with pytest.raises(_C.TrlError, match="fill_mask"):
        _C.frame_stack_push(u8(2, 4, 16), u8(2, 16), u8(3))
    with pytest.raises(_C.TrlError, match="dtype"):
        _C.frame_stack_push(u8(2, 4, 16).float(), u8(2, 16))
    with pytest.raises(_C.TrlError, match="no CPU path"):
        _C.frame_stack_push(torch.zeros(2, 4, 16, dtype=torch.uint8), u8(2, 16))
    st = u8(1, 1, 16)
    code = _C.lib().trl_frame_stack_push_u8(ctypes.c_void_p(st.data_ptr()), None, None, 1, 1, 16, _C.stream_ptr(st.device))
    with pytest.raises(_C.TrlError, match="null pointer"):
        _C.check(code, "trl_frame_stack_push_u8")
    # no envs: nothing is launched, nothing is read
    assert _C.lib().trl_frame_stack_push_u8(None, None, None, 0, 4, 16, _C.stream_ptr(st.device)) == 0


# ---------------------------------------------------------------- collection
def _venv(mode):
    """frames: (H, W) single frames; frames1: (1, H, W); stacks: the envs stack four frames themselves."""
    from torchrl.env import VecEnv
    args = [(i, LENGTHS[i], (84, 84), 3, 4 if mode == "stacks" else 0, mode == "frames1") for i in range(len(LENGTHS))]
    return VecEnv(len(LENGTHS), [ScriptedFrameEnv] * len(LENGTHS), args)


def _collect(mode, max_frames, buf_cls=None, **buf_kw):
    from torchrl.collector import VecCollector
    from torchrl.env import HostFrameBridge
    from torchrl.policies import EpsilonGreedyDQNDiscretePolicy
    from torchrl.replay_buffers import BaseReplayBuffer
    from tests.test_dqn_gpu import small_qnet
    N = len(LENGTHS)
    env, eval_env = _venv(mode), _venv(mode)
    if mode != "stacks":
        env = HostFrameBridge(env, DEV, frame_stack=4)                    # (a plain VecEnv is wrapped by the collector)
        eval_env = HostFrameBridge(eval_env, DEV, frame_stack=4)
    torch.manual_seed(3)
    qf = small_qnet(3).to(DEV)
    pf = EpsilonGreedyDQNDiscretePolicy(qf=qf, start_epsilon=0.9, end_epsilon=0.5, decay_frames=1000, action_shape=3)
    buf = (buf_cls or BaseReplayBuffer)(N * STEPS, env_nums=N, **buf_kw)
    col = VecCollector(env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=torch.device(DEV), epoch_frames=N * STEPS,
                       max_episode_frames=max_frames, eval_episodes=1)
    np.random.seed(17)
    res = col.train_one_epoch()
    return col, buf, res


def _single_frame_envs():
    return [ScriptedFrameEnv(i, LENGTHS[i]) for i in range(len(LENGTHS))]


@pytest.mark.parametrize("max_frames", [999, 4])                         # 4: over-length resets with terminals False
@pytest.mark.parametrize("mode", ["frames", "frames1", "stacks"])
def test_collection_equals_the_host_restatement(mode, max_frames):
    from torchrl.env import HostFrameBridge
    N = len(LENGTHS)
    col, buf, res = _collect(mode, max_frames)
    env = col.env
    assert isinstance(env, HostFrameBridge) and isinstance(col.eval_env, HostFrameBridge)
    assert env.kind == "frames" and env.is_host_env and not env.is_device_env
    assert env.frame_shape == (4, 84, 84) and env.action_num == 3 and env.frame_stack == (0 if mode == "stacks" else 4)
    assert env.observation_space.shape == (4, 84, 84) and np.dtype(env.observation_space.dtype) == np.uint8
    assert env.cur_obs.dtype == torch.uint8 and tuple(env.cur_obs.shape) == (N, 4, 84, 84) and env.cur_obs.is_cuda
    acts = buf._acts.cpu().numpy()[:, :, 0]
    assert acts.shape == (STEPS, N) and set(np.unique(acts)) <= {0.0, 1.0, 2.0}
    ref = replay(_single_frame_envs(), acts.astype(np.int64), 4, max_frames)
    for key in ("obs", "next_obs", "rewards", "terminals", "time_limits"):
        got = getattr(buf, "_" + key).cpu().numpy()
        assert got.dtype == ref[key].dtype and np.array_equal(got, ref[key]), key
    assert np.array_equal(env.cur_obs.cpu().numpy(), ref["cur_obs"])
    assert np.array_equal(np.array(res["train_rewards"], dtype=np.float32), np.array([r for _, _, r in ref["episodes"]], dtype=np.float32))
    assert res["train_epoch_reward"] == ref["total"] and len(ref["episodes"]) >= 2
    assert ref["time_limits"].sum() > 0 or max_frames == 4
    if max_frames == 4:                                                   # resets of envs that did not report done
        fresh = (ref["obs"][1:, :, 3, 0, 2] == 0) & (ref["terminals"][:-1, :, 0] == 0)    # t == 0 after a non-terminal step
        assert fresh.any()
    # bytes uploaded: one frame per env and step (and per reset) against the whole stack
    per = 84 * 84 * (4 if mode == "stacks" else 1)
    resets = N + int((ref["obs"][1:, :, 3, 0, 2] == 0).sum()) + int(ref["cur_obs"][:, 3, 0, 2].tolist().count(0))
    assert env.h2d_bytes == (STEPS * N + resets) * per + STEPS * 3 * N * 4


@pytest.mark.parametrize("mode", ["frames", "stacks"])
def test_dedup_buffer_over_host_frames_equals_the_plain_ring(mode):
    from torchrl.replay_buffers import BaseReplayBuffer, MemoryEfficientReplayBuffer
    N = len(LENGTHS)
    _, plain, r1 = _collect(mode, 4, BaseReplayBuffer)
    _, dedup, r2 = _collect(mode, 4, MemoryEfficientReplayBuffer, min_episode_frames=3)
    assert r1["train_epoch_reward"] == r2["train_epoch_reward"] and list(r1["train_rewards"]) == list(r2["train_rewards"])
    assert not hasattr(dedup, "_obs") and not hasattr(dedup, "_next_obs")
    keys = ["obs", "next_obs", "acts", "rewards", "terminals"]
    for k in range(3):
        np.random.seed(100 + k)
        a = plain.random_batch(N * 4, keys)
        np.random.seed(100 + k)
        b = dedup.random_batch(N * 4, keys)
        for key in keys:
            assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), (k, key)
    idx = torch.arange(STEPS, device=DEV)
    assert torch.equal(dedup._gather("obs", idx), plain._obs.reshape(STEPS * N, 4, 84, 84))
    assert torch.equal(dedup._gather("next_obs", idx), plain._next_obs.reshape(STEPS * N, 4, 84, 84))
    dedup.check_overrun()


def test_eval_one_epoch_returns_first_episodes_and_stops_with_the_last_env():
    col, _, _ = _collect("frames", 4)
    ev = col.eval_one_epoch()
    envs = col.eval_env.venv.envs
    assert [len(e.taken) for e in envs] == [max(LENGTHS)] * len(LENGTHS)   # stopped when the 7-step env had finished
    acts = np.array([e.taken for e in envs]).T
    ref = replay(_single_frame_envs(), acts, 4, 2 ** 31 - 1)
    first = {}
    for step, i, ret in ref["episodes"]:
        first.setdefault(i, (ret, step + 1))
    assert [float(r) for r in ev["eval_rewards"]] == [first[i][0] for i in range(len(LENGTHS))]
    assert [first[i][1] for i in range(len(LENGTHS))] == list(LENGTHS) and ev["eval_traj_length"] == float(np.mean(LENGTHS))
    assert col.eval_env.training is False and col.env.training is True


def test_subproc_vecenv_under_the_bridge_stores_what_vecenv_stores():
    """`SubProcVecEnv` (2 workers) over PyCatch-v0: same ring as `VecEnv`; the eval env the collector deep-copies (a fresh
    SubProcVecEnv object) is bridged with the training env's settings."""
    from torchrl.collector import VecCollector
    from torchrl.env import get_subprocvec_env, get_vec_env
    from torchrl.policies import EpsilonGreedyDQNDiscretePolicy
    from torchrl.replay_buffers import BaseReplayBuffer
    from tests.test_dqn_gpu import small_qnet
    N, steps, rings = 2, 22, []                                           # one episode end inside
    param = {"frame_stack": True, "clip_rewards": True}
    for make in (lambda: get_vec_env("PyCatch-v0", param, N), lambda: get_subprocvec_env("PyCatch-v0", param, N, 2)):
        env = make()
        env.seed(3)
        torch.manual_seed(3)
        pf = EpsilonGreedyDQNDiscretePolicy(qf=small_qnet(3).to(DEV), start_epsilon=0.9, end_epsilon=0.5, decay_frames=1000,
                                            action_shape=3)
        buf = BaseReplayBuffer(N * steps, env_nums=N)
        col = VecCollector(env=env, eval_env=None, pf=pf, replay_buffer=buf, device=torch.device(DEV), epoch_frames=N * steps,
                           max_episode_frames=999, eval_episodes=1)
        try:
            assert col.eval_env.frame_stack == 4 and col.eval_env.clip_rewards and col.eval_env.venv is not env
            np.random.seed(17)
            col.train_one_epoch()
            rings.append({k: getattr(buf, "_" + k).cpu() for k in ("obs", "next_obs", "acts", "rewards", "terminals", "time_limits")})
        finally:
            col.terminate()
    for k in rings[0]:
        assert torch.equal(rings[0][k], rings[1][k]), k
    assert rings[0]["terminals"].sum() == N and rings[0]["obs"].dtype == torch.uint8


# ---------------------------------------------------------------- refusals
class _FakeEnv:
    def __init__(self, shape, dtype, action_space):
        from gym import spaces
        self.observation_space = spaces.Box(0, 255, shape, dtype=dtype)
        self.action_space = action_space

    def reset(self):
        return np.zeros(self.observation_space.shape, dtype=self.observation_space.dtype)


def test_bridge_refuses_what_it_cannot_carry():
    from gym import spaces
    from torchrl.env import HostFrameBridge, VecEnv
    fake = lambda shape, dtype=np.uint8, act=None: VecEnv(2, _FakeEnv, (shape, dtype, act or spaces.Discrete(3)))
    with pytest.raises(ValueError, match="float32"):
        HostFrameBridge(fake((84, 84), np.float32), DEV, frame_stack=4)
    with pytest.raises(ValueError, match="5 x 5 = 25"):
        HostFrameBridge(fake((5, 5)), DEV, frame_stack=4)
    with pytest.raises(ValueError, match="Discrete"):
        HostFrameBridge(fake((84, 84), act=spaces.Box(-1.0, 1.0, (2,))), DEV, frame_stack=4)
    with pytest.raises(ValueError, match=r"\(4, 84, 84\)"):
        HostFrameBridge(fake((4, 84, 84)), DEV, frame_stack=4)             # stacked by the env AND by the bridge
    with pytest.raises(ValueError, match=r"\(84, 84\)"):
        HostFrameBridge(fake((84, 84)), DEV)                               # single frames and nobody stacks them
    with pytest.raises(ValueError, match="cuda"):
        HostFrameBridge(fake((84, 84)), "cpu", frame_stack=4)
    ok = HostFrameBridge(fake((1, 8, 8)), DEV, frame_stack=True)
    assert ok.frame_shape == (4, 8, 8) and torch.equal(ok.reset(), torch.zeros(2, 4, 8, 8, dtype=torch.uint8, device=DEV))


def test_other_collectors_refuse_host_pixel_envs_with_a_clear_error():
    from torchrl.collector import VecCollector
    from torchrl.collector.on_policy import VecOnPolicyCollector
    from torchrl.env import get_vec_env
    from torchrl.policies import EpsilonGreedyDQNDiscretePolicy
    from torchrl.replay_buffers import BaseReplayBuffer
    from torchrl_amd import _C
    from tests.test_dqn_gpu import small_qnet
    make = lambda: get_vec_env("PyCatch-v0", {"frame_stack": True}, 2)
    kw = dict(replay_buffer=BaseReplayBuffer(8, env_nums=2), device=torch.device(DEV), epoch_frames=4, eval_episodes=1)

    class Boot:                                                           # (what marks a Bootstrapped DQN policy)
        head_num = 4
    with pytest.raises(_C.TrlError, match="HostFrameBridge"):
        VecCollector(env=make(), eval_env=make(), pf=Boot(), **kw)
    pf = EpsilonGreedyDQNDiscretePolicy(qf=small_qnet(3), start_epsilon=1, end_epsilon=0.1, decay_frames=10, action_shape=3)
    with pytest.raises(_C.TrlError, match="VecOnPolicyCollector"):
        VecOnPolicyCollector(small_qnet(1), env=make(), eval_env=make(), pf=pf, **kw)


# ---------------------------------------------------------------- the product on PyCatch-v0
class _Rec:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


@pytest.mark.parametrize("algo,dedup", [("dqn", False), ("dqn", True), ("qrdqn", True)])
def test_dqn_and_qrdqn_train_on_catch(algo, dedup):
    from torchrl.algo import DQN, QRDQN
    from torchrl.collector import VecCollector
    from torchrl.env import HostFrameBridge, get_vec_env
    from torchrl.policies import EpsilonGreedyDQNDiscretePolicy, EpsilonGreedyQRDQNDiscretePolicy
    from torchrl.replay_buffers import BaseReplayBuffer, MemoryEfficientReplayBuffer
    from tests.test_dqn_gpu import small_qnet
    N, B, Q, rows = 2, 8, (8 if algo == "qrdqn" else 1), 64
    env = get_vec_env("PyCatch-v0", {"frame_stack": True, "clip_rewards": True, "scale": True}, N)
    env.seed(1)
    torch.manual_seed(5)
    np.random.seed(6)
    qf = small_qnet(3, Q).to(DEV)
    kwp = dict(qf=qf, start_epsilon=1, end_epsilon=0.1, decay_frames=1000, action_shape=3)
    pf = EpsilonGreedyQRDQNDiscretePolicy(quantile_num=Q, **kwp) if Q > 1 else EpsilonGreedyDQNDiscretePolicy(**kwp)
    buf = MemoryEfficientReplayBuffer(N * rows, env_nums=N, min_episode_frames=20) if dedup else BaseReplayBuffer(N * rows, env_nums=N)
    col = VecCollector(env=env, eval_env=None, pf=pf, replay_buffer=buf, device=torch.device(DEV), epoch_frames=N * 24,
                       max_episode_frames=999, eval_episodes=1)
    assert isinstance(col.env, HostFrameBridge) and col.env.frame_stack == 4 and col.env.clip_rewards
    assert isinstance(col.eval_env, HostFrameBridge) and col.eval_env.frame_stack == 4 and col.eval_env.venv is not env
    log = _Rec()
    kw = dict(qf=qf, pf=pf, qlr=2.5e-4, env=col.env, replay_buffer=buf, collector=col, logger=log, discount=0.99,
              num_epochs=2, batch_size=B, device=torch.device(DEV), save_dir=None, tau=0.005, use_soft_update=True, opt_times=2)
    agent = QRDQN(quantile_num=Q, **kw) if Q > 1 else DQN(**kw)
    before = [p.detach().clone() for p in qf.parameters()]
    finished = []
    for _ in range(2):
        res = col.train_one_epoch()
        finished += list(res["train_rewards"])
        agent.update_per_epoch()                                          # (checks the frame stream for overruns)
    assert len(log.infos) == 4 and all(np.isfinite(list(i.values())).all() for i in log.infos)
    assert any((a - b.detach()).abs().max().item() > 0 for a, b in zip(before, qf.parameters()))
    assert len(finished) == 2 * N and set(finished) <= {1.0, -1.0}         # 48 steps: two 20-step episodes per env
    if dedup:
        buf.check_overrun()
    ev = col.eval_one_epoch()
    assert len(ev["eval_rewards"]) == N and set(float(r) for r in ev["eval_rewards"]) <= {1.0, -1.0}
    assert ev["eval_traj_length"] == 20.0
