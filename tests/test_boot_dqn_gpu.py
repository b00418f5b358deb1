"""Bootstrapped DQN end to end on the GPU: the three fixture cases through `BootstrappedDQN.update`, the network and the
policy against the fixture's outputs and actions, launch-mode equality (eager / captured and replayed / whole epochs as
one graph), collection on the device env against the restated draws, whole epochs of the host cart-pole and the device
wiring without leaving the HIP path, and snapshots."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _boot_dqn_ref as R                                                     # noqa: E402
from torchrl.algo import BootstrappedDQN                                      # noqa: E402,F401  (no test here runs without the feature)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
D, A, K, H = 17, 3, 4, 32


class _Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(d)
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


class _Stub:
    epoch_frames = 0


@pytest.fixture(scope="module")
def g():
    return R.load_fixture()


def make_net(append, obs_dim=D, n_act=A, heads=K, hidden=(H, H)):
    from torchrl import networks
    return networks.BootstrappedNet(output_shape=n_act, head_num=heads, append_hidden_shapes=append,
                                    activation_func=torch.nn.ReLU, base_type=networks.MLPBase, input_shape=obs_dim,
                                    hidden_shapes=list(hidden))


def fixture_net(g, tag):
    qf = make_net([int(v) for v in g[tag + "_append"]])
    qf.load_state_dict({k: torch.from_numpy(v) for k, v in R.state_dict_of(g, tag + "_qf0_").items()})
    return qf.to(DEV)


def make_agent(qf, n_act=A, heads=K, B=48, env=None, buf=None, col=None, **kw):
    import gym
    from torchrl.algo import BootstrappedDQN
    from torchrl.policies import BootstrappedDQNDiscretePolicy

    class Env:
        action_space = gym.spaces.Discrete(n_act)
    pf = kw.pop("pf", None) or BootstrappedDQNDiscretePolicy(qf=qf, head_num=heads, action_shape=n_act)
    args = dict(head_num=heads, bernoulli_p=0.5, qf=qf, pf=pf, qlr=1e-3, env=env or Env(), replay_buffer=buf,
                collector=col or _Stub(), logger=_Log(), discount=0.99, num_epochs=10, batch_size=B, device=DEV,
                save_dir=None, tau=0.005, use_soft_update=True, opt_times=1)
    args.update(kw)
    return BootstrappedDQN(**args), pf


# ------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("tag", R.CASES)
def test_updates_match_the_reference(g, tag, errlog):
    """Parameters within 3e-6 after two updates (the bound consumers of the SAC-V fixture use under the same conditioning
    rule: the reference's own fp32 run lies within 1e-6 of the float64 update), info rel 1e-4 / abs 1e-5, exact key set."""
    _, soft, period, steps = (int(v) for v in g[tag + "_args"][1:5])
    qf = fixture_net(g, tag)
    agent, _ = make_agent(qf, use_soft_update=bool(soft), target_hard_update_period=period)
    for s in range(steps):
        info = agent.update({k: g[f"{tag}_s{s}_batch_{k}"] for k in R.BATCH_KEYS})
        want = dict(zip([str(k) for k in g[f"{tag}_s{s}_info_keys"]], g[f"{tag}_s{s}_info_vals"]))
        assert sorted(info) == sorted(want) == ["Reward_Mean", "Training/qf_loss"]
        for k in want:
            errlog(f"{tag} s{s} {k}", abs(info[k] - want[k]), 1e-4 * abs(want[k]) + 1e-5)
            assert info[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5), k
    for name, mod in (("qf1", qf), ("tqf1", agent.target_qf)):
        sd = mod.state_dict()
        assert sorted(sd) == sorted(R.state_dict_of(g, f"{tag}_{name}_"))
        worst = max(float(np.abs(p.cpu().numpy() - g[f"{tag}_{name}_{k.replace('.', '__')}"]).max()) for k, p in sd.items())
        errlog(f"{tag} {name} params", worst, 3e-6)
        assert worst < 3e-6, (name, worst)
    if tag == "hard":
        assert all(torch.equal(a, b) for a, b in zip(qf.state_dict().values(), agent.target_qf.state_dict().values()))


@pytest.mark.parametrize("tag", R.CASES)
def test_network_and_policy_match_the_fixture(g, tag, errlog):
    """Q values: three dense layers of 17, 32 and 32 (or 16) terms on O(1) activations differ from the CPU's summation
    order by at most (17 + 32 + 32) U of the terms' magnitude; the last layer's weights (|w| <= 3e-3 over 32 inputs) scale
    what the trunk contributes by 0.1: abs 1e-6 + rel 1e-5 holds with room.  Actions: the CPU test shows every top-two gap
    of these cells above 4e-6, so the float32 arg-max is the reference's."""
    from torchrl.policies import BootstrappedDQNDiscretePolicy
    from torchrl_amd import _C
    qf = fixture_net(g, tag)
    obs = torch.from_numpy(g[tag + "_s0_batch_obs"]).to(DEV)
    before = _C.eager_fallback_count()
    with torch.no_grad():
        out = qf(obs, range(K))
        sub = qf(obs, [3, 1])
    assert len(out) == K and out[0].shape == (obs.shape[0], A) and _C.eager_fallback_count() == before
    got = np.stack([o.cpu().numpy() for o in out])
    err = np.abs(got - g[tag + "_q0"])
    errlog(tag + " q", float((err / (1e-6 + 1e-5 * np.abs(g[tag + "_q0"]))).max()), 1.0)
    assert np.all(err <= 1e-6 + 1e-5 * np.abs(g[tag + "_q0"]))
    assert torch.equal(sub[0], out[3]) and torch.equal(sub[1], out[1])
    pf = BootstrappedDQNDiscretePolicy(qf=qf, head_num=K, action_shape=A)
    pf1 = BootstrappedDQNDiscretePolicy(qf=qf, head_num=K, action_shape=A)  # one env: a (1, D) input, the reference's call
    single = torch.from_numpy(g[tag + "_single_obs"]).to(DEV)
    for k in range(K):
        pf.set_head(k)
        res = pf.explore(single)
        assert res["action"].shape == (8, 1) and res["action"].dtype == torch.int64 and res["q_value"].shape == (8, A)
        assert np.array_equal(res["action"].cpu().numpy()[:, 0], g[tag + "_explore"][k])
        assert torch.equal(pf.idx, torch.full((8,), k, dtype=torch.int64, device=DEV))
        pf1.set_head(k)
        one = pf1.explore(single[2:3])
        assert int(one["action"]) == int(g[tag + "_explore"][k][2]) and pf1.idx.tolist() == [k]
        pf.set_head(torch.full((8,), k))
        assert np.array_equal(pf.explore(single)["action"].cpu().numpy()[:, 0], g[tag + "_explore"][k])
    ev = pf.eval_act(single)
    assert isinstance(ev, np.ndarray) and ev.shape == (8, 1) and np.array_equal(ev[:, 0], g[tag + "_eval"].reshape(-1))
    # a policy that has seen no env yet draws a head for every env at its first explore
    pf2 = BootstrappedDQNDiscretePolicy(qf=qf, head_num=K, action_shape=A)
    pf2.explore(single)
    assert np.array_equal(pf2.idx.cpu().numpy(), R.heads_ref(np.zeros(8), K, pf2.seed, -1))


# ------------------------------------------------------------------ launch modes
def _run_mode(mode, monkeypatch):
    """Four updates at B = 64 from one seeded state; returns (parameters, target parameters, infos, agent)."""
    from torchrl.replay_buffers import BaseReplayBuffer
    torch.manual_seed(5)
    qf = make_net([16], n_act=6, heads=5).to(DEV)
    N, rows, B = 16, 8, 64
    buf = BaseReplayBuffer(rows * N, env_nums=N)
    rs = np.random.RandomState(3)
    for _ in range(rows):
        buf.add_sample({"obs": rs.randn(N, D).astype(np.float32), "next_obs": rs.randn(N, D).astype(np.float32),
                        "acts": rs.randint(0, 6, (N, 1)).astype(np.float32), "rewards": rs.randn(N, 1).astype(np.float32),
                        "terminals": (rs.rand(N, 1) < 0.2).astype(np.float32),
                        "masks": (rs.rand(N, 5) < 0.5).astype(np.float32),
                        "time_limits": np.zeros((N, 1), dtype=np.float32)})
    agent, _ = make_agent(qf, n_act=6, heads=5, B=B, buf=buf, opt_times=2)
    if mode == "eager":
        monkeypatch.setenv("TRL_NO_GRAPH", "1")
    np.random.seed(9)
    infos = []
    if mode == "epoch":
        infos += [agent.update(agent._sample())]                         # the first batch shows the shapes
        first = agent.update_epoch_deferred(1)
        assert first is not None
        infos += agent.resolve_updates(first)
        handles = agent.update_epoch_deferred(1)                          # captured
        infos += agent.resolve_updates(handles)
        infos += agent.resolve_updates(agent.update_epoch_deferred(1))    # replayed
    else:
        handles = [agent.update_deferred(agent._sample()) for _ in range(4)]
        infos = agent.resolve_updates(handles)
    torch.cuda.synchronize()
    return ([p.detach().cpu().clone() for p in qf.parameters()], [p.detach().cpu().clone() for p in agent.target_qf.parameters()],
            infos, agent)


def test_launch_modes_give_the_same_bits(monkeypatch):
    eager = _run_mode("eager", monkeypatch)
    monkeypatch.delenv("TRL_NO_GRAPH", raising=False)
    default = _run_mode("default", monkeypatch)
    epoch = _run_mode("epoch", monkeypatch)
    assert len(default[3].engine()._graphs) == 1 and len(eager[3].engine()._graphs) == 0
    assert any(k[0] == "epoch" for k in epoch[3].engine()._graphs if isinstance(k, tuple))
    for other in (default, epoch):
        assert all(torch.equal(a, b) for a, b in zip(eager[0], other[0]))
        assert all(torch.equal(a, b) for a, b in zip(eager[1], other[1]))
        assert [sorted(i.items()) for i in eager[2]] == [sorted(i.items()) for i in other[2]]
    assert len(eager[2]) == 4 and all(np.isfinite(list(i.values())).all() for i in eager[2])
    # after an epoch `qf_optimizer.state` holds the engine's moments
    agent = epoch[3]
    eng = agent.engine()
    assert float(eng.m.abs().sum()) > 0.0 and float(eng.step_state[0]) == 4.0
    off = 0
    for p in agent.qf.param_list():
        st = agent.qf_optimizer.state[p]
        assert st["exp_avg"].data_ptr() == eng.m.data_ptr() + 4 * off and st["exp_avg_sq"].data_ptr() == eng.v.data_ptr() + 4 * off
        assert p.data_ptr() == eng.flat.data_ptr() + 4 * off
        off += p.numel()
    assert off == eng.flat.numel()


def test_launch_count_does_not_grow_with_the_number_of_heads(monkeypatch):
    """The launch sequence of one update, listed by entry point, has the same length for K = 1, 10 and 12, the most
    problems one grouped dense-layer launch carries; from K = 13 on every grouped launch of the heads becomes
    ceil(K / 12): two head levels forward on two networks (+ 4) and their weight and input gradients (+ 4)."""
    from torchrl_amd import _C
    monkeypatch.setenv("TRL_NO_GRAPH", "1")
    counts = {}
    for heads in (1, 10, 12, 13):
        torch.manual_seed(1)
        qf = make_net([16], n_act=6, heads=heads).to(DEV)
        agent, _ = make_agent(qf, n_act=6, heads=heads, B=64)
        rs = np.random.RandomState(0)
        batch = {"obs": rs.randn(64, D).astype(np.float32), "next_obs": rs.randn(64, D).astype(np.float32),
                 "acts": rs.randint(0, 6, (64, 1)).astype(np.float32), "rewards": rs.randn(64, 1).astype(np.float32),
                 "terminals": np.zeros((64, 1), np.float32), "masks": np.ones((64, heads), np.float32)}
        agent.update(batch)
        calls = []

        class Spy:
            def __init__(self, lib): self._lib = lib

            def __getattr__(self, name):
                fn = getattr(self._lib, name)
                if name.endswith(("_f32", "_i64")):
                    calls.append(name)
                return fn
        real = _C.lib()
        monkeypatch.setattr(_C, "_lib", Spy(real))
        agent.update(batch)
        monkeypatch.setattr(_C, "_lib", real)
        counts[heads] = calls
        print("LAUNCHES K=%d (%d): %s" % (heads, len(calls), " ".join(calls)))
    assert len(counts[1]) == len(counts[10]) == len(counts[12]) and counts[1].count("trl_boot_td_loss_f32") == 1
    assert counts[10].count("trl_boot_fold_f32") == 1
    assert len(counts[13]) == len(counts[12]) + 8 and counts[13].count("trl_boot_td_loss_f32") == 1
    assert counts[13].count("trl_boot_fold_f32") == 1


# ------------------------------------------------------------------ many heads
@pytest.mark.parametrize("heads", [13, 64])
def test_many_heads_forward_policy_and_update(heads, errlog):
    """13 heads: the first size that takes two grouped launches per head level; 64: the most the path carries.  Forward
    against the float64 restatement (the bound of the fixture test: same layer widths), explore / eval_act against the
    restated arg-max on the launch's own Q stack, one update's GRADIENT and loss against the restatement -- the gradient,
    not the stepped parameters: Adam's first step is lr sign(g) whatever the size of g, so a parameter comparison is only
    as good as the smallest gradient entry.  A gradient entry is a sum over at most B K = 4096 (sample, head) terms:
    worst case n U = 2.5e-4 of the sum of their magnitudes, taken relative to the largest entry of its tensor."""
    from torchrl_amd import _C
    n_act, B = 6, 64
    torch.manual_seed(11)
    qf = make_net([16], n_act=n_act, heads=heads).to(DEV)
    g = {"n_" + k.replace(".", "__"): v.cpu().numpy() for k, v in qf.state_dict().items()}
    agent, pf = make_agent(qf, n_act=n_act, heads=heads, B=B)
    rs = np.random.RandomState(heads)
    batch = {"obs": rs.randn(B, D).astype(np.float32), "next_obs": rs.randn(B, D).astype(np.float32),
             "acts": rs.randint(0, n_act, (B, 1)).astype(np.float32), "rewards": rs.randn(B, 1).astype(np.float32),
             "terminals": (rs.rand(B, 1) < 0.2).astype(np.float32), "masks": (rs.rand(B, heads) < 0.5).astype(np.float32)}
    obs = torch.from_numpy(batch["obs"]).to(DEV)
    before = _C.eager_fallback_count()
    with torch.no_grad():
        out = qf(obs, range(heads))
    want, _ = R.q_all(R.net_of(g, "n_", heads), batch["obs"].astype(np.float64))
    got = np.stack([o.cpu().numpy() for o in out])
    assert got.shape == (heads, B, n_act)
    ratio = float((np.abs(got - want) / (1e-6 + 1e-5 * np.abs(want))).max())
    errlog("K=%d q" % heads, ratio, 1.0)
    assert ratio <= 1.0
    head = torch.from_numpy(rs.randint(0, heads, B).astype(np.int64))
    head[0], head[1] = heads - 1, 0
    pf.set_head(head)
    res = pf.explore(obs)
    act_ref, q_ref, _ = R.boot_act_ref(got, head.numpy())
    assert np.array_equal(res["action"].cpu().numpy()[:, 0], act_ref)
    assert np.array_equal(res["q_value"].cpu().numpy().astype(np.float64), q_ref)
    assert np.array_equal(pf.eval_act(obs)[:, 0], R.boot_act_ref(got, None)[0])
    up = R.Update(R.net_of(g, "n_", heads), R.net_of(g, "n_", heads), 1e-3, tau=0.005)
    ref_info = up.update(batch)
    info = agent.update(batch)
    torch.cuda.synchronize()
    assert _C.eager_fallback_count() == before
    for k in ref_info:
        assert info[k] == pytest.approx(ref_info[k], rel=1e-4, abs=1e-5), k
    eng, off, worst = agent.engine(), 0, 0.0
    grads = eng.grads.cpu().numpy().astype(np.float64)
    for p, gr in zip(qf.param_list(), up.last_grads):
        mine = grads[off:off + p.numel()].reshape(gr.shape)
        off += p.numel()
        worst = max(worst, float(np.abs(mine - gr).max() / (2.5e-4 * max(np.abs(gr).max(), 1e-30))))
    errlog("K=%d grads" % heads, worst, 1.0)
    assert off == grads.size and worst <= 1.0, worst
    assert float(eng.step_state[0]) == 1.0 and all(torch.isfinite(p).all() for p in qf.parameters())


def test_more_than_64_heads_are_refused():
    from torchrl.policies import BootstrappedDQNDiscretePolicy
    from torchrl_amd import _C
    with pytest.raises(_C.TrlError, match="1..64 heads"):
        make_net([], heads=65)
    with pytest.raises(_C.TrlError, match="1..64 heads"):
        BootstrappedDQNDiscretePolicy(qf=make_net([]), head_num=65, action_shape=A)
    with pytest.raises(_C.TrlError, match="1 <= K <= 64"):
        _C.boot_act(torch.zeros(65, 2, 2, device=DEV), None)


# ------------------------------------------------------------------ collection
def _collector(env_id, N, heads, n_act, obs_dim, epoch_steps, rows, horizon=None, host=False, seed=4, **agent_kw):
    from torchrl.collector import VecCollector
    from torchrl.env import VecEnv, get_vec_env
    from torchrl.env.py_envs import CartPoleEnv
    from torchrl.policies import BootstrappedDQNDiscretePolicy
    from torchrl.replay_buffers import BaseReplayBuffer
    if host:
        env, eval_env = VecEnv(N, CartPoleEnv, ()), VecEnv(N, CartPoleEnv, ())
        env.seed(0)
        eval_env.seed(1)
    else:
        env, eval_env = (get_vec_env(env_id, {"reward_scale": 1}, N) for _ in range(2))
        env.horizon = eval_env.horizon = horizon
        env.seed(2)
    torch.manual_seed(seed)
    qf = make_net([], obs_dim=obs_dim, n_act=n_act, heads=heads).to(DEV)
    pf = BootstrappedDQNDiscretePolicy(qf=qf, head_num=heads, action_shape=n_act)
    buf = BaseReplayBuffer(rows * N, env_nums=N)
    col = VecCollector(env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, epoch_frames=N * epoch_steps,
                       max_episode_frames=100, eval_episodes=1)
    agent, _ = make_agent(qf, n_act=n_act, heads=heads, B=2 * N, env=col.env, buf=buf, col=col, pf=pf, **agent_kw)
    return agent, pf, buf, col


def test_collection_on_the_device_env_matches_the_restated_draws():
    from torchrl_amd import _C
    N, heads, n_act, steps = 16, 4, 6, 8
    agent, pf, buf, col = _collector("SynthCheetahDiscrete-v0", N, heads, n_act, 17, 4, rows=steps, horizon=3)
    assert pf.bernoulli_p == 0.5 and pf.idx is None
    idx_log = []
    col.rollout(4)
    idx_log.append(pf.idx.clone())
    # an evaluation in between leaves the heads, the ring and the step count alone
    ring0 = {k: getattr(buf, "_" + k).clone() for k in ("obs", "acts", "masks", "rewards", "terminals")}
    res = col.eval_one_epoch()
    assert len(res["eval_rewards"]) == N and res["eval_traj_length"] == 3
    assert torch.equal(pf.idx, idx_log[0]) and col.global_step == 4 and buf._top == 4
    assert all(torch.equal(getattr(buf, "_" + k), v) for k, v in ring0.items())
    col.rollout(4)
    torch.cuda.synchronize()
    assert col.global_step == steps and tuple(buf._masks.shape) == (steps, N, heads) and tuple(buf._acts.shape) == (steps, N, 1)
    idx = R.heads_ref(np.zeros(N), heads, pf.seed, -1)                    # the draw before step 0
    ended_any = 0
    for t in range(steps):
        assert np.array_equal(buf._masks[t].cpu().numpy(), R.masks_ref(N, heads, 0.5, pf.seed, t)), t
        with torch.no_grad():
            q = pf.qf.forward_stack(buf._obs[t]).cpu().numpy()            # the same fp32 kernels on the stored observations
        want, _, _ = R.boot_act_ref(q, idx)
        assert np.array_equal(buf._acts[t].cpu().numpy()[:, 0], want.astype(np.float32)), t
        ended = buf._terminals[t].cpu().numpy()[:, 0] != 0
        ended_any += int(ended.sum())
        idx = R.heads_ref(idx, heads, pf.seed, t, reset_mask=ended)
        if t == 3:
            assert np.array_equal(idx_log[0].cpu().numpy(), idx)
    assert np.array_equal(pf.idx.cpu().numpy(), idx) and ended_any == 2 * N    # horizon 3: steps 2 and 5 end every episode
    assert len(np.unique(idx)) > 1


@pytest.mark.parametrize("host", [True, False])
def test_one_epoch_of_the_wiring_stays_on_the_hip_path(host):
    from torchrl_amd import _C
    before = _C.eager_fallback_count()
    if host:
        agent, pf, buf, col = _collector(None, 8, 10, 2, 4, 8, rows=32, host=True, opt_times=2)
    else:
        agent, pf, buf, col = _collector("SynthCheetahDiscrete-v0", 8, 10, 6, 17, 8, rows=32, horizon=5, opt_times=2)
    np.random.seed(0)
    for _ in range(2):
        res = col.train_one_epoch()
        agent.update_per_epoch()
        ev = col.eval_one_epoch()
    torch.cuda.synchronize()
    assert len(agent.logger.infos) == 4 and len(ev["eval_rewards"]) == 8
    assert all(sorted(i) == ["Reward_Mean", "Training/qf_loss"] and np.isfinite(list(i.values())).all()
               for i in agent.logger.infos)
    assert np.isfinite(res["train_epoch_reward"])
    assert _C.eager_fallback_count() == before, _C.EAGER_FALLBACKS


# ------------------------------------------------------------------ snapshots
def test_snapshot_round_trip_and_rehoming(g, tmp_path):
    tag = "hid"
    qf = fixture_net(g, tag)
    agent, _ = make_agent(qf)
    batch = {k: g[f"{tag}_s0_batch_{k}"] for k in R.BATCH_KEYS}
    agent.update(batch)
    assert [n for n, _ in agent.snapshot_networks] == ["pf"]
    agent.snapshot(str(tmp_path), "best")
    state = torch.load(os.path.join(str(tmp_path), "model_pf_best.pth"), map_location="cpu")
    assert sorted(state) == sorted(R.state_dict_of(g, tag + "_qf0_"))     # the reference's keys
    assert all(torch.equal(state[k], v.cpu()) for k, v in qf.state_dict().items())
    eng = agent.engine()
    # a load copies in place: the parameters stay views of the flat buffer, and the next update steps the loaded values
    agent.update(batch)
    qf.load_state_dict(state)
    agent.target_qf.load_state_dict(state)
    assert qf.param_list()[0].data_ptr() == eng.flat.data_ptr()
    assert torch.equal(eng.flat[:qf.param_list()[0].numel()].cpu(), state["base.seq_fcs.0.weight"].reshape(-1))
    # storage that moved (here: a round trip through the CPU) is re-homed at the next update
    qf.to("cpu")
    qf.to(DEV)
    assert qf.param_list()[0].data_ptr() != eng.flat.data_ptr()
    info = agent.update(batch)
    assert np.isfinite(list(info.values())).all()
    off = 0
    for p in qf.param_list():
        assert p.data_ptr() == eng.flat.data_ptr() + 4 * off
        off += p.numel()
    assert not torch.equal(qf.state_dict()["head0.0.weight"].cpu(), state["head0.0.weight"])
