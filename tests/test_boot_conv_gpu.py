"""Bootstrapped DQN over conv trunks and pixel envs (TRL_BOOT_CONV=1) end to end on the GPU: the three cases of
tests/golden/boot_dqn_conv_update.npz (the unmodified reference classes on the CPU) through `BootstrappedDQN.update`
after each of their two updates -- parameters, optimiser state under torch's names, info --, the policy against the
stored actions, launch-mode equality, re-homing and snapshots, and collection: the per-step frame route on the synthetic
frame env over the plain ring and the frame-deduplicating buffer against the restated draws, and `PyCatch-v0` through
`HostFrameBridge` against the numpy loop of tests/_host_frames_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import _boot_conv_ref as R                                                    # noqa: E402
import _boot_dqn_ref as RB                                                    # noqa: E402
from _host_frames_ref import replay                                           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
A, K = 3, 3
SHAPE = (4, 44, 44)
CONVS = [[8, [8, 8], [4, 4], [0, 0]], [8, [4, 4], [2, 2], [0, 0]], [16, [3, 3], [1, 1], [0, 0]]]


class _Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


class _Stub:
    epoch_frames = 0


@pytest.fixture(scope="module")
def g():
    return R.load_fixture()


@pytest.fixture(autouse=True)
def switch_on(monkeypatch):
    monkeypatch.setenv("TRL_BOOT_CONV", "1")


def make_net(append, shape=SHAPE, n_act=A, heads=K, act=torch.nn.ReLU):
    import functools
    from torchrl import networks
    return networks.BootstrappedNet(output_shape=n_act, head_num=heads, append_hidden_shapes=append, activation_func=act,
                                    base_type=functools.partial(networks.CNNBase, input_shape=shape, hidden_shapes=CONVS))


def fixture_net(g, tag):
    qf = make_net(R.case_args(g, tag)["append"])
    qf.load_state_dict({k: torch.from_numpy(v) for k, v in R.state_dict_of(g, tag + "_qf0_").items()})
    return qf.to(DEV)


def make_agent(qf, n_act=A, heads=K, B=4, env=None, buf=None, col=None, **kw):
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


def fixture_agent(g, tag, **kw):
    a = R.case_args(g, tag)
    qf = fixture_net(g, tag)
    opt = dict(optimizer_class=torch.optim.Adam) if a["opt"][0] == "adam" else \
        dict(optimizer_class=torch.optim.RMSprop, optimizer_info=dict(alpha=a["opt"][1], eps=a["opt"][2]))
    agent, pf = make_agent(qf, B=a["B"], qlr=a["qlr"], tau=a["tau"], use_soft_update=a["soft"],
                           target_hard_update_period=a["period"], **opt, **kw)
    return agent, pf, qf, a


def device_batch(g, s):
    b = R.batch_of(g, s)
    return dict(b, obs=torch.from_numpy(b["obs"]).to(DEV), next_obs=torch.from_numpy(b["next_obs"]).to(DEV))


# ------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", R.CASES)
def test_updates_match_the_reference(g, tag, fused, errlog, monkeypatch):
    """After EACH of the two updates: online and target parameters within 3e-6 (the bound of tests/test_boot_dqn_gpu.py and
    of the conv DQN fixture test, under the same conditioning rule: the reference's own fp32 run lies within 1e-6 of the
    float64 update -- `meta` records 3.6e-7 -- and the conv reductions here, at most 4 x 8 x 8 = 256 terms, are no longer
    than the 84 x 84 DQN fixture's); the optimiser's state under torch's names at the same bound in relative terms (3e-6
    over the scale of the parameter tensor, times the scale of the state tensor: tests/test_optim_engines_gpu.py's rule);
    info rel 1e-4 / abs 1e-5 on exactly the reference's keys.  fused: trl_boot_head_dx_f32 or the three launches."""
    from torchrl_amd.algo.off_policy import bootstrapped_dqn as mod
    monkeypatch.setattr(mod, "HEAD_DX_FUSED", fused)
    agent, _, qf, a = fixture_agent(g, tag)
    names = [n for n, _ in qf.named_parameters()]
    for s in range(a["steps"]):
        info = agent.update(device_batch(g, s))
        want = dict(zip([str(k) for k in g[f"{tag}_s{s}_info_keys"]], g[f"{tag}_s{s}_info_vals"]))
        assert sorted(info) == sorted(want) == ["Reward_Mean", "Training/qf_loss"]
        for k in want:
            errlog(f"{tag} s{s} {k}", abs(info[k] - want[k]), 1e-4 * abs(want[k]) + 1e-5)
            assert info[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5), k
        for name, mod_ in (("qf%d" % (s + 1), qf), ("tqf%d" % (s + 1), agent.target_qf)):
            sd = mod_.state_dict()
            assert list(sd) == list(R.state_dict_of(g, f"{tag}_{name}_"))
            worst = max(float(np.abs(p.cpu().numpy() - g[f"{tag}_{name}_{k.replace('.', '__')}"]).max()) for k, p in sd.items())
            errlog(f"{tag} {name} params", worst, 3e-6)
            assert worst < 3e-6, (name, worst)
        want_states = ("exp_avg", "exp_avg_sq") if a["opt"][0] == "adam" else ("square_avg",)
        worst = 0.0
        for pn, p in qf.named_parameters():
            state = agent.qf_optimizer.state[p]
            assert sorted(k for k in state if k != "step") == sorted(want_states), (pn, sorted(state))
            p_scale = float(np.abs(g[f"{tag}_qf{s + 1}_{pn.replace('.', '__')}"]).max())
            for sn in want_states:
                ref = g[f"{tag}_state{s + 1}_{sn}_{pn.replace('.', '__')}"]
                tol = 3e-6 * float(np.abs(ref).max()) / p_scale
                err = float(np.abs(state[sn].cpu().numpy() - ref).max())
                worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else float("inf")))
        errlog(f"{tag} s{s} state over bound", worst, 1.0)
        assert worst <= 1.0, (tag, s, worst)
    eng = agent.engine()
    assert eng.is_conv and eng.head_dx_fused == fused and eng.opt_spec[0] == a["opt"][0] and len(names) == len(qf.param_list())
    assert eng.head_dx_route == ("fused" if fused else "three_launches")     # the route that actually ran
    if tag == "rms":                                                     # period 2: the hard copy after update 2
        assert all(torch.equal(x, y) for x, y in zip(qf.state_dict().values(), agent.target_qf.state_dict().values()))


@pytest.mark.parametrize("tag", R.CASES)
def test_network_and_policy_match_the_fixture(g, tag, errlog):
    """Q values at abs 1e-6 + rel 1e-5 (the bound of the MLP fixture test; the conv layers' 256-, 128- and 72-term sums on
    |x| <= 0.5 inputs and the heads' small last-layer weights keep the same room); actions equal the reference's (the CPU
    test shows every top-two gap above 4e-6)."""
    from torchrl.policies import BootstrappedDQNDiscretePolicy
    from torchrl_amd import _C
    qf = fixture_net(g, tag)
    frames = torch.from_numpy(g["batch_s0_obs"]).to(DEV)
    before = _C.eager_fallback_count()
    with torch.no_grad():
        out = qf(frames, range(K))
        sub = qf(frames, [2, 0])
    assert len(out) == K and out[0].shape == (frames.shape[0], A) and _C.eager_fallback_count() == before
    got = np.stack([o.cpu().numpy() for o in out])
    err = np.abs(got - g[tag + "_q0"])
    errlog(tag + " q", float((err / (1e-6 + 1e-5 * np.abs(g[tag + "_q0"]))).max()), 1.0)
    assert np.all(err <= 1e-6 + 1e-5 * np.abs(g[tag + "_q0"]))
    assert torch.equal(sub[0], out[2]) and torch.equal(sub[1], out[0])
    pf = BootstrappedDQNDiscretePolicy(qf=qf, head_num=K, action_shape=A)
    n = int(frames.shape[0])
    for k in range(K):
        pf.set_head(k)
        res = pf.explore(frames)
        assert res["action"].shape == (n, 1) and res["action"].dtype == torch.int64 and res["q_value"].shape == (n, A)
        assert np.array_equal(res["action"].cpu().numpy()[:, 0], g[tag + "_explore"][k])
        assert torch.equal(pf.idx, torch.full((n,), k, dtype=torch.int64, device=DEV))
    ev = pf.eval_act(frames)
    assert isinstance(ev, np.ndarray) and ev.shape == (n, 1) and np.array_equal(ev[:, 0], g[tag + "_eval"].reshape(-1))
    with pytest.raises(_C.TrlError, match="uint8"):
        qf.forward_stack(frames.float())


# ------------------------------------------------------------------ launch modes, re-homing, snapshots
def _run_mode(g, mode, fused, monkeypatch):
    from torchrl_amd.algo.off_policy import bootstrapped_dqn as mod
    monkeypatch.setattr(mod, "HEAD_DX_FUSED", fused)
    if mode == "eager":
        monkeypatch.setenv("TRL_NO_GRAPH", "1")
    else:
        monkeypatch.delenv("TRL_NO_GRAPH", raising=False)
    agent, _, qf, _ = fixture_agent(g, "rms")
    infos = []
    for s in (0, 1, 0, 1):                                               # eager, captured, replayed, replayed
        infos.append(agent.update(device_batch(g, s)))
    torch.cuda.synchronize()
    return ([p.detach().cpu().clone() for p in qf.parameters()], [p.detach().cpu().clone() for p in agent.target_qf.parameters()],
            infos, agent)


@pytest.mark.parametrize("fused", [False, True])
def test_launch_modes_give_the_same_bits(g, fused, monkeypatch):
    eager = _run_mode(g, "eager", fused, monkeypatch)
    default = _run_mode(g, "default", fused, monkeypatch)
    assert eager[3].engine().head_dx_route == default[3].engine().head_dx_route == ("fused" if fused else "three_launches")
    assert len(default[3].engine()._graphs) == 1 and len(eager[3].engine()._graphs) == 0
    assert all(torch.equal(x, y) for x, y in zip(eager[0], default[0]))
    assert all(torch.equal(x, y) for x, y in zip(eager[1], default[1]))
    assert [sorted(i.items()) for i in eager[2]] == [sorted(i.items()) for i in default[2]]
    eng = default[3].engine()
    assert float(eng.step_state[0]) == 4.0 and float(eng.m.abs().sum()) > 0.0
    off = 0
    for p in default[3].qf.param_list():                                 # RMSprop's square_avg IS the engine's buffer
        st = default[3].qf_optimizer.state[p]
        assert st["square_avg"].data_ptr() == eng.m.data_ptr() + 4 * off and p.data_ptr() == eng.flat.data_ptr() + 4 * off
        off += p.numel()
    assert off == eng.flat.numel()


def test_snapshot_round_trip_and_rehoming(g, tmp_path):
    tag = "hid"
    agent, _, qf, _ = fixture_agent(g, tag)
    batch = device_batch(g, 0)
    agent.update(batch)
    agent.snapshot(str(tmp_path), "best")
    state = torch.load(os.path.join(str(tmp_path), "model_pf_best.pth"), map_location="cpu")
    assert list(state) == list(R.state_dict_of(g, tag + "_qf0_"))        # the reference's keys, in its order
    assert all(torch.equal(state[k], v.cpu()) for k, v in qf.state_dict().items())
    eng = agent.engine()
    # a reference-shaped dict loads in place: the parameters stay views of the flat buffer
    ref_sd = {k: torch.from_numpy(v) for k, v in R.state_dict_of(g, tag + "_qf2_").items()}
    qf.load_state_dict(ref_sd)
    agent.target_qf.load_state_dict(ref_sd)
    assert qf.param_list()[0].data_ptr() == eng.flat.data_ptr()
    assert torch.equal(eng.flat[:qf.param_list()[0].numel()].cpu(), ref_sd["base.seq_convs.0.weight"].reshape(-1))
    assert all(torch.equal(ref_sd[k], v.cpu()) for k, v in qf.state_dict().items())
    # storage that moved (a round trip through the CPU) is re-homed at the next update
    qf.to("cpu")
    qf.to(DEV)
    assert qf.param_list()[0].data_ptr() != eng.flat.data_ptr()
    info = agent.update(batch)
    assert np.isfinite(list(info.values())).all()
    off = 0
    for p in qf.param_list():
        assert p.data_ptr() == eng.flat.data_ptr() + 4 * off
        off += p.numel()
    assert off == eng.flat.numel()


# ------------------------------------------------------------------ collection
def _synth_collector(dedup, N=4, heads=K, steps=8, horizon=3):
    from torchrl.collector import VecCollector
    from torchrl.policies import BootstrappedDQNDiscretePolicy
    from torchrl.replay_buffers import BaseReplayBuffer, MemoryEfficientReplayBuffer
    from torchrl_amd.env.synth import SynthFrameVecEnv
    env, eval_env = (SynthFrameVecEnv(N, frame_shape=SHAPE, action_num=A, horizon=horizon, device=DEV) for _ in range(2))
    env.seed(2)
    torch.manual_seed(4)
    qf = make_net([], heads=heads).to(DEV)
    pf = BootstrappedDQNDiscretePolicy(qf=qf, head_num=heads, action_shape=A)
    buf = MemoryEfficientReplayBuffer(steps * N, env_nums=N, device=DEV, min_episode_frames=horizon) if dedup else \
        BaseReplayBuffer(steps * N, env_nums=N)
    col = VecCollector(env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, epoch_frames=N * 4,
                       max_episode_frames=100, eval_episodes=1)
    agent, _ = make_agent(qf, heads=heads, B=2 * N, env=col.env, buf=buf, col=col, pf=pf)
    return agent, pf, buf, col


@pytest.mark.parametrize("dedup", [False, True])
def test_collection_on_the_frame_env_matches_the_restated_draws(dedup):
    _check_collection(dedup)


def test_plain_ring_and_dedup_buffer_hold_the_same_transitions():
    plain, dedup = _check_collection(False), _check_collection(True)
    assert sorted(plain) == sorted(dedup) and all(torch.equal(plain[k], dedup[k]) for k in plain)


def _check_collection(dedup):
    """The checks of one buffer kind; returns what the buffer holds (on the host)."""
    N, heads, steps = 4, K, 8
    agent, pf, buf, col = _synth_collector(dedup)
    assert pf.bernoulli_p == 0.5 and pf.idx is None
    col.rollout(4)
    idx4 = pf.idx.clone()
    keys = ("acts", "masks", "rewards", "terminals")
    ring0 = {k: getattr(buf, "_" + k).clone() for k in keys}
    res = col.eval_one_epoch()                                           # the ensemble vote: draws nothing, shifts nothing
    assert len(res["eval_rewards"]) == N
    assert torch.equal(pf.idx, idx4) and col.global_step == 4 and buf._top == 4
    assert all(torch.equal(getattr(buf, "_" + k), v) for k, v in ring0.items())
    col.rollout(4)
    torch.cuda.synchronize()
    assert col.global_step == steps and tuple(buf._masks.shape) == (steps, N, heads) and tuple(buf._acts.shape) == (steps, N, 1)
    all_rows = torch.arange(steps, device=DEV)
    obs = (buf._gather("obs", all_rows) if dedup else buf._obs).reshape((steps, N) + SHAPE)
    assert obs.dtype == torch.uint8
    idx = RB.heads_ref(np.zeros(N), heads, pf.seed, -1)                   # the draw before step 0
    ended_any = 0
    for t in range(steps):
        assert np.array_equal(buf._masks[t].cpu().numpy(), RB.masks_ref(N, heads, 0.5, pf.seed, t)), t
        with torch.no_grad():
            q = pf.qf.forward_stack(obs[t]).cpu().numpy()                # the same fp32 kernels on the stored frame stacks
        want, _, _ = RB.boot_act_ref(q, idx)
        assert np.array_equal(buf._acts[t].cpu().numpy()[:, 0], want.astype(np.float32)), t
        ended = buf._terminals[t].cpu().numpy()[:, 0] != 0
        ended_any += int(ended.sum())
        new = RB.heads_ref(idx, heads, pf.seed, t, reset_mask=ended)
        assert np.array_equal(new[~ended], idx[~ended])                   # heads change only where an episode ended
        idx = new
        if t == 3:
            assert np.array_equal(idx4.cpu().numpy(), idx)
    assert np.array_equal(pf.idx.cpu().numpy(), idx) and ended_any == 2 * N      # horizon 3: steps 2 and 5 end every episode
    # `random_batch` carries `masks` aligned with the other keys: every sampled row is one stored (step, env) cell
    np.random.seed(21)
    batch = buf.random_batch(2 * N, agent.sample_key)
    np.random.seed(21)
    rows = np.random.randint(0, buf.num_steps_can_sample(), 2)
    assert batch["obs"].dtype == torch.uint8 and tuple(batch["obs"].shape) == (2 * N,) + SHAPE
    assert tuple(batch["masks"].shape) == (2 * N, heads)
    for j, r in enumerate(rows):
        sl = slice(j * N, (j + 1) * N)
        assert torch.equal(batch["masks"][sl], buf._masks[r]) and torch.equal(batch["acts"][sl], buf._acts[r])
        assert torch.equal(batch["obs"][sl], obs[r]) and torch.equal(batch["rewards"][sl], buf._rewards[r])
        assert np.array_equal(batch["masks"][sl].cpu().numpy(), RB.masks_ref(N, heads, 0.5, pf.seed, int(r)))
    info = agent.update(batch)
    assert sorted(info) == ["Reward_Mean", "Training/qf_loss"] and np.isfinite(list(info.values())).all()
    if dedup:
        buf.check_overrun()
    held = {k: getattr(buf, "_" + k).cpu() for k in keys}
    held["obs"] = obs.cpu()
    return held


def test_two_epochs_of_catch_through_the_host_frame_bridge():
    """PyCatch-v0, 4 envs, two epochs of 12 vector steps (the 20-step episodes end once inside): the run completes, the stored
    frame stacks are byte-equal to the numpy loop of tests/_host_frames_ref.py replayed with the stored actions, `masks`
    is there with the restated draws, and updates on the sampled batches stay finite and on the HIP path."""
    from torchrl.collector import VecCollector
    from torchrl.env import HostFrameBridge, get_vec_env
    from torchrl.env.py_envs import CatchEnv
    from torchrl.policies import BootstrappedDQNDiscretePolicy
    from torchrl.replay_buffers import BaseReplayBuffer
    from torchrl_amd import _C
    N, heads, per_epoch = 4, K, 12
    steps = 2 * per_epoch
    env = get_vec_env("PyCatch-v0", {"frame_stack": True, "clip_rewards": True, "scale": True}, N)
    env.seed(1)
    torch.manual_seed(5)
    np.random.seed(6)
    qf = make_net([16], shape=(4, 84, 84), heads=heads).to(DEV)
    pf = BootstrappedDQNDiscretePolicy(qf=qf, head_num=heads, action_shape=A)
    buf = BaseReplayBuffer(N * steps, env_nums=N)
    before = _C.eager_fallback_count()
    col = VecCollector(env=env, eval_env=None, pf=pf, replay_buffer=buf, device=DEV, epoch_frames=N * per_epoch,
                       max_episode_frames=999, eval_episodes=1)
    assert isinstance(col.env, HostFrameBridge) and col.env.frame_stack == 4
    agent, _ = make_agent(qf, heads=heads, B=2 * N, env=col.env, buf=buf, col=col, pf=pf, opt_times=2, num_epochs=2)
    finished = []
    for _ in range(2):
        res = col.train_one_epoch()
        finished += list(res["train_rewards"])
        agent.update_per_epoch()
    torch.cuda.synchronize()
    assert len(agent.logger.infos) == 4 and all(np.isfinite(list(i.values())).all() for i in agent.logger.infos)
    assert len(finished) == N and set(finished) <= {1.0, -1.0}            # step 20 ends every env's first episode
    assert _C.eager_fallback_count() == before, _C.EAGER_FALLBACKS
    acts = buf._acts.cpu().numpy()[:, :, 0]
    assert acts.shape == (steps, N) and set(np.unique(acts)) <= {0.0, 1.0, 2.0}
    ref = replay([CatchEnv(1 * N + i) for i in range(N)], acts.astype(np.int64), 4, 999, clip_rewards=True)
    for key in ("obs", "next_obs", "rewards", "terminals", "time_limits"):
        got = getattr(buf, "_" + key).cpu().numpy()
        assert got.dtype == ref[key].dtype and np.array_equal(got, ref[key]), key
    assert buf._obs.dtype == torch.uint8 and tuple(buf._masks.shape) == (steps, N, heads)
    for t in range(steps):
        assert np.array_equal(buf._masks[t].cpu().numpy(), RB.masks_ref(N, heads, 0.5, pf.seed, t)), t
    ev = col.eval_one_epoch()
    assert len(ev["eval_rewards"]) == N and ev["eval_traj_length"] == 20.0 and col.global_step == steps
