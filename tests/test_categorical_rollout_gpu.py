"""One-launch rollouts for categorical policies (trl_rollout_synth_cat_f32): the collector's choice of route, the fused
rollout against the per-step route and against CPU stepping, greedy evaluation, and whole PPO / A2C iterations on the
fused collection + the generic update engine.  The route test fails on a build without the categorical head."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _categorical_ref as ref                                                # noqa: E402
import _categorical_rollout_ref as rr                                         # noqa: E402

pytestmark = pytest.mark.gpu
SWITCH = "TRL_CAT_FUSED_ROLLOUT"                                              # the fused route is opt-in (NOTES_categorical_rollout.md)
DEV = torch.device("cuda:0")
RING_KEYS = ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits", "old_logp")
# bounds of tests/test_categorical_gpu.py::test_collector_ring_vs_cpu_stepping; terminals / time_limits exact
TOL = {"obs": (0, 1e-5), "next_obs": (0, 1e-5), "values": (0, 1e-5), "rewards": (0, 1e-5), "terminals": (0, 0),
       "time_limits": (0, 0), "old_logp": (1e-4, 2e-3)}


class _Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


def make_collector(c, N, T, horizon, hidden=(64, 64)):
    """Collector + nets of case `c` on a discrete synthetic env: the registered SynthCheetahDiscrete-v0 for its 17 / 6
    shape, the same env class at the case's sizes otherwise."""
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.env.synth import SynthVecEnv
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    D, A = c["D"], c["A"]
    pf, vf = rr.nets_of(D, A, c["act"], c["net_seed"], hidden=hidden)
    if (D, A) == (17, 6):
        env, eval_env = (get_vec_env("SynthCheetahDiscrete-v0", {"reward_scale": 1, "obs_norm": False}, N, device=DEV)
                         for _ in range(2))
    else:
        env, eval_env = (SynthVecEnv(N, obs_dim=D, act_dim=A, device=DEV, discrete=True) for _ in range(2))
    for e in (env, eval_env):
        e.horizon = horizon
    env.seed(c["env_seed"])
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               epoch_frames=N * T, max_episode_frames=c["max_frames"], eval_episodes=1, noise_mode="device")
    return pf, vf, env, buf, col


def collect(col, buf, epochs):
    """-> per epoch: the ring's tensors on the CPU + the epoch result."""
    out = []
    for _ in range(epochs):
        res = col.train_one_epoch()
        snap = {k: getattr(buf, "_" + k).cpu().numpy().copy() for k in RING_KEYS}
        snap["epoch_reward"] = float(res["train_epoch_reward"])
        snap["episodes"] = [float(x) for x in res["train_rewards"]]
        out.append(snap)
    return out


def compare_rollouts(got, want, borderline, alive, label):
    """`got` / `want`: dicts of (T, N, .) arrays; `borderline` (T, N) bool.  Actions equal, except that an env whose action
    differs on a borderline row leaves the comparison from that step on.  Returns the number of envs dropped."""
    T, N = got["acts"].shape[:2]
    dropped = 0
    for t in range(T):
        differ = (got["acts"][t, :, 0] != want["acts"][t, :, 0]) & alive
        assert not (differ & ~borderline[t]).any(), "%s step %d: a non-borderline action differs" % (label, t)
        dropped += int(differ.sum())
        alive &= ~differ
        for k, (rtol, atol) in TOL.items():
            if k not in want:
                continue
            err = np.abs(got[k][t][alive] - want[k][t][alive])
            print("%s step %d %s: max abs err %.3e" % (label, t, k, err.max() if err.size else 0.0))
            np.testing.assert_allclose(got[k][t][alive], want[k][t][alive], rtol=rtol, atol=atol,
                                       err_msg="%s: %s at step %d" % (label, k, t))
    return dropped


# ---------------------------------------------------------------- route
def test_route_is_the_fused_rollout_for_64_wide_nets(monkeypatch):
    monkeypatch.delenv("TRL_GENERIC_PPO", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.delenv("TRL_NO_RT_ROLLOUT", raising=False)
    c = rr.PAIR_CASES[0]
    col = make_collector(c, 16, 4, 5)[4]
    assert col._spec is not None and col._cat
    assert tuple(col._spec[:3]) == (17, 64, 6)
    assert make_collector(c, 16, 4, 5, hidden=(24, 40))[4]._spec is None     # no mlp2 pair: per-step
    monkeypatch.setenv("TRL_GENERIC_PPO", "1")
    col = make_collector(c, 16, 4, 5)[4]
    assert col._spec is None and col._cat
    monkeypatch.delenv("TRL_GENERIC_PPO")
    monkeypatch.delenv(SWITCH)
    assert make_collector(c, 16, 4, 5)[4]._spec is None                     # without the switch: the per-step route


# ---------------------------------------------------------------- fused vs per-step
@pytest.mark.parametrize("c", rr.PAIR_CASES, ids=rr.case_id)
def test_fused_rollout_vs_per_step_route(c, monkeypatch):
    fused_vs_per_step(c, rr.PAIR_N, rr.PAIR_T, rr.PAIR_HORIZON, rr.PAIR_EPOCHS, monkeypatch)


def test_fused_rollout_vs_per_step_route_wide_relu_partial_tile(monkeypatch):
    fused_vs_per_step(rr.WIDE_RELU_CASE, rr.WIDE_RELU_N, rr.WIDE_RELU_T, rr.WIDE_RELU_HORIZON, rr.PAIR_EPOCHS, monkeypatch)


def fused_vs_per_step(c, N, T, horizon, epochs, monkeypatch):
    monkeypatch.delenv("TRL_GENERIC_PPO", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    pf, vf, env, buf, col = make_collector(c, N, T, horizon)
    assert col._spec is not None
    fused = collect(col, buf, epochs)
    monkeypatch.setenv("TRL_GENERIC_PPO", "1")
    pf2, vf2, env2, buf2, col2 = make_collector(c, N, T, horizon)
    assert col2._spec is None
    step = collect(col2, buf2, epochs)
    assert col.global_step == col2.global_step == epochs * T
    cpf = rr.restated(pf2, c["act"])
    alive = np.ones(N, dtype=bool)
    dropped = 0
    for e in range(epochs):
        assert fused[e]["acts"].shape == (T, N, 1)
        border = np.zeros((T, N), dtype=bool)
        with torch.no_grad():
            for t in range(T):                                             # borderline rows of the per-step run's own inputs
                u = ref.uniforms(col2._noise_seed, e * T + t, 1, N)[0]
                _, _, pre, S = ref.cat_act(cpf(torch.from_numpy(step[e]["obs"][t])), u)
                border[t] = ref.borderline(u, pre, S).numpy()
        dropped += compare_rollouts(fused[e], step[e], border, alive, "%s epoch %d" % (rr.case_id(c), e))
        assert len(fused[e]["episodes"]) == len(step[e]["episodes"])     # (episode ends do not depend on the actions)
        if dropped == 0:
            # (T * N rewards within 1e-5 each; an episode sums at most `horizon` of them)
            assert fused[e]["epoch_reward"] == pytest.approx(step[e]["epoch_reward"], abs=1e-5 * T * N)
            np.testing.assert_allclose(fused[e]["episodes"], step[e]["episodes"], rtol=0, atol=1e-5 * horizon)
    print("%s: envs dropped after a borderline draw: %d" % (rr.case_id(c), dropped))
    assert dropped <= rr.BORDERLINE_CAP * epochs * T * N
    tl, term = step[0]["time_limits"].sum(), step[0]["terminals"].sum()
    assert term > 0 and (tl == 0 if c["max_frames"] < horizon else tl == term)
    assert len(set(fused[0]["acts"].reshape(-1).tolist())) > 1


# ---------------------------------------------------------------- fused vs CPU stepping
def test_fused_rollout_vs_cpu_stepping(monkeypatch):
    monkeypatch.delenv("TRL_GENERIC_PPO", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    c, N, T, horizon = rr.CPU_CASE, rr.CPU_N, rr.CPU_T, rr.CPU_HORIZON
    pf, vf, env, buf, col = make_collector(c, N, T, horizon)
    assert col._spec is not None and col._cat
    want = rr.cpu_rollout(c, N, T, horizon, nets=(pf, vf))
    got = collect(col, buf, 1)[0]
    alive = np.ones(N, dtype=bool)
    dropped = compare_rollouts(got, want, want["borderline"], alive, "cpu")
    print("envs dropped after a borderline draw: %d" % dropped)
    assert dropped <= rr.BORDERLINE_CAP * T * N
    assert got["terminals"].sum() > 0 and np.isfinite(got["epoch_reward"])
    if dropped == 0:
        assert got["epoch_reward"] == pytest.approx(float(np.sum(want["epoch_reward"])), abs=1e-5 * T * N)
        np.testing.assert_allclose(got["episodes"], [r for _, _, r in want["episodes"]], rtol=0, atol=1e-5 * horizon)


# ---------------------------------------------------------------- evaluation
def test_eval_on_the_fused_route_equals_the_per_step_route(monkeypatch):
    c, N, horizon = rr.PAIR_CASES[0], rr.PAIR_N, rr.PAIR_HORIZON
    monkeypatch.delenv("TRL_GENERIC_PPO", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    col = make_collector(c, N, 4, horizon)[4]
    assert col._spec is not None
    ev = col.eval_one_epoch()
    col.eval_env.seed(0)                                                   # (every reset starts the env's NEXT episode: rewind it)
    again = col.eval_one_epoch()
    monkeypatch.setenv("TRL_GENERIC_PPO", "1")
    col2 = make_collector(c, N, 4, horizon)[4]
    assert col2._spec is None
    ev2 = col2.eval_one_epoch()
    assert len(ev["eval_rewards"]) == N and ev["eval_traj_length"] == ev2["eval_traj_length"] == horizon
    np.testing.assert_allclose(ev["eval_rewards"], ev2["eval_rewards"], rtol=0, atol=1e-5 * horizon)
    assert [float(x) for x in ev["eval_rewards"]] == [float(x) for x in again["eval_rewards"]]   # deterministic
    assert col.global_step == 0 and col.replay_buffer._top == 0            # nothing stored, no noise consumed


# ---------------------------------------------------------------- whole iterations
@pytest.mark.parametrize("algo", ["PPO", "A2C"])
def test_whole_iterations_on_the_fused_collection(algo, monkeypatch):
    from torchrl_amd import _C, algo as algos
    monkeypatch.delenv("TRL_GENERIC_PPO", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    N, T, B = 32, 16, 256
    np.random.seed(4)
    pf, vf, env, buf, col = make_collector(dict(rr.PAIR_CASES[0], max_frames=999), N, T, 9)
    assert col._spec is not None
    logger = _Log()
    general = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, gae=True, env=env, replay_buffer=buf,
                   collector=col, logger=logger, device=DEV, save_dir=None)
    if algo == "PPO":
        agent = algos.PPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, entropy_coeff=0.005, **general)
    else:
        agent = algos.A2C(pf=pf, vf=vf, plr=3e-4, vlr=1e-3, entropy_coeff=0.01, **general)
    before = _C.eager_fallback_count()
    p0 = torch.cat([p.detach().reshape(-1) for p in pf.parameters()]).clone()
    for epoch in range(2):
        res = col.train_one_epoch()
        agent.current_epoch = epoch
        agent.update_per_epoch()
        assert np.isfinite(res["train_epoch_reward"]) and len(res["train_rewards"]) > 0
    torch.cuda.synchronize()
    assert len(logger.infos) > 0 and all(np.isfinite(list(i.values())).all() for i in logger.infos)
    if algo == "PPO":
        # log pi_old is the rollout kernel's, log pi the update's dense-layer kernels': logits of magnitude <~ 32 (ulp 4e-6)
        # from 64-term sums in two orders agree to a few ulp, so the first minibatch's ratio is exp(+-~1e-5)
        assert abs(logger.infos[0]["ratio/max"] - 1.0) <= 1e-4 and abs(logger.infos[0]["ratio/min"] - 1.0) <= 1e-4
    assert _C.eager_fallback_count() == before
    assert type(agent.engine()).__name__ == "_GenericPPO" and agent.engine().categorical
    assert col._spec is not None and buf._acts.shape == (T, N, 1)
    assert not torch.equal(p0, torch.cat([p.detach().reshape(-1) for p in pf.parameters()]))
