"""One-launch rollouts for state-dependent-std Gaussian policies (trl_rollout_synth_sd_f32): the collector's choice of
route, the fused rollout against the per-step route and against CPU stepping, single steps with stress heads against the
float64 restatement, greedy evaluation, and whole PPO / A2C iterations on the fused collection + the generic update engine.
The route test fails on a build without the state-dependent-std head.

Device noise: the persistent kernel draws Philox keyed by (env seed, global step) while the per-step route draws one block
keyed by the collector's noise seed, so the two routes are compared on the SAME values -- the per-step collector is handed
the kernel's stream, restated by oracle.philox (tests/_gauss_sd_rollout_ref.py::device_noise), as its noise block."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_sd_rollout_ref as rr                                            # noqa: E402

pytestmark = pytest.mark.gpu
SWITCH = "TRL_SD_FUSED_ROLLOUT"                                               # the fused route is opt-in
DEV = torch.device("cuda:0")
RING_KEYS = ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits", "old_logp")


class _Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


def make_collector(c, N, T, horizon, hidden=(64, 64), noise_mode="device", obs_norm=False):
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.env.synth import SynthVecEnv
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    D, A = c["D"], c["A"]
    pf, vf = rr.nets_of(c, hidden=hidden)
    if (D, A) == (17, 6):
        env, eval_env = (get_vec_env("SynthHalfCheetah-v0", {"reward_scale": 1, "obs_norm": obs_norm}, N, device=DEV)
                         for _ in range(2))
    else:
        env, eval_env = (SynthVecEnv(N, obs_dim=D, act_dim=A, device=DEV) for _ in range(2))
    for e in (env, eval_env):
        e.horizon = horizon
    env.seed(c["env_seed"])
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               epoch_frames=N * T, max_episode_frames=c["max_frames"], eval_episodes=1, noise_mode=noise_mode)
    return pf, vf, env, buf, col


def collect(col, buf, epochs):
    out = []
    for _ in range(epochs):
        res = col.train_one_epoch()
        snap = {k: getattr(buf, "_" + k).cpu().numpy().copy() for k in RING_KEYS}
        snap["epoch_reward"] = float(res["train_epoch_reward"])
        snap["episodes"] = [float(x) for x in res["train_rewards"]]
        out.append(snap)
    return out


def per_step_collector(c, N, T, horizon, mode, monkeypatch):
    """The per-step route on the noise the fused route of `mode` consumes (see the module docstring)."""
    monkeypatch.setenv("TRL_GENERIC_PPO", "1")
    pf, vf, env, buf, col = make_collector(c, N, T, horizon, noise_mode="host")
    monkeypatch.delenv("TRL_GENERIC_PPO")
    assert col._spec is None and col._sd
    if mode == "device":
        def kernel_stream(n_steps, env_):
            return rr.device_noise(n_steps, N, c["A"], c["env_seed"], step0=col.global_step).to(DEV).contiguous()
        col._host_noise = kernel_stream
    return pf, vf, env, buf, col


def report(label, got, want, tol=rr.TOL):
    worst = {}
    for k, (rtol, atol) in tol.items():
        worst[k] = rr.worst_ratio(got[k], want[k], rtol, atol)
        print("%s %s: max abs err %.3e, worst err / bound %.4f" % (label, k, worst[k][1], worst[k][0]))
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    assert not bad, (label, bad)


# ---------------------------------------------------------------- route
def test_route_is_the_fused_rollout_for_64_wide_nets(monkeypatch):
    monkeypatch.delenv("TRL_GENERIC_PPO", raising=False)
    monkeypatch.delenv("TRL_NO_RT_ROLLOUT", raising=False)
    monkeypatch.delenv("TRL_PREFETCH_NOISE", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    c = rr.PAIR_CASES[0]
    col = make_collector(c, 16, 4, 5)[4]
    assert col._spec is not None and col._sd and not col._cat and col._mlp2 is None
    assert tuple(col._spec[:3]) == (17, 64, 6) and col._head_w == 12
    assert make_collector(c, 16, 4, 5, hidden=(24, 40))[4]._spec is None     # no mlp2 pair: per-step
    assert make_collector(dict(c, D=17, A=9), 16, 4, 5)[4]._spec is None     # 9 action dims: an 18-row head
    assert make_collector(c, 16, 4, 5, obs_norm=True)[4]._spec is None       # running observation normaliser
    monkeypatch.setenv("TRL_GENERIC_PPO", "1")
    col = make_collector(c, 16, 4, 5)[4]
    assert col._spec is None and col._sd
    monkeypatch.delenv("TRL_GENERIC_PPO")
    monkeypatch.delenv(SWITCH)
    for case in rr.PAIR_CASES[:4]:
        assert make_collector(case, 16, 4, 5)[4]._spec is None              # without the switch: the per-step route


# ---------------------------------------------------------------- fused vs per-step
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("c", rr.PAIR_CASES, ids=rr.case_id)
def test_fused_rollout_vs_per_step_route(c, mode, monkeypatch):
    fused_vs_per_step(c, mode, rr.PAIR_N, rr.PAIR_T, rr.PAIR_HORIZON, rr.PAIR_EPOCHS, monkeypatch)


@pytest.mark.parametrize("c", rr.WIDE_RELU_CASES, ids=rr.case_id)
def test_fused_rollout_vs_per_step_route_wide_relu_partial_tile(c, monkeypatch):
    fused_vs_per_step(c, "device", rr.WIDE_RELU_N, rr.WIDE_RELU_T, rr.WIDE_RELU_HORIZON, rr.PAIR_EPOCHS, monkeypatch)


def fused_vs_per_step(c, mode, N, T, horizon, epochs, monkeypatch):
    monkeypatch.delenv("TRL_GENERIC_PPO", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    pf, vf, env, buf, col = make_collector(c, N, T, horizon, noise_mode=mode)
    assert col._spec is not None and col._sd
    torch.manual_seed(rr.HOST_SEED)
    fused = collect(col, buf, epochs)
    pf2, vf2, env2, buf2, col2 = per_step_collector(c, N, T, horizon, mode, monkeypatch)
    torch.manual_seed(rr.HOST_SEED)
    step = collect(col2, buf2, epochs)
    assert col.global_step == col2.global_step == epochs * T
    for e in range(epochs):
        assert fused[e]["acts"].shape == (T, N, c["A"])
        report("%s %s epoch %d" % (rr.case_id(c), mode, e), fused[e], step[e])
        assert len(fused[e]["episodes"]) == len(step[e]["episodes"])
        # (T * N rewards within 1e-5 each; an episode sums at most `horizon` of them)
        assert fused[e]["epoch_reward"] == pytest.approx(step[e]["epoch_reward"], abs=1e-5 * T * N)
        np.testing.assert_allclose(fused[e]["episodes"], step[e]["episodes"], rtol=0, atol=1e-5 * horizon)
    tl, term = step[0]["time_limits"].sum(), step[0]["terminals"].sum()
    assert term > 0 and (tl == 0 if c["max_frames"] < horizon else tl == term)
    assert fused[0]["terminals"].sum() == term and np.abs(fused[0]["acts"]).std() > 0.1   # the noise reached the actions
    assert not np.array_equal(fused[0]["acts"], fused[1]["acts"])          # ... and moved on between the epochs


# ---------------------------------------------------------------- single steps, stress heads
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("c", rr.STRESS_CASES, ids=rr.case_id)
def test_steps_with_stress_heads_vs_float64_restatement(c, mode, monkeypatch):
    """Every stored (t, n) against the float64 restatement of the ring's OWN obs[t, n] and the step's noise (no error
    accumulates), with the bounds a head error of 1e-5 * (1 + |head element|) allows (_gauss_sd_rollout_ref.step_terms);
    log pi_old against trl_gauss_sd_logp_f32 on the dense-layer head of the same obs and the stored action -- what
    PPO._fill_old_logp would have written -- except on rows with an element on the lower clamp (std = e^-20:
    ill-conditioned), which must be finite.

    Measured (worst err / bound over the four cases and both noise modes): see profiles/NOTES_state_std_rollout.md."""
    from torchrl_amd import _C, ops
    N, T, A = rr.STRESS_N, rr.STRESS_T, c["A"]
    monkeypatch.delenv("TRL_GENERIC_PPO", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    pf, vf, env, buf, col = make_collector(c, N, T, rr.STRESS_HORIZON, noise_mode=mode)
    assert col._spec is not None and col._sd
    torch.manual_seed(rr.HOST_SEED)
    got = collect(col, buf, 1)[0]
    eps = rr.noise_of(mode, T, N, A, c["env_seed"]).reshape(T * N, A).numpy()
    flat = lambda k: got[k].reshape(T * N, -1)
    want = rr.step_terms(c, rr.params_of(pf, torch.float64), flat("obs"), eps, reward_scale=float(env.effective_reward_scale))
    label = "%s %s" % (rr.case_id(c), mode)
    worst = {}
    for k, ring, b in (("act", flat("acts"), want["b_act"]), ("next_obs", flat("next_obs"), want["b_next"]),
                       ("reward", flat("rewards")[:, 0], want["b_rew"])):
        err = np.abs(ring.astype(np.float64) - want[k])
        worst[k] = (float((err / b).max()), float(err.max()))
    low = want["raw"] <= -20.0
    hi_share, lo_share = float((want["raw"] >= 2.0).mean()), float(low.mean())
    print("%s: share at +2 %.4f, at -20 %.4f" % (label, hi_share, lo_share))
    assert c["share_hi"][0] <= hi_share <= c["share_hi"][1]
    assert lo_share <= c["share_lo"][1] + 1e-12                              # no more exempted than the asserted clamp share
    keep = ~low.any(axis=1)
    with torch.no_grad():
        head, _ = ops.mlp_forward(ops.linear_layers(pf), buf._obs.reshape(T * N, -1).contiguous(), ops.act_code(pf), keep=False)
        lp, _ = _C.gauss_sd_logp(head, buf._acts.reshape(T * N, -1).contiguous(), False)
    if keep.any():
        worst["old_logp"] = rr.worst_ratio(flat("old_logp")[keep, 0], lp.cpu().numpy()[keep], 1e-4, 2e-3)
    assert keep.all() == (c["stress"] == "span")
    for k, (ratio, err) in worst.items():
        print("%s %s: max abs err %.3e, worst err / bound %.4f" % (label, k, err, ratio))
    assert all(np.isfinite(got[k]).all() for k in RING_KEYS)
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    assert not bad, (label, bad)
    assert got["terminals"].sum() > 0 and got["time_limits"].sum() == got["terminals"].sum()


# ---------------------------------------------------------------- fused vs CPU stepping
def test_fused_rollout_vs_cpu_stepping(monkeypatch):
    monkeypatch.delenv("TRL_GENERIC_PPO", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    c, N, T, horizon = rr.CPU_CASE, rr.CPU_N, rr.CPU_T, rr.CPU_HORIZON
    pf, vf, env, buf, col = make_collector(c, N, T, horizon, noise_mode="host")
    assert col._spec is not None and col._sd
    want = rr.cpu_rollout(c, N, T, horizon, (pf, vf), rr.host_noise(T, N, c["A"]))
    torch.manual_seed(rr.HOST_SEED)
    got = collect(col, buf, 1)[0]
    report("cpu", got, want)
    assert got["terminals"].sum() > 0 and got["time_limits"].sum() == got["terminals"].sum()
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
    print("eval: max abs err %.3e (bound %.1e)" % (np.abs(np.array(ev["eval_rewards"]) - np.array(ev2["eval_rewards"])).max(),
                                                   1e-5 * horizon))
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
    pf, vf, env, buf, col = make_collector(rr.PAIR_CASES[0], N, T, 9)
    assert col._spec is not None and col._sd
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
        # log pi_old is the rollout kernel's (head rows summed over four waves' partial tiles), log pi the update's
        # dense-layer kernels': the two summation orders agree to a few ulp of a head element, so the ratio is exp(+-~1e-5)
        print("first minibatch: ratio/max %.9f ratio/min %.9f" % (logger.infos[0]["ratio/max"], logger.infos[0]["ratio/min"]))
        assert abs(logger.infos[0]["ratio/max"] - 1.0) <= 1e-4 and abs(logger.infos[0]["ratio/min"] - 1.0) <= 1e-4
    assert _C.eager_fallback_count() == before
    eng = agent.engine()
    assert type(eng).__name__ == "_GenericPPO" and eng.state_std and not eng.categorical
    assert col._spec is not None and buf._acts.shape == (T, N, 6)
    assert not torch.equal(p0, torch.cat([p.detach().reshape(-1) for p in pf.parameters()]))
