"""One-launch rollouts for `add_ln=True` networks (trl_rollout_synth_ln_f32; rollout_kernel / value_pass_kernel with LN = true,
torchrl_amd/csrc/trl_rollout.h): every stored cell against the float64 restatement of the launch's own observations, the
collector's route, the fused collection against the per-step one, and whole PPO / A2C iterations.  The float32 numpy
restatement is held to the same bounds without a GPU (the one test here that is not marked `gpu`).

Measured worst err / bound per quantity: profiles/NOTES_layernorm_rollout.md."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_sd_rollout_ref as rr                                            # noqa: E402
import _layernorm_rollout_ref as L                                            # noqa: E402
from _rollout_ref import F32, U                                               # noqa: E402

SWITCH = "TRL_LN_FUSED_ROLLOUT"                                               # the fused route is opt-in
RING_KEYS = ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits", "old_logp")
T_CELLS, HORIZON, MAX_FRAMES = 3, 5, 2                # every env passes max_episode_frames in step 1: bootstrapped cells, no done


def case(head, D, A, act, N, pf_ln, vf_ln, seed, tanh=True, zero=False, plant=None):
    return dict(head=head, D=D, A=A, act=act, N=N, pf_ln=pf_ln, vf_ln=vf_ln, seed=seed, tanh=tanh and head != "cat", zero=zero,
                plant=plant, logstd=np.full(A, -1.5))


# pairwise over D in {3, 17, 27} x A in {1, 6, 8} x act x head x (policy LN, critic LN) x N in {16, 17}; a ZeroNet critic;
# the two planted first layers (zero variance: W1 = 0, constant b1; large mean: ReLU, b1 = 64 + U(-0.5, 0.5))
CELL_CASES = [case("gauss", 3, 1, "tanh", 16, 1, 1, 1), case("gauss", 17, 6, "relu", 17, 1, 0, 2, tanh=False),
              case("gauss", 27, 8, "tanh", 17, 0, 1, 3), case("cat", 3, 6, "relu", 17, 1, 1, 4), case("cat", 17, 8, "tanh", 16, 0, 1, 5),
              case("cat", 27, 6, "tanh", 17, 1, 0, 6), case("sd", 3, 8, "tanh", 17, 1, 0, 7), case("sd", 17, 1, "relu", 16, 0, 1, 8),
              case("sd", 27, 6, "relu", 17, 1, 1, 9), case("gauss", 17, 6, "tanh", 17, 1, 0, 10, zero=True),
              case("sd", 27, 1, "tanh", 16, 1, 0, 13), case("gauss", 3, 6, "relu", 17, 0, 1, 14),
              case("gauss", 17, 6, "tanh", 16, 1, 1, 11, plant="zero-variance"), case("sd", 27, 6, "relu", 17, 1, 1, 12, plant="large-mean")]
case_id = lambda c: "%s-D%d-A%d-%s-N%d-ln%d%d%s%s" % (c["head"], c["D"], c["A"], c["act"], c["N"], c["pf_ln"], c["vf_ln"],
                                                       "-zeronet" if c["zero"] else "", "-" + c["plant"] if c["plant"] else "")


def nets_of(c):
    """(pf, vf) on the CPU; gamma in +-[0.5, 2], beta in [-1, 1], heads scaled to outputs of a few tenths."""
    from torchrl_amd import networks, policies
    torch.manual_seed(c["seed"])
    D, A = c["D"], c["A"]
    net = lambda ln: dict(hidden_shapes=[64, 64], append_hidden_shapes=[], base_type=networks.MLPBase, add_ln=bool(ln),
                          activation_func={"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}[c["act"]])
    if c["head"] == "gauss":
        pf = policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=c["tanh"], **net(c["pf_ln"]))
    elif c["head"] == "cat":
        pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net(c["pf_ln"]))
    else:
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=c["tanh"], **net(c["pf_ln"]))
    vf = networks.ZeroNet() if c["zero"] else networks.Net(input_shape=(D,), output_shape=1, **net(c["vf_ln"]))
    with torch.no_grad():
        for n_ in (pf, vf):
            for m in n_.modules():
                if isinstance(m, torch.nn.LayerNorm):
                    m.weight.copy_((0.5 + 1.5 * torch.rand(64)) * (1.0 - 2.0 * (torch.rand(64) < 0.3).float()))
                    m.bias.uniform_(-1.0, 1.0)
            if not isinstance(n_, networks.ZeroNet):
                first, last = n_.base.seq_fcs[0], n_.seq_append_fcs[-1]
                last.weight.mul_(30.0)
                if c["plant"] == "zero-variance":
                    first.weight.zero_()
                    first.bias.fill_(0.3)
                elif c["plant"] == "large-mean":
                    first.bias.copy_(64.0 + torch.rand(64) - 0.5)
        if c["head"] == "gauss":
            pf.logstd.fill_(-1.5)
        elif c["head"] == "sd":
            pf.seq_append_fcs[-1].bias[A:].fill_(-1.5)
    return pf, vf


def make_collector(c, N, T, horizon, max_frames, noise_mode=None, obs_norm=False):
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.env.synth import SynthVecEnv
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    dev = torch.device("cuda:0")
    pf, vf = nets_of(c)
    if obs_norm:
        env, eval_env = (get_vec_env("SynthHalfCheetah-v0", {"reward_scale": 1, "obs_norm": True}, N, device=dev) for _ in range(2))
    else:
        env, eval_env = (SynthVecEnv(N, obs_dim=c["D"], act_dim=c["A"], device=dev, discrete=c["head"] == "cat") for _ in range(2))
    for e in (env, eval_env):
        e.horizon = horizon
    env.seed(c["seed"])
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=dev, train_render=False,
                               epoch_frames=N * T, max_episode_frames=max_frames, eval_episodes=1,
                               noise_mode=noise_mode or ("device" if c["head"] == "cat" else "host"))
    return pf, vf, env, buf, col


def collect(col, buf):
    torch.manual_seed(rr.HOST_SEED)
    res = col.train_one_epoch()
    snap = {k: getattr(buf, "_" + k).cpu().numpy().copy() for k in RING_KEYS}
    snap.update(epoch_reward=float(res["train_epoch_reward"]), episodes=[float(x) for x in res["train_rewards"]])
    return snap


def clean_env(monkeypatch, switch=True):
    for k in ("TRL_GENERIC_PPO", "TRL_NO_RT_ROLLOUT", "TRL_PREFETCH_NOISE", SWITCH):
        monkeypatch.delenv(k, raising=False)
    if switch:
        monkeypatch.setenv(SWITCH, "1")


def noise_of(c, T, N):
    if c["head"] == "cat":
        return L.uniforms(0, T, N).reshape(T * N, 1)
    return rr.host_noise(T, N, c["A"]).numpy().reshape(T * N, c["A"])


# ---------------------------------------------------------------- 1. stored cells against float64
def test_float32_restatement_stays_inside_the_bounds():
    """The bounds come from the float64 restatement alone; the same restatement in float32 numpy must fit them on every case,
    planted rows included (no GPU)."""
    for c in CELL_CASES:
        pf, vf = nets_of(c)
        P, V = L.params_of(pf), None if c["zero"] else L.params_of(vf)
        rs = np.random.RandomState(c["seed"])
        M = 3 * c["N"]
        obs, nxt = (0.5 * rs.randn(M, c["D"])).astype(np.float32), np.tanh(rs.randn(M, c["D"])).astype(np.float32)
        eps = noise_of(c, 3, c["N"])
        if c["head"] == "cat":
            acts = rs.randint(0, c["A"], (M, 1)).astype(np.float32)
        else:
            acts = L.quantities(c, P, V, obs, nxt, eps, np.zeros((M, c["A"])), np.float32)["act"]
        q64, q32 = L.quantities(c, P, V, obs, nxt, eps, acts), L.quantities(c, P, V, obs, nxt, eps, acts, np.float32)
        r = L.ratios(q32, q64)
        print(case_id(c), {k: round(v, 4) for k, v in r.items()})
        assert all(v <= 1.0 for v in r.values()), (case_id(c), r)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CELL_CASES, ids=case_id)
def test_stored_cells_vs_float64_restatement(c, monkeypatch):
    clean_env(monkeypatch)
    N, T, A = c["N"], T_CELLS, c["A"]
    pf, vf, env, buf, col = make_collector(c, N, T, HORIZON, MAX_FRAMES)
    assert col._spec is not None and col._ln == (bool(c["pf_ln"]), bool(c["vf_ln"]))
    g = collect(col, buf)
    assert all(np.isfinite(g[k]).all() for k in RING_KEYS)
    flat = lambda k: g[k].reshape(T * N, -1)
    over = flat("terminals")[:, 0] == 1.0
    assert over.reshape(T, N)[1].all() and over.sum() == N and g["time_limits"].sum() == 0
    q = L.quantities(c, L.params_of(pf), None if c["zero"] else L.params_of(vf), flat("obs"), flat("next_obs"), noise_of(c, T, N),
                     flat("acts"))
    got = dict(logp=flat("old_logp")[:, 0], v=flat("values")[:, 0])
    if c["head"] == "cat":
        assert q["allowed"].all(), "a stored index is neither the restated draw nor its neighbour across a close prefix sum"
    else:
        got["act"] = flat("acts")
    r = L.ratios(got, q)
    if c["plant"] == "zero-variance":                                  # the normed row is beta exactly, whatever the input
        assert np.ptp(q["v"]) == 0.0 and np.ptp(flat("values")) <= 2.0 * q["b_v"][0]
    # rewards: the raw reward from the stored next_obs / actions, + discount V(next_obs) on the over-length cells; boot
    a = np.ones((T * N, 1)) if c["head"] == "cat" else flat("acts").astype(np.float64)
    asq, scale, disc = (a * a).sum(-1), F32(env.effective_reward_scale), F32(col.discount)
    raw = flat("next_obs")[:, 0].astype(np.float64) - F32(0.1) * asq
    want = scale * raw + over * disc * q["v2"]
    b = scale * U * (6.0 * F32(0.1) * asq + 2.0 * np.abs(raw)) + over * (disc * q["b_v2"] + U * (np.abs(disc * q["v2"]) + np.abs(want)))
    r["rewards"] = float((np.abs(flat("rewards")[:, 0] - want) / b).max())
    last = slice((T - 1) * N, T * N)
    r["boot"] = float((np.abs(buf._boot.cpu().numpy().reshape(N) - q["v2"][last]) / q["b_v2"][last]).max())
    print(case_id(c), {k: round(v, 4) for k, v in r.items()})
    assert all(v <= 1.0 for v in r.values()), r


# ---------------------------------------------------------------- 2. route
@pytest.mark.gpu
def test_route(monkeypatch):
    from torchrl_amd import _C, algo as algos
    clean_env(monkeypatch)
    c = CELL_CASES[0]
    pf, vf, env, buf, col = make_collector(dict(c, D=17, A=6), 16, 4, 9, 99)
    assert col._spec == (17, 64, 6, _C.ACT_TANH) and col._ln == (True, True) and col._mlp2 is None   # (None on the parent)
    assert pf.mlp2_spec() is None and pf.mlp2_ln_spec() == (17, 64, 6, _C.ACT_TANH)
    agent = algos.PPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=1, entropy_coeff=0.0, tau=0.95, shuffle=True,
                      discount=0.99, num_epochs=1, batch_size=32, gae=True, env=env, replay_buffer=buf, collector=col,
                      logger=None, device=torch.device("cuda:0"), save_dir=None)
    eng = agent.engine()
    calls = []
    real = _C.rollout_ln
    monkeypatch.setattr(_C, "rollout_ln", lambda *a: (calls.append(a[1:4]), real(*a))[1])
    monkeypatch.setattr(col, "_step_launches", lambda *a, **k: pytest.fail("a per-step launch sequence on the fused route"))
    for _ in range(2):
        assert pf.flat_plan_params().data_ptr() == eng.flat.data_ptr()
        assert vf.flat_plan_params().data_ptr() == eng.flat.data_ptr() + 4 * eng.P_pf
        assert pf.flat_plan_params().numel() == eng.P_pf and vf.flat_plan_params().numel() == eng.P_vf
        col.train_one_epoch()
    assert calls == [(0, True, True)] * 2
    monkeypatch.undo()
    clean_env(monkeypatch, switch=False)
    assert make_collector(c, 16, 4, 9, 99)[4]._spec is None              # without the switch: the per-step route
    clean_env(monkeypatch)
    assert make_collector(dict(c, D=17, A=6), 16, 4, 9, 99, obs_norm=True)[4]._spec is None   # a running observation normaliser
    a = _C.RolloutArgs()
    a.norm_state = 64
    with pytest.raises(_C.TrlError, match="no running observation normaliser"):
        _C.rollout_ln(a, 0, True, True, 0, 0, torch.device("cuda:0"))


# ---------------------------------------------------------------- 3. fused against per-step collection
PAIR_CASES = [case(h, D, A, act, 33, 1, 1, 20 + k) for k, (h, D, A, act) in enumerate(
    [("gauss", 17, 6, "tanh"), ("gauss", 27, 8, "relu"), ("cat", 17, 6, "tanh"), ("cat", 27, 8, "relu"), ("sd", 17, 6, "tanh"),
     ("sd", 27, 8, "relu")])]


@pytest.mark.gpu
@pytest.mark.parametrize("c", PAIR_CASES, ids=case_id)
def test_fused_vs_per_step_collection(c, monkeypatch):
    """Same nets, same device Philox noise (the per-step Gaussian route is handed the kernel's stream, as in
    tests/test_gauss_sd_rollout_gpu.py); ring and env state at that test's tolerances; greedy evaluation on both routes."""
    N, T, horizon = 33, 4, 3
    clean_env(monkeypatch)
    pf, vf, env, buf, col = make_collector(c, N, T, horizon, 999, noise_mode="device")
    assert col._spec is not None and col._ln == (True, True)
    fused, ev = collect(col, buf), col.eval_one_epoch()
    clean_env(monkeypatch, switch=False)
    pf2, vf2, env2, buf2, col2 = make_collector(c, N, T, horizon, 999, noise_mode="device" if c["head"] == "cat" else "host")
    assert col2._spec is None
    if c["head"] != "cat":
        col2._host_noise = lambda n, e: rr.device_noise(n, N, c["A"], c["seed"], step0=col2.global_step).to(e.device).contiguous()
    step, ev2 = collect(col2, buf2), col2.eval_one_epoch()
    for k, (rtol, atol) in rr.TOL.items():
        ratio, err = rr.worst_ratio(fused[k], step[k], rtol, atol)
        print("%s %s: max abs err %.3e, worst err / bound %.4f" % (case_id(c), k, err, ratio))
        assert ratio <= 1.0, k
    assert fused["terminals"].sum() > 0 and fused["episodes"] and len(fused["episodes"]) == len(step["episodes"])
    np.testing.assert_allclose(fused["episodes"], step["episodes"], rtol=0, atol=1e-5 * horizon)
    assert fused["epoch_reward"] == pytest.approx(step["epoch_reward"], abs=1e-5 * T * N)
    np.testing.assert_allclose(env.cur_obs.cpu().numpy(), env2.cur_obs.cpu().numpy(), rtol=0, atol=1e-5)
    for k in ("t_env", "cur_step", "episode_idx"):
        assert torch.equal(getattr(env, k).cpu(), getattr(env2, k).cpu()), k
    np.testing.assert_allclose(env.ep_return.cpu().numpy(), env2.ep_return.cpu().numpy(), rtol=0, atol=1e-5 * horizon)
    assert len(ev["eval_rewards"]) == N and ev["eval_traj_length"] == ev2["eval_traj_length"] == horizon
    np.testing.assert_allclose(ev["eval_rewards"], ev2["eval_rewards"], rtol=0, atol=1e-5 * horizon)


# ---------------------------------------------------------------- 4. whole iterations
class _Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["PPO", "A2C"])
def test_whole_iterations_on_the_fused_collection(algo, monkeypatch):
    from torchrl_amd import _C, algo as algos
    clean_env(monkeypatch)
    N, T = 32, 16
    np.random.seed(4)
    pf, vf, env, buf, col = make_collector(case("gauss", 17, 6, "tanh", N, 1, 1, 30), N, T, 9, 999, noise_mode="device")
    assert col._spec is not None and col._ln == (True, True)
    logger = _Log()
    general = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=256, gae=True, env=env, replay_buffer=buf,
                   collector=col, logger=logger, device=torch.device("cuda:0"), save_dir=None)
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
    assert _C.eager_fallback_count() == before and col._spec is not None
    assert not torch.equal(p0, torch.cat([p.detach().reshape(-1) for p in pf.parameters()]))
