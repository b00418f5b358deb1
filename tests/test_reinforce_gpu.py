"""REINFORCE, the product: `Reinforce.update` against what the REFERENCE's Reinforce.update produced
(tests/golden/reinforce_update.npz) for the three policy heads, the fused engine against the generic one, an `add_ln` policy
against float64 autograd, and collect + update iterations with the vacant critic through the fused rollout, the per-step
collector and the single-env collector."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _ppo_update_ref as pref                                                # noqa: E402
import _reinforce_ref as R                                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SWITCHES = ("TRL_GENERIC_PPO", "TRL_NO_GRAPH", "TRL_NO_RT_ROLLOUT", "TRL_CAT_FUSED_UPDATE", "TRL_SD_FUSED_UPDATE",
            "TRL_CAT_FUSED_ROLLOUT", "TRL_SD_FUSED_ROLLOUT")


class _Stub:
    epoch_frames = 0


class ListLogger:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "reinforce_update.npz"))


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def policy_of(head, D, A, hidden, add_ln=False, seed=0):
    from torchrl_amd import networks, policies
    torch.manual_seed(seed)
    net = dict(hidden_shapes=list(hidden), append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh,
               add_ln=add_ln)
    if head == "gauss":
        return policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=True, **net)
    if head == "sd":
        return policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net)
    return policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)


def fixture_agent(g, tag):
    from torchrl_amd.algo import Reinforce
    from torchrl_amd.env.synth import SynthVecEnv
    D, A, Hh, B = (int(x) for x in g[f"{tag}_args"][:4])
    plr, ent = (float(x) for x in g[f"{tag}_hyper"])
    pf = policy_of(R.HEADS[tag], D, A, (Hh, Hh))
    prefix = f"{tag}_pf0_"
    pf.load_state_dict({k[len(prefix):].replace("__", "."): torch.from_numpy(g[k].copy()) for k in g.files if k.startswith(prefix)})
    agent = Reinforce(pf=pf, plr=plr, entropy_coeff=ent, shuffle=True, discount=0.99, num_epochs=10, batch_size=B,
                      env=SynthVecEnv(4, device=DEV), replay_buffer=None, collector=_Stub(), logger=ListLogger(), device=DEV,
                      save_dir=None)
    return agent, pf


def state_errors(g, prefix, tensors_by_name):
    return max(float(np.abs(t.detach().cpu().numpy().astype(np.float64) - g[prefix + n.replace(".", "__")]).max())
               for n, t in tensors_by_name)


def run_fixture(g, tag, errlog=None):
    """Two chained updates against the fixture at SURVEY a11's bounds: info scalars rel 1e-4 / abs 1e-5 in the reference's key
    order, parameters abs 1e-6 per update, Adam's moments (read through the torch optimiser object) within the same bound."""
    agent, pf = fixture_agent(g, tag)
    for s in range(2):
        info = agent.update(R.batch_of(g, tag))
        want = R.info_of(g, tag, s)
        assert list(info.keys()) == R.INFO_KEYS == list(want.keys())
        worst = R.info_close(info, want)
        err = state_errors(g, f"{tag}_pf{s + 1}_", pf.state_dict().items())
        st = agent.pf_optimizer.state
        err_m = state_errors(g, f"{tag}_adam{s + 1}_m_", [(n, st[p]["exp_avg"]) for n, p in pf.named_parameters()])
        err_v = state_errors(g, f"{tag}_adam{s + 1}_v_", [(n, st[p]["exp_avg_sq"]) for n, p in pf.named_parameters()])
        print("%s update %d (%s): info err / bound %.3f, params %.3e, exp_avg %.3e, exp_avg_sq %.3e"
              % (tag, s, type(agent.engine()).__name__, worst, err, err_m, err_v))
        assert worst <= 1.0, (info, want)
        assert err <= 1e-6 * (s + 1) and err_m <= 1e-6 and err_v <= 1e-6, (s, err, err_m, err_v)
    assert agent.training_update_num == 2 and all(float(st[p]["step"]) == 2.0 for p in pf.parameters())
    return agent, pf


@pytest.mark.parametrize("tag", list(R.HEADS))
def test_update_matches_the_reference(g, tag):
    agent, pf = run_fixture(g, tag)
    assert type(agent.engine()).__name__ == ("_FusedReinforce" if tag == "g" else "_GenericReinforce")
    assert agent.engine().P_vf == 0 and agent.engine().flat.numel() == sum(p.numel() for p in pf.parameters())
    assert [n for n, _ in agent.snapshot_networks] == ["pf"]


def test_fused_engine_against_the_generic_one(g, monkeypatch):
    """The 17-64-64-6 shared-std shape on both engines from the fixture's (well-conditioned) draw: each holds the fixture's
    bounds, and against each other the bounds tests/test_a2c_gpu.py holds its two engines to (infos rtol 2e-4 / atol 2e-5,
    parameters 2e-6)."""
    assert tuple(int(x) for x in g["g_args"][:3]) == (17, 6, 64)
    fused, pf_f = run_fixture(g, "g")
    monkeypatch.setenv("TRL_GENERIC_PPO", "1")
    generic, pf_g = run_fixture(g, "g")
    assert type(fused.engine()).__name__ == "_FusedReinforce" and type(generic.engine()).__name__ == "_GenericReinforce"
    for (n, a), (_, b) in zip(pf_f.state_dict().items(), pf_g.state_dict().items()):
        assert float((a - b).abs().max()) < 2e-6, n
    monkeypatch.delenv("TRL_GENERIC_PPO")
    i_f, i_g = fused.update(R.batch_of(g, "g")), generic.update(R.batch_of(g, "g"))
    np.testing.assert_allclose([i_f[k] for k in R.INFO_KEYS], [i_g[k] for k in R.INFO_KEYS], rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("head,switch", [("cat", "TRL_CAT_FUSED_UPDATE"), ("sd", "TRL_SD_FUSED_UPDATE")])
def test_opt_in_fused_engine_of_the_other_heads(head, switch, monkeypatch):
    """A 17-64-64 categorical (6 actions) / state-dependent-std (3 dims) policy goes to the generic engine by default and to
    the fused one under the head's existing opt-in.  One update on each from the same parameters: the info dicts within
    rtol 2e-4 / atol 2e-5 (tests/test_a2c_gpu.py's bound for its two engines) and the folded gradients within 1e-4 of the
    largest element (tests/test_categorical_update_gpu.py's bound on a gradient).  The parameters are not compared: with eps
    = 1e-8 the first step of an element with a tiny gradient is decided by that gradient's last bits."""
    from torchrl_amd.algo import Reinforce
    from torchrl_amd.env.synth import SynthVecEnv
    D, A, B = 17, 6 if head == "cat" else 3, 64
    rs = np.random.RandomState(31)
    obs = rs.randn(B, D).astype(np.float32)
    acts = rs.randint(0, A, size=(B,)).astype(np.float32) if head == "cat" else \
        np.tanh(0.5 * rs.randn(B, A)).clip(-0.995, 0.995).astype(np.float32)
    batch = {"obs": obs, "acts": acts, "advs": (rs.randn(B, 1) * 2 + 0.5).astype(np.float32)}
    out = {}
    for route in ("generic", "fused"):
        if route == "fused":
            monkeypatch.setenv(switch, "1")
        agent = Reinforce(pf=policy_of(head, D, A, (64, 64), seed=9), plr=3e-3, entropy_coeff=0.001, shuffle=True,
                          discount=0.99, num_epochs=10, batch_size=B, env=SynthVecEnv(4, device=DEV), replay_buffer=None,
                          collector=_Stub(), logger=ListLogger(), device=DEV, save_dir=None)
        eng = agent.engine()
        assert type(eng).__name__ == ("_FusedReinforce" if route == "fused" else "_GenericReinforce")
        p0 = eng.flat.detach().clone()
        info = agent.update(batch)
        torch.cuda.synchronize()
        assert list(info) == R.INFO_KEYS and not torch.equal(eng.flat, p0) and bool(torch.isfinite(eng.flat).all())
        out[route] = (info, eng.grads.detach().cpu().double(), p0.cpu())
    (i_g, g_g, p_g), (i_f, g_f, p_f) = out["generic"], out["fused"]
    assert torch.equal(p_g, p_f)                                              # the same flat layout, the same start
    np.testing.assert_allclose([i_f[k] for k in R.INFO_KEYS], [i_g[k] for k in R.INFO_KEYS], rtol=2e-4, atol=2e-5)
    err, top = float((g_f - g_g).abs().max()), float(g_g.abs().max())
    print("%s: fused against generic gradient, max abs err %.3e of max %.3e" % (head, err, top))
    assert top > 0 and err <= 1e-4 * top


def test_layernorm_policy_against_float64_autograd():
    """An `add_ln=True` policy (5-32-32-2, shared-std head) on the generic engine.  The engine's folded gradient against torch
    autograd in float64 at the bound of tests/test_layernorm_gpu.py (rel 1e-4 of the element + 1e-5 of the tensor's largest);
    the parameters against a float64 clip + Adam(eps 1e-8) step on THAT gradient within 1e-6 (with eps = 1e-8 the first step
    of an element whose gradient is of the size of eps is decided by the gradient's last bits -- lr g / (|g| + eps) -- so the
    step is checked on the engine's own gradient and the gradient on its own); the info dict rel 1e-4 / abs 1e-5."""
    from torchrl_amd import networks, ops
    from torchrl_amd.algo import Reinforce
    from torchrl_amd.env.synth import SynthVecEnv
    D, A, B, plr, c_ent = 5, 2, 64, 3e-3, 0.001
    pf = policy_of("gauss", D, A, (32, 32), add_ln=True, seed=3)
    cpu = policy_of("gauss", D, A, (32, 32), add_ln=True, seed=3).double()
    rs = np.random.RandomState(12)
    obs = rs.randn(B, D).astype(np.float32)
    with torch.no_grad():
        mean = networks.Net.forward(cpu, torch.from_numpy(obs).double())
        acts = torch.tanh(mean + torch.exp(cpu.logstd) * torch.from_numpy(rs.randn(B, A))).clamp(-0.995, 0.995).float().numpy()
    batch = {"obs": obs, "acts": acts, "advs": (rs.randn(B, 1) * 2 + 0.5).astype(np.float32)}
    agent = Reinforce(pf=pf, plr=plr, entropy_coeff=c_ent, shuffle=True, discount=0.99, num_epochs=10, batch_size=B,
                      env=SynthVecEnv(4, device=DEV), replay_buffer=None, collector=_Stub(), logger=ListLogger(), device=DEV,
                      save_dir=None)
    eng = agent.engine()
    assert type(eng).__name__ == "_GenericReinforce" and ops.has_post(eng.pf_layers)
    p0 = eng.flat.detach().cpu().numpy().copy()
    info = agent.update(batch)
    # float64: the restatement's objective on the torch module
    import _gauss_ref as gr
    t = lambda x: torch.from_numpy(np.asarray(x)).double()
    advs = t(batch["advs"]).reshape(-1)
    advn = (advs - advs.mean()) / (advs.std() + 1e-5)
    lp = gr.logp(networks.Net.forward(cpu, t(obs)), cpu.logstd, t(acts), True)
    ent = (0.5 + gr.HALF_LOG_2PI + cpu.logstd.clamp(-20.0, 2.0)).sum()
    loss = (-lp * advn).mean() - c_ent * ent
    loss.backward()
    names = dict((id(p), n) for n, p in pf.named_parameters())
    want = dict(cpu.named_parameters())
    order = ops.plan_params(eng.pf_layers) + [pf.logstd]
    got_g = eng.grads.detach().cpu().numpy().astype(np.float64)
    off = 0
    for p in order:
        w = want[names[id(p)]].grad.numpy().reshape(-1)
        e = np.abs(got_g[off:off + w.size] - w)
        print("%s grad max abs err %.3e (max |grad| %.3e)" % (names[id(p)], e.max(), np.abs(w).max()))
        assert (e <= 1e-4 * np.abs(w) + 1e-5 * np.abs(w).max()).all(), names[id(p)]
        off += w.size
    assert off == eng.P_pf == got_g.size
    opt = pref.AdamRef(p0, np.zeros_like(p0), np.zeros_like(p0), (eng.P_pf,), eps=1e-8)
    opt.step(got_g, (np.float32(plr),), 0.5, 1.0, 1)
    err = float(np.abs(eng.flat.detach().cpu().numpy().astype(np.float64) - opt.p).max())
    print("parameters after the step on the engine's own gradient: max abs err %.3e" % err)
    assert err <= 1e-6
    a_np = batch["advs"].astype(np.float64)
    lp = lp.detach()
    want_info = {'advs/mean': a_np.mean(), 'advs/std': a_np.std(), 'advs/max': a_np.max(), 'advs/min': a_np.min(),
                 'Training/policy_loss': loss.item(), 'ent': ent.item(), 'logprob/mean': lp.mean().item(),
                 'logprob/std': lp.std().item(), 'logprob/max': lp.max().item(), 'logprob/min': lp.min().item()}
    assert list(info) == R.INFO_KEYS and R.info_close(info, want_info) <= 1.0, (info, want_info)


# ---------------------------------------------------------------- collect + update
def make_loop(N, T, B, head="gauss", single=False, hidden=(64, 64), seed=5):
    from torchrl_amd import networks
    from torchrl_amd.algo import Reinforce
    from torchrl_amd.collector.on_policy import OnPolicyCollectorBase, VecOnPolicyCollector
    from torchrl_amd.env import get_env, get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    cfg = {"reward_scale": 1, "obs_norm": False}
    if single:
        env, eval_env = get_env("SynthHalfCheetah-v0", cfg, device=DEV), get_env("SynthHalfCheetah-v0", cfg, device=DEV)
        buf = OnPolicyReplayBuffer(N * T, time_limit_filter=True)
    else:
        env, eval_env = (get_vec_env("SynthHalfCheetah-v0", cfg, N, device=DEV) for _ in range(2))
        buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    for e in (env, eval_env):
        e.horizon = 5                                                          # episodes end inside the rollout
    env.seed(seed)
    pf = policy_of(head, env.observation_space.shape[0], env.action_space.shape[0], hidden, seed=seed).to(DEV)
    cls = OnPolicyCollectorBase if single else VecOnPolicyCollector
    col = cls(networks.ZeroNet(), env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
              epoch_frames=N * T, max_episode_frames=3, eval_episodes=1, noise_mode="device")
    logger = ListLogger()
    agent = Reinforce(pf=pf, plr=3e-3, entropy_coeff=0.001, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, env=env,
                      replay_buffer=buf, collector=col, logger=logger, device=DEV, save_dir=None)
    return agent, pf, buf, col, logger


def iterate(agent, pf, buf, col, logger, N, T, B, fused_rollout):
    assert (col._spec is not None) == fused_rollout and col._no_critic
    for it in range(2):
        before = [p.detach().clone() for p in pf.parameters()]
        res = col.train_one_epoch()
        np.random.seed(20 + it)
        agent.update_per_epoch()
        torch.cuda.synchronize()
        assert bool((buf._values == 0.0).all())
        assert torch.equal(buf._advs, buf._estimate_returns) and bool(torch.isfinite(buf._advs).all())
        assert bool((buf._terminals != 0).any())                              # over-length cells: the bootstrap would have fired
        assert len(logger.infos) == (it + 1) * (T * N // B) and list(logger.infos[-1]) == R.INFO_KEYS
        assert all(np.isfinite(v) for i in logger.infos for v in i.values())
        assert np.isfinite(res["train_epoch_reward"])
        after = list(pf.parameters())
        assert all(bool(torch.isfinite(p).all()) for p in after) and any(not torch.equal(a, b) for a, b in zip(after, before))
    assert [n for n, _ in agent.snapshot_networks] == ["pf"] and agent.training_update_num == 2 * (T * N // B)
    # returns: the discounted sum of the stored rewards, restarted after a terminal (values are zero: nothing else enters)
    want = R.discounted_returns(buf._rewards.cpu().numpy(), buf._terminals.cpu().numpy(), 0.99)
    np.testing.assert_allclose(buf._estimate_returns.cpu().numpy(), want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("route", ["fused", "per_step"])
def test_iterations_with_the_vacant_critic(route, monkeypatch):
    N, T, B = 16, 8, 32
    if route == "per_step":
        monkeypatch.setenv("TRL_GENERIC_PPO", "1")                            # per-step launch sequence + the generic engine
    agent, pf, buf, col, logger = make_loop(N, T, B)
    iterate(agent, pf, buf, col, logger, N, T, B, route == "fused")
    assert type(agent.engine()).__name__ == ("_FusedReinforce" if route == "fused" else "_GenericReinforce")
    ev = col.eval_one_epoch()
    assert len(ev["eval_rewards"]) == N and all(np.isfinite(r) for r in ev["eval_rewards"])


def test_single_env_collector():
    N, T, B = 1, 16, 8
    agent, pf, buf, col, logger = make_loop(N, T, B, single=True)
    iterate(agent, pf, buf, col, logger, N, T, B, col._spec is not None)


def test_two_ranks_are_refused_by_name(monkeypatch):
    from torchrl_amd import _C, dist
    agent, pf, buf, col, logger = make_loop(16, 8, 32)
    monkeypatch.setattr(dist, "collectives_active", lambda: True)
    monkeypatch.setattr(dist, "world_size", lambda: 2)
    with pytest.raises(_C.TrlError, match="Reinforce runs on one rank"):
        agent.update({"obs": np.zeros((32, 17), np.float32), "acts": np.zeros((32, 6), np.float32),
                      "advs": np.ones((32, 1), np.float32)})


def test_example_script_runs_one_epoch(tmp_path, monkeypatch):
    params = json.load(open(os.path.join(REPO, "config", "reinforce_synth_halfcheetah.json")))
    assert params["reinforce"] == {"plr": 3e-3, "entropy_coeff": 0.001, "shuffle": True}
    params["replay_buffer"]["size"] = 16 * 8
    params["collector"]["epoch_frames"] = 16 * 8
    params["general_setting"].update(num_epochs=1, batch_size=32, eval_interval=1)
    cfg = tmp_path / "reinforce_small.json"
    cfg.write_text(json.dumps(params))
    sys.path.insert(0, os.path.join(REPO, "examples"))
    try:
        import reinforce_continuous_vec as ex
    finally:
        sys.path.pop(0)
    agent = ex.main(["--config", str(cfg), "--vec_env_nums", "16", "--seed", "1", "--log_dir", str(tmp_path / "log"), "--overwrite"])
    assert agent.training_update_num == 4 and type(agent).__name__ == "Reinforce"
    model_dir = tmp_path / "log" / "reinforce_small" / "SynthHalfCheetah-v0" / "1" / "model"
    assert os.path.exists(model_dir / "model_pf_finish.pth") and not os.path.exists(model_dir / "model_vf_finish.pth")
