"""Categorical policies on the HIP path: trl_cat_act_f32 / trl_cat_logp_f32 / trl_cat_losses_f32 against the torch
restatement (tests/_categorical_ref.py) and the reference fixture (tests/golden/categorical_update.npz), the generic
PPO / A2C engine, the per-step collector on SynthCheetahDiscrete-v0 and the refusals.  Every test here fails on a build
without the categorical kernels."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _categorical_ref as ref                                                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TAGS = ["s4", "s17"]
BORDERLINE_CAP = 0.01


class _Stub:
    epoch_frames = 0


class _Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "categorical_update.npz"))


def dev(x):
    return torch.as_tensor(np.asarray(x)).to(DEV).contiguous()


def nets_of(D, A, H, seed, act=torch.nn.Tanh, hidden=None):
    from torchrl_amd import networks, policies
    torch.manual_seed(seed)
    net = dict(hidden_shapes=hidden or [H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=act)
    pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    return pf, vf


def fixture_agent(g, tag, algo_cls, **kw):
    """The fixture's networks (the reference's draw for that seed, tests/test_categorical_cpu.py) in a product agent."""
    from torchrl_amd.env.synth import SynthVecEnv
    D, A, H, B = (int(x) for x in g[f"{tag}_args"])
    pf, vf = nets_of(D, A, H, 5 + D)
    agent = algo_cls(pf=pf, vf=vf, tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, gae=True,
                     env=SynthVecEnv(4, obs_dim=D, act_dim=A, device=DEV, discrete=True), replay_buffer=None,
                     collector=_Stub(), logger=_Log(), device=DEV, save_dir=None, **kw)
    return pf, vf, agent


def batch_of(g, tag):
    return {k: g[f"{tag}_batch_{k}"] for k in ("obs", "acts", "advs", "values", "estimate_returns")}


def linear_params(mod):
    return [p for l in (list(mod.base.seq_fcs) + list(mod.seq_append_fcs)) if isinstance(l, torch.nn.Linear)
            for p in (l.weight, l.bias)]


def param_error(mod, g, prefix):
    return max((a.detach().cpu() - b).abs().max().item() for a, b in zip(linear_params(mod), ref.params_from(g, prefix)))


def assert_info(info, g, prefix, absent):
    keys = [str(k) for k in g[prefix + "_keys"]]
    want = dict(zip(keys, g[prefix + "_vals"]))
    kept = [k for k in keys if not k.startswith(absent)]
    assert sorted(info) == sorted(kept)
    assert not any(k.startswith(("log_std/", "std/")) for k in info)
    for k in kept:
        assert info[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5), k


# ---------------------------------------------------------------- trl_cat_act_f32
@pytest.mark.parametrize("A", [2, 6, 18])
def test_cat_act_vs_restatement(A):
    from torchrl_amd import _C
    logits, seed, counter = ref.act_case(A)
    N = logits.shape[0]
    u = ref.uniforms(seed, counter, 1, N)[0]
    want_a, want_lp, pre, S = ref.cat_act(logits, u)
    onehot = torch.empty(N, A, device=DEV)
    act, lp = _C.cat_act(dev(logits), seed=seed, counter=counter, onehot=onehot)
    assert act.shape == (N, 1) and lp.shape == (N,)
    got_a = act.view(-1).cpu().to(torch.int64)
    # the in-launch draw is the up-front draw, bit for bit
    u_dev = _C.philox_uniform(torch.empty(1, N, device=DEV), seed, counter)
    assert np.array_equal(u_dev.cpu().numpy()[0], u)
    act_u, lp_u = _C.cat_act(dev(logits), u=u_dev[0])
    assert torch.equal(act_u, act) and torch.equal(lp_u, lp)
    differ = got_a != want_a
    border = ref.borderline(u, pre, S)
    print("A=%d: %d rows differ, %d borderline of %d" % (A, int(differ.sum()), int(border.sum()), N))
    assert border.float().mean().item() <= BORDERLINE_CAP
    assert not bool((differ & ~border).any()), "an action differs on a row that is not borderline"
    same = ~differ
    err = (lp.cpu()[same] - want_lp[same]).abs()
    assert bool((err <= 2e-6 + 1e-5 * want_lp[same].abs()).all()), err.max().item()
    assert torch.equal(onehot.cpu(), torch.nn.functional.one_hot(got_a, A).float())
    # deterministic: exactly arg-max (lowest index on ties)
    tied = logits.clone()
    tied[::7, 1] = tied[::7].max(dim=-1)[0]                              # rows with the maximum twice
    tied[::7, A - 1] = tied[::7, 1]
    act_d, _ = _C.cat_act(dev(tied), deterministic=True)
    assert torch.equal(act_d.view(-1).cpu().to(torch.int64), ref.cat_act(tied, deterministic=True)[0])
    # two half-shards reproduce the single-process draw
    h = N // 2
    a0, l0 = _C.cat_act(dev(logits[:h]), seed=seed, counter=counter, env_offset=0)
    a1, l1 = _C.cat_act(dev(logits[h:]), seed=seed, counter=counter, env_offset=h)
    assert torch.equal(torch.cat([a0, a1]), act) and torch.equal(torch.cat([l0, l1]), lp)


# ---------------------------------------------------------------- the policy's protocol and the updates vs the fixture
@pytest.mark.parametrize("tag", TAGS)
def test_policy_outputs_vs_fixture(g, tag):
    from torchrl_amd import _C
    D, A, H, B = (int(x) for x in g[f"{tag}_args"])
    pf, _ = nets_of(D, A, H, 5 + D)
    pf.to(DEV)
    obs, acts = dev(g[f"{tag}_batch_obs"]), dev(g[f"{tag}_batch_acts"])
    before = _C.eager_fallback_count()
    with torch.no_grad():
        out = pf.update(obs, acts)
        probs = pf(obs)
        ex = pf.explore(obs, return_log_probs=True)
    assert out["log_prob"].shape == (B, 1) and out["ent"].shape == (B,)
    np.testing.assert_allclose(out["log_prob"].cpu().numpy(), g[f"{tag}_upd_log_prob"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(out["ent"].cpu().numpy(), g[f"{tag}_upd_ent"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(probs.cpu().numpy(), g[f"{tag}_probs"], rtol=1e-5, atol=1e-7)
    assert np.array_equal(pf.eval_act(obs), g[f"{tag}_eval_act"])
    assert ex["action"].shape == (B, 1) and ex["log_prob"].shape == (B,) and ex["dis"].shape == (B, A)
    a = ex["action"].view(-1).long()
    assert int(a.min()) >= 0 and int(a.max()) < A
    np.testing.assert_allclose(ex["log_prob"].cpu().numpy(), torch.log(probs.gather(1, a[:, None]))[:, 0].cpu().numpy(),
                               rtol=1e-5, atol=2e-6)
    assert _C.eager_fallback_count() == before                        # kernels only


@pytest.mark.parametrize("tag", TAGS)
def test_a2c_update_vs_fixture(g, tag, errlog):
    from torchrl_amd.algo import A2C
    pf, vf, agent = fixture_agent(g, tag, A2C, plr=3e-4, vlr=1e-3, entropy_coeff=0.01)
    info = agent.update(batch_of(g, tag))
    assert type(agent.engine()).__name__ == "_GenericPPO" and agent.engine().categorical
    assert_info(info, g, f"{tag}_a2c_info", ("std/",))
    for name, mod in (("pf", pf), ("vf", vf)):
        err = param_error(mod, g, f"{tag}_a2c_{name}1_")
        errlog("a2c_%s_%s" % (tag, name), err, 1e-6)
        assert err <= 1e-6, (name, err)


@pytest.mark.parametrize("tag", TAGS)
def test_ppo_chain_vs_fixture(g, tag, errlog):
    from torchrl_amd.algo import PPO
    pf, vf, agent = fixture_agent(g, tag, PPO, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, entropy_coeff=0.005)
    tgt = {k[len(f"{tag}_ppo_tpf0_"):].replace("__", "."): torch.from_numpy(g[k].copy())
           for k in g.files if k.startswith(f"{tag}_ppo_tpf0_")}
    agent.target_pf.load_state_dict(tgt)
    assert not hasattr(pf, "logstd")
    for s, clipv in enumerate(g[f"{tag}_ppo_clipv"]):
        agent.clipped_value_loss = bool(clipv)
        info = agent.update(batch_of(g, tag))
        assert_info(info, g, f"{tag}_ppo_info{s}", ("log_std/",))
        for name, mod in (("pf", pf), ("vf", vf)):
            err = param_error(mod, g, f"{tag}_ppo_{name}{s + 1}_")
            errlog("ppo_%s_update%d_%s" % (tag, s, name), err, 1e-6)
            assert err <= 1e-6, (s, name, err)
    eng = agent.engine()
    assert type(eng).__name__ == "_GenericPPO" and eng.P_pf == sum(p.numel() for p in linear_params(pf))


# ---------------------------------------------------------------- trl_cat_losses_f32 gradients
@pytest.mark.parametrize("loss_mode,clipv", [(ref.LOSS_PPO_CLIP, False), (ref.LOSS_PPO_CLIP, True), (ref.LOSS_A2C, False)])
def test_cat_losses_gradients_vs_autograd(loss_mode, clipv):
    """d_logits / d_v at a shape outside the fixture (A = 18, B = 1000: the last block is partial) against torch autograd
    on the restatement's objective in fp64 on the CPU.  tests/test_generic_shapes_gpu.py has no separate gradient bound
    for the Gaussian loss kernel, so the bound is rel 1e-4 / abs 1e-6, the absolute part scaled by 1 / B (every
    gradient carries the 1 / B of the batch mean)."""
    from torchrl_amd import _C
    B, A = 1000, 18
    rs = np.random.RandomState(77)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    logits, v, advs, rets, v_old = t(B, A) * 1.5, t(B), t(B) * 2 + 0.5, t(B), t(B)
    acts = torch.from_numpy(rs.randint(0, A, size=(B,)).astype(np.float32))
    old_lp = ref.cat_logp(logits, acts)[0] + 0.15 * t(B)                  # ratios on both sides of the clip
    clip, c_ent = 0.2, 0.01
    l64, v64 = logits.double().requires_grad_(True), v.double().requires_grad_(True)
    ref.objective(l64, v64, acts, advs.double(), rets.double(), v_old.double(), old_lp.double(), clip, c_ent, clipv,
                  loss_mode).backward()
    raw = torch.tensor([advs.double().sum(), (advs.double() ** 2).sum(), advs.max(), -advs.min()], dtype=torch.float64)
    info = torch.zeros(24, dtype=torch.float64, device=DEV)
    d_logits, d_v = _C.cat_losses(dev(logits), dev(acts), dev(advs), dev(old_lp), dev(v), dev(rets), dev(v_old), dev(raw),
                                  float(B), clip, c_ent, clipv, loss_mode, info)
    for name, got, want in (("d_logits", d_logits.cpu().double(), l64.grad), ("d_v", d_v.view(-1).cpu().double(), v64.grad)):
        err = (got - want).abs()
        bound = 1e-6 / B + 1e-4 * want.abs()
        print(name, "max abs err %.3e, max |grad| %.3e" % (err.max().item(), want.abs().max().item()))
        assert bool((err <= bound).all()), (name, (err - bound).max().item())
    r = ref.losses(logits, v, acts, advs, rets, v_old, old_lp, clip, c_ent, clipv, loss_mode)
    i = info.cpu()
    assert i[20].item() == pytest.approx(r["ent"].double().sum().item(), rel=1e-5)
    assert i[1].item() == pytest.approx(r["lp"].double().sum().item(), rel=1e-5)
    assert i[0].item() == pytest.approx(r["surr"].double().sum().item(), rel=1e-4, abs=1e-3)
    assert all(i[k].item() == 0.0 for k in (8, 9, 10, 11, 16, 17, 18, 19))


@pytest.mark.parametrize("loss_mode,clipv", [(ref.LOSS_PPO_CLIP, False), (ref.LOSS_PPO_CLIP, True), (ref.LOSS_A2C, False)])
@pytest.mark.parametrize("B,A", [(B, A) for A in (2, 64) for B in (2, 256, 257)])
def test_cat_losses_gradients_at_the_edges_of_the_sizes(B, A, loss_mode, clipv):
    """The smallest and the largest head (A = 2, 64) at B = 2 (the smallest batch an unbiased advantage std exists for), one
    full block and one sample more, against float64 autograd with the bound form of the test above."""
    from torchrl_amd import _C
    rs = np.random.RandomState(7700 + 3 * B + A)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    logits, v, advs, rets, v_old = t(B, A) * 1.5, t(B), t(B) * 2 + 0.5, t(B), t(B)
    acts = torch.from_numpy(rs.randint(0, A, size=(B,)).astype(np.float32))
    old_lp = ref.cat_logp(logits, acts)[0] + 0.15 * t(B)
    clip, c_ent = 0.2, 0.01
    l64, v64 = logits.double().requires_grad_(True), v.double().requires_grad_(True)
    ref.objective(l64, v64, acts, advs.double(), rets.double(), v_old.double(), old_lp.double(), clip, c_ent, clipv,
                  loss_mode).backward()
    raw = torch.tensor([advs.double().sum(), (advs.double() ** 2).sum(), advs.max(), -advs.min()], dtype=torch.float64)
    info = torch.zeros(24, dtype=torch.float64, device=DEV)
    d_logits, d_v = _C.cat_losses(dev(logits), dev(acts), dev(advs), dev(old_lp), dev(v), dev(rets), dev(v_old), dev(raw),
                                  float(B), clip, c_ent, clipv, loss_mode, info)
    assert d_logits.shape == (B, A) and d_v.shape == (B, 1)
    for name, got, want in (("d_logits", d_logits.cpu().double(), l64.grad), ("d_v", d_v.view(-1).cpu().double(), v64.grad)):
        err = (got - want).abs()
        bound = 1e-6 / B + 1e-4 * want.abs()
        print(name, "B %d A %d: max err / bound %.3e, max |grad| %.3e" % (B, A, (err / bound).max().item(), want.abs().max().item()))
        assert bool((err <= bound).all()), (name, (err - bound).max().item())


# ---------------------------------------------------------------- trl_cat_logp_f32: log pi, entropy, probabilities
@pytest.mark.parametrize("scale", [1.0, 40.0], ids=["ordinary", "peaked"])
@pytest.mark.parametrize("B,A", [(B, A) for A in (2, 7, 64) for B in (1, 255, 256, 257)])
def test_cat_logp_probs_and_entropy_in_float64(B, A, scale, errlog):
    """log pi, probabilities and entropy of stored (logits, index) pairs against `_categorical_ref.cat_logp` in float64, per
    element, at one sample, a block of 256 and its neighbours, the smallest head, an odd one and the largest; logits 1.5 N(0, 1)
    and 40 times that (most terms of the sum underflow).  U = 2^-24; x_k = m - l_k; the inputs are exact, so the bounds are the
    float32 roundings of tests/_rollout_ref.py::cat_terms alone:
      log pi_k  U (x_k + 4 |log S| + |log pi_k| + 2A + 2): the subtraction, S's (2A + 2) U, logf, the last subtraction
      p_k       p_k U (x_k + 2A + 5) + 1.2e-38: the exponent's rounding U x_k and expf's 2 U on e_k, S's (2A + 2) U, the division;
                a term below the smallest normal number may be flushed
      entropy   sum_k (b_p |log pi_k| + p_k b_logpi + U |p_k log pi_k|) + A U sum_k |p_k log pi_k|: each product, the A additions
    Guard words behind every output; `_C.cat_probs` returns the same bits."""
    from torchrl_amd import _C
    rs = np.random.RandomState(8800 + 5 * B + A)
    logits = torch.from_numpy((rs.randn(B, A) * 1.5 * scale).astype(np.float32))
    acts = torch.from_numpy(rs.randint(0, A, size=(B,)).astype(np.float32))
    acts[0], acts[-1] = A - 1, 0
    want_lp, want_H, want_p = ref.cat_logp(logits.double(), acts)
    lp_all, _, _ = ref.log_probs(logits.double())
    U, G, SENT = 2.0 ** -24, 64, -777.25
    x = logits.double().max(dim=-1, keepdim=True)[0] - logits.double()
    logS = torch.log(torch.exp(-x).sum(-1, keepdim=True))
    b_lp_all = U * (x + 4.0 * logS.abs() + lp_all.abs() + 2.0 * A + 2.0)
    b_p = want_p * U * (x + 2.0 * A + 5.0) + 1.2e-38
    plp = (want_p * lp_all).abs()
    b_H = (b_p * lp_all.abs() + want_p * b_lp_all + U * plp).sum(-1) + A * U * plp.sum(-1)
    bufs = {k: torch.full((n + G,), SENT, device=DEV) for k, n in (("lp", B), ("ent", B), ("probs", B * A))}
    dl, da = dev(logits), dev(acts)
    _C.cat_logp(dl, da, out=bufs["lp"][:B], ent=bufs["ent"][:B])
    _C.check(_C.lib().trl_cat_logp_f32(_C.dev_ptr(dl, name="logits"), None, None, None, _C.dev_ptr(bufs["probs"], name="probs"), B, A,
                                       _C.stream_ptr(DEV)), "trl_cat_logp_f32")
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in bufs.items()}
    for k, n in (("lp", B), ("ent", B), ("probs", B * A)):
        assert bool((got[k][n:] == SENT).all()), "guard behind %s overwritten" % k
        assert bool(torch.isfinite(got[k][:n]).all()), k
    assert torch.equal(_C.cat_probs(dl).cpu().view(-1), got["probs"][:B * A])
    idx = acts.long()[:, None]
    worst = {"logp": ((got["lp"][:B].double() - want_lp).abs() / b_lp_all.gather(1, idx)[:, 0]).max().item(),
             "probs": ((got["probs"][:B * A].view(B, A).double() - want_p).abs() / b_p).max().item(),
             "ent": ((got["ent"][:B].double() - want_H).abs() / b_H).max().item()}
    print("B %d A %d x%g: worst err / bound %s" % (B, A, scale, {k: round(v, 4) for k, v in worst.items()}))
    for k, v in worst.items():
        errlog("cat_logp_%s" % k, v, 1.0)
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------- collector
def make_collector(N, T, horizon, max_frames, seed=3, hidden=(24, 40), noise_mode="device", D=17, A=6):
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    pf, vf = nets_of(D, A, None, 0, hidden=list(hidden))
    with torch.no_grad():
        pf.seq_append_fcs[-1].weight.mul_(30.0)                          # leave the near-uniform initial policy
    env, eval_env = (get_vec_env("SynthCheetahDiscrete-v0", {"reward_scale": 1, "obs_norm": False}, N, device=DEV)
                     for _ in range(2))
    for e in (env, eval_env):
        e.horizon = horizon
    env.seed(seed)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               epoch_frames=N * T, max_episode_frames=max_frames, eval_episodes=1, noise_mode=noise_mode)
    return pf, vf, env, buf, col


def test_collector_ring_vs_cpu_stepping():
    """One rollout on SynthCheetahDiscrete-v0 (N = 64, T = 16, episodes end inside it) against oracle.synth_env + the
    restatement stepped on the CPU.  Tolerances of test_rollout_vs_reference_golden (1e-5; log pi rtol 1e-4 / atol 2e-3).
    An env whose action differs -- only allowed on a borderline row -- leaves the comparison from that step on and counts
    against the cap (1 % of the T * N rows)."""
    from oracle.synth_env import SynthVecEnvCPU
    import gym
    N, T, horizon = 64, 16, 7
    pf, vf, env, buf, col = make_collector(N, T, horizon, max_frames=999)
    assert isinstance(env.action_space, gym.spaces.Discrete) and env.action_space.n == 6
    assert col._spec is None and col._cat
    cpf, cvf = ref.MLP([p.detach().cpu() for p in linear_params(pf)]), ref.MLP([p.detach().cpu() for p in linear_params(vf)])
    res = col.train_one_epoch()
    got = {k: getattr(buf, "_" + k).cpu() for k in ("obs", "next_obs", "acts", "values", "rewards", "terminals", "old_logp")}
    assert got["acts"].shape == (T, N, 1)
    cenv = SynthVecEnvCPU(N, horizon=horizon)
    cenv.seed(3)
    ob = torch.from_numpy(cenv.reset().astype(np.float32))
    alive = torch.ones(N, dtype=torch.bool)
    dropped = 0
    tol = {"obs": (0, 1e-5), "next_obs": (0, 1e-5), "values": (0, 1e-5), "rewards": (0, 1e-5), "terminals": (0, 0),
           "old_logp": (1e-4, 2e-3)}
    with torch.no_grad():
        for t in range(T):
            logits, v = cpf(ob), cvf(ob)
            u = ref.uniforms(col._noise_seed, t, 1, N)[0]
            a, lp, pre, S = ref.cat_act(logits, u)
            ga = got["acts"][t, :, 0].to(torch.int64)
            differ = (ga != a) & alive
            assert not bool((differ & ~ref.borderline(u, pre, S)).any()), "step %d: a non-borderline action differs" % t
            dropped += int(differ.sum())
            alive &= ~differ
            nxt, rew, done, _ = cenv.step(torch.nn.functional.one_hot(a, 6).float().numpy())
            want = {"obs": ob, "next_obs": torch.from_numpy(nxt), "values": v, "rewards": torch.from_numpy(rew),
                    "terminals": torch.from_numpy(done.astype(np.float32)), "old_logp": lp[:, None]}
            for k, (rtol, atol) in tol.items():
                np.testing.assert_allclose(got[k][t][alive].numpy(), want[k].reshape(N, -1)[alive].numpy(), rtol=rtol,
                                           atol=atol, err_msg="%s at step %d" % (k, t))
            ob = torch.from_numpy(cenv.partial_reset(done[:, 0]).astype(np.float32))
    print("envs dropped after a borderline draw: %d" % dropped)
    assert dropped <= BORDERLINE_CAP * T * N
    assert got["terminals"].sum() > 0 and np.isfinite(res["train_epoch_reward"])
    ev = col.eval_one_epoch()                                             # greedy evaluation through cat_act's arg-max
    assert len(ev["eval_rewards"]) == N and ev["eval_traj_length"] == horizon


def test_captured_rollout_draws_what_the_eager_one_draws(monkeypatch):
    N, T = 16, 12
    results = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("TRL_NO_GRAPH", no_graph)
        pf, vf, env, buf, col = make_collector(N, T, horizon=7, max_frames=5, seed=1)
        snaps = []
        for _ in range(4):
            res = col.train_one_epoch()
            snaps.append({k: getattr(buf, "_" + k).clone() for k in ("obs", "next_obs", "acts", "values", "rewards",
                                                                     "terminals", "old_logp")}
                         | {"reward": res["train_epoch_reward"], "n_eps": len(res["train_rewards"])})
        assert (col._roll_graph["graph"] is not None) == (no_graph == "0")
        results.append(snaps)
    for a, b in zip(*results):
        assert a["reward"] == b["reward"] and a["n_eps"] == b["n_eps"]
        for k in a:
            if isinstance(a[k], torch.Tensor):
                assert torch.equal(a[k], b[k]), k
    assert len({float(x) for x in results[0][0]["acts"].view(-1)}) > 1


def test_ppo_epochs_replayed_from_graphs_equal_eager(monkeypatch):
    """train_one_epoch + update_per_epoch, three visits: the third replays the captured rollout and update graphs and
    leaves the parameters of the run that never captured, bit for bit."""
    from torchrl_amd.algo import PPO
    N, T = 32, 16
    finals = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("TRL_NO_GRAPH", no_graph)
        np.random.seed(4)
        pf, vf, env, buf, col = make_collector(N, T, horizon=9, max_frames=999, seed=2)
        logger = _Log()
        agent = PPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, tau=0.95, shuffle=True,
                    entropy_coeff=0.005, discount=0.99, num_epochs=10, batch_size=N * 4, gae=True, env=env, replay_buffer=buf,
                    collector=col, logger=logger, device=DEV, save_dir=None)
        per_epoch = []
        for epoch in range(3):
            res = col.train_one_epoch()
            agent.current_epoch = epoch
            agent.update_per_epoch()
            per_epoch.append((float(res["train_epoch_reward"]),
                              torch.cat([p.detach().reshape(-1) for p in list(pf.parameters()) + list(vf.parameters())]).clone()))
        assert len(logger.infos) == 3 * 2 * (T // 4)
        assert all(np.isfinite(list(i.values())).all() for i in logger.infos)
        assert logger.infos[0]["ratio/max"] == 1.0 and logger.infos[0]["ratio/min"] == 1.0   # log pi_old from the same kernels
        assert not any(k.startswith("log_std/") for k in logger.infos[0])
        if no_graph == "0":
            assert col._roll_graph["graph"] is not None and len(agent.engine()._graphs) > 0
        finals.append(per_epoch)
    for (r0, p0), (r1, p1) in zip(*finals):
        assert r0 == r1 and torch.equal(p0, p1)
    assert not torch.equal(finals[0][0][1], finals[0][2][1])


def test_host_noise_is_refused():
    from torchrl_amd import _C
    with pytest.raises(_C.TrlError, match="noise_mode"):
        make_collector(8, 4, horizon=7, max_frames=5, noise_mode="host")


def test_ppo_on_host_cartpole_runs_the_shipped_config():
    """PyCartPole-v0 behind the host bridge with the shipped config (16 envs): integer actions reach the envs, the ring
    stores them as (N, 1), two epochs of collection + update + a greedy evaluation stay finite."""
    import json
    from torchrl_amd import networks, policies
    from torchrl_amd.algo import PPO
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    params = json.load(open(os.path.join(os.path.dirname(HERE), "config", "ppo_cartpole_host.json")))
    n = 16
    env, eval_env = (get_vec_env(params["env_name"], params["env"], n) for _ in range(2))
    env.seed(0)
    eval_env.seed(1)
    torch.manual_seed(0)
    np.random.seed(0)
    buf = OnPolicyReplayBuffer(env_nums=n, max_replay_buffer_size=params["replay_buffer"]["size"], time_limit_filter=True)
    net = dict(params["net"], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    pf = policies.CategoricalDisPolicy(input_shape=4, output_shape=env.action_space.n, **net)
    vf = networks.Net(input_shape=(4,), output_shape=1, **net)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               noise_mode="device", **params["collector"])
    logger = _Log()
    general = dict(params["general_setting"], env=col.env, replay_buffer=buf, logger=logger, device=DEV, collector=col,
                   save_dir=None)
    agent = PPO(pf=pf, vf=vf, **params["ppo"], **general)
    for epoch in range(2):
        res = col.train_one_epoch()
        assert np.isfinite(res["train_epoch_reward"]) and len(res["train_rewards"]) > 0
        agent.current_epoch = epoch
        agent.update_per_epoch()
    acts = buf._acts.cpu()
    assert acts.shape == (params["replay_buffer"]["size"] // n, n, 1)
    assert set(acts.view(-1).tolist()) == {0.0, 1.0}
    assert all(np.isfinite(list(i.values())).all() for i in logger.infos) and len(logger.infos) == 2 * 4 * 8
    ev = col.eval_one_epoch()
    assert len(ev["eval_rewards"]) == n and all(np.isfinite(ev["eval_rewards"]))


# The CPU restatement (tests/_categorical_ref.py::train_host_env_cpu) trained with the shipped config, 16 envs, seed 0:
# mean training-episode return 31.99 over the first five epochs, 170.75 over the last five (profiles/NOTES_categorical.md).
CPU_FIRST5, CPU_LAST5 = 31.99, 170.75


def test_ppo_learns_cartpole():
    """The shipped config on PyCartPole-v0 (16 envs, seed 0, all 40 epochs): the product's mean training-episode return
    over the last five epochs exceeds its own first-epoch return by at least HALF of the CPU restatement's improvement.
    Half, because the two action streams part at the first borderline draw: the runs are statistically comparable, not
    equal."""
    import json
    from torchrl_amd import networks, policies
    from torchrl_amd.algo import PPO
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    params = json.load(open(os.path.join(os.path.dirname(HERE), "config", "ppo_cartpole_host.json")))
    n, seed = 16, 0
    env, eval_env = (get_vec_env(params["env_name"], params["env"], n) for _ in range(2))
    env.seed(seed)
    eval_env.seed(seed + 1)
    torch.manual_seed(seed)
    np.random.seed(seed)
    buf = OnPolicyReplayBuffer(env_nums=n, max_replay_buffer_size=params["replay_buffer"]["size"], time_limit_filter=True)
    net = dict(params["net"], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    pf = policies.CategoricalDisPolicy(input_shape=4, output_shape=2, **net)
    vf = networks.Net(input_shape=(4,), output_shape=1, **net)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               noise_mode="device", **params["collector"])
    general = dict(params["general_setting"], env=col.env, replay_buffer=buf, logger=_Log(), device=DEV, collector=col,
                   save_dir=None)
    agent = PPO(pf=pf, vf=vf, **params["ppo"], **general)
    returns = []
    for epoch in range(params["general_setting"]["num_epochs"]):
        res = col.train_one_epoch()
        returns.append(float(np.mean(res["train_rewards"])) if len(res["train_rewards"]) else float("nan"))
        agent.current_epoch = epoch
        agent.update_per_epoch()
    first, last5 = returns[0], float(np.nanmean(returns[-5:]))
    print("per-epoch mean training-episode return:", [round(r, 1) for r in returns])
    print("first epoch %.2f, last five %.2f; CPU restatement: first five %.2f, last five %.2f" % (first, last5, CPU_FIRST5, CPU_LAST5))
    assert last5 - first >= 0.5 * (CPU_LAST5 - CPU_FIRST5)
