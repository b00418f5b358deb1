"""State-dependent-std Gaussian policies on the HIP path: trl_gauss_sd_explore_f32 / trl_gauss_sd_logp_f32 /
trl_gauss_sd_losses_f32 against the torch restatement in float64 (tests/_gauss_sd_ref.py) and the reference fixture
(tests/golden/gauss_sd_update.npz), the generic PPO / A2C engine, and the per-step collector on SynthHalfCheetah-v0.
Every test here fails on a build without k_gauss_sd.hip."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_sd_ref as ref                                                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


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
    return np.load(os.path.join(HERE, "golden", "gauss_sd_update.npz"))


def dev(x):
    return None if x is None else torch.as_tensor(np.asarray(x)).to(DEV).contiguous()


def nets_of(D, A, tanh, hidden, seed=0, act=torch.nn.Tanh):
    from torchrl_amd import networks, policies
    torch.manual_seed(seed)
    net = dict(hidden_shapes=list(hidden), append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=act)
    pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=tanh, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    return pf, vf


def linear_params(mod):
    return [p for l in (list(mod.base.seq_fcs) + list(mod.seq_append_fcs)) if isinstance(l, torch.nn.Linear)
            for p in (l.weight, l.bias)]


# ---------------------------------------------------------------- kernels against the restatement in float64
def loss_case(B, A, tanh, seed, ls_lo=-1.5, ls_hi=0.5):
    """Seeded float32 inputs of one minibatch: log_std uniform in [ls_lo, ls_hi], actions drawn from the head itself (tanh
    actions clamped to +-0.995 as in the fixture), log pi_old = log pi + 0.3 N(0, 1) so that the clip fires on both sides.
    A ratio that float64 puts within 2e-3 of a clip boundary would make the float32 kernel's choice of surrogate -- a jump
    of the gradient -- depend on the last bits: those samples' log pi_old is moved by 0.05."""
    rs = np.random.RandomState(seed)
    t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
    head = torch.cat([t(B, A) * 0.5, torch.from_numpy(rs.uniform(ls_lo, ls_hi, (B, A)).astype(np.float32))], dim=1)
    acts = ref.explore(head, t(B, A), tanh)[0]
    if tanh:
        acts = acts.clamp(-0.995, 0.995)
    v, advs, rets, v_old = t(B), t(B) * 2 + 0.5, t(B), t(B)
    lp64 = ref.logp(head.double(), acts.double(), tanh)[0]
    old = lp64 + 0.3 * t(B).double()
    ratio = torch.exp(lp64 - old)
    near = ((ratio - 0.8).abs() < 2e-3) | ((ratio - 1.2).abs() < 2e-3)
    old = torch.where(near, old + 0.05, old).float()
    return dict(head=head, acts=acts.contiguous(), v=v, advs=advs, rets=rets, v_old=v_old, old=old)


def run_losses(c, tanh, loss_mode, clipv, clip=0.2, c_ent=0.01):
    from torchrl_amd import _C
    B = c["head"].shape[0]
    a64 = c["advs"].double()
    raw = torch.tensor([a64.sum(), (a64 ** 2).sum(), a64.max(), -a64.min()], dtype=torch.float64)
    info = torch.zeros(24, dtype=torch.float64, device=DEV)
    d_head, d_v = _C.gauss_sd_losses(dev(c["head"]), dev(c["acts"]), dev(c["advs"]), dev(c["old"]), dev(c["v"]), dev(c["rets"]),
                                     dev(c["v_old"]), dev(raw), float(B), clip, c_ent, clipv, tanh, loss_mode, info)
    torch.cuda.synchronize()
    want = ref.losses(c["head"].double(), c["v"].double(), c["acts"].double(), a64, c["rets"].double(), c["v_old"].double(),
                      c["old"].double(), clip, c_ent, clipv, loss_mode, tanh)
    return d_head.cpu().double(), d_v.view(-1).cpu().double(), info.cpu().numpy(), want


SUM_SLOTS = (0, 1, 2, 7, 12, 13, 20)


@pytest.mark.parametrize("B", [64, 300])
@pytest.mark.parametrize("A", [1, 6, 32])
@pytest.mark.parametrize("tanh,loss_mode,clipv", [(True, ref.LOSS_PPO_CLIP, False), (False, ref.LOSS_PPO_CLIP, True),
                                                   (True, ref.LOSS_A2C, False), (False, ref.LOSS_A2C, True)])
def test_losses_vs_restatement_in_float64(B, A, tanh, loss_mode, clipv):
    """d_head, d_v and all 24 info slots.  B = 64 is less than one block, B = 300 two blocks and a ragged tail (the fold).

    Bounds, from the float32 arithmetic on identical inputs:  d_v has the value loss's few roundings, the clipped
    value's sum v_old + clamp(v - v_old) among them (abs 2e-7 at |v| <= 4): rel 1e-5, abs 1e-6 / B.  d_head: its factor
    g_lp carries exp(log pi - log pi_old), and log pi is a sum of A terms of size up to ~10 with ~1e-7 relative error
    each -- up to 3e-5 for A = 32: rel 1e-4.  Its factor zc = [atanh](a) - mean has an
    ABSOLUTE error up to 5e-7 for tanh actions (|atanh| <= 3 at |a| <= 0.995 from a 1-ulp log2 of a quotient with 2e-7
    relative error), which reaches the gradient times |g_lp| / var <= (3.5 * 3 / B) * e^3 (|adv_n| <= 3.5, ratio <= 3,
    log_std >= -1.5) and, in the log_std half, times another 2 |zc| / std <= 8: abs 1e-4 / B -- about 1e-4 of the typical
    element (1 / (B std)).  Scalars: the project's rel 1e-4 / abs 1e-5 on a logged mean, so abs 1e-5 * B on the slots that
    hold sums."""
    c = loss_case(B, A, tanh, 1000 + 7 * A + B)
    d_head, d_v, info, want = run_losses(c, tanh, loss_mode, clipv)
    assert d_head.shape == (B, 2 * A) and torch.isfinite(d_head).all()
    for name, got, w, rel, ab in (("d_head", d_head, want["d_head"], 1e-4, 1e-4 / B), ("d_v", d_v, want["d_v"], 1e-5, 1e-6 / B)):
        err = (got - w).abs()
        print("%s max abs err %.3e (max |grad| %.3e, worst err / bound %.3f)"
              % (name, err.max().item(), w.abs().max().item(), (err / (ab + rel * w.abs())).max().item()))
        assert bool((err <= ab + rel * w.abs()).all()), name
    for k in range(24):
        ab = 1e-5 * B if k in SUM_SLOTS else 1e-5
        print("info[%d] %.9g want %.9g" % (k, info[k], want["info"][k]))
        assert info[k] == pytest.approx(want["info"][k], rel=1e-4, abs=ab), k
    assert all(info[k] == 0.0 for k in (21, 22, 23))


def test_clamped_log_std_columns_get_no_gradient():
    """Raw log_std columns at -25 and +3 (outside [-20, 2]), actions = mean + sigma eps: the gate closes those columns
    exactly, everything stays finite, and the statistics see the clamped values."""
    B, A = 300, 6
    c = loss_case(B, A, False, 31)
    c["head"][:, A + 1] = -25.0
    c["head"][:, A + 4] = 3.0
    c["acts"] = ref.explore(c["head"], torch.from_numpy(np.random.RandomState(5).randn(B, A).astype(np.float32)), False)[0]
    c["old"] = ref.logp(c["head"], c["acts"], False)[0] + 0.1
    d_head, d_v, info, _ = run_losses(c, False, ref.LOSS_PPO_CLIP, False)
    assert torch.isfinite(d_head).all() and torch.isfinite(d_v).all() and np.isfinite(info).all()
    assert bool((d_head[:, A + 1] == 0).all()) and bool((d_head[:, A + 4] == 0).all())
    assert bool((d_head[:, A] != 0).any()) and bool((d_head[:, A + 5] != 0).any())
    assert info[10] == 2.0 and info[11] == -20.0
    assert info[18] == pytest.approx(np.exp(2.0), rel=1e-6) and info[19] == pytest.approx(np.exp(-20.0), rel=1e-5)


@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("A", [1, 6, 32])
def test_explore_and_logp(A, tanh):
    """act / log pi against the restatement in float64, the deterministic form, and the bit-identity the ratio relies on.
    Bounds: act = [tanh](fma(exp(ls), eps, mean)) with a fast exp (2 ulp) and the kernels' tanh (abs 2e-7, trl_mlp.h):
    abs 2e-6 + rel 1e-6.  log pi of the stored action: the 5e-7 absolute error of zc (test_losses_vs_restatement_in_float64)
    moves a term by |zc| / var * 5e-7 <= 2e-6 / std <= 9e-6 at log_std >= -1.5: A * 1e-5, plus rel 1e-5 of |log pi|."""
    from torchrl_amd import _C
    N = 300
    c = loss_case(N, A, tanh, 50 + A)
    head = c["head"]
    eps = torch.from_numpy(np.random.RandomState(9).randn(N, A).astype(np.float32))
    act, lp = _C.gauss_sd_explore(dev(head), dev(eps), tanh)
    want_act, _ = ref.explore(head.double(), eps.double(), tanh)
    err = (act.cpu().double() - want_act).abs()
    assert bool((err <= 2e-6 + 1e-6 * want_act.abs()).all()), err.max().item()
    # log pi of the STORED (float32) action
    want_lp, want_ent = ref.logp(head.double(), act.cpu().double(), tanh)
    if tanh:                                                               # |a| -> 1: the atanh amplifies the last bit
        keep = act.cpu().abs().max(dim=1)[0] <= 0.995
    else:
        keep = torch.ones(N, dtype=torch.bool)
    assert keep.float().mean() > 0.5
    lerr = (lp.cpu().double() - want_lp).abs()[keep]
    assert bool((lerr <= A * 1e-5 + 1e-5 * want_lp.abs()[keep]).all()), lerr.max().item()
    # the same (head, act) through the log-prob kernel: the same bits, every row (saturated ones included)
    lp2, ent = _C.gauss_sd_logp(dev(head), act, tanh, want_ent=True)
    assert np.array_equal(lp2.cpu().numpy(), lp.cpu().numpy())
    np.testing.assert_allclose(ent.cpu().double().numpy(), want_ent.numpy(), rtol=1e-6, atol=1e-6)
    # eps = NULL: the deterministic action [tanh](mean)
    det, _ = _C.gauss_sd_explore(dev(head), None, tanh)
    mean = head[:, :A]
    if tanh:
        np.testing.assert_allclose(det.cpu().numpy(), torch.tanh(mean.double()).numpy(), rtol=0, atol=3e-7)
    else:
        assert np.array_equal(det.cpu().numpy(), mean.numpy())


# ---------------------------------------------------------------- the policy's protocol and the updates vs the fixture
def fixture_nets(g, tag):
    """The fixture's networks: the reference's draw for that seed (tests/test_gauss_sd_cpu.py), the policy's overwritten
    log_std rows loaded on top."""
    D, A, H, B, tanh = (int(x) for x in g[f"{tag}_args"])
    pf, vf = nets_of(D, A, bool(tanh), [H, H], seed=5 + D)
    pf.load_state_dict({k: torch.from_numpy(g[f"{tag}_pf0_" + k.replace(".", "__")].copy()) for k in pf.state_dict()})
    for k, v_ in vf.state_dict().items():
        assert np.array_equal(v_.numpy(), g[f"{tag}_vf0_" + k.replace(".", "__")]), k
    return pf, vf


def fixture_agent(g, tag, algo_cls, **kw):
    from torchrl_amd.env.synth import SynthVecEnv
    D, A, H, B, tanh = (int(x) for x in g[f"{tag}_args"])
    pf, vf = fixture_nets(g, tag)
    agent = algo_cls(pf=pf, vf=vf, tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, gae=True,
                     env=SynthVecEnv(4, obs_dim=D, act_dim=A, device=DEV), replay_buffer=None,
                     collector=_Stub(), logger=_Log(), device=DEV, save_dir=None, **kw)
    return pf, vf, agent


def param_error(mod, g, prefix):
    return max((a.detach().cpu() - b).abs().max().item() for a, b in zip(linear_params(mod), ref.params_from(g, prefix)))


def assert_info(info, g, prefix):
    want = ref.info_of(g, prefix)
    assert sorted(info) == sorted(want)
    bad = []
    for k in sorted(want):
        print("%s %s got %.9g want %.9g (err %.3e, bound %.3e)" % (prefix, k, info[k], want[k], abs(info[k] - want[k]),
                                                                     1e-5 + 1e-4 * abs(want[k])))
        if not info[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5):
            bad.append(k)
    assert not bad, bad


@pytest.mark.parametrize("tag", ref.TAGS)
def test_policy_outputs_vs_fixture(g, tag):
    """GuassianContPolicy.update / eval_act / explore on the GPU, kernels only, against the reference's outputs: the
    project's rel 1e-4 / abs 1e-5 on log_prob, ent and log_std in every case (the float32 CPU restatement is within 4.8e-7
    of the fixture in all four, profiles/NOTES_state_std.md, so no case has a bound of its own); mean and the greedy action
    abs 1e-5."""
    from torchrl_amd import _C
    D, A, H, B, tanh = (int(x) for x in g[f"{tag}_args"])
    pf, _ = fixture_nets(g, tag)
    pf.to(DEV)
    obs, acts = dev(g[f"{tag}_batch_obs"]), dev(g[f"{tag}_batch_acts"])
    before = _C.eager_fallback_count()
    with torch.no_grad():
        out = pf.update(obs, acts)
        ex = pf.explore(obs, return_log_probs=True)
        ev = pf.eval_act(obs)
    assert _C.eager_fallback_count() == before                            # kernels only
    assert out["log_prob"].shape == (B, 1) and out["ent"].shape == (B, 1)
    for k in ("mean", "log_std", "ent", "log_prob"):
        got, want = out[k].cpu().numpy(), g[f"{tag}_upd_{k}"]
        err = np.abs(got - want)
        print("%s %s: max abs err %.3e, worst err / bound %.3f" % (tag, k, err.max(), (err / (1e-5 + 1e-4 * np.abs(want))).max()))
    np.testing.assert_allclose(out["mean"].cpu().numpy(), g[f"{tag}_upd_mean"], rtol=0, atol=1e-5)
    for k in ("log_std", "ent", "log_prob"):
        np.testing.assert_allclose(out[k].cpu().numpy(), g[f"{tag}_upd_{k}"], rtol=1e-4, atol=1e-5, err_msg=k)
    np.testing.assert_allclose(ev, g[f"{tag}_eval_act"], rtol=0, atol=1e-5)
    assert ex["action"].shape == (B, A) and ex["log_prob"].shape == (B, 1) and torch.isfinite(ex["action"]).all()
    # the base class's keys: a tanh policy returns the pre-tanh sample with its log-prob (continuous_policy.py:109-116)
    assert ("pre_tanh" in ex) == bool(tanh)
    if tanh:
        assert ex["pre_tanh"].shape == (B, A)
        np.testing.assert_allclose(ex["action"].cpu().numpy(), torch.tanh(ex["pre_tanh"].double()).cpu().numpy(), rtol=0, atol=3e-7)
    with torch.no_grad():
        lp2, _ = _C.gauss_sd_logp(pf._head(obs), ex["action"].contiguous(), bool(tanh))
    assert torch.equal(lp2.view(B, 1), ex["log_prob"])


@pytest.mark.parametrize("tag", ref.TAGS)
def test_a2c_update_vs_fixture(g, tag, errlog):
    """Scalars rel 1e-4 / abs 1e-5, post-step parameters abs 1e-6.  The float32 CPU restatement is
    within 3e-8 of the fixture's parameters in every case (profiles/NOTES_state_std.md), so no case needs another bound."""
    from torchrl_amd.algo import A2C
    pf, vf, agent = fixture_agent(g, tag, A2C, plr=3e-4, vlr=1e-3, entropy_coeff=0.01)
    info = agent.update(ref.batch_of(g, tag))
    eng = agent.engine()
    assert type(eng).__name__ == "_GenericPPO" and eng.state_std and not eng.categorical and not hasattr(eng, "g_logstd")
    assert eng.P_pf == sum(p.numel() for p in linear_params(pf))
    errs = {name: param_error(mod, g, f"{tag}_a2c_{name}1_") for name, mod in (("pf", pf), ("vf", vf))}
    for name, err in errs.items():
        errlog("a2c_%s_%s" % (tag, name), err, 1e-6)
        print("a2c %s %s parameter error %.3e" % (tag, name, err))
    assert_info(info, g, f"{tag}_a2c_info")
    assert all(e <= 1e-6 for e in errs.values()), errs


@pytest.mark.parametrize("tag", ref.TAGS)
def test_ppo_chain_vs_fixture(g, tag, errlog):
    """Four chained PPO.update calls, the third with the clipped value loss; the same bounds for every update of the chain
    (tests/test_categorical_gpu.py allows its chain no growth either)."""
    from torchrl_amd.algo import PPO
    pf, vf, agent = fixture_agent(g, tag, PPO, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, entropy_coeff=0.005)
    agent.current_epoch = 3
    tgt = {k[len(f"{tag}_ppo_tpf0_"):].replace("__", "."): torch.from_numpy(g[k].copy())
           for k in g.files if k.startswith(f"{tag}_ppo_tpf0_")}
    agent.target_pf.load_state_dict(tgt)
    worst, bad = {}, []
    for s, clipv in enumerate(g[f"{tag}_ppo_clipv"]):
        agent.clipped_value_loss = bool(clipv)
        info = agent.update(ref.batch_of(g, tag))
        for name, mod in (("pf", pf), ("vf", vf)):
            err = param_error(mod, g, f"{tag}_ppo_{name}{s + 1}_")
            errlog("ppo_%s_update%d_%s" % (tag, s, name), err, 1e-6)
            print("ppo %s update %d %s parameter error %.3e" % (tag, s, name, err))
            worst[(s, name)] = err
        try:
            assert_info(info, g, f"{tag}_ppo_info{s}")
        except AssertionError as exc:
            bad.append((s, str(exc)))
    assert not bad, bad
    assert all(e <= 1e-6 for e in worst.values()), worst
    assert type(agent.engine()).__name__ == "_GenericPPO"


# ---------------------------------------------------------------- collector
def make_collector(N, T, horizon, max_frames, seed=3, hidden=(24, 40), noise_mode="device", obs_norm=False, tanh=True):
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    pf, vf = nets_of(17, 6, tanh, hidden)
    env, eval_env = (get_vec_env("SynthHalfCheetah-v0", {"reward_scale": 1, "obs_norm": obs_norm}, N, device=DEV)
                     for _ in range(2))
    for e in (env, eval_env):
        e.horizon = horizon
    env.seed(seed)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               epoch_frames=N * T, max_episode_frames=max_frames, eval_episodes=1, noise_mode=noise_mode)
    return pf, vf, env, buf, col


def check_ring(pf, buf, col, eps, T, N):
    """Stored acts == the restatement on the stored policy input and the given noise; old_logp == the log-prob kernel on
    the head of that input, bit for bit (the per-step forward, as the collector ran it)."""
    from torchrl_amd import _C, ops
    cpf = ref.MLP([p.detach().cpu() for p in linear_params(pf)])
    obs, acts, old = buf._obs, buf._acts, buf._old_logp
    assert acts.shape == (T, N, 6) and old.shape == (T, N, 1)
    layers, code = ops.linear_layers(pf), ops.act_code(pf)
    for t in range(T):
        with torch.no_grad():
            want, _ = ref.explore(cpf(obs[t].cpu()), eps[t].cpu(), bool(pf.tanh_action))
            head, _ = ops.mlp_forward(layers, obs[t].contiguous(), code, keep=False)
        np.testing.assert_allclose(acts[t].cpu().numpy(), want.numpy(), rtol=0, atol=1e-5, err_msg="acts at step %d" % t)
        lp, _ = _C.gauss_sd_logp(head, acts[t].contiguous(), bool(pf.tanh_action))
        assert torch.equal(lp, old[t].view(-1)), "old_logp at step %d" % t
    assert torch.isfinite(old).all() and len({float(x) for x in acts.view(-1)[:64]}) > 1


@pytest.mark.parametrize("noise_mode", ["host", "device"])
def test_collector_ring_vs_restatement(noise_mode):
    from torchrl_amd import _C
    N, T = 8, 16
    pf, vf, env, buf, col = make_collector(N, T, horizon=7, max_frames=999, noise_mode=noise_mode)
    assert col._spec is None and col._sd and not col._cat and col._dims == (17, 6)
    torch.manual_seed(11)
    res = col.train_one_epoch()
    if noise_mode == "host":                                              # the reference's stream: one (N, A) draw per step
        torch.manual_seed(11)
        eps = torch.stack([torch.randn(N, 6) for _ in range(T)])
    else:
        eps = _C.philox_normal(torch.empty(T, N, 6, device=DEV), col._noise_seed, 0)
    check_ring(pf, buf, col, eps, T, N)
    assert buf._terminals.sum() > 0 and np.isfinite(res["train_epoch_reward"])
    ev = col.eval_one_epoch()                                             # greedy evaluation through the eps == NULL form
    assert len(ev["eval_rewards"]) == N and ev["eval_traj_length"] == 7


def test_collector_with_a_running_observation_normaliser():
    from torchrl_amd import _C
    N, T = 8, 16
    pf, vf, env, buf, col = make_collector(N, T, horizon=7, max_frames=999, obs_norm=True)
    assert hasattr(env, "_obs_normalizer") and col._spec is None
    res = col.train_one_epoch()
    eps = _C.philox_normal(torch.empty(T, N, 6, device=DEV), col._noise_seed, 0)
    check_ring(pf, buf, col, eps, T, N)
    assert np.isfinite(res["train_epoch_reward"])
    assert len(col.eval_one_epoch()["eval_rewards"]) == N


def test_fill_old_logp_when_the_collector_did_not_write_it(monkeypatch):
    """PPO._fill_old_logp's branch for this head (the rollout wrote only part of the ring, or somebody cleared the flag):
    log pi_old of every stored pair under target_pf -- the log-prob kernel on the target's head, and the float32 CPU
    restatement within the project's rel 1e-4 / abs 1e-5.  Then an epoch that goes through it: the target is the policy
    there, so the first minibatch's ratio is 1 to rounding (the forward runs on T * N rows here and on B rows in the
    update: equal to 1e-5, not asserted bit for bit)."""
    from torchrl_amd import _C, ops
    monkeypatch.setenv("TRL_STRICT", "1")
    N, T = 8, 16
    np.random.seed(4)
    pf, vf, env, buf, col = make_collector(N, T, horizon=9, max_frames=999, seed=2)
    logger = _Log()
    agent = ppo_agent(pf, vf, env, buf, col, logger, 64)
    col.train_one_epoch()
    with torch.no_grad():                                                # a target that is NOT the collecting policy
        for p in agent.target_pf.parameters():
            p.add_(0.01 * torch.randn(p.shape, device=p.device))
    collected = buf._old_logp.clone()
    buf._old_logp.zero_()
    agent._fill_old_logp()
    tgt = agent.target_pf
    head, _ = ops.mlp_forward(ops.linear_layers(tgt), buf._obs.reshape(T * N, -1), ops.act_code(tgt), keep=False)
    want, _ = _C.gauss_sd_logp(head, buf._acts.reshape(T * N, -1), True)
    assert torch.equal(buf._old_logp.view(-1), want) and not torch.equal(buf._old_logp, collected)
    cpu_head = ref.MLP([p.detach().cpu() for p in linear_params(tgt)])(buf._obs.reshape(T * N, -1).cpu())
    cpu_lp = ref.logp(cpu_head.detach(), buf._acts.reshape(T * N, -1).cpu(), True)[0]
    np.testing.assert_allclose(buf._old_logp.view(-1).cpu().numpy(), cpu_lp.numpy(), rtol=1e-4, atol=1e-5)
    buf._old_logp.zero_()
    buf._old_logp_fresh = False                                          # the epoch's prologue has to fill it
    agent.current_epoch = 0
    agent.update_per_epoch()
    assert logger.infos[0]["ratio/max"] == pytest.approx(1.0, abs=1e-5) and logger.infos[0]["ratio/min"] == pytest.approx(1.0, abs=1e-5)
    assert all(np.isfinite(list(i.values())).all() for i in logger.infos)


# ---------------------------------------------------------------- end to end
def ppo_agent(pf, vf, env, buf, col, logger, B):
    from torchrl_amd.algo import PPO
    return PPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, tau=0.95, shuffle=True, entropy_coeff=0.005,
               discount=0.99, num_epochs=10, batch_size=B, gae=True, env=env, replay_buffer=buf, collector=col, logger=logger,
               device=DEV, save_dir=None)


def test_one_ppo_iteration_under_strict(monkeypatch):
    """N = 8, T = 16, B = 64, two passes, TRL_STRICT=1: no eager torch arithmetic on the way; the first minibatch meets the
    policy that collected it, so its ratio is exactly 1 -- log pi_old (collector) and log pi (loss kernel) are the same bits."""
    from torchrl_amd import _C
    monkeypatch.setenv("TRL_STRICT", "1")
    N, T = 8, 16
    np.random.seed(4)
    pf, vf, env, buf, col = make_collector(N, T, horizon=9, max_frames=999, seed=2)
    logger = _Log()
    agent = ppo_agent(pf, vf, env, buf, col, logger, 64)
    flat = lambda: torch.cat([p.detach().reshape(-1) for p in list(pf.parameters()) + list(vf.parameters())]).clone()
    before, count = flat(), _C.eager_fallback_count()
    col.train_one_epoch()
    agent.current_epoch = 0
    agent.update_per_epoch()
    torch.cuda.synchronize()
    assert _C.eager_fallback_count() == count
    assert len(logger.infos) == 2 * (N * T // 64)
    assert logger.infos[0]["ratio/max"] == 1.0 and logger.infos[0]["ratio/min"] == 1.0
    assert all(np.isfinite(list(i.values())).all() for i in logger.infos)
    assert all(k in logger.infos[0] for k in ("log_std/mean", "log_std/std", "log_std/max", "log_std/min"))
    after = flat()
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    assert type(agent.engine()).__name__ == "_GenericPPO" and agent.engine().state_std


def test_ppo_epochs_replayed_from_graphs_equal_eager(monkeypatch):
    """train_one_epoch + update_per_epoch, three visits: the third replays the captured rollout and update graphs and
    leaves the parameters of the run that never captured, bit for bit."""
    N, T = 8, 16
    finals = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("TRL_NO_GRAPH", no_graph)
        np.random.seed(4)
        pf, vf, env, buf, col = make_collector(N, T, horizon=9, max_frames=999, seed=2)
        logger = _Log()
        agent = ppo_agent(pf, vf, env, buf, col, logger, 64)
        per_epoch = []
        for epoch in range(3):
            res = col.train_one_epoch()
            agent.current_epoch = epoch
            agent.update_per_epoch()
            per_epoch.append((float(res["train_epoch_reward"]),
                              torch.cat([p.detach().reshape(-1) for p in list(pf.parameters()) + list(vf.parameters())]).clone()))
        assert all(np.isfinite(list(i.values())).all() for i in logger.infos)
        if no_graph == "0":
            assert col._roll_graph["graph"] is not None and len(agent.engine()._graphs) > 0
        finals.append(per_epoch)
    for (r0, p0), (r1, p1) in zip(*finals):
        assert r0 == r1 and torch.equal(p0, p1)
    assert not torch.equal(finals[0][0][1], finals[0][2][1])
