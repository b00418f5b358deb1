"""The fused two-launch PPO / A2C update for 64-wide `add_ln` nets (TRL_LN_FUSED_UPDATE=1; trl_ppo_ln_*, the LN passes of
ppo_wave_pass): every flat gradient element against float64 autograd, the fused engine against the generic one, the two
chain modes, the engine choice and whole iterations with both LayerNorm switches.

Worst err / bound per gradient case: profiles/NOTES_layernorm_update.md."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _layernorm_update_ref as R                                             # noqa: E402

pytestmark = pytest.mark.gpu
SWITCH = "TRL_LN_FUSED_UPDATE"
PPO_CLIP, A2C_LOSS = 0, 1


def case(head, D, A, act, ln, N, rows_mb, mode=PPO_CLIP, clipv=0, plant=None):
    return dict(head=head, D=D, A=A, act=act, ln=ln, N=N, rows_mb=rows_mb, mode=mode, clipv=clipv, plant=plant, tanh=head != "cat",
                c_ent=0.01)


# heads x Tanh / ReLU x LN on the policy (1) / the critic (2) / both (3) x D in {3, 17, 27} x A in {1, 6, 8}; B = 40 (N = 40: a
# ragged last tile, fewer tiles than waves), B = 96 as 3 rows of N = 32 (contiguous tiles) and 4 rows of N = 24 (per-lane cells)
GRAD_CASES = [case("gauss", 17, 6, "tanh", 3, 32, 3), case("gauss", 3, 1, "relu", 1, 40, 1, clipv=1),
              case("gauss", 27, 8, "tanh", 2, 24, 4, mode=A2C_LOSS), case("gauss", 27, 8, "relu", 1, 32, 3),
              case("cat", 3, 6, "relu", 3, 24, 4, clipv=1), case("cat", 17, 8, "tanh", 1, 32, 3, mode=A2C_LOSS),
              case("cat", 27, 6, "tanh", 2, 40, 1), case("sd", 3, 8, "tanh", 1, 32, 3, clipv=1),
              case("sd", 17, 1, "relu", 2, 40, 1, mode=A2C_LOSS), case("sd", 27, 6, "tanh", 3, 24, 4),
              case("gauss", 17, 6, "tanh", 3, 32, 3, plant="zero-variance"), case("gauss", 27, 6, "relu", 3, 24, 4, clipv=1, plant="large-mean")]
case_id = lambda c: "%s-D%d-A%d-%s-ln%d-N%dx%d-m%d-cv%d%s" % (c["head"], c["D"], c["A"], c["act"], c["ln"], c["N"], c["rows_mb"],
                                                            c["mode"], c["clipv"], "-" + c["plant"] if c["plant"] else "")


@pytest.mark.parametrize("c", GRAD_CASES, ids=case_id)
def test_gradients_vs_float64(c):
    """trl_ppo_ln_minibatch_grad_f32 + trl_ppo_ln_reduce_f32 on two workgroups.  Bound: 1e-4 of the largest
    float64 gradient entry of the network; the float32 run of the restatement stays below a quarter of it, or -- the planted
    first layers only -- the bound is scaled by max(1, rstd max|gamma|) of the case's worst row."""
    from torchrl_amd import _C
    dev, rs = torch.device("cuda:0"), np.random.RandomState(GRAD_CASES.index(c))
    D, A, N, rows_mb, T, head = c["D"], c["A"], c["N"], c["rows_mb"], 6, R.HEAD[c["head"]]
    O = 2 * A if c["head"] == "sd" else A
    pf, vf = R.draw_net(rs, D, O, c["ln"] & 1, c["plant"]), R.draw_net(rs, D, 1, c["ln"] & 2, c["plant"])
    ls = torch.from_numpy(-0.5 + 0.1 * rs.randn(A)) if c["head"] == "gauss" else None
    idx = torch.from_numpy(rs.permutation(T)[:rows_mb].astype(np.int64))       # shuffled time rows of a ring of T
    B = rows_mb * N
    ring = {"obs": rs.randn(T, N, D), "advs": rs.randn(T, N, 1), "rets": rs.randn(T, N, 1), "old_values": rs.randn(T, N, 1),
            "acts": rs.randint(0, A, (T, N, 1)).astype(np.float64) if c["head"] == "cat" else np.tanh(rs.randn(T, N, A))}
    ring = {k: torch.from_numpy(v) for k, v in ring.items()}
    mb = {k: v[idx].reshape(B, -1) for k, v in ring.items()}
    ring["old_logp"] = torch.zeros(T, N, 1, dtype=torch.float64)
    ring["old_logp"][idx] = (R.old_logp(c, pf, ls, mb) + torch.from_numpy(0.15 * rs.randn(B))).reshape(rows_mb, N, 1)
    mb["old_logp"] = ring["old_logp"][idx].reshape(B, -1)
    amp = []
    want, f32 = R.flat_grads(c, pf, ls, vf, mb, torch.float64, amp), R.flat_grads(c, pf, ls, vf, mb, torch.float32)
    # the launches: rows outside the minibatch are NaN, the partial rows start as NaN (every float of a row is written)
    outside = torch.ones(T, dtype=torch.bool)
    outside[idx] = False
    t = {}
    for k, v in ring.items():
        v = v.clone()
        v[outside] = float("nan")
        t[k] = v.float().to(dev).contiguous()
    flat = lambda plist: torch.cat([p.reshape(-1) for p in plist]).float().to(dev)
    f_pf, f_vf = flat(pf + ([ls] if ls is not None else [])), flat(vf)
    ps = _C.ppo_ln_partial_stride(D, 64, A, head, c["ln"])
    partial = torch.full((2, ps), float("nan"), device=dev)
    scal = torch.zeros(2, _C.ppo_sd_scalar_stride() if c["head"] == "sd" else 8, dtype=torch.float64, device=dev)
    adv = mb["advs"].float().double()
    raw = torch.tensor([adv.sum(), (adv * adv).sum(), adv.max(), -adv.min()], dtype=torch.float64, device=dev)
    idx_dev = idx.to(dev)
    g = _C.PpoBatchArgs()
    for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp"):
        setattr(g, k, t[k].data_ptr())
    g.row_idx, g.rows_mb, g.N, g.adv_raw, g.n_global = idx_dev.data_ptr(), rows_mb, N, raw.data_ptr(), float(B)
    g.pf_params, g.vf_params = f_pf.data_ptr(), f_vf.data_ptr()
    g.D, g.H, g.A, g.act = D, 64, A, {"tanh": 0, "relu": 1}[c["act"]]
    g.clip_para, g.entropy_coeff, g.clipped_value_loss, g.tanh_action, g.loss_mode = 0.2, c["c_ent"], c["clipv"], int(c["tanh"]), c["mode"]
    g.partial, g.scal_partial, g.n_wg, g.n_wg_pf = partial.data_ptr(), scal.data_ptr(), 2, 0
    grads = torch.full((f_pf.numel() + f_vf.numel(),), float("nan"), device=dev)
    info = torch.zeros(24, dtype=torch.float64, device=dev)
    _C.ppo_ln_minibatch_grad(g, head, c["ln"], dev)
    _C.ppo_ln_reduce(partial, scal, 2, D, 64, A, head, c["ln"], grads, info, pf_params=f_pf)
    got = grads.cpu().double().numpy()
    assert np.isfinite(partial.cpu().numpy()).all()
    worst = 0.0
    for name, sl in (("policy", slice(0, f_pf.numel())), ("value", slice(f_pf.numel(), None))):
        bound = 1e-4 * np.abs(want[sl]).max()
        e32 = np.abs(f32[sl] - want[sl]).max()
        if e32 > bound / 4:
            assert c["plant"], "the float32 restatement leaves a quarter of the bound on a case without a planted first layer"
            bound *= max(1.0, max(amp))
            assert e32 <= bound / 4
        err = np.abs(got[sl] - want[sl]).max()
        worst = max(worst, err / bound)
        print("%s %s err %.3e bound %.3e (float32 restatement %.3e)" % (case_id(c), name, err, bound, e32))
    assert worst <= 1.0


# ---------------------------------------------------------------- the engines
class _Stub:
    epoch_frames = 0


class _Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


def make_nets(head, D=17, A=6, act=torch.nn.Tanh, ln=3, width=64, seed=0):
    from torchrl_amd import networks, policies
    torch.manual_seed(seed)
    net = lambda on: dict(hidden_shapes=[width, width], append_hidden_shapes=[], base_type=networks.MLPBase, add_ln=bool(on),
                          activation_func=act)
    cls, O = {"gauss": (policies.GuassianContPolicyBasicBias, A), "cat": (policies.CategoricalDisPolicy, A),
              "sd": (policies.GuassianContPolicy, 2 * A)}[head]
    pf = cls(input_shape=D, output_shape=O, **({} if head == "cat" else {"tanh_action": True}), **net(ln & 1))
    vf = networks.Net(input_shape=(D,), output_shape=1, **net(ln & 2))
    with torch.no_grad():
        for m in list(pf.modules()) + list(vf.modules()):
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.3 * torch.randn(width))
                m.bias.copy_(0.2 * torch.randn(width))
    return pf, vf


def make_agent(cls, head, monkeypatch, fused, nets=None, D=17, A=6, B=48, env=None, **kw):
    from torchrl_amd import algo as algos
    from torchrl_amd.env.synth import SynthVecEnv
    dev = torch.device("cuda:0")
    for k in ("TRL_GENERIC_PPO", "TRL_PPO_CHAINS", SWITCH):
        monkeypatch.delenv(k, raising=False)
    if fused:
        monkeypatch.setenv(SWITCH, "1")
    pf, vf = nets or make_nets(head, D, A)
    pf.to(dev), vf.to(dev)
    extra = dict(clip_para=0.2, opt_epochs=2) if cls == "PPO" else {}
    general = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, gae=True, replay_buffer=None,
                   collector=_Stub(), logger=_Log(), device=dev, save_dir=None, plr=3e-4, vlr=1e-3, entropy_coeff=0.01)
    general.update(extra, **kw)
    agent = getattr(algos, cls)(pf=pf, vf=vf, env=env or SynthVecEnv(4, obs_dim=D, act_dim=A, device=dev, discrete=head == "cat"),
                                **general)
    return agent


def batch_of(head, D=17, A=6, B=48, seed=1):
    rs = np.random.RandomState(seed)
    acts = rs.randint(0, A, (B, 1)).astype(np.float32) if head == "cat" else np.tanh(rs.randn(B, A)).astype(np.float32)
    return {"obs": rs.randn(B, D).astype(np.float32), "acts": acts, "advs": rs.randn(B, 1).astype(np.float32),
            "estimate_returns": rs.randn(B, 1).astype(np.float32), "values": rs.randn(B, 1).astype(np.float32)}


def params_of(agent):
    return torch.cat([p.detach().reshape(-1) for net in (agent.pf, agent.vf) for p in net.parameters()]).cpu().numpy()


def assert_same(fa, ga, fi, gi):
    assert sorted(fi) == sorted(gi)
    for k in gi:
        assert np.isnan(fi[k]) == np.isnan(gi[k]) and (np.isnan(gi[k]) or fi[k] == pytest.approx(gi[k], rel=1e-4, abs=1e-5)), (k, fi[k], gi[k])
    err = np.abs(params_of(fa) - params_of(ga)).max()
    print("parameter difference fused / generic %.3e" % err)
    assert err <= 1e-6


@pytest.mark.parametrize("head", ["gauss", "cat", "sd"])
def test_fused_engine_vs_generic_engine(head, monkeypatch):
    """One A2C.update and four chained PPO.update (the third with the clipped value loss) on identical copies."""
    for cls, steps in (("A2C", [0]), ("PPO", [0, 0, 1, 0])):
        nets = make_nets(head, seed=3)
        fa = make_agent(cls, head, monkeypatch, True, nets=copy.deepcopy(nets))
        assert type(fa.engine()).__name__ == "_FusedPPO" and fa.engine().ln_mask == 3
        ga = make_agent(cls, head, monkeypatch, False, nets=copy.deepcopy(nets))
        assert type(ga.engine()).__name__ == "_GenericPPO"
        for clipv in steps:
            fa.clipped_value_loss = ga.clipped_value_loss = bool(clipv)
            assert_same(fa, ga, fa.update(batch_of(head)), ga.update(batch_of(head)))


def test_chain_modes_give_the_same_bits(monkeypatch):
    """An epoch of 4 minibatches through the two chains and through the joint sequence."""
    dev, out = torch.device("cuda:0"), []
    rs = np.random.RandomState(5)
    T, N, D, A = 8, 32, 17, 6
    t = {"obs": rs.randn(T, N, D), "acts": np.tanh(rs.randn(T, N, A)), "advs": rs.randn(T, N, 1), "rets": rs.randn(T, N, 1),
         "old_values": rs.randn(T, N, 1), "old_logp": -3.0 + 0.1 * rs.randn(T, N, 1)}
    t = {k: torch.from_numpy(v).float().to(dev) for k, v in t.items()}
    for chains in ("two", "joint"):
        agent = make_agent("PPO", "gauss", monkeypatch, True, nets=make_nets("gauss", ln=1, seed=4))
        monkeypatch.setenv("TRL_PPO_CHAINS", chains)
        eng = agent.engine()
        assert type(eng).__name__ == "_FusedPPO" and eng.two_chains == (chains == "two")
        eng.run(t, np.random.RandomState(6).permutation(T).reshape(4, 2).astype(np.int64), N)
        torch.cuda.synchronize()
        out.append(params_of(agent))
    assert np.array_equal(out[0], out[1])


def test_engine_choice(monkeypatch):
    name = lambda agent: type(agent.engine()).__name__
    assert name(make_agent("PPO", "gauss", monkeypatch, False)) == "_GenericPPO"
    assert name(make_agent("A2C", "gauss", monkeypatch, True, nets=make_nets("gauss", ln=2))) == "_FusedPPO"
    assert name(make_agent("PPO", "gauss", monkeypatch, True, nets=make_nets("gauss", width=128))) == "_GenericPPO"
    assert name(make_agent("PPO", "gauss", monkeypatch, True, optimizer_class=torch.optim.RMSprop)) == "_GenericPPO"
    agent = make_agent("PPO", "gauss", monkeypatch, True)
    monkeypatch.setenv("TRL_GENERIC_PPO", "1")
    assert name(agent) == "_GenericPPO"


def test_whole_iterations_with_both_switches(monkeypatch):
    """Two iterations (N = 32, T = 8) on a device synthetic env: one-launch rollout + fused update against per-step + generic
    (a categorical pair: both collection routes draw the same device noise)."""
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env.synth import SynthVecEnv
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    dev, N, T, D, A, runs = torch.device("cuda:0"), 32, 8, 17, 6, []
    nets = make_nets("cat", seed=7)
    for fused in (True, False):
        monkeypatch.delenv("TRL_LN_FUSED_ROLLOUT", raising=False)
        if fused:
            monkeypatch.setenv("TRL_LN_FUSED_ROLLOUT", "1")
        pf, vf = copy.deepcopy(nets)
        env, eval_env = (SynthVecEnv(N, obs_dim=D, act_dim=A, device=dev, discrete=True) for _ in range(2))
        env.horizon = eval_env.horizon = 9
        env.seed(11)
        buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
        col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=dev, train_render=False,
                                   epoch_frames=N * T, max_episode_frames=999, eval_episodes=1, noise_mode="device")
        agent = make_agent("PPO", "cat", monkeypatch, fused, nets=(pf, vf), B=128, env=env, replay_buffer=buf, collector=col)
        assert (col._ln == (True, True)) == fused and type(agent.engine()).__name__ == ("_FusedPPO" if fused else "_GenericPPO")
        np.random.seed(4)
        torch.manual_seed(12)
        for epoch in range(2):
            col.train_one_epoch()
            agent.current_epoch = epoch
            agent.update_per_epoch()
        torch.cuda.synchronize()
        runs.append(({k: getattr(buf, "_" + k).cpu().numpy().copy() for k in ("obs", "acts", "rewards", "values", "advs")},
                     params_of(agent)))
    for k, v in runs[1][0].items():
        np.testing.assert_allclose(runs[0][0][k], v, rtol=1e-4, atol=1e-5, err_msg=k)
    assert np.abs(runs[0][1] - runs[1][1]).max() <= 1e-6
