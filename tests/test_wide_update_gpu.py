"""The fused two-launch PPO / A2C update for plain 128-wide nets (TRL_WIDE_FUSED_UPDATE=1; trl_ppo_wide_*, k_ppo_wide.hip): every
flat gradient element against float64 autograd, single-network launches against the joint one, the fused engine against the
generic one, the engine choice and whole iterations with both wide switches.

Worst err / bound per gradient case: profiles/NOTES_wide_update.md."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _layernorm_update_ref as R                                             # noqa: E402
import test_layernorm_update_fused_gpu as L                                   # noqa: E402  (its agent / batch helpers)

pytestmark = pytest.mark.gpu
SWITCH, H = "TRL_WIDE_FUSED_UPDATE", 128
PPO_CLIP, A2C_LOSS = 0, 1


def case(head, D, A, act, N, rows_mb, mode=PPO_CLIP, clipv=0):
    return dict(head=head, D=D, A=A, act=act, ln=0, N=N, rows_mb=rows_mb, mode=mode, clipv=clipv, tanh=head != "cat", c_ent=0.01)


# 40 x 1: a ragged tile, fewer tiles than S; 32 x 3: contiguous cells, two tiles on a workgroup; 24 x 4: per-lane cells, tiles
# that straddle time rows; 40 x 5: four tiles per workgroup, ragged last tile, accumulation across tiles
GRAD_CASES = [case("gauss", 17, 6, "tanh", 32, 3), case("gauss", 3, 1, "relu", 40, 1, clipv=1),
              case("gauss", 27, 8, "tanh", 24, 4, mode=A2C_LOSS), case("gauss", 32, 8, "relu", 40, 5),
              case("cat", 3, 6, "relu", 24, 4, clipv=1), case("cat", 17, 8, "tanh", 40, 5, mode=A2C_LOSS),
              case("cat", 32, 2, "tanh", 40, 1), case("sd", 3, 8, "relu", 32, 3, clipv=1),
              case("sd", 17, 1, "relu", 40, 1, mode=A2C_LOSS), case("sd", 27, 6, "tanh", 40, 5)]
case_id = lambda c: "%s-D%d-A%d-%s-N%dx%d-m%d-cv%d" % (c["head"], c["D"], c["A"], c["act"], c["N"], c["rows_mb"], c["mode"], c["clipv"])


def draw(c, seed, T=6):
    """The case's float64 nets (W ~ N(0, 1 / fan-in)), a ring of T time rows of which shuffled `rows_mb` are the minibatch, and
    the minibatch itself; log pi_old = the float64 log pi + 0.15 z."""
    rs = np.random.RandomState(seed)
    D, A, N, rows_mb = c["D"], c["A"], c["N"], c["rows_mb"]
    O, B = (2 * A if c["head"] == "sd" else A), rows_mb * N
    net = lambda o: [torch.from_numpy(x) for x in (rs.randn(H, D) / np.sqrt(D), 0.1 * rs.randn(H), rs.randn(H, H) / np.sqrt(H),
                                                   0.1 * rs.randn(H), rs.randn(o, H) / np.sqrt(H), 0.1 * rs.randn(o))]
    pf, vf = net(O), net(1)
    ls = torch.from_numpy(-0.5 + 0.1 * rs.randn(A)) if c["head"] == "gauss" else None
    idx = torch.from_numpy(rs.permutation(T)[:rows_mb].astype(np.int64))
    ring = {"obs": rs.randn(T, N, D), "advs": rs.randn(T, N, 1), "rets": rs.randn(T, N, 1), "old_values": rs.randn(T, N, 1),
            "acts": rs.randint(0, A, (T, N, 1)).astype(np.float64) if c["head"] == "cat" else np.tanh(0.4 * rs.randn(T, N, A))}
    ring = {k: torch.from_numpy(v) for k, v in ring.items()}
    mb = {k: v[idx].reshape(B, -1) for k, v in ring.items()}
    ring["old_logp"] = torch.zeros(T, N, 1, dtype=torch.float64)
    ring["old_logp"][idx] = (R.old_logp(c, pf, ls, mb) + torch.from_numpy(0.15 * rs.randn(B))).reshape(rows_mb, N, 1)
    mb["old_logp"] = ring["old_logp"][idx].reshape(B, -1)
    return pf, vf, ls, idx, ring, mb


class Launch:
    """The device side of a drawn case: ring rows outside the minibatch are NaN, partial rows start as NaN."""

    def __init__(self, c, pf, vf, ls, idx, ring, mb):
        from torchrl_amd import _C
        self.c, self.dev = c, torch.device("cuda:0")
        outside = torch.ones(ring["obs"].shape[0], dtype=torch.bool)
        outside[idx] = False
        self.t = {}
        for k, v in ring.items():
            v = v.clone()
            v[outside] = float("nan")
            self.t[k] = v.float().to(self.dev).contiguous()
        flat = lambda plist: torch.cat([p.reshape(-1) for p in plist]).float()
        self.P_pf, self.P_vf = flat(pf).numel() + (0 if ls is None else ls.numel()), flat(vf).numel()
        self.flat0 = torch.cat([flat(pf + ([ls] if ls is not None else [])), flat(vf)]).to(self.dev)
        self.head = R.HEAD[c["head"]]
        self.ps = _C.ppo_wide_partial_stride(c["D"], H, c["A"], self.head)
        adv = mb["advs"].float().double()
        self.raw = torch.tensor([adv.sum(), (adv * adv).sum(), adv.max(), -adv.min()], dtype=torch.float64, device=self.dev)
        self.idx = idx.to(self.dev)

    def rows(self, n_wg):
        from torchrl_amd import _C
        return (torch.full((n_wg, self.ps), float("nan"), device=self.dev),
                torch.zeros(n_wg, _C.ppo_sd_scalar_stride() if self.c["head"] == "sd" else 8, dtype=torch.float64, device=self.dev))

    def grad(self, flat, n_wg, n_wg_pf, partial, scal):
        from torchrl_amd import _C
        c, g = self.c, _C.PpoBatchArgs()
        for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp"):
            setattr(g, k, self.t[k].data_ptr())
        g.row_idx, g.rows_mb, g.N, g.adv_raw, g.n_global = self.idx.data_ptr(), c["rows_mb"], c["N"], self.raw.data_ptr(), float(c["rows_mb"] * c["N"])
        g.pf_params, g.vf_params = flat.data_ptr(), flat.data_ptr() + 4 * self.P_pf
        g.D, g.H, g.A, g.act = c["D"], H, c["A"], {"tanh": 0, "relu": 1}[c["act"]]
        g.clip_para, g.entropy_coeff, g.clipped_value_loss, g.tanh_action, g.loss_mode = 0.2, c["c_ent"], c["clipv"], int(c["tanh"]), c["mode"]
        g.partial, g.scal_partial, g.n_wg, g.n_wg_pf = partial.data_ptr(), scal.data_ptr(), n_wg, n_wg_pf
        _C.ppo_wide_minibatch_grad(g, self.head, self.dev)


@pytest.mark.parametrize("c", GRAD_CASES, ids=case_id)
def test_gradients_vs_float64(c):
    """trl_ppo_wide_minibatch_grad_f32 + trl_ppo_wide_reduce_f32 on two workgroups.  Bound: per network 1e-4 of
    the largest float64 gradient entry; the float32 run of the restatement stays below a quarter of it."""
    from torchrl_amd import _C
    pf, vf, ls, idx, ring, mb = draw(c, GRAD_CASES.index(c))
    want, f32 = R.flat_grads(c, pf, ls, vf, mb, torch.float64), R.flat_grads(c, pf, ls, vf, mb, torch.float32)
    x = Launch(c, pf, vf, ls, idx, ring, mb)
    partial, scal = x.rows(2)
    grads = torch.full((x.P_pf + x.P_vf,), float("nan"), device=x.dev)
    info = torch.zeros(24, dtype=torch.float64, device=x.dev)
    x.grad(x.flat0, 2, 0, partial, scal)
    _C.ppo_wide_reduce(partial, scal, 2, c["D"], H, c["A"], x.head, grads, info, pf_params=x.flat0)
    got = grads.cpu().double().numpy()
    assert np.isfinite(partial.cpu().numpy()).all()
    worst = 0.0
    for name, sl in (("policy", slice(0, x.P_pf)), ("value", slice(x.P_pf, None))):
        bound = 1e-4 * np.abs(want[sl]).max()
        e32 = np.abs(f32[sl] - want[sl]).max()
        assert e32 <= bound / 4, "the float32 restatement leaves a quarter of the bound"
        err = np.abs(got[sl] - want[sl]).max()
        worst = max(worst, err / bound)
        print("%s %s err %.3e bound %.3e (float32 restatement %.3e)" % (case_id(c), name, err, bound, e32))
    assert worst <= 1.0


@pytest.mark.parametrize("c", [GRAD_CASES[3], GRAD_CASES[5], GRAD_CASES[9]], ids=case_id)
def test_single_network_launches_match_joint(c):
    """An all-policy launch (n_wg_pf = n_wg) and an all-value launch (n_wg_pf = -1), each folded by the `_net` fold / clip / Adam,
    give the bits of the joint launch + joint fold -- two steps, the second on stepped parameters and moments."""
    from torchrl_amd import _C
    lib = _C.lib()
    x = Launch(c, *draw(c, 20 + GRAD_CASES.index(c)))
    P, dev, rs = x.P_pf + x.P_vf, x.dev, np.random.RandomState(5)
    m0 = torch.from_numpy(rs.randn(P).astype(np.float32) * 1e-3).to(dev)
    v0 = torch.from_numpy((rs.rand(P).astype(np.float32) + 0.1) * 1e-5).to(dev)
    state = lambda: dict(flat=x.flat0.clone(), m=m0.clone(), v=v0.clone(), grads=torch.zeros(P, device=dev),
                         info=torch.zeros(2, 24, dtype=torch.float64, device=dev), norms=torch.zeros(2, 2, device=dev))
    ws = [torch.zeros(lib.trl_ppo_wide_reduce_adam_workspace(c["D"], H, c["A"], x.head), device=dev) for _ in range(3)]
    joint, split, stream = state(), state(), _C.stream_ptr(dev)

    def fold(fn, s, step, partial, scal, n_wg, which, w):
        a = _C.AdamArgs()
        a.params, a.grads, a.exp_avg, a.exp_avg_sq = s["flat"].data_ptr(), s["grads"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr()
        a.n_groups, a.group_sizes[0], a.group_sizes[1], a.group_lr[0], a.group_lr[1] = 2, x.P_pf, x.P_vf, 3e-4, 1e-3
        a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale = 0.5, 0.9, 0.999, 1e-5, 1.0
        a.step_count, a.norms_out, a.device_state = 3 + step, s["norms"][step].data_ptr(), 0
        _C.check(getattr(lib, fn)(partial.data_ptr(), scal.data_ptr(), n_wg, which, c["D"], H, c["A"], x.head, s["grads"].data_ptr(),
                                  s["info"][step].data_ptr(), C.byref(a), w.data_ptr(), stream), fn)

    for step in (0, 1):
        partial, scal = x.rows(4)
        x.grad(joint["flat"], 4, 2, partial, scal)
        fold("trl_ppo_wide_reduce_adam_f32", joint, step, partial, scal, 4, 2, ws[0])
        for net, n_wg_pf in ((0, 2), (1, -1)):
            partial, scal = x.rows(2)
            x.grad(split["flat"], 2, n_wg_pf, partial, scal)
            fold("trl_ppo_wide_reduce_adam_net_f32", split, step, partial, scal, 2, net, ws[1 + net])
    torch.cuda.synchronize()
    assert all(int(w[0].item()) == 0 for w in ws)                             # no norm rendezvous timed out
    for k in ("flat", "m", "v", "grads", "norms", "info"):
        assert torch.equal(joint[k], split[k]), k
    assert not torch.equal(joint["flat"], x.flat0) and torch.isfinite(joint["flat"]).all() and (joint["norms"] > 0).all()


# ---------------------------------------------------------------- the engines
def make_agent(cls, head, monkeypatch, fused, **kw):
    monkeypatch.delenv(SWITCH, raising=False)
    agent = L.make_agent(cls, head, monkeypatch, False, **kw)               # (clears the other engine switches)
    if fused:
        monkeypatch.setenv(SWITCH, "1")
    return agent


wide_nets = lambda head, seed=0, **kw: L.make_nets(head, ln=0, width=H, seed=seed, **kw)


@pytest.mark.parametrize("head", ["gauss", "cat", "sd"])
def test_fused_engine_vs_generic_engine(head, monkeypatch):
    """One A2C.update and four chained PPO.update (the third with the clipped value loss) on identical copies; then an epoch of
    4 minibatches through the two chains and through the joint sequence: equal bits."""
    for cls, steps in (("A2C", [0]), ("PPO", [0, 0, 1, 0])):
        nets = wide_nets(head, seed=3)
        fa = make_agent(cls, head, monkeypatch, True, nets=copy.deepcopy(nets))
        assert type(fa.engine()).__name__ == "_FusedPPO" and fa.engine().wide
        ga = make_agent(cls, head, monkeypatch, False, nets=copy.deepcopy(nets))
        assert type(ga.engine()).__name__ == "_GenericPPO"
        for clipv in steps:
            fa.clipped_value_loss = ga.clipped_value_loss = bool(clipv)
            L.assert_same(fa, ga, fa.update(L.batch_of(head)), ga.update(L.batch_of(head)))
    dev, out, rs = torch.device("cuda:0"), [], np.random.RandomState(5)
    T, N, D, A = 8, 32, 17, 6
    t = {"obs": rs.randn(T, N, D), "acts": rs.randint(0, A, (T, N, 1)) if head == "cat" else np.tanh(rs.randn(T, N, A)),
         "advs": rs.randn(T, N, 1), "rets": rs.randn(T, N, 1), "old_values": rs.randn(T, N, 1), "old_logp": -3.0 + 0.1 * rs.randn(T, N, 1)}
    t = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).float().to(dev) for k, v in t.items()}
    for chains in ("two", "joint"):
        agent = make_agent("PPO", head, monkeypatch, True, nets=wide_nets(head, seed=4))
        monkeypatch.setenv("TRL_PPO_CHAINS", chains)
        eng = agent.engine()
        assert eng.wide and eng.two_chains == (chains == "two")
        eng.run(t, np.random.RandomState(6).permutation(T).reshape(4, 2).astype(np.int64), N)
        torch.cuda.synchronize()
        out.append(L.params_of(agent))
    assert np.array_equal(out[0], out[1])


def test_engine_choice(monkeypatch):
    from torchrl_amd import algo as algos
    name = lambda agent: type(agent.engine()).__name__
    assert name(make_agent("PPO", "gauss", monkeypatch, False, nets=wide_nets("gauss"))) == "_GenericPPO"
    assert name(make_agent("A2C", "sd", monkeypatch, True, nets=wide_nets("sd"))) == "_FusedPPO"
    assert name(make_agent("PPO", "gauss", monkeypatch, True, nets=L.make_nets("gauss", ln=0, width=256))) == "_GenericPPO"
    assert name(make_agent("PPO", "gauss", monkeypatch, True, nets=wide_nets("gauss"), optimizer_class=torch.optim.RMSprop)) == "_GenericPPO"
    assert name(make_agent("PPO", "gauss", monkeypatch, True, nets=L.make_nets("gauss", ln=3, width=H))) == "_GenericPPO"
    agent = make_agent("PPO", "gauss", monkeypatch, True, nets=wide_nets("gauss"))
    monkeypatch.setenv("TRL_GENERIC_PPO", "1")
    assert name(agent) == "_GenericPPO"
    monkeypatch.delenv("TRL_GENERIC_PPO")
    # REINFORCE: a vacant critic, every workgroup the policy's
    from torchrl_amd.env.synth import SynthVecEnv
    dev = torch.device("cuda:0")
    pf, _ = wide_nets("gauss", seed=2)
    before = torch.cat([p.detach().reshape(-1) for p in pf.parameters()]).clone()
    agent = algos.Reinforce(pf=pf.to(dev), env=SynthVecEnv(4, obs_dim=17, act_dim=6, device=dev), discount=0.99, num_epochs=10,
                            batch_size=48, replay_buffer=None, collector=L._Stub(), logger=L._Log(), device=dev, save_dir=None,
                            plr=3e-4, entropy_coeff=0.01, shuffle=True)
    assert type(agent.engine()).__name__ == "_FusedReinforce" and agent.engine().wide
    info = agent.update({k: v for k, v in L.batch_of("gauss").items() if k in ("obs", "acts", "advs")})
    after = torch.cat([p.detach().reshape(-1) for p in pf.parameters()]).cpu()
    assert np.isfinite(list(info.values())).all() and torch.isfinite(after).all() and not torch.equal(after, before.cpu())


def test_whole_iterations_with_both_switches(monkeypatch):
    """Two iterations (N = 32, T = 8) on a device synthetic env: one-launch rollout + fused update against per-step + generic
    (a categorical pair: both collection routes draw the same device noise)."""
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env.synth import SynthVecEnv
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    dev, N, T, D, A, runs = torch.device("cuda:0"), 32, 8, 17, 6, []
    nets = wide_nets("cat", seed=7)
    for fused in (True, False):
        monkeypatch.delenv("TRL_WIDE_FUSED_ROLLOUT", raising=False)
        if fused:
            monkeypatch.setenv("TRL_WIDE_FUSED_ROLLOUT", "1")
        pf, vf = copy.deepcopy(nets)
        env, eval_env = (SynthVecEnv(N, obs_dim=D, act_dim=A, device=dev, discrete=True) for _ in range(2))
        env.horizon = eval_env.horizon = 9
        env.seed(11)
        buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
        col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=dev, train_render=False,
                                   epoch_frames=N * T, max_episode_frames=999, eval_episodes=1, noise_mode="device")
        agent = make_agent("PPO", "cat", monkeypatch, fused, nets=(pf, vf), B=128, env=env, replay_buffer=buf, collector=col)
        assert type(agent.engine()).__name__ == ("_FusedPPO" if fused else "_GenericPPO")
        np.random.seed(4)
        torch.manual_seed(12)
        for epoch in range(2):
            col.train_one_epoch()
            agent.current_epoch = epoch
            agent.update_per_epoch()
        torch.cuda.synchronize()
        runs.append(({k: getattr(buf, "_" + k).cpu().numpy().copy() for k in ("obs", "acts", "rewards", "values", "advs")},
                     L.params_of(agent)))
    for k, v in runs[1][0].items():
        np.testing.assert_allclose(runs[0][0][k], v, rtol=1e-4, atol=1e-5, err_msg=k)
    assert np.abs(runs[0][1] - runs[1][1]).max() <= 1e-6
