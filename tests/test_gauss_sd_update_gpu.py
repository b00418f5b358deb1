"""The fused two-launch PPO / A2C update for state-dependent-std Gaussian policies (ppo_grad_wave_kernel<..., SD>,
trl_ppo_sd_*): the reference fixture through the fused engine, the engine choice, gradients and statistics against the
float64 restatement (tests/_gauss_sd_ref.py), exact zeros behind the clamp, the single-network launches against the joint
one, the fused against the generic engine, the engine's launch modes, and whole iterations on the fused rollout.
Tolerances are the project's: scalars rel 1e-4 / abs 1e-5, post-step parameters abs 1e-6, gradients
1e-4 of the network's largest entry.  The fixture test fails on a build without the fused update."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _gauss_sd_ref as ref                                                   # noqa: E402
import _gauss_sd_update_cases as su                                           # noqa: E402

pytestmark = pytest.mark.gpu
SWITCH = "TRL_SD_FUSED_UPDATE"                                                # the fused update is opt-in
DEV = torch.device("cuda:0")
H = su.H


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


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("TRL_GENERIC_PPO", "TRL_PPO_CHAINS", "TRL_NO_GRAPH", "TRL_NO_RT_ROLLOUT", SWITCH, "TRL_SD_FUSED_ROLLOUT"):
        monkeypatch.delenv(k, raising=False)


def dev(x, dtype=None):
    t = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def make_agent(algo_cls, pf, vf, D, A, B, **kw):
    from torchrl_amd.env.synth import SynthVecEnv
    return algo_cls(pf=pf, vf=vf, tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, gae=True,
                    env=SynthVecEnv(4, obs_dim=D, act_dim=A, device=DEV), replay_buffer=None,
                    collector=_Stub(), logger=_Log(), device=DEV, save_dir=None, **kw)


def fixture_agent(g, tag, algo_cls, **kw):
    """The fixture's networks (the reference's draw for that seed, the policy's overwritten log_std rows loaded on top)."""
    D, A, Hh, B, tanh = (int(x) for x in g[f"{tag}_args"])
    pf, vf = su.nets_of(D, A, 5 + D, hidden=(Hh, Hh), tanh=bool(tanh))
    pf.load_state_dict({k: torch.from_numpy(g[f"{tag}_pf0_" + k.replace(".", "__")].copy()) for k in pf.state_dict()})
    return pf, vf, make_agent(algo_cls, pf, vf, D, A, B, **kw)


def param_error(mod, g, prefix):
    return max((a.detach().cpu() - b).abs().max().item() for a, b in zip(su.linear_params(mod), ref.params_from(g, prefix)))


def assert_info(info, g, prefix, errlog, label):
    want = ref.info_of(g, prefix)
    assert sorted(info) == sorted(want)
    worst = 0.0
    for k in sorted(want):
        print("%s %s got %.9g want %.9g" % (prefix, k, info[k], want[k]))
        worst = max(worst, abs(info[k] - want[k]) / (1e-5 + 1e-4 * abs(want[k])))
    errlog(label + "_info_worst_over_bound", worst, 1.0)
    for k in sorted(want):
        assert info[k] == pytest.approx(want[k], rel=1e-4, abs=1e-5), k


def is_fused(eng):
    return type(eng).__name__ == "_FusedPPO" and eng.state_std and not eng.categorical


# ---------------------------------------------------------------- 1. the reference fixture through the fused engine
@pytest.mark.parametrize("tag", ["t_s17", "n_s17"])
def test_fixture_a2c_and_ppo_on_the_fused_engine(g, tag, monkeypatch, errlog):
    from torchrl_amd.algo import A2C, PPO
    monkeypatch.setenv(SWITCH, "1")
    assert tuple(int(x) for x in g[f"{tag}_args"])[:4] == (17, 6, 64, 96)
    pf, vf, agent = fixture_agent(g, tag, A2C, plr=3e-4, vlr=1e-3, entropy_coeff=0.01)
    info = agent.update(ref.batch_of(g, tag))
    eng = agent.engine()
    assert is_fused(eng) and not hasattr(pf, "logstd") and eng.A == 6
    assert eng.P_pf == sum(p.numel() for p in su.linear_params(pf)) == 64 * 17 + 64 + 4096 + 64 + 64 * 12 + 12
    assert_info(info, g, f"{tag}_a2c_info", errlog, "a2c_" + tag)
    for name, mod in (("pf", pf), ("vf", vf)):
        err = param_error(mod, g, f"{tag}_a2c_{name}1_")
        errlog("a2c_%s_%s" % (tag, name), err, 1e-6)
        assert err <= 1e-6, (name, err)

    pf, vf, agent = fixture_agent(g, tag, PPO, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, entropy_coeff=0.005)
    agent.current_epoch = 3
    tgt = {k[len(f"{tag}_ppo_tpf0_"):].replace("__", "."): torch.from_numpy(g[k].copy())
           for k in g.files if k.startswith(f"{tag}_ppo_tpf0_")}
    agent.target_pf.load_state_dict(tgt)
    assert len(g[f"{tag}_ppo_clipv"]) == 4
    for s, clipv in enumerate(g[f"{tag}_ppo_clipv"]):
        agent.clipped_value_loss = bool(clipv)
        info = agent.update(ref.batch_of(g, tag))
        assert_info(info, g, f"{tag}_ppo_info{s}", errlog, "ppo_%s_update%d" % (tag, s))
        for name, mod in (("pf", pf), ("vf", vf)):
            err = param_error(mod, g, f"{tag}_ppo_{name}{s + 1}_")
            errlog("ppo_%s_update%d_%s" % (tag, s, name), err, 1e-6)
            assert err <= 1e-6, (s, name, err)
    assert is_fused(agent.engine())
    # H = 32: not a shape the fused kernels carry -- the generic engine, switch or not
    _, _, small = fixture_agent(g, tag.replace("s17", "s3"), A2C, plr=3e-4, vlr=1e-3, entropy_coeff=0.01)
    assert int(g[tag.replace("s17", "s3") + "_args"][2]) == 32
    assert type(small.engine()).__name__ == "_GenericPPO" and small.engine().state_std


# ---------------------------------------------------------------- 2. engine choice
def test_engine_choice(monkeypatch):
    """Without the switch nothing changes; with it, only Adam on 64-wide matching nets with 1-8 action dimensions on one rank
    takes the fused engine."""
    from torchrl_amd import dist
    from torchrl_amd.algo import A2C

    def mk(hidden=(64, 64), A=6, **kw):
        pf, vf = su.nets_of(17, A, 1, hidden=hidden)
        return make_agent(A2C, pf, vf, 17, A, 64, **kw)
    generic = lambda agent: type(agent.engine()).__name__ == "_GenericPPO" and agent.engine().state_std
    assert generic(mk())
    monkeypatch.setenv(SWITCH, "1")
    assert is_fused(mk().engine())
    assert is_fused(mk(A=1).engine()) and is_fused(mk(A=8).engine())
    assert generic(mk(hidden=(64, 32)))
    assert generic(mk(hidden=(32, 32)))
    assert generic(mk(A=9))
    assert generic(mk(optimizer_class=torch.optim.RMSprop))
    monkeypatch.setenv(SWITCH, "0")
    assert generic(mk())
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("TRL_GENERIC_PPO", "1")
    assert generic(mk())
    monkeypatch.delenv("TRL_GENERIC_PPO")
    # ranks active: the choice falls on the generic engine (which then refuses the head on several ranks, as before)
    agent = mk()
    monkeypatch.setattr(dist, "collectives_active", lambda: True)
    from torchrl_amd import _C
    with pytest.raises(_C.TrlError, match="one rank"):
        agent.engine()


# ---------------------------------------------------------------- direct kernel calls
def flat_of(x):
    flat = torch.cat([p.reshape(-1) for p in x["pf"] + x["vf"]])
    return flat, sum(p.numel() for p in x["pf"]), sum(p.numel() for p in x["vf"])


def adv_raw_of(advs):
    a = advs.double().reshape(-1)
    return torch.tensor([a.sum(), (a * a).sum(), a.max(), -a.min()], dtype=torch.float64)


class Launch:
    """Device copies of an input set and the descriptor of trl_ppo_sd_minibatch_grad_f32 on them."""

    def __init__(self, x):
        from torchrl_amd import _C
        self.x = x
        self.t = {k: dev(x[k]) for k in ("obs", "acts", "advs", "rets", "old_values", "old_logp")}
        self.row_idx = dev(x["row_idx"])
        self.raw = dev(adv_raw_of(su.minibatch(x)["advs"]))
        flat, self.P_pf, self.P_vf = flat_of(x)
        self.flat0 = dev(flat)
        self.ps = _C.ppo_sd_partial_stride(x["D"], H, x["A"])
        self.sw = _C.ppo_sd_scalar_stride()
        self.act = _C.ACT_TANH if x["act"] == "tanh" else _C.ACT_RELU

    def args(self, flat, loss_mode, clipv, n_wg, n_wg_pf, partial, scal):
        from torchrl_amd import _C
        x, g = self.x, _C.PpoBatchArgs()
        for k, v in self.t.items():
            setattr(g, k, v.data_ptr())
        if loss_mode == ref.LOSS_A2C:
            g.old_logp = None                                                # A2C never reads log pi_old
        if not clipv:
            g.old_values = None
        g.row_idx, g.rows_mb, g.N = self.row_idx.data_ptr(), x["rows"], x["N"]
        g.adv_raw, g.n_global = self.raw.data_ptr(), float(x["rows"] * x["N"])
        g.pf_params, g.vf_params = flat.data_ptr(), flat.data_ptr() + 4 * self.P_pf
        g.D, g.H, g.A, g.act = x["D"], H, x["A"], self.act
        g.clip_para, g.entropy_coeff, g.clipped_value_loss, g.tanh_action = su.CLIP, su.C_ENT, int(clipv), int(x["tanh"])
        g.loss_mode = loss_mode
        g.partial, g.scal_partial, g.n_wg, g.n_wg_pf = partial.data_ptr(), scal.data_ptr(), n_wg, n_wg_pf
        return g

    def rows(self, n):
        # (filled with NaN: every slot the fold reads has to be written by the launch)
        return (torch.full((n, self.ps), float("nan"), device=DEV),
                torch.full((n * self.sw,), float("nan"), dtype=torch.float64, device=DEV))


def restatement_fp64(x, loss_mode, clipv):
    """Gradients by float64 autograd of the restatement's objective, and its info row."""
    mb = su.minibatch(x)
    pf = [p.double().requires_grad_(True) for p in x["pf"]]
    vf = [p.double().requires_grad_(True) for p in x["vf"]]
    obs = mb["obs"].double()
    head, v = su.forward(pf, obs, x["act"]), su.forward(vf, obs, x["act"])
    a = (mb["acts"].double(), mb["advs"].double().reshape(-1), mb["rets"].double(), mb["old_values"].double(),
         mb["old_logp"].double(), su.CLIP, su.C_ENT, clipv, loss_mode, x["tanh"])
    pl, vl, _ = ref.objective(head, v, *a)
    (pl + vl).backward()                                                      # (disjoint parameters: each gets its own loss's gradient)
    info = ref.losses(head.detach(), v.detach(), *a)["info"]
    return torch.cat([p.grad.reshape(-1) for p in pf]), torch.cat([p.grad.reshape(-1) for p in vf]), info


SUM_SLOTS = (0, 1, 7, 20)


# ---------------------------------------------------------------- 3. + 4. gradients, statistics, the clamp's exact zeros
@pytest.mark.parametrize("c", su.GRAD_CASES, ids=su.case_id)
def test_gradients_and_statistics_vs_fp64_restatement(c, errlog):
    from torchrl_amd import _C
    x = su.grad_inputs(c)
    L = Launch(x)
    D, A, n_wg, B = x["D"], x["A"], x["n_wg"], x["rows"] * x["N"]
    for loss_mode, clipv in su.LOSSES:
        label = "mode%d_clipv%d" % (loss_mode, int(clipv))
        partial, scal = L.rows(n_wg)
        grads = torch.full((L.P_pf + L.P_vf,), float("nan"), device=DEV)
        info = torch.full((24,), float("nan"), dtype=torch.float64, device=DEV)
        _C.ppo_sd_minibatch_grad(L.args(L.flat0, loss_mode, clipv, n_wg, 0, partial, scal), DEV)
        _C.ppo_sd_reduce(partial, scal, n_wg, D, H, A, grads, info)
        got = grads.cpu().double()
        assert torch.isfinite(got).all()
        want_pf, want_vf, winfo = restatement_fp64(x, loss_mode, clipv)
        for name, gg, ww in (("pf", got[:L.P_pf], want_pf), ("vf", got[L.P_pf:], want_vf)):
            err, top = (gg - ww).abs().max().item(), ww.abs().max().item()
            errlog("%s_%s_grad_over_max" % (label, name), err / top, 1e-4)
            print("%s %s %s: max abs err %.3e, max |grad| %.3e" % (su.case_id(c), label, name, err, top))
            assert err <= 1e-4 * top, (label, name, err, top)
        i = info.cpu().numpy()
        # sums over the minibatch: the project's bound on the logged MEAN, i.e. rel 1e-4 / abs 1e-5 * B on the sum
        worst = 0.0
        for k in SUM_SLOTS:
            worst = max(worst, abs(i[k] - winfo[k]) / (1e-5 * B + 1e-4 * abs(winfo[k])))
        for k in (8, 9, 10, 11, 16, 17, 18, 19):
            worst = max(worst, abs(i[k] - winfo[k]) / (1e-5 + 1e-4 * abs(winfo[k])))
        errlog(label + "_info_worst_over_bound", worst, 1.0)
        print("%s %s info %s want %s" % (su.case_id(c), label, i[:21], winfo[:21]))
        for k in SUM_SLOTS:
            assert i[k] == pytest.approx(winfo[k], rel=1e-4, abs=1e-5 * B), (label, k)
        for k in (8, 9, 10, 11, 16, 17, 18, 19):
            assert i[k] == pytest.approx(winfo[k], rel=1e-4, abs=1e-5), (label, k)
        if x["clamp"]:
            # the gate: a clamped element contributes an exact zero, so a wholly clamped column's head row gets exactly 0
            off_w3 = 64 * D + 64 + 4096 + 64
            gw3, gb3 = got[off_w3:off_w3 + 2 * A * 64].reshape(2 * A, 64), got[off_w3 + 2 * A * 64:off_w3 + 2 * A * 64 + 2 * A]
            for k in su.clamp_columns(A):
                assert bool((gw3[A + k] == 0.0).all()) and gb3[A + k].item() == 0.0, (label, k)
            free = [k for k in range(A) if k not in su.clamp_columns(A)]
            assert all(bool((gw3[A + k] != 0.0).any()) and gb3[A + k].item() != 0.0 for k in free)
            assert i[10] == 2.0 and i[11] == -20.0
            # (every slot the fold reads: the policy's rows up to P_pf, the value net's up to P_vf)
            assert np.isfinite(i[:21]).all()
            assert torch.isfinite(partial[:n_wg // 2, :L.P_pf]).all() and torch.isfinite(partial[n_wg // 2:, :L.P_vf]).all()


# ---------------------------------------------------------------- 5. single-network launches
def adam_args(flat, grads, m, v, P_pf, P_vf, norms, step):
    from torchrl_amd import _C
    a = _C.AdamArgs()
    a.params, a.grads, a.exp_avg, a.exp_avg_sq = flat.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr()
    a.n_groups = 2
    a.group_sizes[0], a.group_sizes[1] = P_pf, P_vf
    a.group_lr[0], a.group_lr[1] = 3e-4, 1e-3
    a.max_norm, a.beta1, a.beta2, a.eps, a.grad_scale = 0.5, 0.9, 0.999, 1e-5, 1.0
    a.step_count, a.norms_out, a.device_state = step, norms.data_ptr(), 0
    return a


@pytest.mark.parametrize("c", su.NET_CASES, ids=su.case_id)
def test_single_network_launches_match_the_joint_launch_bitwise(c):
    from torchrl_amd import _C
    lib = _C.lib()
    x = su.grad_inputs(c)
    L = Launch(x)
    per_net = x["n_wg"] // 2
    n_ws = lib.trl_ppo_sd_reduce_adam_workspace(x["D"], H, x["A"])
    rs = np.random.RandomState(5)
    P = L.P_pf + L.P_vf
    m0, v0 = dev(rs.randn(P).astype(np.float32) * 1e-3), dev((rs.rand(P).astype(np.float32) + 0.1) * 1e-5)
    stream = _C.stream_ptr(DEV)

    def state():
        return dict(flat=L.flat0.clone(), m=m0.clone(), v=v0.clone(), grads=torch.zeros(P, device=DEV),
                    info=torch.zeros(2, 24, dtype=torch.float64, device=DEV), norms=torch.zeros(2, 2, device=DEV))

    for loss_mode, clipv in su.LOSSES:
        joint, split = state(), state()
        ws = [torch.zeros(n_ws, device=DEV) for _ in range(3)]
        for step in (0, 1):                                                   # two steps: the second reads stepped parameters and moments
            s = joint
            partial, scal = L.rows(2 * per_net)
            _C.ppo_sd_minibatch_grad(L.args(s["flat"], loss_mode, clipv, 2 * per_net, per_net, partial, scal), DEV)
            a = adam_args(s["flat"], s["grads"], s["m"], s["v"], L.P_pf, L.P_vf, s["norms"][step], 3 + step)
            _C.check(lib.trl_ppo_sd_reduce_adam_f32(partial.data_ptr(), scal.data_ptr(), 2 * per_net, per_net, x["D"], H, x["A"],
                                                    s["grads"].data_ptr(), s["info"][step].data_ptr(), C.byref(a),
                                                    ws[0].data_ptr(), stream), "trl_ppo_sd_reduce_adam_f32")
            s = split
            for net, n_wg_pf in ((0, per_net), (1, -1)):
                partial, scal = L.rows(per_net)
                _C.ppo_sd_minibatch_grad(L.args(s["flat"], loss_mode, clipv, per_net, n_wg_pf, partial, scal), DEV)
                a = adam_args(s["flat"], s["grads"], s["m"], s["v"], L.P_pf, L.P_vf, s["norms"][step], 3 + step)
                _C.check(lib.trl_ppo_sd_reduce_adam_net_f32(partial.data_ptr(), scal.data_ptr(), per_net, net, x["D"], H, x["A"],
                                                            s["grads"].data_ptr(), s["info"][step].data_ptr(), C.byref(a),
                                                            ws[1 + net].data_ptr(), stream), "trl_ppo_sd_reduce_adam_net_f32")
        torch.cuda.synchronize()
        assert all(int(w[:1].view(torch.int32).item()) == 0 for w in ws)      # no norm rendezvous timed out
        for k in ("flat", "m", "v", "grads", "norms", "info"):
            assert torch.equal(joint[k], split[k]), (loss_mode, clipv, k)
        assert not torch.equal(joint["flat"], L.flat0) and torch.isfinite(joint["flat"]).all()
        assert torch.isfinite(joint["info"][:, :21]).all() and (joint["norms"] > 0).all()
        assert (joint["info"][:, 16] > 0).all() and (joint["info"][:, 20] != 0).all()


# ---------------------------------------------------------------- 6. fused against generic engine
def engine_tensors(x, old_logp):
    t = {k: dev(x[k]) for k in ("obs", "acts", "advs", "rets", "old_values")}
    t["old_logp"] = dev(old_logp)
    return t


def all_params(pf, vf):
    return torch.cat([p.detach().reshape(-1) for p in su.linear_params(pf) + su.linear_params(vf)]).clone()


@pytest.mark.parametrize("c", su.ENGINE_CASES, ids=lambda c: "D%d_A%d" % c[:2])
def test_fused_engine_vs_generic_engine(c, monkeypatch, errlog):
    from torchrl_amd.algo import PPO
    x = su.engine_inputs(c)
    D, A, seed = c
    _, old_logp = su.engine_old_logp(x)
    B = su.ENGINE_ROWS_MB * su.ENGINE_N
    kw = dict(plr=3e-4, vlr=1e-3, clip_para=su.CLIP, opt_epochs=1, entropy_coeff=su.C_ENT, clipped_value_loss=True)
    agents = []
    for switch in ("0", "1"):
        monkeypatch.setenv(SWITCH, switch)
        pf, vf = su.nets_of(D, A, seed)
        agent = make_agent(PPO, pf, vf, D, A, B, **kw)
        agents.append((pf, vf, agent, agent.engine(), engine_tensors(x, old_logp)))
    (gpf, gvf, _, geng, gt), (fpf, fvf, _, feng, ft) = agents
    assert type(geng).__name__ == "_GenericPPO" and geng.state_std and is_fused(feng)
    start = all_params(fpf, fvf)
    assert torch.equal(all_params(gpf, gvf), start)
    for e, row_idx in enumerate(x["epochs"]):
        gi, fi = geng.run(gt, row_idx, su.ENGINE_N), feng.run(ft, row_idx, su.ENGINE_N)
        err = (all_params(gpf, gvf) - all_params(fpf, fvf)).abs().max().item()
        errlog("epoch%d_params" % e, err, 1e-6)
        assert err <= 1e-6, (e, err)
        assert len(gi) == len(fi) == len(row_idx)
        worst = 0.0
        for a, b in zip(gi, fi):
            assert sorted(a) == sorted(b) and "log_std/mean" in b
            for k in a:
                worst = max(worst, abs(a[k] - b[k]) / (1e-5 + 1e-4 * abs(a[k])))
        errlog("epoch%d_info_worst_over_bound" % e, worst, 1.0)
        for a, b in zip(gi, fi):
            for k in a:
                assert b[k] == pytest.approx(a[k], rel=1e-4, abs=1e-5), (e, k)
    assert not torch.equal(all_params(fpf, fvf), start)


# ---------------------------------------------------------------- 7. engine modes
def run_mode(x, old_logp, chains, monkeypatch, no_graph=False):
    from torchrl_amd.algo import PPO
    monkeypatch.setenv(SWITCH, "1")
    if chains is None:
        monkeypatch.delenv("TRL_PPO_CHAINS", raising=False)                  # the default: two chains
    else:
        monkeypatch.setenv("TRL_PPO_CHAINS", chains)
    if no_graph:
        monkeypatch.setenv("TRL_NO_GRAPH", "1")
    else:
        monkeypatch.delenv("TRL_NO_GRAPH", raising=False)
    pf, vf = su.nets_of(x["D"], x["A"], x["seed"])
    agent = make_agent(PPO, pf, vf, x["D"], x["A"], su.ENGINE_ROWS_MB * su.ENGINE_N, plr=3e-4, vlr=1e-3, clip_para=su.CLIP,
                       opt_epochs=1, entropy_coeff=su.C_ENT)
    eng = agent.engine()
    assert is_fused(eng) and eng.two_chains == (chains != "joint")
    t = engine_tensors(x, old_logp)
    out = []
    for e in range(3):                                                        # eager, captured, replayed
        infos = eng.run(t, x["epochs"][e], su.ENGINE_N)
        torch.cuda.synchronize()
        out.append((all_params(pf, vf), eng.m.clone(), eng.v.clone(), infos))
    replayed = bool(eng._chain_graphs) if chains != "joint" else eng._graph is not None
    assert replayed == (not no_graph)                                         # the third epoch came from captured graphs
    return out


def test_engine_modes_are_bit_identical_and_deterministic(monkeypatch):
    from torchrl_amd import _C
    x = su.engine_inputs(su.ENGINE_CASES[1])
    _, old_logp = su.engine_old_logp(x)
    before = _C.eager_fallback_count()
    two = run_mode(x, old_logp, None, monkeypatch)
    assert _C.eager_fallback_count() == before                                # kernels only, whole epochs
    joint = run_mode(x, old_logp, "joint", monkeypatch)
    eager = run_mode(x, old_logp, None, monkeypatch, no_graph=True)
    again = run_mode(x, old_logp, None, monkeypatch)
    assert _C.eager_fallback_count() == before
    for other in (joint, eager, again):
        for e, ((p0, m0, v0, i0), (p1, m1, v1, i1)) in enumerate(zip(two, other)):
            assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1), e
            assert len(i0) == len(i1) and all(a == b for a, b in zip(i0, i1)), e
    assert not torch.equal(two[0][0], two[2][0])
    assert all(np.isfinite(list(i.values())).all() for ep in two for i in ep[3])


# ---------------------------------------------------------------- 8. whole iterations with both fused routes
@pytest.mark.parametrize("algo", ["PPO", "A2C"])
def test_whole_iterations_on_the_fused_rollout_and_the_fused_update(algo, monkeypatch):
    from torchrl_amd import _C, algo as algos
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("TRL_SD_FUSED_ROLLOUT", "1")
    N, T, B = 64, 16, 256
    np.random.seed(4)
    pf, vf = su.nets_of(17, 6, 0)
    env, eval_env = (get_vec_env("SynthHalfCheetah-v0", {"reward_scale": 1, "obs_norm": False}, N, device=DEV) for _ in range(2))
    for e_ in (env, eval_env):
        e_.horizon = 9
    env.seed(2)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               epoch_frames=N * T, max_episode_frames=999, eval_episodes=1, noise_mode="device")
    assert col._spec is not None and col._sd                                  # the one-launch rollout
    logger = _Log()
    later = []
    logger.add_update_infos_later = later.append                              # deferred statistics
    general = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B, gae=True, env=env, replay_buffer=buf,
                   collector=col, logger=logger, device=DEV, save_dir=None)
    if algo == "PPO":
        agent = algos.PPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, clip_para=0.2, opt_epochs=2, entropy_coeff=0.005, **general)
    else:
        agent = algos.A2C(pf=pf, vf=vf, plr=3e-4, vlr=1e-3, entropy_coeff=0.01, **general)
    eng = agent.engine()
    assert is_fused(eng)
    before = _C.eager_fallback_count()
    p0 = eng.flat.clone()
    for epoch in range(2):
        res = col.train_one_epoch()
        agent.current_epoch = epoch
        agent.update_per_epoch()
        assert np.isfinite(float(res["train_epoch_reward"]))
    for resolve in later:
        logger.infos.extend(dict(d) for d in resolve())
    torch.cuda.synchronize()
    assert _C.eager_fallback_count() == before
    assert len(logger.infos) == eng.step_count > 0
    assert all(np.isfinite(list(i.values())).all() for i in logger.infos)
    assert torch.isfinite(eng.flat).all() and not torch.equal(p0, eng.flat)
    assert buf._acts.shape == (T, N, 6) and is_fused(agent.engine())
    if algo == "PPO":
        # log pi_old is the rollout kernel's, log pi the gradient kernel's: two summation orders of the same terms
        first = logger.infos[0]
        print("first minibatch: ratio/max %.9f ratio/min %.9f" % (first["ratio/max"], first["ratio/min"]))
        assert abs(first["ratio/max"] - 1.0) <= 1e-4 and abs(first["ratio/min"] - 1.0) <= 1e-4
        assert "log_std/mean" in first
    else:
        assert "std/mean" in logger.infos[0]
