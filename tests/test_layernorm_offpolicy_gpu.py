"""`add_ln=True` networks on the off-policy engines: the grouped dense-network routes with post-ops
(ops.mlp_forward_group / mlp_backward_group, with and without a _C.FoldPlan) against torch autograd in float64 and against
the ungrouped route; TwinSACQ, SAC, TwinSAC, DDPG, TD3, DQN and QR-DQN against the reference fixture
(tests/golden/layernorm_offpolicy*.npz) after each of four chained updates; graph replay, target updates, snapshots, the
collector's policy pass, and the refusals that remain.  On a tree without the feature every engine test fails at
construction with the dense kernels' LayerNorm refusal and the ops tests on the grouped routes' missing post-ops."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _layernorm_offpolicy as lo                                             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STRUCT_TAGS = ["sacq_relu", "sacq_tanh_app", "ddpg_tanh", "td3_relu_app"]     # the four (activation, append) structures


@pytest.fixture(scope="module")
def fx():
    return lo.load_fixture()


@pytest.fixture(autouse=True)
def offpolicy_layernorm_on(monkeypatch):
    """The off-policy engines carry `add_ln` nets under TRL_OFFPOLICY_LN=1 only (unset: their refusal, as before)."""
    monkeypatch.setenv("TRL_OFFPOLICY_LN", "1")


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV).contiguous()


def critic_pair(g, tag):
    """Two critics of the case's structure with different parameters (the first critic before the first and after the last
    update), on the GPU and as float64 CPU copies."""
    a = lo.args_of(g, tag)
    name = "qf1" if "qf1" in a["nets"] else "qf"
    out = []
    for i in (0, 4):
        mods = [lo.build_nets(a)[name] for _ in range(2)]
        for m in mods:
            m.load_state_dict(lo.state_of(g, f"{tag}_{name}{i}_"))
        out.append((mods[0].to(DEV), mods[1].double()))
    return a, out


def home_of(*nets):
    """The engines' flat home (`_engine.net_home`) over `nets` as twin critics, each with a copy as its target."""
    import copy
    from torchrl_amd.algo.off_policy._engine import net_home
    names = ["qf%d" % (k + 1) for k in range(len(nets))]
    return net_home(list(zip(names, nets)), [("target_" + n, copy.deepcopy(m)) for n, m in zip(names, nets)],
                    [torch.optim.Adam(m.parameters(), lr=1e-3) for m in nets], same=(tuple(names),))


def autograd_reference(cpu, x, d_out):
    from torchrl_amd import networks
    for p in cpu.parameters():
        p.grad = None
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    out = networks.Net.forward(cpu, x64)
    out.backward(torch.from_numpy(d_out).double())
    return out.detach().numpy(), [p.grad.numpy().copy() for p in cpu.parameters()], x64.grad.numpy().copy()


def close(got, want, what):
    """rel 1e-4 of the element plus 1e-5 of the tensor's largest (tests/test_layernorm_gpu.py, the ungrouped route)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else want
    e = np.abs(got.astype(np.float64) - want)
    tol = 1e-4 * np.abs(want) + 1e-5 * np.abs(want).max()
    assert (e <= tol).all(), (what, float(e.max()), float(np.abs(want).max()))
    return float((e / np.maximum(tol, 1e-30)).max())


# ---------------------------------------------------------------- 1. the grouped routes
@pytest.mark.parametrize("with_plan", [False, True])
@pytest.mark.parametrize("tag", STRUCT_TAGS)
def test_grouped_routes_vs_autograd_and_the_ungrouped_route(fx, tag, with_plan, monkeypatch):
    """Three problems as the engines pose them -- critic A on x0 and critic B on x1 with weight gradients, critic A once more
    on x2 for its input gradient alone (no dgamma / dbeta: a NULL problem of the norm launches) -- through
    ops.mlp_forward_group / mlp_backward_group, kernels only (TRL_STRICT=1).  Outputs rel 1e-4 / abs 1e-5 and every gradient
    (gamma / beta included, and d(input)) rel 1e-4 + 1e-5 of the tensor's largest, against torch autograd in float64 on the
    CPU -- the bounds of the ungrouped route's test, B <= 80 rows.  The ungrouped mlp_forward / mlp_backward of each copy
    agrees with the grouped result within the same bounds.  with_plan: the gradient views are those of the engines' flat
    home, the weight-gradient GEMMs are deferred and the norms' slabs are entries of the plan's fold: nothing but
    `plan.run()` finishes dgamma / dbeta."""
    from torchrl_amd import _C, ops
    monkeypatch.setenv("TRL_STRICT", "1")
    g, _ = fx
    a, ((netA, cpuA), (netB, cpuB)) = critic_pair(g, tag)
    B, Din = a["B"], a["D"] + a["A"]
    rs = np.random.RandomState(7)
    xs = [rs.randn(B, Din).astype(np.float32) for _ in range(3)]
    ds = [rs.randn(B, 1).astype(np.float32) for _ in range(3)]
    (lA, lB), _, act, home = home_of(netA, netB)
    assert ops.has_post(lA) and len(home.layer_views([lA, lB])[0][0]) == 4
    vA, vB = home.layer_views([lA, lB])
    before = _C.eager_fallback_count()
    outs, tapes = ops.mlp_forward_group([lA, lB, lA], [dev(x) for x in xs], act, keep=[True, True, True])
    assert all(t.posts is not None and len(t.stats) == len(lA) for t in tapes)
    home.grads.fill_(float("nan"))
    plan = _C.FoldPlan(torch.empty(1 << 22, device=DEV), defer_gemm=True) if with_plan else None
    dxs = ops.mlp_backward_group(tapes, [dev(d) for d in ds], grads_list=[vA, vB, None], need_input=[False, False, True],
                                 plan=plan)
    if with_plan:
        n_ln = sum(1 for l in lA if l[2] is not None and l[2][0] == "ln")
        assert sum(1 for e in plan.entries if e[2] == 2 * int(e[1].numel())) == 2 * n_ln     # [dgamma | dbeta] of A and of B
        torch.cuda.synchronize()
        assert bool(torch.isnan(vA[0][2]).all())                                          # not final before the fold
        assert plan.tiles(home.grads)
        plan.run()
    torch.cuda.synchronize()
    assert _C.eager_fallback_count() == before
    assert dxs[0] is None and dxs[1] is None and tuple(dxs[2].shape) == (B, Din)
    worst = 0.0
    for k, (cpu, views) in enumerate(((cpuA, vA), (cpuB, vB), (cpuA, None))):
        want_out, want_grads, want_dx = autograd_reference(cpu, xs[k], ds[k])
        e = np.abs(outs[k].cpu().numpy() - want_out)
        assert (e <= 1e-5 + 1e-4 * np.abs(want_out)).all()
        layers = (lA, lB, lA)[k]
        # the ungrouped route on the same copy
        y1, t1 = ops.mlp_forward(layers, dev(xs[k]), act)
        assert (np.abs(outs[k].cpu().numpy() - y1.cpu().numpy()) <= 1e-5 + 1e-4 * np.abs(y1.cpu().numpy())).all()
        own = [tuple(torch.zeros_like(v) for v in vs) for vs in (vA if views is None else views)]
        dx1 = ops.mlp_backward(t1, dev(ds[k]), grads=own, need_input=True)
        if views is None:
            worst = max(worst, close(dxs[2], want_dx, "dx"))
            close(dxs[2], dx1, "dx vs ungrouped")
            continue
        flat_views = [v for vs in views for v in vs]
        for got, want, single, p in zip(flat_views, want_grads, [v for vs in own for v in vs], cpu.named_parameters()):
            worst = max(worst, close(got, want, p[0]))
            close(got, single, p[0] + " vs ungrouped")
    print("%s plan=%s worst err / bound %.3f" % (tag, with_plan, worst))


def test_a_view_under_two_tapes_and_mixed_tapes_are_refused(fx):
    from torchrl_amd import _C, ops
    g, _ = fx
    a, ((netA, _), (netB, _)) = critic_pair(g, "sacq_relu")
    (lA, lB), _, act, home = home_of(netA, netB)
    vA, vB = home.layer_views([lA, lB])
    x = torch.randn(a["B"], a["D"] + a["A"], device=DEV)
    d = torch.randn(a["B"], 1, device=DEV)
    _, tapes = ops.mlp_forward_group([lA, lA], [x, x], act)
    with pytest.raises(_C.TrlError, match="under two tapes"):
        ops.mlp_backward_group(tapes, [d, d], grads_list=[vA, vA])
    plain = [(l[0], l[1]) for l in lA]
    _, t_plain = ops.mlp_forward_group([plain], [x], act)
    with pytest.raises(_C.TrlError, match="with and without post-ops"):
        ops.mlp_backward_group([tapes[0], t_plain[0]], [d, d], grads_list=[vA, vB])
    with pytest.raises(_C.TrlError, match="layer 0 has a LayerNorm"):
        ops.mlp_backward_group(tapes[:1], [d], grads_list=[[v[:2] for v in vA]])


def test_head_dx_is_ignored_behind_a_post_op_and_a_plan_is_accepted(fx):
    """`mlp_backward` of a post-op tape with a plan (refused before) runs the grouped route; a head_dx handed in although
    the last hidden layer has a LayerNorm is ignored, not an error: the gradients are those of the call without it."""
    from torchrl_amd import _C, ops
    g, _ = fx
    a, ((netA, cpuA), _) = critic_pair(g, "sacq_tanh_app")
    (lA,), _, act, home = home_of(netA)
    assert lA[-2][2][0] == "ln"
    vA, = home.layer_views([lA])
    rs = np.random.RandomState(3)
    x, d = rs.randn(a["B"], a["D"] + a["A"]).astype(np.float32), rs.randn(a["B"], 1).astype(np.float32)
    y, tape = ops.mlp_forward(lA, dev(x), act)
    ws = torch.empty(1 << 20, device=DEV)
    res = []
    for head_dx in (None, torch.full((a["B"], int(lA[-2][0].shape[0])), 1e6, device=DEV)):
        home.grads.zero_()
        plan = _C.FoldPlan(ws, defer_gemm=True)
        ops.mlp_backward(tape, dev(d), grads=vA, plan=plan, head_dx=head_dx)
        plan.run()
        res.append(home.grads.clone())
    assert torch.equal(res[0], res[1])
    _, want, _ = autograd_reference(cpuA, x, d)
    for got, w, p in zip([v for vs in vA for v in vs], want, cpuA.named_parameters()):
        close(got, w, p[0])


# ---------------------------------------------------------------- 2. the engines against the fixture
@pytest.mark.parametrize("tag", lo.TAGS)
def test_four_chained_updates_vs_fixture(fx, tag, errlog, monkeypatch):
    """After EACH of the four chained updates: every key of every state dict -- trained networks and targets, gamma / beta
    included -- abs 1e-6, log_alpha with them, info scalars rel 1e-4 / abs 1e-5 (the reference's own
    float32 run is within a quarter of these, tests/test_layernorm_offpolicy_cpu.py).  Kernels only: TRL_STRICT=1, the eager
    counter does not move."""
    from torchrl_amd import _C
    monkeypatch.setenv("TRL_STRICT", "1")
    g, _ = fx
    a = lo.args_of(g, tag)
    agent, nets, targets = lo.build_agent(g, tag, DEV)
    before = _C.eager_fallback_count()
    bad, worst_p, worst_i = [], 0.0, 0.0
    for s in range(a["steps"]):
        torch.manual_seed(100 + s)                                           # the reference's CPU draws of this update
        info = agent.update(lo.batch_of(g, tag))
        for name, mod in list(nets.items()) + targets:
            err = lo.param_error(mod, g, f"{tag}_{name}{s + 1}_")
            errlog("%s_update%d_%s" % (tag, s, name), err, lo.PARAM_BOUND)
            print("%s update %d %s parameter error %.3e" % (tag, s, name, err))
            worst_p = max(worst_p, err)
            if not err <= lo.PARAM_BOUND:
                bad.append((s, name, err))
        if a["algo"] in ("TwinSACQ", "SAC", "TwinSAC"):
            err = float(np.abs(agent.log_alpha.cpu().numpy().astype(np.float64) - g[f"{tag}_log_alpha{s + 1}"]).max())
            print("%s update %d log_alpha error %.3e" % (tag, s, err))
            if not err <= lo.PARAM_BOUND:
                bad.append((s, "log_alpha", err))
        errs = lo.info_errors(info, lo.info_of(g, tag, s))
        for k, e in errs.items():
            worst_i = max(worst_i, e)
            if not e <= 1.0:
                bad.append((s, k, info[k], lo.info_of(g, tag, s)[k]))
    print("%s worst parameter error %.3e (%.2f of the bound), worst info error %.2f of its bound"
          % (tag, worst_p, worst_p / lo.PARAM_BOUND, worst_i))
    assert _C.eager_fallback_count() == before
    assert not bad, bad


@pytest.mark.parametrize("tag,updates", [("sacq_tanh_app", 5), ("sacv", 5), ("td3_relu_app", 10), ("qrdqn_tanh", 5)])
def test_updates_replayed_from_graphs_equal_eager_updates(fx, tag, updates, monkeypatch):
    """A configuration's third and later visits replay a captured graph (TD3 has two configurations, with and without the
    delayed policy step): at least three replayed updates per configuration leave the parameters, the targets and the
    info dicts of the run that never captured, bit for bit -- the norms' slab folds have a fixed order and the graph holds
    the pointer tables of the grouped norm launches by value."""
    g, _ = fx
    results = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("TRL_NO_GRAPH", no_graph)
        agent, nets, targets = lo.build_agent(g, tag, DEV)
        infos = []
        for s in range(updates):
            torch.manual_seed(500 + s)
            infos.append(agent.update(lo.batch_of(g, tag)))
        eng = agent.engine()
        assert len(eng._graphs) == (0 if no_graph == "1" else (2 if tag.startswith("td3") else 1))
        results.append((infos, eng.flat.cpu().clone(), eng.tflat.cpu().clone()))
    (ia, fa, ta), (ib, fb, tb) = results
    assert torch.equal(fa, fb) and torch.equal(ta, tb)
    assert ia == ib and all(np.isfinite(list(i.values())).all() for i in ia)


def ln_state(mod):
    return {n + "." + k: v.detach().clone() for n, m in mod.named_modules() if isinstance(m, torch.nn.LayerNorm)
            for k, v in (("weight", m.weight), ("bias", m.bias))}


@pytest.mark.parametrize("tag", ["sacq_relu", "twinsacv", "ddpg_tanh", "dqn_relu"])
def test_targets_norm_parameters_follow_polyak_and_the_hard_copy(fx, tag):
    """The targets' gamma / beta are homed in the flat target buffer in the trained networks' order: the Polyak step moves
    them to (1 - tau) old + tau new, and the hard copy (use_soft_update=False, period 1) makes them the trained ones."""
    g, _ = fx
    source = {"tqf1": "qf1", "tqf2": "qf2", "tqf": "qf", "tvf": "vf", "tpf": "pf"}
    for soft in (True, False):
        agent, nets, targets = lo.build_agent(g, tag, DEV, use_soft_update=soft, target_hard_update_period=1)
        old = {name: ln_state(mod) for name, mod in targets}
        assert all(len(v) > 0 for v in old.values())
        torch.manual_seed(100)
        agent.update(lo.batch_of(g, tag))
        torch.cuda.synchronize()
        for name, mod in targets:
            new, src = ln_state(mod), ln_state(nets[source[name]])
            for k in new:
                if soft:
                    assert not torch.equal(new[k], old[name][k]), (name, k)
                    torch.testing.assert_close(new[k], 0.995 * old[name][k] + 0.005 * src[k], rtol=0, atol=2e-7)
                else:
                    assert torch.equal(new[k], src[k]) and not torch.equal(new[k], old[name][k]), (name, k)


@pytest.mark.parametrize("tag", ["sacq_tanh_app", "td3_relu_app", "sacv"])
def test_state_dicts_round_trip_through_snapshot(fx, tag, tmp_path):
    """After an update (the parameters are views of the engine's flat buffer by then) `snapshot` writes state dicts with
    torch's names -- the LayerNorms' `.2.weight` / `.2.bias` among them -- that load back into fresh networks bit for bit."""
    g, _ = fx
    a = lo.args_of(g, tag)
    agent, nets, _ = lo.build_agent(g, tag, DEV)
    torch.manual_seed(100)
    agent.update(lo.batch_of(g, tag))
    agent.snapshot(str(tmp_path), 0)
    fresh = lo.build_nets(a)
    for name, mod in agent.snapshot_networks:
        state = torch.load(os.path.join(str(tmp_path), "model_%s_0.pth" % name), map_location="cpu")
        assert list(state) == list(mod.state_dict()) == list(fresh[name].state_dict())
        n_ln = sum(isinstance(m, torch.nn.LayerNorm) for m in mod.modules())
        assert n_ln > 0 and sum(k.endswith(".2.weight") for k in state) == n_ln
        fresh[name].load_state_dict(state)
        for (k, x), y in zip(mod.state_dict().items(), fresh[name].state_dict().values()):
            assert torch.equal(x.cpu(), y), (name, k)
        assert not torch.equal(state[list(state)[0]], lo.state_of(g, f"{tag}_{name}0_")[list(state)[0]])


# ---------------------------------------------------------------- 3. the collector's policy pass
def test_vector_step_stores_the_action_of_the_layernorm_policy(monkeypatch):
    """One vector step of VecCollector on SynthHalfCheetah-v0, N = 8, host noise, under TRL_STRICT=1: the stored action row is
    what the policy gives on the stored observation row with the step's N(0, 1) draw -- the bits of the kernel route
    (Net.forward + the sampler on the same rows), and tanh(mean + exp(clamp(log_std)) eps) of the torch module in float64
    within rel 1e-4 / abs 1e-5."""
    import copy
    from torchrl_amd import _C, networks, policies
    from torchrl_amd.collector import VecCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers import BaseReplayBuffer
    monkeypatch.setenv("TRL_STRICT", "1")
    N = 8
    torch.manual_seed(0)
    net = dict(hidden_shapes=[24, 40], append_hidden_shapes=[20], base_type=networks.MLPBase, activation_func=torch.nn.Tanh,
               add_ln=True)
    pf = policies.GuassianContPolicy(input_shape=17, output_shape=12, tanh_action=True, **net)
    rs = np.random.RandomState(1)
    with torch.no_grad():
        for m in pf.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(torch.from_numpy((1 + 0.3 * rs.randn(*m.weight.shape)).astype(np.float32)))
                m.bias.copy_(torch.from_numpy((0.2 * rs.randn(*m.bias.shape)).astype(np.float32)))
    cpu = copy.deepcopy(pf).double()
    pf.to(DEV)
    env, ev = (get_vec_env("SynthHalfCheetah-v0", {"reward_scale": 1, "obs_norm": False}, N, device=DEV) for _ in range(2))
    env.seed(3)
    buf = BaseReplayBuffer(N * 4, env_nums=N)
    col = VecCollector(env=env, eval_env=ev, pf=pf, replay_buffer=buf, device=DEV, epoch_frames=N, max_episode_frames=999,
                       eval_episodes=1, noise_mode="host")
    assert col._one_launch_step(env, None)
    before = _C.eager_fallback_count()
    torch.manual_seed(77)
    col.train_one_epoch()
    torch.cuda.synchronize()
    assert _C.eager_fallback_count() == before and buf._top == 1
    torch.manual_seed(77)
    eps = torch.randn(N, 6)
    obs, act = buf._obs[0].clone(), buf._acts[0].clone()
    assert obs.shape == (N, 17) and act.shape == (N, 6) and bool(torch.isfinite(act).all())
    with torch.no_grad():
        head = networks.Net.forward(pf, obs)
        head64 = networks.Net.forward(cpu, obs.cpu().double())
    want_bits, _ = _C.rsample_fwd(head, eps.to(DEV), True)
    assert torch.equal(act, want_bits)
    want = torch.tanh(head64[:, :6] + torch.exp(head64[:, 6:].clamp(-20, 2)) * eps.double()).numpy()
    assert (np.abs(act.cpu().numpy() - want) <= 1e-5 + 1e-4 * np.abs(want)).all()
    ev_res = col.eval_one_epoch()                                            # the deterministic pass: the same layers
    assert len(ev_res["eval_rewards"]) == N and _C.eager_fallback_count() == before


def test_deterministic_policy_pass_of_the_collector(fx):
    """`_policy_action` of a DDPG / TD3 policy with LayerNorm: [tanh](mlp(obs)) through the plan's launches, against the
    torch module in float64."""
    from torchrl_amd import networks
    from torchrl_amd.collector.base import _policy_mlp
    g, _ = fx
    a = lo.args_of(g, "td3_relu_app")
    pf, cpu = lo.build_nets(a)["pf"], lo.build_nets(a)["pf"]
    for m in (pf, cpu):
        m.load_state_dict(lo.state_of(g, "td3_relu_app_pf0_"))
    pf.to(DEV), cpu.double()
    obs = lo.batch_of(g, "td3_relu_app")["obs"]
    from torchrl_amd import _C
    got = _policy_mlp(pf, dev(obs), last_act=_C.ACT_TANH)
    with torch.no_grad():
        want = torch.tanh(networks.Net.forward(cpu, torch.from_numpy(obs).double())).numpy()
    assert (np.abs(got.cpu().numpy() - want) <= 1e-5 + 1e-4 * np.abs(want)).all()


# ---------------------------------------------------------------- 4. what keeps refusing
def test_remaining_refusals_name_what_they_refuse(fx):
    """Bootstrapped DQN and conv trunks keep refusing LayerNorm nets with their own messages; twin critics that differ in
    `add_ln` are refused by name; a LayerNorm policy beside plain critics (and the reverse, critic_only_ln) runs."""
    import gym
    from torchrl_amd import _C, networks
    from torchrl_amd.algo import DQN
    from torchrl_amd.policies import EpsilonGreedyDQNDiscretePolicy
    g, _ = fx
    off = dict(replay_buffer=None, collector=lo.Stub(), logger=lo.Log(), discount=0.99, num_epochs=10, batch_size=8, device=DEV,
               save_dir=None, tau=0.005, use_soft_update=True, opt_times=1)

    class Env:
        action_space = gym.spaces.Discrete(4)
    with pytest.raises(_C.TrlError, match=r"BootstrappedNet\(add_ln=True\) is not built"):      # refused where the net is built
        networks.BootstrappedNet(output_shape=4, head_num=3, append_hidden_shapes=[], activation_func=torch.nn.ReLU,
                                 base_type=networks.MLPBase, input_shape=6, hidden_shapes=[16, 16], add_ln=True)
    convs = [[16, [8, 8], [4, 4], [0, 0]], [32, [4, 4], [2, 2], [0, 0]]]
    cq = networks.Net(output_shape=4, base_type=networks.CNNBase, append_hidden_shapes=[32], activation_func=torch.nn.ReLU,
                      input_shape=(4, 84, 84), hidden_shapes=convs, add_ln=True)
    agent = DQN(qf=cq, pf=EpsilonGreedyDQNDiscretePolicy(qf=cq, start_epsilon=1, end_epsilon=0.1, decay_frames=10, action_shape=4),
                qlr=1e-3, env=Env(), **off)
    with pytest.raises(_C.TrlError, match="conv kernels do not support LayerNorm"):
        agent.engine()
    a = lo.args_of(g, "sacq_relu")
    nets = lo.build_nets(a)
    nets["qf2"] = lo.build_nets(a, q_ln=False)["qf2"]
    with pytest.raises(_C.TrlError, match="qf1 and qf2 .* must agree on add_ln"):
        lo.build_agent(g, "sacq_relu", DEV, nets=nets)[0].engine()
    nets = lo.build_nets(a, q_ln=False)                                      # LayerNorm policy, plain twin critics: runs
    agent = lo.build_agent(g, "sacq_relu", DEV, nets=nets)[0]
    torch.manual_seed(1)
    info = agent.update(lo.batch_of(g, "sacq_relu"))
    assert all(np.isfinite(v) for v in info.values())


def test_without_the_switch_every_engine_refuses_as_before(fx, monkeypatch):
    """TRL_OFFPOLICY_LN unset: the engines refuse the fixture's nets with the message they have always given."""
    from torchrl_amd import _C
    monkeypatch.delenv("TRL_OFFPOLICY_LN")
    g, _ = fx
    for tag in lo.TAGS:
        with pytest.raises(_C.TrlError, match="without LayerNorm"):
            lo.build_agent(g, tag, DEV)[0].engine()
