"""SAC and TwinSAC (soft actor-critics with a value network) on the GPU: the whole update against the fixture the
reference's own classes wrote (tests/golden/make_golden_sac_v.py), graph replay against eager launches, the deferred
and whole-epoch paths, training through RLAlgo and the two example scripts.  The bounds are the project's for the same
arithmetic (tests/test_sac_gpu.py::test_twin_sac_q_update_matches_reference)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _sac_v_ref as R                                                        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(HERE)


class _Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


def make_nets(twin, H, D=R.D, A=R.A):
    import torchrl.networks as networks
    import torchrl.policies as policies
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.ReLU)
    nets = {"pf": policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net)}
    for name in (("qf1", "qf2") if twin else ("qf",)):
        nets[name] = networks.QNet(input_shape=D + A, output_shape=1, **net)
    nets["vf"] = networks.Net(input_shape=D, output_shape=1, **net)
    return nets


def build(g, tag, **over):
    """The agent of fixture case `tag` at its stored initial state."""
    from torchrl.algo import SAC, TwinSAC
    from torchrl.env.synth import SynthVecEnv
    H, B, w_reg, clip, tune, steps = g[tag + "_args"]
    twin = str(g[tag + "_class"]) == "TwinSAC"
    nets = make_nets(twin, int(H))
    for name, mod in nets.items():
        mod.load_state_dict({k: torch.as_tensor(v) for k, v in R.state_dict_of(g, "%s_%s0_" % (tag, name)).items()})

    class Stub:
        epoch_frames = 0
    kw = dict(plr=3e-4, vlr=1e-3, qlr=1e-3, policy_std_reg_weight=float(w_reg), policy_mean_reg_weight=float(w_reg),
              reparameterization=True, automatic_entropy_tuning=bool(tune), env=SynthVecEnv(4, device=torch.device(DEV)),
              replay_buffer=None, collector=Stub(), logger=_Log(), grad_clip=float(clip) if clip > 0 else None, discount=0.99,
              num_epochs=10, batch_size=int(B), device=torch.device(DEV), save_dir=None, tau=0.005, use_soft_update=True,
              opt_times=1)
    kw.update(over)
    return (TwinSAC if twin else SAC)(**nets, **kw), nets, int(B), int(steps)


@pytest.mark.parametrize("tag", R.CASES)
def test_update_matches_reference(tag):
    g = R.load_fixture()
    agent, nets, B, steps = build(g, tag)
    vf0 = {k: v.detach().cpu().clone() for k, v in nets["vf"].state_dict().items()}
    for s in range(steps):
        batch = {k: g["%s_s%d_batch_%s" % (tag, s, k)] for k in R.BATCH_KEYS}
        torch.manual_seed(100 + s)                                       # the reference's one CPU draw per update
        info = agent.update(batch)
        keys = [str(k) for k in g["%s_s%d_info_keys" % (tag, s)]]
        assert sorted(info.keys()) == keys
        got = np.array([info[k] for k in keys])
        np.testing.assert_allclose(got, g["%s_s%d_info_vals" % (tag, s)], rtol=2e-4, atol=5e-5)
        if tag == "twin_fixed":
            assert "Alpha" not in info and "Alpha_loss" not in info
            if s == 0:                                                   # exactly one Polyak step from the initial V:
                for k, t in agent.target_vf.state_dict().items():        # (1 - tau) V0 + tau V1 to four fp32 roundings
                    want = vf0[k].double() * (1.0 - 0.005) + nets["vf"].state_dict()[k].cpu().double() * 0.005
                    assert float((t.cpu().double() - want).abs().max()) <= 4 * R.U * float(want.abs().max()), k
                    assert float((t.cpu() - vf0[k]).abs().max()) > 0
    worst = 0.0
    for name, mod in list(nets.items()) + [("tvf", agent.target_vf)]:
        for k, p in mod.state_dict().items():
            err = np.abs(p.cpu().numpy() - g["%s_%s1_%s" % (tag, name, k.replace(".", "__"))]).max()
            worst = max(worst, float(err))
            assert err < 3e-6, (name, k, err)
    print("RATIO sac_v update %s: parameters %.4f" % (tag, worst / 3e-6))
    if tag + "_log_alpha" in g:
        np.testing.assert_allclose(agent.log_alpha.cpu().numpy(), g[tag + "_log_alpha"], atol=1e-6)
    else:
        assert float(agent.log_alpha) == 0.0 and float(agent.engine().alpha_out[0]) == 1.0
    assert float(agent.vf_optimizer.state[nets["vf"].seq_append_fcs[0].weight]["exp_avg"].abs().sum()) > 0


def _batches(B, count, seed):
    gen = torch.Generator().manual_seed(seed)
    return [{"obs": torch.randn(B, R.D, generator=gen), "next_obs": torch.randn(B, R.D, generator=gen),
             "acts": torch.rand(B, R.A, generator=gen) * 2 - 1, "rewards": torch.randn(B, 1, generator=gen),
             "terminals": (torch.rand(B, 1, generator=gen) < 0.2).float()} for _ in range(count)]


@pytest.mark.parametrize("tag", ["sac_reg", "twin_reg"])
def test_graph_replayed_updates_equal_eager_updates(tag, monkeypatch):
    """Updates 3+ of a configuration replay a captured HIP graph: the same launches, so parameters, target, log_alpha and
    the logged statistics are bit-identical to the eager sequence; one graph is cached."""
    g = R.load_fixture()
    B = int(g[tag + "_args"][1])
    batches = _batches(B, 6, seed=11)
    results = []
    for no_graph in ("1", "0"):
        monkeypatch.setenv("TRL_NO_GRAPH", no_graph)
        agent, nets, _, _ = build(g, tag)
        infos = []
        for s, b in enumerate(batches):
            torch.manual_seed(500 + s)
            infos.append(agent.update(b))
        eng = agent.engine()
        assert len(eng._graphs) == (0 if no_graph == "1" else 1)
        assert eng.step_state.cpu().tolist()[0] == len(batches)
        results.append((infos, eng.flat.cpu().clone(), eng.tflat.cpu().clone(), agent.log_alpha.cpu().clone()))
    (ia, fa, ta, la), (ib, fb, tb, lb) = results
    assert torch.equal(fa, fb) and torch.equal(ta, tb) and torch.equal(la, lb)
    assert ia == ib and len({i["Training/vf_loss"] for i in ia}) == 6


def _train_setup(twin, H=64, N=64, B=256, opt_times=4, noise="device", rows=64, **over):
    from torchrl.algo import SAC, TwinSAC
    from torchrl.collector import VecCollector
    from torchrl.env.synth import SynthVecEnv
    from torchrl.replay_buffers import BaseReplayBuffer
    dev = torch.device(DEV)
    torch.manual_seed(21)
    nets = make_nets(twin, H)
    env, ev = SynthVecEnv(N, horizon=20, device=dev), SynthVecEnv(N, horizon=20, device=dev)
    env.seed(0)
    buf = BaseReplayBuffer(N * rows, env_nums=N)
    col = VecCollector(env=env, eval_env=ev, pf=nets["pf"], replay_buffer=buf, device=dev, epoch_frames=N * 8,
                       max_episode_frames=999, eval_episodes=1, noise_mode=noise)
    kw = dict(plr=3e-4, vlr=3e-4, qlr=3e-4, policy_std_reg_weight=0, policy_mean_reg_weight=0, reparameterization=True,
              automatic_entropy_tuning=True, noise_mode=noise, env=env, replay_buffer=buf, collector=col, logger=_Log(),
              discount=0.99, num_epochs=3, batch_size=B, device=dev, save_dir=None, tau=0.005, use_soft_update=True,
              opt_times=opt_times, pretrain_epochs=1, eval_interval=1)
    kw.update(over)
    return (TwinSAC if twin else SAC)(**nets, **kw), nets, col


def _deferred_run(twin, mode, epochs=3, noise="device"):
    """mode: "update" (sample -> update, read back each), "deferred" (update_deferred + one resolve per epoch, the
    whole-epoch hook declining), "epoch" (update_per_epoch as shipped: update_epoch_deferred where it applies)."""
    agent, nets, col = _train_setup(twin, noise=noise)
    torch.manual_seed(5)
    col.train_one_epoch()
    np.random.seed(9)
    for _ in range(epochs):
        if mode == "update":
            for _ in range(agent.opt_times):
                agent._one_update()
        elif mode == "deferred":
            handles = [agent.update_deferred(agent._sample()) for _ in range(agent.opt_times)]
            for info in agent.resolve_updates(handles):
                agent.logger.add_update_info(info)
        else:
            agent.update_per_epoch()
    eng = agent.engine()
    return agent.logger.infos, eng.flat.cpu().clone(), eng.tflat.cpu().clone(), agent.log_alpha.cpu().clone(), agent


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "single"])
def test_deferred_and_whole_epoch_paths_equal_update_by_update(twin):
    """Device noise: `update_deferred` + `resolve_updates` give the infos of `update`, and `update_epoch_deferred(4)`
    (eager, captured, replayed) equals four sample -> update pairs bit for bit."""
    ia, fa, ta, la, _ = _deferred_run(twin, "update")
    ib, fb, tb, lb, _ = _deferred_run(twin, "deferred")
    ic, fc, tc, lc, agent = _deferred_run(twin, "epoch")
    assert len(ia) == len(ib) == len(ic) == 12
    for infos, f, t, l in ((ib, fb, tb, lb), (ic, fc, tc, lc)):
        assert torch.equal(fa, f) and torch.equal(ta, t) and torch.equal(la, l)
        assert infos == ia
    assert len({i["Training/vf_loss"] for i in ic}) == 12               # every ring slot carries its own update
    assert any(k[0] == "epoch" for k in agent.engine()._graphs if isinstance(k, tuple))
    assert agent.training_update_num == 12 and agent.engine().noise_ctr == 12      # one counter per update


def test_whole_epoch_path_declines_with_host_noise():
    agent, nets, col = _train_setup(True, noise="host")
    torch.manual_seed(5)
    col.train_one_epoch()
    state = np.random.get_state()[1].copy()
    assert agent.update_epoch_deferred(4) is None
    assert (np.random.get_state()[1] == state).all() and agent.training_update_num == 0


def test_hard_target_updates_copy_the_value_network():
    """use_soft_update=False: the target stays put between the periods and is the value network at them."""
    agent, nets, col = _train_setup(False, use_soft_update=False, target_hard_update_period=3, noise="host")
    torch.manual_seed(5)
    col.train_one_epoch()
    np.random.seed(9)
    eng = agent.engine()
    t0 = eng.tflat.clone()
    for step in (1, 2, 3):
        info = agent.update(agent._sample())
        assert np.isfinite(list(info.values())).all()
        vf_flat = eng.flat[eng.target_off:]
        assert torch.equal(eng.tflat, vf_flat if step == 3 else t0) and not torch.equal(vf_flat, t0)


@pytest.mark.parametrize("twin", [True, False], ids=["twin", "single"])
def test_trains_through_rlalgo(twin, tmp_path):
    """64 envs, H = 64, B = 256, 3 epochs on SynthVecEnv: finite infos, every network moved, the target is not V, and the
    snapshot carries the reference's names."""
    from torchrl_amd import _C
    agent, nets, col = _train_setup(twin, save_dir=str(tmp_path))
    eager0 = _C.eager_fallback_count()
    before = {name: [p.detach().clone() for p in mod.parameters()] for name, mod in nets.items()}
    moved = lambda ps, qs: [float((p.detach() - q.detach()).abs().max()) > 0 for p, q in zip(ps, qs)]
    agent.train()
    infos = agent.logger.infos
    assert len(infos) == 12 and all(np.isfinite(list(i.values())).all() for i in infos)
    for name, mod in nets.items():
        assert all(moved(mod.parameters(), before[name])), name
    assert any(moved(agent.vf.parameters(), agent.target_vf.parameters()))
    names = ["pf", "qf1", "qf2", "vf"] if twin else ["pf", "qf", "vf"]
    files = sorted(os.listdir(tmp_path))
    assert [f for f in files if f.endswith("_finish.pth")] == sorted("model_%s_finish.pth" % n for n in names)
    state = torch.load(os.path.join(tmp_path, "model_vf_finish.pth"))
    assert all(torch.equal(v.cpu(), agent.vf.state_dict()[k].cpu()) for k, v in state.items())
    assert _C.eager_fallback_count() == eager0                          # nothing left the HIP path


@pytest.mark.parametrize("algo", ["sac", "twin_sac"])
def test_example_scripts_run(tmp_path, algo):
    params = json.load(open(os.path.join(REPO, "config", "%s_synth_halfcheetah.json" % algo)))
    assert "vlr" in params[algo]
    params["net"]["hidden_shapes"] = [64, 64]
    params["replay_buffer"]["size"] = 64 * 64
    params["collector"]["epoch_frames"] = 64 * 8
    params["general_setting"].update(num_epochs=2, batch_size=256, opt_times=3, eval_interval=1, pretrain_epochs=1)
    cfg = tmp_path / ("%s_small.json" % algo)
    cfg.write_text(json.dumps(params))
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "%s_continuous_vec.py" % algo), "--config", str(cfg),
                          "--vec_env_nums", "64", "--seed", "1", "--log_dir", str(tmp_path / "log"), "--overwrite"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "EPOCH:1" in out.stdout
