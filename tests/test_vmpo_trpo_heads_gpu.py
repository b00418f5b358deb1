"""V-MPO and TRPO with a categorical and with a state-dependent-std policy, built from the public classes, against what the
REFERENCE's VMPO.update / TRPO.update / update_vf produced for the same parameters and batches
(tests/golden/vmpo_trpo_heads.npz, tests/golden/make_golden_vmpo_trpo_heads.py): info dicts with their NaN positions, eta /
alpha, the parameters after every chained update, the line search's accepted backtrack index and its acceptance ratios;
then three epochs of train() on the device envs.  Bounds: those of tests/test_vmpo_gpu.py and tests/test_trpo_gpu.py for the
same quantities.  Every test here fails on a build without the head kernels (TRPO / VMPO refused both policies)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TAGS = ["s4", "s17"]


class _Stub:
    epoch_frames = 0


class _Log:
    def __init__(self): self.infos, self.epochs = [], []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): self.epochs.append(a)
    def log(self, *a): pass
    def finish(self): pass


def _nets(g, pre, kind, D, A, H, tanh):
    import torchrl.networks as networks
    import torchrl.policies as policies
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    if kind == "cat":
        pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
    else:
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=tanh, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    for prefix, mod in ((pre + "_pf0_", pf), (pre + "_vf0_", vf)):
        mod.load_state_dict({k[len(prefix):].replace("__", "."): torch.tensor(g[k]) for k in g.files if k.startswith(prefix)})
    return pf, vf


def _env(kind, D, A):
    from torchrl.env import get_vec_env
    from torchrl.env.synth import SynthVecEnv
    if kind == "cat":                                                          # (only its action space is read here)
        return get_vec_env("SynthCheetahDiscrete-v0", {"reward_scale": 1, "obs_norm": False}, 4, device=DEV)
    return SynthVecEnv(4, obs_dim=D, act_dim=A, device=DEV)


def _state_err(mod, g, prefix):
    return max(np.abs(p.cpu().numpy() - g[prefix + name.replace(".", "__")]).max() for name, p in mod.state_dict().items())


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kind", ["cat", "sd"])
def test_vmpo_update_matches_reference(golden, kind, tag):
    from torchrl.algo import VMPO
    g = golden("vmpo_trpo_heads")
    pre = f"vmpo_{kind}_{tag}"
    D, A, H, B, tanh = (int(v) for v in g[pre + "_args"])
    pf, vf = _nets(g, pre, kind, D, A, H, bool(tanh))
    agent = VMPO(pf=pf, vf=vf, plr=1e-3, vlr=1e-3, opt_epochs=2, eta_eps=0.02, alpha_eps=0.1, tau=0.95, shuffle=True,
                 discount=0.99, num_epochs=10, batch_size=B, gae=True, env=_env(kind, D, A), replay_buffer=None,
                 collector=_Stub(), logger=_Log(), device=DEV, save_dir=None)
    agent.engine().sync_target_pf()
    for s in range(4):
        batch = {k: g[f"{pre}_s{s}_batch_{k}"] for k in ("obs", "acts", "advs", "values", "estimate_returns")}
        if kind == "cat":
            assert batch["acts"].shape == (B,)
        info = agent.update(batch)
        keys = [str(k) for k in g[f"{pre}_s{s}_info_keys"]]
        assert sorted(info.keys()) == keys
        got, want = np.array([info[k] for k in keys], dtype=np.float64), g[f"{pre}_s{s}_info_vals"]
        print(pre, s, "max info err", np.nanmax(np.abs(got - want) / (2e-5 + 2e-4 * np.abs(want))))
        assert np.array_equal(np.isnan(got), np.isnan(want))                   # KL/std of the categorical policy's summed KL
        np.testing.assert_allclose(got, want, rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose([agent.eta.item(), agent.alpha.item()], g[f"{pre}_s{s}_eta_alpha"], rtol=2e-6)
        err = _state_err(pf, g, f"{pre}_pf{s + 1}_")
        print(pre, s, "pf err", err)
        assert err < 3e-6, (s, err)
    assert _state_err(vf, g, f"{pre}_vf4_") < 3e-6
    assert agent.training_update_num == 4


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kind", ["cat", "sd"])
def test_trpo_update_matches_reference(golden, kind, tag):
    from torchrl.algo import TRPO
    g = golden("vmpo_trpo_heads")
    pre = f"trpo_{kind}_{tag}"
    D, A, H, B, tanh = (int(v) for v in g[pre + "_args"])
    pf, vf = _nets(g, pre, kind, D, A, H, bool(tanh))
    agent = TRPO(pf=pf, vf=vf, plr=3e-4, vlr=1e-3, max_kl=0.01, cg_damping=0.1, cg_iters=10, residual_tol=1e-10,
                 entropy_coeff=0.01, shuffle=True, v_opt_times=2, tau=0.95, discount=0.99, num_epochs=10, batch_size=64,
                 gae=True, env=_env(kind, D, A), replay_buffer=None, collector=_Stub(), logger=_Log(), device=DEV,
                 save_dir=None)
    batch = {k: g[f"{pre}_batch_{k}"] for k in ("obs", "acts", "advs", "estimate_returns")}
    info = agent.update(batch)
    keys = [str(k) for k in g[pre + "_info_keys"]]
    assert sorted(info.keys()) == keys
    np.testing.assert_allclose([info[k] for k in keys], g[pre + "_info_vals"], rtol=2e-4, atol=2e-5)
    # ---- the line search: the same trials, the same decision ----
    search = agent.engine().search
    accepted = len(search) - 1 if search[-1] is not None else -1
    ratios = np.array([t[1] for t in search if t is not None])
    print(pre, "accepted", accepted, "ratios", ratios, "reference", g[pre + "_search_ratio"])
    assert accepted == int(g[pre + "_accepted"])
    np.testing.assert_allclose(ratios, g[pre + "_search_ratio"], rtol=2e-3)    # (every ratio is >= 0.02 away from 0.1)
    err = _state_err(pf, g, pre + "_pf1_")
    print(pre, "pf err", err)
    assert err < 1e-4, err                                                     # tests/test_trpo_gpu.py: the first step's bound
    if kind == "cat":                                                          # the same update from (B, 1) actions
        pf2, vf2 = _nets(g, pre, kind, D, A, H, False)
        agent2 = TRPO(pf=pf2, vf=vf2, plr=3e-4, vlr=1e-3, max_kl=0.01, cg_damping=0.1, cg_iters=10, residual_tol=1e-10,
                      entropy_coeff=0.01, shuffle=True, v_opt_times=2, tau=0.95, discount=0.99, num_epochs=10, batch_size=64,
                      gae=True, env=_env(kind, D, A), replay_buffer=None, collector=_Stub(), logger=_Log(), device=DEV,
                      save_dir=None)
        info2 = agent2.update(dict(batch, acts=batch["acts"].reshape(-1, 1)))
        assert info2 == info and all(torch.equal(p, q) for p, q in zip(pf.parameters(), pf2.parameters()))
    for s in range(2):
        vinfo = agent.update_vf(batch)
        np.testing.assert_allclose([vinfo[k] for k in sorted(vinfo)], g[f"{pre}_vinfo{s}_vals"], rtol=2e-4, atol=2e-5)
        assert _state_err(vf, g, f"{pre}_vf{s + 1}_") < 3e-6


# ---------------------------------------------------------------- train() on the device envs
def _train(kind, algo):
    import torchrl.networks as networks
    import torchrl.policies as policies
    from torchrl.algo import TRPO, VMPO
    from torchrl.collector.on_policy import VecOnPolicyCollector
    from torchrl.env import get_vec_env
    from torchrl.replay_buffers.on_policy import OnPolicyReplayBuffer
    N, T = 8, 16
    name = "SynthCheetahDiscrete-v0" if kind == "cat" else "SynthHalfCheetah-v0"
    env, eval_env = (get_vec_env(name, {"reward_scale": 1, "obs_norm": False}, N, device=DEV) for _ in range(2))
    env.seed(5)
    eval_env.seed(6)
    torch.manual_seed(0)
    np.random.seed(0)
    D = env.observation_space.shape[0]
    net = dict(hidden_shapes=[64, 64], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    if kind == "cat":
        pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=env.action_space.n, **net)
    else:
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * env.action_space.shape[0], tanh_action=algo == "vmpo", **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=DEV, train_render=False,
                               epoch_frames=N * T, max_episode_frames=9, eval_episodes=1, noise_mode="device")
    logger = _Log()
    general = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=3, eval_interval=1, batch_size=N * 4, gae=True,
                   env=col.env, replay_buffer=buf, collector=col, logger=logger, device=DEV, save_dir=None)
    if algo == "trpo":
        agent = TRPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, max_kl=0.01, cg_damping=0.1, cg_iters=10, residual_tol=1e-10,
                     entropy_coeff=0.01, v_opt_times=2, **general)
    else:
        agent = VMPO(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, opt_epochs=2, **general)
    return agent, pf, vf, logger, T


@pytest.mark.parametrize("algo", ["trpo", "vmpo"])
@pytest.mark.parametrize("kind", ["cat", "sd"])
def test_three_epochs_of_train(kind, algo):
    agent, pf, vf, logger, T = _train(kind, algo)
    p0 = torch.cat([p.detach().reshape(-1) for p in pf.parameters()]).clone()
    agent.train()
    updates_per_epoch = (1 + 2 * (T // 4)) if algo == "trpo" else 2 * (T // 4)
    assert len(logger.infos) == 3 * updates_per_epoch and len(logger.epochs) == 3
    for net in (pf, vf):
        assert all(torch.isfinite(p).all() for p in net.parameters())
    moved = (torch.cat([p.detach().reshape(-1) for p in pf.parameters()]) - p0).abs().max().item()
    assert 0 < moved < 1.0
    skip = {"KL/std"} if (kind == "cat" and algo == "vmpo") else set()
    for i in logger.infos:
        assert all(np.isfinite(v) for k, v in i.items() if k not in skip)
        assert all(np.isnan(i[k]) for k in skip if k in i)
