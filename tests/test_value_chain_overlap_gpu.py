"""Per-step rollouts beside the PPO value chain.

One process runs an epoch's critic and actor updates as two launch sequences on two streams (`_FusedPPO._run_chains`);
the value chain is still stepping the value function, and still reading the ring's observations, returns and old
values, when the next rollout is issued.  `test_two_update_chains_match_the_joint_sequence` (test_product_gpu.py) pins
the fused rollout on that route.  This module pins every rollout that goes through the per-step launch sequence
(`VecOnPolicyCollector._rollout_per_step`) while the update is still the two-chain engine: host Python envs, a running
observation normaliser the persistent kernel does not carry (forced, or a shape without the fused forward), eager and
graph-replayed, PPO and A2C.  Each route is run twice from the same seeds -- TRL_PPO_CHAINS=joint, and two chains with
every value chain held back on the device -- and the two runs must agree bit for bit, epoch by epoch.

The joint runs of three routes are also anchored to the CPU oracle over the first two iterations: each iteration's
oracle starts from the GPU's own state at the start of that iteration (parameters, Adam state, env, normaliser, noise
stream), so a rollout that FOLLOWS an update is compared with the reference too."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, T, HORIZON, MAX_FRAMES, SEED = 32, 8, 6, 4, 5
B = N * T                                         # one minibatch per pass: the parameter bound holds per update
EPOCHS = 6                                        # eager, captured, replayed visits of the chain and rollout graphs

# route -> (env kind, algorithm, noise mode, obs dim, act dim, force_per_step, TRL_NO_GRAPH, replayed rollout graph)
ROUTES = {
    "host_ppo": ("host", "ppo", "host", 17, 6, False, False, False),
    "host_a2c": ("host", "a2c", "host", 17, 6, False, False, False),
    "norm_forced_graph": ("norm", "ppo", "device", 17, 6, True, False, True),
    "norm_forced_eager": ("norm", "ppo", "host", 17, 6, True, False, False),
    "norm_hopper_graph": ("norm", "ppo", "device", 11, 3, False, False, True),
    "norm_hopper_nograph": ("norm", "ppo", "device", 11, 3, False, True, False),
}
ANCHORED = ("host_ppo", "norm_forced_eager", "norm_hopper_graph")
BUF_KEYS = ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits", "old_logp", "advs",
            "estimate_returns")


class _Logger:
    """utils.Logger's deferred protocol: the updates are launched, their info dicts resolved later."""
    def __init__(self):
        self.infos, self.later = [], []

    def add_update_info(self, d):
        self.infos.append(dict(d))

    def add_update_infos_later(self, resolve):
        self.later.append(resolve)

    def add_epoch_info(self, *a, **k):
        pass

    def log(self, *a):
        pass

    def finish(self):
        pass


def _build(route):
    import torchrl.networks as networks
    import torchrl.policies as policies
    from torchrl.algo import A2C, PPO
    from torchrl.collector.on_policy import VecOnPolicyCollector
    from torchrl.env import VecEnv
    from torchrl.env.base_wrapper import NormObs
    from torchrl.env.synth import SynthVecEnv
    from torchrl.replay_buffers.on_policy import OnPolicyReplayBuffer
    from oracle.synth_env import SynthSingleEnvCPU
    kind, algo, noise_mode, D, A, force, _, _ = ROUTES[route]
    dev = torch.device(DEV)
    torch.manual_seed(SEED)
    net = dict(hidden_shapes=[64, 64], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    pf = policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=True, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    if kind == "host":
        # the reference's VecEnv.seed gives env i the seed s * N + i (vecenv.py:63-65); the oracle's vector env keeps the
        # array `step` returned when it resets (see test_host_env_gpu.host_vec_env)
        env = VecEnv(N, [SynthSingleEnvCPU] * N, [(SEED * N + i, HORIZON) for i in range(N)])
        env.alias_reset_obs = False
        eval_env = None
    else:
        env = NormObs(SynthVecEnv(N, obs_dim=D, act_dim=A, horizon=HORIZON, device=dev))
        eval_env = NormObs(SynthVecEnv(N, obs_dim=D, act_dim=A, horizon=HORIZON, device=dev))
        env.seed(SEED)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=dev, train_render=False,
                               epoch_frames=N * T, max_episode_frames=MAX_FRAMES, eval_episodes=1, noise_mode=noise_mode)
    col.force_per_step = force
    logger = _Logger()
    common = dict(plr=3e-4, vlr=3e-4, entropy_coeff=0.005, tau=0.95, shuffle=True, discount=0.99, num_epochs=10,
                  batch_size=B, gae=True, env=col.env, replay_buffer=buf, collector=col, logger=logger, device=dev,
                  save_dir=None)
    if algo == "ppo":
        agent = PPO(pf=pf, vf=vf, clip_para=0.2, opt_epochs=2, **common)
    else:
        agent = A2C(pf=pf, vf=vf, **common)
    return pf, vf, col.env, buf, col, agent, logger


def _gpu_state(pf, vf, env, col, eng):
    """What an iteration starts from, on the host: parameters, Adam state, env, collector counters, normaliser, noise."""
    cpu = lambda x: x.detach().cpu().clone()
    st = {"pf": [cpu(p) for p in pf._mlp2_param_list()], "logstd": cpu(pf.logstd),
          "vf": [cpu(p) for p in vf._mlp2_param_list()], "m": cpu(eng.m), "v": cpu(eng.v), "t": eng.step_count,
          "current_ob": torch.as_tensor(col.current_ob).detach().cpu().numpy().astype(np.float32),
          "cur_obs": env.cur_obs.cpu().numpy(), "cur_step": env.cur_step.cpu().numpy(),
          "ep_return": env.ep_return.cpu().numpy(), "rng": torch.get_rng_state(), "global_step": int(col.global_step)}
    if getattr(env, "is_host_env", False):
        st["episode_idx"] = np.array([e.episode_idx for e in env.venv.envs], dtype=np.int64)
        st["t_env"] = np.array([e.t for e in env.venv.envs], dtype=np.int64)
    else:
        st["episode_idx"] = env.episode_idx.cpu().numpy().astype(np.int64)
        st["t_env"] = env.t_env.cpu().numpy().astype(np.int64)
    nz = getattr(env, "_obs_normalizer", None)
    st["norm"] = None if nz is None else nz.state.cpu().numpy().copy()
    return st


def _oracle_iteration(route, st, epoch):
    """One collect + PPO epoch on the CPU oracle, started from the GPU's state `st`: (ring data, infos, parameters,
    normaliser state or None)."""
    from oracle import philox
    from oracle import replay as oreplay
    from oracle.collector import VecOnPolicyCollectorOracle
    from oracle.normalizer import NormObsOracle
    from oracle.ppo import PPOOracle
    from oracle.synth_env import SynthVecEnvCPU
    kind, _, noise_mode, D, A, _, _, _ = ROUTES[route]
    oenv = SynthVecEnvCPU(N, horizon=HORIZON, obs_dim=D, act_dim=A)
    oenv.seed(SEED)
    env = NormObsOracle(oenv) if st["norm"] is not None else oenv
    ring = oreplay.RingOracle(N * T, env_nums=N, time_limit_filter=True)
    ocol = VecOnPolicyCollectorOracle(env, ring, st["pf"], st["logstd"], st["vf"], epoch_frames=N * T,
                                      max_episode_frames=MAX_FRAMES, discount=0.99)
    # (the constructor reset the env: put the GPU's state in place of what that reset left)
    oenv.episode_idx, oenv.t, oenv._obs = st["episode_idx"].copy(), st["t_env"].copy(), st["cur_obs"].copy()
    if st["norm"] is not None:
        nz = env._obs_normalizer
        nz._mean, nz._var, nz._count = st["norm"][:D].copy(), st["norm"][D:2 * D].copy(), float(st["norm"][2 * D])
    ocol.current_ob = st["current_ob"]
    ocol.current_step = st["cur_step"].astype(np.float64)[:, None]
    ocol.train_rew = st["ep_return"].astype(np.float64)[:, None]
    noise = None
    if noise_mode == "device":
        # the replayed rollout draws its whole (T, N, A) block in one Philox launch keyed (0xC011, global step):
        # element e is normal e & 3 of block e >> 2
        gs, n = st["global_step"], T * N * A
        z = philox.normals4(gs & 0xFFFFFFFF, gs >> 32, np.arange((n + 3) // 4), philox.TAG_NOISE, 0xC011)
        noise = torch.as_tensor(z.reshape(-1)[:n].reshape(T, N, A))
    torch.set_rng_state(st["rng"])
    ocol.train_one_epoch(noise)
    o = PPOOracle(st["pf"], st["logstd"], st["vf"], plr=3e-4, vlr=3e-4, entropy_coeff=0.005, clip_para=0.2, opt_epochs=2,
                  act="tanh", tanh_action=True, discount=0.99, tau=0.95, num_epochs=10, batch_size=B)
    # Adam state of the GPU run: [pf | logstd | vf] in the flat buffers, the shared step count
    off = 0
    for opt, params in ((o.pf_opt, o.pf + [o.logstd]), (o.vf_opt, o.vf)):
        opt.t = st["t"]
        for i, p in enumerate(params):
            k = p.numel()
            opt.m[i], opt.v[i] = st["m"][off:off + k].view(p.shape).clone(), st["v"][off:off + k].view(p.shape).clone()
            off += k
    np.random.seed(SEED + epoch)
    infos = o.epoch(ring, epoch)
    params = torch.cat([p.detach().reshape(-1) for p in o.pf + [o.logstd] + o.vf])
    norm = None if st["norm"] is None else env._obs_normalizer.state()
    return ring, infos, params, norm


def _run(route, chains, monkeypatch, anchor=None):
    kind, algo, noise_mode, D, A, force, no_graph, graph = ROUTES[route]
    monkeypatch.setenv("TRL_PPO_CHAINS", chains)
    monkeypatch.setenv("TRL_NO_GRAPH", "1" if no_graph else "0")
    pf, vf, env, buf, col, agent, logger = _build(route)
    eng = agent.engine()
    assert type(eng).__name__ == "_FusedPPO"
    assert eng.two_chains == (chains == "two")
    if chains == "two":
        # hold every value chain back (device spin): the next rollout is issued, and would run, while the chain is still
        # reading the ring and stepping the value function
        eng._test_value_chain_delay = 5_000_000
    per_step = []
    real = col._rollout_per_step
    monkeypatch.setattr(col, "_rollout_per_step", lambda n: (per_step.append(n), real(n))[1])
    snaps, anchors = [], []
    for epoch in range(EPOCHS):
        st = _gpu_state(pf, vf, env, col, eng) if anchor is not None and epoch < 2 else None
        col.train_one_epoch()
        agent.current_epoch = epoch
        np.random.seed(SEED + epoch)
        agent.update_per_epoch()
        snap = {k: getattr(buf, "_" + k).clone() for k in BUF_KEYS}
        nz = getattr(env, "_obs_normalizer", None)
        if nz is not None:
            snap["norm_state"] = nz.state.clone()
        snaps.append(snap)
        if st is not None:                                  # (a joint run has no overlap: the snapshot disturbs nothing)
            anchors.append((st, eng.flat.clone()))
    # the route really is the per-step one, on the two-chain engine where asked for
    assert per_step == [T] * EPOCHS
    if kind == "host":
        assert col.env.is_host_env
    roll = getattr(col, "_roll_graph", None)
    assert (roll is not None and roll["graph"] is not None) == graph
    if chains == "two" and not no_graph:
        assert len(eng._chain_graphs) > 0
    per_epoch = [[dict(d) for d in resolve()] for resolve in logger.later]   # read in order, after everything was launched
    assert len(per_epoch) == EPOCHS and not logger.infos
    saved = {k: v.cpu() for k, v in vf.state_dict().items()}
    v_now = vf(torch.zeros(3, D, device=DEV))                                # a reader of the value function settles first
    torch.cuda.synchronize()
    assert all(torch.equal(saved[k], v.cpu()) for k, v in vf.state_dict().items())
    n_updates = sum(len(i) for i in per_epoch)
    assert int(eng.red_ws[:2].view(torch.int32)[1].item()) == eng.step_count == n_updates
    if chains == "two":
        assert int(eng.red_ws_v[:2].view(torch.int32)[1].item()) == eng.step_count
    if anchor is not None:
        anchor(anchors, snaps, per_epoch)
    return eng.flat.clone(), eng.m.clone(), eng.v.clone(), per_epoch, snaps, v_now.clone()


def _check_against_oracle(route, errlog):
    from oracle import nets as onets
    D, A = ROUTES[route][3], ROUTES[route][4]

    def check(anchors, snaps, per_epoch):
        assert len(anchors) == 2
        for epoch, (st, flat_after) in enumerate(anchors):
            ring, want_infos, want_params, want_norm = _oracle_iteration(route, st, epoch)
            got = {k: v.cpu().numpy().astype(np.float64) for k, v in snaps[epoch].items()}
            for k in ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits"):
                err = np.abs(got[k] - ring.data[k].reshape(T, N, -1)).max()
                errlog("it%d buffer %s abs" % (epoch, k), err, 1e-5)
                assert err < 1e-5, (epoch, k, err)
            if epoch == 0:
                assert got["terminals"].sum() > 0                    # the over-length bootstrap fired
            # log pi_old of the stored actions under the collecting policy (test_generic_shapes_gpu's bound)
            obs_t = torch.as_tensor(ring.data["obs"], dtype=torch.float32).reshape(T * N, D)
            act_t = torch.as_tensor(ring.data["acts"], dtype=torch.float32).reshape(T * N, A)
            with torch.no_grad():
                lp = onets.policy_update_terms(obs_t, act_t, st["pf"], st["logstd"], "tanh", True)["log_prob"]
            np.testing.assert_allclose(got["old_logp"], lp.reshape(T, N, 1).numpy(), rtol=2e-4, atol=2e-4)
            # advantages and returns: fp32 scan vs fp64 reference, abs 2e-5 / rel 1e-3
            for k in ("advs", "estimate_returns"):
                want = ring.data[k].reshape(T, N, 1)
                errlog("it%d %s: max |got - want| / (2e-5 + 1e-3 |want|)" % (epoch, k),
                       (np.abs(got[k] - want) / (2e-5 + 1e-3 * np.abs(want))).max(), 1.0)
                np.testing.assert_allclose(got[k], want, rtol=1e-3, atol=2e-5)
            if want_norm is not None:
                np.testing.assert_allclose(got["norm_state"], want_norm, rtol=1e-5, atol=1e-6)
            # info scalars: rel 1e-4 / abs 1e-5
            keys = sorted(want_infos[0].keys())
            assert len(per_epoch[epoch]) == len(want_infos) and sorted(per_epoch[epoch][0].keys()) == keys
            gi = np.array([[i[k] for k in keys] for i in per_epoch[epoch]])
            wi = np.array([[i[k] for k in keys] for i in want_infos])
            errlog("it%d info scalars: max |got - want| / (1e-5 + 1e-4 |want|)" % epoch,
                   (np.abs(gi - wi) / (1e-5 + 1e-4 * np.abs(wi))).max(), 1.0)
            bad = np.argwhere(np.abs(gi - wi) > 1e-5 + 1e-4 * np.abs(wi))
            assert len(bad) == 0, [(int(r), keys[c], float(gi[r, c]), float(wi[r, c])) for r, c in bad]
            # parameters after the epoch's updates: abs 1e-6
            perr = (flat_after.cpu() - want_params).abs().max().item()
            errlog("it%d params abs (%d updates)" % (epoch, len(want_infos)), perr, 1e-6)
            assert perr < 1e-6, (epoch, perr)
    return check


@pytest.mark.parametrize("route", list(ROUTES))
def test_per_step_rollout_beside_the_value_chain_matches_the_joint_sequence(route, monkeypatch, errlog):
    """TRL_PPO_CHAINS=joint vs two chains with every value chain held back: the per-step rollout that follows an update
    must not overwrite the ring rows the value chain still reads, nor read a value function it is still stepping --
    same buffers and normaliser state every epoch, same parameters, Adam state, info dicts and value forward at the end.
    The joint runs of the ANCHORED routes are checked against the CPU oracle over their first two iterations."""
    joint = _run(route, "joint", monkeypatch, anchor=_check_against_oracle(route, errlog) if route in ANCHORED else None)
    two = _run(route, "two", monkeypatch)
    (f0, m0, v0, i0, s0, y0), (f1, m1, v1, i1, s1, y1) = joint, two
    diff = [(e, k) for e, (a, b) in enumerate(zip(s0, s1)) for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff
    assert torch.equal(f0, f1) and torch.equal(m0, m1) and torch.equal(v0, v1) and torch.equal(y0, y1)
    assert i0 == i1
