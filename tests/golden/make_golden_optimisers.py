#!/usr/bin/env python
"""Generate tests/golden/optimisers_{onpolicy,dqn,qrdqn,detac}.npz (four files: none may pass 1 MiB) by running the REFERENCE
implementation on the CPU with optimisers other than Adam: its own `A2C.update`, `PPO.update`, `DQN.update`, `QRDQN.update`,
`DDPG.update` and `TD3.update`, four chained calls each on one seeded batch of B = 64.

  a2c_cat / ppo_cat   RMSprop (the constructor's eps = 1e-5), CategoricalDisPolicy (D 4, A 3, H 32)
  a2c_g / ppo_g       RMSprop, GuassianContPolicyBasicBias (17, 6, 64) -- the shape with a fused Adam-only engine
  dqn_* / qrdqn_*     MLP Q-net (D 4, A 2, H 32; QR-DQN with 8 quantiles): RMSprop defaults (`rms`), RMSprop(alpha=0.95,
                      eps=0.01, centered=True, momentum=0.95) (`rmsc`), SGD(momentum=0.9, nesterov=True) (`sgdn`), each with
                      soft (`_soft`) and hard (`_hard`, period 2) target updates
  ddpg_* / td3_*      (D 5, A 2, H 32), TD3 with policy_update_delay = 2: RMSprop defaults (`rms`), SGD(momentum=0.9) (`sgdm`)

Recorded per case: the batch, the initial parameters, and after EACH update its info dict (sorted keys), the parameters, the
target networks and every optimiser state tensor under torch's own name (the two 17-64-64 cases: the state after the fourth
update only, the file's size).

Conditioning (make_golden_reinforce.py's rule, for the same reason: with torch's default eps = 1e-8 an RMSprop step is
lr g / (sqrt(sq) + eps), whose sensitivity to g reaches lr / eps where |g| is of the size of eps): every draw is run FOUR
times, three of them with the 64 batch rows (and TD3's noise rows) in another order -- the same mathematics, other float32
sums -- and the network seed is redrawn, at most 50 times, until the reference's runs agree within SPREAD = 1e-7 on the
parameters after all four updates.  Only the run in the stored order is recorded; the condition is evaluated on the
reference's runs alone.

The on-policy cases also record `<tag>_ref_f32_err`: how far the reference's float32 run is from its own float64 run in the
optimiser state (`reference_error`), which is what a test's bound on that state is derived from.

    python tests/golden/make_golden_optimisers.py            # writes the four files
    python tests/golden/make_golden_optimisers.py --check    # regenerates into a scratch dir, compares bit for bit

Data only: batches, parameters, info dicts, optimiser state, settings.
"""
import functools
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                                     # noqa: E402 -- helpers only
import make_golden_categorical as mgc                                        # noqa: E402 -- the categorical nets

B, STEPS, SPREAD, DRAWS = 64, 4, 1e-7, 50
OPTS = {"rms": ("RMSprop", {}), "rmsc": ("RMSprop", dict(alpha=0.95, eps=0.01, centered=True, momentum=0.95)),
        "sgdn": ("SGD", dict(momentum=0.9, nesterov=True)), "sgdm": ("SGD", dict(momentum=0.9))}
STATE_NAMES = ("square_avg", "momentum_buffer", "grad_avg")
ON_POLICY = {"a2c_cat": ("A2C", "cat", 4, 3, 32), "ppo_cat": ("PPO", "cat", 4, 3, 32),
             "a2c_g": ("A2C", "g", 17, 6, 64), "ppo_g": ("PPO", "g", 17, 6, 64)}
DQN_CASES = {"%s_%s_%s" % (a, o, t): (a, o, t == "soft") for a in ("dqn", "qrdqn") for o in ("rms", "rmsc", "sgdn")
             for t in ("soft", "hard")}
DETAC_CASES = {"%s_%s" % (a, o): (a, o) for a in ("ddpg", "td3") for o in ("rms", "sgdm")}
QUANTILES = 8
# small steps: the spread of a default RMSprop (eps = 1e-8) under a reordered batch scales with the learning rate
DQN_LR, PLR, QLR = 2.5e-4, 1e-4, 2e-4
# A2C / PPO: RMSprop's first step moves every parameter by lr / sqrt(1 - alpha) = 10 lr whatever its gradient; at 3e-5 that is
# the 3e-4 an Adam(lr=3e-4) first step moves it (at 3e-4 four updates on one batch take PPO's ratio/max past 1e4)
ON_LR = 3e-5
# stored actions of the tanh-Gaussian policy: |a| <= 0.5, where atanh(a) and log(1 - a^2) are benign in float32 (at 0.98,
# 1 - |a| alone carries a relative rounding of 2^-24 / 0.02 = 3e-6 into every log-prob)
ACT_SCALE = 0.5


def common():
    return dict(replay_buffer=None, collector=mg._StubCollector(), logger=mg.NullLogger(), discount=0.99, num_epochs=10,
                batch_size=B, device=torch.device("cpu"), save_dir=tempfile.mkdtemp(prefix="trl_save_"))


def permuted(batch, order):
    return batch if order is None else {k: np.ascontiguousarray(v[order]) for k, v in batch.items()}


FINAL_KEYS = set()                                                           # parameter keys after the last update


def start(out, tag, batch, nets, opt):
    """The batch, the settings and the initial parameters `<tag>_<net>0_*` of nets = [(name, module)]."""
    out.update({f"{tag}_batch_{k}": v for k, v in batch.items()})
    out[f"{tag}_opt"] = np.array(json.dumps({"cls": OPTS[opt][0], "kw": OPTS[opt][1]}))
    for name, mod in nets:
        out.update(mg.state_arrays(f"{tag}_{name}0_", mod))


def snapshot(out, tag, s, info, nets, targets, optimizers, with_state=True):
    """After update s (1-based): its info dict `<tag>_info<s-1>`, the parameters `<tag>_<net><s>_*` of nets and targets and,
    with_state, every optimiser state tensor `<tag>_state<s>_<net>_<torch's name>_<parameter>`."""
    # (log_std/ of a categorical PPO is the reference wrapper's one-element placeholder: its std is NaN, no test reads it)
    assert all(np.isfinite(float(v)) for k, v in info.items() if not k.startswith("log_std/")), (tag, s, info)
    out.update(mgc.info_arrays(f"{tag}_info{s - 1}", {k: float(v) for k, v in info.items()}))
    for name, mod in list(nets) + list(targets):
        arrays = mg.state_arrays(f"{tag}_{name}{s}_", mod)
        out.update(arrays)
        if s == STEPS:
            FINAL_KEYS.update(arrays)
    if with_state:
        for name, optimizer, mod in optimizers:
            for pn, p in mod.named_parameters():
                for sn in STATE_NAMES:
                    st = optimizer.state[p].get(sn)
                    if st is not None:
                        out[f"{tag}_state{s}_{name}_{sn}_{pn.replace('.', '__')}"] = st.detach().numpy().copy()


def run_on_policy(tag, seed, order=None, double=False):
    """double: the same float32 draw of the networks and the same batch, every later operation in float64 -- what the
    reference's own float32 run is measured against (`reference_error`)."""
    import gym
    from torchrl.algo import A2C
    from oracle.synth_env import SynthVecEnvCPU
    algo, head, D, A, H = ON_POLICY[tag]
    out = {f"{tag}_args": np.array([D, A, H, B, seed], dtype=np.int64)}
    rs = np.random.RandomState(500 + D)
    batch = {"obs": rs.randn(B, D).astype(np.float32),
             "acts": rs.randint(0, A, size=(B,)).astype(np.float32) if head == "cat"
             else (np.tanh(rs.randn(B, A)) * ACT_SCALE).astype(np.float32),
             "advs": rs.randn(B, 1).astype(np.float32) * 2 + 0.5, "values": rs.randn(B, 1).astype(np.float32),
             "estimate_returns": rs.randn(B, 1).astype(np.float32)}
    batch = permuted(batch, order)
    pf, vf = mgc.build(D, A, H, seed, algo == "PPO") if head == "cat" else mg.build_nets(D, A, H, seed)
    env = SynthVecEnvCPU(4)
    env.action_space = gym.spaces.Discrete(A) if head == "cat" else gym.spaces.Box(-1, 1, (A,))
    if double:
        torch.set_default_dtype(torch.float64)
        pf.double(), vf.double()
    try:
        return _run_on_policy(out, tag, algo, head, pf, vf, env, batch)
    finally:
        torch.set_default_dtype(torch.float32)


def _run_on_policy(out, tag, algo, head, pf, vf, env, batch):
    from torchrl.algo import A2C
    start(out, tag, batch, [("pf", pf), ("vf", vf)], "rms")
    if algo == "A2C":
        agent = A2C(pf=pf, vf=vf, plr=ON_LR, vlr=ON_LR, entropy_coeff=0.01, env=env, tau=0.95, shuffle=True, gae=True,
                    optimizer_class=torch.optim.RMSprop, **common())
    else:
        agent = mg.make_ppo(pf, vf, env, None, mg._StubCollector(), mg.NullLogger(), batch_size=B, plr=ON_LR, vlr=ON_LR,
                            optimizer_class=torch.optim.RMSprop)
        agent.current_epoch = 3
        prs = np.random.RandomState(9)
        with torch.no_grad():                                                # perturb the target: ratio != 1 at step 0
            for p in agent.target_pf.parameters():
                p.add_((torch.as_tensor(prs.randn(*p.shape).astype(np.float32)) * 0.01).to(p.dtype))
        out.update(mg.state_arrays(f"{tag}_tpf0_", agent.target_pf))
    g = agent.pf_optimizer.param_groups[0]
    assert type(agent.pf_optimizer) is torch.optim.RMSprop and g["eps"] == 1e-5 and g["alpha"] == 0.99
    for s in range(1, STEPS + 1):                                            # (the 17-64-64 nets: state after the last update
        snapshot(out, tag, s, agent.update(batch), [("pf", pf), ("vf", vf)], [],   # only, the file's size)
                 [("pf", agent.pf_optimizer, pf), ("vf", agent.vf_optimizer, vf)], with_state=head == "cat" or s == STEPS)
    return out


def run_dqn(tag, seed, order=None):
    import gym
    import torchrl.networks as networks
    from torchrl.algo.off_policy.dqn import DQN
    from torchrl.algo.off_policy.qrdqn import QRDQN
    algo, opt, soft = DQN_CASES[tag]
    D, A, H, Q = 4, 2, 32, (QUANTILES if algo == "qrdqn" else 1)
    out = {f"{tag}_args": np.array([D, A, H, B, Q, int(soft), seed], dtype=np.int64)}

    class Env:
        action_space = gym.spaces.Discrete(A)

    class Pf:
        epsilon = 0.25
    rs = np.random.RandomState(600 + Q)
    batch = {"obs": rs.randn(B, D).astype(np.float32), "next_obs": rs.randn(B, D).astype(np.float32),
             "acts": rs.randint(0, A, size=(B, 1) if Q == 1 else (B,)).astype(np.float32),
             "rewards": rs.randn(B, 1).astype(np.float32), "terminals": (rs.rand(B, 1) < 0.2).astype(np.float32)}
    batch = permuted(batch, order)
    torch.manual_seed(seed)
    qf = networks.Net(output_shape=A * Q, base_type=networks.MLPBase, append_hidden_shapes=[], hidden_shapes=[H, H],
                      activation_func=torch.nn.ReLU, input_shape=(D,))
    start(out, tag, batch, [("qf", qf)], opt)
    kw = dict(common(), qf=qf, pf=Pf(), qlr=DQN_LR, env=Env(), tau=0.005, use_soft_update=soft, target_hard_update_period=2,
              opt_times=1, optimizer_class=getattr(torch.optim, OPTS[opt][0]), optimizer_info=dict(OPTS[opt][1]))
    agent = QRDQN(quantile_num=Q, **kw) if Q > 1 else DQN(**kw)
    for s in range(1, STEPS + 1):
        snapshot(out, tag, s, agent.update(batch), [("qf", qf)], [("tqf", agent.target_qf)], [("qf", agent.qf_optimizer, qf)])
    return out


def run_detac(tag, seed, order=None, noise=None):
    """noise: the stored-order run's N(0, 1) draws per update, handed to a permuted run in ITS row order."""
    import gym
    import torchrl.policies as policies
    import torchrl.networks as networks
    from torch.distributions import Normal
    from torchrl.algo import DDPG, TD3
    from oracle.synth_env import SynthVecEnvCPU
    algo, opt = DETAC_CASES[tag]
    D, A, H = 5, 2, 32
    out = {f"{tag}_args": np.array([D, A, H, B, seed], dtype=np.int64)}
    rs = np.random.RandomState(700)
    batch = {"obs": rs.randn(B, D).astype(np.float32), "next_obs": rs.randn(B, D).astype(np.float32),
             "acts": np.tanh(rs.randn(B, A)).astype(np.float32), "rewards": rs.randn(B, 1).astype(np.float32),
             "terminals": (rs.rand(B, 1) < 0.1).astype(np.float32)}
    batch = permuted(batch, order)
    torch.manual_seed(seed)
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.ReLU)
    pf = policies.FixGuassianContPolicy(input_shape=D, output_shape=A, tanh_action=True, norm_std_explore=0.1, **net)
    qf1 = networks.QNet(input_shape=D + A, output_shape=1, **net)
    qf2 = networks.QNet(input_shape=D + A, output_shape=1, **net)
    env = SynthVecEnvCPU(4)
    env.action_space = gym.spaces.Box(-1, 1, (A,))
    cls = functools.partial(getattr(torch.optim, OPTS[opt][0]), **OPTS[opt][1])
    kw = dict(common(), env=env, grad_clip=0.5, tau=0.005, use_soft_update=True, opt_times=1, optimizer_class=cls)
    if algo == "ddpg":
        agent = DDPG(pf=pf, qf=qf1, plr=PLR, qlr=QLR, **kw)
        nets, targets = [("pf", pf), ("qf1", qf1)], [("tpf", agent.target_pf), ("tqf1", agent.target_qf)]
        opts = [("pf", agent.pf_optimizer, pf), ("qf1", agent.qf_optimizer, qf1)]
    else:
        agent = TD3(pf=pf, qf1=qf1, qf2=qf2, plr=PLR, qlr=QLR, policy_update_delay=2, norm_std_policy=0.2,
                    noise_clip=0.5, **kw)
        nets = [("pf", pf), ("qf1", qf1), ("qf2", qf2)]
        targets = [("tpf", agent.target_pf), ("tqf1", agent.target_qf1), ("tqf2", agent.target_qf2)]
        opts = [("pf", agent.pf_optimizer, pf), ("qf1", agent.qf1_optimizer, qf1), ("qf2", agent.qf2_optimizer, qf2)]
    start(out, tag, batch, nets, opt)
    drawn = []
    for s in range(STEPS):
        if noise is None:
            torch.manual_seed(200 + s)
            state = torch.get_rng_state()
            info = agent.update(batch)
            after = torch.get_rng_state()
            if algo == "td3":                                                # explore noise of target_pf, then the smoothing noise
                torch.set_rng_state(state)
                drawn.append((torch.randn(B, A), torch.randn(B, A)))
                assert torch.equal(torch.get_rng_state(), after), "noise stream mismatch"
                out[f"{tag}_s{s}_eps_explore"], out[f"{tag}_s{s}_eps_smooth"] = (d.numpy() for d in drawn[-1])
        else:
            queue = [torch.as_tensor(np.ascontiguousarray(d.numpy()[order])) for d in noise[s]] if algo == "td3" else []
            real = Normal.sample
            Normal.sample = lambda self, sample_shape=torch.Size(): self.loc + self.scale * queue.pop(0)
            try:
                info = agent.update(batch)
            finally:
                Normal.sample = real
            assert not queue
        snapshot(out, tag, s + 1, info, nets, targets, opts)
    return out, drawn


def conditioned(tag, run, base):
    """The arrays of the first draw of `tag` whose four runs agree within SPREAD on the parameters after all updates."""
    orders = [np.random.RandomState(7 + k).permutation(B) for k in range(3)]
    final = lambda arrays: {k: v for k, v in arrays.items() if k in FINAL_KEYS}
    for attempt in range(DRAWS):
        seed = base + 1000 * attempt
        res = run(tag, seed)
        arrays, noise = res if isinstance(res, tuple) else (res, None)
        others = []
        for order in orders:
            r = run(tag, seed, order, noise) if noise is not None else run(tag, seed, order)
            others.append(r[0] if isinstance(r, tuple) else r)
        want = final(arrays)
        assert want
        spread = max(float(np.abs(want[k] - final(o)[k]).max()) for o in others for k in want)
        if spread <= SPREAD:
            print("%-18s network seed %d (draw %d), parameters under a reordered batch within %.3e"
                  % (tag, seed, attempt + 1, spread))
            arrays[f"{tag}_spread"] = np.array([spread, SPREAD])
            return arrays
    raise AssertionError("no draw of %s meets the conditioning requirement in %d draws" % (tag, DRAWS))


def reference_error(tag, arrays):
    """The reference's OWN float32 error in the optimiser state, measured on its runs alone: its float32 run (`arrays`)
    against `run_on_policy(double=True)`, per network the largest |float32 - float64| of a recorded state tensor in units of
    1e-6 x (scale of the state tensor) / (scale of the parameter tensor) -- the units of the parameters' bound of abs 1e-6.
    A test that holds a float32 kernel against the float32 fixture allows 1 + 2 x this: either run is that far from the
    exact value."""
    exact = run_on_policy(tag, int(arrays[f"{tag}_args"][-1]), double=True)
    units = {"pf": 0.0, "vf": 0.0}
    for k, got in arrays.items():
        if k.startswith(f"{tag}_state"):
            step, name, rest = k[len(tag) + 6:].split("_", 2)
            pn = rest.split("_", 2)[2]                                       # (torch's state names are two words)
            want = exact[k]
            p_scale = float(np.abs(exact[f"{tag}_{name}{step}_{pn}"]).max())
            units[name] = max(units[name], float(np.abs(got - want).max()) / (1e-6 * float(np.abs(want).max()) / p_scale))
    print("%-18s the reference's own float32 error in the state: policy %.2f, critic %.2f (units of the 1e-6 bound)"
          % (tag, units["pf"], units["vf"]))
    return np.array([units["pf"], units["vf"]])


FILES = {"optimisers_onpolicy": (ON_POLICY, run_on_policy, 11), "optimisers_dqn": (None, run_dqn, 31),
         "optimisers_qrdqn": (None, run_dqn, 37), "optimisers_detac": (DETAC_CASES, run_detac, 61)}


def generate(name):
    tags, run, base = FILES[name]
    if tags is None:
        tags = [t for t in DQN_CASES if t.startswith(name[len("optimisers_"):] + "_")]
    out = {}
    for k, tag in enumerate(tags):
        arrays = conditioned(tag, run, base + k)
        if run is run_on_policy:
            arrays[f"{tag}_ref_f32_err"] = reference_error(tag, arrays)
        out.update(arrays)
    return out


def main():
    mg.install_stubs()
    check, ok = "--check" in sys.argv[1:], True
    for name in FILES:
        arrays = generate(name)
        path = os.path.join(tempfile.mkdtemp(prefix="trl_golden_check_") if check else HERE, name + ".npz")
        np.savez_compressed(path, meta=np.array(mg.META), **arrays)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20), "over the 1 MiB limit for a committed file"
        if check:
            new, old = np.load(path), np.load(os.path.join(HERE, name + ".npz"))
            same = sorted(new.files) == sorted(old.files) and all(
                new[k].shape == old[k].shape and np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f")
                for k in new.files if k != "meta")
            print("%-24s %s" % (name + ".npz", "identical" if same else "DIFFERS"))
            ok = ok and same
    if check:
        sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
