#!/usr/bin/env python
"""Generate tests/golden/layernorm_offpolicy*.npz by running the REFERENCE implementation's off-policy algorithms on the
CPU with `add_ln=True` networks (networks/base.py:29-41, nets.py:13-52): its own `TwinSACQ`, `SAC`, `TwinSAC`, `DDPG`,
`TD3`, `DQN` and `QRDQN` classes, four chained `update` calls each on one seeded batch.

    tag             algorithm  nets
    sacq_relu       TwinSACQ   ReLU, hidden [32, 48], D 11, A 3, B 64; policy and critics add_ln
    sacq_tanh_app   TwinSACQ   Tanh, hidden [24, 40] + append [20], D 9, A 2, B 80 (double tanh and a norm into the head);
                               regularisers 1e-3, grad_clip 1
    sacv            SAC        ReLU, hidden [32, 48], D 11, A 3, B 64; regularisers 1e-3, grad_clip 1
    twinsacv        TwinSAC    the same nets, no regularisers, no clip
    ddpg_tanh       DDPG       Tanh, hidden [32, 48], D 11, A 3, B 64; FixGuassianContPolicy, tanh_action, grad_clip 0.5
    td3_relu_app    TD3        ReLU, hidden [24, 40] + append [20], D 9, A 2, B 80; tanh_action, policy_update_delay 2 (updates
                               1 and 3 step the policy), exploration and smoothing noise
    dqn_relu        DQN        ReLU, hidden [32, 48] MLPBase, D 6, 4 actions, B 64
    qrdqn_tanh      QR-DQN     Tanh, the same trunk, 8 quantiles
    critic_only_ln  TwinSACQ   the nets of sacq_relu with add_ln on the critics only

Before the first update every LayerNorm's weight is set to 1 + 0.3 N(0, 1) and its bias to 0.2 N(0, 1)
(make_golden_layernorm.perturb_norms), so neither is invisible.  Stored per case: the batch, the N(0, 1) draws of every
update in draw order, the info dict after every update, and every state dict -- trained networks AND targets -- before
the first update (index 0) and after each of the four (1 .. 4), `log_alpha` for the soft actor-critics.

Why this runs under `python -O`: see make_golden_sac_v.py (sac.py:130 / twin_sac.py:142 assert a tensor comparison).  Started
without -O the script starts itself again as a fresh child process with -O.

The reference's own error.  Every case is run a second time with torch.set_default_dtype(torch.float64): the same float32
draw of the networks cast up, the same stored batch and the same stored N(0, 1) draws (handed to
torch.distributions.Normal.sample in draw order), every later operation in float64.  `meta["distance"][tag]` records the
largest float32-vs-float64 distance over all four updates as a fraction of the bound the fixture's consumers hold the
kernels to -- post-step parameters abs 1e-6 (log_alpha with them), info scalars rel 1e-4 / abs 1e-5.  A case is kept only
if both fractions are at most 0.25; otherwise the network seed -- the one thing a case leaves open -- moves on by 1000,
and `meta["rejected"]` records the seeds passed over with their fractions.

Three files, because no file in this repository may exceed 1 MiB (fp32 parameters do not compress):
layernorm_offpolicy.npz (meta, the list of cases, the deterministic-policy and Q-learning cases),
layernorm_offpolicy_sacq.npz (the three TwinSACQ cases), layernorm_offpolicy_sacv.npz (SAC, TwinSAC).
tests/_layernorm_offpolicy.py::load_fixture reads them back as one mapping.

    python tests/golden/make_golden_layernorm_offpolicy.py            # writes tests/golden/layernorm_offpolicy*.npz
    python tests/golden/make_golden_layernorm_offpolicy.py --check    # regenerates into a scratch dir, compares bit for bit

Data only: parameters, batches, noise draws, info dicts.
"""
import copy
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                                     # noqa: E402 -- helpers only
import make_golden_layernorm as mgl                                          # noqa: E402 -- perturb_norms, info_arrays

NAME = "layernorm_offpolicy"
STEPS, QUANTILES = 4, 8
PARAM_BOUND, INFO_REL, INFO_ABS, KEEP = 1e-6, 1e-4, 1e-5, 0.25
DRAWS = 12
# tag: algorithm, activation, hidden, append, D, A, B, add_ln of the policy, of the critics, regulariser weight, grad_clip (0: none), seed
CASES = {
    "sacq_relu": ("TwinSACQ", "ReLU", [32, 48], [], 11, 3, 64, True, True, 0.0, 0.0, 51),
    "sacq_tanh_app": ("TwinSACQ", "Tanh", [24, 40], [20], 9, 2, 80, True, True, 1e-3, 1.0, 52),
    "sacv": ("SAC", "ReLU", [32, 48], [], 11, 3, 64, True, True, 1e-3, 1.0, 53),
    "twinsacv": ("TwinSAC", "ReLU", [32, 48], [], 11, 3, 64, True, True, 0.0, 0.0, 54),
    "ddpg_tanh": ("DDPG", "Tanh", [32, 48], [], 11, 3, 64, True, True, 0.0, 0.5, 55),
    "td3_relu_app": ("TD3", "ReLU", [24, 40], [20], 9, 2, 80, True, True, 0.0, 0.0, 56),
    "dqn_relu": ("DQN", "ReLU", [32, 48], [], 6, 4, 64, True, True, 0.0, 0.0, 57),
    "qrdqn_tanh": ("QRDQN", "Tanh", [32, 48], [], 6, 4, 64, True, True, 0.0, 0.0, 58),
    "critic_only_ln": ("TwinSACQ", "ReLU", [32, 48], [], 11, 3, 64, False, True, 0.0, 0.0, 59),
}
FILES = {"sacq": ("sacq_relu", "sacq_tanh_app", "critic_only_ln"), "sacv": ("sacv", "twinsacv")}   # the rest: NAME.npz
NOISE = {"TwinSACQ": ("eps1", "eps2"), "SAC": ("eps1",), "TwinSAC": ("eps1",), "DDPG": (), "TD3": ("eps_explore", "eps_smooth"),
         "DQN": (), "QRDQN": ()}


def build(tag, seed):
    """{name: module} of the trained networks of a case, drawn in float32 under `seed`, the norms perturbed."""
    import torchrl.policies as policies
    import torchrl.networks as networks
    algo, act, hidden, append, D, A, B, pf_ln, q_ln, w_reg, clip, _ = CASES[tag]
    torch.manual_seed(seed)
    net = lambda ln: dict(hidden_shapes=list(hidden), append_hidden_shapes=list(append), base_type=networks.MLPBase,
                          activation_func=getattr(torch.nn, act), **({"add_ln": True} if ln else {}))
    nets = {}
    if algo in ("DQN", "QRDQN"):
        nets["qf"] = networks.Net(input_shape=(D,), output_shape=A * (QUANTILES if algo == "QRDQN" else 1), **net(q_ln))
    else:
        if algo in ("DDPG", "TD3"):
            nets["pf"] = policies.FixGuassianContPolicy(input_shape=D, output_shape=A, tanh_action=True, norm_std_explore=0.1,
                                                        **net(pf_ln))
        else:
            nets["pf"] = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net(pf_ln))
        for name in {"TwinSACQ": ("qf1", "qf2"), "SAC": ("qf",), "TwinSAC": ("qf1", "qf2"), "DDPG": ("qf",),
                     "TD3": ("qf1", "qf2")}[algo]:
            nets[name] = networks.QNet(input_shape=D + A, output_shape=1, **net(q_ln))
        if algo in ("SAC", "TwinSAC"):
            nets["vf"] = networks.Net(input_shape=D, output_shape=1, **net(q_ln))
    for k, (name, mod) in enumerate(nets.items()):
        mgl.perturb_norms(mod, 1000 * (k + 1) + seed)
    return nets


def batch_of(tag):
    algo, act, hidden, append, D, A, B = CASES[tag][:7]
    rs = np.random.RandomState(800 + CASES[tag][-1])
    f = np.float32
    batch = {"obs": rs.randn(B, D).astype(f), "next_obs": rs.randn(B, D).astype(f)}
    if algo in ("DQN", "QRDQN"):
        batch["acts"] = rs.randint(0, A, size=(B, 1) if algo == "DQN" else (B,)).astype(f)
    else:
        batch["acts"] = np.tanh(rs.randn(B, A)).astype(f)
    batch["rewards"], batch["terminals"] = rs.randn(B, 1).astype(f), (rs.rand(B, 1) < 0.2).astype(f)
    return batch


def make_agent(tag, nets):
    """The reference's agent over `nets` and [(name, target module)] of its targets."""
    import gym
    import torchrl.algo as algos
    from torchrl.algo.off_policy.dqn import DQN
    from torchrl.algo.off_policy.qrdqn import QRDQN
    from oracle.synth_env import SynthVecEnvCPU
    algo, act, hidden, append, D, A, B, pf_ln, q_ln, w_reg, clip, _ = CASES[tag]
    kw = dict(replay_buffer=None, collector=mg._StubCollector(), logger=mg.NullLogger(), discount=0.99, num_epochs=10,
              batch_size=B, device=torch.device("cpu"), save_dir=tempfile.mkdtemp(prefix="trl_save_"), tau=0.005,
              use_soft_update=True, opt_times=1)
    if algo in ("DQN", "QRDQN"):
        class Env:
            action_space = gym.spaces.Discrete(A)

        class Pf:
            epsilon = 0.25
        kw.update(qf=nets["qf"], pf=Pf(), qlr=1e-3, env=Env())
        agent = QRDQN(quantile_num=QUANTILES, **kw) if algo == "QRDQN" else DQN(**kw)
        return agent, [("tqf", agent.target_qf)]
    env = SynthVecEnvCPU(4)
    env.action_space = gym.spaces.Box(-1, 1, (A,))
    kw.update(env=env, grad_clip=clip if clip else None, plr=3e-4, qlr=1e-3, **nets)
    if algo in ("TwinSACQ", "SAC", "TwinSAC"):
        kw.update(policy_std_reg_weight=w_reg, policy_mean_reg_weight=w_reg, reparameterization=True,
                  automatic_entropy_tuning=True)
        if algo != "TwinSACQ":
            kw.update(vlr=1e-3)
        agent = getattr(algos, algo)(**kw)
        if algo == "TwinSACQ":
            return agent, [("tqf1", agent.target_qf1), ("tqf2", agent.target_qf2)]
        return agent, [("tvf", agent.target_vf)]
    if algo == "DDPG":
        agent = algos.DDPG(**kw)
        return agent, [("tpf", agent.target_pf), ("tqf", agent.target_qf)]
    agent = algos.TD3(policy_update_delay=2, norm_std_policy=0.2, noise_clip=0.5, **kw)
    return agent, [("tpf", agent.target_pf), ("tqf1", agent.target_qf1), ("tqf2", agent.target_qf2)]


def run(tag, seed, noise=None):
    """The four updates of a case.  noise None: the reference's float32 run, drawing from its own CPU stream (the draws
    are recovered by replaying the generator state and stored).  noise = [[draws of update s]]: the float64 run on them.
    Returns {key: array}."""
    from torch.distributions import Normal
    algo, B, A = CASES[tag][0], CASES[tag][6], CASES[tag][5]
    nets = build(tag, seed)
    double = noise is not None
    out = {}
    if double:
        torch.set_default_dtype(torch.float64)
        for mod in nets.values():
            mod.double()
    try:
        agent, targets = make_agent(tag, nets)
        batch = batch_of(tag)
        if not double:
            out.update({f"{tag}_batch_{k}": v for k, v in batch.items()})
            out[f"{tag}_args"] = np.array(json.dumps(dict(zip(
                ("algo", "act", "hidden", "append", "D", "A", "B", "pf_ln", "q_ln", "w_reg", "clip", "base_seed"), CASES[tag]),
                seed=seed, steps=STEPS, quantiles=QUANTILES, nets=list(nets), targets=[n for n, _ in targets], noise=NOISE[algo])))
        for name, mod in list(nets.items()) + targets:
            out.update(mg.state_arrays(f"{tag}_{name}0_", mod))
        for s in range(STEPS):
            if double:
                queue = [torch.as_tensor(d).double() for d in noise[s]]
                real = Normal.sample
                Normal.sample = lambda self, sample_shape=torch.Size(): self.loc + self.scale * queue.pop(0)
                try:
                    info = agent.update(batch)
                finally:
                    Normal.sample = real
                if queue:
                    raise RuntimeError("%s: the float64 run drew %d tensors fewer than stored" % (tag, len(queue)))
            else:
                torch.manual_seed(100 + s)
                state = torch.get_rng_state()
                info = agent.update(batch)
                after = torch.get_rng_state()
                torch.set_rng_state(state)
                for k in NOISE[algo]:
                    out[f"{tag}_s{s}_{k}"] = torch.randn(B, A).numpy()
                if not torch.equal(torch.get_rng_state(), after):            # (no assert: they are compiled out here)
                    raise RuntimeError("%s: noise stream mismatch" % tag)
            info = {k: float(v) for k, v in info.items()}
            if not all(np.isfinite(v) for v in info.values()):
                raise RuntimeError("%s update %d: %s" % (tag, s, info))
            out.update(mgl.info_arrays(f"{tag}_info{s}", info))
            for name, mod in list(nets.items()) + targets:
                out.update(mg.state_arrays(f"{tag}_{name}{s + 1}_", mod))
            if hasattr(agent, "log_alpha"):
                out[f"{tag}_log_alpha{s + 1}"] = agent.log_alpha.detach().numpy().copy()
    finally:
        torch.set_default_dtype(torch.float32)
    return out


def distance(tag, a32, a64):
    """(parameters, info): the largest float32-vs-float64 distance of a case, as fractions of the consumers' bounds."""
    par = inf = 0.0
    for k, v in a32.items():
        if k.endswith("_keys") or "_batch_" in k or k.endswith("_args") or k[len(tag) + 1:len(tag) + 3] in ("s0", "s1", "s2", "s3"):
            continue
        w = a64[k].astype(np.float64)
        if k.endswith("_vals"):
            inf = max(inf, float((np.abs(v - w) / (INFO_ABS + INFO_REL * np.abs(w))).max()))
        else:
            par = max(par, float(np.abs(v.astype(np.float64) - w).max()) / PARAM_BOUND)
    return par, inf


def generate():
    arrays, dist, rejected = {}, {}, {}
    for tag in CASES:
        base = CASES[tag][-1]
        for attempt in range(DRAWS):
            seed = base + 1000 * attempt
            a32 = run(tag, seed)
            noise = [[a32[f"{tag}_s{s}_{k}"] for k in NOISE[CASES[tag][0]]] for s in range(STEPS)]
            par, inf = distance(tag, a32, run(tag, seed, noise))
            print("%-15s seed %5d: float32 vs float64 parameters %.3f, info %.3f of the bound" % (tag, seed, par, inf))
            if par <= KEEP and inf <= KEEP:
                arrays.update(a32)
                dist[tag] = {"seed": seed, "params": par, "info": inf}
                break
            rejected.setdefault(tag, {})[str(seed)] = {"params": par, "info": inf}
        else:
            raise RuntimeError("no draw of %s stays within a quarter of the bounds in %d draws" % (tag, DRAWS))
    return arrays, dist, rejected


def split(arrays, meta):
    files = {NAME + ".npz": {"meta": np.array(meta), "cases": np.array(list(CASES))}}
    where = {tag: NAME + "_%s.npz" % f for f, tags in FILES.items() for tag in tags}
    for tag in CASES:
        files.setdefault(where.get(tag, NAME + ".npz"), {}).update({k: v for k, v in arrays.items() if k.startswith(tag + "_")})
    if sum(len(f) for f in files.values()) != len(arrays) + 2:
        raise RuntimeError("an array belongs to no case")
    return files


def main():
    if sys.flags.optimize == 0:                                              # see the docstring: a fresh child with -O
        sys.exit(subprocess.call([sys.executable, "-O", os.path.abspath(__file__)] + sys.argv[1:]))
    mg.install_stubs()
    arrays, dist, rejected = generate()
    meta = dict(json.loads(mg.META), optimize=int(sys.flags.optimize), distance=dist, rejected=rejected,
                bounds={"params_abs": PARAM_BOUND, "info_rel": INFO_REL, "info_abs": INFO_ABS, "keep_fraction": KEEP})
    check = "--check" in sys.argv[1:]
    out_dir = tempfile.mkdtemp(prefix="trl_golden_check_") if check else HERE
    same = True
    for fname, part in split(arrays, json.dumps(meta)).items():
        path = os.path.join(out_dir, fname)
        np.savez_compressed(path, **part)
        print("wrote", path, os.path.getsize(path), "bytes")
        if check:
            new, old = np.load(path), np.load(os.path.join(HERE, fname))
            ok = sorted(new.files) == sorted(old.files) and all(
                new[k].shape == old[k].shape and np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f")
                for k in new.files if k != "meta")
            print("%-36s %s" % (fname, "identical" if ok else "DIFFERS"))
            same = same and ok
    if check:
        sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
