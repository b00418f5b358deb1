"""What the tests of `add_ln=True` networks on the off-policy engines share (tests/test_layernorm_offpolicy_*.py): the
fixture tests/golden/layernorm_offpolicy*.npz read back as one mapping, the repo's networks and agents of a fixture case,
and the comparison of an agent's state with the fixture -- test infrastructure, no test of its own.

Fixture keys of case `tag` (tests/golden/make_golden_layernorm_offpolicy.py):
    <tag>_args                 JSON: algo, act, hidden, append, D, A, B, pf_ln, q_ln, w_reg, clip, seed, steps, quantiles, nets,
                               targets, noise
    <tag>_batch_<key>          obs, next_obs, acts, rewards, terminals -- one batch for all four updates
    <tag>_s<s>_<noise>         the N(0, 1) draws of update s, (B, A) each, in draw order (`noise` of the args)
    <tag>_info<s>_keys/_vals   the info dict after update s = 0 .. 3
    <tag>_<net><i>_<name>      state dicts (torch's names, "." as "__") of every trained network and target before the first
                               update (i = 0) and after update i - 1 (i = 1 .. 4)
    <tag>_log_alpha<i>         i = 1 .. 4, soft actor-critics only
"""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAME = "layernorm_offpolicy"
PARTS = ("", "_sacq", "_sacv")
TAGS = ["sacq_relu", "sacq_tanh_app", "sacv", "twinsacv", "ddpg_tanh", "td3_relu_app", "dqn_relu", "qrdqn_tanh", "critic_only_ln"]
PARAM_BOUND, INFO_REL, INFO_ABS = 1e-6, 1e-4, 1e-5
BATCH_KEYS = ("obs", "next_obs", "acts", "rewards", "terminals")


class Stub:
    epoch_frames = 0


class Log:
    def __init__(self): self.infos = []
    def add_update_info(self, d): self.infos.append(dict(d))
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


def load_fixture():
    """{key: array} over the fixture's files, and its meta dict."""
    g = {}
    for part in PARTS:
        with np.load(os.path.join(HERE, "golden", NAME + part + ".npz"), allow_pickle=False) as f:
            g.update({k: f[k] for k in f.files})
    return g, json.loads(str(g["meta"]))


def args_of(g, tag):
    return json.loads(str(g[tag + "_args"]))


def state_of(g, prefix):
    return {k[len(prefix):].replace("__", "."): torch.from_numpy(np.array(g[k])) for k in g if k.startswith(prefix)}


def batch_of(g, tag):
    return {k: g[f"{tag}_batch_{k}"] for k in BATCH_KEYS}


def info_of(g, tag, s):
    return dict(zip((str(k) for k in g[f"{tag}_info{s}_keys"]), (float(x) for x in g[f"{tag}_info{s}_vals"])))


def build_nets(a, pf_ln=None, q_ln=None):
    """{name: module} of the repo's trained networks for the args `a` of a case (add_ln as stored, or overridden)."""
    from torchrl_amd import networks, policies
    pf_ln, q_ln = (a["pf_ln"] if pf_ln is None else pf_ln), (a["q_ln"] if q_ln is None else q_ln)
    D, A, algo = a["D"], a["A"], a["algo"]
    net = lambda ln: dict(hidden_shapes=list(a["hidden"]), append_hidden_shapes=list(a["append"]), base_type=networks.MLPBase,
                          activation_func=getattr(torch.nn, a["act"]), **({"add_ln": True} if ln else {}))
    nets = {}
    if algo in ("DQN", "QRDQN"):
        nets["qf"] = networks.Net(input_shape=(D,), output_shape=A * (a["quantiles"] if algo == "QRDQN" else 1), **net(q_ln))
        return nets
    if algo in ("DDPG", "TD3"):
        nets["pf"] = policies.FixGuassianContPolicy(input_shape=D, output_shape=A, tanh_action=True, norm_std_explore=0.1, **net(pf_ln))
    else:
        nets["pf"] = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net(pf_ln))
    for name in a["nets"][1:]:
        if name == "vf":
            nets[name] = networks.Net(input_shape=D, output_shape=1, **net(q_ln))
        else:
            nets[name] = networks.QNet(input_shape=D + A, output_shape=1, **net(q_ln))
    return nets


def build_agent(g, tag, device, nets=None, **over):
    """(agent, {name: trained network}, [(fixture name, target network)]) of case `tag` at its stored initial state."""
    from torchrl_amd import algo as algos
    from torchrl_amd.env.synth import SynthVecEnv
    from torchrl_amd.policies import EpsilonGreedyDQNDiscretePolicy
    a = args_of(g, tag)
    if nets is None:
        nets = build_nets(a)
        for name, mod in nets.items():
            mod.load_state_dict(state_of(g, f"{tag}_{name}0_"))
    dev = torch.device(device)
    kw = dict(replay_buffer=None, collector=Stub(), logger=Log(), discount=0.99, num_epochs=10, batch_size=a["B"], device=dev,
              save_dir=None, tau=0.005, use_soft_update=True, opt_times=1)
    name = a["algo"]
    if name in ("DQN", "QRDQN"):
        class Env:
            action_space = type("Discrete", (), {"n": a["A"]})()
        pf = EpsilonGreedyDQNDiscretePolicy(qf=nets["qf"], start_epsilon=0.25, end_epsilon=0.25, decay_frames=10, action_shape=a["A"])
        kw.update(qf=nets["qf"], pf=pf, qlr=1e-3, env=Env())
        kw.update(over)
        agent = algos.QRDQN(quantile_num=a["quantiles"], **kw) if name == "QRDQN" else algos.DQN(**kw)
        return agent, nets, [("tqf", agent.target_qf)]
    kw.update(env=SynthVecEnv(4, obs_dim=a["D"], act_dim=a["A"], device=dev), grad_clip=a["clip"] if a["clip"] else None,
              plr=3e-4, qlr=1e-3, **nets)
    if name in ("TwinSACQ", "SAC", "TwinSAC"):
        kw.update(policy_std_reg_weight=a["w_reg"], policy_mean_reg_weight=a["w_reg"], reparameterization=True,
                  automatic_entropy_tuning=True)
        if name != "TwinSACQ":
            kw.update(vlr=1e-3)
        kw.update(over)
        agent = getattr(algos, name)(**kw)
        if name == "TwinSACQ":
            return agent, nets, [("tqf1", agent.target_qf1), ("tqf2", agent.target_qf2)]
        return agent, nets, [("tvf", agent.target_vf)]
    if name == "DDPG":
        kw.update(over)
        agent = algos.DDPG(**kw)
        return agent, nets, [("tpf", agent.target_pf), ("tqf", agent.target_qf)]
    kw.update(over)
    agent = algos.TD3(policy_update_delay=2, norm_std_policy=0.2, noise_clip=0.5, **kw)
    return agent, nets, [("tpf", agent.target_pf), ("tqf1", agent.target_qf1), ("tqf2", agent.target_qf2)]


def param_error(mod, g, prefix):
    """max |parameter - fixture| over the state dict `prefix`, every key (gamma / beta included)."""
    sd = mod.state_dict()
    want = state_of(g, prefix)
    assert sorted(sd) == sorted(want), (prefix, sorted(sd), sorted(want))
    return max(float((p.detach().cpu().double() - want[k].double()).abs().max()) for k, p in sd.items())


def info_errors(info, want):
    """{key: |got - want| / (abs + rel |want|)} -- at most 1 within the bound."""
    assert sorted(info) == sorted(want), (sorted(info), sorted(want))
    return {k: abs(float(info[k]) - want[k]) / (INFO_ABS + INFO_REL * abs(want[k])) for k in want}
