#!/usr/bin/env python
"""Generate tests/golden/layernorm_update.npz by running the REFERENCE implementation on the CPU with `add_ln=True`
networks (networks/base.py:29-41, nets.py:13-52): its own policies' `update` / `eval_act`, `A2C.update` (a2c.py:45-106)
and `PPO.update` (ppo.py:41-152) on seeded batches.

Three cases, one per structural variant of the module list `[Linear, act, LayerNorm] * n` with the last LayerNorm of the
trunk replaced by a second activation, plus `Linear, act, LayerNorm` per appended layer:

    bb_tanh       GuassianContPolicyBasicBias, tanh_action, Tanh, hidden [32, 48]            one LN, tanh(tanh(.)) into the head
    sd_relu_app   GuassianContPolicy, ReLU, hidden [24, 40], append [20]                     two LNs, one feeding the head
    cat_tanh_app  CategoricalDisPolicy (5 actions), Tanh, hidden [17, 33], append [12]       odd widths, double tanh, LN into the head

The value network of a case has the same structure.  Before the first update every LayerNorm's weight is set to
1 + 0.3 randn and its bias to 0.2 randn (seeded), so neither is invisible.  Stored tanh actions are clamped to +-0.995:
unclamped they reach |a| = 1.0 in fp32, where the reference's log-prob is -inf.  For PPO the categorical policy is
subclassed ONLY to add a zero `log_std` entry to the dict `update()` returns, as make_golden_categorical.py does.

    python tests/golden/make_golden_layernorm.py            # writes tests/golden/layernorm_update.npz
    python tests/golden/make_golden_layernorm.py --check    # regenerates into a scratch dir, compares bit for bit

Data only: parameters, batches, policy outputs, info dicts and post-step parameters.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                                     # noqa: E402 -- helpers only

NAME = "layernorm_update"
# tag: head kind, activation, hidden, append, D, A, B, tanh_action, seed
CASES = {
    "bb_tanh": ("bb", "Tanh", [32, 48], [], 11, 3, 64, True, 21),
    "sd_relu_app": ("sd", "ReLU", [24, 40], [20], 17, 6, 96, False, 22),
    "cat_tanh_app": ("cat", "Tanh", [17, 33], [12], 9, 5, 80, False, 23),
}
PPO_CLIPV = (False, False, True, False)                                     # four chained PPO.update, one clipped-value


def perturb_norms(module, seed):
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(torch.as_tensor((1.0 + 0.3 * rs.randn(*m.weight.shape)).astype(np.float32)))
                m.bias.copy_(torch.as_tensor((0.2 * rs.randn(*m.bias.shape)).astype(np.float32)))


def build(tag, with_log_std=False):
    import torchrl.policies as policies
    import torchrl.networks as networks

    class _WithLogStd(policies.CategoricalDisPolicy):
        def update(self, obs, actions):
            out = super().update(obs, actions)
            out["log_std"] = torch.zeros(1)
            return out

    kind, act, hidden, append, D, A, B, tanh, seed = CASES[tag]
    torch.manual_seed(seed)
    net = dict(hidden_shapes=list(hidden), append_hidden_shapes=list(append), base_type=networks.MLPBase,
               activation_func=getattr(torch.nn, act), add_ln=True)
    if kind == "bb":
        pf = policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=tanh, **net)
    elif kind == "sd":
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=tanh, **net)
        last = [m for m in pf.modules() if isinstance(m, torch.nn.Linear)][-1]
        with torch.no_grad():
            last.bias[A:] = torch.linspace(-2.0, -0.5, A)
    else:
        pf = (_WithLogStd if with_log_std else policies.CategoricalDisPolicy)(input_shape=D, output_shape=A, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    perturb_norms(pf, 1000 + seed)
    perturb_norms(vf, 2000 + seed)
    return pf, vf


def info_arrays(prefix, info):
    keys = sorted(info.keys())
    return {prefix + "_keys": np.array(keys), prefix + "_vals": np.array([info[k] for k in keys], dtype=np.float64)}


def generate():
    import gym
    from torchrl.algo import A2C
    from oracle.synth_env import SynthVecEnvCPU
    out = {}
    for tag, (kind, act, hidden, append, D, A, B, tanh, seed) in CASES.items():
        rs = np.random.RandomState(300 + seed)
        obs = rs.randn(B, D).astype(np.float32)
        pf, vf = build(tag)
        n_ln = sum(isinstance(m, torch.nn.LayerNorm) for m in pf.modules())
        assert n_ln == len(hidden) - 1 + len(append), (tag, n_ln)
        if kind == "cat":
            acts = rs.randint(0, A, size=(B,)).astype(np.float32)
        else:
            eps = rs.randn(B, A).astype(np.float32)
            with torch.no_grad():
                mean, std, _ = pf(torch.as_tensor(obs))
                a = mean + std * torch.as_tensor(eps)
                if tanh:
                    a = torch.tanh(a).clamp(-0.995, 0.995)
            acts = a.numpy().astype(np.float32).copy()
        batch = {"obs": obs, "acts": acts,
                 "advs": rs.randn(B, 1).astype(np.float32) * 2 + 0.5,
                 "values": rs.randn(B, 1).astype(np.float32),
                 "estimate_returns": rs.randn(B, 1).astype(np.float32)}
        out.update({f"{tag}_batch_{k}": v for k, v in batch.items()})
        out[f"{tag}_args"] = np.array([D, A, B, int(tanh)], dtype=np.int64)
        env = SynthVecEnvCPU(4)
        env.action_space = gym.spaces.Discrete(A) if kind == "cat" else gym.spaces.Box(-1, 1, (A,))
        common = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, gae=True, env=env, replay_buffer=None,
                      collector=mg._StubCollector(), logger=mg.NullLogger(), device=torch.device("cpu"))

        # ---- the policy's own protocol ----
        out.update(mg.state_arrays(f"{tag}_pf0_", pf))
        out.update(mg.state_arrays(f"{tag}_vf0_", vf))
        with torch.no_grad():
            upd = pf.update(torch.as_tensor(batch["obs"]), torch.as_tensor(batch["acts"]))
            for k in (("log_prob", "ent") if kind == "cat" else ("mean", "log_std", "log_prob", "ent")):
                out[f"{tag}_upd_{k}"] = upd[k].numpy().copy()
            if kind == "cat":
                out[f"{tag}_probs"] = pf(torch.as_tensor(batch["obs"])).numpy().copy()
                out[f"{tag}_eval_act"] = np.asarray(pf.eval_act(torch.as_tensor(batch["obs"]))).astype(np.int64)
            else:
                out[f"{tag}_eval_act"] = np.asarray(pf.eval_act(torch.as_tensor(batch["obs"]))).astype(np.float32)
            out[f"{tag}_v0"] = vf(torch.as_tensor(batch["obs"])).numpy().copy()

        # ---- one A2C.update ----
        agent = A2C(pf=pf, vf=vf, plr=3e-4, vlr=1e-3, entropy_coeff=0.01, batch_size=B,
                    save_dir=tempfile.mkdtemp(prefix="trl_save_"), **common)
        info = agent.update(batch)
        assert all(np.isfinite(v) for v in info.values()), (tag, info)
        out.update(info_arrays(f"{tag}_a2c_info", info))
        out.update(mg.state_arrays(f"{tag}_a2c_pf1_", pf))
        out.update(mg.state_arrays(f"{tag}_a2c_vf1_", vf))

        # ---- four chained PPO.update (same initial draw), the third with the clipped value loss ----
        pf, vf = build(tag, with_log_std=True)
        agent = mg.make_ppo(pf, vf, env, None, mg._StubCollector(), mg.NullLogger())
        agent.current_epoch = 3
        prs = np.random.RandomState(9)
        with torch.no_grad():                                                # perturb the target: ratio != 1 at step 0
            for p in agent.target_pf.parameters():
                p.add_(torch.as_tensor(prs.randn(*p.shape).astype(np.float32)) * 0.01)
        out.update(mg.state_arrays(f"{tag}_ppo_tpf0_", agent.target_pf))
        out[f"{tag}_ppo_clipv"] = np.array(PPO_CLIPV, dtype=np.int64)
        for s, clipv in enumerate(PPO_CLIPV):
            agent.clipped_value_loss = clipv
            info = agent.update(batch)
            if kind == "cat":                                                # (the zero entry's statistics: std of one value is NaN)
                info = {k: v for k, v in info.items() if not k.startswith("log_std/")}
            assert all(np.isfinite(v) for v in info.values()), (tag, s, info)
            out.update(info_arrays(f"{tag}_ppo_info{s}", info))
            out.update(mg.state_arrays(f"{tag}_ppo_pf{s + 1}_", pf))
            out.update(mg.state_arrays(f"{tag}_ppo_vf{s + 1}_", vf))
    return out


def main():
    mg.install_stubs()
    arrays = generate()
    check = "--check" in sys.argv[1:]
    path = os.path.join(tempfile.mkdtemp(prefix="trl_golden_check_") if check else HERE, NAME + ".npz")
    np.savez_compressed(path, meta=np.array(mg.META), **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")
    if check:
        new, old = np.load(path), np.load(os.path.join(HERE, NAME + ".npz"))
        same = sorted(new.files) == sorted(old.files) and all(
            new[k].shape == old[k].shape and np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f")
            for k in new.files if k != "meta")
        print("%-24s %s" % (NAME + ".npz", "identical" if same else "DIFFERS"))
        sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
