#!/usr/bin/env python
"""Generate tests/golden/gauss_sd_update.npz by running the REFERENCE implementation on the CPU: its own
`GuassianContPolicy` (policies/continuous_policy.py:134-170, the [mean | log_std] head with log_std clamped to [-20, 2]
per sample), `A2C.update` (a2c.py:45-106) and `PPO.update` (ppo.py:41-152) on seeded batches.

Four cases: tanh_action on / off x the shapes (D, A, H, B) = (3, 1, 32, 64) and (17, 6, 64, 96).  The last layer's
log_std bias is overwritten so that the exploration scale is neither tiny nor saturated; in the no-tanh cases the
log_std weight rows are scaled by 30, so some samples sit ON the upper clamp (their log_std gradient is zero).  Stored tanh
actions are clamped to +-0.995: unclamped they reach |a| = 1.0 in fp32, where the reference's log-prob is -inf.  The lower
clamp (-20) is not in the fixture: at sigma = e^-20 the reference's own losses are astronomically large.

    python tests/golden/make_golden_gauss_sd.py            # writes tests/golden/gauss_sd_update.npz
    python tests/golden/make_golden_gauss_sd.py --check    # regenerates into a scratch dir, compares bit for bit

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

NAME = "gauss_sd_update"
# tag: D, A, hidden width, batch size
SHAPES = {"s3": (3, 1, 32, 64), "s17": (17, 6, 64, 96)}
PPO_CLIPV = (False, False, True, False)                                     # four chained PPO.update, one clipped-value


def build(D, A, H, seed, tanh):
    import torchrl.policies as policies
    import torchrl.networks as networks
    torch.manual_seed(seed)
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=tanh, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    last = [m for m in pf.modules() if isinstance(m, torch.nn.Linear)][-1]
    assert last.out_features == 2 * A
    with torch.no_grad():
        if A == 1:
            last.bias[A:] = -1.0
        else:
            last.bias[A:] = torch.linspace(-3.0, -0.5 if tanh else 2.5, A)
        if not tanh:
            last.weight[A:].mul_(30.0)
    return pf, vf


def info_arrays(prefix, info):
    keys = sorted(info.keys())
    return {prefix + "_keys": np.array(keys), prefix + "_vals": np.array([info[k] for k in keys], dtype=np.float64)}


def generate():
    import gym
    from torchrl.algo import A2C
    from oracle.synth_env import SynthVecEnvCPU
    out = {}
    for tanh in (True, False):
        for stag, (D, A, H, B) in SHAPES.items():
            tag = ("t_" if tanh else "n_") + stag
            seed = 5 + D
            rs = np.random.RandomState(100 + D)
            obs = rs.randn(B, D).astype(np.float32)
            eps = rs.randn(B, A).astype(np.float32)
            pf, vf = build(D, A, H, seed, tanh)
            with torch.no_grad():
                mean, std, _ = pf(torch.as_tensor(obs))
                acts = mean + std * torch.as_tensor(eps)
                if tanh:
                    acts = torch.tanh(acts).clamp(-0.995, 0.995)
            batch = {"obs": obs, "acts": acts.numpy().astype(np.float32).copy(),
                     "advs": rs.randn(B, 1).astype(np.float32) * 2 + 0.5,
                     "values": rs.randn(B, 1).astype(np.float32),
                     "estimate_returns": rs.randn(B, 1).astype(np.float32)}
            out.update({f"{tag}_batch_{k}": v for k, v in batch.items()})
            out[f"{tag}_args"] = np.array([D, A, H, B, int(tanh)], dtype=np.int64)
            env = SynthVecEnvCPU(4)
            env.action_space = gym.spaces.Box(-1, 1, (A,))
            common = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, gae=True, env=env, replay_buffer=None,
                          collector=mg._StubCollector(), logger=mg.NullLogger(), device=torch.device("cpu"))

            # ---- the policy's own protocol ----
            out.update(mg.state_arrays(f"{tag}_pf0_", pf))
            out.update(mg.state_arrays(f"{tag}_vf0_", vf))
            with torch.no_grad():
                upd = pf.update(torch.as_tensor(batch["obs"]), torch.as_tensor(batch["acts"]))
                for k in ("mean", "log_std", "log_prob", "ent"):
                    out[f"{tag}_upd_{k}"] = upd[k].numpy().copy()
                out[f"{tag}_eval_act"] = np.asarray(pf.eval_act(torch.as_tensor(batch["obs"]))).astype(np.float32)

            # ---- one A2C.update ----
            agent = A2C(pf=pf, vf=vf, plr=3e-4, vlr=1e-3, entropy_coeff=0.01, batch_size=B,
                        save_dir=tempfile.mkdtemp(prefix="trl_save_"), **common)
            out.update(info_arrays(f"{tag}_a2c_info", agent.update(batch)))
            out.update(mg.state_arrays(f"{tag}_a2c_pf1_", pf))
            out.update(mg.state_arrays(f"{tag}_a2c_vf1_", vf))

            # ---- four chained PPO.update (same initial draw), the third with the clipped value loss ----
            pf, vf = build(D, A, H, seed, tanh)
            agent = mg.make_ppo(pf, vf, env, None, mg._StubCollector(), mg.NullLogger())
            agent.current_epoch = 3
            prs = np.random.RandomState(9)
            with torch.no_grad():                                            # perturb the target: ratio != 1 at step 0
                for p in agent.target_pf.parameters():
                    p.add_(torch.as_tensor(prs.randn(*p.shape).astype(np.float32)) * 0.01)
            out.update(mg.state_arrays(f"{tag}_ppo_tpf0_", agent.target_pf))
            out[f"{tag}_ppo_clipv"] = np.array(PPO_CLIPV, dtype=np.int64)
            for s, clipv in enumerate(PPO_CLIPV):
                agent.clipped_value_loss = clipv
                info = agent.update(batch)
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
