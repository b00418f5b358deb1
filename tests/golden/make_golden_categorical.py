#!/usr/bin/env python
"""Generate tests/golden/categorical_update.npz by running the REFERENCE implementation on the CPU: its own
`CategoricalDisPolicy` (policies/discrete_policies.py:124-168), `A2C.update` (a2c.py:45-106, the discrete branch) and
`PPO.update` (ppo.py:41-152) on seeded batches whose `acts` have shape (B,), as the reference needs.

For PPO the reference policy is subclassed ONLY to add a zero `log_std` entry to the dict `update()` returns
(`PPO.update_actor` reads that key for its log and never differentiates it); nothing else is touched.

    python tests/golden/make_golden_categorical.py            # writes tests/golden/categorical_update.npz
    python tests/golden/make_golden_categorical.py --check    # regenerates into a scratch dir, compares bit for bit

Data only: parameters, batches, info dicts and post-step parameters.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                                     # noqa: E402 -- helpers only

NAME = "categorical_update"
# tag: D, A, hidden width, batch size
SHAPES = {"s4": (4, 2, 32, 64), "s17": (17, 6, 64, 96)}
PPO_CLIPV = (False, False, True, False)                                     # four chained PPO.update, one clipped-value


def build(D, A, H, seed, with_log_std):
    import torchrl.policies as policies
    import torchrl.networks as networks

    class _WithLogStd(policies.CategoricalDisPolicy):
        def update(self, obs, actions):
            out = super().update(obs, actions)
            out["log_std"] = torch.zeros(1)
            return out

    torch.manual_seed(seed)
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    cls = _WithLogStd if with_log_std else policies.CategoricalDisPolicy
    pf = cls(input_shape=D, output_shape=A, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    return pf, vf


def info_arrays(prefix, info):
    keys = sorted(info.keys())
    return {prefix + "_keys": np.array(keys), prefix + "_vals": np.array([info[k] for k in keys], dtype=np.float64)}


def generate():
    import gym
    from torchrl.algo import A2C
    from oracle.synth_env import SynthVecEnvCPU
    out = {}
    for tag, (D, A, H, B) in SHAPES.items():
        seed = 5 + D
        rs = np.random.RandomState(100 + D)
        batch = {"obs": rs.randn(B, D).astype(np.float32),
                 "acts": rs.randint(0, A, size=(B,)).astype(np.float32),
                 "advs": rs.randn(B, 1).astype(np.float32) * 2 + 0.5,
                 "values": rs.randn(B, 1).astype(np.float32),
                 "estimate_returns": rs.randn(B, 1).astype(np.float32)}
        out.update({f"{tag}_batch_{k}": v for k, v in batch.items()})
        out[f"{tag}_args"] = np.array([D, A, H, B], dtype=np.int64)
        env = SynthVecEnvCPU(4)
        env.action_space = gym.spaces.Discrete(A)
        common = dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, gae=True, env=env, replay_buffer=None,
                      collector=mg._StubCollector(), logger=mg.NullLogger(), device=torch.device("cpu"))

        # ---- the policy's own protocol ----
        pf, vf = build(D, A, H, seed, False)
        out.update(mg.state_arrays(f"{tag}_pf0_", pf))
        out.update(mg.state_arrays(f"{tag}_vf0_", vf))
        with torch.no_grad():
            upd = pf.update(torch.as_tensor(batch["obs"]), torch.as_tensor(batch["acts"]))
            out[f"{tag}_upd_log_prob"] = upd["log_prob"].numpy().copy()
            out[f"{tag}_upd_ent"] = upd["ent"].numpy().copy()
            out[f"{tag}_probs"] = pf(torch.as_tensor(batch["obs"])).numpy().copy()
            out[f"{tag}_eval_act"] = np.asarray(pf.eval_act(torch.as_tensor(batch["obs"]))).astype(np.int64)

        # ---- one A2C.update ----
        agent = A2C(pf=pf, vf=vf, plr=3e-4, vlr=1e-3, entropy_coeff=0.01, batch_size=B,
                    save_dir=tempfile.mkdtemp(prefix="trl_save_"), **common)
        out.update(info_arrays(f"{tag}_a2c_info", agent.update(batch)))
        out.update(mg.state_arrays(f"{tag}_a2c_pf1_", pf))
        out.update(mg.state_arrays(f"{tag}_a2c_vf1_", vf))

        # ---- four chained PPO.update (same initial draw), the third with the clipped value loss ----
        pf, vf = build(D, A, H, seed, True)
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
            out.update(info_arrays(f"{tag}_ppo_info{s}", agent.update(batch)))
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
