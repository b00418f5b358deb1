#!/usr/bin/env python
"""Generate tests/golden/boot_dqn_update.npz by running the REFERENCE implementation on the CPU: its own
`BootstrappedDQN` (algo/off_policy/bootstrapped_dqn.py:7-104), `BootstrappedNet` (networks/nets.py:71-121) and
`BootstrappedDQNDiscretePolicy` (policies/discrete_policies.py:92-121), all UNMODIFIED.

How the unmodified classes are made to run.  `BootstrappedNet.__init__` cannot be called as written: its trunk call reads
`add_ln=add_ln` followed by `**kwargs` on the next line, which parses as the power `add_ln ** kwargs`.  So this script
passes `base_type=functools.partial(MLPBase, input_shape=..., hidden_shapes=...)`, no extra keyword arguments (kwargs is
then `{}`), and for `add_ln` a falsy stand-in object whose `__pow__` returns False: the trunk gets `add_ln=False`, and the
later `if self.add_ln` tests see a falsy value.  With that the class constructs; `BootstrappedDQN.update` runs with `acts`
of shape (B,), `rewards` / `terminals` of shape (B, 1) and `masks` of shape (B, K) and returns its two info keys
(`Reward_Mean`, `Training/qf_loss`); the policy's `explore` / `eval_act` work on (1, D) inputs (they call `.item()`).
The reference's `sample_key` names "actions" while `update` reads `batch['acts']`; `update` is called directly here.

Three cases, each two chained updates, D = 17, A = 3, K = 4, trunk 32 x 32 ReLU, B = 48, a fifth of the terminals set,
Bernoulli(0.5) masks, qlr = 1e-3, discount 0.99, tau = 0.005:

    lin    append_hidden_shapes []     soft target update
    hid    append_hidden_shapes [16]   soft target update
    hard   append_hidden_shapes []     use_soft_update=False, target_hard_update_period=2

Conditioning (the rule of make_golden_sac_v.py).  Adam's step is ill-conditioned where a gradient entry lies near its
eps; there the reference's own fp32 rounding decides the step.  The initialisation seed -- the one thing the cases leave
open -- is the first from 31 on at which all final parameters (online and target) of the reference's fp32 run lie within
1e-6 of the same updates carried out in float64 by tests/_boot_dqn_ref.py; `meta` records the seed taken and the seeds
rejected with their errors.

Stored per case (data only): initial and final state dicts of the online and the target network, the batches, the info
keys and values of every update, per head `qf(obs, range(K))` on the first batch (initial parameters), and the
`explore` / `eval_act` actions of the initial network for eight single observations under each head.

    python tests/golden/make_golden_boot_dqn.py            # writes tests/golden/boot_dqn_update.npz
    python tests/golden/make_golden_boot_dqn.py --check    # regenerates into a scratch dir, compares bit for bit
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

NAME = "boot_dqn_update"
D, A, K, H, B, STEPS, P = 17, 3, 4, 32, 48, 2, 0.5
QLR, TAU = 1e-3, 0.005
SEED0, REF_ERR_MAX = 31, 1e-6
# tag: append_hidden_shapes, use_soft_update, target_hard_update_period
CASES = {"lin": ([], True, 1000), "hid": ([16], True, 1000), "hard": ([], False, 2)}
BATCH_KEYS = ("obs", "next_obs", "acts", "rewards", "terminals", "masks")


class _FalsyLn:
    """Stands in for `add_ln=False`: falsy, and `add_ln ** kwargs` (what the reference's trunk call parses as) is False."""
    def __bool__(self): return False
    def __pow__(self, other): return False


def reference_error(arrays):
    """The reference's OWN rounding error in the stored final parameters: their largest distance from the same two
    updates carried out in float64 (tests/_boot_dqn_ref.py, explicit chain rule)."""
    sys.path.insert(0, os.path.dirname(HERE))
    import _boot_dqn_ref as ref
    worst = 0.0
    for tag in CASES:
        up, k, steps = ref.update_from_fixture(arrays, tag)
        for s in range(steps):
            up.update({key: arrays[f"{tag}_s{s}_batch_{key}"] for key in BATCH_KEYS})
        for mine, name in ((up.net, "qf1"), (up.tnet, "tqf1")):
            want = ref.net_of(arrays, f"{tag}_{name}_", k)
            for pair, pair_ref in zip(mine[0] + [wb for h in mine[1] for wb in h], want[0] + [wb for h in want[1] for wb in h]):
                worst = max([worst] + [float(np.abs(x - y).max()) for x, y in zip(pair, pair_ref)])
    return worst


def generate_conditioned():
    rejected = {}
    for seed in range(SEED0, SEED0 + 16):
        arrays = generate(seed)
        err = reference_error(arrays)
        print("init seed %d: the reference's fp32 parameters are within %.3g of the float64 update" % (seed, err))
        if err < REF_ERR_MAX:
            return arrays, seed, rejected
        rejected[str(seed)] = err
    raise RuntimeError("no init seed in [%d, %d) gives a well-conditioned fixture" % (SEED0, SEED0 + 16))


def generate(seed):
    import gym
    import torchrl.networks as networks
    import torchrl.policies as policies
    from torchrl.algo.off_policy.bootstrapped_dqn import BootstrappedDQN
    out = {}

    class Env:
        action_space = gym.spaces.Discrete(A)
    for tag, (append, soft, period) in CASES.items():
        torch.manual_seed(seed)
        qf = networks.BootstrappedNet(output_shape=A, head_num=K, append_hidden_shapes=append, add_ln=_FalsyLn(),
                                      activation_func=torch.nn.ReLU,
                                      base_type=functools.partial(networks.MLPBase, input_shape=D, hidden_shapes=[H, H]))
        pf = policies.BootstrappedDQNDiscretePolicy(qf=qf, head_num=K, action_shape=A)
        agent = BootstrappedDQN(head_num=K, bernoulli_p=P, qf=qf, pf=pf, qlr=QLR, env=Env(), replay_buffer=None,
                                collector=mg._StubCollector(), logger=mg.NullLogger(), discount=0.99, num_epochs=10,
                                batch_size=B, device=torch.device("cpu"), save_dir=tempfile.mkdtemp(prefix="trl_save_"),
                                tau=TAU, use_soft_update=soft, target_hard_update_period=period, opt_times=1)
        out.update(mg.state_arrays(f"{tag}_qf0_", qf))
        out.update(mg.state_arrays(f"{tag}_tqf0_", agent.target_qf))
        out[f"{tag}_args"] = np.array([K, B, int(soft), period, STEPS, QLR, TAU, len(append)], dtype=np.float64)
        out[f"{tag}_append"] = np.array(append, dtype=np.int64)
        rs = np.random.RandomState(19)
        batches = []
        for s in range(STEPS):
            batches.append({"obs": rs.randn(B, D).astype(np.float32), "next_obs": rs.randn(B, D).astype(np.float32),
                            "acts": rs.randint(0, A, size=(B,)).astype(np.float32),
                            "rewards": rs.randn(B, 1).astype(np.float32),
                            "terminals": (rs.rand(B, 1) < 0.2).astype(np.float32),
                            "masks": rs.binomial(1, P, size=(B, K)).astype(np.float32)})
        with torch.no_grad():
            q0 = qf(torch.from_numpy(batches[0]["obs"]), range(K))
            out[f"{tag}_q0"] = np.stack([q.numpy() for q in q0])                          # (K, B, A)
            single = rs.randn(8, D).astype(np.float32)
            out[f"{tag}_single_obs"] = single
            explore = np.zeros((K, 8), dtype=np.int64)
            for k in range(K):
                pf.set_head(k)
                for i in range(8):
                    explore[k, i] = pf.explore(torch.from_numpy(single[i:i + 1]))["action"]
            out[f"{tag}_explore"] = explore
            out[f"{tag}_eval"] = np.array([pf.eval_act(torch.from_numpy(single[i:i + 1])) for i in range(8)], dtype=np.int64)
        for s, batch in enumerate(batches):
            out.update({f"{tag}_s{s}_batch_{k}": v for k, v in batch.items()})
            info = agent.update(batch)
            keys = sorted(info.keys())
            out[f"{tag}_s{s}_info_keys"] = np.array(keys)
            out[f"{tag}_s{s}_info_vals"] = np.array([float(info[k]) for k in keys], dtype=np.float64)
        out.update(mg.state_arrays(f"{tag}_qf1_", qf))
        out.update(mg.state_arrays(f"{tag}_tqf1_", agent.target_qf))
    return out


def main():
    mg.install_stubs()
    arrays, seed, rejected = generate_conditioned()
    meta = dict(json.loads(mg.META), init_seed=seed, rejected_init_seeds=rejected, reference_error_max=REF_ERR_MAX,
                how="unmodified reference classes; add_ln is a falsy stand-in whose __pow__ returns False (see the docstring)")
    check = "--check" in sys.argv[1:]
    out_dir = tempfile.mkdtemp(prefix="trl_golden_check_") if check else HERE
    path = os.path.join(out_dir, NAME + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), cases=np.array(list(CASES)), **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")
    if check:
        new, old = np.load(path), np.load(os.path.join(HERE, NAME + ".npz"))
        ok = sorted(new.files) == sorted(old.files) and all(
            new[k].shape == old[k].shape and np.array_equal(new[k], old[k], equal_nan=new[k].dtype.kind == "f")
            for k in new.files if k != "meta")
        print("%-32s %s" % (NAME + ".npz", "identical" if ok else "DIFFERS"))
        sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
