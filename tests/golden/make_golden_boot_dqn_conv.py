#!/usr/bin/env python
"""Generate tests/golden/boot_dqn_conv_update.npz by running the REFERENCE implementation on the CPU: its own
`BootstrappedDQN` (algo/off_policy/bootstrapped_dqn.py:7-104), `BootstrappedNet` (networks/nets.py:71-121) over
`functools.partial(CNNBase, ...)` (networks/base.py:59-107) and `BootstrappedDQNDiscretePolicy`
(policies/discrete_policies.py:92-121), all UNMODIFIED -- made to run as make_golden_boot_dqn.py makes them run (the
`_FalsyLn` stand-in for `add_ln`, no extra keyword arguments), and fed the float frames u8 / 255 - 0.5 of
ScaledFloatFrame as make_golden.py's DQN case feeds them.

Three cases, each two chained updates, K = 3 heads, A = 3 actions, the conv stack of tests/test_dqn_gpu.py
[[8, 8x8, s4], [8, 4x4, s2], [16, 3x3, s1]] over (4, 44, 44) frames (10 -> 4 -> 2: P = 4, F = 64), ReLU, B = 4, a fifth of
the terminals set, Bernoulli(0.5) masks, qlr = 1e-3, discount 0.99, tau = 0.005:

    lin    append_hidden_shapes []     Adam                               soft target update
    hid    append_hidden_shapes [32]   Adam                               soft target update
    rms    append_hidden_shapes [32]   RMSprop(alpha=0.95, eps=0.01)      use_soft_update=False, target_hard_update_period=2

The two batches (uint8 frames and all) are shared by the cases and stored once.

Conditioning (the rule of make_golden_boot_dqn.py): the initialisation seed is the first from 31 on at which all
parameters (online and target, after either update) of the reference's fp32 run lie within 1e-6 of the same updates
carried out in float64 by tests/_boot_conv_ref.py; `meta` records the seed taken, the seeds rejected with their errors and
the error at the seed taken.

Stored per case (data only): the initial state dict (the target starts as its copy), after each update the state dicts of
the online and the target network, the optimiser's state under torch's names and the info keys and values; per head
`qf(obs, range(K))` on the first batch (initial parameters), and the `explore` / `eval_act` actions of the initial
network for the first batch's four frame stacks under each head.

    python tests/golden/make_golden_boot_dqn_conv.py            # writes tests/golden/boot_dqn_conv_update.npz
    python tests/golden/make_golden_boot_dqn_conv.py --check    # regenerates into a scratch dir, compares bit for bit
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
from make_golden_boot_dqn import _FalsyLn                                    # noqa: E402

NAME = "boot_dqn_conv_update"
A, K, B, STEPS, P = 3, 3, 4, 2, 0.5
SHAPE = (4, 44, 44)
CONVS = [[8, [8, 8], [4, 4], [0, 0]], [8, [4, 4], [2, 2], [0, 0]], [16, [3, 3], [1, 1], [0, 0]]]
QLR, TAU = 1e-3, 0.005
SEED0, REF_ERR_MAX = 31, 1e-6
# tag: append_hidden_shapes, optimiser (class name, keyword arguments), use_soft_update, target_hard_update_period
CASES = {"lin": ([], ("Adam", {}), True, 1000), "hid": ([32], ("Adam", {}), True, 1000),
         "rms": ([32], ("RMSprop", {"alpha": 0.95, "eps": 0.01}), False, 2)}
BATCH_KEYS = ("obs", "next_obs", "acts", "rewards", "terminals", "masks")


def batches():
    rs = np.random.RandomState(19)
    out = []
    for _ in range(STEPS):
        out.append({"obs": rs.randint(0, 256, size=(B,) + SHAPE).astype(np.uint8),
                    "next_obs": rs.randint(0, 256, size=(B,) + SHAPE).astype(np.uint8),
                    "acts": rs.randint(0, A, size=(B,)).astype(np.float32),
                    "rewards": rs.randn(B, 1).astype(np.float32),
                    "terminals": (rs.rand(B, 1) < 0.2).astype(np.float32),
                    "masks": rs.binomial(1, P, size=(B, K)).astype(np.float32)})
    return out


def to_float(u8):
    return u8.astype(np.float32) / 255.0 - 0.5


def reference_error(arrays):
    """The reference's OWN rounding error in the stored parameters: their largest distance from the same updates carried
    out in float64 (tests/_boot_conv_ref.py, explicit chain rule), over both updates, online and target."""
    sys.path.insert(0, os.path.dirname(HERE))
    import _boot_conv_ref as ref
    worst = 0.0
    for tag in CASES:
        up, a = ref.update_from_fixture(arrays, tag)
        for s in range(a["steps"]):
            up.update(ref.batch_of(arrays, s))
            for mine, name in ((up.params, "qf%d" % (s + 1)), (up.tparams, "tqf%d" % (s + 1))):
                want = ref.params_of(ref.net_of(arrays, f"{tag}_{name}_", a["K"]))
                worst = max([worst] + [float(np.abs(x - y).max()) for x, y in zip(mine, want)])
    return worst


def generate_conditioned():
    rejected = {}
    for seed in range(SEED0, SEED0 + 16):
        arrays = generate(seed)
        err = reference_error(arrays)
        print("init seed %d: the reference's fp32 parameters are within %.3g of the float64 update" % (seed, err))
        if err < REF_ERR_MAX:
            return arrays, seed, rejected, err
        rejected[str(seed)] = err
    raise RuntimeError("no init seed in [%d, %d) gives a well-conditioned fixture" % (SEED0, SEED0 + 16))


def generate(seed):
    import gym
    import torchrl.networks as networks
    import torchrl.policies as policies
    from torchrl.algo.off_policy.bootstrapped_dqn import BootstrappedDQN
    out = {}
    data = batches()
    for s, batch in enumerate(data):
        out.update({f"batch_s{s}_{k}": v for k, v in batch.items()})

    class Env:
        action_space = gym.spaces.Discrete(A)
    for tag, (append, (opt_name, opt_kw), soft, period) in CASES.items():
        torch.manual_seed(seed)
        qf = networks.BootstrappedNet(output_shape=A, head_num=K, append_hidden_shapes=append, add_ln=_FalsyLn(),
                                      activation_func=torch.nn.ReLU,
                                      base_type=functools.partial(networks.CNNBase, input_shape=SHAPE, hidden_shapes=CONVS))
        pf = policies.BootstrappedDQNDiscretePolicy(qf=qf, head_num=K, action_shape=A)
        agent = BootstrappedDQN(head_num=K, bernoulli_p=P, qf=qf, pf=pf, qlr=QLR, env=Env(), replay_buffer=None,
                                collector=mg._StubCollector(), logger=mg.NullLogger(), discount=0.99, num_epochs=10,
                                batch_size=B, device=torch.device("cpu"), save_dir=tempfile.mkdtemp(prefix="trl_save_"),
                                tau=TAU, use_soft_update=soft, target_hard_update_period=period, opt_times=1,
                                optimizer_class=getattr(torch.optim, opt_name), optimizer_info=dict(opt_kw))
        out.update(mg.state_arrays(f"{tag}_qf0_", qf))
        t0 = mg.state_arrays("", agent.target_qf)
        assert all(np.array_equal(v, out[f"{tag}_qf0_" + k]) for k, v in t0.items())      # (the target starts as a copy)
        out[f"{tag}_args"] = np.array([K, B, int(soft), period, STEPS, QLR, TAU, len(append)], dtype=np.float64)
        out[f"{tag}_append"] = np.array(append, dtype=np.int64)
        out[f"{tag}_opt"] = np.array([0.0, 0.0, 0.0] if opt_name == "Adam" else [1.0, opt_kw["alpha"], opt_kw["eps"]])
        with torch.no_grad():
            frames = torch.from_numpy(to_float(data[0]["obs"]))
            out[f"{tag}_q0"] = np.stack([q.numpy() for q in qf(frames, range(K))])         # (K, B, A)
            explore = np.zeros((K, B), dtype=np.int64)
            for k in range(K):
                pf.set_head(k)
                for i in range(B):
                    explore[k, i] = pf.explore(frames[i:i + 1])["action"]
            out[f"{tag}_explore"] = explore
            out[f"{tag}_eval"] = np.array([pf.eval_act(frames[i:i + 1]) for i in range(B)], dtype=np.int64)
        for s, batch in enumerate(data):
            info = agent.update(dict(batch, obs=to_float(batch["obs"]), next_obs=to_float(batch["next_obs"])))
            keys = sorted(info.keys())
            out[f"{tag}_s{s}_info_keys"] = np.array(keys)
            out[f"{tag}_s{s}_info_vals"] = np.array([float(info[k]) for k in keys], dtype=np.float64)
            out.update(mg.state_arrays(f"{tag}_qf{s + 1}_", qf))
            out.update(mg.state_arrays(f"{tag}_tqf{s + 1}_", agent.target_qf))
            for pn, p in qf.named_parameters():
                for sn, v in agent.qf_optimizer.state[p].items():
                    if sn != "step":
                        out[f"{tag}_state{s + 1}_{sn}_{pn.replace('.', '__')}"] = v.detach().numpy().copy()
    return out


def main():
    mg.install_stubs()
    arrays, seed, rejected, err = generate_conditioned()
    meta = dict(json.loads(mg.META), init_seed=seed, rejected_init_seeds=rejected, reference_error_max=REF_ERR_MAX,
                reference_error=err,
                how="unmodified reference classes; add_ln is a falsy stand-in whose __pow__ returns False; float frames "
                    "u8 / 255 - 0.5 (see the docstring)")
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
