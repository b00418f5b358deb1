#!/usr/bin/env python
"""Generate tests/golden/sac_v_update*.npz by running the REFERENCE implementation on the CPU: its own `SAC`
(algo/off_policy/sac.py:74-208) and `TwinSAC` (algo/off_policy/twin_sac.py:82-229), the soft actor-critics that keep a
value network V and its Polyak target beside the critic(s).

Why this runs under `python -O`: both `update` methods contain `assert v_target == v_pred` (sac.py:130,
twin_sac.py:142), which for a batch of more than one row raises "Boolean value of Tensor with more than one value is
ambiguous".  With assertions compiled out the unmodified classes run; the evident intent of the line is a shape check.
Started without -O (`sys.flags.optimize == 0`) this script starts itself again as a fresh child process with -O and
returns that child's exit status.  `meta` records the generating versions and the optimize flag.

Five cases, all with D = 17, A = 6, tanh_action=True, ReLU nets, two chained updates under torch.manual_seed(100 + s)
and a fifth of the terminals set:

    sac_h128    SAC      H = 128  B = 256  no regularisers  no clip  entropy tuning on
    twin_h128   TwinSAC  H = 128  B = 256  no regularisers  no clip  entropy tuning on
    sac_reg     SAC      H = 64   B = 96   1e-3             clip 1   entropy tuning on
    twin_reg    TwinSAC  H = 64   B = 96   1e-3             clip 1   entropy tuning on
    twin_fixed  TwinSAC  H = 64   B = 96   no regularisers  no clip  entropy tuning off (alpha = 1)

Conditioning.  Adam's step lr * m / (sqrt(v) + 1e-8) is ill-conditioned where a gradient entry comes near 1e-8 in
size: there the reference's own fp32 rounding decides the step (at the initialisation seeded with 31 one first-layer
weight of V in `sac_h128` ends 5.0e-6 away from the exact result, every other parameter of every case within 1.2e-6).
A fixture is meant to pin the algorithm, not one machine's rounding, and its consumers hold parameters to 3e-6.  So the
initialisation seed -- the one thing the cases leave open -- is the first from 31 on at which all final parameters of
the reference's fp32 run lie within 1e-6, a third of that bound, of the same updates carried out in float64 by
tests/_sac_v_ref.py.  This measures the reference's own error and nothing else; `meta` records the seed taken and the
seeds rejected with their errors.

The 64-wide cases, `meta` and the list of cases are in sac_v_update.npz; each 128-wide case has a file of its own,
sac_v_update_<case>.npz, because no file in this repository may exceed 1 MiB (fp32 parameters do not compress).
tests/_sac_v_ref.py::load_fixture reads them back as one mapping.

    python -O tests/golden/make_golden_sac_v.py            # writes tests/golden/sac_v_update*.npz
    python tests/golden/make_golden_sac_v.py --check       # regenerates into a scratch dir, compares bit for bit

Data only: initial and final state dicts (target_vf included), batches, the policy noise, info keys / values, log_alpha.
"""
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

NAME = "sac_v_update"
D, A, STEPS = 17, 6, 2
SEED0, REF_ERR_MAX = 31, 1e-6                                                # see "Conditioning" in the docstring
# tag: class name, hidden width, batch size, regulariser weights, grad_clip (0: none), entropy tuning
CASES = {"sac_h128": ("SAC", 128, 256, 0.0, 0.0, 1), "twin_h128": ("TwinSAC", 128, 256, 0.0, 0.0, 1),
         "sac_reg": ("SAC", 64, 96, 1e-3, 1.0, 1), "twin_reg": ("TwinSAC", 64, 96, 1e-3, 1.0, 1),
         "twin_fixed": ("TwinSAC", 64, 96, 0.0, 0.0, 0)}


def net_names(cls):
    return ("pf", "qf", "vf") if cls == "SAC" else ("pf", "qf1", "qf2", "vf")


def reference_error(arrays):
    """The reference's OWN rounding error in the stored final parameters: their largest distance from the same two
    updates carried out in float64 (tests/_sac_v_ref.py, explicit chain rule)."""
    sys.path.insert(0, os.path.dirname(HERE))
    import _sac_v_ref as ref
    worst = 0.0
    for tag in CASES:
        up, _, steps = ref.update_from_fixture(arrays, tag)
        for s in range(steps):
            up.update({k: arrays[f"{tag}_s{s}_batch_{k}"] for k in ref.BATCH_KEYS}, arrays[f"{tag}_s{s}_eps"])
        mine = dict(zip(net_names(CASES[tag][0]), [up.pf] + up.qfs + [up.vf]), tvf=up.tvf)
        for name, layers in mine.items():
            for pair, pair_ref in zip(layers, ref.layers_of(arrays, f"{tag}_{name}1_")):
                worst = max([worst] + [float(np.abs(x - y).max()) for x, y in zip(pair, pair_ref)])
    return worst


def generate_conditioned():
    """(arrays, init seed, {rejected seed: error}): the first init seed from SEED0 on at which the reference's own error
    stays below REF_ERR_MAX."""
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
    import torchrl.policies as policies
    import torchrl.networks as networks
    import torchrl.algo as algo
    from oracle.synth_env import SynthVecEnvCPU
    out = {}
    for tag, (cls, H, B, w_reg, clip, tune) in CASES.items():
        torch.manual_seed(seed)
        net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase,
                   activation_func=torch.nn.ReLU)
        nets = {"pf": policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net)}
        for name in net_names(cls)[1:-1]:
            nets[name] = networks.QNet(input_shape=D + A, output_shape=1, **net)
        nets["vf"] = networks.Net(input_shape=D, output_shape=1, **net)
        env = SynthVecEnvCPU(4)
        env.action_space = gym.spaces.Box(-1, 1, (A,))
        agent = getattr(algo, cls)(plr=3e-4, vlr=1e-3, qlr=1e-3, policy_std_reg_weight=w_reg, policy_mean_reg_weight=w_reg,
                                   reparameterization=True, automatic_entropy_tuning=bool(tune), env=env,
                                   replay_buffer=None, collector=mg._StubCollector(), logger=mg.NullLogger(),
                                   grad_clip=clip if clip else None, discount=0.99, num_epochs=10, batch_size=B,
                                   device=torch.device("cpu"), save_dir=tempfile.mkdtemp(prefix="trl_save_"), tau=0.005,
                                   use_soft_update=True, opt_times=1, **nets)
        for name, mod in nets.items():
            out.update(mg.state_arrays(f"{tag}_{name}0_", mod))
        out[f"{tag}_args"] = np.array([H, B, w_reg, clip, tune, STEPS], dtype=np.float64)
        out[f"{tag}_class"] = np.array(cls)
        rs = np.random.RandomState(17)
        for s in range(STEPS):
            batch = {"obs": rs.randn(B, D).astype(np.float32), "next_obs": rs.randn(B, D).astype(np.float32),
                     "acts": np.tanh(rs.randn(B, A)).astype(np.float32), "rewards": rs.randn(B, 1).astype(np.float32),
                     "terminals": (rs.rand(B, 1) < 0.2).astype(np.float32)}
            out.update({f"{tag}_s{s}_batch_{k}": v for k, v in batch.items()})
            torch.manual_seed(100 + s)
            state = torch.get_rng_state()
            info = agent.update(batch)
            after = torch.get_rng_state()
            torch.set_rng_state(state)
            out[f"{tag}_s{s}_eps"] = torch.randn(B, A).numpy()            # the one policy sample of the update
            if not torch.equal(torch.get_rng_state(), after):               # (no assert: they are compiled out here)
                raise RuntimeError("noise stream mismatch")
            keys = sorted(info.keys())
            out[f"{tag}_s{s}_info_keys"] = np.array(keys)
            out[f"{tag}_s{s}_info_vals"] = np.array([float(info[k]) for k in keys], dtype=np.float64)
        for name, mod in list(nets.items()) + [("tvf", agent.target_vf)]:
            out.update(mg.state_arrays(f"{tag}_{name}1_", mod))
        if tune:
            out[f"{tag}_log_alpha"] = agent.log_alpha.detach().numpy().copy()
    return out


def split(arrays, meta):
    """{file name: arrays}: the cases wider than 64 in files of their own (the 1 MiB limit), the rest in NAME.npz."""
    files = {NAME + ".npz": {"meta": np.array(meta), "cases": np.array(list(CASES))}}
    for tag, case in CASES.items():
        fname = NAME + (".npz" if case[1] <= 64 else "_%s.npz" % tag)
        files.setdefault(fname, {}).update({k: v for k, v in arrays.items() if k.startswith(tag + "_")})
    if sum(len(f) for f in files.values()) != len(arrays) + 2:
        raise RuntimeError("an array belongs to no case")
    return files


def main():
    if sys.flags.optimize == 0:                                              # see the docstring: a fresh child with -O
        sys.exit(subprocess.call([sys.executable, "-O", os.path.abspath(__file__)] + sys.argv[1:]))
    mg.install_stubs()
    arrays, seed, rejected = generate_conditioned()
    meta = dict(json.loads(mg.META), optimize=int(sys.flags.optimize), init_seed=seed, rejected_init_seeds=rejected,
                reference_error_max=REF_ERR_MAX,
                why_optimize="sac.py:130 / twin_sac.py:142 assert a tensor comparison; -O compiles assertions out")
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
            print("%-32s %s" % (fname, "identical" if ok else "DIFFERS"))
            same = same and ok
    if check:
        sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
