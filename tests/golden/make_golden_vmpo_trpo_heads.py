#!/usr/bin/env python
"""Generate tests/golden/vmpo_trpo_heads.npz by running the REFERENCE implementation on the CPU: its own `VMPO.update`
(v_mpo.py:57-181) and `TRPO.update` / `update_vf` (trpo.py:153-257) with its own `CategoricalDisPolicy`
(policies/discrete_policies.py:124-168, `acts` of shape (B,), as the reference needs) and `GuassianContPolicy`
(policies/continuous_policy.py:156-170).

V-MPO takes both reference policies unchanged.  For TRPO with the categorical policy the reference's discrete
`mean_kl_divergence` (trpo.py:53-61) does arithmetic on the `"dis"` entry of what `update()` returns, which the reference
policy fills with a `Categorical` object; the policy is subclassed ONLY so that `update()` puts the probability tensor
(`dis.probs`) under `"dis"` -- nothing else is touched (`_WithLogStd` of make_golden_categorical.py is the precedent).
That subclass is used for TRPO only.

The line search's trials are read off the reference by wrapping the agent's own `linesearch` / `surrogate_loss` bound
methods (their arguments and return values are recorded, nothing is changed): the acceptance ratio and the actual
improvement of every trial, and the accepted backtrack index (-1: none).

Seeds.  A TRPO case whose accept / reject decision is marginal would test rounding: for each case the first seed of
SEEDS + 0, 1, ... is taken for which (checked here, against the float64 restatement tests/_vmpo_trpo_heads_ref.py::HeadTRPO
on the same parameters and batch) the reference's accepted backtrack index equals the restatement's, every trial's
acceptance ratio is at least 0.02 away from 0.1, every actual improvement is at least 1e-4 away from 0, the policy
gradient is non-zero, and -- so that the case does not sit at the edge of the 1e-4 the parameters are compared within
(tests/test_trpo_gpu.py) because the reference's own ten float32 CG iterations are ill-conditioned there -- the
restatement's stepped parameters are within 2.5e-5 of the reference's.  The seed taken is stored.

    python tests/golden/make_golden_vmpo_trpo_heads.py            # writes tests/golden/vmpo_trpo_heads.npz
    python tests/golden/make_golden_vmpo_trpo_heads.py --check    # regenerates into a scratch dir, compares bit for bit

Data only: parameters, batches, info dicts (NaN where the reference logs NaN), line-search records, post-step parameters.
"""
import contextlib
import io
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                                     # noqa: E402 -- helpers only

NAME = "vmpo_trpo_heads"
# tag: D, A, hidden width, batch size
SHAPES = {"s4": (4, 2, 32, 64), "s17": (17, 6, 64, 96)}
SEEDS = {"vmpo": 21, "trpo": 40}
VMPO_STEPS = 4
TRPO_MARGIN_RATIO, TRPO_MARGIN_IMPROVE, TRPO_MARGIN_PARAMS = 0.02, 1e-4, 2.5e-5


def build(kind, D, A, H, seed, tanh_action=False, probs_as_dis=False):
    import torchrl.policies as policies
    import torchrl.networks as networks

    class _ProbsAsDis(policies.CategoricalDisPolicy):
        def update(self, obs, actions):
            out = super().update(obs, actions)
            out["dis"] = out["dis"].probs
            return out

    torch.manual_seed(seed)
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    if kind == "cat":
        pf = (_ProbsAsDis if probs_as_dis else policies.CategoricalDisPolicy)(input_shape=D, output_shape=A, **net)
    else:
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=tanh_action, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    with torch.no_grad():                                   # away from the +-3e-3 head init
        pf.seq_append_fcs[-1].weight.mul_(30.0)
        vf.seq_append_fcs[-1].weight.mul_(30.0)
        if kind == "sd":
            pf.seq_append_fcs[-1].bias[A:].sub_(0.7)        # log_std around -0.7
    return pf, vf


def make_batch(kind, pf, rs, D, A, B, tanh_action):
    obs = rs.randn(B, D).astype(np.float32)
    if kind == "cat":
        acts = rs.randint(0, A, size=(B,)).astype(np.float32)
    else:
        with torch.no_grad():
            mean, std, _ = pf(torch.tensor(obs))
        z = mean + std * torch.tensor(rs.randn(B, A).astype(np.float32))
        acts = (torch.tanh(z).clamp(-0.98, 0.98) if tanh_action else z).numpy()
    return {"obs": obs, "acts": acts, "advs": rs.randn(B, 1).astype(np.float32) * 2 + 0.5,
            "values": rs.randn(B, 1).astype(np.float32), "estimate_returns": rs.randn(B, 1).astype(np.float32)}


def info_arrays(prefix, info):
    keys = sorted(info.keys())
    return {prefix + "_keys": np.array(keys), prefix + "_vals": np.array([info[k] for k in keys], dtype=np.float64)}


def flat_params(module):
    import torch.nn as nn
    lin = [m for m in list(module.base.seq_fcs) + list(module.seq_append_fcs) if isinstance(m, nn.Linear)]
    return [t.detach().clone() for m in lin for t in (m.weight, m.bias)]


def env_for(kind, A):
    import gym
    from oracle.synth_env import SynthVecEnvCPU
    env = SynthVecEnvCPU(4)
    env.action_space = gym.spaces.Discrete(A) if kind == "cat" else gym.spaces.Box(-1, 1, (A,))
    return env


def common(kind, A):
    return dict(tau=0.95, shuffle=True, discount=0.99, num_epochs=10, gae=True, env=env_for(kind, A), replay_buffer=None,
                collector=mg._StubCollector(), logger=mg.NullLogger(), device=torch.device("cpu"),
                save_dir=tempfile.mkdtemp(prefix="trl_save_"))


def vmpo_case(kind, tag, D, A, H, B):
    import torchrl.algo.utils as atu
    from torchrl.algo import VMPO
    tanh_action = kind == "sd"
    pre = f"vmpo_{kind}_{tag}"
    out = {}
    pf, vf = build(kind, D, A, H, SEEDS["vmpo"] + D, tanh_action)
    agent = VMPO(pf=pf, vf=vf, plr=1e-3, vlr=1e-3, opt_epochs=2, eta_eps=0.02, alpha_eps=0.1, batch_size=B, **common(kind, A))
    atu.copy_model_params_from_to(agent.pf, agent.target_pf)
    out[pre + "_args"] = np.array([D, A, H, B, int(tanh_action)], dtype=np.int64)
    out.update(mg.state_arrays(pre + "_pf0_", pf))
    out.update(mg.state_arrays(pre + "_vf0_", vf))
    rs = np.random.RandomState(300 + D)
    for s in range(VMPO_STEPS):
        batch = make_batch(kind, pf, rs, D, A, B, tanh_action)
        out.update({f"{pre}_s{s}_batch_{k}": v for k, v in batch.items()})
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                               # (std of one element: the NaN the reference logs)
            out.update(info_arrays(f"{pre}_s{s}_info", agent.update(batch)))
        out[f"{pre}_s{s}_eta_alpha"] = np.array([agent.eta.item(), agent.alpha.item()], dtype=np.float64)
        out.update(mg.state_arrays(f"{pre}_pf{s + 1}_", pf))
    out.update(mg.state_arrays(f"{pre}_vf{VMPO_STEPS}_", vf))
    return out


TRPO_HYPER = dict(max_kl=0.01, cg_damping=0.1, cg_iters=10, residual_tol=1e-10, entropy_coeff=0.01)


def trpo_once(kind, tag, D, A, H, B, seed):
    """-> (arrays, why the seed is refused or None)."""
    from torchrl.algo import TRPO
    sys.path.insert(0, os.path.dirname(HERE))
    import _vmpo_trpo_heads_ref as ref
    pre = f"trpo_{kind}_{tag}"
    out = {}
    pf, vf = build(kind, D, A, H, seed, False, probs_as_dis=True)
    agent = TRPO(pf=pf, vf=vf, plr=3e-4, vlr=1e-3, v_opt_times=2, batch_size=64, **TRPO_HYPER, **common(kind, A))
    out[pre + "_args"] = np.array([D, A, H, B, 0], dtype=np.int64)
    out[pre + "_seed"] = np.array(seed, dtype=np.int64)
    out.update(mg.state_arrays(pre + "_pf0_", pf))
    out.update(mg.state_arrays(pre + "_vf0_", vf))
    batch = make_batch(kind, pf, np.random.RandomState(seed + 1000), D, A, B, False)
    batch.pop("values")
    out.update({f"{pre}_batch_{k}": v for k, v in batch.items()})
    restated = ref.HeadTRPO(kind, flat_params(pf), flat_params(vf), dtype=torch.float64, vlr=1e-3, **TRPO_HYPER)

    # ---- record the reference's own line search: arguments and return values of its bound methods ----
    rec = {"fvals": [], "rate": None}
    ls, sl = agent.linesearch, agent.surrogate_loss

    def surrogate_loss(theta):
        val = sl(theta)
        rec["fvals"].append(float(val))
        return val

    def linesearch(x, fullstep, rate):
        rec["rate"] = float(rate)
        return ls(x, fullstep, rate)

    agent.surrogate_loss, agent.linesearch = surrogate_loss, linesearch
    with contextlib.redirect_stdout(io.StringIO()):
        info = agent.update(batch)
    if rec["rate"] is None:
        return out, "the policy gradient is zero"
    fval, trials = rec["fvals"][0], rec["fvals"][1:]
    actual = np.array([fval - f for f in trials])
    ratios = actual / (rec["rate"] * 0.5 ** np.arange(len(trials)))
    accepted = len(trials) - 1 if (ratios[-1] > 0.1 and actual[-1] > 0) else -1
    out.update(info_arrays(pre + "_info", info))
    out[pre + "_search_actual"], out[pre + "_search_ratio"] = actual, ratios
    out[pre + "_accepted"] = np.array(accepted, dtype=np.int64)
    out.update(mg.state_arrays(pre + "_pf1_", pf))
    vbatch = {"obs": batch["obs"], "estimate_returns": batch["estimate_returns"]}
    for s in range(2):
        out.update(info_arrays(f"{pre}_vinfo{s}", agent.update_vf(vbatch)))
        out.update(mg.state_arrays(f"{pre}_vf{s + 1}_", vf))

    # ---- the conditions on the case ----
    restated.update(batch)
    if not restated.grad_nonzero:
        return out, "the restatement's policy gradient is zero"
    if restated.accepted != accepted:
        return out, "accepted backtrack %d, the float64 restatement accepts %d" % (accepted, restated.accepted)
    both = list(ratios) + [r for _, r in restated.search]
    if min(abs(r - 0.1) for r in both) < TRPO_MARGIN_RATIO:
        return out, "an acceptance ratio within %g of 0.1" % TRPO_MARGIN_RATIO
    if min(abs(a) for a in list(actual) + [a for a, _ in restated.search]) < TRPO_MARGIN_IMPROVE:
        return out, "an actual improvement within %g of 0" % TRPO_MARGIN_IMPROVE
    dev = max((p.detach() - q.double()).abs().max().item() for p, q in zip(restated.pf, flat_params(pf)))
    if dev > TRPO_MARGIN_PARAMS:
        return out, "the float64 restatement's step is %.1e away from the reference's" % dev
    return out, None


def trpo_case(kind, tag, D, A, H, B):
    for seed in range(SEEDS["trpo"] + D, SEEDS["trpo"] + D + 32):
        arrays, why = trpo_once(kind, tag, D, A, H, B, seed)
        if why is None:
            return arrays
        print("trpo %s %s: seed %d refused (%s)" % (kind, tag, seed, why))
    raise SystemExit("no seed meets the conditions for trpo %s %s" % (kind, tag))


def generate():
    out = {}
    for tag, (D, A, H, B) in SHAPES.items():
        for kind in ("cat", "sd"):
            out.update(vmpo_case(kind, tag, D, A, H, B))
            out.update(trpo_case(kind, tag, D, A, H, B))
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
