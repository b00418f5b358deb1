#!/usr/bin/env python
"""Generate tests/golden/reinforce_update.npz by running the REFERENCE implementation on the CPU: its own
`Reinforce.update` (torchrl/algo/on_policy/reinforce.py:33-75) -- two chained calls on one seeded batch of B = 64 samples
(N = 8 envs x 8 of the T = 16 rows) -- for the three policy heads, and its `discount_reward`
(replay_buffers/on_policy.py:46-70) on a T = 16, N = 8 ring whose `values` are all zero, the critic REINFORCE has.

Heads (tag: D, A, H): `GuassianContPolicyBasicBias` g (17, 6, 64), `GuassianContPolicy` sd (5, 2, 32) and
`CategoricalDisPolicy` cat (4, 3, 32); Tanh nets, tanh actions clamped to +-0.995 (unclamped they reach |a| = 1.0 in fp32,
where the reference's log-prob is -inf).  After each update the info dict (in the reference's key order), the parameters
and Adam's exp_avg / exp_avg_sq are recorded.

Adam with torch's default eps = 1e-8 -- what the reference's constructor leaves it at -- makes the first steps ill-conditioned
for a parameter whose gradient is of the size of eps: step = lr g / (|g| + eps), so d step / d g = lr eps / (|g| + eps)^2,
up to lr / eps = 3e5.  A gradient element that is a sum of 64 cancelling terms carries an absolute float32 rounding error of
about 1e-10 in the reference's own run; where such an element is itself below ~1e-7, that rounding decides the parameter at
the 1e-5 level and the fixture would record the rounding, not the algorithm.  The reference's own error is measured, not
guessed: every draw is run FOUR times, three of them with the 64 batch rows in another order -- the same mathematics, other
float32 sums -- and the draw (network seed) is repeated until the parameters of the runs agree within SPREAD = 1e-7
after both updates, a tenth of the project's bound of 1e-6 on post-step parameters.  Only the run in the stored order is
recorded.  The condition is evaluated on the reference's runs alone.

    python tests/golden/make_golden_reinforce.py            # writes tests/golden/reinforce_update.npz
    python tests/golden/make_golden_reinforce.py --check    # regenerates into a scratch dir, compares bit for bit

Data only: parameters, batches, info dicts, optimiser moments, returns.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                                     # noqa: E402 -- helpers only

NAME = "reinforce_update"
N, T, B = 8, 16, 64
# tag: head, D, A, hidden width
HEADS = {"g": ("gauss", 17, 6, 64), "sd": ("sd", 5, 2, 32), "cat": ("cat", 4, 3, 32)}
PLR, ENT = 3e-3, 0.001                                                       # config/reinforce.json
SPREAD = 1e-7                                                                # see the module docstring


def build(head, D, A, H, seed):
    import torchrl.policies as policies
    import torchrl.networks as networks
    torch.manual_seed(seed)
    net = dict(hidden_shapes=[H, H], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    if head == "gauss":
        return policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=True, **net)
    if head == "cat":
        return policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
    pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net)
    last = [m for m in pf.modules() if isinstance(m, torch.nn.Linear)][-1]
    with torch.no_grad():
        last.bias[A:] = torch.linspace(-1.5, -0.5, A)                         # an exploration scale neither tiny nor saturated
    return pf


def moments(prefix, agent, pf):
    out = {}
    for name, p in pf.named_parameters():
        st = agent.pf_optimizer.state[p]
        out[prefix + "m_" + name.replace(".", "__")] = st["exp_avg"].detach().numpy().copy()
        out[prefix + "v_" + name.replace(".", "__")] = st["exp_avg_sq"].detach().numpy().copy()
    return out


def run_head(tag, head, D, A, H, seed, order=None):
    """-> arrays of this head's case; order: the batch rows are handed to the reference in this order."""
    import gym
    from torchrl.algo import Reinforce
    from oracle.synth_env import SynthVecEnvCPU
    out = {}
    rs = np.random.RandomState(300 + D)
    obs = rs.randn(B, D).astype(np.float32)
    pf = build(head, D, A, H, seed)
    if head == "cat":
        acts = rs.randint(0, A, size=(B,)).astype(np.float32)
    else:
        eps = rs.randn(B, A).astype(np.float32)
        with torch.no_grad():
            mean, std, _ = pf(torch.as_tensor(obs))
            acts = torch.tanh(mean + std * torch.as_tensor(eps)).clamp(-0.995, 0.995).numpy().astype(np.float32).copy()
    batch = {"obs": obs, "acts": acts, "advs": rs.randn(B, 1).astype(np.float32) * 2 + 0.5}
    if order is not None:
        batch = {k: np.ascontiguousarray(v[order]) for k, v in batch.items()}
    out.update({f"{tag}_batch_{k}": v for k, v in batch.items()})
    out[f"{tag}_args"] = np.array([D, A, H, B, seed], dtype=np.int64)
    out[f"{tag}_hyper"] = np.array([PLR, ENT], dtype=np.float64)
    out.update(mg.state_arrays(f"{tag}_pf0_", pf))
    env = SynthVecEnvCPU(4)
    env.action_space = gym.spaces.Discrete(A) if head == "cat" else gym.spaces.Box(-1, 1, (A,))
    agent = Reinforce(pf=pf, plr=PLR, entropy_coeff=ENT, shuffle=True, discount=0.99, num_epochs=10, batch_size=B,
                      env=env, replay_buffer=None, collector=mg._StubCollector(), logger=mg.NullLogger(),
                      device=torch.device("cpu"), save_dir=tempfile.mkdtemp(prefix="trl_save_"))
    assert agent.gae is False and type(agent.vf).__name__ == "ZeroNet"
    assert agent.pf_optimizer.param_groups[0]["eps"] == 1e-8
    for s in range(2):
        info = agent.update(batch)
        assert all(np.isfinite(v) for v in info.values()), (tag, s, info)
        out[f"{tag}_info{s}_keys"] = np.array(list(info.keys()))              # the reference's order
        out[f"{tag}_info{s}_vals"] = np.array(list(info.values()), dtype=np.float64)
        out.update(mg.state_arrays(f"{tag}_pf{s + 1}_", pf))
        out.update(moments(f"{tag}_adam{s + 1}_", agent, pf))
    return out


def case_updates(out):
    orders = [np.random.RandomState(7 + k).permutation(B) for k in range(3)]
    for tag, (head, D, A, H) in HEADS.items():
        for attempt in range(200):
            seed = 11 + D + 1000 * attempt
            arrays = run_head(tag, head, D, A, H, seed)
            others = [run_head(tag, head, D, A, H, seed, order) for order in orders]
            spread = max(float(np.abs(arrays[k] - other[k]).max()) for other in others for k in arrays
                         if k.startswith(f"{tag}_pf1_") or k.startswith(f"{tag}_pf2_"))
            if spread <= SPREAD:
                break
        else:
            raise AssertionError("no draw of %s meets the conditioning requirement" % tag)
        print("%s: network seed %d (draw %d), parameters under a reordered batch within %.3e" % (tag, seed, attempt + 1, spread))
        out[f"{tag}_spread"] = np.array([spread, SPREAD])
        out.update(arrays)


def case_discount(out):
    """Zero values: rewards, terminals and time limits that hit both (a terminal with and without a time limit, the last
    row included), for time_limit_filter False and True."""
    from torchrl.replay_buffers.on_policy import OnPolicyReplayBuffer
    rs = np.random.RandomState(41)
    r = rs.randn(T, N, 1).astype(np.float32)
    d = rs.rand(T, N, 1) < 0.2
    tl = (rs.rand(T, N, 1) < 0.5) & d
    d[T - 1, 0], tl[T - 1, 0] = True, True
    d[T - 1, 1], tl[T - 1, 1] = True, False
    assert tl.any() and (d & ~tl).any()
    out.update(disc_rewards=r, disc_terminals=d, disc_time_limits=tl, disc_args=np.array([T, N, 0.99]))
    for filt in (0, 1):
        buf = OnPolicyReplayBuffer(T * N, env_nums=N, time_limit_filter=bool(filt))
        buf._rewards, buf._values = r.astype(np.float64), np.zeros((T, N, 1))
        buf._terminals, buf._time_limits = d.astype(np.float64), tl.astype(np.float64)
        buf.discount_reward(np.zeros((N, 1)), 0.99)
        out[f"disc{filt}_advs"], out[f"disc{filt}_rets"] = buf._advs.copy(), buf._estimate_returns.copy()


def generate():
    out = {}
    case_updates(out)
    case_discount(out)
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
