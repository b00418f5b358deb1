"""The cases of the fused categorical rollout tests and their CPU restatement -- test infrastructure, imported by
tests/test_categorical_rollout_*.py only.

`cpu_rollout` steps oracle.synth_env.SynthVecEnvCPU with the restatement of the categorical draw
(tests/_categorical_ref.py) and the collector's bookkeeping (torchrl/collector/on_policy.py:90-155): over-length
bootstrap r += discount * vf(next_obs) * surpass, terminals = done | surpass, partial reset.  It also marks the
borderline rows (threshold within 1e-5 * S of a prefix sum), on which a kernel may draw the neighbouring action."""
import numpy as np
import torch

import _categorical_ref as ref

NOISE_SEED = 0xC011                                                   # VecCollector._noise_seed
DISCOUNT = 0.99                                                       # VecOnPolicyCollector's default
BORDERLINE_CAP = 0.01
ACTS = {"tanh": (torch.nn.Tanh, torch.tanh), "relu": (torch.nn.ReLU, torch.relu)}

# fused vs per-step: N = 40 is two full 16-env tiles and a partial one; horizon 5 < T = 12: episodes end and reset inside a
# rollout; two epochs: the second rollout's Philox keys continue from the global step.  max_frames = 4 < horizon: the
# over-length bootstrap fires (and `done` never does); 999: `done` fires alone.  (D, A) = (32, 8) is the wide tile,
# (4, 2) the smallest head.  The seeds were fixed after test_categorical_rollout_cpu.py's borderline check.
PAIR_N, PAIR_T, PAIR_HORIZON, PAIR_EPOCHS = 40, 12, 5, 2
PAIR_CASES = [dict(D=17, A=6, act="tanh", net_seed=21, env_seed=3, max_frames=999),
              dict(D=5, A=3, act="relu", net_seed=22, env_seed=4, max_frames=4),
              dict(D=32, A=8, act="tanh", net_seed=23, env_seed=5, max_frames=999),
              dict(D=4, A=2, act="tanh", net_seed=24, env_seed=6, max_frames=999)]
# the wide tile with ReLU at the smallest head on 24 envs (one full and one partial 16-env tile) x 2 steps: a branch of the
# tile / activation / head dispatch no other case reaches.  horizon 2: every episode ends inside the rollout.
WIDE_RELU_CASE = dict(D=18, A=2, act="relu", net_seed=25, env_seed=7, max_frames=999)
WIDE_RELU_N, WIDE_RELU_T, WIDE_RELU_HORIZON = 24, 2, 2
# fused vs CPU stepping: the shape of tests/test_categorical_gpu.py::test_collector_ring_vs_cpu_stepping with 64 x 64 nets
CPU_CASE = dict(D=17, A=6, act="tanh", net_seed=0, env_seed=3, max_frames=999)
CPU_N, CPU_T, CPU_HORIZON = 64, 16, 7


def case_id(c):
    return "D%d-A%d-%s-mf%d" % (c["D"], c["A"], c["act"], c["max_frames"])


def nets_of(D, A, act, net_seed, hidden=(64, 64), head_scale=30.0):
    """(pf, vf) on the CPU; the policy head scaled away from the near-uniform initial policy."""
    from torchrl_amd import networks, policies
    torch.manual_seed(net_seed)
    net = dict(hidden_shapes=list(hidden), append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=ACTS[act][0])
    pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    with torch.no_grad():
        pf.seq_append_fcs[-1].weight.mul_(head_scale)
    return pf, vf


def linear_params(mod):
    return [p for l in (list(mod.base.seq_fcs) + list(mod.seq_append_fcs)) if isinstance(l, torch.nn.Linear)
            for p in (l.weight, l.bias)]


def restated(mod, act):
    return ref.MLP([p.detach().cpu() for p in linear_params(mod)], act=ACTS[act][1])


def cpu_rollout(c, N, steps, horizon, nets=None):
    """`steps` vector steps from a fresh env -> dict of (steps, N, .) float32 arrays (obs, next_obs, acts, values, rewards,
    terminals, time_limits, old_logp) plus `borderline` (steps, N) bool, `epoch_reward` per step (steps,) float64 and
    `episodes`: [(step, env, return)] in (step, env) order."""
    from oracle.synth_env import SynthVecEnvCPU
    D, A = c["D"], c["A"]
    pf, vf = nets if nets is not None else nets_of(D, A, c["act"], c["net_seed"])
    cpf, cvf = restated(pf, c["act"]), restated(vf, c["act"])
    env = SynthVecEnvCPU(N, horizon=horizon, obs_dim=D, act_dim=A)
    env.seed(c["env_seed"])
    ob = torch.from_numpy(env.reset().astype(np.float32))
    cur_step, run_ret = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.float32)
    out = {k: [] for k in ("obs", "next_obs", "acts", "values", "rewards", "terminals", "time_limits", "old_logp",
                           "borderline", "epoch_reward")}
    episodes = []
    with torch.no_grad():
        for g in range(steps):
            logits, v = cpf(ob), cvf(ob)
            u = ref.uniforms(NOISE_SEED, g, 1, N)[0]
            a, lp, pre, S = ref.cat_act(logits, u)
            out["borderline"].append(ref.borderline(u, pre, S).numpy())
            nxt, rew, done, _ = env.step(torch.nn.functional.one_hot(a, A).float().numpy())
            done = done[:, 0]
            cur_step += 1
            run_ret += rew[:, 0]
            out["epoch_reward"].append(float(rew.astype(np.float64).sum()))
            for n in np.nonzero(done)[0]:
                episodes.append((g, int(n), float(run_ret[n])))
            run_ret[done] = 0
            surpass = cur_step >= c["max_frames"]
            v_next = cvf(torch.from_numpy(nxt)).numpy()[:, 0]
            stored_rew = (rew[:, 0] + np.float32(DISCOUNT) * v_next * surpass.astype(np.float32)).astype(np.float32)
            term = done | surpass
            for k, val in (("obs", ob.numpy()), ("next_obs", nxt), ("acts", a.numpy()[:, None].astype(np.float32)),
                           ("values", v.numpy()), ("rewards", stored_rew[:, None]),
                           ("terminals", term[:, None].astype(np.float32)), ("time_limits", done[:, None].astype(np.float32)),
                           ("old_logp", lp.numpy()[:, None])):
                out[k].append(np.array(val, dtype=np.float32))
            cur_step[term] = 0
            ob = torch.from_numpy(env.partial_reset(term).astype(np.float32))
    res = {k: np.stack(v) for k, v in out.items()}
    res["episodes"] = episodes
    return res
