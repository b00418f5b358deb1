"""What the on-policy update engines compute, over their route matrix, as arrays -- to compare two commits bit for bit.

    python tools/dump_onpolicy_update.py OUT.npz            # run every case on cuda:0, write the arrays
    python tools/dump_onpolicy_update.py --compare A.npz B.npz   # every array must be array_equal; prints the count

Cases: {PPO, A2C} x {Gaussian, categorical (TRL_CAT_FUSED_UPDATE=1), state-dependent std (TRL_SD_FUSED_UPDATE=1)}
x {two chains, TRL_PPO_CHAINS=joint, TRL_GENERIC_PPO=1} x {graphs, TRL_NO_GRAPH=1}, plus V-MPO and TRPO (one update
each).  Every case: 17 / 6 / 64 x 64 nets, 64 envs x 16 steps, minibatches of 256, two passes; four iterations of
collect + update, so that eager, captured and replayed visits all occur.  Per case `flat`, `m`, `v`, `target_flat` and
every column of the info dicts are kept.  Only `agent.update_per_epoch()`, `agent.engine()` and the environment switches
are used, so the same file runs on any commit."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N, T, B, D, A = 64, 16, 256, 17, 6
SWITCHES = ("TRL_PPO_CHAINS", "TRL_GENERIC_PPO", "TRL_NO_GRAPH", "TRL_CAT_FUSED_UPDATE", "TRL_SD_FUSED_UPDATE")
ROUTES = {"two": {}, "joint": {"TRL_PPO_CHAINS": "joint"}, "generic": {"TRL_GENERIC_PPO": "1"}}
HEADS = {"gauss": {}, "cat": {"TRL_CAT_FUSED_UPDATE": "1"}, "sd": {"TRL_SD_FUSED_UPDATE": "1"}}


class _Log:
    def __init__(self):
        self.infos = []

    def add_update_info(self, d):
        self.infos.append(dict(d))

    def add_epoch_info(self, *a, **k):
        pass

    def log(self, *a):
        pass

    def finish(self):
        pass


def run_case(algo, head, env_switches, epochs):
    import torchrl_amd.networks as networks
    import torchrl_amd.policies as policies
    from torchrl_amd import algo as algos
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env_switches)
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    net = dict(hidden_shapes=[64, 64], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    if head == "cat":
        pf = policies.CategoricalDisPolicy(input_shape=D, output_shape=A, **net)
        with torch.no_grad():
            pf.seq_append_fcs[-1].weight.mul_(30.0)                      # leave the near-uniform initial policy
    elif head == "sd":
        pf = policies.GuassianContPolicy(input_shape=D, output_shape=2 * A, tanh_action=True, **net)
    else:
        pf = policies.GuassianContPolicyBasicBias(input_shape=D, output_shape=A, tanh_action=algo != "trpo", **net)
    vf = networks.Net(input_shape=(D,), output_shape=1, **net)
    name = "SynthCheetahDiscrete-v0" if head == "cat" else "SynthHalfCheetah-v0"
    env, eval_env = (get_vec_env(name, {"reward_scale": 1, "obs_norm": False}, N, device=dev) for _ in range(2))
    for e in (env, eval_env):
        e.horizon = 10
    env.seed(0)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=dev, train_render=False,
                               epoch_frames=N * T, max_episode_frames=7, eval_episodes=1, noise_mode="device")
    logger = _Log()
    general = dict(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, tau=0.95, shuffle=True, discount=0.99, num_epochs=10, batch_size=B,
                   gae=True, env=env, replay_buffer=buf, collector=col, logger=logger, device=dev, save_dir=None)
    if algo == "ppo":
        agent = algos.PPO(clip_para=0.2, opt_epochs=2, entropy_coeff=0.005, **general)
    elif algo == "a2c":
        agent = algos.A2C(entropy_coeff=0.005, **general)
    elif algo == "vmpo":
        agent = algos.VMPO(opt_epochs=2, **general)
    else:
        agent = algos.TRPO(max_kl=0.01, cg_damping=0.1, v_opt_times=1, cg_iters=10, residual_tol=1e-10, entropy_coeff=0.005,
                           **general)
    torch.manual_seed(0)
    for epoch in range(epochs):
        col.train_one_epoch()
        agent.current_epoch = epoch
        np.random.seed(epoch)
        agent.update_per_epoch()
    torch.cuda.synchronize()
    eng = agent.engine()
    out = {k: getattr(eng, k).detach().cpu().numpy() for k in ("flat", "m", "v")}
    if getattr(eng, "target_flat", None) is not None:
        out["target_flat"] = eng.target_flat.detach().cpu().numpy()
    for key in sorted({k for d in logger.infos for k in d}):
        out["info." + key.replace("/", ".")] = np.array([float(d.get(key, np.nan)) for d in logger.infos])
    out["n_infos"] = np.array(len(logger.infos))
    return out, type(eng).__name__


def cases():
    for algo in ("ppo", "a2c"):
        for head, hs in HEADS.items():
            for route, rs in ROUTES.items():
                for graph, gs in (("graph", {}), ("eager", {"TRL_NO_GRAPH": "1"})):
                    yield "%s-%s-%s-%s" % (algo, head, route, graph), algo, head, dict(hs, **rs, **gs), 4
    yield "vmpo", "vmpo", "gauss", {}, 1
    yield "trpo", "trpo", "gauss", {}, 1


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    if sorted(a.files) != sorted(b.files):
        print("different arrays:", sorted(set(a.files) ^ set(b.files)))
        return 1
    bad = [k for k in a.files if not np.array_equal(a[k], b[k], equal_nan=True)]
    for k in bad:
        print("DIFFERENT", k, float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()))
    print("%d arrays compared, %d different" % (len(a.files), len(bad)))
    return 1 if bad else 0


def main(argv):
    if argv[:1] == ["--compare"]:
        return compare(argv[1], argv[2])
    arrays = {}
    for name, algo, head, switches, epochs in cases():
        out, engine = run_case(algo, head, switches, epochs)
        print("%-28s %-14s %3d updates  |flat| %.6f" % (name, engine, int(out["n_infos"]), float(np.abs(out["flat"]).sum())),
              flush=True)
        arrays.update({name + "." + k: v for k, v in out.items()})
    os.makedirs(os.path.dirname(os.path.abspath(argv[0])), exist_ok=True)
    np.savez(argv[0], **arrays)
    print("%d arrays written to %s" % (len(arrays), argv[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
