"""REINFORCE against A2C at the benchmark size (2048 envs x 128 steps, 17-64-64-6, B = 65 536), one MI355X:

  rollout    one fused rollout (`collector.train_one_epoch()`: the persistent kernel + what follows it) with the vacant
             critic -- the zero-storing streaming launch -- against the same with a value network -- the MFMA value pass;
  iteration  collect + `update_per_epoch` of `Reinforce` against the same of `A2C` on config/a2c_synth_halfcheetah.json's
             sizes (4 minibatches per epoch).

Both pairs run in ONE process, alternating, after `--warmup` rounds (the launch sequences are captured into HIP graphs on
their second or third visit); each sample is a host clock around work that ends in a device synchronise; medians and the
spread (min, max) over `--reps` samples.  Device noise, no logger, no evaluation.  Prints one JSON line.

    python tools/time_reinforce.py [--envs 2048] [--steps 128] [--batch 65536] [--reps 30] [--warmup 6]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


class _Log:
    def add_update_info(self, d): pass
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


def make(kind, N, T, B, dev):
    from torchrl_amd import networks, policies
    from torchrl_amd.algo import A2C, Reinforce
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    torch.manual_seed(0)
    cfg = {"reward_scale": 1, "obs_norm": False}
    env, eval_env = (get_vec_env("SynthHalfCheetah-v0", cfg, N, device=dev) for _ in range(2))
    env.seed(0)
    net = dict(hidden_shapes=[64, 64], append_hidden_shapes=[], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    pf = policies.GuassianContPolicyBasicBias(input_shape=17, output_shape=6, tanh_action=True, **net).to(dev)
    vf = networks.ZeroNet() if kind == "reinforce" else networks.Net(input_shape=(17,), output_shape=1, **net).to(dev)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=dev, train_render=False,
                               epoch_frames=N * T, max_episode_frames=1000, eval_episodes=1, noise_mode="device")
    common = dict(shuffle=True, discount=0.99, num_epochs=1000, batch_size=B, env=env, replay_buffer=buf, collector=col,
                  logger=_Log(), device=dev, save_dir=None)
    if kind == "reinforce":
        agent = Reinforce(pf=pf, plr=3e-4, entropy_coeff=0.005, **common)
    else:
        agent = A2C(pf=pf, vf=vf, plr=3e-4, vlr=3e-4, tau=0.95, gae=True, entropy_coeff=0.005, **common)
    assert col._spec is not None, "the fused rollout is not the route at this shape"
    return agent, col


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(samples):
    a = np.asarray(samples)
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    kinds = ("reinforce", "a2c")
    made = {k: make(k, a.envs, a.steps, a.batch, dev) for k in kinds}

    def rollout(k):
        made[k][1].train_one_epoch()                                       # (enqueues the rollout; its result is read lazily)

    def iteration(k):
        agent, col = made[k]
        col.train_one_epoch()
        agent.update_per_epoch()

    out = {"envs": a.envs, "steps": a.steps, "batch": a.batch, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for name, fn in (("rollout", rollout), ("iteration", iteration)):
        samples = {k: [] for k in kinds}
        for r in range(a.warmup + a.reps):
            for k in kinds:                                                   # alternating: both see the same machine
                ms = timed(lambda: fn(k))
                if r >= a.warmup:
                    samples[k].append(ms)
        out[name] = {k: stats(v) for k, v in samples.items()}
        out[name]["reinforce_over_a2c"] = round(out[name]["reinforce"]["median_ms"] / out[name]["a2c"]["median_ms"], 4)
    engines = {k: type(made[k][0].engine()).__name__ for k in kinds}
    out["engines"] = engines
    print(json.dumps(out))


if __name__ == "__main__":
    main()
