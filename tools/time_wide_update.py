"""One PPO epoch of updates (`update_per_epoch`: GAE, 10 passes x 4 minibatches of 65 536 = 40 minibatch updates) of
config/ppo_synth_halfcheetah_w128.json's networks (plain, Tanh, 17 -> 128 -> 128 -> 6) at 2048 envs x 128 steps on both
engines, one MI355X:

  generic    `_GenericPPO`, as without TRL_WIDE_FUSED_UPDATE: ~25 dense-layer and loss launches per minibatch, replayed
             as a HIP graph from its third visit on -- what the parent commit does;
  fused      TRL_WIDE_FUSED_UPDATE=1: `_FusedPPO` on trl_ppo_wide_minibatch_grad_f32 + trl_ppo_wide_reduce_adam_net_f32.

Both agents live in ONE process, each with its own collector and ring (collected once, on the one-launch wide rollout),
and alternate after `--warmup` rounds; a sample is a host clock around `update_per_epoch()` + a device synchronise.
`iteration` is the same for rollout + update with both wide switches against neither.  Medians and the spread (min, max)
over `--reps` samples; prints one JSON line.

    python tools/time_wide_update.py [--envs 2048] [--steps 128] [--reps 20] [--warmup 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SWITCHES = ("TRL_WIDE_FUSED_UPDATE", "TRL_WIDE_FUSED_ROLLOUT")


class _Log:
    def add_update_info(self, d): pass
    def add_epoch_info(self, *a, **k): pass
    def log(self, *a): pass
    def finish(self): pass


def make(fused_update, fused_rollout, cfg, N, T, dev):
    from torchrl_amd import networks, policies
    from torchrl_amd.algo import PPO
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    torch.manual_seed(0)
    env, eval_env = (get_vec_env(cfg["env_name"], cfg["env"], N, device=dev) for _ in range(2))
    env.seed(0)
    net = dict(cfg["net"], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    pf = policies.GuassianContPolicyBasicBias(input_shape=env.obs_dim, output_shape=env.act_dim, **cfg["policy"], **net).to(dev)
    vf = networks.Net(input_shape=(env.obs_dim,), output_shape=1, **net).to(dev)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    for name, on in zip(SWITCHES, (fused_update, fused_rollout)):
        os.environ.pop(name, None)
        if on:
            os.environ[name] = "1"
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=dev, train_render=False,
                               epoch_frames=N * T, max_episode_frames=cfg["collector"]["max_episode_frames"], eval_episodes=1,
                               noise_mode=cfg["collector"]["noise_mode"])
    general = dict(cfg["general_setting"], batch_size=cfg["general_setting"]["batch_size"] * N * T // cfg["collector"]["epoch_frames"])
    general = {k: v for k, v in general.items() if k not in ("eval_interval", "save_interval")}
    agent = PPO(pf=pf, vf=vf, env=env, replay_buffer=buf, collector=col, logger=_Log(), device=dev, save_dir=None,
                **cfg["ppo"], **general)
    agent.current_epoch = 0
    want = "_FusedPPO" if fused_update else "_GenericPPO"
    assert type(agent.engine()).__name__ == want and bool(col._wide) == fused_rollout, "route not taken"
    for name in SWITCHES:
        os.environ.pop(name, None)
    return col, agent


def stats(v):
    v = np.asarray(v)
    return {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, "config", "ppo_synth_halfcheetah_w128.json")) as f:
        cfg = json.load(f)
    out = {"envs": a.envs, "steps": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "minibatches": cfg["ppo"]["opt_epochs"] * (cfg["collector"]["epoch_frames"] // cfg["general_setting"]["batch_size"])}
    # the update alone: both engines behind the one-launch wide rollout; whole iterations: both switches against neither
    for what, pairs in (("update", {"generic": (False, True), "fused": (True, True)}),
                        ("iteration", {"generic": (False, False), "fused": (True, True)})):
        runs = {k: make(u, r, cfg, a.envs, a.steps, dev) for k, (u, r) in pairs.items()}
        samples = {k: [] for k in runs}
        for col, agent in runs.values():
            col.train_one_epoch()
        for r in range(a.warmup + a.reps):
            for k, (col, agent) in runs.items():                                 # alternating: both see the same machine
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if what == "iteration":
                    col.train_one_epoch()
                agent.update_per_epoch()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    samples[k].append((time.perf_counter() - t0) * 1e3)
        out[what] = {k: stats(v) for k, v in samples.items()}
        out[what]["generic_over_fused"] = round(out[what]["generic"]["median_ms"] / out[what]["fused"]["median_ms"], 2)
        del runs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
