"""One rollout of config/ppo_synth_halfcheetah_ln.json's networks (`add_ln=True` two-layer MLPs, Tanh, 17 -> 6, device noise) at
2048 envs x 128 steps on both routes, at the config's width (128) and the same nets at 256 (`--widths`), one MI355X:

  per_step   the collector as it is without TRL_WIDE_LN_FUSED_ROLLOUT -- the per-step launch sequence, replayed as a HIP graph
             from its third visit on: what the parent commit does;
  fused      TRL_WIDE_LN_FUSED_ROLLOUT=1: trl_rollout_synth_wide_ln_f32, the persistent kernel + the value pass.

Both collectors of a width live in ONE process and alternate after `--warmup` rounds; a sample is a host clock around
`train_one_epoch()` + a device synchronise; medians and the spread (min, max) over `--reps` samples.  Prints one JSON line per
width.

    python tools/time_wide_layernorm_rollout.py [--envs 2048] [--steps 128] [--widths 128 256] [--reps 30] [--warmup 6]
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
SWITCH = "TRL_WIDE_LN_FUSED_ROLLOUT"


def make(fused, cfg, N, T, width, dev):
    from torchrl_amd import networks, policies
    from torchrl_amd.collector.on_policy import VecOnPolicyCollector
    from torchrl_amd.env import get_vec_env
    from torchrl_amd.replay_buffers.on_policy import OnPolicyReplayBuffer
    torch.manual_seed(0)
    env, eval_env = (get_vec_env(cfg["env_name"], cfg["env"], N, device=dev) for _ in range(2))
    env.seed(0)
    net = dict(cfg["net"], hidden_shapes=[width, width], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    assert net["add_ln"], "the config's networks carry the LayerNorm"
    pf = policies.GuassianContPolicyBasicBias(input_shape=env.obs_dim, output_shape=env.act_dim, **cfg["policy"], **net).to(dev)
    vf = networks.Net(input_shape=(env.obs_dim,), output_shape=1, **net).to(dev)
    buf = OnPolicyReplayBuffer(N * T, env_nums=N, time_limit_filter=True)
    if fused:
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)
    col = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=buf, device=dev, train_render=False,
                               epoch_frames=N * T, max_episode_frames=cfg["collector"]["max_episode_frames"], eval_episodes=1,
                               noise_mode=cfg["collector"]["noise_mode"])
    os.environ.pop(SWITCH, None)
    assert (col._spec is not None) == fused, "the collector did not take the %s route" % ("fused" if fused else "per-step")
    return col


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--widths", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with open(os.path.join(ROOT, "config", "ppo_synth_halfcheetah_ln.json")) as f:
        cfg = json.load(f)
    for width in a.widths:
        cols = {"per_step": make(False, cfg, a.envs, a.steps, width, dev), "fused": make(True, cfg, a.envs, a.steps, width, dev)}
        samples = {k: [] for k in cols}
        for r in range(a.warmup + a.reps):
            for k, col in cols.items():                                          # alternating: both see the same machine
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                col.train_one_epoch()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    samples[k].append((time.perf_counter() - t0) * 1e3)
        out = {"envs": a.envs, "steps": a.steps, "width": width, "reps": a.reps,
               "device": torch.cuda.get_device_name(0), "per_step_graph": cols["per_step"]._roll_graph["graph"] is not None}
        for k, v in samples.items():
            v = np.asarray(v)
            out[k] = {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(v.min()), 4), "max_ms": round(float(v.max()), 4)}
        out["per_step_over_fused"] = round(out["per_step"]["median_ms"] / out["fused"]["median_ms"], 2)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
