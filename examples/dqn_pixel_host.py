"""DQN / QR-DQN on a pixel task stepped in Python -- what the reference's examples/dqn_atari_vec.py exists for (a host env
behind WarpFrame -> FrameStack -> VecEnv) with its config/dqn_pong.json network, on the pure-Python `PyCatch-v0` (no ALE
in the image): the env draws one 84 x 84 uint8 frame per step on the host, `torchrl.env.HostFrameBridge` uploads that one
frame and keeps the 4-stacks on the device, the conv Q-network, the TD / quantile-Huber loss, Adam and the target update
run on the GPU kernels.

    python examples/dqn_pixel_host.py --config config/dqn_catch_host.json --vec_env_nums 16 --seed 0 --overwrite
    python examples/dqn_pixel_host.py --config config/dqn_catch_host.json --vec_env_nums 16 --qrdqn --dedup --overwrite

`--qrdqn`: QR-DQN (the config's "qrdqn" section) instead of DQN; `--dedup`: the frame-deduplicating
MemoryEfficientReplayBuffer instead of BaseReplayBuffer.
"""
import argparse
import os.path as osp
import random
import sys

import numpy as np
import torch

sys.path.append(osp.join(osp.dirname(osp.abspath(__file__)), ".."))
import torchrl.networks as networks                       # noqa: E402
import torchrl.policies as policies                       # noqa: E402
from torchrl.algo import DQN, QRDQN                       # noqa: E402
from torchrl.collector import VecCollector                # noqa: E402
from torchrl.env import get_vec_env                       # noqa: E402
from torchrl.replay_buffers import BaseReplayBuffer, MemoryEfficientReplayBuffer    # noqa: E402
from torchrl.utils import Logger, get_args, get_params    # noqa: E402


def main():
    own = argparse.ArgumentParser(add_help=False)
    for flag in ("--qrdqn", "--dedup"):
        own.add_argument(flag, action="store_true")
    opts, rest = own.parse_known_args()
    args = get_args(rest)
    params = get_params(args.config)
    device = torch.device("cuda:{}".format(args.device))
    torch.cuda.set_device(device)
    n = args.vec_env_nums
    env, eval_env = (get_vec_env(params["env_name"], params["env"], n) for _ in range(2))
    env.seed(args.seed)
    eval_env.seed(args.seed + 1)
    for seed_fn in (torch.manual_seed, np.random.seed, random.seed):
        seed_fn(args.seed)
    name = args.id if args.id is not None else osp.splitext(osp.basename(args.config))[0]
    logger = Logger(name, params['env_name'], args.seed, params, args.log_dir, args.overwrite)
    size = int(params['replay_buffer']['size'])
    if opts.dedup:
        replay_buffer = MemoryEfficientReplayBuffer(size, env_nums=n, time_limit_filter=params['replay_buffer']['time_limit_filter'],
                                                    min_episode_frames=min(int(env._max_episode_steps),
                                                                           int(params["collector"]["max_episode_frames"])))
    else:
        replay_buffer = BaseReplayBuffer(env_nums=n, max_replay_buffer_size=size,
                                         time_limit_filter=params['replay_buffer']['time_limit_filter'])
    quantiles = int(params.get("qrdqn", {}).get("quantile_num", 32)) if opts.qrdqn else 1
    frame_stack = 4 if params["env"].get("frame_stack", False) else 1
    net = dict(params['net'], base_type=networks.CNNBase, activation_func=torch.nn.Tanh)
    qf = networks.Net(input_shape=(frame_stack,) + tuple(env.observation_space.shape[-2:]),
                      output_shape=env.action_space.n * quantiles, **net)
    if opts.qrdqn:
        pf = policies.EpsilonGreedyQRDQNDiscretePolicy(quantile_num=quantiles, qf=qf, action_shape=env.action_space.n,
                                                       **params['policy'])
    else:
        pf = policies.EpsilonGreedyDQNDiscretePolicy(qf=qf, action_shape=env.action_space.n, **params['policy'])
    collector = VecCollector(env=env, pf=pf, eval_env=eval_env, replay_buffer=replay_buffer, device=device,
                             train_render=False, **params["collector"])
    general = dict(params['general_setting'], env=collector.env, replay_buffer=replay_buffer, logger=logger, device=device,
                   collector=collector, save_dir=osp.join(logger.work_dir, "model"))
    try:
        if opts.qrdqn:
            QRDQN(pf=pf, qf=qf, quantile_num=quantiles, **params["dqn"], **general).train()
        else:
            DQN(pf=pf, qf=qf, **params["dqn"], **general).train()
    finally:
        collector.terminate()


if __name__ == "__main__":
    main()
