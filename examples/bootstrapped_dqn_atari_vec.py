"""Bootstrapped DQN on pixel envs -- the wiring of examples/dqn_atari_vec.py (conv trunk over uint8 frame stacks,
VecCollector, BaseReplayBuffer) with a `BootstrappedNet` of K heads over the conv feature and the
`BootstrappedDQNDiscretePolicy`: the net (16/8/4 -> 32/4/2 -> 64/3/1 convs, heads 3136 -> 512 -> A), K = 10, p = 0.5,
RMSprop(alpha 0.95, eps 0.01) and the hard target copy of the reference's config/bootstrapped_dqn.json.  Conv trunks,
pixel envs and RMSprop under Bootstrapped DQN are opt-in: this script sets TRL_BOOT_CONV=1 for itself.  The on-GPU synthetic
Atari-shaped env, or the host "catch" game (env on the host, frame stacks kept on the device, everything else on the GPU
kernels):

    python examples/bootstrapped_dqn_atari_vec.py --config config/bootstrapped_dqn_synth_atari.json --vec_env_nums 32 --overwrite
    python examples/bootstrapped_dqn_atari_vec.py --config config/bootstrapped_dqn_catch_host.json --vec_env_nums 16 --seed 0 --overwrite
"""
import os
import os.path as osp
import random
import sys

import numpy as np
import torch

os.environ.setdefault("TRL_BOOT_CONV", "1")
sys.path.append(osp.join(osp.dirname(osp.abspath(__file__)), ".."))
import torchrl.networks as networks                       # noqa: E402
import torchrl.policies as policies                       # noqa: E402
from torchrl.algo import BootstrappedDQN                  # noqa: E402
from torchrl.collector import VecCollector                # noqa: E402
from torchrl.env import get_vec_env                       # noqa: E402
from torchrl.replay_buffers import BaseReplayBuffer       # noqa: E402
from torchrl.utils import Logger, get_args, get_params    # noqa: E402


def main():
    args = get_args()
    params = get_params(args.config)
    device = torch.device("cuda:{}".format(args.device))
    torch.cuda.set_device(device)                        # envs / replay buffers allocate on the current device
    n = args.vec_env_nums
    env = get_vec_env(params["env_name"], params["env"], n)
    eval_env = get_vec_env(params["env_name"], params["env"], n)
    env.seed(args.seed)
    eval_env.seed(args.seed + 1)
    for seed_fn in (torch.manual_seed, np.random.seed, random.seed):
        seed_fn(args.seed)
    name = args.id if args.id is not None else osp.splitext(osp.basename(args.config))[0]
    logger = Logger(name, params['env_name'], args.seed, params, args.log_dir, args.overwrite)
    replay_buffer = BaseReplayBuffer(env_nums=n, max_replay_buffer_size=int(params['replay_buffer']['size']),
                                     time_limit_filter=params['replay_buffer']['time_limit_filter'])
    algo = dict(params["bootstrapped dqn"])
    heads = int(algo["head_num"])
    if "optimizer_class" in algo:
        algo["optimizer_class"] = getattr(torch.optim, algo["optimizer_class"])
    net = dict(params['net'], base_type=networks.CNNBase, activation_func=torch.nn.ReLU)
    shape = tuple(env.observation_space.shape)
    if len(shape) == 2:                                  # single (H, W) host frames: the bridge stacks four of them
        shape = (4,) + shape
    qf = networks.BootstrappedNet(input_shape=shape, output_shape=env.action_space.n, head_num=heads, **net)
    pf = policies.BootstrappedDQNDiscretePolicy(qf, head_num=heads, action_shape=env.action_space.n)
    collector = VecCollector(env=env, pf=pf, eval_env=eval_env, replay_buffer=replay_buffer, device=device,
                             train_render=False, **params["collector"])
    general = dict(params['general_setting'], env=collector.env, replay_buffer=replay_buffer, logger=logger, device=device,
                   collector=collector, save_dir=osp.join(logger.work_dir, "model"))
    BootstrappedDQN(pf=pf, qf=qf, **algo, **general).train()


if __name__ == "__main__":
    main()
