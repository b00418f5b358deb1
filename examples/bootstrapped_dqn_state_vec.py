"""Bootstrapped DQN on state-vector envs -- the wiring of examples/dqn_state_vec.py (MLP trunk, VecCollector,
BaseReplayBuffer) with a `BootstrappedNet` of K heads and the `BootstrappedDQNDiscretePolicy`: every env plays one head
per episode, every stored transition carries a Bernoulli(p) mask per head, evaluation acts on the ensemble vote.
K = 10 and p = 0.5 as in the reference's config/bootstrapped_dqn.json.  Host cart-pole (env physics on the host,
everything else on the GPU kernels) or the on-GPU synthetic id:

    python examples/bootstrapped_dqn_state_vec.py --config config/bootstrapped_dqn_cartpole_host.json --vec_env_nums 8 --seed 0 --overwrite
    python examples/bootstrapped_dqn_state_vec.py --config config/bootstrapped_dqn_synth_discrete.json --vec_env_nums 256 --seed 0 --overwrite
"""
import os.path as osp
import random
import sys

import numpy as np
import torch

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
    heads = int(params["bootstrapped dqn"]["head_num"])
    net = dict(params['net'], base_type=networks.MLPBase, activation_func=torch.nn.ReLU)
    qf = networks.BootstrappedNet(input_shape=env.observation_space.shape, output_shape=env.action_space.n,
                                  head_num=heads, **net)
    pf = policies.BootstrappedDQNDiscretePolicy(qf, head_num=heads, action_shape=env.action_space.n)
    collector = VecCollector(env=env, pf=pf, eval_env=eval_env, replay_buffer=replay_buffer, device=device,
                             train_render=False, **params["collector"])
    general = dict(params['general_setting'], env=collector.env, replay_buffer=replay_buffer, logger=logger, device=device,
                   collector=collector, save_dir=osp.join(logger.work_dir, "model"))
    BootstrappedDQN(pf=pf, qf=qf, **params["bootstrapped dqn"], **general).train()


if __name__ == "__main__":
    main()
