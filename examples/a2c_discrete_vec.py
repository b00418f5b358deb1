"""A2C with a categorical policy on a vectorised discrete-action env: the wiring of examples/a2c_continuous_vec.py with
`CategoricalDisPolicy` in place of the Gaussian policy; the `a2c` section of the config is A2C's keyword arguments:

    python examples/a2c_discrete_vec.py --config config/ppo_synth_discrete.json --vec_env_nums 2048 --seed 0 --overwrite

With TRL_CAT_FUSED_ROLLOUT=1 TRL_CAT_FUSED_UPDATE=1 (both opt-in) the synthetic config's 64 x 64 nets are collected by the
one-launch rollout and updated by the fused two-launch sequence instead of the per-step collector and the generic engine.

`--optimizer {adam,rmsprop,sgd}` (default adam) with `--optimizer_info '{"alpha": 0.95}'` (a JSON object of keyword arguments)
chooses the optimiser class; A2C constructs it with eps = 1e-5 as the reference does, so `sgd` fails in torch's constructor.
RMSprop -- the optimiser A2C was published with -- steps on the generic engine.
"""
import os.path as osp
import random
import sys

import numpy as np
import torch

sys.path.append(osp.join(osp.dirname(osp.abspath(__file__)), ".."))
import torchrl.networks as networks                       # noqa: E402
import torchrl.policies as policies                       # noqa: E402
from torchrl.algo import A2C                              # noqa: E402
from torchrl.collector.on_policy import VecOnPolicyCollector  # noqa: E402
from torchrl.env import get_vec_env                       # noqa: E402
from torchrl.replay_buffers.on_policy import OnPolicyReplayBuffer  # noqa: E402
from torchrl.utils import Logger, get_args, get_params    # noqa: E402
from torchrl.utils.args import optimizer_kwargs           # noqa: E402


def main():
    args = get_args()
    params = get_params(args.config)
    device = torch.device("cuda:{}".format(args.device))
    torch.cuda.set_device(device)                        # envs / replay buffers allocate on the current device

    env = get_vec_env(params["env_name"], params["env"], args.vec_env_nums)
    eval_env = get_vec_env(params["env_name"], params["env"], args.vec_env_nums)
    env.seed(args.seed)
    eval_env.seed(args.seed + 1)
    for seed_fn in (torch.manual_seed, np.random.seed, random.seed):
        seed_fn(args.seed)

    name = args.id if args.id is not None else osp.splitext(osp.basename(args.config))[0]
    logger = Logger(name, params['env_name'], args.seed, params, args.log_dir, args.overwrite)

    replay_buffer = OnPolicyReplayBuffer(env_nums=args.vec_env_nums,
                                         max_replay_buffer_size=int(params['replay_buffer']['size']),
                                         time_limit_filter=params['replay_buffer']['time_limit_filter'])
    net = dict(params['net'], base_type=networks.MLPBase, activation_func=torch.nn.Tanh)
    pf = policies.CategoricalDisPolicy(input_shape=env.observation_space.shape[0], output_shape=env.action_space.n, **net)
    vf = networks.Net(input_shape=env.observation_space.shape, output_shape=1, **net)
    # a categorical policy samples from the device Philox stream: noise_mode "device" is the only one
    collector = VecOnPolicyCollector(vf, env=env, eval_env=eval_env, pf=pf, replay_buffer=replay_buffer,
                                     device=device, train_render=False, noise_mode="device", **params["collector"])
    general = dict(params['general_setting'], env=collector.env, replay_buffer=replay_buffer, logger=logger,
                   device=device, collector=collector, save_dir=osp.join(logger.work_dir, "model"))
    A2C(pf=pf, vf=vf, **dict(params["a2c"], **optimizer_kwargs(args, with_info=False)), **general).train()


if __name__ == "__main__":
    main()
