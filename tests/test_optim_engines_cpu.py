"""The algorithms that keep stepping with Adam alone still say so for RMSprop / SGD, before any device is touched; A2C
and PPO build their optimisers with eps = 1e-5 as the reference does, so SGD fails in torch's own constructor.  No GPU."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def _off_policy(cls, nets, **kw):
    """An off-policy agent without a value network (test_sac_v_cpu's `_agent` without `vlr`)."""
    from oracle.synth_env import SynthVecEnvCPU

    class Stub:
        epoch_frames = 0
    return cls(**nets, plr=3e-4, qlr=3e-4, env=SynthVecEnvCPU(4), replay_buffer=None, collector=Stub(), logger=None,
               device=torch.device("cpu"), save_dir=None, batch_size=8, **kw)


def test_adam_only_algorithms_still_refuse():
    import test_boot_dqn_cpu as boot
    import test_reinforce_cpu as rf
    import test_sac_v_cpu as sv
    import test_vmpo_trpo_heads_cpu as vt
    from torchrl_amd import _C
    from torchrl_amd.algo import SAC, TRPO, VMPO, TwinSAC, TwinSACQ
    with pytest.raises(_C.TrlError, match="Adam only"):
        rf._agent(rf._policies()[0], optimizer_class=torch.optim.RMSprop).engine()
    with pytest.raises(_C.TrlError, match="Adam only"):
        boot.make_algo(optimizer_class=torch.optim.RMSprop)[0].update({})
    for kind in ("gauss", "cat", "sd"):
        with pytest.raises(_C.TrlError, match="implements torch.optim.Adam only"):
            vt._agent(VMPO, *vt._nets(kind), optimizer_class=torch.optim.RMSprop)
        with pytest.raises(_C.TrlError, match="implements torch.optim.Adam only"):
            vt._agent(TRPO, *vt._nets(kind), optimizer_class=torch.optim.RMSprop, **vt.TRPO_KW)
    for cls, twin in ((SAC, False), (TwinSAC, True)):
        with pytest.raises(_C.TrlError, match="torch.optim.Adam only, got RMSprop"):
            sv._agent(cls, sv._nets(twin=twin), optimizer_class=torch.optim.RMSprop)
    nets = sv._nets(twin=True)
    nets.pop("vf")
    with pytest.raises(_C.TrlError, match="implements torch.optim.Adam only"):
        _off_policy(TwinSACQ, nets, optimizer_class=torch.optim.SGD).engine()


def test_a2c_and_ppo_pass_eps_to_the_constructor_as_the_reference_does():
    import test_vmpo_trpo_heads_cpu as vt
    from torchrl_amd.algo import A2C, PPO
    for cls in (A2C, PPO):
        with pytest.raises(TypeError, match="eps"):
            vt._agent(cls, *vt._nets("gauss"), optimizer_class=torch.optim.SGD)
        agent = vt._agent(cls, *vt._nets("gauss"), optimizer_class=torch.optim.RMSprop)
        assert type(agent.pf_optimizer) is torch.optim.RMSprop and agent.pf_optimizer.param_groups[0]["eps"] == 1e-5


def test_dqn_ddpg_td3_construct_with_rmsprop_and_sgd():
    """What used to be refused: the constructors were never the obstacle, `engine()` was (it needs a GPU: see the GPU file)."""
    import functools
    import test_sac_v_cpu as sv
    from torchrl_amd.algo import DDPG, TD3
    nets = sv._nets(twin=True)
    sgd = functools.partial(torch.optim.SGD, momentum=0.9)
    a = _off_policy(TD3, dict(pf=nets["pf"], qf1=nets["qf1"], qf2=nets["qf2"]), optimizer_class=sgd)
    assert type(a.qf2_optimizer) is torch.optim.SGD and a.pf_optimizer.param_groups[0]["momentum"] == 0.9
    b = _off_policy(DDPG, dict(pf=nets["pf"], qf=nets["qf1"]), optimizer_class=torch.optim.RMSprop)
    assert type(b.qf_optimizer) is torch.optim.RMSprop
