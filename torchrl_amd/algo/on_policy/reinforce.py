"""REINFORCE (torchrl/algo/on_policy/reinforce.py:7-81): a policy, its one Adam optimiser (torch's default eps 1e-8,
no learning-rate schedule), a vacant critic (`networks.ZeroNet`, V == 0) and plain discounted returns (`gae = False`).

`update(batch)` is L = mean(-log pi(a|s) * adv_normalised) - c_ent * mean(ent), clip_grad_norm_(0.5), one Adam step
(reinforce.py:33-75) -- the policy half of the A2C launch sequence with `loss_mode = TRL_LOSS_REINFORCE`: no value
forward, no value loss, no value reduction, one optimiser group.  `update_per_epoch` keeps OnRLAlgo's single pass of
`one_iteration` minibatches (on_rl_algo.py:35-40), through the row indices on the device-resident buffer.

The engines are algo/on_policy/ppo.py's two, which carry a vacant critic as data (no value parameters, workgroups,
pointers or optimiser group): `_FusedReinforce` (64-wide two-layer shapes of the fused gradient kernel: one all-policy
gradient launch + the policy's fold / clip / Adam launch per minibatch, graph-replayed) and `_GenericReinforce` (any MLP,
`add_ln` included, on the dense-layer kernels), routed by `ppo.make_engine`.  What is REINFORCE's own sits in `_PolicyOnly`:
the all-policy workgroup count, the info dict, and the refusals of a target policy and of a second rank.  With V == 0 the
rollout needs no value pass either: the collector stores zeros (one launch on the fused route, trl_rollout_t.vf_params =
NULL) and `advs == estimate_returns`."""
import math

import numpy as np
import torch
import torch.optim as optim

from ... import _C
from ... import dist
from ...networks import ZeroNet
from .a2c import A2C
from .on_rl_algo import OnRLAlgo
from .ppo import _FusedPPO, _GenericPPO, _HALF_LOG_2PI_PLUS_HALF, make_engine


class Reinforce(OnRLAlgo):
    loss_mode = _C.LOSS_REINFORCE
    sample_key = ("obs", "acts", "advs")

    def __init__(self, pf=None, plr=None, optimizer_class=optim.Adam, entropy_coeff=0.001, **kwargs):
        if pf is None or plr is None:
            raise _C.TrlError("Reinforce without a policy (`pf`, `plr`) is not built: pass the policy network and its "
                              "learning rate (reference: torchrl/algo/on_policy/reinforce.py)")
        super().__init__(**kwargs)
        self.pf = pf
        self.vf = ZeroNet()                                            # a vacant critic keeps the collector's interface
        self.to(self.device)
        self.plr = plr
        self.optimizer_class = optimizer_class
        self.pf_optimizer = optimizer_class(self.pf.parameters(), lr=self.plr)
        self.entropy_coeff = entropy_coeff
        self.gae = False
        self._engine = None

    def engine(self):
        if self._engine is None:
            if self.optimizer_class is not optim.Adam:
                raise _C.TrlError("the Reinforce step implements torch.optim.Adam only")
            if dist.collectives_active() or dist.world_size() > 1:
                raise _C.TrlError(_PolicyOnly.one_rank)
            self._engine = make_engine(self, fused=_FusedReinforce, generic=_GenericReinforce)
        return self._engine

    _run_and_log = A2C._run_and_log

    def update_per_epoch(self):
        self.process_epoch_samples()
        buf = self.replay_buffer
        row_idx = buf.epoch_row_indices(self.batch_size, self.shuffle)      # one pass (on_rl_algo.py:37-40)
        tensors = {"obs": buf._obs, "acts": buf._acts, "advs": buf._advs}
        self._run_and_log(tensors, row_idx, buf.env_nums)

    def update(self, batch):
        self.training_update_num += 1
        dev = self.device
        as_t = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))) \
            .to(device=dev, dtype=torch.float32).contiguous()
        obs, acts = as_t(batch['obs']), as_t(batch['acts'])
        B = obs.shape[0]
        tensors = {"obs": obs.reshape(1, B, -1), "acts": acts.reshape(1, B, -1), "advs": as_t(batch['advs']).reshape(1, B, 1)}
        return self.engine().run(tensors, np.zeros((1, 1), dtype=np.int64), B)[0]

    @property
    def snapshot_networks(self):
        return [("pf", self.pf)]


class _PolicyOnly:
    """What REINFORCE's engines add to ppo.py's, which carry the vacant critic themselves (`P_vf = 0`, `flat` = [pf
    (| logstd)], one optimiser group with the optimiser's own eps -- torch's 1e-8: reinforce.py:25-28 passes none)."""
    one_rank = "Reinforce runs on one rank (several ranks are not built: no cross-rank fold of a policy-only update exists)"

    def _n_wg(self, n_samples):
        """Workgroups of one minibatch's gradient launch, all of them the policy's: one 16-sample tile per wave while the
        chip has room."""
        tiles = (n_samples + 15) // 16
        n_wg = max(1, min(self.max_wg, (tiles + 3) // 4))
        return n_wg, n_wg

    def sync_target_pf(self, in_prologue=False):
        raise _C.TrlError("Reinforce has no target policy")

    def _infos_reinforce(self, raw, info, norms, n):
        """The info dict of Reinforce.update (reinforce.py:42-73), in its order.  `advs/*` are numpy statistics of the
        float64 batch there, so `advs/std` is the POPULATION std (A2C / PPO log torch's unbiased one); `logprob/std` is
        unbiased."""
        c_ent = float(self.algo.entropy_coeff)
        out = []
        for r, i in zip(raw, info):
            adv_var = max((r[1] - r[0] * r[0] / n) / n, 0.0)
            lp_var = max((i[2] - i[1] * i[1] / n) / (n - 1), 0.0)
            ent = i[20] / n if (self.categorical or self.state_std) else self.A * _HALF_LOG_2PI_PLUS_HALF + self.A * i[8]
            out.append({'advs/mean': r[0] / n, 'advs/std': math.sqrt(adv_var), 'advs/max': r[2], 'advs/min': -r[3],
                        'Training/policy_loss': i[0] / n - c_ent * ent, 'ent': ent,
                        'logprob/mean': i[1] / n, 'logprob/std': math.sqrt(lp_var), 'logprob/max': i[3], 'logprob/min': -i[4]})
        return [{k: float(v) for k, v in d.items()} for d in out]


class _FusedReinforce(_PolicyOnly, _FusedPPO):
    """Per minibatch two launches: the all-policy gradient launch (trl_ppo_*minibatch_grad_f32, n_wg_pf == n_wg,
    TRL_LOSS_REINFORCE: no returns, old values, log pi_old or value parameters) and the policy's fold / clip / Adam
    (trl_ppo_*reduce_adam_net_f32, net 0, one optimiser group) -- the joint sequence of `_FusedPPO.run`."""


class _GenericReinforce(_PolicyOnly, _GenericPPO):
    """The minibatch loop for ARBITRARY policy MLPs (`add_ln` included): the layers on the dense-layer kernels, the loss
    half on trl_ppo_generic_losses_f32 / trl_cat_losses_f32 / trl_gauss_sd_losses_f32 in TRL_LOSS_REINFORCE mode (no value
    pointers), clip + Adam on trl_clip_adam_f32 with one group -- `_GenericPPO.run` with empty `vf_layers`."""
