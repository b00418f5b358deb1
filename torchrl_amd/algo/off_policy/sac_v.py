"""SAC and TwinSAC, the soft actor-critics with a value network, on the HIP path (reference:
torchrl/algo/off_policy/sac.py:10-231, twin_sac.py:10-254).

Beside the policy and one (`SAC`) or two (`TwinSAC`) critics they train V(s) and keep its Polyak target; `update(batch)`
keeps the reference's order -- one policy sample, temperature step (alpha is re-read AFTER it), critic regression(s)
against r + (1 - d) gamma V'(s'), V regression against min Q(s, a~) - alpha log pi, policy loss through min Q(s, a~),
optimiser steps pf -> qf(1, 2) -> vf, target update of V only -- as a fixed launch sequence with an explicit chain rule:
  sample + critic inputs ... trl_sacv_samples_f32 (one launch; device noise: counter u + 1 of update u)
  losses, dQ, dV ........... trl_sacv_losses_f32 (one launch; temperature step and moment fold ride along on one rank)
  everything else .......... the launches of twin_sac_q.py: grouped dense layers, trl_sac_policy_grad_f32 with one or two
                             critics, fold / clip / Adam on one flat [pf | qf1 | (qf2) | vf] buffer, Polyak on its vf tail
The engine derives from twin_sac_q._FusedSAC: graph cache, statistics ring, deferred and whole-epoch paths are that class.
policy_loss.backward() in the reference also deposits gradients in the critics that their zero_grad() discards; only
d/d(action) is propagated here.  `assert v_target == v_pred` of the reference (sac.py:130, twin_sac.py:142; it raises
for every batch of more than one row) is taken as the shape check it evidently stands for: both are (B, 1) here by
construction.

Under TRL_OFFPOLICY_LN=1 `add_ln=True` networks run on the grouped LayerNorm launches (ops.mlp_forward_group / mlp_backward_group): the policy,
the critics and V may each carry norms or not; twin critics must agree, and V's target is V's copy.

Not built: reparameterization=False, optimisers other than Adam, several ranks.
"""
import copy

import numpy as np
import torch
import torch.optim as optim

from ... import _C, dist, ops
from .off_rl_algo import OffRLAlgo
from .twin_sac_q import _FusedSAC, _SoftSurface


class _ValueSAC(_SoftSurface, OffRLAlgo):
    """What SAC and TwinSAC share: `_setup` behind their reference-shaped constructors."""

    def _setup(self, pf, vf, critics, plr, vlr, qlr, optimizer_class, policy_std_reg_weight, policy_mean_reg_weight,
               reparameterization, automatic_entropy_tuning, target_entropy, noise_mode, kwargs):
        self.optimizer_class, self.reparameterization = optimizer_class, reparameterization
        self._critic_names = [name for name, _ in critics]
        self.pf, self.vf = pf, vf
        for name, net in critics:
            setattr(self, name, net)
        self._refuse()                                                   # before anything looks at a device
        if noise_mode not in ("host", "device"):
            raise ValueError("noise_mode must be 'host' or 'device'")
        OffRLAlgo.__init__(self, **kwargs)
        self.target_vf = copy.deepcopy(vf)
        self.to(self.device)
        self.plr, self.vlr, self.qlr = plr, vlr, qlr
        for name, net in critics:
            setattr(self, name + "_optimizer", optimizer_class(net.parameters(), lr=qlr))
        self.vf_optimizer = optimizer_class(vf.parameters(), lr=vlr)
        self.pf_optimizer = optimizer_class(pf.parameters(), lr=plr)
        self.automatic_entropy_tuning = automatic_entropy_tuning
        self.target_entropy = target_entropy if target_entropy else -float(np.prod(self.env.action_space.shape))
        self.policy_std_reg_weight, self.policy_mean_reg_weight = policy_std_reg_weight, policy_mean_reg_weight
        self.noise_mode = noise_mode
        self._engine = None

    def _refuse(self):
        name = type(self).__name__
        if not self.reparameterization:
            raise NotImplementedError("%s(reparameterization=False): the likelihood-ratio policy loss is not built; the HIP "
                                      "path carries the reparameterised loss mean(alpha log pi - Q) only" % name)
        if self.optimizer_class is not optim.Adam:
            raise _C.TrlError("%s: the fused SAC step implements torch.optim.Adam only, got %s"
                              % (name, getattr(self.optimizer_class, "__name__", self.optimizer_class)))
        if dist.collectives_active():
            raise _C.TrlError("%s runs on one rank: the exchange of gradients and statistics between several ranks is not "
                              "built for the value-network soft actor-critics (TwinSACQ has it)" % name)
        for net in self._critics() + [self.pf, self.vf]:
            ops.offpolicy_layers(net)                   # Tanh / ReLU MLPs (with LayerNorm: under TRL_OFFPOLICY_LN=1), or TrlError

    def _critics(self):
        return [getattr(self, name) for name in self._critic_names]

    @property
    def networks(self):
        return [self.pf] + self._critics() + [self.vf, self.target_vf]

    @property
    def snapshot_networks(self):
        return [["pf", self.pf]] + [[name, getattr(self, name)] for name in self._critic_names] + [["vf", self.vf]]

    @property
    def target_networks(self):
        return [(self.vf, self.target_vf)]

    def engine(self):
        if self._engine is None:
            self._refuse()                                               # (a process group may have come up since)
        return super().engine()


class SAC(_ValueSAC):
    def __init__(self, pf, vf, qf, plr, vlr, qlr, optimizer_class=optim.Adam, policy_std_reg_weight=1e-3,
                 policy_mean_reg_weight=1e-3, reparameterization=True, automatic_entropy_tuning=True,
                 target_entropy=None, noise_mode="host", **kwargs):
        self._setup(pf, vf, [("qf", qf)], plr, vlr, qlr, optimizer_class, policy_std_reg_weight, policy_mean_reg_weight,
                    reparameterization, automatic_entropy_tuning, target_entropy, noise_mode, kwargs)


class TwinSAC(_ValueSAC):
    def __init__(self, pf, vf, qf1, qf2, plr, vlr, qlr, optimizer_class=optim.Adam, policy_std_reg_weight=1e-3,
                 policy_mean_reg_weight=1e-3, reparameterization=True, automatic_entropy_tuning=True,
                 target_entropy=None, noise_mode="host", **kwargs):
        self._setup(pf, vf, [("qf1", qf1), ("qf2", qf2)], plr, vlr, qlr, optimizer_class, policy_std_reg_weight,
                    policy_mean_reg_weight, reparameterization, automatic_entropy_tuning, target_entropy, noise_mode, kwargs)


class _FusedSACV(_FusedSAC):
    N_SUMS = 5                                                          # qf1, qf2, vf, policy, reward
    NOISE = ("eps1",)                                                   # one policy sample per update

    def _roles(self, algo):
        names = algo._critic_names
        return ((algo.pf, *algo._critics(), algo.vf),
                (algo.pf_optimizer, *[getattr(algo, n + "_optimizer") for n in names], algo.vf_optimizer),
                (algo.target_vf,))

    def _names(self, algo):
        names = tuple(algo._critic_names)
        return ("pf",) + names + ("vf",), ("target_vf",), ((names,) if len(names) > 1 else ())

    def _sequence(self, st, soft):
        """The fixed launch sequence of one update on the static inputs (eager, or under graph capture)."""
        algo, A = self.algo, self.A
        obs, acts, nobs, eps = st["obs"], st["acts"], st["next_obs"], st["eps1"]
        rew, term = st["rewards"].view(-1), st["terminals"].view(-1)
        B = int(obs.shape[0])
        ws = self._ws(B)
        pf_l, q_ls, v_l = self.layers[0], self.layers[1:-1], self.layers[-1]
        k = len(q_ls)
        tanh_action = bool(algo.pf.tanh_action)
        # ---- policy head on obs; V(obs) and the target V(next_obs) as one group (the target pass leaves no tape) ----
        head, tape_pf = ops.mlp_forward(pf_l, obs, self.act)
        (v, tv), (tape_v, _) = ops.mlp_forward_group([v_l, self.tlayers[0]], [obs, nobs], self.act, keep=[True, False])
        # the sample and the critic inputs [obs | acts], [obs | new_a]: one launch; temperature step, logged moments and the
        # filing of the statistics ride on the update's own launches exactly as in _FusedSAC._sequence
        ride = self._stats_ride_along(soft)
        if ride and (self._mom_part is None or self._mom_part.shape[0] != (B + 63) // 64):
            self._mom_part = torch.zeros((B + 63) // 64, 12, dtype=torch.float64, device=self.dev)
        new_a, logp, x_sa, x_new = _C.sacv_samples(
            head, eps, obs, acts, tanh_action, philox=(self.step_state, self.noise_seed) if self._inline_noise() else None,
            mom_part=self._mom_part if ride else None)
        if algo.automatic_entropy_tuning and not ride:
            _C.sac_alpha_step(logp, algo.target_entropy, algo.plr, self.alpha_state, self.alpha_out)
        # ---- the critic passes as one group: Q_i(s, a), then Q_i(s, new a) ----
        qs, tapes = ops.mlp_forward_group(q_ls + q_ls, [x_sa] * k + [x_new] * k, self.act)
        q1, q2, q1n, q2n = (qs[0], qs[1], qs[2], qs[3]) if k == 2 else (qs[0], None, qs[1], None)
        alpha = self.alpha_out[0:1]                                      # re-read AFTER the alpha step, as the reference does
        dq1, dq2, dv, dq1n, dq2n = _C.sacv_losses(
            q1, q2, tv, rew, term, v, q1n, q2n, logp, alpha, algo.discount, self.sums,
            alpha_step=(algo.target_entropy, algo.plr, self.alpha_state, self.alpha_out)
            if ride and algo.automatic_entropy_tuning else None,
            fold=(self._mom_part, A, self.mom) if ride else None)
        # ---- backward: the critics on [obs | new_a] down to the action columns (no weight gradients) grouped with their
        # regression passes on [obs | acts] (weight gradients only), then V, then the policy ----
        plan = _C.FoldPlan(ws, defer_gemm=True)
        first = []
        dxs = ops.mlp_backward_group(tapes[k:] + tapes[:k], [dq1n, dq2n][:k] + [dq1, dq2][:k],
                                     grads_list=[None] * k + self.gviews[1:1 + k],
                                     need_input=[True] * k + [False] * k, plan=plan,
                                     input_sink=(lambda *a: first.append(a)) if self._pg_fused else None)
        ops.mlp_backward(tape_v, dv, grads=self.gviews[-1], plan=plan)
        self._policy_backward(first, dxs[:k], head, eps, new_a, tape_pf, alpha, plan)
        self._tail(plan, soft, ride, head, logp)

    def _info(self, raw, B):
        algo = self.algo
        sums, mom, aout, norms = raw                                     # 5 sums, 3 x (mean, std, max, min), (alpha, loss), norms
        names = algo._critic_names
        info = {'Reward_Mean': sums[4] / B}
        if algo.automatic_entropy_tuning:
            info["Alpha"], info["Alpha_loss"] = aout
        info['Training/policy_loss'] = sums[3] / B + self._reg_terms(mom, B)
        info['Training/vf_loss'] = sums[2] / B
        for k, name in enumerate(names):
            info['Training/%s_loss' % name] = sums[k] / B
        if algo.grad_clip is not None:
            for name, norm in zip(["pf"] + names + ["vf"], norms):
                info['Training/%s_grad_norm' % name] = norm
        for k, key in enumerate(("log_std", "log_probs", "mean")):
            info[key + '/mean'], info[key + '/std'], info[key + '/max'], info[key + '/min'] = mom[4 * k:4 * k + 4]
        return info


_ValueSAC._engine_class = _FusedSACV
