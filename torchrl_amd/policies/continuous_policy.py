"""Gaussian policies with the reference's API
(torchrl/policies/continuous_policy.py:77-188).

`GuassianContPolicyBasicBias` (PPO/A2C: MLP mean + state-independent `logstd`
parameter initialised to log(log_init), clamped to [-20, 2]) is the policy of
the benchmark path.  Inside the fused collector / PPO kernels its parameters are
read from `flat_params()` (MLP2 block + logstd tail); the methods below keep the
reference protocol (`explore` / `update` / `eval_act` dicts) for callers that
use the policy directly: the mean comes from the HIP MLP kernel, log-probs from
trl_gauss_logp_f32.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.distributions import Normal

from .. import _C
from .. import networks
from .distribution import TanhNormal

LOG_SIG_MAX = 2
LOG_SIG_MIN = -20


class GuassianContPolicyBase:
    def eval_act(self, x):
        return self.torch_eval_act(x).squeeze(0).cpu().numpy()

    def torch_eval_act(self, x):
        with torch.no_grad():
            mean, _, _ = self.forward(x)
        return (torch.tanh(mean) if self.tanh_action else mean).detach()

    def _dist(self, mean, std):
        return TanhNormal(mean, std) if self.tanh_action else Normal(mean, std)

    def explore(self, x, return_log_probs=False, return_pre_tanh=False):
        """The reference's direct-call protocol (continuous_policy.py:92-131) on torch.distributions; the collectors do
        not come through here (their sampling is in the rollout / rsample kernels)."""
        mean, std, log_std = self.forward(x)
        if mean.is_cuda:
            _C.note_eager(type(self).__name__ + ".explore", "torch.distributions sampling")
        dis = self._dist(mean, std)
        out = {"mean": mean, "log_std": log_std, "std": std,
               "ent": dis.entropy().sum(-1, keepdim=True)}
        if return_log_probs:
            if self.tanh_action:
                action, z = dis.rsample(return_pretanh_value=True)
                log_prob = dis.log_prob(action, pre_tanh_value=z)
                out["pre_tanh"] = z.squeeze(0)
            else:
                action = dis.sample()
                log_prob = dis.log_prob(action)
            out["log_prob"] = log_prob.sum(dim=-1, keepdim=True)
        elif self.tanh_action:
            if return_pre_tanh:
                action, z = dis.rsample(return_pretanh_value=True)
                out["pre_tanh"] = z.squeeze(0)
            action = dis.rsample(return_pretanh_value=False)
        else:
            action = dis.sample()
        out["action"] = action.squeeze(0)
        return out

    def update(self, obs, actions):
        mean, std, log_std = self.forward(obs)
        if mean.is_cuda and not (torch.is_grad_enabled() and mean.requires_grad):
            ls = log_std if log_std.dim() == 1 else None
            if ls is not None:
                lp = _C.gauss_logp(mean.contiguous(), actions.float().contiguous(), ls.float().contiguous(),
                                   self.tanh_action).unsqueeze(-1)
            else:
                _C.note_eager(type(self).__name__ + ".update", "state-dependent std has no log-prob kernel")
                lp = self._dist(mean, std).log_prob(actions).sum(-1, keepdim=True)
        else:
            if mean.is_cuda:
                _C.note_eager(type(self).__name__ + ".update", "autograd is on")
            lp = self._dist(mean, std).log_prob(actions).sum(-1, keepdim=True)
        return {"mean": mean, "dis": Normal(mean, std), "log_std": log_std, "std": std,
                "log_prob": lp, "ent": Normal(mean, std).entropy().sum(-1, keepdim=True)}


def is_state_std(pf):
    """Is `pf` a state-dependent-std Gaussian policy for the on-policy kernels (k_gauss_sd.hip): continuous, no `logstd`
    parameter, and a head of even width that emits [mean | log_std]?  The one test both the on-policy collector and the
    PPO / A2C engine use.  (Deterministic policies are continuous without a `logstd` too; they have no `explore`-time
    distribution and are told apart by what they lack: the Gaussian protocol of GuassianContPolicyBase.)"""
    if getattr(pf, "continuous", None) is not True or hasattr(pf, "logstd") or not isinstance(pf, GuassianContPolicyBase):
        return False
    from .. import ops
    return int(ops.linear_layers(pf)[-1][0].shape[0]) % 2 == 0


# The policy heads of the on-policy kernels (csrc/trl_head.h): a diagonal Gaussian with a free `logstd`
# (GuassianContPolicyBasicBias), a categorical head (CategoricalDisPolicy) and a state-dependent-std Gaussian (GuassianContPolicy)
HEAD_GAUSS, HEAD_CAT, HEAD_SD = 0, 1, 2
HEAD_TAG = ("", "cat_", "sd_")                        # in the entry points' names: trl_ppo_<tag>..., trl_rollout_<tag>supported
HEAD_NAME = ("Gaussian", "categorical", "state-dependent-std")


def head_kind(pf, refuse=None):
    """Which head `pf` has -- the one place the collector, the PPO / A2C engines, TRPO and V-MPO ask.  A network with none of
    them (a value network, a deterministic or a Q policy): TrlError(`refuse`) when the caller refuses it, None otherwise."""
    if getattr(pf, "continuous", True) is False and hasattr(pf, "logits"):
        return HEAD_CAT
    if is_state_std(pf):
        return HEAD_SD
    if hasattr(pf, "logstd"):
        return HEAD_GAUSS
    if refuse is not None:
        raise _C.TrlError(refuse)
    return None


class GuassianContPolicy(networks.Net, GuassianContPolicyBase):
    """State-dependent std (SAC): head emits [mean | log_std] (continuous_policy.py:156-170)."""

    def __init__(self, tanh_action=False, **kwargs):
        super().__init__(**kwargs)
        self.continuous = True
        self.tanh_action = tanh_action

    def forward(self, x):
        mean, log_std = super().forward(x).chunk(2, dim=-1)
        log_std = torch.clamp(log_std, LOG_SIG_MIN, LOG_SIG_MAX)
        return mean, torch.exp(log_std), log_std

    # On the GPU without autograd the protocol below runs on k_gauss_sd.hip: the head (N, 2A) = [mean | raw log_std] comes
    # from the network's forward kernels, actions / log pi / entropy from trl_gauss_sd_explore_f32 / trl_gauss_sd_logp_f32
    # (the kernels PPO / A2C and the on-policy collector use for this head).  SAC does not come through here: TwinSACQ and
    # the off-policy collector read `forward` and sample in their own rsample kernels.
    def _head(self, x):
        """The raw head (N, 2A) when the kernels apply: a CUDA input of rank <= 2 and no autograd graph wanted."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() <= 2):
            return None
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return None
        with torch.no_grad():
            head = networks.Net.forward(self, x if x.dim() == 2 else x.unsqueeze(0))
        return head.float().contiguous() if head.shape[-1] % 2 == 0 and head.shape[-1] <= 64 else None

    @staticmethod
    def _parts(head):
        mean, log_std = head.chunk(2, dim=-1)
        log_std = torch.clamp(log_std, LOG_SIG_MIN, LOG_SIG_MAX)
        return mean, torch.exp(log_std), log_std

    def update(self, obs, actions):
        head = self._head(obs)
        if head is None or obs.dim() != 2:
            return super().update(obs, actions)
        mean, std, log_std = self._parts(head)
        acts = actions.to(device=head.device, dtype=torch.float32).reshape(head.shape[0], -1).contiguous()
        lp, ent = _C.gauss_sd_logp(head, acts, self.tanh_action, want_ent=True)
        return {"mean": mean, "dis": Normal(mean, std), "log_std": log_std, "std": std,
                "log_prob": lp.unsqueeze(-1), "ent": ent.unsqueeze(-1)}

    def explore(self, x, return_log_probs=False, return_pre_tanh=False):
        """The base class's dict, key for key (`pre_tanh` of a tanh policy included), from the kernels.  One difference for
        direct callers: the noise is one torch.randn block on the device, not Normal.sample / rsample's own draw."""
        head = self._head(x)
        if head is None:
            return super().explore(x, return_log_probs=return_log_probs, return_pre_tanh=return_pre_tanh)
        mean, std, log_std = self._parts(head)
        N, A = head.shape[0], head.shape[1] // 2
        eps = torch.randn(N, A, device=head.device)
        act, lp = _C.gauss_sd_explore(head, eps, self.tanh_action)
        _, ent = _C.gauss_sd_logp(head, act, self.tanh_action, want_ent=True)
        squeeze = (lambda t: t.squeeze(0)) if x.dim() == 1 else (lambda t: t)
        out = {"mean": squeeze(mean), "log_std": squeeze(log_std), "std": squeeze(std), "ent": squeeze(ent.unsqueeze(-1)),
               "action": squeeze(act).squeeze(0)}
        if return_log_probs:
            out["log_prob"] = squeeze(lp.unsqueeze(-1))
        if self.tanh_action and (return_log_probs or return_pre_tanh):
            # z = mean + std * eps as the kernel forms it before its tanh: the same launch without the tanh, the same bits
            z, _ = _C.gauss_sd_explore(head, eps, False)
            out["pre_tanh"] = squeeze(z).squeeze(0)
        return out

    def torch_eval_act(self, x):
        head = self._head(x)
        if head is None:
            return super().torch_eval_act(x)
        act, _ = _C.gauss_sd_explore(head, None, self.tanh_action)
        return act if x.dim() == 2 else act.squeeze(0)


class GuassianContPolicyBasicBias(networks.Net, GuassianContPolicyBase):
    def __init__(self, output_shape, tanh_action=False, log_init=0.125, **kwargs):
        super().__init__(output_shape=output_shape, **kwargs)
        self.continuous = True
        self.logstd = nn.Parameter(torch.ones(output_shape) * np.log(log_init))
        self.tanh_action = tanh_action

    def _extra_flat_params(self):
        return [self.logstd]

    def forward(self, x):
        mean = super().forward(x)
        logstd = torch.clamp(self.logstd, LOG_SIG_MIN, LOG_SIG_MAX)
        std = torch.exp(logstd).unsqueeze(0).expand_as(mean)
        return mean, std, logstd


class DetContPolicy(networks.Net):
    """Deterministic policy (torchrl/policies/continuous_policy.py:28-47): action = [tanh](mlp(x))."""

    def __init__(self, tanh_action=False, **kwargs):
        super().__init__(**kwargs)
        self.continuous = True
        self.tanh_action = tanh_action

    def forward(self, x):
        out = super().forward(x)
        return torch.tanh(out) if self.tanh_action else out

    def eval_act(self, x):
        with torch.no_grad():
            return self.forward(x).squeeze(0).detach().cpu().numpy()

    def explore(self, x):
        return {"action": self.forward(x).squeeze(0)}


class FixGuassianContPolicy(networks.Net):
    def __init__(self, norm_std_explore, tanh_action=False, **kwargs):
        super().__init__(**kwargs)
        self.continuous = True
        self.tanh_action = tanh_action
        self.norm_std_explore = norm_std_explore

    def forward(self, x):
        out = super().forward(x)
        return torch.tanh(out) if self.tanh_action else out

    def eval_act(self, x):
        with torch.no_grad():
            return self.forward(x).squeeze(0).detach().cpu().numpy()

    def explore(self, x):
        action = self.forward(x).squeeze(0)
        noise = Normal(0, self.norm_std_explore).sample(action.shape).to(action.device)
        return {"action": action + noise}


class UniformPolicyContinuous(nn.Module):
    def __init__(self, action_shape):
        super().__init__()
        self.continuous = True
        self.action_shape = action_shape

    def forward(self, x):
        return torch.Tensor(np.random.uniform(-1., 1., self.action_shape))

    def explore(self, x):
        return {"action": self.forward(x)}
