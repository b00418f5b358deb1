"""Plain torch restatement (CPU, float32 or float64) of the state-dependent-std Gaussian kernels
(torchrl_amd/csrc/k_gauss_sd.hip) and of the updates built on them -- test infrastructure, imported by
tests/test_gauss_sd_*.py only.

The head is (B, 2A) = [mean | raw log_std]; ls = clamp(raw, -20, 2), std = exp(ls).  Per element
log pi = -(z - mean)^2 / (2 std^2) - ls - log(2 pi) / 2 [- log(1 - a^2 + 1e-6), z = log((1 + a) / (1 - a)) / 2 for tanh
actions] (torchrl/policies/distribution.py:33-45), entropy = 1/2 + log(2 pi) / 2 + ls.  Gradients come from autograd on the
differentiable objective: torch.clamp passes the gradient on the closed interval, torch.minimum / maximum split a tie
evenly -- the kernels' gate and tie conventions."""
import math

import numpy as np
import torch

from _categorical_ref import MLP, adv_normalize, params_from, LOSS_PPO_CLIP, LOSS_A2C      # noqa: F401

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def parts(head):
    """-> (mean (B, A), ls (B, A) clamped, std (B, A))."""
    mean, raw = head.chunk(2, dim=-1)
    ls = raw.clamp(-20.0, 2.0)
    return mean, ls, torch.exp(ls)


def explore(head, eps, tanh):
    """-> (act (B, A), log pi(act) (B,)); eps None: the deterministic action [tanh](mean)."""
    mean, ls, std = parts(head)
    z = mean if eps is None else mean + std * eps
    act = torch.tanh(z) if tanh else z
    return act, logp(head, act, tanh)[0]


def logp(head, acts, tanh):
    """-> (log pi (B,), entropy (B,))."""
    mean, ls, std = parts(head)
    pre, corr = acts, 0.0
    if tanh:
        pre = 0.5 * torch.log((1.0 + acts) / (1.0 - acts))
        corr = torch.log(1.0 - acts * acts + 1e-6)
    zc = pre - mean
    terms = -(zc * zc) / (2.0 * std * std) - ls - HALF_LOG_2PI - corr
    return terms.sum(-1), (0.5 + HALF_LOG_2PI + ls).sum(-1)


def objective(head, v, acts, advs, rets, v_old, old_logp, clip_para, entropy_coeff, clipped_value_loss, loss_mode, tanh):
    """-> (policy loss, value loss, dict of the per-sample terms); the advantage is normalised outside the graph."""
    lp, ent = logp(head, acts, tanh)
    advn = adv_normalize(advs).detach()
    if loss_mode == LOSS_A2C:
        ratio = torch.ones_like(lp)
        surr = -(lp * advn)
    else:
        ratio = torch.exp(lp - old_logp.reshape(-1))
        surr = -torch.minimum(ratio * advn, ratio.clamp(1.0 - clip_para, 1.0 + clip_para) * advn)
    pl = surr.mean() - entropy_coeff * ent.mean()
    vv, R = v.reshape(-1), rets.reshape(-1)
    if clipped_value_loss:
        vc = v_old.reshape(-1) + (vv - v_old.reshape(-1)).clamp(-clip_para, clip_para)
        vloss = 0.5 * torch.maximum((vv - R) ** 2, (vc - R) ** 2)
    else:
        vloss = (vv - R) ** 2
    return pl, vloss.mean(), dict(lp=lp, ent=ent, ratio=ratio, surr=surr, vloss=vloss, v=vv)


def losses(head, v, acts, advs, rets, v_old, old_logp, clip_para, entropy_coeff, clipped_value_loss, loss_mode, tanh):
    """The loss half of one minibatch in the dtype of `head`: -> dict(d_head, d_v, info (24 float64, the kernel's slots))."""
    head = head.detach().clone().requires_grad_(True)
    v = v.detach().clone().reshape(-1).requires_grad_(True)
    pl, vl, r = objective(head, v, acts, advs, rets, v_old, old_logp, clip_para, entropy_coeff, clipped_value_loss,
                          loss_mode, tanh)
    d_head, = torch.autograd.grad(pl, head)
    d_v, = torch.autograd.grad(vl, v)
    _, ls, std = parts(head.detach())
    d = lambda t: t.detach().double()
    lp, ratio, vv = d(r["lp"]), d(r["ratio"]), d(r["v"])
    info = np.zeros(24)
    info[0:8] = [d(r["surr"]).sum(), lp.sum(), (lp * lp).sum(), lp.max(), -lp.min(), ratio.max(), -ratio.min(),
                 d(r["vloss"]).sum()]
    info[12:16] = [vv.sum(), (vv * vv).sum(), vv.max(), -vv.min()]
    for base, x in ((8, d(ls).reshape(-1)), (16, d(std).reshape(-1))):
        info[base:base + 4] = [x.mean(), x.std() if x.numel() > 1 else float("nan"), x.max(), x.min()]
    info[20] = d(r["ent"]).sum()
    return dict(d_head=d_head, d_v=d_v, info=info, lp=r["lp"].detach(), ent=r["ent"].detach(), ratio=r["ratio"].detach())


class SdUpdate:
    """A2C.update / PPO.update with a GuassianContPolicy (a2c.py:45-106, ppo.py:41-152): the layers by torch, the loss half by
    `objective`, clip_grad_norm_(0.5) + Adam(eps=1e-5) per network."""

    def __init__(self, pf_params, vf_params, plr, vlr, entropy_coeff, tanh, clip_para=0.2, target_params=None, act=torch.tanh):
        self.pf, self.vf = MLP(pf_params, act), MLP(vf_params, act)
        self.target = MLP(pf_params if target_params is None else target_params, act)
        self.opt_pf = torch.optim.Adam(self.pf.params, lr=plr, eps=1e-5)
        self.opt_vf = torch.optim.Adam(self.vf.params, lr=vlr, eps=1e-5)
        self.entropy_coeff, self.clip_para, self.tanh = entropy_coeff, clip_para, tanh

    def update(self, batch, loss_mode, clipped_value_loss=False, old_logp=None):
        t = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k, v in batch.items()}
        obs, acts, advs, rets = t["obs"], t["acts"], t["advs"].reshape(-1), t["estimate_returns"].reshape(-1)
        if loss_mode == LOSS_PPO_CLIP and old_logp is None:
            with torch.no_grad():
                old_logp = logp(self.target(obs), acts, self.tanh)[0]
        head, v = self.pf(obs), self.vf(obs)
        pl, vl, r = objective(head, v, acts, advs, rets, t.get("values"), old_logp, self.clip_para, self.entropy_coeff,
                              clipped_value_loss, loss_mode, self.tanh)
        norms = []
        for loss, opt, params in ((pl, self.opt_pf, self.pf.params), (vl, self.opt_vf, self.vf.params)):
            opt.zero_grad()
            loss.backward()
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, 0.5)))
            opt.step()
        _, ls, std = parts(head.detach())
        lp, vv, ent = r["lp"].detach(), v.detach().reshape(-1), r["ent"].detach().mean().item()
        if loss_mode == LOSS_A2C:
            return {'Training/policy_loss': pl.item(), 'Training/vf_loss': vl.item(),
                    'v_pred/mean': vv.mean().item(), 'v_pred/std': vv.std().item(), 'v_pred/max': vv.max().item(),
                    'v_pred/min': vv.min().item(), 'std/mean': std.mean().item(), 'std/std': std.std().item(),
                    'std/max': std.max().item(), 'std/min': std.min().item(), 'ent': ent, 'log_prob': lp.mean().item()}
        ratio = r["ratio"].detach()
        return {'advs/mean': advs.mean().item(), 'advs/std': advs.std().item(), 'advs/max': advs.max().item(),
                'advs/min': advs.min().item(), 'Training/vf_loss': vl.item(), 'grad_norm/vf': norms[1],
                'Training/policy_loss': pl.item(), 'logprob/mean': lp.mean().item(), 'logprob/std': lp.std().item(),
                'logprob/max': lp.max().item(), 'logprob/min': lp.min().item(), 'log_std/mean': ls.mean().item(),
                'log_std/std': ls.std().item(), 'log_std/max': ls.max().item(), 'log_std/min': ls.min().item(),
                'ratio/max': ratio.max().item(), 'ratio/min': ratio.min().item(), 'grad_norm/pf': norms[0]}


TAGS = ["t_s3", "t_s17", "n_s3", "n_s17"]


def batch_of(g, tag):
    return {k: g[f"{tag}_batch_{k}"] for k in ("obs", "acts", "advs", "values", "estimate_returns")}


def info_of(g, prefix):
    return dict(zip((str(k) for k in g[prefix + "_keys"]), (float(x) for x in g[prefix + "_vals"])))
