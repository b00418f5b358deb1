"""Plain torch restatement (any dtype, autograd) of what the fused LayerNorm update differentiates: the two-layer block
Linear, act, [LayerNorm(64, eps 1e-5), Linear, act, act | Linear, act], Linear on explicit plan-ordered parameter lists
[W1 b1 (gamma beta) W2 b2 W3 b3], under the PPO-clip / A2C objectives of the three heads (`_gauss_sd_ref.objective`,
`_categorical_ref.objective`; the shared-std Gaussian is the [mean | log_std] objective with log_std = the logstd vector)."""
import numpy as np
import torch

import _categorical_ref as cat
import _gauss_sd_ref as sd

ACT = {"tanh": torch.tanh, "relu": torch.relu}
HEAD = {"gauss": 0, "cat": 1, "sd": 2}


def draw_net(rs, D, O, ln, plant=None):
    """float64 parameters in plan order; gamma = 1 + 0.3 randn, beta = 0.2 randn; the two planted first layers."""
    W1, b1 = rs.randn(64, D) / np.sqrt(D), 0.1 * rs.randn(64)
    if plant == "zero-variance":
        W1, b1 = np.zeros((64, D)), np.full(64, 0.3)
    if plant == "large-mean":
        b1 = 64.0 + rs.uniform(-0.5, 0.5, 64)
    norm = [1.0 + 0.3 * rs.randn(64), 0.2 * rs.randn(64)] if ln else []
    rest = [rs.randn(64, 64) / 8.0, 0.1 * rs.randn(64), rs.randn(O, 64) / 8.0, 0.1 * rs.randn(O)]
    return [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)) for x in [W1, b1] + norm + rest]


def forward(p, x, act, ln, amp=None):
    """`amp` (a list): gets max over rows of rstd * max|gamma|, the factor the norm multiplies a rounding error of its input by."""
    f = ACT[act]
    h = f(x @ p[0].t() + p[1])
    if ln:
        mean = h.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((h - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
        if amp is not None:
            amp.append(float((rstd.max() * p[2].abs().max()).detach()))
        h = (h - mean) * rstd * p[2] + p[3]
        return f(f(h @ p[4].t() + p[5])) @ p[6].t() + p[7]
    return f(h @ p[2].t() + p[3]) @ p[4].t() + p[5]


def flat_grads(c, pf, ls, vf, mb, dtype, amp=None):
    """Gradient of policy loss + value loss by every parameter, flat [policy block (logstd) | value block], in `dtype`."""
    cast = lambda t: t.to(dtype).clone().requires_grad_(True)
    pf, vf, ls = [cast(t) for t in pf], [cast(t) for t in vf], None if ls is None else cast(ls)
    x, data = mb["obs"].to(dtype), {k: mb[k].to(dtype) for k in ("advs", "rets", "old_values", "old_logp")}
    out = forward(pf, x, c["act"], c["ln"] & 1, amp)
    v = forward(vf, x, c["act"], c["ln"] & 2, amp)
    args = (data["advs"], data["rets"], data["old_values"], data["old_logp"], 0.2, c["c_ent"], c["clipv"], c["mode"])
    if c["head"] == "cat":
        loss = cat.objective(out, v, mb["acts"], *args)
    else:
        head = out if c["head"] == "sd" else torch.cat([out, ls.expand_as(out)], -1)
        pl, vl, _ = sd.objective(head, v, mb["acts"].to(dtype), *args, c["tanh"])
        loss = pl + vl
    params = pf + ([ls] if ls is not None else []) + vf
    return torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, params)]).double().numpy()


def old_logp(c, pf, ls, mb):
    """log pi(act) under the float64 parameters (the clipped surrogate's log pi_old is drawn around it)."""
    out = forward(pf, mb["obs"], c["act"], c["ln"] & 1)
    if c["head"] == "cat":
        return cat.cat_logp(out, mb["acts"].reshape(-1).to(torch.int64))[0]
    return sd.logp(out if c["head"] == "sd" else torch.cat([out, ls.expand_as(out)], -1), mb["acts"], c["tanh"])[0]
