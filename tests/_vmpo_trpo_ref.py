"""Plain torch restatement (CPU, float32 or float64) of the V-MPO and TRPO loss kernels (torchrl_amd/csrc/k_vmpo.hip,
k_trpo.hip), written from the reference's formulas (torchrl/algo/on_policy/v_mpo.py:57-181, trpo.py:28-226,
torchrl/policies/distribution.py) -- test infrastructure, imported by tests/test_vmpo_trpo_kernels_*.py only.

The policy is a diagonal Gaussian with one log_std per action dimension: ls = clamp(logstd, -20, 2), std = exp(ls).  Per
element log pi = -(z - mean)^2 / (2 std^2) - ls - log(2 pi) / 2 [- log(1 - a^2 + 1e-6), z = log((1 + a) / (1 - a)) / 2 for
tanh actions], entropy = 1/2 + log(2 pi) / 2 + ls.  Gradients come from autograd; torch.clamp passes the gradient on the
closed interval, which is the kernels' gate.  d_logstd is taken through a (n, A) copy of log_std, so that the per-sample
terms whose sum it is are available too (the tests' absolute bound is built from them).

Also the seeded float32 input builders that the CPU and the GPU tests share, and the list of cases with the bounds."""
import math

import numpy as np
import torch

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
ACT_TANH, ACT_RELU, ACT_NONE = 0, 1, 2


# ---------------------------------------------------------------- the policy
def _logp_rows(mean, ls, acts, tanh):
    """ls: clamped, broadcastable to (n, A) -> log pi (n,)."""
    pre, corr = acts, 0.0
    if tanh:
        pre = 0.5 * torch.log((1.0 + acts) / (1.0 - acts))
        corr = torch.log(1.0 - acts * acts + 1e-6)
    zc = pre - mean
    return (-(zc * zc) / (2.0 * torch.exp(2.0 * ls)) - ls - HALF_LOG_2PI - corr).sum(-1)


def logp(mean, logstd, acts, tanh):
    """logstd (A,) raw -> log pi (n,)."""
    return _logp_rows(mean, logstd.clamp(-20.0, 2.0), acts, tanh)


def kl_rows(mean, ls, tmean, tls):
    """KL(N(mean, e^ls) || N(tmean, e^tls)) summed over the action dimensions, both log_std already clamped."""
    return ((tls - ls) + (torch.exp(2.0 * ls) + (mean - tmean) ** 2) / (2.0 * torch.exp(2.0 * tls)) - 0.5).sum(-1)


def _stats(x):
    x = x.detach().double()
    return [x.mean().item(), x.std().item() if x.numel() > 1 else float("nan"), x.max().item(), x.min().item()]


# ---------------------------------------------------------------- the small kernels
def adv_normalize(advs_local, advs_all, eps):
    return (advs_local - advs_all.mean()) / (advs_all.std() + eps)


def mse_value(v, rets, n_global):
    """-> (d_v of mean-over-n_global (v - R)^2, the local loss SUM)."""
    d = v.reshape(-1) - rets.reshape(-1)
    return 2.0 * d / n_global, (d * d).sum()


def ratio_loss(lp_new, lp_old, adv):
    return -(torch.exp(lp_new - lp_old) * adv).mean()


def jvp_gate(a, b, h, act):
    v = a if b is None else a + b
    if h is None or act == ACT_NONE:
        return v
    return v * ((1.0 - h * h) if act == ACT_TANH else (h > 0).to(v.dtype))


def fisher_scale(d_mu, logstd):
    return d_mu * torch.exp(-2.0 * logstd.clamp(-20.0, 2.0)) / d_mu.shape[0]


# ---------------------------------------------------------------- V-MPO
DUAL0 = (1.0, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0)                 # eta, alpha, exp_avg x2, exp_avg_sq x2, steps


def vmpo_losses(mean, tmean, logstd, tlogstd, acts, adv, dual, tanh, eta_eps, alpha_eps, lr):
    """The loss half of VMPO.update_actor on the n selected samples, in the dtype of `mean`.  dual: 7 values {eta, alpha,
    Adam's exp_avg x2, exp_avg_sq x2, steps}.  -> dict(d_mean (n, A), d_logstd (A,), dls_abs (A,) the sum over samples of
    the absolute per-sample term of d_logstd, info (12 float64, the slots of include/trl_hip.h), dual (7, after the step),
    phi, lp, kl)."""
    dt = mean.dtype
    n, A = mean.shape
    dual = torch.as_tensor(dual, dtype=dt)
    m = mean.detach().clone().requires_grad_(True)
    ls_rows = logstd.detach().expand(n, A).clone().requires_grad_(True)
    eta = dual[0:1].clone().requires_grad_(True)
    alpha = dual[1:2].clone().requires_grad_(True)
    ls, tls = ls_rows.clamp(-20.0, 2.0), tlogstd.detach().clamp(-20.0, 2.0)
    adv = adv.detach().reshape(-1)
    lp = _logp_rows(m, ls, acts, tanh)
    kl = kl_rows(m, ls, tmean.detach(), tls)
    phi = torch.softmax(adv / eta.detach(), dim=0)
    l_pi = (-phi * lp + alpha.detach() * kl).mean()
    l_eta = eta * eta_eps + eta * (torch.logsumexp(adv / eta, dim=0) - math.log(n))
    l_alpha = alpha * alpha_eps - alpha * kl.detach().mean()
    d_mean, d_rows = torch.autograd.grad(l_pi, [m, ls_rows])
    eta.grad, = torch.autograd.grad(l_eta.sum(), eta)
    alpha.grad, = torch.autograd.grad(l_alpha.sum(), alpha)
    opt = torch.optim.Adam([eta, alpha], lr=lr, eps=1e-5, foreach=False)
    for k, p in enumerate((eta, alpha)):
        opt.state[p] = dict(step=torch.tensor(float(dual[6])), exp_avg=dual[2 + k:3 + k].clone(),
                            exp_avg_sq=dual[4 + k:5 + k].clone())
    opt.step()
    with torch.no_grad():
        eta.clamp_(min=1e-8)
        alpha.clamp_(min=1e-8)
    new = torch.stack([eta.detach()[0], alpha.detach()[0], opt.state[eta]["exp_avg"][0], opt.state[alpha]["exp_avg"][0],
                       opt.state[eta]["exp_avg_sq"][0], opt.state[alpha]["exp_avg_sq"][0],
                       opt.state[eta]["step"].to(dt)]).double()
    info = np.array([l_pi.item()] + _stats(lp) + _stats(kl) + [l_alpha.item(), new[1].item(), new[0].item()])
    return dict(d_mean=d_mean, d_logstd=d_rows.sum(0), dls_abs=d_rows.double().abs().sum(0), info=info, dual=new,
                phi=phi.detach(), lp=lp.detach(), kl=kl.detach())


# ---------------------------------------------------------------- TRPO
def trpo_surrogate(mean, logstd, acts, adv, tanh, c_ent, prob_eps=1e-8):
    """L = -mean(p / (p.detach() + 1e-8) * adv) - c_ent * mean over samples of the Normal entropy (trpo.py:170-180).
    -> dict(d_mean, d_logstd, dls_abs, info (5 float64: L, log pi mean / unbiased std / max / min), w (n,), lp)."""
    n, A = mean.shape
    m = mean.detach().clone().requires_grad_(True)
    ls_rows = logstd.detach().expand(n, A).clone().requires_grad_(True)
    ls = ls_rows.clamp(-20.0, 2.0)
    lp = _logp_rows(m, ls, acts, tanh)
    p = torch.exp(lp)
    ratio = p / (p.detach() + prob_eps)
    ent = (0.5 + HALF_LOG_2PI + ls).sum(-1)
    loss = -(ratio * adv.detach().reshape(-1)).mean() - c_ent * ent.mean()
    d_mean, d_rows = torch.autograd.grad(loss, [m, ls_rows])
    return dict(d_mean=d_mean, d_logstd=d_rows.sum(0), dls_abs=d_rows.double().abs().sum(0),
                info=np.array([loss.item()] + _stats(lp)), w=ratio.detach(), lp=lp.detach())


# ---------------------------------------------------------------- seeded float32 inputs
def _acts_of(mean, std, eps, scale, tanh):
    z = mean + std * eps * scale[:, None]
    return torch.tanh(z).clamp(-0.995, 0.995) if tanh else z


def policy_case(n, A, tanh, seed, ls_range=(-1.5, 0.5), lp_range=None, raw_logstd=None):
    """Float32 inputs of one batch: mean = 0.5 N(0, 1), log_std uniform in ls_range (raw_logstd = {index: value} overwrites
    entries, the same in the target unless the key is ("target", index)), actions drawn from the policy itself (tanh
    actions clamped to +-0.995), the target policy = the policy + 0.05 N(0, 1) in mean and log_std.
    lp_range = (lo, hi): every sample's noise is scaled by a factor of its own, found by bisection, so that the float64
    log pi of its float32 action is a uniform draw from [lo, hi] (as far as the factor's range [0, 50] reaches)."""
    rs = np.random.RandomState(seed)
    f = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32))
    mean = f(0.5 * rs.randn(n, A))
    logstd = f(rs.uniform(ls_range[0], ls_range[1], A))
    eps = f(rs.randn(n, A))
    tmean = mean + f(0.05 * rs.randn(n, A))
    tlogstd = logstd + f(0.05 * rs.randn(A))
    for k, val in (raw_logstd or {}).items():
        if isinstance(k, tuple):
            tlogstd[k[1]] = val
        else:
            logstd[k] = val
            tlogstd[k] = val
    std = torch.exp(logstd.clamp(-20.0, 2.0))
    scale = torch.ones(n)
    if lp_range is not None:
        target = torch.from_numpy(rs.uniform(lp_range[0], lp_range[1], n))
        lo, hi = torch.zeros(n), torch.full((n,), 50.0)
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            above = logp(mean.double(), logstd.double(), _acts_of(mean, std, eps, mid, tanh).double(), tanh) > target
            lo, hi = torch.where(above, mid, lo), torch.where(above, hi, mid)
        scale = lo
    acts = _acts_of(mean, std, eps, scale, tanh).contiguous()
    return dict(mean=mean, logstd=logstd, acts=acts, tmean=tmean, tlogstd=tlogstd)


def vmpo_adv(n, seed):
    """The host's selection (v_mpo.py:64-70, :181): 2n advantages 2 N(0, 1) + 0.5, normalised, the top half, descending."""
    rs = np.random.RandomState(seed)
    a = torch.from_numpy((2.0 * rs.randn(2 * n) + 0.5).astype(np.float32))
    a = (a - a.mean()) / (a.std() + 1e-5)
    return torch.sort(a, descending=True)[0][:n].contiguous()


def trpo_adv(n, seed):
    return torch.from_numpy(np.random.RandomState(seed).randn(n).astype(np.float32))


# ---------------------------------------------------------------- the cases (CPU: conditions on them; GPU: the kernels)
# every n at A = 6, every A at n = 300: a partial wave, one full block, one valid lane in the second block, two blocks
# with a ragged tail, four blocks
SHAPES = [(1, 6), (48, 6), (256, 6), (257, 6), (300, 6), (1000, 6), (300, 1), (300, 64)]
GATE = {1: -25.0, 4: 3.0}                                             # raw log_std outside [-20, 2]
VMPO_GATE = {1: -25.0, 4: 3.0, ("target", 2): 3.0}
# TRPO: log_std per A such that log pi at the mean is above -6 and the per-sample noise factor can reach -22
TRPO_LS = {1: (-1.5, -1.0), 6: (-1.5, -1.0), 64: (-1.6, -1.2)}
TRPO_LP = (-22.0, -6.0)                                               # w = p / (p + 1e-8) moves between -23 and -13.8
TRPO_LP_WIDE = (-30.0, -8.0)
# seeds of the small-eta advantages: chosen (on the inputs alone) so that at least 3 samples carry phi > 1e-3
SMALL_ETA = 0.02
SMALL_ETA_SEED = {300: 8, 1000: 8}


def vmpo_case(n, A, tanh, gate=False):
    c = policy_case(n, A, tanh, 7000 + 13 * n + A + int(tanh), raw_logstd=VMPO_GATE if gate else None)
    c["adv"] = vmpo_adv(n, 100 + n + A)
    return c


def vmpo_small_eta_case(n):
    c = policy_case(n, 6, True, 7500 + n)
    c["adv"] = vmpo_adv(n, SMALL_ETA_SEED[n])
    return c


def trpo_case(n, A, tanh, gate=False, wide=False):
    c = policy_case(n, A, tanh, 9000 + 13 * n + A + int(tanh) + 500 * int(wide), ls_range=TRPO_LS[A],
                    lp_range=TRPO_LP_WIDE if wide else TRPO_LP, raw_logstd=GATE if gate else None)
    c["adv"] = trpo_adv(n, 200 + n + A)
    return c


def vmpo_cases():
    """-> list of (id, case, tanh, eta) for every V-MPO comparison of the GPU test."""
    out = [("n%d-A%d-tanh%d" % (n, A, t), vmpo_case(n, A, bool(t)), bool(t), 1.0) for n, A in SHAPES for t in (0, 1)]
    out.append(("gate", vmpo_case(300, 6, False, gate=True), False, 1.0))
    out += [("small-eta-n%d" % n, vmpo_small_eta_case(n), True, SMALL_ETA) for n in (300, 1000)]
    return out


def trpo_cases():
    """-> list of (id, case, tanh) for every TRPO comparison of the GPU test."""
    out = [("n%d-A%d-tanh%d" % (n, A, t), trpo_case(n, A, bool(t)), bool(t)) for n, A in SHAPES for t in (0, 1)]
    out.append(("gate", trpo_case(300, 6, False, gate=True), False))
    out.append(("wide", trpo_case(300, 6, False, wide=True), False))
    return out


# ---------------------------------------------------------------- the bounds
def grad_ratios(got, want):
    """Worst err / bound of d_mean (rel 1e-4, abs 1e-4 / n) and of d_logstd (rel 1e-4, abs 1e-5 * the float64 sum over
    samples of the absolute per-sample term).  `want` is a float64 result of vmpo_losses / trpo_surrogate."""
    n = want["d_mean"].shape[0]
    dm = (got["d_mean"].double() - want["d_mean"]).abs() / (1e-4 / n + 1e-4 * want["d_mean"].abs())
    dl = (got["d_logstd"].double() - want["d_logstd"]).abs() / (1e-5 * want["dls_abs"] + 1e-4 * want["d_logstd"].abs())
    dl = torch.where(want["dls_abs"] == 0, (got["d_logstd"].double() != 0).double() * 2.0, dl)   # gated: exactly zero
    return dm.max().item(), dl.max().item()


def info_ratios(got, want, nan_slots=()):
    """err / bound per info slot (rel 1e-4, abs 1e-5); a slot in nan_slots has to be NaN in both."""
    out = []
    for k in range(len(want)):
        if k in nan_slots:
            out.append(0.0 if (math.isnan(got[k]) and math.isnan(want[k])) else float("inf"))
        else:
            r = abs(got[k] - want[k]) / (1e-5 + 1e-4 * abs(want[k]))
            out.append(r if math.isfinite(r) else float("inf"))
    return out


def dual_ratios(got, want, moments=True):
    """eta, alpha: rel 2e-6; Adam's moments: rel 1e-4; the step count: exact.  moments=False (small eta: the gradient of
    eta is a difference of two terms of ~max(adv) / eta, so its digits beyond the fifth are float32 round-off): eta and
    alpha only."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    r = [abs(got[k] - want[k]) / (2e-6 * abs(want[k])) for k in (0, 1)]
    if not moments:
        return r
    r += [abs(got[k] - want[k]) / (1e-4 * abs(want[k])) if want[k] != 0 else float(got[k] != 0) * 2.0 for k in (2, 3, 4, 5)]
    r.append(0.0 if got[6] == want[6] else float("inf"))
    return r
