"""Plain torch restatement (CPU, float32 or float64) of the TRPO / V-MPO kernels for the categorical and the
state-dependent-std head (torchrl_amd/csrc/k_trpo.hip, k_vmpo.hip: trl_trpo_surrogate_{cat,sd}_f32,
trl_fisher_scale_{cat,sd}_f32, trl_vmpo_losses_{cat,sd}_f32), written from the reference's formulas
(torchrl/algo/on_policy/trpo.py:28-226, v_mpo.py:57-181, policies/discrete_policies.py:124-168,
continuous_policy.py:134-170) -- test infrastructure, imported by tests/test_vmpo_trpo_heads_*.py only.

Heads.  "cat": the head row holds A logits, log p = log_softmax, a stored action is truncated and clamped into [0, A).
"sd": the head row is [mean | raw log_std], ls = clamp(raw, -20, 2) per sample (torch.clamp passes the gradient on the
closed interval: the kernels' gate), log pi and entropy per element as in tests/_vmpo_trpo_ref.py.

Every gradient comes from autograd.  Beside each compared quantity stands its RUNNING MAGNITUDE M (float64): the sum of the
absolute values of the terms the quantity is the sum of, with the products' factors replaced by their own magnitudes.
A float32 evaluation in any summation order errs by a small multiple K of u M; the tests bound err <= K M + FLOOR with
K = 4 x the largest err / M the float32 run of this restatement shows against its float64 run over all cases (the
table K below; `python tests/_vmpo_trpo_heads_ref.py` prints the measurement, profiles/NOTES_vmpo_trpo_heads.md keeps it).

Also: the Fisher-vector products by double backward of the mean KL through a small MLP; the whole V-MPO / TRPO updates
restated over flat parameter lists (`HeadVMPO`, `HeadTRPO`) for the fixture tests; the seeded inputs and the case tables."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _vmpo_trpo_ref as gref                                                 # noqa: E402

HALF_LOG_2PI = gref.HALF_LOG_2PI
KL_MEAN, KL_SUM = 0, 1
FLOOR = 2.0 ** -126                    # float32's smallest normal number: below it a kernel may flush to zero
U = 2.0 ** -24


# ---------------------------------------------------------------- the two heads
def cat_terms(logits, acts):
    """-> lsm (n, A) = log p, p, the action index (n,), log pi(a) (n,), entropy (n,)."""
    A = logits.shape[1]
    lsm = torch.log_softmax(logits, -1)
    p = lsm.exp()
    a = acts.reshape(-1).to(torch.int64).clamp(0, A - 1)                      # (.to(int64) truncates, as the kernel's cast)
    return lsm, p, a, lsm.gather(1, a[:, None])[:, 0], -(p * lsm).sum(-1)


def sd_split(head):
    A = head.shape[1] // 2
    return head[:, :A], head[:, A:]


def sd_terms(head, acts, tanh):
    """-> mean, clamped log_std, log pi (n,), entropy (n,)."""
    mean, raw = sd_split(head)
    ls = raw.clamp(-20.0, 2.0)
    return mean, ls, gref._logp_rows(mean, ls, acts, tanh), (0.5 + HALF_LOG_2PI + ls).sum(-1)


def _sd_mags(head, acts, tanh):
    """float64 magnitudes of one sd head: zc, |pre| + |mean| (+ 1 for the atanh), the quadratic term's and log pi's M."""
    mean, raw = sd_split(head.double())
    ls = raw.clamp(-20.0, 2.0)
    a = acts.double()
    pre = 0.5 * torch.log((1.0 + a) / (1.0 - a)) if tanh else a
    corr = torch.log(1.0 - a * a + 1e-6).abs() if tanh else torch.zeros_like(a)
    zc = pre - mean
    zmag = pre.abs() + mean.abs() + (1.0 if tanh else 0.0)
    ivv = torch.exp(-2.0 * ls)
    q = 0.5 * zc * zc * ivv + zc.abs() * zmag * ivv                           # d(zc^2) = 2 zc d zc, |d zc| <= u zmag
    return dict(zc=zc, zmag=zmag, ivv=ivv, ls=ls, q=q, lp=(q + ls.abs() + HALF_LOG_2PI + corr).sum(-1),
                gate=((raw >= -20.0) & (raw <= 2.0)).double())


def _cat_mags(logits, acts):
    l = logits.double()
    lsm, p, a, lp, H = cat_terms(l, acts)
    m = l.max(-1).values
    logS = torch.logsumexp(l - m[:, None], -1)
    lpk = (l.abs() + m.abs()[:, None]) + logS.abs()[:, None]                   # M of log p_k
    return dict(p=p, lpk=lpk, lp=lpk.gather(1, a[:, None])[:, 0], H=(p * lpk).sum(-1), a=a)


def _stats_mag(m):
    """M of the four logged statistics (mean, unbiased std, max, min) of per-sample values with magnitudes m."""
    return [m.mean().item(), m.max().item(), m.max().item(), m.max().item()]


# ---------------------------------------------------------------- TRPO: surrogate
def trpo_surrogate(kind, head, acts, adv, tanh, c_ent, prob_eps=1e-8):
    """L = -mean(p / (p.detach() + 1e-8) * adv) - c_ent * mean(H) in the dtype of `head`.
    -> dict(d_head, info (5 float64: L, log pi mean / unbiased std / max / min), w, lp, mag: dict(d_head, info))."""
    n = head.shape[0]
    h = head.detach().clone().requires_grad_(True)
    adv = adv.detach().reshape(-1)
    if kind == "cat":
        lp, ent = cat_terms(h, acts)[3:]
    else:
        lp, ent = sd_terms(h, acts, tanh)[2:]
    p = torch.exp(lp)
    w = p / (p.detach() + prob_eps)
    loss = -(w * adv).mean() - c_ent * ent.mean()
    d_head, = torch.autograd.grad(loss, h)
    # ---- magnitudes (float64) ----
    a64, w64 = adv.double().abs(), w.detach().double()
    g = a64 * w64 / n                                                          # |d L / d log pi|
    ce = abs(c_ent) / n
    if kind == "cat":
        mg = _cat_mags(head, acts)
        onehot = torch.zeros_like(mg["p"]).scatter_(1, mg["a"][:, None], 1.0)
        m_d = g[:, None] * (onehot + mg["p"]) + ce * mg["p"] * (mg["lpk"] + mg["H"][:, None])
        m_lp, m_ent = mg["lp"], mg["H"]
    else:
        mg = _sd_mags(head, acts, tanh)
        m_d = torch.cat([g[:, None] * mg["zmag"] * mg["ivv"],
                         mg["gate"] * (g[:, None] * (2.0 * mg["q"] + 1.0) + ce)], 1)
        m_lp, m_ent = mg["lp"], (0.5 + HALF_LOG_2PI + mg["ls"].abs()).sum(-1)
    # the weight w = p / (p + 1e-8) moves by (1 - w) d lp: log pi's own magnitude enters d L / d log pi
    m_d = m_d * (1.0 + ((1.0 - w64) * m_lp)[:, None])
    m_loss = (a64 * w64 * (1.0 + (1.0 - w64) * m_lp)).mean().item() + abs(c_ent) * m_ent.mean().item()
    return dict(d_head=d_head, info=np.array([loss.item()] + gref._stats(lp)), w=w.detach(), lp=lp.detach(),
                mag=dict(d_head=m_d, info=np.array([m_loss] + _stats_mag(m_lp))))


# ---------------------------------------------------------------- TRPO: Fisher scaling and products
def fisher_scale(kind, t, head):
    """H t / n with H the Hessian of KL(pi || pi.detach()) in the head at the expansion point.  -> (out, M)."""
    n = head.shape[0]
    if kind == "cat":
        p = torch.softmax(head, -1)
        out = p * (t - (p * t).sum(-1, keepdim=True)) / n
        p64, t64 = torch.softmax(head.double(), -1), t.double().abs()
        return out, p64 * (t64 + (p64 * t64).sum(-1, keepdim=True)) / n
    mean, raw = sd_split(head)
    A = mean.shape[1]
    gate = ((raw >= -20.0) & (raw <= 2.0)).to(head.dtype)
    out = torch.cat([t[:, :A] * torch.exp(-2.0 * raw.clamp(-20.0, 2.0)), 2.0 * gate * t[:, A:]], 1) / n
    return out, out.double().abs()


def mlp(x, params):
    """Tanh after every hidden layer, a linear head; params = [W1, b1, ..., Wh, bh] (nn.Linear layout)."""
    for i in range(len(params) // 2 - 1):
        x = torch.tanh(torch.nn.functional.linear(x, params[2 * i], params[2 * i + 1]))
    return torch.nn.functional.linear(x, params[-2], params[-1])


def mean_kl(kind, head, prob_eps):
    """mean KL(pi_theta || pi_theta.detach()) as trpo.py:29-63 writes it (prob_eps = 1e-8 inside the discrete log; 0.0 is
    the KL whose Hessian the kernels take -- the two Hessians differ by O(1e-8 / p))."""
    if kind == "cat":
        p = torch.softmax(head, -1)
        return torch.sum(p * torch.log(p / (p.detach() + prob_eps)), 1).mean()
    mean, raw = sd_split(head)
    s_old = torch.exp(raw.clamp(-20.0, 2.0))
    m_new, s_new = mean.detach(), s_old.detach()
    return torch.mean(torch.sum(torch.log(s_new) - torch.log(s_old) + (s_old * s_old + (mean - m_new) ** 2)
                                / (2.0 * s_new * s_new) - 0.5, 1))


def fvp_double_backward(kind, params, obs, v, prob_eps=0.0):
    """(Hessian of the mean KL in the flat parameters) v, by double backward (trpo.py:65-86, without the damping)."""
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    g = torch.autograd.grad(mean_kl(kind, mlp(obs, ps), prob_eps), ps, create_graph=True)
    gv = torch.sum(torch.cat([x.reshape(-1) for x in g]) * v)
    return torch.cat([x.contiguous().reshape(-1) for x in torch.autograd.grad(gv, ps)])


# ---------------------------------------------------------------- V-MPO: the loss half
DUAL0 = gref.DUAL0


def _adam_scalar(p, g, m, v, t, lr):
    """One Adam(lr, (0.9, 0.999), eps 1e-5) step of a float64 scalar, clamped at 1e-8 (v_mpo.py:34-38, :113-115)."""
    m, v, t = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g, t + 1.0
    return max(p - lr / (1.0 - 0.9 ** t) * m / (math.sqrt(v) / math.sqrt(1.0 - 0.999 ** t) + 1e-5), 1e-8), m, v


def vmpo_losses(kind, head, thead, acts, adv, dual, tanh, kl_reduce, eta_eps, alpha_eps, lr):
    """The loss half of VMPO.update_actor on the n selected samples in the dtype of `head`.  dual: 7 values {eta, alpha,
    Adam's exp_avg x2, exp_avg_sq x2, steps}.  kl_reduce KL_SUM: sum_b KL_b stands where mean_b KL_b does.
    -> dict(d_head, info (12 float64), dual (7 float64, after the step), g (the gradients of eta and alpha), phi, lp, kl,
    mag: dict(d_head, info, g, dual))."""
    dt = head.dtype
    n = head.shape[0]
    dual = torch.as_tensor(dual, dtype=dt)
    h = head.detach().clone().requires_grad_(True)
    eta = dual[0:1].clone().requires_grad_(True)
    alpha = dual[1:2].clone().requires_grad_(True)
    adv = adv.detach().reshape(-1)
    if kind == "cat":
        lsm, p, _, lp, _ = cat_terms(h, acts)
        tlsm = torch.log_softmax(thead.detach(), -1)
        kl = (p * (lsm - tlsm)).sum(-1)
    else:
        mean, ls, lp, _ = sd_terms(h, acts, tanh)
        tmean, traw = sd_split(thead.detach())
        kl = gref.kl_rows(mean, ls, tmean, traw.clamp(-20.0, 2.0))
    red = (lambda x: x.sum()) if kl_reduce == KL_SUM else (lambda x: x.mean())
    phi = torch.softmax(adv / eta.detach(), dim=0)
    l_pi = (-phi * lp).mean() + alpha.detach()[0] * red(kl)
    l_eta = eta * eta_eps + eta * (torch.logsumexp(adv / eta, dim=0) - math.log(n))
    l_alpha = alpha * alpha_eps - alpha * red(kl.detach())
    d_head, = torch.autograd.grad(l_pi, h)
    eta.grad, = torch.autograd.grad(l_eta.sum(), eta)
    alpha.grad, = torch.autograd.grad(l_alpha.sum(), alpha)
    g = np.array([eta.grad.item(), alpha.grad.item()])
    opt = torch.optim.Adam([eta, alpha], lr=lr, eps=1e-5, foreach=False)
    for k, q in enumerate((eta, alpha)):
        opt.state[q] = dict(step=torch.tensor(float(dual[6])), exp_avg=dual[2 + k:3 + k].clone(),
                            exp_avg_sq=dual[4 + k:5 + k].clone())
    opt.step()
    with torch.no_grad():
        eta.clamp_(min=1e-8)
        alpha.clamp_(min=1e-8)
    new = torch.stack([eta.detach()[0], alpha.detach()[0], opt.state[eta]["exp_avg"][0], opt.state[alpha]["exp_avg"][0],
                       opt.state[eta]["exp_avg_sq"][0], opt.state[alpha]["exp_avg_sq"][0],
                       opt.state[eta]["step"].to(dt)]).double()
    if kl_reduce == KL_SUM:
        s = kl.detach().double().sum().item()
        kl_stats = [s, float("nan"), s, s]
    else:
        kl_stats = gref._stats(kl)
    info = np.array([l_pi.item()] + gref._stats(lp) + kl_stats + [l_alpha.item(), new[1].item(), new[0].item()])
    # ---- magnitudes (float64) ----
    d0 = np.asarray(dual.double())
    eta0, alpha0 = d0[0], d0[1]
    phi64 = phi.detach().double()
    x = adv.double() / eta0
    phi_rel = 1.0 + (x - x.max()).abs() + x.abs()                             # phi moves by u (|x| + |x - max|) of itself
    g_lp = phi64 * phi_rel / n
    kw = alpha0 if kl_reduce == KL_SUM else alpha0 / n
    if kind == "cat":
        mg = _cat_mags(head, acts)
        tmg = _cat_mags(thead, acts)
        dl = mg["lpk"] + tmg["lpk"]
        m_kl = (mg["p"] * dl).sum(-1)
        onehot = torch.zeros_like(mg["p"]).scatter_(1, mg["a"][:, None], 1.0)
        m_d = g_lp[:, None] * (onehot + mg["p"]) + kw * mg["p"] * (dl + m_kl[:, None])
        m_lp = mg["lp"]
    else:
        mg = _sd_mags(head, acts, tanh)
        tmean, traw = sd_split(thead.double())
        tls = traw.clamp(-20.0, 2.0)
        tivv, var = torch.exp(-2.0 * tls), torch.exp(2.0 * mg["ls"])
        mean64 = sd_split(head.double())[0]
        dm, dmag = (mean64 - tmean).abs(), mean64.abs() + tmean.abs()
        m_kl = (tls.abs() + mg["ls"].abs() + 0.5 * (var + dm * dm + 2.0 * dm * dmag) * tivv + 0.5).sum(-1)
        m_d = torch.cat([g_lp[:, None] * mg["zmag"] * mg["ivv"] + kw * dmag * tivv,
                         mg["gate"] * (g_lp[:, None] * (2.0 * mg["q"] + 1.0) + kw * (var * tivv + 1.0))], 1)
        m_lp = mg["lp"]
    kl_red_mag = m_kl.sum().item() if kl_reduce == KL_SUM else m_kl.mean().item()
    m_info = [(phi64 * (m_lp + phi_rel * lp.detach().double().abs())).mean().item() + alpha0 * kl_red_mag] + _stats_mag(m_lp)
    m_info += [kl_red_mag] * 4 if kl_reduce == KL_SUM else _stats_mag(m_kl)
    m_info.append(alpha0 * (abs(alpha_eps) + kl_red_mag))
    # g_eta = eps + log mean exp(x) - sum_b phi_b x_b: a difference of two terms of ~max |x|
    m_g = np.array([abs(eta_eps) + 2.0 * x.abs().max().item() + abs(math.log(n)) + 1.0, abs(alpha_eps) + kl_red_mag])
    return dict(d_head=d_head, info=info, dual=new, g=g, phi=phi.detach(), lp=lp.detach(), kl=kl.detach(),
                mag=dict(d_head=m_d, info=np.array(m_info), g=m_g))


def dual_bounds(want, dual0, lr, K_g):
    """Bounds of the 7 dual values after the step, from the bound K_g M_g of the two gradients: exp_avg and exp_avg_sq
    directly, eta and alpha by putting g -+ K_g M_g through the float64 Adam step (and the step count is exact).  Every
    float32 value carries 4 u of its own magnitude on top."""
    d0 = np.asarray(dual0, dtype=np.float64)
    out = np.zeros(7)
    for k in range(2):
        g, e = want["g"][k], K_g * want["mag"]["g"][k]
        ref_p = _adam_scalar(d0[k], g, d0[2 + k], d0[4 + k], d0[6], lr)[0]
        moved = max(abs(_adam_scalar(d0[k], g + s * e, d0[2 + k], d0[4 + k], d0[6], lr)[0] - ref_p) for s in (-1.0, -0.5, 0.5, 1.0))
        out[k] = moved + 4 * U * (abs(d0[k]) + lr)
        out[2 + k] = 0.1 * e + 4 * U * (abs(0.9 * d0[2 + k]) + 0.1 * abs(g))
        out[4 + k] = 0.001 * (2.0 * abs(g) * e + e * e) + 4 * U * (0.999 * d0[4 + k] + 0.001 * g * g)
    return out


# ---------------------------------------------------------------- the bounds
# K per compared quantity: 4 x the largest err / M of the float32 run of this restatement against its float64 run over
# every case below (measure(); the measured values are in profiles/NOTES_vmpo_trpo_heads.md).
K = {
    "trpo_cat_d_head": 8.9e-05,         # measured 2.222e-05
    "trpo_cat_info": 2.4e-07,           # measured 5.806e-08
    "trpo_sd_d_head": 9.8e-07,          # measured 2.441e-07
    "trpo_sd_info": 3.6e-07,            # measured 8.844e-08
    "fisher_cat": 1.6e-06,              # measured 3.830e-07
    "fisher_sd": 6.3e-07,               # measured 1.575e-07
    "vmpo_cat_d_head": 7.4e-06,         # measured 1.832e-06
    "vmpo_cat_info": 1.4e-07,           # measured 3.277e-08
    "vmpo_cat_g": 2.7e-07,              # measured 6.564e-08
    "vmpo_sd_d_head": 7.6e-07,          # measured 1.892e-07
    "vmpo_sd_info": 4.6e-07,            # measured 1.137e-07
    "vmpo_sd_g": 2.9e-07,               # measured 7.186e-08
}


def ratio(got, want, mag):
    """Worst |got - want| / M over the elements (float64); an element whose M is zero has to be equal (inf otherwise); a
    NaN in `want` has to be a NaN in `got`."""
    got, want, mag = (np.asarray(torch.as_tensor(x).detach().double()) for x in (got, want, mag))
    nan = np.isnan(want)
    if (np.isnan(got) != nan).any():
        return float("inf")
    err = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want)))
    err = np.maximum(err - FLOOR, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(mag > 0, err / mag, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------- seeded float32 inputs
NS = (1, 2, 255, 256, 257, 1025)
CAT_A = (2, 6, 64)
SD_A = (1, 6, 32)
F32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32))


def cat_case(n, A, seed, edges=True):
    """logits N(0, 1), target logits = logits + 0.1 N(0, 1), uniform stored actions.  edges (n >= 8): row 0 spreads its
    logits over +-40 (and, A >= 3, one at -75: that probability is zero in float32), the action on the +40; row 1 the same
    with the action on the -40 (log pi = -80); rows 2 / 3 take an action with log pi ~ -18 / ~ -30 (every other logit but
    the first at -60); rows 4 / 5 store an action index above A - 1 / below 0."""
    rs = np.random.RandomState(seed)
    logits = rs.randn(n, A)
    tlogits = logits + 0.1 * rs.randn(n, A)
    acts = rs.randint(0, A, size=n).astype(np.float64)
    if edges and n >= 8:
        for r, (second, a) in enumerate(((-40.0, 0), (-40.0, 1), (-18.0, 1), (-30.0, 1))):
            logits[r] = -60.0
            logits[r, 0], logits[r, 1] = (40.0 if r < 2 else 0.0), second
            if r < 2 and A >= 3:
                logits[r, 2] = -75.0
            tlogits[r] = logits[r] + 0.1 * rs.randn(A)
            acts[r] = a
        acts[4], acts[5] = A + 3, -2
    return dict(head=F32(logits), thead=F32(tlogits), acts=F32(acts))


SD_EDGE = (-25.0, 3.0, -20.0, 2.0)                                            # raw log_std: below, above, exactly at the ends


def sd_case(n, A, tanh, seed, edges=True):
    """head = [0.5 N(0, 1) | U(-1.5, 0.5)], target = head + 0.05 N(0, 1), actions drawn from the policy (tanh actions
    clamped to +-0.995).  edges: rows 0..3 carry SD_EDGE in log_std column 0, rows 4..7 carry it in the TARGET's last
    log_std column (as far as n reaches); the actions of the edge rows are drawn with the clamped std as well -- but where
    the policy's own std is e^-20 = 2e-9, float32 cannot place an action within a standard deviation of any mean but 0
    (log pi would be its round-off times 2e17), so that element's mean and action are both exactly 0."""
    rs = np.random.RandomState(seed)
    mean, raw = 0.5 * rs.randn(n, A), rs.uniform(-1.5, 0.5, (n, A))
    tmean, traw = mean + 0.05 * rs.randn(n, A), raw + 0.05 * rs.randn(n, A)
    if edges:
        for r, val in enumerate(SD_EDGE):
            if r < n:
                raw[r, 0] = val
                traw[r, 0] = val
            if 4 + r < n:
                traw[4 + r, A - 1] = val
    tight = [r for r, val in enumerate(SD_EDGE) if edges and r < n and val <= -20.0]
    mean[tight, 0] = 0.0
    z = mean + np.exp(np.clip(raw, -20.0, 2.0)) * rs.randn(n, A)
    acts = np.clip(np.tanh(z), -0.995, 0.995) if tanh else z
    acts[tight, 0] = 0.0
    return dict(head=F32(np.concatenate([mean, raw], 1)), thead=F32(np.concatenate([tmean, traw], 1)), acts=F32(acts))


def trpo_cases():
    """-> {id: (kind, case with "adv", tanh)}: every n at the middle A, every A at n = 257, both tanh values for sd."""
    out = {}
    for n in NS:
        for A in (CAT_A if n == 257 else CAT_A[1:2]):
            c = cat_case(n, A, 11000 + 7 * n + A)
            c["adv"] = gref.trpo_adv(n, 300 + n + A)
            out["cat-n%d-A%d" % (n, A)] = ("cat", c, False)
        for A in (SD_A if n == 257 else SD_A[1:2]):
            for t in (0, 1):
                c = sd_case(n, A, bool(t), 12000 + 7 * n + A + t)
                c["adv"] = gref.trpo_adv(n, 400 + n + A)
                out["sd-n%d-A%d-tanh%d" % (n, A, t)] = ("sd", c, bool(t))
    return out


ETA_FLOOR = 1e-8


def vmpo_cases():
    """-> {id: (kind, case with "adv", tanh, dual, kl_reduce)}.  Beside the shapes: eta at its 1e-8 floor, all advantages
    equal, a dual state in the middle of a run (non-zero moments), and both kl_reduce values for both heads."""
    out = {}
    mid = (0.7, 0.05, 0.3, -0.02, 0.2, 0.001, 5.0)

    def add(name, kind, n, A, tanh, dual=DUAL0, red=None, adv=None, seed=0):
        c = cat_case(n, A, 13000 + 7 * n + A + seed) if kind == "cat" else sd_case(n, A, tanh, 14000 + 7 * n + A + int(tanh) + seed)
        c["adv"] = gref.vmpo_adv(n, 500 + n + A) if adv is None else adv
        out[name] = (kind, c, tanh, dual, (KL_SUM if kind == "cat" else KL_MEAN) if red is None else red)

    for n in NS:
        for A in (CAT_A if n == 257 else CAT_A[1:2]):
            add("cat-n%d-A%d" % (n, A), "cat", n, A, False)
        for A in (SD_A if n == 257 else SD_A[1:2]):
            for t in (0, 1):
                add("sd-n%d-A%d-tanh%d" % (n, A, t), "sd", n, A, bool(t))
    add("cat-mean", "cat", 257, 6, False, red=KL_MEAN)
    add("sd-sum", "sd", 257, 6, True, red=KL_SUM)
    add("cat-mid-run", "cat", 257, 6, False, dual=mid, seed=1)
    add("sd-mid-run", "sd", 257, 6, True, dual=mid, seed=1)
    floor = (ETA_FLOOR,) + DUAL0[1:]
    add("cat-eta-floor", "cat", 257, 6, False, dual=floor, seed=2)
    add("sd-eta-floor", "sd", 257, 6, False, dual=floor, seed=2)
    add("cat-equal-adv", "cat", 257, 6, False, adv=torch.full((257,), 0.25), seed=3)
    add("sd-equal-adv", "sd", 257, 6, True, adv=torch.full((257,), 0.25), seed=3)
    return out


HYPER = dict(eta_eps=0.02, alpha_eps=0.1, lr=1e-3)
C_ENT = 0.01


def small_mlp(D, H, O, seed, dtype=torch.float32):
    """[W1, b1, W2, b2, W3, b3] of a D-H-H-O Tanh MLP with weights of unit scale (a head that is far from linear)."""
    rs = np.random.RandomState(seed)
    shapes = [(H, D), (H,), (H, H), (H,), (O, H), (O,)]
    return [torch.from_numpy((rs.randn(*s) / math.sqrt(s[-1] if len(s) == 2 else 4.0)).astype(np.float32)).to(dtype) for s in shapes]


FVP_NETS = {"3-8-8": (3, 8, 40), "17-64-64": (17, 64, 257)}                  # D, H, batch; the head has 6 columns
# F v through the engine against double backward: the bound tests/test_trpo_gpu.py holds the Gaussian head's F v to
FVP_TOL = 2e-5


# ---------------------------------------------------------------- the whole updates over flat parameter lists
class _Adam:
    def __init__(self, params, lr, eps=1e-5):
        self.lr, self.eps, self.t = lr, eps, 0
        self.m, self.v = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]

    def step(self, params, grads):
        self.t += 1
        bc1, bc2 = 1 - 0.9 ** self.t, 1 - 0.999 ** self.t
        for p, g, m, v in zip(params, grads, self.m, self.v):
            m.mul_(0.9).add_(g, alpha=0.1)
            v.mul_(0.999).addcmul_(g, g, value=0.001)
            p.data.addcdiv_(m, (v.sqrt() / math.sqrt(bc2)).add_(self.eps), value=-self.lr / bc1)


def _clip(grads, max_norm):
    total = torch.sqrt(sum((g ** 2).sum() for g in grads))
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return [g * coef for g in grads], float(total)


def _update_terms(kind, params, obs, acts, tanh):
    """== pf.update(obs, acts): head, log_prob (n, 1), ent (n,) / (n, 1) as the reference's policies shape them."""
    head = mlp(obs, params)
    if kind == "cat":
        lp, ent = cat_terms(head, acts)[3:]
        return head, lp[:, None], ent
    lp, ent = sd_terms(head, acts, tanh)[2:]
    return head, lp[:, None], ent[:, None]


class HeadVMPO:
    """VMPO.update (v_mpo.py:57-181) with a categorical or [mean | log_std] policy, in `dtype`; the categorical KL as the
    reference executes it (summed over the half-batch)."""

    def __init__(self, kind, pf, vf, dtype=torch.float64, plr=1e-3, vlr=1e-3, eta_eps=0.02, alpha_eps=0.1, tanh_action=False):
        self.kind, self.dt, self.tanh = kind, dtype, tanh_action
        self.pf = [p.detach().to(dtype).clone().requires_grad_(True) for p in pf]
        self.vf = [p.detach().to(dtype).clone().requires_grad_(True) for p in vf]
        self.eta = torch.tensor([1.0], dtype=dtype, requires_grad=True)
        self.alpha = torch.tensor([0.1], dtype=dtype, requires_grad=True)
        self.pf_opt, self.vf_opt, self.param_opt = _Adam(self.pf, plr), _Adam(self.vf, vlr), _Adam([self.eta, self.alpha], plr)
        self.eta_eps, self.alpha_eps = eta_eps, alpha_eps
        self.sync_target()

    def sync_target(self):
        self.tpf = [p.detach().clone() for p in self.pf]

    def update(self, batch):
        f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(self.dt)
        obs, acts, advs, rets = f(batch["obs"]), f(batch["acts"]), f(batch["advs"]), f(batch["estimate_returns"])
        info = {"advs/mean": advs.mean().item(), "advs/std": advs.std().item(), "advs/max": advs.max().item(),
                "advs/min": advs.min().item()}
        advs = (advs - advs.mean()) / (advs.std() + 1e-5)
        vf_loss = ((mlp(obs, self.vf) - rets) ** 2).mean()
        g, gn = _clip(torch.autograd.grad(vf_loss, self.vf), 0.5)
        self.vf_opt.step(self.vf, g)
        info["Training/vf_loss"], info["grad_norm/vf"] = vf_loss.item(), gn
        idx = torch.sort(advs, dim=0, descending=True)[1].reshape(-1).long().chunk(2, dim=0)[0]
        obs, acts, advs = obs[idx], acts[idx], advs[idx]
        head, lp, _ = _update_terms(self.kind, self.pf, obs, acts, self.tanh)
        with torch.no_grad():
            thead = mlp(obs, self.tpf)
        phis = torch.softmax(advs / self.eta.detach(), dim=0)
        eta_loss = self.eta * self.eta_eps + self.eta * torch.log(torch.mean(torch.exp(advs / self.eta)))
        if self.kind == "cat":                                                # kl_divergence(Categorical, Categorical): (B',)
            lsm = torch.log_softmax(head, -1)
            kl = (lsm.exp() * (lsm - torch.log_softmax(thead, -1))).sum(-1).sum(-1, keepdim=True)
        else:
            mean, raw = sd_split(head)
            tmean, traw = sd_split(thead)
            kl = gref.kl_rows(mean, raw.clamp(-20.0, 2.0), tmean, traw.clamp(-20.0, 2.0))[:, None]
        alpha_loss = self.alpha * self.alpha_eps - self.alpha * kl.detach().mean()
        policy_loss = (-phis * lp + self.alpha.detach() * kl).mean()
        grads = torch.autograd.grad(policy_loss + eta_loss + alpha_loss, self.pf + [self.eta, self.alpha])
        g_pf, gn = _clip(grads[:-2], 0.5)
        self.pf_opt.step(self.pf, g_pf)
        self.param_opt.step([self.eta, self.alpha], list(grads[-2:]))
        with torch.no_grad():
            self.eta.clamp_(min=1e-8)
            self.alpha.clamp_(min=1e-8)
        k = kl.detach()
        info.update({"Training/policy_loss": policy_loss.item(), "Training/alpha_loss": alpha_loss.item(),
                     "Training/alpha": self.alpha.item(), "Training/eta": self.eta.item(),
                     "logprob/mean": lp.mean().item(), "logprob/std": lp.std().item(),
                     "logprob/max": lp.max().item(), "logprob/min": lp.min().item(),
                     "KL/mean": k.mean().item(), "KL/std": k.std().item() if k.numel() > 1 else float("nan"),
                     "KL/max": k.max().item(), "KL/min": k.min().item(), "grad_norm/pf": gn})
        return info


class HeadTRPO:
    """TRPO.update / update_vf (trpo.py:28-251) with a categorical or [mean | log_std] policy, in `dtype`.  After update():
    `search` = [(actual improvement, acceptance ratio), ...] of the line search's trials, `accepted` = the accepted
    backtrack index (-1: none), `grad_nonzero`."""

    def __init__(self, kind, pf, vf, dtype=torch.float64, vlr=1e-3, max_kl=0.01, cg_damping=0.1, cg_iters=10,
                 residual_tol=1e-10, entropy_coeff=0.01, tanh_action=False):
        self.kind, self.dt, self.tanh = kind, dtype, tanh_action
        self.pf = [p.detach().to(dtype).clone().requires_grad_(True) for p in pf]
        self.vf = [p.detach().to(dtype).clone().requires_grad_(True) for p in vf]
        self.vf_opt = _Adam(self.vf, vlr)
        self.max_kl, self.cg_damping, self.cg_iters, self.residual_tol = max_kl, cg_damping, cg_iters, residual_tol
        self.entropy_coeff = entropy_coeff

    def _flat(self):
        return torch.cat([p.detach().reshape(-1) for p in self.pf])

    def _unflat(self, theta):
        out, off = [], 0
        for p in self.pf:
            out.append(theta[off:off + p.numel()].view_as(p)); off += p.numel()
        return out

    def _fvp(self, v):
        g = torch.autograd.grad(mean_kl(self.kind, mlp(self.obs, self.pf), 1e-8), self.pf, create_graph=True)
        gv = torch.sum(torch.cat([x.reshape(-1) for x in g]) * v)
        h = torch.autograd.grad(gv, self.pf)
        return torch.cat([x.contiguous().reshape(-1) for x in h]) + self.cg_damping * v.detach()

    def _cg(self, b):
        p, r, x = b.clone(), b.clone(), torch.zeros_like(b)
        rdotr = r.double().dot(r.double())
        for _ in range(self.cg_iters):
            z = self._fvp(p)
            v = (rdotr / p.double().dot(z.double())).to(self.dt)
            x += v * p
            r -= v * z
            newrdotr = r.double().dot(r.double())
            p = r + (newrdotr / rdotr).to(self.dt) * p
            rdotr = newrdotr
            if rdotr < self.residual_tol:
                break
        return x

    def _surrogate(self, theta):
        with torch.no_grad():
            new = _update_terms(self.kind, self._unflat(theta.detach()), self.obs, self.acts, self.tanh)[1]
            old = _update_terms(self.kind, self.pf, self.obs, self.acts, self.tanh)[1]
            return -torch.mean(torch.exp(new - old) * self.advs)

    def _linesearch(self, x, fullstep, rate):
        fval = self._surrogate(x)
        self.search, self.accepted = [], -1
        for k, stepfrac in enumerate(.5 ** np.arange(10)):
            xnew = x + float(stepfrac) * fullstep
            actual = fval - self._surrogate(xnew)
            r = actual / (rate * float(stepfrac))
            self.search.append((float(actual), float(r)))
            if r > .1 and actual > 0:
                self.accepted = k
                return xnew
        return x.detach()

    def update(self, batch):
        f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(self.dt)
        self.obs, self.acts, advs = f(batch["obs"]), f(batch["acts"]), f(batch["advs"])
        info = {"advs/mean": advs.mean().item(), "advs/std": advs.std().item(), "advs/max": advs.max().item(),
                "advs/min": advs.min().item()}
        self.advs = (advs - advs.mean()) / (advs.std() + 1e-4)
        _, lp, ent = _update_terms(self.kind, self.pf, self.obs, self.acts, self.tanh)
        p_new = torch.exp(lp)
        loss = -torch.mean(p_new / (p_new.detach() + 1e-8) * self.advs) - self.entropy_coeff * ent.mean()
        g = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, self.pf)]).detach()
        self.grad_nonzero, self.search, self.accepted = bool(g.nonzero().size()[0]), [], -1
        if self.grad_nonzero:
            step = self._cg(-g)
            lm = torch.sqrt(.5 * step.dot(self._fvp(step)) / self.max_kl)
            theta = self._linesearch(self._flat(), step / lm, -g.dot(step) / lm)
            if not torch.isnan(theta).any():
                with torch.no_grad():
                    for p, q in zip(self.pf, self._unflat(theta)):
                        p.copy_(q)
        info.update({"Training/policy_loss": loss.item(), "logprob/mean": lp.mean().item(), "logprob/std": lp.std().item(),
                     "logprob/max": lp.max().item(), "logprob/min": lp.min().item()})
        return info

    def update_vf(self, batch):
        f = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(self.dt)
        obs, rets = f(batch["obs"]), f(batch["estimate_returns"])
        vf_loss = 0.5 * ((mlp(obs, self.vf) - rets) ** 2).mean()
        g, gn = _clip(torch.autograd.grad(vf_loss, self.vf), 0.5)
        self.vf_opt.step(self.vf, g)
        return {"Training/vf_loss": vf_loss.item(), "grad_norm/vf": gn}


# ---------------------------------------------------------------- the measurement behind K
def measure():
    """-> {key of K: the largest err / M of the float32 run against the float64 run over all cases}."""
    worst = {k: 0.0 for k in K}

    def up(key, r):
        worst[key] = max(worst[key], r)

    for name, (kind, c, tanh) in trpo_cases().items():
        want = trpo_surrogate(kind, c["head"].double(), c["acts"].double(), c["adv"].double(), tanh, C_ENT)
        got = trpo_surrogate(kind, c["head"], c["acts"], c["adv"], tanh, C_ENT)
        up("trpo_%s_d_head" % kind, ratio(got["d_head"], want["d_head"], want["mag"]["d_head"]))
        up("trpo_%s_info" % kind, ratio(got["info"], want["info"], want["mag"]["info"]))
        t = F32(np.random.RandomState(5).randn(*c["head"].shape))
        w_out, w_mag = fisher_scale(kind, t.double(), c["head"].double())
        up("fisher_" + kind, ratio(fisher_scale(kind, t, c["head"])[0], w_out, w_mag))
    for name, (kind, c, tanh, dual, red) in vmpo_cases().items():
        args = lambda dt: (kind, c["head"].to(dt), c["thead"].to(dt), c["acts"].to(dt), c["adv"].to(dt),
                           np.asarray(dual, dtype=np.float32), tanh, red)
        want, got = vmpo_losses(*args(torch.float64), **HYPER), vmpo_losses(*args(torch.float32), **HYPER)
        up("vmpo_%s_d_head" % kind, ratio(got["d_head"], want["d_head"], want["mag"]["d_head"]))
        up("vmpo_%s_info" % kind, ratio(got["info"][:10], want["info"][:10], want["mag"]["info"]))
        up("vmpo_%s_g" % kind, ratio(got["g"], want["g"], want["mag"]["g"]))
    return worst


if __name__ == "__main__":
    for key, val in measure().items():
        print("%-18s measured %.3e   x4 = %.3e   K = %.3e" % (key, val, 4 * val, K[key]))
