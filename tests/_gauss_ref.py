"""Plain restatements (CPU; torch in float32 or float64, numpy for the integer bookkeeping) of the oldest kernel family:
the generic on-policy loss kernel for a state-independent-std Gaussian policy (torchrl_amd/csrc/k_ppo_generic.hip), the
per-step collection kernels beside it (k_rollout.hip: explore / log-prob / bookkeeping / select; k_sac.hip: the off-policy
collector's bookkeeping and select) and the running observation normaliser (k_norm.hip) -- test infrastructure, imported
by tests/test_gauss_collector_kernels_*.py only.

log pi, the entropy and the gate / tie conventions are those of tests/_gauss_sd_ref.py with one log_std row shared by all
samples; the advantage is normalised from given raw sums and n_global (what a rank sees under data parallelism), and the
objectives are sums over the B local samples divided by n_global."""
import math

import numpy as np
import torch

import _gauss_sd_ref as sd
from _categorical_ref import LOSS_PPO_CLIP, LOSS_A2C                                   # noqa: F401

HALF_LOG_2PI = sd.HALF_LOG_2PI
U = 2.0 ** -24                                                                          # float32 unit round-off
SENTINEL = -777.25                                                                      # info slots the fold leaves alone
SUM_SLOTS = (0, 1, 2, 7, 12, 13)
COMBOS = [(True, LOSS_PPO_CLIP, False), (False, LOSS_PPO_CLIP, True), (True, LOSS_A2C, False), (False, LOSS_A2C, True)]
CROSS = [(t, m, c) for t in (True, False) for m in (LOSS_PPO_CLIP, LOSS_A2C) for c in (False, True)]
LOSS_B, LOSS_A = (2, 64, 255, 256, 257, 700), (1, 6, 33, 64)
EXPLORE_N, EXPLORE_A = (1, 255, 256, 257, 1000), (1, 6, 64)
BOOK_N = (1, 63, 64, 65, 256, 257, 1000)
NORM_D, NORM_N = (1, 3, 17, 33, 64), (1, 2, 15, 1000, 5000)
NORM_STATE_RTOL, NORM_OUT_RTOL, NORM_OUT_ATOL = 1e-11, 2e-7, 1e-7


# ------------------------------------------------------------------ log pi, explore
def head_of(mean, logstd):
    """(B, A) means and the shared (A,) log_std as the (B, 2A) head of tests/_gauss_sd_ref.py."""
    return torch.cat([mean, logstd.reshape(1, -1).expand(mean.shape[0], -1)], dim=1)


def _rows(logstd):
    """A shared (A,) log_std as one broadcast row; a per-sample (B, A) one as it is."""
    return logstd if logstd.dim() == 2 else logstd.reshape(1, -1)


def logp_parts(mean, logstd, acts, tanh):
    """-> dict of (B, A) tensors: quad = zc^2 / (2 var), ls (clamped), corr, zc, var; log pi = sum(-quad - ls - log(2 pi) / 2
    - corr), sd.logp's formula.  `logstd` is the shared (A,) row, or (B, A): one raw log_std per sample and dim (a
    state-dependent-std head)."""
    ls = _rows(logstd.clamp(-20.0, 2.0)).expand_as(mean)
    var = torch.exp(ls) ** 2
    pre, corr = acts, torch.zeros_like(mean)
    if tanh:
        pre = 0.5 * torch.log((1.0 + acts) / (1.0 - acts))
        corr = torch.log((1.0 - acts) * (1.0 + acts) + 1e-6)       # 1 - a^2 without the cancellation (the kernel: one fma)
    zc = pre - mean
    return dict(quad=zc * zc / (2.0 * var), ls=ls, corr=corr, zc=zc, var=var)


def logp(mean, logstd, acts, tanh):
    p = logp_parts(mean, logstd, acts, tanh)
    return (-p["quad"] - p["ls"] - HALF_LOG_2PI - p["corr"]).sum(-1)


def explore(mean, logstd, eps, tanh):
    """-> (act (N, A), log pi(act) (N,)); eps None: the deterministic action [tanh](mean).  The std is exp of the CLAMPED
    log_std."""
    std = _rows(torch.exp(logstd.clamp(-20.0, 2.0)))
    z = mean if eps is None else mean + std * eps
    act = torch.tanh(z) if tanh else z
    return act, logp(mean, logstd, act, tanh)


def act_bound(mean, logstd, eps, tanh):
    """|act - float64 act| of z = fma(__expf(ls), eps, mean), a = [trl_tanh](z), from float64 inputs.  __expf(x) =
    exp2(x log2 e): the rounded product puts |x| 2^-23 into the result and the hardware exp2 one ulp, (2 + |ls|) 2^-23
    relative on the std (profiles/NOTES_offpolicy_kernel_tests.md, alpha); the fma rounds once, 2^-24 |z|; trl_tanh is
    within 2e-7 absolute (trl_mlp.h) and has slope <= 1."""
    ls = _rows(logstd.double().clamp(-20.0, 2.0))
    se = torch.exp(ls) * (0.0 if eps is None else eps.double())
    z = mean.double() + se
    return se.abs() * (2.0 + ls.abs()) * 2.0 * U + U * z.abs() + (2e-7 if tanh else 0.0)


def logp_bound(mean, logstd, acts, tanh):
    """|log pi - float64 log pi| at the SAME float32 action, per sample.  Per dimension 2^-23 (4 |quad| + |ls| + |corr| + 1):
    quad = zc^2 * 0.5 * exp(-2 ls) carries the rounding of zc twice, of the square and of the two products; the other
    terms round once each.  Tanh actions: zc carries the absolute atanh error d = 5e-7 that tests/test_gauss_sd_gpu.py
    derives for |a| <= 0.995, which moves quad = zc^2 / (2 var) by |zc| d / var to first order.  (The second-order part
    d^2 / (2 var) is 2.5e-12 at log_std = -1.5.  In a column clamped at -20, var = e^-40, it is 3e4: there log pi of a
    tanh action is float32 atanh noise divided by e^-40 and no bound on it says anything, so the tests compare tanh log
    pi under `logstd_lp`, which has no such column.)  The A additions: A 2^-24 of the sum of the absolute terms."""
    p = logp_parts(mean.double(), logstd.double(), acts.double(), tanh)
    quad, ls, corr = p["quad"].abs(), p["ls"].abs(), p["corr"].abs()
    per = 2.0 * U * (4.0 * quad + ls + corr + 1.0)
    if tanh:
        per = per + p["zc"].abs() * 5e-7 / p["var"]
    A = mean.shape[1]
    return per.sum(-1) + A * U * (quad + ls + HALF_LOG_2PI + corr).sum(-1)


def explore_case(N, A, tanh, seed):
    """Means 0.5 N(0, 1), log_std uniform in [-1.5, 0.5] with entry 0 at -25 and entry A - 1 at +3 (A = 1: -25 for tanh
    actions, +3 otherwise), eps N(0, 1).  For tanh actions the +3 column's eps is scaled by 0.1: with std e^2 a unit
    normal would saturate two thirds of the rows, and the clamp still shows (e^3 / e^2 = 2.7 in that column's step).
    `logstd_lp` is what log pi is compared with float64 under: for tanh actions the -25 entry keeps its uniform draw instead
    (see `logp_bound`); otherwise it is `logstd`.  The draw is repeated with the next seed until at least max(1, N / 4)
    rows have every |tanh(z)| <= 0.995 under both (`logp_keep`)."""
    for attempt in range(64):
        rs = np.random.RandomState(seed + 7919 * attempt)
        mean = torch.from_numpy((0.5 * rs.randn(N, A)).astype(np.float32))
        logstd = torch.from_numpy(rs.uniform(-1.5, 0.5, (A,)).astype(np.float32))
        eps = torch.from_numpy(rs.randn(N, A).astype(np.float32))
        logstd_lp = logstd.clone()
        if A == 1:
            logstd[0] = -25.0 if tanh else 3.0
        else:
            logstd[0], logstd[A - 1] = -25.0, 3.0
        if tanh and float(logstd[A - 1]) == 3.0:
            eps[:, A - 1] *= 0.1
        if tanh:
            logstd_lp[1:] = logstd[1:]
        else:
            logstd_lp = logstd.clone()
        zmax = lambda ls: (mean.double() + torch.exp(ls.double().clamp(-20.0, 2.0)) * eps.double()).abs().max(dim=1)[0]
        kept = int(((zmax(logstd) < 2.9) & (zmax(logstd_lp) < 2.9)).sum())                  # atanh(0.995) = 2.994
        if not tanh or kept >= max(1, N // 4):
            return dict(mean=mean, logstd=logstd, eps=eps, logstd_lp=logstd_lp)
    raise AssertionError("no inputs meet the conditions")


def big_z_case(N, A, seed):
    """Tanh actions with pre-tanh values z = +-U(3, 7), planted through the means: mean = z - std eps, log_std uniform in
    [-1.5, -0.5], eps N(0, 1) clipped to +-2."""
    rs = np.random.RandomState(seed)
    logstd = torch.from_numpy(rs.uniform(-1.5, -0.5, (A,)).astype(np.float32))
    eps = torch.from_numpy(np.clip(rs.randn(N, A), -2, 2).astype(np.float32))
    z = rs.uniform(3.0, 7.0, (N, A)) * rs.choice([-1.0, 1.0], (N, A))
    z[0, 0], z[N - 1, A - 1] = 7.0, -7.0
    mean = torch.from_numpy(z - np.exp(logstd.double().numpy())[None] * eps.double().numpy()).float()
    return dict(mean=mean, logstd=logstd, eps=eps)


def logp_keep(act, tanh):
    """Rows the float64 comparison of log pi covers: for tanh actions those with every |a| <= 0.995, the range the atanh
    part of `logp_bound` is derived for."""
    if not tanh:
        return torch.ones(act.shape[0], dtype=torch.bool)
    return act.abs().max(dim=1)[0] <= 0.995


# ------------------------------------------------------------------ the loss half
def adv_raw_of(pop):
    """The four raw advantage statistics of trl_adv_stats_f64 over a population: sum, sum of squares, max, -min (float64)."""
    a = pop.double().reshape(-1)
    return torch.stack([a.sum(), (a * a).sum(), a.max(), -a.min()])


def adv_normalize(advs, adv_raw, n_global):
    """_categorical_ref.adv_normalize from given raw sums: mean and 1 / (unbiased std + 1e-5) in float64, applied in the
    dtype of advs."""
    s, sq, ng = float(adv_raw[0]), float(adv_raw[1]), float(n_global)
    mean = torch.tensor(s / ng, dtype=torch.float64)
    var = torch.tensor((sq - s * s / ng) / (ng - 1.0), dtype=torch.float64)
    mu = mean.to(advs.dtype)
    rstd = 1.0 / (torch.sqrt(var.clamp(min=0.0)).to(advs.dtype) + 1e-5)
    return (advs.reshape(-1) - mu) * rstd


def losses(mean, v, logstd, acts, advs, rets, v_old, old_logp, adv_raw, n_global, clip_para, entropy_coeff,
           clipped_value_loss, loss_mode, tanh):
    """The loss half of one minibatch in the dtype of `mean`: -> dict(d_mean (B, A), d_logstd (A,), d_v (B,), info (24
    float64 in ppo_generic_fold_kernel's layout, SENTINEL where that kernel writes nothing for a Gaussian head),
    dls_terms (B, A): the per-sample terms whose sum is d_logstd, lp, ratio, advn, ent: the entropy of one sample)."""
    mean = mean.detach().clone().requires_grad_(True)
    logstd = logstd.detach().clone().requires_grad_(True)
    v = v.detach().clone().reshape(-1).requires_grad_(True)
    B, A = mean.shape
    ng = float(n_global)
    ls = logstd.clamp(-20.0, 2.0)
    lp = logp(mean, logstd, acts, tanh)
    ent = (0.5 + HALF_LOG_2PI + ls).sum()
    advn = adv_normalize(advs, adv_raw, ng).detach()
    if loss_mode == LOSS_A2C:
        ratio = torch.ones_like(lp)
        surr = -(lp * advn)
    else:
        ratio = torch.exp(lp - old_logp.reshape(-1))
        surr = -torch.minimum(ratio * advn, ratio.clamp(1.0 - clip_para, 1.0 + clip_para) * advn)
    pl = surr.sum() / ng - entropy_coeff * ent * (B / ng)
    R = rets.reshape(-1)
    if clipped_value_loss:
        vo = v_old.reshape(-1)
        vc = vo + (v - vo).clamp(-clip_para, clip_para)
        vloss = 0.5 * torch.maximum((v - R) ** 2, (vc - R) ** 2)
    else:
        vloss = (v - R) ** 2
    vl = vloss.sum() / ng
    d_mean, d_logstd, g_lp = torch.autograd.grad(pl, [mean, logstd, lp], retain_graph=True)
    d_v, = torch.autograd.grad(vl, v)
    d = lambda t: t.detach().double()
    p = logp_parts(d(mean), d(logstd), acts.double(), tanh)
    raw = d(logstd)
    gate = ((raw >= -20.0) & (raw <= 2.0)).double().reshape(1, -1)
    dls_terms = gate * (d(g_lp).reshape(-1, 1) * (p["zc"] ** 2 / p["var"] - 1.0) - entropy_coeff / ng)
    lp64, r64, v64 = d(lp), d(ratio), d(v)
    info = np.full(24, SENTINEL)
    info[0:8] = [d(surr).sum(), lp64.sum(), (lp64 * lp64).sum(), lp64.max(), -lp64.min(), r64.max(), -r64.min(),
                 d(vloss).sum()]
    info[12:16] = [v64.sum(), (v64 * v64).sum(), v64.max(), -v64.min()]
    x = d(ls)
    for base, t in ((8, x), (16, torch.exp(x))):
        info[base:base + 4] = [t.mean(), t.std() if A > 1 else float("nan"), t.max(), t.min()]
    return dict(d_mean=d_mean, d_logstd=d_logstd, d_v=d_v, info=info, dls_terms=dls_terms, lp=lp.detach(),
                ratio=ratio.detach(), advn=advn, ent=ent.detach())


def loss_case(B, A, tanh, seed, n_mult=1, clip=0.2):
    """Seeded float32 inputs of one minibatch, generated like loss_case of tests/test_gauss_sd_gpu.py with a shared log_std:
    means 0.5 N(0, 1), log_std uniform in [-1.5, 0.5], actions drawn from the head itself (tanh actions clamped to
    +-0.995), log pi_old = log pi + 0.3 N(0, 1); samples whose float64 ratio is within 2e-3 of a clip boundary have
    log pi_old moved by 0.05.  n_mult = 3: the advantages are a population of 3 B of which the kernel sees the middle third
    (n_global = 3 B).  The draw is repeated with the next seed until the inputs meet `loss_case_conditions`."""
    for attempt in range(64):
        rs = np.random.RandomState(seed + 7919 * attempt)
        t = lambda *s: torch.from_numpy(rs.randn(*s).astype(np.float32))
        mean = t(B, A) * 0.5
        logstd = torch.from_numpy(rs.uniform(-1.5, 0.5, (A,)).astype(np.float32))
        acts = explore(mean, logstd, t(B, A), tanh)[0]
        if tanh:
            acts = acts.clamp(-0.995, 0.995)
        pop = t(n_mult * B) * 2 + 0.5
        lo = (n_mult // 2) * B
        v, advs, rets, v_old = t(B), pop[lo:lo + B].clone(), t(B), t(B)
        lp64 = logp(mean.double(), logstd.double(), acts.double(), tanh)
        old = lp64 + 0.3 * t(B).double()
        ratio = torch.exp(lp64 - old)
        near = ((ratio - (1.0 - clip)).abs() < 2e-3) | ((ratio - (1.0 + clip)).abs() < 2e-3)
        old = torch.where(near, old + 0.05, old).float()
        c = dict(mean=mean, logstd=logstd, acts=acts.contiguous(), v=v, advs=advs, rets=rets, v_old=v_old, old=old,
                 adv_raw=adv_raw_of(pop), n_global=float(n_mult * B), moved=int(near.sum()), attempts=attempt + 1)
        if not loss_case_conditions(c, tanh, clip):
            return c
    raise AssertionError("no inputs meet the conditions")


def loss_case_conditions(c, tanh, clip=0.2):
    """What the grid's inputs guarantee; -> list of the violated conditions (empty: all hold)."""
    B = c["mean"].shape[0]
    ratio = torch.exp(logp(c["mean"].double(), c["logstd"].double(), c["acts"].double(), tanh) - c["old"].double())
    bad = []
    if c["moved"] > 0.02 * B:
        bad.append("moved %d of %d" % (c["moved"], B))
    if bool((((ratio - (1 - clip)).abs() < 1e-3) | ((ratio - (1 + clip)).abs() < 1e-3)).any()):
        bad.append("a ratio within 1e-3 of a clip boundary")
    if B >= 64:
        lo, hi = int((ratio < 1 - clip).sum()), int((ratio > 1 + clip).sum())
        if lo < 0.1 * B or hi < 0.1 * B:
            bad.append("clipped %d below, %d above of %d" % (lo, hi, B))
    if tanh and float(c["acts"].abs().max()) > float(np.float32(0.995)):
        bad.append("|a| > 0.995")
    return bad


def loss_args(c, loss_mode, clipv):
    """(old_logp, v_old) a call with these modes is given."""
    return (c["old"] if loss_mode == LOSS_PPO_CLIP else None), (c["v_old"] if clipv else None)


def run_losses_ref(c, tanh, loss_mode, clipv, dtype, clip=0.2, c_ent=0.01):
    t = lambda x: None if x is None else x.to(dtype)
    old, v_old = loss_args(c, loss_mode, clipv)
    return losses(t(c["mean"]), t(c["v"]), t(c["logstd"]), t(c["acts"]), t(c["advs"]), t(c["rets"]), t(v_old), t(old),
                  c["adv_raw"], c["n_global"], clip, c_ent, clipv, loss_mode, tanh)


def loss_error_ratios(got, want, B, n_global):
    """Worst err / bound of d_mean, d_v, d_logstd and the info row of `got` (dict of float64 tensors / array) against the
    float64 restatement `want`.  d_mean rel 1e-4 abs 1e-4 / n_global, d_v rel 1e-5 abs 1e-6 / n_global (the derivation in
    tests/test_gauss_sd_gpu.py::test_losses_vs_restatement_in_float64, same input ranges); d_logstd[o] is a sum of B terms
    that each carry the log-std half's bound: 1e-4 B / n_global + 1e-4 sum_b |term_b,o|; scalars rel 1e-4, abs 1e-5 (times B
    on slots that hold sums); NaN and sentinel slots must be equal."""
    ng = float(n_global)
    out = {}
    for name, rel, ab in (("d_mean", 1e-4, 1e-4 / ng), ("d_v", 1e-5, 1e-6 / ng)):
        w = want[name].double().reshape(-1)
        out[name] = float(((got[name].double().reshape(-1) - w).abs() / (ab + rel * w.abs())).max())
    w = want["d_logstd"].double()
    bound = 1e-4 * B / ng + 1e-4 * want["dls_terms"].abs().sum(0)
    out["d_logstd"] = float(((got["d_logstd"].double() - w).abs() / bound).max())
    out["info"] = info_error_ratio(got["info"], want["info"], B)
    return out


def info_error_ratio(got, want, B):
    """Worst err / bound over the 24 info slots: rel 1e-4, abs 1e-5 (times B on slots that hold sums); NaN and sentinel slots
    must be equal."""
    worst = 0.0
    for k in range(24):
        g, w = float(got[k]), float(want[k])
        if math.isnan(w) or w == SENTINEL:
            ok = (math.isnan(g) and math.isnan(w)) or g == w
            worst = max(worst, 0.0 if ok else float("inf"))
        else:
            worst = max(worst, abs(g - w) / ((1e-5 * B if k in SUM_SLOTS else 1e-5) + 1e-4 * abs(w)))
    return worst


def value_tie_case(clip=0.25):
    """Rows on a grid of 1/8 (float32 and float64 see the same comparisons), clip 0.25:  v == v_old (l1 == l2, weight 0.5
    each); v - v_old == +clip and == -clip (closed interval, gate open: the clipped value is v itself, l1 == l2);
    |v - v_old| > clip with l1 > l2, with l1 < l2, and with R half way between v and the clipped value (l1 == l2 with the
    gate closed: the only rows on which the tie weight shows, d_v n = (v - R) / 2).  -> dict(v, v_old, rets, kind)."""
    rows = [  # v, v_old, R, kind
        (1.0, 1.0, 0.5, "tie"), (-0.5, -0.5, -0.5, "tie"), (2.0, 2.0, 3.125, "tie"),
        (1.25, 1.0, 0.0, "gate+"), (0.75, 1.0, 2.0, "gate-"), (-1.0, -1.25, -3.0, "gate+"), (0.5, 0.75, 0.125, "gate-"),
        (2.0, 1.0, 0.0, "out_l1"), (-1.5, -0.5, 1.0, "out_l1"),           # clipped value nearer to R: l1 > l2, weight on l1
        (2.0, 1.0, 3.0, "out_l2"), (-1.5, -0.5, -2.5, "out_l2"),          # clipped value farther: l2 wins, gate closed
        (2.0, 1.0, 1.625, "out_tie"), (-1.5, -0.5, -1.125, "out_tie"),
        (0.125, 0.0, 1.0, "in"), (0.0, 0.125, -1.0, "in")]
    f = lambda i: torch.tensor([r[i] for r in rows], dtype=torch.float32)
    return dict(v=f(0), v_old=f(1), rets=f(2), kind=[r[3] for r in rows], clip=clip)


# ------------------------------------------------------------------ bookkeeping (numpy, a dozen lines each)
def bookkeep_case(N, seed, max_frames=10):
    """Rewards and next values on a grid of 1/8 in [-4, 4] (any order of additions is exact in float64 and in float32 up
    to 2^21 terms); planted rows, cyclically from env 0: done only, over-length only with cur_step + 1 == max_frames and
    > max_frames, both, neither, cur_step + 1 == max_frames - 1; the rest random with one done in five."""
    rs = np.random.RandomState(seed)
    g = lambda: (rs.randint(-32, 33, N) / 8.0).astype(np.float32)
    rew, v_next, ep_return = g(), g(), g()
    done = (rs.rand(N) < 0.2).astype(np.float32)
    cur = rs.randint(0, max_frames - 2, N).astype(np.int32)
    plant = [(1.0, 3), (0.0, max_frames - 1), (0.0, max_frames + 2), (1.0, max_frames - 1), (0.0, 2), (0.0, max_frames - 2)]
    kinds = ["done", "over_eq", "over_gt", "both", "neither", "one_short"]
    kind = ["random"] * N
    for n in range(min(N, 12)):
        done[n], cur[n] = plant[n % 6]
        kind[n] = kinds[n % 6]
    return dict(rew=rew, done=done, v_next=v_next, cur_step=cur, ep_return=ep_return, max_frames=max_frames, kind=kind)


def bookkeep(c, step, discount=None):
    """One call of onpolicy_bookkeep_kernel (discount given) / collector_bookkeep_kernel (None) -> dict of the outputs;
    `log` is the list of (step, env, return) of the finished episodes, `rew64` the float64 value of the new rewards."""
    raw, d = c["rew"], c["done"] != 0
    cs = c["cur_step"] + 1
    er = (c["ep_return"] + raw).astype(np.float32)
    log = [(float(step), float(n), float(er[n])) for n in np.nonzero(d)[0]]
    er = np.where(d, np.float32(0), er)
    surpass = cs >= c["max_frames"]
    flag = d | surpass
    out = dict(cur_step=np.where(flag, 0, cs).astype(np.int32), ep_return=er, mask=flag.astype(np.uint8), log=log,
               epoch=float(raw.astype(np.float64).sum()), any=int(flag.any()))
    if discount is not None:
        out["surpass"] = surpass
        out["terminals"] = flag.astype(np.float32)
        out["rew64"] = raw.astype(np.float64) + float(np.float32(discount)) * c["v_next"].astype(np.float64) * surpass
    return out


# ------------------------------------------------------------------ normaliser (base_wrapper.py:44-89)
def norm_init(D):
    return np.zeros(D), np.ones(D), 1e-4


def norm_update(state, x):
    """Two-pass batch mean / population variance in float64, then the Chan merge of base_wrapper.py."""
    mean, var, count = state
    x = np.asarray(x, dtype=np.float64)
    bn = x.shape[0]
    bmean = x.mean(0)
    bvar = ((x - bmean) ** 2).mean(0)
    delta, tot = bmean - mean, count + bn
    m2 = var * count + bvar * bn + delta * delta * count * bn / tot
    return mean + delta * bn / tot, m2 / tot, tot


def norm_filt(state, x, clip):
    mean, var, _ = state
    return np.clip((np.asarray(x, dtype=np.float64) - mean) / (np.sqrt(var) + 1e-4), -clip, clip)


def norm_state_vec(state):
    return np.concatenate([state[0], state[1], [state[2]]])


def norm_batches(D, N, seed):
    """Three batches, like tests/test_obsnorm_gpu.py: scale 1 + k, offset 0.1 k.  A batch is drawn again until
    amplification * chain * 2^-53 of its sums about the running mean (the shard kernels' one pass) is below the state
    tolerance (N = 2 with two nearly equal rows in one of 64 features is not)."""
    rs = np.random.RandomState(seed)
    out, state = [], norm_init(D)
    for k in range(3):
        for attempt in range(64):
            x = (rs.randn(N, D) * (1 + k) + 0.1 * k).astype(np.float32)
            if N == 1 or norm_conditioning(x, N, D, state[0])[2] <= 0.5 * NORM_STATE_RTOL:
                break
        else:
            raise AssertionError("no inputs meet the conditions")
        out.append(x)
        state = norm_update(state, x)
    return out


def norm_chain(N, D):
    """Longest chain of additions of norm_block_moments: a row lane's ceil(N / R) rows, then the R lanes in turn."""
    R = 1024 // D
    return -(-N // R) + min(R, N)


def norm_kernel_moments(x, shift):
    """sum (x - shift) and sum (x - shift)^2 per feature in float64 IN THE KERNEL'S ORDER (norm_block_sums), on the CPU."""
    x = np.asarray(x, dtype=np.float64) - shift
    N, D = x.shape
    R = 1024 // D
    s, q = np.zeros(D), np.zeros(D)
    for r in range(min(R, N)):
        a, b = np.zeros(D), np.zeros(D)
        for n in range(r, N, R):
            a = a + x[n]
            b = b + x[n] * x[n]
        s, q = s + a, q + b
    return s, q


def norm_update_kernel(state, x, mode="batch"):
    """The kernels' update in their order of additions, then the Chan merge.  mode "batch": two passes, sum x and then the
    sums about the batch mean (trl_norm_update_filt_f32, trl_norm_batch_moments_f64 + trl_norm_merge_f64); "running": one
    pass about the running mean (trl_norm_shard_moments_f64 + trl_norm_shard_merge_f64); "zero": one pass about zero, what
    the kernels did before these tests."""
    mean, var, count = state
    bn = np.asarray(x).shape[0]
    if mode == "batch":
        sx, _ = norm_kernel_moments(x, 0.0)
        s, q = norm_kernel_moments(x, sx / bn)
        delta, bvar = sx / bn - mean, np.maximum(q - s * s / bn, 0.0) / bn
    else:
        s, q = norm_kernel_moments(x, mean if mode == "running" else 0.0)
        bmean = s / bn
        delta, bvar = (bmean if mode == "running" else bmean - mean), np.maximum(q / bn - bmean * bmean, 0.0)
    tot = count + bn
    return mean + delta * bn / tot, (var * count + bvar * bn + delta * delta * count * bn / tot) / tot, tot


def norm_warm_state(x):
    """The state of a normaliser that has seen only batches like x: their float64 mean and population variance, count N."""
    x = np.asarray(x, dtype=np.float64)
    return x.mean(0), x.var(0), float(x.shape[0])


def norm_conditioning_batches(N, D, seed):
    """Observations 1000 + 0.01 N(0, 1): two batches, the first to warm the state."""
    rs = np.random.RandomState(seed)
    return [(1000.0 + 0.01 * rs.randn(N, D)).astype(np.float32) for _ in range(2)]


def norm_conditioning(x, N, D, shift=0.0):
    """(amplification, chain, bound): a relative error chain 2^-53 of sum (x - shift)^2 is amplified by (m^2 + var) / var,
    m = mean - shift, in the batch variance E[(x - shift)^2] - E[x - shift]^2 (tests/_offpolicy_ref.py::
    moments_conditioning, the std's factor without the root's half)."""
    x = np.asarray(x, dtype=np.float64) - shift
    amp = float(((x.mean(0) ** 2 + x.var(0)) / x.var(0)).max())
    chain = norm_chain(N, D)
    return amp, chain, amp * chain * 2.0 ** -53
