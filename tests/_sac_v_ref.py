"""float64 restatement of the value-network soft actor-critics (SAC, TwinSAC), written from their formulas:

    head = pf(obs) = [mean | log_std], ls = clamp(log_std, -20, 2), sd = exp(ls), z = mean + sd eps, a = tanh(z)
    logp = sum_o(-eps_o^2 / 2 - ls_o - log sqrt(2 pi) - log(1 - a_o^2 + 1e-6))
    temperature: loss = -mean(log_alpha (logp + H)); one Adam step on log_alpha; alpha = exp(log_alpha) AFTER it
    q_target = r + (1 - d) gamma V'(s')                       qf_i loss = mean((Q_i(s, act) - q_target)^2)
    qn = min_i Q_i(s, a)                                      vf loss = mean((V(s) - (qn - alpha logp))^2)
    policy loss = mean(alpha logp - qn) + w_std mean(ls^2) + w_mean mean(mean^2)
    clip_grad_norm_ and Adam per network in the order pf, qf(1, 2), vf; V' <- (1 - tau) V' + tau V

`samples_ref` / `losses_ref` / `moments_ref` restate the two kernels trl_sacv_samples_f32 and trl_sacv_losses_f32;
`Update` is one whole update by explicit chain rule (no autograd).  numpy only.
"""
import os

import numpy as np

U = 2.0 ** -24                                                           # half an ulp of 1.0 in fp32
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("sac_h128", "twin_h128", "sac_reg", "twin_reg", "twin_fixed")
D, A = 17, 6
BATCH_KEYS = ("obs", "next_obs", "acts", "rewards", "terminals")

_fixture = None


def load_fixture():
    """sac_v_update.npz and the per-case files beside it as one mapping (loaded once, never modified)."""
    global _fixture
    if _fixture is None:
        main = np.load(os.path.join(GOLDEN, "sac_v_update.npz"), allow_pickle=False)
        out = {k: main[k] for k in main.files}
        for tag in (str(t) for t in main["cases"]):
            path = os.path.join(GOLDEN, "sac_v_update_%s.npz" % tag)
            if os.path.exists(path):
                part = np.load(path, allow_pickle=False)
                out.update({k: part[k] for k in part.files})
        _fixture = out
    return _fixture


def net_names(g, tag):
    return ("pf", "qf", "vf") if str(g[tag + "_class"]) == "SAC" else ("pf", "qf1", "qf2", "vf")


def state_dict_of(g, prefix):
    """{state-dict key: array} of one stored network."""
    return {k[len(prefix):].replace("__", "."): g[k] for k in g if k.startswith(prefix)}


def layers_of(g, prefix):
    """[(W, b), ...] float64 of one stored network, trunk first, head last."""
    sd = state_dict_of(g, prefix)
    ws = sorted((k for k in sd if k.endswith(".weight")), key=lambda k: (not k.startswith("base."), k))
    return [(sd[k].astype(np.float64), sd[k[:-6] + "bias"].astype(np.float64)) for k in ws]


# ------------------------------------------------------------------ the two kernels
def samples_ref(head, eps, obs, acts, tanh_action=True):
    head, eps, obs, acts = (np.asarray(t, dtype=np.float64) for t in (head, eps, obs, acts))
    n_a = eps.shape[1]
    mean, ls = head[:, :n_a], np.clip(head[:, n_a:], -20.0, 2.0)
    z = mean + np.exp(ls) * eps
    lp = -0.5 * eps * eps - ls - HALF_LOG_2PI
    act = z
    if tanh_action:
        act = np.tanh(z)
        lp = lp - np.log(1.0 - act * act + 1e-6)
    return act, lp.sum(1), np.concatenate([obs, acts], 1), np.concatenate([obs, act], 1)


def losses_ref(q1, q2, tv, rew, term, v, q1n, q2n, logp, alpha, gamma, n):
    """dict(dq1, dq2, dv, dq1n, dq2n, sums[5], and the per-row terms the error bounds are made of); q2 = q2n = None: one
    critic."""
    f = lambda t: None if t is None else np.asarray(t, dtype=np.float64).reshape(-1)
    q1, q2, tv, rew, term, v, q1n, q2n, logp = (f(t) for t in (q1, q2, tv, rew, term, v, q1n, q2n, logp))
    qt = rew + (1.0 - term) * gamma * tv
    out = {"e1": q1 - qt, "dq1": 2.0 * (q1 - qt) / n, "dq2": None, "dq2n": None, "e2": None}
    if q2 is None:
        qn = q1n
        out["dq1n"] = np.full_like(q1n, -1.0 / n)
    else:
        qn = np.minimum(q1n, q2n)
        out["e2"], out["dq2"] = q2 - qt, 2.0 * (q2 - qt) / n
        out["dq1n"] = -np.where(q1n < q2n, 1.0, np.where(q1n == q2n, 0.5, 0.0)) / n
        out["dq2n"] = -np.where(q2n < q1n, 1.0, np.where(q1n == q2n, 0.5, 0.0)) / n
    ev = v - (qn - alpha * logp)
    out.update(ev=ev, dv=2.0 * ev / n, qn=qn, pol=alpha * logp - qn)
    out["sums"] = np.array([(out["e1"] ** 2).sum(), 0.0 if q2 is None else (out["e2"] ** 2).sum(), (ev ** 2).sum(),
                            out["pol"].sum(), rew.sum()])
    # magnitudes the rounding bounds scale with
    out["mag_q"] = [np.abs(q) + np.abs(rew) + gamma * np.abs(tv) for q in (q1, q2) if q is not None]
    out["mag_v"] = np.abs(v) + np.abs(qn) + abs(alpha) * np.abs(logp)
    out["sum_abs_rew"] = float(np.abs(rew).sum())
    return out


def moments_ref(head, logp, n_a):
    """(3, 4): {mean, unbiased std, max, min} of the clamped log_std, of log_prob and of the mean."""
    head, logp = np.asarray(head, dtype=np.float64), np.asarray(logp, dtype=np.float64).reshape(-1)
    rows = []
    for t in (np.clip(head[:, n_a:], -20.0, 2.0), logp, head[:, :n_a]):
        rows.append([t.mean(), t.std(ddof=1) if t.size > 1 else np.nan, t.max(), t.min()])
    return np.array(rows)


class Adam:
    def __init__(self, params, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        self.lr, self.b1, self.b2, self.eps, self.t = lr, beta1, beta2, eps, 0
        self.m = [np.zeros_like(p) for p in params]
        self.v = [np.zeros_like(p) for p in params]

    def step(self, params, grads):
        """In place on `params` (a flat list of arrays)."""
        self.t += 1
        bc1, bc2 = 1.0 - self.b1 ** self.t, 1.0 - self.b2 ** self.t
        for p, g, m, v in zip(params, grads, self.m, self.v):
            m *= self.b1; m += (1.0 - self.b1) * g
            v *= self.b2; v += (1.0 - self.b2) * g * g
            p -= (self.lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + self.eps))


def alpha_step_ref(log_alpha, opt, logp, target_entropy):
    """(alpha after the step, alpha_loss at the old log_alpha); log_alpha is a 1-element array stepped in place."""
    term = np.mean(logp + target_entropy)
    loss = -log_alpha[0] * term
    opt.step([log_alpha], [np.array([-term])])
    return float(np.exp(log_alpha[0])), float(loss)


# ------------------------------------------------------------------ dense nets by hand (ReLU trunk, linear head)
def mlp_forward(layers, x):
    tape, h = [x], x
    for k, (w, b) in enumerate(layers):
        h = h @ w.T + b
        if k < len(layers) - 1:
            h = np.maximum(h, 0.0)
        tape.append(h)
    return h, tape


def mlp_backward(layers, tape, d_out):
    """([dW, db, dW, db, ...] in layer order, d(input))."""
    grads, d = [], d_out
    for k in range(len(layers) - 1, -1, -1):
        if k < len(layers) - 1:
            d = d * (tape[k + 1] > 0.0)
        grads = [d.T @ tape[k], d.sum(0)] + grads
        d = d @ layers[k][0]
    return grads, d


def flat(layers):
    return [t for wb in layers for t in wb]


def clip_(grads, max_norm):
    norm = float(np.sqrt(sum((g * g).sum() for g in grads)))
    if max_norm:
        coef = min(max_norm / (norm + 1e-6), 1.0)
        grads = [g * coef for g in grads]
    return grads, norm


class Update:
    """One SAC (qfs: one critic) or TwinSAC (two) agent; `update(batch, eps)` returns the info dict."""

    def __init__(self, pf, vf, qfs, names, plr=3e-4, vlr=1e-3, qlr=1e-3, discount=0.99, tau=0.005, w_reg=0.0,
                 grad_clip=None, tune=True, target_entropy=-float(A)):
        self.pf, self.vf, self.qfs, self.names = pf, vf, list(qfs), list(names)      # names: of the critics
        self.tvf = [(w.copy(), b.copy()) for w, b in vf]
        self.opts = [Adam(flat(pf), plr)] + [Adam(flat(q), qlr) for q in self.qfs] + [Adam(flat(vf), vlr)]
        self.log_alpha, self.a_opt = np.zeros(1), Adam([np.zeros(1)], plr)
        self.discount, self.tau, self.w_reg, self.grad_clip = discount, tau, w_reg, grad_clip
        self.tune, self.target_entropy = tune, target_entropy

    def update(self, batch, eps):
        f = lambda t: np.asarray(t, dtype=np.float64)
        obs, nobs, acts, rew, term = (f(batch[k]) for k in BATCH_KEYS)
        eps = f(eps)
        n = obs.shape[0]
        head, tape_pf = mlp_forward(self.pf, obs)
        new_a, logp, x_sa, x_new = samples_ref(head, eps, obs, acts)
        mean, raw = head[:, :A], head[:, A:]
        ls = np.clip(raw, -20.0, 2.0)
        alpha, alpha_loss = 1.0, 0.0
        if self.tune:
            alpha, alpha_loss = alpha_step_ref(self.log_alpha, self.a_opt, logp, self.target_entropy)
        v, tape_v = mlp_forward(self.vf, obs)
        tv, _ = mlp_forward(self.tvf, nobs)
        qp = [mlp_forward(q, x_sa) for q in self.qfs]
        qn = [mlp_forward(q, x_new) for q in self.qfs]
        twin = len(self.qfs) == 2
        lo = losses_ref(qp[0][0], qp[1][0] if twin else None, tv, rew, term, v, qn[0][0], qn[1][0] if twin else None,
                        logp, alpha, self.discount, n)
        col = lambda t: t.reshape(-1, 1)
        # ---- gradients (everything before the first optimiser step) ----
        g_q = [mlp_backward(q, qp[i][1], col(lo["dq1" if i == 0 else "dq2"]))[0] for i, q in enumerate(self.qfs)]
        g_v = mlp_backward(self.vf, tape_v, col(lo["dv"]))[0]
        d_act = sum(mlp_backward(q, qn[i][1], col(lo["dq1n" if i == 0 else "dq2n"]))[1][:, D:]
                    for i, q in enumerate(self.qfs))
        one_a2 = 1.0 - new_a * new_a
        t = 2.0 * new_a * one_a2 / (one_a2 + 1e-6)
        se = np.exp(ls) * eps
        g_z = d_act * one_a2 + (alpha / n) * t
        reg = 2.0 / (n * A)
        inside = (raw >= -20.0) & (raw <= 2.0)
        d_head = np.concatenate([g_z + self.w_reg * reg * mean,
                                 inside * (g_z * se - alpha / n + self.w_reg * reg * ls)], 1)
        g_p = mlp_backward(self.pf, tape_pf, d_head)[0]
        # ---- steps pf -> qf(1, 2) -> vf, then the target ----
        norms = []
        for layers, grads, opt in zip([self.pf] + self.qfs + [self.vf], [g_p] + g_q + [g_v], self.opts):
            grads, norm = clip_(grads, self.grad_clip)
            norms.append(norm)
            opt.step(flat(layers), grads)
        for (w, b), (tw, tb) in zip(self.vf, self.tvf):
            tw *= 1.0 - self.tau; tw += self.tau * w
            tb *= 1.0 - self.tau; tb += self.tau * b
        # ---- what is logged ----
        info = {"Reward_Mean": rew.mean()}
        if self.tune:
            info["Alpha"], info["Alpha_loss"] = alpha, alpha_loss
        info["Training/policy_loss"] = lo["sums"][3] / n + self.w_reg * ((ls ** 2).mean() + (mean ** 2).mean())
        info["Training/vf_loss"] = lo["sums"][2] / n
        for i, name in enumerate(self.names):
            info["Training/%s_loss" % name] = lo["sums"][i] / n
        if self.grad_clip is not None:
            for name, norm in zip(["pf"] + self.names + ["vf"], norms):
                info["Training/%s_grad_norm" % name] = norm
        mom = moments_ref(head, logp, A)
        for k, key in enumerate(("log_std", "log_probs", "mean")):
            info[key + "/mean"], info[key + "/std"], info[key + "/max"], info[key + "/min"] = mom[k]
        return {k: float(x) for k, x in info.items()}


def update_from_fixture(g, tag):
    """An `Update` at the stored initial state of case `tag`, and that case's arguments."""
    H, B, w_reg, clip, tune, steps = g[tag + "_args"]
    names = net_names(g, tag)
    nets = {name: layers_of(g, "%s_%s0_" % (tag, name)) for name in names}
    up = Update(nets["pf"], nets["vf"], [nets[q] for q in names[1:-1]], names[1:-1], w_reg=float(w_reg),
                grad_clip=float(clip) if clip > 0 else None, tune=bool(tune))
    return up, int(B), int(steps)
