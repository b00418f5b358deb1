"""Plain torch restatement (CPU) of the categorical kernels' arithmetic (torchrl_amd/csrc/k_categorical.hip) and of
the updates built on them -- test infrastructure, imported by tests/test_categorical_*.py only.

Fixed arithmetic, as the kernels' header states it:  m = max_k l_k, e_k = exp(l_k - m), S = sum_k e_k and the prefix
sums in ascending k in fp32 (torch.cumsum on the CPU is a sequential scan per row), p_k = e_k / S,
log p_k = (l_k - m) - log S.  The uniform of (seed, counter, global env index g) is element g & 3 of Philox block
g >> 2 under the CATEGORICAL tag, mapped by (x >> 8) * 2^-24 + 2^-25 (oracle/philox.py conventions)."""
import numpy as np
import torch

from oracle import philox

TAG_CATEGORICAL = 0x43415447
LOSS_PPO_CLIP, LOSS_A2C = 0, 1


def philox_uniform(seed, counter, g):
    """float32 uniforms for (broadcast) int64 counter / global env index arrays."""
    counter, g = np.broadcast_arrays(np.asarray(counter, dtype=np.int64), np.asarray(g, dtype=np.int64))
    ctr = np.stack([counter & 0xFFFFFFFF, (counter >> 32) & 0xFFFFFFFF, (g >> 2) & 0xFFFFFFFF,
                    np.full_like(g, TAG_CATEGORICAL)], axis=-1).astype(np.uint32)
    seed = np.full_like(g, seed)
    key = np.stack([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], axis=-1).astype(np.uint32)
    x = philox.philox4x32_10(ctr, key)
    return philox.u32_to_unit(np.take_along_axis(x, (g & 3)[..., None], axis=-1)[..., 0])


def uniforms(seed, counter0, T, N, env_offset=0):
    """(T, N): what trl_philox_uniform_f32 writes."""
    t = np.arange(T, dtype=np.int64)[:, None] + np.int64(counter0)
    return philox_uniform(seed, t, np.arange(N, dtype=np.int64)[None, :] + np.int64(env_offset))


def act_case(A, N=4096):
    """The seeded logits / draw parameters of the action tests: (logits (N, A) float32, seed, counter)."""
    rs = np.random.RandomState(1000 + A)
    return torch.from_numpy((rs.randn(N, A) * 1.5).astype(np.float32)), 0xC011, 12345 + A


def softmax_terms(logits):
    """(m (B,1), e (B,A), prefix sums (B,A), S (B,1)) in the dtype of `logits`."""
    m = logits.max(dim=-1, keepdim=True)[0]
    e = torch.exp(logits - m)
    pre = torch.cumsum(e, dim=-1)
    return m, e, pre, pre[:, -1:]


def cat_act(logits, u=None, deterministic=False):
    """-> (action (N,) int64, log pi (N,), prefix sums (N, A), S (N,)).  Smallest k whose prefix sum is >= u * S, else
    A - 1; deterministic: arg-max, lowest index on ties."""
    logits = torch.as_tensor(logits)
    m, e, pre, S = softmax_terms(logits)
    A = logits.shape[1]
    if deterministic:
        a = (logits == m).to(torch.int64).argmax(dim=-1)                    # first maximum
    else:
        thr = torch.as_tensor(u, dtype=logits.dtype).reshape(-1, 1) * S
        hit = pre >= thr
        a = torch.where(hit.any(dim=-1), hit.to(torch.int64).argmax(dim=-1), torch.full((logits.shape[0],), A - 1))
    lp = (logits.gather(1, a[:, None]) - m) - torch.log(S)
    return a, lp[:, 0], pre, S[:, 0]


def borderline(u, pre, S, tol=1e-5):
    """Rows whose threshold u * S lies within tol * S of one of the prefix sums: a last-ulp difference of exp may move
    their action by one."""
    thr = (torch.as_tensor(u, dtype=pre.dtype) * S)[:, None]
    return ((pre - thr).abs() <= tol * S[:, None]).any(dim=-1)


def log_probs(logits):
    """-> (log p (B, A), p (B, A), entropy (B,))."""
    m, e, pre, S = softmax_terms(logits)
    logp_all = (logits - m) - torch.log(S)
    p = e / S
    return logp_all, p, -torch.cumsum(p * logp_all, dim=-1)[:, -1]


def cat_logp(logits, acts):
    """-> (log pi(a) (B,), entropy (B,), probabilities (B, A))."""
    logp_all, p, H = log_probs(logits)
    a = torch.as_tensor(acts).reshape(-1).to(torch.int64)
    return logp_all.gather(1, a[:, None])[:, 0], H, p


def adv_normalize(advs):
    """ppo.py:141-147 with the kernels' constants: mean / unbiased std from float64 sums, applied in the dtype of advs."""
    a64 = advs.double().reshape(-1)
    n = a64.numel()
    mean = a64.sum() / n
    var = ((a64 * a64).sum() - a64.sum() ** 2 / n) / (n - 1)
    mu = mean.to(advs.dtype)
    rstd = 1.0 / (torch.sqrt(var.clamp(min=0.0)).to(advs.dtype) + 1e-5)
    return (advs.reshape(-1) - mu) * rstd


def losses(logits, v, acts, advs, rets, v_old, old_logp, clip_para, entropy_coeff, clipped_value_loss, loss_mode,
           n_global=None):
    """The loss half of one minibatch, the kernel's formulas: -> dict(d_logits, d_v, lp, ent, ratio, surr, vloss, advn).
    `surr` = -min(s1, s2) per sample (A2C: -log pi * adv), `vloss` the per-sample value-loss terms."""
    B, A = logits.shape
    n = float(B if n_global is None else n_global)
    inv_b = 1.0 / n
    a = torch.as_tensor(acts).reshape(-1).to(torch.int64)
    logp_all, p, H = log_probs(logits)
    lp = logp_all.gather(1, a[:, None])[:, 0]
    advn = adv_normalize(advs)
    if loss_mode == LOSS_A2C:
        ratio = torch.ones_like(lp)
        s1 = s2 = lp * advn
        g_lp = -advn * inv_b
    else:
        ratio = torch.exp(lp - old_logp.reshape(-1))
        s1 = ratio * advn
        s2 = ratio.clamp(1.0 - clip_para, 1.0 + clip_para) * advn
        g_lp = torch.where(s1 <= s2, -advn * ratio * inv_b, torch.zeros_like(lp))
    onehot = torch.zeros_like(logits).scatter_(1, a[:, None], 1.0)
    d_logits = g_lp[:, None] * (onehot - p) + (entropy_coeff * inv_b) * p * (logp_all + H[:, None])
    vv, R = v.reshape(-1), rets.reshape(-1)
    if clipped_value_loss:
        vo = v_old.reshape(-1)
        dc = vv - vo
        vc = vo + dc.clamp(-clip_para, clip_para)
        l1, l2 = (vv - R) ** 2, (vc - R) ** 2
        wa = torch.where(l1 > l2, torch.ones_like(l1), torch.where(l1 == l2, torch.full_like(l1, 0.5), torch.zeros_like(l1)))
        passed = ((dc >= -clip_para) & (dc <= clip_para)).to(vv.dtype)
        vloss = 0.5 * torch.maximum(l1, l2)
        d_v = inv_b * (wa * (vv - R) + (1.0 - wa) * passed * (vc - R))
    else:
        vloss = (vv - R) ** 2
        d_v = 2.0 * (vv - R) * inv_b
    return dict(d_logits=d_logits, d_v=d_v, lp=lp, ent=H, ratio=ratio, surr=-torch.minimum(s1, s2), vloss=vloss, advn=advn)


def objective(logits, v, acts, advs, rets, v_old, old_logp, clip_para, entropy_coeff, clipped_value_loss, loss_mode):
    """policy loss + value loss as ONE differentiable scalar (the two do not share inputs): autograd on it gives what
    `losses` states in closed form.  Any dtype; the advantage is normalised outside the graph."""
    a = torch.as_tensor(acts).reshape(-1).to(torch.int64)
    lp, H, _ = cat_logp(logits, a)
    advn = adv_normalize(advs).detach()
    if loss_mode == LOSS_A2C:
        pl = -(lp * advn).mean()
    else:
        ratio = torch.exp(lp - old_logp.reshape(-1))
        pl = -torch.minimum(ratio * advn, ratio.clamp(1.0 - clip_para, 1.0 + clip_para) * advn).mean()
    pl = pl - entropy_coeff * H.mean()
    vv, R = v.reshape(-1), rets.reshape(-1)
    if clipped_value_loss:
        vc = v_old.reshape(-1) + (vv - v_old.reshape(-1)).clamp(-clip_para, clip_para)
        vl = 0.5 * torch.maximum((vv - R) ** 2, (vc - R) ** 2).mean()
    else:
        vl = ((vv - R) ** 2).mean()
    return pl + vl


class MLP:
    """Tanh / ReLU MLP on explicit parameter lists [W1, b1, W2, b2, ...] (nn.Linear layout)."""

    def __init__(self, params, act=torch.tanh):
        self.params = [torch.as_tensor(p).clone().float().requires_grad_(True) for p in params]
        self.act = act

    def __call__(self, x):
        h = x
        n = len(self.params) // 2
        for k in range(n):
            h = h @ self.params[2 * k].t() + self.params[2 * k + 1]
            if k < n - 1:
                h = self.act(h)
        return h

    def copy_from(self, other):
        with torch.no_grad():
            for a, b in zip(self.params, other.params):
                a.copy_(b)


def params_from(g, prefix):
    """The [W1, b1, ..., W_head, b_head] list of a fixture state dict (base.seq_fcs.*, then seq_append_fcs.*)."""
    index = lambda k: int([x for x in k.split("__") if x.isdigit()][0])
    names = sorted((k[len(prefix):] for k in g.files if k.startswith(prefix)),
                   key=lambda k: (not k.startswith("base"), index(k), k.endswith("bias")))
    return [torch.from_numpy(g[prefix + k].copy()) for k in names]


class CatUpdate:
    """A2C.update / PPO.update with a categorical policy (a2c.py:45-106, ppo.py:41-152): the loss half by `losses`, the
    layers by torch, clip_grad_norm_(0.5) + Adam(eps=1e-5) per network."""

    def __init__(self, pf_params, vf_params, plr, vlr, entropy_coeff, clip_para=0.2, target_params=None, act=torch.tanh):
        self.pf, self.vf = MLP(pf_params, act), MLP(vf_params, act)
        self.target = MLP(pf_params if target_params is None else target_params, act)
        self.opt_pf = torch.optim.Adam(self.pf.params, lr=plr, eps=1e-5)
        self.opt_vf = torch.optim.Adam(self.vf.params, lr=vlr, eps=1e-5)
        self.entropy_coeff, self.clip_para = entropy_coeff, clip_para

    def update(self, batch, loss_mode, clipped_value_loss=False, old_logp=None):
        t = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32) for k, v in batch.items()}
        obs, acts, advs, rets = t["obs"], t["acts"].reshape(-1), t["advs"].reshape(-1), t["estimate_returns"].reshape(-1)
        n = advs.numel()
        if loss_mode == LOSS_PPO_CLIP and old_logp is None:
            with torch.no_grad():
                old_logp = cat_logp(self.target(obs), acts)[0]
        logits, v = self.pf(obs), self.vf(obs)
        with torch.no_grad():
            r = losses(logits.detach(), v.detach(), acts, advs, rets, t.get("values"), old_logp, self.clip_para,
                       self.entropy_coeff, clipped_value_loss, loss_mode)
        norms = []
        for out, d, opt, params in ((logits, r["d_logits"], self.opt_pf, self.pf.params),
                                    (v, r["d_v"].reshape(v.shape), self.opt_vf, self.vf.params)):
            opt.zero_grad()
            out.backward(d)
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, 0.5)))
            opt.step()
        ent, lp, vv = r["ent"].double().mean().item(), r["lp"].double(), v.detach().double().reshape(-1)
        pl = r["surr"].double().mean().item() - self.entropy_coeff * ent
        if loss_mode == LOSS_A2C:
            return {'Training/policy_loss': pl, 'Training/vf_loss': r["vloss"].double().mean().item(),
                    'v_pred/mean': vv.mean().item(), 'v_pred/std': vv.std().item(), 'v_pred/max': vv.max().item(),
                    'v_pred/min': vv.min().item(), 'ent': ent, 'log_prob': lp.mean().item()}
        a64 = advs.double()
        return {'advs/mean': a64.mean().item(), 'advs/std': a64.std().item(), 'advs/max': a64.max().item(),
                'advs/min': a64.min().item(), 'Training/vf_loss': r["vloss"].double().mean().item(),
                'grad_norm/vf': norms[1], 'Training/policy_loss': pl, 'logprob/mean': lp.mean().item(),
                'logprob/std': lp.std().item(), 'logprob/max': lp.max().item(), 'logprob/min': lp.min().item(),
                'ratio/max': r["ratio"].max().item(), 'ratio/min': r["ratio"].min().item(), 'grad_norm/pf': norms[0]}


def train_host_env_cpu(params, env_id, n_envs, seed, pf_params, vf_params, epochs=None):
    """PPO with a categorical policy on a host env, everything on the CPU: the collector's step (on_policy.py:90-155,
    the restatement's action draw keyed by the global step), the ring and GAE of oracle/replay.py, the linear learning-rate
    schedule, `opt_epochs` permutation passes of `CatUpdate` minibatches.  Returns the mean training-episode return of
    every epoch (NaN for an epoch in which no episode ended).  `params`: a config dict as the examples read it."""
    from oracle.replay import RingOracle
    from torchrl_amd.env import get_vec_env
    gs, pp, cp = params["general_setting"], params["ppo"], params["collector"]
    env = get_vec_env(env_id, params["env"], n_envs)
    env.seed(seed)
    np.random.seed(seed)
    T = cp["epoch_frames"] // n_envs
    ring = RingOracle(params["replay_buffer"]["size"], env_nums=n_envs, time_limit_filter=params["replay_buffer"]["time_limit_filter"])
    o = CatUpdate(pf_params, vf_params, plr=pp["plr"], vlr=pp["vlr"], entropy_coeff=pp["entropy_coeff"], clip_para=pp["clip_para"])
    ob = env.reset()
    cur_step, run_ret = np.zeros((n_envs, 1)), np.zeros((n_envs, 1))
    global_step, noise_seed, out = 0, 0xC011, []
    for epoch in range(gs["num_epochs"] if epochs is None else epochs):
        finished = []
        with torch.no_grad():
            for _ in range(T):
                obs_t = torch.as_tensor(np.asarray(ob), dtype=torch.float32)
                a, lp, _, _ = cat_act(o.pf(obs_t), uniforms(noise_seed, global_step, 1, n_envs)[0])
                values = o.vf(obs_t).numpy()
                stored_ob = np.array(ob, dtype=np.float32)
                nxt, rew, done, infos = env.step(a.numpy())
                global_step += 1
                cur_step += 1
                run_ret += rew
                tl = infos["time_limit"][:, None] if "time_limit" in infos else np.zeros_like(done)
                if done.any():
                    finished += list(run_ret[done])
                    run_ret[done] = 0
                surpass = cur_step >= cp["max_episode_frames"]
                terminals = done
                if done.any() or surpass.any():
                    last_v = o.vf(torch.as_tensor(np.asarray(nxt), dtype=torch.float32)).numpy()
                    terminals = done | surpass
                    rew = rew + gs["discount"] * last_v * surpass
                    nxt = env.partial_reset(terminals[:, 0])
                    cur_step[terminals] = 0
                ring.add({"obs": stored_ob, "next_obs": np.array(nxt, dtype=np.float32), "acts": a.numpy()[:, None].astype(np.float32),
                          "values": values, "rewards": rew, "terminals": terminals, "time_limits": tl,
                          "old_logp": lp.numpy()[:, None]})
                ob = nxt
            last = ring.last_row(["next_obs"])["next_obs"]
            ring.gae(o.vf(torch.as_tensor(last, dtype=torch.float32)).numpy(), gs["discount"], pp["tau"])
        out.append(float(np.mean(finished)) if finished else float("nan"))
        frac = 1.0 - epoch / float(gs["num_epochs"])                         # algo/utils.py: linear schedule
        for opt, lr in ((o.opt_pf, pp["plr"]), (o.opt_vf, pp["vlr"])):
            for grp in opt.param_groups:
                grp["lr"] = lr * frac
        keys = ["obs", "acts", "advs", "estimate_returns", "values", "old_logp"]
        for _ in range(pp["opt_epochs"]):
            for _idx, mb in ring.epoch_minibatches(gs["batch_size"], keys, pp["shuffle"]):
                o.update({k: mb[k] for k in keys[:5]}, LOSS_PPO_CLIP, old_logp=torch.as_tensor(mb["old_logp"], dtype=torch.float32))
    return out
