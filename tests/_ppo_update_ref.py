"""Plain restatements (CPU; torch float64 / float32, numpy for the optimiser) of what torchrl_amd/csrc/k_ppo.hip computes for
a shared-std Gaussian policy: one minibatch's gradients of both 3-layer networks (ppo_grad_wave_kernel<..., HEAD_GAUSS>;
reference ppo.py:41-152, a2c.py:29-106, continuous_policy.py, distribution.py), the fold of the workgroup rows
(ppo_reduce_kernel), clip_grad_norm_ + Adam (clip_adam_kernel, include/trl_hip.h "K11") and the Polyak step with its
ring filing (polyak_tick_kernel) -- test infrastructure, imported by tests/test_ppo_update_kernels_{cpu,gpu}.py only.

The loss half is tests/_gauss_ref.py::losses (log pi, entropy, surrogate, value loss with its tie convention, the
log-std gate); this module pushes its per-sample cotangents back through the layers and adds, per gradient element, the
running magnitude M the element bound is relative to:

    dW_k = dZ_k^T X_k    M_W = |dZ_k|^T (|X_k| + F_k)   db_k = sum_s dZ_k    M_b = sum_s |dZ_k|
    d_logstd = sum_s dls_terms                          M_logstd = sum_s |dls_terms|

(X_k: the layer's input, dZ_k: the cotangent of its pre-activation; always float64, from the run's own values.  F_k = |X_{k-1}|
|W_{k-1}|^T + |b_{k-1}| is the running magnitude of the pre-activation X_k is the activation of, F_1 = 0: a hidden unit near zero
is the difference of 64 products, and its error is relative to those, not to itself -- with |X_k| alone a minibatch of two
samples needs K = 16 384 where the others need 128, see profiles/NOTES_ppo_update_kernel_tests.md.)"""
import numpy as np
import torch

import _gauss_ref as gr
from _categorical_update_cases import act_fn

U = gr.U
SENTINEL = gr.SENTINEL
BLOCKS = ("W1", "b1", "W2", "b2", "W3", "b3", "logstd")
GRAD_FLOOR = 1e-6                     # absolute error of one sample's cotangent, times n_global (see `grad_floor`)


# ------------------------------------------------------------------ layers
def layers(params, x, act):
    """-> (output, [X_1, X_2, X_3] layer inputs, [Z_1, Z_2, Z_3] pre-activations) of [W1 b1 W2 b2 W3 b3]."""
    xs, zs, h = [], [], x
    for k in range(3):
        xs.append(h)
        z = h @ params[2 * k].t() + params[2 * k + 1]
        zs.append(z)
        h = act_fn(act)(z) if k < 2 else z
    return h, xs, zs


def block_slices(D, A, policy):
    """name -> slice of the flat block [W1 b1 W2 b2 W3 b3 (logstd)] (MlpFlat, trl_mlp.h), H = 64."""
    O = A if policy else 1
    sizes = [64 * D, 64, 4096, 64, 64 * O, O] + ([A] if policy else [])
    out, off = {}, 0
    for name, n in zip(BLOCKS, sizes):
        out[name] = slice(off, off + n)
        off += n
    return out


def _backward(out, cot, params, xs, zs):
    """Flat gradient of sum(out * cot) w.r.t. [W1 b1 W2 b2 W3 b3] by autograd, and its running magnitude (float64)."""
    g = torch.autograd.grad(out, list(params) + list(zs), grad_outputs=cot)
    gp, dz = g[:6], g[6:]
    M, mz = [], None
    for k in range(3):
        a, x = dz[k].detach().double().abs(), xs[k].detach().double().abs()
        # (X_k = act(Z_{k-1}) is itself computed: its error is relative to the running magnitude of Z_{k-1}, not to |X_k| --
        # a hidden unit near zero is the difference of 64 products)
        M += [(a.t() @ (x if mz is None else x + mz)).reshape(-1), a.sum(0)]
        mz = x @ params[2 * k].detach().double().abs().t() + params[2 * k + 1].detach().double().abs()
    return torch.cat([t.reshape(-1) for t in gp]).detach(), torch.cat(M)


def minibatch_grads(pf, logstd, vf, mb, adv_raw, n_global, loss_mode, clipv, tanh, act, dtype, clip, c_ent):
    """One minibatch in `dtype`.  pf / vf: [W1 b1 W2 b2 W3 b3]; mb: dict(obs, acts, advs, rets, old_values, old_logp) of
    the B local samples in the kernel's order.  -> dict(pf, vf: flat gradients [.. | d_logstd] / [..], M_pf, M_vf: their
    running magnitudes (float64), info: the 24-slot row of _gauss_ref.losses, z: every hidden pre-activation, loss: the
    loss half's dict)."""
    t = lambda x: x.to(dtype)
    pfp = [t(p).clone().requires_grad_(True) for p in pf]
    vfp = [t(p).clone().requires_grad_(True) for p in vf]
    obs = t(mb["obs"])
    mean, pxs, pzs = layers(pfp, obs, act)
    v, vxs, vzs = layers(vfp, obs, act)
    old = t(mb["old_logp"]).reshape(-1) if loss_mode == gr.LOSS_PPO_CLIP else None
    v_old = t(mb["old_values"]).reshape(-1) if clipv else None
    L = gr.losses(mean.detach(), v.detach().reshape(-1), t(logstd), t(mb["acts"]), t(mb["advs"]).reshape(-1),
                  t(mb["rets"]).reshape(-1), v_old, old, adv_raw, n_global, clip, c_ent, clipv, loss_mode, tanh)
    g_pf, M_pf = _backward(mean, L["d_mean"].to(dtype), pfp, pxs, pzs)
    g_vf, M_vf = _backward(v, L["d_v"].to(dtype).reshape(-1, 1), vfp, vxs, vzs)
    z = torch.cat([x.detach().reshape(-1) for x in pzs[:2] + vzs[:2]])
    return dict(pf=torch.cat([g_pf, L["d_logstd"].detach().reshape(-1)]), vf=g_vf,
                M_pf=torch.cat([M_pf, L["dls_terms"].abs().sum(0)]), M_vf=M_vf, info=L["info"], z=z, loss=L)


def grad_floor(mb, pf, vf, act, n_global):
    """The absolute part of the element bound: GRAD_FLOOR / n_global per sample in the place of |dZ_k|.  The loss half's
    cotangents are differences of computed values (v - R, atanh(a) - mean), so their error is absolute: the project's floor
    on one sample's d_v is 1e-6 / n_global and on d_mean 1e-4 / n_global (_gauss_ref.loss_error_ratios); both networks take
    the tighter one here.  -> (floor_pf incl. the logstd tail, floor_vf), float64."""
    out = []
    for params in (pf, vf):
        _, xs, _ = layers([p.double() for p in params], mb["obs"].double(), act)
        f = []
        for k in range(3):
            o = params[2 * k].shape[0]
            f += [xs[k].abs().sum(0).reshape(1, -1).expand(o, -1).reshape(-1), torch.full((o,), float(xs[k].shape[0]),
                                                                                        dtype=torch.float64)]
        out.append(torch.cat(f))
    B, A = mb["obs"].shape[0], pf[4].shape[0]
    out[0] = torch.cat([out[0], torch.full((A,), float(B), dtype=torch.float64)])
    return out[0] * (GRAD_FLOOR / n_global), out[1] * (GRAD_FLOOR / n_global)


def grad_bound(M, floor, K_w, K_ls=None, A=0):
    """|got_e - want_e| <= K u M_e + floor_e; K_ls on the A trailing d_logstd elements."""
    K = torch.full_like(M, float(K_w))
    if A:
        K[-A:] = float(K_ls)
    return K * U * M + floor


def k_needed(got, want, M, floor, margin=4.0):
    """The smallest K with margin * |got - want| <= K u M + floor on every element (inf: an element with M = 0 beyond its
    floor)."""
    need = margin * (got.double() - want.double()).abs() - floor
    if bool((need[M == 0] > 0).any()):
        return float("inf")
    pos = M > 0
    return max(0.0, float((need[pos] / (U * M[pos])).max())) if bool(pos.any()) else 0.0


def pow2_at_least(x):
    return 2.0 ** int(np.ceil(np.log2(x))) if x > 1.0 else 1.0


def grad_error_ratios(got_pf, got_vf, want, floors, K_w, K_ls, D, A):
    """Worst err / bound of the two flat gradients against the float64 dict of `minibatch_grads`: "elem" the element bound
    over both networks' weights and biases, "elem_ls" the same on d_logstd, "blocks" {"pf_W1": err / (1e-4 max|want|), ..}
    the project's contract per block (a block that is zero in float64 must be zero: inf otherwise)."""
    out = {"blocks": {}}
    worst, worst_ls = 0.0, 0.0
    for net, got, w, M, fl in (("pf", got_pf, want["pf"], want["M_pf"], floors[0]), ("vf", got_vf, want["vf"], want["M_vf"], floors[1])):
        err = (got.double() - w.double()).abs()
        bound = grad_bound(M, fl, K_w, K_ls, A if net == "pf" else 0)
        r = err / bound
        if net == "pf":
            worst, worst_ls = max(worst, float(r[:-A].max())), float(r[-A:].max())
        else:
            worst = max(worst, float(r.max()))
        for name, sl in block_slices(D, A, net == "pf").items():
            top = float(w[sl].double().abs().max())
            e = float(err[sl].max())
            out["blocks"][net + "_" + name] = (e / (1e-4 * top)) if top > 0 else (0.0 if e == 0.0 else float("inf"))
    out["elem"], out["elem_ls"] = worst, worst_ls
    return out


# ------------------------------------------------------------------ fold
def fold_kernel_order(rows):
    """The fold in float32 IN THE KERNEL'S ORDER (fold_rows_wave / fold_chain_tree / fold_waves_tree), on the CPU."""
    r = np.asarray(rows, dtype=np.float32)
    n, P = r.shape
    acc = np.zeros((8, 16, P), dtype=np.float32)
    for i in range(n):
        w, k = i % 8, (i // 8) % 16
        acc[w, k] = acc[w, k] + r[i]
    st = 8
    while st > 0:
        acc[:, :st] = acc[:, :st] + acc[:, st:2 * st]
        st //= 2
    a = acc[:, 0]
    return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))


def fold(rows):
    """(n, P) float rows -> (float64 sum, S = sum |row|)."""
    r = rows.double()
    return r.sum(0), r.abs().sum(0)


def fold_bound(n_rows, S):
    """The fold's association order (k_ppo.hip, "pieces of the fold"): a row is dealt to wave r % 8 and chain (r / 8) % 16; a
    chain adds one row per round of 128 (ceil(rows / 128) additions, the first to a zero), 16 chains fold pairwise (4
    additions), 8 waves pairwise (3): every term passes ceil(rows / 128) + 7 roundings at the most."""
    return (-(-n_rows // 128) + 7) * U * S


# ------------------------------------------------------------------ clip_grad_norm_ + Adam, Polyak
def f32v(x):
    """The float64 value of the float32 a launch descriptor carries."""
    return float(np.float32(x))


class AdamRef:
    """trl_clip_adam_f32 (trl_hip.h "K11") on numpy arrays in `dtype`: grads * grad_scale, the clip coefficient
    min(max_norm / (norm + 1e-6), 1) per group (max_norm <= 0: 1), Adam with eps OUTSIDE the root and the bias corrections
    1 - beta1^t, sqrt(1 - beta2^t) formed in float64 from the step count or from the state {steps, beta1^steps,
    beta2^steps}.  Hyper-parameters are the float32 values of the descriptor.  dtype float32: the kernel's operation
    order (only the order of the norm's additions differs)."""

    def __init__(self, params, m, v, sizes, beta1=0.9, beta2=0.999, eps=1e-5, dtype=np.float64):
        self.dtype = dtype
        self.p, self.m, self.v = (np.array(x, dtype=dtype) for x in (params, m, v))
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.b1, self.b2, self.eps = f32v(beta1), f32v(beta2), f32v(eps)
        self.state = np.array([0.0, 1.0, 1.0])                          # the device-resident {steps, beta1^steps, beta2^steps}

    def step(self, grads, lrs, max_norm, grad_scale=1.0, step_count=None):
        """One update; step_count None: from the state (which is advanced).  -> dict(norms, update: the running magnitude
        (lr / bc1) (|beta1 m| + |(1 - beta1) g|) / denom of the step, g: the scaled and clipped gradient, m_mag / v_mag: |beta m| + |(1 - beta) g^(2)|, float64, p_mag: |param| before and after)."""
        dt = self.dtype
        c = lambda x: dt(f32v(x))
        g = np.array(grads, dtype=dt)
        gs, mn = c(grad_scale), c(max_norm)
        if step_count is None:
            bc1, bc2 = 1.0 - self.state[1] * self.b1, 1.0 - self.state[2] * self.b2
            self.state = np.array([self.state[0] + 1.0, self.state[1] * self.b1, self.state[2] * self.b2])
        else:
            bc1, bc2 = 1.0 - self.b1 ** float(step_count), 1.0 - self.b2 ** float(step_count)
        bc1, bc2s = dt(bc1), dt(np.sqrt(bc2))                            # (the kernel rounds them to float32 once, like this)
        norms, coef = np.zeros(len(self.off) - 1, dtype=dt), np.ones(g.shape, dtype=dt)
        for k in range(len(self.off) - 1):
            sl = slice(self.off[k], self.off[k + 1])
            norms[k] = np.sqrt((g[sl] * g[sl]).sum(dtype=dt) * gs * gs)
            if f32v(max_norm) > 0.0:
                coef[sl] = min(mn / (norms[k] + dt(1e-6)), dt(1.0))
        lr = np.zeros(g.shape, dtype=dt)
        for k in range(len(self.off) - 1):
            lr[self.off[k]:self.off[k + 1]] = c(lrs[k])
        b1, b2, one = dt(self.b1), dt(self.b2), dt(1.0)
        gr_ = g * gs * coef
        m_a, m_b = b1 * self.m, (one - b1) * gr_
        v_a, v_b = b2 * self.v, (one - b2) * gr_ * gr_
        p0 = self.p.copy()
        self.m, self.v = m_a + m_b, v_a + v_b
        denom = np.sqrt(self.v) / dt(bc2s) + dt(self.eps)
        update = (lr / dt(bc1)) * (self.m / denom)
        self.p = self.p - update
        f = lambda x: np.abs(np.asarray(x, dtype=np.float64))
        # (the update's running magnitude: m replaced by |beta m| + |(1 - beta) g| -- where the two terms of m cancel, the
        # update inherits m's absolute error, not a relative one)
        m_mag = f(m_a) + f(m_b)
        return dict(norms=norms, update=f(lr / dt(bc1)) * m_mag / f(denom), g=gr_, m_mag=m_mag, v_mag=f(v_a) + f(v_b),
                    p_mag=np.maximum(f(p0), f(self.p)))


class AdamBound:
    """Running error bounds of a chain of AdamRef steps, in units of the constants K:  m, v: E <- beta E + u (|beta m| + |(1
    - beta) g^(2)|);  params: E <- E + K_P u |update| + K_R u |param| (the update's own error, and the rounding of the
    subtraction -- |param| the larger of before and after)."""

    def __init__(self, n):
        self.m, self.v, self.pu, self.pr = (np.zeros(n) for _ in range(4))

    def add(self, r, opt):
        self.m = opt.b1 * self.m + U * r["m_mag"]
        self.v = opt.b2 * self.v + U * r["v_mag"]
        self.pu = self.pu + U * r["update"]
        self.pr = self.pr + U * r["p_mag"]

    def params(self, K_p, K_r):
        return K_p * self.pu + K_r * self.pr


def adam_chain(x, sizes, steps, dtype=np.float64):
    """AdamRef over `steps` = [(grads, lrs, max_norm, grad_scale, step_count or None)] from case x (p, m, v) -> (the
    optimiser, its AdamBound, the last step's dict)."""
    opt = AdamRef(x["p"], x["m"], x["v"], sizes, dtype=dtype)
    bound, r = AdamBound(len(x["p"])), None
    for grads, lrs, max_norm, gs, count in steps:
        r = opt.step(grads, lrs, max_norm, gs, count)
        bound.add(r, opt)
    return opt, bound, r


def adam_error_ratios(got_p, got_m, got_v, opt, bound, K_m, K_v, K_p, K_r):
    """Worst err / bound of params, m, v (float32 arrays) against the float64 optimiser `opt` of `adam_chain`; an element
    whose bound is zero must be equal."""
    out = {}
    for name, got, want, b in (("m", got_m, opt.m, K_m * bound.m), ("v", got_v, opt.v, K_v * bound.v),
                               ("p", got_p, opt.p, bound.params(K_p, K_r))):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        pos = b > 0
        worst = float((err[pos] / b[pos]).max()) if pos.any() else 0.0
        out[name] = float("inf") if (err[~pos] > 0).any() else worst
    return out


def adam_k_needed(got_p, got_m, got_v, opt, bound, K_r, margin=4.0):
    """The K each of m, v, params needs so that margin * err stays under the bound (params: beside K_r u |param|)."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    need = {}
    for name, got, want, b in (("m", got_m, opt.m, bound.m), ("v", got_v, opt.v, bound.v)):
        pos = b > 0
        need[name] = float((margin * np.abs(f(got) - want)[pos] / b[pos]).max()) if pos.any() else 0.0
    rest = margin * np.abs(f(got_p) - opt.p) - K_r * bound.pr
    pos = bound.pu > 0
    need["p"] = max(0.0, float((rest[pos] / bound.pu[pos]).max())) if pos.any() else 0.0
    return need


def polyak(target, source, tau, dtype=np.float64):
    """target <- (1 - tau) target + tau source, the kernel's order: t * (1 - tau) + s * tau."""
    t, s, tau = np.asarray(target, dtype=dtype), np.asarray(source, dtype=dtype), dtype(f32v(tau))
    return t * (dtype(1.0) - tau) + s * tau


def polyak_bound(target, source):
    """Two products and one sum of float32 terms bounded by |t| and |s|: 3 u (|t| + |s|)."""
    return 3.0 * U * (np.abs(np.asarray(target, dtype=np.float64)) + np.abs(np.asarray(source, dtype=np.float64)))


def ring_row(steps_before, slots):
    """The ring row an update's statistics block is filed in: optimiser steps taken BEFORE this update, mod slots."""
    return int(steps_before) % int(slots)


# ------------------------------------------------------------------ whole updates: gradients, fold, clip + Adam
def split_flat(flat, D, A, policy):
    """The flat block [W1 b1 W2 b2 W3 b3 (logstd)] as a list of tensors in nn.Linear layout."""
    O = A if policy else 1
    shapes = dict(W1=(64, D), b1=(64,), W2=(64, 64), b2=(64,), W3=(O, 64), b3=(O,), logstd=(A,))
    return [torch.from_numpy(np.array(flat[sl])).reshape(shapes[k]) for k, sl in block_slices(D, A, policy).items()]


def flat_params(pf, logstd, vf):
    return torch.cat([t.reshape(-1) for t in pf] + [logstd.reshape(-1)] + [t.reshape(-1) for t in vf]).numpy()


def grads_at(flat, x, mb, loss_mode, clipv, dtype, c_ent):
    """minibatch_grads of case x at the flat parameters [policy | value] (numpy)."""
    D, A = x["D"], x["A"]
    p_pf = 64 * D + 64 + 4096 + 64 + 64 * A + 2 * A
    pf, vf = split_flat(flat[:p_pf], D, A, True), split_flat(flat[p_pf:], D, A, False)
    return minibatch_grads(pf[:6], pf[6], vf, mb, x["adv_raw"], x["n_global"], loss_mode, clipv, x["tanh"], x["act"], dtype,
                           x["clip"], c_ent)


def update_chain(x, mb, mv, lrs, steps, loss_mode, clipv, c_ent, np_dtype=np.float64):
    """`steps` whole updates of case x from its own parameters and the moments mv (dict m, v): gradients of the restatement
    at the current parameters, then AdamRef's step on the device-resident state; everything in np_dtype.  -> AdamRef."""
    tdt = torch.float64 if np_dtype is np.float64 else torch.float32
    p0 = flat_params(x["pf"], x["logstd"], x["vf"])
    sizes = (p0.size - sum(t.numel() for t in x["vf"]), sum(t.numel() for t in x["vf"]))
    opt = AdamRef(p0, mv["m"], mv["v"], sizes, dtype=np_dtype)
    for _ in range(steps):
        w = grads_at(opt.p, x, mb, loss_mode, clipv, tdt, c_ent)
        opt.step(torch.cat([w["pf"], w["vf"]]).numpy(), lrs, 0.5, 1.0, None)
    return opt
