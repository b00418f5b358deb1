"""trl_clip_step_f32 (include/trl_hip.h: global-norm clip + RMSprop / SGD) restated in numpy, in a chosen dtype, with the
running magnitude of every stored quantity beside its float64 value -- the shape of AdamRef / AdamBound in
_ppo_update_ref.py.

A float32 run of the step differs from the float64 one by its own roundings and by what it inherits from the quantities of
earlier steps.  To first order, with u = 2^-24 and M_x the running magnitude of x (the error of x is a small multiple of
u M_x; every line: what is inherited, then the magnitude of the terms rounded here):

    g0  = grads * grad_scale * coef                       M_g   = 3 |g0|                     (scale, coef, coef's own norm)
    g   = g0 + weight_decay p  (weight_decay != 0)        M_g  += wd M_p + |g0| + 2 |wd p|   (the product, the sum)
  RMSprop
    sq  = alpha sq + (1 - alpha) g g                      M_sq  = alpha M_sq + 2 (1 - alpha) |g| M_g + |alpha sq| + |(1 - alpha) g g|
    ga  = ga + (g - ga)(1 - alpha)                        M_ga  = alpha M_ga + (1 - alpha) M_g + |ga| + (1 - alpha)(|g| + |ga|)
    arg = sq - ga ga  (centered; else sq)                 M_arg = M_sq + 2 |ga| M_ga + |sq| + ga^2    (it cancels: NOT |arg|)
    avg = sqrt(arg) + eps                                 M_avg = M_arg / (2 sqrt(arg)) + avg
    q   = g / avg                                         M_q   = M_g / avg + |q| M_avg / avg + |q|
    buf = momentum buf + q                                M_buf = momentum M_buf + M_q + |momentum buf| + |q|
    p   = p - lr (buf | q)                                M_p   = M_p + lr M_(buf | q) + |lr (buf | q)| + max |p|
  SGD
    buf = g (first step) | momentum buf + (1 - d) g       M_buf = M_g | momentum M_buf + (1 - d) M_g + |momentum buf| + |(1 - d) g|
    s   = g + momentum buf (nesterov) | buf | g           M_s   = M_g + momentum M_buf + |g| + |momentum buf| | M_buf | M_g
    p   = p - lr s                                        M_p   = M_p + lr M_s + |lr s| + max |p|

A device result is held against  K[kind][x] * u * M_x  per element.  The K below are NOT fitted to the device: they are the
largest err / (u M_x) a float32 numpy run of this restatement shows against the float64 run over every option set, clip mode
and chain of tests/test_optim_kernels_cpu.py, times the margin of 4 `adam_k_needed` uses (the device's sqrtf and division
may be 1-2 ulp where numpy's are correctly rounded, and fmaf contraction moves roundings), rounded up to a power of two.
test_optim_kernels_cpu.py recomputes them and fails when one no longer covers; profiles/NOTES_optimisers.md records them.
"""
import numpy as np

U = 2.0 ** -24
RMSPROP, SGD = 1, 2                                                    # TRL_OPT_* of include/trl_hip.h
STATE_NAMES = {RMSPROP: ("square_avg", "momentum_buffer", "grad_avg"), SGD: ("momentum_buffer",)}

# option sets of the CPU and GPU tests (keyword arguments of torch.optim.RMSprop / torch.optim.SGD)
RMSPROP_OPTIONS = [dict(), dict(momentum=0.9), dict(centered=True),
                   dict(alpha=0.95, eps=0.01, centered=True, momentum=0.95), dict(weight_decay=1e-2)]
SGD_OPTIONS = [dict(), dict(momentum=0.9), dict(momentum=0.9, dampening=0.1), dict(momentum=0.9, nesterov=True),
               dict(weight_decay=1e-2)]

# margin 4 x the largest CPU ratio, rounded up to a power of two (see the module docstring; measured values in the NOTES)
K = {RMSPROP: {"p": 4.0, "s0": 4.0, "s1": 2.0, "s2": 4.0}, SGD: {"p": 4.0, "s0": 4.0}}


def f32v(x):
    """The float64 value of the float32 a launch descriptor carries."""
    return float(np.float32(x))


class OptRef:
    """The step on numpy arrays in `dtype`.  `exact_hyper`: hyper-parameters as Python floats (the comparison with
    torch.optim in float64) instead of the descriptor's float32 values.  State: `p`, `s` = [s0, s1, s2] in trl_opt_t's
    order (None where the options keep none), `steps`; `mag`: the running magnitudes M_x of the module docstring."""

    def __init__(self, kind, params, sizes, *, alpha=0.99, eps=1e-8, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 centered=False, nesterov=False, dtype=np.float64, exact_hyper=False, states=None):
        h = (lambda x: float(x)) if exact_hyper else f32v
        self.kind, self.dtype = kind, dtype
        self.p = np.array(params, dtype=dtype)
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.alpha, self.eps, self.mu, self.damp, self.wd = h(alpha), h(eps), h(momentum), h(dampening), h(weight_decay)
        self.centered, self.nesterov = bool(centered), bool(nesterov)
        self.h = h
        n = len(self.p)
        if kind == RMSPROP:
            used = (True, self.mu != 0.0, self.centered)
        else:
            used = (self.mu != 0.0,)
        self.s = [np.zeros(n, dtype=dtype) if u_ else None for u_ in used]
        if states is not None:
            self.s = [None if (s is None or not u_) else np.array(s, dtype=dtype) for s, u_ in zip(states, used)]
        self.steps = 0
        self.mag = {"p": np.zeros(n)}
        for k, u_ in enumerate(used):
            if u_:
                self.mag["s%d" % k] = np.zeros(n)

    def clip(self, grads, max_norm, grad_scale):
        """(scaled and clipped gradient, norms) -- AdamRef's clip: norm of grads * grad_scale per group, coef = min(max_norm
        / (norm + 1e-6), 1), max_norm <= 0: coef 1 and norms 0."""
        dt, h = self.dtype, self.h
        g = np.array(grads, dtype=dt)
        gs, mn = dt(h(grad_scale)), dt(h(max_norm))
        norms, coef = np.zeros(len(self.off) - 1, dtype=dt), np.ones(g.shape, dtype=dt)
        for k in range(len(self.off) - 1):
            sl = slice(self.off[k], self.off[k + 1])
            if h(max_norm) > 0.0:
                norms[k] = np.sqrt((g[sl] * g[sl]).sum(dtype=dt) * gs * gs)
                coef[sl] = min(mn / (norms[k] + dt(1e-6)), dt(1.0))
        return g * gs * coef, norms

    def step(self, grads, lrs, max_norm=0.0, grad_scale=1.0, first=None):
        """One launch.  `first`: SGD's first-step flag (None: from the step count, which every launch advances)."""
        dt, h = self.dtype, self.h
        f = lambda x: np.abs(np.asarray(x, dtype=np.float64))
        one = dt(1.0)
        lr = np.zeros(len(self.p), dtype=dt)
        for k in range(len(self.off) - 1):
            lr[self.off[k]:self.off[k + 1]] = dt(h(lrs[k]))
        g0, norms = self.clip(grads, max_norm, grad_scale)
        p0, M = self.p, self.mag
        g = g0 + dt(self.wd) * p0 if self.wd != 0.0 else g0
        M_g = 3.0 * f(g0) + (self.wd * (2.0 * f(p0) + M["p"]) + f(g0) if self.wd != 0.0 else 0.0)
        lr64 = f(lr)
        if self.kind == RMSPROP:
            a = dt(self.alpha)
            sq_a, sq_b = a * self.s[0], (one - a) * g * g
            sq = sq_a + sq_b
            M["s0"] = self.alpha * M["s0"] + 2.0 * (1.0 - self.alpha) * f(g) * M_g + f(sq_a) + f(sq_b)
            if self.centered:
                ga0 = self.s[2]
                ga = ga0 + (g - ga0) * (one - a)
                M["s2"] = self.alpha * M["s2"] + (1.0 - self.alpha) * M_g + f(ga0) + (1.0 - self.alpha) * (f(g) + f(ga0))
                arg = sq - ga * ga
                M_arg = M["s0"] + 2.0 * f(ga) * M["s2"] + f(sq) + f(ga) ** 2
                self.s[2] = ga
            else:
                arg, M_arg = sq, M["s0"]
            root = np.sqrt(arg)
            avg = root + dt(self.eps)
            with np.errstate(divide="ignore", invalid="ignore"):
                M_avg = np.where(M_arg > 0, M_arg / (2.0 * f(root)), 0.0) + f(avg)
            q = g / avg
            M_q = M_g / f(avg) + f(q) * M_avg / f(avg) + f(q)
            self.s[0] = sq
            if self.mu != 0.0:
                b_a = dt(self.mu) * self.s[1]
                buf = b_a + q
                M["s1"] = self.mu * M["s1"] + M_q + f(b_a) + f(q)
                self.s[1] = buf
                upd, M_u = lr * buf, M["s1"]
            else:
                upd, M_u = lr * q, M_q
        else:
            if self.mu != 0.0:
                is_first = (self.steps == 0) if first is None else bool(first)
                if is_first:
                    buf = g.copy()
                    M["s0"] = M_g + np.zeros(len(g))
                else:
                    b_a, b_b = dt(self.mu) * self.s[0], (one - dt(self.damp)) * g
                    buf = b_a + b_b
                    M["s0"] = self.mu * M["s0"] + (1.0 - self.damp) * M_g + f(b_a) + f(b_b)
                self.s[0] = buf
                if self.nesterov:
                    n_b = dt(self.mu) * buf
                    s, M_s = g + n_b, M_g + self.mu * M["s0"] + f(g) + f(n_b)
                else:
                    s, M_s = buf, M["s0"]
            else:
                s, M_s = g, M_g
            upd, M_u = lr * s, M_s
        self.p = p0 - upd
        M["p"] = M["p"] + lr64 * M_u + f(upd) + np.maximum(f(p0), f(self.p))
        self.steps += 1
        return dict(norms=norms, g=g)

    def values(self):
        """{"p", "s0", ...: float64 values} of what the options store."""
        out = {"p": np.asarray(self.p, dtype=np.float64)}
        for k, s in enumerate(self.s):
            if s is not None:
                out["s%d" % k] = np.asarray(s, dtype=np.float64)
        return out


def error_ratios(got, ref):
    """{name: worst err / (u M_x)} of `got` ({"p", "s0", ...}: arrays of any float dtype, or another OptRef) against the
    float64 OptRef `ref`; an element whose magnitude is zero must be equal (inf otherwise).  Every element counts."""
    got = got.values() if isinstance(got, OptRef) else got
    want, out = ref.values(), {}
    for name, w in want.items():
        err = np.abs(np.asarray(got[name], dtype=np.float64) - w)
        b = U * ref.mag[name]
        pos = b > 0
        worst = float((err[pos] / b[pos]).max()) if pos.any() else 0.0
        out[name] = float("inf") if ((err[~pos] > 0).any() or not np.isfinite(err).all()) else worst
    return out


def pow2_at_least(x):
    return float(2.0 ** np.ceil(np.log2(max(x, 1.0))))


def polyak(target, source, tau, dtype=np.float64):
    """target <- (1 - tau) target + tau source, the kernel's order: t * (1 - tau) + s * tau."""
    t, s, tau = np.asarray(target, dtype=dtype), np.asarray(source, dtype=dtype), dtype(f32v(tau))
    return t * (dtype(1.0) - tau) + s * tau
